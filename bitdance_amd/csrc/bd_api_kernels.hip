// The kernels' stand-alone entry points of the C ABI (see include/bitdance_hip.h; tests/test_gpu_attn.py, tests/test_gpu_rows.py): no
// context -- host validation of the caller's shapes and buffers, then the launcher the engine's step calls (bd_api.hip).
#include <string>

#include "bd_common.h"
#include "bd_kernels.h"
#include "../../include/bitdance_hip.h"

void bdk_set_error(const std::string& m);    // bd_api.hip: the text behind bd_last_error()

static int fail(const std::string& m) { bdk_set_error(m); return -1; }
static int unsupported(const std::string& m) { bdk_set_error(m); return BD_ERR_UNSUPPORTED; }

extern "C" {

// ---- the decode attentions standalone (tests): host validation, the cache lengths into `state`, then exactly the engine's launch
static int attn_check_lengths(const int* kv_len, int nseq, int P, int Lmax, const char* who) {
    for (int i = 0; i < nseq; ++i)
        if (kv_len[i] < 0 || kv_len[i] + P > Lmax)
            return unsupported(std::string(who) + ": kv_len[" + std::to_string(i) + "] = " + std::to_string(kv_len[i]) + " outside [0, Lmax - P]");
    return 0;
}

int bd_llm_attn(const void* q, const void* k_cache, const void* vt_cache, const int* kv_len, int nseq, int P, int nh, int nkv, int Lmax,
                int splits, int causal, void* state, float* o_part, float* ml_part, void* o_frag, int row_blocks, void* stream) {
    if (nseq < 1 || nseq > BD_MAX_SEQ) return unsupported("bd_llm_attn: 1 <= nseq <= 64");
    if (P < 1 || P > 64) return unsupported("bd_llm_attn: 1 <= P <= 64");
    if (nkv < 1 || nh < nkv || nh % nkv) return unsupported("bd_llm_attn: nh a multiple of nkv");
    if ((nh / nkv) * ((P + 31) / 32) * 64 > 640) return unsupported("bd_llm_attn: G * ceil(P / 32) * 64 > 640 threads");
    if (Lmax < 64 || Lmax % 64) return unsupported("bd_llm_attn: Lmax a positive multiple of 64");
    if (splits < 1) return unsupported("bd_llm_attn: splits >= 1");
    if ((long long)row_blocks * 32 < (long long)nseq * P) return unsupported("bd_llm_attn: row_blocks * 32 < nseq * P");
    if (int r = attn_check_lengths(kv_len, nseq, P, Lmax, "bd_llm_attn")) return r;
    hipStream_t st = (hipStream_t)stream;
    BD_TRY(bdk_step_reset((BdStepState*)state, kv_len, nseq, 0, st));
    LlmAttnArgs aa;
    aa.q = q; aa.k_cache = k_cache; aa.vt_cache = vt_cache; aa.o_part = o_part; aa.ml_part = ml_part; aa.o_frag = o_frag;
    aa.state = (const BdStepState*)state;
    aa.nseq = nseq; aa.P = P; aa.nh = nh; aa.nkv = nkv; aa.Lmax = Lmax; aa.splits = splits; aa.RB = row_blocks; aa.causal = causal != 0;
    BD_TRY(bdk_llm_attn(aa, st));
    return 0;
}

int bd_in_attn(const void* q, const void* k_cache, const void* v_cache, int kv_len, int nseq, int P, int nh, int Lmax, int causal,
               void* state, void* o_frag, int row_blocks, void* stream) {
    if (nseq < 1 || nh < 1) return unsupported("bd_in_attn: nseq, nh >= 1");
    if (Lmax < 64 || Lmax % 64) return unsupported("bd_in_attn: Lmax a positive multiple of 64");
    if ((long long)row_blocks * 32 < (long long)nseq * P) return unsupported("bd_in_attn: row_blocks * 32 < nseq * P");
    if (int r = attn_check_lengths(&kv_len, 1, P, Lmax, "bd_in_attn")) return r;
    const int form = bdk_in_attn_form(P, Lmax);
    if (form == -2) return unsupported("bd_in_attn: 1 <= P <= 16");
    if (form < 0) return unsupported("bd_in_attn: Lmax too long for the score rows of the form P takes (LDS)");
    hipStream_t st = (hipStream_t)stream;
    BD_TRY(bdk_step_reset((BdStepState*)state, &kv_len, 1, 0, st));
    InAttnArgs aa{q, (const bf16_t*)k_cache, (const bf16_t*)v_cache, o_frag, (const BdStepState*)state, nseq, P, nh, Lmax, row_blocks};
    aa.causal = causal != 0;
    BD_TRY(bdk_in_attn(aa, st));
    return 0;
}

// ---- the row kernels and the DiT head attention standalone (tests): host validation, the step state into `state` where the kernel
// reads one, then the launcher the engine calls -- which picks the kernel form -- on the caller's buffers
static const int kMaxRowD = 1024 * 8;   // one thread per 8 channels, at most 1024 threads (row_threads, bd_rowhelp.h)
static int rows_fill_partial(Partial* q, const void* p, const void* bias, int S, int rows, int N, int M, const char* who, bool required) {
    q->p = nullptr; q->bias = nullptr; q->S = 0; q->N = N; q->Mpad = rows;
    if (S < 0) {
        if (required) return unsupported(std::string(who) + ": the Linear output is required (S >= 0)");
        return 0;
    }
    if (!p) return unsupported(std::string(who) + ": S >= 0 without a Linear output");
    if (rows < M) return unsupported(std::string(who) + ": the Linear output has fewer rows than M");
    if (S == 0 && bias) return unsupported(std::string(who) + ": a finished bf16 tensor (S = 0) already holds its bias");
    q->p = (const float*)p; q->bias = bias; q->S = S;
    return 0;
}
static int rows_check_width(int M, int D, int row_blocks, int max_d, const char* who) {
    if (M < 1) return unsupported(std::string(who) + ": M >= 1");
    if (D < 8 || D % 8 || D > max_d) return unsupported(std::string(who) + ": D a multiple of 8, at most " + std::to_string(max_d));
    if ((long long)row_blocks * 32 < (long long)M) return unsupported(std::string(who) + ": row_blocks * 32 < M");
    return 0;
}
static int rows_check_ada(int ada_ld, int D, const int* offs, int n, const char* who) {
    if (ada_ld < D || ada_ld % 8) return unsupported(std::string(who) + ": ada_ld a multiple of 8, at least D");
    for (int i = 0; i < n; ++i)
        if (offs[i] < 0 || offs[i] % 8 || offs[i] + D > ada_ld)
            return unsupported(std::string(who) + ": gate / scale / shift offsets multiples of 8 inside [0, ada_ld - D]");
    return 0;
}
static int rows_check_pos(const void* cond_frag, const float* pos, int pos_rows, int step, int P, const char* who) {
    if (step < 0) return unsupported(std::string(who) + ": step >= 0");
    if (P < 1) return unsupported(std::string(who) + ": P >= 1");
    if (cond_frag && (!pos || (long long)(step + 1) * P > pos_rows))
        return unsupported(std::string(who) + ": cond_frag needs a position table of at least (step + 1) * P rows");
    return 0;
}

int bd_ln_mod(void* X, const void* pend, const void* pend_bias, int pend_S, int pend_rows, const void* ada, int ada_ld, int gate_off,
              int scale_off, int shift_off, const float* ln_w, const float* ln_b, void* h_frag, float* a8_scale, int M, int D,
              int row_blocks, float eps, int wave_rows, void* stream) {
    if (int r = rows_check_width(M, D, row_blocks, kMaxRowD, "bd_ln_mod")) return r;
    if (!X || !ada || !h_frag) return unsupported("bd_ln_mod: X, ada and h_frag are required");
    const int offs[3] = {gate_off, scale_off, shift_off};
    if (int r = rows_check_ada(ada_ld, D, offs, 3, "bd_ln_mod")) return r;
    if ((ln_w == nullptr) != (ln_b == nullptr)) return unsupported("bd_ln_mod: LayerNorm weight and bias come together");
    if (a8_scale && D % 64) return unsupported("bd_ln_mod: the fp8 operand needs D a multiple of 64");
    if (wave_rows && (a8_scale || D > 1024)) return unsupported("bd_ln_mod: wave_rows is the bf16 form for D <= 1024");
    LnModArgs a{};
    if (int r = rows_fill_partial(&a.pend, pend, pend_bias, pend_S, pend_rows, D, M, "bd_ln_mod", false)) return r;
    a.X = X; a.ada = ada; a.ada_ld = ada_ld; a.gate_off = gate_off; a.scale_off = scale_off; a.shift_off = shift_off;
    a.ln_w = ln_w; a.ln_b = ln_b; a.h_frag = h_frag; a.M = M; a.D = D; a.RB = row_blocks; a.eps = eps; a.a8_scale = a8_scale;
    a.wave_rows = wave_rows != 0;
    BD_TRY(bdk_ln_mod(a, (hipStream_t)stream));
    return 0;
}

int bd_rms(float* R, const void* pend, const void* pend_bias, int pend_S, int pend_rows, const void* w, void* a_frag, float* a8_scale,
           float* hidden_out, void* cond_frag, const float* pos, int pos_rows, int step, void* state, int M, int D, int P, int row_blocks,
           float eps, int bf16_stream, void* stream) {
    if (int r = rows_check_width(M, D, row_blocks, kMaxRowD, "bd_rms")) return r;
    if (!R || !w || !state) return unsupported("bd_rms: R, w and state are required");
    if (a8_scale && (!a_frag || D % 64)) return unsupported("bd_rms: the fp8 operand needs a_frag and D a multiple of 64");
    if (int r = rows_check_pos(cond_frag, pos, pos_rows, step, P, "bd_rms")) return r;
    RmsArgs a{};
    if (int r = rows_fill_partial(&a.pend, pend, pend_bias, pend_S, pend_rows, D, M, "bd_rms", false)) return r;
    hipStream_t st = (hipStream_t)stream;
    BD_TRY(bdk_step_reset((BdStepState*)state, nullptr, 0, step, st));
    a.R = R; a.w = w; a.a_frag = a_frag; a.hidden_out = hidden_out; a.cond_frag = cond_frag; a.pos = pos;
    a.state = (const BdStepState*)state; a.M = M; a.D = D; a.RB = row_blocks; a.P = P; a.eps = eps; a.a8_scale = a8_scale;
    a.bf16_stream = bf16_stream != 0;
    BD_TRY(bdk_rms(a, st));
    return 0;
}

int bd_qkv_post(const void* qkv, const void* qkv_bias, int qkv_S, int qkv_rows, const void* qn_w, const void* kn_w, const float* cos,
                const float* sin, int maxpos, void* q_out, void* k_cache, void* vt_cache, const int* kv_len, int nseq, int P, int nh,
                int nkv, int Lmax, float eps, int rope_bf16, void* state, void* stream) {
    if (nseq < 1 || nseq > BD_MAX_SEQ) return unsupported("bd_qkv_post: 1 <= nseq <= 64");
    if (P < 1 || nh < 1 || nkv < 1 || Lmax < 1) return unsupported("bd_qkv_post: P, nh, nkv, Lmax >= 1");
    if (!qn_w || !kn_w || !cos || !sin || !q_out || !k_cache || !vt_cache || !state || !kv_len)
        return unsupported("bd_qkv_post: null pointer");
    if (int r = attn_check_lengths(kv_len, nseq, P, Lmax, "bd_qkv_post")) return r;
    for (int i = 0; i < nseq; ++i)
        if (kv_len[i] + P > maxpos) return unsupported("bd_qkv_post: kv_len + P past the RoPE table");
    QkvPostArgs a{};
    if (int r = rows_fill_partial(&a.qkv, qkv, qkv_bias, qkv_S, qkv_rows, (nh + 2 * nkv) * 128, nseq * P, "bd_qkv_post", true)) return r;
    hipStream_t st = (hipStream_t)stream;
    BD_TRY(bdk_step_reset((BdStepState*)state, kv_len, nseq, 0, st));
    a.qn_w = qn_w; a.kn_w = kn_w; a.cos = cos; a.sin = sin; a.q_out = q_out; a.k_cache = k_cache; a.vt_cache = vt_cache;
    a.state = (const BdStepState*)state; a.M = nseq * P; a.P = P; a.nh = nh; a.nkv = nkv; a.Lmax = Lmax; a.eps = eps;
    a.rope_bf16 = rope_bf16 != 0;
    BD_TRY(bdk_qkv_post(a, st));
    return 0;
}

int bd_head_attn(const void* qkv, const void* qkv_bias, int qkv_S, int qkv_rows, void* o_frag, int nseq, int nhead, int P, int dh,
                 int row_blocks, void* stream) {
    if (nseq < 1 || nhead < 1) return unsupported("bd_head_attn: nseq, nhead >= 1");
    if (!(P == 64 || (P >= 1 && P <= 16))) return unsupported("bd_head_attn: P = 64 or 1 <= P <= 16");
    if (dh != 128 && !(dh == 64 && P <= 16)) return unsupported("bd_head_attn: head_dim 128, or 64 with P <= 16");
    if (!o_frag) return unsupported("bd_head_attn: o_frag is required");
    if ((long long)row_blocks * 32 < (long long)nseq * P) return unsupported("bd_head_attn: row_blocks * 32 < nseq * P");
    HeadAttnArgs a{};
    if (int r = rows_fill_partial(&a.qkv, qkv, qkv_bias, qkv_S, qkv_rows, 3 * nhead * dh, nseq * P, "bd_head_attn", true)) return r;
    a.o_frag = o_frag; a.nseq = nseq; a.nhead = nhead; a.D = nhead * dh; a.RB = row_blocks; a.P = P; a.dh = dh;
    BD_TRY(bdk_head_attn(a, (hipStream_t)stream));
    return 0;
}

int bd_head_final(const void* X, const void* pend, const void* pend_bias, int pend_S, int pend_rows, const void* ada, int ada_ld,
                  int gate_off, int scale_off, int shift_off, const void* lin_w, const void* lin_b, float* xt, const float* noise,
                  int noise_evals, int noise_steps, int eval_index, int step, void* state, float* pred_out, float* tok_cur, float* tok_all,
                  int T, int P, float* xhat_out, const float* scalars7, int is_final, int cfg_mult, int BP, int D, int C, float eps_ln,
                  int sigmoid, const float* cfg_table, int cfg_table_len, int tok_branches, void* X_next, const void* in_w, const void* in_b,
                  void* stream) {
    if (cfg_mult != 1 && cfg_mult != 2) return unsupported("bd_head_final: cfg_mult 1 or 2");
    if (BP < 1) return unsupported("bd_head_final: BP >= 1");
    if (D < 8 || D % 8 || D > 640 * 8) return unsupported("bd_head_final: D a multiple of 8, at most 5120");
    if (C < 1 || C > 32) return unsupported("bd_head_final: 1 <= C <= 32");
    if (!X || !ada || !lin_w || !lin_b || !xt || !state || !scalars7) return unsupported("bd_head_final: null pointer");
    const int offs[3] = {gate_off, scale_off, shift_off};
    if (int r = rows_check_ada(ada_ld, D, offs, 3, "bd_head_final")) return r;
    if (step < 0 || P < 1) return unsupported("bd_head_final: step >= 0, P >= 1");
    if (is_final) {
        if (tok_branches < 1) return unsupported("bd_head_final: tok_branches >= 1");
        if (tok_all && (BP % P || (long long)(step + 1) * P > T)) return unsupported("bd_head_final: tok_all needs BP a multiple of P and (step + 1) * P <= T");
    } else {
        if (!noise || step >= noise_steps || eval_index < 0 || eval_index + 1 >= noise_evals)
            return unsupported("bd_head_final: a non-final step reads noise[step][eval_index + 1] inside [noise_steps][noise_evals]");
        if (X_next && (!in_w || !in_b)) return unsupported("bd_head_final: X_next needs the input projection");
    }
    if (cfg_table && step >= cfg_table_len) return unsupported("bd_head_final: step past the guidance table");
    HeadFinalArgs a{};
    if (int r = rows_fill_partial(&a.pend, pend, pend_bias, pend_S, pend_rows, D, cfg_mult * BP, "bd_head_final", false)) return r;
    hipStream_t st = (hipStream_t)stream;
    BD_TRY(bdk_step_reset((BdStepState*)state, nullptr, 0, step, st));
    a.X = X; a.ada = ada; a.ada_ld = ada_ld; a.gate_off = gate_off; a.scale_off = scale_off; a.shift_off = shift_off;
    a.lin_w = lin_w; a.lin_b = lin_b; a.xt = xt; a.noise = noise; a.noise_step_stride = (long long)noise_evals * BP * C;
    a.eval_index = eval_index; a.state = (const BdStepState*)state; a.pred_out = pred_out; a.tok_cur = tok_cur; a.tok_all = tok_all;
    a.T = T; a.P = P; a.xhat_out = xhat_out;
    a.sc.t = scalars7[0]; a.sc.dt = scalars7[1]; a.sc.den = scalars7[2]; a.sc.var = scalars7[3]; a.sc.omt = scalars7[4];
    a.sc.noise_scale = scalars7[5]; a.sc.cfg = scalars7[6]; a.sc.is_final = is_final != 0; a.sc.cfg_mult = cfg_mult;
    a.BP = BP; a.D = D; a.C = C; a.M = cfg_mult * BP; a.eps_ln = eps_ln; a.sigmoid = sigmoid != 0; a.cfg_table = cfg_table;
    a.tok_branches = tok_branches; a.X_next = X_next; a.in_w = in_w; a.in_b = in_b;
    BD_TRY(bdk_head_final(a, st));
    return 0;
}

int bd_swiglu_rows(const void* up, const void* up_bias, int up_S, int up_rows, void* act_frag, int M, int F, int row_blocks,
                   int interleaved, void* stream) {
    if (M < 1) return unsupported("bd_swiglu_rows: M >= 1");
    if (F < 8 || F % 8 || (interleaved && F % 16)) return unsupported("bd_swiglu_rows: F a multiple of 8 (16 for the interleaved column order)");
    if ((long long)row_blocks * 32 < (long long)M) return unsupported("bd_swiglu_rows: row_blocks * 32 < M");
    if (!act_frag) return unsupported("bd_swiglu_rows: act_frag is required");
    SwigluArgs a{};
    if (int r = rows_fill_partial(&a.up, up, up_bias, up_S, up_rows, 2 * F, M, "bd_swiglu_rows", true)) return r;
    a.act_frag = act_frag; a.M = M; a.F = F; a.RB = row_blocks; a.interleaved = interleaved != 0;
    BD_TRY(bdk_swiglu_rows(a, (hipStream_t)stream));
    return 0;
}

int bd_in_rms(float* R, const void* pend, const void* pend_bias, int pend_S, int pend_rows, int init_from_pend, int renorm_to_R,
              const float* w, void* a_frag, float* hidden_out, void* cond_frag, const float* pos, int pos_rows, int step, void* state,
              int M, int D, int P, int row_blocks, float eps, int f32_stream, void* stream) {
    if (int r = rows_check_width(M, D, row_blocks, kMaxRowD, "bd_in_rms")) return r;
    if (!R || !w || !state) return unsupported("bd_in_rms: R, w and state are required");
    if (int r = rows_check_pos(cond_frag, pos, pos_rows, step, P, "bd_in_rms")) return r;
    InRmsArgs a{};
    if (int r = rows_fill_partial(&a.pend, pend, pend_bias, pend_S, pend_rows, D, M, "bd_in_rms", init_from_pend != 0)) return r;
    hipStream_t st = (hipStream_t)stream;
    BD_TRY(bdk_step_reset((BdStepState*)state, nullptr, 0, step, st));
    a.R = R; a.init_from_pend = init_from_pend != 0; a.renorm_to_R = renorm_to_R != 0; a.w = w; a.a_frag = a_frag;
    a.hidden_out = hidden_out; a.cond_frag = cond_frag; a.pos = pos; a.state = (const BdStepState*)state;
    a.M = M; a.D = D; a.RB = row_blocks; a.P = P; a.eps = eps; a.f32_stream = f32_stream != 0;
    BD_TRY(bdk_in_rms(a, st));
    return 0;
}

int bd_in_qkv_post(const void* qkv, const void* qkv_bias, int qkv_S, int qkv_rows, const float* rope, int rope_rows, void* q_out,
                   void* k_cache, void* v_cache, int kv_len, int nseq, int P, int nh, int Lmax, void* state, void* stream) {
    if (nseq < 1 || P < 1 || nh < 1 || Lmax < 1) return unsupported("bd_in_qkv_post: nseq, P, nh, Lmax >= 1");
    if (!rope || !q_out || !k_cache || !v_cache || !state) return unsupported("bd_in_qkv_post: null pointer");
    if (int r = attn_check_lengths(&kv_len, 1, P, Lmax, "bd_in_qkv_post")) return r;
    if (kv_len + P > rope_rows) return unsupported("bd_in_qkv_post: kv_len + P past the RoPE table");
    InQkvPostArgs a{};
    if (int r = rows_fill_partial(&a.qkv, qkv, qkv_bias, qkv_S, qkv_rows, 3 * nh * 64, nseq * P, "bd_in_qkv_post", true)) return r;
    hipStream_t st = (hipStream_t)stream;
    BD_TRY(bdk_step_reset((BdStepState*)state, &kv_len, 1, 0, st));
    a.rope = rope; a.q_out = q_out; a.k_cache = (bf16_t*)k_cache; a.v_cache = (bf16_t*)v_cache; a.state = (const BdStepState*)state;
    a.M = nseq * P; a.P = P; a.nh = nh; a.Lmax = Lmax;
    BD_TRY(bdk_in_qkv_post(a, st));
    return 0;
}

int bd_head_y_all(const void* cemb, const void* temb, void* y_all, float* a8_scale, int M, int D, int row_blocks, int n_evals, int G,
                  void* stream) {
    if (int r = rows_check_width(M, D, row_blocks, kMaxRowD, "bd_head_y_all")) return r;
    if (!cemb || !temb || !y_all) return unsupported("bd_head_y_all: null pointer");
    if (n_evals < 1 || n_evals > 65535) return unsupported("bd_head_y_all: 1 <= n_evals <= 65535");
    if (G < 1 || (G > 1 && (row_blocks * G) % 8)) return unsupported("bd_head_y_all: G >= 1, and row_blocks * G a multiple of 8 when G > 1");
    if (a8_scale && D % 64) return unsupported("bd_head_y_all: the fp8 operand needs D a multiple of 64");
    HeadYAllArgs a{cemb, temb, y_all, M, D, row_blocks, row_blocks * 32, n_evals, G};
    a.a8_scale = a8_scale;
    BD_TRY(bdk_head_y_all(a, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
