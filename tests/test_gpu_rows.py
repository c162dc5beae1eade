"""The row kernels of bitdance_amd/csrc/bd_rows.hip and the DiT head attention of bd_attn.hip, each launcher alone against a float64
reference of the same operation (tests/rows_ref.py), through the standalone entry points bd_ln_mod, bd_rms, bd_qkv_post,
bd_head_attn, bd_head_final, bd_swiglu_rows, bd_in_rms, bd_in_qkv_post and bd_head_y_all.  Each entry fills the launcher's argument
struct and calls the launcher the engine calls, so the launcher picks the kernel form; the case names say which form that is
(ln_mod_kernel<5|4> through "rows.ln_occ", ln_mod_rows_kernel<1|2> through wave_rows and D, the thread cap of swiglu_rows through
"rows.swiglu_t", head_attn_kernel / head_attn16_mfma_kernel<128|64> / head_attn16_kernel through P, head_dim and slabs vs a
finished tensor: rows_ref.head_attn_form).

Reference.  Plain torch in float64 on the bf16 / fp32 inputs the kernel reads, with exactly the rounding points the kernel comments
attribute to the reference model, written as .to(bfloat16).  tests/test_rows_ref_cpu.py shows without a GPU that the float32 run of
the same functions stays inside the bounds below with a quarter of the flip cap, and that the bounds reject every fault of a list
(a dropped intermediate rounding, eps x 10, swapped gate / scale / shift offsets, a dropped slab or bias, 1 + scale rounded after
the multiply, a RoPE row off by one, a flipped rotate_half, a wrong pair partner, K appended one slot off, V untransposed, the
plain column order for the interleaved SwiGLU, swapped CFG rows, tok_all one step early, a dropped key, swapped heads ...).

Bounds (U = 2^-8; u = the bf16 spacing at the reference value; gamma(n) = (n + 16) 2^-24, the worst relative error of an n-term
fp32 sum in any order).  The device differs from the reference only through its fp32 reductions ahead of a bf16 rounding:
  (a) |got - bf16(ref)| <= u + tol for every element.  tol is derived next to each output in rows_ref.py:
      - slab sums: gamma(S) sum |slab|;
      - LayerNorm / RMSNorm: the mean is off by <= gamma(D) mean|x|, rstd by gamma(D) relative, so
        tol(h) = |1 + scale| |w| (gamma(D) mean|x| rstd + 2 gamma(D) |ln|) + 4 * 2^-24 (|ln (1 + scale)| + |shift|);
      - where an earlier rounding of the same kernel feeds the output (bf16(branch) -> bf16(branch * gate) -> bf16(x + ..);
        bf16(x rstd) -> bf16(w ..); the q / k norm in front of RoPE; silu in front of the product; the Linear and the sigmoid of
        head_final) one spacing of that intermediate times the derivative is added: a flip there is rare but legitimate;
      - head_final's D -> C dot: gamma(D) sum |h w|, plus eight elements of h one spacing off.
  (b) at most 1 % of a case's elements differ from bf16(ref) at all (expected: fp32 error / bf16 spacing ~ 1e-4 .. 1e-3 per
      rounding point; a wrong rounding point, offset or index moves a large share).
  Intermediates the kernel writes back (X of ln_mod, R of rms / in_rms) are checked first and the next stage is computed from the
  device's own copy, so that one flipped element of the row is not charged to every element behind the row statistics.
  fp32 outputs (R of the fp32 streams, hidden_out) are held to tol alone.  fp8 outputs: the row scale equals amax / 448 of the
  reference row to 8 fp32 ulps (+ tol at the row maximum); the codes lie within one e4m3 step of the oracle quantiser's
  ((v / scale).to(float8_e4m3fn)) and <= 1 % of them differ.
  head_final: x_hat under (a) / (b); then x_t, pred, tok_cur and tok_all bit for bit from the device's own x_hat in torch fp32
  (sampling_x.py:77-95 op for op).  X_next is a C-term fp32 dot whose summation order torch does not reproduce: it is held to
  (a) / (b) from the device's own new x_t.
  qkv_post / in_qkv_post: (a) / (b) on q and on the appended K / V rows; every other cache element bit-identical to what the
  cache held before, in the [Lmax][128] K layout and the transposed [128][Lmax] V layout.
  Head attention, P = 64: fp32 scores, un-normalised P in bf16, fp32 accumulation, one output rounding -- test_gpu_attn's tol_llm
  with L = 64 and RMS_QW.  P <= 16: bf16 scores, bf16 P = e / sum -- tol_in and RMS_IN.  q / k / v lie on a grid and the slabs
  sum exactly in any order, so every q . k is exact in fp32 and the bf16 score is the reference's.  The probes have integer
  scores, a grade per (key, head, sequence) and one-hot V channels: output channel j spells the weight of key j.

Every output buffer is NaN (0xFF for fp8) before the call and read back whole: the rows past M of the fragment-major and
row-major outputs must still hold that.

Not covered here, each a single path without a shape-dependent form: finalize_rows, head_prologue, proj_fc1, in_proj_fc1,
embed_finalize, init_latent, step_advance (the input projection's arithmetic is reached through X_next).

Measured on an MI355X, worst case of each launcher (flip = share of elements that differ from the rounded reference, cap 1e-2;
excess = worst (|got - ref| - allowed) in bf16 spacings, reported from -1 (no element differs, or tol >= one spacing) up to 0):
  ln_mod 7.3e-5 / -0.03     rms 1.1e-4 / -0.03     qkv_post 2.0e-3 (one element of a 4-row case) / -0.002
  head_final 5.2e-4 / -0.002     swiglu_rows 8.8e-5 / -1     in_rms 6.1e-5 / -0.00001     in_qkv_post 1.6e-4 / -1
  head_y_all 9.8e-5 / -0.00001 -- no element anywhere further than one spacing from the reference.
  head_attn: relative rms 1.96e-3 at P = 64 (bound 6.4e-3) and 1.66e-3 at P <= 16 (bound 4.5e-3); worst |error| / tol 0.58.
No kernel fault was found.  Each case prints its two figures (`pytest -s`, lines "ROWSTAT").
"""
from __future__ import annotations

import contextlib
import ctypes

import pytest
import torch

from tests import rows_ref as rr
from tests.rows_ref import BF16, unfrag, unfrag8

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


def _lib():
    from bitdance_amd._lib import lib
    return lib()


def _check(rc, what):
    from bitdance_amd._lib import check
    check(rc, what)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return t.data_ptr() if t is not None else None


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def _ff(n):
    return torch.full((n,), 0xFF, dtype=torch.uint8, device=DEV)


def _state():
    return torch.full((65,), -7, dtype=torch.int32, device=DEV)


def _padded(t, rows):
    """t's rows followed by NaN rows up to `rows`."""
    out = _nan((rows,) + tuple(t.shape[1:]), t.dtype)
    out[: t.shape[0]] = t
    return out


def _untouched(t, what):
    assert torch.isnan(t).all() if t.is_floating_point() else (t == 0xFF).all(), f"{what}: written past the last row"


def _frag_rows(buf, rb, width, M, what):
    rows = unfrag(buf, rb, width)
    _untouched(rows[M:], what)
    return rows[:M]


def _frag8_rows(buf, scale, rb, width, M, what):
    rows = unfrag8(buf, rb, width)
    _untouched(rows[M:], what)
    _untouched(scale[M:], what + " scales")
    return rows[:M], scale[:M]


def _finish(rep):
    print(rep.line())
    assert not rep.fail, "\n".join(rep.fail)


@contextlib.contextmanager
def _option(name, value, default):
    """A process-wide A/B switch of the row launchers, set for one call and restored whatever happens."""
    _check(_lib().bd_set_gemm_option(name.encode(), value), name)
    try:
        yield
    finally:
        _check(_lib().bd_set_gemm_option(name.encode(), default), name)


def _params(cases):
    return [pytest.param(k, id=k) for k in cases]


# ---------------------------------------------------------------------------------------------------------------------------------
def run_ln_mod(c):
    rb = c.rows // 32
    X = _padded(c.X, c.rows)
    h = _ff(c.rows * c.D) if c.fp8 else _nan((c.rows * c.D,), BF16)
    scale = _nan((c.rows,)) if c.fp8 else None
    go, so, fo = c.offs
    with _option("rows.ln_occ", c.occ, 5):
        _check(_lib().bd_ln_mod(_p(X), _p(c.pend), _p(c.bias), c.S, c.rows, _p(c.ada), c.ada_ld, go, so, fo, _p(c.ln_w), _p(c.ln_b), _p(h),
                                _p(scale), c.M, c.D, rb, c.eps, c.wave_rows, _stream()), "bd_ln_mod")
        torch.cuda.synchronize()
    _untouched(X[c.M:], "X")
    got = dict(X=X[:c.M])
    if c.fp8:
        got["h8"], got["scale"] = _frag8_rows(h, scale, rb, c.D, c.M, "h (fp8)")
    else:
        got["h"] = _frag_rows(h, rb, c.D, c.M, "h")
    return got


@pytest.mark.parametrize("name", _params(rr.LN_CASES))
def test_ln_mod(name):
    c = rr.to_device(rr.LN_CASES[name](), DEV)
    _finish(rr.judge_ln_mod(c, run_ln_mod(c), f"ln_mod/{name}"))


def run_rms(c):
    rb = c.rows // 32
    R = _padded(c.R, c.rows)
    a = (_ff(c.rows * c.D) if c.fp8 else _nan((c.rows * c.D,), BF16)) if c.a_frag else None
    scale = _nan((c.rows,)) if c.fp8 else None
    hidden = _nan((c.M, c.D)) if c.hidden else None
    cond = _nan((c.rows * c.D,), BF16) if c.cond else None
    state = _state()
    _check(_lib().bd_rms(_p(R), _p(c.pend), _p(c.bias), c.S, c.rows, _p(c.w), _p(a), _p(scale), _p(hidden), _p(cond), _p(c.pos),
                         c.pos.shape[0] if c.cond else 0, c.step, _p(state), c.M, c.D, c.P, rb, c.eps, c.bf16_stream, _stream()), "bd_rms")
    torch.cuda.synchronize()
    assert state[0].item() == c.step and (state[1:] == 0).all()
    _untouched(R[c.M:], "R")
    got = dict(R=R[:c.M])
    if c.a_frag:
        if c.fp8:
            got["a8"], got["scale"] = _frag8_rows(a, scale, rb, c.D, c.M, "a (fp8)")
        else:
            got["a"] = _frag_rows(a, rb, c.D, c.M, "a")
    if c.hidden:
        got["hidden"] = hidden
    if c.cond:
        got["cond"] = _frag_rows(cond, rb, c.D, c.M, "cond")
    return got


@pytest.mark.parametrize("name", _params(rr.RMS_CASES))
def test_rms(name):
    c = rr.to_device(rr.RMS_CASES[name](), DEV)
    _finish(rr.judge_rms(c, run_rms(c), f"rms/{name}"))


def run_qkv_post(c):
    q = _nan((c.rows, c.nh * 128), BF16)
    K, VT = c.k0.clone(), c.v0.clone()
    state = _state()
    kv = (ctypes.c_int * c.nseq)(*c.kv)
    _check(_lib().bd_qkv_post(_p(c.qkv), _p(c.bias), c.S, c.rows, _p(c.qn), _p(c.kn), _p(c.cos), _p(c.sin), c.cos.shape[0], _p(q), _p(K), _p(VT),
                              kv, c.nseq, c.P, c.nh, c.nkv, c.Lmax, c.eps, c.rope_bf16, _p(state), _stream()), "bd_qkv_post")
    torch.cuda.synchronize()
    assert state[0].item() == 0 and state[1:1 + c.nseq].tolist() == c.kv
    _untouched(q[c.M:], "q")
    return dict(q=q[:c.M], K=K, VT=VT)


@pytest.mark.parametrize("name", _params(rr.QKV_CASES))
def test_qkv_post(name):
    c = rr.to_device(rr.QKV_CASES[name](), DEV)
    _finish(rr.judge_qkv_post(c, run_qkv_post(c), f"qkv_post/{name}"))


def run_head_attn(c):
    rb = c.rows // 32
    o = _nan((c.rows * c.D,), BF16)
    _check(_lib().bd_head_attn(_p(c.qkv), _p(c.bias), c.S, c.rows, _p(o), c.nseq, c.nhead, c.P, c.dh, rb, _stream()), "bd_head_attn")
    torch.cuda.synchronize()
    return dict(o=_frag_rows(o, rb, c.D, c.M, "o"))


@pytest.mark.parametrize("name", _params(rr.ATTN_CASES))
def test_head_attn(name):
    c = rr.to_device(rr.ATTN_CASES[name](), DEV)
    form = rr.head_attn_form(c)
    assert form == ("head_attn" if name.startswith("p64") else "head_attn16_mfma<%d>" % c.dh if "mfma" in name else "head_attn16"), form
    _finish(rr.judge_head_attn(c, run_head_attn(c), f"head_attn/{name} ({form})"))


def run_head_final(c):
    X = _padded(c.X, c.rows)
    xt = c.xt.clone()
    state = _state()
    B = c.BP // c.P if c.is_final else 1
    pred, tok_cur, tok_all = _nan((c.BP, c.C)), _nan((c.tok_branches, c.BP, c.C)), _nan((B, c.T, c.C))
    xhat = _nan((c.M, c.C))
    X_next = _nan((c.rows, c.D), BF16) if c.x_next else None
    sc = (ctypes.c_float * 7)(*c.sc.tolist())
    go, so, fo = c.offs
    table = c.cfg_table
    _check(_lib().bd_head_final(_p(X), _p(c.pend), _p(c.bias), c.S, c.rows, _p(c.ada), c.ada_ld, go, so, fo, _p(c.lin_w), _p(c.lin_b), _p(xt),
                                _p(c.noise), c.n_evals, c.step + 1, c.eval_index, c.step, _p(state), _p(pred), _p(tok_cur),
                                _p(tok_all) if c.is_final else None, c.T, c.P, _p(xhat), sc, c.is_final, c.cfg_mult, c.BP, c.D, c.C, c.eps,
                                c.sigmoid, _p(table), table.shape[0] if table is not None else 0, c.tok_branches, _p(X_next), _p(c.in_w),
                                _p(c.in_b), _stream()), "bd_head_final")
    torch.cuda.synchronize()
    assert state[0].item() == c.step
    assert torch.equal(X[:c.M], c.X) and torch.isnan(X[c.M:]).all(), "head_final wrote X"
    got = dict(xhat=xhat.cpu(), xt=xt.cpu())
    if c.is_final:
        got.update(pred=pred.cpu(), tok_cur=tok_cur.cpu(), tok_all=tok_all.cpu())
    else:
        for t in (pred, tok_cur, tok_all):
            _untouched(t, "a final-step output on a non-final step")
    if c.x_next:
        if c.is_final:
            _untouched(X_next, "X_next on the final step")
        else:
            _untouched(X_next[c.M:], "X_next")
            got["X_next"] = X_next[:c.M].cpu()
    return got


@pytest.mark.parametrize("name", _params(rr.HF_CASES))
def test_head_final(name):
    c = rr.to_device(rr.HF_CASES[name](), DEV)
    _finish(rr.judge_head_final(c, run_head_final(c), f"head_final/{name}"))


def run_swiglu(c):
    rb = c.rows // 32
    act = _nan((c.rows * c.F,), BF16)
    with _option("rows.swiglu_t", c.threads, 512):
        _check(_lib().bd_swiglu_rows(_p(c.up), _p(c.bias), c.S, c.rows, _p(act), c.M, c.F, rb, c.interleaved, _stream()), "bd_swiglu_rows")
        torch.cuda.synchronize()
    return dict(act=_frag_rows(act, rb, c.F, c.M, "act"))


@pytest.mark.parametrize("name", _params(rr.SWIGLU_CASES))
def test_swiglu_rows(name):
    c = rr.to_device(rr.SWIGLU_CASES[name](), DEV)
    _finish(rr.judge_swiglu(c, run_swiglu(c), f"swiglu_rows/{name}"))


def run_in_rms(c):
    rb = c.rows // 32
    R = _padded(c.R, c.rows)
    a = _nan((c.rows * c.D,), BF16)
    hidden = _nan((c.M, c.D)) if c.hidden else None
    cond = _nan((c.rows * c.D,), BF16) if c.cond else None
    state = _state()
    _check(_lib().bd_in_rms(_p(R), _p(c.pend), _p(c.bias), c.S, c.rows, c.init, c.renorm, _p(c.w), _p(a), _p(hidden), _p(cond), _p(c.pos),
                            c.pos.shape[0] if c.cond else 0, c.step, _p(state), c.M, c.D, c.P, rb, c.eps, c.f32_stream, _stream()), "bd_in_rms")
    torch.cuda.synchronize()
    assert state[0].item() == c.step
    _untouched(R[c.M:], "R")
    got = dict(R=R[:c.M], a=_frag_rows(a, rb, c.D, c.M, "a"))
    if c.hidden:
        got["hidden"] = hidden
    if c.cond:
        got["cond"] = _frag_rows(cond, rb, c.D, c.M, "cond")
    return got


@pytest.mark.parametrize("name", _params(rr.INRMS_CASES))
def test_in_rms(name):
    c = rr.to_device(rr.INRMS_CASES[name](), DEV)
    _finish(rr.judge_in_rms(c, run_in_rms(c), f"in_rms/{name}"))


def run_in_qkv_post(c):
    q = _nan((c.rows, c.D), BF16)
    K, V = c.k0.clone(), c.v0.clone()
    state = _state()
    _check(_lib().bd_in_qkv_post(_p(c.qkv), _p(c.bias), c.S, c.rows, _p(c.rope), c.rope.shape[0], _p(q), _p(K), _p(V), c.kv, c.nseq, c.P, c.nh,
                                 c.Lmax, _p(state), _stream()), "bd_in_qkv_post")
    torch.cuda.synchronize()
    assert state[:2].tolist() == [0, c.kv]
    _untouched(q[c.M:], "q")
    return dict(q=q[:c.M], K=K, V=V)


@pytest.mark.parametrize("name", _params(rr.INQKV_CASES))
def test_in_qkv_post(name):
    c = rr.to_device(rr.INQKV_CASES[name](), DEV)
    _finish(rr.judge_in_qkv_post(c, run_in_qkv_post(c), f"in_qkv_post/{name}"))


def run_y_all(c):
    """Group g of G evaluations is one operand matrix at element g * G * Mpad * D of y_all (fp8: the same BYTE offset of the bf16
    span), evaluation i at rows (i % G) * Mpad of it; a short last group keeps ceil(RB * left / 8) * 8 row blocks, zero-filled."""
    Mpad, D, G, n = c.rb * 32, c.D, c.G, c.n_evals
    ng = (n + G - 1) // G
    span = G * Mpad * D
    y = _ff(ng * span * 2) if c.fp8 else _nan((ng * span,), BF16)
    scale = _nan((ng * G, Mpad)) if c.fp8 else None
    _check(_lib().bd_head_y_all(_p(c.cemb), _p(c.temb), _p(y), _p(scale), c.M, D, c.rb, n, G, _stream()), "bd_head_y_all")
    torch.cuda.synchronize()
    out, sc = [], []
    for g in range(ng):
        left = min(G, n - g * G)
        short = left < G and G > 1
        rbg = ((c.rb * left + 7) & ~7) if short else c.rb * G
        if c.fp8:
            rows = unfrag8(y[g * span * 2: g * span * 2 + rbg * 32 * D], rbg, D)
        else:
            rows = unfrag(y[g * span: g * span + rbg * 32 * D], rbg, D)
        for e in range(left):
            out.append(rows[e * Mpad: e * Mpad + c.M])
            pad = rows[e * Mpad + c.M: (e + 1) * Mpad]
            if c.fp8:
                sc.append(scale[g * G + e, :c.M])
                spad = scale[g * G + e, c.M:]
            if short:                                              # the launcher zero-fills the whole short group first
                assert (pad.view(torch.int16) == 0).all() if not c.fp8 else ((pad == 0).all() and (spad == 0).all()), "short group: pad rows not zero"
            else:
                _untouched(pad, "y pad rows")
                if c.fp8:
                    _untouched(spad, "y pad scales")
        if short:
            tail = rows[left * Mpad:]
            assert (tail.view(torch.int16) == 0).all() if not c.fp8 else (tail == 0).all(), "short group: rows past its evaluations not zero"
            if c.fp8:
                assert (scale[g * G + left: (g + 1) * G] == 0).all(), "short group: scales past its evaluations not zero"
    if c.fp8:
        return dict(y8=torch.stack(out), scale=torch.stack(sc))
    return dict(y=torch.stack(out))


@pytest.mark.parametrize("name", _params(rr.YALL_CASES))
def test_head_y_all(name):
    c = rr.to_device(rr.YALL_CASES[name](), DEV)
    _finish(rr.judge_y_all(c, run_y_all(c), f"head_y_all/{name}"))


# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    """Every documented refusal returns BD_ERR_UNSUPPORTED with a text, from host validation alone: the state block and the output
    buffer of the refused calls are still what they were."""
    from bitdance_amd._lib import BD_ERR_UNSUPPORTED
    l, st = _lib(), _stream()
    state = _state()
    buf = torch.zeros(1 << 20, device=DEV)                         # every input (4 MiB)
    out = _nan((1 << 20,))                                         # every output
    b, o, s = buf.data_ptr(), out.data_ptr(), state.data_ptr()
    sc = (ctypes.c_float * 7)(0.3, 0.1, 0.7, 0.4, 0.7, 0.2, 2.0)
    kv2 = lambda *v: (ctypes.c_int * len(v))(*v)

    def ln(M=8, D=256, rb=1, ada_ld=768, offs=(0, 256, 512), S=1, rows=32, a8=None, wave=0, ln_b=b):
        return l.bd_ln_mod(o, b, None, S, rows, b, ada_ld, *offs, b, ln_b, o, a8, M, D, rb, 1e-6, wave, st)

    def rms(M=8, D=256, rb=1, S=1, rows=32, a8=None, cond=None, pos_rows=64, step=0, P=4):
        return l.bd_rms(o, b, None, S, rows, b, o, a8, None, cond, b, pos_rows, step, s, M, D, P, rb, 1e-6, 0, st)

    def qkv(nseq=2, P=4, nh=2, nkv=1, Lmax=64, kv=(0, 0), maxpos=64, rows=32, S=1):
        return l.bd_qkv_post(b, None, S, rows, b, b, b, b, maxpos, o, o, o, kv2(*kv), nseq, P, nh, nkv, Lmax, 1e-6, 0, s, st)

    def attn(nseq=1, nhead=2, P=16, dh=128, rb=1, rows=32, S=0):
        return l.bd_head_attn(b, None, S, rows, o, nseq, nhead, P, dh, rb, st)

    def hf(BP=4, D=256, C=16, cfg_mult=2, ada_ld=768, offs=(0, 256, 512), is_final=0, step=0, T=64, P=4, noise_evals=4, noise_steps=1,
           eval_index=0, table_len=0, x_next=None, in_w=None, tok_all=None, rows=32):
        return l.bd_head_final(b, b, None, 1, rows, b, ada_ld, *offs, b, b, o, b, noise_evals, noise_steps, eval_index, step, s, o, o, tok_all,
                               T, P, o, sc, is_final, cfg_mult, BP, D, C, 1e-6, 1, b if table_len else None, table_len, 1, x_next, in_w, in_w, st)

    def swi(M=8, F=256, rb=1, il=1, S=1, rows=32):
        return l.bd_swiglu_rows(b, None, S, rows, o, M, F, rb, il, st)

    def inrms(M=8, D=256, rb=1, S=1, rows=32, init=0, cond=None, pos_rows=64, step=0, P=4):
        return l.bd_in_rms(o, b if S >= 0 else None, None, S, rows, init, 0, b, o, None, cond, b, pos_rows, step, s, M, D, P, rb, 1e-6, 0, st)

    def inqkv(nseq=2, P=4, nh=2, Lmax=64, kv=0, rope_rows=64, rows=32, S=1):
        return l.bd_in_qkv_post(b, None, S, rows, b, rope_rows, o, o, o, kv, nseq, P, nh, Lmax, s, st)

    def yall(M=8, D=256, rb=1, n=3, G=1, a8=None):
        return l.bd_head_y_all(b, b, o, a8, M, D, rb, n, G, st)

    refused = [
        ln(D=260), ln(D=8200), ln(M=33), ln(M=0), ln(offs=(0, 256, 520)), ln(offs=(4, 256, 512)), ln(ada_ld=200), ln(rows=4),
        ln(ln_b=None), ln(D=288, ada_ld=3 * 288, offs=(0, 288, 576), a8=o), ln(wave=1, a8=o), ln(D=2048, ada_ld=6144, offs=(0, 2048, 4096), wave=1),
        rms(D=252), rms(M=40), rms(rows=4), rms(D=288, a8=o), rms(cond=o, pos_rows=7, step=1), rms(step=-1), rms(P=0),
        qkv(nseq=65, P=1, kv=(0,) * 65, rows=96), qkv(nseq=0), qkv(kv=(0, 61)), qkv(kv=(-1, 0)), qkv(kv=(0, 40), maxpos=43), qkv(rows=4), qkv(S=-1),
        attn(P=17), attn(P=32), attn(P=64, dh=64), attn(dh=96), attn(nseq=3), attn(nseq=2, rows=16, rb=4), attn(S=-1),
        hf(C=33), hf(C=0), hf(D=5128), hf(D=252), hf(cfg_mult=3), hf(BP=0), hf(offs=(0, 256, 516)), hf(eval_index=3), hf(step=1),
        hf(step=2, table_len=2, noise_steps=3), hf(x_next=o), hf(is_final=1, tok_all=o, step=16), hf(is_final=1, tok_all=o, BP=6, rows=32), hf(BP=32),
        swi(F=260), swi(F=264), swi(M=33), swi(rows=4), swi(S=-1),
        inrms(D=8200), inrms(M=33), inrms(S=-1, init=1), inrms(cond=o, pos_rows=3), inrms(rows=4),
        inqkv(kv=61), inqkv(kv=-1), inqkv(kv=40, rope_rows=43), inqkv(rows=4), inqkv(nh=0),
        yall(D=260), yall(M=33), yall(n=0), yall(G=0), yall(G=3), yall(D=288, a8=o),
    ]
    assert all(r == BD_ERR_UNSUPPORTED for r in refused), [i for i, r in enumerate(refused) if r != BD_ERR_UNSUPPORTED]
    assert l.bd_last_error()
    torch.cuda.synchronize()
    assert (state == -7).all() and torch.isnan(out).all(), "a refused call launched something"
    # the same helpers with their defaults run
    for rc, what in ((ln(), "ln"), (rms(), "rms"), (qkv(), "qkv"), (attn(), "attn"), (hf(), "hf"), (swi(), "swi"), (inrms(), "inrms"),
                     (inqkv(), "inqkv"), (yall(), "yall")):
        _check(rc, what)
    torch.cuda.synchronize()
