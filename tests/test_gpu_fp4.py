"""MXFP4 weights x fp8 activations (``weights="fp4a"``, ``wdtype`` 3; csrc/bd_gemm4.hip, bd_gemm_kernel.h WT = 3) through the C ABI.

  1. operand-mapping probes: one-hot activations make every output one exactly representable term, so the fp64 product must come
     back EXACTLY -- nibble order, low / high nibble, which lane's exponent byte scales which 32 k, and which byte of an exponent
     dword belongs to which 64-deep stage (also from a K slice that does not start at a multiple of four stages);
  2. random data against the exact product of the two quantised operands (both exact in fp64: only the fp32 summation order
     differs, so the bounds of test_gpu_fp8.py::test_gemm_fp8_weights_and_activations carry over);
  3. head evaluation / LLM step at true width against the oracle under a policy defined HERE (MXFP4 weights by this file's own
     restatement of the quantiser, e4m3 rows as the oracle's "fp8wa"), and the distance to the bf16 flow relative to fp8a's;
  4. the tiny pipeline; 5. what the mode refuses.

e2m1 has 15 values, so a fixed arithmetic pattern of codes repeats inside a block of 32; the probes therefore draw codes and exponents
from a seeded generator: every (row, k) position differs from any other in most of the >= 64 rows, and any swap of two positions shows."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
E4M3_ONE = 0x38                                              # sign 0, exponent field 7 (bias 7), mantissa 0


def dequant(codes, exps):
    """fp64 values of e2m1 codes [N, K] (bit 3 = sign) with E8M0 exponents [N, K / 32]."""
    grid = torch.tensor(GRID, dtype=torch.float64, device=codes.device)
    v = grid[(codes & 7).long()] * torch.where((codes & 8) != 0, -1.0, 1.0).double()
    return v * torch.exp2(exps.double() - 127.0).repeat_interleave(32, dim=1)


def restated_quant(w):
    """This file's own MXFP4 quantiser (engine.quantize_rows_mxfp4 reads exponent fields and rounds with torch.round; this one takes
    the exponent from frexp and searches the value table, ties to the even code).  w: bf16-representable [N, K] -> (codes, exps)."""
    N, K = w.shape
    codes = torch.empty(N, K, dtype=torch.uint8, device=w.device)
    exps = torch.empty(N, K // 32, dtype=torch.uint8, device=w.device)
    grid = torch.tensor(GRID, dtype=torch.float64, device=w.device)
    odd = (torch.arange(8, device=w.device) & 1).double() * 2.0 ** -30       # a tie goes to the even code (distances are multiples of 2^-11 and more)
    for r0 in range(0, N, 2048):
        blk = w[r0:r0 + 2048].double().view(-1, K // 32, 32)
        amax = blk.abs().amax(dim=2)
        _, ex = torch.frexp(amax)                            # amax = m 2^ex, m in [0.5, 1)
        e = torch.where(amax == 0, torch.full_like(ex, -127), ex - 3).clamp(-127, 127)
        a = blk.abs() * torch.exp2(-e.double())[:, :, None]
        c = ((a[..., None] - grid).abs() + odd).argmin(dim=-1).to(torch.uint8)
        codes[r0:r0 + 2048] = (c | (torch.signbit(blk).to(torch.uint8) << 3)).view(-1, K)
        exps[r0:r0 + 2048] = (e + 127).to(torch.uint8)
    return codes, exps


def a8_layout(rows_u8, rb):
    """e4m3 bytes [rb * 32, K] row-major -> the A8 operand layout [stage of 64][row block][half][lane = row % 32 + 32 (k / 32 % 2)][16 B]
    (what test_gpu_fp8.py::test_gemm_fp8_weights_and_activations reads back from bd_quant_rows8)."""
    K = rows_u8.shape[1]
    return rows_u8.view(rb, 32, K // 64, 2, 2, 16).permute(2, 0, 4, 3, 1, 5).contiguous().view(-1)


def pack4(codes, exps, swiglu_up=None):
    from bitdance_amd import engine as E
    from bitdance_amd._lib import check, lib
    N, K = codes.shape
    st = torch.cuda.current_stream().cuda_stream
    nib = E.mxfp4_nibbles(codes)
    if swiglu_up is None:
        wp = torch.zeros(N * K // 2, dtype=torch.uint8, device=DEV)
        ep = torch.zeros(E.mxfp4_exp_bytes(N, K), dtype=torch.uint8, device=DEV)
        check(lib().bd_pack_weight4k(wp.data_ptr(), ep.data_ptr(), nib.data_ptr(), exps.contiguous().data_ptr(), N, K, 0, N, st), "bd_pack_weight4k")
    else:
        cu, eu = swiglu_up
        nu = E.mxfp4_nibbles(cu)
        wp = torch.zeros(N * K, dtype=torch.uint8, device=DEV)
        ep = torch.zeros(E.mxfp4_exp_bytes(2 * N, K), dtype=torch.uint8, device=DEV)
        check(lib().bd_pack_weight4k_swiglu(wp.data_ptr(), ep.data_ptr(), nib.data_ptr(), exps.contiguous().data_ptr(), nu.data_ptr(),
                                            eu.contiguous().data_ptr(), N, K, st), "bd_pack_weight4k_swiglu")
    torch.cuda.synchronize()
    return wp, ep


def gemm4(a8, asc, rb, wp, ep, N, K, S, nw, epi, bias=None):
    from bitdance_amd._lib import check, lib
    st = torch.cuda.current_stream().cuda_stream
    scratch = torch.zeros(max(S, 1), rb * 32, N, device=DEV)
    cnt = torch.zeros(16384, dtype=torch.int32, device=DEV)
    if epi == 0:
        out = scratch
    elif epi == 2:
        out = torch.zeros(rb * 32, N, dtype=torch.bfloat16, device=DEV)
    else:
        out = torch.zeros(rb * 32, N, device=DEV)
    check(lib().bd_gemm_w4a8(a8.data_ptr(), asc.data_ptr(), rb, wp.data_ptr(), ep.data_ptr(), bias.data_ptr() if bias is not None else None,
                             N, K, S, nw + 32, epi, scratch.data_ptr(), cnt.data_ptr(), out.data_ptr(), st), "bd_gemm_w4a8")
    torch.cuda.synchronize()
    assert int(cnt.abs().sum()) == 0                         # the in-launch reduction leaves its tickets re-armed
    return out


# ------------------------------------------------------------------------------------------------ 1. operand-mapping probes
@pytest.mark.parametrize("M,N,K,S,nw,epi,swiglu", [
    (64, 64, 64, 1, 2, 0, False),                 # one stage
    (128, 128, 320, 1, 4, 0, False),              # 5 stages: the last exponent dword is partly filled
    (128, 256, 832, 2, 8, 3, False),              # 13 stages in slices of 7 + 6: the second slice starts at byte 3 of a dword
    (128, 128, 1024, 3, 4 + 256, 3, False),       # two K parts per workgroup (stages alternate between the waves), 3 slices reduced in the launch
    (128, 128, 1024, 3, 4 + 256, 0, False),       # ... and as fp32 slabs
    (32, 256, 576, 1, 8, 0, False),               # 32 rows on an 8-wave workgroup: the threads past the A stage (bd_gemm_kernel.h DUP)
    (128, 256, 320, 1, 4, 0, True),               # SwiGLU packing: 16 gate rows, then the 16 matching up rows per panel
    (256, 128, 640, 1, 4, 2, False),              # the 256-row pass (bf16 epilogue; every value here is a bf16 value)
])
def test_operand_mapping_probes(M, N, K, S, nw, epi, swiglu):
    """Activation row i is 1.0 at k = k0 + i and 0 elsewhere (row scale exactly 1: the A8 bytes are written here, bd_quant_rows8
    would scale the row to 448 and bring in an inexact 1 / 448), so out[i, n] = W[n, k0 + i] with no rounding anywhere; k0 steps
    through K until every k was hot once."""
    from bitdance_amd import engine as E
    g = torch.Generator(device=DEV).manual_seed(N * 7 + K)
    codes = torch.randint(0, 16, (N, K), device=DEV, generator=g, dtype=torch.uint8)
    # exponents 2^-7 .. 2^6 (products exact in bf16 and fp32), parity = parity of row + block: (row, block) neighbours always differ
    exps = 120 + 2 * torch.randint(0, 7, (N, K // 32), device=DEV, generator=g, dtype=torch.uint8)
    exps = exps + ((torch.arange(N, device=DEV)[:, None] + torch.arange(K // 32, device=DEV)[None, :]) & 1).to(torch.uint8)
    W = dequant(codes, exps)                                  # [N, K] fp64, the row order of the source tensors
    if swiglu:
        F_ = N // 2
        wp, ep = pack4(codes[:F_], exps[:F_], swiglu_up=(codes[F_:], exps[F_:]))
        order = torch.stack([torch.arange(F_, device=DEV).view(-1, 16), F_ + torch.arange(F_, device=DEV).view(-1, 16)], dim=1).reshape(-1)
        W = W[order]                                          # packed row order: the raw accumulators come out in it
    else:
        wp, ep = pack4(codes, exps)
        assert ep.numel() == N // 32 * ((K // 64 + 3) // 4) * 256 and wp.numel() == N * K // 2
    rb = E.row_blocks(M)
    asc = torch.ones(rb * 32, dtype=torch.float32, device=DEV)
    seen = torch.zeros(K, dtype=torch.bool)
    for k0 in range(0, K, M):
        rows = min(M, K - k0)
        x = torch.zeros(rb * 32, K, dtype=torch.uint8, device=DEV)
        x[torch.arange(rows, device=DEV), k0 + torch.arange(rows, device=DEV)] = E4M3_ONE
        out = gemm4(a8_layout(x, rb), asc, rb, wp, ep, N, K, S, nw, epi)
        got = (out.sum(0) if epi == 0 else out)[:rows].double()
        want = W[:, k0:k0 + rows].t()
        if not torch.equal(got, want):
            bad = (got != want).nonzero()
            i, n = (int(v) for v in bad[0])
            where = (W[n] == got[i, n]).nonzero().flatten().tolist()[:8]
            pytest.fail(f"{len(bad)} of {got.numel()} outputs differ; first: activation row {i} (k = {k0 + i}), column {n}: got {got[i, n].item()} "
                        f"want {want[i, n].item()}; that column holds the value got at k = {where}")
        seen[k0:k0 + rows] = True
    assert bool(seen.all())


# ------------------------------------------------------------------------------------------------ 2. random data
@pytest.mark.parametrize("M,N,K,S,nw,epi", [
    (128, 256, 256, 1, 4, 0), (128, 15360, 5120, 2, 4, 2), (128, 71680, 1024, 1, 8, 2), (128, 7168, 5120, 4, 8 + 256, 0),
    (32, 5120, 5120, 4, 4, 0), (64, 1024, 512, 2, 2, 2), (256, 5120, 5120, 1, 4, 2)])
def test_gemm_fp4_weights_fp8_activations(M, N, K, S, nw, epi):
    """bd_gemm_w4a8 == the exact product of the two quantised operands x the activation row scale (no per-channel factor)."""
    from bitdance_amd import engine as E
    from bitdance_amd._lib import check, lib
    g = torch.Generator(device=DEV).manual_seed(M + N + K + 1)
    x = torch.randn(M, K, device=DEV, generator=g) * (1 + torch.rand(M, 1, device=DEV, generator=g) * 3)
    w = (torch.randn(N, K, device=DEV, generator=g) / K ** 0.5 * (1 + torch.rand(N, 1, device=DEV, generator=g))).to(torch.bfloat16)
    b = (torch.randn(N, device=DEV, generator=g) * 0.1).to(torch.bfloat16)
    rb = E.row_blocks(M)
    st = torch.cuda.current_stream().cuda_stream
    a8 = torch.zeros(rb * 32 * K, dtype=torch.uint8, device=DEV)
    asc = torch.zeros(rb * 32, dtype=torch.float32, device=DEV)
    check(lib().bd_quant_rows8(a8.data_ptr(), asc.data_ptr(), x.contiguous().data_ptr(), M, K, rb, st), "bd_quant_rows8")
    am = x.abs().amax(dim=1, keepdim=True)
    xq = (x * (448.0 / am)).to(torch.float8_e4m3fn)
    codes, exps = E.quantize_rows_mxfp4(w)
    c2, e2 = restated_quant(w.float())
    assert torch.equal(codes, c2) and torch.equal(exps, e2)   # the engine's quantiser == this file's restatement, on the device
    wp, ep = E.pack_linear_fp4([w], DEV)
    ref = (xq.double() @ dequant(codes, exps).t()) * asc[:M, None].double()
    out = gemm4(a8, asc, rb, wp, ep, N, K, S, nw, epi, bias=b if epi == 2 else None)
    if epi == 0:
        got = out.sum(0)[:M].double() if S > 1 else out[0, :M].double()
        err, bound = (got - ref).abs().max().item(), 3e-5 * K ** 0.5 * max(1.0, ref.abs().max().item()) + 1e-5
        print(f"[fp4a gemm {M}x{N}x{K} S{S}] max err {err:.3g} (bound {bound:.3g})")
        assert err <= bound
    else:
        want = (ref + b.double()).float()
        d = (out[:M].float() - want).abs()
        off = (out[:M] != want.to(torch.bfloat16)).float().mean().item()
        print(f"[fp4a gemm {M}x{N}x{K} S{S} bf16] max err {d.max().item():.3g}, off the correctly rounded bf16: {off:.5f}")
        assert d.max().item() <= 0.04 * max(1.0, want.abs().max().item())
        assert off <= 0.02


def test_swiglu_fp4_epilogue():
    """The fused SwiGLU epilogue over two K slices at the head's w1 shape: bounds of test_gpu_fp8.py::test_swiglu_fp8_epilogue (h rounded
    once to bf16, then silu(gate) * up in fp32, rounded once more: at most 2 % of the elements off a torch restatement, by <= 0.07)."""
    from bitdance_amd import engine as E
    from bitdance_amd._lib import check, lib
    M, F_, K = 128, 7680, 5120
    g = torch.Generator(device=DEV).manual_seed(13)
    x = torch.randn(M, K, device=DEV, generator=g)
    w = (torch.randn(2 * F_, K, device=DEV, generator=g) / K ** 0.5).to(torch.bfloat16)
    b = (torch.randn(2 * F_, device=DEV, generator=g) * 0.1).to(torch.bfloat16)
    rb = 4
    st = torch.cuda.current_stream().cuda_stream
    a8 = torch.zeros(rb * 32 * K, dtype=torch.uint8, device=DEV)
    asc = torch.zeros(rb * 32, dtype=torch.float32, device=DEV)
    check(lib().bd_quant_rows8(a8.data_ptr(), asc.data_ptr(), x.contiguous().data_ptr(), M, K, rb, st), "bd_quant_rows8")
    xq = (x * (448.0 / x.abs().amax(dim=1, keepdim=True))).to(torch.float8_e4m3fn)
    wp, ep = E.pack_swiglu_fp4(w[:F_], w[F_:], DEV)
    bp = E.pack_swiglu_bias(b[:F_], b[F_:], DEV)
    act = torch.zeros(rb * 32 * F_, dtype=torch.bfloat16, device=DEV)
    scratch = torch.zeros(2, rb * 32, 2 * F_, device=DEV)
    cnt = torch.zeros(16384, dtype=torch.int32, device=DEV)
    check(lib().bd_gemm_w4a8(a8.data_ptr(), asc.data_ptr(), rb, wp.data_ptr(), ep.data_ptr(), bp.data_ptr(), 2 * F_, K, 2, 4 + 32, 1,
                             scratch.data_ptr(), cnt.data_ptr(), act.data_ptr(), st), "bd_gemm_w4a8")
    torch.cuda.synchronize()
    c, e = restated_quant(w.float())
    h = ((xq.double() @ dequant(c, e).t()) * asc[:M, None].double() + b.double()).float().to(torch.bfloat16)
    ref = torch.nn.functional.silu(h[:, :F_]) * h[:, F_:]
    a = act.view(F_ // 16, rb, 2, 32, 8).permute(1, 3, 0, 2, 4).reshape(rb * 32, F_)[:M]
    d = (a.float() - ref.float()).abs()
    assert (d > 0).float().mean() <= 0.02 and d.max() <= 0.07, ((d > 0).float().mean(), d.max())


# ------------------------------------------------------------------------------------------------ 3. true width against the oracle
def fp4_policy():
    from oracle.numerics import BF16, F32, Policy

    class Fp4aPolicy(Policy):
        """The oracle's "fp8wa" flow with the weights of the ``quant and act8`` Linears stored as MXFP4 (this file's restatement)."""

        def __init__(self):
            super().__init__("fp8wa")
            self._w = {}

        def linear(self, x, w, b=None, quant=True, act8=False):
            if not (quant and act8):
                return super().linear(x, w, b, quant=quant, act8=act8)
            xs = x.to(F32)
            am = xs.abs().amax(dim=-1, keepdim=True)
            inv = torch.where(am > 0, 448.0 / am, torch.zeros_like(am))
            xq = (xs * inv).to(torch.float8_e4m3fn).to(F32)
            key = (w.data_ptr(), tuple(w.shape))
            if key not in self._w:                           # (the table search is done where it is fast; the values are exact either way)
                wd = w.to(BF16).to(F32).to(DEV)
                self._w[key] = dequant(*restated_quant(wd)).to(F32).cpu()
            acc = (xq @ self._w[key].t()) * (am / 448.0)
            if b is not None:
                acc = acc + b.to(BF16).to(F32)
            return acc.to(BF16)

    return Fp4aPolicy()


def head_eval_device(sd_dev, weights, D, P, depth, nada, seed, C=32, B=1, branches=2, n_steps=3, eval_index=1):
    """The device side of oracle/true_dims.py head_case (that driver maps an unknown mode to the bf16 policy, so its few lines are restated)."""
    from bitdance_amd import engine as E
    hw = E.HeadWeights.from_state_dict(sd_dev, DEV, weights=weights)
    eng = E.Engine(hw, None, None, num_images=B, branches=branches, device=DEV, max_tokens=P, parallel_num=P)
    M = branches * B * P
    g = torch.Generator().manual_seed(seed + 1)
    z = torch.randn(branches * B, P, D, generator=g)
    x = torch.randn(B, P, C, generator=g)
    eng.set_schedule(n_steps, 3.0, 1)
    eng.load_noise(torch.zeros(1, n_steps + 1, B, P, C))
    eng.reset([0] * (branches * B))
    eng.set_int("rt.dump_xhat", 1)
    eng.set_cond(z.to(DEV))
    eng.view("head.xt", torch.float32, (B * P, C)).copy_(x.reshape(B * P, C).to(DEV))
    eng.head_cond()
    eng.head_eval(eval_index)
    torch.cuda.synchronize()
    xhat = eng.view("head.xhat", torch.float32, (eng.Mpad, C))[:M].cpu().view(branches * B, P, C)
    return xhat, float(eng._sc[eval_index, 0]), z, torch.cat([x] * branches)


@pytest.mark.parametrize("D,P,depth,nada", [(256, 64, 4, 2), (5120, 64, 2, 2)])
def test_head_eval_fp4a_vs_oracle(D, P, depth, nada):
    """Bounds: those of test_gpu_fp8.py::test_head_eval_fp8a_vs_oracle against the same-policy oracle -- both sides quantise the weights
    identically, the residual is activations that land on an e4m3 rounding boundary after a different fp32 summation order.  The
    distance to the bf16 flow is bounded relative to fp8a's on the same seeded model: mean <= 4.4 x 1.5 x fp8a's mean (4.4 = the ratio
    of the relative rms error of one GEMM, MXFP4 0.116 against per-channel e4m3 0.026 at K = 5120; 1.5 = head-room for the layers
    between).  Measured on an MI355X (vs the same-policy oracle max / mean; vs the bf16 flow mean fp4a / fp8a / ratio):
    D = 256: 0.199 / 0.0209; 0.1202 / 0.0445 / 2.70.  D = 5120: 0.074 / 0.0129; 0.0983 / 0.0358 / 2.75."""
    from oracle import diff_head, tiny_models as tm
    from oracle.numerics import Policy
    from oracle.true_dims import device_seeded_state
    seed = 401
    cfgd = dict(ch_target=32, ch_cond=D, ch_latent=D, depth_latent=depth, depth_adanln=nada)
    sd_dev = device_seeded_state(tm.head_shapes(cfgd), seed, DEV)
    x4, t_i, z, comb = head_eval_device(sd_dev, "fp4a", D, P, depth, nada, seed)
    x8, t8, _, _ = head_eval_device(sd_dev, "fp8a", D, P, depth, nada, seed)
    assert t8 == t_i
    sd = {k: v.cpu() for k, v in sd_dev.items()}
    del sd_dev
    tt = torch.full((2,), t_i)
    with torch.no_grad():
        ref4 = diff_head.net_forward(sd, comb, tt, z, fp4_policy(), final_sigmoid=True, head_dim=128).float()
        ref16 = diff_head.net_forward(sd, comb, tt, z, Policy("autocast"), final_sigmoid=True, head_dim=128).float()
    err = (x4 - ref4).abs()
    d4, d8 = (x4 - ref16).abs(), (x8 - ref16).abs()
    r = dict(max_err=err.max().item(), mean_err=err.mean().item(), vs_bf16_max=d4.max().item(), vs_bf16_mean=d4.mean().item(),
             fp8a_vs_bf16_max=d8.max().item(), fp8a_vs_bf16_mean=d8.mean().item())
    print(f"[fp4a head D={D}] vs fp4a oracle: max {r['max_err']:.4f} mean {r['mean_err']:.5f}; vs bf16 flow: max {r['vs_bf16_max']:.4f} mean "
          f"{r['vs_bf16_mean']:.5f}; fp8a vs bf16 flow: max {r['fp8a_vs_bf16_max']:.4f} mean {r['fp8a_vs_bf16_mean']:.5f}; ratio of the means "
          f"{r['vs_bf16_mean'] / r['fp8a_vs_bf16_mean']:.2f}")
    assert bool(torch.isfinite(x4).all()) and r["max_err"] <= 0.25 and r["mean_err"] <= 3.5e-2, r
    if D == 5120:
        assert r["max_err"] <= 0.15 and r["mean_err"] <= 2.2e-2, r
    assert r["vs_bf16_mean"] <= 4.4 * 1.5 * r["fp8a_vs_bf16_mean"], r


def llm_step_device(sd_dev, c, weights, past, P, seed):
    """The device side of oracle/true_dims.py llm_case, restated for the same reason as head_eval_device."""
    from bitdance_amd import engine as E
    layers, nkv, hd, D = c["num_hidden_layers"], c["num_key_value_heads"], c["head_dim"], c["hidden_size"]
    lw = E.LlmWeights.from_state_dict(sd_dev, c, DEV, keep_for_prefill=False, weights=weights)
    nseq = len(past)
    eng = E.Engine(None, None, lw, num_images=nseq, branches=1, device=DEV, max_tokens=P, max_kv=max(past) + 2 * P, parallel_num=P)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(nseq, P, D, generator=g)
    kc = eng.ws["llm.k_cache"].view(torch.bfloat16).view(layers, nseq, nkv, eng.Lmax, hd)
    vc = eng.ws["llm.vt_cache"].view(torch.bfloat16).view(layers, nseq, nkv, hd, eng.Lmax)
    caches = []
    for b, L in enumerate(past):
        per = []
        for li in range(layers):
            k = torch.randn(1, nkv, L, hd, generator=g).to(torch.bfloat16)
            v = torch.randn(1, nkv, L, hd, generator=g).to(torch.bfloat16)
            kc[li, b, :, :L] = k[0].to(DEV)
            vc[li, b, :, :, :L] = v[0].transpose(1, 2).to(DEV)
            per.append([k, v])
        caches.append(per)
    eng.set_int("rt.emit_cond", 0)
    eng.reset(list(past))
    eng.residual()[: nseq * P].copy_(x.reshape(nseq * P, D).to(DEV))
    eng.llm_step()
    torch.cuda.synchronize()
    return eng.hidden().cpu().view(nseq, P, D).float(), x, caches


def test_llm_step_fp4a_vs_oracle_true_dims():
    """Bounds of test_gpu_fp8.py::test_llm_step_fp8a_vs_oracle_true_dims against the same-policy oracle; the distance to the bf16 flow
    relative to fp8a's as in the head test.  Measured on an MI355X: vs the same-policy oracle max 0.036 / mean 0.0024; vs the bf16 flow
    mean 0.0721 (fp8a 0.0249, ratio 2.89)."""
    from oracle import qwen3, tiny_models as tm
    from oracle.numerics import Policy
    from oracle.true_dims import QWEN3_14B, device_seeded_state
    seed, past, P = 403, (1000, 1017), 64
    c = dict(QWEN3_14B, num_hidden_layers=1)
    sd_dev = {k: v.to(torch.bfloat16) for k, v in device_seeded_state(tm.llm_shapes(c), seed, DEV).items()}
    h4, x, caches = llm_step_device(sd_dev, c, "fp4a", past, P, seed)
    h8, _, _ = llm_step_device(sd_dev, c, "fp8a", past, P, seed)
    w = {k: v.cpu() for k, v in sd_dev.items()}
    del sd_dev

    def oracle(pol):
        refs = []
        with torch.no_grad():
            for b, L in enumerate(past):
                ones = torch.ones(1, 1, P, L + P, dtype=torch.bool)
                o, _ = qwen3.model_forward(w, c, x[b:b + 1], [list(kv) for kv in caches[b]], ones, pol)
                refs.append(o.float())
        return torch.cat(refs)

    ref4, ref16 = oracle(fp4_policy()), oracle(Policy("autocast"))
    err, d4, d8 = (h4 - ref4).abs(), (h4 - ref16).abs(), (h8 - ref16).abs()
    r = dict(max_err=err.max().item(), mean_err=err.mean().item(), vs_bf16_max=d4.max().item(), vs_bf16_mean=d4.mean().item(),
             fp8a_vs_bf16_max=d8.max().item(), fp8a_vs_bf16_mean=d8.mean().item())
    print(f"[fp4a llm] vs fp4a oracle: max {r['max_err']:.4f} mean {r['mean_err']:.5f}; vs bf16 flow: max {r['vs_bf16_max']:.4f} mean "
          f"{r['vs_bf16_mean']:.5f}; fp8a vs bf16 flow: max {r['fp8a_vs_bf16_max']:.4f} mean {r['fp8a_vs_bf16_mean']:.5f}; ratio of the means "
          f"{r['vs_bf16_mean'] / r['fp8a_vs_bf16_mean']:.2f}")
    assert bool(torch.isfinite(h4).all()) and r["max_err"] <= 0.15 and r["mean_err"] <= 1.2e-2, r
    assert r["vs_bf16_mean"] <= 4.4 * 1.5 * r["fp8a_vs_bf16_mean"], r


# ------------------------------------------------------------------------------------------------ 4. pipeline
def tiny_pipeline_mode(weights):
    from bitdance_amd.autoencoder import VQModel
    from bitdance_amd.t2i_pipeline import BitDanceT2IPipeline
    from oracle import tiny_models as tm
    llm_sd = {k: v.to(torch.bfloat16) for k, v in tm.seeded_state(tm.llm_shapes(tm.TINY_LLM), seed=22).items()}
    ae_shapes = {k: tuple(v.shape) for k, v in VQModel(**tm.TINY_AE).state_dict().items()}
    return BitDanceT2IPipeline.from_components(
        tokenizer=tm.FakeTokenizer(), llm_cfg=tm.TINY_LLM, llm_sd=llm_sd, ae_config=tm.TINY_AE,
        ae_sd=tm.seeded_state(ae_shapes, seed=44, gain=1.4), head_config=dict(tm.TINY_HEAD),
        head_sd=tm.seeded_state(tm.head_shapes(tm.TINY_HEAD), seed=11), proj_sd=tm.seeded_state(tm.proj_shapes(32, 256), seed=33),
        device=DEV, weights=weights)


def test_pipeline_fp4a():
    """The tiny pipeline of test_gpu_fp8.py::test_pipeline_fp8_runs_and_tracks_bf16 with weights="fp4a".  Token agreement with the bf16
    pipeline on the first patch is printed, not asserted (8-bit weights sit at 0.70 there against a chance level of 0.5; measured on an
    MI355X: fp4a 0.679, fp8a 0.796)."""
    p4, p8, p16 = tiny_pipeline_mode("fp4a"), tiny_pipeline_mode("fp8a"), tiny_pipeline_mode("bf16")
    n, steps = 3, 2
    noise = torch.randn(steps, n + 1, 1, 64, 32, generator=torch.Generator().manual_seed(7))
    kw = dict(guidance_scale=3.0, num_sampling_steps=n, max_length=128, num_images=1, image_size=[256, 128], noise=noise)
    p4.use_graph = False
    t_eager = p4.gen_image("a red fox", "<|", return_tokens=True, **kw).cpu()
    p4.use_graph = True
    t_graph = p4.gen_image("a red fox", "<|", return_tokens=True, **kw).cpu()
    t_again = p4.gen_image("a red fox", "<|", return_tokens=True, **kw).cpu()
    assert torch.equal(t_eager, t_graph) and torch.equal(t_graph, t_again)
    assert set(t_graph.unique().tolist()) <= {-1.0, 0.0, 1.0}
    img = p4.gen_image("a red fox", "<|", **kw)
    assert img.shape == (1, 3, 256, 128) and torch.isfinite(img).all()
    t16 = p16.gen_image("a red fox", "<|", return_tokens=True, **kw).cpu()
    t8 = p8.gen_image("a red fox", "<|", return_tokens=True, **kw).cpu()
    print(f"[fp4a tiny pipeline] first-patch token agreement with the bf16 pipeline: fp4a {(t_graph[:, :64] == t16[:, :64]).float().mean().item():.4f}, "
          f"fp8a {(t8[:, :64] == t16[:, :64]).float().mean().item():.4f} (chance 0.5)")
    # storage: the five GEMMs' weights are half of fp8a's bytes + one exponent byte per 32 weights (whole dwords per lane and four stages);
    # no per-channel scale; every other streamed Linear is stored as in fp8a
    from bitdance_amd import engine as E
    five = 0
    for w4, w8 in ((p4.head_w.ptrs, p8.head_w.ptrs), (p4.llm_w.ptrs, p8.llm_w.ptrs), (p4.proj_w.ptrs, p8.proj_w.ptrs)):
        assert {k for k in w8 if not k.endswith("_s")} == {k for k in w4 if not k.endswith(("_s", "_e"))}
        for k in w8:
            if k.endswith("_s"):
                continue
            if k + "_e" in w4:
                five += 1
                assert k + "_s" not in w4 and w4[k].dtype == torch.uint8 and 2 * w4[k].numel() == w8[k].numel(), k
                N = w8[k + "_s"].numel()
                K = w8[k].numel() // N
                assert w4[k + "_e"].numel() == E.mxfp4_exp_bytes(N, K) >= N * K // 32, k
            else:
                assert (k + "_s" in w4) == (k + "_s" in w8) and w4[k].numel() == w8[k].numel() and w4[k].dtype == w8[k].dtype, k
    nblk, nl = p4.head_w.nblocks, p4.llm_w.cfg["num_hidden_layers"]
    assert five == 1 + 2 * nblk + 2 * nl, five               # adaLN + (qkv, w1) per head block + (qkv, gate/up) per LLM layer


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals():
    from bitdance_amd._lib import BD_ERR_UNSUPPORTED, lib
    l = lib()
    st = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    f32 = torch.ones(128, device=DEV)
    out = torch.zeros(128 * 64, device=DEV)
    p = buf.data_ptr()
    # K % 64 != 0; a null exponent stream: refused before any launch
    assert l.bd_gemm_w4a8(p, f32.data_ptr(), 4, p, p, None, 64, 96, 1, 2 + 32, 0, None, None, out.data_ptr(), st) == BD_ERR_UNSUPPORTED
    assert b"64" in l.bd_last_error()
    assert l.bd_gemm_w4a8(p, f32.data_ptr(), 4, p, None, None, 64, 64, 1, 2 + 32, 0, None, None, out.data_ptr(), st) == BD_ERR_UNSUPPORTED
    assert b"exponent" in l.bd_last_error()
    assert l.bd_pack_weight4k(p, p, p, p, 32, 96, 0, 32, st) == BD_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0

    def finalize(ints):
        ctx = l.bd_ctx_create()
        try:
            for k, v in ints.items():
                assert l.bd_ctx_set_int(ctx, k.encode(), v) == 0, k
            return l.bd_ctx_finalize(ctx), l.bd_last_error().decode()
        finally:
            l.bd_ctx_destroy(ctx)

    llm = {"B": 1, "branches": 2, "P": 64, "llm.D": 256, "llm.L": 1, "llm.nh": 2, "llm.nkv": 2, "llm.F": 512, "llm.Lmax": 256, "llm.head_dim": 64}
    rc, msg = finalize(dict(llm, **{"wdtype": 3, "llm.variant": 1}))              # the imagenet transformer
    assert rc == BD_ERR_UNSUPPORTED and "wdtype 3" in msg, (rc, msg)
    for bad in (4, -1, 17):
        rc, msg = finalize({"B": 1, "branches": 2, "P": 64, "wdtype": bad})
        assert rc != 0 and "wdtype" in msg, (bad, rc, msg)
    for ok in (0, 1, 2, 3):
        rc, msg = finalize({"B": 1, "branches": 2, "P": 64, "wdtype": ok})
        assert rc == 0, (ok, rc, msg)
    from bitdance_amd import engine as E
    from oracle import tiny_models as tm
    sd = tm.seeded_state(tm.mlp_head_shapes(dict(ch_target=32, ch_cond=256, ch_latent=256, depth_latent=2, depth_adanln=1)), seed=3)
    with pytest.raises(E.BitDanceUnsupported):
        E.HeadWeights.from_state_dict(sd, DEV, weights="fp4a")
