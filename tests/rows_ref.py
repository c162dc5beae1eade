"""References, input generators, bounds and the judge for tests/test_gpu_rows.py and tests/test_rows_ref_cpu.py.

Every reference is plain torch on the bf16 / fp32 inputs the kernel reads, in the dtype it is given (float64: the reference; float32:
the precision check of the CPU test), with the rounding points the kernel comments attribute to the reference model written as
`bfr()` (.to(bfloat16).to(dtype)) and nothing else.  A reference takes a `fault` name and then computes that wrong thing instead
(the CPU test proves the bounds reject every fault).

The judge (`Report`) holds an implementation -- the device, the float32 run, or a faulted float64 run -- to two conditions per
bf16 output, with u = the bf16 spacing at the reference value:

  (a) |got - bf16(ref)| <= u + tol, where tol is the propagated term the reference function derives next to each output: the fp32
      reductions of the kernel (gamma(n) = (n + 16) 2^-24 relative, the worst case of an n-term fp32 sum in any order) and, where
      an earlier rounding of the SAME kernel feeds the output, one spacing of that intermediate times the derivative;
  (b) at most FLIP_CAP = 1 % of the elements differ from bf16(ref) at all.

Outputs that are fp32 are held to tol alone, integer-valued and copied ones to equality.  Where a kernel writes an intermediate back
(the residual stream X / R), the judge checks it first and computes the next stage from the implementation's own copy, so that one
rare flip of the intermediate is not charged to every element behind the row statistics.
"""
from __future__ import annotations

import math
import types

import torch

BF16 = torch.bfloat16
U = 2.0 ** -8
F32 = 2.0 ** -24
FLIP_CAP = 0.01


def bfr(x):
    return x.to(BF16).to(x.dtype)


def gamma(n):
    return (n + 16) * F32


def ulp_bf16(v):
    """Spacing of bf16 (8 significant bits) at |v|, float64."""
    _, e = torch.frexp(v.double().abs().clamp_min(2.0 ** -120))
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - 8)


def unfrag(buf: torch.Tensor, rb: int, width: int) -> torch.Tensor:
    """Fragment-major bf16 [width / 16][rb][2][32][8] -> row-major [rb * 32][width] (as test_gemm_swiglu un-fragments)."""
    return buf.view(width // 16, rb, 2, 32, 8).permute(1, 3, 0, 2, 4).reshape(rb * 32, width)


def unfrag8(buf: torch.Tensor, rb: int, width: int) -> torch.Tensor:
    """The A8 layout [stage of 64][row block][k / 16 % 2][k / 32 % 2][row % 32][16 bytes] -> row-major uint8 [rb * 32][width]
    (the un-fragmenting of tests/test_gpu_fp8.py)."""
    return buf.view(width // 64, rb, 2, 2, 32, 16).permute(1, 4, 0, 3, 2, 5).reshape(rb * 32, width)


def case(**kw):
    return types.SimpleNamespace(**kw)


def to_device(c, dev):
    return types.SimpleNamespace(**{k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in vars(c).items()})


# ---------------------------------------------------------------------------------------------------------------------------------
class Report:
    """Collects the failures and the two headroom figures of one case: `flip` = the worst share of elements that differ from the
    rounded reference, `excess` = the worst (|got - ref| - allowed) in units of the bf16 spacing (<= 0 passes; -1 = identical)."""

    def __init__(self, what):
        self.what, self.fail, self.flip, self.excess = what, [], 0.0, -1.0

    def _worst(self, name, ex, got, ref, allow):
        w = int(ex.argmax())
        self.fail.append(f"{self.what} {name}: {int((ex > 0).sum())} elements out of bounds; worst at flat index {w}: "
                         f"got {got.flatten()[w].item():.8g} ref {ref.flatten()[w].item():.8g} tol {allow.flatten()[w].item():.3g}")

    def bf16(self, name, got, val, tol=None):
        exp = val.to(BF16).double()
        g = got.double()
        if g.shape != exp.shape:
            self.fail.append(f"{self.what} {name}: shape {tuple(g.shape)} vs {tuple(exp.shape)}")
            return
        if g.numel() == 0:
            return
        if not torch.isfinite(g).all():
            self.fail.append(f"{self.what} {name}: {int((~torch.isfinite(g)).sum())} non-finite elements")
            return
        u = ulp_bf16(exp)
        allow = u if tol is None else u + tol.double()
        ex = ((g - exp).abs() - allow) / u
        self.excess = max(self.excess, ex.max().item())
        if ex.max() > 0:
            self._worst(name, ex, g, exp, allow)
        flip = (g != exp).double().mean().item()
        self.flip = max(self.flip, flip)
        if flip > FLIP_CAP:
            self.fail.append(f"{self.what} {name}: {flip:.4%} of the elements differ from the rounded reference (cap {FLIP_CAP:.0%})")

    def f32(self, name, got, val, tol, tight=None):
        """An fp32 output: every element within tol; with `tight` (the fp32-only part of tol, without the spacing of an earlier
        rounding) at most FLIP_CAP of the elements further than that from the reference."""
        g, v = got.double(), val.double()
        if not torch.isfinite(g).all():
            self.fail.append(f"{self.what} {name}: non-finite")
            return
        ex = (g - v).abs() - tol.double() - 1e-30
        if ex.max() > 0:
            self._worst(name, ex, g, v, tol.double())
        if tight is not None:
            flip = ((g - v).abs() > tight.double() + 1e-30).double().mean().item()
            self.flip = max(self.flip, flip)
            if flip > FLIP_CAP:
                self.fail.append(f"{self.what} {name}: {flip:.4%} of the elements off by more than the fp32 term (cap {FLIP_CAP:.0%})")

    def equal(self, name, got, want):
        if got.shape != want.shape or not torch.equal(got, want):
            n = int((got != want).sum()) if got.shape == want.shape else -1
            self.fail.append(f"{self.what} {name}: {n} elements differ from the expected bits")

    def fp8(self, name, codes, scale, val, tol):
        """Row-quantised e4m3 output: scale = amax / 448 of the reference row to a few fp32 ulps (+ the propagated tol at the
        row maximum); codes within one e4m3 step of the oracle quantiser's ((v / scale).to(float8_e4m3fn)), <= 1 % different."""
        v = val.double()
        amax = v.abs().amax(-1)
        s_ref = amax / 448.0
        s_tol = s_ref * 8 * F32 + tol.double().amax(-1) / 448.0 + 1e-30
        self.f32(name + ".scale", scale, s_ref, s_tol)
        s32 = s_ref.float().clamp_min(1e-30)
        want = (v.float() / s32[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
        sgn = lambda q: torch.where(q >= 128, -(q.int() - 128), q.int())
        d = (sgn(codes) - sgn(want)).abs()
        if d.max() > 1:
            self.fail.append(f"{self.what} {name}: {int((d > 1).sum())} codes more than one e4m3 step from the oracle quantiser's")
        flip = (d > 0).double().mean().item()
        self.flip = max(self.flip, flip)
        if flip > FLIP_CAP:
            self.fail.append(f"{self.what} {name}: {flip:.4%} of the codes differ (cap {FLIP_CAP:.0%})")

    def line(self):
        return f"ROWSTAT {self.what} flip={self.flip:.3e} excess={self.excess:+.3f}"


# ---------------------------------------------------------------------------------------------------------------------------------
# a Linear output as the row kernels read it: S >= 1 split-K slabs [S][rows][N] fp32 (+ bf16 bias), S == 0 finished bf16, S < 0 none
def linear_out(p, bias, S, M, dtype, fault=None):
    """-> (unrounded value, its fp32-summation tol, the bf16-rounded value), rows 0 .. M - 1."""
    if S == 0:
        v = p[:M].to(dtype)
        return v, torch.zeros_like(v), v
    slabs = p[:, :M].to(dtype)
    if fault == "drop_last_slab":
        slabs = slabs[:-1]
    v = slabs.sum(0)
    mag = slabs.abs().sum(0)
    if bias is not None and fault != "drop_bias":
        v = v + bias.to(dtype)
        mag = mag + bias.to(dtype).abs()
    return v, gamma(S) * mag, bfr(v)


def gen_linear(g, S, bias, rows, N, M, scale=1.0, row_scale=None):
    """Slabs whose sum is ~ N(0, scale^2) (rows past M hold other finite values: nobody may read them into a result)."""
    if S < 0:
        return None, None
    f = torch.ones(rows, 1) if row_scale is None else torch.cat([row_scale, torch.ones(rows - M, 1)])
    if S == 0:
        return (torch.randn(rows, N, generator=g) * scale * f).to(BF16), None
    p = torch.randn(S, rows, N, generator=g) * (scale / math.sqrt(S)) * f
    b = (torch.randn(N, generator=g) * 0.3 * scale).to(BF16) if bias else None
    return p, b


def small_rows(M, eps, var=2.0):
    """Row factors: rows 0, 4, 8 .. are scaled so that their variance is ~ 3 eps (eps matters there), the rest 1."""
    f = torch.ones(M, 1)
    f[0::4] = min(1.0, math.sqrt(3 * eps / var))
    return f


# ---------------------------------------------------------------------------------------------------------------------------------
# ln_mod:  x = bf16(x + bf16(bf16(branch) * gate)) ; h = LN(x) [* w + b] * bf16(1 + scale) + shift          (bd_rows.hip ln_mod_kernel)
LN_FAULTS = ("no_bfr_branch", "no_bfr_gated", "no_bfr_resid", "no_bfr_1p_scale", "round_after_mul", "eps10", "swap_gate_scale",
             "swap_gate_shift", "swap_scale_shift", "drop_last_slab", "drop_bias")


def gen_ln_mod(M, D, S, bias, affine, ada_ld, offs, eps, seed, fp8=0, wave_rows=0, occ=5, rows=None):
    g = torch.Generator().manual_seed(seed)
    rows = rows or (M + 31) // 32 * 32
    f = small_rows(M, eps)
    go, so, fo = offs
    ada = (torch.randn(M, ada_ld, generator=g) * 0.5).to(BF16)
    ada[:, go:go + D] = (torch.randn(M, D, generator=g) * f).to(BF16)          # gate ~ x: the gated branch is comparable to x
    X = (torch.randn(M, D, generator=g) * f).to(BF16)
    pend, b = gen_linear(g, S, bias, rows, D, M)
    ln_w = (1 + 0.3 * torch.randn(D, generator=g)) if affine else None
    ln_b = (0.3 * torch.randn(D, generator=g)) if affine else None
    return case(M=M, D=D, S=S, X=X, pend=pend, bias=b, ada=ada, ada_ld=ada_ld, offs=offs, ln_w=ln_w, ln_b=ln_b, eps=eps, fp8=fp8,
                wave_rows=wave_rows, occ=occ, rows=rows)


def ref_ln_mod(c, dtype=torch.float64, fault=None, X=None, with_pend=True):
    """-> dict: x / x_tol (the residual written back; None without a pending branch), h / h_tol (unrounded)."""
    go, so, fo = c.offs
    if fault == "swap_gate_scale": go, so = so, go
    if fault == "swap_gate_shift": go, fo = fo, go
    if fault == "swap_scale_shift": so, fo = fo, so
    M, D = c.M, c.D
    eps = c.eps * (10 if fault == "eps10" else 1)
    x = (c.X if X is None else X)[:M].to(dtype)
    out = dict(x=None, x_tol=None)
    if with_pend and c.S >= 0:
        o, o_tol, ob = linear_out(c.pend, c.bias, c.S, M, dtype, fault)
        if fault == "no_bfr_branch": ob = o
        gt = c.ada[:M, go:go + D].to(dtype)
        t = ob * gt
        tb = t if fault == "no_bfr_gated" else bfr(t)
        xs = x + tb
        out["x"], out["x_tol"] = xs, ulp_bf16(t).to(dtype) + gt.abs() * (ulp_bf16(o).to(dtype) + o_tol)
        x = xs if fault == "no_bfr_resid" else bfr(xs)
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = ((xc * xc).mean(-1, keepdim=True) + eps).rsqrt()
    ln = xc * rstd
    w = c.ln_w.to(dtype) if c.ln_w is not None else torch.ones(D, dtype=dtype, device=x.device)
    lna = ln * w + c.ln_b.to(dtype) if c.ln_w is not None else ln
    sc1 = 1 + c.ada[:M, so:so + D].to(dtype)
    sf = c.ada[:M, fo:fo + D].to(dtype)
    if fault == "round_after_mul":
        h = bfr(lna * sc1) + sf
    else:
        h = lna * (sc1 if fault == "no_bfr_1p_scale" else bfr(sc1)) + sf
    gm = gamma(D)
    dm = gm * x.abs().mean(-1, keepdim=True)                                   # fp32 error of the mean; rstd: gm relative
    out["h"] = h
    out["h_tol"] = bfr(sc1).abs() * w.abs() * (dm * rstd + ln.abs() * 2 * gm) + 4 * F32 * ((lna * sc1).abs() + sf.abs())
    return out


def impl_ln_mod(c, dtype, fault=None):
    r = ref_ln_mod(c, dtype, fault)
    got = dict(X=r["x"].to(BF16) if r["x"] is not None else c.X[:c.M].clone())
    if c.fp8:
        got["h8"], got["scale"] = quant_rows(r["h"])
    else:
        got["h"] = r["h"].to(BF16)
    return got


def quant_rows(h):
    """The oracle's row quantiser in fp32: scale = amax / 448, codes = e4m3(v / scale)."""
    v = h.float()
    s = v.abs().amax(-1) / 448.0
    return (v / s.clamp_min(1e-30)[:, None]).to(torch.float8_e4m3fn).view(torch.uint8), s


def judge_ln_mod(c, got, what):
    rep = Report(what)
    if c.S >= 0:
        r = ref_ln_mod(c)
        rep.bf16("X", got["X"], r["x"], r["x_tol"])
    else:
        rep.equal("X", got["X"], c.X[:c.M])
    r = ref_ln_mod(c, X=got["X"], with_pend=False)
    if c.fp8:
        rep.fp8("h8", got["h8"], got["scale"], r["h"], r["h_tol"])
    else:
        rep.bf16("h", got["h"], r["h"], r["h_tol"])
    return rep


_A6 = 6 * 5120
LN_CASES = {
    # released head: D 5120, the adaLN row of six chunks; every order of (gate, scale, shift) over the cases
    "d5120_m128_s6_bias": lambda: gen_ln_mod(128, 5120, 6, 1, 0, _A6, (0, 5120, 10240), 1e-6, 1),
    "d5120_m33_s7_occ4": lambda: gen_ln_mod(33, 5120, 7, 1, 0, _A6, (25600, 15360, 20480), 1e-6, 2, occ=4),
    "d5120_m1_s13_affine": lambda: gen_ln_mod(1, 5120, 13, 0, 1, _A6, (10240, 0, 5120), 1e-6, 3),
    "d5120_m40_s6_fp8": lambda: gen_ln_mod(40, 5120, 6, 1, 0, _A6, (5120, 10240, 0), 1e-6, 4, fp8=1),
    "d5120_m8_s0_fp8_occ4": lambda: gen_ln_mod(8, 5120, 0, 0, 1, _A6, (0, 10240, 5120), 1e-5, 5, fp8=1, occ=4),
    "d8192_m5_nopend": lambda: gen_ln_mod(5, 8192, -1, 0, 0, 3 * 8192, (16384, 8192, 0), 1e-6, 6),
    "d256_m37_s1": lambda: gen_ln_mod(37, 256, 1, 1, 1, 1024, (768, 8, 264), 1e-2, 7),
    "d1280_m12_s0_occ4": lambda: gen_ln_mod(12, 1280, 0, 0, 1, 6 * 1280, (1280, 0, 2560), 1e-6, 8, occ=4),
    "d768_m3_nopend_fp8": lambda: gen_ln_mod(3, 768, -1, 0, 1, 6 * 768, (0, 768, 1536), 1e-5, 9, fp8=1),
    # the wave-per-row form: NPASS 1 (D <= 512) and 2, M not a multiple of 8
    "rows_d256_m13_s6": lambda: gen_ln_mod(13, 256, 6, 1, 0, 6 * 256, (512, 256, 0), 1e-6, 10, wave_rows=1),
    "rows_d512_m64_nopend": lambda: gen_ln_mod(64, 512, -1, 0, 1, 6 * 512, (0, 1024, 512), 1e-2, 11, wave_rows=1),
    "rows_d768_m203_s7": lambda: gen_ln_mod(203, 768, 7, 1, 1, 6 * 768, (1536, 768, 0), 1e-6, 12, wave_rows=1),
    "rows_d1024_m9_s0": lambda: gen_ln_mod(9, 1024, 0, 0, 0, 6 * 1024, (3072, 4096, 5120), 1e-6, 13, wave_rows=1),
    "rows_d1024_m1_s1": lambda: gen_ln_mod(1, 1024, 1, 0, 0, 3 * 1024, (1024, 2048, 0), 1e-6, 14, wave_rows=1),
}


# ---------------------------------------------------------------------------------------------------------------------------------
# rms (Qwen3):  R += bf16(branch) [bf16 stream: rounded] ; n = w * (R rsqrt(mean R^2 + eps)) [bf16 stream: bf16(w * bf16(..))]
RMS_FAULTS = ("no_bfr_branch", "no_bfr_resid", "no_bfr_inner", "eps10", "drop_last_slab", "drop_bias", "pos_prev_step", "pos_next_row")


def gen_rms(M, D, S, bias, bf16_stream, eps, seed, fp8=0, hidden=0, cond=0, P=1, step=0, a_frag=1):
    g = torch.Generator().manual_seed(seed)
    rows = (M + 31) // 32 * 32
    f = small_rows(M, eps) if not bias else None
    R = torch.randn(M, D, generator=g) * (f if f is not None else 1.0)
    if bf16_stream:
        R = R.to(BF16).float()
    pend, b = gen_linear(g, S, bias, rows, D, M, row_scale=f)
    w = (1 + 0.3 * torch.randn(D, generator=g)).to(BF16)
    pos = torch.randn((step + 1) * P + 1, D, generator=g) if cond else None
    return case(M=M, D=D, S=S, R=R, pend=pend, bias=b, w=w, eps=eps, bf16_stream=bf16_stream, fp8=fp8, hidden=hidden, cond=cond,
                P=P, step=step, pos=pos, rows=rows, a_frag=a_frag)


def ref_rms(c, dtype=torch.float64, fault=None, R=None, with_pend=True):
    M, D = c.M, c.D
    eps = c.eps * (10 if fault == "eps10" else 1)
    r = (c.R if R is None else R)[:M].to(dtype)
    out = dict(r=None)
    if with_pend and c.S >= 0:
        o, o_tol, ob = linear_out(c.pend, c.bias, c.S, M, dtype, fault)
        if fault == "no_bfr_branch": ob = o
        rs_ = r + ob
        out["r"], out["r_tol"] = rs_, ulp_bf16(o).to(dtype) + o_tol + 2 * F32 * rs_.abs()
        out["r_tight"] = 2 * F32 * rs_.abs()
        r = bfr(rs_) if (c.bf16_stream and fault != "no_bfr_resid") else rs_
    rs = ((r * r).mean(-1, keepdim=True) + eps).rsqrt()
    w = c.w.to(dtype)
    gm = gamma(D)
    inner = r * rs
    if c.bf16_stream:
        ib = inner if fault == "no_bfr_inner" else bfr(inner)
        n = w * ib
        n_tol = w.abs() * (ulp_bf16(inner).to(dtype) + inner.abs() * (gm + 2 * F32))
        nb = bfr(n)                                                # what hidden_out / the position add see
    else:
        n = w * inner
        n_tol = n.abs() * (gm + 4 * F32)
        nb = n
    out.update(n=n, n_tol=n_tol)
    if c.cond:
        step = c.step - (1 if fault == "pos_prev_step" else 0)
        idx = step * c.P + torch.arange(M, device=r.device) % c.P + (1 if fault == "pos_next_row" else 0)
        pe = c.pos.to(dtype)[idx]
        out["cond"] = nb + pe
        out["cond_tol"] = n_tol + (ulp_bf16(n).to(dtype) if c.bf16_stream else 0) + 2 * F32 * (nb + pe).abs()
    return out


def impl_rms(c, dtype, fault=None):
    r = ref_rms(c, dtype, fault)
    if r["r"] is not None:
        Rn = bfr(r["r"]).float() if (c.bf16_stream and fault != "no_bfr_resid") else r["r"].float()
    else:
        Rn = c.R[:c.M].clone()
    got = dict(R=Rn)
    n = bfr(r["n"]) if c.bf16_stream else r["n"]
    if c.a_frag:
        if c.fp8:
            got["a8"], got["scale"] = quant_rows(n)
        else:
            got["a"] = r["n"].to(BF16)
    if c.hidden:
        got["hidden"] = n.float()
    if c.cond:
        got["cond"] = r["cond"].to(BF16)
    return got


def judge_rms(c, got, what):
    rep = Report(what)
    if c.S >= 0:
        r = ref_rms(c)
        if c.bf16_stream:
            rep.bf16("R", got["R"], r["r"], r["r_tol"])
        else:
            rep.f32("R", got["R"], r["r"], r["r_tol"], r["r_tight"])
    else:
        rep.equal("R", got["R"], c.R[:c.M])
    r = ref_rms(c, R=got["R"], with_pend=False)
    if c.a_frag:
        if c.fp8:
            rep.fp8("a8", got["a8"], got["scale"], bfr(r["n"]) if c.bf16_stream else r["n"], r["n_tol"] + (ulp_bf16(r["n"]) if c.bf16_stream else 0))
        else:
            rep.bf16("a", got["a"], r["n"], r["n_tol"])
    if c.hidden:
        if c.bf16_stream:
            rep.bf16("hidden", got["hidden"], r["n"], r["n_tol"])
        else:
            rep.f32("hidden", got["hidden"], r["n"], r["n_tol"])
    if c.cond:
        rep.bf16("cond", got["cond"], r["cond"], r["cond_tol"])
    return rep


RMS_CASES = {
    "d5120_m128_s6": lambda: gen_rms(128, 5120, 6, 0, 0, 1e-6, 21),
    "d5120_m33_s7_bias_eps": lambda: gen_rms(33, 5120, 7, 1, 0, 5e-2, 22),
    "d5120_m1_s13_bf16": lambda: gen_rms(1, 5120, 13, 0, 1, 1e-6, 23, hidden=1),
    "d5120_m40_s1_fp8": lambda: gen_rms(40, 5120, 1, 0, 0, 1e-6, 24, fp8=1),
    "d5120_m9_s0_fp8_bf16": lambda: gen_rms(9, 5120, 0, 0, 1, 1e-6, 25, fp8=1),
    "d5120_m128_final_step2": lambda: gen_rms(128, 5120, 6, 0, 0, 1e-6, 26, hidden=1, cond=1, P=64, step=2, a_frag=0),
    "d8192_m5_nopend": lambda: gen_rms(5, 8192, -1, 0, 0, 1e-6, 27, hidden=1),
    "d256_m37_s1_bias_bf16": lambda: gen_rms(37, 256, 1, 1, 1, 5e-2, 28, hidden=1, cond=1, P=16, step=1),
    "d768_m12_s0_cond_step0": lambda: gen_rms(12, 768, 0, 0, 0, 1e-5, 29, cond=1, P=4, step=0),
    "d1280_m3_s6_last_step": lambda: gen_rms(3, 1280, 6, 0, 1, 1e-6, 30, cond=1, P=1, step=63, hidden=1),
}


# ---------------------------------------------------------------------------------------------------------------------------------
# swiglu_rows:  act = bf16( bf16(silu(bf16 gate)) * bf16 up )
SWIGLU_FAULTS = ("no_bfr_silu", "no_bfr_branch", "drop_last_slab", "drop_bias", "plain_columns", "up_is_gate")


def gen_swiglu(M, F, S, bias, interleaved, threads, seed):
    g = torch.Generator().manual_seed(seed)
    rows = (M + 31) // 32 * 32
    up, b = gen_linear(g, S, bias, rows, 2 * F, M, scale=1.5)
    return case(M=M, F=F, S=S, up=up, bias=b, interleaved=interleaved, threads=threads, rows=rows)


def ref_swiglu(c, dtype=torch.float64, fault=None):
    F_ = c.F
    v, v_tol, vb = linear_out(c.up, c.bias, c.S, c.M, dtype, fault)
    if fault == "no_bfr_branch": vb = v
    f = torch.arange(F_, device=v.device)
    if c.interleaved and fault != "plain_columns":
        cg = (f >> 4) * 32 + (f & 15)
        cu = cg + 16
    else:
        cg, cu = f, F_ + f
    if fault == "up_is_gate": cu = cg
    gt, up = vb[:, cg], vb[:, cu]
    s = gt * torch.sigmoid(gt)
    sb = s if fault == "no_bfr_silu" else bfr(s)
    o = sb * up
    tol = up.abs() * (ulp_bf16(s).to(dtype) + 8 * F32 * s.abs() + 1.1 * (ulp_bf16(gt).to(dtype) + v_tol[:, cg])) \
        + sb.abs() * (ulp_bf16(up).to(dtype) + v_tol[:, cu])
    return dict(o=o, o_tol=tol)


def impl_swiglu(c, dtype, fault=None):
    return dict(act=ref_swiglu(c, dtype, fault)["o"].to(BF16))


def judge_swiglu(c, got, what):
    rep = Report(what)
    r = ref_swiglu(c)
    rep.bf16("act", got["act"], r["o"], r["o_tol"])
    return rep


SWIGLU_CASES = {
    "f13824_m5_s2_il_t512": lambda: gen_swiglu(5, 13824, 2, 1, 1, 512, 41),          # F / 8 = 1728 > 512: the column loop iterates
    "f8208_m32_s1_plain_t1024": lambda: gen_swiglu(32, 8208, 1, 0, 0, 1024, 42),      # F / 8 = 1026 > 1024
    "f13824_m33_s7_il_t1024": lambda: gen_swiglu(33, 13824, 7, 1, 1, 1024, 43),
    "f256_m1_s13_il_t512": lambda: gen_swiglu(1, 256, 13, 1, 1, 512, 44),
    "f3072_m12_s0_plain_t512": lambda: gen_swiglu(12, 3072, 0, 0, 0, 512, 45),
    "f4096_m128_s6_plain_t512": lambda: gen_swiglu(128, 4096, 6, 1, 0, 512, 46),
}


# ---------------------------------------------------------------------------------------------------------------------------------
# qkv_post (Qwen3): q / k head RMSNorm (bf16 in -> bf16 out), RoPE (fp32 tables: fp32 products, one rounding; bf16 tables: every op
# rounds), K appended at [seq][kvh][kv_len + p][128], V at [seq][kvh][128][kv_len + p]
QKV_FAULTS = ("no_bfr_branch", "no_bfr_inner", "no_bfr_norm", "eps10", "drop_last_slab", "drop_bias", "rope_pos1", "rotate_sign",
              "k_pos1", "v_untransposed", "swap_heads", "no_bfr_rope_mul")


def gen_qkv_post(nseq, P, nh, nkv, Lmax, kv, S, bias, rope_bf16, eps, seed):
    g = torch.Generator().manual_seed(seed)
    M = nseq * P
    rows = (M + 31) // 32 * 32
    N = (nh + 2 * nkv) * 128
    f = small_rows(M, eps, var=1.0) if not bias else None
    qkv, b = gen_linear(g, S, bias, rows, N, M, row_scale=f)
    qn = (1 + 0.3 * torch.randn(128, generator=g)).to(BF16)
    kn = (1 + 0.3 * torch.randn(128, generator=g)).to(BF16)
    ang = 0.3 + torch.rand(Lmax + 1, 128, generator=g) * (2 * math.pi - 0.6)  # an angle per (position, channel), none near 0
    k0 = torch.randn(nseq, nkv, Lmax, 128, generator=g).to(BF16)               # what the caches hold before the call
    v0 = torch.randn(nseq, nkv, 128, Lmax, generator=g).to(BF16)
    return case(nseq=nseq, P=P, nh=nh, nkv=nkv, Lmax=Lmax, kv=list(kv), S=S, qkv=qkv, bias=b, qn=qn, kn=kn, cos=ang.cos(), sin=ang.sin(),
                k0=k0, v0=v0, rope_bf16=rope_bf16, eps=eps, M=M, rows=rows)


def _positions(c, dev, shift=0):
    m = torch.arange(c.M, device=dev)
    return torch.tensor(c.kv, device=dev)[m // c.P] + m % c.P + shift


def ref_qkv_post(c, dtype=torch.float64, fault=None):
    """-> q [M, nh, 128], k [M, nkv, 128], v [M, nkv, 128] (unrounded) and their tols."""
    M, nh, nkv = c.M, c.nh, c.nkv
    eps = c.eps * (10 if fault == "eps10" else 1)
    x, x_tol, xb = linear_out(c.qkv, c.bias, c.S, M, dtype, fault)
    if fault == "no_bfr_branch": xb = x
    x, x_tol, xb = (t.view(M, nh + 2 * nkv, 128) for t in (x, x_tol, xb))
    qk = xb[:, :nh + nkv]
    rs = ((qk * qk).mean(-1, keepdim=True) + eps).rsqrt()
    inner = qk * rs
    ib = inner if fault == "no_bfr_inner" else bfr(inner)
    w = torch.cat([c.qn.to(dtype).expand(nh, 128), c.kn.to(dtype).expand(nkv, 128)])
    xn = w * ib
    xnb = xn if fault == "no_bfr_norm" else bfr(xn)
    # spacing of the two intermediates and of the Linear output, carried to xn
    t_xn = ulp_bf16(xn).to(dtype) + w.abs() * (ulp_bf16(inner).to(dtype) + inner.abs() * gamma(128) + rs * (ulp_bf16(x[:, :nh + nkv]).to(dtype) + x_tol[:, :nh + nkv]))
    pos = _positions(c, xb.device, 1 if fault == "rope_pos1" else 0)
    cs, sn = c.cos.to(dtype)[pos][:, None], c.sin.to(dtype)[pos][:, None]
    sg = -1.0 if fault == "rotate_sign" else 1.0
    rot = torch.cat([-sg * xnb[..., 64:], sg * xnb[..., :64]], -1)
    t_rot = torch.cat([t_xn[..., 64:], t_xn[..., :64]], -1)
    if c.rope_bf16:
        cs, sn = bfr(cs), bfr(sn)
        a, b = xnb * cs, rot * sn
        y = (a + b) if fault == "no_bfr_rope_mul" else (bfr(a) + bfr(b))
        y_tol = cs.abs() * t_xn + sn.abs() * t_rot + ulp_bf16(a).to(dtype) + ulp_bf16(b).to(dtype)
    else:
        y = xnb * cs + rot * sn
        y_tol = cs.abs() * t_xn + sn.abs() * t_rot + 4 * F32 * ((xnb * cs).abs() + (rot * sn).abs())
    q, k = y[:, :nh], y[:, nh:]
    if fault == "swap_heads" and nh > 1:
        q = torch.cat([q[:, 1:2], q[:, 0:1], q[:, 2:]], 1)
    return dict(q=q, q_tol=y_tol[:, :nh], k=k, k_tol=y_tol[:, nh:], v=x[:, nh + nkv:], v_tol=x_tol[:, nh + nkv:])


def _cache_rows(c, dev):
    """Index tensors (seq, pos) of the appended rows, row m of the block."""
    m = torch.arange(c.M, device=dev)
    return m // c.P, _positions(c, dev)


def impl_qkv_post(c, dtype, fault=None):
    r = ref_qkv_post(c, dtype, fault)
    dev = r["q"].device
    K, VT = c.k0.clone(), c.v0.clone()
    seq = torch.arange(c.M, device=dev) // c.P
    pos = _positions(c, dev, 1 if fault == "k_pos1" else 0).clamp_max(c.Lmax - 1)
    K[seq, :, pos] = r["k"].to(BF16)
    pos = _positions(c, dev)
    if fault == "v_untransposed":
        flat = VT.view(c.nseq, c.nkv, c.Lmax, 128)
        flat[seq, :, pos] = r["v"].to(BF16)
    else:
        VT[seq, :, :, pos] = r["v"].to(BF16)
    return dict(q=r["q"].to(BF16).reshape(c.M, c.nh * 128), K=K, VT=VT)


def judge_qkv_post(c, got, what):
    rep = Report(what)
    r = ref_qkv_post(c)
    dev = got["q"].device
    rep.bf16("q", got["q"].view(c.M, c.nh, 128), r["q"], r["q_tol"])
    seq, pos = _cache_rows(c, dev)
    rep.bf16("k", got["K"][seq, :, pos], r["k"], r["k_tol"])
    rep.bf16("v", got["VT"][seq, :, :, pos], r["v"], r["v_tol"])
    new = torch.zeros(c.nseq, c.Lmax, dtype=torch.bool, device=dev)
    new[seq, pos] = True
    keep = ~new
    rep.equal("K outside the appended rows", got["K"].transpose(1, 2)[keep], c.k0.transpose(1, 2)[keep])
    rep.equal("V^T outside the appended rows", got["VT"].permute(0, 3, 1, 2)[keep], c.v0.permute(0, 3, 1, 2)[keep])
    return rep


QKV_CASES = {
    "nh40_nkv8_p64_s2_bias": lambda: gen_qkv_post(2, 64, 40, 8, 256, [0, 192], 2, 1, 0, 1e-6, 51),
    "nh5_nkv1_p16_s0": lambda: gen_qkv_post(3, 16, 5, 1, 128, [0, 7, 112], 0, 0, 0, 1e-6, 52),                 # 7 slots: not a multiple of 4
    "nh4_nkv2_p1_s7_bf16": lambda: gen_qkv_post(5, 1, 4, 2, 64, [63, 0, 5, 62, 31], 7, 0, 1, 1e-6, 53),
    "nh2_nkv1_p4_s13_bias_bf16": lambda: gen_qkv_post(1, 4, 2, 1, 64, [60], 13, 1, 1, 5e-2, 54),
    "nh10_nkv2_p64_s6_prefill": lambda: gen_qkv_post(3, 64, 10, 2, 192, [128, 0, 37], 6, 0, 1, 1e-6, 55),
    "nh3_nkv3_p7_s1": lambda: gen_qkv_post(4, 7, 3, 3, 64, [0, 57, 1, 30], 1, 1, 0, 1e-2, 56),
}


# ---------------------------------------------------------------------------------------------------------------------------------
# head_final: pending update, LN (no affine) * bf16(1 + scale) + shift -> bf16, Linear(D -> C) -> bf16, [2 sigmoid - 1 in bf16 ops],
# then the fp32 sampler step (sampling_x.py:77-95), sign, token scatter, the next evaluation's input projection
HF_FAULTS = ("no_bfr_branch", "no_bfr_gated", "no_bfr_resid", "no_bfr_1p_scale", "round_after_mul", "no_bfr_h", "no_bfr_lin",
             "no_bfr_sigmoid", "eps10", "swap_gate_scale", "swap_gate_shift", "swap_scale_shift", "drop_last_slab",
             "drop_bias", "swap_cfg_rows", "tok_prev_step", "uncond_reads_cond_row")


def gen_head_final(BP, P, D, C, cfg_mult, sigmoid, is_final, step, S, bias, offs, ada_ld, eps, seed, cfg_table=0, x_next=0, tok_branches=1,
                   T=None, n_evals=4, eval_index=1):
    g = torch.Generator().manual_seed(seed)
    M = cfg_mult * BP
    rows = (M + 31) // 32 * 32
    f = small_rows(M, eps)
    go, so, fo = offs
    ada = (torch.randn(M, ada_ld, generator=g) * 0.5).to(BF16)
    ada[:, go:go + D] = (torch.randn(M, D, generator=g) * f).to(BF16)
    X = (torch.randn(M, D, generator=g) * f).to(BF16)
    pend, b = gen_linear(g, S, bias, rows, D, M)
    # |logits| < 4: h ~ N(0, ~1.3), lin_w ~ N(0, 1 / D) -> logits ~ N(0, ~1.3)
    lin_w = (torch.randn(C, D, generator=g) * 0.8 / math.sqrt(D)).to(BF16)
    lin_b = (torch.randn(C, generator=g) * 0.3).to(BF16)
    xt = torch.randn(BP, C, generator=g)
    T = T or (step + 1) * P
    noise = torch.randn(step + 1, n_evals, BP, C, generator=g)
    t = 0.35
    sc = torch.tensor([t, 0.1, max(1 - t, 0.05), 0.37, 1 - t, 0.21, 2.5], dtype=torch.float32)
    table = (1.0 + 0.5 * torch.arange(step + 2, dtype=torch.float32)) if cfg_table else None
    in_w = (torch.randn(D, C, generator=g) / math.sqrt(C)).to(BF16) if x_next else None
    in_b = (torch.randn(D, generator=g) * 0.3).to(BF16) if x_next else None
    return case(BP=BP, P=P, D=D, C=C, cfg_mult=cfg_mult, sigmoid=sigmoid, is_final=is_final, step=step, S=S, X=X, pend=pend, bias=b,
                ada=ada, ada_ld=ada_ld, offs=offs, lin_w=lin_w, lin_b=lin_b, xt=xt, noise=noise, sc=sc, cfg_table=table, in_w=in_w,
                in_b=in_b, tok_branches=tok_branches, T=T, n_evals=n_evals, eval_index=eval_index, eps=eps, M=M, rows=rows, x_next=x_next,
                ln_w=None, ln_b=None)


def ref_head_final_xhat(c, dtype=torch.float64, fault=None):
    r = ref_ln_mod(c, dtype, fault)                                # the same pending update + modulation (no affine)
    h, D = r["h"], c.D
    if fault == "uncond_reads_cond_row" and c.cfg_mult == 2:
        h = torch.cat([h[:c.BP], h[:c.BP]])
    hb = h if fault == "no_bfr_h" else bfr(h)
    w = c.lin_w.to(dtype)
    o = hb @ w.t() + c.lin_b.to(dtype)
    hw = hb.abs() @ w.abs().t()
    # h itself may sit one spacing off (its own tol, and the residual's): allow eight such elements per row, each moving the dot by
    # at most U max|h w|
    o_tol = gamma(D) * hw + 8 * U * (hb.abs().amax(-1, keepdim=True) * w.abs().amax(-1)[None, :])
    ob = o if fault == "no_bfr_lin" else bfr(o)
    if not c.sigmoid:
        return dict(xhat=o, xhat_tol=o_tol)
    s = torch.sigmoid(ob)
    sb = s if fault == "no_bfr_sigmoid" else bfr(s)
    xv = 2 * sb - 1                                                # (2 * bf16 is exact: the kernel's rounding of it changes nothing)
    tol = 2 * (ulp_bf16(s).to(dtype) + 0.25 * (ulp_bf16(o).to(dtype) + o_tol) + 8 * F32)
    return dict(xhat=xv, xhat_tol=tol)


def sampler_step(c, xhat, fault=None):
    """The fp32 sampler update, op for op (head_final_kernel), from an x_hat [cfg_mult * BP, C] fp32.  CPU tensors."""
    t, dt, den, var, omt, ns, cfg = (c.sc[i] for i in range(7))
    x = c.xt.clone()
    xh = xhat.float().view(c.cfg_mult, c.BP, c.C)
    if fault == "swap_cfg_rows" and c.cfg_mult == 2:
        xh = xh.flip(0)
    v = (xh[0] - x) / den
    if c.cfg_mult == 2:
        vu = (xh[1] - x) / den
        if c.cfg_table is not None:
            cfg = c.cfg_table[c.step]
        v = vu + cfg * (v - vu)
    out = {}
    if not c.is_final:
        score = (t * v - x) / var
        drift = v + omt * score
        xn = x + drift * dt + ns * c.noise[c.step, c.eval_index + 1]
    else:
        xn = x + v * dt
        out["pred"] = xn
        sg = torch.sign(xn)
        out["tok_cur"] = sg.expand(c.tok_branches, c.BP, c.C).contiguous()
        ta = torch.full((c.BP // c.P, c.T, c.C), float("nan"))
        step = c.step - (1 if fault == "tok_prev_step" else 0)
        ta[:, step * c.P:(step + 1) * c.P] = sg.view(c.BP // c.P, c.P, c.C)
        out["tok_all"] = ta
    out["xt"] = xn
    return out


def ref_x_next(c, xt_new, dtype=torch.float64):
    """x0 = bf16(input_proj(bf16(x_t))) of the next evaluation, both CFG rows; a C-term fp32 dot."""
    xb = bfr(xt_new.to(dtype))
    w = c.in_w.to(dtype)
    v = xb @ w.t() + c.in_b.to(dtype)
    tol = gamma(c.C) * (xb.abs() @ w.abs().t() + c.in_b.to(dtype).abs())
    return v.repeat(c.cfg_mult, 1), tol.repeat(c.cfg_mult, 1)


def impl_head_final(c, dtype, fault=None):
    r = ref_head_final_xhat(c, dtype, fault)
    xhat = bfr(r["xhat"]).float().cpu()
    cc = to_device(c, "cpu")
    got = dict(xhat=xhat, **sampler_step(cc, xhat, fault))
    if c.x_next and not c.is_final:
        got["X_next"] = ref_x_next(cc, got["xt"], dtype)[0].to(BF16)
    return got


def judge_head_final(c, got, what):
    """got: CPU tensors.  x_hat under (a) / (b); the sampler outputs bit for bit from the implementation's own x_hat; X_next (a
    C-term fp32 dot whose summation order torch does not reproduce) under (a) / (b) from the implementation's own new x_t."""
    rep = Report(what)
    r = ref_head_final_xhat(c)
    rep.bf16("xhat", got["xhat"].to(r["xhat"].device), r["xhat"], r["xhat_tol"])
    cc = to_device(c, "cpu")
    want = sampler_step(cc, got["xhat"].cpu())
    for k, v in want.items():
        a, b = got[k].cpu(), v
        if k == "tok_all":                                         # NaN = untouched
            rep.equal(k + " (written set)", torch.isnan(a), torch.isnan(b))
            a, b = a.nan_to_num(7.0), b.nan_to_num(7.0)
        rep.equal(k, a, b)
    if c.x_next and not c.is_final:
        v, tol = ref_x_next(cc, got["xt"].cpu())
        rep.bf16("X_next", got["X_next"].cpu(), v, tol)
    return rep


HF_CASES = {
    "d5120_c32_bp64_cfg2_sig_mid": lambda: gen_head_final(64, 64, 5120, 32, 2, 1, 0, 0, 6, 1, (0, 5120, 10240), _A6, 1e-6, 61, x_next=1),
    "d5120_c16_bp16_cfg2_sig_final_step2": lambda: gen_head_final(16, 16, 5120, 16, 2, 1, 1, 2, 7, 1, (25600, 20480, 15360), _A6, 1e-6, 62,
                                                                  cfg_table=1, T=64),
    "d5120_c32_bp1_cfg1_sig_final_last": lambda: gen_head_final(1, 1, 5120, 32, 1, 1, 1, 5, 13, 0, (5120, 0, 10240), _A6, 1e-6, 63, T=6),
    "d768_c16_bp40_cfg2_nosig_mid_table": lambda: gen_head_final(40, 4, 768, 16, 2, 0, 0, 1, 1, 1, (768, 1536, 0), 6 * 768, 1e-5, 64,
                                                                 cfg_table=1, x_next=1),
    "d1024_c16_bp60_cfg2_nosig_final_br2": lambda: gen_head_final(60, 4, 1024, 16, 2, 0, 1, 1, 0, 0, (0, 2048, 1024), 6 * 1024, 1e-6, 65,
                                                                  tok_branches=2, T=12),
    "d1280_c32_bp33_cfg1_nosig_mid": lambda: gen_head_final(33, 1, 1280, 32, 1, 0, 0, 0, -1, 0, (2560, 1280, 0), 3 * 1280, 1e-2, 66, x_next=1),
    "d256_c7_bp100_cfg2_sig_mid": lambda: gen_head_final(100, 5, 256, 7, 2, 1, 0, 3, 2, 1, (8, 264, 520), 1024, 1e-6, 67),
}


# ---------------------------------------------------------------------------------------------------------------------------------
# DiT head attention over one patch of P tokens (no cache, non-causal).  P = 64: fp32 scores, un-normalised bf16 P, fp32
# accumulation, one output rounding (the bound of test_gpu_attn's tol_llm with L = 64).  P <= 16: q * scale in bf16, bf16 scores,
# fp32 softmax, bf16 P = e / sum, one output rounding (tol_in).  q / k / v are built on a grid (multiples of 2^-6 below 4) and split
# into slabs whose sum is exact in any order, so the Linear rounding in front of the attention is exact and every q . k is exact in fp32.
RMS_QW = 2 * math.sqrt(2 / 3) * U
RMS_IN = 2 * math.sqrt(1 / 3) * U
ATTN_FAULTS = ("drop_key", "swap_heads", "swap_keys", "swap_seqs")


def split_exact(g, T, S, bias):
    """Slabs [S][rows][N] fp32 and a bf16 bias whose sum is exactly T (all terms on the grid 2^-6, far below 2^24 grid steps)."""
    if S == 0:
        return T.to(BF16), None
    b = (torch.randint(-32, 33, (T.shape[1],), generator=g).float() / 64).to(BF16) if bias else None
    parts = [torch.randint(-128, 129, T.shape, generator=g).float() / 64 for _ in range(S - 1)]
    first = T - sum(parts) if parts else T.clone()
    if b is not None:
        first = first - b.float()
    return torch.stack([first] + parts), b


def gen_head_attn(nseq, nhead, P, dh, S, bias, probe, seed):
    g = torch.Generator().manual_seed(seed)
    M, D = nseq * P, nhead * dh
    rows = (M + 31) // 32 * 32
    grid = lambda t, lim: (torch.round(t * 64).clamp(-lim * 64 + 1, lim * 64 - 1) / 64)
    if probe:
        # integer scores: q = 8 e_G + 8 a e_A, k_G graded per (key, head, sequence), k_A = b, noise in the channels q does not read;
        # V one-hot: channel j of the output spells the weight of key j
        cg, ca = 93 % dh, 7
        j = torch.arange(P)
        q = torch.zeros(nseq, P, nhead, dh)
        q[..., cg] = 8.0
        q[..., ca] = 8.0 * torch.randint(-1, 2, (nseq, P, nhead), generator=g).float()
        k = grid(torch.randn(nseq, P, nhead, dh, generator=g), 4)
        grade = (j[None, :, None] * 5 + j[None, :, None] // 8 + 3 * torch.arange(nhead)[None, None, :] + 5 * torch.arange(nseq)[:, None, None]) % 8
        k[..., cg] = 16.0 - grade.float()
        k[..., ca] = torch.randint(-1, 2, (nseq, P, nhead), generator=g).float()
        v = torch.zeros(nseq, P, nhead, dh)
        v[:, j, :, j] = 1.0
    else:
        if P == 64:
            q = grid(torch.randn(nseq, P, nhead, dh, generator=g) * 1.5, 4)
        elif dh == 128:   # one binade: bf16(q * 128^-0.5) then lies on the grid 2^-11 below 0.18, every product sum is exact in fp32
            q = (1 + torch.randint(0, 64, (nseq, P, nhead, dh), generator=g).float() / 64) * (torch.randint(0, 2, (nseq, P, nhead, dh), generator=g) * 2 - 1)
        else:
            q = grid(torch.randn(nseq, P, nhead, dh, generator=g) * 1.5, 4)
        k = torch.round(torch.randn(nseq, P, nhead, dh, generator=g) * 8).clamp(-31, 31) / 8
        v = grid(torch.randn(nseq, P, nhead, dh, generator=g), 4)
    T = torch.cat([t.reshape(M, D) for t in (q, k, v)], 1)
    T = torch.cat([T, torch.zeros(rows - M, 3 * D)])
    qkv, b = split_exact(g, T, S, bias)
    return case(nseq=nseq, nhead=nhead, P=P, dh=dh, S=S, qkv=qkv, bias=b, T=T[:M].to(BF16), M=M, D=D, rows=rows, probe=probe)


def ref_head_attn(c, dtype=torch.float64, fault=None):
    """-> (out, A) [M, nhead, dh]: attention output and sum_j w_j |v_j|."""
    T = c.T.to(dtype)
    D, dh, P = c.D, c.dh, c.P
    q, k, v = (T[:, i * D:(i + 1) * D].view(c.nseq, P, c.nhead, dh).permute(0, 2, 1, 3) for i in range(3))   # [s, h, P, dh]
    if fault == "swap_heads":                                      # the keys / values of head 1 under the queries of head 0
        k, v = (torch.cat([t[:, 1:2], t[:, 0:1], t[:, 2:]], 1) for t in (k, v))
    if fault == "swap_seqs":
        k, v = (torch.cat([t[1:2], t[0:1], t[2:]], 0) for t in (k, v))
    if fault == "swap_keys" and P > 1:
        idx = torch.arange(P, device=T.device)
        idx = torch.where(idx % 16 == 4, idx + 4, torch.where(idx % 16 == 8, idx - 4, idx)) if P >= 16 else idx.flip(0)
        v = v[:, :, idx]
    scale = dh ** -0.5
    if P == 64:
        s = (q @ k.transpose(-1, -2)) * torch.tensor(scale, dtype=torch.float32).to(dtype)
    else:
        qs = bfr(q * torch.tensor(0.125 if dh == 64 else 0.08838834764831845, dtype=torch.float32).to(dtype))
        s = qs @ k.transpose(-1, -2)
        s = bfr(s)
    if fault == "drop_key":
        s[..., P - 1] = float("-inf")
    e = torch.exp(s - s.amax(-1, keepdim=True))
    w = e / e.sum(-1, keepdim=True)
    if P <= 16:
        w = bfr(w)
    o, A = w @ v, w @ v.abs()
    back = lambda t: t.permute(0, 2, 1, 3).reshape(c.M, c.nhead, dh)
    return back(o), back(A)


def tol_head_attn(c, ref, A):
    if c.P == 64:
        return 1.01 * U * (A + ref.abs()) + 64 * F32 * A + 1e-6                 # tol_llm, L = 64
    return 2 * U * A + 1.01 * U * ref.abs() + c.P * F32 * A + 1e-6              # tol_in


def impl_head_attn(c, dtype, fault=None):
    return dict(o=ref_head_attn(c, dtype, fault)[0].to(BF16))


def judge_head_attn(c, got, what):
    rep = Report(what)
    ref, A = ref_head_attn(c)
    g = got["o"].double().view(c.M, c.nhead, c.dh)
    tol = tol_head_attn(c, ref, A)
    if not torch.isfinite(g).all():
        rep.fail.append(f"{what}: non-finite output")
        return rep
    ex = (g - ref).abs() - tol
    rep.excess = (ex / tol).max().item()                           # in units of the tolerance here
    if ex.max() > 0:
        rep._worst("o", ex, g, ref, tol)
    rr = ((g - ref).norm() / ref.norm()).item()
    rep.flip = rr                                                  # (reported: the relative rms)
    bound = RMS_QW if c.P == 64 else RMS_IN
    if not c.probe and rr > bound:
        rep.fail.append(f"{what}: relative rms {rr:.3e} above {bound:.3e}")
    return rep


ATTN_CASES = {
    # (nseq, nhead, P, dh, S, bias, probe)
    "p64_probe_slabs": lambda: gen_head_attn(3, 5, 64, 128, 2, 1, 1, 71),
    "p64_probe_finished": lambda: gen_head_attn(2, 3, 64, 128, 0, 0, 1, 72),
    "p64_random_nh40_s3": lambda: gen_head_attn(2, 40, 64, 128, 3, 1, 0, 73),
    "p64_random_finished": lambda: gen_head_attn(3, 8, 64, 128, 0, 0, 0, 74),
    "p16_mfma128_probe_tail": lambda: gen_head_attn(3, 5, 16, 128, 0, 0, 1, 75),       # 15 (sequence, head) pairs: the last workgroup's tail wave returns
    "p16_mfma128_random_nh40": lambda: gen_head_attn(5, 40, 16, 128, 0, 0, 0, 76),
    "p16_mfma64_probe_tail": lambda: gen_head_attn(7, 3, 16, 64, 0, 0, 1, 77),         # 21 pairs
    "p16_mfma64_random_nh12": lambda: gen_head_attn(9, 12, 16, 64, 0, 0, 0, 78),
    "p16_slabs128_probe": lambda: gen_head_attn(3, 5, 16, 128, 2, 1, 1, 79),
    "p16_slabs128_random": lambda: gen_head_attn(4, 40, 16, 128, 7, 1, 0, 80),
    "p16_slabs64_random": lambda: gen_head_attn(3, 12, 16, 64, 1, 0, 0, 81),
    "p4_dh64_probe": lambda: gen_head_attn(5, 3, 4, 64, 0, 0, 1, 82),
    "p4_dh64_random_slabs": lambda: gen_head_attn(9, 12, 4, 64, 6, 1, 0, 83),
    "p4_dh128_random": lambda: gen_head_attn(3, 5, 4, 128, 0, 0, 0, 84),
    "p1_dh64_random": lambda: gen_head_attn(7, 12, 1, 64, 0, 0, 0, 85),
    "p1_dh128_slabs": lambda: gen_head_attn(33, 5, 1, 128, 2, 1, 0, 86),
}


def head_attn_form(c):
    """The kernel bdk_head_attn picks (host rule): P 64 -> head_attn_kernel; P 16 from a finished bf16 tensor -> the matrix-pipe
    form of that head_dim; every other P <= 16 -> head_attn16_kernel."""
    if c.P == 64:
        return "head_attn"
    return f"head_attn16_mfma<{c.dh}>" if (c.P == 16 and c.S == 0) else "head_attn16"


# ---------------------------------------------------------------------------------------------------------------------------------
# ImageNet transformer rows: nn.RMSNorm on a bf16 residual stream held in fp32 storage (fp32 weight, ONE rounding), interleaved-pair
# RoPE, q pre-scaled by 64^-0.5
INRMS_FAULTS = ("no_bfr_branch", "no_bfr_resid", "no_bfr_norm", "eps10", "drop_last_slab", "drop_bias", "pos_prev_step", "pos_next_row",
                "add_R_on_init")


def gen_in_rms(M, D, S, bias, init_from_pend, renorm, f32_stream, eps, seed, hidden=0, cond=0, P=1, step=0):
    g = torch.Generator().manual_seed(seed)
    rows = (M + 31) // 32 * 32
    f = small_rows(M, eps) if not bias else None
    R = torch.randn(M, D, generator=g) * (f if f is not None else 1.0)
    if not f32_stream:
        R = R.to(BF16).float()
    pend, b = gen_linear(g, S, bias, rows, D, M, row_scale=f)
    w = 1 + 0.3 * torch.randn(D, generator=g)
    pos = torch.randn((step + 1) * P + 1, D, generator=g) if cond else None
    return case(M=M, D=D, S=S, R=R, pend=pend, bias=b, w=w, eps=eps, init=init_from_pend, renorm=renorm, f32_stream=f32_stream,
                hidden=hidden, cond=cond, P=P, step=step, pos=pos, rows=rows)


def ref_in_rms(c, dtype=torch.float64, fault=None, X=None):
    """X: the implementation's own summed stream (stage 2); else computed from R and the pending branch."""
    M, D = c.M, c.D
    eps = c.eps * (10 if fault == "eps10" else 1)
    out = dict(x=None)
    if X is not None:
        x = X[:M].to(dtype)
    elif c.S >= 0:
        o, o_tol, ob = linear_out(c.pend, c.bias, c.S, M, dtype, fault)
        if fault == "no_bfr_branch": ob = o
        if c.init and fault != "add_R_on_init":
            xs, x = o, ob
            out["x"], out["x_tol"], out["x_kind"] = o, o_tol, "bf16"
        else:
            xs = c.R[:M].to(dtype) + ob
            x = xs if (c.f32_stream or fault == "no_bfr_resid") else bfr(xs)
            out["x"], out["x_tol"] = xs, ulp_bf16(o).to(dtype) + o_tol + 2 * F32 * xs.abs()
            out["x_tight"] = 2 * F32 * xs.abs()
            out["x_kind"] = "f32" if c.f32_stream else "bf16"
    else:
        x = c.R[:M].to(dtype)
    out["xin"] = x
    rs = ((x * x).mean(-1, keepdim=True) + eps).rsqrt()
    n = x * rs * c.w.to(dtype)
    out["n"], out["n_tol"] = n, n.abs() * (gamma(D) + 4 * F32)
    nb = n if (c.f32_stream or fault == "no_bfr_norm") else bfr(n)
    out["nb"] = nb
    if c.cond:
        step = c.step - (1 if fault == "pos_prev_step" else 0)
        idx = step * c.P + torch.arange(M, device=x.device) % c.P + (1 if fault == "pos_next_row" else 0)
        pe = c.pos.to(dtype)[idx]
        out["cond"] = nb + pe
        out["cond_tol"] = out["n_tol"] + (0 if c.f32_stream else ulp_bf16(n).to(dtype)) + 2 * F32 * (nb + pe).abs()
    return out


def impl_in_rms(c, dtype, fault=None):
    r = ref_in_rms(c, dtype, fault)
    nb = r["nb"]
    got = dict(a=r["n"].to(BF16))
    writes_x = (not c.renorm) and c.S >= 0
    got["R"] = nb.float() if c.renorm else (r["xin"].float() if writes_x else c.R[:c.M].clone())
    if c.hidden:
        got["hidden"] = nb.float()
    if c.cond:
        got["cond"] = r["cond"].to(BF16)
    return got


def judge_in_rms(c, got, what):
    """Without renorm_to_R the kernel writes the summed stream back: checked, then the norm is computed from that copy.  With
    renorm_to_R (and a pending branch) the sum is not visible, so its spacing is carried into the tol of the normalised value."""
    rep = Report(what)
    r1 = ref_in_rms(c)
    staged = (not c.renorm) and c.S >= 0
    if staged:
        if r1["x_kind"] == "f32":
            rep.f32("R", got["R"], r1["x"], r1["x_tol"], r1["x_tight"])
        else:
            rep.bf16("R", got["R"], r1["x"], r1["x_tol"])
        r = ref_in_rms(c, X=got["R"])
        extra = 0
    else:
        if not c.renorm:
            rep.equal("R", got["R"], c.R[:c.M])
        r = r1
        extra = 0
        if c.S >= 0:                                               # d n / d x = rs w, one spacing of x (or of the branch)
            x = r1["xin"]
            rs = ((x * x).mean(-1, keepdim=True) + c.eps).rsqrt()
            extra = rs * c.w.double().abs() * ((0 if c.f32_stream and not c.init else ulp_bf16(x)) + r1["x_tol"])
    n_tol = r["n_tol"] + extra
    if c.f32_stream:
        rep.bf16("a", got["a"], r["n"], n_tol)
        if c.renorm: rep.f32("R", got["R"], r["n"], n_tol)
        if c.hidden: rep.f32("hidden", got["hidden"], r["n"], n_tol)
    else:
        rep.bf16("a", got["a"], r["n"], n_tol)
        if c.renorm: rep.bf16("R", got["R"], r["n"], n_tol)
        if c.hidden: rep.bf16("hidden", got["hidden"], r["n"], n_tol)
    if c.cond:
        rep.bf16("cond", got["cond"], r["cond"], r["cond_tol"] + extra)
    return rep


INRMS_CASES = {
    "d768_m203_s6": lambda: gen_in_rms(203, 768, 6, 0, 0, 0, 0, 1e-6, 91),
    "d1024_m33_s7_bias_init": lambda: gen_in_rms(33, 1024, 7, 1, 1, 0, 0, 5e-2, 92),
    "d1280_m1_s13_init_renorm": lambda: gen_in_rms(1, 1280, 13, 1, 1, 1, 0, 5e-2, 93, hidden=1),
    "d768_m40_s1_f32": lambda: gen_in_rms(40, 768, 1, 0, 0, 0, 1, 1e-6, 94, hidden=1),
    "d256_m12_s0_cond_step3": lambda: gen_in_rms(12, 256, 0, 0, 0, 0, 0, 1e-6, 95, hidden=1, cond=1, P=4, step=3),
    "d8192_m5_nopend_cond_step0": lambda: gen_in_rms(5, 8192, -1, 0, 0, 0, 0, 1e-6, 96, cond=1, P=16, step=0),
    "d1280_m64_nopend_f32_cond_last": lambda: gen_in_rms(64, 1280, -1, 0, 0, 0, 1, 1e-5, 97, cond=1, P=16, step=15, hidden=1),
}


INQKV_FAULTS = ("no_bfr_branch", "drop_last_slab", "drop_bias", "rope_pos1", "rotate_sign", "partner_lane32", "k_pos1",
                "v_pos1", "swap_heads", "no_q_scale")


def gen_in_qkv_post(nseq, P, nh, Lmax, kv, S, bias, seed):
    g = torch.Generator().manual_seed(seed)
    M, D = nseq * P, nh * 64
    rows = (M + 31) // 32 * 32
    qkv, b = gen_linear(g, S, bias, rows, 3 * D, M)
    ang = 0.3 + torch.rand(Lmax + 1, 32, generator=g) * (2 * math.pi - 0.6)
    rope = torch.stack([ang.cos(), ang.sin()], -1).contiguous()
    k0 = torch.randn(nseq, nh, Lmax, 64, generator=g).to(BF16)
    v0 = torch.randn(nseq, nh, Lmax, 64, generator=g).to(BF16)
    return case(nseq=nseq, P=P, nh=nh, Lmax=Lmax, kv=kv, S=S, qkv=qkv, bias=b, rope=rope, k0=k0, v0=v0, M=M, D=D, rows=rows)


def ref_in_qkv_post(c, dtype=torch.float64, fault=None):
    M, nh = c.M, c.nh
    x, x_tol, xb = linear_out(c.qkv, c.bias, c.S, M, dtype, fault)
    if fault == "no_bfr_branch": xb = x
    x, x_tol, xb = (t.view(M, 3, nh, 64) for t in (x, x_tol, xb))
    pos = c.kv + torch.arange(M, device=xb.device) % c.P + (1 if fault == "rope_pos1" else 0)
    cs = c.rope.to(dtype)[pos, :, 0].repeat_interleave(2, -1)[:, None, None]
    sn = c.rope.to(dtype)[pos, :, 1].repeat_interleave(2, -1)[:, None, None]
    qk = xb[:, :2]
    if fault == "partner_lane32":
        other = qk.roll(32, -1)
    else:
        other = qk.view(M, 2, nh, 32, 2).flip(-1).reshape(M, 2, nh, 64)
    sign = torch.tensor([-1.0, 1.0], dtype=dtype, device=xb.device).repeat(32) * (-1.0 if fault == "rotate_sign" else 1.0)
    y = qk * cs + sign * other * sn
    t_x = ulp_bf16(x[:, :2]).to(dtype) + x_tol[:, :2]
    t_o = t_x.view(M, 2, nh, 32, 2).flip(-1).reshape(M, 2, nh, 64)
    y_tol = cs.abs() * t_x + sn.abs() * t_o + 4 * F32 * ((qk * cs).abs() + (other * sn).abs())
    q = y[:, 0] * (1.0 if fault == "no_q_scale" else 0.125)      # bf16(y) * 0.125: the scaling is exact, one rounding
    k = y[:, 1]
    if fault == "swap_heads" and nh > 1:
        k = torch.cat([k[:, 1:2], k[:, 0:1], k[:, 2:]], 1)
    return dict(q=q, q_tol=y_tol[:, 0] * 0.125, k=k, k_tol=y_tol[:, 1], v=x[:, 2], v_tol=x_tol[:, 2])


def impl_in_qkv_post(c, dtype, fault=None):
    r = ref_in_qkv_post(c, dtype, fault)
    dev = r["q"].device
    m = torch.arange(c.M, device=dev)
    seq, p = m // c.P, c.kv + m % c.P
    K, V = c.k0.clone(), c.v0.clone()
    K[seq, :, (p + (1 if fault == "k_pos1" else 0)).clamp_max(c.Lmax - 1)] = r["k"].to(BF16)
    V[seq, :, (p + (1 if fault == "v_pos1" else 0)).clamp_max(c.Lmax - 1)] = r["v"].to(BF16)
    return dict(q=r["q"].to(BF16).reshape(c.M, c.D), K=K, V=V)


def judge_in_qkv_post(c, got, what):
    rep = Report(what)
    r = ref_in_qkv_post(c)
    dev = got["q"].device
    m = torch.arange(c.M, device=dev)
    seq, p = m // c.P, c.kv + m % c.P
    rep.bf16("q", got["q"].view(c.M, c.nh, 64), r["q"], r["q_tol"])
    rep.bf16("k", got["K"][seq, :, p], r["k"], r["k_tol"])
    rep.bf16("v", got["V"][seq, :, p], r["v"], r["v_tol"])
    keep = torch.ones(c.Lmax, dtype=torch.bool, device=dev)
    keep[c.kv:c.kv + c.P] = False
    rep.equal("K outside the appended rows", got["K"][:, :, keep], c.k0[:, :, keep])
    rep.equal("V outside the appended rows", got["V"][:, :, keep], c.v0[:, :, keep])
    return rep


INQKV_CASES = {
    "nh12_p16_s2_bias": lambda: gen_in_qkv_post(5, 16, 12, 320, 79, 2, 1, 101),
    "nh16_p4_s0_last": lambda: gen_in_qkv_post(3, 4, 16, 320, 316, 0, 0, 102),
    "nh20_p1_s7_first": lambda: gen_in_qkv_post(7, 1, 20, 64, 0, 7, 1, 103),
    "nh3_p16_s13": lambda: gen_in_qkv_post(2, 16, 3, 64, 48, 13, 0, 104),              # 9 slots: not a multiple of 4
    "nh12_p64_s1_prefill": lambda: gen_in_qkv_post(2, 64, 12, 128, 0, 1, 0, 105),
}


# ---------------------------------------------------------------------------------------------------------------------------------
# head_y_all:  y_i = bf16(silu(bf16(temb_i + cemb)))
YALL_FAULTS = ("no_bfr_sum", "temb_next_eval", "cemb_next_row")


def gen_y_all(M, D, n_evals, G, rb, fp8, seed):
    g = torch.Generator().manual_seed(seed)
    cemb = torch.randn(rb * 32 + 1, D, generator=g).to(BF16)
    temb = torch.randn(n_evals + 1, D, generator=g).to(BF16)
    return case(M=M, D=D, n_evals=n_evals, G=G, rb=rb, fp8=fp8, cemb=cemb, temb=temb)


def ref_y_all(c, dtype=torch.float64, fault=None):
    """-> y [n_evals, M, D] unrounded, tol."""
    te = c.temb.to(dtype)[(1 if fault == "temb_next_eval" else 0):][:c.n_evals]
    ce = c.cemb.to(dtype)[(1 if fault == "cemb_next_row" else 0):][:c.M]
    t = te[:, None] + ce[None]
    tb = t if fault == "no_bfr_sum" else bfr(t)
    y = tb * torch.sigmoid(tb)
    return dict(y=y, y_tol=8 * F32 * y.abs())


def impl_y_all(c, dtype, fault=None):
    r = ref_y_all(c, dtype, fault)
    if c.fp8:
        q, s = quant_rows(bfr(r["y"]).reshape(-1, c.D))
        return dict(y8=q.view(c.n_evals, c.M, c.D), scale=s.view(c.n_evals, c.M))
    return dict(y=r["y"].to(BF16))


def judge_y_all(c, got, what):
    rep = Report(what)
    r = ref_y_all(c)
    if c.fp8:
        yb = bfr(r["y"]).reshape(-1, c.D)
        rep.fp8("y8", got["y8"].reshape(-1, c.D), got["scale"].reshape(-1), yb, (r["y_tol"] + ulp_bf16(r["y"])).reshape(-1, c.D))
    else:
        rep.bf16("y", got["y"], r["y"], r["y_tol"])
    return rep


YALL_CASES = {
    "d5120_m128_e5_g1": lambda: gen_y_all(128, 5120, 5, 1, 4, 0, 111),
    "d5120_m33_e7_g4_short": lambda: gen_y_all(33, 5120, 7, 4, 2, 0, 112),             # 7 % 4 = 3 evaluations in the last group
    "d768_m40_e5_g4_short_fp8": lambda: gen_y_all(40, 768, 5, 4, 2, 1, 113),
    "d1280_m1_e3_g1_fp8": lambda: gen_y_all(1, 1280, 3, 1, 1, 1, 114),
    "d256_m12_e9_g8_short": lambda: gen_y_all(12, 256, 9, 8, 1, 0, 115),
}


LAUNCHERS = {
    "ln_mod": (LN_CASES, impl_ln_mod, judge_ln_mod, LN_FAULTS),
    "rms": (RMS_CASES, impl_rms, judge_rms, RMS_FAULTS),
    "qkv_post": (QKV_CASES, impl_qkv_post, judge_qkv_post, QKV_FAULTS),
    "head_attn": (ATTN_CASES, impl_head_attn, judge_head_attn, ATTN_FAULTS),
    "head_final": (HF_CASES, impl_head_final, judge_head_final, HF_FAULTS),
    "swiglu_rows": (SWIGLU_CASES, impl_swiglu, judge_swiglu, SWIGLU_FAULTS),
    "in_rms": (INRMS_CASES, impl_in_rms, judge_in_rms, INRMS_FAULTS),
    "in_qkv_post": (INQKV_CASES, impl_in_qkv_post, judge_in_qkv_post, INQKV_FAULTS),
    "head_y_all": (YALL_CASES, impl_y_all, judge_y_all, YALL_FAULTS),
}


def applies(launcher, c, fault):
    """Whether `fault` changes what this case computes at all (a dropped bias needs a bias, a swapped head a second head ...)."""
    S = getattr(c, "S", 1)
    if fault == "drop_last_slab" or fault == "no_bfr_branch":
        return S >= 1
    if fault == "drop_bias":
        return c.bias is not None
    if fault in ("no_bfr_gated", "no_bfr_resid") and launcher in ("ln_mod", "head_final"):
        return S >= 0
    if fault == "eps10" and launcher in ("rms", "qkv_post", "in_rms"):
        return c.bias is None or c.eps >= 1e-2                     # (rows of small variance, or an eps that matters against variance 1)
    if launcher == "rms":
        if fault == "no_bfr_resid": return bool(c.bf16_stream) and S >= 0
        if fault == "no_bfr_inner": return bool(c.bf16_stream)
    if launcher == "in_rms":
        if fault == "no_bfr_resid": return S >= 0 and not c.f32_stream and not c.init
        if fault == "no_bfr_norm": return not c.f32_stream and bool(c.hidden or c.renorm or c.cond)
        if fault == "add_R_on_init": return bool(c.init)
    if fault in ("pos_prev_step", "pos_next_row"):
        return bool(c.cond) and (fault == "pos_next_row" or c.step > 0)
    if launcher == "qkv_post":
        if fault == "no_bfr_rope_mul": return bool(c.rope_bf16)
        if fault == "swap_heads": return c.nh > 1
    if launcher == "in_qkv_post" and fault == "swap_heads":
        return c.nh > 1
    if launcher == "head_final":
        if fault in ("no_bfr_sigmoid", "no_bfr_lin"): return bool(c.sigmoid)      # (without it the output rounding is the same one)
        if fault in ("swap_cfg_rows", "uncond_reads_cond_row"): return c.cfg_mult == 2
        if fault == "tok_prev_step": return bool(c.is_final) and c.step > 0
    if launcher == "swiglu_rows" and fault == "plain_columns":
        return bool(c.interleaved)
    if launcher == "head_attn":
        if fault in ("drop_key", "swap_keys"): return c.P > 1
        if fault == "swap_heads": return c.nhead > 1
        if fault == "swap_seqs": return c.nseq > 1
    return True
