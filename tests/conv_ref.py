"""References, input sets, bounds and the judge for tests/test_gpu_conv.py and tests/test_conv_ref_cpu.py: the tokenizer kernels of
bitdance_amd/csrc/bd_conv.hip (conv_tile_kernel, gn_stats_kernel / gn_finalize_kernel, gn_apply_kernel, tokens_to_padded_kernel).

The design is that of tests/rows_ref.py, whose `Report`, `bfr`, `gamma`, `ulp_bf16` are used here: a reference is plain torch in the
dtype it is given (float64: the reference; float32: the CPU precision run) with `bfr()` exactly where the kernel comments place a
rounding, and it takes a `fault` name and then computes that wrong thing instead.

Convolution.  conv = bf16(sum_{ky, kx, ci} x w + bias), then by out_mode: 0 (+ residual; fp32 out: the fp32 sum, bf16 out: a second
rounding), 1 depth-to-space (DCR: channel = (dy, dx, c)), 2 fp32 NCHW, 3 the interior of a padded bf16 NHWC tensor.
  tol = gamma(K) conv(|x|, |w|) (+ |bias|), K = taps Cin: the fp32 accumulation in any order.  Where the residual follows the
  rounding, one spacing of the rounded conv value is added (a flip there is rare but legitimate) and 2 * 2^-24 |sum| for the fp32
  add.  fp32 outputs are held to that tol, and at most FLIP_CAP of them may be further than the fp32 term alone (`tight`) away.
  Exact probes: integer inputs (1 .. 199, distinct per (pixel, channel) modulo the prime 199; 0 / 1 for the power-of-two probe),
  one-hot integer weights, integer bias and residual, every value and every partial sum an integer below 2^8: any summation order
  is exact, the output is one shifted input value (+ bias + residual) or the border's zero, and it is judged bit for bit.

GroupNorm statistics.  float64 mean and 1 / sqrt(biased variance + eps) per (image, group).  The kernel sums x and x^2 in fp32 over
chunks of 256 pixels (n_t = 256 C / 32 terms), then in double: mean within gamma(n_t) E|x|, the variance within
gamma(n_t) (E[x^2] + 2 |mean| E|x|), hence rstd within 0.5 gamma(n_t) (E[x^2] + 2 |mean| E|x|) / (var + eps) relative; 4 fp32
spacings for the stored values.

GroupNorm apply.  The statistics are judged first and the reference output is computed from the implementation's OWN statistics
(the rows_ref rule for written-back intermediates).  tol = the fp32 roundings of the chain (x - mean) rstd [gamma, beta]
[scale, bias] and, for the swish, (8 + 2 |t|) 2^-24 |t sigmoid(t)|: exp2 and rcp at one ulp each, the rounded argument of exp2
(relative 2^-23 of |t| in the exponent), 1 + e and the product.  The re-layout form (no statistics, affine, AdaGN or swish) and
bd_tokens_to_padded are bit-exact.

A "got" dict holds what the kernel leaves in memory: the whole padded tensor where the output is padded (the border of a
convolution output must still hold the sentinel it was filled with, that of a GroupNorm output zero).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from tests.rows_ref import BF16, F32, FLIP_CAP, Report, bfr, case, gamma, to_device, ulp_bf16  # noqa: F401  (re-exported)

SENT16 = 0x7FA5                 # bf16 sentinel: a NaN bit pattern no kernel produces
PRIME = 199


class ConvReport(Report):
    """`excess` (bf16 spacings) covers the outputs judged by Report.bf16; for those judged by Report.f32 (the statistics, the fp32
    outputs) `ratio` is the worst |got - ref| / tol (<= 1 passes), printed where a case has such an output."""

    def __init__(self, what):
        super().__init__(what)
        self.ratio = None

    def f32(self, name, got, val, tol, tight=None):
        g, v = got.double(), val.double()
        if g.shape == v.shape and g.numel() and bool(torch.isfinite(g).all()):
            self.ratio = max(self.ratio or 0.0, ((g - v).abs() / (tol.double() + 1e-30)).max().item())
        super().f32(name, got, val, tol, tight)

    def line(self):
        r = "" if self.ratio is None else f" f32ratio={self.ratio:.3f}"
        return f"CONVSTAT {self.what} flip={self.flip:.3e} excess={self.excess:+.3f}{r}"


def sentinel(shape, dtype, device="cpu"):
    if dtype == BF16:
        return torch.full(shape, SENT16, dtype=torch.int16, device=device).view(BF16)
    return torch.full(shape, float("nan"), dtype=dtype, device=device)


def bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


def border_mask(n, H, W, C, device="cpu"):
    m = torch.ones(n, H + 2, W + 2, C, dtype=torch.bool, device=device)
    m[:, 1:-1, 1:-1] = False
    return m


# ---------------------------------------------------------------------------------------------------------------------------------
# the launcher's geometry (bd_conv_strided): tile width by least padded area, the first of {32, 16, 8} wins ties
def tile_width(H, W):
    best, TW = -1, 32
    for tw in (32, 16, 8):
        th = 256 // tw
        area = -(-W // tw) * tw * -(-H // th) * th
        if best < 0 or area < best:
            best, TW = area, tw
    return TW


def geometry(s):
    """s: a convolution spec (dict) or case -> TW, TH, pixel tiles MT, channel tiles NT, K stages nst, partial tiles, last tile."""
    g = (lambda k, d=None: s.get(k, d)) if isinstance(s, dict) else (lambda k, d=None: getattr(s, k, d))
    H, W, n, cout, cin, k = g("H"), g("W"), g("n"), g("cout"), g("cin"), g("k")
    TW = tile_width(H, W)
    TH = 256 // TW
    NT = (cout + 255) // 256
    return case(TW=TW, TH=TH, MT=n * -(-W // TW) * -(-H // TH), NT=NT, nst=k * k * cin // 32, part_x=W % TW != 0, part_y=H % TH != 0,
                last=cout - (NT - 1) * 256)


# ---------------------------------------------------------------------------------------------------------------------------------
# convolution
CONV_FAULTS = ("drop_tap_last_row", "drop_tap_last_col", "swap_kykx", "stride_origin", "clamp_edge", "bias_last_ctile",
               "res_before_rounding", "no_second_rounding", "dcr_swap_dydx", "dcr_as_crd", "octet_shift", "drop_last_stage")
# the faults of an index, not of a rounding: the exact probes reject each of them on their own (test_conv_ref_cpu.py)
MAPPING_FAULTS = ("drop_tap_last_row", "drop_tap_last_col", "swap_kykx", "stride_origin", "clamp_edge", "bias_last_ctile",
                  "dcr_swap_dydx", "dcr_as_crd", "octet_shift", "drop_last_stage")


def gen_conv(n, H, W, cin, cout, k, stride=1, mode=0, res=None, bias=True, probe=None, seed=0):
    """H, W: the OUTPUT size (the input is stride times that).  res: None, "bf16" or "f32" (the output dtype of mode 0 follows the
    residual's, as in the decoder).  probe: None, ("tap", t) or "pow2"."""
    g = torch.Generator().manual_seed(1000 + seed)
    Hi, Wi = H * stride, W * stride
    K = k * k * cin
    rdt = {None: None, "bf16": BF16, "f32": torch.float32}[res]
    if probe is None:
        x = torch.randn(n, cin, Hi, Wi, generator=g).to(BF16)
        w = (torch.randn(cout, cin, k, k, generator=g) / math.sqrt(K)).to(BF16)
        b = (torch.randn(cout, generator=g) * 0.3).to(BF16) if bias else None
        r = torch.randn(n, H, W, cout, generator=g).to(rdt) if res else None
    else:
        idx = torch.arange(n * Hi * Wi * cin, dtype=torch.int64).view(n, Hi, Wi, cin).permute(0, 3, 1, 2)
        co = torch.arange(cout)
        ci = (co * 5 + 3) % cin
        w = torch.zeros(cout, cin, k, k)
        if probe == "pow2":                                    # taps 0 .. 7 -> 2^t, tap 8 -> -2^8: every sum of 0 / 1 inputs is an integer in [-256, 255]
            x = ((idx * 2654435761 % 2 ** 32) >> 13) & 1
            for t in range(k * k):
                w[co, ci, t // k, t % k] = float(2 ** t) if t < 8 else -256.0
            bias = False
            r = None
            assert res is None
        else:
            t = probe[1]
            x = 1 + (idx * 37) % PRIME
            w[co, ci, t // k, t % k] = 1.0
            r = ((torch.arange(n * H * W * cout, dtype=torch.int64) * 11) % 7).view(n, H, W, cout).to(rdt) if res else None
        x = x.to(BF16)
        w = w.to(BF16)
        b = ((co * 7) % 50).to(BF16) if bias else None
    return case(n=n, H=H, W=W, cin=cin, cout=cout, k=k, stride=stride, mode=mode, res=r, out_f32=int(res == "f32" or mode == 2),
                bias=b, probe=probe, x=x.contiguous(), w=w)


def _conv(x, w, c, origin_off=False):
    if origin_off:                                             # the taps gathered around (2y + 1, 2x + 1) instead of (2y, 2x)
        return F.conv2d(F.pad(x, (0, 2, 0, 2)), w, stride=c.stride)
    return F.conv2d(x, w, stride=c.stride, padding=c.k // 2)


def _d2s(t, fault=None):
    """NCHW [n][4 Cq][H][W] -> NHWC [n][2H][2W][Cq], DCR: channel = (dy, dx, c)."""
    n, C4, H, W = t.shape
    Cq = C4 // 4
    if fault == "dcr_as_crd":
        v = t.view(n, Cq, 2, 2, H, W).permute(0, 4, 2, 5, 3, 1)
    else:
        v = t.view(n, 2, 2, Cq, H, W)
        v = v.permute(0, 4, 2, 5, 1, 3) if fault == "dcr_swap_dydx" else v.permute(0, 4, 1, 5, 2, 3)
    return v.reshape(n, 2 * H, 2 * W, Cq)


def _trunc_bf16(v):
    """fp32 -> bf16 by dropping the low half (no rounding)."""
    return (v.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF16)


def ref_conv(c, dtype=torch.float64, fault=None):
    """-> dict: val / tol in the logical output layout (mode 3: the interior), kind "bf16" / "f32", tight (fp32 outputs), and
    out = what an implementation computing `val` leaves in the output tensor (border included)."""
    geo = geometry(c)
    k = c.k
    x, w = c.x.to(dtype), c.w.to(dtype)
    if fault == "swap_kykx":
        w = w.transpose(2, 3)
    if fault == "drop_last_stage":
        w = w.clone()
        w[:, -32:, k - 1, k - 1] = 0
    acc = _conv(x, w, c, fault == "stride_origin" and c.stride == 2)
    if fault in ("drop_tap_last_row", "drop_tap_last_col"):
        row = fault == "drop_tap_last_row"
        ky, kx = (0, 0) if k == 1 else (0, 1) if row else (1, 0)   # a tap that reads the image there (the opposite one reads the border)
        w1 = torch.zeros_like(w)
        w1[:, :, ky, kx] = w[:, :, ky, kx]
        d = _conv(x, w1, c)
        if row:
            acc[:, :, -1, :] -= d[:, :, -1, :]
        else:
            acc[:, :, :, -1] -= d[:, :, :, -1]
    mag = _conv(x.abs(), w.abs(), c)
    if c.bias is not None:
        b = c.bias.to(dtype).clone()
        if fault == "bias_last_ctile":
            b[(geo.NT - 1) * 256:] = 0
        acc = acc + b[None, :, None, None]
        mag = mag + b.abs()[None, :, None, None]
    if fault == "clamp_edge":                                  # the clamp of a partial tile one pixel short: its last pixel re-reads the neighbour
        acc = acc.clone()
        if geo.part_x and c.W >= 2:
            acc[:, :, :, -1] = acc[:, :, :, -2]
        if geo.part_y and c.H >= 2:
            acc[:, :, -1, :] = acc[:, :, -2, :]
    if fault == "octet_shift":
        acc = torch.roll(acc, -8, dims=1)
    tol = gamma(k * k * c.cin) * mag + 1e-30
    pre, convb = acc, bfr(acc)
    out = dict(kind="f32" if c.out_f32 else "bf16", tight=None)
    if c.mode == 0:
        pre, convb, tol = (t.permute(0, 2, 3, 1) for t in (pre, convb, tol))
        if c.res is None:
            out["val"], out["tol"] = pre, tol
        else:
            s = (pre if fault == "res_before_rounding" else convb) + c.res.to(dtype)
            out["val"], out["tight"] = s, 2 * F32 * s.abs() + 1e-30
            out["tol"] = ulp_bf16(pre).to(dtype) + tol + out["tight"]
    elif c.mode == 1:
        out["val"], out["tol"] = _d2s(pre, fault), _d2s(tol)
    elif c.mode == 2:
        out["val"], out["tol"], out["tight"] = convb, ulp_bf16(pre).to(dtype) + tol, torch.full_like(tol, 1e-30)
    else:
        out["val"], out["tol"] = pre.permute(0, 2, 3, 1), tol.permute(0, 2, 3, 1)
    return out


def impl_conv(c, dtype, fault=None):
    r = ref_conv(c, dtype, fault)
    v = r["val"]
    if c.out_f32:
        o = v.float()
    elif fault == "no_second_rounding":
        o = _trunc_bf16(v)
    else:
        o = v.to(BF16)
    if c.mode == 3:
        full = sentinel((c.n, c.H + 2, c.W + 2, c.cout), BF16)
        full[:, 1:-1, 1:-1] = o
        o = full
    return dict(out=o.contiguous())


def judge_conv(c, got, what):
    rep = ConvReport(what)
    r = ref_conv(c)
    o = got["out"]
    if c.mode == 3:
        m = border_mask(c.n, c.H, c.W, c.cout, o.device)
        if o.shape != m.shape:
            rep.fail.append(f"{what}: shape {tuple(o.shape)}")
            return rep
        if not bool((bits(o)[m] == SENT16).all()):
            rep.fail.append(f"{what}: the border of the padded output was written")
        o = o[:, 1:-1, 1:-1]
    if c.probe is not None:
        want = r["val"].float() if c.out_f32 else r["val"].to(BF16)
        assert torch.equal(want.double(), r["val"].double()), "a probe's expected value must be exact"
        rep.equal("out", o.contiguous(), want.contiguous())
        if not rep.fail:
            rep.excess = -1.0
    elif c.out_f32:
        rep.f32("out", o, r["val"], r["tol"], r["tight"])
    else:
        rep.bf16("out", o, r["val"], r["tol"])
    return rep


def conv_fault_applies(c, fault):
    geo = geometry(c)
    if c.probe is not None:                                    # exact: a fault counts iff it changes the expected bits at all
        if fault not in MAPPING_FAULTS:
            return False
        a, b = impl_conv(c, torch.float64)["out"], impl_conv(c, torch.float64, fault)["out"]
        return not torch.equal(bits(a), bits(b))
    if fault == "drop_tap_last_row": return c.H >= 2
    if fault == "drop_tap_last_col": return c.W >= 2
    if fault == "swap_kykx": return c.k == 3
    if fault == "stride_origin": return c.stride == 2
    if fault == "clamp_edge": return (geo.part_x and c.W >= 2) or (geo.part_y and c.H >= 2)
    if fault == "bias_last_ctile": return c.bias is not None
    if fault == "res_before_rounding": return c.res is not None
    if fault == "no_second_rounding": return c.res is not None and not c.out_f32
    if fault in ("dcr_swap_dydx", "dcr_as_crd"): return c.mode == 1
    if fault == "octet_shift": return c.cout > 8
    return True


def _conv_specs():
    S = {}

    def add(name, **kw):
        assert name not in S
        kw.setdefault("seed", len(S))
        S[name] = kw

    # every tile width with full tiles and with partial tiles in x, in y and in both (shape -> TW by the launcher's rule)
    shapes = {"tw32_full": (8, 32), "tw32_px": (8, 40), "tw32_py": (12, 32), "tw32_pxy": (20, 60),
              "tw16_full": (16, 16), "tw16_px": (16, 12), "tw16_py": (24, 16), "tw16_pxy": (24, 12),
              "tw8_full": (32, 8), "tw8_px": (32, 5), "tw8_py": (40, 8), "tw8_pxy": (40, 5)}
    res = (None, "bf16", "f32")
    for i, (nm, (H, W)) in enumerate(shapes.items()):
        add(f"{nm}_3x3_c64_o72", n=1 + i % 3, H=H, W=W, cin=64, cout=72, k=3, res=res[i % 3])
    # stage counts 1 .. 9 of the DMA ring through 1x1 shortcuts, on tile shapes of every width
    for i, cin in enumerate(range(32, 289, 32)):
        H, W = list(shapes.values())[(5 * i + 3) % 12]
        add(f"nst{cin // 32}_1x1_c{cin}_{H}x{W}", n=1 + i % 2, H=H, W=W, cin=cin, cout=64 if i % 2 else 320, k=1, res=res[(i + 1) % 3])
    add("nst9_3x3_c32", n=1, H=16, W=32, cin=32, cout=64, k=3)
    add("nst18_3x3_c64", n=2, H=16, W=16, cin=64, cout=248, k=3, res="f32")
    add("nst144_3x3_c512", n=1, H=8, W=8, cin=512, cout=64, k=3, res="bf16")
    # pixel-tile counts 1, 7, 8, 9, 12 x 1, 2, 3 channel tiles (the short last group of the block-to-tile map: MT % 8 != 0, NT > 1)
    mts = {1: (1, 8, 32), 7: (1, 56, 32), 8: (2, 32, 32), 9: (1, 48, 48), 12: (3, 32, 32)}
    for i, (mt, (n, H, W)) in enumerate(mts.items()):
        for j, cout in enumerate((64, 264, 520)):
            k = 3 if (i + j) % 2 else 1
            add(f"mt{mt}_nt{j + 1}_{k}x{k}_o{cout}", n=n, H=H, W=W, cin=32, cout=cout, k=k, res=res[(i + j) % 3], mode=0)
    add("last248_nt2_o504", n=1, H=12, W=40, cin=32, cout=504, k=3)
    # the other epilogues, on partial tiles
    for cout in (3, 4, 12):
        add(f"image_o{cout}", n=2, H=20, W=60 if cout == 3 else 12, cin=32, cout=cout, k=3, mode=2)
    add("d2s_o32", n=2, H=24, W=12, cin=64, cout=32, k=3, mode=1)
    add("d2s_o1024", n=1, H=12, W=40, cin=32, cout=1024, k=3, mode=1)
    add("d2s_1x1_o64_tw8", n=1, H=40, W=5, cin=96, cout=64, k=1, mode=1)
    add("padded_o72", n=2, H=20, W=60, cin=32, cout=72, k=3, mode=3)
    add("padded_o264_tw8", n=1, H=40, W=5, cin=64, cout=264, k=1, mode=3)
    add("nobias_o64", n=1, H=16, W=12, cin=32, cout=64, k=3, bias=False, res="bf16")
    # stride 2: odd output sizes (partial tiles in both directions), H or W of one pixel
    add("s2_7x5", n=3, H=7, W=5, cin=32, cout=64, k=3, stride=2)
    add("s2_37x19_o264", n=1, H=37, W=19, cin=64, cout=264, k=3, stride=2, res="f32")
    add("s2_1x9", n=2, H=1, W=9, cin=32, cout=264, k=3, stride=2, res="bf16")
    add("s2_6x1", n=3, H=6, W=1, cin=64, cout=264, k=3, stride=2)
    add("s2_13x33_padded", n=1, H=13, W=33, cin=32, cout=72, k=3, stride=2, mode=3)
    add("s2_9x9_d2s", n=1, H=9, W=9, cin=32, cout=32, k=3, stride=2, mode=1)
    add("s2_15x7_image", n=3, H=15, W=7, cin=32, cout=3, k=3, stride=2, mode=2)
    # exact probes: one per tap (partial tiles, two channel tiles with channel padding, several K stages), the power-of-two
    # probe per stride, one per out_mode and per stride
    for t in range(9):
        H, W = ((20, 60), (24, 12), (40, 5))[t % 3]
        add(f"probe_tap{t}", n=1 + t % 2, H=H, W=W, cin=64, cout=264, k=3, probe=("tap", t), res=res[t % 3])
    add("probe_pow2", n=2, H=12, W=40, cin=32, cout=264, k=3, probe="pow2")
    add("probe_pow2_s2", n=2, H=7, W=5, cin=64, cout=72, k=3, stride=2, probe="pow2")
    for t in (0, 2, 6, 8):
        add(f"probe_s2_tap{t}", n=1, H=9, W=13, cin=32, cout=72, k=3, stride=2, probe=("tap", t))
    add("probe_1x1_c96", n=2, H=24, W=12, cin=96, cout=520, k=1, probe=("tap", 0), res="f32")
    add("probe_d2s", n=2, H=12, W=40, cin=32, cout=64, k=3, mode=1, probe=("tap", 3))
    add("probe_d2s_pow2_s2", n=1, H=9, W=5, cin=32, cout=32, k=3, mode=1, stride=2, probe="pow2")
    add("probe_image_o12", n=2, H=40, W=5, cin=32, cout=12, k=3, mode=2, probe=("tap", 5))
    add("probe_image_o3_s2", n=1, H=5, W=7, cin=32, cout=3, k=3, mode=2, stride=2, probe=("tap", 1))
    add("probe_padded", n=2, H=20, W=60, cin=32, cout=264, k=3, mode=3, probe=("tap", 7))
    add("probe_padded_pow2_s2", n=1, H=13, W=33, cin=32, cout=40, k=3, mode=3, stride=2, probe="pow2")
    return S


CONV_SPECS = _conv_specs()
CONV_CASES = {name: (lambda kw=kw: gen_conv(**kw)) for name, kw in CONV_SPECS.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# GroupNorm(32) statistics
GN_EPS = 1e-6
STATS_FAULTS = ("eps10", "unbiased", "group_shift", "img0_stats")


def gen_gn_x(g, n, HW, C, f32, kind):
    """[n][HW][C].  general: mean 0.5, std 2.  varied: a mean and a std of its own per (image, group), std over two decades,
    mean^2 <= var, and image 1 a thousand times smaller (its variances are of the order of eps).  (m, s): that mean and std."""
    cpg = C // 32
    z = torch.randn(n, HW, 32, cpg, generator=g)
    if kind == "general":
        x = z * 2 + 0.5
    elif kind == "varied":
        std = 10 ** (torch.rand(n, 1, 32, 1, generator=g) * 2 - 1.5)
        mean = std * (torch.rand(n, 1, 32, 1, generator=g) * 2 - 1)
        x = z * std + mean
        if n > 1:
            x[1] *= 1e-3
    else:
        x = z * kind[1] + kind[0]
    return x.reshape(n, HW, C).to(torch.float32 if f32 else BF16)


def gen_gn_stats(n, HW, C, f32, kind, seed, eps=GN_EPS, char=False):
    g = torch.Generator().manual_seed(2000 + seed)
    return case(n=n, HW=HW, C=C, f32=int(f32), kind=kind, eps=eps, char=char, x=gen_gn_x(g, n, HW, C, f32, kind))


def ref_gn_stats(c, dtype=torch.float64, fault=None, x=None):
    """-> mean, rstd [n][32] and their tolerances (absolute)."""
    x = (c.x if x is None else x).reshape(c.n, -1, c.C).to(dtype)
    cpg = c.C // 32
    if fault == "group_shift":
        x = torch.roll(x, -1, dims=-1)
    gq = x.view(c.n, -1, 32, cpg)
    N = gq.shape[1] * cpg
    mean = gq.mean((1, 3))
    var = ((gq - mean[:, None, :, None]) ** 2).mean((1, 3))
    if fault == "unbiased":
        var = var * N / (N - 1)
    eps = c.eps * (10 if fault == "eps10" else 1)
    rstd = (var + eps).rsqrt()
    if fault == "img0_stats":
        mean, rstd = mean[:1].expand_as(mean), rstd[:1].expand_as(rstd)
    a1, a2 = gq.abs().mean((1, 3)), (gq * gq).mean((1, 3))
    gm = gamma(256 * cpg)
    rel = 0.5 * gm * (a2 + 2 * mean.abs() * a1) / (var + eps) + 4 * F32
    return dict(mean=mean, rstd=rstd, mean_tol=gm * a1 + 4 * F32 * mean.abs() + 1e-30, rstd_tol=rstd * rel, rstd_rel=rel)


def impl_gn_stats(c, dtype, fault=None):
    r = ref_gn_stats(c, dtype, fault)
    return dict(stats=torch.stack([r["mean"], r["rstd"]], -1).float())


def _judge_stats(rep, c, stats, x=None):
    r = ref_gn_stats(c, x=x)
    if stats.shape != (c.n, 32, 2):
        rep.fail.append(f"{rep.what}: stats shape {tuple(stats.shape)}")
        return r
    rep.f32("mean", stats[..., 0], r["mean"], r["mean_tol"])
    rep.f32("rstd", stats[..., 1], r["rstd"], r["rstd_tol"])
    return r


def judge_gn_stats(c, got, what):
    rep = ConvReport(what)
    _judge_stats(rep, c, got["stats"])
    return rep


def rstd_rel_error(c, stats):
    """Worst relative rstd error of `stats` against float64, and the worst derived bound."""
    r = ref_gn_stats(c)
    return ((stats[..., 1].double() - r["rstd"]).abs() / r["rstd"]).max().item(), r["rstd_rel"].max().item()


def emulate_gn_stats(c):
    """bd_gn_stats as gn_stats_kernel / gn_finalize_kernel sum it, on the CPU in fp32 (C >= 256: an octet inside one group): a
    thread keeps one channel octet and adds its pixels of a 256-pixel chunk in order, per channel; the eight channel sums are
    added, then the threads of a group in (pixel lane, octet) order; the chunk sums are added in double.  -> stats [n][32][2]."""
    x = c.x.float().reshape(c.n, -1, c.C)
    n, HW, C = x.shape
    C8, cpg = C // 8, C // 32
    assert cpg >= 8
    step, opg = 256 // C8, cpg // 8
    S1, S2 = torch.zeros(n, 32, dtype=torch.float64), torch.zeros(n, 32, dtype=torch.float64)
    for ch in range((HW + 255) // 256):
        xs = x[:, ch * 256:(ch + 1) * 256]
        pad = (-xs.shape[1]) % step
        if pad:
            xs = torch.cat([xs, torch.zeros(n, pad, C)], 1)
        v = xs.view(n, -1, step, C)                            # pixel = i * step + pixel lane
        a1, a2 = torch.zeros(n, step, C), torch.zeros(n, step, C)
        for i in range(v.shape[1]):
            a1, a2 = a1 + v[:, i], a2 + v[:, i] * v[:, i]
        a1, a2 = a1.view(n, step, C8, 8), a2.view(n, step, C8, 8)
        u1, u2 = torch.zeros(n, step, C8), torch.zeros(n, step, C8)
        for j in range(8):
            u1, u2 = u1 + a1[..., j], u2 + a2[..., j]
        u1, u2 = u1.view(n, step, 32, opg), u2.view(n, step, 32, opg)
        r1, r2 = torch.zeros(n, 32), torch.zeros(n, 32)
        for lp in range(step):
            for o in range(opg):
                r1, r2 = r1 + u1[:, lp, :, o], r2 + u2[:, lp, :, o]
        S1, S2 = S1 + r1.double(), S2 + r2.double()
    mean = S1 / (HW * cpg)
    var = (S2 / (HW * cpg) - mean * mean).clamp_min(0)
    return torch.stack([mean, (var + c.eps).rsqrt()], -1).float()


def stats_fault_applies(c, fault):
    if c.char:
        return False                                           # characterisation sets: the derived bound is loose or vacuous there
    if fault == "eps10": return c.kind == "varied" and c.n > 1              # image 1: variances of the order of eps
    if fault == "unbiased":                                    # 0.5 / (N - 1) >= 8e-3 against a bound <= 1e-3; N = 1 has no unbiased variance
        return c.kind == "general" and 2 <= c.HW * (c.C // 32) <= 64
    if fault == "img0_stats": return c.n > 1
    return True


def _stats_specs():
    S = {}
    i = 0
    for C in (32, 64, 128, 256, 512, 1024, 2048):
        for HW in (1, 64, 255, 256, 257, 703):
            varied = i % 3 == 1 and HW > 1
            nm = f"c{C}_hw{HW}_{'f32' if i % 2 else 'bf16'}_{'varied' if varied else 'general'}"
            S[nm] = dict(n=2 if varied or i % 4 == 0 else 1, HW=HW, C=C, f32=i % 2, kind="varied" if varied else "general", seed=i)
            i += 1
    S["c32_hw65792_f32_general"] = dict(n=1, HW=65792, C=32, f32=1, kind="general", seed=90)      # 257 chunks: the strided loop of the finalize
    S["c32_hw66000_bf16_varied"] = dict(n=2, HW=66000, C=32, f32=0, kind="varied", seed=91)
    S["c32_hw703_f32_offset64"] = dict(n=2, HW=703, C=32, f32=1, kind=(8.0, 1.0), seed=92)        # mean^2 / var = 64: bound ~ 2e-3
    S["char_c512_hw1024_mean4_std0.5"] = dict(n=1, HW=1024, C=512, f32=1, kind=(4.0, 0.5), seed=93, char=True)
    S["char_c2048_hw1000_mean8_std0.25"] = dict(n=1, HW=1000, C=2048, f32=1, kind=(8.0, 0.25), seed=94, char=True)
    return S


STATS_SPECS = _stats_specs()
STATS_CASES = {name: (lambda kw=kw: gen_gn_stats(**kw)) for name, kw in STATS_SPECS.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# GroupNorm apply
APPLY_FAULTS = ("ada_before_affine", "swish_pre_affine", "border_written", "img0_stats", "group_shift")


def gen_gn_apply(n, H, W, C, f32, stats, affine, ada, swish, mode, seed):
    g = torch.Generator().manual_seed(3000 + seed)
    x = gen_gn_x(g, n, H * W, C, f32, "varied").view(n, H, W, C)
    if n > 1:
        x[1] = (x[1].float() * 300).to(x.dtype)                # (image 1 of the varied set is 1e-3 of image 0: keep it above eps here)
    rn = lambda *s: torch.randn(*s, generator=g)
    return case(n=n, H=H, W=W, HW=H * W, C=C, f32=int(f32), stats=bool(stats), swish=int(swish), mode=mode, eps=GN_EPS, x=x,
                gamma=1 + 0.5 * rn(C) if affine else None, beta=0.5 * rn(C) if affine else None,
                scale=1 + 0.5 * rn(n, C) if ada else None, bias=0.5 * rn(n, C) if ada else None)


def relayout(c):
    return not c.stats and c.gamma is None and c.scale is None and not c.swish


def ref_gn_apply(c, stats, dtype=torch.float64, fault=None):
    """stats: [n][32][2] fp32 as the implementation holds them (None: y = x) -> val, tol [n][H][W][C]."""
    x = c.x.to(dtype)
    cpg = c.C // 32
    if stats is not None:
        ch = torch.arange(c.C, device=x.device)
        grp = ((ch + 1) // cpg).clamp_max(31) if fault == "group_shift" else ch // cpg
        st = stats.to(dtype)
        if fault == "img0_stats":
            st = st[:1].expand_as(st)
        mu, rs = st[:, grp, 0][:, None, None, :], st[:, grp, 1][:, None, None, :]
        t0 = x - mu
        t = t0 * rs
        err = F32 * t0.abs() * rs + F32 * t.abs()
    else:
        t, err = x, torch.zeros_like(x)
    sw = lambda v: v * torch.sigmoid(v)
    if c.swish and fault == "swish_pre_affine":
        t = sw(t)

    def aff(t, err):
        if c.gamma is None:
            return t, err
        ga, be = c.gamma.to(dtype), c.beta.to(dtype)
        return t * ga + be, ga.abs() * err + 2 * F32 * ((t * ga).abs() + be.abs())

    def ada(t, err):
        if c.scale is None:
            return t, err
        sc, bi = c.scale.to(dtype)[:, None, None, :], c.bias.to(dtype)[:, None, None, :]
        return sc * t + bi, sc.abs() * err + 2 * F32 * ((sc * t).abs() + bi.abs())

    for f in ((ada, aff) if fault == "ada_before_affine" else (aff, ada)):
        t, err = f(t, err)
    if c.swish:
        s = t if fault == "swish_pre_affine" else sw(t)
        err = 1.1 * err + (8 + 2 * t.abs()) * F32 * sw(t).abs()
        t = s
    return dict(val=t, tol=err + 1e-30)


def impl_gn_apply(c, dtype, fault=None):
    stats = impl_gn_stats(c, dtype)["stats"] if c.stats else None
    v = ref_gn_apply(c, stats, dtype, fault)["val"]
    if c.mode == 0:
        o = torch.zeros(c.n, c.H + 2, c.W + 2, c.C, dtype=BF16)
        if fault == "border_written":
            o[:, :, -1] = 1.0
        o[:, 1:-1, 1:-1] = v.to(BF16)
    else:
        o = v.float() if c.mode == 1 else v.to(BF16)
    return dict(stats=stats, out=o)


def judge_gn_apply(c, got, what):
    rep = ConvReport(what)
    o = got["out"]
    if c.stats:
        _judge_stats(rep, c, got["stats"])
    if c.mode == 0:
        m = border_mask(c.n, c.H, c.W, c.C, o.device)
        if o.shape != m.shape:
            rep.fail.append(f"{what}: shape {tuple(o.shape)}")
            return rep
        if not bool((bits(o)[m] == 0).all()):
            rep.fail.append(f"{what}: the zero border of the padded output was written")
        o = o[:, 1:-1, 1:-1]
    r = ref_gn_apply(c, got["stats"] if c.stats else None)
    if relayout(c):
        rep.equal("out", o.contiguous(), (r["val"].float() if c.mode == 1 else r["val"].to(BF16)).contiguous())
    elif c.mode == 1:
        rep.f32("out", o, r["val"], r["tol"])
    else:
        rep.bf16("out", o, r["val"], r["tol"])
    return rep


def apply_fault_applies(c, fault):
    if fault == "ada_before_affine": return c.gamma is not None and c.scale is not None
    if fault == "swish_pre_affine": return bool(c.swish) and (c.gamma is not None or c.scale is not None)
    if fault == "border_written": return c.mode == 0
    if fault == "img0_stats": return c.stats and c.n > 1
    if fault == "group_shift": return c.stats
    return True


def _apply_specs():
    S = {}
    Ws, Cs = (1, 5, 64, 100), (32, 64, 128, 256, 512, 1024, 2048)
    i = 0
    for stats in (1, 0):
        for form in ("affine", "ada", "plain", "both"):
            for swish in (0, 1):
                for mode in (0, 1, 2):
                    if form == "both" and (mode != (swish + stats) % 3):
                        continue                               # affine AND AdaGN (not a decoder form, but the kernel's order matters): a few
                    W, C = Ws[i % 4], Cs[(i * 3 + i // 7) % 7]
                    nm = f"{'stats' if stats else 'nostats'}_{form}_{'swish' if swish else 'lin'}_m{mode}_c{C}_w{W}"
                    S[nm] = dict(n=2, H=1 + i % 3, W=W, C=C, f32=(i // 2) % 2, stats=stats, affine=form in ("affine", "both"),
                                 ada=form in ("ada", "both"), swish=swish, mode=mode, seed=i)
                    i += 1
    S["stats_affine_swish_m0_c2048_w100"] = dict(n=2, H=2, W=100, C=2048, f32=0, stats=1, affine=True, ada=False, swish=1, mode=0, seed=80)
    S["nostats_plain_lin_m0_c2048_w5_f32"] = dict(n=1, H=3, W=5, C=2048, f32=1, stats=0, affine=False, ada=False, swish=0, mode=0, seed=81)
    return S


APPLY_SPECS = _apply_specs()
APPLY_CASES = {name: (lambda kw=kw: gen_gn_apply(**kw)) for name, kw in APPLY_SPECS.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# bd_tokens_to_padded: [n][C][H][W] fp32 -> the interior of a padded bf16 NHWC tensor, bit-exact
TOKEN_FAULTS = ("nchw_as_nhwc", "border_written")


def gen_tokens(n, C, H, W, seed):
    g = torch.Generator().manual_seed(4000 + seed)
    return case(n=n, C=C, H=H, W=W, z=torch.randn(n, C, H, W, generator=g))


def impl_tokens(c, dtype, fault=None):
    z = c.z.view(c.n, c.H, c.W, c.C) if fault == "nchw_as_nhwc" else c.z.permute(0, 2, 3, 1)
    o = sentinel((c.n, c.H + 2, c.W + 2, c.C), BF16)
    if fault == "border_written":
        o[:, 0] = 0.0
    o[:, 1:-1, 1:-1] = z.to(dtype).to(BF16)
    return dict(out=o)


def judge_tokens(c, got, what):
    rep = ConvReport(what)
    rep.equal("out", bits(got["out"]), bits(impl_tokens(c, torch.float64)["out"].to(got["out"].device)))
    return rep


TOKEN_SPECS = {
    "n1_c32_1x1": dict(n=1, C=32, H=1, W=1, seed=0),
    "n2_c32_16x24": dict(n=2, C=32, H=16, W=24, seed=1),
    "n3_c256_5x7": dict(n=3, C=256, H=5, W=7, seed=2),
    "n1_c7_3x250": dict(n=1, C=7, H=3, W=250, seed=3),
    "n2_c64_96x96_gridstride": dict(n=2, C=64, H=96, W=96, seed=4),          # 1.18 M elements > 4096 * 256: the grid-stride loop
}
TOKEN_CASES = {name: (lambda kw=kw: gen_tokens(**kw)) for name, kw in TOKEN_SPECS.items()}


LAUNCHERS = {
    "conv": (CONV_CASES, impl_conv, judge_conv, CONV_FAULTS, conv_fault_applies),
    "gn_stats": (STATS_CASES, impl_gn_stats, judge_gn_stats, STATS_FAULTS, stats_fault_applies),
    "gn_apply": (APPLY_CASES, impl_gn_apply, judge_gn_apply, APPLY_FAULTS, apply_fault_applies),
    "tokens": (TOKEN_CASES, impl_tokens, judge_tokens, TOKEN_FAULTS, lambda c, f: f != "nchw_as_nhwc" or (c.H * c.W > 1 and c.C > 1)),
}


def coverage():
    """What the case lists cover, from the specs alone (no tensors): the sets the coverage test asserts."""
    conv = [(kw, geometry(kw)) for kw in CONV_SPECS.values()]
    mode0 = [kw for kw, _ in conv if kw.get("mode", 0) == 0]
    return case(
        tiles={(g.TW, g.part_x, g.part_y) for _, g in conv},
        nst_1x1={g.nst for kw, g in conv if kw["k"] == 1},
        nst_3x3={g.nst for kw, g in conv if kw["k"] == 3},
        mt_nt={(g.MT, g.NT) for _, g in conv},
        short_group_multi_nt={(g.MT, g.NT) for _, g in conv if g.MT % 8 and g.NT > 1},
        last={g.last for kw, g in conv if kw.get("mode", 0) != 2},
        image_cout={kw["cout"] for kw, _ in conv if kw.get("mode", 0) == 2},
        d2s_cout={kw["cout"] for kw, _ in conv if kw.get("mode", 0) == 1},
        res={kw.get("res") for kw in mode0},
        partial_modes={kw.get("mode", 0) for kw, g in conv if g.part_x and g.part_y},
        s2={(kw["H"], kw["W"]) for kw, _ in conv if kw.get("stride", 1) == 2},
        s2_partial={(g.part_x, g.part_y) for kw, g in conv if kw.get("stride", 1) == 2},
        n={kw["n"] for kw, _ in conv},
        probe_taps={kw["probe"][1] for kw, _ in conv if isinstance(kw.get("probe"), tuple) and kw["k"] == 3 and kw.get("stride", 1) == 1},
        probe_modes={(kw.get("mode", 0), kw.get("stride", 1)) for kw, _ in conv if kw.get("probe")},
        probe_pow2={kw.get("stride", 1) for kw, _ in conv if kw.get("probe") == "pow2"},
        gn_c_hw={(kw["C"], kw["HW"]) for kw in STATS_SPECS.values()},
        gn_dtypes={kw["f32"] for kw in STATS_SPECS.values()},
        gn_chunks=max(-(-kw["HW"] // 256) for kw in STATS_SPECS.values()),
        gn_varied_n2=any(kw["kind"] == "varied" and kw["n"] == 2 for kw in STATS_SPECS.values()),
        apply_forms={(kw["stats"], kw["affine"], kw["ada"], kw["swish"], kw["mode"]) for kw in APPLY_SPECS.values()},
        apply_w={kw["W"] for kw in APPLY_SPECS.values()},
        apply_c={kw["C"] for kw in APPLY_SPECS.values()},
        token_grid_stride=any(kw["n"] * kw["C"] * kw["H"] * kw["W"] > 4096 * 256 for kw in TOKEN_SPECS.values()),
    )
