"""Exact probes, host-side operand writers, the form table and the float64 references of tests/test_gpu_gemm.py and
tests/test_gemm_ref_cpu.py.

Exactness.  Activations are non-zero small integers (+-1 .. +-7) times a power of two per row, weights +-1 .. +-15 times a power of
two per output channel (bf16 / e4m3) or e2m1 values (0.5 .. 3) times a power of two per 32-k block (MXFP4), the bias a multiple of
2^-9.  Every product and every partial sum of a case is then an integer multiple of one quantum and stays below 2^24 quanta
(`Probe.__init__` asserts it for the largest K), so an fp32 accumulation is exact in ANY order, through any tile form, slice count,
ring depth or in-workgroup K split, and the kernel's fp32 output must equal the float64 product bit for bit; the bf16(+bias) output
is one rounding of an exactly known number (the ranges are wide enough that a one-stage sum already needs that rounding, so a
misplaced bias or a second rounding shows on the smallest probe).  Only silu (hardware exp2 / rcp) is not bit-reproducible: the SwiGLU output is judged by
rows_ref.ref_swiglu with its tolerance and its 1 % flip cap.

Column convention.  A weight matrix W [N][K] is indexed by PACKED row = output column of the slab / bf16 / fp32 epilogues.  The
SwiGLU epilogue reads the same packed rows as 16 gate | 16 up features per 32-row panel (feature f: gate = packed row
(f >> 4) * 32 + (f & 15), up = that + 16), so one packed operand serves all four epilogues.  Packed rows with (row & 16) == 0 -- the
gate rows -- carry an extra power of two chosen per stage count (`Probe.gshift`) that keeps the gate pre-activation at a standard
deviation of ~2, where silu is neither x nor 0.

Layouts (written here from the comments of bd_common.h, bd_gemm.hip, bd_gemm8.hip and bd_gemm4.hip; nothing is shared with the
device pack kernels, which tests/test_gpu_gemm.py compares against these writers bit for bit):
  afrag   bf16 A, 1 KiB chunk per (k-step of 16, row block of 32), chunks [ks][rb]; lane l = row l & 31, k = ks * 16 + (l >> 5) * 8 + 0..7
  a8      e4m3 A, 2 KiB chunk per (64-deep stage, row block) as two 1 KiB halves h; lane l = row l & 31, k = st * 64 + (l >> 5) * 32 + 16 h + 0..15
  w bf16  16 B unit (panel, ks, lane) at panel * PS + (ks >> 2) * SS + (ks & 3) * 64 + lane; panel-major PS = K / 16 * 64, SS = 256;
          stage-major PS = 256, SS = panels * 256; lane l = packed row panel * 32 + (l & 31), k as afrag
  w8      (panel, PAIR of k-steps kp, lane): low 8 bytes = k-step 2 kp, high 8 = 2 kp + 1, each k = ks * 16 + (l >> 5) * 8 + 0..7
  w8k     (panel, stage, half h, lane): k = st * 64 + (l >> 5) * 32 + 16 h + 0..15
  w4k     (panel, stage, lane): the 16 source bytes (two e2m1 nibbles each, even k low) of k = st * 64 + (l >> 5) * 32 + 0..31;
          exponents: dword (panel, g, lane), byte b = E8M0 of (row, k block 2 (4 g + b) + (l >> 5)); stages past K hold 127
"""
from __future__ import annotations

import math
import types

import torch

from tests import rows_ref as rr
from tests.rows_ref import BF16

EPI_PARTIAL, EPI_SWIGLU, EPI_BF16, EPI_F32 = 0, 1, 2, 3
EPIS = (EPI_PARTIAL, EPI_SWIGLU, EPI_BF16, EPI_F32)
NSTAGE = 30                                    # stage counts 1 .. 30
E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# The form table: one entry per tile form gemm_kernel<NP, KW, MB, EPI, R, RED, MODE, WT> that bdk_gemm / bdk_gemm8 / bdk_gemm8a /
# bdk_gemm4a dispatch, with the `nw` code (waves + 16 ring + 256 (kw - 1) + 2048 pipe) and the row-block count RB that select it.
def _form(wt, np_, kw, mb, ring, pipe=0, req_ring=None, note=""):
    nw = np_ * kw
    code = nw + 16 * (ring if req_ring is None else req_ring) + 256 * (kw - 1) + 2048 * pipe
    return types.SimpleNamespace(wt=wt, np=np_, kw=kw, mb=mb, ring=ring, pipe=pipe, nw=code, rb=mb, note=note,
                                 id=f"wt{wt}-np{np_}-kw{kw}-mb{mb}-r{ring}" + ("-pipe" if pipe else ""))


def _bf16_forms():
    f = []
    # BD_CASE_PIPE (ring 2, LDS reads one stage ahead)
    for np_, kw, mb in ((4, 1, 4), (2, 1, 4), (2, 2, 4), (4, 1, 2), (4, 1, 1)):
        f.append(_form(0, np_, kw, mb, 2, pipe=1))
    # BD_CASE, in the launcher's order.  MB = 8: RB % 8 == 0, >= 4 waves, kw 1, ring forced to 2.  (8, 1, 8) at N % 256 == 0 reaches
    # the generic kernel through the fp32-sum epilogue and the S >= 2 reduced epilogues at RB 8; its other calls run gemm_wide_kernel,
    # so form_ns gives it a second width, N = 480, where every slab / bf16 / SwiGLU call is this form's
    f += [_form(0, 4, 1, 8, 2), _form(0, 8, 1, 8, 2, note="at N = 512 slabs / bf16 / SwiGLU at S = 1 run gemm_wide_kernel; at N = 480 this form"),
          _form(0, 10, 1, 4, 2), _form(0, 9, 1, 4, 2), _form(0, 5, 1, 4, 2),
          _form(0, 2, 1, 4, 2), _form(0, 4, 1, 4, 2), _form(0, 8, 1, 4, 2), _form(0, 4, 1, 4, 3), _form(0, 8, 1, 4, 3),
          _form(0, 4, 1, 4, 4), _form(0, 8, 1, 4, 4),
          # MB <= 2: a requested ring 3 becomes 4; MB = 1: always ring 2
          _form(0, 2, 1, 2, 2), _form(0, 4, 1, 2, 2), _form(0, 8, 1, 2, 2), _form(0, 4, 1, 2, 4, req_ring=3), _form(0, 8, 1, 2, 4),
          _form(0, 2, 1, 1, 2), _form(0, 4, 1, 1, 2, req_ring=4), _form(0, 8, 1, 1, 2),
          # K-part tiles: ring 2 except 2 x 2 waves at 128 rows
          _form(0, 1, 2, 4, 2), _form(0, 2, 2, 4, 2), _form(0, 4, 2, 4, 2, req_ring=3), _form(0, 5, 2, 4, 2), _form(0, 2, 2, 4, 3),
          _form(0, 1, 2, 2, 2), _form(0, 2, 2, 2, 2), _form(0, 4, 2, 2, 2),
          _form(0, 1, 2, 1, 2), _form(0, 2, 2, 1, 2), _form(0, 4, 2, 1, 2)]
    return f


def _fp8_forms(wt):
    """BD_CASE8 (wt 1: ring 2) / BD_CASE8A (wt 2) / BD_CASE4A (wt 3): ring 4, and the 256-row pass (4, 1, 8) that the two take only
    at one slice with the bf16 epilogue (every other call at RB = 8 runs the (4, 1, 4) form over two row tiles)."""
    ring = 2 if wt == 1 else 4
    f = [_form(wt, 4, 1, 8, ring, note="MB = 8 only at S = 1 with the bf16 epilogue")] if wt >= 2 else []
    tiles4 = ((4, 1), (8, 1), (10, 1), (2, 1), (4, 2), (2, 2)) if wt == 1 else ((4, 1), (8, 1), (2, 1), (4, 2), (2, 2))
    for mb in (4, 2, 1):
        for np_, kw in (tiles4 if mb == 4 else ((4, 1), (8, 1), (2, 1), (4, 2), (2, 2))):
            f.append(_form(wt, np_, kw, mb, ring))
    return f


FORMS = _bf16_forms() + _fp8_forms(1) + _fp8_forms(2) + _fp8_forms(3)

# The three big-tile kernels (bf16 weights, nw = 8, RB % 8 == 0), selected by process-wide options (restored by the tests)
BIG_FORMS = ([types.SimpleNamespace(kernel="wide", opts={"wide.ring": r, "wide.xcd": x}, id=f"wide-ring{r}-xcd{x}") for r in (2, 3) for x in (0, 1)]
             + [types.SimpleNamespace(kernel="half", opts={"half": 2, "half.form": v}, id=f"half-form{v}") for v in (0, 1, 4, 12)]
             + [types.SimpleNamespace(kernel="tile", opts={"tile": v}, id=f"tile-{v}") for v in (2, 3, 4)])
OPTION_DEFAULTS = {"wide.ring": 2, "wide.xcd": -1, "half": 1, "half.form": 1, "tile": 1}


def form_ns(f):
    """Output widths of a form: two tiles; the ragged bf16 forms also one panel less.  The bf16 (8, 1, 8) form too: at N % 256 == 0
    bdk_gemm sends its slab, bf16 and SwiGLU calls to gemm_wide_kernel, and only a width that is no multiple of 256 (N = 480, a ragged
    second tile) launches gemm_kernel<8, 1, 8> with those epilogues."""
    ns = [2 * 32 * f.np]
    if f.wt == 0 and ((f.np in (5, 9, 10) and (f.kw == 1 or f.np == 5)) or (f.np, f.kw, f.mb) == (8, 1, 8)):
        ns.append(32 * (2 * f.np - 1))
    return ns


def empty_split(stages, S):
    q = (stages + S - 1) // S
    return (S - 1) * q >= stages


def slice_ranges(stages, S):
    """[first, end) stage range of every K slice: q = ceil(stages / S) stages each, the last one what is left (bd_gemm_kernel.h:
    st0 = s * q, nst = min(q, stages - st0); bd_gemm_empty_split refuses a split whose last slice would be empty)."""
    q = (stages + S - 1) // S
    return [(s * q, min(s * q + q, stages)) for s in range(S)]


def refused(f, N, stages, S, epi):
    """The launcher rules under which a generic-form call returns an error before it launches."""
    nw = f.np * f.kw
    if empty_split(stages, S):
        return True
    if f.wt >= 1 and N % (32 * f.np):
        return True
    if epi != EPI_PARTIAL and S > 1:
        if f.wt == 0 and nw >= 9 and f.kw == 1:
            return True                                              # single-slice tiles only
        if f.wt == 1 and nw == 10 and f.kw == 1:
            return True
        if (N // 32) % f.np:
            return True                                              # the in-launch reduction indexes its slabs by whole tiles
    return False


# ---------------------------------------------------------------------------------------------------------------------------------
# host-side operand writers (index arithmetic per element, scattered into a flat buffer)
def _rk(rows, K):
    return torch.arange(rows)[:, None].expand(rows, K), torch.arange(K)[None, :].expand(rows, K)


def _scatter(size, off, val, dtype):
    buf = torch.zeros(size, dtype=dtype)
    buf[off.reshape(-1)] = val.reshape(-1).to(dtype)
    return buf


def afrag_off(r, k, RB):
    return ((((k >> 4) * RB + (r >> 5)) * 64) + ((r & 31) + (((k >> 3) & 1) << 5))) * 8 + (k & 7)


def a8_off(r, k, RB):
    return (((((k >> 6) * RB + (r >> 5)) * 2 + ((k >> 4) & 1)) * 64) + ((r & 31) + (((k >> 5) & 1) << 5))) * 16 + (k & 15)


def write_afrag(a, RB):
    """[rows][K] -> fragment-major flat [RB * 32 * K] of a's dtype (rows past a's stay zero)."""
    r, k = _rk(*a.shape)
    return _scatter(RB * 32 * a.shape[1], afrag_off(r, k, RB), a, a.dtype)


def read_afrag(buf, rows, K, RB):
    r, k = _rk(rows, K)
    return buf[afrag_off(r, k, RB)]


def write_a8(codes, RB):
    r, k = _rk(*codes.shape)
    return _scatter(RB * 32 * codes.shape[1], a8_off(r, k, RB), codes, codes.dtype)


def read_a8(buf, rows, K, RB):
    r, k = _rk(rows, K)
    return buf[a8_off(r, k, RB)]


def interleave(gate, up):
    """Packed row order of a SwiGLU pair: panel p = gate rows 16 p .. + 15, then up rows 16 p .. + 15."""
    F, K = gate.shape
    return torch.stack([gate.view(F // 16, 16, K), up.view(F // 16, 16, K)], 1).reshape(2 * F, K)


def w_off(n, k, K, panels_total, stage_major=False, row0=0):
    pn, l, ks = (n + row0) >> 5, (n & 31) + (((k >> 3) & 1) << 5), k >> 4
    PS, SS = (256, panels_total * 256) if stage_major else ((K >> 4) * 64, 256)
    return (pn * PS + (ks >> 2) * SS + (ks & 3) * 64 + l) * 8 + (k & 7)


def write_w(w, rows_total=None, row0=0, stage_major=False, out=None):
    """bf16 weights [N][K] in packed-row order -> flat packed buffer (pack_w_kernel; `row0` / `rows_total`: dst_row0 stacking)."""
    N, K = w.shape
    rows_total = rows_total or N
    n, k = _rk(N, K)
    off = w_off(n, k, K, rows_total // 32, stage_major, row0)
    if out is None:
        out = torch.zeros(rows_total * K, dtype=w.dtype)
    out[off.reshape(-1)] = w.reshape(-1)
    return out


def read_w(buf, N, K, rows_total=None, row0=0, stage_major=False):
    n, k = _rk(N, K)
    return buf[w_off(n, k, K, (rows_total or N) // 32, stage_major, row0)]


def w8_off(n, k, K, row0=0):
    ks = k >> 4
    return ((((n + row0) >> 5) * (K >> 5) + (ks >> 1)) * 64 + (n & 31) + (((k >> 3) & 1) << 5)) * 16 + (ks & 1) * 8 + (k & 7)


def w8k_off(n, k, K, row0=0):
    return (((((n + row0) >> 5) * (K >> 6) + (k >> 6)) * 2 + ((k >> 4) & 1)) * 64 + (n & 31) + (((k >> 5) & 1) << 5)) * 16 + (k & 15)


def write_w8(codes, rows_total=None, row0=0, k64=False):
    """e4m3 bytes [N][K] -> the K = 16-pair order (pack_w8_kernel) or, k64, the K = 64 order (pack_w8k_kernel)."""
    N, K = codes.shape
    n, k = _rk(N, K)
    return _scatter((rows_total or N) * K, (w8k_off if k64 else w8_off)(n, k, K, row0), codes, codes.dtype)


def read_w8(buf, N, K, k64=False, row0=0):
    n, k = _rk(N, K)
    return buf[(w8k_off if k64 else w8_off)(n, k, K, row0)]


def nibbles_to_bytes(nib):
    """e2m1 codes [N][K] (one per element, 0 .. 15) -> source bytes [N][K / 2]: k = 2 b low nibble, 2 b + 1 high."""
    return (nib[:, 0::2] | (nib[:, 1::2] << 4)).to(torch.uint8)


def write_w4(nib, exps, rows_total=None, row0=0):
    """e2m1 codes [N][K] + E8M0 exponents [N][K / 32] -> (packed bytes flat, packed exponent bytes flat [panels][EG][64][4])."""
    N, K = nib.shape
    rows_total = rows_total or N
    KS, EG = K >> 6, ((K >> 6) + 3) >> 2
    src = nibbles_to_bytes(nib)
    n, b = _rk(N, K // 2)                                            # source byte b holds k = 2 b, 2 b + 1
    k = 2 * b
    off = ((((n + row0) >> 5) * KS + (k >> 6)) * 64 + (n & 31) + (((k >> 5) & 1) << 5)) * 16 + (b & 15)
    packed = _scatter(rows_total * K // 2, off, src, torch.uint8)
    n, blk = _rk(N, K // 32)
    st = blk >> 1
    eoff = ((((n + row0) >> 5) * EG + (st >> 2)) * 64 + (n & 31) + ((blk & 1) << 5)) * 4 + (st & 3)
    pe = torch.full((rows_total // 32 * EG * 64 * 4,), 127, dtype=torch.uint8)
    if row0 or rows_total != N:
        pe.zero_()                                                   # (stacking: the other rows' dwords are not this call's)
        pe.view(rows_total // 32, EG, 64, 4)[row0 // 32:(row0 + N) // 32] = 127
    pe[eoff.reshape(-1)] = exps.reshape(-1).to(torch.uint8)
    return packed, pe


def read_w4(packed, pe, N, K):
    n, k = _rk(N, K)
    b = k >> 1
    byte = packed[((((n >> 5) * (K >> 6) + (k >> 6)) * 64 + (n & 31) + (((k >> 5) & 1) << 5)) * 16 + (b & 15))]
    nib = torch.where((k & 1) == 1, byte >> 4, byte & 15)
    n, blk = _rk(N, K // 32)
    st, EG = blk >> 1, ((K >> 6) + 3) >> 2
    return nib, pe[(((n >> 5) * EG + (st >> 2)) * 64 + (n & 31) + ((blk & 1) << 5)) * 4 + (st & 3)]


def e4m3(x):
    """Integer-valued tensor -> e4m3 bytes (exact for the probe values)."""
    b = x.float().to(torch.float8_e4m3fn)
    assert torch.equal(b.float(), x.float())
    return b.view(torch.uint8)


# ---------------------------------------------------------------------------------------------------------------------------------
class Probe:
    """One seeded operand pair at the largest K.  wt: 0 bf16 x bf16, 1 bf16 x e4m3, 2 e4m3 x e4m3, 3 e4m3 x e2m1 (MXFP4).  `stage` =
    k per stage count (64 kw; 32 for the tiled kernel).  All tensors on the CPU; .to(dev) moves what the references use."""

    def __init__(self, wt, rows, N, stage, nstage=NSTAGE, seed=0):
        g = torch.Generator().manual_seed(1000 + seed)
        K = stage * nstage
        self.wt, self.rows, self.N, self.stage, self.nstage, self.K = wt, rows, N, stage, nstage, K
        sgn = lambda shape: torch.randint(0, 2, shape, generator=g) * 2 - 1
        self.a_code = (torch.randint(1, 8, (rows, K), generator=g) * sgn((rows, K))).to(torch.int8)
        r, c = torch.arange(rows), torch.arange(N)
        # per-row activation scales (e4m3 activations): differ between r and r +- 1, r +- 4
        self.a_exp = -(((r >> 2) + r) % 3) if wt >= 2 else torch.zeros(rows, dtype=torch.int64)
        if wt == 3:
            mag = torch.randint(1, 6, (N, K), generator=g)            # e2m1 0.5, 1, 1.5, 2, 3
            self.w_nib = (mag | (torch.randint(0, 2, (N, K), generator=g) << 3)).to(torch.uint8)
            self.w_code = torch.tensor(E2M1)[mag] * (1 - 2 * (self.w_nib >> 3).float())
            blk = torch.arange(K // 32)
            self.w_bexp = -5 + (blk[None, :] + c[:, None]) % 3        # block exponents: differ block to block and row to row
            self.w_exp = None
            wq, wmax = 0.5 * 2.0 ** -5, 3 * 2.0 ** -3
        else:
            self.w_code = (torch.randint(1, 16, (N, K), generator=g) * sgn((N, K))).float()
            self.w_exp = (-7 + 0 * c) if wt == 0 else -(6 + c % 3)   # bf16: one quantum; e4m3: per-channel scales, c vs c +- 1 differ
            self.w_bexp = None
            wq, wmax = 2.0 ** int(self.w_exp.min()), 15 * 2.0 ** int(self.w_exp.max())
        # the bias: a bf16-exact multiple of 2^-9 below 0.5, so that sum + bias needs a real rounding from the first stage on
        self.bias = (torch.randint(1, 256, (N,), generator=g) * sgn((N,))).float() / 512
        self.gate = (c & 16) == 0
        # gate shift per stage count: the gate pre-activation's standard deviation ~ 2
        sd = self.a_real(torch.float64).std().item() * self.w_real(torch.float64).std().item()
        self.gshift = [0] + [max(-6, min(6, round(math.log2(2.0 / (sd * math.sqrt(n * stage)))))) for n in range(1, nstage + 1)]
        # every partial sum, and sum + bias, of every case fits 24 bits of the finest quantum in play (gate and up columns apart)
        aq, amax = 2.0 ** int(self.a_exp.min()), 7.0
        self.bits = 0.0
        for n in range(1, nstage + 1):
            for sh in (self.gshift[n], 0):
                worst = n * stage * amax * wmax * 2.0 ** sh + 0.5
                self.bits = max(self.bits, math.log2(worst / min(aq * wq * 2.0 ** sh, 2.0 ** -9)))
        assert self.bits < 24, self.bits

    def to(self, dev):
        p = object.__new__(Probe)
        p.__dict__ = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in self.__dict__.items()}
        return p

    # -- real values
    def a_real(self, dtype, fault=None):
        e = self.a_exp
        if fault in ("row_scale_r+4", "row_scale_r-4"):             # row r multiplied by the scale of row r + 4 / r - 4
            e = torch.roll(e, -4 if fault.endswith("+4") else 4)
        return self.a_code.to(dtype) * torch.exp2(e.to(dtype))[:, None]

    def w_real(self, dtype, fault=None):
        """Without the gate shift (colmul applies it to the products)."""
        if self.wt == 3:
            e = self.w_bexp
            if fault in ("block_exp_next", "block_exp_prev"):       # a block scaled by its neighbour's exponent
                e = torch.roll(e, -1 if fault.endswith("next") else 1, dims=1)
            return self.w_code.to(dtype) * torch.exp2(e.to(dtype)).repeat_interleave(32, dim=1)
        e = self.w_exp
        if fault in ("col_scale_c+1", "col_scale_c-1"):
            e = torch.roll(e, -1 if fault.endswith("+1") else 1)
        return self.w_code.to(dtype) * torch.exp2(e.to(dtype))[:, None]

    def colmul(self, n, dtype=torch.float64):
        return torch.where(self.gate, 2.0 ** self.gshift[n], 1.0).to(dtype)

    def prefix(self, dtype=torch.float64):
        """C[n] = A[:, :n stage] @ W[:, :n stage]^T for n = 0 .. nstage, [nstage + 1][rows][N] (exact in float64)."""
        a = self.a_real(dtype).view(self.rows, self.nstage, self.stage)
        w = self.w_real(dtype).view(self.N, self.nstage, self.stage)
        per = torch.einsum("rsk,nsk->srn", a, w)
        return torch.cat([torch.zeros_like(per[:1]), per.cumsum(0)])


def slab(C, p, n, lo, hi):
    """The exact product over stages [lo, hi) of the n-stage case."""
    return (C[hi] - C[lo]) * p.colmul(n, C.dtype)


def ref_bf16(v, bias, fault=None):
    """bf16(sum + bias): one rounding."""
    if fault == "drop_bias":
        return v.to(BF16)
    if fault == "bias_after_round":
        return (v.to(BF16).to(v.dtype) + bias).to(BF16)
    if fault == "second_rounding":
        return (v + bias).to(torch.float16).to(BF16)
    return (v + bias).to(BF16)


def swiglu_case(p, v, fault=None):
    """rows_ref's SwiGLU case of a finished Linear output v [rows][N] (one fp32 slab + the bf16 bias, interleaved columns)."""
    if fault == "swap_gate_up":
        c = torch.arange(v.shape[1], device=v.device)
        v = v[:, c ^ 16]
    return rr.case(M=v.shape[0], F=v.shape[1] // 2, S=1, up=v.float()[None], bias=p.bias.to(BF16), interleaved=1)


def judge_swiglu(p, v, act, what):
    """act: row-major bf16 [rows][F] (un-fragmented).  Reference: rows_ref.ref_swiglu on the exact Linear output."""
    return rr.judge_swiglu(swiglu_case(p, v), dict(act=act), what)


# ---------------------------------------------------------------------------------------------------------------------------------
# A plain emulation of one call, with the faults the CPU test proves detectable.  dtype float32 = the precision check (the sum is
# taken over shuffled 16-wide chunks, per slice, with the kw = 2 split); float64 = the reference.
FAULTS = ("hazard_rows_27_31", "drop_product", "swap_slabs", "drop_slab", "drop_bias", "bias_after_round", "second_rounding",
          "col_scale_c+1", "col_scale_c-1", "row_scale_r+4", "row_scale_r-4", "block_exp_next", "block_exp_prev", "swap_gate_up",
          "plain_columns")


def fault_applies(p, S, epi, fault):
    if fault == "drop_product":                                       # one small term: a rounded output may hide it, an fp32 one cannot
        return epi in (EPI_PARTIAL, EPI_F32)
    if fault == "swap_slabs":
        return S >= 2 and epi == EPI_PARTIAL
    if fault == "drop_slab":
        return S >= 2 and epi != EPI_PARTIAL
    if fault in ("drop_bias", "bias_after_round", "second_rounding"):
        return epi == EPI_BF16
    if fault.startswith("col_scale"):
        return p.wt in (1, 2)
    if fault.startswith("row_scale"):
        return p.wt >= 2
    if fault.startswith("block_exp"):
        return p.wt == 3
    if fault in ("swap_gate_up", "plain_columns"):
        return epi == EPI_SWIGLU
    return True


def emulate(p, n, S, epi, dtype=torch.float64, fault=None, kw=1, seed=0):
    """-> slabs [S][rows][N] (EPI_PARTIAL), the fp32 sum (EPI_F32), bf16 [rows][N] (EPI_BF16) or the bf16 SwiGLU output [rows][F]."""
    K = n * p.stage
    a, w = p.a_real(dtype, fault)[:, :K], p.w_real(dtype, fault)[:, :K] * p.colmul(n, dtype)[:, None]
    g = torch.Generator().manual_seed(seed)
    k16 = 16 if p.wt < 2 else 64                                       # depth of one MFMA

    def product(lo, hi):
        """sum over k in [lo, hi): one accumulator per K part, chunks of one MFMA in a shuffled order, parts added at the end."""
        parts = []
        for part in range(kw):
            acc = torch.zeros(p.rows, p.N, dtype=dtype)
            ch = [c for c in range(lo, hi, k16) if ((c - lo) // 64) % kw == part]
            if dtype == torch.float32:
                ch = [ch[i] for i in torch.randperm(len(ch), generator=g).tolist()]
            for c in ch:
                t = a[:, c:c + k16] @ w[:, c:c + k16].t()
                if fault == "hazard_rows_27_31" and c == K - k16:      # the last MFMA of the last stage, rows 27 / 31 of the last block
                    t[[p.rows - 5, p.rows - 1]] = 0
                if fault == "drop_product" and c == lo and lo == 0 and part == 0:
                    t[3, 5] -= a[3, 2] * w[5, 2]
                acc = acc + t
            parts.append(acc)
        return sum(parts[1:], parts[0])

    slabs = [product(lo * p.stage, hi * p.stage) for lo, hi in slice_ranges(n, S)]
    if epi == EPI_PARTIAL:
        if fault == "swap_slabs":
            slabs[0], slabs[1] = slabs[1], slabs[0]
        return torch.stack(slabs)
    if fault == "drop_slab":
        slabs = slabs[:-1]
    v = sum(slabs[1:], slabs[0])
    if epi == EPI_F32:
        return v
    if epi == EPI_BF16:
        return ref_bf16(v, p.bias.to(dtype), fault)
    c = swiglu_case(p, v, fault)
    return rr.ref_swiglu(c, dtype, "plain_columns" if fault == "plain_columns" else None)["o"].to(BF16)
