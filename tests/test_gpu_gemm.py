"""Every dispatched tile form of the Linear GEMMs through every K-stage count, bit for bit on exact probes (tests/gemm_ref.py).

One parametrized test per entry of gemm_ref.FORMS -- every gemm_kernel<NP, KW, MB, EPI, R, RED, MODE, WT> tile form that bdk_gemm,
bdk_gemm8, bdk_gemm8a and bdk_gemm4a dispatch (tests/test_gemm_ref_cpu.py keeps the table equal to the BD_CASE* lines) -- at
RB = the form's MB and N = two tiles (the ragged bf16 forms also at one panel less; so is the bf16 (8, 1, 8) form, whose slab, bf16
and SwiGLU calls run gemm_wide_kernel at N % 256 == 0 and launch gemm_kernel<8, 1, 8> only at a width like 480):
  S = 1      stage counts 1 .. 30 through the slab, SwiGLU, bf16(+bias) and fp32-sum epilogues;
  S = 2, 3   stage counts S .. 30 through the slab epilogue and the in-launch-reduced bf16 / fp32 / SwiGLU epilogues, with scratch and
             zeroed counters.
Every launch runs twice on the same counters, which must read zero after each.  The operands are the host writers' (no device pack
kernel is involved), sliced by K prefix from one seeded pair per form.  Checks, with no tolerance: every slab equals the float64
product of its own K range (read off bd_gemm_kernel.h: gemm_ref.slice_ranges), the fp32 sum equals the float64 product, the bf16
output equals bf16(product + bias); all by their bits (a NaN or a lost sign of zero differs), because every fp32 partial sum of a probe is exact in any order.  The fused
SwiGLU goes through hardware exp2 / rcp and is held to rows_ref.ref_swiglu's bound (a) and its 1 % flip cap.  Every output is NaN
before the call with a NaN guard block behind it; the guard must be intact and a compared output cannot keep a NaN.  Where a
launcher rule refuses a call (an empty split, the single-slice 9 / 10-wave tiles, N % (32 np) for the fp8 / fp4 launchers, a ragged
tile under the in-launch reduction) the error return and an untouched output are asserted instead.

The three big-tile kernels run at their smallest shapes under every value of their options (restored in `finally`):
gemm_wide_kernel (RB 8, N 256, K = 64 n, n = 1 .. 30; RB 16 for the two-slice reduced epilogues), gemm_half_kernel (RB 16, N 128 and
256, at least two stages per slice), gemm_tile_kernel (RB 32, N 4096, K = 32 n, n = 1 .. 36: the odd n are refused by the launcher's
K % 64 rule, S = 1 .. 3 on slabs).  The pack and layout kernels are compared with the host writers bit for bit.

Not launched here: the operand-wait and push forms (GemmCall::wait / push), which poll a peer's flags (tests/test_gpu_tp.py).

The half / tile launchers' own "S > 1 needs the slab epilogue" rule cannot be reached through the entry points: bdk_gemm routes such
a call to the 256-row or the generic kernel, where the sweeps above run it.

Measured on an MI355X (each case prints a line "GEMMSTAT": launches, seconds, the worst SwiGLU flip share; `pytest -s`):
  worst SwiGLU flip share (cap 1e-2): bf16 weights 1.5e-3, fp8 9.8e-4, fp8a 9.8e-4, fp4a 1.2e-3 -- one to three elements of a
  32 .. 256-row case; no element further than bound (a) allows;
  every slab, fp32 sum and bf16 output of all 84 tile forms and the three big-tile kernels equal to the float64 reference bit for
  bit, at every stage count: no kernel fault was found;
  64 068 launches in all (688 per tile form and width; fewer at a ragged width, where the reduced epilogues are refused); the
  slowest parametrized case takes 0.6 .. 1.4 s (the first one, which loads the library), every other one at most 0.4 s, the whole
  module (100 tests) 21 .. 23 s.
"""
from __future__ import annotations

import contextlib
import time

import pytest
import torch

from tests import gemm_ref as gr
from tests import rows_ref as rr
from tests.gemm_ref import EPI_BF16, EPI_F32, EPI_PARTIAL, EPI_SWIGLU
from tests.rows_ref import BF16

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
GUARD = 256
EPI_NAME = {EPI_PARTIAL: "slabs", EPI_SWIGLU: "swiglu", EPI_BF16: "bf16", EPI_F32: "f32"}


def _lib():
    from bitdance_amd._lib import lib
    return lib()


def _check(rc, what):
    from bitdance_amd._lib import check
    check(rc, what)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


class Operands:
    """The device operands of one probe at its largest K, written by the host writers, and their K-prefix slices."""

    def __init__(self, p, RB):
        self.p, self.RB, self.wt = p, RB, p.wt
        N, K = p.N, p.K
        lane_gate = (torch.arange(64) & 31) < 16                      # the lanes that hold gate rows (packed row & 16 == 0)
        self.lane_gate = lane_gate.to(DEV)
        if p.wt < 2:
            self.A = gr.write_afrag(p.a_real(torch.float32).to(BF16), RB).to(DEV)
            self.ascale = None
        else:
            self.A = gr.write_a8(gr.e4m3(p.a_code), RB).to(DEV)
            self.ascale = torch.exp2(p.a_exp.float()).to(DEV)
        if p.wt == 0:
            self.W = gr.write_w(p.w_real(torch.float32).to(BF16)).view(N // 32, K // 16, 64, 8).to(DEV)
        elif p.wt == 1:
            self.W = gr.write_w8(gr.e4m3(p.w_code)).view(N // 32, K // 32, 64, 16).to(DEV)
        elif p.wt == 2:
            self.W = gr.write_w8(gr.e4m3(p.w_code), k64=True).view(N // 32, K // 64, 2, 64, 16).to(DEV)
        else:
            pk, pe = gr.write_w4(p.w_nib, p.w_bexp + 127)
            self.W = pk.view(N // 32, K // 64, 64, 16).to(DEV)
            self.E = pe.view(N // 32, -1, 64, 4).to(DEV)
        if p.wt in (1, 2):
            self.wscale = torch.exp2(p.w_exp.double()).to(DEV)
        self.bias = p.bias.to(BF16).to(DEV)
        self.cache = {}

    def at(self, K, n):
        """(A, W, weight scale or exponent stream) of the K-deep prefix, with stage count n's gate shift."""
        if n in self.cache:
            return self.cache[n]
        p, g = self.p, self.p.gshift[n]
        A = self.A[: self.RB * 32 * K]                               # both activation layouts are K-major: a prefix
        sc = None
        if p.wt == 0:
            W = self.W[:, : K // 16].clone()
            W[:, :, self.lane_gate] = (W[:, :, self.lane_gate].float() * 2.0 ** g).to(BF16)
        elif p.wt == 1:
            W = self.W[:, : K // 32].contiguous()
        elif p.wt == 2:
            W = self.W[:, : K // 64].contiguous()
        else:
            KS = K // 64
            W = self.W[:, :KS].contiguous()
            e = self.E[:, : (KS + 3) // 4].to(torch.int32)
            e[:, :, self.lane_gate] += g
            stage = torch.arange(e.shape[1], device=DEV)[:, None, None] * 4 + torch.arange(4, device=DEV)[None, None, :]
            sc = torch.where(stage >= KS, 127, e).to(torch.uint8).contiguous()
        if p.wt in (1, 2):
            sc = (self.wscale * torch.where(p.gate.to(DEV), 2.0 ** g, 1.0)).float().contiguous()
        self.cache = {n: (A, W, sc)}                                  # (one entry: the callers walk n in order)
        return self.cache[n]


def launch(nw, ops, n_ops, RB, N, K, S, epi, out, scratch, cnt):
    """One call through the C entry point of (weight type, epilogue) -> return code."""
    L, st = _lib(), _stream()
    A, W, sc = n_ops
    b = _ptr(ops.bias)
    if ops.wt == 0:
        if epi == EPI_PARTIAL:
            return L.bd_gemm_partial(_ptr(A), RB, _ptr(W), N, K, S, nw, _ptr(out), st)
        if epi == EPI_BF16:
            return L.bd_gemm_bf16(_ptr(A), RB, _ptr(W), b, N, K, S, nw, _ptr(scratch), _ptr(cnt), _ptr(out), st)
        if epi == EPI_F32:
            return L.bd_gemm_f32(_ptr(A), RB, _ptr(W), N, K, S, nw, _ptr(scratch), _ptr(cnt), _ptr(out), st)
        if S == 1:
            return L.bd_gemm_swiglu(_ptr(A), RB, _ptr(W), b, N, K, nw, _ptr(out), st)
        return L.bd_gemm_swiglu_splitk(_ptr(A), RB, _ptr(W), b, N, K, S, nw, _ptr(scratch), _ptr(cnt), _ptr(out), st)
    if ops.wt == 1:
        return L.bd_gemm_w8(_ptr(A), RB, _ptr(W), _ptr(sc), b, N, K, S, nw, epi, _ptr(scratch), _ptr(cnt), _ptr(out), st)
    fn = L.bd_gemm_w8a8 if ops.wt == 2 else L.bd_gemm_w4a8
    return fn(_ptr(A), _ptr(ops.ascale), RB, _ptr(W), _ptr(sc), b, N, K, S, nw, epi, _ptr(scratch), _ptr(cnt), _ptr(out), st)


class Sweep:
    """Runs the calls of one probe and collects the verdicts on the device; `finish` reads them back once."""

    def __init__(self, what, p, RB):
        self.what, self.p, self.RB = what, p, RB
        self.dp = p.to(DEV)
        self.C = self.dp.prefix()
        self.ops = Operands(p, RB)
        self.cnt = torch.zeros(16384, dtype=torch.int32, device=DEV)
        self.flags, self.desc, self.fail = [], [], []
        self.launches, self.flip = 0, 0.0
        self.t0 = time.time()

    def _flag(self, bad, desc, mism=None):
        self.flags.append(bad)
        self.desc.append((desc, mism))

    def call(self, nw, n, S, epi, refuse, ranges=None):
        """The n-stage case through S slices and one epilogue, twice.  `refuse`: the launcher must return an error and leave the
        output alone."""
        p, rows, N = self.p, self.RB * 32, self.p.N
        K = n * p.stage
        tag = f"{self.what} n={n} S={S} {EPI_NAME[epi]}"
        numel = {EPI_PARTIAL: S * rows * N, EPI_F32: rows * N, EPI_BF16: rows * N, EPI_SWIGLU: rows * N // 2}[epi]
        dtype = torch.float32 if epi in (EPI_PARTIAL, EPI_F32) else BF16
        n_ops = self.ops.at(K, n)
        scratch = torch.empty(S * rows * N, dtype=torch.float32, device=DEV) if (S > 1 and epi != EPI_PARTIAL) else None
        full = gr.slab(self.C, self.dp, n, 0, n)
        for run in range(2):
            buf = torch.full((numel + GUARD,), NAN, dtype=dtype, device=DEV)
            out = buf[:numel]
            rc = launch(nw, self.ops, n_ops, self.RB, N, K, S, epi, out, scratch, self.cnt)
            if refuse:
                assert rc != 0, f"{tag}: the launcher accepted a call its rules refuse"
                self._flag((~torch.isnan(buf)).any(), f"{tag}: a refused call wrote its output")
                return
            assert rc == 0, f"{tag}: rc {rc}: {_lib().bd_last_error().decode()}"
            self.launches += 1
            self._flag((~torch.isnan(buf[numel:])).any() | (self.cnt != 0).any(), f"{tag} run {run}: guard block or counters touched")
            if epi == EPI_PARTIAL:
                ref = torch.stack([gr.slab(self.C, self.dp, n, lo, hi) for lo, hi in (ranges or gr.slice_ranges(n, S))]).float()
                mism = out.view(torch.int32).view(S, rows, N) != ref.view(torch.int32)      # bits: a NaN or a lost sign of zero differs too
            elif epi == EPI_F32:
                mism = out.view(torch.int32).view(rows, N) != full.float().view(torch.int32)
            elif epi == EPI_BF16:
                mism = out.view(torch.int16).view(rows, N) != gr.ref_bf16(full, self.dp.bias.double()).view(torch.int16)
            else:
                rep = gr.judge_swiglu(self.dp, full, rr.unfrag(out, self.RB, N // 2), f"{tag} run {run}")
                self.fail += rep.fail
                self.flip = max(self.flip, rep.flip)
                continue
            self._flag(mism.any(), f"{tag} run {run}", mism)

    def finish(self):
        torch.cuda.synchronize()
        bad = torch.stack([f.reshape(()) for f in self.flags]).cpu().tolist() if self.flags else []
        for b, (desc, mism) in zip(bad, self.desc):
            if b:
                msg = desc
                if mism is not None:
                    idx = mism.nonzero()
                    rows_, cols = idx[:, -2].unique().tolist(), idx[:, -1].unique().tolist()
                    msg += f": {idx.shape[0]} elements differ; rows {rows_[:12]}{'...' if len(rows_) > 12 else ''} cols {cols[:12]}{'...' if len(cols) > 12 else ''}"
                self.fail.append(msg)
        print(f"GEMMSTAT {self.what} launches={self.launches} seconds={time.time() - self.t0:.2f} swiglu_flip={self.flip:.3e} bits={self.p.bits:.1f}")
        return self.fail


def _report(fails):
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])


@pytest.mark.parametrize("f", gr.FORMS, ids=[f.id for f in gr.FORMS])
def test_form_every_stage_count(f):
    fails = []
    for N in gr.form_ns(f):
        p = gr.Probe(f.wt, 32 * f.rb, N, 64 * f.kw, seed=gr.FORMS.index(f) * 2 + (N != 64 * f.np))
        sw = Sweep(f"{f.id} N={N}", p, f.rb)
        for S in (1, 2, 3):
            for n in range(S, gr.NSTAGE + 1):
                for epi in gr.EPIS:
                    sw.call(f.nw, n, S, epi, gr.refused(f, N, n, S, epi))
        fails += sw.finish()
    _report(fails)


@pytest.mark.parametrize("wt", (1, 2, 3))
def test_fp8_launchers_refuse_a_ragged_tile(wt):
    """N % (32 np) != 0: bdk_gemm8 / bdk_gemm8a / bdk_gemm4a have no ragged last tile; every epilogue returns an error, nothing is written."""
    f = next(f for f in gr.FORMS if (f.wt, f.np, f.kw, f.mb) == (wt, 4, 1, 4))
    N = 32 * (2 * f.np - 1)
    sw = Sweep(f"{f.id} N={N}", gr.Probe(wt, 32 * f.rb, N, 64, nstage=2, seed=930 + wt), f.rb)
    for epi in gr.EPIS:
        assert gr.refused(f, N, 2, 1, epi)
        sw.call(f.nw, 2, 1, epi, True)
    _report(sw.finish())
    assert sw.launches == 0


@contextlib.contextmanager
def _options(opts):
    """Process-wide GEMM options for the body; every one is back at its default afterwards, also when setting one of them fails."""
    try:
        for k, v in opts.items():
            _check(_lib().bd_set_gemm_option(k.encode(), v), k)
        yield
    finally:
        for k in opts:
            _check(_lib().bd_set_gemm_option(k.encode(), gr.OPTION_DEFAULTS[k]), k)


@pytest.mark.parametrize("b", gr.BIG_FORMS, ids=[b.id for b in gr.BIG_FORMS])
def test_big_tile_kernels(b):
    fails = []
    with _options(b.opts):
        if b.kernel == "wide":
            # RB 8: one slice through slabs / bf16 / SwiGLU, 2 and 3 slices on slabs; RB 16 (two row tiles: the XCD placement applies):
            # the same plus the two-slice reduced bf16 / SwiGLU epilogues
            for RB in (8, 16):
                sw = Sweep(f"{b.id} RB={RB}", gr.Probe(0, 32 * RB, 256, 64, seed=900 + RB), RB)
                for S in (1, 2, 3):
                    for n in range(S, gr.NSTAGE + 1):
                        epis = [EPI_PARTIAL] + ([EPI_SWIGLU, EPI_BF16] if S == 1 or (S == 2 and RB == 16) else [])
                        for epi in epis:
                            sw.call(8, n, S, epi, gr.empty_split(n, S))
                fails += sw.finish()
        elif b.kernel == "half":
            for N in (128, 256):
                sw = Sweep(f"{b.id} N={N}", gr.Probe(0, 512, N, 64, seed=910 + N), 16)
                for S in (1, 2, 3):
                    for n in range(2 * S, gr.NSTAGE + 1):              # (n // S >= 2: what bdk_gemm routes to this kernel)
                        q = (n + S - 1) // S
                        refuse = (S - 1) * q >= n or n - (S - 1) * q < 2 or q < 2
                        for epi in [EPI_PARTIAL] + ([EPI_SWIGLU, EPI_BF16] if S == 1 else []):
                            sw.call(8, n, S, epi, refuse)
                fails += sw.finish()
        else:
            sw = Sweep(b.id, gr.Probe(0, 1024, 4096, 32, nstage=36, seed=920), 32)
            for S in (1, 2, 3):
                for n in range(S, 37):                                  # 32-deep stages; the launcher wants K % 64 == 0
                    refuse = n % 2 == 1 or gr.empty_split(n // 2, S) or gr.empty_split(n, S)
                    for epi in [EPI_PARTIAL] + ([EPI_SWIGLU, EPI_BF16] if S == 1 else []):
                        sw.call(8, n, S, epi, refuse)
            fails += sw.finish()
    _report(fails)


# ---------------------------------------------------------------------------------------------------------------------------------
# the pack and layout kernels against the host writers
def _eq(a, b, what):
    a, b = a.cpu(), b.cpu()
    view = {2: torch.int16, 4: torch.int32, 1: torch.uint8}[a.element_size()]
    assert a.shape == b.shape and torch.equal(a.view(view), b.view(view)), f"{what}: {(a.view(view) != b.view(view)).sum().item()} units differ"


def test_rows_to_frag_and_quant_rows8():
    L, st = _lib(), _stream()
    g = torch.Generator().manual_seed(3)
    M, K, RB = 70, 192, 3
    x = torch.randn(M, K, generator=g)
    for src in (x, x.to(BF16)):
        out = torch.zeros(RB * 32 * K, dtype=BF16, device=DEV)
        d = src.to(DEV)
        _check(L.bd_rows_to_frag(out.data_ptr(), d.data_ptr(), int(src.dtype == torch.float32), M, K, RB, st), "bd_rows_to_frag")
        _eq(out, gr.write_afrag(src.to(BF16), RB), f"bd_rows_to_frag {src.dtype}")
    # rows with amax = 3.5: the row scale is exactly 2^-7 and every code exact; one zero row (scale 0, codes 0)
    v = (torch.randint(1, 4, (M, K), generator=g) * (torch.randint(0, 2, (M, K), generator=g) * 2 - 1)).float()
    v[torch.arange(M), torch.randint(0, K, (M,), generator=g)] = 3.5
    v[1::2] *= -1
    v[5] = 0
    a8 = torch.zeros(RB * 32 * K, dtype=torch.uint8, device=DEV)
    sc = torch.full((RB * 32,), NAN, device=DEV)
    d = v.to(DEV)
    _check(L.bd_quant_rows8(a8.data_ptr(), sc.data_ptr(), d.data_ptr(), M, K, RB, st), "bd_quant_rows8")
    want_sc = torch.full((M,), 2.0 ** -7)
    want_sc[5] = 0
    _eq(sc[:M], want_sc, "bd_quant_rows8 scales")
    assert torch.isnan(sc[M:]).all()
    _eq(a8, gr.write_a8((v * 128).to(torch.float8_e4m3fn).view(torch.uint8), RB), "bd_quant_rows8 codes")


def test_pack_weight_kernels():
    L, st = _lib(), _stream()
    g = torch.Generator().manual_seed(4)
    N, K = 160, 192
    w = torch.randn(N, K, generator=g).to(BF16)
    d = w.to(DEV)
    try:
        for sm in (0, 1):
            _check(L.bd_set_weight_layout(sm), "layout")
            out = torch.zeros(N * K, dtype=BF16, device=DEV)
            _check(L.bd_pack_weight(out.data_ptr(), d.data_ptr(), N, K, 0, N, st), "bd_pack_weight")
            _eq(out, gr.write_w(w, stage_major=bool(sm)), f"bd_pack_weight layout {sm}")
            out = torch.zeros(N * K, dtype=BF16, device=DEV)                       # two calls stacked by dst_row0
            _check(L.bd_pack_weight(out.data_ptr(), d[:64].contiguous().data_ptr(), 64, K, 0, N, st), "bd_pack_weight")
            _check(L.bd_pack_weight(out.data_ptr(), d[64:].contiguous().data_ptr(), N - 64, K, 64, N, st), "bd_pack_weight")
            _eq(out, gr.write_w(w, stage_major=bool(sm)), f"bd_pack_weight stacked, layout {sm}")
            out = torch.zeros(N * K, dtype=BF16, device=DEV)
            _check(L.bd_pack_weight_swiglu(out.data_ptr(), d[: N // 2].contiguous().data_ptr(), d[N // 2:].contiguous().data_ptr(), N // 2, K, st),
                   "bd_pack_weight_swiglu")
            _eq(out, gr.write_w(gr.interleave(w[: N // 2], w[N // 2:]), stage_major=bool(sm)), f"bd_pack_weight_swiglu layout {sm}")
    finally:
        L.bd_set_weight_layout(0)
    c = torch.randint(0, 256, (N, K), generator=g).to(torch.uint8)
    dc = c.to(DEV)
    for name, k64 in (("bd_pack_weight8", False), ("bd_pack_weight8k", True)):
        out = torch.zeros(N * K, dtype=torch.uint8, device=DEV)
        _check(getattr(L, name)(out.data_ptr(), dc[:96].contiguous().data_ptr(), 96, K, 0, N, st), name)
        _check(getattr(L, name)(out.data_ptr(), dc[96:].contiguous().data_ptr(), N - 96, K, 96, N, st), name)
        _eq(out, gr.write_w8(c, k64=k64), name)
        out = torch.zeros(N * K, dtype=torch.uint8, device=DEV)
        _check(getattr(L, name + "_swiglu")(out.data_ptr(), dc[: N // 2].contiguous().data_ptr(), dc[N // 2:].contiguous().data_ptr(), N // 2, K, st), name)
        _eq(out, gr.write_w8(gr.interleave(c[: N // 2], c[N // 2:]), k64=k64), name + "_swiglu")
    nib = torch.randint(0, 16, (N, K), generator=g).to(torch.uint8)
    ex = torch.randint(100, 140, (N, K // 32), generator=g).to(torch.uint8)
    src, dex = gr.nibbles_to_bytes(nib).to(DEV), ex.to(DEV)
    EG = (K // 64 + 3) // 4
    out = torch.zeros(N * K // 2, dtype=torch.uint8, device=DEV)
    oe = torch.zeros(N // 32 * EG * 64 * 4, dtype=torch.uint8, device=DEV)
    _check(L.bd_pack_weight4k(out.data_ptr(), oe.data_ptr(), src[:96].contiguous().data_ptr(), dex[:96].contiguous().data_ptr(), 96, K, 0, N, st), "bd_pack_weight4k")
    _check(L.bd_pack_weight4k(out.data_ptr(), oe.data_ptr(), src[96:].contiguous().data_ptr(), dex[96:].contiguous().data_ptr(), N - 96, K, 96, N, st), "bd_pack_weight4k")
    pk, pe = gr.write_w4(nib, ex)
    _eq(out, pk, "bd_pack_weight4k codes")
    _eq(oe, pe, "bd_pack_weight4k exponents")
    out.zero_(), oe.zero_()
    h = N // 2
    _check(L.bd_pack_weight4k_swiglu(out.data_ptr(), oe.data_ptr(), src[:h].contiguous().data_ptr(), dex[:h].contiguous().data_ptr(),
                                     src[h:].contiguous().data_ptr(), dex[h:].contiguous().data_ptr(), h, K, st), "bd_pack_weight4k_swiglu")
    pk, pe = gr.write_w4(gr.interleave(nib[:h], nib[h:]), gr.interleave(ex[:h], ex[h:]))
    _eq(out, pk, "bd_pack_weight4k_swiglu codes")
    _eq(oe, pe, "bd_pack_weight4k_swiglu exponents")
