"""The probes, writers, form table and references of tests/test_gpu_gemm.py, checked without a GPU (tests/gemm_ref.py holds them).

* exactness: a float32 evaluation of every probe family -- one accumulator per K part, MFMA-sized chunks added in a shuffled
  order, 1 to 3 slices, the kw = 2 split -- equals the float64 product bit for bit (slabs, the fp32 sum, the bf16(+bias) output);
* writers: every host-side operand writer inverts under rows_ref.unfrag / unfrag8 (activations) and under its own reader;
* table freshness: the form table lists exactly the BD_CASE / BD_CASE_PIPE / BD_CASE8 / BD_CASE8A / BD_CASE4A lines of the three
  launchers, so a new instantiation cannot go untested silently;
* faults: every fault of gemm_ref.FAULTS changes at least one output bit on the smallest probe it applies to (one stage and one
  row block; two stages for the faults that need two slices), and the SwiGLU judge rejects the SwiGLU ones;
* SwiGLU bounds: the float32 run of the SwiGLU reference stays inside rows_ref's bounds with a quarter of the flip cap.
"""
from __future__ import annotations

import os
import re

import pytest
import torch

from tests import gemm_ref as gr
from tests import rows_ref as rr

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bitdance_amd", "csrc")
WTS = (0, 1, 2, 3)


def bits(t):
    return t.view(torch.int16) if t.dtype == rr.BF16 else t


@pytest.mark.parametrize("wt", WTS)
def test_float32_evaluation_is_exact(wt):
    p = gr.Probe(wt, 64, 96, 128, nstage=gr.NSTAGE, seed=wt)
    assert p.bits < 24
    C = p.prefix()
    for n, S, kw in ((1, 1, 1), (1, 1, 2), (7, 2, 1), (15, 3, 2), (30, 1, 1), (30, 3, 2), (29, 2, 2)):
        ref = torch.stack([gr.slab(C, p, n, lo, hi) for lo, hi in gr.slice_ranges(n, S)])
        for seed in (0, 1):
            got = gr.emulate(p, n, S, gr.EPI_PARTIAL, torch.float32, kw=kw, seed=seed)
            assert got.dtype == torch.float32 and torch.equal(got.double(), ref), (n, S, kw)
        assert torch.equal(gr.emulate(p, n, S, gr.EPI_PARTIAL), ref)
        full = gr.slab(C, p, n, 0, n)
        assert torch.equal(gr.emulate(p, n, S, gr.EPI_F32, torch.float32, kw=kw, seed=2).double(), full)
        want = gr.ref_bf16(full, p.bias.double())
        assert torch.equal(bits(gr.emulate(p, n, S, gr.EPI_BF16, torch.float32, kw=kw, seed=3)), bits(want))
    # the probe is not trivial: a real share of the bf16 outputs needs a rounding, and every output sees its bias
    v = gr.slab(C, p, 30, 0, 30) + p.bias.double()
    assert (v.to(rr.BF16).double() != v).double().mean() > 0.2


@pytest.mark.parametrize("wt", WTS)
def test_swiglu_float32_inside_bounds(wt):
    p = gr.Probe(wt, 64, 128, 64, seed=10 + wt)
    C = p.prefix()
    for n in (1, 2, 9, 30):
        v = gr.slab(C, p, n, 0, n)
        h1 = (v + p.bias.double())[:, p.gate]
        assert (h1.abs() <= 8).double().mean() > 0.9 and (h1.abs() > 0.25).double().mean() > 0.5, n   # silu is neither x nor 0
        rep = gr.judge_swiglu(p, v, gr.emulate(p, n, 1, gr.EPI_SWIGLU, torch.float32), f"wt{wt} n{n} float32")
        assert not rep.fail, "\n".join(rep.fail)
        assert rep.flip <= rr.FLIP_CAP / 4, rep.line()


@pytest.mark.parametrize("wt", WTS)
def test_every_fault_changes_the_output(wt):
    seen = set()
    for n, S in ((1, 1), (2, 2)):                                   # one stage; two stages in two slices for the slab faults
        p = gr.Probe(wt, 32, 64, 64, nstage=2, seed=20 + wt)
        C = p.prefix()
        v = gr.slab(C, p, n, 0, n)
        for epi in gr.EPIS:
            good = gr.emulate(p, n, S, epi)
            for f in gr.FAULTS:
                if not gr.fault_applies(p, S, epi, f):
                    continue
                seen.add(f)
                bad = gr.emulate(p, n, S, epi, fault=f)
                assert not torch.equal(bits(bad), bits(good)), f"wt{wt} n{n} S{S} epi{epi}: the fault {f} changes no output bit"
                if epi == gr.EPI_SWIGLU:
                    rep = gr.judge_swiglu(p, v, bad, f"wt{wt} {f}")
                    assert rep.fail, f"wt{wt} n{n} S{S}: the SwiGLU bounds do not reject {f} ({rep.line()})"
    want = {f for f in gr.FAULTS if any(gr.fault_applies(gr.Probe(wt, 32, 64, 64, nstage=2), S, e, f) for S in (1, 2) for e in gr.EPIS)}
    assert seen == want


def test_every_fault_applies_to_some_weight_type():
    ps = [gr.Probe(wt, 32, 64, 64, nstage=2) for wt in WTS]
    for f in gr.FAULTS:
        assert any(gr.fault_applies(p, S, e, f) for p in ps for S in (1, 2) for e in gr.EPIS), f


def test_writers_invert():
    rb, K, N = 2, 192, 96
    rows = rb * 32
    a = (torch.arange(rows)[:, None] * 1000 + torch.arange(K)[None, :]).to(torch.int64)
    assert torch.equal(rr.unfrag(gr.write_afrag(a, rb), rb, K), a)
    assert torch.equal(gr.read_afrag(gr.write_afrag(a, rb), rows, K, rb), a)
    assert torch.equal(rr.unfrag8(gr.write_a8(a, rb), rb, K), a)
    assert torch.equal(gr.read_a8(gr.write_a8(a, rb), rows, K, rb), a)
    a40 = a[:40]                                                      # rows past M stay zero
    assert torch.equal(rr.unfrag(gr.write_afrag(a40, rb), rb, K)[40:], torch.zeros(rows - 40, K, dtype=torch.int64))
    w = (torch.arange(N)[:, None] * 1000 + torch.arange(K)[None, :]).to(torch.int64)
    for sm in (False, True):
        buf = gr.write_w(w, stage_major=sm)
        assert torch.equal(gr.read_w(buf, N, K, stage_major=sm), w) and sorted(buf.tolist()) == sorted(w.flatten().tolist())
        two = gr.write_w(w[32:], rows_total=N, row0=32, stage_major=sm, out=gr.write_w(w[:32], rows_total=N, stage_major=sm))
        assert torch.equal(two, buf)                                  # dst_row0 stacking = one call over all rows
    # panel-major bf16: unit (panel, ks, lane), 8 elements = row panel * 32 + (lane & 31), k = ks * 16 + (lane >> 5) * 8 + 0..7
    u = gr.write_w(w).view(N // 32, K // 16, 64, 8)
    assert u[2, 5, 37].tolist() == [(2 * 32 + 5) * 1000 + 5 * 16 + 8 + j for j in range(8)]
    for k64 in (False, True):
        buf = gr.write_w8(w, k64=k64)
        assert torch.equal(gr.read_w8(buf, N, K, k64=k64), w) and sorted(buf.tolist()) == sorted(w.flatten().tolist())
        # dst_row0 stacking: two calls into disjoint panels add up to the one call over all rows
        two = gr.write_w8(w[:32], rows_total=N, k64=k64) + gr.write_w8(w[32:], rows_total=N, row0=32, k64=k64)
        assert torch.equal(two, buf) and torch.equal(gr.read_w8(two, N - 32, K, k64=k64, row0=32), w[32:])
    u = gr.write_w8(w).view(N // 32, K // 32, 64, 16)                # lane's low 8 bytes = k-step 2 kp, high 8 = 2 kp + 1
    assert u[1, 2, 40].tolist() == [(32 + 8) * 1000 + k for k in list(range(64 + 8, 64 + 16)) + list(range(80 + 8, 80 + 16))]
    u = gr.write_w8(w, k64=True).view(N // 32, K // 64, 2, 64, 16)
    assert u[1, 2, 1, 40].tolist() == [(32 + 8) * 1000 + 128 + 32 + 16 + j for j in range(16)]
    gate, up = w[: N // 2], w[N // 2:] + 500000
    il = gr.interleave(gate, up)
    assert torch.equal(il[32:48], gate[16:32]) and torch.equal(il[48:64], up[16:32])
    g = torch.Generator().manual_seed(5)
    nib = torch.randint(0, 16, (N, K), generator=g).to(torch.uint8)
    ex = torch.randint(100, 140, (N, K // 32), generator=g).to(torch.uint8)
    pk, pe = gr.write_w4(nib, ex)
    n2, e2 = gr.read_w4(pk, pe, N, K)
    assert torch.equal(n2, nib) and torch.equal(e2, ex)
    d = pe.view(N // 32, 1, 64, 4)                                    # K = 192: three stages, the fourth byte of every dword is 2^0
    assert (d[..., 3] == 127).all() and d[1, 0, 37, 2] == ex[32 + 5, 2 * 2 + 1]
    lo, hi = gr.write_w4(nib[:64], ex[:64], rows_total=N), gr.write_w4(nib[64:], ex[64:], rows_total=N, row0=64)
    assert torch.equal(lo[0] + hi[0], pk) and torch.equal(lo[1] + hi[1], pe)          # stacked calls: disjoint panels, zero elsewhere
    assert (hi[1].view(N // 32, 1, 64, 4)[:2] == 0).all() and (hi[1].view(N // 32, 1, 64, 4)[2:, ..., 3] == 127).all()
    src = gr.nibbles_to_bytes(nib)
    assert pk.view(N // 32, K // 64, 64, 16)[1, 2, 37].tolist() == src[32 + 5, 2 * 32 + 16: 2 * 32 + 32].tolist()
    assert torch.equal(gr.e4m3(torch.tensor([1., -2., 3.])), torch.tensor([0x38, 0xC0, 0x44], dtype=torch.uint8))


def _cases(path, macro, n):
    src = open(os.path.join(CSRC, path)).read()
    return [tuple(int(x) for x in m) for m in re.findall(macro + r"\(" + ", *".join([r"(\d+)"] * n) + r"\)", src)]


def test_form_table_lists_exactly_the_dispatched_forms():
    want = []
    want += [(0, np_, kw, mb, r, 0) for np_, kw, mb, r in _cases("bd_gemm.hip", r"\bBD_CASE", 4)]
    want += [(0, np_, kw, mb, 2, 1) for np_, kw, mb in _cases("bd_gemm.hip", r"\bBD_CASE_PIPE", 3)]
    want += [(1, np_, kw, mb, 2, 0) for np_, kw, mb in _cases("bd_gemm8.hip", r"\bBD_CASE8", 3)]
    want += [(2, np_, kw, mb, 4, 0) for np_, kw, mb in _cases("bd_gemm8.hip", r"\bBD_CASE8A", 3)]
    want += [(3, np_, kw, mb, 4, 0) for np_, kw, mb in _cases("bd_gemm4.hip", r"\bBD_CASE4A", 3)]
    have = [(f.wt, f.np, f.kw, f.mb, f.ring, f.pipe) for f in gr.FORMS]
    assert len(want) == len(set(want)) and len(have) == len(set(have))
    assert set(have) == set(want), (sorted(set(want) - set(have)), sorted(set(have) - set(want)))
    assert len(want) >= 84
    # the ring / MODE the macros instantiate are what the table assumes
    for path, text in (("bd_gemm8.hip", "launch_gemm<NPV, KWV, MBV, 2, 0, 1>"), ("bd_gemm8.hip", "launch_gemm<NPV, KWV, MBV, 4, 0, 2>"),
                       ("bd_gemm4.hip", "launch_gemm<NPV, KWV, MBV, 4, 0, 3>"), ("bd_gemm.hip", "launch_gemm<NPV, KWV, MBV, 2, 1>"),
                       ("bd_gemm.hip", "launch_gemm<NPV, KWV, MBV, RV>")):
        assert text in open(os.path.join(CSRC, path)).read(), text
    # the nw code of an entry decodes to the entry (bdk_gemm's rewriting rules)
    for f in gr.FORMS:
        nw, ring, kw, pipe = f.nw & 15, (f.nw >> 4) & 15, ((f.nw >> 8) & 3) + 1, (f.nw >> 11) & 1
        assert (nw, kw, pipe) == (f.np * f.kw, f.kw, f.pipe) and f.rb == f.mb
        if f.wt == 0 and not pipe:
            ring = ring or 2
            if f.mb == 8 or nw == 2 or nw >= 9 or (kw == 2 and not (nw == 4 and f.mb == 4 and ring == 3)):
                ring = 2
            if f.mb <= 2 and ring == 3:
                ring = 4
            if f.mb == 1:
                ring = 2
            assert ring == f.ring, f.id
    assert gr.slice_ranges(7, 3) == [(0, 3), (3, 6), (6, 7)] and gr.empty_split(4, 3) and not gr.empty_split(5, 3)
