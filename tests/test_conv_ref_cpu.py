"""The references and bounds of tests/test_gpu_conv.py, checked without a GPU (tests/conv_ref.py holds both).

For every kernel family (conv, gn_stats, gn_apply, tokens) and every input set of the GPU module:

* precision: the float32 run of the reference, judged against the float64 run exactly as the device is, stays inside the bounds
  and flips at most a quarter of the 1 % cap -- the cap is a condition with headroom, not a measurement;
* the float64 run flips at most 1e-4 of the elements;
* faults: every fault of the family's list that changes what the case computes, run through the float64 reference, breaks a bound
  or an equality.  test_every_fault_is_exercised proves that no fault of a list is vacuous, test_probes_reject_every_mapping_fault
  that the exact probes alone reject every index fault of the convolution, and test_case_lists_cover that the input sets reach
  every tile width, K-stage count, tile-count / channel-tile combination and GroupNorm shape the kernels branch on.
"""
from __future__ import annotations

import pytest
import torch

from tests import conv_ref as cr

ALL = [(l, n) for l, (cases, *_) in cr.LAUNCHERS.items() for n in cases]


@pytest.mark.parametrize("launcher,name", ALL, ids=[f"{l}-{n}" for l, n in ALL])
def test_float32_run_and_faults(launcher, name):
    cases, impl, judge, faults, applies = cr.LAUNCHERS[launcher]
    c = cases[name]()
    rep = judge(c, impl(c, torch.float32), f"{launcher}/{name} float32")
    assert not rep.fail, "\n".join(rep.fail)
    assert rep.flip <= cr.FLIP_CAP / 4, rep.line()
    same = judge(c, impl(c, torch.float64), f"{launcher}/{name} float64")
    assert not same.fail and same.flip <= 1e-4, "\n".join(same.fail) + same.line()
    for f in faults:
        if applies(c, f):
            bad = judge(c, impl(c, torch.float64, f), f"{launcher}/{name} {f}")
            assert bad.fail, f"{launcher}/{name}: the bounds do not reject the fault {f} ({bad.line()})"


@pytest.mark.parametrize("launcher", list(cr.LAUNCHERS))
def test_every_fault_is_exercised(launcher):
    cases, _, _, faults, applies = cr.LAUNCHERS[launcher]
    left = set(faults)
    for name, make in cases.items():
        if launcher == "conv" and cr.CONV_SPECS[name].get("probe"):
            continue                                            # (the probes have a test of their own below)
        c = make()
        left -= {f for f in left if applies(c, f)}
        if not left:
            break
    assert not left, f"{launcher}: no input set exercises the faults {sorted(left)}"


def test_probes_reject_every_mapping_fault():
    left = set(cr.MAPPING_FAULTS)
    for name, kw in cr.CONV_SPECS.items():
        if not kw.get("probe"):
            continue
        c = cr.CONV_CASES[name]()
        for f in sorted(left):
            if cr.conv_fault_applies(c, f) and cr.judge_conv(c, cr.impl_conv(c, torch.float64, f), f"{name} {f}").fail:
                left.discard(f)
    assert not left, f"no exact probe rejects the faults {sorted(left)}"


def test_tile_width_rule():
    """The launcher's rule (least padded area, the first of 32, 16, 8 wins ties), at shapes that pick each width."""
    assert cr.tile_width(8, 8) == 32 and cr.tile_width(32, 8) == 8 and cr.tile_width(40, 5) == 8
    assert cr.tile_width(16, 16) == 16 and cr.tile_width(32, 32) == 32 and cr.tile_width(48, 48) == 16
    g = cr.geometry(dict(n=3, H=32, W=32, cin=32, cout=520, k=3))
    assert (g.TW, g.MT, g.NT, g.nst, g.last) == (32, 12, 3, 9, 8)


def test_case_lists_cover():
    cov = cr.coverage()
    for tw in (32, 16, 8):
        for px in (False, True):
            for py in (False, True):
                assert (tw, px, py) in cov.tiles, f"no convolution case with TW {tw}, partial x {px}, partial y {py}"
    assert set(range(1, 10)) <= cov.nst_1x1, cov.nst_1x1               # 1x1, Cin 32 .. 288: every short path of the DMA ring
    assert {9, 18, 144} <= cov.nst_3x3
    for mt in (1, 7, 8, 9, 12):
        for nt in (1, 2, 3):
            assert (mt, nt) in cov.mt_nt, f"no case with {mt} pixel tiles and {nt} channel tiles"
    assert {(7, 2), (9, 3), (12, 2), (12, 3)} <= cov.short_group_multi_nt
    assert {8, 64, 248} <= cov.last
    assert {3, 4, 12} <= cov.image_cout and {32, 1024} <= cov.d2s_cout
    assert cov.res == {None, "bf16", "f32"}
    assert cov.partial_modes == {0, 1, 2, 3}
    assert any(h % 2 and w % 2 for h, w in cov.s2) and any(h == 1 for h, _ in cov.s2) and any(w == 1 for _, w in cov.s2)
    assert (True, True) in cov.s2_partial
    assert {1, 2, 3} <= cov.n
    assert cov.probe_taps == set(range(9)) and cov.probe_pow2 == {1, 2}
    assert {(m, 1) for m in range(4)} <= cov.probe_modes and {(m, 2) for m in range(4)} <= cov.probe_modes
    for C in (32, 64, 128, 256, 512, 1024, 2048):
        for HW in (1, 64, 255, 256, 257, 703):
            assert (C, HW) in cov.gn_c_hw
    assert cov.gn_chunks > 256 and cov.gn_dtypes == {0, 1} and cov.gn_varied_n2
    for stats in (0, 1):
        for affine, ada in ((True, False), (False, True), (False, False)):
            for swish in (0, 1):
                for mode in (0, 1, 2):
                    assert (stats, affine, ada, swish, mode) in cov.apply_forms
    assert cov.apply_w == {1, 5, 64, 100} and 2048 in cov.apply_c and 32 in cov.apply_c
    assert cov.token_grid_stride


def test_sentinel_and_probe_values_are_exact():
    s = cr.sentinel((4,), cr.BF16)
    assert torch.isnan(s.float()).all() and (cr.bits(s) == cr.SENT16).all()
    c = cr.CONV_CASES["probe_tap4"]()
    assert torch.equal(c.x.double(), c.x.double().round()) and c.x.min() >= 1 and c.x.max() <= cr.PRIME
    assert (c.w.double().sum((1, 2, 3)) == 1).all()


@pytest.mark.parametrize("name", [n for n, kw in cr.STATS_SPECS.items() if kw.get("char")])
def test_one_pass_statistics_in_the_kernels_order(name):
    """The characterisation sets (mean large against the spread) through a CPU restatement of the kernel's fp32 summation order:
    inside the derived bound, and the relative rstd error below 2^-10, a quarter of a bf16 spacing -- what the GPU module asserts of
    the device (measured there: the same 3.55e-6 and 7.06e-5 as here)."""
    c = cr.STATS_CASES[name]()
    st = cr.emulate_gn_stats(c)
    rep = cr.judge_gn_stats(c, dict(stats=st), f"gn_stats/{name} emulated")
    assert not rep.fail, "\n".join(rep.fail)
    err, bound = cr.rstd_rel_error(c, st)
    print(f"CONVCHAR {name} emulated rstd relative error {err:.3e} (derived bound {bound:.3e})")
    assert err < 2.0 ** -10, err
