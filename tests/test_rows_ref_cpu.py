"""The references and bounds of tests/test_gpu_rows.py, checked without a GPU (tests/rows_ref.py holds both).

For every launcher and every input set of the GPU module:

* precision: the float32 run of the reference, judged against the float64 run exactly as the device is, stays inside bound (a)
  and flips at most a quarter of the 1 % cap of bound (b) -- the cap is a condition with headroom, not a measurement;
* faults: every fault of the launcher's list that changes what the case computes, run through the float64 reference, breaks
  (a) or (b) (or an equality the judge asserts).  test_every_fault_is_exercised proves no fault of a list is vacuous.

The head attention is judged by the per-element bound and the relative-rms bound of test_gpu_attn.py instead of (a) / (b).
"""
from __future__ import annotations

import pytest
import torch

from tests import rows_ref as rr

ALL = [(l, n) for l, (cases, _, _, _) in rr.LAUNCHERS.items() for n in cases]


@pytest.mark.parametrize("launcher,name", ALL, ids=[f"{l}-{n}" for l, n in ALL])
def test_float32_run_and_faults(launcher, name):
    cases, impl, judge, faults = rr.LAUNCHERS[launcher]
    c = cases[name]()
    rep = judge(c, impl(c, torch.float32), f"{launcher}/{name} float32")
    assert not rep.fail, "\n".join(rep.fail)
    if launcher != "head_attn":
        assert rep.flip <= rr.FLIP_CAP / 4, rep.line()
    same = judge(c, impl(c, torch.float64), f"{launcher}/{name} float64")
    assert not same.fail and (launcher == "head_attn" or same.flip <= 1e-4), "\n".join(same.fail) + same.line()
    for f in faults:
        if rr.applies(launcher, c, f):
            bad = judge(c, impl(c, torch.float64, f), f"{launcher}/{name} {f}")
            assert bad.fail, f"{launcher}/{name}: the bounds do not reject the fault {f} ({bad.line()})"


@pytest.mark.parametrize("launcher", list(rr.LAUNCHERS))
def test_every_fault_is_exercised(launcher):
    cases, _, _, faults = rr.LAUNCHERS[launcher]
    built = [c() for c in cases.values()]
    for f in faults:
        assert any(rr.applies(launcher, c, f) for c in built), f"{launcher}: no input set exercises the fault {f}"


def test_ulp_and_unfragmenting():
    v = torch.tensor([1.0, 1.5, 2.0, 0.75, -3.0, 2.0 ** -20])
    assert rr.ulp_bf16(v).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -6, 2.0 ** -27]
    nxt = (v.to(rr.BF16).view(torch.int16) + 1).view(rr.BF16).double()
    assert torch.equal((nxt - v.double()).abs(), rr.ulp_bf16(v))
    rb, K = 2, 128
    rows = torch.arange(rb * 32)[:, None].expand(rb * 32, K)
    ks = torch.arange(K)[None, :].expand(rb * 32, K)
    off = (((ks // 16) * rb + rows // 32) * 64 + rows % 32 + 32 * (ks // 8 % 2)) * 8 + ks % 8       # afrag_off (bd_common.h)
    buf = torch.zeros(rb * 32 * K, dtype=torch.int64)
    buf[off.flatten()] = (rows * 1000 + ks).flatten()
    assert torch.equal(rr.unfrag(buf, rb, K), rows * 1000 + ks)
    off8 = ((((ks // 64) * rb + rows // 32) * 2 + (ks // 16 % 2)) * 64 + rows % 32 + 32 * (ks // 32 % 2)) * 16 + ks % 16   # a8_off
    buf8 = torch.zeros(rb * 32 * K, dtype=torch.int64)
    buf8[off8.flatten()] = (rows * 1000 + ks).flatten()
    assert torch.equal(rr.unfrag8(buf8, rb, K), rows * 1000 + ks)
