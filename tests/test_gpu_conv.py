"""The tokenizer kernels of bitdance_amd/csrc/bd_conv.hip, each alone against a float64 reference of the same operation
(tests/conv_ref.py), through the C entry points bd_conv, bd_conv_strided, bd_gn_stats, bd_gn_apply and bd_tokens_to_padded: the
launcher picks the tile width, the grid and the K-stage count exactly as for the decoder and the encoder, and the case names say which
(tests/test_conv_ref_cpu.py::test_case_lists_cover proves that the list reaches TW 32 / 16 / 8 with full and partial tiles, 1 .. 9
and 18 / 144 K stages, 1 / 7 / 8 / 9 / 12 pixel tiles x 1 / 2 / 3 channel tiles, every epilogue on partial tiles, stride 2 with odd
and one-pixel outputs, GroupNorm at C 32 .. 2048 and HW 1 .. 703 and above 65536, and every form of gn_apply).

Reference and bounds: the module docstring of tests/conv_ref.py.  In short, with u = the bf16 spacing at the reference value:
  convolution   |got - bf16(ref)| <= u + gamma(9 Cin) conv(|x|, |w|) and at most 1 % of a case's elements differ from bf16(ref) at
                all; fp32 outputs within one spacing of the rounded conv value + the fp32 term, at most 1 % beyond the fp32 term;
                the exact probes (integer inputs, one-hot weights) bit for bit: tap order, stride-2 origin, DCR order, the clamp of
                partial tiles, channel-tile padding, bias and residual indices without any tolerance;
  gn_stats      mean within gamma(256 C / 32) E|x|, rstd within 0.5 gamma (E[x^2] + 2 |mean| E|x|) / (var + eps) relative, both
                + 4 fp32 spacings; equal bits on a second call and after a call on other data in the same scratch;
  gn_apply      the statistics as above, then the output against the reference computed from the device's own statistics: the
                fp32 roundings of the chain and the one-ulp exp2 / rcp of the swish; the re-layout form bit-exact;
  tokens        bit-exact.
Every output is filled with a sentinel (NaN; 0x7FA5 for bf16) and sits between two guard bands of 256 elements: an element the
kernel skips fails, the border of a padded convolution output must still hold the sentinel (that of a GroupNorm output zero), the
guard bands their bits.  Every combination the host validation names is refused with BD_ERR_UNSUPPORTED and a sentinel output
left as it was.

Measured on an MI355X over the 172 cases (flip = share of elements that differ from the rounded reference, cap 1e-2; excess = worst
(|got - ref| - allowed) in bf16 spacings, from -1 (no element differs) up to 0):
  conv 2.2e-4 / -0.003 (78 cases; the 22 exact probes bit-identical)     gn_apply 7.8e-5 / -0.0 (42 cases; re-layouts bit-identical)
  gn_stats inside the derived bounds, equal bits call to call and after other data in the scratch (47 cases)     tokens bit-identical
No element anywhere is further than one spacing from the reference; no kernel fault was found.
The one-pass statistics where the mean is large against the spread (characterisation sets, held to the derived bound, which is loose
or vacuous there): relative rstd error against float64, beside torch's float32 native_group_norm on the same data
  mean 4, std 0.5, C 512, HW 1024:   device 3.55e-6   torch 1.1e-7   (derived bound 2.4e-2)
  mean 8, std 0.25, C 2048, HW 1000: device 7.06e-5   torch 1.2e-7   (derived bound 1.5)
Both stay below 2^-10 = 9.8e-4, a quarter of a bf16 spacing (the widest format any consumer of the statistics writes), so the kernel
keeps its one-pass sums.  Each case prints its figures (`pytest -s`, lines "CONVSTAT" and "CONVCHAR").
"""
from __future__ import annotations

import pytest
import torch

from tests import conv_ref as cr
from tests.conv_ref import BF16

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 256
UNSUPPORTED = -22


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


class _Out:
    """An output tensor of `shape` filled with the sentinel, between two guard bands; `zero_border`: a padded tensor whose
    one-pixel border is zero (what gn_apply's out_mode 0 writes into)."""

    def __init__(self, shape, dtype, zero_border=False):
        numel = 1
        for s in shape:
            numel *= s
        self.flat = cr.sentinel((numel + 2 * GUARD,), dtype, DEV)
        self.t = self.flat[GUARD:GUARD + numel].view(shape)
        if zero_border:
            n, Hp, Wp, C = shape
            self.t[cr.border_mask(n, Hp - 2, Wp - 2, C, DEV)] = 0
        self.before = self.flat.clone()

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self, what):
        a, b = cr.bits(self.flat), cr.bits(self.before)
        assert torch.equal(a[:GUARD], b[:GUARD]) and torch.equal(a[-GUARD:], b[-GUARD:]), f"{what}: written outside the output tensor"

    def unchanged(self):
        return torch.equal(cr.bits(self.flat), cr.bits(self.before))


def _finish(rep):
    print(rep.line())
    assert not rep.fail, "\n".join(rep.fail)


def _pack(c, d):
    K, npad = c.k * c.k * c.cin, (c.cout + 255) // 256 * 256
    m = torch.zeros(npad, K, dtype=BF16, device=DEV)
    m[:c.cout] = d.w.permute(0, 2, 3, 1).reshape(c.cout, K)                  # K ordered (ky, kx, ci)
    wp = torch.empty(npad * K, dtype=BF16, device=DEV)
    _check(_lib().bd_pack_weight(wp.data_ptr(), m.data_ptr(), npad, K, 0, npad, _stream()), "bd_pack_weight")
    return wp


def _conv_input(c, d):
    xh = d.x.permute(0, 2, 3, 1).contiguous()
    if c.k == 1:
        return xh
    xin = torch.zeros(c.n, xh.shape[1] + 2, xh.shape[2] + 2, c.cin, dtype=BF16, device=DEV)
    xin[:, 1:-1, 1:-1] = xh
    return xin


def _conv_out_shape(c):
    return {0: (c.n, c.H, c.W, c.cout), 1: (c.n, 2 * c.H, 2 * c.W, c.cout // 4), 2: (c.n, c.cout, c.H, c.W),
            3: (c.n, c.H + 2, c.W + 2, c.cout)}[c.mode]


def _run_conv(c):
    l = _lib()
    d = cr.to_device(c, DEV)
    wp, xin = _pack(c, d), _conv_input(c, d)
    out = _Out(_conv_out_shape(c), torch.float32 if c.out_f32 else BF16)
    res_f32 = int(c.res is not None and c.res.dtype == torch.float32)
    args = (xin.data_ptr(), wp.data_ptr(), _p(d.bias), _p(d.res), res_f32, out.ptr(), c.mode, c.out_f32, c.n, c.H, c.W, c.cin, c.cout, c.k * c.k)
    if c.stride == 1:
        _check(l.bd_conv(*args, _stream()), "bd_conv")
    else:
        _check(l.bd_conv_strided(*args, c.stride, _stream()), "bd_conv_strided")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", list(cr.CONV_CASES))
def test_conv(name):
    c = cr.CONV_CASES[name]()
    out = _run_conv(c)
    out.guards_intact(name)
    _finish(cr.judge_conv(c, dict(out=out.t.cpu()), f"conv/{name}"))


def _run_stats(c, x, partial=None):
    chunks = (c.HW + 255) // 256
    if partial is None:
        partial = cr.sentinel((c.n, chunks, 32, 2), torch.float32, DEV)
    stats = _Out((c.n, 32, 2), torch.float32)
    _check(_lib().bd_gn_stats(x.data_ptr(), c.f32, partial.data_ptr(), stats.ptr(), c.n, c.HW, c.C, c.eps, _stream()), "bd_gn_stats")
    torch.cuda.synchronize()
    stats.guards_intact("gn_stats")
    return stats.t, partial


@pytest.mark.parametrize("name", list(cr.STATS_CASES))
def test_gn_stats(name):
    c = cr.STATS_CASES[name]()
    x = c.x.to(DEV)
    stats, partial = _run_stats(c, x)
    _finish(cr.judge_gn_stats(c, dict(stats=stats.cpu()), f"gn_stats/{name}"))
    again, _ = _run_stats(c, x, partial)
    assert torch.equal(cr.bits(stats), cr.bits(again)), "the statistics differ between two calls"
    # the summation order is fixed: the same call after one on OTHER data in the same scratch gives the same bits
    other = (torch.randn(c.x.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)) * 3 - 2).to(c.x.dtype)
    _run_stats(c, other, partial)
    third, _ = _run_stats(c, x, partial)
    assert torch.equal(cr.bits(stats), cr.bits(third)), "the statistics depend on what the scratch held before"
    if c.char:
        dev_err, bound = cr.rstd_rel_error(c, stats.cpu())
        xn = x.float().view(c.n, c.HW, c.C).permute(0, 2, 1).contiguous()
        _, _, t_rstd = torch.native_group_norm(xn, None, None, c.n, c.C, c.HW, 32, c.eps)
        ts = torch.stack([t_rstd.view(c.n, 32), t_rstd.view(c.n, 32)], -1).cpu()
        torch_err, _ = cr.rstd_rel_error(c, ts)
        print(f"CONVCHAR {name} rstd relative error: device {dev_err:.3e}  torch float32 native_group_norm {torch_err:.3e}  "
              f"derived bound {bound:.3e}  quarter bf16 spacing {2.0 ** -10:.3e}")
        # the one-pass sums are kept BECAUSE the error stays below a quarter of a bf16 spacing (the widest format a consumer of the
        # statistics writes): past that, summing about a per-chunk shift or carrying the chunk sums in double is due
        assert dev_err < 2.0 ** -10, f"{name}: relative rstd error {dev_err:.3e} of the one-pass statistics"


@pytest.mark.parametrize("name", list(cr.APPLY_CASES))
def test_gn_apply(name):
    c = cr.APPLY_CASES[name]()
    d = cr.to_device(c, DEV)
    stats = _run_stats(c, d.x)[0] if c.stats else None
    shape = (c.n, c.H + 2, c.W + 2, c.C) if c.mode == 0 else (c.n, c.H, c.W, c.C)
    out = _Out(shape, torch.float32 if c.mode == 1 else BF16, zero_border=c.mode == 0)
    _check(_lib().bd_gn_apply(d.x.data_ptr(), c.f32, _p(stats), _p(d.gamma), _p(d.beta), _p(d.scale), _p(d.bias), out.ptr(), c.mode, c.swish,
                              c.n, c.H, c.W, c.C, _stream()), "bd_gn_apply")
    torch.cuda.synchronize()
    out.guards_intact(name)
    _finish(cr.judge_gn_apply(c, dict(stats=None if stats is None else stats.cpu(), out=out.t.cpu()), f"gn_apply/{name}"))


@pytest.mark.parametrize("name", list(cr.TOKEN_CASES))
def test_tokens_to_padded(name):
    c = cr.TOKEN_CASES[name]()
    z = c.z.to(DEV)
    out = _Out((c.n, c.H + 2, c.W + 2, c.C), BF16)
    _check(_lib().bd_tokens_to_padded(z.data_ptr(), out.ptr(), c.n, c.C, c.H, c.W, _stream()), "bd_tokens_to_padded")
    torch.cuda.synchronize()
    out.guards_intact(name)
    _finish(cr.judge_tokens(c, dict(out=out.t.cpu()), f"tokens/{name}"))


def test_unsupported_shapes_are_refused_before_any_launch():
    """Every combination the host validation names: BD_ERR_UNSUPPORTED, and the sentinel output keeps its bits."""
    l = _lib()
    st = _stream()
    x = torch.zeros(1 << 16, dtype=BF16, device=DEV)
    w = torch.zeros(1 << 18, dtype=BF16, device=DEV)
    f = torch.zeros(1 << 14, dtype=torch.float32, device=DEV)
    out = _Out((1 << 16,), torch.float32)

    def conv(n=1, H=8, W=8, cin=32, cout=64, taps=9, stride=1, mode=0):
        return l.bd_conv_strided(x.data_ptr(), w.data_ptr(), None, None, 0, out.ptr(), mode, int(mode == 2), n, H, W, cin, cout, taps, stride, st)

    def stats(n=1, HW=64, C=64):
        return l.bd_gn_stats(x.data_ptr(), 0, f.data_ptr(), out.ptr(), n, HW, C, 1e-6, st)

    def apply(n=1, H=4, W=4, C=64, mode=2):
        return l.bd_gn_apply(x.data_ptr(), 0, None, None, None, None, None, out.ptr(), mode, 0, n, H, W, C, st)

    def tokens(n=1, C=8, H=4, W=4):
        return l.bd_tokens_to_padded(f.data_ptr(), out.ptr(), n, C, H, W, st)

    refused = {
        "Cin % 32": lambda: conv(cin=48), "Cin 16": lambda: conv(cin=16), "Cin 0": lambda: conv(cin=0), "Cout 0": lambda: conv(cout=0),
        "Cout % 8, mode 0": lambda: conv(cout=60), "Cout % 8, mode 1": lambda: conv(cout=36, mode=1), "Cout % 8, mode 3": lambda: conv(cout=12, mode=3),
        "mode 1, Cout / 4 % 8": lambda: conv(cout=48, mode=1), "mode 1, Cout / 4 % 8 (16)": lambda: conv(cout=16, mode=1),
        "taps 3": lambda: conv(taps=3), "taps 4": lambda: conv(taps=4), "taps 25": lambda: conv(taps=25), "taps 0": lambda: conv(taps=0),
        "stride 2, taps 1": lambda: conv(taps=1, stride=2), "stride 3": lambda: conv(stride=3), "stride 0": lambda: conv(stride=0),
        "out_mode -1": lambda: conv(mode=-1), "out_mode 4": lambda: conv(mode=4),
        "conv n 0": lambda: conv(n=0), "conv n -1": lambda: conv(n=-1), "conv H 0": lambda: conv(H=0), "conv W 0": lambda: conv(W=0),
        "bd_conv n 0": lambda: l.bd_conv(x.data_ptr(), w.data_ptr(), None, None, 0, out.ptr(), 0, 0, 0, 8, 8, 32, 64, 9, st),
        "stats C 96": lambda: stats(C=96), "stats C 48": lambda: stats(C=48), "stats C 16": lambda: stats(C=16), "stats C 0": lambda: stats(C=0),
        "stats C 4096": lambda: stats(C=4096), "stats C 2080": lambda: stats(C=2080), "stats n 0": lambda: stats(n=0), "stats HW 0": lambda: stats(HW=0),
        "stats HW -1": lambda: stats(HW=-1),
        "apply C 96": lambda: apply(C=96), "apply C 48": lambda: apply(C=48), "apply C 0": lambda: apply(C=0), "apply C 3072": lambda: apply(C=3072),
        "apply out_mode 3": lambda: apply(mode=3), "apply out_mode -1": lambda: apply(mode=-1), "apply n 0": lambda: apply(n=0),
        "apply H 0": lambda: apply(H=0), "apply W 0": lambda: apply(W=0), "apply W -2": lambda: apply(W=-2),
        "tokens n 0": lambda: tokens(n=0), "tokens C 0": lambda: tokens(C=0), "tokens H 0": lambda: tokens(H=0), "tokens W -1": lambda: tokens(W=-1),
    }
    for what, call in refused.items():
        rc = call()
        assert rc == UNSUPPORTED, f"{what}: returned {rc}, expected BD_ERR_UNSUPPORTED"
        assert l.bd_last_error(), what
    torch.cuda.synchronize()
    assert out.unchanged(), "a refused call wrote to its output"
    # and the neighbours of each refusal are accepted (the validation refuses no more than it names)
    assert conv(cout=3, mode=2) == 0 and conv(cout=32, mode=1) == 0 and conv(taps=1) == 0 and conv(stride=2) == 0
    assert stats(C=2048, HW=1) == 0 and apply(C=2048, H=1, W=1, mode=0) == 0 and tokens() == 0
    torch.cuda.synchronize()
