"""The MXFP4 weight quantiser of ``weights="fp4a"`` (engine.quantize_rows_mxfp4) on the CPU, against an independent restatement:
the block exponent through ``math.frexp`` and the e2m1 code through a search of the value table (nearest; on a tie the code with the
even mantissa bit), where the engine reads the fp32 exponent field and rounds with ``torch.round``.

Format (OCP Microscaling v1.0, MXFP4): blocks of 32 consecutive k of one output channel share one E8M0 exponent byte (value
2^(byte - 127)); elements are e2m1: 0, 0.5, 1, 1.5, 2, 3, 4, 6 and their negatives (bit 3 of the code = sign).
e = floor(log2(amax)) - 2, clamped to [-127, 127]; an all-zero block gets -127; values beyond 6 x 2^e saturate."""
import math

import pytest
import torch

GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def ref_block(vals):
    """(codes, biased exponent) of one block of 32 Python floats."""
    amax = max(abs(v) for v in vals)
    if amax == 0.0:
        e = -127
    else:
        m, ex = math.frexp(amax)                 # amax = m * 2^ex, 0.5 <= m < 1  ->  floor(log2(amax)) = ex - 1
        e = min(127, max(-127, ex - 1 - 2))
    codes = []
    for v in vals:
        a = math.ldexp(abs(v), -e)               # exact: a power-of-two scaling of a bf16 value in fp64
        best, bd = 0, None
        for c, gv in enumerate(GRID):
            d = abs(a - gv)
            if bd is None or d < bd or (d == bd and c % 2 == 0):
                best, bd = c, d
        if a > 6.0:
            best = 7
        codes.append(best | (8 if math.copysign(1.0, v) < 0 else 0))
    return codes, e + 127


def ref_quant(w):
    N, K = w.shape
    codes = torch.zeros(N, K, dtype=torch.uint8)
    exps = torch.zeros(N, K // 32, dtype=torch.uint8)
    wl = w.double().tolist()
    for n in range(N):
        for b in range(K // 32):
            c, e = ref_block(wl[n][32 * b:32 * b + 32])
            codes[n, 32 * b:32 * b + 32] = torch.tensor(c, dtype=torch.uint8)
            exps[n, b] = e
    return codes, exps


def check(w):
    from bitdance_amd import engine as E
    w = w.to(torch.bfloat16).float()
    c, e = E.quantize_rows_mxfp4(w)
    cr, er = ref_quant(w)
    assert c.dtype == torch.uint8 and e.dtype == torch.uint8 and c.shape == w.shape and e.shape == (w.shape[0], w.shape[1] // 32)
    assert torch.equal(e, er), (e, er)
    assert torch.equal(c, cr), (c != cr).nonzero()[:8]
    return c, e


def test_quantiser_random_weights():
    g = torch.Generator().manual_seed(5)
    w = torch.randn(24, 256, generator=g) / 16 * (1 + 3 * torch.rand(24, 1, generator=g))
    w[3, 64:96] = 0                                           # an all-zero block
    w[5, :32] = 0
    w[5, 7] = -0.0
    c, e = check(w)
    assert e[3, 2] == 0 and (c[3, 64:96] == 0).all()          # smallest exponent, +0 codes
    assert int((c & 7).max()) >= 6                            # every block reaches the top binade: code 6 (4) or 7 (6)
    assert ((c.view(24, 8, 32) & 7).amax(dim=2)[e > 0] >= 6).all()


def test_quantiser_power_of_two_amax_and_ties():
    # amax = 2^k exactly: floor(log2) = k, e = k - 2, the largest element scales to 4.0 (code 6)
    for k in (-9, 0, 3):
        w = torch.zeros(1, 32)
        w[0, 0] = 2.0 ** k
        w[0, 1] = -(2.0 ** k) * 0.75                          # scaled 3.0
        c, e = check(w)
        assert int(e[0, 0]) == k - 2 + 127 and int(c[0, 0]) == 6 and int(c[0, 1]) == (5 | 8)
    # rounding ties, round to nearest EVEN code: the block holds 4.0 (so e = 0 and scaled == raw) and the tie values
    w = torch.zeros(1, 32)
    ties = {0.25: 0.0, 0.75: 1.0, 1.25: 1.0, 1.75: 2.0, 2.5: 2.0, 3.5: 4.0, 5.0: 4.0}
    w[0, 0] = 4.0
    for i, t in enumerate(ties):
        w[0, 1 + i] = t
        w[0, 11 + i] = -t
    c, e = check(w)
    assert int(e[0, 0]) == 127
    for i, (t, want) in enumerate(ties.items()):
        assert GRID[int(c[0, 1 + i]) & 7] == want, (t, want, int(c[0, 1 + i]))
        assert GRID[int(c[0, 11 + i]) & 7] == want and int(c[0, 11 + i]) & 8
    # 7 x 2^e (amax in [4, 8) x 2^e) lies above the largest e2m1 value: saturates to 6; so does 5 -> 4 stay a tie below it
    w = torch.zeros(1, 32)
    w[0, 0], w[0, 1], w[0, 2] = 7.0, -7.5, 5.0
    c, e = check(w)
    assert int(e[0, 0]) == 127 and int(c[0, 0]) == 7 and int(c[0, 1]) == 15 and int(c[0, 2]) == 6


def test_quantiser_tiny_and_huge_blocks_clamp_the_exponent():
    w = torch.zeros(4, 32)
    w[0, 0] = 2.0 ** -133                                     # the smallest bf16 subnormal: e would be -135 -> clamped to -127, rounds to 0
    w[1, 0], w[1, 1] = 2.0 ** -126, 2.0 ** -127               # e = -128 -> -127: scaled 2.0 and 1.0
    w[2, 0], w[2, 1] = 3.0 * 2.0 ** 126, -(2.0 ** 120)        # near the top of bf16: e = 125
    w[3, 0] = 2.0 ** -125                                     # e = -127 exactly, scaled 4.0
    c, e = check(w)
    assert e[:, 0].tolist() == [0, 0, 252, 0]
    assert int(c[0, 0]) == 0 and int(c[1, 0]) == 4 and int(c[1, 1]) == 2 and int(c[2, 0]) == 7 and int(c[3, 0]) == 6


def test_every_code_exponent_pair_round_trips():
    """Every (code, exponent) pair a bf16 weight can produce dequantises and re-quantises to itself.  A block that holds all sixteen
    codes has amax = 6 x 2^e, so its exponent is e again; 0.5 x 2^e .. 6 x 2^e are bf16 values for e in [-127, 125] (126 and 127 would
    need an amax beyond the largest bf16)."""
    from bitdance_amd import engine as E
    exps = torch.arange(0, 253, dtype=torch.uint8)            # biased: e = -127 .. 125
    codes = torch.arange(16, dtype=torch.uint8).repeat(2)[None, :].expand(len(exps), 32).contiguous()
    w = E.dequantize_mxfp4(codes, exps[:, None])
    assert torch.equal(w, w.to(torch.bfloat16).double())      # representable
    c2, e2 = E.quantize_rows_mxfp4(w.float())
    assert torch.equal(e2[:, 0], exps) and torch.equal(c2, codes)
    cr, er = ref_quant(w.float())
    assert torch.equal(cr, codes) and torch.equal(er[:, 0], exps)
    # the table itself
    v = E.dequantize_mxfp4(torch.arange(16, dtype=torch.uint8).repeat(2)[None, :], torch.tensor([[127]], dtype=torch.uint8))[0, :16]
    assert v.tolist() == list(GRID) + [-x for x in GRID]


def test_nibble_packing_and_sizes():
    from bitdance_amd import engine as E
    codes = (torch.arange(64, dtype=torch.uint8) % 16)[None, :]
    nib = E.mxfp4_nibbles(codes)
    assert nib.shape == (1, 32) and int(nib[0, 0]) == 0x10 and int(nib[0, 3]) == 0x76      # k even in the low nibble
    assert E.mxfp4_exp_bytes(32, 64) == 256 and E.mxfp4_exp_bytes(64, 5120) == 2 * 20 * 256 and E.mxfp4_exp_bytes(32, 320) == 2 * 256
    with pytest.raises(E.BitDanceHipError):
        E.quantize_rows_mxfp4(torch.zeros(2, 48))


def test_mode_flag():
    from bitdance_amd import engine as E
    assert E._fp8_flag("fp4a") == 3
    assert [E._fp8_flag(m) for m in ("bf16", "fp8", "fp8a")] == [0, 1, 2]
    for bad in ("fp4", "mxfp4", "FP4A", ""):
        with pytest.raises(E.BitDanceHipError):
            E._fp8_flag(bad)
