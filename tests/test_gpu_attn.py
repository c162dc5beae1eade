"""The two decode attentions of bitdance_amd/csrc/bd_attn.hip, each against a float64 reference of the same operation.

* bd_llm_attn: the Qwen3 flash-decode (llm_attn_kernel + llm_attn_combine_kernel) over the static KV cache.
* bd_in_attn: the ImageNet transformer's attention (in_attn_small_kernel<1|4>, in_attn_mfma_kernel, in_attn_kernel).

The reference is plain torch in float64 on the same bf16 inputs the kernel reads.  For the ImageNet kernels it applies the two
roundings the reference model specifies (in_attn_kernel's comment): bf16 scores and bf16 P = e / sum.  Nothing else.

Rounding points and the bounds derived from them (U = 2^-8, the unit roundoff of bf16's 8 significant bits):

* Qwen3.  The scores are fp32.  The un-normalised P is rounded to bf16 before P.V, which is a relative error <= U on every
  weight.  The accumulation is fp32, at most L * 2^-24 relative to A = sum_j w_j |v_j|.  The output is rounded once to bf16,
  <= U |o|.  Per element:  |got - ref| <= 1.01 U (A + |ref|) + L 2^-24 A + 1e-6.
  On random data the rounding errors are independent and each has rms <= U / sqrt(3) relative, so the two roundings together
  give a relative rms <= sqrt(2/3) U = 0.32 %.  The bound is twice that: 0.65 %.
* ImageNet.  The reference rounds the scores and P itself.  The kernel's fp32 e / sum differs from the fp64 one by ~1e-7, so a
  bf16 P can land one ulp (2U) away, and the scores of these tests are exact in fp32 (see below).  Then the output rounding
  adds <= U |o|.  Per element:  |got - ref| <= 2U A + 1.01 U |ref| + L 2^-24 A + 1e-6.  Random data: the output rounding alone is
  <= U / sqrt(3) rms, and P flips are rare (~1e-5 of the weights), so the relative rms bound is 2 U / sqrt(3) = 0.45 %.

test_tolerances_see_the_faults proves, in the reference domain alone, that these bounds catch a dropped last visible key, an
added first invisible key, a dropped 64-key tile and a wrong split weight.
"""
from __future__ import annotations

import ctypes
import math

import pytest
import torch

from tests.rows_ref import unfrag

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
U = 2.0 ** -8
QW_SCALE = 128 ** -0.5
RMS_QW = 2 * math.sqrt(2 / 3) * U
RMS_IN = 2 * math.sqrt(1 / 3) * U
FAULTS = ("drop_last", "add_invisible", "drop_tile", "split_weight")


def _lib():
    from bitdance_amd._lib import lib
    return lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels through the C ABI
def run_llm(q, K, VT, kv, P, nh, nkv, splits, causal):
    """q [nseq * P, nh, 128], K [nseq, nkv, Lmax, 128], VT [nseq, nkv, 128, Lmax] bf16 -> [nseq * P, nh, 128] fp32."""
    from bitdance_amd._lib import check
    nseq, Lmax, G = K.shape[0], K.shape[2], nh // nkv
    rb = (nseq * P + 31) // 32
    state = torch.zeros(65, dtype=torch.int32, device=DEV)
    # NaN scratch: a partial row the combine reads but the split kernel never wrote shows up in the output
    o_part = torch.full((nseq * nkv * splits * G * P * 128,), float("nan"), device=DEV)
    ml_part = torch.full((nseq * nkv * splits * G * P * 2,), float("nan"), device=DEV)
    o = torch.full((rb * 32 * nh * 128,), float("nan"), dtype=BF16, device=DEV)
    arr = (ctypes.c_int * nseq)(*kv)
    check(_lib().bd_llm_attn(q.data_ptr(), K.data_ptr(), VT.data_ptr(), arr, nseq, P, nh, nkv, Lmax, splits, int(causal),
                             state.data_ptr(), o_part.data_ptr(), ml_part.data_ptr(), o.data_ptr(), rb, _stream()), "bd_llm_attn")
    torch.cuda.synchronize()
    assert state[1:1 + nseq].tolist() == list(kv)
    return unfrag(o, rb, nh * 128)[: nseq * P].view(nseq * P, nh, 128).float()


def run_in(q, K, V, kv, P, causal):
    """q [nseq * P, nh * 64] (scaled), K / V [nseq, nh, Lmax, 64] bf16 -> [nseq * P, nh, 64] fp32."""
    from bitdance_amd._lib import check
    nseq, nh, Lmax = K.shape[0], K.shape[1], K.shape[2]
    rb = (nseq * P + 31) // 32
    state = torch.zeros(65, dtype=torch.int32, device=DEV)
    o = torch.full((rb * 32 * nh * 64,), float("nan"), dtype=BF16, device=DEV)
    check(_lib().bd_in_attn(q.data_ptr(), K.data_ptr(), V.data_ptr(), kv, nseq, P, nh, Lmax, int(causal), state.data_ptr(),
                            o.data_ptr(), rb, _stream()), "bd_in_attn")
    torch.cuda.synchronize()
    return unfrag(o, rb, nh * 64)[: nseq * P].view(nseq * P, nh, 64).float()


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 reference, with the faults of the tolerance self-check
def _attn64(qh, kh, vh, vis, scale, boost=None, bf16_rounding=False):
    """qh [H, P, d], kh [H, Lmax, d], vh [H, Lmax, dv] float64; vis [P, Lmax] bool; boost [P, Lmax] added to the scaled scores.
    Returns (out, A) [H, P, dv]: the attention output and sum_j w_j |v_j|."""
    s = torch.matmul(qh, kh.transpose(1, 2)) * scale
    if bf16_rounding:
        s = s.to(BF16).double()
    s = s.masked_fill(~vis, float("-inf"))
    if boost is not None:
        s = s + boost
    m = s.amax(-1, keepdim=True).clamp_min(-1e300)              # a row without visible keys: all weights 0
    e = torch.exp(s - m)
    w = e / e.sum(-1, keepdim=True).clamp_min(1e-300)
    if bf16_rounding:
        w = w.to(BF16).double()
    return w @ vh, w @ vh.abs()


def _visibility(kv, P, Lmax, causal, fault=None, splits=1):
    """[P, Lmax] bool (query i sees key j) and the logit boost, with one fault applied."""
    L = kv + P
    i = torch.arange(P, device=DEV)[:, None]
    j = torch.arange(Lmax, device=DEV)[None, :]
    last = (kv + i) if causal else torch.full_like(i, L - 1)    # last visible key of row i
    vis = j <= last
    boost = torch.zeros(P, Lmax, dtype=torch.float64, device=DEV)
    ntiles = (L + 63) // 64
    tile = (ntiles - 1) // 2
    if fault == "drop_last":
        vis &= j != last
    elif fault == "add_invisible":
        vis |= (j == last + 1)
    elif fault == "drop_tile":
        vis &= (j // 64) != tile
    elif fault == "split_weight":                               # the split that holds `tile` merged with twice its weight
        per = -(-ntiles // splits)
        boost[:, (tile // per) * per * 64: ((tile // per) + 1) * per * 64] = math.log(2.0)
    return vis, boost


def ref_llm(q, K, VT, kv, P, nh, nkv, causal, splits=1, fault=None):
    nseq, Lmax, G = K.shape[0], K.shape[2], nh // nkv
    outs, accs = [], []
    for s in range(nseq):
        qh = q[s * P:(s + 1) * P].double().permute(1, 0, 2)
        kh = K[s].double().repeat_interleave(G, 0)
        vh = VT[s].double().transpose(1, 2).repeat_interleave(G, 0)
        vis, boost = _visibility(kv[s], P, Lmax, causal, fault, splits)
        o, a = _attn64(qh, kh, vh, vis, QW_SCALE, boost)
        outs.append(o.permute(1, 0, 2))
        accs.append(a.permute(1, 0, 2))
    return torch.cat(outs), torch.cat(accs)


def ref_in(q, K, V, kv, P, causal, fault=None):
    nseq, nh, Lmax = K.shape[0], K.shape[1], K.shape[2]
    vis, boost = _visibility(kv, P, Lmax, causal, fault)
    outs, accs = [], []
    for s in range(nseq):
        qh = q[s * P:(s + 1) * P].double().view(P, nh, 64).permute(1, 0, 2)
        o, a = _attn64(qh, K[s].double(), V[s].double(), vis, 1.0, boost, bf16_rounding=True)
        outs.append(o.permute(1, 0, 2))
        accs.append(a.permute(1, 0, 2))
    return torch.cat(outs), torch.cat(accs)


def tol_llm(ref, A, L):
    return 1.01 * U * (A + ref.abs()) + L * 2.0 ** -24 * A + 1e-6


def tol_in(ref, A, L):
    return 2 * U * A + 1.01 * U * ref.abs() + L * 2.0 ** -24 * A + 1e-6


def rel_rms(got, ref):
    return ((got.double() - ref).norm() / ref.norm()).item()


def assert_within(got, ref, tol, what):
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    excess = (got.double() - ref).abs() - tol
    worst = excess.argmax()
    assert excess.max() <= 0, (f"{what}: {int((excess > 0).sum())} elements out of bounds; worst at flat index {int(worst)}: "
                               f"got {got.flatten()[worst].item():.6g} ref {ref.flatten()[worst].item():.6g} "
                               f"tol {tol.flatten()[worst].item():.3g}")


# ---------------------------------------------------------------------------------------------------------------------------------
# probes: every score an exact integer, a graded set of selected keys with one-hot V channels, a sentinel past the visible keys
QD_G, QD_A = 93, 7              # the channels q reads (different k-steps of 16 channels)
IND_G, IND_A = 45, 22            # (head_dim 64)
LEAK_QW, LEAK_IN = 100, 50       # V channel of the sentinel keys
SENTINEL_V = 1000.0


def probe_keys(kv, P, causal, tile):
    """Selected keys of one sequence: key 0, both sides of every `tile`-key boundary (the split boundaries are 64-key tile
    boundaries), the last visible key of each row (kv + i causal, L - 1 otherwise) and, causal, the first invisible key of each
    row but the last (kv + i + 1).  The first invisible key of the last row (L) is the first sentinel."""
    L = kv + P
    sel = {0, L - 1}
    for t in range(1, (L + tile - 1) // tile):
        sel |= {tile * t - 1, tile * t}
    if causal:
        sel |= set(range(kv, L))
    return sorted(j for j in sel if j < L)


def _channels(n, width, leak):
    ch = torch.tensor([c for c in range(width) if c != leak])
    return ch[torch.arange(n) % (width - 1)]


def llm_probe(nseq, nh, nkv, P, Lmax, kv, causal, seed):
    """Scores 8 * (k_G + a * b) with q = 8 e_G + 8 a e_A: selected keys k_G = 16 - (tile % 3) (0.707-nat steps that move the running
    max up and down from tile to tile and split to split), a, b in {-1, 0, 1}; the rest k_G = -24 (>= 25 nats below); the
    sentinel past kv + P k_G = 64 (45 nats above) with V = 1000 in the leak channel."""
    g = torch.Generator().manual_seed(seed)
    K = torch.randn(nseq, nkv, Lmax, 128, generator=g)           # noise in every channel q does not read
    VT = torch.zeros(nseq, nkv, 128, Lmax)
    for s in range(nseq):
        L = kv[s] + P
        sel = torch.tensor(probe_keys(kv[s], P, causal, 64))
        kg = torch.full((nkv, Lmax), -24.0)
        kg[:, sel] = 16.0 - (sel // 64 % 3).float()
        kg[:, L:] = 64.0
        pb = torch.randint(-1, 2, (nkv, Lmax), generator=g).float()
        pb[:, L:] = 0.0
        K[s, :, :, QD_G], K[s, :, :, QD_A] = kg, pb
        VT[s, :, _channels(len(sel), 128, LEAK_QW), sel] = 1.0
        VT[s, :, LEAK_QW, L:] = SENTINEL_V
    q = torch.zeros(nseq * P, nh, 128)
    q[..., QD_G] = 8.0
    q[..., QD_A] = 8.0 * torch.randint(-1, 2, (nseq * P, nh), generator=g).float()
    return q.to(BF16).to(DEV), K.to(BF16).to(DEV), VT.to(BF16).to(DEV)


def in_probe(nseq, nh, P, Lmax, kv, causal, seed):
    """The same for head_dim 64 and a pre-scaled q: scores 0.5 * (k_G + a * b) nats with q = 0.5 e_G + 0.5 a e_A; selected
    k_G = 32 - (key // 32 % 3), the rest -20, the sentinel 128.  Scores are multiples of 0.5 below 64: exact in bf16."""
    g = torch.Generator().manual_seed(seed)
    K = torch.randn(nseq, nh, Lmax, 64, generator=g)
    V = torch.zeros(nseq, nh, Lmax, 64)
    L = kv + P
    sel = torch.tensor(probe_keys(kv, P, causal, 32))
    kg = torch.full((Lmax,), -20.0)
    kg[sel] = 32.0 - (sel // 32 % 3).float()
    kg[L:] = 128.0
    pb = torch.randint(-1, 2, (nseq, nh, Lmax), generator=g).float()
    pb[..., L:] = 0.0
    K[..., IND_G], K[..., IND_A] = kg, pb
    V[:, :, sel, _channels(len(sel), 64, LEAK_IN)] = 1.0
    V[:, :, L:, LEAK_IN] = SENTINEL_V
    q = torch.zeros(nseq * P, nh, 64)
    q[..., IND_G] = 0.5
    q[..., IND_A] = 0.5 * torch.randint(-1, 2, (nseq * P, nh), generator=g).float()
    return q.view(nseq * P, nh * 64).to(BF16).to(DEV), K.to(BF16).to(DEV), V.to(BF16).to(DEV)


# (nh, nkv, P, splits, causal, Lmax, kv): G = nh / nkv; 640-thread workgroups (G 5, P 64) and 512 (G 4, P 64) take the pipelined
# K / V loader, the rest the plain one
LLM_PROBES = [
    pytest.param(40, 8, 64, 12, 0, 4416, [4352, 4290], id="g5_nh40_p64_s12_full_cache"),        # the 1024 px headline shape
    pytest.param(40, 8, 64, 12, 1, 4416, [4000, 65], id="g5_nh40_p64_s12_causal"),
    pytest.param(20, 4, 64, 16, 1, 2048, [0, 63, 64, 65], id="g5_nh20_p64_s16_causal_short"),   # ntiles < splits: empty splits
    pytest.param(10, 2, 64, 24, 0, 4416, [1000, 4352], id="g5_nh10_p64_s24"),
    pytest.param(5, 1, 64, 32, 1, 4416, [4352, 3001], id="g5_nh5_p64_s32_causal"),
    pytest.param(16, 4, 64, 17, 0, 1536, [700, 1472], id="g4_p64_s17"),                         # 512 threads: pipelined loader
    pytest.param(8, 4, 64, 8, 1, 1088, [1024, 0], id="g2_p64_s8_causal"),
    pytest.param(40, 8, 16, 12, 1, 4416, [4400, 2000], id="g5_nh40_p16_s12_causal"),
    pytest.param(8, 4, 16, 8, 1, 1024, [0, 1, 63, 64, 65, 500, 1000, 1008], id="g2_p16_s8_causal_nseq8"),
    pytest.param(16, 4, 16, 1, 0, 256, [63, 64], id="g4_p16_s1"),
    pytest.param(4, 4, 4, 1, 0, 512, [0, 131, 508], id="g1_p4_s1"),
    pytest.param(8, 8, 1, 12, 1, 256, [255, 17], id="g1_p1_s12"),
]


@pytest.mark.parametrize("nh,nkv,P,splits,causal,Lmax,kv", LLM_PROBES)
def test_llm_attn_probe(nh, nkv, P, splits, causal, Lmax, kv):
    """Exactly which keys every row attended, with which weight: the one-hot V channels spell out the weight of each selected key,
    the leak channel any weight on the sentinel keys past kv_len + P (the masked tail of the last tile included)."""
    q, K, VT = llm_probe(len(kv), nh, nkv, P, Lmax, kv, causal, seed=nh * 1000 + P + splits)
    got = run_llm(q, K, VT, kv, P, nh, nkv, splits, causal)
    ref, A = ref_llm(q, K, VT, kv, P, nh, nkv, causal)
    assert got[..., LEAK_QW].abs().max() == 0, "weight on a key past kv_len + P"
    assert_within(got, ref, tol_llm(ref, A, max(kv) + P), "llm_attn probe")


# (P, causal, Lmax, kv, form): the form follows from bdk_in_attn's LDS formulas --
#   in_attn_small_kernel<P> (P = 1 / 4): 4 P (((Lmax + 127) & ~63) + 4) floats <= 64 KiB  ->  P = 4: Lmax <= 896, P = 1: <= 3968;
#   in_attn_mfma_kernel (P = 16):       4 (16 (((Lmax + 127) & ~63) + 8) + 4096) bf16 <= 160 KiB  ->  Lmax <= 896;
#   in_attn_kernel (every P <= 16):      (1024 + 4160 + 16 (Lmax + 65)) floats <= 160 KiB  ->  Lmax <= 2112;  longer: refused.
IN_PROBES = [
    pytest.param(1, 0, 320, 319, "small", id="p1_small_256px_last"),
    pytest.param(1, 0, 3968, 3967, "small", id="p1_small_lmax3968"),
    pytest.param(4, 0, 320, 315, "small", id="p4_small_256px_last"),
    pytest.param(4, 1, 896, 500, "small", id="p4_small_causal_lmax896"),
    pytest.param(4, 1, 960, 500, "generic", id="p4_generic_causal_lmax960"),
    pytest.param(4, 0, 2112, 2108, "generic", id="p4_generic_lmax2112"),
    pytest.param(16, 0, 320, 303, "mfma", id="p16_mfma_256px_last"),
    pytest.param(16, 1, 320, 48, "mfma", id="p16_mfma_causal_first_step"),
    pytest.param(16, 1, 896, 63, "mfma", id="p16_mfma_causal_lmax896"),
    pytest.param(16, 0, 1088, 1072, "generic", id="p16_generic_512px_last"),
    pytest.param(16, 1, 2112, 2000, "generic", id="p16_generic_causal_lmax2112"),
]


@pytest.mark.parametrize("P,causal,Lmax,kv,form", IN_PROBES)
def test_in_attn_probe(P, causal, Lmax, kv, form):
    """The ImageNet attention's probe on each of its three forms (`form`: the kernel bdk_in_attn picks for P and Lmax)."""
    nh, nseq = 4, 3
    q, K, V = in_probe(nseq, nh, P, Lmax, kv, causal, seed=P * 10000 + Lmax)
    got = run_in(q, K, V, kv, P, causal)
    ref, A = ref_in(q, K, V, kv, P, causal)
    assert got[..., LEAK_IN].abs().max() == 0, "weight on a key past kv_len + P"
    assert_within(got, ref, tol_in(ref, A, kv + P), f"in_attn probe ({form})")


@pytest.mark.parametrize("P,causal,kv,lmax_fast,lmax_generic", [
    pytest.param(4, 0, 700, 896, 960, id="p4_small_vs_generic"),
    pytest.param(4, 1, 140, 896, 2112, id="p4_small_vs_generic_causal"),
    pytest.param(16, 1, 300, 896, 960, id="p16_mfma_vs_generic_causal"),
    pytest.param(16, 0, 880, 896, 2112, id="p16_mfma_vs_generic"),
])
def test_in_attn_forms_agree(P, causal, kv, lmax_fast, lmax_generic):
    """The same random keys in a cache of lmax_fast positions (small / mfma form) and of lmax_generic (in_attn_kernel): both within
    the bound of the reference and within one such bound of each other."""
    nseq, nh = 2, 4
    q, K, V = in_random(nseq, nh, P, lmax_fast, kv, seed=kv + P)
    pad = lambda t: torch.nn.functional.pad(t, (0, 0, 0, lmax_generic - lmax_fast))
    a = run_in(q, K, V, kv, P, causal)
    b = run_in(q, pad(K).contiguous(), pad(V).contiguous(), kv, P, causal)
    ref, A = ref_in(q, K, V, kv, P, causal)
    tol = tol_in(ref, A, kv + P)
    assert_within(a, ref, tol, "fast form")
    assert_within(b, ref, tol, "generic form")
    assert ((a - b).abs() <= tol.float()).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# random data at production geometry
def llm_random(nseq, nh, nkv, P, Lmax, seed, spread=1.5):
    """q ~ N(0, spread^2), K, V ~ N(0, 1), bf16: scaled scores ~ N(0, spread^2)."""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(nseq * P, nh, 128, generator=g) * spread).to(BF16)
    K = torch.randn(nseq, nkv, Lmax, 128, generator=g).to(BF16)
    VT = torch.randn(nseq, nkv, 128, Lmax, generator=g).to(BF16)
    return q.to(DEV), K.to(DEV), VT.to(DEV)


def in_random(nseq, nh, P, Lmax, kv, seed, spread=1.5):
    """q on a grid of 1/64, K on a grid of 1/16 (every q . k exact in fp32, so the bf16 score is the reference's), V ~ N(0, 1);
    the scores ~ N(0, spread^2).  Keys past kv + P hold the sentinel (the masked tail of the last tile)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.round(torch.randn(nseq * P, nh * 64, generator=g) * (spread / 8) * 64) / 64
    K = torch.round(torch.randn(nseq, nh, Lmax, 64, generator=g) * 16).clamp(-255, 255) / 16
    V = torch.randn(nseq, nh, Lmax, 64, generator=g)
    K[:, :, kv + P:] = 64.0
    V[:, :, kv + P:] = SENTINEL_V
    return q.to(BF16).to(DEV), K.to(BF16).to(DEV), V.to(BF16).to(DEV)


# (nh, nkv, P, splits, causal, Lmax, kv)
LLM_RANDOM = [
    pytest.param(40, 8, 64, 12, 0, 4416, [4300, 4211], id="headline_1024px_s12"),
    pytest.param(20, 4, 64, 24, 0, 4416, [4352, 4100], id="tp2_rank_s24"),
    pytest.param(10, 2, 64, 32, 0, 4416, [4290, 3900], id="tp4_rank_s32"),
    pytest.param(5, 1, 64, 32, 0, 4416, [4320, 4000], id="tp8_rank_s32"),
    pytest.param(40, 8, 16, 8, 0, 4416, [1000, 4300], id="p16_s8"),
    pytest.param(40, 8, 64, 8, 0, 1536, [1100, 1133, 1160, 1201, 1250, 1290, 1333, 1400], id="b4_nseq8_s8"),
    pytest.param(40, 8, 64, 8, 1, 1536, [0, 700], id="prefill_causal_s8"),
]


@pytest.mark.parametrize("nh,nkv,P,splits,causal,Lmax,kv", LLM_RANDOM)
def test_llm_attn_random(nh, nkv, P, splits, causal, Lmax, kv):
    """Random bf16 q / K / V at the geometry production launches: relative rms and per-element bounds of the module docstring."""
    q, K, VT = llm_random(len(kv), nh, nkv, P, Lmax, seed=sum(kv) + splits)
    got = run_llm(q, K, VT, kv, P, nh, nkv, splits, causal)
    ref, A = ref_llm(q, K, VT, kv, P, nh, nkv, causal)
    r = rel_rms(got, ref)
    assert r <= RMS_QW, (r, RMS_QW)
    assert_within(got, ref, tol_llm(ref, A, max(kv) + P), "llm_attn random")


# the released 256 px models: 64 class tokens, 256 image tokens, a cache of 320 positions; the first decode step sees
# kv_len = 64 + P - 1 cached tokens, the last one ends at position 319 (P = 16: kv_len 303, P = 4: 315, P = 1: 319)
IN_RANDOM = [
    pytest.param(16, 0, 320, 79, id="p16_first_decode"),
    pytest.param(16, 0, 320, 303, id="p16_last_decode"),
    pytest.param(16, 1, 320, 32, id="p16_first_step_causal_block"),
    pytest.param(4, 0, 320, 67, id="p4_first_decode"),
    pytest.param(4, 0, 320, 315, id="p4_last_decode"),
    pytest.param(1, 0, 320, 319, id="p1_last_decode"),
]


@pytest.mark.parametrize("P,causal,Lmax,kv", IN_RANDOM)
def test_in_attn_random(P, causal, Lmax, kv):
    nseq, nh = 16, 16
    q, K, V = in_random(nseq, nh, P, Lmax, kv, seed=P * 1000 + kv)
    got = run_in(q, K, V, kv, P, causal)
    ref, A = ref_in(q, K, V, kv, P, causal)
    r = rel_rms(got, ref)
    assert r <= RMS_IN, (r, RMS_IN)
    assert_within(got, ref, tol_in(ref, A, kv + P), "in_attn random")


# ---------------------------------------------------------------------------------------------------------------------------------
# the bounds see the bugs they are meant to see (reference domain only: no kernel runs here)
def _violates(bad, ref, tol, rms_bound=None):
    if not torch.isfinite(bad).all() or ((bad - ref).abs() > tol).any():
        return True
    return rms_bound is not None and rel_rms(bad, ref) > rms_bound


@pytest.mark.parametrize("causal", [0, 1])
def test_tolerances_see_the_faults(causal):
    """Each fault, computed in float64, violates the bounds the kernels are held to.

    * probes (Qwen3 and ImageNet): all four faults break the per-element bound.
    * random, Qwen3 headline (two sequences at ~4.3k keys, 12 splits): a dropped tile or a wrong split weight breaks the relative
      rms bound.  A single-key fault moves the output by ~1 / sqrt(L) = 1.5 % rms, above the 0.65 % bound: asserted too.
    * random, ImageNet 256 px (~300 keys): every fault is >= 1 / sqrt(320) = 5.6 % rms, asserted for all but the split fault (the
      ImageNet attention has no splits)."""
    nh, nkv, P, splits, Lmax = 10, 2, 64, 12, 4416
    kv = [4000, 4290] if causal else [4290, 4352 - 64]
    q, K, VT = llm_probe(2, nh, nkv, P, Lmax, kv, causal, seed=7)
    ref, A = ref_llm(q, K, VT, kv, P, nh, nkv, causal, splits)
    tol = tol_llm(ref, A, max(kv) + P)
    for f in FAULTS:
        bad, _ = ref_llm(q, K, VT, kv, P, nh, nkv, causal, splits, fault=f)
        assert _violates(bad, ref, tol), f"llm probe misses {f}"

    for Pi, Lm, kvi in ((16, 320, 200), (4, 960, 700), (1, 320, 200)):
        q, K, V = in_probe(2, 4, Pi, Lm, kvi, causal, seed=Pi)
        ref, A = ref_in(q, K, V, kvi, Pi, causal)
        tol = tol_in(ref, A, kvi + Pi)
        for f in FAULTS[:3]:
            bad, _ = ref_in(q, K, V, kvi, Pi, causal, fault=f)
            assert _violates(bad, ref, tol), f"in_attn probe (P {Pi}) misses {f}"

    kv = [4300, 4211]
    q, K, VT = llm_random(2, nh, nkv, P, Lmax, seed=11)
    ref, A = ref_llm(q, K, VT, kv, P, nh, nkv, causal, splits)
    tol = tol_llm(ref, A, max(kv) + P)
    for f in FAULTS:
        bad, _ = ref_llm(q, K, VT, kv, P, nh, nkv, causal, splits, fault=f)
        assert _violates(bad, ref, tol, RMS_QW), f"llm random misses {f}"

    for Pi, kvi in ((16, 79), (4, 315)):
        q, K, V = in_random(4, 4, Pi, 320, kvi, seed=3)
        ref, A = ref_in(q, K, V, kvi, Pi, causal)
        tol = tol_in(ref, A, kvi + Pi)
        for f in FAULTS[:3]:
            bad, _ = ref_in(q, K, V, kvi, Pi, causal, fault=f)
            assert _violates(bad, ref, tol, RMS_IN), f"in_attn random (P {Pi}) misses {f}"


# ---------------------------------------------------------------------------------------------------------------------------------
# refused before anything is launched
def test_unsupported_shapes_are_refused():
    from bitdance_amd._lib import BD_ERR_UNSUPPORTED, check
    l, st = _lib(), _stream()
    state = torch.full((65,), -7, dtype=torch.int32, device=DEV)
    buf = torch.zeros(1 << 20, device=DEV)                     # inputs and scratch (4 MiB) ...
    out = torch.zeros(1 << 20, device=DEV)                     # ... and the output of the two calls that run

    def llm(nseq=1, P=64, nh=40, nkv=8, Lmax=256, splits=8, kv=None):
        arr = (ctypes.c_int * nseq)(*(kv if kv is not None else [0] * nseq))
        return l.bd_llm_attn(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), arr, nseq, P, nh, nkv, Lmax, splits, 0,
                             state.data_ptr(), buf.data_ptr(), buf.data_ptr(), out.data_ptr(), 64, st)

    def ina(P=16, Lmax=320, kv=0, nseq=1):
        return l.bd_in_attn(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), kv, nseq, P, 4, Lmax, 0, state.data_ptr(),
                            out.data_ptr(), 64, st)

    assert llm(nh=48, nkv=8) == BD_ERR_UNSUPPORTED              # G 6 x 2 halves x 64 = 768 threads
    assert llm(P=33, nh=30, nkv=5) == BD_ERR_UNSUPPORTED        # G 6 x 2 halves
    assert llm(P=65) == BD_ERR_UNSUPPORTED
    assert llm(nh=40, nkv=7) == BD_ERR_UNSUPPORTED
    assert llm(Lmax=200) == BD_ERR_UNSUPPORTED
    assert llm(splits=0) == BD_ERR_UNSUPPORTED
    assert llm(nseq=65, P=1) == BD_ERR_UNSUPPORTED
    assert llm(kv=[193]) == BD_ERR_UNSUPPORTED                  # 193 + 64 > 256
    assert llm(nseq=2, kv=[0, -1]) == BD_ERR_UNSUPPORTED
    assert ina(P=17) == BD_ERR_UNSUPPORTED
    assert ina(P=16, kv=305) == BD_ERR_UNSUPPORTED              # 305 + 16 > 320
    assert ina(P=4, Lmax=2176) == BD_ERR_UNSUPPORTED            # past in_attn_kernel's LDS
    assert ina(P=16, Lmax=2176) == BD_ERR_UNSUPPORTED
    assert ina(P=1, Lmax=4032) == BD_ERR_UNSUPPORTED            # past in_attn_small_kernel<1>'s 64 KiB
    torch.cuda.synchronize()
    assert (state == -7).all(), "a refused call launched the state write"
    check(ina(P=1, Lmax=3968, kv=3967))                         # the longest caches that still run
    check(ina(P=4, Lmax=2112, kv=2108))
    torch.cuda.synchronize()


def test_step_reset_refuses_lengths_past_the_cache():
    """bd_step_reset: the step appends P keys at kv_len[i] inside sequence i's cache slice of Lmax positions."""
    from bitdance_amd import engine as E
    from bitdance_amd._lib import BitDanceHipError
    from oracle import tiny_models as tm
    c = tm.TINY_LLM
    sd = {k: v.to(DEV) for k, v in tm.seeded_state(tm.llm_shapes(c), 5).items()}
    lw = E.LlmWeights.from_state_dict(sd, c, DEV, keep_for_prefill=False)
    eng = E.Engine(None, None, lw, num_images=2, branches=1, device=DEV, max_tokens=64, max_kv=256)
    eng.reset([0, 256 - 64])
    for bad in ([0, 256 - 63], [-1, 0]):
        with pytest.raises(BitDanceHipError, match="kv_len"):
            eng.reset(bad)


# ---------------------------------------------------------------------------------------------------------------------------------
# in situ: the arguments the engine assembles
def _engine_attention_check(eng, nh, nkv, P, kv, causal):
    nseq, Lmax = len(kv), eng.Lmax
    rb = eng.Mpad // 32
    q = eng.view("llm.q", BF16, (eng.Mpad, nh, 128))[: nseq * P]
    K = eng.view("llm.k_cache", BF16, (nseq, nkv, Lmax, 128))
    VT = eng.view("llm.vt_cache", BF16, (nseq, nkv, 128, Lmax))
    got = unfrag(eng.ws["llm.attn_frag"].view(BF16)[: rb * 32 * nh * 128], rb, nh * 128)[: nseq * P].view(nseq * P, nh, 128).float()
    ref, A = ref_llm(q, K, VT, kv, P, nh, nkv, causal)
    assert_within(got, ref, tol_llm(ref, A, max(kv) + P), "engine attention")
    return K, VT


def test_engine_decode_attention_in_situ():
    """One Qwen3-14B-width decode layer with 12 splits over a cache longer than 2048: the attention output the step wrote
    against float64 attention on the q and caches the step itself left on the device."""
    from bitdance_amd import engine as E
    from oracle import tiny_models as tm, true_dims as td
    c = dict(td.QWEN3_14B, num_hidden_layers=1)
    nh, nkv, P, kv = c["num_attention_heads"], c["num_key_value_heads"], 64, [4100, 3987]
    sd = {k: v.to(BF16) for k, v in td.device_seeded_state(tm.llm_shapes(c), 202, DEV).items()}
    lw = E.LlmWeights.from_state_dict(sd, c, DEV, keep_for_prefill=False)
    del sd
    eng = E.Engine(None, None, lw, num_images=2, branches=1, device=DEV, max_tokens=P, max_kv=max(kv) + 2 * P,
                   parallel_num=P, attn_splits=12)
    assert eng.Lmax > 2048
    g = torch.Generator(device=DEV).manual_seed(203)
    K = eng.view("llm.k_cache", BF16, (2, nkv, eng.Lmax, 128))
    VT = eng.view("llm.vt_cache", BF16, (2, nkv, 128, eng.Lmax))
    K.copy_(torch.randn(K.shape, generator=g, device=DEV))
    VT.copy_(torch.randn(VT.shape, generator=g, device=DEV))
    eng.set_int("rt.emit_cond", 0)
    eng.reset(kv)
    eng.residual()[: 2 * P].copy_(torch.randn(2 * P, c["hidden_size"], generator=g, device=DEV))
    eng.llm_step()
    torch.cuda.synchronize()
    _engine_attention_check(eng, nh, nkv, P, kv, causal=0)


def test_engine_causal_prefill_attention_in_situ():
    """A native causal prefill block (llm._run_block: rt.llm_causal / rt.llm_bf16 / rt.no_advance) with ragged per-sequence
    lengths at tiny dims: attention against float64 on the device's own q and caches, and the block's K / V appended at
    kv_len[i] .. kv_len[i] + P - 1 of sequence i, nowhere else."""
    from bitdance_amd import engine as E, llm
    from oracle import tiny_models as tm
    c = dict(tm.TINY_LLM, num_hidden_layers=1)
    nh, nkv, P, kv = c["num_attention_heads"], c["num_key_value_heads"], 64, [0, 37, 128, 191]
    sd = {k: v.to(DEV) for k, v in tm.seeded_state(tm.llm_shapes(c), 9).items()}
    lw = E.LlmWeights.from_state_dict(sd, c, DEV, keep_for_prefill=False)
    eng = E.Engine(None, None, lw, num_images=4, branches=1, device=DEV, max_tokens=P, max_kv=256)
    g = torch.Generator(device=DEV).manual_seed(10)
    K = eng.view("llm.k_cache", BF16, (4, nkv, eng.Lmax, 128))
    VT = eng.view("llm.vt_cache", BF16, (4, nkv, 128, eng.Lmax))
    K.copy_(torch.randn(K.shape, generator=g, device=DEV))
    VT.copy_(torch.randn(VT.shape, generator=g, device=DEV))
    K0, VT0 = K.clone(), VT.clone()
    rows = [torch.randn(P, c["hidden_size"], generator=g, device=DEV).to(BF16) for _ in kv]
    llm._run_block(eng, rows, kv, causal=True)
    torch.cuda.synchronize()
    _engine_attention_check(eng, nh, nkv, P, kv, causal=1)
    for s, L0 in enumerate(kv):
        new = torch.zeros(eng.Lmax, dtype=torch.bool, device=DEV)
        new[L0:L0 + P] = True
        assert torch.equal(K[s][:, ~new], K0[s][:, ~new]) and torch.equal(VT[s][:, :, ~new], VT0[s][:, :, ~new]), s
        assert (K[s][:, new] != K0[s][:, new]).any(-1).all() and (VT[s][:, :, new] != VT0[s][:, :, new]).any(1).all(), s
