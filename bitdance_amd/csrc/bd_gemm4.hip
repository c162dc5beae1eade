// MXFP4 weight path of the weight-streaming GEMM ("wdtype" 3, weights="fp4a"): the GEMMs that run fp8 x fp8 in "fp8a" (head adaLN /
// qkv / w1, LLM q/k/v and gate/up) with their weights stored as OCP MXFP4 along K -- e2m1 elements (0, 0.5, 1, 1.5, 2, 3, 4, 6, signed),
// one E8M0 exponent byte per 32 consecutive k of an output channel, no per-channel factor -- on the same block-scaled MFMA with the B
// format switched to e2m1 (bd_gemm_kernel.h WT = 3, mfma32_f8f4).  Activations, row scales, epilogues and launch table: bdk_gemm8a.
// A translation unit of its own so that its 16 instances compile beside bd_gemm8.hip's.
//
// Source form (engine.quantize_rows_mxfp4): codes [rows][K / 2] bytes, k = 2 b in the low nibble of byte b and k = 2 b + 1 in the high
// one (bit 3 of a nibble = sign); exponents [rows][K / 32] bytes.
// Packed weights: 1 KiB per (32-row panel, 64-deep stage); lane l = the 16 source bytes of row panel * 32 + (l & 31) that hold
// k = stage * 64 + (l >> 5) * 32 .. + 31.  Chunks of a panel are contiguous in K.
// Packed exponents: dwords [panel][g < ceil(K / 256)][lane l]; byte b = the exponent of row (l & 31), k block 2 (4 g + b) + (l >> 5),
// i.e. of the lane's weights in stage 4 g + b; stages past K carry 127 (2^0) and are never multiplied.
#include "bd_gemm_kernel.h"

__global__ void pack_w4k_kernel(u32x4* __restrict__ dst, unsigned* __restrict__ dst_e, const unsigned char* __restrict__ src,
                                const unsigned char* __restrict__ src_e, const unsigned char* __restrict__ src2,
                                const unsigned char* __restrict__ src2_e, int panels, int K, int nb0, int mode) {
    const int KS = K >> 6, EG = (KS + 3) >> 2;               // 64-deep stages, exponent dwords per lane
    const size_t total = (size_t)panels * KS * 64;
    for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (size_t)gridDim.x * blockDim.x) {
        const int l = (int)(u & 63);
        const size_t c = u >> 6;
        const int kk = (int)(c % KS);
        const int pn = (int)(c / KS);
        const int i = l & 31;
        // mode 1 (SwiGLU): a panel = 16 gate rows, then the 16 matching up rows (pack_w8k_kernel)
        const bool second = (mode != 0) && i >= 16;
        const size_t r = (mode == 0) ? (size_t)pn * 32 + i : (size_t)pn * 16 + (i & 15);
        const unsigned char* row = (second ? src2 : src) + r * (size_t)(K >> 1);
        dst[((size_t)(nb0 + pn) * KS + kk) * 64 + l] = *reinterpret_cast<const u32x4*>(row + kk * 32 + (l >> 5) * 16);
        if ((kk & 3) == 0) {
            const unsigned char* er = (second ? src2_e : src_e) + r * (size_t)(K >> 5);
            unsigned v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const unsigned e = (kk + b < KS) ? er[2 * (kk + b) + (l >> 5)] : 127u;
                v |= e << (8 * b);
            }
            dst_e[((size_t)(nb0 + pn) * EG + (kk >> 2)) * 64 + l] = v;
        }
    }
}

int bdk_pack_w4k(void* dst, void* dst_e, const void* src, const void* src_e, const void* src2, const void* src2_e, int panels, int K, int nb0,
                 int panels_total, int mode, hipStream_t st) {
    if (K % 64 || K < 64 || panels < 0 || nb0 < 0 || nb0 + panels > panels_total) return -2;
    if (!dst || !dst_e || !src || !src_e || (mode != 0 && (!src2 || !src2_e))) return -7;
    const size_t total = (size_t)panels * (K / 64) * 64;
    if (total == 0) return 0;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    BD_LAUNCH(pack_w4k_kernel, dim3(blocks), dim3(256), 0, st, (u32x4*)dst, (unsigned*)dst_e, (const unsigned char*)src,
              (const unsigned char*)src_e, (const unsigned char*)src2, (const unsigned char*)src2_e, panels, K, nb0, mode);
    return bd_launch_status();
}

// MXFP4 weights x fp8 activations (A: the A8 layout + `ascale` [rows] fp32; `wexp`: the packed exponent stream): the launch forms of
// bdk_gemm8a, instance for instance
int bdk_gemm4a(const GemmCall& c, hipStream_t st) {
    if (c.wait) return -10;                                  // (the sequence-parallel hand-off carries bf16 rows only)
    const int RB = c.RB, N = c.N, K = c.K, S = c.S, epi = c.epi, nw = c.nw & 15, kw = ((c.nw >> 8) & 3) + 1;
    if (kw > 2 || nw == 0 || nw % kw || !c.ascale || !c.wexp || !c.A || !c.W) return -7;
    const int np = nw / kw;
    if (K < 64 || K % (64 * kw) || N < 32 || N % (32 * np) || S < 1 || RB < 1) return -2;
    if (bd_gemm_empty_split(K / (64 * kw), S)) return -3;
    if (epi != BD_EPI_PARTIAL && S != 1 && (c.out_partial == nullptr || c.cnt == nullptr)) return -4;
    const size_t PS = (size_t)(K >> 6) * 64, SS = 64;        // 16 B units: panel stride, 64-deep stage stride (one load per lane)
    GemmP p{(const u32x4*)c.A, (const u32x4*)c.W, c.out_partial, (bf16_t*)c.out_act, (const bf16_t*)c.bias, c.cnt, (const float*)c.wexp, RB, N, K, S, RB * 32, PS, SS};
    p.ascale = c.ascale;
    const int MB = (RB % 8 == 0 && kw == 1 && np == 4 && S == 1 && epi == BD_EPI_BF16) ? 8 : ((RB % 4 == 0) ? 4 : RB);   // (256-row passes: bdk_gemm8a)
    if (MB != 8 && MB != 4 && MB != 2 && MB != 1) return -5;
    // ring 4 as in bdk_gemm8a: a stage is 1 KiB + 256 B per wave, the loop is bound by bytes in flight
#define BD_CASE4A(NPV, KWV, MBV) if (np == NPV && kw == KWV && MB == MBV) return launch_gemm<NPV, KWV, MBV, 4, 0, 3>(p, epi, st);
    BD_CASE4A(4, 1, 8)
    BD_CASE4A(4, 1, 4) BD_CASE4A(8, 1, 4) BD_CASE4A(2, 1, 4) BD_CASE4A(4, 2, 4) BD_CASE4A(2, 2, 4)
    BD_CASE4A(4, 1, 2) BD_CASE4A(8, 1, 2) BD_CASE4A(2, 1, 2) BD_CASE4A(4, 2, 2) BD_CASE4A(2, 2, 2)
    BD_CASE4A(4, 1, 1) BD_CASE4A(8, 1, 1) BD_CASE4A(2, 1, 1) BD_CASE4A(4, 2, 1) BD_CASE4A(2, 2, 1)
#undef BD_CASE4A
    return -6;
}
