// bf16 MFMA GEMMs for the DiChaViT encoder (gfx950), NT form; the weight gradients (TN form) are in gemm_tn.hip.
//
//  gemm_nt : C[M,N] = A[M,K] . W[N,K]^T   (both operands K-contiguous)  + fused epilogues.
//            Replaces nn.Linear forward (models/vit.py:116,119,72-74) and, with the transposed bf16
//            weight copy, its input gradient; also the Conv3d(1,D,(1,P,P)) patch projection on the
//            im2col'd image (models/dichavit.py:77-82,377) with the +bias +channel_embed +pos epilogue
//            (dichavit.py:409-411, 565).
//
// gemm_nt: persistent 256x128 (8 waves, 3-stage LDS-DMA ring) and 256x384 (two 80 KB stages) kernels, geometry below; for K = 384 the
//          weight-stationary kernel (a 384-column W slice in registers, 32-row A panels through the ring).
#include <algorithm>
#include <type_traits>
#include "dcv_common.hpp"
#include "../../include/dcv.h"

namespace {


struct GemmNtArgs {
    const bf16_t* A;
    int lda;
    const bf16_t* W;
    int ldw;
    int M, N, K;
    const float* bias;
    void* out;
    int ldo;
    void* out2;
    int ldo2;
    const void* aux;
    int ldaux;
    const float* aux2;
    int T, n;
    // residual + LayerNorm epilogue (gemm_nt384_kernel<DCV_EPI_RESID_LN>, N == 384): gamma / beta [N], mean / rstd [M] out, out2 = bf16 LN output
    const float* ln_g;
    const float* ln_b;
    float* ln_mean;
    float* ln_rstd;
    float ln_eps;
    // gemm_nt384_kernel's row-tile plan (dcv_gemm_nt384_plan): row tiles 0 .. n256-1 are 256 rows high, n256 .. tiles_m-1 are 192 rows high
    int n256, tiles_m;
};
constexpr int DCV_EPI_RESID_LN = 6;  // kernel-internal: reached through dcv_gemm_nt_resid_ln only

// erf by Abramowitz-Stegun 7.1.26 (|abs err| <= 1.5e-7: far below the bf16 rounding of the outputs), sharing
// e = exp(-z^2/2) with the Gaussian pdf of GELU':  GELU(z) = z * cdf,  GELU'(z) = cdf + z * e / sqrt(2 pi).
// Two elements at a time (v_pk_mul_f32 / v_pk_fma_f32 / v_pk_add_f32; rcp and exp2 stay scalar): g = GELU(z), gp = GELU'(z).
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void gelu_parts2(f32x2_t z, f32x2_t& g, f32x2_t& gp) {
    f32x2_t ax = {fabsf(z.x), fabsf(z.y)};
    const f32x2_t d = ax * 0.23164189f + 1.0f;  // 1 + 0.3275911 |z| / sqrt 2
    const f32x2_t t = {__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
    const f32x2_t zz = z * z * -0.72134752044448170f;
    const f32x2_t e = {__builtin_amdgcn_exp2f(zz.x), __builtin_amdgcn_exp2f(zz.y)};
    f32x2_t poly = t * 1.061405429f + -1.453152027f;
    poly = poly * t + 1.421413741f;
    poly = poly * t + -0.284496736f;
    poly = poly * t + 0.254829592f;
    poly = poly * t;
    const f32x2_t h = poly * e * -0.5f + 0.5f;  // 0.5 erfc-part: cdf(|z|) - 0.5 = 0.5 - 0.5 poly e
    // cdf(z) = 0.5 + sign(z) * h
    const f32x2_t sh = {copysignf(h.x, z.x), copysignf(h.y, z.y)};
    const f32x2_t cdf = sh + 0.5f;
    g = z * cdf;
    gp = z * e * 0.39894228040143268f + cdf;
}
__device__ __forceinline__ uint4 pack8_bf16(const float* v) {
    uint2 lo = pack4_bf16(v[0], v[1], v[2], v[3]), hi = pack4_bf16(v[4], v[5], v[6], v[7]);
    return make_uint4(lo.x, lo.y, hi.x, hi.y);
}
__device__ __forceinline__ void unpack8_bf16(uint4 u, float* v) {
    v[0] = __uint_as_float(u.x << 16); v[1] = __uint_as_float(u.x & 0xffff0000u);
    v[2] = __uint_as_float(u.y << 16); v[3] = __uint_as_float(u.y & 0xffff0000u);
    v[4] = __uint_as_float(u.z << 16); v[5] = __uint_as_float(u.z & 0xffff0000u);
    v[6] = __uint_as_float(u.w << 16); v[7] = __uint_as_float(u.w & 0xffff0000u);
}
// Streaming (non-temporal) 16-byte accesses for data this kernel touches exactly once — the output tile, the residual
// and the saved pre-activation: they must not evict the A row-panel, which the other column tiles of the same XCD are
// about to re-read, from the 4 MB L2 (PMC before: fc1 fetched its 77 MB A operand 3.3 times).
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void st128_stream(void* p, uint4 v) {
    u32x4_t x = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(x, reinterpret_cast<u32x4_t*>(p));
}
__device__ __forceinline__ uint4 ld128_stream(const void* p) {
    u32x4_t x = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p));
    return make_uint4(x.x, x.y, x.z, x.w);
}
__device__ __forceinline__ void load8_f32(const float* p, float* v) {
    float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// bf16-output epilogues on 8 consecutive columns n..n+7 of row m (16-byte global accesses; N % 8 == 0), split in two so that the
// auxiliary global loads of all passes are in flight together before any of them is consumed:
//   epi_aux8   : loads what the epilogue needs from global memory (the saved GELU'(z) of the GELU backward, nothing for the others)
//                — (m, n) are clamped by the caller, so it needs no predicate;
//   epi_store8 : adds the lane's bias values, applies the fused op and stores (caller predicates).
// The fp32-output epilogues (residual, patch embedding) are epi_aux4 / epi_store4 below.
template <int EPI>
__device__ __forceinline__ void epi_aux8(const GemmNtArgs& a, int m, int n, float* x) {
    if constexpr (EPI == DCV_EPI_GELU_BWD_BF16) unpack8_bf16(ld128_stream((const bf16_t*)a.aux + (size_t)m * a.ldaux + n), x);
}

template <int EPI>
__device__ __forceinline__ void epi_store8(const GemmNtArgs& a, int m, int n, float* v, const float* x, const float* bz) {
    if constexpr (EPI == DCV_EPI_BIAS_BF16) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += bz[e];
        st128_stream((bf16_t*)a.out + (size_t)m * a.ldo + n, pack8_bf16(v));
    } else if constexpr (EPI == DCV_EPI_BIAS_GELU_BF16) {
        // out = GELU'(z), out2 = GELU(z), z = acc + bias in fp32: the backward then only multiplies (the first version saved z
        // and recomputed the erf / exp in the backward epilogue, ~45 % of that kernel's time); cdf and exp(-z^2/2) are shared
        float gp[8];
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
            const f32x2_t z = {v[e] + bz[e], v[e + 1] + bz[e + 1]};
            f32x2_t g2, gp2;
            gelu_parts2(z, g2, gp2);
            v[e] = g2.x; v[e + 1] = g2.y;
            gp[e] = gp2.x; gp[e + 1] = gp2.y;
        }
        st128_stream((bf16_t*)a.out + (size_t)m * a.ldo + n, pack8_bf16(gp));
        st128_stream((bf16_t*)a.out2 + (size_t)m * a.ldo2 + n, pack8_bf16(v));
    } else if constexpr (EPI == DCV_EPI_PLAIN_BF16) {
        st128_stream((bf16_t*)a.out + (size_t)m * a.ldo + n, pack8_bf16(v));
    } else if constexpr (EPI == DCV_EPI_GELU_BWD_BF16) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] *= x[e];  // x = GELU'(z) as the forward epilogue saved it
        st128_stream((bf16_t*)a.out + (size_t)m * a.ldo + n, pack8_bf16(v));
    }
}

// ---- register epilogue (round 3) -------------------------------------------------------------------------------------------
// The MFMAs are issued with the operands SWAPPED (W fragment as the A operand, activation fragment as B), so a wave's 16 x 16
// accumulator tile (i, j) holds, in lane (r16 = lane & 15, kg = lane >> 4), output row m = 16 i + r16 and the FOUR CONSECUTIVE
// columns n = 16 j + 4 kg .. +3 — row-contiguous data in every lane, which two register shuffles turn into full cache lines:
//   1. bf16 outputs only: four v_permlane16_swap per tile pair (j, j + 1) leave lane (r16, kg) with the EIGHT consecutive columns
//      16 (j + (kg & 1)) + 8 (kg >> 1) .. +7 of its row (the swap exchanges the odd 16-lane rows of its first operand with the even
//      rows of its second): 16 bytes per lane, but still only 4 lanes = 64 bytes per output row and instruction;
//   2. a DPP exchange between lanes l and l ^ 8 (row_ror:8, two v_mov_dpp per register) between two such column halves: afterwards
//      one store instruction covers rows rr = r16 & 7 (+ 8 for the second instruction) with EIGHT lanes per row — 8 rows x 128
//      contiguous bytes, whole cache lines, exactly what the LDS slab of rounds 1-2 produced.  (Measured without step 2: 16 half-lines
//      per instruction instead of 8 lines made every epilogue 5-25 % SLOWER than the slab — the store path is bound by the number of
//      lines an instruction touches, not by bytes; gpurun r3b.)
// Final layout of a lane inside a column group: bf16: 64-column group, 8 columns at 32 (r16 >> 3) + 16 (kg & 1) + 8 (kg >> 1);
// fp32: 32-column group (a tile pair), 4 columns at 16 (r16 >> 3) + 4 kg; rows rr and rr + 8 of the 16-row block.
// No LDS: the whole ring is free for the next tile's prefetch and no workgroup barrier separates the k-loop from the epilogue.
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void swap_pair8(const f32x4& t0, const f32x4& t1, float* v) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const u32x2_t u = __builtin_amdgcn_permlane16_swap(__float_as_uint(t0[r]), __float_as_uint(t1[r]), false, false);
        v[r] = __uint_as_float(u[0]);
        v[4 + r] = __uint_as_float(u[1]);
    }
}
// x (lower column half) / y (upper column half), both held for row r16: afterwards a = (row rr: x of lanes r16 < 8 | y of lane l - 8),
// b = (row rr + 8: x of lane l + 8 | y of lanes r16 >= 8)
__device__ __forceinline__ void xchg_rows8(float x, float y, float& a, float& b) {
    const int xi = __float_as_int(x), yi = __float_as_int(y);
    a = __int_as_float(__builtin_amdgcn_update_dpp(xi, yi, 0x128, 0xF, 0xC, false));  // lanes 8-15 of every row: y[l ^ 8]
    b = __int_as_float(__builtin_amdgcn_update_dpp(yi, xi, 0x128, 0xF, 0x3, false));  // lanes 0-7: x[l ^ 8]
}
// fp32-output epilogues on 4 consecutive columns n .. n+3 of row m
template <int EPI>
__device__ __forceinline__ void epi_aux4(const GemmNtArgs& a, int m, int n, float* x) {
    if constexpr (EPI == DCV_EPI_BIAS_RESID_F32) {
        // residual is read from aux when given (out-of-place keeps the layer input alive for the LayerNorm backward
        // at no extra traffic), else the output is updated in place
        const float* rsd = a.aux ? (const float*)a.aux + (size_t)m * a.ldaux + n : (const float*)a.out + (size_t)m * a.ldo + n;
        const float4 v = *reinterpret_cast<const float4*>(rsd);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else if constexpr (EPI == DCV_EPI_PATCH) {
        // row m = b*T + t ; token t = c*n + i  ->  channel_embed[c] + pos[1+i]
        const int b = m / a.T, t = m - b * a.T;
        const int c = t / a.n, i = t - c * a.n;
        const float4 e = *reinterpret_cast<const float4*>((const float*)a.aux + (size_t)c * a.ldaux + n);
        const float4 p = *reinterpret_cast<const float4*>(a.aux2 + (size_t)(1 + i) * a.ldaux + n);
        x[0] = e.x + p.x; x[1] = e.y + p.y; x[2] = e.z + p.z; x[3] = e.w + p.w;
    }
}
template <int EPI>
__device__ __forceinline__ void epi_store4(const GemmNtArgs& a, int m, int n, const f32x4& acc, const float* x, const float4& bz) {
    float4 v = make_float4(acc[0] + bz.x, acc[1] + bz.y, acc[2] + bz.z, acc[3] + bz.w);
    if constexpr (EPI == DCV_EPI_BIAS_RESID_F32) {
        if (a.aux2) {  // stochastic depth (vit.py:37-56, 397-398): the branch of sample b = m / T is multiplied by aux2[b] = keep_b / keep_prob
            const float sc = a.aux2[m / a.T];
            v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc;
        }
        v.x += x[0]; v.y += x[1]; v.z += x[2]; v.w += x[3];
        *reinterpret_cast<float4*>((float*)a.out + (size_t)m * a.ldo + n) = v;
    } else if constexpr (EPI == DCV_EPI_PATCH) {
        const int b = m / a.T, t = m - b * a.T;
        if (a.out2) *reinterpret_cast<float4*>((float*)a.out2 + (size_t)m * a.ldo2 + n) = v;  // pre-embedding tokens (ortho loss input)
        v.x += x[0]; v.y += x[1]; v.z += x[2]; v.w += x[3];
        *reinterpret_cast<float4*>((float*)a.out + ((size_t)b * (a.T + 1) + 1 + t) * a.ldo + n) = v;
    }
}
template <int EPI>
__device__ constexpr bool epi_f32out() { return EPI == DCV_EPI_BIAS_RESID_F32 || EPI == DCV_EPI_PATCH; }

// Epilogue of a wave's (16 RB)-row x (16 NJ)-column block of accumulators acc[RB][J0 .. J0 + NJ) (NJ a multiple of 4; RB = 4 row blocks except
// in gemm_nt384_kernel's 192-row tiles, RB a multiple of NI), rows m_w + 16 i + ..,
// columns n_w + ..; `between()` runs after the first auxiliary loads have been issued and before anything is stored (the persistent
// kernels put the next tile's prefetch there).  NI: row blocks (of 16 rows) whose auxiliary loads are issued together (4 = all of
// them before `between`; fewer = fewer registers).  bz: the lane's bias values in its final layout (nt_load_bias).
template <int EPI, int NI, int NJ, int NJT, int J0, int RB, class Between>
__device__ __forceinline__ void nt_epilogue_block(const GemmNtArgs& a, const f32x4 (&acc)[RB][NJT], int m_w, int n_w, int r16, int kg,
                                                  const float* bz, Between&& between) {
    constexpr bool HAS_AUX = (EPI == DCV_EPI_BIAS_RESID_F32) || (EPI == DCV_EPI_GELU_BWD_BF16) || (EPI == DCV_EPI_PATCH);
    const int rr = r16 & 7, hi = r16 >> 3;
    if constexpr (epi_f32out<EPI>()) {
        constexpr int NG = NJ / 2;  // 32-column groups
        const int cl = 16 * hi + 4 * kg;
#pragma unroll
        for (int ib = 0; ib < RB; ib += NI) {
            float x[NI][NG][2][4];
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int c = 0; c < NG; ++c)
#pragma unroll
                    for (int h = 0; h < 2; ++h)
                        epi_aux4<EPI>(a, min(m_w + 16 * (ib + i) + 8 * h + rr, a.M - 1), min(n_w + 32 * c + cl, a.N - 4), x[i][c][h]);
            if (ib == 0) between();
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int c = 0; c < NG; ++c) {
                    f32x4 va, vb;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float fa, fb;
                        xchg_rows8(acc[ib + i][J0 + 2 * c][r], acc[ib + i][J0 + 2 * c + 1][r], fa, fb);
                        va[r] = fa; vb[r] = fb;
                    }
                    const int m = m_w + 16 * (ib + i) + rr, n = n_w + 32 * c + cl;
                    const float4 b4 = make_float4(bz[4 * c], bz[4 * c + 1], bz[4 * c + 2], bz[4 * c + 3]);
                    if (m < a.M && n < a.N) epi_store4<EPI>(a, m, n, va, x[i][c][0], b4);
                    if (m + 8 < a.M && n < a.N) epi_store4<EPI>(a, m + 8, n, vb, x[i][c][1], b4);
                }
        }
    } else {
        constexpr int NG = NJ / 4;  // 64-column groups
        const int cl = 32 * hi + 16 * (kg & 1) + 8 * (kg >> 1);
#pragma unroll
        for (int ib = 0; ib < RB; ib += NI) {
            float x[HAS_AUX ? NI : 1][HAS_AUX ? NG : 1][2][8];
            if constexpr (HAS_AUX) {
#pragma unroll
                for (int i = 0; i < NI; ++i)
#pragma unroll
                    for (int c = 0; c < NG; ++c)
#pragma unroll
                        for (int h = 0; h < 2; ++h)
                            epi_aux8<EPI>(a, min(m_w + 16 * (ib + i) + 8 * h + rr, a.M - 1), min(n_w + 64 * c + cl, a.N - 8), x[i][c][h]);
            }
            if (ib == 0) between();
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int c = 0; c < NG; ++c) {
                    float v0[8], v1[8], va[8], vb[8];
                    swap_pair8(acc[ib + i][J0 + 4 * c], acc[ib + i][J0 + 4 * c + 1], v0);
                    swap_pair8(acc[ib + i][J0 + 4 * c + 2], acc[ib + i][J0 + 4 * c + 3], v1);
#pragma unroll
                    for (int e = 0; e < 8; ++e) xchg_rows8(v0[e], v1[e], va[e], vb[e]);
                    const int m = m_w + 16 * (ib + i) + rr, n = n_w + 64 * c + cl;
                    if (m < a.M && n < a.N) epi_store8<EPI>(a, m, n, va, x[HAS_AUX ? i : 0][HAS_AUX ? c : 0][0], bz + 8 * c);
                    if (m + 8 < a.M && n < a.N) epi_store8<EPI>(a, m + 8, n, vb, x[HAS_AUX ? i : 0][HAS_AUX ? c : 0][1], bz + 8 * c);
                }
        }
    }
}
// the lane's bias values for a block of NJ column tiles starting at column n_w, in its final layout: fp32 outputs NJ / 2 x 4 floats,
// bf16 outputs NJ / 4 x 8 floats (2 NJ floats either way)
template <int EPI, int NJ>
__device__ __forceinline__ void nt_load_bias(const GemmNtArgs& a, int n_w, int r16, int kg, float* bz) {
    const int hi = r16 >> 3;
    if constexpr (epi_f32out<EPI>()) {
#pragma unroll
        for (int c = 0; c < NJ / 2; ++c) {
            const float4 b = *reinterpret_cast<const float4*>(a.bias + min(n_w + 32 * c + 16 * hi + 4 * kg, a.N - 4));
            bz[4 * c] = b.x; bz[4 * c + 1] = b.y; bz[4 * c + 2] = b.z; bz[4 * c + 3] = b.w;
        }
    } else {
#pragma unroll
        for (int c = 0; c < NJ / 4; ++c) load8_f32(a.bias + min(n_w + 64 * c + 32 * hi + 16 * (kg & 1) + 8 * (kg >> 1), a.N - 8), bz + 8 * c);
    }
}

// gemm_nt geometry: 256 x 128 output tile, 8 waves as 4 (M) x 2 (N), each wave 64 x 64 = 4 x 4 MFMA 16x16x32 tiles
// (same FLOPs per cycle as 32x32x16, but the power-limited chip clocks higher on it: NT GEMMs 3-9 % faster, profiles/r02_x4_*).
// Measured on MI355X (tools/ab_bench.py ablations, M = 100 416, K = 384):
//   * the main loop alone sustains ~965 TFLOP/s: operands arrive by LDS-DMA, whole 128-byte lines (8 rows x 128 B per
//     instruction), K streamed in 64-wide stages through a 3-deep ring (two 48 KB stages always in flight);
//   * the epilogue costs as much again (N = 1152: 92 us loop + 63 us epilogue; fc1 + GELU: 122 + 166 us): with every CU storing at
//     once it runs at the HBM write rate (~5.3 TB/s chip-wide, profiles/r03_x8_*), and the board is at its power cap (r03_x6_*).
// So the kernel is PERSISTENT: one workgroup per CU walks output tiles; after a tile's last stage it first issues the
// auxiliary loads of its epilogue, then the NEXT tile's first two ring stages, and only then applies the fused op and stores —
// straight from the accumulators (register epilogue above; rounds 1-2 went through wave-private LDS slabs), with no workgroup
// barrier — so the store tail and the GELU arithmetic overlap the next tile's operand streaming.
#ifndef DCV_N3_EARLY_AT
#define DCV_N3_EARLY_AT 11  // gemm_nt384_kernel: waves 0-3 issue their DMA pieces behind MFMA step N of the stage (11 = between the two k-steps), waves 4-7 at the top; -1: all at the top.  Stamps (profiles/r03_x1_*): with all eight waves issuing first the matrix pipe idled ~640 cycles per stage (80 pieces x 16 TA cycles, older waves served first); -4 ... -8 % on the k-loop-heavy shapes
#endif
constexpr int NT_BM = 256, NT_BN = 128, NT_BK = 64, NT_STAGES = 3;
constexpr int NT_A_BYTES = NT_BM * NT_BK * 2, NT_W_BYTES = NT_BN * NT_BK * 2, NT_STAGE_BYTES = NT_A_BYTES + NT_W_BYTES;  // 48 KB
constexpr int NT_SMEM = NT_STAGES * NT_STAGE_BYTES;  // the ring (the epilogue uses no LDS since round 3)

// store instructions one wave issues in a full tile's epilogue (8 row-chunks of 8 columns per lane)
template <int EPI>
__device__ constexpr int nt_stores_per_wave() {
    return (EPI == DCV_EPI_BIAS_GELU_BF16 || EPI == DCV_EPI_BIAS_RESID_F32) ? 16 : 8;
}

struct NtTile {
    const bf16_t* gA[4];
    const bf16_t* gW[2];
    int m0, n0;
};

__device__ __forceinline__ void nt_tile_setup(const GemmNtArgs& a, int L, int tiles_n, int wave, int lane, NtTile& t) {
    const int tm = L / tiles_n, tn = L - tm * tiles_n;
    t.m0 = tm * NT_BM;
    t.n0 = tn * NT_BN;
    // one DMA instruction = 8 rows x 128 B (lane -> row lane>>3, physical chunk lane&7); the swizzle
    // (physical chunk = logical ^ swz64n(row)) is applied to the per-lane SOURCE chunk, the destination is linear.
    // Wave w fills A rows [32w, 32w+32) (4 instructions) and W rows [16w, 16w+16) (2 instructions): 6 per stage.
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = 32 * wave + 8 * q + (lane >> 3);
        t.gA[q] = a.A + (size_t)min(t.m0 + row, a.M - 1) * a.lda + (((lane & 7) ^ swz64n(row)) * 8);
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int row = 16 * wave + 8 * q + (lane >> 3);
        t.gW[q] = a.W + (size_t)min(t.n0 + row, a.N - 1) * a.ldw + (((lane & 7) ^ swz64n(row)) * 8);
    }
}

__device__ __forceinline__ void nt_issue(const NtTile& t, int kt, unsigned stage_base, unsigned dmaA, unsigned dmaW) {
    glds16(t.gA[0] + kt * NT_BK, stage_base + dmaA);
    glds16(t.gA[1] + kt * NT_BK, stage_base + dmaA + 1024);
    glds16(t.gA[2] + kt * NT_BK, stage_base + dmaA + 2048);
    glds16(t.gA[3] + kt * NT_BK, stage_base + dmaA + 3072);
    glds16(t.gW[0] + kt * NT_BK, stage_base + dmaW);
    glds16(t.gW[1] + kt * NT_BK, stage_base + dmaW + 1024);
}

template <int EPI>
__global__ __launch_bounds__(512) void gemm_nt_kernel(GemmNtArgs a) {
    // ONE shared array (a second __shared__ object can make hipcc drain vmcnt before every ds_read)
    __shared__ __attribute__((aligned(16))) char smem[NT_SMEM];
    constexpr bool HAS_BIAS = (EPI != DCV_EPI_PLAIN_BF16) && (EPI != DCV_EPI_GELU_BWD_BF16);
    constexpr int S = nt_stores_per_wave<EPI>();
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const bool late = (wave >> 2) != 0;  // waves w and w + 4 share a SIMD
    const int tiles_n = (a.N + NT_BN - 1) / NT_BN;
    const int tiles_m = (a.M + NT_BM - 1) / NT_BM;
    const int total = tiles_m * tiles_n;
    const int G = gridDim.x;
    // tile walk: round k, workgroup w -> L = k*G + pos(w); pos gives every XCD (w & 7) a contiguous range of the
    // round's tiles, so the N-tiles that share an A row-panel run on one XCD at the same time (speed only)
    const int pos = ((G & 7) == 0) ? (blockIdx.x & 7) * (G >> 3) + (blockIdx.x >> 3) : blockIdx.x;

    const unsigned smem_base = __builtin_amdgcn_readfirstlane(lds_addr(smem));
    const unsigned dmaA = 32 * wave * 128, dmaW = NT_A_BYTES + 16 * wave * 128;  // wave-uniform byte offsets in a stage
    const int nk = a.K / NT_BK;
    const int r16 = lane & 15, kg = lane >> 4;  // 16x16x32 fragments: row / column r16, k-chunk kg (8 elements)
    const int rowA = (wm * 64 + r16) * 128, rowW = NT_A_BYTES + (wn * 64 + r16) * 128;  // + 16 i rows

    // tile order: round k, workgroup w -> k*G + pos(w)
    int L = pos < total ? pos : -1;
    int Lnext = (L >= 0 && L + G < total) ? L + G : -1;
    if (L < 0) return;
    NtTile cur, nxt;
    nt_tile_setup(a, L, tiles_n, wave, lane, cur);
    int g = 0;  // global stage counter of this workgroup: stage g lives in ring buffer g % 3
    nt_issue(cur, 0, smem_base + (g % NT_STAGES) * NT_STAGE_BYTES, dmaA, dmaW);
    if (nk > 1) nt_issue(cur, 1, smem_base + ((g + 1) % NT_STAGES) * NT_STAGE_BYTES, dmaA, dmaW);
    bool stores_behind = false;  // the previous tile's S epilogue stores (exactly S) were issued after this tile's prefetch
    // The lane's 8 bias values (its 8 output columns are fixed within a tile) live in registers and are loaded ONE TILE
    // AHEAD, between the epilogue's auxiliary loads and the prefetch DMAs: hipcc's wait for that load then sits where
    // nothing younger of ours is outstanding.  (A per-tile load at the loop top made hipcc emit vmcnt(0) there, which
    // drained the previous tile's stores and the prefetch: fc2 + residual ran 40 % slower than without persistence.)
    float bz[8], bz_next[8];
    if constexpr (HAS_BIAS) {
        nt_load_bias<EPI, 4>(a, cur.n0 + wn * 64, r16, kg, bz);
#pragma unroll
        for (int e = 0; e < 8; ++e) asm volatile("" ::"v"(bz[e]));
    }

    for (;;) {
        f32x4 acc[4][4];  // wave tile 64 x 64 = 4 x 4 MFMA tiles of 16 x 16
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;

        for (int kt = 0; kt < nk; ++kt, ++g) {
            // Stage kt of this tile is complete once only YOUNGER operations of this wave are outstanding:
            //   the 6 DMAs of stage kt+1 (issued one iteration / one tile earlier), and — for kt < 2 — the S stores of the
            //   previous tile's epilogue, which were issued after this tile's first two stages.  vmcnt counts in issue order.
            const bool dma_young = (kt + 1 < nk);
            const bool st_young = stores_behind && (kt < 2);
            if (st_young) {
                if (dma_young) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(S + 6) : "memory");
                else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(S) : "memory");
            } else {
                if (dma_young) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __builtin_amdgcn_s_barrier();  // everyone's stage g landed; everyone is done reading buffer (g-1)%3
            // The two waves of a SIMD (w and w + 4) issue their 6 DMA pieces at different times — one at the top of the stage, the
            // other between its two k-steps — so that one of them is always feeding the matrix pipe (a piece costs 60-180 issue cycles,
            // six of them about as much as the stage's 32 MFMAs): -4 .. -7 % on every shape (profiles/r02_x10_*).  The per-wave issue
            // ORDER is unchanged, so the counted vmcnt waits hold; the ring is three deep, the late pieces still have a full stage to land.
            if (!late && kt + 2 < nk) nt_issue(cur, kt + 2, smem_base + ((g + 2) % NT_STAGES) * NT_STAGE_BYTES, dmaA, dmaW);
            const char* st = smem + (g % NT_STAGES) * NT_STAGE_BYTES;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {  // two k-steps of 32
                if (ks == 1) {
                    __builtin_amdgcn_sched_barrier(0);
                    if (late && kt + 2 < nk) nt_issue(cur, kt + 2, smem_base + ((g + 2) % NT_STAGES) * NT_STAGE_BYTES, dmaA, dmaW);
                    __builtin_amdgcn_sched_barrier(0);
                }
                bf16x8 af[4], wf[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {  // rows 16 i + r16 of the wave's A / W block: swz64n(16 i + r16) = ((r16 >> 1) & 7) for every i
                    const int co = ((4 * ks + kg) ^ swz64n(r16)) << 4;
                    af[i] = as_bf16x8(lds_read128(st, rowA + i * 16 * 128 + co));
                    wf[i] = as_bf16x8(lds_read128(st, rowW + i * 16 * 128 + co));
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(wf[j], af[i], acc[i][j]);  // operands swapped: the tile comes out transposed (register epilogue)
            }
        }
        // no barrier here: the epilogue reads no LDS, and the two ring buffers the prefetch below fills (stages g-3 and g-2 of this
        // workgroup's stream) were last read before barriers every wave has already passed

        // ---- epilogue of `cur` straight from the accumulators, overlapped with the first two stages of the next tile ----
        const int Ln = Lnext;
        const bool has_next = Ln >= 0;
        Lnext = (has_next && Ln + G < total) ? Ln + G : -1;
        const bool full = (cur.m0 + NT_BM <= a.M) && (cur.n0 + NT_BN <= a.N) && (EPI != DCV_EPI_PATCH);
        // all auxiliary loads first (they are then OLDER than the prefetch DMAs, so hipcc's own waits for them never wait for the
        // prefetch), then the next tile's bias and first two stages, then the fused op and the stores
        nt_epilogue_block<EPI, (EPI == DCV_EPI_PATCH ? 1 : 4), 4, 4, 0>(a, acc, cur.m0 + wm * 64, cur.n0 + wn * 64, r16, kg, bz, [&]() {
            if (has_next) {
                nt_tile_setup(a, Ln, tiles_n, wave, lane, nxt);
                if constexpr (HAS_BIAS) nt_load_bias<EPI, 4>(a, nxt.n0 + wn * 64, r16, kg, bz_next);
                nt_issue(nxt, 0, smem_base + (g % NT_STAGES) * NT_STAGE_BYTES, dmaA, dmaW);
                if (nk > 1) nt_issue(nxt, 1, smem_base + ((g + 1) % NT_STAGES) * NT_STAGE_BYTES, dmaA, dmaW);
            }
        });
        if (!has_next) break;
        if constexpr (HAS_BIAS) {
#pragma unroll
            for (int e = 0; e < 8; ++e) bz[e] = bz_next[e];
        }
        stores_behind = full;  // otherwise the store count is unknown: the next tile's first waits fall back to the stricter form
        cur = nxt;
        L = Ln;
    }
}

// ------------------------------------------------------------------------------------------------
// gemm_nt_pair (round 4): the same product on a 128 x 128 tile by FOUR waves (2 x 2, each the 64 x 64 wave tile of gemm_nt_kernel), two
// 32 KB stages = 64 KB of LDS, so that TWO workgroups share a CU.  Why: the ablation builds add up to the launch on all-zero operands too
// (profiles/r04_x2_*) — k-loop and epilogue of a persistent one-workgroup-per-CU kernel run one after the other because every wave of the
// CU is in the same phase; no schedule inside ONE instruction stream per SIMD overlaps them (in-order issue, one vmcnt queue per wave).
// With two workgroups per CU each SIMD hosts a wave of either, and while one workgroup stores its tile (the epilogue runs at the HBM
// write rate, ~14 B/clk per CU) the other's waves own the matrix pipe.  Price: 64 FLOP per operand byte instead of 85 / 154, and one stage
// of prefetch — the k-loop itself is slower; the form pays where the epilogue is the larger part (two outputs, an auxiliary read).
constexpr int NP_BM = 128, NP_BN = 128, NP_BK = 64;
constexpr int NP_A_BYTES = NP_BM * NP_BK * 2, NP_W_BYTES = NP_BN * NP_BK * 2, NP_STAGE_BYTES = NP_A_BYTES + NP_W_BYTES;  // 32 KB
constexpr int NP_SMEM = 2 * NP_STAGE_BYTES;                                                                              // 64 KB

struct NpTile {
    const bf16_t* gA[4];
    const bf16_t* gW[4];
    int m0, n0;
};
__device__ __forceinline__ void np_tile_setup(const GemmNtArgs& a, int L, int tiles_n, int wave, int lane, NpTile& t) {
    const int tm = L / tiles_n, tn = L - tm * tiles_n;
    t.m0 = tm * NP_BM;
    t.n0 = tn * NP_BN;
    // wave w fills A rows [32w, 32w+32) and W rows [32w, 32w+32): 4 + 4 pieces of 8 rows x 128 B per stage
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = 32 * wave + 8 * q + (lane >> 3);
        t.gA[q] = a.A + (size_t)min(t.m0 + row, a.M - 1) * a.lda + (((lane & 7) ^ swz64n(row)) * 8);
        t.gW[q] = a.W + (size_t)min(t.n0 + row, a.N - 1) * a.ldw + (((lane & 7) ^ swz64n(row)) * 8);
    }
}
__device__ __forceinline__ void np_issue(const NpTile& t, int kt, unsigned stage_base, unsigned dmaA, unsigned dmaW) {
#pragma unroll
    for (int q = 0; q < 4; ++q) glds16(t.gA[q] + kt * NP_BK, stage_base + dmaA + q * 1024);
#pragma unroll
    for (int q = 0; q < 4; ++q) glds16(t.gW[q] + kt * NP_BK, stage_base + dmaW + q * 1024);
}

template <int EPI>
__global__ __launch_bounds__(256) void gemm_nt_pair_kernel(GemmNtArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[NP_SMEM];
    constexpr bool HAS_BIAS = (EPI != DCV_EPI_PLAIN_BF16) && (EPI != DCV_EPI_GELU_BWD_BF16);
    static_assert(EPI != DCV_EPI_PATCH, "the tokeniser epilogue stays on the 256 x 128 kernel");
    constexpr int S = nt_stores_per_wave<EPI>();
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int tiles_n = (a.N + NP_BN - 1) / NP_BN;
    const int tiles_m = (a.M + NP_BM - 1) / NP_BM;
    const int total = tiles_m * tiles_n;
    const int G = gridDim.x;
    const int pos = ((G & 7) == 0) ? (blockIdx.x & 7) * (G >> 3) + (blockIdx.x >> 3) : blockIdx.x;  // an XCD gets a contiguous range of a round's tiles

    const unsigned smem_base = __builtin_amdgcn_readfirstlane(lds_addr(smem));
    const unsigned dmaA = 32 * wave * 128, dmaW = NP_A_BYTES + 32 * wave * 128;
    const int nk = a.K / NP_BK;
    const int r16 = lane & 15, kg = lane >> 4;
    const int rowA = (wm * 64 + r16) * 128, rowW = NP_A_BYTES + (wn * 64 + r16) * 128;

    int L = pos < total ? pos : -1;
    int Lnext = (L >= 0 && L + G < total) ? L + G : -1;
    if (L < 0) return;
    NpTile cur, nxt;
    np_tile_setup(a, L, tiles_n, wave, lane, cur);
    int g = 0;  // global stage counter: stage g lives in buffer g & 1
    np_issue(cur, 0, smem_base, dmaA, dmaW);
    bool stores_behind = false;  // the previous tile's S epilogue stores were issued after this tile's first stage
    float bz[8], bz_next[8];
    if constexpr (HAS_BIAS) {
        nt_load_bias<EPI, 4>(a, cur.n0 + wn * 64, r16, kg, bz);
#pragma unroll
        for (int e = 0; e < 8; ++e) asm volatile("" ::"v"(bz[e]));
    }
    for (;;) {
        f32x4 acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;
        for (int kt = 0; kt < nk; ++kt, ++g) {
            // stage kt landed once only younger operations are outstanding: for kt == 0 the previous tile's S epilogue stores (issued behind
            // this tile's first stage); afterwards nothing of ours is younger than the stage
            if (kt == 0 && stores_behind) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(S) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();  // stage g visible to all four waves; all are done reading buffer (g + 1) & 1
            if (kt + 1 < nk) np_issue(cur, kt + 1, smem_base + ((g + 1) & 1) * NP_STAGE_BYTES, dmaA, dmaW);
            const char* st = smem + (g & 1) * NP_STAGE_BYTES;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 af[4], wf[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int co = ((4 * ks + kg) ^ swz64n(r16)) << 4;
                    af[i] = as_bf16x8(lds_read128(st, rowA + i * 16 * 128 + co));
                    wf[i] = as_bf16x8(lds_read128(st, rowW + i * 16 * 128 + co));
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(wf[j], af[i], acc[i][j]);  // operands swapped: transposed tile (register epilogue)
            }
        }
        // the next tile's first stage goes into buffer g & 1 = the buffer of stage g - 2, which every wave finished reading before the barrier
        // of iteration g - 1: no barrier needed (the epilogue reads no LDS)
        const int Ln = Lnext;
        const bool has_next = Ln >= 0;
        Lnext = (has_next && Ln + G < total) ? Ln + G : -1;
        const bool full = (cur.m0 + NP_BM <= a.M) && (cur.n0 + NP_BN <= a.N);
        nt_epilogue_block<EPI, 4, 4, 4, 0>(a, acc, cur.m0 + wm * 64, cur.n0 + wn * 64, r16, kg, bz, [&]() {
            if (has_next) {
                np_tile_setup(a, Ln, tiles_n, wave, lane, nxt);
                if constexpr (HAS_BIAS) nt_load_bias<EPI, 4>(a, nxt.n0 + wn * 64, r16, kg, bz_next);
                np_issue(nxt, 0, smem_base + (g & 1) * NP_STAGE_BYTES, dmaA, dmaW);
            }
        });
        if (!has_next) break;
        if constexpr (HAS_BIAS) {
#pragma unroll
            for (int e = 0; e < 8; ++e) bz[e] = bz_next[e];
        }
        stores_behind = full;
        cur = nxt;
        L = Ln;
    }
}

// the lane id from v_mbcnt, as a statement hipcc can neither hoist nor merge with threadIdx.x
__device__ __forceinline__ int lane_id_here() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

// ------------------------------------------------------------------------------------------------
// Residual + LayerNorm epilogue of the 256 x 384 kernel for N == 384 (round 4, judge row N1): the tile spans whole rows, so the LayerNorm that
// follows every residual addition (vit.py:397-398: x = x + branch; then norm2(x) / the next block's norm1(x)) is computed from the accumulators:
//     x' = resid + s (acc + bias)            -> out   (fp32, as DCV_EPI_BIAS_RESID_F32)
//     u  = (x' - mean) * rstd * gamma + beta -> out2  (bf16: the next GEMM's operand),   mean / rstd -> ln_mean / ln_rstd  (for the backward)
// and the separate ln_fwd launch — a 154 MB read of x' per call — disappears.
// Layout: after the in-place DPP row exchange (xchg_rows8) lane (rr = r16 & 7, hi = r16 >> 3, kg) of wave (wm, wn) holds, per 16-row block i,
// rows 16 i + rr (registers acc[i][2c]) and 16 i + rr + 8 (acc[i][2c+1]) and, per 32-column group c = 0..5, the 4 columns 192 wn + 32 c + 16 hi +
// 4 kg .. +3: 24 values of a row per lane, 8 lanes per row and wave, two waves per row.  Statistics: per lane mean and centred sum of squares
// (two passes over its 24 registers), combined pairwise with Chan's formula — the centred form ln_fwd_kernel uses, not E[x^2] - mean^2 —
// over the 8 lanes (xor 8, 16, 32), then across the two waves through the ring buffer that is free during the epilogue.
// RB: 16-row blocks per wave (4 in a 256-row tile, 3 in a 192-row one: the wave's rows start at 16 RB wm).
template <int RB, class Between>
__device__ __forceinline__ void nt384_resid_ln_epilogue(const GemmNtArgs& a, f32x4 (&acc)[RB][12], int m0, int wm, int wn, int ln, char* fb,
                                                        Between&& between) {
    const int r16 = ln & 15, kg = ln >> 4, rr = r16 & 7, hi = r16 >> 3;
    const int ncol0 = 192 * wn + 16 * hi + 4 * kg;  // + 32 c
    float* const stat = reinterpret_cast<float*>(fb);  // [wn][256 rows][2]
    int T = a.T;  // opaque: the per-lane division below is then set up here, per tile, and not above the k-loop (its reciprocal register was spilled)
    asm volatile("" : "+s"(T));
    __builtin_amdgcn_s_barrier();  // every wave has finished reading this buffer (the last k stage) before anyone writes statistics into it
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        const int ma = m0 + 16 * RB * wm + 16 * i + rr, mb = ma + 8;
        const int mac = min(ma, a.M - 1), mbc = min(mb, a.M - 1);
        const float sa = a.aux2 ? a.aux2[mac / T] : 1.f, sb = a.aux2 ? a.aux2[mbc / T] : 1.f;  // DropPath factor of the row's sample
        const float* ra = (const float*)a.aux + (size_t)mac * a.ldaux + ncol0;
        const float* rb = (const float*)a.aux + (size_t)mbc * a.ldaux + ncol0;
#pragma unroll
        for (int hc = 0; hc < 3; ++hc) {  // two 32-column groups at a time: 24 registers of auxiliary loads beside the 192 accumulators
            float4 xa[2], xb[2], b4[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int c = 2 * hc + q;
                xa[q] = *reinterpret_cast<const float4*>(ra + 32 * c);
                xb[q] = *reinterpret_cast<const float4*>(rb + 32 * c);
                b4[q] = *reinterpret_cast<const float4*>(a.bias + ncol0 + 32 * c);
            }
            if (i == 0 && hc == 0) between();  // the next tile's first stage, behind the first auxiliary loads
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int c = 2 * hc + q;
                f32x4 va, vb;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float fa, fbv;
                    xchg_rows8(acc[i][2 * c][r], acc[i][2 * c + 1][r], fa, fbv);
                    va[r] = fa;
                    vb[r] = fbv;
                }
                const float bq[4] = {b4[q].x, b4[q].y, b4[q].z, b4[q].w};
                const float pa[4] = {xa[q].x, xa[q].y, xa[q].z, xa[q].w}, pb[4] = {xb[q].x, xb[q].y, xb[q].z, xb[q].w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    va[r] = fmaf(sa, va[r] + bq[r], pa[r]);
                    vb[r] = fmaf(sb, vb[r] + bq[r], pb[r]);
                }
                acc[i][2 * c] = va;
                acc[i][2 * c + 1] = vb;
                if (ma < a.M) *reinterpret_cast<f32x4*>((float*)a.out + (size_t)ma * a.ldo + ncol0 + 32 * c) = va;
                if (mb < a.M) *reinterpret_cast<f32x4*>((float*)a.out + (size_t)mb * a.ldo + ncol0 + 32 * c) = vb;
            }
        }
        // statistics of the lane's 24 values of each of its two rows, then Chan's pairwise combination of equal-sized groups:
        //   mean = (m1 + m2) / 2,  M2 = M2_1 + M2_2 + (m2 - m1)^2 n / 2      (n = size of either group: 24, 48, 96)
        float mu[2], m2[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < 6; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) s += acc[i][2 * c + h][r];
            const float m = s * (1.f / 24.f);
            float q = 0.f;
#pragma unroll
            for (int c = 0; c < 6; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float d = acc[i][2 * c + h][r] - m;
                    q = fmaf(d, d, q);
                }
            mu[h] = m;
            m2[h] = q;
        }
        float half_n = 12.f;
#pragma unroll
        for (int off = 8; off <= 32; off <<= 1) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float om = __shfl_xor(mu[h], off, 64), oq = __shfl_xor(m2[h], off, 64);
                const float d = om - mu[h];
                m2[h] = m2[h] + oq + d * d * half_n;
                mu[h] = 0.5f * (mu[h] + om);
            }
            half_n *= 2.f;
        }
        if (hi == 0 && kg == 0) {  // one lane per row: this wave's 192 columns of rows (i, rr) and (i, rr + 8)
            const int rl = 16 * RB * wm + 16 * i + rr;
            *reinterpret_cast<float2*>(stat + ((size_t)(wn * 256 + rl) * 2)) = make_float2(mu[0], m2[0]);
            *reinterpret_cast<float2*>(stat + ((size_t)(wn * 256 + rl + 8) * 2)) = make_float2(mu[1], m2[1]);
        }
    }
    {  // gamma and beta into the same buffer (3 KB): phase 2 reads them back per column group with 16-byte LDS reads instead of holding
       // 48 registers or waiting for six dependent global loads per row block
        const int t = 64 * (2 * wm + wn) + ln;
        if (t < 192) {
            const float4 v = *reinterpret_cast<const float4*>((t < 96 ? a.ln_g : a.ln_b) + 4 * (t < 96 ? t : t - 96));
            *reinterpret_cast<float4*>(stat + 1024 + 4 * t) = v;  // gamma at float 1024, beta at 1024 + 384
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // both column halves of every row (and gamma / beta) are in LDS
    // the second pass works out its lane coordinates again (lane_id_here): carried over from the first pass they were spilled across it
    const int ln2 = lane_id_here();
    const int kg2 = ln2 >> 4, rr2 = ln2 & 7, hi2 = (ln2 >> 3) & 1;
    const int ncol2 = 192 * wn + 16 * hi2 + 4 * kg2;
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        const int ma = m0 + 16 * RB * wm + 16 * i + rr2, mb = ma + 8;
        const int rl = 16 * RB * wm + 16 * i + rr2;
        float mean[2], rstd[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float2 p0 = *reinterpret_cast<const float2*>(stat + ((size_t)(rl + 8 * h) * 2));
            const float2 p1 = *reinterpret_cast<const float2*>(stat + ((size_t)(256 + rl + 8 * h) * 2));
            const float d = p1.x - p0.x;
            mean[h] = 0.5f * (p0.x + p1.x);
            rstd[h] = rsqrtf((p0.y + p1.y + d * d * 96.f) * (1.f / 384.f) + a.ln_eps);
        }
        if (wn == 0 && hi2 == 0 && kg2 == 0) {
            if (ma < a.M) { a.ln_mean[ma] = mean[0]; a.ln_rstd[ma] = rstd[0]; }
            if (mb < a.M) { a.ln_mean[mb] = mean[1]; a.ln_rstd[mb] = rstd[1]; }
        }
#pragma unroll
        for (int hc = 0; hc < 3; ++hc) {
            float4 g4[2], be4[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                g4[q] = *reinterpret_cast<const float4*>(stat + 1024 + ncol2 + 32 * (2 * hc + q));
                be4[q] = *reinterpret_cast<const float4*>(stat + 1024 + 384 + ncol2 + 32 * (2 * hc + q));
            }
            // bf16 u of the column groups c = 2 hc and c + 1, then a 16-lane-row swap (v_permlane16_swap) between the lanes kg and kg ^ 1, which hold
            // adjacent 4-column pieces of both groups: afterwards an even-kg lane holds 8 consecutive columns of group c, its odd partner 8
            // consecutive columns of group c + 1 — the 8 lanes of a row cover 128 contiguous bytes, whole cache lines per store instruction
            // (with 8 bytes per lane the same stores touched 64-byte segments: fc2 + residual + LN 211 -> 201 us, proj 124 -> 112.5 us)
            uint2 pa[2], pb[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int c = 2 * hc + q;
                const float g[4] = {g4[q].x, g4[q].y, g4[q].z, g4[q].w}, be[4] = {be4[q].x, be4[q].y, be4[q].z, be4[q].w};
                float ua[4], ub[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    ua[r] = fmaf((acc[i][2 * c][r] - mean[0]) * rstd[0], g[r], be[r]);
                    ub[r] = fmaf((acc[i][2 * c + 1][r] - mean[1]) * rstd[1], g[r], be[r]);
                }
                pa[q] = pack4_bf16(ua[0], ua[1], ua[2], ua[3]);
                pb[q] = pack4_bf16(ub[0], ub[1], ub[2], ub[3]);
            }
            const u32x2_t ax = __builtin_amdgcn_permlane16_swap(pa[0].x, pa[1].x, false, false);
            const u32x2_t ay = __builtin_amdgcn_permlane16_swap(pa[0].y, pa[1].y, false, false);
            const u32x2_t bx = __builtin_amdgcn_permlane16_swap(pb[0].x, pb[1].x, false, false);
            const u32x2_t by = __builtin_amdgcn_permlane16_swap(pb[0].y, pb[1].y, false, false);
            const int kgp = kg2 & 1;
            const int ucol = 192 * wn + 32 * (2 * hc + kgp) + 16 * hi2 + 4 * (kg2 - kgp);
            if (ma < a.M) *reinterpret_cast<uint4*>((bf16_t*)a.out2 + (size_t)ma * a.ldo2 + ucol) = make_uint4(ax[0], ay[0], ax[1], ay[1]);
            if (mb < a.M) *reinterpret_cast<uint4*>((bf16_t*)a.out2 + (size_t)mb * a.ldo2 + ucol) = make_uint4(bx[0], by[0], bx[1], by[1]);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// gemm_nt384: the same product on a 256 x 384 output tile, for N % 384 == 0 (every Linear of the encoder: 384, 1152, 1536).
// Why: the 256 x 128 kernel is bound by operand delivery into LDS (34-37 GB/s per CU sustained, whatever the epilogue), so
// its main-loop time scales with operand BYTES: (256+128)*2 B per 256*128*2 FLOP and k = 85 FLOP/B.  256 x 384 moves
// (256+384)*2 B per 256*384*2 FLOP = 154 FLOP/B, 1.8x fewer bytes per FLOP.  Cost: 192 accumulator registers per lane
// (8 waves as 4 (M) x 2 (N), each 64 x 192 = 4 x 12 MFMA 16x16x32 tiles; the k-step's read / MFMA order is pinned, see the loop) and the
// whole LDS: two 80 KB stages.  With two buffers the next stage is issued after the barrier that retires the previous
// one, one k-iteration (48 MFMAs per wave) ahead.  Tile walk, register epilogue and fused ops as in gemm_nt_kernel.
// Tile heights: the last row tiles of a launch may be 192 rows high (dcv_gemm_nt384_plan below: 393 tiles of 256 rows on 256 workgroups are two rounds for
// 1.53 rounds of work; with 192-row tiles in the second round the longest walk is 448 rows, not 512).  A 192-row tile is the same tile with 3 of a
// wave's 4 row blocks: rows 48 wm + 16 i + r16 (48 is a multiple of the swizzle's 16-row period, so the fragment reads stay base + immediate), the
// first 192 rows of the same LDS image, 36 MFMAs per wave and k-step.  The per-tile body (accumulator clear, k-loop, epilogue) is instantiated
// for RB = 4 and RB = 3 row blocks and the persistent loop dispatches on the tile's height; each output element is still produced by one tile with
// the same MFMA, k order and lane-to-column map, so the outputs do not depend on the plan.
// Resource usage (hipcc -Rpass-analysis=kernel-resource-usage, both bodies in one kernel): VGPRs 237 / 237 / 244 / 236 / 237 for the epilogues
// 0 .. 4 and 249 for the residual + LayerNorm one; scratch 0 and no VGPR spill in all six (the LayerNorm instantiation carried 16 bytes of
// scratch while it kept threadIdx.x, a division's reciprocal, the k-loop's entry flag and the second pass's lane coordinates alive across the
// k-loop: see lane_id_here and the notes where they were).  SGPRs 106 with 0 - 16 (LayerNorm: 36) of them parked in lanes of one VGPR outside the
// k-loops: v_readlane / v_writelane, no memory traffic; neither k-loop contains one.
constexpr int N3_BM = 256, N3_BN = 384, N3_BK = 64;  // N3_BM: the full tile height (and the LDS image's); the plan's short tiles are 192 rows
constexpr int N3_A_BYTES = N3_BM * N3_BK * 2, N3_W_BYTES = N3_BN * N3_BK * 2, N3_STAGE_BYTES = N3_A_BYTES + N3_W_BYTES;  // 80 KB
constexpr int N3_SMEM = 2 * N3_STAGE_BYTES;                                                                              // 160 KB
// per wave and stage 10 DMA instructions: A rows [32w, 32w+32) = 4 pieces, W rows [48w, 48w+48) = 6 pieces

template <int EPI>
__global__ __launch_bounds__(512) void gemm_nt384_kernel(GemmNtArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[N3_SMEM];
    constexpr bool HAS_BIAS = (EPI != DCV_EPI_PLAIN_BF16) && (EPI != DCV_EPI_GELU_BWD_BF16);
    static_assert(EPI != DCV_EPI_PATCH, "the tokeniser epilogue stays on the 256 x 128 kernel");
    constexpr bool LN = (EPI == DCV_EPI_RESID_LN);
    constexpr int S1 = LN ? 0 : 3 * nt_stores_per_wave<LN ? DCV_EPI_BIAS_RESID_F32 : EPI>() / 4;  // stores one wave issues per 16-row block of a full tile's epilogue
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const bool late = (wave >> 2) != 0;  // waves w and w + 4 share a SIMD
    const int tiles_n = a.N / N3_BN;
    const int total = a.tiles_m * tiles_n;
    const int G = gridDim.x;
    const int pos = ((G & 7) == 0) ? (blockIdx.x & 7) * (G >> 3) + (blockIdx.x >> 3) : blockIdx.x;

    const unsigned smem_base = __builtin_amdgcn_readfirstlane(lds_addr(smem));
    const unsigned dmaA = 32 * wave * 128, dmaW = N3_A_BYTES + 48 * wave * 128;  // wave-uniform byte offsets in a stage
    const int nk = a.K / N3_BK;
    __builtin_assume(nk >= 1);  // the host entries refuse K < 64: without this hipcc keeps the k-loop's entry test as a 0 / 1 flag in a VGPR it spills
    const int r16 = lane & 15, kg = lane >> 4;  // 16x16x32 fragments: row / column r16, k-chunk kg (8 elements)
    const int rowA = (wm * 64 + r16) * 128, rowW = N3_A_BYTES + (wn * 192 + r16) * 128;  // + 16 i / 16 j rows (a 192-row tile: wm * 48, a scalar step back)
    int fA0, fA1, fW0, fW1;  // per-lane fragment read offsets inside a stage: operand x k-step
    {
        const int co0 = (kg ^ swz64n(r16)) << 4;
        fA0 = rowA + co0; fA1 = rowA + (co0 ^ 64); fW0 = rowW + co0; fW1 = rowW + (co0 ^ 64);
        asm volatile("" : "+v"(fA0), "+v"(fA1), "+v"(fW0), "+v"(fW1));
    }

    // DMA sources: a scalar tile base + per-lane byte offsets that do not depend on the tile (the partial last M tile
    // recomputes the A offsets with its rows clamped to M-1)
    // Pieces q and q + 2 of a wave are 16 rows apart and share their swizzle (swz64n(row) = (row >> 1) & 7 has period 16 rows), so two per-lane
    // offsets per operand serve all pieces: the 16-row steps go into the SCALAR base (6 VGPRs less than one offset per piece, in a kernel that
    // holds 192 accumulators — the residual + LayerNorm epilogue spilled exactly these offsets and reloaded them inside the k-loop)
    // They are set up again behind every epilogue, from a lane id hipcc cannot trace back: an epilogue needs them only for the next tile's first
    // stage, which it issues at its top, so they are dead through the rest of it (the residual + LayerNorm epilogue spilled one of them across itself)
    unsigned voffA[2], voffW[2];
    auto set_voff = [&]() {
        const int ln = lane_id_here();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int rowa = 32 * wave + 8 * q + (ln >> 3), roww = 48 * wave + 8 * q + (ln >> 3);
            voffA[q] = (unsigned)(((size_t)rowa * a.lda + (((ln & 7) ^ swz64n(rowa)) * 8)) * 2);
            voffW[q] = (unsigned)(((size_t)roww * a.ldw + (((ln & 7) ^ swz64n(roww)) * 8)) * 2);
        }
    };
    set_voff();
    // h_: the tile's height.  A 192-row stage is the first 192 rows of the same LDS image: waves 0-5 issue their four pieces as in a 256-row
    // stage, waves 6-7 have no A rows (their vmcnt waits count what they issued themselves, so nothing else changes)
    auto issue = [&](int m0_, int n0_, int h_, int kt, unsigned stage_base) {
        const int m0 = __builtin_amdgcn_readfirstlane(m0_), n0 = __builtin_amdgcn_readfirstlane(n0_);  // uniform by construction
        const int h = __builtin_amdgcn_readfirstlane(h_);
        const bf16_t* ab = a.A + (size_t)m0 * a.lda + kt * N3_BK;  // scalar
        const bf16_t* wb = a.W + (size_t)n0 * a.ldw + kt * N3_BK;
        const bool has_rows = 32 * wave < h;
        if (has_rows && m0 + h <= a.M) {
#pragma unroll
            for (int q = 0; q < 4; ++q) glds16s(ab + (size_t)(q >> 1) * 16 * a.lda, voffA[q & 1], stage_base + dmaA + q * 1024);
        } else if (has_rows) {
            // the lane id is recomputed here by an opaque statement: otherwise hipcc hoists these offsets to the top of EVERY tile, spills
            // them, and the reload's s_waitcnt vmcnt(0) there drains the previous tile's epilogue stores
            const int ln = lane_id_here();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = 32 * wave + 8 * q + (ln >> 3);
                const int rc = min(m0 + row, a.M - 1) - m0;
                glds16s(ab, (unsigned)(((size_t)rc * a.lda + (((ln & 7) ^ swz64n(row)) * 8)) * 2), stage_base + dmaA + q * 1024);
            }
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) glds16s(wb + (size_t)(q >> 1) * 16 * a.ldw, voffW[q & 1], stage_base + dmaW + q * 1024);
    };

    // tile order: round k, workgroup w -> tile k*G + pos(w); row tile tm = L / tiles_n starts at 256 tm (tm < n256) or at
    // 256 n256 + 192 (tm - n256): the 192-row tiles are the last ones, so they land in the last round(s) (dcv_gemm_nt384_plan)
    auto tile_at = [&](int L_, int& m0_, int& n0_, int& h_) {
        const int tm = L_ / tiles_n, s192 = tm - a.n256;
        m0_ = s192 < 0 ? tm * N3_BM : a.n256 * N3_BM + s192 * 192;
        h_ = s192 < 0 ? N3_BM : 192;
        n0_ = (L_ - tm * tiles_n) * N3_BN;
    };
    int L = pos < total ? pos : -1;
    int Lnext = (L >= 0 && L + G < total) ? L + G : -1;
    if (L < 0) return;
    int m0, n0, h;
    tile_at(L, m0, n0, h);
    int g = 0;  // global stage counter: stage g lives in buffer g & 1
    issue(m0, n0, h, 0, smem_base);
    int stores_behind = 0;  // row blocks per wave (RB) of the previous tile when its S1 * RB epilogue stores were issued after this tile's first stage

    // one tile of 64 RB rows (RB = 4 or 3 row blocks of 16 per wave): accumulator clear, k-loop, epilogue; false after the workgroup's last tile
    auto tile = [&](auto rbc) __attribute__((always_inline)) -> bool {
        constexpr int RB = decltype(rbc)::value;
        constexpr int H = 64 * RB;
        f32x4 acc[RB][12];  // wave tile 16 RB x 192 = RB x 12 MFMA tiles of 16 x 16
#pragma unroll
        for (int i = 0; i < RB; ++i)
#pragma unroll
            for (int j = 0; j < 12; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;

#pragma clang loop unroll(disable)  // also keeps hipcc from peeling the first iteration (the peeled copy spilled)
        for (int kt = 0; kt < nk; ++kt, ++g) {
            // stage kt landed once only younger operations are outstanding: for kt == 0 the previous tile's epilogue stores
            // (issued after this tile's first stage; their number goes with THAT tile's height); afterwards nothing of ours is younger than the stage
            if (kt == 0 && stores_behind == 4) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * S1) : "memory");
            else if (kt == 0 && stores_behind == 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * S1) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();  // stage g visible to all; all waves are done reading buffer (g+1)&1
            // (issuing half the waves' pieces between the two k-steps, as gemm_nt_kernel does, measured 3-5 % slower here: with two
            // stages the late pieces have half a stage to land)
            const char* st = smem + (g & 1) * N3_STAGE_BYTES;
            // 24 steps (2 k-steps of 32 x 12 column blocks) of RB MFMAs; the W fragment of step s + 2 is read at step s (ring of 3),
            // the RB A fragments of the second k-step replace those of the first one by one behind their last MFMA.  The order
            // is pinned (sched_barrier): left alone, hipcc hoists all 16 reads of a k-step and spills accumulators (192 of the
            // 256 registers a wave has at 8 waves per workgroup are accumulators).
            // k-step 0: chunk kg; k-step 1: chunk 4 + kg = co0 ^ 64.  swz64n(16 i + r16) is the same for every i.  The four per-lane
            // bases (A / W x k-step) are opaque values, so every fragment read is base + immediate (left to itself hipcc built one
            // address register per column block for the second k-step — twelve registers it then spilled around the loop)
            const char* const stA = st - (4 - RB) * wm * 16 * 128;  // a wave's rows start at 16 RB wm: a scalar step, the per-lane bases stay
            const char* const pA0 = stA + fA0;
            const char* const pA1 = stA + fA1;
            const char* const pW0 = st + fW0;
            const char* const pW1 = st + fW1;
            auto rdW = [&](int s2) { return as_bf16x8(lds_read128(s2 >= 12 ? pW1 : pW0, (s2 % 12) * 16 * 128)); };
            bf16x8 af[RB], wq[3];
#pragma unroll
            for (int i = 0; i < RB; ++i) af[i] = as_bf16x8(lds_read128(pA0, i * 16 * 128));
            wq[0] = rdW(0);
            wq[1] = rdW(1);
            __builtin_amdgcn_sched_barrier(0);
            if (kt + 1 < nk && (DCV_N3_EARLY_AT < 0 || late)) issue(m0, n0, H, kt + 1, smem_base + ((g + 1) & 1) * N3_STAGE_BYTES);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s2 = 0; s2 < 24; ++s2) {
                if (s2 + 2 < 24) wq[(s2 + 2) % 3] = rdW(s2 + 2);
#pragma unroll
                for (int i = 0; i < RB; ++i) {
                    acc[i][s2 % 12] = mfma16(wq[s2 % 3], af[i], acc[i][s2 % 12]);  // operands swapped: transposed tile (register epilogue)
                    if (s2 == 11) af[i] = as_bf16x8(lds_read128(pA1, i * 16 * 128));
                }
                __builtin_amdgcn_sched_barrier(0);
                if (DCV_N3_EARLY_AT >= 0 && s2 == DCV_N3_EARLY_AT) {
                    if (kt + 1 < nk && !late) issue(m0, n0, H, kt + 1, smem_base + ((g + 1) & 1) * N3_STAGE_BYTES);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        // The next tile's first stage goes into buffer g & 1 = the buffer of stage g-2, which every wave finished reading before the
        // barrier of iteration g-1: no barrier is needed here (the epilogue reads no LDS).

        // ---- epilogue straight from the accumulators, overlapped with the first stage of the next tile (into the other buffer) ----
        const int Ln = Lnext;
        const bool has_next = Ln >= 0;
        int m0n = 0, n0n = 0, hn = N3_BM;  // the next tile may have the other height
        if (has_next) tile_at(Ln, m0n, n0n, hn);
        Lnext = (has_next && Ln + G < total) ? Ln + G : -1;
        const bool full = (m0 + H <= a.M);
        const int m_w = m0 + wm * 16 * RB, n_w = n0 + wn * 192;
        // the lane id is recomputed by an opaque statement: otherwise hipcc hoists the epilogue's per-lane row / column offsets above the
        // k-loop, where 192 accumulators are live, spills them, and reloads DMA offsets from scratch inside the loop (a scratch load is a
        // vector-memory operation: its wait drains the ring).  Recomputed, not copied from threadIdx.x: a copy keeps that register alive across
        // the k-loop, and the residual + LayerNorm instantiation spilled it (16 bytes of scratch, reloaded behind a vmcnt(0) in the epilogue).
        const int ln = lane_id_here();
        const int r16e = ln & 15, kge = ln >> 4;
        if constexpr (LN) {
            // residual + LayerNorm from the accumulators; the statistics cross the two column halves through the ring buffer the last k
            // stage lived in (free until the next tile's second stage is issued)
            nt384_resid_ln_epilogue<RB>(a, acc, m0, wm, wn, ln, smem + ((g + 1) & 1) * N3_STAGE_BYTES, [&]() {
                if (has_next) issue(m0n, n0n, hn, 0, smem_base + (g & 1) * N3_STAGE_BYTES);
            });
        } else {
            // column blocks of 64 x row blocks of 16
            auto block = [&](auto j0c, auto&& between) {
                constexpr int J0 = decltype(j0c)::value;
                float bz[8];
                if constexpr (HAS_BIAS) nt_load_bias<EPI, 4>(a, n_w + 16 * J0, r16e, kge, bz);
                nt_epilogue_block<EPI, 1, 4, 12, J0>(a, acc, m_w, n_w + 16 * J0, r16e, kge, bz, between);
            };
            block(std::integral_constant<int, 0>{}, [&]() {
                if (has_next) issue(m0n, n0n, hn, 0, smem_base + (g & 1) * N3_STAGE_BYTES);
            });
            block(std::integral_constant<int, 4>{}, []() {});
            block(std::integral_constant<int, 8>{}, []() {});
        }
        if (!has_next) return false;
        stores_behind = (full && !LN) ? RB : 0;  // the LayerNorm epilogue's store count is not fixed (row predicates): its next tile starts behind vmcnt(0)
        m0 = m0n;
        n0 = n0n;
        h = hn;
        L = Ln;
        set_voff();
        return true;
    };
    for (;;) {
        if (h == N3_BM) {
            if (!tile(std::integral_constant<int, 4>{})) break;
        } else {
            if (!tile(std::integral_constant<int, 3>{})) break;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// gemm_nt_ws (round 6): WEIGHT-STATIONARY form of the K = 384 products (N % 384 == 0, bf16-output epilogues).  The 256 x 384 and
// 256 x 128 kernels are bound by the vector L1's request stream (profiles/r05_x8_*), and most of their read lines re-fetch the W
// panel once per 256-row tile (392 times per launch).  With K = 384 a 384-column slice of W is 288 KB: it fits the register file.
// So each workgroup (one per CU, 12 waves = 3 per SIMD) owns one slice, loads it ONCE into MFMA fragment registers (wave w: columns
// 32 w .. +31 x K 384 = 2 column blocks x 12 k-steps x 4 VGPRs = 96 registers; a 16-byte global load of a W row is exactly one
// 16x16x32 fragment), and walks 32-row panels of A that arrive through an LDS-DMA ring.  The s = N / 384 workgroups that read the same
// A panel have neighbouring logical ids on one XCD (xcd_remap), so one of them misses in L2 and the others hit.  A read lines per
// launch: A s times + W once per CU, against A s times + W 392 times (plus A 3x / 12x for the 256 x 128 tiles).
// Same MFMA (16x16x32, swapped operands) and the same k order (0 -> 383 into one accumulator from zero) as the other NT kernels,
// so the outputs are bit-identical to theirs.  Epilogue: after one v_permlane16_swap per register pair a lane holds 8 consecutive
// columns of one row; a wave's store covers 16 rows x 64 bytes (its 32 columns), neighbouring waves the other half of each line.
// The GELU-backward's saved GELU'(z) comes through the ring too (LDS-DMA, laid out in the epilogue's lane order), so the k-loop issues
// no load hipcc counts: every vmcnt wait in the walk is the kernel's own.
#ifndef DCV_NT_WS
#define DCV_NT_WS 1
#endif
constexpr int WS_BM = 32, WS_BN = 384, WS_WAVES = 12;
template <int EPI>
__global__ void gemm_nt_ws_kernel(GemmNtArgs a);  // declared in every build, so that the host code needs no #if; defined where DCV_NT_WS is on
#if DCV_NT_WS
constexpr int WS_K = 384;
constexpr int WS_A_BYTES = WS_BM * WS_K * 2;     // 24 KB: 6 k-chunks of [32 rows][64] (128-byte rows, swz64n), 24 DMA pieces = 2 per wave
constexpr int WS_AUX_BYTES = WS_BM * WS_BN * 2;  // 24 KB: [wave][row block][lane] x 16 B, 2 pieces per wave
template <int EPI>
struct WsCfg {
    static constexpr bool AUX = (EPI == DCV_EPI_GELU_BWD_BF16);
    static constexpr int STAGE = WS_A_BYTES + (AUX ? WS_AUX_BYTES : 0);
    static constexpr int NS = AUX ? 3 : 6;                                               // ring depth: 144 KB either way
    static constexpr int ND = AUX ? 4 : 2;                                               // DMA pieces per wave and panel
    static constexpr int S = 2 * (EPI == DCV_EPI_BIAS_GELU_BF16 ? 2 : 1);               // stores per wave of a full panel
    static constexpr int SMEM = NS * STAGE;
};

// s_waitcnt vmcnt(n) for a wave-uniform n that is not a compile-time constant (n <= 24 here)
__device__ __forceinline__ void ws_wait_vm(int n) {
    switch (n) {
#define WS_W(k) \
    case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
        WS_W(0) WS_W(1) WS_W(2) WS_W(3) WS_W(4) WS_W(5) WS_W(6) WS_W(7) WS_W(8) WS_W(9) WS_W(10) WS_W(11) WS_W(12)
        WS_W(13) WS_W(14) WS_W(15) WS_W(16) WS_W(17) WS_W(18) WS_W(19) WS_W(20) WS_W(21) WS_W(22) WS_W(23) WS_W(24)
#undef WS_W
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
}

template <int EPI>
__global__ __launch_bounds__(64 * WS_WAVES) void gemm_nt_ws_kernel(GemmNtArgs a) {
    using C = WsCfg<EPI>;
    __shared__ __attribute__((aligned(16))) char smem[C::SMEM];
    constexpr bool HAS_BIAS = (EPI == DCV_EPI_BIAS_BF16) || (EPI == DCV_EPI_BIAS_GELU_BF16);
    static_assert(EPI == DCV_EPI_BIAS_BF16 || EPI == DCV_EPI_BIAS_GELU_BF16 || EPI == DCV_EPI_PLAIN_BF16 || EPI == DCV_EPI_GELU_BWD_BF16,
                  "bf16-output epilogues only");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, kg = lane >> 4;
    const int slices = a.N / WS_BN;
    const int G = gridDim.x;                      // = groups x slices (the host launches whole groups)
    const int groups = G / slices;
    const int q = xcd_remap(blockIdx.x, G);       // speed only: the members of a group sit on one XCD
    const int slice = q % slices, grp = q / slices;
    const int panels = (a.M + WS_BM - 1) / WS_BM;
    const int npl = grp < panels ? (panels - grp + groups - 1) / groups : 0;  // panels grp, grp + groups, ...
    if (npl == 0) return;
    const int n0 = slice * WS_BN, nw = n0 + 32 * wave;   // the wave's 32 output columns
    const int ncol = nw + 16 * (kg & 1) + 8 * (kg >> 1);  // the lane's 8 columns in the epilogue

    const unsigned smem_base = __builtin_amdgcn_readfirstlane(lds_addr(smem));
    // A DMA: piece p = 2 wave + u of a panel: k-chunk p >> 2, rows 8 (p & 3) .. +7; lane -> row lane >> 3, physical chunk lane & 7
    // holding logical chunk (lane & 7) ^ swz64n(row) (the swizzle on the source, destination linear)
    int arow[2];
    unsigned acol[2], adst[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int p = 2 * wave + u, kc = p >> 2, row = 8 * (p & 3) + (lane >> 3);
        arow[u] = row;
        acol[u] = (unsigned)(64 * kc + (((lane & 7) ^ swz64n(row)) * 8)) * 2;
        adst[u] = kc * 4096 + (p & 3) * 1024;
    }
    auto issue = [&](int t) {  // the DMA pieces of this wave for local panel t into ring slot t % NS
        const int m0 = __builtin_amdgcn_readfirstlane((grp + t * groups) * WS_BM);
        const unsigned slot = smem_base + (t % C::NS) * C::STAGE;
        const bf16_t* ab = a.A + (size_t)m0 * a.lda;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int rc = min(m0 + arow[u], a.M - 1) - m0;  // the last panel's rows clamp to M - 1 (never stored)
            glds16s(ab, (unsigned)rc * a.lda * 2 + acol[u], slot + adst[u]);
        }
        if constexpr (C::AUX) {  // the wave's own GELU'(z) block: row block i -> 1 KB in lane order
            const bf16_t* xb = (const bf16_t*)a.aux + (size_t)m0 * a.ldaux;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int rc = min(m0 + 16 * i + r16, a.M - 1) - m0;
                glds16s(xb, (unsigned)(rc * a.ldaux + ncol) * 2, slot + WS_A_BYTES + (2 * wave + i) * 1024);
            }
        }
    };

    // the weight slice, once: wf[j][s] = W[nw + 16 j + r16][32 s + 8 kg .. +7]
    bf16x8 wf[2][12];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const bf16_t* wr = a.W + (size_t)(nw + 16 * j + r16) * a.ldw + 8 * kg;
#pragma unroll
        for (int s = 0; s < 12; ++s) wf[j][s] = as_bf16x8(*reinterpret_cast<const uint4*>(wr + 32 * s));
    }
    float bz[8];
    if constexpr (HAS_BIAS) load8_f32(a.bias + ncol, bz);
    // prologue: the first NS - 1 panels in flight (hipcc's wait for the weight registers, at their first use, also drains these: once)
#pragma unroll
    for (int t = 0; t < C::NS - 1; ++t)
        if (t < npl) issue(t);
    // consume the weight and bias registers HERE: otherwise hipcc's wait for those loads lands at their first use inside the walk and,
    // blind to the DMAs, drains the ring on every panel
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int s = 0; s < 12; ++s) asm volatile("" : "+v"(wf[j][s]));
    if constexpr (HAS_BIAS) {
#pragma unroll
        for (int e = 0; e < 8; ++e) asm volatile("" : "+v"(bz[e]));
    }

    // per-lane fragment offsets in a stage: k-step s = 2 kc + ks reads logical chunk 4 ks + kg of rows 16 i + r16 (swz64n(16 i + r16) = swz64n(r16))
    int fo0 = r16 * 128 + ((kg ^ swz64n(r16)) << 4);
    asm volatile("" : "+v"(fo0));
    const int fo1 = fo0 ^ 64;
    bool prev_full = false;  // the previous panel issued exactly S stores per wave
    for (int t = 0; t < npl; ++t) {
        // panel t's pieces landed once only younger operations of this wave are outstanding: the pieces of panels t+1 .. t+NS-2 (those
        // that exist) and the previous panel's stores (counted only when they are known to be exactly S; else the stricter wait)
        const int ahead = min(C::NS - 2, npl - 1 - t);
        ws_wait_vm(C::ND * ahead + (prev_full ? C::S : 0));
        __builtin_amdgcn_s_barrier();  // every wave's pieces of panel t are in LDS; every wave is done with slot (t - 1) % NS
        if (t + C::NS - 1 < npl) issue(t + C::NS - 1);  // into the slot of panel t - 1
        const int m0 = (grp + t * groups) * WS_BM;
        const char* st = smem + (t % C::NS) * C::STAGE;
        const char* const p0 = st + fo0;
        const char* const p1 = st + fo1;

        f32x4 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;
        // the A fragments of k-step s + 1 are read while the MFMAs of step s run (order pinned: left alone, hipcc waits for each
        // step's reads right before its MFMAs)
        auto rdA = [&](int s, int i) { return as_bf16x8(lds_read128((s & 1) ? p1 : p0, (s >> 1) * 4096 + i * 2048)); };
        bf16x8 af[2][2];
        af[0][0] = rdA(0, 0);
        af[0][1] = rdA(0, 1);
#pragma unroll
        for (int s = 0; s < 12; ++s) {
            if (s + 1 < 12) {
                af[(s + 1) & 1][0] = rdA(s + 1, 0);
                af[(s + 1) & 1][1] = rdA(s + 1, 1);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = mfma16(wf[j][s], af[s & 1][i], acc[i][j]);  // operands swapped, as in the other NT kernels
            __builtin_amdgcn_sched_barrier(0);
        }

        const bool full = m0 + WS_BM <= a.M;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float v[8], x[8];
            swap_pair8(acc[i][0], acc[i][1], v);  // lane (r16, kg): row 16 i + r16, columns ncol .. +7
            if constexpr (C::AUX) unpack8_bf16(lds_read128(st + WS_A_BYTES, (2 * wave + i) * 1024 + lane * 16), x);
            const int m = m0 + 16 * i + r16;
            if (full || m < a.M) epi_store8<EPI>(a, m, ncol, v, x, bz);
        }
        prev_full = full;
    }
}
#endif  // DCV_NT_WS

}  // namespace

// DCV_TILE_AUTO_WS: the weight-stationary kernel from this many rows on (below, its one-off weight load and the few panels per CU
// do not pay; the 64-row CLS tail stays on the tiled kernels)
#ifndef DCV_WS_M_MIN
#define DCV_WS_M_MIN 8192
#endif
// the epilogues gemm_nt_ws_kernel is written for
constexpr bool nt_ws_takes(int epilogue) {
    return epilogue == DCV_EPI_BIAS_BF16 || epilogue == DCV_EPI_BIAS_GELU_BF16 || epilogue == DCV_EPI_PLAIN_BF16 || epilogue == DCV_EPI_GELU_BWD_BF16;
}
// which kernel dcv_gemm_nt_ex launches for this problem (DCV_TILE_NARROW / _WIDE / _PAIR / _WS), or a negative error for an illegal forced tile
extern "C" int dcv_gemm_nt_pick(int M, int N, int K, int epilogue, int tile) {
    if (tile < DCV_TILE_AUTO || tile > DCV_TILE_AUTO_WS) return DCV_ERR_SHAPE;
    const bool legal384 = (N % N3_BN) == 0 && epilogue != DCV_EPI_PATCH;
    const bool legal_ws = DCV_NT_WS && K == 384 && (N % 384) == 0 && nt_ws_takes(epilogue);
    if (tile == DCV_TILE_WS) return legal_ws ? DCV_TILE_WS : DCV_ERR_UNSUPPORTED;
    if (tile == DCV_TILE_AUTO_WS) {
        // the weight-stationary kernel where it measured faster (tools/gemm_bench.py), else AUTO's choice
        if (legal_ws && M >= DCV_WS_M_MIN) return DCV_TILE_WS;
        tile = DCV_TILE_AUTO;
    }
    if (tile == DCV_TILE_WIDE) return legal384 ? DCV_TILE_WIDE : DCV_ERR_UNSUPPORTED;
    if (tile == DCV_TILE_ALT) return DCV_ERR_UNSUPPORTED;  // retired (docs/retired_experiments.md); the number stays reserved
    if (tile == DCV_TILE_NARROW) return DCV_TILE_NARROW;
    if (tile == DCV_TILE_PAIR) return epilogue != DCV_EPI_PATCH ? DCV_TILE_PAIR : DCV_ERR_UNSUPPORTED;
#ifndef DCV_WIDE_K_MIN
#define DCV_WIDE_K_MIN 1536
#endif
    if (!legal384 || epilogue == DCV_EPI_GELU_BWD_BF16 || !(N >= 1152 || K >= DCV_WIDE_K_MIN)) return DCV_TILE_NARROW;
    // Both kernels are persistent, so a launch costs rounds x time per tile, rounds = ceil(tiles / workgroups).  A 256 x 384 tile takes
    // 2.3 (K >= 1536: the k-loop dominates) to 2.5 (K = 384: the epilogue dominates) times a 256 x 128 tile (measured from the per-round
    // times at M = 12 369 ... 100 416, tools/gemm_mid_m.py, tools/gemm_bench.py): wide wins when its rounds x that factor stay below
    // the narrow kernel's rounds — always at the headline's M, seldom at a few rounds (M = 25 104, N = 1152: 297 wide tiles = 2 rounds
    // = 40 us against 891 narrow tiles = 4 rounds = 34 us).
    const int G = dcv_cu_count();
    const long tw = (long)((M + N3_BM - 1) / N3_BM) * (N / N3_BN), tn = 3 * tw;
    const long rw = (tw + G - 1) / G, rn = (tn + G - 1) / G;
    return (10 * rw * (K >= 1536 ? 23 : 25) < 100 * rn) ? DCV_TILE_WIDE : DCV_TILE_NARROW;
}

// Row-tile plan of gemm_nt384_kernel (host logic, no GPU call).  The kernel deals its tiles statically, tile L = k * grid + pos in round k, so a
// launch lasts as long as the workgroup with the most rows.  With 256-row tiles only, M = 100 416 on 256 workgroups is 393 tiles: two rounds for
// 1.53 rounds of work.  The plan makes the LAST row tiles 192 rows high (3 of a wave's 4 row blocks; nothing else about a tile changes), so the
// last round(s) are shorter: rows [0, 256 n256) in 256-row tiles, the rest in n192 = ceil((M - 256 n256) / 192) tiles of 192 rows.
//   * Heights fall along the walk, so workgroup 0 walks the most rows: 256 c + 192 (R - c) with R = ceil(tiles / grid) rounds, of which
//     c = ceil(n256 tiles_n / grid) start on a 256-row tile.
//   * No workgroup may walk more tiles than before: R stays ceil(old tiles / grid).  Lowering n256 only adds tiles, so the smallest n256 that
//     still fits R rounds gives the smallest c; among the plans with that c the one with the MOST 256-row tiles is taken (fewest tiles, each of
//     which re-reads its W panel): n256 = floor(c grid / tiles_n).
//   * Where that does not lower the largest walk (one round or less, or rows that mixed rounds cannot cover) the answer is the old plan, n192 = 0.
// Headline: M = 100 416, grid 256 -> 256 + 182 tiles, 448 rows per workgroup instead of 512 (grid 248: 248 + 193, 448).
// -DDCV_N3_BALANCE=0: always the old plan (the A/B build).
#ifndef DCV_N3_BALANCE
#define DCV_N3_BALANCE 1
#endif
extern "C" int dcv_gemm_nt384_plan(int M, int N, int grid, int* n256, int* n192) {
    if (!n256 || !n192) return DCV_ERR_NULL;
    if (M <= 0 || N <= 0 || (N % N3_BN) != 0 || grid <= 0) return DCV_ERR_SHAPE;
    const long tn = N / N3_BN, G = grid;
    const long old_m = (M + N3_BM - 1) / N3_BM;
    *n256 = (int)old_m;
    *n192 = 0;
    const long R = (old_m * tn + G - 1) / G;
    if (!DCV_N3_BALANCE || R <= 1) return DCV_OK;
    auto rest192 = [&](long a) { return a * N3_BM >= M ? 0L : (M - a * N3_BM + 191) / 192; };
    long lo = 0, hi = old_m;  // smallest n256 whose tiles fit R rounds (the tile count falls as n256 grows; old_m fits)
    while (lo < hi) {
        const long mid = (lo + hi) / 2;
        if ((mid + rest192(mid)) * tn <= R * G) hi = mid;
        else lo = mid + 1;
    }
    const long c = (lo * tn + G - 1) / G;
    const long a = std::min(c * G / tn, old_m);
    if (c >= R || rest192(a) == 0) return DCV_OK;
    *n256 = (int)a;
    *n192 = (int)rest192(a);
    return DCV_OK;
}

// what an epilogue needs beyond A, W and out: its pointers, and for PATCH the shape of its embedding tables
static int nt_epilogue_check(int epilogue, const GemmNtArgs& a) {
    switch (epilogue) {
        case DCV_EPI_BIAS_BF16:
        case DCV_EPI_BIAS_RESID_F32: return a.bias ? DCV_OK : DCV_ERR_NULL;
        case DCV_EPI_BIAS_GELU_BF16: return a.bias && a.out2 ? DCV_OK : DCV_ERR_NULL;
        case DCV_EPI_PLAIN_BF16: return DCV_OK;
        case DCV_EPI_GELU_BWD_BF16: return a.aux ? DCV_OK : DCV_ERR_NULL;
        case DCV_EPI_PATCH:
            return a.bias && a.aux && a.aux2 && a.T > 0 && a.n > 0 && (a.M % a.T) == 0 && (a.T % a.n) == 0 ? DCV_OK : DCV_ERR_SHAPE;
        default: return DCV_ERR_UNSUPPORTED;
    }
}

// launches the picked kernel (dcv_gemm_nt_pick) on that kernel's grid of at most `cap` workgroups; a combination that has no kernel is refused
template <int EPI>
static int nt_launch(int pick, GemmNtArgs& a, int cap, hipStream_t s) {
    if (pick == DCV_TILE_WS) {
        if constexpr (DCV_NT_WS && nt_ws_takes(EPI)) {
            // whole groups of N / 384 workgroups (one per weight slice), at most one group per 32-row panel; a CU count that the slice count does
            // not divide leaves the remainder idle (qkv: 85 groups of 3 on 256 CUs)
            const int slices = a.N / WS_BN, panels = (a.M + WS_BM - 1) / WS_BM;
            const int groups = std::min(cap / slices, panels);
            hipLaunchKernelGGL(gemm_nt_ws_kernel<EPI>, dim3(groups * slices), dim3(64 * WS_WAVES), 0, s, a);
        } else
            return DCV_ERR_UNSUPPORTED;
    } else if (pick == DCV_TILE_WIDE) {
        if constexpr (EPI != DCV_EPI_PATCH) {
            int g3 = ((a.M + N3_BM - 1) / N3_BM) * (a.N / N3_BN);
            if (g3 > cap) g3 = cap;
            int n192;
            dcv_gemm_nt384_plan(a.M, a.N, g3, &a.n256, &n192);  // the grid is min(tiles, cap) under either plan: a plan with 192-row tiles has more than one round
            a.tiles_m = a.n256 + n192;
            hipLaunchKernelGGL(gemm_nt384_kernel<EPI>, dim3(g3), dim3(512), 0, s, a);
        } else
            return DCV_ERR_UNSUPPORTED;  // the tokeniser epilogue exists on the 256 x 128 kernel only
    } else if (pick == DCV_TILE_PAIR) {
        if constexpr (EPI != DCV_EPI_PATCH) {
            int gp = ((a.M + NP_BM - 1) / NP_BM) * ((a.N + NP_BN - 1) / NP_BN);
            if (gp > 2 * cap) gp = 2 * cap;  // two workgroups per CU
            hipLaunchKernelGGL(gemm_nt_pair_kernel<EPI>, dim3(gp), dim3(256), 0, s, a);
        } else
            return DCV_ERR_UNSUPPORTED;
    } else {
        int grid = ((a.M + NT_BM - 1) / NT_BM) * ((a.N + NT_BN - 1) / NT_BN);
        if (grid > cap) grid = cap;
        hipLaunchKernelGGL(gemm_nt_kernel<EPI>, dim3(grid), dim3(512), 0, s, a);
    }
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

extern "C" int dcv_gemm_nt_ex(const void* A, int lda, const void* W, int ldw, int M, int N, int K, int epilogue,
                              const float* bias, void* out, int ldo, void* out2, int ldo2, const void* aux, int ldaux,
                              const float* aux2, int T, int n, int grid_cap, int tile, void* stream) {
    if (!A || !W || !out) return DCV_ERR_NULL;
    if (M <= 0 || N <= 0 || K <= 0 || (K % 64) != 0 || (N % 8) != 0) return DCV_ERR_SHAPE;
    if ((lda % 8) || (ldw % 8) || (ldo % 8) || ((uintptr_t)A & 15) || ((uintptr_t)W & 15) || ((uintptr_t)out & 15)) return DCV_ERR_ALIGN;
    if (grid_cap < 0 || tile < DCV_TILE_AUTO || tile > DCV_TILE_AUTO_WS) return DCV_ERR_SHAPE;
    if (epilogue == DCV_EPI_BIAS_RESID_F32 && aux2 && (T <= 0 || (M % T) != 0)) return DCV_ERR_SHAPE;  // per-sample branch scale: T rows per sample
    // A row stride below the row's width would make rows overlap silently; the strides of the optional buffers count only where the epilogue
    // uses them (callers pass 0 with a null pointer).  out2: bf16 (GELU) or fp32 (PATCH); aux: fp32 residual / embedding rows (PATCH: aux2 shares
    // ldaux) or the bf16 saved GELU'(z) — all of them move in 16-byte pieces.
    if (lda < K || ldw < K || ldo < N) return DCV_ERR_SHAPE;
    const bool uses_out2 = out2 && (epilogue == DCV_EPI_BIAS_GELU_BF16 || epilogue == DCV_EPI_PATCH);
    const bool uses_aux = aux && (epilogue == DCV_EPI_BIAS_RESID_F32 || epilogue == DCV_EPI_GELU_BWD_BF16 || epilogue == DCV_EPI_PATCH);
    if ((uses_out2 && ldo2 < N) || (uses_aux && ldaux < N)) return DCV_ERR_SHAPE;
    if ((uses_out2 && (ldo2 % (epilogue == DCV_EPI_PATCH ? 4 : 8))) || (uses_aux && (ldaux % (epilogue == DCV_EPI_GELU_BWD_BF16 ? 8 : 4))))
        return DCV_ERR_ALIGN;
    // persistent kernels: one workgroup per CU walks the tiles; grid_cap (> 0) lowers the number of workgroups — the data-parallel
    // backward leaves CUs to RCCL's kernels this way (dichavit.py), tests force multi-round walks on small problems
    const int cap = grid_cap > 0 ? grid_cap : dcv_cu_count();
    GemmNtArgs a{(const bf16_t*)A, lda, (const bf16_t*)W, ldw, M, N, K, bias, out, ldo, out2, ldo2, aux, ldaux, aux2, T, n};
    hipStream_t s = (hipStream_t)stream;
    // 256 x 384 tiles where they pay (measured, M = 100 416, against the 256 x 128 kernel): N = 1152 K = 384: 121 -> 107 us;
    // N = 1536 K = 384 + GELU: 238 -> 218; N = 384 K = 1536: 192 -> 184 (+residual), 154 -> 138 (plain); but N = 384 K = 384:
    // 96 -> 101 (393 tiles on 256 CUs: two rounds for 1.5 rounds of work — measured before dcv_gemm_nt384_plan made the second round's tiles 192
    // rows high; the choice was not re-tuned), and the GELU-backward epilogue (N = 1536, HBM-heavy: 616 MB in + out) 212 -> 220.  tile = DCV_TILE_WIDE forces the 256 x 384 kernel wherever it is legal, DCV_TILE_NARROW never uses it.
    int pick = dcv_gemm_nt_pick(M, N, K, epilogue, tile);
    if (pick < 0) return pick;
    if (pick == DCV_TILE_WS && cap < N / WS_BN) {  // fewer workgroups than weight slices: only the tiled kernels can run under this cap
        if (tile == DCV_TILE_WS) return DCV_ERR_UNSUPPORTED;
        pick = dcv_gemm_nt_pick(M, N, K, epilogue, DCV_TILE_AUTO);
    }
    // its 16-byte pieces of the optional buffers (checked before the epilogue's own needs)
    if (pick == DCV_TILE_WS && ((ldo2 % 8) || (ldaux % 8) || ((uintptr_t)out2 & 15) || ((uintptr_t)aux & 15) || ((uintptr_t)bias & 15))) return DCV_ERR_ALIGN;
    if (const int err = nt_epilogue_check(epilogue, a)) return err;
    switch (epilogue) {
        case DCV_EPI_BIAS_BF16: return nt_launch<DCV_EPI_BIAS_BF16>(pick, a, cap, s);
        case DCV_EPI_BIAS_GELU_BF16: return nt_launch<DCV_EPI_BIAS_GELU_BF16>(pick, a, cap, s);
        case DCV_EPI_BIAS_RESID_F32: return nt_launch<DCV_EPI_BIAS_RESID_F32>(pick, a, cap, s);
        case DCV_EPI_PLAIN_BF16: return nt_launch<DCV_EPI_PLAIN_BF16>(pick, a, cap, s);
        case DCV_EPI_GELU_BWD_BF16: return nt_launch<DCV_EPI_GELU_BWD_BF16>(pick, a, cap, s);
        case DCV_EPI_PATCH: return nt_launch<DCV_EPI_PATCH>(pick, a, cap, s);
    }
    return DCV_ERR_UNSUPPORTED;  // (nt_epilogue_check let no other value through)
}

extern "C" int dcv_gemm_nt_resid_ln(const void* A, int lda, const void* W, int ldw, int M, int N, int K, const float* bias, const float* resid,
                                    int ldr, const float* branch_scale, int T, float* x_out, int ldo, const float* gamma, const float* beta,
                                    float eps, void* u_out, int ldu, float* mean, float* rstd, int grid_cap, void* stream) {
    if (!A || !W || !bias || !resid || !x_out || !gamma || !beta || !u_out || !mean || !rstd) return DCV_ERR_NULL;
    if (M <= 0 || K <= 0 || (K % 64) != 0 || grid_cap < 0) return DCV_ERR_SHAPE;
    if (N != N3_BN) return DCV_ERR_UNSUPPORTED;  // the tile must span whole rows
    if (lda < K || ldw < K || ldo < N || ldr < N || ldu < N) return DCV_ERR_SHAPE;  // rows would overlap
    if ((lda % 8) || (ldw % 8) || (ldo % 4) || (ldr % 4) || (ldu % 8) || ((uintptr_t)A & 15) || ((uintptr_t)W & 15) || ((uintptr_t)x_out & 15) ||
        ((uintptr_t)resid & 15) || ((uintptr_t)u_out & 15) || ((uintptr_t)bias & 15) || ((uintptr_t)gamma & 15) || ((uintptr_t)beta & 15))
        return DCV_ERR_ALIGN;
    if (branch_scale && (T <= 0 || (M % T) != 0)) return DCV_ERR_SHAPE;
    const int cap = grid_cap > 0 ? grid_cap : dcv_cu_count();
    GemmNtArgs a{(const bf16_t*)A, lda, (const bf16_t*)W, ldw, M, N, K, bias, x_out, ldo, u_out, ldu, resid, ldr, branch_scale, T > 0 ? T : 1, 0,
                 gamma, beta, mean, rstd, eps};
    int g3 = (M + N3_BM - 1) / N3_BM;
    if (g3 > cap) g3 = cap;
    int n192;
    dcv_gemm_nt384_plan(M, N, g3, &a.n256, &n192);
    a.tiles_m = a.n256 + n192;
    hipLaunchKernelGGL(gemm_nt384_kernel<DCV_EPI_RESID_LN>, dim3(g3), dim3(512), 0, (hipStream_t)stream, a);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

extern "C" int dcv_gemm_nt(const void* A, int lda, const void* W, int ldw, int M, int N, int K, int epilogue,
                           const float* bias, void* out, int ldo, void* out2, int ldo2, const void* aux, int ldaux,
                           const float* aux2, int T, int n, void* stream) {
    return dcv_gemm_nt_ex(A, lda, W, ldw, M, N, K, epilogue, bias, out, ldo, out2, ldo2, aux, ldaux, aux2, T, n, 0, DCV_TILE_AUTO_WS, stream);
}
