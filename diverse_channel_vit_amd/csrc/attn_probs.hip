// Attention probabilities of one encoder block, written once: the inspection path of ChannelVisionTransformer.get_last_selfattention
// (models/dichavit.py:654-663 returns Block(x, return_attention=True), i.e. softmax(q k^T * scale) of models/vit.py:128-129).
//     qkv [B,N,3,H,64] bf16 + the forward's LSE [B,H,N] f32 (natural log)  ->  P [B,H,Nq,N] f32, row pitch N floats
// P[b,h,q,k] = exp(s_qk - LSE_q): no second pass over the keys, no maximum, no sum — the forward already found them.
//
// The kernel is bound by its stores (B 64, H 6, N 1569: 3.78 GB written for 121 GFLOP of Q K^T), so its shape follows the store stream:
//   * S = Q . K^T on v_mfma_f32_32x32x16_bf16 with the KEY on the lane (as the dK / dV kernels): accumulator register r of a wave is
//     then two 128-byte runs of keys in two query rows, the access shape that stores at the full plain-store rate;
//   * one workgroup (4 waves x 32 query rows) sweeps ALL key tiles of its 128 query rows, so every cache line of a row is completed by
//     one workgroup, inside one XCD's L2 (rows are N * 4 bytes: 6276 B at N = 1569, not 128-B aligned);
//   * the row constant -LSE log2(e) is read once per row and is the accumulator's initial value in the pre-scaled-q form (q' = q scale
//     log2 e, attn_fwd3_kernel<true>): p = exp2(accumulator); the plain form pays one fma more per score;
//   * K tiles (64 keys x 64 dims, 8 KB) are staged in LDS by the whole workgroup, one tile ahead in registers.
// No atomics: each element is written once by one lane, so the output is bitwise reproducible, and row q does not depend on Nq.
#include "attn_common.hpp"

#ifndef DCV_PROBS_NT
#define DCV_PROBS_NT 0  // 1 (variant builds, tools/attn_probs_bench.py): non-temporal stores instead of plain ones
#endif

namespace {

struct ProbsArgs {
    const bf16_t* qkv;  // [B,N,3,H,64]
    const float* lse;   // [B,H,N]
    float* P;           // [B,H,Nq,N]
    int B, N, Nq, H;
    float c;  // plain form: scale * log2(e)
};

constexpr int PROBS_QTILE = 128;  // query rows per workgroup (4 waves x 32)

__device__ __forceinline__ void probs_store(float* p, float v) {
    if (DCV_PROBS_NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

template <bool PS>
__global__ __launch_bounds__(256) void attn_probs_kernel(ProbsArgs a) {
    __shared__ __attribute__((aligned(16))) char sK[64 * 128];
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, r32 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nqt = (a.Nq + PROBS_QTILE - 1) / PROBS_QTILE;
    const int bh = blockIdx.x / nqt, qt = blockIdx.x % nqt;
    const int b = bh / a.H, hh = bh % a.H;
    const int D = a.H * 64;
    const size_t rs = (size_t)3 * D;
    const bf16_t* Qb = a.qkv + (size_t)b * a.N * rs + hh * 64;
    const bf16_t* Kb = Qb + D;
    const int nt = (a.N + 63) / 64;
    const int q0 = qt * PROBS_QTILE + wave * 32;  // this wave's first query row
    const bool active = q0 < a.Nq;               // wave-uniform: a wave past Nq only helps stage K

    // A operand: lane (row r32, half h) holds Q[q0 + r32][16 ks + 8 h .. +7] (rows clamped in bounds; their results are not stored)
    bf16x8 qf[4];
    const int qc = min(q0 + r32, a.N - 1);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = as_bf16x8(*reinterpret_cast<const uint4*>(Qb + (size_t)qc * rs + 16 * ks + 8 * h));
    // accumulator register r of this lane is query row q0 + acc_row(r, h): its -LSE log2(e)
    f32x16 rowc;
    const float* lrow = a.lse + (size_t)bh * a.N;
#pragma unroll
    for (int r = 0; r < 16; ++r) rowc[r] = -lrow[min(q0 + acc_row(r, h), a.N - 1)] * LOG2E;
    float* Pw = a.P + (size_t)bh * a.Nq * a.N;
    const bool full_rows = q0 + 32 <= a.Nq;

    Stage64 st;
    stage_load(st, Kb, rs, 0, a.N, tid);
    for (int t = 0; t < nt; ++t) {
        if (t) __syncthreads();  // every wave is done reading the previous tile
        stage_store(st, sK, tid);
        __syncthreads();
        if (t + 1 < nt) stage_load(st, Kb, rs, (t + 1) * 64, a.N, tid);
        if (!active) continue;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const int key0 = t * 64 + kb * 32;
            if (key0 >= a.N) break;
            f32x16 s;
            if constexpr (PS) s = rowc;
            else zero_acc(s);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) s = mfma32(qf[ks], frag_rows(sK, kb * 32, r32, h, ks), s);
            const int key = key0 + r32;
            float* pk = Pw + key;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = q0 + acc_row(r, h);
                const float p = PS ? __builtin_amdgcn_exp2f(s[r]) : __builtin_amdgcn_exp2f(fmaf(s[r], a.c, rowc[r]));
                if (key < a.N && (full_rows || row < a.Nq)) probs_store(pk + (size_t)row * a.N, p);
            }
        }
    }
}

}  // namespace

static int attn_probs_launch(const void* qkv, const float* lse, float* P, int B, int N, int Nq, int H, int head_dim, float scale, bool ps,
                             void* stream) {
    int rc = attn_check(qkv, B, N, H, head_dim);
    if (rc) return rc;
    if (!lse || !P) return DCV_ERR_NULL;
    if (Nq < 1 || Nq > N) return DCV_ERR_SHAPE;
    if ((uintptr_t)P & 3 || (uintptr_t)lse & 3) return DCV_ERR_ALIGN;
    ProbsArgs a{(const bf16_t*)qkv, lse, P, B, N, Nq, H, scale * LOG2E};
    const long grid = (long)B * H * ((Nq + PROBS_QTILE - 1) / PROBS_QTILE);
    if (grid > 0x7fffffff) return DCV_ERR_SHAPE;
    if (ps) hipLaunchKernelGGL(attn_probs_kernel<true>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(attn_probs_kernel<false>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

extern "C" int dcv_attn_probs_rows(const void* qkv, const float* lse, float* P, int B, int N, int Nq, int H, int head_dim, float scale,
                                   void* stream) {
    return attn_probs_launch(qkv, lse, P, B, N, Nq, H, head_dim, scale, false, stream);
}

// the q part of qkv holds q * scale * log2(e) (dcv_attn_fwd_rows_ps); lse as that entry wrote it (natural log)
extern "C" int dcv_attn_probs_rows_ps(const void* qkv, const float* lse, float* P, int B, int N, int Nq, int H, int head_dim, void* stream) {
    return attn_probs_launch(qkv, lse, P, B, N, Nq, H, head_dim, 0.f, true, stream);
}
