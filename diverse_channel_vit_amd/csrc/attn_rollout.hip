// One step of attention rollout over one encoder block, heads averaged: the path of ChannelVisionTransformer.get_attention_rollout.
//     qkv [B,N,3,H,64] bf16 + the forward's LSE [B,H,N] f32 (natural log) + w [B,N] f32 (w >= 0)  ->  out [B,N] f32
//     out[b,k] = alpha w[b,k] + (1 - alpha) / H  sum_h sum_q w[b,q] P[b,h,q,k]
// with P[b,h,q,k] = exp(s_qk - LSE_q) exactly as attn_probs_kernel forms it: the row vector w pushed through alpha I + (1 - alpha) mean_h P.
// No [., N, N] array is written anywhere and there is no workspace: what get_last_selfattention plus a torch reduction moves through HBM
// (3.78 GB written and read again per block at B 64, H 6, N 1569) stays in registers.
//
// Skeleton of attn_channel_mass_kernel with the roles of the two axes exchanged: a workgroup of 4 waves owns 128 KEYS of one image and sweeps
// ALL query tiles (64 queries x 64 dims, 8 KB, staged in LDS by the whole workgroup, one tile ahead in registers) of head 0, then head 1, ...
//   * S = Q . K^T with the KEY on the lane: the B operand (this wave's 32 keys of the running head) stays in registers for the whole head,
//     the A operand comes from the LDS tile; accumulator register r of lane (r32, h) is query q0 + acc_row(r, h) of key k0 + r32;
//   * the query weight rides in the row constant c_q = log2(w_q) - LSE_q log2(e), staged with the Q tile (64 floats): w_q p_qk = exp2(s_qk + c_q).
//     In the pre-scaled-q form c_q is the initial accumulator of the MFMA chain; the plain form pays one fma more per score.  w_q = 0 — and every
//     query row past N, which the tile loads clamp in bounds — has c_q = -inf: exp2(-inf) = 0, the row contributes exactly nothing;
//   * a lane's 16 registers are 16 queries of ONE key: they are added as a fixed tree, the tree sums of the sweep as a chain into one running
//     sum; at the end of a head the two half-waves' partials are added once (lower half + upper half) and that total joins the head sum, heads
//     in increasing order.
// Everything after the bf16 operands is fp32.  No atomics, LDS or global: out[b,k] is written once by one lane, and the order of every add is a
// function of (N, H) alone — bitwise reproducible, and out[b,k] does not depend on which other keys are computed.  Every workgroup reads all of
// w[b,:], so out must not overlap w (refused).
#include <cmath>
#include "attn_common.hpp"

namespace {

struct RolloutArgs {
    const bf16_t* qkv;  // [B,N,3,H,64]
    const float* lse;   // [B,H,N]
    const float* w;     // [B,N]
    float* out;         // [B,N]
    int B, N, H;
    float c;      // plain form: scale * log2(e)
    float alpha;  // weight of the identity
    float beta;   // (1 - alpha) / H
};

constexpr int RO_KTILE = 128;  // keys per workgroup (4 waves x 32)

template <bool PS>
__global__ __launch_bounds__(256) void attn_rollout_kernel(RolloutArgs a) {
    __shared__ __attribute__((aligned(16))) char sQ[64 * 128];
    __shared__ __attribute__((aligned(16))) float sC[64];  // the row constants of the tile's 64 queries
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, r32 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nkt = (a.N + RO_KTILE - 1) / RO_KTILE;
    const int b = blockIdx.x / nkt, kt = blockIdx.x % nkt;
    const int D = a.H * 64;
    const size_t rs = (size_t)3 * D;
    const bf16_t* Qb = a.qkv + (size_t)b * a.N * rs;  // head 0; + 64 per head
    const int nt = (a.N + 63) / 64;
    const int k0 = kt * RO_KTILE + wave * 32;  // this wave's first key
    const bool active = k0 < a.N;              // wave-uniform: a wave past N only helps stage Q
    const int key = k0 + r32, kc = min(key, a.N - 1);
    const float* wb = a.w + (size_t)b * a.N;
    const float* lb = a.lse + (size_t)b * a.H * a.N;  // head 0; + N per head

    // tile (head hn, query tile tn) on its way to LDS: the Q rows (clamped in bounds) and, in threads 0 .. 63, the query's weight and LSE — the
    // row constant is formed when the tile is stored, a tile later, so that these loads too stay in flight behind the running tile's MFMAs
    Stage64 st;
    float wq = 0.f, lq = 0.f;
    auto fetch = [&](int hn, int tn) {
        stage_load(st, Qb + hn * 64, rs, tn * 64, a.N, tid);
        if (tid < 64) {
            const int q = tn * 64 + tid, qc = min(q, a.N - 1);
            wq = q < a.N ? wb[qc] : 0.f;
            lq = lb[(size_t)hn * a.N + qc];
        }
    };

    float tot = 0.f;  // sum over the heads done so far of this key's column sum
    fetch(0, 0);
    for (int hh = 0; hh < a.H; ++hh) {
        // B operand: lane (column r32, half h) holds K[k0 + r32][16 ks + 8 h .. +7] of head hh (rows clamped in bounds; their results are not stored)
        bf16x8 kf[4];
        const bf16_t* Kr = Qb + D + hh * 64 + (size_t)kc * rs;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) kf[ks] = as_bf16x8(*reinterpret_cast<const uint4*>(Kr + 16 * ks + 8 * h));
        float acc = 0.f;
        for (int t = 0; t < nt; ++t) {
            if (hh | t) __syncthreads();  // every wave is done reading the previous tile
            stage_store(st, sQ, tid);
            if (tid < 64) sC[tid] = wq > 0.f ? log2f(wq) - lq * LOG2E : -INFINITY;
            __syncthreads();
            if (t + 1 < nt) fetch(hh, t + 1);
            else if (hh + 1 < a.H) fetch(hh + 1, 0);
            if (!active) continue;
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) {
                if (t * 64 + qb * 32 >= a.N) break;
                // register r is query qb * 32 + acc_row(r, h) of the tile: four runs of four consecutive row constants
                f32x16 rowc;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 c4 = *reinterpret_cast<const float4*>(sC + qb * 32 + 8 * g + 4 * h);
                    rowc[4 * g] = c4.x; rowc[4 * g + 1] = c4.y; rowc[4 * g + 2] = c4.z; rowc[4 * g + 3] = c4.w;
                }
                f32x16 s;
                if constexpr (PS) s = rowc;
                else zero_acc(s);
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) s = mfma32(frag_rows(sQ, qb * 32, r32, h, ks), kf[ks], s);
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = PS ? __builtin_amdgcn_exp2f(s[r]) : __builtin_amdgcn_exp2f(fmaf(s[r], a.c, rowc[r]));
                // 16 queries of this lane's key: a fixed tree, then one add into the running sum
#pragma unroll
                for (int w2 = 8; w2 > 0; w2 >>= 1)
#pragma unroll
                    for (int r = 0; r < w2; ++r) s[r] += s[r + w2];
                acc += s[0];
            }
        }
        if (active) tot += sum_halves(acc);
    }
    if (active && h == 0 && key < a.N) a.out[(size_t)b * a.N + key] = a.alpha * wb[key] + a.beta * tot;
}

}  // namespace

static int attn_rollout_launch(const void* qkv, const float* lse, const float* w, float* out, int B, int N, int H, int head_dim, float scale,
                               float alpha, bool ps, void* stream) {
    int rc = attn_check(qkv, B, N, H, head_dim);
    if (rc) return rc;
    if (!lse || !w || !out) return DCV_ERR_NULL;
    if (((uintptr_t)lse | (uintptr_t)w | (uintptr_t)out) & 3) return DCV_ERR_ALIGN;
    if (!(alpha >= 0.f && alpha < 1.f)) return DCV_ERR_UNSUPPORTED;  // NaN included
    const long grid = (long)B * (((long)N + RO_KTILE - 1) / RO_KTILE);
    if (grid > 0x7fffffff) return DCV_ERR_SHAPE;
    const uintptr_t nbytes = (uintptr_t)B * (uintptr_t)N * sizeof(float), w0 = (uintptr_t)w, o0 = (uintptr_t)out;
    if (w0 < o0 + nbytes && o0 < w0 + nbytes) return DCV_ERR_UNSUPPORTED;  // every workgroup reads all of w[b,:]
    RolloutArgs a{(const bf16_t*)qkv, lse, w, out, B, N, H, scale * LOG2E, alpha, (1.f - alpha) / (float)H};
    if (ps) hipLaunchKernelGGL(attn_rollout_kernel<true>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(attn_rollout_kernel<false>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

extern "C" int dcv_attn_rollout_step(const void* qkv, const float* lse, const float* w, float* out, int B, int N, int H, int head_dim, float scale,
                                     float alpha, void* stream) {
    return attn_rollout_launch(qkv, lse, w, out, B, N, H, head_dim, scale, alpha, false, stream);
}

// the q part of qkv holds q * scale * log2(e) (dcv_attn_fwd_rows_ps); lse as that entry wrote it (natural log)
extern "C" int dcv_attn_rollout_step_ps(const void* qkv, const float* lse, const float* w, float* out, int B, int N, int H, int head_dim,
                                        float alpha, void* stream) {
    return attn_rollout_launch(qkv, lse, w, out, B, N, H, head_dim, 0.f, alpha, true, stream);
}
