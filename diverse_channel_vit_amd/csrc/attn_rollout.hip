// One step, over one encoder block with the heads averaged, of the two probes that push a row vector w [B,N] f32 (w >= 0) through the attention maps:
//     qkv [B,N,3,H,64] bf16 + the forward's LSE [B,H,N] f32 (natural log) + w  (+ dO [B,N,H*64] bf16)  ->  out [B,N] f32
//   rollout (Abnar & Zuidema; ChannelVisionTransformer.get_attention_rollout), GRAD = false, launched with Nq = N and no dO:
//     out[b,k] = alpha w[b,k] + (1 - alpha) / H  sum_h sum_q w[b,q] P[b,h,q,k]                  w through alpha I + (1 - alpha) mean_h P
//   gradient-weighted relevance (Chefer, Gur & Wolf 2021; get_attention_relevance), GRAD = true:
//     out[b,k] = w[b,k] + 1 / H  sum_h sum_{q < Nq} w[b,q] P[b,h,q,k] max(G[b,h,q,k], 0)        w through I + mean_h relu(grad A . A)
// with P[b,h,q,k] = exp(s_qk - LSE_q) exactly as attn_probs_kernel forms it and G[b,h,q,k] = sum_d dO[b,q,h,d] V[b,k,h,d] = d(target) / dP, the
// dP of the flash backward (bf16 operands, fp32 accumulation).  Neither P nor G reaches HBM, no [., N, N] array is written anywhere and there is
// no workspace: what get_last_selfattention plus a torch reduction moves through HBM (3.78 GB written and read again per block at B 64, H 6,
// N 1569) stays in registers.
//
// Skeleton of attn_channel_mass_kernel with the roles of the two axes exchanged: a workgroup of 4 waves owns 128 KEYS of one image and sweeps
// ALL query tiles (64 queries x 64 dims, 8 KB; with GRAD also the dO tile of the same 64 queries) of head 0, then head 1, ...; the tiles are
// staged in LDS by the whole workgroup, one tile ahead in registers.
//   * S = Q . K^T with the KEY on the lane: the B operand (this wave's 32 keys of the running head; with GRAD also the V fragment of the same
//     keys) stays in registers for the whole head, the A operands (Q rows for S, dO rows for G) come from the LDS tiles; accumulator register r of
//     lane (r32, h) is query q0 + acc_row(r, h) of key k0 + r32 in both products;
//   * the query weight rides in the row constant c_q = log2(w_q) - LSE_q log2(e), staged with the tile (64 floats): w_q p_qk = exp2(s_qk + c_q).
//     In the pre-scaled-q form c_q is the initial accumulator of the MFMA chain; the plain form pays one fma more per score.  w_q = 0 — and every
//     query row at or past Nq — has c_q = -inf: exp2(-inf) = 0, the row contributes exactly nothing;
//   * with GRAD the product with max(G, 0) is SELECTED on the weight: a row with c_q = -inf contributes an exact +0 whatever its dO row holds
//     (NaN and Inf included; 0 * Inf is never formed);
//   * only query rows [0, Nq) are read, from qkv, lse, w and dO: the tile loads clamp into [0, Nq).  In the CLS-only last block dO holds the CLS
//     rows only (Nq = 1);
//   * a lane's 16 registers are 16 queries of ONE key: they are added as a fixed tree, the tree sums of the sweep as a chain into one running
//     sum; at the end of a head the two half-waves' partials are added once (lower half + upper half) and that total joins the head sum, heads
//     in increasing order.
// Everything after the bf16 operands is fp32.  No atomics, LDS or global: out[b,k] is written once by one lane, and the order of every add is a
// function of (N, Nq, H) alone — bitwise reproducible, and out[b,k] does not depend on which other keys are computed.  Every workgroup reads all
// of w[b,:Nq], so out must not overlap w (refused).
#include <cmath>
#include "attn_common.hpp"

namespace {

struct KeysweepArgs {
    const bf16_t* qkv;  // [B,N,3,H,64]
    const float* lse;   // [B,H,N]
    const bf16_t* dO;   // [B,N,H*64]; GRAD only
    const float* w;     // [B,N]
    float* out;         // [B,N]
    int B, N, Nq, H;
    float c;      // plain form: scale * log2(e)
    float alpha;  // weight of the identity; rollout only
    float beta;   // rollout: (1 - alpha) / H; relevance: 1 / H
};

constexpr int KS_KTILE = 128;  // keys per workgroup (4 waves x 32)

template <bool PS, bool GRAD>
__global__ __launch_bounds__(256) void attn_keysweep_kernel(KeysweepArgs a) {
    __shared__ __attribute__((aligned(16))) char sQ[64 * 128];
    __shared__ __attribute__((aligned(16))) char sG[64 * 128];  // the dO rows of the same 64 queries; never named without GRAD: no LDS there
    __shared__ __attribute__((aligned(16))) float sC[64];       // their row constants
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, r32 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nkt = (a.N + KS_KTILE - 1) / KS_KTILE;
    const int b = blockIdx.x / nkt, kt = blockIdx.x % nkt;
    const int D = a.H * 64;
    const size_t rs = (size_t)3 * D;
    const bf16_t* Qb = a.qkv + (size_t)b * a.N * rs;                  // head 0; + 64 per head
    const bf16_t* Gb = GRAD ? a.dO + (size_t)b * a.N * D : nullptr;  // head 0; + 64 per head
    const int nt = (a.Nq + 63) / 64;
    const int k0 = kt * KS_KTILE + wave * 32;  // this wave's first key
    const bool active = k0 < a.N;              // wave-uniform: a wave past N only helps stage the tiles
    const int key = k0 + r32, kc = min(key, a.N - 1);
    const float* wb = a.w + (size_t)b * a.N;
    const float* lb = a.lse + (size_t)b * a.H * a.N;  // head 0; + N per head

    // tile (head hn, query tile tn) on its way to LDS: the Q and dO rows (clamped into [0, Nq)) and, in threads 0 .. 63, the query's weight and
    // LSE — the row constant is formed when the tile is stored, a tile later, so that these loads too stay in flight behind the running tile's MFMAs
    Stage64 stq, stg;
    float wq = 0.f, lq = 0.f;
    auto fetch = [&](int hn, int tn) {
        stage_load(stq, Qb + hn * 64, rs, tn * 64, a.Nq, tid);
        if constexpr (GRAD) stage_load(stg, Gb + hn * 64, (size_t)D, tn * 64, a.Nq, tid);
        if (tid < 64) {
            const int q = tn * 64 + tid, qc = min(q, a.Nq - 1);
            wq = q < a.Nq ? wb[qc] : 0.f;
            lq = lb[(size_t)hn * a.N + qc];
        }
    };

    float tot = 0.f;  // sum over the heads done so far of this key's column sum
    fetch(0, 0);
    for (int hh = 0; hh < a.H; ++hh) {
        // B operands: lane (column r32, half h) holds K[k0 + r32][16 ks + 8 h .. +7] and, with GRAD, V[k0 + r32][the same] of head hh (rows
        // clamped in bounds; their results are not stored)
        bf16x8 kf[4], vf[4];
        const bf16_t* Kr = Qb + D + hh * 64 + (size_t)kc * rs;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            kf[ks] = as_bf16x8(*reinterpret_cast<const uint4*>(Kr + 16 * ks + 8 * h));
            if constexpr (GRAD) vf[ks] = as_bf16x8(*reinterpret_cast<const uint4*>(Kr + D + 16 * ks + 8 * h));
        }
        float acc = 0.f;
        for (int t = 0; t < nt; ++t) {
            if (hh | t) __syncthreads();  // every wave is done reading the previous tiles
            stage_store(stq, sQ, tid);
            if constexpr (GRAD) stage_store(stg, sG, tid);
            if (tid < 64) sC[tid] = wq > 0.f ? log2f(wq) - lq * LOG2E : -INFINITY;
            __syncthreads();
            if (t + 1 < nt) fetch(hh, t + 1);
            else if (hh + 1 < a.H) fetch(hh + 1, 0);
            if (!active) continue;
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) {
                if (t * 64 + qb * 32 >= a.Nq) break;
                // register r is query qb * 32 + acc_row(r, h) of the tile: four runs of four consecutive row constants
                f32x16 rowc;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 c4 = *reinterpret_cast<const float4*>(sC + qb * 32 + 8 * g + 4 * h);
                    rowc[4 * g] = c4.x; rowc[4 * g + 1] = c4.y; rowc[4 * g + 2] = c4.z; rowc[4 * g + 3] = c4.w;
                }
                f32x16 s, gr;
                if constexpr (PS) s = rowc;
                else zero_acc(s);
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) s = mfma32(frag_rows(sQ, qb * 32, r32, h, ks), kf[ks], s);
                if constexpr (GRAD) {
                    zero_acc(gr);
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) gr = mfma32(frag_rows(sG, qb * 32, r32, h, ks), vf[ks], gr);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    // a local: exp2 written to s[r] and multiplied there costs the <true, true> form 8 VGPRs (184 against 176)
                    const float p = PS ? __builtin_amdgcn_exp2f(s[r]) : __builtin_amdgcn_exp2f(fmaf(s[r], a.c, rowc[r]));
                    // selected on the weight, not multiplied: a row of weight 0 adds +0 whatever its gradient row holds
                    if constexpr (GRAD) s[r] = rowc[r] == -INFINITY ? 0.f : p * fmaxf(gr[r], 0.f);
                    else s[r] = p;
                }
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
    if (active && h == 0 && key < a.N) {
        // the rollout's form compiles to two rounded products and an add (v_pk_mul_f32, v_add_f32); a mul + fma would be other output bits
        if constexpr (GRAD) a.out[(size_t)b * a.N + key] = fmaf(a.beta, tot, wb[key]);
        else a.out[(size_t)b * a.N + key] = a.alpha * wb[key] + a.beta * tot;
    }
}

}  // namespace

// grad = false: the rollout step (Nq = N, dO unused); grad = true: the relevance step (alpha = 0)
static int attn_keysweep_launch(const void* qkv, const float* lse, const void* dO, const float* w, float* out, int B, int N, int Nq, int H,
                                int head_dim, float scale, float alpha, bool ps, bool grad, void* stream) {
    int rc = attn_check(qkv, B, N, H, head_dim);
    if (rc) return rc;
    if (!lse || (grad && !dO) || !w || !out) return DCV_ERR_NULL;
    if (Nq < 1 || Nq > N) return DCV_ERR_SHAPE;
    if (grad && ((uintptr_t)dO & 15)) return DCV_ERR_ALIGN;
    if (((uintptr_t)lse | (uintptr_t)w | (uintptr_t)out) & 3) return DCV_ERR_ALIGN;
    if (!grad && !(alpha >= 0.f && alpha < 1.f)) return DCV_ERR_UNSUPPORTED;  // NaN included
    const long grid = (long)B * (((long)N + KS_KTILE - 1) / KS_KTILE);
    if (grid > 0x7fffffff) return DCV_ERR_SHAPE;
    const uintptr_t nbytes = (uintptr_t)B * (uintptr_t)N * sizeof(float), w0 = (uintptr_t)w, o0 = (uintptr_t)out;
    if (w0 < o0 + nbytes && o0 < w0 + nbytes) return DCV_ERR_UNSUPPORTED;  // every workgroup reads all of w[b,:Nq]
    KeysweepArgs a{(const bf16_t*)qkv, lse, (const bf16_t*)dO, w, out, B, N, Nq, H, scale * LOG2E, alpha, (1.f - alpha) / (float)H};
    auto kernel = grad ? (ps ? attn_keysweep_kernel<true, true> : attn_keysweep_kernel<false, true>)
                       : (ps ? attn_keysweep_kernel<true, false> : attn_keysweep_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

extern "C" int dcv_attn_rollout_step(const void* qkv, const float* lse, const float* w, float* out, int B, int N, int H, int head_dim, float scale,
                                     float alpha, void* stream) {
    return attn_keysweep_launch(qkv, lse, nullptr, w, out, B, N, N, H, head_dim, scale, alpha, false, false, stream);
}

// the q part of qkv holds q * scale * log2(e) (dcv_attn_fwd_rows_ps); lse as that entry wrote it (natural log)
extern "C" int dcv_attn_rollout_step_ps(const void* qkv, const float* lse, const float* w, float* out, int B, int N, int H, int head_dim,
                                        float alpha, void* stream) {
    return attn_keysweep_launch(qkv, lse, nullptr, w, out, B, N, N, H, head_dim, 0.f, alpha, true, false, stream);
}

extern "C" int dcv_attn_relevance_step(const void* qkv, const float* lse, const void* dO, const float* w, float* out, int B, int N, int Nq, int H,
                                       int head_dim, float scale, void* stream) {
    return attn_keysweep_launch(qkv, lse, dO, w, out, B, N, Nq, H, head_dim, scale, 0.f, false, true, stream);
}

// pre-scaled q, as dcv_attn_rollout_step_ps
extern "C" int dcv_attn_relevance_step_ps(const void* qkv, const float* lse, const void* dO, const float* w, float* out, int B, int N, int Nq, int H,
                                          int head_dim, void* stream) {
    return attn_keysweep_launch(qkv, lse, dO, w, out, B, N, Nq, H, head_dim, 0.f, 0.f, true, true, stream);
}
