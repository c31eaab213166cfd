// Attention of one encoder block reduced to CHANNEL granularity inside the kernel: the path of ChannelVisionTransformer.get_channel_attention.
// Every token belongs to one channel (token 1 + c n_p + i = patch i of channel c, token 0 = CLS), so the key axis falls into the segments
//     S_0 = {0},  S_{1+c} = {1 + c n_p, ..., (c + 1) n_p}                                          (N = 1 + C n_p tokens)
//     qkv [B,N,3,H,64] bf16 + the forward's LSE [B,H,N] f32 (natural log)  ->
//         tok [B,H,N,1+C]   f32: T[b,h,q,j] = sum_{k in S_j} P[b,h,q,k]              (every row sums to 1)
//         ch  [B,H,1+C,1+C] f32: A[b,h,i,j] = (1 / |S_i|) sum_{q in S_i} T[b,h,q,j]  (row-stochastic; row 0 = the CLS query)
// with P[b,h,q,k] = exp(s_qk - LSE_q) exactly as attn_probs_kernel forms it.  No [., N, N] array is written anywhere: what get_last_selfattention
// plus a torch reduction moves through HBM (3.78 GB written and read again per block at B 64, H 6, N 1569) stays in registers.
//
// Skeleton of attn_probs_kernel (one workgroup of 4 waves sweeps all key tiles for its 128 query rows, K tiles staged in LDS one tile ahead) with the
// MFMA operands SWAPPED: S^T = K . Q^T puts the QUERY on the lane, and accumulator register r of lane (r32, h) is key key0 + acc_row(r, h) of query
// q0 + r32.  A lane then holds 16 keys of ONE query per 32-key block, and a segment's mass is a chain of in-register adds into one running sum:
//   * the running segment (index, first key, end key) is wave-uniform state, advanced as the sweep passes the boundaries — no division;
//   * a block that lies inside the running segment (five of six at n_p = 196) takes 16 unconditional adds;
//   * a block that boundaries cross takes, per segment it touches, a select on the key index per register, and every segment that ENDS in the block
//     is flushed: the two half-waves' partials of the query are added once (v_permlane32_swap, lower half + upper half) and stored;
//   * keys past N in the last block fall outside every segment (the last one ends at N) and are never added.
// Everything after the bf16 operands is fp32.  No atomics, LDS or global: each element of T is written once by one lane, and the order of the adds of
// row q is a function of (N, n_p) alone — bitwise reproducible, and row q does not depend on which other rows are computed.
//
// The query-side mean is a second, small launch over T (fixed order: row slot s adds rows s, s + R, ... of the segment, the R slot sums are added in
// slot order).  When the caller does not want T it goes to the workspace instead (B H N (1 + C) floats: 21.7 MB at the headline shape, written and
// read once — 0.6 % of what the N x N map would move).  Every element the second launch reads was written by the first: the workspace's contents
// on entry are irrelevant.
#include "attn_common.hpp"

namespace {

struct ChMassArgs {
    const bf16_t* qkv;  // [B,N,3,H,64]
    const float* lse;   // [B,H,N]
    float* T;           // [B,H,N,1+C]
    int B, N, H, C, n_p;
    float c;  // plain form: scale * log2(e)
};

constexpr int CHM_QTILE = 128;  // query rows per workgroup (4 waves x 32)

template <bool PS>
__global__ __launch_bounds__(256) void attn_channel_mass_kernel(ChMassArgs a) {
    __shared__ __attribute__((aligned(16))) char sK[64 * 128];
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, r32 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nqt = (a.N + CHM_QTILE - 1) / CHM_QTILE;
    const int bh = blockIdx.x / nqt, qt = blockIdx.x % nqt;
    const int b = bh / a.H, hh = bh % a.H;
    const int D = a.H * 64;
    const size_t rs = (size_t)3 * D;
    const bf16_t* Qb = a.qkv + (size_t)b * a.N * rs + hh * 64;
    const bf16_t* Kb = Qb + D;
    const int nt = (a.N + 63) / 64;
    const int W = a.C + 1;
    const int q0 = qt * CHM_QTILE + wave * 32;  // this wave's first query row
    const bool active = q0 < a.N;              // wave-uniform: a wave past N only helps stage K

    // B operand: lane (column r32, half h) holds Q[q0 + r32][16 ks + 8 h .. +7] (rows clamped in bounds; their results are not stored)
    bf16x8 qf[4];
    const int q = q0 + r32, qc = min(q, a.N - 1);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = as_bf16x8(*reinterpret_cast<const uint4*>(Qb + (size_t)qc * rs + 16 * ks + 8 * h));
    // every accumulator register of this lane is query row q: one -LSE log2(e)
    const float rowc = -a.lse[(size_t)bh * a.N + qc] * LOG2E;
    float* Tq = a.T + ((size_t)bh * a.N + qc) * W;
    const bool writer = h == 0 && q < a.N;

    // the running segment [cur_lo, cur_hi) of the key sweep and this lane's partial of its mass
    int cur = 0, cur_lo = 0, cur_hi = 1;
    float acc = 0.f;
    auto flush = [&]() {
        const float tot = sum_halves(acc);
        if (writer && cur <= a.C) Tq[cur] = tot;
        acc = 0.f;
        ++cur;
        cur_lo = cur_hi;
        cur_hi += a.n_p;
    };

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
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = PS ? rowc : 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) s = mfma32(frag_rows(sK, kb * 32, r32, h, ks), qf[ks], s);
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = PS ? __builtin_amdgcn_exp2f(s[r]) : __builtin_amdgcn_exp2f(fmaf(s[r], a.c, rowc));
            const int kend = min(key0 + 32, a.N);
            const bool whole = cur_hi >= key0 + 32;  // cur_lo <= key0 always: the block lies inside the running segment
            if (whole) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc += s[r];
                if (cur_hi == key0 + 32) flush();
            } else {
                for (;;) {
                    // keys [cur_lo, cur_hi) of this block; register r is key key0 + acc_row(r, h)
                    const unsigned rel = (unsigned)(key0 + 4 * h - cur_lo), len = (unsigned)(cur_hi - cur_lo);
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc += (rel + (unsigned)acc_row(r, 0) < len) ? s[r] : 0.f;
                    if (cur_hi > kend) break;  // the segment goes on in the next block
                    flush();
                    if (cur_lo >= kend) break;
                }
            }
        }
    }
}

// A[bh, i, :] = mean over the rows q of S_i of T[bh, q, :].  One workgroup per (bh, i).  The rows of S_i are contiguous in T: with Wc = min(W, 256)
// columns per pass, thread (slot s = tid / Wc, column j) adds the rows s, s + R, s + 2 R, ... (R = 256 / Wc) in increasing order, then the R slot
// sums are added in slot order — fixed by (C, n_p) alone.
__global__ __launch_bounds__(256) void attn_channel_mean_kernel(const float* __restrict__ T, float* __restrict__ A, int N, int C, int n_p) {
    __shared__ float red[256];
    const int W = C + 1;
    const int bh = blockIdx.x / W, i = blockIdx.x % W;
    const int lo = i == 0 ? 0 : 1 + (i - 1) * n_p, len = i == 0 ? 1 : n_p;
    const int Wc = W < 256 ? W : 256, R = 256 / Wc;
    const int tid = threadIdx.x, slot = tid / Wc, jj = tid % Wc;
    const float* Ts = T + ((size_t)bh * N + lo) * W;
    float* Ao = A + ((size_t)bh * W + i) * W;
    const float inv = 1.0f / (float)len;
    for (int j0 = 0; j0 < W; j0 += Wc) {
        const int j = j0 + jj;
        float s = 0.f;
        if (slot < R && j < W)
            for (int r = slot; r < len; r += R) s += Ts[(size_t)r * W + j];
        if (j0) __syncthreads();
        red[tid] = s;
        __syncthreads();
        if (slot == 0 && j < W) {
            float t = red[jj];
            for (int k = 1; k < R; ++k) t += red[k * Wc + jj];
            Ao[j] = t * inv;
        }
    }
}

inline long chm_ws_floats(int B, int N, int H, int C) {
    if (B <= 0 || N <= 0 || H <= 0 || C <= 0 || C >= N) return DCV_ERR_SHAPE;
    return (long)B * H * N * (C + 1);
}

}  // namespace

extern "C" long dcv_attn_channel_mass_ws_floats(int B, int N, int H, int C) { return chm_ws_floats(B, N, H, C); }

static int attn_channel_mass_launch(const void* qkv, const float* lse, float* tok, float* ch, int B, int N, int H, int head_dim, float scale,
                                    int C, int n_p, float* ws, long ws_floats, bool ps, void* stream) {
    int rc = attn_check(qkv, B, N, H, head_dim);
    if (rc) return rc;
    if (!lse || (!tok && !ch)) return DCV_ERR_NULL;
    if (C < 1 || n_p < 1 || (long)C * n_p + 1 != (long)N) return DCV_ERR_SHAPE;
    if (((uintptr_t)lse | (uintptr_t)tok | (uintptr_t)ch | (uintptr_t)ws) & 3) return DCV_ERR_ALIGN;
    float* T = tok;
    if (!T) {  // the channel matrix alone: the token masses go through the workspace
        if (!ws) return DCV_ERR_NULL;
        if (ws_floats < chm_ws_floats(B, N, H, C)) return DCV_ERR_SHAPE;
        T = ws;
    }
    const long grid = (long)B * H * ((N + CHM_QTILE - 1) / CHM_QTILE), grid2 = (long)B * H * (C + 1);
    if (grid > 0x7fffffff || grid2 > 0x7fffffff) return DCV_ERR_SHAPE;
    ChMassArgs a{(const bf16_t*)qkv, lse, T, B, N, H, C, n_p, scale * LOG2E};
    if (ps) hipLaunchKernelGGL(attn_channel_mass_kernel<true>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(attn_channel_mass_kernel<false>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
    DCV_LAUNCH_CHECK();
    if (ch) {
        hipLaunchKernelGGL(attn_channel_mean_kernel, dim3((unsigned)grid2), dim3(256), 0, (hipStream_t)stream, T, ch, N, C, n_p);
        DCV_LAUNCH_CHECK();
    }
    return DCV_OK;
}

extern "C" int dcv_attn_channel_mass(const void* qkv, const float* lse, float* tok, float* ch, int B, int N, int H, int head_dim, float scale, int C,
                                     int n_p, float* ws, long ws_floats, void* stream) {
    return attn_channel_mass_launch(qkv, lse, tok, ch, B, N, H, head_dim, scale, C, n_p, ws, ws_floats, false, stream);
}

// the q part of qkv holds q * scale * log2(e) (dcv_attn_fwd_rows_ps); lse as that entry wrote it (natural log)
extern "C" int dcv_attn_channel_mass_ps(const void* qkv, const float* lse, float* tok, float* ch, int B, int N, int H, int head_dim, int C, int n_p,
                                        float* ws, long ws_floats, void* stream) {
    return attn_channel_mass_launch(qkv, lse, tok, ch, B, N, H, head_dim, 0.f, C, n_p, ws, ws_floats, true, stream);
}
