// AdamW over the flat parameter arena with PARAMETER GROUPS: one launch, a table of runs.
// The arena is cut into sorted runs of float4 (a parameter's slot is 16-byte aligned and rounded up to 4 floats, so a float4 never
// straddles two parameters); every run names the row of hyper-parameters its elements take, or -1: skipped (a frozen parameter, or
// one without a gradient in this step: p, m, v are not written and g is not read).  The element update is optim.hip's adamw_kernel's:
//   p *= 1 - lr*wd ; m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps)
// with the same expression tree, so that the contraction the compiler chooses (-ffp-contract=fast) is the same and the result is
// bit-identical to dcv_adamw_dyn called once per run (tests/test_finetune_gpu.py holds it to that).
//
// Work split: chunks of ADAMW_G_CHUNK4 float4, chunk c to workgroup c % grid.  The table (and the rows) are copied to LDS once per
// workgroup; a chunk's first run is found once, uniformly for the workgroup, by a binary search in LDS.  Almost every chunk lies
// inside ONE run: those take the straight loop (four independent float4 per lane in flight, no table read at all).  A chunk that a
// run boundary crosses takes the per-lane loop: each lane compares its index with the current run's end and steps forward.
#include "dcv_common.hpp"
#include "../../include/dcv.h"

namespace {

constexpr int ADAMW_G_CHUNK4 = 1024;  // float4 per chunk = 4 per lane of a 256-lane workgroup (16 KB of each of p, g, m, v)
// Grid cap: past it workgroups walk chunks.  The kernel takes 86 VGPRs (the straight loop's 16 float4 in flight) and no scratch, so 5 waves per
// SIMD: 5 workgroups per CU, 1280 resident on 256 CUs; a grid of 2048 is NOT resident at once, the dispatcher hands the rest out as workgroups
// end.  Measured on DiChaViT-S's arena (5223 chunks, profiles/finetune_bench_gridcap.txt): a cap of 1280 (exactly the resident set, 4.1 rounds
// with a thin last one) is 9 us slower than dcv_adamw_dyn's 96 us; 2048 and 8192 (no walking at all) both tie it within 3 us.  2048 stays:
// the same time, and fewer copies of the table into LDS.  -DDCV_ADAMW_G_GRID_CAP=n (_build.build_variant) rebuilds that comparison.
#ifndef DCV_ADAMW_G_GRID_CAP
#define DCV_ADAMW_G_GRID_CAP 2048
#endif
constexpr int ADAMW_G_GRID_CAP = DCV_ADAMW_G_GRID_CAP;

struct AdamwRow {
    float lr, b1, b2, eps, wd, inv_bc1, inv_sqrt_bc2, gscale;
};

__device__ __forceinline__ void adamw_elem(float& pe_, float ge, float& me, float& ve, const AdamwRow& h, float decay, float step) {
    float gr = ge * h.gscale;
    float pe = pe_ * decay;
    me = h.b1 * me + (1.f - h.b1) * gr;
    ve = h.b2 * ve + (1.f - h.b2) * gr * gr;
    pe_ = pe - step * me / (sqrtf(ve) * h.inv_sqrt_bc2 + h.eps);
}

__device__ __forceinline__ void adamw_vec4(float4& P, const float4& G, float4& Mv, float4& V, const AdamwRow& h, float decay, float step) {
    adamw_elem(P.x, G.x, Mv.x, V.x, h, decay, step);
    adamw_elem(P.y, G.y, Mv.y, V.y, h, decay, step);
    adamw_elem(P.z, G.z, Mv.z, V.z, h, decay, step);
    adamw_elem(P.w, G.w, Mv.w, V.w, h, decay, step);
}

__device__ __forceinline__ AdamwRow adamw_row(const float* r) {
    AdamwRow h;
    h.lr = r[0]; h.b1 = r[1]; h.b2 = r[2]; h.eps = r[3]; h.wd = r[4]; h.inv_bc1 = r[5]; h.inv_sqrt_bc2 = r[6]; h.gscale = r[7];
    return h;
}

__global__ __launch_bounds__(256) void adamw_groups_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, int n4, const int* __restrict__ seg_end4,
                                                           const int* __restrict__ seg_group, int n_seg, const float* __restrict__ hyper,
                                                           int n_groups) {
    __shared__ int s_end[DCV_ADAMW_MAX_SEGS];
    __shared__ int s_grp[DCV_ADAMW_MAX_SEGS];
    __shared__ float s_hyp[DCV_ADAMW_MAX_GROUPS * 8];
    const int t = threadIdx.x;
    for (int i = t; i < n_seg; i += 256) {
        s_end[i] = seg_end4[i];
        const int gi = seg_group[i];
        s_grp[i] = (gi >= 0 && gi < n_groups) ? gi : -1;  // a row that does not exist is never read: the run is skipped
    }
    for (int i = t; i < n_groups * 8; i += 256) s_hyp[i] = hyper[i];
    __syncthreads();
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    const int nchunks = (n4 + ADAMW_G_CHUNK4 - 1) / ADAMW_G_CHUNK4;
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int base = c * ADAMW_G_CHUNK4;
        const int cend = min(base + ADAMW_G_CHUNK4, n4);
        // first run that ends past the chunk's first float4 (uniform); the last run takes whatever a short table leaves uncovered
        int lo = 0, hi = n_seg - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_end[mid] > base) hi = mid;
            else lo = mid + 1;
        }
        if (lo == n_seg - 1 || s_end[lo] >= cend) {
            // the whole chunk inside one run
            const int gi = s_grp[lo];
            if (gi < 0) continue;
            const AdamwRow h = adamw_row(s_hyp + 8 * gi);
            const float decay = 1.f - h.lr * h.wd, step = h.lr * h.inv_bc1;
            if (cend - base == ADAMW_G_CHUNK4) {
                float4 P[4], G[4], Mv[4], V[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i = base + j * 256 + t;
                    P[j] = p4[i]; G[j] = g4[i]; Mv[j] = m4[i]; V[j] = v4[i];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i = base + j * 256 + t;
                    adamw_vec4(P[j], G[j], Mv[j], V[j], h, decay, step);
                    p4[i] = P[j]; m4[i] = Mv[j]; v4[i] = V[j];
                }
            } else {
                for (int i = base + t; i < cend; i += 256) {
                    float4 P = p4[i], G = g4[i], Mv = m4[i], V = v4[i];
                    adamw_vec4(P, G, Mv, V, h, decay, step);
                    p4[i] = P; m4[i] = Mv; v4[i] = V;
                }
            }
            continue;
        }
        // a run boundary inside the chunk: every lane walks the table from the chunk's first run
        int s = lo, cur = -1;
        AdamwRow h = {};
        float decay = 0.f, step = 0.f;
        for (int i = base + t; i < cend; i += 256) {
            while (s < n_seg - 1 && i >= s_end[s]) ++s;
            const int gi = s_grp[s];
            if (gi < 0) continue;
            if (gi != cur) {
                cur = gi;
                h = adamw_row(s_hyp + 8 * gi);
                decay = 1.f - h.lr * h.wd;
                step = h.lr * h.inv_bc1;
            }
            float4 P = p4[i], G = g4[i], Mv = m4[i], V = v4[i];
            adamw_vec4(P, G, Mv, V, h, decay, step);
            p4[i] = P; m4[i] = Mv; v4[i] = V;
        }
    }
}

struct AdamwRows {
    float r[DCV_ADAMW_MAX_GROUPS * 8];
};

// the rows arrive as the kernel's ARGUMENT (1 KB by value): stream-ordered, no staging buffer
__global__ __launch_bounds__(256) void adamw_hyper_groups_kernel(float* __restrict__ hyper, AdamwRows rows, int n) {
    const int i = threadIdx.x;
    if (i < n) hyper[i] = rows.r[i];
}

}  // namespace

extern "C" int dcv_adamw_set_hyper_groups(float* hyper_dev, const float* rows_host, const int* steps_host, int n_groups, float grad_scale,
                                          void* stream) {
    if (!hyper_dev || !rows_host || !steps_host) return DCV_ERR_NULL;
    if (n_groups < 1 || n_groups > DCV_ADAMW_MAX_GROUPS) return DCV_ERR_SHAPE;
    for (int k = 0; k < n_groups; ++k)
        if (steps_host[k] <= 0) return DCV_ERR_SHAPE;
    AdamwRows rows = {};
    for (int k = 0; k < n_groups; ++k) {
        const float* r = rows_host + 5 * k;
        const double bc1 = 1.0 - pow((double)r[1], steps_host[k]), bc2 = 1.0 - pow((double)r[2], steps_host[k]);
        float* o = rows.r + 8 * k;
        o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; o[3] = r[3]; o[4] = r[4];
        o[5] = (float)(1.0 / bc1); o[6] = (float)(1.0 / sqrt(bc2)); o[7] = grad_scale;
    }
    static_assert(DCV_ADAMW_MAX_GROUPS * 8 <= 256, "one workgroup writes the table");
    hipLaunchKernelGGL(adamw_hyper_groups_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, hyper_dev, rows, n_groups * 8);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

extern "C" int dcv_adamw_groups(float* p, const float* g, float* m, float* v, long n, const int* seg_end4, const int* seg_group, int n_seg,
                                const float* hyper_dev, int n_groups, void* stream) {
    if (!p || !g || !m || !v || !seg_end4 || !seg_group || !hyper_dev) return DCV_ERR_NULL;
    if (n <= 0 || n % 4 || n / 4 > 0x7FFFFFFFL - ADAMW_G_CHUNK4) return DCV_ERR_SHAPE;  // run ends are int32 float4 indices
    if (n_seg < 1 || n_seg > DCV_ADAMW_MAX_SEGS || n_groups < 1 || n_groups > DCV_ADAMW_MAX_GROUPS) return DCV_ERR_SHAPE;
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) return DCV_ERR_ALIGN;
    if (((uintptr_t)seg_end4 | (uintptr_t)seg_group | (uintptr_t)hyper_dev) & 3) return DCV_ERR_ALIGN;
    const long n4 = n / 4;
    long grid = (n4 + ADAMW_G_CHUNK4 - 1) / ADAMW_G_CHUNK4;
    if (grid > ADAMW_G_GRID_CAP) grid = ADAMW_G_GRID_CAP;
    hipLaunchKernelGGL(adamw_groups_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (int)n4, seg_end4, seg_group,
                       n_seg, hyper_dev, n_groups);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}
