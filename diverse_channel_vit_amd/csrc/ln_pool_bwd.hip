// Adjoint of dcv_ln_pool_channels (ln_pool.hip): the gradient of a channel-pooled feature tap (DiChaViT.forward_with_features,
// pool="channel") added to the fp32 gradient of the residual stream, with the final norm's dgamma / dbeta.
//   x f32 [B, N, D], N = 1 + C * n_p;  dout f32 [B, 1 + C, D];  dx f32 [B, N, D], ACCUMULATED in place;  dgamma, dbeta f32 [D], accumulated.
// With g = dout[b, 1 + c], h = gamma * g / n_p (one vector per segment) and x^_i = (x_i - mu_i) rstd_i for row i of segment (b, c):
//   dx_i   += rstd_i (h - mean_D(h) - x^_i mean_D(h x^_i))          the CLS row: the same with n_p = 1 and g = dout[b, 0]
//   dgamma += sum_b dout[b, 0] x^_cls + sum_{b,c} dout[b, 1 + c] (1 / n_p) sum_i x^_i
//   dbeta  += sum_{b,j} dout[b, j]
// ONE pass: x is read once, dx read and written once.  A row's du (the broadcast of g / n_p) never exists in memory: h lives in the registers of
// the wave for the whole segment.  mu and rstd are not arguments: they are recomputed from the row with the expressions of
// ln_fwd_kernel (norm.hip) and ln_pool_kernel — one wave per row, float4 loads, wave_sum of the row, then of the centred squares — so that x^ is
// meant to be the forward's.  The expressions are the same; that the compiler contracts them the same way in both translation units
// (-ffp-contract=fast) is not tested: no entry returns the recomputed statistics.
//
// PLAN (lp_plan of ln_pool_plan.hpp, a host function of (B, C, n_p) alone: the forward kernel's own cut): a segment's n_p rows are cut into S contiguous
// splits of R = ceil(n_p / S0) rows, S = ceil(n_p / R), S0 = ceil(2048 / (B C)) capped so that a split keeps at least 8 rows.  Workgroups
// [0, B C S): one (segment, split) each, four waves; wave w owns rows w, w + 4, w + 8, ... of its split.  Workgroups [B C S, B C S + ceil(B / 4)):
// four CLS rows each, one per wave.  G = B C S + ceil(B / 4) workgroups in all.
// Deterministic, no atomics.  Every row of dx is read and written by exactly one wave.  A wave adds the x^ of its rows in increasing row order;
// the four wave sums are added in wave order through LDS, multiplied by g / n_p and stored as the workgroup's dgamma partial to ws[wg][D].  A
// second, tiny launch (det_reduce) adds the G partials to dgamma in workgroup order; a third adds the B (1 + C) rows of dout to dbeta in row
// order — dout itself is the table of partials.  Every order is a function of (B, C, n_p, D): two calls are bit-identical.
// Workspace: G * D floats (dcv_ln_pool_channels_bwd_ws_floats); not read when dgamma is NULL.  dgamma NULL / dbeta NULL: that sum is skipped and
// dx has the same bits.
//
// Measured on the MI355X (tools/feature_taps_bench.py, profiles/feature_taps_bench.txt; medians of 50, candidates alternating, three repeats
// that differed by at most 1.2 us for the kernel and 2.2 us for the composite), B 64, n_p 196, D 384, all three launches: C 8 133.8 us against
// 223.1 us for what it replaces (torch materialises the broadcast du in fp32, dcv_ln_fwd for the statistics, dcv_ln_bwd with f32 du into dx) and
// 97.0 us for a device copy that moves 3 B N D 4 bytes (1.38 x that floor, 3.5 TB/s); C 3 61.2 / 98.7 / 36.9 us (1.66 x).  Nothing of the plan
// has been varied: the workgroup target and the row minimum are ln_pool.hip's, a wave keeps one row's two loads (x, dx) in flight, and how
// much of the time the two reduction launches take was not measured apart.
#include "dcv_common.hpp"
#include "../../include/dcv.h"
#include "ln_pool_plan.hpp"  // lp_plan, lp_shape_ok: the forward kernel's own

namespace {

template <int MAXV>
__global__ __launch_bounds__(256) void ln_pool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                          const float* __restrict__ dout, float* dx, float* __restrict__ part, int B, int C,
                                                          int n_p, int D, float eps, int S, int R) {
    __shared__ f32x4 red[3][MAXV][64];  // the x^ sums of waves 1 .. 3
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nv = D >> 2;
    const long N = 1 + (long)C * n_p;
    const int nwork = B * C * S;
    const bool cls = (int)blockIdx.x >= nwork;
    int b, j;          // image, row of dout
    long row0;         // first row (inside the image) of this workgroup's rows
    int nrows;         // rows of this workgroup; wave w takes w, w + 4, ...
    float inv;
    if (cls) {
        const int b0 = ((int)blockIdx.x - nwork) * 4;
        b = b0 + wave;  // one CLS row per wave
        j = 0;
        row0 = 0;
        nrows = 0;  // set below per wave
        inv = 1.0f;
    } else {
        const int seg = (int)blockIdx.x / S, split = (int)blockIdx.x % S;
        b = seg / C;
        const int ch = seg % C;
        j = 1 + ch;
        const int r0 = split * R;
        const int r1 = (r0 + R < n_p) ? r0 + R : n_p;
        row0 = 1 + (long)ch * n_p + r0;
        nrows = r1 - r0;
        inv = 1.0f / (float)n_p;
    }
    const bool live = b < B;  // CLS workgroups: the last one may hold fewer than four images
    // h = gamma * g / n_p and its mean over D, once per wave
    f32x4 gq[MAXV], h[MAXV], acc[MAXV];
    float s1 = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = lane + 64 * i;
        gq[i] = h[i] = acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < nv && live) {
            const f32x4 g = reinterpret_cast<const f32x4*>(dout + ((size_t)b * (1 + C) + j) * D)[c];
            const float4 gm = reinterpret_cast<const float4*>(gamma)[c];
            gq[i] = f32x4{g.x * inv, g.y * inv, g.z * inv, g.w * inv};
            h[i] = f32x4{gm.x * gq[i].x, gm.y * gq[i].y, gm.z * gq[i].z, gm.w * gq[i].w};
            s1 += h[i].x + h[i].y + h[i].z + h[i].w;
        }
    }
    const float m1 = wave_sum(s1) / D;
    auto do_row = [&](long row) {
        const size_t off = ((size_t)b * N + row) * D;
        const f32x4* xr = reinterpret_cast<const f32x4*>(x + off);
        f32x4* dr = reinterpret_cast<f32x4*>(dx + off);
        f32x4 v[MAXV], d[MAXV];
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = lane + 64 * i;
            v[i] = d[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (c < nv) {
                v[i] = xr[c];
                d[i] = dr[c];
            }
        }
        // mean and rstd: the expressions of ln_fwd_kernel's finish_row and ln_pool_kernel's row_stats
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) s += v[i].x + v[i].y + v[i].z + v[i].w;
        const float mu = wave_sum(s) / D;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = lane + 64 * i;
            if (c < nv) {
                float a = v[i].x - mu, bb = v[i].y - mu, cc = v[i].z - mu, dd = v[i].w - mu;
                q += a * a + bb * bb + cc * cc + dd * dd;
            }
        }
        const float rs = rsqrtf(wave_sum(q) / D + eps);
        float s2 = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            // lanes past the row hold zeros in h: they add nothing; their x^ sums are never read
            v[i] = f32x4{(v[i].x - mu) * rs, (v[i].y - mu) * rs, (v[i].z - mu) * rs, (v[i].w - mu) * rs};
            s2 += h[i].x * v[i].x + h[i].y * v[i].y + h[i].z * v[i].z + h[i].w * v[i].w;
            acc[i].x += v[i].x; acc[i].y += v[i].y; acc[i].z += v[i].z; acc[i].w += v[i].w;
        }
        const float m2 = wave_sum(s2) / D;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = lane + 64 * i;
            if (c < nv)
                dr[c] = f32x4{d[i].x + rs * (h[i].x - m1 - v[i].x * m2), d[i].y + rs * (h[i].y - m1 - v[i].y * m2),
                              d[i].z + rs * (h[i].z - m1 - v[i].z * m2), d[i].w + rs * (h[i].w - m1 - v[i].w * m2)};
        }
    };
    if (cls) {
        if (live) do_row(0);
    } else {
        for (int r = wave; r < nrows; r += 4) do_row(row0 + r);
    }
    if (!part) return;  // uniform: no dgamma asked for
    // the workgroup's dgamma partial.  Patch segments: (g / n_p) * (sum of the four waves' x^ sums, in wave order).  CLS workgroups: the sum
    // over its (up to four) images of dout[b, 0] * x^_cls, in image order.
    if (cls) {
#pragma unroll
        for (int i = 0; i < MAXV; ++i)
            acc[i] = f32x4{gq[i].x * acc[i].x, gq[i].y * acc[i].y, gq[i].z * acc[i].z, gq[i].w * acc[i].w};
    }
    if (wave > 0) {
#pragma unroll
        for (int i = 0; i < MAXV; ++i) red[wave - 1][i][lane] = acc[i];
    }
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = lane + 64 * i;
        if (c >= nv) continue;
        f32x4 t = acc[i];
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            const f32x4 p = red[w][i][lane];
            t.x += p.x; t.y += p.y; t.z += p.z; t.w += p.w;
        }
        if (!cls) t = f32x4{gq[i].x * t.x, gq[i].y * t.y, gq[i].z * t.z, gq[i].w * t.w};
        reinterpret_cast<f32x4*>(part + (size_t)blockIdx.x * D)[c] = t;
    }
}

inline long lpb_workgroups(int B, int C, int n_p) { return (long)B * C * lp_plan(B, C, n_p).S + (B + 3) / 4; }

}  // namespace

extern "C" long dcv_ln_pool_channels_bwd_ws_floats(int B, int C, int n_p, int D) {
    if (!lp_shape_ok(B, C, n_p, D)) return DCV_ERR_SHAPE;
    return lpb_workgroups(B, C, n_p) * D;
}

extern "C" int dcv_ln_pool_channels_bwd(const float* x, const float* gamma, float eps, const float* dout, float* dx, float* dgamma,
                                        float* dbeta, int B, int C, int n_p, int D, float* ws, long ws_floats, void* stream) {
    if (!x || !gamma || !dout || !dx) return DCV_ERR_NULL;
    if (!lp_shape_ok(B, C, n_p, D)) return DCV_ERR_SHAPE;
    if (((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)dout | (uintptr_t)dx | (uintptr_t)dgamma | (uintptr_t)dbeta | (uintptr_t)ws) & 15)
        return DCV_ERR_ALIGN;
    const LpPlan p = lp_plan(B, C, n_p);
    const long grid = lpb_workgroups(B, C, n_p);
    if (grid > 0x7fffffffL) return DCV_ERR_SHAPE;
    const long need = dgamma ? grid * D : 0;
    if (need > 0 && !ws) return DCV_ERR_NULL;
    if (ws_floats < need) return DCV_ERR_SHAPE;
    float* part = dgamma ? ws : nullptr;
    if (D <= 512)
        hipLaunchKernelGGL(ln_pool_bwd_kernel<2>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, x, gamma, dout, dx, part, B, C, n_p, D,
                           eps, p.S, p.R);
    else
        hipLaunchKernelGGL(ln_pool_bwd_kernel<4>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, x, gamma, dout, dx, part, B, C, n_p, D,
                           eps, p.S, p.R);
    DCV_LAUNCH_CHECK();
    if (dgamma && !det_reduce(ws, (int)grid, D, dgamma, D, D, D, nullptr, 0, (hipStream_t)stream)) return DCV_ERR_LAUNCH;
    if (dbeta && !det_reduce(dout, B * (1 + C), D, dbeta, D, D, D, nullptr, 0, (hipStream_t)stream)) return DCV_ERR_LAUNCH;
    return DCV_OK;
}
