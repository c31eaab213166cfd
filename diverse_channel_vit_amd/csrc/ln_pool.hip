// Final LayerNorm of the residual stream pooled per input channel: the reduction behind
// ChannelVisionTransformer.get_intermediate_layers(pool="channel").
//   x f32 [B, N, D], N = 1 + C * n_p (CLS first, then the n_p patch tokens of channel 0, of channel 1, ...)
//   out f32 [B, 1 + C, D]: row 0 = LayerNorm(x[b, 0]); row 1 + c = mean over i < n_p of LayerNorm(x[b, 1 + c * n_p + i])
// The normed tokens ([64, 1569, 384] fp32 = 154 MB at the headline shape) are never written: the kernel reads the stream once and
// writes B (1 + C) D floats.
//
// Per row the statistics are formed exactly as ln_fwd_kernel (norm.hip) forms them: one wave per row, float4 loads, wave_sum of the
// row, then of the centred squares.  LayerNorm's affine is linear in the normalised row, so it commutes with the mean: a segment
// (image, channel) sums x^ = (x - mean) * rstd over its rows and gamma / beta are applied once, to the mean.  The CLS row goes through
// the same expressions as ln_fwd_kernel's fp32 output, so it is bit-identical to dcv_ln_fwd on that row.
//
// Deterministic, no atomics.  A segment's n_p rows are cut into S contiguous splits of R = ceil(n_p / S0) rows, S = ceil(n_p / R), where
// S0 = ceil(TARGET_WGS / (B C)) capped so that a split keeps at least MIN_ROWS rows: one 4-wave workgroup per (segment, split).  Wave w
// adds the rows w, w + 4, w + 8, ... of its split in increasing order; the four wave sums are added in wave order through LDS.  With
// S == 1 the workgroup finishes the segment itself.  With S > 1 (B C segments would not fill the chip: one image, three channels) it
// stores its partial to the workspace and a SECOND, tiny launch adds the S partials of a segment in split order and applies the affine —
// chosen over a last-arriver scheme because it needs no counter to reset and no cross-workgroup ordering.  S, R and every order above
// are functions of (B, C, n_p, D) alone — never of the device's CU count or of the dispatch order — so two calls are bit-identical.
//
// Measured on the MI355X (tools/intermediate_layers_bench.py --variants, profiles/intermediate_layers_bench.txt; medians of 50, candidates
// alternating; an earlier run of the same builds differed by 1-2 us), B 64, n_p 196, D 384: C 8 55.2 us (both launches) against 87.4 us
// for dcv_ln_fwd (fp32 output) + torch.mean and 29.9 us for a copy that moves the same bytes (1.85 x that floor, 2.8 TB/s); C 3
// 30.8 / 41.0 / 12.0 us.  The split plan pays even where B C already covers the CUs: asking for 512 workgroups (DCV_LP_TARGET_WGS=512 —
// whole segments at C 8, no workspace, no second launch) takes 69.2 us at C 8 and 32.3 us at C 3; two workgroups of four waves per CU
// leave too few loads in flight.  A wave keeps ONE row's loads in flight: with two (a retired variant, the same summation order) the
// split plan measured 56.2 vs 55.2 us at C 8 and 31.9 vs 30.8 us at C 3, and the 512-workgroup plan 82.6 vs 69.2 us and 35.4 vs 32.3 us
// — never faster, as ln_fwd_kernel found for its own loop.  LP_MIN_ROWS = 8 has not been varied.  What holds the kernel at 1.85 x the
// copy floor has not been profiled.
#include "dcv_common.hpp"
#include "../../include/dcv.h"
#include "ln_pool_plan.hpp"  // lp_plan, lp_shape_ok and their constants: shared with ln_pool_bwd.hip

namespace {

// Workgroups [0, B C S): one (segment, split) each.  Workgroups from B C S on: four CLS rows each (one per wave).
template <int MAXV>
__global__ __launch_bounds__(256) void ln_pool_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float* __restrict__ out, float* __restrict__ ws,
                                                      int B, int C, int n_p, int D, float eps, int S, int R) {
    __shared__ f32x4 red[3][MAXV][64];  // the sums of waves 1 .. 3
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nv = D >> 2;
    const long N = 1 + (long)C * n_p;
    const int nwork = B * C * S;
    auto load_row = [&](const float* xr, f32x4(&v)[MAXV]) {
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            int c = lane + 64 * i;
            v[i] = (c < nv) ? reinterpret_cast<const f32x4*>(xr)[c] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    // mean and rstd of one row: the expressions of ln_fwd_kernel's finish_row
    auto row_stats = [&](const f32x4(&v)[MAXV], float& mu, float& rs) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) s += v[i].x + v[i].y + v[i].z + v[i].w;
        mu = wave_sum(s) / D;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            int c = lane + 64 * i;
            if (c < nv) {
                float a = v[i].x - mu, b = v[i].y - mu, cc = v[i].z - mu, d = v[i].w - mu;
                q += a * a + b * b + cc * cc + d * d;
            }
        }
        rs = rsqrtf(wave_sum(q) / D + eps);
    };
    if ((int)blockIdx.x >= nwork) {
        // --- CLS rows: plain LayerNorm ---
        const int b = ((int)blockIdx.x - nwork) * 4 + wave;
        if (b >= B) return;
        f32x4 v[MAXV];
        load_row(x + (size_t)b * N * D, v);
        float mu, rs;
        row_stats(v, mu, rs);
        float* o = out + (size_t)b * (1 + C) * D;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            int c = lane + 64 * i;
            if (c < nv) {
                const float4 g = reinterpret_cast<const float4*>(gamma)[c];
                const float4 bb = reinterpret_cast<const float4*>(beta)[c];
                float o0 = (v[i].x - mu) * rs * g.x + bb.x, o1 = (v[i].y - mu) * rs * g.y + bb.y;
                float o2 = (v[i].z - mu) * rs * g.z + bb.z, o3 = (v[i].w - mu) * rs * g.w + bb.w;
                reinterpret_cast<f32x4*>(o)[c] = f32x4{o0, o1, o2, o3};
            }
        }
        return;
    }
    // --- one split of one (image, channel) segment ---
    const int seg = (int)blockIdx.x / S, split = (int)blockIdx.x % S;
    const int b = seg / C, ch = seg % C;
    const int r0 = split * R;
    const int r1 = (r0 + R < n_p) ? r0 + R : n_p;
    const float* xs = x + ((size_t)b * N + 1 + (size_t)ch * n_p) * D;
    f32x4 acc[MAXV];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto add_row = [&](const f32x4(&v)[MAXV]) {
        float mu, rs;
        row_stats(v, mu, rs);
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            // lanes past the row hold zeros in v: their sums are never read
            acc[i].x += (v[i].x - mu) * rs;
            acc[i].y += (v[i].y - mu) * rs;
            acc[i].z += (v[i].z - mu) * rs;
            acc[i].w += (v[i].w - mu) * rs;
        }
    };
    int r = r0 + wave;
    for (; r < r1; r += 4) {
        f32x4 va[MAXV];
        load_row(xs + (size_t)r * D, va);
        add_row(va);
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
        if (S > 1) {
            reinterpret_cast<f32x4*>(ws + (size_t)blockIdx.x * D)[c] = t;
        } else {
            const float inv = 1.0f / (float)n_p;
            const float4 g = reinterpret_cast<const float4*>(gamma)[c];
            const float4 bb = reinterpret_cast<const float4*>(beta)[c];
            reinterpret_cast<f32x4*>(out + ((size_t)b * (1 + C) + 1 + ch) * D)[c] =
                f32x4{t.x * inv * g.x + bb.x, t.y * inv * g.y + bb.y, t.z * inv * g.z + bb.z, t.w * inv * g.w + bb.w};
        }
    }
}

// S > 1: the partials of a segment, added in split order; one thread per (segment, float4 column)
__global__ __launch_bounds__(256) void ln_pool_finish_kernel(const float* __restrict__ ws, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float* __restrict__ out, int B, int C,
                                                             int n_p, int D, int S) {
    const int nv = D >> 2;
    const long total = (long)B * C * nv;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int seg = (int)(t / nv), c = (int)(t % nv);
    const int b = seg / C, ch = seg % C;
    const f32x4* p = reinterpret_cast<const f32x4*>(ws + (size_t)seg * S * D) + c;
    f32x4 s = p[0];
    for (int k = 1; k < S; ++k) {
        const f32x4 q = p[(size_t)k * nv];
        s.x += q.x; s.y += q.y; s.z += q.z; s.w += q.w;
    }
    const float inv = 1.0f / (float)n_p;
    const float4 g = reinterpret_cast<const float4*>(gamma)[c];
    const float4 bb = reinterpret_cast<const float4*>(beta)[c];
    reinterpret_cast<f32x4*>(out + ((size_t)b * (1 + C) + 1 + ch) * D)[c] =
        f32x4{s.x * inv * g.x + bb.x, s.y * inv * g.y + bb.y, s.z * inv * g.z + bb.z, s.w * inv * g.w + bb.w};
}

}  // namespace

extern "C" long dcv_ln_pool_channels_ws_floats(int B, int C, int n_p, int D) {
    if (!lp_shape_ok(B, C, n_p, D)) return DCV_ERR_SHAPE;
    const LpPlan p = lp_plan(B, C, n_p);
    return p.S > 1 ? (long)B * C * p.S * D : 0;
}

extern "C" int dcv_ln_pool_channels(const float* x, const float* gamma, const float* beta, float eps, float* out, int B, int C, int n_p,
                                    int D, float* ws, long ws_floats, void* stream) {
    if (!x || !gamma || !beta || !out) return DCV_ERR_NULL;
    if (!lp_shape_ok(B, C, n_p, D)) return DCV_ERR_SHAPE;
    if (((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out | (uintptr_t)ws) & 15) return DCV_ERR_ALIGN;
    const LpPlan p = lp_plan(B, C, n_p);
    const long need = p.S > 1 ? (long)B * C * p.S * D : 0;
    if (need > 0 && !ws) return DCV_ERR_NULL;
    if (ws_floats < need) return DCV_ERR_SHAPE;
    const long nwork = (long)B * C * p.S;
    const long grid = nwork + (B + 3) / 4;
    if (grid > 0x7fffffffL) return DCV_ERR_SHAPE;
    if (D <= 512)
        hipLaunchKernelGGL(ln_pool_kernel<2>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, out, ws, B, C, n_p, D,
                           eps, p.S, p.R);
    else
        hipLaunchKernelGGL(ln_pool_kernel<4>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, out, ws, B, C, n_p, D,
                           eps, p.S, p.R);
    DCV_LAUNCH_CHECK();
    if (p.S > 1) {
        const long total = (long)B * C * (D >> 2);
        hipLaunchKernelGGL(ln_pool_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ws, gamma, beta, out,
                           B, C, n_p, D, p.S);
        DCV_LAUNCH_CHECK();
    }
    return DCV_OK;
}
