// Train-time image augmentation of the reference's CHAMMI recipe on the device (datasets/dataset_utils.py:234-243): a thin-plate-spline warp
// (datasets/tps_transform.py:22-134) and torchvision's resized crop + horizontal flip, one launch each.  Both are gather kernels: no MFMA, no
// atomics, no scratch; every sum has a fixed order, so two launches on the same inputs agree bit for bit.
//
// dcv_tps_warp, per flagged sample (a workgroup of an unflagged sample returns at once; its slab of `out` is not touched):
//   a. the COARSE grid of n x n points, n = int((W - 1) / 10), at k (W - 1) / (n - 1) on both axes: f = a1 + ax x + ay y + sum_i w_i U(r_i),
//      U(r) = r^2 ln r, in fp64, kept as fp32 in LDS.  A workgroup evaluates only the TPS_CROWS coarse rows its TPS_ROWS image rows read.
//   b. the reference's upsampling rule, quirk included: pos = (steps - 1) i / (W - 1) with the FLOAT steps = (W - 1) / 10, upper index
//      min(idx + 1, int(steps - 1)).  pos and its fraction in fp64 (the operations numpy performs, in its order), the blend in fp32.
//   c. a bilinear sample at the (axis 0, axis 1) coordinate with scipy's mode="reflect" (half-sample symmetric, period 2 W): taps floor(c) and
//      floor(c) + 1, each folded.  The coordinate is computed once per pixel and shared by the C channels.
// dcv_crop_resize_flip: torch's antialiased bilinear resize (the triangle filter over max(scale, 1) input pixels, fp32 centres and weights as
// ATen computes them) of the box (i, j, h, w) of every sample to S x S, the output column mirrored where flip is set.  A thread owns one output
// column of CRF_ROWS output rows: it filters each input row of the tile horizontally and adds it into the rows' accumulators with the
// vertical weights, which sit in LDS as one row of CRF_ROWS weights per input row.  Both axes in one pass, nothing staged but those weights.
#include "dcv_common.hpp"

namespace {

// Image rows per workgroup.  Measured at B 64 (profiles/device_augment_bench.txt, stand-alone builds with -DDCV_TPS_ROWS=n): with every sample warped
// 1 / 2 / 4 / 8 rows took 108 / 106 / 106 / 103 us at 8 x 224^2 and 313 / 223 / 203 / 223 us at 4 x 512^2; with one sample in five warped, the recipe's
// case, 33 / 39 / 48 / 63 us and 62 / 53 / 61 / 77 us (each figure includes the 13-16 us that the events around an empty launch cost): few
// workgroups are then in flight and short ones fill the chip.  2 is chosen for the recipe's case; with every sample warped it costs 9 us
// against 8 rows at 5 x 160^2 (42 against 33) and nothing at the other two shapes.
#ifndef DCV_TPS_ROWS
#define DCV_TPS_ROWS 2
#endif
constexpr int TPS_ROWS = DCV_TPS_ROWS;
constexpr int TPS_CROWS = TPS_ROWS / 10 + 3;    // coarse rows they can read: pos advances by < 0.1 per row -> at most 2 lower indices, + 1 upper
constexpr int TPS_MAXW = 1024;
constexpr int TPS_MAXN = (TPS_MAXW - 1) / 10;   // 102 coarse points per axis
constexpr int TPS_MAXK = 32;

__device__ __forceinline__ float px_load(const uint8_t* p, int i) { return (float)p[i]; }
__device__ __forceinline__ float px_load(const float* p, int i) { return p[i]; }

// scipy's "reflect": ... 1 0 | 0 1 ... W-1 | W-1 W-2 ...   (any distance; the result is always inside [0, W))
__device__ __forceinline__ int fold_reflect(int i, int W) {
    const int P = 2 * W;
    int m = i % P;
    if (m < 0) m += P;
    return m < W ? m : P - 1 - m;
}

// the reference's position of pixel i on the coarse grid: numpy's ((steps - 1) * i) / (W - 1) and modf, in fp64
__device__ __forceinline__ void tps_pos(int i, int W, int* idx, float* frac) {
    const double steps = (double)(W - 1) / 10.0;
    const double pos = ((steps - 1.0) * (double)i) / (double)(W - 1);
    const int k = (int)pos;
    *idx = k;
    *frac = (float)(pos - (double)k);
}

template <typename T>
__global__ __launch_bounds__(256) void tps_warp_kernel(const T* __restrict__ x, const double* __restrict__ P, const double* __restrict__ coef,
                                                       const int* __restrict__ apply, float* __restrict__ out, int C, int W, int K) {
    const int b = blockIdx.y;
    if (!apply[b]) return;
    __shared__ float s_grid[2][TPS_CROWS][TPS_MAXN];
    __shared__ float s_cfrac[TPS_MAXW];
    __shared__ short s_cidx[TPS_MAXW];
    __shared__ float s_rfrac[TPS_ROWS];
    __shared__ int s_ridx[TPS_ROWS];
    __shared__ double s_P[TPS_MAXK][2];
    __shared__ double s_w[2][TPS_MAXK + 3];

    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * TPS_ROWS;
    const int nrows = min(TPS_ROWS, W - r0);
    const int n = (W - 1) / 10;
    const int cap = (int)((double)(W - 1) / 10.0 - 1.0);  // int(steps - 1)

    for (int i = tid; i < 2 * K; i += 256) s_P[i >> 1][i & 1] = P[(size_t)b * 2 * K + i];
    for (int i = tid; i < 2 * (K + 3); i += 256) s_w[i / (K + 3)][i % (K + 3)] = coef[(size_t)b * 2 * (K + 3) + i];
    for (int j = tid; j < W; j += 256) {
        int k;
        float f;
        tps_pos(j, W, &k, &f);
        s_cidx[j] = (short)k;
        s_cfrac[j] = f;
    }
    if (tid < nrows) tps_pos(r0 + tid, W, &s_ridx[tid], &s_rfrac[tid]);
    int lo, lo_last;
    float fr;
    tps_pos(r0, W, &lo, &fr);
    tps_pos(r0 + nrows - 1, W, &lo_last, &fr);
    const int ncr = min(min(lo_last + 1, cap) - lo + 1, TPS_CROWS);  // coarse rows lo .. lo + ncr - 1
    __syncthreads();

    // a. coarse points (lo + cr, cc): four lanes per point, lane q takes the terms q, q + 4, ...; the four partial sums meet in a fixed order
    const double gstep = (double)(W - 1) / (double)(n - 1);  // numpy's mgrid[0 : W - 1 : n j]: point k sits at k * step
    for (int item = tid; item < ncr * n * 4; item += 256) {
        const int pt = item >> 2, q = item & 3;
        const int cr = pt / n, cc = pt - cr * n;
        const double gx = (double)(lo + cr) * gstep, gy = (double)cc * gstep;
        double s0 = 0.0, s1 = 0.0;
        for (int k = q; k < K; k += 4) {
            const double dx = s_P[k][0] - gx, dy = s_P[k][1] - gy;
            const double r2 = dx * dx + dy * dy;
            const double u = r2 < 1e-200 ? 0.0 : r2 * (0.5 * log(r2));
            s0 += s_w[0][k] * u;
            s1 += s_w[1][k] * u;
        }
        s0 += __shfl_xor(s0, 1, 64);
        s1 += __shfl_xor(s1, 1, 64);
        s0 += __shfl_xor(s0, 2, 64);
        s1 += __shfl_xor(s1, 2, 64);
        if (q == 0) {
            s_grid[0][cr][cc] = (float)(s_w[0][K] + s_w[0][K + 1] * gx + s_w[0][K + 2] * gy + s0);
            s_grid[1][cr][cc] = (float)(s_w[1][K] + s_w[1][K + 1] * gx + s_w[1][K + 2] * gy + s1);
        }
    }
    __syncthreads();

    // b + c. one pixel per lane, the channels in a loop
    const int plane = W * W;
    const T* __restrict__ xb = x + (size_t)b * C * plane;
    float* __restrict__ ob = out + (size_t)b * C * plane;
    for (int px = tid; px < nrows * W; px += 256) {
        const int rr = px / W, col = px - rr * W;
        const int row = r0 + rr;
        const int ri = s_ridx[rr];
        const float rf = s_rfrac[rr];
        const int ci = s_cidx[col];
        const float cf = s_cfrac[col];
        const int a0 = min(ri - lo, TPS_CROWS - 1), a1 = min(min(ri + 1, cap) - lo, TPS_CROWS - 1);
        const int c0 = ci, c1 = min(ci + 1, cap);
        const float x1 = 1.f - rf, y1 = 1.f - cf;
        const float w00 = x1 * y1, w01 = x1 * cf, w10 = rf * y1, w11 = rf * cf;
        float cx = fmaf(s_grid[0][a1][c1], w11, fmaf(s_grid[0][a1][c0], w10, fmaf(s_grid[0][a0][c1], w01, s_grid[0][a0][c0] * w00)));
        float cy = fmaf(s_grid[1][a1][c1], w11, fmaf(s_grid[1][a1][c0], w10, fmaf(s_grid[1][a0][c1], w01, s_grid[1][a0][c0] * w00)));
        // out of any sensible range (or NaN, which fmaxf / fminf drop): still an index that folds inside the image
        cx = fminf(fmaxf(cx, -1e9f), 1e9f);
        cy = fminf(fmaxf(cy, -1e9f), 1e9f);
        const float flx = floorf(cx), fly = floorf(cy);
        const float fx = cx - flx, fy = cy - fly;
        const int ix = (int)flx, iy = (int)fly;
        const int rx0 = fold_reflect(ix, W) * W, rx1 = fold_reflect(ix + 1, W) * W;
        const int ry0 = fold_reflect(iy, W), ry1 = fold_reflect(iy + 1, W);
        const float gx = 1.f - fx, gy = 1.f - fy;
        const int o = row * W + col;
#pragma unroll 4
        for (int c = 0; c < C; ++c) {
            const T* __restrict__ xc = xb + (size_t)c * plane;
            const float v00 = px_load(xc, rx0 + ry0), v01 = px_load(xc, rx0 + ry1);
            const float v10 = px_load(xc, rx1 + ry0), v11 = px_load(xc, rx1 + ry1);
            // the contraction written out: uint8 and float32 images of the same values give the same bits
            ob[(size_t)c * plane + o] = fmaf(fx, fmaf(fy, v11, gy * v10), gx * fmaf(fy, v01, gy * v00));
        }
    }
}

constexpr int CRF_ROWS = 8;    // output rows per workgroup: one accumulator each per lane
constexpr int CRF_MAXT = 17;   // taps per axis at scale <= 8: int(c + 8.5) - int(c - 7.5) = 16, one more for an fp32 centre on a boundary

// ATen's antialias index / weight rule for one output position: taps [lo, lo + cnt), weight k = max(0, 1 - |(lo + k - center + 0.5) invs|) / total
struct AaTaps {
    int lo, cnt;
    float center, invs, inv_total;
};
__device__ __forceinline__ float aa_raw(const AaTaps& t, int k) { return fmaxf(0.f, 1.f - fabsf(((float)(t.lo + k) - t.center + 0.5f) * t.invs)); }
__device__ __forceinline__ AaTaps aa_taps(int o, int n_in, float scale) {
    AaTaps t;
    const float support = fmaxf(scale, 1.f);
    t.invs = scale >= 1.f ? 1.f / scale : 1.f;
    t.center = scale * ((float)o + 0.5f);
    t.lo = max((int)(t.center - support + 0.5f), 0);
    t.cnt = min(min((int)(t.center + support + 0.5f), n_in) - t.lo, CRF_MAXT);
    float total = 0.f;
    for (int k = 0; k < t.cnt; ++k) total += aa_raw(t, k);
    t.inv_total = total != 0.f ? 1.f / total : 0.f;
    return t;
}

constexpr int CRF_UNROLL = 4;  // input rows in flight per lane
// input rows one tile can read at scale <= 8: its first taps move by at most 8 (+ 1 for the truncation) per output row, the last row adds its taps
constexpr int CRF_MAXROWS = (CRF_ROWS - 1) * 9 + CRF_MAXT;

// One output column of CRF_ROWS output rows.  s_wt[y - y_lo][r] is the vertical weight of input row y in output row r (0 outside r's taps), so
// a row costs two broadcast LDS reads and CRF_ROWS fmas; CRF_UNROLL rows are filtered together, their loads independent of each other.
template <typename T>
__device__ __forceinline__ void crf_tile(const T* __restrict__ src, int ld, float* __restrict__ dst, int S, int oy0, int oxw, int nrows, const AaTaps& tx,
                                         const float4 (*s_wt)[2]) {
    float acc[CRF_ROWS];
#pragma unroll
    for (int r = 0; r < CRF_ROWS; ++r) acc[r] = 0.f;
    for (int y = 0; y < nrows; y += CRF_UNROLL) {
        const T* __restrict__ row[CRF_UNROLL];
        float h[CRF_UNROLL];
#pragma unroll
        for (int u = 0; u < CRF_UNROLL; ++u) {
            row[u] = src + (size_t)min(y + u, nrows - 1) * ld + tx.lo;  // past the tile: a row that is there, its sum dropped below
            h[u] = 0.f;
        }
        for (int k = 0; k < tx.cnt; ++k) {
            const float w = aa_raw(tx, k) * tx.inv_total;
#pragma unroll
            for (int u = 0; u < CRF_UNROLL; ++u) h[u] = fmaf(w, px_load(row[u], k), h[u]);
        }
#pragma unroll
        for (int u = 0; u < CRF_UNROLL; ++u) {
            if (y + u < nrows) {
                const float4 wa = s_wt[y + u][0], wb = s_wt[y + u][1];
                acc[0] = fmaf(wa.x, h[u], acc[0]);
                acc[1] = fmaf(wa.y, h[u], acc[1]);
                acc[2] = fmaf(wa.z, h[u], acc[2]);
                acc[3] = fmaf(wa.w, h[u], acc[3]);
                acc[4] = fmaf(wb.x, h[u], acc[4]);
                acc[5] = fmaf(wb.y, h[u], acc[5]);
                acc[6] = fmaf(wb.z, h[u], acc[6]);
                acc[7] = fmaf(wb.w, h[u], acc[7]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < CRF_ROWS; ++r)
        if (oy0 + r < S) dst[(size_t)(oy0 + r) * S + oxw] = acc[r];
}
static_assert(CRF_ROWS == 8, "crf_tile spells out its eight accumulators");

template <typename T>
__global__ __launch_bounds__(256) void crop_resize_flip_kernel(const T* __restrict__ x, const float* __restrict__ warped, const int* __restrict__ use_warped,
                                                               const int* __restrict__ box, const int* __restrict__ flip, float* __restrict__ out, int C,
                                                               int H, int W, int S, int xchunks) {
    __shared__ float4 s_wt[CRF_MAXROWS][2];
    const int b = blockIdx.z, c = blockIdx.y;
    const int oy0 = (blockIdx.x / xchunks) * CRF_ROWS;
    const int ox = (blockIdx.x % xchunks) * 256 + threadIdx.x;
    // a box that leaves the image is cut to it: whatever the table holds, nothing outside the sample is read
    const int bi = min(max(box[4 * b + 0], 0), H - 1), bj = min(max(box[4 * b + 1], 0), W - 1);
    const int bh = min(max(box[4 * b + 2], 1), H - bi), bw = min(max(box[4 * b + 3], 1), W - bj);
    const float sy = (float)bh / (float)S, sx = (float)bw / (float)S;
    // the tile's input rows [y_lo, y_hi): the first tap of its first output row to the last tap of its last one (both are monotone in the row)
    const int rlast = min(CRF_ROWS, S - oy0) - 1;
    const AaTaps t0 = aa_taps(oy0, bh, sy), t1 = aa_taps(oy0 + rlast, bh, sy);
    const int y_lo = t0.lo;
    const int nrows = min(t1.lo + t1.cnt - y_lo, CRF_MAXROWS);  // more only at a scale above 8, which the caller refuses
    float* wt = reinterpret_cast<float*>(s_wt);
    for (int i = threadIdx.x; i < nrows * CRF_ROWS; i += 256) wt[i] = 0.f;
    __syncthreads();
    if (threadIdx.x <= rlast) {
        const int r = threadIdx.x;
        const AaTaps t = aa_taps(oy0 + r, bh, sy);
        for (int k = 0; k < t.cnt; ++k)
            if (t.lo - y_lo + k < nrows) wt[(t.lo - y_lo + k) * CRF_ROWS + r] = aa_raw(t, k) * t.inv_total;
    }
    __syncthreads();
    if (ox >= S) return;
    const AaTaps tx = aa_taps(ox, bw, sx);
    const int oxw = flip[b] ? S - 1 - ox : ox;
    const size_t plane = (size_t)H * W, img = ((size_t)b * C + c) * plane + (size_t)(bi + y_lo) * W + bj;
    float* __restrict__ dst = out + ((size_t)b * C + c) * S * S;
    if (warped && use_warped[b]) crf_tile<float>(warped + img, W, dst, S, oy0, oxw, nrows, tx, s_wt);
    else crf_tile<T>(x + img, W, dst, S, oy0, oxw, nrows, tx, s_wt);
}

}  // namespace

extern "C" int dcv_tps_warp(const void* x, int x_is_u8, const double* P, const double* coef, const int* apply, float* out, int B, int C, int W,
                            int K, void* stream) {
    if (!x || !P || !coef || !apply || !out) return DCV_ERR_NULL;
    if (B < 0 || C < 1 || K < 1) return DCV_ERR_SHAPE;
    if (W < 21 || W > TPS_MAXW || K > TPS_MAXK || B > 65535) return DCV_ERR_UNSUPPORTED;
    if ((long)C * W * W > 0x7fffffffL) return DCV_ERR_UNSUPPORTED;  // 32-bit offsets inside a sample
    if (((uintptr_t)P | (uintptr_t)coef) & 7) return DCV_ERR_ALIGN;
    if (((uintptr_t)apply | (uintptr_t)out | (x_is_u8 ? 0 : (uintptr_t)x)) & 3) return DCV_ERR_ALIGN;
    if (B == 0) return DCV_OK;
    const dim3 grid((unsigned)((W + TPS_ROWS - 1) / TPS_ROWS), (unsigned)B);
    if (x_is_u8)
        hipLaunchKernelGGL(tps_warp_kernel<uint8_t>, grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)x, P, coef, apply, out, C, W, K);
    else
        hipLaunchKernelGGL(tps_warp_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)x, P, coef, apply, out, C, W, K);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

extern "C" int dcv_crop_resize_flip(const void* x, int x_is_u8, const float* warped, const int* use_warped, const int* box, const int* flip,
                                    float* out, int B, int C, int H, int W, int S, void* stream) {
    if (!x || (warped && !use_warped) || !box || !flip || !out) return DCV_ERR_NULL;  // warped NULL: every sample is read from x
    if (B < 0 || C < 1 || H < 1 || W < 1 || S < 1) return DCV_ERR_SHAPE;
    if (B > 65535 || C > 65535 || H > 32768 || W > 32768 || S > 32768) return DCV_ERR_UNSUPPORTED;
    if (((uintptr_t)warped | (uintptr_t)use_warped | (uintptr_t)box | (uintptr_t)flip | (uintptr_t)out | (x_is_u8 ? 0 : (uintptr_t)x)) & 3)
        return DCV_ERR_ALIGN;
    if (B == 0) return DCV_OK;
    const int xchunks = (S + 255) / 256;
    const dim3 grid((unsigned)(((S + CRF_ROWS - 1) / CRF_ROWS) * xchunks), (unsigned)C, (unsigned)B);
    if (x_is_u8)
        hipLaunchKernelGGL(crop_resize_flip_kernel<uint8_t>, grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)x, warped, use_warped, box, flip,
                           out, C, H, W, S, xchunks);
    else
        hipLaunchKernelGGL(crop_resize_flip_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)x, warped, use_warped, box, flip, out,
                           C, H, W, S, xchunks);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}
