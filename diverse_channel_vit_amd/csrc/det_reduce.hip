// The deterministic-mode reduction of libdcv_hip.so (gfx950): its kernels and the launchers det_reduce() / det_reduce_multi() that
// gemm_tn.hip, norm.hip, optim.hip and tokenizer.hip call (declared in dcv_common.hpp).  Compiled here once; the kernels stay `static`
// so that a profile names them as it always did.
#include "dcv_common.hpp"

// ---- deterministic mode (the reference trains with cudnn.deterministic = True, utils.py:394-401) -------------------------------
// Kernels that combine partial sums of several workgroups have a second form that STORES the partials to a caller-supplied
// workspace instead of adding them atomically; this kernel then adds them to the destination in index order — a fixed summation
// order whatever the dispatch order was, so two runs on the same inputs are bit-identical.  Column c of a part goes to
// dstA[(c / QA) * ldA + c % QA] for c < nA and to dstB[c - nA] for nA <= c < nA + nB.  VEC: four columns per thread (all of nA, QA,
// ldA, nB, part_stride multiples of 4 and 16-byte aligned pointers).
template <bool VEC>
static __global__ __launch_bounds__(256) void det_reduce_kernel(const float* __restrict__ part, int nparts, long part_stride,
                                                                float* __restrict__ dstA, long nA, int QA, long ldA,
                                                                float* __restrict__ dstB, long nB) {
    constexpr int W = VEC ? 4 : 1;
    const long nv = (nA + nB) / W;
    for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < nv; v += (long)gridDim.x * 256) {
        const long c = v * W;
        float s[W];
#pragma unroll
        for (int e = 0; e < W; ++e) s[e] = 0.f;
        const float* src = part + c;
        int k = 0;
        // eight parts' loads in flight, added in part order (a thread walking its parts one load at a time ran at ~2 TB/s)
        for (; k + 8 <= nparts; k += 8) {
            if constexpr (VEC) {
                float4 t[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) t[j] = *reinterpret_cast<const float4*>(src + (size_t)(k + j) * part_stride);
#pragma unroll
                for (int j = 0; j < 8; ++j) { s[0] += t[j].x; s[1] += t[j].y; s[2] += t[j].z; s[3] += t[j].w; }
            } else {
                float t[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) t[j] = src[(size_t)(k + j) * part_stride];
#pragma unroll
                for (int j = 0; j < 8; ++j) s[0] += t[j];
            }
        }
        for (; k < nparts; ++k) {
            if constexpr (VEC) {
                const float4 t = *reinterpret_cast<const float4*>(src + (size_t)k * part_stride);
                s[0] += t.x; s[1] += t.y; s[2] += t.z; s[3] += t.w;
            } else {
                s[0] += src[(size_t)k * part_stride];
            }
        }
        float* d = (c < nA) ? dstA + (c / QA) * ldA + (c % QA) : dstB + (c - nA);
#pragma unroll
        for (int e = 0; e < W; ++e) d[e] += s[e];
    }
}
// Same sum for MANY parts of FEW columns (LayerNorm: 1024 parts x 768 columns; one thread per column group would walk all parts alone):
// a workgroup owns 4 column groups; part lane pl = thread / 4 adds parts pl, pl + 64, pl + 128, ... in increasing order (eight loads in flight),
// the 64 lane sums are then added in lane order by the threads of lane 0.  The association order is fixed by (nparts) alone: deterministic.
constexpr int DET_TALL_CG = 4, DET_TALL_PL = 256 / DET_TALL_CG;
template <bool VEC>
static __global__ __launch_bounds__(256) void det_reduce_tall_kernel(const float* __restrict__ part, int nparts, long part_stride,
                                                                     float* __restrict__ dstA, long nA, int QA, long ldA,
                                                                     float* __restrict__ dstB, long nB) {
    constexpr int W = VEC ? 4 : 1;
    __shared__ float red[DET_TALL_PL][DET_TALL_CG][W];
    const int pl = threadIdx.x / DET_TALL_CG, cg = threadIdx.x % DET_TALL_CG;
    const long nv = (nA + nB) / W;
    const long v = (long)blockIdx.x * DET_TALL_CG + cg;
    float s[W];
#pragma unroll
    for (int e = 0; e < W; ++e) s[e] = 0.f;
    if (v < nv) {
        const float* src = part + v * W;
        int k = pl;
        for (; k + 7 * DET_TALL_PL < nparts; k += 8 * DET_TALL_PL) {
            if constexpr (VEC) {
                float4 t[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) t[j] = *reinterpret_cast<const float4*>(src + (size_t)(k + j * DET_TALL_PL) * part_stride);
#pragma unroll
                for (int j = 0; j < 8; ++j) { s[0] += t[j].x; s[1] += t[j].y; s[2] += t[j].z; s[3] += t[j].w; }
            } else {
                float t[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) t[j] = src[(size_t)(k + j * DET_TALL_PL) * part_stride];
#pragma unroll
                for (int j = 0; j < 8; ++j) s[0] += t[j];
            }
        }
        for (; k < nparts; k += DET_TALL_PL) {
            if constexpr (VEC) {
                const float4 t = *reinterpret_cast<const float4*>(src + (size_t)k * part_stride);
                s[0] += t.x; s[1] += t.y; s[2] += t.z; s[3] += t.w;
            } else {
                s[0] += src[(size_t)k * part_stride];
            }
        }
    }
#pragma unroll
    for (int e = 0; e < W; ++e) red[pl][cg][e] = s[e];
    __syncthreads();
    if (pl == 0 && v < nv) {
        const long c = v * W;
        float* d = (c < nA) ? dstA + (c / QA) * ldA + (c % QA) : dstB + (c - nA);
#pragma unroll
        for (int e = 0; e < W; ++e) {
            float t = 0.f;
#pragma unroll
            for (int l = 0; l < DET_TALL_PL; ++l) t += red[l][cg][e];
            d[e] += t;
        }
    }
}
// Several of those sums in ONE launch (the grouped weight-gradient GEMM: up to 8 products x (weight, bias) = 16 jobs, each a few microseconds
// of work behind a launch): workgroup b belongs to the job j with wg_start[j] <= b < wg_start[j + 1]; inside a job exactly det_reduce_kernel<true>.
static __global__ __launch_bounds__(256) void det_reduce_multi_kernel(DetJobs jb) {
    int j = 0;
    while (j + 1 < jb.n && (int)blockIdx.x >= jb.wg_start[j + 1]) ++j;
    const long v = (long)((int)blockIdx.x - jb.wg_start[j]) * 256 + threadIdx.x;
    if (v >= jb.nv[j]) return;
    const long c = v * 4;
    const float* src = jb.part[j] + c;
    const long stride = jb.stride[j];
    const int nparts = jb.nparts[j];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int k = 0;
    for (; k + 8 <= nparts; k += 8) {
        float4 t[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) t[i] = *reinterpret_cast<const float4*>(src + (size_t)(k + i) * stride);
#pragma unroll
        for (int i = 0; i < 8; ++i) { s0 += t[i].x; s1 += t[i].y; s2 += t[i].z; s3 += t[i].w; }
    }
    for (; k < nparts; ++k) {
        const float4 t = *reinterpret_cast<const float4*>(src + (size_t)k * stride);
        s0 += t.x; s1 += t.y; s2 += t.z; s3 += t.w;
    }
    float* d = jb.dst[j] + (c / jb.Q[j]) * jb.ld[j] + (c % jb.Q[j]);
    d[0] += s0; d[1] += s1; d[2] += s2; d[3] += s3;
}

bool det_reduce_multi(const DetJobs& jb, hipStream_t s) {
    if (jb.n <= 0) return true;
    hipLaunchKernelGGL(det_reduce_multi_kernel, dim3((unsigned)jb.wg_start[jb.n]), dim3(256), 0, s, jb);
    return hipGetLastError() == hipSuccess;
}
// launches the reduction; returns false when the launch failed
bool det_reduce(const float* part, int nparts, long part_stride, float* dstA, long nA, int QA, long ldA, float* dstB, long nB, hipStream_t s) {
    const bool vec = !(nA & 3) && !(QA & 3) && !(ldA & 3) && !(nB & 3) && !(part_stride & 3) && !((uintptr_t)part & 15) &&
                     !((uintptr_t)dstA & 15) && !((uintptr_t)dstB & 15);
    const long nv = (nA + nB) / (vec ? 4 : 1);
    if (nparts >= 32 && nv <= 16384) {  // many parts, few columns
        const unsigned grid = (unsigned)((nv + DET_TALL_CG - 1) / DET_TALL_CG);
        if (vec) hipLaunchKernelGGL(det_reduce_tall_kernel<true>, dim3(grid), dim3(256), 0, s, part, nparts, part_stride, dstA, nA, QA, ldA, dstB, nB);
        else hipLaunchKernelGGL(det_reduce_tall_kernel<false>, dim3(grid), dim3(256), 0, s, part, nparts, part_stride, dstA, nA, QA, ldA, dstB, nB);
        return hipGetLastError() == hipSuccess;
    }
    long grid = (nv + 255) / 256;
    if (grid > 2048) grid = 2048;
    if (grid < 1) grid = 1;
    if (vec) hipLaunchKernelGGL(det_reduce_kernel<true>, dim3((unsigned)grid), dim3(256), 0, s, part, nparts, part_stride, dstA, nA, QA, ldA, dstB, nB);
    else hipLaunchKernelGGL(det_reduce_kernel<false>, dim3((unsigned)grid), dim3(256), 0, s, part, nparts, part_stride, dstA, nA, QA, ldA, dstB, nB);
    return hipGetLastError() == hipSuccess;
}
