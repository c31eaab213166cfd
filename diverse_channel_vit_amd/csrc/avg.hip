// Weight averaging over the flat parameter arena: avg <- lerp(avg, p, w) in ONE streaming launch (SWA / SWAD / EMA of the weights;
// torch.optim.swa_utils.AveragedModel.update_parameters walks ~150 parameter views through multi-tensor lerps and branches on the host).
//   count == 0 : w = 1                      (the first update copies, as torch's class does)
//   SWA        : w = 1 / (count + 1)         (fp32, correctly rounded: the quotient torch computes from its long counter)
//   EMA        : w = ema_weight              (the host passes float(1 - decay), what torch hands to _foreach_lerp_)
// The count comes by value or from a device word (a captured step replays with the live count); the kernel never writes that word.
// Element update = ATen's two-sided lerp with the contraction written out, so that -ffp-contract changes nothing:
//   w == 1  : a <- p                         (the bits of p: -0.0, denormals, infinities, NaN payloads)
//   w < 0.5 : a <- fma(w, p - a, a)
//   else    : a <- fma(-(p - a), 1 - w, p)
// The branch on w is uniform for the whole launch.  No atomics: deterministic.  p is read only.
//
// Work split: chunks of AVG_ILP * 256 float4, chunk c to workgroup c % grid; a full chunk keeps AVG_ILP float4 of each operand in
// flight per lane, the ragged last chunk goes one float4 at a time, workgroup 0 takes the n % 4 scalar tail.
#include "dcv_common.hpp"
#include "../../include/dcv.h"

namespace {

// float4 of avg and of p in flight per lane, and the grid cap past which workgroups walk chunks: dcv_adamw_groups' values on the same arena.
// Measured on DiChaViT-S's full arena (profiles/weight_average_bench.txt; 1, 2, 8 in flight are stand-alone builds with
// -DDCV_AVG_ILP=n, the caps go through the grid_cap argument): from 512 workgroups on every shape is within 3.7 us of every other (42.3 .. 46.0 us)
// with 2 us between two entries of the same shape; 1 or 2 in flight without a cap measured 2.5 us under 4 without a cap.  4 and 2048 stay until a
// run that rotates the candidates' order separates them.  60 VGPRs, no scratch: eight waves per SIMD, 2048 workgroups of four waves all resident.
#ifndef DCV_AVG_ILP
#define DCV_AVG_ILP 4
#endif
#ifndef DCV_AVG_GRID_CAP
#define DCV_AVG_GRID_CAP 2048
#endif
constexpr int AVG_ILP = DCV_AVG_ILP;
constexpr int AVG_CHUNK4 = AVG_ILP * 256;
constexpr int AVG_GRID_CAP = DCV_AVG_GRID_CAP;

enum { AVG_COPY = 0, AVG_LOW = 1, AVG_HIGH = 2 };

template <int KIND>
__device__ __forceinline__ float avg_elem(float a, float p, float w, float omw) {
    if (KIND == AVG_COPY) return p;
    const float d = p - a;
    if (KIND == AVG_LOW) return fmaf(w, d, a);
    return fmaf(-d, omw, p);
}

template <int KIND>
__device__ __forceinline__ float4 avg_vec4(const float4& A, const float4& P, float w, float omw) {
    float4 r;
    r.x = avg_elem<KIND>(A.x, P.x, w, omw);
    r.y = avg_elem<KIND>(A.y, P.y, w, omw);
    r.z = avg_elem<KIND>(A.z, P.z, w, omw);
    r.w = avg_elem<KIND>(A.w, P.w, w, omw);
    return r;
}

template <int KIND>
__device__ __forceinline__ void avg_walk(float* __restrict__ avg, const float* __restrict__ p, long n4, long n, float w) {
    const float omw = 1.f - w;
    const unsigned t = threadIdx.x;
    float4* a4 = reinterpret_cast<float4*>(avg);
    const float4* p4 = reinterpret_cast<const float4*>(p);
    const long nchunks = (n4 + AVG_CHUNK4 - 1) / AVG_CHUNK4;
    for (long c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const long base = c * AVG_CHUNK4;
        if (base + AVG_CHUNK4 <= n4) {
            // a uniform base and a 32-bit lane index: 64 VGPRs, eight waves per SIMD (64-bit lane addresses took 66)
            const float4* __restrict__ pc = p4 + base;
            float4* __restrict__ ac = a4 + base;
            float4 A[AVG_ILP], P[AVG_ILP];
#pragma unroll
            for (int j = 0; j < AVG_ILP; ++j) {
                P[j] = pc[j * 256 + t];
                if constexpr (KIND != AVG_COPY) A[j] = ac[j * 256 + t];
                else A[j] = P[j];  // a copy never reads avg
            }
#pragma unroll
            for (int j = 0; j < AVG_ILP; ++j) ac[j * 256 + t] = avg_vec4<KIND>(A[j], P[j], w, omw);
        } else {
            for (long i = base + t; i < n4; i += 256) {
                const float4 P = p4[i];
                float4 A = P;
                if constexpr (KIND != AVG_COPY) A = a4[i];
                a4[i] = avg_vec4<KIND>(A, P, w, omw);
            }
        }
    }
    // scalar tail
    if (blockIdx.x == 0) {
        for (long i = n4 * 4 + t; i < n; i += 256) {
            const float pe = p[i];
            avg[i] = avg_elem<KIND>(KIND != AVG_COPY ? avg[i] : pe, pe, w, omw);
        }
    }
}

__global__ __launch_bounds__(256) void avg_update_kernel(float* __restrict__ avg, const float* __restrict__ p, long n4, long n, int mode,
                                                         float ema_weight, long count, const long long* __restrict__ count_dev) {
    if (count_dev) count = (long)count_dev[0];
    float w = 1.f;
    if (count != 0) w = (mode == DCV_AVG_SWA) ? __fdiv_rn(1.f, (float)(count + 1)) : ema_weight;
    if (w == 1.f) avg_walk<AVG_COPY>(avg, p, n4, n, w);
    else if (w < 0.5f) avg_walk<AVG_LOW>(avg, p, n4, n, w);
    else avg_walk<AVG_HIGH>(avg, p, n4, n, w);
}

}  // namespace

extern "C" int dcv_avg_update(float* avg, const float* p, long n, int mode, float ema_weight, long n_averaged,
                              const long long* n_averaged_dev, int grid_cap, void* stream) {
    if (!avg || !p) return DCV_ERR_NULL;
    if (n < 0) return DCV_ERR_SHAPE;
    if (((uintptr_t)avg | (uintptr_t)p) & 15) return DCV_ERR_ALIGN;
    if ((uintptr_t)n_averaged_dev & 7) return DCV_ERR_ALIGN;
    if (mode != DCV_AVG_SWA && mode != DCV_AVG_EMA) return DCV_ERR_UNSUPPORTED;
    if (!(ema_weight >= 0.f && ema_weight <= 1.f)) return DCV_ERR_SHAPE;  // NaN fails both comparisons
    if (!n_averaged_dev && n_averaged < 0) return DCV_ERR_SHAPE;
    if (grid_cap < 0) return DCV_ERR_SHAPE;
    if (n == 0) return DCV_OK;
    const long n4 = n / 4;
    long grid = (n4 + AVG_CHUNK4 - 1) / AVG_CHUNK4;
    const long cap = grid_cap > 0 ? grid_cap : AVG_GRID_CAP;
    if (grid > cap) grid = cap;
    if (grid < 1) grid = 1;  // n < 4: the scalar tail alone
    hipLaunchKernelGGL(avg_update_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, avg, p, n4, n, mode, ema_weight,
                       n_averaged, n_averaged_dev);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}
