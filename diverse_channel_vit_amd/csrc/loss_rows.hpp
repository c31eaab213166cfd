// Device helpers shared by the row-streaming distillation losses (dino_loss.hip, ibot_loss.hip): a row's columns in tiles of DL_TILE = 1024, one
// wave per tile, lane l holding the 16 columns tile * 1024 + (64 u + l) * 4 + e, u, e < 4 (slot 4 u + e).  Inline helpers only: the kernels live
// in the .hip files.
#pragma once
#include "dcv_common.hpp"

#include <math.h>

namespace {

constexpr int DL_TILE = 1024, DL_SLOTS = 16, DL_WAVES = 4, DL_GRID_CAP = 2048;
constexpr double DL_LOG2E = 1.4426950408889634;

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// T - c without its rounding error: hi = fl(t - c) and lo with hi + lo = t - c exactly (Knuth's two-sum; every operation rounded on its own).  With a
// centre of 1e3 the rounding of hi alone is 3e-5, 8e-4 in the exponent at a temperature of 0.04: enough to move a softmax that is not one-hot.
__device__ __forceinline__ void dl_diff(float t, float c, float& hi, float& lo) {
    hi = __fsub_rn(t, c);
    const float bb = __fsub_rn(hi, t);
    lo = __fsub_rn(__fsub_rn(t, __fsub_rn(hi, bb)), __fadd_rn(c, bb));
}

// A product that must be rounded before it is used.  The library is built with -ffp-contract=fast, under which hipcc fuses a multiply into the add or
// subtract that consumes it wherever it sees one — HIP's __fmul_rn is a plain operator to it, and the option ignores contraction pragmas — and it saw
// different ones in the 16-byte and the 4-byte instantiation of the backward (with m_v folded to 1 the product e * inv met the subtraction of Q in one
// of them: 3 of 6000 dS entries one ulp apart).  An empty asm statement hides the value's origin; it costs no instruction.
__device__ __forceinline__ float dl_rounded(float x) {
    asm volatile("" : "+v"(x));
    return x;
}

// the column of a lane's slot j: the same with either load width, so that the association order does not depend on the alignment
template <int VEC>
__device__ __forceinline__ int dl_col(int tile0, int lane, int j) {
    return tile0 + (((j >> 2) * 64 + lane) << 2) + (j & 3);
}

// the 16 slots of a lane from the row that starts at `row` (wave-uniform): the descriptor's range ends the row at column K, a load past it returns 0
template <int VEC>
__device__ __forceinline__ void dl_load(const float* row, int K, int tile0, int lane, float (&x)[DL_SLOTS]) {
    const __amdgpu_buffer_rsrc_t d = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(row), 0, K * 4, 0x00020000);
    if constexpr (VEC == 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const auto t = __builtin_amdgcn_raw_buffer_load_b128(d, (tile0 + ((u * 64 + lane) << 2)) * 4, 0, 0);
#pragma unroll
            for (int e = 0; e < 4; ++e) x[4 * u + e] = __uint_as_float(t[e]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < DL_SLOTS; ++j) x[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(d, dl_col<VEC>(tile0, lane, j) * 4, 0, 0));
    }
}

// a wave-uniform pointer the compiler can see is one: its two halves through readfirstlane
__device__ __forceinline__ const float* dl_uniform(const float* p) {
    const uintptr_t a = (uintptr_t)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    return (const float*)(((uintptr_t)hi << 32) | lo);
}

}  // namespace
