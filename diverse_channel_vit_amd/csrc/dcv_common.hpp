// Shared device helpers for the gfx950 (CDNA4 / MI355X) kernels of libdcv_hip.so.
// wave = 64 lanes; MFMA bf16 32x32x16; LDS tiles are XOR-swizzled so that the same image
// serves ds_read_b128 row reads and ds_read_b64_tr_b16 transposed reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef __bf16 bf16_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#include "../../include/dcv.h"

#define DCV_LAUNCH_CHECK()                                   \
    do {                                                     \
        hipError_t e__ = hipGetLastError();                  \
        if (e__ != hipSuccess) return DCV_ERR_LAUNCH;        \
    } while (0)

#define LDS_PTR(T, p) ((__attribute__((address_space(3))) T*)(p))

union U128 {
    uint4 u;
    bf16x8 h;
    bf16x4 q[2];
    uint2 d[2];
};

__device__ __forceinline__ bf16x8 as_bf16x8(uint4 v) {
    U128 x;
    x.u = v;
    return x.h;
}
__device__ __forceinline__ uint4 as_uint4(bf16x8 v) {
    U128 x;
    x.h = v;
    return x.u;
}

__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);

}

// 16x16x32: lane l holds A[row l&15][k = 8(l>>4) + j], B[k = 8(l>>4) + j][col l&15]; the 4 accumulator registers of lane l are
// rows 4(l>>4) .. +3 of column l&15.  Same FLOPs per cycle as 32x32x16, but the chip — clock-limited by power on this workload —
// holds a higher clock on this shape (cdna guide rule 28; measured here: the NT GEMMs 7 % faster with the same operand traffic).
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// 32x32 accumulator: register r of lane l holds row acc_row(r, l>>5), column l&31.
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// pack registers 8s..8s+7 of a 32x32 f32 accumulator into the bf16 operand fragment of k-step s
// of a following 32x32x16 MFMA that sums over the accumulator's ROW index.  The k order inside the
// step is permuted: element j of lane half h is accumulator row 16s + 8(j>>2) + 4h + (j&3).
__device__ __forceinline__ bf16x8 acc_to_frag(const f32x16& x, int s) {
    bf16x8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (bf16_t)x[8 * s + j];
    return r;
}

// ---- 64-column bf16 LDS tile (128-byte rows, 8 chunks of 16 B) ------------------------------
// chunk' = chunk ^ f(row), f(row) = k ^ ((k & 1) << 2), k = (row >> 1) & 7.
//  * ds_read_b128 row reads (lane = row, same chunk): 16 rows of a lane group hit 16 distinct
//    16-B slots of the 256-B bank row -> conflict-free.
//  * ds_read_b64_tr_b16 (4 rows x 64 B per 32-lane half): rows q and q+2 land in different 64-B
//    halves -> conflict-free.
__device__ __forceinline__ int swz64(int row) {
    int k = (row >> 1) & 7;
    return k ^ ((k & 1) << 2);
}
// The same tile read ONLY by rows with 16x16x32 fragments (the NT GEMMs): lane (row l&15, k-chunk l>>4) — a ds_read_b128 lane group
// holds all 16 rows once, half of them at chunk c and half at c + 1, and rows r and r ^ 2 always fall in the same half, so the
// plain chunk ^ (row >> 1) swizzle is conflict-free.
__device__ __forceinline__ int swz64n(int row) { return (row >> 1) & 7; }
// byte offset of element (row, col) in a [rows][64] bf16 tile
__device__ __forceinline__ int lds64_off(int row, int col) {
    return row * 128 + ((((col >> 3) ^ swz64(row)) << 4) | ((col & 7) << 1));
}

// ---- 128-column bf16 LDS tile (256-byte rows, 16 chunks) for transposed reads only ----------
// 64-B segment index (4 per row) is XORed with (row & 3): the 4 rows of a tr read go to 4
// different segments of the bank row.
__device__ __forceinline__ int lds128_off(int row, int col) {
    int chunk = (col >> 3) ^ ((row & 3) << 2);
    return row * 256 + ((chunk << 4) | ((col & 7) << 1));
}

// transposed read: a 16-lane group reads a 4-row x 16-column block; lane i of the group passes
// the address of (row i>>2, cols 4*(i&3)..+3) and receives column i, rows 0..3.
__device__ __forceinline__ bf16x4 lds_tr_read(const char* base_generic, int byte_off) {
    s16x4 t = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, base_generic + byte_off));
    union {
        s16x4 s;
        bf16x4 b;
    } u;
    u.s = t;
    return u.b;
}

__device__ __forceinline__ bf16x8 join4(bf16x4 lo, bf16x4 hi) {
    U128 x;
    x.q[0] = lo;
    x.q[1] = hi;
    return x.h;
}

__device__ __forceinline__ uint4 lds_read128(const char* base, int byte_off) {
    return *reinterpret_cast<const uint4*>(base + byte_off);
}
__device__ __forceinline__ void lds_write128(char* base, int byte_off, uint4 v) {
    *reinterpret_cast<uint4*>(base + byte_off) = v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ uint2 pack4_bf16(float a, float b, float c, float d) {
    union {
        bf16x4 v;
        uint2 u;
    } x;
    x.v[0] = (bf16_t)a;
    x.v[1] = (bf16_t)b;
    x.v[2] = (bf16_t)c;
    x.v[3] = (bf16_t)d;
    return x.u;
}

__device__ __forceinline__ float bf16_bits_to_f32(unsigned short b) { return __uint_as_float(((unsigned)b) << 16); }

// ---- LDS-DMA (global_load_lds_dwordx4): destination is wave-uniform base + lane*16; any swizzle is applied to the
// per-lane SOURCE address (linear destination + permuted source + the same permutation on the read).
// Issued through inline asm on purpose: hipcc then neither counts it in its own vmcnt bookkeeping nor fences the
// following ds_reads with vmcnt(0) (which it does for the builtin and which would serialise the ring); the
// kernel waits with hand-counted s_waitcnt vmcnt(N) + a raw s_barrier.  M0 (the LDS base) is saved and restored
// inside the statement (cdna_hip_programming.md §5.7).
__device__ __forceinline__ void glds16(const bf16_t* g, unsigned lds_wave_base) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(g), "s"(lds_wave_base)
        : "memory");
}
// same DMA with a wave-uniform base (SGPR pair) and a per-lane 32-bit byte offset: a loop that walks tiles advances the
// base with scalar adds and keeps the lane offsets loop-invariant (no per-tile vector address arithmetic)
__device__ __forceinline__ void glds16s(const void* sbase, unsigned voff, unsigned lds_wave_base) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %2\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(sbase), "s"(lds_wave_base)
        : "memory");
}
// 4-byte-per-lane form (64 consecutive floats per wave instruction)
__device__ __forceinline__ void glds4s(const void* sbase, unsigned voff, unsigned lds_wave_base) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dword %1, %2\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(sbase), "s"(lds_wave_base)
        : "memory");
}
__device__ __forceinline__ unsigned lds_addr(const void* p) {
    return (unsigned)(size_t)(const __attribute__((address_space(3))) void*)p;
}

// XCD-aware remap: blocks b and b+8 share an XCD (round-robin dispatch, speed only).  Gives each
// XCD a contiguous range of logical ids.  Bijective for any n.
__device__ __forceinline__ int xcd_remap(int bid, int n) {
    int q = n >> 3, r = n & 7;
    int xcd = bid & 7, slot = bid >> 3;
    int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + slot;
}

// ---- deterministic mode (the reference trains with cudnn.deterministic = True, utils.py:394-401) -------------------------------
// Kernels that combine partial sums of several workgroups have a second form that STORES the partials to a caller-supplied
// workspace instead of adding them atomically; det_reduce() then adds them to the destination in index order.  The kernels and
// both launchers live in det_reduce.hip, compiled once; here is only what a caller needs to describe a job.
// det_reduce_multi: several of those sums in ONE launch, up to DET_MULTI_MAX jobs described by a DetJobs table.
constexpr int DET_MULTI_MAX = 16;
struct DetJobs {
    int n;
    int wg_start[DET_MULTI_MAX + 1];
    const float* part[DET_MULTI_MAX];
    int nparts[DET_MULTI_MAX];
    long stride[DET_MULTI_MAX];
    float* dst[DET_MULTI_MAX];
    long nv[DET_MULTI_MAX];  // float4 columns
    int Q[DET_MULTI_MAX];
    long ld[DET_MULTI_MAX];
};
// adds job (part, nparts, stride) -> dst[(c / Q) * ld + c % Q], c < n, to jb; false when the job does not fit the vector form or the table
static inline bool det_jobs_add(DetJobs& jb, const float* part, int nparts, long stride, float* dst, long n, int Q, long ld) {
    if (jb.n >= DET_MULTI_MAX || (n & 3) || (Q & 3) || (ld & 3) || (stride & 3) || ((uintptr_t)part & 15) || ((uintptr_t)dst & 15)) return false;
    const int j = jb.n++;
    jb.part[j] = part; jb.nparts[j] = nparts; jb.stride[j] = stride; jb.dst[j] = dst; jb.nv[j] = n / 4; jb.Q[j] = Q; jb.ld[j] = ld;
    jb.wg_start[j + 1] = jb.wg_start[j] + (int)((n / 4 + 255) / 256);
    return true;
}
// det_reduce.hip.  Column c of a part goes to dstA[(c / QA) * ldA + c % QA] for c < nA and to dstB[c - nA] for nA <= c < nA + nB.
// Both return false when the launch failed.
__attribute__((visibility("hidden"))) bool det_reduce(const float* part, int nparts, long part_stride, float* dstA, long nA, int QA, long ldA,
                                                      float* dstB, long nB, hipStream_t s);
__attribute__((visibility("hidden"))) bool det_reduce_multi(const DetJobs& jb, hipStream_t s);

// host_util.hip: CU count of the current device, queried once per device
__attribute__((visibility("hidden"))) int dcv_cu_count();
