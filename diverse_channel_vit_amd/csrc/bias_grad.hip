// Bias gradient without its weight gradient: dbias[p] += sum_m Y[m, p] for bf16 Y [M, P] (row stride ldy), fp32 accumulation.  The sum the weight-gradient
// GEMMs form beside their product (gemm_tn.hip), alone, for a Linear whose bias is trained and whose weight is frozen (DiChaViT's selective backward): one
// pass over Y at the streaming rate instead of a TN product whose result is thrown away.
//
// ALWAYS deterministic: no atomics.  Every workgroup stores its partial column sums to the caller's workspace with plain stores and det_reduce() adds
// the parts to dbias in workgroup order; inside a workgroup every lane adds its rows in row order and the lanes are added in lane order.  The
// association order is a function of the plan (M, P) alone.
//
// The plan (bg_plan, host logic; dcv_bias_grad_plan hands it out):
//   * a lane owns one 16-byte unit of a row — 8 bf16 columns, one buffer_load_dwordx4.  The P / 8 units of a row are cut into `col_chunks` column
//     chunks of `lpc` <= 64 lanes (col_chunks = ceil(P / 512), lpc = ceil(P / 8 / col_chunks): 384 -> 1 x 48, 1152 -> 3 x 48, 1536 -> 3 x 64);
//   * a wave load covers s = 64 / lpc consecutive rows of its column chunk (narrow P: 192 -> 2 rows, 8 -> 64 rows) and a wave keeps BG_U = 8 loads in
//     flight, so one wave step takes rows_per_wave = 8 s rows and a workgroup of four waves rows_per_wg = 32 s rows: 32 KB of Y at full lanes;
//   * the grid is (row workgroups, col_chunks) with row workgroups * col_chunks <= BG_GRID_CAP workgroups; past the cap a workgroup walks the row
//     chunks b, b + row workgroups, ... — `passes` of them at the most — and keeps adding into the same registers: one partial per workgroup,
//     whatever it walked.  The cap is 512, two workgroups per CU, not the other streaming kernels' 2048: every workgroup is one more part for
//     det_reduce to read, and at M = 100 416 the pair of launches measured 34.2 / 31.1 / 29.7 / 30.3 us (P = 384) and 92.3 / 89.1 / 84.4 / 82.6 us
//     (P = 1536) under caps of 2048 / 1024 / 512 / 256 (stand-alone builds with -DDCV_BG_GRID_CAP=n; profiles/selective_backward_bench.txt).  The
//     streaming launch alone runs at the rate of a device copy of the same bytes at P = 384 (19.2 against 18.8 us in a kernel trace).
#include "dcv_common.hpp"

namespace {

#ifndef DCV_BG_GRID_CAP
#define DCV_BG_GRID_CAP 512
#endif
constexpr int BG_U = 8, BG_WAVES = 4, BG_GRID_CAP = DCV_BG_GRID_CAP;

struct BgPlan {
    int col_chunks, lpc, s, rows_per_wave, rows_per_wg, row_wgs, passes;
    long row_chunks;
};

// M >= 1, P >= 8, P % 8 == 0
BgPlan bg_plan(int M, int P) {
    BgPlan p;
    const int units = P / 8;
    p.col_chunks = (units + 63) / 64;
    p.lpc = (units + p.col_chunks - 1) / p.col_chunks;
    p.s = 64 / p.lpc;
    p.rows_per_wave = BG_U * p.s;
    p.rows_per_wg = BG_WAVES * p.rows_per_wave;
    p.row_chunks = ((long)M + p.rows_per_wg - 1) / p.rows_per_wg;
    long cap = BG_GRID_CAP / p.col_chunks;
    if (cap < 1) cap = 1;
    p.row_wgs = (int)(p.row_chunks < cap ? p.row_chunks : cap);
    p.passes = (int)((p.row_chunks + p.row_wgs - 1) / p.row_wgs);
    return p;
}

__global__ __launch_bounds__(256) void bias_grad_kernel(const bf16_t* __restrict__ Y, long ldy, int M, int P, int lpc, int s, long row_chunks,
                                                        float* __restrict__ ws) {
    __shared__ float red[BG_WAVES * 64 * 8];  // [contributor = wave * s + sub-row][column of the chunk]: 4 s * 8 lpc <= 2048 floats
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int q = lane / lpc, cl = lane - q * lpc;  // sub-row of the wave load, lane inside the column chunk
    const int unit = blockIdx.y * lpc + cl;
    const bool active = q < s && unit * 8 < P;
    const int rows_per_wave = BG_U * s, rows_per_wg = BG_WAVES * rows_per_wave;
    // The loads go through a buffer descriptor made per row chunk from wave-uniform values, with loop-invariant 32-bit lane offsets (the host refuses
    // a chunk of 2 GB or more): flat loads kept a 64-bit lane address per load in flight and held the kernel at 4-5 waves per SIMD, this form takes
    // 66 VGPRs.  The descriptor's range ends with the chunk's last row below M, and a load past the range returns zeros — the rows past M need no
    // branch, and a lane without work (past the row's last unit, past the wave load's last sub-row) carries an offset past every range.  Nothing
    // outside [Y, Y + ((M - 1) ldy + P)) is read.
    const int lr0 = w * rows_per_wave + q;  // the lane's first row inside a chunk; its load j takes row lr0 + j s
    unsigned voff[BG_U];
#pragma unroll
    for (int j = 0; j < BG_U; ++j) voff[j] = active ? (unsigned)(((long)(lr0 + j * s) * ldy + (long)unit * 8) * 2) : 0x80000000u;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    for (long rc = blockIdx.x; rc < row_chunks; rc += gridDim.x) {
        const long left = (long)M - rc * rows_per_wg;  // rows of this chunk and after it: only the last chunk can be ragged
        const long rows = left < rows_per_wg ? left : rows_per_wg;
        const __amdgpu_buffer_rsrc_t chunk = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<char*>(reinterpret_cast<const char*>(Y)) + rc * rows_per_wg * ldy * 2, 0, (int)(((rows - 1) * ldy + P) * 2), 0x00020000);
        uint4 v[BG_U];
#pragma unroll
        for (int j = 0; j < BG_U; ++j) {  // all loads first: BG_U rows in flight per lane
            const auto t = __builtin_amdgcn_raw_buffer_load_b128(chunk, (int)voff[j], 0, 0);
            v[j] = make_uint4(t[0], t[1], t[2], t[3]);
        }
#pragma unroll
        for (int j = 0; j < BG_U; ++j) {
            const unsigned u[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[2 * e] += __uint_as_float(u[e] << 16);
                acc[2 * e + 1] += __uint_as_float(u[e] & 0xffff0000u);
            }
        }
    }
    // the lanes that hold the same columns (s sub-rows x 4 waves), added in contributor order by one thread per column
    const int ccols = lpc * 8;
    if (q < s) {
        float* mine = red + (w * s + q) * ccols + cl * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) mine[e] = acc[e];
    }
    __syncthreads();
    const int nc = BG_WAVES * s;
    for (int c = threadIdx.x; c < ccols; c += 256) {
        const int column = blockIdx.y * ccols + c;
        if (column >= P) continue;
        float t = 0.f;
        for (int k = 0; k < nc; ++k) t += red[k * ccols + c];
        ws[(size_t)blockIdx.x * P + column] = t;
    }
}

}  // namespace

extern "C" int dcv_bias_grad_plan(int M, int P, int* col_chunks, int* rows_per_wave, int* rows_per_wg, int* row_wgs, int* passes) {
    if (!col_chunks || !rows_per_wave || !rows_per_wg || !row_wgs || !passes) return DCV_ERR_NULL;
    if (M < 1 || P < 1) return DCV_ERR_SHAPE;
    if (P % 8) return DCV_ERR_UNSUPPORTED;
    const BgPlan p = bg_plan(M, P);
    *col_chunks = p.col_chunks;
    *rows_per_wave = p.rows_per_wave;
    *rows_per_wg = p.rows_per_wg;
    *row_wgs = p.row_wgs;
    *passes = p.passes;
    return DCV_OK;
}

extern "C" long dcv_bias_grad_ws_floats(int M, int P) {
    if (M < 1 || P < 1) return DCV_ERR_SHAPE;
    if (P % 8) return DCV_ERR_UNSUPPORTED;
    return (long)bg_plan(M, P).row_wgs * P;
}

extern "C" int dcv_bias_grad(const void* Y, int ldy, int M, int P, float* dbias, float* ws, long ws_floats, void* stream) {
    if (!Y || !dbias || !ws) return DCV_ERR_NULL;
    if (M < 1 || P < 1 || ldy < P) return DCV_ERR_SHAPE;
    if ((((uintptr_t)Y | (uintptr_t)dbias | (uintptr_t)ws) & 15) || (ldy & 7)) return DCV_ERR_ALIGN;
    if (P % 8) return DCV_ERR_UNSUPPORTED;
    const BgPlan p = bg_plan(M, P);
    if ((long)p.rows_per_wg * ldy * 2 >= (1L << 31)) return DCV_ERR_UNSUPPORTED;  // the kernel's lane offsets inside a row chunk are 32 bits
    if (ws_floats < (long)p.row_wgs * P) return DCV_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(bias_grad_kernel, dim3((unsigned)p.row_wgs, (unsigned)p.col_chunks), dim3(256), 0, st, (const bf16_t*)Y, (long)ldy, M, P, p.lpc,
                       p.s, p.row_chunks, ws);
    DCV_LAUNCH_CHECK();
    if (!det_reduce(ws, p.row_wgs, P, nullptr, 0, 4, 0, dbias, P, st)) return DCV_ERR_LAUNCH;
    return DCV_OK;
}
