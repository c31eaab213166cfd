// bf16 MFMA GEMMs for the DiChaViT encoder (gfx950), TN form; the forward and input-gradient products (NT form) are in gemm_nt.hip.
//
//  gemm_tn : dW[P,Q] += sum_m Y[m,P] . X[m,Q]  (+ dbias[P] += sum_m Y[m,P]); the weight gradient
//            of the layers gemm_nt computes.  Reduction dim is the long one (M = B*N tokens): split over
//            workgroups, fp32 atomics into the gradient arena.
//
// gemm_tn: 128x128 register-staged kernel (4 waves) and the 384x128 LDS-DMA ring kernel (8 waves).
#include <algorithm>
#include "dcv_common.hpp"
#include "../../include/dcv.h"

namespace {

constexpr int BK = 64;  // gemm_tn_kernel reduction rows per stage (the NT kernels stream NT_BK = N3_BK = 64-wide stages, gemm_tn384 T3_BK = 32 rows)

struct GemmTnArgs {
    const bf16_t* Y;
    int ldy;
    const bf16_t* X;
    int ldx;
    int M, P, Q;
    float* dW;
    int lddw;
    float* dbias;
    int m_per_split, splits;
    float* part;       // deterministic mode: split s stores its partial tile to part[s * part_stride + p * Q + q] (and its bias partial to
    long part_stride;  // part[s * part_stride + P * Q + p]) with plain stores instead of adding atomically; det_reduce_kernel sums them
    long bias_off;     // gemm_tn384, deterministic mode: float offset in `part` of the bias partials [splits * tiles_q][P]
};

__global__ __launch_bounds__(256) void gemm_tn_kernel(GemmTnArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[2][2][BK * 128 * 2];  // [buf][Y|X][64 rows x 256 B]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int h = lane >> 5, r32 = lane & 31, li = lane & 15, g1 = (lane >> 4) & 1;
    const int tiles_q = (a.Q + 127) / 128;
    // tile index fastest, splits outer, and an XCD gets a contiguous range of logical ids: the workgroups that
    // stream the SAME rows of Y and X (one split, all output tiles) run together on one XCD and share them in its L2.
    const int tiles = tiles_q * ((a.P + 127) / 128);
    int bid = xcd_remap(blockIdx.x, tiles * a.splits);
    const int split = bid / tiles;
    bid -= split * tiles;
    const int tq = bid % tiles_q, tp = bid / tiles_q;
    const int p0 = tp * 128, q0 = tq * 128;
    const int m_begin = split * a.m_per_split;
    const int m_end = min(a.M, m_begin + a.m_per_split);
    if (m_begin >= m_end) return;
    const int nk = (m_end - m_begin + BK - 1) / BK;

    // staging: tile [64 m][128 cols]; chunk q = tid + 256 i -> row = q>>4 (m), chunk = q&15 (cols 8*chunk..)
    const int srow = tid >> 4, sch = tid & 15;
    // P, Q are multiples of 8; chunks beyond the matrix edge re-read the last valid chunk (their products are never stored)
    const int colY = min(p0 + sch * 8, a.P - 8), colX = min(q0 + sch * 8, a.Q - 8);
    int soff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) soff[i] = lds128_off(srow + 16 * i, sch * 8);
    const bf16_t* gY = a.Y + (size_t)colY;
    const bf16_t* gX = a.X + (size_t)colX;

    uint4 ry[4], rx[4];
    float bs0 = 0.f, bs1 = 0.f, bs2 = 0.f, bs3 = 0.f, bs4 = 0.f, bs5 = 0.f, bs6 = 0.f, bs7 = 0.f;
    const bool do_bias = (a.dbias != nullptr) && (tq == 0);

#define TN_LOAD_TILE(kt_)                                                                                          \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                \
        int m = m_begin + (kt_) * BK + srow + 16 * i;                                                              \
        const bool ok = m < m_end;                                                                                 \
        int mc = ok ? m : (m_end - 1); /* always a valid row; out-of-range rows are zeroed in registers */         \
        uint4 ty = *reinterpret_cast<const uint4*>(gY + (size_t)mc * a.ldy);                                       \
        uint4 tx = *reinterpret_cast<const uint4*>(gX + (size_t)mc * a.ldx);                                       \
        ry[i] = make_uint4(ok ? ty.x : 0u, ok ? ty.y : 0u, ok ? ty.z : 0u, ok ? ty.w : 0u);                        \
        rx[i] = make_uint4(ok ? tx.x : 0u, ok ? tx.y : 0u, ok ? tx.z : 0u, ok ? tx.w : 0u);                        \
    }
#define TN_STORE_TILE(buf_)                                                                                        \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                \
        lds_write128(smem[buf_][0], soff[i], ry[i]);                                                               \
        lds_write128(smem[buf_][1], soff[i], rx[i]);                                                               \
        if (do_bias) {                                                                                             \
            bs0 += __uint_as_float(ry[i].x << 16); bs1 += __uint_as_float(ry[i].x & 0xffff0000u);                  \
            bs2 += __uint_as_float(ry[i].y << 16); bs3 += __uint_as_float(ry[i].y & 0xffff0000u);                  \
            bs4 += __uint_as_float(ry[i].z << 16); bs5 += __uint_as_float(ry[i].z & 0xffff0000u);                  \
            bs6 += __uint_as_float(ry[i].w << 16); bs7 += __uint_as_float(ry[i].w & 0xffff0000u);                  \
        }                                                                                                          \
    }

    TN_LOAD_TILE(0)
    TN_STORE_TILE(0)
    __syncthreads();

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // transposed-read lane addressing: lane supplies (row = 8h + (li>>2) [+4], cols = base + 16*g1 + 4*(li&3))
    const int trow = 8 * h + (li >> 2);
    const int tcolA = wm * 64 + 16 * g1 + 4 * (li & 3);
    const int tcolB = wn * 64 + 16 * g1 + 4 * (li & 3);

    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) { TN_LOAD_TILE(kt + 1) }
        const char* sY = smem[cur][0];
        const char* sX = smem[cur][1];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int row0 = 16 * ks + trow;
            bf16x8 af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                af[i] = join4(lds_tr_read(sY, lds128_off(row0, tcolA + 32 * i)), lds_tr_read(sY, lds128_off(row0 + 4, tcolA + 32 * i)));
                bf[i] = join4(lds_tr_read(sX, lds128_off(row0, tcolB + 32 * i)), lds_tr_read(sX, lds128_off(row0 + 4, tcolB + 32 * i)));
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = mfma32(af[i], bf[j], acc[i][j]);
        }
        if (kt + 1 < nk) { TN_STORE_TILE(cur ^ 1) }
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int q = q0 + wn * 64 + j * 32 + r32;
            if (q >= a.Q) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int p = p0 + wm * 64 + i * 32 + acc_row(r, h);
                if (p < a.P) {
                    if (a.part) a.part[(size_t)split * a.part_stride + (size_t)p * a.Q + q] = acc[i][j][r];
                    else atomicAdd(a.dW + (size_t)p * a.lddw + q, acc[i][j][r]);
                }
            }
        }

    if (do_bias) {
        // reduce the 16 threads that share a column chunk (same tid&15) through LDS
        float* red = reinterpret_cast<float*>(smem[0][0]);  // all tile reads are behind the last barrier
        float* rp = red + (srow * 16 + sch) * 8;
        rp[0] = bs0; rp[1] = bs1; rp[2] = bs2; rp[3] = bs3; rp[4] = bs4; rp[5] = bs5; rp[6] = bs6; rp[7] = bs7;
        __syncthreads();
        if (tid < 128) {
            int ch = tid >> 3, e = tid & 7;
            float s = 0.f;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) s += red[(rr * 16 + ch) * 8 + e];
            int p = p0 + ch * 8 + e;
            if (p < a.P) {
                if (a.part) a.part[(size_t)split * a.part_stride + (size_t)a.P * a.Q + p] = s;
                else atomicAdd(a.dbias + p, s);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// gemm_tn384: the same weight-gradient product with a 384 (P) x 128 (Q) output tile per workgroup: 96 FLOP per operand
// byte pulled through L2 -> LDS instead of 64 (the 128 x 128 kernel's loop is load-bound: 129 of 157 us with its MFMAs
// removed).  8 waves as 4 (P) x 2 (Q), each wave 96 x 64 = 3 x 2 MFMA tiles.  The reduction (token rows) streams in 32-row
// stages through a 4-deep LDS-DMA ring; a stage is four [32 rows][128 cols] images (Y columns 0-127 / 128-255 / 256-383,
// X columns 0-127), each 256-byte row swizzled per 64-byte segment (segment ^= row & 3) so that ds_read_b64_tr_b16 is
// conflict-free; every DMA instruction moves 4 rows x 256 contiguous bytes.  Used when P % 384 == 0 and Q % 128 == 0
// (all DiChaViT-S/B shapes); otherwise gemm_tn_kernel.
#ifndef DCV_T3_STAGES
#define DCV_T3_STAGES 4
#endif
constexpr int T3_BK = 32, T3_STAGES = DCV_T3_STAGES, T3_IMG = T3_BK * 256, T3_STAGE_BYTES = 4 * T3_IMG;  // 8 KB images, 32 KB stages

// bid: the workgroup's logical id inside this product, in [0, tiles * splits), tile index fastest
__device__ __forceinline__ void tn384_body(const GemmTnArgs& a, int bid, char* smem) {  // smem: T3_STAGES * T3_STAGE_BYTES = 128 KB: one workgroup per CU
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wp = wave >> 1, wq = wave & 1;
    const int h = lane >> 5, r32 = lane & 31, li = lane & 15, g1 = (lane >> 4) & 1;
    const int tiles_q = a.Q / 128, tiles = tiles_q * (a.P / 384);
    const int split = bid / tiles;
    bid -= split * tiles;
    const int tq = bid % tiles_q, tp = bid / tiles_q;
    const int p0 = tp * 384, q0 = tq * 128;
    const int m_begin = split * a.m_per_split;
    const int m_end = min(a.M, m_begin + a.m_per_split);
    if (m_begin >= m_end) return;
    const int nk = (m_end - m_begin + T3_BK - 1) / T3_BK;
    const int last_valid = (m_end - m_begin) - (nk - 1) * T3_BK;  // rows of the last stage that exist (1..32)

    // DMA: wave w fills image w>>1, rows [16*(w&1), +16) in four 4-row pieces; lane -> row lane>>4, physical chunk lane&15
    const int img = wave >> 1;
    const bf16_t* gsrc = (img < 3) ? a.Y + p0 + 128 * img : a.X + q0;
    const int ld = (img < 3) ? a.ldy : a.ldx;
    const int prow0 = 16 * (wave & 1) + (lane >> 4);  // + 4*j
    int lc8[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = prow0 + 4 * j, pc = lane & 15;
        lc8[j] = (((((pc >> 2) ^ (row & 3)) << 2) | (pc & 3))) * 8;  // logical chunk for this physical slot
    }
    const unsigned smem_base = __builtin_amdgcn_readfirstlane(lds_addr(smem));
    const unsigned dma_off = img * T3_IMG + 16 * (wave & 1) * 256;

#define T3_ISSUE(kt_)                                                                                     \
    {                                                                                                     \
        const unsigned sb_ = smem_base + ((kt_) % T3_STAGES) * T3_STAGE_BYTES + dma_off;                  \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                   \
            const int m_ = min(m_begin + (kt_) * T3_BK + prow0 + 4 * j, m_end - 1); /* tail rows: zeroed in LDS below */ \
            glds16(gsrc + (size_t)m_ * ld + lc8[j], sb_ + j * 1024);                                      \
        }                                                                                                 \
    }

    for (int st = 0; st < T3_STAGES - 1; ++st)
        if (st < nk) T3_ISSUE(st)

    f32x16 acc[3][2];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // transposed-read lane addressing inside an image: lane supplies (row = 8h + (li>>2) [+4], cols = base + 16*g1 + 4*(li&3))
    const int trow = 8 * h + (li >> 2);
    int offA[3], offB[2];  // byte offset of (image, column) for this wave's MFMA blocks, row 0
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int c = 96 * wp + 32 * i + 16 * g1 + 4 * (li & 3);  // column inside the 384-wide Y tile
        offA[i] = (c >> 7) * T3_IMG + (c & 127);                  // image byte base + column (resolved per row below)
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) offB[j] = 3 * T3_IMG + (64 * wq + 32 * j + 16 * g1 + 4 * (li & 3));
    auto tr_off = [](int imgcol, int row) {  // imgcol = image byte base + column (column < 128)
        const int base = imgcol & ~127, col = imgcol & 127;
        return base + lds128_off(row, col);
    };

    // bias gradient: the workgroups add up their Y images (48 column chunks x 10 row groups) — every workgroup of a row of tiles for the
    // stages kt % tiles_q == tq, so that the tiles of a split keep the same pace.  With the tq == 0 tiles doing all of it (rounds 1-2) they fell
    // behind, the tiles of a split drifted apart and the shared operand rows left L2 before the slower tiles read them: 675 MB from HBM per
    // launch at P = 1536, Q = 384 against 425 MB now (386 MB = the operands once); the launch 175 -> 160 us (profiles/r03_x7_*)
    const bool do_bias = (a.dbias != nullptr);
    const int bch = tid % 48, brg = tid / 48;  // threads >= 480 idle for this
    float bs[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bs[e] = 0.f;

    for (int kt = 0; kt < nk; ++kt) {
        const int rem = nk - 1 - kt;  // younger stages in flight: min(rem, T3_STAGES - 2), 4 DMA pieces per wave each
        if (T3_STAGES >= 5 && rem >= 3) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
        else if (T3_STAGES >= 4 && rem >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else if (T3_STAGES >= 3 && rem >= 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (kt + T3_STAGES - 1 < nk) T3_ISSUE(kt + T3_STAGES - 1)  // (split between the SIMD partners as in gemm_nt_kernel, or issued behind the first fragment reads: +-1 %, not kept)
        char* st = smem + (kt % T3_STAGES) * T3_STAGE_BYTES;
        if (kt == nk - 1 && last_valid < T3_BK) {  // ragged end of the reduction: rows that do not exist must contribute 0
            const int nbad = T3_BK - last_valid;
            for (int idx = tid; idx < nbad * 64; idx += 512) {
                const int r = last_valid + idx / 64, im = (idx & 63) >> 4, ch = idx & 15;
                lds_write128(st, im * T3_IMG + r * 256 + ch * 16, make_uint4(0, 0, 0, 0));
            }
            __syncthreads();
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int row0 = 16 * ks + trow;
            bf16x8 af[3], bf[2];
#pragma unroll
            for (int i = 0; i < 3; ++i) af[i] = join4(lds_tr_read(st, tr_off(offA[i], row0)), lds_tr_read(st, tr_off(offA[i], row0 + 4)));
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = join4(lds_tr_read(st, tr_off(offB[j], row0)), lds_tr_read(st, tr_off(offB[j], row0 + 4)));
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = mfma32(af[i], bf[j], acc[i][j]);
        }
        if (do_bias && (kt % tiles_q) == tq && brg < 10) {
            const int im = bch >> 4, ci = bch & 15;
            for (int r = brg; r < T3_BK; r += 10) {
                const int pc = ((((ci >> 2) ^ (r & 3)) << 2) | (ci & 3));
                const uint4 v = lds_read128(st, im * T3_IMG + r * 256 + pc * 16);
                bs[0] += __uint_as_float(v.x << 16); bs[1] += __uint_as_float(v.x & 0xffff0000u);
                bs[2] += __uint_as_float(v.y << 16); bs[3] += __uint_as_float(v.y & 0xffff0000u);
                bs[4] += __uint_as_float(v.z << 16); bs[5] += __uint_as_float(v.z & 0xffff0000u);
                bs[6] += __uint_as_float(v.w << 16); bs[7] += __uint_as_float(v.w & 0xffff0000u);
            }
        }
    }
#undef T3_ISSUE
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int q = q0 + wq * 64 + j * 32 + r32;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int p = p0 + wp * 96 + i * 32 + acc_row(r, h);
                if (a.part) a.part[(size_t)split * a.part_stride + (size_t)p * a.Q + q] = acc[i][j][r];
                else atomicAdd(a.dW + (size_t)p * a.lddw + q, acc[i][j][r]);
            }
        }
    if (do_bias) {
        __syncthreads();  // all stage reads are done: reuse the ring for the 10 x 384 partial sums
        float* red = reinterpret_cast<float*>(smem);
        if (brg < 10) {
#pragma unroll
            for (int e = 0; e < 8; ++e) red[(brg * 48 + bch) * 8 + e] = bs[e];
        }
        __syncthreads();
        if (tid < 384) {
            float sum = 0.f;
#pragma unroll
            for (int g = 0; g < 10; ++g) sum += red[g * 384 + tid];
            if (a.part) a.part[a.bias_off + ((size_t)split * tiles_q + tq) * a.P + p0 + tid] = sum;  // one row per (split, tq)
            else atomicAdd(a.dbias + p0 + tid, sum);
        }
    }
}

__global__ __launch_bounds__(512) void gemm_tn384_kernel(GemmTnArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[T3_STAGES * T3_STAGE_BYTES];  // 128 KB: one workgroup per CU
    tn384_body(a, xcd_remap(blockIdx.x, (a.Q / 128) * (a.P / 384) * a.splits), smem);
}

// Several weight-gradient products over the SAME token rows in one launch (a block's fc2 / fc1 / proj / qkv gradients: 36 tiles).  The CUs are
// filled by the tiles of all of them, so each tile is split 7 ways over the rows instead of 21 (or 85 for the 384 x 384 product): a third of
// the partial-tile traffic, k-loops three times as long, one launch and one fixed cost (~40 us of flush per launch, tools/tn_bench.py) instead of four.
constexpr int TN_GROUP_MAX = 8;
struct GemmTnGroup {
    int n;
    int start[TN_GROUP_MAX + 1];  // logical ids [start[i], start[i + 1]) belong to item i
    GemmTnArgs d[TN_GROUP_MAX];
};
__global__ __launch_bounds__(512) void gemm_tn384_group_kernel(GemmTnGroup g) {
    __shared__ __attribute__((aligned(16))) char smem[T3_STAGES * T3_STAGE_BYTES];  // 128 KB: one workgroup per CU
    const int id = xcd_remap(blockIdx.x, g.start[g.n]);
    int i = 0;
    while (i + 1 < g.n && id >= g.start[i + 1]) ++i;
    const GemmTnArgs a = g.d[i];
    tn384_body(a, id - g.start[i], smem);
}

}  // namespace

extern "C" int dcv_gemm_tn_pick(int M, int P, int Q, int tile) {
    (void)M;
    if (tile < DCV_TILE_AUTO || tile > DCV_TILE_WIDE) return DCV_ERR_SHAPE;
    const bool legal384 = (P % 384) == 0 && (Q % 128) == 0;
    if (tile == DCV_TILE_WIDE) return legal384 ? DCV_TILE_WIDE : DCV_ERR_UNSUPPORTED;
    if (tile == DCV_TILE_NARROW) return DCV_TILE_NARROW;
    return (legal384 && (P / 384) * (Q / 128) >= 6) ? DCV_TILE_WIDE : DCV_TILE_NARROW;
}

// splits / rows per split of a weight-gradient launch (pure function of the problem, the tile and the device's CU count)
static void tn_plan(int M, int P, int Q, int pick, int cus, int& splits, int& mps) {
    if (pick == DCV_TILE_WIDE) {
        const int tiles3 = (P / 384) * (Q / 128);
        splits = cus / tiles3;  // one 128 KB workgroup per CU, one resident round
        const int max3 = (M + T3_BK - 1) / T3_BK;
        if (splits > max3) splits = max3;
        if (splits < 1) splits = 1;
        mps = ((M + splits - 1) / splits + T3_BK - 1) / T3_BK * T3_BK;
    } else {
        const int tiles = ((P + 127) / 128) * ((Q + 127) / 128);
        // one resident round: 2 workgroups per CU (64 KB LDS each) = 2 x CUs slots; one workgroup more would run
        // alone in a second round and double the launch time.  Every split is a multiple of BK rows.
        splits = 2 * cus / tiles;
        const int max_splits = (M + BK - 1) / BK;
        if (splits > max_splits) splits = max_splits;
        if (splits < 1) splits = 1;
        mps = ((M + splits - 1) / splits + BK - 1) / BK * BK;
    }
    splits = (M + mps - 1) / mps;  // the splits that have rows (the leading ones)
}

static int tn_launch(const void* Y, int ldy, const void* X, int ldx, int M, int P, int Q, float* dW, int lddw, float* dbias, int tile,
                     float* ws, long ws_floats, void* stream) {
    if (!Y || !X || !dW) return DCV_ERR_NULL;
    if (M <= 0 || P <= 0 || Q <= 0 || (P % 8) || (Q % 8)) return DCV_ERR_SHAPE;
    if (ldy < P || ldx < Q || lddw < Q) return DCV_ERR_SHAPE;  // rows would overlap
    if ((ldy % 8) || (ldx % 8) || ((uintptr_t)Y & 15) || ((uintptr_t)X & 15)) return DCV_ERR_ALIGN;
    if (tile < DCV_TILE_AUTO || tile > DCV_TILE_WIDE) return DCV_ERR_SHAPE;
    const int cus = dcv_cu_count();
    // measured (M = 100 416): 1152x384 158 -> 140 us, 1536x384 206 -> 176, 384x1536 203 -> 182, but 384x384 63 -> 79
    // (3 tiles x 85 splits: the fp32 atomic traffic grows faster than the operand traffic shrinks)
    const int pick = dcv_gemm_tn_pick(M, P, Q, tile);
    if (pick < 0) return pick;
    int splits, mps;
    tn_plan(M, P, Q, pick, cus, splits, mps);
    // deterministic workspace: narrow kernel [splits][P*Q + P] (partial tile, then its bias partial); gemm_tn384, whose every tile
    // contributes to the bias gradient: [splits][P*Q], then [splits * tiles_q][P]
    const bool sep = pick != DCV_TILE_NARROW;
    const int tq9 = Q / 128;
    const long stride = sep ? (long)P * Q : (long)P * Q + P;
    const long bias_off = stride * splits;
    const long need = sep ? bias_off + (long)splits * tq9 * P : stride * splits;
    if (ws) {
        if (((uintptr_t)ws & 15) || (lddw % 4) || ((uintptr_t)dW & 15) || (dbias && ((uintptr_t)dbias & 15))) return DCV_ERR_ALIGN;
        if (ws_floats < need) return DCV_ERR_SHAPE;
    }
    GemmTnArgs a{(const bf16_t*)Y, ldy, (const bf16_t*)X, ldx, M, P, Q, dW, lddw, dbias, mps, splits, ws, stride, bias_off};
    if (pick == DCV_TILE_WIDE) {
        hipLaunchKernelGGL(gemm_tn384_kernel, dim3((P / 384) * (Q / 128) * splits), dim3(512), 0, (hipStream_t)stream, a);
    } else {
        hipLaunchKernelGGL(gemm_tn_kernel, dim3(((P + 127) / 128) * ((Q + 127) / 128) * splits), dim3(256), 0, (hipStream_t)stream, a);
    }
    DCV_LAUNCH_CHECK();
    if (ws) {
        if (sep) {
            if (!det_reduce(ws, splits, stride, dW, (long)P * Q, Q, lddw, nullptr, 0, (hipStream_t)stream)) return DCV_ERR_LAUNCH;
            if (dbias && !det_reduce(ws + bias_off, splits * tq9, P, dbias, P, P, P, nullptr, 0, (hipStream_t)stream)) return DCV_ERR_LAUNCH;
        } else if (!det_reduce(ws, splits, stride, dW, (long)P * Q, Q, lddw, dbias, dbias ? P : 0, (hipStream_t)stream)) {
            return DCV_ERR_LAUNCH;
        }
    }
    return DCV_OK;
}

extern "C" int dcv_gemm_tn_acc_ex(const void* Y, int ldy, const void* X, int ldx, int M, int P, int Q, float* dW, int lddw,
                                  float* dbias, int tile, void* stream) {
    return tn_launch(Y, ldy, X, ldx, M, P, Q, dW, lddw, dbias, tile, nullptr, 0, stream);
}

extern "C" long dcv_gemm_tn_det_ws_floats(int M, int P, int Q, int tile) {
    if (M <= 0 || P <= 0 || Q <= 0) return DCV_ERR_SHAPE;
    const int pick = dcv_gemm_tn_pick(M, P, Q, tile);
    if (pick < 0) return pick;
    int splits, mps;
    tn_plan(M, P, Q, pick, dcv_cu_count(), splits, mps);
    if (pick == DCV_TILE_NARROW) return ((long)P * Q + P) * splits;
    return (long)splits * P * Q + (long)splits * (Q / 128) * P;
}

extern "C" int dcv_gemm_tn_acc_det(const void* Y, int ldy, const void* X, int ldx, int M, int P, int Q, float* dW, int lddw,
                                   float* dbias, int tile, float* ws, long ws_floats, void* stream) {
    if (!ws) return DCV_ERR_NULL;
    return tn_launch(Y, ldy, X, ldx, M, P, Q, dW, lddw, dbias, tile, ws, ws_floats, stream);
}

// ---- grouped form (include/dcv.h: dcv_tn_item) --------------------------------------------------------------------------------------------
// The splits over the token rows and the rows per split are the same for every product, so every workgroup of the launch does the same FLOPs; per
// item: its 384 x 128 tiles, the rows of its bias partials (one per split and column tile) and its offset in the workspace.
struct TnGroupPlan {
    int splits, mps;
    int tiles[TN_GROUP_MAX], bias_rows[TN_GROUP_MAX];
    long off[TN_GROUP_MAX];
    long need;
};
static int tn_group_plan(const dcv_tn_item* it, int n, int M, int cus, TnGroupPlan& pl) {
    if (!it) return DCV_ERR_NULL;
    if (n < 1 || n > TN_GROUP_MAX || M <= 0) return DCV_ERR_SHAPE;
    int tiles = 0;
    for (int i = 0; i < n; ++i) {
        if (!it[i].Y || !it[i].X || !it[i].dW) return DCV_ERR_NULL;
        if (it[i].P <= 0 || it[i].Q <= 0 || (it[i].P % 384) || (it[i].Q % 128)) return DCV_ERR_UNSUPPORTED;
        if (it[i].ldy < it[i].P || it[i].ldx < it[i].Q || it[i].lddw < it[i].Q) return DCV_ERR_SHAPE;  // rows would overlap
        if ((it[i].ldy % 8) || (it[i].ldx % 8) || ((uintptr_t)it[i].Y & 15) || ((uintptr_t)it[i].X & 15)) return DCV_ERR_ALIGN;
        pl.tiles[i] = (it[i].P / 384) * (it[i].Q / 128);
        tiles += pl.tiles[i];
    }
    if (tiles > cus) return DCV_ERR_UNSUPPORTED;  // more than one resident round: call the products one by one
    const int sp = std::min(cus / tiles, (M + T3_BK - 1) / T3_BK);
    pl.mps = ((M + sp - 1) / sp + T3_BK - 1) / T3_BK * T3_BK;
    pl.splits = (M + pl.mps - 1) / pl.mps;
    pl.need = 0;
    for (int i = 0; i < n; ++i) {
        // per item: [splits][P * Q] partial tiles (the caller's layout), then the bias partials: [splits * tiles_q][P]
        pl.off[i] = pl.need;
        pl.bias_rows[i] = pl.splits * (it[i].Q / 128);
        pl.need += (long)pl.splits * it[i].P * it[i].Q + (long)pl.bias_rows[i] * it[i].P;
    }
    return DCV_OK;
}

extern "C" long dcv_gemm_tn_group_ws_floats(const dcv_tn_item* items, int n, int M) {
    TnGroupPlan pl;
    const int rc = tn_group_plan(items, n, M, dcv_cu_count(), pl);
    return rc ? rc : pl.need;
}

extern "C" int dcv_gemm_tn_group(const dcv_tn_item* items, int n, int M, float* ws, long ws_floats, void* stream) {
    TnGroupPlan pl;
    const int rc = tn_group_plan(items, n, M, dcv_cu_count(), pl);
    if (rc) return rc;
    if (ws) {
        if ((uintptr_t)ws & 15) return DCV_ERR_ALIGN;
        if (ws_floats < pl.need) return DCV_ERR_SHAPE;
        for (int i = 0; i < n; ++i)
            if ((items[i].lddw % 4) || ((uintptr_t)items[i].dW & 15) || (items[i].dbias && ((uintptr_t)items[i].dbias & 15))) return DCV_ERR_ALIGN;
    }
    GemmTnGroup g;
    g.n = n;
    int id = 0;
    for (int i = 0; i < n; ++i) {
        const dcv_tn_item& t = items[i];
        g.start[i] = id;
        id += pl.tiles[i] * pl.splits;
        const long stride = (long)t.P * t.Q;
        g.d[i] = GemmTnArgs{(const bf16_t*)t.Y, t.ldy, (const bf16_t*)t.X, t.ldx, M, t.P, t.Q, t.dW, t.lddw, t.dbias, pl.mps, pl.splits,
                            ws ? ws + pl.off[i] : nullptr, stride, stride * pl.splits};
    }
    g.start[n] = id;
    for (int i = n + 1; i <= TN_GROUP_MAX; ++i) g.start[i] = id;
    hipLaunchKernelGGL(gemm_tn384_group_kernel, dim3(id), dim3(512), 0, (hipStream_t)stream, g);
    DCV_LAUNCH_CHECK();
    if (ws) {  // the fixed-order second pass of every product (weight, bias) in one launch
        DetJobs jb;
        jb.n = 0;
        jb.wg_start[0] = 0;
        for (int i = 0; i < n; ++i) {
            const dcv_tn_item& t = items[i];
            const long stride = (long)t.P * t.Q;
            float* w = ws + pl.off[i];
            if (!det_jobs_add(jb, w, pl.splits, stride, t.dW, stride, t.Q, t.lddw)) return DCV_ERR_ALIGN;
            if (t.dbias && !det_jobs_add(jb, w + stride * pl.splits, pl.bias_rows[i], t.P, t.dbias, t.P, t.P, t.P)) return DCV_ERR_ALIGN;
        }
        if (!det_reduce_multi(jb, (hipStream_t)stream)) return DCV_ERR_LAUNCH;
    }
    return DCV_OK;
}

extern "C" int dcv_gemm_tn_acc(const void* Y, int ldy, const void* X, int ldx, int M, int P, int Q, float* dW, int lddw,
                               float* dbias, void* stream) {
    return dcv_gemm_tn_acc_ex(Y, ldy, X, ldx, M, P, Q, dW, lddw, dbias, DCV_TILE_AUTO, stream);
}
