// iBOT's masked patch-token distillation loss (Zhou et al. 2022; the patch term of DINOv2) and its gradient, fused: fp32 student logits S [R, K]
// (row stride lds) and teacher logits T [R, K] (row stride ldt), row r of both the same masked token; centre c [K]; row weights w [R].  With
// q_r = softmax((T_r - c) / tt) and p_r = softmax(S_r / ts):
//   loss = sum_r w_r (lse(S_r / ts) - <q_r, S_r> / ts),     dS[r,k] = g w_r (p_r[k] - q_r[k]) / ts,     tsum[k] = sum_r T[r,k] (unweighted).
// At R = 60 000 masked tokens and K = 8192 prototypes S and T are 2 GB each; the textbook form (softmax, log-softmax, product, row sum, weighting,
// autograd) materialises that matrix several times.  Here the forward reads S and T once and the backward reads them once more and writes dS once;
// no p, q or log p ever reaches memory.
//
// ALWAYS deterministic: no atomics.  The association order is a function of (R, K) alone — not of the data, the weights, the strides, the
// alignment or the grid.
//
// The plan (ib_plan, host logic; dcv_ibot_loss_plan hands it out).  The tile geometry is the DINO kernels' (loss_rows.hpp):
//   * the columns of a row are cut into col_tiles = ceil(K / 1024) tiles; the rows into chunks = ceil(R / 32) chunks of IB_CHUNK = 32 consecutive
//     rows.  One wave owns one ITEM = (chunk, tile), item = chunk * col_tiles + tile, and walks the chunk's rows through the tile with the next
//     row's loads of S and T in flight; the centre's tile is loaded once per item.  A lane holds 16 columns of the tile, four 16-byte loads per
//     row (vec = 4) or the same columns in sixteen 4-byte loads (vec = 1), through a buffer descriptor whose range ends the row at column K;
//   * per row of the chunk the wave forms what the DINO forward forms per view — the teacher's tile max of fl(T - c) with its low part and the sum
//     of exponentials relative to it, the student's tile max and sum, and the dot <e, S - student tile max> — and lane 0 stores the
//     (row, tile) record of 6 doubles to the workspace (the two sums of exponentials are formed in double, lane and wave);
//   * tsum, first level: while it walks, the lane adds its 16 teacher logits of every row to 16 double accumulators, in row order, and stores the
//     chunk's column sums as doubles to the workspace: chunks * K doubles, 1 / 16 of T's bytes.  A column sum over ~1e5 rows is not the shape of
//     the DINO finish's re-read of 2 B rows: it would read T a second time;
//   * a workgroup is 4 waves = 4 consecutive items (the tiles of one chunk side by side); the grid is min(ceil(items / 4), 2048) workgroups and
//     workgroup x walks the item groups x, x + grid, ...  Every item has its own records, so the walk does not touch the association order;
//   * the finish launch: thread r of the first ceil(R / 256) blocks merges the records of row r in tile order, writes the row statistics the
//     backward reads and the weighted row term w_r (ln(sum) - <q, S - max> / ts) in double; beside them, block cb of the last ceil(K / 64) blocks
//     forms tsum's second level for 64 columns: four groups of 64 lanes, group g adds the chunks g, g + 4, ... in chunk order, and the groups are
//     added in group order, all in double.  A third, one-block launch adds the R row terms and writes loss[0];
//   * the backward launch walks the same items: q from the saved teacher statistics, p from the saved student statistics, one store of dS.  The
//     incoming gradient g is read from device memory (no host synchronisation).
//
// Row statistics hold the SUM of exponentials, not the log-sum-exp — as a (high, low) pair of floats: s_stats [R, 3] = (max, sum hi, sum lo),
// t_stats [R, 4] = (max, the max's low part, sum hi, sum lo) — and the centred teacher logit keeps its rounding error, as in dino_loss.hip.
// A row of weight 0 has a row term of exactly 0 and a coefficient g w_r / ts of exactly 0: its dS row is 0 (the row is still read: tsum wants it).
#include "loss_rows.hpp"

namespace {

constexpr int IB_CHUNK = 32, IB_REC = 6;

struct IbPlan {
    int vec, col_tiles, chunks, grid, passes;
    long items, groups;
};

// R >= 1, K >= 1
IbPlan ib_plan(int R, int K, bool aligned) {
    IbPlan p;
    p.vec = aligned && K % 4 == 0 ? 4 : 1;
    p.col_tiles = (K + DL_TILE - 1) / DL_TILE;
    p.chunks = (R + IB_CHUNK - 1) / IB_CHUNK;
    p.items = (long)p.chunks * p.col_tiles;
    p.groups = (p.items + DL_WAVES - 1) / DL_WAVES;
    p.grid = (int)(p.groups < DL_GRID_CAP ? p.groups : DL_GRID_CAP);
    p.passes = (int)((p.groups + p.grid - 1) / p.grid);
    return p;
}

// doubles, two floats each: the (row, tile) records of IB_REC, then R (the rows' loss terms), then chunks * K (tsum's first level)
long ib_ws_floats(const IbPlan& p, int R, int K) { return 2L * ((long)R * p.col_tiles * IB_REC + R + (long)p.chunks * K); }

__device__ __forceinline__ double ib_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// dl_rounded for a double: a product that must be rounded before the fma or the conversion that consumes it
__device__ __forceinline__ double ib_rounded(double x) {
    asm volatile("" : "+v"(x));
    return x;
}

template <int VEC, bool TSUM>
__global__ __launch_bounds__(256) void ibot_loss_fwd_kernel(const float* __restrict__ S, long lds, const float* __restrict__ T, long ldt,
                                                            const float* __restrict__ c, int R, int K, int col_tiles, long items, float as, float at,
                                                            double* __restrict__ rec, double* __restrict__ part) {
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (long it = (long)blockIdx.x * DL_WAVES + w; it < items; it += (long)gridDim.x * DL_WAVES) {
        const int ch = (int)(it / col_tiles), tile = (int)(it - (long)ch * col_tiles), tile0 = tile * DL_TILE;
        const int r0 = ch * IB_CHUNK, r1 = r0 + IB_CHUNK < R ? r0 + IB_CHUNK : R;
        float cs[DL_SLOTS], ct[DL_SLOTS], ns[DL_SLOTS], nt[DL_SLOTS], cc[DL_SLOTS];
        double acc[DL_SLOTS];
#pragma unroll
        for (int j = 0; j < DL_SLOTS; ++j) acc[j] = 0.0;
        dl_load<VEC>(dl_uniform(c), K, tile0, lane, cc);
        dl_load<VEC>(dl_uniform(T + (long)r0 * ldt), K, tile0, lane, ct);
        dl_load<VEC>(dl_uniform(S + (long)r0 * lds), K, tile0, lane, cs);
        for (int r = r0; r < r1; ++r) {
            if (r + 1 < r1) {
                dl_load<VEC>(dl_uniform(T + (long)(r + 1) * ldt), K, tile0, lane, nt);
                dl_load<VEC>(dl_uniform(S + (long)(r + 1) * lds), K, tile0, lane, ns);
            }
            if constexpr (TSUM) {
#pragma unroll
                for (int j = 0; j < DL_SLOTS; ++j) acc[j] += (double)ct[j];  // a column >= K loaded 0 and is not stored
            }
            // the teacher's tile: e = exp((T - c) / tt - tile max), fl(T - c) carried with its rounding error
            float lo[DL_SLOTS];
            float tm = -INFINITY;
#pragma unroll
            for (int j = 0; j < DL_SLOTS; ++j) {
                dl_diff(ct[j], cc[j], ct[j], lo[j]);
                if (dl_col<VEC>(tile0, lane, j) >= K) ct[j] = -INFINITY, lo[j] = 0.f;
                tm = fmaxf(tm, ct[j]);
            }
            tm = wave_max(tm);  // finite: the tile's first column is below K
            float tml = -INFINITY;  // the low part that goes with the maximum: the largest among the columns that hold it
#pragma unroll
            for (int j = 0; j < DL_SLOTS; ++j) tml = ct[j] == tm ? fmaxf(tml, lo[j]) : tml;
            tml = wave_max(tml);
            // The sums of exponentials are added in DOUBLE, in the lane and across the wave: a float sum carries half an ulp of itself into
            // 1 / sum, i.e. into every q and p of the row — with a weight of order 1 that alone is 0.9 ulp of a dS entry of order 1 / ts.
            double tsm = 0.0;
#pragma unroll
            for (int j = 0; j < DL_SLOTS; ++j) {
                // every operation rounded on its own, here and below: both load widths must leave the same bits whatever the compiler would contract
                ct[j] = __builtin_amdgcn_exp2f(__fmul_rn(__fadd_rn(__fsub_rn(ct[j], tm), __fsub_rn(lo[j], tml)), at));
                tsm += (double)ct[j];
            }
            tsm = ib_wave_sum(tsm);
            // the student's tile
            float m = -INFINITY;
#pragma unroll
            for (int j = 0; j < DL_SLOTS; ++j) {
                if (dl_col<VEC>(tile0, lane, j) >= K) cs[j] = -INFINITY;
                m = fmaxf(m, cs[j]);
            }
            m = wave_max(m);
            double s = 0.0;
            float d = 0.f;
#pragma unroll
            for (int j = 0; j < DL_SLOTS; ++j) {
                s += (double)__builtin_amdgcn_exp2f(__fmul_rn(__fsub_rn(cs[j], m), as));
                const float x = dl_col<VEC>(tile0, lane, j) < K ? __fsub_rn(cs[j], m) : 0.f;  // relative to the tile max: no S-sized terms to cancel
                d = __fmaf_rn(ct[j], x, d);
            }
            s = ib_wave_sum(s);
            d = wave_sum(d);
            if (lane == 0) {
                double* o = rec + ((long)r * col_tiles + tile) * IB_REC;
                o[0] = tm; o[1] = tml; o[2] = tsm; o[3] = m; o[4] = s; o[5] = d;
            }
#pragma unroll
            for (int j = 0; j < DL_SLOTS; ++j) cs[j] = ns[j], ct[j] = nt[j];
        }
        if constexpr (TSUM) {
            double* o = part + (long)ch * K;
#pragma unroll
            for (int j = 0; j < DL_SLOTS; ++j) {
                const int col = dl_col<VEC>(tile0, lane, j);
                if (col < K) o[col] = acc[j];
            }
        }
    }
}

// blocks [0, row_blocks): thread -> row r, its col_tiles records merged in tile order.  blocks [row_blocks, ...): tsum's second level over 64
// columns per block (see the head of the file).
__global__ __launch_bounds__(256) void ibot_loss_finish_kernel(const double* __restrict__ rec, const float* __restrict__ w, int R, int K,
                                                               int col_tiles, int row_blocks, float as, float at, double inv_ts,
                                                               float* __restrict__ s_stats, float* __restrict__ t_stats,
                                                               double* __restrict__ rowloss, const double* __restrict__ part, int chunks,
                                                               float* __restrict__ tsum) {
    __shared__ double csum[4 * 64];
    if ((int)blockIdx.x < row_blocks) {
        const long r = (long)blockIdx.x * 256 + threadIdx.x;
        if (r >= R) return;
        const double* p = rec + r * col_tiles * IB_REC;  // per tile: (max hi, max lo, sum) of the teacher, (max, sum, dot) of the student
        float M0 = -INFINITY, L0 = -INFINITY, M = -INFINITY;  // maxima and low parts are floats stored as doubles
        for (int j = 0; j < col_tiles; ++j) {
            M0 = fmaxf(M0, (float)p[(long)j * IB_REC]);
            M = fmaxf(M, (float)p[(long)j * IB_REC + 3]);
        }
        for (int j = 0; j < col_tiles; ++j)
            if ((float)p[(long)j * IB_REC] == M0) L0 = fmaxf(L0, (float)p[(long)j * IB_REC + 1]);
        // <q, S> - M = sum_j (d_j + (m_j - M) s_j) w_j / Y0 with s_j, w_j the teacher's tile sum and its rescale exp2(((hi_j - M0) + (lo_j - L0)) at):
        // the weights s_j w_j / Y0 add up to 1, so the row maximum M leaves the row term exactly
        double Y0 = 0.0, Y = 0.0, D = 0.0;  // the sums in double: the loss reads them here, the backward as (high, low) floats
        for (int j = 0; j < col_tiles; ++j) {
            const double* t = p + (long)j * IB_REC;
            const double wt = ((double)((float)t[0] - M0) + (double)((float)t[1] - L0)) * (double)at;
            Y0 += t[2] * exp2(wt);
            Y += t[4] * exp2((double)((float)t[3] - M) * (double)as);
            D += (t[5] + (double)((float)t[3] - M) * t[2]) * exp2(wt);
        }
        if (t_stats) {
            const float hi = (float)Y0;
            t_stats[4 * r] = M0; t_stats[4 * r + 1] = L0; t_stats[4 * r + 2] = hi; t_stats[4 * r + 3] = (float)(Y0 - (double)hi);
        }
        if (s_stats) {
            const float hi = (float)Y;
            s_stats[3 * r] = M; s_stats[3 * r + 1] = hi; s_stats[3 * r + 2] = (float)(Y - (double)hi);
        }
        rowloss[r] = (double)w[r] * (log(Y) - D / Y0 * inv_ts);
        return;
    }
    const int cb = blockIdx.x - row_blocks, lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long col = (long)cb * 64 + lane;
    double a = 0.0;
    if (col < K) {
#pragma unroll 8
        for (int ch = g; ch < chunks; ch += 4) a += part[(long)ch * K + col];
    }
    csum[g * 64 + lane] = a;
    __syncthreads();
    if (g == 0 && col < K) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) t += csum[k * 64 + lane];
        tsum[col] = (float)t;
    }
}

// loss[0] = sum_r rowloss[r]: thread t adds the rows t, t + 256, ... in row order, thread 0 adds the threads in thread order
__global__ __launch_bounds__(256) void ibot_loss_sum_kernel(const double* __restrict__ rowloss, int R, float* __restrict__ loss) {
    __shared__ double red[256];
    double t = 0.0;
    for (int r = threadIdx.x; r < R; r += 256) t += rowloss[r];
    red[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        const int nt = R < 256 ? R : 256;
        for (int k = 0; k < nt; ++k) s += red[k];
        loss[0] = (float)s;
    }
}

template <int VEC>
__global__ __launch_bounds__(256) void ibot_loss_bwd_kernel(const float* __restrict__ S, long lds, const float* __restrict__ T, long ldt,
                                                            const float* __restrict__ c, const float* __restrict__ s_stats,
                                                            const float* __restrict__ t_stats, const float* __restrict__ w,
                                                            const float* __restrict__ g, int R, int K, int col_tiles, long items, float as,
                                                            float at, double inv_ts, float* __restrict__ dS, long ldd) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float g0 = g[0];
    for (long it = (long)blockIdx.x * DL_WAVES + wv; it < items; it += (long)gridDim.x * DL_WAVES) {
        const int ch = (int)(it / col_tiles), tile0 = (int)(it - (long)ch * col_tiles) * DL_TILE;
        const int r0 = ch * IB_CHUNK, r1 = r0 + IB_CHUNK < R ? r0 + IB_CHUNK : R;
        float cs[DL_SLOTS], ct[DL_SLOTS], ns[DL_SLOTS], nt[DL_SLOTS], cc[DL_SLOTS];
        dl_load<VEC>(dl_uniform(c), K, tile0, lane, cc);
        dl_load<VEC>(dl_uniform(T + (long)r0 * ldt), K, tile0, lane, ct);
        dl_load<VEC>(dl_uniform(S + (long)r0 * lds), K, tile0, lane, cs);
        for (int r = r0; r < r1; ++r) {
            if (r + 1 < r1) {
                dl_load<VEC>(dl_uniform(T + (long)(r + 1) * ldt), K, tile0, lane, nt);
                dl_load<VEC>(dl_uniform(S + (long)(r + 1) * lds), K, tile0, lane, ns);
            }
            const float M0 = t_stats[4 * (long)r], L0 = t_stats[4 * (long)r + 1];
            const float M = s_stats[3 * (long)r];
            // The exponentials are float; what follows them — the two divisions by the sums, the difference and the row's coefficient g w_r / ts —
            // runs in double and is rounded ONCE: with a weight of order 1 a dS entry is of order 1 / ts, and four float roundings in a row
            // (p, q, p - q, the product) measured 1.15 ulp of it, more than the float32 restatement's own error at a lucky row allows.
            const double inv0 = 1.0 / ((double)t_stats[4 * (long)r + 2] + (double)t_stats[4 * (long)r + 3]);
            const double inv = 1.0 / ((double)s_stats[3 * (long)r + 1] + (double)s_stats[3 * (long)r + 2]);
            const double coef = (double)g0 * (double)w[r] * inv_ts;
            float* drow = dS + (long)r * ldd;
#pragma unroll
            for (int j = 0; j < DL_SLOTS; ++j) {  // float operations rounded on their own, the double ones written out as one product and one fma: both load widths must give the same bits
                float hi, lo;
                dl_diff(ct[j], cc[j], hi, lo);
                const float eq = dl_rounded(__builtin_amdgcn_exp2f(__fmul_rn(__fadd_rn(__fsub_rn(hi, M0), __fsub_rn(lo, L0)), at)));
                const float ep = dl_rounded(__builtin_amdgcn_exp2f(__fmul_rn(__fsub_rn(cs[j], M), as)));
                const double q = ib_rounded((double)eq * inv0);
                cs[j] = (float)ib_rounded(coef * __builtin_fma((double)ep, inv, -q));  // equal operands (all logits 0, K a power of two) cancel exactly
            }
            if constexpr (VEC == 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int col = dl_col<VEC>(tile0, lane, 4 * u);
                    if (col < K) *reinterpret_cast<float4*>(drow + col) = make_float4(cs[4 * u], cs[4 * u + 1], cs[4 * u + 2], cs[4 * u + 3]);
                }
            } else {
#pragma unroll
                for (int j = 0; j < DL_SLOTS; ++j) {
                    const int col = dl_col<VEC>(tile0, lane, j);
                    if (col < K) drow[col] = cs[j];
                }
            }
#pragma unroll
            for (int j = 0; j < DL_SLOTS; ++j) cs[j] = ns[j], ct[j] = nt[j];
        }
    }
}

bool ib_aligned(const void* a, const void* b, const void* c, const void* d, long l0, long l1, long l2) {
    return !((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) || ((l0 | l1 | l2) & 3));
}

int ib_check(int R, int K, long lds, long ldt, float ts, float tt) {
    if (R < 1 || K < 1 || lds < K || ldt < K || !(ts > 0.f) || !(tt > 0.f)) return DCV_ERR_SHAPE;
    if (((long)K + DL_TILE) * 4 >= (1L << 31)) return DCV_ERR_UNSUPPORTED;  // a row is one buffer range with 32-bit lane offsets: 2 GB with its last tile
    return DCV_OK;
}

}  // namespace

extern "C" int dcv_ibot_loss_plan(int R, int K, int aligned, int* vec, int* tile_cols, int* col_tiles, int* chunk_rows, int* chunks, long* items,
                                  int* waves_per_wg, int* grid, int* passes) {
    if (!vec || !tile_cols || !col_tiles || !chunk_rows || !chunks || !items || !waves_per_wg || !grid || !passes) return DCV_ERR_NULL;
    const int rc = ib_check(R, K, K, K, 1.f, 1.f);
    if (rc) return rc;
    const IbPlan p = ib_plan(R, K, aligned != 0);
    *vec = p.vec;
    *tile_cols = DL_TILE;
    *col_tiles = p.col_tiles;
    *chunk_rows = IB_CHUNK;
    *chunks = p.chunks;
    *items = p.items;
    *waves_per_wg = DL_WAVES;
    *grid = p.grid;
    *passes = p.passes;
    return DCV_OK;
}

extern "C" long dcv_ibot_loss_ws_floats(int R, int K) {
    const int rc = ib_check(R, K, K, K, 1.f, 1.f);
    if (rc) return rc;
    return ib_ws_floats(ib_plan(R, K, true), R, K);
}

extern "C" int dcv_ibot_loss_fwd(const float* S, long lds, const float* T, long ldt, const float* center, const float* weights, int R, int K,
                                 float student_temp, float teacher_temp, float* loss, float* s_stats, float* t_stats, float* tsum, float* ws,
                                 long ws_floats, void* stream) {
    if (!S || !T || !center || !weights || !loss || !ws) return DCV_ERR_NULL;
    const int rc = ib_check(R, K, lds, ldt, student_temp, teacher_temp);
    if (rc) return rc;
    if ((((uintptr_t)S | (uintptr_t)T | (uintptr_t)center | (uintptr_t)weights | (uintptr_t)loss | (uintptr_t)s_stats | (uintptr_t)t_stats |
          (uintptr_t)tsum) & 3) || ((uintptr_t)ws & 15))
        return DCV_ERR_ALIGN;
    const IbPlan p = ib_plan(R, K, ib_aligned(S, T, center, nullptr, lds, ldt, 0));
    if (ws_floats < ib_ws_floats(p, R, K)) return DCV_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const float as = (float)(DL_LOG2E / student_temp), at = (float)(DL_LOG2E / teacher_temp);
    double* rec = reinterpret_cast<double*>(ws);  // ws is 16-byte aligned
    double* rowloss = rec + (long)R * p.col_tiles * IB_REC;
    double* part = rowloss + R;
    const dim3 grid((unsigned)p.grid), block(256);
    if (p.vec == 4 && tsum)
        hipLaunchKernelGGL((ibot_loss_fwd_kernel<4, true>), grid, block, 0, st, S, lds, T, ldt, center, R, K, p.col_tiles, p.items, as, at, rec, part);
    else if (p.vec == 4)
        hipLaunchKernelGGL((ibot_loss_fwd_kernel<4, false>), grid, block, 0, st, S, lds, T, ldt, center, R, K, p.col_tiles, p.items, as, at, rec, part);
    else if (tsum)
        hipLaunchKernelGGL((ibot_loss_fwd_kernel<1, true>), grid, block, 0, st, S, lds, T, ldt, center, R, K, p.col_tiles, p.items, as, at, rec, part);
    else
        hipLaunchKernelGGL((ibot_loss_fwd_kernel<1, false>), grid, block, 0, st, S, lds, T, ldt, center, R, K, p.col_tiles, p.items, as, at, rec, part);
    DCV_LAUNCH_CHECK();
    const int row_blocks = (R + 255) / 256, tsum_blocks = tsum ? (K + 63) / 64 : 0;
    hipLaunchKernelGGL(ibot_loss_finish_kernel, dim3((unsigned)(row_blocks + tsum_blocks)), block, 0, st, (const double*)rec, weights, R, K, p.col_tiles,
                       row_blocks, as, at, 1.0 / (double)student_temp, s_stats, t_stats, rowloss, (const double*)part, p.chunks, tsum);
    DCV_LAUNCH_CHECK();
    hipLaunchKernelGGL(ibot_loss_sum_kernel, dim3(1), block, 0, st, (const double*)rowloss, R, loss);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

extern "C" int dcv_ibot_loss_bwd(const float* S, long lds, const float* T, long ldt, const float* center, const float* weights,
                                 const float* s_stats, const float* t_stats, const float* g, int R, int K, float student_temp, float teacher_temp,
                                 float* dS, long ldd, void* stream) {
    if (!S || !T || !center || !weights || !s_stats || !t_stats || !g || !dS) return DCV_ERR_NULL;
    const int rc = ib_check(R, K, lds, ldt, student_temp, teacher_temp);
    if (rc) return rc;
    if (ldd < K) return DCV_ERR_SHAPE;
    if (((uintptr_t)S | (uintptr_t)T | (uintptr_t)center | (uintptr_t)weights | (uintptr_t)s_stats | (uintptr_t)t_stats | (uintptr_t)g |
         (uintptr_t)dS) & 3)
        return DCV_ERR_ALIGN;
    const IbPlan p = ib_plan(R, K, ib_aligned(S, T, center, dS, lds, ldt, ldd));
    hipStream_t st = (hipStream_t)stream;
    const float as = (float)(DL_LOG2E / student_temp), at = (float)(DL_LOG2E / teacher_temp);
    const double inv_ts = (double)(1.0f / student_temp);  // rounded to float: 10 for 0.1f, 25 for 0.04f, where the double quotient of the float is not
    if (p.vec == 4)
        hipLaunchKernelGGL(ibot_loss_bwd_kernel<4>, dim3((unsigned)p.grid), dim3(256), 0, st, S, lds, T, ldt, center, s_stats, t_stats, weights, g, R,
                           K, p.col_tiles, p.items, as, at, inv_ts, dS, ldd);
    else
        hipLaunchKernelGGL(ibot_loss_bwd_kernel<1>, dim3((unsigned)p.grid), dim3(256), 0, st, S, lds, T, ldt, center, s_stats, t_stats, weights, g, R,
                           K, p.col_tiles, p.items, as, at, inv_ts, dS, ldd);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}
