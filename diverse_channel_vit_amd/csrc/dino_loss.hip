// DINO's multi-crop self-distillation loss (facebookresearch DINO, DINOLoss) and its gradient, fused: fp32 student logits S [V, B, K] (view-major,
// views 0 and 1 the global crops, row stride lds), teacher logits T [2, B, K] (row stride ldt), centre c [K].  With q_i = softmax((T_i - c) / tt),
// p_v = softmax(S_v / ts), n = 2V - 2, m_v = 1 for v < 2 else 2 and Q_v = sum_{i != v} q_i:
//   loss = 1 / (n B) sum_v sum_b [ m_v lse(S_v[b] / ts) - <Q_v[b], S_v[b]> / ts ],     dS_v[b,k] = g (m_v p_v[b,k] - Q_v[b,k]) / (n B ts).
// The textbook form is a softmax, a log-softmax, n pairwise products and their autograd backward: tens of passes over S.  Here the forward reads S and T
// once and the backward reads them once more and writes dS once; no p, q or log p ever reaches memory.
//
// ALWAYS deterministic: no atomics.  The association order is a function of (V, B, K) alone.
//
// The plan (dl_plan, host logic; dcv_dino_loss_plan hands it out):
//   * the columns of a row are cut into col_tiles = ceil(K / 1024) tiles of DL_TILE = 1024 columns.  One wave owns one ITEM = (batch row b, tile) for
//     ALL views: item = b * col_tiles + tile.  A lane holds 16 columns of the tile: slot j = 4 u + e is column tile * 1024 + (64 u + lane) * 4 + e, four
//     16-byte loads per row (vec = 4: every pointer 16-byte aligned, every stride and K a multiple of 4) or, where that does not hold, the same
//     columns in sixteen 4-byte loads (vec = 1): the slower form has the faster one's summation order.  Columns >= K are masked; the loads go through a buffer descriptor whose range ends the row at column K, so nothing
//     past a row's K columns is read (padding may hold NaN);
//   * the wave keeps the tile of exp((T_i - c) / tt - tile max), i = 0, 1, in registers (2 x 16), then streams the V student rows of b through it with
//     the next row's loads in flight: per view the tile max, the sum of exponentials relative to it, and the two dots <e_i, S_v - view's tile max> relative
//     to the TEACHER's tile max.  Lane 0 stores the item's partial record — (max, its low part, sum) of both teachers, then (max, sum, dot_0, dot_1) per view:
//     6 + 4 V floats; the centred teacher logit is carried as fl(T - c) plus its exact rounding error — to the caller's workspace.  Online max / sum-exp happens where partials meet: across lanes in the wave, across tiles in the finish;
//   * a workgroup is 4 waves = 4 consecutive items; the grid is min(ceil(items / 4), DL_GRID_CAP = 2048) workgroups and workgroup x walks the item
//     groups x, x + grid, ... — `passes` of them at the most.  Every item has its own record, so the walk does not touch the association order;
//   * the finish launch: block b < B merges the records of batch row b in tile order, rescaling sums and dots to the row maxima as the attention
//     forward rescales, writes the row statistics the backward reads — (max, sum of exponentials) per student and per teacher row — and the row's
//     loss term in double to the workspace's tail; the blocks after them form the centre statistics tsum[k] = sum_{i,b} T_i[b,k] (below).  A third,
//     one-block launch adds the B row terms in row order and writes loss[0];
//   * the backward launch walks the same items: q_0, q_1 of the tile from the saved teacher statistics, then per view p from the saved student
//     statistics and one store of dS.  The incoming gradient g is read from device memory (no host synchronisation).
//
// Row statistics hold the SUM of exponentials, not the log-sum-exp: p = e / sum is then exact for exact operands (all logits equal and K a power of
// two give p = 1 / K bit for bit; one-hot rows give exactly 0 and 1), which ln and exp of an lse are not.  lse = max / ts + ln(sum).
//
// Centre statistics: tsum is formed in the FINISH launch by re-reading T (2 B K floats, a fifth of the forward's bytes at V = 10), not in the
// streaming launch: there a wave holds one batch row's tile, so a column sum over b would need either B K floats of partials through the workspace —
// the same bytes as the re-read, written and read — or waves that walk several batch rows in sequence, which leaves the launch with a fraction of
// its waves.  The re-read runs beside the row merge in the same launch.
#include "loss_rows.hpp"  // the tile geometry and the lane helpers, shared with ibot_loss.hip

namespace {

struct DlPlan {
    int vec, col_tiles, grid, passes, rec;  // rec: floats of an item's record
    long items, groups;
};

// V >= 2, B >= 1, K >= 1
DlPlan dl_plan(int V, int B, int K, bool aligned) {
    DlPlan p;
    p.vec = aligned && K % 4 == 0 ? 4 : 1;
    p.col_tiles = (K + DL_TILE - 1) / DL_TILE;
    p.items = (long)B * p.col_tiles;
    p.groups = (p.items + DL_WAVES - 1) / DL_WAVES;
    p.grid = (int)(p.groups < DL_GRID_CAP ? p.groups : DL_GRID_CAP);
    p.passes = (int)((p.groups + p.grid - 1) / p.grid);
    p.rec = 6 + 4 * V;
    return p;
}

long dl_ws_floats(const DlPlan& p, int B) { return p.items * p.rec + 2L * B; }  // the records, then B doubles: the rows' loss terms

template <int VEC>
__global__ __launch_bounds__(256) void dino_loss_fwd_kernel(const float* __restrict__ S, long lds, const float* __restrict__ T, long ldt,
                                                            const float* __restrict__ c, int V, int B, int K, int col_tiles, long items, float as,
                                                            float at, float* __restrict__ ws) {
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rec = 6 + 4 * V;
    for (long it = (long)blockIdx.x * DL_WAVES + w; it < items; it += (long)gridDim.x * DL_WAVES) {
        const int b = (int)(it / col_tiles), tile0 = (int)(it - (long)b * col_tiles) * DL_TILE;
        float* out = ws + it * rec;
        float cur[DL_SLOTS], nxt[DL_SLOTS], e0[DL_SLOTS], e1[DL_SLOTS], cc[DL_SLOTS];
        dl_load<VEC>(dl_uniform(c), K, tile0, lane, cc);
        dl_load<VEC>(dl_uniform(T + (long)b * ldt), K, tile0, lane, e0);
        dl_load<VEC>(dl_uniform(T + ((long)B + b) * ldt), K, tile0, lane, e1);
        dl_load<VEC>(dl_uniform(S + (long)b * lds), K, tile0, lane, cur);
        float tm[2], tml[2], tsum[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float(&e)[DL_SLOTS] = i ? e1 : e0;
            float lo[DL_SLOTS];
            float m = -INFINITY;
#pragma unroll
            for (int j = 0; j < DL_SLOTS; ++j) {
                dl_diff(e[j], cc[j], e[j], lo[j]);
                if (dl_col<VEC>(tile0, lane, j) >= K) e[j] = -INFINITY, lo[j] = 0.f;
                m = fmaxf(m, e[j]);
            }
            m = wave_max(m);  // finite: the tile's first column is below K
            float ml = -INFINITY;  // the low part that goes with the maximum: the largest among the columns that hold it
#pragma unroll
            for (int j = 0; j < DL_SLOTS; ++j) ml = e[j] == m ? fmaxf(ml, lo[j]) : ml;
            ml = wave_max(ml);
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < DL_SLOTS; ++j) {
                // every operation rounded on its own, here and below: both load widths must leave the same bits whatever the compiler would contract
                e[j] = __builtin_amdgcn_exp2f(__fmul_rn(__fadd_rn(__fsub_rn(e[j], m), __fsub_rn(lo[j], ml)), at));
                s = __fadd_rn(s, e[j]);
            }
            tm[i] = m;
            tml[i] = ml;
            tsum[i] = wave_sum(s);
        }
        if (lane == 0) {
            out[0] = tm[0]; out[1] = tml[0]; out[2] = tsum[0]; out[3] = tm[1]; out[4] = tml[1]; out[5] = tsum[1];
        }
        for (int v = 0; v < V; ++v) {
            if (v + 1 < V) dl_load<VEC>(dl_uniform(S + ((long)(v + 1) * B + b) * lds), K, tile0, lane, nxt);
            float m = -INFINITY;
#pragma unroll
            for (int j = 0; j < DL_SLOTS; ++j) {
                if (dl_col<VEC>(tile0, lane, j) >= K) cur[j] = -INFINITY;
                m = fmaxf(m, cur[j]);
            }
            m = wave_max(m);
            float s = 0.f, d0 = 0.f, d1 = 0.f;
#pragma unroll
            for (int j = 0; j < DL_SLOTS; ++j) {
                s = __fadd_rn(s, __builtin_amdgcn_exp2f(__fmul_rn(__fsub_rn(cur[j], m), as)));
                const float x = dl_col<VEC>(tile0, lane, j) < K ? __fsub_rn(cur[j], m) : 0.f;  // relative to the view's tile max: no S-sized terms to cancel
                d0 = __fmaf_rn(e0[j], x, d0);
                d1 = __fmaf_rn(e1[j], x, d1);
            }
            s = wave_sum(s);
            d0 = wave_sum(d0);
            d1 = wave_sum(d1);
            if (lane == 0) {
                float* o = out + 6 + 4 * v;
                o[0] = m; o[1] = s; o[2] = d0; o[3] = d1;
            }
#pragma unroll
            for (int j = 0; j < DL_SLOTS; ++j) cur[j] = nxt[j];
        }
    }
}

// blocks [0, B): the records of batch row b merged in tile order.  blocks [B, ...): tsum over 64 VEC columns per block, four row groups of 64 lanes;
// group g adds the rows g, g + 4, ... of T's 2 B rows in row order and the four groups are added in group order, in double.
template <int VEC>
__global__ __launch_bounds__(256) void dino_loss_finish_kernel(const float* __restrict__ ws, int V, int B, int K, int col_tiles, float as, float at,
                                                               double inv_ts, float* __restrict__ s_stats, float* __restrict__ t_stats,
                                                               double* __restrict__ rowloss, const float* __restrict__ T, long ldt,
                                                               float* __restrict__ tsum) {
    __shared__ double red[256];
    __shared__ double csum[4 * 64 * 4];
    if ((int)blockIdx.x < B) {
        const int b = blockIdx.x, rec = 6 + 4 * V;
        const float* p = ws + (long)b * col_tiles * rec;  // per tile: (max hi, max lo, sum) of teacher 0, of teacher 1, then the views
        float M0 = -INFINITY, M1 = -INFINITY, L0 = -INFINITY, L1 = -INFINITY;
        for (int j = 0; j < col_tiles; ++j) {
            M0 = fmaxf(M0, p[(long)j * rec]);
            M1 = fmaxf(M1, p[(long)j * rec + 3]);
        }
        for (int j = 0; j < col_tiles; ++j) {
            if (p[(long)j * rec] == M0) L0 = fmaxf(L0, p[(long)j * rec + 1]);
            if (p[(long)j * rec + 3] == M1) L1 = fmaxf(L1, p[(long)j * rec + 4]);
        }
        // a tile's rescale: exp2 of ((hi_j - M) + (lo_j - L)) at
        auto wt = [&](int j, int i) { const float* t = p + (long)j * rec + 3 * i; return ((double)(t[0] - (i ? M1 : M0)) + (double)(t[1] - (i ? L1 : L0))) * (double)at; };
        float Z0 = 0.f, Z1 = 0.f;  // the backward's statistics, in float; the loss takes the same sums in double
        double Y0 = 0.0, Y1 = 0.0;
        for (int j = 0; j < col_tiles; ++j) {
            Z0 = __fmaf_rn(p[(long)j * rec + 2], exp2f((float)wt(j, 0)), Z0);  // written out: the two instantiations must round alike
            Z1 = __fmaf_rn(p[(long)j * rec + 5], exp2f((float)wt(j, 1)), Z1);
            Y0 += (double)p[(long)j * rec + 2] * exp2(wt(j, 0));
            Y1 += (double)p[(long)j * rec + 5] * exp2(wt(j, 1));
        }
        if (threadIdx.x == 0 && t_stats) {
            float* t0 = t_stats + 3 * (long)b;
            float* t1 = t_stats + 3 * ((long)B + b);
            t0[0] = M0; t0[1] = L0; t0[2] = Z0;
            t1[0] = M1; t1[1] = L1; t1[2] = Z1;
        }
        double acc = 0.0;
        for (int v = threadIdx.x; v < V; v += 256) {
            const float* r = p + 6 + 4 * v;
            float M = -INFINITY;
            for (int j = 0; j < col_tiles; ++j) M = fmaxf(M, r[(long)j * rec]);
            // <q_i, S_v> - M = sum_j (d_ij + (m_vj - M) s_ij) w_ij / Y_i with s_ij, w_ij the teacher's tile sum and its rescale: the weights s_ij w_ij / Y_i
            // add up to 1, so the row maximum M leaves the loss term exactly (m_v of it from the lse, one per teacher from the dots)
            float Z = 0.f;
            double Y = 0.0, D0 = 0.0, D1 = 0.0;
            for (int j = 0; j < col_tiles; ++j) {
                const float* q = r + (long)j * rec;
                const float* t = p + (long)j * rec;
                Z = __fmaf_rn(q[1], exp2f(__fmul_rn(__fsub_rn(q[0], M), as)), Z);
                Y += (double)q[1] * exp2((double)(q[0] - M) * (double)as);
                D0 += ((double)q[2] + (double)(q[0] - M) * (double)t[2]) * exp2(wt(j, 0));
                D1 += ((double)q[3] + (double)(q[0] - M) * (double)t[5]) * exp2(wt(j, 1));
            }
            if (s_stats) {
                s_stats[2 * ((long)v * B + b)] = M;
                s_stats[2 * ((long)v * B + b) + 1] = Z;
            }
            const double dot = (v != 0 ? D0 / Y0 : 0.0) + (v != 1 ? D1 / Y1 : 0.0);
            acc += (v < 2 ? 1.0 : 2.0) * log(Y) - dot * inv_ts;
        }
        red[threadIdx.x] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
            const int nt = V < 256 ? V : 256;
            for (int k = 0; k < nt; ++k) t += red[k];
            rowloss[b] = t;
        }
        return;
    }
    const int cb = blockIdx.x - B, lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long col0 = ((long)cb * 64 + lane) * VEC;
    double a[VEC];  // in double: 2 B terms per column, and a sequential float sum of thousands of rows would carry their rounding into the centre
#pragma unroll
    for (int e = 0; e < VEC; ++e) a[e] = 0.0;
    if (col0 < K) {  // VEC == 4: K % 4 == 0, the four columns are below K together
#pragma unroll 8
        for (int r = g; r < 2 * B; r += 4) {
            if constexpr (VEC == 4) {
                const float4 t = *reinterpret_cast<const float4*>(T + (long)r * ldt + col0);
                a[0] += t.x; a[1] += t.y; a[2] += t.z; a[3] += t.w;
            } else {
                a[0] += T[(long)r * ldt + col0];
            }
        }
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) csum[(g * 64 + lane) * 4 + e] = a[e];
    __syncthreads();
    if (g == 0 && col0 < K) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) t += csum[(k * 64 + lane) * 4 + e];
            tsum[col0 + e] = (float)t;
        }
    }
}

// loss[0] = (sum_b rowloss[b]) / (n B): thread t adds the rows t, t + 256, ... in row order, thread 0 adds the threads in thread order
__global__ __launch_bounds__(256) void dino_loss_sum_kernel(const double* __restrict__ rowloss, int B, double scale, float* __restrict__ loss) {
    __shared__ double red[256];
    double t = 0.0;
    for (int b = threadIdx.x; b < B; b += 256) t += rowloss[b];
    red[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        const int nt = B < 256 ? B : 256;
        for (int k = 0; k < nt; ++k) s += red[k];
        loss[0] = (float)(s * scale);
    }
}

template <int VEC>
__global__ __launch_bounds__(256) void dino_loss_bwd_kernel(const float* __restrict__ S, long lds, const float* __restrict__ T, long ldt,
                                                            const float* __restrict__ c, const float* __restrict__ s_stats,
                                                            const float* __restrict__ t_stats, const float* __restrict__ g, int V, int B, int K,
                                                            int col_tiles, long items, float as, float at, float c0, float* __restrict__ dS,
                                                            long ldd) {
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float coef = g[0] * c0;
    for (long it = (long)blockIdx.x * DL_WAVES + w; it < items; it += (long)gridDim.x * DL_WAVES) {
        const int b = (int)(it / col_tiles), tile0 = (int)(it - (long)b * col_tiles) * DL_TILE;
        float cur[DL_SLOTS], nxt[DL_SLOTS], q0[DL_SLOTS], q1[DL_SLOTS], cc[DL_SLOTS];
        dl_load<VEC>(dl_uniform(c), K, tile0, lane, cc);
        dl_load<VEC>(dl_uniform(T + (long)b * ldt), K, tile0, lane, q0);
        dl_load<VEC>(dl_uniform(T + ((long)B + b) * ldt), K, tile0, lane, q1);
        dl_load<VEC>(dl_uniform(S + (long)b * lds), K, tile0, lane, cur);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float(&q)[DL_SLOTS] = i ? q1 : q0;
            const float* ts = t_stats + 3 * ((long)i * B + b);
            const float M = ts[0], L = ts[1], inv = 1.0f / ts[2];
#pragma unroll
            for (int j = 0; j < DL_SLOTS; ++j) {  // every operation rounded on its own: both load widths must give the same bits
                float hi, lo;
                dl_diff(q[j], cc[j], hi, lo);
                q[j] = dl_rounded(__fmul_rn(__builtin_amdgcn_exp2f(__fmul_rn(__fadd_rn(__fsub_rn(hi, M), __fsub_rn(lo, L)), at)), inv));
            }
        }
        for (int v = 0; v < V; ++v) {
            if (v + 1 < V) dl_load<VEC>(dl_uniform(S + ((long)(v + 1) * B + b) * lds), K, tile0, lane, nxt);
            const float M = s_stats[2 * ((long)v * B + b)], inv = 1.0f / s_stats[2 * ((long)v * B + b) + 1];
            const float mv = v < 2 ? 1.f : 2.f, w0 = v != 0 ? 1.f : 0.f, w1 = v != 1 ? 1.f : 0.f;
            float* drow = dS + ((long)v * B + b) * ldd;
#pragma unroll
            for (int j = 0; j < DL_SLOTS; ++j) {
                const float pj = dl_rounded(__fmul_rn(__builtin_amdgcn_exp2f(__fmul_rn(__fsub_rn(cur[j], M), as)), inv));
                const float Q = __fadd_rn(dl_rounded(__fmul_rn(w0, q0[j])), dl_rounded(__fmul_rn(w1, q1[j])));
                cur[j] = __fmul_rn(coef, __fsub_rn(dl_rounded(__fmul_rn(mv, pj)), Q));
            }
            if constexpr (VEC == 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int col = dl_col<VEC>(tile0, lane, 4 * u);
                    if (col < K) *reinterpret_cast<float4*>(drow + col) = make_float4(cur[4 * u], cur[4 * u + 1], cur[4 * u + 2], cur[4 * u + 3]);
                }
            } else {
#pragma unroll
                for (int j = 0; j < DL_SLOTS; ++j) {
                    const int col = dl_col<VEC>(tile0, lane, j);
                    if (col < K) drow[col] = cur[j];
                }
            }
#pragma unroll
            for (int j = 0; j < DL_SLOTS; ++j) cur[j] = nxt[j];
        }
    }
}

bool dl_aligned(const void* a, const void* b, const void* c, const void* d, long l0, long l1, long l2) {
    return !((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) || ((l0 | l1 | l2) & 3));
}

int dl_check(int V, int B, int K, long lds, long ldt, float ts, float tt) {
    if (V < 2 || B < 1 || K < 1 || lds < K || ldt < K || !(ts > 0.f) || !(tt > 0.f)) return DCV_ERR_SHAPE;
    if (((long)K + DL_TILE) * 4 >= (1L << 31)) return DCV_ERR_UNSUPPORTED;  // a row is one buffer range (the chunk) with 32-bit lane offsets: 2 GB with its last tile
    return DCV_OK;
}

}  // namespace

extern "C" int dcv_dino_loss_plan(int V, int B, int K, int aligned, int* vec, int* tile_cols, int* col_tiles, long* items, int* waves_per_wg,
                                  int* grid, int* passes) {
    if (!vec || !tile_cols || !col_tiles || !items || !waves_per_wg || !grid || !passes) return DCV_ERR_NULL;
    const int rc = dl_check(V, B, K, K, K, 1.f, 1.f);
    if (rc) return rc;
    const DlPlan p = dl_plan(V, B, K, aligned != 0);
    *vec = p.vec;
    *tile_cols = DL_TILE;
    *col_tiles = p.col_tiles;
    *items = p.items;
    *waves_per_wg = DL_WAVES;
    *grid = p.grid;
    *passes = p.passes;
    return DCV_OK;
}

extern "C" long dcv_dino_loss_ws_floats(int V, int B, int K) {
    const int rc = dl_check(V, B, K, K, K, 1.f, 1.f);
    if (rc) return rc;
    return dl_ws_floats(dl_plan(V, B, K, true), B);
}

extern "C" int dcv_dino_loss_fwd(const float* S, long lds, const float* T, long ldt, const float* center, int V, int B, int K, float student_temp,
                                 float teacher_temp, float* loss, float* s_stats, float* t_stats, float* tsum, float* ws, long ws_floats,
                                 void* stream) {
    if (!S || !T || !center || !loss || !ws) return DCV_ERR_NULL;
    const int rc = dl_check(V, B, K, lds, ldt, student_temp, teacher_temp);
    if (rc) return rc;
    if ((((uintptr_t)S | (uintptr_t)T | (uintptr_t)center | (uintptr_t)loss | (uintptr_t)s_stats | (uintptr_t)t_stats | (uintptr_t)tsum) & 3) ||
        ((uintptr_t)ws & 15))
        return DCV_ERR_ALIGN;
    const DlPlan p = dl_plan(V, B, K, dl_aligned(S, T, center, tsum, lds, ldt, 0));
    if (ws_floats < dl_ws_floats(p, B)) return DCV_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const float as = (float)(DL_LOG2E / student_temp), at = (float)(DL_LOG2E / teacher_temp);
    double* rowloss = reinterpret_cast<double*>(ws + p.items * p.rec);  // rec is even: 8-byte aligned
    const int tsum_blocks = tsum ? (K + 64 * p.vec - 1) / (64 * p.vec) : 0;
    if (p.vec == 4) {
        hipLaunchKernelGGL(dino_loss_fwd_kernel<4>, dim3((unsigned)p.grid), dim3(256), 0, st, S, lds, T, ldt, center, V, B, K, p.col_tiles, p.items, as,
                           at, ws);
        DCV_LAUNCH_CHECK();
        hipLaunchKernelGGL(dino_loss_finish_kernel<4>, dim3((unsigned)(B + tsum_blocks)), dim3(256), 0, st, (const float*)ws, V, B, K, p.col_tiles, as,
                           at, 1.0 / (double)student_temp, s_stats, t_stats, rowloss, T, ldt, tsum);
    } else {
        hipLaunchKernelGGL(dino_loss_fwd_kernel<1>, dim3((unsigned)p.grid), dim3(256), 0, st, S, lds, T, ldt, center, V, B, K, p.col_tiles, p.items, as,
                           at, ws);
        DCV_LAUNCH_CHECK();
        hipLaunchKernelGGL(dino_loss_finish_kernel<1>, dim3((unsigned)(B + tsum_blocks)), dim3(256), 0, st, (const float*)ws, V, B, K, p.col_tiles, as,
                           at, 1.0 / (double)student_temp, s_stats, t_stats, rowloss, T, ldt, tsum);
    }
    DCV_LAUNCH_CHECK();
    hipLaunchKernelGGL(dino_loss_sum_kernel, dim3(1), dim3(256), 0, st, (const double*)rowloss, B, 1.0 / ((2.0 * V - 2.0) * B), loss);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

extern "C" int dcv_dino_loss_bwd(const float* S, long lds, const float* T, long ldt, const float* center, const float* s_stats,
                                 const float* t_stats, const float* g, int V, int B, int K, float student_temp, float teacher_temp, float* dS,
                                 long ldd, void* stream) {
    if (!S || !T || !center || !s_stats || !t_stats || !g || !dS) return DCV_ERR_NULL;
    const int rc = dl_check(V, B, K, lds, ldt, student_temp, teacher_temp);
    if (rc) return rc;
    if (ldd < K) return DCV_ERR_SHAPE;
    if (((uintptr_t)S | (uintptr_t)T | (uintptr_t)center | (uintptr_t)s_stats | (uintptr_t)t_stats | (uintptr_t)g | (uintptr_t)dS) & 3)
        return DCV_ERR_ALIGN;
    const DlPlan p = dl_plan(V, B, K, dl_aligned(S, T, center, dS, lds, ldt, ldd));
    hipStream_t st = (hipStream_t)stream;
    const float as = (float)(DL_LOG2E / student_temp), at = (float)(DL_LOG2E / teacher_temp);
    const float c0 = 1.0f / ((2.0f * V - 2.0f) * B * student_temp);
    if (p.vec == 4)
        hipLaunchKernelGGL(dino_loss_bwd_kernel<4>, dim3((unsigned)p.grid), dim3(256), 0, st, S, lds, T, ldt, center, s_stats, t_stats, g, V, B, K,
                           p.col_tiles, p.items, as, at, c0, dS, ldd);
    else
        hipLaunchKernelGGL(dino_loss_bwd_kernel<1>, dim3((unsigned)p.grid), dim3(256), 0, st, S, lds, T, ldt, center, s_stats, t_stats, g, V, B, K,
                           p.col_tiles, p.items, as, at, c0, dS, ldd);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}
