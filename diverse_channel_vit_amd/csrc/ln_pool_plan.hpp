// The launch plan that the channel-pool LayerNorm kernel (ln_pool.hip) and its adjoint (ln_pool_bwd.hip) share: how a segment's n_p rows are cut
// into splits, and which shapes both take.  One definition, so "the same cut" holds in every build, variant builds (-DDCV_LP_TARGET_WGS) included.
#pragma once

namespace {

constexpr int LP_MAXV_MAX = 4;       // float4 per lane: D <= 64 * 4 * 4 = 1024; instantiated for 2 (D <= 512) and 4, as ln_fwd_kernel
#ifndef DCV_LP_TARGET_WGS
#define DCV_LP_TARGET_WGS 2048  // variant builds (tools/intermediate_layers_bench.py --variants): 512 = one workgroup per segment at the headline shape
#endif
constexpr long LP_TARGET_WGS = DCV_LP_TARGET_WGS;  // workgroups asked for: 8 x 4 waves per CU of a 256-CU chip at 2048
constexpr int LP_MIN_ROWS = 8;                     // rows per split at least (two per wave)

struct LpPlan {
    int S;  // splits per segment
    int R;  // rows per split (the last one may hold fewer)
};

inline LpPlan lp_plan(int B, int C, int n_p) {
    const long segs = (long)B * C;
    long s0 = (LP_TARGET_WGS + segs - 1) / segs;
    const long cap = n_p / LP_MIN_ROWS > 1 ? n_p / LP_MIN_ROWS : 1;
    if (s0 > cap) s0 = cap;
    if (s0 < 1) s0 = 1;
    LpPlan p;
    p.R = (int)((n_p + s0 - 1) / s0);
    p.S = (n_p + p.R - 1) / p.R;
    return p;
}

inline bool lp_shape_ok(int B, int C, int n_p, int D) {
    if (B <= 0 || C <= 0 || n_p <= 0 || D <= 0 || (D & 3) || D > 64 * 4 * LP_MAXV_MAX) return false;
    // grid and index arithmetic stay inside int: segments, workgroups and the rows of one image
    if ((long)B * C > (1L << 24) || (long)C * n_p > (1L << 28)) return false;
    return true;
}

}  // namespace
