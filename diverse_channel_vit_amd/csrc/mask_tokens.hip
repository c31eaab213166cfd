// The learned mask token of masked-patch distillation (iBOT), at the tokeniser's seam.
//
//  mask_tokens_fwd : after the EPI_PATCH GEMM and before block 0: every token row (b, t = c n + i) with mask[b, t] != 0 gets
//                    xs[b, 1 + t, :] = mask_token + (E[c] + pos[1 + i]) — the association order of the EPI_PATCH epilogue's (acc + bias) + (E + pos),
//                    so a masked row has the bits the tokeniser writes for a row whose projection output equals mask_token.  Unmasked rows, the
//                    CLS rows and Y (the pre-embedding projection output the ortho regulariser reads) are not touched.
//  mask_tokens_bwd : after patch_bwd: dmask_token[D] += sum over the masked rows of dx0[b, 1 + t, :], and the masked rows of dY_bf16 become
//                    bf16(dYloss row) (the ortho gradient, which still acts on the real patch) or 0: the weight-gradient GEMM, the bias sum and
//                    the input gradient then see no token gradient from a masked patch.  dE and dpos keep the masked rows' dx (patch_bwd added
//                    them).  No atomics in either reduction mode of the library: the flat (b, t) range is cut into parts of MT_ROWS consecutive
//                    rows, a part's sub-lane s adds its masked rows s, s + bpar, ... in row order to a partial in the workspace, and det_reduce adds
//                    the partials in index order.  The partition is fixed by (B, C, n, D): where the mask is set changes which rows are added,
//                    not the order among them.
// The per-token positional mode of the model (one "channel" of C n positions) is the same call with C = 1.
#include "dcv_common.hpp"

namespace {

constexpr int MT_ROWS = 256;  // rows of a part

__global__ __launch_bounds__(256) void mask_tokens_fwd_kernel(float* __restrict__ xs, const unsigned char* __restrict__ mask,
                                                              const float* __restrict__ mt, const float* __restrict__ E,
                                                              const float* __restrict__ pos, long rows, int T, int n, int D) {
    // one wave per token row, four rows per workgroup
    const int lane = threadIdx.x & 63, nv = D >> 2;
    for (long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (long)gridDim.x * 4) {
        if (!mask[row]) continue;
        const long b = row / T;
        const int t = (int)(row - b * T), c = t / n, i = t - c * n;
        float4* dst = reinterpret_cast<float4*>(xs + (b * (T + 1) + 1 + t) * D);
        for (int v = lane; v < nv; v += 64) {
            const float4 m = reinterpret_cast<const float4*>(mt)[v];
            const float4 e = reinterpret_cast<const float4*>(E + (long)c * D)[v];
            const float4 p = reinterpret_cast<const float4*>(pos + (long)(1 + i) * D)[v];
            dst[v] = make_float4(m.x + (e.x + p.x), m.y + (e.y + p.y), m.z + (e.z + p.z), m.w + (e.w + p.w));
        }
    }
}

__global__ __launch_bounds__(256) void mask_tokens_bwd_kernel(const float* __restrict__ dx0, const unsigned char* __restrict__ mask,
                                                              const float* __restrict__ dYloss, bf16_t* __restrict__ dYb, long rows, int T,
                                                              int D, float* __restrict__ part) {
    const int nv = D >> 2, bpar = 256 / nv;
    const int v = threadIdx.x % nv, sub = threadIdx.x / nv;
    if (sub >= bpar) return;
    const long r0 = (long)blockIdx.x * MT_ROWS, r1 = r0 + MT_ROWS < rows ? r0 + MT_ROWS : rows;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long row = r0 + sub; row < r1; row += bpar) {
        if (!mask[row]) continue;
        const long b = row / T;
        const float4 g = reinterpret_cast<const float4*>(dx0 + (b * (T + 1) + 1 + (row - b * T)) * D)[v];
        a.x += g.x; a.y += g.y; a.z += g.z; a.w += g.w;
        uint2 o = make_uint2(0u, 0u);
        if (dYloss) {
            const float4 l = reinterpret_cast<const float4*>(dYloss + row * D)[v];
            o = pack4_bf16(l.x, l.y, l.z, l.w);
        }
        reinterpret_cast<uint2*>(dYb + row * D)[v] = o;
    }
    reinterpret_cast<float4*>(part + ((long)blockIdx.x * bpar + sub) * D)[v] = a;  // every slot is written, a part without masked rows with 0
}

int mt_check(int B, int C, int n, int D) {
    if (B <= 0 || C <= 0 || n <= 0 || D <= 0 || (D & 3) || D > 1024) return DCV_ERR_SHAPE;
    return DCV_OK;
}

long mt_parts(int B, int C, int n, int D) { return (((long)B * C * n + MT_ROWS - 1) / MT_ROWS) * (256 / (D >> 2)); }

}  // namespace

extern "C" int dcv_mask_tokens_fwd(float* xs, const unsigned char* mask, const float* mask_token, const float* E, const float* pos, int B, int C,
                                   int n, int D, void* stream) {
    if (!xs || !mask || !mask_token || !E || !pos) return DCV_ERR_NULL;
    const int rc = mt_check(B, C, n, D);
    if (rc) return rc;
    if (((uintptr_t)xs | (uintptr_t)mask_token | (uintptr_t)E | (uintptr_t)pos) & 15) return DCV_ERR_ALIGN;
    const long rows = (long)B * C * n;
    long grid = (rows + 3) / 4;
    if (grid > 8192) grid = 8192;
    hipLaunchKernelGGL(mask_tokens_fwd_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, xs, mask, mask_token, E, pos, rows, C * n, n,
                       D);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

extern "C" long dcv_mask_tokens_bwd_ws_floats(int B, int C, int n, int D) {
    const int rc = mt_check(B, C, n, D);
    if (rc) return rc;
    return mt_parts(B, C, n, D) * D;
}

extern "C" int dcv_mask_tokens_bwd(const float* dx0, const unsigned char* mask, const float* dYloss, void* dY_bf16, float* dmask_token, int B,
                                   int C, int n, int D, float* ws, long ws_floats, void* stream) {
    if (!dx0 || !mask || !dY_bf16 || !dmask_token || !ws) return DCV_ERR_NULL;
    const int rc = mt_check(B, C, n, D);
    if (rc) return rc;
    if (((uintptr_t)dx0 | (uintptr_t)dYloss | (uintptr_t)dmask_token | (uintptr_t)ws) & 15 || ((uintptr_t)dY_bf16 & 7)) return DCV_ERR_ALIGN;
    const long parts = mt_parts(B, C, n, D), rows = (long)B * C * n;
    if (ws_floats < parts * D || parts > 0x7fffffffL) return DCV_ERR_SHAPE;
    const long blocks = (rows + MT_ROWS - 1) / MT_ROWS;
    hipLaunchKernelGGL(mask_tokens_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dx0, mask, dYloss, (bf16_t*)dY_bf16, rows,
                       C * n, D, ws);
    DCV_LAUNCH_CHECK();
    if (!det_reduce(ws, (int)parts, D, dmask_token, D, D, D, nullptr, 0, (hipStream_t)stream)) return DCV_ERR_LAUNCH;
    return DCV_OK;
}
