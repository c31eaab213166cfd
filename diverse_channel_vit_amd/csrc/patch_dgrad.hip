// Input-image gradient of the patch tokeniser: the adjoint of dcv_im2col_bf16 composed with the patch projection (Conv3d with stride =
// kernel, dichavit.py:377), i.e. one GEMM and a col2im that is a pure permutation — every pixel is written exactly once, no atomics:
//
//     dx[b, ch_idx[c], i*P+u, j*P+v] = scale[c] * sum_d dY[(b*C + c)*n + i*wp + j, d] * W[d, u*P+v]
//
// patch_dgrad_kernel: persistent, 8 waves, one workgroup per CU.  The workgroup holds a Q-column slice of W^T ([Q][D] bf16, transposed once
// on its way into LDS from the straight [D, P*P] operand copy the forward used) and its waves walk tiles of 16 tokens that lie in ONE patch
// row of one (b, c) plane.  The MFMA computes out^T = W^T . dY^T (16x16x32: rows = pixels u*P+v of the patch, columns = tokens), so lane l
// ends with 4 consecutive pixels v .. v+3 of token l & 15: a float4, and the 64 lanes of one store instruction cover a contiguous run of
// 16 tokens * P floats of one image row (1 KB at P = 16) — whole cache lines, no half-line segments.  dY (bf16, 16-byte loads) is read once
// per slice; the next tile's fragments are loaded before the current tile is multiplied.
// patch_dgrad_zero_kernel: the elements the GEMM does not reach — channels outside ch_idx and the border the conv drops — get 0.
#include "dcv_common.hpp"
#include "../../include/dcv.h"

namespace {

constexpr int PD_WAVES = 8;
constexpr int PD_THREADS = PD_WAVES * 64;

template <int D>
__device__ __forceinline__ void pd_load(bf16x8 (&f)[D / 32], const bf16_t* __restrict__ dY, long t, int chunks, int wp, int n, int lane,
                                        bool& valid) {
    const int jc = (int)(t % chunks);
    const long r = t / chunks;  // = bc * hp + i
    const int j = jc * 16 + (lane & 15);
    valid = j < wp;
    // token row (b*C + c)*n + i*wp + j, with r = (b*C + c)*hp + i and n = hp*wp
    const long row = (r / (n / wp)) * n + (r % (n / wp)) * wp + j;
    const uint4* src = reinterpret_cast<const uint4*>(dY + row * D + 8 * (lane >> 4));
#pragma unroll
    for (int ks = 0; ks < D / 32; ++ks) f[ks] = valid ? as_bf16x8(src[4 * ks]) : bf16x8{};
}

struct PdTile {
    const char* smem;
    const int* ch_idx;
    const float* scale;
    float* dx;
    int Ct, C, H, W, hp, chunks, q0, lane;
};

// one tile: out^T [Q pixels, 16 tokens] = W^T slice . dY^T, scaled, stored as float4 runs of image rows
template <int P, int D, int Q>
__device__ __forceinline__ void pd_tile(const PdTile& a, const bf16x8 (&f)[D / 32], bool ok, long t) {
    constexpr int KS = D / 32, NB = Q / 16, PITCH = D + 8;
    const int lane = a.lane;
    int aoff = ((lane & 15) * PITCH + 8 * (lane >> 4)) * 2;
    asm volatile("" : "+v"(aoff));  // opaque per tile: keeps the W^T fragment reads inside the tile loop (hoisted, they would need NB*KS*4 VGPRs)
    f32x4 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) acc[nb] = mfma16(as_bf16x8(lds_read128(a.smem, aoff + (nb * 16 * PITCH + 32 * ks) * 2)), f[ks], acc[nb]);
    }
    if (!ok) return;
    const int jc = (int)(t % a.chunks);
    const long r = t / a.chunks;
    const int i = (int)(r % a.hp);
    const long bc = r / a.hp;
    const int c = (int)(bc % a.C);
    const long b = bc / a.C;
    const float sc = a.scale ? a.scale[c] : 1.f;
    const int j = jc * 16 + (lane & 15);
    float* plane = a.dx + ((size_t)b * a.Ct + a.ch_idx[c]) * a.H * a.W;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int pp = a.q0 + nb * 16 + 4 * (lane >> 4);  // pixels pp .. pp+3 share u (P % 4 == 0)
        const int u = pp / P, v = pp % P;
        *reinterpret_cast<float4*>(plane + (size_t)(i * P + u) * a.W + j * P + v) =
            make_float4(acc[nb][0] * sc, acc[nb][1] * sc, acc[nb][2] * sc, acc[nb][3] * sc);
    }
}

template <int P, int D, int Q>
__global__ __launch_bounds__(PD_THREADS) void patch_dgrad_kernel(const bf16_t* __restrict__ dY, const bf16_t* __restrict__ Wb,
                                                                 const int* __restrict__ ch_idx, const float* __restrict__ scale,
                                                                 float* __restrict__ dx, int Ct, int C, int H, int W, int hp, int wp,
                                                                 int chunks, long tiles, int S) {
    constexpr int PP = P * P;
    constexpr int KS = D / 32;     // 16x16x32 k-steps
    constexpr int PITCH = D + 8;   // bf16 per LDS row: 16 bytes of padding keep 8 consecutive rows on distinct banks for ds_read_b128
    __shared__ __attribute__((aligned(16))) char smem[Q * PITCH * 2];
    bf16_t* sW = reinterpret_cast<bf16_t*>(smem);
    const int s = blockIdx.x % S;  // pixel slice [q0, q0 + Q) of this workgroup
    const int g = blockIdx.x / S, G = gridDim.x / S;
    const int q0 = s * Q;
    // W [D, PP] (pixels contiguous) -> sW[p][d]: coalesced 2-byte reads along p, transposed writes; once per workgroup
    for (int e = threadIdx.x; e < Q * D; e += PD_THREADS) {
        const int d = e / Q, p = e % Q;
        sW[p * PITCH + d] = Wb[(size_t)d * PP + q0 + p];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = hp * wp;
    const long stride = (long)G * PD_WAVES;
    long t = (long)g * PD_WAVES + wave;
    if (t >= tiles) return;
    bf16x8 f0[KS], f1[KS];
    bool ok0, ok1 = false;
    pd_load<D>(f0, dY, t, chunks, wp, n, lane, ok0);
    const PdTile tl{smem, ch_idx, scale, dx, Ct, C, H, W, hp, chunks, q0, lane};
    for (;;) {  // two register buffers in turn: the next tile's loads are in flight while this one is multiplied
        const long t1 = t + stride;
        if (t1 < tiles) pd_load<D>(f1, dY, t1, chunks, wp, n, lane, ok1);
        pd_tile<P, D, Q>(tl, f0, ok0, t);
        if (t1 >= tiles) break;
        const long t2 = t1 + stride;
        if (t2 < tiles) pd_load<D>(f0, dY, t2, chunks, wp, n, lane, ok0);
        pd_tile<P, D, Q>(tl, f1, ok1, t1);
        if (t2 >= tiles) break;
        t = t2;
    }
}

// zeros of dx [B, Ct, H, W] outside the GEMM's reach: whole planes of channels not in ch_idx, and rows >= Hh / columns >= Ww of the others
__global__ __launch_bounds__(256) void patch_dgrad_zero_kernel(const int* __restrict__ ch_idx, float* __restrict__ dx, int Ct, int C, int H,
                                                               int W, int Hh, int Ww, long planes) {
    const int W4 = W / 4, Ww4 = Ww / 4;
    const long per = (long)H * W4;
    for (long pl = blockIdx.y; pl < planes; pl += gridDim.y) {
        const int ct = (int)(pl % Ct);
        bool used = false;
        for (int c = 0; c < C; ++c) used |= ch_idx[c] == ct;
        if (used && Hh == H && Ww == W) continue;
        float4* out = reinterpret_cast<float4*>(dx + pl * H * W);
        for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < per; e += (long)gridDim.x * 256) {
            const int y = (int)(e / W4), x4 = (int)(e % W4);
            if (!used || y >= Hh || x4 >= Ww4) out[e] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

template <int P, int D, int Q>
void pd_launch(const void* dY, const void* Wb, const int* ch_idx, const float* scale, float* dx, int B, int Ct, int C, int H, int W, int cus,
               hipStream_t stream) {
    constexpr int S = P * P / Q;
    const int hp = H / P, wp = W / P, chunks = (wp + 15) / 16;
    const long tiles = (long)B * C * hp * chunks;
    long G = (tiles + PD_WAVES - 1) / PD_WAVES;
    const long cap = cus / S > 0 ? cus / S : 1;
    if (G > cap) G = cap;
    hipLaunchKernelGGL((patch_dgrad_kernel<P, D, Q>), dim3((unsigned)(G * S)), dim3(PD_THREADS), 0, stream, (const bf16_t*)dY,
                       (const bf16_t*)Wb, ch_idx, scale, dx, Ct, C, H, W, hp, wp, chunks, tiles, S);
}

}  // namespace

extern "C" int dcv_patch_dgrad(const void* dY, const void* W_bf16, const int* ch_idx, const float* scale, float* dx, int B, int Ct, int C,
                               int H, int W, int P, int D, void* stream) {
    if (!dY || !W_bf16 || !ch_idx || !dx) return DCV_ERR_NULL;
    // the shapes dcv_im2col_bf16 accepts, plus C <= Ct (ch_idx holds distinct positions of [0, Ct))
    if (B <= 0 || C <= 0 || Ct <= 0 || C > Ct || P <= 0 || (P & 3) || (W & 3) || H < P || W < P || D <= 0) return DCV_ERR_SHAPE;
    if ((P != 8 && P != 16) || (D != 192 && D != 384 && D != 768)) return DCV_ERR_UNSUPPORTED;
    if (((uintptr_t)dY & 15) || ((uintptr_t)dx & 15)) return DCV_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    const int cus = dcv_cu_count();
    // Q: pixel columns of W^T one workgroup holds in LDS (Q * (D + 8) * 2 bytes <= 100 KB)
    if (P == 16) {
        if (D == 192) pd_launch<16, 192, 256>(dY, W_bf16, ch_idx, scale, dx, B, Ct, C, H, W, cus, s);
        else if (D == 384) pd_launch<16, 384, 128>(dY, W_bf16, ch_idx, scale, dx, B, Ct, C, H, W, cus, s);
        else pd_launch<16, 768, 64>(dY, W_bf16, ch_idx, scale, dx, B, Ct, C, H, W, cus, s);
    } else {
        if (D == 192) pd_launch<8, 192, 64>(dY, W_bf16, ch_idx, scale, dx, B, Ct, C, H, W, cus, s);
        else if (D == 384) pd_launch<8, 384, 64>(dY, W_bf16, ch_idx, scale, dx, B, Ct, C, H, W, cus, s);
        else pd_launch<8, 768, 64>(dY, W_bf16, ch_idx, scale, dx, B, Ct, C, H, W, cus, s);
    }
    DCV_LAUNCH_CHECK();
    const int Hh = (H / P) * P, Ww = (W / P) * P;
    if (C < Ct || Hh != H || Ww != W) {  // C == Ct: every channel is in ch_idx (distinct positions)
        const long planes = (long)B * Ct;
        long gx = ((long)H * (W / 4) + 255) / 256;
        if (gx > 64) gx = 64;
        const long gy = planes < 16384 ? planes : 16384;
        hipLaunchKernelGGL(patch_dgrad_zero_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, s, ch_idx, dx, Ct, C, H, W, Hh, Ww, planes);
        DCV_LAUNCH_CHECK();
    }
    return DCV_OK;
}
