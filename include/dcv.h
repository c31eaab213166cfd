/* libdcv_hip.so — C ABI of the MI355X-native DiChaViT training hot path.
 *
 * The reference (chaudatascience/diverse_channel_vit) has NO FFI: its hot path is stock ATen ops
 * called from Python.  The drop-in boundary is therefore the Python plugin contract
 * (models/__init__.py:9 `dichavit`, models/dichavit.py:844-865), mirrored by
 * diverse_channel_vit_amd/dichavit.py.  This header is the native layer beneath it: each entry
 * replaces the ATen op sequence cited next to it.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions: every entry returns 0 or a negative DCV_ERR_* code; never throws, never allocates,
 * never synchronises, never reads the environment; all buffers are device pointers owned by the caller;
 * `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream); entries are re-entrant and
 * graph-capturable: the only process-wide state is a cache of each device's CU count
 * (hipDeviceGetAttribute, read once per device).  Every tuning choice is an explicit argument (the *_ex forms).
 * bf16 buffers are raw 16-bit brain-float; "f32" is IEEE binary32.  Only gfx950 code is built.
 */
#ifndef DCV_H
#define DCV_H
#ifdef __cplusplus
extern "C" {
#endif

#define DCV_OK 0
#define DCV_ERR_SHAPE (-1)
#define DCV_ERR_ALIGN (-2)
#define DCV_ERR_UNSUPPORTED (-3)
#define DCV_ERR_LAUNCH (-4)
#define DCV_ERR_NULL (-5)

/* dcv_gemm_nt epilogues */
#define DCV_EPI_BIAS_BF16 0      /* out bf16 = acc + bias                         (attn.qkv, vit.py:123)            */
#define DCV_EPI_BIAS_GELU_BF16 1 /* z = acc + bias (fp32): out bf16 = GELU_erf'(z), out2 bf16 = GELU_erf(z) (mlp.fc1 + act, vit.py:77-78) */
#define DCV_EPI_BIAS_RESID_F32 2 /* out f32 = (aux f32 ? aux : out) + s (acc + bias) (attn.proj / mlp.fc2 + residual, vit.py:142,397-398);
                                    s = 1, or with aux2 != NULL and T = rows per sample: s = aux2[row / T] — DropPath's per-sample
                                    keep_b / keep_prob (vit.py:37-56) */
#define DCV_EPI_PLAIN_BF16 3     /* out bf16 = acc                                 (input gradients)                */
#define DCV_EPI_GELU_BWD_BF16 4  /* out bf16 = acc * aux bf16, aux = the saved GELU'(z)  (grad through act, vit.py:78)    */
#define DCV_EPI_PATCH 5          /* tokens: out f32[b,1+t,:] = acc + bias + aux[c(t),:] + aux2[1+i(t),:] ;
                                    out2 f32[b*T+t,:] = acc + bias (optional)       (dichavit.py:377,409-415,565)   */

int dcv_version(void);
const char* dcv_error_string(int code);

/* C[M,N] = A[M,K] . W[N,K]^T (bf16 in, f32 accumulate) + epilogue.  K % 64 == 0, N % 8 == 0.
 * Leading dimensions (row strides in elements; every row moves in 16-byte pieces): lda, ldw >= K and ldo >= N, multiples of 8; where the epilogue
 * uses the buffer, ldo2 >= N and ldaux >= N, multiples of 8 for bf16 (GELU's out2, GELU_BWD's aux) and of 4 for fp32 (PATCH's out2; the residual;
 * PATCH's aux and aux2, which share ldaux).  A stride below the width is DCV_ERR_SHAPE (rows would overlap), one off its multiple DCV_ERR_ALIGN; a
 * null optional buffer's stride is not looked at.
 * Replaces F.linear forward / input-gradient and the Conv3d patch projection (on im2col rows). */
int dcv_gemm_nt(const void* A, int lda, const void* W, int ldw, int M, int N, int K, int epilogue, const float* bias,
                void* out, int ldo, void* out2, int ldo2, const void* aux, int ldaux, const float* aux2, int T, int n,
                void* stream);
/* Tile variants of the *_ex forms.  gemm_nt: NARROW = 256 x 128 output tile, WIDE = 256 x 384 (needs N % 384 == 0, not the
 * PATCH epilogue).  gemm_tn_acc: NARROW = 128 x 128, WIDE = 384 x 128 (needs P % 384 == 0, Q % 128 == 0).  AUTO picks by
 * measured shape rules.  Forcing an illegal variant returns DCV_ERR_UNSUPPORTED. */
#define DCV_TILE_AUTO 0
#define DCV_TILE_NARROW 1
#define DCV_TILE_WIDE 2
#define DCV_TILE_PAIR 3 /* dcv_gemm_nt_ex only: 128 x 128 tiles by four-wave workgroups, TWO per CU (one stores while the other computes) */
#define DCV_TILE_ALT 4  /* RETIRED (docs/retired_experiments.md): the number stays reserved so that DCV_TILE_WS / DCV_TILE_AUTO_WS keep their values; dcv_gemm_nt_pick and dcv_gemm_nt_ex answer DCV_ERR_UNSUPPORTED */
#define DCV_TILE_WS 5   /* dcv_gemm_nt_ex only: WEIGHT-STATIONARY kernel for K == 384, N % 384 == 0 and the bf16-output epilogues (BIAS_BF16,
                           BIAS_GELU_BF16, PLAIN_BF16, GELU_BWD_BF16): each workgroup holds one 384-column slice of W in registers and walks 32-row
                           panels of A; needs grid_cap (if set) >= N / 384, ldo2 / ldaux % 8 == 0 and 16-byte aligned out2 / aux / bias.  Outputs are
                           bit-identical to the NARROW / WIDE kernels'.  DCV_ERR_UNSUPPORTED elsewhere, and in builds with -DDCV_NT_WS=0 */
#define DCV_TILE_AUTO_WS 6 /* AUTO's choice, or DCV_TILE_WS where that measured faster (K == 384 products from a few thousand rows on); what
                              dcv_gemm_nt uses */
/* dcv_gemm_nt with its launch controls as arguments: both kernels are persistent (one workgroup per CU walks the output
 * tiles, several rounds when there are more tiles than workgroups); grid_cap > 0 caps the number of workgroups (0 = one per
 * CU of the current device) — the data-parallel backward leaves CUs to RCCL's kernels this way. */
int dcv_gemm_nt_ex(const void* A, int lda, const void* W, int ldw, int M, int N, int K, int epilogue, const float* bias,
                   void* out, int ldo, void* out2, int ldo2, const void* aux, int ldaux, const float* aux2, int T, int n,
                   int grid_cap, int tile, void* stream);

/* dW[P,Q] (f32) += sum_m Y[m,P] * X[m,Q] ; dbias[P] (f32, nullable) += sum_m Y[m,P].  bf16 inputs.  P, Q % 8 == 0; ldy >= P and ldx >= Q,
 * multiples of 8; lddw >= Q (DCV_ERR_SHAPE below the width, DCV_ERR_ALIGN off the multiple; the grouped form checks every item the same way).
 * Replaces the weight/bias gradients of nn.Linear / Conv3d (autograd of vit.py:72-74,123,142; dichavit.py:377). */
int dcv_gemm_tn_acc(const void* Y, int ldy, const void* X, int ldx, int M, int P, int Q, float* dW, int lddw, float* dbias,
                    void* stream);
/* Residual addition AND the LayerNorm that follows it, from the accumulators of one 256 x 384 tile (N must be 384: a tile spans whole rows):
 *   x_out f32 [M,N] = resid + s (A W^T + bias)      (attn.proj / mlp.fc2 + residual, vit.py:397-398; s = branch_scale[row / T] or 1)
 *   u_out bf16 [M,N] = (x_out - mean) * rstd * gamma + beta,   mean / rstd f32 [M]   (norm2 / the next block's norm1, vit.py:397-398; eps as given)
 * = dcv_gemm_nt(DCV_EPI_BIAS_RESID_F32) + dcv_ln_fwd in one launch, without the re-read of x_out.  Statistics are centred (Chan's pairwise
 * combination), as dcv_ln_fwd's.  Returns DCV_ERR_UNSUPPORTED for N != 384.  Alignment (DCV_ERR_ALIGN otherwise): every pointer 16 bytes — u_out
 * included: its rows leave in 16-byte stores — lda, ldw, ldu multiples of 8, ldo, ldr of 4.  lda, ldw >= K and ldo, ldr, ldu >= N, else DCV_ERR_SHAPE. */
int dcv_gemm_nt_resid_ln(const void* A, int lda, const void* W, int ldw, int M, int N, int K, const float* bias, const float* resid, int ldr,
                         const float* branch_scale, int T, float* x_out, int ldo, const float* gamma, const float* beta, float eps,
                         void* u_out, int ldu, float* mean, float* rstd, int grid_cap, void* stream);

/* the variant (DCV_TILE_NARROW / DCV_TILE_WIDE) the *_ex forms launch for a problem — pure functions of their arguments */
int dcv_gemm_nt_pick(int M, int N, int K, int epilogue, int tile);
int dcv_gemm_tn_pick(int M, int P, int Q, int tile);
/* row-tile plan of the 256 x 384 NT kernel (DCV_TILE_WIDE, dcv_gemm_nt_resid_ln) for M rows, N % 384 == 0 columns and `grid` workgroups — host
 * logic, no GPU call: rows [0, 256 n256) in 256-row tiles, the rest in n192 tiles of 192 rows, which fall into the last round(s) of the
 * static walk (tile = round * grid + workgroup) and shorten them.  n192 = 0 wherever that would not lower the most rows a workgroup walks. */
int dcv_gemm_nt384_plan(int M, int N, int grid, int* n256, int* n192);
int dcv_gemm_tn_acc_ex(const void* Y, int ldy, const void* X, int ldx, int M, int P, int Q, float* dW, int lddw, float* dbias,
                       int tile, void* stream);
/* DETERMINISTIC form (the reference trains with cudnn.deterministic = True, utils.py:394-401): the workgroups that split the token
 * rows store their partial tiles to `ws` with plain stores and a second launch adds them to dW / dbias in a fixed order, so two runs on
 * the same inputs give bit-identical gradients (dcv_gemm_tn_acc adds with fp32 atomics in dispatch order).  ws: caller-owned scratch of
 * at least dcv_gemm_tn_det_ws_floats(M, P, Q, tile) floats, 16-byte aligned, contents irrelevant before and after; lddw % 4 == 0. */
long dcv_gemm_tn_det_ws_floats(int M, int P, int Q, int tile);
int dcv_gemm_tn_acc_det(const void* Y, int ldy, const void* X, int ldx, int M, int P, int Q, float* dW, int lddw, float* dbias,
                        int tile, float* ws, long ws_floats, void* stream);

/* Several weight-gradient products over the SAME M token rows in ONE launch (round 3): dW_i[P_i,Q_i] += Y_i[M,P_i]^T X_i[M,Q_i],
 * dbias_i[P_i] += colsum(Y_i) (dbias may be NULL) for i < n <= 8.  Every P_i % 384 == 0 and Q_i % 128 == 0 and the tiles of all products
 * together must fit one resident round (sum of (P_i/384)(Q_i/128) <= CUs), else DCV_ERR_UNSUPPORTED: call the products one by one.  The CUs
 * are filled by the tiles of all products, so each tile is split far fewer ways over the rows than in n separate launches (a block's four
 * gradients: 7 ways instead of 21 / 21 / 28 / 85): a third of the partial-tile traffic and one launch's fixed cost instead of four.
 * ws != NULL: the deterministic form (dcv_gemm_tn_group_ws_floats(items, n, M) floats; partial tiles through ws, fixed-order second pass);
 * ws == NULL: fp32 atomics.  Replaces the four torch.autograd weight-gradient GEMMs of Block.backward (models/vit.py:72-82, 116-142). */
typedef struct dcv_tn_item {
    const void* Y; /* bf16 [M, P], row stride ldy */
    const void* X; /* bf16 [M, Q], row stride ldx */
    float* dW;     /* fp32 [P, Q], row stride lddw, accumulated into */
    float* dbias;  /* fp32 [P] or NULL */
    int ldy, ldx, P, Q, lddw, reserved;
} dcv_tn_item;
long dcv_gemm_tn_group_ws_floats(const dcv_tn_item* items, int n, int M);
int dcv_gemm_tn_group(const dcv_tn_item* items, int n, int M, float* ws, long ws_floats, void* stream);

/* The bias gradient alone (a Linear whose bias is trained and whose weight is frozen): dbias[P] (f32) += sum_m Y[m,P], Y bf16 [M,P] with row
 * stride ldy — the semantics of dcv_gemm_tn_acc's dbias argument without the product.  ALWAYS deterministic (no atomic form): per-workgroup
 * partial sums through ws (at least dcv_bias_grad_ws_floats(M, P) floats, contents irrelevant before and after), added to dbias in workgroup
 * order by a second launch; fp32 accumulation.  One streaming pass over Y in 16-byte loads.  Checked in this order, before any HIP call:
 * Y / dbias / ws NULL -> DCV_ERR_NULL; M < 1, P < 1 or ldy < P -> DCV_ERR_SHAPE; Y, dbias or ws not 16-byte aligned, ldy % 8 != 0 ->
 * DCV_ERR_ALIGN; P % 8 != 0 -> DCV_ERR_UNSUPPORTED, as is a row chunk (rows_per_wg rows of ldy elements) of 2 GB or more; ws_floats too small
 * -> DCV_ERR_SHAPE. */
long dcv_bias_grad_ws_floats(int M, int P);
int dcv_bias_grad(const void* Y, int ldy, int M, int P, float* dbias, float* ws, long ws_floats, void* stream);
/* its launch plan — host logic, no GPU call: the P / 8 16-byte units of a row fall into col_chunks column chunks of at most 64 lanes; one wave
 * step takes rows_per_wave rows of its chunk (8 loads in flight), a workgroup of four waves rows_per_wg; the grid is row_wgs x col_chunks
 * workgroups, capped at 512, and a workgroup walks at most `passes` row chunks (1 below the cap).  ws holds row_wgs * P floats. */
int dcv_bias_grad_plan(int M, int P, int* col_chunks, int* rows_per_wave, int* rows_per_wg, int* row_wgs, int* passes);

/* LayerNorm (eps inside the sqrt, biased variance) — vit.py:361,374 / dichavit.py:651.
 * out is bf16 [M,D] (or f32 when out_is_f32); mean/rstd [M] may be NULL. x rows are x_row_stride floats apart. */
int dcv_ln_fwd(const float* x, long x_row_stride, const float* gamma, const float* beta, void* out, int out_is_f32, float* mean,
               float* rstd, int M, int D, float eps, void* stream);
/* dx_out = (dx_in ? dx_in : 0) + LN'(du) ; dx_bf16 (nullable) = bf16(dx_out) ; dgamma/dbeta += ... */
int dcv_ln_bwd(const void* du, int du_is_f32, const float* x, long x_row_stride, const float* mean, const float* rstd,
               const float* gamma, const float* dx_in, float* dx_out, long dx_row_stride, void* dx_bf16, float* dgamma,
               float* dbeta, int M, int D, void* stream);
/* LayerNorm of a token stream pooled per input channel (ChannelVisionTransformer.get_intermediate_layers, pool="channel"):
 * x f32 [B, N, D] with N = 1 + C * n_p, rows D floats apart (CLS, then the n_p patch tokens of channel 0, 1, ...) ->
 * out f32 [B, 1 + C, D]: row 0 = LN(x[b, 0]) (bit-identical to dcv_ln_fwd's f32 output of that row), row 1 + c = the mean over the n_p
 * rows of channel c of LN(row); gamma / beta are applied once, to the mean of the normalised rows.  Reads x once, never writes the normed
 * tokens.  No atomics, and every summation order is a function of (B, C, n_p, D) alone: bitwise reproducible.  ws: at least
 * dcv_ln_pool_channels_ws_floats(B, C, n_p, D) floats (0 when B * C segments fill the chip: ws may then be NULL), contents irrelevant.
 * D % 4 == 0, D <= 1024 and ws_floats large enough, else DCV_ERR_SHAPE; every pointer 16-byte aligned, else DCV_ERR_ALIGN. */
long dcv_ln_pool_channels_ws_floats(int B, int C, int n_p, int D);
int dcv_ln_pool_channels(const float* x, const float* gamma, const float* beta, float eps, float* out, int B, int C, int n_p, int D,
                         float* ws, long ws_floats, void* stream);
/* Adjoint of dcv_ln_pool_channels (DiChaViT.forward_with_features, pool="channel"): with g = dout[b, 1 + c], h = gamma * g / n_p and
 * x^_i = (x_i - mu_i) rstd_i for row i of segment (b, c),
 *   dx_i += rstd_i (h - mean_D(h) - x^_i mean_D(h x^_i))    (the CLS row: the same with n_p = 1 and g = dout[b, 0]);
 *   dgamma += sum_b dout[b, 0] x^_cls + sum_{b,c} dout[b, 1 + c] (1 / n_p) sum_i x^_i;    dbeta += sum_{b,j} dout[b, j].
 * x f32 [B, N, D], N = 1 + C * n_p; dout f32 [B, 1 + C, D]; dx f32 [B, N, D] is ACCUMULATED in place; dgamma / dbeta f32 [D] are accumulated and
 * may each be NULL (dx has the same bits).  One pass: x is read once, dx read and written once, the broadcast of g never exists in memory;
 * mu and rstd are recomputed from the row exactly as dcv_ln_fwd and dcv_ln_pool_channels form them.  No atomics: every row of dx belongs to one
 * wave, the dgamma partials of the workgroups go through ws and are added in workgroup order, dbeta adds the rows of dout in row order — every
 * order is a function of (B, C, n_p, D) alone, two calls are bit-identical.  The split of a segment's rows over workgroups is that of
 * dcv_ln_pool_channels; ws: at least dcv_ln_pool_channels_bwd_ws_floats(B, C, n_p, D) = (B C S + ceil(B / 4)) D floats (not read when dgamma is
 * NULL), contents irrelevant.  D % 4 == 0, D <= 1024 and ws_floats large enough, else DCV_ERR_SHAPE; every pointer 16-byte aligned, else
 * DCV_ERR_ALIGN. */
long dcv_ln_pool_channels_bwd_ws_floats(int B, int C, int n_p, int D);
int dcv_ln_pool_channels_bwd(const float* x, const float* gamma, float eps, const float* dout, float* dx, float* dgamma, float* dbeta,
                             int B, int C, int n_p, int D, float* ws, long ws_floats, void* stream);

/* DETERMINISTIC forms of the other entries that combine partial sums of several workgroups (LayerNorm's dgamma / dbeta, the tokeniser's
 * d(channel_embed) / d(pos), the diversity loss' per-channel sums, the gradient norm): partials go through `ws` (at least *_det_ws_floats
 * floats, 16-byte aligned, contents irrelevant) and are added in a fixed order by a second launch.  Same arguments and results otherwise.
 * With dcv_gemm_tn_acc_det these make a whole training step bit-reproducible (attention, the NT GEMMs and AdamW never were order-dependent). */
long dcv_ln_bwd_det_ws_floats(int M, int D);
int dcv_ln_bwd_det(const void* du, int du_is_f32, const float* x, long x_row_stride, const float* mean, const float* rstd,
                   const float* gamma, const float* dx_in, float* dx_out, long dx_row_stride, void* dx_bf16, float* dgamma,
                   float* dbeta, int M, int D, float* ws, long ws_floats, void* stream);
long dcv_patch_bwd_det_ws_floats(int B, int C, int n, int D);
int dcv_patch_bwd_det(const float* dx0, const float* dYloss, void* dY_bf16, float* dE, float* dpos, float* dcls, int B, int C, int n,
                      int D, float* ws, long ws_floats, void* stream);
long dcv_ortho_fwd_det_ws_floats(int B, int C, int n, int D);
int dcv_ortho_fwd_det(const float* Y, float* S, float* selfsq, float* tot, float* inv_norm, float* stats, int B, int C, int n, int D,
                      float* ws, long ws_floats, void* stream);
long dcv_sumsq_det_ws_floats(long n);
int dcv_sumsq_acc_det(const float* x, long n, float* acc, float* ws, long ws_floats, void* stream);

/* dcv_ln_bwd with the bf16 copy scaled per sample: dx_bf16 = bf16(bf16_row_scale[row / rows_per_sample] * dx_out) — the copy feeds the
 * backward of the residual branch below this LayerNorm, whose DropPath factor (vit.py:37-56) multiplies that branch's gradient; dx_out itself
 * (the residual stream) is not scaled.  ws NULL: atomic dgamma / dbeta; else the deterministic form (dcv_ln_bwd_det_ws_floats floats). */
int dcv_ln_bwd_scaled(const void* du, int du_is_f32, const float* x, long x_row_stride, const float* mean, const float* rstd,
                      const float* gamma, const float* dx_in, float* dx_out, long dx_row_stride, void* dx_bf16, float* dgamma,
                      float* dbeta, int M, int D, const float* bf16_row_scale, int rows_per_sample, float* ws, long ws_floats, void* stream);

/* softmax(q k^T * scale) v for packed qkv [B,N,3,H,64] bf16 -> o [B,N,H*64] bf16, lse [B,H,N] f32.
 * Replaces Attention.forward's q@k^T / softmax / @v (vit.py:123-141); the [B,H,N,N] matrix is never stored. */
int dcv_attn_fwd(const void* qkv, void* o, float* lse, int B, int N, int H, int head_dim, float scale, void* stream);
/* dqkv [B,N,3,H,64] bf16 from (qkv, o, dO, lse).  ws: f32 workspace of 2*B*H*N floats holding the row statistics
 *   ws[0 .. BHN) = -delta, delta[b,h,q] = sum_d dO*O;  ws[BHN .. 2 BHN) = lse * log2(e).
 * Two launches: dQ (which also writes ws), then dK/dV (which reads it). */
int dcv_attn_bwd(const void* qkv, const void* o, const void* dO, const float* lse, float* ws, void* dqkv, int B, int N,
                 int H, int head_dim, float scale, void* stream);
/* the launches individually (profiling / stream placement).  dcv_attn_bwd_dq fills the dQ slot of dqkv AND ws;
 * dcv_attn_bwd_dkdv fills the dK and dV slots and needs ws filled (by dcv_attn_bwd_dq or by dcv_attn_bwd_delta, which
 * computes only the statistics); its `lse` argument is kept for symmetry and not read. */
int dcv_attn_bwd_delta(const void* o, const void* dO, const float* lse, float* ws, int B, int N, int H, int head_dim, void* stream);
int dcv_attn_bwd_dq(const void* qkv, const void* o, const void* dO, const float* lse, float* ws, void* dqkv, int B, int N, int H,
                    int head_dim, float scale, void* stream);
int dcv_attn_bwd_dkdv(const void* qkv, const void* dO, const float* lse, const float* ws, void* dqkv, int B, int N, int H,
                      int head_dim, float scale, void* stream);
/* Query-row-restricted forms: only the query rows [0, Nq) of every (batch, head) are processed (1 <= Nq <= N); keys and
 * values are always all N rows.  Used for the LAST encoder block, whose output is read at the CLS row only
 * (ChannelVisionTransformer.forward returns norm(x)[:, 0], dichavit.py:651-652): Nq = 1.  Forward writes o / lse rows < Nq
 * only; backward reads dO rows < Nq only, writes dQ = 0 for the rows >= Nq and dK, dV of all keys. */
int dcv_attn_fwd_rows(const void* qkv, void* o, float* lse, int B, int N, int Nq, int H, int head_dim, float scale, void* stream);
int dcv_attn_bwd_rows(const void* qkv, const void* o, const void* dO, const float* lse, float* ws, void* dqkv, int B, int N, int Nq,
                      int H, int head_dim, float scale, void* stream);
int dcv_attn_bwd_dq_rows(const void* qkv, const void* o, const void* dO, const float* lse, float* ws, void* dqkv, int B, int N,
                         int Nq, int H, int head_dim, float scale, void* stream);
int dcv_attn_bwd_dkdv_rows(const void* qkv, const void* dO, const float* lse, const float* ws, void* dqkv, int B, int N, int Nq,
                           int H, int head_dim, float scale, void* stream);

/* Pre-scaled-q forms (round 4).  The q part of qkv holds q * scale * log2(e) — the caller scales the operand copy of W_q and the q part of the
 * bias BEFORE the qkv GEMM (dcv_cast_scaled_ranges), so q is still rounded once.  The score accumulators then start at the row constants (-m,
 * -LSE log2 e, -delta) and p = exp2(accumulator): one vector instruction less per score in each kernel.  Outputs as the plain entries: o, lse
 * (natural log), dqkv with dQ the gradient with respect to the UNSCALED q.  The ws of the _ps pair carries -LSE log2 e: do not mix it with the
 * plain pair's.  Replaces nothing in the reference (vit.py:128-133 computes (q @ k^T) * scale on a materialised matrix). */
int dcv_attn_fwd_rows_ps(const void* qkv, void* o, float* lse, int B, int N, int Nq, int H, int head_dim, void* stream);
int dcv_attn_bwd_rows_ps(const void* qkv, const void* o, const void* dO, const float* lse, float* ws, void* dqkv, int B, int N, int Nq,
                         int H, int head_dim, float scale, void* stream);
int dcv_attn_bwd_dq_rows_ps(const void* qkv, const void* o, const void* dO, const float* lse, float* ws, void* dqkv, int B, int N,
                            int Nq, int H, int head_dim, float scale, void* stream);
int dcv_attn_bwd_dkdv_rows_ps(const void* qkv, const void* dO, const float* lse, const float* ws, void* dqkv, int B, int N, int Nq,
                              int H, int head_dim, float scale, void* stream);

/* Attention probabilities of one block, written once (ChannelVisionTransformer.get_last_selfattention; models/dichavit.py:654-663 returns
 * softmax(q k^T * scale), models/vit.py:128-129): P [B,H,Nq,N] f32 row-major, row pitch exactly N floats, P[b,h,q,k] = exp(q.k scale - lse[b,h,q])
 * for the query rows q < Nq (1 <= Nq <= N) and every key k < N.  qkv [B,N,3,H,64] bf16 and lse [B,H,N] (natural log; rows < Nq read) as
 * dcv_attn_fwd_rows(_ps) produced them; the _ps form takes the pre-scaled q of dcv_attn_fwd_rows_ps.  No atomics: bitwise reproducible, and row
 * q does not depend on Nq.  Store-bound: writes 4 B H Nq N bytes. */
int dcv_attn_probs_rows(const void* qkv, const float* lse, float* P, int B, int N, int Nq, int H, int head_dim, float scale, void* stream);
int dcv_attn_probs_rows_ps(const void* qkv, const float* lse, float* P, int B, int N, int Nq, int H, int head_dim, void* stream);
/* The same probabilities reduced to CHANNEL granularity inside the kernel (ChannelVisionTransformer.get_channel_attention; no counterpart in the
 * reference, whose users reduce get_last_selfattention's map themselves): N = 1 + C * n_p tokens (DCV_ERR_SHAPE otherwise), key segments S_0 = {0}
 * (CLS) and S_{1+c} = the n_p tokens of channel c.  tok [B,H,N,1+C] f32: tok[b,h,q,j] = sum over k in S_j of P[b,h,q,k] (rows sum to 1);
 * ch [B,H,1+C,1+C] f32: ch[b,h,i,j] = mean over q in S_i of tok[b,h,q,j] (row-stochastic; row 0 = tok's CLS row bit for bit).  Either output may be
 * NULL, not both (DCV_ERR_NULL).  qkv / lse (all N rows read) as dcv_attn_fwd_rows(_ps) produced them; the _ps form takes the pre-scaled q.  P is
 * formed as dcv_attn_probs_rows forms it and summed in fp32; no [., N, N] array is written.  No atomics: bitwise reproducible, row q of tok does
 * not depend on the other rows, and the outputs do not depend on which of them are requested.  Two launches when ch is wanted (the query-side mean
 * reads tok).  ws: used only for ch without tok — at least dcv_attn_channel_mass_ws_floats(B, N, H, C) = B H N (1 + C) floats (else
 * DCV_ERR_NULL / DCV_ERR_SHAPE), contents irrelevant before and after; tok, ch, ws, lse 4-byte aligned. */
long dcv_attn_channel_mass_ws_floats(int B, int N, int H, int C);
int dcv_attn_channel_mass(const void* qkv, const float* lse, float* tok, float* ch, int B, int N, int H, int head_dim, float scale, int C, int n_p,
                          float* ws, long ws_floats, void* stream);
int dcv_attn_channel_mass_ps(const void* qkv, const float* lse, float* tok, float* ch, int B, int N, int H, int head_dim, int C, int n_p, float* ws,
                             long ws_floats, void* stream);
/* One step of attention rollout over one block, heads averaged (ChannelVisionTransformer.get_attention_rollout; Abnar & Zuidema's rollout is the
 * row vector pushed through the blocks from the last one down): w, out [B,N] f32, w >= 0,
 *     out[b,k] = alpha w[b,k] + (1 - alpha) / H * sum over h and q of w[b,q] P[b,h,q,k],    P as dcv_attn_probs_rows forms it
 * i.e. out = w^T (alpha I + (1 - alpha) mean_h P); sum_k out = sum_k w.  qkv / lse (all N rows read) as dcv_attn_fwd_rows(_ps) produced them; the
 * _ps form takes the pre-scaled q.  Summed in fp32; no [., N, N] array is written and there is no workspace.  No atomics: the order of every add is
 * fixed by (N, H) — bitwise reproducible, and out[b,k] does not depend on the other keys.  Every out[b,k], k < N, is written once and nothing else.
 * out must not overlap w (every workgroup reads all of w[b,:]): DCV_ERR_UNSUPPORTED, as is alpha outside [0, 1) or NaN.  lse, w, out 4-byte
 * aligned.  A query with w = 0 contributes exactly nothing. */
int dcv_attn_rollout_step(const void* qkv, const float* lse, const float* w, float* out, int B, int N, int H, int head_dim, float scale, float alpha,
                          void* stream);
int dcv_attn_rollout_step_ps(const void* qkv, const float* lse, const float* w, float* out, int B, int N, int H, int head_dim, float alpha,
                             void* stream);
/* One step of gradient-weighted attention relevance over one block, heads averaged (ChannelVisionTransformer.get_attention_relevance; Chefer, Gur &
 * Wolf 2021: R <- R + mean_h relu(grad A . A) R, of which only the CLS row is carried, from the last block down): w, out [B,N] f32, w >= 0,
 *     out[b,k] = w[b,k] + 1 / H * sum over h and q < Nq of w[b,q] P[b,h,q,k] max(G[b,h,q,k], 0),    P as dcv_attn_probs_rows forms it,
 *     G[b,h,q,k] = sum_d dO[b,q,h,d] V[b,k,h,d]   (bf16 operands, fp32 accumulation: the dP of the attention backward)
 * dO [B,N,H*64] bf16 is the gradient with respect to the attention output, 16-byte aligned.  Only the query rows [0, Nq), 1 <= Nq <= N, are read —
 * from qkv (q part), lse, w and dO; keys and values come from all N rows: nothing a row at or past Nq holds reaches a result (Nq = 1: the CLS-only
 * last block, whose dO holds its CLS rows alone).  A query with w = 0 contributes exactly nothing, whatever its dO row holds (NaN and Inf
 * included).  Summed in fp32; no [., N, N] array is written and there is no workspace.  No atomics: the order of every add is fixed by (N, Nq, H) —
 * bitwise reproducible, and out[b,k] does not depend on the other keys.  Every out[b,k], k < N, is written once and nothing else.  out must not
 * overlap w: DCV_ERR_UNSUPPORTED.  lse, w, out 4-byte aligned.  The _ps form takes the pre-scaled q of dcv_attn_fwd_rows_ps. */
int dcv_attn_relevance_step(const void* qkv, const float* lse, const void* dO, const float* w, float* out, int B, int N, int Nq, int H, int head_dim,
                            float scale, void* stream);
int dcv_attn_relevance_step_ps(const void* qkv, const float* lse, const void* dO, const float* w, float* out, int B, int N, int Nq, int H,
                               int head_dim, void* stream);

/* x [B,Ct,H,W] f32 (x_is_u8 == 0: normalised images, the reference's batch format) or u8 (raw pixels), ch_idx int32[C]
 * (device) -> bf16 [B*C*(H/P)*(W/P), P*P] patch rows (dichavit.py:134/210,377).  scale/shift f32[C] (nullable, indexed by
 * gathered position): x*scale[c] + shift[c], i.e. the (x/255 - mean_c)/std_c of the CPU pipeline
 * (jump_cp_transforms.py:119-121) fused into the tokeniser. */
int dcv_im2col_bf16(const void* x, int x_is_u8, const int* ch_idx, const float* scale, const float* shift, void* out, int B, int Ct,
                    int C, int H, int W, int P, void* stream);
/* one pass over d(tokens) f32 [B,1+C*n,D]: dY_bf16 [B*C*n,D] = dx0[:,1:] (+ dYloss) ; dE [C,D], dpos [1+n,D], dcls [D] += */
int dcv_patch_bwd(const float* dx0, const float* dYloss, void* dY_bf16, float* dE, float* dpos, float* dcls, int B, int C, int n,
                  int D, void* stream);
/* Input-image gradient of the tokeniser: the adjoint of dcv_im2col_bf16 composed with the patch projection (autograd of the Conv3d and the
 * channel gather, models/dichavit.py:134/210,377):  dx[b, ch_idx[c], i*P+u, j*P+v] = scale[c] * sum_d dY[(b*C + c)*n + i*(W/P) + j, d] * W[d, u*P+v].
 * dY bf16 [B*C*n, D] (n = (H/P)(W/P); dcv_patch_bwd's dY_bf16), W bf16 [D, P*P] (the straight operand copy of proj.weight the forward used),
 * ch_idx int32 [C] distinct positions of [0, Ct), scale f32 [C] nullable and indexed like im2col's (shift has no gradient), dx f32 [B, Ct, H, W].
 * Writes every element of dx exactly once: channels not in ch_idx and the pixels outside the (H/P)P x (W/P)P window get 0.  No atomics:
 * bitwise reproducible.  Shapes as dcv_im2col_bf16 (and C <= Ct); P in {8, 16} and D in {192, 384, 768}, else DCV_ERR_UNSUPPORTED; dY and dx
 * 16-byte aligned. */
int dcv_patch_dgrad(const void* dY, const void* W, const int* ch_idx, const float* scale, float* dx, int B, int Ct, int C, int H, int W_img,
                    int P, int D, void* stream);
/* dropout_tokens_hcs (dichavit.py:568-627): scatter == 0: out[b,k,:] = x[b,idx[k],:] (x [B,N,D] -> out [B,Nk,D]);
 * scatter != 0: out[b,idx[k],:] = x[b,k,:] (x [B,Nk,D] -> out [B,N,D], caller zero-fills out first).  f32, D % 4 == 0. */
int dcv_gather_tokens(const float* x, const int* idx, float* out, int B, int N, int Nk, int D, int scatter, void* stream);
int dcv_fill_cls(float* x, const float* cls, const float* pos0, int B, long batch_stride, int D, void* stream);

/* Train-time augmentation of the CHAMMI recipe on the device (csrc/augment.hip; the reference runs it per image on the host,
 * datasets/dataset_utils.py:234-243: TPSTransform, RandomResizedCrop(antialias=True), RandomHorizontalFlip).  Two launches, no atomics,
 * bitwise reproducible.
 * Thin-plate-spline warp of square images (datasets/tps_transform.py:22-134, its semantics kept: the coarse grid of int((W - 1) / 10)
 * points per axis evaluated in fp64, the upsampling rule pos = ((W - 1) / 10 - 1) i / (W - 1) — a zero-displacement warp zooms slightly and
 * clamps at the far edge —, then a bilinear sample with scipy's mode="reflect").  x [B, C, W, W] u8 (x_is_u8) or f32; P f64 [B, K, 2] the
 * control points (the displaced points followed by the four corners), coef f64 [B, 2, K + 3] per output axis the K kernel weights then
 * (a1, ax, ay); apply int32 [B]; out f32 [B, C, W, W] in x's units.  Only samples with apply[b] != 0 are written: the others cost no work
 * and their part of out keeps its contents.  21 <= W <= 1024, K <= 32, B <= 65535, C W W < 2^31, else DCV_ERR_UNSUPPORTED; P, coef 8-byte,
 * the rest 4-byte aligned.  Whatever P and coef hold, every read stays inside the sample. */
int dcv_tps_warp(const void* x, int x_is_u8, const double* P, const double* coef, const int* apply, float* out, int B, int C, int W, int K,
                 void* stream);
/* out f32 [B, C, S, S] = the box (i, j, h, w) = box[b] (int32 [B, 4]) of sample b resized with torch's interpolate(mode="bilinear",
 * align_corners=False, antialias=True) rule (fp32 centres and normalised triangle weights over max(n_in / S, 1) pixels per axis), the output
 * column mirrored where flip[b] != 0.  Sample b is read from warped (f32 [B, C, H, W]) where use_warped[b] != 0, else from x (u8 or f32,
 * [B, C, H, W]); warped NULL: all from x, use_warped is not read.  A box is cut to the image before use and at most 17 taps per axis are taken (n_in / S <= 8: the caller checks its boxes),
 * so nothing outside the sample is read whatever the table holds.  B, C <= 65535 and H, W, S <= 32768, else DCV_ERR_UNSUPPORTED. */
int dcv_crop_resize_flip(const void* x, int x_is_u8, const float* warped, const int* use_warped, const int* box, const int* flip, float* out,
                         int B, int C, int H, int W, int S, void* stream);

/* ortho_proj_loss_fn_v2 statistics (loss_fn.py:24-48): stats[b] = (pos_sum, neg_sum) of image b.
 * S [B,C,D], selfsq [B,C], tot [B,D], inv_norm [B,C*n] are outputs kept for the backward.
 * pos_sum is exactly 0 when n == 1 and neg_sum exactly 0 when C == 1: no such pair exists, and the caller divides by a count of 1e-6. */
int dcv_ortho_fwd(const float* Y, float* S, float* selfsq, float* tot, float* inv_norm, float* stats, int B, int C, int n, int D,
                  void* stream);
/* dY [B,C*n,D] f32 = d loss / dY given coef[b] = (dL/dpos_sum_b, dL/dneg_sum_b). */
int dcv_ortho_bwd(const float* Y, const float* S, const float* tot, const float* inv_norm, const float* coef, float* dY, int B,
                  int C, int n, int D, void* stream);

/* The channel-embedding proxy regulariser in ONE launch, value and both gradients (round 3): emb [C, D] and proxies [C, D] fp32 contiguous;
 * loss[0] = cross_entropy(-cdist(scale * normalize(emb), scale * normalize(proxies))^2, eye(C)) (mean over rows), d_emb / d_proxies [C, D] =
 * its gradients (for an upstream gradient of 1).  Replaces proxy_loss(channel_emb_proxies[cur_channels], channel_embed, eye, scale)
 * (models/dichavit.py:399-402, models/loss_fn.py:7-21) and its autograd backward: ~40 launches on [C, D] tensors.  dcv_proxy_loss_supported:
 * C <= 32, D <= 1024, C * D <= 16384 (two normalised copies in LDS); DCV_ERR_UNSUPPORTED otherwise (the caller keeps the op-by-op form). */
int dcv_proxy_loss_supported(int C, int D);
int dcv_proxy_loss(const float* emb, const float* proxies, int C, int D, float scale, float* loss, float* d_emb, float* d_proxies, void* stream);

/* DINO's multi-crop self-distillation loss (facebookresearch DINO, DINOLoss), value and gradient, fp32 in and out.  S: student logits [V, B, K],
 * view-major, views 0 and 1 the global crops, rows lds floats apart; T: teacher logits [2, B, K] of the global crops, rows ldt apart; center [K].
 * With q_i = softmax((T_i - center) / teacher_temp), p_v = softmax(S_v / student_temp), n = 2V - 2, m_v = 1 for v < 2 else 2, Q_v = sum_{i != v} q_i:
 *   loss[0] = 1 / (n B) sum_v sum_b [ m_v lse(S_v[b] / student_temp) - <Q_v[b], S_v[b]> / student_temp ]        (dcv_dino_loss_fwd)
 *   dS_v[b,k] = g[0] (m_v p_v[b,k] - Q_v[b,k]) / (n B student_temp), rows ldd apart, written once             (dcv_dino_loss_bwd)
 * g is read on the device (the incoming gradient: no host synchronisation).  The forward is three launches: one pass over S, T and center that
 * leaves per-(batch row, column tile) partial maxima, sums of exponentials and dots in ws, a finish that merges them in tile order and forms
 * tsum, and a one-block sum of the B row terms (in double).  Besides loss it writes, each unless NULL: s_stats [V B, 2], per row (max, sum of exponentials relative to it) of S /
 * student_temp, and t_stats [2 B, 3], per row (max, the max's low part, sum) of (T - center) / teacher_temp with T - center carried as fl(T - center) plus its
 * exact rounding error — what the backward reads; the log-sum-exp is
 * max / temp + ln(sum) — and tsum [K] = sum_{i,b} T_i[b,k], the centre statistics (formed in the finish launch from a second read of T).  The
 * backward is one launch: S, T, center read once more, dS written once; no probability tensor ever reaches memory.  ALWAYS deterministic: no
 * atomics, and every summation order is a function of (V, B, K) alone — not of the strides, the alignment or the grid.  16-byte loads and stores when
 * every matrix pointer is 16-byte aligned and K and every stride are multiples of 4, 4-byte ones on the same columns otherwise; columns >= K of a
 * row are never read (padding may hold anything).  ws: at least dcv_dino_loss_ws_floats(V, B, K) floats, contents irrelevant before and after.
 * Checked before any HIP call: a required pointer NULL -> DCV_ERR_NULL; V < 2, B < 1, K < 1, a stride below K, a temperature that is not
 * positive, ws_floats too small -> DCV_ERR_SHAPE; a row of 2 GB or more (with its last tile) -> DCV_ERR_UNSUPPORTED; a pointer off 4 bytes
 * (ws: 16) -> DCV_ERR_ALIGN. */
long dcv_dino_loss_ws_floats(int V, int B, int K);
int dcv_dino_loss_fwd(const float* S, long lds, const float* T, long ldt, const float* center, int V, int B, int K, float student_temp,
                      float teacher_temp, float* loss, float* s_stats, float* t_stats, float* tsum, float* ws, long ws_floats, void* stream);
int dcv_dino_loss_bwd(const float* S, long lds, const float* T, long ldt, const float* center, const float* s_stats, const float* t_stats,
                      const float* g, int V, int B, int K, float student_temp, float teacher_temp, float* dS, long ldd, void* stream);
/* their launch plan — host logic, no GPU call.  aligned: does the call meet the 16-byte condition above.  A row's columns fall into col_tiles
 * tiles of tile_cols = 1024; one wave owns one item = (batch row b, tile), item = b * col_tiles + tile, for every view, and lane l holds the 16
 * columns tile * tile_cols + (64 u + l) * 4 + e, u, e < 4 (slot 4 u + e), loaded vec = 4 or 1 floats at a time.  A workgroup is waves_per_wg = 4
 * waves; wave w of workgroup x takes in pass r the item (x + r * grid) * waves_per_wg + w (none past `items`); grid = min(ceil(items / 4), 2048),
 * passes = 1 below the cap.  ws holds items * (6 + 4 V) + 2 B floats. */
int dcv_dino_loss_plan(int V, int B, int K, int aligned, int* vec, int* tile_cols, int* col_tiles, long* items, int* waves_per_wg, int* grid,
                       int* passes);

/* iBOT's masked patch-token distillation loss (Zhou et al. 2022; the patch term of DINOv2), value and gradient, fp32 in and out (csrc/
 * ibot_loss.hip).  S: student logits [R, K], rows lds floats apart; T: teacher logits [R, K], rows ldt apart, row r of both the same masked token;
 * center [K]; weights [R].  With q_r = softmax((T_r - center) / teacher_temp) and p_r = softmax(S_r / student_temp):
 *   loss[0] = sum_r weights[r] (lse(S_r / student_temp) - <q_r, S_r> / student_temp)                        (dcv_ibot_loss_fwd)
 *   dS[r,k] = g[0] weights[r] (p_r[k] - q_r[k]) / student_temp, rows ldd apart, written once              (dcv_ibot_loss_bwd)
 *   tsum[k] = sum_r T[r,k], unweighted: the centre's statistics                                           (dcv_ibot_loss_fwd, unless NULL)
 * g is read on the device.  The forward is three launches: one pass over S, T and center that leaves per-(row, column tile) partial maxima,
 * sums of exponentials and dots and, per chunk of 32 rows, the chunk's column sums of T (in double) in ws; a finish that merges a row's records in
 * tile order and, beside that, adds the chunks' column sums in a fixed order (tsum's second level: T is read once); and a one-block sum of the R
 * weighted row terms (in double).  s_stats [R, 3]: per row (max, sum of exponentials relative to it as a high and a low float: the sums are formed in double) of S /
 * student_temp; t_stats [R, 4]: per row (max, the max's low part, sum high, sum low) of (T - center) / teacher_temp with T - center carried as fl(T - center) plus its exact rounding error; each
 * written unless NULL, and what the backward reads.  The backward is one launch: S, T, center read once more, dS written once; no probability
 * tensor ever reaches memory.  ALWAYS deterministic: no atomics, and every summation order is a function of (R, K) alone — not of the data, the
 * weights, the strides, the alignment or the grid.  A row of weight 0 adds exactly 0 to the loss and its dS row is exactly 0.  16-byte loads and
 * stores when every matrix pointer is 16-byte aligned and K and every stride are multiples of 4, 4-byte ones on the same columns otherwise;
 * columns >= K of a row are never read (padding may hold anything).  ws: at least dcv_ibot_loss_ws_floats(R, K) floats, contents irrelevant before
 * and after.  Checked before any HIP call: a required pointer NULL -> DCV_ERR_NULL; R < 1, K < 1, a stride below K, a temperature that is not
 * positive, ws_floats too small -> DCV_ERR_SHAPE; a row of 2 GB or more (with its last tile) -> DCV_ERR_UNSUPPORTED; a pointer off 4 bytes
 * (ws: 16) -> DCV_ERR_ALIGN. */
long dcv_ibot_loss_ws_floats(int R, int K);
int dcv_ibot_loss_fwd(const float* S, long lds, const float* T, long ldt, const float* center, const float* weights, int R, int K,
                      float student_temp, float teacher_temp, float* loss, float* s_stats, float* t_stats, float* tsum, float* ws, long ws_floats,
                      void* stream);
int dcv_ibot_loss_bwd(const float* S, long lds, const float* T, long ldt, const float* center, const float* weights, const float* s_stats,
                      const float* t_stats, const float* g, int R, int K, float student_temp, float teacher_temp, float* dS, long ldd, void* stream);
/* their launch plan — host logic, no GPU call.  A row's columns fall into col_tiles tiles of tile_cols = 1024 and the rows into chunks =
 * ceil(R / chunk_rows) chunks of chunk_rows = 32 consecutive rows; one wave owns one item = (chunk, tile), item = chunk * col_tiles + tile, and
 * walks the chunk's rows in row order; lane l holds the 16 columns tile * tile_cols + (64 u + l) * 4 + e, u, e < 4, loaded vec = 4 or 1 floats at
 * a time.  A workgroup is waves_per_wg = 4 waves; wave w of workgroup x takes in pass r the item (x + r * grid) * waves_per_wg + w (none past
 * `items`); grid = min(ceil(items / 4), 2048), passes = 1 below the cap.  ws holds 2 (6 R col_tiles + R + chunks K) floats (doubles: the records, the row terms, tsum's first level). */
int dcv_ibot_loss_plan(int R, int K, int aligned, int* vec, int* tile_cols, int* col_tiles, int* chunk_rows, int* chunks, long* items,
                       int* waves_per_wg, int* grid, int* passes);

/* The learned mask token of masked-patch distillation at the tokeniser's seam (csrc/mask_tokens.hip).  mask: uint8 [B, C n], nonzero = masked.
 * dcv_mask_tokens_fwd, after the DCV_EPI_PATCH GEMM: every masked token row (b, t = c n + i) gets xs[b, 1 + t, :] = mask_token + (E[c] +
 * pos[1 + i]) — the bits the epilogue writes for a row whose acc + bias equals mask_token; nothing else is written (xs f32 [B, 1 + C n, D], E
 * [C, D], pos [1 + n, D], mask_token [D], 16-byte aligned).
 * dcv_mask_tokens_bwd, after dcv_patch_bwd: dmask_token[D] += the sum of dx0[b, 1 + t, :] over the masked rows, and the masked rows of dY_bf16
 * [B C n, D] become bf16(dYloss row), or 0 when dYloss is NULL.  No atomics: parts of 256 consecutive rows of the flat (b, t) range, 256 / (D / 4)
 * sub-lanes per part, partials through ws (>= dcv_mask_tokens_bwd_ws_floats floats), added in index order.  D % 4 == 0, D <= 1024. */
int dcv_mask_tokens_fwd(float* xs, const unsigned char* mask, const float* mask_token, const float* E, const float* pos, int B, int C, int n, int D,
                        void* stream);
long dcv_mask_tokens_bwd_ws_floats(int B, int C, int n, int D);
int dcv_mask_tokens_bwd(const float* dx0, const unsigned char* mask, const float* dYloss, void* dY_bf16, float* dmask_token, int B, int C, int n,
                        int D, float* ws, long ws_floats, void* stream);

/* fused AdamW over a flat fp32 range; g is multiplied by grad_scale first (1/world for data parallel). */
int dcv_adamw(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
              float weight_decay, int step, float grad_scale, void* stream);
/* same update with the scalars read from device memory: hyper_dev[8] = {lr, beta1, beta2, eps, weight_decay,
 * 1/(1-beta1^t), 1/sqrt(1-beta2^t), grad_scale}.  Lets a captured HIP graph of the step be replayed while the
 * step count and the schedulers' lr / weight decay advance (dcv_adamw_set_hyper rewrites the 32 bytes between replays). */
int dcv_adamw_dyn(float* p, const float* g, float* m, float* v, long n, const float* hyper_dev, void* stream);
/* writes hyper_dev[8] for step `step` (bias corrections computed in double on the host, passed BY VALUE to a one-thread
 * kernel): stream-ordered, no host staging buffer, so a host that runs many steps ahead of the device cannot overwrite the
 * scalars of a step that has not executed yet. */
int dcv_adamw_set_hyper(float* hyper_dev, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                        float grad_scale, void* stream);
/* AdamW with PARAMETER GROUPS over the flat arena (csrc/optim_groups.hip): one launch whatever the number of groups, frozen
 * parameters included — the DINO decay / no-decay split, layer-wise learning-rate decay, fine-tuning with a frozen prefix. */
#define DCV_ADAMW_MAX_GROUPS 32    /* 32 x 8 floats = 1 KB, passed by value; LLRD at depth 12 with a decay / no-decay split needs 2 x 14 = 28 */
#define DCV_ADAMW_MAX_SEGS   1024  /* DiChaViT has 149 encoder tensors; 8 KB of LDS for the table */
/* hyper_dev[n_groups][8], one row per group in dcv_adamw_set_hyper's layout {lr, b1, b2, eps, wd, 1/bc1, 1/sqrt(bc2), grad_scale};
 * rows_host[n_groups][5] = {lr, b1, b2, eps, wd}, steps_host[n_groups] >= 1 (bias corrections in double on the host, as
 * dcv_adamw_set_hyper).  The rows travel BY VALUE as the argument of one small kernel: stream-ordered, no staging buffer. */
int dcv_adamw_set_hyper_groups(float* hyper_dev, const float* rows_host, const int* steps_host, int n_groups, float grad_scale, void* stream);
/* One launch over p, g, m, v [n] (n % 4 == 0, 16-byte aligned).  seg_end4 / seg_group: device int32 [n_seg], sorted runs that cover
 * [0, n / 4) in float4 units: run s is [seg_end4[s-1], seg_end4[s]) and takes hyper row seg_group[s]; seg_group[s] == -1 is a
 * SKIPPED run: p, m, v are not written and g is not read there (a row index outside [0, n_groups) skips too; float4 past the last
 * end belong to the last run; nothing outside [0, n) is touched whatever the table holds).  Element update = dcv_adamw_dyn's with
 * that row, bit for bit. */
int dcv_adamw_groups(float* p, const float* g, float* m, float* v, long n, const int* seg_end4, const int* seg_group, int n_seg,
                     const float* hyper_dev, int n_groups, void* stream);
/* Weight averaging over the flat parameter arena (csrc/avg.hip): avg[i] <- lerp(avg[i], p[i], w) for i < n in ONE launch — SWA / SWAD and
 * EMA of the weights (torch.optim.swa_utils.AveragedModel.update_parameters; the reference trainer's train.swa / train.swad, trainer.py:810-812,
 * 957-959).  The count of updates so far is read from the device word *n_averaged_dev when that is not NULL (n_averaged is then ignored; the
 * kernel never writes the word: the caller bumps it, stream-ordered, so a captured step replays with the live count), else it is n_averaged.
 *   count == 0: w = 1 in both modes (the first update copies);  DCV_AVG_SWA: w = 1.0f / (float)(count + 1), correctly rounded;
 *   DCV_AVG_EMA: w = ema_weight (pass (float)(1 - decay)).
 * Element: w == 1: avg = p bit for bit; w < 0.5: fmaf(w, p - avg, avg); else fmaf(-(p - avg), 1 - w, p) (ATen's two-sided lerp).  No atomics:
 * bitwise reproducible; p is read only; avg and p must not overlap.  grid_cap > 0 caps the number of workgroups (0: the product's cap).
 * Checked in this order, before any HIP call: avg / p NULL -> DCV_ERR_NULL; n < 0 -> DCV_ERR_SHAPE; avg / p not 16-byte (n_averaged_dev not
 * 8-byte) aligned -> DCV_ERR_ALIGN; an unknown mode -> DCV_ERR_UNSUPPORTED; ema_weight outside [0, 1] or NaN, n_averaged < 0 (when it is used),
 * grid_cap < 0 -> DCV_ERR_SHAPE.  n == 0 succeeds and launches nothing. */
#define DCV_AVG_SWA 0
#define DCV_AVG_EMA 1
int dcv_avg_update(float* avg, const float* p, long n, int mode, float ema_weight, long n_averaged, const long long* n_averaged_dev,
                   int grid_cap, void* stream);
/* Gradient clipping (trainer.py:1003-1004 -> torch.nn.utils.clip_grad_norm_, L2): dcv_sumsq_acc adds sum(x^2) of a flat fp32
 * range to the device scalar *acc (zero it first; call once per gradient buffer); dcv_clip_scale multiplies a range by
 * min(1, max_norm / (sqrt(*sumsq_dev) + 1e-6)).  Everything stays on the device: no host sync, graph-capturable. */
int dcv_sumsq_acc(const float* x, long n, float* acc, void* stream);
int dcv_clip_scale(float* x, long n, const float* sumsq_dev, float max_norm, void* stream);
/* bf16 operand copies of the parameter arena */
int dcv_cast_bf16(const float* src, void* dst, long n, void* stream);
/* desc_dev: device int64 [n_desc][4] = {src offset, dst offset, R, C}; dst[C][R] = bf16(src[R][C]) */
int dcv_cast_transpose_bf16(const float* src_base, void* dst_base, const long long* desc_dev, int n_desc, int max_tiles, void* stream);
/* Stochastically rounded variants for the TRAINING operand copies: bf16 = (fp32 bits + r) >> 16 with r = the low 16
 * bits of lowbias32(element_offset_from_src_base ^ seed_dev[0]*0x9E3779B9).  Both use the offset from the arena base, so a
 * weight and its transposed copy round identically; seed_dev is a device word the host bumps once per step (graph-replay
 * safe).  The reference trains in fp32 (trainer.py:963-1006, no autocast on CPU): round-to-nearest copies lag the fp32
 * master coherently under AdamW's +-lr steps, unbiased rounding removes that lag. */
int dcv_cast_bf16_sr(const float* src, void* dst, long n, const unsigned* seed_dev, void* stream);
int dcv_cast_transpose_bf16_sr(const float* src_base, void* dst_base, const long long* desc_dev, int n_desc, int max_tiles,
                               const unsigned* seed_dev, void* stream);

/* Scaled re-cast of parts of an operand copy.  desc_dev: device int64 [n_desc][5] = {src offset (floats from src_base), dst offset, count,
 * scaled_count, kind}.  kind 0: dst_bf16[dst + i] = bf16(f_i * src[i]), kind 1: dst_f32[dst + i] = f_i * src[i], with f_i = scale for i <
 * scaled_count and 1 after.  seed_dev NULL: round to nearest; else the stochastic rounding of dcv_cast_bf16_sr with the same per-element bits
 * (offset from src_base), so the rewritten range is what that cast would have produced from scale * src.  blocks_per_desc: grid.x. */
int dcv_cast_scaled_ranges(const float* src_base, void* dst_bf16, float* dst_f32, const long long* desc_dev, int n_desc, int blocks_per_desc,
                           float scale, const unsigned* seed_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
