/* prx.h -- C ABI of libprx_hip.so, the MI355X (gfx950) implementation of
 * pixray's per-iteration hot path:
 *
 *   drawer.synth (VQGAN decode) -> MakeCutouts -> CLIP ViT encode_image ->
 *   Prompt spherical-distance loss -> backward to z -> Adam + clip_z
 *
 * The reference (pixray/pixray) has NO FFI: its boundary for this path is the
 * Python plugin surface (DrawingInterface / LossInterface / FilterInterface /
 * Prompt / perceptor.encode_image / MakeCutouts) and every operator below is
 * what PyTorch/cuDNN executes underneath it.  Each entry point cites the
 * reference call site (file:line in /root/reference) whose arithmetic it
 * replaces.  See INTEGRATION.md for the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - plain C: pointers, ints, floats; no torch/HIP C++ types in signatures
 *     (`prx_stream_t` is a hipStream_t passed as an opaque pointer).
 *   - every function returns 0 on success, <0 on error; prx_last_error() gives
 *     a thread-local message.  Nothing throws across the ABI.
 *   - all pointers named d_* / documented "device" are HBM addresses owned by
 *     the caller; the library owns only handles made by prx_*_create.
 *   - all work is enqueued asynchronously on the given stream; no hidden
 *     device synchronisation; handles are re-entrant per handle (one forward
 *     may be in flight per handle until its backward has been enqueued).
 *   - tensors at this boundary are fp32, NCHW / row-major, exactly as the
 *     reference's PyTorch tensors are laid out.  Internal layouts (NHWC bf16
 *     operand packs, fp32 residual streams) are private.
 */
#ifndef PRX_H_
#define PRX_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRX_ABI_VERSION 3   /* 3: prx_gemm_args.row16; prx_prompt_loss_fwd_bwd(loss, ticket); 36-word cutout descriptors */

typedef void* prx_stream_t; /* hipStream_t */

const char* prx_last_error(void);
int prx_abi_version(void);
int prx_device_info(int* cu_count, char* arch_name, int arch_name_len);

/* ------------------------------------------------------------------------ */
/* Kernel-level entry points (used by tests/ to check every kernel alone)    */
/* ------------------------------------------------------------------------ */

/* activation / A-operand modes of the GEMM engine */
#define PRX_ACT_NONE 0
#define PRX_ACT_QUICKGELU 1      /* CLIP QuickGELU, x*sigmoid(1.702x)  [UPSTREAM clip/model.py] */
#define PRX_ACT_MUL_DQUICKGELU 2 /* multiply by QuickGELU'(aux) (backward) */
#define PRX_ACT_RELU 3           /* max(v, 0) after bias / residual (CLIP ModifiedResNet [UPSTREAM clip/model.py]) */
#define PRX_ACT_MUL_RELUMASK 4   /* multiply by (aux > 0): ReLU backward, aux = the forward output */
#define PRX_ACT_RELUMASK_POST 5  /* the same mask applied AFTER the residual add: (acc + resid) * (aux > 0) -- the gradient
                                    arriving at a Bottleneck's output ReLU, formed in the epilogue of the GEMM that sums it */
#define PRX_ACT_GELU 6           /* the exact GELU, 0.5 t (1 + erf(t / sqrt 2)) (timm VisionTransformer MLP: the SLIP towers); writes the
                                    pre-activation to out_bf16_pre as PRX_ACT_QUICKGELU does.  This code and the next: 16-bit operand
                                    modes with the vector epilogue (N % 4 == 0, aligned operands) only; the exact-f32 kernels refuse them
                                    (the ViT runner's parity mode applies the activation in a pass of its own) */
#define PRX_ACT_MUL_DGELU 7      /* multiply by GELU'(aux) = Phi(aux) + aux phi(aux) (backward) */
#define PRX_A_ROWMAJOR 0
#define PRX_A_CONV3X3 1          /* implicit im2col of an NHWC tensor, 3x3 pad 1 */

/* Operand precision of a runner handle (the `precision` field of the *_config structs below):
 *   PRX_PREC_BF16  GEMM operands (inter-kernel activations, weight packs) bf16, fp32 accumulate on
 *                  v_mfma_f32_32x32x16_bf16; residual streams, norms, softmax statistics, loss, optimiser fp32.
 *   PRX_PREC_F32   every operand fp32 end to end on v_mfma_f32_32x32x2_f32 (exact f32 = what the reference's CPU
 *                  path computes, pixray.py:275-280, vqgan.py:60-79, slip.py:21-66): the parity mode, 1/16 of the rate.
 *   PRX_PREC_F16   the same data flow as PRX_PREC_BF16 with IEEE half operands on v_mfma_f32_32x32x16_f16 (same MFMA rate):
 *                  the arithmetic the reference's CLIP towers run in on a GPU -- `clip.load` keeps fp16 weights and
 *                  activations with fp32 LayerNorm (slip.py:175) -- with 11 significand bits instead
 *                  of bf16's 8.  Conversions saturate at +-65504, and every runner backward runs under a power-of-two
 *                  gradient scale S chosen ON THE DEVICE from the gradient entering it (S * max|g| in [8, 16); no host
 *                  synchronisation; exact, because each backward op is linear in the incoming gradient and ClampWithGrad /
 *                  ReLU masks only read signs) that is removed before anything leaves the handle.  The VGG16 extractor of the StyleLoss plugin has the same three modes; the VQGAN encoder and the CLIP text tower (forward only) stay bf16 / fp32. */
#define PRX_PREC_BF16 0
#define PRX_PREC_F32 1
#define PRX_PREC_F16 2

/* Engine state of ONE handle: tile / split-K overrides and the optional per-launch timing log.  Each runner handle owns
 * one (prx_*_gemm_ctx below); the library has no process-global mutable state. */
typedef struct prx_gemm_ctx prx_gemm_ctx;
prx_gemm_ctx* prx_gemm_ctx_create(void);
void prx_gemm_ctx_destroy(prx_gemm_ctx* c);

/* C[M,N] = epilogue(alpha * A[M,K] * Bt[N,K]^T); MFMA, fp32 accumulate.
 * Replaces torch.nn.functional.linear / conv2d under clip.model.* and
 * taming Decoder (call sites slip.py:65, vqgan.py:195). */
typedef struct prx_gemm_args {
    const void* A;      /* device; bf16 (a_is_f32=0) or fp32 converted on load */
    int a_is_f32, a_mode, lda;
    const void* B;      /* device bf16 [N, K], K contiguous */
    int ldb;
    int M, N, K;
    int H, W, Cin, up;  /* conv geometry (a_mode == PRX_A_CONV3X3): output H x W; up = 0 source H x W, 1 source H/2 x W/2 read through
                         * a nearest-2x upsample, 2 source 2H x 2W read with stride 2 and taming's (0,1,0,1) Downsample padding */
    float alpha;
    const float* bias_n;
    const float* bias_m;
    const void* aux;    /* bf16 [M, ldaux] */
    int ldaux;
    const float* resid; /* fp32 [M, ldr] */
    int ldr;
    int act;
    float* out_f32; int ldc_f32;
    void* out_bf16; void* out_bf16_pre; int ldc_bf16;
    int f32;            /* operand precision, PRX_PREC_*: _F32 = A, B, aux, out_bf16, out_bf16_pre are all fp32 and the product is
                         * exact f32; _F16 = the 16-bit operands are IEEE half; _BF16 (0) = bf16 */
    int row16;          /* 16-bit operand modes: bit 0 = `resid` addresses a 16-bit stream in the operand format (the runners' lean
                         * layout: residual / feature-map streams kept in 16 bits), bit 1 = so does prx_k_gemm_gn's `gnb_x` */
    prx_gemm_ctx* ctx;  /* tuning / timing context or NULL (built-in heuristics) */
} prx_gemm_args;
int prx_k_gemm(const prx_gemm_args* g, void* ws, size_t ws_bytes, prx_stream_t stream);
/* The same product with the decoder's fused GroupNorm sums in the epilogue (taming `Normalize`, 32 groups of gn_gs = N / 32
 * consecutive channels; call site vqgan.py:195): gn_stats (double[64], pre-zeroed, accumulated with atomics) receives per group
 * {sum, sum of squares} of the fp32 output -- or, when gnb_x is given (the forward INPUT [M, N] of the GroupNorm whose output
 * gradient this product is, with its forward sums gnb_fstats and affine parameters), that GroupNorm's backward sums
 * {sum dxhat, sum dxhat * xhat}.  Needs N == 32 * gn_gs, gn_gs a multiple of 4, 16-bit operands. */
int prx_k_gemm_gn(const prx_gemm_args* g, double* gn_stats, int gn_gs, const float* gnb_x, const double* gnb_fstats,
                  const float* gnb_gamma, const float* gnb_beta, int gnb_swish, float gnb_eps, void* ws, size_t ws_bytes,
                  prx_stream_t stream);
/* Diagnostics: how many launches of this process ran a fit or 8-phase kernel whose epilogue is specialised at compile time
 * (csrc/gemmfit_kernel.h FIT_EPI_*, csrc/gemm8p.hip: the descriptor patterns of the two runners, IEEE-half operands) -- tests use it to know that the specialised kernel,
 * not the generic one, produced what they compare. */
long long prx_gemm_fit_spec_launches(void);
/* ... and how many ran a row-streaming kernel (csrc/gemmrow.hip: row-major 16-bit products with K <= 640 and N a multiple of 160, 128
 * or 80 -- only 80 beyond K = 320 --, and implicit 3x3 convolutions with (N, Cin) in {40, 80}^2 or (160, 160); from M N >= 24 Mi output
 * elements on (PRX_GEMM_ROWK_MIN, override -14) -- the ModifiedResNet runner's stage-1 / stage-2 convolutions; PRX_GEMM_ROWK=0 keeps
 * them on the tiled kernels). */
long long prx_gemm_row_launches(void);
/* n (1..4) products in one launch: g[0..n) agree in every field except A, B, out_f32 and out_bf16 (and share one ctx), and their
 * outputs do not overlap -- the decoder AttnBlock's dq / dk / dv (call site vqgan.py:195, the backward of taming's AttnBlock): one
 * shape, three operand pairs, three column slices of one buffer.  Where member 0 plans onto a single direct-to-LDS 4-wave launch
 * without split-K (row-major A) and the others plan alike, one grid runs them all, bit for bit what n prx_k_gemm calls give; every
 * other case IS n prx_k_gemm calls in order. */
int prx_k_gemm_group(const prx_gemm_args* g, int n, void* ws, size_t ws_bytes, prx_stream_t stream);
/* ... and how many prx_k_gemm_group calls (the decoder runner's included) ran as one grouped launch. */
long long prx_gemm_group_launches(void);

/* taming `Normalize` = GroupNorm(32, C, eps 1e-6) (+ swish `nonlinearity`) on an NHWC fp32
 * tensor x[NB][P][C]  [UPSTREAM taming/modules/diffusionmodules/model.py; call site vqgan.py:195].
 * stats: double[NB*64] workspace (sum, sum of squares per group).  bwd returns the activation
 * gradient only (weights are frozen, vqgan.py:125). */
int prx_k_groupnorm_fwd(const float* x, const float* gamma, const float* beta, double* stats, void* out_bf16,
                        float* out_f32, int NB, int P, int C, int swish, float eps, prx_stream_t s);
int prx_k_groupnorm_bwd(const float* g, const float* x, const float* gamma, const float* beta, const double* fstats,
                        double* bstats, const float* add, float* dx, int NB, int P, int C, int swish, float eps,
                        prx_stream_t s);
/* CLIP LayerNorm (eps 1e-5, computed in fp32) [UPSTREAM clip/model.py; call site slip.py:65] */
int prx_k_layernorm_fwd(const float* x, long long ldx, const float* gamma, const float* beta, void* out_bf16,
                        float* out_f32, float* mean, float* rstd, int rows, int C, float eps, prx_stream_t s);
int prx_k_layernorm_bwd(const float* g, long long ldg, const float* x, long long ldx, const float* gamma,
                        const float* mean, const float* rstd, const float* add, long long ldadd, float* dx,
                        long long lddx, int rows, int C, prx_stream_t s);
int prx_k_transpose_bf16(const void* in, int ldin, void* out, int ldout, int R, int C, prx_stream_t s);
/* taming AttnBlock softmax over keys (single head) */
int prx_k_softmax_rows(const float* S, int lds_, float scale, void* P, int ldp, void* PT, int ldpt, int rows, int cols,
                       prx_stream_t s);
int prx_k_softmax_rows_bwd(const void* P, int ldp, const float* dP, int lddp, float scale, void* dS, int ldds,
                           void* dST, int lddst, int rows, int cols, prx_stream_t s);
/* backward of taming Upsample's nearest-2x interpolate */
int prx_k_upsample2x_bwd(const float* hi, float* low, int NB, int Hl, int Wl, int C, prx_stream_t s);
int prx_k_nchw_to_nhwc(const float* in, float* out_f32, void* out_bf16, int NB, int C, int HW, int Cpad,
                       prx_stream_t s);
int prx_k_nhwc_to_nchw(const float* in, int ldc, float* out, int NB, int C, int HW, prx_stream_t s);
/* VqganDrawer.synth tail: clamp_with_grad(decode(z_q).add(1).div(2), 0, 1)  (vqgan.py:66-79,195) */
int prx_k_image_head_fwd(const float* x, int ldc, float* img, int NB, int C, int HW, prx_stream_t s);
int prx_k_image_head_bwd(const float* x, int ldc, const float* gimg, float* dx, void* dx_bf16, int ldo, int NB, int C,
                         int HW, prx_stream_t s);
/* nn.MultiheadAttention core of CLIP's ResidualAttentionBlock.  Every prx_k_mha_* call is a view of the one attention dispatcher
 * (csrc/attention.h: a descriptor of the problem, one function that picks the kernel family or refuses): the call's name and
 * arguments fill the descriptor, the dispatcher checks and launches.  These two: bf16, head dim 64, the recomputing form (no lse, the
 * backward reads no `out`), which has kernels for T <= 64 */
int prx_k_mha_fwd(const void* qkv, void* out, int N, int T, int C, int heads, prx_stream_t s);
int prx_k_mha_bwd(const void* qkv, const void* dout, void* dqkv, int N, int T, int C, int heads, prx_stream_t s);

/* The same kernels with EVERY argument of the internal functions exposed (test surface only; the product's Python never calls
 * these): `h16` selects the 16-bit operand format (0 bf16, 1 IEEE half with saturating conversion), `s16` the lean layout
 * (stream inputs are 16-bit tensors in that format: a flag for GroupNorm / upsample / LayerNorm forward, bits 1 = x, 2 = g,
 * 4 = add for the LayerNorm backward), `*16` outputs may be the only output (fp32 twin null), `add_every` > 0 reads `add` on
 * the rows that are multiples of it only, `zero_stats` / `stats_ready` skip the memset / the statistics pass (sums supplied by
 * the caller), `gscale` is a device scalar multiplying the outgoing gradient, `prec` a PRX_PREC_* value, `f32` the element
 * type of an untyped buffer.  tests/test_kernels_half_gpu.py holds each variant to a float64 reference. */
int prx_k_groupnorm_fwd_op(const void* x, const float* gamma, const float* beta, double* stats, void* out16, float* out_f32,
                           int NB, int P, int C, int swish, float eps, int zero_stats, int stats_ready, int h16, int s16,
                           prx_stream_t s);
int prx_k_groupnorm_bwd_op(const void* g, const void* x, const float* gamma, const float* beta, const double* fstats,
                           double* bstats, const void* add, float* dx, void* dx16, int NB, int P, int C, int swish, float eps,
                           int zero_stats, int stats_ready, int h16, int s16, prx_stream_t s);
int prx_k_layernorm_fwd_op(const void* x, long long ldx, const float* gamma, const float* beta, void* out16, float* out_f32,
                           float* mean, float* rstd, int rows, int C, float eps, int h16, int s16, prx_stream_t s);
int prx_k_layernorm_bwd_op(const void* g, long long ldg, const void* x, long long ldx, const float* gamma, const float* mean,
                           const float* rstd, const void* add, long long ldadd, float* dx, long long lddx, void* dx16,
                           long long lddxb, int rows, int C, int h16, int add_every, int s16, prx_stream_t s);
/* the dispatcher's views with the 16-bit format as an argument: _op the recomputing form (T <= 64), _gen_op the saving form (any T:
 * `out` and `lse` are kept for the backward), both at head dim 64 */
int prx_k_mha_fwd_op(const void* qkv, void* out, int N, int T, int C, int heads, int h16, prx_stream_t s);
int prx_k_mha_bwd_op(const void* qkv, const void* dout, void* dqkv, int N, int T, int C, int heads, int h16, prx_stream_t s);
int prx_k_mha_fwd_gen_op(const void* qkv, void* out, float* lse, int N, int T, int C, int heads, int h16, prx_stream_t s);
int prx_k_mha_bwd_gen_op(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int N, int T, int C,
                         int heads, int h16, prx_stream_t s);
/* prx_k_mha_{fwd,bwd}_gen_op with the operand columns per head as an argument (64 | 96, anything else is refused here): the
 * descriptor's head dim is 64 or 80.  head_cols 64: the two calls above, bit for bit.  head_cols 96: heads of dim 80 zero-padded to 96 columns (OpenCLIP ViT-H/14; the 96-wide instances of csrc/attention_kernels.h): C == heads * 96, head h at
 * columns 96h .. 96h+95 of q, k, v, out and their gradients, the caller's columns 80 .. 95 of every head zero, softmax scale
 * 1 / sqrt(80), 1 <= T <= 640; columns 80 .. 95 of `out` and `dqkv` are written as exact zeros. */
int prx_k_mha_fwd_hd_op(const void* qkv, void* out, float* lse, int N, int T, int C, int heads, int h16, int head_cols, prx_stream_t s);
int prx_k_mha_bwd_hd_op(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int N, int T, int C,
                        int heads, int h16, int head_cols, prx_stream_t s);
/* the head padding prx_vit_tower_create applies when it packs a block's weights (fp32 device tensors, width == heads * hd):
 * qkv_w [3 width, width] -> qkv_w_pad [3 heads hp, width] (every head's hd rows of q, k and v become the first hd of hp rows),
 * out_w [width, width] -> out_w_pad [width, heads hp] (the matching input columns); pad rows / columns are zero. */
/* the same two calls with the descriptor's head dim as an argument (>= 64, checked here; the dispatcher derives the columns per head
 * from it and refuses a C that is not heads times that many, so head_cols only says what C / heads has to be): head_dim 64 at
 * head_cols 64 are prx_k_mha_{fwd,bwd}_gen_op; 80 | 88 at
 * head_cols 96 and 104 at head_cols 128 (OpenCLIP ViT-H-14 | ViT-g-14 and ViT-bigG-14) run the 96- / 128-wide instances with the softmax
 * scale 1 / sqrt(head_dim).  The caller's columns head_dim .. head_cols - 1 of every head are zero, and so are those of `out` and `dqkv`.
 * Any other pair is refused by the dispatcher. */
int prx_k_mha_fwd_hdim_op(const void* qkv, void* out, float* lse, int N, int T, int C, int heads, int h16, int head_cols, int head_dim,
                          prx_stream_t s);
int prx_k_mha_bwd_hdim_op(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int N, int T, int C,
                          int heads, int h16, int head_cols, int head_dim, prx_stream_t s);
/* prx_k_layernorm_{fwd,bwd}_op in the ragged form the ViT runner uses: C a multiple of 128 (not only of 256), C <= 2048 -- the last
 * float4 vector of a row is held by half a wave.  384 ... 896 run the MAXV = 4 instances, 1152 ... 1920 the MAXV = 8 ones. */
int prx_k_layernorm_fwd_rag_op(const void* x, long long ldx, const float* gamma, const float* beta, void* out16, float* out_f32,
                               float* mean, float* rstd, int rows, int C, float eps, int h16, int s16, prx_stream_t s);
int prx_k_layernorm_bwd_rag_op(const void* g, long long ldg, const void* x, long long ldx, const float* gamma, const float* mean,
                               const float* rstd, const void* add, long long ldadd, float* dx, long long lddx, void* dx16, long long lddxb,
                               int rows, int C, int h16, int add_every, int s16, prx_stream_t s);
int prx_k_vit_pad_heads(const float* qkv_w, float* qkv_w_pad, const float* out_w, float* out_w_pad, int width, int heads, int hd, int hp,
                        prx_stream_t s);
/* the dispatcher's causal view: forward only, head dim 64, no lse (CLIP text transformer) */
int prx_k_mha_fwd_causal_op(const void* qkv, void* out, int N, int T, int C, int heads, int h16, prx_stream_t s);
int prx_k_softmax_rows_op(const float* S, int lds_, float scale, void* P, int ldp, void* PT, int ldpt, int rows, int cols,
                          int prec, prx_stream_t s);
int prx_k_softmax_rows_bwd_op(const void* P, int ldp, const float* dP, int lddp, float scale, void* dS, int ldds, void* dST,
                              int lddst, int rows, int cols, int prec, prx_stream_t s);
/* the two softmax launches with the independent transpose tout[c][r] = tin[r][c] (tR x tC, operand precision) in the same launch:
 * the bytes of prx_k_softmax_rows(_bwd)_op followed by prx_k_transpose_op (taming AttnBlock forward q|k|v -> v^T and backward
 * d(out) -> d(out)^T; call site vqgan.py:195) */
int prx_k_softmax_rows_tr_op(const float* S, int lds_, float scale, void* P, int ldp, void* PT, int ldpt, int rows, int cols,
                             const void* tin, int ldtin, void* tout, int ldtout, int tR, int tC, int prec, prx_stream_t s);
int prx_k_softmax_rows_bwd_tr_op(const void* P, int ldp, const float* dP, int lddp, float scale, void* dS, int ldds, void* dST,
                                 int lddst, int rows, int cols, const void* tin, int ldtin, void* tout, int ldtout, int tR, int tC,
                                 int prec, prx_stream_t s);
int prx_k_transpose_op(const void* in, int ldin, void* out, int ldout, int R, int C, int f32, prx_stream_t s);
int prx_k_upsample2x_bwd_op(const void* hi, float* low, void* low16, int NB, int Hl, int Wl, int C, int h16, int s16,
                            prx_stream_t s);
int prx_k_nchw_to_nhwc_op(const float* in, float* out_f32, void* out16, int NB, int C, int HW, int Cpad, int h16, prx_stream_t s);
int prx_k_image_head_bwd_op(const float* x, int ldc, const float* gimg, float* dx, void* dx16, int ldo, int NB, int C, int HW,
                            int h16, const float* gscale, prx_stream_t s);
/* ... written as the im2col matrix [H*W][ldk] of the 3x3 convolution that follows (tap-major, 8 channels per tap, columns
 * 72 .. ldk-1 zero); batch 1 */
int prx_k_image_head_bwd_im2col(const float* x, int ldc, const float* gimg, void* col, int ldk, int C, int H, int W, int h16,
                                const float* gscale, prx_stream_t s);
/* power-of-two gradient scale of the half mode: scale2 = {S, 1/S}, S * max|g| in [2^(T-1), 2^T), T = target_log2; S = 1 for an
 * all-zero gradient or one that holds an inf or a NaN.  part: nparts floats of scratch (count * nparts_each for _multi) */
int prx_k_grad_scale(const float* g, size_t n, float* part, int nparts, int target_log2, float* scale2, prx_stream_t s);
int prx_k_grad_scale_multi(const float* const* gs, const size_t* ns, int count, float* part, int nparts_each, int target_log2,
                           float* scale2, prx_stream_t s);
/* x[i] *= *scale (device scalar); out16 (optional): the scaled values in the 16-bit operand format */
int prx_k_scale_dev(float* x, size_t n, const float* scale, void* out16, int h16, prx_stream_t s);
int prx_k_f32_to_op16(const float* in, void* out16, size_t n, int h16, prx_stream_t s);
int prx_k_add_f32(const float* a, const float* b, float* out, size_t n, prx_stream_t s);

/* ---- the runners' own kernels, each through the host launcher its runner calls (csrc/resnet.h, cutouts.h, vgg.h, vit.h,
   clip_text.h, prompt_vq.h, vqgan.h, vqgan_enc.h), one kernel at a time (tests/test_kernels_runner_gpu.py).  `prec` = PRX_PREC_*
   selects the operand element type of the `void*` buffers.  Test surface only: the product's Python never calls them. ---- */
/* CLIP ModifiedResNet (resnet.hip) */
int prx_k_rn_pack_conv3x3(const float* w, void* Wf, void* Wd, int Cout, int Cin, int prec, prx_stream_t s);
int prx_k_stem1_fwd(const float* cut, const float* mm, const float* w, const float* b, void* out, int N, int S, int CO, int prec,
                    prx_stream_t s);
int prx_k_stem1_bwd(const void* g, const float* w, float* dY, int N, int S, int CO, const float* oscale_dev, int prec, prx_stream_t s);
int prx_k_avgpool2_fwd(const void* x, void* out, int N, int H, int W, int C, int prec, prx_stream_t s);
int prx_k_avgpool2_bwd(const float* g, const void* mask, float* dx_f32, void* dx_op, int N, int H, int W, int C, int prec,
                       prx_stream_t s);
int prx_k_relu_mask(float* g, const void* out, void* g_op, size_t n, int prec, prx_stream_t s);
int prx_k_tokens_fwd(const float* x, const float* pos, void* t, int N, int P, int C, int prec, prx_stream_t s);
int prx_k_tokens_bwd(const float* dt, float* dx, int N, int P, int C, int prec, prx_stream_t s);
int prx_k_tok0_gather(const void* t, void* out, int N, int T, int C, int prec, prx_stream_t s);
int prx_k_tok0_scatter(const void* g0, void* dt, int N, int T, int C, int prec, prx_stream_t s);
/* OpenCLIP ConvNeXt (convnext.hip).  Maps are NHWC [N][H][W][C], C a multiple of 8, N*H*W*C below 2^31.
 * pack_dw: the depthwise weight [C][49] as [2][49][C] in the operand format, the taps as given and flipped (the data gradient's).
 * dwconv: out = 7x7 depthwise convolution of x with padding 3, taps pack[flip] [+ bias[c]] [+ add (fp32 [N][H][W][C])]; out_op
 *   (operand format) and / or out_f32.  space_to_depth: [N][H][W][C] -> [N][H/2][W/2][4C], output channel (dy * 2 + dx) * C + c;
 *   depth_to_space takes the [N][H/2][W/2][4C] map back (N, H, W, C are those of the large map in both).  avgpool_fwd: the mean over
 *   HW of [N][HW][C] as fp32 [N][C]; avgpool_bwd: g[n][c] / HW on every pixel.  layernorm: over the channels of `rows` pixels; x is
 *   fp32 when x_f32, else in the operand format; group > 0: x (and dx) have one unused leading row per `group` rows (the stem). */
int prx_k_cnx_pack_dw(const float* w, void* pack, int C, int prec, prx_stream_t s);
int prx_k_cnx_dwconv(const void* x, const void* pack, const float* bias, const float* add, void* out_op, float* out_f32, int N, int H,
                     int W, int C, int flip, int prec, prx_stream_t s);
int prx_k_cnx_space_to_depth(const void* in, void* out, int N, int H, int W, int C, int prec, prx_stream_t s);
int prx_k_cnx_depth_to_space(const void* in, void* out, int N, int H, int W, int C, int prec, prx_stream_t s);
int prx_k_cnx_avgpool_fwd(const void* x, float* out, int N, int HW, int C, int prec, prx_stream_t s);
int prx_k_cnx_avgpool_bwd(const float* g, float* dx_f32, void* dx_op, int N, int HW, int C, int prec, prx_stream_t s);
int prx_k_cnx_layernorm_fwd(const void* x, int x_f32, const float* gamma, const float* beta, void* out_op, float* out_f32, float* mean,
                            float* rstd, int rows, int C, float eps, int group, int prec, prx_stream_t s);
int prx_k_cnx_layernorm_bwd(const float* g, const void* x, int x_f32, const float* gamma, const float* mean, const float* rstd,
                            void* dx_op, float* dx_f32, int rows, int C, int group, int prec, prx_stream_t s);
/* batch min / max, patchify and the min/max renormalisation backward (cutouts.hip); m0..s2: the channel means / stds */
int prx_k_minmax(const float* x, size_t n, float* part, int nparts, float* mm, prx_stream_t s);
int prx_k_patchify_fwd(const float* cut, const float* mm, void* A, int prec, int N, int S, int P, int T, float m0, float m1, float m2,
                       float s0, float s1, float s2, prx_stream_t s);
int prx_k_patchify_bwd_reduce(const float* cut, const float* mm, const float* dA, double* acc, int N, int S, int P, int T, float m0,
                              float m1, float m2, float s0, float s1, float s2, prx_stream_t s);
int prx_k_patchify_bwd_apply(const float* cut, const float* mm, const float* dA, const double* acc, float* gcut, int N, int S, int P,
                             int T, float m0, float m1, float m2, float s0, float s1, float s2, prx_stream_t s);
int prx_k_preproc_bwd_reduce(const float* cut, const float* mm, const float* dY, double* acc, int N, int S, prx_stream_t s);
int prx_k_preproc_bwd_apply(const float* cut, const float* mm, const float* dY, const double* acc, float* gcut, int N, int S,
                            prx_stream_t s);
/* the cutout stages one at a time (cutouts.hip; tests/test_kernels_cutouts_gpu.py).  desc: n_cut descriptors of 36 doubles (layout: at
 * prx_cutouts_forward).  uv: [n_cut][dst pixels][2] floats of scratch; gsrc_priv: [n_cut][3][Hs][Ws] scratch, gsrc: [3][Hs][Ws] their sum;
 * grgb: [n_cut][3][S][S], the incoming gradient pulled back through the colour jitter (written for jittered cutouts only);
 * maps_scratch: >= 64 bytes per cutout (forms 0 and 1).  form: -1 = the PRX_CUTOUT_BWD environment switch decides (the product),
 * 0 = workgroup scatter, 1 = one-wave scatter, 2 = per-pixel gather */
int prx_k_pool_fwd(const float* img, float* pooled, int* argmax, const unsigned char* mask, int C, int H, int W, int S, prx_stream_t s);
int prx_k_pool_bwd(const float* g, const int* argmax, const unsigned char* mask, float* gimg, int C, int H, int W, int S, prx_stream_t s);
int prx_k_rescale_fwd(const float* pooled, float* base, int C, int S, int Hb, int Wb, prx_stream_t s);
int prx_k_rescale_bwd(const float* g_base, float* g_pooled, int C, int S, int Hb, int Wb, prx_stream_t s);
int prx_k_warp_a_fwd(const float* src, int Hs, int Ws, const double* desc, float* out, int n_cut, int Ha, int Wa, prx_stream_t s);
int prx_k_warp_a_bwd(const float* g, int Hs, int Ws, const double* desc, float* uv, float* gsrc_priv, float* gsrc, int n_cut, int Ha,
                     int Wa, int form, prx_stream_t s);
int prx_k_warp_b_fwd(const float* a, int Ha, int Wa, const double* desc, const float* noise, float* out, int n_cut, int S,
                     prx_stream_t s);
int prx_k_warp_b_bwd(const float* a, int Ha, int Wa, const double* desc, const float* g, float* grgb, float* uv, float* ga, int n_cut,
                     int S, float* maps_scratch, size_t maps_scratch_bytes, int form, prx_stream_t s);
/* Form 0 of the two warp backwards runs the tiles of an axis-aligned affine stage under zeros / fill padding through a separable
 * gather (two 1-D coordinate tables, proved exact per tile) and every other tile through the scatter.  prx_cutout_bwd_separable
 * switches that path for the following launches of the process (a captured graph keeps the value it was captured with):
 * 0: off, form 0 is exactly the scatter; 1: on, the sums in the per-pixel gather's order (equal to form 2 bit for bit); 2: on, the
 * same terms in the scatter's order (equal to setting 0 bit for bit: the iteration keeps its bits); -1: query.  Returns the previous
 * value.  Default 2; PRX_CUTOUT_BWD_SEP=0 / =1 in the environment start the process at 0 / 1. */
int prx_cutout_bwd_separable(int on);
/* VGG16 extractor (vgg.hip) */
int prx_k_vgg_pack(const float* w, void* Wf, void* Wd, int Cout, int Cin, int CiP, int prec, prx_stream_t s);
int prx_k_vgg_input(const float* x, void* out, int HW, int prec, prx_stream_t s);
int prx_k_vgg_input_grad(const float* d, float* gx, int HW, const float* unscale, prx_stream_t s);
int prx_k_vgg_maxpool(const void* x, void* out, void* arg, int H, int W, int C, int prec, prx_stream_t s);
int prx_k_vgg_combine(const float* above, const void* arg, const float* gcap, const void* act, void* gpre, int H, int W, int C,
                      const float* gscale, int prec, prx_stream_t s);
/* ViT runner (vit.hip) */
int prx_k_pack_transpose_op(const float* in, void* out, int R, int C, int prec, prx_stream_t s);
int prx_k_vit_add_cls_pos(float* x, const float* cls, const float* pos, int N, int T, int W, prx_stream_t s);
int prx_k_vit_embed_tokens(const float* x, const float* cls, const float* pos, void* out, int out16, int N, int T, int W,
                           prx_stream_t s);
int prx_k_vit_gelu_f32(const float* t, float* io, size_t n, int bwd, prx_stream_t s);
int prx_k_vit_scale_f32(float* x, size_t n, float scale, int blocks, prx_stream_t s);
/* CLIP text tower (clip_text.hip) */
int prx_k_text_embed(const int* tokens, const float* emb, const float* pos, float* x, int* eot, int n, int ctx, int W, int vocab,
                     prx_stream_t s);
int prx_k_gather_rows(const float* x, const int* eot, float* out, int n, int ctx, int W, prx_stream_t s);
/* prompt_vq.hip (prx_k_sqnorm_rows: above) */
int prx_k_l2norm_fwd(const float* e, float* out, int n, int D, prx_stream_t s);
int prx_k_l2norm_bwd(const float* e, const float* g, float* de, int n, int D, prx_stream_t s);
/* VQGAN decoder / encoder weight packs and the codebook's column bounds (vqgan.hip, vqgan_enc.hip) */
int prx_k_vqgan_pack_conv3x3(const float* w, void* Wf, void* Wd, int Cout, int Cin, int CoP, int prec, prx_stream_t s);
int prx_k_vqgan_enc_pack_conv3x3(const float* w, void* Wf, int Cout, int Cin, int CiP, prx_stream_t s);
int prx_k_colminmax(const float* w, float* mn, float* mx, int rows, int D, prx_stream_t s);
/* The one 3x3 weight pack behind the four pack entries above (csrc/weight_pack.h), with both paddings at once:
 * Wf [Cout][9*CiP], Wf[co][tap*CiP + ci] = w[co][ci][ky][kx]; Wd [CiP][9*CoP], Wd[ci][tap*CoP + co] = w[co][ci][2-ky][2-kx]; the
 * padding is zero.  Either pack may be null, not both; CiP >= Cin and CoP >= Cout. */
int prx_k_pack_conv3x3(const float* w, void* Wf, void* Wd, int Cout, int Cin, int CiP, int CoP, int prec, prx_stream_t s);

/* ------------------------------------------------------------------------ */
/* Path-level operators: the drop-in boundary of the hot path                */
/* ------------------------------------------------------------------------ */

/* --- VqganDrawer (vqgan.py:83-214): synth = vector_quantize (60-64, straight-through 48-58) ->
 *     taming VQModel.decode [UPSTREAM] -> add(1).div(2) -> clamp_with_grad(0,1) (66-79,195).
 * weights[]: fp32 device tensors in taming state-dict order:
 *   quantize.embedding.weight [n_embed, embed_dim];
 *   post_quant_conv.{weight[zc,ed,1,1], bias}; decoder.conv_in.{weight, bias};
 *   mid.block_1 (ResnetBlock), mid.attn_1 (AttnBlock), mid.block_2;
 *   for level = n_mult-1 .. 0: (num_res_blocks+1) x [ResnetBlock (+ AttnBlock at attn_resolution)], then
 *     upsample.conv.{weight,bias} when level != 0;
 *   norm_out.{weight,bias}; conv_out.{weight,bias}.
 *   ResnetBlock = norm1.{w,b}, conv1.{w,b}, norm2.{w,b}, conv2.{w,b} [, nin_shortcut.{w,b} if Cin != Cout]
 *   AttnBlock   = norm.{w,b}, q.{w,b}, k.{w,b}, v.{w,b}, proj_out.{w,b}
 * The caller may free the weight tensors after the stream has drained. */
typedef struct prx_vqgan prx_vqgan;
typedef struct prx_vqgan_config {
    int ch;                /* 128 */
    int ch_mult[8];        /* {1,1,2,2,4} */
    int n_mult;            /* 5 -> f = 16 (DrawingInterface.get_num_resolutions, vqgan.py:187-188) */
    int num_res_blocks;    /* 2 */
    int attn_resolution;   /* 16 */
    int resolution;        /* nominal training resolution of the config, 256 */
    int z_channels;        /* 256 */
    int embed_dim;         /* 256 */
    int n_embed;           /* 16384 */
    int out_ch;            /* 3 */
    int latent_h, latent_w;/* z is [1, z_channels, latent_h, latent_w] */
    int precision;         /* PRX_PREC_F16 | PRX_PREC_BF16 (fast paths) | PRX_PREC_F32 (exact-f32 MFMA parity mode); the encoder ignores it */
} prx_vqgan_config;
int prx_vqgan_create(prx_vqgan** out, const prx_vqgan_config* cfg, const float* const* weights, int n_weights,
                     prx_stream_t s);
void prx_vqgan_destroy(prx_vqgan* h);
/* per-channel codebook min/max used by VqganDrawer.clip_z (vqgan.py:155-158, 202-204) */
int prx_vqgan_z_bounds(prx_vqgan* h, float* zmin, float* zmax, prx_stream_t s);
/* z [1,zc,h,w] -> img [1,out_ch,16h,16w] in [0,1]; indices (optional, int32 [h*w]) = chosen codes;
 * quantize=0 skips the VQ step (decode of an already-quantised latent). */
int prx_vqgan_synth(prx_vqgan* h, const float* z, float* img, int* indices, int quantize, prx_stream_t s);
/* d loss / d img -> d loss / d z of the forward in flight on this handle */
int prx_vqgan_synth_backward(prx_vqgan* h, const float* g_img, float* dz, prx_stream_t s);
/* Diagnostic (tools/debug_repeat.py, tests): copies one intermediate of the last forward, fp32, to dst and returns the
 * number of floats copied (-1: bad stage).  stage -2 quantised latent, -1 conv_in output, 0..n-1 decoder stage outputs,
 * n conv_out output [H*W,4], n+1 the forward GroupNorm sums. */
long long prx_vqgan_debug_stage(prx_vqgan* h, int stage, float* dst, long long max_floats, prx_stream_t stream);

/* --- VqganDrawer.init_from_tensor / reapply_from_tensor / get_z_from_tensor (vqgan.py:174-185):
 *     `z, *_ = model.encode(img)` = taming Encoder -> quant_conv -> VectorQuantizer2 nearest code [UPSTREAM].  Forward only.
 * cfg: the same prx_vqgan_config (out_ch unused; latent_h/latent_w ignored: the latent is H/f x W/f).
 * weights[]: fp32 device tensors in this order:
 *   quantize.embedding.weight [n_embed, embed_dim]; encoder.conv_in.{weight,bias};
 *   for level = 0 .. n_mult-1: num_res_blocks x [ResnetBlock (+ AttnBlock at attn_resolution)], then
 *     downsample.conv.{weight,bias} when level != n_mult-1;
 *   mid.block_1, mid.attn_1, mid.block_2; norm_out.{weight,bias}; conv_out.{weight,bias}; quant_conv.{weight,bias}.
 * img: NCHW [1, in_channels, H, W] fp32 in [-1,1] (pixray.py:718-727); z: NCHW [1, embed_dim, H/f, W/f] = the chosen code
 * vectors; z_pre (optional): the latent before quantisation; indices (optional): int32 [H/f * W/f]. */
typedef struct prx_vqgan_enc prx_vqgan_enc;
int prx_vqgan_enc_create(prx_vqgan_enc** out, const prx_vqgan_config* cfg, int in_channels, int H, int W,
                         const float* const* weights, int n_weights, prx_stream_t s);
void prx_vqgan_enc_destroy(prx_vqgan_enc* h);
int prx_vqgan_encode(prx_vqgan_enc* h, const float* img, float* z, float* z_pre, int* indices, prx_stream_t s);

/* --- VGG16 feature extractor of the StyleLoss plugin (Losses/StyleLoss.py:24-47: torchvision `vgg16().features`, frozen,
 * the nine captured ReLU outputs at features[1,3,6,8,11,13,15,22,29]).  Batch 1, any H x W in [16, max] x [16, max].
 * weights: fp32 device pointers in torchvision order {features.N.weight [Cout,Cin,3,3], features.N.bias} for the 13 convs.
 * x: [3,H,W] fp32, already in the extractor's input space (StyleLoss.py:41-45 normalises outside this call).
 * feats[k] (k = 0..8, or NULL when not wanted): fp32 NHWC [h_k*w_k, C_k], shape from prx_vgg16_feature_shape.
 * workspace: caller-owned device buffer of prx_vgg16_workspace_bytes(H, W) bytes holding this forward's activations; the
 * matching backward reads it, so any number of forward passes can be alive at once.  precision: PRX_PREC_BF16 | PRX_PREC_F16 |
 * PRX_PREC_F32 (the workspace of the exact mode is twice as large; the half mode's backward runs under the power-of-two
 * gradient scale described at PRX_PREC_F16, chosen from max |g_feats| on the device).
 * backward: g_feats[k] fp32 NHWC gradient of feature k (or NULL); g_x: [3,H,W] fp32, overwritten. */
typedef struct prx_vgg16 prx_vgg16;
int prx_vgg16_create(prx_vgg16** out, const float* const* weights, int n_weights, int max_h, int max_w, int precision,
                     prx_stream_t s);
void prx_vgg16_destroy(prx_vgg16* h);
long long prx_vgg16_workspace_bytes(int H, int W, int precision);
int prx_vgg16_feature_shape(int H, int W, int k, int* h, int* w, int* c);
int prx_vgg16_forward(prx_vgg16* h, const float* x, int H, int W, void* workspace, float* const* feats, prx_stream_t s);
int prx_vgg16_backward(prx_vgg16* h, int H, int W, const void* workspace, const float* const* g_feats, float* g_x, prx_stream_t s);

/* --- the fft drawer's spectrum -> image map and its backward (BASELINE.json configs[3]; fftdrawer.py:45-62 `init_from_tensor`,
 * 79-86 `synth`: aphantasia fft_image(sd 0.01, decay_power) + to_valid_rgb(colors), evaluated at `contrast`):
 *   image = sigmoid(colour matrix (irfft2(scale * spectrum, s = (H, W), norm = "ortho") * contrast / std))
 * The inverse real transform runs as exact-f32 GEMMs against twiddle matrices built in float64 at creation (no FFT library;
 * csrc/fft_drawer.hip).  params / g_params: fp32 [3][H][Wf][2] (real, imaginary), Wf = prx_fft_drawer_freq_columns() =
 * W/2 + 1, or W/2 + 2 for an odd W (the surplus column of the lucid frequency helper is ignored and gets a zero gradient).
 * image / g_image: fp32 [3][H][W] in (0,1).  backward differentiates the LAST synth of the handle (it keeps the
 * un-normalised image and its moments).  Asynchronous on `stream`; one handle per canvas size, not shared between threads. */
typedef struct prx_fft_drawer prx_fft_drawer;
prx_fft_drawer* prx_fft_drawer_create(int W, int H, float decay, float colors);
void prx_fft_drawer_destroy(prx_fft_drawer* h);
int prx_fft_drawer_freq_columns(const prx_fft_drawer* h);
int prx_fft_drawer_synth(prx_fft_drawer* h, const float* params, float contrast, float* image, prx_stream_t stream);
int prx_fft_drawer_backward(prx_fft_drawer* h, const float* g_image, float* g_params, prx_stream_t stream);
/* Test surface.  Read-only copy of one of the handle's tables into a device buffer of exactly its size, fp32:
 *   0 scale [H][Wh]   1 A1 [W][K1p]   2 A1T [K1p][WP]   3 T2 [H][HP2]   4 T2T [HP2][HP]   5 colour matrix [c][d]
 * with Wh = W/2 + 1 and the padded strides HP = up4(H), HP2 = up4(2 H), WP = up4(W), K1p = up4(2 Wh) (up4: next multiple of 4). */
int prx_fft_drawer_table(const prx_fft_drawer* h, int which, float* dst, size_t dst_elems, prx_stream_t stream);
/* The drawer's kernels one at a time, through the launchers synth / backward call (csrc/fft_drawer.h), for a W x H canvas:
 *   pack:     params [3][H][Wf][2], scale [H][Wh] -> bt1 [3 HP2][K1p] (both copies of the spectrum, (re, im) and i * it, times scale)
 *   unpack:   dP [3 HP2][K1p], scale -> g_params [3][H][Wf][2] (the adjoint of pack)
 *   moments:  acc[0..2] = sum x, sum x^2, sum x y (y may be null: 0) over n elements, in double and in a fixed order;
 *             part: scratch of 3 * min(ceil(n / 256), 1024) doubles
 *   tail_fwd: x [3][H][W], acc = moments(x) -> rgb [3][H][W] = sigmoid(cm^T (contrast / std) x), std unbiased over all of x
 *   tail_bwd_gy: g = d/d(rgb) -> gy = d/d(contrast / std * x) [3][H][W]
 *   tail_bwd_dx: bacc = moments(gy, x) -> dxT [3][W][HP] = d/dx, transposed, rows zero padded to HP */
int prx_k_fft_pack(const float* params, const float* scale, float* bt1, int W, int H, prx_stream_t s);
int prx_k_fft_unpack(const float* dP, const float* scale, float* g_params, int W, int H, prx_stream_t s);
int prx_k_fft_moments(const float* x, const float* y, size_t n, double* part, double* acc, prx_stream_t s);
int prx_k_fft_tail_fwd(const float* x, const double* acc, float contrast, const float* cm, float* rgb, int W, int H, prx_stream_t s);
int prx_k_fft_tail_bwd_gy(const float* x, const float* g, const double* acc, float contrast, const float* cm, float* gy, int W, int H,
                          prx_stream_t s);
int prx_k_fft_tail_bwd_dx(const float* x, const float* gy, const double* acc, const double* bacc, float contrast, float* dxT, int W, int H,
                          prx_stream_t s);

/* --- SuperResolutionDrawer.synth (super_resolution.py:34-102): clamp_with_grad(RRDBNet(z), 0, 1), the RealESRGAN x4 network
 * [UPSTREAM basicsr/archs/rrdbnet_arch.py] with the drawer's arguments (scale 4, no tiling, no padding, fp32), and its data
 * gradient (the weights are frozen).  csrc/rrdbnet.hip, layout and memory formula in csrc/rrdbnet.h.
 *   z / g_z: fp32 [3][h][w] in [0,1];  image / g_image: fp32 [3][4h][4w].
 *   weights: 2 (15 num_block + 6) fp32 device tensors in torch layout, (weight [Cout][Cin][3][3], bias [Cout]) per convolution,
 *   in the order conv_first, body.{i}.rdb{1,2,3}.conv{1..5}, conv_body, conv_up1, conv_up2, conv_hr, conv_last; they are
 *   copied / packed on `stream` at creation (synchronise before releasing them).
 *   The kernels are built for num_feat = 64, num_grow = 32 and PRX_PREC_F16 / PRX_PREC_F32; anything else is refused by name.
 * clamp = 0: image = the raw network output and backward is the identity rule (tests).  backward differentiates the handle's
 * LAST synth.  Everything is allocated at creation; synth / backward only launch on `stream` and never synchronise. */
typedef struct prx_rrdbnet prx_rrdbnet;
int prx_rrdbnet_create(prx_rrdbnet** out, int num_feat, int num_grow, int num_block, int h, int w, const float* const* weights,
                       int n_weights, int precision, prx_stream_t stream);
void prx_rrdbnet_destroy(prx_rrdbnet* h);
int prx_rrdbnet_synth(prx_rrdbnet* h, const float* z, float* image, int clamp, prx_stream_t stream);
int prx_rrdbnet_backward(prx_rrdbnet* h, const float* g_image, float* g_z, prx_stream_t stream);
/* one 3x3 convolution of the family on caller-owned buffers (synchronises: a test entry).  T = half / float by `prec`.
 * forward (dgrad = 0): in T [pixels][ld_in], channels in_off .. + Cin -> v = conv + bias, LeakyReLU(0.2) if lrelu, then
 *   v = alpha v + beta r1 + r2 (r1, r2: fp32 [pixels][ld_r*], first 64 channels, null: absent), written as T into
 *   out[pixels][ld_out] at out_off and / or as fp32 into out_f32 at of_off.  H x W: the output grid; up: in is [H/2][W/2],
 *   read nearest-2x.
 * data gradient (dgrad = 1): in fp32 [pixels][ld_in], the gradient of the Cout outputs at in_off, multiplied on load by the
 *   LeakyReLU derivative of act (T [pixels][ld_act] at act_off; a > 0: 1, else 0.2; null: none); the Cin results go through the
 *   same v = alpha v + beta r1 + r2 and are stored (accum = 0) or added (accum = 1) into out_f32 at of_off.
 * wt: the torch weight [Cout][Cin][3][3] fp32; Cin, Cout multiples of 32. */
int prx_k_rrdb_conv(int dgrad, const void* in, int ld_in, int in_off, const void* act, int ld_act, int act_off, const float* wt,
                    const float* bias, int Cin, int Cout, int H, int W, int up, int lrelu, float alpha, float beta, const float* r1,
                    int ld_r1, const float* r2, int ld_r2, void* out, int ld_out, int out_off, float* out_f32, int ld_of, int of_off,
                    int accum, int prec, prx_stream_t stream);
/* the backward of a nearest-2x read: out [h][w][64] = 2 x 2 block sums of in [2h][2w][64] */
int prx_k_rrdb_sum2x2(const float* in, float* out, int h, int w, int C, prx_stream_t stream);
/* conv_first (3 -> 64: z NCHW fp32 -> T [pixels][ld_out] and / or fp32 [pixels][64]) and its data gradient of g1 + g2 */
int prx_k_rrdb_conv_first(const float* z, const float* wt, const float* bias, int h, int w, void* out, int ld_out, float* out_f32, int prec,
                          prx_stream_t stream);
int prx_k_rrdb_conv_first_bwd(const float* g1, int ld1, const float* g2, int ld2, const float* wt, int h, int w, float* dz, prx_stream_t stream);
/* conv_last (64 -> 3: T [pixels][64] -> image NCHW fp32, clamped to [0,1] if clamp; raw: the un-clamped values) and its
 * backward: g_image through g * ((g * (raw - clamp(raw))) >= 0) if clamp, then the data gradient -> g_out fp32 [pixels][64] */
int prx_k_rrdb_conv_last(const void* in, const float* wt, const float* bias, int H, int W, int clamp, float* image, float* raw, int prec,
                         prx_stream_t stream);
int prx_k_rrdb_conv_last_bwd(const float* g_image, const float* raw, const float* wt, int H, int W, int clamp, float* g_out, prx_stream_t stream);

/* --- STROTSS hyper-column sampling of the StyleLoss plugin (`spatial_feature_extract`, Losses/StyleLoss.py:169-223): n
 * positions, one bilinear sample of each of n_layers NHWC fp32 feature maps per position, concatenated over channels, plus
 * the two coordinate channels -> out [n, ldo] (ldo >= sum(channels) + 2).
 * feats / g_feats / channels: HOST arrays of n_layers device pointers / channel counts.  rows: device int64 [n_layers][4][n],
 * flat row (pixel) index of the four taps; weights: device fp32 [4*n_layers + 2][n], the tap weights, then the x and y
 * coordinate channels.  Same roundings as the composed torch expression (products added left to right).
 * backward: g_feats[l] (or NULL) must be zero-initialised [h_l*w_l, C_l]; adds weight * g_out to the four taps. */
int prx_hypercolumns_fwd(const float* const* feats, const int* channels, int n_layers, const long long* rows, const float* weights,
                         int n, float* out, int ldo, prx_stream_t s);
int prx_hypercolumns_bwd(float* const* g_feats, const int* channels, int n_layers, const long long* rows, const float* weights,
                         int n, const float* g_out, int ldo, prx_stream_t s);

/* --- STROTSS distance arithmetic of the StyleLoss plugin (Losses/StyleLoss.py:225-293), csrc/strotss.hip.  All matrices fp32
 * row-major on the device; the products G = X Y^T are the caller's (plain library GEMMs).
 * xs / ys: the squared row norms `pairwise_distances_cos` / `_sq_l2` take (225-237), the caller's reductions.
 * remd_fwd (`style_loss`, 272-293): G [n, m], xs [n], ys [m] -> stats = {max(rmean, cmean), rmean, cmean} where rmean / cmean are
 *   the means of the row / column minima of M = 1 - (G / |x|) / |y| (+ sqrt(clamp(|x|^2 + |y|^2 - 2 G, 1e-5, 1e5) / d) when l2:
 *   the 3-channel palette term); rowpack [n] / colpack [m]: {ordered value << 32 | position} of each minimum (ties: smallest
 *   position), kept for the backward.
 * remd_bwd: dX [n, d] = g_out[0] * d stats[0] / dX, visiting only the n + m selected pairs (X [n, d], Y [m, d]; Y takes no gradient:
 *   it is the style image's), a row's pairs in chunks of 32 per workgroup, added in ascending column order (no floating-point
 *   atomics).  d <= 4096; workspace: remd_bwd_workspace_bytes(n, m, d) bytes, 16-byte aligned.
 * selfsim_fwd (`content_loss`, 246-265): out[0] = mean |D(X, X) - D(Y, Y)| from Gx = X X^T, Gy = Y Y^T [n, n]; partial: n doubles.
 * selfsim_bwd: Sx / Sy [n, lds] = dL/dG + (dL/dG)^T of each product and cx / cy [n] such that dX = Sx X + cx (.) X (rows scaled),
 *   dY = Sy Y + cy (.) Y. */
long long prx_strotss_remd_bwd_workspace_bytes(int n, int m, int d);
int prx_strotss_remd_fwd(const float* G, int ldg, const float* xs, const float* ys, int n, int m, int l2, int d,
                         unsigned long long* rowpack, unsigned long long* colpack, float* stats, prx_stream_t s);
int prx_strotss_remd_bwd(const float* G, int ldg, const float* X, int ldx, const float* Y, int ldy, int d, const float* xs, const float* ys,
                         const unsigned long long* rowpack, const unsigned long long* colpack, int n, int m, int l2, const float* stats,
                         const float* g_out, void* workspace, long long workspace_bytes, float* dX, int lddx, prx_stream_t s);
int prx_strotss_selfsim_fwd(const float* Gx, int ldgx, const float* xs, const float* Gy, int ldgy, const float* ys, int n,
                            double* partial, float* out, prx_stream_t s);
int prx_strotss_selfsim_bwd(const float* Gx, int ldgx, const float* xs, const float* Gy, int ldgy, const float* ys, int n,
                            const float* g_out, float* Sx, float* Sy, int lds, float* cx, float* cy, prx_stream_t s);

/* --- MakeCutouts.forward (pixray.py:445-511) with explicit randomness.
 * desc: fp64 [n_cut][36] per-cutout descriptor (built by pixray_amd/cutouts.py::build_descriptors):
 *   [0..8] stage-A 3x3, [9..17] stage-B 3x3: kornia's src_norm_trans_dst_norm (normalised destination
 *          coords -> normalised source coords, [0,W-1]->[-1,1] convention),
 *   [18] stage-A mode, [19] stage-B mode (0 copy, 1 zeros, 2 border, 3 reflection, 4 fill, 5 reflection under align_corners=True),
 *   [20] fill gray, [21] jitter on/off, [22] saturation factor, [23] hue shift (rad), [24] saturation-first,
 *   [25] noise factor, [26]/[27] stage-A/B grid flavour = which kornia 0.6.2 call built the sampling grid AND the
 *   align_corners flag that call hands to F.grid_sample (the convention is data, pixray_amd.cutouts.KORNIA_062_CONVENTIONS):
 *   0 warp_perspective(align_corners=False): create_meshgrid + transform_points, sampled with (g+1)*W/2-0.5 (RandomPerspective);
 *   1 warp_affine(align_corners=False): F.affine_grid pixel-centre grid (RandomAffine); 2 warp_affine(align_corners=True):
 *   corner-aligned grid sampled with (g+1)/2*(W-1) (RandomResizedCrop / CenterCrop via crop_by_transform_mat);
 *   3 warp_perspective(align_corners=True) (the cached-transform path, pixray.py:482-485),
 *   [28..31] stage-B source window (x, y, width, height) inside the stage-A image,
 *   [32] noise seed (an integer < 2^53, 0 = none): with `noise` NULL and a non-zero factor [25] the cutout's additive N(0,1)
 *        draws (pixray.py:508-510, randn_like) are generated in the kernel -- Philox4x32-10 keyed by the seed, counter = pixel
 *        index, Box-Muller; [33..35] reserved (zero).
 * Geometry: the canvas is pooled to [3,S,S] (pixray.py:463); on a W != H canvas the reference rescales that to the
 * canvas aspect (pixray.py:468-472): the "base" image [3,Hb,Wb] with Hb == S or Wb == S (Hb = Wb = S on a square
 * canvas, `base` may then be NULL).  Stage A renders [n_cut,3,Hb,Wb] from the base, stage B the S x S cutouts.
 * noise: fp32 [n_cut,3,S,S] explicit N(0,1) draws (parity tests hand the oracle's), or NULL (see [32]).  pooled/argmax/base/stage_a are caller-owned save-for-backward
 * buffers ([3,S,S] f32, [3,S,S] i32, [3,Hb,Wb] f32, [n_cut,3,Hb,Wb] f32).
 * spot_mask (optional): uint8 [3,S,S]; pooled pixels where it is non-zero are set to 0 (spot prompts, pixray.py:453-466). */
int prx_cutouts_forward(const float* img, int H, int W, const double* desc, const float* noise, const unsigned char* spot_mask,
                        int n_cut, int S, int Hb, int Wb, float* pooled, int* argmax, float* base, float* stage_a, float* out,
                        prx_stream_t s);
/* scratch: g_stage_a and g_base_priv are [n_cut,3,Hb,Wb] fp32 each, uv_scratch is [n_cut,Hb*Wb,2] fp32 (the forward's sampling
 * coordinates, recomputed per stage), g_base is [3,Hb,Wb], g_pooled is [3,S,S].  The backward is in
 * gather form (every source pixel sums its contributions in a fixed order): no atomics, bit-reproducible (cf. pixray.py:29). */
int prx_cutouts_backward(const float* g_out, const double* desc, const unsigned char* spot_mask, int n_cut, int S, int Hb, int Wb,
                         int H, int W, const float* stage_a, const int* argmax, float* g_stage_a, float* g_base_priv, float* uv_scratch,
                         float* g_base, float* g_pooled, float* g_img, prx_stream_t s);

/* --- CLIP_Base.encode_image (slip.py:62-66) for a ViT visual tower [UPSTREAM clip/model.py].
 * weights[]: fp32 device tensors in OpenAI state-dict order under `visual.`:
 *   conv1.weight, class_embedding, positional_embedding, ln_pre.{weight,bias},
 *   per layer: ln_1.{weight,bias}, attn.in_proj_{weight,bias}, attn.out_proj.{weight,bias},
 *              ln_2.{weight,bias}, mlp.c_fc.{weight,bias}, mlp.c_proj.{weight,bias},
 *   ln_post.{weight,bias}, proj.
 * The batch-global min/max renorm (slip.py:21-36) couples all cutouts, so the call sequence is split to
 * let a sharded caller all-reduce the two small buffers in between:
 *   minmax(cutouts) -> mm[2] {min,max}      [all-reduce MIN/MAX over ranks]
 *   encode(cutouts, mm) -> embeds [n, output_dim] (unit vectors)
 *   backward_reduce(d_embeds) -> acc[4] doubles {sum g, sum g*y, #min, #max}   [all-reduce SUM]
 *   backward_finish(acc) -> g_cutouts [n,3,R,R] */
typedef struct prx_clip_vit prx_clip_vit;
typedef struct prx_clip_vit_config {
    int input_resolution;  /* 224; 336 (ViT-L/14@336px: 577 tokens) */
    int patch_size;        /* 32 | 16 | 14 */
    int width;             /* 768 | 1024 (ViT-L/14, ViT-L/14@336px) */
    int layers;            /* 12 | 24 */
    int heads;             /* 12 | 16 */
    int output_dim;        /* 512 | 768 */
    int max_batch;         /* capacity in cutouts: create allocates one forward's activations for this many; an allocation that fails
                              is an error of the call (rc < 0, prx_last_error names the bytes asked for and the bytes held), nothing stays
                              allocated -- as in every prx_*_create: a handle frees its device memory on every path (csrc/dev_arena.h) */
    int precision;         /* PRX_PREC_F16 | PRX_PREC_BF16 | PRX_PREC_F32 */
} prx_clip_vit_config;
int prx_clip_vit_create(prx_clip_vit** out, const prx_clip_vit_config* cfg, const float* const* weights, int n_weights,
                        prx_stream_t s);
/* --- the same runner for a tower FAMILY: SLIP_Base.encode_image (slip.py:151-157) runs a timm VisionTransformer
 *     (`timm.create_model(vit_*_patch16_224, num_classes=0)`) followed by `@ image_projection` [UPSTREAM facebookresearch/SLIP
 *     models.py, timm vision_transformer.py; the SLIP/ submodule is absent from the reference checkout, parity unpinned].
 *     Against the CLIP tower it has a patch-embed bias, no ln_pre, LayerNorm eps 1e-6, the exact GELU, and is fed through
 *     `Normalize` with the ImageNet constants (slip.py:117-121).  Returns the same handle type: minmax / encode /
 *     backward_reduce / backward_finish / destroy / gemm_ctx above are shared.
 * family PRX_VIT_FAMILY_CLIP: weights[] as for prx_clip_vit_create (ln_eps, mean, std as given: 1e-5 and CLIP's constants
 *   reproduce it bit for bit).
 * family PRX_VIT_FAMILY_SLIP: weights[] are fp32 device tensors in timm state-dict order under `visual.`:
 *   patch_embed.proj.weight [width,3,P,P], patch_embed.proj.bias, cls_token [1,1,width], pos_embed [1,T,width],
 *   per block i: blocks.i.norm1.{weight,bias}, blocks.i.attn.qkv.{weight [3 width, width] rows q|k|v, bias},
 *                blocks.i.attn.proj.{weight,bias}, blocks.i.norm2.{weight,bias}, blocks.i.mlp.fc1.{weight,bias},
 *                blocks.i.mlp.fc2.{weight,bias},
 *   norm.{weight,bias}, then `image_projection` [width, output_dim] (no bias).
 * head_dim: 0 / 64, or 32 / 16 (= width / heads; SLIP's ViT-S/16 has 12 heads of 32 on width 384).  Narrower heads are zero-padded
 *   to 64 when the weights are packed (q, k, v rows of qkv.weight / qkv.bias, input columns of proj.weight; sqrt(64 / head_dim)
 *   folded into the q rows): the values and gradients of the narrow heads, at 64 / head_dim times the qkv, attention and
 *   out-projection work.  width must be a multiple of 128.
 *   80 (OpenCLIP ViT-H/14: 16 heads on width 1280) is zero-padded to 96 the same way and runs on the 96-wide attention kernels, which
 *   take the softmax scale 1 / sqrt(80) as an argument (nothing is folded into q) and at most 640 tokens.
 *   88 (OpenCLIP ViT-g-14: 16 heads on width 1408) runs there too with 1 / sqrt(88); 104 (ViT-bigG-14: 16 heads on width 1664) is
 *   zero-padded to 128 and runs on the 128-wide instances of the same kernels with 1 / sqrt(104), at most 640 tokens.  Any other head
 *   dim is refused by name.
 * family PRX_VIT_FAMILY_OPENCLIP: the OpenCLIP (LAION) ViT towers [UPSTREAM open_clip model_configs ViT-B-32, ViT-B-16, ViT-L-14, ViT-H-14]:
 *   weights[] and every switch as for PRX_VIT_FAMILY_CLIP (no patch-embed bias, ln_pre, ln_eps 1e-5 and CLIP's constants as given),
 *   but the MLP activation is the exact GELU. */
#define PRX_VIT_FAMILY_CLIP 0
#define PRX_VIT_FAMILY_SLIP 1
#define PRX_VIT_FAMILY_OPENCLIP 2
typedef struct prx_vit_tower_config {
    int input_resolution;  /* 224 */
    int patch_size;        /* 16 */
    int width;             /* 768 | 1024 */
    int layers;            /* 12 | 24 */
    int heads;             /* 12 | 16 */
    int output_dim;        /* 512 */
    int max_batch;         /* capacity in cutouts */
    int precision;         /* PRX_PREC_F16 | PRX_PREC_BF16 | PRX_PREC_F32 (the reference runs this family in fp32 on a GPU) */
    int family;            /* PRX_VIT_FAMILY_* */
    int head_dim;          /* 0 = 64; 32 | 16: padded to 64; 80 | 88: padded to 96; 104: padded to 128 */
    float ln_eps;          /* 1e-6 (timm) | 1e-5 (CLIP) */
    float mean[3];         /* Normalize constants of the fused preprocessing: ImageNet's (0.485, 0.456, 0.406) */
    float std[3];          /* (0.229, 0.224, 0.225) */
} prx_vit_tower_config;
int prx_vit_tower_create(prx_clip_vit** out, const prx_vit_tower_config* cfg, const float* const* weights, int n_weights,
                         prx_stream_t s);
/* prx_vit_tower_create with the hidden width of the MLP as an argument: c_fc.weight [mlp_width, width], c_fc.bias [mlp_width],
 * c_proj.weight [width, mlp_width] (fc1 / fc2 of the SLIP family).  0 = 4 * width: prx_vit_tower_create itself.  OpenCLIP ViT-g-14 has
 * 6144 on width 1408, ViT-bigG-14 8192 on width 1664.  Must be a multiple of 8. */
int prx_vit_tower_create_mlp(prx_clip_vit** out, const prx_vit_tower_config* cfg, int mlp_width, const float* const* weights, int n_weights,
                             prx_stream_t s);
/* TEST DIAGNOSTIC, not part of the ABI contract (it may change or go without a version bump; no product code calls it): copies the
 * d(qkv) buffer as the last backward left it -- block 0's gradient, [n * T][3 * heads * 64] in the handle's operand format, padded
 * lanes included -- to dst.  Returns the bytes copied, or -1 when no forward is in flight or max_bytes is too small. */
long long prx_vit_tower_debug_dqkv(prx_clip_vit* h, void* dst, long long max_bytes, prx_stream_t s);
void prx_clip_vit_destroy(prx_clip_vit* h);
int prx_clip_vit_minmax(prx_clip_vit* h, const float* cutouts, int n, float* mm, prx_stream_t s);
int prx_clip_vit_encode(prx_clip_vit* h, const float* cutouts, int n, const float* mm, float* embeds, prx_stream_t s);
int prx_clip_vit_backward_reduce(prx_clip_vit* h, const float* cutouts, const float* mm, const float* d_embeds,
                                 double* acc, prx_stream_t s);
int prx_clip_vit_backward_finish(prx_clip_vit* h, const float* cutouts, const float* mm, const double* acc,
                                 float* g_cutouts, prx_stream_t s);

/* --- CLIP_Base.encode_image for a ModifiedResNet visual tower (RN50, RN101, RN50x4, RN50x16, RN50x64) [UPSTREAM clip/model.py: ModifiedResNet,
 *     Bottleneck, AttentionPool2d].  Same call sequence and min/max contract as the ViT entry points above.
 * weights[]: fp32 device tensors with the eval-mode BatchNorms folded into their convolutions on the host
 *   (pixray_amd/weights.py::fold_clip_resnet_params, from the `visual.*` state dict):
 *   stem conv1 {weight [w/2,3,3,3], bias}, stem conv2 {weight, bias}, stem conv3 {weight, bias};
 *   per Bottleneck: conv1 {weight [planes,in,1,1], bias}, conv2 {weight [planes,planes,3,3], bias}, conv3 {weight
 *   [4*planes,planes,1,1], bias} [, downsample {weight [4*planes,in,1,1], bias}];
 *   attnpool.positional_embedding [(R/32)^2+1, 32w], in_proj {weight [3*32w, 32w] = q|k|v, bias}, c_proj {weight, bias}. */
typedef struct prx_clip_resnet prx_clip_resnet;
typedef struct prx_clip_resnet_config {
    int input_resolution;  /* 224 (RN50, RN101) | 288 (RN50x4) | 384 (RN50x16) | 448 (RN50x64); a multiple of 32 */
    int width;             /* 64 | 80 | 96 | 128; width / 2 (the stem kernels' channel count) one of 8, 16, 32, 40, 48, 64 */
    int layers[4];         /* {3,4,6,3} | {3,4,23,3} | {4,6,10,6} | {6,8,18,8} | {3,15,36,10} */
    int heads;             /* width * 32 / 64: 32 | 40 | 48 | 64 (attention pool over (R/32)^2 + 1 = 50 | 82 | 145 | 197 tokens) */
    int output_dim;        /* 1024 | 512 | 640 | 768 | 1024 */
    int max_batch;         /* capacity in cutouts: create allocates one forward's activations for this many (RN50x64 at 448^2: 572 MiB
                              per cutout with half operands, 1077 MiB with bf16, 1561 MiB in the exact mode); an allocation that fails
                              is an error of the call (rc < 0, prx_last_error names the bytes asked for and the bytes held), nothing stays
                              allocated -- as in every prx_*_create (prx_fft_drawer_create returns null) */
    int precision;         /* PRX_PREC_F16 | PRX_PREC_BF16 | PRX_PREC_F32 */
} prx_clip_resnet_config;
int prx_clip_resnet_create(prx_clip_resnet** out, const prx_clip_resnet_config* cfg, const float* const* weights, int n_weights,
                           prx_stream_t s);
void prx_clip_resnet_destroy(prx_clip_resnet* h);
int prx_clip_resnet_minmax(prx_clip_resnet* h, const float* cutouts, int n, float* mm, prx_stream_t s);
int prx_clip_resnet_encode(prx_clip_resnet* h, const float* cutouts, int n, const float* mm, float* embeds, prx_stream_t s);
int prx_clip_resnet_backward_reduce(prx_clip_resnet* h, const float* cutouts, const float* mm, const float* d_embeds,
                                    double* acc, prx_stream_t s);
int prx_clip_resnet_backward_finish(prx_clip_resnet* h, const float* cutouts, const float* mm, const double* acc,
                                    float* g_cutouts, prx_stream_t s);

/* --- encode_image for an OpenCLIP ConvNeXt visual tower (convnext_base, convnext_base_w, convnext_base_w_320, convnext_large_d,
 *     convnext_large_d_320, convnext_xxlarge) [UPSTREAM timm convnext.py ConvNeXt + open_clip timm_model.py head; neither package is
 *     installed: restated from the published sources, parity unpinned].  Same call sequence and min/max contract as the ResNet entry
 *     points above; CLIP's preprocessing constants.  csrc/convnext.hip.
 * weights[]: fp32 device tensors as pixray_amd/weights.py::fold_clip_convnext_params lays them out from the `visual.*` state dict:
 *   stem {weight [d0, 3*4*4], bias, LayerNorm weight, bias};
 *   per stage i: for i > 0 the downsample {LayerNorm weight [d(i-1)], bias, conv weight [d(i), 4*d(i-1)] with the input column
 *   (dy * 2 + dx) * d(i-1) + c, bias}; then per block: conv_dw {weight [C, 49], bias}, norm {weight, bias}, mlp.fc1 {weight [4C, C],
 *   bias}, mlp.fc2 {weight [C, 4C], bias} with the block's layer scale gamma[C] folded into both (rows of the weight, the bias);
 *   head.norm {weight [d3], bias}; then proj.weight [embed, d3] (proj_mlp == 0) or mlp.fc1 {weight [2*embed, d3], bias},
 *   mlp.fc2.weight [embed, 2*embed] (proj_mlp == 1).  4 + 12 + 8 * sum(depths) + 2 + (1 | 3) tensors.
 * Device memory per cutout of max_batch, beside the packed weights (saved GELU pre-activations [pixels][4C] and stencil outputs
 * [pixels][C] of every block, the fp32 residual stream with its operand twin as two buffers per stage, the backward's gradient
 * streams): convnext_base_w at 256^2: 95 181 104 bytes (90.8 MiB) with half or bf16 operands -- 46.5 MiB of it the pre-activations
 * --, 163 087 760 (155.5 MiB) in the exact mode; convnext_base at 224^2: 69.5 / 119.1 MiB; convnext_base_w_320: 141.8 / 243.0 MiB;
 * convnext_large_d at 256^2: 135.5 / 232.4 MiB; convnext_large_d_320: 211.6 / 363.1 MiB; convnext_xxlarge at 256^2: 288.3 / 500.6 MiB
 * (pixray_amd/weights.py::clip_convnext_activation_bytes restates the allocation list). */
typedef struct prx_clip_convnext prx_clip_convnext;
typedef struct prx_clip_convnext_config {
    int input_resolution;  /* 224 | 256 | 320; a multiple of 32 (the maps are R/4, R/8, R/16, R/32 on a side) */
    int depths[4];         /* {3,3,27,3} | {3,4,30,3}; each >= 1 */
    int dims[4];           /* {128,256,512,1024} | {192,384,768,1536} | {384,768,1536,3072}; multiples of 8 */
    int output_dim;        /* 512 | 640 | 768 | 1024; a multiple of 8 */
    int proj_mlp;          /* 0: linear projection; 1: fc1 (2 * output_dim), GELU, fc2 (the convnext_large_d towers) */
    float ln_eps;          /* 1e-6; convnext_xxlarge: 1e-5 */
    int max_batch;         /* capacity in cutouts: create allocates one forward's activations for this many (figures above); an allocation
                              that fails is an error of the call (rc < 0, prx_last_error names the bytes asked for and the bytes held),
                              nothing stays allocated */
    int precision;         /* PRX_PREC_F16 | PRX_PREC_BF16 | PRX_PREC_F32 */
} prx_clip_convnext_config;
int prx_clip_convnext_create(prx_clip_convnext** out, const prx_clip_convnext_config* cfg, const float* const* weights, int n_weights,
                             prx_stream_t s);
void prx_clip_convnext_destroy(prx_clip_convnext* h);
int prx_clip_convnext_minmax(prx_clip_convnext* h, const float* cutouts, int n, float* mm, prx_stream_t s);
int prx_clip_convnext_encode(prx_clip_convnext* h, const float* cutouts, int n, const float* mm, float* embeds, prx_stream_t s);
int prx_clip_convnext_backward_reduce(prx_clip_convnext* h, const float* cutouts, const float* mm, const float* d_embeds,
                                      double* acc, prx_stream_t s);
int prx_clip_convnext_backward_finish(prx_clip_convnext* h, const float* cutouts, const float* mm, const double* acc,
                                      float* g_cutouts, prx_stream_t s);

/* --- CLIP_Base.encode_text (slip.py:68-70) = openai/CLIP `CLIP.encode_text` [UPSTREAM clip/model.py] on token ids:
 *     token_embedding[tokens] + positional_embedding -> causal transformer -> ln_final -> row at argmax(tokens) (the EOT
 *     token) @ text_projection.  Forward only; the result is NOT normalised (as the reference's, slip.py:70).
 * weights[]: fp32 device tensors in state-dict order: token_embedding.weight [vocab, width], positional_embedding
 *   [context, width], transformer.resblocks.{i}.{ln_1.weight, ln_1.bias, attn.in_proj_weight, attn.in_proj_bias,
 *   attn.out_proj.weight, attn.out_proj.bias, ln_2.weight, ln_2.bias, mlp.c_fc.weight, mlp.c_fc.bias, mlp.c_proj.weight,
 *   mlp.c_proj.bias}, ln_final.{weight,bias}, text_projection [width, output_dim].
 * tokens: int32 device [n, context] as `clip.tokenize` returns them (SOT ... EOT, zero padded). */
typedef struct prx_clip_text prx_clip_text;
typedef struct prx_clip_text_config {
    int vocab_size;       /* 49408 */
    int context_length;   /* 77 */
    int width;            /* 512 (ViT-B/32, B/16), 768 (ViT-L/14); heads = width / 64 */
    int layers;           /* 12 */
    int heads;            /* 8 */
    int output_dim;       /* 512 */
    int max_batch;
} prx_clip_text_config;
int prx_clip_text_create(prx_clip_text** out, const prx_clip_text_config* cfg, const float* const* weights, int n_weights,
                         prx_stream_t s);
/* The same runner for a family of text towers: PRX_TEXT_FAMILY_CLIP is prx_clip_text_create; PRX_TEXT_FAMILY_OPENCLIP has the exact
 * GELU in place of QuickGELU (the OpenCLIP / LAION text transformers; ViT-H-14: width 1024, 16 heads, 24 layers).  weights[] as above. */
#define PRX_TEXT_FAMILY_CLIP 0
#define PRX_TEXT_FAMILY_OPENCLIP 1
typedef struct prx_text_tower_config {
    int vocab_size, context_length, width, layers, heads, output_dim, max_batch;      /* as prx_clip_text_config */
    int family;           /* PRX_TEXT_FAMILY_* */
} prx_text_tower_config;
int prx_text_tower_create(prx_clip_text** out, const prx_text_tower_config* cfg, const float* const* weights, int n_weights,
                          prx_stream_t s);
void prx_clip_text_destroy(prx_clip_text* h);
int prx_clip_text_encode(prx_clip_text* h, const int* tokens, int n, float* embeds, prx_stream_t s);

/* --- Prompt.forward (pixray.py:275-280) fused with its backward.
 * rowloss[i] = sum_j sign(w) * 2*asin(|x^_i - e^_j|/2)^2;  *loss (optional, may be NULL) = |w| * sum(rowloss) / denom, the value
 * Prompt.forward returns, written by the workgroup that finishes last (rows added in a fixed order); `ticket`: one device word
 * that is zero on entry and zero again on exit (needed with `loss`; one per stream that may run this concurrently);
 * grad = d/d input of |w| * mean(max(sign(w) d, stop)) with the mean over `denom` (= global n*m) pairs.
 * D: a multiple of 64, at most 1024 (a row lives in registers, 16 steps of 64).
 * prx_prompt_loss_fwd_bwd_wide: the same call for D up to 2048 (OpenCLIP ViT-bigG-14 embeds into 1280): the same kernel up to 1024, its
 * 32-step instance beyond. */
int prx_prompt_loss_fwd_bwd(const float* input, const float* embed, int n, int m, int D, float weight, float stop,
                            float denom, float* rowloss, float* grad, float* loss, unsigned* ticket, prx_stream_t s);
int prx_prompt_loss_fwd_bwd_wide(const float* input, const float* embed, int n, int m, int D, float weight, float stop,
                                 float denom, float* rowloss, float* grad, float* loss, unsigned* ticket, prx_stream_t s);

/* --- optim.Adam([z], lr) step (pixray.py:539,1484-1485) fused with VqganDrawer.clip_z (vqgan.py:202-204).
 * z/exp_avg/exp_avg_sq/grad: [1,C,hw] fp32; zmin/zmax per channel or NULL; step is 1-based. */
int prx_adam_clamp_step(float* z, float* exp_avg, float* exp_avg_sq, const float* grad, const float* zmin,
                        const float* zmax, int hw, size_t n, float lr, float beta1, float beta2, float eps, int step,
                        prx_stream_t s);

/* same step with the step-dependent scalars read from device memory: hyper = {lr / (1 - beta1^t), sqrt(1 - beta2^t)}.
 * Used when the whole iteration is captured in a hipGraph and replayed (kernel arguments are frozen at capture). */
int prx_adam_clamp_step_dev(float* z, float* exp_avg, float* exp_avg_sq, const float* grad, const float* zmin,
                            const float* zmax, int hw, size_t n, const float* hyper, float beta1, float beta2, float eps,
                            prx_stream_t s);

/* --- the other rules of --optimiser (pixray.py:541-550: optim.AdamW / Adagrad / Adamax, torch_optimizer's DiffGrad), only `lr`
 * given as there, each fused with VqganDrawer.clip_z (vqgan.py:202-204); the step-dependent scalars are read from device memory
 * like prx_adam_clamp_step_dev's.  p / grad / state tensors: n fp32 elements.  zmin / zmax: per channel, both or both NULL; with
 * them p is seen as [rows, C, hw] (n a multiple of C * hw), without them C and hw are ignored.  State tensors and hyper[0..2]:
 *   PRX_OPT_ADAMW    s1 exp_avg, s2 exp_avg_sq, s3 NULL        {lr / (1 - beta1^t), sqrt(1 - beta2^t), 1 - lr * weight_decay}
 *   PRX_OPT_ADAGRAD  s1 sum, s2 NULL, s3 NULL (betas unused)   {lr}
 *   PRX_OPT_ADAMAX   s1 exp_avg, s2 exp_inf, s3 NULL           {lr / (1 - beta1^t)}
 *   PRX_OPT_DIFFGRAD s1 exp_avg, s2 exp_avg_sq, s3 prev. grad  {lr * sqrt(1 - beta2^t) / (1 - beta1^t)}
 * hyper holds 4 floats.  The betas are doubles so that 1 - beta is formed before it is rounded to fp32. */
#define PRX_OPT_ADAMW 0
#define PRX_OPT_ADAGRAD 1
#define PRX_OPT_ADAMAX 2
#define PRX_OPT_DIFFGRAD 3
int prx_optim_step_dev(int rule, float* p, float* s1, float* s2, float* s3, const float* grad, const float* zmin,
                       const float* zmax, int C, int hw, size_t n, const float* hyper, double beta1, double beta2, float eps,
                       prx_stream_t s);

/* --- torch_optimizer's AdamP([z], lr) (pixray.py:549-550; delta as given, weight decay 0, nesterov off) fused with clip_z: two
 * launches, no atomics (pass 1: moments + per-workgroup partial dot products into `scratch`; pass 2: every workgroup adds the
 * partials in the same order, takes the projection decision and applies update and clamp).  rows >= 1: the tensor's shape[0], the
 * test runs on the [rows, n / rows] view, then on [1, n]; rows == 0: a 1-D tensor, never projected.  rows <= 4096.
 * hyper = {lr / (1 - beta1^t), sqrt(1 - beta2^t)} (4 floats); scratch: prx_optim_adamp_scratch_floats(rows, n) floats, 16-byte
 * aligned, `scratch_floats` its size; bounds as for prx_optim_step_dev. */
size_t prx_optim_adamp_scratch_floats(int rows, size_t n);
int prx_optim_adamp_step_dev(float* p, float* exp_avg, float* exp_avg_sq, const float* grad, const float* zmin,
                             const float* zmax, int rows, int C, int hw, size_t n, const float* hyper, float* scratch,
                             size_t scratch_floats, double beta1, double beta2, float eps, float delta, prx_stream_t s);

int prx_k_vq_nearest(const float* z, long long tok_stride, long long ch_stride, const float* codebook,
                     const float* cnorm, int P, int NC, int D, float* pmin, int* pidx, int* idx_out, float* zq,
                     prx_stream_t s);
int prx_k_sqnorm_rows(const float* w, float* out, int rows, int D, prx_stream_t s);

/* the dispatcher's saving form in bf16 at head dim 64: any sequence length T >= 1; `out` and `lse` (fp32 [N*heads*T]) are kept for the
 * backward.  Two kernel
 * families: workgroups per (image, head) with a wave per 32 tokens for T <= 640 (ViT-B/16 197 tokens, ViT-L/14 257, ViT-L/14@336px 577,
 * the ModifiedResNet attention pools 50 ... 197), and one wave per 64-token tile with an online softmax for every larger T.
 * prx_mha_route chooses the family of the following general-T calls of the process: -1 that rule (PRX_MHA_TILES=1 in the environment:
 * tiles everywhere), 0 the workgroup family wherever it is able (T <= 640), 1 the tile kernels; it returns the previous setting.
 * Both families are atomic-free and bit-reproducible. */
int prx_mha_route(int route);
/* What the dispatcher does with a problem (host only, nothing is launched; the same routing function the launches go through):
 * precision a PRX_PREC_* value, head_dim as the operands carry it, `recompute` 1 for the recomputing form, `route` as for
 * prx_mha_route (it is an argument here; the process setting is neither read nor changed).  Fills *family with 1 the wave-per-head
 * recomputing kernels, 2 the workgroup family, 3 the tile kernels, 4 the exact-f32 kernels; *head_cols with the operand columns per
 * head (64 | 96 | 128); *saves_out with whether the caller keeps `out` + `lse` for the backward.  A problem without a kernel returns
 * nonzero with *family 0 and the refusal in prx_last_error. */
int prx_mha_describe(int precision, int head_dim, int T, int causal, int recompute, int route, int* family, int* head_cols,
                     int* saves_out);
int prx_k_mha_fwd_gen(const void* qkv, void* out, float* lse, int N, int T, int C, int heads, prx_stream_t s);
int prx_k_mha_bwd_gen(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int N, int T, int C,
                      int heads, prx_stream_t s);

/* the dispatcher's fp32 view: the exact-f32 attention of the PRX_PREC_F32 mode (fp32 qkv / out / dout / dqkv, any T, head dim 64) */
int prx_k_mha_fwd_f32(const float* qkv, float* out, float* lse, int N, int T, int C, int heads, prx_stream_t s);
int prx_k_mha_bwd_f32(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, int N, int T, int C,
                      int heads, prx_stream_t s);

/* tuning override of the tile / split-K heuristic of one context: bm,bn a 4-wave tile (128x128, 128x64, 64x64), the 8-phase 256x256
 * or a fit tile (csrc/gemmfit.hip: 256x128, 160x256, ...; the three shapes both families have mean the 4-wave kernel unless (-12,_,1));
 * (0,0,0) = heuristic.  Negative bm selects a switch: (-1,_,v) XCD-aware tile order 0 off / 1 on / 2 narrow row-major problems /
 * 3 every tiled launch; (-2,_,n) LDS pipeline depth (0 = heuristic); (-3,_,v) 1 = direct-to-LDS v2 kernel (default), 0 = register-staged
 * v1; (-5,_,v) scalar-tap conv gather; (-6,_,n) 256x256 8-phase tiles from n tiles on (0 = never); (-7,_,v) fit tiles; (-8,_,bits)
 * fit kernel switches (bit 0 staggered wave groups); (-9,_,v) fit tiles for the implicit convolutions too; (-12,_,v) a forced
 * 128x128 / 128x64 / 64x64 tile means the fit kernel of that shape; (-13,_,i) bisection aid: only the i-th fit convolution since
 * this call gets its fit tile (-1: all, counted; -2: off); (-14,_,n) row-streaming kernels from n output elements on (0 = 24 Mi). */
void prx_gemm_tile_override(prx_gemm_ctx* c, int bm, int bn, int splits);
/* the same per problem shape (tools/gemm_rules.py): mode = a_mode + 2*up + 4*a_is_f32; splits 0 = heuristic; bm = 0 drops
 * the rule, M = 0 drops all rules */
void prx_gemm_tile_rule(prx_gemm_ctx* c, int M, int N, int K, int mode, int bm, int bn, int splits);

/* what the launch planner does with a row-major 16-bit C[M,N] = A[M,K] * Bt[N,K]^T (no launch, no device needed): returns the number of
 * leading rows it gives to the 256 x 256 8-phase kernel -- M (all), 0 (none: 4-wave kernels), or a multiple of 256 in between
 * (whole rounds of 256 tiles on the 8-phase kernel, the remaining rows on the 4-wave kernels).  c may be NULL (default tuning); a forced
 * tile in c, or a tile rule of c for that shape, gives 0: the launch then follows the override (= out[4] of prx_gemm_plan below). */
int prx_gemm_plan_rows_8phase(prx_gemm_ctx* c, int M, int N, int K);
/* the launch plan of the product prx_k_gemm(g, ws, ws_bytes, ...) would run with context c (NULL: default tuning; g->ctx is not read)
 * on a device of n_cu compute units (0: 256), a 16-byte-aligned workspace of ws_bytes assumed; no launch, no device needed.  Returns
 * 0 or prx_k_gemm's validation error.  out[9]: the kernel family of the first launch (0 register-staged 4-wave, 1 direct-to-LDS
 * 4-wave, 2 exact-f32 4-wave, 3 fit, 4 8-phase, 5 row-streaming, 6 row-streaming 3x3 convolution), its bm, bn, split-K count;
 * out[4] the 8-phase row split (as prx_gemm_plan_rows_8phase); out[5..8] the same four for the second launch that plans the rows
 * after the split on their own (family -1: no second launch).  bn of the row-streaming kernels is their slab width, 80 for the
 * convolutions (the convention of the timing dump). */
int prx_gemm_plan(prx_gemm_ctx* c, const prx_gemm_args* g, size_t ws_bytes, int n_cu, int* out);

/* per-launch GEMM timing (HIP events on the launch stream) for bench.py */
void prx_profile_gemm_enable(prx_gemm_ctx* c, int on);
int prx_profile_gemm_collect(prx_gemm_ctx* c, double* total_ms, double* total_flop, long long* launches);

/* the engine context owned by a runner handle (valid for the handle's lifetime; do not destroy) */
prx_gemm_ctx* prx_vqgan_gemm_ctx(prx_vqgan* h);
prx_gemm_ctx* prx_clip_vit_gemm_ctx(prx_clip_vit* h);
prx_gemm_ctx* prx_clip_resnet_gemm_ctx(prx_clip_resnet* h);
prx_gemm_ctx* prx_clip_convnext_gemm_ctx(prx_clip_convnext* h);
prx_gemm_ctx* prx_vgg16_gemm_ctx(prx_vgg16* h);

/* ---- the exchange step of the cutout-sharded iteration ------------------------------------------------
 * The reference has no distributed code; what this replaces is the seam in `train()` between
 * `loss.backward()` and `opt.step()` (pixray.py:1482-1485) where a data-parallel port would all-reduce the gradient.
 * prx_allreduce_grad is a ONE-SHOT DIRECT-WRITE all-reduce (SUM, fp32, in place) over IPC-mapped peer windows: every rank
 * writes its vector straight into each peer's window over xGMI, raises a flag, waits for the peers' flags in its own window
 * and sums the slots in rank order -- bit-identical on every rank, one kernel, no ring (csrc/comm.hip).
 *   prx_comm_create    allocates this rank's window (slots of max_bytes for 2 calls in flight x world ranks)
 *   prx_comm_export    the window's IPC handle, prx_comm_handle_bytes() bytes, to be exchanged by the host side
 *   prx_comm_connect   maps the peers' windows from `world` handles in rank order (own entry ignored)
 *   prx_allreduce_grad n floats, n % 4 == 0, 16-byte aligned, n * 4 <= max_bytes; asynchronous on `stream`
 *   prx_comm_status    0, or 1 + r when a wait for rank r's data timed out (synchronises) */
typedef struct prx_comm prx_comm;
int prx_comm_handle_bytes(void);
int prx_comm_create(prx_comm** out, int rank, int world, size_t max_bytes);
int prx_comm_export(prx_comm* c, void* handle_out);
int prx_comm_connect(prx_comm* c, const void* handles);
int prx_allreduce_grad(prx_comm* c, float* grad, size_t n, prx_stream_t stream);
/* the same exchange for the two scalar-sized collectives of the sharded iteration, so that a C-ABI caller needs nothing else:
 * PRX_COMM_MAX_F32 for the {-min, max} pair of the batch-global renormalisation (slip.py:21-36), PRX_COMM_SUM_F64 for its four
 * backward sums.  n_words counts 4-byte words (a double = 2), a multiple of 4; data 16-byte aligned.  A wait that times out
 * poisons the result with NaN (never a plausible partial sum) and is reported by prx_comm_status.  The kernel's <= 64 blocks
 * must be co-resident (they are on an otherwise idle stream; see csrc/comm.hip). */
#define PRX_COMM_SUM_F32 0
#define PRX_COMM_MAX_F32 1
#define PRX_COMM_SUM_F64 2
int prx_allreduce(prx_comm* c, void* data, size_t n_words, int op, prx_stream_t stream);
int prx_comm_status(prx_comm* c);
void prx_comm_destroy(prx_comm* c);

/* --- built-in custom losses and filters (pixray Losses/, filters/): csrc/plugin_losses.hip, plugin_filters.hip.
 * fp32 tensors, contiguous NCHW.  Every loss scalar is reduced in a fixed order: `partials` is a scratch of
 * 4 * 1024 doubles, `ticket` one device word that is zero on entry and zero again on exit (as prx_prompt_loss_fwd_bwd's).
 * `gout` / `gloss` are the incoming gradients of the loss scalars, read on the device.
 * saturation: x [n][3][hw]; stats (4 doubles) saved for the backward.  loss = -(std_rggb + 0.3 mean_rggb) * w / 10 */
int prx_saturation_fwd(const float* x, int n, int hw, float weight, double* partials, double* stats, float* loss, unsigned* ticket,
                       prx_stream_t s);
int prx_saturation_bwd(const float* x, int n, int hw, float weight, const double* stats, const float* gout, float* grad, prx_stream_t s);
/* symmetry: MSE(x, flip_W(x)) * w over planes x h x w; grad = d loss / dx */
int prx_symmetry_fwd_bwd(const float* x, int planes, int h, int w, float weight, double* partials, float* grad, float* loss,
                         unsigned* ticket, prx_stream_t s);
/* edge: x [planes = 3k][h][w] against colour (r, g, b): margin bands (pixels) weighted by inv_* = 1 / band elements (0 = band
 * off), inv_all = global weight / all elements; everything times edge_weight */
int prx_edge_fwd_bwd(const float* x, int planes, int h, int w, float r, float g, float b, int left, int right, int upper, int lower,
                     float inv_l, float inv_r, float inv_u, float inv_d, float inv_all, float edge_weight, double* partials, float* grad,
                     float* loss, unsigned* ticket, prx_stream_t s);
/* edge with a target image and / or a mask: as prx_edge_fwd_bwd, but the per-element target is target [3][h][w] (null: the flat
 * colour), and with mask [h][w] (null: none) the bands are ignored and every element where mask <= 0 weighs inv_mask */
int prx_edge_target_fwd_bwd(const float* x, int planes, int h, int w, const float* target, float r, float g, float b, const float* mask,
                            int left, int right, int upper, int lower, float inv_l, float inv_r, float inv_u, float inv_d, float inv_mask,
                            float inv_all, float edge_weight, double* partials, float* grad, float* loss, unsigned* ticket, prx_stream_t s);
/* gaussian: x [planes = 3k][h][w] against colour (r, g, b), weighed |1 - gy[y] gx[c]|: loss = scale * sum a |d|, grad = scale a sign(d) */
int prx_gaussian_fwd_bwd(const float* x, int planes, int h, int w, const float* gy, const float* gx, float r, float g, float b, float scale,
                         double* partials, float* grad, float* loss, unsigned* ticket, prx_stream_t s);
/* aesthetic: embeds [n][d], head w [d] + bias on the L2-normalised rows (eps 1e-12); loss = 0.02 / n * sum (rating - target)^2 */
int prx_aesthetic_fwd_bwd(const float* embeds, int n, int d, const float* w, float bias, float target, double* partials, float* grad,
                          float* loss, unsigned* ticket, prx_stream_t s);
/* palette: x [n][3][hw], palette [np <= 256][3]; loss = scale * sum over pixels of |pixel - nearest entry| */
int prx_palette_fwd_bwd(const float* x, int n, int hw, const float* palette, int np, float scale, double* partials, float* grad,
                        float* loss, unsigned* ticket, prx_stream_t s);
/* smoothness: x [n][3][h][w] seen as [n*h][w][3]; type 0 default, 1 clipped, 2 log; edge_order 1 | 2; tfac [n*h*w] saved */
int prx_smoothness_fwd(const float* x, int n, int h, int w, int type, int edge_order, float spacing, float weight, double* partials,
                       float* tfac, float* loss, unsigned* ticket, prx_stream_t s);
int prx_smoothness_bwd(const float* tfac, const float* x, int n, int h, int w, int edge_order, float spacing, float weight,
                       const float* gout, float* grad, prx_stream_t s);
/* depthwise valid k x k blur (k <= 33): y [planes][h-k+1][w-k+1]; the backward takes the input's h, w */
int prx_blur_fwd(const float* x, int planes, int h, int w, const float* taps, int k, float* y, prx_stream_t s);
int prx_blur_bwd(const float* gy, int planes, int h, int w, const float* taps, int k, float* gx, prx_stream_t s);
/* lookup filter: x [b][c = 3 | 4][hw] -> out (straight-through nearest palette colour; alpha copied), lgrad = d loss / dx,
 * loss = (beta + 1) * mean((q - x)^2) over the colour channels */
int prx_color_lookup_fwd(const float* x, int b, int c, int hw, const float* palette, int np, float beta, double* partials, float* out,
                         float* lgrad, float* loss, unsigned* ticket, prx_stream_t s);
/* tiler / wallpaper filter: shifts = device {rand_h, rand_w}; em = --wallpaper_edge_match (0 off, else >= 2).
 * out [planes][2h][w] in shift mode, else [planes][h - 2 th][w - 2 tw] with the edge-match trims; loss = the seam term */
#define PRX_WALL_BOTH 0
#define PRX_WALL_HORIZONTAL 1
#define PRX_WALL_VERTICAL 2
#define PRX_WALL_SHIFT 3
int prx_wallpaper_fwd(const float* x, int planes, int h, int w, int mode, int em, const int* shifts, double* partials, float* out,
                      float* loss, unsigned* ticket, prx_stream_t s);
int prx_wallpaper_bwd(const float* x, const float* gout, int planes, int h, int w, int mode, int em, const int* shifts,
                      const float* gloss, float* grad, prx_stream_t s);

/* --- pixel drawer (pixray pixeldrawer.py): csrc/pixel_raster.hip.  A w x h canvas of filled polygons, composited in index order
 * ("over", nonzero winding, 2 x 2 jittered samples per pixel; conventions in INTEGRATION.md).
 * verts [n][PRX_PIXEL_MAX_VERTS][2] (padded), nverts [n], colors [n][4] RGBA.  The canvas is cut into PRX_PIXEL_TILE-pixel
 * square tiles, row-major, ceil(w / 16) per row: tile t lists the shapes that may cover it, ascending, in
 * tile_shapes[tile_start[t] .. tile_start[t + 1]).  seed = one device word (the iteration).
 * forward: out [4][h][w] (RGBA planes); ids [h][w][4] int32 = the topmost shape per sample (-1: none), or NULL.
 * backward: gout [4][h][w] -> grad [n][4] = d loss / d colors; partials = scratch of 4 doubles per tile_shapes entry;
 * shape k's entries (indices into tile_shapes, in tile order) are shape_entries[shape_start[k] .. shape_start[k + 1]).
 * sample offsets: uv [h][w][4][2] = the jitter (u, v) of sample 2 sy + sx of every pixel for the seed in `seed`. */
#define PRX_PIXEL_TILE 16
#define PRX_PIXEL_MAX_VERTS 8
int prx_pixel_raster_fwd(const float* verts, const int* nverts, const float* colors, const int* tile_start, const int* tile_shapes,
                         int w, int h, const int* seed, float* out, int* ids, prx_stream_t s);
int prx_pixel_raster_bwd(const float* verts, const int* nverts, const float* colors, const int* tile_start, const int* tile_shapes,
                         int w, int h, const int* seed, const float* gout, double* partials, const int* shape_start,
                         const int* shape_entries, int n_shapes, float* grad, prx_stream_t s);
int prx_pixel_sample_offsets(int w, int h, const int* seed, float* uv, prx_stream_t s);

/* --- stroke drawers (pixray linedrawer.py `line_sketch`, clipdrawer.py `clipdraw`): csrc/stroke_raster.hip.  A w x h canvas of
 * open paths of cubic Bezier segments, stroked with a pre-filtered coverage clamp(width - d + 0.5, 0, 1) (width = the
 * half-width, d = the distance to the centre line), composited in index order over an optional paper colour ("over", 2 x 2
 * jittered samples per pixel, the pixel drawer's jitter; conventions in INTEGRATION.md).
 * points [P][2] (pixels); path k owns points[path_start[k] .. path_start[k + 1]), 1 + 3 S of them for S segments, at most
 * max_points (<= PRX_STROKE_MAX_POINTS); widths [n], colors [n][4] RGBA; paper [4] RGBA or NULL.  seed = one device word.
 * Workspaces, sized from n, max_points and the canvas alone (tiles = ceil(w / 16) * ceil(h / 16)): boxes [n][4] fp32,
 * tile_count [tiles] int32, tile_paths [tiles][n] int32; the backward's partials [tiles][n][2 max_points + 5] fp64 and
 * paper_partials [tiles][4] fp64.  Both calls rebuild boxes and tile lists from the points on the device.
 * forward: out [h][w][4] RGBA.  backward: gout [h][w][4] -> grad_points [P][2], grad_widths [n], grad_colors [n][4], and
 * grad_paper [4] when not NULL (then paper and paper_partials are required).  Fixed summation order: a run repeats bit for bit.
 * sample offsets: uv [h][w][4][2], as prx_pixel_sample_offsets. */
#define PRX_STROKE_TILE 16
#define PRX_STROKE_MAX_POINTS 193
int prx_stroke_raster_fwd(const float* points, const int* path_start, int n_paths, int max_points, const float* widths,
                          const float* colors, const float* paper, int w, int h, const int* seed, float* boxes, int* tile_count,
                          int* tile_paths, float* out, prx_stream_t s);
int prx_stroke_raster_bwd(const float* points, const int* path_start, int n_paths, int max_points, const float* widths,
                          const float* colors, const float* paper, int w, int h, const int* seed, const float* gout, float* boxes,
                          int* tile_count, int* tile_paths, double* partials, double* paper_partials, float* grad_points,
                          float* grad_widths, float* grad_colors, float* grad_paper, prx_stream_t s);
int prx_stroke_sample_offsets(int w, int h, const int* seed, float* uv, prx_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* PRX_H_ */
