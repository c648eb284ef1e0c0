// C-ABI kernel-level entry points (tests/ check every kernel alone through these).
// The first block pins every kernel to its bf16 / fp32-stream build (the defaults of norms.h, elementwise.h, attention.h).  The
// `_op` siblings at the end forward EVERY argument of the internal functions -- the 16-bit format (h16), the lean-layout stream
// flags (s16), add_every, the 16-bit-only outputs, gscale, prec -- so that tests/test_kernels_half_gpu.py can hold the
// instantiations the product's default (IEEE half, lean layout) launches to a float64 reference one kernel at a time.  Test
// surface only: the product's Python never calls them.
#include "common.h"
#include "norms.h"
#include "elementwise.h"
#include "attention.h"
#include "resnet.h"
#include "convnext.h"
#include "cutouts.h"
#include "vgg.h"
#include "vit.h"
#include "clip_text.h"
#include "prompt_vq.h"
#include "vqgan.h"
#include "vqgan_enc.h"
#include "weight_pack.h"
#include "fft_drawer.h"
#include "../../include/prx.h"

#define S_(x) ((hipStream_t)(x))
#define B_(x) ((bf16_t*)(x))
#define CB_(x) ((const bf16_t*)(x))

extern "C" {

int prx_k_groupnorm_fwd(const float* x, const float* gamma, const float* beta, double* stats, void* out_bf16,
                        float* out_f32, int NB, int P, int C, int swish, float eps, prx_stream_t s) {
    return prx_groupnorm_fwd(x, gamma, beta, stats, B_(out_bf16), out_f32, NB, P, C, swish, eps, S_(s));
}
int prx_k_groupnorm_bwd(const float* g, const float* x, const float* gamma, const float* beta, const double* fstats,
                        double* bstats, const float* add, float* dx, int NB, int P, int C, int swish, float eps,
                        prx_stream_t s) {
    return prx_groupnorm_bwd(g, x, gamma, beta, fstats, bstats, add, dx, nullptr, NB, P, C, swish, eps, S_(s));
}
int prx_k_layernorm_fwd(const float* x, long long ldx, const float* gamma, const float* beta, void* out_bf16,
                        float* out_f32, float* mean, float* rstd, int rows, int C, float eps, prx_stream_t s) {
    return prx_layernorm_fwd(x, ldx, gamma, beta, B_(out_bf16), out_f32, mean, rstd, rows, C, eps, S_(s));
}
int prx_k_layernorm_bwd(const float* g, long long ldg, const float* x, long long ldx, const float* gamma,
                        const float* mean, const float* rstd, const float* add, long long ldadd, float* dx,
                        long long lddx, int rows, int C, prx_stream_t s) {
    return prx_layernorm_bwd(g, ldg, x, ldx, gamma, mean, rstd, add, ldadd, dx, lddx, nullptr, 0, rows, C, S_(s));
}
int prx_k_transpose_bf16(const void* in, int ldin, void* out, int ldout, int R, int C, prx_stream_t s) {
    return prx_transpose_op(in, ldin, out, ldout, R, C, PRX_PREC_BF16, S_(s));
}
int prx_k_softmax_rows(const float* S, int lds_, float scale, void* P, int ldp, void* PT, int ldpt, int rows, int cols,
                       prx_stream_t s) {
    return prx_softmax_rows(S, lds_, scale, P, ldp, PT, ldpt, rows, cols, PRX_PREC_BF16, S_(s));
}
int prx_k_softmax_rows_bwd(const void* P, int ldp, const float* dP, int lddp, float scale, void* dS, int ldds,
                           void* dST, int lddst, int rows, int cols, prx_stream_t s) {
    return prx_softmax_rows_bwd(P, ldp, dP, lddp, scale, dS, ldds, dST, lddst, rows, cols, PRX_PREC_BF16, S_(s));
}
int prx_k_upsample2x_bwd(const float* hi, float* low, int NB, int Hl, int Wl, int C, prx_stream_t s) {
    return prx_upsample2x_bwd(hi, low, nullptr, NB, Hl, Wl, C, S_(s));
}
int prx_k_nchw_to_nhwc(const float* in, float* out_f32, void* out_bf16, int NB, int C, int HW, int Cpad,
                       prx_stream_t s) {
    return prx_nchw_to_nhwc(in, out_f32, B_(out_bf16), NB, C, HW, Cpad, S_(s));
}
int prx_k_nhwc_to_nchw(const float* in, int ldc, float* out, int NB, int C, int HW, prx_stream_t s) {
    return prx_nhwc_to_nchw(in, ldc, out, NB, C, HW, S_(s));
}
int prx_k_image_head_fwd(const float* x, int ldc, float* img, int NB, int C, int HW, prx_stream_t s) {
    return prx_image_head_fwd(x, ldc, img, NB, C, HW, S_(s));
}
int prx_k_image_head_bwd(const float* x, int ldc, const float* gimg, float* dx, void* dx_bf16, int ldo, int NB, int C,
                         int HW, prx_stream_t s) {
    return prx_image_head_bwd(x, ldc, gimg, dx, B_(dx_bf16), ldo, NB, C, HW, S_(s));
}
// ---- attention: every prx_k_mha_* call is a view of the one dispatcher (attention.h): it fills the descriptor and calls it ----------
static MhaDesc mha_desc(int N, int T, int C, int heads, int hd, int prec, int recompute = 0, int causal = 0) {
    MhaDesc d;
    d.N = N; d.T = T; d.C = C; d.heads = heads; d.hd = hd; d.prec = prec; d.recompute = recompute; d.causal = causal;
    return d;
}
static int prec16(int h16) { return h16 ? PRX_PREC_F16 : PRX_PREC_BF16; }
int prx_k_mha_fwd(const void* qkv, void* out, int N, int T, int C, int heads, prx_stream_t s) {
    return prx_mha_fwd(mha_desc(N, T, C, heads, 64, PRX_PREC_BF16, 1), qkv, out, nullptr, S_(s));
}
int prx_k_mha_bwd(const void* qkv, const void* dout, void* dqkv, int N, int T, int C, int heads, prx_stream_t s) {
    return prx_mha_bwd(mha_desc(N, T, C, heads, 64, PRX_PREC_BF16, 1), qkv, nullptr, dout, nullptr, dqkv, S_(s));
}

int prx_k_mha_fwd_gen(const void* qkv, void* out, float* lse, int N, int T, int C, int heads, prx_stream_t s) {
    return prx_mha_fwd(mha_desc(N, T, C, heads, 64, PRX_PREC_BF16), qkv, out, lse, S_(s));
}
int prx_k_mha_bwd_gen(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int N, int T, int C,
                      int heads, prx_stream_t s) {
    return prx_mha_bwd(mha_desc(N, T, C, heads, 64, PRX_PREC_BF16), qkv, out, dout, lse, dqkv, S_(s));
}

int prx_k_mha_fwd_f32(const float* qkv, float* out, float* lse, int N, int T, int C, int heads, prx_stream_t s) {
    return prx_mha_fwd(mha_desc(N, T, C, heads, 64, PRX_PREC_F32), qkv, out, lse, S_(s));
}
int prx_k_mha_bwd_f32(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, int N, int T, int C,
                      int heads, prx_stream_t s) {
    return prx_mha_bwd(mha_desc(N, T, C, heads, 64, PRX_PREC_F32), qkv, out, dout, lse, dqkv, S_(s));
}

// ---- OpenCLIP ConvNeXt runner kernels (convnext.hip; tests/test_convnext_gpu.py) ------------------------------------------------
int prx_k_cnx_pack_dw(const float* w, void* pack, int C, int prec, prx_stream_t s) { return prx_cnx_pack_dw(w, pack, C, prec, S_(s)); }
int prx_k_cnx_dwconv(const void* x, const void* pack, const float* bias, const float* add, void* out_op, float* out_f32, int N, int H,
                     int W, int C, int flip, int prec, prx_stream_t s) {
    return prx_cnx_dwconv(x, pack, bias, add, out_op, out_f32, N, H, W, C, flip, prec, S_(s));
}
int prx_k_cnx_space_to_depth(const void* in, void* out, int N, int H, int W, int C, int prec, prx_stream_t s) {
    return prx_cnx_space_to_depth(in, out, N, H, W, C, prec, S_(s));
}
int prx_k_cnx_depth_to_space(const void* in, void* out, int N, int H, int W, int C, int prec, prx_stream_t s) {
    return prx_cnx_depth_to_space(in, out, N, H, W, C, prec, S_(s));
}
int prx_k_cnx_avgpool_fwd(const void* x, float* out, int N, int HW, int C, int prec, prx_stream_t s) {
    return prx_cnx_avgpool_fwd(x, out, N, HW, C, prec, S_(s));
}
int prx_k_cnx_avgpool_bwd(const float* g, float* dx_f32, void* dx_op, int N, int HW, int C, int prec, prx_stream_t s) {
    return prx_cnx_avgpool_bwd(g, dx_f32, dx_op, N, HW, C, prec, S_(s));
}
int prx_k_cnx_layernorm_fwd(const void* x, int x_f32, const float* gamma, const float* beta, void* out_op, float* out_f32, float* mean,
                            float* rstd, int rows, int C, float eps, int group, int prec, prx_stream_t s) {
    return prx_cnx_layernorm_fwd(x, x_f32, gamma, beta, out_op, out_f32, mean, rstd, rows, C, eps, group, prec, S_(s));
}
int prx_k_cnx_layernorm_bwd(const float* g, const void* x, int x_f32, const float* gamma, const float* mean, const float* rstd,
                            void* dx_op, float* dx_f32, int rows, int C, int group, int prec, prx_stream_t s) {
    return prx_cnx_layernorm_bwd(g, x, x_f32, gamma, mean, rstd, dx_op, dx_f32, rows, C, group, prec, S_(s));
}

// ---- every argument forwarded: the half-mode / lean-layout variants (tests/test_kernels_half_gpu.py) ----------------------------
int prx_k_groupnorm_fwd_op(const void* x, const float* gamma, const float* beta, double* stats, void* out16, float* out_f32,
                           int NB, int P, int C, int swish, float eps, int zero_stats, int stats_ready, int h16, int s16,
                           prx_stream_t s) {
    return prx_groupnorm_fwd(x, gamma, beta, stats, B_(out16), out_f32, NB, P, C, swish, eps, S_(s), zero_stats, stats_ready, h16, s16);
}
int prx_k_groupnorm_bwd_op(const void* g, const void* x, const float* gamma, const float* beta, const double* fstats,
                           double* bstats, const void* add, float* dx, void* dx16, int NB, int P, int C, int swish, float eps,
                           int zero_stats, int stats_ready, int h16, int s16, prx_stream_t s) {
    return prx_groupnorm_bwd(g, x, gamma, beta, fstats, bstats, add, dx, B_(dx16), NB, P, C, swish, eps, S_(s), zero_stats,
                             stats_ready, h16, s16);
}
int prx_k_layernorm_fwd_op(const void* x, long long ldx, const float* gamma, const float* beta, void* out16, float* out_f32,
                           float* mean, float* rstd, int rows, int C, float eps, int h16, int s16, prx_stream_t s) {
    return prx_layernorm_fwd(x, ldx, gamma, beta, B_(out16), out_f32, mean, rstd, rows, C, eps, S_(s), h16, s16);
}
int prx_k_layernorm_bwd_op(const void* g, long long ldg, const void* x, long long ldx, const float* gamma, const float* mean,
                           const float* rstd, const void* add, long long ldadd, float* dx, long long lddx, void* dx16,
                           long long lddxb, int rows, int C, int h16, int add_every, int s16, prx_stream_t s) {
    return prx_layernorm_bwd(g, ldg, x, ldx, gamma, mean, rstd, add, ldadd, dx, lddx, B_(dx16), lddxb, rows, C, S_(s), h16,
                             add_every, s16);
}
int prx_k_mha_fwd_op(const void* qkv, void* out, int N, int T, int C, int heads, int h16, prx_stream_t s) {
    return prx_mha_fwd(mha_desc(N, T, C, heads, 64, prec16(h16), 1), qkv, out, nullptr, S_(s));
}
int prx_k_mha_bwd_op(const void* qkv, const void* dout, void* dqkv, int N, int T, int C, int heads, int h16, prx_stream_t s) {
    return prx_mha_bwd(mha_desc(N, T, C, heads, 64, prec16(h16), 1), qkv, nullptr, dout, nullptr, dqkv, S_(s));
}
int prx_k_mha_fwd_gen_op(const void* qkv, void* out, float* lse, int N, int T, int C, int heads, int h16, prx_stream_t s) {
    return prx_mha_fwd(mha_desc(N, T, C, heads, 64, prec16(h16)), qkv, out, lse, S_(s));
}
int prx_k_mha_bwd_gen_op(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int N, int T, int C,
                         int heads, int h16, prx_stream_t s) {
    return prx_mha_bwd(mha_desc(N, T, C, heads, 64, prec16(h16)), qkv, out, dout, lse, dqkv, S_(s));
}
// columns per head as the argument: 64 is head dim 64, 96 is head dim 80 zero-padded
int prx_k_mha_fwd_hd_op(const void* qkv, void* out, float* lse, int N, int T, int C, int heads, int h16, int head_cols, prx_stream_t s) {
    PRX_REQUIRE(head_cols == 64 || head_cols == 96, "mha_fwd_hd: %d columns per head (64 | 96)", head_cols);
    return prx_mha_fwd(mha_desc(N, T, C, heads, head_cols == 64 ? 64 : 80, prec16(h16)), qkv, out, lse, S_(s));
}
int prx_k_mha_bwd_hd_op(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int N, int T, int C,
                        int heads, int h16, int head_cols, prx_stream_t s) {
    PRX_REQUIRE(head_cols == 64 || head_cols == 96, "mha_bwd_hd: %d columns per head (64 | 96)", head_cols);
    return prx_mha_bwd(mha_desc(N, T, C, heads, head_cols == 64 ? 64 : 80, prec16(h16)), qkv, out, dout, lse, dqkv, S_(s));
}
// the head dim as the argument.  The dispatcher derives the columns per head from it and holds C against them, so `head_cols`
// (what C / heads has to be) adds nothing and is not read
int prx_k_mha_fwd_hdim_op(const void* qkv, void* out, float* lse, int N, int T, int C, int heads, int h16, int head_cols, int head_dim,
                          prx_stream_t s) {
    PRX_REQUIRE(head_dim >= 64, "mha_fwd_hdim: head dim %d at %d columns per head (the kernels take head dims >= 64)", head_dim, head_cols);
    return prx_mha_fwd(mha_desc(N, T, C, heads, head_dim, prec16(h16)), qkv, out, lse, S_(s));
}
int prx_k_mha_bwd_hdim_op(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int N, int T, int C,
                          int heads, int h16, int head_cols, int head_dim, prx_stream_t s) {
    PRX_REQUIRE(head_dim >= 64, "mha_bwd_hdim: head dim %d at %d columns per head (the kernels take head dims >= 64)", head_dim, head_cols);
    return prx_mha_bwd(mha_desc(N, T, C, heads, head_dim, prec16(h16)), qkv, out, dout, lse, dqkv, S_(s));
}
int prx_k_layernorm_fwd_rag_op(const void* x, long long ldx, const float* gamma, const float* beta, void* out16, float* out_f32,
                               float* mean, float* rstd, int rows, int C, float eps, int h16, int s16, prx_stream_t s) {
    return prx_layernorm_fwd(x, ldx, gamma, beta, B_(out16), out_f32, mean, rstd, rows, C, eps, S_(s), h16, s16, 1);
}
int prx_k_layernorm_bwd_rag_op(const void* g, long long ldg, const void* x, long long ldx, const float* gamma, const float* mean,
                               const float* rstd, const void* add, long long ldadd, float* dx, long long lddx, void* dx16, long long lddxb,
                               int rows, int C, int h16, int add_every, int s16, prx_stream_t s) {
    return prx_layernorm_bwd(g, ldg, x, ldx, gamma, mean, rstd, add, ldadd, dx, lddx, B_(dx16), lddxb, rows, C, S_(s), h16,
                             add_every, s16, 1);
}
int prx_k_vit_pad_heads(const float* qkv_w, float* qkv_w_pad, const float* out_w, float* out_w_pad, int width, int heads, int hd, int hp,
                        prx_stream_t s) {
    PRX_REQUIRE(qkv_w && qkv_w_pad && out_w && out_w_pad && width == heads * hd, "vit_pad_heads: null argument or width != heads * head dim");
    int r = prx_vit_pad_head_rows(qkv_w, qkv_w_pad, heads, hd, hp, width, S_(s));
    return r ? r : prx_vit_pad_head_cols(out_w, out_w_pad, width, heads, hd, hp, S_(s));
}
int prx_k_mha_fwd_causal_op(const void* qkv, void* out, int N, int T, int C, int heads, int h16, prx_stream_t s) {
    return prx_mha_fwd(mha_desc(N, T, C, heads, 64, prec16(h16), 0, 1), qkv, out, nullptr, S_(s));
}
int prx_k_softmax_rows_op(const float* S, int lds_, float scale, void* P, int ldp, void* PT, int ldpt, int rows, int cols,
                          int prec, prx_stream_t s) {
    PRX_REQUIRE(prec_valid(prec), "softmax_rows: unknown precision %d", prec);
    return prx_softmax_rows(S, lds_, scale, P, ldp, PT, ldpt, rows, cols, prec, S_(s));
}
int prx_k_softmax_rows_bwd_op(const void* P, int ldp, const float* dP, int lddp, float scale, void* dS, int ldds, void* dST,
                              int lddst, int rows, int cols, int prec, prx_stream_t s) {
    PRX_REQUIRE(prec_valid(prec), "softmax_rows_bwd: unknown precision %d", prec);
    return prx_softmax_rows_bwd(P, ldp, dP, lddp, scale, dS, ldds, dST, lddst, rows, cols, prec, S_(s));
}
int prx_k_softmax_rows_tr_op(const float* S, int lds_, float scale, void* P, int ldp, void* PT, int ldpt, int rows, int cols,
                             const void* tin, int ldtin, void* tout, int ldtout, int tR, int tC, int prec, prx_stream_t s) {
    PRX_REQUIRE(prec_valid(prec), "softmax_rows_tr: unknown precision %d", prec);
    return prx_softmax_rows_tr(S, lds_, scale, P, ldp, PT, ldpt, rows, cols, tin, ldtin, tout, ldtout, tR, tC, prec, S_(s));
}
int prx_k_softmax_rows_bwd_tr_op(const void* P, int ldp, const float* dP, int lddp, float scale, void* dS, int ldds, void* dST,
                                 int lddst, int rows, int cols, const void* tin, int ldtin, void* tout, int ldtout, int tR, int tC,
                                 int prec, prx_stream_t s) {
    PRX_REQUIRE(prec_valid(prec), "softmax_rows_bwd_tr: unknown precision %d", prec);
    return prx_softmax_rows_bwd_tr(P, ldp, dP, lddp, scale, dS, ldds, dST, lddst, rows, cols, tin, ldtin, tout, ldtout, tR, tC, prec, S_(s));
}
int prx_k_transpose_op(const void* in, int ldin, void* out, int ldout, int R, int C, int f32, prx_stream_t s) {
    return prx_transpose_op(in, ldin, out, ldout, R, C, f32, S_(s));
}
int prx_k_upsample2x_bwd_op(const void* hi, float* low, void* low16, int NB, int Hl, int Wl, int C, int h16, int s16,
                            prx_stream_t s) {
    return prx_upsample2x_bwd(hi, low, B_(low16), NB, Hl, Wl, C, S_(s), h16, s16);
}
int prx_k_nchw_to_nhwc_op(const float* in, float* out_f32, void* out16, int NB, int C, int HW, int Cpad, int h16, prx_stream_t s) {
    return prx_nchw_to_nhwc(in, out_f32, B_(out16), NB, C, HW, Cpad, S_(s), h16);
}
int prx_k_image_head_bwd_op(const float* x, int ldc, const float* gimg, float* dx, void* dx16, int ldo, int NB, int C, int HW,
                            int h16, const float* gscale, prx_stream_t s) {
    return prx_image_head_bwd(x, ldc, gimg, dx, B_(dx16), ldo, NB, C, HW, S_(s), h16, gscale);
}
int prx_k_image_head_bwd_im2col(const float* x, int ldc, const float* gimg, void* col, int ldk, int C, int H, int W, int h16,
                                const float* gscale, prx_stream_t s) {
    return prx_image_head_bwd_im2col(x, ldc, gimg, B_(col), ldk, C, H, W, S_(s), h16, gscale);
}
int prx_k_grad_scale(const float* g, size_t n, float* part, int nparts, int target_log2, float* scale2, prx_stream_t s) {
    return prx_grad_scale(g, n, part, nparts, target_log2, scale2, S_(s));
}
int prx_k_grad_scale_multi(const float* const* gs, const size_t* ns, int count, float* part, int nparts_each, int target_log2,
                           float* scale2, prx_stream_t s) {
    return prx_grad_scale_multi(gs, ns, count, part, nparts_each, target_log2, scale2, S_(s));
}
int prx_k_scale_dev(float* x, size_t n, const float* scale, void* out16, int h16, prx_stream_t s) {
    return prx_scale_dev(x, n, scale, S_(s), B_(out16), h16);
}
int prx_k_f32_to_op16(const float* in, void* out16, size_t n, int h16, prx_stream_t s) {
    return prx_f32_to_bf16(in, B_(out16), n, S_(s), h16);
}
int prx_k_add_f32(const float* a, const float* b, float* out, size_t n, prx_stream_t s) {
    return prx_add_f32(a, b, out, n, S_(s));
}

// ---- the runners' own kernels through the launchers the runners call (tests/test_kernels_runner_gpu.py) -----------------------
int prx_k_rn_pack_conv3x3(const float* w, void* Wf, void* Wd, int Cout, int Cin, int prec, prx_stream_t s) {
    return prx_pack_conv3x3(w, Wf, Wd, Cout, Cin, Cin, Cout, prec, S_(s));
}
int prx_k_stem1_fwd(const float* cut, const float* mm, const float* w, const float* b, void* out, int N, int S, int CO, int prec, prx_stream_t s) {
    return prx_stem1_fwd(cut, mm, w, b, out, N, S, CO, prec, S_(s));
}
int prx_k_stem1_bwd(const void* g, const float* w, float* dY, int N, int S, int CO, const float* oscale_dev, int prec, prx_stream_t s) {
    return prx_stem1_bwd(g, w, dY, N, S, CO, oscale_dev, prec, S_(s));
}
int prx_k_avgpool2_fwd(const void* x, void* out, int N, int H, int W, int C, int prec, prx_stream_t s) {
    return prx_avgpool2_fwd(x, out, N, H, W, C, prec, S_(s));
}
int prx_k_avgpool2_bwd(const float* g, const void* mask, float* dx_f32, void* dx_op, int N, int H, int W, int C, int prec, prx_stream_t s) {
    return prx_avgpool2_bwd(g, mask, dx_f32, dx_op, N, H, W, C, prec, S_(s));
}
int prx_k_relu_mask(float* g, const void* out, void* g_op, size_t n, int prec, prx_stream_t s) {
    return prx_relu_mask(g, out, g_op, n, prec, S_(s));
}
int prx_k_tokens_fwd(const float* x, const float* pos, void* t, int N, int P, int C, int prec, prx_stream_t s) {
    return prx_tokens_fwd(x, pos, t, N, P, C, prec, S_(s));
}
int prx_k_tokens_bwd(const float* dt, float* dx, int N, int P, int C, int prec, prx_stream_t s) {
    return prx_tokens_bwd(dt, dx, N, P, C, prec, S_(s));
}
int prx_k_tok0_gather(const void* t, void* out, int N, int T, int C, int prec, prx_stream_t s) {
    return prx_tok0_gather(t, out, N, T, C, prec, S_(s));
}
int prx_k_tok0_scatter(const void* g0, void* dt, int N, int T, int C, int prec, prx_stream_t s) {
    return prx_tok0_scatter(g0, dt, N, T, C, prec, S_(s));
}
int prx_k_minmax(const float* x, size_t n, float* part, int nparts, float* mm, prx_stream_t s) {
    return prx_minmax(x, n, part, nparts, mm, S_(s));
}
int prx_k_patchify_fwd(const float* cut, const float* mm, void* A, int prec, int N, int S, int P, int T, float m0, float m1, float m2, float s0, float s1, float s2, prx_stream_t s) {
    return prx_patchify_fwd(cut, mm, A, prec, N, S, P, T, S_(s), PatchNorm{{m0, m1, m2}, {s0, s1, s2}});
}
int prx_k_patchify_bwd_reduce(const float* cut, const float* mm, const float* dA, double* acc, int N, int S, int P, int T, float m0, float m1, float m2, float s0, float s1, float s2, prx_stream_t s) {
    return prx_patchify_bwd_reduce(cut, mm, dA, acc, N, S, P, T, S_(s), PatchNorm{{m0, m1, m2}, {s0, s1, s2}});
}
int prx_k_patchify_bwd_apply(const float* cut, const float* mm, const float* dA, const double* acc, float* gcut, int N, int S, int P, int T, float m0, float m1, float m2, float s0, float s1, float s2, prx_stream_t s) {
    return prx_patchify_bwd_apply(cut, mm, dA, acc, gcut, N, S, P, T, S_(s), PatchNorm{{m0, m1, m2}, {s0, s1, s2}});
}
int prx_k_preproc_bwd_reduce(const float* cut, const float* mm, const float* dY, double* acc, int N, int S, prx_stream_t s) {
    return prx_preproc_bwd_reduce(cut, mm, dY, acc, N, S, S_(s));
}
int prx_k_preproc_bwd_apply(const float* cut, const float* mm, const float* dY, const double* acc, float* gcut, int N, int S, prx_stream_t s) {
    return prx_preproc_bwd_apply(cut, mm, dY, acc, gcut, N, S, S_(s));
}
// the cutout stages one at a time (tests/test_kernels_cutouts_gpu.py); `form` of the two backward launchers: cutouts.h
int prx_k_pool_fwd(const float* img, float* pooled, int* argmax, const unsigned char* mask, int C, int H, int W, int S, prx_stream_t s) {
    PRX_REQUIRE(img && pooled && argmax, "prx_k_pool_fwd: null argument");
    PRX_REQUIRE(C > 0 && H > 0 && W > 0 && S > 0, "prx_k_pool_fwd: sizes must be positive (C=%d H=%d W=%d S=%d)", C, H, W, S);
    return prx_pool_fwd(img, pooled, argmax, mask, C, H, W, S, S_(s));
}
int prx_k_pool_bwd(const float* g, const int* argmax, const unsigned char* mask, float* gimg, int C, int H, int W, int S, prx_stream_t s) {
    PRX_REQUIRE(g && argmax && gimg, "prx_k_pool_bwd: null argument");
    PRX_REQUIRE(C > 0 && H > 0 && W > 0 && S > 0, "prx_k_pool_bwd: sizes must be positive (C=%d H=%d W=%d S=%d)", C, H, W, S);
    return prx_pool_bwd(g, argmax, mask, gimg, C, H, W, S, S_(s));
}
int prx_k_rescale_fwd(const float* pooled, float* base, int C, int S, int Hb, int Wb, prx_stream_t s) {
    PRX_REQUIRE(pooled && base, "prx_k_rescale_fwd: null argument");
    PRX_REQUIRE(C > 0 && S > 0 && Hb > 0 && Wb > 0, "prx_k_rescale_fwd: sizes must be positive (C=%d S=%d Hb=%d Wb=%d)", C, S, Hb, Wb);
    return prx_rescale_fwd(pooled, base, C, S, Hb, Wb, S_(s));
}
int prx_k_rescale_bwd(const float* g_base, float* g_pooled, int C, int S, int Hb, int Wb, prx_stream_t s) {
    PRX_REQUIRE(g_base && g_pooled, "prx_k_rescale_bwd: null argument");
    PRX_REQUIRE(C > 0 && S > 0 && Hb > 0 && Wb > 0, "prx_k_rescale_bwd: sizes must be positive (C=%d S=%d Hb=%d Wb=%d)", C, S, Hb, Wb);
    return prx_rescale_bwd(g_base, g_pooled, C, S, Hb, Wb, S_(s));
}
int prx_k_warp_a_fwd(const float* src, int Hs, int Ws, const double* desc, float* out, int n_cut, int Ha, int Wa, prx_stream_t s) {
    PRX_REQUIRE(src && desc && out, "prx_k_warp_a_fwd: null argument");
    PRX_REQUIRE(n_cut > 0 && Hs > 1 && Ws > 1 && Ha > 1 && Wa > 1, "prx_k_warp_a_fwd: n_cut=%d source %dx%d destination %dx%d", n_cut, Hs, Ws, Ha, Wa);
    return prx_warp_a_fwd(src, Hs, Ws, desc, out, n_cut, Ha, Wa, S_(s));
}
int prx_k_warp_a_bwd(const float* g, int Hs, int Ws, const double* desc, float* uv, float* gsrc_priv, float* gsrc, int n_cut, int Ha, int Wa,
                     int form, prx_stream_t s) {
    PRX_REQUIRE(g && desc && uv && gsrc_priv && gsrc, "prx_k_warp_a_bwd: null argument");
    PRX_REQUIRE(n_cut > 0 && Hs > 1 && Ws > 1 && Ha > 1 && Wa > 1, "prx_k_warp_a_bwd: n_cut=%d source %dx%d destination %dx%d", n_cut, Hs, Ws, Ha, Wa);
    return prx_warp_a_bwd(g, Hs, Ws, desc, uv, gsrc_priv, gsrc, n_cut, Ha, Wa, S_(s), form);
}
int prx_k_warp_b_fwd(const float* a, int Ha, int Wa, const double* desc, const float* noise, float* out, int n_cut, int S, prx_stream_t s) {
    PRX_REQUIRE(a && desc && out, "prx_k_warp_b_fwd: null argument");
    PRX_REQUIRE(n_cut > 0 && Ha > 1 && Wa > 1 && S > 1, "prx_k_warp_b_fwd: n_cut=%d stage-A image %dx%d S=%d", n_cut, Ha, Wa, S);
    return prx_warp_b_fwd(a, Ha, Wa, desc, noise, out, n_cut, S, S_(s));
}
int prx_k_warp_b_bwd(const float* a, int Ha, int Wa, const double* desc, const float* g, float* grgb, float* uv, float* ga, int n_cut, int S,
                     float* maps_scratch, size_t maps_scratch_bytes, int form, prx_stream_t s) {
    PRX_REQUIRE(a && desc && g && grgb && uv && ga, "prx_k_warp_b_bwd: null argument");
    PRX_REQUIRE(n_cut > 0 && Ha > 1 && Wa > 1 && S > 1, "prx_k_warp_b_bwd: n_cut=%d stage-A image %dx%d S=%d", n_cut, Ha, Wa, S);
    return prx_warp_b_bwd(a, Ha, Wa, desc, g, grgb, uv, ga, n_cut, S, S_(s), maps_scratch, maps_scratch_bytes, form);
}
int prx_k_vgg_pack(const float* w, void* Wf, void* Wd, int Cout, int Cin, int CiP, int prec, prx_stream_t s) {
    return prx_pack_conv3x3(w, Wf, Wd, Cout, Cin, CiP, Cout, prec, S_(s));
}
int prx_k_vgg_input(const float* x, void* out, int HW, int prec, prx_stream_t s) {
    return prx_vgg_input(x, out, HW, prec, S_(s));
}
int prx_k_vgg_input_grad(const float* d, float* gx, int HW, const float* unscale, prx_stream_t s) {
    return prx_vgg_input_grad(d, gx, HW, unscale, S_(s));
}
int prx_k_vgg_maxpool(const void* x, void* out, void* arg, int H, int W, int C, int prec, prx_stream_t s) {
    return prx_vgg_maxpool(x, out, (unsigned char*)arg, H, W, C, prec, S_(s));
}
int prx_k_vgg_combine(const float* above, const void* arg, const float* gcap, const void* act, void* gpre, int H, int W, int C, const float* gscale, int prec, prx_stream_t s) {
    return prx_vgg_combine(above, (const unsigned char*)arg, gcap, act, gpre, H, W, C, gscale, prec, S_(s));
}
int prx_k_pack_conv3x3(const float* w, void* Wf, void* Wd, int Cout, int Cin, int CiP, int CoP, int prec, prx_stream_t s) {
    return prx_pack_conv3x3(w, Wf, Wd, Cout, Cin, CiP, CoP, prec, S_(s));
}
int prx_k_pack_transpose_op(const float* in, void* out, int R, int C, int prec, prx_stream_t s) {
    return prx_pack_transpose_op(in, out, R, C, prec, S_(s));
}
int prx_k_vit_add_cls_pos(float* x, const float* cls, const float* pos, int N, int T, int W, prx_stream_t s) {
    return prx_vit_add_cls_pos(x, cls, pos, N, T, W, S_(s));
}
int prx_k_vit_embed_tokens(const float* x, const float* cls, const float* pos, void* out, int out16, int N, int T, int W, prx_stream_t s) {
    return prx_vit_embed_tokens(x, cls, pos, out, out16, N, T, W, S_(s));
}
int prx_k_vit_gelu_f32(const float* t, float* io, size_t n, int bwd, prx_stream_t s) {
    return prx_vit_gelu_f32(t, io, n, bwd, S_(s));
}
int prx_k_vit_scale_f32(float* x, size_t n, float scale, int blocks, prx_stream_t s) {
    return prx_vit_scale_f32(x, n, scale, blocks, S_(s));
}
int prx_k_text_embed(const int* tokens, const float* emb, const float* pos, float* x, int* eot, int n, int ctx, int W, int vocab, prx_stream_t s) {
    return prx_text_embed(tokens, emb, pos, x, eot, n, ctx, W, vocab, S_(s));
}
int prx_k_gather_rows(const float* x, const int* eot, float* out, int n, int ctx, int W, prx_stream_t s) {
    return prx_gather_rows(x, eot, out, n, ctx, W, S_(s));
}
int prx_k_l2norm_fwd(const float* e, float* out, int n, int D, prx_stream_t s) {
    return prx_l2norm_fwd(e, out, n, D, S_(s));
}
int prx_k_l2norm_bwd(const float* e, const float* g, float* de, int n, int D, prx_stream_t s) {
    return prx_l2norm_bwd(e, g, de, n, D, S_(s));
}
int prx_k_vqgan_pack_conv3x3(const float* w, void* Wf, void* Wd, int Cout, int Cin, int CoP, int prec, prx_stream_t s) {
    return prx_pack_conv3x3(w, Wf, Wd, Cout, Cin, Cin, CoP, prec, S_(s));
}
int prx_k_vqgan_enc_pack_conv3x3(const float* w, void* Wf, int Cout, int Cin, int CiP, prx_stream_t s) {
    return prx_pack_conv3x3(w, Wf, nullptr, Cout, Cin, CiP, Cout, PRX_PREC_BF16, S_(s));
}
int prx_k_colminmax(const float* w, float* mn, float* mx, int rows, int D, prx_stream_t s) {
    return prx_colminmax(w, mn, mx, rows, D, S_(s));
}

// ---- the fft drawer's kernels (fft_drawer.hip), through the launchers prx_fft_drawer_synth / _backward call
int prx_k_fft_pack(const float* params, const float* scale, float* bt1, int W, int H, prx_stream_t s) {
    return prx_fft_pack(params, scale, bt1, W, H, S_(s));
}
int prx_k_fft_unpack(const float* dP, const float* scale, float* g_params, int W, int H, prx_stream_t s) {
    return prx_fft_unpack(dP, scale, g_params, W, H, S_(s));
}
int prx_k_fft_moments(const float* x, const float* y, size_t n, double* part, double* acc, prx_stream_t s) {
    return prx_fft_moments(x, y, n, part, acc, S_(s));
}
int prx_k_fft_tail_fwd(const float* x, const double* acc, float contrast, const float* cm, float* rgb, int W, int H, prx_stream_t s) {
    return prx_fft_tail_fwd(x, acc, contrast, cm, rgb, W, H, S_(s));
}
int prx_k_fft_tail_bwd_gy(const float* x, const float* g, const double* acc, float contrast, const float* cm, float* gy, int W, int H,
                          prx_stream_t s) {
    return prx_fft_tail_bwd_gy(x, g, acc, contrast, cm, gy, W, H, S_(s));
}
int prx_k_fft_tail_bwd_dx(const float* x, const float* gy, const double* acc, const double* bacc, float contrast, float* dxT, int W, int H,
                          prx_stream_t s) {
    return prx_fft_tail_bwd_dx(x, gy, acc, bacc, contrast, dxT, W, H, S_(s));
}

}  // extern "C"
