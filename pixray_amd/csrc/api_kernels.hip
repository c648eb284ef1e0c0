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
int prx_k_mha_fwd(const void* qkv, void* out, int N, int T, int C, int heads, prx_stream_t s) {
    return prx_mha_fwd(CB_(qkv), B_(out), N, T, C, heads, S_(s));
}
int prx_k_mha_bwd(const void* qkv, const void* dout, void* dqkv, int N, int T, int C, int heads, prx_stream_t s) {
    return prx_mha_bwd(CB_(qkv), CB_(dout), B_(dqkv), N, T, C, heads, S_(s));
}

int prx_k_mha_fwd_gen(const void* qkv, void* out, float* lse, int N, int T, int C, int heads, prx_stream_t s) {
    return prx_mha_fwd_gen(CB_(qkv), B_(out), lse, N, T, C, heads, S_(s));
}
int prx_k_mha_bwd_gen(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int N, int T, int C,
                      int heads, prx_stream_t s) {
    return prx_mha_bwd_gen(CB_(qkv), CB_(out), CB_(dout), lse, B_(dqkv), N, T, C, heads, S_(s));
}

int prx_k_mha_fwd_f32(const float* qkv, float* out, float* lse, int N, int T, int C, int heads, prx_stream_t s) {
    return prx_mha_fwd_f32(qkv, out, lse, N, T, C, heads, S_(s));
}
int prx_k_mha_bwd_f32(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, int N, int T, int C,
                      int heads, prx_stream_t s) {
    return prx_mha_bwd_f32(qkv, out, dout, lse, dqkv, N, T, C, heads, S_(s));
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
    return prx_mha_fwd(CB_(qkv), B_(out), N, T, C, heads, S_(s), h16);
}
int prx_k_mha_bwd_op(const void* qkv, const void* dout, void* dqkv, int N, int T, int C, int heads, int h16, prx_stream_t s) {
    return prx_mha_bwd(CB_(qkv), CB_(dout), B_(dqkv), N, T, C, heads, S_(s), h16);
}
int prx_k_mha_fwd_gen_op(const void* qkv, void* out, float* lse, int N, int T, int C, int heads, int h16, prx_stream_t s) {
    return prx_mha_fwd_gen(CB_(qkv), B_(out), lse, N, T, C, heads, S_(s), h16);
}
int prx_k_mha_bwd_gen_op(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int N, int T, int C,
                         int heads, int h16, prx_stream_t s) {
    return prx_mha_bwd_gen(CB_(qkv), CB_(out), CB_(dout), lse, B_(dqkv), N, T, C, heads, S_(s), h16);
}
int prx_k_mha_fwd_causal_op(const void* qkv, void* out, int N, int T, int C, int heads, int h16, prx_stream_t s) {
    return prx_mha_fwd_causal(CB_(qkv), B_(out), N, T, C, heads, S_(s), h16);
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

}  // extern "C"
