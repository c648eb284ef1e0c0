// CLIP ViT multi-head self-attention (nn.MultiheadAttention inside
// clip.model.ResidualAttentionBlock [UPSTREAM openai/CLIP clip/model.py], call
// site slip.py:65), forward and activation-gradient backward, for sequences of
// T <= 64 tokens with head dim 64 (ViT-B/32: T = 50).  One wave owns one
// (image, head): Q/K/V tiles live in LDS, S = QK^T, P = softmax(S/8) and O = PV
// run on v_mfma_f32_32x32x16_bf16 with the softmax done in the MFMA C layout by
// 32-lane butterflies.  Backward recomputes P and produces dQ/dK/dV in one pass.
//
// The kernels live in attention_kernels.h, templates on the 16-bit operand format: bf16 (FmtBf16, v_mfma_f32_32x32x16_bf16) and
// IEEE half (FmtF16, v_mfma_f32_32x32x16_f16, PRX_PREC_F16 -- the arithmetic of the reference's fp16 CLIP towers, slip.py:175); the
// public entry points pick the instantiation from `h16`.  The workgroup-per-(image, head) family is also a template on the operand
// columns per head: 64, and 96 for heads of 80 zero-padded (OpenCLIP ViT-H/14, prx_mha_*_hd96).
#include "attention_kernels.h"
#include <stdlib.h>
#include <atomic>

// Which family takes a general-T call.  The workgroup-per-(image, head) kernels (attention_kernels.h, "blk") split a head over
// gridDim.z workgroups of <= 5 waves, each streaming the head's whole K / V (or Q / dO), so nothing in them depends on T; they take
// T <= MHA_BLK_MAX_T = 640 (ViT-L/14@336px: 577 tokens = 19 token blocks on 4 x 5 waves), the tile kernels everything longer.  At N = 32,
// T = 577, 16 heads they measured 147 us forward / 441 us backward against the tile kernels' 623 / 3269 us.
// prx_mha_route (include/prx.h) chooses the route of the NEXT calls: -1 the rule above (PRX_MHA_TILES=1 in the environment: tiles
// everywhere, A/B measurements), 0 the workgroup family wherever it is able, 1 the tile kernels.  The 96-wide instances have no tile
// fallback: prx_mha_*_hd96 refuse T > MHA_BLK_MAX_T and ignore the route.
constexpr int MHA_BLK_MAX_T = 640;
static std::atomic<int> g_mha_route{-1};
extern "C" int prx_mha_route(int route) { return g_mha_route.exchange(route < 0 ? -1 : (route ? 1 : 0)); }
static bool prx_mha_blk_route(int T) {
    static const bool env_tiles = [] { const char* e = getenv("PRX_MHA_TILES"); return e && e[0] == '1'; }();
    const int route = g_mha_route.load(std::memory_order_relaxed);
    return T <= MHA_BLK_MAX_T && route != 1 && !(route < 0 && env_tiles);
}

namespace {

template <typename F>
int mha_fwd(const El<F>* qkv, El<F>* out, int N, int T, int C, int heads, hipStream_t s) {
    PRX_REQUIRE(T <= 64 && C == heads * 64, "mha: needs T <= 64 and head dim 64 (T=%d C=%d heads=%d)", T, C, heads);
    hipLaunchKernelGGL(mha_fwd_kernel<F>, dim3(heads, N), dim3(128), 0, s, qkv, out, T, C, 0.125f, prx_xcd_local());
    PRX_LAUNCH_CHECK();
    return 0;
}
template <typename F>
int mha_bwd(const El<F>* qkv, const El<F>* dout, El<F>* dqkv, int N, int T, int C, int heads, hipStream_t s) {
    PRX_REQUIRE(T <= 64 && C == heads * 64, "mha bwd: needs T <= 64 and head dim 64 (T=%d C=%d heads=%d)", T, C, heads);
    hipLaunchKernelGGL(mha_bwd_kernel<F>, dim3(heads, N), dim3(128), 0, s, qkv, dout, dqkv, T, C, 0.125f, prx_xcd_local());
    PRX_LAUNCH_CHECK();
    return 0;
}

// the blk family: workgroups of <= WPB waves per (image, head), one wave per 32 tokens
template <typename F, int HDP>
int mha_fwd_blk(const El<F>* qkv, El<F>* out, float* lse, int N, int T, int C, int heads, float scale, hipStream_t s) {
    const int nw = ceil_div(T, 32), nsplit = ceil_div(nw, WPB), wpb = ceil_div(nw, nsplit);
    hipLaunchKernelGGL((mha_fwd_blk_kernel<F, HDP>), dim3(heads, N, nsplit), dim3(64 * wpb), 0, s, qkv, out, lse, T, C, heads, scale,
                       prx_xcd_local());
    PRX_LAUNCH_CHECK();
    return 0;
}
template <typename F, int HDP>
int mha_bwd_blk(const El<F>* qkv, const El<F>* out, const El<F>* dout, const float* lse, El<F>* dqkv, int N, int T, int C, int heads,
                float scale, hipStream_t s) {
    const int nw = ceil_div(T, 32), nsplit = ceil_div(nw, WPB), wpb = ceil_div(nw, nsplit);
    const dim3 g(heads, N, nsplit), b(64 * wpb);
    const int xcd = prx_xcd_local();
    hipLaunchKernelGGL((mha_bwd_dq_blk_kernel<F, HDP>), g, b, 0, s, qkv, out, dout, lse, dqkv, T, C, heads, scale, xcd);
    PRX_LAUNCH_CHECK();
    hipLaunchKernelGGL((mha_bwd_dkv_blk_kernel<F, HDP>), g, b, 0, s, qkv, out, dout, lse, dqkv, T, C, heads, scale, xcd);
    PRX_LAUNCH_CHECK();
    return 0;
}

template <typename F>
int mha_fwd_gen(const El<F>* qkv, El<F>* out, float* lse, int N, int T, int C, int heads, hipStream_t s) {
    PRX_REQUIRE(C == heads * 64 && T >= 1, "mha(gen): needs head dim 64 (T=%d C=%d heads=%d)", T, C, heads);
    if (prx_mha_blk_route(T)) return mha_fwd_blk<F, 64>(qkv, out, lse, N, T, C, heads, 0.125f, s);
    hipLaunchKernelGGL((mha_fwd_gen_kernel<F, false>), dim3(ceil_div(T, 64), heads, N), dim3(64), 0, s, qkv, out, lse, T, C, heads, 0.125f);
    PRX_LAUNCH_CHECK();
    return 0;
}
template <typename F>
int mha_fwd_causal(const El<F>* qkv, El<F>* out, int N, int T, int C, int heads, hipStream_t s) {
    PRX_REQUIRE(C == heads * 64 && T >= 1, "mha(causal): needs head dim 64 (T=%d C=%d heads=%d)", T, C, heads);
    hipLaunchKernelGGL((mha_fwd_gen_kernel<F, true>), dim3(ceil_div(T, 64), heads, N), dim3(64), 0, s, qkv, out, (float*)nullptr, T, C,
                       heads, 0.125f);
    PRX_LAUNCH_CHECK();
    return 0;
}
template <typename F>
int mha_bwd_gen(const El<F>* qkv, const El<F>* out, const El<F>* dout, const float* lse, El<F>* dqkv, int N, int T, int C, int heads,
                hipStream_t s) {
    PRX_REQUIRE(C == heads * 64 && T >= 1, "mha(gen) bwd: needs head dim 64 (T=%d C=%d heads=%d)", T, C, heads);
    if (prx_mha_blk_route(T)) return mha_bwd_blk<F, 64>(qkv, out, dout, lse, dqkv, N, T, C, heads, 0.125f, s);
    dim3 grid(ceil_div(T, 64), heads, N);
    hipLaunchKernelGGL(mha_bwd_dq_gen_kernel<F>, grid, dim3(64), 0, s, qkv, out, dout, lse, dqkv, T, C, heads, 0.125f);
    PRX_LAUNCH_CHECK();
    hipLaunchKernelGGL(mha_bwd_dkv_gen_kernel<F>, grid, dim3(64), 0, s, qkv, out, dout, lse, dqkv, T, C, heads, 0.125f);
    PRX_LAUNCH_CHECK();
    return 0;
}

}  // namespace

#define H(p) reinterpret_cast<const half_t*>(p)
#define HM(p) reinterpret_cast<half_t*>(p)
int prx_mha_fwd(const bf16_t* qkv, bf16_t* out, int N, int T, int C, int heads, hipStream_t s, int h16) {
    return h16 ? mha_fwd<FmtF16>(H(qkv), HM(out), N, T, C, heads, s) : mha_fwd<FmtBf16>(qkv, out, N, T, C, heads, s);
}
int prx_mha_bwd(const bf16_t* qkv, const bf16_t* dout, bf16_t* dqkv, int N, int T, int C, int heads, hipStream_t s, int h16) {
    return h16 ? mha_bwd<FmtF16>(H(qkv), H(dout), HM(dqkv), N, T, C, heads, s) : mha_bwd<FmtBf16>(qkv, dout, dqkv, N, T, C, heads, s);
}
int prx_mha_fwd_gen(const bf16_t* qkv, bf16_t* out, float* lse, int N, int T, int C, int heads, hipStream_t s, int h16) {
    return h16 ? mha_fwd_gen<FmtF16>(H(qkv), HM(out), lse, N, T, C, heads, s) : mha_fwd_gen<FmtBf16>(qkv, out, lse, N, T, C, heads, s);
}
int prx_mha_fwd_causal(const bf16_t* qkv, bf16_t* out, int N, int T, int C, int heads, hipStream_t s, int h16) {
    return h16 ? mha_fwd_causal<FmtF16>(H(qkv), HM(out), N, T, C, heads, s) : mha_fwd_causal<FmtBf16>(qkv, out, N, T, C, heads, s);
}
int prx_mha_bwd_gen(const bf16_t* qkv, const bf16_t* out, const bf16_t* dout, const float* lse, bf16_t* dqkv, int N, int T,
                    int C, int heads, hipStream_t s, int h16) {
    return h16 ? mha_bwd_gen<FmtF16>(H(qkv), H(out), H(dout), lse, HM(dqkv), N, T, C, heads, s)
               : mha_bwd_gen<FmtBf16>(qkv, out, dout, lse, dqkv, N, T, C, heads, s);
}
int prx_mha_fwd_hd96(const bf16_t* qkv, bf16_t* out, float* lse, int N, int T, int C, int heads, float scale, hipStream_t s, int h16) {
    PRX_REQUIRE(C == heads * 96 && T >= 1 && T <= MHA_BLK_MAX_T && N >= 1,
                "mha(hd96): needs 96 columns per head and 1 <= T <= %d (T=%d C=%d heads=%d)", MHA_BLK_MAX_T, T, C, heads);
    return h16 ? mha_fwd_blk<FmtF16, 96>(H(qkv), HM(out), lse, N, T, C, heads, scale, s)
               : mha_fwd_blk<FmtBf16, 96>(qkv, out, lse, N, T, C, heads, scale, s);
}
int prx_mha_bwd_hd96(const bf16_t* qkv, const bf16_t* out, const bf16_t* dout, const float* lse, bf16_t* dqkv, int N, int T, int C,
                     int heads, float scale, hipStream_t s, int h16) {
    PRX_REQUIRE(C == heads * 96 && T >= 1 && T <= MHA_BLK_MAX_T && N >= 1,
                "mha(hd96) bwd: needs 96 columns per head and 1 <= T <= %d (T=%d C=%d heads=%d)", MHA_BLK_MAX_T, T, C, heads);
    return h16 ? mha_bwd_blk<FmtF16, 96>(H(qkv), H(out), H(dout), lse, HM(dqkv), N, T, C, heads, scale, s)
               : mha_bwd_blk<FmtBf16, 96>(qkv, out, dout, lse, dqkv, N, T, C, heads, scale, s);
}
// heads of 104 zero-padded to 128 columns (OpenCLIP ViT-bigG-14); the chunked kernels do not depend on T, so the cap is the family's
int prx_mha_fwd_hd128(const bf16_t* qkv, bf16_t* out, float* lse, int N, int T, int C, int heads, float scale, hipStream_t s, int h16) {
    PRX_REQUIRE(C == heads * 128 && T >= 1 && T <= MHA_BLK_MAX_T && N >= 1,
                "mha(hd128): needs 128 columns per head and 1 <= T <= %d (T=%d C=%d heads=%d)", MHA_BLK_MAX_T, T, C, heads);
    return h16 ? mha_fwd_blk<FmtF16, 128>(H(qkv), HM(out), lse, N, T, C, heads, scale, s)
               : mha_fwd_blk<FmtBf16, 128>(qkv, out, lse, N, T, C, heads, scale, s);
}
int prx_mha_bwd_hd128(const bf16_t* qkv, const bf16_t* out, const bf16_t* dout, const float* lse, bf16_t* dqkv, int N, int T, int C,
                      int heads, float scale, hipStream_t s, int h16) {
    PRX_REQUIRE(C == heads * 128 && T >= 1 && T <= MHA_BLK_MAX_T && N >= 1,
                "mha(hd128) bwd: needs 128 columns per head and 1 <= T <= %d (T=%d C=%d heads=%d)", MHA_BLK_MAX_T, T, C, heads);
    return h16 ? mha_bwd_blk<FmtF16, 128>(H(qkv), H(out), H(dout), lse, HM(dqkv), N, T, C, heads, scale, s)
               : mha_bwd_blk<FmtBf16, 128>(qkv, out, dout, lse, dqkv, N, T, C, heads, scale, s);
}
