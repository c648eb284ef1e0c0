// CLIP ViT multi-head self-attention (nn.MultiheadAttention inside
// clip.model.ResidualAttentionBlock [UPSTREAM openai/CLIP clip/model.py], call
// site slip.py:65), forward and activation-gradient backward, for sequences of
// T <= 64 tokens with head dim 64 (ViT-B/32: T = 50).  One wave owns one
// (image, head): Q/K/V tiles live in LDS, S = QK^T, P = softmax(S/8) and O = PV
// run on v_mfma_f32_32x32x16_bf16 with the softmax done in the MFMA C layout by
// 32-lane butterflies.  Backward recomputes P and produces dQ/dK/dV in one pass.
//
// The kernels live in attention_kernels.h, templates on the 16-bit operand format: bf16 (FmtBf16, v_mfma_f32_32x32x16_bf16) and
// IEEE half (FmtF16, v_mfma_f32_32x32x16_f16, PRX_PREC_F16 -- the arithmetic of the reference's fp16 CLIP towers, slip.py:175).
// The workgroup-per-(image, head) family ("blk") is also a template on the operand columns per head: 64, 96 for heads of 80
// (OpenCLIP ViT-H/14) and 88 (ViT-g-14) zero-padded, 128 for heads of 104 (ViT-bigG-14).  The exact-f32 family is attention_f32.hip.
//
// This file is the host layer of all of them: prx_mha_fwd / prx_mha_bwd take a description of the problem (MhaDesc, attention.h),
// mha_plan decides which family takes it or refuses it, and the launchers below it only launch.
#include "attention_kernels.h"
#include "attention_f32.h"
#include <stdlib.h>
#include <atomic>

// Which family takes a general-T call at 64 columns.  The blk kernels split a head over gridDim.z workgroups of <= 5 waves, each
// streaming the head's whole K / V (or Q / dO), so nothing in them depends on T; they take T <= MHA_BLK_MAX_T = 640 (ViT-L/14@336px:
// 577 tokens = 19 token blocks on 4 x 5 waves), the tile kernels everything longer.  At N = 32, T = 577, 16 heads they measured
// 147 us forward / 441 us backward against the tile kernels' 623 / 3269 us.
// prx_mha_route (include/prx.h) chooses the route of the NEXT calls: -1 the rule above (PRX_MHA_TILES=1 in the environment: tiles
// everywhere, A/B measurements), 0 the blk family wherever it is able, 1 the tile kernels.  It is read at every launch, never kept
// in a handle.  The 96- and 128-wide instances have no tile fallback: they refuse T > MHA_BLK_MAX_T and ignore the route.
constexpr int MHA_BLK_MAX_T = 640;
static std::atomic<int> g_mha_route{-1};
extern "C" int prx_mha_route(int route) { return g_mha_route.exchange(route < 0 ? -1 : (route ? 1 : 0)); }
static bool prx_mha_blk_route(int T, int route) {
    static const bool env_tiles = [] { const char* e = getenv("PRX_MHA_TILES"); return e && e[0] == '1'; }();
    return T <= MHA_BLK_MAX_T && route != 1 && !(route < 0 && env_tiles);
}

int prx_mha_head_cols(int hd) {
    return (hd == 16 || hd == 32 || hd == 64) ? 64 : (hd == 80 || hd == 88) ? 96 : hd == 104 ? 128 : 0;
}
bool prx_mha_can_recompute(const MhaDesc& d) { return !prec_is_f32(d.prec) && !d.causal && d.hd == 64 && d.T <= 64; }

namespace {

// the family codes of prx_mha_describe (include/prx.h)
enum { MHA_WAVE = 1, MHA_BLK = 2, MHA_TILE = 3, MHA_F32 = 4 };

// The routing table: the family that takes `d` under `route` and the operand columns per head, or a refusal.
int mha_plan(const MhaDesc& d, int route, bool backward, int* family, int* cols_out) {
    PRX_REQUIRE(prec_valid(d.prec) && d.N >= 1 && d.T >= 1 && d.heads >= 1,
                "mha: needs a PRX_PREC_* precision and N, T, heads >= 1 (precision %d N=%d T=%d heads=%d)", d.prec, d.N, d.T, d.heads);
    const int cols = d.hd >= 64 ? prx_mha_head_cols(d.hd) : 0;
    PRX_REQUIRE(cols != 0, "mha: no kernel for head dim %d at %d columns per head (64 runs at 64, 80 | 88 at 96, 104 at 128)", d.hd,
                d.C / d.heads);
    PRX_REQUIRE(d.C == d.heads * cols, "mha: head dim %d at %d columns per head (C=%d heads=%d): it needs %d columns per head", d.hd,
                d.C / d.heads, d.C, d.heads, cols);
    *cols_out = cols;
    if (d.causal) {
        PRX_REQUIRE(!backward && !prec_is_f32(d.prec) && d.hd == 64,
                    "mha: the causal form is forward only, on 16-bit operands, and needs head dim 64 (head dim %d, precision %d)", d.hd, d.prec);
        *family = MHA_TILE;
    } else if (d.recompute) {
        PRX_REQUIRE(prx_mha_can_recompute(d), "mha: the recomputing form needs 16-bit operands, T <= 64 and head dim 64 (T=%d, head dim %d, precision %d)",
                    d.T, d.hd, d.prec);
        *family = MHA_WAVE;
    } else if (prec_is_f32(d.prec)) {
        *family = MHA_F32;
    } else if (cols != 64) {
        PRX_REQUIRE(d.T <= MHA_BLK_MAX_T, "mha: heads of %d columns have the blk family alone, which needs 1 <= T <= %d (T=%d, head dim %d)", cols,
                    MHA_BLK_MAX_T, d.T, d.hd);
        *family = MHA_BLK;
    } else {
        *family = prx_mha_blk_route(d.T, route) ? MHA_BLK : MHA_TILE;
    }
    return 0;
}

// the blk family: workgroups of <= WPB waves per (image, head), one wave per 32 tokens
template <typename F, int HDP>
int mha_fwd_blk(const MhaDesc& d, const El<F>* qkv, El<F>* out, float* lse, hipStream_t s) {
    const int nw = ceil_div(d.T, 32), nsplit = ceil_div(nw, WPB), wpb = ceil_div(nw, nsplit);
    hipLaunchKernelGGL((mha_fwd_blk_kernel<F, HDP>), dim3(d.heads, d.N, nsplit), dim3(64 * wpb), 0, s, qkv, out, lse, d.T, d.C, d.heads,
                       prx_mha_scale(d.hd), prx_xcd_local());
    PRX_LAUNCH_CHECK();
    return 0;
}
template <typename F, int HDP>
int mha_bwd_blk(const MhaDesc& d, const El<F>* qkv, const El<F>* out, const El<F>* dout, const float* lse, El<F>* dqkv, hipStream_t s) {
    const int nw = ceil_div(d.T, 32), nsplit = ceil_div(nw, WPB), wpb = ceil_div(nw, nsplit);
    const dim3 g(d.heads, d.N, nsplit), b(64 * wpb);
    const float scale = prx_mha_scale(d.hd);
    const int xcd = prx_xcd_local();
    hipLaunchKernelGGL((mha_bwd_dq_blk_kernel<F, HDP>), g, b, 0, s, qkv, out, dout, lse, dqkv, d.T, d.C, d.heads, scale, xcd);
    PRX_LAUNCH_CHECK();
    hipLaunchKernelGGL((mha_bwd_dkv_blk_kernel<F, HDP>), g, b, 0, s, qkv, out, dout, lse, dqkv, d.T, d.C, d.heads, scale, xcd);
    PRX_LAUNCH_CHECK();
    return 0;
}

template <typename F>
int mha_fwd_16(const MhaDesc& d, int family, int cols, const El<F>* qkv, El<F>* out, float* lse, hipStream_t s) {
    if (family == MHA_BLK)
        return cols == 64 ? mha_fwd_blk<F, 64>(d, qkv, out, lse, s) : cols == 96 ? mha_fwd_blk<F, 96>(d, qkv, out, lse, s)
                                                                                 : mha_fwd_blk<F, 128>(d, qkv, out, lse, s);
    const float scale = prx_mha_scale(d.hd);
    if (family == MHA_WAVE) {        // one wave per (image, head), T <= 64
        hipLaunchKernelGGL(mha_fwd_kernel<F>, dim3(d.heads, d.N), dim3(128), 0, s, qkv, out, d.T, d.C, scale, prx_xcd_local());
    } else if (d.causal) {           // the tile kernels: one wave per 64-token tile, online softmax
        hipLaunchKernelGGL((mha_fwd_gen_kernel<F, true>), dim3(ceil_div(d.T, 64), d.heads, d.N), dim3(64), 0, s, qkv, out, (float*)nullptr, d.T,
                           d.C, d.heads, scale);
    } else {
        hipLaunchKernelGGL((mha_fwd_gen_kernel<F, false>), dim3(ceil_div(d.T, 64), d.heads, d.N), dim3(64), 0, s, qkv, out, lse, d.T, d.C,
                           d.heads, scale);
    }
    PRX_LAUNCH_CHECK();
    return 0;
}
template <typename F>
int mha_bwd_16(const MhaDesc& d, int family, int cols, const El<F>* qkv, const El<F>* out, const El<F>* dout, const float* lse, El<F>* dqkv,
               hipStream_t s) {
    if (family == MHA_BLK)
        return cols == 64 ? mha_bwd_blk<F, 64>(d, qkv, out, dout, lse, dqkv, s) : cols == 96 ? mha_bwd_blk<F, 96>(d, qkv, out, dout, lse, dqkv, s)
                                                                                             : mha_bwd_blk<F, 128>(d, qkv, out, dout, lse, dqkv, s);
    const float scale = prx_mha_scale(d.hd);
    if (family == MHA_WAVE) {
        hipLaunchKernelGGL(mha_bwd_kernel<F>, dim3(d.heads, d.N), dim3(128), 0, s, qkv, dout, dqkv, d.T, d.C, scale, prx_xcd_local());
        PRX_LAUNCH_CHECK();
        return 0;
    }
    const dim3 grid(ceil_div(d.T, 64), d.heads, d.N);
    hipLaunchKernelGGL(mha_bwd_dq_gen_kernel<F>, grid, dim3(64), 0, s, qkv, out, dout, lse, dqkv, d.T, d.C, d.heads, scale);
    PRX_LAUNCH_CHECK();
    hipLaunchKernelGGL(mha_bwd_dkv_gen_kernel<F>, grid, dim3(64), 0, s, qkv, out, dout, lse, dqkv, d.T, d.C, d.heads, scale);
    PRX_LAUNCH_CHECK();
    return 0;
}

}  // namespace

int prx_mha_fwd(const MhaDesc& d, const void* qkv, void* out, float* lse, hipStream_t s) {
    int family, cols, r;
    if ((r = mha_plan(d, g_mha_route.load(std::memory_order_relaxed), false, &family, &cols))) return r;
    if (family == MHA_F32) return prx_mha_f32_fwd(d, (const float*)qkv, (float*)out, lse, s);
    return prec_is_h16(d.prec) ? mha_fwd_16<FmtF16>(d, family, cols, (const half_t*)qkv, (half_t*)out, lse, s)
                               : mha_fwd_16<FmtBf16>(d, family, cols, (const bf16_t*)qkv, (bf16_t*)out, lse, s);
}
int prx_mha_bwd(const MhaDesc& d, const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, hipStream_t s) {
    int family, cols, r;
    if ((r = mha_plan(d, g_mha_route.load(std::memory_order_relaxed), true, &family, &cols))) return r;
    if (family == MHA_F32) return prx_mha_f32_bwd(d, (const float*)qkv, (const float*)out, (const float*)dout, lse, (float*)dqkv, s);
    return prec_is_h16(d.prec)
               ? mha_bwd_16<FmtF16>(d, family, cols, (const half_t*)qkv, (const half_t*)out, (const half_t*)dout, lse, (half_t*)dqkv, s)
               : mha_bwd_16<FmtBf16>(d, family, cols, (const bf16_t*)qkv, (const bf16_t*)out, (const bf16_t*)dout, lse, (bf16_t*)dqkv, s);
}

// include/prx.h: what the two functions above would do with such a problem under `route`, from the same mha_plan
extern "C" int prx_mha_describe(int precision, int head_dim, int T, int causal, int recompute, int route, int* family, int* head_cols,
                                int* saves_out) {
    MhaDesc d;
    d.N = 1; d.T = T; d.heads = 1; d.hd = head_dim; d.prec = precision; d.causal = causal; d.recompute = recompute;
    d.C = (head_dim >= 64 && prx_mha_head_cols(head_dim)) ? prx_mha_head_cols(head_dim) : head_dim;
    *family = 0; *head_cols = 0;       // a refusal leaves the family at 0; its text is prx_last_error's
    *saves_out = prx_mha_saves_out(d);
    return mha_plan(d, route < 0 ? -1 : (route ? 1 : 0), false, family, head_cols);
}
