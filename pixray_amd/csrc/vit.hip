// CLIP visual tower runner (clip.model.VisionTransformer [UPSTREAM openai/CLIP], as called by
// CLIP_Base.encode_image, slip.py:62-66): forward and activation-gradient backward on the
// MFMA engine.  The same runner serves the SLIP family (SLIP_Base.encode_image, slip.py:151-157: a timm VisionTransformer
// [UPSTREAM facebookresearch/SLIP models.py, timm]) through the four switches of VitFamily (vit.h): a patch-embed bias, no
// ln_pre, LayerNorm eps 1e-6, the exact GELU -- and the preprocessing constants of the first kernel.  Residual stream and LayerNorm statistics stay fp32; every GEMM operand
// (LN outputs, qkv, attention output, MLP hidden) is bf16; weights are packed once to bf16 in
// both orientations (forward Bt = W[out,in], dgrad Bt = W^T[in,out]) because they are frozen
// (slip.py:176).  With precision == PRX_PREC_F32 the same operand buffers hold fp32, the GEMMs run on
// v_mfma_f32_32x32x2_f32 and attention on the fp32 kernels of attention_f32.hip: the exact parity mode.
#include "vit.h"
#include <stdlib.h>
#include "gemm.h"
#include "norms.h"
#include "attention.h"
#include "cutouts.h"
#include "prompt_vq.h"
#include "elementwise.h"
#include "weight_pack.h"
#include "runner_core.h"
#include <vector>
#include <memory>

namespace {

__global__ __launch_bounds__(256) void add_cls_pos_kernel(float* __restrict__ x, const float* __restrict__ cls,
                                                          const float* __restrict__ pos, int N, int T, int W) {
    const size_t total = (size_t)N * T * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % W);
        const int t = (int)((i / W) % T);
        float v = x[i] + pos[(size_t)t * W + c];
        if (t == 0) v += cls[c];
        x[i] = v;
    }
}

// the family without ln_pre: tokens = [cls + pos[0] ; conv + bias + pos[t]] go straight into the first block's stream (fp32, or the
// 16-bit stream of the lean layout).  The class-token row of the patch-embed product holds the bias alone (its A row is zero) and is
// not read.
template <typename TOut>
__global__ __launch_bounds__(256) void embed_tokens_kernel(const float* __restrict__ x, const float* __restrict__ cls,
                                                           const float* __restrict__ pos, TOut* __restrict__ out, int N, int T, int W) {
    const size_t total = (size_t)N * T * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % W);
        const int t = (int)((i / W) % T);
        const float p = pos[(size_t)t * W + c];
        op_st(out, i, t == 0 ? cls[c] + p : x[i] + p);
    }
}

// The exact mode's GELU: the fp32-operand 4-wave kernel has the scalar epilogue only, which carries no erff (gemm_epi.h), so the
// parity mode of the SLIP family applies the activation in a pass of its own -- out = gelu(t), or io *= gelu'(t) in the backward
// (the same expressions as the fused epilogues of the 16-bit modes; at 1/16 of the MFMA rate the extra pass is not the cost)
__global__ __launch_bounds__(256) void scale_f32_kernel(float* __restrict__ x, size_t n, float s) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) x[i] *= s;
}

template <bool BWD>
__global__ __launch_bounds__(256) void gelu_f32_kernel(const float* __restrict__ t, float* __restrict__ io, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float x = t[i];
        const float cdf = 0.5f * (1.f + erff(x * 0.70710678f));
        if (BWD) io[i] *= cdf + x * (0.39894228f * expf(-0.5f * x * x));
        else io[i] = x * cdf;
    }
}

}  // namespace

// launchers of the token-embedding and exact-mode activation kernels (vit.h): shared by the runner below and the kernel-level tests
int prx_vit_add_cls_pos(float* x, const float* cls, const float* pos, int N, int T, int W, hipStream_t s) {
    hipLaunchKernelGGL(add_cls_pos_kernel, dim3(2048), dim3(256), 0, s, x, cls, pos, N, T, W);
    PRX_LAUNCH_CHECK();
    return 0;
}
int prx_vit_embed_tokens(const float* x, const float* cls, const float* pos, void* out, int out16, int N, int T, int W, hipStream_t s) {
    if (out16) hipLaunchKernelGGL(embed_tokens_kernel<half_t>, dim3(2048), dim3(256), 0, s, x, cls, pos, (half_t*)out, N, T, W);   // lean implies IEEE half
    else hipLaunchKernelGGL(embed_tokens_kernel<float>, dim3(2048), dim3(256), 0, s, x, cls, pos, (float*)out, N, T, W);
    PRX_LAUNCH_CHECK();
    return 0;
}
int prx_vit_gelu_f32(const float* t, float* io, size_t n, int bwd, hipStream_t s) {
    if (bwd) hipLaunchKernelGGL(gelu_f32_kernel<true>, dim3(2048), dim3(256), 0, s, t, io, n);
    else hipLaunchKernelGGL(gelu_f32_kernel<false>, dim3(2048), dim3(256), 0, s, t, io, n);
    PRX_LAUNCH_CHECK();
    return 0;
}
int prx_vit_scale_f32(float* x, size_t n, float scale, int blocks, hipStream_t s) {
    PRX_REQUIRE(blocks >= 1, "scale_f32: %d workgroups", blocks);
    hipLaunchKernelGGL(scale_f32_kernel, dim3(blocks), dim3(256), 0, s, x, n, scale);
    PRX_LAUNCH_CHECK();
    return 0;
}

// Padded heads (PrxVit::hd below): every head's hd rows of the qkv projection (sections q | k | v; `row` floats per row: the weight's
// width, or 1 for the bias) become the first hd of hp rows, the rest zero ...
int prx_vit_pad_head_rows(const float* src, float* dst, int heads, int hd, int hp, int row, hipStream_t s) {
    PRX_REQUIRE(heads >= 1 && hd >= 1 && hp >= hd && row >= 1, "pad_head_rows: %d heads of %d -> %d, %d floats per row", heads, hd, hp, row);
    PRX_CHECK_HIP(hipMemsetAsync(dst, 0, sizeof(float) * (size_t)3 * heads * hp * row, s));
    for (int sect = 0; sect < 3; ++sect)
        PRX_CHECK_HIP(hipMemcpy2DAsync(dst + (size_t)sect * heads * hp * row, sizeof(float) * hp * row, src + (size_t)sect * heads * hd * row,
                                       sizeof(float) * hd * row, sizeof(float) * hd * row, heads, hipMemcpyDeviceToDevice, s));
    return 0;
}
// ... and the matching input columns of the out-projection: [W, heads * hd] -> [W, heads * hp]
int prx_vit_pad_head_cols(const float* src, float* dst, int W, int heads, int hd, int hp, hipStream_t s) {
    PRX_REQUIRE(W >= 1 && heads >= 1 && hd >= 1 && hp >= hd, "pad_head_cols: %d heads of %d -> %d", heads, hd, hp);
    PRX_CHECK_HIP(hipMemsetAsync(dst, 0, sizeof(float) * (size_t)W * heads * hp, s));
    PRX_CHECK_HIP(hipMemcpy2DAsync(dst, sizeof(float) * hp, src, sizeof(float) * hd, sizeof(float) * hd, (size_t)W * heads, hipMemcpyDeviceToDevice, s));
    return 0;
}

struct VitLayer {
    float *ln1_g, *ln1_b, *bqkv, *bo, *ln2_g, *ln2_b, *b1, *b2;
    void *Wqkv, *WqkvT, *Wo, *WoT, *W1, *W1T, *W2, *W2T;   // operand precision (bf16 | fp32)
    // saved activations (x_in / x_mid: the residual stream, fp32 -- or the 16-bit operand format in the lean layout)
    void *x_in, *x_mid;
    float *mean1, *rstd1, *mean2, *rstd2;
    void *qkv, *t;    // operand precision
    void* o_save;     // attention output and log-sum-exp, kept for the backward where prx_mha_saves_out(PrxVit::att); else null
    float* lse;
};

struct PrxVit : ImageTower {
    int patch, width, layers, heads, T, KP;
    // Padded heads (SLIP's ViT-S/16: 12 heads of 32 on width 384): the attention kernels are head-dim-64, so every head's q, k and v
    // rows of the qkv projection (weight and bias) are zero-padded to 64 at packing time, and so are the matching input columns of the
    // out-projection; sqrt(64 / head dim) is folded into the q rows before they are rounded to the operand format, because the
    // kernels' softmax scale is fixed at 1 / sqrt(64).  The padded lanes carry exact zeros forward (zero weights, zero bias) and
    // backward (dQ_pad = dS K_pad, dK_pad = dS^T Q_pad, dV_pad = P^T dO_pad with dO_pad = dx Wo_pad^T = 0), so values and gradients
    // are those of the narrow heads; the price is 64 / head dim times the qkv, attention and out-projection work.
    // Heads of 80 (OpenCLIP ViT-H/14: 16 heads on width 1280) are padded the same way to hp = 96 columns and run on the 96-wide
    // attention family (the 96-wide instances of attention_kernels.h), which takes the softmax scale 1 / sqrt(80) as an argument: nothing is folded into q.
    // Heads of 88 (ViT-g-14: 16 heads on width 1408) run there too with 1 / sqrt(88); heads of 104 (ViT-bigG-14: 16 on 1664) are padded to
    // hp = 128 and run on the 128-wide instances with 1 / sqrt(104) (prx_mha_head_cols, attention.h, is the mapping).
    int hd, hp, aw;    // head dim of the weights; operand columns per head (64 | 96 | 128); attention width = heads * hp (== width when hd == 64)
    MhaDesc att;       // the attention of every block (N is set per call): the recomputing form where it has a kernel, else out + lse are saved
    int mlp;           // hidden width of the MLP: fam.mlp_width, or 4 * width (every tower but OpenCLIP's ViT-g-14 6144 and ViT-bigG-14 8192)
    // RunnerEngine::mem holds every device buffer below (weights + one forward's activations for max_n cutouts)
    void *Wp, *WpT, *projT, *proj;
    float *cls, *pos, *lnpre_g, *lnpre_b, *lnpost_g, *lnpost_b;
    std::vector<VitLayer> L;
    // workspace
    void *A0, *h, *att_o, *u, *hpost, *dt, *do_, *dqkv, *dx_bf, *dh_bf;   // operand precision
    float *xpre, *mean_pre, *rstd_pre, *mean_post, *rstd_post, *dx, *dh, *dA0, *dhpost;
    void* x_final;
    // The lean layout (half mode, PRX_LEAN): the residual stream and its gradient live in IEEE half only -- the reference's own
    // GPU arithmetic for this tower (slip.py:175: the CLIP model runs in fp16, residual adds included).  One 16-bit tensor is
    // the saved activation, the LayerNorm input and the residual operand of the next product; dx / dh have no fp32 copy.
    int lean;
    VitFamily fam;     // what differs between the CLIP and the SLIP towers (vit.h)
    float* bp;         // patch-embed bias (fam.patch_bias), else null
    int cls_tail;      // 1 (default): the class-token tail below; PRX_VIT_CLS_TAIL=0 runs the last block on every token row (A/B, bisection)
    // The class-token tail: only the class token of the LAST block's output is ever read (ln_post on token 0, slip.py:66 / clip
    // VisionTransformer), so that block's out-projection, MLP and their backward run on the n class-token rows (row stride
    // T * width into the same buffers) instead of all n * T token rows: the same values for everything that is read, 3 + 3 of
    // the tower's 48 + 48 wide products reduced to M = n.  K and V of that block still need every token.  (Round-5 A/B on the
    // device: 140.1 -> 141.2 and 138.0 -> 139.5 it/s, profiles/r05_first_call/, r05_timeline/.)
    int forward(const float* cutouts, int n, const float* mm, float* embeds, hipStream_t s) override;
    int backward_a(const float* cutouts, const float* mm, const float* d_embeds, double* acc, hipStream_t s) override;
    int backward_b(const float* cutouts, const float* mm, const double* acc, float* g_cutouts, hipStream_t s) override;
};

VitFamily prx_vit_family_clip() {
    VitFamily f;
    f.patch_bias = 0; f.ln_pre = 1; f.eps = 1e-5f; f.act = PRX_ACT_QUICKGELU; f.dact = PRX_ACT_MUL_DQUICKGELU;
    f.norm = prx_patch_norm_clip(); f.head_dim = 64; f.mlp_width = 0;
    return f;
}

int prx_vit_create_impl(ImageTower** out, int res, int patch, int width, int layers, int heads, int out_dim, int max_n,
                        int precision, const float* const* w, int n_w, hipStream_t s, const VitFamily* family) {
    const VitFamily fam = family ? *family : prx_vit_family_clip();
    // weights ahead of the blocks: conv weight [, conv bias], class token, positions [, ln_pre gamma, beta]
    const int n_head = 3 + (fam.patch_bias ? 1 : 0) + (fam.ln_pre ? 2 : 0);
    PRX_REQUIRE(prec_valid(precision), "vit_create: unknown precision %d", precision);
    PRX_REQUIRE(n_w == n_head + 12 * layers + 3, "vit_create: expected %d weight tensors, got %d", n_head + 12 * layers + 3, n_w);
    const int hd = fam.head_dim > 0 ? fam.head_dim : 64;
    const int hp = prx_mha_head_cols(hd);
    PRX_REQUIRE(hp != 0, "vit_create: no attention kernel for a head dim of %d (16 | 32 | 64 run at 64 columns, 80 | 88 at 96, 104 at 128)", hd);
    PRX_REQUIRE(res % patch == 0 && width == heads * hd && width % 128 == 0 && width <= 2048,
                "vit_create: unsupported geometry (width %d, %d heads of %d; the width must be heads * head dim, a multiple of 128 and <= 2048)", width, heads, hd);
    const int MW = fam.mlp_width > 0 ? fam.mlp_width : 4 * width;
    PRX_REQUIRE(MW % 8 == 0, "vit_create: the MLP width %d must be a multiple of 8", MW);
    PRX_REQUIRE(fam.ln_pre || layers >= 1, "vit_create: a tower without ln_pre needs at least one block");
    PRX_REQUIRE(fam.eps > 0.f && fam.norm.std[0] > 0.f && fam.norm.std[1] > 0.f && fam.norm.std[2] > 0.f,
                "vit_create: LayerNorm eps and the channel std must be positive");
    const int G = res / patch;
    const int T = G * G + 1;
    PRX_REQUIRE(hp == 64 || T <= 640 || prec_is_f32(precision), "vit_create: heads of %d run on the %d-wide attention kernels, which take at most 640 tokens (got %d)", hd, hp, T);
    std::unique_ptr<PrxVit> guard(new PrxVit());      // a failed create frees what it allocated (DevArena)
    PrxVit* v = guard.get();
    DevArena& m = v->mem;
    const int f32 = prec_is_f32(precision);
    // the runner keeps one forward's activations for max_n cutouts, so a smaller max_batch is the way out of a failed allocation
    v->mem.describe("vit_create", ": the runner keeps one forward's activations for max_batch = %d cutouts of %d tokens (width %d, %d layers)",
                    max_n, T, width, layers);
    v->name = "vit"; v->T = T; v->max_n = max_n;
    v->res = res; v->patch = patch; v->width = width; v->layers = layers; v->heads = heads; v->out_dim = out_dim;
    v->set_precision(precision);
    v->fam = fam; v->bp = nullptr; v->hd = hd; v->hp = hp; v->aw = heads * hp; v->mlp = MW;
    const int AW = v->aw;
    // heads narrower than 64 reach the kernels as heads of 64 (folded below)
    v->att.T = T; v->att.heads = heads; v->att.hd = hd < 64 ? 64 : hd; v->att.C = AW; v->att.prec = precision;
    v->att.recompute = prx_mha_can_recompute(v->att);
    float *pad_w = nullptr, *pad_b = nullptr;       // fp32 staging of the padded qkv / out-projection weights, reused by every block (stream order)
    if (hd != 64) {
        DEV_ALLOC(m, alloc, pad_w, (size_t)3 * AW * width);
        DEV_ALLOC(m, alloc, pad_b, (size_t)3 * AW);
    }
    { const char* e = getenv("PRX_LEAN"); v->lean = (v->h16 && !(e && atoi(e) == 0)) ? 1 : 0; }
    { const char* e = getenv("PRX_VIT_CLS_TAIL"); v->cls_tail = (e && atoi(e) == 0) ? 0 : 1; }
    v->T = T; v->max_n = max_n; v->KP = (3 * patch * patch + 7) / 8 * 8; v->cur_n = 0;   // K padded to x8 (L/14: 588 -> 592)
    const int W = width, KP = v->KP;
    int r;
    {   // conv1.weight [W, 3*P*P] -> zero-padded to KP columns, both orientations
        const int K0 = 3 * patch * patch;
        float* padded;
        DEV_ALLOC(m, alloc, padded, (size_t)W * KP);
        PRX_CHECK_HIP(hipMemsetAsync(padded, 0, sizeof(float) * (size_t)W * KP, s));
        PRX_CHECK_HIP(hipMemcpy2DAsync(padded, sizeof(float) * KP, w[0], sizeof(float) * K0, sizeof(float) * K0, W,
                                       hipMemcpyDeviceToDevice, s));
        if ((r = prx_pack_pair(v->mem, &v->Wp, &v->WpT, padded, W, KP, v->prec, s))) return r;
    }
    const float* const* wh = w + 1;
    if (fam.patch_bias) { if ((r = v->mem.copy_f32(&v->bp, *wh++, W, s))) return r; }
    if ((r = v->mem.copy_f32(&v->cls, *wh++, W, s))) return r;
    if ((r = v->mem.copy_f32(&v->pos, *wh++, (size_t)T * W, s))) return r;
    v->lnpre_g = v->lnpre_b = nullptr;
    if (fam.ln_pre) {
        if ((r = v->mem.copy_f32(&v->lnpre_g, *wh++, W, s))) return r;
        if ((r = v->mem.copy_f32(&v->lnpre_b, *wh++, W, s))) return r;
    }
    v->L.resize(layers);
    const size_t R = (size_t)max_n * T;
    for (int l = 0; l < layers; ++l) {
        const float* const* q = w + n_head + 12 * l;
        VitLayer& y = v->L[l];
        if ((r = v->mem.copy_f32(&y.ln1_g, q[0], W, s))) return r;
        if ((r = v->mem.copy_f32(&y.ln1_b, q[1], W, s))) return r;
        if (hd == 64) {
            if ((r = prx_pack_pair(v->mem, &y.Wqkv, &y.WqkvT, q[2], 3 * W, W, v->prec, s))) return r;
            if ((r = v->mem.copy_f32(&y.bqkv, q[3], 3 * W, s))) return r;
            if ((r = prx_pack_pair(v->mem, &y.Wo, &y.WoT, q[4], W, W, v->prec, s))) return r;
        } else {
            if ((r = prx_vit_pad_head_rows(q[2], pad_w, heads, hd, hp, W, s))) return r;
            if ((r = prx_vit_pad_head_rows(q[3], pad_b, heads, hd, hp, 1, s))) return r;
            if (hp == 64) {      // the 64-wide kernels' softmax scale is fixed at 1 / sqrt(64)
                const float qs = sqrtf(64.f / (float)hd);
                if ((r = prx_vit_scale_f32(pad_w, (size_t)AW * W, qs, 256, s))) return r;
                if ((r = prx_vit_scale_f32(pad_b, (size_t)AW, qs, 1, s))) return r;
            }
            if ((r = prx_pack_pair(v->mem, &y.Wqkv, &y.WqkvT, pad_w, 3 * AW, W, v->prec, s))) return r;
            if ((r = v->mem.copy_f32(&y.bqkv, pad_b, 3 * AW, s))) return r;
            if ((r = prx_vit_pad_head_cols(q[4], pad_w, W, heads, hd, hp, s))) return r;
            if ((r = prx_pack_pair(v->mem, &y.Wo, &y.WoT, pad_w, W, AW, v->prec, s))) return r;
        }
        if ((r = v->mem.copy_f32(&y.bo, q[5], W, s))) return r;
        if ((r = v->mem.copy_f32(&y.ln2_g, q[6], W, s))) return r;
        if ((r = v->mem.copy_f32(&y.ln2_b, q[7], W, s))) return r;
        if ((r = prx_pack_pair(v->mem, &y.W1, &y.W1T, q[8], MW, W, v->prec, s))) return r;
        if ((r = v->mem.copy_f32(&y.b1, q[9], MW, s))) return r;
        if ((r = prx_pack_pair(v->mem, &y.W2, &y.W2T, q[10], W, MW, v->prec, s))) return r;
        if ((r = v->mem.copy_f32(&y.b2, q[11], W, s))) return r;
        if (v->lean) { DEV_ALLOC(m, alloc_op, y.x_in, R * W, f32); DEV_ALLOC(m, alloc_op, y.x_mid, R * W, f32); }
        else { float *a_, *b_; DEV_ALLOC(m, alloc, a_, R * W); DEV_ALLOC(m, alloc, b_, R * W); y.x_in = a_; y.x_mid = b_; }
        DEV_ALLOC(m, alloc, y.mean1, R); DEV_ALLOC(m, alloc, y.rstd1, R); DEV_ALLOC(m, alloc, y.mean2, R); DEV_ALLOC(m, alloc, y.rstd2, R);
        DEV_ALLOC(m, alloc_op, y.qkv, R * 3 * AW, f32); DEV_ALLOC(m, alloc_op, y.t, R * MW, f32);
        y.o_save = nullptr; y.lse = nullptr;
        if (prx_mha_saves_out(v->att)) { DEV_ALLOC(m, alloc_op, y.o_save, R * AW, f32); DEV_ALLOC(m, alloc, y.lse, (size_t)max_n * heads * T); }
    }
    const float* const* q = w + n_head + 12 * layers;
    if ((r = v->mem.copy_f32(&v->lnpost_g, q[0], W, s))) return r;
    if ((r = v->mem.copy_f32(&v->lnpost_b, q[1], W, s))) return r;
    // proj is [width, out]: forward Bt = proj^T [out, width]; dgrad Bt = proj [width, out]
    if ((r = prx_pack_pair(v->mem, &v->proj, &v->projT, q[2], W, out_dim, v->prec, s))) return r;
    DEV_ALLOC(m, alloc_op, v->A0, R * KP, f32); DEV_ALLOC(m, alloc_op, v->h, R * W, f32);
    DEV_ALLOC(m, alloc_op, v->att_o, R * AW, f32); DEV_ALLOC(m, alloc_op, v->u, R * MW, f32);
    DEV_ALLOC(m, alloc_op, v->hpost, (size_t)max_n * W, f32); DEV_ALLOC(m, alloc_op, v->de16, (size_t)max_n * out_dim, f32);
    DEV_ALLOC(m, alloc_op, v->dt, R * MW, f32); DEV_ALLOC(m, alloc_op, v->do_, R * AW, f32); DEV_ALLOC(m, alloc_op, v->dqkv, R * 3 * AW, f32);
    DEV_ALLOC(m, alloc, v->xpre, R * W); DEV_ALLOC(m, alloc, v->mean_pre, R); DEV_ALLOC(m, alloc, v->rstd_pre, R);
    if (v->lean) DEV_ALLOC(m, alloc_op, v->x_final, R * W, f32);
    else { float* a_; DEV_ALLOC(m, alloc, a_, R * W); v->x_final = a_; }
    DEV_ALLOC(m, alloc, v->mean_post, max_n); DEV_ALLOC(m, alloc, v->rstd_post, max_n); DEV_ALLOC(m, alloc, v->e, (size_t)max_n * out_dim);
    v->dx = v->dh = nullptr;
    if (!v->lean) { DEV_ALLOC(m, alloc, v->dx, R * W); DEV_ALLOC(m, alloc, v->dh, R * W); }
    DEV_ALLOC(m, alloc, v->dA0, R * KP); DEV_ALLOC(m, alloc, v->de, (size_t)max_n * out_dim);
    // bf16 twins of the fp32 gradient streams (the dgrad GEMMs' A operands); the exact mode reads the fp32 streams themselves;
    // in the lean layout they ARE the gradient streams
    if (v->f32) { v->dx_bf = v->dx; v->dh_bf = v->dh; }
    else { DEV_ALLOC(m, alloc_op, v->dx_bf, R * W, f32); DEV_ALLOC(m, alloc_op, v->dh_bf, R * W, f32); }
    DEV_ALLOC(m, alloc, v->dhpost, (size_t)max_n * W);
    if ((r = v->alloc_tail())) return r;
    *out = guard.release();
    return 0;
}

long long prx_vit_debug_dqkv_impl(ImageTower* h, void* dst, long long max_bytes, hipStream_t s) {
    const PrxVit* v = static_cast<const PrxVit*>(h);
    if (!v || v->cur_n < 1) return -1;
    const long long bytes = (long long)op_esz(v->f32) * v->cur_n * v->T * 3 * v->aw;
    if (bytes > max_bytes || hipMemcpyAsync(dst, v->dqkv, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) return -1;
    return bytes;
}

// LayerNorm whose output is a GEMM operand: bf16, or fp32 in the exact mode (the kernel has both outputs)
static int ln_op(PrxVit* v, const void* x, long long ldx, const float* g, const float* b, void* out, float* mean, float* rstd,
                 int rows, hipStream_t s) {
    return prx_layernorm_fwd(x, ldx, g, b, v->f32 ? nullptr : (bf16_t*)out, v->f32 ? (float*)out : nullptr, mean, rstd, rows,
                             v->width, v->fam.eps, s, v->h16, v->lean, 1);
}
// LayerNorm backward producing the fp32 gradient stream + its operand twin (the same buffer in the exact mode)
// `s16`: which of x (1), g (2), add (4) are 16-bit streams (the lean layout; dx is then null and dx_op the only output)
static int ln_bwd_op(PrxVit* v, const void* g, long long ldg, const void* x, long long ldx, const float* gamma, const float* mean,
                     const float* rstd, const void* add, long long ldadd, float* dx, long long lddx, void* dx_op, int rows,
                     hipStream_t s, int add_every = 0, int s16 = 0) {
    return prx_layernorm_bwd(g, ldg, x, ldx, gamma, mean, rstd, add, ldadd, dx, lddx, v->f32 ? nullptr : (bf16_t*)dx_op, lddx, rows,
                             v->width, s, v->h16, add_every, s16, 1);
}

int PrxVit::forward(const float* cutouts, int n, const float* mm, float* embeds, hipStream_t s) {
    PrxVit* const v = this;
    int r;
    if ((r = begin_forward(n))) return r;
    const int W = v->width, T = v->T, R = n * T, KP = v->KP, AW = v->aw, MW = v->mlp;
    if ((r = prx_patchify_fwd(cutouts, mm, v->A0, v->prec, n, v->res, v->patch, T, s, v->fam.norm))) return r;
    {   // conv1 (patch embed) as GEMM
        GemmDesc d; d.A = v->A0; d.lda = KP; d.B = v->Wp; d.ldb = KP; d.M = R; d.N = W; d.K = KP;
        d.bias_n = v->bp;
        d.out_f32 = v->xpre; d.ldc_f32 = W;
        if ((r = v->gemm(d, s))) return r;
    }
    const int lean = v->lean;
    MhaDesc mha = v->att; mha.N = n;
    void* x0 = v->layers > 0 ? v->L[0].x_in : v->x_final;
    if (v->fam.ln_pre) {
        if ((r = prx_vit_add_cls_pos(v->xpre, v->cls, v->pos, n, T, W, s))) return r;
        if ((r = prx_layernorm_fwd(v->xpre, W, v->lnpre_g, v->lnpre_b, lean ? (bf16_t*)x0 : nullptr, lean ? nullptr : (float*)x0, v->mean_pre,
                                   v->rstd_pre, R, W, v->fam.eps, s, v->h16, 0, 1))) return r;
    } else {
        if ((r = prx_vit_embed_tokens(v->xpre, v->cls, v->pos, x0, lean, n, T, W, s))) return r;
    }
    for (int l = 0; l < v->layers; ++l) {
        VitLayer& y = v->L[l];
        void* x_next = (l + 1 < v->layers) ? v->L[l + 1].x_in : v->x_final;
        if ((r = ln_op(v, y.x_in, W, y.ln1_g, y.ln1_b, v->h, y.mean1, y.rstd1, R, s))) return r;
        {   GemmDesc d; d.A = v->h; d.lda = W; d.B = y.Wqkv; d.ldb = W; d.M = R; d.N = 3 * AW; d.K = W;
            d.bias_n = y.bqkv; d.out_bf16 = y.qkv; d.ldc_bf16 = 3 * AW;
            if ((r = v->gemm(d, s))) return r; }
        void* att = prx_mha_saves_out(mha) ? y.o_save : v->att_o;
        if ((r = prx_mha_fwd(mha, y.qkv, att, y.lse, s))) return r;
        // the class-token tail: rows = the n class tokens, reached through a row stride of T * W in the token-major buffers;
        // LN / MLP intermediates of those rows are stored densely ([n][...]) at the start of their buffers
        const bool tail = v->cls_tail && l == v->layers - 1;
        const int rows = tail ? n : R;
        const int ldt = tail ? T * W : W;            // row stride of the token-major fp32 / 16-bit [R, W] buffers
        {   GemmDesc d; d.A = att; d.lda = tail ? T * AW : AW; d.B = y.Wo; d.ldb = AW; d.M = rows; d.N = W; d.K = AW;
            d.bias_n = y.bo; d.ldr = ldt;
            if (lean) { d.resid = (const float*)y.x_in; d.row16 = 1; d.out_bf16 = y.x_mid; d.ldc_bf16 = ldt; }
            else { d.resid = (const float*)y.x_in; d.out_f32 = (float*)y.x_mid; d.ldc_f32 = ldt; }
            if ((r = v->gemm(d, s))) return r; }
        if ((r = ln_op(v, y.x_mid, ldt, y.ln2_g, y.ln2_b, v->h, y.mean2, y.rstd2, rows, s))) return r;
        if ((r = linear_act(v->fam.act, v->h, W, y.W1, y.b1, y.t, v->u, rows, MW, W, s))) return r;
        {   GemmDesc d; d.A = v->u; d.lda = MW; d.B = y.W2; d.ldb = MW; d.M = rows; d.N = W; d.K = MW;
            d.bias_n = y.b2; d.ldr = ldt;
            if (lean) { d.resid = (const float*)y.x_mid; d.row16 = 1; d.out_bf16 = x_next; d.ldc_bf16 = ldt; }
            else { d.resid = (const float*)y.x_mid; d.out_f32 = (float*)x_next; d.ldc_f32 = ldt; }
            if ((r = v->gemm(d, s))) return r; }
    }
    // ln_post on the class token, projection, L2 normalisation (slip.py:66)
    if ((r = ln_op(v, v->x_final, (long long)T * W, v->lnpost_g, v->lnpost_b, v->hpost, v->mean_post, v->rstd_post, n, s))) return r;
    {   GemmDesc d; d.A = v->hpost; d.lda = W; d.B = v->projT; d.ldb = W; d.M = n; d.N = v->out_dim; d.K = W;
        d.out_f32 = v->e; d.ldc_f32 = v->out_dim;
        if ((r = v->gemm(d, s))) return r; }
    return head_fwd(embeds, n, s);
}

// Backward part A: from d(embeds) down to the patch-embed input gradient and the reduction the
// batch-global min/max renorm needs (acc[4] doubles, to be summed over ranks when the cutout
// batch is sharded).
int PrxVit::backward_a(const float* cutouts, const float* mm, const float* d_embeds, double* acc, hipStream_t s) {
    PrxVit* const v = this;
    int n, r;
    if ((r = backward_n(&n))) return r;
    const int W = v->width, T = v->T, R = n * T, KP = v->KP, AW = v->aw, MW = v->mlp;
    if ((r = head_bwd(d_embeds, n, s))) return r;
    {   GemmDesc d; d.A = v->de; d.a_is_f32 = 1; d.lda = v->out_dim; d.B = v->proj; d.ldb = v->out_dim;
        d.M = n; d.N = W; d.K = v->out_dim; d.out_f32 = v->dhpost; d.ldc_f32 = W;
        // half mode: the scaled d e leaves head_bwd as the half operand of this product too: a 16-bit A puts the M = n product on a
        // fit tile with K groups (6 us) instead of the register-staged 128 x 64 kernel on 12 workgroups (26 us)
        if (v->h16) { d.A = v->de16; d.a_is_f32 = 0; }
        if ((r = v->gemm(d, s))) return r; }
    // the residual-stream gradient is kept in fp32 (dx) with a bf16 twin (dx_bf) that feeds the dgrad GEMMs.  It enters the last
    // block on the class-token rows only; that block's kernels read those rows alone (the class-token tail) until its ln_1
    // backward, which takes the incoming gradient as zero on every other row (add_every = T) and writes all of them -- so the
    // streams need no clearing (two fills of 14.7 MB per iteration at the headline)
    const int lean = v->lean;
    MhaDesc mha = v->att; mha.N = n;
    if (v->layers == 0 || !v->cls_tail) PRX_CHECK_HIP(hipMemsetAsync(lean ? v->dx_bf : (void*)v->dx, 0, (lean ? sizeof(bf16_t) : sizeof(float)) * (size_t)R * W, s));
    // lean layout: dxs / dhs are the 16-bit gradient streams themselves (no fp32 copies exist)
    const void* dxs = lean ? v->dx_bf : (const void*)v->dx;
    const void* dhs = lean ? v->dh_bf : (const void*)v->dh;
    if ((r = ln_bwd_op(v, v->dhpost, W, v->x_final, (long long)T * W, v->lnpost_g, v->mean_post, v->rstd_post,
                       nullptr, 0, v->dx, (long long)T * W, v->dx_bf, n, s, 0, lean ? 1 : 0))) return r;
    for (int l = v->layers - 1; l >= 0; --l) {
        VitLayer& y = v->L[l];
        // the class-token tail (see the forward): the gradient entering the last block is non-zero on the class-token rows only
        const bool tail = v->cls_tail && l == v->layers - 1;
        const int rows = tail ? n : R;
        const int ldt = tail ? T * W : W;
        // MLP: x_next = x_mid + c_proj(act(c_fc(ln_2(x_mid)))), act = QuickGELU (CLIP) | GELU (SLIP)
        if ((r = linear_dact(v->fam.dact, v->dx_bf, ldt, y.W2T, y.t, v->dt, rows, MW, W, s))) return r;
        {   GemmDesc d; d.A = v->dt; d.lda = MW; d.B = y.W1T; d.ldb = MW; d.M = rows; d.N = W; d.K = MW;
            if (lean) { d.out_bf16 = v->dh_bf; d.ldc_bf16 = W; } else { d.out_f32 = v->dh; d.ldc_f32 = W; }
            if ((r = v->gemm(d, s))) return r; }
        if ((r = ln_bwd_op(v, dhs, W, y.x_mid, ldt, y.ln2_g, y.mean2, y.rstd2, dxs, ldt, v->dx, ldt, v->dx_bf, rows, s, 0, lean ? 7 : 0))) return r;
        // attention: x_mid = x_in + out_proj(mha(ln_1(x_in)))
        if (tail)       // d(attention output) is written on the class-token rows only: the other rows must read as zero
            PRX_CHECK_HIP(hipMemsetAsync(v->do_, 0, op_esz(v->f32) * (size_t)R * AW, s));
        {   GemmDesc d; d.A = v->dx_bf; d.lda = ldt; d.B = y.WoT; d.ldb = W; d.M = rows; d.N = AW; d.K = W;
            d.out_bf16 = v->do_; d.ldc_bf16 = tail ? T * AW : AW;
            if ((r = v->gemm(d, s))) return r; }
        if ((r = prx_mha_bwd(mha, y.qkv, y.o_save, v->do_, y.lse, v->dqkv, s))) return r;
        {   GemmDesc d; d.A = v->dqkv; d.lda = 3 * AW; d.B = y.WqkvT; d.ldb = 3 * AW; d.M = R; d.N = W; d.K = 3 * AW;
            if (lean) { d.out_bf16 = v->dh_bf; d.ldc_bf16 = W; } else { d.out_f32 = v->dh; d.ldc_f32 = W; }
            if ((r = v->gemm(d, s))) return r; }
        if ((r = ln_bwd_op(v, dhs, W, y.x_in, W, y.ln1_g, y.mean1, y.rstd1, dxs, W, v->dx, W, v->dx_bf, R, s, tail ? T : 0, lean ? 7 : 0))) return r;
    }
    // ln_pre backward (in place on dx), then patch-embed dgrad; without ln_pre the stream's gradient is the token gradient itself and
    // its operand twin (dx_bf, written by the first block's ln_1 backward) feeds the dgrad directly -- the bias takes no gradient
    // (frozen weights) and the class-token row of d(tokens) meets a zero row of A
    if (v->fam.ln_pre) { if ((r = ln_bwd_op(v, dxs, W, v->xpre, W, v->lnpre_g, v->mean_pre, v->rstd_pre, nullptr, 0, v->dh, W, v->dh_bf, R, s, 0, lean ? 2 : 0))) return r; }
    {   GemmDesc d; d.A = v->fam.ln_pre ? v->dh_bf : v->dx_bf; d.lda = W; d.B = v->WpT; d.ldb = W; d.M = R; d.N = KP; d.K = W;
        d.out_f32 = v->dA0; d.ldc_f32 = KP;
        if (v->h16) d.alpha_dev = v->gs + 1;      // ... and is unscaled (1/S) here, before the (rank-summed) renormalisation sums
        if ((r = v->gemm(d, s))) return r; }
    return prx_patchify_bwd_reduce(cutouts, mm, v->dA0, acc, n, v->res, v->patch, T, s, v->fam.norm);
}

int PrxVit::backward_b(const float* cutouts, const float* mm, const double* acc, float* g_cutouts, hipStream_t s) {
    int n;
    if (int r = backward_n(&n)) return r;
    return prx_patchify_bwd_apply(cutouts, mm, dA0, acc, g_cutouts, n, res, patch, T, s, fam.norm);
}
