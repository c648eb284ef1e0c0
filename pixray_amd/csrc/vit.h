#pragma once
#include "common.h"
#include "cutouts.h"
#include "attention.h"     // prx_mha_head_cols: the head dims VitFamily::head_dim may take
// What differs between the tower families this runner serves.  CLIP (clip.model.VisionTransformer): no patch-embed bias, ln_pre,
// eps 1e-5, QuickGELU, CLIP's preprocessing constants.  SLIP (timm VisionTransformer): a bias, no ln_pre, eps 1e-6, exact GELU,
// the ImageNet constants.
struct VitFamily {
    int patch_bias;     // the patch-embed convolution has a bias (bias_n epilogue of its product)
    int ln_pre;         // a LayerNorm between the token embedding and the first block
    float eps;          // every LayerNorm's eps
    int act, dact;      // PRX_ACT_* of the c_fc product and of its dgrad
    PatchNorm norm;     // channel mean / std of the fused preprocessing
    int head_dim;       // 0 / 64, or 32 / 16: narrower heads are zero-padded to 64 at weight-packing time (vit.hip PrxVit::hd);
                        // 80 | 88: zero-padded to 96, 104: to 128, the attention on the 96- / 128-wide instances of attention_kernels.h
    int mlp_width;      // hidden width of the MLP; 0 = 4 * width (OpenCLIP ViT-g-14: 6144 on 1408, ViT-bigG-14: 8192 on 1664)
};
VitFamily prx_vit_family_clip();
struct ImageTower;      // runner_core.h: the tower protocol the created handle is driven through
int prx_vit_create_impl(ImageTower** out, int res, int patch, int width, int layers, int heads, int out_dim, int max_n,
                        int precision, const float* const* w, int n_w, hipStream_t s, const VitFamily* family = nullptr);
long long prx_vit_debug_dqkv_impl(ImageTower* v, void* dst, long long max_bytes, hipStream_t s);   // a handle of this runner only
// launchers of the runner's own token-embedding / exact-mode activation kernels (the runner calls these; exported as prx_k_* for
// the kernel-level tests).  embed_tokens: `out` is IEEE half when out16, else fp32; scale_f32: x *= scale on `blocks` workgroups
int prx_vit_add_cls_pos(float* x, const float* cls, const float* pos, int N, int T, int W, hipStream_t s);
int prx_vit_embed_tokens(const float* x, const float* cls, const float* pos, void* out, int out16, int N, int T, int W, hipStream_t s);
int prx_vit_gelu_f32(const float* t, float* io, size_t n, int bwd, hipStream_t s);
int prx_vit_scale_f32(float* x, size_t n, float scale, int blocks, hipStream_t s);
// the head padding of the weight packs (fp32 device tensors): qkv rows [3 * heads * hd, row] -> [3 * heads * hp, row], out-projection
// input columns [W, heads * hd] -> [W, heads * hp]; the pad rows / columns are zero
int prx_vit_pad_head_rows(const float* src, float* dst, int heads, int hd, int hp, int row, hipStream_t s);
int prx_vit_pad_head_cols(const float* src, float* dst, int W, int heads, int hd, int hp, hipStream_t s);
