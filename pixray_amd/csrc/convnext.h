// OpenCLIP ConvNeXt visual tower runner (convnext_base ... convnext_xxlarge); see convnext.hip.
#pragma once
#include "common.h"

struct ImageTower;      // runner_core.h: the tower protocol the created handle is driven through
int prx_convnext_create_impl(ImageTower** out, int res, const int* depths, const int* dims, int out_dim, int proj_mlp, float ln_eps,
                             int max_n, int precision, const float* const* w, int n_w, hipStream_t s);
// One host launcher per runner-private kernel (the runner calls these; csrc/api_kernels.hip exports them as prx_k_cnx_* for the
// kernel-level tests).  Maps are NHWC [N][H][W][C]; `prec` = PRX_PREC_* is the element type of the `void*` buffers; C % 8 == 0.
// pack: the depthwise weight [C][7*7] (fp32) as [2][49][C] in the operand format -- the taps channel-contiguous, then the same with
// the taps flipped (the data gradient's stencil)
int prx_cnx_pack_dw(const float* w, void* pack, int C, int prec, hipStream_t s);
// out = dwconv7x7(x, pad 3) [+ bias[c]] [+ add], taps from pack[flip]; fp32 accumulation in the fixed order kx-major, ky-minor.
// out_op (operand format) and / or out_f32; add: fp32 [N][H][W][C] (may be out_f32 itself)
int prx_cnx_dwconv(const void* x, const void* pack, const float* bias, const float* add, void* out_op, float* out_f32, int N, int H,
                   int W, int C, int flip, int prec, hipStream_t s);
// [N][H][W][C] -> [N][H/2][W/2][4C], output channel (dy * 2 + dx) * C + c = input pixel (2 oy + dy, 2 ox + dx) channel c; and back
int prx_cnx_space_to_depth(const void* in, void* out, int N, int H, int W, int C, int prec, hipStream_t s);
int prx_cnx_depth_to_space(const void* in, void* out, int N, int H, int W, int C, int prec, hipStream_t s);
// [N][HW][C] -> fp32 [N][C] (the mean over HW), and the broadcast of g / HW back: fp32 and / or operand-format output
int prx_cnx_avgpool_fwd(const void* x, float* out, int N, int HW, int C, int prec, hipStream_t s);
int prx_cnx_avgpool_bwd(const float* g, float* dx_f32, void* dx_op, int N, int HW, int C, int prec, hipStream_t s);
// LayerNorm over the channels of `rows` pixels, any C % 8 == 0 (the engine's LayerNorm takes multiples of 128 / 256 only).  x is fp32
// (x_f32 != 0) or in the operand format.  group > 0: x (and the backward's outputs) live in a patch-embed layout with one unused
// leading row per `group` rows (row r of the map is row r + r / group + 1 there: the stem).
int prx_cnx_layernorm_fwd(const void* x, int x_f32, const float* gamma, const float* beta, void* out_op, float* out_f32, float* mean,
                          float* rstd, int rows, int C, float eps, int group, int prec, hipStream_t s);
int prx_cnx_layernorm_bwd(const float* g, const void* x, int x_f32, const float* gamma, const float* mean, const float* rstd,
                          void* dx_op, float* dx_f32, int rows, int C, int group, int prec, hipStream_t s);
