// CLIP ModifiedResNet visual tower runner (RN50x4 of BASELINE.json configs[2]); see resnet.hip.
#pragma once
#include "common.h"

struct ImageTower;      // runner_core.h: the tower protocol the created handle is driven through
int prx_resnet_create_impl(ImageTower** out, int res, int width, const int* layers, int heads, int out_dim, int max_n,
                           int precision, const float* const* w, int n_w, hipStream_t s);
// One host launcher per runner-private kernel: grid computation and the operand-type (`prec` = PRX_PREC_*) / CO dispatch.  The runner
// calls these; csrc/api_kernels.hip exports them as prx_k_* for the kernel-level tests.  Operand-format buffers are `void*`.
// CO = width / 2, one of 8, 16, 32, 40, 48, 64 (anything else is refused)
int prx_stem1_fwd(const float* cut, const float* mm, const float* w, const float* b, void* out, int N, int S, int CO, int prec,
                  hipStream_t s);
int prx_stem1_bwd(const void* g, const float* w, float* dY, int N, int S, int CO, const float* oscale_dev, int prec, hipStream_t s);
int prx_avgpool2_fwd(const void* x, void* out, int N, int H, int W, int C, int prec, hipStream_t s);
int prx_avgpool2_bwd(const float* g, const void* mask, float* dx_f32, void* dx_op, int N, int H, int W, int C, int prec, hipStream_t s);
int prx_relu_mask(float* g, const void* out, void* g_op, size_t n, int prec, hipStream_t s);
int prx_tokens_fwd(const float* x, const float* pos, void* t, int N, int P, int C, int prec, hipStream_t s);
int prx_tokens_bwd(const float* dt, float* dx, int N, int P, int C, int prec, hipStream_t s);
int prx_tok0_gather(const void* t, void* out, int N, int T, int C, int prec, hipStream_t s);
int prx_tok0_scatter(const void* g0, void* dt, int N, int T, int C, int prec, hipStream_t s);
