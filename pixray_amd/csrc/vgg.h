// VGG16 feature extractor of the StyleLoss plugin (reference Losses/StyleLoss.py:24-47) on the MFMA
// implicit-GEMM engine.  See vgg.hip.
#pragma once
#include "common.h"

struct PrxVgg16;
int prx_vgg16_create_impl(PrxVgg16** out, const float* const* weights, int n_weights, int max_h, int max_w, int precision, hipStream_t s);
void prx_vgg16_destroy_impl(PrxVgg16* v);
long long prx_vgg16_workspace_bytes_impl(int H, int W, int precision);
int prx_vgg16_feature_shape_impl(int H, int W, int k, int* h, int* w, int* c);
int prx_vgg16_forward_impl(PrxVgg16* v, const float* x, int H, int W, void* workspace, float* const* feats, hipStream_t s);
int prx_vgg16_backward_impl(PrxVgg16* v, int H, int W, const void* workspace, const float* const* g_feats, float* g_x, hipStream_t s);
// One host launcher per runner-private kernel (grid computation, operand-type dispatch on `prec` = PRX_PREC_*): the runner calls
// these, csrc/api_kernels.hip exports them as prx_k_* for the kernel-level tests.
int prx_vgg_input(const float* x, void* out, int HW, int prec, hipStream_t s);
int prx_vgg_input_grad(const float* d, float* gx, int HW, const float* unscale, hipStream_t s);
int prx_vgg_maxpool(const void* x, void* out, unsigned char* arg, int H, int W, int C, int prec, hipStream_t s);
int prx_vgg_combine(const float* above, const unsigned char* arg, const float* gcap, const void* act, void* gpre, int H, int W, int C,
                    const float* gscale, int prec, hipStream_t s);
