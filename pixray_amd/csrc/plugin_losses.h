#pragma once
// Built-in custom losses (pixray Losses/*.py) as HIP kernels.  Launchers; the C ABI (include/prx.h) forwards to them.
#include "plugin_common.h"
int plug_saturation_fwd(const float* x, int n, int hw, float weight, double* partials, double* stats, float* loss, unsigned* ticket, hipStream_t s);
int plug_saturation_bwd(const float* x, int n, int hw, float weight, const double* stats, const float* gout, float* grad, hipStream_t s);
int plug_symmetry(const float* x, int planes, int h, int w, float weight, double* partials, float* grad, float* loss, unsigned* ticket, hipStream_t s);
int plug_edge(const float* x, int planes, int h, int w, float r, float g, float b, int left, int right, int upper, int lower,
              float inv_l, float inv_r, float inv_u, float inv_d, float inv_all, float edge_weight, double* partials, float* grad,
              float* loss, unsigned* ticket, hipStream_t s);
int plug_edge_target(const float* x, int planes, int h, int w, const float* target, float r, float g, float b, const float* mask,
                     int left, int right, int upper, int lower, float inv_l, float inv_r, float inv_u, float inv_d, float inv_mask,
                     float inv_all, float edge_weight, double* partials, float* grad, float* loss, unsigned* ticket, hipStream_t s);
int plug_gaussian(const float* x, int planes, int h, int w, const float* gy, const float* gx, float r, float g, float b, float scale,
                  double* partials, float* grad, float* loss, unsigned* ticket, hipStream_t s);
int plug_aesthetic(const float* embeds, int n, int d, const float* w, float bias, float target, double* partials, float* grad, float* loss,
                   unsigned* ticket, hipStream_t s);
int plug_palette(const float* x, int n, int hw, const float* palette, int np, float scale, double* partials, float* grad, float* loss,
                 unsigned* ticket, hipStream_t s);
int plug_smoothness_fwd(const float* x, int n, int h, int w, int type, int edge_order, float spacing, float weight, double* partials,
                        float* tfac, float* loss, unsigned* ticket, hipStream_t s);
int plug_smoothness_bwd(const float* tfac, const float* x, int n, int h, int w, int edge_order, float spacing, float weight,
                        const float* gout, float* grad, hipStream_t s);
int plug_blur_fwd(const float* x, int planes, int h, int w, const float* taps, int k, float* y, hipStream_t s);
int plug_blur_bwd(const float* gy, int planes, int h, int w, const float* taps, int k, float* gx, hipStream_t s);
