#pragma once
// Built-in image filters (pixray filters/*.py) as HIP kernels.  Launchers; the C ABI (include/prx.h) forwards to them.
#include "plugin_common.h"
// wallpaper modes (prx.h PRX_WALL_*): 0 roll both axes (also `tiler`), 1 horizontal, 2 vertical, 3 shift
int plug_color_lookup(const float* x, int b, int c, int hw, const float* palette, int np, float beta, double* partials, float* out,
                      float* lgrad, float* loss, unsigned* ticket, hipStream_t s);
int plug_wallpaper_fwd(const float* x, int planes, int h, int w, int mode, int em, const int* shifts, double* partials, float* out,
                       float* loss, unsigned* ticket, hipStream_t s);
int plug_wallpaper_bwd(const float* x, const float* gout, int planes, int h, int w, int mode, int em, const int* shifts,
                       const float* gloss, float* grad, hipStream_t s);
