#pragma once
// Polygon-coverage rasteriser of the pixel drawer (pixray pixeldrawer.py).  Launchers; the C ABI (include/prx.h) forwards to them.
#include "common.h"

constexpr int PXR_TILE = 16;                    // tile edge in pixels (prx.h PRX_PIXEL_TILE)
constexpr int PXR_THREADS = PXR_TILE * PXR_TILE; // one pixel (its 2 x 2 samples) per lane
constexpr int PXR_MAXV = 8;                     // vertices per shape, padded (prx.h PRX_PIXEL_MAX_VERTS)
constexpr int PXR_CHUNK = 64;                   // shapes staged in LDS at a time; one coverage bit per shape and sample

int pxr_forward(const float* verts, const int* nverts, const float* colors, const int* tile_start, const int* tile_shapes, int w,
                int h, const int* seed, float* out, int* ids, hipStream_t s);
int pxr_backward(const float* verts, const int* nverts, const float* colors, const int* tile_start, const int* tile_shapes, int w,
                 int h, const int* seed, const float* gout, double* partials, const int* shape_start, const int* shape_entries,
                 int n_shapes, float* grad, hipStream_t s);
int pxr_sample_offsets(int w, int h, const int* seed, float* uv, hipStream_t s);
