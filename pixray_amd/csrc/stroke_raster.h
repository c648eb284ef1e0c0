#pragma once
// Stroke rasteriser of the line_sketch and clipdraw drawers (pixray linedrawer.py / clipdrawer.py).  Launchers; the C ABI
// (include/prx.h) forwards to them.
#include "common.h"

constexpr int STR_TILE = 16;                      // tile edge in pixels (prx.h PRX_STROKE_TILE)
constexpr int STR_THREADS = STR_TILE * STR_TILE;  // one pixel (its 2 x 2 samples) per lane
constexpr int STR_MAX_SEGS = 64;                  // cubic segments per path: one bit each in the backward's segment masks
constexpr int STR_MAX_POINTS = 1 + 3 * STR_MAX_SEGS;   // prx.h PRX_STROKE_MAX_POINTS
constexpr int STR_MAX_SLOT = 2 * STR_MAX_POINTS + 5;   // per-path gradient values: points (x, y), width, RGBA
constexpr int STR_CHUNK = 16;                     // layers whose per-sample coverage the backward keeps in LDS at a time
constexpr int STR_TSTEPS = 32;                    // closest point: t = i / 32 for i = 0 .. 32, then Newton
constexpr int STR_NEWTON = 5;

int str_forward(const float* points, const int* path_start, int n_paths, int max_points, const float* widths, const float* colors,
                const float* paper, int w, int h, const int* seed, float* boxes, int* tile_count, int* tile_paths, float* out,
                hipStream_t s);
int str_backward(const float* points, const int* path_start, int n_paths, int max_points, const float* widths, const float* colors,
                 const float* paper, int w, int h, const int* seed, const float* gout, float* boxes, int* tile_count,
                 int* tile_paths, double* partials, double* paper_partials, float* grad_points, float* grad_widths,
                 float* grad_colors, float* grad_paper, hipStream_t s);
int str_sample_offsets(int w, int h, const int* seed, float* uv, hipStream_t s);
