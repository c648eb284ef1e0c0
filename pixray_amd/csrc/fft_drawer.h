#pragma once
// The fft drawer's private kernels (fft_drawer.hip), one host launcher each.  prx_fft_drawer_synth / _backward call these, and
// csrc/api_kernels.hip exports them as prx_k_fft_* for the kernel-level tests, so the launch code under test is the product's.
#include "common.h"
#include <algorithm>

inline int fft_up4(int v) { return (v + 3) & ~3; }
// the padded geometry of a W x H canvas: every row stride is a multiple of 4 floats (the engine's 16-byte operand chunks)
struct FftGeom {
    int W, H;
    int Wh;        // W / 2 + 1 frequency columns of the real transform
    int Wf;        // columns of the spectrum tensor: Wh, + 1 surplus column (the lucid frequency helper's) for an odd width
    int HP, HP2;   // up4(H), up4(2 H)
    int WP;        // up4(W)
    int K1p;       // up4(2 Wh): the (v, part) contraction of the first GEMM
};
inline FftGeom fft_geom(int W, int H) {
    FftGeom g;
    g.W = W; g.H = H;
    g.Wh = W / 2 + 1;
    g.Wf = W / 2 + (W % 2 ? 2 : 1);
    g.HP = fft_up4(H); g.HP2 = fft_up4(2 * H); g.WP = fft_up4(W); g.K1p = fft_up4(2 * g.Wh);
    return g;
}
// grid of a grid-stride elementwise kernel: at most 8192 workgroups of 256
inline int fft_grid(size_t total) { return (int)std::min<size_t>((total + 255) / 256, 8192); }
constexpr int FFT_MOM_BLOCKS = 1024;
// workgroups of fft_moments_kernel over n elements; `part` holds 3 doubles for each
inline int fft_moment_blocks(size_t n) { return std::min(fft_grid(n), FFT_MOM_BLOCKS); }

// params [3][H][Wf][2], scale [H][Wh] -> bt1 [3 HP2][K1p], zero padded
int prx_fft_pack(const float* params, const float* scale, float* bt1, int W, int H, hipStream_t s);
// dP [3 HP2][K1p], scale [H][Wh] -> g_params [3][H][Wf][2]
int prx_fft_unpack(const float* dP, const float* scale, float* g_params, int W, int H, hipStream_t s);
// acc[0..2] = sum x, sum x^2, sum x y (0 without y) over n elements in double, fixed order; part: 3 * fft_moment_blocks(n) doubles
int prx_fft_moments(const float* x, const float* y, size_t n, double* part, double* acc, hipStream_t s);
// x [3][H][W], acc (its sums), cm [3][3] -> rgb [3][H][W]
int prx_fft_tail_fwd(const float* x, const double* acc, float contrast, const float* cm, float* rgb, int W, int H, hipStream_t s);
// x, g [3][H][W] -> gy [3][H][W]
int prx_fft_tail_bwd_gy(const float* x, const float* g, const double* acc, float contrast, const float* cm, float* gy, int W, int H,
                        hipStream_t s);
// x, gy [3][H][W], acc (sums of x), bacc (sums of gy; bacc[2] = sum gy x) -> dxT [3][W][HP]
int prx_fft_tail_bwd_dx(const float* x, const float* gy, const double* acc, const double* bacc, float contrast, float* dxT, int W, int H,
                        hipStream_t s);
