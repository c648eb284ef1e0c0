// OpenCLIP ConvNeXt visual tower runner (timm ConvNeXt trunk + open_clip head [UPSTREAM timm convnext.py, open_clip timm_model.py;
// neither is installed: restated from the published sources, parity unpinned]): forward and activation-gradient backward.
//   stem   Conv2d(3, d0, 4, stride 4) = patchify (P = 4, the fused min/max renormalisation + Normalize of cutouts.hip) + one product,
//          LayerNorm over the channels
//   stage  [LayerNorm, Conv2d(2, stride 2) = space-to-depth + one product with K = 4C]  then `depth` blocks
//   block  x + fc2'(gelu(fc1(LayerNorm(dwconv7x7(x)))))     fc2' = diag(gamma) fc2, folded on the host (weights.py)
//   head   mean over H x W, LayerNorm, projection (linear | fc1, GELU, fc2), L2 normalisation
// New here: the depthwise 7x7 stencil and its data gradient (one kernel template), the 2x2 space-to-depth permutation and its
// inverse, the global average pool pair, and a LayerNorm over any channel count that is a multiple of 8 (the engine's takes multiples
// of 128 / 256 up to 2048: the towers have 192, 384 x 8 = 3072, the reduced ones 64 and 96).  Both MLP products with GELU / GELU' in
// the epilogue, the residual epilogue, the downsample / stem / head products run on the GEMM engine.
// The residual stream is fp32 with a twin in the operand format (the stencil's input, and the dgrad products' A); the weights are
// frozen, so a block's input is not kept: the backward needs the stencil's output y (the LayerNorm input) and the GELU
// pre-activation t only.
#include "convnext.h"
#include "gemm.h"
#include "cutouts.h"
#include "prompt_vq.h"
#include "elementwise.h"
#include "weight_pack.h"
#include "runner_core.h"
#include <vector>
#include <memory>

namespace {

// ---- depthwise 7x7 ------------------------------------------------------------------------------------------------------
// A 256-lane workgroup owns an 8 x 16 tile of output pixels and a slab of 8 lanes x 16 bytes of channels (64 channels of a
// 16-bit map, 32 of an fp32 one).  The (8 + 6) x (16 + 6) input pixels of the slab are fetched ONCE, 16 bytes per lane (a pixel's
// slab is 128 contiguous bytes), into LDS with zeros outside the map: every halo re-read, and every border, is an LDS read.  The
// slab's 49 taps sit beside it.  Lane (pixel lane p, channel lane c) then produces a column strip of 4 vertically adjacent
// outputs: per filter column kx it holds the 7 taps of that column in registers and walks the 10 input rows of the strip, each
// LDS vector feeding up to 4 accumulators -- 70 + 49 LDS vectors for 4 outputs instead of 4 x 98.  Wave-wide the x reads are 8
// adjacent pixels x 128 bytes = 1 KiB contiguous (conflict-free ds_read_b128), the tap reads a broadcast.
// Accumulation is fp32, per output in the fixed order kx = 0..6 outer, ky = 0..6 inner; out-of-map taps add an exact zero product.
constexpr int CNX_TH = 8, CNX_TW = 16, CNX_CL = 8, CNX_STRIP = 4;
constexpr int CNX_IH = CNX_TH + 6, CNX_IW = CNX_TW + 6;

template <typename T>
__global__ __launch_bounds__(256) void cnx_dwconv_kernel(const T* __restrict__ x, const T* __restrict__ taps,
                                                         const float* __restrict__ bias, const float* add, T* out_op, float* out_f32,
                                                         int H, int W, int C, int tiles_x) {
    constexpr int VEC = 16 / (int)sizeof(T);
    typedef T vec_t __attribute__((ext_vector_type(VEC)));
    __shared__ vec_t s_x[CNX_IH * CNX_IW * CNX_CL];
    __shared__ vec_t s_w[49 * CNX_CL];
    const int tid = threadIdx.x, cl = tid & (CNX_CL - 1), pl = tid >> 3;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * CNX_TH, x0 = tx * CNX_TW, n = blockIdx.z;
    const int c = (blockIdx.y * CNX_CL + cl) * VEC;
    const bool c_ok = c < C;
    vec_t zero;
#pragma unroll
    for (int e = 0; e < VEC; ++e) zero[e] = (T)0.f;
    for (int p = pl; p < CNX_IH * CNX_IW; p += 32) {
        const int iy = p / CNX_IW, ix = p - iy * CNX_IW;
        const int gy = y0 - 3 + iy, gx = x0 - 3 + ix;
        vec_t v = zero;
        if (c_ok && gy >= 0 && gy < H && gx >= 0 && gx < W)
            v = *reinterpret_cast<const vec_t*>(x + ((unsigned)((n * H + gy) * W + gx) * (unsigned)C + (unsigned)c));
        s_x[p * CNX_CL + cl] = v;
    }
    for (int t = pl; t < 49; t += 32) s_w[t * CNX_CL + cl] = c_ok ? *reinterpret_cast<const vec_t*>(taps + t * C + c) : zero;
    __syncthreads();
    const int col = pl & (CNX_TW - 1), r0 = (pl >> 4) * CNX_STRIP;
    float acc[CNX_STRIP][VEC];
#pragma unroll
    for (int j = 0; j < CNX_STRIP; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[j][e] = 0.f;
#pragma unroll 1       // one filter column at a time: unrolled, the 70 LDS vectors and 49 taps of all seven are hoisted together and spill
    for (int kx = 0; kx < 7; ++kx) {
        float w[7][VEC];
#pragma unroll
        for (int ky = 0; ky < 7; ++ky) {
            const vec_t t = s_w[(ky * 7 + kx) * CNX_CL + cl];
#pragma unroll
            for (int e = 0; e < VEC; ++e) w[ky][e] = (float)t[e];
        }
#pragma unroll
        for (int iy = 0; iy < CNX_STRIP + 6; ++iy) {
            const vec_t xv = s_x[((r0 + iy) * CNX_IW + col + kx) * CNX_CL + cl];
            float xf[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) xf[e] = (float)xv[e];
#pragma unroll
            for (int j = 0; j < CNX_STRIP; ++j) {
                const int ky = iy - j;
                if (ky >= 0 && ky < 7) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) acc[j][e] = fmaf(xf[e], w[ky][e], acc[j][e]);
                }
            }
        }
    }
    const int gx = x0 + col;
    if (!c_ok || gx >= W) return;
    float b[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) b[e] = 0.f;
    if (bias) {
#pragma unroll
        for (int q = 0; q < VEC; q += 4) {
            const float4 t = *reinterpret_cast<const float4*>(bias + c + q);
            b[q] = t.x; b[q + 1] = t.y; b[q + 2] = t.z; b[q + 3] = t.w;
        }
    }
#pragma unroll
    for (int j = 0; j < CNX_STRIP; ++j) {
        const int gy = y0 + r0 + j;
        if (gy >= H) continue;
        const unsigned o = (unsigned)((n * H + gy) * W + gx) * (unsigned)C + (unsigned)c;
        float v[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = acc[j][e] + b[e];
        if (add) {
#pragma unroll
            for (int q = 0; q < VEC; q += 4) {
                const float4 t = *reinterpret_cast<const float4*>(add + o + q);
                v[q] += t.x; v[q + 1] += t.y; v[q + 2] += t.z; v[q + 3] += t.w;
            }
        }
        if (out_f32) {
#pragma unroll
            for (int q = 0; q < VEC; q += 4) *reinterpret_cast<float4*>(out_f32 + o + q) = make_float4(v[q], v[q + 1], v[q + 2], v[q + 3]);
        }
        if (out_op) {
            vec_t r;
#pragma unroll
            for (int e = 0; e < VEC; ++e) r[e] = op_cvt<T>(v[e]);
            *reinterpret_cast<vec_t*>(out_op + o) = r;
        }
    }
}

// pack[0][t][c] = w[c][t], pack[1][t][c] = w[c][48 - t]
template <typename T>
__global__ __launch_bounds__(256) void cnx_pack_dw_kernel(const float* __restrict__ w, T* __restrict__ pack, int C) {
    const int total = 2 * 49 * C;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int c = i % C, t = (i / C) % 49, f = i / (49 * C);
        pack[i] = op_cvt<T>(w[c * 49 + (f ? 48 - t : t)]);
    }
}

// ---- space-to-depth 2x2 and its inverse, in 16-byte chunks (CP chunks per input pixel) -------------------------------------------
template <bool INVERSE>
__global__ __launch_bounds__(256) void cnx_s2d_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, int N, int H, int W, int CP) {
    const int Wo = W >> 1, Ho = H >> 1;
    const size_t total = (size_t)N * H * W * CP;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int k = (int)(i % (size_t)(4 * CP));
        const size_t opix = i / (size_t)(4 * CP);
        const int q = k / CP, cc = k - q * CP;
        const int ox = (int)(opix % Wo), oy = (int)((opix / Wo) % Ho), n = (int)(opix / ((size_t)Wo * Ho));
        const size_t j = (((size_t)n * H + 2 * oy + (q >> 1)) * W + 2 * ox + (q & 1)) * CP + cc;      // index in the [N][H][W][C] map
        if (INVERSE) dst[j] = src[i];
        else dst[i] = src[j];
    }
}

// ---- global average pool ---------------------------------------------------------------------------------------------------
// one lane per (n, c): HW terms in their order, accumulated in double (the sum's own rounding stays below the fp32 result's)
template <typename T>
__global__ __launch_bounds__(256) void cnx_avgpool_fwd_kernel(const T* __restrict__ x, float* __restrict__ out, int N, int HW, int C) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * C) return;
    const int n = i / C, c = i - n * C;
    const T* p = x + (size_t)n * HW * C + c;
    double s = 0.0;
    for (int k = 0; k < HW; ++k) s += (double)(float)p[(size_t)k * C];
    out[i] = (float)(s / (double)HW);
}
template <typename T>
__global__ __launch_bounds__(256) void cnx_avgpool_bwd_kernel(const float* __restrict__ g, float* __restrict__ dx_f32, T* __restrict__ dx_op,
                                                              int N, int HW, int C, float inv) {
    const int C4 = C >> 2;
    const size_t total = (size_t)N * HW * C4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        const int n = (int)(i / ((size_t)HW * C4));
        const float4 t = *reinterpret_cast<const float4*>(g + (size_t)n * C + 4 * c4);
        const float a = t.x * inv, b = t.y * inv, c = t.z * inv, d = t.w * inv;
        if (dx_f32) *reinterpret_cast<float4*>(dx_f32 + i * 4) = make_float4(a, b, c, d);
        if (dx_op) op_st4(dx_op, i * 4, a, b, c, d);
    }
}

// ---- LayerNorm over the channels, one wave per pixel -----------------------------------------------------------------------
__device__ __forceinline__ size_t cnx_row(int r, int group) { return group > 0 ? (size_t)r + r / group + 1 : (size_t)r; }

template <typename TX, typename TO>
__global__ __launch_bounds__(256) void cnx_ln_fwd_kernel(const TX* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         TO* __restrict__ out_op, float* __restrict__ out_f32, float* __restrict__ mean,
                                                         float* __restrict__ rstd, int rows, int C, float eps, int group) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const TX* xp = x + cnx_row(r, group) * C;
    float s = 0.f;
    for (int i = lane * 4; i < C; i += 256) { const float4 v = op_ld4v(xp, i); s += (v.x + v.y) + (v.z + v.w); }
    const float m = wave_sum(s) / (float)C;
    float q = 0.f;
    for (int i = lane * 4; i < C; i += 256) {
        const float4 v = op_ld4v(xp, i);
        const float a = v.x - m, b = v.y - m, c = v.z - m, d = v.w - m;
        q += (a * a + b * b) + (c * c + d * d);
    }
    const float rs = 1.f / sqrtf(wave_sum(q) / (float)C + eps);
    for (int i = lane * 4; i < C; i += 256) {
        const float4 v = op_ld4v(xp, i);
        const float4 g = *reinterpret_cast<const float4*>(gamma + i), bt = *reinterpret_cast<const float4*>(beta + i);
        const float a = (v.x - m) * rs * g.x + bt.x, b = (v.y - m) * rs * g.y + bt.y, c = (v.z - m) * rs * g.z + bt.z, d = (v.w - m) * rs * g.w + bt.w;
        if (out_f32) *reinterpret_cast<float4*>(out_f32 + (size_t)r * C + i) = make_float4(a, b, c, d);
        if (out_op) op_st4(out_op, (size_t)r * C + i, a, b, c, d);
    }
    if (lane == 0) { mean[r] = m; rstd[r] = rs; }
}

// dx = rstd * (g gamma - mean(g gamma) - xhat mean(g gamma xhat))
template <typename TX, typename TO>
__global__ __launch_bounds__(256) void cnx_ln_bwd_kernel(const float* __restrict__ g, const TX* __restrict__ x, const float* __restrict__ gamma,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd, TO* __restrict__ dx_op,
                                                         float* __restrict__ dx_f32, int rows, int C, int group) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const size_t ro = cnx_row(r, group) * C;
    const TX* xp = x + ro;
    const float* gp = g + (size_t)r * C;
    const float m = mean[r], rs = rstd[r];
    float s1 = 0.f, s2 = 0.f;
    for (int i = lane * 4; i < C; i += 256) {
        const float4 v = op_ld4v(xp, i), gv = *reinterpret_cast<const float4*>(gp + i), ga = *reinterpret_cast<const float4*>(gamma + i);
        const float g0 = gv.x * ga.x, g1 = gv.y * ga.y, g2 = gv.z * ga.z, g3 = gv.w * ga.w;
        s1 += (g0 + g1) + (g2 + g3);
        s2 += (g0 * ((v.x - m) * rs) + g1 * ((v.y - m) * rs)) + (g2 * ((v.z - m) * rs) + g3 * ((v.w - m) * rs));
    }
    const float m1 = wave_sum(s1) / (float)C, m2 = wave_sum(s2) / (float)C;
    for (int i = lane * 4; i < C; i += 256) {
        const float4 v = op_ld4v(xp, i), gv = *reinterpret_cast<const float4*>(gp + i), ga = *reinterpret_cast<const float4*>(gamma + i);
        const float a = rs * (gv.x * ga.x - m1 - (v.x - m) * rs * m2), b = rs * (gv.y * ga.y - m1 - (v.y - m) * rs * m2);
        const float c = rs * (gv.z * ga.z - m1 - (v.z - m) * rs * m2), d = rs * (gv.w * ga.w - m1 - (v.w - m) * rs * m2);
        if (dx_f32) *reinterpret_cast<float4*>(dx_f32 + ro + i) = make_float4(a, b, c, d);
        if (dx_op) op_st4(dx_op, ro + i, a, b, c, d);
    }
}

int stream_grid(size_t total) { return (int)std::min<size_t>((total + 255) / 256, 4096); }

}  // namespace

// ---- launchers (convnext.h) ---------------------------------------------------------------------------------------------------
static int cnx_check_map(const char* who, int N, int H, int W, int C) {
    PRX_REQUIRE(N >= 1 && H >= 1 && W >= 1 && C >= 8, "%s: bad map %d x %d x %d x %d", who, N, H, W, C);
    PRX_REQUIRE(C % 8 == 0, "%s: the channel count must be a multiple of 8 (C=%d)", who, C);
    PRX_REQUIRE((unsigned long long)N * H * W * C < (1ull << 31), "%s: %d x %d x %d x %d elements exceed the 32-bit index range", who, N, H, W, C);
    return 0;
}

int prx_cnx_pack_dw(const float* w, void* pack, int C, int prec, hipStream_t s) {
    PRX_REQUIRE(prec_valid(prec) && C >= 8 && C % 8 == 0, "cnx_pack_dw: the channel count must be a multiple of 8 (C=%d)", C);
    PRX_OP_DISPATCH(prec_is_f32(prec), prec_is_h16(prec), T,
                    hipLaunchKernelGGL(cnx_pack_dw_kernel<T>, dim3(stream_grid((size_t)98 * C)), dim3(256), 0, s, w, (T*)pack, C));
    PRX_LAUNCH_CHECK();
    return 0;
}

int prx_cnx_dwconv(const void* x, const void* pack, const float* bias, const float* add, void* out_op, float* out_f32, int N, int H,
                   int W, int C, int flip, int prec, hipStream_t s) {
    if (int r = cnx_check_map("cnx_dwconv", N, H, W, C)) return r;
    PRX_REQUIRE(prec_valid(prec) && (out_op || out_f32), "cnx_dwconv: unknown precision %d, or no output", prec);
    PRX_REQUIRE(N <= 65535, "cnx_dwconv: at most 65535 maps per launch (N=%d)", N);
    const int f32 = prec_is_f32(prec);
    const int slab = CNX_CL * (f32 ? 4 : 8);
    const int tiles_x = ceil_div(W, CNX_TW), tiles_y = ceil_div(H, CNX_TH);
    const dim3 grid(tiles_x * tiles_y, ceil_div(C, slab), N);
    const void* taps = op_off(pack, flip ? (size_t)49 * C : 0, f32);
    PRX_OP_DISPATCH(f32, prec_is_h16(prec), T,
                    hipLaunchKernelGGL(cnx_dwconv_kernel<T>, grid, dim3(256), 0, s, (const T*)x, (const T*)taps, bias, add, (T*)out_op,
                                       out_f32, H, W, C, tiles_x));
    PRX_LAUNCH_CHECK();
    return 0;
}

static int cnx_s2d(const void* src, void* dst, int N, int H, int W, int C, int prec, bool inverse, hipStream_t s) {
    const char* who = inverse ? "cnx_depth_to_space" : "cnx_space_to_depth";
    if (int r = cnx_check_map(who, N, H, W, C)) return r;
    PRX_REQUIRE(prec_valid(prec) && H % 2 == 0 && W % 2 == 0, "%s: the map must have even sides (%d x %d)", who, H, W);
    const int CP = C * (int)op_esz(prec_is_f32(prec)) / 16;
    const int grid = stream_grid((size_t)N * H * W * CP);
    if (inverse) hipLaunchKernelGGL(cnx_s2d_kernel<true>, dim3(grid), dim3(256), 0, s, (const uint4*)src, (uint4*)dst, N, H, W, CP);
    else hipLaunchKernelGGL(cnx_s2d_kernel<false>, dim3(grid), dim3(256), 0, s, (const uint4*)src, (uint4*)dst, N, H, W, CP);
    PRX_LAUNCH_CHECK();
    return 0;
}
int prx_cnx_space_to_depth(const void* in, void* out, int N, int H, int W, int C, int prec, hipStream_t s) {
    return cnx_s2d(in, out, N, H, W, C, prec, false, s);
}
int prx_cnx_depth_to_space(const void* in, void* out, int N, int H, int W, int C, int prec, hipStream_t s) {
    return cnx_s2d(in, out, N, H, W, C, prec, true, s);
}

int prx_cnx_avgpool_fwd(const void* x, float* out, int N, int HW, int C, int prec, hipStream_t s) {
    if (int r = cnx_check_map("cnx_avgpool_fwd", N, HW, 1, C)) return r;
    PRX_REQUIRE(prec_valid(prec), "cnx_avgpool_fwd: unknown precision %d", prec);
    PRX_OP_DISPATCH(prec_is_f32(prec), prec_is_h16(prec), T,
                    hipLaunchKernelGGL(cnx_avgpool_fwd_kernel<T>, dim3(ceil_div(N * C, 256)), dim3(256), 0, s, (const T*)x, out, N, HW, C));
    PRX_LAUNCH_CHECK();
    return 0;
}
int prx_cnx_avgpool_bwd(const float* g, float* dx_f32, void* dx_op, int N, int HW, int C, int prec, hipStream_t s) {
    if (int r = cnx_check_map("cnx_avgpool_bwd", N, HW, 1, C)) return r;
    PRX_REQUIRE(prec_valid(prec) && (dx_f32 || dx_op), "cnx_avgpool_bwd: unknown precision %d, or no output", prec);
    const int grid = stream_grid((size_t)N * HW * C / 4);
    PRX_OP_DISPATCH(prec_is_f32(prec), prec_is_h16(prec), T,
                    hipLaunchKernelGGL(cnx_avgpool_bwd_kernel<T>, dim3(grid), dim3(256), 0, s, g, dx_f32, (T*)dx_op, N, HW, C, 1.f / (float)HW));
    PRX_LAUNCH_CHECK();
    return 0;
}

int prx_cnx_layernorm_fwd(const void* x, int x_f32, const float* gamma, const float* beta, void* out_op, float* out_f32, float* mean,
                          float* rstd, int rows, int C, float eps, int group, int prec, hipStream_t s) {
    PRX_REQUIRE(prec_valid(prec) && rows >= 1 && C >= 8 && C % 8 == 0 && group >= 0, "cnx_layernorm: the channel count must be a multiple of 8 (C=%d, %d rows)", C, rows);
    const dim3 grid(ceil_div(rows, 4));
    if (x_f32 || prec_is_f32(prec))
        PRX_OP_DISPATCH(prec_is_f32(prec), prec_is_h16(prec), TO,
                        hipLaunchKernelGGL((cnx_ln_fwd_kernel<float, TO>), grid, dim3(256), 0, s, (const float*)x, gamma, beta, (TO*)out_op, out_f32,
                                           mean, rstd, rows, C, eps, group));
    else
        PRX_OP_DISPATCH(0, prec_is_h16(prec), TO,
                        hipLaunchKernelGGL((cnx_ln_fwd_kernel<TO, TO>), grid, dim3(256), 0, s, (const TO*)x, gamma, beta, (TO*)out_op, out_f32,
                                           mean, rstd, rows, C, eps, group));
    PRX_LAUNCH_CHECK();
    return 0;
}
int prx_cnx_layernorm_bwd(const float* g, const void* x, int x_f32, const float* gamma, const float* mean, const float* rstd,
                          void* dx_op, float* dx_f32, int rows, int C, int group, int prec, hipStream_t s) {
    PRX_REQUIRE(prec_valid(prec) && rows >= 1 && C >= 8 && C % 8 == 0 && group >= 0 && (dx_op || dx_f32),
                "cnx_layernorm bwd: the channel count must be a multiple of 8 (C=%d, %d rows), one output is needed", C, rows);
    const dim3 grid(ceil_div(rows, 4));
    if (x_f32 || prec_is_f32(prec))
        PRX_OP_DISPATCH(prec_is_f32(prec), prec_is_h16(prec), TO,
                        hipLaunchKernelGGL((cnx_ln_bwd_kernel<float, TO>), grid, dim3(256), 0, s, g, (const float*)x, gamma, mean, rstd, (TO*)dx_op,
                                           dx_f32, rows, C, group));
    else
        PRX_OP_DISPATCH(0, prec_is_h16(prec), TO,
                        hipLaunchKernelGGL((cnx_ln_bwd_kernel<TO, TO>), grid, dim3(256), 0, s, g, (const TO*)x, gamma, mean, rstd, (TO*)dx_op,
                                           dx_f32, rows, C, group));
    PRX_LAUNCH_CHECK();
    return 0;
}

// ---- the runner ---------------------------------------------------------------------------------------------------------------
struct CnxBlock {
    void* dwpack;                                   // [2][49][C], operand format
    float *dwb, *ln_g, *ln_b, *b1, *b2;
    void *W1, *W1T, *W2, *W2T;                      // fc1 [4C, C], fc2' [C, 4C] and their transposes, operand format
    void *y, *t;                                    // saved: the stencil's output [M][C], the GELU pre-activation [M][4C]
    float *mean, *rstd;
};
struct CnxStage {
    int C, G, depth;                                // channels, map side, blocks
    float *ds_ln_g, *ds_ln_b, *ds_b, *ds_mean, *ds_rstd;   // the downsample ahead of the stage (stages 1..3)
    void *Wd, *WdT;                                 // [C, 4 Cprev] and its transpose
    float* xs[2]; void* xo[2];                      // the residual stream, ping-pong: fp32 and its operand-format twin (one buffer in the exact mode)
    std::vector<CnxBlock> B;
};
struct PrxConvNext : ImageTower {
    int proj_mlp, T;
    float eps;
    CnxStage S[4];
    void *Wstem, *WstemT; float *stem_b, *stem_ln_g, *stem_ln_b, *stem_mean, *stem_rstd;
    float *head_ln_g, *head_ln_b, *head_mean, *head_rstd, *hb1;
    void *P0, *P0T, *P1, *P1T;                      // linear: P0 = proj [E, d3]; mlp: P0 = fc1 [2E, d3], P1 = fc2 [E, 2E]
    // workspace
    void *A0, *h, *u, *dt, *dy, *dx_op, *dxpre, *hpost, *ht, *hu, *dht;
    float *xpre, *dA0, *dh, *dh2, *dx, *pooled, *dpool, *dhpost;
    int forward(const float* cutouts, int n, const float* mm, float* embeds, hipStream_t s) override;
    int backward_a(const float* cutouts, const float* mm, const float* d_embeds, double* acc, hipStream_t s) override;
    int backward_b(const float* cutouts, const float* mm, const double* acc, float* g_cutouts, hipStream_t s) override;
};

int prx_convnext_create_impl(ImageTower** out, int res, const int* depths, const int* dims, int out_dim, int proj_mlp, float ln_eps,
                             int max_n, int precision, const float* const* w, int n_w, hipStream_t s) {
    PRX_REQUIRE(prec_valid(precision), "convnext_create: unknown precision %d", precision);
    PRX_REQUIRE(res >= 32 && res % 32 == 0, "convnext_create: the input resolution must be a multiple of 32 (R=%d)", res);
    PRX_REQUIRE(max_n >= 1 && out_dim >= 8 && out_dim % 8 == 0 && ln_eps > 0.f, "convnext_create: bad max_batch %d / output_dim %d / ln_eps", max_n, out_dim);
    int n_blocks = 0;
    for (int i = 0; i < 4; ++i) {
        PRX_REQUIRE(depths[i] >= 1, "convnext_create: stage %d has %d blocks", i, depths[i]);
        PRX_REQUIRE(dims[i] >= 8 && dims[i] % 8 == 0, "convnext_create: the channel count must be a multiple of 8 (stage %d: C=%d)", i, dims[i]);
        n_blocks += depths[i];
    }
    const int n_expect = 4 + 3 * 4 + 8 * n_blocks + 2 + (proj_mlp ? 3 : 1);
    PRX_REQUIRE(n_w == n_expect, "convnext_create: expected %d weight tensors, got %d", n_expect, n_w);
    const int G0 = res / 4;
    size_t Emax = 0;
    for (int i = 0; i < 4; ++i) {
        const unsigned long long e = (unsigned long long)max_n * (G0 >> i) * (G0 >> i) * dims[i];
        PRX_REQUIRE(e < (1ull << 31), "convnext_create: %d cutouts of %d x %d x %d elements exceed the 32-bit index range", max_n, G0 >> i, G0 >> i, dims[i]);
        Emax = std::max<size_t>(Emax, (size_t)e);
    }
    std::unique_ptr<PrxConvNext> guard(new PrxConvNext());      // a failed create frees what it allocated (DevArena)
    PrxConvNext* v = guard.get();
    DevArena& m = v->mem;
    m.describe("convnext_create", ": the runner keeps one forward's activations for max_batch = %d cutouts of %d x %d (%d blocks, widths %d..%d)",
               max_n, res, res, n_blocks, dims[0], dims[3]);
    v->name = "convnext"; v->res = res; v->out_dim = out_dim; v->proj_mlp = proj_mlp; v->max_n = max_n; v->eps = ln_eps;
    v->set_precision(precision); v->T = G0 * G0 + 1; v->cur_n = 0;
    const int f32 = v->f32;
    int r;
    const float* const* q = w;
    const int d0 = dims[0];
    if ((r = prx_pack_pair(m, &v->Wstem, &v->WstemT, q[0], d0, 48, precision, s))) return r;
    if ((r = m.copy_f32(&v->stem_b, q[1], d0, s))) return r;
    if ((r = m.copy_f32(&v->stem_ln_g, q[2], d0, s))) return r;
    if ((r = m.copy_f32(&v->stem_ln_b, q[3], d0, s))) return r;
    q += 4;
    for (int i = 0; i < 4; ++i) {
        CnxStage& st = v->S[i];
        st.C = dims[i]; st.G = G0 >> i; st.depth = depths[i];
        const int C = st.C;
        const size_t M = (size_t)max_n * st.G * st.G;
        st.ds_ln_g = st.ds_ln_b = st.ds_b = st.ds_mean = st.ds_rstd = nullptr; st.Wd = st.WdT = nullptr;
        if (i > 0) {
            const int Cp = dims[i - 1];
            if ((r = m.copy_f32(&st.ds_ln_g, q[0], Cp, s))) return r;
            if ((r = m.copy_f32(&st.ds_ln_b, q[1], Cp, s))) return r;
            if ((r = prx_pack_pair(m, &st.Wd, &st.WdT, q[2], C, 4 * Cp, precision, s))) return r;
            if ((r = m.copy_f32(&st.ds_b, q[3], C, s))) return r;
            q += 4;
            DEV_ALLOC(m, alloc, st.ds_mean, 4 * M); DEV_ALLOC(m, alloc, st.ds_rstd, 4 * M);
        }
        for (int k = 0; k < 2; ++k) {
            DEV_ALLOC(m, alloc, st.xs[k], M * C);
            if (f32) st.xo[k] = st.xs[k];
            else DEV_ALLOC(m, alloc_op, st.xo[k], M * C, 0);
        }
        st.B.resize(st.depth);
        for (CnxBlock& b : st.B) {
            DEV_ALLOC(m, alloc_op, b.dwpack, (size_t)98 * C, f32);
            if ((r = prx_cnx_pack_dw(q[0], b.dwpack, C, precision, s))) return r;
            if ((r = m.copy_f32(&b.dwb, q[1], C, s))) return r;
            if ((r = m.copy_f32(&b.ln_g, q[2], C, s))) return r;
            if ((r = m.copy_f32(&b.ln_b, q[3], C, s))) return r;
            if ((r = prx_pack_pair(m, &b.W1, &b.W1T, q[4], 4 * C, C, precision, s))) return r;
            if ((r = m.copy_f32(&b.b1, q[5], 4 * C, s))) return r;
            if ((r = prx_pack_pair(m, &b.W2, &b.W2T, q[6], C, 4 * C, precision, s))) return r;
            if ((r = m.copy_f32(&b.b2, q[7], C, s))) return r;
            q += 8;
            DEV_ALLOC(m, alloc_op, b.y, M * C, f32); DEV_ALLOC(m, alloc_op, b.t, M * 4 * C, f32);
            DEV_ALLOC(m, alloc, b.mean, M); DEV_ALLOC(m, alloc, b.rstd, M);
        }
    }
    const int d3 = dims[3], E = out_dim;
    if ((r = m.copy_f32(&v->head_ln_g, q[0], d3, s))) return r;
    if ((r = m.copy_f32(&v->head_ln_b, q[1], d3, s))) return r;
    v->P1 = v->P1T = nullptr; v->hb1 = nullptr;
    if (proj_mlp) {
        if ((r = prx_pack_pair(m, &v->P0, &v->P0T, q[2], 2 * E, d3, precision, s))) return r;
        if ((r = m.copy_f32(&v->hb1, q[3], 2 * E, s))) return r;
        if ((r = prx_pack_pair(m, &v->P1, &v->P1T, q[4], E, 2 * E, precision, s))) return r;
    } else {
        if ((r = prx_pack_pair(m, &v->P0, &v->P0T, q[2], E, d3, precision, s))) return r;
    }
    const size_t RT = (size_t)max_n * v->T, N = max_n;
    DEV_ALLOC(m, alloc_op, v->A0, RT * 48, f32); DEV_ALLOC(m, alloc, v->xpre, RT * d0); DEV_ALLOC(m, alloc, v->dA0, RT * 48);
    DEV_ALLOC(m, alloc_op, v->dxpre, RT * d0, f32);
    PRX_CHECK_HIP(hipMemsetAsync(v->dxpre, 0, op_esz(f32) * RT * d0, s));       // the unused leading row of every cutout stays zero
    DEV_ALLOC(m, alloc, v->stem_mean, RT); DEV_ALLOC(m, alloc, v->stem_rstd, RT);
    DEV_ALLOC(m, alloc_op, v->h, Emax, f32); DEV_ALLOC(m, alloc_op, v->u, 4 * Emax, f32); DEV_ALLOC(m, alloc_op, v->dt, 4 * Emax, f32);
    DEV_ALLOC(m, alloc_op, v->dy, Emax, f32);
    DEV_ALLOC(m, alloc, v->dh, Emax); DEV_ALLOC(m, alloc, v->dh2, Emax); DEV_ALLOC(m, alloc, v->dx, Emax);
    if (f32) v->dx_op = v->dx;
    else DEV_ALLOC(m, alloc_op, v->dx_op, Emax, 0);
    DEV_ALLOC(m, alloc, v->pooled, N * d3); DEV_ALLOC(m, alloc, v->dpool, N * d3); DEV_ALLOC(m, alloc, v->dhpost, N * d3);
    DEV_ALLOC(m, alloc, v->head_mean, N); DEV_ALLOC(m, alloc, v->head_rstd, N);
    DEV_ALLOC(m, alloc_op, v->hpost, N * d3, f32); DEV_ALLOC(m, alloc_op, v->ht, N * 2 * E, f32); DEV_ALLOC(m, alloc_op, v->hu, N * 2 * E, f32);
    DEV_ALLOC(m, alloc_op, v->dht, N * 2 * E, f32); DEV_ALLOC(m, alloc_op, v->de16, N * E, f32);
    DEV_ALLOC(m, alloc, v->e, N * E); DEV_ALLOC(m, alloc, v->de, N * E);
    if ((r = v->alloc_tail())) return r;
    *out = guard.release();
    return 0;
}

int PrxConvNext::forward(const float* cutouts, int n, const float* mm, float* embeds, hipStream_t s) {
    PrxConvNext* const v = this;
    int r;
    if ((r = begin_forward(n))) return r;
    const int T = v->T, prec = v->prec;
    if ((r = prx_patchify_fwd(cutouts, mm, v->A0, prec, n, v->res, 4, T, s))) return r;
    {   GemmDesc d; d.A = v->A0; d.lda = 48; d.B = v->Wstem; d.ldb = 48; d.M = n * T; d.N = v->S[0].C; d.K = 48;
        d.bias_n = v->stem_b; d.out_f32 = v->xpre; d.ldc_f32 = v->S[0].C;
        if ((r = v->gemm(d, s))) return r; }
    if ((r = prx_cnx_layernorm_fwd(v->xpre, 1, v->stem_ln_g, v->stem_ln_b, v->f32 ? nullptr : v->S[0].xo[0], v->S[0].xs[0], v->stem_mean,
                                   v->stem_rstd, n * (T - 1), v->S[0].C, v->eps, T - 1, prec, s))) return r;
    for (int i = 0; i < 4; ++i) {
        CnxStage& st = v->S[i];
        const int C = st.C, G = st.G, M = n * G * G;
        if (i > 0) {
            CnxStage& pv = v->S[i - 1];
            const int Cp = pv.C, Mp = n * pv.G * pv.G;
            if ((r = prx_cnx_layernorm_fwd(pv.xs[pv.depth & 1], 1, st.ds_ln_g, st.ds_ln_b, v->h, nullptr, st.ds_mean, st.ds_rstd, Mp, Cp, v->eps, 0,
                                           prec, s))) return r;
            if ((r = prx_cnx_space_to_depth(v->h, v->u, n, pv.G, pv.G, Cp, prec, s))) return r;
            GemmDesc d; d.A = v->u; d.lda = 4 * Cp; d.B = st.Wd; d.ldb = 4 * Cp; d.M = M; d.N = C; d.K = 4 * Cp;
            d.bias_n = st.ds_b; d.out_f32 = st.xs[0]; d.ldc_f32 = C;
            if (!v->f32) { d.out_bf16 = st.xo[0]; d.ldc_bf16 = C; }
            if ((r = v->gemm(d, s))) return r;
        }
        for (int k = 0; k < st.depth; ++k) {
            CnxBlock& b = st.B[k];
            const int in = k & 1, on = in ^ 1;
            if ((r = prx_cnx_dwconv(st.xo[in], b.dwpack, b.dwb, nullptr, b.y, nullptr, n, G, G, C, 0, prec, s))) return r;
            if ((r = prx_cnx_layernorm_fwd(b.y, 0, b.ln_g, b.ln_b, v->h, nullptr, b.mean, b.rstd, M, C, v->eps, 0, prec, s))) return r;
            if ((r = linear_act(PRX_ACT_GELU, v->h, C, b.W1, b.b1, b.t, v->u, M, 4 * C, C, s))) return r;
            GemmDesc d; d.A = v->u; d.lda = 4 * C; d.B = b.W2; d.ldb = 4 * C; d.M = M; d.N = C; d.K = 4 * C;
            d.bias_n = b.b2; d.resid = st.xs[in]; d.ldr = C; d.out_f32 = st.xs[on]; d.ldc_f32 = C;
            if (!v->f32) { d.out_bf16 = st.xo[on]; d.ldc_bf16 = C; }
            if ((r = v->gemm(d, s))) return r;
        }
    }
    const CnxStage& l = v->S[3];
    const int d3 = l.C, E = v->out_dim;
    if ((r = prx_cnx_avgpool_fwd(l.xs[l.depth & 1], v->pooled, n, l.G * l.G, d3, PRX_PREC_F32, s))) return r;
    if ((r = prx_cnx_layernorm_fwd(v->pooled, 1, v->head_ln_g, v->head_ln_b, v->hpost, nullptr, v->head_mean, v->head_rstd, n, d3, v->eps, 0, prec, s))) return r;
    const void* last = v->hpost; const void* Wl = v->P0; int Kl = d3;
    if (v->proj_mlp) {
        if ((r = linear_act(PRX_ACT_GELU, v->hpost, d3, v->P0, v->hb1, v->ht, v->hu, n, 2 * E, d3, s))) return r;
        last = v->hu; Wl = v->P1; Kl = 2 * E;
    }
    {   GemmDesc d; d.A = last; d.lda = Kl; d.B = Wl; d.ldb = Kl; d.M = n; d.N = E; d.K = Kl; d.out_f32 = v->e; d.ldc_f32 = E;
        if ((r = v->gemm(d, s))) return r; }
    return head_fwd(embeds, n, s);
}

// Backward part A: from d(embeds) down to the stem product's input gradient and the sums the batch-global min/max renormalisation
// needs (acc[4] doubles, summed over ranks by the caller when the cutout batch is sharded).  Half mode: everything between the
// L2-normalisation backward and the stem dgrad runs under the device-chosen power-of-two scale S (every step is linear in the gradient).
int PrxConvNext::backward_a(const float* cutouts, const float* mm, const float* d_embeds, double* acc, hipStream_t s) {
    PrxConvNext* const v = this;
    int n, r;
    if ((r = backward_n(&n))) return r;
    const int T = v->T, prec = v->prec, E = v->out_dim, d3 = v->S[3].C;
    if ((r = head_bwd(d_embeds, n, s))) return r;
    // the next product reads d(e) itself in the exact mode, else a 16-bit twin: the scaled one head_bwd wrote (half), or a bf16 copy
    const void* dE = v->de;
    if (!v->f32) {
        if (!v->h16 && (r = prx_f32_to_bf16(v->de, (bf16_t*)v->de16, (size_t)n * E, s, 0))) return r;
        dE = v->de16;
    }
    if (v->proj_mlp) {
        if ((r = linear_dact(PRX_ACT_MUL_DGELU, dE, E, v->P1T, v->ht, v->dht, n, 2 * E, E, s))) return r;
        GemmDesc d; d.A = v->dht; d.lda = 2 * E; d.B = v->P0T; d.ldb = 2 * E; d.M = n; d.N = d3; d.K = 2 * E; d.out_f32 = v->dhpost; d.ldc_f32 = d3;
        if ((r = v->gemm(d, s))) return r;
    } else {
        GemmDesc d; d.A = dE; d.lda = E; d.B = v->P0T; d.ldb = E; d.M = n; d.N = d3; d.K = E; d.out_f32 = v->dhpost; d.ldc_f32 = d3;
        if ((r = v->gemm(d, s))) return r;
    }
    if ((r = prx_cnx_layernorm_bwd(v->dhpost, v->pooled, 1, v->head_ln_g, v->head_mean, v->head_rstd, nullptr, v->dpool, n, d3, 0, prec, s))) return r;
    void* dxo = v->f32 ? nullptr : v->dx_op;           // the operand twin of the stream gradient (the exact mode reads the fp32 stream itself)
    if ((r = prx_cnx_avgpool_bwd(v->dpool, v->dx, dxo, n, v->S[3].G * v->S[3].G, d3, prec, s))) return r;
    for (int i = 3; i >= 0; --i) {
        CnxStage& st = v->S[i];
        const int C = st.C, G = st.G, M = n * G * G;
        for (int k = st.depth - 1; k >= 0; --k) {
            CnxBlock& b = st.B[k];
            if ((r = linear_dact(PRX_ACT_MUL_DGELU, v->dx_op, C, b.W2T, b.t, v->dt, M, 4 * C, C, s))) return r;
            {   GemmDesc d; d.A = v->dt; d.lda = 4 * C; d.B = b.W1T; d.ldb = 4 * C; d.M = M; d.N = C; d.K = 4 * C; d.out_f32 = v->dh; d.ldc_f32 = C;
                if ((r = v->gemm(d, s))) return r; }
            if ((r = prx_cnx_layernorm_bwd(v->dh, b.y, 0, b.ln_g, b.mean, b.rstd, v->dy, nullptr, M, C, 0, prec, s))) return r;
            // d(block input) = stencil^T d(y) + the gradient that went round the branch
            if ((r = prx_cnx_dwconv(v->dy, b.dwpack, nullptr, v->dx, dxo, v->dx, n, G, G, C, 1, prec, s))) return r;
        }
        if (i > 0) {
            CnxStage& pv = v->S[i - 1];
            const int Cp = pv.C, Mp = n * pv.G * pv.G;
            GemmDesc d; d.A = v->dx_op; d.lda = C; d.B = st.WdT; d.ldb = C; d.M = M; d.N = 4 * Cp; d.K = C; d.out_f32 = v->dh; d.ldc_f32 = 4 * Cp;
            if ((r = v->gemm(d, s))) return r;
            if ((r = prx_cnx_depth_to_space(v->dh, v->dh2, n, pv.G, pv.G, Cp, PRX_PREC_F32, s))) return r;
            if ((r = prx_cnx_layernorm_bwd(v->dh2, pv.xs[pv.depth & 1], 1, st.ds_ln_g, st.ds_mean, st.ds_rstd, dxo, v->dx, Mp, Cp, 0, prec, s))) return r;
        }
    }
    const int d0 = v->S[0].C;
    if ((r = prx_cnx_layernorm_bwd(v->dx, v->xpre, 1, v->stem_ln_g, v->stem_mean, v->stem_rstd, v->dxpre, nullptr, n * (T - 1), d0, T - 1, prec, s))) return r;
    {   GemmDesc d; d.A = v->dxpre; d.lda = d0; d.B = v->WstemT; d.ldb = d0; d.M = n * T; d.N = 48; d.K = d0; d.out_f32 = v->dA0; d.ldc_f32 = 48;
        if (v->h16) d.alpha_dev = v->gs + 1;        // unscaled (1/S) here, before the (rank-summed) renormalisation sums
        if ((r = v->gemm(d, s))) return r; }
    return prx_patchify_bwd_reduce(cutouts, mm, v->dA0, acc, n, v->res, 4, T, s);
}

int PrxConvNext::backward_b(const float* cutouts, const float* mm, const double* acc, float* g_cutouts, hipStream_t s) {
    int n;
    if (int r = backward_n(&n)) return r;
    return prx_patchify_bwd_apply(cutouts, mm, dA0, acc, g_cutouts, n, res, 4, T, s);
}
