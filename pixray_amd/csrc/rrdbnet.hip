// RRDBNet x4 runner (super_resolution drawer): see rrdbnet.h for the layout and the memory formula.
//
// The convolution family is one kernel template, rrdb_conv_kernel<T, GIN, UP>: an implicit 3x3 GEMM on the small MFMA shape,
// TRANSPOSED as in gemmrow_kernel.h (weights are the A operand, pixels the B operand), so a lane ends up with 4 consecutive
// output channels of one pixel per accumulator and the epilogue runs from registers.  A workgroup owns 16 consecutive pixels
// x 32 output channels (two accumulators per lane); the grid is (pixels / 16, N / 32).  Why this tile: a latent convolution
// has M = h w = 4096 pixels at a 256^2 canvas and N = 32, i.e. 256 such tiles for 256 CUs -- any larger tile leaves CUs
// idle, and tile count, not FLOPs, decides the time of these launches.  For the same reason the tile's K loop (9 taps x Cin,
// up to 54 dependent load -> MFMA steps) is SPLIT over the workgroup's four waves, one per SIMD: each runs every fourth K
// step, waves 1..3 leave their partial sums in LDS, wave 0 adds them in a fixed order and runs the epilogue.  The operands go
// from L2 straight into the MFMA registers (16 bytes per lane and K step): a (pixel, tap) row of the concat buffer is a
// contiguous channel prefix, so there is nothing to re-arrange through LDS.  The weight pack of a launch (<= 108 KB in half)
// is read by every workgroup and stays in L2.
//   half mode: v_mfma_f32_16x16x32_f16, a lane loads 8 consecutive channels of its K step of 32;
//   f32 mode : v_mfma_f32_16x16x4_f32 four times per 16-byte load; a lane's j-th float feeds step j, which permutes k inside a
//              block of 16 channels identically for both operands (a sum over k does not care).
// GIN: the data-gradient direction -- the input is an fp32 gradient slice, multiplied on load by the LeakyReLU derivative of
// the stored activation and rounded to T there; the weights are the flipped, transposed pack; the result accumulates into the
// prefix of an fp32 gradient concat buffer.  Every output element has exactly one owner lane: no atomics, same bits every run.
#include "rrdbnet.h"

#include <memory>
#include <new>
#include <vector>

#include "weight_pack.h"

#include "../../include/prx.h"

namespace {

template <typename T> struct RrdbFrag;
template <> struct RrdbFrag<half_t> { typedef f16x8 V; static constexpr int E = 8; };
template <> struct RrdbFrag<float> { typedef f32x4 V; static constexpr int E = 4; };

__device__ __forceinline__ f32x4 rrdb_mfma(const f16x8& a, const f16x8& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 rrdb_mfma(const f32x4& a, const f32x4& b, f32x4 c) {
#pragma unroll
    for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], c, 0, 0, 0);
    return c;
}
__device__ __forceinline__ float lrelu_slope(float a) { return a > 0.f ? 1.f : 0.2f; }

// the E channels ch .. ch + E of source pixel `src` as an MFMA operand; !valid (a tap outside the image): zeros
template <typename T, bool GIN>
__device__ __forceinline__ typename RrdbFrag<T>::V rrdb_load_px(const RrdbConvArgs& a, size_t src, int ch, bool valid) {
    typedef typename RrdbFrag<T>::V V;
    constexpr int E = RrdbFrag<T>::E;
    V v;
    if constexpr (!GIN) {
        v = *reinterpret_cast<const V*>(reinterpret_cast<const T*>(a.in) + src * a.ld_in + a.in_off + ch);
    } else {
        const float* g = reinterpret_cast<const float*>(a.in) + src * a.ld_in + a.in_off + ch;
        float t[E];
#pragma unroll
        for (int q = 0; q < E; q += 4) {
            const float4 f = *reinterpret_cast<const float4*>(g + q);
            t[q] = f.x; t[q + 1] = f.y; t[q + 2] = f.z; t[q + 3] = f.w;
        }
        if (a.act) {
            const V s = *reinterpret_cast<const V*>(reinterpret_cast<const T*>(a.act) + src * a.ld_act + a.act_off + ch);
#pragma unroll
            for (int e = 0; e < E; ++e) t[e] *= lrelu_slope((float)s[e]);
        }
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = op_cvt<T>(t[e]);
    }
    if (!valid) {
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = (T)0.f;
    }
    return v;
}

template <typename T, bool GIN, bool UP>
__global__ __launch_bounds__(256) void rrdb_conv_kernel(RrdbConvArgs a) {
    typedef typename RrdbFrag<T>::V V;
    constexpr int E = RrdbFrag<T>::E, CS = 4 * E;          // channels per lane and per K step
    __shared__ __attribute__((aligned(16))) float red[3 * 64 * 8];
    const int tid = threadIdx.x, lane = tid & 63, m_l = lane & 15, kg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = a.H * a.W;
    const int pix = blockIdx.x * 16 + m_l;
    const bool live = pix < M;
    const int pc = live ? pix : M - 1;
    const int y = pc / a.W, x = pc - y * a.W;
    const int n0 = blockIdx.y * 32;
    const int Kc = a.Kc, K9 = 9 * Kc;
    const int Win = UP ? a.W >> 1 : a.W;
    const T* w0 = reinterpret_cast<const T*>(a.w) + (size_t)(n0 + m_l) * K9 + kg * E;
    const T* w1 = w0 + (size_t)16 * K9;
    f32x4 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 4; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }

    // the K steps (tap, block of CS channels) are dealt round-robin to the four waves: a quarter of the dependent
    // load -> MFMA chain each, four times as many waves in flight; the partial sums meet in LDS in a fixed order
    const int spt = Kc / CS, S = 9 * spt;
#pragma unroll 2
    for (int s = wave; s < S; s += 4) {
        const int tap = s / spt, c = (s - tap * spt) * CS;
        const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
        const bool valid = yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
        const int sy = UP ? yy >> 1 : yy, sx = UP ? xx >> 1 : xx;
        const size_t src = valid ? (size_t)sy * Win + sx : 0;
        const V p = rrdb_load_px<T, GIN>(a, src, c + kg * E, valid);
        const V b0 = *reinterpret_cast<const V*>(w0 + tap * Kc + c);
        const V b1 = *reinterpret_cast<const V*>(w1 + tap * Kc + c);
        acc0 = rrdb_mfma(b0, p, acc0);
        acc1 = rrdb_mfma(b1, p, acc1);
    }
    if (wave) {
        float* r = red + ((wave - 1) * 64 + lane) * 8;
        *reinterpret_cast<float4*>(r) = make_float4(acc0[0], acc0[1], acc0[2], acc0[3]);
        *reinterpret_cast<float4*>(r + 4) = make_float4(acc1[0], acc1[1], acc1[2], acc1[3]);
    }
    __syncthreads();
    if (wave) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* r = red + (k * 64 + lane) * 8;
        const float4 u = *reinterpret_cast<const float4*>(r), v = *reinterpret_cast<const float4*>(r + 4);
        acc0[0] += u.x; acc0[1] += u.y; acc0[2] += u.z; acc0[3] += u.w;
        acc1[0] += v.x; acc1[1] += v.y; acc1[2] += v.z; acc1[3] += v.w;
    }

    // epilogue: lane = pixel m_l, channels n0 + 16 j + 4 kg .. + 3 of accumulator j
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + 16 * j + 4 * kg;
        const f32x4 acc = j ? acc1 : acc0;
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float t = acc[i] + (a.bias ? a.bias[n + i] : 0.f);
            if (a.lrelu) t = t > 0.f ? t : 0.2f * t;
            v[i] = a.alpha * t;
        }
        if (live) {
            if (n < a.rn) {
                if (a.r1) {
                    const float4 r = *reinterpret_cast<const float4*>(a.r1 + (size_t)pix * a.ld_r1 + n);
                    v[0] += a.beta * r.x; v[1] += a.beta * r.y; v[2] += a.beta * r.z; v[3] += a.beta * r.w;
                }
                if (a.r2) {
                    const float4 r = *reinterpret_cast<const float4*>(a.r2 + (size_t)pix * a.ld_r2 + n);
                    v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
                }
            }
            if (a.out_f32) {
                float* o = a.out_f32 + (size_t)pix * a.ld_of + a.of_off + n;
                if (a.accum) {
                    const float4 r = *reinterpret_cast<const float4*>(o);
                    v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
                }
                *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
            }
            if (a.out) op_st4<T>(reinterpret_cast<T*>(a.out), (size_t)pix * a.ld_out + a.out_off + n, v[0], v[1], v[2], v[3]);
        }
    }
}

// the backward of a nearest-2x read: out[y][x][c] = the sum of the 2 x 2 block of in [2h][2w][C], in a fixed order
__global__ __launch_bounds__(256) void rrdb_sum2x2_kernel(const float* __restrict__ in, float* __restrict__ out, int h, int w, int C4) {
    const size_t total = (size_t)h * w * C4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % C4);
        const size_t p = i / C4;
        const int x = (int)(p % w), y = (int)(p / w);
        const float4* s = reinterpret_cast<const float4*>(in);
        const size_t r0 = ((size_t)(2 * y) * (2 * w) + 2 * x) * C4 + c, r1 = r0 + (size_t)2 * w * C4;
        const float4 a = s[r0], b = s[r0 + C4], d = s[r1], e = s[r1 + C4];
        reinterpret_cast<float4*>(out)[i] = make_float4((a.x + b.x) + (d.x + e.x), (a.y + b.y) + (d.y + e.y), (a.z + b.z) + (d.z + e.z),
                                                        (a.w + b.w) + (d.w + e.w));
    }
}

// ---- the edge convolutions: Cin = 3 and Cout = 3 are not MFMA shapes; direct kernels, fp32 weights in the torch layout ----
// conv_first: z NCHW fp32 [3][h][w] -> 64 channels NHWC; a thread owns (pixel, 4 output channels)
template <typename T>
__global__ __launch_bounds__(256) void rrdb_first_kernel(const float* __restrict__ z, const float* __restrict__ wt, const float* __restrict__ bias,
                                                         int h, int w, T* __restrict__ out, int ld_out, float* __restrict__ out_f32) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int pix = t >> 4, co = (t & 15) * 4;
    if (pix >= h * w) return;
    const int y = pix / w, x = pix - y * w;
    float v[4] = {bias[co], bias[co + 1], bias[co + 2], bias[co + 3]};
    for (int tap = 0; tap < 9; ++tap) {
        const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
        if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
            const float s = z[((size_t)ci * h + yy) * w + xx];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = fmaf(s, wt[((co + i) * 3 + ci) * 9 + tap], v[i]);
        }
    }
    if (out) op_st4<T>(out, (size_t)pix * ld_out + co, v[0], v[1], v[2], v[3]);
    if (out_f32) *reinterpret_cast<float4*>(out_f32 + (size_t)pix * 64 + co) = make_float4(v[0], v[1], v[2], v[3]);
}
// its data gradient: dz[c][p] = sum over taps, co of (g1 + g2)[p + d][co] w[co][c][8 - tap]; a thread owns (pixel, c)
__global__ __launch_bounds__(256) void rrdb_first_bwd_kernel(const float* __restrict__ g1, int ld1, const float* __restrict__ g2, int ld2,
                                                             const float* __restrict__ wt, int h, int w, float* __restrict__ dz) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int pix = t >> 2, c = t & 3;
    if (pix >= h * w || c >= 3) return;
    const int y = pix / w, x = pix - y * w;
    float acc = 0.f;
    for (int tap = 0; tap < 9; ++tap) {
        const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
        if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
        const size_t q = (size_t)yy * w + xx;
        for (int co = 0; co < 64; co += 4) {
            float4 g = *reinterpret_cast<const float4*>(g1 + q * ld1 + co);
            if (g2) {
                const float4 e = *reinterpret_cast<const float4*>(g2 + q * ld2 + co);
                g.x += e.x; g.y += e.y; g.z += e.z; g.w += e.w;
            }
            const float* ww = wt + ((size_t)co * 3 + c) * 9 + (8 - tap);
            acc = fmaf(g.x, ww[0], acc); acc = fmaf(g.y, ww[27], acc); acc = fmaf(g.z, ww[54], acc); acc = fmaf(g.w, ww[81], acc);
        }
    }
    dz[(size_t)c * h * w + pix] = acc;
}
// conv_last + clamp_with_grad: 64 NHWC -> image NCHW fp32 [3][H][W]; `raw` keeps the un-clamped value for the backward
template <typename T>
__global__ __launch_bounds__(256) void rrdb_last_kernel(const T* __restrict__ in, const float* __restrict__ wt, const float* __restrict__ bias,
                                                        int H, int W, int clamp, float* __restrict__ image, float* __restrict__ raw) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= H * W) return;
    const int y = pix / W, x = pix - y * W;
    float v[3] = {bias[0], bias[1], bias[2]};
    for (int tap = 0; tap < 9; ++tap) {
        const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
        const T* p = in + ((size_t)yy * W + xx) * 64;
        for (int ci = 0; ci < 64; ci += 4) {
            const float4 s = op_ld4v<T>(p, ci);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* ww = wt + ((size_t)c * 64 + ci) * 9 + tap;
                v[c] = fmaf(s.x, ww[0], v[c]); v[c] = fmaf(s.y, ww[9], v[c]); v[c] = fmaf(s.z, ww[18], v[c]); v[c] = fmaf(s.w, ww[27], v[c]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t o = (size_t)c * H * W + pix;
        if (raw) raw[o] = v[c];
        image[o] = clamp ? fminf(fmaxf(v[c], 0.f), 1.f) : v[c];
    }
}
// clamp_with_grad's backward rule, g * ((g * (x - clamp(x))) >= 0), then conv_last's data gradient: a thread owns (pixel, 4 ci)
__device__ __forceinline__ float rrdb_clamp_grad(float g, float x) {
    const float c = fminf(fmaxf(x, 0.f), 1.f);
    return g * (x - c) >= 0.f ? g : 0.f;
}
__global__ __launch_bounds__(256) void rrdb_last_bwd_kernel(const float* __restrict__ g_image, const float* __restrict__ raw,
                                                            const float* __restrict__ wt, int H, int W, int clamp, float* __restrict__ g_out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int pix = t >> 4, ci = (t & 15) * 4;
    if (pix >= H * W) return;
    const int y = pix / W, x = pix - y * W;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int tap = 0; tap < 9; ++tap) {
        const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const size_t o = ((size_t)c * H + yy) * W + xx;
            float g = g_image[o];
            if (clamp) g = rrdb_clamp_grad(g, raw[o]);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = fmaf(g, wt[((size_t)c * 64 + ci + i) * 9 + (8 - tap)], v[i]);
        }
    }
    *reinterpret_cast<float4*>(g_out + (size_t)pix * 64 + ci) = make_float4(v[0], v[1], v[2], v[3]);
}

template <typename T>
void rrdb_conv_dispatch(const RrdbConvArgs& a, int dgrad, hipStream_t s) {
    const dim3 grid(ceil_div(a.H * a.W, 16), a.N / 32);
    if (dgrad) hipLaunchKernelGGL((rrdb_conv_kernel<T, true, false>), grid, dim3(256), 0, s, a);
    else if (a.up) hipLaunchKernelGGL((rrdb_conv_kernel<T, false, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((rrdb_conv_kernel<T, false, false>), grid, dim3(256), 0, s, a);
}

}  // namespace

int rrdb_conv_launch(const RrdbConvArgs& a, int dgrad, int f32, hipStream_t s) {
    PRX_REQUIRE(a.in && a.w && (a.out || a.out_f32), "rrdb conv: null input, weights or output");
    PRX_REQUIRE(a.Kc >= 32 && a.Kc % 32 == 0 && a.N >= 32 && a.N % 32 == 0, "rrdb conv: channels must be multiples of 32 (Kc=%d, N=%d)", a.Kc, a.N);
    PRX_REQUIRE(a.H >= 1 && a.W >= 1 && (long long)a.H * a.W <= (1ll << 27), "rrdb conv: bad grid %d x %d", a.H, a.W);
    PRX_REQUIRE(!a.up || (!dgrad && a.H % 2 == 0 && a.W % 2 == 0), "rrdb conv: the nearest-2x read is a forward variant on an even grid");
    PRX_REQUIRE(a.ld_in % 8 == 0 && a.in_off % 8 == 0 && a.in_off + a.Kc <= a.ld_in, "rrdb conv: input slice [%d, +%d) of stride %d", a.in_off, a.Kc, a.ld_in);
    PRX_REQUIRE(!a.act || (dgrad && a.ld_act % 8 == 0 && a.act_off % 8 == 0 && a.act_off + a.Kc <= a.ld_act), "rrdb conv: bad activation slice");
    PRX_REQUIRE(!a.out || (a.ld_out % 8 == 0 && a.out_off % 8 == 0 && a.out_off + a.N <= a.ld_out), "rrdb conv: bad output slice");
    PRX_REQUIRE(!a.out_f32 || (a.ld_of % 4 == 0 && a.of_off % 4 == 0 && a.of_off + a.N <= a.ld_of), "rrdb conv: bad fp32 output slice");
    PRX_REQUIRE((!a.r1 || a.ld_r1 % 4 == 0) && (!a.r2 || a.ld_r2 % 4 == 0) && a.rn % 4 == 0, "rrdb conv: bad residual stride");
    PRX_REQUIRE((!a.r1 || a.ld_r1 >= a.rn) && (!a.r2 || a.ld_r2 >= a.rn), "rrdb conv: residual narrower than rn");
    if (f32) rrdb_conv_dispatch<float>(a, dgrad, s);
    else rrdb_conv_dispatch<half_t>(a, dgrad, s);
    PRX_LAUNCH_CHECK();
    return 0;
}

static int rrdb_prec(int prec, int* f32) {
    PRX_REQUIRE(prec != PRX_PREC_BF16, "rrdbnet: bf16 operands are not built (the kernels exist for \"fp16\" and \"f32\")");
    PRX_REQUIRE(prec == PRX_PREC_F32 || prec == PRX_PREC_F16, "rrdbnet: unknown precision %d", prec);
    *f32 = prec == PRX_PREC_F32;
    return 0;
}

// ---- the runner ---------------------------------------------------------------------------------------------------------------
struct RrdbConvW { void* wf; void* wd; const float* bias; int cin, cout; };
struct prx_rrdbnet {
    int nb = 0, h = 0, w = 0, f32 = 0, have_fwd = 0, clamp = 1;
    size_t esz = 2;
    DevArena mem;                        // every device buffer below: freed with the handle
    float *w_first = nullptr, *b_first = nullptr, *w_last = nullptr, *b_last = nullptr;
    std::vector<RrdbConvW> convs;        // 15 per RRDB (rdb1.conv1 .. rdb3.conv5), then conv_body, conv_up1, conv_up2, conv_hr
    std::vector<void*> cat;              // 3 nb concat buffers [h w][192] T
    float* X[4] = {};                    // trunk ring [h w][64] fp32: X[j % 4] is the input of RDB j (RDB 0: feat)
    float* feat = nullptr;
    float* G[4] = {};                    // gradient ring [h w][192] fp32: G[j % 4] belongs to RDB j, G[3 nb % 4][:, :64] to the trunk output
    void *tb = nullptr, *u0 = nullptr, *u1 = nullptr, *u2 = nullptr, *u3 = nullptr;
    float *raw = nullptr, *gA = nullptr, *gB = nullptr, *gC = nullptr, *gD = nullptr;
    const float* xin(int j) const { return j == 0 ? feat : X[j & 3]; }
};

extern "C" void prx_rrdbnet_destroy(prx_rrdbnet* h) { delete h; }

extern "C" int prx_rrdbnet_create(prx_rrdbnet** out, int num_feat, int num_grow, int num_block, int h, int w, const float* const* weights,
                                  int n_weights, int precision, prx_stream_t stream) {
    PRX_REQUIRE(out && weights, "prx_rrdbnet_create: null argument");
    *out = nullptr;
    PRX_REQUIRE(num_feat == 64 && num_grow == 32,
                "prx_rrdbnet_create: the kernels are built for num_feat = 64, num_grow = 32 (got %d, %d)", num_feat, num_grow);
    PRX_REQUIRE(num_block >= 1 && num_block <= 64, "prx_rrdbnet_create: num_block = %d is outside [1, 64]", num_block);
    PRX_REQUIRE(h >= 1 && w >= 1 && (long long)h * w <= (1ll << 22), "prx_rrdbnet_create: latent %d x %d is outside [1, 2^22 pixels]", h, w);
    const int n_conv = 15 * num_block + 6;
    PRX_REQUIRE(n_weights == 2 * n_conv, "prx_rrdbnet_create: %d blocks take %d tensors (weight, bias per convolution), got %d", num_block,
                2 * n_conv, n_weights);
    for (int i = 0; i < n_weights; ++i) PRX_REQUIRE(weights[i], "prx_rrdbnet_create: weight tensor %d is null", i);
    int f32 = 0;
    if (int rc = rrdb_prec(precision, &f32)) return rc;
    hipStream_t s = (hipStream_t)stream;
    std::unique_ptr<prx_rrdbnet> guard(new (std::nothrow) prx_rrdbnet());      // a failed create frees what it allocated (DevArena)
    prx_rrdbnet* r = guard.get();
    PRX_REQUIRE(r, "prx_rrdbnet_create: out of host memory");
    r->nb = num_block; r->h = h; r->w = w; r->f32 = f32; r->esz = f32 ? 4 : 2;
    const size_t hw = (size_t)h * w;
    DevArena& m = r->mem;
    m.describe("prx_rrdbnet_create", ": the runner keeps every activation and gradient buffer of %d blocks at %d x %d (the concat buffers alone take %.0f MB)",
               num_block, h, w, 3.0 * num_block * 192 * r->esz * hw / 1e6);
    int rc;
    // the weights are copied: the caller may release its tensors once the stream has run
    if ((rc = m.copy_f32(&r->w_first, weights[0], 64 * 27, s))) return rc;
    if ((rc = m.copy_f32(&r->b_first, weights[1], 64, s))) return rc;
    if ((rc = m.copy_f32(&r->w_last, weights[2 * (n_conv - 1)], 3 * 64 * 9, s))) return rc;
    if ((rc = m.copy_f32(&r->b_last, weights[2 * (n_conv - 1) + 1], 3, s))) return rc;
    for (int i = 1; i < n_conv - 1; ++i) {
        const int k = i - 1;
        int cin = 64, cout = 64;
        if (k < 15 * num_block) { const int c = k % 5; cin = 64 + 32 * c; cout = c == 4 ? 64 : 32; }
        RrdbConvW cw;
        cw.cin = cin; cw.cout = cout;
        DEV_ALLOC(m, alloc_op, cw.wf, (size_t)cin * cout * 9, f32);
        DEV_ALLOC(m, alloc_op, cw.wd, (size_t)cin * cout * 9, f32);
        float* bias;
        if ((rc = m.copy_f32(&bias, weights[2 * i + 1], cout, s))) return rc;
        cw.bias = bias;
        if ((rc = prx_pack_conv3x3(weights[2 * i], cw.wf, cw.wd, cout, cin, cin, cout, precision, s))) return rc;
        r->convs.push_back(cw);
    }
    for (int j = 0; j < 3 * num_block; ++j) { void* c; DEV_ALLOC(m, alloc_op, c, hw * 192, f32); r->cat.push_back(c); }
    for (int i = 0; i < 4; ++i) { DEV_ALLOC(m, alloc, r->X[i], hw * 64); DEV_ALLOC(m, alloc, r->G[i], hw * 192); }
    DEV_ALLOC(m, alloc, r->feat, hw * 64);
    DEV_ALLOC(m, alloc_op, r->tb, hw * 64, f32); DEV_ALLOC(m, alloc_op, r->u0, hw * 64, f32); DEV_ALLOC(m, alloc_op, r->u1, 4 * hw * 64, f32);
    DEV_ALLOC(m, alloc_op, r->u2, 16 * hw * 64, f32); DEV_ALLOC(m, alloc_op, r->u3, 16 * hw * 64, f32);
    DEV_ALLOC(m, alloc, r->raw, 48 * hw);
    DEV_ALLOC(m, alloc, r->gA, 16 * hw * 64); DEV_ALLOC(m, alloc, r->gB, 16 * hw * 64);
    DEV_ALLOC(m, alloc, r->gC, 4 * hw * 64); DEV_ALLOC(m, alloc, r->gD, hw * 64);
    *out = guard.release();
    return 0;
}

static RrdbConvArgs rrdb_args0() {
    RrdbConvArgs a = {};
    a.alpha = 1.f; a.beta = 1.f;
    return a;
}

extern "C" int prx_rrdbnet_synth(prx_rrdbnet* r, const float* z, float* image, int clamp, prx_stream_t stream) {
    PRX_REQUIRE(r && z && image, "prx_rrdbnet_synth: null argument");
    hipStream_t s = (hipStream_t)stream;
    const int h = r->h, w = r->w, hw = h * w, f32 = r->f32, nR = 3 * r->nb;
    if (f32) hipLaunchKernelGGL((rrdb_first_kernel<float>), dim3(ceil_div(hw * 16, 256)), dim3(256), 0, s, z, r->w_first, r->b_first, h, w, (float*)r->cat[0], 192, r->feat);
    else hipLaunchKernelGGL((rrdb_first_kernel<half_t>), dim3(ceil_div(hw * 16, 256)), dim3(256), 0, s, z, r->w_first, r->b_first, h, w, (half_t*)r->cat[0], 192, r->feat);
    PRX_LAUNCH_CHECK();
    for (int j = 0; j < nR; ++j) {
        for (int c = 0; c < 5; ++c) {
            const RrdbConvW& cw = r->convs[5 * j + c];
            RrdbConvArgs a = rrdb_args0();
            a.in = r->cat[j]; a.ld_in = 192; a.in_off = 0;
            a.w = cw.wf; a.bias = cw.bias; a.Kc = cw.cin; a.N = cw.cout; a.H = h; a.W = w;
            if (c < 4) {
                a.lrelu = 1;
                a.out = r->cat[j]; a.ld_out = 192; a.out_off = 64 + 32 * c;
            } else {
                // x5 * 0.2 + x, and in the third block of an RRDB (x5 * 0.2 + x) * 0.2 + x0 = 0.04 x5 + 0.2 x + x0
                const bool third = j % 3 == 2;
                a.alpha = third ? 0.04f : 0.2f; a.beta = third ? 0.2f : 1.f;
                a.r1 = r->xin(j); a.ld_r1 = 64; a.rn = 64;
                if (third) { a.r2 = r->xin(j - 2); a.ld_r2 = 64; }
                if (j + 1 < nR) { a.out = r->cat[j + 1]; a.ld_out = 192; }
                else { a.out = r->tb; a.ld_out = 64; }
                a.out_f32 = r->X[(j + 1) & 3]; a.ld_of = 64;
            }
            if (int rc = rrdb_conv_launch(a, 0, f32, s)) return rc;
        }
    }
    const RrdbConvW* tail = &r->convs[5 * nR];      // conv_body, conv_up1, conv_up2, conv_hr
    {
        RrdbConvArgs a = rrdb_args0();               // feat + conv_body(trunk)
        a.in = r->tb; a.ld_in = 64; a.w = tail[0].wf; a.bias = tail[0].bias; a.Kc = 64; a.N = 64; a.H = h; a.W = w;
        a.r1 = r->feat; a.ld_r1 = 64; a.rn = 64;
        a.out = r->u0; a.ld_out = 64;
        if (int rc = rrdb_conv_launch(a, 0, f32, s)) return rc;
    }
    const void* tin[3] = {r->u0, r->u1, r->u2};
    void* tout[3] = {r->u1, r->u2, r->u3};
    for (int k = 0; k < 3; ++k) {                    // conv_up1, conv_up2 (nearest-2x reads), conv_hr, each + LeakyReLU
        RrdbConvArgs a = rrdb_args0();
        a.in = tin[k]; a.ld_in = 64; a.w = tail[1 + k].wf; a.bias = tail[1 + k].bias; a.Kc = 64; a.N = 64;
        a.H = k == 0 ? 2 * h : 4 * h; a.W = k == 0 ? 2 * w : 4 * w; a.up = k < 2; a.lrelu = 1;
        a.out = tout[k]; a.ld_out = 64;
        if (int rc = rrdb_conv_launch(a, 0, f32, s)) return rc;
    }
    const int H = 4 * h, W = 4 * w;
    if (f32) hipLaunchKernelGGL((rrdb_last_kernel<float>), dim3(ceil_div(H * W, 256)), dim3(256), 0, s, (const float*)r->u3, r->w_last, r->b_last, H, W, clamp, image, r->raw);
    else hipLaunchKernelGGL((rrdb_last_kernel<half_t>), dim3(ceil_div(H * W, 256)), dim3(256), 0, s, (const half_t*)r->u3, r->w_last, r->b_last, H, W, clamp, image, r->raw);
    PRX_LAUNCH_CHECK();
    r->clamp = clamp; r->have_fwd = 1;
    return 0;
}

static int rrdb_sum2x2(const float* in, float* out, int h, int w, hipStream_t s) {
    hipLaunchKernelGGL(rrdb_sum2x2_kernel, dim3(ceil_div(h * w * 16, 256)), dim3(256), 0, s, in, out, h, w, 16);
    PRX_LAUNCH_CHECK();
    return 0;
}

extern "C" int prx_rrdbnet_backward(prx_rrdbnet* r, const float* g_image, float* g_z, prx_stream_t stream) {
    PRX_REQUIRE(r && g_image && g_z, "prx_rrdbnet_backward: null argument");
    PRX_REQUIRE(r->have_fwd, "prx_rrdbnet_backward: no synth has run on this handle");
    hipStream_t s = (hipStream_t)stream;
    const int h = r->h, w = r->w, f32 = r->f32, nR = 3 * r->nb, H = 4 * h, W = 4 * w;
    const RrdbConvW* tail = &r->convs[5 * nR];
    hipLaunchKernelGGL(rrdb_last_bwd_kernel, dim3(ceil_div(H * W * 16, 256)), dim3(256), 0, s, g_image, r->raw, r->w_last, H, W, r->clamp, r->gA);
    PRX_LAUNCH_CHECK();
    auto dgrad = [&](const float* gin, int ld_in, int in_off, const void* act, int ld_act, int act_off, const RrdbConvW& cw, int HH, int WW, float* gout,
                     int ld_of, RrdbConvArgs extra) {
        RrdbConvArgs a = extra;
        a.in = gin; a.ld_in = ld_in; a.in_off = in_off; a.act = act; a.ld_act = ld_act; a.act_off = act_off;
        a.w = cw.wd; a.Kc = cw.cout; a.N = cw.cin; a.H = HH; a.W = WW;
        a.out_f32 = gout; a.ld_of = ld_of;
        return rrdb_conv_launch(a, 1, f32, s);
    };
    int rc;
    if ((rc = dgrad(r->gA, 64, 0, r->u3, 64, 0, tail[3], H, W, r->gB, 64, rrdb_args0()))) return rc;            // conv_hr
    if ((rc = dgrad(r->gB, 64, 0, r->u2, 64, 0, tail[2], H, W, r->gA, 64, rrdb_args0()))) return rc;            // conv_up2, then its 2x read
    if ((rc = rrdb_sum2x2(r->gA, r->gC, 2 * h, 2 * w, s))) return rc;
    if ((rc = dgrad(r->gC, 64, 0, r->u1, 64, 0, tail[1], 2 * h, 2 * w, r->gB, 64, rrdb_args0()))) return rc;    // conv_up1
    if ((rc = rrdb_sum2x2(r->gB, r->gD, h, w, s))) return rc;                                                    // gD = d(feat + body)
    if ((rc = dgrad(r->gD, 64, 0, nullptr, 0, 0, tail[0], h, w, r->G[nR & 3], 192, rrdb_args0()))) return rc;   // conv_body
    for (int j = nR - 1; j >= 0; --j) {
        float* Gj = r->G[j & 3];
        const float* gout = r->G[(j + 1) & 3];       // the gradient of this block's output, channels [0, 64)
        {
            // conv5: the block's output is alpha x5 + beta x (+ x0): G[:, 0:192) = alpha dgrad(gout), + beta gout on the first 64
            // channels; the first block of an RRDB also receives the RRDB-level skip's gradient, which is the gradient of the
            // RRDB's output: G[(j + 3) % 4]
            RrdbConvArgs e = rrdb_args0();
            const bool third = j % 3 == 2;
            e.alpha = third ? 0.04f : 0.2f; e.beta = third ? 0.2f : 1.f;
            e.r1 = gout; e.ld_r1 = 192; e.rn = 64;
            if (j % 3 == 0) { e.r2 = r->G[(j + 3) & 3]; e.ld_r2 = 192; }
            if ((rc = dgrad(gout, 192, 0, nullptr, 0, 0, r->convs[5 * j + 4], h, w, Gj, 192, e))) return rc;
        }
        for (int c = 3; c >= 0; --c) {               // conv4 .. conv1: the gradient slice times LeakyReLU', accumulated into the prefix
            RrdbConvArgs e = rrdb_args0();
            e.accum = 1;
            if ((rc = dgrad(Gj, 192, 64 + 32 * c, r->cat[j], 192, 64 + 32 * c, r->convs[5 * j + c], h, w, Gj, 192, e))) return rc;
        }
    }
    hipLaunchKernelGGL(rrdb_first_bwd_kernel, dim3(ceil_div(h * w * 4, 256)), dim3(256), 0, s, (const float*)r->G[0], 192, (const float*)r->gD, 64, r->w_first, h, w, g_z);
    PRX_LAUNCH_CHECK();
    return 0;
}

// ---- one kernel at a time on caller-owned buffers (tests/test_kernels_rrdbnet_gpu.py) -----------------------------------------------
extern "C" int prx_k_rrdb_conv(int dgrad, const void* in, int ld_in, int in_off, const void* act, int ld_act, int act_off, const float* wt,
                               const float* bias, int Cin, int Cout, int H, int W, int up, int lrelu, float alpha, float beta, const float* r1,
                               int ld_r1, const float* r2, int ld_r2, void* out, int ld_out, int out_off, float* out_f32, int ld_of, int of_off,
                               int accum, int prec, prx_stream_t stream) {
    int f32 = 0;
    if (int rc = rrdb_prec(prec, &f32)) return rc;
    PRX_REQUIRE(wt && Cin >= 32 && Cout >= 32 && Cin % 32 == 0 && Cout % 32 == 0 && Cin <= 4096 && Cout <= 4096, "prx_k_rrdb_conv: Cin = %d, Cout = %d", Cin, Cout);
    hipStream_t s = (hipStream_t)stream;
    void* pack = nullptr;
    PRX_CHECK_HIP(hipMalloc(&pack, (size_t)Cin * Cout * 9 * (f32 ? 4 : 2)));
    int rc = prx_pack_conv3x3(wt, dgrad ? nullptr : pack, dgrad ? pack : nullptr, Cout, Cin, Cin, Cout, prec, s);      // the one side this convolution reads
    if (!rc) {
        RrdbConvArgs a = rrdb_args0();
        a.in = in; a.ld_in = ld_in; a.in_off = in_off; a.act = act; a.ld_act = ld_act; a.act_off = act_off;
        a.w = pack; a.bias = bias; a.Kc = dgrad ? Cout : Cin; a.N = dgrad ? Cin : Cout; a.H = H; a.W = W; a.up = up; a.lrelu = lrelu;
        a.alpha = alpha; a.beta = beta; a.r1 = r1; a.ld_r1 = ld_r1; a.r2 = r2; a.ld_r2 = ld_r2; a.rn = (r1 || r2) ? 64 : 0;
        a.out = out; a.ld_out = ld_out; a.out_off = out_off; a.out_f32 = out_f32; a.ld_of = ld_of; a.of_off = of_off; a.accum = accum;
        rc = rrdb_conv_launch(a, dgrad, f32, s);
    }
    (void)hipStreamSynchronize(s);
    (void)hipFree(pack);
    return rc;
}

extern "C" int prx_k_rrdb_sum2x2(const float* in, float* out, int h, int w, int C, prx_stream_t stream) {
    PRX_REQUIRE(in && out && h >= 1 && w >= 1 && C == 64, "prx_k_rrdb_sum2x2: needs C = 64 and a non-empty grid");
    return rrdb_sum2x2(in, out, h, w, (hipStream_t)stream);
}

extern "C" int prx_k_rrdb_conv_first(const float* z, const float* wt, const float* bias, int h, int w, void* out, int ld_out, float* out_f32, int prec,
                                     prx_stream_t stream) {
    int f32 = 0;
    if (int rc = rrdb_prec(prec, &f32)) return rc;
    PRX_REQUIRE(z && wt && bias && h >= 1 && w >= 1 && (!out || (ld_out >= 64 && ld_out % 8 == 0)), "prx_k_rrdb_conv_first: bad argument");
    hipStream_t s = (hipStream_t)stream;
    if (f32) hipLaunchKernelGGL((rrdb_first_kernel<float>), dim3(ceil_div(h * w * 16, 256)), dim3(256), 0, s, z, wt, bias, h, w, (float*)out, ld_out, out_f32);
    else hipLaunchKernelGGL((rrdb_first_kernel<half_t>), dim3(ceil_div(h * w * 16, 256)), dim3(256), 0, s, z, wt, bias, h, w, (half_t*)out, ld_out, out_f32);
    PRX_LAUNCH_CHECK();
    return 0;
}

extern "C" int prx_k_rrdb_conv_first_bwd(const float* g1, int ld1, const float* g2, int ld2, const float* wt, int h, int w, float* dz, prx_stream_t stream) {
    PRX_REQUIRE(g1 && wt && dz && h >= 1 && w >= 1 && ld1 >= 64 && ld1 % 4 == 0 && (!g2 || (ld2 >= 64 && ld2 % 4 == 0)), "prx_k_rrdb_conv_first_bwd: bad argument");
    hipLaunchKernelGGL(rrdb_first_bwd_kernel, dim3(ceil_div(h * w * 4, 256)), dim3(256), 0, (hipStream_t)stream, g1, ld1, g2, ld2, wt, h, w, dz);
    PRX_LAUNCH_CHECK();
    return 0;
}

extern "C" int prx_k_rrdb_conv_last(const void* in, const float* wt, const float* bias, int H, int W, int clamp, float* image, float* raw, int prec,
                                    prx_stream_t stream) {
    int f32 = 0;
    if (int rc = rrdb_prec(prec, &f32)) return rc;
    PRX_REQUIRE(in && wt && bias && image && H >= 1 && W >= 1, "prx_k_rrdb_conv_last: bad argument");
    hipStream_t s = (hipStream_t)stream;
    if (f32) hipLaunchKernelGGL((rrdb_last_kernel<float>), dim3(ceil_div(H * W, 256)), dim3(256), 0, s, (const float*)in, wt, bias, H, W, clamp, image, raw);
    else hipLaunchKernelGGL((rrdb_last_kernel<half_t>), dim3(ceil_div(H * W, 256)), dim3(256), 0, s, (const half_t*)in, wt, bias, H, W, clamp, image, raw);
    PRX_LAUNCH_CHECK();
    return 0;
}

extern "C" int prx_k_rrdb_conv_last_bwd(const float* g_image, const float* raw, const float* wt, int H, int W, int clamp, float* g_out, prx_stream_t stream) {
    PRX_REQUIRE(g_image && wt && g_out && H >= 1 && W >= 1 && (!clamp || raw), "prx_k_rrdb_conv_last_bwd: bad argument");
    hipLaunchKernelGGL(rrdb_last_bwd_kernel, dim3(ceil_div(H * W * 16, 256)), dim3(256), 0, (hipStream_t)stream, g_image, raw, wt, H, W, clamp, g_out);
    PRX_LAUNCH_CHECK();
    return 0;
}
