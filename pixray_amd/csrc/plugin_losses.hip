// Built-in custom losses of pixray (Losses/SaturationLoss.py, SymmetryLoss.py, SmoothnessLoss.py, PaletteLoss.py,
// EdgeLoss.py, GaussianLoss.py, AestheticLoss.py) in fp32 with fp64 accumulators.  Each loss scalar leaves its launch through plug_reduce (fixed summation order,
// no float atomics).  Where the gradient is local (symmetry, edge, gaussian, aesthetic, palette) the forward launch writes it too; saturation needs
// the batch statistics first and smoothness a neighbourhood of per-pixel factors, so they take a second, elementwise launch.
#include "plugin_losses.h"
#include "../../include/prx.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- saturation
// x: [n][3][hw].  rg = r - g, yb = (r + g) / 2 - b over all n*hw pixels; sums of rg, rg^2, yb, yb^2.
__global__ __launch_bounds__(PLUG_THREADS) void saturation_fwd_kernel(const float* __restrict__ x, int n, int hw, float weight,
                                                                      double* __restrict__ partials, double* __restrict__ stats,
                                                                      float* __restrict__ loss, unsigned* __restrict__ ticket) {
    const long long N = (long long)n * hw;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long p = (long long)blockIdx.x * PLUG_THREADS + threadIdx.x; p < N; p += (long long)gridDim.x * PLUG_THREADS) {
        const long long b = p / hw, q = p - b * hw;
        const float* px = x + b * 3 * hw + q;
        const float r = px[0], g = px[hw], bl = px[2 * hw];
        const float rg = r - g, yb = 0.5f * (r + g) - bl;
        v[0] += rg; v[1] += (double)rg * rg; v[2] += yb; v[3] += (double)yb * yb;
    }
    if (!plug_reduce<4>(v, partials, ticket)) return;
    const double Nd = (double)N;
    const double mrg = v[0] / Nd, myb = v[2] / Nd;
    const double vrg = (v[1] - v[0] * mrg) / (Nd - 1.0), vyb = (v[3] - v[2] * myb) / (Nd - 1.0);   // unbiased, as torch.std
    const double S = sqrt(fmax(vrg, 0.0) + fmax(vyb, 0.0)), M = sqrt(mrg * mrg + myb * myb);
    stats[0] = mrg; stats[1] = myb; stats[2] = S; stats[3] = M;
    *loss = (float)(-(S + 0.3 * M) * (double)weight / 10.0);
}

// d loss / d rg_i = -w/10 (rg_i - mean_rg) / ((N-1) S) - w/10 * 0.3 mean_rg / (N M), the same for yb; then through rg, yb to r, g, b
__global__ __launch_bounds__(PLUG_THREADS) void saturation_bwd_kernel(const float* __restrict__ x, int n, int hw, float weight,
                                                                      const double* __restrict__ stats, const float* __restrict__ gout,
                                                                      float* __restrict__ grad) {
    const long long N = (long long)n * hw;
    const double mrg = stats[0], myb = stats[1], S = stats[2], M = stats[3];
    const double c = -(double)weight / 10.0 * (double)*gout;
    const float a1 = (float)(S > 0.0 ? c / ((double)(N - 1) * S) : 0.0);
    const float brg = (float)(M > 0.0 ? c * 0.3 * mrg / ((double)N * M) : 0.0);
    const float byb = (float)(M > 0.0 ? c * 0.3 * myb / ((double)N * M) : 0.0);
    const float fmrg = (float)mrg, fmyb = (float)myb;
    for (long long p = (long long)blockIdx.x * PLUG_THREADS + threadIdx.x; p < N; p += (long long)gridDim.x * PLUG_THREADS) {
        const long long b = p / hw, q = p - b * hw;
        const float* px = x + b * 3 * hw + q;
        const float r = px[0], g = px[hw], bl = px[2 * hw];
        const float drg = a1 * ((r - g) - fmrg) + brg;
        const float dyb = a1 * ((0.5f * (r + g) - bl) - fmyb) + byb;
        float* pg = grad + b * 3 * hw + q;
        pg[0] = drg + 0.5f * dyb;
        pg[hw] = -drg + 0.5f * dyb;
        pg[2 * hw] = -dyb;
    }
}

// ---------------------------------------------------------------------------------------------------------------- symmetry
// MSE(x, flip_W(x)) * w over planes*h*w elements; d/dx_j = 4 w (x_j - x_mirror(j)) / N
__global__ __launch_bounds__(PLUG_THREADS) void symmetry_kernel(const float* __restrict__ x, int planes, int h, int w, float weight,
                                                                double* __restrict__ partials, float* __restrict__ grad,
                                                                float* __restrict__ loss, unsigned* __restrict__ ticket) {
    const long long N = (long long)planes * h * w;
    const float gs = 4.f * weight / (float)N;
    double v[1] = {0.0};
    for (long long e = (long long)blockIdx.x * PLUG_THREADS + threadIdx.x; e < N; e += (long long)gridDim.x * PLUG_THREADS) {
        const long long row = e / w;
        const int c = (int)(e - row * w);
        const float d = x[e] - x[row * w + (w - 1 - c)];
        v[0] += (double)d * d;
        grad[e] = gs * d;
    }
    if (plug_reduce<1>(v, partials, ticket)) *loss = (float)(v[0] / (double)N * (double)weight);
}

// ---------------------------------------------------------------------------------------------------------------- edge
// out [1..][3][h][w] against a flat colour.  Each element weighs a = sum over the margin bands holding it of 1 / (band size)
// (+ the global term's weight / N): loss = edge_weight * sum a d^2, grad = 2 edge_weight a d.  Bands as EdgeLoss.py slices them:
// left = cols [0, left), right = cols [w - right, w), up / down = rows [0, upper) / [h - lower, h) between the side bands.
__global__ __launch_bounds__(PLUG_THREADS) void edge_kernel(const float* __restrict__ x, int planes, int h, int w, float cr, float cg,
                                                            float cb, int left, int right, int upper, int lower, float inv_l,
                                                            float inv_r, float inv_u, float inv_d, float inv_all, float edge_weight,
                                                            double* __restrict__ partials, float* __restrict__ grad,
                                                            float* __restrict__ loss, unsigned* __restrict__ ticket) {
    const long long N = (long long)planes * h * w;
    double v[1] = {0.0};
    for (long long e = (long long)blockIdx.x * PLUG_THREADS + threadIdx.x; e < N; e += (long long)gridDim.x * PLUG_THREADS) {
        const long long pl = e / ((long long)h * w);
        const int rem = (int)(e - pl * h * w), y = rem / w, c = rem - y * w;
        const int ch = (int)(pl % 3);
        const float col = ch == 0 ? cr : (ch == 1 ? cg : cb);
        float a = inv_all;
        if (c < left) a += inv_l;
        if (c >= w - right) a += inv_r;
        if (c >= left && c < w - right) {
            if (y < upper) a += inv_u;
            if (y >= h - lower) a += inv_d;
        }
        const float d = x[e] - col;
        v[0] += (double)a * ((double)d * d);
        grad[e] = 2.f * edge_weight * a * d;
    }
    if (plug_reduce<1>(v, partials, ticket)) *loss = (float)(v[0] * (double)edge_weight);
}

// ---------------------------------------------------------------------------------------------------------------- edge, target image / mask
// edge_kernel with a per-element target (target [3][h][w], or the flat colour where it is null) and an optional mask [h][w]:
// with a mask the bands are ignored and every element where mask <= 0 weighs inv_mask (EdgeLoss.py:100-103: the masked-in part
// is replaced by the target, so it adds nothing).  Both pointers are kernel arguments: wave-uniform branches.
__global__ __launch_bounds__(PLUG_THREADS) void edge_target_kernel(const float* __restrict__ x, int planes, int h, int w,
                                                                   const float* __restrict__ target, float cr, float cg, float cb,
                                                                   const float* __restrict__ mask, int left, int right, int upper,
                                                                   int lower, float inv_l, float inv_r, float inv_u, float inv_d,
                                                                   float inv_mask, float inv_all, float edge_weight,
                                                                   double* __restrict__ partials, float* __restrict__ grad,
                                                                   float* __restrict__ loss, unsigned* __restrict__ ticket) {
    const long long N = (long long)planes * h * w;
    const long long hw = (long long)h * w;
    double v[1] = {0.0};
    for (long long e = (long long)blockIdx.x * PLUG_THREADS + threadIdx.x; e < N; e += (long long)gridDim.x * PLUG_THREADS) {
        const long long pl = e / hw;
        const int rem = (int)(e - pl * hw), y = rem / w, c = rem - y * w;
        const int ch = (int)(pl % 3);
        const float tgt = target ? target[(size_t)ch * hw + rem] : (ch == 0 ? cr : (ch == 1 ? cg : cb));
        float a = inv_all;
        if (mask) {
            if (mask[rem] <= 0.f) a += inv_mask;
        } else {
            if (c < left) a += inv_l;
            if (c >= w - right) a += inv_r;
            if (c >= left && c < w - right) {
                if (y < upper) a += inv_u;
                if (y >= h - lower) a += inv_d;
            }
        }
        const float d = x[e] - tgt;
        v[0] += (double)a * ((double)d * d);
        grad[e] = 2.f * edge_weight * a * d;
    }
    if (plug_reduce<1>(v, partials, ticket)) *loss = (float)(v[0] * (double)edge_weight);
}

// ---------------------------------------------------------------------------------------------------------------- gaussian
// GaussianLoss.py: x [planes = 3k][h][w] against a flat colour, each element weighed a = |1 - gy[y] gx[c]| (the outer product of
// two 1-D gaussian tables, rounded to fp32 before the subtraction as torch.outer does): loss = scale * sum a |d|,
// grad = scale a sign(d), sign(0) = 0 (torch.abs's subgradient)
__global__ __launch_bounds__(PLUG_THREADS) void gaussian_kernel(const float* __restrict__ x, int planes, int h, int w,
                                                                const float* __restrict__ gy, const float* __restrict__ gx, float cr,
                                                                float cg, float cb, float scale, double* __restrict__ partials,
                                                                float* __restrict__ grad, float* __restrict__ loss,
                                                                unsigned* __restrict__ ticket) {
    const long long N = (long long)planes * h * w;
    const long long hw = (long long)h * w;
    double v[1] = {0.0};
    for (long long e = (long long)blockIdx.x * PLUG_THREADS + threadIdx.x; e < N; e += (long long)gridDim.x * PLUG_THREADS) {
        const long long pl = e / hw;
        const int rem = (int)(e - pl * hw), y = rem / w, c = rem - y * w;
        const int ch = (int)(pl % 3);
        const float col = ch == 0 ? cr : (ch == 1 ? cg : cb);
        const float a = fabsf(1.f - __fmul_rn(gy[y], gx[c]));
        const float d = x[e] - col;
        v[0] += (double)a * (double)fabsf(d);
        grad[e] = d > 0.f ? scale * a : (d < 0.f ? -(scale * a) : 0.f);
    }
    if (plug_reduce<1>(v, partials, ticket)) *loss = (float)(v[0] * (double)scale);
}

// ---------------------------------------------------------------------------------------------------------------- aesthetic
// AestheticLoss.py: a linear head on the normalised embeddings, r_i = w . e_i / max(|e_i|, 1e-12) + bias (F.normalize's eps),
// loss = 0.02 / n * sum_i (r_i - target)^2.  One wave per row, lanes stride over d; both row sums in double through wave_sum_d.
// grad[i][j] = 0.04 / n * diff_i * (w[j] inv_i - e[i][j] dot_i inv_i^3) above the eps floor; at or below it the divisor is the
// constant 1e-12 and only the first term remains.  The row loop is wave-uniform and every thread reaches plug_reduce.
__global__ __launch_bounds__(PLUG_THREADS) void aesthetic_kernel(const float* __restrict__ embeds, int n, int d,
                                                                 const float* __restrict__ w, float bias, float target,
                                                                 double* __restrict__ partials, float* __restrict__ grad,
                                                                 float* __restrict__ loss, unsigned* __restrict__ ticket) {
    constexpr int ROWS = PLUG_THREADS / 64;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const double gs = 0.04 / (double)n;
    double v[1] = {0.0};
    for (long long row = (long long)blockIdx.x * ROWS + wid; row < n; row += (long long)gridDim.x * ROWS) {
        const float* e = embeds + (size_t)row * d;
        double ss = 0.0, dot = 0.0;
        for (int j = lane; j < d; j += 64) {
            const double ej = (double)e[j];
            ss += ej * ej;
            dot += (double)w[j] * ej;
        }
        ss = wave_sum_d(ss);
        dot = wave_sum_d(dot);
        const double nrm = sqrt(ss);
        const bool floor_ = nrm <= 1e-12;
        const double inv = 1.0 / (floor_ ? 1e-12 : nrm);
        const double diff = dot * inv + (double)bias - (double)target;
        const double ga = gs * diff * inv, gb = floor_ ? 0.0 : gs * diff * dot * inv * inv * inv;
        float* g = grad + (size_t)row * d;
        for (int j = lane; j < d; j += 64) g[j] = (float)(ga * (double)w[j] - gb * (double)e[j]);
        if (lane == 0) v[0] += diff * diff;
    }
    if (plug_reduce<1>(v, partials, ticket)) *loss = (float)(v[0] * 0.02 / (double)n);
}

// ---------------------------------------------------------------------------------------------------------------- palette
// per pixel the nearest palette entry (squared distance, first index on ties), loss = scale * sum |p - c|, grad = scale (p - c)/|p - c|
// (0 where the pixel sits on its entry, as torch.norm's subgradient)
constexpr int PLUG_MAX_PALETTE = 256;
__global__ __launch_bounds__(PLUG_THREADS) void palette_kernel(const float* __restrict__ x, int n, int hw, const float* __restrict__ palette,
                                                               int np, float scale, double* __restrict__ partials, float* __restrict__ grad,
                                                               float* __restrict__ loss, unsigned* __restrict__ ticket) {
    __shared__ float pal[PLUG_MAX_PALETTE * 3];
    for (int i = threadIdx.x; i < np * 3; i += PLUG_THREADS) pal[i] = palette[i];
    __syncthreads();
    const long long N = (long long)n * hw;
    double v[1] = {0.0};
    for (long long p = (long long)blockIdx.x * PLUG_THREADS + threadIdx.x; p < N; p += (long long)gridDim.x * PLUG_THREADS) {
        const long long b = p / hw, q = p - b * hw;
        const float* px = x + b * 3 * hw + q;
        const float r = px[0], g = px[hw], bl = px[2 * hw];
        float best = INFINITY;
        int bi = 0;
        for (int j = 0; j < np; ++j) {
            const float dr = r - pal[3 * j], dg = g - pal[3 * j + 1], db = bl - pal[3 * j + 2];
            const float d2 = dr * dr + dg * dg + db * db;
            if (d2 < best) { best = d2; bi = j; }
        }
        const float dr = r - pal[3 * bi], dg = g - pal[3 * bi + 1], db = bl - pal[3 * bi + 2];
        const float nrm = sqrtf(dr * dr + dg * dg + db * db);
        v[0] += nrm;
        const float f = nrm > 0.f ? scale / nrm : 0.f;
        float* pg = grad + b * 3 * hw + q;
        pg[0] = f * dr; pg[hw] = f * dg; pg[2 * hw] = f * db;
    }
    if (plug_reduce<1>(v, partials, ticket)) *loss = (float)(v[0] * (double)scale);
}

// ---------------------------------------------------------------------------------------------------------------- smoothness
// torch.gradient along an axis of length L (uniform spacing): g[i] = sum_j coef(i, j) f[j], |i - j| <= 2.  Interior: central
// difference; the two end points one-sided, first or second order.  The backward is the transpose: df[j] = sum_i coef(i, j) u[i].
template <typename T>
__device__ __forceinline__ T grad_coef(int i, int j, int L, int eo, T inv_h) {
    const int d = j - i;
    if (i == 0) {
        if (eo == 1) return d == 0 ? -inv_h : (d == 1 ? inv_h : T(0));
        return d == 0 ? T(-1.5) * inv_h : (d == 1 ? T(2) * inv_h : (d == 2 ? T(-0.5) * inv_h : T(0)));
    }
    if (i == L - 1) {
        if (eo == 1) return d == 0 ? inv_h : (d == -1 ? -inv_h : T(0));
        return d == 0 ? T(1.5) * inv_h : (d == -1 ? T(-2) * inv_h : (d == -2 ? T(0.5) * inv_h : T(0)));
    }
    return d == 1 ? T(0.5) * inv_h : (d == -1 ? T(-0.5) * inv_h : T(0));
}

// The reference's view: cutouts [n][3][h][w] -> pixels [n*h][w][3]; rows run through all cutouts (row r is row r % h of cutout
// r / h), so the row-direction stencil crosses cutout boundaries exactly as torch.gradient over that view does.
struct SmoothView {
    const float* x;
    int n, h, w;
    __device__ __forceinline__ float at(int r, int c, int ch) const {
        const int b = r / h, y = r - b * h;
        return x[(((size_t)b * 3 + ch) * h + y) * w + c];
    }
    // the two gradients of channel ch at (r, c), in T = float (backward) or double (forward)
    template <typename T>
    __device__ __forceinline__ void grads(int r, int c, int ch, int eo, T inv_h, T& gy, T& gx) const {
        const int R = n * h;
        gy = T(0); gx = T(0);
        for (int d = -2; d <= 2; ++d) {
            const int rr = r + d, cc = c + d;
            if (rr >= 0 && rr < R) { const T k = grad_coef(r, rr, R, eo, inv_h); if (k != T(0)) gy += k * (T)at(rr, c, ch); }
            if (cc >= 0 && cc < w) { const T k = grad_coef(c, cc, w, eo, inv_h); if (k != T(0)) gx += k * (T)at(r, cc, ch); }
        }
    }
};

// per pixel: s = |(gy, gx) over 3 channels|, v = s | min(s, 0.5) | log(1 + s); loss = w * mean v.
// tfac[pixel] = dv/ds / s (0 where s == 0: the zero subgradient at a flat pixel, where the reference's sqrt gives NaN).
// The pixel is evaluated in double (stencil with 1 / spacing formed in double, root, logarithm): with fp32 values the scalar was the sum
// of per-pixel roundings plus its own conversion, up to 1.5 * 2^-24 off on a 3 x 3 cutout; now it is the fp32 rounding of the float64 sum,
// the best an fp32 result can be, and tfac is rounded once.  15 loads per channel dominate either way.
__global__ __launch_bounds__(PLUG_THREADS) void smoothness_fwd_kernel(const float* __restrict__ x, int n, int h, int w, int type, int eo,
                                                                      float spacing, float weight, double* __restrict__ partials,
                                                                      float* __restrict__ tfac, float* __restrict__ loss,
                                                                      unsigned* __restrict__ ticket) {
    const SmoothView V{x, n, h, w};
    const long long N = (long long)n * h * w;
    const double inv_h = 1.0 / (double)spacing;
    double v[1] = {0.0};
    for (long long p = (long long)blockIdx.x * PLUG_THREADS + threadIdx.x; p < N; p += (long long)gridDim.x * PLUG_THREADS) {
        const int r = (int)(p / w), c = (int)(p - (long long)r * w);
        double ss = 0.0;
        for (int ch = 0; ch < 3; ++ch) {
            double gy, gx;
            V.grads(r, c, ch, eo, inv_h, gy, gx);
            ss += gy * gy + gx * gx;
        }
        const double s = sqrt(ss);
        double val, dv;
        if (type == 1) { val = fmin(s, 0.5); dv = s <= 0.5 ? 1.0 : 0.0; }
        else if (type == 2) { val = log(1.0 + s); dv = 1.0 / (1.0 + s); }
        else { val = s; dv = 1.0; }
        v[0] += val;
        tfac[p] = s > 0.0 ? (float)(dv / s) : 0.f;
    }
    if (plug_reduce<1>(v, partials, ticket)) *loss = (float)(v[0] / (double)N * (double)weight);
}

// df(r, c, ch) = gs * [ sum_i coef_row(i, r) tfac(i, c) gy(i, c, ch) + sum_i coef_col(i, c) tfac(r, i) gx(r, i, ch) ]
__global__ __launch_bounds__(PLUG_THREADS) void smoothness_bwd_kernel(const float* __restrict__ tfac, const float* __restrict__ x, int n,
                                                                      int h, int w, int eo, float inv_h, float weight,
                                                                      const float* __restrict__ gout, float* __restrict__ grad) {
    const SmoothView V{x, n, h, w};
    const int R = n * h;
    const long long N = (long long)R * w;
    const float gs = (float)((double)weight * (double)*gout / (double)N);
    for (long long p = (long long)blockIdx.x * PLUG_THREADS + threadIdx.x; p < N; p += (long long)gridDim.x * PLUG_THREADS) {
        const int r = (int)(p / w), c = (int)(p - (long long)r * w);
        float acc[3] = {0.f, 0.f, 0.f};
        for (int d = -2; d <= 2; ++d) {
            const int rr = r + d;
            if (rr >= 0 && rr < R) {
                const float k = grad_coef(rr, r, R, eo, inv_h);
                const float t = k != 0.f ? tfac[(size_t)rr * w + c] : 0.f;
                if (t != 0.f)
                    for (int ch = 0; ch < 3; ++ch) { float gy, gx; V.grads(rr, c, ch, eo, inv_h, gy, gx); acc[ch] += k * t * gy; }
            }
            const int cc = c + d;
            if (cc >= 0 && cc < w) {
                const float k = grad_coef(cc, c, w, eo, inv_h);
                const float t = k != 0.f ? tfac[(size_t)r * w + cc] : 0.f;
                if (t != 0.f)
                    for (int ch = 0; ch < 3; ++ch) { float gy, gx; V.grads(r, cc, ch, eo, inv_h, gy, gx); acc[ch] += k * t * gx; }
            }
        }
        const int b = r / h, y = r - b * h;
        for (int ch = 0; ch < 3; ++ch) grad[(((size_t)b * 3 + ch) * h + y) * w + c] = gs * acc[ch];
    }
}

// ---------------------------------------------------------------------------------------------------------------- gaussian blur
// depthwise "valid" cross-correlation with one k x k tap table (GaussianSmoothing: F.conv2d, groups = channels) and its adjoint
constexpr int PLUG_MAX_TAPS = 33;
__global__ __launch_bounds__(PLUG_THREADS) void blur_fwd_kernel(const float* __restrict__ x, int planes, int h, int w,
                                                                const float* __restrict__ taps, int k, float* __restrict__ y) {
    __shared__ float t[PLUG_MAX_TAPS * PLUG_MAX_TAPS];
    for (int i = threadIdx.x; i < k * k; i += PLUG_THREADS) t[i] = taps[i];
    __syncthreads();
    const int ho = h - k + 1, wo = w - k + 1;
    const long long N = (long long)planes * ho * wo;
    for (long long e = (long long)blockIdx.x * PLUG_THREADS + threadIdx.x; e < N; e += (long long)gridDim.x * PLUG_THREADS) {
        const long long pl = e / ((long long)ho * wo);
        const int rem = (int)(e - pl * ho * wo), oy = rem / wo, ox = rem - oy * wo;
        const float* src = x + ((size_t)pl * h + oy) * w + ox;
        float acc = 0.f;
        for (int a = 0; a < k; ++a)
            for (int b = 0; b < k; ++b) acc += t[a * k + b] * src[(size_t)a * w + b];
        y[e] = acc;
    }
}
__global__ __launch_bounds__(PLUG_THREADS) void blur_bwd_kernel(const float* __restrict__ gy, int planes, int h, int w,
                                                                const float* __restrict__ taps, int k, float* __restrict__ gx) {
    __shared__ float t[PLUG_MAX_TAPS * PLUG_MAX_TAPS];
    for (int i = threadIdx.x; i < k * k; i += PLUG_THREADS) t[i] = taps[i];
    __syncthreads();
    const int ho = h - k + 1, wo = w - k + 1;
    const long long N = (long long)planes * h * w;
    for (long long e = (long long)blockIdx.x * PLUG_THREADS + threadIdx.x; e < N; e += (long long)gridDim.x * PLUG_THREADS) {
        const long long pl = e / ((long long)h * w);
        const int rem = (int)(e - pl * h * w), iy = rem / w, ix = rem - iy * w;
        float acc = 0.f;
        for (int a = 0; a < k; ++a) {
            const int oy = iy - a;
            if (oy < 0 || oy >= ho) continue;
            for (int b = 0; b < k; ++b) {
                const int ox = ix - b;
                if (ox >= 0 && ox < wo) acc += t[a * k + b] * gy[((size_t)pl * ho + oy) * wo + ox];
            }
        }
        gx[e] = acc;
    }
}

}  // namespace

int plug_saturation_fwd(const float* x, int n, int hw, float weight, double* partials, double* stats, float* loss, unsigned* ticket,
                        hipStream_t s) {
    PRX_REQUIRE(x && partials && stats && loss && ticket && n > 0 && hw > 0 && (long long)n * hw > 1, "saturation: bad arguments");
    hipLaunchKernelGGL(saturation_fwd_kernel, dim3(plug_blocks((long long)n * hw)), dim3(PLUG_THREADS), 0, s, x, n, hw, weight, partials, stats, loss, ticket);
    PRX_LAUNCH_CHECK();
    return 0;
}
int plug_saturation_bwd(const float* x, int n, int hw, float weight, const double* stats, const float* gout, float* grad, hipStream_t s) {
    PRX_REQUIRE(x && stats && gout && grad && n > 0 && hw > 0, "saturation backward: bad arguments");
    hipLaunchKernelGGL(saturation_bwd_kernel, dim3(plug_blocks((long long)n * hw)), dim3(PLUG_THREADS), 0, s, x, n, hw, weight, stats, gout, grad);
    PRX_LAUNCH_CHECK();
    return 0;
}
int plug_symmetry(const float* x, int planes, int h, int w, float weight, double* partials, float* grad, float* loss, unsigned* ticket,
                  hipStream_t s) {
    PRX_REQUIRE(x && partials && grad && loss && ticket && planes > 0 && h > 0 && w > 0, "symmetry: bad arguments");
    hipLaunchKernelGGL(symmetry_kernel, dim3(plug_blocks((long long)planes * h * w)), dim3(PLUG_THREADS), 0, s, x, planes, h, w, weight, partials, grad, loss, ticket);
    PRX_LAUNCH_CHECK();
    return 0;
}
int plug_edge(const float* x, int planes, int h, int w, float r, float g, float b, int left, int right, int upper, int lower,
              float inv_l, float inv_r, float inv_u, float inv_d, float inv_all, float edge_weight, double* partials, float* grad,
              float* loss, unsigned* ticket, hipStream_t s) {
    PRX_REQUIRE(x && partials && grad && loss && ticket && planes > 0 && planes % 3 == 0 && h > 0 && w > 0, "edge: bad arguments");
    hipLaunchKernelGGL(edge_kernel, dim3(plug_blocks((long long)planes * h * w)), dim3(PLUG_THREADS), 0, s, x, planes, h, w, r, g, b, left, right, upper, lower,
                       inv_l, inv_r, inv_u, inv_d, inv_all, edge_weight, partials, grad, loss, ticket);
    PRX_LAUNCH_CHECK();
    return 0;
}
int plug_edge_target(const float* x, int planes, int h, int w, const float* target, float r, float g, float b, const float* mask,
                     int left, int right, int upper, int lower, float inv_l, float inv_r, float inv_u, float inv_d, float inv_mask,
                     float inv_all, float edge_weight, double* partials, float* grad, float* loss, unsigned* ticket, hipStream_t s) {
    PRX_REQUIRE(x && partials && grad && loss && ticket && planes > 0 && planes % 3 == 0 && h > 0 && w > 0, "edge (target): bad arguments");
    PRX_REQUIRE(left >= 0 && right >= 0 && upper >= 0 && lower >= 0, "edge (target): negative margins");
    hipLaunchKernelGGL(edge_target_kernel, dim3(plug_blocks((long long)planes * h * w)), dim3(PLUG_THREADS), 0, s, x, planes, h, w, target, r, g, b, mask,
                       left, right, upper, lower, inv_l, inv_r, inv_u, inv_d, inv_mask, inv_all, edge_weight, partials, grad, loss, ticket);
    PRX_LAUNCH_CHECK();
    return 0;
}
int plug_gaussian(const float* x, int planes, int h, int w, const float* gy, const float* gx, float r, float g, float b, float scale,
                  double* partials, float* grad, float* loss, unsigned* ticket, hipStream_t s) {
    PRX_REQUIRE(x && gy && gx && partials && grad && loss && ticket && planes > 0 && planes % 3 == 0 && h > 0 && w > 0, "gaussian: bad arguments");
    hipLaunchKernelGGL(gaussian_kernel, dim3(plug_blocks((long long)planes * h * w)), dim3(PLUG_THREADS), 0, s, x, planes, h, w, gy, gx, r, g, b, scale,
                       partials, grad, loss, ticket);
    PRX_LAUNCH_CHECK();
    return 0;
}
int plug_aesthetic(const float* embeds, int n, int d, const float* w, float bias, float target, double* partials, float* grad, float* loss,
                   unsigned* ticket, hipStream_t s) {
    PRX_REQUIRE(embeds && w && partials && grad && loss && ticket && n >= 1 && d >= 1, "aesthetic: bad arguments");
    hipLaunchKernelGGL(aesthetic_kernel, dim3(plug_blocks((long long)n * 64)), dim3(PLUG_THREADS), 0, s, embeds, n, d, w, bias, target, partials, grad,
                       loss, ticket);
    PRX_LAUNCH_CHECK();
    return 0;
}
int plug_palette(const float* x, int n, int hw, const float* palette, int np, float scale, double* partials, float* grad, float* loss,
                 unsigned* ticket, hipStream_t s) {
    PRX_REQUIRE(x && palette && partials && grad && loss && ticket && n > 0 && hw > 0, "palette: bad arguments");
    PRX_REQUIRE(np >= 1 && np <= PLUG_MAX_PALETTE, "palette: %d entries (1 .. %d supported)", np, PLUG_MAX_PALETTE);
    hipLaunchKernelGGL(palette_kernel, dim3(plug_blocks((long long)n * hw)), dim3(PLUG_THREADS), 0, s, x, n, hw, palette, np, scale, partials, grad, loss, ticket);
    PRX_LAUNCH_CHECK();
    return 0;
}
int plug_smoothness_fwd(const float* x, int n, int h, int w, int type, int edge_order, float spacing, float weight, double* partials,
                        float* tfac, float* loss, unsigned* ticket, hipStream_t s) {
    PRX_REQUIRE(x && partials && tfac && loss && ticket && n > 0, "smoothness: bad arguments");
    PRX_REQUIRE((edge_order == 1 || edge_order == 2) && h > edge_order && w > edge_order && spacing != 0.f && type >= 0 && type <= 2,
                "smoothness: edge order %d on %d x %d, type %d", edge_order, h, w, type);
    hipLaunchKernelGGL(smoothness_fwd_kernel, dim3(plug_blocks((long long)n * h * w)), dim3(PLUG_THREADS), 0, s, x, n, h, w, type, edge_order, spacing, weight,
                       partials, tfac, loss, ticket);
    PRX_LAUNCH_CHECK();
    return 0;
}
int plug_smoothness_bwd(const float* tfac, const float* x, int n, int h, int w, int edge_order, float spacing, float weight,
                        const float* gout, float* grad, hipStream_t s) {
    PRX_REQUIRE(tfac && x && gout && grad && n > 0 && h > edge_order && w > edge_order && spacing != 0.f, "smoothness backward: bad arguments");
    hipLaunchKernelGGL(smoothness_bwd_kernel, dim3(plug_blocks((long long)n * h * w)), dim3(PLUG_THREADS), 0, s, tfac, x, n, h, w, edge_order, 1.f / spacing, weight,
                       gout, grad);
    PRX_LAUNCH_CHECK();
    return 0;
}
int plug_blur_fwd(const float* x, int planes, int h, int w, const float* taps, int k, float* y, hipStream_t s) {
    PRX_REQUIRE(x && taps && y && planes > 0 && k >= 1 && k <= PLUG_MAX_TAPS && h >= k && w >= k, "blur: bad arguments (k = %d)", k);
    hipLaunchKernelGGL(blur_fwd_kernel, dim3(plug_blocks((long long)planes * (h - k + 1) * (w - k + 1))), dim3(PLUG_THREADS), 0, s, x, planes, h, w, taps, k, y);
    PRX_LAUNCH_CHECK();
    return 0;
}
int plug_blur_bwd(const float* gy, int planes, int h, int w, const float* taps, int k, float* gx, hipStream_t s) {
    PRX_REQUIRE(gy && taps && gx && planes > 0 && k >= 1 && k <= PLUG_MAX_TAPS && h >= k && w >= k, "blur backward: bad arguments");
    hipLaunchKernelGGL(blur_bwd_kernel, dim3(plug_blocks((long long)planes * h * w)), dim3(PLUG_THREADS), 0, s, gy, planes, h, w, taps, k, gx);
    PRX_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- C ABI
#define S_(x) ((hipStream_t)(x))
extern "C" {
int prx_saturation_fwd(const float* x, int n, int hw, float weight, double* partials, double* stats, float* loss, unsigned* ticket,
                       prx_stream_t s) {
    return plug_saturation_fwd(x, n, hw, weight, partials, stats, loss, ticket, S_(s));
}
int prx_saturation_bwd(const float* x, int n, int hw, float weight, const double* stats, const float* gout, float* grad, prx_stream_t s) {
    return plug_saturation_bwd(x, n, hw, weight, stats, gout, grad, S_(s));
}
int prx_symmetry_fwd_bwd(const float* x, int planes, int h, int w, float weight, double* partials, float* grad, float* loss,
                         unsigned* ticket, prx_stream_t s) {
    return plug_symmetry(x, planes, h, w, weight, partials, grad, loss, ticket, S_(s));
}
int prx_edge_fwd_bwd(const float* x, int planes, int h, int w, float r, float g, float b, int left, int right, int upper, int lower,
                     float inv_l, float inv_r, float inv_u, float inv_d, float inv_all, float edge_weight, double* partials, float* grad,
                     float* loss, unsigned* ticket, prx_stream_t s) {
    return plug_edge(x, planes, h, w, r, g, b, left, right, upper, lower, inv_l, inv_r, inv_u, inv_d, inv_all, edge_weight, partials,
                     grad, loss, ticket, S_(s));
}
int prx_edge_target_fwd_bwd(const float* x, int planes, int h, int w, const float* target, float r, float g, float b, const float* mask,
                            int left, int right, int upper, int lower, float inv_l, float inv_r, float inv_u, float inv_d, float inv_mask,
                            float inv_all, float edge_weight, double* partials, float* grad, float* loss, unsigned* ticket, prx_stream_t s) {
    return plug_edge_target(x, planes, h, w, target, r, g, b, mask, left, right, upper, lower, inv_l, inv_r, inv_u, inv_d, inv_mask, inv_all,
                            edge_weight, partials, grad, loss, ticket, S_(s));
}
int prx_gaussian_fwd_bwd(const float* x, int planes, int h, int w, const float* gy, const float* gx, float r, float g, float b, float scale,
                         double* partials, float* grad, float* loss, unsigned* ticket, prx_stream_t s) {
    return plug_gaussian(x, planes, h, w, gy, gx, r, g, b, scale, partials, grad, loss, ticket, S_(s));
}
int prx_aesthetic_fwd_bwd(const float* embeds, int n, int d, const float* w, float bias, float target, double* partials, float* grad,
                          float* loss, unsigned* ticket, prx_stream_t s) {
    return plug_aesthetic(embeds, n, d, w, bias, target, partials, grad, loss, ticket, S_(s));
}
int prx_palette_fwd_bwd(const float* x, int n, int hw, const float* palette, int np, float scale, double* partials, float* grad,
                        float* loss, unsigned* ticket, prx_stream_t s) {
    return plug_palette(x, n, hw, palette, np, scale, partials, grad, loss, ticket, S_(s));
}
int prx_smoothness_fwd(const float* x, int n, int h, int w, int type, int edge_order, float spacing, float weight, double* partials,
                       float* tfac, float* loss, unsigned* ticket, prx_stream_t s) {
    return plug_smoothness_fwd(x, n, h, w, type, edge_order, spacing, weight, partials, tfac, loss, ticket, S_(s));
}
int prx_smoothness_bwd(const float* tfac, const float* x, int n, int h, int w, int edge_order, float spacing, float weight,
                       const float* gout, float* grad, prx_stream_t s) {
    return plug_smoothness_bwd(tfac, x, n, h, w, edge_order, spacing, weight, gout, grad, S_(s));
}
int prx_blur_fwd(const float* x, int planes, int h, int w, const float* taps, int k, float* y, prx_stream_t s) {
    return plug_blur_fwd(x, planes, h, w, taps, k, y, S_(s));
}
int prx_blur_bwd(const float* gy, int planes, int h, int w, const float* taps, int k, float* gx, prx_stream_t s) {
    return plug_blur_bwd(gy, planes, h, w, taps, k, gx, S_(s));
}
}
