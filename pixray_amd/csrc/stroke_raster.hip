// The stroke drawers' renderer (pixray linedrawer.py / clipdrawer.py draw open paths of cubic Bezier segments with diffvg).
// Conventions ("Stroke drawers"); bit-parity with diffvg is not claimed:
//  * every pixel is the mean of 2 x 2 jittered samples, with the jitter of csrc/pixel_raster.hip restated below;
//  * d(s) = the Euclidean distance from sample s to the path's centre line (minimum over its segments and t in [0, 1]);
//    stroke_width is the half-width; the layer alpha is colour.a * cov with the pre-filtered coverage
//    cov = clamp(w - d + 0.5, 0, 1), a ramp one pixel wide centred on the edge (round caps and joins follow);
//  * the paper colour (optional) covers every sample at the bottom; the paths follow in index order with "over" on
//    premultiplied colour (C = a c + (1 - a) C, A = a + (1 - a) A), un-premultiplied per sample when A > 1e-6.
//
// Jitter: PCG32 per sample, idx = ((y W + x) 2 + sy) 2 + sx, inc = idx << 1 | 1, one step, state += seed, one step, then u and v as
// ((r >> 9) | 0x3f800000) - 1.  The sample sits at (x + (sx + u) / 2, y + (sy + v) / 2), in fp32.  The seed is read from a
// one-word device buffer, so a captured graph replays with whatever the host staged there.
//
// Closest point of a segment: C(t) at t = i / 32 (i = 0 .. 32); every local minimum among them is polished by 5 Newton steps on
// (C - s) . C' = 0 (a step is taken only where the second derivative is positive, t clamped to [0, 1]); the best point seen wins.
// A segment whose control-point box, grown by w + 1, excludes the sample is skipped.
//
// Layout, all of it recomputed on the device every launch (nothing on the host per iteration, graph-capturable):
//  1. one lane per path: the control-point hull grown by w + 1 -> boxes [n];
//  2. one workgroup per 16 x 16-pixel tile: the boxes meeting the tile, ballot-compacted in ascending order into
//     tile_paths[tile][0 .. tile_count[tile]) (n slots per tile: no list can overflow);
//  3. forward: one workgroup per tile, one pixel per lane, the tile's paths in order;
//  4. backward: the same tiles, the list taken in chunks of 16 layers from the last to the first.  Per chunk, the state of every
//     sample at the chunk's start is recomposited from the paper and the earlier chunks, the chunk's coverages are kept in LDS,
//     and the state below each layer is recomposited from the chunk start over them -- no division by (1 - a), no depth bound.
//     Each (tile, path) writes one slot of exact partial gradients (fp64 sums in a fixed order: width and colour, then the
//     four control points of every segment that is the closest one for some sample, segments ascending); a second launch adds
//     each path's slots in tile order.  Gradient of d w.r.t. the points: the envelope theorem, dd/dP_i = B_i(t*) (C(t*) - s) / d
//     with t* held fixed; a zero subgradient where d = 0.  No float atomics: a run repeats bit for bit.
#include "stroke_raster.h"
#include "../../include/prx.h"

namespace {

constexpr float STR_INF = 3.0e38f;
constexpr int STR_WAVES = STR_THREADS / 64;

struct Pcg32 {
    uint64_t state, inc;
};

__device__ __forceinline__ uint32_t pcg32_next(Pcg32& r) {
    const uint64_t old = r.state;
    r.state = old * 6364136223846793005ULL + (r.inc | 1ULL);
    const uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u);
    const uint32_t rot = (uint32_t)(old >> 59u);
    return (xs >> rot) | (xs << ((0u - rot) & 31u));
}

__device__ __forceinline__ float pcg32_float(Pcg32& r) {
    const uint32_t u = (pcg32_next(r) >> 9) | 0x3f800000u;
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f - 1.0f;
}

// the jitter (u, v) of sample s = 2 sy + sx of pixel (x, y)
__device__ __forceinline__ void sample_jitter(int x, int y, int w, int s, uint32_t seed, float& u, float& v) {
    const uint64_t idx = ((uint64_t)y * (uint64_t)w + (uint64_t)x) * 4u + (uint64_t)s;
    Pcg32 r{0ULL, (idx << 1u) | 1ULL};
    pcg32_next(r);
    r.state += (uint64_t)seed;
    pcg32_next(r);
    u = pcg32_float(r);
    v = pcg32_float(r);
}

struct TilePixel {
    int x, y;
    bool live;
    float px[4], py[4];
    __device__ TilePixel(int w, int h, int tiles_x, uint32_t seed) {
        const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
        x = tx * STR_TILE + (threadIdx.x % STR_TILE);
        y = ty * STR_TILE + (threadIdx.x / STR_TILE);
        live = x < w && y < h;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float u, v;
            sample_jitter(x, y, w, s, seed, u, v);
            px[s] = (float)x + ((float)(s & 1) + u) * 0.5f;
            py[s] = (float)y + ((float)(s >> 1) + v) * 0.5f;
        }
    }
};

__device__ __forceinline__ void bezier(float t, float2 q0, float2 q1, float2 q2, float2 q3, float& x, float& y) {
    const float m = 1.f - t;
    const float b0 = m * m * m, b1 = 3.f * m * m * t, b2 = 3.f * m * t * t, b3 = t * t * t;
    x = b0 * q0.x + b1 * q1.x + b2 * q2.x + b3 * q3.x;
    y = b0 * q0.y + b1 * q1.y + b2 * q2.y + b3 * q3.y;
}

__device__ __forceinline__ float dist2_at(float t, float2 q0, float2 q1, float2 q2, float2 q3) {
    float x, y;
    bezier(t, q0, q1, q2, q3, x, y);
    return x * x + y * y;
}

// Newton on (C - s) . C' = 0 from t (a step only where the second derivative is positive, t clamped to [0, 1])
__device__ __forceinline__ float polish(float t, float2 q0, float2 q1, float2 q2, float2 q3) {
    for (int it = 0; it < STR_NEWTON; ++it) {
        const float m = 1.f - t;
        float cx, cy;
        bezier(t, q0, q1, q2, q3, cx, cy);
        const float a1 = 3.f * m * m, a2 = 6.f * m * t, a3 = 3.f * t * t;
        const float dx = a1 * (q1.x - q0.x) + a2 * (q2.x - q1.x) + a3 * (q3.x - q2.x);
        const float dy = a1 * (q1.y - q0.y) + a2 * (q2.y - q1.y) + a3 * (q3.y - q2.y);
        const float ex = 6.f * (m * (q2.x - 2.f * q1.x + q0.x) + t * (q3.x - 2.f * q2.x + q1.x));
        const float ey = 6.f * (m * (q2.y - 2.f * q1.y + q0.y) + t * (q3.y - 2.f * q2.y + q1.y));
        const float f = cx * dx + cy * dy, fp = dx * dx + dy * dy + cx * ex + cy * ey;
        if (fp > 0.f) t = fminf(fmaxf(t - f / fp, 0.f), 1.f);
    }
    return t;
}

// squared distance from the origin to the segment q0..q3 (control points relative to the sample) and its t: every local
// minimum of the distance over the t grid (a cubic has at most three) is polished, and the best point seen is kept
__device__ __forceinline__ float seg_closest(float2 q0, float2 q1, float2 q2, float2 q3, float& tbest) {
    constexpr float dt = 1.f / STR_TSTEPS;
    float best = STR_INF, dprev = STR_INF, dcur = dist2_at(0.f, q0, q1, q2, q3);
    tbest = 0.f;
    for (int i = 0; i <= STR_TSTEPS; ++i) {
        const float dnext = i < STR_TSTEPS ? dist2_at((float)(i + 1) * dt, q0, q1, q2, q3) : STR_INF;
        if (dcur <= dprev && dcur <= dnext) {
            const float ti = (float)i * dt;
            if (dcur < best) { best = dcur; tbest = ti; }
            const float tp = polish(ti, q0, q1, q2, q3);
            const float dp = dist2_at(tp, q0, q1, q2, q3);
            if (dp < best) { best = dp; tbest = tp; }
        }
        dprev = dcur;
        dcur = dnext;
    }
    return best;
}

__device__ __forceinline__ float2 rel(const float2* __restrict__ pts, int i, float sx, float sy) {
    const float2 p = pts[i];
    return make_float2(p.x - sx, p.y - sy);
}

// closest segment of the path pts[0 .. np) to (sx, sy) among those whose box grown by r holds the sample: squared distance
// (STR_INF if none), the segment (-1 if none) and t
__device__ __forceinline__ float path_closest(const float2* __restrict__ pts, int np, float sx, float sy, float r, int& seg, float& t) {
    float best = STR_INF;
    seg = -1;
    t = 0.f;
    const int nseg = (np - 1) / 3;
    for (int sg = 0; sg < nseg; ++sg) {
        const float2 q0 = rel(pts, 3 * sg, sx, sy), q1 = rel(pts, 3 * sg + 1, sx, sy);
        const float2 q2 = rel(pts, 3 * sg + 2, sx, sy), q3 = rel(pts, 3 * sg + 3, sx, sy);
        if (fminf(fminf(q0.x, q1.x), fminf(q2.x, q3.x)) > r || fmaxf(fmaxf(q0.x, q1.x), fmaxf(q2.x, q3.x)) < -r ||
            fminf(fminf(q0.y, q1.y), fminf(q2.y, q3.y)) > r || fmaxf(fmaxf(q0.y, q1.y), fmaxf(q2.y, q3.y)) < -r)
            continue;
        float ts;
        const float d2 = seg_closest(q0, q1, q2, q3, ts);
        if (d2 < best) { best = d2; seg = sg; t = ts; }
    }
    return best;
}

__device__ __forceinline__ float grow(float w) { return fmaxf(w, 0.f) + 1.f; }

__device__ __forceinline__ float coverage(float w, float d) { return fminf(fmaxf(w - d + 0.5f, 0.f), 1.f); }

// the coverage of sample (sx, sy) by path k
__device__ __forceinline__ float layer_cov(const float2* __restrict__ pts, const int* __restrict__ path_start, int max_points,
                                           const float* __restrict__ widths, int k, float sx, float sy) {
    const int p0 = path_start[k], np = min(path_start[k + 1] - p0, max_points);
    const float w = widths[k];
    int seg;
    float t;
    const float d2 = path_closest(pts + p0, np, sx, sy, grow(w), seg, t);
    return seg < 0 ? 0.f : coverage(w, sqrtf(d2));
}

__device__ __forceinline__ void over(float (&C)[3], float& A, const float* __restrict__ c, float a) {
    const float t = 1.f - a;
    C[0] = a * c[0] + t * C[0];
    C[1] = a * c[1] + t * C[1];
    C[2] = a * c[2] + t * C[2];
    A = a + t * A;
}

__device__ __forceinline__ void paper_state(const float* __restrict__ paper, float (&C)[4][3], float (&A)[4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        C[s][0] = C[s][1] = C[s][2] = 0.f;
        A[s] = 0.f;
        if (paper) over(C[s], A[s], paper, paper[3]);
    }
}

__device__ __forceinline__ bool meets_x(float4 b, int tx) { return b.x <= (float)(tx * STR_TILE + STR_TILE) && b.z >= (float)(tx * STR_TILE); }
__device__ __forceinline__ bool meets_y(float4 b, int ty) { return b.y <= (float)(ty * STR_TILE + STR_TILE) && b.w >= (float)(ty * STR_TILE); }

__global__ __launch_bounds__(256) void str_box_kernel(const float2* __restrict__ pts, const int* __restrict__ path_start, int n,
                                                      int max_points, const float* __restrict__ widths, float4* __restrict__ boxes) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int p0 = path_start[k], np = min(path_start[k + 1] - p0, max_points);
    if (np < 4) {                                                   // no segment: meets no tile
        boxes[k] = make_float4(STR_INF, STR_INF, -STR_INF, -STR_INF);
        return;
    }
    float x0 = STR_INF, y0 = STR_INF, x1 = -STR_INF, y1 = -STR_INF;
    for (int i = 0; i < np; ++i) {
        const float2 p = pts[p0 + i];
        x0 = fminf(x0, p.x); x1 = fmaxf(x1, p.x);
        y0 = fminf(y0, p.y); y1 = fmaxf(y1, p.y);
    }
    const float r = grow(widths[k]);
    boxes[k] = make_float4(x0 - r, y0 - r, x1 + r, y1 + r);
}

__global__ __launch_bounds__(STR_THREADS) void str_cull_kernel(const float4* __restrict__ boxes, int n, int tiles_x,
                                                               int* __restrict__ tile_count, int* __restrict__ tile_paths) {
    __shared__ int wcnt[STR_WAVES];
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int* list = tile_paths + (size_t)blockIdx.x * n;
    int total = 0;
    for (int b = 0; b < n; b += STR_THREADS) {
        const int k = b + threadIdx.x;
        bool hit = false;
        if (k < n) {
            const float4 bx = boxes[k];
            hit = meets_x(bx, tx) && meets_y(bx, ty);
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) wcnt[wid] = __popcll(m);
        __syncthreads();
        int off = total, all = 0;
        for (int q = 0; q < STR_WAVES; ++q) {
            off += q < wid ? wcnt[q] : 0;
            all += wcnt[q];
        }
        if (hit) list[off + __popcll(m & ((1ULL << lane) - 1ULL))] = k;
        total += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

__global__ __launch_bounds__(STR_THREADS) void str_fwd_kernel(const float2* __restrict__ pts, const int* __restrict__ path_start, int n,
                                                              int max_points, const float* __restrict__ widths,
                                                              const float* __restrict__ colors, const float* __restrict__ paper,
                                                              const int* __restrict__ tile_count, const int* __restrict__ tile_paths,
                                                              int w, int h, int tiles_x, const int* __restrict__ seed,
                                                              float* __restrict__ out) {
    const TilePixel P(w, h, tiles_x, (uint32_t)*seed);
    if (!P.live) return;
    float C[4][3], A[4];
    paper_state(paper, C, A);
    const int cnt = tile_count[blockIdx.x];
    const int* list = tile_paths + (size_t)blockIdx.x * n;
    for (int j = 0; j < cnt; ++j) {
        const int k = list[j];
        const float* c = colors + (size_t)k * 4;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float cov = layer_cov(pts, path_start, max_points, widths, k, P.px[s], P.py[s]);
            if (cov > 0.f) over(C[s], A[s], c, c[3] * cov);
        }
    }
    float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const bool un = A[s] > 1e-6f;
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] += un ? C[s][k] / A[s] : C[s][k];
        o[3] += A[s];
    }
    const size_t p = (size_t)P.y * w + P.x;
    *reinterpret_cast<float4*>(out + p * 4) = make_float4(o[0] * 0.25f, o[1] * 0.25f, o[2] * 0.25f, o[3] * 0.25f);
}

// dst[i] += the workgroup's sum of v[i], i < N (lanes in order within a wave, waves in order); all threads call it
template <int N>
__device__ __forceinline__ void block_add(const double (&v)[N], double (*red)[8], double* dst) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double s = wave_sum_d(v[i]);
        if (lane == 0) red[wid][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        double s = 0.0;
        for (int q = 0; q < STR_WAVES; ++q) s += red[q][threadIdx.x];
        dst[threadIdx.x] += s;
    }
    __syncthreads();
}

__device__ __forceinline__ unsigned long long wave_or64(unsigned long long m) {
    unsigned lo = (unsigned)m, hi = (unsigned)(m >> 32);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo |= __shfl_xor(lo, o, 64);
        hi |= __shfl_xor(hi, o, 64);
    }
    return ((unsigned long long)hi << 32) | lo;
}

// d loss / d (premultiplied colour, alpha) of a sample's final state, through the un-premultiply
__device__ __forceinline__ void final_grad(const float* g, const float (&C)[3], float A, float (&gC)[3], float& gA) {
    if (A > 1e-6f) {
        const float ia = 1.f / A;
        gC[0] = g[0] * ia; gC[1] = g[1] * ia; gC[2] = g[2] * ia;
        gA = g[3] - (gC[0] * C[0] + gC[1] * C[1] + gC[2] * C[2]) * ia;
    } else {
        gC[0] = g[0]; gC[1] = g[1]; gC[2] = g[2];
        gA = g[3];
    }
}

__global__ __launch_bounds__(STR_THREADS) void str_bwd_kernel(const float2* __restrict__ pts, const int* __restrict__ path_start, int n,
                                                              int max_points, int slot, const float* __restrict__ widths,
                                                              const float* __restrict__ colors, const float* __restrict__ paper,
                                                              const int* __restrict__ tile_count, const int* __restrict__ tile_paths,
                                                              int w, int h, int tiles_x, const int* __restrict__ seed,
                                                              const float* __restrict__ gout, double* __restrict__ partials,
                                                              double* __restrict__ paper_partials) {
    __shared__ float cov_l[STR_CHUNK][4][STR_THREADS];   // each lane reads back only its own coverages
    __shared__ double red[STR_WAVES][8];
    __shared__ double acc[STR_MAX_SLOT];
    __shared__ unsigned long long red_m[STR_WAVES];
    const TilePixel P(w, h, tiles_x, (uint32_t)*seed);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, tid = threadIdx.x;
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    if (P.live) {
        const size_t p = (size_t)P.y * w + P.x;
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = gout[p * 4 + k] * 0.25f;
    }
    const int cnt = tile_count[blockIdx.x];
    const int* list = tile_paths + (size_t)blockIdx.x * n;
    const int nch = (cnt + STR_CHUNK - 1) / STR_CHUNK;
    float gC[4][3], gA[4];
    if (nch == 0) {
        float C[4][3], A[4];
        paper_state(paper, C, A);
#pragma unroll
        for (int s = 0; s < 4; ++s) final_grad(g, C[s], A[s], gC[s], gA[s]);
    }
    for (int c = nch - 1; c >= 0; --c) {
        float Cs[4][3], As[4];                                   // the state at the start of chunk c
        paper_state(paper, Cs, As);
        for (int j = 0; j < c * STR_CHUNK; ++j) {
            const int k = list[j];
            const float* ck = colors + (size_t)k * 4;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float cov = P.live ? layer_cov(pts, path_start, max_points, widths, k, P.px[s], P.py[s]) : 0.f;
                if (cov > 0.f) over(Cs[s], As[s], ck, ck[3] * cov);
            }
        }
        const int c0 = c * STR_CHUNK, cc = min(STR_CHUNK, cnt - c0);
        for (int j = 0; j < cc; ++j) {
            const int k = list[c0 + j];
#pragma unroll
            for (int s = 0; s < 4; ++s)
                cov_l[j][s][tid] = P.live ? layer_cov(pts, path_start, max_points, widths, k, P.px[s], P.py[s]) : 0.f;
        }
        if (c == nch - 1) {                                      // the final state and d loss / d (C, A) of it
            float C[4][3], A[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) { C[s][0] = Cs[s][0]; C[s][1] = Cs[s][1]; C[s][2] = Cs[s][2]; A[s] = As[s]; }
            for (int j = 0; j < cc; ++j) {
                const float* ck = colors + (size_t)list[c0 + j] * 4;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float cov = cov_l[j][s][tid];
                    if (cov > 0.f) over(C[s], A[s], ck, ck[3] * cov);
                }
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) final_grad(g, C[s], A[s], gC[s], gA[s]);
        }
        for (int j = cc - 1; j >= 0; --j) {
            const int k = list[c0 + j];
            const int p0 = path_start[k], np = min(path_start[k + 1] - p0, max_points);
            const int nvals = 2 * np + 5;
            const float wk = widths[k];
            const float* ck = colors + (size_t)k * 4;
            float Cp[4][3], Ap[4];                               // the state below layer j
#pragma unroll
            for (int s = 0; s < 4; ++s) { Cp[s][0] = Cs[s][0]; Cp[s][1] = Cs[s][1]; Cp[s][2] = Cs[s][2]; Ap[s] = As[s]; }
            for (int i = 0; i < j; ++i) {
                const float* ci = colors + (size_t)list[c0 + i] * 4;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float cov = cov_l[i][s][tid];
                    if (cov > 0.f) over(Cp[s], Ap[s], ci, ci[3] * cov);
                }
            }
            for (int i = tid; i < nvals; i += STR_THREADS) acc[i] = 0.0;
            double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};             // width, RGBA
            float gd[4], ts[4], ex[4], ey[4];
            int sg[4];
            unsigned long long m = 0ULL;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                gd[s] = 0.f; ts[s] = 0.f; ex[s] = 0.f; ey[s] = 0.f; sg[s] = -1;
                const float cov = cov_l[j][s][tid];
                if (!(cov > 0.f)) continue;
                const float a = ck[3] * cov;
                const float galpha = gC[s][0] * (ck[0] - Cp[s][0]) + gC[s][1] * (ck[1] - Cp[s][1]) + gC[s][2] * (ck[2] - Cp[s][2]) +
                                     gA[s] * (1.f - Ap[s]);
                v[1] += (double)(gC[s][0] * a);
                v[2] += (double)(gC[s][1] * a);
                v[3] += (double)(gC[s][2] * a);
                v[4] += (double)(galpha * cov);
                const float gcov = galpha * ck[3];
                int seg;
                float t;
                const float d = sqrtf(path_closest(pts + p0, np, P.px[s], P.py[s], grow(wk), seg, t));
                const float ramp = wk - d + 0.5f;
                if (ramp > 0.f && ramp < 1.f) {
                    v[0] += (double)gcov;
                    if (d > 0.f) {
                        float cx, cy;
                        bezier(t, rel(pts + p0, 3 * seg, P.px[s], P.py[s]), rel(pts + p0, 3 * seg + 1, P.px[s], P.py[s]),
                               rel(pts + p0, 3 * seg + 2, P.px[s], P.py[s]), rel(pts + p0, 3 * seg + 3, P.px[s], P.py[s]), cx, cy);
                        gd[s] = -gcov;
                        ts[s] = t;
                        sg[s] = seg;
                        ex[s] = cx / d;
                        ey[s] = cy / d;
                        m |= 1ULL << seg;
                    }
                }
                const float tr = 1.f - a;
                gC[s][0] *= tr; gC[s][1] *= tr; gC[s][2] *= tr;
                gA[s] *= tr;
            }
            __syncthreads();                                     // acc zeroed
            block_add<5>(v, red, acc + 2 * np);
            m = wave_or64(m);
            if (lane == 0) red_m[wid] = m;
            __syncthreads();
            unsigned long long all = 0ULL;
            for (int q = 0; q < STR_WAVES; ++q) all |= red_m[q];
            for (; all; all &= all - 1ULL) {                     // the segments that are closest for some sample, ascending
                const int q = __builtin_ctzll(all);
                double vp[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    if (sg[s] != q) continue;
                    const float t = ts[s], mt = 1.f - t;
                    const float b[4] = {mt * mt * mt, 3.f * mt * mt * t, 3.f * mt * t * t, t * t * t};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        vp[2 * i] += (double)(gd[s] * b[i] * ex[s]);
                        vp[2 * i + 1] += (double)(gd[s] * b[i] * ey[s]);
                    }
                }
                block_add<8>(vp, red, acc + 6 * q);
            }
            double* dst = partials + ((size_t)blockIdx.x * n + k) * slot;
            for (int i = tid; i < nvals; i += STR_THREADS) dst[i] = acc[i];
            __syncthreads();                                     // acc and red_m read
        }
    }
    if (paper && paper_partials) {                               // the bottom layer: the paper, a = paper.a, coverage 1
        double v[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float a = paper[3];
            v[0] += (double)(gC[s][0] * a);
            v[1] += (double)(gC[s][1] * a);
            v[2] += (double)(gC[s][2] * a);
            v[3] += (double)(gC[s][0] * paper[0] + gC[s][1] * paper[1] + gC[s][2] * paper[2] + gA[s]);
        }
        if (tid < 4) acc[tid] = 0.0;
        __syncthreads();
        block_add<4>(v, red, acc);
        if (tid < 4) paper_partials[(size_t)blockIdx.x * 4 + tid] = acc[tid];
    }
}

// path k's gradient = its (tile, path) slots added in tile order, over the tiles its box meets (the cull's own test)
__global__ __launch_bounds__(256) void str_path_sum_kernel(const double* __restrict__ partials, const float4* __restrict__ boxes,
                                                           const int* __restrict__ path_start, int n, int max_points, int slot,
                                                           int tiles_x, int tiles_y, float* __restrict__ grad_points,
                                                           float* __restrict__ grad_widths, float* __restrict__ grad_colors) {
    const int k = blockIdx.x;
    const int p0 = path_start[k], np = min(path_start[k + 1] - p0, max_points);
    const int nvals = 2 * np + 5;
    const float4 b = boxes[k];
    for (int i = threadIdx.x; i < nvals; i += 256) {
        double v = 0.0;
        for (int ty = 0; ty < tiles_y; ++ty) {
            if (!meets_y(b, ty)) continue;
            for (int tx = 0; tx < tiles_x; ++tx)
                if (meets_x(b, tx)) v += partials[((size_t)(ty * tiles_x + tx) * n + k) * slot + i];
        }
        if (i < 2 * np) grad_points[(size_t)p0 * 2 + i] = (float)v;
        else if (i == 2 * np) grad_widths[k] = (float)v;
        else grad_colors[(size_t)k * 4 + (i - 2 * np - 1)] = (float)v;
    }
}

__global__ __launch_bounds__(64) void str_paper_sum_kernel(const double* __restrict__ paper_partials, int tiles, float* __restrict__ grad) {
    if (threadIdx.x >= 4) return;
    double v = 0.0;
    for (int t = 0; t < tiles; ++t) v += paper_partials[(size_t)t * 4 + threadIdx.x];
    grad[threadIdx.x] = (float)v;
}

__global__ __launch_bounds__(256) void str_offsets_kernel(int w, int h, const int* __restrict__ seed, float* __restrict__ uv) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)w * h * 4) return;
    const int s = (int)(i & 3);
    const long long p = i >> 2;
    const int y = (int)(p / w), x = (int)(p - (long long)y * w);
    float u, v;
    sample_jitter(x, y, w, s, (uint32_t)*seed, u, v);
    uv[2 * i] = u;
    uv[2 * i + 1] = v;
}

int cull(const float* points, const int* path_start, int n, int max_points, const float* widths, int w, int h, float* boxes,
         int* tile_count, int* tile_paths, hipStream_t s) {
    const int tiles_x = (w + STR_TILE - 1) / STR_TILE, tiles_y = (h + STR_TILE - 1) / STR_TILE;
    hipLaunchKernelGGL(str_box_kernel, dim3((n + 255) / 256), dim3(256), 0, s, reinterpret_cast<const float2*>(points), path_start, n,
                       max_points, widths, reinterpret_cast<float4*>(boxes));
    PRX_LAUNCH_CHECK();
    hipLaunchKernelGGL(str_cull_kernel, dim3(tiles_x * tiles_y), dim3(STR_THREADS), 0, s, reinterpret_cast<const float4*>(boxes), n,
                       tiles_x, tile_count, tile_paths);
    PRX_LAUNCH_CHECK();
    return 0;
}

bool canvas_ok(int w, int h) { return w > 0 && h > 0 && (long long)w * h * 4 < (1LL << 31); }

}  // namespace

int str_forward(const float* points, const int* path_start, int n_paths, int max_points, const float* widths, const float* colors,
                const float* paper, int w, int h, const int* seed, float* boxes, int* tile_count, int* tile_paths, float* out,
                hipStream_t s) {
    PRX_REQUIRE(points && path_start && widths && colors && seed && boxes && tile_count && tile_paths && out,
                "stroke raster: null argument");
    PRX_REQUIRE(canvas_ok(w, h) && n_paths > 0 && max_points >= 1 && max_points <= STR_MAX_POINTS,
                "stroke raster: canvas %d x %d, %d paths, %d points per path (at most %d)", w, h, n_paths, max_points, STR_MAX_POINTS);
    if (int rc = cull(points, path_start, n_paths, max_points, widths, w, h, boxes, tile_count, tile_paths, s)) return rc;
    const int tiles_x = (w + STR_TILE - 1) / STR_TILE, tiles_y = (h + STR_TILE - 1) / STR_TILE;
    hipLaunchKernelGGL(str_fwd_kernel, dim3(tiles_x * tiles_y), dim3(STR_THREADS), 0, s, reinterpret_cast<const float2*>(points),
                       path_start, n_paths, max_points, widths, colors, paper, tile_count, tile_paths, w, h, tiles_x, seed, out);
    PRX_LAUNCH_CHECK();
    return 0;
}

int str_backward(const float* points, const int* path_start, int n_paths, int max_points, const float* widths, const float* colors,
                 const float* paper, int w, int h, const int* seed, const float* gout, float* boxes, int* tile_count,
                 int* tile_paths, double* partials, double* paper_partials, float* grad_points, float* grad_widths,
                 float* grad_colors, float* grad_paper, hipStream_t s) {
    PRX_REQUIRE(points && path_start && widths && colors && seed && gout && boxes && tile_count && tile_paths && partials &&
                grad_points && grad_widths && grad_colors, "stroke raster backward: null argument");
    PRX_REQUIRE(!grad_paper || (paper && paper_partials), "stroke raster backward: a paper gradient needs the paper and its partials");
    PRX_REQUIRE(canvas_ok(w, h) && n_paths > 0 && max_points >= 1 && max_points <= STR_MAX_POINTS,
                "stroke raster backward: canvas %d x %d, %d paths, %d points per path (at most %d)", w, h, n_paths, max_points,
                STR_MAX_POINTS);
    if (int rc = cull(points, path_start, n_paths, max_points, widths, w, h, boxes, tile_count, tile_paths, s)) return rc;
    const int tiles_x = (w + STR_TILE - 1) / STR_TILE, tiles_y = (h + STR_TILE - 1) / STR_TILE;
    const int slot = 2 * max_points + 5;
    double* pp = grad_paper ? paper_partials : nullptr;
    hipLaunchKernelGGL(str_bwd_kernel, dim3(tiles_x * tiles_y), dim3(STR_THREADS), 0, s, reinterpret_cast<const float2*>(points),
                       path_start, n_paths, max_points, slot, widths, colors, paper, tile_count, tile_paths, w, h, tiles_x, seed, gout,
                       partials, pp);
    PRX_LAUNCH_CHECK();
    hipLaunchKernelGGL(str_path_sum_kernel, dim3(n_paths), dim3(256), 0, s, partials, reinterpret_cast<const float4*>(boxes), path_start,
                       n_paths, max_points, slot, tiles_x, tiles_y, grad_points, grad_widths, grad_colors);
    PRX_LAUNCH_CHECK();
    if (grad_paper) {
        hipLaunchKernelGGL(str_paper_sum_kernel, dim3(1), dim3(64), 0, s, paper_partials, tiles_x * tiles_y, grad_paper);
        PRX_LAUNCH_CHECK();
    }
    return 0;
}

int str_sample_offsets(int w, int h, const int* seed, float* uv, hipStream_t s) {
    PRX_REQUIRE(seed && uv && canvas_ok(w, h), "stroke sample offsets: bad arguments");
    hipLaunchKernelGGL(str_offsets_kernel, dim3((unsigned)(((long long)w * h * 4 + 255) / 256)), dim3(256), 0, s, w, h, seed, uv);
    PRX_LAUNCH_CHECK();
    return 0;
}

#define S_(x) ((hipStream_t)(x))
extern "C" {
int prx_stroke_raster_fwd(const float* points, const int* path_start, int n_paths, int max_points, const float* widths,
                          const float* colors, const float* paper, int w, int h, const int* seed, float* boxes, int* tile_count,
                          int* tile_paths, float* out, prx_stream_t s) {
    return str_forward(points, path_start, n_paths, max_points, widths, colors, paper, w, h, seed, boxes, tile_count, tile_paths, out,
                       S_(s));
}
int prx_stroke_raster_bwd(const float* points, const int* path_start, int n_paths, int max_points, const float* widths,
                          const float* colors, const float* paper, int w, int h, const int* seed, const float* gout, float* boxes,
                          int* tile_count, int* tile_paths, double* partials, double* paper_partials, float* grad_points,
                          float* grad_widths, float* grad_colors, float* grad_paper, prx_stream_t s) {
    return str_backward(points, path_start, n_paths, max_points, widths, colors, paper, w, h, seed, gout, boxes, tile_count, tile_paths,
                        partials, paper_partials, grad_points, grad_widths, grad_colors, grad_paper, S_(s));
}
int prx_stroke_sample_offsets(int w, int h, const int* seed, float* uv, prx_stream_t s) {
    return str_sample_offsets(w, h, seed, uv, S_(s));
}
}
