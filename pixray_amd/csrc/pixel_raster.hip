// The pixel drawer's renderer (pixray pixeldrawer.py renders a grid of filled polygons with diffvg): every pixel is the mean of
// 2 x 2 stratified, jittered samples; a sample is inside a polygon by the nonzero winding rule; the shapes covering a sample are
// composited in index order with "over" (premultiplied C = a c + (1 - a) C, A = a + (1 - a) A) and un-premultiplied per sample
// when A > 1e-6; an uncovered sample is (0, 0, 0, 0).
//
// Jitter: PCG32 per sample, idx = ((y W + x) 2 + sy) 2 + sx, inc = idx << 1 | 1, one step, state += seed, one step, then u and v as
// ((r >> 9) | 0x3f800000) - 1.  The sample sits at (x + (sx + u) / 2, y + (sy + v) / 2), in fp32.  The seed is read from a
// one-word device buffer, so a captured graph replays with whatever the host staged there.
//
// Layout: the host sorts the (fixed) shapes into 16 x 16-pixel tiles by bounding box (CSR tile_start / tile_shapes, ascending
// shape ids per tile).  One workgroup per tile, one pixel per lane; the tile's shapes pass through LDS in chunks of 64.
// Backward (colours only; the geometry is fixed): the same tiles write one row of 4 partial sums per (tile, slot) entry, reduced
// across the workgroup in a fixed order; a second launch adds each shape's rows in tile order (CSR shape_start / shape_entries).
// No float atomics: a run repeats bit for bit.
#include "pixel_raster.h"
#include "../../include/prx.h"

namespace {

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

// nonzero winding number of (px, py) against the closed polygon v[0..nv)
__device__ __forceinline__ bool inside(const float2* __restrict__ v, int nv, float px, float py) {
    int wn = 0;
    float2 a = v[nv - 1];
    for (int k = 0; k < nv; ++k) {
        const float2 b = v[k];
        const float is_left = (b.x - a.x) * (py - a.y) - (px - a.x) * (b.y - a.y);
        if (a.y <= py) {
            if (b.y > py && is_left > 0.f) ++wn;
        } else if (b.y <= py && is_left < 0.f) {
            --wn;
        }
        a = b;
    }
    return wn != 0;
}

struct Chunk {
    float2 v[PXR_CHUNK][PXR_MAXV];
    float c[PXR_CHUNK][4];
    int n[PXR_CHUNK];
    int id[PXR_CHUNK];
};

// tile entries [e0, e0 + cnt) -> LDS (callers put a barrier before, for the previous chunk's readers, and after)
__device__ __forceinline__ void load_chunk(Chunk& ch, const float2* __restrict__ verts, const int* __restrict__ nverts,
                                           const float* __restrict__ colors, const int* __restrict__ tile_shapes, int e0, int cnt) {
    for (int i = threadIdx.x; i < cnt * PXR_MAXV; i += PXR_THREADS) {
        const int j = i / PXR_MAXV, k = i - j * PXR_MAXV;
        ch.v[j][k] = verts[(size_t)tile_shapes[e0 + j] * PXR_MAXV + k];
    }
    for (int i = threadIdx.x; i < cnt * 4; i += PXR_THREADS) {
        const int j = i >> 2;
        ch.c[j][i & 3] = colors[(size_t)tile_shapes[e0 + j] * 4 + (i & 3)];
    }
    for (int j = threadIdx.x; j < cnt; j += PXR_THREADS) {
        const int id = tile_shapes[e0 + j];
        const int nv = nverts[id];
        ch.n[j] = nv < 3 ? 0 : (nv > PXR_MAXV ? PXR_MAXV : nv);       // fewer than 3 vertices cover nothing
        ch.id[j] = id;
    }
}

__device__ __forceinline__ void over(float (&C)[3], float& A, const float* __restrict__ c) {
    const float a = c[3], t = 1.f - a;
    C[0] = a * c[0] + t * C[0];
    C[1] = a * c[1] + t * C[1];
    C[2] = a * c[2] + t * C[2];
    A = a + t * A;
}

struct TilePixel {
    int x, y;
    bool live;
    float px[4], py[4];
    __device__ TilePixel(int w, int h, int tiles_x, uint32_t seed) {
        const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
        x = tx * PXR_TILE + (threadIdx.x % PXR_TILE);
        y = ty * PXR_TILE + (threadIdx.x / PXR_TILE);
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

__global__ __launch_bounds__(PXR_THREADS) void pxr_fwd_kernel(const float2* __restrict__ verts, const int* __restrict__ nverts,
                                                              const float* __restrict__ colors, const int* __restrict__ tile_start,
                                                              const int* __restrict__ tile_shapes, int w, int h, int tiles_x,
                                                              const int* __restrict__ seed, float* __restrict__ out,
                                                              int* __restrict__ ids) {
    __shared__ Chunk ch;
    const TilePixel P(w, h, tiles_x, (uint32_t)*seed);
    float C[4][3], A[4];
    int top[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) { C[s][0] = C[s][1] = C[s][2] = 0.f; A[s] = 0.f; top[s] = -1; }
    const int e0 = tile_start[blockIdx.x], e1 = tile_start[blockIdx.x + 1];
    for (int base = e0; base < e1; base += PXR_CHUNK) {
        const int cnt = min(PXR_CHUNK, e1 - base);
        __syncthreads();
        load_chunk(ch, verts, nverts, colors, tile_shapes, base, cnt);
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const int nv = ch.n[j];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (nv && inside(ch.v[j], nv, P.px[s], P.py[s])) {
                    over(C[s], A[s], ch.c[j]);
                    top[s] = ch.id[j];
                }
            }
        }
    }
    if (!P.live) return;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const bool un = A[s] > 1e-6f;
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] += un ? C[s][k] / A[s] : C[s][k];
        o[3] += A[s];
    }
    const size_t hw = (size_t)w * h, p = (size_t)P.y * w + P.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k * hw + p] = o[k] * 0.25f;
    if (ids) {
#pragma unroll
        for (int s = 0; s < 4; ++s) ids[p * 4 + s] = top[s];
    }
}

// d loss / d colour.  Per sample, with the chunks of the tile taken last to first: the state the samples had when the chunk began
// (recomposited from the earlier chunks), the chunk's coverage bits, then its slots last to first.  The running gC, gA are
// d loss / d (premultiplied colour, alpha) of the state after the slot; the state before it is recomposited from the chunk-start
// state over the lower coverage bits (a handful per sample).  Each slot's 4 sums leave through a fixed-order workgroup reduction.
__global__ __launch_bounds__(PXR_THREADS) void pxr_bwd_kernel(const float2* __restrict__ verts, const int* __restrict__ nverts,
                                                              const float* __restrict__ colors, const int* __restrict__ tile_start,
                                                              const int* __restrict__ tile_shapes, int w, int h, int tiles_x,
                                                              const int* __restrict__ seed, const float* __restrict__ gout,
                                                              double* __restrict__ partials) {
    __shared__ Chunk ch;
    __shared__ double red[PXR_THREADS / 64][4];
    const TilePixel P(w, h, tiles_x, (uint32_t)*seed);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int e0 = tile_start[blockIdx.x], e1 = tile_start[blockIdx.x + 1];
    const int nch = (e1 - e0 + PXR_CHUNK - 1) / PXR_CHUNK;
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    if (P.live) {
        const size_t hw = (size_t)w * h, p = (size_t)P.y * w + P.x;
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = gout[k * hw + p] * 0.25f;
    }
    float gC[4][3], gA[4];
    for (int c = nch - 1; c >= 0; --c) {
        float C0[4][3], A0[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) { C0[s][0] = C0[s][1] = C0[s][2] = 0.f; A0[s] = 0.f; }
        for (int pc = 0; pc < c; ++pc) {                        // the state at the start of chunk c
            const int base = e0 + pc * PXR_CHUNK;
            __syncthreads();
            load_chunk(ch, verts, nverts, colors, tile_shapes, base, PXR_CHUNK);
            __syncthreads();
            for (int j = 0; j < PXR_CHUNK; ++j) {
                const int nv = ch.n[j];
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    if (nv && inside(ch.v[j], nv, P.px[s], P.py[s])) over(C0[s], A0[s], ch.c[j]);
            }
        }
        const int base = e0 + c * PXR_CHUNK, cnt = min(PXR_CHUNK, e1 - base);
        __syncthreads();
        load_chunk(ch, verts, nverts, colors, tile_shapes, base, cnt);
        __syncthreads();
        uint64_t m[4] = {0ULL, 0ULL, 0ULL, 0ULL};
        if (P.live) {
            for (int j = 0; j < cnt; ++j) {
                const int nv = ch.n[j];
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    if (nv && inside(ch.v[j], nv, P.px[s], P.py[s])) m[s] |= 1ULL << j;
            }
        }
        if (c == nch - 1) {                                     // the final state and d loss / d (C, A) of it
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                float C[3] = {C0[s][0], C0[s][1], C0[s][2]}, A = A0[s];
                for (uint64_t b = m[s]; b; b &= b - 1) over(C, A, ch.c[__builtin_ctzll(b)]);
                if (A > 1e-6f) {
                    const float ia = 1.f / A;
                    gC[s][0] = g[0] * ia; gC[s][1] = g[1] * ia; gC[s][2] = g[2] * ia;
                    gA[s] = g[3] - (gC[s][0] * C[0] + gC[s][1] * C[1] + gC[s][2] * C[2]) * ia;
                } else {
                    gC[s][0] = g[0]; gC[s][1] = g[1]; gC[s][2] = g[2];
                    gA[s] = g[3];
                }
            }
        }
        for (int j = cnt - 1; j >= 0; --j) {
            float d[4] = {0.f, 0.f, 0.f, 0.f};
            const float* cj = ch.c[j];
            const float a = cj[3], t = 1.f - a;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (!((m[s] >> j) & 1ULL)) continue;
                float Cp[3] = {C0[s][0], C0[s][1], C0[s][2]}, Ap = A0[s];
                for (uint64_t b = m[s] & ((1ULL << j) - 1ULL); b; b &= b - 1) over(Cp, Ap, ch.c[__builtin_ctzll(b)]);
                d[0] += gC[s][0] * a;
                d[1] += gC[s][1] * a;
                d[2] += gC[s][2] * a;
                d[3] += gC[s][0] * (cj[0] - Cp[0]) + gC[s][1] * (cj[1] - Cp[1]) + gC[s][2] * (cj[2] - Cp[2]) + gA[s] * (1.f - Ap);
                gC[s][0] *= t; gC[s][1] *= t; gC[s][2] *= t;
                gA[s] *= t;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double v = wave_sum_d((double)d[k]);
                if (lane == 0) red[wid][k] = v;
            }
            __syncthreads();
            if (threadIdx.x < 4) {
                double v = 0.0;
                for (int q = 0; q < PXR_THREADS / 64; ++q) v += red[q][threadIdx.x];
                partials[(size_t)(base + j) * 4 + threadIdx.x] = v;
            }
            __syncthreads();
        }
    }
}

// grad[k] = the shape's (tile, slot) rows in tile order
__global__ __launch_bounds__(256) void pxr_shape_sum_kernel(const double* __restrict__ partials, const int* __restrict__ shape_start,
                                                            const int* __restrict__ shape_entries, int n_shapes,
                                                            float* __restrict__ grad) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_shapes * 4) return;
    const int k = i >> 2, ch = i & 3;
    double v = 0.0;
    for (int e = shape_start[k]; e < shape_start[k + 1]; ++e) v += partials[(size_t)shape_entries[e] * 4 + ch];
    grad[i] = (float)v;
}

__global__ __launch_bounds__(256) void pxr_offsets_kernel(int w, int h, const int* __restrict__ seed, float* __restrict__ uv) {
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

int tiles_of(int w, int h) { return ((w + PXR_TILE - 1) / PXR_TILE) * ((h + PXR_TILE - 1) / PXR_TILE); }

}  // namespace

int pxr_forward(const float* verts, const int* nverts, const float* colors, const int* tile_start, const int* tile_shapes, int w,
                int h, const int* seed, float* out, int* ids, hipStream_t s) {
    PRX_REQUIRE(verts && nverts && colors && tile_start && tile_shapes && seed && out, "pixel raster: null argument");
    PRX_REQUIRE(w > 0 && h > 0 && (long long)w * h * 4 < (1LL << 31), "pixel raster: canvas %d x %d", w, h);
    const int tiles_x = (w + PXR_TILE - 1) / PXR_TILE;
    hipLaunchKernelGGL(pxr_fwd_kernel, dim3(tiles_of(w, h)), dim3(PXR_THREADS), 0, s, reinterpret_cast<const float2*>(verts), nverts,
                       colors, tile_start, tile_shapes, w, h, tiles_x, seed, out, ids);
    PRX_LAUNCH_CHECK();
    return 0;
}

int pxr_backward(const float* verts, const int* nverts, const float* colors, const int* tile_start, const int* tile_shapes, int w,
                 int h, const int* seed, const float* gout, double* partials, const int* shape_start, const int* shape_entries,
                 int n_shapes, float* grad, hipStream_t s) {
    PRX_REQUIRE(verts && nverts && colors && tile_start && tile_shapes && seed && gout && partials && shape_start && shape_entries &&
                grad, "pixel raster backward: null argument");
    PRX_REQUIRE(w > 0 && h > 0 && (long long)w * h * 4 < (1LL << 31) && n_shapes > 0, "pixel raster backward: canvas %d x %d, %d shapes",
                w, h, n_shapes);
    const int tiles_x = (w + PXR_TILE - 1) / PXR_TILE;
    hipLaunchKernelGGL(pxr_bwd_kernel, dim3(tiles_of(w, h)), dim3(PXR_THREADS), 0, s, reinterpret_cast<const float2*>(verts), nverts,
                       colors, tile_start, tile_shapes, w, h, tiles_x, seed, gout, partials);
    PRX_LAUNCH_CHECK();
    hipLaunchKernelGGL(pxr_shape_sum_kernel, dim3((n_shapes * 4 + 255) / 256), dim3(256), 0, s, partials, shape_start, shape_entries,
                       n_shapes, grad);
    PRX_LAUNCH_CHECK();
    return 0;
}

int pxr_sample_offsets(int w, int h, const int* seed, float* uv, hipStream_t s) {
    PRX_REQUIRE(seed && uv && w > 0 && h > 0 && (long long)w * h * 4 < (1LL << 31), "pixel sample offsets: bad arguments");
    hipLaunchKernelGGL(pxr_offsets_kernel, dim3((unsigned)(((long long)w * h * 4 + 255) / 256)), dim3(256), 0, s, w, h, seed, uv);
    PRX_LAUNCH_CHECK();
    return 0;
}

#define S_(x) ((hipStream_t)(x))
extern "C" {
int prx_pixel_raster_fwd(const float* verts, const int* nverts, const float* colors, const int* tile_start, const int* tile_shapes,
                         int w, int h, const int* seed, float* out, int* ids, prx_stream_t s) {
    return pxr_forward(verts, nverts, colors, tile_start, tile_shapes, w, h, seed, out, ids, S_(s));
}
int prx_pixel_raster_bwd(const float* verts, const int* nverts, const float* colors, const int* tile_start, const int* tile_shapes,
                         int w, int h, const int* seed, const float* gout, double* partials, const int* shape_start,
                         const int* shape_entries, int n_shapes, float* grad, prx_stream_t s) {
    return pxr_backward(verts, nverts, colors, tile_start, tile_shapes, w, h, seed, gout, partials, shape_start, shape_entries,
                        n_shapes, grad, S_(s));
}
int prx_pixel_sample_offsets(int w, int h, const int* seed, float* uv, prx_stream_t s) {
    return pxr_sample_offsets(w, h, seed, uv, S_(s));
}
}
