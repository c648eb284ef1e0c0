// Built-in image filters of pixray (filters/colorlookup.py, tiler.py, wallpaper.py).
// lookup: nearest palette colour per pixel with the straight-through value x + (q - x), its commitment loss and that loss's local
//         gradient from one launch.
// tiler / wallpaper: one gather per direction.  The random shifts are read from a 2-word device buffer {rand_h, rand_w}, so a
//         captured graph replays with whatever the host staged there; the backward is the adjoint gather (in `shift` mode each
//         source pixel feeds two outputs, added in a fixed order -- no scatter, no atomics).  The `--wallpaper_edge_match` seam
//         loss leaves the forward launch (plug_reduce); its gradient is added by the backward launch.
#include "plugin_filters.h"
#include "../../include/prx.h"

namespace {

constexpr int LOOKUP_MAX_PALETTE = 256;
__global__ __launch_bounds__(PLUG_THREADS) void color_lookup_kernel(const float* __restrict__ x, int b, int c, int hw,
                                                                    const float* __restrict__ palette, int np, float beta,
                                                                    double* __restrict__ partials, float* __restrict__ out,
                                                                    float* __restrict__ lgrad, float* __restrict__ loss,
                                                                    unsigned* __restrict__ ticket) {
    __shared__ float pal[LOOKUP_MAX_PALETTE * 3];
    for (int i = threadIdx.x; i < np * 3; i += PLUG_THREADS) pal[i] = palette[i];
    __syncthreads();
    const long long N = (long long)b * hw;
    const float gs = 2.f * beta / (float)(N * 3);
    double v[1] = {0.0};
    for (long long p = (long long)blockIdx.x * PLUG_THREADS + threadIdx.x; p < N; p += (long long)gridDim.x * PLUG_THREADS) {
        const long long bi = p / hw, q = p - bi * hw;
        const size_t base = (size_t)bi * c * hw + q;
        const float px[3] = {x[base], x[base + hw], x[base + 2 * hw]};
        float best = INFINITY;
        int k = 0;
        for (int j = 0; j < np; ++j) {
            const float d0 = px[0] - pal[3 * j], d1 = px[1] - pal[3 * j + 1], d2 = px[2] - pal[3 * j + 2];
            const float d = d0 * d0 + d1 * d1 + d2 * d2;
            if (d < best) { best = d; k = j; }
        }
        for (int ch = 0; ch < 3; ++ch) {
            const float qv = pal[3 * k + ch], dv = qv - px[ch];
            out[base + (size_t)ch * hw] = px[ch] + dv;            // z3 + (z_q - z3).detach(), the reference's rounding
            lgrad[base + (size_t)ch * hw] = -gs * dv;
            v[0] += (double)dv * dv;
        }
        if (c == 4) { out[base + 3 * (size_t)hw] = x[base + 3 * (size_t)hw]; lgrad[base + 3 * (size_t)hw] = 0.f; }
    }
    if (plug_reduce<1>(v, partials, ticket)) {
        const float m = (float)(v[0] / (double)(N * 3));
        *loss = beta * m + m;
    }
}

__device__ __forceinline__ int pmod(int a, int m) { a %= m; return a < 0 ? a + m : a; }

struct WallGeom {
    int h, w, mode, em;
    int th, tw, ho, wo, rh, rw;        // trim offsets, output size, effective shifts
    bool hseam, vseam;
    int vc0, vc1;                      // columns the vertical seam covers
    double ch, cv;                     // 1 / (elements * em) of the two seam terms
    __device__ WallGeom(int planes, int h_, int w_, int mode_, int em_, const int* shifts) : h(h_), w(w_), mode(mode_), em(em_) {
        const int em2 = em / 2;
        th = (em > 0 && (mode == PRX_WALL_BOTH || mode == PRX_WALL_VERTICAL)) ? em2 : 0;
        tw = (em > 0 && (mode == PRX_WALL_BOTH || mode == PRX_WALL_HORIZONTAL)) ? em2 : 0;
        if (mode == PRX_WALL_SHIFT) { th = tw = 0; }
        ho = mode == PRX_WALL_SHIFT ? 2 * h : h - 2 * th;
        wo = w - 2 * tw;
        rh = mode == PRX_WALL_HORIZONTAL ? 0 : pmod(shifts[0], ho);
        rw = mode == PRX_WALL_VERTICAL ? 0 : pmod(shifts[1], wo);
        hseam = em > 0 && (mode == PRX_WALL_BOTH || mode == PRX_WALL_HORIZONTAL);
        vseam = em > 0 && (mode == PRX_WALL_BOTH || mode == PRX_WALL_VERTICAL);
        vc0 = tw; vc1 = w - tw;
        ch = hseam ? 1.0 / ((double)planes * h * em * em) : 0.0;
        cv = vseam ? 1.0 / ((double)planes * em * (vc1 - vc0) * em) : 0.0;
    }
};

__global__ __launch_bounds__(PLUG_THREADS) void wallpaper_fwd_kernel(const float* __restrict__ x, int planes, int h, int w, int mode,
                                                                     int em, const int* __restrict__ shifts,
                                                                     double* __restrict__ partials, float* __restrict__ out,
                                                                     float* __restrict__ loss, unsigned* __restrict__ ticket) {
    const WallGeom G(planes, h, w, mode, em, shifts);
    const long long No = (long long)planes * G.ho * G.wo;
    const long long stride = (long long)gridDim.x * PLUG_THREADS, first = (long long)blockIdx.x * PLUG_THREADS + threadIdx.x;
    for (long long e = first; e < No; e += stride) {
        const long long pl = e / ((long long)G.ho * G.wo);
        const int rem = (int)(e - pl * G.ho * G.wo), oy = rem / G.wo, ox = rem - oy * G.wo;
        int sy = pmod(oy - G.rh, G.ho), sx = pmod(ox - G.rw, G.wo);
        if (mode == PRX_WALL_SHIFT) {
            if (sy >= h) { sy -= h; sx = pmod(sx - w / 2, w); }     // second row: the image rolled by half its width
        } else {
            sy += G.th; sx += G.tw;
        }
        out[e] = x[((size_t)pl * h + sy) * w + sx];
    }
    double v[2] = {0.0, 0.0};
    if (G.hseam) {
        const long long Ns = (long long)planes * h * em;
        for (long long e = first; e < Ns; e += stride) {
            const long long row = e / em;
            const int j = (int)(e - row * em);
            const float d = x[row * w + j] - x[row * w + (w - em + j)];
            v[0] += (double)d * d;
        }
    }
    if (G.vseam) {
        const int nc = G.vc1 - G.vc0;
        const long long Ns = (long long)planes * em * nc;
        for (long long e = first; e < Ns; e += stride) {
            const long long pl = e / ((long long)em * nc);
            const int rem = (int)(e - pl * em * nc), j = rem / nc, cx = G.vc0 + (rem - j * nc);
            const float d = x[((size_t)pl * h + j) * w + cx] - x[((size_t)pl * h + (h - em + j)) * w + cx];
            v[1] += (double)d * d;
        }
    }
    if (plug_reduce<2>(v, partials, ticket)) *loss = (float)(v[0] * G.ch) + (float)(v[1] * G.cv);
}

__global__ __launch_bounds__(PLUG_THREADS) void wallpaper_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gout,
                                                                     int planes, int h, int w, int mode, int em,
                                                                     const int* __restrict__ shifts, const float* __restrict__ gloss,
                                                                     float* __restrict__ grad) {
    const WallGeom G(planes, h, w, mode, em, shifts);
    const float gl = gloss ? *gloss : 0.f;
    const float kh = (float)(2.0 * G.ch) * gl, kv = (float)(2.0 * G.cv) * gl;
    const long long N = (long long)planes * h * w;
    for (long long e = (long long)blockIdx.x * PLUG_THREADS + threadIdx.x; e < N; e += (long long)gridDim.x * PLUG_THREADS) {
        const long long pl = e / ((long long)h * w);
        const int rem = (int)(e - pl * h * w), y = rem / w, xx = rem - y * w;
        const float* go = gout + (size_t)pl * G.ho * G.wo;
        float g = 0.f;
        if (mode == PRX_WALL_SHIFT) {
            g = go[(size_t)pmod(y + G.rh, G.ho) * G.wo + pmod(xx + G.rw, G.wo)];
            g += go[(size_t)pmod(y + h + G.rh, G.ho) * G.wo + pmod(pmod(xx + w / 2, w) + G.rw, G.wo)];
        } else {
            const int ty = y - G.th, tx = xx - G.tw;
            if (ty >= 0 && ty < G.ho && tx >= 0 && tx < G.wo) g = go[(size_t)pmod(ty + G.rh, G.ho) * G.wo + pmod(tx + G.rw, G.wo)];
        }
        const float* xp = x + (size_t)pl * h * w;
        if (G.hseam) {
            if (xx < em) g += kh * (xp[(size_t)y * w + xx] - xp[(size_t)y * w + (w - em + xx)]);
            if (xx >= w - em) g -= kh * (xp[(size_t)y * w + (xx - (w - em))] - xp[(size_t)y * w + xx]);
        }
        if (G.vseam && xx >= G.vc0 && xx < G.vc1) {
            if (y < em) g += kv * (xp[(size_t)y * w + xx] - xp[(size_t)(h - em + y) * w + xx]);
            if (y >= h - em) g -= kv * (xp[(size_t)(y - (h - em)) * w + xx] - xp[(size_t)y * w + xx]);
        }
        grad[e] = g;
    }
}

}  // namespace

int plug_color_lookup(const float* x, int b, int c, int hw, const float* palette, int np, float beta, double* partials, float* out,
                      float* lgrad, float* loss, unsigned* ticket, hipStream_t s) {
    PRX_REQUIRE(x && palette && partials && out && lgrad && loss && ticket && b > 0 && hw > 0 && (c == 3 || c == 4),
                "color lookup: bad arguments (channels %d)", c);
    PRX_REQUIRE(np >= 1 && np <= LOOKUP_MAX_PALETTE, "color lookup: %d palette entries (1 .. %d supported)", np, LOOKUP_MAX_PALETTE);
    hipLaunchKernelGGL(color_lookup_kernel, dim3(plug_blocks((long long)b * hw)), dim3(PLUG_THREADS), 0, s, x, b, c, hw, palette, np,
                       beta, partials, out, lgrad, loss, ticket);
    PRX_LAUNCH_CHECK();
    return 0;
}

static bool wall_args_ok(int planes, int h, int w, int mode, int em) {
    if (planes <= 0 || h <= 0 || w <= 0 || mode < PRX_WALL_BOTH || mode > PRX_WALL_SHIFT || em < 0) return false;
    if (em == 0 || mode == PRX_WALL_SHIFT) return true;
    const bool hz = mode != PRX_WALL_VERTICAL, vt = mode != PRX_WALL_HORIZONTAL;
    return em >= 2 && (!hz || 2 * em <= w) && (!vt || 2 * em <= h);
}

int plug_wallpaper_fwd(const float* x, int planes, int h, int w, int mode, int em, const int* shifts, double* partials, float* out,
                       float* loss, unsigned* ticket, hipStream_t s) {
    PRX_REQUIRE(x && shifts && partials && out && loss && ticket, "wallpaper: null argument");
    PRX_REQUIRE(wall_args_ok(planes, h, w, mode, em), "wallpaper: mode %d, edge match %d on %d x %d", mode, em, h, w);
    hipLaunchKernelGGL(wallpaper_fwd_kernel, dim3(plug_blocks((long long)planes * h * w)), dim3(PLUG_THREADS), 0, s, x, planes, h, w,
                       mode, em, shifts, partials, out, loss, ticket);
    PRX_LAUNCH_CHECK();
    return 0;
}
int plug_wallpaper_bwd(const float* x, const float* gout, int planes, int h, int w, int mode, int em, const int* shifts,
                       const float* gloss, float* grad, hipStream_t s) {
    PRX_REQUIRE(x && gout && shifts && grad, "wallpaper backward: null argument");
    PRX_REQUIRE(wall_args_ok(planes, h, w, mode, em), "wallpaper backward: mode %d, edge match %d on %d x %d", mode, em, h, w);
    hipLaunchKernelGGL(wallpaper_bwd_kernel, dim3(plug_blocks((long long)planes * h * w)), dim3(PLUG_THREADS), 0, s, x, gout, planes, h,
                       w, mode, em, shifts, gloss, grad);
    PRX_LAUNCH_CHECK();
    return 0;
}

#define S_(x) ((hipStream_t)(x))
extern "C" {
int prx_color_lookup_fwd(const float* x, int b, int c, int hw, const float* palette, int np, float beta, double* partials, float* out,
                         float* lgrad, float* loss, unsigned* ticket, prx_stream_t s) {
    return plug_color_lookup(x, b, c, hw, palette, np, beta, partials, out, lgrad, loss, ticket, S_(s));
}
int prx_wallpaper_fwd(const float* x, int planes, int h, int w, int mode, int em, const int* shifts, double* partials, float* out,
                      float* loss, unsigned* ticket, prx_stream_t s) {
    return plug_wallpaper_fwd(x, planes, h, w, mode, em, shifts, partials, out, loss, ticket, S_(s));
}
int prx_wallpaper_bwd(const float* x, const float* gout, int planes, int h, int w, int mode, int em, const int* shifts,
                      const float* gloss, float* grad, prx_stream_t s) {
    return plug_wallpaper_bwd(x, gout, planes, h, w, mode, em, shifts, gloss, grad, S_(s));
}
}
