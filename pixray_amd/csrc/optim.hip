// The `--optimiser` rules besides plain Adam (pixray.py:520-555): AdamW, Adagrad, Adamax (torch.optim defaults), DiffGrad and
// AdamP (torch_optimizer defaults, restated from the papers: Dubey et al. 2019; Heo et al., ICLR 2021), each fused with
// VqganDrawer.clip_z (vqgan.py:202-204).  Plain Adam stays in elementwise.hip (adam_clamp_kernel).
#include "optim.h"
#include <algorithm>

namespace {

// Channel (i / hw) % C of an element index that advances by a fixed stride: both divisions are done once per thread.
struct ChanIter {
    int r, ch, dr, dch, hw, C;
    __device__ __forceinline__ void init(size_t i, size_t stride, int hw_, int C_) {
        hw = hw_; C = C_;
        const size_t q = i / hw, dq = stride / hw;
        r = (int)(i - q * hw); ch = (int)(q % C);
        dr = (int)(stride - dq * hw); dch = (int)(dq % C);
    }
    __device__ __forceinline__ void next() {
        r += dr; ch += dch;
        if (r >= hw) { r -= hw; ++ch; }
        if (ch >= C) ch -= C;
    }
};

struct RuleArgs {
    float h0, h1, h2;             // hyper[0..2] (optim.h)
    float b1, omb1, b2, omb2;     // beta and 1 - beta, each rounded from the double on the host (1.f - 0.999f is off by 1.3e-5)
    float eps;
};

// One element of one rule; a / b / c are the rule's state tensors (optim.h).  Returns the new p before the clamp.
template <int RULE>
__device__ __forceinline__ float rule_step(float p, float& a, float& b, float& c, float g, const RuleArgs& k) {
    if (RULE == PRX_OPT_ADAMW) {            // torch.optim.AdamW: decoupled decay, then Adam's update
        p *= k.h2;
        a = a + k.omb1 * (g - a);           // exp_avg.lerp_(grad, 1 - beta1)
        b = k.b2 * b + k.omb2 * g * g;
        return p - k.h0 * (a / (sqrtf(b) / k.h1 + k.eps));
    } else if (RULE == PRX_OPT_ADAGRAD) {   // torch.optim.Adagrad, lr_decay 0
        a = a + g * g;
        return p - k.h0 * (g / (sqrtf(a) + k.eps));
    } else if (RULE == PRX_OPT_ADAMAX) {    // torch.optim.Adamax
        a = a + k.omb1 * (g - a);
        b = fmaxf(k.b2 * b, fabsf(g) + k.eps);
        return p - k.h0 * (a / b);
    } else {                                // DiffGrad: Adam's moments, the step damped where the gradient did not change
        a = k.b1 * a + k.omb1 * g;
        b = k.b2 * b + k.omb2 * g * g;
        const float dfc = 1.f / (1.f + expf(-fabsf(c - g)));
        c = g;
        return p - k.h0 * ((a * dfc) / (sqrtf(b) + k.eps));     // eps before the bias correction (folded into h0)
    }
}
template <int RULE> struct RuleStates { static constexpr int n = RULE == PRX_OPT_ADAGRAD ? 1 : RULE == PRX_OPT_DIFFGRAD ? 3 : 2; };

// V = 4: 16-byte accesses over the first n / 4 * 4 elements (pointers 16-byte aligned; with bounds hw % 4 == 0, so the four share a
// channel) and a scalar tail; V = 1 otherwise.
template <int RULE, int V>
__global__ __launch_bounds__(256) void optim_clamp_kernel(float* __restrict__ p, float* __restrict__ s1, float* __restrict__ s2,
                                                          float* __restrict__ s3, const float* __restrict__ g,
                                                          const float* __restrict__ zmin, const float* __restrict__ zmax, int C,
                                                          int hw, size_t n, const float* __restrict__ hyper, float b1, float omb1,
                                                          float b2, float omb2, float eps) {
    constexpr int NS = RuleStates<RULE>::n;
    const RuleArgs k = {hyper[0], hyper[1], hyper[2], b1, omb1, b2, omb2, eps};
    const size_t nu = n / V, stride = (size_t)gridDim.x * blockDim.x;
    size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    ChanIter ci;
    if (zmin) ci.init(u * V, stride * V, hw, C);
    for (; u < nu; u += stride) {
        float lo = 0.f, hi = 0.f;
        if (zmin) { lo = zmin[ci.ch]; hi = zmax[ci.ch]; ci.next(); }
        if (V == 4) {
            float4 pv = reinterpret_cast<float4*>(p)[u];
            const float4 gv = reinterpret_cast<const float4*>(g)[u];
            float4 av = reinterpret_cast<float4*>(s1)[u], bv = av, cv = av;
            if (NS > 1) bv = reinterpret_cast<float4*>(s2)[u];
            if (NS > 2) cv = reinterpret_cast<float4*>(s3)[u];
            pv.x = rule_step<RULE>(pv.x, av.x, bv.x, cv.x, gv.x, k);
            pv.y = rule_step<RULE>(pv.y, av.y, bv.y, cv.y, gv.y, k);
            pv.z = rule_step<RULE>(pv.z, av.z, bv.z, cv.z, gv.z, k);
            pv.w = rule_step<RULE>(pv.w, av.w, bv.w, cv.w, gv.w, k);
            if (zmin) {
                pv.x = fminf(fmaxf(pv.x, lo), hi); pv.y = fminf(fmaxf(pv.y, lo), hi);
                pv.z = fminf(fmaxf(pv.z, lo), hi); pv.w = fminf(fmaxf(pv.w, lo), hi);
            }
            reinterpret_cast<float4*>(p)[u] = pv;
            reinterpret_cast<float4*>(s1)[u] = av;
            if (NS > 1) reinterpret_cast<float4*>(s2)[u] = bv;
            if (NS > 2) reinterpret_cast<float4*>(s3)[u] = cv;
        } else {
            float a = s1[u], b = NS > 1 ? s2[u] : 0.f, c = NS > 2 ? s3[u] : 0.f;
            float pi = rule_step<RULE>(p[u], a, b, c, g[u], k);
            if (zmin) pi = fminf(fmaxf(pi, lo), hi);
            p[u] = pi; s1[u] = a;
            if (NS > 1) s2[u] = b;
            if (NS > 2) s3[u] = c;
        }
    }
    if (V > 1) {                                       // the n % 4 elements after the last whole vector
        const size_t i = nu * V + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (i < n) {
            float a = s1[i], b = NS > 1 ? s2[i] : 0.f, c = NS > 2 ? s3[i] : 0.f;
            float pi = rule_step<RULE>(p[i], a, b, c, g[i], k);
            if (zmin) { const int ch = (int)((i / hw) % C); pi = fminf(fmaxf(pi, zmin[ch]), zmax[ch]); }
            p[i] = pi; s1[i] = a;
            if (NS > 1) s2[i] = b;
            if (NS > 2) s3[i] = c;
        }
    }
}

inline bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

template <int RULE>
int launch_rule(float* p, float* s1, float* s2, float* s3, const float* g, const float* zmin, const float* zmax, int C, int hw,
                size_t n, const float* hyper, double b1, double b2, float eps, hipStream_t s) {
    constexpr int NS = RuleStates<RULE>::n;
    PRX_REQUIRE(s1 && (NS < 2 || s2) && (NS < 3 || s3), "optim: rule %d needs %d state tensors", RULE, NS);
    const bool vec = n >= 4 && aligned16(p) && aligned16(g) && aligned16(s1) && aligned16(s2) && aligned16(s3) && (!zmin || hw % 4 == 0);
    const float fb1 = (float)b1, fo1 = (float)(1.0 - b1), fb2 = (float)b2, fo2 = (float)(1.0 - b2);
    const int grid = (int)std::min<size_t>((n / (vec ? 4 : 1) + 255) / 256, 8192);
    if (vec) hipLaunchKernelGGL((optim_clamp_kernel<RULE, 4>), dim3(grid), dim3(256), 0, s, p, s1, s2, s3, g, zmin, zmax, C, hw, n, hyper,
                                fb1, fo1, fb2, fo2, eps);
    else hipLaunchKernelGGL((optim_clamp_kernel<RULE, 1>), dim3(grid), dim3(256), 0, s, p, s1, s2, s3, g, zmin, zmax, C, hw, n, hyper, fb1,
                            fo1, fb2, fo2, eps);
    PRX_LAUNCH_CHECK();
    return 0;
}

// ---- AdamP ------------------------------------------------------------------------------------------------------------------
// Workgroup (r, b) owns elements [b * chunk, min((b + 1) * chunk, L)) of row r in both passes.  Pass 1 leaves four partial sums
// per workgroup; pass 2 has EVERY workgroup add all of them in the same order, so all take the same decision and subtract the
// same projection: no atomics, the same bits on every run and every rank.
struct AdampGeom { int rows, nb; size_t L, chunk; };

inline AdampGeom adamp_geom(int rows, size_t n) {
    AdampGeom q;
    q.rows = std::max(rows, 1);
    q.L = n / q.rows;
    const size_t want = std::min<size_t>(std::max<size_t>((q.L + 4095) / 4096, 1), std::max(1, 256 / q.rows));
    q.chunk = std::max<size_t>(((q.L + want - 1) / want + 3) / 4 * 4, 4);
    q.nb = (int)std::max<size_t>((q.L + q.chunk - 1) / q.chunk, 1);
    return q;
}

// sums of `v[0..NV)` over the workgroup's 256 work-items, in a fixed order, returned to every work-item
template <int NV>
__device__ __forceinline__ void block_sum(float (&v)[NV], float (*lds)[NV]) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = wave_sum(v[i]);
    __syncthreads();                                  // the previous use of `lds` has been read
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int i = 0; i < NV; ++i) lds[threadIdx.x >> 6][i] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = ((lds[0][i] + lds[1][i]) + lds[2][i]) + lds[3][i];
}

template <int V>
__global__ __launch_bounds__(256) void adamp_moments_kernel(const float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                            const float* __restrict__ g, AdampGeom q, const float* __restrict__ hyper,
                                                            float* __restrict__ part, float b1, float omb1, float b2, float omb2,
                                                            float eps) {
    __shared__ float lds[4][4];
    const float bc2s = hyper[1];
    const int r = blockIdx.x / q.nb, b = blockIdx.x - r * q.nb;
    const size_t base = (size_t)r * q.L, end = (size_t)(b + 1) * q.chunk < q.L ? (size_t)(b + 1) * q.chunk : q.L;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};              // g.p, g.g, p.p, p.perturb
    auto one = [&](float pi, float& mi, float& vi, float gi) {
        mi = b1 * mi + omb1 * gi;
        vi = b2 * vi + omb2 * gi * gi;
        const float pert = mi / (sqrtf(vi) / bc2s + eps);
        acc[0] += gi * pi; acc[1] += gi * gi; acc[2] += pi * pi; acc[3] += pi * pert;
    };
    for (size_t j = (size_t)b * q.chunk + (size_t)threadIdx.x * V; j < end; j += 256 * V) {
        if (V == 4) {
            const float4 pv = *reinterpret_cast<const float4*>(p + base + j), gv = *reinterpret_cast<const float4*>(g + base + j);
            float4 mv = *reinterpret_cast<float4*>(m + base + j), vv = *reinterpret_cast<float4*>(v + base + j);
            one(pv.x, mv.x, vv.x, gv.x); one(pv.y, mv.y, vv.y, gv.y); one(pv.z, mv.z, vv.z, gv.z); one(pv.w, mv.w, vv.w, gv.w);
            *reinterpret_cast<float4*>(m + base + j) = mv;
            *reinterpret_cast<float4*>(v + base + j) = vv;
        } else {
            float mi = m[base + j], vi = v[base + j];
            one(p[base + j], mi, vi, g[base + j]);
            m[base + j] = mi; v[base + j] = vi;
        }
    }
    block_sum<4>(acc, lds);
    if (threadIdx.x < 4) part[(size_t)blockIdx.x * 4 + threadIdx.x] = acc[threadIdx.x];
}

template <int V>
__global__ __launch_bounds__(256) void adamp_apply_kernel(float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v,
                                                          const float* __restrict__ zmin, const float* __restrict__ zmax, AdampGeom q,
                                                          int project, int C, int hw, const float* __restrict__ hyper,
                                                          const float* __restrict__ part, float eps, float delta) {
    __shared__ float lds[4][4];
    __shared__ float own[2], cm[4];
    const float step = hyper[0], bc2s = hyper[1];
    const int r = blockIdx.x / q.nb, b = blockIdx.x - r * q.nb;
    float coef = 0.f;                                  // perturb -= p * coef: the projection onto the complement of p's row
    if (project) {
        // every workgroup: row totals (partials added b = 0, 1, ...), the rows' largest |cos(g, p)|, and the whole-tensor totals
        float t[4] = {0.f, 0.f, 0.f, 0.f};             // g.p, g.g, p.p, p.perturb over all rows
        float cmax = 0.f;
        for (int rr = threadIdx.x; rr < q.rows; rr += 256) {
            float gp = 0.f, gg = 0.f, pp = 0.f, pq = 0.f;
            for (int bb = 0; bb < q.nb; ++bb) {
                const float4 w = *reinterpret_cast<const float4*>(part + ((size_t)rr * q.nb + bb) * 4);
                gp += w.x; gg += w.y; pp += w.z; pq += w.w;
            }
            cmax = fmaxf(cmax, fabsf(gp) / (sqrtf(gg) * sqrtf(pp) + eps));
            t[0] += gp; t[1] += gg; t[2] += pp; t[3] += pq;
            if (rr == r) { own[0] = pp; own[1] = pq; }
        }
        cmax = wave_max(cmax);
        if ((threadIdx.x & 63) == 0) cm[threadIdx.x >> 6] = cmax;
        block_sum<4>(t, lds);                          // its barriers also publish `own` and `cm`
        cmax = fmaxf(fmaxf(cm[0], cm[1]), fmaxf(cm[2], cm[3]));
        float pp = 0.f, pq = 0.f;
        bool hit = false;
        if (cmax < delta / sqrtf((float)q.L)) {        // channel view [rows, L]
            hit = true; pp = own[0]; pq = own[1];
        } else if (fabsf(t[0]) / (sqrtf(t[1]) * sqrtf(t[2]) + eps) < delta / sqrtf((float)q.L * (float)q.rows)) {   // layer view [1, n]
            hit = true; pp = t[2]; pq = t[3];
        }
        if (hit) {
            const float inv = 1.f / (sqrtf(pp) + eps);
            coef = pq * inv * inv;                     // p_n * sum(p_n * perturb), p_n = p / (|p_row| + eps)
        }
    }
    const size_t base = (size_t)r * q.L, end = (size_t)(b + 1) * q.chunk < q.L ? (size_t)(b + 1) * q.chunk : q.L;
    size_t j = (size_t)b * q.chunk + (size_t)threadIdx.x * V;
    ChanIter ci;
    if (zmin) ci.init(base + j, (size_t)256 * V, hw, C);
    auto one = [&](float pi, float mi, float vi, float lo, float hi) {
        float pert = mi / (sqrtf(vi) / bc2s + eps);
        pert -= pi * coef;
        pi -= step * pert;
        return zmin ? fminf(fmaxf(pi, lo), hi) : pi;
    };
    for (; j < end; j += 256 * V) {
        float lo = 0.f, hi = 0.f;
        if (zmin) { lo = zmin[ci.ch]; hi = zmax[ci.ch]; ci.next(); }
        if (V == 4) {
            float4 pv = *reinterpret_cast<float4*>(p + base + j);
            const float4 mv = *reinterpret_cast<const float4*>(m + base + j), vv = *reinterpret_cast<const float4*>(v + base + j);
            pv.x = one(pv.x, mv.x, vv.x, lo, hi); pv.y = one(pv.y, mv.y, vv.y, lo, hi);
            pv.z = one(pv.z, mv.z, vv.z, lo, hi); pv.w = one(pv.w, mv.w, vv.w, lo, hi);
            *reinterpret_cast<float4*>(p + base + j) = pv;
        } else {
            p[base + j] = one(p[base + j], m[base + j], v[base + j], lo, hi);
        }
    }
}

}  // namespace

int prx_optim_elementwise(int rule, float* p, float* s1, float* s2, float* s3, const float* g, const float* zmin,
                          const float* zmax, int C, int hw, size_t n, const float* hyper, double b1, double b2, float eps,
                          hipStream_t s) {
    PRX_REQUIRE(p && g && hyper && n > 0, "optim: null argument or empty tensor");
    PRX_REQUIRE((zmin == nullptr) == (zmax == nullptr), "optim: zmin and zmax come together");
    PRX_REQUIRE(!zmin || (C >= 1 && hw >= 1 && hw < (1 << 30) && n % ((size_t)C * hw) == 0), "optim: n is not rows * C * hw (C %d, hw %d)", C, hw);
    switch (rule) {
        case PRX_OPT_ADAMW: return launch_rule<PRX_OPT_ADAMW>(p, s1, s2, s3, g, zmin, zmax, C, hw, n, hyper, b1, b2, eps, s);
        case PRX_OPT_ADAGRAD: return launch_rule<PRX_OPT_ADAGRAD>(p, s1, s2, s3, g, zmin, zmax, C, hw, n, hyper, b1, b2, eps, s);
        case PRX_OPT_ADAMAX: return launch_rule<PRX_OPT_ADAMAX>(p, s1, s2, s3, g, zmin, zmax, C, hw, n, hyper, b1, b2, eps, s);
        case PRX_OPT_DIFFGRAD: return launch_rule<PRX_OPT_DIFFGRAD>(p, s1, s2, s3, g, zmin, zmax, C, hw, n, hyper, b1, b2, eps, s);
    }
    PRX_REQUIRE(false, "optim: unknown rule %d", rule);
    return 0;
}

size_t prx_adamp_scratch_floats(int rows, size_t n) {
    if (n == 0) return 4;
    const AdampGeom q = adamp_geom(rows, n);
    return (size_t)q.rows * q.nb * 4;
}

int prx_optim_adamp(float* p, float* m, float* v, const float* g, const float* zmin, const float* zmax, int rows, int C, int hw,
                    size_t n, const float* hyper, float* scratch, size_t scratch_floats, double b1, double b2, float eps,
                    float delta, hipStream_t s) {
    PRX_REQUIRE(p && m && v && g && hyper && scratch && n > 0, "adamp: null argument or empty tensor");
    PRX_REQUIRE((zmin == nullptr) == (zmax == nullptr), "adamp: zmin and zmax come together");
    PRX_REQUIRE(!zmin || (C >= 1 && hw >= 1 && hw < (1 << 30) && n % ((size_t)C * hw) == 0), "adamp: n is not rows * C * hw (C %d, hw %d)", C, hw);
    PRX_REQUIRE(rows >= 0 && rows <= 4096 && n % std::max(rows, 1) == 0, "adamp: rows %d (at most 4096, and a divisor of n)", rows);
    const AdampGeom q = adamp_geom(rows, n);
    PRX_REQUIRE((size_t)q.rows * q.nb * 4 <= scratch_floats && aligned16(scratch), "adamp: scratch too small or not 16-byte aligned");
    const bool vec = q.L % 4 == 0 && aligned16(p) && aligned16(m) && aligned16(v) && aligned16(g) && (!zmin || hw % 4 == 0);
    const float fb1 = (float)b1, fo1 = (float)(1.0 - b1), fb2 = (float)b2, fo2 = (float)(1.0 - b2);
    const dim3 grid(q.rows * q.nb);
    if (vec) hipLaunchKernelGGL(adamp_moments_kernel<4>, grid, dim3(256), 0, s, p, m, v, g, q, hyper, scratch, fb1, fo1, fb2, fo2, eps);
    else hipLaunchKernelGGL(adamp_moments_kernel<1>, grid, dim3(256), 0, s, p, m, v, g, q, hyper, scratch, fb1, fo1, fb2, fo2, eps);
    PRX_LAUNCH_CHECK();
    if (vec) hipLaunchKernelGGL(adamp_apply_kernel<4>, grid, dim3(256), 0, s, p, m, v, zmin, zmax, q, rows > 0 ? 1 : 0, C, hw, hyper, scratch, eps, delta);
    else hipLaunchKernelGGL(adamp_apply_kernel<1>, grid, dim3(256), 0, s, p, m, v, zmin, zmax, q, rows > 0 ? 1 : 0, C, hw, hyper, scratch, eps, delta);
    PRX_LAUNCH_CHECK();
    return 0;
}
