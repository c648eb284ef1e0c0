// The 16-bit attention kernels of attention.hip, templated on the operand format F:
//   F::T     element type (bf16_t | half_t), F::V8 / F::V4 its 8- / 4-vectors
//   F::mfma  c += a b on the matching v_mfma_f32_32x32x16_* builtin
// Conversions are the element type's own (round-to-nearest-even); everything else is format-agnostic.
// (mfma accumulates into a reference: a wrapper that RETURNS the product marks the value noundef, the optimiser then drops the
// freeze it puts on two products of mha_bwd_kernel, and that kernel's schedule moves -- 31 more instructions.)
#pragma once
#include "attention.h"

namespace {

struct FmtBf16 {
    using T = bf16_t; using V8 = bf16x8; using V4 = bf16x4;
    static __device__ __forceinline__ void mfma(V8 a, V8 b, f32x16& c) { c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
struct FmtF16 {
    using T = half_t; using V8 = f16x8; using V4 = f16x4;
    static __device__ __forceinline__ void mfma(V8 a, V8 b, f32x16& c) { c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};
template <typename F> using El = typename F::T;
template <typename F> using V8 = typename F::V8;
template <typename F> using V4 = typename F::V4;

constexpr int LD = 72;             // padded LDS row (elements) of the 64-wide tiles, 144 B
constexpr int TILE = 64 * LD;      // one [64][72] buffer
constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ float half_max(float v) {  // reduce over the 32 lanes of a half-wave
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// acc[mi][nj] += A[(mi*32 + r)][k] * B[(nj*32 + c)][k] over k in [0,64)
template <typename F>
__device__ __forceinline__ void mma_64x64x64(const El<F>* A, const El<F>* B, f32x16 (&acc)[2][2], int lane) {
    const int fr = lane & 31, fk = 8 * (lane >> 5);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        V8<F> a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            a[i] = *reinterpret_cast<const V8<F>*>(&A[(i * 32 + fr) * LD + ks * 16 + fk]);
            b[i] = *reinterpret_cast<const V8<F>*>(&B[(i * 32 + fr) * LD + ks * 16 + fk]);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) F::mfma(a[i], b[j], acc[i][j]);
    }
}

__device__ __forceinline__ void zero16(f32x16& a) {
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = 0.f;
}
template <int NB>
__device__ __forceinline__ void zero_blocks(f32x16 (&o)[NB]) {
#pragma unroll
    for (int i = 0; i < NB; ++i) zero16(o[i]);
}
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[2][2]) {
    zero_blocks(acc[0]); zero_blocks(acc[1]);
}

// (image, head) from the flat workgroup id through the XCD map (common.h): an XCD works on a contiguous range of images,
// the same token rows whose qkv the projection GEMM of that XCD just wrote
__device__ __forceinline__ void block_head(int xcd, int& h, int& n) {
    const unsigned flat = blockIdx.y * gridDim.x + blockIdx.x, nwg = gridDim.x * gridDim.y;
    const unsigned lin = xcd ? xcd_linear(flat, nwg) : flat;
    h = (int)(lin % gridDim.x); n = (int)(lin / gridDim.x);
}

// Column swizzle of the transposed images written by load_tile and read by tr_frag: element (d, t) lives at column
// t ^ tr_swz(d).  Unswizzled, the 64 two-byte writes of one instruction land in 8 banks (rows 8 apart are 1152 B = 0 mod
// 128 apart) and the 8-byte fragment reads of rows d and d+16 collide; with bits 4-5 of d moved into bits 2-4 of the
// column both are conflict-free in a 64-bank model (exhaustive search over the linear swizzles; the unswizzled kernel showed
// SQ_LDS_BANK_CONFLICT = 18 % of its wave cycles, profiles/r01_h_pmc_sq_stalls.csv).  Worth 0.02 ms per iteration.
// Only bits >= 2 of t change, so the 4-element groups the reader fetches stay contiguous.
__device__ __forceinline__ int tr_swz(int d) { return (((d >> 4) & 1) * 12) ^ (((d >> 5) & 1) * 16); }

// 128 threads load a [T][64] tile (row stride ld) into dst[t][d] and optionally dstT[d][t ^ tr_swz(d)]; rows >= T are zero.
// In two halves -- tile_get requests a thread's four 16-byte pieces, tile_put writes them to LDS -- so that a kernel can request ALL
// its tiles before the first LDS write: written as one load -> write loop per tile (round 1 - 5), every piece was followed by
// s_waitcnt vmcnt(0) and its write, i.e. 12 (forward) / 24 (backward) dependent global round trips in front of the first MFMA of a
// kernel that computes for ~3 us.  The backward also keeps the Q and dO pieces in registers and writes their transposed images from
// there instead of fetching both tiles a second time.
template <typename F>
__device__ __forceinline__ void tile_get(const El<F>* src, long long ld, int T, int tid, V8<F> (&v)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = tid + 128 * i;
        const int row = c >> 3, kc = c & 7;
        // clamped address + select, not a branch around the load: a join point makes the compiler wait for everything in flight
        const V8<F> z = {0, 0, 0, 0, 0, 0, 0, 0};
        const V8<F> x = *reinterpret_cast<const V8<F>*>(src + (long long)(row < T ? row : T - 1) * ld + kc * 8);
        v[i] = row < T ? x : z;
    }
}
template <typename F>
__device__ __forceinline__ void tile_put(const V8<F> (&v)[4], El<F>* dst, El<F>* dstT, int tid) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = tid + 128 * i;
        const int row = c >> 3, kc = c & 7;
        if (dst) *reinterpret_cast<V8<F>*>(&dst[row * LD + kc * 8]) = v[i];
        if (dstT) {
#pragma unroll
            for (int e = 0; e < 8; ++e) dstT[(kc * 8 + e) * LD + (row ^ tr_swz(kc * 8))] = v[i][e];
        }
    }
}

// acc[mi] += A[(mi*32 + r)][k] * B[(nb*32 + c)][k] over k in [0,64): the 64 x 32 column block `nb` of A B^T
template <typename F>
__device__ __forceinline__ void mma_64x32x64(const El<F>* A, const El<F>* B, int nb, f32x16 (&acc)[2], int lane) {
    const int fr = lane & 31, fk = 8 * (lane >> 5);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const V8<F> b = *reinterpret_cast<const V8<F>*>(&B[(nb * 32 + fr) * LD + ks * 16 + fk]);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const V8<F> a = *reinterpret_cast<const V8<F>*>(&A[(i * 32 + fr) * LD + ks * 16 + fk]);
            F::mfma(a, b, acc[i]);
        }
    }
}
// write the C-layout rows 32*rb .. 32*rb+31 of a [t][32 NDJ] result (a[dj] = columns 32dj ..) to global rows < T
template <typename F, int NDJ>
__device__ __forceinline__ void store_rows_global(const f32x16 (&a)[NDJ], int rb, El<F>* out, long long ld, int T, int lane) {
    const int col = lane & 31, r0 = 32 * rb + 4 * (lane >> 5);
#pragma unroll
    for (int dj = 0; dj < NDJ; ++dj)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = r0 + (r & 3) + 8 * (r >> 2);
            if (i < T) out[(long long)i * ld + dj * 32 + col] = (El<F>)a[dj][r];
        }
}

// write a C-layout 64x64 tile to LDS as dst[i][j] and/or dstT[j][i]
template <typename F>
__device__ __forceinline__ void store_c_tile(const f32x16 (&a)[2][2], El<F>* dst, El<F>* dstT, int lane) {
    const int col = lane & 31, rb = 4 * (lane >> 5);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int nj = 0; nj < 2; ++nj)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = mi * 32 + (r & 3) + 8 * (r >> 2) + rb;
                const int j = nj * 32 + col;
                El<F> v = (El<F>)a[mi][nj][r];
                if (dst) dst[i * LD + j] = v;
                if (dstT) dstT[j * LD + i] = v;
            }
}

// write a C-layout [t][d] tile to global rows < T
template <typename F>
__device__ __forceinline__ void store_c_global(const f32x16 (&a)[2][2], El<F>* out, long long ld, int T, int lane) {
    const int col = lane & 31, rb = 4 * (lane >> 5);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int nj = 0; nj < 2; ++nj)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = mi * 32 + (r & 3) + 8 * (r >> 2) + rb;
                if (i < T) out[(long long)i * ld + nj * 32 + col] = (El<F>)a[mi][nj][r];
            }
}

// Forward, "swapped" formulation: S^T = K Q^T puts one QUERY per lane column (C layout: lane l holds query l&31 of its
// block, 16 of its keys in registers, the other 16 in lane l^32), so the softmax is an in-register reduction plus ONE
// cross-half exchange per statistic instead of a 5-step butterfly per row; and the normalised P^T accumulators are
// already the A operand of O = P V (rows = queries = this lane, k slots = the keys it holds) -- P never goes through
// LDS.  The MFMA only needs A and B to agree on which key sits in which k slot: slot 8h+s of step (mi, G) is key
// 32mi + 16G + 8(s>>2) + 4h + (s&3), which for the B operand (rows = head-dim d of V^T) is two 8-byte reads of the
// transposed V image.
// Two waves per (image, head): wave w owns queries 32w .. 32w+31 (its column block of S^T, its rows of O).  768
// one-wave workgroups left every CU with 3 waves in flight and each of them latency-bound; the split halves the MFMA
// chain per wave and doubles the waves a CU can interleave.
template <typename F>
__device__ __forceinline__ V8<F> acc_frag(const f32x16& a, int G) {        // accumulator registers 8G .. 8G+7 as an A fragment
    V8<F> f;
#pragma unroll
    for (int s = 0; s < 8; ++s) f[s] = (El<F>)a[8 * G + s];
    return f;
}
template <typename F>
__device__ __forceinline__ V8<F> tr_frag(const El<F>* Tt, int dj, int mi, int G, int lane) {
    const int d = dj * 32 + (lane & 31), t0 = 32 * mi + 16 * G + 4 * (lane >> 5), sw = tr_swz(d);
    const V4<F> lo = *reinterpret_cast<const V4<F>*>(Tt + d * LD + (t0 ^ sw));
    const V4<F> hi = *reinterpret_cast<const V4<F>*>(Tt + d * LD + ((t0 + 8) ^ sw));
    return V8<F>{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
// o[dj] += sum over the contraction axis of A (accumulators a[mi], rows = this lane's column index) x B^T image
template <typename F>
__device__ __forceinline__ void mma_acc_tr(const f32x16 (&a)[2], const El<F>* Tt, f32x16 (&o)[2], int lane) {
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int G = 0; G < 2; ++G) {
            const V8<F> fa = acc_frag<F>(a[mi], G);
#pragma unroll
            for (int dj = 0; dj < 2; ++dj) F::mfma(fa, tr_frag<F>(Tt, dj, mi, G, lane), o[dj]);
        }
}

template <typename F>
__global__ __launch_bounds__(128) void mha_fwd_kernel(const El<F>* __restrict__ qkv, El<F>* __restrict__ out, int T, int C, float scale,
                                                      int xcd) {
    using E = El<F>;
    __shared__ __attribute__((aligned(16))) E smem[3 * TILE];
    E* Qs = smem;
    E* Ks = smem + TILE;
    E* Vt = smem + 2 * TILE;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int h, n;
    block_head(xcd, h, n);
    const long long ld = 3LL * C;
    const E* base = qkv + (long long)n * T * ld + h * 64;
    {
        V8<F> tq[4], tk[4], tv[4];
        tile_get<F>(base, ld, T, tid, tq);
        tile_get<F>(base + C, ld, T, tid, tk);
        tile_get<F>(base + 2 * C, ld, T, tid, tv);
        tile_put<F>(tq, Qs, nullptr, tid);
        tile_put<F>(tk, Ks, nullptr, tid);
        tile_put<F>(tv, nullptr, Vt, tid);
    }
    __syncthreads();
    f32x16 st[2];                          // st[mi]: keys 32mi.., queries 32w..
    zero_blocks(st);
    mma_64x32x64<F>(Ks, Qs, w, st, lane);
    const int hh = lane >> 5;
    {
        float m = -INFINITY;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                const float v = (j < T) ? st[mi][r] * scale : -INFINITY;
                st[mi][r] = v;
                m = fmaxf(m, v);
            }
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        float sum = 0.f;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float e = __expf(st[mi][r] - m);
                st[mi][r] = e;
                sum += e;
            }
        sum += __shfl_xor(sum, 32, 64);
        const float inv = 1.f / sum;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) st[mi][r] *= inv;
    }
    f32x16 o[2];                           // o[dj]: queries 32w.., head-dim 32dj..
    zero_blocks(o);
    mma_acc_tr<F>(st, Vt, o, lane);
    store_rows_global<F>(o, w, out + (long long)n * T * C + h * 64, C, T, lane);
}

// Backward, same register-resident scheme as the forward, in two orientations:
//   (1) queries on lanes:  P^T = softmax(K Q^T), dP^T = V dO^T, D_i = sum_j P dP, dS^T  ->  dQ = dS K   (A = dS^T accumulators)
//   (2) keys on lanes:     P = exp(Q K^T / 8 - lse_i), dP = dO V^T, dS               ->  dK = dS^T Q, dV = P^T dO
// Orientation 2 recomputes the two score products instead of transposing dS / P through LDS; it gets the per-query
// log-sum-exp and D_i from orientation 1 through two 64-float LDS arrays.  The B operands K^T, Q^T, dO^T are transposed
// LDS images built one after the other in the fifth tile.  Two waves per (image, head), as in the forward: wave w owns
// queries 32w.. in orientation 1 (its rows of dQ) and keys 32w.. in orientation 2 (its rows of dK and dV).
template <typename F>
__global__ __launch_bounds__(128) void mha_bwd_kernel(const El<F>* __restrict__ qkv, const El<F>* __restrict__ dout, El<F>* __restrict__ dqkv,
                                                      int T, int C, float scale, int xcd) {
    using E = El<F>;
    __shared__ __attribute__((aligned(16))) E smem[5 * TILE];
    __shared__ __attribute__((aligned(16))) float s_lse[64], s_D[64];
    E* Qs = smem;
    E* Ks = smem + TILE;
    E* Vs = smem + 2 * TILE;
    E* dOs = smem + 3 * TILE;
    E* Tt = smem + 4 * TILE;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int h, n;
    block_head(xcd, h, n);
    const int hh = lane >> 5;
    const long long ld = 3LL * C;
    const E* base = qkv + (long long)n * T * ld + h * 64;
    const E* dobase = dout + (long long)n * T * C + h * 64;
    V8<F> tq[4], tdo[4];                                 // kept: their transposed images are written from here later
    {
        V8<F> tk[4], tv[4];
        tile_get<F>(base, ld, T, tid, tq);
        tile_get<F>(base + C, ld, T, tid, tk);
        tile_get<F>(base + 2 * C, ld, T, tid, tv);
        tile_get<F>(dobase, C, T, tid, tdo);
        tile_put<F>(tq, Qs, nullptr, tid);
        tile_put<F>(tk, Ks, Tt, tid);                    // K row-major and K^T
        tile_put<F>(tv, Vs, nullptr, tid);
        tile_put<F>(tdo, dOs, nullptr, tid);
    }
    __syncthreads();
    E* obase = dqkv + (long long)n * T * ld + h * 64;
    {   // ---- orientation 1: [key j][query i], lane column = query 32w + (lane & 31)
        f32x16 pt[2], dpt[2];
        zero_blocks(pt);
        mma_64x32x64<F>(Ks, Qs, w, pt, lane);
        zero_blocks(dpt);
        mma_64x32x64<F>(Vs, dOs, w, dpt, lane);
        float m = -INFINITY;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                const float v = (j < T) ? pt[mi][r] * scale : -INFINITY;
                pt[mi][r] = v;
                m = fmaxf(m, v);
            }
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        float sum = 0.f;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float e = __expf(pt[mi][r] - m);
                pt[mi][r] = e;
                sum += e;
            }
        sum += __shfl_xor(sum, 32, 64);
        const float inv = 1.f / sum;
        float dot = 0.f;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                pt[mi][r] *= inv;
                dot += pt[mi][r] * dpt[mi][r];
            }
        dot += __shfl_xor(dot, 32, 64);
        if (hh == 0) { s_lse[w * 32 + lane] = m + __logf(sum); s_D[w * 32 + lane] = dot; }
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) dpt[mi][r] = scale * pt[mi][r] * (dpt[mi][r] - dot);   // dS^T
        f32x16 acc[2];
        zero_blocks(acc);
        mma_acc_tr<F>(dpt, Tt, acc, lane);               // dQ[i][d] = sum_j dS[i][j] K[j][d]
        store_rows_global<F>(acc, w, obase, ld, T, lane);
    }
    __syncthreads();                                      // s_lse / s_D visible, K^T image free
    tile_put<F>(tq, nullptr, Tt, tid);                    // Q^T
    // ---- orientation 2: [query i][key j], lane column = key 32w + (lane & 31)
    f32x16 p[2], dp[2];
    zero_blocks(p);
    mma_64x32x64<F>(Qs, Ks, w, p, lane);
    zero_blocks(dp);
    mma_64x32x64<F>(dOs, Vs, w, dp, lane);
    const bool key_ok = w * 32 + (lane & 31) < T;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
            const int i0 = mi * 32 + 8 * rg + 4 * hh;
            const float4 l4 = *reinterpret_cast<const float4*>(&s_lse[i0]);
            const float4 d4 = *reinterpret_cast<const float4*>(&s_D[i0]);
            const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = rg * 4 + q;
                const float pv = key_ok ? __expf(p[mi][r] * scale - lv[q]) : 0.f;
                p[mi][r] = pv;
                dp[mi][r] = scale * pv * (dp[mi][r] - dv[q]);   // dS
            }
        }
    __syncthreads();                                      // Q^T image complete
    {
        f32x16 acc[2];
        zero_blocks(acc);
        mma_acc_tr<F>(dp, Tt, acc, lane);                 // dK[j][d] = sum_i dS[i][j] Q[i][d]
        store_rows_global<F>(acc, w, obase + C, ld, T, lane);
    }
    __syncthreads();
    tile_put<F>(tdo, nullptr, Tt, tid);                    // dO^T
    __syncthreads();
    {
        f32x16 acc[2];
        zero_blocks(acc);
        mma_acc_tr<F>(p, Tt, acc, lane);                  // dV[j][d] = sum_i P[i][j] dO[i][d]
        store_rows_global<F>(acc, w, obase + 2 * C, ld, T, lane);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// General sequence length (T > 64: ViT-B/16 has 197 tokens, ViT-L/14 257), head dim 64: flash-style tiling over
// 64-token tiles with an online softmax.  One wave per (64-query tile, head, image).
//   forward : O = softmax(QK^T/8) V, also writes LSE_i = m_i + log(l_i) (fp32) for the backward
//   backward: dQ kernel (one wave per query tile, loops over key tiles) and dK/dV kernel (one wave per key tile,
//             loops over query tiles); both recompute P from LSE.  D_i = sum_d dO_id * O_id is recomputed per tile.
// ---------------------------------------------------------------------------------------------------------------
template <typename F>
__device__ __forceinline__ void load_rows(const El<F>* src, long long ld, int t0, int T, El<F>* dst, El<F>* dstT, int lane) {
    // rows t0 .. t0+63 of a [T][64] matrix (zero beyond T)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = lane + 64 * i;
        const int row = c >> 3, kc = c & 7;
        V8<F> v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (t0 + row < T) v = *reinterpret_cast<const V8<F>*>(src + (long long)(t0 + row) * ld + kc * 8);
        if (dst) *reinterpret_cast<V8<F>*>(&dst[row * LD + kc * 8]) = v;
        if (dstT) {
#pragma unroll
            for (int e = 0; e < 8; ++e) dstT[(kc * 8 + e) * LD + row] = v[e];
        }
    }
}

// CAUSAL: CLIP's text transformer mask (key j visible to query i iff j <= i); K tiles entirely in the future are skipped
template <typename F, bool CAUSAL>
__global__ __launch_bounds__(64) void mha_fwd_gen_kernel(const El<F>* __restrict__ qkv, El<F>* __restrict__ out, float* __restrict__ lse, int T,
                                                         int C, int heads, float scale) {
    using E = El<F>;
    __shared__ __attribute__((aligned(16))) E smem[4 * TILE];
    E* Qs = smem; E* Ks = smem + TILE; E* Vt = smem + 2 * TILE; E* Ps = smem + 3 * TILE;
    const int lane = threadIdx.x;
    const int qt = blockIdx.x, h = blockIdx.y, n = blockIdx.z;
    const long long ld = 3LL * C;
    const E* base = qkv + (long long)n * T * ld + h * 64;
    const int q0 = qt * 64;
    load_rows<F>(base, ld, q0, T, Qs, nullptr, lane);
    f32x16 o[2][2];
    zero_acc(o);
    float m_run[2][16], l_run[2][16];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) { m_run[mi][r] = -INFINITY; l_run[mi][r] = 0.f; }
    const int j0l = lane & 31;
    const int k_end = CAUSAL ? min(T, q0 + 64) : T;
    for (int k0 = 0; k0 < k_end; k0 += 64) {
        __syncthreads();
        load_rows<F>(base + C, ld, k0, T, Ks, nullptr, lane);
        load_rows<F>(base + 2 * C, ld, k0, T, nullptr, Vt, lane);
        __syncthreads();
        f32x16 s[2][2];
        zero_acc(s);
        mma_64x64x64<F>(Qs, Ks, s, lane);
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qi = q0 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);     // this accumulator's query row
                const int lim = CAUSAL ? min(T, qi + 1) : T;
                const float v0 = (k0 + j0l < lim) ? s[mi][0][r] * scale : -INFINITY;
                const float v1 = (k0 + j0l + 32 < lim) ? s[mi][1][r] * scale : -INFINITY;
                const float mx = fmaxf(m_run[mi][r], half_max(fmaxf(v0, v1)));
                const float alpha = __expf(m_run[mi][r] - mx);          // 0 on the first tile (m = -inf)
                const float e0 = __expf(v0 - mx), e1 = __expf(v1 - mx);
                l_run[mi][r] = l_run[mi][r] * alpha + half_sum(e0 + e1);
                m_run[mi][r] = mx;
                s[mi][0][r] = e0; s[mi][1][r] = e1;
                o[mi][0][r] *= alpha; o[mi][1][r] *= alpha;
            }
        store_c_tile<F>(s, Ps, nullptr, lane);
        __syncthreads();
        mma_64x64x64<F>(Ps, Vt, o, lane);
    }
    const int col = lane & 31, rb = 4 * (lane >> 5);
    E* obase = out + (long long)n * T * C + h * 64;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = q0 + mi * 32 + (r & 3) + 8 * (r >> 2) + rb;
            if (i < T) {
                const float inv = 1.f / l_run[mi][r];
                obase[(long long)i * C + col] = (E)(o[mi][0][r] * inv);
                obase[(long long)i * C + 32 + col] = (E)(o[mi][1][r] * inv);
                if (col == 0 && lse) lse[((long long)n * heads + h) * T + i] = m_run[mi][r] + __logf(l_run[mi][r]);
            }
        }
}

// P (C layout, rows = this wave's queries) from LSE, and dS = scale * P o (dP - D)
__device__ __forceinline__ void probs_from_lse(f32x16 (&s)[2][2], const float (&lse_r)[2][16], float scale, int k0, int T, int lane) {
    const int j0l = lane & 31;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[mi][0][r] = (k0 + j0l < T) ? __expf(s[mi][0][r] * scale - lse_r[mi][r]) : 0.f;
            s[mi][1][r] = (k0 + j0l + 32 < T) ? __expf(s[mi][1][r] * scale - lse_r[mi][r]) : 0.f;
        }
}

// per-row quantities of the 64 query rows starting at q0 in the C layout: LSE and D = rowsum(dO o O)
template <typename F>
__device__ __forceinline__ void row_stats(const float* lse_h, const El<F>* o_h, const El<F>* do_h, long long ldo, int q0, int T,
                                          float (&lse_r)[2][16], float (&d_r)[2][16], int lane) {
    const int rb = 4 * (lane >> 5);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = q0 + mi * 32 + (r & 3) + 8 * (r >> 2) + rb;
            float dsum = 0.f, l = 0.f;
            if (i < T) {
                l = lse_h[i];
                // 32 lanes of the half-wave share row i: each handles 2 of the 64 columns
                const int c = (lane & 31) * 2;
                dsum = (float)do_h[(long long)i * ldo + c] * (float)o_h[(long long)i * ldo + c] +
                       (float)do_h[(long long)i * ldo + c + 1] * (float)o_h[(long long)i * ldo + c + 1];
            }
            d_r[mi][r] = half_sum(dsum);
            lse_r[mi][r] = (i < T) ? l : INFINITY;     // exp(x - inf) = 0 for padded query rows
        }
}

template <typename F>
__global__ __launch_bounds__(64) void mha_bwd_dq_gen_kernel(const El<F>* __restrict__ qkv, const El<F>* __restrict__ o,
                                                            const El<F>* __restrict__ dout, const float* __restrict__ lse,
                                                            El<F>* __restrict__ dqkv, int T, int C, int heads, float scale) {
    using E = El<F>;
    __shared__ __attribute__((aligned(16))) E smem[5 * TILE];
    E* Qs = smem; E* dOs = smem + TILE; E* Ks = smem + 2 * TILE; E* Vs = smem + 3 * TILE; E* Kt = smem + 4 * TILE;
    const int lane = threadIdx.x;
    const int qt = blockIdx.x, h = blockIdx.y, n = blockIdx.z;
    const long long ld = 3LL * C;
    const E* base = qkv + (long long)n * T * ld + h * 64;
    const E* dob = dout + (long long)n * T * C + h * 64;
    const E* ob = o + (long long)n * T * C + h * 64;
    const int q0 = qt * 64;
    load_rows<F>(base, ld, q0, T, Qs, nullptr, lane);
    load_rows<F>(dob, C, q0, T, dOs, nullptr, lane);
    float lse_r[2][16], d_r[2][16];
    row_stats<F>(lse + ((long long)n * heads + h) * T, ob, dob, C, q0, T, lse_r, d_r, lane);
    f32x16 dq[2][2];
    zero_acc(dq);
    for (int k0 = 0; k0 < T; k0 += 64) {
        __syncthreads();
        load_rows<F>(base + C, ld, k0, T, Ks, Kt, lane);
        load_rows<F>(base + 2 * C, ld, k0, T, Vs, nullptr, lane);
        __syncthreads();
        f32x16 p[2][2], dp[2][2];
        zero_acc(p);
        mma_64x64x64<F>(Qs, Ks, p, lane);
        probs_from_lse(p, lse_r, scale, k0, T, lane);
        zero_acc(dp);
        mma_64x64x64<F>(dOs, Vs, dp, lane);
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                dp[mi][0][r] = scale * p[mi][0][r] * (dp[mi][0][r] - d_r[mi][r]);
                dp[mi][1][r] = scale * p[mi][1][r] * (dp[mi][1][r] - d_r[mi][r]);
            }
        __syncthreads();
        store_c_tile<F>(dp, Ks, nullptr, lane);      // Ks <- dS [i][j]  (K itself is no longer needed, K^T is)
        __syncthreads();
        mma_64x64x64<F>(Ks, Kt, dq, lane);           // dQ += dS K
    }
    store_c_global<F>(dq, dqkv + (long long)n * T * ld + h * 64 + (long long)q0 * ld, ld, T - q0, lane);
}

template <typename F>
__global__ __launch_bounds__(64) void mha_bwd_dkv_gen_kernel(const El<F>* __restrict__ qkv, const El<F>* __restrict__ o,
                                                             const El<F>* __restrict__ dout, const float* __restrict__ lse,
                                                             El<F>* __restrict__ dqkv, int T, int C, int heads, float scale) {
    using E = El<F>;
    __shared__ __attribute__((aligned(16))) E smem[6 * TILE];
    E* Ks = smem; E* Vs = smem + TILE; E* Qs = smem + 2 * TILE; E* dOs = smem + 3 * TILE;
    E* Qt = smem + 4 * TILE; E* dOt = smem + 5 * TILE;
    const int lane = threadIdx.x;
    const int kt = blockIdx.x, h = blockIdx.y, n = blockIdx.z;
    const long long ld = 3LL * C;
    const E* base = qkv + (long long)n * T * ld + h * 64;
    const E* dob = dout + (long long)n * T * C + h * 64;
    const E* ob = o + (long long)n * T * C + h * 64;
    const int k0 = kt * 64;
    load_rows<F>(base + C, ld, k0, T, Ks, nullptr, lane);
    load_rows<F>(base + 2 * C, ld, k0, T, Vs, nullptr, lane);
    f32x16 dk[2][2], dv[2][2];
    zero_acc(dk); zero_acc(dv);
    for (int q0 = 0; q0 < T; q0 += 64) {
        __syncthreads();
        load_rows<F>(base, ld, q0, T, Qs, Qt, lane);
        load_rows<F>(dob, C, q0, T, dOs, dOt, lane);
        __syncthreads();
        float lse_r[2][16], d_r[2][16];
        row_stats<F>(lse + ((long long)n * heads + h) * T, ob, dob, C, q0, T, lse_r, d_r, lane);
        f32x16 p[2][2], dp[2][2];
        zero_acc(p);
        mma_64x64x64<F>(Qs, Ks, p, lane);
        probs_from_lse(p, lse_r, scale, k0, T, lane);
        zero_acc(dp);
        mma_64x64x64<F>(dOs, Vs, dp, lane);
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                dp[mi][0][r] = scale * p[mi][0][r] * (dp[mi][0][r] - d_r[mi][r]);
                dp[mi][1][r] = scale * p[mi][1][r] * (dp[mi][1][r] - d_r[mi][r]);
            }
        __syncthreads();
        store_c_tile<F>(p, nullptr, Qs, lane);       // Qs  <- P^T  [j][i]
        store_c_tile<F>(dp, nullptr, dOs, lane);     // dOs <- dS^T [j][i]
        __syncthreads();
        mma_64x64x64<F>(Qs, dOt, dv, lane);          // dV += P^T dO
        mma_64x64x64<F>(dOs, Qt, dk, lane);          // dK += dS^T Q
    }
    E* ob2 = dqkv + (long long)n * T * ld + h * 64 + (long long)k0 * ld;
    store_c_global<F>(dk, ob2 + C, ld, T - k0, lane);
    store_c_global<F>(dv, ob2 + 2 * C, ld, T - k0, lane);
}


// ---------------------------------------------------------------------------------------------------------------
// The "blk" family, T <= 640 (ViT-B/16: 197, ViT-L/14 and ViT-H/14: 257, ViT-L/14@336px: 577, the ModifiedResNet attention pools:
// 50 ... 197): workgroups per (image, head) with one wave per 32 tokens, the register-resident scheme of the T <= 64 kernels above
// (scores with the owned tokens on the lane columns, so that the probabilities are already the A operand of the second product)
// streamed over 128-token LDS chunks of the other operand.  The tile kernels above (one wave per 64-query tile, every wave
// re-staging and re-transposing K / V for itself, 36-55 KB of LDS per wave) ran ViT-L/14 at 256 cutouts at 1.5 / 1.9 / 6.0 ms per
// layer (forward / dQ / dK+dV: 2-3 waves per CU); they remain for T > 640 and for the causal text tower.
//   forward : online softmax per owned query (running max / sum per lane); the rescale factors reach the O accumulators
//             (queries on register rows) through a 32-float LDS line per wave
//   backward: dQ kernel (owned queries, chunks of K / V / K^T) and dK+dV kernel (owned keys, chunks of Q / dO / Q^T /
//             dO^T with the per-query LSE and D = rowsum(dO o O) staged beside them); both recompute P from the LSE
// Templated on HDP, the operand columns per head: 64 (head dim 64), 96 = head dim 80 (OpenCLIP ViT-H/14: 1280 / 16 [UPSTREAM
// open_clip model_configs]) or 88 (ViT-g-14: 1408 / 16), and 128 = head dim 104 (ViT-bigG-14: 1664 / 16), zero-padded to three / four
// 32-column MFMA blocks when the runner packs its weights (vit.hip).  The softmax scale is an argument (1 / 8; in the padded widths
// 1 / sqrt(head dim), not 1 / sqrt(columns)): the padded columns are zero in q, k and v, so scores, output and gradients are those of
// the narrower head, and the padded columns of `out` and `dqkv` are exact zeros (sums of products with a zero operand).
// Per width, 64 | 96 | 128:
//   score products   4 | 6 | 8 k-steps of v_mfma_f32_32x32x16_{bf16,f16} (own_frags keeps as many fragments per tensor)
//   second products  2 | 3 | 4 output blocks of 32 columns (16 accumulator registers per lane, block and product)
//   row-major image  rows of 72 | 104 | 136 elements = 9 | 13 | 17 16-byte slots: all odd, so the 16 rows of every ds_read_b128 lane
//                    group (rows distinct mod 16) start in 16 distinct slots of the 64-bank row -- conflict-free
//   transposed image 64 | 96 | 128 rows of TRS = 132 elements
//   staging          8 | 16 | 16 piece slots per token row, 8 | 12 | 16 of them live: the slot index stays a shift / mask at every
//                    width; at 96 and 128 the eight-lane row sum of the dK / dV kernel becomes a sixteen-lane one, dead slots hold
//                    zeros and write nothing (at 64 the dead-slot test and the fourth shuffle step fold away, at 128 the test alone)
//   waves_per_eu     4 / 4 / 3 | 3 / 3 / 2 | 3 / 2 / 2 (forward / dQ / dK+dV), i.e. budgets of 128 / 128 / 168 | 168 / 168 / 256 |
//                    168 / 256 / 256 registers per lane.
//                    At 96 columns the forward spills 8 registers at 4 waves (qf 24 + O accumulators 48 + the score tile 16 +
//                    addressing) and uses 137 at 3; the dK + dV kernel keeps its keys' K and V fragments (48) and the dK / dV
//                    accumulators (96) in registers, cannot run at 3, and its LDS allows one workgroup per CU anyway.
//                    At 128 columns the forward (qf 32 + O 64 + score tile 16 + addressing = 161) still fits 3; dQ (qf, dof 64 +
//                    accumulators 64 + two score tiles 32 = 231) needs the 256 budget; dK + dV in one pass (fragments 64 + accumulators
//                    128 + two score tiles 32 + staging) takes all 256 and spills 15 registers, so it runs in two column passes
//                    (Blk::NCP, the note in the kernel): 248 registers, no scratch.  AGPR accumulators were the other way out: they
//                    need one wave per SIMD, i.e. workgroups of at most four waves and nothing to overlap a wave's LDS and global
//                    latency with; two waves per SIMD at 1.5 x the MFMA work of that kernel were preferred.
//   LDS              forward 35 968 | 52 608 | 69 248 B, dQ 53 760 | 78 592 | 103 424 B, dK + dV 71 680 | 104 960 | 138 240 B of the
//                    CU's 160 KiB: the chunk stays 128 tokens at every width, so T <= 640 holds at 128 columns too.
//                    Registers, LDS and occupancy of the padded instances: DESIGN.md, the attention table of section 6d.
// ---------------------------------------------------------------------------------------------------------------
constexpr int CH = 128;             // tokens per LDS chunk (four 32-token MFMA blocks)
constexpr int TRS = CH + 4;         // row stride (elements) of a transposed [HDP][CH] image: 66 dwords = 2 mod 64 banks, so the 32
                                    // rows d .. d+31 of one 8-byte fragment read fall into 32 distinct bank pairs
constexpr int STG_NP = 4;           // pieces in flight per thread and tensor (CH * 8 = 1024 pieces at 64 columns: one pass for >= 256 threads)
constexpr int WPB = 5;              // waves per workgroup: a head with more 32-token blocks is split over gridDim.z workgroups
template <int HDP>
struct Blk {
    static_assert(HDP == 64 || HDP == 96 || HDP == 128, "operand columns per head");
    static constexpr int KS = HDP / 16;             // k-steps of a score product
    static constexpr int NDJ = HDP / 32;            // 32-column blocks of a second product's output
    static constexpr int NPR = HDP / 8;             // live 16-byte pieces per token row
    static constexpr int LD = HDP + 8;              // row-major LDS row (elements)
    static constexpr int SPR = HDP == 64 ? 8 : 16;  // piece slots per staged token row (a power of two >= NPR)
    static constexpr int NSLOT = CH * SPR;          // piece slots per chunk
    static constexpr int WPE_FWD = HDP == 64 ? 4 : 3, WPE_DQ = HDP == 128 ? 2 : WPE_FWD, WPE_DKV = HDP == 64 ? 3 : 2;      // the waves_per_eu pins
    static constexpr int NCP = HDP == 128 ? 2 : 1;  // column passes of the dK + dV kernel: each holds NDJ / NCP output blocks of dK and of dV
};

// rows t0 .. t0+CH-1 of a [T][HDP] matrix (zero beyond T) -> row-major image and / or transposed image, by 16-byte piece slots.
// ALL the pieces a thread owns are requested before the first one is written to LDS: written as load -> write per piece
// (the loop this replaces) every piece paid its own global round trip -- 3-4 dependent round trips per tensor and chunk, and with two
// workgroups per CU nothing to hide them behind: the dK / dV kernel spent 760 of its 990 us per layer (ViT-L/14, 256 cutouts) in
// its staging loops, reading 0.8 GB at 1.1 TB/s (timing experiment of round 6: staging only 763 us, compute only 363 us).
template <typename F, int HDP>
__device__ __forceinline__ void stage_put(const V8<F>& v, int c, El<F>* rm, El<F>* tr) {
    using B = Blk<HDP>;
    const int row = c / B::SPR, kc = c % B::SPR;
    if (kc >= B::NPR) return;
    if (rm) *reinterpret_cast<V8<F>*>(&rm[row * B::LD + kc * 8]) = v;
    if (tr) {
#pragma unroll
        for (int e = 0; e < 8; ++e) tr[(kc * 8 + e) * TRS + row] = v[e];
    }
}
// piece slot c of a chunk; zero beyond T, in a dead slot and beyond the chunk
template <typename F, int HDP>
__device__ __forceinline__ V8<F> stage_get(const El<F>* src, long long ld, int t0, int T, int c) {
    using B = Blk<HDP>;
    const int row = c / B::SPR, kc = c % B::SPR;
    V8<F> v = {0, 0, 0, 0, 0, 0, 0, 0};          // (a branch here, not tile_get's clamp + select: that form measured 2 % slower in these kernels)
    if (c < B::NSLOT && kc < B::NPR && t0 + row < T) v = *reinterpret_cast<const V8<F>*>(src + (long long)(t0 + row) * ld + kc * 8);
    return v;
}
// two matrices with the same row stride at once (K and V of a chunk): both tensors' pieces in flight together
template <typename F, int HDP>
__device__ __forceinline__ void stage_chunk2(const El<F>* srcA, const El<F>* srcB, long long ld, int t0, int T, El<F>* rmA, El<F>* trA,
                                             El<F>* rmB, El<F>* trB, int tid, int nthr) {
    constexpr int NSLOT = Blk<HDP>::NSLOT;
    for (int cb = tid; cb < NSLOT; cb += STG_NP * nthr) {
        V8<F> va[STG_NP], vb[STG_NP];
#pragma unroll
        for (int i = 0; i < STG_NP; ++i) va[i] = stage_get<F, HDP>(srcA, ld, t0, T, cb + i * nthr);
#pragma unroll
        for (int i = 0; i < STG_NP; ++i) vb[i] = stage_get<F, HDP>(srcB, ld, t0, T, cb + i * nthr);
#pragma unroll
        for (int i = 0; i < STG_NP; ++i)
            if (cb + i * nthr < NSLOT) stage_put<F, HDP>(va[i], cb + i * nthr, rmA, trA);
#pragma unroll
        for (int i = 0; i < STG_NP; ++i)
            if (cb + i * nthr < NSLOT) stage_put<F, HDP>(vb[i], cb + i * nthr, rmB, trB);
    }
}
// the B-operand fragments of this lane's owned token t (zero beyond T)
template <typename F, int KS>
__device__ __forceinline__ void own_frags(const El<F>* src, long long ld, int t, int T, V8<F> (&f)[KS], int lane) {
    const int fk = 8 * (lane >> 5);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        f[ks] = V8<F>{0, 0, 0, 0, 0, 0, 0, 0};
        if (t < T) f[ks] = *reinterpret_cast<const V8<F>*>(src + (long long)t * ld + ks * 16 + fk);
    }
}
// acc = rows 32sb.. of the row-major chunk image (A) x owned tokens (B): [chunk token][owned token]
template <typename F, int KS>
__device__ __forceinline__ void mma_chunk_own(const El<F>* A, int sb, const V8<F> (&b)[KS], f32x16& acc, int lane) {
    constexpr int LD = 16 * KS + 8;
    const int fr = lane & 31, fk = 8 * (lane >> 5);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const V8<F> a = *reinterpret_cast<const V8<F>*>(&A[(sb * 32 + fr) * LD + ks * 16 + fk]);
        F::mfma(a, b[ks], acc);
    }
}
// k slot 8h+s of step (sb, G) is chunk token 32sb + 16G + 8(s>>2) + 4h + (s&3)
template <typename F>
__device__ __forceinline__ V8<F> tr_frag_chunk(const El<F>* Tt, int dj, int sb, int G, int lane) {
    const int d = dj * 32 + (lane & 31), t0 = 32 * sb + 16 * G + 4 * (lane >> 5);
    const V4<F> lo = *reinterpret_cast<const V4<F>*>(Tt + d * TRS + t0);
    const V4<F> hi = *reinterpret_cast<const V4<F>*>(Tt + d * TRS + t0 + 8);
    return V8<F>{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
// o[dj] += (accumulators a: rows = chunk tokens 32sb.., lane column = owned token) as A  x  transposed chunk image
template <typename F, int NDJ>
__device__ __forceinline__ void mma_acc_tr_chunk(const f32x16& a, const El<F>* Tt, int sb, f32x16 (&o)[NDJ], int lane) {
#pragma unroll
    for (int G = 0; G < 2; ++G) {
        const V8<F> fa = acc_frag<F>(a, G);
#pragma unroll
        for (int dj = 0; dj < NDJ; ++dj) F::mfma(fa, tr_frag_chunk<F>(Tt, dj, sb, G, lane), o[dj]);
    }
}
// multiply the register rows of o (row of register r: (r&3) + 8(r>>2) + 4(lane>>5)) by line[row]
template <int NDJ>
__device__ __forceinline__ void scale_rows(f32x16 (&o)[NDJ], const float* line, int lane) {
    const int hh = lane >> 5;
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
        const float4 a4 = *reinterpret_cast<const float4*>(&line[8 * rg + 4 * hh]);
        const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int dj = 0; dj < NDJ; ++dj) o[dj][rg * 4 + q] *= av[q];
    }
}

// forward; also writes LSE_i (natural log) for the backward
template <typename F, int HDP>
__global__ __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(Blk<HDP>::WPE_FWD, Blk<HDP>::WPE_FWD))) void mha_fwd_blk_kernel(
    const El<F>* __restrict__ qkv, El<F>* __restrict__ out, float* __restrict__ lse, int T, int C, int heads, float scale, int xcd) {
    using E = El<F>;
    using B = Blk<HDP>;
    __shared__ __attribute__((aligned(16))) E Ks[CH * B::LD];
    __shared__ __attribute__((aligned(16))) E Vt[HDP * TRS];
    __shared__ __attribute__((aligned(16))) float s_line[WPB][32];
    const int tid = threadIdx.x, lane = tid & 63, w = blockIdx.z * (blockDim.x >> 6) + (tid >> 6), hh = lane >> 5;
    const bool active = 32 * w < T;                        // the last workgroup of a head may carry a wave without tokens
    int h, n;
    block_head(xcd, h, n);
    const long long ld = 3LL * C;
    const E* base = qkv + (long long)n * T * ld + h * HDP;
    const int q = 32 * w + (lane & 31);                    // this lane's query
    V8<F> qf[B::KS];
    own_frags<F>(base, ld, q, T, qf, lane);
    float m = -INFINITY, l = 0.f;                           // running max (base-2 domain) and sum of this lane's query
    const float sl2 = scale * LOG2E;
    f32x16 o[B::NDJ];
    zero_blocks(o);
    float* line = s_line[tid >> 6];
    for (int c0 = 0; c0 < T; c0 += CH) {
        __syncthreads();
        stage_chunk2<F, HDP>(base + C, base + 2 * C, ld, c0, T, Ks, nullptr, nullptr, Vt, tid, blockDim.x);
        __syncthreads();
        const int nsb = active ? min(CH / 32, (T - c0 + 31) / 32) : 0;
        for (int sb = 0; sb < nsb; ++sb) {
            f32x16 st;                                      // [key 32sb..][query]
            zero16(st);
            mma_chunk_own<F>(Ks, sb, qf, st, lane);
            // scores in the base-2 domain (one multiply by scale * log2(e), then v_exp_f32 directly); only the last 32-key
            // block of a head can hold keys beyond T (wave-uniform test)
            float bm = -INFINITY;
            const bool partial = c0 + sb * 32 + 32 > T;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = st[r] * sl2;
                if (partial) {
                    const int j = c0 + sb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                    v = (j < T) ? v : -INFINITY;
                }
                st[r] = v;
                bm = fmaxf(bm, v);
            }
            bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
            const float mn = fmaxf(m, bm);                  // finite: every 32-key block that is visited has a valid key
            const float alpha = __builtin_amdgcn_exp2f(m - mn);     // 0 on the first block
            float sum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float e = __builtin_amdgcn_exp2f(st[r] - mn);
                st[r] = e;
                sum += e;
            }
            sum += __shfl_xor(sum, 32, 64);
            l = l * alpha + sum;
            m = mn;
            if (__any(alpha != 1.f)) {                      // the running maximum of some query moved: rescale its O row
                if (hh == 0) line[lane] = alpha;
                __builtin_amdgcn_wave_barrier();
                scale_rows(o, line, lane);
                __builtin_amdgcn_wave_barrier();
            }
            mma_acc_tr_chunk<F>(st, Vt, sb, o, lane);       // O[query][d] += P[query][key] V[key][d]
        }
    }
    if (!active) return;
    if (hh == 0) {
        line[lane] = 1.f / l;
        if (q < T && lse) lse[((long long)n * heads + h) * T + q] = (m + __builtin_amdgcn_logf(l)) * 0.6931471805599453f;
    }
    __builtin_amdgcn_wave_barrier();
    scale_rows(o, line, lane);
    store_rows_global<F>(o, w, out + (long long)n * T * C + h * HDP, C, T, lane);
}

// dQ: P is recomputed from the LSE, D_q = sum_d dO_qd O_qd from global
template <typename F, int HDP>
__global__ __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(Blk<HDP>::WPE_DQ, Blk<HDP>::WPE_DQ))) void mha_bwd_dq_blk_kernel(
    const El<F>* __restrict__ qkv, const El<F>* __restrict__ o, const El<F>* __restrict__ dout, const float* __restrict__ lse,
    El<F>* __restrict__ dqkv, int T, int C, int heads, float scale, int xcd) {
    using E = El<F>;
    using B = Blk<HDP>;
    __shared__ __attribute__((aligned(16))) E Ks[CH * B::LD];
    __shared__ __attribute__((aligned(16))) E Vs[CH * B::LD];
    __shared__ __attribute__((aligned(16))) E Kt[HDP * TRS];
    const int tid = threadIdx.x, lane = tid & 63, w = blockIdx.z * (blockDim.x >> 6) + (tid >> 6), hh = lane >> 5;
    const bool active = 32 * w < T;
    int h, n;
    block_head(xcd, h, n);
    const long long ld = 3LL * C;
    const E* base = qkv + (long long)n * T * ld + h * HDP;
    const E* dob = dout + (long long)n * T * C + h * HDP;
    const E* ob = o + (long long)n * T * C + h * HDP;
    const int q = 32 * w + (lane & 31);
    V8<F> qf[B::KS], dof[B::KS];
    own_frags<F>(base, ld, q, T, qf, lane);
    own_frags<F>(dob, C, q, T, dof, lane);
    float lse_q = INFINITY, D_q = 0.f;                      // exp(x - inf) = 0 for padded queries
    if (q < T) {
        lse_q = lse[((long long)n * heads + h) * T + q];
        float dsum = 0.f;
#pragma unroll
        for (int i = 0; i < B::NPR / 2; ++i) {              // this half-wave's half of the head's columns
            const V8<F> a = *reinterpret_cast<const V8<F>*>(dob + (long long)q * C + hh * (HDP / 2) + i * 8);
            const V8<F> b = *reinterpret_cast<const V8<F>*>(ob + (long long)q * C + hh * (HDP / 2) + i * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) dsum += (float)a[e] * (float)b[e];
        }
        D_q = dsum;
    }
    D_q += __shfl_xor(D_q, 32, 64);
    const float sl2 = scale * LOG2E, lse2 = lse_q * LOG2E;  // base-2 domain
    f32x16 acc[B::NDJ];
    zero_blocks(acc);
    for (int c0 = 0; c0 < T; c0 += CH) {
        __syncthreads();
        stage_chunk2<F, HDP>(base + C, base + 2 * C, ld, c0, T, Ks, Kt, Vs, nullptr, tid, blockDim.x);
        __syncthreads();
        const int nsb = active ? min(CH / 32, (T - c0 + 31) / 32) : 0;
        for (int sb = 0; sb < nsb; ++sb) {
            f32x16 pt, dpt;                                 // [key][query]
            zero16(pt); zero16(dpt);
            mma_chunk_own<F>(Ks, sb, qf, pt, lane);         // S^T  = K Q^T
            mma_chunk_own<F>(Vs, sb, dof, dpt, lane);       // dP^T = V dO^T
            const bool partial = c0 + sb * 32 + 32 > T;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float p = __builtin_amdgcn_exp2f(pt[r] * sl2 - lse2);
                if (partial) {
                    const int j = c0 + sb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                    p = (j < T) ? p : 0.f;
                }
                dpt[r] = scale * p * (dpt[r] - D_q);        // dS^T
            }
            mma_acc_tr_chunk<F>(dpt, Kt, sb, acc, lane);    // dQ[query][d] += dS[query][key] K[key][d]
        }
    }
    if (active) store_rows_global<F>(acc, w, dqkv + (long long)n * T * ld + h * HDP, ld, T, lane);
}

// dK, dV
template <typename F, int HDP>
__global__ __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(Blk<HDP>::WPE_DKV, Blk<HDP>::WPE_DKV))) void mha_bwd_dkv_blk_kernel(
    const El<F>* __restrict__ qkv, const El<F>* __restrict__ o, const El<F>* __restrict__ dout, const float* __restrict__ lse,
    El<F>* __restrict__ dqkv, int T, int C, int heads, float scale, int xcd) {
    using E = El<F>;
    using B = Blk<HDP>;
    __shared__ __attribute__((aligned(16))) E Qs[CH * B::LD];
    __shared__ __attribute__((aligned(16))) E dOs[CH * B::LD];
    __shared__ __attribute__((aligned(16))) E Qt[HDP * TRS];
    __shared__ __attribute__((aligned(16))) E dOt[HDP * TRS];
    __shared__ __attribute__((aligned(16))) float s_lse[CH], s_D[CH];
    const int tid = threadIdx.x, lane = tid & 63, w = blockIdx.z * (blockDim.x >> 6) + (tid >> 6), hh = lane >> 5;
    const bool active = 32 * w < T;
    int h, n;
    block_head(xcd, h, n);
    const long long ld = 3LL * C;
    const E* base = qkv + (long long)n * T * ld + h * HDP;
    const E* dob = dout + (long long)n * T * C + h * HDP;
    const E* ob = o + (long long)n * T * C + h * HDP;
    const float* lse_h = lse + ((long long)n * heads + h) * T;
    const int key = 32 * w + (lane & 31);
    const bool key_ok = key < T;
    const float sl2 = scale * LOG2E;
    V8<F> kf[B::KS], vf[B::KS];
    own_frags<F>(base + C, ld, key, T, kf, lane);
    own_frags<F>(base + 2 * C, ld, key, T, vf, lane);
    const int nthr = blockDim.x;
    // Column passes (B::NCP; 1 at 64 and 96 columns, where this loop folds away): at 128 columns the K and V fragments (64 registers)
    // and all of dK and dV (128) do not fit the 256 registers of two waves per SIMD beside the score tiles and the staging pieces, so
    // a pass accumulates NDJ / NCP = 2 of the four 32-column blocks of dK and of dV and the chunks are streamed once per pass
    // (the scores are recomputed: 16 + 8 MFMAs per 32 x 32 block and pass instead of 16 + 16 once)
    constexpr int NDP = B::NDJ / B::NCP;
    int cp = 0;
    do {        // (a do-while whose condition is a constant false at one pass: the front end emits no loop there)
        f32x16 dk[NDP], dv[NDP];
        zero_blocks(dk); zero_blocks(dv);
        for (int c0 = 0; c0 < T; c0 += CH) {
            __syncthreads();
            // Q chunk, dO chunk and beside it D_i = sum_d dO_id O_id (the SPR slots of a row sit in SPR neighbouring lanes, one 8-column
            // piece each; dead slots hold zeros); the pieces of all three tensors are requested before the first LDS write (stage_put's note)
            for (int cb = tid; cb < B::NSLOT; cb += STG_NP * nthr) {
                V8<F> vq[STG_NP], vd[STG_NP], vo[STG_NP];
#pragma unroll
                for (int i = 0; i < STG_NP; ++i) vq[i] = stage_get<F, HDP>(base, ld, c0, T, cb + i * nthr);
#pragma unroll
                for (int i = 0; i < STG_NP; ++i) vd[i] = stage_get<F, HDP>(dob, C, c0, T, cb + i * nthr);
#pragma unroll
                for (int i = 0; i < STG_NP; ++i) vo[i] = stage_get<F, HDP>(ob, C, c0, T, cb + i * nthr);
#pragma unroll
                for (int i = 0; i < STG_NP; ++i)
                    if (cb + i * nthr < B::NSLOT) stage_put<F, HDP>(vq[i], cb + i * nthr, Qs, Qt);
#pragma unroll
                for (int i = 0; i < STG_NP; ++i) {
                    const int c = cb + i * nthr;                // (c >= NSLOT only in whole waves: the shuffles below stay converged)
                    if (c < B::NSLOT) {
                        const int row = c / B::SPR, kc = c % B::SPR;
                        float part = 0.f;
#pragma unroll
                        for (int e = 0; e < 8; ++e) part += (float)vd[i][e] * (float)vo[i][e];
                        stage_put<F, HDP>(vd[i], c, dOs, dOt);
                        part += __shfl_xor(part, 1, 64);
                        part += __shfl_xor(part, 2, 64);
                        part += __shfl_xor(part, 4, 64);
                        if (B::SPR == 16) part += __shfl_xor(part, 8, 64);
                        if (kc == 0) {
                            s_D[row] = part;
                            s_lse[row] = (c0 + row < T) ? lse_h[c0 + row] * LOG2E : INFINITY;      // base-2 domain
                        }
                    }
                }
            }
            __syncthreads();
            const int nsb = active ? min(CH / 32, (T - c0 + 31) / 32) : 0;
            for (int sb = 0; sb < nsb; ++sb) {
                f32x16 p, dp;                                   // [query 32sb..][key]
                zero16(p); zero16(dp);
                mma_chunk_own<F>(Qs, sb, kf, p, lane);          // S  = Q K^T
                mma_chunk_own<F>(dOs, sb, vf, dp, lane);        // dP = dO V^T
#pragma unroll
                for (int rg = 0; rg < 4; ++rg) {
                    const int i0 = sb * 32 + 8 * rg + 4 * hh;
                    const float4 l4 = *reinterpret_cast<const float4*>(&s_lse[i0]);
                    const float4 d4 = *reinterpret_cast<const float4*>(&s_D[i0]);
                    const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dvv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) {
                        const int r = rg * 4 + qq;
                        const float pv = key_ok ? __builtin_amdgcn_exp2f(p[r] * sl2 - lv[qq]) : 0.f;
                        p[r] = pv;
                        dp[r] = scale * pv * (dp[r] - dvv[qq]);   // dS
                    }
                }
                mma_acc_tr_chunk<F>(dp, Qt + cp * 32 * NDP * TRS, sb, dk, lane);     // dK[key][d] += dS[query][key] Q[query][d]
                mma_acc_tr_chunk<F>(p, dOt + cp * 32 * NDP * TRS, sb, dv, lane);     // dV[key][d] += P[query][key] dO[query][d]
            }
        }
        if (!active) continue;                              // (a wave without tokens still stages and meets the barriers of the next pass)
        E* obase = dqkv + (long long)n * T * ld + h * HDP + cp * 32 * NDP;
        store_rows_global<F>(dk, w, obase + C, ld, T, lane);
        store_rows_global<F>(dv, w, obase + 2 * C, ld, T, lane);
    } while (B::NCP > 1 && ++cp < B::NCP);
}

}  // namespace
