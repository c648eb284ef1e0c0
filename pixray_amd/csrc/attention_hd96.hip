// Multi-head self-attention for heads of 96 operand columns: head dim 80 (OpenCLIP ViT-H/14: 1280 / 16 [UPSTREAM open_clip
// model_configs]) zero-padded to three 32-column MFMA blocks when the runner packs its weights (vit.hip).  The workgroup-per-(image,
// head) family of attention_kernels.inc ("blk": one wave per 32 owned tokens, the other operand streamed over 128-token LDS chunks,
// scores with the owned tokens on the lane columns so that the probabilities are already the A operand of the second product),
// restated for a wider head:
//   score products   6 k-steps of v_mfma_f32_32x32x16_{bf16,f16} instead of 4 (own_frags keeps 6 fragments per tensor)
//   second products  3 output blocks of 32 columns instead of 2 (16 more accumulator registers per lane and product)
//   row-major image  rows of 104 elements = 52 dwords = 13 16-byte slots: 13 is odd, so the 16 rows of every ds_read_b128 lane
//                    group (rows distinct mod 16) start in 16 distinct slots of the 64-bank row -- conflict-free, as the 64-wide
//                    kernels' 72-element rows (9 slots) are
//   transposed image 96 rows of 132 elements, the 64-wide kernels' stride (66 dwords = 2 mod 64 banks)
//   staging          16 piece slots per token row, 12 of them live: the slot index stays a shift / mask and the eight-lane row sum
//                    of the dK / dV kernel becomes a sixteen-lane one; dead slots hold zeros and write nothing
// The softmax scale is an argument (1 / sqrt(80), not 1 / sqrt(96)): the padded columns are zero in q, k and v, so scores, output
// and gradients are those of the 80-wide head, and the padded columns of `out` and `dqkv` are exact zeros (sums of products with a
// zero operand).  T <= 640, as for the 64-wide family; there is no tile-kernel fallback at this width -- a longer sequence is an
// error.  Registers, LDS and occupancy of the six instances: DESIGN.md, the attention table.
#include "attention.h"

namespace {

struct FmtBf16 {
    using T = bf16_t; using V8 = bf16x8; using V4 = bf16x4;
    static __device__ __forceinline__ f32x16 mfma(V8 a, V8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
struct FmtF16 {
    using T = half_t; using V8 = f16x8; using V4 = f16x4;
    static __device__ __forceinline__ f32x16 mfma(V8 a, V8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};

constexpr int HDP = 96;             // operand columns per head
constexpr int KS = HDP / 16;        // k-steps of a score product
constexpr int NDJ = HDP / 32;       // 32-column blocks of a second product's output
constexpr int NPR = HDP / 8;        // live 16-byte pieces per token row
constexpr int LD = HDP + 8;         // row-major LDS row (elements)
constexpr int CH = 128;             // tokens per LDS chunk (four 32-token MFMA blocks)
constexpr int TRS = CH + 4;         // row stride of a transposed [HDP][CH] image
constexpr int SPR = 16;             // piece slots per staged token row (a power of two >= NPR)
constexpr int NSLOT = CH * SPR;     // piece slots per chunk
constexpr int STG_NP = 4;           // pieces in flight per thread and tensor
constexpr int WPB = 5;              // waves per workgroup: a head with more 32-token blocks is split over gridDim.z workgroups
constexpr float LOG2E = 1.4426950408889634f;

template <typename F>
__device__ __forceinline__ void stage_put(const typename F::V8& v, int c, typename F::T* rm, typename F::T* tr) {
    const int row = c / SPR, kc = c % SPR;
    if (kc >= NPR) return;
    if (rm) *reinterpret_cast<typename F::V8*>(&rm[row * LD + kc * 8]) = v;
    if (tr) {
#pragma unroll
        for (int e = 0; e < 8; ++e) tr[(kc * 8 + e) * TRS + row] = v[e];
    }
}
// piece slot c of rows t0 .. t0+CH-1 of a [T][HDP] matrix; zero beyond T, in a dead slot and beyond the chunk
template <typename F>
__device__ __forceinline__ typename F::V8 stage_get(const typename F::T* src, long long ld, int t0, int T, int c) {
    const int row = c / SPR, kc = c % SPR;
    typename F::V8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (c < NSLOT && kc < NPR && t0 + row < T) v = *reinterpret_cast<const typename F::V8*>(src + (long long)(t0 + row) * ld + kc * 8);
    return v;
}
// two matrices with the same row stride at once (K and V of a chunk): all of a thread's pieces are requested before the first LDS write
template <typename F>
__device__ __forceinline__ void stage_chunk2(const typename F::T* srcA, const typename F::T* srcB, long long ld, int t0, int T,
                                             typename F::T* rmA, typename F::T* trA, typename F::T* rmB, typename F::T* trB, int tid, int nthr) {
    for (int cb = tid; cb < NSLOT; cb += STG_NP * nthr) {
        typename F::V8 va[STG_NP], vb[STG_NP];
#pragma unroll
        for (int i = 0; i < STG_NP; ++i) va[i] = stage_get<F>(srcA, ld, t0, T, cb + i * nthr);
#pragma unroll
        for (int i = 0; i < STG_NP; ++i) vb[i] = stage_get<F>(srcB, ld, t0, T, cb + i * nthr);
#pragma unroll
        for (int i = 0; i < STG_NP; ++i)
            if (cb + i * nthr < NSLOT) stage_put<F>(va[i], cb + i * nthr, rmA, trA);
#pragma unroll
        for (int i = 0; i < STG_NP; ++i)
            if (cb + i * nthr < NSLOT) stage_put<F>(vb[i], cb + i * nthr, rmB, trB);
    }
}
// the B-operand fragments of this lane's owned token t (zero beyond T)
template <typename F>
__device__ __forceinline__ void own_frags(const typename F::T* src, long long ld, int t, int T, typename F::V8 (&f)[KS], int lane) {
    const int fk = 8 * (lane >> 5);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        f[ks] = typename F::V8{0, 0, 0, 0, 0, 0, 0, 0};
        if (t < T) f[ks] = *reinterpret_cast<const typename F::V8*>(src + (long long)t * ld + ks * 16 + fk);
    }
}
// acc = rows 32sb.. of the row-major chunk image (A) x owned tokens (B): [chunk token][owned token]
template <typename F>
__device__ __forceinline__ void mma_chunk_own(const typename F::T* A, int sb, const typename F::V8 (&b)[KS], f32x16& acc, int lane) {
    const int fr = lane & 31, fk = 8 * (lane >> 5);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const typename F::V8 a = *reinterpret_cast<const typename F::V8*>(&A[(sb * 32 + fr) * LD + ks * 16 + fk]);
        acc = F::mfma(a, b[ks], acc);
    }
}
// accumulator registers 8G .. 8G+7 as an A fragment: k slot 8h+s of step (sb, G) is chunk token 32sb + 16G + 8(s>>2) + 4h + (s&3)
template <typename F>
__device__ __forceinline__ typename F::V8 acc_frag(const f32x16& a, int G) {
    typename F::V8 f;
#pragma unroll
    for (int s = 0; s < 8; ++s) f[s] = (typename F::T)a[8 * G + s];
    return f;
}
template <typename F>
__device__ __forceinline__ typename F::V8 tr_frag_chunk(const typename F::T* Tt, int dj, int sb, int G, int lane) {
    const int d = dj * 32 + (lane & 31), t0 = 32 * sb + 16 * G + 4 * (lane >> 5);
    const typename F::V4 lo = *reinterpret_cast<const typename F::V4*>(Tt + d * TRS + t0);
    const typename F::V4 hi = *reinterpret_cast<const typename F::V4*>(Tt + d * TRS + t0 + 8);
    return typename F::V8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
// o[dj] += (accumulators a: rows = chunk tokens 32sb.., lane column = owned token) as A  x  transposed chunk image
template <typename F>
__device__ __forceinline__ void mma_acc_tr_chunk(const f32x16& a, const typename F::T* Tt, int sb, f32x16 (&o)[NDJ], int lane) {
#pragma unroll
    for (int G = 0; G < 2; ++G) {
        const typename F::V8 fa = acc_frag<F>(a, G);
#pragma unroll
        for (int dj = 0; dj < NDJ; ++dj) o[dj] = F::mfma(fa, tr_frag_chunk<F>(Tt, dj, sb, G, lane), o[dj]);
    }
}
__device__ __forceinline__ void zero16(f32x16& a) {
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = 0.f;
}
__device__ __forceinline__ void zero_blocks(f32x16 (&o)[NDJ]) {
#pragma unroll
    for (int dj = 0; dj < NDJ; ++dj) zero16(o[dj]);
}
// multiply the register rows of o (row of register r: (r&3) + 8(r>>2) + 4(lane>>5)) by line[row]
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
// write the C-layout rows 32*rb .. 32*rb+31 of a [t][HDP] result (a[dj] = columns 32dj ..) to global rows < T
template <typename F>
__device__ __forceinline__ void store_rows_global(const f32x16 (&a)[NDJ], int rb, typename F::T* out, long long ld, int T, int lane) {
    const int col = lane & 31, r0 = 32 * rb + 4 * (lane >> 5);
#pragma unroll
    for (int dj = 0; dj < NDJ; ++dj)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = r0 + (r & 3) + 8 * (r >> 2);
            if (i < T) out[(long long)i * ld + dj * 32 + col] = (typename F::T)a[dj][r];
        }
}
__device__ __forceinline__ void block_head(int xcd, int& h, int& n) {
    const unsigned flat = blockIdx.y * gridDim.x + blockIdx.x, nwg = gridDim.x * gridDim.y;
    const unsigned lin = xcd ? xcd_linear(flat, nwg) : flat;
    h = (int)(lin % gridDim.x); n = (int)(lin / gridDim.x);
}

// forward: online softmax per owned query (running max / sum per lane, base-2 domain); the rescale factors reach the O accumulators
// (queries on register rows) through a 32-float LDS line per wave.  Also writes LSE_i (natural log) for the backward.
template <typename F>
__global__ __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(3, 3))) void mha96_fwd_kernel(
    const typename F::T* __restrict__ qkv, typename F::T* __restrict__ out, float* __restrict__ lse, int T, int C, int heads, float scale, int xcd) {
    using E = typename F::T;
    __shared__ __attribute__((aligned(16))) E Ks[CH * LD];
    __shared__ __attribute__((aligned(16))) E Vt[HDP * TRS];
    __shared__ __attribute__((aligned(16))) float s_line[WPB][32];
    const int tid = threadIdx.x, lane = tid & 63, w = blockIdx.z * (blockDim.x >> 6) + (tid >> 6), hh = lane >> 5;
    const bool active = 32 * w < T;                        // the last workgroup of a head may carry a wave without tokens
    int h, n;
    block_head(xcd, h, n);
    const long long ld = 3LL * C;
    const E* base = qkv + (long long)n * T * ld + h * HDP;
    const int q = 32 * w + (lane & 31);                    // this lane's query
    typename F::V8 qf[KS];
    own_frags<F>(base, ld, q, T, qf, lane);
    float m = -INFINITY, l = 0.f;
    const float sl2 = scale * LOG2E;
    f32x16 o[NDJ];
    zero_blocks(o);
    float* line = s_line[tid >> 6];
    for (int c0 = 0; c0 < T; c0 += CH) {
        __syncthreads();
        stage_chunk2<F>(base + C, base + 2 * C, ld, c0, T, Ks, nullptr, nullptr, Vt, tid, blockDim.x);
        __syncthreads();
        const int nsb = active ? min(CH / 32, (T - c0 + 31) / 32) : 0;
        for (int sb = 0; sb < nsb; ++sb) {
            f32x16 st;                                      // [key 32sb..][query]
            zero16(st);
            mma_chunk_own<F>(Ks, sb, qf, st, lane);
            float bm = -INFINITY;
            const bool partial = c0 + sb * 32 + 32 > T;     // only the last 32-key block of a head can hold keys beyond T
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

// dQ: owned queries, chunks of K / V / K^T; P is recomputed from the LSE, D_q = sum_d dO_qd O_qd from global
template <typename F>
__global__ __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(3, 3))) void mha96_bwd_dq_kernel(
    const typename F::T* __restrict__ qkv, const typename F::T* __restrict__ o, const typename F::T* __restrict__ dout,
    const float* __restrict__ lse, typename F::T* __restrict__ dqkv, int T, int C, int heads, float scale, int xcd) {
    using E = typename F::T;
    __shared__ __attribute__((aligned(16))) E Ks[CH * LD];
    __shared__ __attribute__((aligned(16))) E Vs[CH * LD];
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
    typename F::V8 qf[KS], dof[KS];
    own_frags<F>(base, ld, q, T, qf, lane);
    own_frags<F>(dob, C, q, T, dof, lane);
    float lse_q = INFINITY, D_q = 0.f;                      // exp(x - inf) = 0 for padded queries
    if (q < T) {
        lse_q = lse[((long long)n * heads + h) * T + q];
        float dsum = 0.f;
#pragma unroll
        for (int i = 0; i < NPR / 2; ++i) {                 // this half-wave's half of the head's columns
            const typename F::V8 a = *reinterpret_cast<const typename F::V8*>(dob + (long long)q * C + hh * (HDP / 2) + i * 8);
            const typename F::V8 b = *reinterpret_cast<const typename F::V8*>(ob + (long long)q * C + hh * (HDP / 2) + i * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) dsum += (float)a[e] * (float)b[e];
        }
        D_q = dsum;
    }
    D_q += __shfl_xor(D_q, 32, 64);
    const float sl2 = scale * LOG2E, lse2 = lse_q * LOG2E;  // base-2 domain
    f32x16 acc[NDJ];
    zero_blocks(acc);
    for (int c0 = 0; c0 < T; c0 += CH) {
        __syncthreads();
        stage_chunk2<F>(base + C, base + 2 * C, ld, c0, T, Ks, Kt, Vs, nullptr, tid, blockDim.x);
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

// dK, dV: owned keys, chunks of Q / dO / Q^T / dO^T with the per-query LSE and D staged beside them
template <typename F>
__global__ __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(2, 2))) void mha96_bwd_dkv_kernel(
    const typename F::T* __restrict__ qkv, const typename F::T* __restrict__ o, const typename F::T* __restrict__ dout,
    const float* __restrict__ lse, typename F::T* __restrict__ dqkv, int T, int C, int heads, float scale, int xcd) {
    using E = typename F::T;
    __shared__ __attribute__((aligned(16))) E Qs[CH * LD];
    __shared__ __attribute__((aligned(16))) E dOs[CH * LD];
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
    typename F::V8 kf[KS], vf[KS];
    own_frags<F>(base + C, ld, key, T, kf, lane);
    own_frags<F>(base + 2 * C, ld, key, T, vf, lane);
    f32x16 dk[NDJ], dv[NDJ];
    zero_blocks(dk); zero_blocks(dv);
    const int nthr = blockDim.x;
    for (int c0 = 0; c0 < T; c0 += CH) {
        __syncthreads();
        // Q chunk, dO chunk and beside it D_i = sum_d dO_id O_id (the sixteen slots of a row sit in sixteen neighbouring lanes; dead
        // slots hold zeros); the pieces of all three tensors are requested before the first LDS write
        for (int cb = tid; cb < NSLOT; cb += STG_NP * nthr) {
            typename F::V8 vq[STG_NP], vd[STG_NP], vo[STG_NP];
#pragma unroll
            for (int i = 0; i < STG_NP; ++i) vq[i] = stage_get<F>(base, ld, c0, T, cb + i * nthr);
#pragma unroll
            for (int i = 0; i < STG_NP; ++i) vd[i] = stage_get<F>(dob, C, c0, T, cb + i * nthr);
#pragma unroll
            for (int i = 0; i < STG_NP; ++i) vo[i] = stage_get<F>(ob, C, c0, T, cb + i * nthr);
#pragma unroll
            for (int i = 0; i < STG_NP; ++i)
                if (cb + i * nthr < NSLOT) stage_put<F>(vq[i], cb + i * nthr, Qs, Qt);
#pragma unroll
            for (int i = 0; i < STG_NP; ++i) {
                const int c = cb + i * nthr;                // (c >= NSLOT only in whole waves: the shuffles below stay converged)
                if (c < NSLOT) {
                    const int row = c / SPR, kc = c % SPR;
                    float part = 0.f;
#pragma unroll
                    for (int e = 0; e < 8; ++e) part += (float)vd[i][e] * (float)vo[i][e];
                    stage_put<F>(vd[i], c, dOs, dOt);
                    part += __shfl_xor(part, 1, 64);
                    part += __shfl_xor(part, 2, 64);
                    part += __shfl_xor(part, 4, 64);
                    part += __shfl_xor(part, 8, 64);
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
            mma_acc_tr_chunk<F>(dp, Qt, sb, dk, lane);      // dK[key][d] += dS[query][key] Q[query][d]
            mma_acc_tr_chunk<F>(p, dOt, sb, dv, lane);      // dV[key][d] += P[query][key] dO[query][d]
        }
    }
    if (!active) return;
    E* obase = dqkv + (long long)n * T * ld + h * HDP;
    store_rows_global<F>(dk, w, obase + C, ld, T, lane);
    store_rows_global<F>(dv, w, obase + 2 * C, ld, T, lane);
}

constexpr int MHA96_MAX_T = 640;

template <typename F>
int fwd96(const typename F::T* qkv, typename F::T* out, float* lse, int N, int T, int C, int heads, float scale, hipStream_t s) {
    const int nw = ceil_div(T, 32), nsplit = ceil_div(nw, WPB), wpb = ceil_div(nw, nsplit);
    hipLaunchKernelGGL(mha96_fwd_kernel<F>, dim3(heads, N, nsplit), dim3(64 * wpb), 0, s, qkv, out, lse, T, C, heads, scale, prx_xcd_local());
    PRX_LAUNCH_CHECK();
    return 0;
}
template <typename F>
int bwd96(const typename F::T* qkv, const typename F::T* out, const typename F::T* dout, const float* lse, typename F::T* dqkv, int N, int T,
          int C, int heads, float scale, hipStream_t s) {
    const int nw = ceil_div(T, 32), nsplit = ceil_div(nw, WPB), wpb = ceil_div(nw, nsplit);
    const dim3 g(heads, N, nsplit), b(64 * wpb);
    const int xcd = prx_xcd_local();
    hipLaunchKernelGGL(mha96_bwd_dq_kernel<F>, g, b, 0, s, qkv, out, dout, lse, dqkv, T, C, heads, scale, xcd);
    PRX_LAUNCH_CHECK();
    hipLaunchKernelGGL(mha96_bwd_dkv_kernel<F>, g, b, 0, s, qkv, out, dout, lse, dqkv, T, C, heads, scale, xcd);
    PRX_LAUNCH_CHECK();
    return 0;
}

}  // namespace

int prx_mha_fwd_hd96(const bf16_t* qkv, bf16_t* out, float* lse, int N, int T, int C, int heads, float scale, hipStream_t s, int h16) {
    PRX_REQUIRE(C == heads * HDP && T >= 1 && T <= MHA96_MAX_T && N >= 1,
                "mha(hd96): needs 96 columns per head and 1 <= T <= %d (T=%d C=%d heads=%d)", MHA96_MAX_T, T, C, heads);
    if (h16) return fwd96<FmtF16>(reinterpret_cast<const half_t*>(qkv), reinterpret_cast<half_t*>(out), lse, N, T, C, heads, scale, s);
    return fwd96<FmtBf16>(qkv, out, lse, N, T, C, heads, scale, s);
}
int prx_mha_bwd_hd96(const bf16_t* qkv, const bf16_t* out, const bf16_t* dout, const float* lse, bf16_t* dqkv, int N, int T, int C,
                     int heads, float scale, hipStream_t s, int h16) {
    PRX_REQUIRE(C == heads * HDP && T >= 1 && T <= MHA96_MAX_T && N >= 1,
                "mha(hd96) bwd: needs 96 columns per head and 1 <= T <= %d (T=%d C=%d heads=%d)", MHA96_MAX_T, T, C, heads);
    if (h16)
        return bwd96<FmtF16>(reinterpret_cast<const half_t*>(qkv), reinterpret_cast<const half_t*>(out), reinterpret_cast<const half_t*>(dout),
                             lse, reinterpret_cast<half_t*>(dqkv), N, T, C, heads, scale, s);
    return bwd96<FmtBf16>(qkv, out, dout, lse, dqkv, N, T, C, heads, scale, s);
}
