// Exact-f32 multi-head self-attention for the PRX_PREC_F32 parity mode (same operator as attention.hip:
// nn.MultiheadAttention inside clip.model.ResidualAttentionBlock [UPSTREAM openai/CLIP clip/model.py], call site
// slip.py:65), any sequence length, head dims 64 | 80 | 88 | 104, forward and activation-gradient backward.  Reached through the
// dispatcher of attention.hip alone (attention_f32.h).
//
// This is the checker's arithmetic, not the fast path: fp32 operands, fp32 VALU fma chains, one query (or key) per lane,
// the other side of the product broadcast from LDS in 64-token blocks with an online softmax.  What it must be is
// simple and exact; the bf16 MFMA kernels in attention.hip are measured against it.
#include "attention_f32.h"

namespace {

// Every kernel is templated on the head dim HD and on the head's column stride HS >= HD in qkv / out / dqkv: <64, 64> are the towers
// with 64-wide heads, <80, 96> the towers whose 80-wide heads are zero-padded to 96 operand columns (attention_kernels.h, vit.hip) --
// there the HS - HD pad columns are not read, and are written as zeros.
constexpr int BT = 64;        // tokens per LDS block

// stage `rows` x HD floats of a [T, ld] matrix (rows r0.., columns c0..c0+HD-1) into lds[BT][HD]; rows >= T are zeroed
template <int HD>
__device__ __forceinline__ void stage_block(const float* __restrict__ src, long long ld, int r0, int T, float* lds, int lane) {
#pragma unroll 4
    for (int idx = lane; idx < BT * (HD / 4); idx += 64) {
        const int row = idx / (HD / 4), c4 = idx % (HD / 4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r0 + row < T) v = *reinterpret_cast<const float4*>(src + (long long)(r0 + row) * ld + c4 * 4);
        *reinterpret_cast<float4*>(lds + row * HD + c4 * 4) = v;
    }
}

// grid (ceil(T/64), heads, N), one wave; lane = one query
template <int HD, int HS>
__global__ __launch_bounds__(64) void mha_fwd_f32_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                         float* __restrict__ lse, int T, int C, int heads, float scale) {
    __shared__ __attribute__((aligned(16))) float Ks[BT * HD];
    __shared__ __attribute__((aligned(16))) float Vs[BT * HD];
    __shared__ float Ss[BT * 64];
    const int lane = threadIdx.x;
    const int h = blockIdx.y, n = blockIdx.z;
    const int t = blockIdx.x * 64 + lane;
    const bool live = t < T;
    const long long ld = 3LL * C;
    const float* base = qkv + (long long)n * T * ld + h * HS;
    float q[HD], o[HD];
#pragma unroll
    for (int d = 0; d < HD; d += 4) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live) v = *reinterpret_cast<const float4*>(base + (long long)t * ld + d);
        q[d] = v.x * scale; q[d + 1] = v.y * scale; q[d + 2] = v.z * scale; q[d + 3] = v.w * scale;
        o[d] = o[d + 1] = o[d + 2] = o[d + 3] = 0.f;
    }
    float m = -INFINITY, l = 0.f;
    for (int k0 = 0; k0 < T; k0 += BT) {
        __syncthreads();
        stage_block<HD>(base + C, ld, k0, T, Ks, lane);
        stage_block<HD>(base + 2 * C, ld, k0, T, Vs, lane);
        __syncthreads();
        const int nk = min(BT, T - k0);
        float bm = -INFINITY;
        for (int j = 0; j < nk; ++j) {          // scores of this block -> LDS (lane-contiguous, conflict-free)
            float a = 0.f;
#pragma unroll
            for (int d = 0; d < HD; d += 4) {
                const float4 kv = *reinterpret_cast<const float4*>(Ks + j * HD + d);
                a = fmaf(q[d], kv.x, a); a = fmaf(q[d + 1], kv.y, a); a = fmaf(q[d + 2], kv.z, a); a = fmaf(q[d + 3], kv.w, a);
            }
            Ss[j * 64 + lane] = a;
            bm = fmaxf(bm, a);
        }
        const float mn = fmaxf(m, bm);
        const float corr = expf(m - mn);      // exp(-inf) = 0 on the first block
        l *= corr;
#pragma unroll
        for (int d = 0; d < HD; ++d) o[d] *= corr;
        for (int j = 0; j < nk; ++j) {
            const float p = expf(Ss[j * 64 + lane] - mn);
            l += p;
#pragma unroll
            for (int d = 0; d < HD; d += 4) {
                const float4 vv = *reinterpret_cast<const float4*>(Vs + j * HD + d);
                o[d] = fmaf(p, vv.x, o[d]); o[d + 1] = fmaf(p, vv.y, o[d + 1]);
                o[d + 2] = fmaf(p, vv.z, o[d + 2]); o[d + 3] = fmaf(p, vv.w, o[d + 3]);
            }
        }
        m = mn;
    }
    if (!live) return;
    const float inv = 1.f / l;
    float* op = out + ((long long)n * T + t) * C + h * HS;
#pragma unroll
    for (int d = 0; d < HD; d += 4)
        *reinterpret_cast<float4*>(op + d) = make_float4(o[d] * inv, o[d + 1] * inv, o[d + 2] * inv, o[d + 3] * inv);
#pragma unroll
    for (int d = HD; d < HS; d += 4) *reinterpret_cast<float4*>(op + d) = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lse) lse[((long long)n * heads + h) * T + t] = m + logf(l);
}

// dQ: lane = one query; recomputes P from the saved log-sum-exp.  D = rowsum(dO o O).
template <int HD, int HS>
__global__ __launch_bounds__(64) void mha_bwd_dq_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ o,
                                                            const float* __restrict__ dout, const float* __restrict__ lse,
                                                            float* __restrict__ dqkv, int T, int C, int heads, float scale) {
    __shared__ __attribute__((aligned(16))) float Ks[BT * HD];
    __shared__ __attribute__((aligned(16))) float Vs[BT * HD];
    const int lane = threadIdx.x;
    const int h = blockIdx.y, n = blockIdx.z;
    const int t = blockIdx.x * 64 + lane;
    const bool live = t < T;
    const long long ld = 3LL * C;
    const float* base = qkv + (long long)n * T * ld + h * HS;
    float q[HD], dO[HD], dq[HD];
    float D = 0.f;
#pragma unroll
    for (int d = 0; d < HD; d += 4) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f), g = v, ov = v;
        if (live) {
            v = *reinterpret_cast<const float4*>(base + (long long)t * ld + d);
            g = *reinterpret_cast<const float4*>(dout + ((long long)n * T + t) * C + h * HS + d);
            ov = *reinterpret_cast<const float4*>(o + ((long long)n * T + t) * C + h * HS + d);
        }
        q[d] = v.x * scale; q[d + 1] = v.y * scale; q[d + 2] = v.z * scale; q[d + 3] = v.w * scale;
        dO[d] = g.x; dO[d + 1] = g.y; dO[d + 2] = g.z; dO[d + 3] = g.w;
        D = fmaf(g.x, ov.x, D); D = fmaf(g.y, ov.y, D); D = fmaf(g.z, ov.z, D); D = fmaf(g.w, ov.w, D);
        dq[d] = dq[d + 1] = dq[d + 2] = dq[d + 3] = 0.f;
    }
    const float L = live ? lse[((long long)n * heads + h) * T + t] : 0.f;
    for (int k0 = 0; k0 < T; k0 += BT) {
        __syncthreads();
        stage_block<HD>(base + C, ld, k0, T, Ks, lane);
        stage_block<HD>(base + 2 * C, ld, k0, T, Vs, lane);
        __syncthreads();
        const int nk = min(BT, T - k0);
        for (int j = 0; j < nk; ++j) {
            float a = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < HD; d += 4) {
                const float4 kv = *reinterpret_cast<const float4*>(Ks + j * HD + d);
                const float4 vv = *reinterpret_cast<const float4*>(Vs + j * HD + d);
                a = fmaf(q[d], kv.x, a); a = fmaf(q[d + 1], kv.y, a); a = fmaf(q[d + 2], kv.z, a); a = fmaf(q[d + 3], kv.w, a);
                dp = fmaf(dO[d], vv.x, dp); dp = fmaf(dO[d + 1], vv.y, dp); dp = fmaf(dO[d + 2], vv.z, dp); dp = fmaf(dO[d + 3], vv.w, dp);
            }
            const float p = expf(a - L);
            const float ds = p * (dp - D);
#pragma unroll
            for (int d = 0; d < HD; d += 4) {
                const float4 kv = *reinterpret_cast<const float4*>(Ks + j * HD + d);
                dq[d] = fmaf(ds, kv.x, dq[d]); dq[d + 1] = fmaf(ds, kv.y, dq[d + 1]);
                dq[d + 2] = fmaf(ds, kv.z, dq[d + 2]); dq[d + 3] = fmaf(ds, kv.w, dq[d + 3]);
            }
        }
    }
    if (!live) return;
    float* dst = dqkv + ((long long)n * T + t) * ld + h * HS;
#pragma unroll
    for (int d = 0; d < HD; d += 4)
        *reinterpret_cast<float4*>(dst + d) = make_float4(dq[d] * scale, dq[d + 1] * scale, dq[d + 2] * scale, dq[d + 3] * scale);
#pragma unroll
    for (int d = HD; d < HS; d += 4) *reinterpret_cast<float4*>(dst + d) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// dK, dV: lane = one key; the queries (scaled), their dO, log-sum-exp and D are broadcast from LDS in 64-token blocks
template <int HD, int HS>
__global__ __launch_bounds__(64) void mha_bwd_dkv_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ o,
                                                             const float* __restrict__ dout, const float* __restrict__ lse,
                                                             float* __restrict__ dqkv, int T, int C, int heads, float scale) {
    __shared__ __attribute__((aligned(16))) float Qs[BT * HD];
    __shared__ __attribute__((aligned(16))) float Gs[BT * HD];
    __shared__ float Ls[BT], Ds[BT];
    const int lane = threadIdx.x;
    const int h = blockIdx.y, n = blockIdx.z;
    const int t = blockIdx.x * 64 + lane;
    const bool live = t < T;
    const long long ld = 3LL * C;
    const float* base = qkv + (long long)n * T * ld + h * HS;
    const float* obase = o + (long long)n * T * C + h * HS;
    const float* gbase = dout + (long long)n * T * C + h * HS;
    float k[HD], v[HD], dk[HD], dv[HD];
#pragma unroll
    for (int d = 0; d < HD; d += 4) {
        float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
        if (live) {
            kv = *reinterpret_cast<const float4*>(base + C + (long long)t * ld + d);
            vv = *reinterpret_cast<const float4*>(base + 2 * C + (long long)t * ld + d);
        }
        k[d] = kv.x; k[d + 1] = kv.y; k[d + 2] = kv.z; k[d + 3] = kv.w;
        v[d] = vv.x; v[d + 1] = vv.y; v[d + 2] = vv.z; v[d + 3] = vv.w;
        dk[d] = dk[d + 1] = dk[d + 2] = dk[d + 3] = 0.f;
        dv[d] = dv[d + 1] = dv[d + 2] = dv[d + 3] = 0.f;
    }
    for (int q0 = 0; q0 < T; q0 += BT) {
        __syncthreads();
        stage_block<HD>(base, ld, q0, T, Qs, lane);
        stage_block<HD>(gbase, C, q0, T, Gs, lane);
        {
            const int qi = q0 + lane;
            float D = 0.f, L = 0.f;
            if (qi < T) {
#pragma unroll
                for (int d = 0; d < HD; d += 4) {
                    const float4 g = *reinterpret_cast<const float4*>(gbase + (long long)qi * C + d);
                    const float4 ov = *reinterpret_cast<const float4*>(obase + (long long)qi * C + d);
                    D = fmaf(g.x, ov.x, D); D = fmaf(g.y, ov.y, D); D = fmaf(g.z, ov.z, D); D = fmaf(g.w, ov.w, D);
                }
                L = lse[((long long)n * heads + h) * T + qi];
            }
            Ds[lane] = D; Ls[lane] = L;
        }
        __syncthreads();
        const int nq = min(BT, T - q0);
        for (int i = 0; i < nq; ++i) {
            float a = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < HD; d += 4) {
                const float4 qv = *reinterpret_cast<const float4*>(Qs + i * HD + d);
                const float4 g = *reinterpret_cast<const float4*>(Gs + i * HD + d);
                a = fmaf(qv.x * scale, k[d], a); a = fmaf(qv.y * scale, k[d + 1], a);
                a = fmaf(qv.z * scale, k[d + 2], a); a = fmaf(qv.w * scale, k[d + 3], a);
                dp = fmaf(g.x, v[d], dp); dp = fmaf(g.y, v[d + 1], dp); dp = fmaf(g.z, v[d + 2], dp); dp = fmaf(g.w, v[d + 3], dp);
            }
            const float p = expf(a - Ls[i]);
            const float ds = p * (dp - Ds[i]);
#pragma unroll
            for (int d = 0; d < HD; d += 4) {
                const float4 qv = *reinterpret_cast<const float4*>(Qs + i * HD + d);
                const float4 g = *reinterpret_cast<const float4*>(Gs + i * HD + d);
                dv[d] = fmaf(p, g.x, dv[d]); dv[d + 1] = fmaf(p, g.y, dv[d + 1]);
                dv[d + 2] = fmaf(p, g.z, dv[d + 2]); dv[d + 3] = fmaf(p, g.w, dv[d + 3]);
                dk[d] = fmaf(ds, qv.x * scale, dk[d]); dk[d + 1] = fmaf(ds, qv.y * scale, dk[d + 1]);
                dk[d + 2] = fmaf(ds, qv.z * scale, dk[d + 2]); dk[d + 3] = fmaf(ds, qv.w * scale, dk[d + 3]);
            }
        }
    }
    if (!live) return;
    float* dst = dqkv + ((long long)n * T + t) * ld + h * HS;
#pragma unroll
    for (int d = 0; d < HD; d += 4) {
        *reinterpret_cast<float4*>(dst + C + d) = make_float4(dk[d], dk[d + 1], dk[d + 2], dk[d + 3]);
        *reinterpret_cast<float4*>(dst + 2 * C + d) = make_float4(dv[d], dv[d + 1], dv[d + 2], dv[d + 3]);
    }
#pragma unroll
    for (int d = HD; d < HS; d += 4) {
        *reinterpret_cast<float4*>(dst + C + d) = make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(dst + 2 * C + d) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// one launcher per direction: the tile grid, one wave per workgroup, any T
template <int HD, int HS>
int mha_fwd_f32(const MhaDesc& d, const float* qkv, float* out, float* lse, hipStream_t s) {
    hipLaunchKernelGGL((mha_fwd_f32_kernel<HD, HS>), dim3(ceil_div(d.T, 64), d.heads, d.N), dim3(64), 0, s, qkv, out, lse, d.T, d.C, d.heads,
                       prx_mha_scale(HD));
    PRX_LAUNCH_CHECK();
    return 0;
}
template <int HD, int HS>
int mha_bwd_f32(const MhaDesc& d, const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, hipStream_t s) {
    const dim3 grid(ceil_div(d.T, 64), d.heads, d.N);
    const float scale = prx_mha_scale(HD);
    hipLaunchKernelGGL((mha_bwd_dq_f32_kernel<HD, HS>), grid, dim3(64), 0, s, qkv, out, dout, lse, dqkv, d.T, d.C, d.heads, scale);
    PRX_LAUNCH_CHECK();
    hipLaunchKernelGGL((mha_bwd_dkv_f32_kernel<HD, HS>), grid, dim3(64), 0, s, qkv, out, dout, lse, dqkv, d.T, d.C, d.heads, scale);
    PRX_LAUNCH_CHECK();
    return 0;
}

// head dim -> instance <HD, HS = prx_mha_head_cols(HD)>, for both directions: `launch` is called with the instance as its argument
template <int HD_, int HS_>
struct Inst { static constexpr int HD = HD_, HS = HS_; };
template <typename Launch>
int mha_f32_instance(int hd, Launch launch) {
    switch (hd) {
        case 64: return launch(Inst<64, 64>{});
        case 80: return launch(Inst<80, 96>{});
        case 88: return launch(Inst<88, 96>{});
        case 104: return launch(Inst<104, 128>{});
    }
    PRX_REQUIRE(false, "mha(f32): no instance for head dim %d (64 | 80 | 88 | 104)", hd);
}

}  // namespace

int prx_mha_f32_fwd(const MhaDesc& d, const float* qkv, float* out, float* lse, hipStream_t s) {
    return mha_f32_instance(d.hd, [&](auto i) { return mha_fwd_f32<decltype(i)::HD, decltype(i)::HS>(d, qkv, out, lse, s); });
}
int prx_mha_f32_bwd(const MhaDesc& d, const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, hipStream_t s) {
    return mha_f32_instance(d.hd, [&](auto i) { return mha_bwd_f32<decltype(i)::HD, decltype(i)::HS>(d, qkv, out, dout, lse, dqkv, s); });
}
