// Phase timing of the T<=64 attention forward/backward (one wave per head): instrumented copies of the kernels with
// s_memtime stamps, plus end-to-end timing of the real kernels.  Build:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I pixray_amd/csrc tools/micro/mha_phase.hip pixray_amd/csrc/attention_f32.hip -o mha_phase
#include "../../pixray_amd/csrc/attention.hip"
#include <cstdio>
#include <cstdarg>
#include <vector>
void prx_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc(10, stderr); }
int prx_xcd_local() { return 1; }
using F = FmtBf16;

// softmax over j in the C layout (one wave holds all 64 keys of a row: 32-lane butterflies); s holds raw q.k sums; returns p in s
__device__ __forceinline__ void softmax_c_layout(f32x16 (&s)[2][2], float scale, int T, int lane) {
    const int j0 = lane & 31;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v0 = (j0 < T) ? s[mi][0][r] * scale : -INFINITY;
            float v1 = (j0 + 32 < T) ? s[mi][1][r] * scale : -INFINITY;
            float mx = half_max(fmaxf(v0, v1));
            float e0 = __expf(v0 - mx), e1 = __expf(v1 - mx);
            float sum = half_sum(e0 + e1);
            float inv = 1.f / sum;
            s[mi][0][r] = e0 * inv;
            s[mi][1][r] = e1 * inv;
        }
}

__global__ __launch_bounds__(64) void fwd_timed(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, int T, int C, float scale,
                                                long long* __restrict__ stamps) {
    __shared__ __attribute__((aligned(16))) bf16_t smem[4 * TILE];
    bf16_t* Qs = smem; bf16_t* Ks = smem + TILE; bf16_t* Vt = smem + 2 * TILE; bf16_t* Ps = smem + 3 * TILE;
    const int lane = threadIdx.x;
    const int h = blockIdx.x, n = blockIdx.y;
    const long long ld = 3LL * C;
    const bf16_t* base = qkv + (long long)n * T * ld + h * 64;
    long long t[8]; int k = 0;
    t[k++] = __builtin_amdgcn_s_memtime();
    load_rows<F>(base, ld, 0, T, Qs, nullptr, lane);
    load_rows<F>(base + C, ld, 0, T, Ks, nullptr, lane);
    t[k++] = __builtin_amdgcn_s_memtime();
    load_rows<F>(base + 2 * C, ld, 0, T, nullptr, Vt, lane);
    __syncthreads();
    t[k++] = __builtin_amdgcn_s_memtime();
    f32x16 s[2][2];
    zero_acc(s);
    mma_64x64x64<F>(Qs, Ks, s, lane);
    t[k++] = __builtin_amdgcn_s_memtime();
    softmax_c_layout(s, scale, T, lane);
    t[k++] = __builtin_amdgcn_s_memtime();
    store_c_tile<F>(s, Ps, nullptr, lane);
    __syncthreads();
    t[k++] = __builtin_amdgcn_s_memtime();
    f32x16 o[2][2];
    zero_acc(o);
    mma_64x64x64<F>(Ps, Vt, o, lane);
    t[k++] = __builtin_amdgcn_s_memtime();
    store_c_global<F>(o, out + (long long)n * T * C + h * 64, C, T, lane);
    t[k++] = __builtin_amdgcn_s_memtime();
    if (lane == 0 && h == 3 && n == 5) for (int i = 0; i < 8; ++i) stamps[i] = t[i];
}

int main() {
    const int N = 64, T = 50, C = 768, heads = 12;
    size_t nq = (size_t)N * T * 3 * C;
    std::vector<bf16_t> hq(nq);
    for (size_t i = 0; i < nq; ++i) hq[i] = (bf16_t)(((int)(i * 2654435761u % 2001) - 1000) / 1000.f);
    bf16_t *qkv, *out, *dout, *dqkv; long long* st;
    hipMalloc(&qkv, nq * 2); hipMalloc(&out, nq * 2 / 3); hipMalloc(&dout, nq * 2 / 3); hipMalloc(&dqkv, nq * 2); hipMalloc(&st, 64);
    hipMemcpy(qkv, hq.data(), nq * 2, hipMemcpyHostToDevice);
    hipMemcpy(dout, hq.data(), nq * 2 / 3, hipMemcpyHostToDevice);
    for (int rep = 0; rep < 3; ++rep) {
        hipLaunchKernelGGL(fwd_timed, dim3(heads, N), dim3(64), 0, 0, qkv, out, T, C, 0.125f, st);
        hipDeviceSynchronize();
        long long h[8]; hipMemcpy(h, st, 64, hipMemcpyDeviceToHost);
        const char* names[7] = {"load Q,K", "load V (transposed LDS image)", "S = QK^T", "softmax", "P -> LDS", "O = PV", "store O"};
        printf("rep %d (s_memtime ticks, 100 MHz => x10 ns):", rep);
        for (int i = 0; i < 7; ++i) printf("  %s %lld", names[i], h[i + 1] - h[i]);
        printf("  total %lld\n", h[7] - h[0]);
    }
    MhaDesc d;      // the recomputing form: the wave-per-head kernels
    d.N = N; d.T = T; d.heads = heads; d.C = C; d.recompute = 1;
    hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
    for (int which = 0; which < 2; ++which) {
        for (int i = 0; i < 3; ++i) { if (which == 0) prx_mha_fwd(d, qkv, out, nullptr, 0); else prx_mha_bwd(d, qkv, nullptr, dout, nullptr, dqkv, 0); }
        hipEventRecord(a, 0);
        for (int i = 0; i < 200; ++i) { if (which == 0) prx_mha_fwd(d, qkv, out, nullptr, 0); else prx_mha_bwd(d, qkv, nullptr, dout, nullptr, dqkv, 0); }
        hipEventRecord(b, 0); hipEventSynchronize(b);
        float ms; hipEventElapsedTime(&ms, a, b);
        printf("%s: %.2f us per launch (back-to-back)\n", which == 0 ? "mha_fwd" : "mha_bwd", ms * 1e3f / 200);
    }
    return 0;
}
