// Weight packing (weight_pack.h): every runner's fp32 weights become GEMM operands here, once, while the handle is created.
#include "weight_pack.h"
#include "elementwise.h"
#include <algorithm>

namespace {

// Wf[co][tap*CiP + ci] = w[co][ci][ky][kx]            (forward pack; ci zero-padded to CiP)
// Wd[ci][tap*CoP + co] = w[co][ci][2-ky][2-kx]        (dgrad pack; ci zero-padded to CiP, co to CoP)
// a null pack is skipped
template <typename TOp>
__global__ __launch_bounds__(256) void pack_conv3x3_kernel(const float* __restrict__ w, TOp* __restrict__ Wf,
                                                           TOp* __restrict__ Wd, int Cout, int Cin, int CiP, int CoP) {
    const size_t total_f = Wf ? (size_t)Cout * 9 * CiP : 0;
    const size_t total_d = Wd ? (size_t)CiP * 9 * CoP : 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total_f + total_d;
         i += (size_t)gridDim.x * blockDim.x) {
        if (i < total_f) {
            const int ci = (int)(i % CiP), tap = (int)((i / CiP) % 9), co = (int)(i / ((size_t)9 * CiP));
            Wf[i] = op_cvt<TOp>(ci < Cin ? w[(((size_t)co * Cin + ci) * 3 + tap / 3) * 3 + tap % 3] : 0.f);
        } else {
            const size_t j = i - total_f;
            const int co = (int)(j % CoP), tap = (int)((j / CoP) % 9), ci = (int)(j / ((size_t)9 * CoP));
            Wd[j] = op_cvt<TOp>((ci < Cin && co < Cout) ? w[(((size_t)co * Cin + ci) * 3 + (2 - tap / 3)) * 3 + (2 - tap % 3)] : 0.f);
        }
    }
}

template <typename TOp>
__global__ __launch_bounds__(256) void pack_transpose_kernel(const float* __restrict__ in, TOp* __restrict__ out,
                                                             int R, int C) {
    // out[c][r] = TOp(in[r][c])
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int r = r0 + ty + 8 * i, c = c0 + tx;
        tile[ty + 8 * i][tx] = (r < R && c < C) ? in[(size_t)r * C + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int c = c0 + ty + 8 * i, r = r0 + tx;
        if (c < C && r < R) out[(size_t)c * R + r] = op_cvt<TOp>(tile[tx][ty + 8 * i]);
    }
}

}  // namespace

int prx_pack_conv3x3(const float* w, void* Wf, void* Wd, int Cout, int Cin, int CiP, int CoP, int prec, hipStream_t s) {
    PRX_REQUIRE(w && (Wf || Wd), "pack_conv3x3: null weights, or neither pack asked for");
    PRX_REQUIRE(Cout >= 1 && Cin >= 1 && CiP >= Cin && CoP >= Cout, "pack_conv3x3: %d x %d channels do not fit the padded %d x %d", Cout, Cin, CoP, CiP);
    PRX_REQUIRE(prec_valid(prec), "pack_conv3x3: unknown precision %d", prec);
    const size_t total = (Wf ? (size_t)Cout * 9 * CiP : 0) + (Wd ? (size_t)CiP * 9 * CoP : 0);
    const dim3 grid((unsigned)std::min<size_t>((total + 255) / 256, 1024));
    PRX_OP_DISPATCH(prec_is_f32(prec), prec_is_h16(prec), TO,
                    hipLaunchKernelGGL(pack_conv3x3_kernel<TO>, grid, dim3(256), 0, s, w, (TO*)Wf, (TO*)Wd, Cout, Cin, CiP, CoP));
    PRX_LAUNCH_CHECK();
    return 0;
}

int prx_pack_op(const float* in, void* out, size_t n, int prec, hipStream_t s) {
    if (!prec_is_f32(prec)) return prx_f32_to_bf16(in, (bf16_t*)out, n, s, prec_is_h16(prec));
    PRX_CHECK_HIP(hipMemcpyAsync(out, in, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}
int prx_pack_transpose_op(const float* in, void* out, int R, int C, int prec, hipStream_t s) {
    const dim3 grid(ceil_div(C, 32), ceil_div(R, 32));
    PRX_OP_DISPATCH(prec_is_f32(prec), prec_is_h16(prec), TO,
                    hipLaunchKernelGGL(pack_transpose_kernel<TO>, grid, dim3(256), 0, s, in, (TO*)out, R, C));
    PRX_LAUNCH_CHECK();
    return 0;
}
int prx_pack_bf16(const float* in, bf16_t* out, size_t n, hipStream_t s) { return prx_pack_op(in, out, n, 0, s); }
int prx_pack_transpose_bf16(const float* in, bf16_t* out, int R, int C, hipStream_t s) { return prx_pack_transpose_op(in, out, R, C, 0, s); }

int prx_pack_pair(DevArena& mem, void** W, void** WT, const float* src, int out, int in, int prec, hipStream_t s) {
    const size_t n = (size_t)out * in;
    DEV_ALLOC(mem, alloc_op, *W, n, prec_is_f32(prec));
    DEV_ALLOC(mem, alloc_op, *WT, n, prec_is_f32(prec));
    if (int r = prx_pack_op(src, *W, n, prec, s)) return r;
    return prx_pack_transpose_op(src, *WT, out, in, prec, s);
}

int prx_cat_qkv(DevArena& mem, float** wcat, float** bcat, WeightCursor& cur, int C, hipStream_t s) {
    const float *w[3], *b[3];
    for (int i = 0; i < 3; ++i) { NEXT_WEIGHT(cur, w[i]); NEXT_WEIGHT(cur, b[i]); }
    DEV_ALLOC(mem, alloc, *wcat, (size_t)3 * C * C); DEV_ALLOC(mem, alloc, *bcat, 3 * C);
    for (int i = 0; i < 3; ++i) {
        PRX_CHECK_HIP(hipMemcpyAsync(*wcat + (size_t)i * C * C, w[i], sizeof(float) * C * C, hipMemcpyDeviceToDevice, s));
        PRX_CHECK_HIP(hipMemcpyAsync(*bcat + i * C, b[i], sizeof(float) * C, hipMemcpyDeviceToDevice, s));
    }
    return 0;
}
