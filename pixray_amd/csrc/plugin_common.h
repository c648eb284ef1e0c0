// Shared pieces of the built-in plugin kernels (plugin_losses.hip, plugin_filters.hip): a grid-stride launch shape and the
// deterministic "partials, then the last workgroup adds up" reduction of prompt_vq.hip's prompt_loss_kernel.
#pragma once
#include "common.h"

constexpr int PLUG_THREADS = 256;
constexpr int PLUG_MAX_BLOCKS = 1024;   // capacity of the caller's partials buffer, in rows of PLUG_K doubles
constexpr int PLUG_K = 4;               // values reduced per launch (at most)

static inline int plug_blocks(long long items) {
    long long b = (items + PLUG_THREADS - 1) / PLUG_THREADS;
    return (int)(b < 1 ? 1 : (b > PLUG_MAX_BLOCKS ? PLUG_MAX_BLOCKS : b));
}

// Every thread hands in its K running sums.  Workgroup sums go to partials[blockIdx.x][k]; the workgroup that draws the last
// ticket (atomicInc wraps the word back to zero) adds the rows in block order.  Returns true on thread 0 of that workgroup only,
// with the grid totals in v.  The order of every addition is fixed by the launch shape, so a run repeats bit for bit.
template <int K>
__device__ __forceinline__ bool plug_reduce(double (&v)[K], double* __restrict__ partials, unsigned* __restrict__ ticket) {
    __shared__ double red[PLUG_THREADS / 64][PLUG_K];
    __shared__ unsigned last;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double t = wave_sum_d(v[k]);
        if (lane == 0) red[wid][k] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double t = 0.0;
            for (int w = 0; w < PLUG_THREADS / 64; ++w) t += red[w][k];
            partials[(size_t)blockIdx.x * PLUG_K + k] = t;
        }
    }
    __threadfence();                       // this workgroup's row is visible device-wide before its ticket is drawn
    __syncthreads();
    if (threadIdx.x == 0) last = atomicInc(ticket, gridDim.x - 1) == gridDim.x - 1 ? 1u : 0u;
    __syncthreads();
    if (!last || threadIdx.x >= 64) return false;
    __threadfence();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double t = 0.0;
        for (int r = lane; r < (int)gridDim.x; r += 64)          // rows written by other workgroups: read past this CU's L1
            t += *reinterpret_cast<const volatile double*>(partials + (size_t)r * PLUG_K + k);
        v[k] = wave_sum_d(t);
    }
    return lane == 0;
}
