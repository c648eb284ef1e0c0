#pragma once
#include "common.h"
#include <math.h>
// Multi-head self-attention, softmax(q k^T / sqrt(head dim)) v per (image, head): one description of the problem, one place that
// decides which kernel family takes it and refuses what has none (attention.hip).  Callers only describe.
// Operands: qkv [N*T, 3C] (q | k | v, head h at columns h * cols..), out / dout [N*T, C], dqkv like qkv, lse fp32 [N*heads*T];
// bf16, IEEE half or fp32 by `prec`.  cols = prx_mha_head_cols(hd) >= hd; the cols - hd pad columns of a head are zeros in qkv and
// come out as exact zeros in out / dqkv.
struct MhaDesc {
    int N = 0, T = 0, heads = 0;
    int hd = 64;                 // head dim as the operands carry it: 64 (also the 16- and 32-wide heads a runner folds into 64 columns), 80, 88, 104
    int C = 0;                   // columns of out: must be heads * prx_mha_head_cols(hd)
    int prec = PRX_PREC_BF16;    // PRX_PREC_*
    int causal = 0;              // causal mask (CLIP text transformer): forward only, 16-bit, head dim 64; takes no lse, `recompute` is not read
    int recompute = 0;           // 0: the caller keeps out + lse for the backward (any T).  1: the recomputing form, which takes no lse and
                                 // whose backward does not read out: the wave-per-head kernels, where prx_mha_can_recompute holds
};
// operand columns per head for a head dim of the weights: {16, 32, 64} -> 64, {80, 88} -> 96, 104 -> 128, else 0 (no kernel)
int prx_mha_head_cols(int hd);
// the recomputing form has a kernel for this problem (16-bit operands, head dim 64, T <= 64, not causal): what a runner that can
// work either way sets `recompute` from
bool prx_mha_can_recompute(const MhaDesc& d);
// the caller must allocate out + lse per layer and hand the same buffers to the backward
inline bool prx_mha_saves_out(const MhaDesc& d) { return !d.causal && !d.recompute; }
// the softmax scale of every family
inline float prx_mha_scale(int hd) { return 1.f / sqrtf((float)hd); }

// `lse` is null where !prx_mha_saves_out(d); the backward then reads neither `out` nor `lse`
int prx_mha_fwd(const MhaDesc& d, const void* qkv, void* out, float* lse, hipStream_t s);
int prx_mha_bwd(const MhaDesc& d, const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, hipStream_t s);
