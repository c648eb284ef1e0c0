// How a runner turns the caller's fp32 weights into GEMM operands while it is created (host launchers; the kernels are in
// weight_pack.hip).  Nothing here runs in an iteration.
#pragma once
#include "common.h"
#include "dev_arena.h"

// The 3x3 convolution packs, operand precision `prec` (PRX_PREC_*), one launch for both:
//   Wf [Cout][9*CiP]:  Wf[co][tap*CiP + ci] = w[co][ci][ky][kx]        (tap = 3 ky + kx), zero for ci >= Cin
//   Wd [CiP][9*CoP]:   Wd[ci][tap*CoP + co] = w[co][ci][2-ky][2-kx]    (the flipped, transposed dgrad pack), zero for ci >= Cin or co >= Cout
// Either pointer may be null (that pack is not written), not both.  Exactly Cout forward rows are written: a runner whose forward
// product wants CoP rows zeroes the rest itself.
int prx_pack_conv3x3(const float* w, void* Wf, void* Wd, int Cout, int Cin, int CiP, int CoP, int prec, hipStream_t s);

// plain and transposed packs of a [R][C] matrix at operand precision `prec` (f32: plain copy / fp32 transpose)
int prx_pack_op(const float* in, void* out, size_t n, int prec, hipStream_t s);
int prx_pack_transpose_op(const float* in, void* out, int R, int C, int prec, hipStream_t s);
int prx_pack_bf16(const float* in, bf16_t* out, size_t n, hipStream_t s);
int prx_pack_transpose_bf16(const float* in, bf16_t* out, int R, int C, hipStream_t s);

// a frozen linear layer src [out][in] in both orientations (forward Bt = W, dgrad Bt = W^T): allocates W, then WT, then packs both
int prx_pack_pair(DevArena& mem, void** W, void** WT, const float* src, int out, int in, int prec, hipStream_t s);

// The caller's weight list, consumed in order.  `who` is the create's name: the messages begin with it.
struct WeightCursor {
    const float* const* w;
    int n, pos;
    const char* who;
    int done() const {
        PRX_REQUIRE(pos == n, "%s: %d weight tensors given, %d consumed", who, n, pos);
        return 0;
    }
};
// NEXT_WEIGHT(cur, dst): dst = the next tensor, or return the error from the enclosing function (as DEV_ALLOC does)
#define NEXT_WEIGHT(cur, dst) do { PRX_REQUIRE((cur).pos < (cur).n, "%s: weight list too short", (cur).who); (dst) = (cur).w[(cur).pos++]; } while (0)

// the q, k, v 1x1 convolutions of a VQGAN AttnBlock as one [3C, C] product: takes {weight, bias} of q, k, v from the cursor and
// allocates the fp32 concatenations wcat [3C][C], then bcat [3C]
int prx_cat_qkv(DevArena& mem, float** wcat, float** bcat, WeightCursor& cur, int C, hipStream_t s);
