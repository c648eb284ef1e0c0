// RRDBNet x4 (the network of pixray's super_resolution drawer, super_resolution.py:34-102: RealESRGAN_x4plus) on its own
// HIP kernels: rrdbnet.hip.  Self-contained: nothing here goes through the shared GEMM engine.
//
// Layout.  Activations are NHWC.  Every residual dense block (RDB) owns one concat buffer [h*w, 192] in the operand type T
// (IEEE half, or fp32 in the exact mode): channels [0, 64) are the block's input x, convolution k = 1..4 reads the prefix
// [0, 64 + 32 (k - 1)) at pixel stride 192 and writes its 32 LeakyReLU'd outputs into [64 + 32 (k - 1), 64 + 32 k); conv5
// reads all 192 and writes the NEXT block's first 64 channels with 0.2 v + x fused (and the RRDB-level 0.2 y + x0 as a second
// residual in every third block).  All 3 num_block buffers are kept for the backward: LeakyReLU preserves the sign, so the
// stored post-activation is its own derivative mask (a > 0: 1, else 0.2 -- zero takes the 0.2 side, as torch does).
//
// The trunk (the residual stream x) is ALSO kept in fp32 in a ring of four [h*w, 64] buffers, and the backward accumulates
// in a ring of four fp32 gradient concat buffers [h*w, 192]: in the half mode only MFMA operands are 16-bit (the stored
// activations, the weight packs and a gradient at the moment it enters a dgrad), never a running sum.
//
// Device memory of a handle, h x w the latent (a quarter of the canvas), e = sizeof(T), nb = num_block:
//     concat buffers       3 nb * h w * 192 * e          (23 blocks, 512^2 canvas: 69 * 16384 * 192 * 2 B = 434 MB; 868 MB in f32)
//     trunk ring + feat    5 * h w * 64 * 4
//     gradient ring        4 * h w * 192 * 4
//     tail activations     h w * 64 * e * (2 + 4 + 16 + 16)  (trunk out, body, up1, up2, hr)
//     tail gradients       16 h w * 64 * 4 * 2 + 4 h w * 64 * 4 + h w * 64 * 4,   raw image 48 h w * 4
//     weight packs         forward + flipped-transposed dgrad pack of every convolution: 2 * 16.7 M * e at 23 blocks
// Everything is allocated by prx_rrdbnet_create and never afterwards; synth / backward only launch on the given stream.
#pragma once
#include "common.h"

// one convolution of the family (forward or data gradient) on caller-owned buffers; every pointer is a device pointer
struct RrdbConvArgs {
    const void* in;       // forward: T [pixels][ld_in]; dgrad: fp32 gradient [pixels][ld_in]
    int ld_in, in_off;    // the Kc input channels are in_off .. in_off + Kc
    const void* act;      // dgrad: T, the stored activation of the same channels (LeakyReLU derivative on load); null: none
    int ld_act, act_off;
    const void* w;        // T [N][9 Kc], K index = tap * Kc + channel
    const float* bias;    // [N] or null
    int Kc, N;            // input / output channels, multiples of 32
    int H, W;             // the convolution's output grid; up: the input is [H/2][W/2], read nearest-2x
    int up, lrelu;
    float alpha, beta;    // v = alpha * v + beta * r1 + r2 on the first `rn` output channels, alpha * v on the rest
    const float* r1; int ld_r1;
    const float* r2; int ld_r2;
    int rn;
    void* out; int ld_out, out_off;         // T [pixels][ld_out], or null
    float* out_f32; int ld_of, of_off;      // fp32 copy / accumulation target, or null
    int accum;                               // out_f32 += v instead of = v
};
int rrdb_conv_launch(const RrdbConvArgs& a, int dgrad, int f32, hipStream_t s);
