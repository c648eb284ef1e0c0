#pragma once
#include "common.h"
// 16-bit operand buffers (`bf16_t*`): bf16, or IEEE half when h16 != 0
// qkv: bf16 [N*T, 3C] (q | k | v, head h at columns h*64..), out/dout: bf16 [N*T, C]
int prx_mha_fwd(const bf16_t* qkv, bf16_t* out, int N, int T, int C, int heads, hipStream_t s, int h16 = 0);
int prx_mha_bwd(const bf16_t* qkv, const bf16_t* dout, bf16_t* dqkv, int N, int T, int C, int heads, hipStream_t s, int h16 = 0);
// any sequence length (64-token tiles, online softmax); out must be kept for the backward, lse: fp32 [N*heads*T]
int prx_mha_fwd_gen(const bf16_t* qkv, bf16_t* out, float* lse, int N, int T, int C, int heads, hipStream_t s, int h16 = 0);
int prx_mha_bwd_gen(const bf16_t* qkv, const bf16_t* out, const bf16_t* dout, const float* lse, bf16_t* dqkv, int N, int T,
                    int C, int heads, hipStream_t s, int h16 = 0);
// forward only, causal mask (CLIP text transformer, context 77)
int prx_mha_fwd_causal(const bf16_t* qkv, bf16_t* out, int N, int T, int C, int heads, hipStream_t s, int h16 = 0);
// exact-f32 attention of the PRX_PREC_F32 parity mode (attention_f32.hip): any T, fp32 operands; `out` and `lse`
// ([N*heads*T]) are kept for the backward
int prx_mha_fwd_f32(const float* qkv, float* out, float* lse, int N, int T, int C, int heads, hipStream_t s);
int prx_mha_bwd_f32(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, int N, int T, int C,
                    int heads, hipStream_t s);
// heads of 96 operand columns = head dim 80 zero-padded (the 96-wide instances of attention_kernels.h; OpenCLIP ViT-H/14): qkv [N*T, 3C] with head h at columns
// h*96.., C == heads * 96, 1 <= T <= 640, `scale` the softmax scale (1 / sqrt(80)); pad columns of out / dqkv come out as exact zeros
int prx_mha_fwd_hd96(const bf16_t* qkv, bf16_t* out, float* lse, int N, int T, int C, int heads, float scale, hipStream_t s, int h16 = 0);
int prx_mha_bwd_hd96(const bf16_t* qkv, const bf16_t* out, const bf16_t* dout, const float* lse, bf16_t* dqkv, int N, int T, int C,
                     int heads, float scale, hipStream_t s, int h16 = 0);
// ... and their exact-f32 form (attention_f32.hip instantiated for head dim 80 at column stride 96, scale 1 / sqrt(80); any T)
int prx_mha_fwd_f32_hd96(const float* qkv, float* out, float* lse, int N, int T, int C, int heads, hipStream_t s);
int prx_mha_bwd_f32_hd96(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, int N, int T, int C,
                         int heads, hipStream_t s);
// heads of 128 operand columns = head dim 104 zero-padded (OpenCLIP ViT-bigG-14): the 128-wide instances of the same family, same contract
// (heads of 88, ViT-g-14, run on prx_mha_*_hd96 with scale 1 / sqrt(88))
int prx_mha_fwd_hd128(const bf16_t* qkv, bf16_t* out, float* lse, int N, int T, int C, int heads, float scale, hipStream_t s, int h16 = 0);
int prx_mha_bwd_hd128(const bf16_t* qkv, const bf16_t* out, const bf16_t* dout, const float* lse, bf16_t* dqkv, int N, int T, int C,
                      int heads, float scale, hipStream_t s, int h16 = 0);
// exact-f32 form for any padded head dim hd: 80 | 88 in 96 columns, 104 in 128; scale 1 / sqrt(hd); any T
int prx_mha_fwd_f32_pad(const float* qkv, float* out, float* lse, int N, int T, int C, int heads, int hd, hipStream_t s);
int prx_mha_bwd_f32_pad(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, int N, int T, int C,
                        int heads, int hd, hipStream_t s);
