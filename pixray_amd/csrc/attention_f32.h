#pragma once
#include "attention.h"
// The exact-f32 family (attention_f32.hip) as the dispatcher of attention.hip reaches it: prx_mha_fwd / prx_mha_bwd have checked the
// descriptor (a head dim with an instance at its column count, fp32 operands, saving form); nothing else calls these.
int prx_mha_f32_fwd(const MhaDesc& d, const float* qkv, float* out, float* lse, hipStream_t s);
int prx_mha_f32_bwd(const MhaDesc& d, const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, hipStream_t s);
