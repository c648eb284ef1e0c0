// CLIP_Base.encode_text runner (slip.py:68-70 -> openai/CLIP `CLIP.encode_text` [UPSTREAM clip/model.py]).  Forward only.
#pragma once
#include "common.h"

struct PrxClipText;
// gelu: the MLP activation is the exact (erf) GELU of the OpenCLIP towers instead of OpenAI's QuickGELU
int prx_clip_text_create_impl(PrxClipText** out, int vocab, int ctx, int width, int layers, int heads, int out_dim, int max_n,
                              const float* const* w, int n_w, hipStream_t s, int gelu = 0);
void prx_clip_text_destroy_impl(PrxClipText* t);
int prx_clip_text_encode_impl(PrxClipText* t, const int* tokens, int n, float* embeds, hipStream_t s);
// launchers of the runner's own kernels (the runner calls these; exported as prx_k_* for the kernel-level tests)
// x[i][j] = emb[tokens[i][j]] + pos[j]; eot[i] = first index of the largest token id of sequence i
int prx_text_embed(const int* tokens, const float* emb, const float* pos, float* x, int* eot, int n, int ctx, int W, int vocab,
                   hipStream_t s);
// out[i] = x[i][eot[i]]
int prx_gather_rows(const float* x, const int* eot, float* out, int n, int ctx, int W, hipStream_t s);
