// What every runner handle on the GEMM engine shares (host code): RunnerEngine -- the operand precision, the engine context, the
// device memory and the split-K workspace, with the one GEMM wrapper --, and ImageTower, the protocol of the three image towers
// behind prx_clip_vit / prx_clip_resnet / prx_clip_convnext (minmax / encode / backward_reduce / backward_finish / gemm_ctx /
// destroy; csrc/api_path.hip forwards to it).  A new tower derives from ImageTower, names itself, allocates e / de (and de16 where its
// next product reads a 16-bit operand) in its create, ends the create with alloc_tail(), and supplies forward / backward_a /
// backward_b, which open with begin_forward / backward_n and use head_fwd / head_bwd for the L2-normalised embedding.
#pragma once
#include "common.h"
#include "gemm.h"
#include "dev_arena.h"
#include "cutouts.h"
#include "prompt_vq.h"
#include "elementwise.h"

int prx_vit_gelu_f32(const float* t, float* io, size_t n, int bwd, hipStream_t s);   // vit.h: the exact mode's GELU pass

struct RunnerEngine {
    int prec = 0;             // PRX_PREC_*: element type of the handle's operand buffers (void*)
    int f32 = 0, h16 = 0;     // derived: operands are fp32 / the 16-bit operand format is IEEE half
    GemmCtx gctx;             // this handle's engine state (tile overrides, timing log)
    DevArena mem;             // every device buffer of the handle: freed with it
    float* ws = nullptr; size_t ws_bytes = 0;   // split-K scratch
    float* gs = nullptr;      // half mode: device {S, 1/S} = the power-of-two scale of the backward in flight (common.h) + the partial maxima; else null

    void set_precision(int precision) { prec = precision; f32 = prec_is_f32(precision); h16 = prec_is_h16(precision); }
    int alloc_ws() {
        ws_bytes = (size_t)64 << 20;
        DEV_ALLOC(mem, alloc, ws, ws_bytes / sizeof(float));
        return 0;
    }
    // the handle's operand format on a descriptor (on its own for prx_gemm_launch_group), and the launch
    void operands(GemmDesc& d) const {
        if (f32) { d.f32 = 1; d.a_is_f32 = 0; }
        d.h16 = h16;
    }
    int gemm(GemmDesc& d, hipStream_t s) {
        operands(d);
        return prx_gemm_launch(d, ws, ws_bytes, s, &gctx);
    }
    // Linear + activation with the pre-activation saved, and its backward.  A: [M, K] rows of stride lda; W / WT: the [N, K] pack;
    // pre, out: dense [M, N].  The fp32 kernels carry no erff (gemm_epi.h), so the exact mode runs PRX_ACT_GELU / PRX_ACT_MUL_DGELU as a
    // pass of its own over the saved pre-activation (the expressions of the fused epilogues; at 1/16 of the MFMA rate the pass is not
    // the cost); every other case is the epilogue form.
    // out = act(A W^T + b), pre = A W^T + b
    int linear_act(int act, const void* A, int lda, const void* W, const float* b, void* pre, void* out, int M, int N, int K, hipStream_t s) {
        GemmDesc d; d.A = A; d.lda = lda; d.B = W; d.ldb = K; d.M = M; d.N = N; d.K = K; d.bias_n = b; d.ldc_bf16 = N;
        const bool own_pass = f32 && act == PRX_ACT_GELU;
        if (own_pass) d.out_bf16 = pre;
        else { d.act = act; d.out_bf16 = out; d.out_bf16_pre = pre; }
        if (int r = gemm(d, s)) return r;
        return own_pass ? prx_vit_gelu_f32((const float*)pre, (float*)out, (size_t)M * N, 0, s) : 0;
    }
    // out = (A WT^T) * act'(pre)
    int linear_dact(int dact, const void* A, int lda, const void* WT, const void* pre, void* out, int M, int N, int K, hipStream_t s) {
        GemmDesc d; d.A = A; d.lda = lda; d.B = WT; d.ldb = K; d.M = M; d.N = N; d.K = K; d.out_bf16 = out; d.ldc_bf16 = N;
        const bool own_pass = f32 && dact == PRX_ACT_MUL_DGELU;
        if (!own_pass) { d.act = dact; d.aux = pre; d.ldaux = N; }
        if (int r = gemm(d, s)) return r;
        return own_pass ? prx_vit_gelu_f32((const float*)pre, (float*)out, (size_t)M * N, 1, s) : 0;
    }
};

struct ImageTower : RunnerEngine {
    const char* name = "";    // the word the handle's messages begin with
    int res = 0, out_dim = 0, max_n = 0;
    int cur_n = 0;            // cutouts of the forward whose activations the handle holds; 0: none
    float *e = nullptr, *de = nullptr;   // [max_n, out_dim]: the embedding before its L2 normalisation, and its gradient
    void* de16 = nullptr;     // the half mode's scaled d(e) as a 16-bit operand, for towers whose next product reads one; else null
    float* mm_part = nullptr;

    virtual ~ImageTower() = default;
    virtual int forward(const float* cutouts, int n, const float* mm, float* embeds, hipStream_t s) = 0;
    // part A: from d(embeds) down to the input gradient and acc[4], the sums the batch-global min/max renorm needs (summed over ranks
    // by the caller when the cutout batch is sharded); part B applies them
    virtual int backward_a(const float* cutouts, const float* mm, const float* d_embeds, double* acc, hipStream_t s) = 0;
    virtual int backward_b(const float* cutouts, const float* mm, const double* acc, float* g_cutouts, hipStream_t s) = 0;

    int check_batch(int n) const {
        PRX_REQUIRE(n >= 1 && n <= max_n, "%s: batch %d exceeds handle capacity %d", name, n, max_n);
        return 0;
    }
    int begin_forward(int n) {
        if (int r = check_batch(n)) return r;
        cur_n = n;
        return 0;
    }
    int backward_n(int* n) const {
        PRX_REQUIRE(cur_n >= 1, "%s backward: no forward in flight on this handle", name);
        *n = cur_n;
        return 0;
    }
    int minmax(const float* cutouts, int n, float* mm, hipStream_t s) {
        if (int r = check_batch(n)) return r;
        return prx_minmax(cutouts, (size_t)n * 3 * res * res, mm_part, 1024, mm, s);
    }
    int head_fwd(float* embeds, int n, hipStream_t s) { return prx_l2norm_fwd(e, embeds, n, out_dim, s); }
    // d(embeds) -> de.  Half mode: everything below runs scaled by a power of two S chosen from max|d e| (exact: the backward is linear
    // in g).  S multiplies d e in fp32, BEFORE a GEMM's load converts it to half: entries of d e are ~1e-5 at the headline and shrink
    // with the prompt weight and the world size -- unscaled they would land in half's subnormals or flush to zero.  The runner
    // unscales (gs + 1 = 1/S) at its last product, before the (rank-summed) renormalisation sums.
    int head_bwd(const float* d_embeds, int n, hipStream_t s) {
        int r;
        if ((r = prx_l2norm_bwd(e, d_embeds, de, n, out_dim, s))) return r;
        if (!h16) return 0;
        if ((r = prx_grad_scale(de, (size_t)n * out_dim, gs + 2, 64, prx_grad_target_log2(), gs, s))) return r;
        return prx_scale_dev(de, (size_t)n * out_dim, gs, s, (bf16_t*)de16, de16 ? 1 : 0);
    }
    // the allocations every tower's create ends with
    int alloc_tail() {
        DEV_ALLOC(mem, alloc, mm_part, 2 * 1024);
        if (h16) DEV_ALLOC(mem, alloc, gs, 2 + 64);
        return alloc_ws();
    }
};
