#pragma once
#include "common.h"
// The update rules of `--optimiser` other than plain Adam (pixray.py:520-555), each fused with VqganDrawer.clip_z
// (vqgan.py:202-204).  p and its state tensors are fp32 with n elements; with bounds (zmin / zmax, both or neither) p is seen
// as [rows, C, hw] and element i is clamped to channel (i / hw) % C.  The step-dependent scalars come from the device buffer
// `hyper` (4 floats, see each rule), so a captured hipGraph replays with new scalars.
enum { PRX_OPT_ADAMW = 0, PRX_OPT_ADAGRAD = 1, PRX_OPT_ADAMAX = 2, PRX_OPT_DIFFGRAD = 3, PRX_OPT_RULES = 4 };
// s1 / s2 / s3, hyper per rule:
//   AdamW    exp_avg, exp_avg_sq, -          {lr / (1 - b1^t), sqrt(1 - b2^t), 1 - lr * weight_decay}
//   Adagrad  sum, -, -                       {lr}
//   Adamax   exp_avg, exp_inf, -             {lr / (1 - b1^t)}
//   DiffGrad exp_avg, exp_avg_sq, prev_grad  {lr * sqrt(1 - b2^t) / (1 - b1^t)}
int prx_optim_elementwise(int rule, float* p, float* s1, float* s2, float* s3, const float* g, const float* zmin,
                          const float* zmax, int C, int hw, size_t n, const float* hyper, double b1, double b2, float eps,
                          hipStream_t s);
// AdamP: two launches.  rows >= 1: the projection test runs on the [rows, n / rows] view and then on [1, n]; rows == 0: no
// projection (a 1-D tensor).  scratch: prx_adamp_scratch_floats(rows, n) floats.  hyper = {lr / (1 - b1^t), sqrt(1 - b2^t)}.
size_t prx_adamp_scratch_floats(int rows, size_t n);
int prx_optim_adamp(float* p, float* m, float* v, const float* g, const float* zmin, const float* zmax, int rows, int C, int hw,
                    size_t n, const float* hyper, float* scratch, size_t scratch_floats, double b1, double b2, float eps,
                    float delta, hipStream_t s);
