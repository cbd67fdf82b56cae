// AdamW element update shared by loss.hip (cnr_adamw_step) and render_loss.hip (cnr_adamw_epilogue).
// torch.optim.AdamW as configured at train.py:40,54-64: decoupled weight decay, bias corrections from the step count.
#pragma once
#include "cnr_common.h"

namespace cnr {
struct AdamArgs {
  float* p; const float* g; float* m; float* v; int64_t n;
  float lr, b1, b2, eps, wd, gunscale;
};
// step size and 1 / sqrt(bias correction 2) for optimiser step t (1-based)
__device__ __forceinline__ void adam_coefficients(const AdamArgs& a, int64_t t, float& step_size, float& inv_bc2_sqrt) {
  const double td = (double)t;
  step_size = (float)((double)a.lr / (1.0 - pow((double)a.b1, td)));
  inv_bc2_sqrt = (float)(1.0 / sqrt(1.0 - pow((double)a.b2, td)));
}
// one element's update, by value (loads and stores are the caller's): parameter p, moments m and v, gradient g;
// decay = 1 - lr * weight decay
struct AdamElement { float p, m, v; };
__device__ __forceinline__ AdamElement adam_element(float p, float m, float v, float g, float decay, float step_size,
                                                    float inv_bc2_sqrt, float b1, float b2, float eps) {
  float pi = p * decay;
  const float mi = m + (g - m) * (1.0f - b1);
  const float vi = v * b2 + (1.0f - b2) * g * g;
  const float denom = sqrtf(vi) * inv_bc2_sqrt + eps;
  pi -= step_size * (mi / denom);
  return {pi, mi, vi};
}
// grid-stride over the flat buffer: block `blk` of `nblk` 256-thread blocks
__device__ __forceinline__ void adam_update(const AdamArgs& a, float step_size, float inv_bc2_sqrt, int blk, int nblk) {
  for (int64_t i = (int64_t)blk * 256 + threadIdx.x; i < a.n; i += (int64_t)nblk * 256) {
    // (the gradient is read first: with p, m, v read ahead of it the compiler contracts the other product of v's sum into the
    //  multiply-add, and v differs in the last place)
    const float gi = a.g[i] * a.gunscale;
    const AdamElement e = adam_element(a.p[i], a.m[i], a.v[i], gi, 1.0f - a.lr * a.wd, step_size, inv_bc2_sqrt, a.b1, a.b2, a.eps);
    a.p[i] = e.p; a.m[i] = e.m; a.v[i] = e.v;
  }
}
}  // namespace cnr
