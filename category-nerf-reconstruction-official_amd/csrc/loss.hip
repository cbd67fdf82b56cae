// a14-a15: masks, L1 residuals, masked means and their gradient w.r.t. the rendered values in ONE
// launch and with no host synchronisation (src/loss.py:18-74, src/render_rays.py:52-95).  The
// reference syncs the host six times per step here ((mask_num == 0).any() and (loss > 1e5).any() in each
// of three reduce_batch_loss calls); this kernel keeps both checks on the device:
//   - "any class has an empty mask -> that loss term is zero, with no gradient, for ALL classes"
//     (render_rays.py:67-72) is evaluated by every block from the labels of all classes;
//   - "loss explode" (render_rays.py:87-89, exit(-1) there) is reported in flags[c] bit 0.
// One 256-thread block per class.
#include "adamw_common.h"
#include "render_common.h"

namespace {
using namespace cnr_rl;
__device__ __forceinline__ float block_sum(float v, float* sm /*[4]*/) {
  v = cnr::wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return sm[0] + sm[1] + sm[2] + sm[3];
}

__global__ __launch_bounds__(256) void loss_kernel(
    const float* __restrict__ depth, const float* __restrict__ var, const float* __restrict__ rgb,
    const float* __restrict__ opacity, const float* __restrict__ gt_depth, const float* __restrict__ gt_rgb,
    const uint8_t* __restrict__ labels, const uint8_t* __restrict__ depth_mask, float color_scaling,
    float opacity_scaling, float grad_scale, float* __restrict__ losses, int32_t* __restrict__ flags,
    float* __restrict__ d_depth, float* __restrict__ d_rgb, float* __restrict__ d_opacity, int C, int R) {
  __shared__ float sm[4];
  const int c = blockIdx.x;
  // ---- mask counts of every class (cheap: 2 bytes per ray) -----------------------------------
  bool empty_d = false, empty_c = false, empty_o = false;
  float nd = 0.f, nc = 0.f, no = 0.f;
  for (int cc = 0; cc < C; ++cc) {
    float a = 0.f, b = 0.f, d = 0.f;
    for (int r = threadIdx.x; r < R; r += 256) {
      const MaskBits m = mask_bits(labels[(size_t)cc * R + r], depth_mask[(size_t)cc * R + r] != 0);
      a += m.md ? 1.f : 0.f; b += m.mo ? 1.f : 0.f; d += m.ms ? 1.f : 0.f;
    }
    a = block_sum(a, sm); b = block_sum(b, sm); d = block_sum(d, sm);
    empty_d |= (a == 0.f); empty_c |= (b == 0.f); empty_o |= (d == 0.f);
    if (cc == c) { nd = a; nc = b; no = d; }
  }
  const MaskWeights mw = mask_weights(nd, nc, no, empty_d, empty_c, empty_o);
  // ---- per-ray residuals, gradients (render_common.h; the terms are accumulated here, in this file's contraction mode) ----
  float ld = 0.f, lc = 0.f, lo = 0.f;
  for (int r = threadIdx.x; r < R; r += 256) {
    const size_t i = (size_t)c * R + r;
    const Renders q{depth[i], var[i], opacity[i], rgb[i * 3 + 0], rgb[i * 3 + 1], rgb[i * 3 + 2]};
    const RayLoss l = ray_loss(q, gt_depth[i], gt_rgb[i * 3 + 0], gt_rgb[i * 3 + 1], gt_rgb[i * 3 + 2], labels[i],
                               depth_mask[i] != 0, mw.wd, mw.wc, mw.wo, color_scaling, opacity_scaling, grad_scale);
    ld += l.ad * l.info; lc += l.ac * l.fo; lo += l.ao * l.fs;
    d_depth[i] = l.dD;
    d_rgb[i * 3 + 0] = l.dR; d_rgb[i * 3 + 1] = l.dG; d_rgb[i * 3 + 2] = l.dBl;
    d_opacity[i] = l.dO;
  }
  ld = block_sum(ld, sm) * mw.wd; lc = block_sum(lc, sm) * mw.wc; lo = block_sum(lo, sm) * mw.wo;
  if (threadIdx.x == 0) {
    losses[0 * C + c] = ld; losses[1 * C + c] = lc; losses[2 * C + c] = lo;
    flags[c] = mask_flags(empty_d, empty_c, empty_o) | ((ld > 100000.f || lc > 100000.f || lo > 100000.f) ? 1 : 0);
  }
}

__global__ __launch_bounds__(256) void adamw_kernel(cnr::AdamArgs a, float step_size, float inv_bc2_sqrt,
                                                    const int64_t* __restrict__ d_state) {
  if (d_state) cnr::adam_coefficients(a, d_state[2] + 1, step_size, inv_bc2_sqrt);  // step number on the device
  cnr::adam_update(a, step_size, inv_bc2_sqrt, blockIdx.x, gridDim.x);
}
}  // namespace

extern "C" int cnr_loss_fwd_bwd(const float* depth, const float* var, const float* rgb, const float* opacity,
                                const float* gt_depth, const float* gt_rgb, const uint8_t* labels,
                                const uint8_t* depth_mask, float color_scaling, float opacity_scaling,
                                float grad_scale, float* losses, int32_t* flags, float* d_depth, float* d_rgb,
                                float* d_opacity, int C, int R, void* stream) {
  if (!depth || !var || !rgb || !opacity || !gt_depth || !gt_rgb || !labels || !depth_mask || !losses ||
      !flags || !d_depth || !d_rgb || !d_opacity || C <= 0 || R <= 0)
    return CNR_E_ARG;
  hipLaunchKernelGGL(loss_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, depth, var, rgb, opacity,
                     gt_depth, gt_rgb, labels, depth_mask, color_scaling, opacity_scaling, grad_scale, losses,
                     flags, d_depth, d_rgb, d_opacity, C, R);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                              float lr, float beta1, float beta2, float eps, float weight_decay,
                              int64_t step_count, float grad_unscale, const int64_t* d_state, void* stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || n <= 0 || (step_count <= 0 && !d_state)) return CNR_E_ARG;
  if (step_count <= 0) step_count = 1;
  const double bc1 = 1.0 - pow((double)beta1, (double)step_count);
  const double bc2 = 1.0 - pow((double)beta2, (double)step_count);
  const float step_size = (float)((double)lr / bc1);
  const float inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
  int64_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  cnr::AdamArgs a{param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, grad_unscale};
  hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, step_size,
                     inv_bc2_sqrt, d_state);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}
