// a11-a13: occupancy activation + exclusive-cumprod termination + the four renders, and their
// backward (src/render_rays.py:3-7, 25-33, 46-50; src/loss.py:41-48).  Modular exact-fp32 kernels:
// one wavefront per ray, lane = sample (S <= 64: one pass; larger S: 64-sample chunks with a carried
// transmittance).  The arithmetic -- recurrence, scans, the double-precision backward -- is render_common.h's
// ray_forward / ray_backward, which cnr_render_loss (render_loss.hip) runs in one launch and is tested bitwise against;
// the fused trainer does its own 32-lane scan inside fused_fwd.hip / fused_bwd_pipe8_kernel.h without ever writing
// alpha / color to HBM.
#include "render_common.h"

namespace {
using namespace cnr_rl;

__global__ __launch_bounds__(256) void composite_fwd_kernel(
    const float* __restrict__ alpha, const float* __restrict__ color, const float* __restrict__ z,
    float* __restrict__ term_out, float* __restrict__ depth, float* __restrict__ var,
    float* __restrict__ rgb, float* __restrict__ opacity, int64_t NR, int S, int in_is_occ) {
  const int lane = threadIdx.x & 63;
  const int64_t ray = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (ray >= NR) return;
  const Renders q = ray_forward<false>(alpha, color, z, term_out, (size_t)(ray * S), S, in_is_occ, lane, nullptr);
  if (lane == 0) {
    if (depth) depth[ray] = q.sd;
    if (var) var[ray] = q.sv;
    if (opacity) opacity[ray] = q.so;
    if (rgb) { rgb[ray * 3 + 0] = q.sr; rgb[ray * 3 + 1] = q.sg; rgb[ray * 3 + 2] = q.sb; }
  }
}

__global__ __launch_bounds__(256) void composite_bwd_kernel(
    const float* __restrict__ alpha, const float* __restrict__ color, const float* __restrict__ z,
    const float* __restrict__ d_depth, const float* __restrict__ d_rgb, const float* __restrict__ d_opacity,
    const float* __restrict__ d_term, float* __restrict__ d_alpha, float* __restrict__ d_color,
    int64_t NR, int S, int in_is_occ) {
  const int lane = threadIdx.x & 63;
  const int64_t ray = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (ray >= NR) return;
  const size_t base = (size_t)(ray * S);
  const float dD = d_depth ? d_depth[ray] : 0.f, dO = d_opacity ? d_opacity[ray] : 0.f;
  const float dR = d_rgb ? d_rgb[ray * 3 + 0] : 0.f, dG = d_rgb ? d_rgb[ray * 3 + 1] : 0.f,
              dBl = d_rgb ? d_rgb[ray * 3 + 2] : 0.f;
  // front to back for the transmittance entering each chunk (the renders themselves are not needed: S <= 64 * RL_MAX_CHUNKS)
  float carry_in[RL_MAX_CHUNKS];
  ray_forward<true>(alpha, nullptr, nullptr, nullptr, base, S, in_is_occ, lane, carry_in);
  ray_backward(alpha, color, z, d_term, dD, dR, dG, dBl, dO, d_alpha, d_color, base, S, in_is_occ, lane, carry_in);
}
}  // namespace

extern "C" int cnr_composite_fwd(const float* alpha, const float* color, const float* z, float* term,
                                 float* depth, float* var, float* rgb, float* opacity, int64_t NR, int S,
                                 int in_is_occ, void* stream) {
  if (!alpha || NR <= 0 || S <= 0) return CNR_E_ARG;
  if ((rgb && !color) || ((depth || var) && !z)) return CNR_E_ARG;
  const int64_t blocks = (NR + 3) / 4;
  hipLaunchKernelGGL(composite_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     alpha, color, z, term, depth, var, rgb, opacity, NR, S, in_is_occ);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_composite_bwd(const float* alpha, const float* color, const float* z,
                                 const float* d_depth, const float* d_rgb, const float* d_opacity,
                                 const float* d_term, float* d_alpha, float* d_color, int64_t NR, int S,
                                 int in_is_occ, void* stream) {
  if (!alpha || !d_alpha || NR <= 0 || S <= 0) return CNR_E_ARG;
  if ((d_rgb && !color) || (d_depth && !z) || (d_color && !color)) return CNR_E_ARG;
  if (S > 64 * cnr_rl::RL_MAX_CHUNKS) return CNR_E_SHAPE;
  const int64_t blocks = (NR + 3) / 4;
  hipLaunchKernelGGL(composite_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     alpha, color, z, d_depth, d_rgb, d_opacity, d_term, d_alpha, d_color, NR, S, in_is_occ);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}
