// The ray compositor -- composite recurrence, per-ray loss terms, composite backward, mask weights -- for every kernel that
// evaluates it in exact fp32: composite.hip, loss.hip, render_loss.hip, bg_fused.hip, pool_step_common.h (obj_fused.hip,
// code_fit.hip), and the masks and mask weights of fused_fwd.hip.  Also the block shape of cnr_render_loss and the reduction
// of its per-block loss partials into loss values and flags (render_loss.hip, tail.hip, bg_fused.hip).
#pragma once
#include "cnr_common.h"

namespace cnr_rl {
constexpr int RL_WAVES = 16, RL_THREADS = RL_WAVES * 64, RL_MAX_CHUNKS = 8;
// rays per block = 16 waves x rays per wave: one ray per wave (all rays in flight at once) until the grid is
// several blocks per CU, then more rays per wave so that the per-block mask count (2 bytes x C x R) stays small
__host__ __device__ inline int rl_rays_per_block(int C, int R) {
  int rpw = (int)(((int64_t)C * R + 8191) / 8192);
  if (rpw < 1) rpw = 1;
  if (rpw > 8) rpw = 8;
  return RL_WAVES * rpw;
}

// one wave per class: partials in a fixed order, flags
__device__ __forceinline__ void finish_class(const float* __restrict__ partials, int nb, float* __restrict__ losses,
                                             int32_t* __restrict__ flags, int C, int c, int lane) {
  const float* hdr = partials + (size_t)C * nb * 3 + (size_t)c * 4;
  const float wd = hdr[0], wc = hdr[1], wo = hdr[2];
  float sd = 0.f, sc = 0.f, so = 0.f;
  const float* pp = partials + (size_t)c * nb * 3;
  for (int b = lane; b < nb; b += 64) { sd += pp[b * 3 + 0]; sc += pp[b * 3 + 1]; so += pp[b * 3 + 2]; }
  sd = cnr::wave_sum(sd) * wd; sc = cnr::wave_sum(sc) * wc; so = cnr::wave_sum(so) * wo;
  if (lane == 0) {
    losses[0 * C + c] = sd; losses[1 * C + c] = sc; losses[2 * C + c] = so;
    int32_t fl = (int32_t)hdr[3];
    if (sd > 100000.f || sc > 100000.f || so > 100000.f) fl |= 1;
    flags[c] = fl;
  }
}

// ---- the ray compositor: every expression of the composite recurrence, of the per-ray loss terms and of the composite backward
// is written ONCE below.  The modular kernels (composite.hip, loss.hip), the one-launch form (render_loss.hip), the background
// backward (bg_fused.hip) and the per-object / code-fit steps (pool_step_common.h) are tested bit for bit against one another, so
// every piece turns fused multiply-add contraction off at function scope: it rounds the same way in whatever unit inlines it.
//
//   occ_i = sigmoid(alpha_i) ; f_i = 1 - occ_i + 1e-10 ; T_i = prod_{j<i} f_j ; term_i = occ_i T_i
//   depth = sum term z ; var = sum term (z - depth)^2 (detached) ; rgb = sum term c ; opacity = sum term
// backward, with g_i = dD z_i + dC.c_i + dO (+ d_term_i) and Suf_i = sum_{k>i} term_k g_k:
//   d occ_i = T_i g_i - Suf_i / f_i          (same division ATen's cumprod backward performs)
//   d alpha_i = d occ_i occ_i (1 - occ_i) ; d c_i = term_i dC
// One wave per ray, lane = sample, rays longer than a wave in 64-sample chunks: the transmittance is carried forward from chunk
// to chunk, the suffix sum backward.  T and term are fp32 as in the forward; g, the suffix sum and d occ are formed in double and
// rounded once.  T_i g_i and Suf_i / f_i nearly cancel wherever g varies slowly along the ray, which leaves the fp32 roundings of
// g_i and of the suffix sum standing at up to 17 ulp of the result; ATen's CPU cumsum / cumprod, which the reference's backward
// runs through, accumulate float32 in double as well.
constexpr float MASK_EPS = 1e-10f;   // in f_i and in 1 / (mask count + eps), as src/render_rays.py

// inclusive product scan across the wave (Hillis-Steele, 6 steps)
__device__ __forceinline__ float incl_prod(float v, int lane) {
#pragma clang fp contract(off)
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float p = __shfl_up(v, o, 64);
    if (lane >= o) v *= p;
  }
  return v;
}
// inclusive suffix sum across the wave
__device__ __forceinline__ double incl_suffix_sum(double v, int lane) {
#pragma clang fp contract(off)
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double p = __shfl_down(v, o, 64);
    if (lane + o < 64) v += p;
  }
  return v;
}
// exclusive suffix sum (k > i) from the inclusive one: the next lane's value.  Not (incl - v): that difference carries the
// rounding of v = term_i g_i, which the backward divides by f_i, and f_i is 1e-10 where occ_i = 1.
__device__ __forceinline__ double excl_suffix(double incl, int lane) {
  const double nxt = __shfl_down(incl, 1, 64);
  return lane == 63 ? 0.0 : nxt;
}
__device__ __forceinline__ float sigmoid_exact(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float sgn(float x) { return (x > 0.f) ? 1.f : ((x < 0.f) ? -1.f : 0.f); }

// the three masks of a ray from its label and its depth bit (src/loss.py:18-40): depth (a valid depth on this or another
// object), colour (label != 0: an object), opacity (label != 2: this object or empty space)
struct MaskBits { bool md, mo, ms; };
__device__ __forceinline__ MaskBits mask_bits(unsigned lab, bool depth_ok) {
  const bool mo = lab != 0;
  return {depth_ok && mo, mo, lab != 2};
}
// 1 / mask count of the three terms, and the flag bits 2, 4, 8: a term whose mask is empty (in ANY class, render_rays.py:67-72)
// is zero and has no gradient.  (The bits are a function of their own: formed with the weights they stay live across the ray loop
// of bg_bwd_kernel<RENDER>, one register above its 128.)
struct MaskWeights { float wd, wc, wo; };
__device__ __forceinline__ MaskWeights mask_weights(float nd, float nc, float no, bool empty_d, bool empty_c, bool empty_o) {
#pragma clang fp contract(off)
  return {empty_d ? 0.f : 1.0f / (nd + MASK_EPS), empty_c ? 0.f : 1.0f / (nc + MASK_EPS), empty_o ? 0.f : 1.0f / (no + MASK_EPS)};
}
__device__ __forceinline__ int mask_flags(bool empty_d, bool empty_c, bool empty_o) {
  return (empty_d ? 2 : 0) | (empty_c ? 4 : 0) | (empty_o ? 8 : 0);
}

// one 64-sample chunk: this lane's occupancy (v is alpha, or occ itself with in_is_occ; dead lanes are neutral), f, and the
// inclusive / exclusive product of f over the chunk's lanes
struct Chunk { float occ, f, incl, excl; };
__device__ __forceinline__ Chunk scan_chunk(float v, bool live, int in_is_occ, int lane) {
#pragma clang fp contract(off)
  Chunk k;
  k.occ = live ? (in_is_occ ? v : sigmoid_exact(v)) : 0.0f;
  k.f = live ? (1.0f - k.occ + MASK_EPS) : 1.0f;
  k.incl = incl_prod(k.f, lane);
  k.excl = __shfl_up(k.incl, 1, 64);
  if (lane == 0) k.excl = 1.0f;
  return k;
}

// the renders of one ray (all lanes).  color / z / term_out may be null.  CARRIES: carry_in[RL_MAX_CHUNKS] receives the
// transmittance entering each chunk, which ray_backward needs back to front (S <= 64 * RL_MAX_CHUNKS then), and the variance
// pass reads it back; without, S has no limit, carry_in is not touched and the second pass carries the transmittance again.
// (A compile-time choice: a null test in front of the store moves the array from registers to LDS.)
struct Renders { float sd, sv, so, sr, sg, sb; };
template <bool CARRIES>
__device__ __forceinline__ Renders ray_forward(const float* __restrict__ alpha, const float* __restrict__ color,
                                               const float* __restrict__ z, float* __restrict__ term_out, size_t base, int S,
                                               int in_is_occ, int lane, float* carry_in) {
#pragma clang fp contract(off)
  Renders r;
  float carry = 1.0f;  // transmittance entering this chunk
  float sd = 0.f, so = 0.f, sr = 0.f, sg = 0.f, sb = 0.f;
  for (int s0 = 0; s0 < S; s0 += 64) {
    if constexpr (CARRIES) carry_in[s0 >> 6] = carry;
    const int s = s0 + lane;
    const bool live = s < S;
    const Chunk k = scan_chunk(live ? alpha[base + s] : 0.0f, live, in_is_occ, lane);
    const float term = k.occ * (carry * k.excl);
    if (live) {
      const float zz = z ? z[base + s] : 0.0f;
      if (term_out) term_out[base + s] = term;
      sd += term * zz; so += term;
      if (color) {
        const float* cp = color + (base + s) * 3;
        sr += term * cp[0]; sg += term * cp[1]; sb += term * cp[2];
      }
    }
    carry *= __shfl(k.incl, 63, 64);
  }
  r.sd = cnr::wave_sum(sd); r.so = cnr::wave_sum(so);
  r.sr = cnr::wave_sum(sr); r.sg = cnr::wave_sum(sg); r.sb = cnr::wave_sum(sb);
  // var = sum term (z - depth)^2, second pass for the exact two-pass form the reference uses; (occ carry) excl, left to right
  float sv = 0.f;
  carry = 1.0f;
  for (int s0 = 0; s0 < S; s0 += 64) {
    const int s = s0 + lane;
    const bool live = s < S;
    const Chunk k = scan_chunk(live ? alpha[base + s] : 0.0f, live, in_is_occ, lane);
    if constexpr (CARRIES) carry = carry_in[s0 >> 6];
    if (live) { const float dz = (z ? z[base + s] : 0.0f) - r.sd; sv += k.occ * carry * k.excl * dz * dz; }
    if constexpr (!CARRIES) carry *= __shfl(k.incl, 63, 64);
  }
  r.sv = cnr::wave_sum(sv);
  return r;
}

// a ray's loss terms and their gradients w.r.t. its renders (src/loss.py:18-74).  The un-normalised terms come as the two
// factors of their last product -- depth ad * info, colour ac * fo, opacity ao * fs --, so that a caller that accumulates them
// writes `sum += a * b` in its OWN contraction mode (loss.hip contracts that multiply-add, the others do not).
struct RayLoss {
  float ad, info, ac, fo, ao, fs;
  float dD, dR, dG, dBl, dO;         // d loss / d depth, rgb, opacity (x grad_scale)
};
__device__ __forceinline__ RayLoss ray_loss(const Renders& q, float gtd, float g0, float g1, float g2, unsigned lab, bool depth_ok,
                                            float wd, float wc, float wo, float color_scaling, float opacity_scaling,
                                            float grad_scale) {
#pragma clang fp contract(off)
  RayLoss l;
  const MaskBits m = mask_bits(lab, depth_ok);
  const float fd = m.md ? 1.f : 0.f;
  l.fo = m.mo ? 1.f : 0.f; l.fs = m.ms ? 1.f : 0.f;
  const float rd = q.sd - gtd;
  l.info = 1.0f / (sqrtf(q.sv) + 1e-4f);
  const float rc0 = q.sr - g0, rc1 = q.sg - g1, rc2 = q.sb - g2;
  const float ro = q.so - l.fo;
  l.ad = fabsf(rd) * fd;
  l.ac = fabsf(rc0) + fabsf(rc1) + fabsf(rc2);
  l.ao = fabsf(ro);
  l.dD = grad_scale * sgn(rd) * fd * l.info * wd;
  l.dR = grad_scale * color_scaling * sgn(rc0) * l.fo * wc;
  l.dG = grad_scale * color_scaling * sgn(rc1) * l.fo * wc;
  l.dBl = grad_scale * color_scaling * sgn(rc2) * l.fo * wc;
  l.dO = grad_scale * opacity_scaling * sgn(ro) * l.fs * wo;
  return l;
}

// g_i of this lane's sample (0 for a dead lane) from the upstream gradients and the sample's z and colour
__device__ __forceinline__ double sample_g(bool live, float dD, float zz, float dR, float dG, float dBl, float c0, float c1, float c2,
                                           float dO) {
#pragma clang fp contract(off)
  return live ? (double)dD * (double)zz + (double)dR * (double)c0 + (double)dG * (double)c1 + (double)dBl * (double)c2 + (double)dO
              : 0.0;
}
// d occ of this lane's sample from T_i, g_i, f_i, its own term_i g_i and the suffix sum of the later chunks (added AFTER the
// exclusive suffix of this chunk).  incl_suf: this chunk's inclusive suffix sum, whose lane 0 the next chunk's suf_carry takes up.
__device__ __forceinline__ double sample_docc(float T, double g, float f, float term, double suf_carry, int lane, double& incl_suf) {
#pragma clang fp contract(off)
  const double tg = (double)term * g;
  incl_suf = incl_suffix_sum(tg, lane);
  const double suf = excl_suffix(incl_suf, lane) + suf_carry;
  return (double)T * g - suf / (double)f;
}

// composite backward of one ray, back to front: d_alpha (d occ with in_is_occ) and, where d_color is given, d colour of every
// sample.  carry_in: ray_forward's.  color / z / d_term / d_color may be null.
__device__ __forceinline__ void ray_backward(const float* __restrict__ alpha, const float* __restrict__ color,
                                             const float* __restrict__ z, const float* __restrict__ d_term, float dD, float dR,
                                             float dG, float dBl, float dO, float* __restrict__ d_alpha,
                                             float* __restrict__ d_color, size_t base, int S, int in_is_occ, int lane,
                                             const float* carry_in) {
#pragma clang fp contract(off)
  double suf_carry = 0.0;  // sum_{k in later chunks} term_k g_k
  for (int ch = (S + 63) / 64 - 1; ch >= 0; --ch) {
    const int s = ch * 64 + lane;
    const bool live = s < S;
    const Chunk k = scan_chunk(live ? alpha[base + s] : 0.0f, live, in_is_occ, lane);
    const float T = carry_in[ch] * k.excl;
    const float term = k.occ * T;
    float zz = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f;
    if (live) {
      if (z) zz = z[base + s];
      if (color) { const float* cp = color + (base + s) * 3; c0 = cp[0]; c1 = cp[1]; c2 = cp[2]; }
    }
    double g = sample_g(live, dD, zz, dR, dG, dBl, c0, c1, c2, dO);
    if (live && d_term) g += (double)d_term[base + s];
    double incl_suf;
    const double docc = sample_docc(T, g, k.f, term, suf_carry, lane, incl_suf);
    if (live) {
      d_alpha[base + s] = (float)(in_is_occ ? docc : docc * (double)k.occ * (1.0 - (double)k.occ));
      if (d_color) { float* dc = d_color + (base + s) * 3; dc[0] = term * dR; dc[1] = term * dG; dc[2] = term * dBl; }
    }
    suf_carry += __shfl(incl_suf, 0, 64);
  }
}

// ---- one ray of S <= 64 samples on one wave (lane = sample): the same pieces with the whole ray in one register per lane --
// sigmoid, scan and loads happen once -- down to d sigma / d colour of this lane's sample.  cnr_render_loss's fast path, the
// background backward's in-kernel composite and the per-object / code-fit composite are this function.
struct RayOut {
  float sd, sv, so, sr, sg, sb;      // depth, variance, opacity, rgb of the ray (all lanes)
  float ld, lc, lo;                  // the ray's un-normalised loss terms (all lanes)
  float dsig, dc0, dc1, dc2;         // this lane's sample: d sigma, d colour (x grad_scale); 0 for lanes >= S
  bool live;
};
__device__ __forceinline__ RayOut ray_small(const float* __restrict__ sigmas, const float* __restrict__ colors,
                                            const float* __restrict__ z, size_t base, int S, int lane, float gtd, float g0,
                                            float g1, float g2, uint8_t lab, uint8_t dmask, float wd, float wc, float wo,
                                            float color_scaling, float opacity_scaling, float grad_scale) {
#pragma clang fp contract(off)
  RayOut r;
  const bool live = lane < S;
  const Chunk k = scan_chunk(live ? sigmas[base + lane] : 0.0f, live, 0, lane);
  const float T = k.excl;
  const float term = k.occ * (1.0f * T);
  float zz = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f;
  if (live) { zz = z[base + lane]; const float* cp = colors + (base + lane) * 3; c0 = cp[0]; c1 = cp[1]; c2 = cp[2]; }
  float sd = 0.f, so = 0.f, sr = 0.f, sg = 0.f, sb = 0.f;
  if (live) { sd += term * zz; so += term; sr += term * c0; sg += term * c1; sb += term * c2; }
  Renders q;
  q.sd = cnr::wave_sum(sd); q.so = cnr::wave_sum(so);
  q.sr = cnr::wave_sum(sr); q.sg = cnr::wave_sum(sg); q.sb = cnr::wave_sum(sb);
  float sv = 0.f;
  if (live) { const float dz = zz - q.sd; sv += k.occ * 1.0f * T * dz * dz; }
  q.sv = cnr::wave_sum(sv);
  r.sd = q.sd; r.sv = q.sv; r.so = q.so; r.sr = q.sr; r.sg = q.sg; r.sb = q.sb;
  const RayLoss l = ray_loss(q, gtd, g0, g1, g2, lab, dmask != 0, wd, wc, wo, color_scaling, opacity_scaling, grad_scale);
  r.ld = l.ad * l.info; r.lc = l.ac * l.fo; r.lo = l.ao * l.fs;
  const double g = sample_g(live, l.dD, zz, l.dR, l.dG, l.dBl, c0, c1, c2, l.dO);
  double incl_suf;
  const double docc = sample_docc(T, g, k.f, term, 0.0, lane, incl_suf);
  r.live = live;
  r.dsig = 0.0f; r.dc0 = 0.0f; r.dc1 = 0.0f; r.dc2 = 0.0f;
  if (live) {
    r.dsig = (float)(docc * (double)k.occ * (1.0 - (double)k.occ));
    r.dc0 = term * l.dR; r.dc1 = term * l.dG; r.dc2 = term * l.dBl;
  }
  return r;
}
}  // namespace cnr_rl
