// Shared by sample.hip (cnr_sample_rays), fused_fwd.hip (cnr_step_prologue) and bg_fused.hip (cnr_bg_tail_sample): a2-a5 for ONE ray
// on one wavefront -- sample_ray, and sample_ray_pool: the same ray with its draws and its sort under its loads.
// See sample.hip for what it restates (src/scene_cateogries.py:24-96, 453-546).
#pragma once
#include "cnr_common.h"

namespace cnr_sample {

struct SampleArgs {
  const uint8_t* rgbs; const float* depth; const float* dirs_c; const float* T; const float* u; const float* g;
  uint64_t seed, offset; const int64_t* d_state; int64_t pool_rows; const float* max_bound; int world_frame;
  int C, R, n1, n2; float eps, stop_eps, min_bound;
  float* z; float* pts; float* origins; float* dirs_o; float* gt_rgb; float* gt_depth; uint8_t* depth_mask;
  uint8_t* labels; const int64_t* pool_indices; int n_obj; int* ray_row; const int* perm;
  // max_bound layout: mb_slices <= 1: one value per class (this step's slice); mb_slices > 1: a (C, mb_slices) table
  // over the epoch's slices, indexed by device cursor / R (filled once per reshuffle by cnr_slice_maxdepth)
  int mb_slices;
  // Philox counter of ray r of local class c: ((c * rng_cstride + rng_c0) * rng_R + rng_r0 + r) * 64 + lane -- the
  // index the ray has in the GLOBAL batch when classes (rng_c0 = first global class, rng_cstride = ranks) or rays
  // (rng_R = global rays per class, rng_r0 = this rank's first ray) are sharded over GPUs, so that N ranks draw
  // exactly what one rank would.  All zero: the local index c * R + r.
  int rng_c0, rng_cstride, rng_R, rng_r0;
};


// ---- Philox4x32-10 (perf mode draws) ---------------------------------------------------------
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
  const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
  c[1] = (uint32_t)p1; c[3] = (uint32_t)p0; c[0] = n0; c[2] = n2;
}
__device__ __forceinline__ void philox4(uint64_t seed, uint64_t ctr_lo, uint64_t ctr_hi, uint32_t (&out)[4]) {
  uint32_t c[4] = {(uint32_t)ctr_lo, (uint32_t)(ctr_lo >> 32), (uint32_t)ctr_hi, (uint32_t)(ctr_hi >> 32)};
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int i = 0; i < 10; ++i) { philox_round(c, k0, k1); k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
  out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = c[3];
}
__device__ __forceinline__ float u01(uint32_t x) { return (float)(x >> 8) * (1.0f / 16777216.0f); }

// torch.linspace(0, 1, n + 1)[i] exactly as ATen computes it on CPU and GPU: step = 1/n, lower half
// counted up from 0, upper half counted down from 1 (scene_cateogries.py:54 calls it per bin count).
__device__ __forceinline__ float linspace01(int i, int n) {
  const float step = 1.0f / (float)n;
  const int steps = n + 1;
  return (i < steps / 2) ? step * (float)i : 1.0f - step * (float)(steps - i - 1);
}

// (cnr::xor_lane, cnr_common.h: lane ^ j on DPP moves for j = 1, 2, 4, 8, ds_bpermute for 16 and 32 -- the network below was 54
//  ds_bpermute per ray, ~3 k cycles of the one wave that samples the ray, on the step's first launch's longest job)
// compare-exchange network over the wave's 64 lanes (one element per lane), ascending
__device__ __forceinline__ void bitonic64(float& v, int lane) {
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const float p = cnr::xor_lane(v, j, lane);
      const bool upper = (lane & j) != 0, asc = (lane & k) == 0;
      v = (upper == asc) ? fmaxf(v, p) : fminf(v, p);
    }
  }
}
// compare-exchange helper for the 128-element bitonic network held as (v0: elem lane, v1: elem lane+64)
__device__ __forceinline__ void bitonic128(float& v0, float& v1, int lane) {
#pragma unroll
  for (int k = 2; k <= 128; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (j == 64) {
        // partner is the other register of the same lane; k == 128 here: ascending everywhere
        const float lo = fminf(v0, v1), hi = fmaxf(v0, v1);
        v0 = lo; v1 = hi;
      } else {
        const float p0 = cnr::xor_lane(v0, j, lane);
        const float p1 = cnr::xor_lane(v1, j, lane);
        const bool upper = (lane & j) != 0;
        const bool asc0 = ((lane) & k) == 0;          // element index lane
        const bool asc1 = ((lane + 64) & k) == 0;     // element index lane + 64
        v0 = (upper == asc0) ? fmaxf(v0, p0) : fminf(v0, p0);
        v1 = (upper == asc1) ? fmaxf(v1, p1) : fminf(v1, p1);
      }
    }
  }
}

// ---- the per-ray arithmetic, shared by sample_ray and sample_ray_pool (one text: the two agree bit for bit) ----------------------
typedef float f4v __attribute__((ext_vector_type(4)));
struct RayFrame { float ox, oy, oz, ex, ey, ez; };
// a2: origin / direction in object (or world) frame from the first three rows m[0..11] of the ray's pose
__device__ __forceinline__ RayFrame ray_frame(const float (&m)[12], float dx, float dy, float dz, int world_frame) {
  const float m00 = m[0], m01 = m[1], m02 = m[2], t0 = m[3];
  const float m10 = m[4], m11 = m[5], m12 = m[6], t1 = m[7];
  const float m20 = m[8], m21 = m[9], m22 = m[10], t2 = m[11];
  float ox, oy, oz, ex, ey, ez;
  if (world_frame) {
    ox = t0; oy = t1; oz = t2;
    ex = m00 * dx + m01 * dy + m02 * dz;
    ey = m10 * dx + m11 * dy + m12 * dz;
    ez = m20 * dx + m21 * dy + m22 * dz;
  } else {
    // general 3x3 inverse (adjugate / det); bottom row of T is (0,0,0,1) for the sim3 poses of
    // the path (scene_cateogries.py:234-238), so inv(T) = [A^-1 | -A^-1 t].
    const float c00 = m11 * m22 - m12 * m21, c01 = m02 * m21 - m01 * m22, c02 = m01 * m12 - m02 * m11;
    const float c10 = m12 * m20 - m10 * m22, c11 = m00 * m22 - m02 * m20, c12 = m02 * m10 - m00 * m12;
    const float c20 = m10 * m21 - m11 * m20, c21 = m01 * m20 - m00 * m21, c22 = m00 * m11 - m01 * m10;
    const float idet = 1.0f / (m00 * c00 + m01 * c10 + m02 * c20);
    const float i00 = c00 * idet, i01 = c01 * idet, i02 = c02 * idet;
    const float i10 = c10 * idet, i11 = c11 * idet, i12 = c12 * idet;
    const float i20 = c20 * idet, i21 = c21 * idet, i22 = c22 * idet;
    ox = -(i00 * t0 + i01 * t1 + i02 * t2);
    oy = -(i10 * t0 + i11 * t1 + i12 * t2);
    oz = -(i20 * t0 + i21 * t1 + i22 * t2);
    ex = i00 * dx + i01 * dy + i02 * dz;
    ey = i10 * dx + i11 * dy + i12 * dz;
    ez = i20 * dx + i21 * dy + i22 * dz;
  }
  return RayFrame{ox, oy, oz, ex, ey, ez};
}
// a4: this lane's Gaussian draws of the ray with Philox index rng_ray: elements lane and lane + 64 of its n2 (+inf beyond n2)
__device__ __forceinline__ void gauss_draws(uint64_t seed, uint64_t rng_ray, uint64_t offset, float eps, int n2, int lane,
                                            float& g0, float& g1) {
  uint32_t rnd[4];
  philox4(seed, rng_ray * 64 + lane, offset ^ 0x9E3779B97F4A7C15ull, rnd);
  const float sd = eps / 3.0f;
  const float r0 = sqrtf(-2.0f * __logf(1.0f - u01(rnd[0]))), a0 = 6.28318530718f * u01(rnd[1]);
  const float r1 = sqrtf(-2.0f * __logf(1.0f - u01(rnd[2]))), a1 = 6.28318530718f * u01(rnd[3]);
  if (lane < n2) g0 = sd * r0 * __cosf(a0);
  if (lane + 64 < n2) g1 = sd * r1 * __cosf(a1);
}
// ... sorted over the ray, clipped to +-eps
__device__ __forceinline__ void sort_clip(float& g0, float& g1, int n2, float eps, int lane) {
  // (up to 64 draws: the second register is all +inf and stays the network's upper half -- the 64-lane network gives the same order)
  if (n2 <= 64) bitonic64(g0, lane); else bitonic128(g0, g1, lane);
  g0 = fminf(fmaxf(g0, -eps), eps);
  g1 = fminf(fmaxf(g1, -eps), eps);
}
// this lane's uniform draw of column s0 + lane
__device__ __forceinline__ float uniform_draw(uint64_t seed, uint64_t rng_ray, uint64_t offset, int s0, int lane) {
  uint32_t rnd[4];
  philox4(seed, rng_ray * 64 + lane, offset + 1 + (s0 >> 6), rnd);
  return u01(rnd[0]);
}
// Column s's z with every product and sum rounded on its own -- no fused multiply-add, except inside linspace01, where ATen's
// linspace fuses too: the reference's CPU arithmetic (stratified_bins, normal_bins_sampling) bit for bit.  write_samples<true>
// (cnr_obj_train, whose z is held to the reference's exactly); the default keeps the contracted expressions below, whose bits the
// other launches are tested to share.
__device__ __forceinline__ float z_unfused(int s, int S, int n1, int n2, float d, bool invalid, bool this_obj, float mb, float gsel,
                                           float uu, float eps, float stop_eps, float min_bound) {
#pragma clang fp contract(off)
  if (invalid) {
    const float range = mb - min_bound;
    return (range * linspace01(s, S) + min_bound) + uu * (range / (float)S);
  }
  if (s < n1) {
    const float range = (d - eps) - min_bound;
    return (range * linspace01(s, n1) + min_bound) + uu * (range / (float)n1);
  }
  if (this_obj) return d + gsel;
  const float lo = d - eps, range = (d + stop_eps) - lo;
  return (range * linspace01(s - n1, n2) + lo) + uu * (range / (float)n2);
}
// a3/a5: per-column z and the sample points of one ray (depth d, slice maximum mb, sorted draws g0 / g1 of "this object" rays)
// (have_uu0: uu0 is this lane's uniform draw of the first 64 columns, drawn by the caller ahead of its loads)
template <bool UNFUSED = false>
__device__ __forceinline__ void write_samples(const SampleArgs& a, int64_t ray, int lane, const RayFrame& f, float d, bool invalid,
                                              bool this_obj, float mb, float g0, float g1, uint64_t rng_ray, uint64_t offset,
                                              bool have_uu0 = false, float uu0 = 0.0f) {
  const float* __restrict__ u = a.u;
  float* __restrict__ z = a.z; float* __restrict__ pts = a.pts;
  const int n1 = a.n1, n2 = a.n2, S = n1 + n2;
  const float eps = a.eps, stop_eps = a.stop_eps, min_bound = a.min_bound;
  const float ox = f.ox, oy = f.oy, oz = f.oz, ex = f.ex, ey = f.ey, ez = f.ez;
  // (loop is wave-uniform: every lane takes part in the shuffles, only loads/stores are predicated)
  for (int s0 = 0; s0 < S; s0 += 64) {
    const int s = s0 + lane;
    const bool live = s < S;
    float uu = 0.0f;
    if (u) {
      if (live) uu = u[ray * S + s];
    } else if (have_uu0 && s0 == 0) {
      uu = uu0;
    } else {
      uu = uniform_draw(a.seed, rng_ray, offset, s0, lane);
    }
    const int i = s - n1;
    const int isrc = i < 0 ? 0 : i;
    const float ga = __shfl(g0, isrc & 63, 64), gb = __shfl(g1, isrc & 63, 64);
    float zz;
    if constexpr (UNFUSED) {
      zz = z_unfused(s, S, n1, n2, d, invalid, this_obj, mb, isrc < 64 ? ga : gb, uu, eps, stop_eps, min_bound);
    } else if (invalid) {
      // stratified(min_bound, max_bound, n1+n2)
      const float range = mb - min_bound;
      zz = (range * linspace01(s, S) + min_bound) + uu * (range / (float)S);
    } else if (s < n1) {
      const float range = (d - eps) - min_bound;
      zz = (range * linspace01(s, n1) + min_bound) + uu * (range / (float)n1);
    } else if (this_obj) {
      zz = d + (isrc < 64 ? ga : gb);
    } else {
      const float lo = d - eps, range = (d + stop_eps) - lo;
      zz = (range * linspace01(i, n2) + lo) + uu * (range / (float)n2);
    }
    if (live) {
      z[ray * S + s] = zz;
      float* p = pts + (ray * S + s) * 3;
      p[0] = ox + ex * zz; p[1] = oy + ey * zz; p[2] = oz + ez * zz;
    }
  }
}
// Philox index of ray r of local class c (SampleArgs::rng_*)
__device__ __forceinline__ uint64_t rng_index(const SampleArgs& a, int c, int64_t ray) {
  return a.rng_R > 0 ? ((uint64_t)c * (uint64_t)(a.rng_cstride > 0 ? a.rng_cstride : 1) + (uint64_t)a.rng_c0) * (uint64_t)a.rng_R
                           + (uint64_t)a.rng_r0 + (uint64_t)(ray - (int64_t)c * a.R)
                     : (uint64_t)ray;
}

// ---- the keyed bijection of the epoch shuffle (cnr_epoch_perm, and cnr_obj_train, which evaluates it per row in its kernel):
// a 6-round balanced Feistel network on 2 * half_bits bits, round keys from Philox4x32 of (seed, epoch, id), cycle-walked back
// into [0, n) (a value >= n is encrypted again: the domain is < 4 n, so at most four expected trips)
__device__ __forceinline__ void epoch_perm_keys(uint64_t seed, uint64_t epoch, uint64_t id, uint32_t (&key)[6]) {
  uint32_t k0[4], k1[4];
  philox4(seed ^ 0x5851F42D4C957F2Dull, epoch, id * 2 + 0, k0);
  philox4(seed ^ 0x5851F42D4C957F2Dull, epoch, id * 2 + 1, k1);
  key[0] = k0[0]; key[1] = k0[1]; key[2] = k0[2]; key[3] = k0[3]; key[4] = k1[0]; key[5] = k1[1];
}
// half the bits of the next even power of two at or above n
__host__ __device__ inline int epoch_perm_half_bits(int64_t n) {
  int bits = 2;
  while ((1ll << bits) < n) bits += 2;
  return bits / 2;
}
__device__ __forceinline__ uint32_t epoch_perm_at(const uint32_t (&key)[6], uint32_t i, int64_t n, int half_bits) {
  const uint32_t mask = (1u << half_bits) - 1u;
  uint32_t x = i;
  do {
    uint32_t l = x >> half_bits, r = x & mask;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      uint32_t f = (r ^ key[t]) * 0x9E3779B1u;
      f ^= f >> 15; f *= 0x85EBCA77u; f ^= f >> 13;
      const uint32_t nl = r;
      r = (l ^ f) & mask;
      l = nl;
    }
    x = (l << half_bits) | r;
  } while ((int64_t)x >= n);
  return x;
}

// one wavefront, one ray whose pool row, Philox index and offset, and slice maximum the caller has worked out: outputs at index
// `ray`, inputs at row `prow` (c: the ray's class, for ray_row only)
template <bool UNFUSED = false>
__device__ __forceinline__ void sample_ray_at(const SampleArgs& a, int64_t ray, int64_t prow, int c, uint64_t rng_ray,
                                              uint64_t offset, float mb, int lane) {
  const uint8_t* __restrict__ rgbs = a.rgbs; const float* __restrict__ depth = a.depth;
  const float* __restrict__ dirs_c = a.dirs_c; const float* __restrict__ T = a.T;
  const float* __restrict__ g = a.g;
  const int n2 = a.n2; const float eps = a.eps, min_bound = a.min_bound;
  float* __restrict__ origins = a.origins;
  float* __restrict__ dirs_o = a.dirs_o; float* __restrict__ gt_rgb = a.gt_rgb; float* __restrict__ gt_depth = a.gt_depth;
  uint8_t* __restrict__ depth_mask = a.depth_mask; uint8_t* __restrict__ labels = a.labels;
  const int64_t* __restrict__ pool_indices = a.pool_indices; const int n_obj = a.n_obj; int* __restrict__ ray_row = a.ray_row;

  const float* Tm = T + prow * 16;
  const float m[12] = {Tm[0], Tm[1], Tm[2], Tm[3], Tm[4], Tm[5], Tm[6], Tm[7], Tm[8], Tm[9], Tm[10], Tm[11]};
  const RayFrame f = ray_frame(m, dirs_c[prow * 3 + 0], dirs_c[prow * 3 + 1], dirs_c[prow * 3 + 2], a.world_frame);

  const float d = depth[prow];
  const uint8_t state = rgbs[prow * 4 + 3];
  const bool invalid = d <= min_bound;
  const bool this_obj = (state == 1) && !invalid;
  if (lane == 0) {
    if (origins) { origins[ray * 3 + 0] = f.ox; origins[ray * 3 + 1] = f.oy; origins[ray * 3 + 2] = f.oz; }
    if (dirs_o) { dirs_o[ray * 3 + 0] = f.ex; dirs_o[ray * 3 + 1] = f.ey; dirs_o[ray * 3 + 2] = f.ez; }
    depth_mask[ray] = invalid ? 0 : 1;
    labels[ray] = state;
    if (ray_row) ray_row[ray] = (int)pool_indices[prow] + c * n_obj;   // row of the class-major code tables
  }
  if (lane < 3) gt_rgb[ray * 3 + lane] = (float)rgbs[prow * 4 + lane] / 255.0f;
  if (lane == 3 && gt_depth) gt_depth[ray] = d;

  // ---- a4: sorted, clipped Gaussian offsets for "this object" rays --------------------------
  float g0 = INFINITY, g1 = INFINITY;  // elements lane and lane+64 of the ray's n2 draws
  if (this_obj) {
    if (g) {
      if (lane < n2) g0 = g[ray * n2 + lane];
      if (lane + 64 < n2) g1 = g[ray * n2 + lane + 64];
    } else {
      gauss_draws(a.seed, rng_ray, offset, eps, n2, lane, g0, g1);
    }
    sort_clip(g0, g1, n2, eps, lane);
  }
  // ---- a3/a5: per-column z -------------------------------------------------------------------
  write_samples<UNFUSED>(a, ray, lane, f, d, invalid, this_obj, mb, g0, g1, rng_ray, offset);
}

// one wavefront, one ray (ray < C * R)
__device__ __forceinline__ void sample_ray(const SampleArgs& a, int64_t ray, int lane) {
  const float* __restrict__ depth = a.depth;
  uint64_t offset = a.offset;
  const int64_t* __restrict__ d_state = a.d_state; const int64_t pool_rows = a.pool_rows;
  const float* __restrict__ max_bound = a.max_bound;
  const int R = a.R;
  const int* __restrict__ perm = a.perm;
  const int c = (int)(ray / R);
  const uint64_t rng_ray = rng_index(a, c, ray);
  // pool row of this ray: either the slice itself (pool_rows == 0) or row cursor + r of a device-resident
  // (C, pool_rows, ...) pool whose cursor lives on the device (hipGraph replay advances it, no host work)
  int64_t prow = ray;
  if (pool_rows > 0) {
    prow = (int64_t)c * pool_rows + d_state[0] + (ray - (int64_t)c * R);
    if (perm) prow = (int64_t)c * pool_rows + perm[prow];   // epoch shuffle = a new permutation, the pool stays put
    offset += (uint64_t)d_state[1] * 4;
  }
  float mb;
  if (max_bound) mb = a.mb_slices > 1 ? max_bound[(int64_t)c * a.mb_slices + (int)(d_state[0] / R)] : max_bound[c];
  else {  // max depth of this step's slice of class c, by this wave (same value as cnr_sample_maxdepth: max is exact)
    float mx = -INFINITY;
    const int64_t base = pool_rows > 0 ? (int64_t)c * pool_rows + d_state[0] : (int64_t)c * R;
    for (int r = lane; r < R; r += 64)
      mx = fmaxf(mx, depth[perm ? (int64_t)c * pool_rows + perm[base + r] : base + r]);
    mb = cnr::wave_max(mx);
  }
  sample_ray_at(a, ray, prow, c, rng_ray, offset, mb, lane);
}

// sample_ray for a ray of a device-resident pool (pool_rows > 0, max_bound given, Philox draws: u = g = NULL, T 16-byte and rgbs
// 4-byte aligned: the caller checks), scheduled for the step's first launch, whose longest job it is.  sample_ray is three
// dependent round trips (device cursor -> permutation entry -> pool row) and only then, because `this_obj` comes out of the pool
// row, the Gaussian draws, the sort and the uniform draws: all of the arithmetic behind all of the waiting.  None of that
// arithmetic needs a loaded value beyond the state -- this_obj only decides whether the sorted draws are USED -- so here the
// Gaussian draws run while the permutation entry is on its way, and the sort and the first uniform draw while the pool row is
// (a pose row as three 16-byte loads, a pixel as one word).  Same functions, same operands per ray: same bits.
__device__ __forceinline__ void sample_ray_pool(const SampleArgs& a, int64_t ray, int lane) {
  const int R = a.R, n2 = a.n2;
  const int64_t pool_rows = a.pool_rows;
  const int64_t cursor = a.d_state[0];
  const uint64_t offset = a.offset + (uint64_t)a.d_state[1] * 4;
  const int c = (int)(ray / R);
  const uint64_t rng_ray = rng_index(a, c, ray);
  // ---- round 2: permutation entry and slice maximum
  int64_t prow = (int64_t)c * pool_rows + cursor + (ray - (int64_t)c * R);
  const int pe = a.perm ? a.perm[prow] : 0;
  const float mb = a.mb_slices > 1 ? a.max_bound[(int64_t)c * a.mb_slices + (int)(cursor / R)] : a.max_bound[c];
  __builtin_amdgcn_sched_barrier(0);
  float g0 = INFINITY, g1 = INFINITY;
  gauss_draws(a.seed, rng_ray, offset, a.eps, n2, lane, g0, g1);   // behind the loads above
  __builtin_amdgcn_sched_barrier(0);
  // ---- round 3: the pool row
  if (a.perm) prow = (int64_t)c * pool_rows + pe;
  const f4v* Tm = reinterpret_cast<const f4v*>(a.T + prow * 16);
  const f4v T0 = Tm[0], T1 = Tm[1], T2 = Tm[2];
  const float dx = a.dirs_c[prow * 3 + 0], dy = a.dirs_c[prow * 3 + 1], dz = a.dirs_c[prow * 3 + 2];
  const float d = a.depth[prow];
  const uint32_t px = *reinterpret_cast<const uint32_t*>(a.rgbs + prow * 4);   // r, g, b, state
  const int64_t pidx = a.ray_row ? a.pool_indices[prow] : 0;
  __builtin_amdgcn_sched_barrier(0);
  sort_clip(g0, g1, n2, a.eps, lane);                                           // behind the loads above
  const float uu0 = uniform_draw(a.seed, rng_ray, offset, 0, lane);
  __builtin_amdgcn_sched_barrier(0);
  const float m[12] = {T0[0], T0[1], T0[2], T0[3], T1[0], T1[1], T1[2], T1[3], T2[0], T2[1], T2[2], T2[3]};
  const RayFrame f = ray_frame(m, dx, dy, dz, a.world_frame);
  const uint8_t state = (uint8_t)(px >> 24);
  const bool invalid = d <= a.min_bound;
  const bool this_obj = (state == 1) && !invalid;
  if (lane == 0) {
    if (a.origins) { a.origins[ray * 3 + 0] = f.ox; a.origins[ray * 3 + 1] = f.oy; a.origins[ray * 3 + 2] = f.oz; }
    if (a.dirs_o) { a.dirs_o[ray * 3 + 0] = f.ex; a.dirs_o[ray * 3 + 1] = f.ey; a.dirs_o[ray * 3 + 2] = f.ez; }
    a.depth_mask[ray] = invalid ? 0 : 1;
    a.labels[ray] = state;
    if (a.ray_row) a.ray_row[ray] = (int)pidx + c * a.n_obj;
  }
  if (lane < 3) a.gt_rgb[ray * 3 + lane] = (float)(uint8_t)(px >> (8 * lane)) / 255.0f;
  if (lane == 3 && a.gt_depth) a.gt_depth[ray] = d;
  write_samples(a, ray, lane, f, d, invalid, this_obj, mb, g0, g1, rng_ray, offset, true, uu0);
}
// whether sample_ray_pool may take a launch's rays (decided on the host, per launch)
inline bool pool_form_ok(const SampleArgs& a) {
  return a.pool_rows > 0 && a.d_state && a.max_bound && !a.u && !a.g && ((uintptr_t)a.T & 15) == 0 && ((uintptr_t)a.rgbs & 3) == 0;
}
}  // namespace cnr_sample
