// Scene view rendering: which pixel rays meet which entity's volume and over what depth range
// (cnr_view_segments_*), the sample points of every segment in its field's frame (cnr_view_points), and the per-pixel merge
// of several fields' samples into one alpha composite with an instance label (cnr_view_composite).  The field values in
// between come from the existing kernels (cnr_field_fwd, the background forward).  With empty-space skipping
// cnr_view_active_count / _emit stand in for cnr_view_points: they list the samples that lie in set cells of their entity's
// occupancy grid (viewgrid.hip), the fields run on that list alone, and cnr_view_scatter_active puts the values back.
//
// An entity is a box: to_box (3,4) maps a world point into [-1,1]^3.  Ray directions are (x, y, 1) in the camera frame (z-depth
// convention, not normalised) and every transform is a similarity, so the parameter z of o + z d is the camera depth in every
// frame; samples of different entities along one pixel ray are merged by z.
//
// Determinism: no atomics.  Segment positions come from wave ballots and one exclusive scan of the per-wave counts; the
// composite's sums run in a fixed order.  The count and emit launches evaluate the same slab test (one device function,
// no fused multiply-add contraction) so that they agree on every hit.
#include "cnr_common.h"
#include "geom_common.h"
#include "render_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int KMAX = CNR_VIEW_KMAX;
constexpr int SMAX = CNR_VIEW_SMAX;

struct Cam { float r[9]; float t[3]; };

__device__ __forceinline__ Cam load_cam(const float* __restrict__ T) {
  Cam c;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) c.r[i * 3 + j] = T[i * 4 + j];
    c.t[i] = T[i * 4 + 3];
  }
  return c;
}

// a (3,4) affine applied to a point / to a direction, sums left to right
__device__ __forceinline__ void affine_point(const float* __restrict__ A, float x, float y, float z, float* out) {
#pragma unroll
  for (int k = 0; k < 3; ++k) out[k] = A[k * 4 + 0] * x + A[k * 4 + 1] * y + A[k * 4 + 2] * z + A[k * 4 + 3];
}
__device__ __forceinline__ void affine_dir(const float* __restrict__ A, float x, float y, float z, float* out) {
#pragma unroll
  for (int k = 0; k < 3; ++k) out[k] = A[k * 4 + 0] * x + A[k * 4 + 1] * y + A[k * 4 + 2] * z;
}

// slab test of t + z dw against the box of `A`; [zn, zf] clipped to [zmin, zmax].  An axis with a zero direction component
// passes iff the origin lies inside the slab and bounds nothing (no 0 * inf).
__device__ __forceinline__ bool slab(const float* __restrict__ A, const Cam& cam, const float* dw, float zmin, float zmax,
                                     float& zn, float& zf) {
  float o[3], d[3];
  affine_point(A, cam.t[0], cam.t[1], cam.t[2], o);
  affine_dir(A, dw[0], dw[1], dw[2], d);
  zn = zmin; zf = zmax;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (d[k] == 0.0f) {
      ok = ok && (fabsf(o[k]) <= 1.0f);
    } else {
      const float t1 = (-1.0f - o[k]) / d[k], t2 = (1.0f - o[k]) / d[k];
      zn = fmaxf(zn, fminf(t1, t2));
      zf = fminf(zf, fmaxf(t1, t2));
    }
  }
  return ok && zf > zn;
}

__device__ __forceinline__ void world_dir(const Cam& cam, const float* __restrict__ dirs, int64_t p, float* dw) {
  const float x = dirs[p * 3 + 0], y = dirs[p * 3 + 1], z = dirs[p * 3 + 2];
#pragma unroll
  for (int k = 0; k < 3; ++k) dw[k] = cam.r[k * 3 + 0] * x + cam.r[k * 3 + 1] * y + cam.r[k * 3 + 2] * z;
}

// workspace: counts (E * nw) i32 | over (nw) i32 | offsets (E * nw) i64, nw = waves of 64 pixels
__host__ __device__ inline int64_t n_waves(int64_t P) { return (P + 63) / 64; }
__host__ __device__ inline int64_t ws_counts_bytes(int64_t P, int E) { return ((E + 1) * n_waves(P) * 4 + 15) / 16 * 16; }

__global__ __launch_bounds__(256) void segments_count_kernel(const float* __restrict__ T_wc, const float* __restrict__ dirs,
                                                             const float* __restrict__ to_box, int64_t P, int E, float zmin,
                                                             float zmax, int* __restrict__ counts, int* __restrict__ over) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = n_waves(P);
  const int64_t wv = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wv >= nw) return;
  const int64_t p = wv * 64 + lane;
  const bool live = p < P;
  const Cam cam = load_cam(T_wc);
  float dw[3] = {0.f, 0.f, 0.f};
  if (live) world_dir(cam, dirs, p, dw);
  int mine = 0;
  for (int e = 0; e < E; ++e) {
    float zn, zf;
    const bool hit = live && slab(to_box + (int64_t)e * 12, cam, dw, zmin, zmax, zn, zf);
    const unsigned long long m = __ballot(hit);
    mine += hit ? 1 : 0;
    if (lane == 0) counts[(int64_t)e * nw + wv] = __popcll(m);
  }
  const unsigned long long mo = __ballot(mine > KMAX);
  if (lane == 0) over[wv] = __popcll(mo);
}

// one block: exclusive scan of the (E * nw) counts in (entity, wave) order -> offsets; entity_offset, total, overflow
__global__ __launch_bounds__(1024) void segments_scan_kernel(const int* __restrict__ counts, const int* __restrict__ over,
                                                             int64_t nw, int E, int64_t* __restrict__ offsets,
                                                             int64_t* __restrict__ entity_offset, int64_t* __restrict__ total,
                                                             int64_t* __restrict__ overflow) {
  __shared__ int64_t part[cnr::SCAN_THREADS];
  const int t = threadIdx.x;
  cnr::scan_block_counts<1>(counts, nw * E, offsets, total, part);
  if (t == 1023 && entity_offset) entity_offset[E] = part[1023];
  __syncthreads();
  if (entity_offset) for (int e = t; e < E; e += 1024) entity_offset[e] = offsets[(int64_t)e * nw];
  if (overflow) {
    int64_t ov = 0;
    for (int64_t i = t; i < nw; i += 1024) ov += over[i];
    __syncthreads();
    part[t] = ov;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) { if (t < o) part[t] += part[t + o]; __syncthreads(); }
    if (t == 0) overflow[0] = part[0];
  }
}

__global__ __launch_bounds__(256) void segments_emit_kernel(const float* __restrict__ T_wc, const float* __restrict__ dirs,
                                                            const float* __restrict__ to_box, int64_t P, int E, float zmin,
                                                            float zmax, const int64_t* __restrict__ offsets,
                                                            int* __restrict__ seg_pixel, int* __restrict__ seg_entity,
                                                            float* __restrict__ seg_z, int* __restrict__ pix_segs) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = n_waves(P);
  const int64_t wv = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wv >= nw) return;
  const int64_t p = wv * 64 + lane;
  const bool live = p < P;
  const Cam cam = load_cam(T_wc);
  float dw[3] = {0.f, 0.f, 0.f};
  if (live) world_dir(cam, dirs, p, dw);
  int ks[KMAX];
  float kz[KMAX];
#pragma unroll
  for (int j = 0; j < KMAX; ++j) { ks[j] = -1; kz[j] = 0.f; }
  int n = 0;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int e = 0; e < E; ++e) {
    float zn, zf;
    const bool hit = live && slab(to_box + (int64_t)e * 12, cam, dw, zmin, zmax, zn, zf);
    const unsigned long long m = __ballot(hit);
    if (!hit) continue;
    const int64_t s = offsets[(int64_t)e * nw + wv] + __popcll(m & below);
    seg_pixel[s] = (int)p;
    seg_entity[s] = e;
    seg_z[s * 2 + 0] = zn;
    seg_z[s * 2 + 1] = zf;
    if (n < KMAX) {
#pragma unroll
      for (int j = 0; j < KMAX; ++j) if (j == n) { ks[j] = (int)s; kz[j] = zn; }
      ++n;
    } else {                       // more than KMAX boxes: keep the KMAX nearest by z_near (ties: the earlier entity), entity order
      int w = 0;
      float wz = kz[0];
#pragma unroll
      for (int j = 1; j < KMAX; ++j) if (kz[j] >= wz) { w = j; wz = kz[j]; }
      if (zn < wz) {
#pragma unroll
        for (int j = 0; j < KMAX - 1; ++j) if (j >= w) { ks[j] = ks[j + 1]; kz[j] = kz[j + 1]; }
        ks[KMAX - 1] = (int)s; kz[KMAX - 1] = zn;
      }
    }
  }
  if (live) {
#pragma unroll
    for (int j = 0; j < KMAX; ++j) pix_segs[p * KMAX + j] = ks[j];
  }
}

// sample i of S of segment [zn, zf] on pixel ray p: z, and the point in the frame of the affine F (sums left to right)
__device__ __forceinline__ float sample_world(const Cam& cam, const float* __restrict__ dirs, int64_t p, float zn, float zf, int i,
                                              int S, float* w) {
  const float z = zn + ((float)i + 0.5f) * (zf - zn) / (float)S;
  const float cx = z * dirs[p * 3 + 0], cy = z * dirs[p * 3 + 1], cz = z * dirs[p * 3 + 2];
#pragma unroll
  for (int k = 0; k < 3; ++k) w[k] = cam.r[k * 3 + 0] * cx + cam.r[k * 3 + 1] * cy + cam.r[k * 3 + 2] * cz + cam.t[k];
  return z;
}

__global__ __launch_bounds__(256) void points_kernel(const float* __restrict__ T_wc, const float* __restrict__ dirs,
                                                     const float* __restrict__ to_field, const int* __restrict__ seg_pixel,
                                                     const int* __restrict__ seg_entity, const float* __restrict__ seg_z,
                                                     int64_t N, int S, float* __restrict__ z_out,
                                                     float* __restrict__ pts) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= N * S) return;
  const int64_t s = idx / S;
  const int i = (int)(idx - s * S);
  const Cam cam = load_cam(T_wc);
  const int64_t p = seg_pixel[s];
  const float* F = to_field + (int64_t)seg_entity[s] * 12;
  float w[3], f[3];
  const float z = sample_world(cam, dirs, p, seg_z[s * 2], seg_z[s * 2 + 1], i, S, w);
  affine_point(F, w[0], w[1], w[2], f);
  z_out[idx] = z;
  pts[idx * 3 + 0] = f[0]; pts[idx * 3 + 1] = f[1]; pts[idx * 3 + 2] = f[2];
}

// ---- active samples (empty-space skipping) ----------------------------------------------------------------------------------
// Sample idx = n * S + i of the (N,S) samples is active iff the cell of its entity's occupancy grid that holds its box
// coordinate is set, or the entity has no grid.  The compact list keeps the active samples in idx order (= entity, segment,
// sample), every entity's run padded to whole blocks of 64.  Position of an active sample: active_offset[e] + (its rank among
// all active samples) - (the rank of the entity's first sample).  The ranks come from one 64-bit mask per wave of 64
// consecutive samples, the wave's offset inside its count block of ACT_WAVES waves, and one exclusive scan of the blocks'
// counts; the emit launch reads the masks, so that it cannot disagree with the count launch.
// workspace: mask (nw) u64 | wave_local (nw) i32 | blk_count (nb) i32 | blk_off (nb) i64 | first (E+1) i64 | padded (E) i64,
// nb = ceil(nw / ACT_WAVES), each part 16-aligned
constexpr int ACT_WAVES = 16;
struct ActiveWs { uint64_t* mask; int* wave_local; int* blk_count; int64_t* blk_off; int64_t* first; int64_t* padded; int64_t bytes; };
__host__ __device__ inline int64_t up16(int64_t x) { return (x + 15) / 16 * 16; }
__host__ __device__ inline int64_t n_count_blocks(int64_t NS) { return (n_waves(NS) + ACT_WAVES - 1) / ACT_WAVES; }
__host__ __device__ inline ActiveWs active_ws(void* base, int64_t NS, int E) {
  const int64_t nw = n_waves(NS), nb = n_count_blocks(NS);
  char* b = static_cast<char*>(base);
  ActiveWs w;
  int64_t o = 0;
  w.mask = reinterpret_cast<uint64_t*>(b + o); o += up16(nw * 8);
  w.wave_local = reinterpret_cast<int*>(b + o); o += up16(nw * 4);
  w.blk_count = reinterpret_cast<int*>(b + o); o += up16(nb * 4);
  w.blk_off = reinterpret_cast<int64_t*>(b + o); o += up16(nb * 8);
  w.first = reinterpret_cast<int64_t*>(b + o); o += up16(((int64_t)E + 1) * 8);
  w.padded = reinterpret_cast<int64_t*>(b + o); o += up16((int64_t)E * 8);
  w.bytes = o;
  return w;
}

__device__ __forceinline__ int grid_axis(float b, int G) {
  return min(G - 1, max(0, (int)floorf((b + 1.0f) * 0.5f * (float)G)));
}

__global__ __launch_bounds__(ACT_WAVES * 64) void active_count_kernel(const float* __restrict__ T_wc, const float* __restrict__ dirs,
                                                           const float* __restrict__ to_box, const int* __restrict__ seg_pixel,
                                                           const int* __restrict__ seg_entity, const float* __restrict__ seg_z,
                                                           int64_t NS, int S, const int* __restrict__ grid_words,
                                                           const int* __restrict__ entity_grid, int G,
                                                           uint64_t* __restrict__ mask, int* __restrict__ wave_local,
                                                           int* __restrict__ blk_count) {
  __shared__ int s_wave[ACT_WAVES];
  const int lane = threadIdx.x & 63;
  const int64_t wv = (int64_t)blockIdx.x * ACT_WAVES + (threadIdx.x >> 6);      // (a wave past the last one counts nothing)
  const int64_t idx = wv * 64 + lane;
  bool active = false;
  if (idx < NS) {
    const int64_t s = idx / S;
    const int i = (int)(idx - s * S);
    const int e = seg_entity[s];
    const int g = entity_grid[e];
    active = g < 0;
    if (!active) {
      const Cam cam = load_cam(T_wc);
      float w[3], b[3];
      sample_world(cam, dirs, seg_pixel[s], seg_z[s * 2], seg_z[s * 2 + 1], i, S, w);
      affine_point(to_box + (int64_t)e * 12, w[0], w[1], w[2], b);
      const int64_t cell = ((int64_t)grid_axis(b[0], G) * G + grid_axis(b[1], G)) * G + grid_axis(b[2], G);
      const int64_t words = (int64_t)G * G * G / 32;
      active = (grid_words[(int64_t)g * words + (cell >> 5)] >> (int)(cell & 31)) & 1;
    }
  }
  const unsigned long long m = __ballot(active);
  int block_total;
  const int base = cnr::block_prefix_waves<ACT_WAVES>(0, __popcll(m), s_wave, &block_total);
  if (lane == 0 && wv < n_waves(NS)) { mask[wv] = m; wave_local[wv] = base; }
  if (threadIdx.x == 0) blk_count[blockIdx.x] = block_total;
}

// the number of active samples below sample idx (idx <= NS; the workspace as the count launch and the scan left it)
__device__ __forceinline__ int64_t active_rank(const ActiveWs& w, int64_t idx, int64_t NS, int64_t total) {
  if (idx >= NS) return total;
  const int64_t wv = idx >> 6;
  const int l = (int)(idx & 63);
  return w.blk_off[wv / ACT_WAVES] + w.wave_local[wv] + __popcll(w.mask[wv] & ((1ull << l) - 1ull));
}

// one block: exclusive scan of the count blocks' counts; per entity the rank of its first sample and its run padded to 64; the
// exclusive scan of those -> active_offset (E+1); the unpadded total
__global__ __launch_bounds__(1024) void active_scan_kernel(ActiveWs w, const int64_t* __restrict__ entity_offset, int64_t NS,
                                                           int S, int E, int64_t* __restrict__ active_offset,
                                                           int64_t* __restrict__ total_out) {
  __shared__ int64_t part[cnr::SCAN_THREADS];
  __shared__ int64_t total;
  const int t = threadIdx.x;
  cnr::scan_block_counts<1>(w.blk_count, n_count_blocks(NS), w.blk_off, &total, part);
  __syncthreads();
  for (int e = t; e <= E; e += 1024) w.first[e] = active_rank(w, entity_offset[e] * S, NS, total);
  __syncthreads();
  for (int e = t; e < E; e += 1024) w.padded[e] = (w.first[e + 1] - w.first[e] + 63) / 64 * 64;
  __syncthreads();
  cnr::scan_block_counts<1>(w.padded, (int64_t)E, active_offset, active_offset + E, part);
  if (t == 0) total_out[0] = total;
}

__global__ __launch_bounds__(256) void active_emit_kernel(const float* __restrict__ T_wc, const float* __restrict__ dirs,
                                                          const float* __restrict__ to_field, const int* __restrict__ seg_pixel,
                                                          const int* __restrict__ seg_entity, const float* __restrict__ seg_z,
                                                          int64_t NS, int S, int E, const int* __restrict__ entity_row,
                                                          ActiveWs w, const int64_t* __restrict__ active_offset, int64_t M,
                                                          float* __restrict__ z_out, int64_t* __restrict__ active_idx,
                                                          float* __restrict__ pts_c, int* __restrict__ block_row) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx < NS) {
    const int64_t s = idx / S;
    const int i = (int)(idx - s * S);
    const int e = seg_entity[s];
    const Cam cam = load_cam(T_wc);
    float wp[3], f[3];
    z_out[idx] = sample_world(cam, dirs, seg_pixel[s], seg_z[s * 2], seg_z[s * 2 + 1], i, S, wp);
    if ((w.mask[idx >> 6] >> (idx & 63)) & 1ull) {
      const int64_t pos = active_offset[e] + active_rank(w, idx, NS, 0) - w.first[e];
      if (pos >= 0 && pos < M) {
        affine_point(to_field + (int64_t)e * 12, wp[0], wp[1], wp[2], f);
        active_idx[pos] = idx;
        pts_c[pos * 3 + 0] = f[0]; pts_c[pos * 3 + 1] = f[1]; pts_c[pos * 3 + 2] = f[2];
      }
    }
  }
  // the padding behind every entity's run (fewer than 64 entries): lane l of the first E * 64 threads
  if (idx < (int64_t)E * 64) {
    const int e = (int)(idx >> 6);
    const int64_t pos = active_offset[e] + (w.first[e + 1] - w.first[e]) + (idx & 63);
    if (pos < active_offset[e + 1] && pos < M) {
      active_idx[pos] = -1;
      pts_c[pos * 3 + 0] = 0.f; pts_c[pos * 3 + 1] = 0.f; pts_c[pos * 3 + 2] = 0.f;
    }
  }
  // the code-table row of every block of 64: the entity whose run holds it (runs of no block are passed over)
  if (idx < M / 64) {
    int lo = 0, hi = E;                      // the last e with active_offset[e] <= idx * 64
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (active_offset[mid] <= idx * 64) lo = mid; else hi = mid;
    }
    block_row[idx] = entity_row[lo];
  }
}

__global__ __launch_bounds__(256) void fill_empty_kernel(int64_t NS, float* __restrict__ sigma, float* __restrict__ color) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= NS) return;
  sigma[idx] = -INFINITY;
  color[idx * 3 + 0] = 0.f; color[idx * 3 + 1] = 0.f; color[idx * 3 + 2] = 0.f;
}

__global__ __launch_bounds__(256) void scatter_active_kernel(const float* __restrict__ sigma_c, const float* __restrict__ color_c,
                                                             const int64_t* __restrict__ active_idx, int64_t M, int64_t NS,
                                                             float* __restrict__ sigma, float* __restrict__ color) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= M) return;
  const int64_t idx = active_idx[j];
  if (idx < 0 || idx >= NS) return;
  sigma[idx] = sigma_c[j];
  color[idx * 3 + 0] = color_c[j * 3 + 0]; color[idx * 3 + 1] = color_c[j * 3 + 1]; color[idx * 3 + 2] = color_c[j * 3 + 2];
}

// the number of elements of the ascending run zs[0..S) that are < v (strict) or <= v
__device__ __forceinline__ int count_below(const float* zs, int S, float v, bool or_equal) {
  int lo = 0, hi = S;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const float m = zs[mid];
    if (or_equal ? (m <= v) : (m < v)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One wave (= one workgroup) per pixel.  LDS: zin | occ (later: term) | order, KMAX * S entries each.
__global__ __launch_bounds__(64) void composite_kernel(const float* __restrict__ sigma, const float* __restrict__ color,
                                                       const float* __restrict__ z, const int* __restrict__ pix_segs,
                                                       const int* __restrict__ seg_entity, const int* __restrict__ entity_inst,
                                                       int64_t P, int S, float thr, float* __restrict__ rgb_out,
                                                       float* __restrict__ depth_out, float* __restrict__ opa_out,
                                                       float* __restrict__ var_out, float* __restrict__ mass_out,
                                                       int* __restrict__ inst_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int cap = KMAX * S;
  float* zin = reinterpret_cast<float*>(smem);
  float* occ = zin + cap;
  unsigned short* order = reinterpret_cast<unsigned short*>(occ + cap);
  const int lane = threadIdx.x;
  const int64_t p = blockIdx.x;
  int segs[KMAX];
  int K = 0;
#pragma unroll
  for (int j = 0; j < KMAX; ++j) { segs[j] = pix_segs[p * KMAX + j]; if (segs[j] >= 0 && K == j) K = j + 1; }
  if (K == 0) {
    if (lane == 0) {
      rgb_out[p * 3 + 0] = 0.f; rgb_out[p * 3 + 1] = 0.f; rgb_out[p * 3 + 2] = 0.f;
      depth_out[p] = 0.f; opa_out[p] = 0.f; var_out[p] = 0.f; inst_out[p] = -1;
    }
    if (lane < KMAX) mass_out[p * KMAX + lane] = 0.f;
    return;
  }
  const int n = K * S;
  // stage: z and occupancy of every sample, segment after segment
  for (int idx = lane; idx < n; idx += 64) {
    const int k = idx / S, i = idx - k * S;
    int sg = segs[0];
#pragma unroll
    for (int j = 1; j < KMAX; ++j) if (j == k) sg = segs[j];
    const int64_t g = (int64_t)sg * S + i;
    zin[idx] = z[g];
    occ[idx] = cnr_rl::sigmoid_exact(sigma[g]);
  }
  __syncthreads();
  // merged rank by (z, segment, sample): own index plus a binary search in every other segment
  for (int idx = lane; idx < n; idx += 64) {
    const int k = idx / S, i = idx - k * S;
    const float v = zin[idx];
    int r = i;
    for (int k2 = 0; k2 < K; ++k2)
      if (k2 != k) r += count_below(zin + k2 * S, S, v, k2 < k);
    order[r] = (unsigned short)idx;
  }
  __syncthreads();
  // transmittance: per-lane serial products over c consecutive ranks (c odd: conflict-free LDS stride), one exclusive scan
  int c = (n + 63) / 64;
  c |= 1;
  const int r0 = lane * c;
  float prod = 1.0f;
  for (int j = 0; j < c; ++j) {
    const int r = r0 + j;
    if (r < n) prod *= 1.0f - occ[min((int)order[r], n - 1)] + 1e-10f;
  }
  float incl = prod;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float q = __shfl_up(incl, o, 64);
    if (lane >= o) incl *= q;
  }
  float T = __shfl_up(incl, 1, 64);
  if (lane == 0) T = 1.0f;
  for (int j = 0; j < c; ++j) {
    const int r = r0 + j;
    if (r < n) {
      const int idx = min((int)order[r], n - 1);      // (a rank is unique when every segment's z ascends, as documented)
      const float oc = occ[idx];
      occ[idx] = oc * T;                   // term, back at the sample's own place
      T *= 1.0f - oc + 1e-10f;
    }
  }
  __syncthreads();
  // sums in source order: coalesced colour loads, one wave reduction per output
  float so = 0.f, sd = 0.f, sr = 0.f, sg_ = 0.f, sb = 0.f;
  float best = -1.0f;
  int best_k = 0;
  for (int k = 0; k < K; ++k) {
    int sg = segs[0];
#pragma unroll
    for (int j = 1; j < KMAX; ++j) if (j == k) sg = segs[j];
    float m = 0.f;
    for (int i = lane; i < S; i += 64) {
      const float term = occ[k * S + i];
      const float* cp = color + ((int64_t)sg * S + i) * 3;
      m += term;
      sd += term * zin[k * S + i];
      sr += term * cp[0]; sg_ += term * cp[1]; sb += term * cp[2];
    }
    m = cnr::wave_sum(m);
    so += m;
    if (m > best) { best = m; best_k = k; }
    if (lane == 0) mass_out[p * KMAX + k] = m;
  }
  if (lane == 0) for (int k = K; k < KMAX; ++k) mass_out[p * KMAX + k] = 0.f;
  sd = cnr::wave_sum(sd);
  sr = cnr::wave_sum(sr); sg_ = cnr::wave_sum(sg_); sb = cnr::wave_sum(sb);
  float sv = 0.f;
  for (int idx = lane; idx < n; idx += 64) { const float dz = zin[idx] - sd; sv += occ[idx] * dz * dz; }
  sv = cnr::wave_sum(sv);
  if (lane == 0) {
    int sgb = segs[0];
#pragma unroll
    for (int j = 1; j < KMAX; ++j) if (j == best_k) sgb = segs[j];
    rgb_out[p * 3 + 0] = sr; rgb_out[p * 3 + 1] = sg_; rgb_out[p * 3 + 2] = sb;
    depth_out[p] = sd; opa_out[p] = so; var_out[p] = sv;
    inst_out[p] = so >= thr ? entity_inst[seg_entity[sgb]] : -1;
  }
}

// ---- surface normals -------------------------------------------------------------------------------
// The winning segment of a pixel by composite_kernel's rule: the largest mass of its pix_segs row, the earlier one among equals;
// none when the row is empty or the pixel is not opaque enough.  -> the entity, or -1
__device__ __forceinline__ int surface_entity(const float* __restrict__ mass, const int* __restrict__ pix_segs,
                                              const int* __restrict__ seg_entity, const float* __restrict__ opacity, float thr,
                                              int64_t p) {
  float best = -1.0f;
  int best_seg = pix_segs[p * KMAX];                      // (the first one when no mass compares above -1, as there)
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    const int sg = pix_segs[p * KMAX + j];
    if (sg < 0) break;
    const float m = mass[p * KMAX + j];
    if (m > best) { best = m; best_seg = sg; }
  }
  if (best_seg < 0 || !(opacity[p] >= thr)) return -1;
  return seg_entity[best_seg];
}

// per wave of 64 pixels and field run: the number of pixels whose surface lies in an entity of that run
__global__ __launch_bounds__(256) void surface_count_kernel(const float* __restrict__ mass, const int* __restrict__ pix_segs,
                                                            const int* __restrict__ seg_entity, const float* __restrict__ opacity,
                                                            float thr, const int* __restrict__ entity_run, int64_t P, int n_runs,
                                                            int* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = n_waves(P);
  const int64_t wv = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wv >= nw) return;
  const int64_t p = wv * 64 + lane;
  const int e = p < P ? surface_entity(mass, pix_segs, seg_entity, opacity, thr, p) : -1;
  const int run = e >= 0 ? entity_run[e] : -1;
  for (int r = 0; r < n_runs; ++r) {
    const unsigned long long m = __ballot(run == r);
    if (lane == 0) counts[(int64_t)r * nw + wv] = __popcll(m);
  }
}

// one block: exclusive scan of the (n_runs * nw) counts in (run, wave) order; run_offset (n_runs + 1)
__global__ __launch_bounds__(1024) void surface_scan_kernel(const int* __restrict__ counts, int64_t nw, int n_runs,
                                                            int64_t* __restrict__ offsets, int64_t* __restrict__ run_offset) {
  __shared__ int64_t part[cnr::SCAN_THREADS];
  const int t = threadIdx.x;
  cnr::scan_block_counts<1>(counts, nw * n_runs, offsets, run_offset + n_runs, part);
  __syncthreads();
  for (int r = t; r < n_runs; r += 1024) run_offset[r] = offsets[(int64_t)r * nw];
}

__global__ __launch_bounds__(256) void surface_emit_kernel(const float* __restrict__ T_wc, const float* __restrict__ dirs,
                                                           const float* __restrict__ to_field, const float* __restrict__ depth,
                                                           const float* __restrict__ opacity, float thr,
                                                           const float* __restrict__ mass, const int* __restrict__ pix_segs,
                                                           const int* __restrict__ seg_entity, const int* __restrict__ entity_run,
                                                           const int* __restrict__ entity_row, int64_t P, int n_runs,
                                                           const int64_t* __restrict__ offsets, int* __restrict__ surf_entity,
                                                           int* __restrict__ surf_slot, float* __restrict__ surf_pts,
                                                           float* __restrict__ list_pts, int* __restrict__ list_row) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = n_waves(P);
  const int64_t wv = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wv >= nw) return;
  const int64_t p = wv * 64 + lane;
  const bool live = p < P;
  const int e = live ? surface_entity(mass, pix_segs, seg_entity, opacity, thr, p) : -1;
  const int run = e >= 0 ? entity_run[e] : -1;
  const unsigned long long below = (1ull << lane) - 1ull;
  int64_t slot = -1;
  for (int r = 0; r < n_runs; ++r) {
    const unsigned long long m = __ballot(run == r);
    if (run == r) slot = offsets[(int64_t)r * nw + wv] + __popcll(m & below);
  }
  if (!live) return;
  float f[3] = {0.f, 0.f, 0.f};
  if (e >= 0 && slot >= 0 && slot < P) {
    // cnr_view_points' expressions at z = the rendered depth
    const Cam cam = load_cam(T_wc);
    const float z = depth[p];
    const float cx = z * dirs[p * 3 + 0], cy = z * dirs[p * 3 + 1], cz = z * dirs[p * 3 + 2];
    float w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = cam.r[k * 3 + 0] * cx + cam.r[k * 3 + 1] * cy + cam.r[k * 3 + 2] * cz + cam.t[k];
    affine_point(to_field + (int64_t)e * 12, w[0], w[1], w[2], f);
    list_pts[slot * 3 + 0] = f[0]; list_pts[slot * 3 + 1] = f[1]; list_pts[slot * 3 + 2] = f[2];
    list_row[slot] = entity_row[e];
  }
  surf_entity[p] = e;
  surf_slot[p] = (e >= 0 && slot >= 0 && slot < P) ? (int)slot : -1;
  surf_pts[p * 3 + 0] = f[0]; surf_pts[p * 3 + 1] = f[1]; surf_pts[p * 3 + 2] = f[2];
}

// n = -A^T g / |A^T g|, A = to_field[entity][:, :3], g = the field-frame gradient at the pixel's slot of the compact list
__global__ __launch_bounds__(256) void normals_kernel(const float* __restrict__ grad_c, const int* __restrict__ surf_slot,
                                                      const int* __restrict__ surf_entity, const float* __restrict__ to_field,
                                                      int64_t P, int64_t M, float* __restrict__ normal) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const int slot = surf_slot[p], e = surf_entity[p];
  float v[3] = {0.f, 0.f, 0.f};
  if (slot >= 0 && slot < M && e >= 0) {
    const float* A = to_field + (int64_t)e * 12;
    const float g0 = grad_c[(int64_t)slot * 3 + 0], g1 = grad_c[(int64_t)slot * 3 + 1], g2 = grad_c[(int64_t)slot * 3 + 2];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = -(A[0 * 4 + k] * g0 + A[1 * 4 + k] * g1 + A[2 * 4 + k] * g2);
    // scaled by the largest component first: the squares of a gradient of 1e-20 or 1e20 neither vanish nor overflow
    const float big = fmaxf(fabsf(v[0]), fmaxf(fabsf(v[1]), fabsf(v[2])));
    if (big > 0.0f && fabsf(v[0]) + fabsf(v[1]) + fabsf(v[2]) < INFINITY) {      // (false for a NaN or an infinite component)
      const float a = v[0] / big, b = v[1] / big, c = v[2] / big;
      const float len = sqrtf(a * a + b * b + c * c);
      v[0] = a / len; v[1] = b / len; v[2] = c / len;
    } else {
      v[0] = 0.f; v[1] = 0.f; v[2] = 0.f;
    }
  }
  normal[p * 3 + 0] = v[0]; normal[p * 3 + 1] = v[1]; normal[p * 3 + 2] = v[2];
}

}  // namespace

extern "C" int64_t cnr_view_surface_workspace_bytes(int64_t P, int n_runs) {
  if (P <= 0 || n_runs <= 0) return 0;
  return ws_counts_bytes(P, n_runs) + n_waves(P) * n_runs * 8;
}

extern "C" int cnr_view_surface_points(const float* T_wc, const float* dirs, const float* to_field, const float* depth,
                                       const float* opacity, float opacity_threshold, const float* mass, const int* pix_segs,
                                       const int* seg_entity, const int* entity_run, const int* entity_row, int64_t P, int n_runs,
                                       void* workspace, int64_t* run_offset, int* surf_entity, int* surf_slot, float* surf_pts,
                                       float* list_pts, int* list_row, void* stream) {
  if (!T_wc || !dirs || !to_field || !depth || !opacity || !mass || !pix_segs || !seg_entity || !entity_run || !entity_row ||
      !workspace || !run_offset || !surf_entity || !surf_slot || !surf_pts || !list_pts || !list_row || P <= 0 || n_runs <= 0)
    return CNR_E_ARG;
  if (P >= (1ll << 31) || n_runs > 32767) return CNR_E_SHAPE;
  const int64_t nw = n_waves(P);
  int* counts = static_cast<int*>(workspace);
  int64_t* offsets = reinterpret_cast<int64_t*>(static_cast<char*>(workspace) + ws_counts_bytes(P, n_runs));
  hipLaunchKernelGGL(surface_count_kernel, dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, (hipStream_t)stream, mass, pix_segs,
                     seg_entity, opacity, opacity_threshold, entity_run, P, n_runs, counts);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(surface_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, counts, nw, n_runs, offsets, run_offset);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(surface_emit_kernel, dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, (hipStream_t)stream, T_wc, dirs, to_field,
                     depth, opacity, opacity_threshold, mass, pix_segs, seg_entity, entity_run, entity_row, P, n_runs, offsets,
                     surf_entity, surf_slot, surf_pts, list_pts, list_row);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_view_normals(const float* grad_c, const int* surf_slot, const int* surf_entity, const float* to_field,
                                int64_t P, int64_t M, float* normal, void* stream) {
  if (!surf_slot || !surf_entity || !to_field || !normal || P <= 0 || M < 0 || (M > 0 && !grad_c)) return CNR_E_ARG;
  if ((P + 255) / 256 >= (1ll << 31)) return CNR_E_SHAPE;
  hipLaunchKernelGGL(normals_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, grad_c, surf_slot,
                     surf_entity, to_field, P, M, normal);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int64_t cnr_view_segments_workspace_bytes(int64_t P, int E) {
  if (P <= 0 || E <= 0) return 0;
  return ws_counts_bytes(P, E) + n_waves(P) * E * 8;
}

extern "C" int cnr_view_segments_count(const float* T_wc, const float* dirs, const float* to_box, int64_t P, int E, float zmin,
                                       float zmax, void* workspace, int64_t* entity_offset, int64_t* count_out,
                                       int64_t* overflow, void* stream) {
  if (!T_wc || !dirs || !to_box || !workspace || !entity_offset || !count_out || !overflow || P <= 0 || E <= 0)
    return CNR_E_ARG;
  if (P >= (1ll << 31) || E > 32767) return CNR_E_SHAPE;
  const int64_t nw = n_waves(P);
  int* counts = static_cast<int*>(workspace);
  int* over = counts + nw * E;
  int64_t* offsets = reinterpret_cast<int64_t*>(static_cast<char*>(workspace) + ws_counts_bytes(P, E));
  hipLaunchKernelGGL(segments_count_kernel, dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, (hipStream_t)stream, T_wc, dirs,
                     to_box, P, E, zmin, zmax, counts, over);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(segments_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, counts, over, nw, E, offsets,
                     entity_offset, count_out, overflow);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_view_segments_emit(const float* T_wc, const float* dirs, const float* to_box, int64_t P, int E, float zmin,
                                      float zmax, const void* workspace, int* seg_pixel, int* seg_entity, float* seg_z,
                                      int* pix_segs, void* stream) {
  if (!T_wc || !dirs || !to_box || !workspace || !pix_segs || P <= 0 || E <= 0) return CNR_E_ARG;
  if (P >= (1ll << 31) || E > 32767) return CNR_E_SHAPE;
  const int64_t nw = n_waves(P);
  const int64_t* offsets = reinterpret_cast<const int64_t*>(static_cast<const char*>(workspace) + ws_counts_bytes(P, E));
  hipLaunchKernelGGL(segments_emit_kernel, dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, (hipStream_t)stream, T_wc, dirs,
                     to_box, P, E, zmin, zmax, offsets, seg_pixel, seg_entity, seg_z, pix_segs);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_view_points(const float* T_wc, const float* dirs, const float* to_field, const int* seg_pixel,
                               const int* seg_entity, const float* seg_z, int64_t N, int S, float* z, float* pts,
                               void* stream) {
  if (!T_wc || !dirs || !to_field || !seg_pixel || !seg_entity || !seg_z || !z || !pts || N <= 0) return CNR_E_ARG;
  if (S < 1 || S > SMAX) return CNR_E_SHAPE;
  const int64_t blocks = (N * S + 255) / 256;
  if (blocks >= (1ll << 31)) return CNR_E_SHAPE;
  hipLaunchKernelGGL(points_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, T_wc, dirs, to_field,
                     seg_pixel, seg_entity, seg_z, N, S, z, pts);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_view_composite(const float* sigma, const float* color, const float* z, const int* pix_segs,
                                  const int* seg_entity, const int* entity_inst, int64_t P, int S, float opacity_threshold,
                                  float* rgb, float* depth, float* opacity, float* var, float* mass, int* instance,
                                  void* stream) {
  if (!sigma || !color || !z || !pix_segs || !seg_entity || !entity_inst || !rgb || !depth || !opacity || !var || !mass || !instance || P <= 0) return CNR_E_ARG;
  if (S < 1 || S > SMAX) return CNR_E_SHAPE;
  if (P >= (1ll << 31)) return CNR_E_SHAPE;
  const unsigned lds = (unsigned)(KMAX * S * 10);        // <= 10 KiB: z, occupancy / term (f32) and the merged order (u16)
  hipLaunchKernelGGL(composite_kernel, dim3((unsigned)P), dim3(64), lds, (hipStream_t)stream, sigma, color, z, pix_segs,
                     seg_entity, entity_inst, P, S, opacity_threshold, rgb, depth, opacity, var, mass, instance);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int64_t cnr_view_active_workspace_bytes(int64_t N, int S, int E) {
  if (N <= 0 || S < 1 || S > SMAX || E <= 0) return 0;
  return active_ws(nullptr, N * S, E).bytes;
}

extern "C" int cnr_view_active_count(const float* T_wc, const float* dirs, const float* to_box, const int* seg_pixel,
                                     const int* seg_entity, const float* seg_z, const int64_t* entity_offset, int64_t N, int S,
                                     int E, const int* grid_words, const int* entity_grid, int G, void* workspace,
                                     int64_t* active_offset, int64_t* count_out, void* stream) {
  if (!T_wc || !dirs || !to_box || !seg_pixel || !seg_entity || !seg_z || !entity_offset || !grid_words || !entity_grid ||
      !workspace || !active_offset || !count_out || N <= 0 || E <= 0)
    return CNR_E_ARG;
  if (S < 1 || S > SMAX || E > 32767 || G < 4 || G > 128 || G % 4 != 0) return CNR_E_SHAPE;
  const int64_t NS = N * S, nb = n_count_blocks(NS);
  if (nb >= (1ll << 31)) return CNR_E_SHAPE;
  const ActiveWs w = active_ws(workspace, NS, E);
  hipLaunchKernelGGL(active_count_kernel, dim3((unsigned)nb), dim3(ACT_WAVES * 64), 0, (hipStream_t)stream, T_wc, dirs, to_box,
                     seg_pixel, seg_entity, seg_z, NS, S, grid_words, entity_grid, G, w.mask, w.wave_local, w.blk_count);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(active_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, w, entity_offset, NS, S, E, active_offset,
                     count_out);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_view_active_emit(const float* T_wc, const float* dirs, const float* to_field, const int* seg_pixel,
                                    const int* seg_entity, const float* seg_z, int64_t N, int S, int E, const int* entity_row,
                                    const void* workspace, const int64_t* active_offset, int64_t M, float* z,
                                    int64_t* active_idx, float* pts_c, int* block_row, void* stream) {
  if (!T_wc || !dirs || !to_field || !seg_pixel || !seg_entity || !seg_z || !entity_row || !workspace || !active_offset || !z ||
      N <= 0 || E <= 0 || M < 0)
    return CNR_E_ARG;
  if (M > 0 && (!active_idx || !pts_c || !block_row)) return CNR_E_ARG;
  if (S < 1 || S > SMAX || E > 32767 || M % 64 != 0) return CNR_E_SHAPE;
  const int64_t NS = N * S;
  const int64_t threads = NS > (int64_t)E * 64 ? NS : (int64_t)E * 64;
  const int64_t blocks = (threads + 255) / 256;
  if (blocks >= (1ll << 31)) return CNR_E_SHAPE;
  const ActiveWs w = active_ws(const_cast<void*>(workspace), NS, E);
  hipLaunchKernelGGL(active_emit_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, T_wc, dirs, to_field,
                     seg_pixel, seg_entity, seg_z, NS, S, E, entity_row, w, active_offset, M, z, active_idx, pts_c, block_row);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_view_scatter_active(const float* sigma_c, const float* color_c, const int64_t* active_idx, int64_t M,
                                       int64_t NS, float* sigma, float* color, void* stream) {
  if (!sigma || !color || NS <= 0 || M < 0) return CNR_E_ARG;
  if (M > 0 && (!sigma_c || !color_c || !active_idx)) return CNR_E_ARG;
  if ((NS + 255) / 256 >= (1ll << 31) || (M + 255) / 256 >= (1ll << 31)) return CNR_E_SHAPE;
  hipLaunchKernelGGL(fill_empty_kernel, dim3((unsigned)((NS + 255) / 256)), dim3(256), 0, (hipStream_t)stream, NS, sigma, color);
  CNR_LAUNCH_CHECK();
  if (M > 0) {
    hipLaunchKernelGGL(scatter_active_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, sigma_c,
                       color_c, active_idx, M, NS, sigma, color);
    CNR_LAUNCH_CHECK();
  }
  return CNR_OK;
}
