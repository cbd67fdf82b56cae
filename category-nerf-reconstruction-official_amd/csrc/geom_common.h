// The deterministic "count -> scan -> emit" plumbing of the geometry kernels (mcubes, metric, pointcloud, tsdf, fpfh, view,
// frames, teaser), once: workspace alignment and grids, the wave / block / per-block-count prefix sums, the sorted cell list
// of cnr_radius_cell_keys, and the tiling constants of the exact nearest neighbour.  Include after
// cnr_common.h.
//
// Floating-point contraction: tsdf, fpfh, view, frames and teaser compile under `#pragma clang fp contract(off)`; metric,
// pointcloud and mcubes do not.  So nothing here may hold a floating-point expression whose rounding depends on contraction:
// the scans only add, and sq_dist spells its fused multiply-adds out around a single product.
#pragma once
#include "cnr_common.h"

namespace cnr {
// ---- host -----------------------------------------------------------------------------------------------------------------
inline int64_t align256(int64_t x) { return (x + 255) / 256 * 256; }

// workgroups of `block` threads that cover n items, at least 1 and at most cap (the kernels stride over the grid)
inline unsigned grid_of(int64_t n, int block, int64_t cap) {
  const int64_t b = (n + block - 1) / block;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// ---- prefix sums ----------------------------------------------------------------------------------------------------------
// exclusive prefix over the lanes below this one, and the wave total, of a per-lane count in [0, 1 << BITS): ballots and
// mbcnt over the bit planes
template <int BITS>
__device__ __forceinline__ int wave_prefix_bits(int c, int* total) {
  int pre = 0, tot = 0;
#pragma unroll
  for (int b = 0; b < BITS; ++b) {
    const uint64_t m = __ballot((c >> b) & 1);
    const int below = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    pre += below << b;
    tot += __popcll(m) << b;
  }
  *total = tot;
  return pre;
}

// from a lane's prefix inside its wave and the wave's total: the prefix inside the block of WAVES waves (the totals of the
// waves below go through s_wave[WAVES], one barrier), and the block's total
template <int WAVES>
__device__ __forceinline__ int block_prefix_waves(int pre, int wtot, int* s_wave, int* block_total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_wave[wave] = wtot;
  __syncthreads();
  int base = 0, all = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    base += w < wave ? s_wave[w] : 0;
    all += s_wave[w];
  }
  *block_total = all;
  return base + pre;
}

// Hillis-Steele inclusive scan over the block of K values per thread, stream k in s[k * BLOCK .. (k + 1) * BLOCK): a fixed
// order of additions, so a floating-point T scans the same way on every run.  s keeps the inclusive sums.
template <int BLOCK, int K, typename T>
__device__ __forceinline__ void block_scan_streams(const T (&v)[K], T* s) {
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < K; ++k) s[k * BLOCK + t] = v[k];
  __syncthreads();
  for (int d = 1; d < BLOCK; d <<= 1) {
    T a[K];
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = t >= d ? s[k * BLOCK + t - d] : T(0);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) s[k * BLOCK + t] += a[k];
    __syncthreads();
  }
}
// one value per thread -> this thread's inclusive sum
template <int BLOCK, typename T>
__device__ __forceinline__ T block_scan(T v, T* s) {
  const T one[1] = {v};
  block_scan_streams<BLOCK, 1>(one, s);
  return s[threadIdx.x];
}
// ... -> this thread's exclusive sum (of integers); *total = the block's sum
template <int BLOCK>
__device__ __forceinline__ int block_excl_scan(int v, int* s, int* total) {
  const int incl = block_scan<BLOCK>(v, s);
  *total = s[BLOCK - 1];
  return incl - v;
}

// One workgroup of SCAN_THREADS threads: exclusive offsets ofs[K b + k] of the n per-block counts counts[K b + k] of K
// interleaved streams, and the streams' totals (unless totals is NULL).  Each thread sums a contiguous run, the run sums are
// block-scanned in s[K * SCAN_THREADS] (which keeps them), then each thread walks its run again from the sum of the runs
// below -- s[t - 1], not s[t] - run: the same integer, but only the former is the same double.
constexpr int SCAN_THREADS = 1024;
template <int K, typename T, typename C>
__device__ __forceinline__ void scan_block_counts(const C* __restrict__ counts, int64_t n, T* __restrict__ ofs,
                                                  T* __restrict__ totals, T* s) {
  const int t = threadIdx.x;
  const int64_t per = (n + SCAN_THREADS - 1) / SCAN_THREADS;
  const int64_t b0 = t * per < n ? t * per : n, b1 = b0 + per < n ? b0 + per : n;
  T run[K];
#pragma unroll
  for (int k = 0; k < K; ++k) run[k] = T(0);
  for (int64_t b = b0; b < b1; ++b) {
#pragma unroll
    for (int k = 0; k < K; ++k) run[k] += counts[K * b + k];
  }
  block_scan_streams<SCAN_THREADS, K>(run, s);
  T o[K];
#pragma unroll
  for (int k = 0; k < K; ++k) o[k] = t > 0 ? s[k * SCAN_THREADS + t - 1] : T(0);
  for (int64_t b = b0; b < b1; ++b) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      ofs[K * b + k] = o[k];
      o[k] += counts[K * b + k];
    }
  }
  if (totals && t == SCAN_THREADS - 1) {
#pragma unroll
    for (int k = 0; k < K; ++k) totals[k] = s[k * SCAN_THREADS + t];
  }
}
// the launch of just that, <<<1, SCAN_THREADS>>> (static: every unit that includes this header gets its own, none exported)
template <int K, typename T, typename C>
static __global__ __launch_bounds__(SCAN_THREADS) void blocks_scan_kernel(const C* __restrict__ blk_counts, int64_t nblk,
                                                                          T* __restrict__ ofs, T* __restrict__ totals) {
  __shared__ T s[K * SCAN_THREADS];
  scan_block_counts<K>(blk_counts, nblk, ofs, totals, s);
}

// ---- sorted cell lists ----------------------------------------------------------------------------------------------------
// first index in the ascending cells[0 .. C) whose value is >= key
__device__ __forceinline__ int64_t lower_bound(const int64_t* __restrict__ cells, int64_t C, int64_t key) {
  int64_t lo = 0, hi = C;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (cells[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// a cell or unit key: three biased 21-bit indices in one int64 (x the most significant), so keys order as (x, y, z)
constexpr int AXIS_BITS = 21;
constexpr int64_t AXIS_BIAS = (int64_t)1 << (AXIS_BITS - 1);
constexpr int64_t AXIS_MASK = ((int64_t)1 << AXIS_BITS) - 1;
__device__ __forceinline__ int64_t pack_key(int64_t ix, int64_t iy, int64_t iz) {
  return ((ix + AXIS_BIAS) << (2 * AXIS_BITS)) | ((iy + AXIS_BIAS) << AXIS_BITS) | (iz + AXIS_BIAS);
}

// ---- exact nearest neighbour (cnr_nn_dist, cnr_nn_index, cnr_icp_step) ----------------------------------------------------
constexpr int NN_BLOCK = 256;
constexpr int NN_QPT = 8;                                 // queries per lane
constexpr int NN_QBLK = NN_BLOCK * NN_QPT;                // queries per workgroup
constexpr int NN_TILE = 256;                              // reference points per LDS tile (4 KB)
constexpr int64_t NN_TARGET_WG = 2048;                    // 8 workgroups per CU on 256 CUs

// the nr reference points in chunks of whole tiles, about NN_TARGET_WG workgroups over the `rows` (query blocks x candidates)
inline void nn_chunks(int64_t rows, int64_t nr, int64_t* chunk_len, int64_t* chunks) {
  const int64_t tiles = (nr + NN_TILE - 1) / NN_TILE;
  int64_t want = (NN_TARGET_WG + rows - 1) / rows;
  if (want > tiles) want = tiles;
  if (want < 1) want = 1;
  const int64_t tiles_per_chunk = (tiles + want - 1) / want;
  *chunk_len = tiles_per_chunk * NN_TILE;
  *chunks = (nr + *chunk_len - 1) / *chunk_len;
}

__device__ __forceinline__ float sq_dist(float qx, float qy, float qz, float4 p) {
  const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
  return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}
}  // namespace cnr
