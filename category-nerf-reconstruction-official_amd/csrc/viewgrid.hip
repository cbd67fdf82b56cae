// Occupancy grids of the scene view renderer's empty-space skipping: one bit per cell of a G^3 grid
// over an entity's box [-1,1]^3, cell (ix, iy, iz) at linear index l = (ix G + iy) G + iz, bit l & 31 of word l >> 5.
//
//   cnr_view_grid_cells    a (D,D,D) occupancy lattice, D = G sub + 1, reduced to the cells: a cell owns the lattice indices
//                          [i sub, (i + 1) sub] of every axis, faces included, and is set iff one owned value is not below tau
//   cnr_view_grid_dilate   every cell within Chebyshev distance `radius` of a set cell, clamped at the faces
//
// One lane per cell, 64 consecutive cells (one row segment along z, or several whole rows when G < 64) per wave: the wave's
// ballot is the 64-cell mask, which lanes 0 and 1 store as two words.  G is a multiple of 4, so G^3 is a multiple of 64 and no
// wave is partial.
#include "cnr_common.h"

namespace {

__device__ __forceinline__ void store_mask(int* __restrict__ words, int64_t wave, unsigned long long m) {
  const int lane = threadIdx.x & 63;
  if (lane < 2) words[wave * 2 + lane] = (int)(unsigned)(lane == 0 ? m : (m >> 32));
}

__global__ __launch_bounds__(256) void grid_cells_kernel(const float* __restrict__ occ, int G, int sub, float tau,
                                                         int* __restrict__ words) {
  const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t cells = (int64_t)G * G * G;
  if (l - (threadIdx.x & 63) >= cells) return;             // whole waves only: cells is a multiple of 64
  const int D = G * sub + 1;
  const int iz = (int)(l % G), iy = (int)((l / G) % G), ix = (int)(l / ((int64_t)G * G));
  bool set = false;
  for (int a = 0; a <= sub; ++a)
    for (int b = 0; b <= sub; ++b) {
      const float* row = occ + ((int64_t)(ix * sub + a) * D + (iy * sub + b)) * D + iz * sub;
      for (int c = 0; c <= sub; ++c) set = set || !(row[c] < tau);
    }
  store_mask(words, l >> 6, __ballot(set));
}

__global__ __launch_bounds__(256) void grid_dilate_kernel(const int* __restrict__ in, int G, int radius, int* __restrict__ out) {
  const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t cells = (int64_t)G * G * G;
  if (l - (threadIdx.x & 63) >= cells) return;
  const int iz = (int)(l % G), iy = (int)((l / G) % G), ix = (int)(l / ((int64_t)G * G));
  const int x0 = max(ix - radius, 0), x1 = min(ix + radius, G - 1);
  const int y0 = max(iy - radius, 0), y1 = min(iy + radius, G - 1);
  const int z0 = max(iz - radius, 0), z1 = min(iz + radius, G - 1);          // clamped: a row's end does not reach the next row
  bool set = false;
  for (int x = x0; x <= x1; ++x)
    for (int y = y0; y <= y1; ++y)
      for (int z = z0; z <= z1; ++z) {
        const int64_t c = ((int64_t)x * G + y) * G + z;
        set = set || ((in[c >> 5] >> (int)(c & 31)) & 1);
      }
  store_mask(out, l >> 6, __ballot(set));
}

bool grid_ok(int G) { return G >= 4 && G <= 128 && G % 4 == 0; }

}  // namespace

extern "C" int cnr_view_grid_cells(const float* occ, int G, int sub, float tau, int* words, void* stream) {
  if (!occ || !words) return CNR_E_ARG;
  if (!grid_ok(G) || sub < 1 || sub > 4) return CNR_E_SHAPE;
  const int64_t cells = (int64_t)G * G * G;
  hipLaunchKernelGGL(grid_cells_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, (hipStream_t)stream, occ, G, sub,
                     tau, words);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_view_grid_dilate(const int* words_in, int G, int radius, int* words_out, void* stream) {
  if (!words_in || !words_out || words_in == words_out) return CNR_E_ARG;
  if (!grid_ok(G) || radius < 0 || radius > 2) return CNR_E_SHAPE;
  const int64_t cells = (int64_t)G * G * G;
  hipLaunchKernelGGL(grid_dilate_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, (hipStream_t)stream, words_in, G,
                     radius, words_out);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}
