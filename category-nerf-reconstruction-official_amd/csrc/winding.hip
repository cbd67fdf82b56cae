// Generalized winding number (metrics.winding_number, inside, signed_distance, volume_iou): the sum over all faces of a triangle
// mesh of the signed solid angle seen from every query, divided by 4 pi, brute force.  DESIGN.md §3.21 has the contract;
// tests/winding_cpu.py restates it in numpy float64.
//
// Every launch is deterministic: no atomics, faces added in index order within a chunk, chunks added in chunk order.
//   wn_partial   a 2-D grid of (query block, face chunk); the chunk's corners, widened to fp64, go through LDS a tile at a time
//                (every lane reads the same corner: a broadcast), each lane keeps WN_QPT queries in registers with their running sum.
//   wn_finish    the sum over chunks in chunk order, divided by 2 pi.
// Arithmetic: fp64 of the fp32 inputs, one IEEE rounding per operation (contraction off), difference first: A = a - q etc.;
// nothing is evaluated in absolute coordinates, so a translation that keeps the differences exact changes no bit.
// Per pair t = atan2(det, den) with det = A . (B x C), den = |A||B||C| + (A.B)|C| + (B.C)|A| + (C.A)|B| (Van Oosterom and
// Strackee: the solid angle is 2 t), and t = 0 when det == 0 exactly.
#include "cnr_common.h"
#include "geom_common.h"

#include <math.h>

#pragma clang fp contract(off)

using namespace cnr;

namespace {
constexpr int WN_BLOCK = 256;
constexpr int WN_QPT = 2;                                 // queries per lane
constexpr int WN_QBLK = WN_BLOCK * WN_QPT;                // queries per workgroup
constexpr int WN_TILE = 256;                              // faces per LDS tile (9 fp64 each: 18 KB)
constexpr int64_t WN_TARGET_WG = 2048;
constexpr double WN_TWO_PI = 6.283185307179586;

struct WnLayout {
  int64_t qblocks, chunks, chunk_len, part_stride, bytes;
};
// bytes = chunks * align256(8 nq): per chunk nq partial sums (f64)
inline WnLayout wn_layout(int64_t nq, int64_t F) {
  WnLayout L;
  L.qblocks = (nq + WN_QBLK - 1) / WN_QBLK;
  const int64_t tiles = (F + WN_TILE - 1) / WN_TILE;
  int64_t want = (WN_TARGET_WG + L.qblocks - 1) / L.qblocks;
  if (want > tiles) want = tiles;
  if (want < 1) want = 1;
  const int64_t tiles_per_chunk = (tiles + want - 1) / want;
  L.chunk_len = tiles_per_chunk * WN_TILE;
  L.chunks = (F + L.chunk_len - 1) / L.chunk_len;
  L.part_stride = align256(nq * 8);
  L.bytes = L.chunks * L.part_stride;
  return L;
}

__device__ __forceinline__ double wn_dot(double ux, double uy, double uz, double vx, double vy, double vz) {
  return (ux * vx + uy * vy) + uz * vz;
}

// t of one (query, face) pair; c: the face's corners a, b, c in fp64
__device__ __forceinline__ double wn_pair(double qx, double qy, double qz, const double* __restrict__ c) {
  const double ax = c[0] - qx, ay = c[1] - qy, az = c[2] - qz;
  const double bx = c[3] - qx, by = c[4] - qy, bz = c[5] - qz;
  const double cx = c[6] - qx, cy = c[7] - qy, cz = c[8] - qz;
  const double la = sqrt(wn_dot(ax, ay, az, ax, ay, az));
  const double lb = sqrt(wn_dot(bx, by, bz, bx, by, bz));
  const double lc = sqrt(wn_dot(cx, cy, cz, cx, cy, cz));
  const double xx = by * cz - bz * cy;
  const double xy = bz * cx - bx * cz;
  const double xz = bx * cy - by * cx;
  const double det = wn_dot(ax, ay, az, xx, xy, xz);
  const double ab = wn_dot(ax, ay, az, bx, by, bz);
  const double bc = wn_dot(bx, by, bz, cx, cy, cz);
  const double ca = wn_dot(cx, cy, cz, ax, ay, az);
  const double den = ((la * lb) * lc + ab * lc) + (bc * la + ca * lb);
  const double t = atan2(det, den);
  return det == 0.0 ? 0.0 : t;                            // the query in the face's plane: nothing, also where atan2 gives +-pi
}

__global__ __launch_bounds__(WN_BLOCK) void wn_partial_kernel(const float* __restrict__ q, int64_t nq,
                                                              const float* __restrict__ verts, const int* __restrict__ faces,
                                                              int64_t F, int64_t chunk_len, char* __restrict__ part,
                                                              int64_t part_stride) {
  __shared__ double s_c[WN_TILE * 9];
  const int t = threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.x * WN_QBLK;
  const int64_t c = blockIdx.y;
  const int64_t p0 = c * chunk_len;
  const int64_t p1 = p0 + chunk_len < F ? p0 + chunk_len : F;
  double qx[WN_QPT], qy[WN_QPT], qz[WN_QPT], s[WN_QPT];
#pragma unroll
  for (int k = 0; k < WN_QPT; ++k) {
    int64_t i = q0 + k * WN_BLOCK + t;
    i = i < nq ? i : nq - 1;                              // lanes past the end compute on a copy and store nothing
    qx[k] = (double)q[3 * i];
    qy[k] = (double)q[3 * i + 1];
    qz[k] = (double)q[3 * i + 2];
    s[k] = 0.0;
  }
  for (int64_t base = p0; base < p1; base += WN_TILE) {
    const int cnt = p1 - base < WN_TILE ? (int)(p1 - base) : WN_TILE;
    __syncthreads();
    if (t < cnt) {
      const int64_t f = base + t;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int64_t v = faces ? (int64_t)faces[3 * f + k] : 3 * f + k;
        s_c[9 * t + 3 * k] = (double)verts[3 * v];
        s_c[9 * t + 3 * k + 1] = (double)verts[3 * v + 1];
        s_c[9 * t + 3 * k + 2] = (double)verts[3 * v + 2];
      }
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      double cr[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) cr[k] = s_c[9 * j + k];
#pragma unroll
      for (int k = 0; k < WN_QPT; ++k) s[k] = s[k] + wn_pair(qx[k], qy[k], qz[k], cr);
    }
  }
  double* out = (double*)(part + c * part_stride);
#pragma unroll
  for (int k = 0; k < WN_QPT; ++k) {
    const int64_t i = q0 + k * WN_BLOCK + t;
    if (i < nq) out[i] = s[k];
  }
}

__global__ __launch_bounds__(256) void wn_finish_kernel(int64_t nq, const char* __restrict__ part, int64_t part_stride,
                                                        int64_t chunks, double* __restrict__ w_out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nq; i += (int64_t)gridDim.x * 256) {
    double s = ((const double*)part)[i];
    for (int64_t c = 1; c < chunks; ++c) s = s + ((const double*)(part + c * part_stride))[i];
    w_out[i] = s / WN_TWO_PI;
  }
}
}  // namespace

extern "C" int64_t cnr_winding_workspace_bytes(int64_t nq, int64_t F) {
  if (nq < 1 || F < 1 || F > 0x7fffffff) return CNR_E_SHAPE;
  return wn_layout(nq, F).bytes;
}

extern "C" int cnr_winding_number(const float* q, int64_t nq, const float* verts, const int* faces, int64_t F, double* w_out,
                                  void* workspace, void* stream) {
  if (!q || !verts || !w_out || !workspace) return CNR_E_ARG;
  if (nq < 1 || F < 1 || F > 0x7fffffff) return CNR_E_SHAPE;
  const WnLayout L = wn_layout(nq, F);
  if (L.qblocks > 0x7fffffff || L.chunks > 65535) return CNR_E_SHAPE;
  char* part = (char*)workspace;
  hipLaunchKernelGGL(wn_partial_kernel, dim3((unsigned)L.qblocks, (unsigned)L.chunks), dim3(WN_BLOCK), 0, (hipStream_t)stream, q,
                     nq, verts, faces, F, L.chunk_len, part, L.part_stride);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(wn_finish_kernel, dim3(grid_of(nq, 256, 4096)), dim3(256), 0, (hipStream_t)stream, nq, (const char*)part,
                     L.part_stride, L.chunks, w_out);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}
