// TEASER's FPFH mode (src/teaser_utils/helpers.py: extract_fpfh, find_correspondences): open3d's hybrid neighbour search, normal
// estimation, SPFH / FPFH descriptors and the exact nearest neighbour in descriptor space.  DESIGN.md §3.9 has the contract;
// tests/fpfh_cpu.py restates it in numpy.
//
//   cnr_hybrid_search     one wave per query point over the 27 cells around it (the cell tables of cnr_radius_cell_keys); the
//                         in-range candidates go through a per-wave LDS buffer that is cut back to the best max_nn by (d2, index)
//                         whenever it fills, so a neighbourhood of any size is exact.
//   cnr_estimate_normals  one lane per point: fp64 mean and covariance of its list in list order, cyclic Jacobi with a fixed
//                         number of sweeps, the eigenvector of the smallest eigenvalue turned away from the cloud's centroid.
//   cnr_spfh / cnr_fpfh   one lane per point: integer histograms of the pair features of its list; their 1 / d2 weighted sums.
//   cnr_feature_nn        one lane per query row, the reference rows in chunks over the grid's second axis and tiled through
//                         LDS: the exact argmin of the sequential fp32 sum of squared differences (no expanded square, no MFMA);
//                         the chunks' minima are merged in chunk order.
// No float atomics, every loop bounded, results bit-identical run to run.  Every fp64 (and, in cnr_feature_nn, fp32) product,
// sum and quotient is rounded on its own: no contraction in this file.
#include "cnr_common.h"
#include "geom_common.h"

#include <math.h>

#pragma clang fp contract(off)

// (not all of namespace cnr: cnr_feature_nn has tile constants of its own under the names of cnr_nn_dist's)
using cnr::align256;
using cnr::AXIS_BITS;
using cnr::AXIS_MASK;
using cnr::grid_of;
using cnr::lower_bound;

namespace {
constexpr int WAVE = 64;
constexpr int HS_MAX_NN = 128;
constexpr int HS_CAP = 512;                                // candidates a wave buffers before it cuts back: 6 KB of LDS
constexpr int HS_PER_LANE = HS_CAP / WAVE;
static_assert(HS_CAP >= HS_MAX_NN + WAVE && HS_CAP % WAVE == 0, "room for one batch of candidates after every cut");
constexpr int PT_BLOCK = 128;                              // per-point kernels
constexpr int NB = 11;                                     // bins per feature
constexpr int NF = 3 * NB;
constexpr int JACOBI_SWEEPS = 8;
constexpr int NN_BLOCK = 256;                              // queries per workgroup of cnr_feature_nn
constexpr int NN_TILE = 64;                                // reference rows per LDS tile
constexpr int NN_MAX_D = 64;

// ---- hybrid search -----------------------------------------------------------------------------------------------------
// (key, index) ascending: key = the bits of the non-negative double d2, which order like the doubles themselves
__device__ __forceinline__ bool before(uint64_t ka, int ia, uint64_t kb, int ib) { return ka < kb || (ka == kb && ia < ib); }

// The first min(M, K) of the buffer's M entries in (key, index) order, sorted, in its first slots.  Every lane ranks its (at
// most HS_PER_LANE) entries against all M by counting; the indices are distinct, so the ranks are a permutation.  All reads
// happen before the barrier, all writes after it.  -> the new count
__device__ __forceinline__ int cut_back(uint64_t* __restrict__ keys, int* __restrict__ ids, int M, int K, int lane) {
  uint64_t ke[HS_PER_LANE];
  int ie[HS_PER_LANE], rank[HS_PER_LANE];
  __syncthreads();
#pragma unroll
  for (int t = 0; t < HS_PER_LANE; ++t) {
    const int e = t * WAVE + lane;
    ke[t] = e < M ? keys[e] : ~(uint64_t)0;
    ie[t] = e < M ? ids[e] : 0x7fffffff;
    rank[t] = 0;
  }
  for (int j = 0; j < M; ++j) {
    const uint64_t kj = keys[j];
    const int ij = ids[j];
#pragma unroll
    for (int t = 0; t < HS_PER_LANE; ++t) rank[t] += before(kj, ij, ke[t], ie[t]) ? 1 : 0;
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < HS_PER_LANE; ++t) {
    const int e = t * WAVE + lane;
    if (e < M && rank[t] < K) {
      keys[rank[t]] = ke[t];
      ids[rank[t]] = ie[t];
    }
  }
  __syncthreads();
  return M < K ? M : K;
}

// One workgroup of one wave per query, the queries in cell order (neighbouring workgroups share cells).  The three cells
// (X, Y, cz - 1 .. cz + 1) are consecutive keys, so nine ranges of the sorted list cover the 27 cells.
__global__ __launch_bounds__(WAVE) void hybrid_search_kernel(const float* __restrict__ p, int64_t n, const int64_t* __restrict__ perm,
                                                             const int64_t* __restrict__ skeys, const int64_t* __restrict__ cells,
                                                             const int64_t* __restrict__ starts, int64_t C, double r, int K,
                                                             int* __restrict__ idx_out, double* __restrict__ d2_out,
                                                             int* __restrict__ count_out) {
  __shared__ uint64_t keys[HS_CAP];
  __shared__ int ids[HS_CAP];
  const int lane = (int)threadIdx.x;
  const uint64_t below = ((uint64_t)1 << lane) - 1;
  const double r2 = r * r;
  for (int64_t j = blockIdx.x; j < n; j += gridDim.x) {
    const int64_t i = perm[j], key = skeys[j];
    if (i < 0 || i >= n) continue;                          // (uniform: the whole wave reads the same entry)
    int cnt = 0;
    if (key >= 0) {
      const double x = (double)p[3 * i], y = (double)p[3 * i + 1], z = (double)p[3 * i + 2];
      const int64_t kx = (key >> (2 * AXIS_BITS)) & AXIS_MASK, ky = (key >> AXIS_BITS) & AXIS_MASK, kz = key & AXIS_MASK;
      const int64_t z0 = kz > 0 ? kz - 1 : 0, z1 = kz < AXIS_MASK ? kz + 1 : AXIS_MASK;
      bool bounded = false;                                 // once a cut has left K entries, the K-th bounds what may still enter
      uint64_t bound_key = 0;
      int bound_id = 0;
      for (int64_t X = kx - 1; X <= kx + 1; ++X) {
        if (X < 0 || X > AXIS_MASK) continue;
        for (int64_t Y = ky - 1; Y <= ky + 1; ++Y) {
          if (Y < 0 || Y > AXIS_MASK) continue;
          const int64_t row = (X << (2 * AXIS_BITS)) | (Y << AXIS_BITS);
          const int64_t c0 = lower_bound(cells, C, row | z0), c1 = lower_bound(cells, C, (row | z1) + 1);
          int64_t m1 = starts[c1];
          m1 = m1 < n ? m1 : n;
          for (int64_t m0 = starts[c0] > 0 ? starts[c0] : 0; m0 < m1; m0 += WAVE) {
            if (cnt + WAVE > HS_CAP) {
              cnt = cut_back(keys, ids, cnt, K, lane);
              if (cnt == K) {
                bounded = true;
                bound_key = keys[K - 1];
                bound_id = ids[K - 1];
              }
            }
            const int64_t m = m0 + lane;
            bool take = false;
            uint64_t kq = 0;
            int q = 0;
            if (m < m1) {
              const int64_t qq = perm[m];
              if (qq >= 0 && qq < n) {
                q = (int)qq;
                const double dx = x - (double)p[3 * qq], dy = y - (double)p[3 * qq + 1], dz = z - (double)p[3 * qq + 2];
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                kq = (uint64_t)__double_as_longlong(d2);
                take = d2 < r2 && (!bounded || before(kq, q, bound_key, bound_id));
              }
            }
            const uint64_t mask = __ballot(take);
            if (take) {
              const int at = cnt + __popcll(mask & below);
              keys[at] = kq;
              ids[at] = q;
            }
            cnt += __popcll(mask);
          }
        }
      }
      cnt = cut_back(keys, ids, cnt, K, lane);
    }
    for (int t = lane; t < K; t += WAVE) {
      idx_out[i * K + t] = t < cnt ? ids[t] : -1;
      d2_out[i * K + t] = t < cnt ? __longlong_as_double((long long)keys[t]) : 0.0;
    }
    if (lane == 0) count_out[i] = cnt;
    __syncthreads();                                        // the rows are out before the next query fills the buffer
  }
}

// ---- normals -----------------------------------------------------------------------------------------------------------
// One Jacobi rotation of the symmetric 3 x 3 matrix on the pair (p, q); r is the third index.  V's columns follow.
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p,
                                              double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  const double tp = t * apq;
  app = app - tp;
  aqq = aqq + tp;
  apq = 0.0;
  const double rp = c * arp - s * arq, rq = s * arp + c * arq;
  arp = rp;
  arq = rq;
  const double a0 = c * v0p - s * v0q, b0 = s * v0p + c * v0q;
  const double a1 = c * v1p - s * v1q, b1 = s * v1p + c * v1q;
  const double a2 = c * v2p - s * v2q, b2 = s * v2p + c * v2q;
  v0p = a0; v0q = b0; v1p = a1; v1q = b1; v2p = a2; v2q = b2;
}

__global__ __launch_bounds__(PT_BLOCK) void normals_kernel(const float* __restrict__ p, int64_t n, const int* __restrict__ idx,
                                                           const int* __restrict__ count, int K, double cx, double cy, double cz,
                                                           double* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * PT_BLOCK) {
    int k = count[i];
    k = k < 0 ? 0 : (k > K ? K : k);
    const int* __restrict__ row = idx + i * K;
    double nx = 0.0, ny = 0.0, nz = 1.0;
    bool listed = k >= 3;
    for (int t = 0; t < k; ++t) listed = listed && row[t] >= 0 && row[t] < n;
    if (listed) {
      double sx = 0.0, sy = 0.0, sz = 0.0;
      for (int t = 0; t < k; ++t) {
        const int64_t q = row[t];
        sx += (double)p[3 * q];
        sy += (double)p[3 * q + 1];
        sz += (double)p[3 * q + 2];
      }
      const double kd = (double)k;
      const double mx = sx / kd, my = sy / kd, mz = sz / kd;
      double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
      for (int t = 0; t < k; ++t) {
        const int64_t q = row[t];
        const double dx = (double)p[3 * q] - mx, dy = (double)p[3 * q + 1] - my, dz = (double)p[3 * q + 2] - mz;
        a00 += dx * dx; a01 += dx * dy; a02 += dx * dz;
        a11 += dy * dy; a12 += dy * dz; a22 += dz * dz;
      }
      a00 = a00 / kd; a01 = a01 / kd; a02 = a02 / kd; a11 = a11 / kd; a12 = a12 / kd; a22 = a22 / kd;
      double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
      for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
        jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);      // (0, 1), third 2
        jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);      // (0, 2), third 1
        jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);      // (1, 2), third 0
      }
      double ex = v00, ey = v10, ez = v20, l = a00;                                // the smallest eigenvalue, the first of equals
      if (a11 < l) { ex = v01; ey = v11; ez = v21; l = a11; }
      if (a22 < l) { ex = v02; ey = v12; ez = v22; l = a22; }
      const double len = sqrt((ex * ex + ey * ey) + ez * ez);
      nx = ex / len; ny = ey / len; nz = ez / len;
      const double dot = (nx * ((double)p[3 * i] - cx) + ny * ((double)p[3 * i + 1] - cy)) + nz * ((double)p[3 * i + 2] - cz);
      bool flip = dot < 0.0;
      if (dot == 0.0) {
        double big = nx;                                                           // the component of largest magnitude, the first of equals
        if (fabs(ny) > fabs(big)) big = ny;
        if (fabs(nz) > fabs(big)) big = nz;
        flip = big < 0.0;
      }
      if (flip) { nx = -nx; ny = -ny; nz = -nz; }
    }
    out[3 * i] = nx; out[3 * i + 1] = ny; out[3 * i + 2] = nz;
  }
}

// ---- SPFH --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int bin_of(double scaled) {
  const double f = floor(scaled);
  return f >= 10.0 ? 10 : (f >= 0.0 ? (int)f : 0);           // NaN -> 0
}

// The three bins of the pair feature of (p1, n1), (p2, n2), as DESIGN.md §3.9 states it operation by operation.
__device__ __forceinline__ void pair_bins(double p1x, double p1y, double p1z, double n1x, double n1y, double n1z, double p2x,
                                          double p2y, double p2z, double n2x, double n2y, double n2z, int& b0, int& b1, int& b2) {
  double f0 = 0.0, f1 = 0.0, f2 = 0.0;
  double dx = p2x - p1x, dy = p2y - p1y, dz = p2z - p1z;
  const double d = sqrt((dx * dx + dy * dy) + dz * dz);
  if (d != 0.0) {
    const double a1 = ((n1x * dx + n1y * dy) + n1z * dz) / d, a2 = ((n2x * dx + n2y * dy) + n2z * dz) / d;
    double g2;
    if (fabs(a1) < fabs(a2)) {                               // the point whose normal makes the smaller angle with the line is the source
      double t;
      t = n1x; n1x = n2x; n2x = t;
      t = n1y; n1y = n2y; n2y = t;
      t = n1z; n1z = n2z; n2z = t;
      dx = -dx; dy = -dy; dz = -dz;
      g2 = -a2;
    } else {
      g2 = a1;
    }
    double vx = dy * n1z - dz * n1y, vy = dz * n1x - dx * n1z, vz = dx * n1y - dy * n1x;
    const double vn = sqrt((vx * vx + vy * vy) + vz * vz);
    if (vn != 0.0) {
      vx = vx / vn; vy = vy / vn; vz = vz / vn;
      const double wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;
      f1 = (vx * n2x + vy * n2y) + vz * n2z;
      f0 = atan2((wx * n2x + wy * n2y) + wz * n2z, (n1x * n2x + n1y * n2y) + n1z * n2z);
      f2 = g2;
    }
  }
  b0 = bin_of((11.0 * (f0 + M_PI)) / (2.0 * M_PI));
  b1 = bin_of((11.0 * (f1 + 1.0)) * 0.5);
  b2 = bin_of((11.0 * (f2 + 1.0)) * 0.5);
}

// The histograms live in LDS, bin major (lane t owns column t: no bank conflicts, no dynamically indexed registers).
__global__ __launch_bounds__(PT_BLOCK) void spfh_kernel(const float* __restrict__ p, const double* __restrict__ nrm, int64_t n,
                                                        const int* __restrict__ idx, const int* __restrict__ count, int K,
                                                        double* __restrict__ out) {
  __shared__ int hist[NF][PT_BLOCK];
  const int t = (int)threadIdx.x;
  for (int64_t i = (int64_t)blockIdx.x * PT_BLOCK + t; i < n; i += (int64_t)gridDim.x * PT_BLOCK) {
    for (int b = 0; b < NF; ++b) hist[b][t] = 0;
    int k = count[i];
    k = k < 0 ? 0 : (k > K ? K : k);
    const int* __restrict__ row = idx + i * K;
    const double px = (double)p[3 * i], py = (double)p[3 * i + 1], pz = (double)p[3 * i + 2];
    const double nx = nrm[3 * i], ny = nrm[3 * i + 1], nz = nrm[3 * i + 2];
    for (int s = 1; s < k; ++s) {
      const int64_t q = row[s];
      if (q < 0 || q >= n) continue;
      int b0, b1, b2;
      pair_bins(px, py, pz, nx, ny, nz, (double)p[3 * q], (double)p[3 * q + 1], (double)p[3 * q + 2], nrm[3 * q], nrm[3 * q + 1],
                nrm[3 * q + 2], b0, b1, b2);
      hist[b0][t] += 1;
      hist[NB + b1][t] += 1;
      hist[2 * NB + b2][t] += 1;
    }
    const double inc = k > 1 ? 100.0 / (double)(k - 1) : 0.0;
    for (int b = 0; b < NF; ++b) out[i * NF + b] = (double)hist[b][t] * inc;
  }
}

// ---- FPFH --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PT_BLOCK) void fpfh_kernel(const double* __restrict__ spfh, int64_t n, const int* __restrict__ idx,
                                                        const double* __restrict__ d2, const int* __restrict__ count, int K,
                                                        double* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * PT_BLOCK) {
    int k = count[i];
    k = k < 0 ? 0 : (k > K ? K : k);
    double acc[NF], sum[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[j] = 0.0;
    for (int s = 1; s < k; ++s) {
      const int64_t q = idx[i * K + s];
      const double dd = d2[i * K + s];
      if (q < 0 || q >= n || dd == 0.0) continue;
      const double* __restrict__ src = spfh + q * NF;
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const double val = src[j] / dd;
        acc[j] += val;
        sum[j / NB] += val;
      }
    }
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      double v = acc[j];
      if (sum[j / NB] != 0.0) v = v * (100.0 / sum[j / NB]);
      out[i * NF + j] = k > 1 ? v + spfh[i * NF + j] : 0.0;
    }
  }
}

// ---- nearest neighbour in descriptor space ---------------------------------------------------------------------------------
// DP = D padded with zero columns to a multiple of 4: (0 - 0)^2 = 0 leaves a sum of non-negative terms as it is, bit for bit.
// Workgroup (x, y) takes 256 queries and the y-th chunk of reference rows (a multiple of the tile), so a small nq still fills
// the device; with more than one chunk the per-chunk minima go to the workspace and nn_merge_kernel takes them in chunk order
// with a strict <, which keeps the lowest index among equals: the result does not depend on the number of chunks.
template <int DP>
__global__ __launch_bounds__(NN_BLOCK) void feature_nn_kernel(const float* __restrict__ q, int64_t nq, const float* __restrict__ p,
                                                              int64_t nr, int D, int64_t chunk_rows, int* __restrict__ index_out,
                                                              float* __restrict__ dist_out) {
  __shared__ float tile[NN_TILE][DP];
  const int64_t i = (int64_t)blockIdx.x * NN_BLOCK + threadIdx.x;
  const int64_t iq = i < nq ? i : nq - 1;                    // idle lanes repeat the last row: every lane reaches the barriers
  const int64_t r_begin = (int64_t)blockIdx.y * chunk_rows;
  const int64_t r_end = r_begin + chunk_rows < nr ? r_begin + chunk_rows : nr;
  float qv[DP];
#pragma unroll
  for (int j = 0; j < DP; ++j) qv[j] = j < D ? q[iq * D + j] : 0.0f;
  float best = 0.0f;
  int best_at = (int)r_begin;
  for (int64_t r0 = r_begin; r0 < r_end; r0 += NN_TILE) {
    const int rows = (int)(r_end - r0 < NN_TILE ? r_end - r0 : NN_TILE);
    __syncthreads();
    for (int e = (int)threadIdx.x; e < NN_TILE * DP; e += NN_BLOCK) {
      const int rr = e / DP, j = e - rr * DP;
      tile[rr][j] = (rr < rows && j < D) ? p[(r0 + rr) * D + j] : 0.0f;
    }
    __syncthreads();
    for (int rr = 0; rr < rows; ++rr) {
      float s = 0.0f;
#pragma unroll
      for (int j = 0; j < DP; ++j) {
        const float d = qv[j] - tile[rr][j];
        s = s + d * d;
      }
      if ((r0 == r_begin && rr == 0) || s < best) {          // the lowest index among equals
        best = s;
        best_at = (int)(r0 + rr);
      }
    }
  }
  if (i < nq) {
    index_out[(int64_t)blockIdx.y * nq + i] = best_at;
    dist_out[(int64_t)blockIdx.y * nq + i] = best;
  }
}

__global__ __launch_bounds__(NN_BLOCK) void nn_merge_kernel(const int* __restrict__ part_index, const float* __restrict__ part_dist,
                                                            int64_t nq, int chunks, int* __restrict__ index_out,
                                                            float* __restrict__ dist_out) {
  const int64_t i = (int64_t)blockIdx.x * NN_BLOCK + threadIdx.x;
  if (i >= nq) return;
  float best = part_dist[i];
  int best_at = part_index[i];
  for (int c = 1; c < chunks; ++c) {
    const float d = part_dist[(int64_t)c * nq + i];
    if (d < best) {
      best = d;
      best_at = part_index[(int64_t)c * nq + i];
    }
  }
  index_out[i] = best_at;
  dist_out[i] = best;
}

// About NN_TARGET_WORKGROUPS workgroups in all: chunks of whole tiles, none empty, at most 65535.
constexpr int64_t NN_TARGET_WORKGROUPS = 1024;
struct NnPlan { int64_t qblocks, chunk_rows; int chunks; int64_t off_dist, bytes; };
inline NnPlan nn_plan(int64_t nq, int64_t nr) {
  NnPlan P;
  P.qblocks = (nq + NN_BLOCK - 1) / NN_BLOCK;
  const int64_t tiles = (nr + NN_TILE - 1) / NN_TILE;
  int64_t want = NN_TARGET_WORKGROUPS / P.qblocks;
  want = want < 1 ? 1 : (want > tiles ? tiles : (want > 65535 ? 65535 : want));
  P.chunk_rows = (tiles + want - 1) / want * NN_TILE;
  P.chunks = (int)((nr + P.chunk_rows - 1) / P.chunk_rows);
  P.off_dist = align256(P.chunks * nq * (int64_t)sizeof(int));
  P.bytes = P.off_dist + P.chunks * nq * (int64_t)sizeof(float);
  return P;
}

template <int DP>
int launch_feature_nn(const float* q, int64_t nq, const float* p, int64_t nr, int D, int* index_out, float* dist_out,
                      void* workspace, hipStream_t stream) {
  const NnPlan P = nn_plan(nq, nr);
  int* part_index = P.chunks > 1 ? (int*)workspace : index_out;
  float* part_dist = P.chunks > 1 ? (float*)((char*)workspace + P.off_dist) : dist_out;
  hipLaunchKernelGGL(feature_nn_kernel<DP>, dim3((unsigned)P.qblocks, (unsigned)P.chunks), dim3(NN_BLOCK), 0, stream, q, nq, p, nr, D,
                     P.chunk_rows, part_index, part_dist);
  CNR_LAUNCH_CHECK();
  if (P.chunks > 1) {
    hipLaunchKernelGGL(nn_merge_kernel, dim3((unsigned)P.qblocks), dim3(NN_BLOCK), 0, stream, (const int*)part_index,
                       (const float*)part_dist, nq, P.chunks, index_out, dist_out);
    CNR_LAUNCH_CHECK();
  }
  return CNR_OK;
}

inline bool nn_ok(int64_t nq, int64_t nr) { return nq >= 1 && nr >= 1 && nr <= 0x7fffffff && nq <= (int64_t)0x7fffffff; }
inline bool lists_ok(int64_t n, int max_nn) { return n >= 1 && n <= 0x7fffffff && max_nn >= 1 && max_nn <= HS_MAX_NN; }
}  // namespace

// ---- entry points ------------------------------------------------------------------------------------------------------
extern "C" int cnr_hybrid_search_capacity(void) { return HS_CAP; }

extern "C" int cnr_hybrid_search(const float* points, int64_t n, const int64_t* perm, const int64_t* sorted_keys,
                                 const int64_t* cells, const int64_t* starts, int64_t C, double radius, int max_nn, int* idx,
                                 double* d2, int* count, void* stream) {
  if (!points || !perm || !sorted_keys || !cells || !starts || !idx || !d2 || !count) return CNR_E_ARG;
  if (!lists_ok(n, max_nn) || C < 1 || C > n || !(radius > 0.0)) return CNR_E_SHAPE;
  hipLaunchKernelGGL(hybrid_search_kernel, dim3(grid_of(n, 1, 1 << 20)), dim3(WAVE), 0, (hipStream_t)stream, points, n, perm,
                     sorted_keys, cells, starts, C, radius, max_nn, idx, d2, count);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_estimate_normals(const float* points, int64_t n, const int* idx, const int* count, int max_nn, double cx,
                                    double cy, double cz, double* normals, void* stream) {
  if (!points || !idx || !count || !normals) return CNR_E_ARG;
  if (!lists_ok(n, max_nn)) return CNR_E_SHAPE;
  hipLaunchKernelGGL(normals_kernel, dim3(grid_of(n, PT_BLOCK, 65536)), dim3(PT_BLOCK), 0, (hipStream_t)stream, points, n, idx, count,
                     max_nn, cx, cy, cz, normals);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_spfh(const float* points, const double* normals, int64_t n, const int* idx, const int* count, int max_nn,
                        double* spfh, void* stream) {
  if (!points || !normals || !idx || !count || !spfh) return CNR_E_ARG;
  if (!lists_ok(n, max_nn)) return CNR_E_SHAPE;
  hipLaunchKernelGGL(spfh_kernel, dim3(grid_of(n, PT_BLOCK, 65536)), dim3(PT_BLOCK), 0, (hipStream_t)stream, points, normals, n, idx,
                     count, max_nn, spfh);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_fpfh(const double* spfh, int64_t n, const int* idx, const double* d2, const int* count, int max_nn,
                        double* fpfh, void* stream) {
  if (!spfh || !idx || !d2 || !count || !fpfh) return CNR_E_ARG;
  if (!lists_ok(n, max_nn)) return CNR_E_SHAPE;
  hipLaunchKernelGGL(fpfh_kernel, dim3(grid_of(n, PT_BLOCK, 65536)), dim3(PT_BLOCK), 0, (hipStream_t)stream, spfh, n, idx, d2, count,
                     max_nn, fpfh);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int64_t cnr_feature_nn_workspace_bytes(int64_t nq, int64_t nr) {
  if (!nn_ok(nq, nr)) return CNR_E_SHAPE;
  return nn_plan(nq, nr).bytes;
}

extern "C" int cnr_feature_nn(const float* q, int64_t nq, const float* p, int64_t nr, int D, int* index_out, float* dist_out,
                              void* workspace, void* stream) {
  if (!q || !p || !index_out || !dist_out || !workspace) return CNR_E_ARG;
  if (!nn_ok(nq, nr) || D < 1 || D > NN_MAX_D) return CNR_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  if (D <= 4) return launch_feature_nn<4>(q, nq, p, nr, D, index_out, dist_out, workspace, s);
  if (D <= 16) return launch_feature_nn<16>(q, nq, p, nr, D, index_out, dist_out, workspace, s);
  if (D <= 36) return launch_feature_nn<36>(q, nq, p, nr, D, index_out, dist_out, workspace, s);
  return launch_feature_nn<64>(q, nq, p, nr, D, index_out, dist_out, workspace, s);
}
