// Category registration on point clouds (src/category_registration.py, src/utils.py:189-366): unprojection of one instance's
// pixels, open3d's voxel down-sample, exact nearest neighbour WITH its index, and the batched point-to-point ICP step (sums
// for Kabsch, the rigid update, open3d's convergence test).  DESIGN.md §3.9 has the contract.
//
// As in csrc/metric.hip every launch is deterministic: no float atomics, fixed reduction orders, reduce-then-scan for every
// variable-size output, so two runs on the same inputs are bit-identical.
//   cnr_unproject_count / _emit   pixels of obj_mask == inst_id with 0 < depth <= 8 in the MEMORY order of the (W,H) frame arrays
//                                 (i = u H + v); the point in fp64 from the fp32 depth, rounded once.
//   cnr_points_min                per-axis fp32 minimum (exact, order-free).
//   cnr_voxel_keys                floor((p - (min - voxel / 2)) / voxel) per axis in fp64, packed 21 bits per axis; -1 outside.
//   cnr_voxel_segments_count/_emit  runs of equal sorted keys; one lane per run sums its points in fp64 in input order.
//   cnr_nn_index / cnr_icp_step   cnr_nn_dist's tiling (a target tile in LDS, 8 queries per lane in registers) with the index
//                                 carried beside the minimum (strict <, ascending index: ties go to the lowest index), a third
//                                 grid axis over B candidate transforms, then the 17 sums per candidate in fp64.
//   cnr_icp_update                per candidate: Horn's quaternion (largest eigenvector of a symmetric 4x4 by cyclic Jacobi) =
//                                 the proper rotation maximising tr(R H), which is V diag(1,1,det(V U^T)) U^T of H = U S V^T.
#include "cnr_common.h"
#include "geom_common.h"

#include <math.h>

using namespace cnr;

namespace {
constexpr int PC_BLOCK = 256;
constexpr int PC_ITEMS = 4;
constexpr int PC_PER_BLOCK = PC_BLOCK * PC_ITEMS;
constexpr float DEPTH_TRUNC = 8.0f;                       // unproject_colored_pointcloud's depth_trunc

// compaction workspace: per-block counts (int), then their exclusive offsets (int64)
struct CompactLayout {
  int64_t nblk, off_ofs, bytes;
};
inline CompactLayout compact_layout(int64_t n) {
  CompactLayout L;
  L.nblk = (n + PC_PER_BLOCK - 1) / PC_PER_BLOCK;
  L.off_ofs = align256(L.nblk * 4);
  L.bytes = L.off_ofs + align256(L.nblk * 8);
  return L;
}

// ---- unprojection ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool pixel_kept(const float* __restrict__ depth, const int* __restrict__ obj_mask, int64_t i,
                                           int inst_id) {
  const float z = depth[i];
  return obj_mask[i] == inst_id && z > 0.0f && z <= DEPTH_TRUNC;
}

__global__ __launch_bounds__(PC_BLOCK) void unproject_count_kernel(const float* __restrict__ depth,
                                                                   const int* __restrict__ obj_mask, int64_t npix, int inst_id,
                                                                   int* __restrict__ blk_counts) {
  __shared__ int s[PC_BLOCK];
  const int64_t i0 = (int64_t)blockIdx.x * PC_PER_BLOCK + threadIdx.x * PC_ITEMS;
  int c = 0;
#pragma unroll
  for (int k = 0; k < PC_ITEMS; ++k)
    if (i0 + k < npix && pixel_kept(depth, obj_mask, i0 + k, inst_id)) ++c;
  int total;
  block_excl_scan<PC_BLOCK>(c, s, &total);
  if (threadIdx.x == 0) blk_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(PC_BLOCK) void unproject_emit_kernel(const float* __restrict__ depth,
                                                                  const int* __restrict__ obj_mask,
                                                                  const uint8_t* __restrict__ image, int64_t npix, int H,
                                                                  int inst_id, double fx, double fy, double cx, double cy,
                                                                  const double* __restrict__ T, const int64_t* __restrict__ ofs,
                                                                  float* __restrict__ points, float* __restrict__ colors) {
  __shared__ int s[PC_BLOCK];
  const int64_t i0 = (int64_t)blockIdx.x * PC_PER_BLOCK + threadIdx.x * PC_ITEMS;
  bool keep[PC_ITEMS];
  int c = 0;
#pragma unroll
  for (int k = 0; k < PC_ITEMS; ++k) {
    keep[k] = i0 + k < npix && pixel_kept(depth, obj_mask, i0 + k, inst_id);
    c += keep[k] ? 1 : 0;
  }
  int total;
  int64_t o = ofs[blockIdx.x] + block_excl_scan<PC_BLOCK>(c, s, &total);
#pragma unroll
  for (int k = 0; k < PC_ITEMS; ++k) {
    if (!keep[k]) continue;
    const int64_t i = i0 + k;
    const double u = (double)(i / H), v = (double)(i % H), z = (double)depth[i];
    const double x = (u - cx) * z / fx, y = (v - cy) * z / fy;
    points[3 * o] = (float)fma(T[2], z, fma(T[1], y, fma(T[0], x, T[3])));
    points[3 * o + 1] = (float)fma(T[6], z, fma(T[5], y, fma(T[4], x, T[7])));
    points[3 * o + 2] = (float)fma(T[10], z, fma(T[9], y, fma(T[8], x, T[11])));
    colors[3 * o] = (float)((double)image[3 * i] / 255.0);
    colors[3 * o + 1] = (float)((double)image[3 * i + 1] / 255.0);
    colors[3 * o + 2] = (float)((double)image[3 * i + 2] / 255.0);
    ++o;
  }
}

// ---- voxel down-sample -------------------------------------------------------------------------------------------------
constexpr int MIN_BLOCKS = 256;

__device__ __forceinline__ void block_min3(float* sx, float* sy, float* sz) {
  const int t = threadIdx.x;
  __syncthreads();
  for (int d = PC_BLOCK / 2; d > 0; d >>= 1) {
    if (t < d) {
      sx[t] = fminf(sx[t], sx[t + d]);
      sy[t] = fminf(sy[t], sy[t + d]);
      sz[t] = fminf(sz[t], sz[t + d]);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(PC_BLOCK) void min_partial_kernel(const float* __restrict__ p, int64_t n, float* __restrict__ part) {
  __shared__ float sx[PC_BLOCK], sy[PC_BLOCK], sz[PC_BLOCK];
  const int t = threadIdx.x;
  float mx = INFINITY, my = INFINITY, mz = INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * PC_BLOCK + t; i < n; i += (int64_t)MIN_BLOCKS * PC_BLOCK) {
    mx = fminf(mx, p[3 * i]);
    my = fminf(my, p[3 * i + 1]);
    mz = fminf(mz, p[3 * i + 2]);
  }
  sx[t] = mx, sy[t] = my, sz[t] = mz;
  block_min3(sx, sy, sz);
  if (t == 0) {
    part[3 * blockIdx.x] = sx[0];
    part[3 * blockIdx.x + 1] = sy[0];
    part[3 * blockIdx.x + 2] = sz[0];
  }
}

__global__ __launch_bounds__(PC_BLOCK) void min_final_kernel(const float* __restrict__ part, float* __restrict__ out) {
  __shared__ float sx[PC_BLOCK], sy[PC_BLOCK], sz[PC_BLOCK];
  const int t = threadIdx.x;
  sx[t] = part[3 * t], sy[t] = part[3 * t + 1], sz[t] = part[3 * t + 2];
  block_min3(sx, sy, sz);
  if (t == 0) out[0] = sx[0], out[1] = sy[0], out[2] = sz[0];
}
static_assert(MIN_BLOCKS == PC_BLOCK, "min_final_kernel reads one partial per thread");

__global__ __launch_bounds__(PC_BLOCK) void voxel_keys_kernel(const float* __restrict__ p, int64_t n, const float* __restrict__ mn,
                                                              double voxel, int64_t* __restrict__ keys) {
  const double lim = (double)(1 << AXIS_BITS);
  const double m0 = (double)mn[0] - voxel * 0.5, m1 = (double)mn[1] - voxel * 0.5, m2 = (double)mn[2] - voxel * 0.5;
  for (int64_t i = (int64_t)blockIdx.x * PC_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * PC_BLOCK) {
    const double a = floor(((double)p[3 * i] - m0) / voxel), b = floor(((double)p[3 * i + 1] - m1) / voxel),
                 c = floor(((double)p[3 * i + 2] - m2) / voxel);
    const bool ok = a >= 0.0 && a < lim && b >= 0.0 && b < lim && c >= 0.0 && c < lim;   // false for NaN too
    keys[i] = ok ? ((int64_t)a << (2 * AXIS_BITS)) | ((int64_t)b << AXIS_BITS) | (int64_t)c : (int64_t)-1;
  }
}

__device__ __forceinline__ bool run_head(const int64_t* __restrict__ keys, int64_t i) { return i == 0 || keys[i] != keys[i - 1]; }

__global__ __launch_bounds__(PC_BLOCK) void segments_count_kernel(const int64_t* __restrict__ keys, int64_t n,
                                                                  int* __restrict__ blk_counts) {
  __shared__ int s[PC_BLOCK];
  const int64_t i0 = (int64_t)blockIdx.x * PC_PER_BLOCK + threadIdx.x * PC_ITEMS;
  int c = 0;
#pragma unroll
  for (int k = 0; k < PC_ITEMS; ++k)
    if (i0 + k < n && run_head(keys, i0 + k)) ++c;
  int total;
  block_excl_scan<PC_BLOCK>(c, s, &total);
  if (threadIdx.x == 0) blk_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(PC_BLOCK) void segments_emit_kernel(const int64_t* __restrict__ keys,
                                                                 const int64_t* __restrict__ perm, const float* __restrict__ points,
                                                                 const float* __restrict__ colors, int64_t n,
                                                                 const int64_t* __restrict__ ofs, double* __restrict__ out_points,
                                                                 double* __restrict__ out_colors, int64_t* __restrict__ out_keys,
                                                                 int64_t* __restrict__ out_counts) {
  __shared__ int s[PC_BLOCK];
  const int64_t i0 = (int64_t)blockIdx.x * PC_PER_BLOCK + threadIdx.x * PC_ITEMS;
  bool head[PC_ITEMS];
  int c = 0;
#pragma unroll
  for (int k = 0; k < PC_ITEMS; ++k) {
    head[k] = i0 + k < n && run_head(keys, i0 + k);
    c += head[k] ? 1 : 0;
  }
  int total;
  int64_t o = ofs[blockIdx.x] + block_excl_scan<PC_BLOCK>(c, s, &total);
  for (int k = 0; k < PC_ITEMS; ++k) {
    if (!head[k]) continue;
    const int64_t key = keys[i0 + k];
    double sx = 0.0, sy = 0.0, sz = 0.0, cr = 0.0, cg = 0.0, cb = 0.0;
    int64_t j = i0 + k;
    // the sort is stable, so perm ascends inside a run: the sums are in input order
    for (; j < n && keys[j] == key; ++j) {
      const int64_t src = perm[j];
      sx += (double)points[3 * src];
      sy += (double)points[3 * src + 1];
      sz += (double)points[3 * src + 2];
      if (colors) {
        cr += (double)colors[3 * src];
        cg += (double)colors[3 * src + 1];
        cb += (double)colors[3 * src + 2];
      }
    }
    const double cnt = (double)(j - (i0 + k));
    out_points[3 * o] = sx / cnt;
    out_points[3 * o + 1] = sy / cnt;
    out_points[3 * o + 2] = sz / cnt;
    if (colors) {
      out_colors[3 * o] = cr / cnt;
      out_colors[3 * o + 1] = cg / cnt;
      out_colors[3 * o + 2] = cb / cnt;
    }
    out_keys[o] = key;
    out_counts[o] = j - (i0 + k);
    ++o;
  }
}

// ---- nearest neighbour with its index, batched over candidate transforms -----------------------------------------------
constexpr int ICP_RB = 64;                                // workgroups per candidate in the reduction
constexpr int ICP_NSUM = 17;                              // pairs, sum d^2, sum a (3), sum b (3), sum a b^T (9)
constexpr int ICP_NSTATE = 4;                             // fitness, rmse, flag (0 = running), iterations

struct NniLayout {
  int64_t qblocks, chunks, chunk_len, off_idx, off_red, bytes;
};
inline NniLayout nni_layout(int64_t nq, int64_t nr, int64_t B) {
  NniLayout L;
  L.qblocks = (nq + NN_QBLK - 1) / NN_QBLK;
  nn_chunks(L.qblocks * B, nr, &L.chunk_len, &L.chunks);
  L.off_idx = align256(L.chunks * B * nq * 4);
  L.off_red = L.off_idx + align256(L.chunks * B * nq * 4);
  L.bytes = L.off_red + align256(B * ICP_RB * ICP_NSUM * 8);
  return L;
}

// row r of T (4,4 row-major, fp64) applied to the fp32 point, rounded once; explicit fmas so that every kernel that
// transforms a point gets the same bits
__device__ __forceinline__ float xform_row(const double* __restrict__ T, int r, float x, float y, float z) {
  return (float)fma(T[4 * r + 2], (double)z, fma(T[4 * r + 1], (double)y, fma(T[4 * r], (double)x, T[4 * r + 3])));
}

__device__ __forceinline__ bool frozen(const double* __restrict__ state, int b) {
  return state && state[ICP_NSTATE * b + 2] != 0.0;
}

__global__ __launch_bounds__(NN_BLOCK) void nni_partial_kernel(const float* __restrict__ q, int64_t nq, const float* __restrict__ p,
                                                               int64_t nr, int64_t chunk_len, const double* __restrict__ T,
                                                               const double* __restrict__ state, float* __restrict__ part_d,
                                                               int* __restrict__ part_i) {
  __shared__ float4 s_p[NN_TILE];
  const int b = blockIdx.z;
  if (frozen(state, b)) return;                           // the whole workgroup, before any barrier
  const int t = threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.x * NN_QBLK;
  const int64_t c = blockIdx.y;
  const int64_t p0 = c * chunk_len;
  const int64_t p1 = p0 + chunk_len < nr ? p0 + chunk_len : nr;
  float qx[NN_QPT], qy[NN_QPT], qz[NN_QPT], m[NN_QPT];
  int mi[NN_QPT];
#pragma unroll
  for (int k = 0; k < NN_QPT; ++k) {
    int64_t i = q0 + k * NN_BLOCK + t;
    i = i < nq ? i : nq - 1;                              // lanes past the end compute on a copy and store nothing
    const float x = q[3 * i], y = q[3 * i + 1], z = q[3 * i + 2];
    if (T) {
      const double* Tb = T + 16 * (int64_t)b;
      qx[k] = xform_row(Tb, 0, x, y, z);
      qy[k] = xform_row(Tb, 1, x, y, z);
      qz[k] = xform_row(Tb, 2, x, y, z);
    } else {
      qx[k] = x, qy[k] = y, qz[k] = z;
    }
    m[k] = INFINITY;
    mi[k] = (int)p0;                                      // a valid index even when no distance is ever below infinity
  }
  for (int64_t base = p0; base < p1; base += NN_TILE) {
    __syncthreads();
    {
      const int64_t j = base + t;
      // past the chunk: a point at infinity, whose squared distance (inf) is never below the minimum
      s_p[t] = j < p1 ? make_float4(p[3 * j], p[3 * j + 1], p[3 * j + 2], 0.0f) : make_float4(INFINITY, INFINITY, INFINITY, 0.0f);
    }
    __syncthreads();
    const int jb = (int)base;
#pragma unroll 4
    for (int j = 0; j < NN_TILE; ++j) {
      const float4 r = s_p[j];
#pragma unroll
      for (int k = 0; k < NN_QPT; ++k) {
        const float d = sq_dist(qx[k], qy[k], qz[k], r);
        const bool lt = d < m[k];                         // strict: of equal distances the lowest index stays
        m[k] = lt ? d : m[k];
        mi[k] = lt ? jb + j : mi[k];
      }
    }
  }
  const int64_t o = (c * gridDim.z + b) * nq;
#pragma unroll
  for (int k = 0; k < NN_QPT; ++k) {
    const int64_t i = q0 + k * NN_BLOCK + t;
    if (i < nq) {
      part_d[o + i] = m[k];
      part_i[o + i] = mi[k];
    }
  }
}

// min over the chunks in chunk order (strict <: the lowest chunk, so the lowest index, wins a tie) -> squared distance, index
__device__ __forceinline__ float chunks_min(const float* __restrict__ part_d, const int* __restrict__ part_i, int64_t nq, int64_t B,
                                            int64_t chunks, int64_t b, int64_t i, int* idx) {
  float m = part_d[b * nq + i];
  int mi = part_i[b * nq + i];
  for (int64_t c = 1; c < chunks; ++c) {
    const float d = part_d[(c * B + b) * nq + i];
    if (d < m) {
      m = d;
      mi = part_i[(c * B + b) * nq + i];
    }
  }
  *idx = mi;
  return m;
}

__global__ __launch_bounds__(256) void nni_finish_kernel(const float* __restrict__ part_d, const int* __restrict__ part_i,
                                                         int64_t nq, int64_t chunks, float* __restrict__ dist,
                                                         int* __restrict__ index) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nq; i += (int64_t)gridDim.x * 256) {
    int mi;
    const float m = chunks_min(part_d, part_i, nq, 1, chunks, 0, i, &mi);
    dist[i] = __fsqrt_rn(m);
    index[i] = mi;
  }
}

// fixed-order tree over the block's 256 values; thread 0 ends with the total
__device__ __forceinline__ double block_tree(double v, double* s) {
  const int t = threadIdx.x;
  __syncthreads();
  s[t] = v;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (t < d) s[t] += s[t + d];
    __syncthreads();
  }
  return s[0];
}

// grid (ICP_RB, B): each workgroup a fixed contiguous slice of the source, each thread a fixed stride through it
__global__ __launch_bounds__(256) void icp_reduce_partial_kernel(const float* __restrict__ src, int64_t n,
                                                                 const float* __restrict__ tgt, const double* __restrict__ T,
                                                                 const double* __restrict__ state, float max_corr,
                                                                 const float* __restrict__ part_d, const int* __restrict__ part_i,
                                                                 int64_t chunks, double* __restrict__ red, float* __restrict__ dist_out,
                                                                 int* __restrict__ idx_out) {
  __shared__ double s[256];
  const int b = blockIdx.y, B = gridDim.y;
  if (frozen(state, b)) return;
  const double* Tb = T + 16 * (int64_t)b;
  const int64_t per = (n + ICP_RB - 1) / ICP_RB;
  const int64_t i0 = (int64_t)blockIdx.x * per, i1 = i0 + per < n ? i0 + per : n;
  double acc[ICP_NSUM];
#pragma unroll
  for (int v = 0; v < ICP_NSUM; ++v) acc[v] = 0.0;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    int j;
    const float m = chunks_min(part_d, part_i, n, B, chunks, b, i, &j);
    const float d = __fsqrt_rn(m);
    if (dist_out) dist_out[(int64_t)b * n + i] = d;
    if (idx_out) idx_out[(int64_t)b * n + i] = j;
    if (d < max_corr) {
      const float x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
      const double a[3] = {(double)xform_row(Tb, 0, x, y, z), (double)xform_row(Tb, 1, x, y, z), (double)xform_row(Tb, 2, x, y, z)};
      const double t3[3] = {(double)tgt[3 * (int64_t)j], (double)tgt[3 * (int64_t)j + 1], (double)tgt[3 * (int64_t)j + 2]};
      acc[0] += 1.0;
      acc[1] += (double)d * (double)d;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        acc[2 + r] += a[r];
        acc[5 + r] += t3[r];
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) acc[8 + 3 * r + cc] += a[r] * t3[cc];
      }
    }
  }
#pragma unroll
  for (int v = 0; v < ICP_NSUM; ++v) {
    const double tot = block_tree(acc[v], s);
    if (threadIdx.x == 0) red[((int64_t)b * ICP_RB + blockIdx.x) * ICP_NSUM + v] = tot;
  }
}

__global__ __launch_bounds__(256) void icp_reduce_final_kernel(const double* __restrict__ red, const double* __restrict__ state,
                                                               double* __restrict__ sums) {
  __shared__ double s[256];
  const int b = blockIdx.x;
  if (frozen(state, b)) return;
  for (int v = 0; v < ICP_NSUM; ++v) {
    const double x = threadIdx.x < ICP_RB ? red[((int64_t)b * ICP_RB + threadIdx.x) * ICP_NSUM + v] : 0.0;
    const double tot = block_tree(x, s);
    if (threadIdx.x == 0) sums[(int64_t)b * ICP_NSUM + v] = tot;
  }
}

// ---- rigid update ------------------------------------------------------------------------------------------------------
// Eigenvectors of a symmetric 4x4 by cyclic Jacobi rotations; V's columns, A's diagonal the eigenvalues.
__host__ __device__ inline void jacobi4(double A[4][4], double V[4][4]) {
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 32; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < 4; ++i) {
      diag += A[i][i] * A[i][i];
      for (int j = i + 1; j < 4; ++j) off += A[i][j] * A[i][j];
    }
    if (off <= 1e-34 * diag || off == 0.0) break;
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 4; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 4; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 4; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
}

// sums (17) of the pairs (a_i, b_i) -> dT (4,4 row-major): the rigid transform minimising sum |R a + t - b|^2
__host__ __device__ inline void kabsch_from_sums(const double* __restrict__ S, double* __restrict__ dT) {
  const double np = S[0];
  const double ca[3] = {S[2] / np, S[3] / np, S[4] / np}, cb[3] = {S[5] / np, S[6] / np, S[7] / np};
  double H[3][3];                                          // sum (a - ca)(b - cb)^T
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) H[r][c] = S[8 + 3 * r + c] - np * ca[r] * cb[c];
  double N[4][4] = {{H[0][0] + H[1][1] + H[2][2], H[1][2] - H[2][1], H[2][0] - H[0][2], H[0][1] - H[1][0]},
                    {H[1][2] - H[2][1], H[0][0] - H[1][1] - H[2][2], H[0][1] + H[1][0], H[2][0] + H[0][2]},
                    {H[2][0] - H[0][2], H[0][1] + H[1][0], -H[0][0] + H[1][1] - H[2][2], H[1][2] + H[2][1]},
                    {H[0][1] - H[1][0], H[2][0] + H[0][2], H[1][2] + H[2][1], -H[0][0] - H[1][1] + H[2][2]}};
  double V[4][4];
  jacobi4(N, V);
  int best = 0;
  for (int i = 1; i < 4; ++i)
    if (N[i][i] > N[best][best]) best = i;
  double w = V[0][best], x = V[1][best], y = V[2][best], z = V[3][best];
  const double nq = sqrt(w * w + x * x + y * y + z * z);
  w /= nq, x /= nq, y /= nq, z /= nq;
  const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                          {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                          {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) dT[4 * r + c] = R[r][c];
    dT[4 * r + 3] = cb[r] - (R[r][0] * ca[0] + R[r][1] * ca[1] + R[r][2] * ca[2]);
  }
  dT[12] = dT[13] = dT[14] = 0.0;
  dT[15] = 1.0;
}

// one thread per candidate.  state: fitness, rmse, flag, iterations.  flag 1 = converged by open3d's test, 2 = fewer than 3
// pairs (no update possible), 3 = max_iter updates made.
__global__ __launch_bounds__(64) void icp_update_kernel(const double* __restrict__ sums, int64_t n, int B, int max_iter,
                                                        double* __restrict__ T, double* __restrict__ state) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double* st = state + ICP_NSTATE * b;
  if (st[2] != 0.0) return;
  const double* S = sums + (int64_t)ICP_NSUM * b;
  const double np = S[0];
  const double fitness = np / (double)n, rmse = np > 0.0 ? sqrt(S[1] / np) : 0.0;
  const bool first = st[3] == 0.0;
  const bool conv = !first && fabs(fitness - st[0]) < 1e-6 && fabs(rmse - st[1]) < 1e-6;
  st[0] = fitness;
  st[1] = rmse;
  if (conv) {
    st[2] = 1.0;
    return;
  }
  if (np < 3.0) {
    st[2] = 2.0;
    return;
  }
  double dT[16], Tn[16];
  kabsch_from_sums(S, dT);
  double* Tb = T + 16 * (int64_t)b;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      double a = 0.0;
      for (int k = 0; k < 4; ++k) a = fma(dT[4 * r + k], Tb[4 * k + c], a);
      Tn[4 * r + c] = a;
    }
  for (int k = 0; k < 16; ++k) Tb[k] = Tn[k];
  st[3] += 1.0;
  if (st[3] >= (double)max_iter) st[2] = 3.0;
}
}  // namespace

// ---- entry points ------------------------------------------------------------------------------------------------------
extern "C" int64_t cnr_unproject_workspace_bytes(int W, int H) {
  if (W < 1 || H < 1) return CNR_E_SHAPE;
  return compact_layout((int64_t)W * H).bytes;
}

extern "C" int cnr_unproject_count(const float* depth, const int* obj_mask, int W, int H, int inst_id, void* workspace,
                                   int64_t* count_out, void* stream) {
  if (!depth || !obj_mask || !workspace || !count_out) return CNR_E_ARG;
  if (W < 1 || H < 1) return CNR_E_SHAPE;
  const int64_t npix = (int64_t)W * H;
  const CompactLayout L = compact_layout(npix);
  if (L.nblk > 0x7fffffff) return CNR_E_SHAPE;
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(unproject_count_kernel, dim3((unsigned)L.nblk), dim3(PC_BLOCK), 0, (hipStream_t)stream, depth, obj_mask, npix,
                     inst_id, (int*)ws);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL((blocks_scan_kernel<1, int64_t, int>), dim3(1), dim3(SCAN_THREADS), 0, (hipStream_t)stream, (const int*)ws, L.nblk,
                     (int64_t*)(ws + L.off_ofs), count_out);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_unproject_emit(const float* depth, const int* obj_mask, const uint8_t* image, int W, int H, int inst_id,
                                  double fx, double fy, double cx, double cy, const double* T_WC, void* workspace, float* points,
                                  float* colors, void* stream) {
  if (!depth || !obj_mask || !image || !T_WC || !workspace || !points || !colors) return CNR_E_ARG;
  if (W < 1 || H < 1 || !(fx != 0.0) || !(fy != 0.0)) return CNR_E_SHAPE;
  const int64_t npix = (int64_t)W * H;
  const CompactLayout L = compact_layout(npix);
  if (L.nblk > 0x7fffffff) return CNR_E_SHAPE;
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(unproject_emit_kernel, dim3((unsigned)L.nblk), dim3(PC_BLOCK), 0, (hipStream_t)stream, depth, obj_mask, image,
                     npix, H, inst_id, fx, fy, cx, cy, T_WC, (const int64_t*)(ws + L.off_ofs), points, colors);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int64_t cnr_points_min_workspace_bytes(int64_t n) {
  if (n < 1) return CNR_E_SHAPE;
  return align256(MIN_BLOCKS * 3 * 4);
}

extern "C" int cnr_points_min(const float* points, int64_t n, void* workspace, float* min_out, void* stream) {
  if (!points || !workspace || !min_out) return CNR_E_ARG;
  if (n < 1) return CNR_E_SHAPE;
  hipLaunchKernelGGL(min_partial_kernel, dim3(MIN_BLOCKS), dim3(PC_BLOCK), 0, (hipStream_t)stream, points, n, (float*)workspace);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(min_final_kernel, dim3(1), dim3(PC_BLOCK), 0, (hipStream_t)stream, (const float*)workspace, min_out);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_voxel_keys(const float* points, int64_t n, const float* min_xyz, double voxel, int64_t* keys, void* stream) {
  if (!points || !min_xyz || !keys) return CNR_E_ARG;
  if (n < 1 || !(voxel > 0.0)) return CNR_E_SHAPE;
  hipLaunchKernelGGL(voxel_keys_kernel, dim3(grid_of(n, PC_BLOCK, 4096)), dim3(PC_BLOCK), 0, (hipStream_t)stream, points, n, min_xyz, voxel,
                     keys);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int64_t cnr_voxel_segments_workspace_bytes(int64_t n) {
  if (n < 1) return CNR_E_SHAPE;
  return compact_layout(n).bytes;
}

extern "C" int cnr_voxel_segments_count(const int64_t* sorted_keys, int64_t n, void* workspace, int64_t* count_out, void* stream) {
  if (!sorted_keys || !workspace || !count_out) return CNR_E_ARG;
  if (n < 1) return CNR_E_SHAPE;
  const CompactLayout L = compact_layout(n);
  if (L.nblk > 0x7fffffff) return CNR_E_SHAPE;
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(segments_count_kernel, dim3((unsigned)L.nblk), dim3(PC_BLOCK), 0, (hipStream_t)stream, sorted_keys, n, (int*)ws);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL((blocks_scan_kernel<1, int64_t, int>), dim3(1), dim3(SCAN_THREADS), 0, (hipStream_t)stream, (const int*)ws, L.nblk,
                     (int64_t*)(ws + L.off_ofs), count_out);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_voxel_segments_emit(const int64_t* sorted_keys, const int64_t* perm, const float* points, const float* colors,
                                       int64_t n, void* workspace, double* out_points, double* out_colors, int64_t* out_keys,
                                       int64_t* out_counts, void* stream) {
  if (!sorted_keys || !perm || !points || !workspace || !out_points || !out_keys || !out_counts) return CNR_E_ARG;
  if (colors && !out_colors) return CNR_E_ARG;
  if (n < 1) return CNR_E_SHAPE;
  const CompactLayout L = compact_layout(n);
  if (L.nblk > 0x7fffffff) return CNR_E_SHAPE;
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(segments_emit_kernel, dim3((unsigned)L.nblk), dim3(PC_BLOCK), 0, (hipStream_t)stream, sorted_keys, perm, points,
                     colors, n, (const int64_t*)(ws + L.off_ofs), out_points, out_colors, out_keys, out_counts);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

static int nni_check(int64_t nq, int64_t nr, int64_t B, NniLayout* L) {
  if (nq < 1 || nr < 1 || B < 1 || B > 65535 || nr > 0x7fffffff) return CNR_E_SHAPE;
  *L = nni_layout(nq, nr, B);
  if (L->qblocks > 0x7fffffff || L->chunks > 65535) return CNR_E_SHAPE;
  return CNR_OK;
}

extern "C" int64_t cnr_nn_index_workspace_bytes(int64_t nq, int64_t nr) {
  NniLayout L;
  if (nni_check(nq, nr, 1, &L) != CNR_OK) return CNR_E_SHAPE;
  return L.bytes;
}

extern "C" int cnr_nn_index(const float* q, int64_t nq, const float* p, int64_t nr, float* dist_out, int* index_out,
                            void* workspace, void* stream) {
  if (!q || !p || !dist_out || !index_out || !workspace) return CNR_E_ARG;
  NniLayout L;
  if (nni_check(nq, nr, 1, &L) != CNR_OK) return CNR_E_SHAPE;
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(nni_partial_kernel, dim3((unsigned)L.qblocks, (unsigned)L.chunks, 1), dim3(NN_BLOCK), 0, (hipStream_t)stream, q,
                     nq, p, nr, L.chunk_len, (const double*)nullptr, (const double*)nullptr, (float*)ws, (int*)(ws + L.off_idx));
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(nni_finish_kernel, dim3(grid_of(nq, 256, 4096)), dim3(256), 0, (hipStream_t)stream, (const float*)ws,
                     (const int*)(ws + L.off_idx), nq, L.chunks, dist_out, index_out);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int64_t cnr_icp_workspace_bytes(int64_t n_src, int64_t n_tgt, int B) {
  NniLayout L;
  if (nni_check(n_src, n_tgt, B, &L) != CNR_OK) return CNR_E_SHAPE;
  return L.bytes;
}

extern "C" int cnr_icp_step(const float* src, int64_t n_src, const float* tgt, int64_t n_tgt, const double* T, int B,
                            float max_corr, const double* state, void* workspace, double* sums, float* dist_out, int* index_out,
                            void* stream) {
  if (!src || !tgt || !T || !workspace || !sums) return CNR_E_ARG;
  NniLayout L;
  if (nni_check(n_src, n_tgt, B, &L) != CNR_OK || !(max_corr > 0.0f)) return CNR_E_SHAPE;
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(nni_partial_kernel, dim3((unsigned)L.qblocks, (unsigned)L.chunks, (unsigned)B), dim3(NN_BLOCK), 0,
                     (hipStream_t)stream, src, n_src, tgt, n_tgt, L.chunk_len, T, state, (float*)ws, (int*)(ws + L.off_idx));
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(icp_reduce_partial_kernel, dim3(ICP_RB, (unsigned)B), dim3(256), 0, (hipStream_t)stream, src, n_src, tgt, T,
                     state, max_corr, (const float*)ws, (const int*)(ws + L.off_idx), L.chunks, (double*)(ws + L.off_red), dist_out,
                     index_out);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(icp_reduce_final_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream,
                     (const double*)(ws + L.off_red), state, sums);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_icp_update(const double* sums, int64_t n_src, int B, int max_iter, double* T, double* state, void* stream) {
  if (!sums || !T || !state) return CNR_E_ARG;
  if (n_src < 1 || B < 1 || B > 65535 || max_iter < 1) return CNR_E_SHAPE;
  hipLaunchKernelGGL(icp_update_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, sums, n_src, B, max_iter,
                     T, state);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}
