// Mesh simplification by uniform vertex clustering with quadric placement (Lindstrom, "Out-of-core
// simplification of large polygonal models", 2000, quadrics per corner as open3d's simplify_vertex_clustering).  The clusters
// are the cells of cnr_voxel_keys; their numbering, the face remap and the compaction are csrc/mesh_topo.hip's.  This unit adds
// the floating-point part and the face rows.  Rules as in mesh_topo.hip: no floating-point atomic, every sum in an order fixed
// by the data alone, no wait on another workgroup, every loop bounded, indices that arrive in an array are checked before they
// are used (err |= 2, the entry skipped).  The arithmetic is mesh_simplify_common.h's, contraction off.
//
//   err bits: 2 = an index outside its range was met (and skipped), 4 = a vertex has no cell (key -1: a non-finite coordinate,
//             or more than 2^21 cells on an axis).
//
//   cnr_simplify_check_keys    err |= 4 when a key is negative.
//   cnr_simplify_vertex_q      q[3 v + a] = (double)verts[3 v + a] - (double)min[a].
//   cnr_simplify_face_records  records (F,10) f64: face_record of q0, q1, q2 (q as above), one thread per face.
//   cnr_mesh_face_normals_f64  normals (F,3) f64 = (p1 - p0) x (p2 - p0) from the fp32 corners as doubles (no minimum taken off).
//   cnr_segment_sum_f64        out[c][k] = the sum over the positions j of segment c (sorted_seg[j] == c, sorted_seg ascending)
//                              of items[(gather[j] / gather_div)][k]; gather == NULL: position j takes item j.  One GROUP of
//                              16 lanes per segment, group_sum's order; an empty segment gives zeros.  K <= 16.
//   cnr_simplify_place         one thread per cluster c, its cell from keys[roots[c]], its run in sorted_cluster by two binary
//                              searches: mean = possum / count per axis; placement 0 = quadric (solve_quadric about the mean),
//                              1 = mean, both clamped to the cell and rounded by to_f32_in_cell; 2 = the representative
//                              verts[roots[c]] copied as it is.  error[c] = quadric_error at the fp64 position (after the clamp,
//                              before the rounding), clamped[c] = 1 when the clamp moved an axis.
//   cnr_simplify_face_rows     rows[f] = faces[f] rotated so that its smallest index comes first (orientation kept).
//   cnr_mesh_normals_finish    out (V,3) f32 = sums / sqrt((x x + y y) + z z), zeros where that length is 0 or not finite.
#include "cnr_common.h"
#include "geom_common.h"
#include "mesh_simplify_common.h"

#include <math.h>

#pragma clang fp contract(off)

using namespace cnr;

namespace {
constexpr int MS_BLOCK = 256;
constexpr int64_t MS_GRID_CAP = 8192;
constexpr int64_t INDEX_LIMIT = 0x7fffffff;
constexpr int MS_GROUPS = MS_BLOCK / simp::GROUP;
constexpr int MS_MAX_K = 16;

#define MS_GRID_STRIDE(i, n) \
  for (int64_t i = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x; i < (n); i += (int64_t)gridDim.x * MS_BLOCK)

inline unsigned ms_grid(int64_t n) { return grid_of(n, MS_BLOCK, MS_GRID_CAP); }

__device__ __forceinline__ bool in_range(int64_t i, int64_t n) { return i >= 0 && i < n; }

__global__ __launch_bounds__(MS_BLOCK) void check_keys_kernel(const int64_t* __restrict__ keys, int64_t V, int* err) {
  bool bad = false;
  MS_GRID_STRIDE(i, V) bad |= keys[i] < 0;
  if (bad) atomicOr(err, 4);
}

__global__ __launch_bounds__(MS_BLOCK) void vertex_q_kernel(const float* __restrict__ verts, const float* __restrict__ mn, int64_t n3,
                                                            double* __restrict__ q) {
  const double m[3] = {(double)mn[0], (double)mn[1], (double)mn[2]};
  MS_GRID_STRIDE(i, n3) q[i] = (double)verts[i] - m[i % 3];
}

__global__ __launch_bounds__(MS_BLOCK) void face_records_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                                const float* __restrict__ mn, int64_t F, int64_t V,
                                                                double* __restrict__ records, int* err) {
  const double m[3] = {(double)mn[0], (double)mn[1], (double)mn[2]};
  bool bad = false;
  MS_GRID_STRIDE(f, F) {
    const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    simp::FaceRecord r;
    if (in_range(i0, V) && in_range(i1, V) && in_range(i2, V)) {
      double q0[3], q1[3], q2[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        q0[a] = (double)verts[3 * i0 + a] - m[a];
        q1[a] = (double)verts[3 * i1 + a] - m[a];
        q2[a] = (double)verts[3 * i2 + a] - m[a];
      }
      r = simp::face_record(q0, q1, q2);
    } else {
      bad = true;
#pragma unroll
      for (int k = 0; k < simp::RECORD; ++k) r.k[k] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < simp::RECORD; ++k) records[simp::RECORD * f + k] = r.k[k];
  }
  if (bad) atomicOr(err, 2);
}

__global__ __launch_bounds__(MS_BLOCK) void face_normals_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int64_t F,
                                                                int64_t V, double* __restrict__ normals, int* err) {
  bool bad = false;
  MS_GRID_STRIDE(f, F) {
    const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    double n[3] = {0.0, 0.0, 0.0};
    if (in_range(i0, V) && in_range(i1, V) && in_range(i2, V)) {
      double u[3], v[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double p0 = (double)verts[3 * i0 + a];
        u[a] = (double)verts[3 * i1 + a] - p0;
        v[a] = (double)verts[3 * i2 + a] - p0;
      }
      simp::cross3(u, v, n);
    } else {
      bad = true;
    }
    normals[3 * f] = n[0], normals[3 * f + 1] = n[1], normals[3 * f + 2] = n[2];
  }
  if (bad) atomicOr(err, 2);
}

// first position in the ascending a[0 .. n) whose value is >= key
__device__ __forceinline__ int64_t lower_bound_i32(const int* __restrict__ a, int64_t n, int64_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {                                          // at most 32 rounds
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One GROUP of 16 lanes per segment (16 segments per block, 4 per wave).  A group's lanes leave together, and the exchanges
// below stay inside the group (lane ^ d with d < 16), so no lane reads one that has left.  The lanes' loop is lane_partial's,
// for K values at a time; then tree_combine's distances 8, 4, 2, 1.
template <int K>
__global__ __launch_bounds__(MS_BLOCK) void segment_sum_kernel(const double* __restrict__ items, const int64_t* __restrict__ gather,
                                                               int gather_div, const int* __restrict__ sorted_seg, int64_t N,
                                                               int64_t n_items, int64_t C, double* __restrict__ out, int* err) {
  const int lane = threadIdx.x & (simp::GROUP - 1);
  const int64_t c = (int64_t)blockIdx.x * MS_GROUPS + (threadIdx.x / simp::GROUP);
  if (c >= C) return;                                        // the whole group
  const int64_t j0 = lower_bound_i32(sorted_seg, N, c), j1 = lower_bound_i32(sorted_seg, N, c + 1);
  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;
  bool bad = false;
  for (int64_t j = j0 + lane; j < j1; j += simp::GROUP) {    // bounded by N
    const int64_t it = gather ? gather[j] / gather_div : j;
    if (!in_range(it, n_items)) {
      bad = true;
      continue;
    }
    const double* row = items + (int64_t)K * it;
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = acc[k] + row[k];
  }
#pragma unroll
  for (int d = simp::GROUP / 2; d > 0; d >>= 1) {
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = acc[k] + __shfl_xor(acc[k], d, simp::GROUP);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) out[(int64_t)K * c + k] = acc[k];
  }
  if (bad) atomicOr(err, 2);
}

__global__ __launch_bounds__(MS_BLOCK) void place_kernel(const double* __restrict__ quadrics, const double* __restrict__ possum,
                                                         const int* __restrict__ sorted_cluster, const float* __restrict__ verts,
                                                         const int* __restrict__ roots, const int64_t* __restrict__ keys,
                                                         const float* __restrict__ mn, int64_t V, int64_t C, double cell, double tau,
                                                         int placement, float* __restrict__ out, double* __restrict__ error,
                                                         uint8_t* __restrict__ clamped, int* err) {
  int e = 0;
  MS_GRID_STRIDE(c, C) {
    const int64_t rep = roots[c];
    float res[3] = {0.f, 0.f, 0.f};
    double er = 0.0;
    bool moved = false;
    const int64_t key = in_range(rep, V) ? keys[rep] : (int64_t)-1;
    if (!in_range(rep, V)) e |= 2;
    else if (key < 0) e |= 4;
    else {
      double Q[simp::RECORD];
#pragma unroll
      for (int k = 0; k < simp::RECORD; ++k) Q[k] = quadrics[simp::RECORD * c + k];
      double x[3];
      if (placement == 2) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          res[a] = verts[3 * rep + a];
          x[a] = (double)res[a] - (double)mn[a];
        }
      } else {
        const int64_t n = lower_bound_i32(sorted_cluster, V, c + 1) - lower_bound_i32(sorted_cluster, V, c);
        double mean[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) mean[a] = possum[3 * c + a] / (double)n;
        if (placement == 0) simp::solve_quadric(Q, mean, tau, x);
        else x[0] = mean[0], x[1] = mean[1], x[2] = mean[2];
        int64_t ci[3];
        simp::key_cells(key, ci);
        moved = simp::clamp_to_cell(x, ci, cell);
#pragma unroll
        for (int a = 0; a < 3; ++a) res[a] = simp::to_f32_in_cell(x[a], mn[a], ci[a], cell);
      }
      er = simp::quadric_error(Q, x);
    }
    out[3 * c] = res[0], out[3 * c + 1] = res[1], out[3 * c + 2] = res[2];
    error[c] = er;
    clamped[c] = moved ? 1 : 0;
  }
  if (e) atomicOr(err, e);
}

__global__ __launch_bounds__(MS_BLOCK) void face_rows_kernel(const int* __restrict__ faces, int64_t F, int* __restrict__ rows) {
  MS_GRID_STRIDE(f, F) {
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    int r0 = a, r1 = b, r2 = c;                                // the first smallest corner leads
    if (b < a && b <= c) r0 = b, r1 = c, r2 = a;
    else if (c < a && c < b) r0 = c, r1 = a, r2 = b;
    rows[3 * f] = r0, rows[3 * f + 1] = r1, rows[3 * f + 2] = r2;
  }
}

__global__ __launch_bounds__(MS_BLOCK) void normals_finish_kernel(const double* __restrict__ sums, int64_t V, float* __restrict__ out) {
  MS_GRID_STRIDE(v, V) {
    const double x = sums[3 * v], y = sums[3 * v + 1], z = sums[3 * v + 2];
    const double len = sqrt((x * x + y * y) + z * z);
    const bool ok = len > 0.0 && len < INFINITY;
    out[3 * v] = ok ? (float)(x / len) : 0.f;
    out[3 * v + 1] = ok ? (float)(y / len) : 0.f;
    out[3 * v + 2] = ok ? (float)(z / len) : 0.f;
  }
}

#define MS_LAUNCH(kernel, n, ...)                                                                              \
  do {                                                                                                         \
    hipLaunchKernelGGL(kernel, dim3(ms_grid(n)), dim3(MS_BLOCK), 0, (hipStream_t)stream, __VA_ARGS__);         \
    CNR_LAUNCH_CHECK();                                                                                        \
  } while (0)

inline bool sizes_ok(int64_t F, int64_t V) { return F >= 1 && V >= 1 && F <= INDEX_LIMIT / 3 && V <= INDEX_LIMIT; }

template <int K>
int launch_segment_sum(const double* items, const int64_t* gather, int gather_div, const int* sorted_seg, int64_t N, int64_t n_items,
                       int K_run, int64_t C, double* out, int* err, void* stream) {
  if constexpr (K > MS_MAX_K) {
    return CNR_E_SHAPE;
  } else {
    if (K_run != K) return launch_segment_sum<K + 1>(items, gather, gather_div, sorted_seg, N, n_items, K_run, C, out, err, stream);
    hipLaunchKernelGGL(segment_sum_kernel<K>, dim3((unsigned)((C + MS_GROUPS - 1) / MS_GROUPS)), dim3(MS_BLOCK), 0, (hipStream_t)stream,
                       items, gather, gather_div, sorted_seg, N, n_items, C, out, err);
    CNR_LAUNCH_CHECK();
    return CNR_OK;
  }
}
}  // namespace

// ---- entry points --------------------------------------------------------------------------------------------------------
extern "C" int cnr_simplify_check_keys(const int64_t* keys, int64_t V, int* err, void* stream) {
  if (!keys || !err) return CNR_E_ARG;
  if (V < 1 || V > INDEX_LIMIT) return CNR_E_SHAPE;
  MS_LAUNCH(check_keys_kernel, V, keys, V, err);
  return CNR_OK;
}

extern "C" int cnr_simplify_vertex_q(const float* verts, const float* min_xyz, int64_t V, double* q, void* stream) {
  if (!verts || !min_xyz || !q) return CNR_E_ARG;
  if (V < 1 || V > INDEX_LIMIT / 3) return CNR_E_SHAPE;
  MS_LAUNCH(vertex_q_kernel, 3 * V, verts, min_xyz, 3 * V, q);
  return CNR_OK;
}

extern "C" int cnr_simplify_face_records(const float* verts, const int* faces, const float* min_xyz, int64_t F, int64_t V,
                                         double* records, int* err, void* stream) {
  if (!verts || !faces || !min_xyz || !records || !err) return CNR_E_ARG;
  if (!sizes_ok(F, V)) return CNR_E_SHAPE;
  MS_LAUNCH(face_records_kernel, F, verts, faces, min_xyz, F, V, records, err);
  return CNR_OK;
}

extern "C" int cnr_mesh_face_normals_f64(const float* verts, const int* faces, int64_t F, int64_t V, double* normals, int* err,
                                         void* stream) {
  if (!verts || !faces || !normals || !err) return CNR_E_ARG;
  if (!sizes_ok(F, V)) return CNR_E_SHAPE;
  MS_LAUNCH(face_normals_kernel, F, verts, faces, F, V, normals, err);
  return CNR_OK;
}

extern "C" int cnr_segment_sum_f64(const double* items, const int64_t* gather, int gather_div, const int* sorted_seg, int64_t N,
                                   int64_t n_items, int K, int64_t C, double* out, int* err, void* stream) {
  if (!items || !sorted_seg || !out || !err) return CNR_E_ARG;
  if (N < 1 || N > INDEX_LIMIT || n_items < 1 || n_items > INDEX_LIMIT || C < 1 || C > INDEX_LIMIT || K < 1 || K > MS_MAX_K ||
      gather_div < 1)
    return CNR_E_SHAPE;
  if (!gather && n_items < N) return CNR_E_SHAPE;
  return launch_segment_sum<1>(items, gather, gather_div, sorted_seg, N, n_items, K, C, out, err, stream);
}

extern "C" int cnr_simplify_place(const double* quadrics, const double* possum, const int* sorted_cluster, const float* verts,
                                  const int* roots, const int64_t* keys, const float* min_xyz, int64_t V, int64_t C, double cell,
                                  double tau, int placement, float* out_verts, double* error, uint8_t* clamped, int* err,
                                  void* stream) {
  if (!quadrics || !verts || !roots || !keys || !min_xyz || !out_verts || !error || !clamped || !err) return CNR_E_ARG;
  if (placement < 0 || placement > 2) return CNR_E_ARG;
  if (placement != 2 && (!possum || !sorted_cluster)) return CNR_E_ARG;
  if (V < 1 || V > INDEX_LIMIT / 3 || C < 1 || C > V) return CNR_E_SHAPE;
  if (!(cell > 0.0) || !(cell < INFINITY) || !(tau >= 0.0) || !(tau < 1.0)) return CNR_E_ARG;
  MS_LAUNCH(place_kernel, C, quadrics, possum, sorted_cluster, verts, roots, keys, min_xyz, V, C, cell, tau, placement, out_verts, error,
            clamped, err);
  return CNR_OK;
}

extern "C" int cnr_simplify_face_rows(const int* faces, int64_t F, int* rows, void* stream) {
  if (!faces || !rows) return CNR_E_ARG;
  if (F < 1 || F > INDEX_LIMIT / 3) return CNR_E_SHAPE;
  MS_LAUNCH(face_rows_kernel, F, faces, F, rows);
  return CNR_OK;
}

extern "C" int cnr_mesh_normals_finish(const double* sums, int64_t V, float* out, void* stream) {
  if (!sums || !out) return CNR_E_ARG;
  if (V < 1 || V > INDEX_LIMIT / 3) return CNR_E_SHAPE;
  MS_LAUNCH(normals_finish_kernel, V, sums, V, out);
  return CNR_OK;
}
