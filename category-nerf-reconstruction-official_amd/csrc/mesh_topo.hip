// The mesh as a graph: connected components by vertex or by edge, edge statistics (boundary, non-manifold,
// orientation), the per-component table (faces, vertices, bounding box, area), compaction of a face selection, and welding of
// coincident vertices.  Every launch is deterministic: integer atomics only (minima and counts, whose results do not depend on
// their order), no floating-point atomic, fixed reduction orders, count -> scan -> emit for every variable-size output.
// No kernel waits for another workgroup; every loop is bounded and a loop that runs out sets the device word *err.
//
//   err bits: 1 = a union/find or flatten loop ran out of its bound, 2 = an index outside its range was met (and skipped).
//
//   cnr_mesh_check_faces      err |= 2 when a face index lies outside [0, V).  Nothing else here trusts an index before this
//                             has been read back as 0.
//   cnr_mesh_labels_init      L[i] = i.
//   cnr_mesh_union_pairs      joins pairs[2 j], pairs[2 j + 1] (each checked against [0, n): a bad pair is skipped, err |= 2).
//   cnr_mesh_union_faces      vertex connectivity: joins (v0, v1) and (v0, v2) of every face, and sets used[v] = 1.
//   cnr_mesh_edge_keys        keys[3 f + k] = edge_key(faces[3 f + k], faces[3 f + (k + 1) % 3]) (mesh_topo_common.h).
//   cnr_mesh_union_edges      edge connectivity: over the keys sorted (stably) with perm = the slots 3 f + k in sorted order, joins
//                             the faces of neighbouring equal keys >= 0.
//   cnr_mesh_flatten          pointer-jumping sweeps (mesh_topo_common.h) until every L[i] is the root = the set's smallest element.
//   cnr_mesh_roots_count/_emit  the i with L[i] == i (and used[i] != 0 when used is given), ascending: the rank is the component id.
//   cnr_mesh_assign           comp[i] = lower_bound(roots, L[i]), or -1 where used[i] == 0.
//   cnr_mesh_cross_component  mode 0 (edge): vertex_component[v] = the smallest face_component of the faces that use v, -1 for
//                             none (an unsigned atomic minimum over 0xffffffff); mode 1 (vertex): face_component[f] =
//                             vertex_component[faces[3 f]].
//   cnr_mesh_edge_stats       per run of equal keys >= 0, multiplicity m: counts[3 c + 0] += (m == 1), counts[3 c + 1] += (m > 2),
//                             counts[3 c + 2] += (m == 2 and both faces run the edge the same way), c = the component of the
//                             run's first face.  The caller zeroes counts.
//   cnr_mesh_component_stats  n_vertices[c] = the v with vertex_component[v] == c; and over the faces sorted (stably) by
//                             component, order = the face indices in that order: first, one thread per sorted position,
//                                 u = (double)p1 - (double)p0, v = (double)p2 - (double)p0 (per axis),
//                                 cx = u.y v.z - u.z v.y, cy = u.z v.x - u.x v.z, cz = u.x v.y - u.y v.x (each product rounded, then
//                                 the difference), area = 0.5 * sqrt((cx cx + cy cy) + cz cz), and the face's box (fminf / fmaxf
//                                 over its corners) into the workspace; then ONE WAVE PER COMPONENT:
//                               run = [lower_bound(sorted_comp, c), lower_bound(sorted_comp, c + 1)), n_faces[c] = its length;
//                               lane l takes the run's positions l, l + 64, l + 128, ... in that (ascending) order, starting
//                               from acc = 0.0, lo = +inf, hi = -inf: acc = acc + area, lo = fminf(lo, box lo), hi = fmaxf(hi,
//                               box hi) per axis (minima and maxima are exact, so their grouping does not matter);
//                               then the lanes combine over the fixed tree of distances 32, 16, 8, 4, 2, 1:
//                                 a[l] = a[l] + a[l ^ d] (for the minima and maxima: fminf / fmaxf), lane 0 writes.
//                             An empty run cannot occur (every component has a face).  verts == NULL: the counts only.
//   cnr_mesh_compact_count/_emit  the faces with keep_face != 0 in their old order; reindex != 0: re-indexed to the vertices
//                             they use in their old order (vertex_map (V,) = new index or -1, kept_vertices ascending);
//                             reindex == 0: their indices as they are.  counts_out = (kept faces, kept vertices) int64.
//   cnr_weld_runs             over the vertices in sorted order (perm), rows (V,3) int32 = the bit patterns of the positions
//                             (exact mode) or keys (V,) int64 already gathered into sorted order (cell mode): a position starts a
//                             run when it is the first, differs from its predecessor, holds a NaN (exact) or has key -1 (cell);
//                             rep[perm[j]] = perm[head of j's run] -- the lowest input index of the run when the sort was stable.
//   cnr_mesh_remap_faces      out[3 f + k] = remap[faces[3 f + k]]; keep[f] = 0 when drop_degenerate and two corners coincide,
//                             else 1.
//
// Orientation repair: a LINK is a run of exactly two equal keys (degenerate faces' keys all -1), rel = 1 when
// both faces run the edge the same way.
//   cnr_mesh_orient_keys      cnr_mesh_edge_keys with a degenerate face's three keys -1.
//   cnr_mesh_orient_union     words[i] = i << 1, then unite_parity (mesh_topo_common.h) over the links.
//   cnr_mesh_orient_flatten   jump_parity sweeps; labels[i] = root, flip0[i] = i's parity relative to the root.
//   cnr_mesh_orient_check     bad[patch] |= 1 where a link has flip0[f] ^ flip0[g] != rel; counts[patch] = (edge slots in no run of
//                             two, links with rel == 1); then flip0 = 0 in bad patches.
//   cnr_mesh_orient_stats     per patch: its vertex box and its count of flip0 by integer atomics (exact minima / maxima on an
//                             order-preserving image of the floats, sums of integers: any order gives the same); then over the
//                             faces stably sorted by patch the per-face terms, and ONE WAVE PER PATCH sums them; the order of
//                             operations stands at orient_face_term_kernel and orient_patch_sum_kernel below.
//   cnr_mesh_orient_apply     flip = flip0 ^ sign[patch], a flipped (a, b, d) becomes (a, d, b).
#include "cnr_common.h"
#include "geom_common.h"
#include "mesh_topo_common.h"

#include <math.h>

#pragma clang fp contract(off)

using namespace cnr;

namespace {
constexpr int MT_BLOCK = 256;
constexpr int64_t MT_GRID_CAP = 8192;
constexpr int MT_ITEMS = 4;
constexpr int MT_PER_BLOCK = MT_BLOCK * MT_ITEMS;
constexpr int MT_WAVES = MT_BLOCK / 64;
constexpr int64_t INDEX_LIMIT = 0x7fffffff;

#define MT_GRID_STRIDE(i, n) \
  for (int64_t i = (int64_t)blockIdx.x * MT_BLOCK + threadIdx.x; i < (n); i += (int64_t)gridDim.x * MT_BLOCK)

inline unsigned mt_grid(int64_t n) { return grid_of(n, MT_BLOCK, MT_GRID_CAP); }

__global__ __launch_bounds__(MT_BLOCK) void check_faces_kernel(const int* __restrict__ faces, int64_t n3, int V, int* err) {
  bool bad = false;
  MT_GRID_STRIDE(i, n3) {
    const int v = faces[i];
    bad |= v < 0 || v >= V;
  }
  if (bad) atomicOr(err, 2);
}

__global__ __launch_bounds__(MT_BLOCK) void labels_init_kernel(int* __restrict__ L, int64_t n) {
  MT_GRID_STRIDE(i, n) L[i] = (int)i;
}

__global__ __launch_bounds__(MT_BLOCK) void union_pairs_kernel(const int* __restrict__ pairs, int64_t m, int n, int* L, int* err) {
  int e = 0;
  MT_GRID_STRIDE(j, m) {
    const int a = pairs[2 * j], b = pairs[2 * j + 1];
    if (a < 0 || a >= n || b < 0 || b >= n) {
      e |= 2;
      continue;
    }
    int fe = 0;
    ccl::unite_halving(L, a, b, n, &fe);
    e |= fe;
  }
  if (e) atomicOr(err, e);
}

__global__ __launch_bounds__(MT_BLOCK) void union_faces_kernel(const int* __restrict__ faces, int64_t F, int V, int* L,
                                                               uint8_t* __restrict__ used, int* err) {
  int e = 0;
  MT_GRID_STRIDE(f, F) {
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    used[a] = 1, used[b] = 1, used[c] = 1;
    ccl::unite_halving(L, a, b, V, &e);
    ccl::unite_halving(L, a, c, V, &e);
  }
  if (e) atomicOr(err, e);
}

__global__ __launch_bounds__(MT_BLOCK) void edge_keys_kernel(const int* __restrict__ faces, int64_t F, int64_t* __restrict__ keys) {
  MT_GRID_STRIDE(f, F) {
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    keys[3 * f] = ccl::edge_key(a, b);
    keys[3 * f + 1] = ccl::edge_key(b, c);
    keys[3 * f + 2] = ccl::edge_key(c, a);
  }
}

__global__ __launch_bounds__(MT_BLOCK) void union_edges_kernel(const int64_t* __restrict__ keys, const int64_t* __restrict__ perm,
                                                               int64_t E, int F, int* L, int* err) {
  int e = 0;
  MT_GRID_STRIDE(j, E) {
    if (j == 0) continue;
    const int64_t k = keys[j];
    if (k < 0 || k != keys[j - 1]) continue;
    const int64_t s0 = perm[j - 1], s1 = perm[j];
    if (s0 < 0 || s0 >= E || s1 < 0 || s1 >= E) {
      e |= 2;
      continue;
    }
    int fe = 0;
    ccl::unite_halving(L, (int)(s1 / 3), (int)(s0 / 3), F, &fe);
    e |= fe;
  }
  if (e) atomicOr(err, e);
}

// sweep s of the flatten pass; flags[s] = 1 when an element did not reach a root.  A sweep after a clean one does nothing.
__global__ __launch_bounds__(MT_BLOCK) void flatten_sweep_kernel(int* L, int64_t n, int s, int* flags) {
  if (s > 0 && __hip_atomic_load(flags + s - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
  bool open = false;
  MT_GRID_STRIDE(i, n) open |= !ccl::jump(L, (int)i);
  if (open) atomicOr(flags + s, 1);
}
__global__ void flatten_verify_kernel(const int* __restrict__ flags, int sweeps, int* err) {
  if (threadIdx.x == 0 && blockIdx.x == 0 && flags[sweeps - 1] != 0) atomicOr(err, 1);
}

// ---- roots: count -> scan -> emit ----------------------------------------------------------------------------------------
struct CountLayout {
  int64_t nblk, off_ofs, bytes;
};
inline CountLayout count_layout(int64_t n) {
  CountLayout L;
  L.nblk = (n + MT_PER_BLOCK - 1) / MT_PER_BLOCK;
  L.off_ofs = align256(L.nblk * 4);
  L.bytes = L.off_ofs + align256(L.nblk * 8);
  return L;
}

__device__ __forceinline__ bool is_root(const int* __restrict__ L, const uint8_t* __restrict__ used, int64_t i) {
  return L[i] == (int)i && (!used || used[i] != 0);
}

__global__ __launch_bounds__(MT_BLOCK) void roots_count_kernel(const int* __restrict__ L, const uint8_t* __restrict__ used, int64_t n,
                                                               int* __restrict__ blk_counts) {
  __shared__ int s[MT_BLOCK];
  const int64_t i0 = (int64_t)blockIdx.x * MT_PER_BLOCK + threadIdx.x * MT_ITEMS;
  int c = 0;
#pragma unroll
  for (int k = 0; k < MT_ITEMS; ++k)
    if (i0 + k < n && is_root(L, used, i0 + k)) ++c;
  int total;
  block_excl_scan<MT_BLOCK>(c, s, &total);
  if (threadIdx.x == 0) blk_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(MT_BLOCK) void roots_emit_kernel(const int* __restrict__ L, const uint8_t* __restrict__ used, int64_t n,
                                                              const int64_t* __restrict__ ofs, int* __restrict__ roots) {
  __shared__ int s[MT_BLOCK];
  const int64_t i0 = (int64_t)blockIdx.x * MT_PER_BLOCK + threadIdx.x * MT_ITEMS;
  bool r[MT_ITEMS];
  int c = 0;
#pragma unroll
  for (int k = 0; k < MT_ITEMS; ++k) {
    r[k] = i0 + k < n && is_root(L, used, i0 + k);
    c += r[k] ? 1 : 0;
  }
  int total;
  int64_t o = ofs[blockIdx.x] + block_excl_scan<MT_BLOCK>(c, s, &total);
#pragma unroll
  for (int k = 0; k < MT_ITEMS; ++k)
    if (r[k]) roots[o++] = (int)(i0 + k);
}

// first index in the ascending a[0 .. C) whose value is >= key
__device__ __forceinline__ int64_t lower_bound_i32(const int* __restrict__ a, int64_t C, int key) {
  int64_t lo = 0, hi = C;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(MT_BLOCK) void assign_kernel(const int* __restrict__ L, const uint8_t* __restrict__ used, int64_t n,
                                                          const int* __restrict__ roots, int64_t C, int* __restrict__ comp, int* err) {
  bool bad = false;
  MT_GRID_STRIDE(i, n) {
    if (used && used[i] == 0) {
      comp[i] = -1;
      continue;
    }
    const int r = L[i];
    const int64_t c = lower_bound_i32(roots, C, r);
    const bool ok = c < C && roots[c] == r;
    comp[i] = ok ? (int)c : -1;
    bad |= !ok;
  }
  if (bad) atomicOr(err, 1);                 // a label that is no root: the flatten pass did not finish
}

__global__ __launch_bounds__(MT_BLOCK) void spread_min_kernel(const int* __restrict__ faces, int64_t F, const int* __restrict__ face_comp,
                                                              unsigned* vertex_comp) {
  MT_GRID_STRIDE(f, F) {
    const unsigned c = (unsigned)face_comp[f];
#pragma unroll
    for (int k = 0; k < 3; ++k) atomicMin(vertex_comp + faces[3 * f + k], c);
  }
}

__global__ __launch_bounds__(MT_BLOCK) void face_from_vertex_kernel(const int* __restrict__ faces, int64_t F,
                                                                    const int* __restrict__ vertex_comp, int* __restrict__ face_comp) {
  MT_GRID_STRIDE(f, F) face_comp[f] = vertex_comp[faces[3 * f]];
}

__device__ __forceinline__ bool in_range(int64_t i, int64_t n) { return i >= 0 && i < n; }

// ---- edge statistics -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool slot_ascends(const int* __restrict__ faces, int64_t slot) {
  const int64_t f = slot / 3;
  const int k = (int)(slot - 3 * f);
  return faces[3 * f + k] < faces[3 * f + (k + 1) % 3];
}

// counts[K c + k] += v[k] over the wave, one atomic per distinct c: the lanes that hold the same c are summed by the butterfly
// first.  Called by every lane of the wave together (c < 0: nothing to add); at most 64 rounds.
template <int K>
__device__ __forceinline__ void wave_add(int* counts, int c, const int (&v)[K]) {
  const int lane = threadIdx.x & 63;
  uint64_t todo = __ballot(c >= 0);
  while (todo) {
    const int lead = __ffsll((unsigned long long)todo) - 1;
    const int want = __shfl(c, lead, 64);
    const bool mine = c == want;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      int t = mine ? v[k] : 0;
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) t += __shfl_xor(t, d, 64);
      if (lane == lead && t != 0) atomicAdd(counts + K * want + k, t);
    }
    todo &= ~__ballot(mine);
  }
}

// Every lane keeps the counts of the component it met last and hands them over when it meets another one (plain atomics: rare,
// the heads of one component lie together wherever its faces do) and, through wave_add, at the end: a mesh of one component
// costs a few thousand atomics on its three counters, not one per edge.  The sums are integers: any order gives the same.
constexpr int64_t ES_GRID_CAP = 1024;
__global__ __launch_bounds__(MT_BLOCK) void edge_stats_kernel(const int64_t* __restrict__ keys, const int64_t* __restrict__ perm,
                                                              const int* __restrict__ faces, int64_t E,
                                                              const int* __restrict__ face_comp, int C, int* counts) {
  int cur = -1, acc[3] = {0, 0, 0};
  MT_GRID_STRIDE(j, E) {
    const int64_t k = keys[j];
    if (k < 0 || (j > 0 && keys[j - 1] == k)) continue;
    int64_t m = 1;
    while (j + m < E && keys[j + m] == k) ++m;                // bounded by E
    if (!in_range(perm[j], E) || (m == 2 && !in_range(perm[j + 1], E))) continue;
    const int c = face_comp[perm[j] / 3];
    if (c < 0 || c >= C) continue;
    if (c != cur) {
      if (cur >= 0)
        for (int q = 0; q < 3; ++q)
          if (acc[q]) atomicAdd(counts + 3 * cur + q, acc[q]);
      cur = c, acc[0] = acc[1] = acc[2] = 0;
    }
    if (m == 1) ++acc[0];
    else if (m > 2) ++acc[1];
    else if (slot_ascends(faces, perm[j]) == slot_ascends(faces, perm[j + 1])) ++acc[2];
  }
  wave_add<3>(counts, cur, acc);
}

// ---- the component table -------------------------------------------------------------------------------------------------
// as edge_stats_kernel: a lane keeps the count of the component it met last
__global__ __launch_bounds__(MT_BLOCK) void vertex_count_kernel(const int* __restrict__ vertex_comp, int64_t V, int C, int* n_vertices) {
  int cur = -1, acc[1] = {0};
  MT_GRID_STRIDE(v, V) {
    const int c = vertex_comp[v];
    if (c < 0 || c >= C) continue;
    if (c != cur) {
      if (cur >= 0) atomicAdd(n_vertices + cur, acc[0]);
      cur = c, acc[0] = 0;
    }
    ++acc[0];
  }
  wave_add<1>(n_vertices, cur, acc);
}

__device__ __forceinline__ double face_area(const float* __restrict__ p0, const float* __restrict__ p1, const float* __restrict__ p2) {
  const double ux = (double)p1[0] - (double)p0[0], uy = (double)p1[1] - (double)p0[1], uz = (double)p1[2] - (double)p0[2];
  const double vx = (double)p2[0] - (double)p0[0], vy = (double)p2[1] - (double)p0[1], vz = (double)p2[2] - (double)p0[2];
  const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
  return 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
}

// per sorted position j: the area of face order[j] and its box, so that the one wave of a component only adds and compares
__global__ __launch_bounds__(MT_BLOCK) void face_measure_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                                const int64_t* __restrict__ order, int64_t F, double* __restrict__ warea,
                                                                float* __restrict__ wbox) {
  MT_GRID_STRIDE(j, F) {
    const int64_t f = order[j];
    double area = 0.0;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (f >= 0 && f < F) {
      const float* p0 = verts + 3 * (int64_t)faces[3 * f];
      const float* p1 = verts + 3 * (int64_t)faces[3 * f + 1];
      const float* p2 = verts + 3 * (int64_t)faces[3 * f + 2];
      area = face_area(p0, p1, p2);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        lo[a] = fminf(fminf(p0[a], p1[a]), p2[a]);
        hi[a] = fmaxf(fmaxf(p0[a], p1[a]), p2[a]);
      }
    }
    warea[j] = area;
#pragma unroll
    for (int a = 0; a < 3; ++a) wbox[6 * j + a] = lo[a], wbox[6 * j + 3 + a] = hi[a];
  }
}

constexpr int CW_AHEAD = 8;
__global__ __launch_bounds__(MT_BLOCK) void component_walk_kernel(const double* __restrict__ warea, const float* __restrict__ wbox,
                                                                  const int* __restrict__ sorted_comp, int64_t F, int C,
                                                                  int* __restrict__ n_faces, double* __restrict__ area,
                                                                  float* __restrict__ bbox_min, float* __restrict__ bbox_max) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * MT_WAVES + (threadIdx.x >> 6);
  if (c >= C) return;                                          // the whole wave; no barrier below
  const int64_t j0 = lower_bound_i32(sorted_comp, F, (int)c), j1 = lower_bound_i32(sorted_comp, F, (int)c + 1);
  if (lane == 0) n_faces[c] = (int)(j1 - j0);
  if (!warea) return;
  double acc = 0.0;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  // CW_AHEAD positions of the lane at a time, their loads in flight together; the additions stay in ascending order of
  // position, so the sum is the one of the plain loop
  for (int64_t j = j0 + lane; j < j1; j += 64 * CW_AHEAD) {
    double w[CW_AHEAD];
    float bx[CW_AHEAD][6];
#pragma unroll
    for (int u = 0; u < CW_AHEAD; ++u) {
      const int64_t ju = j + 64 * u;
      const bool live = ju < j1;
      w[u] = live ? warea[ju] : 0.0;
#pragma unroll
      for (int a = 0; a < 6; ++a) bx[u][a] = live ? wbox[6 * ju + a] : (a < 3 ? INFINITY : -INFINITY);
    }
#pragma unroll
    for (int u = 0; u < CW_AHEAD; ++u) {
      if (j + 64 * u < j1) acc = acc + w[u];
#pragma unroll
      for (int a = 0; a < 3; ++a) lo[a] = fminf(lo[a], bx[u][a]), hi[a] = fmaxf(hi[a], bx[u][3 + a]);
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    acc = acc + __shfl_xor(acc, d, 64);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = fminf(lo[a], __shfl_xor(lo[a], d, 64));
      hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], d, 64));
    }
  }
  if (lane == 0) {
    area[c] = acc;
#pragma unroll
    for (int a = 0; a < 3; ++a) bbox_min[3 * c + a] = lo[a], bbox_max[3 * c + a] = hi[a];
  }
}

// ---- compaction ----------------------------------------------------------------------------------------------------------
// workspace: used (V) u8 | face block counts (int) | face offsets (int64) | vertex block counts (int) | vertex offsets (int64)
struct CompactLayout {
  int64_t fblk, vblk, off_fcnt, off_fofs, off_vcnt, off_vofs, bytes;
};
inline CompactLayout compact_layout(int64_t F, int64_t V) {
  CompactLayout L;
  L.fblk = (F + MT_PER_BLOCK - 1) / MT_PER_BLOCK;
  L.vblk = (V + MT_PER_BLOCK - 1) / MT_PER_BLOCK;
  L.off_fcnt = align256(V);
  L.off_fofs = L.off_fcnt + align256(L.fblk * 4);
  L.off_vcnt = L.off_fofs + align256(L.fblk * 8);
  L.off_vofs = L.off_vcnt + align256(L.vblk * 4);
  L.bytes = L.off_vofs + align256(L.vblk * 8);
  return L;
}

__global__ __launch_bounds__(MT_BLOCK) void mark_used_kernel(const int* __restrict__ faces, int64_t F, const uint8_t* __restrict__ keep,
                                                             uint8_t* __restrict__ used) {
  MT_GRID_STRIDE(f, F) {
    if (keep && keep[f] == 0) continue;
    used[faces[3 * f]] = 1, used[faces[3 * f + 1]] = 1, used[faces[3 * f + 2]] = 1;
  }
}

__global__ __launch_bounds__(MT_BLOCK) void flags_count_kernel(const uint8_t* __restrict__ flag, int64_t n, int* __restrict__ blk_counts) {
  __shared__ int s[MT_BLOCK];
  const int64_t i0 = (int64_t)blockIdx.x * MT_PER_BLOCK + threadIdx.x * MT_ITEMS;
  int c = 0;
#pragma unroll
  for (int k = 0; k < MT_ITEMS; ++k)
    if (i0 + k < n && flag[i0 + k] != 0) ++c;
  int total;
  block_excl_scan<MT_BLOCK>(c, s, &total);
  if (threadIdx.x == 0) blk_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(MT_BLOCK) void vertices_emit_kernel(const uint8_t* __restrict__ used, int64_t V, const int64_t* __restrict__ ofs,
                                                                 int* __restrict__ vertex_map, int* __restrict__ kept_vertices) {
  __shared__ int s[MT_BLOCK];
  const int64_t i0 = (int64_t)blockIdx.x * MT_PER_BLOCK + threadIdx.x * MT_ITEMS;
  bool u[MT_ITEMS];
  int c = 0;
#pragma unroll
  for (int k = 0; k < MT_ITEMS; ++k) {
    u[k] = i0 + k < V && used[i0 + k] != 0;
    c += u[k] ? 1 : 0;
  }
  int total;
  int64_t o = ofs[blockIdx.x] + block_excl_scan<MT_BLOCK>(c, s, &total);
#pragma unroll
  for (int k = 0; k < MT_ITEMS; ++k) {
    if (i0 + k >= V) continue;
    if (u[k]) {
      vertex_map[i0 + k] = (int)o;
      kept_vertices[o] = (int)(i0 + k);
      ++o;
    } else {
      vertex_map[i0 + k] = -1;
    }
  }
}

__global__ __launch_bounds__(MT_BLOCK) void faces_emit_kernel(const int* __restrict__ faces, const uint8_t* __restrict__ keep, int64_t F,
                                                              const int64_t* __restrict__ ofs, const int* __restrict__ vertex_map,
                                                              int* __restrict__ out_faces) {
  __shared__ int s[MT_BLOCK];
  const int64_t i0 = (int64_t)blockIdx.x * MT_PER_BLOCK + threadIdx.x * MT_ITEMS;
  bool u[MT_ITEMS];
  int c = 0;
#pragma unroll
  for (int k = 0; k < MT_ITEMS; ++k) {
    u[k] = i0 + k < F && keep[i0 + k] != 0;
    c += u[k] ? 1 : 0;
  }
  int total;
  int64_t o = ofs[blockIdx.x] + block_excl_scan<MT_BLOCK>(c, s, &total);
#pragma unroll
  for (int k = 0; k < MT_ITEMS; ++k) {
    if (!u[k]) continue;
    const int64_t f = i0 + k;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int v = faces[3 * f + q];
      out_faces[3 * o + q] = vertex_map ? vertex_map[v] : v;
    }
    ++o;
  }
}

// ---- welding -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool bits_nan(int b) { return (b & 0x7fffffff) > 0x7f800000; }

__device__ __forceinline__ bool weld_head(const int* __restrict__ rows, const int64_t* __restrict__ keys, const int64_t* __restrict__ perm,
                                          int64_t V, int64_t j) {
  if (keys) return j == 0 || keys[j] < 0 || keys[j] != keys[j - 1];
  if (j == 0 || !in_range(perm[j], V) || !in_range(perm[j - 1], V)) return true;
  const int* a = rows + 3 * perm[j];
  if (bits_nan(a[0]) || bits_nan(a[1]) || bits_nan(a[2])) return true;
  const int* b = rows + 3 * perm[j - 1];
  return a[0] != b[0] || a[1] != b[1] || a[2] != b[2];
}

// perm is a permutation of 0 .. V - 1 (the indices of a sort); an entry outside that range is skipped and err |= 2
__global__ __launch_bounds__(MT_BLOCK) void weld_runs_kernel(const int* __restrict__ rows, const int64_t* __restrict__ keys,
                                                             const int64_t* __restrict__ perm, int64_t V, int* __restrict__ rep, int* err) {
  bool bad = false;
  MT_GRID_STRIDE(j, V) {
    if (!in_range(perm[j], V)) {
      bad = true;
      continue;
    }
    if (!weld_head(rows, keys, perm, V, j)) continue;
    const int r = (int)perm[j];
    rep[r] = r;
    for (int64_t k = j + 1; k < V && !weld_head(rows, keys, perm, V, k); ++k)      // bounded by V
      if (in_range(perm[k], V)) rep[perm[k]] = r;
  }
  if (bad) atomicOr(err, 2);
}

__global__ __launch_bounds__(MT_BLOCK) void remap_faces_kernel(const int* __restrict__ faces, int64_t F, const int* __restrict__ remap,
                                                               int drop_degenerate, int* __restrict__ out, uint8_t* __restrict__ keep) {
  MT_GRID_STRIDE(f, F) {
    const int a = remap[faces[3 * f]], b = remap[faces[3 * f + 1]], c = remap[faces[3 * f + 2]];
    out[3 * f] = a, out[3 * f + 1] = b, out[3 * f + 2] = c;
    keep[f] = (drop_degenerate && (a == b || b == c || c == a)) ? 0 : 1;
  }
}

// ---- orientation repair -------------------------------------------------------------------------
__device__ __forceinline__ bool face_degenerate(int a, int b, int c) { return a == b || b == c || c == a; }

__global__ __launch_bounds__(MT_BLOCK) void orient_keys_kernel(const int* __restrict__ faces, int64_t F, int64_t* __restrict__ keys) {
  MT_GRID_STRIDE(f, F) {
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    const bool dead = face_degenerate(a, b, c);
    keys[3 * f] = dead ? -1 : ccl::edge_key(a, b);
    keys[3 * f + 1] = dead ? -1 : ccl::edge_key(b, c);
    keys[3 * f + 2] = dead ? -1 : ccl::edge_key(c, a);
  }
}

__global__ __launch_bounds__(MT_BLOCK) void orient_init_kernel(int* __restrict__ W, int64_t n) {
  MT_GRID_STRIDE(i, n) W[i] = (int)i << 1;
}

// sorted position j belongs to a run of exactly two equal keys >= 0
__device__ __forceinline__ bool in_pair(const int64_t* __restrict__ keys, int64_t E, int64_t j, bool* head) {
  const int64_t k = keys[j];
  if (k < 0) return false;
  const bool prev = j > 0 && keys[j - 1] == k, next = j + 1 < E && keys[j + 1] == k;
  *head = next;
  if (prev == next) return false;                              // alone, or inside a longer run
  return next ? !(j + 2 < E && keys[j + 2] == k) : !(j >= 2 && keys[j - 2] == k);
}

// the link whose run begins at sorted position j: faces f < g and rel = 1 when both run the edge the same way
__device__ __forceinline__ bool link_at(const int64_t* __restrict__ keys, const int64_t* __restrict__ perm, const int* __restrict__ faces,
                                        int64_t E, int64_t j, int* f, int* g, int* rel, int* e) {
  bool head;
  if (!in_pair(keys, E, j, &head) || !head) return false;
  const int64_t s0 = perm[j], s1 = perm[j + 1];
  if (!in_range(s0, E) || !in_range(s1, E)) {
    *e |= 2;
    return false;
  }
  *f = (int)(s0 / 3), *g = (int)(s1 / 3);
  *rel = slot_ascends(faces, s0) == slot_ascends(faces, s1) ? 1 : 0;
  return true;
}

__global__ __launch_bounds__(MT_BLOCK) void orient_union_kernel(const int64_t* __restrict__ keys, const int64_t* __restrict__ perm,
                                                                const int* __restrict__ faces, int64_t E, int F, int* W, int* err) {
  // A wave takes 64 neighbouring sorted positions (coalesced), but the waves take their chunks in a scattered order: chunk
  // (w * odd) mod 2^k is a bijection of [0, 2^k), 2^k >= the number of chunks.  Neighbouring positions are neighbouring faces in
  // a mesh that was written out along its surface, and waves that run at the same time would otherwise hang face after face
  // under its predecessor -- one long chain that every later find has to walk (the ascending ladder of tools/time_meshorient.py).
  // The order of the unions does not change their result.
  int e = 0;
  const int64_t chunks = (E + 63) / 64, waves = (int64_t)gridDim.x * MT_WAVES;
  int64_t pow2 = 1;
  while (pow2 < chunks) pow2 <<= 1;
  for (int64_t w = (int64_t)blockIdx.x * MT_WAVES + (threadIdx.x >> 6); w < pow2; w += waves) {
    const int64_t chunk = (int64_t)(((uint64_t)w * 0x9E3779B1ull) & (uint64_t)(pow2 - 1));
    const int64_t j = chunk * 64 + (threadIdx.x & 63);
    if (chunk >= chunks || j >= E) continue;
    int f, g, rel;
    if (!link_at(keys, perm, faces, E, j, &f, &g, &rel, &e)) continue;
    int fe = 0;
    ccl::unite_parity(W, g, f, rel, F, &fe);
    e |= fe;
  }
  if (e) atomicOr(err, e);
}

__global__ __launch_bounds__(MT_BLOCK) void orient_sweep_kernel(int* W, int64_t n, int s, int* flags) {
  if (s > 0 && __hip_atomic_load(flags + s - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
  bool open = false;
  MT_GRID_STRIDE(i, n) open |= !ccl::jump_parity(W, (int)i);
  if (open) atomicOr(flags + s, 1);
}

__global__ __launch_bounds__(MT_BLOCK) void orient_split_kernel(const int* __restrict__ W, int64_t n, int* __restrict__ labels,
                                                                uint8_t* __restrict__ flip0) {
  MT_GRID_STRIDE(i, n) {
    const int w = W[i];
    labels[i] = w >> 1;
    flip0[i] = (uint8_t)(w & 1);
  }
}

// counts[2 c + 0] += the edge slots of patch c that lie in no run of two (boundary or non-manifold: the patch is not closed),
// counts[2 c + 1] += its links with rel == 1; bad[c] |= 1 when a link contradicts flip0.  Lanes keep the counts of the patch they
// met last, as edge_stats_kernel does.
__global__ __launch_bounds__(MT_BLOCK) void orient_check_kernel(const int64_t* __restrict__ keys, const int64_t* __restrict__ perm,
                                                                const int* __restrict__ faces, int64_t E,
                                                                const int* __restrict__ face_patch, int C,
                                                                const uint8_t* __restrict__ flip0, int* bad, int* counts, int* err) {
  int cur = -1, acc[2] = {0, 0}, e = 0;
  MT_GRID_STRIDE(j, E) {
    if (keys[j] < 0) continue;
    const int64_t s = perm[j];
    if (!in_range(s, E)) {
      e |= 2;
      continue;
    }
    const int c = face_patch[s / 3];
    if (c < 0 || c >= C) continue;
    bool head;
    const bool pair = in_pair(keys, E, j, &head);
    int f, g, rel = 0;
    if (pair && head && link_at(keys, perm, faces, E, j, &f, &g, &rel, &e)) {
      if ((flip0[f] ^ flip0[g]) != rel) atomicOr(bad + c, 1);
    }
    if (c != cur) {
      if (cur >= 0)
        for (int q = 0; q < 2; ++q)
          if (acc[q]) atomicAdd(counts + 2 * cur + q, acc[q]);
      cur = c, acc[0] = acc[1] = 0;
    }
    acc[0] += pair ? 0 : 1;
    acc[1] += rel;
  }
  wave_add<2>(counts, cur, acc);
  if (e) atomicOr(err, e);
}

__global__ __launch_bounds__(MT_BLOCK) void orient_clear_kernel(const int* __restrict__ face_patch, const int* __restrict__ bad, int64_t F,
                                                                int C, uint8_t* __restrict__ flip0) {
  MT_GRID_STRIDE(f, F) {
    const int c = face_patch[f];
    if (c >= 0 && c < C && bad[c] != 0) flip0[f] = 0;
  }
}

// a float as an int that orders the same way (an involution: the same function decodes), so that the exact minima and maxima of a
// patch's box can be taken by INTEGER atomics -- their result does not depend on their order; -0 sorts below +0
__device__ __forceinline__ int float_order(int bits) { return bits >= 0 ? bits : bits ^ 0x7fffffff; }
__device__ __forceinline__ int order_of_float(float x) { return float_order(__float_as_int(x)); }
__device__ __forceinline__ float float_of_order(int k) { return __int_as_float(float_order(k)); }

__global__ __launch_bounds__(MT_BLOCK) void orient_box_init_kernel(int* __restrict__ box, int64_t C) {
  MT_GRID_STRIDE(i, 6 * C) box[i] = order_of_float(i % 6 < 3 ? INFINITY : -INFINITY);
}

// per face f of patch c: n_flip0[c] += flip0[f] and, with verts, box[c] = min / max with the face's corners (box (C,6) int =
// float_order of lo.xyz, hi.xyz).  A wave whose live lanes all hold the same patch combines them over the butterfly first and
// issues one set of atomics; the trip count is the same for every lane of a block, so every lane takes part in the shuffles.
__global__ __launch_bounds__(MT_BLOCK) void orient_gather_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                                 const int* __restrict__ face_patch, const uint8_t* __restrict__ flip0,
                                                                 int64_t F, int C, int* box, int* n_flip0) {
  const int lane = threadIdx.x & 63;
  for (int64_t base = (int64_t)blockIdx.x * MT_BLOCK; base < F; base += (int64_t)gridDim.x * MT_BLOCK) {
    const int64_t f = base + threadIdx.x;
    int c = f < F ? face_patch[f] : -1;
    const bool live = c >= 0 && c < C;
    int fl = live && flip0[f] != 0 ? 1 : 0;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (live && verts) {
      const float* p0 = verts + 3 * (int64_t)faces[3 * f];
      const float* p1 = verts + 3 * (int64_t)faces[3 * f + 1];
      const float* p2 = verts + 3 * (int64_t)faces[3 * f + 2];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        lo[a] = fminf(fminf(p0[a], p1[a]), p2[a]);
        hi[a] = fmaxf(fmaxf(p0[a], p1[a]), p2[a]);
      }
    }
    const uint64_t alive = __ballot(live);
    if (alive == 0) continue;                                  // the whole wave
    const int lead = __ffsll((unsigned long long)alive) - 1;
    const int c0 = __shfl(c, lead, 64);
    const bool uniform = __ballot(live && c != c0) == 0;
    if (uniform) {
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) {
        fl += __shfl_xor(fl, d, 64);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          lo[a] = fminf(lo[a], __shfl_xor(lo[a], d, 64));
          hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], d, 64));
        }
      }
    }
    if (uniform ? lane == lead : live) {
      if (fl) atomicAdd(n_flip0 + c, fl);
      if (verts) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          atomicMin(box + 6 * (int64_t)c + a, order_of_float(lo[a]));
          atomicMax(box + 6 * (int64_t)c + 3 + a, order_of_float(hi[a]));
        }
      }
    }
  }
}

// per sorted position j, face (a, b, d) = order[j] with b and d swapped when flip0 is set,
// c = 0.5 * ((double)lo + (double)hi) per axis of the patch's fp32 vertex box:
//   pa = (double)a - c, pb = (double)b - c, pd = (double)d - c (per axis),
//   cx = pb.y pd.z - pb.z pd.y, cy = pb.z pd.x - pb.x pd.z, cz = pb.x pd.y - pb.y pd.x (each product rounded, then the difference),
//   term = (pa.x cx + pa.y cy) + pa.z cz;  a degenerate face's term is +0.0.
// Swapping b and d negates cx, cy, cz and with them the term exactly, so a flipped patch's sum is the exact negative.
__global__ __launch_bounds__(MT_BLOCK) void orient_face_term_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                                    const int64_t* __restrict__ order, const int* __restrict__ sorted_patch,
                                                                    const uint8_t* __restrict__ flip0, const int* __restrict__ box,
                                                                    int64_t F, int C, double* __restrict__ wterm) {
  MT_GRID_STRIDE(j, F) {
    const int64_t f = order[j];
    const int c = sorted_patch[j];
    double term = 0.0;
    if (in_range(f, F) && c >= 0 && c < C) {
      const int ia = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
      if (!face_degenerate(ia, i1, i2)) {
        const bool fl = flip0[f] != 0;
        const float* a = verts + 3 * (int64_t)ia;
        const float* b = verts + 3 * (int64_t)(fl ? i2 : i1);
        const float* d = verts + 3 * (int64_t)(fl ? i1 : i2);
        const int* bc = box + 6 * (int64_t)c;
        double cc[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) cc[k] = 0.5 * ((double)float_of_order(bc[k]) + (double)float_of_order(bc[3 + k]));
        const double ax = (double)a[0] - cc[0], ay = (double)a[1] - cc[1], az = (double)a[2] - cc[2];
        const double bx = (double)b[0] - cc[0], by = (double)b[1] - cc[1], bz = (double)b[2] - cc[2];
        const double dx = (double)d[0] - cc[0], dy = (double)d[1] - cc[1], dz = (double)d[2] - cc[2];
        const double cx = by * dz - bz * dy, cy = bz * dx - bx * dz, cz = bx * dy - by * dx;
        term = (ax * cx + ay * cy) + az * cz;
      }
    }
    wterm[j] = term;
  }
}

// ONE WAVE PER PATCH over run = [lower_bound(sorted_patch, c), lower_bound(sorted_patch, c + 1)): n_faces[c] = its length;
// lane l takes the run's positions l, l + 64, l + 128, ... in that (ascending) order from acc = 0.0: acc = acc + term; then the
// lanes combine over the fixed tree of distances 32, 16, 8, 4, 2, 1: a[l] = a[l] + a[l ^ d];
// lane 0: s = acc, sign[c] = outward and the patch is orientable and s < 0, signed_volume[c] = (sign ? -s : s) / 6,
// n_flipped[c] = sign ? n_faces - n_flip0 : n_flip0.  wterm == NULL: the counts only, sign = 0.
__global__ __launch_bounds__(MT_BLOCK) void orient_patch_sum_kernel(const double* __restrict__ wterm, const int* __restrict__ sorted_patch,
                                                                    const int* __restrict__ n_flip0, const int* __restrict__ bad,
                                                                    int64_t F, int C, int outward, int* __restrict__ n_faces,
                                                                    int* __restrict__ n_flipped, uint8_t* __restrict__ sign,
                                                                    double* __restrict__ volume) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * MT_WAVES + (threadIdx.x >> 6);
  if (c >= C) return;                                          // the whole wave; no barrier below
  const int64_t j0 = lower_bound_i32(sorted_patch, F, (int)c), j1 = lower_bound_i32(sorted_patch, F, (int)c + 1);
  double acc = 0.0;
  // CW_AHEAD positions of the lane at a time, their loads in flight together; the additions stay in ascending order of position
  for (int64_t j = j0 + lane; wterm && j < j1; j += 64 * CW_AHEAD) {
    double w[CW_AHEAD];
#pragma unroll
    for (int u = 0; u < CW_AHEAD; ++u) w[u] = j + 64 * u < j1 ? wterm[j + 64 * u] : 0.0;
#pragma unroll
    for (int u = 0; u < CW_AHEAD; ++u)
      if (j + 64 * u < j1) acc = acc + w[u];
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) acc = acc + __shfl_xor(acc, d, 64);
  if (lane == 0) {
    const int n = (int)(j1 - j0), nf = n_flip0[c];
    const bool neg = wterm && outward && bad[c] == 0 && acc < 0.0;
    n_faces[c] = n;
    n_flipped[c] = neg ? n - nf : nf;
    sign[c] = neg ? 1 : 0;
    if (volume) volume[c] = (neg ? -acc : acc) / 6.0;
  }
}

__global__ __launch_bounds__(MT_BLOCK) void orient_apply_kernel(const int* __restrict__ faces, int64_t F, const int* __restrict__ face_patch,
                                                                int C, const uint8_t* __restrict__ flip0, const uint8_t* __restrict__ sign,
                                                                int* __restrict__ out_faces, uint8_t* __restrict__ flip) {
  MT_GRID_STRIDE(f, F) {
    const int c = face_patch[f];
    const int a = faces[3 * f], b = faces[3 * f + 1], d = faces[3 * f + 2];
    const bool dead = face_degenerate(a, b, d);
    const bool fl = !dead && ((flip0[f] != 0) != (c >= 0 && c < C && sign[c] != 0));
    out_faces[3 * f] = a, out_faces[3 * f + 1] = fl ? d : b, out_faces[3 * f + 2] = fl ? b : d;
    flip[f] = fl ? 1 : 0;
  }
}

#define MT_LAUNCH(kernel, n, ...)                                                                            \
  do {                                                                                                         \
    hipLaunchKernelGGL(kernel, dim3(mt_grid(n)), dim3(MT_BLOCK), 0, (hipStream_t)stream, __VA_ARGS__);         \
    CNR_LAUNCH_CHECK();                                                                                        \
  } while (0)

inline bool sizes_ok(int64_t F, int64_t V) { return F >= 1 && V >= 1 && F <= INDEX_LIMIT / 3 && V <= INDEX_LIMIT; }
}  // namespace

// ---- entry points --------------------------------------------------------------------------------------------------------
extern "C" int cnr_mesh_check_faces(const int* faces, int64_t F, int64_t V, int* err, void* stream) {
  if (!faces || !err) return CNR_E_ARG;
  if (!sizes_ok(F, V)) return CNR_E_SHAPE;
  MT_LAUNCH(check_faces_kernel, 3 * F, faces, 3 * F, (int)V, err);
  return CNR_OK;
}

extern "C" int cnr_mesh_labels_init(int* labels, int64_t n, void* stream) {
  if (!labels) return CNR_E_ARG;
  if (n < 1 || n > INDEX_LIMIT) return CNR_E_SHAPE;
  MT_LAUNCH(labels_init_kernel, n, labels, n);
  return CNR_OK;
}

extern "C" int cnr_mesh_union_pairs(const int* pairs, int64_t m, int64_t n, int* labels, int* err, void* stream) {
  if (!pairs || !labels || !err) return CNR_E_ARG;
  if (m < 1 || n < 1 || n > INDEX_LIMIT) return CNR_E_SHAPE;
  MT_LAUNCH(union_pairs_kernel, m, pairs, m, (int)n, labels, err);
  return CNR_OK;
}

extern "C" int cnr_mesh_union_faces(const int* faces, int64_t F, int64_t V, int* labels, uint8_t* used, int* err, void* stream) {
  if (!faces || !labels || !used || !err) return CNR_E_ARG;
  if (!sizes_ok(F, V)) return CNR_E_SHAPE;
  MT_LAUNCH(union_faces_kernel, F, faces, F, (int)V, labels, used, err);
  return CNR_OK;
}

extern "C" int cnr_mesh_edge_keys(const int* faces, int64_t F, int64_t* keys, void* stream) {
  if (!faces || !keys) return CNR_E_ARG;
  if (F < 1 || F > INDEX_LIMIT / 3) return CNR_E_SHAPE;
  MT_LAUNCH(edge_keys_kernel, F, faces, F, keys);
  return CNR_OK;
}

extern "C" int cnr_mesh_union_edges(const int64_t* sorted_keys, const int64_t* perm, int64_t F, int* labels, int* err, void* stream) {
  if (!sorted_keys || !perm || !labels || !err) return CNR_E_ARG;
  if (F < 1 || F > INDEX_LIMIT / 3) return CNR_E_SHAPE;
  MT_LAUNCH(union_edges_kernel, 3 * F, sorted_keys, perm, 3 * F, (int)F, labels, err);
  return CNR_OK;
}

extern "C" int64_t cnr_mesh_flatten_workspace_bytes(int64_t n) {
  if (n < 1 || n > INDEX_LIMIT) return CNR_E_SHAPE;
  return align256((int64_t)ccl::sweeps_for(n) * 4);
}

extern "C" int cnr_mesh_flatten(int* labels, int64_t n, void* workspace, int* err, void* stream) {
  if (!labels || !workspace || !err) return CNR_E_ARG;
  if (n < 1 || n > INDEX_LIMIT) return CNR_E_SHAPE;
  const int sweeps = ccl::sweeps_for(n);
  int* flags = (int*)workspace;
  hipError_t e = hipMemsetAsync(flags, 0, (size_t)sweeps * 4, (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  for (int s = 0; s < sweeps; ++s) MT_LAUNCH(flatten_sweep_kernel, n, labels, n, s, flags);
  hipLaunchKernelGGL(flatten_verify_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const int*)flags, sweeps, err);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int64_t cnr_mesh_roots_workspace_bytes(int64_t n) {
  if (n < 1 || n > INDEX_LIMIT) return CNR_E_SHAPE;
  return count_layout(n).bytes;
}

extern "C" int cnr_mesh_roots_count(const int* labels, const uint8_t* used, int64_t n, void* workspace, int64_t* count_out,
                                    void* stream) {
  if (!labels || !workspace || !count_out) return CNR_E_ARG;
  if (n < 1 || n > INDEX_LIMIT) return CNR_E_SHAPE;
  const CountLayout L = count_layout(n);
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(roots_count_kernel, dim3((unsigned)L.nblk), dim3(MT_BLOCK), 0, (hipStream_t)stream, labels, used, n, (int*)ws);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL((blocks_scan_kernel<1, int64_t, int>), dim3(1), dim3(SCAN_THREADS), 0, (hipStream_t)stream, (const int*)ws, L.nblk,
                     (int64_t*)(ws + L.off_ofs), count_out);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_mesh_roots_emit(const int* labels, const uint8_t* used, int64_t n, const void* workspace, int* roots, void* stream) {
  if (!labels || !workspace || !roots) return CNR_E_ARG;
  if (n < 1 || n > INDEX_LIMIT) return CNR_E_SHAPE;
  const CountLayout L = count_layout(n);
  const char* ws = (const char*)workspace;
  hipLaunchKernelGGL(roots_emit_kernel, dim3((unsigned)L.nblk), dim3(MT_BLOCK), 0, (hipStream_t)stream, labels, used, n,
                     (const int64_t*)(ws + L.off_ofs), roots);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_mesh_assign(const int* labels, const uint8_t* used, int64_t n, const int* roots, int64_t C, int* comp, int* err,
                               void* stream) {
  if (!labels || !roots || !comp || !err) return CNR_E_ARG;
  if (n < 1 || n > INDEX_LIMIT || C < 1 || C > n) return CNR_E_SHAPE;
  MT_LAUNCH(assign_kernel, n, labels, used, n, roots, C, comp, err);
  return CNR_OK;
}

extern "C" int cnr_mesh_cross_component(const int* faces, int64_t F, int64_t V, int mode, int* face_component, int* vertex_component,
                                        void* stream) {
  if (!faces || !face_component || !vertex_component) return CNR_E_ARG;
  if (!sizes_ok(F, V) || (mode != 0 && mode != 1)) return CNR_E_SHAPE;
  if (mode == 0) {
    hipError_t e = hipMemsetAsync(vertex_component, 0xff, (size_t)V * 4, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    MT_LAUNCH(spread_min_kernel, F, faces, F, (const int*)face_component, (unsigned*)vertex_component);
  } else {
    MT_LAUNCH(face_from_vertex_kernel, F, faces, F, (const int*)vertex_component, face_component);
  }
  return CNR_OK;
}

extern "C" int cnr_mesh_edge_stats(const int64_t* sorted_keys, const int64_t* perm, const int* faces, int64_t F,
                                   const int* face_component, int64_t C, int* counts, void* stream) {
  if (!sorted_keys || !perm || !faces || !face_component || !counts) return CNR_E_ARG;
  if (F < 1 || F > INDEX_LIMIT / 3 || C < 1 || C > INDEX_LIMIT / 3) return CNR_E_SHAPE;
  hipLaunchKernelGGL(edge_stats_kernel, dim3(grid_of(3 * F, MT_BLOCK, ES_GRID_CAP)), dim3(MT_BLOCK), 0, (hipStream_t)stream, sorted_keys,
                     perm, faces, 3 * F, face_component, (int)C, counts);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int64_t cnr_mesh_component_stats_workspace_bytes(int64_t F) {
  if (F < 1 || F > INDEX_LIMIT / 3) return CNR_E_SHAPE;
  return align256(F * 8) + align256(F * 24);
}

extern "C" int cnr_mesh_component_stats(const float* verts, const int* faces, const int64_t* order, const int* sorted_component,
                                        int64_t F, int64_t V, int64_t C, const int* vertex_component, void* workspace, int* n_faces,
                                        int* n_vertices, double* area, float* bbox_min, float* bbox_max, void* stream) {
  if (!faces || !order || !sorted_component || !vertex_component || !n_faces || !n_vertices) return CNR_E_ARG;
  if (verts && (!workspace || !area || !bbox_min || !bbox_max)) return CNR_E_ARG;
  if (!sizes_ok(F, V) || C < 1 || C > INDEX_LIMIT / 3) return CNR_E_SHAPE;
  hipError_t e = hipMemsetAsync(n_vertices, 0, (size_t)C * 4, (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(vertex_count_kernel, dim3(grid_of(V, MT_BLOCK, ES_GRID_CAP)), dim3(MT_BLOCK), 0, (hipStream_t)stream, vertex_component,
                     V, (int)C, n_vertices);
  CNR_LAUNCH_CHECK();
  double* warea = verts ? (double*)workspace : nullptr;
  float* wbox = verts ? (float*)((char*)workspace + align256(F * 8)) : nullptr;
  if (verts) MT_LAUNCH(face_measure_kernel, F, verts, faces, order, F, warea, wbox);
  hipLaunchKernelGGL(component_walk_kernel, dim3((unsigned)((C + MT_WAVES - 1) / MT_WAVES)), dim3(MT_BLOCK), 0, (hipStream_t)stream,
                     (const double*)warea, (const float*)wbox, sorted_component, F, (int)C, n_faces, area, bbox_min, bbox_max);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int64_t cnr_mesh_compact_workspace_bytes(int64_t F, int64_t V) {
  if (!sizes_ok(F, V)) return CNR_E_SHAPE;
  return compact_layout(F, V).bytes;
}

extern "C" int cnr_mesh_compact_count(const int* faces, int64_t F, int64_t V, const uint8_t* keep_face, int reindex, void* workspace,
                                      int64_t* counts_out, void* stream) {
  if (!faces || !keep_face || !workspace || !counts_out) return CNR_E_ARG;
  if (!sizes_ok(F, V)) return CNR_E_SHAPE;
  const CompactLayout L = compact_layout(F, V);
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(flags_count_kernel, dim3((unsigned)L.fblk), dim3(MT_BLOCK), 0, (hipStream_t)stream, keep_face, F, (int*)(ws + L.off_fcnt));
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL((blocks_scan_kernel<1, int64_t, int>), dim3(1), dim3(SCAN_THREADS), 0, (hipStream_t)stream,
                     (const int*)(ws + L.off_fcnt), L.fblk, (int64_t*)(ws + L.off_fofs), counts_out);
  CNR_LAUNCH_CHECK();
  hipError_t e = reindex ? hipMemsetAsync(ws, 0, (size_t)V, (hipStream_t)stream) : hipMemsetAsync(counts_out + 1, 0, 8, (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  if (!reindex) return CNR_OK;
  MT_LAUNCH(mark_used_kernel, F, faces, F, keep_face, (uint8_t*)ws);
  hipLaunchKernelGGL(flags_count_kernel, dim3((unsigned)L.vblk), dim3(MT_BLOCK), 0, (hipStream_t)stream, (const uint8_t*)ws, V,
                     (int*)(ws + L.off_vcnt));
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL((blocks_scan_kernel<1, int64_t, int>), dim3(1), dim3(SCAN_THREADS), 0, (hipStream_t)stream,
                     (const int*)(ws + L.off_vcnt), L.vblk, (int64_t*)(ws + L.off_vofs), counts_out + 1);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_mesh_compact_emit(const int* faces, int64_t F, int64_t V, const uint8_t* keep_face, int reindex, const void* workspace,
                                     int* out_faces, int* vertex_map, int* kept_vertices, void* stream) {
  if (!faces || !keep_face || !workspace || !out_faces) return CNR_E_ARG;
  if (reindex && (!vertex_map || !kept_vertices)) return CNR_E_ARG;
  if (!sizes_ok(F, V)) return CNR_E_SHAPE;
  const CompactLayout L = compact_layout(F, V);
  const char* ws = (const char*)workspace;
  if (reindex) {
    hipLaunchKernelGGL(vertices_emit_kernel, dim3((unsigned)L.vblk), dim3(MT_BLOCK), 0, (hipStream_t)stream, (const uint8_t*)ws, V,
                       (const int64_t*)(ws + L.off_vofs), vertex_map, kept_vertices);
    CNR_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(faces_emit_kernel, dim3((unsigned)L.fblk), dim3(MT_BLOCK), 0, (hipStream_t)stream, faces, keep_face, F,
                     (const int64_t*)(ws + L.off_fofs), reindex ? (const int*)vertex_map : (const int*)nullptr, out_faces);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_weld_runs(const int* rows, const int64_t* sorted_keys, const int64_t* perm, int64_t V, int* rep, int* err, void* stream) {
  if (!perm || !rep || !err || (!rows && !sorted_keys) || (rows && sorted_keys)) return CNR_E_ARG;
  if (V < 1 || V > INDEX_LIMIT) return CNR_E_SHAPE;
  MT_LAUNCH(weld_runs_kernel, V, rows, sorted_keys, perm, V, rep, err);
  return CNR_OK;
}

extern "C" int cnr_mesh_remap_faces(const int* faces, int64_t F, const int* remap, int drop_degenerate, int* out_faces, uint8_t* keep,
                                    void* stream) {
  if (!faces || !remap || !out_faces || !keep) return CNR_E_ARG;
  if (F < 1 || F > INDEX_LIMIT / 3) return CNR_E_SHAPE;
  MT_LAUNCH(remap_faces_kernel, F, faces, F, remap, drop_degenerate, out_faces, keep);
  return CNR_OK;
}

// ---- orientation repair ----------------------------------------------------------------------------------------------------
extern "C" int cnr_mesh_orient_keys(const int* faces, int64_t F, int64_t* keys, void* stream) {
  if (!faces || !keys) return CNR_E_ARG;
  if (F < 1 || F > INDEX_LIMIT / 3) return CNR_E_SHAPE;
  MT_LAUNCH(orient_keys_kernel, F, faces, F, keys);
  return CNR_OK;
}

extern "C" int cnr_mesh_orient_union(const int64_t* sorted_keys, const int64_t* perm, const int* faces, int64_t F, int* words, int* err,
                                     void* stream) {
  if (!sorted_keys || !perm || !faces || !words || !err) return CNR_E_ARG;
  if (F < 1 || F > INDEX_LIMIT / 3) return CNR_E_SHAPE;
  MT_LAUNCH(orient_init_kernel, F, words, F);
  MT_LAUNCH(orient_union_kernel, 3 * F, sorted_keys, perm, faces, 3 * F, (int)F, words, err);
  return CNR_OK;
}

extern "C" int cnr_mesh_orient_flatten(int* words, int64_t F, void* workspace, int* labels, uint8_t* flip0, int* err, void* stream) {
  if (!words || !workspace || !labels || !flip0 || !err) return CNR_E_ARG;
  if (F < 1 || F > INDEX_LIMIT / 3) return CNR_E_SHAPE;
  const int sweeps = ccl::sweeps_for(F);
  int* flags = (int*)workspace;
  hipError_t e = hipMemsetAsync(flags, 0, (size_t)sweeps * 4, (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  for (int s = 0; s < sweeps; ++s) MT_LAUNCH(orient_sweep_kernel, F, words, F, s, flags);
  hipLaunchKernelGGL(flatten_verify_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const int*)flags, sweeps, err);
  CNR_LAUNCH_CHECK();
  MT_LAUNCH(orient_split_kernel, F, (const int*)words, F, labels, flip0);
  return CNR_OK;
}

extern "C" int cnr_mesh_orient_check(const int64_t* sorted_keys, const int64_t* perm, const int* faces, int64_t F, const int* face_patch,
                                     int64_t C, uint8_t* flip0, int* bad, int* counts, int* err, void* stream) {
  if (!sorted_keys || !perm || !faces || !face_patch || !flip0 || !bad || !counts || !err) return CNR_E_ARG;
  if (F < 1 || F > INDEX_LIMIT / 3 || C < 1 || C > F) return CNR_E_SHAPE;
  hipError_t e = hipMemsetAsync(bad, 0, (size_t)C * 4, (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  e = hipMemsetAsync(counts, 0, (size_t)C * 8, (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(orient_check_kernel, dim3(grid_of(3 * F, MT_BLOCK, ES_GRID_CAP)), dim3(MT_BLOCK), 0, (hipStream_t)stream, sorted_keys,
                     perm, faces, 3 * F, face_patch, (int)C, (const uint8_t*)flip0, bad, counts, err);
  CNR_LAUNCH_CHECK();
  MT_LAUNCH(orient_clear_kernel, F, face_patch, (const int*)bad, F, (int)C, flip0);
  return CNR_OK;
}

// workspace: boxes (C <= F, 6) int | terms (F) f64 | flip0 counts (C <= F) int
extern "C" int64_t cnr_mesh_orient_stats_workspace_bytes(int64_t F) {
  if (F < 1 || F > INDEX_LIMIT / 3) return CNR_E_SHAPE;
  return align256(F * 24) + align256(F * 8) + align256(F * 4);
}

extern "C" int cnr_mesh_orient_stats(const float* verts, const int* faces, const int64_t* order, const int* sorted_patch,
                                     const int* face_patch, int64_t F, int64_t V, int64_t C, const uint8_t* flip0, const int* bad,
                                     int outward, void* workspace, int* n_faces, int* n_flipped, uint8_t* sign, double* signed_volume,
                                     void* stream) {
  if (!faces || !order || !sorted_patch || !face_patch || !flip0 || !bad || !workspace || !n_faces || !n_flipped || !sign) return CNR_E_ARG;
  if (verts && !signed_volume) return CNR_E_ARG;
  if (!sizes_ok(F, V) || C < 1 || C > F) return CNR_E_SHAPE;
  int* box = (int*)workspace;
  double* wterm = verts ? (double*)((char*)workspace + align256(F * 24)) : nullptr;
  int* n_flip0 = (int*)((char*)workspace + align256(F * 24) + align256(F * 8));
  hipError_t e = hipMemsetAsync(n_flip0, 0, (size_t)C * 4, (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  if (verts) MT_LAUNCH(orient_box_init_kernel, 6 * C, box, C);
  MT_LAUNCH(orient_gather_kernel, F, verts, faces, face_patch, flip0, F, (int)C, box, n_flip0);
  if (verts) MT_LAUNCH(orient_face_term_kernel, F, verts, faces, order, sorted_patch, flip0, (const int*)box, F, (int)C, wterm);
  hipLaunchKernelGGL(orient_patch_sum_kernel, dim3((unsigned)((C + MT_WAVES - 1) / MT_WAVES)), dim3(MT_BLOCK), 0, (hipStream_t)stream,
                     (const double*)wterm, sorted_patch, (const int*)n_flip0, bad, F, (int)C, outward, n_faces, n_flipped, sign,
                     verts ? signed_volume : (double*)nullptr);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_mesh_orient_apply(const int* faces, int64_t F, const int* face_patch, int64_t C, const uint8_t* flip0,
                                     const uint8_t* sign, int* out_faces, uint8_t* flip, void* stream) {
  if (!faces || !face_patch || !flip0 || !sign || !out_faces || !flip) return CNR_E_ARG;
  if (F < 1 || F > INDEX_LIMIT / 3 || C < 1 || C > F) return CNR_E_SHAPE;
  MT_LAUNCH(orient_apply_kernel, F, faces, F, face_patch, (int)C, flip0, sign, out_faces, flip);
  return CNR_OK;
}
