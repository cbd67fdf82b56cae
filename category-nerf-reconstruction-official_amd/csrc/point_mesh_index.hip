// Point-to-mesh distance through a tile-box index (metrics.MeshIndex): cnr_point_mesh_dist's result, bit for bit, from far
// fewer pairs.  DESIGN.md §3.20 "The tile-box index" has the contract and the safety argument of the skip rule;
// tests/pointmesh_index_cpu.py restates keys, tile table, skip rule and minimum rule in numpy.
//
//   pm_face_keys    30-bit Morton key of every face's box centre, quantised over the mesh's bounding box (read from device memory)
//   pm_index_build  one wave per tile of PMI_TILE faces in key order: the faces' records (point_mesh_common.h, the face's
//                   ORIGINAL index in the sixteenth float) and the tile's row: box lo / hi (exact min / max of the original
//                   corners), Lmax (sqrtf of the largest fp32 squared edge) and the tile's first key
//   pm_query_keys   the same quantisation for queries, clamped to the box
//   pm_indexed      one workgroup of PMI_WAVES waves per group of PMI_GROUP queries in key order: a seed tile found from the
//                   middle query's key, then every other tile tested 64 at a time (one tile per lane, __ballot) against the
//                   group's largest current minimum and only the survivors evaluated, their faces shared among the waves;
//                   the root, the closest point and the scatter to the queries' original positions in the same launch.
// Deterministic: no atomics; min / max reductions are exact; the minimum rule `d < m || (d == m && orig < mf)` does not depend
// on the order in which tiles are visited.
#include "cnr_common.h"
#include "geom_common.h"
#include "point_mesh_common.h"

#include <math.h>

#pragma clang fp contract(off)

using namespace cnr;

namespace {
constexpr int PMI_TILE = 64;                              // faces per tile: one record per lane when staged (4 KB of LDS)
constexpr int PMI_GROUP = 64;                             // queries per group: one query per lane
constexpr int PMI_WAVES = 8;                              // waves per group, sharing each tile's faces
constexpr int PMI_ROW_F4 = 2;                             // float4 per tile row: (lo, Lmax) (hi, first key)
constexpr float PMI_MARGIN = 32.0f * 5.9604644775390625e-08f;   // C 2^-24, C = 32 (pointmesh_index_cpu.C_MARGIN)

inline int64_t pmi_tiles(int64_t F) { return (F + PMI_TILE - 1) / PMI_TILE; }
inline int64_t pmi_groups(int64_t nq) { return (nq + PMI_GROUP - 1) / PMI_GROUP; }

// the cell of x on the 1024-cell axis [lo, hi]; a zero (or negative) extent, and one that overflows fp32, give cell 0 (so the
// quotient below is a finite number in [0, 1]).  Four roundings: hi - lo, x - lo, the correctly rounded division, the product
// with 1024 (exact).
__device__ __forceinline__ int pmi_cell(float x, float lo, float hi) {
  const float ext = hi - lo;
  if (!(ext > 0.0f && ext < INFINITY)) return 0;
  const float xc = fminf(fmaxf(x, lo), hi);
  const float t = (xc - lo) / ext;
  const int c = (int)(t * 1024.0f);
  return c > 1023 ? 1023 : c;
}
__device__ __forceinline__ int pmi_spread(int v) {        // 10 bits -> every third bit
  v = (v | (v << 16)) & 0x030000FF;
  v = (v | (v << 8)) & 0x0300F00F;
  v = (v | (v << 4)) & 0x030C30C3;
  v = (v | (v << 2)) & 0x09249249;
  return v;
}
__device__ __forceinline__ int pmi_key(float x, float y, float z, const float* __restrict__ bbox) {
  return pmi_spread(pmi_cell(x, bbox[0], bbox[3])) | (pmi_spread(pmi_cell(y, bbox[1], bbox[4])) << 1) |
         (pmi_spread(pmi_cell(z, bbox[2], bbox[5])) << 2);
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fminf(v, __shfl_xor(v, d));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d));
  return v;
}

__global__ __launch_bounds__(256) void pm_face_keys_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                           int64_t F, const float* __restrict__ bbox, int* __restrict__ keys) {
  for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < F; f += (int64_t)gridDim.x * 256) {
    float c[3][3];
    pm_corners(verts, faces, f, c);
    float ctr[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float lo = fminf(fminf(c[0][k], c[1][k]), c[2][k]), hi = fmaxf(fmaxf(c[0][k], c[1][k]), c[2][k]);
      ctr[k] = 0.5f * (lo + hi);
    }
    keys[f] = pmi_key(ctr[0], ctr[1], ctr[2], bbox);
  }
}

__global__ __launch_bounds__(256) void pm_query_keys_kernel(const float* __restrict__ q, int64_t nq, const float* __restrict__ bbox,
                                                            int* __restrict__ keys) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nq; i += (int64_t)gridDim.x * 256)
    keys[i] = pmi_key(q[3 * i], q[3 * i + 1], q[3 * i + 2], bbox);
}

// one wave per tile; lanes past the mesh's end repeat its last face and store no record
__global__ __launch_bounds__(PMI_TILE) void pm_index_build_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                                  int64_t F, const int* __restrict__ keys,
                                                                  const int64_t* __restrict__ order, float4* __restrict__ rec,
                                                                  float4* __restrict__ rows) {
  const int64_t t = blockIdx.x;
  const int64_t base = t * PMI_TILE;
  const int64_t p = base + threadIdx.x;
  const int64_t orig = order[p < F ? p : F - 1];
  float c[3][3];
  pm_corners(verts, faces, orig, c);
  if (p < F) pm_make_record(c, __int_as_float((int)orig), rec + p * PM_REC_F4);
  float lo[3], hi[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] = wave_min(fminf(fminf(c[0][k], c[1][k]), c[2][k]));
    hi[k] = wave_max(fmaxf(fmaxf(c[0][k], c[1][k]), c[2][k]));
  }
  const float abx = c[1][0] - c[0][0], aby = c[1][1] - c[0][1], abz = c[1][2] - c[0][2];
  const float acx = c[2][0] - c[0][0], acy = c[2][1] - c[0][1], acz = c[2][2] - c[0][2];
  const float bcx = c[2][0] - c[1][0], bcy = c[2][1] - c[1][1], bcz = c[2][2] - c[1][2];
  const float e2 = fmaxf(fmaxf(pm_dot(abx, aby, abz, abx, aby, abz), pm_dot(acx, acy, acz, acx, acy, acz)),
                         pm_dot(bcx, bcy, bcz, bcx, bcy, bcz));
  const float lmax = sqrtf(wave_max(e2));                 // correctly rounded and monotone: not below sqrtf of any edge's e2
  if (threadIdx.x == 0) {
    rows[PMI_ROW_F4 * t] = make_float4(lo[0], lo[1], lo[2], lmax);
    rows[PMI_ROW_F4 * t + 1] = make_float4(hi[0], hi[1], hi[2], __int_as_float(keys[order[base]]));
  }
}

// One workgroup of PMI_WAVES waves per group.  Every wave holds the group's 64 queries, one per lane, and makes the same
// decisions; a tile's faces are dealt out to the waves (wave w takes faces w, w + PMI_WAVES, ...) and the waves' minima are
// merged through LDS by the minimum rule after every tile, so all waves go on with the same m, mf, mp: the lane's current
// minimum squared distance, the original index of its face, and that face's position in key order.  The rule is a
// lexicographic minimum over (distance, original index): dealing the faces out changes nothing.
__global__ __launch_bounds__(PMI_GROUP * PMI_WAVES) void pm_indexed_kernel(
    const float* __restrict__ q, int64_t nq, const int* __restrict__ qkeys, const int64_t* __restrict__ qorder,
    const float4* __restrict__ rec, const float4* __restrict__ rows, int64_t F, int64_t T, float* __restrict__ dist_out,
    int* __restrict__ face_out, float* __restrict__ closest_out, int* __restrict__ visited_out) {
  __shared__ float4 s_rec[PMI_TILE * PM_REC_F4];
  __shared__ float s_m[PMI_WAVES][PMI_GROUP];
  __shared__ int s_f[PMI_WAVES][PMI_GROUP], s_p[PMI_WAVES][PMI_GROUP];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t g0 = (int64_t)blockIdx.x * PMI_GROUP;
  const int64_t slot = g0 + lane;
  const int64_t qi = qorder[slot < nq ? slot : nq - 1];   // lanes past the end compute on a copy and store nothing
  const float qx = q[3 * qi], qy = q[3 * qi + 1], qz = q[3 * qi + 2];
  const float glx = wave_min(qx), gly = wave_min(qy), glz = wave_min(qz);
  const float ghx = wave_max(qx), ghy = wave_max(qy), ghz = wave_max(qz);
  float m = INFINITY;
  int mf = 0x7fffffff;
  int mp = 0;                                             // F < 2^31
  int visited = 0;

  // (two barriers per tile: the records are read between them, the waves' minima after the second; the next tile's records are
  // written after every wave's compute, its minima after the next first barrier)
  auto evaluate = [&](int64_t t) {
    const int64_t base = t * PMI_TILE;
    const int cnt = F - base < PMI_TILE ? (int)(F - base) : PMI_TILE;
    if (threadIdx.x < (unsigned)cnt) {
      const float4* gsrc = rec + (base + lane) * PM_REC_F4;
      s_rec[4 * lane] = gsrc[0];
      s_rec[4 * lane + 1] = gsrc[1];
      s_rec[4 * lane + 2] = gsrc[2];
      s_rec[4 * lane + 3] = gsrc[3];
    }
    __syncthreads();
    for (int j = wave; j < cnt; j += PMI_WAVES) {
      const float4 r3 = s_rec[4 * j + 3];
      const PmRec f = pm_unpack(s_rec[4 * j], s_rec[4 * j + 1], s_rec[4 * j + 2], r3);
      const int orig = __float_as_int(r3.w);
      float rx, ry, rz;
      const float d = pm_pair(qx, qy, qz, f, &rx, &ry, &rz);
      if (d < m || (d == m && orig < mf)) {
        m = d;
        mf = orig;
        mp = (int)(base + j);
      }
    }
    s_m[wave][lane] = m;
    s_f[wave][lane] = mf;
    s_p[wave][lane] = mp;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < PMI_WAVES; ++w) {
      const float d = s_m[w][lane];
      const int orig = s_f[w][lane];
      if (d < m || (d == m && orig < mf)) {
        m = d;
        mf = orig;
        mp = s_p[w][lane];
      }
    }
    ++visited;
  };

  // the seed: the last tile whose first key is not above the key of the group's middle query
  const int64_t mid = g0 + PMI_GROUP / 2 < nq ? g0 + PMI_GROUP / 2 : nq - 1;
  const int key = qkeys[qorder[mid]];
  int64_t lo = 0, hi = T;                                  // first key of tile lo <= key (or lo == 0) < first key of tile hi
  while (hi - lo > 1) {
    const int64_t c = (lo + hi) >> 1;
    if (__float_as_int(rows[PMI_ROW_F4 * c + 1].w) <= key) lo = c; else hi = c;
  }
  const int64_t seed = lo;
  evaluate(seed);

  // every other tile, 64 at a time from the seed's block outwards: sb, sb + 1, sb - 1, sb + 2, ...
  const int64_t nb = (T + 63) / 64, sb = seed / 64;
  const int64_t reach = sb > nb - 1 - sb ? sb : nb - 1 - sb;
  for (int64_t step = 0; step <= 2 * reach; ++step) {
    const int64_t off = (step + 1) >> 1;
    const int64_t b = (step & 1) ? sb + off : sb - off;
    if (b < 0 || b >= nb) continue;
    const int64_t t = b * 64 + lane;
    const bool valid = t < T && t != seed;
    const int64_t tr = t < T ? t : T - 1;
    const float4 r0 = rows[PMI_ROW_F4 * tr], r1 = rows[PMI_ROW_F4 * tr + 1];
    // lb: the box-to-box distance, the per-axis gap first; thr = lb - C 2^-24 (lb + Lmax)
    const float gx = fmaxf(fmaxf(r0.x - ghx, glx - r1.x), 0.0f);
    const float gy = fmaxf(fmaxf(r0.y - ghy, gly - r1.y), 0.0f);
    const float gz = fmaxf(fmaxf(r0.z - ghz, glz - r1.z), 0.0f);
    const float lb = sqrtf(pm_dot(gx, gy, gz, gx, gy, gz));
    const float thr = lb - PMI_MARGIN * (lb + r0.w);
    // (the reduction on its own line: inside `valid && ...` the lanes without a tile would not take part in its shuffles)
    float root_m = sqrtf(wave_max(m));
    unsigned long long todo = __ballot(valid && !(thr > root_m));
    while (todo) {
      const int j = __ffsll((long long)todo) - 1;
      evaluate(b * 64 + j);
      root_m = sqrtf(wave_max(m));                         // M has fallen: test what is left again
      todo &= todo - 1;
      todo &= __ballot(valid && !(thr > root_m));
    }
  }

  if (threadIdx.x == 0 && visited_out) visited_out[blockIdx.x] = visited;
  if (wave == 0 && slot < nq) {
    dist_out[qi] = sqrtf(m);                              // correctly rounded (hipcc's default for sqrtf)
    face_out[qi] = mf;
    if (closest_out) {
      const float4* gsrc = rec + (int64_t)mp * PM_REC_F4;
      const PmRec r = pm_unpack(gsrc[0], gsrc[1], gsrc[2], gsrc[3]);
      float rx, ry, rz;
      pm_pair(qx, qy, qz, r, &rx, &ry, &rz);
      closest_out[3 * qi] = qx + rx;
      closest_out[3 * qi + 1] = qy + ry;
      closest_out[3 * qi + 2] = qz + rz;
    }
  }
}
}  // namespace

extern "C" int cnr_pm_index_params(int* tile_faces, int* group_queries) {
  if (!tile_faces || !group_queries) return CNR_E_ARG;
  *tile_faces = PMI_TILE;
  *group_queries = PMI_GROUP;
  return CNR_OK;
}

extern "C" int64_t cnr_pm_index_bytes(int64_t F) {
  if (F < 1 || F > 0x7fffffff) return CNR_E_SHAPE;
  return align256(F * PM_REC_BYTES) + align256(pmi_tiles(F) * PMI_ROW_F4 * 16);
}

extern "C" int64_t cnr_point_mesh_indexed_workspace_bytes(int64_t nq, int64_t F) {
  if (nq < 1 || F < 1 || F > 0x7fffffff) return CNR_E_SHAPE;
  return align256(pmi_groups(nq) * 4);
}

extern "C" int cnr_pm_index_keys(const float* verts, const int* faces, int64_t F, const float* bbox, int* keys_out, void* stream) {
  if (!verts || !bbox || !keys_out) return CNR_E_ARG;
  if (F < 1 || F > 0x7fffffff) return CNR_E_SHAPE;
  hipLaunchKernelGGL(pm_face_keys_kernel, dim3(grid_of(F, 256, 4096)), dim3(256), 0, (hipStream_t)stream, verts, faces, F, bbox,
                     keys_out);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_pm_query_keys(const float* q, int64_t nq, const float* bbox, int* keys_out, void* stream) {
  if (!q || !bbox || !keys_out) return CNR_E_ARG;
  if (nq < 1) return CNR_E_SHAPE;
  hipLaunchKernelGGL(pm_query_keys_kernel, dim3(grid_of(nq, 256, 4096)), dim3(256), 0, (hipStream_t)stream, q, nq, bbox, keys_out);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_pm_index_build(const float* verts, const int* faces, int64_t F, const int* keys, const int64_t* order,
                                  void* index_out, void* stream) {
  if (!verts || !keys || !order || !index_out) return CNR_E_ARG;
  if (F < 1 || F > 0x7fffffff) return CNR_E_SHAPE;
  float4* rec = (float4*)index_out;
  float4* rows = (float4*)((char*)index_out + align256(F * PM_REC_BYTES));
  hipLaunchKernelGGL(pm_index_build_kernel, dim3((unsigned)pmi_tiles(F)), dim3(PMI_TILE), 0, (hipStream_t)stream, verts, faces, F,
                     keys, order, rec, rows);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_point_mesh_dist_indexed(const float* q, int64_t nq, const int* qkeys, const int64_t* qorder, const void* index,
                                           int64_t F, float* dist_out, int* face_out, float* closest_out, void* workspace,
                                           void* stream) {
  if (!q || !qkeys || !qorder || !index || !dist_out || !face_out || !workspace) return CNR_E_ARG;
  if (nq < 1 || F < 1 || F > 0x7fffffff) return CNR_E_SHAPE;
  const int64_t groups = pmi_groups(nq);
  if (groups > 0x7fffffff) return CNR_E_SHAPE;
  const float4* rec = (const float4*)index;
  const float4* rows = (const float4*)((const char*)index + align256(F * PM_REC_BYTES));
  hipLaunchKernelGGL(pm_indexed_kernel, dim3((unsigned)groups), dim3(PMI_GROUP * PMI_WAVES), 0, (hipStream_t)stream, q, nq, qkeys,
                     qorder, rec, rows, F, pmi_tiles(F), dist_out, face_out, closest_out, (int*)workspace);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}
