// Point-to-mesh distance (metrics.point_mesh_distance, calc_3d_metric_surface, meshops.deviation): the exact closest point of a
// triangle mesh to every query, brute force.  DESIGN.md §3.20 has the contract; tests/pointmesh_cpu.py restates it in numpy.
//
// Every launch is deterministic: no atomics, faces visited in index order with a strict `<`, chunks merged in chunk order.
//   pm_record    one record per face: corner a, edges ab = b - a and ac = c - a, ab.ab, ab.ac, ac.ac, and the unit normal (fp64
//                cross product of the fp32 edges, normalised in fp64, rounded once).  Only the corner is in absolute coordinates.  A face whose edge vectors are exactly parallel (or zero) stands for its longest edge:
//                its record is that segment as a triangle with ac = 0, which the per-pair code below resolves as vertex / edge.
//   pm_partial   a 2-D grid of (query block, face chunk); the chunk's records go through LDS a tile at a time (every lane reads
//                the same record: a broadcast), each lane keeps PM_QPT queries in registers with their running minimum squared
//                distance and its face.
//   pm_finish    the minimum over chunks in chunk order (strict `<`: the lowest face index wins), the correctly rounded sqrt,
//                and, when asked for, the closest point q + r of the winning face recomputed once.
// Arithmetic: fp32, one IEEE rounding per operation (contraction off), difference first: ap = q - a, then dot products of
// differences; nothing is evaluated in absolute coordinates, so a translation that keeps the differences exact changes no bit.
#include "cnr_common.h"
#include "geom_common.h"
#include "point_mesh_common.h"

#include <math.h>

#pragma clang fp contract(off)

using namespace cnr;

namespace {
constexpr int PM_BLOCK = 256;
constexpr int PM_QPT = 4;                                 // queries per lane
constexpr int PM_QBLK = PM_BLOCK * PM_QPT;                // queries per workgroup
constexpr int PM_TILE = 256;                              // face records per LDS tile (16 KB)
constexpr int64_t PM_TARGET_WG = 2048;

struct PmLayout {
  int64_t qblocks, chunks, chunk_len, rec_bytes, part_stride, bytes;
};
// bytes = align256(64 F) + chunks * align256(8 nq): the records, then per chunk nq minima (f32) followed by nq faces (i32)
inline PmLayout pm_layout(int64_t nq, int64_t F) {
  PmLayout L;
  L.qblocks = (nq + PM_QBLK - 1) / PM_QBLK;
  const int64_t tiles = (F + PM_TILE - 1) / PM_TILE;
  int64_t want = (PM_TARGET_WG + L.qblocks - 1) / L.qblocks;
  if (want > tiles) want = tiles;
  if (want < 1) want = 1;
  const int64_t tiles_per_chunk = (tiles + want - 1) / want;
  L.chunk_len = tiles_per_chunk * PM_TILE;
  L.chunks = (F + L.chunk_len - 1) / L.chunk_len;
  L.rec_bytes = align256(F * PM_REC_BYTES);
  L.part_stride = align256(nq * 8);
  L.bytes = L.rec_bytes + L.chunks * L.part_stride;
  return L;
}

__global__ __launch_bounds__(256) void pm_record_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int64_t F,
                                                        float4* __restrict__ rec) {
  for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < F; f += (int64_t)gridDim.x * 256) {
    float c[3][3];
    pm_corners(verts, faces, f, c);
    pm_make_record(c, 0.0f, rec + 4 * f);
  }
}

__global__ __launch_bounds__(PM_BLOCK) void pm_partial_kernel(const float* __restrict__ q, int64_t nq,
                                                              const float4* __restrict__ rec, int64_t F, int64_t chunk_len,
                                                              char* __restrict__ part, int64_t part_stride) {
  __shared__ float4 s_rec[PM_TILE * PM_REC_F4];
  const int t = threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.x * PM_QBLK;
  const int64_t c = blockIdx.y;
  const int64_t p0 = c * chunk_len;
  const int64_t p1 = p0 + chunk_len < F ? p0 + chunk_len : F;
  float qx[PM_QPT], qy[PM_QPT], qz[PM_QPT], m[PM_QPT];
  int mf[PM_QPT];
#pragma unroll
  for (int k = 0; k < PM_QPT; ++k) {
    int64_t i = q0 + k * PM_BLOCK + t;
    i = i < nq ? i : nq - 1;                              // lanes past the end compute on a copy and store nothing
    qx[k] = q[3 * i];
    qy[k] = q[3 * i + 1];
    qz[k] = q[3 * i + 2];
    m[k] = INFINITY;
    mf[k] = (int)p0;
  }
  for (int64_t base = p0; base < p1; base += PM_TILE) {
    const int cnt = p1 - base < PM_TILE ? (int)(p1 - base) : PM_TILE;
    __syncthreads();
    if (t < cnt) {
      const float4* g = rec + (base + t) * PM_REC_F4;
      s_rec[4 * t] = g[0];
      s_rec[4 * t + 1] = g[1];
      s_rec[4 * t + 2] = g[2];
      s_rec[4 * t + 3] = g[3];
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const PmRec f = pm_unpack(s_rec[4 * j], s_rec[4 * j + 1], s_rec[4 * j + 2], s_rec[4 * j + 3]);
      const int fi = (int)(base + j);
#pragma unroll
      for (int k = 0; k < PM_QPT; ++k) {
        float rx, ry, rz;
        const float d = pm_pair(qx[k], qy[k], qz[k], f, &rx, &ry, &rz);
        if (d < m[k]) {
          m[k] = d;
          mf[k] = fi;
        }
      }
    }
  }
  float* od = (float*)(part + c * part_stride);
  int* of = (int*)(od + nq);
#pragma unroll
  for (int k = 0; k < PM_QPT; ++k) {
    const int64_t i = q0 + k * PM_BLOCK + t;
    if (i < nq) {
      od[i] = m[k];
      of[i] = mf[k];
    }
  }
}

__global__ __launch_bounds__(256) void pm_finish_kernel(const float* __restrict__ q, int64_t nq, const float4* __restrict__ rec,
                                                        const char* __restrict__ part, int64_t part_stride, int64_t chunks,
                                                        float* __restrict__ dist_out, int* __restrict__ face_out,
                                                        float* __restrict__ closest_out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nq; i += (int64_t)gridDim.x * 256) {
    const float* d0 = (const float*)part;
    float m = d0[i];
    int f = ((const int*)(d0 + nq))[i];
    for (int64_t c = 1; c < chunks; ++c) {
      const float* dc = (const float*)(part + c * part_stride);
      const float d = dc[i];
      if (d < m) {
        m = d;
        f = ((const int*)(dc + nq))[i];
      }
    }
    dist_out[i] = sqrtf(m);                               // correctly rounded (hipcc's default for sqrtf; __fsqrt_rn is the bare v_sqrt_f32)
    face_out[i] = f;
    if (closest_out) {
      const float4* g = rec + (int64_t)f * PM_REC_F4;
      const PmRec r = pm_unpack(g[0], g[1], g[2], g[3]);
      const float qx = q[3 * i], qy = q[3 * i + 1], qz = q[3 * i + 2];
      float rx, ry, rz;
      pm_pair(qx, qy, qz, r, &rx, &ry, &rz);
      closest_out[3 * i] = qx + rx;
      closest_out[3 * i + 1] = qy + ry;
      closest_out[3 * i + 2] = qz + rz;
    }
  }
}
}  // namespace

extern "C" int64_t cnr_point_mesh_workspace_bytes(int64_t nq, int64_t F) {
  if (nq < 1 || F < 1 || F > 0x7fffffff) return CNR_E_SHAPE;
  return pm_layout(nq, F).bytes;
}

// stage: 0 = all three passes; 1, 2, 3 = the record, partial or finish pass alone (tools/time_pointmesh.py times them apart)
static int pm_run(const float* q, int64_t nq, const float* verts, const int* faces, int64_t F, float* dist_out, int* face_out,
                  float* closest_out, void* workspace, void* stream, int stage) {
  if (!q || !verts || !dist_out || !face_out || !workspace) return CNR_E_ARG;
  if (nq < 1 || F < 1 || F > 0x7fffffff) return CNR_E_SHAPE;
  const PmLayout L = pm_layout(nq, F);
  if (L.qblocks > 0x7fffffff || L.chunks > 65535) return CNR_E_SHAPE;
  char* ws = (char*)workspace;
  float4* rec = (float4*)ws;
  char* part = ws + L.rec_bytes;
  if (stage == 0 || stage == 1) {
    hipLaunchKernelGGL(pm_record_kernel, dim3(grid_of(F, 256, 4096)), dim3(256), 0, (hipStream_t)stream, verts, faces, F, rec);
    CNR_LAUNCH_CHECK();
  }
  if (stage == 0 || stage == 2) {
    hipLaunchKernelGGL(pm_partial_kernel, dim3((unsigned)L.qblocks, (unsigned)L.chunks), dim3(PM_BLOCK), 0, (hipStream_t)stream, q,
                       nq, (const float4*)rec, F, L.chunk_len, part, L.part_stride);
    CNR_LAUNCH_CHECK();
  }
  if (stage == 0 || stage == 3) {
    hipLaunchKernelGGL(pm_finish_kernel, dim3(grid_of(nq, 256, 4096)), dim3(256), 0, (hipStream_t)stream, q, nq,
                       (const float4*)rec, (const char*)part, L.part_stride, L.chunks, dist_out, face_out, closest_out);
    CNR_LAUNCH_CHECK();
  }
  return CNR_OK;
}

extern "C" int cnr_point_mesh_dist(const float* q, int64_t nq, const float* verts, const int* faces, int64_t F, float* dist_out,
                                   int* face_out, float* closest_out, void* workspace, void* stream) {
  return pm_run(q, nq, verts, faces, F, dist_out, face_out, closest_out, workspace, stream, 0);
}

extern "C" int cnr_point_mesh_pass(const float* q, int64_t nq, const float* verts, const int* faces, int64_t F, float* dist_out,
                                   int* face_out, float* closest_out, void* workspace, int pass, void* stream) {
  if (pass < 1 || pass > 3) return CNR_E_ARG;
  return pm_run(q, nq, verts, faces, F, dist_out, face_out, closest_out, workspace, stream, pass);
}
