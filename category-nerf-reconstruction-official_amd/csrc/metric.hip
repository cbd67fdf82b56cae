// Mesh evaluation (metric/eval_3D_obj.py, metric/metrics.py): exact nearest-neighbour distances, their mean / threshold count,
// area-weighted surface sampling and clipping to an oriented box.  DESIGN.md §3.7 has the contract.
//
// Every launch is deterministic: no atomics, fixed reduction orders, and reduce-then-scan for every variable-size output, so
// two runs on the same inputs are bit-identical.
//   cnr_nn_dist          nn_partial: a 2-D grid of (query block, reference chunk); the chunk's points go through LDS a tile at
//                        a time (every lane reads the same point: a broadcast), each lane keeps NN_QPT queries in registers and
//                        their running minimum squared distance, (q - p)^2 summed directly (no |q|^2 + |p|^2 - 2 q.p: at scene
//                        coordinates of metres that form cancels the centimetres the metric measures).  nn_finish: the min
//                        over chunks in chunk order, then the correctly rounded sqrt.
//   cnr_dist_stats       DS_BLOCKS workgroups sum a fixed contiguous slice each in fp64 (tree in LDS), one workgroup the rest.
//   cnr_face_area_scan   per-face area (fp64 cross product of the fp32 corners), its inclusive prefix: block sums, one-workgroup
//                        scan of them, block scans.
//   cnr_sample_surface   per sample: searchsorted-left on the prefix, the reflected barycentric point (fp64, rounded once).
//   cnr_sample_faces     the face index of that search alone, through the same device function.
//   cnr_clip_box_*       Sutherland-Hodgman against 6 planes in registers (fp64), fan triangulation; classify, scan, emit as
//                        csrc/mcubes.hip does, so the output is in (face, fan) order.
#include "cnr_common.h"
#include "geom_common.h"

#include <math.h>

using namespace cnr;

namespace {
// ---- nearest-neighbour distance ----------------------------------------------------------------------------------------
struct NnLayout {
  int64_t qblocks, chunks, chunk_len, bytes;
};
inline NnLayout nn_layout(int64_t nq, int64_t nr) {
  NnLayout L;
  L.qblocks = (nq + NN_QBLK - 1) / NN_QBLK;
  nn_chunks(L.qblocks, nr, &L.chunk_len, &L.chunks);
  L.bytes = align256(L.chunks * nq * 4);
  return L;
}

__global__ __launch_bounds__(NN_BLOCK) void nn_partial_kernel(const float* __restrict__ q, int64_t nq,
                                                              const float* __restrict__ p, int64_t nr, int64_t chunk_len,
                                                              float* __restrict__ part) {
  __shared__ float4 s_p[NN_TILE];
  const int t = threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.x * NN_QBLK;
  float qx[NN_QPT], qy[NN_QPT], qz[NN_QPT], m[NN_QPT];
#pragma unroll
  for (int k = 0; k < NN_QPT; ++k) {
    int64_t i = q0 + k * NN_BLOCK + t;
    i = i < nq ? i : nq - 1;                              // lanes past the end compute on a copy and store nothing
    qx[k] = q[3 * i];
    qy[k] = q[3 * i + 1];
    qz[k] = q[3 * i + 2];
    m[k] = INFINITY;
  }
  const int64_t c = blockIdx.y;
  const int64_t p0 = c * chunk_len;
  const int64_t p1 = p0 + chunk_len < nr ? p0 + chunk_len : nr;
  for (int64_t base = p0; base < p1; base += NN_TILE) {
    __syncthreads();
    {
      const int64_t j = base + t;
      // past the chunk: a point at infinity, whose squared distance (inf) never wins the min
      s_p[t] = j < p1 ? make_float4(p[3 * j], p[3 * j + 1], p[3 * j + 2], 0.0f) : make_float4(INFINITY, INFINITY, INFINITY, 0.0f);
    }
    __syncthreads();
    // four points per step: two v_min3_f32 per query (min3 of three distances, then min3 with the running minimum and the fourth)
#pragma unroll 2
    for (int j = 0; j < NN_TILE; j += 4) {
      const float4 r0 = s_p[j], r1 = s_p[j + 1], r2 = s_p[j + 2], r3 = s_p[j + 3];
#pragma unroll
      for (int k = 0; k < NN_QPT; ++k) {
        const float m3 =
            fminf(fminf(sq_dist(qx[k], qy[k], qz[k], r0), sq_dist(qx[k], qy[k], qz[k], r1)), sq_dist(qx[k], qy[k], qz[k], r2));
        m[k] = fminf(fminf(m[k], m3), sq_dist(qx[k], qy[k], qz[k], r3));
      }
    }
  }
  float* o = part + c * nq;
#pragma unroll
  for (int k = 0; k < NN_QPT; ++k) {
    const int64_t i = q0 + k * NN_BLOCK + t;
    if (i < nq) o[i] = m[k];
  }
}

__global__ __launch_bounds__(256) void nn_finish_kernel(const float* __restrict__ part, int64_t nq, int64_t chunks,
                                                        float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nq; i += (int64_t)gridDim.x * 256) {
    float m = part[i];
    for (int64_t c = 1; c < chunks; ++c) m = fminf(m, part[c * nq + i]);
    out[i] = __fsqrt_rn(m);
  }
}

// ---- distance statistics -----------------------------------------------------------------------------------------------
constexpr int DS_BLOCKS = 256;
constexpr int DS_THREADS = 256;

// fixed-order tree over the block's 256 values (sum and count); thread 0 ends with the totals
__device__ __forceinline__ void block_tree(double* s_sum, int64_t* s_cnt) {
  const int t = threadIdx.x;
  __syncthreads();
  for (int d = DS_THREADS / 2; d > 0; d >>= 1) {
    if (t < d) {
      s_sum[t] += s_sum[t + d];
      s_cnt[t] += s_cnt[t + d];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(DS_THREADS) void ds_partial_kernel(const float* __restrict__ d, int64_t n, float th,
                                                                double* __restrict__ psum, int64_t* __restrict__ pcnt) {
  __shared__ double s_sum[DS_THREADS];
  __shared__ int64_t s_cnt[DS_THREADS];
  const int t = threadIdx.x;
  const int64_t per = (n + DS_BLOCKS - 1) / DS_BLOCKS;
  const int64_t b0 = (int64_t)blockIdx.x * per, b1 = b0 + per < n ? b0 + per : n;
  double s = 0.0;
  int64_t c = 0;
  for (int64_t i = b0 + t; i < b1; i += DS_THREADS) {
    const float v = d[i];
    s += (double)v;
    c += v < th ? 1 : 0;
  }
  s_sum[t] = s;
  s_cnt[t] = c;
  block_tree(s_sum, s_cnt);
  if (t == 0) {
    psum[blockIdx.x] = s_sum[0];
    pcnt[blockIdx.x] = s_cnt[0];
  }
}

__global__ __launch_bounds__(DS_THREADS) void ds_final_kernel(const double* __restrict__ psum, const int64_t* __restrict__ pcnt,
                                                              double* __restrict__ sum_out, int64_t* __restrict__ count_out) {
  __shared__ double s_sum[DS_THREADS];
  __shared__ int64_t s_cnt[DS_THREADS];
  const int t = threadIdx.x;
  s_sum[t] = psum[t];
  s_cnt[t] = pcnt[t];
  block_tree(s_sum, s_cnt);
  if (t == 0) {
    *sum_out = s_sum[0];
    *count_out = s_cnt[0];
  }
}
static_assert(DS_BLOCKS == DS_THREADS, "ds_final_kernel reads one partial per thread");

// ---- triangles: indexed (faces != NULL) or a soup (faces == NULL: verts is (F,3,3)) ----------------------------------------
struct D3 {
  double x, y, z;
};
__device__ __forceinline__ D3 corner(const float* __restrict__ verts, const int* __restrict__ faces, int64_t f, int k) {
  const int64_t v = faces ? (int64_t)faces[3 * f + k] : 3 * f + k;
  return D3{(double)verts[3 * v], (double)verts[3 * v + 1], (double)verts[3 * v + 2]};
}
__device__ __forceinline__ D3 sub(D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }

__device__ __forceinline__ double tri_area(D3 a, D3 b, D3 c) {
  const D3 u = sub(b, a), v = sub(c, a);
  const double cx = u.y * v.z - u.z * v.y, cy = u.z * v.x - u.x * v.z, cz = u.x * v.y - u.y * v.x;
  return 0.5 * sqrt(cx * cx + cy * cy + cz * cz);
}

// ---- face areas and their inclusive prefix -----------------------------------------------------------------------------
constexpr int FA_BLOCK = 256;
constexpr int FA_ITEMS = 4;
constexpr int FA_PER_BLOCK = FA_BLOCK * FA_ITEMS;

struct FaLayout {
  int64_t nblk, off_ofs, bytes;
};
inline FaLayout fa_layout(int64_t F) {
  FaLayout L;
  L.nblk = (F + FA_PER_BLOCK - 1) / FA_PER_BLOCK;
  L.off_ofs = align256(L.nblk * 8);
  L.bytes = L.off_ofs + align256(L.nblk * 8);
  return L;
}

__global__ __launch_bounds__(FA_BLOCK) void fa_reduce_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                             int64_t F, double* __restrict__ area,
                                                             double* __restrict__ blk_sum) {
  __shared__ double s[FA_BLOCK];
  const int64_t f0 = (int64_t)blockIdx.x * FA_PER_BLOCK + threadIdx.x * FA_ITEMS;
  double run = 0.0;
#pragma unroll
  for (int k = 0; k < FA_ITEMS; ++k) {
    const int64_t f = f0 + k;
    if (f < F) {
      const double a = tri_area(corner(verts, faces, f, 0), corner(verts, faces, f, 1), corner(verts, faces, f, 2));
      area[f] = a;
      run += a;
    }
  }
  const double incl = block_scan<FA_BLOCK>(run, s);
  if (threadIdx.x == FA_BLOCK - 1) blk_sum[blockIdx.x] = incl;
}

__global__ __launch_bounds__(FA_BLOCK) void fa_scan_kernel(const double* __restrict__ area, int64_t F,
                                                           const double* __restrict__ ofs, double* __restrict__ cum) {
  __shared__ double s[FA_BLOCK];
  const int64_t f0 = (int64_t)blockIdx.x * FA_PER_BLOCK + threadIdx.x * FA_ITEMS;
  double a[FA_ITEMS], run = 0.0;
#pragma unroll
  for (int k = 0; k < FA_ITEMS; ++k) {
    a[k] = f0 + k < F ? area[f0 + k] : 0.0;
    run += a[k];
  }
  block_scan<FA_BLOCK>(run, s);
  double base = threadIdx.x > 0 ? s[threadIdx.x - 1] : 0.0;
  const double o = ofs[blockIdx.x];
#pragma unroll
  for (int k = 0; k < FA_ITEMS; ++k) {
    base += a[k];
    if (f0 + k < F) cum[f0 + k] = o + base;
  }
}

// ---- surface sampling --------------------------------------------------------------------------------------------------
// searchsorted(cum, u0 * total, side='left'): the first f with cum[f] >= u0 * total (the last face when there is none)
__device__ __forceinline__ int64_t sample_face(const double* __restrict__ cum, int64_t F, double total, double u0) {
  const double target = u0 * total;
  int64_t lo = 0, hi = F;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (cum[mid] < target) lo = mid + 1;
    else hi = mid;
  }
  return lo < F ? lo : F - 1;
}

// the face index alone (cnr_sample_faces): u is the same (n,3) array of draws, of which only u0 is read
__global__ __launch_bounds__(256) void sample_faces_kernel(int64_t F, const double* __restrict__ cum, const double* __restrict__ u,
                                                           int64_t n, int* __restrict__ face_out) {
  const double total = cum[F - 1];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    face_out[i] = (int)sample_face(cum, F, total, u[3 * i]);
}

__global__ __launch_bounds__(256) void sample_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int64_t F,
                                                     const double* __restrict__ cum, const double* __restrict__ u, int64_t n,
                                                     float* __restrict__ out) {
  const double total = cum[F - 1];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t f = sample_face(cum, F, total, u[3 * i]);
    double a = u[3 * i + 1], b = u[3 * i + 2];
    if (a + b > 1.0) {
      a = fabs(a - 1.0);
      b = fabs(b - 1.0);
    }
    const D3 v0 = corner(verts, faces, f, 0), v1 = corner(verts, faces, f, 1), v2 = corner(verts, faces, f, 2);
    const D3 e1 = sub(v1, v0), e2 = sub(v2, v0);
    out[3 * i] = (float)(e1.x * a + e2.x * b + v0.x);
    out[3 * i + 1] = (float)(e1.y * a + e2.y * b + v0.y);
    out[3 * i + 2] = (float)(e1.z * a + e2.z * b + v0.z);
  }
}

// ---- clipping to a box of 6 planes -------------------------------------------------------------------------------------
constexpr int CL_BLOCK = 256;
constexpr int CL_WAVES = CL_BLOCK / 64;
constexpr int CL_MAXV = 15;                               // polygon vertices kept (a triangle gains at most one per plane: 9)

struct ClLayout {
  int64_t nblk, off_ofs, bytes;
};
inline ClLayout cl_layout(int64_t F) {
  ClLayout L;
  L.nblk = (F + CL_BLOCK - 1) / CL_BLOCK;
  L.off_ofs = align256(L.nblk * 4);
  L.bytes = L.off_ofs + align256(L.nblk * 8);
  return L;
}

// Sutherland-Hodgman: planes (6,6) = origin, inward normal; a point is kept when (x - o) . n >= 0.  The polygon of face f
// ends in P[0 .. n); returns n (0 when nothing is left).  Intersections: a + (b - a) * da / (da - db) from the kept end's side.
__device__ int clip_face(const float* __restrict__ verts, const int* __restrict__ faces, int64_t f,
                         const double* __restrict__ planes, D3* P) {
  D3 Q[CL_MAXV];
  double dist[CL_MAXV];
  int n = 3;
  P[0] = corner(verts, faces, f, 0);
  P[1] = corner(verts, faces, f, 1);
  P[2] = corner(verts, faces, f, 2);
  for (int pl = 0; pl < 6 && n > 0; ++pl) {
    const double* h = planes + 6 * pl;
    bool all_in = true;
    for (int i = 0; i < n; ++i) {
      dist[i] = (P[i].x - h[0]) * h[3] + (P[i].y - h[1]) * h[4] + (P[i].z - h[2]) * h[5];
      all_in = all_in && dist[i] >= 0.0;
    }
    if (all_in) continue;
    int m = 0;
    for (int i = 0; i < n; ++i) {
      const int j = i + 1 < n ? i + 1 : 0;
      const double da = dist[i], db = dist[j];
      if (da >= 0.0 && m < CL_MAXV) Q[m++] = P[i];
      if ((da >= 0.0) != (db >= 0.0) && m < CL_MAXV) {
        const double t = da / (da - db);
        Q[m++] = D3{P[i].x + (P[j].x - P[i].x) * t, P[i].y + (P[j].y - P[i].y) * t, P[i].z + (P[j].z - P[i].z) * t};
      }
    }
    for (int i = 0; i < m; ++i) P[i] = Q[i];
    n = m;
  }
  return n >= 3 ? n : 0;
}

__global__ __launch_bounds__(CL_BLOCK) void clip_count_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                              int64_t F, const double* __restrict__ planes,
                                                              int* __restrict__ blk_counts) {
  __shared__ int s_w[CL_WAVES];
  const int64_t f = (int64_t)blockIdx.x * CL_BLOCK + threadIdx.x;
  int nt = 0;
  if (f < F) {
    D3 P[CL_MAXV];
    const int n = clip_face(verts, faces, f, planes, P);
    nt = n ? n - 2 : 0;
  }
  int wt, total;
  wave_prefix_bits<4>(nt, &wt);
  block_prefix_waves<CL_WAVES>(0, wt, s_w, &total);
  if (threadIdx.x == 0) blk_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(CL_BLOCK) void clip_emit_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                             int64_t F, const double* __restrict__ planes,
                                                             const int64_t* __restrict__ ofs, float* __restrict__ tris) {
  __shared__ int s_w[CL_WAVES];
  const int64_t f = (int64_t)blockIdx.x * CL_BLOCK + threadIdx.x;
  D3 P[CL_MAXV];
  int n = 0;
  if (f < F) n = clip_face(verts, faces, f, planes, P);
  const int nt = n ? n - 2 : 0;
  int wt, total;
  const int pre = block_prefix_waves<CL_WAVES>(wave_prefix_bits<4>(nt, &wt), wt, s_w, &total);
  if (!nt) return;
  float* o = tris + (ofs[blockIdx.x] + pre) * 9;
  for (int k = 0; k < nt; ++k) {
    const D3 c[3] = {P[0], P[k + 1], P[k + 2]};
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      o[9 * k + 3 * v] = (float)c[v].x;
      o[9 * k + 3 * v + 1] = (float)c[v].y;
      o[9 * k + 3 * v + 2] = (float)c[v].z;
    }
  }
}
}  // namespace

extern "C" int64_t cnr_nn_workspace_bytes(int64_t nq, int64_t nr) {
  if (nq < 1 || nr < 1) return CNR_E_SHAPE;
  return nn_layout(nq, nr).bytes;
}

extern "C" int cnr_nn_dist(const float* q, int64_t nq, const float* p, int64_t nr, float* dist_out, void* workspace,
                           void* stream) {
  if (!q || !p || !dist_out || !workspace) return CNR_E_ARG;
  if (nq < 1 || nr < 1) return CNR_E_SHAPE;
  const NnLayout L = nn_layout(nq, nr);
  if (L.qblocks > 0x7fffffff || L.chunks > 65535) return CNR_E_SHAPE;
  hipLaunchKernelGGL(nn_partial_kernel, dim3((unsigned)L.qblocks, (unsigned)L.chunks), dim3(NN_BLOCK), 0, (hipStream_t)stream, q,
                     nq, p, nr, L.chunk_len, (float*)workspace);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(nn_finish_kernel, dim3(grid_of(nq, 256, 4096)), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, nq,
                     L.chunks, dist_out);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int64_t cnr_dist_stats_workspace_bytes(int64_t n) {
  if (n < 1) return CNR_E_SHAPE;
  return align256(DS_BLOCKS * 8) * 2;
}

extern "C" int cnr_dist_stats(const float* dist, int64_t n, float th, void* workspace, double* sum_out, int64_t* count_out,
                              void* stream) {
  if (!dist || !workspace || !sum_out || !count_out) return CNR_E_ARG;
  if (n < 1) return CNR_E_SHAPE;
  char* ws = (char*)workspace;
  double* psum = (double*)ws;
  int64_t* pcnt = (int64_t*)(ws + align256(DS_BLOCKS * 8));
  hipLaunchKernelGGL(ds_partial_kernel, dim3(DS_BLOCKS), dim3(DS_THREADS), 0, (hipStream_t)stream, dist, n, th, psum, pcnt);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(ds_final_kernel, dim3(1), dim3(DS_THREADS), 0, (hipStream_t)stream, (const double*)psum,
                     (const int64_t*)pcnt, sum_out, count_out);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int64_t cnr_face_area_workspace_bytes(int64_t F) {
  if (F < 1) return CNR_E_SHAPE;
  return fa_layout(F).bytes;
}

extern "C" int cnr_face_area_scan(const float* verts, const int* faces, int64_t F, void* workspace, double* area, double* cum,
                                  void* stream) {
  if (!verts || !workspace || !area || !cum) return CNR_E_ARG;
  if (F < 1) return CNR_E_SHAPE;
  const FaLayout L = fa_layout(F);
  if (L.nblk > 0x7fffffff) return CNR_E_SHAPE;
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(fa_reduce_kernel, dim3((unsigned)L.nblk), dim3(FA_BLOCK), 0, (hipStream_t)stream, verts, faces, F, area,
                     (double*)ws);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL((blocks_scan_kernel<1, double, double>), dim3(1), dim3(SCAN_THREADS), 0, (hipStream_t)stream,
                     (const double*)ws, L.nblk, (double*)(ws + L.off_ofs), (double*)nullptr);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(fa_scan_kernel, dim3((unsigned)L.nblk), dim3(FA_BLOCK), 0, (hipStream_t)stream, (const double*)area, F,
                     (const double*)(ws + L.off_ofs), cum);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_sample_surface(const float* verts, const int* faces, int64_t F, const double* cum, const double* u, int64_t n,
                                  float* out, void* stream) {
  if (!verts || !cum || !u || !out) return CNR_E_ARG;
  if (F < 1 || n < 0) return CNR_E_SHAPE;
  if (n == 0) return CNR_OK;
  hipLaunchKernelGGL(sample_kernel, dim3(grid_of(n, 256, 4096)), dim3(256), 0, (hipStream_t)stream, verts, faces, F, cum, u, n, out);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_sample_faces(const double* cum, int64_t F, const double* u, int64_t n, int* face_out, void* stream) {
  if (!cum || !u || !face_out) return CNR_E_ARG;
  if (F < 1 || F > 0x7fffffff || n < 0) return CNR_E_SHAPE;
  if (n == 0) return CNR_OK;
  hipLaunchKernelGGL(sample_faces_kernel, dim3(grid_of(n, 256, 4096)), dim3(256), 0, (hipStream_t)stream, F, cum, u, n, face_out);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int64_t cnr_clip_box_workspace_bytes(int64_t F) {
  if (F < 1) return CNR_E_SHAPE;
  return cl_layout(F).bytes;
}

extern "C" int cnr_clip_box_count(const float* verts, const int* faces, int64_t F, const double* planes, void* workspace,
                                  int64_t* count_out, void* stream) {
  if (!verts || !planes || !workspace || !count_out) return CNR_E_ARG;
  if (F < 1) return CNR_E_SHAPE;
  const ClLayout L = cl_layout(F);
  if (L.nblk > 0x7fffffff) return CNR_E_SHAPE;
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(clip_count_kernel, dim3((unsigned)L.nblk), dim3(CL_BLOCK), 0, (hipStream_t)stream, verts, faces, F, planes,
                     (int*)ws);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL((blocks_scan_kernel<1, int64_t, int>), dim3(1), dim3(SCAN_THREADS), 0, (hipStream_t)stream, (const int*)ws, L.nblk,
                     (int64_t*)(ws + L.off_ofs), count_out);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_clip_box_emit(const float* verts, const int* faces, int64_t F, const double* planes, void* workspace,
                                 float* tris, void* stream) {
  if (!verts || !planes || !workspace || !tris) return CNR_E_ARG;
  if (F < 1) return CNR_E_SHAPE;
  const ClLayout L = cl_layout(F);
  if (L.nblk > 0x7fffffff) return CNR_E_SHAPE;
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(clip_emit_kernel, dim3((unsigned)L.nblk), dim3(CL_BLOCK), 0, (hipStream_t)stream, verts, faces, F, planes,
                     (const int64_t*)(ws + L.off_ofs), tris);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}
