// Meshing (src/trainer.py:62-123, src/vis.py:6-20, src/render_rays.py:97-121): marching cubes over a D^3 fp32 volume and the
// grid points it is evaluated on.  DESIGN.md §3.6 has the contract; tools/gen_mc_table.py writes the case table.
//
// Four launches, reduce-then-scan, no cross-workgroup waits, so the output order is fixed and every run is bit-identical:
//   classify (cnr_mc_count)   one thread per grid point p: its three owned edges (p -> p + e_axis, crossed when exactly one end
//                             is inside, v > level), the case of the cell whose min corner p is; per-workgroup vertex and
//                             triangle counts.
//   scan     (cnr_mc_count)   one workgroup: exclusive offsets of those counts (int64), totals to counts_out.
//   vertices (cnr_mc_emit)    vbase[p] = first vertex id of p's owned edges; the vertices and normals of those edges.
//   faces    (cnr_mc_emit)    the triangles of p's cell, in table order; an edge's vertex id is
//                             vbase[q] + popcount(mask[q] & ((1 << axis) - 1)) with q the edge's owning point.
// In-wave prefix sums run on ballots and mbcnt over the bit planes of the per-lane counts (counts < 8 for vertices, < 8 for
// triangles per cell: three planes each), the wave totals through LDS.
#include "cnr_common.h"
#include "geom_common.h"

#define MC_CONST __constant__ const
#include "mc_table.h"

using namespace cnr;

namespace {
constexpr int MC_BLOCK = 256;
constexpr int MC_WAVES = MC_BLOCK / 64;

// workspace: info (u16 per point: bits 0-2 owned crossed edges, bits 3-10 the cell's case) | vbase (i32 per point) |
// per-workgroup counts (i32 x 2) | their exclusive offsets (i64 x 2)
struct McLayout {
  int64_t n, nblk, off_vbase, off_cnt, off_ofs, bytes;
};
inline McLayout mc_layout(int D) {
  McLayout L;
  L.n = (int64_t)D * D * D;
  L.nblk = (L.n + MC_BLOCK - 1) / MC_BLOCK;
  L.off_vbase = align256(L.n * 2);
  L.off_cnt = L.off_vbase + align256(L.n * 4);
  L.off_ofs = L.off_cnt + align256(L.nblk * 2 * 4);
  L.bytes = L.off_ofs + align256(L.nblk * 2 * 8);
  return L;
}

__device__ __forceinline__ bool inside(float v, float level) { return v > level; }   // NaN: outside

// block-wide exclusive prefix of c (each < 8) in point order, and the block total
__device__ __forceinline__ int block_prefix(int c, int* s_wave, int* block_total) {
  int wtot;
  const int pre = wave_prefix_bits<3>(c, &wtot);
  return block_prefix_waves<MC_WAVES>(pre, wtot, s_wave, block_total);
}

__global__ __launch_bounds__(MC_BLOCK) void mc_classify_kernel(const float* __restrict__ vol, int D, float level,
                                                               uint16_t* __restrict__ info, int* __restrict__ blk_counts) {
  __shared__ int s_v[MC_WAVES], s_t[MC_WAVES];
  const int64_t n = (int64_t)D * D * D, DD = (int64_t)D * D;
  const int64_t p = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  int mask = 0, cs = 0;
  if (p < n) {
    const int i0 = (int)(p / DD), i1 = (int)((p / D) % D), i2 = (int)(p % D);
    const bool h0 = i0 < D - 1, h1 = i1 < D - 1, h2 = i2 < D - 1;
    // corner k at offset ((k >> 2) & 1, (k >> 1) & 1, k & 1); corners beyond the grid are never read
    bool in[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int a = (k >> 2) & 1, b = (k >> 1) & 1, c = k & 1;
      in[k] = false;
      if ((!a || h0) && (!b || h1) && (!c || h2)) in[k] = inside(vol[p + a * DD + b * D + c], level);
    }
    mask = (h0 && in[0] != in[4] ? 1 : 0) | (h1 && in[0] != in[2] ? 2 : 0) | (h2 && in[0] != in[1] ? 4 : 0);
    if (h0 && h1 && h2) {
#pragma unroll
      for (int k = 0; k < 8; ++k) cs |= (in[k] ? 1 : 0) << k;
    }
    info[p] = (uint16_t)(mask | (cs << 3));
  }
  int a, b;
  block_prefix(__popc(mask), s_v, &a);
  block_prefix(MC_NTRI[cs], s_t, &b);
  if (threadIdx.x == 0) {
    blk_counts[2 * blockIdx.x] = a;
    blk_counts[2 * blockIdx.x + 1] = b;
  }
}

// central difference in index space, one-sided at the border (np.gradient, edge_order 1)
__device__ __forceinline__ float grad_axis(const float* __restrict__ vol, int64_t q, int i, int D, int64_t stride) {
  if (i == 0) return vol[q + stride] - vol[q];
  if (i == D - 1) return vol[q] - vol[q - stride];
  return (vol[q + stride] - vol[q - stride]) * 0.5f;
}

__global__ __launch_bounds__(MC_BLOCK) void mc_vertices_kernel(const float* __restrict__ vol, int D, float level, int ascent,
                                                               const uint16_t* __restrict__ info, int* __restrict__ vbase,
                                                               const int64_t* __restrict__ ofs, float* __restrict__ verts,
                                                               float* __restrict__ normals) {
  __shared__ int s_w[MC_WAVES];
  const int64_t n = (int64_t)D * D * D, DD = (int64_t)D * D;
  const int64_t p = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  const int mask = p < n ? (info[p] & 7) : 0;
  int btot;
  const int pre = block_prefix(__popc(mask), s_w, &btot);
  if (p >= n) return;
  const int64_t id0 = ofs[2 * blockIdx.x] + pre;
  vbase[p] = (int)id0;
  if (!mask) return;
  const int idx[3] = {(int)(p / DD), (int)((p / D) % D), (int)(p % D)};
  const int64_t stride[3] = {DD, (int64_t)D, 1};
  const float v0 = vol[p];
  float g0[3];
#pragma unroll
  for (int b = 0; b < 3; ++b) g0[b] = grad_axis(vol, p, idx[b], D, stride[b]);
  int64_t id = id0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!((mask >> a) & 1)) continue;
    const int64_t q = p + stride[a];
    const float v1 = vol[q];
    float t = (level - v0) / (v1 - v0);
    t = fminf(fmaxf(t, 0.0f), 1.0f);      // NaN -> 0
    float* o = verts + id * 3;
    float* nn = normals + id * 3;
    float g[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const int j = b == a ? idx[b] + 1 : idx[b];
      const float g1 = grad_axis(vol, q, j, D, stride[b]);
      g[b] = g0[b] + t * (g1 - g0[b]);
      o[b] = (b == a ? (float)idx[b] + t : (float)idx[b]) / (float)(D - 1);
    }
    const float len = sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
    const float s = len > 0.0f ? (ascent ? 1.0f : -1.0f) : 0.0f;
#pragma unroll
    for (int b = 0; b < 3; ++b) nn[b] = len > 0.0f ? s * (g[b] / len) : 0.0f;
    ++id;
  }
}

__global__ __launch_bounds__(MC_BLOCK) void mc_faces_kernel(int D, int ascent, const uint16_t* __restrict__ info,
                                                            const int* __restrict__ vbase, const int64_t* __restrict__ ofs,
                                                            int* __restrict__ faces) {
  __shared__ int s_w[MC_WAVES];
  const int64_t n = (int64_t)D * D * D, DD = (int64_t)D * D;
  const int64_t p = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  const int cs = p < n ? (info[p] >> 3) : 0;
  const int nt = MC_NTRI[cs];
  int btot;
  const int pre = block_prefix(nt, s_w, &btot);
  if (!nt) return;
  const int64_t f0 = ofs[2 * blockIdx.x + 1] + pre;
  for (int t = 0; t < nt; ++t) {
    int id[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int lo = MC_EDGE_LO[MC_TRI[cs][3 * t + k]];
      const int corner = lo >> 2, axis = lo & 3;
      const int64_t q = p + ((corner >> 2) & 1) * DD + ((corner >> 1) & 1) * (int64_t)D + (corner & 1);
      id[k] = vbase[q] + __popc(info[q] & 7 & ((1 << axis) - 1));
    }
    int* o = faces + (f0 + t) * 3;
    o[0] = id[0];
    o[1] = ascent ? id[1] : id[2];
    o[2] = ascent ? id[2] : id[1];
  }
}

// torch.linspace(lo, hi, D) (two-sided: lo + step i below D / 2, hi - step (D - 1 - i) from there), meshgrid 'ij', then
// * scale, then r_k . p summed left to right (x, y, z) as the reference's (R_k * grid).sum(-1), then + t; no contractions.
__device__ __forceinline__ float linspace_at(float lo, float hi, float step, int i, int D) {
  return i < D / 2 ? __fadd_rn(lo, __fmul_rn(step, (float)i)) : __fsub_rn(hi, __fmul_rn(step, (float)(D - 1 - i)));
}

__global__ __launch_bounds__(256) void grid_points_kernel(int D, float lo, float hi, const float* __restrict__ scale,
                                                          const float* __restrict__ T, float* __restrict__ out) {
  const int64_t n = (int64_t)D * D * D, DD = (int64_t)D * D;
  const float step = __fdiv_rn(__fsub_rn(hi, lo), (float)(D - 1));
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
    float x[3] = {linspace_at(lo, hi, step, (int)(p / DD), D), linspace_at(lo, hi, step, (int)((p / D) % D), D),
                  linspace_at(lo, hi, step, (int)(p % D), D)};
    if (scale) {
#pragma unroll
      for (int b = 0; b < 3; ++b) x[b] = __fmul_rn(x[b], scale[b]);
    }
    float* o = out + p * 3;
    if (T) {
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const float* R = T + 4 * r;
        o[r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(R[0], x[0]), __fmul_rn(R[1], x[1])), __fmul_rn(R[2], x[2])), R[3]);
      }
    } else {
#pragma unroll
      for (int b = 0; b < 3; ++b) o[b] = x[b];
    }
  }
}

inline bool mc_dim_ok(int D) { return D >= 2 && D <= 512; }
}  // namespace

extern "C" int64_t cnr_mc_workspace_bytes(int D) {
  if (!mc_dim_ok(D)) return CNR_E_SHAPE;
  return mc_layout(D).bytes;
}

extern "C" int cnr_mc_count(const float* vol, int D, float level, void* workspace, int64_t* counts_out, void* stream) {
  if (!vol || !workspace || !counts_out || level != level) return CNR_E_ARG;
  if (!mc_dim_ok(D)) return CNR_E_SHAPE;
  const McLayout L = mc_layout(D);
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(mc_classify_kernel, dim3((unsigned)L.nblk), dim3(MC_BLOCK), 0, (hipStream_t)stream, vol, D, level,
                     (uint16_t*)ws, (int*)(ws + L.off_cnt));
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL((blocks_scan_kernel<2, int64_t, int>), dim3(1), dim3(SCAN_THREADS), 0, (hipStream_t)stream,
                     (const int*)(ws + L.off_cnt), L.nblk, (int64_t*)(ws + L.off_ofs), counts_out);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_mc_emit(const float* vol, int D, float level, int ascent, void* workspace, float* verts, float* normals,
                           int* faces, void* stream) {
  if (!vol || !workspace || !verts || !normals || !faces || level != level) return CNR_E_ARG;
  if (!mc_dim_ok(D)) return CNR_E_SHAPE;
  const McLayout L = mc_layout(D);
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(mc_vertices_kernel, dim3((unsigned)L.nblk), dim3(MC_BLOCK), 0, (hipStream_t)stream, vol, D, level,
                     ascent ? 1 : 0, (const uint16_t*)ws, (int*)(ws + L.off_vbase), (const int64_t*)(ws + L.off_ofs), verts,
                     normals);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(mc_faces_kernel, dim3((unsigned)L.nblk), dim3(MC_BLOCK), 0, (hipStream_t)stream, D, ascent ? 1 : 0,
                     (const uint16_t*)ws, (const int*)(ws + L.off_vbase), (const int64_t*)(ws + L.off_ofs), faces);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_grid_points(int D, float lo, float hi, const float* scale, const float* transform, float* out,
                               void* stream) {
  if (!out) return CNR_E_ARG;
  if (!mc_dim_ok(D)) return CNR_E_SHAPE;
  const int64_t n = (int64_t)D * D * D;
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(grid_points_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, (hipStream_t)stream,
                     D, lo, hi, scale, transform, out);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}
