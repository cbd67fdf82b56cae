// Triangle mesh of a TSDF volume (utils.TSDFVolume.extract_triangle_mesh): marching cubes over the sparse 16^3-voxel units of
// csrc/tsdf.hip, across unit faces, edges and corners and around unobserved voxels.  DESIGN.md §3.10 has the contract;
// tests/tsdfmesh_cpu.py restates it in numpy and the two agree bit for bit.
//
// One workgroup per unit.  It gathers the unit and its halo, voxels -1 .. 17 per axis, from the up to 27 units of its row of
// the `hood` table into one 19^3 LDS tile (27 KB; an unobserved voxel -- absent unit or weight 0 -- is one NaN bit pattern that
// no observed value keeps).  Everything the contract asks is decided from that tile: a cell's 8 corners, the four cells around
// an owned edge (back to voxel -1), the central differences at an edge's far end (up to voxel 17).  No atomics, no waits
// between workgroups, so the order is fixed and every run is bit-identical.
//   classify (cnr_tsdf_mesh_count)  per row of 19 tile voxels along z two bit masks (observed-and-next-observed, negative); per
//                                   voxel, from those masks alone: its three owned edges that a valid cell uses, the case of its
//                                   cell (0 unless valid), its first vertex id inside the unit; per-unit vertex and face counts.
//   scan     (cnr_tsdf_mesh_count)  one workgroup: exclusive int64 offsets of those counts, totals to counts_out.
//   vertices (cnr_tsdf_mesh_emit)   the tile again; position, colour and normal of every used edge in fp64.
//   faces    (cnr_tsdf_mesh_emit)   the triangles of every valid cell in table order; an edge's vertex id is the owning unit's
//                                   offset + the owning voxel's base + popcount of its lower used bits, through `hood`.
// Every fp64 product and sum is rounded on its own (no contraction in this file).
#include "cnr_common.h"
#include "geom_common.h"

#include <math.h>

#pragma clang fp contract(off)

#define MC_CONST __constant__ const
#include "mc_table.h"

using namespace cnr;

namespace {
constexpr int TM_BLOCK = 256;
constexpr int TM_WAVES = TM_BLOCK / 64;
constexpr int RES = 16;
constexpr int VOX = RES * RES * RES;
constexpr int TILE = RES + 3;                             // voxels -1 .. 17
constexpr int TILE2 = TILE * TILE, TILE3 = TILE2 * TILE;
constexpr int HOOD = 27;
constexpr uint32_t UNOBSERVED = 0xFFFFFFFFu;              // a NaN; an observed NaN is stored as QUIET_NAN
constexpr uint32_t QUIET_NAN = 0x7FC00000u;
constexpr int64_t MAX_VERTS_PER_UNIT = 3 * VOX;
static_assert(VOX == TM_BLOCK * RES, "a lane holds one row of voxels along z");

// workspace: info (u16 per voxel: bits 0-2 used owned edges, bits 3-10 the cell's case) | vbase (u16 per voxel: first vertex id
// inside its unit) | per-unit counts (i32 x 2: vertices, faces) | their exclusive offsets (i64 x 2)
struct MeshLayout {
  int64_t off_vbase, off_cnt, off_ofs, bytes;
};
inline MeshLayout mesh_layout(int64_t U) {
  MeshLayout L;
  L.off_vbase = align256(U * VOX * 2);
  L.off_cnt = L.off_vbase + align256(U * VOX * 2);
  L.off_ofs = L.off_cnt + align256(U * 2 * 4);
  L.bytes = L.off_ofs + align256(U * 2 * 8);
  return L;
}
inline bool units_ok(int64_t U) { return U >= 1 && U <= 0x7fffffff; }

__device__ __forceinline__ double key_axis(int64_t key, int a) {
  return (double)(((key >> ((2 - a) * AXIS_BITS)) & AXIS_MASK) - AXIS_BIAS);
}

// hood row of unit u -> s_hood[27] (-1 for an index outside [0, U)), then tile[e], e = (ti 19 + tj) 19 + tk, = voxel
// (ti - 1, tj - 1, tk - 1) of the unit's frame.  Lanes run along z.  Ends with a barrier.
__device__ __forceinline__ void stage_tile(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                           const int* __restrict__ hood, int64_t u, int64_t U, uint32_t* tile, int* s_hood) {
  const int t = threadIdx.x;
  if (t < HOOD) {
    const int v = hood[HOOD * u + t];
    s_hood[t] = v >= 0 && v < U ? v : -1;
  }
  __syncthreads();
  for (int e = t; e < TILE3; e += TM_BLOCK) {
    const int ti = e / TILE2, r = e - ti * TILE2, tj = r / TILE, tk = r - tj * TILE;
    // tile index 0 -> unit -1, voxel 15; 1 .. 16 -> the unit itself; 17, 18 -> unit +1, voxels 0, 1
    const int col = ((ti + 15) >> 4) * 9 + ((tj + 15) >> 4) * 3 + ((tk + 15) >> 4);
    const int nu = s_hood[col];
    uint32_t bits = UNOBSERVED;
    if (nu >= 0) {
      const int64_t q = (int64_t)nu * VOX + ((((ti - 1) & 15) * RES + ((tj - 1) & 15)) * RES + ((tk - 1) & 15));
      const float w = weight[q], f = tsdf[q];
      if (w != 0.0f) bits = f != f ? QUIET_NAN : __float_as_uint(f);
    }
    tile[e] = bits;
  }
  __syncthreads();
}

__global__ __launch_bounds__(TM_BLOCK) void mesh_count_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                              const int* __restrict__ hood, int64_t U, uint16_t* __restrict__ info,
                                                              uint16_t* __restrict__ vbase, int* __restrict__ cnt) {
  __shared__ uint32_t tile[TILE3];
  __shared__ uint32_t s_pair[TILE2], s_neg[TILE2];
  __shared__ int s_hood[HOOD], s_wv[TM_WAVES], s_wf[TM_WAVES];
  const int64_t u = blockIdx.x;
  const int t = threadIdx.x;
  stage_tile(tsdf, weight, hood, u, U, tile, s_hood);
  // per row along z: bit tk of s_pair = voxels tk and tk + 1 both observed, bit tk of s_neg = tsdf < 0 (never for unobserved)
  for (int r = t; r < TILE2; r += TM_BLOCK) {
    uint32_t obs = 0, neg = 0;
#pragma unroll
    for (int tk = 0; tk < TILE; ++tk) {
      const uint32_t b = tile[r * TILE + tk];
      obs |= (b != UNOBSERVED ? 1u : 0u) << tk;
      neg |= (__uint_as_float(b) < 0.0f ? 1u : 0u) << tk;
    }
    s_pair[r] = obs & (obs >> 1);
    s_neg[r] = neg;
  }
  __syncthreads();
  // lane t walks the voxels t 16 .. t 16 + 15 (i = t >> 4, j = t & 15, k the walk): lane order is voxel order
  const int I = (t >> 4) + 1, J = (t & 15) + 1;
  uint32_t z[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) z[a][b] = s_pair[(I + a - 1) * TILE + (J + b - 1)];
  }
  // bit tk of cXY: the cell with min corner (I - 1 + X, J - 1 + Y, tk) (tile indices) is valid
  const uint32_t c11 = z[1][1] & z[2][1] & z[1][2] & z[2][2], c10 = z[1][0] & z[2][0] & z[1][1] & z[2][1];
  const uint32_t c01 = z[0][1] & z[1][1] & z[0][2] & z[1][2], c00 = z[0][0] & z[1][0] & z[0][1] & z[1][1];
  const uint32_t around_x = c11 | c10, around_y = c11 | c01, around_z = c11 | c10 | c01 | c00;
  const uint32_t n00 = s_neg[I * TILE + J], n01 = s_neg[I * TILE + J + 1], n10 = s_neg[(I + 1) * TILE + J],
                 n11 = s_neg[(I + 1) * TILE + J + 1];
  uint32_t inf[RES];
  int nv = 0, nf = 0;
#pragma unroll
  for (int k = 0; k < RES; ++k) {
    const int K = k + 1;
    const uint32_t b0 = (n00 >> K) & 1, b1 = (n00 >> (K + 1)) & 1, b2 = (n01 >> K) & 1, b3 = (n01 >> (K + 1)) & 1;
    const uint32_t b4 = (n10 >> K) & 1, b5 = (n10 >> (K + 1)) & 1, b6 = (n11 >> K) & 1, b7 = (n11 >> (K + 1)) & 1;
    // an owned edge is used when it is crossed and one of the four cells around it is valid (which makes both ends observed)
    const uint32_t used = (((around_x >> (K - 1)) & 3) != 0 && b0 != b4 ? 1u : 0u) | (((around_y >> (K - 1)) & 3) != 0 && b0 != b2 ? 2u : 0u) |
                          (((around_z >> K) & 1) != 0 && b0 != b1 ? 4u : 0u);
    const uint32_t cs = (c11 >> K) & 1 ? b0 | b1 << 1 | b2 << 2 | b3 << 3 | b4 << 4 | b5 << 5 | b6 << 6 | b7 << 7 : 0u;
    inf[k] = used | cs << 3;
    nv += __popc(used);
    nf += MC_NTRI[cs];
  }
  int wv, wf, tot_v, tot_f;
  const int pv = wave_prefix_bits<6>(nv, &wv), pf = wave_prefix_bits<7>(nf, &wf);       // nv <= 48, nf <= 80
  int run = block_prefix_waves<TM_WAVES>(pv, wv, s_wv, &tot_v);
  block_prefix_waves<TM_WAVES>(pf, wf, s_wf, &tot_f);
  uint32_t pi[RES / 2], pb[RES / 2];
#pragma unroll
  for (int k = 0; k < RES; k += 2) {
    const int v0 = run, v1 = run + __popc(inf[k] & 7);
    run = v1 + __popc(inf[k + 1] & 7);
    pi[k >> 1] = inf[k] | inf[k + 1] << 16;
    pb[k >> 1] = (uint32_t)v0 | (uint32_t)v1 << 16;
  }
  uint4* oi = (uint4*)(info + u * VOX + t * RES);
  uint4* ob = (uint4*)(vbase + u * VOX + t * RES);
  oi[0] = make_uint4(pi[0], pi[1], pi[2], pi[3]);
  oi[1] = make_uint4(pi[4], pi[5], pi[6], pi[7]);
  ob[0] = make_uint4(pb[0], pb[1], pb[2], pb[3]);
  ob[1] = make_uint4(pb[4], pb[5], pb[6], pb[7]);
  if (t == 0) {
    cnt[2 * u] = tot_v;
    cnt[2 * u + 1] = tot_f;
  }
}

// the tsdf gradient's component along the axis of tile stride `s` at tile element e (observed): central where both
// neighbours are observed, one-sided where one is, else 0
__device__ __forceinline__ double grad_at(const uint32_t* tile, int e, int s) {
  const uint32_t bm = tile[e - s], bp = tile[e + s];
  const double f = (double)__uint_as_float(tile[e]), fm = (double)__uint_as_float(bm), fp = (double)__uint_as_float(bp);
  const bool om = bm != UNOBSERVED, op = bp != UNOBSERVED;
  if (om && op) return (fp - fm) * 0.5;
  if (op) return fp - f;
  if (om) return f - fm;
  return 0.0;
}

__global__ __launch_bounds__(TM_BLOCK) void mesh_vertices_kernel(const int64_t* __restrict__ units, const float* __restrict__ tsdf,
                                                                 const float* __restrict__ weight, const float* __restrict__ colors,
                                                                 const int* __restrict__ hood, int64_t U, double voxel,
                                                                 const uint16_t* __restrict__ info, const uint16_t* __restrict__ vbase,
                                                                 const int64_t* __restrict__ ofs, double* __restrict__ verts,
                                                                 double* __restrict__ cols, double* __restrict__ normals) {
  __shared__ uint32_t tile[TILE3];
  __shared__ int s_hood[HOOD];
  const int64_t u = blockIdx.x;
  const int t = threadIdx.x, i = t >> 4, j = t & 15;
  // the lane's 16 x 3 used bits in one word, bit 3 k + axis: its vertices are the set bits in ascending order
  const uint4* pi = (const uint4*)(info + u * VOX + t * RES);
  const uint4 lo = pi[0], hi = pi[1];
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  uint64_t used = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) used |= (uint64_t)((w[q] & 7) | ((w[q] >> 16) & 7) << 3) << (6 * q);
  const int64_t id0 = ofs[2 * u] + vbase[u * VOX + t * RES];
  stage_tile(tsdf, weight, hood, u, U, tile, s_hood);
  if (!used) return;
  const int64_t key = units[u];
  const double unit_len = (double)RES * voxel;
  const double cx = key_axis(key, 0) * unit_len + ((double)i + 0.5) * voxel, cy = key_axis(key, 1) * unit_len + ((double)j + 0.5) * voxel;
  const double oz = key_axis(key, 2) * unit_len;
  for (uint64_t m = used; m; m &= m - 1) {
    const int b = __ffsll((unsigned long long)m) - 1, k = b / 3, a = b - 3 * k;
    const int64_t id = id0 + __popcll(used & (((uint64_t)1 << b) - 1));
    const int e0 = ((i + 1) * TILE + (j + 1)) * TILE + (k + 1), e1 = e0 + (a == 0 ? TILE2 : (a == 1 ? TILE : 1));
    const double r0 = fabs((double)__uint_as_float(tile[e0])), r1 = fabs((double)__uint_as_float(tile[e1])), rs = r0 + r1;
    const double cz = oz + ((double)k + 0.5) * voxel;
    const double p0 = a == 0 ? cx : (a == 1 ? cy : cz), p1 = p0 + voxel;
    const double pa = (p0 * r1 + p1 * r0) / rs;
    verts[3 * id] = a == 0 ? pa : cx;
    verts[3 * id + 1] = a == 1 ? pa : cy;
    verts[3 * id + 2] = a == 2 ? pa : cz;
    // the far end may be voxel 0 of the next unit along the axis
    const int fi = i + (a == 0), fj = j + (a == 1), fk = k + (a == 2);
    const int nu = s_hood[13 + 9 * (fi >> 4) + 3 * (fj >> 4) + (fk >> 4)];
    const int64_t q0 = 3 * (u * VOX + t * RES + k);
    const int64_t q1 = nu >= 0 ? 3 * ((int64_t)nu * VOX + (((fi & 15) * RES + (fj & 15)) * RES + (fk & 15))) : q0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const double c0 = (double)colors[q0 + ch], c1 = (double)colors[q1 + ch];
      cols[3 * id + ch] = (c0 * r1 + c1 * r0) / rs / 255.0;
    }
    const double nx = (grad_at(tile, e0, TILE2) * r1 + grad_at(tile, e1, TILE2) * r0) / rs;
    const double ny = (grad_at(tile, e0, TILE) * r1 + grad_at(tile, e1, TILE) * r0) / rs;
    const double nz = (grad_at(tile, e0, 1) * r1 + grad_at(tile, e1, 1) * r0) / rs;
    const double len = __dsqrt_rn((nx * nx + ny * ny) + nz * nz);
    const bool has = len > 0.0;                            // false for NaN too
    normals[3 * id] = has ? nx / len : 0.0;
    normals[3 * id + 1] = has ? ny / len : 0.0;
    normals[3 * id + 2] = has ? nz / len : 0.0;
  }
}

__global__ __launch_bounds__(TM_BLOCK) void mesh_faces_kernel(const int* __restrict__ hood, int64_t U, const uint16_t* __restrict__ info,
                                                              const uint16_t* __restrict__ vbase, const int64_t* __restrict__ ofs,
                                                              int* __restrict__ faces) {
  __shared__ int s_hood[HOOD], s_w[TM_WAVES];
  const int64_t u = blockIdx.x;
  const int t = threadIdx.x, i = t >> 4, j = t & 15;
  if (t < HOOD) {
    const int v = hood[HOOD * u + t];
    s_hood[t] = v >= 0 && v < U ? v : -1;
  }
  const uint4* pi = (const uint4*)(info + u * VOX + t * RES);
  const uint4 lo = pi[0], hi = pi[1];
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  uint64_t cs_lo = 0, cs_hi = 0;                           // the lane's 16 cases, 8 bits each
  int nf = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const uint32_t a = (w[q] >> 3) & 255, b = (w[q] >> 19) & 255;
    const uint64_t two = (uint64_t)(a | b << 8) << (16 * (q & 3));
    if (q < 4) cs_lo |= two; else cs_hi |= two;
    nf += MC_NTRI[a] + MC_NTRI[b];
  }
  int wf, tot;
  const int pf = wave_prefix_bits<7>(nf, &wf);
  int64_t f = ofs[2 * u + 1] + block_prefix_waves<TM_WAVES>(pf, wf, s_w, &tot);         // (its barrier publishes s_hood too)
  if (!nf) return;
  for (int k = 0; k < RES; ++k) {
    const int cs = (int)(((k < 8 ? cs_lo : cs_hi) >> (8 * (k & 7))) & 255);
    const int nt = MC_NTRI[cs];
    for (int tr = 0; tr < nt; ++tr, ++f) {
      int id[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int el = MC_EDGE_LO[MC_TRI[cs][3 * tr + c]];
        const int corner = el >> 2, axis = el & 3;
        const int oi = i + ((corner >> 2) & 1), oj = j + ((corner >> 1) & 1), ok = k + (corner & 1);
        const int nu = s_hood[13 + 9 * (oi >> 4) + 3 * (oj >> 4) + (ok >> 4)];
        id[c] = 0;
        if (nu >= 0) {                                     // always: the cell is valid, so the owner's unit exists
          const int64_t q = (int64_t)nu * VOX + (((oi & 15) * RES + (oj & 15)) * RES + (ok & 15));
          id[c] = (int)(ofs[2 * (int64_t)nu] + vbase[q] + __popc(info[q] & 7 & ((1 << axis) - 1)));
        }
      }
      // the table's right-hand normal points to the negative corners: swap two for increasing tsdf
      faces[3 * f] = id[0];
      faces[3 * f + 1] = id[2];
      faces[3 * f + 2] = id[1];
    }
  }
}
}  // namespace

// ---- entry points ------------------------------------------------------------------------------------------------------
extern "C" int64_t cnr_tsdf_mesh_workspace_bytes(int64_t U) {
  if (!units_ok(U)) return CNR_E_SHAPE;
  return mesh_layout(U).bytes;
}

extern "C" int cnr_tsdf_mesh_count(const float* tsdf, const float* weight, const int* hood, int64_t U, void* workspace,
                                   int64_t* counts_out, void* stream) {
  if (!tsdf || !weight || !hood || !workspace || !counts_out) return CNR_E_ARG;
  if (!units_ok(U)) return CNR_E_SHAPE;
  const MeshLayout L = mesh_layout(U);
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(mesh_count_kernel, dim3((unsigned)U), dim3(TM_BLOCK), 0, (hipStream_t)stream, tsdf, weight, hood, U,
                     (uint16_t*)ws, (uint16_t*)(ws + L.off_vbase), (int*)(ws + L.off_cnt));
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL((blocks_scan_kernel<2, int64_t, int>), dim3(1), dim3(SCAN_THREADS), 0, (hipStream_t)stream,
                     (const int*)(ws + L.off_cnt), U, (int64_t*)(ws + L.off_ofs), counts_out);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_tsdf_mesh_emit(const int64_t* units, const float* tsdf, const float* weight, const float* colors, const int* hood,
                                  int64_t U, double voxel, void* workspace, double* verts, double* colors_out, double* normals,
                                  int* faces, void* stream) {
  if (!units || !tsdf || !weight || !colors || !hood || !workspace || !verts || !colors_out || !normals || !faces) return CNR_E_ARG;
  if (!units_ok(U) || !(voxel > 0.0)) return CNR_E_SHAPE;
  const MeshLayout L = mesh_layout(U);
  char* ws = (char*)workspace;
  const uint16_t* info = (const uint16_t*)ws;
  const uint16_t* vbase = (const uint16_t*)(ws + L.off_vbase);
  const int64_t* ofs = (const int64_t*)(ws + L.off_ofs);
  if (U * MAX_VERTS_PER_UNIT > 0x7fffffff) {
    // only a volume this large can hold 2^31 vertices, which i32 faces cannot name: read the count back before emitting
    int64_t last_ofs = 0;
    int last_cnt = 0;
    hipError_t e = hipMemcpyAsync(&last_ofs, ofs + 2 * (U - 1), sizeof(last_ofs), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(&last_cnt, (const int*)(ws + L.off_cnt) + 2 * (U - 1), sizeof(last_cnt), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    if (last_ofs + last_cnt > 0x7fffffff) return CNR_E_SHAPE;
  }
  hipLaunchKernelGGL(mesh_vertices_kernel, dim3((unsigned)U), dim3(TM_BLOCK), 0, (hipStream_t)stream, units, tsdf, weight, colors, hood,
                     U, voxel, info, vbase, ofs, verts, colors_out, normals);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(mesh_faces_kernel, dim3((unsigned)U), dim3(TM_BLOCK), 0, (hipStream_t)stream, hood, U, info, vbase, ofs, faces);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}
