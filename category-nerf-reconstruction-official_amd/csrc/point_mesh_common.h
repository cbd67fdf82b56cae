// What csrc/point_mesh.hip (brute force) and csrc/point_mesh_index.hip (tile-box index) share: the face record, its
// construction and the per-pair code, so that both evaluate a (query, face) pair through the one device function and agree
// bit for bit.  DESIGN.md §3.20 has the contract; tests/pointmesh_cpu.py restates it in numpy.  Include after cnr_common.h,
// in a unit compiled under `#pragma clang fp contract(off)` (repeated below: the pragma is scoped to the file it stands in).
#pragma once
#include "cnr_common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace cnr {
constexpr int PM_REC_F4 = 4;                              // float4 per record: (a, ab.x) (ab.yz, ac.xy) (ac.z, e00, e01, e11) (n, w)
constexpr int64_t PM_REC_BYTES = PM_REC_F4 * 16;

struct PmRec {
  float ax, ay, az, abx, aby, abz, acx, acy, acz, e00, e01, e11, nx, ny, nz;
};
__device__ __forceinline__ PmRec pm_unpack(float4 r0, float4 r1, float4 r2, float4 r3) {
  return PmRec{r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z};
}

__device__ __forceinline__ float pm_dot(float ux, float uy, float uz, float vx, float vy, float vz) {
  return (ux * vx + uy * vy) + uz * vz;
}

// The closest point of the record's triangle to q, as r = closest - q; returns r.r.  Ericson's seven regions (Real-Time
// Collision Detection 5.1.5) with d3 .. d6 taken from d1, d2 and the record's edge products; in the vertex and edge regions
// the barycentric numerators and the denominator are selected first, one division; in the interior r = -(n . ap) n with the
// record's unit normal (the barycentric form loses a sliver's closest point to the cancellation in va, vb, vc).
__device__ __forceinline__ float pm_pair(float qx, float qy, float qz, const PmRec& f, float* rx, float* ry, float* rz) {
  const float apx = qx - f.ax, apy = qy - f.ay, apz = qz - f.az;
  const float d1 = pm_dot(f.abx, f.aby, f.abz, apx, apy, apz);
  const float d2 = pm_dot(f.acx, f.acy, f.acz, apx, apy, apz);
  const float d3 = d1 - f.e00, d4 = d2 - f.e01;           // ab.bp, ac.bp with bp = ap - ab
  const float d5 = d1 - f.e01, d6 = d2 - f.e11;           // ab.cp, ac.cp with cp = ap - ac
  const float vc = d1 * d4 - d3 * d2;
  const float vb = d5 * d2 - d1 * d6;
  const float va = d3 * d6 - d5 * d4;
  const float g43 = d4 - d3, g56 = d5 - d6;
  // from the last region to the first, so that the first one that holds wins
  float nv = 0.0f, nw = 0.0f, den = 1.0f;
  bool interior = true;
  if (va <= 0.0f && g43 >= 0.0f && g56 >= 0.0f) {         // edge bc
    nv = g56;
    nw = g43;
    den = g43 + g56;
    interior = false;
  }
  if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {           // edge ac
    nv = 0.0f;
    nw = d2;
    den = d2 - d6;
    interior = false;
  }
  if (d6 >= 0.0f && d5 <= d6) {                           // vertex c
    nv = 0.0f;
    nw = 1.0f;
    den = 1.0f;
    interior = false;
  }
  if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {           // edge ab
    nv = d1;
    nw = 0.0f;
    den = d1 - d3;
    interior = false;
  }
  if (d3 >= 0.0f && d4 <= d3) {                           // vertex b
    nv = 1.0f;
    nw = 0.0f;
    den = 1.0f;
    interior = false;
  }
  if (d1 <= 0.0f && d2 <= 0.0f) {                         // vertex a
    nv = 0.0f;
    nw = 0.0f;
    den = 1.0f;
    interior = false;
  }
  if (!(den > 0.0f)) {                                    // the edge products lost below the rounding of d1, d2: vertex a
    nv = 0.0f;
    nw = 0.0f;
    den = 1.0f;
  }
  const float inv = 1.0f / den;
  const float v = nv * inv, w = nw * inv;
  *rx = (v * f.abx + w * f.acx) - apx;
  *ry = (v * f.aby + w * f.acy) - apy;
  *rz = (v * f.abz + w * f.acz) - apz;
  if (interior) {
    const float h = 0.0f - pm_dot(f.nx, f.ny, f.nz, apx, apy, apz);
    *rx = h * f.nx;
    *ry = h * f.ny;
    *rz = h * f.nz;
  }
  return pm_dot(*rx, *ry, *rz, *rx, *ry, *rz);
}

// the three corners of face f (faces == NULL: a soup)
__device__ __forceinline__ void pm_corners(const float* __restrict__ verts, const int* __restrict__ faces, int64_t f,
                                           float (&c)[3][3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int64_t v = faces ? (int64_t)faces[3 * f + k] : 3 * f + k;
    c[k][0] = verts[3 * v];
    c[k][1] = verts[3 * v + 1];
    c[k][2] = verts[3 * v + 2];
  }
}

// The record of the face with corners c, into rec[0 .. 4); `w` fills the free sixteenth float.
__device__ __forceinline__ void pm_make_record(const float (&c)[3][3], float w, float4* __restrict__ rec) {
  float ax = c[0][0], ay = c[0][1], az = c[0][2];
  float abx = c[1][0] - ax, aby = c[1][1] - ay, abz = c[1][2] - az;
  float acx = c[2][0] - ax, acy = c[2][1] - ay, acz = c[2][2] - az;
  float e00 = pm_dot(abx, aby, abz, abx, aby, abz);
  float e01 = pm_dot(abx, aby, abz, acx, acy, acz);
  float e11 = pm_dot(acx, acy, acz, acx, acy, acz);
  // ab x ac in fp64 of the fp32 edges: the products are exact, so it is zero exactly when the edges are parallel or zero
  const double nx = (double)aby * (double)acz - (double)abz * (double)acy;
  const double ny = (double)abz * (double)acx - (double)abx * (double)acz;
  const double nz = (double)abx * (double)acy - (double)aby * (double)acx;
  const double nn = (nx * nx + ny * ny) + nz * nz;
  float ux = 0.0f, uy = 0.0f, uz = 0.0f;                  // the unit normal; a degenerate face never reaches the interior
  if (nx == 0.0 && ny == 0.0 && nz == 0.0) {
    // the longest edge (ab, then ac, then bc, a later one only when strictly longer) as a triangle with ac = 0
    const float bcx = c[2][0] - c[1][0], bcy = c[2][1] - c[1][1], bcz = c[2][2] - c[1][2];
    const float e22 = pm_dot(bcx, bcy, bcz, bcx, bcy, bcz);
    float best = e00;
    if (e11 > best) {
      best = e11;
      abx = acx;
      aby = acy;
      abz = acz;
    }
    if (e22 > best) {
      best = e22;
      ax = c[1][0];
      ay = c[1][1];
      az = c[1][2];
      abx = bcx;
      aby = bcy;
      abz = bcz;
    }
    e00 = best;
    e01 = 0.0f;
    e11 = 0.0f;
    acx = 0.0f;
    acy = 0.0f;
    acz = 0.0f;
  } else {
    const double len = sqrt(nn);
    ux = (float)(nx / len);
    uy = (float)(ny / len);
    uz = (float)(nz / len);
  }
  rec[0] = make_float4(ax, ay, az, abx);
  rec[1] = make_float4(aby, abz, acx, acy);
  rec[2] = make_float4(acz, e00, e01, e11);
  rec[3] = make_float4(ux, uy, uz, w);
}
}  // namespace cnr
