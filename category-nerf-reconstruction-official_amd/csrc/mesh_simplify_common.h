// Arithmetic of the mesh simplification unit (csrc/mesh_simplify.hip), written once for the device and
// for a plain host compiler: tests/meshsimplify_solve_main.cpp runs these very functions without a GPU.  Everything is fp64
// and every expression is written in the order it is meant to be evaluated in; the units that include this header compile
// with floating-point contraction off, so a product is rounded before it is added.
//
//   face_record    the ten products of one face's plane (n, d), n = (q1 - q0) x (q2 - q0) NOT normalised (its length is twice
//                  the area, so the quadric is weighted by Lindstrom's squared area), d = n . q0:
//                    nx nx, nx ny, nx nz, ny ny, ny nz, nz nz, nx d, ny d, nz d, d d
//                  i.e. A (upper triangle, row-major), b = n d, c = d d of  (n . x - d)^2 = x^T A x - 2 b^T x + c.
//   lane_partial / tree_combine / group_sum
//                  the fixed-order sum of one segment by a group of GROUP = 16 lanes: lane l adds the positions l, l + 16, ...
//                  in ascending order starting from 0.0, then a[l] += a[l ^ 8], ^ 4, ^ 2, ^ 1 and lane 0 holds the sum.
//   jacobi3        cyclic Jacobi on a symmetric 3 x 3: JACOBI_SWEEPS sweeps over (0,1), (0,2), (1,2), always all of them.
//   solve_quadric  x = mean + pinv_tau(A) (b - A mean): eigenvalues <= tau * lambda_max are dropped; lambda_max <= 0 (a zero
//                  quadric) drops all of them and leaves the mean.
//   clamp_to_cell  per axis into [(i - 0.5) cell, (i + 0.5) cell]; -> true when an axis moved.
//   quadric_error  x^T A x - 2 b^T x + c in the order written there.
//   to_f32_in_cell (float)(q + min), then at most one step of one unit in the last place back towards the cell when the
//                  rounding to fp32 left it, so that lo <= (double)result - (double)min <= hi holds for the fp32 value too.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CNR_SIMP_HD __host__ __device__
#else
#define CNR_SIMP_HD
#endif

// a product is rounded before it is added, in this header too (the including unit's own pragma comes after its includes);
// the host test is built by g++ for baseline x86-64, which has no fused multiply-add to contract into
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace cnr {
namespace simp {

constexpr int RECORD = 10;
constexpr int GROUP = 16;
constexpr int JACOBI_SWEEPS = 8;

struct FaceRecord {
  double k[RECORD];
};

// n = u x v with each product rounded, then the difference
CNR_SIMP_HD inline void cross3(const double* u, const double* v, double* n) {
  n[0] = u[1] * v[2] - u[2] * v[1];
  n[1] = u[2] * v[0] - u[0] * v[2];
  n[2] = u[0] * v[1] - u[1] * v[0];
}

CNR_SIMP_HD inline FaceRecord face_record(const double* q0, const double* q1, const double* q2) {
  const double u[3] = {q1[0] - q0[0], q1[1] - q0[1], q1[2] - q0[2]};
  const double v[3] = {q2[0] - q0[0], q2[1] - q0[1], q2[2] - q0[2]};
  double n[3];
  cross3(u, v, n);
  const double d = (n[0] * q0[0] + n[1] * q0[1]) + n[2] * q0[2];
  FaceRecord r;
  r.k[0] = n[0] * n[0], r.k[1] = n[0] * n[1], r.k[2] = n[0] * n[2];
  r.k[3] = n[1] * n[1], r.k[4] = n[1] * n[2], r.k[5] = n[2] * n[2];
  r.k[6] = n[0] * d, r.k[7] = n[1] * d, r.k[8] = n[2] * d, r.k[9] = d * d;
  return r;
}

// lane's share of a segment of n positions; load(j) = the value at position j
template <class Load>
CNR_SIMP_HD inline double lane_partial(Load load, int64_t n, int lane) {
  double acc = 0.0;
  for (int64_t j = lane; j < n; j += GROUP) acc = acc + load(j);
  return acc;
}

// the lanes' tree on an array of GROUP partial sums (the device does the same with lane exchanges); a[0] = the sum
CNR_SIMP_HD inline double tree_combine(double* a) {
  for (int d = GROUP / 2; d > 0; d >>= 1)
    for (int l = 0; l < d; ++l) a[l] = a[l] + a[l ^ d];               // (the lanes >= d no longer reach lane 0)
  return a[0];
}

template <class Load>
CNR_SIMP_HD inline double group_sum(Load load, int64_t n) {
  double a[GROUP];
  for (int l = 0; l < GROUP; ++l) a[l] = lane_partial(load, n, l);
  return tree_combine(a);
}

// A (symmetric, a[i][j]) -> eigenvalues w[i] with eigenvectors the COLUMNS of v
CNR_SIMP_HD inline void jacobi3(double a[3][3], double* w, double v[3][3]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
    for (int pq = 0; pq < 3; ++pq) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      const double apq = a[p][q];
      if (apq == 0.0) continue;
      const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
      const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
      const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
      const int r = 3 - p - q;
      const double arp = a[r][p], arq = a[r][q];
      a[p][p] = a[p][p] - t * apq;
      a[q][q] = a[q][q] + t * apq;
      a[p][q] = a[q][p] = 0.0;
      a[r][p] = a[p][r] = c * arp - s * arq;
      a[r][q] = a[q][r] = s * arp + c * arq;
      for (int i = 0; i < 3; ++i) {
        const double vip = v[i][p], viq = v[i][q];
        v[i][p] = c * vip - s * viq;
        v[i][q] = s * vip + c * viq;
      }
    }
  }
  for (int i = 0; i < 3; ++i) w[i] = a[i][i];
}

// Q = the ten sums of face_record over a cluster; -> x (3), the number of eigenvalues kept
CNR_SIMP_HD inline int solve_quadric(const double* Q, const double* mean, double tau, double* x) {
  double a[3][3] = {{Q[0], Q[1], Q[2]}, {Q[1], Q[3], Q[4]}, {Q[2], Q[4], Q[5]}};
  double r[3];
  for (int i = 0; i < 3; ++i) r[i] = Q[6 + i] - ((a[i][0] * mean[0] + a[i][1] * mean[1]) + a[i][2] * mean[2]);
  double w[3], v[3][3];
  jacobi3(a, w, v);
  const double wmax = fmax(fmax(w[0], w[1]), w[2]);
  x[0] = mean[0], x[1] = mean[1], x[2] = mean[2];
  int kept = 0;
  if (!(wmax > 0.0)) return 0;
  for (int k = 0; k < 3; ++k) {
    if (!(w[k] > tau * wmax)) continue;
    const double g = ((v[0][k] * r[0] + v[1][k] * r[1]) + v[2][k] * r[2]) / w[k];
    for (int i = 0; i < 3; ++i) x[i] = x[i] + v[i][k] * g;
    ++kept;
  }
  return kept;
}

CNR_SIMP_HD inline void cell_bounds(int64_t i, double cell, double* lo, double* hi) {
  *lo = ((double)i - 0.5) * cell;
  *hi = ((double)i + 0.5) * cell;
}

// i (3) = the cluster's cell indices -> true when an axis moved; a NaN coordinate goes to the lower bound
CNR_SIMP_HD inline bool clamp_to_cell(double* x, const int64_t* i, double cell) {
  bool moved = false;
  for (int a = 0; a < 3; ++a) {
    double lo, hi;
    cell_bounds(i[a], cell, &lo, &hi);
    if (!(x[a] >= lo)) x[a] = lo, moved = true;
    else if (x[a] > hi) x[a] = hi, moved = true;
  }
  return moved;
}

CNR_SIMP_HD inline double quadric_error(const double* Q, const double* x) {
  const double ax = (Q[0] * x[0] + Q[1] * x[1]) + Q[2] * x[2];
  const double ay = (Q[1] * x[0] + Q[3] * x[1]) + Q[4] * x[2];
  const double az = (Q[2] * x[0] + Q[4] * x[1]) + Q[5] * x[2];
  const double xax = (x[0] * ax + x[1] * ay) + x[2] * az;
  const double bx = (Q[6] * x[0] + Q[7] * x[1]) + Q[8] * x[2];
  return (xax - 2.0 * bx) + Q[9];
}

CNR_SIMP_HD inline float to_f32_in_cell(double q, float mn, int64_t i, double cell) {
  double lo, hi;
  cell_bounds(i, cell, &lo, &hi);
  float f = (float)(q + (double)mn);
  const double back = (double)f - (double)mn;
  if (back > hi) f = nextafterf(f, -INFINITY);
  else if (back < lo) f = nextafterf(f, INFINITY);
  return f;
}

// the key of cnr_voxel_keys -> its three cell indices
CNR_SIMP_HD inline void key_cells(int64_t key, int64_t* i) {
  i[0] = (key >> 42) & 0x1fffff, i[1] = (key >> 21) & 0x1fffff, i[2] = key & 0x1fffff;
}

}  // namespace simp
}  // namespace cnr
