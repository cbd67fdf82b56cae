// Stand-alone host program: the arithmetic of csrc/mesh_simplify_common.h, the very functions the simplification kernels
// call -- the face record, the 16-lane group sum, the Jacobi solve of a cluster's quadric, the clamp to the cluster's cell and
// the rounding to fp32 inside it.  The solve is checked where the answer is known in closed form: one plane (rank 1: only the
// normal component of the mean moves), two planes (rank 2: the point lands on their edge and keeps the mean's place along it),
// three orthogonal planes (the corner), a zero quadric (the mean, bit for bit), and random symmetric positive definite
// matrices by the residual |A x - b|.  Prints "ok <checks>" and exits 0, or names the first mismatch and exits 1.
// Built and run by tests/test_meshsimplify_host.py (no GPU, no HIP headers).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "mesh_simplify_common.h"

namespace simp = cnr::simp;

static int checks = 0;
#define REQUIRE(cond, ...)                      \
  do {                                          \
    ++checks;                                   \
    if (!(cond)) {                              \
      std::printf("FAILED %s: ", #cond);        \
      std::printf(__VA_ARGS__);                 \
      std::printf("\n");                        \
      std::exit(1);                             \
    }                                           \
  } while (0)

static uint32_t rng_state = 2463534242u;
static double rnd() { rng_state = rng_state * 1664525u + 1013904223u; return (double)(rng_state >> 8) / 16777216.0; }

static const double EPS = std::numeric_limits<double>::epsilon();

// the quadric of the planes n_k . x = d_k, each with weight 1: Q as face_record lays it out
static void add_plane(double* Q, const double* n, double d) {
  Q[0] += n[0] * n[0], Q[1] += n[0] * n[1], Q[2] += n[0] * n[2], Q[3] += n[1] * n[1], Q[4] += n[1] * n[2], Q[5] += n[2] * n[2];
  Q[6] += n[0] * d, Q[7] += n[1] * d, Q[8] += n[2] * d, Q[9] += d * d;
}
static double dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// lane 0 after the distances 8, 4, 2, 1, written as the tree it is: T(l, 16) = p[l], T(l, s) = T(l, 2 s) + T(l + s, 2 s)
static double tree(const double* p, int l, int s) { return s == simp::GROUP ? p[l] : tree(p, l, 2 * s) + tree(p, l + s, 2 * s); }

static void check_record() {
  const double q0[3] = {1, 2, 3}, q1[3] = {2, 2, 3}, q2[3] = {1, 4, 3};           // u = (1,0,0), v = (0,2,0): n = (0,0,2), d = 6
  const simp::FaceRecord r = simp::face_record(q0, q1, q2);
  const double want[10] = {0, 0, 0, 0, 0, 4, 0, 0, 12, 36};
  for (int k = 0; k < 10; ++k) REQUIRE(r.k[k] == want[k], "record %d: %g", k, r.k[k]);
  const double x[3] = {7, -5, 3.5};                                                // (n . x - d)^2 = (7 - 6)^2 = 1
  REQUIRE(simp::quadric_error(r.k, x) == 1.0, "error %g", simp::quadric_error(r.k, x));
}

static void check_group_sum() {
  const int lengths[6] = {0, 1, 15, 16, 17, 33};
  for (int n : lengths) {
    std::vector<double> a(n);
    for (double& v : a) v = rnd() * 2.0 - 1.0;
    double lanes[simp::GROUP];
    for (int l = 0; l < simp::GROUP; ++l) {
      lanes[l] = 0.0;
      for (int j = l; j < n; j += simp::GROUP) lanes[l] = lanes[l] + a[j];
    }
    const double want = tree(lanes, 0, 1);
    const double* base = a.data();
    const double got = simp::group_sum([base](int64_t j) { return base[j]; }, n);
    REQUIRE(got == want, "group sum of %d: %.17g != %.17g", n, got, want);
    if (n == 0) REQUIRE(got == 0.0 && !std::signbit(got), "empty segment");
    if (n == 1) REQUIRE(got == a[0], "one position");
  }
}

static void check_solve() {
  const double tau = 1e-3;
  for (int trial = 0; trial < 200; ++trial) {
    // an orthonormal frame from two random vectors
    double e0[3] = {rnd() - 0.5, rnd() - 0.5, rnd() - 0.5}, t[3] = {rnd() - 0.5, rnd() - 0.5, rnd() - 0.5}, e1[3], e2[3];
    double l = std::sqrt(dot(e0, e0));
    for (double& v : e0) v /= l;
    simp::cross3(e0, t, e1);
    l = std::sqrt(dot(e1, e1));
    if (l < 0.1) continue;
    for (double& v : e1) v /= l;
    simp::cross3(e0, e1, e2);
    const double* frame[3] = {e0, e1, e2};
    const double w[3] = {0.5 + rnd(), 0.5 + rnd(), 0.5 + rnd()}, d[3] = {rnd() - 0.5, rnd() - 0.5, rnd() - 0.5};
    const double mean[3] = {rnd() - 0.5, rnd() - 0.5, rnd() - 0.5};
    for (int rank = 0; rank <= 3; ++rank) {
      double Q[10] = {0};
      for (int k = 0; k < rank; ++k) {
        const double n[3] = {w[k] * frame[k][0], w[k] * frame[k][1], w[k] * frame[k][2]};
        add_plane(Q, n, w[k] * d[k]);
      }
      double x[3];
      const int kept = simp::solve_quadric(Q, mean, tau, x);
      REQUIRE(kept == rank, "rank %d: %d eigenvalues kept", rank, kept);
      const double tol = 64 * EPS;
      for (int k = 0; k < 3; ++k) {
        // on the planes that were given: e_k . x = d_k; along the free directions: the mean's coordinate
        const double want = k < rank ? d[k] : dot(frame[k], mean);
        REQUIRE(std::fabs(dot(frame[k], x) - want) <= tol, "rank %d axis %d: %.3g off", rank, k, dot(frame[k], x) - want);
      }
      if (rank == 0) REQUIRE(x[0] == mean[0] && x[1] == mean[1] && x[2] == mean[2], "a zero quadric must leave the mean");
    }
  }
  // random symmetric positive definite matrices: A = sum of 6 planes, tau = 0 keeps every eigenvalue
  for (int trial = 0; trial < 200; ++trial) {
    double Q[10] = {0};
    for (int k = 0; k < 6; ++k) {
      const double n[3] = {rnd() - 0.5, rnd() - 0.5, rnd() - 0.5};
      add_plane(Q, n, rnd() - 0.5);
    }
    const double mean[3] = {rnd() - 0.5, rnd() - 0.5, rnd() - 0.5};
    double x[3];
    const int kept = simp::solve_quadric(Q, mean, 0.0, x);
    REQUIRE(kept == 3, "SPD: %d eigenvalues kept", kept);
    const double A[3][3] = {{Q[0], Q[1], Q[2]}, {Q[1], Q[3], Q[4]}, {Q[2], Q[4], Q[5]}};
    double res = 0, scale = 0, amax = 0;
    for (int i = 0; i < 3; ++i) {
      res = std::fmax(res, std::fabs(dot(A[i], x) - Q[6 + i]));
      scale = std::fmax(scale, std::fabs(x[i]) + std::fabs(mean[i]));
      for (int j = 0; j < 3; ++j) amax = std::fmax(amax, std::fabs(A[i][j]));
    }
    REQUIRE(res <= 256 * EPS * amax * scale + 64 * EPS, "SPD residual %.3g (|A| %.3g, |x| %.3g)", res, amax, scale);
  }
  // the Jacobi decomposition itself: V diag(w) V^T = A and V^T V = 1
  for (int trial = 0; trial < 200; ++trial) {
    double a[3][3], a0[3][3], w[3], v[3][3];
    for (int i = 0; i < 3; ++i)
      for (int j = i; j < 3; ++j) a[i][j] = a[j][i] = a0[i][j] = a0[j][i] = rnd() - 0.5;
    simp::jacobi3(a, w, v);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double back = 0, gram = 0;
        for (int k = 0; k < 3; ++k) back += v[i][k] * w[k] * v[j][k], gram += v[k][i] * v[k][j];
        REQUIRE(std::fabs(back - a0[i][j]) <= 64 * EPS, "V w V^T (%d,%d): %.3g off", i, j, back - a0[i][j]);
        REQUIRE(std::fabs(gram - (i == j ? 1.0 : 0.0)) <= 64 * EPS, "V^T V (%d,%d): %.3g off", i, j, gram - (i == j));
      }
  }
}

static void check_clamp() {
  const double cell = 0.25;
  const int64_t i[3] = {0, 3, 2097151};
  double lo, hi;
  simp::cell_bounds(3, cell, &lo, &hi);
  REQUIRE(lo == 0.625 && hi == 0.875, "bounds %g %g", lo, hi);
  double x[3] = {0.1, 0.7, 2097151 * cell};
  REQUIRE(!simp::clamp_to_cell(x, i, cell) && x[0] == 0.1 && x[1] == 0.7, "inside: nothing moves");
  double y[3] = {-0.2, 0.9, 2097151 * cell + 1.0};
  REQUIRE(simp::clamp_to_cell(y, i, cell), "outside: moved");
  REQUIRE(y[0] == -0.125 && y[1] == 0.875 && y[2] == 2097151.5 * cell, "clamped to %g %g %g", y[0], y[1], y[2]);
  double e[3] = {-0.125, 0.875, 2097150.5 * cell};
  REQUIRE(!simp::clamp_to_cell(e, i, cell), "the closed cell: its boundary is inside");
  double z[3] = {std::nan(""), 0.7, 2097151 * cell};
  REQUIRE(simp::clamp_to_cell(z, i, cell) && z[0] == -0.125, "a NaN goes to the lower bound");
  // the rounding to fp32 stays inside the cell: a minimum that makes q + min inexact in fp32
  const float mn = 0.1f;
  for (int trial = 0; trial < 2000; ++trial) {
    const int64_t c = trial % 7;
    simp::cell_bounds(c, cell, &lo, &hi);
    const double q = trial % 3 == 0 ? lo : trial % 3 == 1 ? hi : lo + (hi - lo) * rnd();
    const float f = simp::to_f32_in_cell(q, mn, c, cell);
    const double back = (double)f - (double)mn;
    REQUIRE(back >= lo && back <= hi, "fp32 %.9g left the cell [%g, %g]", (double)f, lo, hi);
    REQUIRE(std::fabs((double)f - (q + (double)mn)) <= 1.5 * std::fabs((double)f) * 5.97e-8 + 1e-45, "more than a step away");
  }
  int64_t k[3];
  simp::key_cells(((int64_t)5 << 42) | ((int64_t)2097151 << 21) | 7, k);
  REQUIRE(k[0] == 5 && k[1] == 2097151 && k[2] == 7, "key cells");
}

int main() {
  check_record();
  check_group_sum();
  check_solve();
  check_clamp();
  std::printf("ok %d\n", checks);
  return 0;
}
