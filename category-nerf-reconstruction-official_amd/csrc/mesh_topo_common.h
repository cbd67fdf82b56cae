// Union/find over a pair list for the mesh clean-up unit (csrc/mesh_topo.hip), on top of csrc/ccl_common.h and, like it,
// written once for the device and for a plain host compiler: tests/meshcc_unionfind_main.cpp runs these very functions on
// adversarial pair orders without a GPU.
//
// What is built, and its bounds:
//   find_halving   a find with PATH HALVING: every element met on the way is hung under its grandparent
//                  (fetch_min(L + x, grandparent): parents only ever decrease and a grandparent is an element of the same
//                  set, so the forest stays a min-rooted forest of the same sets whatever other threads do meanwhile).  At
//                  most `bound` steps (bound = the number of elements: a chain is never longer), else *err = 1.
//   unite_halving  both ends to their roots by find_halving, then cnr::ccl::unite on the two roots (whose own finds then
//                  return at once unless another union landed in between; unite carries a lost link on as before).
//   jump           one element's share of a POINTER-JUMPING sweep of the flatten pass: follow up to JUMP parents from L[i]
//                  and hang i under where that ends.  During the flatten pass no union runs, so a root stays a root; a sweep
//                  takes an element of depth d to depth <= ceil(d / (JUMP + 1)) (in place, other elements' jumps only
//                  shorten the way), and sweeps_for(n) = the smallest S with (JUMP + 1)^S >= n sweeps leave every L[i] a
//                  root -- at most 11 for n < 2^31.  A sweep in which every element saw a root ends the pass early.
//   find_parity, unite_parity, jump_parity   the same three on words parent << 1 | parity, for orientation repair (below;
//                  tests/meshorient_unionfind_main.cpp runs them on the host).
// The root of a finished set is its smallest element, so the labels depend on the sets alone: not on the order of the pairs
// and not on scheduling.
#pragma once
#include <stdint.h>

#include "ccl_common.h"

namespace cnr {
namespace ccl {

CNR_CCL_HD inline int find_halving(int* L, int x, int bound, int* err) {
  for (int it = 0; it <= bound; ++it) {
    const int p = load(L + x);
    if (p == x) return x;
    const int g = load(L + p);
    if (g == p) return p;
    fetch_min(L + x, g);
    x = g;
  }
  *err = 1;
  return x;
}

CNR_CCL_HD inline void unite_halving(int* L, int a, int b, int bound, int* err) {
  a = find_halving(L, a, bound, err);
  b = find_halving(L, b, bound, err);
  if (a != b) unite(L, a, b, bound, err);
}

constexpr int JUMP = 7;

// -> true when L[i] is a root afterwards
CNR_CCL_HD inline bool jump(int* L, int i) {
  int x = load(L + i);
  bool root = false;
  for (int k = 0; k <= JUMP; ++k) {
    const int p = load(L + x);
    if (p == x) { root = true; break; }
    if (k < JUMP) x = p;
  }
  fetch_min(L + i, x);
  return root;
}

inline int sweeps_for(int64_t n) {
  int s = 1;
  for (int64_t reach = JUMP + 1; reach < n; reach *= JUMP + 1) ++s;
  return s;
}

// ---- union/find with a parity bit (orientation repair) -------------------------------------------
// One word per element: W[x] = parent << 1 | parity (elements < 2^30), a root is x << 1.  A non-root's word states a
// permanent fact, "x's orientation relative to that ancestor is parity"; in an orientable set all such facts agree, so
// replacing one true word by another is harmless.  The words order as (parent, parity), so fetch_min keeps the smaller
// parent exactly as the plain forest does: the sets and their roots are those of find_halving / unite whatever the parities.
// Two parities meeting for the same (element, parent) can happen only in a set that is not orientable; the minimum keeps
// parity 0 there and the caller's check over all links finds the set out afterwards.
//   find_parity    path halving on words: (p, a), (g, b) -> fetch_min(W + x, (g, a ^ b)).  -> the root, *parity = x's
//                  parity relative to it.  At most `bound` steps, else *err = 1.
//   unite_parity   a and b are linked with rel = orientation(a) ^ orientation(b).  With roots ra, rb and parities pa, pb the
//                  larger root goes under the smaller with q = pa ^ pb ^ rel.  When the minimum meets a word (p', a') that
//                  is no longer a root, one of the two links did not land: (p', smaller root) with rel = a' ^ q is carried on.
//   jump_parity    jump with the parities XOR-ed along the way.
CNR_CCL_HD inline int find_parity(int* W, int x, int bound, int* parity, int* err) {
  int par = 0;
  for (int it = 0; it <= bound; ++it) {
    const int w = load(W + x), p = w >> 1, a = w & 1;
    if (p == x) { *parity = par; return x; }
    const int wp = load(W + p), g = wp >> 1, b = wp & 1;
    if (g == p) { *parity = par ^ a; return p; }
    fetch_min(W + x, (g << 1) | (a ^ b));
    par ^= a ^ b;
    x = g;
  }
  *err = 1;
  *parity = par;
  return x;
}

CNR_CCL_HD inline void unite_parity(int* W, int a, int b, int rel, int bound, int* err) {
  for (int it = 0; it <= bound; ++it) {
    int pa, pb;
    a = find_parity(W, a, bound, &pa, err);
    b = find_parity(W, b, bound, &pb, err);
    if (a == b) return;                        // one set already (pa ^ pb != rel: not orientable, found by the check)
    if (a < b) { const int t = a; a = b; b = t; }
    const int q = pa ^ pb ^ (rel & 1);
    const int old = fetch_min(W + a, (b << 1) | q);
    if (old == (a << 1)) return;
    rel = (old & 1) ^ q;                       // a -> (old >> 1, old & 1) and a -> (b, q): one of them did not land
    a = old >> 1;
  }
  *err = 1;
}

// -> true when W[i]'s parent is a root afterwards
CNR_CCL_HD inline bool jump_parity(int* W, int i) {
  const int w = load(W + i);
  int x = w >> 1, par = w & 1;
  bool root = false;
  for (int k = 0; k <= JUMP; ++k) {
    const int wp = load(W + x), p = wp >> 1;
    if (p == x) { root = true; break; }
    if (k < JUMP) { x = p; par ^= wp & 1; }
  }
  fetch_min(W + i, (x << 1) | par);
  return root;
}

// the undirected edge (a, b) as min << 32 | max; -1 for a == b (a degenerate edge joins nothing and counts nowhere)
CNR_CCL_HD inline int64_t edge_key(int a, int b) {
  if (a == b) return -1;
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  return ((int64_t)lo << 32) | (int64_t)hi;
}

}  // namespace ccl
}  // namespace cnr
