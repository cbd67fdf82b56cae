// Union/find over a label array for connected-component labelling (csrc/geoseg.hip), written once for the device and for a
// plain host compiler: tests/geoseg_unionfind_main.cpp runs the same functions on adversarial masks without a GPU.
//
// L[x] is the parent of element x, L[x] == x a root; a union always hangs the LARGER root under the smaller one, so parents
// only ever decrease and the root of a finished set is its smallest element -- the result depends on the set alone, not on the
// order in which concurrent unions land.  Nothing here waits for another thread: every loop is bounded by `bound` steps and a
// loop that runs out sets *err to 1 and returns.
#pragma once
#if defined(__HIPCC__)
#define CNR_CCL_HD __host__ __device__
#else
#define CNR_CCL_HD
#endif

namespace cnr {
namespace ccl {

CNR_CCL_HD inline int load(const int* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // never a stale line of another CU's unions
#else
  return *p;
#endif
}

// *p = min(*p, v), returns the value before
CNR_CCL_HD inline int fetch_min(int* p, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicMin(p, v);
#else
  const int old = *p;
  if (v < old) *p = v;
  return old;
#endif
}

CNR_CCL_HD inline int find(const int* L, int x, int bound, int* err) {
  for (int it = 0; it <= bound; ++it) {
    const int p = load(L + x);
    if (p == x) return x;
    x = p;
  }
  *err = 1;
  return x;
}

// joins the sets of a and b.  When the minimum lands on an element that has stopped being a root in the meantime, its old parent
// is carried on and joined in the next round, so no link is lost.
CNR_CCL_HD inline void unite(int* L, int a, int b, int bound, int* err) {
  for (int it = 0; it <= bound; ++it) {
    a = find(L, a, bound, err);
    b = find(L, b, bound, err);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = fetch_min(L + a, b);
    if (old == a) return;
    a = old;
  }
  *err = 1;
}

constexpr int TILE = 16;     // the labelling tile is TILE x TILE pixels, one workgroup

// One tile, one thread `t` = ty * TILE + tx of it (the host program calls this for t = 0..255 in any order): joins the pixel
// with its left / upper (and, with conn8, upper-left / upper-right) neighbours inside the tile.  lab[t] = t or -1 beforehand.
CNR_CCL_HD inline void tile_unions(int* lab, int t, bool conn8, int* err) {
  const int tx = t % TILE, ty = t / TILE, bound = TILE * TILE;
  if (lab[t] < 0) return;
  if (tx > 0 && lab[t - 1] >= 0) unite(lab, t, t - 1, bound, err);
  if (ty > 0 && lab[t - TILE] >= 0) unite(lab, t, t - TILE, bound, err);
  if (conn8 && ty > 0) {
    if (tx > 0 && lab[t - TILE - 1] >= 0) unite(lab, t, t - TILE - 1, bound, err);
    if (tx < TILE - 1 && lab[t - TILE + 1] >= 0) unite(lab, t, t - TILE + 1, bound, err);
  }
}

// Pixel (x, y) of an H x W frame whose labels hold, per masked pixel, an element of its tile's set: joins it with those of its
// left / upper (/ upper-left / upper-right) neighbours that lie in ANOTHER tile.
CNR_CCL_HD inline void border_unions(int* L, int x, int y, int H, int W, bool conn8, int* err) {
  const int p = y * W + x, bound = H * W;
  if (load(L + p) < 0) return;
  const int tx = x % TILE, ty = y % TILE;
  if (tx == 0 && x > 0 && load(L + p - 1) >= 0) unite(L, p, p - 1, bound, err);
  if (ty == 0 && y > 0 && load(L + p - W) >= 0) unite(L, p, p - W, bound, err);
  if (conn8 && y > 0) {
    if ((tx == 0 || ty == 0) && x > 0 && load(L + p - W - 1) >= 0) unite(L, p, p - W - 1, bound, err);
    if ((tx == TILE - 1 || ty == 0) && x < W - 1 && load(L + p - W + 1) >= 0) unite(L, p, p - W + 1, bound, err);
  }
}

}  // namespace ccl
}  // namespace cnr
