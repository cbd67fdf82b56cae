// Stand-alone host program: the union/find of csrc/mesh_topo_common.h (on csrc/ccl_common.h), the very functions the mesh
// kernels call -- unite_halving over a pair list, then the pointer-jumping sweeps of the flatten pass -- on adversarial pair
// orders: a ladder's pairs ascending, descending, shuffled, and with its element indices permuted; a bare chain (the deepest
// tree the sweep bound has to cope with); a star; nothing at all.  The per-"thread" work of every phase is visited forwards,
// backwards and shuffled.  Every label must be the smallest element of its set (against a breadth-first search), err must stay
// 0 and sweeps_for(n) sweeps must suffice.  Prints "ok <cases>" and exits 0, or names the first mismatch and exits 1.
// Built and run by tests/test_meshops_host.py (no GPU, no HIP headers).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <utility>
#include <vector>

#include "mesh_topo_common.h"

namespace ccl = cnr::ccl;
using Pairs = std::vector<std::pair<int, int>>;

static uint32_t rng_state = 2463534242u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static std::vector<int> order_of(int n, int mode) {
  std::vector<int> o(n);
  std::iota(o.begin(), o.end(), 0);
  if (mode == 1) std::reverse(o.begin(), o.end());
  if (mode == 2) for (int i = n - 1; i > 0; --i) std::swap(o[i], o[rnd() % (i + 1)]);
  return o;
}

static std::vector<int> bfs(const Pairs& pairs, int n) {
  std::vector<std::vector<int>> adj(n);
  for (const auto& p : pairs) { adj[p.first].push_back(p.second); adj[p.second].push_back(p.first); }
  std::vector<int> lab(n, -1), queue;
  for (int s = 0; s < n; ++s) {
    if (lab[s] >= 0) continue;
    lab[s] = s;
    queue.assign(1, s);
    for (size_t h = 0; h < queue.size(); ++h)
      for (int r : adj[queue[h]])
        if (lab[r] < 0) { lab[r] = s; queue.push_back(r); }
  }
  return lab;
}

// the kernels' phases on the host; -> the number of sweeps that did work, -1 when the bound did not suffice
static int label(const Pairs& pairs, int n, int mode, std::vector<int>* out, int* err) {
  std::vector<int> L(n);
  std::iota(L.begin(), L.end(), 0);
  for (int j : order_of((int)pairs.size(), mode)) ccl::unite_halving(L.data(), pairs[j].first, pairs[j].second, n, err);
  const int sweeps = n > 0 ? ccl::sweeps_for(n) : 0;
  int used = 0;
  bool open = n > 0;
  for (int s = 0; s < sweeps && open; ++s) {
    open = false;
    for (int i : order_of(n, mode)) open |= !ccl::jump(L.data(), i);
    ++used;
  }
  *out = L;
  return open ? -1 : used;
}

static Pairs ladder_pairs(int n) {      // the vertex pairs (v0,v1), (v0,v2) of the strip between rails 0..n-1 and n..2n-1
  Pairs p;
  for (int i = 0; i + 1 < n; ++i) {
    p.push_back({i, i + 1}); p.push_back({i, n + i});
    p.push_back({i + 1, n + i + 1}); p.push_back({i + 1, n + i});
  }
  return p;
}

static int cases = 0;
static bool run(const char* name, const Pairs& pairs, int n) {
  const std::vector<int> want = bfs(pairs, n);
  for (int mode = 0; mode < 3; ++mode) {
    std::vector<int> got;
    int err = 0;
    const int sweeps = label(pairs, n, mode, &got, &err);
    if (err != 0 || sweeps < 0) { std::printf("%s mode %d: err %d, sweeps %d\n", name, mode, err, sweeps); return false; }
    for (int i = 0; i < n; ++i)
      if (got[i] != want[i]) { std::printf("%s mode %d: label[%d] = %d, want %d\n", name, mode, i, got[i], want[i]); return false; }
    ++cases;
  }
  return true;
}

// a chain written straight into the label array (no union could build one this deep with halving on): the sweep bound itself
static bool chain_sweeps(int n) {
  for (int mode = 0; mode < 3; ++mode) {
    std::vector<int> L(n);
    for (int i = 0; i < n; ++i) L[i] = i > 0 ? i - 1 : 0;
    const int sweeps = ccl::sweeps_for(n);
    bool open = true;
    for (int s = 0; s < sweeps; ++s) {
      open = false;
      for (int i : order_of(n, mode)) open |= !ccl::jump(L.data(), i);
    }
    for (int i = 0; i < n; ++i)
      if (open || L[i] != 0) { std::printf("chain %d mode %d: L[%d] = %d after %d sweeps\n", n, mode, i, L[i], sweeps); return false; }
    int err = 0;
    if (ccl::find_halving(L.data(), n - 1, n, &err) != 0 || err) { std::printf("chain %d: find_halving\n", n); return false; }
    ++cases;
  }
  return true;
}

int main() {
  bool ok = true;
  for (int n : {2, 3, 64, 1000, 20000}) {
    Pairs asc = ladder_pairs(n), desc = asc, shuf = asc, perm = asc;
    std::reverse(desc.begin(), desc.end());
    for (int i = (int)shuf.size() - 1; i > 0; --i) std::swap(shuf[i], shuf[rnd() % (i + 1)]);
    std::vector<int> pi = order_of(2 * n, 2);
    for (auto& p : perm) p = {pi[p.first], pi[p.second]};
    ok = ok && run("ladder ascending", asc, 2 * n) && run("ladder descending", desc, 2 * n) && run("ladder shuffled", shuf, 2 * n) &&
         run("ladder permuted", perm, 2 * n);
  }
  {
    Pairs star, two, self;
    for (int i = 1; i < 500; ++i) star.push_back({499, i - 1});
    for (int i = 0; i + 2 < 301; ++i) two.push_back({i + 2, i});            // evens and odds apart
    for (int i = 0; i < 10; ++i) self.push_back({i, i});
    ok = ok && run("star", star, 500) && run("two chains", two, 301) && run("self pairs", self, 10) && run("no pairs", Pairs(), 7);
  }
  for (int n : {1, 2, 8, 9, 64, 65, 4096, 4097, 40000}) ok = ok && chain_sweeps(n);
  if (ccl::sweeps_for(1) != 1 || ccl::sweeps_for(8) != 1 || ccl::sweeps_for(9) != 2 || ccl::sweeps_for(0x7fffffff) != 11) {
    std::printf("sweeps_for\n");
    ok = false;
  }
  if (ccl::edge_key(5, 3) != (((int64_t)3 << 32) | 5) || ccl::edge_key(3, 5) != ccl::edge_key(5, 3) || ccl::edge_key(4, 4) != -1) {
    std::printf("edge_key\n");
    ok = false;
  }
  if (!ok) return 1;
  std::printf("ok %d\n", cases);
  return 0;
}
