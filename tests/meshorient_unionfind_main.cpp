// Stand-alone host program: the union/find with a parity bit of csrc/mesh_topo_common.h (find_parity, unite_parity,
// jump_parity), the very functions the orientation-repair kernels call, on adversarial link orders: a chain of 4097 faces with
// random rel, its links ascending, descending, bit-reversed and shuffled with 3 seeds; the same chain closed to a cycle of even
// total parity (orientable) and of odd total parity (not orientable); a ladder of links with consistent random orientations;
// a star; nothing at all.  After the unions and the flatten sweeps every word must hold root 0 (the set's smallest element)
// and, in an orientable set, the XOR of rel along the chain; the conflict flag -- some link with flip0[f] ^ flip0[g] != rel --
// must be set exactly for the odd cycle; err must stay 0 and sweeps_for(n) sweeps must suffice.  Prints "ok <cases>" and exits
// 0, or names the first mismatch and exits 1.  Built and run by tests/test_meshorient_host.py (no GPU, no HIP headers).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

#include "mesh_topo_common.h"

namespace ccl = cnr::ccl;
struct Link { int f, g, rel; };
using Links = std::vector<Link>;

static uint32_t rng_state = 2463534242u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static void shuffle(std::vector<int>& o) {
  for (int i = (int)o.size() - 1; i > 0; --i) std::swap(o[i], o[rnd() % (i + 1)]);
}

// 0 ascending, 1 descending, 2 bit-reversed, 3.. shuffled (seeded by the mode)
static std::vector<int> order_of(int n, int mode) {
  std::vector<int> o(n);
  std::iota(o.begin(), o.end(), 0);
  if (mode == 1) std::reverse(o.begin(), o.end());
  if (mode == 2) {
    int bits = 0;
    while ((1 << bits) < n) ++bits;
    o.clear();
    for (int i = 0; i < (1 << bits); ++i) {
      int r = 0;
      for (int b = 0; b < bits; ++b) r |= ((i >> b) & 1) << (bits - 1 - b);
      if (r < n) o.push_back(r);
    }
  }
  if (mode >= 3) {
    rng_state = 2463534242u + 7919u * (uint32_t)mode;
    shuffle(o);
  }
  return o;
}

struct Result { std::vector<int> root, parity; bool conflict; int err, sweeps; };

// the kernels' phases on the host: union over the links, flatten sweeps, the check over every link
static Result orient(const Links& links, int n, int mode) {
  Result r;
  r.err = 0;
  std::vector<int> W(n);
  for (int i = 0; i < n; ++i) W[i] = i << 1;
  for (int j : order_of((int)links.size(), mode)) ccl::unite_parity(W.data(), links[j].g, links[j].f, links[j].rel, n, &r.err);
  const int sweeps = n > 0 ? ccl::sweeps_for(n) : 0;
  bool open = n > 0;
  r.sweeps = 0;
  for (int s = 0; s < sweeps && open; ++s) {
    open = false;
    for (int i : order_of(n, mode)) open |= !ccl::jump_parity(W.data(), i);
    ++r.sweeps;
  }
  if (open) r.sweeps = -1;
  r.root.resize(n), r.parity.resize(n);
  for (int i = 0; i < n; ++i) r.root[i] = W[i] >> 1, r.parity[i] = W[i] & 1;
  r.conflict = false;
  for (const Link& l : links) r.conflict |= (r.parity[l.f] ^ r.parity[l.g]) != l.rel;
  // a find after the flatten pass: the root at once, the same parity
  for (int i = 0; i < n; i += std::max(1, n / 17)) {
    int par = -1;
    if (ccl::find_parity(W.data(), i, n, &par, &r.err) != r.root[i] || par != r.parity[i]) r.err |= 4;
  }
  return r;
}

static int cases = 0;
// want_root / want_parity per element (want_parity empty: not orientable, only the roots and the flag are checked)
static bool run(const char* name, const Links& links, int n, const std::vector<int>& want_root, const std::vector<int>& want_parity,
                bool want_conflict) {
  for (int mode = 0; mode < 6; ++mode) {
    const Result r = orient(links, n, mode);
    if (r.err != 0 || r.sweeps < 0) { std::printf("%s mode %d: err %d, sweeps %d\n", name, mode, r.err, r.sweeps); return false; }
    if (r.conflict != want_conflict) { std::printf("%s mode %d: conflict %d\n", name, mode, (int)r.conflict); return false; }
    for (int i = 0; i < n; ++i) {
      if (r.root[i] != want_root[i]) { std::printf("%s mode %d: root[%d] = %d, want %d\n", name, mode, i, r.root[i], want_root[i]); return false; }
      if (!want_parity.empty() && r.parity[i] != want_parity[i]) {
        std::printf("%s mode %d: parity[%d] = %d, want %d\n", name, mode, i, r.parity[i], want_parity[i]);
        return false;
      }
    }
    ++cases;
  }
  return true;
}

int main() {
  bool ok = true;
  for (int n : {2, 3, 65, 4097}) {
    Links chain;
    std::vector<int> root(n, 0), parity(n, 0);
    for (int i = 0; i + 1 < n; ++i) {
      const int rel = (int)(rnd() & 1);
      chain.push_back({i, i + 1, rel});
      parity[i + 1] = parity[i] ^ rel;
    }
    ok = ok && run("chain", chain, n, root, parity, false);
    if (n < 3) continue;
    Links even = chain, odd = chain;
    even.push_back({0, n - 1, parity[n - 1]});                 // closes the cycle consistently
    odd.push_back({0, n - 1, parity[n - 1] ^ 1});              // odd total parity: a Moebius band
    ok = ok && run("even cycle", even, n, root, parity, false) && run("odd cycle", odd, n, root, std::vector<int>(), true);
    // the odd cycle beside an orientable chain on elements of its own: the chain's parities are untouched
    Links both = odd;
    std::vector<int> root2(2 * n, 0);
    for (int i = 0; i + 1 < n; ++i) both.push_back({n + i, n + i + 1, chain[i].rel});
    for (int i = 0; i < n; ++i) root2[n + i] = n;
    for (int mode = 0; mode < 6 && ok; ++mode) {
      const Result r = orient(both, 2 * n, mode);
      ok = r.err == 0 && r.sweeps >= 0 && r.conflict;
      for (int i = 0; i < 2 * n && ok; ++i) ok = r.root[i] == root2[i] && (i < n || r.parity[i] == parity[i - n]);
      if (!ok) std::printf("odd cycle beside a chain %d mode %d\n", n, mode);
      ++cases;
    }
  }
  {
    // a ladder: element i has orientation o[i]; links (i, i + 1) and (i, i + 2) with rel = o ^ o: many cycles, all consistent
    const int n = 2000;
    std::vector<int> o(n), root(n, 0), parity(n);
    for (int i = 0; i < n; ++i) o[i] = (int)(rnd() & 1);
    Links links;
    for (int i = 0; i + 1 < n; ++i) links.push_back({i, i + 1, o[i] ^ o[i + 1]});
    for (int i = 0; i + 2 < n; ++i) links.push_back({i, i + 2, o[i] ^ o[i + 2]});
    for (int i = 0; i < n; ++i) parity[i] = o[i] ^ o[0];
    ok = ok && run("ladder", links, n, root, parity, false);
    // the same with its elements renumbered at random: the root is whichever element got the number 0 ... of its set
    std::vector<int> pi(n);
    std::iota(pi.begin(), pi.end(), 0);
    shuffle(pi);
    Links perm;
    for (const Link& l : links) perm.push_back({std::min(pi[l.f], pi[l.g]), std::max(pi[l.f], pi[l.g]), l.rel});
    std::vector<int> inv(n), pparity(n);
    for (int i = 0; i < n; ++i) inv[pi[i]] = i;
    for (int i = 0; i < n; ++i) pparity[i] = o[inv[i]] ^ o[inv[0]];
    ok = ok && run("ladder permuted", perm, n, root, pparity, false);
  }
  {
    Links star;
    std::vector<int> root(500, 0), parity(500, 0);
    for (int i = 0; i < 499; ++i) {
      const int rel = (int)(rnd() & 1);
      star.push_back({i, 499, rel});
      if (i == 0) parity[499] = rel;
    }
    for (int i = 1; i < 499; ++i) parity[i] = parity[499] ^ star[i].rel;
    ok = ok && run("star", star, 500, root, parity, false);
    std::vector<int> id(7), zero(7, 0);
    std::iota(id.begin(), id.end(), 0);
    ok = ok && run("no links", Links(), 7, id, zero, false);
  }
  if (!ok) return 1;
  std::printf("ok %d\n", cases);
  return 0;
}
