// Stand-alone host program: the union/find helpers of csrc/ccl_common.h, the very functions the labelling kernels call, run
// through the kernels' three phases (tile-local unions, unions across tile borders, flattening) on adversarial masks, with the
// per-thread work visited in forward, reverse and shuffled order, against a flood fill.  Prints "ok <cases>" and exits 0, or
// names the first mismatch and exits 1.  Built and run by tests/test_geoseg_host.py (no GPU, no HIP headers).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

#include "ccl_common.h"

namespace ccl = cnr::ccl;
constexpr int T = ccl::TILE;

static std::vector<int> flood(const std::vector<uint8_t>& m, int H, int W, bool conn8) {
  std::vector<int> lab(H * W, -1), stack;
  for (int p = 0; p < H * W; ++p) {
    if (!m[p] || lab[p] >= 0) continue;          // raster order: p is the smallest index of its component
    lab[p] = p;
    stack.assign(1, p);
    while (!stack.empty()) {
      const int q = stack.back();
      stack.pop_back();
      const int y = q / W, x = q % W;
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          if ((dy == 0 && dx == 0) || (!conn8 && dy != 0 && dx != 0)) continue;
          const int yy = y + dy, xx = x + dx;
          if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
          const int r = yy * W + xx;
          if (m[r] && lab[r] < 0) { lab[r] = p; stack.push_back(r); }
        }
    }
  }
  return lab;
}

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static std::vector<int> order_of(int n, int mode) {
  std::vector<int> o(n);
  std::iota(o.begin(), o.end(), 0);
  if (mode == 1) std::reverse(o.begin(), o.end());
  if (mode == 2) for (int i = n - 1; i > 0; --i) std::swap(o[i], o[rnd() % (i + 1)]);
  return o;
}

// the kernels' phases; `mode` permutes the order in which the "threads" of every phase run
static std::vector<int> label(const std::vector<uint8_t>& m, int H, int W, bool conn8, int mode, int* err) {
  std::vector<int> L(H * W, -1);
  const int tw = (W + T - 1) / T, th = (H + T - 1) / T;
  for (int tile : order_of(tw * th, mode)) {
    const int x0 = (tile % tw) * T, y0 = (tile / tw) * T;
    int lab[T * T];
    for (int t = 0; t < T * T; ++t) {
      const int x = x0 + t % T, y = y0 + t / T;
      lab[t] = (x < W && y < H && m[y * W + x]) ? t : -1;
    }
    for (int t : order_of(T * T, mode)) ccl::tile_unions(lab, t, conn8, err);
    for (int t = 0; t < T * T; ++t) {
      const int x = x0 + t % T, y = y0 + t / T;
      if (x >= W || y >= H || lab[t] < 0) continue;
      const int r = ccl::find(lab, t, T * T, err);
      L[y * W + x] = (y0 + r / T) * W + x0 + r % T;
    }
  }
  for (int p : order_of(H * W, mode)) ccl::border_unions(L.data(), p % W, p / W, H, W, conn8, err);
  for (int p : order_of(H * W, mode))
    if (L[p] >= 0) L[p] = ccl::find(L.data(), p, H * W, err);
  return L;
}

struct Case { const char* name; int H, W; std::vector<uint8_t> m; };

static Case make(const char* name, int H, int W, int kind) {
  Case c{name, H, W, std::vector<uint8_t>(H * W, 0)};
  auto at = [&](int y, int x) -> uint8_t& { return c.m[y * W + x]; };
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) switch (kind) {
        case 0: break;                                                   // zeros
        case 1: at(y, x) = 1; break;                                     // ones
        case 2: at(y, x) = (x + y) % 2 == 0; break;                      // checkerboard
        case 3: at(y, x) = y % 2 == 0 || (y % 4 == 1 && x == W - 1) || (y % 4 == 3 && x == 0); break;   // serpentine
        case 4: at(y, x) = x % 2 == 0 || y == H - 1; break;              // U shapes joined at the bottom row
        case 5: at(y, x) = y == 0 || x == 0 || y == H - 1 || x == W - 1; break;                          // ring on the frame
        case 6: at(y, x) = rnd() % 100 < 50; break;
        case 7: at(y, x) = rnd() % 100 < 62; break;
        case 8: {                                                        // concentric one-pixel rings, opened alternately: a spiral
          const int k = std::min(std::min(x, y), std::min(W - 1 - x, H - 1 - y));
          at(y, x) = k % 2 == 0;
          break;
        }
      }
  if (kind == 8)                                    // join ring k to ring k + 2 through one pixel, alternately left and right
    for (int k = 0; 2 * k + 5 < std::min(H, W); k += 2) {
      const int y = H / 2;
      if ((k / 2) % 2 == 0) at(y, k + 1) = 1; else at(y, W - 2 - k) = 1;
    }
  return c;
}

int main() {
  std::vector<Case> cases;
  const char* names[] = {"zeros", "ones", "checkerboard", "serpentine", "u_shapes", "frame_ring", "random_half", "random_dense", "rings"};
  const int sizes[][2] = {{70, 45}, {1, 131}, {77, 1}, {16, 16}, {17, 33}, {48, 64}};
  for (auto& s : sizes)
    for (int kind = 0; kind < 9; ++kind) cases.push_back(make(names[kind], s[0], s[1], kind));
  int n = 0;
  for (const Case& c : cases)
    for (int conn8 = 0; conn8 < 2; ++conn8) {
      const std::vector<int> want = flood(c.m, c.H, c.W, conn8 != 0);
      for (int mode = 0; mode < 3; ++mode) {
        int err = 0;
        const std::vector<int> got = label(c.m, c.H, c.W, conn8 != 0, mode, &err);
        if (err || got != want) {
          std::printf("MISMATCH %s %dx%d connectivity %d order %d err %d\n", c.name, c.H, c.W, conn8 ? 8 : 4, mode, err);
          return 1;
        }
        ++n;
      }
    }
  std::printf("ok %d\n", n);
  return 0;
}
