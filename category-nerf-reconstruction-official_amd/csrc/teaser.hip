// The two device stages of the TEASER-style global registration (category_registration.TeaserSolver; the
// stages follow Yang, Shi, Carlone, "TEASER: Fast and Certifiable Point Cloud Registration", arXiv 2001.07715):
//   cnr_teaser_graph    the compatibility graph over N correspondences (a_i, b_i): i ~ j iff | |b_i - b_j| - |a_i - a_j| | <= thr,
//                       in fp32 without contraction, as a symmetric bitset (N rows of ceil(N / 64) 64-bit words) plus degrees.
//   cnr_clique_search   the exact maximum clique of such a bitset graph: vertices relabelled by `order` (the caller's fixed
//                       order, ascending degree), one wave per root vertex whose candidates are its LATER neighbours, the
//                       candidate set a bitset spread over the lanes that shrinks by an AND with an adjacency row per step,
//                       pruned by |R| + |P| <= best.
// Determinism: integers only, no float atomics.  The size pass shares `best` through integer atomics; its VALUE at the end
// does not depend on timing when no root ran out of budget.  The clique that is returned is then rebuilt by a second pass whose
// pruning depends on that size alone: the lowest root that holds a clique of that size (integer atomic max of N - root), and a
// last launch of one wave that repeats that root's depth-first search and writes the first clique it meets.  Candidates are
// taken in ascending order, so that clique is the lexicographically smallest maximum clique in the relabelled order.
// Every loop is bounded: a root spends at most `budget` row ANDs, then gives up and says so (info_out); if the size pass
// was cut short the size is a lower bound, and if the second pass cannot re-find it in its budget the greedy clique of the
// first pass (deterministic) is returned.  Either way exact = 0.
#include "cnr_common.h"
#include "geom_common.h"

#include <limits.h>

using cnr::align256;

namespace {
constexpr int TG_BLOCK = 256;                 // 4 waves
constexpr int TG_WAVES = TG_BLOCK / 64;
constexpr int CLIQUE_MAX_N = CNR_TEASER_MAX_N;
constexpr int CLIQUE_MAX_BLOCKS = 1280;       // 5 workgroups per CU at <= 32 KB of LDS each

// ---- the graph ---------------------------------------------------------------------------------------------------------
// One workgroup per row i; its waves stride over the row's words, lane l of word w tests j = 64 w + l.
__global__ __launch_bounds__(TG_BLOCK) void graph_kernel(const float* __restrict__ A, const float* __restrict__ B, int N, int W,
                                                         float thr, uint64_t* __restrict__ adj, int* __restrict__ deg) {
#pragma clang fp contract(off)
  __shared__ int s_deg[TG_WAVES];
  const int i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float ax = A[3 * (int64_t)i], ay = A[3 * (int64_t)i + 1], az = A[3 * (int64_t)i + 2];
  const float bx = B[3 * (int64_t)i], by = B[3 * (int64_t)i + 1], bz = B[3 * (int64_t)i + 2];
  int cnt = 0;
  for (int w = wave; w < W; w += TG_WAVES) {
    const int j = w * 64 + lane;
    bool e = false;
    if (j < N && j != i) {
      const float dax = ax - A[3 * (int64_t)j], day = ay - A[3 * (int64_t)j + 1], daz = az - A[3 * (int64_t)j + 2];
      const float dbx = bx - B[3 * (int64_t)j], dby = by - B[3 * (int64_t)j + 1], dbz = bz - B[3 * (int64_t)j + 2];
      const float na = sqrtf((dax * dax + day * day) + daz * daz);       // correctly rounded, no fused multiply-add
      const float nb = sqrtf((dbx * dbx + dby * dby) + dbz * dbz);
      e = fabsf(nb - na) <= thr;
    }
    const uint64_t m = __ballot(e);
    if (lane == 0) adj[(int64_t)i * W + w] = m;
    cnt += __popcll(m);
  }
  if (lane == 0) s_deg[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int k = 0; k < TG_WAVES; ++k) s += s_deg[k];
    deg[i] = s;
  }
}

// out[i'][j'] = adj[order[i']][order[j']]; bits at and beyond N are zero; an entry of `order` outside [0, N) reads as no edge
__global__ __launch_bounds__(TG_BLOCK) void permute_kernel(const uint64_t* __restrict__ adj, const int* __restrict__ order, int N,
                                                           int W, uint64_t* __restrict__ out) {
  const int i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = order[i];
  const bool row_ok = (unsigned)r < (unsigned)N;
  for (int w = wave; w < W; w += TG_WAVES) {
    const int j = w * 64 + lane;
    bool e = false;
    if (row_ok && j < N && j != i) {
      const int c = order[j];
      if ((unsigned)c < (unsigned)N) e = (adj[(int64_t)r * W + (c >> 6)] >> (c & 63)) & 1ull;
    }
    const uint64_t m = __ballot(e);
    if (lane == 0) out[(int64_t)i * W + w] = m;
  }
}

// ---- the search --------------------------------------------------------------------------------------------------------
struct Ctl {                       // zeroed by the host wrapper before the first launch
  int best;                        // the largest clique any wave has built (greedy pass, then the size pass)
  int greedy_best;                 // ... by the greedy pass alone
  int find_key;                    // find pass: N - (lowest root that holds a clique of size best); 0 = none
  int find_oob_key;                // find pass: N - (lowest root that ran out of budget); 0 = none
  int size_oob;                    // size pass: roots that ran out of budget
  int overflow;                    // a root met more candidates than max_degree allows
  int max_steps;                   // size pass: the most steps one root took
  int pad;
  unsigned long long steps_size, steps_find;
};

enum { MODE_SIZE = 0, MODE_FIND = 1, MODE_EMIT = 2 };
enum { ST_DONE = 0, ST_FOUND = 1, ST_BUDGET = 2, ST_ABORT = 3, ST_OVERFLOW = 4 };

template <int WPL> struct Levels { static constexpr int KL = WPL == 4 ? 4 : 8; };   // candidate sets kept in LDS: <= 32 KB per workgroup

// one relaxed load of a shared word, the same value in every lane by construction (it steers wave-uniform branches)
__device__ __forceinline__ int load_uniform(const int* p) {
  return __builtin_amdgcn_readfirstlane(__atomic_load_n(p, __ATOMIC_RELAXED));
}
__device__ __forceinline__ int wave_sum_int(int v) {
  const int lane = (int)(threadIdx.x & 63);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __builtin_bit_cast(int, cnr::xor_lane(__builtin_bit_cast(float, v), o, lane));
  return v;
}
// the bits of word w whose vertex index is above v / below N
__device__ __forceinline__ uint64_t above_mask(int w, int v) {
  const int d = v - 64 * w;                    // the bit of v in this word
  return d < 0 ? ~0ull : (d >= 63 ? 0ull : (~0ull << (d + 1)));
}
__device__ __forceinline__ uint64_t below_mask(int w, int N) {
  const int d = N - 64 * w;                    // the bits of this word that are vertices
  return d >= 64 ? ~0ull : (d <= 0 ? 0ull : ((1ull << d) - 1ull));
}

template <int WPL> struct Set {
  uint64_t x[WPL];                             // word lane + 64 k of the N-bit set
  __device__ __forceinline__ void load_row(const uint64_t* __restrict__ adj, int W, int u, int lane) {
#pragma unroll
    for (int k = 0; k < WPL; ++k) x[k] = lane + 64 * k < W ? adj[(int64_t)u * W + lane + 64 * k] : 0ull;
  }
  __device__ __forceinline__ void and_row(const uint64_t* __restrict__ adj, int W, int u, int lane) {
#pragma unroll
    for (int k = 0; k < WPL; ++k) x[k] &= lane + 64 * k < W ? adj[(int64_t)u * W + lane + 64 * k] : 0ull;
  }
  __device__ __forceinline__ void keep_above(int v, int lane) {
#pragma unroll
    for (int k = 0; k < WPL; ++k) x[k] &= above_mask(lane + 64 * k, v);
  }
  __device__ __forceinline__ void keep_below(int N, int lane) {
#pragma unroll
    for (int k = 0; k < WPL; ++k) x[k] &= below_mask(lane + 64 * k, N);
  }
  __device__ __forceinline__ void clear(int u, int lane) {
#pragma unroll
    for (int k = 0; k < WPL; ++k)
      if ((u >> 6) == lane + 64 * k) x[k] &= ~(1ull << (u & 63));
  }
  __device__ __forceinline__ int count() const {
    int c = 0;
#pragma unroll
    for (int k = 0; k < WPL; ++k) c += __popcll(x[k]);
    return wave_sum_int(c);
  }
  // the lowest member, or -1 (the same value in every lane)
  __device__ __forceinline__ int lowest() const {
    int u = -1;
#pragma unroll
    for (int k = 0; k < WPL; ++k) {
      if (u < 0) {
        const uint64_t m = __ballot(x[k] != 0ull);
        if (m) {
          const int src = __ffsll((unsigned long long)m) - 1;
          const unsigned long long word = __shfl((unsigned long long)x[k], src, 64);
          u = (src + 64 * k) * 64 + __ffsll(word) - 1;
        }
      }
    }
    return u;
  }
  __device__ __forceinline__ void store(uint64_t* s, int lane) const {
#pragma unroll
    for (int k = 0; k < WPL; ++k) s[64 * k + lane] = x[k];
  }
  __device__ __forceinline__ void load(const uint64_t* s, int lane) {
#pragma unroll
    for (int k = 0; k < WPL; ++k) x[k] = s[64 * k + lane];
  }
};

// The depth-first search below root v (R = {v}, candidates = v's later neighbours, taken in ascending order).
//   MODE_SIZE  prune |R| + |P| <= ctl->best, raise ctl->best with every larger clique, run to exhaustion.
//   MODE_FIND  prune |R| + |P| < target, stop at the first clique of size target; give way once a lower root holds one.
//   MODE_EMIT  as MODE_FIND without giving way.
// stack: this wave's KL candidate sets in LDS (the untried candidates of levels 1..KL); deeper levels are rebuilt from level KL
// and the rows of rstack.  rstack (cap): the vertices of R.  *steps: row ANDs spent (at most budget + cap).
template <int WPL, int MODE>
__device__ int dfs_root(const uint64_t* __restrict__ adj, int N, int W, int v, int target, int budget, int cap, uint64_t* stack,
                        int* rstack, Ctl* ctl, int* steps_out) {
  constexpr int KL = Levels<WPL>::KL;
  constexpr int SLOT = 64 * WPL;
  const int lane = threadIdx.x & 63;
  Set<WPL> cur;
  cur.load_row(adj, W, v, lane);
  cur.keep_above(v, lane);
  cur.keep_below(N, lane);
  if (lane == 0) rstack[0] = v;
  int l = 1, steps = 0, status = ST_DONE;
  if (MODE != MODE_SIZE && target <= 1) {
    *steps_out = 0;
    return ST_FOUND;
  }
  // every turn either spends a step or lowers l, and l rises only with a step: at most 2 (budget + cap) + 1 turns
  for (;;) {
    const int cnt = cur.count();
    bool prune;
    int b = 0;
    if (MODE == MODE_SIZE) {
      b = load_uniform(&ctl->best);
      prune = l + cnt <= b;
    } else {
      prune = l + cnt < target;
      if (MODE == MODE_FIND && load_uniform(&ctl->find_key) > N - v) {
        status = ST_ABORT;
        break;
      }
    }
    if (cnt == 0 || prune) {
      l -= 1;
      if (l == 0) break;
      if (l <= KL) {
        cur.load(stack + (l - 1) * SLOT, lane);
      } else {
        cur.load(stack + (KL - 1) * SLOT, lane);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");      // lane 0's stores to rstack, read by every lane
        for (int t = KL; t < l; ++t) cur.and_row(adj, W, load_uniform(rstack + t), lane);
        cur.keep_above(load_uniform(rstack + l), lane);
        steps += l - KL;
      }
    } else {
      const int u = cur.lowest();
      cur.clear(u, lane);
      if (l <= KL) cur.store(stack + (l - 1) * SLOT, lane);
      if (l >= cap) {
        status = ST_OVERFLOW;
        break;
      }
      if (lane == 0) rstack[l] = u;
      cur.and_row(adj, W, u, lane);
      l += 1;
      steps += 1;
      if (MODE == MODE_SIZE) {
        if (l > b && lane == 0) atomicMax(&ctl->best, l);
      } else if (l == target) {
        status = ST_FOUND;
        break;
      }
    }
    if (steps >= budget) {
      status = ST_BUDGET;
      break;
    }
  }
  *steps_out = steps;
  return status;
}

// greedy: always the lowest candidate -> the clique's size; with out != NULL its vertices in the caller's labels
template <int WPL>
__device__ int greedy_root(const uint64_t* __restrict__ adj, int N, int W, int v, int cap, const int* __restrict__ order, int* out) {
  const int lane = threadIdx.x & 63;
  Set<WPL> cur;
  cur.load_row(adj, W, v, lane);
  cur.keep_above(v, lane);
  cur.keep_below(N, lane);
  if (out && lane == 0) out[0] = order[v];
  int l = 1;
  while (l < cap) {
    const int u = cur.lowest();
    if (u < 0) break;
    cur.clear(u, lane);
    cur.and_row(adj, W, u, lane);
    if (out && lane == 0) out[l] = order[u];
    l += 1;
  }
  return l;
}

template <int WPL>
__global__ __launch_bounds__(TG_BLOCK) void greedy_kernel(const uint64_t* __restrict__ adj, int N, int W, int cap,
                                                          int* __restrict__ gsize, Ctl* ctl) {
  const int lane = threadIdx.x & 63, gw = blockIdx.x * TG_WAVES + (threadIdx.x >> 6), nw = gridDim.x * TG_WAVES;
  int mine = 0;
  for (int v = gw; v < N; v += nw) {
    const int l = greedy_root<WPL>(adj, N, W, v, cap, nullptr, nullptr);
    if (lane == 0) gsize[v] = l;
    mine = max(mine, l);
  }
  if (lane == 0 && mine > 0) {
    atomicMax(&ctl->best, mine);
    atomicMax(&ctl->greedy_best, mine);
  }
}

template <int WPL, int MODE>
__global__ __launch_bounds__(TG_BLOCK) void search_kernel(const uint64_t* __restrict__ adj, int N, int W, int budget, int cap,
                                                          int* __restrict__ rstacks, Ctl* ctl) {
  __shared__ uint64_t s_stack[TG_WAVES][Levels<WPL>::KL * 64 * WPL];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gw = blockIdx.x * TG_WAVES + wave, nw = gridDim.x * TG_WAVES;
  int* rstack = rstacks + (int64_t)gw * cap;
  // the size is settled between the launches: the find pass reads what the size pass left
  const int target = MODE == MODE_SIZE ? 0 : load_uniform(&ctl->best);
  unsigned long long total = 0;
  int most = 0;
  for (int v = gw; v < N; v += nw) {
    int steps = 0;
    const int st = dfs_root<WPL, MODE>(adj, N, W, v, target, budget, cap, s_stack[wave], rstack, ctl, &steps);
    total += (unsigned long long)steps;
    most = max(most, steps);
    if (lane == 0) {
      if (st == ST_OVERFLOW) atomicMax(&ctl->overflow, 1);
      if (MODE == MODE_SIZE && st == ST_BUDGET) atomicAdd(&ctl->size_oob, 1);
      if (MODE == MODE_FIND && st == ST_BUDGET) atomicMax(&ctl->find_oob_key, N - v);
      if (MODE == MODE_FIND && st == ST_FOUND) atomicMax(&ctl->find_key, N - v);
    }
  }
  if (lane == 0) {
    atomicAdd(MODE == MODE_SIZE ? &ctl->steps_size : &ctl->steps_find, total);
    if (MODE == MODE_SIZE) atomicMax(&ctl->max_steps, most);
  }
}

// one wave: the clique of the lowest root found, or the greedy clique, in the caller's labels; info_out (8)
template <int WPL>
__global__ __launch_bounds__(64) void emit_kernel(const uint64_t* __restrict__ adj, const int* __restrict__ order, int N, int W,
                                                  int budget, int cap, const int* __restrict__ gsize, int* __restrict__ rstacks,
                                                  Ctl* ctl, int* __restrict__ clique_out, int64_t* __restrict__ info_out) {
  __shared__ uint64_t s_stack[Levels<WPL>::KL * 64 * WPL];
  const int lane = threadIdx.x & 63;
  const int target = load_uniform(&ctl->best), key = load_uniform(&ctl->find_key);
  int size = 0, exact = 0, fallback = 0;
  if (key > 0) {
    int steps = 0;
    const int st = dfs_root<WPL, MODE_EMIT>(adj, N, W, N - key, target, budget, cap, s_stack, rstacks, ctl, &steps);
    if (st == ST_FOUND) {
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      for (int t = lane; t < target; t += 64) clique_out[t] = order[rstacks[t]];
      size = target;
      exact = ctl->size_oob == 0 && ctl->overflow == 0 && !(ctl->find_oob_key > key);
    }
  }
  if (size == 0) {                             // the greedy pass's clique: the lowest root that reached greedy_best
    fallback = 1;
    const int g = load_uniform(&ctl->greedy_best);
    int root = -1;
    for (int base = 0; base < N && root < 0; base += 64) {
      const uint64_t m = __ballot(base + lane < N && gsize[base + lane] == g);
      if (m) root = base + __ffsll((unsigned long long)m) - 1;
    }
    if (root >= 0) size = greedy_root<WPL>(adj, N, W, root, cap, order, clique_out);
  }
  if (lane == 0) {
    info_out[0] = size;
    info_out[1] = exact;
    info_out[2] = (int64_t)ctl->steps_size;
    info_out[3] = (int64_t)ctl->steps_find;
    info_out[4] = ctl->max_steps;
    info_out[5] = ctl->size_oob;
    info_out[6] = ctl->greedy_best;
    info_out[7] = (ctl->overflow ? 1 : 0) | (fallback ? 2 : 0);
  }
}

struct CliqueLayout {
  int W, cap, blocks;
  int64_t off_gsize, off_adj, off_rstack, bytes;
};
inline int clique_layout(int N, int max_degree, CliqueLayout* L) {
  if (N < 1 || N > CLIQUE_MAX_N || max_degree < 0 || max_degree >= N) return CNR_E_SHAPE;
  L->W = (N + 63) / 64;
  L->cap = max_degree + 1;
  L->blocks = (N + TG_WAVES - 1) / TG_WAVES;
  if (L->blocks > CLIQUE_MAX_BLOCKS) L->blocks = CLIQUE_MAX_BLOCKS;
  L->off_gsize = align256((int64_t)sizeof(Ctl));
  L->off_adj = L->off_gsize + align256((int64_t)N * 4);
  L->off_rstack = L->off_adj + align256((int64_t)N * L->W * 8);
  L->bytes = L->off_rstack + align256((int64_t)L->blocks * TG_WAVES * L->cap * 4);
  return CNR_OK;
}

template <int WPL>
int clique_launch(const uint64_t* adj, const int* order, int N, int budget, const CliqueLayout& L, char* ws, int* clique_out,
                  int64_t* info_out, hipStream_t s) {
  Ctl* ctl = (Ctl*)ws;
  int* gsize = (int*)(ws + L.off_gsize);
  uint64_t* padj = (uint64_t*)(ws + L.off_adj);
  int* rstacks = (int*)(ws + L.off_rstack);
  hipError_t e = hipMemsetAsync(ws, 0, (size_t)L.off_gsize, s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(permute_kernel, dim3((unsigned)N), dim3(TG_BLOCK), 0, s, adj, order, N, L.W, padj);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(greedy_kernel<WPL>, dim3((unsigned)L.blocks), dim3(TG_BLOCK), 0, s, (const uint64_t*)padj, N, L.W, L.cap, gsize,
                     ctl);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL((search_kernel<WPL, MODE_SIZE>), dim3((unsigned)L.blocks), dim3(TG_BLOCK), 0, s, (const uint64_t*)padj, N, L.W,
                     budget, L.cap, rstacks, ctl);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL((search_kernel<WPL, MODE_FIND>), dim3((unsigned)L.blocks), dim3(TG_BLOCK), 0, s, (const uint64_t*)padj, N, L.W,
                     budget, L.cap, rstacks, ctl);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(emit_kernel<WPL>, dim3(1), dim3(64), 0, s, (const uint64_t*)padj, order, N, L.W, budget, L.cap,
                     (const int*)gsize, rstacks, ctl, clique_out, info_out);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}
}  // namespace

extern "C" int cnr_teaser_graph(const float* A, const float* B, int N, float threshold, uint64_t* adj, int* deg, void* stream) {
  if (!A || !B || !adj || !deg) return CNR_E_ARG;
  if (N < 1 || N > CLIQUE_MAX_N || !(threshold >= 0.0f)) return CNR_E_SHAPE;
  hipLaunchKernelGGL(graph_kernel, dim3((unsigned)N), dim3(TG_BLOCK), 0, (hipStream_t)stream, A, B, N, (N + 63) / 64, threshold, adj,
                     deg);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int64_t cnr_clique_workspace_bytes(int N, int max_degree) {
  CliqueLayout L;
  if (clique_layout(N, max_degree, &L) != CNR_OK) return CNR_E_SHAPE;
  return L.bytes;
}

extern "C" int cnr_clique_search(const uint64_t* adj, const int* order, int N, int max_degree, int budget, void* workspace,
                                 int* clique_out, int64_t* info_out, void* stream) {
  if (!adj || !order || !workspace || !clique_out || !info_out) return CNR_E_ARG;
  CliqueLayout L;
  if (clique_layout(N, max_degree, &L) != CNR_OK || budget < 1) return CNR_E_SHAPE;
  char* ws = (char*)workspace;
  if (L.W <= 64) return clique_launch<1>(adj, order, N, budget, L, ws, clique_out, info_out, (hipStream_t)stream);
  if (L.W <= 128) return clique_launch<2>(adj, order, N, budget, L, ws, clique_out, info_out, (hipStream_t)stream);
  return clique_launch<4>(adj, order, N, budget, L, ws, clique_out, info_out, (hipStream_t)stream);
}
