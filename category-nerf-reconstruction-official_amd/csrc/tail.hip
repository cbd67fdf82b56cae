// The tail of the fused trainer's step in ONE launch: latent backward, AdamW on every parameter, and the step
// epilogue -- three jobs that the stock sequence (cnr_latent_bwd -> cnr_adamw_step -> cnr_step_epilogue) runs as
// dependent launches.  What makes them independent here:
//   * parameters ping-pong like the step state: every kernel of step k READS theta_in and this launch WRITES
//     theta_out (AdamW out of place; exp_avg / exp_avg_sq are touched by AdamW only).  The latent backward reads
//     trunk weights, latent weights and codes while other blocks update exactly those -- out of place, no race;
//   * the thread that produces a latent-path gradient element applies AdamW to it straight away (one producer per
//     element); the trunk entries the latent path adds to are finished by the AdamW blocks themselves
//     (latent_trunk_term: n_obj multiply-adds from dbiasrows and zl);
//   * the epilogue blocks only read the render-loss partials, the depth pool and the CURRENT state.
//   * (records != NULL) the fixed-order reduction of the field backward's records moves in as well: a block sums
//     TAIL_EPB record entries over all workgroups from 16-byte loads -- every load of the block, records included, in ONE
//     round trip (reduce_block) -- and applies AdamW to them at once; the latent path takes its input, the per-object
//     bias-row sums, from a fixed-point table the field backward filled with integer atomics (order-free, hence still
//     bitwise reproducible) instead of waiting for that reduction.
// grid: [ do_latent ? NL latent blocks per class : 0 ] [ NA AdamW blocks over the flat (C, P) buffer, or with records
//        NR = REC_ENTRIES / TAIL_EPB reduce-and-update blocks per class ] [ C epilogue ].
// With do_latent = 0 (the gradient was completed by cnr_latent_bwd, e.g. before a multi-GPU all-reduce) the AdamW
// blocks cover every parameter and nothing else changes.
#include "adamw_common.h"
#include "latent_common.h"
#include "records_common.h"
#include "render_common.h"

namespace {
using namespace cnr;

struct TailArgs {
  const float* theta_in; float* theta_out; float* grad; float* m; float* v;
  FlatLayout lay; int64_t off_B; int C;
  const float* zl; float* dbiasrows; float reg_scale;
  float lr, b1, b2, eps, wd;
  float code_lr, code_wd;   // the code tables' own AdamW group (train.py:40,54-64: code_lr / code_weight_decay); = lr, wd when not given
  const int64_t* state_cur; int64_t* state_next; int64_t add_rows;
  const float* partials; int nb; float* losses; int32_t* flags;
  const float* depth; int64_t pool_rows; const int* perm; int R; float* max_bound;
  int do_latent, NL, NA;
  int local_latent;   // latent blocks in the per-block form of latent_bwd_block_local (more than four objects, rows from the table)
  // optional: the field backward's per-workgroup records (nwg per class) are reduced HERE, and the per-object
  // bias-row sums come from the fixed-point table the field backward accumulated with integer atomics
  const cnr_rec::rec_t* records; int nwg; const long long* rows_fix; int NR;
  // grad_only: stop at the finished gradient (no AdamW, no epilogue blocks): the multi-GPU step all-reduces it first
  int grad_only;
  const int* n_obj_cls;  // optional (C,): objects each class really has (<= lay.n_obj; the rest of its rows are padding)
  int* clamp_flags;  // optional (C,): bits the field backward raised this step (cnr_field_bwd_pipe); or-ed into flags, cleared
};

// (is_code: the element belongs to a shape / texture code table of its class row)
__device__ __forceinline__ bool is_code_off(const cnr::FlatLayout& lay, int64_t q) {
  const int64_t n = (int64_t)lay.n_obj * lay.L;
  return (q >= lay.shape && q < lay.shape + n) || (q >= lay.tex && q < lay.tex + n);
}
__device__ __forceinline__ void adam_one(const TailArgs& a, int64_t e, float g, float step_size, float inv_bc2_sqrt,
                                         bool is_code) {
  float pi = a.theta_in[e] * (1.0f - (is_code ? a.code_lr * a.code_wd : a.lr * a.wd));
  if (is_code) step_size *= a.code_lr / a.lr;
  const float mi = a.m[e] + (g - a.m[e]) * (1.0f - a.b1);
  const float vi = a.v[e] * a.b2 + (1.0f - a.b2) * g * g;
  const float denom = sqrtf(vi) * inv_bc2_sqrt + a.eps;
  pi -= step_size * (mi / denom);
  a.theta_out[e] = pi; a.m[e] = mi; a.v[e] = vi;
}

struct AdamSink {  // latent-path gradient element -> gradient buffer (kept for inspection) + AdamW, same thread
  const TailArgs& a; int64_t row0; float step_size, inv_bc2_sqrt;
  mutable float p0, m0, v0;  // parameter and moments of the element in work, loaded while its gradient is computed
  __device__ __forceinline__ void trunk_add(int, float) const {}
  __device__ __forceinline__ void prefetch(int64_t idx) const {
    if (a.grad_only) return;
    p0 = a.theta_in[row0 + idx]; m0 = a.m[row0 + idx]; v0 = a.v[row0 + idx];
  }
  __device__ __forceinline__ void latent_set(int64_t idx, float g) const {
    const int64_t e = row0 + idx;
    a.grad[e] = g;
    if (a.grad_only) return;
    const bool is_code = is_code_off(a.lay, idx);
    float pi = p0 * (1.0f - (is_code ? a.code_lr * a.code_wd : a.lr * a.wd));
    const float mi = m0 + (g - m0) * (1.0f - a.b1);
    const float vi = v0 * a.b2 + (1.0f - a.b2) * g * g;
    const float denom = sqrtf(vi) * inv_bc2_sqrt + a.eps;
    pi -= (is_code ? step_size * (a.code_lr / a.lr) : step_size) * (mi / denom);
    a.theta_out[e] = pi; a.m[e] = mi; a.v[e] = vi;
  }
};

// this class's (n_obj,4,32) bias-row gradient as floats in LDS, from the fixed-point table
__device__ __forceinline__ void load_rows_fix(const TailArgs& a, int c, float* dst) {
  const int n = a.lay.n_obj * 128;
  // four entries per thread at a time, all 32 table loads in flight together (one entry at a time was one memory round trip
  // per 256 entries: four trips for a class of seven objects)
  for (int i0 = threadIdx.x; i0 < n; i0 += 4 * 256) {
    long long f[4][cnr_rec::ROWS_FIX_COPIES];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + 256 * u;
#pragma unroll
      for (int k = 0; k < cnr_rec::ROWS_FIX_COPIES; ++k) f[u][k] = i < n ? a.rows_fix[((size_t)k * a.C + c) * n + i] : 0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + 256 * u;
      long long t = 0;
#pragma unroll
      for (int k = 0; k < cnr_rec::ROWS_FIX_COPIES; ++k) t += f[u][k];
      if (i < n) dst[i] = (float)((double)t * (1.0 / cnr_rec::ROWS_FIX_SCALE));
    }
  }
  __syncthreads();
}

// ... and straight to the float rows in global memory (no staging: the row count is not bounded by the block's LDS)
__device__ __forceinline__ void publish_rows_fix(const TailArgs& a, int c) {
  const int n = a.lay.n_obj * 128;
  for (int i0 = threadIdx.x; i0 < n; i0 += 4 * 256) {
    long long f[4][cnr_rec::ROWS_FIX_COPIES];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + 256 * u;
#pragma unroll
      for (int k = 0; k < cnr_rec::ROWS_FIX_COPIES; ++k) f[u][k] = i < n ? a.rows_fix[((size_t)k * a.C + c) * n + i] : 0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + 256 * u;
      long long t = 0;
#pragma unroll
      for (int k = 0; k < cnr_rec::ROWS_FIX_COPIES; ++k) t += f[u][k];
      if (i < n) a.dbiasrows[(int64_t)c * n + i] = (float)((double)t * (1.0 / cnr_rec::ROWS_FIX_SCALE));
    }
  }
}

// ---- A reducing block: TAIL_EPB = 64 record entries of class c summed over all nwg records, the latent path's share added, AdamW.
// The sums are record_range_sum's, bit for bit (records_common.h), over the four quarters of the record range, combined
// t0 += t2, t1 += t3, t0 += t1 -- from 16-byte loads, one tile of 64 entries (record_tile_*).  Nothing a block loads has an
// address that depends on a loaded value, so EVERYTHING goes out in one round in front of one scheduling barrier: the table
// entries and z of the latent-path term, theta / m / v of the entries the block finishes, and every record load (at
// nwg <= 256; more records, or more than two objects per chain of the latent-path term, loop behind that round).
// (Blocks of 128 entries -- half the blocks, twice the loads in flight per thread -- measured no faster than two-byte loads:
// CHANGELOG.md, profiles/tail_wide_reduce.txt.)
static_assert(cnr_rec::TAIL_EPB == cnr_rec::TILE, "a reducing block owns one tile");
// blocks with dB entries (record entries [TRUNK, TRUNK + 63); their second addends are the entries 63 further on, which a
// 16-byte load cannot reach from the first addend's lane: these blocks sum the tile behind their own as well and pick
// entry + 63 out of LDS)
constexpr int DB_BLK0 = TRUNK / cnr_rec::TAIL_EPB, DB_BLK1 = (TRUNK + 62) / cnr_rec::TAIL_EPB;
static_assert((DB_BLK1 + 2) * cnr_rec::TILE <= cnr_rec::REC_ENTRIES, "the extra tile lies inside the record");
static_assert(OFF_T1_B + 32 <= DB_BLK0 * cnr_rec::TAIL_EPB, "no latent-conditioned entry in a dB block");
// LDS floats of a reducing block: transposition buffer, quarter sums of two tiles, the latent-path term's four chains
constexpr int TAIL_REDUCE_LDS = cnr_rec::TILE_LDS_FLOATS + 2 * 4 * cnr_rec::TILE + 4 * cnr_rec::TILE;
constexpr int LAT_B = 2;   // objects per chain of the latent-path term in flight at a time

// the record sums of NT tiles from entry i0 on, as acc[tile][quarter][entry of the thread's group] per accumulator slot of the
// thread.  K = 1: a quarter has at most 32 records (nwg <= 128), one load per quarter and tile; K = 2: two, and a loop
// beyond 256 records.  The first round's loads end in front of the scheduling barrier that the caller's loads share.
template <int NT, int K>
__device__ __forceinline__ void reduce_tiles(float (&acc)[NT][4][8], const cnr_rec::rec_t* rc, int i0, int nwg) {
  using namespace cnr_rec;
  const int nk = ((nwg + 3) / 4 + 31) / 32;      // values of k in a quarter
  rec8_t v[NT][4][K];
  record_tile_issue<NT, K>(v, rc, i0, nwg, 0);
  __builtin_amdgcn_sched_barrier(0);             // ---- everything above is in flight together
  record_tile_accumulate<NT, K>(acc, v, nwg, 0);
  for (int k0 = K; k0 < nk; k0 += K) {           // (more than 256 records)
    record_tile_issue<NT, K>(v, rc, i0, nwg, k0);
    __builtin_amdgcn_sched_barrier(0);
    record_tile_accumulate<NT, K>(acc, v, nwg, k0);
  }
}

template <int NT, bool LAT>
__device__ __forceinline__ void reduce_block(const TailArgs& a, int c, int blk, float* sm, float step_size, float inv_bc2_sqrt) {
  using namespace cnr_rec;
  float* tr = sm;                                // [4 * 64][32] swizzled
  float* qs = sm + TILE_LDS_FLOATS;              // [NT * 64][4]: quarter sums of the block's entries (and the tile behind them)
  float* lat = qs + 2 * 4 * TILE;                // [64][4]: the latent-path term's chains
  const int P = (int)a.lay.stride;
  const int le = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int i = blk * TILE + le;
  // The latent path's share of a latent-conditioned layer's weight / bias gradient, sum over objects of d biasrow[ob][k][o] *
  // (z[ob][k][j] | 1), in four chains per entry: thread (le, q) runs chain q (objects q, q + 4, ..) and reads its table entries
  // straight into registers, LAT_B objects at a time.  Every load is unconditional -- from object 0 where the chain has no
  // such object, dropped afterwards: loads under a condition become branches with waits inside.
  int lk = 0, lo_ = 0, lj = 0;
  bool has_lat = false;
  if constexpr (LAT) has_lat = i < TRUNK && latent_trunk_index(i, lk, lo_, lj);
  const int n_obj = a.lay.n_obj, n = n_obj * 128;
  const long long* tabc = a.rows_fix + (size_t)c * n;
  const float* zc = a.zl + (int64_t)c * n;
  long long f[LAT_B][ROWS_FIX_COPIES];
  float zz[LAT_B];
  float lat_part = 0.0f;
  if constexpr (LAT) {
#pragma unroll
    for (int u = 0; u < LAT_B; ++u) {
      const int ob = q + 4 * u, ix = ((ob < n_obj ? ob : 0) * 4 + lk) * 32;
#pragma unroll
      for (int k = 0; k < ROWS_FIX_COPIES; ++k) f[u][k] = tabc[(size_t)k * a.C * n + ix + lo_];
      zz[u] = zc[ix + (lj & 31)];
    }
  }
  // trunk entries and the first dB half own an output; the second dB half is the other addend of the first.  Thread le of the
  // block finishes entry le.
  const bool owner = q == 0 && i < TRUNK + 63;
  const int64_t idx = (int64_t)c * P + (i < TRUNK ? i : a.off_B + (i - TRUNK));
  float p0 = 0.f, m0 = 0.f, v0 = 0.f;
  if (!a.grad_only) {                            // (uniform; a thread that owns nothing loads the class's first element)
    const int64_t ic = owner ? idx : (int64_t)c * P;
    p0 = a.theta_in[ic]; m0 = a.m[ic]; v0 = a.v[ic];
  }
  const rec_t* rc = a.records + (size_t)c * a.nwg * REC_ENTRIES;
  float acc[NT][4][8];
#pragma unroll
  for (int p = 0; p < NT; ++p) {
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[p][qq][j] = 0.0f;
    }
  }
  if (a.nwg <= 4 * 32) reduce_tiles<NT, 1>(acc, rc, blk * TILE, a.nwg);   // (uniform)
  else reduce_tiles<NT, 2>(acc, rc, blk * TILE, a.nwg);
  if constexpr (LAT) {
    for (int b0 = 0;;) {
#pragma unroll
      for (int u = 0; u < LAT_B; ++u) {
        const bool on = has_lat && q + 4 * (b0 + u) < n_obj;
        long long t = 0;
#pragma unroll
        for (int k = 0; k < ROWS_FIX_COPIES; ++k) t += f[u][k];
        const float z = on ? (lj < 32 ? zz[u] : 1.0f) : 0.0f;
        lat_part = fmaf((float)((double)(on ? t : 0) * (1.0 / ROWS_FIX_SCALE)), z, lat_part);
      }
      b0 += LAT_B;
      if (4 * b0 >= n_obj) break;                // (more than 4 LAT_B objects: further rounds)
#pragma unroll
      for (int u = 0; u < LAT_B; ++u) {
        const int ob = q + 4 * (b0 + u), ix = ((ob < n_obj ? ob : 0) * 4 + lk) * 32;
#pragma unroll
        for (int k = 0; k < ROWS_FIX_COPIES; ++k) f[u][k] = tabc[(size_t)k * a.C * n + ix + lo_];
        zz[u] = zc[ix + (lj & 31)];
      }
    }
    lat[le * 4 + q] = lat_part;
  }
#pragma unroll
  for (int p = 0; p < NT; ++p) {
    float t = record_tile_finish(acc[p], tr);    // thread (le, q): quarter q of entry blk * 64 + 64 p + le
    // entries no launch writes sit in uncleared workspace: their sums are dropped here, per entry
    if (!rec_entry_written(blk * TILE + p * TILE + le, n_obj)) t = 0.0f;
    qs[(p * TILE + le) * 4 + q] = t;
  }
  __syncthreads();
  if (owner) {
    auto quarters = [](const float* pp) {        // fixed-order pairwise sum of an entry's four partials
      float t0 = pp[0], t1 = pp[1];
      const float t2 = pp[2], t3 = pp[3];
      t0 += t2; t1 += t3; t0 += t1;
      return t0;
    };
    float g = quarters(qs + le * 4);
    if (i >= TRUNK) g += quarters(qs + (le + 63) * 4);
    if constexpr (LAT) { if (i < TRUNK) g += quarters(lat + le * 4); }   // (+0 for an entry the latent path does not reach)
    a.grad[idx] = g;
    if (!a.grad_only) {
      float pi = p0 * (1.0f - a.lr * a.wd);
      const float mi = m0 + (g - m0) * (1.0f - a.b1);
      const float vi = v0 * a.b2 + (1.0f - a.b2) * g * g;
      const float denom = sqrtf(vi) * inv_bc2_sqrt + a.eps;
      pi -= step_size * (mi / denom);
      a.theta_out[idx] = pi; a.m[idx] = mi; a.v[idx] = vi;
    }
  }
}

#ifdef CNR_TAIL_STAMPS  // tools/exp only
__device__ unsigned long long g_tail_t[8];  // [type 0..2][min start, max end], [6] = min start over all
#define TAIL_T0() const unsigned long long tt0 = __builtin_amdgcn_s_memrealtime(); \
  if (threadIdx.x == 0) atomicMin(&g_tail_t[6], tt0)
#define TAIL_T1(type) do { __syncthreads(); if (threadIdx.x == 0) { atomicMin(&g_tail_t[2 * (type)], tt0); \
  atomicMax(&g_tail_t[2 * (type) + 1], __builtin_amdgcn_s_memrealtime()); } } while (0)
extern "C" int cnr_tail_stamps(unsigned long long* host, int reset) {
  if (reset) {
    unsigned long long init[8] = {~0ull, 0, ~0ull, 0, ~0ull, 0, ~0ull, 0};
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_tail_t), init, sizeof(init));
  }
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_tail_t), sizeof(unsigned long long) * 8);
}
#else
#define TAIL_T0() do {} while (0)
#define TAIL_T1(type) do {} while (0)
#endif

__global__ __launch_bounds__(256) void tail_kernel(TailArgs a) {
  extern __shared__ float sm[];
  TAIL_T0();
  const int C = a.C, P = (int)a.lay.stride;
  const int nlat = a.do_latent ? a.NL * C : 0;
  int b = blockIdx.x;
  float step_size = 0.0f, inv_bc2_sqrt = 0.0f;
  if (!a.grad_only) {
    AdamArgs co{nullptr, nullptr, nullptr, nullptr, 0, a.lr, a.b1, a.b2, a.eps, a.wd, 1.0f};
    adam_coefficients(co, a.state_cur[2] + 1, step_size, inv_bc2_sqrt);
  }
  if (b < nlat) {  // ---- latent backward of class c + AdamW on what it produces
    const int c = b / a.NL, blk = b % a.NL;
    const int n_real = a.n_obj_cls ? a.n_obj_cls[c] : a.lay.n_obj;
    const float reg_c = n_real > 1 ? a.reg_scale : 0.0f;        // src/loss.py:5-15: classes with one object: no regulariser
    AdamSink sink{a, (int64_t)c * P, step_size, inv_bc2_sqrt};
    const float* dbr = a.dbiasrows + (int64_t)c * a.lay.n_obj * 128;
    float* scratch = sm;
    const int64_t nlat_out = (int64_t)4 * 32 * a.lay.L + 128 + (int64_t)2 * a.lay.n_obj * a.lay.L;
    if (a.rows_fix && a.lay.n_obj <= 4 && a.lay.L <= 256 && (int64_t)a.NL * 256 >= nlat_out) {
      // the common case: one element per thread, every load of the block in one round trip
      const int n = a.lay.n_obj * 128;
      latent_bwd_block_1trip(a.theta_in + (int64_t)c * P, a.lay, a.zl + (int64_t)c * n, a.rows_fix + (size_t)c * n,
                             (int64_t)a.C * n, cnr_rec::ROWS_FIX_COPIES, 1.0 / cnr_rec::ROWS_FIX_SCALE,
                             blk == 0 ? a.dbiasrows + (int64_t)c * n : nullptr, reg_c, sm, sink, blk, n_real);
      TAIL_T1(0);
      return;
    }
    if (a.rows_fix && a.local_latent) {
      // more than four objects: every block builds only the d pre entries its own elements read (latent_common.h); the float
      // rows are published by the class's epilogue block
      const int n = a.lay.n_obj * 128;
      latent_bwd_block_local(a.theta_in + (int64_t)c * P, a.lay, a.zl + (int64_t)c * n, a.rows_fix + (size_t)c * n,
                             (int64_t)a.C * n, cnr_rec::ROWS_FIX_COPIES, 1.0 / cnr_rec::ROWS_FIX_SCALE, reg_c, sm, sink, blk,
                             n_real);
      if (a.grad_only && blk == 0 && a.dbiasrows) publish_rows_fix(a, c);   // (no epilogue blocks in the gradient-only launch)
      TAIL_T1(0);
      return;
    }
    if (a.rows_fix) {  // rows from the fixed-point table (block 0 of the class also publishes them as floats)
      float* rows = sm;
      load_rows_fix(a, c, rows);
      if (blk == 0)
        for (int i = threadIdx.x; i < a.lay.n_obj * 128; i += 256) a.dbiasrows[(int64_t)c * a.lay.n_obj * 128 + i] = rows[i];
      dbr = rows;
      scratch = sm + a.lay.n_obj * 128;
    }
    latent_bwd_block(a.theta_in + (int64_t)c * P, a.lay, a.zl + (int64_t)c * a.lay.n_obj * 128, dbr, reg_c,
                     scratch, sink, blk, a.NL, false, n_real);
    TAIL_T1(0);
    return;
  }
  b -= nlat;
  if (a.records) {  // ---- reduce TAIL_EPB record entries of class c over all workgroups, finish the gradient, AdamW
    if (b < a.NR * C) {
      const int c = b / a.NR, blk = b % a.NR;
      // (block-uniform) the blocks that own dB entries also sum the tile behind their own: the second addends sit 63 entries on
      if (blk > DB_BLK1) return;                 // second dB halves and row sums only: no output of its own
      if (blk >= DB_BLK0) reduce_block<2, false>(a, c, blk, sm, step_size, inv_bc2_sqrt);
      else reduce_block<1, true>(a, c, blk, sm, step_size, inv_bc2_sqrt);
      TAIL_T1(1);
      return;
    }
    b -= a.NR * C;
  } else if (b < a.NA) {  // ---- AdamW over the flat buffer; with do_latent only the trunk and B ranges (+ the latent-path term)
    const int64_t n = (int64_t)C * P;
    for (int64_t e = (int64_t)b * 256 + threadIdx.x; e < n; e += (int64_t)a.NA * 256) {
      const int c = (int)(e / P), q = (int)(e - (int64_t)c * P);
      float g = a.grad[e];
      if (a.do_latent) {
        const bool is_trunk = q < CNR_TRUNK_PARAMS, is_B = q >= a.off_B && q < a.off_B + 63;
        if (!is_trunk && !is_B) continue;  // a latent block owns this element
        if (is_trunk) {
          const float t = latent_trunk_term(q, a.zl + (int64_t)c * a.lay.n_obj * 128,
                                            a.dbiasrows + (int64_t)c * a.lay.n_obj * 128, a.lay.n_obj);
          if (t != 0.0f) { g += t; a.grad[e] = g; }
        }
      }
      adam_one(a, e, g, step_size, inv_bc2_sqrt, is_code_off(a.lay, q));
    }
    return;
  } else {
    b -= a.NA;
  }
  // ---- epilogue of class b: loss values + flags, next slice's max depth, next step state (class 0)
  const int c = b, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float* red = sm;
  if (a.local_latent && a.rows_fix && a.dbiasrows)     // the class's bias-row gradient as floats (the latent blocks no longer walk the
    publish_rows_fix(a, c);                            // whole table): table -> registers -> global, any number of objects
  const int64_t cursor = a.state_cur[0] + a.add_rows;
  if (wv == 0) {
    cnr_rl::finish_class(a.partials, a.nb, a.losses, a.flags, C, c, lane);
    if (a.clamp_flags && lane == 0) { a.flags[c] |= a.clamp_flags[c]; a.clamp_flags[c] = 0; }   // same lane wrote flags[c]
  }
  if (a.max_bound) {
    float mx = -INFINITY;
    const int64_t cbase = (int64_t)c * a.pool_rows, base = cbase + cursor;
    // this block is the launch's critical path (cursor -> permutation entry -> depth are dependent loads): eight rays
    // per thread at a time, all permutation entries together, then all depths together = two round trips per 2048 rays
    for (int r0 = 0; r0 < a.R; r0 += 8 * 256) {
      int64_t at[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int r = r0 + u * 256 + threadIdx.x;
        at[u] = r < a.R ? (a.perm ? cbase + a.perm[base + r] : base + r) : -1;
      }
      float d[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) d[u] = at[u] >= 0 ? a.depth[at[u]] : -INFINITY;
#pragma unroll
      for (int u = 0; u < 8; ++u) mx = fmaxf(mx, d[u]);
    }
    mx = wave_max(mx);
    if (lane == 0) red[wv] = mx;
    __syncthreads();
    if (threadIdx.x == 0) a.max_bound[c] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  }
  if (c == 0 && threadIdx.x == 0) {
    a.state_next[0] = cursor; a.state_next[1] = a.state_cur[1] + 1; a.state_next[2] = a.state_cur[2] + 1;
  }
  TAIL_T1(2);
}
}  // namespace

constexpr int LOCAL_MIN_OBJ = 5;   // classes of up to four objects take the one-trip latent blocks (latent_bwd_block_1trip)
// dynamic LDS of a tail block: the reducing blocks' transposition buffer and partial sums (TAIL_REDUCE_LDS floats, 35 KB: two
// blocks per CU as before), the epilogue's 8 floats, the general latent blocks' two whole
// (n_obj, 4, 32) tables + norms, or the per-block form's own rows (latent_local_lds_floats) -- which is what lets a class hold up to
// ROWS_TILE_MAX objects: 100 objects need 29 KB there, where the whole tables would need 103 KB and one block per CU
static size_t tail_lds_bytes(int do_latent, int local_latent, int L, int n_obj, bool reducing) {
  const int general = 2 * n_obj * 128 + 2 * n_obj + 520;
  const int local = latent_local_lds_floats(L, n_obj) + 8;
  int need = !do_latent ? 776 : local_latent ? (local > 776 ? local : 776) : general;
  if (reducing && need < TAIL_REDUCE_LDS) need = TAIL_REDUCE_LDS;
  return (size_t)need * sizeof(float);
}

extern "C" int cnr_step_tail(const cnr_step_tail_args* args, void* stream) {
  if (!args || args->struct_size != sizeof(cnr_step_tail_args) || args->abi_version != CNR_ABI_VERSION) return CNR_E_ARG;
  const float* theta_in = args->theta_in; float* theta_out = args->theta_out; float* grad = args->grad;
  float* exp_avg = args->exp_avg; float* exp_avg_sq = args->exp_avg_sq;
  const int64_t class_stride = args->class_stride, off_B = args->off_B, off_latW = args->off_latW, off_latb = args->off_latb,
                off_shape = args->off_shape, off_tex = args->off_tex, add_rows = args->add_rows, pool_rows = args->pool_rows;
  const int L = args->L, n_obj = args->n_obj, C = args->C, do_latent = args->do_latent, R = args->R, nwg = args->nwg,
            rl_blocks = args->rl_blocks;
  const float* zl = args->zl; float* dbiasrows = args->dbiasrows;
  const float reg_scale = args->reg_scale, lr = args->lr, beta1 = args->beta1, beta2 = args->beta2, eps = args->eps,
              weight_decay = args->weight_decay, code_lr = args->code_lr, code_weight_decay = args->code_weight_decay;
  const int64_t* state_cur = args->state_cur; int64_t* state_next = args->state_next;
  const void* rl_workspace = args->rl_workspace; float* losses = args->losses; int32_t* flags = args->flags;
  const float* depth = args->depth; const int* perm = args->perm; float* next_max_bound = args->next_max_bound;
  const void* records = args->records; const long long* rows_fix = args->rows_fix; int* clamp_flags = args->clamp_flags;
  const int* n_obj_cls = args->n_obj_cls;
  if (!theta_in || !theta_out || theta_in == theta_out || !grad || !exp_avg || !exp_avg_sq || class_stride <= 0 ||
      L <= 0 || n_obj <= 0 || C <= 0 || !state_cur || !state_next || state_cur == state_next || !rl_workspace ||
      !losses || !flags || R <= 0)
    return CNR_E_ARG;
  if (do_latent && (!zl || !dbiasrows)) return CNR_E_ARG;
  // (more than ROWS_MAX object rows: the records carry no row sums, the fixed-point table has them all -- cnr_field_train's
  //  one-object-per-tile form)
  if (records && (!do_latent || !rows_fix || nwg <= 0 || n_obj > cnr_rec::ROWS_TILE_MAX)) return CNR_E_ARG;
  if (records && ((uintptr_t)records & 15)) return CNR_E_ARG;   // the reduction loads 16 bytes at a time
  if (rows_fix && !do_latent) return CNR_E_ARG;
  if (n_obj > cnr_rec::ROWS_TILE_MAX) return CNR_E_SHAPE;
  if (n_obj > 32 && do_latent && !(rows_fix && latent_local_ok(L, n_obj))) return CNR_E_SHAPE;   // the general latent blocks keep whole tables in LDS
  if (next_max_bound && (!depth || pool_rows < R)) return CNR_E_ARG;
  TailArgs a{};
  a.theta_in = theta_in; a.theta_out = theta_out; a.grad = grad; a.m = exp_avg; a.v = exp_avg_sq;
  a.lay = FlatLayout{class_stride, off_latW, off_latb, off_shape, off_tex, L, n_obj};
  a.off_B = off_B; a.C = C; a.zl = zl; a.dbiasrows = dbiasrows; a.reg_scale = reg_scale; a.n_obj_cls = n_obj_cls;
  a.lr = lr; a.b1 = beta1; a.b2 = beta2; a.eps = eps; a.wd = weight_decay;
  a.code_lr = code_lr > 0.0f ? code_lr : lr; a.code_wd = code_lr > 0.0f ? code_weight_decay : weight_decay;
  if (!(lr > 0.0f)) return CNR_E_ARG;
  a.state_cur = state_cur; a.state_next = state_next; a.add_rows = add_rows;
  const int rpb = cnr_rl::rl_rays_per_block(C, R);
  a.partials = (const float*)rl_workspace; a.nb = rl_blocks > 0 ? rl_blocks : (R + rpb - 1) / rpb;
  a.losses = losses; a.flags = flags;
  a.depth = depth; a.pool_rows = pool_rows; a.perm = perm; a.R = R; a.max_bound = next_max_bound;
  a.do_latent = do_latent ? 1 : 0;
  const int64_t nlat_out = (int64_t)4 * 32 * L + 128 + (int64_t)2 * n_obj * L;
  a.NL = (int)((nlat_out + 255) / 256);
  if (a.NL > 256) a.NL = 256;
  a.local_latent = (do_latent && rows_fix && n_obj >= LOCAL_MIN_OBJ && latent_local_ok(L, n_obj)) ? 1 : 0;
  if (a.local_latent) a.NL = latent_local_blocks(L, n_obj);
  const int64_t n = (int64_t)C * class_stride;
  int64_t na = (n + 255) / 256;
  if (na > 2048) na = 2048;
  a.NA = (int)na;
  a.records = (const cnr_rec::rec_t*)records; a.nwg = nwg; a.rows_fix = rows_fix; a.NR = cnr_rec::REC_ENTRIES / cnr_rec::TAIL_EPB;
  a.clamp_flags = clamp_flags;
  const unsigned grid = (unsigned)((a.do_latent ? a.NL * C : 0) + (records ? a.NR * C : a.NA) + C);
  const size_t lds = tail_lds_bytes(a.do_latent, a.local_latent, L, n_obj, records != nullptr);
  hipLaunchKernelGGL(tail_kernel, dim3(grid), dim3(256), lds, (hipStream_t)stream, a);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

// The gradient half of cnr_step_tail on its own, for a host that needs the finished gradient before the optimiser
// (data parallel: all-reduce in between): fixed-order reduction of the field backward's records + latent backward +
// code regulariser, side by side in one launch, into `grad` (class_stride floats per class, the layout of theta).
// Afterwards: all-reduce, then cnr_step_tail(..., do_latent = 0, records = NULL, ...) for AdamW + epilogue.
extern "C" int cnr_step_grad(const float* theta, float* grad, int64_t class_stride, int64_t off_B, int64_t off_latW,
                             int64_t off_latb, int64_t off_shape, int64_t off_tex, int L, int n_obj, int C,
                             const float* zl, float* dbiasrows, float reg_scale, const void* records, int nwg,
                             const long long* rows_fix, const int* n_obj_cls, void* stream) {
  if (!theta || !grad || class_stride <= 0 || L <= 0 || n_obj <= 0 || C <= 0 || !zl || !dbiasrows || !records ||
      nwg <= 0 || !rows_fix)
    return CNR_E_ARG;
  if ((uintptr_t)records & 15) return CNR_E_ARG;   // the reduction loads 16 bytes at a time
  if (n_obj > cnr_rec::ROWS_TILE_MAX) return CNR_E_SHAPE;
  TailArgs a{};
  a.theta_in = theta; a.grad = grad;
  a.lay = FlatLayout{class_stride, off_latW, off_latb, off_shape, off_tex, L, n_obj};
  a.off_B = off_B; a.C = C; a.zl = zl; a.dbiasrows = dbiasrows; a.reg_scale = reg_scale; a.n_obj_cls = n_obj_cls;
  a.do_latent = 1; a.grad_only = 1;
  const int64_t nlat_out = (int64_t)4 * 32 * L + 128 + (int64_t)2 * n_obj * L;
  a.NL = (int)((nlat_out + 255) / 256);
  if (a.NL > 256) a.NL = 256;
  a.local_latent = (n_obj >= LOCAL_MIN_OBJ && latent_local_ok(L, n_obj)) ? 1 : 0;
  if (a.local_latent) a.NL = latent_local_blocks(L, n_obj);
  a.records = (const cnr_rec::rec_t*)records; a.nwg = nwg; a.rows_fix = rows_fix; a.NR = cnr_rec::REC_ENTRIES / cnr_rec::TAIL_EPB;
  const unsigned grid = (unsigned)(a.NL * C + a.NR * C);
  if (n_obj > 32 && !a.local_latent) return CNR_E_SHAPE;
  const size_t lds = tail_lds_bytes(1, a.local_latent, L, n_obj, true);
  hipLaunchKernelGGL(tail_kernel, dim3(grid), dim3(256), lds, (hipStream_t)stream, a);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}
