// Per-workgroup record format of the fused field backward and its fixed-order reduction, shared by the backward
// translation units (fused_bwd_common.h) and tail.hip.
#pragma once
#include "cnr_common.h"

namespace cnr_rec {
using namespace cnr;
// rows_per_class <= 15: per-object bias-row sums travel in the record / the fixed-point table (the 8-wave kernel's
// row-sum blocks have 32 rows each: one block of 4 latent slots x <= 7 objects + 2 bias rows, or two blocks of
// 2 latent slots x <= 15 objects, the first with the 2 bias rows)
constexpr int ROWS_MAX = 15;
// rows_per_class <= 128 on the one-launch path with one object per tile (fused_bwd_pipe8.hip, WIDE = 3): the sums go to the
// fixed-point table only, the record carries none.  (The reference caps a scene at n_models = 100 categories + instances,
// configs/Replica/config_replica_room0.json:15; nothing in the kernels depends on the count any more -- the tail launch's latent
// blocks read only the rows they need, latent_common.h.)
constexpr int ROWS_TILE_MAX = 128;
constexpr int REC_ENTRIES = ((TRUNK + 126 + ROWS_MAX * 128 + 255) / 256) * 256;  // one workgroup's record
// A record entry is a bf16 (round 4; fp32 before): 256 records x 64.5 KB written by the field kernel and read once by the step's
// last launch were 15 of the 21 MB the step body moves at configs[1].  Each workgroup's partial sum is rounded once (half an ulp
// at most: 2^-9 relative to the PARTIAL, unbiased); the fixed-order sum over the records stays fp32.  The summed gradient therefore
// carries rounding noise of 2^-9 / sqrt(records) relative to the partials, records per class = 256 / C: ~1e-4 .. 2e-4 at the 256
// records of configs[1] (measured 2.0e-4 on the trunk) -- under the f16 forward's own, tests/test_fullsize_gpu.py bars unchanged --
// but 5e-4 .. 1.4e-3 at the 10 .. 63 records of many classes per GPU and of the small test shapes.  An entry whose partials CANCEL
// keeps an absolute error of 2^-9 |partial| per record, whatever the sum: with random upstream gradients 256 records leave 2e-3
// (tests/test_fused_gpu.py, linearity).  The noise is predictable entry by entry from the records themselves (sum of ulp^2 / 12);
// tests/record_noise.py turns that into the checks of the gradient-equivalence tests.  bf16, not f16: a workgroup's share of a small
// gradient entry sits far below f16's 6e-8.  The per-object bias-row sums of the step go through the int64 fixed-point table as
// before (exact).
typedef unsigned short rec_t;
__device__ __forceinline__ rec_t rec_pack(float v) { return __builtin_bit_cast(unsigned short, (__bf16)v); }   // v_cvt_pk_bf16_f32: RNE
__device__ __forceinline__ float rec_unpack(rec_t b) { return __builtin_bit_cast(float, (unsigned int)b << 16); }
constexpr double ROWS_FIX_SCALE = 1099511627776.0;  // 2^40: bias-row sums as int64 fixed point (order-free atomics)
constexpr int TAIL_EPB = 64;  // record entries per reducing block of the tail launch = one tile of record_tile_* below (128, and 32 / 16 with two-byte loads, measured slower)
constexpr int ROWS_FIX_COPIES = 8;  // the table is replicated: a workgroup adds into copy (its index & 7), which
                                    // cuts the same-address atomic queue 8-fold; consumers add the copies (exact)

// Entries no launch writes (latent-layer biases, padding, unused row sums) are skipped, so the workspace needs no
// clearing.
__device__ __forceinline__ bool rec_entry_written(int i, int rows_per_class) {
  if (i < TRUNK)
    return !((i >= OFF_S1_B && i < OFF_S1_B + 32) || (i >= OFF_CAT_B && i < OFF_CAT_B + 32) ||
             (i >= OFF_S2_B && i < OFF_S2_B + 32) || (i >= OFF_T1_B && i < OFF_T1_B + 32));
  if (i < TRUNK + 126) return true;
  return rows_per_class <= ROWS_MAX && (i - (TRUNK + 126)) < rows_per_class * 128;
}
// sum of entry i over records [w0, w1) of one class (r = that class's first record + i).  32 loads in flight per
// thread: the reducing kernels run a few waves per CU, so the loads in flight per thread are what hides the memory
// latency (8 in flight: 64 records = 8 round trips = 8 us; 32: 2 round trips).  Fixed order -> reproducible bits.
// The ORDER this routine defines is the contract of every record reduction: accumulators a[0..31] from +0, a[u] += record
// (w0 + u + 32 k) for k = 0, 1, .. (records past w1 add +0), then a[u] += a[u + st] for st = 16, 8, 4, 2, 1.  It is the form
// of the stand-alone backward (reduce_records_kernel: one entry per thread, two-byte loads); the step's last launch computes
// the same sums from 16-byte loads with record_tile_* below.
__device__ __forceinline__ float record_range_sum(const rec_t* __restrict__ r, int w0, int w1) {
  constexpr int U = 32;
  float a[U];
#pragma unroll
  for (int u = 0; u < U; ++u) a[u] = 0.0f;
  int w = w0;
  // (loads into their own registers, a scheduling barrier, then the adds: written as a[u] += r[..] the compiler is free to
  //  serialise load -> wait -> add per record, and without the SLP vectoriser it does: 19 instead of 5 us per reduction)
  for (; w + U - 1 < w1; w += U) {
    rec_t v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = r[(size_t)(w + u) * REC_ENTRIES];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u) a[u] += rec_unpack(v[u]);
  }
  {
    rec_t v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = (w + u < w1) ? r[(size_t)(w + u) * REC_ENTRIES] : (rec_t)0;   // the rest (< U records), issued together
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u) a[u] += rec_unpack(v[u]);
  }
#pragma unroll
  for (int st = U / 2; st >= 1; st >>= 1) {
#pragma unroll
    for (int u = 0; u < st; ++u) a[u] += a[u + st];
  }
  return a[0];
}

// ---- The same sums from 16-byte loads, for a block of 256 threads and TILES tiles of 64 consecutive entries.
// Thread (g = tid & 7, u = tid >> 3) loads the 8 entries [8 g, 8 g + 8) of a tile from the records that land in accumulator
// slot u: of quarter q (records [q per, min(nwg, q per + per)), per = ceil(nwg / 4) -- the four sub-ranges the entry's four
// threads had with two-byte loads) the records q per + u + 32 k.  A wave load covers 8 records x 128 contiguous bytes.  One
// round holds K values of k for all four quarters of every tile: with K = 2 8 loads per thread and tile, which at nwg <= 256
// is every record -- the whole reduction is ONE memory round trip; more records loop.  K = 1 is enough up to 128 records
// (a quarter then has at most 32) and spares the wholly masked second load.  As in record_range_sum the loads go to their
// own registers (record_tile_issue), the caller places ONE __builtin_amdgcn_sched_barrier(0) behind everything it wants
// in flight together, and only then come the adds (record_tile_accumulate), in increasing k per accumulator.
// record_tile_finish transposes a tile's partials through LDS so that thread (entry e = tid & 63, quarter q = tid >> 6)
// holds a[0..31] of its quarter and runs the st = 16..1 tree on them: bit for bit record_range_sum(r + entry, q per, ..).
// The entry offset i0 must be a multiple of 8 and the class's first record 16-byte aligned (a record is 32 256 bytes).
typedef unsigned int rec8_t __attribute__((ext_vector_type(4)));   // 8 consecutive entries
constexpr int TILE = 64;                       // entries per tile
constexpr int TILE_LDS_FLOATS = 4 * TILE * 32; // the transposition buffer of record_tile_finish
static_assert(REC_ENTRIES % 8 == 0 && (REC_ENTRIES * sizeof(rec_t)) % 16 == 0, "16-byte loads need aligned records");

template <int TILES, int K>
__device__ __forceinline__ void record_tile_issue(rec8_t (&v)[TILES][4][K], const rec_t* __restrict__ rc, int i0, int nwg,
                                                  int k0) {
  const int g = threadIdx.x & 7, u = threadIdx.x >> 3, per = (nwg + 3) / 4;
#pragma unroll
  for (int p = 0; p < TILES; ++p) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        // (a slot past its quarter loads the class's last record and is zeroed in record_tile_accumulate: a load under a
        //  condition becomes a branch, and the compiler waits for earlier loads inside such branches)
        const int s = u + 32 * (k0 + k), w = q * per + s;
        const int wc = (s < per && w < nwg) ? w : nwg - 1;
        v[p][q][k] = *reinterpret_cast<const rec8_t*>(rc + (size_t)wc * REC_ENTRIES + i0 + p * TILE + 8 * g);
      }
    }
  }
}
template <int TILES, int K>
__device__ __forceinline__ void record_tile_accumulate(float (&acc)[TILES][4][8], const rec8_t (&v)[TILES][4][K], int nwg,
                                                       int k0) {
  const int u = threadIdx.x >> 3, per = (nwg + 3) / 4;
#pragma unroll
  for (int p = 0; p < TILES; ++p) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int s = u + 32 * (k0 + k);
        const unsigned keep = (s < per && q * per + s < nwg) ? 0xffffffffu : 0u;   // +0 for a slot past its quarter
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const unsigned x = v[p][q][k][d] & keep;
          acc[p][q][2 * d] += __builtin_bit_cast(float, x << 16);
          acc[p][q][2 * d + 1] += __builtin_bit_cast(float, x & 0xffff0000u);
        }
      }
    }
  }
}
// (the buffer is swizzled: a thread's 32 reads and the writes of a wave spread over the banks).  Ends on a barrier, so the
// buffer can take the next tile; garbage in one entry (an unwritten one) stays in that entry's rows.
__device__ __forceinline__ float record_tile_finish(const float (&acc)[4][8], float* __restrict__ tr) {
  const int g = threadIdx.x & 7, u = threadIdx.x >> 3;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int row = q * TILE + 8 * g + j;
      tr[row * 32 + (u ^ (row & 31))] = acc[q][j];
    }
  }
  __syncthreads();
  constexpr int U = 32;
  float a[U];
  const int row = threadIdx.x;   // = q * TILE + e
#pragma unroll
  for (int s = 0; s < U; ++s) a[s] = tr[row * 32 + (s ^ (row & 31))];
#pragma unroll
  for (int st = U / 2; st >= 1; st >>= 1) {
#pragma unroll
    for (int s = 0; s < st; ++s) a[s] += a[s + st];
  }
  __syncthreads();
  return a[0];
}
}  // namespace cnr_rec
