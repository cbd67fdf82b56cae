// The step skeleton of the kernels in which ONE WORKGROUP owns one optimisation problem on a ray pool for a whole step:
// cnr_obj_train (obj_fused.hip: an owner is an object) and cnr_code_fit (code_fit.hip: an owner is a candidate).  What the two
// must agree on -- the workspace layout (obj_args.h), row selection, the zero-count rule, the flag bits, the state rule -- and
// what they merely had in common -- sampling, the PE forward, the composite loop, the AdamW element, the test outputs, the launch
// -- is defined here once.  The network of each kernel (its LDS map, layers, heads, backward and update) stays in its own file.
#pragma once
#include "sample_common.h"
#include "render_common.h"
#include "adamw_common.h"
#include "obj_args.h"

namespace cnr_pool_step {
using cnr_obj::Workspace;
constexpr int THREADS = 512, WAVES = THREADS / 64, TS = 64, H = 32, NDIR = 21;
constexpr float PI_F = 3.14159265358979323846f;
static_assert(WAVES <= 8 && cnr_obj::MAX_S == TS, "RED holds 8 values per reduced quantity; a tile is whole rays of <= 64 samples");

typedef float f4 __attribute__((ext_vector_type(4)));

// the arguments both entry points take (include/cnr_hip.h); each kernel's own follow in a struct derived from this one.
// Pointers and 64-bit words first, the 32-bit scalars behind them: measured, cnr_code_fit's step is 1.5 % shorter than with the
// scalars between the pointers (0.623 against 0.634 ms at K = 64), cnr_obj_train's the same within its windows' spread.
struct StepArgs {
  const uint8_t* rgbs; const float* depth; const float* dirs_c; const float* T; const int64_t* pool_off;
  const int* rows; const float* u; const float* g;
  int64_t* d_state; float* exp_avg; float* exp_avg_sq;
  float* losses; int32_t* flags; float* grad; float* sigma; float* rgb; float* z; int* rows_out;
  uint32_t* ws; int64_t ws_stride; uint64_t seed;
  int R, n1, n2; float eps, stop_eps, min_bound, scale;
  float lr, b1, b2, adam_eps, wd, color_scaling, opacity_scaling;
};

// offset in D of D[layer or buffer][sample][j] (j a multiple of 4 for a 16-byte access): the four-float groups of a row are
// XOR-ed with the sample's low bits, so that the 16-byte accesses of consecutive samples fall on different banks
__device__ __forceinline__ int dix(int l, int s, int j) { return ((l * TS + s) << 5) + (j ^ ((s & 7) << 2)); }
__device__ __forceinline__ f4 ld4(const float* p) { return *reinterpret_cast<const f4*>(p); }
__device__ __forceinline__ float dot4(f4 a, f4 b, float acc) {
  acc = fmaf(a[0], b[0], acc); acc = fmaf(a[1], b[1], acc); acc = fmaf(a[2], b[2], acc); return fmaf(a[3], b[3], acc);
}

// max depth of the step's rows; 1 / mask count of the depth, colour and opacity terms; the flag bits 2, 4, 8 (a zero count) and 32
struct RowStats { float mb, wd, wc, wo; int flag; };
// The rows of owner o's step into w.rows -- the keyed permutation of its epoch from `cursor` on, or the given parity rows -- with
// their max depth and mask counts (reduce_batch_loss's, over this owner's R rows), reduced over the waves through red[0 .. 40).
// Both barriers are inside: red is free again on return.
__device__ __forceinline__ RowStats select_rows(const StepArgs& a, float* red, const Workspace& w, int o, int64_t seg0, int64_t rows_o,
                                                uint64_t gid, int64_t cursor, int64_t epoch, int tid, int lane, int wv) {
  const int R = a.R;
  const uint8_t* rgbs = a.rgbs + seg0 * 4;
  const float* depth = a.depth + seg0;
  {
    uint32_t key[6];
    cnr_sample::epoch_perm_keys(a.seed, (uint64_t)epoch, gid, key);
    const int hb = cnr_sample::epoch_perm_half_bits(rows_o);
    float mx = -INFINITY;
    int c_d = 0, c_o = 0, c_s = 0, bad = 0;
    for (int r = tid; r < R; r += THREADS) {
      int64_t row;
      if (a.rows) {
        row = a.rows[(size_t)o * R + r];
        if (row < 0 || row >= rows_o) { row = 0; bad = 1; }
      } else {
        row = (int64_t)cnr_sample::epoch_perm_at(key, (uint32_t)(cursor + r), rows_o, hb);
      }
      w.rows[r] = (int)row;
      const float d = depth[row];
      const uint8_t lab = rgbs[row * 4 + 3];
      mx = fmaxf(mx, d);
      const cnr_rl::MaskBits m = cnr_rl::mask_bits(lab, d > a.min_bound);
      c_d += m.md ? 1 : 0; c_o += m.mo ? 1 : 0; c_s += m.ms ? 1 : 0;
    }
    mx = cnr::wave_max(mx);
    for (int off = 32; off > 0; off >>= 1) {
      c_d += __shfl_xor(c_d, off, 64); c_o += __shfl_xor(c_o, off, 64); c_s += __shfl_xor(c_s, off, 64); bad |= __shfl_xor(bad, off, 64);
    }
    if (lane == 0) {
      red[wv] = mx; red[8 + wv] = (float)c_d; red[16 + wv] = (float)c_o; red[24 + wv] = (float)c_s;
      red[32 + wv] = (float)bad;
    }
  }
  __syncthreads();
  float mb = red[0], n_d = 0.f, n_o = 0.f, n_s = 0.f, n_bad = 0.f;
  for (int i = 0; i < WAVES; ++i) {   // (counts <= R: exact in fp32)
    mb = fmaxf(mb, red[i]); n_d += red[8 + i]; n_o += red[16 + i]; n_s += red[24 + i];
    n_bad += red[32 + i];
  }
  // a zero mask count zeroes that term and its gradient (render_rays.py:67-72 with one class), flags as cnr_render_loss's
  const cnr_rl::MaskWeights mw = cnr_rl::mask_weights(n_d, n_o, n_s, n_d == 0.f, n_o == 0.f, n_s == 0.f);
  __syncthreads();      // (RED is reused by the caller)
  return {mb, mw.wd, mw.wc, mw.wo, cnr_rl::mask_flags(n_d == 0.f, n_o == 0.f, n_s == 0.f) | (n_bad != 0.f ? 32 : 0)};
}

// a2-a5 of owner o's R rays into its workspace, one wave per ray (sample_common.h; z without fused multiply-adds: the
// reference's bits).  Rows and draws are keyed by gid, not by o: an owner's rays do not depend on its place in the launch.
__device__ __forceinline__ void sample_rays(const StepArgs& a, const Workspace& w, int o, int64_t seg0, int world_frame, uint64_t gid,
                                            int64_t rng_step, float mb, int lane, int wv) {
  const int R = a.R, RS = R * (a.n1 + a.n2);
  cnr_sample::SampleArgs sa{};
  sa.rgbs = a.rgbs + seg0 * 4; sa.depth = a.depth + seg0; sa.dirs_c = a.dirs_c + seg0 * 3; sa.T = a.T + seg0 * 16;
  sa.u = a.u ? a.u + (size_t)o * RS : nullptr; sa.g = a.g ? a.g + (size_t)o * R * a.n2 : nullptr;
  sa.seed = a.seed; sa.world_frame = world_frame; sa.C = 1; sa.R = R; sa.n1 = a.n1; sa.n2 = a.n2;
  sa.eps = a.eps; sa.stop_eps = a.stop_eps; sa.min_bound = a.min_bound;
  sa.z = w.z; sa.pts = w.pts; sa.gt_rgb = w.gtc; sa.gt_depth = w.gtd; sa.depth_mask = w.dm; sa.labels = w.lab;
  for (int r = wv; r < R; r += WAVES)
    cnr_sample::sample_ray_at<true>(sa, r, w.rows[r], 0, gid * (uint64_t)R + (uint64_t)r, (uint64_t)rng_step * 4, mb, lane);
}

// PE forward of one sample into its ACT row e (cnr_pe_fwd's expressions): t = x / scale for point m of pts (0 off the tile: !on),
// e = (t, sin(pi 2^f B_d . t)); wave og takes directions og, og + 8, ...  t comes back for the caller's PE backward.  (The
// point's address is formed inside the branch: formed by the caller it stays live and costs cnr_code_fit two VGPRs.)
__device__ __forceinline__ void pe_forward(float* e, const float* B, bool on, const float* pts, size_t m, float scale, int og, float& t0,
                                           float& t1, float& t2) {
  t0 = 0.f; t1 = 0.f; t2 = 0.f;
  if (on) {
    const float* p = pts + m * 3;
    t0 = p[0] / scale; t1 = p[1] / scale; t2 = p[2] / scale;
  }
  if (og == 0) { e[0] = t0; e[1] = t1; e[2] = t2; }
  for (int d = og; d < NDIR; d += WAVES) {
    const float* Bd = B + d * 3;
    const float pd = Bd[0] * t0 + Bd[1] * t1 + Bd[2] * t2;
#pragma unroll
    for (int f = 0; f < 6; ++f) e[3 + NDIR * f + d] = sinf((pd * (float)(1 << f)) * PI_F);
  }
}

// composite, loss terms and their gradient of the tile's rays r0 .. r0 + nrays - 1, one ray per wave (render_common.h): the
// wave's loss terms are added to l_d, l_c, l_o, the tile's samples get d of the raw logit and of the pre-sigmoid colour
__device__ __forceinline__ void composite_tile(const StepArgs& a, const Workspace& w, const RowStats& rs, float* dsig, float* drgb, int r0,
                                               int nrays, int S, int lane, int wv, float& l_d, float& l_c, float& l_o) {
  for (int rr = wv; rr < nrays; rr += WAVES) {
    const int ray = r0 + rr;
    const size_t base = (size_t)ray * S;
    const cnr_rl::RayOut q = cnr_rl::ray_small(w.sig, w.rgb, w.z, base, S, lane, w.gtd[ray], w.gtc[ray * 3 + 0], w.gtc[ray * 3 + 1],
                                               w.gtc[ray * 3 + 2], w.lab[ray], w.dm[ray], rs.wd, rs.wc, rs.wo, a.color_scaling,
                                               a.opacity_scaling, 1.0f);
    l_d += q.ld; l_c += q.lc; l_o += q.lo;
    if (lane < S) {
      const int sl = rr * S + lane;
      const float c0 = w.rgb[(base + lane) * 3 + 0], c1 = w.rgb[(base + lane) * 3 + 1], c2 = w.rgb[(base + lane) * 3 + 2];
      dsig[sl] = q.dsig * 10.0f;                                   // d of the raw logit
      drgb[sl * 3 + 0] = q.dc0 * (c0 * (1.0f - c0));             // d of the pre-sigmoid colour
      drgb[sl * 3 + 1] = q.dc1 * (c1 * (1.0f - c1));
      drgb[sl * 3 + 2] = q.dc2 * (c2 * (1.0f - c2));
    }
  }
}

// the waves' loss terms into red (the caller's barrier follows), then, by ONE thread: their sums in a fixed order, scaled by
// the mask counts, and the step's flags with bit 1 for a term above 100000
struct StepLoss { float d, c, o; int flag; };
__device__ __forceinline__ void stage_losses(float* red, float l_d, float l_c, float l_o, int lane, int wv) {
  if (lane == 0) { red[wv * 3 + 0] = l_d; red[wv * 3 + 1] = l_c; red[wv * 3 + 2] = l_o; }
}
__device__ __forceinline__ StepLoss finish_losses(const float* red, const RowStats& rs) {
  float sd = 0.f, sc = 0.f, so = 0.f;
  for (int i = 0; i < WAVES; ++i) { sd += red[i * 3 + 0]; sc += red[i * 3 + 1]; so += red[i * 3 + 2]; }
  sd *= rs.wd; sc *= rs.wc; so *= rs.wo;
  return {sd, sc, so, rs.flag | ((sd > 100000.f || sc > 100000.f || so > 100000.f) ? 1 : 0)};
}
// the step state after a step: rows, RNG step, optimiser step; the owner's own epoch end (src/scene_cateogries.py:439-449:
// when fewer than R rows are left behind the next slice)
__device__ __forceinline__ void advance_state(int64_t* st, int64_t cursor, int64_t rng_step, int64_t opt_step, int64_t epoch, int R,
                                              int64_t rows_o) {
  int64_t cur = cursor + R, ep = epoch;
  if (cur >= rows_o - R) { cur = 0; ep += 1; }
  st[0] = cur; st[1] = rng_step + 1; st[2] = opt_step + 1; st[3] = ep;
}

// step size and 1 / sqrt(bias correction 2) of optimiser step t (adamw_common.h)
__device__ __forceinline__ void adam_coefficients(const StepArgs& a, int64_t t, float& step_size, float& inv_bc2_sqrt) {
  cnr::AdamArgs aa{};
  aa.lr = a.lr; aa.b1 = a.b1; aa.b2 = a.b2;
  cnr::adam_coefficients(aa, t, step_size, inv_bc2_sqrt);
}

// the optional test outputs of owner o: its sigma, z, rgb and rows
__device__ __forceinline__ void copy_test_outputs(const StepArgs& a, const Workspace& w, int o, int tid) {
  const int R = a.R, RS = R * (a.n1 + a.n2);
  if (a.sigma) for (int i = tid; i < RS; i += THREADS) a.sigma[(size_t)o * RS + i] = w.sig[i];
  if (a.z) for (int i = tid; i < RS; i += THREADS) a.z[(size_t)o * RS + i] = w.z[i];
  if (a.rgb) for (int i = tid; i < 3 * RS; i += THREADS) a.rgb[(size_t)o * RS * 3 + i] = w.rgb[i];
  if (a.rows_out) for (int i = tid; i < R; i += THREADS) a.rows_out[(size_t)o * R + i] = w.rows[i];
}

// one workgroup per owner, `lds_bytes` of dynamic LDS (above 64 KB: told to the device once)
template <typename Args>
int launch(cnr::DeviceOnce& once, void (*kernel)(Args), int lds_bytes, int owners, void* stream, const Args& a) {
  const int rc = cnr::set_max_dynamic_lds(once, reinterpret_cast<const void*>(kernel), lds_bytes);
  if (rc) return rc;
  hipLaunchKernelGGL(kernel, dim3((unsigned)owners), dim3(THREADS), lds_bytes, (hipStream_t)stream, a);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}
}  // namespace cnr_pool_step
