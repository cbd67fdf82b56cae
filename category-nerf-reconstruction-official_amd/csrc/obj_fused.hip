// cnr_obj_train: one launch = one train step of EVERY per-object field of a scene (registration's pretrained fields: a vMAP-style
// OccupancyMap(hidden 32) + UniDirsEmbed per object, src/model.py:86-155; the step is the reference's background branch,
// train.py:113-121,172-184, with a leading dimension of 1 per object).  Objects share nothing, so ONE WORKGROUP owns one object
// for the whole step: rows -> rays -> PE -> field -> composite + losses -> backward -> dB -> AdamW, with no cross-workgroup
// reduction, no wait across workgroups and no float atomic: every gradient element is accumulated by exactly one thread in a
// fixed order, and the same thread applies AdamW to it.
//
// Arithmetic: exact fp32 on the vector unit (fused multiply-adds, fp32 accumulation) -- the object's 11 008 matrix weights sit
// TRANSPOSED in LDS as fp32 for the whole step, the activations and pre-activation gradients of one tile of whole rays beside
// them.  A tile is floor(64 / S) whole rays (S <= 64), so a ray's sigma / colour are complete before its composite and its
// d sigma / d colour before the tile's backward by construction: no ray straddles a tile.  ("Per-object fields", has
// the LDS map and why this is not the f16 MFMA layout of bg_fused.hip.)
#include "sample_common.h"
#include "render_common.h"
#include "adamw_common.h"
#include "obj_args.h"

namespace {
constexpr int H = 32, E1 = CNR_E1, E2 = CNR_E2, NDIR = 21;
constexpr int THREADS = 512, WAVES = THREADS / 64, TS = 64;
constexpr float PI_F = 3.14159265358979323846f;
// theta: the 14 tensors of OccupancyMap(87, 42, 32) in registration order, then B_layer.weight (include/cnr_hip.h)
constexpr int K_IN = E1, K_CAT = H + E1, K_CL = H + E2;
constexpr int O_IN_W = 0, O_IN_B = O_IN_W + H * K_IN, O_M1_W = O_IN_B + H, O_M1_B = O_M1_W + H * H, O_CAT_W = O_M1_B + H,
              O_CAT_B = O_CAT_W + H * K_CAT, O_M2_W = O_CAT_B + H, O_M2_B = O_M2_W + H * H, O_OA_W = O_M2_B + H, O_OA_B = O_OA_W + H,
              O_CL_W = O_OA_B + 1, O_CL_B = O_CL_W + H * K_CL, O_OC_W = O_CL_B + H, O_OC_B = O_OC_W + 3 * H, O_B = O_OC_B + 3,
              NPARAM = O_B + NDIR * 3;
static_assert(NPARAM == 11363, "OccupancyMap(87, 42, 32) + UniDirsEmbed");
// rows of the transposed weight image WT[q][32]: WT[Q_l + k][j] = W_l[j][k] for the five 32-wide layers
constexpr int Q_IN = 0, Q_M1 = Q_IN + K_IN, Q_CAT = Q_M1 + H, Q_M2 = Q_CAT + K_CAT, Q_CL = Q_M2 + H, QN = Q_CL + K_CL;
static_assert(QN == 344, "weight rows");
constexpr int UNITS = QN * 4;                       // weight-gradient units: (row q, 8 outputs)
constexpr int UNITS_PER_THREAD = (UNITS + THREADS - 1) / THREADS;
static_assert(UNITS_PER_THREAD == 3 && UNITS - 2 * THREADS + 5 * H == THREADS, "units, then the 160 biases, fill the last round");
// columns of the activation image ACT[sample][AW]: PE features (e1 | e2), then the post-ReLU outputs of the five layers
constexpr int A_E = 0, A_E2 = E1, A_H1 = E1 + E2, A_H2 = A_H1 + H, A_H3 = A_H2 + H, A_H4 = A_H3 + H, A_H5 = A_H4 + H, AW = A_H5 + H;
static_assert((AW & 1) == 1, "odd row stride: a column over samples and a row over columns are both bank-conflict free");
// small parameters SP[]: the five biases, out_alpha, out_color, B
constexpr int SP_BIAS = 0, SP_OA_W = 5 * H, SP_OA_B = SP_OA_W + H, SP_OC_W = SP_OA_B + 1, SP_OC_B = SP_OC_W + 3 * H,
              SP_B = SP_OC_B + 3, SP_N = (SP_B + NDIR * 3 + 3) & ~3;
constexpr int N_HEAD = 3 * H + 3 + H + 1;            // out_color W, b; out_alpha W, b: one gradient element per thread
// LDS (floats): WT | ACT | D (5 layers x 64 samples x 32, swizzled) | SP | PTS | DSIG | DRGB | RED
constexpr int L_WT = 0, L_ACT = L_WT + QN * H, L_D = L_ACT + TS * AW, L_SP = L_D + 5 * TS * H, L_PTS = L_SP + SP_N,
              L_DSIG = L_PTS + TS * 3, L_DRGB = L_DSIG + TS, L_RED = L_DRGB + TS * 3, L_END = L_RED + 64;
constexpr int LDS_BYTES = L_END * 4;
static_assert(LDS_BYTES <= 160 * 1024, "one workgroup per CU: 160 KB of LDS");

typedef float f4 __attribute__((ext_vector_type(4)));

struct ObjArgs {
  const uint8_t* rgbs; const float* depth; const float* dirs_c; const float* T; const int64_t* pool_off; const int* obj_ids;
  int N, R, n1, n2; float eps, stop_eps, min_bound, scale; uint64_t seed;
  const int* rows; const float* u; const float* g;
  int64_t* d_state; float* theta; float* exp_avg; float* exp_avg_sq;
  float lr, b1, b2, adam_eps, wd, color_scaling, opacity_scaling;
  float* losses; int32_t* flags; float* grad; float* sigma; float* rgb; float* z; int* rows_out;
  uint32_t* ws; int64_t ws_stride;
};

// index of D[layer][sample][j] (j a multiple of 4 for a 16-byte access): the four-float groups of a row are XOR-ed with the
// sample's low bits, so that the 16-byte accesses of consecutive samples fall on different banks
__device__ __forceinline__ int dix(int l, int s, int j) { return L_D + ((l * TS + s) << 5) + (j ^ ((s & 7) << 2)); }
__device__ __forceinline__ f4 ld4(const float* p) { return *reinterpret_cast<const f4*>(p); }
__device__ __forceinline__ float dot4(f4 a, f4 b, float acc) {
  acc = fmaf(a[0], b[0], acc); acc = fmaf(a[1], b[1], acc); acc = fmaf(a[2], b[2], acc); return fmaf(a[3], b[3], acc);
}
// sum over j < 32 of drow[j] * WT[q][j] (drow: the sample's row of one D layer in registers)
__device__ __forceinline__ float dot32(const f4 (&drow)[8], const float* __restrict__ lds, int q) {
  const float* w = lds + L_WT + q * H;
  float a = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) a = dot4(drow[i], ld4(w + 4 * i), a);
  return a;
}
__device__ __forceinline__ void load_drow(f4 (&drow)[8], const float* __restrict__ lds, int l, int s) {
#pragma unroll
  for (int i = 0; i < 8; ++i) drow[i] = ld4(lds + dix(l, s, 4 * i));
}

// layer, input index and ACT column of weight row q; offset of W_l / b_l in theta and the layer's input width
struct RowInfo { int l, k, col; };
__device__ __forceinline__ RowInfo row_info(int q) {
  if (q < Q_M1) return {0, q, A_E + q};
  if (q < Q_CAT) return {1, q - Q_M1, A_H1 + q - Q_M1};
  if (q < Q_M2) { const int k = q - Q_CAT; return {2, k, k < H ? A_H2 + k : A_E + k - H}; }
  if (q < Q_CL) return {3, q - Q_M2, A_H3 + q - Q_M2};
  const int k = q - Q_CL;
  return {4, k, k < H ? A_H4 + k : A_E2 + k - H};
}
__device__ __forceinline__ int w_off(int l) { return l == 0 ? O_IN_W : l == 1 ? O_M1_W : l == 2 ? O_CAT_W : l == 3 ? O_M2_W : O_CL_W; }
__device__ __forceinline__ int b_off(int l) { return l == 0 ? O_IN_B : l == 1 ? O_M1_B : l == 2 ? O_CAT_B : l == 3 ? O_M2_B : O_CL_B; }
__device__ __forceinline__ int k_of(int l) { return l == 0 ? K_IN : l == 2 ? K_CAT : l == 4 ? K_CL : H; }

// one 32-wide layer + ReLU for sample s, outputs 4 og .. 4 og + 3: inputs are ACT columns colA .. colA + nA - 1, then
// colB .. (weight rows q0 ..); the result goes to ACT columns out ..
__device__ __forceinline__ void layer_fwd(float* __restrict__ lds, int s, int og, int q0, int l, int colA, int nA, int colB, int nB,
                                          int out) {
  const float* x = lds + L_ACT + s * AW;
  const float* w = lds + L_WT + q0 * H + 4 * og;
  f4 acc = ld4(lds + L_SP + SP_BIAS + l * H + 4 * og);
  for (int k = 0; k < nA; ++k) {
    const float xv = x[colA + k];
    const f4 wv = ld4(w + k * H);
    acc[0] = fmaf(xv, wv[0], acc[0]); acc[1] = fmaf(xv, wv[1], acc[1]); acc[2] = fmaf(xv, wv[2], acc[2]); acc[3] = fmaf(xv, wv[3], acc[3]);
  }
  w += nA * H;
  for (int k = 0; k < nB; ++k) {
    const float xv = x[colB + k];
    const f4 wv = ld4(w + k * H);
    acc[0] = fmaf(xv, wv[0], acc[0]); acc[1] = fmaf(xv, wv[1], acc[1]); acc[2] = fmaf(xv, wv[2], acc[2]); acc[3] = fmaf(xv, wv[3], acc[3]);
  }
  float* y = lds + L_ACT + s * AW + out + 4 * og;
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = fmaxf(acc[i], 0.f);
}
// backward through one layer's first 32 input columns: d h[j] = sum_j' D[lsrc][s][j'] W[j'][j] (+ extra[j]), times the ReLU
// mask of ACT column hcol + j -> D[ldst][s][j], for j = 4 og .. 4 og + 3
__device__ __forceinline__ void layer_bwd(float* __restrict__ lds, int s, int og, int lsrc, int q0, int hcol, int ldst, f4 extra) {
  f4 drow[8];
  load_drow(drow, lds, lsrc, s);
  f4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = 4 * og + i;
    const float dh = dot32(drow, lds, q0 + j) + extra[i];
    o[i] = lds[L_ACT + s * AW + hcol + j] > 0.f ? dh : 0.f;
  }
  *reinterpret_cast<f4*>(lds + dix(ldst, s, 4 * og)) = o;
}

__device__ __forceinline__ void adam_one(const ObjArgs& a, size_t base, int idx, float g, float step_size, float inv_bc2_sqrt) {
  const size_t i = base + idx;
  if (a.grad) a.grad[i] = g;
  float pi = a.theta[i] * (1.0f - a.lr * a.wd);
  const float m0 = a.exp_avg[i], v0 = a.exp_avg_sq[i];
  const float mi = m0 + (g - m0) * (1.0f - a.b1);
  const float vi = v0 * a.b2 + (1.0f - a.b2) * g * g;
  const float denom = sqrtf(vi) * inv_bc2_sqrt + a.adam_eps;
  pi -= step_size * (mi / denom);
  a.theta[i] = pi; a.exp_avg[i] = mi; a.exp_avg_sq[i] = vi;
}

__global__ __launch_bounds__(THREADS) void obj_train_kernel(ObjArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int o = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int s = lane, og = wv;                       // the per-sample phases: thread = (sample, 4 outputs)
  const int R = a.R, S = a.n1 + a.n2, RS = R * S;
  const int64_t seg0 = a.pool_off[o], rows_o = a.pool_off[o + 1] - seg0;
  int64_t* st = a.d_state + (size_t)o * 4;
  const size_t pbase = (size_t)o * NPARAM;
  if (rows_o < R) {     // (the host checks the shortest segment; a wrong answer there must not become a read out of bounds)
    if (tid == 0) { a.flags[o] = 16; a.losses[o] = 0.f; a.losses[a.N + o] = 0.f; a.losses[2 * a.N + o] = 0.f; }
    return;
  }
  const int64_t cursor = st[0], rng_step = st[1], opt_step = st[2], epoch = st[3];
  const uint64_t gid = (uint64_t)(a.obj_ids ? a.obj_ids[o] : o);
  // workspace of this object (4-byte words): z | pts | sigma | rgb | gt_rgb | gt_depth | rows | depth_mask, labels (bytes)
  uint32_t* ws = a.ws + (size_t)o * a.ws_stride;
  float* w_z = reinterpret_cast<float*>(ws);
  float* w_pts = w_z + RS;
  float* w_sig = w_pts + 3 * (size_t)RS;
  float* w_rgb = w_sig + RS;
  float* w_gtc = w_rgb + 3 * (size_t)RS;
  float* w_gtd = w_gtc + 3 * R;
  int* w_rows = reinterpret_cast<int*>(w_gtd + R);
  uint8_t* w_dm = reinterpret_cast<uint8_t*>(w_rows + R);
  uint8_t* w_lab = w_dm + R;
  const uint8_t* rgbs = a.rgbs + seg0 * 4;
  const float* depth = a.depth + seg0;

  // ---- the object's parameters into LDS: transposed weights, small parameters ---------------------------------------------
  const float* th = a.theta + pbase;
  for (int i = tid; i < QN * H; i += THREADS) {
    const int q = i >> 5, j = i & 31;
    const RowInfo ri = row_info(q);
    lds[L_WT + i] = th[w_off(ri.l) + j * k_of(ri.l) + ri.k];
  }
  for (int i = tid; i < 5 * H; i += THREADS) lds[L_SP + SP_BIAS + i] = th[b_off(i >> 5) + (i & 31)];
  for (int i = tid; i < H + 1; i += THREADS) lds[L_SP + SP_OA_W + i] = th[O_OA_W + i];
  for (int i = tid; i < 3 * H + 3; i += THREADS) lds[L_SP + SP_OC_W + i] = th[O_OC_W + i];
  for (int i = tid; i < NDIR * 3; i += THREADS) lds[L_SP + SP_B + i] = th[O_B + i];

  // ---- rows of the step, their max depth and mask counts (reduce_batch_loss's, over this object's R rows) -------------------
  int flag = 0;
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
      w_rows[r] = (int)row;
      const float d = depth[row];
      const uint8_t lab = rgbs[row * 4 + 3];
      mx = fmaxf(mx, d);
      const bool mo = lab != 0, ms = lab != 2, md = d > a.min_bound;
      c_d += (md && mo) ? 1 : 0; c_o += mo ? 1 : 0; c_s += ms ? 1 : 0;
    }
    mx = cnr::wave_max(mx);
    for (int off = 32; off > 0; off >>= 1) {
      c_d += __shfl_xor(c_d, off, 64); c_o += __shfl_xor(c_o, off, 64); c_s += __shfl_xor(c_s, off, 64); bad |= __shfl_xor(bad, off, 64);
    }
    if (lane == 0) {
      lds[L_RED + wv] = mx; lds[L_RED + 8 + wv] = (float)c_d; lds[L_RED + 16 + wv] = (float)c_o; lds[L_RED + 24 + wv] = (float)c_s;
      lds[L_RED + 32 + wv] = (float)bad;
    }
  }
  __syncthreads();
  float mb = lds[L_RED], n_d = 0.f, n_o = 0.f, n_s = 0.f, n_bad = 0.f;
  for (int w = 0; w < WAVES; ++w) {   // (counts <= R: exact in fp32)
    mb = fmaxf(mb, lds[L_RED + w]); n_d += lds[L_RED + 8 + w]; n_o += lds[L_RED + 16 + w]; n_s += lds[L_RED + 24 + w];
    n_bad += lds[L_RED + 32 + w];
  }
  // a zero mask count zeroes that term and its gradient (render_rays.py:67-72 with one class), flags as cnr_render_loss's
  const float wd = n_d == 0.f ? 0.f : 1.0f / (n_d + 1e-10f), wc = n_o == 0.f ? 0.f : 1.0f / (n_o + 1e-10f),
              wo = n_s == 0.f ? 0.f : 1.0f / (n_s + 1e-10f);
  flag = (n_d == 0.f ? 2 : 0) | (n_o == 0.f ? 4 : 0) | (n_s == 0.f ? 8 : 0) | (n_bad != 0.f ? 32 : 0);
  __syncthreads();      // (RED is reused below)

  // ---- a2-a5: one wave per ray (sample_common.h; z without fused multiply-adds: the reference's bits) -------------------
  {
    cnr_sample::SampleArgs sa{};
    sa.rgbs = rgbs; sa.depth = depth; sa.dirs_c = a.dirs_c + seg0 * 3; sa.T = a.T + seg0 * 16;
    sa.u = a.u ? a.u + (size_t)o * RS : nullptr; sa.g = a.g ? a.g + (size_t)o * R * a.n2 : nullptr;
    sa.seed = a.seed; sa.world_frame = 1; sa.C = 1; sa.R = R; sa.n1 = a.n1; sa.n2 = a.n2;
    sa.eps = a.eps; sa.stop_eps = a.stop_eps; sa.min_bound = a.min_bound;
    sa.z = w_z; sa.pts = w_pts; sa.gt_rgb = w_gtc; sa.gt_depth = w_gtd; sa.depth_mask = w_dm; sa.labels = w_lab;
    for (int r = wv; r < R; r += WAVES)
      cnr_sample::sample_ray_at<true>(sa, r, w_rows[r], 0, gid * (uint64_t)R + (uint64_t)r, (uint64_t)rng_step * 4, mb, lane);
  }
  __syncthreads();

  // ---- gradient accumulators: this thread's weight units (row q, 8 outputs), one bias or head element, its wave's share of dB --
  float acc[UNITS_PER_THREAD][8];
  int ucol[UNITS_PER_THREAD], ulay[UNITS_PER_THREAD];
#pragma unroll
  for (int i = 0; i < UNITS_PER_THREAD; ++i) {
    const int un = tid + THREADS * i;
    const RowInfo ri = row_info(un < UNITS ? un >> 2 : 0);
    ucol[i] = ri.col; ulay[i] = ri.l;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
  }
  const int bias_e = tid - (UNITS - 2 * THREADS);      // >= 0: this thread owns bias element bias_e (layer bias_e / 32)
  float acc_bias = 0.f, acc_head = 0.f;
  float acc_B[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};   // directions wv, wv + 8, wv + 16 (all lanes hold the sums)
  float l_d = 0.f, l_c = 0.f, l_o = 0.f;                 // this wave's rays' loss terms

  const int G = TS / S;                                  // whole rays per tile
  const float scale = a.scale;
  for (int r0 = 0; r0 < R; r0 += G) {
    const int nrays = min(G, R - r0), ns = nrays * S;
    const size_t m0 = (size_t)r0 * S;                    // first sample of the tile
    const bool on = s < ns;
    // ---- PE (cnr_pe_fwd's expressions): t = x / scale ; e = (t, sin(pi 2^f B_d . t))
    float t0 = 0.f, t1 = 0.f, t2 = 0.f;
    if (on) {
      const float* p = w_pts + (m0 + s) * 3;
      t0 = p[0] / scale; t1 = p[1] / scale; t2 = p[2] / scale;
    }
    {
      float* e = lds + L_ACT + s * AW;
      if (og == 0) {
        e[0] = t0; e[1] = t1; e[2] = t2;
        lds[L_PTS + s * 3 + 0] = t0; lds[L_PTS + s * 3 + 1] = t1; lds[L_PTS + s * 3 + 2] = t2;
      }
      for (int d = og; d < NDIR; d += WAVES) {
        const float* Bd = lds + L_SP + SP_B + d * 3;
        const float p = Bd[0] * t0 + Bd[1] * t1 + Bd[2] * t2;
#pragma unroll
        for (int f = 0; f < 6; ++f) e[3 + NDIR * f + d] = sinf((p * (float)(1 << f)) * PI_F);
      }
    }
    __syncthreads();
    // ---- forward
    layer_fwd(lds, s, og, Q_IN, 0, A_E, E1, 0, 0, A_H1);
    __syncthreads();
    layer_fwd(lds, s, og, Q_M1, 1, A_H1, H, 0, 0, A_H2);
    __syncthreads();
    layer_fwd(lds, s, og, Q_CAT, 2, A_H2, H, A_E, E1, A_H3);
    __syncthreads();
    layer_fwd(lds, s, og, Q_M2, 3, A_H3, H, 0, 0, A_H4);
    __syncthreads();
    layer_fwd(lds, s, og, Q_CL, 4, A_H4, H, A_E2, E2, A_H5);
    __syncthreads();
    if (og < 4 && on) {          // heads: wave 0 the x10 occupancy logit, waves 1..3 one colour channel each
      const float* x = lds + L_ACT + s * AW + (og == 0 ? A_H4 : A_H5);
      const float* w = lds + L_SP + (og == 0 ? SP_OA_W : SP_OC_W + (og - 1) * H);
      float v = lds[L_SP + (og == 0 ? SP_OA_B : SP_OC_B + og - 1)];
      for (int j = 0; j < H; ++j) v = fmaf(x[j], w[j], v);
      if (og == 0) w_sig[m0 + s] = v * 10.0f;
      else w_rgb[(m0 + s) * 3 + og - 1] = cnr_rl::sigmoid_exact(v);
    }
    __syncthreads();
    // ---- composite, loss terms and their gradient: one ray per wave (render_common.h)
    for (int rr = wv; rr < nrays; rr += WAVES) {
      const int ray = r0 + rr;
      const size_t base = (size_t)ray * S;
      const cnr_rl::RayOut q = cnr_rl::ray_small(w_sig, w_rgb, w_z, base, S, lane, w_gtd[ray], w_gtc[ray * 3 + 0], w_gtc[ray * 3 + 1],
                                                 w_gtc[ray * 3 + 2], w_lab[ray], w_dm[ray], wd, wc, wo, a.color_scaling,
                                                 a.opacity_scaling, 1.0f);
      l_d += q.ld; l_c += q.lc; l_o += q.lo;
      if (lane < S) {
        const int sl = rr * S + lane;
        const float c0 = w_rgb[(base + lane) * 3 + 0], c1 = w_rgb[(base + lane) * 3 + 1], c2 = w_rgb[(base + lane) * 3 + 2];
        lds[L_DSIG + sl] = q.dsig * 10.0f;                                   // d of the raw logit
        lds[L_DRGB + sl * 3 + 0] = q.dc0 * (c0 * (1.0f - c0));             // d of the pre-sigmoid colour
        lds[L_DRGB + sl * 3 + 1] = q.dc1 * (c1 * (1.0f - c1));
        lds[L_DRGB + sl * 3 + 2] = q.dc2 * (c2 * (1.0f - c2));
      }
    }
    __syncthreads();
    // ---- backward chain: color_linear <- out_color ; mid2 <- color_linear + out_alpha ; cat ; mid1 ; in
    if (on) {
      const float d0 = lds[L_DRGB + s * 3 + 0], d1 = lds[L_DRGB + s * 3 + 1], d2 = lds[L_DRGB + s * 3 + 2];
      f4 ov;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = 4 * og + i;
        const float dh = d0 * lds[L_SP + SP_OC_W + j] + d1 * lds[L_SP + SP_OC_W + H + j] + d2 * lds[L_SP + SP_OC_W + 2 * H + j];
        ov[i] = lds[L_ACT + s * AW + A_H5 + j] > 0.f ? dh : 0.f;
      }
      *reinterpret_cast<f4*>(lds + dix(4, s, 4 * og)) = ov;
    }
    __syncthreads();
    if (on) {
      const float da = lds[L_DSIG + s];
      const f4 oa = ld4(lds + L_SP + SP_OA_W + 4 * og);
      layer_bwd(lds, s, og, 4, Q_CL, A_H4, 3, f4{da * oa[0], da * oa[1], da * oa[2], da * oa[3]});
    }
    __syncthreads();
    if (on) layer_bwd(lds, s, og, 3, Q_M2, A_H3, 2, f4{0.f, 0.f, 0.f, 0.f});
    __syncthreads();
    if (on) layer_bwd(lds, s, og, 2, Q_CAT, A_H2, 1, f4{0.f, 0.f, 0.f, 0.f});
    __syncthreads();
    if (on) layer_bwd(lds, s, og, 1, Q_M1, A_H1, 0, f4{0.f, 0.f, 0.f, 0.f});
    __syncthreads();
    // ---- weight gradients: each unit's owner walks the tile's samples in order
#pragma unroll
    for (int i = 0; i < UNITS_PER_THREAD; ++i) {
      const int un = tid + THREADS * i;
      if (un < UNITS) {
        const int jg = un & 3, col = ucol[i], l = ulay[i];
        for (int ss = 0; ss < ns; ++ss) {
          const float x = lds[L_ACT + ss * AW + col];
          const f4 da = ld4(lds + dix(l, ss, 8 * jg)), db = ld4(lds + dix(l, ss, 8 * jg + 4));
#pragma unroll
          for (int j = 0; j < 4; ++j) { acc[i][j] = fmaf(x, da[j], acc[i][j]); acc[i][4 + j] = fmaf(x, db[j], acc[i][4 + j]); }
        }
      }
    }
    if (bias_e >= 0) {
      const int l = bias_e >> 5, j = bias_e & 31;
      for (int ss = 0; ss < ns; ++ss) acc_bias += lds[L_D + ((l * TS + ss) << 5) + (j ^ ((ss & 7) << 2))];
    }
    if (tid < N_HEAD) {
      if (tid < 3 * H) {                       // out_color W[c][j]
        const int c = tid >> 5, j = tid & 31;
        for (int ss = 0; ss < ns; ++ss) acc_head = fmaf(lds[L_DRGB + ss * 3 + c], lds[L_ACT + ss * AW + A_H5 + j], acc_head);
      } else if (tid < 3 * H + 3) {            // out_color b[c]
        for (int ss = 0; ss < ns; ++ss) acc_head += lds[L_DRGB + ss * 3 + tid - 3 * H];
      } else if (tid < 4 * H + 3) {            // out_alpha W[j]
        const int j = tid - (3 * H + 3);
        for (int ss = 0; ss < ns; ++ss) acc_head = fmaf(lds[L_DSIG + ss], lds[L_ACT + ss * AW + A_H4 + j], acc_head);
      } else {                                 // out_alpha b
        for (int ss = 0; ss < ns; ++ss) acc_head += lds[L_DSIG + ss];
      }
    }
    // ---- PE backward to dB (cnr_pe_bwd's expressions): d p_d = sum_f d e[3 + 21 f + d] cos(pi 2^f p_d) pi 2^f ; dB_d += d p_d t
    {
      float dp[3] = {0.f, 0.f, 0.f}, cf[3][6];
#pragma unroll
      for (int dd = 0; dd < 3; ++dd) {
        const int d = min(og + WAVES * dd, NDIR - 1);
        const float* Bd = lds + L_SP + SP_B + d * 3;
        const float p = Bd[0] * t0 + Bd[1] * t1 + Bd[2] * t2;
#pragma unroll
        for (int f = 0; f < 6; ++f) { const float fk = (float)(1 << f); cf[dd][f] = cosf((p * fk) * PI_F) * (fk * PI_F); }
      }
      const int sr = on ? s : 0;
      f4 drow[8];
      // e1 feeds in_layer (D layer 0, rows Q_IN + k) and cat_layer (D layer 2, rows Q_CAT + 32 + k); e2 feeds color_linear
#pragma unroll
      for (int pass = 0; pass < 3; ++pass) {
        const int l = pass == 0 ? 0 : pass == 1 ? 2 : 4;
        const int qb = pass == 0 ? Q_IN : pass == 1 ? Q_CAT + H : Q_CL + H - E1;       // row of PE feature k: qb + k
        load_drow(drow, lds, l, sr);
#pragma unroll
        for (int dd = 0; dd < 3; ++dd) {
          const int d = og + WAVES * dd;
          if (d < NDIR) {
#pragma unroll
            for (int f = 0; f < 6; ++f)
              if ((f < 4) == (pass < 2)) dp[dd] = fmaf(dot32(drow, lds, qb + 3 + NDIR * f + d), cf[dd][f], dp[dd]);
          }
        }
      }
#pragma unroll
      for (int dd = 0; dd < 3; ++dd) {
        const float v = on ? dp[dd] : 0.f;
        acc_B[dd][0] += cnr::wave_sum(v * t0); acc_B[dd][1] += cnr::wave_sum(v * t1); acc_B[dd][2] += cnr::wave_sum(v * t2);
      }
    }
    __syncthreads();
  }

  // ---- loss values and flags (the waves' terms in a fixed order)
  if (lane == 0) { lds[L_RED + wv * 3 + 0] = l_d; lds[L_RED + wv * 3 + 1] = l_c; lds[L_RED + wv * 3 + 2] = l_o; }
  __syncthreads();
  if (tid == 0) {
    float sd = 0.f, sc = 0.f, so = 0.f;
    for (int w = 0; w < WAVES; ++w) { sd += lds[L_RED + w * 3 + 0]; sc += lds[L_RED + w * 3 + 1]; so += lds[L_RED + w * 3 + 2]; }
    sd *= wd; sc *= wc; so *= wo;
    a.losses[o] = sd; a.losses[a.N + o] = sc; a.losses[2 * a.N + o] = so;
    if (sd > 100000.f || sc > 100000.f || so > 100000.f) flag |= 1;
    a.flags[o] = flag;
    // the step state: rows, RNG step, optimiser step; the object's own epoch end (src/scene_cateogries.py:439-449)
    int64_t cur = cursor + R, ep = epoch;
    if (cur >= rows_o - R) { cur = 0; ep += 1; }
    st[0] = cur; st[1] = rng_step + 1; st[2] = opt_step + 1; st[3] = ep;
  }

  // ---- AdamW by each gradient element's owner (torch.optim.AdamW, adamw_common.h's expressions)
  float step_size, inv_bc2_sqrt;
  {
    cnr::AdamArgs aa{};
    aa.lr = a.lr; aa.b1 = a.b1; aa.b2 = a.b2;
    cnr::adam_coefficients(aa, opt_step + 1, step_size, inv_bc2_sqrt);
  }
#pragma unroll
  for (int i = 0; i < UNITS_PER_THREAD; ++i) {
    const int un = tid + THREADS * i;
    if (un < UNITS) {
      const RowInfo ri = row_info(un >> 2);
      const int base = w_off(ri.l) + ri.k, K = k_of(ri.l), j0 = 8 * (un & 3);
#pragma unroll
      for (int j = 0; j < 8; ++j) adam_one(a, pbase, base + (j0 + j) * K, acc[i][j], step_size, inv_bc2_sqrt);
    }
  }
  if (bias_e >= 0) adam_one(a, pbase, b_off(bias_e >> 5) + (bias_e & 31), acc_bias, step_size, inv_bc2_sqrt);
  if (tid < N_HEAD) {
    const int idx = tid < 3 * H + 3 ? O_OC_W + tid : O_OA_W + tid - (3 * H + 3);      // (W then b, contiguous in theta, both heads)
    adam_one(a, pbase, idx, acc_head, step_size, inv_bc2_sqrt);
  }
  if (lane < 9) {
    float v = 0.f;
#pragma unroll
    for (int dd = 0; dd < 3; ++dd)
#pragma unroll
      for (int i = 0; i < 3; ++i) if (lane == dd * 3 + i) v = acc_B[dd][i];
    const int d = og + WAVES * (lane / 3);
    if (d < NDIR) adam_one(a, pbase, O_B + d * 3 + lane % 3, v, step_size, inv_bc2_sqrt);
  }
  // ---- the test outputs
  if (a.sigma) for (int i = tid; i < RS; i += THREADS) a.sigma[(size_t)o * RS + i] = w_sig[i];
  if (a.z) for (int i = tid; i < RS; i += THREADS) a.z[(size_t)o * RS + i] = w_z[i];
  if (a.rgb) for (int i = tid; i < 3 * RS; i += THREADS) a.rgb[(size_t)o * RS * 3 + i] = w_rgb[i];
  if (a.rows_out) for (int i = tid; i < R; i += THREADS) a.rows_out[(size_t)o * R + i] = w_rows[i];
}

cnr::DeviceOnce g_lds_once;
}  // namespace

extern "C" int cnr_obj_param_count(void) { return NPARAM; }

static_assert(cnr_obj::MAX_S == TS && cnr_obj::E_ARG == CNR_E_ARG, "obj_args.h");
extern "C" int64_t cnr_obj_workspace_bytes(int N, int R, int S) { return cnr_obj::workspace_bytes(N, R, S); }

extern "C" int cnr_obj_train(const uint8_t* rgbs, const float* depth, const float* dirs_c, const float* T, const int64_t* pool_off,
                             int64_t min_pool_rows, const int* obj_ids, int N, int R, int n1, int n2, float eps, float stop_eps,
                             float min_bound, float scale, uint64_t seed, const int* rows, const float* u, const float* g,
                             int64_t* d_state, float* theta, float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2,
                             float adam_eps, float weight_decay, float color_scaling, float opacity_scaling, float* losses,
                             int32_t* flags, float* grad, float* sigma, float* rgb, float* z, int* rows_out, void* workspace,
                             int64_t workspace_bytes, void* stream) {
  const cnr_obj::Required req{rgbs, depth, dirs_c, T, pool_off, d_state, theta, exp_avg, exp_avg_sq, losses, flags, workspace};
  if (cnr_obj::check_args(req, min_pool_rows, N, R, n1, n2, scale, rows, u, g, workspace_bytes)) return CNR_E_ARG;
  ObjArgs a{};
  a.rgbs = rgbs; a.depth = depth; a.dirs_c = dirs_c; a.T = T; a.pool_off = pool_off; a.obj_ids = obj_ids;
  a.N = N; a.R = R; a.n1 = n1; a.n2 = n2; a.eps = eps; a.stop_eps = stop_eps; a.min_bound = min_bound; a.scale = scale; a.seed = seed;
  a.rows = rows; a.u = u; a.g = g; a.d_state = d_state; a.theta = theta; a.exp_avg = exp_avg; a.exp_avg_sq = exp_avg_sq;
  a.lr = lr; a.b1 = beta1; a.b2 = beta2; a.adam_eps = adam_eps; a.wd = weight_decay; a.color_scaling = color_scaling;
  a.opacity_scaling = opacity_scaling; a.losses = losses; a.flags = flags; a.grad = grad; a.sigma = sigma; a.rgb = rgb; a.z = z;
  a.rows_out = rows_out; a.ws = static_cast<uint32_t*>(workspace); a.ws_stride = cnr_obj::ws_words(R, n1 + n2);
  const int rc = cnr::set_max_dynamic_lds(g_lds_once, reinterpret_cast<const void*>(obj_train_kernel), LDS_BYTES);
  if (rc) return rc;
  hipLaunchKernelGGL(obj_train_kernel, dim3((unsigned)N), dim3(THREADS), LDS_BYTES, (hipStream_t)stream, a);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}
