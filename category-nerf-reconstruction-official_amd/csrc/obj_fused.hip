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
#include "pool_step_common.h"

namespace {
using namespace cnr_pool_step;      // the step skeleton shared with cnr_code_fit: THREADS, WAVES, TS, H, NDIR and the steps
constexpr int E1 = CNR_E1, E2 = CNR_E2;
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

struct ObjArgs : StepArgs { const int* obj_ids; int N; float* theta; };

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
  for (int i = 0; i < 8; ++i) drow[i] = ld4(lds + L_D + dix(l, s, 4 * i));
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
  *reinterpret_cast<f4*>(lds + L_D + dix(ldst, s, 4 * og)) = o;
}

__device__ __forceinline__ void adam_one(const ObjArgs& a, size_t base, int idx, float g, float step_size, float inv_bc2_sqrt) {
  const size_t i = base + idx;
  if (a.grad) a.grad[i] = g;
  const cnr::AdamElement e = cnr::adam_element(a.theta[i], a.exp_avg[i], a.exp_avg_sq[i], g, 1.0f - a.lr * a.wd, step_size, inv_bc2_sqrt,
                                               a.b1, a.b2, a.adam_eps);
  a.theta[i] = e.p; a.exp_avg[i] = e.m; a.exp_avg_sq[i] = e.v;
}

__global__ __launch_bounds__(THREADS) void obj_train_kernel(ObjArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int o = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int s = lane, og = wv;                       // the per-sample phases: thread = (sample, 4 outputs)
  const int R = a.R, S = a.n1 + a.n2;
  const int64_t seg0 = a.pool_off[o], rows_o = a.pool_off[o + 1] - seg0;
  int64_t* st = a.d_state + (size_t)o * 4;
  const size_t pbase = (size_t)o * NPARAM;
  if (rows_o < R) {     // (the host checks the shortest segment; a wrong answer there must not become a read out of bounds)
    if (tid == 0) { a.flags[o] = 16; a.losses[o] = 0.f; a.losses[a.N + o] = 0.f; a.losses[2 * a.N + o] = 0.f; }
    return;
  }
  const int64_t cursor = st[0], rng_step = st[1], opt_step = st[2], epoch = st[3];
  const uint64_t gid = (uint64_t)(a.obj_ids ? a.obj_ids[o] : o);
  const Workspace ws = cnr_obj::carve(a.ws + (size_t)o * a.ws_stride, R, S);

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

  // ---- rows of the step, their max depth and mask counts; a2-a5, one wave per ray, in the world frame ----------------------
  const RowStats rs = select_rows(a, lds + L_RED, ws, o, seg0, rows_o, gid, cursor, epoch, tid, lane, wv);
  sample_rays(a, ws, o, seg0, 1, gid, rng_step, rs.mb, lane, wv);
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
  for (int r0 = 0; r0 < R; r0 += G) {
    const int nrays = min(G, R - r0), ns = nrays * S;
    const size_t m0 = (size_t)r0 * S;                    // first sample of the tile
    const bool on = s < ns;
    // ---- PE; t stays for dB
    float t0, t1, t2;
    pe_forward(lds + L_ACT + s * AW, lds + L_SP + SP_B, on, ws.pts, m0 + s, a.scale, og, t0, t1, t2);
    if (og == 0) { lds[L_PTS + s * 3 + 0] = t0; lds[L_PTS + s * 3 + 1] = t1; lds[L_PTS + s * 3 + 2] = t2; }
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
      if (og == 0) ws.sig[m0 + s] = v * 10.0f;
      else ws.rgb[(m0 + s) * 3 + og - 1] = cnr_rl::sigmoid_exact(v);
    }
    __syncthreads();
    // ---- composite, loss terms and their gradient: one ray per wave
    composite_tile(a, ws, rs, lds + L_DSIG, lds + L_DRGB, r0, nrays, S, lane, wv, l_d, l_c, l_o);
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
      *reinterpret_cast<f4*>(lds + L_D + dix(4, s, 4 * og)) = ov;
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
          const f4 da = ld4(lds + L_D + dix(l, ss, 8 * jg)), db = ld4(lds + L_D + dix(l, ss, 8 * jg + 4));
#pragma unroll
          for (int j = 0; j < 4; ++j) { acc[i][j] = fmaf(x, da[j], acc[i][j]); acc[i][4 + j] = fmaf(x, db[j], acc[i][4 + j]); }
        }
      }
    }
    if (bias_e >= 0) {
      const int l = bias_e >> 5, j = bias_e & 31;
      for (int ss = 0; ss < ns; ++ss) acc_bias += lds[L_D + dix(l, ss, j)];
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

  // ---- loss values, flags and the step state
  stage_losses(lds + L_RED, l_d, l_c, l_o, lane, wv);
  __syncthreads();
  if (tid == 0) {
    const StepLoss sl = finish_losses(lds + L_RED, rs);
    a.losses[o] = sl.d; a.losses[a.N + o] = sl.c; a.losses[2 * a.N + o] = sl.o;
    a.flags[o] = sl.flag;
    advance_state(st, cursor, rng_step, opt_step, epoch, R, rows_o);
  }

  // ---- AdamW by each gradient element's owner (torch.optim.AdamW)
  float step_size, inv_bc2_sqrt;
  adam_coefficients(a, opt_step + 1, step_size, inv_bc2_sqrt);
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
  copy_test_outputs(a, ws, o, tid);
}

cnr::DeviceOnce g_lds_once;
}  // namespace

extern "C" int cnr_obj_param_count(void) { return NPARAM; }

static_assert(cnr_obj::E_ARG == CNR_E_ARG, "obj_args.h");
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
  return launch(g_lds_once, obj_train_kernel, LDS_BYTES, N, stream, a);
}
