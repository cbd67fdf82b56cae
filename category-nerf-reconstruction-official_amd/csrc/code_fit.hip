// cnr_code_fit: one launch = one optimisation step of EVERY candidate of a code fit.  A candidate is one (instance, starting
// code) pair: a shape code and a texture code of a FROZEN CodeNeRF category (src/model.py:23-84), fitted to the instance's own ray
// pool by the reference's object step with a one-object class (train.py:123-167, src/loss.py:5-74) and the network held fixed.
// Candidates share nothing they write, so ONE WORKGROUP owns one candidate for the whole step, on the step skeleton it shares with
// cnr_obj_train (pool_step_common.h): rows -> rays -> latent layers -> PE -> trunk -> composite + losses -> backward to the four latent outputs ->
// latent layers backward -> regulariser -> AdamW on the two codes.  No cross-workgroup reduction, no wait across workgroups and no
// float atomic: every sum has one owner and a fixed order, so two runs give the same bits and a candidate's result does not depend
// on what else is in the launch.
//
// Frozen weights make the backward short: no weight-gradient product, no PE backward, no gradient record.  It runs only down the
// 32-wide activation path and collects, per candidate, the four 32-vectors d z_k (the gradients of the latent layers' outputs,
// which enter the trunk as x_k = a_k + z_k: d z_k = the sum over all samples of d x_k); a (4 x 32 x L) transposed mat-vec takes
// those to the two codes.
//
// Arithmetic: exact fp32 on the vector unit (fused multiply-adds, fp32 accumulation).  The trunk's seven 32-wide matrices sit
// TRANSPOSED in LDS for the whole step (the same image serves the forward, by columns, and the backward, by rows), the activations
// of one tile of whole rays beside them; the latent matrices (4 x 32 x L: 131 KB at L = 256) do not fit and are read from global
// memory, once for the latent forward and once for the code gradient.  (DESIGN.md 3.14 has the LDS map.)
#include "pool_step_common.h"

namespace {
using namespace cnr;
using namespace cnr_pool_step;      // the step skeleton shared with cnr_obj_train: THREADS, WAVES, TS, H, NDIR and the steps
constexpr int H2 = 16;
// rows of the transposed weight image WT[q][32]: WT[Q_l + k][j] = W_l[j][k] for the seven 32-wide layers
constexpr int Q_XYZ = 0, Q_S1 = Q_XYZ + E1, Q_CAT = Q_S1 + H, Q_S2 = Q_CAT + H + E1, Q_ES = Q_S2 + H, Q_VD = Q_ES + H,
              Q_T1 = Q_VD + H + E2, QN = Q_T1 + H;
static_assert(QN == 408, "weight rows");
// columns of the activation image ACT[sample][AW]: PE features (e1 | e2), then the post-ReLU outputs a_l of the layers (the latent
// rows z_k are added when the next layer reads them, so that a_l > 0 stays the layer's ReLU mask).  Column block A_P holds
// encoding_xyz's output until shape_layer_1 has read it, then encoding_shape's (which has no ReLU and no mask to keep).
constexpr int A_E = 0, A_E2 = E1, A_P = E1 + E2, A_A1 = A_P + H, A_A2 = A_A1 + H, A_A3 = A_A2 + H, A_A5 = A_A3 + H, A_A6 = A_A5 + H,
              A_A7 = A_A6 + H, AW = A_A7 + H2;
static_assert((AW & 1) == 1, "odd row stride: a column over samples and a row over columns are both bank-conflict free");
// small parameters SP[]: seven biases, rgb.0's bias, sigma.0, rgb.2, B, a zero row, the latent outputs z (4,32), the masked d z
constexpr int SP_BIAS = 0, SP_R0_B = 7 * H, SP_SG_W = SP_R0_B + H2, SP_SG_B = SP_SG_W + H, SP_R2_W = SP_SG_B + 1, SP_R2_B = SP_R2_W + 3 * H2,
              SP_B = SP_R2_B + 3, SP_ZERO = (SP_B + NDIR * 3 + 3) & ~3, SP_ZL = SP_ZERO + H, SP_DZ = SP_ZL + 4 * H, SP_NORM = SP_DZ + 4 * H,
              SP_N = SP_NORM + 4;
enum { B_XYZ = 0, B_S1, B_CAT, B_S2, B_ES, B_VD, B_T1 };
// LDS (floats): WT | R0T (rgb.0 transposed, [32][16]) | ACT | D (two buffers of 64 samples x 32, swizzled) | SP | DSIG | DRGB | RED
constexpr int L_WT = 0, L_R0T = L_WT + QN * H, L_ACT = L_R0T + H * H2, L_D = L_ACT + TS * AW, L_SP = L_D + 2 * TS * H, L_DSIG = L_SP + SP_N,
              L_DRGB = L_DSIG + TS, L_RED = L_DRGB + TS * 3, L_END = L_RED + 64;
constexpr int LDS_BYTES = L_END * 4;
static_assert((L_R0T & 3) == 0 && (L_D & 3) == 0 && (L_SP & 3) == 0, "16-byte accesses");
static_assert(LDS_BYTES <= 160 * 1024, "one workgroup per CU: 160 KB of LDS");

struct FitArgs : StepArgs {
  const float* theta; int64_t class_stride, off_trunk, off_latW, off_latb, off_B; int n_nets, L;
  const int* pool_ids; const int* pool_world_frame; int P;
  const int* cand_net; const int* cand_pool; int K; float* codes; int update; float reg_scaling;
};

// one 32-wide layer for sample s, outputs 4 og .. 4 og + 3: inputs are ACT columns colA .. colA + nA - 1 PLUS the row zrow[0 .. nA)
// (a latent row, or the zero row: nA <= 32), then ACT columns colB .. colB + nB - 1 (weight rows q0 ..); the result, after a ReLU when `relu`,
// goes to ACT columns out ..
__device__ __forceinline__ void layer_fwd(float* __restrict__ lds, int s, int og, int q0, int bias, int colA, int nA, int zrow, int colB,
                                          int nB, int out, bool relu) {
  const float* x = lds + L_ACT + s * AW;
  const float* w = lds + L_WT + q0 * H + 4 * og;
  const float* zr = lds + L_SP + zrow;
  f4 acc = ld4(lds + L_SP + SP_BIAS + bias * H + 4 * og);
  for (int k = 0; k < nA; ++k) {
    const float xv = x[colA + k] + zr[k];
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
  for (int i = 0; i < 4; ++i) y[i] = relu ? fmaxf(acc[i], 0.f) : acc[i];
}
// backward through one layer's first 32 input columns: d x[j] = sum_j' D[src][s][j'] W[j'][j] for j = 4 og .. 4 og + 3 (W[.][j] is
// row q0 + j of the transposed image)
__device__ __forceinline__ f4 layer_bwd(const float* __restrict__ lds, int s, int og, int src, int q0) {
  f4 drow[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) drow[i] = ld4(lds + L_D + dix(src, s, 4 * i));
  f4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float* w = lds + L_WT + (q0 + 4 * og + i) * H;
    float a = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t) a = dot4(drow[t], ld4(w + 4 * t), a);
    o[i] = a;
  }
  return o;
}
// v where ACT column col + 4 og + i of sample s is positive (the ReLU mask of that layer), else 0
__device__ __forceinline__ f4 relu_mask(const float* __restrict__ lds, int s, int og, int col, f4 v) {
  const float* a = lds + L_ACT + s * AW + col + 4 * og;
  return f4{a[0] > 0.f ? v[0] : 0.f, a[1] > 0.f ? v[1] : 0.f, a[2] > 0.f ? v[2] : 0.f, a[3] > 0.f ? v[3] : 0.f};
}
__device__ __forceinline__ void st4(float* __restrict__ lds, int b, int s, int og, f4 v) {
  *reinterpret_cast<f4*>(lds + L_D + dix(b, s, 4 * og)) = v;
}

__global__ __launch_bounds__(THREADS) void code_fit_kernel(FitArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int s = lane, og = wv;                       // the per-sample phases: thread = (sample, 4 outputs)
  const int K = a.K, R = a.R, S = a.n1 + a.n2, L = a.L;
  const int net = a.cand_net[c], pool = a.cand_pool[c];
  // a candidate that names no network or no pool, or a pool shorter than a step, is skipped: nothing of it is read
  int skip = 0;
  int64_t seg0 = 0, rows_o = 0;
  if (net < 0 || net >= a.n_nets || pool < 0 || pool >= a.P) skip = 64;
  else {
    seg0 = a.pool_off[pool]; rows_o = a.pool_off[pool + 1] - seg0;
    if (rows_o < R) skip = 16;
  }
  if (skip) {
    if (tid == 0) a.flags[c] = skip;
    if (tid < 5) a.losses[tid * K + c] = 0.f;
    return;
  }
  int64_t* st = a.d_state + (size_t)c * 4;
  const int64_t cursor = st[0], rng_step = st[1], opt_step = st[2], epoch = st[3];
  const uint64_t gid = (uint64_t)(a.pool_ids ? a.pool_ids[pool] : pool);     // rows and draws follow the POOL, not the candidate
  const float* th = a.theta + (size_t)net * a.class_stride;
  const float* trunk = th + a.off_trunk;
  const float* latW = th + a.off_latW;
  const float* latb = th + a.off_latb;
  float* code = a.codes + (size_t)c * 2 * L;            // shape code, then texture code
  const Workspace ws = cnr_obj::carve(a.ws + (size_t)c * a.ws_stride, R, S);

  // ---- the frozen trunk into LDS: transposed weights, small parameters ------------------------------------------------------
  for (int i = tid; i < QN * H; i += THREADS) {
    const int q = i >> 5, j = i & 31;
    int off, k, kin;
    if (q < Q_S1) { off = OFF_XYZ_W; k = q; kin = E1; }
    else if (q < Q_CAT) { off = OFF_S1_W; k = q - Q_S1; kin = H; }
    else if (q < Q_S2) { off = OFF_CAT_W; k = q - Q_CAT; kin = H + E1; }
    else if (q < Q_ES) { off = OFF_S2_W; k = q - Q_S2; kin = H; }
    else if (q < Q_VD) { off = OFF_ES_W; k = q - Q_ES; kin = H; }
    else if (q < Q_T1) { off = OFF_VD_W; k = q - Q_VD; kin = H + E2; }
    else { off = OFF_T1_W; k = q - Q_T1; kin = H; }
    lds[L_WT + i] = trunk[off + j * kin + k];
  }
  for (int i = tid; i < H * H2; i += THREADS) lds[L_R0T + i] = trunk[OFF_R0_W + (i & 15) * H + (i >> 4)];     // R0T[k][j] = W[j][k]
  for (int i = tid; i < 7 * H; i += THREADS) {
    const int l = i >> 5;
    const int off = l == B_XYZ ? OFF_XYZ_B : l == B_S1 ? OFF_S1_B : l == B_CAT ? OFF_CAT_B : l == B_S2 ? OFF_S2_B : l == B_ES ? OFF_ES_B
                    : l == B_VD ? OFF_VD_B : OFF_T1_B;
    lds[L_SP + SP_BIAS + i] = trunk[off + (i & 31)];
  }
  for (int i = tid; i < H2; i += THREADS) lds[L_SP + SP_R0_B + i] = trunk[OFF_R0_B + i];
  for (int i = tid; i < H + 1; i += THREADS) lds[L_SP + SP_SG_W + i] = trunk[OFF_SG_W + i];
  for (int i = tid; i < 3 * H2 + 3; i += THREADS) lds[L_SP + SP_R2_W + i] = trunk[OFF_R2_W + i];
  for (int i = tid; i < NDIR * 3; i += THREADS) lds[L_SP + SP_B + i] = th[a.off_B + i];
  for (int i = tid; i < H; i += THREADS) lds[L_SP + SP_ZERO + i] = 0.f;

  // ---- latent layers (a7): z_k = relu(W_k code + b_k), k = 0 .. 2 on the shape code, 3 on the texture code; one output per wave
  // at a time, the lanes along the code, a butterfly sum -- and the two code norms the same way
  for (int o = wv * (4 * H / WAVES); o < (wv + 1) * (4 * H / WAVES); ++o) {
    const float* w = latW + (size_t)o * L;
    const float* cd = code + (o >= 3 * H ? L : 0);
    float acc = 0.f;
    for (int l = lane; l < L; l += 64) acc = fmaf(w[l], cd[l], acc);
    acc = wave_sum(acc);
    if (lane == 0) lds[L_SP + SP_ZL + o] = fmaxf(acc + latb[o], 0.f);
  }
  if (wv < 2) {
    const float* cd = code + wv * L;
    float ss = 0.f;
    for (int l = lane; l < L; l += 64) ss = fmaf(cd[l], cd[l], ss);
    ss = wave_sum(ss);
    if (lane == 0) lds[L_SP + SP_NORM + wv] = sqrtf(ss);
  }

  // ---- rows of the step, their max depth and mask counts; a2-a5, one wave per ray, in the pool's frame --------------------
  const RowStats rs = select_rows(a, lds + L_RED, ws, c, seg0, rows_o, gid, cursor, epoch, tid, lane, wv);
  sample_rays(a, ws, c, seg0, a.pool_world_frame ? (a.pool_world_frame[pool] != 0) : 0, gid, rng_step, rs.mb, lane, wv);
  __syncthreads();

  // d z_k[4 og + i] of this thread's samples (summed over the wave's lanes at the end); this wave's rays' loss terms
  float dz[4][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  float l_d = 0.f, l_c = 0.f, l_o = 0.f;

  const int G = TS / S;                                  // whole rays per tile
  for (int r0 = 0; r0 < R; r0 += G) {
    const int nrays = min(G, R - r0), ns = nrays * S;
    const size_t m0 = (size_t)r0 * S;                    // first sample of the tile
    const bool on = s < ns;
    float t0, t1, t2;
    pe_forward(lds + L_ACT + s * AW, lds + L_SP + SP_B, on, ws.pts, m0 + s, a.scale, og, t0, t1, t2);
    __syncthreads();
    // ---- forward (src/model.py:56-84)
    layer_fwd(lds, s, og, Q_XYZ, B_XYZ, 0, 0, SP_ZERO, A_E, E1, A_P, true);               // encoding_xyz
    __syncthreads();
    layer_fwd(lds, s, og, Q_S1, B_S1, A_P, H, SP_ZL + 0 * H, 0, 0, A_A1, true);           // shape_layer_1 on a0 + z0
    __syncthreads();
    layer_fwd(lds, s, og, Q_CAT, B_CAT, A_A1, H, SP_ZL + 1 * H, A_E, E1, A_A2, true);     // cat_layer on (a1 + z1 | e1)
    __syncthreads();
    layer_fwd(lds, s, og, Q_S2, B_S2, A_A2, H, SP_ZL + 2 * H, 0, 0, A_A3, true);          // shape_layer_2 on a2 + z2
    __syncthreads();
    layer_fwd(lds, s, og, Q_ES, B_ES, A_A3, H, SP_ZERO, 0, 0, A_P, false);                // encoding_shape (no ReLU)
    __syncthreads();
    layer_fwd(lds, s, og, Q_VD, B_VD, A_P, H, SP_ZERO, A_E2, E2, A_A5, true);             // encoding_viewdir on (y4 | e2)
    __syncthreads();
    layer_fwd(lds, s, og, Q_T1, B_T1, A_A5, H, SP_ZL + 3 * H, 0, 0, A_A6, true);          // texture_layer_1 on a5 + z3
    __syncthreads();
    if (og < 4) {                // rgb.0: 16 outputs
      const float* x = lds + L_ACT + s * AW + A_A6;
      f4 acc = ld4(lds + L_SP + SP_R0_B + 4 * og);
      for (int k = 0; k < H; ++k) {
        const float xv = x[k];
        const f4 wv4 = ld4(lds + L_R0T + k * H2 + 4 * og);
        acc[0] = fmaf(xv, wv4[0], acc[0]); acc[1] = fmaf(xv, wv4[1], acc[1]); acc[2] = fmaf(xv, wv4[2], acc[2]); acc[3] = fmaf(xv, wv4[3], acc[3]);
      }
      float* y = lds + L_ACT + s * AW + A_A7 + 4 * og;
#pragma unroll
      for (int i = 0; i < 4; ++i) y[i] = fmaxf(acc[i], 0.f);
    }
    __syncthreads();
    if (og < 4 && on) {          // heads: wave 0 the x10 occupancy logit, waves 1..3 one colour channel each
      if (og == 0) {
        const float* x = lds + L_ACT + s * AW + A_P;
        float v = lds[L_SP + SP_SG_B];
        for (int j = 0; j < H; ++j) v = fmaf(x[j], lds[L_SP + SP_SG_W + j], v);
        ws.sig[m0 + s] = v * 10.0f;
      } else {
        const float* x = lds + L_ACT + s * AW + A_A7;
        const float* w = lds + L_SP + SP_R2_W + (og - 1) * H2;
        float v = lds[L_SP + SP_R2_B + og - 1];
        for (int j = 0; j < H2; ++j) v = fmaf(x[j], w[j], v);
        ws.rgb[(m0 + s) * 3 + og - 1] = cnr_rl::sigmoid_exact(v);
      }
    }
    __syncthreads();
    // ---- composite, loss terms and their gradient: one ray per wave
    composite_tile(a, ws, rs, lds + L_DSIG, lds + L_DRGB, r0, nrays, S, lane, wv, l_d, l_c, l_o);
    __syncthreads();
    // ---- backward, down the activation path only: rgb.2 -> rgb.0 -> texture_layer_1 (d z3) -> encoding_viewdir + sigma.0 ->
    // encoding_shape -> shape_layer_2 (d z2) -> cat_layer (d z1) -> shape_layer_1 (d z0).  The buffers D0 / D1 alternate.
    if (on && og < 4) {
      const float d0 = lds[L_DRGB + s * 3 + 0], d1 = lds[L_DRGB + s * 3 + 1], d2 = lds[L_DRGB + s * 3 + 2];
      f4 v;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = 4 * og + i;
        v[i] = d0 * lds[L_SP + SP_R2_W + j] + d1 * lds[L_SP + SP_R2_W + H2 + j] + d2 * lds[L_SP + SP_R2_W + 2 * H2 + j];
      }
      st4(lds, 0, s, og, relu_mask(lds, s, og, A_A7, v));
    }
    __syncthreads();
    if (on) {                    // rgb.0 backward: d a6[j] = sum_{j' < 16} d a7[j'] W[j'][j], W[.][j] = row j of R0T
      f4 drow[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) drow[i] = ld4(lds + L_D + dix(0, s, 4 * i));
      f4 v;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float* w = lds + L_R0T + (4 * og + i) * H2;
        float acc = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) acc = dot4(drow[t], ld4(w + 4 * t), acc);
        v[i] = acc;
      }
      st4(lds, 1, s, og, relu_mask(lds, s, og, A_A6, v));
    }
    __syncthreads();
    if (on) {
      const f4 v = layer_bwd(lds, s, og, 1, Q_T1);                  // d x6 = d (a5 + z3)
#pragma unroll
      for (int i = 0; i < 4; ++i) dz[3][i] += v[i];
      st4(lds, 0, s, og, relu_mask(lds, s, og, A_A5, v));
    }
    __syncthreads();
    if (on) {
      f4 v = layer_bwd(lds, s, og, 0, Q_VD);                        // d y4, + the occupancy head's share
      const float da = lds[L_DSIG + s];
      const f4 sg = ld4(lds + L_SP + SP_SG_W + 4 * og);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = fmaf(da, sg[i], v[i]);
      st4(lds, 1, s, og, v);
    }
    __syncthreads();
    if (on) st4(lds, 0, s, og, relu_mask(lds, s, og, A_A3, layer_bwd(lds, s, og, 1, Q_ES)));
    __syncthreads();
    if (on) {
      const f4 v = layer_bwd(lds, s, og, 0, Q_S2);                  // d x3 = d (a2 + z2)
#pragma unroll
      for (int i = 0; i < 4; ++i) dz[2][i] += v[i];
      st4(lds, 1, s, og, relu_mask(lds, s, og, A_A2, v));
    }
    __syncthreads();
    if (on) {
      const f4 v = layer_bwd(lds, s, og, 1, Q_CAT);                 // d x2 = d (a1 + z1)
#pragma unroll
      for (int i = 0; i < 4; ++i) dz[1][i] += v[i];
      st4(lds, 0, s, og, relu_mask(lds, s, og, A_A1, v));
    }
    __syncthreads();
    if (on) {
      const f4 v = layer_bwd(lds, s, og, 0, Q_S1);                  // d x1 = d (a0 + z0)
#pragma unroll
      for (int i = 0; i < 4; ++i) dz[0][i] += v[i];
    }
    __syncthreads();
  }

  // ---- d z_k over all samples (a butterfly over the wave's lanes), through the latent layers' ReLU
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float v = wave_sum(dz[k][i]);
      const int j = k * H + 4 * og + i;
      if (lane == 0) lds[L_SP + SP_DZ + j] = lds[L_SP + SP_ZL + j] > 0.f ? v : 0.f;
    }
  stage_losses(lds + L_RED, l_d, l_c, l_o, lane, wv);
  __syncthreads();

  // ---- loss values, flags and the step state
  const float n_sh = lds[L_SP + SP_NORM + 0], n_tx = lds[L_SP + SP_NORM + 1];
  if (tid == 0) {
    const StepLoss sl = finish_losses(lds + L_RED, rs);
    a.losses[c] = sl.d; a.losses[K + c] = sl.c; a.losses[2 * K + c] = sl.o; a.losses[3 * K + c] = n_sh; a.losses[4 * K + c] = n_tx;
    a.flags[c] = sl.flag;
    if (a.update) advance_state(st, cursor, rng_step, opt_step, epoch, R, rows_o);
  }

  // ---- latent layers backward to the codes, the code-norm regulariser (src/loss.py:5-15; zero at a zero code, as torch's norm),
  // AdamW by each element's owner (torch.optim.AdamW)
  float step_size, inv_bc2_sqrt;
  adam_coefficients(a, opt_step + 1, step_size, inv_bc2_sqrt);
  for (int i = tid; i < 2 * L; i += THREADS) {
    const int tex = i >= L ? 1 : 0, l = i - tex * L;
    const int k0 = tex ? 3 : 0, k1 = tex ? 4 : 3;
    float gsum = 0.f;
    for (int j = k0 * H; j < k1 * H; ++j) gsum = fmaf(lds[L_SP + SP_DZ + j], latW[(size_t)j * L + l], gsum);
    const float cv = code[i], nrm = tex ? n_tx : n_sh;
    if (a.reg_scaling > 0.f && nrm > 0.f) gsum += a.reg_scaling * (cv / nrm);
    const size_t e = (size_t)c * 2 * L + i;
    if (a.grad) a.grad[e] = gsum;
    if (a.update) {
      const AdamElement n = adam_element(cv, a.exp_avg[e], a.exp_avg_sq[e], gsum, 1.0f - a.lr * a.wd, step_size, inv_bc2_sqrt, a.b1, a.b2,
                                         a.adam_eps);
      code[i] = n.p; a.exp_avg[e] = n.m; a.exp_avg_sq[e] = n.v;
    }
  }
  copy_test_outputs(a, ws, c, tid);
}

cnr::DeviceOnce g_lds_once;
}  // namespace

extern "C" int64_t cnr_code_fit_workspace_bytes(int K, int R, int S) { return cnr_obj::workspace_bytes(K, R, S); }

extern "C" int cnr_code_fit(const float* theta, int64_t class_stride, int64_t off_trunk, int64_t off_latW, int64_t off_latb,
                            int64_t off_B, int n_nets, int L, const uint8_t* rgbs, const float* depth, const float* dirs_c,
                            const float* T, const int64_t* pool_off, int64_t min_pool_rows, const int* pool_ids,
                            const int* pool_world_frame, int P, const int* cand_net, const int* cand_pool, int K, int R, int n1,
                            int n2, float eps, float stop_eps, float min_bound, float scale, uint64_t seed, const int* rows,
                            const float* u, const float* g, int64_t* d_state, float* codes, float* exp_avg, float* exp_avg_sq,
                            int update, float lr, float beta1, float beta2, float adam_eps, float weight_decay, float color_scaling,
                            float opacity_scaling, float reg_scaling, float* losses, int32_t* flags, float* grad, float* sigma,
                            float* rgb, float* z, int* rows_out, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!theta || !pool_world_frame || !cand_net || !cand_pool || !codes) return CNR_E_ARG;
  if (n_nets <= 0 || P <= 0 || class_stride <= 0 || off_trunk < 0 || off_latW < 0 || off_latb < 0 || off_B < 0) return CNR_E_ARG;
  const cnr_obj::Required req{rgbs, depth, dirs_c, T, pool_off, d_state, theta, exp_avg, exp_avg_sq, losses, flags, workspace};
  if (cnr_obj::check_args(req, min_pool_rows, K, R, n1, n2, scale, rows, u, g, workspace_bytes)) return CNR_E_ARG;
  if (L <= 0 || !(256 % L == 0 || L % 256 == 0)) return CNR_E_SHAPE;      // the code lengths the latent kernels accept
  // every block of a network's row ends inside the row: a wrong offset from a foreign layout is refused, not read
  if (off_trunk + cnr::TRUNK > class_stride || off_latW + 4 * (int64_t)H * L > class_stride || off_latb + 4 * H > class_stride ||
      off_B + NDIR * 3 > class_stride)
    return CNR_E_ARG;
  FitArgs a{};
  a.theta = theta; a.class_stride = class_stride; a.off_trunk = off_trunk; a.off_latW = off_latW; a.off_latb = off_latb; a.off_B = off_B;
  a.n_nets = n_nets; a.L = L; a.rgbs = rgbs; a.depth = depth; a.dirs_c = dirs_c; a.T = T; a.pool_off = pool_off; a.pool_ids = pool_ids;
  a.pool_world_frame = pool_world_frame; a.P = P; a.cand_net = cand_net; a.cand_pool = cand_pool; a.K = K; a.R = R; a.n1 = n1; a.n2 = n2;
  a.eps = eps; a.stop_eps = stop_eps; a.min_bound = min_bound; a.scale = scale; a.seed = seed; a.rows = rows; a.u = u; a.g = g;
  a.d_state = d_state; a.codes = codes; a.exp_avg = exp_avg; a.exp_avg_sq = exp_avg_sq; a.update = update; a.lr = lr; a.b1 = beta1;
  a.b2 = beta2; a.adam_eps = adam_eps; a.wd = weight_decay; a.color_scaling = color_scaling; a.opacity_scaling = opacity_scaling;
  a.reg_scaling = reg_scaling; a.losses = losses; a.flags = flags; a.grad = grad; a.sigma = sigma; a.rgb = rgb; a.z = z;
  a.rows_out = rows_out; a.ws = static_cast<uint32_t*>(workspace); a.ws_stride = cnr_obj::ws_words(R, n1 + n2);
  return launch(g_lds_once, code_fit_kernel, LDS_BYTES, K, stream, a);
}
