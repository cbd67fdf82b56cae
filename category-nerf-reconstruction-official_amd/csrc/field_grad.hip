// Field gradients: sigma = the x10 occupancy logit of a field and d sigma / d x at N points, for one
// CodeNeRF category (cnr_field_grad; geometry branch only, src/model.py:56-75) and for an OccupancyMap of hidden size 32 or 128
// (cnr_occmap_grad; src/model.py:129-147).
//
// Forward mode, exact fp32 on the vector unit.  A workgroup takes tiles of TP = 32 points.  Every activation travels as a float4
// (value, d/dx, d/dy, d/dz); a layer is  pre = W (value, tangents) + (b, 0, 0, 0),  out = pre.value > 0 ? pre : 0  (ReLU'(0) = 0).
// The first 87 embedding features and their Jacobian rows (I / scale | pi 2^k cos(pi 2^k B_j . x / scale) B_j / scale) are formed
// once per tile with the accurate sinf / cosf and stay in LDS for the two layers that read them (the first and the cat layer).
//
// LDS per workgroup:  xe float4[87][TP] | act float4[H][TP] | wp float[KP][H + 4]   (64 KiB at H = 32, 124 KiB at H = 128).
// The weights of every layer stream through `wp` in panels of KP = 32 input columns, transposed on the way in so that a thread
// reads the RPT output rows it owns as float4s; the next panel is fetched into registers while the current one is multiplied.
// A thread owns one point and RPT consecutive output rows: per input column one float4 of the point and RPT / 4 float4s of
// weights feed 4 RPT fused multiply-adds.  The layer's outputs wait in registers until every thread has finished reading `act`,
// then replace it: one activation buffer, no stash.
//
// A point's arithmetic does not depend on its tile, the grid or its neighbours (fixed summation order over the input columns,
// no atomics): every output is the same bit for bit from run to run and for any split of the points into calls.
#include "cnr_common.h"

namespace {

constexpr float PI_F = 3.14159265358979323846f;
constexpr int TP = 32;   // points per tile
constexpr int KP = 32;   // input columns per weight panel

// The value and d/dx, and d/dy and d/dz, travel as two packed pairs: one v_pk_fma_f32 does two of a weight's four multiply-adds
// (each half an IEEE fma: the same bits as four scalar fmaf; 9 .. 14 % less time at 816 000 points.  The Makefile's note against
// packed fp32 is about kernels that run them beside MFMAs; there are none here).
typedef float f2 __attribute__((ext_vector_type(2)));
struct Acc { f2 lo, hi; };        // (value, d/dx), (d/dy, d/dz)

template <int H, int RPT>
struct Tile {
  static_assert(RPT % 4 == 0 && H % RPT == 0, "a thread reads its rows as float4s");
  static constexpr int THREADS = TP * H / RPT;
  static constexpr int WLD = H + 4;                       // panel row stride (floats): 16-byte aligned rows, 4-way store conflicts
  static constexpr int NW = KP * H / THREADS;             // panel elements a thread stages
  static constexpr int LDS_BYTES = (cnr::E1 * TP + H * TP) * 16 + KP * WLD * 4;
  static_assert(KP * H % THREADS == 0, "whole panel elements per thread");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};

// acc += W[:, 0 .. K) X, W row-major with leading dimension ld (Wg points at the first column taken), X float4[K][TP] in LDS
template <int H, int RPT>
__device__ __forceinline__ void gemm_seg(const float* __restrict__ Wg, int ld, int K, const float4* __restrict__ X,
                                         float* __restrict__ wp, Acc (&acc)[RPT], int pt, int r0) {
  using T = Tile<H, RPT>;
  const int tid = threadIdx.x;
  float wr[T::NW];
#pragma unroll
  for (int i = 0; i < T::NW; ++i) {
    const int idx = tid + i * T::THREADS, kk = idx % KP, o = idx / KP;
    wr[i] = kk < K ? Wg[(int64_t)o * ld + kk] : 0.0f;
  }
  for (int k0 = 0; k0 < K; k0 += KP) {
    __syncthreads();                                      // the previous panel (and whatever else lived in LDS) has been read
#pragma unroll
    for (int i = 0; i < T::NW; ++i) {
      const int idx = tid + i * T::THREADS, kk = idx % KP, o = idx / KP;
      wp[kk * T::WLD + o] = wr[i];
    }
    __syncthreads();
    if (k0 + KP < K) {
#pragma unroll
      for (int i = 0; i < T::NW; ++i) {
        const int idx = tid + i * T::THREADS, k = k0 + KP + idx % KP, o = idx / KP;
        wr[i] = k < K ? Wg[(int64_t)o * ld + k] : 0.0f;
      }
    }
    const int kmax = min(KP, K - k0);
#pragma unroll 4
    for (int kk = 0; kk < kmax; ++kk) {
      const float4 x = X[(k0 + kk) * TP + pt];
      const f2 xl = {x.x, x.y}, xh = {x.z, x.w};
      const float4* wrow = reinterpret_cast<const float4*>(wp + kk * T::WLD + r0);
#pragma unroll
      for (int q = 0; q < RPT / 4; ++q) {
        const float4 w4 = wrow[q];
        const float w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const f2 w2 = {w[r], w[r]};
          acc[q * 4 + r].lo = __builtin_elementwise_fma(w2, xl, acc[q * 4 + r].lo);
          acc[q * 4 + r].hi = __builtin_elementwise_fma(w2, xh, acc[q * 4 + r].hi);
        }
      }
    }
  }
}

// bias (H floats in global memory, this point's) on the value, the ReLU mask on all four, then the outputs replace `act`
template <int H, int RPT>
__device__ __forceinline__ void finish(Acc (&acc)[RPT], const float* __restrict__ bias, bool relu, float4* __restrict__ act,
                                       int pt, int r0) {
#pragma unroll
  for (int r = 0; r < RPT; ++r) {
    acc[r].lo.x += bias[r0 + r];
    if (relu && !(acc[r].lo.x > 0.0f)) acc[r].lo = acc[r].hi = f2{0.f, 0.f};
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < RPT; ++r) {
    act[(r0 + r) * TP + pt] = make_float4(acc[r].lo.x, acc[r].lo.y, acc[r].hi.x, acc[r].hi.y);
    acc[r].lo = acc[r].hi = f2{0.f, 0.f};
  }
  __syncthreads();
}

// CAT: theta = the trunk blob, latent layers as bias rows; else theta = OccupancyMap(H) parameters in module order
template <int H, int RPT, bool CAT>
__global__ __launch_bounds__((Tile<H, RPT>::THREADS)) void grad_kernel(const float* __restrict__ pts, const int* __restrict__ row,
                                                                     const float* __restrict__ B, const float* __restrict__ theta,
                                                                     const float* __restrict__ biasrows, float scale, int64_t N,
                                                                     float* __restrict__ sigma, float* __restrict__ grad) {
  using T = Tile<H, RPT>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* xe = reinterpret_cast<float4*>(smem);
  float4* act = xe + cnr::E1 * TP;
  float* wp = reinterpret_cast<float*>(act + H * TP);
  const int tid = threadIdx.x, pt = tid % TP, r0 = (tid / TP) * RPT;
  const int64_t ntiles = (N + TP - 1) / TP;
  const float inv = 1.0f / scale;
  // layer offsets inside theta (floats)
  constexpr int W0 = CAT ? cnr::OFF_XYZ_W : 0, B0 = CAT ? cnr::OFF_XYZ_B : 87 * H;
  constexpr int W1 = CAT ? cnr::OFF_S1_W : 88 * H, B1 = 88 * H + H * H;
  constexpr int WC = CAT ? cnr::OFF_CAT_W : 89 * H + H * H, BC = 176 * H + 2 * H * H;
  constexpr int W2 = CAT ? cnr::OFF_S2_W : 177 * H + 2 * H * H, B2 = 177 * H + 3 * H * H;
  constexpr int WH = CAT ? cnr::OFF_SG_W : 178 * H + 3 * H * H, BH = CAT ? cnr::OFF_SG_B : 179 * H + 3 * H * H;
  Acc acc[RPT];
#pragma unroll
  for (int r = 0; r < RPT; ++r) acc[r].lo = acc[r].hi = f2{0.f, 0.f};

  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t n = tile * TP + pt;
    const bool live = n < N;
    __syncthreads();                                      // the previous tile's head has read act
    // ---- the 87 features and their Jacobian rows: item = (direction j or the identity block, point)
    // (one item per feature with sincosf, 87 x 32 of them, measured SLOWER: 1.58 -> 1.80 ms at 816 000 points for the category)
    for (int item = tid; item < TP * (CNR_NDIR + 1); item += T::THREADS) {
      const int p = item % TP, j = item / TP;
      const int64_t np = tile * TP + p;
      float t[3] = {0.f, 0.f, 0.f};
      if (np < N) { t[0] = pts[np * 3 + 0] / scale; t[1] = pts[np * 3 + 1] / scale; t[2] = pts[np * 3 + 2] / scale; }
      if (j == CNR_NDIR) {
        xe[0 * TP + p] = make_float4(t[0], inv, 0.f, 0.f);
        xe[1 * TP + p] = make_float4(t[1], 0.f, inv, 0.f);
        xe[2 * TP + p] = make_float4(t[2], 0.f, 0.f, inv);
      } else {
        const float b0 = B[j * 3 + 0], b1 = B[j * 3 + 1], b2 = B[j * 3 + 2];
        const float pr = t[0] * b0 + t[1] * b1 + t[2] * b2;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float fk = (float)(1 << k);
          const float a = (pr * fk) * PI_F;
          const float c = cosf(a) * (fk * PI_F) * inv;
          xe[(3 + CNR_NDIR * k + j) * TP + p] = make_float4(sinf(a), c * b0, c * b1, c * b2);
        }
      }
    }
    // (gemm_seg's first barrier orders these stores before the first read)
    const float* brow = nullptr;
    if (CAT) brow = biasrows + (int64_t)((row && live) ? row[n] : 0) * (CNR_NLAT * 32);

    // the layers as a run-time loop over segments (one copy of the product code; nothing of a layer's addressing is kept
    // alive across the others): {weight offset, leading dimension, columns, from xe?, 0 go on / 1 ReLU / 2 linear, bias offset
    // in theta or -1 - slot of the bias row}
#pragma unroll 1
    for (int l = 0; l < (CAT ? 6 : 5); ++l) {
      int w_off, ld, K, from_xe, fin, b_off;
      switch (l) {
        case 0: w_off = W0; ld = 87; K = 87; from_xe = 1; fin = 1; b_off = B0; break;
        case 1: w_off = W1; ld = H; K = H; from_xe = 0; fin = 1; b_off = CAT ? -1 : B1; break;
        case 2: w_off = WC; ld = H + 87; K = H; from_xe = 0; fin = 0; b_off = 0; break;
        case 3: w_off = WC + H; ld = H + 87; K = 87; from_xe = 1; fin = 1; b_off = CAT ? -2 : BC; break;
        case 4: w_off = W2; ld = H; K = H; from_xe = 0; fin = 1; b_off = CAT ? -3 : B2; break;
        default: w_off = cnr::OFF_ES_W; ld = H; K = H; from_xe = 0; fin = 2; b_off = cnr::OFF_ES_B; break;   // encoding_shape
      }
      gemm_seg<H, RPT>(theta + w_off, ld, K, from_xe ? xe : act, wp, acc, pt, r0);
      if (fin) finish<H, RPT>(acc, b_off < 0 ? brow + (-1 - b_off) * 32 : theta + b_off, fin == 1, act, pt, r0);
    }
    // ---- the head: H -> 1, times 10; thread = (point, channel)
    if (tid < TP * 4) {
      const int p = tid >> 2, c = tid & 3;
      const int64_t np = tile * TP + p;
      const float* a = reinterpret_cast<const float*>(act);
      float s = 0.0f;
      for (int o = 0; o < H; ++o) s = fmaf(theta[WH + o], a[(o * TP + p) * 4 + c], s);
      if (np < N) {
        if (c == 0) { if (sigma) sigma[np] = (s + theta[BH]) * 10.0f; }
        else grad[np * 3 + (c - 1)] = s * 10.0f;
      }
    }
  }
}

template <int H, int RPT, bool CAT>
int launch(const float* pts, const int* row, const float* B, const float* theta, const float* biasrows, float scale, int64_t N,
           float* sigma, float* grad, void* stream) {
  using T = Tile<H, RPT>;
  static cnr::DeviceOnce once;
  const int rc = cnr::set_max_dynamic_lds(once, reinterpret_cast<const void*>(&grad_kernel<H, RPT, CAT>), T::LDS_BYTES);
  if (rc) return rc;
  const int64_t ntiles = (N + TP - 1) / TP;
  const unsigned blocks = (unsigned)(ntiles < 4096 ? ntiles : 4096);
  hipLaunchKernelGGL((grad_kernel<H, RPT, CAT>), dim3(blocks), dim3(T::THREADS), T::LDS_BYTES, (hipStream_t)stream, pts, row, B,
                     theta, biasrows, scale, N, sigma, grad);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

}  // namespace

extern "C" int cnr_field_grad(const float* pts, const int* row, const float* B, const float* trunk, const float* biasrows,
                              float scale, int64_t N, float* sigma, float* grad, void* stream) {
  if (N < 0 || !(scale != 0.0f)) return CNR_E_ARG;
  if (N == 0) return CNR_OK;
  if (!pts || !B || !trunk || !biasrows || !grad) return CNR_E_ARG;
  return launch<32, 4, true>(pts, row, B, trunk, biasrows, scale, N, sigma, grad, stream);
}

extern "C" int cnr_occmap_grad(const float* pts, const float* theta, const float* B, int H, float scale, int64_t N, float* sigma,
                               float* grad, void* stream) {
  if (N < 0 || !(scale != 0.0f)) return CNR_E_ARG;
  if (H != 32 && H != 128) return CNR_E_SHAPE;
  if (N == 0) return CNR_OK;
  if (!pts || !theta || !B || !grad) return CNR_E_ARG;
  if (H == 32) return launch<32, 4, false>(pts, nullptr, B, theta, nullptr, scale, N, sigma, grad, stream);
  return launch<128, 8, false>(pts, nullptr, B, theta, nullptr, scale, N, sigma, grad, stream);
}
