// Image-space view scores: per (image, row) the sums behind PSNR, SSIM, depth L1 and mask IoU of a
// reconstruction against a ground truth, one read of the images for everything.  include/cnr_hip.h has the definitions.
//
//   im_tile_kernel    one workgroup per (tile of IM_TW x IM_TH pixels, image).  The tile's rgb plus a 5-pixel halo of both
//                     images is staged in LDS as f32 planes (a u8 ground truth as the byte's value; it enters the arithmetic
//                     through a 256-entry table of v / 255.0 in double).  Per channel the 11-tap Gaussian runs along W into
//                     s_mid (five moments, double), then along H out of it; S of the three channels is averaged per pixel.
//                     se, the depth terms and the label rows of the thread's two pixels sit in registers meanwhile (depth
//                     and labels need no halo: they are read once, straight into them).  Afterwards the per-pixel values go
//                     to LDS (over s_mid) and wave w reduces the present rows w, w + 4, .. of the tile: lane l adds its
//                     pixels l, l + 64, .. in that order, a 32, 16, .., 1 butterfly adds the lanes, counts are ballots.  A
//                     row is present when a pixel of the tile has its id in label_gt or label_rec; row K always is.  The
//                     partial of every (tile, row) is written, zeros for the absent rows.
//   im_finish_kernel  one workgroup per (row, image): thread t adds the partials of tiles t, t + 256, .. in that order, a
//                     fixed tree adds the threads.
// No atomics of any kind: every sum is formed in an order that W, H and the tile shape fix.
//
// Contraction is off: the products of se are rounded on their own, the filter's multiply-adds are spelt fma().
#pragma clang fp contract(off)
#include "cnr_common.h"
#include "geom_common.h"

#include <math.h>

using namespace cnr;

namespace {
constexpr int IM_TW = CNR_IMG_TILE_W, IM_TH = CNR_IMG_TILE_H;          // output pixels of a tile along W and along H (the fast axis)
constexpr int IM_R = 5, IM_TAPS = 2 * IM_R + 1;
constexpr int IM_SW = IM_TW + 2 * IM_R, IM_SH = IM_TH + 2 * IM_R;      // staged: 26 x 42 = 1092 pixels
constexpr int IM_BLOCK = 256, IM_WAVES = IM_BLOCK / 64;
constexpr int IM_PIX = IM_TW * IM_TH;                                  // 512
constexpr int IM_PPT = IM_PIX / IM_BLOCK;                              // pixels per thread: 2
constexpr int IM_PPL = IM_PIX / 64;                                    // pixels per lane in the row reduction: 8
constexpr int IM_MAXK = 255;
constexpr int IM_NF = 3, IM_NI = 7;                                    // float sums and counts per (image, row)
constexpr double IM_C1 = 1e-4, IM_C2 = 9e-4;
static_assert(IM_PIX % IM_BLOCK == 0 && IM_TH == 32, "a thread's pixels are (t / 32 + 8 j, t % 32)");
// per-pixel values after the filter, over s_mid: 3 doubles and 3 ints per pixel
static_assert(IM_PIX * (IM_NF * 8 + 3 * 4) <= 5 * IM_TW * IM_SH * 8, "the per-pixel arrays must fit in s_mid");

enum : int { F_VALID = 1, F_SSIM = 2, F_BOTH = 4, F_ONLY_REC = 8, F_ONLY_GT = 16, F_EQ = 32 };

struct ImWeights {
  double g[IM_TAPS];
};

struct ImLayout {
  int64_t tw, th, tiles, off_i, bytes;
};
inline ImLayout im_layout(int64_t N, int64_t W, int64_t H, int64_t K) {
  ImLayout L;
  L.tw = (W + IM_TW - 1) / IM_TW;
  L.th = (H + IM_TH - 1) / IM_TH;
  L.tiles = L.tw * L.th;
  L.off_i = align256(N * (K + 1) * IM_NF * L.tiles * 8);
  L.bytes = L.off_i + align256(N * (K + 1) * IM_NI * L.tiles * 4);
  return L;
}

// the index of v in the ascending s_ids[0 .. K), -1 when it is not there
__device__ __forceinline__ int find_row(const int* s_ids, int K, int v) {
  int lo = 0, hi = K;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s_ids[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo < K && s_ids[lo] == v ? lo : -1;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <bool U8>
__global__ __launch_bounds__(IM_BLOCK) void im_tile_kernel(const float* __restrict__ rgb_rec, const void* __restrict__ rgb_gt,
                                                           const float* __restrict__ depth_rec,
                                                           const float* __restrict__ depth_gt,
                                                           const int* __restrict__ label_rec, const int* __restrict__ label_gt,
                                                           const int* __restrict__ ids, int K, int W, int H, int tiles_h,
                                                           int64_t tiles, ImWeights wt, float* __restrict__ ssim_map,
                                                           double* __restrict__ part_f, int* __restrict__ part_i) {
  __shared__ float s_a[3][IM_SW][IM_SH];                  // 13 104 B
  __shared__ float s_b[3][IM_SW][IM_SH];                  // 13 104 B
  __shared__ double s_mid[5 * IM_TW * IM_SH];             // 26 880 B: [moment][w][staged h]; later the per-pixel arrays
  __shared__ double s_tab[256];                           //  2 048 B: v / 255.0
  __shared__ int s_ids[IM_MAXK + 1];
  __shared__ int s_present[IM_MAXK + 1];
  __shared__ int s_list[IM_MAXK + 1];
  __shared__ int s_wave[IM_WAVES];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t tile = blockIdx.x, n = blockIdx.y;
  const int w0 = (int)(tile / tiles_h) * IM_TW, h0 = (int)(tile % tiles_h) * IM_TH;
  const int64_t img = n * W;                              // pixel (w, h) of image n: (img + w) * H + h

  if (U8) s_tab[t] = (double)t / 255.0;
  s_ids[t] = t < K ? ids[t] : 0;
  s_present[t] = 0;

  // ---- stage both rgb tiles with their halo; outside the image: 0 (such windows are never counted)
  for (int i = t; i < IM_SW * IM_SH; i += IM_BLOCK) {
    const int sw = i / IM_SH, sh = i % IM_SH;
    const int gw = w0 - IM_R + sw, gh = h0 - IM_R + sh;
    float a[3] = {0.f, 0.f, 0.f}, b[3] = {0.f, 0.f, 0.f};
    if (gw >= 0 && gw < W && gh >= 0 && gh < H) {
      const int64_t p = ((img + gw) * H + gh) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        a[c] = rgb_rec[p + c];
        b[c] = U8 ? (float)((const uint8_t*)rgb_gt)[p + c] : ((const float*)rgb_gt)[p + c];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      s_a[c][sw][sh] = a[c];
      s_b[c][sw][sh] = b[c];
    }
  }
  __syncthreads();

  // ---- the thread's pixels: se, depth terms, rows
  int flag[IM_PPT], row[IM_PPT], rrow[IM_PPT];
  double se[IM_PPT], dabs[IM_PPT], ss[IM_PPT];
#pragma unroll
  for (int j = 0; j < IM_PPT; ++j) {
    const int lw = (t >> 5) + (IM_TW / IM_PPT) * j, lh = t & 31;
    const int gw = w0 + lw, gh = h0 + lh;
    flag[j] = 0, row[j] = -1, rrow[j] = -1;
    se[j] = 0.0, dabs[j] = 0.0, ss[j] = 0.0;
    if (gw < W && gh < H) {
      flag[j] = F_VALID;
      if (gw >= IM_R && gw < W - IM_R && gh >= IM_R && gh < H - IM_R) flag[j] |= F_SSIM;
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double a = (double)s_a[c][lw + IM_R][lh + IM_R];
        const float bf = s_b[c][lw + IM_R][lh + IM_R];
        const double b = U8 ? s_tab[(int)bf] : (double)bf;
        const double d = a - b;
        s += d * d;
      }
      se[j] = s;
      const int64_t p = (img + gw) * H + gh;
      if (depth_rec) {
        const float dr = depth_rec[p], dg = depth_gt[p];
        const bool hr = dr > 0.f, hg = dg > 0.f;
        if (hr && hg) {
          flag[j] |= F_BOTH;
          dabs[j] = fabs((double)dr - (double)dg);
        } else if (hr) {
          flag[j] |= F_ONLY_REC;
        } else if (hg) {
          flag[j] |= F_ONLY_GT;
        }
      }
      if (label_rec) {
        const int lr = label_rec[p], lg = label_gt[p];
        if (lr == lg) flag[j] |= F_EQ;
        row[j] = find_row(s_ids, K, lg);
        rrow[j] = find_row(s_ids, K, lr);
        if (row[j] >= 0) s_present[row[j]] = 1;
        if (rrow[j] >= 0) s_present[rrow[j]] = 1;
      }
    }
  }

  // ---- SSIM: per channel the five moments, filtered along W into s_mid, then along H out of it
  for (int c = 0; c < 3; ++c) {
    for (int q = t; q < IM_TW * IM_SH; q += IM_BLOCK) {
      const int ow = q / IM_SH, sh = q % IM_SH;
      double ma = 0.0, mb = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
#pragma unroll
      for (int i = 0; i < IM_TAPS; ++i) {
        const double a = (double)s_a[c][ow + i][sh];
        const float bf = s_b[c][ow + i][sh];
        const double b = U8 ? s_tab[(int)bf] : (double)bf;
        const double ga = wt.g[i] * a, gb = wt.g[i] * b;
        ma += ga;
        mb += gb;
        aa = fma(ga, a, aa);
        bb = fma(gb, b, bb);
        ab = fma(ga, b, ab);
      }
      s_mid[0 * IM_TW * IM_SH + q] = ma;
      s_mid[1 * IM_TW * IM_SH + q] = mb;
      s_mid[2 * IM_TW * IM_SH + q] = aa;
      s_mid[3 * IM_TW * IM_SH + q] = bb;
      s_mid[4 * IM_TW * IM_SH + q] = ab;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < IM_PPT; ++j) {
      const int lw = (t >> 5) + (IM_TW / IM_PPT) * j, lh = t & 31;
      const double* m = s_mid + lw * IM_SH + lh;
      double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int i = 0; i < IM_TAPS; ++i) {
#pragma unroll
        for (int k = 0; k < 5; ++k) v[k] = fma(wt.g[i], m[k * IM_TW * IM_SH + i], v[k]);
      }
      const double ma = v[0], mb = v[1], mab = ma * mb;
      const double va = v[2] - ma * ma, vb = v[3] - mb * mb, cab = v[4] - mab;
      const double S = ((2.0 * mab + IM_C1) * (2.0 * cab + IM_C2)) / ((ma * ma + mb * mb + IM_C1) * (va + vb + IM_C2));
      ss[j] += S;
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < IM_PPT; ++j) {
    ss[j] = (flag[j] & F_SSIM) ? ss[j] / 3.0 : 0.0;
    if (ssim_map && (flag[j] & F_VALID)) {
      const int lw = (t >> 5) + (IM_TW / IM_PPT) * j, lh = t & 31;
      ssim_map[(img + w0 + lw) * H + h0 + lh] = (float)ss[j];
    }
  }

  // ---- the per-pixel values to LDS (s_mid is free: the loop above ended in a barrier), pixel lw * 32 + lh
  double* px_f = s_mid;                                   // [3][IM_PIX]: se, ssim, depth_abs
  int* px_i = (int*)(s_mid + IM_NF * IM_PIX);             // [3][IM_PIX]: flag, row, rrow
#pragma unroll
  for (int j = 0; j < IM_PPT; ++j) {
    const int p = t + IM_BLOCK * j;                       // == lw * 32 + lh
    px_f[p] = se[j];
    px_f[IM_PIX + p] = ss[j];
    px_f[2 * IM_PIX + p] = dabs[j];
    px_i[p] = flag[j];
    px_i[IM_PIX + p] = row[j];
    px_i[2 * IM_PIX + p] = rrow[j];
  }
  __syncthreads();

  // ---- the present rows, ascending, then row K
  int wtot, n_list;
  const int mine = t < K && s_present[t] ? 1 : 0;
  const int pos = block_prefix_waves<IM_WAVES>(wave_prefix_bits<1>(mine, &wtot), wtot, s_wave, &n_list);
  if (mine) s_list[pos] = t;
  if (t == 0) s_list[n_list] = K;
  __syncthreads();

  const int64_t nrow = (n * (K + 1));
  for (int e = wave; e <= n_list; e += IM_WAVES) {
    const int r = s_list[e];
    const bool all = r == K;
    double f0 = 0.0, f1 = 0.0, f2 = 0.0;
    int cnt[IM_NI] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < IM_PPL; ++j) {
      const int p = lane + 64 * j;
      const int fl = px_i[p];
      const bool in = all ? (fl & F_VALID) != 0 : px_i[IM_PIX + p] == r;
      const bool rec = !all && px_i[2 * IM_PIX + p] == r;
      f0 += in ? px_f[p] : 0.0;
      f1 += in ? px_f[IM_PIX + p] : 0.0;
      f2 += in ? px_f[2 * IM_PIX + p] : 0.0;
      cnt[0] += __popcll(__ballot(in));
      cnt[1] += __popcll(__ballot(in && (fl & F_SSIM)));
      cnt[2] += __popcll(__ballot(in && (fl & F_BOTH)));
      cnt[3] += __popcll(__ballot(in && (fl & F_ONLY_REC)));
      cnt[4] += __popcll(__ballot(in && (fl & F_ONLY_GT)));
      cnt[5] += __popcll(__ballot(rec));
      cnt[6] += __popcll(__ballot(all ? in && (fl & F_EQ) : in && rec));
    }
    f0 = wave_sum_f64(f0);
    f1 = wave_sum_f64(f1);
    f2 = wave_sum_f64(f2);
    if (lane == 0) {
      double* pf = part_f + (nrow + r) * IM_NF * tiles + tile;
      int* pi = part_i + (nrow + r) * IM_NI * tiles + tile;
      pf[0] = f0;
      pf[tiles] = f1;
      pf[2 * tiles] = f2;
#pragma unroll
      for (int k = 0; k < IM_NI; ++k) pi[k * tiles] = cnt[k];
    }
  }
  // the rows that no pixel of this tile belongs to: zeros
  if (t < K && !mine) {
    double* pf = part_f + (nrow + t) * IM_NF * tiles + tile;
    int* pi = part_i + (nrow + t) * IM_NI * tiles + tile;
#pragma unroll
    for (int k = 0; k < IM_NF; ++k) pf[k * tiles] = 0.0;
#pragma unroll
    for (int k = 0; k < IM_NI; ++k) pi[k * tiles] = 0;
  }
}

constexpr int FIN_BLOCK = 256;
__global__ __launch_bounds__(FIN_BLOCK) void im_finish_kernel(const double* __restrict__ part_f, const int* __restrict__ part_i,
                                                              int K, int N, int64_t tiles, int64_t n_rec_all,
                                                              int64_t* __restrict__ counts, double* __restrict__ sums) {
  __shared__ double s_f[IM_NF][FIN_BLOCK];
  __shared__ int64_t s_i[IM_NI][FIN_BLOCK];
  const int t = threadIdx.x;
  const int r = blockIdx.x;
  const int64_t n = blockIdx.y, slot = n * (K + 1) + r;
  const double* pf = part_f + slot * IM_NF * tiles;
  const int* pi = part_i + slot * IM_NI * tiles;
  double f[IM_NF] = {0.0, 0.0, 0.0};
  int64_t c[IM_NI] = {0, 0, 0, 0, 0, 0, 0};
  for (int64_t i = t; i < tiles; i += FIN_BLOCK) {
#pragma unroll
    for (int k = 0; k < IM_NF; ++k) f[k] += pf[k * tiles + i];
#pragma unroll
    for (int k = 0; k < IM_NI; ++k) c[k] += pi[k * tiles + i];
  }
#pragma unroll
  for (int k = 0; k < IM_NF; ++k) s_f[k][t] = f[k];
#pragma unroll
  for (int k = 0; k < IM_NI; ++k) s_i[k][t] = c[k];
  __syncthreads();
  for (int d = FIN_BLOCK / 2; d > 0; d >>= 1) {
    if (t < d) {
#pragma unroll
      for (int k = 0; k < IM_NF; ++k) s_f[k][t] += s_f[k][t + d];
#pragma unroll
      for (int k = 0; k < IM_NI; ++k) s_i[k][t] += s_i[k][t + d];
    }
    __syncthreads();
  }
  const int64_t table = (int64_t)N * (K + 1);
  if (t < IM_NF) sums[t * table + slot] = s_f[t][0];
  if (t < IM_NI) counts[t * table + slot] = (t == 5 && r == K) ? n_rec_all : s_i[t][0];
}

inline int im_check(int N, int W, int H, int K) {
  if (N < 1 || W < 1 || H < 1 || K < 0 || K > IM_MAXK) return CNR_E_ARG;
  if (N > 65535 || W > 32768 || H > 32768) return CNR_E_SHAPE;
  return CNR_OK;
}
}  // namespace

extern "C" int64_t cnr_image_scores_workspace_bytes(int N, int W, int H, int K) {
  const int rc = im_check(N, W, H, K);
  if (rc) return rc;
  return im_layout(N, W, H, K).bytes;
}

extern "C" int cnr_image_scores(const float* rgb_rec, const void* rgb_gt, int gt_u8, const float* depth_rec,
                                const float* depth_gt, int has_depth, const int* label_rec, const int* label_gt,
                                int has_labels, const int* ids, int K, int N, int W, int H, void* workspace, float* ssim_map,
                                int64_t* counts, double* sums, void* stream) {
  const int rc = im_check(N, W, H, K);
  if (rc) return rc;
  if (!rgb_rec || !rgb_gt || !workspace || !counts || !sums) return CNR_E_ARG;
  if ((has_depth != 0) != (depth_rec != nullptr) || (has_depth != 0) != (depth_gt != nullptr)) return CNR_E_ARG;
  if ((has_labels != 0) != (label_rec != nullptr) || (has_labels != 0) != (label_gt != nullptr)) return CNR_E_ARG;
  if (K > 0 && (!has_labels || !ids)) return CNR_E_ARG;
  if (((uintptr_t)workspace & 7) != 0) return CNR_E_ALIGN;
  const ImLayout L = im_layout(N, W, H, K);
  ImWeights wt;
  double sum = 0.0;
  for (int i = 0; i < IM_TAPS; ++i) {
    const double x = (double)(i - IM_R);
    wt.g[i] = exp(-(x * x) / (2.0 * 1.5 * 1.5));
    sum += wt.g[i];
  }
  for (int i = 0; i < IM_TAPS; ++i) wt.g[i] /= sum;
  char* ws = (char*)workspace;
  double* part_f = (double*)ws;
  int* part_i = (int*)(ws + L.off_i);
  const dim3 grid((unsigned)L.tiles, (unsigned)N);
  if (gt_u8) {
    hipLaunchKernelGGL(im_tile_kernel<true>, grid, dim3(IM_BLOCK), 0, (hipStream_t)stream, rgb_rec, rgb_gt, depth_rec, depth_gt,
                       label_rec, label_gt, ids, K, W, H, (int)L.th, L.tiles, wt, ssim_map, part_f, part_i);
  } else {
    hipLaunchKernelGGL(im_tile_kernel<false>, grid, dim3(IM_BLOCK), 0, (hipStream_t)stream, rgb_rec, rgb_gt, depth_rec, depth_gt,
                       label_rec, label_gt, ids, K, W, H, (int)L.th, L.tiles, wt, ssim_map, part_f, part_i);
  }
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(im_finish_kernel, dim3((unsigned)(K + 1), (unsigned)N), dim3(FIN_BLOCK), 0, (hipStream_t)stream,
                     (const double*)part_f, (const int*)part_i, K, N, L.tiles, has_labels ? (int64_t)W * H : (int64_t)0, counts,
                     sums);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}
