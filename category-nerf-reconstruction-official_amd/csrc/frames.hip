// Frame parsing for the dataset loaders (src/dataset.py get_all_frames, src/image_transforms.py): each label frame's instance
// table, the finished frame arrays in the reference's (W, H) layout, and cv2-style resizes.  DESIGN.md §3.8 has the contract.
//
// Instance table, reduce-then-scan with integer atomics only (order-independent, so every run is bit-identical and independent
// of the workgroup count):
//   zero      (cnr_frame_instances_count)  the per-frame presence bitmaps.
//   presence  (cnr_frame_instances_count)  grid (chunks, F): an LDS bitmap of the chunk's ids, OR-ed into the frame's bitmap.
//   rank      (cnr_frame_instances_count)  one workgroup per frame: exclusive popcount prefix per bitmap word, the frame count.
//   offsets   (cnr_frame_instances_count)  one thread: CSR offsets over the frames.
//   init      (cnr_frame_instances_emit)   one thread per bitmap word: the ids of its set bits (ascending), neutral statistics.
//   reduce    (cnr_frame_instances_emit)   grid (chunks, F): per pixel its id's rank = rank[word] + popcount(lower bits); count,
//                                          row / column / class min and max into LDS partials when the frame has at most
//                                          FR_PRIV ids, else straight into the global table.
#include "cnr_common.h"
#include "geom_common.h"

#pragma clang fp contract(off)

using cnr::align256;

namespace {
constexpr int FR_BLOCK = 256;
constexpr int FR_CHUNK = FR_BLOCK * 64;          // pixels per workgroup of the presence and reduce passes
constexpr int FR_MAX_BOUND = 65537;              // ids 0 .. 65536 (ScanNet's raw ids shifted by +1)
constexpr int FR_MAX_WORDS = (FR_MAX_BOUND + 31) / 32;
constexpr int FR_PRIV = 1024;                    // LDS-privatised statistics up to this many ids per frame
constexpr int FR_NSTAT = CNR_FRAME_NSTAT;        // count, row min, row max, col min, col max, class min, class max

struct FrLayout {
  int64_t nw, off_rank, off_cnt, bytes;
};
inline FrLayout fr_layout(int F, int id_bound) {
  FrLayout L;
  L.nw = (id_bound + 31) / 32;
  L.off_rank = align256((int64_t)F * L.nw * 4);
  L.off_cnt = L.off_rank + align256((int64_t)F * L.nw * 4);
  L.bytes = L.off_cnt + align256((int64_t)F * 4);
  return L;
}

__device__ __forceinline__ int load_label(const void* p, int i32, int64_t i) {
  return i32 ? ((const int32_t*)p)[i] : (int)((const uint16_t*)p)[i];
}

// pixel p (0 <= p < H * W) of frame f's analysed region -> element index in the stored (H + 2 edge) x (W + 2 edge) frame
__device__ __forceinline__ int64_t stored_index(int f, int64_t p, int H, int W, int edge) {
  const int64_t Ws = W + 2 * edge, Hs = H + 2 * edge;
  const int64_t r = p / W, c = p - r * W;
  return ((int64_t)f * Hs + r + edge) * Ws + c + edge;
}

__global__ void fr_zero_kernel(uint32_t* __restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = 0u;
}

__global__ __launch_bounds__(FR_BLOCK) void fr_presence_kernel(const void* __restrict__ inst, int i32, int H, int W, int edge,
                                                               int shift, int bound, int nw, uint32_t* __restrict__ bitmap) {
  __shared__ uint32_t s_bits[FR_MAX_WORDS];
  const int f = blockIdx.y;
  for (int w = threadIdx.x; w < nw; w += FR_BLOCK) s_bits[w] = 0u;
  __syncthreads();
  const int64_t npix = (int64_t)H * W, p0 = (int64_t)blockIdx.x * FR_CHUNK;
  const int64_t p1 = p0 + FR_CHUNK < npix ? p0 + FR_CHUNK : npix;
  int last = -1;
  for (int64_t p = p0 + threadIdx.x; p < p1; p += FR_BLOCK) {
    const int v = load_label(inst, i32, stored_index(f, p, H, W, edge)) + shift;
    if (v != last && v >= 0 && v < bound) {
      atomicOr(&s_bits[v >> 5], 1u << (v & 31));
      last = v;
    }
  }
  __syncthreads();
  uint32_t* out = bitmap + (int64_t)f * nw;
  for (int w = threadIdx.x; w < nw; w += FR_BLOCK)
    if (s_bits[w]) atomicOr(&out[w], s_bits[w]);
}

// one workgroup per frame: rank[w] = set bits in words < w; cnt[f] = all set bits
__global__ __launch_bounds__(FR_BLOCK) void fr_rank_kernel(const uint32_t* __restrict__ bitmap, int nw, int* __restrict__ rank,
                                                           int* __restrict__ cnt) {
  __shared__ int s_sum[FR_BLOCK];
  const int f = blockIdx.x;
  const uint32_t* bits = bitmap + (int64_t)f * nw;
  const int per = (nw + FR_BLOCK - 1) / FR_BLOCK;
  const int w0 = threadIdx.x * per, w1 = w0 + per < nw ? w0 + per : nw;
  int local = 0;
  for (int w = w0; w < w1; ++w) local += __popc(bits[w]);
  s_sum[threadIdx.x] = local;
  __syncthreads();
  if (threadIdx.x == 0) {                       // 256 partials: a serial scan is the simple form
    int run = 0;
    for (int t = 0; t < FR_BLOCK; ++t) {
      const int c = s_sum[t];
      s_sum[t] = run;
      run += c;
    }
    cnt[f] = run;
  }
  __syncthreads();
  int run = s_sum[threadIdx.x];
  for (int w = w0; w < w1; ++w) {
    rank[(int64_t)f * nw + w] = run;
    run += __popc(bits[w]);
  }
}

__global__ void fr_offsets_kernel(const int* __restrict__ cnt, int F, int64_t* __restrict__ offsets) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int64_t run = 0;
  offsets[0] = 0;
  for (int f = 0; f < F; ++f) {
    run += cnt[f];
    offsets[f + 1] = run;
  }
}

__device__ __forceinline__ void stat_init(int32_t* s, int64_t stride) {
  s[0] = 0;
  s[stride] = INT32_MAX;
  s[2 * stride] = -1;
  s[3 * stride] = INT32_MAX;
  s[4 * stride] = -1;
  s[5 * stride] = INT32_MAX;
  s[6 * stride] = INT32_MIN;
}

__global__ void fr_init_kernel(const uint32_t* __restrict__ bitmap, const int* __restrict__ rank, const int64_t* __restrict__ offsets,
                               int F, int nw, int32_t* __restrict__ ids, int32_t* __restrict__ stats) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)F * nw) return;
  const int f = (int)(t / nw), w = (int)(t - (int64_t)f * nw);
  uint32_t bits = bitmap[t];
  int64_t k = offsets[f] + rank[t];
  while (bits) {
    const int j = __ffs(bits) - 1;
    bits &= bits - 1;
    ids[k] = w * 32 + j;
    stat_init(stats + k * FR_NSTAT, 1);
    ++k;
  }
}

// statistic j of an entry at s[j * stride] (LDS partials: structure of arrays; the global table: rows of FR_NSTAT)
__device__ __forceinline__ void stat_add(int32_t* s, int64_t stride, int n, int rmin, int rmax, int cmin, int cmax, int kmin,
                                         int kmax) {
  atomicAdd(&s[0], n);
  atomicMin(&s[stride], rmin);
  atomicMax(&s[2 * stride], rmax);
  atomicMin(&s[3 * stride], cmin);
  atomicMax(&s[4 * stride], cmax);
  atomicMin(&s[5 * stride], kmin);
  atomicMax(&s[6 * stride], kmax);
}

__global__ __launch_bounds__(FR_BLOCK) void fr_reduce_kernel(const void* __restrict__ inst, const void* __restrict__ cls, int i32,
                                                             int H, int W, int edge, int shift, int bound, int nw,
                                                             const uint32_t* __restrict__ bitmap, const int* __restrict__ rank,
                                                             const int64_t* __restrict__ offsets, int32_t* __restrict__ stats) {
  __shared__ uint32_t s_bits[FR_MAX_WORDS];
  __shared__ int s_rank[FR_MAX_WORDS];
  __shared__ int32_t s_stat[FR_NSTAT * FR_PRIV];       // structure of arrays: statistic j of rank r at j * FR_PRIV + r
  const int f = blockIdx.y;
  const int64_t base = offsets[f];
  const int n_ids = (int)(offsets[f + 1] - base);
  const bool priv = n_ids <= FR_PRIV;
  for (int w = threadIdx.x; w < nw; w += FR_BLOCK) {
    s_bits[w] = bitmap[(int64_t)f * nw + w];
    s_rank[w] = rank[(int64_t)f * nw + w];
  }
  if (priv)
    for (int r = threadIdx.x; r < n_ids; r += FR_BLOCK) stat_init(s_stat + r, FR_PRIV);
  __syncthreads();
  const int64_t npix = (int64_t)H * W, p0 = (int64_t)blockIdx.x * FR_CHUNK;
  const int64_t p1 = p0 + FR_CHUNK < npix ? p0 + FR_CHUNK : npix;
  // a run of pixels of one id (this thread's pixels, in order) is accumulated in registers and added once
  int cur = -1, n = 0, rmin = 0, rmax = 0, cmin = 0, cmax = 0, kmin = 0, kmax = 0;
  auto flush = [&]() {
    const int w = cur >> 5;
    const int rk = s_rank[w] + __popc(s_bits[w] & ((1u << (cur & 31)) - 1u));
    if (priv)
      stat_add(s_stat + rk, FR_PRIV, n, rmin, rmax, cmin, cmax, kmin, kmax);
    else
      stat_add(stats + (base + rk) * FR_NSTAT, 1, n, rmin, rmax, cmin, cmax, kmin, kmax);
  };
  for (int64_t p = p0 + threadIdx.x; p < p1; p += FR_BLOCK) {
    const int64_t si = stored_index(f, p, H, W, edge);
    int v = load_label(inst, i32, si) + shift;
    if (v < 0 || v >= bound) v = -1;
    const int r = (int)(p / W), c = (int)(p - (int64_t)r * W);
    const int k = cls ? load_label(cls, i32, si) : 0;
    if (v != cur && cur >= 0) flush();
    if (v < 0) {
      cur = -1;
    } else if (v != cur) {
      cur = v;
      n = 1;
      rmin = rmax = r;
      cmin = cmax = c;
      kmin = kmax = k;
    } else {
      ++n;
      rmax = r;                                   // a thread's pixels come in increasing order: rows never decrease
      cmin = c < cmin ? c : cmin;
      cmax = c > cmax ? c : cmax;
      kmin = k < kmin ? k : kmin;
      kmax = k > kmax ? k : kmax;
    }
  }
  if (cur >= 0) flush();
  if (!priv) return;
  __syncthreads();
  for (int rk = threadIdx.x; rk < n_ids; rk += FR_BLOCK) {
    const int32_t* s = s_stat + rk;
    if (s[0] > 0)
      stat_add(stats + (base + rk) * FR_NSTAT, 1, s[0], s[FR_PRIV], s[2 * FR_PRIV], s[3 * FR_PRIV], s[4 * FR_PRIV],
               s[5 * FR_PRIV], s[6 * FR_PRIV]);
  }
}

__global__ void fr_finish_kernel(const void* __restrict__ inst, int i32, const uint16_t* __restrict__ depth,
                                 const uint8_t* __restrict__ rgb, int F, int H, int W, int edge, int label_edge, int shift, int bound,
                                 int nw, const uint32_t* __restrict__ bitmap, const int* __restrict__ rank,
                                 const int64_t* __restrict__ offsets, const uint8_t* __restrict__ keep, float depth_scale,
                                 float max_depth, int32_t* __restrict__ obj_mask, float* __restrict__ depth_out,
                                 uint8_t* __restrict__ image_out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t per = (int64_t)W * H;
  if (t >= (int64_t)F * per) return;
  const int f = (int)(t / per);
  const int64_t q = t - f * per;
  const int x = (int)(q / H), y = (int)(q - (int64_t)x * H);       // output (W, H): x along the image row
  const int64_t p = (int64_t)y * W + x;
  int v = load_label(inst, i32, stored_index(f, p, H, W, label_edge)) + shift;
  int out = 0;
  if (v >= 0 && v < bound) {
    const int w = v >> 5;
    const int64_t fw = (int64_t)f * nw + w;
    const int64_t k = offsets[f] + rank[fw] + __popc(bitmap[fw] & ((1u << (v & 31)) - 1u));
    out = keep[k] ? v : 0;
  }
  obj_mask[t] = out;
  const int64_t si = stored_index(f, p, H, W, edge);
  float d = (float)depth[si] * depth_scale;
  depth_out[t] = (d != d || d > max_depth) ? 0.0f : d;
  image_out[3 * t] = rgb[3 * si];
  image_out[3 * t + 1] = rgb[3 * si + 1];
  image_out[3 * t + 2] = rgb[3 * si + 2];
}

// cv2.resize(INTER_LINEAR) on 8-bit, 3 channels: coefficients as OpenCV's resize computes them (half-pixel centres, 11-bit
// fixed point, edge clamp), the horizontal pass in exact integers, the vertical pass in the form of its vectorised 32s -> 8u
// kernel: ((h0 >> 4) * b0 >> 16) + ((h1 >> 4) * b1 >> 16), rounded as (x + 2) >> 2 and saturated.
__device__ __forceinline__ void linear_coef(int d, int ssize, double scale, int* s0, int* s1, int* a0, int* a1, bool clamp_coef) {
  float fx = (float)__dadd_rn(__dmul_rn((double)d + 0.5, scale), -0.5);
  int sx = (int)floorf(fx);
  fx -= (float)sx;
  if (clamp_coef) {
    if (sx < 0) { fx = 0.f; sx = 0; }
    if (sx >= ssize - 1) { fx = 0.f; sx = ssize - 1; }
  }
  *a0 = __float2int_rn((1.f - fx) * 2048.f);
  *a1 = __float2int_rn(fx * 2048.f);
  const int lo = sx < 0 ? 0 : (sx > ssize - 1 ? ssize - 1 : sx);
  const int hi = sx + 1 < 0 ? 0 : (sx + 1 > ssize - 1 ? ssize - 1 : sx + 1);
  *s0 = lo;
  *s1 = hi;
}

__global__ void fr_resize_linear_kernel(const uint8_t* __restrict__ src, int F, int sh, int sw, uint8_t* __restrict__ dst, int dh, int dw,
                                        double scale_y, double scale_x) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t per = (int64_t)dh * dw;
  if (t >= (int64_t)F * per) return;
  const int f = (int)(t / per);
  const int64_t q = t - f * per;
  const int dy = (int)(q / dw), dx = (int)(q - (int64_t)dy * dw);
  int x0, x1, a0, a1, y0, y1, b0, b1;
  linear_coef(dx, sw, scale_x, &x0, &x1, &a0, &a1, true);
  linear_coef(dy, sh, scale_y, &y0, &y1, &b0, &b1, false);     // rows are clamped, their weights are not
  const uint8_t* r0 = src + ((int64_t)f * sh + y0) * sw * 3;
  const uint8_t* r1 = src + ((int64_t)f * sh + y1) * sw * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int h0 = r0[3 * x0 + c] * a0 + r0[3 * x1 + c] * a1;
    const int h1 = r1[3 * x0 + c] * a0 + r1[3 * x1 + c] * a1;
    int v = (((h0 >> 4) * b0) >> 16) + (((h1 >> 4) * b1) >> 16);
    v = (v + 2) >> 2;
    dst[3 * t + c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
  }
}

// cv2.resize(INTER_NEAREST): source index min(floor(d * (1 / (dsize / ssize))), ssize - 1) per axis
__global__ void fr_resize_nearest_kernel(const void* __restrict__ src, int elem_bytes, int F, int sh, int sw, void* __restrict__ dst,
                                         int dh, int dw, double iy, double ix) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t per = (int64_t)dh * dw;
  if (t >= (int64_t)F * per) return;
  const int f = (int)(t / per);
  const int64_t q = t - f * per;
  const int dy = (int)(q / dw), dx = (int)(q - (int64_t)dy * dw);
  int sy = (int)floor(__dmul_rn((double)dy, iy)), sx = (int)floor(__dmul_rn((double)dx, ix));
  sy = sy < sh - 1 ? sy : sh - 1;
  sx = sx < sw - 1 ? sx : sw - 1;
  const int64_t si = ((int64_t)f * sh + sy) * sw + sx;
  if (elem_bytes == 4)
    ((int32_t*)dst)[t] = ((const int32_t*)src)[si];
  else
    ((uint16_t*)dst)[t] = ((const uint16_t*)src)[si];
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

inline bool frame_args_ok(int F, int H, int W, int edge, int shift, int id_bound) {
  return F >= 1 && F <= 65535 && H >= 1 && W >= 1 && edge >= 0 && (shift == 0 || shift == 1) && id_bound >= 1 &&
         id_bound <= FR_MAX_BOUND && (int64_t)F * (H + 2 * edge) * (W + 2 * edge) < ((int64_t)1 << 40) &&
         (int64_t)(H + 2 * edge) * (W + 2 * edge) < ((int64_t)1 << 31);
}
}  // namespace

extern "C" int64_t cnr_frame_instances_workspace_bytes(int F, int id_bound) {
  if (F < 1 || F > 65535 || id_bound < 1 || id_bound > FR_MAX_BOUND) return CNR_E_SHAPE;
  return fr_layout(F, id_bound).bytes;
}

extern "C" int cnr_frame_instances_count(const void* inst, int label_i32, int F, int H, int W, int edge, int id_shift, int id_bound,
                                         void* workspace, int64_t* offsets_out, void* stream) {
  if (!inst || !workspace || !offsets_out) return CNR_E_ARG;
  if (!frame_args_ok(F, H, W, edge, id_shift, id_bound)) return CNR_E_SHAPE;
  const FrLayout L = fr_layout(F, id_bound);
  uint32_t* bitmap = (uint32_t*)workspace;
  int* rank = (int*)((char*)workspace + L.off_rank);
  int* cnt = (int*)((char*)workspace + L.off_cnt);
  const int64_t nbits = (int64_t)F * L.nw;
  const unsigned chunks = (unsigned)(((int64_t)H * W + FR_CHUNK - 1) / FR_CHUNK);
  hipLaunchKernelGGL(fr_zero_kernel, dim3(blocks_of(nbits) < 4096 ? blocks_of(nbits) : 4096), dim3(256), 0, (hipStream_t)stream,
                     bitmap, nbits);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(fr_presence_kernel, dim3(chunks, (unsigned)F), dim3(FR_BLOCK), 0, (hipStream_t)stream, inst, label_i32, H, W,
                     edge, id_shift, id_bound, (int)L.nw, bitmap);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(fr_rank_kernel, dim3((unsigned)F), dim3(FR_BLOCK), 0, (hipStream_t)stream, (const uint32_t*)bitmap, (int)L.nw,
                     rank, cnt);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(fr_offsets_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const int*)cnt, F, offsets_out);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_frame_instances_emit(const void* inst, const void* cls, int label_i32, int F, int H, int W, int edge, int id_shift,
                                        int id_bound, const void* workspace, const int64_t* offsets, int32_t* ids, int32_t* stats,
                                        void* stream) {
  if (!inst || !workspace || !offsets || !ids || !stats) return CNR_E_ARG;
  if (!frame_args_ok(F, H, W, edge, id_shift, id_bound)) return CNR_E_SHAPE;
  const FrLayout L = fr_layout(F, id_bound);
  const uint32_t* bitmap = (const uint32_t*)workspace;
  const int* rank = (const int*)((const char*)workspace + L.off_rank);
  const int64_t nbits = (int64_t)F * L.nw;
  const unsigned chunks = (unsigned)(((int64_t)H * W + FR_CHUNK - 1) / FR_CHUNK);
  hipLaunchKernelGGL(fr_init_kernel, dim3(blocks_of(nbits)), dim3(256), 0, (hipStream_t)stream, bitmap, rank, offsets, F, (int)L.nw,
                     ids, stats);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(fr_reduce_kernel, dim3(chunks, (unsigned)F), dim3(FR_BLOCK), 0, (hipStream_t)stream, inst, cls, label_i32, H, W,
                     edge, id_shift, id_bound, (int)L.nw, bitmap, rank, offsets, stats);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_frame_finish(const void* inst, int label_i32, int label_edge, const uint16_t* depth, const uint8_t* rgb, int F,
                                int H, int W, int edge, int id_shift, int id_bound, const void* workspace, const int64_t* offsets,
                                const uint8_t* keep, float depth_scale, float max_depth, int32_t* obj_mask, float* depth_out,
                                uint8_t* image_out, void* stream) {
  if (!inst || !depth || !rgb || !workspace || !offsets || !keep || !obj_mask || !depth_out || !image_out) return CNR_E_ARG;
  if (!frame_args_ok(F, H, W, edge, id_shift, id_bound) || !frame_args_ok(F, H, W, label_edge, id_shift, id_bound))
    return CNR_E_SHAPE;
  const FrLayout L = fr_layout(F, id_bound);
  const int64_t n = (int64_t)F * H * W;
  hipLaunchKernelGGL(fr_finish_kernel, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, inst, label_i32, depth, rgb, F, H, W,
                     edge, label_edge, id_shift, id_bound, (int)L.nw, (const uint32_t*)workspace,
                     (const int*)((const char*)workspace + L.off_rank), offsets, keep, depth_scale, max_depth, obj_mask, depth_out,
                     image_out);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_resize_linear_u8c3(const uint8_t* src, int F, int sh, int sw, uint8_t* dst, int dh, int dw, void* stream) {
  if (!src || !dst) return CNR_E_ARG;
  if (F < 1 || sh < 1 || sw < 1 || dh < 1 || dw < 1 || (int64_t)F * sh * sw * 3 >= ((int64_t)1 << 40) ||
      (int64_t)F * dh * dw >= ((int64_t)1 << 40))
    return CNR_E_SHAPE;
  const double scale_y = 1.0 / ((double)dh / sh), scale_x = 1.0 / ((double)dw / sw);
  hipLaunchKernelGGL(fr_resize_linear_kernel, dim3(blocks_of((int64_t)F * dh * dw)), dim3(256), 0, (hipStream_t)stream, src, F, sh, sw,
                     dst, dh, dw, scale_y, scale_x);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_resize_nearest(const void* src, int elem_bytes, int F, int sh, int sw, void* dst, int dh, int dw, void* stream) {
  if (!src || !dst) return CNR_E_ARG;
  if ((elem_bytes != 2 && elem_bytes != 4) || F < 1 || sh < 1 || sw < 1 || dh < 1 || dw < 1 ||
      (int64_t)F * sh * sw >= ((int64_t)1 << 40) || (int64_t)F * dh * dw >= ((int64_t)1 << 40))
    return CNR_E_SHAPE;
  const double iy = 1.0 / ((double)dh / sh), ix = 1.0 / ((double)dw / sw);
  hipLaunchKernelGGL(fr_resize_nearest_kernel, dim3(blocks_of((int64_t)F * dh * dw)), dim3(256), 0, (hipStream_t)stream, src,
                     elem_bytes, F, sh, sw, dst, dh, dw, iy, ix);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}
