// Geometry segmentation and mask refinement of one depth frame (src/utils.py: geometry_segmentation, refine_inst_data;
// DESIGN.md section 3.12): the depth-discontinuity and convexity maps (cnr_geoseg_maps), their morphology (cnr_geoseg_edge_map),
// connected-component labelling (cnr_ccl, cnr_label_counts), the 9x9 label growth onto edge pixels (cnr_geoseg_grow), hole
// filling (cnr_fill_holes) and the overlap vote against the raw instance map (cnr_refine_vote, cnr_refine_apply).  The point
// map and the normals come from the existing kernels (csrc/pointcloud.hip, csrc/fpfh.hip).
//
// Every fp32 product, sum, quotient and square root is rounded on its own (no contraction), so tests/geoseg_cpu.py repeats the
// image stages bit for bit.  No float atomics; the integer atomics (the union/find minima, the pixel counts) commute, so every
// output is defined by the inputs alone.  Every loop is bounded.
#include "cnr_common.h"
#include "ccl_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int T = cnr::ccl::TILE;        // 16 x 16 pixels per workgroup, one thread each
constexpr int HALO = 2, TH = T + 2 * HALO;   // 20: the 5x5 stencil / two 3x3 passes
constexpr int VOTE_MAX_IDS = 2048;
constexpr int VOTE_PIXELS = 4096;        // pixels per workgroup of the vote

__host__ __device__ inline int reflect101(int g, int n) {
  int r = g < 0 ? -g : (g >= n ? 2 * (n - 1) - g : g);
  return r < 0 ? 0 : (r >= n ? n - 1 : r);     // (only cells that feed no pixel of the image reach the clamp)
}

// ---- 2.2 discontinuity and convexity ------------------------------------------------------------------------------------
__global__ __launch_bounds__(T * T) void maps_kernel(const float* __restrict__ P, const float* __restrict__ N,
                                                      const float* __restrict__ depth, int H, int W,
                                                      uint8_t* __restrict__ disc, uint8_t* __restrict__ conv) {
  __shared__ float sP[3][TH * TH], sN[3][TH * TH], sD[TH * TH];
  const int x0 = blockIdx.x * T, y0 = blockIdx.y * T;
  for (int c = threadIdx.x; c < TH * TH; c += T * T) {
    const int gy = reflect101(y0 + c / TH - HALO, H), gx = reflect101(x0 + c % TH - HALO, W);
    const int64_t g = (int64_t)gy * W + gx;
#pragma unroll
    for (int k = 0; k < 3; ++k) { sP[k][c] = P[g * 3 + k]; sN[k][c] = N[g * 3 + k]; }
    sD[c] = depth[g];
  }
  __syncthreads();
  const int tx = threadIdx.x % T, ty = threadIdx.x / T, x = x0 + tx, y = y0 + ty;
  if (x >= W || y >= H) return;
  const int c = (ty + HALO) * TH + tx + HALO;
  const float d = sD[c];
  float ero = d, dil = d;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      if (y + dy < 0 || y + dy >= H || x + dx < 0 || x + dx >= W) continue;
      const float v = sD[c + dy * TH + dx];
      ero = fminf(ero, v);
      dil = fmaxf(dil, v);
    }
  const float ratio = d > 0.0f ? fmaxf(d - ero, dil - d) / d : 0.0f;
  const float nx = sN[0][c], ny = sN[1][c], nz = sN[2][c];
  const float px = sP[0][c], py = sP[1][c], pz = sP[2][c];
  float m = 10.0f;
  for (int dy = -2; dy <= 2; ++dy)
    for (int dx = -2; dx <= 2; ++dx) {
      if (dy == 0 && dx == 0) continue;
      const int n = c + dy * TH + dx;
      const float ex = sP[0][n] - px, ey = sP[1][n] - py, ez = sP[2][n] - pz;
      const float dot = (ex * (-nx) + ey * (-ny)) + ez * (-nz);
      const float proj = (nx * sN[0][n] + ny * sN[1][n]) + nz * sN[2][n];
      m = fminf(m, dot > -0.0005f ? 1.0f : proj);
    }
  const int64_t p = (int64_t)y * W + x;
  disc[p] = ratio > 0.01f ? 1 : 0;
  conv[p] = m > 0.9f ? 1 : 0;
}

// ---- 2.3 open(conv) & ~close(disc) & valid ------------------------------------------------------------------------------
__global__ __launch_bounds__(T * T) void edge_kernel(const uint8_t* __restrict__ disc, const uint8_t* __restrict__ conv,
                                                      const float* __restrict__ depth, int H, int W, uint8_t* __restrict__ edge) {
  constexpr int TI = T + 2;               // 18: the first pass is needed one pixel around the tile
  __shared__ signed char sc[TH * TH], sd[TH * TH], se[TI * TI], sl[TI * TI];      // -1: outside the image
  const int x0 = blockIdx.x * T, y0 = blockIdx.y * T;
  for (int c = threadIdx.x; c < TH * TH; c += T * T) {
    const int gy = y0 + c / TH - HALO, gx = x0 + c % TH - HALO;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
    sc[c] = in ? (conv[(int64_t)gy * W + gx] != 0) : -1;
    sd[c] = in ? (disc[(int64_t)gy * W + gx] != 0) : -1;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < TI * TI; c += T * T) {
    const int hy = c / TI + 1, hx = c % TI + 1, h = hy * TH + hx;
    int e = -1, l = -1;
    if (sc[h] >= 0) {
      e = 1; l = 0;
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          const int n = h + dy * TH + dx;
          if (sc[n] < 0) continue;
          e = min(e, (int)sc[n]);           // erode(conv)
          l = max(l, (int)sd[n]);           // dilate(disc)
        }
    }
    se[c] = (signed char)e;
    sl[c] = (signed char)l;
  }
  __syncthreads();
  const int tx = threadIdx.x % T, ty = threadIdx.x / T, x = x0 + tx, y = y0 + ty;
  if (x >= W || y >= H) return;
  const int c = (ty + 1) * TI + tx + 1;
  int open = 0, close = 1;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      const int n = c + dy * TI + dx;
      if (se[n] < 0) continue;
      open = max(open, (int)se[n]);
      close = min(close, (int)sl[n]);
    }
  const int64_t p = (int64_t)y * W + x;
  edge[p] = (open && !close && depth[p] > 0.0f) ? 1 : 0;
}

// ---- 2.4 connected components -------------------------------------------------------------------------------------------
// tile-local labelling in LDS; labels[p] = the frame-raster index of the smallest pixel of p's component WITHIN its tile
__global__ __launch_bounds__(T * T) void ccl_local_kernel(const uint8_t* __restrict__ mask, int H, int W, int conn8,
                                                           int* __restrict__ labels, int* __restrict__ err) {
  __shared__ int lab[T * T];
  const int t = threadIdx.x, tx = t % T, ty = t / T, x = blockIdx.x * T + tx, y = blockIdx.y * T + ty;
  const int64_t base = (int64_t)blockIdx.z * H * W;
  const bool in = x < W && y < H;
  const bool m = in && mask[base + (int64_t)y * W + x] != 0;
  lab[t] = m ? t : -1;
  __syncthreads();
  int e = 0;
  cnr::ccl::tile_unions(lab, t, conn8 != 0, &e);
  __syncthreads();
  if (in) {
    int out = -1;
    if (m) {
      const int r = cnr::ccl::find(lab, t, T * T, &e);
      out = (blockIdx.y * T + r / T) * W + blockIdx.x * T + r % T;
    }
    labels[base + (int64_t)y * W + x] = out;
  }
  if (e) *err = 1;
}

__global__ __launch_bounds__(T * T) void ccl_border_kernel(int H, int W, int conn8, int* __restrict__ labels, int* __restrict__ err) {
  const int t = threadIdx.x, x = blockIdx.x * T + t % T, y = blockIdx.y * T + t / T;
  if (x >= W || y >= H) return;
  int e = 0;
  cnr::ccl::border_unions(labels + (int64_t)blockIdx.z * H * W, x, y, H, W, conn8 != 0, &e);
  if (e) *err = 1;
}

__global__ __launch_bounds__(T * T) void ccl_flatten_kernel(int H, int W, int* __restrict__ labels, int* __restrict__ err) {
  const int t = threadIdx.x, x = blockIdx.x * T + t % T, y = blockIdx.y * T + t / T;
  if (x >= W || y >= H) return;
  int* L = labels + (int64_t)blockIdx.z * H * W;
  const int p = y * W + x;
  if (cnr::ccl::load(L + p) < 0) return;
  int e = 0;
  const int r = cnr::ccl::find(L, p, H * W, &e);
  // (another thread's walk may pass through p while this lands: the old parent and the root are both on its way up)
  __hip_atomic_store(L + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (e) *err = 1;
}

int launch_ccl(const uint8_t* mask, int F, int H, int W, int conn8, int* labels, int* err, hipStream_t s) {
  const dim3 grid((W + T - 1) / T, (H + T - 1) / T, F);
  ccl_local_kernel<<<grid, T * T, 0, s>>>(mask, H, W, conn8, labels, err);
  CNR_LAUNCH_CHECK();
  ccl_border_kernel<<<grid, T * T, 0, s>>>(H, W, conn8, labels, err);
  CNR_LAUNCH_CHECK();
  ccl_flatten_kernel<<<grid, T * T, 0, s>>>(H, W, labels, err);
  CNR_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(256) void label_counts_kernel(const int* __restrict__ labels, int64_t HW, int* __restrict__ counts) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t base = (int64_t)blockIdx.y * HW;
  const int l = p < HW ? labels[base + p] : -1;
  const bool on = l >= 0 && l < HW;
  // a wave's 64 consecutive pixels mostly lie in one region: one add of the wave's count instead of 64 adds to one address
  const unsigned long long active = __ballot(on);
  if (active == 0) return;
  const int leader = __ffsll((long long)active) - 1;
  const int first = __shfl(l, leader, 64);
  if (__ballot(on && l == first) == active) {
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(counts + base + first, __popcll(active));
  } else if (on) {
    atomicAdd(counts + base + l, 1);
  }
}

// ---- 2.5 label growth ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ int kept_label(const int* __restrict__ labels, const int* __restrict__ counts, int min_area, int64_t p,
                                          int64_t HW) {
  const int l = labels[p];
  if (l < 0 || l >= HW) return -1;
  return (counts == nullptr || counts[l] >= min_area) ? l : -1;
}

__global__ __launch_bounds__(256) void grow_kernel(const float* __restrict__ P, const float* __restrict__ depth,
                                                   const uint8_t* __restrict__ edge, const int* __restrict__ labels,
                                                   const int* __restrict__ counts, int min_area, int H, int W,
                                                   int* __restrict__ out) {
  const int64_t HW = (int64_t)H * W, p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  if (edge[p] != 0) { out[p] = kept_label(labels, counts, min_area, p, HW); return; }
  int best_label = -1;
  if (depth[p] > 0.0f) {
    const int y = (int)(p / W), x = (int)(p % W);
    const float px = P[p * 3], py = P[p * 3 + 1], pz = P[p * 3 + 2];
    float best = 0.05f;
    for (int i = -4; i <= 4; ++i)
      for (int j = -4; j <= 4; ++j) {
        if (i == 0 && j == 0) continue;
        const int xx = x + i, yy = y + j;
        if (xx < 0 || xx >= W || yy < 0 || yy >= H) continue;
        const int64_t q = (int64_t)yy * W + xx;
        if (edge[q] == 0) continue;                       // an edge pixel itself (or without depth: no label either)
        const int l = kept_label(labels, counts, min_area, q, HW);
        if (l < 0) continue;
        const float dx = px - P[q * 3], dy = py - P[q * 3 + 1], dz = pz - P[q * 3 + 2];
        const float dist = sqrtf((dx * dx + dy * dy) + dz * dz);
        if (dist < best) { best = dist; best_label = l; }
      }
  }
  out[p] = best_label;
}

// ---- 2.6 hole filling ---------------------------------------------------------------------------------------------------
// filled <- the complement of segment k (1 outside the segment)
__global__ __launch_bounds__(256) void complement_kernel(const int* __restrict__ labels, const int* __restrict__ seg_ids,
                                                         const uint8_t* __restrict__ masks, int64_t HW, uint8_t* __restrict__ comp) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const int64_t k = blockIdx.y;
  const bool inside = labels ? labels[p] == seg_ids[k] : masks[k * HW + p] != 0;
  comp[k * HW + p] = inside ? 0 : 1;
}

// flags[root] = 1 for every component of the complement with a pixel on the image border
__global__ __launch_bounds__(256) void border_flag_kernel(const int* __restrict__ lab, int H, int W, uint8_t* __restrict__ flags) {
  const int b = blockIdx.x * 256 + threadIdx.x;            // 0 .. 2W + 2H - 1: top row, bottom row, left column, right column
  if (b >= 2 * W + 2 * H) return;
  int x, y;
  if (b < W) { x = b; y = 0; }
  else if (b < 2 * W) { x = b - W; y = H - 1; }
  else if (b < 2 * W + H) { x = 0; y = b - 2 * W; }
  else { x = W - 1; y = b - 2 * W - H; }
  const int64_t base = (int64_t)blockIdx.y * H * W;
  const int l = lab[base + (int64_t)y * W + x];
  if (l >= 0) flags[base + l] = 1;
}

__global__ __launch_bounds__(256) void fill_kernel(const int* __restrict__ lab, const uint8_t* __restrict__ flags, int64_t HW,
                                                   uint8_t* __restrict__ filled) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const int64_t base = (int64_t)blockIdx.y * HW;
  const int l = lab[base + p];                              // -1 inside the segment
  filled[base + p] = (l < 0 || flags[base + l] == 0) ? 1 : 0;
}

__host__ inline int64_t round16(int64_t v) { return (v + 15) / 16 * 16; }

// ---- 2.7 the vote -------------------------------------------------------------------------------------------------------
// counts (K, O + 1): [k][o] = |filled_k & inst == obj_ids[o]|, [k][O] = |filled_k|
__global__ __launch_bounds__(256) void vote_kernel(const uint8_t* __restrict__ filled, const int* __restrict__ inst,
                                                   const int* __restrict__ obj_ids, int O, int64_t HW, int* __restrict__ counts) {
  __shared__ int hist[VOTE_MAX_IDS + 1];
  for (int o = threadIdx.x; o <= O; o += 256) hist[o] = 0;
  __syncthreads();
  const int64_t k = blockIdx.y, p0 = (int64_t)blockIdx.x * VOTE_PIXELS;
  for (int i = threadIdx.x; i < VOTE_PIXELS; i += 256) {
    const int64_t p = p0 + i;
    if (p >= HW || filled[k * HW + p] == 0) continue;
    atomicAdd(&hist[O], 1);
    const int v = inst[p];
    int lo = 0, hi = O;                                     // the first obj_ids[lo] >= v, at most 12 halvings
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (obj_ids[mid] < v) lo = mid + 1; else hi = mid; }
    if (lo < O && obj_ids[lo] == v) atomicAdd(&hist[lo], 1);
  }
  __syncthreads();
  for (int o = threadIdx.x; o <= O; o += 256)
    if (hist[o]) atomicAdd(counts + k * (O + 1) + o, hist[o]);
}

__global__ __launch_bounds__(256) void choose_kernel(const int* __restrict__ counts, int K, int O, double threshold,
                                                     int* __restrict__ chosen) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  const int total = counts[(int64_t)k * (O + 1) + O];
  int arg = -1;
  double best = 0.0;
  if (total > 0)
    for (int o = 0; o < O; ++o) {
      const double rate = (double)counts[(int64_t)k * (O + 1) + o] / (double)total;
      if (arg < 0 || rate > best) { best = rate; arg = o; }
    }
  chosen[k] = (arg >= 0 && best > threshold) ? arg : -1;
}

__global__ __launch_bounds__(256) void apply_kernel(const uint8_t* __restrict__ filled, const int* __restrict__ chosen,
                                                    const int* __restrict__ obj_ids, int K, int64_t HW, int* __restrict__ refined) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  int v = 0;
  for (int k = K - 1; k >= 0; --k)
    if (chosen[k] >= 0 && filled[(int64_t)k * HW + p] != 0) { v = obj_ids[chosen[k]]; break; }
  refined[p] = v;
}

inline bool bad_frame(int H, int W) { return H <= 0 || W <= 0 || (int64_t)H * W >= (1ll << 31) - 1; }
constexpr int MAX_STACK = 65535;          // frames / segments per call (the grid's third dimension)

}  // namespace

extern "C" {

int cnr_geoseg_maps(const float* P, const float* N, const float* depth, int H, int W, uint8_t* disc, uint8_t* conv, void* stream) {
  if (!P || !N || !depth || !disc || !conv) return CNR_E_ARG;
  if (bad_frame(H, W) || H < 3 || W < 3) return CNR_E_SHAPE;
  maps_kernel<<<dim3((W + T - 1) / T, (H + T - 1) / T), T * T, 0, (hipStream_t)stream>>>(P, N, depth, H, W, disc, conv);
  CNR_LAUNCH_CHECK();
  return 0;
}

int cnr_geoseg_edge_map(const uint8_t* disc, const uint8_t* conv, const float* depth, int H, int W, uint8_t* edge, void* stream) {
  if (!disc || !conv || !depth || !edge) return CNR_E_ARG;
  if (bad_frame(H, W)) return CNR_E_SHAPE;
  edge_kernel<<<dim3((W + T - 1) / T, (H + T - 1) / T), T * T, 0, (hipStream_t)stream>>>(disc, conv, depth, H, W, edge);
  CNR_LAUNCH_CHECK();
  return 0;
}

int cnr_ccl(const uint8_t* mask, int F, int H, int W, int connectivity, int* labels, int* err, void* stream) {
  if (!mask || !labels || !err) return CNR_E_ARG;
  if (bad_frame(H, W) || F <= 0 || F > MAX_STACK || (connectivity != 4 && connectivity != 8)) return CNR_E_SHAPE;
  return launch_ccl(mask, F, H, W, connectivity == 8, labels, err, (hipStream_t)stream);
}

int cnr_label_counts(const int* labels, int F, int H, int W, int* counts, void* stream) {
  if (!labels || !counts) return CNR_E_ARG;
  if (bad_frame(H, W) || F <= 0 || F > MAX_STACK) return CNR_E_SHAPE;
  const int64_t HW = (int64_t)H * W;
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)F * HW * sizeof(int), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  label_counts_kernel<<<dim3((unsigned)((HW + 255) / 256), F), 256, 0, (hipStream_t)stream>>>(labels, HW, counts);
  CNR_LAUNCH_CHECK();
  return 0;
}

int cnr_geoseg_grow(const float* P, const float* depth, const uint8_t* edge, const int* labels, const int* counts, int min_area,
                    int H, int W, int* labels_out, void* stream) {
  if (!P || !depth || !edge || !labels || !labels_out) return CNR_E_ARG;
  if (bad_frame(H, W)) return CNR_E_SHAPE;
  const int64_t HW = (int64_t)H * W;
  grow_kernel<<<(unsigned)((HW + 255) / 256), 256, 0, (hipStream_t)stream>>>(P, depth, edge, labels, counts, min_area, H, W,
                                                                             labels_out);
  CNR_LAUNCH_CHECK();
  return 0;
}

int64_t cnr_fill_holes_workspace_bytes(int K, int H, int W) {
  if (bad_frame(H, W) || K < 0 || K > MAX_STACK) return CNR_E_SHAPE;
  const int64_t n = (int64_t)K * H * W;
  return round16(n * 4) + round16(n);                       // labels of the complements (i32) | border flags (u8)
}

int cnr_fill_holes(const int* labels, const int* seg_ids, const uint8_t* masks, int K, int H, int W, void* workspace,
                   uint8_t* filled, int* err, void* stream) {
  if (bad_frame(H, W) || K < 0 || K > MAX_STACK) return CNR_E_SHAPE;
  if ((labels != nullptr) == (masks != nullptr) || (labels && !seg_ids) || !err) return CNR_E_ARG;
  if (K == 0) return 0;
  if (!workspace || !filled) return CNR_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int64_t HW = (int64_t)H * W, n = (int64_t)K * HW;
  int* lab = (int*)workspace;
  uint8_t* flags = (uint8_t*)workspace + round16(n * 4);
  const dim3 grid((unsigned)((HW + 255) / 256), K);
  complement_kernel<<<grid, 256, 0, s>>>(labels, seg_ids, masks, HW, filled);
  CNR_LAUNCH_CHECK();
  int rc = launch_ccl(filled, K, H, W, 0, lab, err, s);
  if (rc) return rc;
  hipError_t e = hipMemsetAsync(flags, 0, (size_t)n, s);
  if (e != hipSuccess) return (int)e;
  border_flag_kernel<<<dim3((2 * W + 2 * H + 255) / 256, K), 256, 0, s>>>(lab, H, W, flags);
  CNR_LAUNCH_CHECK();
  fill_kernel<<<grid, 256, 0, s>>>(lab, flags, HW, filled);
  CNR_LAUNCH_CHECK();
  return 0;
}

int cnr_refine_vote(const uint8_t* filled, const int* inst, const int* obj_ids, int K, int O, int H, int W, int* counts,
                    void* stream) {
  if (bad_frame(H, W) || K < 0 || K > MAX_STACK || O < 0 || O > VOTE_MAX_IDS) return CNR_E_SHAPE;
  if (!inst || !counts || (K > 0 && !filled) || (O > 0 && !obj_ids)) return CNR_E_ARG;
  if (K == 0) return 0;
  const int64_t HW = (int64_t)H * W;
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)K * (O + 1) * sizeof(int), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  vote_kernel<<<dim3((unsigned)((HW + VOTE_PIXELS - 1) / VOTE_PIXELS), K), 256, 0, (hipStream_t)stream>>>(filled, inst, obj_ids, O,
                                                                                                          HW, counts);
  CNR_LAUNCH_CHECK();
  return 0;
}

int cnr_refine_apply(const uint8_t* filled, const int* counts, const int* obj_ids, int K, int O, int H, int W, double threshold,
                     int* chosen, int* refined, void* stream) {
  if (bad_frame(H, W) || K < 0 || K > MAX_STACK || O < 0 || O > VOTE_MAX_IDS) return CNR_E_SHAPE;
  if (!refined || (K > 0 && (!filled || !counts || !chosen)) || (O > 0 && !obj_ids)) return CNR_E_ARG;
  const int64_t HW = (int64_t)H * W;
  if (K > 0) {
    choose_kernel<<<(K + 255) / 256, 256, 0, (hipStream_t)stream>>>(counts, K, O, threshold, chosen);
    CNR_LAUNCH_CHECK();
  }
  apply_kernel<<<(unsigned)((HW + 255) / 256), 256, 0, (hipStream_t)stream>>>(filled, chosen, obj_ids, K, HW, refined);
  CNR_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
