// Mesh rasterisation: which pixel of a pinhole view sees which triangle at what z-depth, then colour, label
// and normal images from the winner, and per-face visibility over many views.
//
// Coverage is homogeneous rasterisation in the camera frame: no projected vertices, no clipping.  Per (view, face), from the
// fp64 camera-frame corners v0 v1 v2:  n0 = v1 x v2, n1 = v2 x v0, n2 = v0 x v1, det = (v0.x n0.x + v0.y n0.y) + v0.z n0.z,
// s = sign(det).  Per pixel with ray d = (dx, dy, 1):  e_i = (n_i.x dx + n_i.y dy) + n_i.z, S = (e0 + e1) + e2, t = det / S;
// covered iff s e_i >= 0 for all i, s S > 0 and zmin <= t <= zmax.  The winner of a pixel is the covered face with the
// smallest (t, face index), so the result does not depend on the order a pixel meets its faces in.  Everything is fp64 with
// contraction off in the parenthesisation written here: tests/raster_cpu.py restates it in numpy and the images are held to
// that bit for bit.
//
//   setup  (cnr_raster_bin_count)  one thread per (view, face): the 10 doubles above, a conservative box of 8 x 8 pixel tiles
//                                  (the triangle cut at z >= zmin, projected, grown by a pixel; NEAR_EPS below has the case
//                                  zmin = 0), one integer atomic add per (view, tile) the box holds.
//   scan   (cnr_raster_bin_count)  one workgroup: where every (view, tile) list starts (int64), the number of pairs.
//   emit   (cnr_raster_bin_emit)   the same boxes again: the face into its tiles' lists through an integer cursor per list.
//                                  The order inside a list changes from run to run; the (t, face) rule makes that invisible.
//   tiles  (cnr_raster_tiles)      one wave per (view, tile), one pixel per lane; the list's records go through LDS 64 at a
//                                  time and every lane reads the same record (a broadcast read, as in cnr_nn_dist).
// A face whose box holds more than BIG_BOX tiles is spread over its wave's 64 lanes, so that a wall-sized triangle does not
// leave one lane walking thousands of tiles.  No floating-point atomics anywhere.
#include "cnr_common.h"
#include "geom_common.h"

#pragma clang fp contract(off)

using namespace cnr;

namespace {
constexpr int TILE = 8;                   // pixels per tile side: 64 pixels = one wave
constexpr int REC = 10;                   // doubles per (view, face): n0 n1 n2 det
constexpr int CHUNK = 64;                 // records per LDS stage (5 KB)
constexpr int BIN_BLOCK = 256;
constexpr int BIG_BOX = 16;
constexpr int MAX_SIDE = 32768;           // tile indices then fit 16 bits
// The box comes from the triangle cut at z >= max(zmin, NEAR_EPS), which can be projected.  With zmin below NEAR_EPS (configs
// carry min_depth = 0) the part nearer than that is seen by a pixel only where |x| <= z |dx| < NEAR_EPS max|dx| (y alike):
// a triangle whose bounds meet that small box before the camera gets every tile, every other one loses nothing.
constexpr double NEAR_EPS = 1.0 / 8192;

struct RasterLayout {
  int64_t items, tiles, TW, TH, off_box, off_count, off_cursor, off_start, bytes;
};
inline RasterLayout raster_layout(int64_t F, int V, int W, int H) {
  RasterLayout L;
  L.items = F * V;
  L.TW = (W + TILE - 1) / TILE;
  L.TH = (H + TILE - 1) / TILE;
  L.tiles = L.TW * L.TH * V;
  L.off_box = align256(L.items * REC * 8);
  L.off_count = L.off_box + align256(L.items * 8);
  L.off_cursor = L.off_count + align256(L.tiles * 4);
  L.off_start = L.off_cursor + align256(L.tiles * 4);
  L.bytes = L.off_start + align256(L.tiles * 8);
  return L;
}
inline bool raster_shape_ok(int64_t F, int V, int W, int H) {
  if (F < 1 || F > 0x7fffffff || V < 1 || W < 1 || H < 1 || W > MAX_SIDE || H > MAX_SIDE) return false;
  if (F * V > ((int64_t)1 << 40)) return false;           // before the layout multiplies it by 80
  return raster_layout(F, V, W, H).tiles <= 0x7fffffff;
}

struct Corners { double v[3][3]; };

// the camera-frame corners of face f: row r of T_cw (4x4, row-major) . (p, 1) as ((T0 x + T1 y) + T2 z) + T3
__device__ __forceinline__ Corners camera_corners(const float* __restrict__ verts, const int* __restrict__ faces,
                                                  const double* __restrict__ T, int64_t f) {
  Corners c;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float* p = verts + (int64_t)faces[3 * f + k] * 3;
    const double x = p[0], y = p[1], z = p[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) c.v[k][r] = ((T[4 * r] * x + T[4 * r + 1] * y) + T[4 * r + 2] * z) + T[4 * r + 3];
  }
  return c;
}

__device__ __forceinline__ void cross(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// box = (tx0 | tx1 << 16, ty0 | ty1 << 16); an empty box has tx0 > tx1
__device__ __forceinline__ int box_tiles(int2 box) {
  const int nx = (box.x >> 16) - (box.x & 0xffff) + 1, ny = (box.y >> 16) - (box.y & 0xffff) + 1;
  return nx > 0 && ny > 0 ? nx * ny : 0;
}
__device__ __forceinline__ int box_tile(int2 box, int i, int TH) {
  const int ny = (box.y >> 16) - (box.y & 0xffff) + 1;
  return ((box.x & 0xffff) + i / ny) * TH + (box.y & 0xffff) + i % ny;
}

// fn(item, tile of its view) for every tile of every lane's box; all 64 lanes of the wave must call this together.  Small
// boxes are walked by their own lane, large ones by the whole wave, one after the other.
template <typename Fn>
__device__ __forceinline__ void for_each_tile(int64_t item, int2 box, int TH, Fn fn) {
  const int cnt = box_tiles(box);
  if (cnt <= BIG_BOX) {
    for (int i = 0; i < cnt; ++i) fn(item, box_tile(box, i, TH));
  }
  uint64_t big = __ballot(cnt > BIG_BOX);
  const int lane = threadIdx.x & 63;
  while (big) {
    const int src = __ffsll((unsigned long long)big) - 1;
    big &= big - 1;
    const int2 b = make_int2(__shfl(box.x, src), __shfl(box.y, src));
    const int64_t it = ((int64_t)__shfl((int)(item >> 32), src) << 32) | (uint32_t)__shfl((int)item, src);
    const int n = box_tiles(b);
    for (int i = lane; i < n; i += 64) fn(it, box_tile(b, i, TH));
  }
}

__global__ __launch_bounds__(BIN_BLOCK) void raster_setup_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                                 int64_t F, const double* __restrict__ T_cw, int64_t items,
                                                                 int W, int H, double fx, double fy, double cx, double cy,
                                                                 double zmin, double near_x, double near_y, int cull,
                                                                 double* __restrict__ rec,
                                                                 int2* __restrict__ boxes, int* __restrict__ tile_count) {
  const int TH = (H + TILE - 1) / TILE, TW = (W + TILE - 1) / TILE;
  const int64_t per_view = (int64_t)TW * TH;
  for (int64_t base = (int64_t)blockIdx.x * BIN_BLOCK; base < items; base += (int64_t)gridDim.x * BIN_BLOCK) {
    const int64_t item = base + threadIdx.x;
    int2 box = make_int2(1, 1);                 // tx0 = 1 > tx1 = 0: empty
    if (item < items) {
      const int64_t view = item / F, f = item - view * F;
      const Corners c = camera_corners(verts, faces, T_cw + view * 16, f);
      double n[3][3];
      cross(c.v[1], c.v[2], n[0]);
      cross(c.v[2], c.v[0], n[1]);
      cross(c.v[0], c.v[1], n[2]);
      const double det = (c.v[0][0] * n[0][0] + c.v[0][1] * n[0][1]) + c.v[0][2] * n[0][2];
      double* o = rec + item * REC;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int b = 0; b < 3; ++b) o[3 * i + b] = n[i][b];
      }
      o[9] = det;
      if (det > 0.0 || (det < 0.0 && !cull)) {
        // the polygon z >= zcut of the triangle (at most 4 corners), projected as it is met
        const double zcut = fmax(zmin, NEAR_EPS);
        double ulo = INFINITY, uhi = -INFINITY, vlo = INFINITY, vhi = -INFINITY;
        bool any = false, odd = false;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double* a = c.v[k];
          const double* b = c.v[(k + 1) % 3];
          const bool ain = a[2] >= zcut, bin = b[2] >= zcut;
          double q[2][3];
          int m = 0;
          if (ain) {
            q[m][0] = a[0], q[m][1] = a[1], q[m][2] = a[2];
            ++m;
          }
          if (ain != bin) {
            const double r = (zcut - a[2]) / (b[2] - a[2]);
            q[m][0] = a[0] + r * (b[0] - a[0]), q[m][1] = a[1] + r * (b[1] - a[1]), q[m][2] = zcut;
            ++m;
          }
          if (!(a[2] == a[2])) odd = true;
          for (int j = 0; j < m; ++j) {
            const double u = fx * q[j][0] / q[j][2] + cx, v = fy * q[j][1] / q[j][2] + cy;
            ulo = fmin(ulo, u), uhi = fmax(uhi, u), vlo = fmin(vlo, v), vhi = fmax(vhi, v);
            if (!(u == u) || !(v == v)) odd = true;
            any = true;
          }
        }
        if (zmin < NEAR_EPS) {
          const double x0 = fmin(fmin(c.v[0][0], c.v[1][0]), c.v[2][0]), x1 = fmax(fmax(c.v[0][0], c.v[1][0]), c.v[2][0]);
          const double y0 = fmin(fmin(c.v[0][1], c.v[1][1]), c.v[2][1]), y1 = fmax(fmax(c.v[0][1], c.v[1][1]), c.v[2][1]);
          const double z0 = fmin(fmin(c.v[0][2], c.v[1][2]), c.v[2][2]), z1 = fmax(fmax(c.v[0][2], c.v[1][2]), c.v[2][2]);
          if (x0 <= near_x && x1 >= -near_x && y0 <= near_y && y1 >= -near_y && z0 <= NEAR_EPS && z1 >= zmin) odd = true;
        }
        if (odd) {                              // near the camera centre, or a corner that is not a number: every tile
          ulo = vlo = 0.0, uhi = W, vhi = H, any = true;
        }
        // pixel w sits at u = w; grown by one pixel, which also covers the fp32 rounding of the ray table
        const double w0 = fmax(floor(ulo) - 1.0, 0.0), w1 = fmin(ceil(uhi) + 1.0, (double)(W - 1));
        const double h0 = fmax(floor(vlo) - 1.0, 0.0), h1 = fmin(ceil(vhi) + 1.0, (double)(H - 1));
        if (any && w0 <= w1 && h0 <= h1)
          box = make_int2(((int)w0 / TILE) | (((int)w1 / TILE) << 16), ((int)h0 / TILE) | (((int)h1 / TILE) << 16));
      }
      boxes[item] = box;
    }
    for_each_tile(item, box, TH, [&](int64_t it, int tile) { atomicAdd(tile_count + (it / F) * per_view + tile, 1); });
  }
}

__global__ __launch_bounds__(BIN_BLOCK) void raster_emit_kernel(int64_t F, int64_t items, int W, int H,
                                                                const int2* __restrict__ boxes,
                                                                const int64_t* __restrict__ tile_start,
                                                                int* __restrict__ cursor, int* __restrict__ pair_face) {
  const int TH = (H + TILE - 1) / TILE, TW = (W + TILE - 1) / TILE;
  const int64_t per_view = (int64_t)TW * TH;
  for (int64_t base = (int64_t)blockIdx.x * BIN_BLOCK; base < items; base += (int64_t)gridDim.x * BIN_BLOCK) {
    const int64_t item = base + threadIdx.x;
    const int2 box = item < items ? boxes[item] : make_int2(1, 1);
    for_each_tile(item, box, TH, [&](int64_t it, int tile) {
      const int64_t k = (it / F) * per_view + tile;
      pair_face[tile_start[k] + atomicAdd(cursor + k, 1)] = (int)(it % F);
    });
  }
}

struct Hit { double e[3], S; };
__device__ __forceinline__ Hit edge_values(const double* r, double dx, double dy) {
  Hit h;
#pragma unroll
  for (int i = 0; i < 3; ++i) h.e[i] = (r[3 * i] * dx + r[3 * i + 1] * dy) + r[3 * i + 2];
  h.S = (h.e[0] + h.e[1]) + h.e[2];
  return h;
}

__global__ __launch_bounds__(64) void raster_tiles_kernel(const float* __restrict__ dirs, int64_t F, int W, int H, double zmin,
                                                          double zmax, const double* __restrict__ rec,
                                                          const int64_t* __restrict__ tile_start,
                                                          const int* __restrict__ tile_count,
                                                          const int* __restrict__ pair_face, float* __restrict__ depth,
                                                          int* __restrict__ face, float* __restrict__ bary) {
  __shared__ double s_rec[CHUNK * REC];
  __shared__ int s_face[CHUNK];
  const int TH = (H + TILE - 1) / TILE, TW = (W + TILE - 1) / TILE;
  const int64_t k = blockIdx.x, view = k / ((int64_t)TW * TH);
  const int tile = (int)(k - view * TW * TH), lane = threadIdx.x;
  const int w = (tile / TH) * TILE + (lane >> 3), h = (tile % TH) * TILE + (lane & 7);
  const bool inside = w < W && h < H;
  const int64_t pix = (int64_t)w * H + h;
  const double dx = inside ? (double)dirs[pix * 3] : 0.0, dy = inside ? (double)dirs[pix * 3 + 1] : 0.0;
  const int64_t start = tile_start[k];
  const int n = tile_count[k];
  double best_t = INFINITY, best_b1 = 0.0, best_b2 = 0.0;
  int best_f = -1;
  for (int c0 = 0; c0 < n; c0 += CHUNK) {
    const int m = n - c0 < CHUNK ? n - c0 : CHUNK;
    __syncthreads();
    if (lane < m) {
      const int f = pair_face[start + c0 + lane];
      const double* r = rec + (view * F + f) * REC;
      s_face[lane] = f;
#pragma unroll
      for (int q = 0; q < REC; ++q) s_rec[lane * REC + q] = r[q];
    }
    __syncthreads();
    for (int j = 0; j < m; ++j) {
      const double* r = s_rec + j * REC;
      const double det = r[9], s = det > 0.0 ? 1.0 : -1.0;
      const Hit hit = edge_values(r, dx, dy);
      if (s * hit.e[0] >= 0.0 && s * hit.e[1] >= 0.0 && s * hit.e[2] >= 0.0 && s * hit.S > 0.0) {
        const double t = det / hit.S;
        const int f = s_face[j];
        if (t >= zmin && t <= zmax && (t < best_t || (t == best_t && f < best_f))) {
          best_t = t, best_f = f, best_b1 = hit.e[1] / hit.S, best_b2 = hit.e[2] / hit.S;
        }
      }
    }
  }
  if (!inside) return;
  const int64_t o = view * W * H + pix;
  depth[o] = best_f >= 0 ? (float)best_t : 0.0f;
  face[o] = best_f;
  bary[2 * o] = (float)best_b1;
  bary[2 * o + 1] = (float)best_b2;
}

__device__ __forceinline__ void store_unit(double x, double y, double z, float* o) {
  const double len = sqrt((x * x + y * y) + z * z);
  const bool ok = len > 0.0 && len < INFINITY;
  o[0] = ok ? (float)(x / len) : 0.0f;
  o[1] = ok ? (float)(y / len) : 0.0f;
  o[2] = ok ? (float)(z / len) : 0.0f;
}

__global__ __launch_bounds__(256) void raster_attributes_kernel(const float* __restrict__ dirs, const float* __restrict__ verts,
                                                                const int* __restrict__ faces, const float* __restrict__ colors,
                                                                const float* __restrict__ normals,
                                                                const int* __restrict__ face_label,
                                                                const double* __restrict__ T_cw, int64_t F, int64_t P, int64_t n,
                                                                int vertex_normals, const double* __restrict__ rec,
                                                                const int* __restrict__ face_img, float* __restrict__ rgb,
                                                                int* __restrict__ instance, float* __restrict__ normal) {
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < n; o += (int64_t)gridDim.x * 256) {
    const int f = face_img[o];
    if (f < 0) {
      instance[o] = -1;
#pragma unroll
      for (int b = 0; b < 3; ++b) rgb[3 * o + b] = 0.0f, normal[3 * o + b] = 0.0f;
      continue;
    }
    const int64_t view = o / P, pix = o - view * P;
    const double dx = dirs[pix * 3], dy = dirs[pix * 3 + 1];
    const Hit hit = edge_values(rec + (view * F + f) * REC, dx, dy);
    const double b0 = hit.e[0] / hit.S, b1 = hit.e[1] / hit.S, b2 = hit.e[2] / hit.S;
    const int i0 = faces[3 * (int64_t)f], i1 = faces[3 * (int64_t)f + 1], i2 = faces[3 * (int64_t)f + 2];
    instance[o] = face_label[f];
#pragma unroll
    for (int b = 0; b < 3; ++b)
      rgb[3 * o + b] = (float)((b0 * (double)colors[3 * (int64_t)i0 + b] + b1 * (double)colors[3 * (int64_t)i1 + b]) +
                               b2 * (double)colors[3 * (int64_t)i2 + b]);
    double g[3];
    if (vertex_normals) {
#pragma unroll
      for (int b = 0; b < 3; ++b)
        g[b] = (b0 * (double)normals[3 * (int64_t)i0 + b] + b1 * (double)normals[3 * (int64_t)i1 + b]) +
               b2 * (double)normals[3 * (int64_t)i2 + b];
    } else {
      // the geometric normal in the world frame, turned towards the camera: g . (R_cw^T d) < 0
      double a[3], c[3];
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        a[b] = (double)verts[3 * (int64_t)i1 + b] - (double)verts[3 * (int64_t)i0 + b];
        c[b] = (double)verts[3 * (int64_t)i2 + b] - (double)verts[3 * (int64_t)i0 + b];
      }
      cross(a, c, g);
      const double* T = T_cw + view * 16;
      double dw[3];
#pragma unroll
      for (int b = 0; b < 3; ++b) dw[b] = (T[b] * dx + T[4 + b] * dy) + T[8 + b];
      if ((g[0] * dw[0] + g[1] * dw[1]) + g[2] * dw[2] > 0.0) g[0] = -g[0], g[1] = -g[1], g[2] = -g[2];
    }
    store_unit(g[0], g[1], g[2], normal + 3 * o);
  }
}

// flag[view F + f] = 1 where face f won a pixel of the view that passes the occluder test: every writer stores the same byte
__global__ __launch_bounds__(256) void raster_visible_mark_kernel(const int* __restrict__ face_img, const float* __restrict__ depth,
                                                                  const float* __restrict__ depth_obs, double tol, int64_t F,
                                                                  int64_t P, int64_t n, uint8_t* __restrict__ flag) {
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < n; o += (int64_t)gridDim.x * 256) {
    const int f = face_img[o];
    if (f < 0 || f >= F) continue;
    if (depth_obs && !(depth_obs[o] > 0.0f && (double)depth[o] <= (double)depth_obs[o] + tol)) continue;
    flag[(o / P) * F + f] = 1;
  }
}
__global__ __launch_bounds__(256) void raster_visible_sum_kernel(const uint8_t* __restrict__ flag, int64_t F, int V,
                                                                 uint8_t* __restrict__ seen, int* __restrict__ count) {
  for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < F; f += (int64_t)gridDim.x * 256) {
    int c = 0;
    for (int v = 0; v < V; ++v) c += flag[v * F + f];
    if (c) {
      seen[f] = 1;
      count[f] += c;
    }
  }
}
}  // namespace

extern "C" int64_t cnr_raster_workspace_bytes(int64_t F, int V, int W, int H) {
  if (!raster_shape_ok(F, V, W, H)) return CNR_E_SHAPE;
  return raster_layout(F, V, W, H).bytes;
}

extern "C" int cnr_raster_bin_count(const float* verts, const int* faces, int64_t F, const double* T_cw, int V, int W, int H,
                                    double fx, double fy, double cx, double cy, double zmin, int cull_backfaces, void* workspace,
                                    int64_t* n_pairs, void* stream) {
  if (!verts || !faces || !T_cw || !workspace || !n_pairs || !(zmin >= 0.0) || !(fx == fx) || !(fy == fy) || !(cx == cx) ||
      !(cy == cy))
    return CNR_E_ARG;
  if (!raster_shape_ok(F, V, W, H)) return CNR_E_SHAPE;
  const RasterLayout L = raster_layout(F, V, W, H);
  char* ws = (char*)workspace;
  hipError_t e = hipMemsetAsync(ws + L.off_count, 0, (size_t)(L.off_start - L.off_count), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  // the largest |dx|, |dy| of the ray table, a pixel to spare, times NEAR_EPS (fx = 0: infinite, every near face gets every tile)
  const double near_x = NEAR_EPS * (fmax(fabs(cx), fabs(W - 1 - cx)) + 1.0) / fabs(fx);
  const double near_y = NEAR_EPS * (fmax(fabs(cy), fabs(H - 1 - cy)) + 1.0) / fabs(fy);
  hipLaunchKernelGGL(raster_setup_kernel, dim3(grid_of(L.items, BIN_BLOCK, 1 << 16)), dim3(BIN_BLOCK), 0, (hipStream_t)stream,
                     verts, faces, F, T_cw, L.items, W, H, fx, fy, cx, cy, zmin, near_x, near_y, cull_backfaces ? 1 : 0, (double*)ws,
                     (int2*)(ws + L.off_box), (int*)(ws + L.off_count));
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL((blocks_scan_kernel<1, int64_t, int>), dim3(1), dim3(SCAN_THREADS), 0, (hipStream_t)stream,
                     (const int*)(ws + L.off_count), L.tiles, (int64_t*)(ws + L.off_start), n_pairs);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_raster_bin_emit(int64_t F, int V, int W, int H, void* workspace, int* pair_face, void* stream) {
  if (!workspace || !pair_face) return CNR_E_ARG;
  if (!raster_shape_ok(F, V, W, H)) return CNR_E_SHAPE;
  const RasterLayout L = raster_layout(F, V, W, H);
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(raster_emit_kernel, dim3(grid_of(L.items, BIN_BLOCK, 1 << 16)), dim3(BIN_BLOCK), 0, (hipStream_t)stream, F,
                     L.items, W, H, (const int2*)(ws + L.off_box), (const int64_t*)(ws + L.off_start),
                     (int*)(ws + L.off_cursor), pair_face);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_raster_tiles(const float* dirs, int64_t F, int V, int W, int H, double zmin, double zmax,
                                const void* workspace, const int* pair_face, float* depth, int* face, float* bary,
                                void* stream) {
  if (!dirs || !workspace || !pair_face || !depth || !face || !bary || !(zmin >= 0.0) || !(zmax >= zmin)) return CNR_E_ARG;
  if (!raster_shape_ok(F, V, W, H)) return CNR_E_SHAPE;
  const RasterLayout L = raster_layout(F, V, W, H);
  const char* ws = (const char*)workspace;
  hipLaunchKernelGGL(raster_tiles_kernel, dim3((unsigned)L.tiles), dim3(64), 0, (hipStream_t)stream, dirs, F, W, H, zmin, zmax,
                     (const double*)ws, (const int64_t*)(ws + L.off_start), (const int*)(ws + L.off_count), pair_face, depth,
                     face, bary);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_raster_attributes(const float* dirs, const float* verts, const int* faces, const float* colors,
                                     const float* normals, const int* face_label, const double* T_cw, int64_t F, int V, int W,
                                     int H, int vertex_normals, const void* workspace, const int* face_img, float* rgb,
                                     int* instance, float* normal, void* stream) {
  if (!dirs || !verts || !faces || !colors || !normals || !face_label || !T_cw || !workspace || !face_img || !rgb || !instance ||
      !normal)
    return CNR_E_ARG;
  if (!raster_shape_ok(F, V, W, H)) return CNR_E_SHAPE;
  const int64_t P = (int64_t)W * H, n = P * V;
  hipLaunchKernelGGL(raster_attributes_kernel, dim3(grid_of(n, 256, 1 << 16)), dim3(256), 0, (hipStream_t)stream, dirs, verts,
                     faces, colors, normals, face_label, T_cw, F, P, n, vertex_normals ? 1 : 0, (const double*)workspace,
                     face_img, rgb, instance, normal);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int64_t cnr_raster_visible_workspace_bytes(int64_t F, int V) {
  if (F < 1 || F > 0x7fffffff || V < 1) return CNR_E_SHAPE;
  return align256(F * V);
}

extern "C" int cnr_raster_visible(const int* face_img, const float* depth, const float* depth_obs, double tol, int64_t F, int V,
                                  int W, int H, void* workspace, uint8_t* seen, int* count, void* stream) {
  if (!face_img || !workspace || !seen || !count || (depth_obs && (!depth || !(tol == tol)))) return CNR_E_ARG;
  if (F < 1 || F > 0x7fffffff || V < 1 || W < 1 || H < 1) return CNR_E_SHAPE;
  const int64_t P = (int64_t)W * H, n = P * V;
  hipError_t e = hipMemsetAsync(workspace, 0, (size_t)(F * V), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(raster_visible_mark_kernel, dim3(grid_of(n, 256, 1 << 16)), dim3(256), 0, (hipStream_t)stream, face_img,
                     depth, depth_obs, tol, F, P, n, (uint8_t*)workspace);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(raster_visible_sum_kernel, dim3(grid_of(F, 256, 1 << 16)), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t*)workspace, F, V, seen, count);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}
