// TSDF fusion and radius outlier counts for ScanNet category registration (src/utils.py:212-247: ScalableTSDFVolume at 1 cm,
// extract_point_cloud, remove_radius_outlier).  DESIGN.md §3.10 has the contract; tests/tsdf_cpu.py restates it in numpy and
// the two agree bit for bit.
//
// A volume is a sorted list of units of 16^3 voxels (unit key = three biased 21-bit indices in one int64).
//   cnr_tsdf_depth_image      the metric depth masked to one instance, through uint16 millimetres, as the volume sees it.
//   cnr_tsdf_touch            every 4th pixel of every 4th column with a depth: the world point in fp64 and the keys of the (at
//                             most 8) units within the truncation distance of it; -1 in the unused slots.  The caller sorts.
//   cnr_tsdf_integrate        one workgroup per unit, 16 voxels per lane in registers; the unit's frames in the caller's (CSR)
//                             order, because the running weighted mean depends on it; one store of the unit at the end.
//   cnr_tsdf_extract_count/_emit  one point per valid voxel, axis and sign change towards the +1 neighbour (through the neighbour
//                             table at a unit's face), in the order unit, voxel, axis: count -> scan -> emit.
//   cnr_radius_cell_keys / cnr_radius_count  cells of edge r; per point the points of the 27 cells around it with squared
//                             distance < r^2, in fp64 from the fp32 coordinates: an exact integer.
// No float atomics; the only atomic is the integer OR of an error flag.  Every fp64 product and sum is rounded on its own
// (no contraction in this file), so a numpy restatement reproduces every bit.
#include "cnr_common.h"
#include "geom_common.h"

#include <math.h>

#pragma clang fp contract(off)

using namespace cnr;

namespace {
constexpr int TS_BLOCK = 256;
constexpr int UNIT_RES = 16;                              // ScalableTSDFVolume's volume_unit_resolution
constexpr int UNIT_VOX = UNIT_RES * UNIT_RES * UNIT_RES;
constexpr int VOX_PER_LANE = UNIT_VOX / TS_BLOCK;
constexpr int TOUCH_STRIDE = 4;                           // depth_sampling_stride
constexpr int TOUCH_SLOTS = 8;
static_assert(VOX_PER_LANE == UNIT_RES, "a lane of the integration holds one row of voxels along x");

__device__ __forceinline__ double key_axis(int64_t key, int a) {
  return (double)(((key >> ((2 - a) * AXIS_BITS)) & AXIS_MASK) - AXIS_BIAS);
}

// ---- depth image -------------------------------------------------------------------------------------------------------
// The division by a scalar is a kernel of its own because torch multiplies by the reciprocal on the device.
__global__ __launch_bounds__(TS_BLOCK) void depth_image_kernel(const float* __restrict__ depth, const int* __restrict__ obj_mask,
                                                               int64_t n, int inst_id, double depth_scale, double max_depth,
                                                               float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * TS_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * TS_BLOCK) {
    const double t = trunc((double)(obj_mask[i] == inst_id ? depth[i] : 0.0f) / depth_scale);
    const uint64_t u16 = t >= 0.0 && t < 9.2e18 ? (uint64_t)t & 0xFFFF : 0;          // numpy's astype(uint16) wraps; NaN -> 0
    const float d = (float)u16 / 1000.0f;
    out[i] = (double)d > max_depth ? 0.0f : d;
  }
}

// ---- touch -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TS_BLOCK) void touch_kernel(const float* __restrict__ depth, int W, int H, double fx, double fy,
                                                         double cx, double cy, const double* __restrict__ T, double unit_len,
                                                         double trunc, int frame, int64_t* __restrict__ keys,
                                                         int* __restrict__ frames, int* __restrict__ err) {
  const int sh = (H + TOUCH_STRIDE - 1) / TOUCH_STRIDE;
  const int64_t ns = (int64_t)((W + TOUCH_STRIDE - 1) / TOUCH_STRIDE) * sh;
  for (int64_t s = (int64_t)blockIdx.x * TS_BLOCK + threadIdx.x; s < ns; s += (int64_t)gridDim.x * TS_BLOCK) {
    const int x = (int)(s / sh) * TOUCH_STRIDE, y = (int)(s % sh) * TOUCH_STRIDE;
    const float df = depth[(int64_t)x * H + y];
    int64_t out[TOUCH_SLOTS];
#pragma unroll
    for (int k = 0; k < TOUCH_SLOTS; ++k) out[k] = -1;
    if (df > 0.0f) {
      const double d = (double)df;
      const double px = ((double)x - cx) * d / fx, py = ((double)y - cy) * d / fy;
      double lo[3], hi[3];
      bool ok = true;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double p = ((T[4 * a] * px + T[4 * a + 1] * py) + T[4 * a + 2] * d) + T[4 * a + 3];
        lo[a] = floor((p - trunc) / unit_len);
        hi[a] = floor((p + trunc) / unit_len);
        // false for NaN too; hi - lo > 1 cannot happen for trunc <= 8 voxel except by rounding exactly at that bound, and is
        // then reported like a key out of range instead of dropping the unit at hi
        ok = ok && lo[a] >= (double)-AXIS_BIAS && hi[a] < (double)AXIS_BIAS && hi[a] - lo[a] <= 1.0;
      }
      if (!ok) {
        atomicOr(err, 1);
      } else {
#pragma unroll
        for (int k = 0; k < TOUCH_SLOTS; ++k) {
          const double ux = lo[0] + (double)((k >> 2) & 1), uy = lo[1] + (double)((k >> 1) & 1), uz = lo[2] + (double)(k & 1);
          if (ux <= hi[0] && uy <= hi[1] && uz <= hi[2]) out[k] = pack_key((int64_t)ux, (int64_t)uy, (int64_t)uz);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < TOUCH_SLOTS; ++k) {
      keys[s * TOUCH_SLOTS + k] = out[k];
      frames[s * TOUCH_SLOTS + k] = frame;
    }
  }
}

// ---- integration -------------------------------------------------------------------------------------------------------
// Lane t holds the voxels (k, t >> 4, t & 15), k = 0 .. 15, of the unit: linear index k 256 + t, so the final stores coalesce.
__global__ __launch_bounds__(TS_BLOCK) void integrate_kernel(const int64_t* __restrict__ units, const int64_t* __restrict__ frame_ofs,
                                                             const int* __restrict__ frame_idx, const float* __restrict__ depth,
                                                             const uint8_t* __restrict__ color, const double* __restrict__ T_CW,
                                                             int F, int W, int H, double fx, double fy, double cx, double cy,
                                                             double voxel, double unit_len, double trunc, float* __restrict__ tsdf,
                                                             float* __restrict__ weight, float* __restrict__ colors) {
  const int64_t u = blockIdx.x;
  const int t = threadIdx.x;
  const int64_t key = units[u];
  const double ox = key_axis(key, 0) * unit_len;
  const double yw = key_axis(key, 1) * unit_len + ((double)(t >> 4) + 0.5) * voxel;
  const double zw = key_axis(key, 2) * unit_len + ((double)(t & 15) + 0.5) * voxel;
  const double umax = (double)W - 0.0001, vmax = (double)H - 0.0001;
  const int64_t npix = (int64_t)W * H;
  float f[VOX_PER_LANE], w[VOX_PER_LANE], cr[VOX_PER_LANE], cg[VOX_PER_LANE], cb[VOX_PER_LANE];
#pragma unroll
  for (int k = 0; k < VOX_PER_LANE; ++k) f[k] = w[k] = cr[k] = cg[k] = cb[k] = 0.0f;
  const int64_t j1 = frame_ofs[u + 1];
  for (int64_t j = frame_ofs[u]; j < j1; ++j) {
    const int fr = frame_idx[j];
    if ((unsigned)fr >= (unsigned)F) continue;            // never true for the wrapper's lists; no read outside the frames
    const double* T = T_CW + 16 * (int64_t)fr;
    const float* dimg = depth + fr * npix;
    const uint8_t* cimg = color + 3 * fr * npix;
    // the parts of T_CW . centre that do not depend on k, in the contract's order ((T0 x + T1 y) + T2 z) + T3
    const double t00 = T[0], t10 = T[4], t20 = T[8], t03 = T[3], t13 = T[7], t23 = T[11];
    const double a0y = T[1] * yw, a1y = T[5] * yw, a2y = T[9] * yw, a0z = T[2] * zw, a1z = T[6] * zw, a2z = T[10] * zw;
#pragma unroll
    for (int k = 0; k < VOX_PER_LANE; ++k) {
      const double xw = ox + ((double)k + 0.5) * voxel;
      const double z = ((t20 * xw + a2y) + a2z) + t23;
      if (z <= 0.0) continue;
      const double x = ((t00 * xw + a0y) + a0z) + t03, y = ((t10 * xw + a1y) + a1z) + t13;
      const double uf = (x * fx / z + cx) + 0.5, vf = (y * fy / z + cy) + 0.5;
      if (!(uf >= 0.0001 && uf < umax && vf >= 0.0001 && vf < vmax)) continue;
      const int pu = (int)uf, pv = (int)vf;
      const int64_t pix = (int64_t)pu * H + pv;
      const float df = dimg[pix];
      if (!(df > 0.0f)) continue;
      const double a = ((double)pu - cx) / fx, b = ((double)pv - cy) / fy;
      const double sdf = ((double)df - z) * __dsqrt_rn((a * a + b * b) + 1.0);
      if (!(sdf > -trunc)) continue;
      const double q = sdf / trunc;
      const float tf = (float)(q < 1.0 ? q : 1.0);
      const float wk = w[k], wn = wk + 1.0f;
      f[k] = (f[k] * wk + tf) / wn;
      cr[k] = (cr[k] * wk + (float)cimg[3 * pix]) / wn;
      cg[k] = (cg[k] * wk + (float)cimg[3 * pix + 1]) / wn;
      cb[k] = (cb[k] * wk + (float)cimg[3 * pix + 2]) / wn;
      w[k] = wn;
    }
  }
  const int64_t base = u * UNIT_VOX + t;
#pragma unroll
  for (int k = 0; k < VOX_PER_LANE; ++k) {
    const int64_t i = base + k * TS_BLOCK;
    tsdf[i] = f[k];
    weight[i] = w[k];
    colors[3 * i] = cr[k];
    colors[3 * i + 1] = cg[k];
    colors[3 * i + 2] = cb[k];
  }
}

// ---- extraction --------------------------------------------------------------------------------------------------------
struct ExtractLayout {
  int64_t off_ofs, bytes;
};
inline ExtractLayout extract_layout(int64_t U) {
  ExtractLayout L;
  L.off_ofs = align256(U * 4);
  L.bytes = L.off_ofs + align256(U * 8);
  return L;
}

__device__ __forceinline__ bool voxel_valid(float f, float w) { return w != 0.0f && f < 0.98f && f >= -0.98f; }

// Lane t walks the voxels t 16 .. t 16 + 15 (ix = t >> 4, iy = t & 15, iz the walk), so lane order is voxel order.  (Lanes are 64 B
// apart in each load and the emit kernel walks twice: unmeasured, the first thing to look at if extraction shows up in a profile.)
// the +1 neighbour of voxel (ix, iy, iz) along axis a: *nu = its unit (-1: absent), the return value its linear index
__device__ __forceinline__ int neighbour_of(const int* __restrict__ nb, int64_t u, int64_t U, int ix, int iy, int iz, int a,
                                            int64_t* nu) {
  const int c[3] = {ix, iy, iz};
  const int step = a == 0 ? UNIT_RES * UNIT_RES : (a == 1 ? UNIT_RES : 1);
  const int idx = (ix * UNIT_RES + iy) * UNIT_RES + iz;
  if (c[a] + 1 < UNIT_RES) {
    *nu = u;
    return idx + step;
  }
  const int64_t v = nb[3 * u + a];
  *nu = v >= 0 && v < U ? v : -1;
  return idx - (UNIT_RES - 1) * step;
}

template <bool EMIT>
__device__ __forceinline__ int extract_walk(const int64_t* __restrict__ units, const float* __restrict__ tsdf,
                                            const float* __restrict__ weight, const float* __restrict__ colors,
                                            const int* __restrict__ nb, int64_t U, double voxel, int64_t o,
                                            double* __restrict__ out_p, double* __restrict__ out_c) {
  const int64_t u = blockIdx.x;
  const int t = threadIdx.x, ix = t >> 4, iy = t & 15;
  const int64_t base = u * UNIT_VOX;
  int c = 0;
  for (int iz = 0; iz < UNIT_RES; ++iz) {
    const int idx = t * UNIT_RES + iz;
    const float f0 = tsdf[base + idx];
    if (!voxel_valid(f0, weight[base + idx])) continue;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      int64_t nu;
      const int nidx = neighbour_of(nb, u, U, ix, iy, iz, a, &nu);
      if (nu < 0) continue;
      const int64_t n1 = nu * UNIT_VOX + nidx;
      const float f1 = tsdf[n1];
      if (!voxel_valid(f1, weight[n1]) || !(f0 * f1 < 0.0f)) continue;
      if (EMIT) {
        const int64_t key = units[u];
        const double unit_len = (double)UNIT_RES * voxel;
        double p[3] = {key_axis(key, 0) * unit_len + ((double)ix + 0.5) * voxel,
                       key_axis(key, 1) * unit_len + ((double)iy + 0.5) * voxel,
                       key_axis(key, 2) * unit_len + ((double)iz + 0.5) * voxel};
        const double r0 = fabs((double)f0), r1 = fabs((double)f1), rs = r0 + r1;
        const double p0 = p[a], p1 = p0 + voxel;
        p[a] = (p0 * r1 + p1 * r0) / rs;
        const int64_t q = o + c;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          out_p[3 * q + ch] = p[ch];
          const double c0 = (double)colors[3 * (base + idx) + ch], c1 = (double)colors[3 * n1 + ch];
          out_c[3 * q + ch] = (c0 * r1 + c1 * r0) / rs / 255.0;
        }
      }
      ++c;
    }
  }
  return c;
}

__global__ __launch_bounds__(TS_BLOCK) void extract_count_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                                 const int* __restrict__ nb, int64_t U, int* __restrict__ blk_counts) {
  __shared__ int s[TS_BLOCK];
  const int c = extract_walk<false>(nullptr, tsdf, weight, nullptr, nb, U, 0.0, 0, nullptr, nullptr);
  int total;
  block_excl_scan<TS_BLOCK>(c, s, &total);
  if (threadIdx.x == 0) blk_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(TS_BLOCK) void extract_emit_kernel(const int64_t* __restrict__ units, const float* __restrict__ tsdf,
                                                                const float* __restrict__ weight, const float* __restrict__ colors,
                                                                const int* __restrict__ nb, int64_t U, double voxel,
                                                                const int64_t* __restrict__ ofs, double* __restrict__ out_p,
                                                                double* __restrict__ out_c) {
  __shared__ int s[TS_BLOCK];
  const int c = extract_walk<false>(nullptr, tsdf, weight, nullptr, nb, U, 0.0, 0, nullptr, nullptr);
  int total;
  const int64_t o = ofs[blockIdx.x] + block_excl_scan<TS_BLOCK>(c, s, &total);
  extract_walk<true>(units, tsdf, weight, colors, nb, U, voxel, o, out_p, out_c);
}

// ---- radius count ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TS_BLOCK) void cell_keys_kernel(const float* __restrict__ p, int64_t n, double r,
                                                             int64_t* __restrict__ keys, int* __restrict__ err) {
  for (int64_t i = (int64_t)blockIdx.x * TS_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * TS_BLOCK) {
    const double a = floor((double)p[3 * i] / r), b = floor((double)p[3 * i + 1] / r), c = floor((double)p[3 * i + 2] / r);
    const double lo = (double)-AXIS_BIAS, hi = (double)AXIS_BIAS;
    const bool ok = a >= lo && a < hi && b >= lo && b < hi && c >= lo && c < hi;     // false for NaN too
    if (!ok) atomicOr(err, 1);
    keys[i] = ok ? pack_key((int64_t)a, (int64_t)b, (int64_t)c) : (int64_t)-1;
  }
}

// Lane j takes the j-th point in cell order (neighbours in the wave share cells).  The three cells (X, Y, cz - 1 .. cz + 1) are
// consecutive keys, so nine ranges of the cell list cover the 27 cells.
__global__ __launch_bounds__(TS_BLOCK) void radius_count_kernel(const float* __restrict__ p, int64_t n, const int64_t* __restrict__ perm,
                                                                const int64_t* __restrict__ skeys, const int64_t* __restrict__ cells,
                                                                const int64_t* __restrict__ starts, int64_t C, double r,
                                                                int* __restrict__ counts) {
  const double r2 = r * r;
  for (int64_t j = (int64_t)blockIdx.x * TS_BLOCK + threadIdx.x; j < n; j += (int64_t)gridDim.x * TS_BLOCK) {
    const int64_t i = perm[j], key = skeys[j];
    if (i < 0 || i >= n || key < 0) continue;
    const double x = (double)p[3 * i], y = (double)p[3 * i + 1], z = (double)p[3 * i + 2];
    const int64_t kx = (key >> (2 * AXIS_BITS)) & AXIS_MASK, ky = (key >> AXIS_BITS) & AXIS_MASK, kz = key & AXIS_MASK;
    const int64_t z0 = kz > 0 ? kz - 1 : 0, z1 = kz < AXIS_MASK ? kz + 1 : AXIS_MASK;
    int cnt = 0;
    for (int64_t X = kx - 1; X <= kx + 1; ++X) {
      if (X < 0 || X > AXIS_MASK) continue;
      for (int64_t Y = ky - 1; Y <= ky + 1; ++Y) {
        if (Y < 0 || Y > AXIS_MASK) continue;
        const int64_t row = (X << (2 * AXIS_BITS)) | (Y << AXIS_BITS);
        const int64_t c0 = lower_bound(cells, C, row | z0), c1 = lower_bound(cells, C, (row | z1) + 1);
        int64_t m1 = starts[c1];
        m1 = m1 < n ? m1 : n;
        for (int64_t m = starts[c0] > 0 ? starts[c0] : 0; m < m1; ++m) {
          const int64_t q = perm[m];
          if (q < 0 || q >= n) continue;
          const double dx = x - (double)p[3 * q], dy = y - (double)p[3 * q + 1], dz = z - (double)p[3 * q + 2];
          cnt += ((dx * dx + dy * dy) + dz * dz) < r2 ? 1 : 0;
        }
      }
    }
    counts[i] = cnt;
  }
}

inline bool camera_ok(int W, int H, double fx, double fy) { return W >= 1 && H >= 1 && W <= 32768 && H <= 32768 && fx != 0.0 && fy != 0.0; }
// [p - trunc, p + trunc] may not be longer than a unit's edge: a sample then touches at most two units per axis, the 8 slots
inline bool volume_ok(double voxel, double trunc) { return voxel > 0.0 && trunc > 0.0 && 2.0 * trunc <= (double)UNIT_RES * voxel; }
}  // namespace

// ---- entry points ------------------------------------------------------------------------------------------------------
extern "C" int cnr_tsdf_depth_image(const float* depth, const int* obj_mask, int64_t n, int inst_id, double depth_scale,
                                    double max_depth, float* out, void* stream) {
  if (!depth || !obj_mask || !out) return CNR_E_ARG;
  if (n < 1 || !(depth_scale > 0.0)) return CNR_E_SHAPE;
  hipLaunchKernelGGL(depth_image_kernel, dim3(grid_of(n, TS_BLOCK, 4096)), dim3(TS_BLOCK), 0, (hipStream_t)stream, depth, obj_mask, n,
                     inst_id, depth_scale, max_depth, out);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int64_t cnr_tsdf_touch_slots(int W, int H) {
  if (W < 1 || H < 1 || W > 32768 || H > 32768) return CNR_E_SHAPE;
  return (int64_t)((W + TOUCH_STRIDE - 1) / TOUCH_STRIDE) * ((H + TOUCH_STRIDE - 1) / TOUCH_STRIDE) * TOUCH_SLOTS;
}

extern "C" int cnr_tsdf_touch(const float* depth, int W, int H, double fx, double fy, double cx, double cy, const double* T_WC,
                              double voxel, double trunc, int frame, int64_t* keys, int* frames, int* err, void* stream) {
  if (!depth || !T_WC || !keys || !frames || !err) return CNR_E_ARG;
  if (!camera_ok(W, H, fx, fy) || !volume_ok(voxel, trunc) || frame < 0) return CNR_E_SHAPE;
  const int64_t ns = cnr_tsdf_touch_slots(W, H) / TOUCH_SLOTS;
  hipLaunchKernelGGL(touch_kernel, dim3(grid_of(ns, TS_BLOCK, 4096)), dim3(TS_BLOCK), 0, (hipStream_t)stream, depth, W, H, fx, fy, cx, cy,
                     T_WC, (double)UNIT_RES * voxel, trunc, frame, keys, frames, err);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_tsdf_integrate(const int64_t* units, int64_t U, const int64_t* frame_ofs, const int* frame_idx,
                                  const float* depth, const uint8_t* color, const double* T_CW, int F, int W, int H, double fx,
                                  double fy, double cx, double cy, double voxel, double trunc, float* tsdf, float* weight,
                                  float* colors, void* stream) {
  if (!units || !frame_ofs || !frame_idx || !depth || !color || !T_CW || !tsdf || !weight || !colors) return CNR_E_ARG;
  if (U < 1 || U > 0x7fffffff || F < 1 || !camera_ok(W, H, fx, fy) || !volume_ok(voxel, trunc)) return CNR_E_SHAPE;
  hipLaunchKernelGGL(integrate_kernel, dim3((unsigned)U), dim3(TS_BLOCK), 0, (hipStream_t)stream, units, frame_ofs, frame_idx, depth,
                     color, T_CW, F, W, H, fx, fy, cx, cy, voxel, (double)UNIT_RES * voxel, trunc, tsdf, weight, colors);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int64_t cnr_tsdf_extract_workspace_bytes(int64_t U) {
  if (U < 1 || U > 0x7fffffff) return CNR_E_SHAPE;
  return extract_layout(U).bytes;
}

extern "C" int cnr_tsdf_extract_count(const float* tsdf, const float* weight, const int* neighbours, int64_t U, void* workspace,
                                      int64_t* count_out, void* stream) {
  if (!tsdf || !weight || !neighbours || !workspace || !count_out) return CNR_E_ARG;
  if (U < 1 || U > 0x7fffffff) return CNR_E_SHAPE;
  const ExtractLayout L = extract_layout(U);
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(extract_count_kernel, dim3((unsigned)U), dim3(TS_BLOCK), 0, (hipStream_t)stream, tsdf, weight, neighbours, U,
                     (int*)ws);
  CNR_LAUNCH_CHECK();
  hipLaunchKernelGGL((blocks_scan_kernel<1, int64_t, int>), dim3(1), dim3(SCAN_THREADS), 0, (hipStream_t)stream, (const int*)ws, U,
                     (int64_t*)(ws + L.off_ofs), count_out);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_tsdf_extract_emit(const int64_t* units, const float* tsdf, const float* weight, const float* colors,
                                     const int* neighbours, int64_t U, double voxel, void* workspace, double* points,
                                     double* colors_out, void* stream) {
  if (!units || !tsdf || !weight || !colors || !neighbours || !workspace || !points || !colors_out) return CNR_E_ARG;
  if (U < 1 || U > 0x7fffffff || !(voxel > 0.0)) return CNR_E_SHAPE;
  const ExtractLayout L = extract_layout(U);
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(extract_emit_kernel, dim3((unsigned)U), dim3(TS_BLOCK), 0, (hipStream_t)stream, units, tsdf, weight, colors,
                     neighbours, U, voxel, (const int64_t*)(ws + L.off_ofs), points, colors_out);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_radius_cell_keys(const float* points, int64_t n, double radius, int64_t* keys, int* err, void* stream) {
  if (!points || !keys || !err) return CNR_E_ARG;
  if (n < 1 || !(radius > 0.0)) return CNR_E_SHAPE;
  hipLaunchKernelGGL(cell_keys_kernel, dim3(grid_of(n, TS_BLOCK, 4096)), dim3(TS_BLOCK), 0, (hipStream_t)stream, points, n, radius, keys,
                     err);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}

extern "C" int cnr_radius_count(const float* points, int64_t n, const int64_t* perm, const int64_t* sorted_keys,
                                const int64_t* cells, const int64_t* starts, int64_t C, double radius, int* counts, void* stream) {
  if (!points || !perm || !sorted_keys || !cells || !starts || !counts) return CNR_E_ARG;
  if (n < 1 || C < 1 || C > n || !(radius > 0.0)) return CNR_E_SHAPE;
  hipLaunchKernelGGL(radius_count_kernel, dim3(grid_of(n, TS_BLOCK, 65536)), dim3(TS_BLOCK), 0, (hipStream_t)stream, points, n, perm,
                     sorted_keys, cells, starts, C, radius, counts);
  CNR_LAUNCH_CHECK();
  return CNR_OK;
}
