// Host-side argument rules of cnr_obj_train / cnr_obj_workspace_bytes (obj_fused.hip), in plain C++ so that a stand-alone host
// program can run them under the address and undefined-behaviour sanitizers (tests/obj_args_main.cpp): what is refused here is
// refused before anything is launched.
#pragma once
#include <stdint.h>

namespace cnr_obj {
constexpr int MAX_S = 64;             // one ray per wave in the composite, whole rays per 64-sample tile
constexpr int E_ARG = -1;             // CNR_E_ARG

#ifdef __HIPCC__
#define CNR_OBJ_HD __host__ __device__
#else
#define CNR_OBJ_HD
#endif
// One owner's workspace (an object of cnr_obj_train, a candidate of cnr_code_fit), the layout both kernels and the host's word
// count share: z | pts | sigma | rgb | gt_rgb | gt_depth | rows | depth_mask, labels (bytes)
struct Workspace { float *z, *pts, *sig, *rgb, *gtc, *gtd; int* rows; uint8_t *dm, *lab; };
CNR_OBJ_HD inline Workspace carve(uint32_t* ws, int R, int S) {
  const int64_t RS = (int64_t)R * S;
  Workspace w;
  w.z = reinterpret_cast<float*>(ws);
  w.pts = w.z + RS;
  w.sig = w.pts + 3 * RS;
  w.rgb = w.sig + RS;
  w.gtc = w.rgb + 3 * RS;
  w.gtd = w.gtc + 3 * R;
  w.rows = reinterpret_cast<int*>(w.gtd + R);
  w.dm = reinterpret_cast<uint8_t*>(w.rows + R);
  w.lab = w.dm + R;
  return w;
}
// 4-byte words of carve()'s blocks: z | pts | sigma | rgb (8 R S) | gt_rgb | gt_depth | rows (5 R) | depth_mask, labels
// (2 R bytes); a multiple of 4 words, so that every owner's block starts 16-byte aligned
inline int64_t ws_words(int R, int S) {
  const int64_t RS = (int64_t)R * S;
  return (8 * RS + 5 * (int64_t)R + (2 * (int64_t)R + 3) / 4 + 3) & ~(int64_t)3;
}
inline int64_t workspace_bytes(int N, int R, int S) {
  if (N <= 0 || R <= 0 || S <= 0 || S > MAX_S) return E_ARG;
  int64_t bytes;      // (R S <= 2^37: ws_words cannot overflow; the product with N can)
  if (__builtin_mul_overflow((int64_t)N * 4, ws_words(R, S), &bytes)) return E_ARG;
  return bytes;
}
struct Required {      // the pointers that may not be NULL
  const void *rgbs, *depth, *dirs_c, *T, *pool_off, *d_state, *theta, *exp_avg, *exp_avg_sq, *losses, *flags, *workspace;
};
// 0, or E_ARG: a required pointer NULL, N <= 0, R <= 0, n1 < 0, n2 <= 0, S > 64, a segment shorter than R, scale <= 0, a partial
// parity set (rows, u, g: all three or none), a misaligned or short workspace
inline int check_args(const Required& p, int64_t min_pool_rows, int N, int R, int n1, int n2, float scale, const void* rows,
                      const void* u, const void* g, int64_t workspace_bytes_given) {
  if (!p.rgbs || !p.depth || !p.dirs_c || !p.T || !p.pool_off || !p.d_state || !p.theta || !p.exp_avg || !p.exp_avg_sq || !p.losses ||
      !p.flags || !p.workspace)
    return E_ARG;
  if (N <= 0 || R <= 0 || n1 < 0 || n2 <= 0 || n1 > MAX_S || n2 > MAX_S || n1 + n2 > MAX_S) return E_ARG;
  if (min_pool_rows < R || !(scale > 0.f)) return E_ARG;
  if ((rows == nullptr) != (u == nullptr) || (u == nullptr) != (g == nullptr)) return E_ARG;
  if (((uintptr_t)p.workspace & 15) != 0 || workspace_bytes_given < workspace_bytes(N, R, n1 + n2)) return E_ARG;
  return 0;
}
}  // namespace cnr_obj
