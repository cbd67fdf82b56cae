/*
 * cnr_hip.h -- C-ABI of libcnr_hip.so: MI355X (gfx950) kernels for the volumetric-rendering
 * train-step hot path of Taekbum/category-nerf-reconstruction-official.
 *
 * The reference is pure Python/PyTorch: there is no FFI to replace.  Each entry
 * point below therefore cites the reference *function* whose arithmetic it implements; the Python
 * binding (category-nerf-reconstruction-official_amd/_C.py, ctypes) sits under the reference's own
 * call surface (trainer.py / scene_cateogries.py / embedding.py / model.py / render_rays.py /
 * loss.py).  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to caller-allocated, contiguous, row-major memory;
 *     f32 unless the name says otherwise.  No hidden allocation, no host sync, no global state.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream).
 *   - return 0 on success, a CNR_E_* code (<0) for argument errors, or a positive hipError_t.
 *   - C = classes (the functorch vmap axis of train.py:154-155), R = rays per class,
 *     S = samples per ray, N = R*S, L = latent dim, E = 129 = E1 (87) + E2 (42).
 */
#ifndef CNR_HIP_H
#define CNR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CNR_OK 0
#define CNR_E_ARG (-1)     /* bad size / null pointer                                  */
#define CNR_E_SHAPE (-2)   /* shape not supported by this kernel (see function doc)    */
#define CNR_E_ALIGN (-3)   /* pointer not aligned as documented                        */

#define CNR_E1 87
#define CNR_E2 42
#define CNR_E 129
#define CNR_W 32
#define CNR_NDIR 21
#define CNR_NFREQ 6
/* fp32 trunk blob: the 10 per-sample Linear layers of CodeNeRF (src/model.py:35-54) in
 * state_dict order, each as weight (out x in, row-major) followed by bias (out):
 *   encoding_xyz.0 87->32 | shape_layer_1.0 32->32 | shape_layer_2.0 32->32 | cat_layer.0 119->32
 *   encoding_shape 32->32 | sigma.0 32->1 | encoding_viewdir.0 74->32 | texture_layer_1.0 32->32
 *   rgb.0 32->16 | rgb.2 16->3                                              = 13 892 floats   */
#define CNR_TRUNK_PARAMS 13892
/* latent slots of zlat (.., 4, 32): post-ReLU outputs of the four latent layers, per ray:
 *   0 shape_latent_layer_1 | 1 cat_latent_layer | 2 shape_latent_layer_2 | 3 texture_latent_layer_1 */
#define CNR_NLAT 4

/* library / device probe: returns CNR_OK and fills n_cu, lds_bytes when a gfx950 device is current */
int cnr_version(void);
int cnr_device_info(int* n_cu, int* lds_bytes, int* gcn_arch_is_gfx950);

/* ---- a1: cameraInfo.get_rays_dirs (src/scene_cateogries.py:613-629) --------------------------------------------------
 * dirs (W,H,3): dirs[w][h] = ((w - cx) / fx, (h - cy) / fy, 1) -- indexed [w, h] (the reference transposes images at load),
 * NOT normalised (z-depth convention).  Correctly rounded fp32 subtraction and division: bit-equal to the reference. */
int cnr_camera_rays(float* dirs, int W, int H, float fx, float fy, float cx, float cy, void* stream);

/* ---- a2-a5: ray transform + depth-guided sampling (src/scene_cateogries.py:24-47, 51-96, 453-546)
 * One pool slice of R rays (per class; C slices batched).  Inputs:
 *   rgbs  (C,R,4) u8  [r,g,b,state]      depth (C,R)      dirs_c (C,R,3)     T (C,R,4,4)
 *   u     (C,R,n1+n2) uniform [0,1) draws, g (C,R,n2) N(0,(eps/3)^2) draws  (parity mode), or both
 *         NULL with `seed`/`offset` != 0 for in-kernel Philox draws (perf mode).  n2 <= 128 in either mode.  In-kernel draws
 *         need S = n1 + n2 <= 256 as well (CNR_E_SHAPE beyond, here and in cnr_step_prologue / cnr_bg_tail_sample; nothing is
 *         launched): lane l of the ray with Philox index i draws from Philox4x32-10(key = seed) at the counter
 *         (low 64 bits i * 64 + l, high 64 bits h).  With o = offset + 4 * d_state[1] (d_state[1] counted only with pool_rows > 0):
 *         h = o ^ 0x9E3779B97F4A7C15 gives the Gaussian draws of elements l (words 0, 1) and l + 64 (words 2, 3);
 *         h = o + 1 + b, word 0, gives the uniform draw of column 64 b + l.  A step owns the four high words o + 1 .. o + 4,
 *         so a fifth column block (S > 256) would be the next step's first.  Recorded draws have no such limit.
 *   world_frame: 0 -> origin_dirs_O (T is T_CO, inverted in-kernel, sim3 closed form is NOT assumed:
 *         a general 3x3 inverse is used), 1 -> origin_dirs_W (T is T_WC).
 *   max_bound (C,) : per-class max(depth) over the slice (reference :486); computed by
 *         cnr_sample_maxdepth below (or by the previous step's cnr_step_epilogue) so that no host sync is
 *         needed; NULL: every wave takes the maximum itself (same value, R extra loads per ray).
 * Outputs: z (C,R,S) with S = n1+n2, pts (C,R,S,3), origins (C,R,3) and dirs_o (C,R,3) (may be NULL),
 *   gt_rgb (C,R,3) f32 already /255 (train.py:144), gt_depth (C,R) copy of the slice's depth (may be
 *   NULL), depth_mask (C,R) u8, labels (C,R) u8; ray_row (C,R) i32 = pool_indices[slice] + c * n_obj, the row of
 *   each ray in class-major (C*n_obj, ...) code / bias-row tables (NULL to skip; pool_indices is (C,R) or,
 *   with pool_rows > 0, the (C,pool_rows) int64 base). */
/* cnr_sample_rays, max_bound_slices = k > 1: max_bound is a (C, k) table over the epoch's slices (cnr_slice_maxdepth), indexed on
 * the device by d_state[0] / R -- no per-step maximum launch; 0 or 1: one value per class for this step's slice. */
int cnr_sample_maxdepth(const float* depth, float* max_bound, const int64_t* d_state, int64_t pool_rows,
                        const int* perm, int C, int R, void* stream);
int cnr_sample_rays(const uint8_t* rgbs, const float* depth, const float* dirs_c, const float* T,
                    const float* u, const float* g, uint64_t seed, uint64_t offset,
                    const int64_t* d_state, int64_t pool_rows,
                    const float* max_bound, int world_frame, int C, int R, int n1, int n2,
                    float eps, float stop_eps, float min_bound,
                    float* z, float* pts, float* origins, float* dirs_o,
                    float* gt_rgb, float* gt_depth, uint8_t* depth_mask, uint8_t* labels,
                    const int64_t* pool_indices, int n_obj, int* ray_row, const int* perm, int max_bound_slices,
                    void* stream);
/* Device-resident step state int64[3] = {pool cursor (rows), rng step, optimiser step}.  With pool_rows > 0
 * the four pool pointers above are the BASES of (C, pool_rows, ...) pools and the slice starts at row
 * d_state[0] (src/scene_cateogries.py:422-431's i_batch); the Philox offset advances by 4 * d_state[1].
 * cnr_step_advance adds (add_rows, 1, 1): a captured hipGraph of the train step replays unchanged.
 * perm (C,pool_rows) i32, optional with pool_rows > 0: row r of the slice is pool row perm[c][cursor + r] -- the
 * per-epoch reshuffle (src/scene_cateogries.py:439-449) becomes a new permutation instead of moving the pool. */
int cnr_step_advance(int64_t* d_state, int64_t add_rows, void* stream);

/* ---- a8: UniDirsEmbed (src/embedding.py:82-92).  x (C,N,3), B (C,21,3) -> e (C,N,129).
 * e[0:3] = x/scale ; e[3+21k+j] = sin(pi * 2^k * (B_j . x/scale)), k = 0..5.
 * bwd: de (C,N,129) -> dB (C,21,3) (accumulated with atomics: zero it first), dx NULL or (C,N,3). */
int cnr_pe_fwd(const float* x, const float* B, float* e, int C, int64_t N, float scale, void* stream);
int cnr_pe_bwd(const float* x, const float* B, const float* de, float* dB, float* dx,
               int C, int64_t N, float scale, void* stream);

/* ---- a9: CodeNeRF trunk, exact fp32 (src/model.py:56-84 with do_cat=True, noise_std=None).
 * e (C,R,S,129), zlat (C,R,4,32) post-ReLU latent-layer outputs per ray (slots above),
 * trunk (C,13892) -> sigmas (C,R,S) (= raw*10), rgbs (C,R,S,3).
 * bwd recomputes the forward, then: dsig (C,R,S), drgb (C,R,S,3) ->
 *   de (C,R,S,129), dzlat (C,R,4,32) and dtrunk (C,13892); dzlat/dtrunk are ACCUMULATED (zero first). */
int cnr_mlp_fwd_f32(const float* e, const float* zlat, const float* trunk, float* sigmas, float* rgbs,
                    int C, int R, int S, void* stream);
int cnr_mlp_bwd_f32(const float* e, const float* zlat, const float* trunk,
                    const float* dsig, const float* drgb,
                    float* de, float* dzlat, float* dtrunk, int C, int R, int S, void* stream);

/* ---- a11-a13: occupancy_activation + occupancy_to_termination + render x4
 * (src/render_rays.py:3-7,25-33,46-50 ; src/loss.py:41-48).  NR = C*R rays.
 * alpha (NR,S), color (NR,S,3), z (NR,S) -> term (NR,S) [may be NULL], depth, var, opacity (NR,), rgb (NR,3).
 * bwd: d_depth, d_opacity (NR,), d_rgb (NR,3) [var is detached in the reference] and optional
 * d_term (NR,S) [NULL = none] -> d_alpha (NR,S), d_color (NR,S,3).
 * in_is_occ = 1: `alpha` already holds occupancies (occupancy_to_termination called on its own, as
 * src/trainer.py:147 / src/category_registration.py:152 do); d_alpha is then d/d(occupancy).
 * color/z and the outputs that need them may be NULL. */
int cnr_composite_fwd(const float* alpha, const float* color, const float* z, float* term,
                      float* depth, float* var, float* rgb, float* opacity,
                      int64_t NR, int S, int in_is_occ, void* stream);
int cnr_composite_bwd(const float* alpha, const float* color, const float* z,
                      const float* d_depth, const float* d_rgb, const float* d_opacity,
                      const float* d_term, float* d_alpha, float* d_color,
                      int64_t NR, int S, int in_is_occ, void* stream);

/* ---- a14-a15 fused: masks + L1 losses + masked means + their gradient w.r.t. the rendered values
 * (src/loss.py:18-74, src/render_rays.py:52-95).  Per class c: mask counts are reduced in-kernel
 * (no host sync, no workspace).  Reference quirk kept: if ANY class has an empty mask for a term, that term is
 * zero (no gradient) for ALL classes (render_rays.py:67-72).
 * inputs (C,R): depth, var, opacity, gt_depth ; rgb, gt_rgb (C,R,3) ; labels, depth_mask (C,R) u8.
 * outputs: losses (3,C) [depth,color,opacity]; flags (C,) i32: bit0 = "loss explode" (> 1e5,
 *   render_rays.py:87-89 -- reported, never exit()), bits1-3 = the depth / colour / opacity term was
 *   zeroed because some class has an empty mask, bit4 (fused trainer only) = the field backward clipped a scaled
 *   gradient (cnr_step_tail); d_depth/d_opacity (C,R), d_rgb (C,R,3) = dLoss/d(render),
 *   already multiplied by color_scaling / opacity_scaling and by `grad_scale`. */
int cnr_loss_fwd_bwd(const float* depth, const float* var, const float* rgb, const float* opacity,
                     const float* gt_depth, const float* gt_rgb, const uint8_t* labels,
                     const uint8_t* depth_mask, float color_scaling, float opacity_scaling,
                     float grad_scale, float* losses, int32_t* flags,
                     float* d_depth, float* d_rgb, float* d_opacity, int C, int R, void* stream);

/* ---- a18: AdamW on one flat fp32 buffer (train.py:40,183; torch.optim.AdamW semantics,
 * amsgrad=False, maximize=False).  step_count is the 1-based step number held on the host, or, when
 * d_state != NULL, the step is d_state[2] + 1 read on the device. */
int cnr_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                   float lr, float beta1, float beta2, float eps, float weight_decay,
                   int64_t step_count, float grad_unscale, const int64_t* d_state, void* stream);

/* ---- a7 + latent layers over the fused trainer's flat parameter rows (csrc/latent.hip).  theta / grad: (C,
 * class_stride) floats, each row [trunk 13892 | ...]; off_* = float offsets of latent W (4,32,L), latent b (4,32),
 * shape codes (n_obj,L), texture codes (n_obj,L) inside a row.  fwd -> zl (C*n_obj,4,32) post-ReLU latent outputs,
 * biasrows (C*n_obj,4,32).  bwd: dbiasrows -> grad rows: latent W/b and code entries are WRITTEN, the trunk's
 * Wt_k[:, :32] / bt_k entries are ADDED (cnr_field_bwd's dtrunk must already be there); the code-norm regulariser
 * reg_scale * code / ||code|| (src/loss.py:5-15, train.py:165-167) is included when n_obj > 1. */
int cnr_latent_fwd(const float* theta, int64_t class_stride, int64_t off_latW, int64_t off_latb,
                   int64_t off_shape, int64_t off_tex, int L, int n_obj, int C, float* zl, float* biasrows,
                   void* stream);
int cnr_latent_bwd(const float* theta, int64_t class_stride, int64_t off_latW, int64_t off_latb,
                   int64_t off_shape, int64_t off_tex, int L, int n_obj, int C, const float* zl,
                   const float* dbiasrows, float reg_scale, float* grad, const int* n_obj_cls, void* stream);
/* n_obj_cls (optional, (C,) int32 on the device; also cnr_step_tail / cnr_step_grad): the number of objects each class really
 * has when classes differ (train.py:92-96): rows n_obj_cls[c] .. n_obj - 1 of class c are padding (no ray refers to them); the
 * regulariser applies to a class's real rows, and only when it has more than one object (src/loss.py:5-15).  NULL: n_obj. */

/* ================= fused f16-MFMA field path (a8 + a9 in one launch) ================================
 * Packed operand image per class, produced on device from the fp32 trunk blob: forward A fragments,
 * fp32 constants, transposed (backward) A fragments -- layout contract in csrc/fused_common.h.
 * The four latent layers and the code tables stay in PyTorch (per-object work);
 * they reach the kernels as effective bias rows
 *     biasrows[row][slot][32] = W_l . relu(latent_l(code[row])) + b_l ,
 *     slot 0 shape_layer_1 | 1 cat_layer (first 32 columns) | 2 shape_layer_2 | 3 texture_layer_1
 * (row = object, or ray when codes are per ray) because W (a + z) + b = W a + (W z + b).
 * ray_row (C*R,) int32 maps a ray to its row (NULL: row = ray). */
int64_t cnr_pack_bytes(void);
int cnr_pack_weights(const float* trunk, void* packed, int C, void* stream);

/* pts (C,R,S,3), B (C,21,3), packed (C,cnr_pack_bytes()), biasrows (rows,4,32) -> sigmas (C,R,S) = raw*10,
 * rgbs (C,R,S,3).  f16 MFMA operands / fp32 accumulate, fp32 PE, fp32 sigma head.  Any S. */
/* Precise geometry branch (packed_lo != NULL in cnr_field_fwd / cnr_field_fwd_render / cnr_field_train): the layers
 * between the sample position and the x10 occupancy logit (encoding_xyz, shape_layer_1, cat_layer, shape_layer_2,
 * encoding_shape; src/model.py:56-75) are computed as THREE f16 products per fragment,
 *     W x ~= Wh xh + Wl xh + Wh xl,   Wh = f16(W), Wl = f16(W - Wh), xh = f16(x), xl = f16(x - xh),   fp32 accumulate,
 * i.e. with ~22 mantissa bits on both operands; the colour branch stays plain f16.  Needed for north_star's 1e-3 on the
 * occupancy of TRAINED models: the logit reaches several hundred, and plain f16 operands then give 1.8e-3 .. 2.0e-3
 * (weights and activations contribute equally; splitting either alone leaves 1.2e-3 .. 1.6e-3), this form 2e-6.
 * packed_lo: (C, cnr_pack_lo_bytes()) = the 20 residual fragments Wl of those layers, from cnr_pack_weights_lo(trunk
 * (C,13892), ...) or cnr_step_prologue.  The backward's data-gradient chain uses f16(W) alone. */
int64_t cnr_pack_lo_bytes(void);
int cnr_pack_weights_lo(const float* trunk, void* packed_lo, int C, void* stream);

/* Class strides (floats; 0 = dense): B_stride between the (21,3) direction matrices of consecutive classes,
 * dtrunk_stride / dB_stride between the per-class gradient blocks -- so that B, dtrunk and dB may be views of a flat
 * (C, P) parameter / gradient buffer (the fused trainer's layout) with no gather or scatter copies. */
int cnr_field_fwd(const float* pts, const float* B, const void* packed, const float* biasrows,
                  const int* ray_row, float scale, float* sigmas, float* rgbs, int C, int R, int S,
                  int64_t B_stride, const void* packed_lo,
                  void* stream);

/* Backward of cnr_field_fwd: cnr_field_bwd_pipe, declared below beside the one-launch step body it shares its kernel with
 * (the block-split cnr_field_bwd of rounds 1-3 is gone).  Size of its per-workgroup records: */
int64_t cnr_field_bwd_workspace_bytes(int C, int max_blocks);

/* ---- dense layers of the background model, OccupancyMap (src/model.py:86-155) -----------------
 * y (M,N) = act(x (M,K) W^T + b), W (N,K) row-major as torch.nn.Linear stores it, relu != 0: act = ReLU.
 * Exact fp32 on the matrix core (v_mfma_f32_32x32x2_f32: fp32 products, fp32 accumulation).
 * Backward: dpre = dy * (y > 0) (relu) or dy; dx (M,K) = dpre W (NULL to skip), dW (N,K) = dpre^T x, db (N,) =
 * column sums of dpre (NULL to skip); all three OVERWRITTEN.  y is only read when relu != 0.
 * workspace: >= cnr_dense_bwd_workspace_bytes(M, K, N) bytes (0 for M <= 256): the dW product is split over
 * chunks of samples whose partial results are added in a fixed order (reproducible, no atomics). */
int cnr_dense_fwd(const float* x, const float* W, const float* b, float* y, int M, int K, int N, int relu,
                  int f16_operands, void* stream);
int64_t cnr_dense_bwd_workspace_bytes(int M, int K, int N);
int cnr_dense_bwd(const float* x, const float* W, const float* y, const float* dy, float* dx, float* dW, float* db,
                  int M, int K, int N, int relu, void* workspace, int64_t workspace_bytes, int f16_operands,
                  float grad_scale, void* stream);
/* f16_operands != 0: both operands of every product are rounded to f16 as they are staged in LDS and the matrix instruction
 * is v_mfma_f32_32x32x16_f16 (fp32 accumulation, fp32 results): the f16 tier of the background model.  In the backward the
 * gradient operand is multiplied by grad_scale (a power of two, the loss scale of the f16 chain; <= 0: 1) on the way in and
 * the products by 1 / grad_scale on the way out. */

/* ---- ray-pool construction from frames (src/scene_cateogries.py:164-260, 262-325) ------------
 * images (F,W,H,3) u8, depth (F,W,H) f32, obj_mask (F,W,H) i32 (instance id per pixel, -1 unknown), rays_dir (W,H,3):
 * the frames of one scene stacked in HBM.  crops (n_crops,8) i32 = {frame slot, instance id, object index, w0, w1,
 * h0, h1, frame index in the instance's own frame list}; crop_offset (n_crops + 1) i64 = exclusive prefix sum of the crop areas; T_crop (n_crops,4,4) = the pose
 * every ray of the crop carries (T_co = inv(T_wc) T_obj, or T_wc for the background / a single object).
 * perm (N,) i64 or NULL: output row r is source row perm[r] (the reference's global shuffle x = x[shuffled_idx]).
 * Outputs, N = crop_offset[n_crops] rows: rgbs (N,4) u8 [r,g,b,state], depth (N,), dirs (N,3), T (N,4,4) (NULL to
 * skip), indices (N,) i64 = object index (NULL to skip), frame (N,) i64 = that frame index (NULL to skip). */
int cnr_gather_pool(const uint8_t* images, const float* depth, const int32_t* obj_mask, const float* rays_dir,
                    const float* T_crop, const int32_t* crops, const int64_t* crop_offset, const int64_t* perm, int W,
                    int H, int n_crops, int64_t N, uint8_t* rgbs, float* depth_out, float* dirs, float* T_out,
                    int64_t* indices, int64_t* frame_out, void* stream);

/* Parameter-only work of one fused-trainer step in ONE launch, three independent jobs side by side in the grid:
 * cnr_pack_weights (trunk of class c at theta + c * class_stride + off_trunk), cnr_latent_fwd (same arguments), and
 * a zero fill of zero_buf[0 .. zero_count) (the gradient buffers; 16-B aligned; zero_count 0 to skip). */
int cnr_param_prep(const float* theta, int64_t class_stride, int64_t off_trunk, int64_t off_latW, int64_t off_latb,
                   int64_t off_shape, int64_t off_tex, int L, int n_obj, int C, void* packed, float* zl,
                   float* biasrows, float* zero_buf, int64_t zero_count, void* stream);

/* cnr_field_fwd and cnr_render_loss in ONE launch for S in {32, 64, 96, 128}: a wave owns whole rays (S / 32
 * consecutive tiles), composites them in registers and writes d_sigmas / d_colors (and the optional renders) instead of
 * sigmas / colours.  Arguments as the two calls; results agree with them to fp32 summation order (lane sums run over
 * 32-lane tiles here).  workspace >= cnr_field_fwd_render_workspace_bytes(C, R, S): per-block loss partials for
 * cnr_render_loss_finish / cnr_step_tail, which must be told rl_blocks = cnr_field_fwd_render_blocks(R, S).
 * Returns CNR_E_SHAPE for any other S (use the two calls). */
int cnr_field_fwd_render_blocks(int R, int S);
int64_t cnr_field_fwd_render_workspace_bytes(int C, int R, int S);
int cnr_field_fwd_render(const float* pts, const float* B, const void* packed, const float* biasrows,
                         const int* ray_row, float scale, const float* z, const float* gt_depth, const float* gt_rgb,
                         const uint8_t* labels, const uint8_t* depth_mask, float color_scaling, float opacity_scaling,
                         float grad_scale, float* d_sigmas, float* d_colors, float* depth, float* var, float* rgb,
                         float* opacity, int C, int R, int S, int64_t B_stride, void* workspace,
                         int64_t workspace_bytes, const void* packed_lo, const float* counts_tab,
                         const int64_t* d_state, void* stream);

/* Mask counts of every slice of an epoch in one launch (the per-step counts of src/render_rays.py:66-95 depend on the pool
 * rows only: label = pool state, depth mask = depth > min_bound): out (slices, C + 1, 4) floats,
 *   out[s][c] = {#(valid depth & label != 0), #(label != 0), #(label != 2), 0} over rows perm[c][s R .. s R + R) of class c,
 *   out[s][C] = {1 if ANY class has a zero depth / colour / opacity count in slice s, ..., ..., 0}   (render_rays.py:67-72).
 * cnr_field_fwd_render / cnr_render_loss take such a table as `counts_tab` (NULL: they count the step's labels
 * themselves) and read entry d_state[0] / R (d_state NULL: entry 0).  The host may combine tables between GPUs before
 * use -- sum the counts of ray shards of one class, or the flags of class shards -- which is how N ranks x R rays equal
 * one rank x N R rays, and how the empty-mask rule spans ranks, with no collective inside the step. */
int cnr_slice_maskcounts(const uint8_t* rgbs, const float* depth, const int* perm, int64_t pool_rows, int C, int R,
                         int slices, float min_bound, float* out, void* stream);

/* The epoch shuffle in one launch: perm (C, pool_rows) i32, perm[c] = a pseudo-random permutation of [0, pool_rows) that is a
 * function of (seed, epoch, class id) only -- class id = class_ids[c] (device, C entries) or c when NULL -- so the ranks of a
 * class-sharded run produce the same order for a class without drawing each other's (the reference reshuffles with
 * torch.randperm, src/scene_cateogries.py:439-449; the order is not a parity target).  A keyed 6-round Feistel
 * bijection, cycle-walked into range.  state_cursor != NULL: the launch also sets state_cursor[0] = cursor0 (the pool cursor of
 * the device step state starts the epoch).  pool_rows <= 2^30. */
int cnr_epoch_perm(int* perm, int64_t pool_rows, int C, uint64_t seed, uint64_t epoch, const int* class_ids,
                   int64_t* state_cursor, int64_t cursor0, void* stream);

/* Max depth of every slice of an epoch in one launch: out[c][s] = max over r < R of depth[c][perm[c][s R + r]]
 * (perm NULL: identity), s < slices, slices * R <= pool_rows.  cnr_step_prologue takes such a table as max_bound when
 * max_bound_slices = slices > 1 and indexes it with the device cursor / R -- the fused trainer fills it once per
 * reshuffle instead of computing the next slice's maximum in every step's last launch. */
int cnr_slice_maxdepth(const float* depth, const int* perm, int64_t pool_rows, int C, int R, int slices, float* out,
                       void* stream);

/* ---- versioned argument blocks -----------------------------------------------------------------------------------------
 * The three launches of the fused trainer's step (cnr_step_prologue -> cnr_field_train -> cnr_step_tail) take their
 * arguments as ONE struct by pointer instead of 35-50 positional values: `struct_size` = sizeof(the struct) and
 * `abi_version` = CNR_ABI_VERSION come first and the entry point returns CNR_E_ARG for any other value, so a caller
 * compiled (or a ctypes table written) against another revision of this header is refused instead of reading shifted
 * fields.  Field meaning is the positional entry points' of the calls they fuse (cnr_param_prep / cnr_sample_rays, ...). */
#define CNR_ABI_VERSION 3

/* cnr_param_prep and cnr_sample_rays side by side in ONE launch (max_bound must be given here, max_bound_slices = 0 or 1
 * for the per-class form): the sampler needs the ray pool and the step state only, so the first node of the fused
 * trainer's step runs it beside the parameter-only jobs instead of after them.  packed_lo (optional,
 * (C, cnr_pack_lo_bytes())): the residual image of the geometry branch (cnr_pack_weights_lo) is built in the same launch.
 * rgbs = NULL: the parameter-only jobs without the sampler blocks (a host that samples elsewhere, e.g. on another stream). */
typedef struct cnr_step_prologue_args {
  uint32_t struct_size;
  uint32_t abi_version;
  const float* theta;
  int64_t class_stride;
  int64_t off_trunk;
  int64_t off_latW;
  int64_t off_latb;
  int64_t off_shape;
  int64_t off_tex;
  int32_t L;
  int32_t n_obj;
  int32_t C;
  void* packed;
  void* packed_lo;
  float* zl;
  float* biasrows;
  float* zero_buf;
  int64_t zero_count;
  const uint8_t* rgbs;
  const float* depth;
  const float* dirs_c;
  const float* T;
  const float* u;
  const float* g;
  uint64_t seed;
  uint64_t offset;
  const int64_t* d_state;
  int64_t pool_rows;
  const float* max_bound;
  int32_t world_frame;
  int32_t R;
  int32_t n1;
  int32_t n2;
  float eps;
  float stop_eps;
  float min_bound;
  float* z;
  float* pts;
  float* origins;
  float* dirs_o;
  float* gt_rgb;
  float* gt_depth;
  uint8_t* depth_mask;
  uint8_t* labels;
  const int64_t* pool_indices;
  int32_t* ray_row;
  const int32_t* perm;
  int32_t max_bound_slices;
  int32_t rng_c0;
  int32_t rng_cstride;
  int32_t rng_R;
  int32_t rng_r0;
} cnr_step_prologue_args;
int cnr_step_prologue(const cnr_step_prologue_args* args, void* stream);
/* rng_*: the Philox counter of ray r of local class c is ((c * rng_cstride + rng_c0) * rng_R + rng_r0 + r) * 64 + lane,
 * i.e. the ray's index in the GLOBAL batch when classes (rng_c0 = rank, rng_cstride = ranks) or rays (rng_R = global rays
 * per class, rng_r0 = rank * R) are sharded over GPUs: N ranks then draw exactly the samples one rank would.  All zero:
 * the local index c * R + r. */

/* a11-a15 fused for the render + loss step of the fused trainer: cnr_composite_fwd -> cnr_loss_fwd_bwd ->
 * cnr_composite_bwd in ONE kernel (src/render_rays.py:3-7,25-33,46-95; src/loss.py:18-74).  Possible because the
 * gradient of the masked-mean losses w.r.t. one ray's renders needs that ray's values and the mask counts only.
 * sigmas (C,R,S) are the pre-sigmoid occupancy logits (CodeNeRF's raw * 10), colors (C,R,S,3), z (C,R,S).
 * Outputs: d_sigmas (C,R,S), d_colors (C,R,S,3) = dL/dsigmas, dL/dcolors of
 *   sum_c depth + color_scaling * color + opacity_scaling * opacity,  times grad_scale,
 * bit-identical to the three-call sequence; depth, var (C,R), rgb (C,R,3), opacity (C,R): the renders, each
 * optional (NULL to skip); per-block partial sums of the three loss terms into `workspace`
 * (>= cnr_render_loss_workspace_bytes(C, R) bytes).  S <= 512.
 * cnr_render_loss_finish turns those partials into losses (3,C) and flags (C), exactly as cnr_loss_fwd_bwd
 * defines them (fixed summation order, no float atomics).  It only needs the stream order after
 * cnr_render_loss, so a trainer can run it on a side stream beside the field backward. */
int64_t cnr_render_loss_workspace_bytes(int C, int R);
int cnr_render_loss(const float* sigmas, const float* colors, const float* z, const float* gt_depth,
                    const float* gt_rgb, const uint8_t* labels, const uint8_t* depth_mask, float color_scaling,
                    float opacity_scaling, float grad_scale, float* d_sigmas, float* d_colors, float* depth,
                    float* var, float* rgb, float* opacity, int C, int R, int S, void* workspace,
                    int64_t workspace_bytes, const float* counts_tab, const int64_t* d_state, void* stream);
int cnr_render_loss_finish(const void* workspace, float* losses, int32_t* flags, int C, int R, int rl_blocks,
                           void* stream);   /* rl_blocks: partials per class, 0 = cnr_render_loss's own count */
/* Last node of the fused trainer's captured step, one launch: cnr_render_loss_finish, then (next_max_bound !=
 * NULL) cnr_sample_maxdepth for the NEXT step's slice [cursor + add_rows, + R) of the (C,pool_rows) depth pool,
 * then cnr_step_advance(d_state, add_rows).  The next step's cnr_sample_rays reads next_max_bound. */
int cnr_step_epilogue(int64_t* d_state, int64_t add_rows, const void* workspace, float* losses, int32_t* flags,
                      const float* depth, int64_t pool_rows, const int* perm, float* next_max_bound, int C, int R,
                      void* stream);

/* cnr_adamw_step and cnr_step_epilogue side by side in ONE launch, for a step state that ping-pongs between two
 * int64[3] buffers: every kernel of step k reads state_cur, this launch writes state_next = state_cur + (add_rows,
 * 1, 1); the caller swaps the two for step k + 1 (two captured graphs, or a pointer swap in eager mode).  With the
 * current state read-only during the launch, the AdamW blocks (optimiser step = state_cur[2] + 1) and the epilogue
 * block need no ordering.  Arguments as in cnr_adamw_step / cnr_step_epilogue. */
int cnr_adamw_epilogue(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                       float beta1, float beta2, float eps, float weight_decay, float grad_unscale,
                       const int64_t* state_cur, int64_t* state_next, int64_t add_rows, const void* workspace,
                       float* losses, int32_t* flags, const float* depth, int64_t pool_rows, const int* perm,
                       float* next_max_bound, int C, int R, void* stream);

/* The tail of the fused trainer's step in ONE launch: cnr_latent_bwd (do_latent != 0), AdamW on the flat parameter
 * buffer and cnr_step_epilogue, for PING-PONG parameters and step state: every kernel of step k reads theta_in /
 * state_cur, this launch writes theta_out / state_next (AdamW out of place), the caller swaps them for step k + 1.
 * With nothing written that anything in the launch reads, the three jobs run side by side; a latent-path gradient
 * element is applied by the thread that produces it, and the trunk entries the latent path adds to are finished by
 * the AdamW blocks.  do_latent = 0: grad already holds the complete gradient (cnr_latent_bwd ran, e.g. before a
 * multi-GPU all-reduce) and only AdamW + epilogue run.  grad is updated to the complete gradient either way.
 * Layout arguments as cnr_latent_bwd (trunk at offset 0 of a class row, B at off_B); rl_workspace etc. as
 * cnr_step_epilogue.
 * records != NULL (with do_latent, n_obj <= 4): the launch ALSO replaces the record reduction of
 * cnr_field_bwd_pipe(..., skip_reduce = 1): `records` is that call's workspace, nwg =
 * cnr_field_bwd_pipe_blocks(...), and rows_fix the (8, C, n_obj, 4, 32) int64 table that call accumulated (2^-40 fixed
 * point, integer atomics: any order, same sum) -- zero it before every field backward.  dbiasrows then receives the
 * float form of that table.  `records` must be 16-byte aligned (the reduction loads 16 bytes at a time; a record is
 * 32 256 bytes, so every record then is): CNR_E_ARG otherwise.
 * rl_blocks: loss partials per class in rl_workspace; 0 = cnr_render_loss's own block count.
 * code_lr > 0: the shape / texture code tables are an AdamW group of their own (code_lr, code_weight_decay: train.py:40,
 * 54-64, configs' code_lr / code_weight_decay); 0 = they share lr / weight_decay. */
typedef struct cnr_step_tail_args {
  uint32_t struct_size;
  uint32_t abi_version;
  const float* theta_in;
  float* theta_out;
  float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t class_stride;
  int64_t off_B;
  int64_t off_latW;
  int64_t off_latb;
  int64_t off_shape;
  int64_t off_tex;
  int32_t L;
  int32_t n_obj;
  int32_t C;
  const float* zl;
  float* dbiasrows;
  float reg_scale;
  int32_t do_latent;
  float lr;
  float beta1;
  float beta2;
  float eps;
  float weight_decay;
  const int64_t* state_cur;
  int64_t* state_next;
  int64_t add_rows;
  const void* rl_workspace;
  float* losses;
  int32_t* flags;
  const float* depth;
  int64_t pool_rows;
  const int32_t* perm;
  float* next_max_bound;
  int32_t R;
  const void* records;
  int32_t nwg;
  const long long* rows_fix;
  int32_t rl_blocks;
  int32_t* clamp_flags;
  const int32_t* n_obj_cls;
  float code_lr;
  float code_weight_decay;
} cnr_step_tail_args;
int cnr_step_tail(const cnr_step_tail_args* args, void* stream);
/* clamp_flags (optional, (C,) int32, zero before the first step): what cnr_field_bwd_pipe raised during this step -- bit 4
 * (16) = a scaled upstream gradient |d sigma| * grad_scale exceeded 8192 and was clipped for the f16 chain; the epilogue
 * or-s the word into flags[c] and clears it. */

/* The gradient half of cnr_step_tail on its own (records reduction + latent backward + code regulariser in one launch,
 * no optimiser, no epilogue): for hosts that need the finished gradient first, e.g. to all-reduce it across GPUs.
 * Same arguments as the corresponding ones of cnr_step_tail (`records` 16-byte aligned, CNR_E_ARG otherwise); follow it (after the collective) with
 * cnr_step_tail(..., do_latent = 0, ..., records = NULL, nwg = 0, rows_fix = NULL, ...). */
int cnr_step_grad(const float* theta, float* grad, int64_t class_stride, int64_t off_B, int64_t off_latW,
                  int64_t off_latb, int64_t off_shape, int64_t off_tex, int L, int n_obj, int C, const float* zl,
                  float* dbiasrows, float reg_scale, const void* records, int nwg, const long long* rows_fix,
                  const int* n_obj_cls, void* stream);

/* Backward of cnr_field_fwd (recomputes the forward per tile): d_sigma (C,R,S) = dL/dsigmas, d_rgb (C,R,S,3) -> dtrunk
 * (C,13892), dB (C,21,3), dbiasrows (rows,4,32); all three ACCUMULATED (zero them first).  dtrunk receives no bias gradient for
 * the four latent-conditioned layers: those biases reach the kernel only through biasrows, whose gradient the caller
 * back-propagates (cnr_latent_bwd / cnr_step_tail).  grad_scale: power-of-two loss scale applied to d_sigma / d_rgb on load and
 * removed on store (the data-gradient chain runs on f16 MFMA operands); scaled d_sigma is clamped to +-8192.  S <= 240.
 * ONE field kernel + the record reduction: a workgroup is four chain waves that run forward recompute + data-gradient chain + PE
 * backward for one 32-sample tile each, plus four waves that own the weight-gradient accumulators and consume the chain waves'
 * per-layer images behind a workgroup barrier -- eight waves, two per SIMD (csrc/fused_bwd_pipe8_kernel.h).  chain_waves must be
 * 4 (kept in the signature).  max_blocks: workgroups per class (0 = 256).  workspace: caller-allocated, 16-B aligned, contents
 * irrelevant, >= cnr_field_bwd_workspace_bytes(C, max_blocks) bytes: every workgroup stores one record of partial sums into it
 * with plain stores -- 16 128 bf16 entries, each the workgroup's fp32 sum rounded once -- and a last small kernel sums the records
 * in fp32, in a fixed order: no float atomic anywhere, bitwise reproducible.
 * packed_lo (optional): the residual image the FORWARD ran with (cnr_field_fwd / cnr_field_fwd_render, precise geometry branch):
 * the recompute then forms the same activations and ReLU masks as that forward -- without it the backward of a precise forward
 * would be the gradient of the plain-f16 function.
 * Rows: ray_row REQUIRED, class-major, 1 .. 15 per class (their bias-row sums travel in the records and in rows_fix);
 * CNR_E_SHAPE otherwise -- larger classes (up to 128 objects) train on cnr_field_train, one object per tile. */
/* rows_fix (optional): per-object bias-row sums also accumulated as 2^-40 fixed point into this (8, C, n_obj, 4, 32)
 * int64 table (8 copies, a workgroup uses copy index & 7, to shorten the same-address atomic queues; caller zeroes it); skip_reduce != 0: stop after the field kernel, the caller reduces the nwg =
 * cnr_field_bwd_pipe_blocks(R, S, chain_waves, max_blocks) records per class in `workspace` itself (cnr_step_tail). */
int cnr_field_bwd_pipe_blocks(int R, int S, int chain_waves, int max_blocks);
int cnr_field_bwd_pipe(const float* pts, const float* B, const void* packed, const void* packed_lo, const float* biasrows,
                       const int* ray_row, float scale, const float* d_sigma, const float* d_rgb,
                       float grad_scale, float* dtrunk, float* dB, float* dbiasrows, int C, int R, int S,
                       int rows_per_class, int max_blocks, int chain_waves, void* workspace,
                       int64_t workspace_bytes, int64_t B_stride,
                       int64_t dtrunk_stride, int64_t dB_stride, long long* rows_fix, int skip_reduce,
                       int* clamp_flags, void* stream);

/* ---- BASELINE.json configs[4]: the field forward on the gfx950 fp8 matrix instruction (v_mfma_f32_32x32x16_fp8_fp8) ----
 * Same contract as cnr_field_fwd with OCP e4m3 operands: weights as `terms` fp8 planes of 64 W (plane p = fp8 of what planes
 * 0..p-1 left over), activations / PE features as `terms` planes of 16 x formed on the fly, terms^2 MFMAs per fragment into
 * one fp32 accumulator, fp32 sigma head.  terms in {1, 2, 3}.  `packed` is the f16 image (its fp32 constants are used),
 * `packed8` = (C, cnr_pack_fp8_bytes(terms)) from cnr_pack_weights_fp8.  Forward only: measured against the oracle, terms = 1
 * is 6e-2 on occupancy (60x outside the 1e-3 bar), 2 -> 1.8e-3, 3 -> 1.5e-4, while the f16 kernel's ONE MFMA of the same
 * rate gives 7e-4 -- which is why the train step stays on f16. */
int64_t cnr_pack_fp8_bytes(int terms);
int cnr_pack_weights_fp8(const float* trunk, void* packed8, int C, int terms, void* stream);
int cnr_field_fwd_fp8(const float* pts, const float* B, const void* packed, const void* packed8, const float* biasrows,
                      const int* ray_row, float scale, float* sigmas, float* rgbs, int C, int R, int S, int64_t B_stride,
                      int terms, void* stream);

/* ---- the step body in ONE launch: cnr_field_fwd_render + cnr_field_bwd_pipe (chain_waves = 4) fused ---------------------
 * a8-a15 forward, the loss gradient and the whole field backward (train.py:154-182 for the object branch) with ONE field
 * forward per sample (cnr_field_bwd_pipe recomputes it), no d sigma / d colour round trip through HBM and one launch less.
 * Any S <= 128: a ray occupies 16, 32, 64 or 128 padded sample slots (the smallest that holds S; slots beyond S are dead
 * lanes).  With 16 slots two rays share a 32-sample tile, one per DPP row (the reference's real batch is 10 samples per
 * ray); with 64 / 128 the ray's 2 / 4 tiles sit in neighbouring chain waves of a workgroup iteration and exchange the tile
 * products / partial renders / suffix sums of the composite through LDS.  Arguments as the two calls it replaces;
 * counts_tab (cnr_slice_maskcounts) is REQUIRED -- the kernel never counts masks --, d_state selects its entry (NULL: 0);
 * loss_scale multiplies the loss gradient (what cnr_field_fwd_render calls grad_scale), grad_scale is the power-of-two
 * scale of the f16 data-gradient chain.  Outputs: the renders (each optional), the per-workgroup gradient records in
 * `records` (>= C * cnr_field_train_blocks() * record size = cnr_field_bwd_workspace_bytes(C, blocks); reduce with
 * cnr_step_tail / cnr_step_grad, nwg = cnr_field_train_blocks()), rows_fix as cnr_field_bwd_pipe, and per-block loss
 * partials in loss_workspace (>= cnr_field_train_workspace_bytes()) for cnr_step_tail with rl_blocks =
 * cnr_field_train_blocks().
 * rows_per_class (objects per class): up to 15 travel in the kernel's row-sum blocks (and in the records); 16 .. 32 are taken
 * when a ray has at least 32 sample slots (S > 16) and rows_fix is given: a 32-sample tile then lies inside one ray, i.e.
 * belongs to one object, and its column sums go straight to the fixed-point table at that object's row (integer atomics,
 * once per workgroup iteration); the records carry no row sums then and cnr_step_tail / cnr_step_grad take all of them from
 * the table.  Returns CNR_E_SHAPE for S > 128, for more than 32 rows per class, and for more than 15 with S <= 16 or without
 * rows_fix (use the two calls). */
int cnr_field_train_blocks(int R, int S, int max_blocks, int rows_per_class);
int64_t cnr_field_train_workspace_bytes(int C, int R, int S, int max_blocks, int rows_per_class);
/* (rows_per_class: more than 15 object rows per class need one object per tile, so rays of up to 16 samples -- otherwise two
 *  to a tile -- are padded to a 32-slot tile of their own there: the block count depends on it) */
/* packed_lo (optional, (C, cnr_pack_lo_bytes()) from cnr_pack_weights_lo / cnr_step_prologue): the forward's geometry
 * branch as three products per fragment (see cnr_pack_weights_lo) -- the trainer's default; NULL: plain f16 operands. */
typedef struct cnr_field_train_args {
  uint32_t struct_size;
  uint32_t abi_version;
  const float* pts;
  const float* B;
  const void* packed;
  const void* packed_lo;
  const float* biasrows;
  const int32_t* ray_row;
  float scale;
  const float* z;
  const float* gt_depth;
  const float* gt_rgb;
  const uint8_t* labels;
  const uint8_t* depth_mask;
  const float* counts_tab;
  const int64_t* d_state;
  float color_scaling;
  float opacity_scaling;
  float loss_scale;
  float grad_scale;
  float* depth;
  float* var;
  float* rgb;
  float* opacity;
  int32_t C;
  int32_t R;
  int32_t S;
  int32_t rows_per_class;
  int32_t max_blocks;
  void* records;
  int64_t records_bytes;
  void* loss_workspace;
  int64_t loss_workspace_bytes;
  int64_t B_stride;
  long long* rows_fix;
  int32_t* clamp_flags;
} cnr_field_train_args;
int cnr_field_train(const cnr_field_train_args* args, void* stream);

/* ---- the background field's train step on f16 MFMA, fused (csrc/bg_fused.hip) ----------------------------
 * OccupancyMap(hidden 128), src/model.py:86-155, called every iteration at train.py:113-121,172-180 on R x S world-frame
 * samples (1200 x 14).  theta: the flat fp32 parameter buffer in the modules' registration order,
 *   in_layer.0 W (128,87) b | mid1.0.0 W (128,128) b | cat_layer.0 W (128,215) b | mid2.0.0 W (128,128) b | out_alpha W (1,128) b |
 *   color_linear.0 W (128,170) b | out_color W (3,128) b | B_layer.weight (21,3)          = cnr_bg_param_count() = 94 403 floats.
 * One step = cnr_bg_pack -> cnr_bg_forward -> cnr_render_loss (+ _finish) -> cnr_bg_backward -> cnr_bg_dw -> cnr_bg_tail, M = R S
 * (or, one launch less, cnr_bg_forward -> cnr_bg_backward_render -> cnr_bg_dw -> cnr_bg_tail, below):
 *   pack:     theta -> (cnr_bg_pack_bytes()) f16 MFMA fragments: forward, geometry-branch residual, transposed.
 *   forward:  pts (M,3) -> sigma (M,) = 10 raw, rgb (M,3); act (5,M,128) f16 = post-ReLU outputs of in_layer, mid1, cat_layer,
 *             mid2, color_linear; eimg (M,144) f16 = PE features (E1 in columns 0..95, E2 in 96..143).  Geometry branch
 *             (in_layer .. mid2 -> out_alpha) as three f16 products per fragment, fp32 occupancy head; colour branch plain f16.
 *   backward: d_sigma (M,), d_rgb (M,3) (already multiplied by the loss scale) -> dpre (5,M,128) f16 pre-activation gradients,
 *             records (cnr_bg_blocks(M), cnr_bg_record_floats()): per-workgroup gradients of out_color, out_alpha, B_layer.
 *   dw:       weight / bias gradients of the five 128-wide layers over sample chunks of `chunk` (a multiple of 64) samples
 *             -> partials (cnr_bg_dw_chunks(M, chunk), cnr_bg_param_count()).  d_state != NULL: the launch also advances the
 *             step state by (add_rows, 1, 1) (for steps whose backward is cnr_bg_backward_render; then pass add_rows = -1 to the tail).
 *   tail:     fixed-order sums of partials and records, x 1 / grad_scale -> grad; AdamW in place (step = d_state[2] + 1);
 *             d_state += (add_rows, 1, 1).  With d_state given to cnr_bg_backward (it then advances the state: the sampler, which
 *             reads the cursor, ran before it, the optimiser, which reads the step count, runs after it) pass add_rows = -1
 *             here: the step count is then d_state[2] as it stands and no state launch follows.
 *             packed != NULL: every weight's f16 fragment slots are refreshed by the thread that updates it (the next step then
 *             needs no cnr_bg_pack; call cnr_bg_pack once before the first step and after any outside change of theta);
 *             rl_workspace != NULL: cnr_render_loss's workspace for R rays -> losses (3,1), flags (1) (= cnr_render_loss_finish);
 *             R = 0: rl_workspace is cnr_bg_backward_render's loss workspace (one partial per backward block, nrec of them).
 * No float atomics: two runs give the same bits. */
int64_t cnr_bg_pack_bytes(void);
int cnr_bg_param_count(void);
int cnr_bg_blocks(int M);
int cnr_bg_dw_chunks(int M, int chunk);
int cnr_bg_record_floats(void);
int cnr_bg_pack(const float* theta, void* packed, void* stream);
int cnr_bg_forward(const float* pts, const float* theta, const void* packed, float scale, int M, float* sigma, float* rgb,
                   void* act, void* eimg, void* stream);   /* act = eimg = NULL: the forward alone, nothing kept for a backward
                                                              (Trainer.eval_points' meshing queries, src/trainer.py:125-151) */
int cnr_bg_backward(const float* pts, const float* theta, const void* packed, float scale, int M, const float* d_sigma,
                    const float* d_rgb, const float* rgb, const void* act, void* dpre, float* records, int64_t* d_state,
                    int64_t add_rows, void* stream);
int cnr_bg_dw(const void* act, const void* dpre, const void* eimg, int M, int chunk, float* partials, int64_t* d_state,
              int64_t add_rows, void* stream);
/* cnr_render_loss + cnr_bg_backward in ONE launch (R rays x S <= 64 samples, ray-major: sample m = ray S + s): every backward
 * workgroup first composites the (at most 32 / S + 2) rays its 32-sample tile touches -- one wave per ray, cnr_render_loss's
 * arithmetic expression for expression, so d sigma / d colour are that call's bit for bit -- and walks straight into the
 * data-gradient chain; d sigma / d colour never reach memory.  The tile that holds a ray's first sample writes its renders
 * (depth / var / rgb_render / opacity, each optional) and accounts for its loss terms: loss_workspace
 * (cnr_bg_backward_render_workspace_bytes(M)) holds one partial per workgroup, which cnr_bg_tail (rl_workspace, R = 0) turns
 * into loss values and flags.  counts_tab (cnr_slice_maskcounts, C = 1) is required; d_state (may be NULL: entry 0) is READ for
 * the cursor and not advanced here: give d_state to cnr_bg_dw.  rgb = the forward's per-sample colours.  d_sigma (M,) /
 * d_rgb (M,3), optional: the loss gradient per sample as cnr_render_loss writes it (the chain itself does not need them). */
typedef struct cnr_bg_backward_render_args {
  uint32_t struct_size;
  uint32_t abi_version;
  const float* pts;
  const float* theta;
  const void* packed;
  float scale;
  int32_t R;
  int32_t S;
  const float* sigma;
  const float* rgb;
  const float* z;
  const float* gt_depth;
  const float* gt_rgb;
  const uint8_t* labels;
  const uint8_t* depth_mask;
  const float* counts_tab;
  const int64_t* d_state;
  float color_scaling;
  float opacity_scaling;
  float grad_scale;
  const void* act;
  void* dpre;
  float* records;
  float* depth;
  float* var;
  float* rgb_render;
  float* opacity;
  float* d_sigma;
  float* d_rgb;
  void* loss_workspace;
  int64_t loss_workspace_bytes;
} cnr_bg_backward_render_args;
int64_t cnr_bg_backward_render_workspace_bytes(int M);
int cnr_bg_backward_render(const cnr_bg_backward_render_args* args, void* stream);
int cnr_bg_tail(float* theta, float* grad, float* exp_avg, float* exp_avg_sq, const float* partials, int chunks,
                const float* records, int nrec, float grad_scale, float lr, float beta1, float beta2, float eps,
                float weight_decay, int64_t* d_state, int64_t add_rows, void* packed, const void* rl_workspace, int R,
                float* losses, int32_t* flags, void* stream);

/* cnr_bg_tail with the NEXT step's sampler (cnr_sample_rays: world or object frame, device pool + cursor + permutation, in-kernel
 * Philox, C = 1) as extra blocks of the same launch: nothing in the tail reads what the sampler writes, and the step state has
 * been advanced earlier in the step (cnr_bg_dw with d_state; this entry point has cnr_bg_tail's add_rows = -1 semantics), so
 * cursor and RNG step are the next step's -- the step after then starts with cnr_bg_forward straight away.  When no whole slice
 * is left in the epoch (cursor + R > pool_rows) the sampler blocks write nothing: the host reshuffles and calls cnr_sample_rays.
 * Tail fields as cnr_bg_tail's (rl_R = its R: 0 for cnr_bg_backward_render's workspace); sampler fields as cnr_sample_rays'. */
typedef struct cnr_bg_tail_sample_args {
  uint32_t struct_size;
  uint32_t abi_version;
  float* theta;
  float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  const float* partials;
  int32_t chunks;
  const float* records;
  int32_t nrec;
  float grad_scale;
  float lr;
  float beta1;
  float beta2;
  float adam_eps;
  float weight_decay;
  void* packed;
  const void* rl_workspace;
  int32_t rl_R;
  float* losses;
  int32_t* flags;
  const uint8_t* rgbs;
  const float* depth;
  const float* dirs_c;
  const float* T;
  uint64_t seed;
  uint64_t offset;
  const int64_t* d_state;
  int64_t pool_rows;
  const float* max_bound;
  int32_t max_bound_slices;
  int32_t world_frame;
  int32_t R;
  int32_t n1;
  int32_t n2;
  float eps;
  float stop_eps;
  float min_bound;
  const int32_t* perm;
  float* z;
  float* pts;
  float* origins;
  float* dirs_o;
  float* gt_rgb;
  float* gt_depth;
  uint8_t* depth_mask;
  uint8_t* labels;
} cnr_bg_tail_sample_args;
int cnr_bg_tail_sample(const cnr_bg_tail_sample_args* args, void* stream);

/* ---- Meshing: Trainer.meshing (src/trainer.py:62-123), vis.marching_cubes (src/vis.py:6-20), make_3D_grid
 * (src/render_rays.py:97-121).  DESIGN.md §3.6.
 * vol (D,D,D) f32, C-contiguous, axis 0 = x: point (i0,i1,i2) at (i0 D + i1) D + i2, 2 <= D <= 512 (else CNR_E_SHAPE).
 * A corner is inside when v > level (NaN: outside); an edge is crossed when exactly one end is inside, and its vertex lies at
 * t = (level - v0) / (v1 - v0) clamped to [0,1] from the lower end, in index space / (D - 1).  One vertex per crossed edge,
 * owned by the edge's lower grid point; vertices sorted by (owning point, axis), faces by (cell = its min corner, table order;
 * table: csrc/mc_table.h, generated by tools/gen_mc_table.py).  ascent != 0: the right-hand face normal points towards
 * increasing values; 0: the same faces with columns 1 and 2 swapped.  Normals: np.gradient-style central differences
 * (one-sided at the border) at both ends of the edge, interpolated with t, normalised, on the faces' side (0 when zero).
 * Two steps so that the caller allocates exact outputs:
 *   workspace >= cnr_mc_workspace_bytes(D) bytes (CNR_E_SHAPE for a bad D);
 *   cnr_mc_count writes counts_out (2,) i64 = {V, F} (device memory) and keeps the classification in workspace;
 *   cnr_mc_emit, with the same vol / D / level / workspace after cnr_mc_count on the same stream, writes verts (V,3),
 *   normals (V,3), faces (F,3) i32.  V = F = 0 when no edge crosses (then do not call cnr_mc_emit). */
int64_t cnr_mc_workspace_bytes(int D);
int cnr_mc_count(const float* vol, int D, float level, void* workspace, int64_t* counts_out, void* stream);
int cnr_mc_emit(const float* vol, int D, float level, int ascent, void* workspace, float* verts, float* normals, int* faces,
                void* stream);
/* make_3D_grid(occ_range = [lo, hi], dim = D, transform, scale).view(-1, 3) in one pass: out (D^3, 3); scale (3,) or NULL,
 * transform (3,4) row-major [R | t] or NULL.  torch.linspace's two-sided formula, then * scale, then r_k . p summed x, y, z
 * left to right, then + t; 2 <= D <= 512. */
int cnr_grid_points(int D, float lo, float hi, const float* scale, const float* transform, float* out, void* stream);

/* ---- Frame parsing: the dataset loaders' get_all_frames (src/dataset.py:96-186, :273-430), src/image_transforms.py.
 * DESIGN.md §3.8.  Label frames: F frames stored (H + 2 edge) x (W + 2 edge), row-major as decoded, of int32 (label_i32 != 0)
 * or uint16; the analysed region is their centre H x W (the reference's `mw` crop).  A stored value v is id v + id_shift
 * (id_shift 0 or 1: ScanNet's raw masks); ids outside [0, id_bound) are skipped (the caller checks the bound), id_bound <=
 * 65537.  Instance table in two steps so that the caller allocates exact outputs:
 *   workspace >= cnr_frame_instances_workspace_bytes(F, id_bound) (CNR_E_SHAPE for a bad F or id_bound);
 *   cnr_frame_instances_count writes offsets_out (F + 1) i64 (device): frame f's distinct ids are entries
 *   [offsets[f], offsets[f + 1]) of a CSR table; the workspace keeps each frame's id bitmap and ranks;
 *   cnr_frame_instances_emit, same frames and arguments and workspace after _count on the same stream, writes ids (N,) i32 in
 *   ascending order per frame (np.unique's) and stats (N, CNR_FRAME_NSTAT) i32 per id: pixel count, min and max row, min and
 *   max column (region coordinates), min and max of `cls` over the id's pixels (0, 0 when cls is NULL; cls has inst's layout).
 * Integer atomics only: every run is bit-identical. */
#define CNR_FRAME_NSTAT 7
int64_t cnr_frame_instances_workspace_bytes(int F, int id_bound);
int cnr_frame_instances_count(const void* inst, int label_i32, int F, int H, int W, int edge, int id_shift, int id_bound,
                              void* workspace, int64_t* offsets_out, void* stream);
int cnr_frame_instances_emit(const void* inst, const void* cls, int label_i32, int F, int H, int W, int edge, int id_shift,
                             int id_bound, const void* workspace, const int64_t* offsets, int32_t* ids, int32_t* stats, void* stream);
/* The frame arrays of the reference's sample_dict, (W, H) after its transpose(1, 0), one thread per output pixel:
 *   obj_mask (F, W, H) i32 = the pixel's id (label frames as above, crop label_edge) when keep[its table entry] != 0, else 0;
 *   depth_out (F, W, H) f32 = depth (F, H + 2 edge, W + 2 edge) u16 * depth_scale in fp32, NaN -> 0, > max_depth -> 0;
 *   image_out (F, W, H, 3) u8 = rgb (F, H + 2 edge, W + 2 edge, 3) u8.
 * workspace and offsets: the table's, after cnr_frame_instances_count on the same label frames; keep (N,) u8. */
int cnr_frame_finish(const void* inst, int label_i32, int label_edge, const uint16_t* depth, const uint8_t* rgb, int F, int H, int W,
                     int edge, int id_shift, int id_bound, const void* workspace, const int64_t* offsets, const uint8_t* keep,
                     float depth_scale, float max_depth, int32_t* obj_mask, float* depth_out, uint8_t* image_out, void* stream);
/* cv2.resize(src, (dw, dh), INTER_LINEAR) on (F, sh, sw, 3) u8 -> (F, dh, dw, 3) u8: OpenCV's coefficients (half-pixel centres,
 * edge clamp, 11-bit fixed point) and the rounding of its vectorised vertical pass. */
int cnr_resize_linear_u8c3(const uint8_t* src, int F, int sh, int sw, uint8_t* dst, int dh, int dw, void* stream);
/* cv2.resize(src, (dw, dh), INTER_NEAREST) on (F, sh, sw) elements of elem_bytes 2 or 4 -> (F, dh, dw). */
int cnr_resize_nearest(const void* src, int elem_bytes, int F, int sh, int sw, void* dst, int dh, int dw, void* stream);

/* ---- Mesh evaluation: metric/metrics.py, metric/eval_3D_obj.py:10-39.  DESIGN.md §3.7.  Every call is bit-identical run to
 * run (no atomics; fixed reduction orders).  Points are (n,3) f32, C-contiguous.
 * Nearest-neighbour distance: dist_out[i] = min_j |q_i - p_j| (Euclidean, fp32: (q - p)^2 summed per component, the min of the
 * squares, one correctly rounded sqrt).  nq, nr >= 1 (else CNR_E_SHAPE); workspace >= cnr_nn_workspace_bytes(nq, nr). */
int64_t cnr_nn_workspace_bytes(int64_t nq, int64_t nr);
int cnr_nn_dist(const float* q, int64_t nq, const float* p, int64_t nr, float* dist_out, void* workspace, void* stream);
/* *sum_out (f64, device) = sum of dist[0..n) in a fixed order, *count_out (i64, device) = #{i : dist[i] < th}; n >= 1,
 * workspace >= cnr_dist_stats_workspace_bytes(n). */
int64_t cnr_dist_stats_workspace_bytes(int64_t n);
int cnr_dist_stats(const float* dist, int64_t n, float th, void* workspace, double* sum_out, int64_t* count_out, void* stream);
/* Triangles: verts f32 and faces (F,3) i32 into verts, or faces == NULL for a soup (verts (F,3,3): what cnr_clip_box_emit
 * writes).  area (F,) f64 = |(v1 - v0) x (v2 - v0)| / 2 in fp64, cum (F,) f64 its inclusive prefix sum; F >= 1,
 * workspace >= cnr_face_area_workspace_bytes(F). */
int64_t cnr_face_area_workspace_bytes(int64_t F);
int cnr_face_area_scan(const float* verts, const int* faces, int64_t F, void* workspace, double* area, double* cum, void* stream);
/* Area-weighted surface samples from caller-drawn uniforms u (n,3) f64 in [0,1): face = the first f with cum[f] >= u0 cum[F-1]
 * (searchsorted, side 'left'); (a, b) = (u1, u2), reflected to (1 - a, 1 - b) when a + b > 1; out[i] (f32) =
 * (v1 - v0) a + (v2 - v0) b + v0 in fp64, rounded once.  Same triangle forms as cnr_face_area_scan, cum from it. */
int cnr_sample_surface(const float* verts, const int* faces, int64_t F, const double* cum, const double* u, int64_t n,
                       float* out, void* stream);
/* The part of the triangles inside a convex box: planes (6,6) f64 rows (origin xyz, inward normal xyz); a point is kept when
 * (x - o) . n >= 0 for all six.  Each triangle is clipped in turn against the six planes (Sutherland-Hodgman, fp64) and the
 * polygon left is fan-triangulated from its first vertex; output tris (T,3,3) f32 in (face, fan) order.  Two steps as for
 * marching cubes: cnr_clip_box_count writes count_out (1,) i64 = T (device) and keeps per-workgroup offsets in workspace
 * (>= cnr_clip_box_workspace_bytes(F)); cnr_clip_box_emit, with the same inputs and workspace after it on the same stream,
 * writes tris (do not call it when T = 0). */
int64_t cnr_clip_box_workspace_bytes(int64_t F);
int cnr_clip_box_count(const float* verts, const int* faces, int64_t F, const double* planes, void* workspace,
                       int64_t* count_out, void* stream);
int cnr_clip_box_emit(const float* verts, const int* faces, int64_t F, const double* planes, void* workspace, float* tris,
                      void* stream);
/* The face index of cnr_sample_surface's search alone: face_out[i] (i32) = the first f with cum[f] >= u[3 i] cum[F-1], the last
 * face when there is none; u is the same (n,3) f64 array of draws (only u0 is read).  1 <= F < 2^31, n >= 0. */
int cnr_sample_faces(const double* cum, int64_t F, const double* u, int64_t n, int* face_out, void* stream);
/* Point-to-mesh distance, exact and brute force (tests/pointmesh_cpu.py restates it).  q (nq,3) f32; the
 * triangle forms of cnr_face_area_scan (faces == NULL: a soup).  Per query: dist_out (f32) = sqrt of the minimum over all faces
 * of the fp32 squared distance to the face's closest point, face_out (i32) = the lowest face index that attains it,
 * closest_out (nq,3) f32 or NULL = q + r with r = closest - q of that face.  fp32 without contraction, difference first
 * (ap = q - a, then dot products of ap and the edges): Ericson's seven regions with ab.bp = ab.ap - ab.ab etc., one division
 * in the vertex and edge regions, r = -(n . ap) n with the face's unit normal in the interior; a face whose fp32 edge vectors
 * are exactly parallel or zero stands for its longest edge.  Inputs must be finite.
 * nq >= 1, 1 <= F < 2^31; workspace >= cnr_point_mesh_workspace_bytes(nq, F) = align256(64 F) + chunks * align256(8 nq), where
 * chunks is the number of face chunks of the grid.  No atomics; bit-identical run to run. */
int64_t cnr_point_mesh_workspace_bytes(int64_t nq, int64_t F);
int cnr_point_mesh_dist(const float* q, int64_t nq, const float* verts, const int* faces, int64_t F, float* dist_out,
                        int* face_out, float* closest_out, void* workspace, void* stream);
/* One pass of cnr_point_mesh_dist alone, for timing: pass 1 = face records, 2 = partial minima, 3 = finish; same arguments
 * and workspace, the passes in that order give cnr_point_mesh_dist's result. */
int cnr_point_mesh_pass(const float* q, int64_t nq, const float* verts, const int* faces, int64_t F, float* dist_out,
                        int* face_out, float* closest_out, void* workspace, int pass, void* stream);
/* The same result, bit for bit, through a tile-box index that culls (DESIGN.md §3.20 "The tile-box index";
 * tests/pointmesh_index_cpu.py restates it).  Built once per mesh, used for any number of query sets; opt-in.
 * cnr_pm_index_params: *tile_faces = TILE, the faces per tile, *group_queries = GROUP, the queries per culling group.
 * cnr_pm_index_keys: keys_out[f] (i32) = the 30-bit Morton code (10 bits per axis, x the lowest bit of each triple) of the centre
 * 0.5 (min + max) of face f's box, quantised over bbox (6 f32 on the device: lo xyz, hi xyz): per axis 0 when hi - lo is not
 * a positive finite fp32 number, else min(1023, (int)(((clamp(x, lo, hi) - lo) / (hi - lo)) * 1024)), fp32 without contraction.  cnr_pm_query_keys: the same
 * of the queries themselves.  The caller sorts (stably) and passes the permutations as int64 `order` / `qorder`
 * (torch.sort's indices): position -> original index.
 * cnr_pm_index_build(verts, faces | NULL, F, keys, order, index_out): index_out (cnr_pm_index_bytes(F) = align256(64 F) +
 * align256(32 tiles) bytes, tiles = ceil(F / TILE)) receives cnr_point_mesh_dist's face records in key order, the face's original
 * index bit-cast into the sixteenth float, then one row of 8 floats per tile of TILE consecutive faces: box lo xyz, Lmax, box hi
 * xyz, the tile's first key (bit-cast); lo / hi are the exact min / max of the faces' corners, Lmax = sqrtf of the largest fp32
 * squared edge (ab, ac, bc: differences first) of the tile.
 * cnr_point_mesh_dist_indexed: q, dist_out, face_out (ORIGINAL face indices), closest_out | NULL as for cnr_point_mesh_dist, all
 * at the queries' original positions; qkeys from cnr_pm_query_keys with the index's bbox, qorder their stable order.  A group of
 * GROUP consecutive queries in key order evaluates a seed tile, then every tile t for which NOT
 * lb - 32 2^-24 (lb + Lmax_t) > sqrt(M): lb = sqrtf of the squared per-axis gaps max(lo_t - hi_g, lo_g - hi_t, 0) between the
 * tile's box and the group's, M the largest current minimum of the group's queries, re-read after every tile.  Among equal
 * minima the lowest original index wins.  workspace >= cnr_point_mesh_indexed_workspace_bytes(nq, F) = align256(4 groups),
 * groups = ceil(nq / GROUP); after the call its first `groups` i32 hold the number of tiles each group evaluated.
 * nq >= 1, 1 <= F < 2^31.  No atomics, one launch, bit-identical run to run. */
int cnr_pm_index_params(int* tile_faces, int* group_queries);
int64_t cnr_pm_index_bytes(int64_t F);
int cnr_pm_index_keys(const float* verts, const int* faces, int64_t F, const float* bbox, int* keys_out, void* stream);
int cnr_pm_index_build(const float* verts, const int* faces, int64_t F, const int* keys, const int64_t* order, void* index_out,
                       void* stream);
int cnr_pm_query_keys(const float* q, int64_t nq, const float* bbox, int* keys_out, void* stream);
int64_t cnr_point_mesh_indexed_workspace_bytes(int64_t nq, int64_t F);
int cnr_point_mesh_dist_indexed(const float* q, int64_t nq, const int* qkeys, const int64_t* qorder, const void* index, int64_t F,
                                float* dist_out, int* face_out, float* closest_out, void* workspace, void* stream);
/* Generalized winding number (Jacobson et al. 2013), exact and brute force (tests/winding_cpu.py restates it).
 * q (nq,3) f32; the triangle forms of cnr_face_area_scan (faces == NULL: a soup).  w_out (nq,) f64 = (sum over all faces of t) /
 * 6.283185307179586, +1 inside a closed mesh whose right-hand normals point outward.  Per (query, face) pair, in fp64 of the
 * fp32 inputs without contraction, every operation one rounding, dot(u,v) = (u.x v.x + u.y v.y) + u.z v.z, difference first:
 * A = a - q, B = b - q, C = c - q; la = sqrt(dot(A,A)), lb, lc likewise; X = B x C, each component two products and one
 * subtraction; det = dot(A,X); den = ((la lb) lc + dot(A,B) lc) + (dot(B,C) la + dot(C,A) lb); t = atan2(det, den) (Van Oosterom
 * and Strackee: the signed solid angle is 2 t), and t = 0 when det == 0 exactly (the query in the face's plane, on the face or
 * not; an exactly degenerate face).  Sum order: within a face chunk the terms are added in face order onto a running fp64 sum
 * that starts at 0, the chunks' sums are added in chunk order.  Inputs must be finite.
 * nq >= 1, 1 <= F < 2^31; workspace >= cnr_winding_workspace_bytes(nq, F) = chunks * align256(8 nq), where chunks is the number
 * of face chunks of the grid (query blocks of 512, whole tiles of 256 faces per chunk, about 2048 workgroups): per chunk nq
 * partial sums (f64).  The chunk count depends on nq, so the result of one query may differ in the last bits between batch
 * sizes.  No atomics, no allocation, no host synchronisation; bit-identical run to run. */
int64_t cnr_winding_workspace_bytes(int64_t nq, int64_t F);
int cnr_winding_number(const float* q, int64_t nq, const float* verts, const int* faces, int64_t F, double* w_out,
                       void* workspace, void* stream);

/* ---- Category registration on point clouds: src/category_registration.py, src/utils.py:189-366.  DESIGN.md §3.9.  The
 * contracts of the metric kernels hold: caller-allocated outputs, workspace queries, no float atomics, fixed reduction
 * orders (bit-identical run to run).  Points and colours are (n,3) f32, C-contiguous.
 * Unprojection of one frame as sample_dict stores it: depth (W,H) f32, obj_mask (W,H) i32, image (W,H,3) u8.  A pixel is kept
 * when obj_mask == inst_id and 0 < depth <= 8.0; kept pixels are emitted in the arrays' memory order (i = u H + v: column by
 * column of the image).  point = T_WC (4,4 row-major f64, device) . ((u - cx) z / fx, (v - cy) z / fy, z, 1) in fp64, rounded
 * once; colour = u8 / 255.  cnr_unproject_count writes count_out (1,) i64 (device) and keeps per-workgroup offsets in
 * workspace (>= cnr_unproject_workspace_bytes(W, H)); cnr_unproject_emit, with the same inputs and workspace after it on the
 * same stream, writes count points and colours at the pointers given (the caller's cursor into a growing buffer). */
int64_t cnr_unproject_workspace_bytes(int W, int H);
int cnr_unproject_count(const float* depth, const int* obj_mask, int W, int H, int inst_id, void* workspace, int64_t* count_out,
                        void* stream);
int cnr_unproject_emit(const float* depth, const int* obj_mask, const uint8_t* image, int W, int H, int inst_id, double fx,
                       double fy, double cx, double cy, const double* T_WC, void* workspace, float* points, float* colors,
                       void* stream);
/* open3d's voxel_down_sample in four steps.  cnr_points_min: min_out (3,) f32 = the per-axis minimum.  cnr_voxel_keys:
 * keys[i] = (ix << 42) | (iy << 21) | iz with i* = floor((double(p) - (double(min) - voxel / 2)) / voxel), or -1 when an index
 * is outside [0, 2^21) or not a number.  The caller sorts the keys (stable) and passes the sorted keys and the permutation:
 * cnr_voxel_segments_count writes the number of distinct keys to count_out (1,) i64 (device); cnr_voxel_segments_emit writes
 * per distinct key, in ascending key order = ascending (ix, iy, iz), the fp64 mean of its points (and colours, unless colors
 * is NULL) summed in input order, the key and the number of points. */
int64_t cnr_points_min_workspace_bytes(int64_t n);
int cnr_points_min(const float* points, int64_t n, void* workspace, float* min_out, void* stream);
int cnr_voxel_keys(const float* points, int64_t n, const float* min_xyz, double voxel, int64_t* keys, void* stream);
int64_t cnr_voxel_segments_workspace_bytes(int64_t n);
int cnr_voxel_segments_count(const int64_t* sorted_keys, int64_t n, void* workspace, int64_t* count_out, void* stream);
int cnr_voxel_segments_emit(const int64_t* sorted_keys, const int64_t* perm, const float* points, const float* colors, int64_t n,
                            void* workspace, double* out_points, double* out_colors, int64_t* out_keys, int64_t* out_counts,
                            void* stream);
/* cnr_nn_dist with the index: dist_out[i] = min_j |q_i - p_j| in cnr_nn_dist's arithmetic, index_out[i] = the lowest j that
 * attains it.  nr < 2^31. */
int64_t cnr_nn_index_workspace_bytes(int64_t nq, int64_t nr);
int cnr_nn_index(const float* q, int64_t nq, const float* p, int64_t nr, float* dist_out, int* index_out, void* workspace,
                 void* stream);
/* One point-to-point ICP evaluation for B candidate transforms T (B,4,4 row-major f64, device) of one source cloud against one
 * target cloud.  Per candidate b: a_i = f32(T_b . src_i) (fp64 fused multiply-adds, rounded once), j = its exact nearest target
 * (ties: lowest index), d = their fp32 distance; over the pairs with d < max_corr, in a fixed order and in fp64, sums (B,17) =
 * [pairs, sum d^2, sum a (3), sum b (3), sum a b^T (9, row-major)].  dist_out / index_out (B, n_src), when not NULL, receive
 * d and j of every source point.  state (B,4) f64 or NULL: candidates whose state[b][2] != 0 are skipped: their sums and
 * their rows of dist_out / index_out are left as the caller's buffers held them.  workspace >= cnr_icp_workspace_bytes(n_src, n_tgt, B); B <= 65535.
 * cnr_icp_update, per running candidate: fitness = pairs / n_src and rmse = sqrt(sum d^2 / pairs) go to state[b][0..1]; when
 * both moved by less than 1e-6 since the last call (open3d's test) state[b][2] = 1; with fewer than 3 pairs state[b][2] = 2;
 * otherwise T_b <- dT . T_b for the rigid dT = (R, t) that minimises sum |R a + t - b|^2 (R = V diag(1,1,det(V U^T)) U^T of
 * sum (a - ca)(b - cb)^T = U S V^T, computed as Horn's quaternion), state[b][3] += 1, and state[b][2] = 3 once that reaches
 * max_iter.  A fresh state is all zeros. */
int64_t cnr_icp_workspace_bytes(int64_t n_src, int64_t n_tgt, int B);
int cnr_icp_step(const float* src, int64_t n_src, const float* tgt, int64_t n_tgt, const double* T, int B, float max_corr,
                 const double* state, void* workspace, double* sums, float* dist_out, int* index_out, void* stream);
int cnr_icp_update(const double* sums, int64_t n_src, int B, int max_iter, double* T, double* state, void* stream);

/* ---- TEASER-style global registration (category_registration.TeaserSolver): the two device stages.  The
 * contracts above hold: caller-allocated outputs, a workspace query, explicit stream, integer work only beyond the fp32 test
 * (no float atomics; results bit-identical run to run).
 * cnr_teaser_graph: the compatibility graph of N correspondences a_i -> b_i (A, B (N,3) f32): i ~ j (i != j) iff
 * fabsf(nb - na) <= threshold with na = sqrtf((dx dx + dy dy) + dz dz) of d = a_i - a_j and nb likewise of b_i - b_j, every
 * operation a single correctly rounded fp32 operation in this order (no fused multiply-add).  adj (N, ceil(N / 64)) u64: bit
 * (j & 63) of word j >> 6 of row i; bits at and beyond N are zero; deg (N,) i32 the row sums.  1 <= N <= CNR_TEASER_MAX_N. */
#define CNR_TEASER_MAX_N 16384
int cnr_teaser_graph(const float* A, const float* B, int N, float threshold, uint64_t* adj, int* deg, void* stream);
/* The maximum clique of a symmetric bitset graph in cnr_teaser_graph's layout.  order (N,) i32: a permutation of the vertices,
 * the fixed order of the search (the caller sorts by ascending degree, ties by index); max_degree >= the largest row sum.
 * Exact depth-first search, one wave per root vertex over its later neighbours in that order, pruned by the best size so far;
 * then the clique that is lexicographically smallest in positions of `order` among those of that size is rebuilt.  clique_out
 * (>= max_degree + 1) i32: its vertices (the caller's labels) in ascending position.  info_out (8) i64: [size, exact,
 * steps of the size pass, steps of the rebuilding pass, most steps of one root, roots that ran out of budget, the greedy
 * pass's size, flags (1: a row held more than max_degree neighbours, 2: the greedy clique was returned)].  A step is one AND
 * of the candidate set with an adjacency row; a root that has spent `budget` (>= 1) of them stops, and exact = 0 then: the
 * clique returned is still a clique, its size a lower bound.  With exact = 1 the result does not depend on timing.
 * workspace >= cnr_clique_workspace_bytes(N, max_degree). */
int64_t cnr_clique_workspace_bytes(int N, int max_degree);
int cnr_clique_search(const uint64_t* adj, const int* order, int N, int max_degree, int budget, void* workspace, int* clique_out,
                      int64_t* info_out, void* stream);

/* ---- TSDF fusion and radius outlier counts for ScanNet registration (src/utils.py:212-247).  DESIGN.md §3.10 has the whole
 * contract; every launch is deterministic and every fp64 product and sum is rounded on its own.
 * A volume is a list of units of 16^3 voxels of edge `voxel`; a unit's key is (ix + 2^20) << 42 | (iy + 2^20) << 21 | (iz + 2^20)
 * of its index floor(p / (16 voxel)); 0 < trunc <= 8 voxel (else CNR_E_SHAPE: a sample's
 * [p - trunc, p + trunc] then spans at most two units per axis).  Frames are in the loader's (W,H) layout: pixel
 * (x, y) at x H + y.
 * cnr_tsdf_touch: for the pixels with x % 4 == 0, y % 4 == 0 and depth > 0, in the order x major, the world point T_WC (4,4
 * row-major f64, device) . ((x - cx) d / fx, (y - cy) d / fy, d) and the keys of the units floor((p - trunc) / UL) ..
 * floor((p + trunc) / UL) per axis, 8 slots per sample (slot bits: x, y, z offset; -1 when unused), cnr_tsdf_touch_slots(W, H)
 * slots in all; frames[slot] = frame.  A unit index outside [-2^20, 2^20) or not a number (or, by rounding at trunc = 8 voxel, a third unit on an axis): bit 0 of *err (device int, the
 * caller zeroes it) is set and the sample emits nothing.
 * cnr_tsdf_integrate: units (U,) ascending keys; unit u is updated by frames frame_idx[frame_ofs[u] .. frame_ofs[u + 1]) in that
 * order (indices into depth (F,W,H) f32, color (F,W,H,3) u8, T_CW (F,4,4) f64: world -> camera).  Writes tsdf (U,4096), weight
 * (U,4096), colors (U,4096,3) f32, voxel (i, j, k) of a unit at (i 16 + j) 16 + k.
 * cnr_tsdf_extract_count / _emit: neighbours (U,3) i32 = each unit's +x, +y, +z unit or -1.  count writes count_out (1,) i64
 * (device) and keeps per-unit offsets in workspace (>= cnr_tsdf_extract_workspace_bytes(U)); emit, with the same inputs and
 * workspace after it on the same stream, writes count points and colours (f64) in the order unit, voxel, axis. */
/* cnr_tsdf_depth_image: out[i] = the depth the volume sees, from n pixels of metric f32 depth: 0 unless obj_mask[i] == inst_id,
 * u16 = uint16(trunc(double(depth) / depth_scale)) (wrapping; 0 when negative or not a number), float(u16) / 1000.0f, 0 when
 * that exceeds max_depth (compared in fp64). */
int cnr_tsdf_depth_image(const float* depth, const int* obj_mask, int64_t n, int inst_id, double depth_scale, double max_depth,
                         float* out, void* stream);
int64_t cnr_tsdf_touch_slots(int W, int H);
int cnr_tsdf_touch(const float* depth, int W, int H, double fx, double fy, double cx, double cy, const double* T_WC, double voxel,
                   double trunc, int frame, int64_t* keys, int* frames, int* err, void* stream);
int cnr_tsdf_integrate(const int64_t* units, int64_t U, const int64_t* frame_ofs, const int* frame_idx, const float* depth,
                       const uint8_t* color, const double* T_CW, int F, int W, int H, double fx, double fy, double cx, double cy,
                       double voxel, double trunc, float* tsdf, float* weight, float* colors, void* stream);
int64_t cnr_tsdf_extract_workspace_bytes(int64_t U);
int cnr_tsdf_extract_count(const float* tsdf, const float* weight, const int* neighbours, int64_t U, void* workspace,
                           int64_t* count_out, void* stream);
int cnr_tsdf_extract_emit(const int64_t* units, const float* tsdf, const float* weight, const float* colors, const int* neighbours,
                          int64_t U, double voxel, void* workspace, double* points, double* colors_out, void* stream);
/* The triangle mesh of an integrated volume (csrc/tsdf_mesh.hip): marching cubes across units.
 * Inputs: units (U,) ascending keys, tsdf (U,4096), weight (U,4096), colors (U,4096,3) f32 as cnr_tsdf_integrate writes them, and
 * hood (U,27) i32: for the offset (dx, dy, dz) in {-1,0,1}^3 at column (dx + 1) 9 + (dy + 1) 3 + (dz + 1) the index of that unit
 * or -1 (column 13: the unit itself; an index outside [0, U) counts as -1).
 * A voxel is observed when its unit exists and weight != 0 (no +-0.98 band).  A cell is named by its min-corner voxel; corner c
 * is the voxel at +((c >> 2) & 1, (c >> 1) & 1, c & 1) (mc_table.h's numbering); the cell is valid when all 8 corners are
 * observed; bit c of its case is set when tsdf[c] < 0 (+0, -0 and NaN: not set); its triangles are MC_NTRI / MC_TRI's, each
 * edge named by MC_EDGE_LO's owning voxel and axis.
 * Vertices: one per (owner voxel, axis) that a valid cell uses, none else.  fp64, every product and sum rounded on its own:
 * the owner's centre unit 16 voxel + (ijk + 0.5) voxel with coordinate `axis` replaced by (p0 r1 + p1 r0) / (r0 + r1),
 * p1 = p0 + voxel, r = |tsdf| of the two ends (cnr_tsdf_extract_emit's formulas); colours (c0 r1 + c1 r0) / (r0 + r1) / 255.
 * Normals: per end and axis (f+ - f-) 0.5 where both axis neighbours are observed, the one-sided difference where one is, else
 * 0; the two ends blended (g0 r1 + g1 r0) / (r0 + r1); divided by sqrt((nx nx + ny ny) + nz nz) where that is > 0, else 0.
 * They point to increasing tsdf, and so does every face's right-hand normal (cnr_mc's faces on -tsdf, level 0, ascent 0).
 * Order: vertices by (unit, voxel, axis), faces by (unit, cell's voxel, table order); bit-identical from run to run.
 * cnr_tsdf_mesh_count writes counts_out (2,) i64 = {V, F} (device) and keeps per-voxel and per-unit tables in workspace
 * (>= cnr_tsdf_mesh_workspace_bytes(U)); cnr_tsdf_mesh_emit, with the same inputs and workspace after it on the same stream,
 * writes verts, colors_out, normals (V,3) f64 and faces (F,3) i32.  V >= 2^31: CNR_E_SHAPE (emit reads the count back, and
 * waits for the stream, only for U >= 174763, below which no volume holds that many). */
int64_t cnr_tsdf_mesh_workspace_bytes(int64_t U);
int cnr_tsdf_mesh_count(const float* tsdf, const float* weight, const int* hood, int64_t U, void* workspace, int64_t* counts_out,
                        void* stream);
int cnr_tsdf_mesh_emit(const int64_t* units, const float* tsdf, const float* weight, const float* colors, const int* hood, int64_t U,
                       double voxel, void* workspace, double* verts, double* colors_out, double* normals, int* faces, void* stream);
/* open3d's remove_radius_outlier counts.  cnr_radius_cell_keys: keys[i] = the packed cell floor(double(p) / radius) per axis
 * (biased like a unit key), or -1 and bit 0 of *err for an index outside [-2^20, 2^20) or not a number.  The caller sorts the
 * keys (stable) and passes the permutation, the sorted keys, the C distinct keys ascending and starts (C + 1,) i64 (cell c holds
 * sorted positions starts[c] .. starts[c + 1]).  cnr_radius_count: counts[i] (i32) = the number of points j, i included, with
 * (dx dx + dy dy) + dz dz < radius radius in fp64 from the f32 coordinates. */
int cnr_radius_cell_keys(const float* points, int64_t n, double radius, int64_t* keys, int* err, void* stream);
int cnr_radius_count(const float* points, int64_t n, const int64_t* perm, const int64_t* sorted_keys, const int64_t* cells,
                     const int64_t* starts, int64_t C, double radius, int* counts, void* stream);

/* ---- TEASER's FPFH mode (src/teaser_utils/helpers.py: extract_fpfh, find_correspondences).  The contracts
 * above hold: caller-allocated outputs, an explicit stream, argument errors as return codes before the device is touched, no
 * float atomics, every loop bounded, results bit-identical run to run.  Every fp64 product, sum and quotient is rounded on its
 * own (no fused multiply-add), so a numpy restatement repeats it.  Equality with open3d is unverified.
 * cnr_hybrid_search: open3d's KDTreeSearchParamHybrid(radius, max_nn) for every point of the cloud against the cloud itself.
 * points (n,3) f32; perm, sorted_keys, cells, starts, C: the cell tables of cnr_radius_cell_keys at edge `radius`, built by the
 * caller as for cnr_radius_count.  The candidates of point i are the points j of the 27 cells around it, i included, with d2 =
 * (dx dx + dy dy) + dz dz < radius radius in fp64 from the f32 coordinates; ordered by (d2, j) ascending, the first max_nn are
 * kept: idx (n, max_nn) i32 padded with -1, d2 (n, max_nn) f64 padded with 0, count (n,) i32.  1 <= max_nn <= 128, n < 2^31
 * (else CNR_E_SHAPE).  A point whose key is -1 (not a number, or outside the cell range) gets count 0 and is nobody's
 * neighbour.  One wave per point; the candidates pass through a buffer of cnr_hybrid_search_capacity() entries per wave that is
 * cut back to the best max_nn whenever it fills: a neighbourhood with more candidates than that is still exact. */
int cnr_hybrid_search_capacity(void);
int cnr_hybrid_search(const float* points, int64_t n, const int64_t* perm, const int64_t* sorted_keys, const int64_t* cells,
                      const int64_t* starts, int64_t C, double radius, int max_nn, int* idx, double* d2, int* count,
                      void* stream);
/* normals (n,3) f64 from the lists idx (n, max_nn), count (n,) of a hybrid search.  Fewer than 3 neighbours (or an entry
 * outside [0, n)): (0, 0, 1).  Otherwise, with k = count[i] and the listed points in list order: mean = (sequential sum) / k;
 * covariance entries = (sequential sum of (p - mean)_a (p - mean)_b) / k; cyclic Jacobi on the pairs (0,1), (0,2), (1,2), 8
 * sweeps, per pair with a_pq != 0: theta = (a_qq - a_pp) / (2 a_pq), t = sign(theta) / (|theta| + sqrt(theta theta + 1))
 * (sign(0) = 1), c = 1 / sqrt(t t + 1), s = t c; a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0, (a_rp, a_rq) <- (c a_rp - s a_rq,
 * s a_rp + c a_rq), the same for every row of V.  The normal is the column of V of the smallest diagonal entry (the first of
 * equals), divided by its length sqrt((x x + y y) + z z), negated when d = (n_x (p_x - c_x) + n_y (p_y - c_y)) + n_z (p_z -
 * c_z) < 0 with p = point i and c = (cx, cy, cz), the centroid of the whole cloud, which the caller computes once; when d == 0,
 * negated when its component of largest magnitude (the first of equals) is negative.  open3d keeps the eigen-solver's sign:
 * this orientation is a deliberate difference (it moves with the cloud under a rigid motion; the descriptors need that). */
int cnr_estimate_normals(const float* points, int64_t n, const int* idx, const int* count, int max_nn, double cx, double cy,
                         double cz, double* normals, void* stream);
/* spfh (n,33) f64 from points, normals (n,3) f64 and the lists of one hybrid search.  Row i with k = count[i] <= 1 is zero.
 * Otherwise every listed neighbour after the first (the first is i itself) adds 1 to three integer histograms of 11 bins at
 * offsets 0, 11, 22: the bins min(max(floor(x), 0), 10) of x = (11 (f0 + pi)) / (2 pi), (11 (f1 + 1)) 0.5, (11 (f2 + 1)) 0.5
 * of the pair feature of (p1, n1) = point i and (p2, n2) = the neighbour: dp = p2 - p1, d = sqrt((dp_x dp_x + dp_y dp_y) +
 * dp_z dp_z); d == 0: f = 0.  a1 = n1.dp / d, a2 = n2.dp / d (dots as (x x + y y) + z z); if fabs(a1) < fabs(a2) the normals
 * swap, dp = -dp and f2 = -a2, else f2 = a1.  v = dp x n1, |v| == 0: f = 0 (f2 too); v = v / |v| per component, w = n1 x v,
 * f1 = v.n2, f0 = atan2(w.n2, n1.n2).  The row is (double)count (100.0 / (k - 1)).
 * cnr_fpfh: fpfh (n,33) f64 from spfh and the lists with their d2.  Row i with k <= 1 is zero.  Otherwise over the listed
 * neighbours after the first with d2 != 0, in list order, and j = 0..32 in order: val = spfh[nbr][j] / d2, out[j] += val,
 * sum[j / 11] += val; then out[j] = out[j] (100.0 / sum[j / 11]) where that sum is not 0; then out[j] += spfh[i][j]. */
int cnr_spfh(const float* points, const double* normals, int64_t n, const int* idx, const int* count, int max_nn, double* spfh,
             void* stream);
int cnr_fpfh(const double* spfh, int64_t n, const int* idx, const double* d2, const int* count, int max_nn, double* fpfh,
             void* stream);
/* The exact nearest neighbour in descriptor space: q (nq,D), p (nr,D) f32, 1 <= D <= 64, nr < 2^31 (else CNR_E_SHAPE).
 * dist2(i, r) = the sequential fp32 sum over j = 0..D-1 of (q_ij - p_rj)^2 from 0, one rounded subtraction, one rounded product
 * and one rounded sum each (no expanded square, no matrix instruction); index_out[i] (i32) = the lowest r that attains the
 * minimum (row 0 when nothing compares below it), dist_out[i] (f32) = that minimum.  p is tiled through LDS, in chunks of rows
 * spread over the grid so that few queries still fill the device; the chunks' minima pass through workspace (>=
 * cnr_feature_nn_workspace_bytes(nq, nr); nq < 2^31) and are merged in chunk order, so the result is the same for any split. */
int64_t cnr_feature_nn_workspace_bytes(int64_t nq, int64_t nr);
int cnr_feature_nn(const float* q, int64_t nq, const float* p, int64_t nr, int D, int* index_out, float* dist_out, void* workspace,
                   void* stream);

/* ---- Scene view rendering: a camera pose in, an image of the composed scene out.  DESIGN.md section 3.11.
 * An entity is a field with a box: to_box (E,3,4) maps a world point into [-1,1]^3 of the volume that is meshed for it,
 * to_field (E,3,4) into the frame its field takes.  T_wc (4,4) row-major camera-to-world, dirs (P,3) the camera-frame pixel
 * directions (x, y, 1) of cnr_camera_rays: the ray parameter z is the camera depth in every frame, since every transform is a
 * similarity.  No atomics anywhere: every output is the same bit for bit from run to run.
 *
 * Segments.  Per (pixel, entity) a slab test of T_wc (z d, 1) in box coordinates: an axis whose direction component is exactly
 * zero passes iff |origin| <= 1 there and bounds nothing; otherwise [z_near, z_far] is the intersection of the three slabs
 * with [zmin, zmax], and a segment exists iff z_far > z_near.  cnr_view_segments_count writes count_out (1,) i64 = N,
 * entity_offset (E+1,) i64 and overflow (1,) i64 = the number of pixels met by more than CNR_VIEW_KMAX boxes (all on the
 * device) and keeps per-wave offsets in workspace (>= cnr_view_segments_workspace_bytes(P, E)); cnr_view_segments_emit, with
 * the same inputs and workspace after it on the same stream, writes the segments in (entity, pixel) order -- seg_pixel (N,)
 * i32, seg_entity (N,) i32, seg_z (N,2) f32 = z_near, z_far; entity e owns [entity_offset[e], entity_offset[e+1]) -- and
 * pix_segs (P, CNR_VIEW_KMAX) i32: the segment indices of every pixel in entity order, -1-padded.  A pixel met by more boxes
 * keeps the CNR_VIEW_KMAX nearest by z_near (ties: the earlier entity) in pix_segs; all of its segments are still emitted.
 * P < 2^31, E <= 32767 (else CNR_E_SHAPE).  With N = 0 the three seg_* pointers may be NULL. */
#define CNR_VIEW_KMAX 8
#define CNR_VIEW_SMAX 128
int64_t cnr_view_segments_workspace_bytes(int64_t P, int E);
int cnr_view_segments_count(const float* T_wc, const float* dirs, const float* to_box, int64_t P, int E, float zmin,
                            float zmax, void* workspace, int64_t* entity_offset, int64_t* count_out, int64_t* overflow,
                            void* stream);
int cnr_view_segments_emit(const float* T_wc, const float* dirs, const float* to_box, int64_t P, int E, float zmin,
                           float zmax, const void* workspace, int* seg_pixel, int* seg_entity, float* seg_z, int* pix_segs,
                           void* stream);
/* S uniform midpoints per segment: z (N,S), z_i = z_near + (i + 0.5) (z_far - z_near) / S, and pts (N,S,3) =
 * to_field[seg_entity] . (T_wc . (z_i d, 1)).  1 <= S <= CNR_VIEW_SMAX (else CNR_E_SHAPE). */
int cnr_view_points(const float* T_wc, const float* dirs, const float* to_field, const int* seg_pixel, const int* seg_entity,
                    const float* seg_z, int64_t N, int S, float* z, float* pts, void* stream);
/* The merged composite.  sigma (N,S) the field kernels' x10 logit, color (N,S,3), z (N,S) ascending within a segment.  The
 * samples of a pixel's segments (pix_segs row, at most CNR_VIEW_KMAX S of them) are ordered by (z, position in the row, sample
 * index); occ_i = sigmoid(sigma_i), term_i = occ_i prod_{j<i} (1 - occ_j + 1e-10) as in cnr_composite_fwd, and
 *   rgb (P,3) = sum term c | depth (P,) = sum term z | opacity (P,) = sum term | var (P,) = sum term (z - depth)^2
 *   mass (P, CNR_VIEW_KMAX) = sum term per segment of the row (0 where the row is padded)
 *   instance (P,) i32 = entity_inst[seg_entity[.]] of the segment with the largest mass (ties: the earlier one) when
 *   opacity >= opacity_threshold, else -1.
 * A pixel without a segment gives zeros and -1.  1 <= S <= CNR_VIEW_SMAX (else CNR_E_SHAPE), P < 2^31. */
int cnr_view_composite(const float* sigma, const float* color, const float* z, const int* pix_segs, const int* seg_entity,
                       const int* entity_inst, int64_t P, int S, float opacity_threshold, float* rgb, float* depth,
                       float* opacity, float* var, float* mass, int* instance, void* stream);
/* Empty-space skipping.  An occupancy grid is one bit per cell of a G^3 grid over an entity's box [-1,1]^3, G a multiple of 4
 * in 4 .. 128: cell (ix, iy, iz) has the linear index l = (ix G + iy) G + iz and is bit l & 31 of word l >> 5 of the grid's
 * G^3 / 32 i32 words.
 *
 * cnr_view_grid_cells: occ (D,D,D) f32, D = G sub + 1, 1 <= sub <= 4, a lattice of occupancies over the box, first axis x
 * -> words.  A cell owns the lattice indices [i sub, (i + 1) sub] of every axis, both faces included, and is set iff some
 * owned value v satisfies !(v < tau): a value equal to tau sets it, and so does a NaN.
 * cnr_view_grid_dilate: words_out = every cell within Chebyshev distance radius (0 .. 2) of a set cell of words_in, the
 * neighbourhood clamped at the faces of the grid; out of place (words_in == words_out is CNR_E_ARG).
 *
 * Active samples: the count / emit pair that stands in for cnr_view_points.  Sample n S + i of the (N,S) samples of the
 * segments (z_i and the world point as in cnr_view_points) is active iff entity_grid[seg_entity[n]] < 0 (no grid: all set) or
 * the cell c of grid entity_grid[.] of grid_words (grids, G^3 / 32) is set, b = to_box[seg_entity[n]] . world point,
 * c_k = min(G - 1, max(0, (int)floorf((b_k + 1) 0.5 G))).  cnr_view_active_count, with entity_offset as
 * cnr_view_segments_count left it, writes active_offset (E+1,) i64 and count_out (1,) i64 = the number of active samples, and
 * keeps its masks and ranks in workspace (>= cnr_view_active_workspace_bytes(N, S, E)).  The compact list holds the active
 * samples in (entity, segment, sample) order, every entity's run padded to a multiple of 64 entries: entity e owns
 * [active_offset[e], active_offset[e+1]), M = active_offset[E].  cnr_view_active_emit, after it on the same stream with the same
 * workspace, writes z (N,S) of every sample, active_idx (M,) i64 = n S + i, or -1 at a padding entry, pts_c (M,3) =
 * to_field . world point, bit for bit what cnr_view_points writes for that sample, the origin at a padding entry, and
 * block_row (M/64,) i32 = entity_row[e] of the entity e whose run holds the block.  With M = 0 those three may be NULL. */
int cnr_view_grid_cells(const float* occ, int G, int sub, float tau, int* words, void* stream);
int cnr_view_grid_dilate(const int* words_in, int G, int radius, int* words_out, void* stream);
int64_t cnr_view_active_workspace_bytes(int64_t N, int S, int E);
int cnr_view_active_count(const float* T_wc, const float* dirs, const float* to_box, const int* seg_pixel,
                          const int* seg_entity, const float* seg_z, const int64_t* entity_offset, int64_t N, int S, int E,
                          const int* grid_words, const int* entity_grid, int G, void* workspace, int64_t* active_offset,
                          int64_t* count_out, void* stream);
int cnr_view_active_emit(const float* T_wc, const float* dirs, const float* to_field, const int* seg_pixel,
                         const int* seg_entity, const float* seg_z, int64_t N, int S, int E, const int* entity_row,
                         const void* workspace, const int64_t* active_offset, int64_t M, float* z, int64_t* active_idx,
                         float* pts_c, int* block_row, void* stream);
/* sigma (NS,) = -inf and color (NS,3) = 0 everywhere, then sigma[active_idx[j]] = sigma_c[j], color[active_idx[j]] = color_c[j]
 * for the M entries of the compact list; an entry with active_idx < 0 (padding) writes nothing.  cnr_view_composite gives a
 * sample of sigma -inf the occupancy 0 exactly, so it multiplies the transmittance by exactly 1. */
int cnr_view_scatter_active(const float* sigma_c, const float* color_c, const int64_t* active_idx, int64_t M, int64_t NS,
                            float* sigma, float* color, void* stream);

/* ---- ScanNet mask refinement (src/utils.py: geometry_segmentation, refine_inst_data).  The contracts
 * above hold: caller-allocated outputs, an explicit stream, argument errors as return codes before the device is touched, no
 * host sync, no float atomics, every loop bounded, results identical run to run.  Every fp32 product, sum, quotient and square
 * root is rounded on its own.  Images are (H,W) row-major, pixel (v,u) at v W + u; H W < 2^31 - 1 (else CNR_E_SHAPE).
 * Equality with cv2 is unverified (DESIGN.md says which stages are pinned to what).
 *
 * cnr_geoseg_maps: P (H,W,3) f32 the camera-frame point map (zero at invalid pixels), N (H,W,3) f32 the normals, depth (H,W) f32
 * with 0 = invalid -> disc, conv (H,W) u8.  ero / dil = min / max of depth over the 3x3 window, pixels outside the image
 * ignored, zeros taking part as zeros; ratio = max(depth - ero, dil - depth) / depth where depth > 0, else 0; disc = ratio >
 * 0.01f.  conv: over the 24 offsets of the 5x5 window without its centre, neighbour indices reflected without repeating the
 * edge (-1 -> 1, H -> H - 2): d = P[n] - P[c], dot = ((d_x (-N_x) + d_y (-N_y)) + d_z (-N_z)) with N at the centre, proj =
 * ((N_x N'_x + N_y N'_y) + N_z N'_z) with N' at the neighbour, term = 1 if dot > -0.0005f else proj; conv = (min of the terms
 * and 10) > 0.9f.  H, W >= 3 (else CNR_E_SHAPE). */
int cnr_geoseg_maps(const float* P, const float* N, const float* depth, int H, int W, uint8_t* disc, uint8_t* conv, void* stream);
/* edge (H,W) u8 = open3(conv) & ~close3(disc) & (depth > 0): open3 = dilate(erode(.)), close3 = erode(dilate(.)), 3x3, pixels
 * outside the image ignored in each pass.  1 marks a region pixel (the reference's edge_map_uint8). */
int cnr_geoseg_edge_map(const uint8_t* disc, const uint8_t* conv, const float* depth, int H, int W, uint8_t* edge, void* stream);
/* Connected components of F stacked masks (F,H,W) u8 (non-zero = set), connectivity 4 or 8 (else CNR_E_SHAPE), 1 <= F <= 65535:
 * labels (F,H,W) i32 = the smallest raster index v W + u, within its frame, among the pixels of the pixel's component; -1 where
 * the mask is 0.  Tile-local labelling in LDS, unions across the tile borders, then flattening, all on the device; the result is
 * defined by the mask alone.  Every union/find loop is bounded by H W steps; one that runs out sets err (1,) i32, which the
 * caller zeroes beforehand and reads when it next synchronises (it never happens on a valid label array).
 * cnr_label_counts: counts (F,H,W) i32, counts[f][l] = the pixels of frame f with label l (labels outside [0, H W) are skipped). */
int cnr_ccl(const uint8_t* mask, int F, int H, int W, int connectivity, int* labels, int* err, void* stream);
int cnr_label_counts(const int* labels, int F, int H, int W, int* counts, void* stream);
/* The 9x9 label growth.  labels (H,W) i32 of cnr_ccl on edge; with counts (H,W) i32 (may be NULL) a label with counts[label] <
 * min_area counts as -1.  labels_out = that label where edge != 0.  An edge pixel (edge == 0 and depth > 0) walks the offsets i
 * = -4..4 in x (outer loop) and j = -4..4 in y (inner loop) without (0,0); a neighbour qualifies when it lies inside the image,
 * has edge != 0 and a label >= 0; its distance is sqrtf((dx dx + dy dy) + dz dz) of the two rows of P; the pixel takes the label
 * of the neighbour with the smallest distance < 0.05f, the first in loop order among equals, else -1.  depth == 0: -1. */
int cnr_geoseg_grow(const float* P, const float* depth, const uint8_t* edge, const int* labels, const int* counts, int min_area,
                    int H, int W, int* labels_out, void* stream);
/* scipy's binary_fill_holes (default structure) of K masks: filled (K,H,W) u8 = the mask plus every pixel outside it whose
 * 4-connected component of the complement does not touch the image border.  The masks are either labels (H,W) i32 == seg_ids[k]
 * (seg_ids (K,) i32; masks NULL) or masks (K,H,W) u8 (labels and seg_ids NULL): exactly one of the two, else CNR_E_ARG.
 * 0 <= K <= 65535 (else CNR_E_SHAPE; K = 0 does nothing); workspace >= cnr_fill_holes_workspace_bytes(K, H, W); err as for
 * cnr_ccl. */
int64_t cnr_fill_holes_workspace_bytes(int K, int H, int W);
int cnr_fill_holes(const int* labels, const int* seg_ids, const uint8_t* masks, int K, int H, int W, void* workspace,
                   uint8_t* filled, int* err, void* stream);
/* The overlap vote.  inst (H,W) i32 the raw instance map, obj_ids (O,) i32 ascending and distinct, 0 <= O <= 2048 (else
 * CNR_E_SHAPE).  cnr_refine_vote: counts (K, O + 1) i32, [k][o] = |filled_k & inst == obj_ids[o]|, [k][O] = |filled_k|.
 * cnr_refine_apply: chosen (K,) i32 = the first o that attains the largest fp64 quotient counts[k][o] / counts[k][O] when that
 * quotient is > threshold, else -1 (also for an empty mask); refined (H,W) i32 = obj_ids[chosen[k]] of the last k whose filled
 * mask holds the pixel and that has chosen, else 0. */
int cnr_refine_vote(const uint8_t* filled, const int* inst, const int* obj_ids, int K, int O, int H, int W, int* counts,
                    void* stream);
int cnr_refine_apply(const uint8_t* filled, const int* counts, const int* obj_ids, int K, int O, int H, int W, double threshold,
                     int* chosen, int* refined, void* stream);

/* ---- registration's per-object fields: ONE launch = one train step of every object (csrc/obj_fused.hip) -------------------------
 * N independent OccupancyMap(87, 42, hidden 32) + UniDirsEmbed models (src/model.py:86-155), each trained on its own ray pool by the
 * reference's background step (train.py:113-121,172-184 with one class): R rays x S = n1 + n2 <= 64 samples, world-frame rays,
 * depth-guided sampling, composite, the three loss terms (color_scaling, opacity_scaling), backward, AdamW.  One workgroup per
 * object; exact fp32 arithmetic; no float atomics and no cross-workgroup reduction: two runs give the same bits, and an object's
 * result does not depend on what else is in the launch.
 *   theta, exp_avg, exp_avg_sq (N, P) f32, P = cnr_obj_param_count() = 11 363: per object
 *     in_layer.0 W (32,87) b | mid1.0.0 W (32,32) b | cat_layer.0 W (32,119) b | mid2.0.0 W (32,32) b | out_alpha W (1,32) b |
 *     color_linear.0 W (32,74) b | out_color W (3,32) b | B_layer.weight (21,3)        (the modules' registration order).
 *   pools: the objects' rows concatenated -- rgbs (rows,4) u8 [r,g,b,state], depth (rows,), dirs_c (rows,3), T (rows,4,4) = T_wc --
 *     object o owns rows [pool_off[o], pool_off[o+1]) (pool_off: N + 1 i64 on the device); min_pool_rows: the shortest segment,
 *     which the host checks against R (an object whose segment is shorter all the same is skipped with flag 16).
 *   d_state (N,4) i64 = {cursor, rng step, optimiser step, epoch} per object.  Row r of the step is
 *     bijection(seed, id, epoch)(cursor + r) of the object's segment -- cnr_epoch_perm's keyed permutation evaluated in the kernel,
 *     id = obj_ids[o] (device, N entries) or o when NULL; the Philox draws are keyed by (seed, id, rng step).  After the step
 *     cursor += R, and cursor >= rows_o - R starts the object's next epoch (cursor 0, epoch + 1: src/scene_cateogries.py:439-449).
 *   rows (N,R) i32 (segment-relative), u (N,R,S), g (N,R,n2): all three or none -- the step's rows and draws given (parity tests);
 *     a row outside the segment is read as row 0 and sets flag 32.
 *   max_bound and the mask counts of reduce_batch_loss are taken over the object's R rows; a zero count zeroes that term and its
 *     gradient for that object only (render_rays.py:67-72) and sets flag 2 / 4 / 8 (depth / colour / opacity); flag 1: a term
 *     above 100 000.  losses (3,N), flags (N).
 *   Outputs skipped when NULL: grad (N,P) the step's gradient, sigma (N,R,S), rgb (N,R,S,3), z (N,R,S), rows_out (N,R) i32
 *     (segment-relative).  workspace: cnr_obj_workspace_bytes(N, R, S) bytes, 16-byte aligned.
 * CNR_E_ARG: a required pointer NULL, N <= 0, R <= 0, S > 64, min_pool_rows < R, a partial parity set, a short workspace. */
int cnr_obj_param_count(void);
int64_t cnr_obj_workspace_bytes(int N, int R, int S);
int cnr_obj_train(const uint8_t* rgbs, const float* depth, const float* dirs_c, const float* T, const int64_t* pool_off,
                  int64_t min_pool_rows, const int* obj_ids, int N, int R, int n1, int n2, float eps, float stop_eps,
                  float min_bound, float scale, uint64_t seed, const int* rows, const float* u, const float* g,
                  int64_t* d_state, float* theta, float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2,
                  float adam_eps, float weight_decay, float color_scaling, float opacity_scaling, float* losses,
                  int32_t* flags, float* grad, float* sigma, float* rgb, float* z, int* rows_out, void* workspace,
                  int64_t workspace_bytes, void* stream);

/* ---- fitting codes to a frozen category: ONE launch = one optimisation step of every candidate (csrc/code_fit.hip) --------------
 * A candidate is one (instance, starting code) pair: a shape code and a texture code of a frozen CodeNeRF category, fitted to the
 * instance's own ray pool by the reference's object step with a one-object class and the network held fixed (train.py:123-167,
 * src/model.py:56-84, src/loss.py:5-74): rows, origin_dirs_O / origin_dirs_W, depth-guided sampling, UniDirsEmbed, CodeNeRF
 * forward, composite, the three masked L1 terms, backward to the four latent outputs and through the latent layers to the two
 * codes, the code-norm regulariser, AdamW on the codes.  One workgroup per candidate; exact fp32 arithmetic; no float atomics and
 * no cross-workgroup reduction: two runs give the same bits, and a candidate's result does not depend on what else is in the launch.
 *   theta: n_nets rows of class_stride floats, the frozen networks; inside a row the trunk (CNR_TRUNK_PARAMS floats, the blob
 *     order above) at off_trunk, the latent matrices (4,32,L) at off_latW, their biases (4,32) at off_latb, B (21,3) at off_B --
 *     fused.ParamLayout's row, so a live FusedCategoryTrainer buffer or a packed snapshot can both be passed.  Never written.
 *   pools: P segments concatenated as for cnr_obj_train (rgbs, depth, dirs_c, T, pool_off (P + 1), min_pool_rows); pool_ids (P)
 *     i32 or NULL (the segment index); pool_world_frame (P) i32: 0 = the T rows are T_CO (origin_dirs_O inverts them), else T_WC.
 *   cand_net, cand_pool (K) i32: the network and the pool of every candidate.  Several candidates may share a pool: rows and
 *     draws are keyed by (seed, pool id, epoch or rng step), not by the candidate, so candidates of one pool with equal state see
 *     the same rays and draws and differ only in their codes.  An index out of range sets flag 64 and the candidate is skipped:
 *     nothing of it is read and its five loss values are zero.
 *   codes, exp_avg, exp_avg_sq (K,2,L) f32: shape code, then texture code.  d_state (K,4) i64 = {cursor, rng step, optimiser step,
 *     epoch} with cnr_obj_train's rule.  update = 0: evaluation only -- losses, flags and the optional outputs are written; codes,
 *     moments and state are untouched.
 *   rows (K,R) i32 (segment-relative), u (K,R,S), g (K,R,n2): all three or none, as cnr_obj_train.
 *   The regulariser adds reg_scaling * c / ||c|| to each code's gradient when reg_scaling > 0 (zero at ||c|| = 0, as torch's norm).
 *   losses (5,K) = depth, colour, opacity, ||shape code||, ||texture code||; flags (K): cnr_obj_train's bits (1 a term above
 *     100 000; 2 / 4 / 8 a zero depth / colour / opacity count, which zeroes that term and its gradient for that candidate only;
 *     16 a pool shorter than R, skipped; 32 a given row out of range) and 64.  Outputs skipped when NULL: grad (K,2,L), sigma
 *     (K,R,S), rgb (K,R,S,3), z (K,R,S), rows_out (K,R) i32.  workspace: cnr_code_fit_workspace_bytes(K, R, S), 16-byte aligned.
 * CNR_E_ARG: a required pointer NULL, K <= 0, R <= 0, n_nets <= 0, P <= 0, S > 64, min_pool_rows < R, a partial parity set, a
 * short workspace, a trunk / latent W / latent b / B block that would end past class_stride.  CNR_E_SHAPE: a code length L other than a divisor or a multiple of 256 (the latent kernels' rule). */
int64_t cnr_code_fit_workspace_bytes(int K, int R, int S);
int cnr_code_fit(const float* theta, int64_t class_stride, int64_t off_trunk, int64_t off_latW, int64_t off_latb, int64_t off_B,
                 int n_nets, int L, const uint8_t* rgbs, const float* depth, const float* dirs_c, const float* T,
                 const int64_t* pool_off, int64_t min_pool_rows, const int* pool_ids, const int* pool_world_frame, int P,
                 const int* cand_net, const int* cand_pool, int K, int R, int n1, int n2, float eps, float stop_eps,
                 float min_bound, float scale, uint64_t seed, const int* rows, const float* u, const float* g, int64_t* d_state,
                 float* codes, float* exp_avg, float* exp_avg_sq, int update, float lr, float beta1, float beta2, float adam_eps,
                 float weight_decay, float color_scaling, float opacity_scaling, float reg_scaling, float* losses, int32_t* flags,
                 float* grad, float* sigma, float* rgb, float* z, int* rows_out, void* workspace, int64_t workspace_bytes,
                 void* stream);

/* ---- field gradients: the x10 occupancy logit sigma and its spatial derivative d sigma / d x (csrc/field_grad.hip; DESIGN.md
 * section 3.15).  Forward mode: the value and its three tangents pass through every layer together, T' = mask . (W T), so sigma
 * comes out on the way and nothing is stashed.  Exact fp32 on the vector unit: fp32 products and sums, accurate sinf / cosf (the
 * arguments reach 8 pi |x / scale|), ReLU'(0) = 0.  No atomics, and a point's arithmetic does not depend on N, on its place in
 * the array or on its neighbours: outputs are bit-identical run to run and for any split of the points into calls.  Any N >= 1;
 * N = 0 returns CNR_OK and launches nothing; pointers of N = 0 are not looked at.  sigma (N,) may be NULL; grad (N,3).
 *
 * cnr_field_grad: one CodeNeRF category, geometry branch only (src/model.py:56-75: encoding_xyz, shape_layer_1, cat_layer,
 * shape_layer_2, encoding_shape, sigma) on e[:87] of the embedding, whose Jacobian is I / scale stacked on
 * pi 2^k cos(pi 2^k B_j . x / scale) B_j / scale, k = 0..3.  pts (N,3) in the field frame, B (21,3), trunk (CNR_TRUNK_PARAMS) the
 * fp32 blob (only its first 9 857 floats are read), biasrows (rows,4,32) as cnr_latent_fwd / ops.bias_rows produce them (slots 0..2
 * are read), row (N,) i32 = every point's row of biasrows, which may change from point to point (NULL: row 0); rows are not
 * range-checked here.
 * cnr_occmap_grad: an OccupancyMap (src/model.py:129-147: in_layer, mid1, cat_layer, mid2, out_alpha).  theta: the flat
 * concatenation of the module's parameters in registration order (in_layer.0 W (H,87) b | mid1.0.0 W (H,H) b | cat_layer.0 W
 * (H,H+87) b | mid2.0.0 W (H,H) b | out_alpha W (1,H) b | ...; the colour layers behind them are not read), B (21,3).
 * H = 32 or 128; any other H returns CNR_E_SHAPE before anything else is looked at. */
int cnr_field_grad(const float* pts, const int* row, const float* B, const float* trunk, const float* biasrows,
                   float scale, int64_t N, float* sigma, float* grad, void* stream);
int cnr_occmap_grad(const float* pts, const float* theta, const float* B, int H, float scale, int64_t N,
                    float* sigma, float* grad, void* stream);

/* ---- surface normals of a rendered view (csrc/view.hip).  After cnr_view_composite on the same P pixels.
 * cnr_view_surface_points: per pixel the winning segment = the one cnr_view_composite took the label from (the largest entry of
 * its mass row, the earlier one among equals), its entity e = seg_entity[.], or none when the pixel has no segment or opacity <
 * opacity_threshold; the surface point = to_field[e] . (T_wc . (depth d, 1)) in cnr_view_points' expressions at z = the rendered
 * depth.  The pixels with a surface are bucketed by field run, run = entity_run[e] in [0, n_runs): a compact list in (run, pixel)
 * order, run r owning [run_offset[r], run_offset[r+1]), run_offset (n_runs + 1,) i64 on the device, M = run_offset[n_runs] <= P.
 * Outputs: surf_entity (P,) i32 (-1: none), surf_slot (P,) i32 = the pixel's place in the list (-1: none), surf_pts (P,3) (zero
 * for none), list_pts (P,3) and list_row (P,) i32 = entity_row[e], of which the first M entries are written.
 * workspace >= cnr_view_surface_workspace_bytes(P, n_runs).  P < 2^31, n_runs <= 32767 (else CNR_E_SHAPE).  No atomics.
 * cnr_view_normals: grad_c (M,3) = d sigma / d x at list_pts in the field frame -> normal (P,3) = -A^T g / |A^T g| with A =
 * to_field[surf_entity[p]][:, :3] and g = grad_c[surf_slot[p]]: the world-frame unit vector out of the surface, towards
 * decreasing occupancy; exactly zero where the pixel has no surface or A^T g is zero (or not finite).  Every pixel is written. */
int64_t cnr_view_surface_workspace_bytes(int64_t P, int n_runs);
int cnr_view_surface_points(const float* T_wc, const float* dirs, const float* to_field, const float* depth,
                            const float* opacity, float opacity_threshold, const float* mass, const int* pix_segs,
                            const int* seg_entity, const int* entity_run, const int* entity_row, int64_t P, int n_runs,
                            void* workspace, int64_t* run_offset, int* surf_entity, int* surf_slot, float* surf_pts,
                            float* list_pts, int* list_row, void* stream);
int cnr_view_normals(const float* grad_c, const int* surf_slot, const int* surf_entity, const float* to_field, int64_t P,
                     int64_t M, float* normal, void* stream);

/* ---- mesh rasterisation: which pixel sees which triangle at what z-depth (csrc/raster.hip).
 * verts (Nv,3) f32, faces (F,3) i32 (indices are NOT range-checked here: cnr_amd.raster.MeshScene does), T_cw (V,4,4) f64
 * row-major world -> camera, dirs (W*H,3) f32 = the cameraInfo cache rows, pixel (w,h) at row w H + h, of the intrinsics fx fy
 * cx cy.  All images are (V,W,H,...).  0 <= zmin <= zmax; 1 <= W, H <= 32768; V >= 1; 1 <= F < 2^31; F V <= 2^40; V x tiles < 2^31
 * with tiles = ceil(W / 8) ceil(H / 8) (else CNR_E_SHAPE).  workspace >= cnr_raster_workspace_bytes(F, V, W, H) and the SAME
 * workspace goes through bin_count -> bin_emit -> tiles -> attributes.
 *
 * Coverage (fp64, no contraction, as parenthesised): v_k = ((T_r0 x + T_r1 y) + T_r2 z) + T_r3 per row r of T_cw; n0 = v1 x v2,
 * n1 = v2 x v0, n2 = v0 x v1 with (a x b).x = a.y b.z - a.z b.y and so on; det = (v0.x n0.x + v0.y n0.y) + v0.z n0.z,
 * s = sign(det), det == 0 covers nothing.  Per pixel, d = (dx, dy, 1) widened from dirs: e_i = (n_i.x dx + n_i.y dy) + n_i.z,
 * S = (e0 + e1) + e2, t = det / S; covered iff s e_i >= 0 (all i), s S > 0, zmin <= t <= zmax.  Winner: smallest (t, face).
 *
 * cnr_raster_bin_count: the records, a conservative box of 8 x 8 pixel tiles per (view, face) (the triangle cut at z >=
 * max(zmin, 2^-13), projected, grown by one pixel, clamped; every tile for a face that comes nearer than 2^-13 where a pixel
 * could still see it, which only zmin < 2^-13 allows; none for det == 0, for a face wholly nearer than zmin, and with cull_backfaces for
 * det < 0), the per-(view, tile) list lengths and starts; n_pairs (1,) i64 on the device = the number of (view, tile, face)
 * pairs.  cnr_raster_bin_emit: pair_face (n_pairs,) i32, the lists (integer cursors: the order inside a list is not fixed, the
 * images are).  cnr_raster_tiles: depth f32 (0: no hit; else t rounded once), face i32 (-1: no hit), bary (.,2) f32 = e1 / S,
 * e2 / S of the winner (0: no hit); every pixel is written.
 * cnr_raster_attributes: from face_img (the face image of cnr_raster_tiles on the same workspace) and fp64 barycentrics b_i =
 * e_i / S recomputed from the records: rgb = (b0 c0 + b1 c1) + b2 c2 of colors (Nv,3), instance = face_label[face] (-1: no
 * hit), normal (world frame, unit): vertex_normals = 0 the geometric normal (p1 - p0) x (p2 - p0) turned so that n . d_world < 0,
 * vertex_normals = 1 the normalised (b0 N0 + b1 N1) + b2 N2 of normals (Nv,3) with its sign as given; exactly zero where nothing
 * was hit or the vector vanishes.
 * cnr_raster_visible: seen (F,) u8 |= 1 and count (F,) i32 += the number of the V views in which the face won a pixel; with
 * depth_obs (V,W,H) (may be NULL, then depth may be too) a pixel counts only if depth_obs > 0 and (double)depth <=
 * (double)depth_obs + tol.  Plain stores of one value, no atomics; the caller zeroes seen and count before the first call.
 * workspace >= cnr_raster_visible_workspace_bytes(F, V).  No floating-point atomics anywhere; bit-identical run to run. */
int64_t cnr_raster_workspace_bytes(int64_t F, int V, int W, int H);
int cnr_raster_bin_count(const float* verts, const int* faces, int64_t F, const double* T_cw, int V, int W, int H,
                         double fx, double fy, double cx, double cy, double zmin, int cull_backfaces, void* workspace,
                         int64_t* n_pairs, void* stream);
int cnr_raster_bin_emit(int64_t F, int V, int W, int H, void* workspace, int* pair_face, void* stream);
int cnr_raster_tiles(const float* dirs, int64_t F, int V, int W, int H, double zmin, double zmax,
                     const void* workspace, const int* pair_face, float* depth, int* face, float* bary,
                     void* stream);
int cnr_raster_attributes(const float* dirs, const float* verts, const int* faces, const float* colors,
                          const float* normals, const int* face_label, const double* T_cw, int64_t F, int V, int W,
                          int H, int vertex_normals, const void* workspace, const int* face_img, float* rgb,
                          int* instance, float* normal, void* stream);
int64_t cnr_raster_visible_workspace_bytes(int64_t F, int V);
int cnr_raster_visible(const int* face_img, const float* depth, const float* depth_obs, double tol, int64_t F, int V,
                       int W, int H, void* workspace, uint8_t* seen, int* count, void* stream);

/* ---- the mesh as a graph: components, edge statistics, compaction, welding (csrc/mesh_topo.hip) ----
 * faces (F,3) i32 into V vertices, F <= (2^31 - 1) / 3, V < 2^31.  err (1,) i32 on the device, zeroed by the caller, is OR-ed
 * with 1 when a bounded union/find or flatten loop ran out and with 2 when an index outside its range was met (and skipped).
 * Integer atomics only (minima, counts); bit-identical run to run.
 *
 * check_faces: err |= 2 when a face index is outside [0, V); the other entry points trust faces only after that.
 * labels_init: L[i] = i.  union_pairs: joins pairs (m,2) i32 of elements of [0, n).  union_faces (vertex connectivity): joins
 * (v0,v1), (v0,v2) of every face and sets used[v] = 1 (used (V,) u8, zeroed by the caller).  edge_keys: keys (3F,) i64,
 * keys[3 f + k] = min << 32 | max of corners k, (k + 1) % 3, or -1 when they are equal.  union_edges (edge connectivity): keys
 * sorted stably, perm (3F,) i64 = the slots 3 f + k in sorted order; joins the faces of neighbouring equal keys >= 0.
 * flatten: afterwards L[i] = the smallest element of i's set (workspace >= cnr_mesh_flatten_workspace_bytes(n)).
 * roots_count/_emit: the i with L[i] == i and (used == NULL or used[i]), ascending, roots (C,) i32; the rank is the component id.
 * assign: comp[i] = the rank of L[i] in roots, -1 where used[i] == 0.  cross_component: mode 0 vertex_component (V,) = the
 * smallest face_component over the faces that use the vertex, -1 for none; mode 1 face_component[f] = vertex_component[v0].
 * edge_stats: counts (C,3) i32 zeroed by the caller; per run of equal keys of multiplicity m, for the component c of its first
 * face: counts[c][0] += m == 1 (boundary), [1] += m > 2 (non-manifold), [2] += m == 2 and both faces run the edge the same way.
 * component_stats: order (F,) i64 = the faces stably sorted by component, sorted_component (F,) i32 their components;
 * n_faces, n_vertices (C,) i32 (a vertex counts for vertex_component[v]), and with verts (V,3) f32 != NULL area (C,) f64,
 * bbox_min/max (C,3) f32 -- per-face areas and boxes into workspace (>= cnr_mesh_component_stats_workspace_bytes(F); may be
 * NULL without verts), then one wave per component; the exact order of operations is in csrc/mesh_topo.hip.
 * compact_count/_emit: the faces with keep_face != 0 in their old order; reindex != 0 re-indexes them to the vertices they use
 * in their old order (vertex_map (V,) i32, -1 = dropped; kept_vertices ascending), reindex == 0 keeps their indices
 * (vertex_map, kept_vertices may be NULL).  counts_out (2,) i64 = kept faces, kept vertices (0 without reindex).
 * weld_runs: perm (V,) i64 = the vertices in sorted order; rows (V,3) i32 the positions' bit patterns in INPUT order (exact
 * mode) or sorted_keys (V,) i64 in SORTED order (cell mode), exactly one of them; a sorted position starts a run when it is
 * the first, differs from its predecessor, holds a NaN (rows) or is -1 (keys); rep[perm[j]] = perm[head of j's run].
 * remap_faces: out = remap[faces], keep[f] = 0 when drop_degenerate and two corners of out coincide, else 1. */
int cnr_mesh_check_faces(const int* faces, int64_t F, int64_t V, int* err, void* stream);
int cnr_mesh_labels_init(int* labels, int64_t n, void* stream);
int cnr_mesh_union_pairs(const int* pairs, int64_t m, int64_t n, int* labels, int* err, void* stream);
int cnr_mesh_union_faces(const int* faces, int64_t F, int64_t V, int* labels, uint8_t* used, int* err, void* stream);
int cnr_mesh_edge_keys(const int* faces, int64_t F, int64_t* keys, void* stream);
int cnr_mesh_union_edges(const int64_t* sorted_keys, const int64_t* perm, int64_t F, int* labels, int* err, void* stream);
int64_t cnr_mesh_flatten_workspace_bytes(int64_t n);
int cnr_mesh_flatten(int* labels, int64_t n, void* workspace, int* err, void* stream);
int64_t cnr_mesh_roots_workspace_bytes(int64_t n);
int cnr_mesh_roots_count(const int* labels, const uint8_t* used, int64_t n, void* workspace, int64_t* count_out,
                         void* stream);
int cnr_mesh_roots_emit(const int* labels, const uint8_t* used, int64_t n, const void* workspace, int* roots, void* stream);
int cnr_mesh_assign(const int* labels, const uint8_t* used, int64_t n, const int* roots, int64_t C, int* comp, int* err,
                    void* stream);
int cnr_mesh_cross_component(const int* faces, int64_t F, int64_t V, int mode, int* face_component, int* vertex_component,
                             void* stream);
int cnr_mesh_edge_stats(const int64_t* sorted_keys, const int64_t* perm, const int* faces, int64_t F,
                        const int* face_component, int64_t C, int* counts, void* stream);
int64_t cnr_mesh_component_stats_workspace_bytes(int64_t F);
int cnr_mesh_component_stats(const float* verts, const int* faces, const int64_t* order, const int* sorted_component,
                             int64_t F, int64_t V, int64_t C, const int* vertex_component, void* workspace, int* n_faces,
                             int* n_vertices, double* area, float* bbox_min, float* bbox_max, void* stream);
int64_t cnr_mesh_compact_workspace_bytes(int64_t F, int64_t V);
int cnr_mesh_compact_count(const int* faces, int64_t F, int64_t V, const uint8_t* keep_face, int reindex, void* workspace,
                           int64_t* counts_out, void* stream);
int cnr_mesh_compact_emit(const int* faces, int64_t F, int64_t V, const uint8_t* keep_face, int reindex,
                          const void* workspace, int* out_faces, int* vertex_map, int* kept_vertices, void* stream);
int cnr_weld_runs(const int* rows, const int64_t* sorted_keys, const int64_t* perm, int64_t V, int* rep, int* err,
                  void* stream);
int cnr_mesh_remap_faces(const int* faces, int64_t F, const int* remap, int drop_degenerate, int* out_faces, uint8_t* keep,
                         void* stream);

/* ---- orientation repair: consistent winding per patch, outward patches (csrc/mesh_topo.hip) ----
 * faces, F, V, err as above; integer atomics only, no floating-point atomic, every loop bounded, bit-identical run to run.
 * A face with two equal corners is degenerate: it has no edges, is a patch of its own and is never flipped.  A LINK is a run of
 * exactly two equal keys in the sorted edge keys: its faces f < g and rel = 1 when both run the edge in the same direction.
 * Patches are the connected components of the faces under links, numbered by their smallest face.
 *
 * orient_keys: cnr_mesh_edge_keys with all three keys of a degenerate face -1.  Sort them stably as for union_edges.
 * orient_union: words (F,) i32, word = parent << 1 | parity (F < 2^30); sets words[i] = i << 1, then joins the two faces of
 * every link with the parity its rel demands (csrc/mesh_topo_common.h: find_parity, unite_parity).
 * orient_flatten: pointer-jumping sweeps with the parities XOR-ed along (workspace >= cnr_mesh_flatten_workspace_bytes(F)),
 * then labels[i] = the smallest face of i's patch (for cnr_mesh_roots_* / cnr_mesh_assign) and flip0 (F,) u8 = i's parity
 * relative to it.
 * orient_check: face_patch (F,) i32 from cnr_mesh_assign, C patches.  bad (C,) i32 = 1 where a link has
 * flip0[f] ^ flip0[g] != rel (the patch is not orientable); counts (C,2) i32 = the edge slots of the patch that lie in no run
 * of two (0: the patch is closed), and its links with rel == 1 in the input; both zeroed here.  Then flip0 = 0 on every face
 * of a bad patch.
 * orient_stats: order (F,) i64 = the faces stably sorted by patch, sorted_patch (F,) i32; n_faces, n_flipped (C,) i32,
 * sign (C,) u8; workspace >= cnr_mesh_orient_stats_workspace_bytes(F).  With verts (V,3) f32 != NULL, per patch: its fp32
 * vertex box (exact minima and maxima, taken by integer atomics on an order-preserving image of the floats), c = 0.5 * (min +
 * max) in fp64, s = sum over its faces (flip0 applied) of (a - c) . ((b - c) x (d - c)) in fp64, one wave per patch in the fixed
 * order written out in csrc/mesh_topo.hip; sign = outward != 0 and the patch is orientable and s < 0; signed_volume (C,) f64 =
 * (sign ? -s : s) / 6.  Without verts sign = 0 and signed_volume may be NULL.  n_flipped counts flip0 ^ sign.
 * orient_apply: flip (F,) u8 = flip0 ^ sign[face_patch]; out_faces = (a, d, b) where flip is set, (a, b, d) elsewhere. */
int cnr_mesh_orient_keys(const int* faces, int64_t F, int64_t* keys, void* stream);
int cnr_mesh_orient_union(const int64_t* sorted_keys, const int64_t* perm, const int* faces, int64_t F, int* words, int* err,
                          void* stream);
int cnr_mesh_orient_flatten(int* words, int64_t F, void* workspace, int* labels, uint8_t* flip0, int* err, void* stream);
int cnr_mesh_orient_check(const int64_t* sorted_keys, const int64_t* perm, const int* faces, int64_t F, const int* face_patch,
                          int64_t C, uint8_t* flip0, int* bad, int* counts, int* err, void* stream);
int64_t cnr_mesh_orient_stats_workspace_bytes(int64_t F);
int cnr_mesh_orient_stats(const float* verts, const int* faces, const int64_t* order, const int* sorted_patch,
                          const int* face_patch, int64_t F, int64_t V, int64_t C, const uint8_t* flip0, const int* bad,
                          int outward, void* workspace, int* n_faces, int* n_flipped, uint8_t* sign, double* signed_volume,
                          void* stream);
int cnr_mesh_orient_apply(const int* faces, int64_t F, const int* face_patch, int64_t C, const uint8_t* flip0,
                          const uint8_t* sign, int* out_faces, uint8_t* flip, void* stream);

/* ---- mesh simplification: uniform vertex clustering with quadric placement (csrc/mesh_simplify.hip) ----
 * The clusters are the cells of cnr_voxel_keys, numbered by cnr_weld_runs / cnr_mesh_roots_* / cnr_mesh_assign; the faces go
 * through cnr_mesh_remap_faces and cnr_mesh_compact_*.  These entry points add the fp64 part and the face rows.  No
 * floating-point atomics, every sum in an order fixed by the data, bit-identical run to run; none needs a workspace.  err (1,)
 * i32 on the device, zeroed by the caller, as above: |= 2 for an index outside its range (the entry is skipped), |= 4 for a
 * vertex without a cell (key -1).  The arithmetic, operation by operation, is csrc/mesh_simplify_common.h.
 *
 * check_keys: err |= 4 when a key (V,) i64 is negative.  vertex_q: q (V,3) f64 = (double)verts - (double)min_xyz.
 * face_records: records (F,10) f64 per face, with q as above, n = (q1 - q0) x (q2 - q0) (products rounded, then the difference),
 * d = (nx q0x + ny q0y) + nz q0z: nx nx, nx ny, nx nz, ny ny, ny nz, nz nz, nx d, ny d, nz d, d d.
 * face_normals_f64: normals (F,3) f64 = (p1 - p0) x (p2 - p0) of the fp32 corners as doubles.
 * segment_sum_f64: items (n_items,K) f64, 1 <= K <= 16; position j < N belongs to segment sorted_seg[j] (i32, ascending) and
 * takes item gather[j] / gather_div (gather (N,) i64; NULL: item j); out (C,K) f64.  A group of 16 lanes per segment: lane l
 * adds the segment's positions l, l + 16, ... in ascending order from 0.0, then a[l] += a[l ^ 8], ^ 4, ^ 2, ^ 1, lane 0 writes;
 * an empty segment gives zeros.
 * place: per cluster c < C with representative roots[c] and cell keys[roots[c]] (keys (V,) i64 in INPUT order); quadrics (C,10)
 * and possum (C,3) the segment sums of the records and of q; sorted_cluster (V,) i32 the vertices' clusters sorted (for the
 * count).  placement 0: x = mean + pinv_tau(A) (b - A mean) by a cyclic Jacobi decomposition, eigenvalues <= tau * the largest
 * dropped; 1: the mean; both clamped per axis to [(i - 0.5) cell, (i + 0.5) cell], moved back by + min and rounded to fp32
 * (stepped one unit in the last place back when that rounding left the cell); 2: verts[roots[c]] as it is (possum and
 * sorted_cluster may be NULL).  error (C,) f64 = x^T A x - 2 b^T x + c at the fp64 position, clamped (C,) u8.
 * face_rows: rows (F,3) i32 = the face rotated so that its smallest index leads.  normals_finish: out (V,3) f32 = sums (V,3) f64
 * divided by their length sqrt((x x + y y) + z z), zeros where that is 0 or not finite. */
int cnr_simplify_check_keys(const int64_t* keys, int64_t V, int* err, void* stream);
int cnr_simplify_vertex_q(const float* verts, const float* min_xyz, int64_t V, double* q, void* stream);
int cnr_simplify_face_records(const float* verts, const int* faces, const float* min_xyz, int64_t F, int64_t V,
                              double* records, int* err, void* stream);
int cnr_mesh_face_normals_f64(const float* verts, const int* faces, int64_t F, int64_t V, double* normals, int* err,
                              void* stream);
int cnr_segment_sum_f64(const double* items, const int64_t* gather, int gather_div, const int* sorted_seg, int64_t N,
                        int64_t n_items, int K, int64_t C, double* out, int* err, void* stream);
int cnr_simplify_place(const double* quadrics, const double* possum, const int* sorted_cluster, const float* verts,
                       const int* roots, const int64_t* keys, const float* min_xyz, int64_t V, int64_t C, double cell,
                       double tau, int placement, float* out_verts, double* error, uint8_t* clamped, int* err, void* stream);
int cnr_simplify_face_rows(const int* faces, int64_t F, int* rows, void* stream);
int cnr_mesh_normals_finish(const double* sums, int64_t V, float* out, void* stream);

/* ---- image-space view scores: PSNR, SSIM, depth L1 and mask IoU sums per (image, row) (csrc/image_metric.hip; DESIGN.md
 * section 3.18).  N pairs of W x H images, (N,W,H,...) contiguous, pixel (w,h) at w H + h.  rgb_rec (N,W,H,3) f32; rgb_gt f32
 * (gt_u8 = 0) or u8 (gt_u8 = 1: a byte v enters as the double v / 255.0, an f32 as its exact double).  depth_rec, depth_gt
 * (N,W,H) f32, 0 = nothing there, both NULL with has_depth = 0.  label_rec, label_gt (N,W,H) i32, both NULL with has_labels = 0
 * (then K must be 0).  ids (K,) i32 on the device, strictly ascending (NOT checked here: the caller does, on the host),
 * 0 <= K <= 255; may be NULL with K = 0.  Row k < K: the pixels with label_gt == ids[k]; row K: every pixel.
 *
 * counts (7,N,K+1) i64, field-major: n_pix, n_ssim, n_both, n_only_rec, n_only_gt, n_rec, inter.  sums (3,N,K+1) f64: se,
 * ssim, depth_abs.  se = sum over the row's pixels and 3 channels of (a - b)^2 in double.  n_ssim / ssim: the row's pixels
 * whose 11 x 11 window lies inside the image, and the sum over them of S averaged over the channels; S is Wang et al.'s SSIM
 * with the normalised Gaussian weights exp(-i^2 / 4.5), i = -5..5, moments accumulated in double, C1 = 1e-4, C2 = 9e-4.  "hit"
 * is depth > 0: n_both, n_only_rec, n_only_gt count, depth_abs sums |double(rec) - double(gt)| over the pixels hit in both
 * (all 0 without depth).  Row k < K: n_rec = |label_rec == ids[k]|, inter = those with label_gt == ids[k] too; row K: n_rec =
 * W H and inter = |label_rec == label_gt| (both 0 without labels).  A NaN is not masked: it reaches the float sums of every
 * row that holds the pixel and no count.  ssim_map (N,W,H) f32 (may be NULL): the channel mean of S, 0 where the window is
 * not inside the image.  W < 11 or H < 11 is valid (n_ssim = 0).
 *
 * Tiles of CNR_IMG_TILE_W x CNR_IMG_TILE_H pixels with a 5-pixel halo; no floating-point atomics and no integer ones: every
 * sum is formed in an order fixed by W, H and the tile shape, so an image's rows are bit-identical from run to run and for
 * any N it is batched with.  workspace >= cnr_image_scores_workspace_bytes(N, W, H, K), 8-byte aligned.
 * CNR_E_ARG: W, H or N < 1, K outside 0..255, a required pointer NULL, a flag that contradicts its pointers, K > 0 without
 * labels.  CNR_E_SHAPE: N > 65535, W or H > 32768. */
#define CNR_IMG_TILE_W 16
#define CNR_IMG_TILE_H 32
int64_t cnr_image_scores_workspace_bytes(int N, int W, int H, int K);
int cnr_image_scores(const float* rgb_rec, const void* rgb_gt, int gt_u8, const float* depth_rec, const float* depth_gt,
                     int has_depth, const int* label_rec, const int* label_gt, int has_labels, const int* ids, int K, int N,
                     int W, int H, void* workspace, float* ssim_map, int64_t* counts, double* sums, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CNR_HIP_H */
