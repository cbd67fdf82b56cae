"""The step tail's latent path and its AdamW restated in float64 (plain torch on the CPU, no kernel of the package).

cnr_step_tail / cnr_step_grad (csrc/tail.hip, csrc/latent_common.h) finish a category step: the latent backward from the
per-object bias-row sums, the code regulariser, AdamW in two parameter groups.  They switch code paths on the object count
and the code length (tail_path below); tests/test_tail_paths_gpu.py holds every path to these restatements, and
tests/test_tail_paths_host.py checks the restatements themselves.

The flat parameter row of a class (fused.ParamLayout): [ trunk 13892 | latent W (4,32,L) | latent b (4,32) | B 63 | shape codes
(n_obj,L) | texture codes (n_obj,L) ].  `lay` is such a layout: anything with .total and .views(flat (C, total)).
"""
import torch

TRUNK = 13892
# (weight offset, bias offset, row length) in the trunk blob of the layer each latent slot feeds: shape_layer_1, cat_layer,
# shape_layer_2, texture_layer_1 (csrc/latent_common.h, latent_target); the latent output meets the first 32 inputs of a row
LATENT_TARGETS = ((2816, 3840, 32), (4928, 8736, 119), (3872, 4896, 32), (12257, 13281, 32))
LATENT_TARGET_NAMES = ("shape_layer_1", "cat_layer", "shape_layer_2", "texture_layer_1")


def latent_trunk_blocks():
    """{name: int64 indices into the trunk blob}: the eight blocks the latent path reaches -- the [:, :32] weights (row-major
    (32, 32)) and the biases of the four latent-conditioned layers.  Every other trunk entry gets nothing from it."""
    out = {}
    for name, (wo, bo, ld) in zip(LATENT_TARGET_NAMES, LATENT_TARGETS):
        o, j = torch.meshgrid(torch.arange(32), torch.arange(32), indexing="ij")
        out[name + ".weight[:, :32]"] = (wo + o * ld + j).reshape(-1)
        out[name + ".bias"] = bo + torch.arange(32)
    return out


def latent_activations(views):
    """views of a float64 parameter buffer -> z (C, n_obj, 4, 32) = relu(Wl_k code_k + bl_k); slot 3 reads the texture code"""
    zs = []
    for k in range(4):
        code = views["tex"] if k == 3 else views["shape"]
        zs.append(torch.relu(torch.einsum("col,cnl->cno", views["latW"][:, k], code) + views["latb"][:, k][:, None, :]))
    return torch.stack(zs, dim=2)


def bias_rows(trunk, z):
    """trunk (C, 13892), z (C, n_obj, 4, 32) -> (C, n_obj, 4, 32): Wt_k[:, :32] z_k + bt_k, the bias each object hands the trunk"""
    C = trunk.shape[0]
    outs = []
    for k, (wo, bo, ld) in enumerate(LATENT_TARGETS):
        W = trunk[:, wo:wo + 32 * ld].reshape(C, 32, ld)[:, :, :32]
        outs.append(torch.einsum("coj,cnj->cno", W, z[:, :, k]) + trunk[:, bo:bo + 32][:, None, :])
    return torch.stack(outs, dim=2)


def latent_reference(theta64, lay, L, n_obj, C, rows64, reg, n_real=None):
    """The full (C, lay.total) float64 gradient of the latent path: autograd of

        sum(bias_rows(theta) * rows) + reg * sum over the class's REAL objects of (||shape code|| + ||texture code||)

    with z and the ReLU mask recomputed in float64.  rows64: the bias-row gradients (C n_obj, 4, 32) or (C, n_obj, 4, 32).
    n_real: objects each class really has (the rest of its rows are padding: no regulariser); None = n_obj everywhere.  A
    class with one real object has no regulariser at all (src/loss.py:5-15)."""
    th = theta64.detach().double().cpu().clone().requires_grad_()
    assert th.shape == (C, lay.total) and lay.L == L and lay.n_obj == n_obj
    v = lay.views(th)
    rws = bias_rows(v["trunk"], latent_activations(v))
    obj = (rws * rows64.detach().double().cpu().reshape(C, n_obj, 4, 32)).sum()
    for c in range(C):
        n = n_obj if n_real is None else int(n_real[c])
        assert 1 <= n <= n_obj
        if n > 1:
            obj = obj + reg * (torch.norm(v["shape"][c, :n], dim=-1).sum() + torch.norm(v["tex"][c, :n], dim=-1).sum())
    obj.backward()
    return th.grad.clone()


def adamw_reference(p, m, v, g, t, lr, wd, code_lr, code_wd, code_mask, b1=0.9, b2=0.999, eps=1e-8, dtype=torch.float64):
    """torch.optim.AdamW's update of step t (1-based) -> (p, exp_avg, exp_avg_sq) after it.  Two parameter groups: the
    elements of code_mask (bool, p's shape) take code_lr / code_wd, the rest lr / wd.  Decoupled decay, bias corrections from t.
    dtype = torch.float32 evaluates the same expression, in the order of csrc/adamw_common.h, with every intermediate rounded
    to fp32 (the coefficients step size and 1 / sqrt(bias correction 2) are formed in double and rounded once, as there)."""
    p, m, v, g = (x.detach().cpu().to(dtype) for x in (p, m, v, g))
    sc = lambda x: torch.tensor(x, dtype=torch.float64).to(dtype)    # a scalar rounded to dtype
    lr_, wd_, clr, cwd, b1_, b2_, eps_ = (sc(x) for x in (lr, wd, code_lr, code_wd, b1, b2, eps))
    one = sc(1.0)
    step_size = sc(float(lr_.double()) / (1.0 - float(b1_.double()) ** t))
    inv_bc2_sqrt = sc(1.0 / (1.0 - float(b2_.double()) ** t) ** 0.5)
    decay = torch.where(code_mask, one - clr * cwd, one - lr_ * wd_)
    step = torch.where(code_mask, step_size * (clr / lr_), step_size)
    pi = p * decay
    mi = m + (g - m) * (one - b1_)
    vi = v * b2_ + (one - b2_) * g * g
    denom = torch.sqrt(vi) * inv_bc2_sqrt + eps_
    pi = pi - step * (mi / denom)
    return pi, mi, vi


def latent_local_ok(L, n_obj):
    """csrc/latent_common.h: the per-block latent form takes a code length that divides 256 (at most 8 rows per block) or is a
    multiple of it, and up to 128 objects"""
    if L <= 0 or n_obj <= 0:
        return False
    if not (256 % L == 0 or L % 256 == 0):
        return False
    per = 1 if L >= 256 else 256 // L
    return n_obj <= 128 and per <= 8


def tail_path(L, n_obj):
    """Which latent blocks cnr_step_tail / cnr_step_grad run with a fixed-point table: "1trip" (latent_bwd_block_1trip), "local"
    (latent_bwd_block_local), "general" (load_rows_fix + latent_bwd_block) or "refused" (CNR_E_SHAPE).  A restatement of the
    dispatch in csrc/tail.hip, used to label the GPU cases and to assert that each joint has one."""
    if n_obj > 128 or (n_obj > 32 and not latent_local_ok(L, n_obj)):
        return "refused"
    outputs = 4 * 32 * L + 128 + 2 * n_obj * L
    NL = min(256, (outputs + 255) // 256)
    if n_obj <= 4 and L <= 256 and NL * 256 >= outputs:
        return "1trip"
    if n_obj >= 5 and latent_local_ok(L, n_obj):
        return "local"
    return "general"


# ---- the cases of tests/test_tail_paths_gpu.py: (L, n_obj, C, path) ------------------------------------------------------------
# L = 32: 8 objects per code block; 5 the first local count; 8 | 9 one round of the reducing blocks' latent-path term | two;
# 16 | 17 two rounds | three; 31, 32 | 33 one chunk of 32 code entries | two, and 8 x 33 = 264 d pre entries: a second pass;
# 64 | 65 two chunks | three; 100 the reference's n_models; 128 the limit (4096 table rows of a weight block: passes beyond 1024).
# L = 256: one row / object per block; 33 and 100 take table passes beyond 1024 rows.  L = 512: the norm loop beyond 256, and at
# three objects the general blocks because the block count is capped.  L = 48 divides nothing: 1trip up to four objects, then
# the general blocks up to 32, refused beyond.
SWEEP = ([(32, 2, 2, "1trip")]
         + [(32, n, 2, "local") for n in (5, 8, 9, 16, 17, 31, 32, 33, 64, 65, 100, 128)]
         + [(64, 20, 2, "local"), (128, 40, 2, "local"),
            (256, 5, 2, "local"), (256, 32, 2, "local"), (256, 33, 2, "local"), (256, 100, 1, "local"),
            (512, 6, 2, "local"), (512, 3, 2, "general"),
            (48, 3, 2, "1trip"), (48, 7, 2, "general"), (48, 32, 2, "general")])
REFUSED = [(48, 33, 2, "refused")]
# (C, n_obj, L, real objects per class)
RAGGED = [(3, 9, 32, (9, 1, 4)), (2, 40, 256, (40, 33)), (2, 4, 256, (4, 1)), (2, 7, 48, (7, 2))]
RAGGED_PATHS = ("local", "local", "1trip", "general")
