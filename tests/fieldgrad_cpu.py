"""TEST INFRASTRUCTURE for the field-gradient kernels (cnr_field_grad, cnr_occmap_grad) and the view normals built on them.

* the input sets the host and GPU tests share (weights of committed goldens, seeded points), built once;
* the geometry branches restated from oracle/ref_cpu.py (``unidirs_embed``, ``_lin``) under torch autograd, in any dtype:
  sigma, d sigma / d x and the smallest |ReLU pre-activation| of the geometry path per point;
* the exclusion rule and the error measure of the tests;
* the winner rule of cnr_view_composite, the surface point and n = -A^T g / |A^T g| in numpy float64;
* ``FieldGradDouble``: tests/cpu_double.Double plus the new entry points (and the dense layers / grid points the host tests
  of ``Trainer.eval_gradient`` and ``meshing(normals="field")`` pass through)."""
import functools
import os

import numpy as np
import torch

import mc_cpu as M
import view_cpu as V
from conftest import GOLDEN
from cpu_double import TRUNK, Double, _unpack
from oracle import ref_cpu as O

KINK = 1e-5          # a point whose smallest fp64 |pre-activation| is below this may be left out of a comparison
MAX_LEFT_OUT = 0.02  # ... but at most this share of a case
SIZES = (1, 63, 64, 65, 4096)
OCC_SIZES = (1, 65, 4096)
LATENT = ("shape_latent_layer_1.0", "cat_latent_layer.0", "shape_latent_layer_2.0", "texture_latent_layer_1.0")
_TARGETS = [(2816, 3840, 32), (4928, 8736, 119), (3872, 4896, 32), (12257, 13281, 32)]       # ops._LATENT_TARGETS
OCC_LAYERS = ("in_layer.0", "mid1.0.0", "cat_layer.0", "mid2.0.0", "out_alpha")


# ---- input sets --------------------------------------------------------------------------------------------------------------
def _bias_rows(trunk, state, codes_shape, codes_tex, factor):
    """(rows,4,32) float32 effective bias rows from float64 arithmetic: W_l relu(latent_l(code)) + b_l (state times factor)"""
    t = trunk.double()
    rows = []
    for k, ((wo, bo, ld), name) in enumerate(zip(_TARGETS, LATENT)):
        code = (codes_tex if k == 3 else codes_shape).double()
        z = torch.relu(code @ (state[name + ".weight"].double() * factor).T + state[name + ".bias"].double() * factor)
        Wk = t[wo:wo + 32 * ld].view(32, ld)[:, :32]
        rows.append(z @ Wk.T + t[bo:bo + 32])
    return torch.stack(rows, 1).float().contiguous()


@functools.lru_cache(maxsize=None)
def category_inputs(name):
    """name in s0, s0_x3, ckpt, ckpt_x3 (every weight and bias times 3) -> dict(trunk (13892,), B (21,3), scale, brows (4,4,32),
    pts (4096,3), state = the module's state_dict, shape_codes / texture_codes (4,32), zlat (4,4,32)), float32"""
    base, factor = (name[:-3], 3.0) if name.endswith("_x3") else (name, 1.0)
    if base == "s0":
        z = np.load(os.path.join(GOLDEN, "s0_c2_r64_s16_l32.npz"))
        state = {k[4:]: torch.from_numpy(z[k][0]) for k in z.files if k.startswith("mlp.")}
        B, scale = torch.from_numpy(z["B"][0]), float(z["scale"])
        cs, ct = torch.from_numpy(z["shape_codes"][0]), torch.from_numpy(z["texture_codes"][0])
    else:
        z = np.load(os.path.join(GOLDEN, "ckpt_ref.npz"))
        pre = "multi.FC_state_dict."
        state = {k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre) and not k.endswith(".keys")}
        B, scale = torch.from_numpy(z["multi.PE_state_dict.B_layer.weight"]), float(z["multi.PE_state_dict.scale"])
        cs, ct = torch.from_numpy(z["multi.shape_code_state_dict.weight"]), torch.from_numpy(z["multi.texture_code_state_dict.weight"])
        cs, ct = torch.cat([cs, -cs[:1]]), torch.cat([ct, -ct[:1]])                   # a fourth object
    trunk = torch.cat([t.reshape(-1) for n, _, _ in TRUNK for t in (state[n + ".weight"], state[n + ".bias"])]).float() * factor
    assert trunk.numel() == 13892 and cs.shape == (4, 32)
    rng = np.random.default_rng(11)
    pts = torch.from_numpy(rng.uniform(-1, 1, (4096, 3)).astype(np.float32))
    state = {k: (v.float() * factor).contiguous() for k, v in state.items()}           # the module's weights of this set
    zlat = torch.stack([torch.relu((ct if k == 3 else cs).double() @ state[n + ".weight"].double().T + state[n + ".bias"].double())
                        for k, n in enumerate(LATENT)], 1).float().contiguous()       # (4,4,32) post-ReLU latent outputs
    return dict(trunk=trunk.contiguous(), B=B.float().contiguous(), scale=scale, brows=_bias_rows(trunk, state, cs, ct, 1.0),
                pts=pts, state=state, shape_codes=cs.float().contiguous(), texture_codes=ct.float().contiguous(), zlat=zlat)


def _theta(state):
    return torch.cat([state[n + s].reshape(-1) for n in OCC_LAYERS + ("color_linear.0", "out_color") for s in (".weight", ".bias")]).float().contiguous()


@functools.lru_cache(maxsize=None)
def occmap_inputs(name):
    """name in h32, h128 (the bg goldens) or h64 (xavier, seeded) -> dict(theta, H, B (21,3), scale, state, golden (n,3) or
    None, random (4096,3))"""
    rng = np.random.default_rng(12)
    if name == "h64":
        H = 64
        g = torch.Generator().manual_seed(5)
        dims = [("in_layer.0", 87, H), ("mid1.0.0", H, H), ("cat_layer.0", H + 87, H), ("mid2.0.0", H, H), ("out_alpha", H, 1),
                ("color_linear.0", H + 42, H), ("out_color", H, 3)]
        state = {}
        for n, fi, fo in dims:
            state[n + ".weight"] = torch.randn(fo, fi, generator=g) * (2.0 / (fi + fo)) ** 0.5
            state[n + ".bias"] = (torch.rand(fo, generator=g) * 2 - 1) / fi ** 0.5
        B, scale, golden = torch.tensor(O.UNIDIRS).reshape(21, 3), 2.0, None
        lo, hi = -np.ones(3), np.ones(3)
    else:
        z = np.load(os.path.join(GOLDEN, {"h32": "bg_r100_s14_h32.npz", "h128": "bg_r240_s14_h128.npz"}[name]))
        state = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("mlp.")}
        H = state["out_alpha.weight"].shape[1]
        B, scale = torch.from_numpy(z["B"][0]), float(z["scale"])
        golden = torch.from_numpy(z["pts"].reshape(-1, 3).astype(np.float32))
        lo, hi = golden.numpy().min(0), golden.numpy().max(0)
    random = torch.from_numpy(rng.uniform(lo, hi, (4096, 3)).astype(np.float32))
    return dict(theta=_theta(state), H=H, B=B.float().contiguous(), scale=scale, state=state, golden=golden, random=random)


# ---- the restatements ---------------------------------------------------------------------------------------------------------
def _embed(x, B, scale):
    return O.unidirs_embed(x[None, :, None, :], B[None], scale)[..., :O.EMB1]         # (1,N,1,87)


def category_forward(trunk, B, scale, x, brow):
    """x (N,3), brow (N,4,32) the bias rows of every point, all of one dtype -> sigma (N,), [the four ReLU pre-activations]"""
    p = _unpack(trunk[None])
    nob = {k: (torch.zeros_like(v) if k.endswith(".bias") else v) for k, v in p.items()}
    e1 = _embed(x, B, scale)
    br = lambda k: brow[None, :, None, k, :]
    a0 = O._lin(p, "encoding_xyz.0", e1)
    a1 = O._lin(nob, "shape_layer_1.0", torch.relu(a0)) + br(0)
    a2 = O._lin(nob, "cat_layer.0", torch.cat((torch.relu(a1), e1), -1)) + br(1)
    a3 = O._lin(nob, "shape_layer_2.0", torch.relu(a2)) + br(2)
    y = O._lin(p, "encoding_shape", torch.relu(a3))
    return (O._lin(p, "sigma.0", y) * 10.0).reshape(-1), [a0, a1, a2, a3]


def occmap_forward(state, B, scale, x):
    p = {n + s: state[n + s][None] for n in OCC_LAYERS for s in (".weight", ".bias")}
    e1 = _embed(x, B, scale)
    a0 = O._lin(p, "in_layer.0", e1)
    a1 = O._lin(p, "mid1.0.0", torch.relu(a0))
    a2 = O._lin(p, "cat_layer.0", torch.cat((torch.relu(a1), e1), -1))
    a3 = O._lin(p, "mid2.0.0", torch.relu(a2))
    return (O._lin(p, "out_alpha", torch.relu(a3)) * 10.0).reshape(-1), [a0, a1, a2, a3]


def _with_gradient(forward, x):
    with torch.enable_grad():
        xv = x.detach().clone().requires_grad_(True)
        sigma, pre = forward(xv)
        grad, = torch.autograd.grad(sigma.sum(), xv)
    minpre = torch.stack([a.detach().abs().reshape(x.shape[0], -1).min(1).values for a in pre], 1).min(1).values
    return sigma.detach(), grad.detach(), minpre


def category_reference(inp, pts, row=None, dtype=torch.float64):
    """-> sigma (N,), grad (N,3), smallest |pre-activation| (N,), in `dtype` on the CPU; the float32 inputs as the kernel gets them"""
    c = lambda t: t.detach().cpu().to(dtype)
    rows = torch.zeros(pts.shape[0], dtype=torch.long) if row is None else row.detach().cpu().long()
    brow = c(inp["brows"])[rows]
    return _with_gradient(lambda x: category_forward(c(inp["trunk"]), c(inp["B"]), inp["scale"], x, brow), c(pts))


def occmap_reference(inp, pts, dtype=torch.float64):
    c = lambda t: t.detach().cpu().to(dtype)
    state = {k: c(v) for k, v in inp["state"].items()}
    return _with_gradient(lambda x: occmap_forward(state, c(inp["B"]), inp["scale"], x), c(pts))


# ---- the comparison rule ------------------------------------------------------------------------------------------------------
def kept_points(minpre64):
    """the points that take part in a comparison; asserts that at most 2 % of the case are left out"""
    keep = minpre64 >= KINK
    left = 1.0 - float(keep.double().mean())
    print("left out {:.3%} of {} points".format(left, keep.numel()))
    assert left <= MAX_LEFT_OUT, left
    return keep


def grad_error(g, g64):
    """|g - g64| / |g64| per point (float64)"""
    g, g64 = g.detach().cpu().double(), g64.detach().cpu().double()
    return (g - g64).norm(dim=-1) / g64.norm(dim=-1)


def direction_error(n, g64):
    """|n - g64 / |g64|| per point"""
    n, g64 = n.detach().cpu().double(), g64.detach().cpu().double()
    return (n - g64 / g64.norm(dim=-1, keepdim=True)).norm(dim=-1)


@functools.lru_cache(maxsize=None)
def category_yardstick(name):
    """of the weight set's largest case (4096 points, row = arange % 4): (keep mask, fp64 sigma, fp64 grad, the float32
    restatement's largest gradient error over the kept points, its largest |sigma - sigma64| / max|sigma64|)"""
    inp = category_inputs(name)
    row = (torch.arange(4096) % 4).int()
    s64, g64, mp = category_reference(inp, inp["pts"], row)
    s32, g32, _ = category_reference(inp, inp["pts"], row, torch.float32)
    keep = kept_points(mp)
    return keep, s64, g64, float(grad_error(g32, g64)[keep].max()), float((s32.double() - s64).abs().max() / s64.abs().max())


@functools.lru_cache(maxsize=None)
def occmap_yardstick(name):
    inp = occmap_inputs(name)
    s64, g64, mp = occmap_reference(inp, inp["random"])
    s32, g32, _ = occmap_reference(inp, inp["random"], torch.float32)
    keep = kept_points(mp)
    return keep, s64, g64, float(grad_error(g32, g64)[keep].max()), float((s32.double() - s64).abs().max() / s64.abs().max())


# ---- view: winner, surface point, normal --------------------------------------------------------------------------------------
def winner_entity(mass, pix_segs, seg_entity, opacity, thr):
    """cnr_view_composite's label rule restated: per pixel the segment of the largest mass of its row (the earlier one among
    equals) -> its entity, or -1 for an empty row or opacity < thr"""
    P, K = pix_segs.shape
    out = np.full(P, -1, np.int32)
    for p in range(P):
        best, best_seg = -1.0, pix_segs[p, 0]
        for j in range(K):
            if pix_segs[p, j] < 0:
                break
            if mass[p, j] > best:
                best, best_seg = mass[p, j], pix_segs[p, j]
        if best_seg >= 0 and opacity[p] >= thr:
            out[p] = seg_entity[best_seg]
    return out


def surface_points(T, dirs, to_field, depth, entity, dtype):
    """to_field[entity] . (T . (depth d, 1)) by view_cpu.points (one sample of a segment [depth, depth]); zero where entity < 0"""
    pix = np.nonzero(entity >= 0)[0]
    out = np.zeros((len(entity), 3), dtype)
    if len(pix):
        seg_z = np.stack([depth[pix], depth[pix]], 1)
        out[pix] = V.points(T, dirs, to_field, pix.astype(np.int32), entity[pix], seg_z, 1, dtype)[1][:, 0]
    return out


def normal_from_gradient(to_field, entity, g):
    """n = -A^T g / |A^T g| per pixel, A = to_field[entity][:, :3] (float64); zero where entity < 0 or A^T g = 0"""
    A = np.asarray(to_field, np.float64)[np.maximum(entity, 0)][:, :, :3]
    v = -np.einsum("pkj,pk->pj", A, np.asarray(g, np.float64))
    ln = np.linalg.norm(v, axis=1, keepdims=True)
    ok = (ln > 0) & (entity >= 0)[:, None]
    return np.where(ok, v / np.where(ln > 0, ln, 1.0), 0.0)


# ---- the test double ----------------------------------------------------------------------------------------------------------
class FieldGradDouble(Double):
    """cpu_double.Double plus cnr_field_grad / cnr_occmap_grad by the restatements above in the tensors' own dtype, and what
    the host tests of Trainer.eval_gradient and meshing pass through on the way: the dense layers and the grid points."""

    def cnr_field_grad(self, pts, row, B, trunk, biasrows, scale, N, sigma, grad):
        inp = dict(trunk=trunk.reshape(-1), B=B.reshape(21, 3), scale=scale, brows=biasrows)
        s, g, _ = category_reference(inp, pts, row, pts.dtype)
        if sigma is not None:
            sigma.copy_(s)
        grad.copy_(g)

    def cnr_occmap_grad(self, pts, theta, B, H, scale, N, sigma, grad):
        if H not in (32, 128):
            return -2
        state, off = {}, 0
        for n, o, i in (("in_layer.0", H, 87), ("mid1.0.0", H, H), ("cat_layer.0", H, H + 87), ("mid2.0.0", H, H), ("out_alpha", 1, H)):
            state[n + ".weight"] = theta[off:off + o * i].reshape(o, i); off += o * i
            state[n + ".bias"] = theta[off:off + o]; off += o
        s, g, _ = occmap_reference(dict(state=state, B=B.reshape(21, 3), scale=scale), pts, pts.dtype)
        if sigma is not None:
            sigma.copy_(s)
        grad.copy_(g)

    def cnr_dense_fwd(self, x, W, b, y, Mr, K, N, relu, f16):
        out = x @ W.T + (b if b is not None else 0)
        y.copy_(torch.relu(out) if relu else out)

    def cnr_dense_bwd(self, x, W, y, dy, dx, dW, db, Mr, K, N, relu, ws, wsb, f16, gs):
        dpre = dy * (y > 0) if relu else dy
        if dx is not None:
            dx.copy_(dpre @ W)
        dW.copy_(dpre.T @ x)
        if db is not None:
            db.copy_(dpre.sum(0))

    def cnr_grid_points(self, D, lo, hi, scale, transform, out):
        sc = None if scale is None else scale.numpy()
        tr = None if transform is None else transform.numpy()
        out.copy_(torch.from_numpy(M.grid_points(D, lo, hi, sc, tr)).reshape(out.shape))


def host_marching_cubes(vis):
    """a stand-in for vis.marching_cubes on a box without a GPU: tests/mc_cpu.py's restatement -> vis.Mesh"""
    def run(occupancy, level=0.5, gradient_direction="ascent"):
        out = M.marching_cubes(occupancy.detach().cpu().numpy(), level, gradient_direction == "ascent")
        return None if out is None else vis.Mesh(*[out[0], out[2], out[1]])
    return run
