"""GPU: cnr_field_grad / cnr_occmap_grad point by point against the fp64 restatements of tests/fieldgrad_cpu.py, the normal image
of SceneRenderer.render(normals=True) and the field normals of Trainer.meshing.

The rule (tests/fieldgrad_cpu.py): a point whose smallest fp64 |ReLU pre-activation| is below 1e-5 may be left out (the
gradient of a ReLU network jumps there), at most 2 % of a case, asserted first.  Error per kept point |g - g64| / |g64|; the
yardstick is the largest such error of the same restatement in float32 on the CPU over the kept points of the weight set's
largest case; the kernel gets 4 x that, unit normals 8 x."""
import ctypes

import numpy as np
import pytest
import torch

import fieldgrad_cpu as F
import view_cpu as V
import view_scene as VS
from modular_cases import check

pytestmark = pytest.mark.gpu
CATS = ("s0", "s0_x3", "ckpt", "ckpt_x3")


@pytest.fixture(scope="module")
def cnr():
    import cnr_amd
    return cnr_amd


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _field_grad(cnr, dev, inp, pts, row, want_sigma=True):
    N = pts.shape[0]
    sigma, grad = (_nan(dev, N) if want_sigma else None), _nan(dev, N + 1, 3)          # one row more: must stay NaN
    cnr._C.call("cnr_field_grad", pts.to(dev), None if row is None else row.to(dev), inp["B"].to(dev), inp["trunk"].to(dev),
                inp["brows"].to(dev), inp["scale"], N, sigma, grad)
    torch.cuda.synchronize()
    assert torch.isnan(grad[N]).all() and torch.isfinite(grad[:N]).all()
    return sigma, grad[:N]


def _compare(what, g, g64, keep, yard, factor=4.0, err_fn=F.grad_error):
    assert float((~keep).double().mean()) <= F.MAX_LEFT_OUT, what
    err = err_fn(g, g64)[keep]
    worst = float(err.max()) if err.numel() else 0.0
    print(f"{what}: kept {int(keep.sum())} of {keep.numel()}, max error {worst:.3e}, yardstick {yard:.3e}, ratio {worst / yard:.2f}")
    assert worst <= factor * yard, (what, worst, yard)


@pytest.mark.parametrize("N", F.SIZES)
@pytest.mark.parametrize("name", CATS)
def test_field_grad_against_fp64(cnr, dev, name, N):
    inp = F.category_inputs(name)
    keep, s64, g64, yard, yard_s = F.category_yardstick(name)
    row = (torch.arange(N) % 4).int()                     # the bias row changes inside every wave
    sigma, grad = _field_grad(cnr, dev, inp, inp["pts"][:N], row)
    _compare(f"{name} N={N} grad", grad, g64[:N], keep[:N], yard)
    es = float((sigma.cpu().double() - s64[:N]).abs().max() / s64.abs().max())
    print(f"{name} N={N} sigma: {es:.3e} of max|sigma|, yardstick {yard_s:.3e}")
    assert es <= 4 * yard_s


@pytest.mark.parametrize("name", CATS)
def test_field_grad_sigma_null_row_null_and_repeat(cnr, dev, name):
    inp = F.category_inputs(name)
    keep, s64, g64, yard, yard_s = F.category_yardstick(name)
    N = 65
    pts, row = inp["pts"][:N], (torch.arange(N) % 4).int()
    sigma, grad = _field_grad(cnr, dev, inp, pts, row)
    sigma2, grad2 = _field_grad(cnr, dev, inp, pts, row)
    assert torch.equal(sigma, sigma2) and torch.equal(grad, grad2), "two launches must give the same bits"
    none, grad3 = _field_grad(cnr, dev, inp, pts, row, want_sigma=False)
    assert none is None and torch.equal(grad3, grad)
    # a point's result does not depend on where it stands: the same points inside the 4096-point launch
    _, big = _field_grad(cnr, dev, inp, inp["pts"], (torch.arange(4096) % 4).int())
    assert torch.equal(big[:N], grad)
    # row = NULL is row 0
    s0, g0 = _field_grad(cnr, dev, inp, pts, None)
    sz, gz = _field_grad(cnr, dev, inp, pts, torch.zeros(N, dtype=torch.int32))
    assert torch.equal(s0, sz) and torch.equal(g0, gz)
    r64 = F.category_reference(inp, pts, None)
    _compare(f"{name} row=NULL", g0, r64[1], F.kept_points(r64[2]), yard)


@pytest.mark.parametrize("name", CATS)
def test_field_grad_sigma_against_the_modular_kernels(cnr, dev, name):
    """sigma of cnr_pe_fwd + cnr_mlp_fwd_f32 on the same points (zlat rows per point), relative to max|sigma|"""
    inp = F.category_inputs(name)
    _, s64, _, _, yard_s = F.category_yardstick(name)
    N = 4096
    row = (torch.arange(N) % 4)
    sigma, _ = _field_grad(cnr, dev, inp, inp["pts"], row.int())
    e = torch.empty(1, N, 129, device=dev)
    cnr._C.call("cnr_pe_fwd", inp["pts"].to(dev), inp["B"].to(dev), e, 1, N, inp["scale"])
    sig, rgb = torch.empty(1, N, 1, device=dev), torch.empty(1, N, 1, 3, device=dev)
    cnr._C.call("cnr_mlp_fwd_f32", e, inp["zlat"][row].contiguous().to(dev), inp["trunk"].to(dev), sig, rgb, 1, N, 1)
    torch.cuda.synchronize()
    d = float((sigma.double() - sig.reshape(-1).double()).abs().max().cpu() / s64.abs().max())
    print(f"{name}: sigma vs modular kernels {d:.3e} of max|sigma|, yardstick {yard_s:.3e}")
    assert d <= 4 * yard_s


@pytest.mark.parametrize("name", ("s0", "ckpt"))
def test_autograd_through_the_modules_agrees(cnr, dev, name):
    inp = F.category_inputs(name)
    keep, s64, g64, yard, _ = F.category_yardstick(name)
    fc = cnr.model.CodeNeRF(87, 42, latent_dim=32).to(dev)
    fc.load_state_dict({k: v.to(dev) for k, v in inp["state"].items()})
    pe = cnr.embedding.UniDirsEmbed(max_deg=5, scale=inp["scale"]).to(dev)
    pe.B_layer.weight.data = inp["B"].to(dev)
    row = torch.arange(4096) % 4
    x = inp["pts"].to(dev).requires_grad_(True)
    sig, _ = fc(pe(x[:, None, :]), inp["shape_codes"][row][:, None, :].to(dev), inp["texture_codes"][row][:, None, :].to(dev))
    g, = torch.autograd.grad(sig.sum(), x)
    _compare(f"{name} autograd through the modules", g, g64, keep, yard)
    _, grad = _field_grad(cnr, dev, inp, inp["pts"], row.int())
    _compare(f"{name} kernel", grad, g64, keep, yard)


def _occ_modules(cnr, dev, inp):
    fc = cnr.model.OccupancyMap(87, 42, hidden_size=inp["H"]).to(dev)
    fc.load_state_dict({k: v.to(dev) for k, v in inp["state"].items()})
    pe = cnr.embedding.UniDirsEmbed(max_deg=5, scale=inp["scale"]).to(dev)
    pe.B_layer.weight.data = inp["B"].to(dev)
    return fc, pe


def _occmap_grad(cnr, dev, inp, pts):
    N = pts.shape[0]
    sigma, grad = _nan(dev, N), _nan(dev, N + 1, 3)
    cnr._C.call("cnr_occmap_grad", pts.to(dev), inp["theta"].to(dev), inp["B"].to(dev), inp["H"], inp["scale"], N, sigma, grad)
    torch.cuda.synchronize()
    assert torch.isnan(grad[N]).all() and torch.isfinite(grad[:N]).all()
    return sigma, grad[:N]


@pytest.mark.parametrize("name", ("h32", "h128"))
def test_occmap_grad_against_fp64(cnr, dev, name):
    inp = F.occmap_inputs(name)
    keep, s64, g64, yard, yard_s = F.occmap_yardstick(name)
    for N in F.OCC_SIZES:
        sigma, grad = _occmap_grad(cnr, dev, inp, inp["random"][:N])
        _compare(f"{name} random N={N}", grad, g64[:N], keep[:N], yard)
        assert float((sigma.cpu().double() - s64[:N]).abs().max() / s64.abs().max()) <= 4 * yard_s
    sigma2, grad2 = _occmap_grad(cnr, dev, inp, inp["random"][:4096])
    assert torch.equal(grad2, grad) and torch.equal(sigma2, sigma), "two launches must give the same bits"
    gs, gg, gm = F.occmap_reference(inp, inp["golden"])
    sigma, grad = _occmap_grad(cnr, dev, inp, inp["golden"])
    _compare(f"{name} golden points", grad, gg, F.kept_points(gm), yard)
    assert float((sigma.cpu().double() - gs).abs().max() / gs.abs().max()) <= 4 * yard_s
    # ops.occmap_grad on the modules is that launch
    fc, pe = _occ_modules(cnr, dev, inp)
    s_ops, g_ops = cnr.ops.occmap_grad(fc, pe, inp["golden"].to(dev))
    assert torch.equal(g_ops, grad) and torch.equal(s_ops, sigma)


def test_occmap_grad_other_hidden_sizes(cnr, dev):
    """H = 64: the entry point refuses the shape before it looks at a pointer; ops.occmap_grad falls back to autograd"""
    inp = F.occmap_inputs("h64")
    keep, s64, g64, yard, yard_s = F.occmap_yardstick("h64")
    lib = cnr._C.load()
    assert lib.cnr_occmap_grad(None, None, None, 64, ctypes.c_float(2.0), 8, None, None, None) == -2
    assert lib.cnr_occmap_grad(None, None, None, 32, ctypes.c_float(2.0), 0, None, None, None) == 0      # N = 0: nothing to do
    assert lib.cnr_field_grad(None, None, None, None, None, ctypes.c_float(2.0), 0, None, None, None) == 0
    fc, pe = _occ_modules(cnr, dev, inp)
    sigma, grad = cnr.ops.occmap_grad(fc, pe, inp["random"].to(dev))
    assert not grad.requires_grad and not sigma.requires_grad
    _compare("h64 fallback", grad, g64, keep, yard)
    assert float((sigma.cpu().double() - s64).abs().max() / s64.abs().max()) <= 4 * yard_s


# ---- the view --------------------------------------------------------------------------------------------------------------
SEED, S = 2, 16


@pytest.fixture(scope="module")
def scene(cnr, dev):
    cfg = VS.small_camera(cnr.cfg.synthetic_config(device=str(dev), latent_dim=32))
    cls_dict, scene_bg = VS.make_scene(cnr, cfg, seed=SEED)
    r = cnr.view.SceneRenderer(cls_dict, scene_bg, cfg)
    T = VS.camera_pose()
    with torch.no_grad():
        out = r.render(T, n_samples=S, return_samples=True, normals=True)
    return cfg, cls_dict, scene_bg, r, T, out


def _entity_reference(cnr, r, cls_dict, scene_bg, ent, pts, dtype):
    """fp64 / fp32 restatement of the entity's field at pts (float32, as the kernel got them)"""
    with torch.no_grad():
        if ent.cat < 0:
            t = scene_bg.trainer
            inp = dict(state={k: v.detach().cpu() for k, v in t.fc_occ_map.state_dict().items()}, B=t.pe.B_layer.weight.detach().cpu(),
                       scale=float(t.pe._scale))
            return F.occmap_reference(inp, pts, dtype)
        t = r.categories[ent.cat].trainer
        trunk, B, brows = t._codenerf_rows(ent.inst_id)
    inp = dict(trunk=trunk.reshape(-1).cpu(), B=B.reshape(21, 3).cpu(), scale=float(t.pe._scale), brows=brows.cpu())
    return F.category_reference(inp, pts, None, dtype)


def _check_view(cnr, r, cls_dict, scene_bg, T, out, what, transforms=None):
    s = out["samples"]
    ents = cnr.view.edited(r.entities, transforms)
    P = r.W * r.H
    flat = lambda k: out[k].reshape(P, *out[k].shape[2:]).cpu().numpy()
    mass, pix_segs, seg_entity = s["mass"].cpu().numpy(), s["pix_segs"].cpu().numpy(), s["seg_entity"].cpu().numpy()
    entity = F.winner_entity(mass, pix_segs, seg_entity, flat("opacity"), 0.5)
    assert np.array_equal(s["surface_entity"].cpu().numpy(), entity), what
    inst = flat("instance")
    assert np.array_equal(entity < 0, inst < 0)
    assert len(np.unique(entity[entity >= 0])) >= 3, "the view must show several fields"
    to_field = s["to_field"].cpu().numpy()
    T32, dirs = np.asarray(T, np.float32), r.dirs().cpu().numpy()
    p64 = F.surface_points(T32, dirs, to_field, flat("depth"), entity, np.float64)
    p32 = F.surface_points(T32, dirs, to_field, flat("depth"), entity, np.float32)
    check(s["surface_pts"].cpu(), torch.from_numpy(p64), torch.from_numpy(p32), f"{what} surface_pts")
    # the gradient at the kernel's own surface points
    spts = s["surface_pts"].cpu()
    g64, g32, minpre = torch.zeros(P, 3, dtype=torch.float64), torch.zeros(P, 3), torch.full((P,), np.inf, dtype=torch.float64)
    for e, ent in enumerate(ents):
        m = torch.from_numpy(np.nonzero(entity == e)[0])
        if len(m):
            _, g64[m], minpre[m] = _entity_reference(cnr, r, cls_dict, scene_bg, ent, spts[m], torch.float64)
            g32[m] = _entity_reference(cnr, r, cls_dict, scene_bg, ent, spts[m], torch.float32)[1]
    on = torch.from_numpy(entity >= 0)
    keep = F.kept_points(minpre[on])
    yard = float(F.grad_error(g32[on], g64[on])[keep].max())
    n64 = torch.from_numpy(F.normal_from_gradient(to_field, entity, g64.numpy()))
    normal = out["normal"].reshape(P, 3).cpu()
    err = (normal.double() - n64).norm(dim=-1)[on][keep]
    print(f"{what}: {int(on.sum())} surface pixels, normal error {float(err.max()):.3e}, gradient yardstick {yard:.3e}")
    assert float(err.max()) <= 8 * yard
    assert not normal[~on].any(), "the normal must be exactly zero where instance == -1"
    assert float((normal[on].double().norm(dim=-1) - 1).abs().max()) <= 4 * 2.0 ** -23
    return normal


def test_view_normals(cnr, dev, scene):
    cfg, cls_dict, scene_bg, r, T, out = scene
    assert out["normal"].shape == (cfg.W, cfg.H, 3) and out["normal"].dtype == torch.float32
    _check_view(cnr, r, cls_dict, scene_bg, T, out, "view")
    with torch.no_grad():
        plain = r.render(T, n_samples=S)
        small = r.render(T, n_samples=S, chunk=100, normals=True)
    assert "normal" not in plain
    for k in plain:
        assert torch.equal(plain[k], out[k]), k
    assert torch.equal(small["normal"], out["normal"]), "the normal image must not depend on the chunk"


def test_view_normals_follow_a_moved_object(cnr, dev, scene):
    cfg, cls_dict, scene_bg, r, T, out = scene
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = 1.2 * V.rot((0, 1, 0.3), 0.5), (0.3, 0.1, -0.2)
    with torch.no_grad():
        moved = r.render(T, n_samples=S, transforms={2: E}, return_samples=True, normals=True)
    assert not torch.equal(moved["normal"], out["normal"])
    _check_view(cnr, r, cls_dict, scene_bg, T, moved, "moved", transforms={2: E})


def test_view_normals_with_empty_space_skipping(cnr, dev, scene):
    cfg, cls_dict, scene_bg, r, T, out = scene
    r.build_grids(resolution=8)
    try:
        with torch.no_grad():
            skipped = r.render(T, n_samples=S, skip_empty=True, return_samples=True, normals=True)
    finally:
        r.set_grids(None)
    _check_view(cnr, r, cls_dict, scene_bg, T, skipped, "skip_empty")


def test_meshing_field_normals(cnr, dev, scene):
    cfg, cls_dict, scene_bg, r, T, out = scene
    t, inst = cls_dict[10].trainer, cls_dict[10].obj_ids[0]
    torch.manual_seed(0)
    grid = t.meshing(inst, grid_dim=16)
    field = t.meshing(inst, grid_dim=16, normals="field")
    again = t.meshing(inst, grid_dim=16, normals="grid")
    assert grid is not None and len(grid.vertices) > 50
    for a in ("vertices", "faces", "vertex_normals"):
        assert np.array_equal(getattr(grid, a), getattr(again, a)), a
    assert np.array_equal(field.vertices, grid.vertices) and np.array_equal(field.faces, grid.faces)
    assert not np.array_equal(field.vertex_normals, grid.vertex_normals)
    pts = torch.from_numpy(field.vertices).float()
    ent = next(e for e in r.entities if e.inst_id == inst)
    _, g64, mp = _entity_reference(cnr, r, cls_dict, scene_bg, ent, pts, torch.float64)
    g32 = _entity_reference(cnr, r, cls_dict, scene_bg, ent, pts, torch.float32)[1]
    keep = F.kept_points(mp)
    yard = float(F.grad_error(g32, g64)[keep].max())
    n = torch.from_numpy(field.vertex_normals)
    _compare("meshing field normals", n, g64, keep, yard, factor=8.0, err_fn=F.direction_error)
    assert float((n.norm(dim=-1) - 1).abs().max()) <= 4 * 2.0 ** -23
    # towards increasing occupancy, as the grid normals: the two agree in the large
    assert float((n * torch.from_numpy(grid.vertex_normals)).sum(-1).median()) > 0.5
    # eval_gradient is what it took them from
    s, g = t.eval_gradient(pts.to(dev), inst_id=inst)
    assert s.shape == (len(pts),) and g.shape == (len(pts), 3) and not g.requires_grad
    _compare("eval_gradient", g, g64, keep, yard)
