"""CPU: the host side of the field gradients -- the exclusion cap on every input set the GPU tests use, Trainer.eval_gradient /
ops.field_grad / ops.occmap_grad / meshing(normals="field") on the test double against autograd through the drop-in modules,
the winner rule and the normal transform, shade and the normal.png encoding, argument errors and return codes."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fieldgrad_cpu as F
import view_cpu as V
import view_scene as VS
from test_abi import assert_row_matches, declared_functions, load_library

NEW = ("cnr_field_grad", "cnr_occmap_grad", "cnr_view_surface_workspace_bytes", "cnr_view_surface_points", "cnr_view_normals")
SEED, S = 2, 16          # the scene of tests/test_fieldgrad_gpu.py


@pytest.fixture(scope="module")
def cnr():
    import cnr_amd
    return cnr_amd


@pytest.fixture()
def double(cnr):
    cnr._C.install_test_double(F.FieldGradDouble())
    yield
    cnr._C.install_test_double(None)


@pytest.fixture(scope="module")
def scene(cnr):
    cfg = VS.small_camera(cnr.cfg.synthetic_config(device="cpu", latent_dim=32))
    cls_dict, scene_bg = VS.make_scene(cnr, cfg, seed=SEED)
    return cfg, cls_dict, scene_bg, cnr.view.SceneRenderer(cls_dict, scene_bg, cfg)


# ---- the exclusion cap ---------------------------------------------------------------------------------------------------------
def test_exclusion_cap_on_the_kernel_cases():
    for name in ("s0", "s0_x3", "ckpt", "ckpt_x3"):
        keep = F.category_yardstick(name)[0]
        for N in F.SIZES:
            assert float((~keep[:N]).double().mean()) <= F.MAX_LEFT_OUT, (name, N)
        inp = F.category_inputs(name)
        F.kept_points(F.category_reference(inp, inp["pts"][:65], None)[2])            # the row = NULL case
    for name in ("h32", "h128", "h64"):
        keep = F.occmap_yardstick(name)[0]
        for N in F.OCC_SIZES:
            assert float((~keep[:N]).double().mean()) <= F.MAX_LEFT_OUT, (name, N)
        inp = F.occmap_inputs(name)
        if inp["golden"] is not None:
            F.kept_points(F.occmap_reference(inp, inp["golden"])[2])


def _entity_inputs(r, scene_bg, ent):
    if ent.cat < 0:
        t = scene_bg.trainer
        return "occ", dict(state={k: v.detach() for k, v in t.fc_occ_map.state_dict().items()}, B=t.pe.B_layer.weight.detach(),
                           scale=float(t.pe._scale))
    t = r.categories[ent.cat].trainer
    with torch.no_grad():
        trunk, B, brows = t._codenerf_rows(ent.inst_id)
    return "cat", dict(trunk=trunk.reshape(-1), B=B.reshape(21, 3), scale=float(t.pe._scale), brows=brows)


@pytest.mark.parametrize("moved", [False, True])
def test_exclusion_cap_on_the_view_cases(cnr, scene, moved):
    """the surface points of the restated render (float64 composite, oracle fields) of the GPU tests' scene and moved scene"""
    cfg, cls_dict, scene_bg, r = scene
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = 1.2 * V.rot((0, 1, 0.3), 0.5), (0.3, 0.1, -0.2)
    tr = {2: E} if moved else None
    T = VS.camera_pose()
    ref = VS.restated_render(r, cls_dict, scene_bg, T, S, np.float64, transforms=tr)
    ents = cnr.view.edited(r.entities, tr)
    entity = F.winner_entity(ref["mass"], ref["seg"]["pix_segs"], ref["seg"]["seg_entity"], ref["opacity"], 0.5)
    assert np.array_equal(entity < 0, ref["instance"] < 0) and (entity >= 0).sum() > 300
    to_field = np.stack([e.to_field for e in ents]).astype(np.float32)
    dirs = V.pinhole_dirs(r.W, r.H, cfg.fx, cfg.cx, cfg.cy)
    pts = F.surface_points(np.asarray(T, np.float32), dirs, to_field, ref["depth"], entity, np.float64).astype(np.float32)
    minpre = []
    for e, ent in enumerate(ents):
        m = np.nonzero(entity == e)[0]
        if len(m):
            kind, inp = _entity_inputs(r, scene_bg, ent)
            fn = F.occmap_reference if kind == "occ" else F.category_reference
            minpre.append(fn(inp, torch.from_numpy(pts[m]))[2])
    F.kept_points(torch.cat(minpre))


# ---- the Python surface on the double -------------------------------------------------------------------------------------------
def _autograd_category(t, inst_id, pts):
    idx = torch.tensor(t.inst_id_to_index[inst_id])
    cs, ct = t.shape_codes(idx).detach(), t.texture_codes(idx).detach()
    x = pts.clone().requires_grad_(True)
    sig, _ = t.fc_occ_map(t.pe(x[:, None, :]), cs.view(1, 1, -1).expand(len(x), 1, -1), ct.view(1, 1, -1).expand(len(x), 1, -1))
    g, = torch.autograd.grad(sig.sum(), x)
    return sig.detach().reshape(-1), g


def _autograd_occmap(t, pts):
    x = pts.clone().requires_grad_(True)
    sig = t.fc_occ_map(t.pe(x[:, None, :]), do_color=False)[0]
    g, = torch.autograd.grad(sig.sum(), x)
    return sig.detach().reshape(-1), g


def _agree(what, g, g_auto, ref):
    """both float32 evaluations within 4 x the float32 restatement's own error of the fp64 gradient, kink points left out"""
    _, g64, mp = ref(torch.float64)
    g32 = ref(torch.float32)[1]
    keep = F.kept_points(mp)
    yard = float(F.grad_error(g32, g64)[keep].max())
    for name, v in (("kernel path", g), ("autograd", g_auto)):
        err = float(F.grad_error(v, g64)[keep].max())
        print(f"{what} {name}: {err:.3e}, yardstick {yard:.3e}")
        assert err <= 4 * yard, (what, name)


def test_eval_gradient_category(cnr, scene, double):
    cfg, cls_dict, scene_bg, r = scene
    t = cls_dict[10].trainer
    pts = torch.from_numpy(np.random.default_rng(3).uniform(-0.8, 0.8, (500, 3)).astype(np.float32))
    for inst in cls_dict[10].obj_ids:
        sigma, grad = t.eval_gradient(pts, inst_id=inst, chunk_size=128)             # four chunks, the last one short
        assert sigma.shape == (500,) and grad.shape == (500, 3) and not grad.requires_grad
        s_auto, g_auto = _autograd_category(t, inst, pts)
        assert float((sigma - s_auto).abs().max()) <= 1e-5 * float(s_auto.abs().max())
        ent = next(e for e in r.entities if e.inst_id == inst)
        inp = _entity_inputs(r, scene_bg, ent)[1]
        _agree(f"object {inst}", grad, g_auto, lambda dt: F.category_reference(inp, pts, None, dt))


def test_eval_gradient_background_and_fallback(cnr, scene, double):
    cfg, cls_dict, scene_bg, r = scene
    t = scene_bg.trainer
    pts = torch.from_numpy(np.random.default_rng(4).uniform(-2.5, 2.5, (400, 3)).astype(np.float32))
    sigma, grad = t.eval_gradient(pts)
    s_auto, g_auto = _autograd_occmap(t, pts)
    assert float((sigma - s_auto).abs().max()) <= 1e-5 * float(s_auto.abs().max())
    inp = _entity_inputs(r, scene_bg, r.entities[0])[1]
    _agree("background", grad, g_auto, lambda dt: F.occmap_reference(inp, pts, dt))
    # hidden size 64: no kernel, autograd through the modules, silently
    inp64 = F.occmap_inputs("h64")
    fc = cnr.model.OccupancyMap(87, 42, hidden_size=64)
    fc.load_state_dict(inp64["state"])
    pe = cnr.embedding.UniDirsEmbed(max_deg=5, scale=inp64["scale"])
    pe.B_layer.weight.data = inp64["B"].clone()
    s, g = cnr.ops.occmap_grad(fc, pe, inp64["random"][:300])
    assert not g.requires_grad and not s.requires_grad
    keep, s64, g64, yard, _ = F.occmap_yardstick("h64")
    assert float(F.grad_error(g, g64[:300])[keep[:300]].max()) <= 4 * yard
    assert all(p.grad is None for p in fc.parameters())


def test_meshing_normals(cnr, scene, double, monkeypatch):
    cfg, cls_dict, scene_bg, r = scene
    t = scene_bg.trainer
    monkeypatch.setattr(cnr.vis, "marching_cubes", F.host_marching_cubes(cnr.vis))
    with pytest.raises(ValueError):
        t.meshing(grid_dim=8, normals="smooth")
    grid, default, field = t.meshing(grid_dim=10, normals="grid"), t.meshing(grid_dim=10), t.meshing(grid_dim=10, normals="field")
    assert grid is not None and len(grid.vertices) > 20
    for a in ("vertices", "faces", "vertex_normals"):
        assert np.array_equal(getattr(grid, a), getattr(default, a)), a
    assert np.array_equal(grid.visual.vertex_colors, default.visual.vertex_colors)
    assert np.array_equal(field.vertices, grid.vertices) and np.array_equal(field.faces, grid.faces)
    pts = torch.from_numpy(field.vertices).float()
    _, g_auto = _autograd_occmap(t, pts)
    inp = _entity_inputs(r, scene_bg, r.entities[0])[1]
    _, g64, mp = F.occmap_reference(inp, pts)
    g32 = F.occmap_reference(inp, pts, torch.float32)[1]
    keep = F.kept_points(mp)
    yard = float(F.grad_error(g32, g64)[keep].max())
    n = torch.from_numpy(field.vertex_normals)
    assert float((n.norm(dim=-1) - 1).abs().max()) <= 1e-12
    assert float(F.direction_error(n, g_auto.double())[keep].max()) <= 8 * yard        # + grad sigma, normalised
    assert float((n * torch.from_numpy(grid.vertex_normals)).sum(-1).median()) > 0      # the side the grid normals point to


# ---- winner rule and normal transform --------------------------------------------------------------------------------------------
def test_winner_rule():
    pix_segs = np.full((6, 8), -1, np.int32)
    mass = np.zeros((6, 8))
    pix_segs[0, :3], mass[0, :3] = (4, 2, 7), (0.2, 0.5, 0.1)          # the largest
    pix_segs[1, :3], mass[1, :3] = (0, 1, 3), (0.4, 0.4, 0.1)          # a tie: the earlier one
    pix_segs[2, :2], mass[2, :2] = (5, 6), (0.1, 0.3)                  # not opaque enough
    pix_segs[4, :1], mass[4, :1] = (8,), (0.9,)                        # an object that carries the background's id 0
    pix_segs[5, :2], mass[5, :2] = (9, 2), (0.0, 0.0)                  # no mass at all: the first, if opaque enough
    seg_entity = np.array([3, 1, 0, 2, 1, 0, 1, 2, 4, 2], np.int32)
    opacity = np.array([0.8, 0.9, 0.4, 0.0, 0.9, 0.6])
    assert F.winner_entity(mass, pix_segs, seg_entity, opacity, 0.5).tolist() == [0, 3, -1, -1, 4, 2]


def test_normal_transform_under_a_similarity():
    """sigma_w(w) = sigma_f(A w + t): its world gradient is A^T grad sigma_f, by finite differences, for a rotation and scale 1.7"""
    rng = np.random.default_rng(0)
    A = 1.7 * V.rot((0.3, -1, 0.2), 0.8)
    to_field = np.concatenate([A, rng.normal(size=(3, 1))], 1)[None]
    c, Q = rng.normal(size=3), rng.normal(size=(3, 3))
    sigma_f = lambda x: x @ c + 0.5 * np.einsum("...i,ij,...j->...", x, Q + Q.T, x)
    w = rng.normal(size=(5, 3))
    x = w @ A.T + to_field[0, :, 3]
    g = c + x @ (Q + Q.T)                                              # field-frame gradient
    h = 1e-6
    fd = np.stack([(sigma_f((w + h * np.eye(3)[k]) @ A.T + to_field[0, :, 3]) - sigma_f((w - h * np.eye(3)[k]) @ A.T + to_field[0, :, 3])) / (2 * h)
                   for k in range(3)], 1)
    n = F.normal_from_gradient(to_field, np.zeros(5, np.int32), g)
    assert np.abs(n + fd / np.linalg.norm(fd, axis=1, keepdims=True)).max() <= 1e-8
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() <= 1e-14
    ent = np.array([0, -1, 0, 0, 0], np.int32)
    g[2] = 0
    n = F.normal_from_gradient(to_field, ent, g)
    assert not n[1].any() and not n[2].any() and n[0].any()


# ---- shade, normal.png ------------------------------------------------------------------------------------------------------------
def test_shade_and_normal_png(cnr, tmp_path):
    from PIL import Image
    W, H = 5, 4
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = 2.0 * V.rot((0.1, 1, 0), 0.6), (1, 2, 3)                      # a similarity: the axis is normalised
    axis = T[:3, 2] / np.linalg.norm(T[:3, 2])
    side = np.cross(axis, (0, 0, 1.0))
    side /= np.linalg.norm(side)
    n = torch.zeros(W, H, 3)
    n[0, 0] = torch.from_numpy(-axis).float()                                          # faces the camera
    n[1, 0] = torch.from_numpy(axis).float()                                           # faces away
    n[2, 1] = torch.from_numpy(side).float()                                           # grazing
    n[3, 2] = torch.from_numpy((-axis + side) / np.sqrt(2)).float()
    result = dict(rgb=torch.rand(W, H, 3), depth=torch.rand(W, H), instance=torch.zeros(W, H, dtype=torch.int32), normal=n)
    img = cnr.view.shade(result, torch.from_numpy(T))
    assert img.shape == (W, H, 3) and img.dtype == torch.float32
    assert torch.equal(img[..., 0], img[..., 1]) and torch.equal(img[..., 0], img[..., 2])
    assert abs(float(img[0, 0, 0]) - 1) <= 1e-6 and float(img[1, 0, 0]) == 0 and abs(float(img[2, 1, 0])) <= 1e-6
    assert abs(float(img[3, 2, 0]) - 2 ** -0.5) <= 1e-6 and float(img[4, 3, 0]) == 0
    with pytest.raises(ValueError):
        cnr.view.shade({k: v for k, v in result.items() if k != "normal"}, T)
    cnr.view.render_to_files(result, str(tmp_path))
    png = np.asarray(Image.open(os.path.join(tmp_path, "normal.png")))
    assert png.shape == (H, W, 3) and png.dtype == np.uint8
    want = np.round((n.numpy().astype(np.float64) * 0.5 + 0.5) * 255).transpose(1, 0, 2)
    assert np.abs(png.astype(np.int64) - want.astype(np.int64)).max() <= 1            # (x.5 may round either way in float32)
    assert (png[3, 4] == 128).all()                                                   # no surface: mid grey
    plain = {k: v for k, v in result.items() if k != "normal"}
    cnr.view.render_to_files(plain, str(tmp_path / "plain"))
    assert not os.path.exists(os.path.join(tmp_path, "plain", "normal.png"))


# ---- arguments --------------------------------------------------------------------------------------------------------------------
def test_argument_errors(cnr, double):
    inp = F.category_inputs("s0")
    ok = dict(pts=inp["pts"][:8], B=inp["B"], trunk=inp["trunk"], brows=inp["brows"], row=None, scale=inp["scale"])
    s, g = cnr.ops.field_grad(**ok)
    assert s.shape == (8,) and g.shape == (8, 3)
    s, g = cnr.ops.field_grad(**dict(ok, pts=inp["pts"][:0]))                           # N = 0: empty outputs, no launch
    assert s.shape == (0,) and g.shape == (0, 3)
    bad = [dict(pts=inp["pts"][:8, :2]), dict(pts=inp["pts"][0]), dict(B=inp["B"][:20]), dict(trunk=inp["trunk"][:-1]),
           dict(brows=inp["brows"][:, :3]), dict(scale=0.0), dict(row=torch.zeros(8, dtype=torch.int64)),
           dict(row=torch.zeros(7, dtype=torch.int32)), dict(row=torch.full((8,), 4, dtype=torch.int32)),
           dict(row=torch.full((8,), -1, dtype=torch.int32))]
    for b in bad:
        with pytest.raises(ValueError):
            cnr.ops.field_grad(**dict(ok, **b))
    with pytest.raises(ValueError):
        cnr.ops.occmap_grad(None, None, torch.zeros(3))


def test_abi_and_return_codes(cnr):
    lib, fns = load_library(), declared_functions()
    for name in NEW:
        assert name in fns and hasattr(lib, name) and name in cnr._C.SIGNATURES, name
        assert_row_matches(name, cnr._C.SIGNATURES[name], fns[name])
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # host pointers: nothing may be read or launched before the arguments are refused
    for H in (0, 31, 64, 256):
        assert lib.cnr_occmap_grad(p, p, p, H, 2.0, 4, p, p, None) == -2
    assert lib.cnr_occmap_grad(p, p, p, 32, 2.0, -1, p, p, None) == -1
    assert lib.cnr_occmap_grad(None, p, p, 32, 2.0, 4, p, p, None) == -1
    assert lib.cnr_occmap_grad(p, p, p, 128, 2.0, 4, p, None, None) == -1
    assert lib.cnr_occmap_grad(p, p, p, 32, 0.0, 4, p, p, None) == -1
    assert lib.cnr_occmap_grad(None, None, None, 128, 2.0, 0, None, None, None) == 0
    assert lib.cnr_field_grad(p, None, p, p, p, 2.0, -1, p, p, None) == -1
    assert lib.cnr_field_grad(p, None, p, p, None, 2.0, 4, None, p, None) == -1
    assert lib.cnr_field_grad(None, None, None, None, None, 2.0, 0, None, None, None) == 0
    assert lib.cnr_view_surface_points(None, p, p, p, p, 0.5, p, p, p, p, p, 4, 1, p, p, p, p, p, p, p, None) == -1
    assert lib.cnr_view_surface_points(p, p, p, p, p, 0.5, p, p, p, p, p, 4, 40000, p, p, p, p, p, p, p, None) == -2
    assert lib.cnr_view_normals(p, None, p, p, 4, 4, p, None) == -1
    assert lib.cnr_view_normals(None, p, p, p, 4, 4, p, None) == -1
    assert lib.cnr_view_surface_workspace_bytes(100, 3) >= 2 * 3 * (4 + 8)
