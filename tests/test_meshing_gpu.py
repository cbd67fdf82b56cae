"""GPU: cnr_mc_* against the numpy restatement (tests/mc_cpu.py), cnr_grid_points against make_3D_grid's torch form, and
Trainer.meshing on trained CodeNeRF objects against a CPU path (oracle forward -> mc_cpu -> the same transforms), plus
train.py's meshing block (:214-243) on sceneCategory objects."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mc_cpu as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cnr():
    import cnr_amd
    return cnr_amd


def _gpu_mc(cnr, vol, dev, level=0.5, ascent=True):
    out = cnr.vis.marching_cubes_raw(torch.from_numpy(np.ascontiguousarray(vol, np.float32)).to(dev), level, ascent)
    return None if out is None else tuple(t.cpu().numpy() for t in out)


def _compare(got, ref):
    (v, n, f), (rv, rn, rf) = got, ref
    assert np.array_equal(f, rf)
    np.testing.assert_allclose(v, rv, rtol=0, atol=2e-6)
    np.testing.assert_allclose(n, rn, rtol=0, atol=2e-6)


VOLUMES = [("sphere17", lambda: M.sphere(17, 0.85)), ("sphere64", lambda: M.sphere(64, 0.85)),
           ("sphere129", lambda: M.sphere(129, 0.85)), ("torus", lambda: M.torus(48)), ("two", lambda: M.two_spheres(48)),
           ("cut", lambda: M.sphere(33, 0.6, 6.0, (1.0, 0.0, 0.0)))] + \
          [("binary%d" % s, (lambda s=s: M.random_binary(16, s))) for s in range(20)]


@pytest.mark.parametrize("name,make", VOLUMES, ids=[v[0] for v in VOLUMES])
def test_mc_matches_the_restatement(cnr, dev, name, make):
    vol = make()
    for ascent in (True, False):
        got = _gpu_mc(cnr, vol, dev, ascent=ascent)
        _compare(got, M.marching_cubes(vol, ascent=ascent))
        again = _gpu_mc(cnr, vol, dev, ascent=ascent)
        assert all(np.array_equal(a, b) for a, b in zip(got, again))


def test_mc_edge_cases(cnr, dev):
    assert _gpu_mc(cnr, np.full((9, 9, 9), 0.3, np.float32), dev) is None
    vol = np.full((4, 4, 4), 0.5, np.float32)
    assert _gpu_mc(cnr, vol, dev) is None
    vol[1, 1, 1], vol[2, 2, 2] = 0.9, np.nan
    _compare(_gpu_mc(cnr, vol, dev), M.marching_cubes(vol))
    one = np.zeros((2, 2, 2), np.float32)
    one[0, 0, 0] = 1.0
    v, n, f = _gpu_mc(cnr, one, dev)
    assert v.shape == (3, 3) and f.shape == (1, 3)
    _compare((v, n, f), M.marching_cubes(one))
    for D in (1, 513):
        with pytest.raises(cnr._C.CnrError):
            cnr.vis.marching_cubes_raw(torch.zeros(D, D, D, device=dev))


def test_mc_256_sphere(cnr, dev):
    vol = M.sphere(256, 0.85)
    _compare(_gpu_mc(cnr, vol, dev), M.marching_cubes(vol))


@pytest.mark.parametrize("D", [511, 512])
def test_mc_largest_grids(cnr, dev, D):
    x = torch.linspace(-1, 1, D, device=dev)
    X, Y, Z = torch.meshgrid(x, x, x, indexing="ij")
    vol = torch.sigmoid(4 * (0.85 - torch.sqrt(X * X + Y * Y + Z * Z))).contiguous()
    del X, Y, Z
    v, n, f = cnr.vis.marching_cubes_raw(vol)
    assert int(f.max()) == v.shape[0] - 1 and int(f.min()) == 0
    ff = f.cpu().numpy()
    _, cnt, _, dup = M.edge_stats(ff)
    assert set(cnt.tolist()) == {2} and not dup
    r = (v * 2 - 1).norm(dim=1)
    assert float((r - 0.85).abs().max()) < 2.0 / (D - 1)


def _torch_grid(occ_range, dim, device, transform=None, scale=None):
    """src/render_rays.py:97-121 restated"""
    t = torch.linspace(occ_range[0], occ_range[1], steps=dim, device=device)
    grid = torch.meshgrid(t, t, t, indexing="ij")
    g = torch.cat((grid[0][..., None], grid[1][..., None], grid[2][..., None]), dim=3)
    if scale is not None:
        g = g * scale
    if transform is not None:
        rows = [(transform[None, None, None, k, :3] * g).sum(-1, keepdim=True) for k in range(3)]
        g = torch.cat(rows, dim=-1) + transform[None, None, None, :3, 3]
    return g


def _ulp_close(a, b, ulps=2):
    a, b = a.double(), b.double()
    tol = ulps * torch.finfo(torch.float32).eps * torch.maximum(a.abs(), b.abs()).clamp_min(1e-30)
    return bool(((a - b).abs() <= tol + 1e-30).all())


@pytest.mark.parametrize("D", [2, 63, 256])
def test_make_3D_grid(cnr, dev, D):
    g = torch.Generator().manual_seed(D)
    scale = (torch.rand(3, generator=g) + 0.5).to(dev)
    T = torch.eye(4)
    T[:3, :3] = torch.linalg.qr(torch.randn(3, 3, generator=g))[0]
    T[:3, 3] = torch.randn(3, generator=g)
    T = T.to(dev)
    for kw in (dict(), dict(scale=scale), dict(transform=T), dict(scale=scale, transform=T)):
        got = cnr.render_rays.make_3D_grid([-1.0, 1.0], D, dev, **kw)
        ref = _torch_grid([-1.0, 1.0], D, dev, **kw)
        assert got.shape == ref.shape
        if "transform" in kw:   # sums of three products: 2 ulp of the largest term
            mag = _torch_grid([-1.0, 1.0], D, dev, scale=kw.get("scale")).abs().amax(-1, keepdim=True) + T[:3, 3].abs()
            assert float(((got - ref).abs() / mag).max()) <= 4 * torch.finfo(torch.float32).eps
        else:
            assert _ulp_close(got, ref)


# ---- Trainer.meshing on trained objects -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(cnr, dev):
    from scene_synth import analytic_pool
    torch.manual_seed(99)
    n_obj, R, n1, n2, L = 4, 512, 4, 28, 32
    cfg = cnr.cfg.synthetic_config(device=str(dev), latent_dim=L, n_bins_cam2surface=n1, n_bins=n2)
    gen = torch.Generator().manual_seed(11)
    tr = cnr.fused.FusedCategoryTrainer(cfg, 1, n_obj, [analytic_pool(64 * R, n_obj, gen)], R, dev, seed=7, generator=gen)
    tr.run(400)
    torch.cuda.synchronize()
    return cfg, tr.state_dicts(0), n_obj


def _load(cnr, cfg, sd, ids, rows):
    t = cnr.trainer.Trainer(cfg, 3, ids)
    with torch.no_grad():
        t.fc_occ_map.load_state_dict({k: v.to(cfg.training_device) for k, v in sd["FC_state_dict"].items()})
        t.pe.B_layer.weight.copy_(sd["PE_state_dict"]["B_layer.weight"])
        t.shape_codes.weight.copy_(sd["shape_code_state_dict"]["weight"][rows])
        t.texture_codes.weight.copy_(sd["texture_code_state_dict"]["weight"][rows])
    return t


def _cpu_mesh(cnr, cfg, sd, row, D, scale_np, transform_np=None):
    from oracle import ref_cpu as O
    grid = M.grid_points(D, -1.0, 1.0, scale_np, None if transform_np is None else transform_np[:3])
    p = {k: v.detach().cpu()[None] for k, v in sd["FC_state_dict"].items()}
    B = sd["PE_state_dict"]["B_layer.weight"].detach().cpu()[None]
    cs = sd["shape_code_state_dict"]["weight"][row].detach().cpu().view(1, 1, 1, -1)
    ct = sd["texture_code_state_dict"]["weight"][row].detach().cpu().view(1, 1, 1, -1)
    occ = []
    with torch.no_grad():
        for k in range(0, len(grid), 1 << 18):
            x = torch.from_numpy(grid[k:k + (1 << 18)])[None, None]
            s, _ = O.codenerf_forward(p, O.unidirs_embed(x, B, cfg.obj_scale), cs, ct)
            occ.append(torch.sigmoid(s.reshape(-1)))
    v, n, f = M.marching_cubes(torch.cat(occ).view(D, D, D).numpy())
    m = cnr.vis.Mesh(v, f, n)
    m.apply_translation([-0.5, -0.5, -0.5])
    m.apply_scale(2)
    m.apply_scale(scale_np)
    if transform_np is not None:
        m.apply_transform(transform_np)
    return m


def _chamfer(a, b):
    from scipy.spatial import cKDTree
    return 0.5 * (cKDTree(b).query(a)[0].mean() + cKDTree(a).query(b)[0].mean())


def _check(cnr, t, mesh, ref, inst_id, extent, center, radius):
    assert abs(len(mesh.vertices) - len(ref.vertices)) <= 0.005 * len(ref.vertices)
    assert _chamfer(mesh.vertices, ref.vertices) <= 1e-3 * float(np.max(extent))
    _, col = t.eval_points(torch.from_numpy(mesh.vertices).float().to(t.device), inst_id=inst_id)
    assert np.array_equal(mesh.visual.vertex_colors[:, :3], (col * 255).cpu().numpy().astype(np.uint8))
    r = np.linalg.norm(mesh.vertices - center, axis=1).mean()
    assert abs(r - radius) < 0.25 * radius, (r, radius)


@pytest.mark.parametrize("D", [64, 128])
def test_meshing_multi_object_category(cnr, dev, trained, D):
    from scene_synth import sphere_radius
    cfg, sd, n_obj = trained
    ids = [10 + k for k in range(n_obj)]
    t = _load(cnr, cfg, sd, ids, list(range(n_obj)))
    t.extent_dict = {10 + k: np.full(3, 2.4 * sphere_radius(k)) for k in range(n_obj)}
    for k in (0, 3):
        mesh = t.meshing(10 + k, grid_dim=D)
        ext = t.extent_dict[10 + k]
        scale_np = (ext / np.max(ext / 2)) / (2.0 * 0.9)
        ref = _cpu_mesh(cnr, cfg, sd, k, D, scale_np)
        _check(cnr, t, mesh, ref, 10 + k, 2 * scale_np, np.zeros(3), sphere_radius(k))


@pytest.mark.parametrize("D", [64, 128])
def test_meshing_single_object_category(cnr, dev, trained, D):
    from scene_synth import sphere_radius
    cfg, sd, _ = trained
    t = _load(cnr, cfg, sd, [7], [1])
    Rm = np.linalg.qr(np.random.default_rng(3).normal(size=(3, 3)))[0].astype(np.float32)
    Rm *= np.sign(np.linalg.det(Rm))
    # (the trained field is a sphere about the origin of the frame it is evaluated in: a box around it, rotated)
    bound = SimpleNamespace(extent=np.full(3, 2.0 * sphere_radius(1) * 1.3), center=np.array([0.03, -0.02, 0.01]), R=Rm)
    t.bound_dict = {7: bound}
    mesh = t.meshing(7, grid_dim=D)
    scale_np = bound.extent / (2.0 * 0.9)
    T = np.eye(4, dtype=np.float32)
    T[:3, 3], T[:3, :3] = bound.center, bound.R
    ref = _cpu_mesh(cnr, cfg, sd, 1, D, scale_np, T)
    _check(cnr, t, mesh, ref, 7, bound.extent, bound.center, sphere_radius(1))


def test_meshing_background_is_the_pipeline(cnr, dev):
    """Background: eval_points (default exact fp32) on make_3D_grid, GPU marching cubes, the same transforms; the output is
    the composition of the parts, and every vertex colour is eval_points' colour at that vertex."""
    cfg = cnr.cfg.synthetic_config(device=str(dev), latent_dim=32)
    torch.manual_seed(4)
    t = cnr.trainer.Trainer(cfg, 0, [0])
    t.bound = SimpleNamespace(extent=np.array([4.0, 3.0, 2.5]), center=np.array([0.5, 0.0, 1.0]), R=np.eye(3, dtype=np.float32))
    D = 48
    mesh = t.meshing(grid_dim=D)
    scale_np = t.bound.extent / (2.0 * 0.995)
    T = np.eye(4, dtype=np.float32)
    T[:3, 3], T[:3, :3] = t.bound.center, t.bound.R
    grid = cnr.render_rays.make_3D_grid([-1.0, 1.0], D, dev, transform=torch.from_numpy(T).to(dev),
                                        scale=torch.from_numpy(scale_np).float().to(dev)).view(-1, 3)
    occ, _ = t.eval_points(grid)
    ref = cnr.vis.marching_cubes(occ.view(D, D, D))
    if ref is None:
        assert mesh is None
        return
    ref.apply_translation([-0.5, -0.5, -0.5])
    ref.apply_scale(2)
    ref.apply_scale(scale_np)
    ref.apply_transform(T)
    assert np.array_equal(mesh.vertices, ref.vertices) and np.array_equal(mesh.faces, ref.faces)
    _, col = t.eval_points(torch.from_numpy(mesh.vertices).float().to(dev))
    assert np.array_equal(mesh.visual.vertex_colors[:, :3], (col * 255).cpu().numpy().astype(np.uint8))


def test_reference_meshing_loop(cnr, dev, tmp_path):
    """train.py:214-243 restated on the categories test_dropin_gpu builds (train.py:33-64)."""
    from test_dropin_gpu import _scene
    cfg, cls_dict, scene_bg = _scene(cnr, dev)
    cfg.grid_dim, cfg.live_voxel_size = 32, 0.005
    scene_bg.trainer.bound.center, scene_bg.trainer.bound.R = np.zeros(3), np.eye(3, dtype=np.float32)
    for sc in cls_dict.values():
        for b in (getattr(sc.trainer, "bound_dict", None) or {}).values():
            b.center, b.R = np.zeros(3), np.eye(3, dtype=np.float32)
    vis_dict = dict(cls_dict)
    vis_dict[0] = scene_bg
    out, iteration, written = str(tmp_path), 10000, []
    for cls_id, cls_k in vis_dict.items():
        if cls_id == 0:
            bound = cls_k.trainer.bound
            adaptive_grid_dim = int(np.minimum(np.max(bound.extent) // cfg.live_voxel_size + 1, cfg.grid_dim))
            mesh = scene_bg.trainer.meshing(grid_dim=adaptive_grid_dim)
            assert mesh is not None
            p = os.path.join(out, "iteration_{}_obj{}.obj".format(iteration, str(0)))
            mesh.export(p)
            written.append(p)
        else:
            for obj_id in cls_k.obj_ids:
                if len(cls_k.obj_ids) > 1:
                    extent = cls_k.trainer.extent_dict[obj_id]
                else:
                    extent = cls_k.trainer.bound_dict[obj_id].extent
                adaptive_grid_dim = int(np.minimum(np.max(extent) // cfg.live_voxel_size + 1, cfg.grid_dim))
                obj_tensor = cls_k.object_tensor_dict[obj_id]
                mesh = cls_k.trainer.meshing(obj_id, grid_dim=adaptive_grid_dim)
                scale_np = obj_tensor[0].detach().cpu().numpy()
                transform_np = cnr.utils.get_transform_from_tensor(obj_tensor[1:]).detach().cpu().numpy()
                if mesh is None:
                    print("mesh failed obj ", obj_id)
                else:
                    if len(cls_k.obj_ids) > 1:
                        mesh.apply_scale(scale_np)
                        mesh.apply_transform(transform_np)
                    p = os.path.join(out, "iteration_{}_obj{}.obj".format(iteration, str(obj_id)))
                    mesh.export(p)
                    written.append(p)
    assert len(written) >= 2
    for p in written:
        v, c, n, f = cnr.vis.load_obj(p)
        assert len(v) > 0 and len(f) > 0 and f.max() < len(v) and len(n) == len(v)
