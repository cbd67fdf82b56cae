"""CPU: the host side of the scene view renderer (cnr_amd.view) -- entity volumes against the grids Trainer.meshing builds,
the edit transforms, the C-ABI of the cnr_view_* entry points, and tests/view_cpu.py against the existing composite
restatement."""
import ctypes

import numpy as np
import pytest
import torch

import mc_cpu as M
import view_cpu as V
import view_scene as VS
from test_abi import assert_row_matches, declared_functions, load_library

NEW = ("cnr_view_segments_workspace_bytes", "cnr_view_segments_count", "cnr_view_segments_emit", "cnr_view_points",
       "cnr_view_composite")


@pytest.fixture(scope="module")
def cnr():
    import cnr_amd
    return cnr_amd


@pytest.fixture(scope="module")
def lib():
    return load_library()


@pytest.fixture(scope="module")
def scene(cnr):
    cfg = VS.small_camera(cnr.cfg.synthetic_config(device="cpu", latent_dim=32))
    cls_dict, scene_bg = VS.make_scene(cnr, cfg, seed=3)
    return cfg, cls_dict, scene_bg, cnr.view.SceneRenderer(cls_dict, scene_bg, cfg)


def _meshing_corners(cnr, sc, inst_id):
    """the eight corners of the grid Trainer.meshing evaluates for this object (trainer.py), in world coordinates (float64)"""
    t = sc.trainer
    if t.cls_id == 0 or t.n_obj == 1:
        bound = t.bound if t.cls_id == 0 else t.bound_dict[inst_id]
        scale = bound.extent / (2.0 * t.bound_extent)
        T = np.eye(4, dtype=np.float32)
        T[:3, 3], T[:3, :3] = bound.center, bound.R
        return M.grid_points(2, -1.0, 1.0, scale, T[:3]).astype(np.float64)
    extent = t.extent_dict[inst_id]
    extent = extent / np.max(extent / 2)
    g = M.grid_points(2, -1.0, 1.0, extent / (2.0 * t.bound_extent)).astype(np.float64)       # object frame
    T_obj = cnr.utils.get_transform_from_tensor_sim3(sc.object_tensor_dict[inst_id].double()).numpy()
    return g @ T_obj[:3, :3].T + T_obj[:3, 3]


def _apply(A, x):
    return x @ A[:, :3].T + A[:, 3]


def test_entity_order_and_kinds(scene):
    cfg, cls_dict, scene_bg, r = scene
    assert [e.inst_id for e in r.entities] == [0, 1, 2, 3]
    assert [e.cat for e in r.entities] == [-1, 0, 0, 1] and [e.row for e in r.entities] == [0, 0, 1, 0]
    for e in (r.entities[0], r.entities[3]):                       # world-frame fields take world points
        assert np.array_equal(e.to_field, np.eye(4)[:3])


def test_to_box_maps_the_meshing_grid_to_the_unit_box(cnr, scene):
    cfg, cls_dict, scene_bg, r = scene
    holders = {0: scene_bg, 1: cls_dict[10], 2: cls_dict[10], 3: cls_dict[30]}
    corners = M.grid_points(2).astype(np.float64)
    for e in r.entities:
        world = _meshing_corners(cnr, holders[e.inst_id], e.inst_id)
        got = _apply(e.to_box.astype(np.float32).astype(np.float64), world)
        assert np.abs(got - corners).max() <= 1e-5, (e.inst_id, np.abs(got - corners).max())
    # the several-object field frame is the object frame: to_field . T_obj = identity
    for i in (1, 2):
        T_obj = cnr.utils.get_transform_from_tensor_sim3(cls_dict[10].object_tensor_dict[i].double()).numpy()
        F = np.concatenate([r.entities[i].to_field, [[0, 0, 0, 1]]])
        assert np.abs(F @ T_obj - np.eye(4)).max() <= 1e-12


def test_transform_edit_moves_the_volume(cnr, scene):
    cfg, cls_dict, scene_bg, r = scene
    holders = {0: scene_bg, 1: cls_dict[10], 2: cls_dict[10], 3: cls_dict[30]}
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = 1.3 * V.rot((0.3, -1, 0.2), 0.8), (0.4, -0.1, 0.25)
    corners = M.grid_points(2).astype(np.float64)
    for inst_id in (0, 2, 3):
        ents = cnr.view.edited(r.entities, transforms={inst_id: E})
        assert [e.inst_id for e in ents] == [0, 1, 2, 3]
        for e, e0 in zip(ents, r.entities):
            if e.inst_id != inst_id:
                assert e is e0
                continue
            world = _apply(E[:3], _meshing_corners(cnr, holders[inst_id], inst_id))
            got = _apply(e.to_box.astype(np.float32).astype(np.float64), world)
            assert np.abs(got - corners).max() <= 1e-5
            # a moved world point reaches the field where its original did
            x = np.random.default_rng(1).normal(size=(5, 3))
            assert np.abs(_apply(e.to_field, _apply(E[:3], x)) - _apply(e0.to_field, x)).max() <= 1e-12
    assert all(e is e0 for e, e0 in zip(cnr.view.edited(r.entities), r.entities))        # no edit: the trained state as it is


def test_hidden_edit_and_unknown_ids(cnr, scene):
    r = scene[3]
    assert [e.inst_id for e in cnr.view.edited(r.entities, hidden={0, 2})] == [1, 3]
    with pytest.raises(ValueError):
        cnr.view.edited(r.entities, hidden={77})
    with pytest.raises(ValueError):
        cnr.view.edited(r.entities, transforms={77: np.eye(4)})
    twice = r.entities + [cnr.view.Entity(0, r.entities[1].to_box, r.entities[1].to_field, 0, 0)]      # an object with id 0
    with pytest.raises(ValueError, match="names 2 entities"):
        cnr.view.edited(twice, hidden={0})
    assert [e.inst_id for e in cnr.view.edited(twice, hidden={2})] == [0, 1, 3, 0]


def test_abi_checks_cover_the_view_entry_points(cnr, lib):
    fns = declared_functions()
    for name in NEW:
        assert name in fns and hasattr(lib, name) and name in cnr._C.SIGNATURES, name
        assert_row_matches(name, cnr._C.SIGNATURES[name], fns[name])
    assert cnr.view.KMAX == V.KMAX == 8 and cnr.view.SMAX == 128
    assert lib.cnr_view_segments_workspace_bytes(100, 3) >= (3 * 2) * (4 + 8) + 2 * 4


def test_shape_and_argument_errors_are_return_codes(lib):
    """host pointers: nothing may be read or launched before the shape is refused"""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for S in (0, 129):
        assert lib.cnr_view_points(p, p, p, p, p, p, 1, S, p, p, None) == -2
    assert lib.cnr_view_composite(p, p, p, p, p, p, 1, 129, 0.5, p, p, p, p, p, p, None) == -2
    assert lib.cnr_view_composite(p, p, p, p, p, p, 1, 0, 0.5, p, p, p, p, p, p, None) == -2
    assert lib.cnr_view_points(None, p, p, p, p, p, 1, 8, p, p, None) == -1
    assert lib.cnr_view_composite(None, p, p, p, p, p, 1, 8, 0.5, p, p, p, p, p, p, None) == -1
    assert lib.cnr_view_segments_count(p, p, p, 0, 1, 0.0, 8.0, p, p, p, p, None) == -1
    assert lib.cnr_view_segments_count(p, p, p, 4, 40000, 0.0, 8.0, p, p, p, p, None) == -2
    assert lib.cnr_view_segments_emit(p, p, p, 4, 0, 0.0, 8.0, p, p, p, p, p, None) == -1


def test_one_segment_composite_is_the_ray_composite():
    """tests/view_cpu.py with one segment per pixel against tests/cpu_double.py's cnr_composite_fwd, both in float64"""
    from cpu_double import Double
    g = torch.Generator().manual_seed(5)
    P, S = 7, 33
    sigma = (torch.randn(P, S, generator=g, dtype=torch.float64) * 3).numpy()
    color = torch.rand(P, S, 3, generator=g, dtype=torch.float64).numpy()
    z = np.sort(torch.rand(P, S, generator=g, dtype=torch.float64).numpy() * 4 + 0.1, axis=1)
    pix_segs = np.full((P, V.KMAX), -1, np.int32)
    pix_segs[:, 0] = np.arange(P)
    out = V.composite(sigma, color, z, pix_segs, np.zeros(P, np.int32), np.array([4], np.int32), 0.5, np.float64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    depth, var, opa, rgb = torch.zeros(P, dtype=torch.float64), torch.zeros(P, dtype=torch.float64), \
        torch.zeros(P, dtype=torch.float64), torch.zeros(P, 3, dtype=torch.float64)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        Double().cnr_composite_fwd(t(sigma), t(color), t(z), None, depth, var, rgb, opa, P, S, 0)
    finally:
        torch.set_default_dtype(old)
    for name, ref in (("depth", depth), ("var", var), ("opacity", opa), ("rgb", rgb)):
        assert np.abs(out[name] - ref.numpy()).max() <= 1e-14, name
    assert np.abs(out["mass"][:, 0] - opa.numpy()).max() <= 1e-14 and not out["mass"][:, 1:].any()
    assert np.array_equal(out["instance"], np.where(opa.numpy() >= 0.5, 4, -1))


def test_restated_segments_match_the_recorded_scenes():
    """the hit counts of the two box scenes, identical in both precisions (the GPU test compares the kernels against these)"""
    for (T, d, A), hits, empty in ((VS.scene_a(), [432, 108, 76, 0, 4], 0), (VS.scene_a(False), [108, 76, 0, 4], 305),
                                   (VS.scene_b(), [63, 19, 432], 0)):
        A32, T32 = A.astype(np.float32), T.astype(np.float32)
        s64 = V.segments(T32, d, A32, VS.ZMIN, VS.ZMAX, np.float64)
        s32 = V.segments(T32, d, A32, VS.ZMIN, VS.ZMAX, np.float32)
        assert s64["hit"].sum(1).tolist() == hits and np.array_equal(s64["hit"], s32["hit"])
        assert int((s64["hit"].sum(0) == 0).sum()) == empty
        assert np.abs(s64["seg_z"] - s32["seg_z"]).max() < 1e-6
    T, d, A = VS.scene_b()
    zero = (d == 0).any(1)
    assert int(zero.sum()) == 41
    assert (V.segments(T, d, A, VS.ZMIN, VS.ZMAX, np.float64)["hit"] & zero[None]).sum(1).tolist() == [15, 3, 41]
    T, d, A = VS.scene_nested()
    s = V.segments(T, d, A, VS.ZMIN, VS.ZMAX, np.float64)
    assert s["overflow"] > 0 and s["overflow"] == int((s["hit"].sum(0) > V.KMAX).sum())
