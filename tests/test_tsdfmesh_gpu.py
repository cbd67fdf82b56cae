"""GPU: csrc/tsdf_mesh.hip through utils.TSDFVolume.extract_triangle_mesh_raw, accumulate_mesh_tsdf and tools/tsdf_mesh.py
 against the numpy restatement tests/tsdfmesh_cpu.py.  Both sides run the same separately rounded IEEE
operations, so every comparison is np.array_equal."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import tsdf_cpu as TC
import tsdfmesh_cpu as TM
from conftest import ROOT
from test_dataset_gpu import _tree_with_cache
from test_dataset_host import DS
from test_tsdf_gpu import K, TRUNC, VOXEL, restated_cloud, run_both, slanted_case
from test_tsdfmesh_host import UNIT_SETS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cnr():
    import cnr_amd
    return cnr_amd


def np_(t):
    return t.cpu().numpy()


def check_mesh(vol, want):
    """the volume's raw mesh equals the restatement's, bit for bit -> (V, F)"""
    got = vol.extract_triangle_mesh_raw()
    if want is None:
        assert got is None
        return 0, 0
    assert got is not None
    assert (len(got[0]), len(got[3])) == (len(want[0]), len(want[3]))
    assert got[3].dtype == torch.int32 and all(g.dtype == torch.float64 for g in got[:3])
    for name, g, w in zip(("verts", "colors", "normals", "faces"), got, want):
        assert np.array_equal(np_(g), w), name
    return len(want[0]), len(want[3])


def from_blocks(cnr, dev, blocks):
    return cnr.utils.TSDFVolume.from_blocks(*[torch.from_numpy(np.asarray(b)) for b in blocks], VOXEL, TRUNC, device=dev)


def test_slanted_plane_crosses_faces_edges_and_corners_gpu(cnr, dev):
    want, vol = run_both(cnr, dev, *slanted_case())
    mesh, parts = TM.mesh(want["units"], want["tsdf"], want["weight"], want["color"], VOXEL, parts=True)
    assert {2, 4, 8} <= set(TM.cell_unit_counts(parts).tolist())
    assert (want["weight"] == 0).any() and len(want["units"]) > 8
    V, F = check_mesh(vol, mesh)
    assert V > 1000 and F > 1000
    hood = np_(cnr.utils.tsdf_unit_neighbourhood(vol.units))
    assert np.array_equal(hood, TM.neighbourhood_brute(want["units"])) and np.array_equal(hood[:, [22, 16, 14]], want["neighbours"])


def test_sphere_blocks_and_the_mesh_consumers_gpu(cnr, dev):
    blocks = TM.sphere_blocks(VOXEL)
    vol = from_blocks(cnr, dev, blocks)
    assert np.array_equal(np_(vol.neighbours), TM.neighbourhood_brute(blocks[0])[:, [22, 16, 14]])
    want = TM.mesh(*blocks, VOXEL)
    check_mesh(vol, want)
    mesh = vol.extract_triangle_mesh()
    assert isinstance(mesh, cnr.vis.Mesh) and mesh.vertices.dtype == np.float64 and mesh.faces.shape == (len(want[3]), 3)
    assert np.array_equal(mesh.vertices, want[0]) and np.array_equal(mesh.vertex_normals, want[2])
    assert np.array_equal(mesh.visual.vertex_colors[:, :3], np.clip(np.rint(255.0 * want[1]), 0, 255).astype(np.uint8))
    from cnr_amd import raster
    rast = raster.MeshRasterizer.from_intrinsics(32, 24, 32.0, 32.0, 15.5, 11.5, 0.05, 5.0, device=dev)
    res = rast.render(raster.MeshScene(mesh, device=dev), TC.look_at((0.0, -0.5, 0.0), (0.0, 0.0, 0.0)))
    depth = np_(res["depth"])
    assert depth.shape == (32, 24) and np.isfinite(depth[16, 12]) and abs(depth[16, 12] - 0.4) < 0.01       # 0.5 m - the 0.1 m radius


def test_random_blocks_reach_every_case_gpu(cnr, dev):
    blocks = TM.random_blocks(UNIT_SETS["cube"], 7)
    want, parts = TM.mesh(*blocks, VOXEL, parts=True)
    assert (blocks[2] == 0).mean() > 0.05
    valid_cases = parts["case"][parts["valid"][:, 1:, 1:, 1:]]
    assert len(np.unique(valid_cases)) == 256
    assert set(TM.cell_unit_counts(parts).tolist()) == {1, 2, 4, 8}
    check_mesh(from_blocks(cnr, dev, blocks), want)


@pytest.mark.parametrize("which", ["no_plus_x", "diagonal"])
def test_missing_units_gpu(cnr, dev, which):
    blocks = TM.random_blocks(UNIT_SETS["no_plus_x"], 11)
    if which == "diagonal":
        ijk = TC.unpack(blocks[0]).reshape(-1, 3)
        keep = [int(np.flatnonzero((ijk == np.array(v)).all(1))[0]) for v in ((0, 0, 0), (1, 1, 0))]
        blocks = tuple(b[keep] for b in blocks)
    V, F = check_mesh(from_blocks(cnr, dev, blocks), TM.mesh(*blocks, VOXEL))
    assert V > 1000 and F > 1000


def test_edge_cases_gpu(cnr, dev):
    units, tsdf, weight, color = TM.random_blocks([(0, 0, 0)], 2)
    assert check_mesh(from_blocks(cnr, dev, (units, tsdf, np.zeros_like(weight), color)), None) == (0, 0)
    flat = np.abs(tsdf) + np.float32(0.01)
    assert TM.mesh(units, flat, weight, color, VOXEL) is None
    vol = from_blocks(cnr, dev, (units, flat, weight, color))
    assert vol.extract_triangle_mesh_raw() is None and vol.extract_triangle_mesh() is None
    blocks = TM.random_blocks(UNIT_SETS["cube"], 9)
    vol = from_blocks(cnr, dev, blocks)
    before = [np_(a) for a in vol.extract_points()]
    a, b = vol.extract_triangle_mesh_raw(), vol.extract_triangle_mesh_raw()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    after = [np_(x) for x in vol.extract_points()]
    assert len(before[0]) > 1000 and all(np.array_equal(x, y) for x, y in zip(before, after))
    want_p, want_c = TC.extract(blocks[0], TM.neighbourhood_brute(blocks[0])[:, [22, 16, 14]], *blocks[1:], VOXEL)
    assert np.array_equal(after[0], want_p) and np.array_equal(after[1], want_c)
    with pytest.raises(ValueError, match="ascending"):
        from_blocks(cnr, dev, tuple(b[::-1].copy() for b in blocks))
    with pytest.raises(ValueError, match="shapes"):
        from_blocks(cnr, dev, (blocks[0], blocks[1][:, :100], blocks[2], blocks[3]))


# ---- the ScanNet fixture -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scannet(cnr, dev, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("scannet_mesh")
    root = _tree_with_cache(tmp, "scannet_refined")
    with open(os.path.join(DS, "scannet_refined.json")) as f:
        c = json.load(f)
    c["dataset"]["path"] = root
    cfg_file = str(tmp / "cfg.json")
    with open(cfg_file, "w") as f:
        json.dump(c, f)
    cfg = cnr.cfg.Config(cfg_file)
    return cfg, cfg_file, cnr.dataset.get_dataset(cfg), tmp


def restated_mesh(inst_id, frame_info, samples, Kc, depth_scale, max_depth):
    frames = [samples[fi["frame"]] for fi in frame_info]
    depths = np.stack([TC.depth_image(s["depth"], s["obj_mask"], inst_id, depth_scale, max_depth) for s in frames])
    r = TC.fuse(depths, np.stack([s["image"] for s in frames]), np.stack([s["T"] for s in frames]), Kc, 0.01, 0.04)
    return TM.mesh(r["units"], r["tsdf"], r["weight"], r["color"], 0.01), len(r["units"])


def test_accumulate_mesh_tsdf_on_the_scannet_fixture_gpu(cnr, dev, scannet):
    cfg, _, ds, _ = scannet
    Kc = (cfg.fx, cfg.fy, cfg.cx, cfg.cy)
    info = ds.inst_dict[0]["frame_info"]
    want, n_units = restated_mesh(0, info, ds.sample_dict, Kc, cfg.depth_scale, cfg.max_depth)
    assert want is not None and len(want[0]) > 1000
    cloud_before = cnr.utils.accumulate_pointcloud_tsdf(0, info, ds.sample_dict, ds.intrinsic_open3d, depth_scale=cfg.depth_scale,
                                                        max_depth=cfg.max_depth, device=dev)
    mesh = cnr.utils.accumulate_mesh_tsdf(0, info, ds.sample_dict, ds.intrinsic_open3d, depth_scale=cfg.depth_scale,
                                          max_depth=cfg.max_depth, device=dev)
    assert mesh.units == n_units
    assert np.array_equal(mesh.vertices, want[0]) and np.array_equal(mesh.vertex_normals, want[2]) and np.array_equal(mesh.faces, want[3])
    assert np.array_equal(mesh.visual.vertex_colors[:, :3], np.clip(np.rint(255.0 * want[1]), 0, 255).astype(np.uint8))
    cloud_want, _ = restated_cloud(0, info, ds.sample_dict, Kc, cfg.depth_scale, cfg.max_depth)
    cloud_after = cnr.utils.accumulate_pointcloud_tsdf(0, info, ds.sample_dict, ds.intrinsic_open3d, depth_scale=cfg.depth_scale,
                                                       max_depth=cfg.max_depth, device=dev)
    assert np.array_equal(np_(cloud_before.points_device), cloud_want) and np.array_equal(np_(cloud_after.points_device), cloud_want)


def _tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tsdf_mesh_tool_writes_what_the_evaluation_reads_gpu(cnr, dev, scannet, capsys):
    cfg, cfg_file, ds, tmp = scannet
    Kc = (cfg.fx, cfg.fy, cfg.cx, cfg.cy)
    tool = _tool("tsdf_mesh")
    ids = tool.instances(ds.inst_dict)
    obj = sorted(i for i in ids if i != 0)[0]
    out = str(tmp / "scene_mesh")
    with torch.cuda.device(dev):
        tool.main(["--config", cfg_file, "--out", out, "--inst", "0", str(obj), "--iteration", "7"])
    rows = [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith("{")]
    assert [r["obj"] for r in rows] == [0, obj]
    for r in rows:
        want, n_units = restated_mesh(r["obj"], ids[r["obj"]], ds.sample_dict, Kc, cfg.depth_scale, cfg.max_depth)
        assert (r["V"], r["F"], r["units"]) == (len(want[0]), len(want[3]), n_units) and r["seconds"] >= 0
        back = cnr.vis.load_mesh(os.path.join(out, "iteration_7_obj%d.obj" % r["obj"]))
        assert (len(back.vertices), len(back.faces)) == (r["V"], r["F"])
        assert np.abs(back.vertices - want[0]).max() < 1e-7 and np.array_equal(back.faces, want[3])
    assert _tool("eval_3d_obj").get_obj_ids(out, 7) == [obj]
