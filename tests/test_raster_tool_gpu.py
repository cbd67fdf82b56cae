"""GPU: tools/render_mesh.py on a mesh written by Mesh.export: the five PNGs at the requested size, and the depth image is the
rasteriser's."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import ROOT
import raster_cpu as RC
from test_dataset_gpu import DS, _tree_with_cache

pytestmark = pytest.mark.gpu


def _tool():
    spec = importlib.util.spec_from_file_location("render_mesh_tool", os.path.join(ROOT, "tools", "render_mesh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_render_mesh_tool(dev, tmp_path, monkeypatch):
    from cnr_amd import raster, vis
    with torch.cuda.device(dev):
        mesh = vis.marching_cubes(RC.sphere_volume(24, 0.3))
    mesh.visual.vertex_colors = np.round(mesh.vertices * 255)
    path = mesh.export(str(tmp_path / "ball.obj"))
    out = tmp_path / "out"
    tool = _tool()
    monkeypatch.setattr(sys, "argv", ["render_mesh.py", "--mesh", path, "--look-at", "2.0", "1.5", "1.2", "0.5", "0.5", "0.5",
                                      "--intrinsics", "72", "48", "80", "80", "35.5", "23.5", "--depth-range", "0.1", "10",
                                      "--out", str(out)])
    tool.main()
    for name in ("rgb.png", "depth.png", "instance.png", "normal.png", "shade.png"):
        assert Image.open(os.path.join(str(out), name)).size == (72, 48), name
    rast = raster.MeshRasterizer.from_intrinsics(72, 48, 80.0, 80.0, 35.5, 23.5, 0.1, 10.0, device=dev)
    res = rast.render(raster.MeshScene(tool.load(path), device=dev), tool.look_at([2.0, 1.5, 1.2], [0.5, 0.5, 0.5]))
    depth = res["depth"].cpu().numpy()
    assert (depth > 0).sum() > 200
    assert (np.asarray(Image.open(os.path.join(str(out), "depth.png"))).T == np.round(depth.astype(np.float64) * 1000)).all()
    inst = np.asarray(Image.open(os.path.join(str(out), "instance.png"))).T
    assert ((inst == 0) == (depth > 0)).all() and ((inst == 65535) == (depth == 0)).all()
    rgb = np.asarray(Image.open(os.path.join(str(out), "rgb.png")))
    assert rgb[depth.T > 0].std() > 5 and (rgb[depth.T == 0] == 0).all()      # the exported colours came back


def test_render_mesh_tool_takes_pose_and_intrinsics_from_a_dataset(dev, tmp_path, monkeypatch):
    """--config CFG --frame K on the committed Replica tree: the camera of the config, the pose of frame K"""
    import cnr_amd as cnr
    from cnr_amd import raster, vis
    root = _tree_with_cache(tmp_path, "replica")
    with open(os.path.join(DS, "replica.json")) as f:
        c = json.load(f)
    c["dataset"]["path"] = root
    c["camera"].update(w=72, h=48, fx=60.0, fy=60.0, cx=35.5, cy=23.5)
    cfg_file = tmp_path / "cfg.json"
    cfg_file.write_text(json.dumps(c))
    cfg = cnr.cfg.Config(str(cfg_file))
    T_wc = np.asarray(cnr.dataset.get_dataset(cfg).sample_dict[1]["T"], np.float64)
    # a one-metre square one metre before that camera, facing it
    corners = np.array([[-0.5, -0.5, 1.0], [0.5, -0.5, 1.0], [0.5, 0.5, 1.0], [-0.5, 0.5, 1.0]]) @ T_wc[:3, :3].T + T_wc[:3, 3]
    path = vis.Mesh(corners, [[0, 1, 2], [0, 2, 3]]).export(str(tmp_path / "plate.obj"))
    out = tmp_path / "out"
    monkeypatch.setattr(sys, "argv", ["render_mesh.py", "--mesh", path, "--config", str(cfg_file), "--frame", "1", "--out", str(out)])
    _tool().main()
    mm = np.asarray(Image.open(os.path.join(str(out), "depth.png")))
    assert mm.shape == (48, 72)
    rast = raster.MeshRasterizer(cfg)
    res = rast.render(raster.MeshScene(_tool().load(path), device=rast.device), T_wc, attributes=False)
    assert (mm.T == np.round(res["depth"].cpu().numpy().astype(np.float64) * 1000)).all()
    assert abs(int(mm[24, 36]) - 1000) <= 1 and (mm > 0).sum() > 1000          # 60 px per metre at one metre: 60 x 48 of it in view
