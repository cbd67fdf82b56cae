"""GPU: tools/render_view.py on the committed Replica tree -- the scene built as train.py builds it, the NEWEST checkpoints
loaded, a dataset pose rendered and written -- against SceneRenderer on the objects that wrote those checkpoints."""
import importlib.util
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import ROOT
from test_dataset_gpu import DS, _tree_with_cache

pytestmark = pytest.mark.gpu


def _tool():
    spec = importlib.util.spec_from_file_location("render_view_tool", os.path.join(ROOT, "tools", "render_view.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _png(d, name):
    return np.asarray(Image.open(os.path.join(d, name)))


def test_render_view_tool(dev, tmp_path, monkeypatch):
    import cnr_amd as cnr
    from cnr_amd.scene_cateogries import cameraInfo, sceneCategory
    root = _tree_with_cache(tmp_path, "replica")
    with open(os.path.join(DS, "replica.json")) as f:
        c = json.load(f)
    c["dataset"]["path"] = root
    c["camera"].update(w=72, h=48, fx=60.0, fy=60.0, cx=35.5, cy=23.5)
    c["model"]["net_hyperparams"]["latent_dim"] = 32
    cfg_file = tmp_path / "cfg.json"
    cfg_file.write_text(json.dumps(c))
    cfg = cnr.cfg.Config(str(cfg_file))
    data = cnr.dataset.get_dataset(cfg)
    rays = cameraInfo(cfg).rays_dir_cache
    np.random.seed(0)
    torch.manual_seed(0)
    cls_dict, scene_bg = {}, None
    logdir = tmp_path / "logs"
    logdir.mkdir()
    for cls_id in data.inst_dict.keys():
        sc = sceneCategory(cfg, cls_id, data.inst_dict[cls_id], data.sample_dict, rays)
        if cls_id == 0:
            b = sc.trainer.bound                                     # a plain object, so that the file unpickles anywhere
            sc.trainer.bound = SimpleNamespace(extent=np.asarray(b.extent), center=np.asarray(b.center), R=np.asarray(b.R))
            scene_bg = sc
        else:
            cls_dict[cls_id] = sc
        sc.save_checkpoints(str(logdir), 3)                          # an older checkpoint with other weights ...
        with torch.no_grad():
            for p in sc.trainer.fc_occ_map.parameters():
                p.add_(0.05 * torch.randn_like(p))
        sc.save_checkpoints(str(logdir), 20)                         # ... and the newest, which the tool must take
    frame = 1
    T_wc = np.asarray(data.sample_dict[frame]["T"], np.float64)
    renderer = cnr.view.SceneRenderer(cls_dict, scene_bg, cfg)
    inst_all = [e.inst_id for e in renderer.entities]
    once = [i for i in inst_all if inst_all.count(i) == 1 and i != 0]      # (this tree has an object with the background's id 0)
    moved, hidden = once[0], once[-1]
    assert moved != hidden
    E = np.eye(4)
    E[:3, 3] = 0.2, -0.1, 0.05
    tool = _tool()
    for name, extra, kw in (("plain", [], {}),
                            ("edited", ["--move", str(moved), "0.2", "-0.1", "0.05", "--hide", str(hidden)],
                             dict(transforms={moved: E}, hidden={hidden}))):
        out, ref = tmp_path / ("out_" + name), tmp_path / ("ref_" + name)
        monkeypatch.setattr(sys, "argv", ["render_view.py", "--config", str(cfg_file), "--logdir", str(logdir), "--frame", str(frame),
                                          "--out", str(out), "--samples", "16", "--allow-pickle"] + extra)
        tool.main()
        with torch.no_grad():
            res = renderer.render(T_wc, n_samples=16, **kw)
        cnr.view.render_to_files(res, str(ref))
        for png in ("rgb.png", "depth.png", "instance.png"):
            a, b = _png(out, png), _png(ref, png)
            assert a.shape[:2] == (cfg.H, cfg.W) and np.array_equal(a, b), (name, png)
        if name == "edited":
            assert hidden not in np.unique(_png(out, "instance.png"))
    assert tool.newest_checkpoint(str(logdir), 0).endswith("cls_0_iteration_00020.pth")
