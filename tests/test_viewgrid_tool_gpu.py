"""GPU: tools/render_view.py --skip-empty on the committed Replica tree (the scene of tests/test_view_tool_gpu.py, built as
train.py builds it, from real sceneCategory objects): the tool builds the occupancy grids from the loaded checkpoints and
renders with them; against build_grids + render(skip_empty=True) on the objects that wrote those checkpoints."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_dataset_gpu import DS, _tree_with_cache
from test_view_tool_gpu import _png, _tool

pytestmark = pytest.mark.gpu


def test_render_view_tool_skips_empty_space(dev, tmp_path, monkeypatch, capsys):
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
        sc.save_checkpoints(str(logdir), 20)
    frame, G, tau = 1, 8, 0.5                  # random weights: occupancies lie around 0.5, so tau = 0.5 clears part of the cells
    T_wc = np.asarray(data.sample_dict[frame]["T"], np.float64)
    renderer = cnr.view.SceneRenderer(cls_dict, scene_bg, cfg)
    inst_all = [e.inst_id for e in renderer.entities]
    assert inst_all.count(0) == 2, "this tree gives an object the background's id 0: grids go by entity index, not by id"
    once = [i for i in inst_all if inst_all.count(i) == 1]
    out, ref = tmp_path / "out", tmp_path / "ref"
    monkeypatch.setattr(sys, "argv", ["render_view.py", "--config", str(cfg_file), "--logdir", str(logdir), "--frame", str(frame),
                                      "--out", str(out), "--samples", "16", "--allow-pickle", "--hide", str(once[-1]),
                                      "--skip-empty", "--grid", str(G), "--tau", str(tau)])
    _tool().main()
    printed = capsys.readouterr().out
    renderer.build_grids(resolution=G, threshold=tau)
    share = float(renderer.grids().float().mean())
    assert 0.05 < share < 0.95, share
    with torch.no_grad():
        res = renderer.render(T_wc, n_samples=16, hidden={once[-1]}, skip_empty=True)
        evaluated, total = renderer.active_samples
        full = renderer.render(T_wc, n_samples=16, hidden={once[-1]})
    assert "evaluated {} of {} samples".format(evaluated, total) in printed and 0 < evaluated < total
    cnr.view.render_to_files(res, str(ref))
    for png in ("rgb.png", "depth.png", "instance.png"):
        a, b = _png(out, png), _png(ref, png)
        assert a.shape[:2] == (cfg.H, cfg.W) and np.array_equal(a, b), png
    assert not torch.equal(res["rgb"], full["rgb"]), "at this threshold the grids must skip something that shows"
