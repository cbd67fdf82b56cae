"""GPU: the frame-parsing kernels (csrc/frames.hip) against the numpy restatement (tests/dataset_cpu.py), bit for bit and run to
run; get_dataset on the committed trees against what the reference's get_all_frames recorded; and train.py:33-64 end to end
on a synthetic tree with a registration pickle written the reference's way."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

from dataset_cpu import CpuFrameTable, resize_linear, resize_nearest
from test_dataset_host import CONFIGS, DS, _config, _frames, check_against_fixture, load_capturing_frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cnr():
    import cnr_amd
    return cnr_amd


def _tables_equal(a, b):
    assert np.array_equal(a.offsets, b.offsets)
    assert np.array_equal(a.ids, b.ids) and np.array_equal(a.stats, b.stats)


def _label_cases(rng):
    """(name, inst (F,Hs,Ws), cls or None, edge, shift)"""
    H, W = 37, 53
    yield "random_u16", rng.integers(0, 40, (3, H, W)).astype(np.uint16), rng.integers(0, 3, (3, H, W)).astype(np.uint16), 0, 0
    blob = np.zeros((2, 61, 45), np.uint16)
    blob[:, 5:20, 3:9], blob[:, 30:31, 40:41], blob[1, 50:, :] = 65535, 7, 12
    yield "blobs_edge_shift", blob, (blob % 5).astype(np.uint16), 4, 1
    yield "every_pixel_own_id", np.arange(3 * 29 * 31).reshape(3, 29, 31).astype(np.int32), None, 0, 0
    yield "one_id", np.full((2, 33, 17), 9, np.uint16), np.full((2, 33, 17), 4, np.uint16), 0, 0
    yield "no_zero", rng.integers(1, 5, (2, 19, 23)).astype(np.int32), rng.integers(0, 2, (2, 19, 23)).astype(np.int32), 2, 0
    big = rng.integers(0, 3000, (1, 300, 257)).astype(np.int32)                  # > 1024 ids: the global-atomics path
    big[0, :3, :3] = 65536
    yield "many_ids_i32", big, (big % 7).astype(np.int32), 0, 0
    yield "large_frame", rng.integers(0, 6, (2, 680, 1200)).astype(np.uint16), None, 0, 0
    yield "single_pixel", np.zeros((1, 1, 1), np.uint16), None, 0, 1


def test_instance_table_matches_the_restatement(cnr, dev):
    rng = np.random.default_rng(3)
    for name, inst, cls, edge, shift in _label_cases(rng):
        ti = torch.from_numpy(inst).to(dev)
        tc = None if cls is None else torch.from_numpy(cls).to(dev)
        got = cnr.dataset.FrameTable(ti, tc, edge=edge, id_shift=shift)
        ref = CpuFrameTable(inst, cls, edge=edge, id_shift=shift)
        _tables_equal(got, ref)
        again = cnr.dataset.FrameTable(ti, tc, edge=edge, id_shift=shift)
        _tables_equal(got, again)
        # finish: keep every other id
        keep = np.arange(len(ref.ids)) % 2 == 0
        F, Hs, Ws = inst.shape
        depth = rng.integers(0, 9000, (F, Hs, Ws)).astype(np.uint16)
        rgb = rng.integers(0, 256, (F, Hs, Ws, 3), dtype=np.uint8)
        g = got.finish(keep, torch.from_numpy(depth).to(dev), torch.from_numpy(rgb).to(dev), edge, 0.001, 8.0)
        r = ref.finish(keep, depth, rgb, edge, 0.001, 8.0)
        for a, b, what in zip(g, r, ("obj_mask", "depth", "image")):
            assert a.dtype == b.dtype and torch.equal(a.cpu(), b), (name, what)
    # ids 0, 65535 and 65536 (a raw 65535 shifted) in one frame
    inst = np.zeros((1, 8, 8), np.uint16)
    inst[0, 0, 0], inst[0, 7, 7] = 65535, 65534
    t = cnr.dataset.FrameTable(torch.from_numpy(inst).to(dev), id_shift=1)
    assert t.ids.tolist() == [1, 65535, 65536] and t.stats[:, 0].tolist() == [62, 1, 1]


def test_instance_table_is_blind_to_the_workgroup_split(cnr, dev):
    """a frame stacked with others or alone gives the same rows (chunks of the grid never shift a result)"""
    rng = np.random.default_rng(5)
    inst = rng.integers(0, 50, (4, 200, 333)).astype(np.uint16)
    all4 = cnr.dataset.FrameTable(torch.from_numpy(inst).to(dev))
    for f in range(4):
        one = cnr.dataset.FrameTable(torch.from_numpy(inst[f:f + 1]).to(dev))
        a, b = all4.frame(f), one.frame(0)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("src,dst", [((968, 1296), (480, 640)), ((48, 72), (48, 72)), ((17, 23), (40, 9)), ((5, 7), (2, 3)),
                                     ((1, 1), (3, 4))])
def test_resize_kernels_match_the_restatement(cnr, dev, src, dst):
    rng = np.random.default_rng(sum(src) + sum(dst))
    a = rng.integers(0, 256, (2,) + src + (3,), dtype=np.uint8)
    got = cnr.dataset.resize_linear(torch.from_numpy(a).to(dev), *dst).cpu()
    assert torch.equal(got, resize_linear(a, *dst))
    if src == dst:
        assert np.array_equal(got.numpy(), a)
    for dt in (np.uint16, np.int32):
        lab = rng.integers(0, 60000, (2,) + src).astype(dt)
        assert torch.equal(cnr.dataset.resize_nearest(torch.from_numpy(lab).to(dev), *dst).cpu(), resize_nearest(lab, *dst))


def _tree_with_cache(tmp_path, name):
    from dataset_synth import write_registration_pickle
    tree = "replica" if name == "replica" else "scannet"
    root = str(tmp_path / tree)
    shutil.copytree(os.path.join(DS, tree), root)
    write_registration_pickle(root, _frames(name))
    return root


@pytest.mark.parametrize("name", CONFIGS)
def test_get_dataset_matches_the_reference(cnr, tmp_path, name):
    cfg = _config(cnr, name, root=_tree_with_cache(tmp_path, name))
    ds, frames_inst_dict = load_capturing_frames(cnr.dataset, cfg)
    assert isinstance(ds, cnr.dataset.Replica if name == "replica" else cnr.dataset.ScanNet)
    check_against_fixture(ds, frames_inst_dict, name)


def test_train_py_construction_end_to_end(cnr, dev, tmp_path):
    """train.py:33-64: cameraInfo, get_dataset, one sceneCategory per class; pools bit-equal to those built from the fixture's
    sample_dict; then FullStepTrainer.from_scene trains a few steps and Trainer.meshing returns a mesh."""
    from cnr_amd.scene_cateogries import cameraInfo, sceneCategory
    root = _tree_with_cache(tmp_path, "replica")
    with open(os.path.join(DS, "replica.json")) as f:
        c = json.load(f)
    c["dataset"]["path"] = root
    c["camera"].update(w=72, h=48, fx=60.0, fy=60.0, cx=35.5, cy=23.5)
    c["model"]["net_hyperparams"]["latent_dim"] = 32
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps(c))
    cfg = cnr.cfg.Config(str(p))
    cam_info = cameraInfo(cfg)
    data = cnr.dataset.get_dataset(cfg)
    z = np.load(os.path.join(DS, "replica_samples.npz"))
    fixture_samples = {int(f): dict(image=z["image"][i], depth=z["depth"][i], obj_mask=z["obj_mask"][i], T=z["T"][i])
                       for i, f in enumerate(z["frames"])}

    def build(sample_dict):
        np.random.seed(0)
        torch.manual_seed(0)
        cls_dict, scene_bg = {}, None
        for cls_id in data.inst_dict.keys():
            sc = sceneCategory(cfg, cls_id, data.inst_dict[cls_id], sample_dict, cam_info.rays_dir_cache)
            if cls_id == 0:
                scene_bg = sc
            else:
                cls_dict[cls_id] = sc
        return cls_dict, scene_bg

    cls_dict, scene_bg = build(data.sample_dict)
    ref_cls, ref_bg = build(fixture_samples)
    for a, b in list(zip(cls_dict.values(), ref_cls.values())) + [(scene_bg, ref_bg)]:
        for key in ("rgbs_batch_all", "depth_batch_all", "ray_dirs_batch_all", "batch_indices_all"):
            assert torch.equal(getattr(a, key), getattr(b, key)), key
    full = cnr.background.FullStepTrainer.from_scene(cls_dict, scene_bg, cfg, seed=1, use_graph=False)
    for _ in range(5):
        full.step()
    torch.cuda.synchronize()
    assert torch.isfinite(full.obj.losses).all() and torch.isfinite(full.bg.losses).all()
    full.sync_to_modules()
    cls_k = next(iter(cls_dict.values()))
    obj_id = cls_k.obj_ids[0]
    mesh = cls_k.trainer.meshing(obj_id, grid_dim=32) if len(cls_k.obj_ids) > 1 else None
    bg_mesh = scene_bg.trainer.meshing(grid_dim=32)
    assert bg_mesh is not None and len(bg_mesh.vertices) > 0 and len(bg_mesh.faces) > 0
    assert mesh is None or len(mesh.faces) > 0
