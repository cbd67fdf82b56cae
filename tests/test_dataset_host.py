"""CPU: cfg.Config on the reference's configs, the dataset helpers of utils, the registration cache's restricted unpickler, and
the loaders' host logic on the numpy restatement of csrc/frames.hip (tests/dataset_cpu.py) against what the reference's
get_all_frames recorded (tests/golden/gen_dataset_golden.py)."""
import json
import os
import pickle
import shutil
import sys
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN

DS = os.path.join(GOLDEN, "dataset")
CONFIGS = ("replica", "scannet_refined", "scannet_raw")


def _frames(name):
    with open(os.path.join(DS, name + "_frames.json")) as f:
        return json.load(f)


def _config(cnr, name, root=None, **over):
    """cfg.Config of a committed config, the dataset path resolved against tests/golden/dataset (or `root`)"""
    with open(os.path.join(DS, name + ".json")) as f:
        c = json.load(f)
    c["dataset"]["path"] = root or os.path.join(DS, c["dataset"]["path"])
    for k, v in over.items():
        sec, key = k.split("__")
        c[sec][key] = v
    import tempfile
    fd, p = tempfile.mkstemp(suffix=".json")
    with os.fdopen(fd, "w") as f:
        json.dump(c, f)
    try:
        return cnr.cfg.Config(p)
    finally:
        os.remove(p)


def inst_dict_rows(inst_dict):
    """inst_dict -> the fixture's form (keys in insertion order, frames, bboxes as lists)"""
    rows = []
    for cls_id, d in inst_dict.items():
        e = {"cls": int(cls_id), "insts": []}
        for key, v in d.items():
            if key == "frame_info":
                e["frame_info"] = [[int(fi["frame"]), [int(b) for b in fi["bbox"]]] for fi in v]
            else:
                e["insts"].append({"inst": int(key), "frame_info": [[int(fi["frame"]), [int(b) for b in fi["bbox"]]]
                                                                   for fi in v["frame_info"]]})
        rows.append(e)
    return rows


def load_capturing_frames(D, cfg):
    """D.get_dataset(cfg) -> (dataset, the inst_dict get_all_frames built before the cached registration replaced it)"""
    seen, load = {}, D._load_inst_dict

    def spy(ds, c):
        seen["inst_dict"] = ds.inst_dict
        load(ds, c)

    D._load_inst_dict = spy
    try:
        return D.get_dataset(cfg), seen["inst_dict"]
    finally:
        D._load_inst_dict = load


def check_against_fixture(ds, inst_dict, name):
    """sample_dict bit-equal to the reference's, frame_info equal including order, n_img equal"""
    z = np.load(os.path.join(DS, name + "_samples.npz"))
    rec = _frames(name)
    assert ds.n_img == rec["n_img"] and len(ds) == rec["n_img"]
    assert list(ds.sample_dict.keys()) == [int(f) for f in z["frames"]]
    for i, f in enumerate(int(f) for f in z["frames"]):
        s = ds.sample_dict[f]
        for key in ("image", "depth", "obj_mask", "T"):
            ref = z[key][i]
            assert s[key].dtype == ref.dtype and s[key].shape == ref.shape, (f, key, s[key].dtype, s[key].shape)
            assert np.array_equal(s[key], ref), (f, key)
        assert s["frame_id"] == int(z["frame_id"][i])
        assert s["image"].dtype == np.uint8 and s["depth"].dtype == np.float32 and s["obj_mask"].dtype == np.int32
    assert inst_dict_rows(inst_dict) == rec["inst_dict"]
    for d in inst_dict.values():
        for v in d.values():
            for fi in (v if isinstance(v, list) else v["frame_info"]):
                assert fi["bbox"].dtype == torch.int64


@pytest.fixture(scope="module")
def cnr():
    import cnr_amd
    return cnr_amd


# ---- Config ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CONFIGS)
def test_config_matches_the_reference(cnr, name, monkeypatch):
    monkeypatch.chdir(DS)
    cfg = cnr.cfg.Config(name + ".json")
    with open(os.path.join(DS, name + "_config.json")) as f:
        rec = json.load(f)
    for k, v in rec.items():
        got = getattr(cfg, k)
        if isinstance(v, dict) and "ndarray" in v:
            assert isinstance(got, np.ndarray) and np.array_equal(got, np.array(v["ndarray"], dtype=v["dtype"])), k
        else:
            assert got == v and type(got) in (type(v), np.float64) or (got == v and isinstance(v, float)), (k, got, v)


def test_scannet_intrinsics_come_from_the_file(cnr, monkeypatch):
    monkeypatch.chdir(DS)
    cfg = cnr.cfg.Config("scannet_raw.json")
    K = cnr.utils.load_matrix_from_txt(os.path.join("scannet", "intrinsic", "intrinsic_depth.txt"))
    assert (cfg.fx, cfg.fy, cfg.cx, cfg.cy) == (K[0, 0], K[1, 1], K[0, 2] - cfg.mw, K[1, 2] - cfg.mh)
    # no file: fx ... stay unset, as before
    monkeypatch.chdir(os.path.dirname(DS))
    assert not hasattr(cnr.cfg.Config(os.path.join(DS, "scannet_raw.json")), "fx")


def test_config_without_dataset_keys_keeps_the_hot_path_attributes(cnr, tmp_path):
    with open(os.path.join(DS, "replica.json")) as f:
        c = json.load(f)
    full = _config(cnr, "replica")
    del c["dataset"], c["registration"]
    p = tmp_path / "c.json"
    p.write_text(json.dumps(c))
    lean = cnr.cfg.Config(str(p))
    for k, v in vars(lean).items():
        assert np.array_equal(v, getattr(full, k)) if isinstance(v, np.ndarray) else v == getattr(full, k), k
    assert not hasattr(lean, "dataset_format") and lean.distortion_array is None


# ---- utils -------------------------------------------------------------------------------------------------------------
def test_enlarge_bbox_values():
    from cnr_amd.utils import enlarge_bbox
    assert enlarge_bbox([10, 20, 40, 25], 0.2, w=100, h=50) is None                 # margin_y = int(0.5) = 0
    assert enlarge_bbox([10, 20, 40, 45], 0.2, w=100, h=50) == [7, 18, 43, 47]
    assert enlarge_bbox([0, 0, 99, 49], 0.2, w=100, h=50) == [0, 0, 99, 49]         # clipped
    t = [torch.tensor(v) for v in (3, 5, 60, 33)]                                   # tensors: float32 margins (Replica)
    assert enlarge_bbox(t, 0.2, w=48, h=72) == [0, 3, 47, 35]
    assert enlarge_bbox([5, 5, 15, 15], 0.0, w=30, h=30) is None


def test_get_bbox2d_batch_values():
    from cnr_amd.utils import get_bbox2d_batch
    m = torch.zeros(3, 7, 5, dtype=torch.bool)
    m[0, 2:4, 1:3] = True
    m[1, 6, 4] = True
    rmins, rmaxs, cmins, cmaxs = get_bbox2d_batch(m)
    assert rmins.tolist() == [2, 6, 0] and rmaxs.tolist() == [4, 7, 7] and cmins.tolist() == [1, 4, 0]
    assert cmaxs.tolist() == [3, 5, 5] and rmins.dtype == torch.int64


# ---- registration cache ------------------------------------------------------------------------------------------------
def test_unpickler_loads_the_reference_pickle(cnr, tmp_path):
    from dataset_synth import write_registration_pickle
    written = write_registration_pickle(str(tmp_path), _frames("replica"))
    got = cnr.dataset.load_registration_result(str(tmp_path / "inst_dict.pkl"))
    assert list(got.keys()) == list(written.keys()) and all(type(k) is np.int32 for k in got)
    for c, d in written.items():
        assert list(got[c].keys()) == list(d.keys())
        for k, v in d.items():
            g = got[c][k]
            if k == "frame_info" or k == "bbox3D":
                v = {k: v}
                g = {k: g}
            for key in v:
                if key == "frame_info":
                    assert [(a["frame"], a["bbox"].tolist()) for a in g[key]] == [(a["frame"], a["bbox"].tolist()) for a in v[key]]
                    assert all(a["bbox"].dtype == torch.int64 for a in g[key])
                elif key == "bbox3D":
                    assert isinstance(g[key], cnr.utils.BoundingBox)
                    assert np.array_equal(g[key].extent, v[key].extent) and np.array_equal(g[key].points3d, v[key].points3d)
                else:
                    assert np.array_equal(g[key], v[key]) and g[key].dtype == np.float64


class Foreign:
    pass


def test_unpickler_refuses_a_foreign_global(cnr, tmp_path):
    p = tmp_path / "inst_dict.pkl"
    p.write_bytes(pickle.dumps({1: {"frame_info": [], "x": Foreign()}}))
    with pytest.raises(pickle.UnpicklingError, match="Foreign"):
        cnr.dataset.load_registration_result(str(p))
    p.write_bytes(pickle.dumps({1: os.system}))
    with pytest.raises(pickle.UnpicklingError, match="system"):
        cnr.dataset.load_registration_result(str(p))


def test_unknown_format_raises(cnr):
    with pytest.raises(ValueError, match="Matterport"):
        cnr.dataset.get_dataset(types.SimpleNamespace(dataset_format="Matterport"))


# ---- the loaders' host logic on the restatement -------------------------------------------------------------------------
@pytest.mark.parametrize("name", CONFIGS)
def test_restatement_reproduces_the_fixtures(cnr, name, tmp_path):
    from dataset_cpu import cpu_loader
    from dataset_synth import write_registration_pickle
    tree = "replica" if name == "replica" else "scannet"
    root = str(tmp_path / tree)
    shutil.copytree(os.path.join(DS, tree), root)
    write_registration_pickle(root, _frames(name))
    cfg = _config(cnr, name, root=root)
    with cpu_loader() as D:
        ds, frames_inst_dict = load_capturing_frames(D, cfg)
    assert isinstance(ds.inst_dict[0]["bbox3D"], cnr.utils.BoundingBox)                       # the cache, loaded
    check_against_fixture(ds, frames_inst_dict, name)


@pytest.mark.parametrize("name", CONFIGS)
def test_missing_cache_raises_not_implemented(cnr, name):
    from dataset_cpu import cpu_loader
    cfg = _config(cnr, name)
    with cpu_loader() as D, pytest.raises(NotImplementedError, match="registration"):
        D.get_dataset(cfg)
    cfg.load_registration_result = False
    with cpu_loader() as D, pytest.raises(NotImplementedError, match="registration"):
        D.get_dataset(cfg)


def test_scannet_without_refined_masks_needs_segmentation(cnr, tmp_path):
    from dataset_cpu import cpu_loader
    root = str(tmp_path / "scannet")
    shutil.copytree(os.path.join(DS, "scannet"), root)
    os.remove(os.path.join(root, "instance-refined", "3.npy"))
    cfg = _config(cnr, "scannet_refined", root=root)
    with cpu_loader() as D, pytest.raises(NotImplementedError, match="geometry_segmentation"):
        D.get_dataset(cfg)


def test_resize_restatement_identities():
    from dataset_cpu import resize_linear, resize_nearest
    rng = np.random.default_rng(0)
    a = rng.integers(0, 256, (2, 9, 13, 3), dtype=np.uint8)
    assert np.array_equal(resize_linear(a, 9, 13).numpy(), a)                       # same size: identity, as cv2 copies
    up = resize_linear(a, 18, 26).numpy()                                           # 2x up: exact pixel centres at 1/4, 3/4
    assert np.array_equal(up[:, ::2, ::2][:, 1:-1, 1:-1].shape, (2, 7, 11, 3))
    assert np.array_equal(resize_nearest(a[..., 0].astype(np.uint16), 18, 26).numpy()[:, ::2, ::2], a[..., 0])
    flat = np.full((1, 5, 7, 3), 77, np.uint8)
    assert (resize_linear(flat, 11, 3).numpy() == 77).all()
