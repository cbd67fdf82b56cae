"""CPU: the host half of category registration: the 24 box symmetries, poses and boxes from point clouds on
hand-computed cases, the restatement's ICP, the cache file's format, and get_dataset's register= argument."""
import pickletools
from itertools import permutations

import numpy as np
import pytest
import torch

import registration_cpu as RC
from test_dataset_host import _config


@pytest.fixture(scope="module")
def cnr():
    import cnr_amd
    return cnr_amd


class _Cloud:
    def __init__(self, pts):
        self.points = np.asarray(pts, np.float64)


def test_possible_transforms_are_the_24_box_symmetries_in_order(cnr):
    L = cnr.utils.get_possible_transform_from_bbox()
    assert len(L) == 24
    seen = set()
    for T in L:
        R = T[:3, :3]
        assert np.array_equal(T[3], [0, 0, 0, 1]) and np.array_equal(T[:3, 3], [0, 0, 0])
        assert np.array_equal(R @ R.T, np.eye(3)) and np.linalg.det(R) == pytest.approx(1.0)
        assert set(np.abs(R).ravel()) == {0.0, 1.0}
        seen.add(tuple(R.astype(int).ravel()))
    assert len(seen) == 24
    # the order: (x, y) axis pairs as itertools.permutations gives them, signs (+,+), (-,+), (+,-), (-,-); columns x, y, x cross y
    k = 0
    for ax, ay in permutations(range(3), 2):
        for sx, sy in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
            x, y = sx * np.eye(3)[ax], sy * np.eye(3)[ay]
            assert np.array_equal(L[k][:3, :3], np.stack([x, y, np.cross(x, y)], 1)), k
            k += 1
    assert np.array_equal(L[0], np.eye(4))
    assert np.array_equal(L[1][:3, :3], np.diag([-1.0, 1.0, -1.0]))


def test_transform_pointcloud_hand_case(cnr):
    T = np.array([[0.0, -1.0, 0.0, 1.0], [1.0, 0.0, 0.0, 2.0], [0.0, 0.0, 1.0, 3.0], [0.0, 0.0, 0.0, 1.0]])
    out = cnr.utils.transform_pointcloud(np.array([[1.0, 0.0, 0.0], [0.0, 2.0, 5.0]]), T)
    assert np.array_equal(out, [[1.0, 3.0, 3.0], [-1.0, 2.0, 8.0]])


def test_get_obb_hand_case(cnr):
    # T_obj: scale 2, rotation 90 degrees about z, centre (1, 1, 0); the cloud's corners in that frame are known
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = 2.0 * Rz, [1.0, 1.0, 0.0]
    local = np.array([[0.5, 0.1, 0.02], [-0.3, -0.2, -0.01], [0.1, 0.25, 0.0]])
    info = {"T_obj": T.copy(), "pcs": _Cloud(local @ Rz.T + [1.0, 1.0, 0.0])}
    cnr.utils.get_obb(info)
    b = info["bbox3D"]
    assert np.allclose(b.R, Rz) and np.allclose(b.center, [1.0, 1.0, 0.0])
    assert np.allclose(b.extent, [1.0, 0.5, 0.10])             # 2 max(|max|, |min|) per axis, at least 10 cm
    assert np.allclose(info["T_obj"][:3, :3], Rz * 0.5) and np.allclose(info["T_obj"][:3, 3], [1.0, 1.0, 0.0])


def test_get_pose_from_pointcloud_hand_case(cnr):
    # the 8 corners and some inner points of a 2 x 1 x 0.5 box, rotated and moved: the oriented box is that box
    rng = np.random.default_rng(0)
    ext = np.array([2.0, 1.0, 0.5])
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * ext / 2
    pts = np.concatenate([corners, (rng.random((200, 3)) - 0.5) * ext])
    a = 0.4
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    c = np.array([0.3, -1.2, 2.0])
    T_obj, box = cnr.utils.get_pose_from_pointcloud(_Cloud(pts @ R.T + c))
    assert np.allclose(box.center, c, atol=1e-9) and np.allclose(sorted(box.extent), sorted(ext), atol=1e-9)
    assert np.allclose(box.R @ box.R.T, np.eye(3), atol=1e-12)
    # every axis of the box is an axis of the true box, up to sign
    assert np.allclose(np.sort(np.abs(box.R.T @ R), axis=None)[-3:], 1.0, atol=1e-9)
    assert np.allclose(T_obj[:3, :3], box.R * 1.0) and np.allclose(T_obj[:3, 3], c, atol=1e-9)      # scale = max extent / 2 = 1
    assert np.linalg.det(T_obj[:3, :3]) > 0
    # small extents are raised to 10 cm
    _, thin = cnr.utils.get_pose_from_pointcloud(_Cloud(pts * [1.0, 1.0, 0.02]))
    assert sorted(thin.extent)[0] == pytest.approx(0.10)


def test_cloud_without_a_hull_raises_naming_the_instance(cnr):
    line = np.stack([np.linspace(0, 1, 20), np.zeros(20), np.zeros(20)], 1)
    assert cnr.utils.get_bound(_Cloud(line)) is None
    with pytest.raises(ValueError, match="instance 17"):
        cnr.utils.get_pose_from_pointcloud(_Cloud(line), inst_id=17)


def test_restatement_icp_recovers_a_known_transform():
    rng = np.random.default_rng(5)
    tgt = rng.random((3000, 3)) * [1.0, 0.6, 0.3]
    a = 0.12
    R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    T_true = np.eye(4)
    T_true[:3, :3], T_true[:3, 3] = R, [0.02, -0.03, 0.01]
    src = (tgt[:2000] - T_true[:3, 3]) @ R                     # T_true . src = tgt
    T, fitness, rmse, updates = RC.icp(src, tgt, np.eye(4), 0.10)
    assert fitness == 1.0 and rmse < 1e-9 and updates < 100
    assert np.allclose(T, T_true, atol=1e-8)
    # the 17 sums give the same update as the direct fit
    a32 = RC.transform32(np.eye(4), src)
    d, j = RC.cKDTree(tgt.astype(np.float32).astype(np.float64)).query(a32.astype(np.float64))
    s, _ = RC.icp_sums(src, tgt, np.eye(4), j, d, 0.10)
    assert s[0] == (d.astype(np.float32) < np.float32(0.10)).sum()
    dT = RC.kabsch(s)
    assert np.allclose(dT[:3, :3] @ dT[:3, :3].T, np.eye(3), atol=1e-12) and np.linalg.det(dT[:3, :3]) > 0


def test_restatement_voxel_down_sample_hand_case():
    p = np.array([[0.0, 0.0, 0.0], [0.004, 0.0, 0.0], [0.006, 0.0, 0.0], [0.02, 0.01, 0.0]], np.float32)
    m, _, keys, counts = RC.voxel_down_sample(p, None, 0.01)
    # min - v / 2 = -0.005: x indices 0, 0, 1, 2
    assert list(counts) == [2, 1, 1] and list(keys >> 42) == [0, 1, 2]
    assert np.allclose(m[0], p[:2].astype(np.float64).mean(0)) and np.allclose(m[2], p[3].astype(np.float64))


def test_written_cache_names_utils_boundingbox_and_reloads(cnr, tmp_path):
    box = cnr.utils.BoundingBox()
    box.center, box.R, box.extent = np.array([1.0, 2.0, 3.0]), np.eye(3), np.array([0.5, 0.4, 0.3])
    inst_dict = {np.int32(20): {np.int32(3): {"frame_info": [{"frame": 0, "bbox": torch.tensor([1, 2, 3, 4])}],
                                              "T_obj": np.eye(4) * 2.0, "bbox3D": box}},
                 0: {"frame_info": [], "bbox3D": box}}
    path = str(tmp_path / "inst_dict.pkl")
    import sys
    before = sys.modules.get("utils")
    cnr.category_registration.write_registration_result(inst_dict, path)
    assert sys.modules.get("utils") is before                 # the stand-in module of the dump is gone again
    raw = open(path, "rb").read()
    names = [arg for op, arg, _ in pickletools.genops(raw) if op.name in ("GLOBAL", "STACK_GLOBAL", "SHORT_BINUNICODE", "BINUNICODE")]
    assert "utils" in names and "BoundingBox" in names
    assert b"cnr_amd" not in raw and b"category-nerf" not in raw
    back = cnr.dataset.load_registration_result(path)
    assert list(back.keys()) == [20, 0]
    got = back[20][3]["bbox3D"]
    assert type(got) is cnr.utils.BoundingBox and got.points3d is None
    assert np.array_equal(got.center, box.center) and np.array_equal(got.extent, box.extent) and np.array_equal(got.R, box.R)
    assert np.array_equal(back[20][3]["T_obj"], np.eye(4) * 2.0)
    assert torch.equal(back[20][3]["frame_info"][0]["bbox"], torch.tensor([1, 2, 3, 4]))


def test_get_dataset_accepts_register_and_scannet_still_raises(cnr):
    from dataset_cpu import cpu_loader
    cfg = _config(cnr, "scannet_refined")
    with cpu_loader() as D, pytest.raises(NotImplementedError, match="registration"):
        D.get_dataset(cfg, register=True)
    with pytest.raises(NotImplementedError, match="ScanNet"):
        cnr.category_registration.get_all_poses({}, {}, None, name="scannet")


def test_register_without_pretrained_fields_raises(cnr):
    """the reference's `else: NotImplementedError()` registers nothing; the driver says so"""
    from dataset_cpu import cpu_loader
    cfg = _config(cnr, "replica")
    cfg.load_pretrained = False
    with cpu_loader() as D, pytest.raises(NotImplementedError, match="load_pretrained"):
        D.get_dataset(cfg, register=True)


def test_icp_case_has_no_pair_at_the_threshold():
    """CPU: in the restatement alone no pair of the ICP case lies within fp32 rounding of max_corr (8 ulp of the distance
    scale, relative 1e-6), so count and membership can be compared exactly"""
    from test_pointcloud_gpu import _icp_case
    src, tgt, Ts, max_corr = _icp_case()
    for T in Ts:
        d, _ = RC.cKDTree(tgt.astype(np.float64)).query(RC.transform32(T, src).astype(np.float64))
        assert (np.abs(d - max_corr) < 1e-6 * max_corr * 8).sum() == 0
        assert 3 < (d < max_corr).sum()


def test_no_replica_fixture_instance_is_degenerate(cnr):
    """CPU guard for test_get_dataset_register_writes_a_cache_that_reloads_gpu: every instance of the committed Replica frames
    (and the background) unprojects to a cloud with a 3-D hull, so registration on a copy of that tree cannot fail on a
    degenerate cloud"""
    from test_pointcloud_gpu import _replica
    cfg, samples, insts = _replica(cnr)
    assert len(insts) == 6
    for cls, inst, info in insts:
        pts = np.concatenate([RC.unproject(samples[fi["frame"]], inst, cfg.fx, cfg.fy, cfg.cx, cfg.cy)[1] for fi in info])
        means, _, _, _ = RC.voxel_down_sample(pts.astype(np.float32), None, 0.01)
        assert len(means) >= 100, (cls, inst)
        box = cnr.utils.get_bound(means)
        assert box is not None and box.extent.min() >= 0.10, (cls, inst)
