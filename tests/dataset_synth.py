"""TEST INFRASTRUCTURE: small seeded Replica- and ScanNet-style trees written with PIL (the layouts src/dataset.py reads).

Replica (72 x 48, 5 frames): rgb/rgb_<i>.png, depth/depth_<i>.png (uint16 mm), semantic_instance/ and semantic_class/
(uint16), traj_w_c.txt.  ScanNet (96 x 64, 6 frames): color/<i>.jpg, depth/<i>.png, instance-filt/ and label-filt/ (raw
uint16), pose/<i>.txt (frame 2 has an inf), intrinsic/intrinsic_depth.txt, and the refined masks instance-refined/<i>.npy
(int32) with inst_to_cls/<i>.pkl.  Colour and depth have the same size, so no resize is involved.

The label maps cover: background classes, an undefined class (class 0 with instance != 0), instance 0, instances of <= 10 px
extent, an instance split into disjoint blobs, instances absent from some frames, depth 0 and depth above max_depth, ids up to
65535 in the raw ScanNet masks (65536 after the loader's +1 shift)."""
import os
import pickle

import numpy as np
from PIL import Image

REPLICA_WH = (72, 48)
SCANNET_WH = (96, 64)
SCANNET_EDGE = 10            # the shipped ScanNet configs' camera.mw: the refined masks are stored cropped


def _png16(path, a):
    Image.fromarray(np.ascontiguousarray(a, dtype=np.uint16)).save(path)


def _box(inst, cls, iid, c, r0, r1, c0, c1):
    inst[r0:r1, c0:c1] = iid
    cls[r0:r1, c0:c1] = c


def _depth(rng, H, W, max_mm):
    d = rng.integers(300, max_mm, (H, W)).astype(np.uint16)
    d[rng.random((H, W)) < 0.05] = 0                                      # invalid
    d[rng.random((H, W)) < 0.05] = max_mm + 1500                          # beyond max_depth
    return d


def _pose(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = rng.uniform(-1, 1, 3)
    return T


def replica_labels(i, H, W):
    """(inst, cls) uint16 of frame i"""
    inst = np.full((H, W), 1, np.uint16)              # wall (93)
    cls = np.full((H, W), 93, np.uint16)
    _box(inst, cls, 2, 40, 38, H, 0, W)               # floor (40)
    _box(inst, cls, 3, 20, 5 + i, 25 + i, 4, 24)      # chair, moves down
    if i != 2:                                        # absent from frame 2
        _box(inst, cls, 4, 20, 8, 22, 40, 46)         # split chair: two blobs
        _box(inst, cls, 4, 20, 26, 36, 58, 70)
    _box(inst, cls, 5, 0, 12, 30, 26, 40)             # undefined class -> 1005
    _box(inst, cls, 6, 33, 2, 10, 60, 68)             # 8 x 8 px: too small
    if i % 2 == 1:
        _box(inst, cls, 7, 33, 30, 45, 30, 52)        # odd frames only
    if i == 0 or i == 3:
        _box(inst, cls, 0, 14, 0, 14, 48, 60)         # instance 0, class 14
    if i == 2 or i == 4:
        _box(inst, cls, 0, 0, 0, 14, 48, 60)          # instance 0, class 0: inst_dict[0][0]
    _box(inst, cls, 8, 12, 40, 47, 60, 72)            # blinds (background class) over the floor
    return inst, cls


def write_replica(root, n=5, seed=0):
    rng = np.random.default_rng(seed)
    W, H = REPLICA_WH
    for sub in ("rgb", "depth", "semantic_instance", "semantic_class"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    poses = []
    for i in range(n):
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(os.path.join(root, "rgb", f"rgb_{i}.png"))
        _png16(os.path.join(root, "depth", f"depth_{i}.png"), _depth(rng, H, W, 8000))
        inst, cls = replica_labels(i, H, W)
        _png16(os.path.join(root, "semantic_instance", f"semantic_instance_{i}.png"), inst)
        _png16(os.path.join(root, "semantic_class", f"semantic_class_{i}.png"), cls)
        poses.append(_pose(rng).reshape(-1))
    np.savetxt(os.path.join(root, "traj_w_c.txt"), np.array(poses), delimiter=" ")


def scannet_labels(i, H, W):
    """raw (inst, label) uint16 of frame i (ids before the loader's +1 shift)"""
    inst = np.zeros((H, W), np.uint16)                # raw 0: wall (class 1) -> id 1, background
    cls = np.full((H, W), 1, np.uint16)
    _box(inst, cls, 9, 3, 50, H, 0, W)                # floor (3)
    _box(inst, cls, 2, 5, 14 + i, 40 + i, 12, 40)     # table (5)
    _box(inst, cls, 3, 5, 14, 24, 50, 62)             # second table: two blobs
    _box(inst, cls, 3, 5, 30, 44, 70, 84)
    if i != 3:
        _box(inst, cls, 65535, 7, 20, 36, 44, 60)     # id 65535 -> 65536
    _box(inst, cls, 4, 7, 11, 19, 80, 88)             # 8 x 8 px: get_bbox2d gives None
    if i % 2 == 0:
        _box(inst, cls, 6, 0, 40, 48, 20, 34)         # class 0: background list
    return inst, cls


def write_scannet(root, n=6, seed=1):
    rng = np.random.default_rng(seed)
    W, H = SCANNET_WH
    e = SCANNET_EDGE
    for sub in ("color", "depth", "instance-filt", "label-filt", "pose", "intrinsic", "instance-refined", "inst_to_cls"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    K = np.array([[80.0, 0, 47.5, 0], [0, 80.0, 31.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    np.savetxt(os.path.join(root, "intrinsic", "intrinsic_depth.txt"), K, fmt="%f")
    for i in range(n):
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(os.path.join(root, "color", f"{i}.jpg"))
        _png16(os.path.join(root, "depth", f"{i}.png"), _depth(rng, H, W, 6000))
        inst, cls = scannet_labels(i, H, W)
        _png16(os.path.join(root, "instance-filt", f"{i}.png"), inst)
        _png16(os.path.join(root, "label-filt", f"{i}.png"), cls)
        T = _pose(rng)
        if i == 2:
            T[0, 3] = np.inf
        with open(os.path.join(root, "pose", f"{i}.txt"), "w") as f:
            f.write("\n".join(" ".join(repr(float(v)) for v in row) for row in T) + "\n")
        # refined masks as the reference stores them: shifted ids, background classes at 0, cropped
        ref = inst.astype(np.int32) + 1
        inst_to_cls = {0: 0}
        for iid in np.unique(ref):
            c = cls[ref == iid][0]
            if c in (1, 3, 0):
                ref[ref == iid] = 0
            else:
                inst_to_cls[iid] = c
        np.save(os.path.join(root, "instance-refined", f"{i}.npy"), ref[e:-e, e:-e])
        with open(os.path.join(root, "inst_to_cls", f"{i}.pkl"), "wb") as f:
            pickle.dump(inst_to_cls, f)


def write_registration_pickle(root, frames_json, seed=0):
    """<root>/inst_dict.pkl the way the reference's registration writes it (pickle.dump of inst_dict): for each class and
    instance of the recorded frame_info, {'frame_info': [{'frame', 'bbox' (int64 tensor)}], 'T_obj' (4,4) float64,
    'bbox3D': utils.BoundingBox}, numpy int32 keys; the background {'frame_info', 'bbox3D'}.  utils.BoundingBox is a stand-in
    module installed for the dump only."""
    import sys
    import types

    import torch
    rng = np.random.default_rng(seed)
    utils = types.ModuleType("utils")

    class BoundingBox:
        def __init__(self):
            self.extent, self.R, self.center, self.points3d = None, None, None, None

    BoundingBox.__module__, BoundingBox.__qualname__ = "utils", "BoundingBox"
    utils.BoundingBox = BoundingBox

    def box(extent):
        b = BoundingBox()
        b.extent, b.R, b.center = np.asarray(extent, np.float64), np.eye(3), np.zeros(3)
        b.points3d = rng.uniform(-1, 1, (8, 3))
        return b

    fi = lambda rows: [{"frame": f, "bbox": torch.from_numpy(np.array(b, dtype=np.int64))} for f, b in rows]
    inst_dict = {}
    for e in frames_json["inst_dict"]:
        c = np.int32(e["cls"])
        if e["cls"] == 0:
            inst_dict[c] = {"frame_info": fi(e["frame_info"]), "bbox3D": box([6.0, 6.0, 3.0])}
            continue
        inst_dict[c] = {}
        for k, i in enumerate(e["insts"]):
            T = _pose(rng)
            T[:3, :3] *= 0.5 + 0.1 * k
            inst_dict[c][np.int32(i["inst"])] = {"frame_info": fi(i["frame_info"]), "T_obj": T,
                                                 "bbox3D": box([1.0 + 0.1 * k, 0.8, 1.2])}
    saved = sys.modules.get("utils")
    sys.modules["utils"] = utils
    try:
        with open(os.path.join(root, "inst_dict.pkl"), "wb") as f:
            pickle.dump(inst_dict, f)
    finally:
        if saved is None:
            del sys.modules["utils"]
        else:
            sys.modules["utils"] = saved
    return inst_dict
