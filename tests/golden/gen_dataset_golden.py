"""Generate tests/golden/dataset/ by RUNNING THE REFERENCE's src/dataset.py and src/cfg.py (build container only).

    python tests/golden/gen_dataset_golden.py REFERENCE_ROOT          (the reference checkout: REFERENCE_ROOT/src/dataset.py)

Writes the synthetic trees of tests/dataset_synth.py (replica/, scannet/), the configs (copies of the reference's
configs/Replica/config_replica_room0.json and configs/ScanNet/config_scannet_0013.json with the dataset path pointed at a
tree; scannet_raw.json with use_refined_mask off), and, per config, what the reference's Replica / ScanNet get_all_frames
made: every sample_dict array (<name>_samples.npz), the inst_dict frame_info in insertion order and n_img (<name>.json),
and the reference Config's attributes (<name>_config.json).

The reference is imported read-only at run time; packages missing here are replaced by stand-ins, installed first:
  cv2         imread via PIL (colour returned BGR, as cv2 does), cvtColor(BGR2RGB) reverses the channels, resize only for an
              unchanged size (the trees keep colour and depth the same size), findContours + boundingRect give the mask's
              bounding box (x, y, w, h) with w, h = max - min + 1;
  open3d      PinholeCameraIntrinsic as a plain record; unproject_pointcloud (ScanNet's 'pcs', out of scope) returns [];
  torchvision transforms.Compose; imgviz, functorch, trimesh, plotly: empty; category_registration: empty (the
  construction stops right after get_all_frames, before registration).
Only data is written -- no reference source or bytecode."""
import importlib
import json
import os
import shutil
import sys
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "dataset")
sys.path.insert(0, os.path.dirname(HERE))          # tests/


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def _install_stand_ins():
    def imread(path, flag=1):
        a = np.asarray(Image.open(path))
        if flag in (-1,):
            return a
        return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"))[..., ::-1])

    def resize(src, dsize, interpolation=None):
        if tuple(src.shape[1::-1]) != tuple(dsize):
            raise NotImplementedError("stand-in cv2.resize: size changes are not recorded")
        return src.copy()

    def find_contours(mask, mode, method):
        ys, xs = np.nonzero(mask)
        if len(xs) == 0:
            return [], None
        return [np.array([[[xs.min(), ys.min()]], [[xs.max(), ys.max()]]], np.int32)], None

    def bounding_rect(cnt):
        p = cnt.reshape(-1, 2)
        x0, y0 = p.min(0)
        x1, y1 = p.max(0)
        return int(x0), int(y0), int(x1 - x0 + 1), int(y1 - y0 + 1)

    _stub("cv2", imread=imread, cvtColor=lambda a, code: np.ascontiguousarray(a[..., ::-1]), resize=resize,
          findContours=find_contours, boundingRect=bounding_rect, IMREAD_UNCHANGED=-1, COLOR_BGR2RGB=4, INTER_LINEAR=1,
          INTER_NEAREST=0, RETR_EXTERNAL=0, CHAIN_APPROX_SIMPLE=2, CV_32FC1=5)

    class PinholeCameraIntrinsic:
        def __init__(self, width, height, fx, fy, cx, cy):
            self.width, self.height, self.fx, self.fy, self.cx, self.cy = width, height, fx, fy, cx, cy

    o3d = _stub("open3d")
    o3d.camera = _stub("open3d.camera", PinholeCameraIntrinsic=PinholeCameraIntrinsic)

    class Compose:
        def __init__(self, ts):
            self.ts = ts

        def __call__(self, x):
            for t in self.ts:
                x = t(x)
            return x

    tv = _stub("torchvision")
    tv.transforms = _stub("torchvision.transforms", Compose=Compose)
    _stub("imgviz")
    _stub("functorch", combine_state_for_ensemble=None, vmap=None)
    _stub("trimesh")
    plotly = _stub("plotly")
    plotly.graph_objs = _stub("plotly.graph_objs")
    plotly.subplots = _stub("plotly.subplots", make_subplots=None)
    _stub("category_registration")


def _configs(ref_root):
    out = {}
    rep = json.load(open(os.path.join(ref_root, "configs", "Replica", "config_replica_room0.json")))
    rep["dataset"]["path"] = "replica"
    out["replica"] = rep
    sn = json.load(open(os.path.join(ref_root, "configs", "ScanNet", "config_scannet_0013.json")))
    sn["dataset"]["path"] = "scannet"
    out["scannet_refined"] = sn
    raw = json.loads(json.dumps(sn))
    raw["dataset"]["use_refined_mask"] = False
    raw["dataset"]["load_refined_mask"] = False
    out["scannet_raw"] = raw
    return out


def _plain(v):
    if isinstance(v, np.ndarray):
        return {"ndarray": v.tolist(), "dtype": str(v.dtype)}
    if isinstance(v, np.generic):
        return v.item()
    return v


class _Stop(Exception):
    pass


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref_root = os.path.abspath(sys.argv[1])
    import dataset_synth
    os.makedirs(OUT, exist_ok=True)
    for name, write in (("replica", dataset_synth.write_replica), ("scannet", dataset_synth.write_scannet)):
        shutil.rmtree(os.path.join(OUT, name), ignore_errors=True)
        write(os.path.join(OUT, name))
    _install_stand_ins()
    sys.path.insert(0, os.path.join(ref_root, "src"))
    ref_cfg = importlib.import_module("cfg")
    ref_ds = importlib.import_module("dataset")
    ref_ds.unproject_pointcloud = lambda *a, **k: []
    os.chdir(OUT)
    for name, cfg_json in _configs(ref_root).items():
        with open(name + ".json", "w") as f:
            json.dump(cfg_json, f, indent=4)
        cfg = ref_cfg.Config(name + ".json")
        with open(name + "_config.json", "w") as f:
            json.dump({k: _plain(v) for k, v in vars(cfg).items()}, f, indent=1, sort_keys=True)
        base = ref_ds.Replica if cfg.dataset_format == "Replica" else ref_ds.ScanNet

        class Rec(base):
            def get_all_frames(self):
                super().get_all_frames()
                raise _Stop(self)

        try:
            Rec(cfg)
            raise RuntimeError("the reference's constructor did not call get_all_frames")
        except _Stop as stop:
            ds = stop.args[0]
        frames = list(ds.sample_dict.keys())
        s = ds.sample_dict
        np.savez_compressed(name + "_samples.npz", frames=np.array(frames),
                            image=np.stack([s[f]["image"] for f in frames]), depth=np.stack([s[f]["depth"] for f in frames]),
                            obj_mask=np.stack([s[f]["obj_mask"] for f in frames]), T=np.stack([s[f]["T"] for f in frames]),
                            frame_id=np.array([s[f]["frame_id"] for f in frames]),
                            obj_mask_dtype=np.array(str(s[frames[0]]["obj_mask"].dtype)))
        info = []
        for cls_id, d in ds.inst_dict.items():
            entry = {"cls": int(cls_id), "insts": []}
            for key, v in d.items():
                if key == "frame_info":
                    entry["frame_info"] = [[int(fi["frame"]), [int(b) for b in fi["bbox"]]] for fi in v]
                else:
                    entry["insts"].append({"inst": int(key),
                                           "frame_info": [[int(fi["frame"]), [int(b) for b in fi["bbox"]]] for fi in v["frame_info"]]})
            info.append(entry)
        with open(name + "_frames.json", "w") as f:
            json.dump({"n_img": int(ds.n_img), "inst_dict": info}, f, indent=1)
        print(name, "n_img", ds.n_img, "classes", [e["cls"] for e in info])


if __name__ == "__main__":
    main()
