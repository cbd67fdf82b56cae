"""Renders the trained scene from one of the dataset's camera poses: builds the categories as train.py does (cameraInfo,
get_dataset, one sceneCategory per class), loads the newest checkpoint of each from --logdir, and writes rgb.png, depth.png
(16 bit, millimetres) and instance.png (16 bit, 65535 = nothing) into --out.  Two edits, neither of which touches the trained
state: --move INST tx ty tz translates an instance in world coordinates, --hide INST leaves it out.  --skip-empty builds
one occupancy grid per entity from the loaded weights (G^3 cells, a cell kept where the occupancy reaches --tau on meshing's
lattice or in a neighbouring cell) and evaluates the fields only inside the kept cells.  --normals adds normal.png (the
world-frame surface normal from the fields' own gradients, n * 0.5 + 0.5 in 8 bits), --shade also shade.png, a grey headlight
Lambert image made from it.

    python tools/render_view.py --config configs/Replica/config_replica_room0.json --logdir logs/room0 --frame 0 --out view0
        [--samples 64] [--move 12 0.3 0 0] [--hide 7] [--skip-empty [--grid 64] [--tau 1e-3]] [--normals] [--shade]"""
import argparse
import glob
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def newest_checkpoint(logdir, cls_id):
    files = sorted(glob.glob(os.path.join(logdir, "**", "cls_{}_iteration_*.pth".format(cls_id)), recursive=True),
                   key=lambda f: int(os.path.splitext(f)[0].rsplit("_", 1)[1]))
    return files[-1] if files else None


def build_scene(config, logdir, allow_pickle=False):
    """The scene as train.py builds it (cameraInfo, get_dataset, one sceneCategory per class) with the newest checkpoint of
    every class under `logdir` loaded -> (cfg, data, SceneRenderer).  tools/eval_views.py builds its scene here too."""
    import cnr_amd as cnr
    from cnr_amd.scene_cateogries import cameraInfo, sceneCategory
    cfg = cnr.cfg.Config(config)
    cam_info = cameraInfo(cfg)
    data = cnr.dataset.get_dataset(cfg)
    cls_dict, scene_bg = {}, None
    for cls_id in data.inst_dict.keys():                              # train.py:46-64
        sc = sceneCategory(cfg, cls_id, data.inst_dict[cls_id], data.sample_dict, cam_info.rays_dir_cache)
        ckpt = newest_checkpoint(logdir, cls_id)
        if ckpt is None:
            raise SystemExit("no checkpoint of class {} under {}".format(cls_id, logdir))
        sc.load_checkpoints(ckpt, allow_pickle=allow_pickle)
        if cls_id == 0:
            scene_bg = sc
        else:
            cls_dict[cls_id] = sc
    return cfg, data, cnr.view.SceneRenderer(cls_dict, scene_bg, cfg)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", required=True)
    ap.add_argument("--logdir", required=True, help="where save_checkpoints wrote cls_<id>_iteration_<n>.pth")
    ap.add_argument("--frame", type=int, default=0, help="the dataset frame whose pose is rendered")
    ap.add_argument("--out", required=True)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--move", nargs=4, action="append", default=[], metavar=("INST", "TX", "TY", "TZ"))
    ap.add_argument("--hide", type=int, action="append", default=[], metavar="INST")
    ap.add_argument("--skip-empty", action="store_true", help="skip the samples in empty cells of per-entity occupancy grids")
    ap.add_argument("--grid", type=int, default=64, metavar="G", help="cells per axis of the occupancy grids (a multiple of 4, 4 .. 128)")
    ap.add_argument("--tau", type=float, default=1e-3, metavar="T", help="a cell is kept where the occupancy reaches T")
    ap.add_argument("--normals", action="store_true", help="also write normal.png: surface normals from the field gradients")
    ap.add_argument("--shade", action="store_true", help="also write shade.png, a headlight Lambert image (implies --normals)")
    ap.add_argument("--allow-pickle", action="store_true", help="unpickle the checkpoints instead of the weights-only read: needed for a background's box object and for numpy "
                    "scalar ids (trusted files only)")
    a = ap.parse_args()
    import cnr_amd as cnr
    cfg, data, renderer = build_scene(a.config, a.logdir, a.allow_pickle)
    transforms = {}
    for inst, tx, ty, tz in a.move:
        E = np.eye(4)
        E[:3, 3] = float(tx), float(ty), float(tz)
        transforms[int(inst)] = E
    T_wc = np.asarray(data.sample_dict[a.frame]["T"], np.float64)
    if a.skip_empty:
        renderer.build_grids(resolution=a.grid, threshold=a.tau)
    with torch.no_grad():
        result = renderer.render(T_wc, n_samples=a.samples, transforms=transforms, hidden=set(a.hide), skip_empty=a.skip_empty,
                                 normals=a.normals or a.shade)
    if a.skip_empty:
        evaluated, total = renderer.active_samples
        print("evaluated {} of {} samples ({:.1%})".format(evaluated, total, evaluated / max(total, 1)))
    cnr.view.render_to_files(result, a.out)
    names = ["rgb.png", "depth.png", "instance.png"] + (["normal.png"] if "normal" in result else [])
    if a.shade:
        from PIL import Image
        grey = (cnr.view.shade(result, T_wc).clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy().transpose(1, 0, 2)
        Image.fromarray(np.ascontiguousarray(grey), "RGB").save(os.path.join(a.out, "shade.png"))
        names.append("shade.png")
    shown = sorted(int(i) for i in torch.unique(result["instance"]).tolist())
    print("wrote {} to {}; instances in view: {}".format(", ".join(names), a.out, shown))


if __name__ == "__main__":
    main()
