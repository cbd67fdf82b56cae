"""Scores rendered views of the trained scene against the sequence's frames: the scene is built as tools/render_view.py builds
it (its build_scene), the chosen frames' poses are rendered, and cnr_amd.image_metrics.evaluate_views compares rgb, depth and
instance with the frame's image, depth and obj_mask -- PSNR, SSIM, depth L1 in metres and mask IoU per instance and for the
whole image.  Prints the table and writes it, with the per-frame values, as JSON.

--against-unskipped scores the --skip-empty render against the full render of the same pose instead of the frames: the error
that empty-space skipping makes, which a grid with every cell set makes exactly zero (PSNR inf).

    python tools/eval_views.py --config CFG --logdir LOGS --frames a:b:step [--samples 64]
        [--skip-empty [--grid 64] [--tau 1e-3]] [--against-unskipped] [--batch 4] [--out scores.json]"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def _render_view():
    """tools/render_view.py as a module (tools/ is a directory of scripts, not a package)"""
    spec = importlib.util.spec_from_file_location("render_view_tool", os.path.join(ROOT, "tools", "render_view.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def frame_slice(text, n):
    """'a:b:step' (python slice syntax, parts may be empty) or a single index -> the list of frame indices below n"""
    parts = text.split(":")
    if len(parts) == 1:
        return [range(n)[int(parts[0])]]
    if len(parts) > 3:
        raise SystemExit("--frames wants a:b:step, not {!r}".format(text))
    return list(range(n)[slice(*[int(p) if p.strip() else None for p in parts])])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", required=True)
    ap.add_argument("--logdir", required=True, help="where save_checkpoints wrote cls_<id>_iteration_<n>.pth")
    ap.add_argument("--frames", default="::1", metavar="a:b:step", help="the dataset frames to score, as a python slice")
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--skip-empty", action="store_true", help="render with per-entity occupancy grids")
    ap.add_argument("--grid", type=int, default=64, metavar="G")
    ap.add_argument("--tau", type=float, default=1e-3, metavar="T")
    ap.add_argument("--against-unskipped", action="store_true", help="score the --skip-empty render against the full render")
    ap.add_argument("--batch", type=int, default=4, help="frames per scoring launch")
    ap.add_argument("--out", default=None, help="the JSON file")
    ap.add_argument("--allow-pickle", action="store_true", help="as tools/render_view.py")
    a = ap.parse_args()
    if a.against_unskipped and not a.skip_empty:
        raise SystemExit("--against-unskipped compares the --skip-empty render with the full one: give --skip-empty too")
    import cnr_amd as cnr
    cfg, data, renderer = _render_view().build_scene(a.config, a.logdir, a.allow_pickle)
    keys = sorted(data.sample_dict.keys())
    chosen = [keys[i] for i in frame_slice(a.frames, len(keys))]
    if not chosen:
        raise SystemExit("--frames {} selects no frame of {}".format(a.frames, len(keys)))
    if a.skip_empty:
        renderer.build_grids(resolution=a.grid, threshold=a.tau)

    def render(skip):
        def fn(T_wc):
            with torch.no_grad():
                return renderer.render(np.asarray(T_wc, np.float64), n_samples=a.samples, skip_empty=skip)
        return fn

    frames = [data.sample_dict[k] for k in chosen]
    scores = cnr.image_metrics.evaluate_views(render(a.skip_empty), frames, batch=a.batch,
                                              reference_fn=render(False) if a.against_unskipped else None)
    print(cnr.image_metrics.format_table(scores))
    if a.out:
        rec = dict(config=a.config, frame_ids=[int(k) for k in chosen], samples=a.samples, skip_empty=a.skip_empty,
                   grid=a.grid if a.skip_empty else None, tau=a.tau if a.skip_empty else None,
                   against="unskipped render" if a.against_unskipped else "dataset frames", **scores.to_json())
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
