"""The classical baseline of a sequence: per instance the triangle mesh of the plain TSDF fusion of its masked depth
(cnr_amd.utils.accumulate_mesh_tsdf), written under the names tools/eval_3d_obj.py reads, so the fusion baseline
is scored by the same command as the trained meshes.

    python tools/tsdf_mesh.py --config CFG --out DIR [--inst ID ...] [--voxel 0.01] [--iteration 10000]
                                 [--clean keep_largest=1,...] [--simplify cell=0.02,...]

The sequence is loaded with get_dataset (a cached registration result gives inst_dict; its frame_info names every instance's
frames).  Without --inst every instance is fused, the background (id 0) included.  Written: DIR/iteration_<IT>_obj<ID>.obj;
printed: one JSON line per object with V, F, units and seconds.  An instance whose volume has no triangle is reported and
skipped.  --clean (default off) drops floaters before the file is written: the options of cnr_amd.meshops.clean_mesh as
name=value pairs (weld=0 also welds the seams between separately fused volumes).  --simplify (default off) then makes the
mesh smaller: the options of cnr_amd.meshops.simplify_mesh as name=value pairs (cell=... or target_faces=..., placement=...)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def instances(inst_dict):
    """inst_dict -> {instance id: frame_info}; the background is id 0"""
    out = {}
    for cls_id, entry in inst_dict.items():
        if int(cls_id) == 0:
            out[0] = entry["frame_info"]
        else:
            for inst_id, e in entry.items():
                out[int(inst_id)] = e["frame_info"]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--inst", type=int, nargs="*", default=None)
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--iteration", type=int, default=10000)
    ap.add_argument("--clean", default=None, help="drop floaters first: clean_mesh options as name=value,... e.g. keep_largest=1,min_faces=20 (default: off)")
    ap.add_argument("--simplify", default=None, help="simplify before writing: simplify_mesh options as name=value,... e.g. cell=0.02 or target_faces=100000 (default: off)")
    a = ap.parse_args(argv)
    import torch

    import cnr_amd as cnr
    cfg = cnr.cfg.Config(a.config)
    ds = cnr.dataset.get_dataset(cfg)
    frames_of = instances(ds.inst_dict)
    wanted = sorted(frames_of) if not a.inst else a.inst
    missing = [i for i in wanted if i not in frames_of]
    if missing:
        raise SystemExit(f"no instance {missing} in the sequence (it has {sorted(frames_of)})")
    os.makedirs(a.out, exist_ok=True)
    clean = cnr.meshops.parse_clean_options(a.clean) if a.clean else None
    simplify = cnr.meshops.parse_simplify_options(a.simplify) if a.simplify else None
    for inst_id in wanted:
        t = time.perf_counter()
        row = dict(obj=inst_id, frames=len(frames_of[inst_id]))
        try:
            mesh = cnr.utils.accumulate_mesh_tsdf(inst_id, frames_of[inst_id], ds.sample_dict, ds.intrinsic_open3d, voxel_size=a.voxel,
                                                  depth_scale=cfg.depth_scale, max_depth=cfg.max_depth)
        except ValueError as e:
            print(json.dumps(dict(row, skipped=str(e))), flush=True)
            continue
        units = mesh.units
        if clean is not None:
            mesh, report = cnr.meshops.clean_mesh(mesh, **clean)
            row.update(components=report["n_components"], kept=report["n_kept"])
        if simplify is not None:
            mesh, report = cnr.meshops.simplify_mesh(mesh, **simplify)
            row.update(cell=report["cell"], clusters=report["clusters"], faces_in=report["faces_in"])
        path = mesh.export(os.path.join(a.out, "iteration_%d_obj%d.obj" % (a.iteration, inst_id)))
        torch.cuda.synchronize()
        print(json.dumps(dict(row, V=len(mesh.vertices), F=len(mesh.faces), units=units, seconds=round(time.perf_counter() - t, 3),
                              file=path)), flush=True)


if __name__ == "__main__":
    main()
