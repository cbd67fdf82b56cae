"""Fits the codes of one instance to a trained, frozen category (code_fit.CodeFitter): the category's checkpoint comes from a
training run's log directory, the instance's pose from the dataset's registration result, its ray pool from the crops of the given
frames -- the partially observed case -- and every start is optimised in the same launches.

    python tools/fit_codes.py --config CFG.json --logdir LOGS --inst I [--frames a:b] [--starts mean,objects] [--iters 500]
                              [--rays 120] [--seed 0] [--mesh OUT.obj] [--grid 128] [--clean keep_largest=1,...]
                              [--simplify cell=0.02,...]

--starts: a comma list of mean | objects | randomM (M random starts).  Prints the score of every start before and after, writes
LOGS/codes_<I>.pt = {inst_id, cls_id, start, score, shape_code, texture_code, scores, codes (M,2,L)} and, with --mesh, the mesh
of the best start (the category's checkpoint stays as it is); --clean (default off) hands Trainer.meshing the options of
cnr_amd.meshops.clean_mesh as name=value pairs, so floaters are dropped before the colour pass; --simplify (default off) the
options of cnr_amd.meshops.simplify (cell=... or target_faces=..., placement=...), applied after --clean and before the colours."""
import argparse
import glob
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_starts(text):
    out = []
    for word in text.split(","):
        word = word.strip()
        if word.startswith("random"):
            out.append(("random", int(word[6:] or 1)))
        elif word in ("mean", "objects"):
            out.append(word)
        else:
            raise SystemExit(f"--starts: {word!r} is none of mean, objects, randomM")
    return out


def latest_checkpoint(logdir, cls_id):
    files = sorted(glob.glob(os.path.join(logdir, "ckpt", f"cls_{cls_id}_iteration_*.pth")) +
                   glob.glob(os.path.join(logdir, f"cls_{cls_id}_iteration_*.pth")))
    if not files:
        raise SystemExit(f"no cls_{cls_id}_iteration_*.pth under {logdir} or {logdir}/ckpt")
    return files[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True)
    ap.add_argument("--logdir", required=True)
    ap.add_argument("--inst", type=int, required=True)
    ap.add_argument("--frames", default=None, help="a:b -- only crops of the frames a <= frame < b")
    ap.add_argument("--starts", default="mean,objects")
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--rays", type=int, default=None, help="rays per step (default: render.n_per_optim)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--mesh", default=None)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--clean", default=None, help="drop floaters first: clean_mesh options as name=value,... e.g. keep_largest=1,min_faces=20 (default: off)")
    ap.add_argument("--simplify", default=None, help="simplify the mesh: simplify options as name=value,... e.g. cell=0.02 or target_faces=20000 (default: off)")
    a = ap.parse_args()
    import cnr_amd as cnr
    from cnr_amd.code_fit import CodeFitter, load_category
    assert torch.cuda.is_available(), "fit_codes needs the GPU"
    cfg = cnr.cfg.Config(a.config)
    ds = cnr.dataset.get_dataset(cfg)
    found = [(cls_id, key, e) for cls_id, d in ds.inst_dict.items() if cls_id != 0 for key, e in d.items() if int(key) == a.inst]
    if not found:
        raise SystemExit(f"instance {a.inst} is not in the dataset's registration result")
    cls_id, key, entry = found[0]
    trainer = load_category(cfg, latest_checkpoint(a.logdir, int(cls_id)))
    frames = None
    if a.frames:
        lo, hi = (int(v) for v in a.frames.split(":"))
        frames = [fi["frame"] for fi in entry["frame_info"] if lo <= int(fi["frame"]) < hi]
    pools = CodeFitter.pools_from_dataset(ds, cfg, {key: np.asarray(entry["T_obj"])}, frames=frames)
    inst = dict(inst_id=a.inst, cls_id=int(cls_id), pool=pools[key])
    fit = CodeFitter(cfg, {int(cls_id): trainer}, [inst], starts=parse_starts(a.starts), rays_per_step=a.rays, seed=a.seed)
    print("instance %d of class %d: %d rows from %s frames, %d starts, %d rays x %d samples per step"
          % (a.inst, cls_id, fit.rows[0], "all" if frames is None else len(frames), fit.K, fit.R, fit.S), flush=True)
    before = fit.score().cpu()
    fit.run(a.iters)
    after = fit.score().cpu()
    for k in range(fit.K):
        print("start %3d  score %.5f -> %.5f  flags %d" % (k, before[k], after[k], int(fit.flags[k])))
    k, shape_code, texture_code = fit.best(a.inst)
    out = os.path.join(a.logdir, "codes_%d.pt" % a.inst)
    torch.save(dict(inst_id=a.inst, cls_id=int(cls_id), start=k, score=float(after[k]), shape_code=shape_code.cpu(),
                    texture_code=texture_code.cpu(), scores=after, codes=fit.codes(a.inst).cpu()), out)
    print("best start %d, score %.5f -> %s" % (k, after[k], out))
    if a.mesh:
        box = entry.get("bbox3D")
        if box is None:
            raise SystemExit(f"--mesh: instance {a.inst} has no bbox3D in the registration result, and meshing needs its extent")
        fit.attach(trainer, a.inst, extent=np.asarray(box.extent))
        mesh = trainer.meshing(a.inst, grid_dim=a.grid, clean=cnr.meshops.parse_clean_options(a.clean) if a.clean else None,
                               simplify=cnr.meshops.parse_simplify_options(a.simplify) if a.simplify else None)
        if mesh is None:
            print("no surface at 0.5 occupancy: no mesh written")
        else:
            mesh.export(a.mesh)
            print(a.mesh)


if __name__ == "__main__":
    main()
