"""Times orientation repair (cnr_amd.meshops.orient) on the GPU: the marching-cubes meshes of an analytic
sphere at grid_dim 64 / 128 / 256 and the ladder of tools/time_meshclean.py (10^6 faces whose indices ascend along it), each
with a random half of its faces flipped.  Per stage of meshops.orient by device events after warm-up, the two torch.sort calls
shown apart from the kernels; meshops.components (edge connectivity) on the same mesh in the same run beside it -- it shares
the key sort, the union and the flatten pass, so it is the yardstick -- and the host breadth-first restatement
(tests/meshorient_cpu.py).

    python tools/time_meshorient.py [--reps 5] [--dims 64,128,256] [--ladder 500001] [--seed 0] [--host_faces 2000000]
                                    [--out profiles/meshorient_time.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

SORTS = ("sort_edges", "sort_faces")


def summary(stages):
    total = sum(stages.values())
    sort = sum(stages[k] for k in SORTS)
    return dict(stages_ms={k: round(v, 3) for k, v in stages.items()}, ms_total=round(total, 3), ms_torch_sort=round(sort, 3),
                sort_share=round(sort / total, 3), ms_without_sort=round(total - sort, 3))


def measure(cnr, name, verts, faces, reps, seed, host_faces):
    from time_meshclean import stage_times
    import meshorient_cpu as OC
    flipped_np, mask = OC.random_flips(faces.cpu().numpy(), seed)
    flipped = torch.from_numpy(flipped_np).to(faces.device)
    V = len(verts)
    rec = dict(mesh=name, V=V, F=len(faces), flipped_in=int(mask.sum()))
    stages, out = stage_times(lambda timer: cnr.meshops.orient(flipped, V, verts, timer=timer), reps)
    rec["orient"] = summary(stages)
    rec["orient"].update(patches=out.n, n_flipped=int(out.n_flipped.sum()), not_orientable=int((~out.orientable).sum()))
    stages, table = stage_times(lambda timer: cnr.meshops.components(flipped, V, verts, connectivity="edge", timer=timer), reps)
    rec["components"] = summary(stages)
    rec["components"].update(components=table.n)
    rec["orient_over_components_without_sort"] = round(rec["orient"]["ms_without_sort"] / rec["components"]["ms_without_sort"], 3)
    rec["orient_over_components"] = round(rec["orient"]["ms_total"] / rec["components"]["ms_total"], 3)
    if len(faces) <= host_faces:
        t = time.perf_counter()
        want = OC.orient(flipped_np, V, verts.cpu().numpy())
        rec["ms_host_bfs"] = round((time.perf_counter() - t) * 1e3, 3)
        rec["host_over_orient"] = round(rec["ms_host_bfs"] / rec["orient"]["ms_total"], 1)
        rec["equal_to_host"] = bool(np.array_equal(out.faces.cpu().numpy(), want["faces"]) and
                                    np.array_equal(out.signed_volume.cpu().numpy(), want["signed_volume"]))
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dims", default="64,128,256")
    ap.add_argument("--ladder", type=int, default=500001, help="rail length: 2 (n - 1) faces")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--host_faces", type=int, default=2000000, help="the host restatement runs on meshes of at most this many faces")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import cnr_amd as cnr
    import meshops_cpu as R
    from time_meshsimplify import sphere_volume
    assert torch.cuda.is_available(), "time_meshorient needs the GPU"
    dev = torch.device("cuda:0")
    rows = []
    for D in (int(d) for d in a.dims.split(",") if d):
        verts, _, faces = cnr.vis.marching_cubes_raw(sphere_volume(D).to(dev))
        rows.append(measure(cnr, "marching cubes sphere %d^3" % D, verts, faces, a.reps, a.seed, a.host_faces))
    if a.ladder:
        v, f = R.ladder(a.ladder, "ascending")
        rows.append(measure(cnr, "ladder ascending", torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), a.reps, a.seed,
                            a.host_faces))
    if not a.out:
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, seed=a.seed, rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
