"""Times the mesh clean-up (cnr_amd.meshops) on the GPU: the marching-cubes meshes of tools/time_meshing.py
(one trained CodeNeRF object at grid_dim 64 / 128 / 256) and a ladder of 10^6 faces whose indices ascend along it (the chain
a plain find would walk), in both connectivities.  Per stage of meshops.components by device events after warm-up, the two
torch.sort calls shown apart from the kernels, the whole of components / compact / weld, and scipy's connected_components on
the host (graph construction included) beside them.

    python tools/time_meshclean.py [--steps 400] [--reps 5] [--dims 64,128,256] [--ladder 500001] [--out profiles/meshclean_time.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SORTS = ("sort_edges", "sort_faces")


def stage_times(call, reps):
    """({stage: ms}, the result) of call(timer) -- meshops.components here, meshops.simplify in tools/time_meshsimplify.py -- as
    the mean over reps after one warm-up call"""
    acc = {}
    for rep in range(reps + 1):
        marks = []

        def timer(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((name, e))
        start = torch.cuda.Event(enable_timing=True)
        start.record()
        out = call(timer)
        torch.cuda.synchronize()
        if rep == 0:
            continue
        prev = start
        for name, e in marks:
            acc[name] = acc.get(name, 0.0) + prev.elapsed_time(e)
            prev = e
    return {k: v / reps for k, v in acc.items()}, out


def whole(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def scipy_ms(faces_np, n_vertices):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    t = time.perf_counter()
    f = faces_np.astype(np.int64)
    rows, cols = np.concatenate([f[:, 0], f[:, 0]]), np.concatenate([f[:, 1], f[:, 2]])
    g = sp.coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n_vertices, n_vertices))
    n, _ = connected_components(g, directed=False)
    return (time.perf_counter() - t) * 1e3, int(n)


def measure(cnr, name, verts, faces, reps):
    rec = dict(mesh=name, V=len(verts), F=len(faces))
    faces_np = faces.cpu().numpy()
    rec["ms_scipy_vertex_host"], rec["scipy_components"] = (round(x, 3) if isinstance(x, float) else x for x in scipy_ms(faces_np, len(verts)))
    for conn in ("edge", "vertex"):
        stages, table = stage_times(lambda timer: cnr.meshops.components(faces, len(verts), verts, connectivity=conn, timer=timer), reps)
        total = sum(stages.values())
        sort = sum(stages[k] for k in SORTS)
        rec[conn] = dict(components=table.n, stages_ms={k: round(v, 3) for k, v in stages.items()}, ms_total=round(total, 3),
                         ms_torch_sort=round(sort, 3), sort_share=round(sort / total, 3), ms_kernels_and_readbacks=round(total - sort, 3))
    keep = (torch.arange(len(faces), device=faces.device) % 3 != 0)
    rec["ms_compact"] = round(whole(lambda: cnr.meshops.compact(faces, len(verts), keep), reps), 3)
    soup = verts[faces.long()].contiguous()
    rec["ms_weld_exact_soup"] = round(whole(lambda: cnr.meshops.weld(soup), reps), 3)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dims", default="64,128,256")
    ap.add_argument("--ladder", type=int, default=500001, help="rail length: 2 (n - 1) faces")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import cnr_amd as cnr
    import meshops_cpu as R
    assert torch.cuda.is_available(), "time_meshclean needs the GPU"
    dev = torch.device("cuda:0")
    rows = []
    if a.dims:
        from time_meshing import trained_trainer
        t = trained_trainer(cnr, dev, a.steps)
        for D in (int(d) for d in a.dims.split(",")):
            mesh = t.meshing(2, grid_dim=D)
            d = cnr.devmesh.device_mesh(mesh, dev)
            rows.append(measure(cnr, "marching cubes %d^3" % D, d.verts, d.faces, a.reps))
    if a.ladder:
        for order in ("ascending", "shuffled"):
            v, f = R.ladder(a.ladder, order)
            rows.append(measure(cnr, "ladder %s" % order, torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), a.reps))
    if not a.out:
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(dict(device=torch.cuda.get_device_name(0), steps=a.steps, reps=a.reps, rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
