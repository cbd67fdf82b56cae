"""Times the mesh simplification (cnr_amd.meshops.simplify) on the GPU, stage by stage by device events after
warm-up: marching-cubes spheres of 64^3, 128^3 and 256^3 and a wavy sheet of 10^6 faces, two cell sizes each.  The torch.sort
calls are shown apart from the kernels; beside every row the whole of weld(cell) of the same mesh (it shares the key sort),
vertex_normals of the output (the third segment sum), the achieved bytes/s of the record and segment-sum kernels, and the numpy
restatement on the host (meshes of at most --host-faces faces: it walks the clusters in python).

    python tools/time_meshsimplify.py [--reps 5] [--dims 64,128,256] [--sheet 708] [--out profiles/meshsimplify_time.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from time_meshclean import stage_times, whole  # noqa: E402  (the per-stage and whole-call timers, shared)

SORTS = ("sort_keys", "sort_rows", "sort_corners", "sort_vertices")


def sphere_volume(D):
    g = torch.linspace(-1, 1, D)
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    return (0.5 + 4.0 * (0.7 - torch.sqrt(x * x + y * y + z * z))).clamp(0, 1)


def wavy_sheet(n):
    """n x n quads over [0, n]^2 with a height of two sines: 2 n^2 faces"""
    import meshops_cpu as R
    v, f = R.open_sheet(n, n)
    v = v.copy()
    v[:, 2] = 3.0 * np.sin(v[:, 0] * 0.05) * np.cos(v[:, 1] * 0.07)
    return v.astype(np.float32), f


def measure(cnr, S, name, verts, faces, cell, reps, host_faces):
    F, V = len(faces), len(verts)
    stages, (out_v, out_f, _, report) = stage_times(lambda timer: cnr.meshops.simplify(verts, faces, cell=cell, timer=timer), reps)
    total = sum(stages.values())
    sort = sum(stages.get(k, 0.0) for k in SORTS)
    C = report["clusters"]
    # bytes the kernels have to move at least: records = 3 indices + 9 coordinates in, 10 doubles out per face; a segment sum =
    # per position its segment id, its gather index and its K doubles, and K doubles out per segment
    b_records = F * (12 + 36 + 80)
    b_quadrics = 3 * F * (4 + 8 + 80) + C * 80
    b_positions = V * (4 + 8 + 24) + C * 24
    rec = dict(mesh=name, V=V, F=F, cell=cell, clusters=C, faces_out=report["faces_out"], vertices_out=report["vertices_out"],
               clamped=report["clamped"], stages_ms={k: round(v, 3) for k, v in stages.items()}, ms_total=round(total, 3),
               ms_torch_sort=round(sort, 3), sort_share=round(sort / total, 3), ms_kernels_and_readbacks=round(total - sort, 3),
               GBps_records=round(b_records / stages["records"] * 1e-6, 1), GBps_sum_quadrics=round(b_quadrics / stages["sum_quadrics"] * 1e-6, 1),
               GBps_sum_positions=round(b_positions / stages["sum_positions"] * 1e-6, 1))
    rec["ms_weld_cell"] = round(whole(lambda: cnr.meshops.weld(verts, faces, cell=cell), reps), 3)
    rec["ms_vertex_normals_out"] = round(whole(lambda: cnr.meshops.vertex_normals(out_v, out_f), reps), 3)
    rec["ms_vertex_normals_in"] = round(whole(lambda: cnr.meshops.vertex_normals(verts, faces), reps), 3)
    if F <= host_faces:
        v_np, f_np = verts.cpu().numpy(), faces.cpu().numpy()
        t = time.perf_counter()
        S.simplify(v_np, f_np, cell)
        rec["ms_numpy_restatement_host"] = round((time.perf_counter() - t) * 1e3, 1)
    else:
        rec["ms_numpy_restatement_host"] = None
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dims", default="64,128,256")
    ap.add_argument("--sheet", type=int, default=708, help="quads per side: 2 n^2 faces")
    ap.add_argument("--host-faces", type=int, default=200000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import cnr_amd as cnr
    import meshsimplify_cpu as S
    assert torch.cuda.is_available(), "time_meshsimplify needs the GPU"
    dev = torch.device("cuda:0")
    rows = []
    for D in (int(d) for d in a.dims.split(",") if d):
        verts, _, faces = cnr.vis.marching_cubes_raw(sphere_volume(D).to(dev))
        for voxels in (2, 4):
            rows.append(measure(cnr, S, "marching-cubes sphere %d^3" % D, verts, faces, voxels / (D - 1.0), a.reps, a.host_faces))
    if a.sheet:
        sheet = cnr.devmesh.device_mesh(wavy_sheet(a.sheet), dev)
        verts, faces = sheet.verts, sheet.faces
        for cell in (2.0, 8.0):
            rows.append(measure(cnr, S, "wavy sheet %d x %d" % (a.sheet, a.sheet), verts, faces, cell, a.reps, a.host_faces))
        # one giant cluster: every corner in ONE segment, which a single 16-lane group walks
        F = len(faces)
        items = torch.rand(F, 10, device=dev, dtype=torch.float64)
        gather = torch.arange(3 * F, device=dev)
        seg = torch.zeros(3 * F, device=dev, dtype=torch.int32)
        err = torch.zeros(1, device=dev, dtype=torch.int32)
        ms = whole(lambda: cnr.meshops._segment_sum(items, gather, 3, seg, 1, err), a.reps)
        rows.append(dict(mesh="one segment of %d corners, K = 10" % (3 * F), ms_segment_sum=round(ms, 3)))
        print(json.dumps(rows[-1]), flush=True)
    if not a.out:
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
