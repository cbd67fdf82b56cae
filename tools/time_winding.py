"""Times the generalized winding number (csrc/winding.hip, cnr_amd.metrics.winding_number) on the GPU by device events after
warm-up, the median of --reps runs with minimum and maximum, all in one process: the scenes of tools/time_pointmesh.py (200 000
area-weighted samples of a slightly larger sphere against the 256^3 marching-cubes sphere, about 442 700 faces, and against its
clipped part, about 30 000 faces); cnr_point_mesh_dist on the same inputs beside it; and what a user could do without the
kernel, the same sum in torch float64 on the device in query chunks, on a subset of the queries large enough to time, scaled
per pair.

--faces F replaces the two scenes by one of F random triangles (tests/pointmesh_cpu.random_case), for a quick run.

    python tools/time_winding.py [--reps 20] [--queries 200000] [--faces F] [--out profiles/winding_time.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

TORCH_PAIRS_PER_CHUNK = 1 << 22
TORCH_CHUNKS = 4


def _spread_ms(fn, reps):
    """-> [median, min, max] in ms of `reps` runs after one warm-up run"""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return [round(float(v), 4) for v in (np.median(times), min(times), max(times))]


def torch_winding(q, tri, step, with_bar=False):
    """the kernel's formula in torch float64 (torch's own norms, sums and their order), `step` queries at a time: q (n,3),
    tri (F,3,3) f64 corners -> w (n,) f64; with_bar=True: -> (w, bar), DESIGN.md 3.21's bar from this evaluation's own terms
    (tests/test_winding_gpu.py's large case)"""
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    F = len(tri)
    out, bars = [], []
    for s in range(0, len(q), step):
        p = q[s:s + step].double()[:, None, :]
        A, B, C = a - p, b - p, c - p
        la, lb, lc = A.norm(dim=-1), B.norm(dim=-1), C.norm(dim=-1)
        det = (A * torch.linalg.cross(B, C)).sum(-1)
        den = la * lb * lc + (A * B).sum(-1) * lc + (B * C).sum(-1) * la + (C * A).sum(-1) * lb
        nz = det != 0
        t = torch.where(nz, torch.atan2(det, den), torch.zeros_like(det))
        out.append(t.sum(1) / (2 * np.pi))
        if with_bar:
            cond = torch.where(nz, la * lb * lc / torch.where(nz, torch.hypot(det, den), torch.ones_like(det)), torch.zeros_like(det))
            bars.append(2.0 ** -52 * ((F + 16) * t.abs().sum(1) + 16 * cond.sum(1)) / (2 * np.pi))
    return (torch.cat(out), torch.cat(bars)) if with_bar else torch.cat(out)


def _row(_C, q, tri, reps):
    verts, faces, F = tri.verts, tri.faces, tri.n_faces
    N, dev = len(q), q.device
    lib = _C.load()
    row = dict(faces=F, queries=N, pairs=N * F)
    ws = torch.empty(int(lib.cnr_winding_workspace_bytes(N, F)), device=dev, dtype=torch.uint8)
    w = torch.empty(N, device=dev, dtype=torch.float64)
    row["winding_ms"] = _spread_ms(lambda: _C.call("cnr_winding_number", q, N, verts, faces, F, w, ws), reps)
    row["winding_pairs_per_s"] = float("%.4g" % (N * F / (row["winding_ms"][0] * 1e-3)))
    pws = torch.empty(int(lib.cnr_point_mesh_workspace_bytes(N, F)), device=dev, dtype=torch.uint8)
    dist, face = torch.empty(N, device=dev), torch.empty(N, device=dev, dtype=torch.int32)
    row["point_mesh_ms"] = _spread_ms(lambda: _C.call("cnr_point_mesh_dist", q, N, verts, faces, F, dist, face, None, pws), reps)
    row["point_mesh_pairs_per_s"] = float("%.4g" % (N * F / (row["point_mesh_ms"][0] * 1e-3)))
    row["winding_over_point_mesh"] = round(row["winding_ms"][0] / row["point_mesh_ms"][0], 3)
    step = max(1, min(N, TORCH_PAIRS_PER_CHUNK // F))
    sub = min(N, step * TORCH_CHUNKS)
    corners = verts.double().view(F, 3, 3) if faces is None else verts.double()[faces.long()]
    row["torch_queries"], row["torch_chunk"] = sub, step
    row["torch_ms"] = _spread_ms(lambda: torch_winding(q[:sub], corners, step), reps)
    row["torch_pairs_per_s"] = float("%.4g" % (sub * F / (row["torch_ms"][0] * 1e-3)))
    row["kernel_over_torch_per_pair"] = round(row["winding_pairs_per_s"] / row["torch_pairs_per_s"], 2)
    row["max_abs_difference_to_torch"] = float((w[:sub] - torch_winding(q[:sub], corners, step)).abs().max())
    row["mean_w"] = float(w.mean())
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--queries", type=int, default=200000)
    ap.add_argument("--faces", type=int, default=None, help="time one scene of this many random triangles instead of the two spheres")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import cnr_amd as cnr
    from cnr_amd import metrics as MT
    _C = cnr._C
    assert torch.cuda.is_available(), "time_winding needs the GPU"
    dev = torch.device("cuda:0")
    N = a.queries
    if a.faces:
        import pointmesh_cpu as P
        q, v, f = P.random_case(N, a.faces)
        scenes = (("random", torch.from_numpy(q).to(dev), cnr.devmesh.device_mesh((v, f), dev)),)
    else:
        import mc_cpu as M
        mesh = cnr.vis.marching_cubes(M.sphere(256, 0.85, 4.0))
        mesh.apply_translation([-0.5, -0.5, -0.5]).apply_scale(2.0)
        whole = cnr.devmesh.device_mesh(mesh, dev)
        clipped = MT._clip(whole, MT.box_planes(np.eye(4), [1.2, 1.2, 1.0]))
        q = MT.sample_surface(cnr.vis.Mesh(mesh.vertices * 1.02, mesh.faces), N, seed=0)
        scenes = (("mc256", q, whole), ("mc256_clipped", q, clipped))
    rows = {}
    for name, pts, tri in scenes:
        rows[name] = _row(_C, pts, tri, a.reps)
        print(name, json.dumps(rows[name]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, statistic="median, min, max", rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
