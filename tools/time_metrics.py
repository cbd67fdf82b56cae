"""Times the mesh-evaluation stages (csrc/metric.hip, cnr_amd.metrics) on the GPU by device events after warm-up:
cnr_nn_dist at 10k x 10k and 200k x 200k (with its pairs/s), cnr_dist_stats at 200k, and on a 256^3 marching-cubes sphere
the area scan, 200k samples and the box clip; then one whole calc_3d_metric at N = 200 000.

    python tools/time_metrics.py [--reps 20] [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import cnr_amd as cnr
    import mc_cpu as M
    from cnr_amd import metrics as MT
    _C = cnr._C
    assert torch.cuda.is_available(), "time_metrics needs the GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rows = {}
    for n in (10000, 200000):
        q = torch.rand(n, 3, device=dev, generator=g) * 4 + 2     # scene coordinates of metres
        p = torch.rand(n, 3, device=dev, generator=g) * 4 + 2
        ws = torch.empty(int(_C.load().cnr_nn_workspace_bytes(n, n)), device=dev, dtype=torch.uint8)
        out = torch.empty(n, device=dev)
        ms = _ms(lambda: _C.call("cnr_nn_dist", q, n, p, n, out, ws), a.reps)
        rows["nn_%dk" % (n // 1000)] = dict(ms=round(ms, 4), pairs_per_s=float("%.4g" % (n * n / (ms * 1e-3))))
        print("nn %d x %d: %.4f ms, %.3g pairs/s" % (n, n, ms, n * n / (ms * 1e-3)), flush=True)
    s_ws = torch.empty(int(_C.load().cnr_dist_stats_workspace_bytes(200000)), device=dev, dtype=torch.uint8)
    s_sum, s_cnt = torch.empty(1, device=dev, dtype=torch.float64), torch.empty(1, device=dev, dtype=torch.int64)
    rows["dist_stats_200k_ms"] = round(_ms(lambda: _C.call("cnr_dist_stats", out, 200000, 0.05, s_ws, s_sum, s_cnt), a.reps), 4)

    mesh = cnr.vis.marching_cubes(M.sphere(256, 0.85, 4.0))
    mesh.apply_translation([-0.5, -0.5, -0.5]).apply_scale(2.0)
    tri = cnr.devmesh.device_mesh(mesh, dev)
    verts, faces, F = tri.verts, tri.faces, tri.n_faces
    rows["mc256_faces"] = F
    fa_ws = torch.empty(int(_C.load().cnr_face_area_workspace_bytes(F)), device=dev, dtype=torch.uint8)
    area, cum = torch.empty(F, device=dev, dtype=torch.float64), torch.empty(F, device=dev, dtype=torch.float64)
    rows["area_scan_ms"] = round(_ms(lambda: _C.call("cnr_face_area_scan", verts, faces, F, fa_ws, area, cum), a.reps), 4)
    N = 200000
    u = torch.from_numpy(np.random.default_rng(0).random((N, 3))).to(dev)
    pts = torch.empty(N, 3, device=dev)
    rows["sample_200k_ms"] = round(_ms(lambda: _C.call("cnr_sample_surface", verts, faces, F, cum, u, N, pts), a.reps), 4)
    T = np.eye(4)
    planes = torch.from_numpy(MT.box_planes(T, [1.2, 1.2, 1.0])).to(dev)      # cuts the sphere of radius 0.85
    cl_ws = torch.empty(int(_C.load().cnr_clip_box_workspace_bytes(F)), device=dev, dtype=torch.uint8)
    cnt = torch.empty(1, device=dev, dtype=torch.int64)
    rows["clip_count_ms"] = round(_ms(lambda: _C.call("cnr_clip_box_count", verts, faces, F, planes, cl_ws, cnt), a.reps), 4)
    Tn = int(cnt.item())
    tris = torch.empty(Tn, 3, 3, device=dev)
    rows["clip_emit_ms"] = round(_ms(lambda: _C.call("cnr_clip_box_emit", verts, faces, F, planes, cl_ws, tris), a.reps), 4)
    rows["clip_triangles"] = Tn
    gt = cnr.vis.Mesh(mesh.vertices * 1.02, mesh.faces)
    rows["calc_3d_metric_200k_ms"] = round(_ms(lambda: MT.calc_3d_metric(mesh, gt, N=N), max(2, a.reps // 5)), 3)
    rows["calc_3d_metric_200k"] = MT.calc_3d_metric(mesh, gt, N=N)
    print(json.dumps(rows), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
