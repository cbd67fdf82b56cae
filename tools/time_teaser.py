"""Times the stages of category_registration.TeaserSolver at N = 10 000 correspondences on the GPU -- graph, clique, rotation +
translation (host), ICP -- on the planted construction of tests/teaser_cpu.py (160 template points; 60 kept, posed, 2 mm noise,
plus 20 unrelated points), and the whole TeaserSolver beside IcpSolver on the same two clouds in the same run.  The graph
and the clique launches (cnr_teaser_graph, cnr_clique_search with its buffers ready) are timed by device events; the *_call_ms
rows are host wall-clock around the Python stage functions, which allocate, sort and synchronise (max_clique reads the largest
degree before and the result after the launches).  Last, both GPU solvers through align_poses on the class of
tests/test_teaser_gpu.py (teaser_cpu.registration_case) with their pose errors.

    python tools/time_teaser.py [--reps 5] [--out profiles/teaser_time.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _wall_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / reps


def _event_ms(fn, reps):
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "teaser_time.json"))
    a = ap.parse_args()
    import cnr_amd as cnr
    import teaser_cpu as TC
    CR = cnr.category_registration
    assert torch.cuda.is_available(), "time_teaser needs the GPU"
    dev = torch.device("cuda:0")
    c = TC.planted_case(11, n_template=160, max_correspondences=10000)
    solver = CR.TeaserSolver(voxel_size=0.02)
    rows = {"case": "teaser_cpu.planted_case(11, n_template=160, max_correspondences=10000), voxel_size 0.02"}

    src, tmpl = c["source"], c["template"]
    A, B, src_ds, tgt_ds, _ = CR.teaser_correspondences(src, tmpl, 0.02, 10000, np.random.default_rng(0), dev)
    rows["N"] = len(A)
    rows["correspondences_ms"] = round(_wall_ms(lambda: CR.teaser_correspondences(src, tmpl, 0.02, 10000, np.random.default_rng(0), dev), a.reps), 3)
    adj, deg = CR.compatibility_graph(A, B)
    rows["edges"], rows["max_degree"], rows["mean_degree"] = int(deg.sum()) // 2, int(deg.max()), round(float(deg.float().mean()), 1)
    _C, N = cnr._C, len(A)
    thr = CR.compatibility_threshold()
    rows["graph_ms"] = round(_event_ms(lambda: _C.call("cnr_teaser_graph", A, B, N, thr, adj, deg), a.reps), 4)
    rows["graph_call_ms"] = round(_wall_ms(lambda: CR.compatibility_graph(A, B), a.reps), 3)
    clique, info = CR.max_clique(adj, deg)
    rows["clique"] = info
    order, max_degree = CR.clique_order(deg), int(deg.max())
    ws = torch.empty(int(_C.load().cnr_clique_workspace_bytes(N, max_degree)), device=dev, dtype=torch.uint8)
    out, inf = torch.zeros(max_degree + 1, device=dev, dtype=torch.int32), torch.zeros(8, device=dev, dtype=torch.int64)
    rows["clique_workspace_mb"] = round(ws.numel() / 2 ** 20, 1)
    rows["clique_ms"] = round(_event_ms(lambda: _C.call("cnr_clique_search", adj, order, N, max_degree, CR.DEFAULT_SEARCH_BUDGET, ws,
                                                        out, inf), a.reps), 4)
    assert np.array_equal(out[:info["size"]].cpu().numpy(), clique)
    rows["clique_call_ms"] = round(_wall_ms(lambda: CR.max_clique(adj, deg), a.reps), 3)
    members = torch.from_numpy(clique).to(dev)
    T0, its = solver.solve_pose(A, B, members)
    rows["gnc_iterations"] = its
    rows["rotation_translation_host_ms"] = round(_wall_ms(lambda: solver.solve_pose(A, B, members), a.reps), 3)
    icp = lambda: CR.icp_device(src_ds.points_device, tgt_ds.points_device, T0[None], solver.noise_bound, solver.icp_max_iteration)
    rows["icp_updates"] = int(icp()[1][0, 3])
    rows["icp_ms"] = round(_wall_ms(icp, a.reps), 3)

    s = torch.from_numpy(src.T[None].copy()).to(dev)
    t = torch.from_numpy(tmpl.T[None].copy()).to(dev)
    want = np.linalg.inv(c["pose"])
    for name, sv in (("TeaserSolver", solver), ("IcpSolver", CR.IcpSolver())):
        R, tr = sv(s, t)
        cosine = (np.trace(R[0].numpy().T @ want[:3, :3]) - 1) / 2
        rows[name] = dict(ms=round(_wall_ms(lambda: sv(s, t), a.reps), 3),
                          rotation_error_deg=round(float(np.degrees(np.arccos(np.clip(cosine, -1, 1)))), 4),
                          translation_error_m=round(float(np.linalg.norm(tr[0].numpy().reshape(3) - want[:3, 3])), 5))
    import registration_cpu as RC
    rows["class_case"] = "teaser_cpu.registration_case(): pose errors per copy (degrees, metres) of each GPU solver through align_poses"
    for name, make in (("TeaserSolver", lambda: CR.TeaserSolver(voxel_size=TC.REG_VOXEL, max_correspondences=TC.REG_MAX_CORR)),
                       ("IcpSolver", lambda: CR.IcpSolver())):
        clouds, poses, counts = TC.registration_case()
        d = RC.build_dicts(clouds, counts, lambda p: cnr.utils.PointCloud(p, device=dev))
        try:
            seen = CR.align_poses(*d, name="replica", device=str(dev), solver=make())
        except ValueError as e:          # e.g. a cloud the solver cannot frame
            rows["class_" + name] = dict(error=str(e))
            continue
        rows["class_" + name] = dict(classes={str(c): list(m.keys()) for c, m in d[0].items()},
                                     errors={str(k): [round(v[0], 4), round(v[1], 5)] for k, v in RC.pose_errors(d[0], poses).items()},
                                     chamfer={str(k): round(float(v), 4) for k, v in seen["chamfer"][7].items()})
    print(json.dumps(rows), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
