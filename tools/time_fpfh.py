"""Times the stages of TEASER's FPFH mode on the GPU by device events -- the hybrid search, the normals, SPFH, FPFH (each with its
inputs ready) and the two descriptor nearest-neighbour launches of mutual_correspondences -- on two clouds voxel-down-sampled
to about 2 000 and about 50 000 points: the chair of tests/registration_cpu.py and a posed, noisy copy, sampled densely and
down-sampled at the voxel size that leaves about that many points.  The *_call_ms rows are host wall-clock around the Python
functions (they sort, allocate and synchronise).

    python tools/time_fpfh.py [--reps 10] [--out profiles/fpfh_time.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


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


def _wall_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / reps


def _down_to(cloud, target, lo=0.001, hi=0.2):
    """the voxel size (by bisection) at which the cloud down-samples to about `target` points -> (voxel, cloud)"""
    for _ in range(30):
        mid = (lo + hi) / 2
        n = len(cloud.voxel_down_sample(mid))
        if abs(n - target) <= 0.01 * target:
            break
        lo, hi = (mid, hi) if n > target else (lo, mid)
    return mid, cloud.voxel_down_sample(mid)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpfh_time.json"))
    a = ap.parse_args()
    import cnr_amd as cnr
    import registration_cpu as RC
    assert torch.cuda.is_available(), "time_fpfh needs the GPU"
    dev = torch.device("cuda:0")
    CR, U, _C = cnr.category_registration, cnr.utils, cnr._C
    rng = np.random.default_rng(5)
    local = RC.chair(rng, 2_000_000)
    P = RC._pose(rng, 1)
    copy = (local[rng.permutation(len(local))[:1_500_000]] + 0.002 * rng.standard_normal((1_500_000, 3))) @ P[:3, :3].T + P[:3, 3]
    rows = {"case": "registration_cpu.chair, 2 000 000 points, and a posed copy of 1 500 000 of them with 2 mm noise", "sizes": {}}
    for target in (2000, 50000):
        voxel, tgt = _down_to(U.PointCloud(local, device=dev), target)
        src = U.PointCloud(copy, device=dev).voxel_down_sample(voxel)
        r = {"voxel_size": round(voxel, 5), "n_tgt": len(tgt), "n_src": len(src)}
        pts, n = tgt.points_device, len(tgt)
        for what, radius, max_nn in (("normals", 2 * voxel, 30), ("features", 5 * voxel, 100)):
            perm, skeys, cells, starts = U._radius_cell_tables(pts, radius)
            idx = torch.empty(n, max_nn, device=dev, dtype=torch.int32)
            d2 = torch.empty(n, max_nn, device=dev, dtype=torch.float64)
            count = torch.empty(n, device=dev, dtype=torch.int32)
            search = lambda: _C.call("cnr_hybrid_search", pts, n, perm, skeys, cells, starts, len(cells), float(radius), max_nn, idx, d2, count)
            r["hybrid_search_%s_ms" % what] = round(_event_ms(search, a.reps), 4)
            r["hybrid_search_%s_call_ms" % what] = round(_wall_ms(lambda: U.hybrid_search(pts, radius, max_nn), a.reps), 3)
            r["mean_neighbours_%s" % what] = round(float(count.float().mean()), 1)
            if what == "normals":
                c = U.sequential_centroid(pts)
                nrm = torch.empty(n, 3, device=dev, dtype=torch.float64)
                r["estimate_normals_ms"] = round(_event_ms(lambda: _C.call("cnr_estimate_normals", pts, n, idx, count, max_nn, float(c[0]),
                                                                           float(c[1]), float(c[2]), nrm), a.reps), 4)
            else:
                spfh = torch.empty(n, 33, device=dev, dtype=torch.float64)
                fpfh = torch.empty(n, 33, device=dev, dtype=torch.float64)
                r["spfh_ms"] = round(_event_ms(lambda: _C.call("cnr_spfh", pts, nrm, n, idx, count, max_nn, spfh), a.reps), 4)
                r["fpfh_ms"] = round(_event_ms(lambda: _C.call("cnr_fpfh", spfh, n, idx, d2, count, max_nn, fpfh), a.reps), 4)
        f_t = CR.extract_fpfh_device(tgt, voxel).float().contiguous()
        f_s = CR.extract_fpfh_device(src, voxel).float().contiguous()
        r["extract_fpfh_call_ms"] = round(_wall_ms(lambda: CR.extract_fpfh_device(tgt, voxel), a.reps), 3)
        index = torch.empty(len(f_s), device=dev, dtype=torch.int32)
        dist = torch.empty(len(f_s), device=dev, dtype=torch.float32)
        ws = _C.workspace(_C.load().cnr_feature_nn_workspace_bytes(len(f_s), len(f_t)), dev, "cnr_feature_nn")
        r["feature_nn_ms"] = round(_event_ms(lambda: _C.call("cnr_feature_nn", f_s, len(f_s), f_t, len(f_t), 33, index, dist, ws), a.reps), 4)
        r["feature_nn_pairs_per_s"] = float("%.3g" % (len(f_s) * len(f_t) / (r["feature_nn_ms"] * 1e-3)))
        i0, _ = CR.mutual_correspondences(f_s, f_t)
        r["mutual_correspondences"] = len(i0)
        r["mutual_correspondences_call_ms"] = round(_wall_ms(lambda: CR.mutual_correspondences(f_s, f_t), a.reps), 3)
        rows["sizes"][str(target)] = r
    print(json.dumps(rows), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
