"""Times the point-to-mesh distance (csrc/point_mesh.hip, cnr_amd.metrics.point_mesh_distance) on the GPU by device events
after warm-up, the median of --reps runs: 200 000 area-weighted samples of a slightly larger sphere against the 256^3
marching-cubes sphere of tools/time_metrics.py (about 442 700 faces) and against its clipped part (about 30 000 faces); the
record, partial and finish passes apart and together, with pairs/s; cnr_nn_dist at 200k x 200k beside it; and the numpy
restatement (tests/pointmesh_cpu.py) on the CPU at a size it can finish.

--index (default off) adds, for each of the two cases and for an adverse third one (the queries within 1e-3 r of the sphere's
centre: every tile is equidistant and nothing can be culled), the tile-box index (csrc/point_mesh_index.hip,
metrics.MeshIndex) beside the brute force of the same run: the build (keys / sort / records + tiles) and the query (keys /
sort / kernel) leg by leg, each as median, minimum and maximum, the share of tiles visited, and whether the two results are equal.

    python tools/time_pointmesh.py [--reps 20] [--out profiles/pointmesh_time.json]
    python tools/time_pointmesh.py --index [--out profiles/pointmesh_index_time.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _median_ms(fn, reps):
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
    return float(np.median(times))


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


def _index_row(_C, MT, q, tri, reps):
    """the index's legs and the brute force on the same queries and mesh, one after the other in this process"""
    verts, faces, F = tri.verts, tri.faces, tri.n_faces
    N, dev = len(q), q.device
    lib = _C.load()
    dist, face = torch.empty(N, device=dev), torch.empty(N, device=dev, dtype=torch.int32)
    near = torch.empty(N, 3, device=dev)
    ws = torch.empty(int(lib.cnr_point_mesh_workspace_bytes(N, F)), device=dev, dtype=torch.uint8)
    row = dict(faces=F, queries=N)
    row["brute_ms"] = _spread_ms(lambda: _C.call("cnr_point_mesh_dist", q, N, verts, faces, F, dist, face, near, ws), reps)
    ix = MT.MeshIndex(tri, check=False)
    keys = torch.empty(F, device=dev, dtype=torch.int32)
    row["build_keys_ms"] = _spread_ms(lambda: _C.call("cnr_pm_index_keys", verts, faces, F, ix.bbox, keys), reps)
    row["build_sort_ms"] = _spread_ms(lambda: torch.sort(keys, stable=True), reps)
    order = torch.sort(keys, stable=True).indices
    row["build_records_tiles_ms"] = _spread_ms(lambda: _C.call("cnr_pm_index_build", verts, faces, F, keys, order, ix.index), reps)
    row["build_ms"] = _spread_ms(lambda: MT.MeshIndex(tri, check=False), reps)
    qkeys = torch.empty(N, device=dev, dtype=torch.int32)
    row["query_keys_ms"] = _spread_ms(lambda: _C.call("cnr_pm_query_keys", q, N, ix.bbox, qkeys), reps)
    row["query_sort_ms"] = _spread_ms(lambda: torch.sort(qkeys, stable=True), reps)
    qorder = torch.sort(qkeys, stable=True).indices
    iws = torch.empty(int(lib.cnr_point_mesh_indexed_workspace_bytes(N, F)), device=dev, dtype=torch.uint8)
    d2, f2, n2 = torch.empty_like(dist), torch.empty_like(face), torch.empty_like(near)
    row["query_kernel_ms"] = _spread_ms(
        lambda: _C.call("cnr_point_mesh_dist_indexed", q, N, qkeys, qorder, ix.index, F, d2, f2, n2, iws), reps)
    row["query_ms"] = _spread_ms(lambda: ix._query(q, closest=True), reps)      # keys + sort + kernel, with its allocations
    st = ix.query(q, stats=True)[2]
    pairs = st["tiles_visited"] * st["tile_faces"] * st["group_queries"]
    row.update(st, visited_share=round(st["tiles_visited"] / (st["groups"] * st["tiles"]), 6), pairs_evaluated=pairs,
               pairs_brute=N * F, pairs_ratio=round(N * F / pairs, 2), speedup=round(row["brute_ms"][0] / row["query_ms"][0], 3),
               equal=bool(torch.equal(dist, d2) and torch.equal(face, f2) and torch.equal(near, n2)))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--queries", type=int, default=200000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--index", action="store_true", help="also time the tile-box index beside the brute force (default: off)")
    a = ap.parse_args()
    import cnr_amd as cnr
    import mc_cpu as M
    import pointmesh_cpu as P
    from cnr_amd import metrics as MT
    _C = cnr._C
    assert torch.cuda.is_available(), "time_pointmesh needs the GPU"
    dev = torch.device("cuda:0")
    N = a.queries
    mesh = cnr.vis.marching_cubes(M.sphere(256, 0.85, 4.0))
    mesh.apply_translation([-0.5, -0.5, -0.5]).apply_scale(2.0)
    whole = cnr.devmesh.device_mesh(mesh, dev)
    clipped = MT._clip(whole, MT.box_planes(np.eye(4), [1.2, 1.2, 1.0]))
    q = MT.sample_surface(cnr.vis.Mesh(mesh.vertices * 1.02, mesh.faces), N, seed=0)
    rows = {}
    for name, tri in (("mc256", whole), ("mc256_clipped", clipped)):
        verts, faces, F = tri.verts, tri.faces, tri.n_faces
        ws = torch.empty(int(_C.load().cnr_point_mesh_workspace_bytes(N, F)), device=dev, dtype=torch.uint8)
        dist, face = torch.empty(N, device=dev), torch.empty(N, device=dev, dtype=torch.int32)
        near = torch.empty(N, 3, device=dev)

        def run_pass(k):
            return lambda: _C.call("cnr_point_mesh_pass", q, N, verts, faces, F, dist, face, near, ws, k)
        row = dict(faces=F, queries=N)
        for k, label in ((1, "record_ms"), (2, "partial_ms"), (3, "finish_ms")):
            row[label] = round(_median_ms(run_pass(k), a.reps), 4)
        ms = _median_ms(lambda: _C.call("cnr_point_mesh_dist", q, N, verts, faces, F, dist, face, near, ws), a.reps)
        row.update(total_ms=round(ms, 4), pairs_per_s=float("%.4g" % (N * F / (ms * 1e-3))), mean_dist=float(dist.double().mean()))
        rows[name] = row
        print(name, json.dumps(row), flush=True)
    g = torch.Generator(device=dev).manual_seed(0)
    p0 = torch.rand(N, 3, device=dev, generator=g) * 4 + 2
    p1 = torch.rand(N, 3, device=dev, generator=g) * 4 + 2
    ws = torch.empty(int(_C.load().cnr_nn_workspace_bytes(N, N)), device=dev, dtype=torch.uint8)
    out = torch.empty(N, device=dev)
    ms = _median_ms(lambda: _C.call("cnr_nn_dist", p0, N, p1, N, out, ws), a.reps)
    rows["nn_dist"] = dict(queries=N, points=N, ms=round(ms, 4), pairs_per_s=float("%.4g" % (N * N / (ms * 1e-3))))
    print("nn_dist", json.dumps(rows["nn_dist"]), flush=True)
    cq, cv, cf = P.random_case(2000, 2000)
    t0 = time.perf_counter()
    P.closest_f32(cq, cv, cf)
    dt = time.perf_counter() - t0
    rows["numpy_restatement_cpu"] = dict(queries=2000, faces=2000, s=round(dt, 3), pairs_per_s=float("%.4g" % (4e6 / dt)))
    print("numpy restatement", json.dumps(rows["numpy_restatement_cpu"]), flush=True)
    if a.index:
        lo, hi = whole.verts.amin(0), whole.verts.amax(0)
        g = torch.Generator(device=dev).manual_seed(1)
        centre_q = (lo + hi) / 2 + (torch.rand(N, 3, device=dev, generator=g) * 2 - 1) * (1e-3 / 3 ** 0.5) * float((hi - lo).max()) / 2
        for name, pts, tri in (("mc256", q, whole), ("mc256_clipped", q, clipped), ("mc256_centre", centre_q.contiguous(), whole)):
            rows["index_" + name] = _index_row(_C, MT, pts, tri, a.reps)
            print("index", name, json.dumps(rows["index_" + name]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, statistic="median", rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
