"""Times the stages of the TSDF path (csrc/tsdf.hip, cnr_amd.utils.TSDFVolume) on the GPU by device events: the
touch list of every frame, the unit tables (torch), the integration, the extraction, the 1 cm down-sample and the radius count,
and the triangle mesh (csrc/tsdf_mesh.hip: the 27-table, count, emit), on a synthetic sequence: a camera turning inside a box
room of 5 x 4 x 2.6 m, 640 x 480 frames.

    python tools/time_tsdf.py [--frames 300] [--reps 3] [--out FILE.json] [--mesh-out profiles/tsdf_mesh_time.json] [--mesh-reps 200]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

ROOM = np.array([[-2.5, -2.0, 0.0], [2.5, 2.0, 2.6]])


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


def room_frames(n, W, H, K, dev):
    """-> (depths (n,W,H) f32 in the volume's form, colors (n,W,H,3) u8, T_WC (n,4,4)): the inside of ROOM from a camera on a
    circle of radius 0.8 m at 1.4 m height, looking outwards and slightly down, millimetre depths"""
    from tsdf_cpu import look_at
    fx, fy, cx, cy = K
    x, y = torch.meshgrid(torch.arange(W, device=dev, dtype=torch.float64), torch.arange(H, device=dev, dtype=torch.float64),
                          indexing="ij")
    cam = torch.stack([(x - cx) / fx, (y - cy) / fy, torch.ones_like(x)], -1)
    lo, hi = (torch.from_numpy(v).to(dev) for v in ROOM)
    depths, poses = [], []
    for f in range(n):
        a = 2 * np.pi * f / n * 3
        eye = np.array([0.8 * np.cos(a), 0.8 * np.sin(a), 1.4 + 0.2 * np.sin(5 * a)])
        T = look_at(eye, eye + [np.cos(a), np.sin(a), -0.25 + 0.2 * np.cos(3 * a)])
        rays = cam @ torch.from_numpy(T[:3, :3].T.copy()).to(dev)
        o = torch.from_numpy(eye).to(dev)
        t = torch.where(rays > 0, (hi - o) / rays, (lo - o) / rays)           # the camera is inside: the nearest exit
        d = t.min(-1)[0].clamp(0.0, 10.0)
        depths.append((torch.round(d * 1000) / 1000).float())
        poses.append(T)
    depths = torch.stack(depths)
    colors = (depths[..., None] * torch.tensor([40.0, 25.0, 60.0], device=dev)).to(torch.uint8)
    return depths, colors.contiguous(), np.stack(poses)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--mesh-reps", type=int, default=200, help="repeats of the sub-millisecond mesh stages")
    ap.add_argument("--mesh-out", default=None, help="write the mesh stages' times and achieved bytes/s (profiles/tsdf_mesh_time.json)")
    a = ap.parse_args()
    import cnr_amd as cnr
    _C, U = cnr._C, cnr.utils
    assert torch.cuda.is_available(), "time_tsdf needs the GPU"
    dev = torch.device("cuda:0")
    W, H, K = 640, 480, (577.6, 578.7, 319.5, 239.5)
    voxel, trunc, F = 0.01, 0.04, a.frames
    depths, colors, T_WC = room_frames(F, W, H, K, dev)
    depths = torch.stack([U.tsdf_depth_image(d, torch.zeros(W, H, dtype=torch.int32, device=dev), 0, 0.001, 6.0) for d in depths])
    rows = dict(frames=F, width=W, height=H)

    slots = int(_C.load().cnr_tsdf_touch_slots(W, H))
    keys = torch.empty(F, slots, device=dev, dtype=torch.int64)
    tags = torch.empty(F, slots, device=dev, dtype=torch.int32)
    err = torch.zeros(1, device=dev, dtype=torch.int32)
    T_dev = torch.from_numpy(T_WC).to(dev)

    def touch():
        for f in range(F):
            _C.call("cnr_tsdf_touch", depths[f], W, H, *K, T_dev[f], voxel, trunc, f, keys[f], tags[f], err)
    rows["touch_all_frames_ms"] = round(_ms(touch, a.reps), 3)
    assert int(err.item()) == 0
    rows["unit_tables_torch_ms"] = round(_ms(lambda: U.tsdf_unit_tables(keys.reshape(-1), tags.reshape(-1)), a.reps), 3)
    units, frame_ofs, frame_idx, nb = U.tsdf_unit_tables(keys.reshape(-1), tags.reshape(-1))
    n_units = len(units)
    rows["units"], rows["unit_frame_pairs"] = n_units, len(frame_idx)
    rows["block_bytes"] = n_units * U.TSDF_BLOCK_BYTES
    tsdf = torch.empty(n_units, 4096, device=dev, dtype=torch.float32)
    weight, color = torch.empty_like(tsdf), torch.empty(n_units, 4096, 3, device=dev, dtype=torch.float32)
    T_CW = torch.from_numpy(np.ascontiguousarray(np.linalg.inv(T_WC))).to(dev)
    ms = _ms(lambda: _C.call("cnr_tsdf_integrate", units, n_units, frame_ofs, frame_idx, depths, colors, T_CW, F, W, H, *K, voxel, trunc,
                             tsdf, weight, color), a.reps)
    rows["integrate_ms"] = round(ms, 3)
    rows["integrate_voxel_frames_per_s"] = float("%.4g" % (len(frame_idx) * 4096 / (ms * 1e-3)))

    vol = U.TSDFVolume(voxel, trunc, device=dev)
    vol.units, vol.neighbours, vol.tsdf, vol.weight, vol.color = units, nb, tsdf, weight, color
    rows["extract_ms"] = round(_ms(vol.extract_points, a.reps), 3)
    cloud = vol.extract_point_cloud()
    rows["extracted_points"] = len(cloud)
    rows["down_sample_1cm_ms"] = round(_ms(lambda: cloud.voxel_down_sample(voxel), a.reps), 3)
    ds = cloud.voxel_down_sample(voxel)
    rows["down_sampled_points"] = len(ds)
    rows["radius_count_ms"] = round(_ms(lambda: U.radius_neighbour_counts(ds.points_device, 0.05), a.reps), 3)
    counts = U.radius_neighbour_counts(ds.points_device, 0.05)
    rows["radius_count_mean"], rows["radius_kept"] = round(float(counts.float().mean()), 2), int((counts > 100).sum())
    # the triangle mesh (csrc/tsdf_mesh.hip): the 27-table (torch), count and emit, against the bytes each stage must read.
    # These stages take a fraction of a millisecond, so they (and the points extraction beside them) are timed over more repeats.
    mreps = max(a.reps, a.mesh_reps)
    hood_ms = _ms(lambda: U.tsdf_unit_neighbourhood(units), mreps)
    hood = U.tsdf_unit_neighbourhood(units)
    ws = _C.workspace(_C.load().cnr_tsdf_mesh_workspace_bytes(n_units), dev, "cnr_tsdf_mesh")
    cnt = torch.zeros(2, device=dev, dtype=torch.int64)
    count_ms = _ms(lambda: _C.call("cnr_tsdf_mesh_count", tsdf, weight, hood, n_units, ws, cnt), mreps)
    V, Fc = (int(v) for v in cnt.tolist())
    verts, vcol, vnor = (torch.empty(max(V, 1), 3, device=dev, dtype=torch.float64) for _ in range(3))
    faces = torch.empty(max(Fc, 1), 3, device=dev, dtype=torch.int32)
    emit_ms = _ms(lambda: _C.call("cnr_tsdf_mesh_emit", units, tsdf, weight, color, hood, n_units, voxel, ws, verts, vcol, vnor, faces),
                  mreps)
    points_ms = _ms(vol.extract_points, mreps)
    count_bytes = n_units * 2 * 4096 * 4                      # tsdf + weight of every unit once
    emit_bytes = count_bytes + V * 2 * 3 * 4                  # ... and the two ends' colours of every emitted vertex
    points_bytes = count_bytes + rows["extracted_points"] * 2 * 3 * 4
    rows.update(neighbourhood_ms=round(hood_ms, 3), mesh_count_ms=round(count_ms, 4), mesh_emit_ms=round(emit_ms, 4), mesh_vertices=V,
                mesh_faces=Fc)
    stage = lambda ms, nbytes: dict(ms=round(ms, 4), must_read_bytes=nbytes, bytes_per_s=float("%.4g" % (nbytes / (ms * 1e-3))))
    mesh_rows = dict(units=n_units, vertices=V, faces=Fc, extracted_points=rows["extracted_points"], block_bytes=rows["block_bytes"],
                     repeats=mreps, neighbourhood=dict(ms=round(hood_ms, 4)), mesh_count=stage(count_ms, count_bytes),
                     mesh_emit=stage(emit_ms, emit_bytes), extract=stage(points_ms, points_bytes))
    t = time.perf_counter()
    v2 = U.TSDFVolume(voxel, trunc, device=dev).integrate_frames(depths, colors, np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]]),
                                                                 T_WC)
    v2.extract_point_cloud().voxel_down_sample(voxel).remove_radius_outlier(100, 0.05)
    torch.cuda.synchronize()
    rows["whole_chain_wall_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    print(json.dumps(rows), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, rows=rows), f, indent=1)
    if a.mesh_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.mesh_out)), exist_ok=True)
        cached = ("the blocks (block_bytes) fit in the 256 MiB Infinity Cache, so bytes_per_s is a cache-resident rate, not an HBM rate; "
                  if rows["block_bytes"] < (256 << 20) else "")
        note = ("device-event times over `repeats` back-to-back calls after one warm-up call; " + cached +
                "must_read_bytes: tsdf + weight of every unit once (8 KB per unit), plus for mesh_emit and extract "
                "the two ends' colours of every emitted vertex or point; extract = extract_points (count, one read-back, emit), the "
                "yardstick of the same run")
        with open(a.mesh_out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, frames=F, note=note, stages=mesh_rows), f, indent=1)


if __name__ == "__main__":
    main()
