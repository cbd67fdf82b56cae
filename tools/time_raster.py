"""Times the mesh rasteriser (csrc/raster.hip, cnr_amd.raster) on the GPU by device events after warm-up, stage by stage
(setup + count with its read-back of the pair count, emit, tiles, attributes):
  * a 256^3 marching-cubes sphere (about 440 k faces) at 1200 x 680, one view per launch and 16 views per launch;
  * a coarse room: a box of 6 x 6 x 2 triangles per wall seen from inside, every triangle over many tiles;
and for context a chunked torch formulation of the same coverage rule (all pixels x all faces, fp64) against the kernels on a
small mesh, and the field render of profiles/view_time.json.

    python tools/time_raster.py [--reps 20] [--out profiles/raster_time.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]


def sphere_volume(D, radius):
    g = torch.linspace(0.0, 1.0, D)
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    return (0.5 + (radius - ((x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2).sqrt())).float()


def room_mesh(n=6, half=(3.0, 2.5, 1.4)):
    """a box around the origin, every wall n x n quads of two triangles: (verts, faces)"""
    verts, faces = [], []
    g = np.linspace(-1.0, 1.0, n + 1)
    for axis in range(3):
        for side in (-1.0, 1.0):
            base = len(verts)
            for a in g:
                for b in g:
                    p = [0.0, 0.0, 0.0]
                    p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = side, a, b
                    verts.append([p[k] * half[k] for k in range(3)])
            for i in range(n):
                for j in range(n):
                    q = base + i * (n + 1) + j
                    faces += [[q, q + 1, q + n + 2], [q, q + n + 2, q + n + 1]]
    return np.array(verts, np.float32), np.array(faces, np.int64)


def torch_raster(rast, scene, T_wc, block=64):
    """the coverage rule in torch, fp64: every pixel against every face, `block` faces at a time -> (depth, face)"""
    dev = rast.device
    T = torch.from_numpy(np.linalg.inv(T_wc)).to(dev)
    p = scene.verts.double()[scene.faces.long()] @ T[:3, :3].T + T[:3, 3]
    n = torch.stack([torch.linalg.cross(p[:, 1], p[:, 2]), torch.linalg.cross(p[:, 2], p[:, 0]), torch.linalg.cross(p[:, 0], p[:, 1])], 1)
    det = (p[:, 0] * n[:, 0]).sum(-1)
    d = rast.dirs().double()
    P = d.shape[0]
    best_t = torch.full((P,), float("inf"), device=dev, dtype=torch.float64)
    best_f = torch.full((P,), -1, device=dev, dtype=torch.int64)
    for a in range(0, len(det), block):
        e = torch.einsum("pk,fik->pfi", d, n[a:a + block])
        S = e.sum(-1)
        s = torch.where(det[a:a + block] > 0, 1.0, -1.0)
        t = det[a:a + block] / S
        cov = ((s[None, :, None] * e >= 0).all(-1) & (s * S > 0) & (t >= rast.zmin) & (t <= rast.zmax) & (det[a:a + block] != 0))
        tc = torch.where(cov, t, torch.full_like(t, float("inf")))
        tj, j = tc.min(1)
        upd = tj < best_t
        best_t = torch.where(upd, tj, best_t)
        best_f = torch.where(upd, j + a, best_f)
    return torch.where(best_f >= 0, best_t, torch.zeros_like(best_t)).float().reshape(rast.W, rast.H), best_f.reshape(rast.W, rast.H)


def timed(rast, fn, reps, warm=2):
    """-> (ms per call, {stage: ms per call}) by device events"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    total, stages = [], {}
    for _ in range(reps):
        rast.stage_events = []
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        total.append(a.elapsed_time(b))
        ev = rast.stage_events
        for (_, e0), (name, e1) in zip(ev[:-1], ev[1:]):
            if name != "start":
                stages[name] = stages.get(name, 0.0) + e0.elapsed_time(e1)
    rast.stage_events = None
    return float(np.median(total)), {k: round(v / reps, 4) for k, v in stages.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import cnr_amd as cnr
    from cnr_amd import raster
    from render_mesh import look_at
    assert torch.cuda.is_available(), "time_raster needs the GPU"
    dev = torch.device("cuda:0")
    W, H = 1200, 680
    rast = raster.MeshRasterizer.from_intrinsics(W, H, 600.0, 600.0, 599.5, 339.5, 0.05, 20.0, device=dev)
    rows = {}

    def record(name, scene, poses, **kw):
        ms, stages = timed(rast, lambda: rast.render(scene, poses, **kw), a.reps)
        V = 1 if poses.ndim == 2 else len(poses)
        res = rast.render(scene, poses, **kw)
        rows[name] = dict(faces=scene.n_faces, views=V, pairs_last_launch=rast.pairs, render_ms=round(ms, 3), ms_per_view=round(ms / V, 3),
                          stage_ms=stages, pixels_hit=int((res["face"] >= 0).sum()))
        print(name, json.dumps(rows[name]), flush=True)

    ball = raster.MeshScene(cnr.vis.marching_cubes(sphere_volume(256, 0.42).to(dev)), device=dev)
    c = np.array([0.5, 0.5, 0.5])
    one = look_at(c + [1.1, 0.6, 0.4], c)
    ring = np.stack([look_at(c + [1.3 * np.cos(t), 1.3 * np.sin(t), 0.4], c) for t in 2 * np.pi * np.arange(16) / 16])
    record("sphere256_1view", ball, one)
    record("sphere256_1view_depth_only", ball, one, attributes=False)
    record("sphere256_16views_per_launch", ball, ring, views_per_launch=16)
    record("sphere256_16views_one_per_launch", ball, ring, views_per_launch=1)
    room = raster.MeshScene(room_mesh(), device=dev)
    record("room_1view", room, look_at([-2.0, -1.5, 0.2], [1.0, 1.0, -0.2]))
    # context: the same rule in torch on a small mesh, and the kernels on that mesh
    small = raster.MeshScene(cnr.vis.marching_cubes(sphere_volume(24, 0.42).to(dev)), device=dev)
    record("sphere24_1view_depth_only", small, one, attributes=False)
    torch_raster(rast, small, one)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        depth_t, face_t = torch_raster(rast, small, one)
    e1.record()
    torch.cuda.synchronize()
    res = rast.render(small, one, attributes=False)
    rows["sphere24_1view_torch_all_pairs"] = dict(faces=small.n_faces, render_ms=round(e0.elapsed_time(e1) / 3, 3),
                                                  faces_equal=bool((face_t == res["face"].long()).all()))
    print("torch", json.dumps(rows["sphere24_1view_torch_all_pairs"]), flush=True)
    view_file = os.path.join(ROOT, "profiles", "view_time.json")
    if os.path.exists(view_file):
        with open(view_file) as f:
            v = json.load(f)
        rows["field_render_view_time_json"] = {k: v["render"][k]["render_ms"] for k in v.get("render", {})}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/time_raster.py", device=torch.cuda.get_device_name(0), camera=[W, H], reps=a.reps, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
