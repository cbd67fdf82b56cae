"""Times the registration stages (csrc/pointcloud.hip, cnr_amd.category_registration) on the GPU by device events after
warm-up, and the same stages in the CPU restatement (tests/registration_cpu.py, scipy cKDTree) on the same machine:
unprojection + down-sample of one instance over 8 synthetic 1200 x 680 frames, one cnr_icp_step at B = 24 for 2.5k x 2.5k and
50k x 50k points, and align_poses on a class of 4 chairs and a pole (tests/registration_cpu.py's solver_case).

    python tools/time_registration.py [--reps 20] [--out FILE.json] [--skip-cpu-class]"""
import argparse
import json
import os
import sys
import time

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


def _wall_ms(fn, reps=1):
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t) * 1e3 / reps


def synthetic_frames(n=8, W=1200, H=680, seed=0):
    """a box-shaped instance in front of a wall, seen from n poses: sample_dict-style (W,H) arrays"""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    samples, info = {}, []
    for f in range(n):
        depth = (3.0 + 0.2 * np.sin(u / 90.0 + f) + 0.1 * np.cos(v / 70.0)).astype(np.float32)
        mask = np.zeros((W, H), np.int32)
        mask[300 + 10 * f:700 + 10 * f, 200:520] = 7
        depth[mask == 7] -= 1.2
        T = np.eye(4)
        T[:3, 3] = [0.05 * f, 0.02 * f, 0.0]
        samples[f] = {"image": rng.integers(0, 256, (W, H, 3), dtype=np.uint8), "depth": depth, "obj_mask": mask, "T": T, "frame_id": f}
        info.append({"frame": f})
    return samples, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-cpu-class", action="store_true")
    a = ap.parse_args()
    import cnr_amd as cnr
    import registration_cpu as RC
    _C = cnr._C
    assert torch.cuda.is_available(), "time_registration needs the GPU"
    dev = torch.device("cuda:0")
    rows = {}

    samples, info = synthetic_frames()
    K = cnr.dataset.PinholeIntrinsics(1200, 680, 600.0, 600.0, 599.5, 339.5)
    on_dev = {f: {k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) and k != "T" else v) for k, v in s.items()}
              for f, s in samples.items()}
    frames = [(on_dev[i["frame"]]["image"], on_dev[i["frame"]]["depth"], on_dev[i["frame"]]["obj_mask"], samples[i["frame"]]["T"])
              for i in info]
    pc = cnr.utils._unproject_frames(frames, [7] * len(frames), K, dev)
    rows["unproject_points"] = len(pc)
    rows["unproject_8_frames_ms"] = round(_ms(lambda: cnr.utils._unproject_frames(frames, [7] * len(frames), K, dev), a.reps), 4)
    rows["down_sample_1cm_ms"] = round(_ms(lambda: pc.voxel_down_sample(0.01), a.reps), 4)
    rows["down_sample_voxels"] = len(pc.voxel_down_sample(0.01))

    def cpu_unproject():
        return np.concatenate([RC.unproject(samples[i["frame"]], 7, 600.0, 600.0, 599.5, 339.5)[1] for i in info]).astype(np.float32)
    rows["cpu_unproject_8_frames_ms"] = round(_wall_ms(cpu_unproject), 2)
    pts = cpu_unproject()
    rows["cpu_down_sample_1cm_ms"] = round(_wall_ms(lambda: RC.voxel_down_sample(pts, None, 0.01)), 2)

    g = torch.Generator(device=dev).manual_seed(0)
    for n in (2500, 50000):
        src = torch.rand(n, 3, device=dev, generator=g) + 2
        tgt = torch.rand(n, 3, device=dev, generator=g) + 2
        B = 24
        T = torch.eye(4, device=dev, dtype=torch.float64).repeat(B, 1, 1).contiguous()
        T[:, :3, 3] = torch.rand(B, 3, device=dev, generator=g).double() * 0.02
        ws = torch.empty(int(_C.load().cnr_icp_workspace_bytes(n, n, B)), device=dev, dtype=torch.uint8)
        sums = torch.zeros(B, 17, device=dev, dtype=torch.float64)
        state = torch.zeros(B, 4, device=dev, dtype=torch.float64)
        ms = _ms(lambda: _C.call("cnr_icp_step", src, n, tgt, n, T, B, 0.1, None, ws, sums, None, None), a.reps)
        key = "icp_step_B24_%gk" % (n / 1000)
        rows[key] = dict(ms=round(ms, 4), pairs_per_s=float("%.4g" % (B * n * n / (ms * 1e-3))))
        Tc = T.clone()
        rows[key]["update_ms"] = round(_ms(lambda: _C.call("cnr_icp_update", sums, n, B, 1 << 30, Tc, state.zero_()), a.reps), 4)
        s_np, t_np, T_np = src.cpu().numpy().astype(np.float64), tgt.cpu().numpy().astype(np.float64), T.cpu().numpy()
        tree = RC.cKDTree(t_np)
        reps = 1 if n > 10000 else 3
        rows[key]["cpu_ms"] = round(_wall_ms(lambda: [tree.query(s_np @ Tb[:3, :3].T + Tb[:3, 3]) for Tb in T_np], reps), 2)
        print(key, rows[key], flush=True)

    clouds, poses, counts = RC.solver_case()

    def gpu_class():
        d = RC.build_dicts(clouds, counts, lambda p: cnr.utils.PointCloud(p, device=dev))
        cnr.category_registration.align_poses(*d, name="replica", device=str(dev))
    gpu_class()
    torch.cuda.synchronize()
    rows["align_class_of_5_ms"] = round(_wall_ms(lambda: (gpu_class(), torch.cuda.synchronize())), 1)
    if not a.skip_cpu_class:
        def cpu_class():
            d = RC.build_dicts(clouds, counts, RC.CpuCloud)
            RC.align_poses_cpu(*d, RC.IcpSolverCpu(0.02, 0.10, get_bound=cnr.utils.get_bound), cnr.utils)
        rows["cpu_align_class_of_5_ms"] = round(_wall_ms(cpu_class), 1)
    print(json.dumps(rows), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
