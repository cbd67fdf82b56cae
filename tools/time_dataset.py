"""Time each stage of the Replica loader (cnr_amd.dataset) on a synthetic 200-frame 1200 x 680 tree and compare with the
reference-style per-instance numpy loop (tests/dataset_cpu.py) on the same frames.  Writes profiles/dataset_time.json.

    python tools/time_dataset.py [--frames 200] [--ref-frames 5] [--out profiles/dataset_time.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def write_tree(root, n, W=1200, H=680, n_obj=40, seed=0):
    rng = np.random.default_rng(seed)
    for sub in ("rgb", "depth", "semantic_instance", "semantic_class"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    boxes = [(rng.integers(0, H - 60), rng.integers(0, W - 80), rng.integers(20, 200), rng.integers(20, 300)) for _ in range(n_obj)]
    classes = rng.integers(1, 100, n_obj)
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(n):
        inst = np.full((H, W), 1, np.uint16)
        cls = np.full((H, W), 93, np.uint16)
        for k, (r, c, h, w) in enumerate(boxes):
            if rng.random() < 0.8:
                r2, c2 = r + rng.integers(-5, 6), c + rng.integers(-5, 6)
                inst[max(r2, 0):r2 + h, max(c2, 0):c2 + w] = k + 2
                cls[max(r2, 0):r2 + h, max(c2, 0):c2 + w] = classes[k]
        rgb = ((np.sin(xx * 0.01 + i) * 100 + 120)[..., None] + rng.integers(0, 30, (H, W, 3))).astype(np.uint8)
        depth = (2000 + 1500 * np.cos(yy * 0.005 + i * 0.1) + rng.integers(0, 50, (H, W))).astype(np.uint16)
        Image.fromarray(rgb).save(os.path.join(root, "rgb", f"rgb_{i}.png"))
        Image.fromarray(depth).save(os.path.join(root, "depth", f"depth_{i}.png"))
        Image.fromarray(inst).save(os.path.join(root, "semantic_instance", f"semantic_instance_{i}.png"))
        Image.fromarray(cls).save(os.path.join(root, "semantic_class", f"semantic_class_{i}.png"))
    T = np.tile(np.eye(4).reshape(1, 16), (n, 1))
    np.savetxt(os.path.join(root, "traj_w_c.txt"), T, delimiter=" ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--ref-frames", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dataset_time.json"))
    args = ap.parse_args()
    import cnr_amd
    from cnr_amd import dataset as D
    from dataset_cpu import CpuFrameTable
    assert torch.cuda.is_available(), "time_dataset needs the GPU"
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        write_tree(root, args.frames)
        t_write = time.perf_counter() - t0
        cfg = cnr_amd.cfg.synthetic_config(device=str(dev))
        cfg.dataset_dir, cfg.depth_scale, cfg.mw, cfg.mh = root, 0.001, 0, 0
        ds = D.Replica.__new__(D.Replica)
        ds.name, ds.device, ds.root_dir = "replica", str(dev), root
        ds.Twc = np.loadtxt(os.path.join(root, "traj_w_c.txt"), delimiter=" ").reshape([-1, 4, 4])
        ds.depth_scale, ds.max_depth = cfg.depth_scale, cfg.max_depth
        ds._camera(cfg)
        ds.background_cls_list, ds.bbox_scale = [5, 12, 30, 31, 40, 60, 92, 93, 95, 97, 98, 79], 0.2
        ds.n_img = args.frames
        ds.get_all_frames()                                      # warm-up: code objects, pinned pool, page cache
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ds.get_all_frames()
        torch.cuda.synchronize()
        t_total = time.perf_counter() - t0
        # the same work stage by stage, one batch at a time, synchronised between stages
        st = dict(decode=0.0, upload=0.0, table_kernels=0.0, host_logic=0.0, finish_kernel=0.0, copy_back=0.0)
        ds.inst_dict, ds.sample_dict = {}, {}
        with D._pool() as pool:
            for b0 in range(0, ds.n_img, D.BATCH):
                idxs = list(range(b0, min(b0 + D.BATCH, ds.n_img)))
                t = time.perf_counter()
                frames = list(pool.map(ds._decode, idxs))
                st["decode"] += time.perf_counter() - t
                t = time.perf_counter()
                rgb, depth, inst, obj = [D._pinned([fr[k] for fr in frames]).to(dev, non_blocking=True) for k in range(4)]
                torch.cuda.synchronize()
                st["upload"] += time.perf_counter() - t
                t = time.perf_counter()
                table = D.FrameTable(inst, obj)
                torch.cuda.synchronize()
                st["table_kernels"] += time.perf_counter() - t
                t = time.perf_counter()
                keep = np.zeros(len(table.ids), dtype=bool)
                for f, idx in enumerate(idxs):
                    keep[table.offsets[f]:table.offsets[f + 1]] = ds._frame_instances(idx, *table.frame(f), table.W, table.H)
                st["host_logic"] += time.perf_counter() - t
                t = time.perf_counter()
                out = table.finish(keep, depth, rgb, 0, ds.depth_scale, ds.max_depth)
                torch.cuda.synchronize()
                st["finish_kernel"] += time.perf_counter() - t
                t = time.perf_counter()
                out = [o.cpu().numpy() for o in out]
                st["copy_back"] += time.perf_counter() - t
        # reference-style loop (full-frame mask per instance) on the first frames, decoded already
        frames = [ds._decode(i) for i in range(args.ref_frames)]
        t0 = time.perf_counter()
        for fr in frames:
            CpuFrameTable(fr[2][None], fr[3][None])
        t_ref = (time.perf_counter() - t0) / args.ref_frames
        n_inst = float(np.mean(np.diff(table.offsets)))
    upload_bytes = args.frames * 1200 * 680 * (3 + 2 + 2 + 2)
    res = dict(device=torch.cuda.get_device_name(0), frames=args.frames, W=1200, H=680, batch=D.BATCH,
               decode_workers=min(D.DECODE_WORKERS, os.cpu_count() or 1), tree_write_s=round(t_write, 2),
               get_all_frames_s=round(t_total, 4), per_frame_ms=round(1e3 * t_total / args.frames, 3),
               stages_s={k: round(v, 4) for k, v in st.items()},
               upload_bytes=upload_bytes, upload_GBps=round(upload_bytes / st["upload"] / 1e9, 2),
               instances_per_frame=n_inst, reference_loop_per_frame_s=round(t_ref, 4),
               reference_loop_frames_timed=args.ref_frames)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
