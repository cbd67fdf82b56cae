"""Trains the per-object fields category registration probes (object_fields.ObjectFieldTrainer: one OccupancyMap(32) +
UniDirsEmbed per instance of a sequence, all instances per launch) and writes them where registration.load_pretrained looks:
<weight_root>/ckpt/<obj_id>/obj_<obj_id>_it_<iters>.pth.

    python tools/pretrain_objects.py --config CFG.json --iters 10000 [--rays 120] [--weight-root DIR] [--seed 0]

The dataset is loaded without a registration cache and without registering (the pools need only the frames); ``bbox`` of every
checkpoint is the oriented box of the instance's cloud (Replica; ScanNet sequences get None, their clouds come with tsdf
registration)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True)
    ap.add_argument("--iters", type=int, required=True)
    ap.add_argument("--rays", type=int, default=None, help="rays per object and step (default: render.n_per_optim)")
    ap.add_argument("--weight-root", default=None, help="default: registration.weight_root of the config")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--log", type=int, default=500)
    a = ap.parse_args()
    import cnr_amd as cnr
    from cnr_amd import category_registration as CR, dataset as D
    from cnr_amd.object_fields import ObjectFieldTrainer
    assert torch.cuda.is_available(), "pretrain_objects needs the GPU"
    cfg = cnr.cfg.Config(a.config)
    root = a.weight_root or getattr(cfg, "weight_root", None)
    if not root:
        raise SystemExit("no --weight-root and no registration.weight_root in the config")
    # the frames alone: _load_inst_dict would want a cache or a registration
    cls = D.Replica if cfg.dataset_format == "Replica" else D.ScanNet
    load = D._load_inst_dict
    D._load_inst_dict = lambda dataset, cfg: None
    try:
        ds = cls(cfg)
    finally:
        D._load_inst_dict = load
    tr = ObjectFieldTrainer.from_dataset(ds, cfg, rays_per_step=a.rays, seed=a.seed)
    print("%d objects, %d rays x %d samples per step, pools of %d..%d rows" % (tr.N, tr.R, tr.S, min(tr.rows), max(tr.rows)), flush=True)
    done = 0
    while done < a.iters:
        n = min(a.log, a.iters - done)
        tr.run(n)
        done += n
        l = tr.losses.cpu()
        print("it %6d  depth %.4f  colour %.4f  opacity %.4f  (means over the objects)  flags %s"
              % (done, l[0].mean(), l[1].mean(), l[2].mean(), sorted(set(tr.flags.cpu().tolist()))), flush=True)
    boxes = {}
    if ds.name == "replica":
        from cnr_amd.utils import accumulate_pointcloud, get_bound
        for cls_id, entries in ds.inst_dict.items():
            if cls_id != 0:
                for obj_id, e in entries.items():
                    boxes[obj_id] = get_bound(accumulate_pointcloud(int(obj_id), e["frame_info"], ds.sample_dict, ds.intrinsic_open3d))
    for f in tr.save_checkpoints(root, boxes):
        print(f)


if __name__ == "__main__":
    main()
