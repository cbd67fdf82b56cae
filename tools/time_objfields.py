"""Times one train step of N per-object fields (R = 120 rays x S = 10 samples each) on the GPU, by device events after warm-up:

  fused     ONE cnr_obj_train launch for all N objects (object_fields.ObjectFieldTrainer.launch), and
  modular   N sequential steps of the exact tier, BackgroundStep(precision="fp32") on a cfg copy with the objects' width, bins
            and rays -- the only way to do this work without cnr_obj_train -- eagerly and, after its warm-up, as its hipGraph.

Both sides alternate inside one process; each figure is the median of `--rounds` windows of `--reps` steps.  The fused side's
arithmetic rate is the step's multiply-adds (counted from the shapes, below) over its time; cnr_obj_train runs them on the vector
unit in fp32, so the achieved MFMA fraction is 0 by construction and the rate is given against the fp32 vector peak.

    python tools/time_objfields.py [--reps 50] [--rounds 5] [--sizes 8,64,256] [--out profiles/objfields_time.json]"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

R, N1, N2 = 120, 1, 9
VECTOR_FP32_PEAK = 157.3e12          # MI355X: 256 CUs x 128 lanes x 2 flop x 2.4 GHz


def step_flops(R, S):
    """multiply-adds x 2 of one object's step: forward (11 136 weights incl. heads), backward chain (the 32-wide inputs of four
    layers + heads), weight gradients (every weight once), PE backward (126 features x 32, e1 twice)"""
    M = R * S
    w_fwd = 32 * (87 + 32 + 119 + 32 + 74) + 32 + 96
    w_chain = 4 * 32 * 32 + 32 + 96
    w_pe = 32 * (84 * 2 + 42)
    return 2 * M * (w_fwd + w_chain + w_fwd + w_pe)


def _window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="8,64,256")
    ap.add_argument("--modular-max", type=int, default=64, help="largest N whose N modular steps are timed (they are sequential)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import cnr_amd as cnr
    from cnr_amd.background import BackgroundStep
    from cnr_amd.object_fields import ObjectFieldTrainer
    assert torch.cuda.is_available(), "time_objfields needs the GPU"
    dev = torch.device("cuda:0")
    cfg = cnr.cfg.synthetic_config(device=str(dev), n_bins_cam2surface=N1, n_bins=N2)
    gen = torch.Generator().manual_seed(0)
    sizes = [int(s) for s in a.sizes.split(",")]
    pools = {o: cnr.scene_cateogries.synthetic_pool(2048, 1, gen, "cpu") for o in range(max(sizes))}
    # the modular tier: one BackgroundStep per object (the object's width, bins, rays and scale)
    mcfg = copy.copy(cfg)
    mcfg.hidden_feature_size_bg, mcfg.n_bins_cam2surface_bg, mcfg.n_per_optim_bg, mcfg.bg_scale = 32, N1, R, cfg.obj_scale
    n_mod = min(max(sizes), a.modular_max)
    mods = [BackgroundStep(mcfg, pools[o], R, dev, seed=o, precision="fp32") for o in range(n_mod)]
    for m in mods:                       # warm-up: three eager steps, then the captured step
        for _ in range(5):
            m.step()
    torch.cuda.synchronize()
    rows = {}
    for N in sizes:
        tr = ObjectFieldTrainer(cfg, pools, list(range(N)), rays_per_step=R, seed=1)
        for _ in range(5):
            tr.launch()
        torch.cuda.synchronize()
        fused, eager, graph = [], [], []
        for _ in range(a.rounds):        # alternate the sides
            fused.append(_window(tr.launch, a.reps))
            if N <= n_mod:
                reps = max(2, a.reps // 10)
                eager.append(_window(lambda: [m.step(use_graph=False) for m in mods[:N]], reps))
                graph.append(_window(lambda: [m.step() for m in mods[:N]], reps))
        f = statistics.median(fused)
        row = dict(fused_ms=round(f, 4), fused_ms_min_max=[round(min(fused), 4), round(max(fused), 4)],
                   fused_us_per_object=round(1e3 * f / N, 3), flops_per_step=N * step_flops(R, N1 + N2),
                   fused_tflops=round(N * step_flops(R, N1 + N2) / (f * 1e-3) / 1e12, 3),
                   fused_share_of_fp32_vector_peak=round(N * step_flops(R, N1 + N2) / (f * 1e-3) / VECTOR_FP32_PEAK, 4),
                   mfma_fraction=0.0, finite=bool(torch.isfinite(tr.theta).all()))
        if eager:
            row.update(modular_eager_ms=round(statistics.median(eager), 3), modular_graph_ms=round(statistics.median(graph), 3),
                       speedup_vs_modular_graph=round(statistics.median(graph) / f, 1))
        rows[str(N)] = row
        print(N, json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(dict(device=torch.cuda.get_device_name(0), R=R, S=N1 + N2, reps=a.reps, rounds=a.rounds, rows=rows), fo, indent=1)


if __name__ == "__main__":
    main()
