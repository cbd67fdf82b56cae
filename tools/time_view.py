"""Times SceneRenderer.render on the GPU: the 1200 x 680 Replica camera, a synthetic scene of a background (hidden size 128)
and 2 categories x 4 objects (random-init weights: the timing does not depend on what the fields hold, only the instance
statistics do), S = 64 samples per segment.  By device events after warm-up, medians over --reps renders:

  * the stages of one render, summed over its pixel chunks: segments (count + emit, including the two small device-to-host
    reads of the counts), points, every field evaluation, composite;
  * the whole render by a host clock around a device synchronise, and pixels per second;
  * cnr_view_composite alone on the arrays of the whole image, against the same composite written with torch ops on the
    device (gather the segments of a pixel, stable sort by z, cumprod, sums), alternating the two, and the largest
    difference between their results.

    python tools/time_view.py [--reps 9] [--samples 64] [--out profiles/view_time.json]

--skip times empty-space skipping instead (render(..., skip_empty=True)) and writes profiles/view_skip_time.json.  Random
initial weights put every occupancy near 0.5, so build_grids would keep every cell; the grids are handed in by set_grids: at
G = 64 a shell for the background (the cells within 2 cells of a face of its box) and a ball of radius 0.6 of the box for every
object, and the all-set grids, which skip nothing and so show what the extra launches and the scatter cost.  Per grid set
and background precision: the share of samples evaluated, the stages and the whole render, beside the unskipped render of the
same run; and build_grids(resolution=64, sub=2) on its own.

    python tools/time_view.py --skip [--reps 9] [--samples 64] [--out profiles/view_skip_time.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def torch_composite(sigma, color, z, pix_segs, thr, seg_inst):
    """the merged composite with torch ops: (P, KMAX * S) padded gather, stable sort by z, cumprod"""
    P, K = pix_segs.shape
    S = sigma.shape[1]
    valid = pix_segs >= 0
    idx = pix_segs.clamp_min(0).long()
    zz = torch.where(valid[..., None], z[idx], torch.full((), float("inf"), device=z.device)).reshape(P, K * S)
    occ = torch.where(valid[..., None], torch.sigmoid(sigma[idx]), torch.zeros((), device=z.device)).reshape(P, K * S)
    col = color[idx].reshape(P, K * S, 3)
    zs, order = torch.sort(zz, dim=1, stable=True)
    occ_s = torch.gather(occ, 1, order)
    free = 1.0 - occ_s + 1e-10
    T = torch.cumprod(torch.cat([torch.ones(P, 1, device=z.device), free[:, :-1]], 1), 1)
    term_s = occ_s * T
    term = torch.zeros_like(term_s).scatter_(1, order, term_s)                 # back in source order
    zz0 = torch.where(valid[..., None], z[idx], torch.zeros((), device=z.device)).reshape(P, K * S)
    depth = (term * zz0).sum(1)
    rgb = (term[..., None] * col).sum(1)
    mass = term.reshape(P, K, S).sum(2)
    opacity = mass.sum(1)
    var = (term * (zz0 - depth[:, None]) ** 2).sum(1)
    best = mass.argmax(1)
    inst = torch.where(opacity >= thr, seg_inst[torch.gather(idx, 1, best[:, None])[:, 0]], torch.full_like(best, -1).int())
    return dict(rgb=rgb, depth=depth, opacity=opacity, var=var, mass=mass, instance=inst)


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def time_render(r, T, S, reps, **kw):
    """medians over `reps` renders after one warm-up: the stages by device events, the whole by a host clock"""
    P = r.W * r.H
    with torch.no_grad():
        r.render(T, n_samples=S, **kw)                                  # warm-up: code objects, allocator
        torch.cuda.synchronize()
        stages, wall = {}, []
        for _ in range(reps):
            r.stage_events = []
            t0 = time.perf_counter()
            r.render(T, n_samples=S, **kw)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ev, tot = r.stage_events, {}
            for (_, e0), (name, e1) in zip(ev[:-1], ev[1:]):
                if name != "start":
                    tot[name] = tot.get(name, 0.0) + e0.elapsed_time(e1)
            for k, v in tot.items():
                stages.setdefault(k, []).append(v)
            r.stage_events = None
    return dict(stage_ms={k: round(statistics.median(v), 3) for k, v in stages.items()},
                render_ms=round(statistics.median(wall), 3),
                render_ms_min_max=[round(min(wall), 3), round(max(wall), 3)],
                pixels_per_s=round(P / (statistics.median(wall) * 1e-3)))


def shell_and_ball_grids(r, G=64, shell=2, radius=0.6):
    """(E,G,G,G) bool: the background keeps the cells within `shell` cells of a face of its box, every object the cells whose
    centre lies within `radius` of its box's centre"""
    i = torch.arange(G)
    edge = (i < shell) | (i >= G - shell)
    shell_bits = edge[:, None, None] | edge[None, :, None] | edge[None, None, :]
    c = (i.float() + 0.5) * 2.0 / G - 1.0
    ball_bits = (c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2) <= radius ** 2
    return torch.stack([shell_bits if e.cat < 0 else ball_bits for e in r.entities])


def skip_leg(a, cnr, r, scene_bg, T, S, dev):
    G = 64
    grid_sets = {"all_set": torch.ones(len(r.entities), G, G, G, dtype=torch.bool), "shell_and_balls": shell_and_ball_grids(r, G)}
    rows = {}
    for bg_precision in ("fp32", "fused"):
        scene_bg.trainer.eval_precision = bg_precision
        row = dict(unskipped=time_render(r, T, S, a.reps))
        for name, bits in grid_sets.items():
            r.set_grids(bits)
            row[name] = time_render(r, T, S, a.reps, skip_empty=True)
            evaluated, total = r.active_samples
            row[name].update(samples_evaluated=evaluated, samples=total, active_share=round(evaluated / total, 4),
                             cells_set_share=round(float(bits.float().mean()), 4),
                             render_ms_over_unskipped=round(row[name]["render_ms"] / row["unskipped"]["render_ms"], 3))
        row["all_set_added_ms"] = round(row["all_set"]["render_ms"] - row["unskipped"]["render_ms"], 3)
        rows[bg_precision] = row
        print(bg_precision, json.dumps(row))
        # build_grids on its own (the grids it builds from random weights keep nearly every cell: only its time is of use)
        r.build_grids(resolution=G, sub=2)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r.build_grids(resolution=G, sub=2)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        row["build_grids_ms"] = round(statistics.median(ms), 3)
        row["build_grids_ms_min_max"] = [round(min(ms), 3), round(max(ms), 3)]
        row["build_grids_cells_set_share"] = round(float(r.grids().float().mean()), 4)
        r.set_grids(None)
    result = dict(tool="tools/time_view.py --skip", device=torch.cuda.get_device_name(0), camera=[r.W, r.H], samples=S, reps=a.reps,
                  entities=len(r.entities), chunk=65536, grid=G, build_grids=dict(resolution=G, sub=2, lattice=G * 2 + 1),
                  render=rows)
    print(json.dumps(result))
    out = a.out or os.path.join(ROOT, "profiles", "view_skip_time.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip", action="store_true", help="time empty-space skipping instead (writes profiles/view_skip_time.json)")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    a = ap.parse_args()
    import cnr_amd as cnr
    import view_scene as VS
    assert torch.cuda.is_available(), "time_view needs the GPU"
    dev = torch.device("cuda:0")
    cfg = cnr.cfg.synthetic_config(device=str(dev), latent_dim=32)
    cfg.min_depth, cfg.max_depth = VS.ZMIN, VS.ZMAX
    cls_dict, scene_bg = VS.make_scene(cnr, cfg, seed=1, n_multi=2, n_obj=4, single=False, bg_hidden=128, spread=1.2)
    r = cnr.view.SceneRenderer(cls_dict, scene_bg, cfg)
    T, S, P = VS.camera_pose(), a.samples, cfg.W * cfg.H
    if a.skip:
        return skip_leg(a, cnr, r, scene_bg, T, S, dev)
    rows = {}
    for bg_precision in ("fp32", "fused"):
        scene_bg.trainer.eval_precision = bg_precision
        rows[bg_precision] = time_render(r, T, S, a.reps)
        print(bg_precision, json.dumps(rows[bg_precision]))
    # the composite alone, whole image in one chunk, kernel against the torch form
    scene_bg.trainer.eval_precision = "fused"
    with torch.no_grad():
        full = r.render(T, n_samples=S, chunk=P, return_samples=True)
    s = full["samples"]
    N = int(s["z"].shape[0])
    seg_inst = s["inst_ids"][s["seg_entity"].long()]
    out = dict(rgb=torch.empty(P, 3, device=dev), depth=torch.empty(P, device=dev), opacity=torch.empty(P, device=dev),
               var=torch.empty(P, device=dev), mass=torch.empty(P, 8, device=dev), instance=torch.empty(P, device=dev, dtype=torch.int32))

    def kernel():
        cnr._C.call("cnr_view_composite", s["sigma"], s["color"], s["z"], s["pix_segs"], s["seg_entity"], s["inst_ids"], P, S, 0.5,
                    out["rgb"], out["depth"], out["opacity"], out["var"], out["mass"], out["instance"])
        return out

    def torch_form():
        return torch_composite(s["sigma"], s["color"], s["z"], s["pix_segs"], 0.5, seg_inst)

    with torch.no_grad():
        kernel(), torch_form()
        torch.cuda.synchronize()
        tk, tt = [], []
        for _ in range(a.reps):
            ms, ok = _event_ms(kernel)
            tk.append(ms)
            ms, ot = _event_ms(torch_form)
            tt.append(ms)
    diff = {k: float((ok[k].double() - ot[k].double()).abs().max()) for k in ("rgb", "depth", "opacity", "var", "mass")}
    same_inst = float((ok["instance"] == ot["instance"]).double().mean())
    segs_per_pixel = (s["pix_segs"] >= 0).sum(1)
    comp = dict(kernel_ms=round(statistics.median(tk), 3), kernel_ms_min_max=[round(min(tk), 3), round(max(tk), 3)],
                torch_ms=round(statistics.median(tt), 3), torch_ms_min_max=[round(min(tt), 3), round(max(tt), 3)],
                torch_over_kernel=round(statistics.median(tt) / statistics.median(tk), 2),
                bytes_read=int(N * S * 20 + P * 32 + N * 4), max_abs_difference=diff, instance_agreement=same_inst)
    comp["kernel_GBps"] = round(comp["bytes_read"] / (comp["kernel_ms"] * 1e-3) / 1e9, 1)
    result = dict(tool="tools/time_view.py", device=torch.cuda.get_device_name(0), camera=[cfg.W, cfg.H], samples=S, reps=a.reps,
                  entities=len(r.entities), segments=N, segments_per_pixel_mean=round(N / P, 3),
                  segments_per_pixel_max=int(segs_per_pixel.max()), chunk=65536, render=rows, composite_whole_image=comp)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
