"""Times SceneRenderer.render on the GPU: the 1200 x 680 Replica camera, a synthetic scene of a background (hidden size 128)
and 2 categories x 4 objects (random-init weights: the timing does not depend on what the fields hold, only the instance
statistics do), S = 64 samples per segment.  By device events after warm-up, medians over --reps renders:

  * the stages of one render, summed over its pixel chunks: segments (count + emit, including the two small device-to-host
    reads of the counts), points, every field evaluation, composite;
  * the whole render by a host clock around a device synchronise, and pixels per second;
  * cnr_view_composite alone on the arrays of the whole image, against the same composite written with torch ops on the
    device (gather the segments of a pixel, stable sort by z, cumprod, sums), alternating the two, and the largest
    difference between their results.

    python tools/time_view.py [--reps 9] [--samples 64] [--out profiles/view_time.json]"""
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


def main():
    ap = argparse.ArgumentParser()
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
    rows = {}
    for bg_precision in ("fp32", "fused"):
        scene_bg.trainer.eval_precision = bg_precision
        with torch.no_grad():
            r.render(T, n_samples=S)                                    # warm-up: code objects, allocator
            torch.cuda.synchronize()
            stages, wall = {}, []
            for _ in range(a.reps):
                r.stage_events = []
                t0 = time.perf_counter()
                r.render(T, n_samples=S)
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
                ev, tot = r.stage_events, {}
                for (_, e0), (name, e1) in zip(ev[:-1], ev[1:]):
                    if name != "start":
                        tot[name] = tot.get(name, 0.0) + e0.elapsed_time(e1)
                for k, v in tot.items():
                    stages.setdefault(k, []).append(v)
                r.stage_events = None
        rows[bg_precision] = dict(stage_ms={k: round(statistics.median(v), 3) for k, v in stages.items()},
                                  render_ms=round(statistics.median(wall), 3),
                                  render_ms_min_max=[round(min(wall), 3), round(max(wall), 3)],
                                  pixels_per_s=round(P / (statistics.median(wall) * 1e-3)))
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
