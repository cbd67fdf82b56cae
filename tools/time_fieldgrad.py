"""Times the field-gradient kernels on the GPU, by device events after warm-up, medians over --reps:

  * cnr_field_grad (one category, per-point rows of 4 objects) and cnr_occmap_grad (hidden 32 and 128) at N = 816 000 points
    (one 1200 x 680 image), each against autograd through the drop-in modules on the same points, alternating the two, with
    the largest difference between their gradients; FLOP counted from the shapes (a multiply-add = 2, four channels per
    weight: the value and three tangents), against the 157.3 TFLOP/s fp32 vector peak;
  * SceneRenderer.render with and without normals=True on the scene tools/time_view.py uses, alternating, by a host clock
    around a device synchronise, and the added stages by device events.

    python tools/time_fieldgrad.py [--reps 9] [--points 816000] [--out profiles/fieldgrad_time.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

PEAK_FP32_VECTOR = 157.3e12


def flop_per_point(H, category):
    """2 x 4 x the weights of the geometry branch's layers (value + 3 tangents each), the head included"""
    w = 87 * H + H * H + (H + 87) * H + H * H + H
    if category:
        w += H * H                      # encoding_shape
    return 8 * w


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def _pair(kernel, autograd, reps):
    kernel(), autograd()
    torch.cuda.synchronize()
    tk, ta = [], []
    for _ in range(reps):
        ms, gk = _event_ms(kernel)
        tk.append(ms)
        ms, ga = _event_ms(autograd)
        ta.append(ms)
    # (a point next to a ReLU kink may get its mask the other way in the two evaluations: its gradient then differs by a whole
    #  term, which is what the largest difference shows; the median and the share above 1e-4 say how rare that is)
    rel = (gk - ga).norm(dim=-1) / ga.norm(dim=-1).clamp_min(1e-30)
    return tk, ta, dict(max_abs_difference=float((gk - ga).abs().max()), median_relative_difference=float(rel.median()),
                        share_relative_difference_above_1e_4=float((rel > 1e-4).double().mean()))


def _row(tk, ta, N, flop, diff):
    k, a = statistics.median(tk), statistics.median(ta)
    tf = N * flop / (k * 1e-3) / 1e12
    return dict(kernel_ms=round(k, 3), kernel_ms_min_max=[round(min(tk), 3), round(max(tk), 3)], autograd_ms=round(a, 3),
                autograd_ms_min_max=[round(min(ta), 3), round(max(ta), 3)], autograd_over_kernel=round(a / k, 2),
                flop_per_point=flop, kernel_TFLOPs=round(tf, 2), share_of_fp32_vector_peak=round(tf * 1e12 / PEAK_FP32_VECTOR, 4),
                points_per_s=round(N / (k * 1e-3)), **diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--points", type=int, default=816000)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import cnr_amd as cnr
    import view_scene as VS
    assert torch.cuda.is_available(), "time_fieldgrad needs the GPU"
    dev = torch.device("cuda:0")
    N = a.points
    cfg = cnr.cfg.synthetic_config(device=str(dev), latent_dim=32)
    cfg.min_depth, cfg.max_depth = VS.ZMIN, VS.ZMAX
    cls_dict, scene_bg = VS.make_scene(cnr, cfg, seed=1, n_multi=2, n_obj=4, single=False, bg_hidden=128, spread=1.2)
    g = torch.Generator(device=dev).manual_seed(7)
    pts = (torch.rand(N, 3, device=dev, generator=g) * 2 - 1).contiguous()
    kernels = {}

    # one category, rows of its 4 objects changing from point to point
    t = cls_dict[10].trainer
    with torch.no_grad():
        rows = [t._codenerf_rows(i) for i in cls_dict[10].obj_ids]
        trunk, B = rows[0][0], rows[0][1]
        brows = torch.cat([r[2] for r in rows], 0).contiguous()
    row = (torch.arange(N, device=dev) % 4).int()
    idx = row.long()
    cs, ct = t.shape_codes.weight.detach()[idx][:, None, :], t.texture_codes.weight.detach()[idx][:, None, :]

    def cat_kernel():
        return cnr.ops.field_grad(pts, B, trunk, brows, row, t.pe._scale)[1]

    def cat_autograd():
        x = pts.clone().requires_grad_(True)
        sig, _ = t.fc_occ_map(t.pe(x[:, None, :]), cs, ct)
        return torch.autograd.grad(sig.sum(), x)[0]

    tk, ta, diff = _pair(cat_kernel, cat_autograd, a.reps)
    kernels["cnr_field_grad"] = _row(tk, ta, N, flop_per_point(32, True), diff)
    print("cnr_field_grad", json.dumps(kernels["cnr_field_grad"]))

    for H in (32, 128):
        bg_cfg = cnr.cfg.synthetic_config(device=str(dev), latent_dim=32)
        bg_cfg.hidden_feature_size = H
        torch.manual_seed(H)
        tb = cnr.trainer.Trainer(bg_cfg, 0, [0])
        span = (pts * float(tb.pe._scale)).contiguous()       # x / scale in [-1, 1]

        def occ_kernel():
            return cnr.ops.occmap_grad(tb.fc_occ_map, tb.pe, span)[1]

        def occ_autograd():
            x = span.clone().requires_grad_(True)
            sig = tb.fc_occ_map(tb.pe(x[:, None, :]), do_color=False)[0]
            return torch.autograd.grad(sig.sum(), x)[0]

        tk, ta, diff = _pair(occ_kernel, occ_autograd, a.reps)
        kernels["cnr_occmap_grad_h{}".format(H)] = _row(tk, ta, N, flop_per_point(H, False), diff)
        print("cnr_occmap_grad H =", H, json.dumps(kernels["cnr_occmap_grad_h{}".format(H)]))

    # the render with and without the normal image
    r = cnr.view.SceneRenderer(cls_dict, scene_bg, cfg)
    T, S = VS.camera_pose(), a.samples
    scene_bg.trainer.eval_precision = "fused"
    render = {}
    with torch.no_grad():
        r.render(T, n_samples=S), r.render(T, n_samples=S, normals=True)
        torch.cuda.synchronize()
        wall = {False: [], True: []}
        stages = {}
        for _ in range(a.reps):
            for normals in (False, True):
                r.stage_events = [] if normals else None
                t0 = time.perf_counter()
                out = r.render(T, n_samples=S, normals=normals)
                torch.cuda.synchronize()
                wall[normals].append((time.perf_counter() - t0) * 1e3)
                if normals:
                    ev, tot = r.stage_events, {}
                    for (_, e0), (name, e1) in zip(ev[:-1], ev[1:]):
                        if name.startswith(("surface", "gradient", "normals")):
                            tot[name] = tot.get(name, 0.0) + e0.elapsed_time(e1)
                    for k, v in tot.items():
                        stages.setdefault(k, []).append(v)
                    r.stage_events = None
    for normals in (False, True):
        w = wall[normals]
        render["normals" if normals else "plain"] = dict(render_ms=round(statistics.median(w), 3),
                                                         render_ms_min_max=[round(min(w), 3), round(max(w), 3)])
    render["added_ms"] = round(render["normals"]["render_ms"] - render["plain"]["render_ms"], 3)
    render["normal_stage_ms"] = {k: round(statistics.median(v), 3) for k, v in stages.items()}
    render["surface_pixels"] = int((out["instance"] >= 0).sum())
    print("render", json.dumps(render))
    result = dict(tool="tools/time_fieldgrad.py", device=torch.cuda.get_device_name(0), points=N, reps=a.reps,
                  peak_fp32_vector_TFLOPs=PEAK_FP32_VECTOR / 1e12, kernels=kernels, camera=[cfg.W, cfg.H], samples=S,
                  entities=len(r.entities), background_precision="fused", render=render)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
