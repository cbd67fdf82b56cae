"""Times Trainer.meshing for one CodeNeRF object (multi-object branch) at grid_dim 64 / 128 / 256 on the GPU: the grid
evaluation (make_3D_grid + ONE precise cnr_field_fwd launch), marching-cubes count (classify + scan), emit (vertices + faces),
the colour pass (eval_points at the vertices) and the whole call, by device events after warm-up; V and F.
The weights are trained for --steps fused steps on tests/scene_synth.py so the surface is a real one.

    python tools/time_meshing.py [--steps 400] [--reps 10] [--out FILE.json]"""
import argparse
import json
import os
import sys

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
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, out


def trained_trainer(cnr, dev, steps):
    """a CodeNeRF Trainer of four objects whose weights were trained for `steps` fused steps on tests/scene_synth.py
    (tools/time_meshclean.py meshes the same one)"""
    from scene_synth import analytic_pool, sphere_radius
    torch.manual_seed(99)
    cfg = cnr.cfg.synthetic_config(device=str(dev), latent_dim=32, n_bins_cam2surface=4, n_bins=28)
    gen = torch.Generator().manual_seed(11)
    ft = cnr.fused.FusedCategoryTrainer(cfg, 1, 4, [analytic_pool(64 * 512, 4, gen)], 512, dev, seed=7, generator=gen)
    ft.run(steps)
    torch.cuda.synchronize()
    sd = ft.state_dicts(0)
    t = cnr.trainer.Trainer(cfg, 3, [0, 1, 2, 3])
    with torch.no_grad():
        t.fc_occ_map.load_state_dict(sd["FC_state_dict"])
        t.pe.B_layer.weight.copy_(sd["PE_state_dict"]["B_layer.weight"])
        t.shape_codes.weight.copy_(sd["shape_code_state_dict"]["weight"])
        t.texture_codes.weight.copy_(sd["texture_code_state_dict"]["weight"])
    t.extent_dict = {k: np.full(3, 2.4 * sphere_radius(k)) for k in range(4)}
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--dims", default="64,128,256")
    ap.add_argument("--out", default=None, help="also write the rows as JSON to this file")
    a = ap.parse_args()
    import cnr_amd as cnr
    assert torch.cuda.is_available(), "time_meshing needs the GPU"
    dev = torch.device("cuda:0")
    t = trained_trainer(cnr, dev, a.steps)
    inst = 2
    ext = t.extent_dict[inst]
    scale = torch.from_numpy((ext / np.max(ext / 2)) / (2.0 * t.bound_extent)).float().to(dev)
    rows = []
    for D in (int(d) for d in a.dims.split(",")):
        def grid_eval():
            g = cnr.render_rays.make_3D_grid([-1.0, 1.0], D, dev, scale=scale).view(-1, 3)
            return t._grid_occupancy(g, inst)
        ms_grid, occ = _ms(grid_eval, a.reps)
        vol = occ.view(D, D, D).contiguous()
        ws = torch.empty(int(cnr._C.load().cnr_mc_workspace_bytes(D)), device=dev, dtype=torch.uint8)
        counts = torch.empty(2, device=dev, dtype=torch.int64)
        ms_count, _ = _ms(lambda: cnr._C.call("cnr_mc_count", vol, D, 0.5, ws, counts), a.reps)
        V, F = (int(x) for x in counts.cpu())
        verts, normals = torch.empty(V, 3, device=dev), torch.empty(V, 3, device=dev)
        faces = torch.empty(F, 3, device=dev, dtype=torch.int32)
        ms_emit, _ = _ms(lambda: cnr._C.call("cnr_mc_emit", vol, D, 0.5, 1, ws, verts, normals, faces), a.reps)
        mesh = t.meshing(inst, grid_dim=D)
        vpts = torch.from_numpy(mesh.vertices).float().to(dev)
        ms_colour, _ = _ms(lambda: t.eval_points(vpts, inst_id=inst), a.reps)
        ms_total, _ = _ms(lambda: t.meshing(inst, grid_dim=D), a.reps)
        rec = dict(grid_dim=D, V=V, F=F, ms_grid_eval=round(ms_grid, 3), ms_mc_count=round(ms_count, 3),
                   ms_mc_emit=round(ms_emit, 3), ms_colour=round(ms_colour, 3), ms_meshing_total=round(ms_total, 3))
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    if not a.out:
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), steps=a.steps, reps=a.reps, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
