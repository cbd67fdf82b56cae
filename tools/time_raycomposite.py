"""Times the kernels that composite rays with two builds of libcnr_hip.so on one GPU, the two alternating:

    python tools/time_raycomposite.py --parent-lib PARENT.so [--runs 5] [--parts micro,bench,bg,objfields,codefit] --out FILE.json

Every run is a fresh process with CNR_HIP_LIB set to one of the libraries (parent, branch, branch, parent, ...).
  micro      one process times, by device events, 300 back-to-back launches after 20 of warm-up of cnr_composite_fwd,
             cnr_composite_bwd and cnr_render_loss at C x R x S = 1 x 2048 x 64 and 1 x 2048 x 200, cnr_loss_fwd_bwd at 4 x 2048 and
             cnr_field_fwd_render at 4 x 2048 x 64 (us per launch);
  bg, objfields, codefit   tools/time_bg.py, tools/time_objfields.py, tools/time_codefit.py (us / ms per step);
  bench      bench.py --gpus 1 --steps 20 --warmup 5, its main figure (rays/s), twice per side.
Per row and side: the runs, their median and spread (max - min).  A row passes when the branch's median is no slower than the
parent's median plus the parent's spread.  --out is merged into when it exists, so the parts can be run in several calls.
`--child` is the micro process itself."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, LAUNCHES = 20, 300


def child():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    import cnr_amd
    _C = cnr_amd._C
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    f = lambda *s: torch.empty(*s, device=dev)

    def window(fn):
        for _ in range(WARMUP):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(LAUNCHES):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / LAUNCHES * 1e3

    def rays(C, R, S):
        sig, col = (torch.randn(C, R, S, generator=gen) * 3).to(dev), torch.rand(C, R, S, 3, generator=gen).to(dev)
        z = (torch.rand(C, R, S, generator=gen).sort(dim=-1).values * 4 + 0.1).to(dev)
        gt_d, gt_c = (torch.rand(C, R, generator=gen) * 4).to(dev), torch.rand(C, R, 3, generator=gen).to(dev)
        labels = torch.randint(0, 3, (C, R), generator=gen).to(torch.uint8).to(dev)
        dmask = (torch.rand(C, R, generator=gen) > 0.2).to(torch.uint8).to(dev)
        return sig, col, z, gt_d, gt_c, labels, dmask

    rows = {}
    for C, R, S in ((1, 2048, 64), (1, 2048, 200)):
        sig, col, z, gt_d, gt_c, labels, dmask = rays(C, R, S)
        depth, var, rgb, opa, dsig, dcol = f(C, R), f(C, R), f(C, R, 3), f(C, R), f(C, R, S), f(C, R, S, 3)
        dd, dr, do = torch.randn(C, R, device=dev), torch.randn(C, R, 3, device=dev), torch.randn(C, R, device=dev)
        ws = torch.zeros(_C.render_loss_workspace_bytes(C, R), device=dev, dtype=torch.uint8)
        tag = "%dx%dx%d" % (C, R, S)
        rows["cnr_composite_fwd " + tag] = window(
            lambda: _C.call("cnr_composite_fwd", sig, col, z, None, depth, var, rgb, opa, C * R, S, 0))
        rows["cnr_composite_bwd " + tag] = window(
            lambda: _C.call("cnr_composite_bwd", sig, col, z, dd, dr, do, None, dsig, dcol, C * R, S, 0))
        rows["cnr_render_loss " + tag] = window(
            lambda: _C.call("cnr_render_loss", sig, col, z, gt_d, gt_c, labels, dmask, 5.0, 10.0, 1.0, dsig, dcol, depth, var, rgb,
                            opa, C, R, S, ws, ws.numel(), None, None))
    C, R = 4, 2048
    _, _, _, gt_d, gt_c, labels, dmask = rays(C, R, 1)
    depth, var, rgb, opa = gt_d + torch.randn(C, R, device=dev), torch.rand(C, R, device=dev), torch.rand(C, R, 3, device=dev), \
        torch.rand(C, R, device=dev)
    losses, flags, dd, dr, do = f(3, C), torch.empty(C, device=dev, dtype=torch.int32), f(C, R), f(C, R, 3), f(C, R)
    rows["cnr_loss_fwd_bwd 4x2048"] = window(
        lambda: _C.call("cnr_loss_fwd_bwd", depth, var, rgb, opa, gt_d, gt_c, labels, dmask, 5.0, 10.0, 1.0, losses, flags, dd, dr,
                        do, C, R))
    S, n_obj = 64, 4
    _, _, z, gt_d, gt_c, labels, dmask = rays(C, R, S)
    theta, lay = cnr_amd.fused.init_params(C, 32, n_obj, gen, dev)
    v = lay.views(theta)
    trunk, B = v["trunk"].contiguous(), v["B"].contiguous()
    packed, lo = cnr_amd.ops.pack_weights(trunk), cnr_amd.ops.pack_weights_lo(trunk)
    brows = (torch.randn(C * n_obj, 4, 32, generator=gen) * 0.1).to(dev)
    ray_row = (torch.randint(0, n_obj, (C, R), generator=gen) + torch.arange(C)[:, None] * n_obj).to(torch.int32).to(dev)
    pts = (torch.rand(C, R, S, 3, generator=gen) * 2 - 1).to(dev)
    ws = torch.zeros(int(_C.load().cnr_field_fwd_render_workspace_bytes(C, R, S)), device=dev, dtype=torch.uint8)
    depth, var, rgb, opa, dsig, dcol = f(C, R), f(C, R), f(C, R, 3), f(C, R), f(C, R, S), f(C, R, S, 3)
    rows["cnr_field_fwd_render 4x2048x64"] = window(
        lambda: _C.call("cnr_field_fwd_render", pts, B, packed, brows, ray_row, 2.0, z, gt_d, gt_c, labels, dmask, 5.0, 10.0, 1.0,
                        dsig, dcol, depth, var, rgb, opa, C, R, S, 0, ws, ws.numel(), lo, None, None))
    print("ROWS " + json.dumps(rows))


def run(cmd, lib, limit):
    """one process under a time limit with CNR_HIP_LIB = lib -> its standard output; any failure ends the whole measurement"""
    env = dict(os.environ, CNR_HIP_LIB=lib)
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit("%s with %s ended with status %d: nothing more is started" % (" ".join(cmd), lib, p.returncode))
    return p.stdout


def part_rows(part, lib):
    """-> {row: (value, unit, higher_is_better)} of one run of `part` with library `lib`"""
    py = sys.executable
    if part == "micro":
        out = run([py, os.path.abspath(__file__), "--child"], lib, 300)
        return {k: (v, "us", False) for k, v in json.loads(re.search(r"^ROWS (.*)$", out, re.M).group(1)).items()}
    if part == "bg":
        out = run([py, "tools/time_bg.py", "fused"], lib, 300)
        rows = {"time_bg fused step": (float(re.search(r"background step ([0-9.]+) us", out).group(1)), "us", False)}
        for k, v in json.loads(re.search(r"^(\{.*\})$", out, re.M).group(1).replace("'", '"')).items():
            rows["time_bg " + k] = (v, "us", False)
        return rows
    if part in ("objfields", "codefit"):
        out = run([py, "tools/time_%s.py" % part, "--sizes", "64", "--modular-max", "0", "--rounds", "5"], lib, 300)
        return {"time_%s 64 fused step" % part: (json.loads(re.search(r"^64 (\{.*\})$", out, re.M).group(1))["fused_ms"], "ms", False)}
    assert part == "bench", part
    out = run([py, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], lib, 600)
    res = [json.loads(l) for l in out.splitlines() if l.startswith("{") and '"metric"' in l]
    return {"bench.py " + res[-1]["metric"][:40]: (res[-1]["value"], res[-1]["unit"], True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--branch-lib", default=os.path.join(ROOT, "category-nerf-reconstruction-official_amd", "libcnr_hip.so"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parts", default="micro,bench,bg,objfields,codefit")
    ap.add_argument("--out", required=False)
    a = ap.parse_args()
    if a.child:
        return child()
    libs = {"parent": os.path.abspath(a.parent_lib), "branch": os.path.abspath(a.branch_lib)}
    result = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {"rows": {}}
    for part in a.parts.split(","):
        runs = 2 if part == "bench" else a.runs
        got = {}
        for i in range(runs):
            for side in (("parent", "branch") if i % 2 == 0 else ("branch", "parent")):     # neither side always runs second
                for k, (v, unit, up) in part_rows(part, libs[side]).items():
                    got.setdefault(k, dict(unit=unit, higher_is_better=up, parent=[], branch=[]))[side].append(v)
                print(part, "run", i, side, "done", flush=True)
        for k, r in got.items():
            pm, bm = statistics.median(r["parent"]), statistics.median(r["branch"])
            spread = max(r["parent"]) - min(r["parent"])
            r.update(parent_median=pm, branch_median=bm, parent_spread=spread,
                     ok=bool(bm >= pm - spread if r["higher_is_better"] else bm <= pm + spread))
            result["rows"][k] = r
            print("%-44s parent %.4g branch %.4g %s (parent spread %.3g) %s" % (k, pm, bm, r["unit"], spread, "ok" if r["ok"] else "MISS"),
                  flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            result["rule"] = "branch median no slower than parent median + parent spread (max - min of its runs)"
            result["launches_per_window"] = LAUNCHES
            with open(a.out, "w") as fo:
                json.dump(result, fo, indent=1)


if __name__ == "__main__":
    main()
