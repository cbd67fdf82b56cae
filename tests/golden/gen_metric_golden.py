"""Generate tests/golden/metric/*.npz by RUNNING THE REFERENCE's metric/metrics.py (build container only).

    python tests/golden/gen_metric_golden.py REFERENCE_ROOT        (the reference checkout: REFERENCE_ROOT/metric/metrics.py)

Imports the reference's metrics module at run time (numpy >= 1.24 dropped np.float, which its ratio functions use: a
`np.float = float` shim is installed first) and records, per case, the two point sets (f32) and what accuracy, completion,
accuracy_ratio, completion_ratio and chamfer return.  Thresholds are moved off any distance by more than 1e-5 so that a ratio
cannot flip between the float64 KD-tree and an fp32 distance.  Only arrays are written -- no reference source or bytecode.
Kept in the subdirectory: tests/conftest.py globs the top-level golden files as object-branch fixtures."""
import importlib.util
import os
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "metric")


def _load(ref_root):
    if not hasattr(np, "float"):
        np.float = float
    spec = importlib.util.spec_from_file_location("ref_metrics", os.path.join(ref_root, "metric", "metrics.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _sphere(n, r, rng, centre=(0.0, 0.0, 0.0), noise=0.0):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * (r + noise * rng.normal(size=(n, 1))) + np.asarray(centre)).astype(np.float32)


def _safe_th(dists, th):
    """th nudged up until no distance lies within 1e-5 of it"""
    while np.abs(np.concatenate(dists) - th).min() < 1e-5:
        th += 3.7e-5
    return th


def cases(rng):
    # object scale: two noisy spheres, equal sizes
    yield "obj_equal", _sphere(2000, 0.30, rng, noise=0.004), _sphere(2000, 0.31, rng, noise=0.004)
    # unequal sizes, a partial reconstruction (upper half only)
    rec = _sphere(3000, 0.25, rng, noise=0.01)
    yield "obj_partial_unequal", _sphere(1500, 0.25, rng), rec[rec[:, 2] > -0.05]
    # scene coordinates several metres from the origin, centimetre offsets
    c = (4.5, -3.2, 1.4)
    yield "scene_offset", _sphere(2500, 1.8, rng, c, noise=0.02), _sphere(1800, 1.8, rng, (4.52, -3.2, 1.41), noise=0.02)
    # duplicates and exact hits: the reconstruction contains half of the ground truth's points, twice
    gt = rng.uniform(-0.5, 0.5, (1200, 3)).astype(np.float32)
    yield "duplicates", gt, np.concatenate([gt[:600], gt[:600], rng.uniform(-0.5, 0.5, (400, 3)).astype(np.float32)])


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = _load(sys.argv[1])
    from scipy.spatial import cKDTree
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20261016)
    for name, gt, rec in cases(rng):
        g, r = gt.astype(np.float64), rec.astype(np.float64)
        d_rec = cKDTree(g).query(r)[0]
        d_gt = cKDTree(r).query(g)[0]
        th_acc = _safe_th([d_rec], 0.01)
        th_comp = _safe_th([d_gt], 0.05)
        out = dict(gt=gt, rec=rec, th_acc=np.float64(th_acc), th_comp=np.float64(th_comp),
                   accuracy=np.float64(ref.accuracy(g, r)), completion=np.float64(ref.completion(g, r)),
                   accuracy_ratio=np.float64(ref.accuracy_ratio(g, r, th_acc)),
                   completion_ratio=np.float64(ref.completion_ratio(g, r, th_comp)), chamfer=np.float64(ref.chamfer(g, r)))
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
        print(name, len(gt), len(rec), {k: float(v) for k, v in out.items() if v.ndim == 0})


if __name__ == "__main__":
    main()
