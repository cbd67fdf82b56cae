"""Times ScanNet mask refinement (cnr_amd.utils.refine_frame: geometry segmentation and the overlap vote, csrc/geoseg.hip) on the
GPU at 620 x 460, a ScanNet depth frame after the 10-pixel crop, on the synthetic room of tests/geoseg_cpu.py (a slanted floor,
a wall, a sphere, pixels without depth) with a raw instance map of a few rectangles.  By device events after warm-up, medians
over --reps runs:

  * the stages of one frame: point map, normals (hybrid search + eigenvectors), maps, edge map, labelling, counts + growth,
    segment selection, hole filling, vote; the normals' share of their sum;
  * the whole refine_frame by a host clock around a device synchronise;
  * the image stages (everything but the point map and the normals, which it takes from the GPU) of the numpy restatement
    tests/geoseg_cpu.py, with scipy.ndimage doing its labelling and hole filling, on this box's CPU threads.  The restatement's
    normals are a brute-force search over all pairs and are not timed at this size.

    python tools/time_geoseg.py [--reps 7] [--out profiles/geoseg_time.json]"""
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

W, H = 620, 460
FX = FY = 577.87                       # ScanNet's depth camera
CX, CY = 319.5 - 10, 239.5 - 10


class Intrinsic:
    fx, fy, cx, cy = FX, FY, CX, CY


def ccl_scipy(mask, connectivity):
    """tests/geoseg_cpu.ccl's labels from scipy.ndimage.label: every component named by its smallest raster index"""
    import scipy.ndimage as ndi
    mask = np.asarray(mask) != 0
    lab, n = ndi.label(mask, structure=np.ones((3, 3)) if connectivity == 8 else None)
    if n == 0:
        return np.full(mask.shape, -1, np.int32)
    first = ndi.minimum(np.arange(mask.size).reshape(mask.shape), lab, index=np.arange(1, n + 1)).astype(np.int32)
    return np.where(lab > 0, first[np.maximum(lab, 1) - 1], -1).astype(np.int32)


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def stages_once(U, depth, inst):
    """one frame stage by stage, synchronised between the stages -> ({stage: ms}, results)"""
    from cnr_amd import _C
    ms = {}
    ms["point_map"], (P, valid) = _timed(lambda: U._geoseg_point_map(depth, Intrinsic))
    pts = P[valid]

    def normals():
        n = U.estimate_normals_device(pts, U.GEOSEG_NORMAL_RADIUS, U.GEOSEG_NORMAL_MAX_NN)
        n = torch.where(n[:, 2:] > 0, -n, n)
        N = torch.zeros_like(P)
        N[valid] = n.float()
        return N

    ms["normals"], N = _timed(normals)
    ms["maps"], (disc, conv) = _timed(lambda: U.geoseg_maps(P, N, depth))
    ms["edge_map"], edge = _timed(lambda: U.geoseg_edge_map(disc, conv, depth))
    ms["labelling"], labels = _timed(lambda: U.connected_components(edge, 8, check=False))
    ms["counts_growth"], grown = _timed(lambda: U.geoseg_grow(P, depth, edge, labels, U.label_counts(labels), 500))
    ms["segment_selection"], seg_ids = _timed(
        lambda: torch.nonzero(U.label_counts(grown).reshape(-1) >= 500).reshape(-1).to(torch.int32).contiguous())
    K = len(seg_ids)
    ms["fill_holes"], (filled, err) = _timed(lambda: U._fill_holes_stack(grown, seg_ids, None, K, H, W, depth.device))
    ms["vote"], refined = _timed(lambda: U._vote(inst, filled, 0.7))
    assert int(err.item()) == 0
    return ms, dict(P=P, N=N, grown=grown, seg_ids=seg_ids, refined=refined, K=K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_geoseg.py measures on the GPU; none is present")
    import cnr_amd
    import geoseg_cpu as G
    U = cnr_amd.utils
    dev = torch.device("cuda:0")
    depth_np, _ = G.room_depth(H, W, FX, FY, CX, CY, n_holes=600, seed=9)
    inst_np = np.zeros((H, W), np.int32)
    inst_np[60:300, 40:330], inst_np[330:450, 20:600], inst_np[20:120, 400:600], inst_np[150:260, 420:580] = 3, 5, 7, 9
    depth, inst = torch.from_numpy(depth_np).to(dev), torch.from_numpy(inst_np).to(dev)
    for _ in range(2):                                          # warm-up: code objects, the allocator's pools
        _, res = stages_once(U, depth, inst)
        U.refine_frame(depth, inst, Intrinsic)
    torch.cuda.synchronize()
    runs, whole = [], []
    for _ in range(args.reps):
        runs.append(stages_once(U, depth, inst)[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        refined = U.refine_frame(depth, inst, Intrinsic)
        torch.cuda.synchronize()
        whole.append(1e3 * (time.perf_counter() - t0))
    assert torch.equal(refined, res["refined"])
    stage_ms = {k: round(statistics.median(r[k] for r in runs), 3) for k in runs[0]}
    total = sum(stage_ms.values())
    # the restatement's image stages on the CPU, from the GPU's point map and normals
    import scipy.ndimage as ndi
    P_np, N_np = res["P"].cpu().numpy(), res["N"].cpu().numpy()
    cpu = {}
    t0 = time.perf_counter()
    seg = G.segmentation(P_np, N_np, depth_np, 500, 500, ccl_fn=ccl_scipy)
    cpu["maps_to_segments"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    filled = [ndi.binary_fill_holes(m) for m in seg["masks"]]
    cpu["fill_holes"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    want, _ = G.vote(inst_np, filled)
    cpu["vote"] = time.perf_counter() - t0
    same = bool(np.array_equal(want, refined.cpu().numpy()) and np.array_equal(seg["grown"], res["grown"].cpu().numpy()))
    gpu_image_ms = total - stage_ms["point_map"] - stage_ms["normals"]
    out = dict(tool="tools/time_geoseg.py", device=torch.cuda.get_device_name(0), frame=[W, H], reps=args.reps,
               valid_pixels=int((depth_np > 0).sum()), segments=res["K"], refined_ids=np.unique(want).tolist(),
               stage_ms=stage_ms, stages_sum_ms=round(total, 3), normals_share=round(stage_ms["normals"] / total, 4),
               refine_frame_ms=round(statistics.median(whole), 3), refine_frame_ms_min_max=[round(min(whole), 3), round(max(whole), 3)],
               image_stages_ms=round(gpu_image_ms, 3),
               restatement_cpu=dict(threads=torch.get_num_threads(), stage_s={k: round(v, 4) for k, v in cpu.items()},
                                    image_stages_s=round(sum(cpu.values()), 4), normals="not measured (all-pairs search)",
                                    equals_gpu=same),
               image_stages_speedup=round(1e3 * sum(cpu.values()) / gpu_image_ms, 1))
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
