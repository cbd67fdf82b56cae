"""GPU: the kernels of csrc/pointcloud.hip against the numpy / scipy restatement tests/registration_cpu.py:
unprojection and accumulation on the committed Replica frames, the voxel down-sample, the nearest neighbour with its index,
and the ICP step's 17 sums and rigid update."""
import json
import os

import numpy as np
import pytest
import torch

import registration_cpu as RC
from test_dataset_host import DS, _config

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cnr():
    import cnr_amd
    return cnr_amd


def _replica(cnr):
    cfg = _config(cnr, "replica")
    z = np.load(os.path.join(DS, "replica_samples.npz"))
    samples = {int(f): {"image": z["image"][i], "depth": z["depth"][i], "obj_mask": z["obj_mask"][i], "T": z["T"][i],
                        "frame_id": int(z["frame_id"][i])} for i, f in enumerate(z["frames"])}
    with open(os.path.join(DS, "replica_frames.json")) as f:
        rec = json.load(f)
    insts = []
    for row in rec["inst_dict"]:
        if row["cls"] == 0:
            insts.append((0, 0, [{"frame": f} for f, _ in row["frame_info"]]))
        for i in row["insts"]:
            if row["cls"] != 0:
                insts.append((row["cls"], i["inst"], [{"frame": f} for f, _ in i["frame_info"]]))
    return cfg, samples, insts


def test_unproject_and_accumulate_on_the_replica_fixture_gpu(dev, cnr):
    """Kept pixels: integer logic, equal.  Coordinates: the kernel evaluates the point in fp64 and rounds once to fp32, so it
    is within half an fp32 ulp of the fp64 restatement plus the restatement's own fp64 error.  Below 16 m an ulp is 2^-20 m =
    9.5e-7 m (1.9e-6 m for a handful of fp32 operations, had the kernel worked in fp32); the bound is 1e-5 m."""
    cfg, samples, insts = _replica(cnr)
    K = cnr.dataset.PinholeIntrinsics(cfg.W, cfg.H, cfg.fx, cfg.fy, cfg.cx, cfg.cy)
    assert len(insts) == 6
    for cls, inst, info in insts:
        want_p, want_c, want_n = [], [], []
        for fi in info:
            idx, p, c = RC.unproject(samples[fi["frame"]], inst, cfg.fx, cfg.fy, cfg.cx, cfg.cy)
            want_p.append(p), want_c.append(c), want_n.append(len(idx))
        want_p, want_c = np.concatenate(want_p), np.concatenate(want_c)
        assert np.abs(want_p).max() < 16.0
        frames = [(samples[fi["frame"]]["image"], samples[fi["frame"]]["depth"], samples[fi["frame"]]["obj_mask"],
                   samples[fi["frame"]]["T"]) for fi in info]
        pc = cnr.utils._unproject_frames(frames, [inst] * len(frames), K, dev)
        # the kept-pixel sets: the same count per frame and, pixel by pixel in order, the same colour and depth-derived point
        assert len(pc) == sum(want_n) > 0, (cls, inst)
        assert [len(cnr.utils._unproject_frames([fr], [inst], K, dev)) for fr in frames] == want_n, (cls, inst)
        got = pc.points
        err = np.abs(got - want_p).max()
        print("instance", cls, inst, "points", len(pc), "max coordinate error %.3g m" % err)
        assert err < 1e-5, (cls, inst, err)
        assert np.array_equal(pc.colors_device.cpu().numpy(), want_c.astype(np.float32))
        # accumulate_pointcloud = the same cloud down-sampled to 1 cm
        acc = cnr.utils.accumulate_pointcloud(inst, info, samples, K)
        m, mc, _, _ = RC.voxel_down_sample(pc.points_device.cpu().numpy(), pc.colors_device.cpu().numpy(), 0.01)
        assert np.array_equal(acc.points_device.cpu().numpy(), m.astype(np.float32))
        assert np.array_equal(acc.colors_device.cpu().numpy(), mc.astype(np.float32))


def test_unproject_depth_limits_and_order_gpu(dev, cnr):
    """0 < depth <= 8.0 exactly, and the single-frame wrapper inverts the extrinsic it is given"""
    W, H = 7, 5
    depth = np.zeros((W, H), np.float32)
    depth[1, 2], depth[2, 0], depth[3, 3], depth[4, 4], depth[6, 1] = 8.0, np.nextafter(np.float32(8.0), np.float32(9)), 1.5, -1.0, 0.25
    rgb = np.arange(W * H * 3, dtype=np.uint8).reshape(W, H, 3)
    T_WC = np.eye(4)
    T_WC[:3, 3] = [0.5, -1.0, 2.0]
    pc = cnr.utils.unproject_colored_pointcloud(rgb, depth, np.array([[10.0, 0, 3.0], [0, 20.0, 2.0], [0, 0, 1.0]]),
                                                np.linalg.inv(T_WC), device=dev)
    kept = [(1, 2), (3, 3), (6, 1)]                           # u-major order
    want = np.array([[(u - 3.0) * depth[u, v] / 10.0 + 0.5, (v - 2.0) * depth[u, v] / 20.0 - 1.0, depth[u, v] + 2.0] for u, v in kept])
    assert np.allclose(pc.points, want, atol=1e-6) and len(pc) == 3
    assert np.array_equal(pc.colors_device.cpu().numpy(), (rgb[[1, 3, 6], [2, 3, 1]].astype(np.float64) / 255.0).astype(np.float32))


def test_unproject_with_more_than_1024_blocks_gpu(dev, cnr):
    """1100 x 960 = 1 056 000 pixels are 1032 blocks of 1024: every thread of blocks_scan_kernel owns a run of `per` = 2 block
    counts, as on a full Replica (1200 x 680) or ScanNet (1296 x 968) frame.  A third of the pixels carry the mask; depths in
    (0, 8] with zeros, values above 8 and 8 itself.  The bounds are those of the Replica fixture above: the kept pixels and
    their order equal, colours equal, coordinates (below 16 m) within 1e-5 m."""
    W, H = 1100, 960
    assert W * H > 1024 * 1024 + 1 and W * H < 1_100_000 and (W * H) % 1024 != 0
    rng = np.random.default_rng(23)
    depth = (rng.random((W, H)) * 9.0).astype(np.float32)
    depth[rng.random((W, H)) < 0.05] = 0.0
    depth[rng.random((W, H)) < 0.01] = 8.0
    mask = rng.integers(0, 3, (W, H)).astype(np.int32)
    image = rng.integers(0, 256, (W, H, 3)).astype(np.uint8)
    ang = 0.3
    T = np.eye(4)
    T[:3, :3] = [[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [0.5, -1.0, 2.0]
    fx, fy, cx, cy = 600.0, 610.0, 549.5, 479.5
    sample = {"image": image, "depth": depth, "obj_mask": mask, "T": T}
    idx, want_p, want_c = RC.unproject(sample, 1, fx, fy, cx, cy)
    assert 0.25 * W * H < len(idx) < 0.33 * W * H and np.abs(want_p).max() < 16.0
    assert (depth.reshape(-1)[idx] == 8.0).any() and (depth[mask == 1] > 8.0).any() and (depth[mask == 1] == 0.0).any()
    K = cnr.dataset.PinholeIntrinsics(W, H, fx, fy, cx, cy)
    pc = cnr.utils._unproject_frames([(image, depth, mask, T)], [1], K, dev)
    assert len(pc) == len(idx)
    err = np.abs(pc.points - want_p).max()
    print("points", len(pc), "max coordinate error %.3g m" % err)
    assert err < 1e-5, err
    assert np.array_equal(pc.colors_device.cpu().numpy(), want_c.astype(np.float32))
    again = cnr.utils._unproject_frames([(image, depth, mask, T)], [1], K, dev)
    assert torch.equal(pc.points_device, again.points_device) and torch.equal(pc.colors_device, again.colors_device)


def _check_down_sample(cnr, dev, p32, c32, voxel):
    P, C = torch.from_numpy(p32).to(dev), (torch.from_numpy(c32).to(dev) if c32 is not None else None)
    out = cnr.utils.voxel_down_sample_device(P, C, voxel)
    again = cnr.utils.voxel_down_sample_device(P, C, voxel)
    m, mc, keys, counts = RC.voxel_down_sample(p32, c32, voxel)
    assert np.array_equal(out[2].cpu().numpy(), keys) and np.array_equal(out[3].cpu().numpy(), counts)   # membership and order
    rel = np.abs(out[0].cpu().numpy() - m).max() / np.abs(m).max()
    assert rel <= 1e-12, rel
    if c32 is not None:
        assert np.abs(out[1].cpu().numpy() - mc).max() <= 1e-12 * np.abs(mc).max()
    for a, b in zip(out, again):
        if a is not None:
            assert torch.equal(a, b)                          # bit-identical run to run
    return out


def test_voxel_down_sample_gpu(dev, cnr):
    rng = np.random.default_rng(11)
    p = (rng.random((60000, 3)) * [1.2, 0.8, 0.5] + [3.0, -2.0, 0.7]).astype(np.float32)
    c = rng.random((60000, 3)).astype(np.float32)
    out = _check_down_sample(cnr, dev, p, c, 0.01)
    assert 1000 < len(out[0]) < 60000
    out = _check_down_sample(cnr, dev, p, None, 0.2)
    assert out[1] is None and int(out[3].max()) > 100         # long runs: many points per voxel
    _check_down_sample(cnr, dev, p[:1], c[:1], 0.01)


def test_voxel_down_sample_with_more_than_1024_blocks_gpu(dev, cnr):
    """1 060 001 sorted keys are 1036 blocks of 1024: blocks_scan_kernel's `per` = 2 under the voxel segments.  A 1 m cube at
    1 cm: about 650 000 occupied voxels, runs of 1 to 9 points."""
    rng = np.random.default_rng(12)
    n = 1_060_001
    assert -(-n // 1024) > 1024 and n % 1024 != 0
    p = (rng.random((n, 3)) + [3.0, -2.0, 0.7]).astype(np.float32)
    c = rng.random((n, 3)).astype(np.float32)
    out = _check_down_sample(cnr, dev, p, c, 0.01)
    assert 600_000 < len(out[0]) < 700_000 and int(out[3].sum()) == n


def test_voxel_down_sample_points_on_voxel_faces_gpu(dev, cnr):
    """voxel 0.25 and a minimum of 0.125 put the grid origin at 0: every multiple of 0.25 lies exactly on a voxel face and
    belongs to the voxel above it (floor)"""
    g = np.arange(1, 6) * 0.25
    grid = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    inner = grid[:40] + 0.1
    eps = np.nextafter(np.float32(grid[:40]), np.float32(-10))     # one ulp below the face: the voxel below
    p = np.concatenate([grid, inner, eps, [[0.125, 0.125, 0.125]]]).astype(np.float32)
    p = p[np.random.default_rng(2).permutation(len(p))]
    assert p.min() == np.float32(0.125)
    out = _check_down_sample(cnr, dev, p, None, 0.25)
    keys = out[2].cpu().numpy()
    ijk = np.stack([keys >> 42, (keys >> 21) & (2 ** 21 - 1), keys & (2 ** 21 - 1)], 1)
    assert ijk.max() == 5 and ijk.min() == 0
    with pytest.raises(ValueError):
        cnr.utils.voxel_down_sample_device(torch.tensor([[0.0, 0.0, float("nan")]], device=dev), None, 0.01)


def _nn_index(cnr, q, p):
    from cnr_amd import _C
    ws = torch.empty(int(_C.load().cnr_nn_index_workspace_bytes(len(q), len(p))), device=q.device, dtype=torch.uint8)
    d = torch.empty(len(q), device=q.device, dtype=torch.float32)
    i = torch.empty(len(q), device=q.device, dtype=torch.int32)
    _C.call("cnr_nn_index", q, len(q), p, len(p), d, i, ws)
    return d, i


@pytest.mark.parametrize("nq,nr", [(1, 1), (777, 300), (5000, 70001)])
def test_nn_index_gpu(dev, cnr, nq, nr):
    """the returned index's TRUE distance equals the brute-force minimum within the bound test_metrics_gpu.py uses for
    cnr_nn_dist: 2e-6 (1 + |q|)"""
    rng = np.random.default_rng(nq + nr)
    q = (rng.random((nq, 3)) * 3 + [5.0, -2.0, 1.0]).astype(np.float32)
    p = (rng.random((nr, 3)) * 3 + [5.0, -2.0, 1.0]).astype(np.float32)
    d, i = _nn_index(cnr, torch.from_numpy(q).to(dev), torch.from_numpy(p).to(dev))
    d, i = d.cpu().numpy(), i.cpu().numpy()
    assert i.min() >= 0 and i.max() < nr
    ref, _ = RC.cKDTree(p.astype(np.float64)).query(q.astype(np.float64))
    true = np.linalg.norm(q.astype(np.float64) - p[i].astype(np.float64), axis=1)
    tol = 2e-6 * (1 + np.linalg.norm(q.astype(np.float64), axis=1))
    assert (np.abs(true - ref) <= tol).all() and (np.abs(d - ref) <= tol).all()
    assert torch.equal(cnr.metrics.nn_dist(torch.from_numpy(q).to(dev), torch.from_numpy(p).to(dev)).cpu(), torch.from_numpy(d))


def test_nn_index_ties_go_to_the_lowest_index_gpu(dev, cnr):
    rng = np.random.default_rng(4)
    base = rng.random((900, 3)).astype(np.float32)
    p = np.concatenate([base, base, base[::-1]])              # every point three times, across tiles and chunks
    q = base[rng.permutation(900)[:500]]
    d, i = _nn_index(cnr, torch.from_numpy(q).to(dev), torch.from_numpy(p).to(dev))
    first = {tuple(v): k for k, v in reversed(list(enumerate(map(tuple, p))))}
    assert np.array_equal(i.cpu().numpy(), [first[tuple(v)] for v in q]) and float(d.abs().max()) == 0.0


def _icp_step(cnr, src, tgt, T, max_corr, state=None):
    from cnr_amd import _C
    B, n, m = len(T), len(src), len(tgt)
    dev = src.device
    ws = torch.empty(int(_C.load().cnr_icp_workspace_bytes(n, m, B)), device=dev, dtype=torch.uint8)
    sums = torch.zeros(B, 17, device=dev, dtype=torch.float64)
    d = torch.empty(B, n, device=dev, dtype=torch.float32)
    i = torch.empty(B, n, device=dev, dtype=torch.int32)
    _C.call("cnr_icp_step", src, n, tgt, m, T, B, float(max_corr), state, ws, sums, d, i)
    return sums, d, i


def _icp_case(seed=9, n=6000, m=9000, B=5):
    """a box surface sampled twice; candidate transforms near the truth and far from it.  max_corr = 0.07."""
    rng = np.random.default_rng(seed)
    surf = lambda k: np.where(rng.random((k, 3)) < 0.34, np.round(rng.random((k, 3))), rng.random((k, 3))) * [0.9, 0.6, 0.4]
    tgt = (surf(m) + [2.0, 1.0, 0.5]).astype(np.float32)
    src = (surf(n) + 0.002 * rng.standard_normal((n, 3))).astype(np.float32)
    Ts = []
    for b in range(B):
        ang, ax = 0.05 * b + (1.5 if b == B - 1 else 0.0), rng.standard_normal(3)
        ax /= np.linalg.norm(ax)
        Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        T = np.eye(4)
        T[:3, :3] = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
        T[:3, 3] = np.array([2.0, 1.0, 0.5]) + 0.02 * b * rng.standard_normal(3)
        Ts.append(T)
    return src, tgt, np.stack(Ts), 0.07


def test_icp_step_sums_and_membership_gpu(dev, cnr):
    """The 17 sums against the restatement fed the GPU's own correspondences.  Tolerance: the transformed source is an fp32
    rounding of an fp64 value, and the two fp64 evaluations (fused multiply-adds on the device, numpy's dot on the host) may
    round a point to neighbouring fp32 values: 2^-23 relative per factor, two factors in a b^T, so 4 x 2^-23 < 1e-6 of the sum
    of the absolute values of the terms (fp64 summation order adds 1e-12 of that)."""
    src, tgt, Ts, max_corr = _icp_case()
    S, G, T = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev), torch.from_numpy(Ts).to(dev)
    sums, d, i = _icp_step(cnr, S, G, T, max_corr)
    sums2, d2, i2 = _icp_step(cnr, S, G, T, max_corr)
    assert torch.equal(sums, sums2) and torch.equal(d, d2) and torch.equal(i, i2)           # bit-identical run to run
    sums, d, i = sums.cpu().numpy(), d.cpu().numpy(), i.cpu().numpy()
    tree = RC.cKDTree(tgt.astype(np.float64))
    for b, Tb in enumerate(Ts):
        want, mag = RC.icp_sums(src, tgt, Tb, i[b], d[b], max_corr)
        assert sums[b][0] == want[0]
        assert (np.abs(sums[b] - want) <= 1e-6 * mag + 1e-300).all(), (b, sums[b] - want, mag)
        # membership under max_corr against the restatement's own search: exactly, but for pairs within fp32 rounding of it
        ref_d, _ = tree.query(RC.transform32(Tb, src).astype(np.float64))
        near = np.abs(ref_d - max_corr) < 8e-6 * max_corr
        differ = (d[b] < np.float32(max_corr)) != (ref_d < max_corr)
        assert not (differ & ~near).any() and near.sum() <= 1e-3 * max(want[0], 1)
        assert (np.abs(d[b] - ref_d) <= 2e-6 * (1 + np.linalg.norm(RC.transform32(Tb, src).astype(np.float64), axis=1))).all()
        print("candidate", b, "pairs", int(want[0]), "of", len(src), "near threshold", int(near.sum()))
    assert sums[0][0] > 0.9 * len(src) and sums[-1][0] < sums[0][0]


def test_icp_update_matches_kabsch_and_freezes_gpu(dev, cnr):
    """cnr_icp_update against R = V diag(1, 1, det(V U^T)) U^T from numpy's SVD (1e-9: both are fp64, the Jacobi sweeps stop at
    1e-17 relative off-diagonal mass), open3d's convergence test, the freeze, and the whole loop against the restatement"""
    from cnr_amd import _C
    src, tgt, Ts, max_corr = _icp_case()
    S, G, T = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev), torch.from_numpy(Ts).to(dev)
    B, n = len(Ts), len(src)
    sums, _, _ = _icp_step(cnr, S, G, T, max_corr)
    state = torch.zeros(B, 4, device=dev, dtype=torch.float64)
    T1 = T.clone()
    _C.call("cnr_icp_update", sums, n, B, 100, T1, state)
    s = sums.cpu().numpy()
    for b in range(B):
        want = RC.kabsch(s[b]) @ Ts[b]
        assert np.abs(T1[b].cpu().numpy() - want).max() < 1e-9, b
        assert state[b].cpu().tolist() == [s[b][0] / n, np.sqrt(s[b][1] / s[b][0]), 0.0, 1.0]
    # a second evaluation from the SAME transforms and sums: nothing moved, so open3d's test fires and T stays
    T2 = T1.clone()
    _C.call("cnr_icp_update", sums, n, B, 100, T2, state)
    assert torch.equal(T2, T1) and state[:, 2].cpu().tolist() == [1.0] * B
    # frozen candidates are skipped by the step: their sums stay
    marked = torch.full_like(sums, -7.0)
    ws = torch.empty(int(_C.load().cnr_icp_workspace_bytes(n, len(tgt), B)), device=dev, dtype=torch.uint8)
    _C.call("cnr_icp_step", S, n, G, len(tgt), T2, B, float(max_corr), state, ws, marked, None, None)
    assert bool((marked == -7.0).all())
    # fewer than 3 pairs: flag 2, no update
    far = torch.eye(4, device=dev, dtype=torch.float64)[None].clone()
    far[0, :3, 3] = 50.0
    sums_far, _, _ = _icp_step(cnr, S, G, far, max_corr)
    st = torch.zeros(1, 4, device=dev, dtype=torch.float64)
    _C.call("cnr_icp_update", sums_far, n, 1, 100, far, st)
    assert st[0].cpu().tolist() == [0.0, 0.0, 2.0, 0.0] and float(far[0, 0, 3]) == 50.0
    # the whole loop from the near starts lands where the fp64 restatement lands
    Tf, stf = cnr.category_registration.icp_device(S, G, Ts[:3], max_corr)
    for b in range(3):
        want, fitness, rmse, _ = RC.icp(src.astype(np.float64), tgt.astype(np.float64), Ts[b], max_corr)
        print("start", b, "state", stf[b], "restatement", fitness, rmse, "dT", np.abs(Tf[b] - want).max())
        assert stf[b][2] in (1.0, 3.0) and abs(stf[b][0] - fitness) < 2e-3 and abs(stf[b][1] - rmse) < 1e-4
        assert np.abs(Tf[b] - want).max() < 2e-3              # the cloud's own noise (sigma 2 mm): ICP resolves nothing finer
