"""GPU: csrc/tsdf.hip and what is built on it against the numpy restatement tests/tsdf_cpu.py.  Both sides run
the same separately rounded IEEE operations, so every comparison is np.array_equal."""
import os
import shutil

import numpy as np
import pytest
import torch

import registration_cpu as RC
import tsdf_cpu as TC
from test_align_poses_gpu import _write_checkpoints
from test_dataset_host import DS, _config

pytestmark = pytest.mark.gpu

K = (32.0, 32.0, 15.5, 11.5)
W, H, VOXEL, TRUNC = 32, 24, 0.01, 0.04


@pytest.fixture(scope="module")
def cnr():
    import cnr_amd
    return cnr_amd


def np_(t):
    return t.cpu().numpy()


def run_both(cnr, dev, depths, imgs, T_WC, K=K, voxel=VOXEL, trunc=TRUNC):
    """-> (the restatement's stages, the integrated utils.TSDFVolume)"""
    want = TC.fuse(depths, imgs, T_WC, K, voxel, trunc)
    vol = cnr.utils.TSDFVolume(voxel, trunc, device=dev)
    vol.integrate_frames(torch.from_numpy(np.asarray(depths, np.float32)), torch.from_numpy(np.asarray(imgs)), np.array(
        [[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]]), T_WC, keep_touch=True)
    return want, vol


def check_tables(want, vol):
    F = len(want["keys"])
    assert np.array_equal(np_(vol.touch_keys).reshape(F, -1, 8), want["keys"])
    assert np.array_equal(np_(vol.touch_frames), np.repeat(np.arange(F, dtype=np.int32)[:, None], vol.touch_frames.shape[1], 1))
    assert np.array_equal(np_(vol.units), want["units"])
    assert np.array_equal(np_(vol.frame_ofs), want["frame_ofs"]) and np.array_equal(np_(vol.frame_idx), want["frame_idx"])
    assert np.array_equal(np_(vol.neighbours), want["neighbours"])


def check_blocks(want, vol):
    for k in ("tsdf", "weight", "color"):
        assert np.array_equal(np_(getattr(vol, k)), want[k]), k


def check_points(want, vol):
    p, c = vol.extract_points()
    assert np.array_equal(np_(p), want["points"]) and np.array_equal(np_(c), want["colors"])
    return len(p)


# ---- the slanted plane through the origin --------------------------------------------------------------------------------
def slanted_case():
    n = np.array([0.3, 0.2, 1.0])
    n /= np.linalg.norm(n)
    poses = [TC.look_at((0.2, -0.3, -1.1), (0.05, 0.0, 0.0), up=(0.1, 1.0, 0.0)),
             TC.look_at((-0.4, 0.3, -0.9), (-0.1, 0.1, 0.0), up=(0.0, 1.0, 0.2)),
             TC.look_at((0.5, 0.4, -1.3), (0.0, -0.1, 0.0), up=(-0.2, 1.0, 0.0))]
    frames = [TC.render_plane(n, 0.0, K, T, W, H) for T in poses]
    return np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), np.stack(poses)


@pytest.fixture(scope="module")
def slanted(cnr, dev):
    return run_both(cnr, dev, *slanted_case())


def test_negative_coordinates_touch_list_gpu(slanted):
    want, vol = slanted
    ijk = TC.unpack(want["units"])
    for a in range(3):                                        # units on both sides of the origin on every axis
        assert ijk[:, a].min() < 0 <= ijk[:, a].max(), a
    assert not np.allclose(np.abs(slanted_case()[2][0][:3, :3]), np.eye(3), atol=0.05)
    assert (np.diff(want["frame_ofs"]) > 1).any() and (want["neighbours"] >= 0).any() and (want["neighbours"] < 0).any()
    check_tables(want, vol)


def test_negative_coordinates_blocks_gpu(slanted):
    want, vol = slanted
    assert want["weight"].max() == 3 and (want["color"] > 0).any()
    check_blocks(want, vol)


def test_negative_coordinates_extraction_gpu(slanted):
    want, vol = slanted
    assert len(want["points"]) > 1000 and (want["points"].min(0) < 0).all() and (want["points"].max(0) > 0).all()
    check_points(want, vol)


def test_largest_truncation_and_its_guard_gpu(cnr, dev):
    """trunc = 8 voxel: every sample touches two units per axis, all 8 slots; beyond it a third unit is possible, which the
    kernel, the volume and the restatement refuse"""
    want, vol = run_both(cnr, dev, *slanted_case(), trunc=8 * VOXEL)
    used = want["keys"][(want["keys"] >= 0).any(-1)]
    assert len(used) > 20 and (used >= 0).all()
    check_tables(want, vol)
    check_blocks(want, vol)
    assert check_points(want, vol) > 1000
    depth = torch.ones(W, H, device=dev)
    slots = int(cnr._C.load().cnr_tsdf_touch_slots(W, H))
    keys, tags = torch.empty(slots, device=dev, dtype=torch.int64), torch.empty(slots, device=dev, dtype=torch.int32)
    err, T = torch.zeros(1, device=dev, dtype=torch.int32), torch.eye(4, device=dev, dtype=torch.float64)
    cnr._C.call("cnr_tsdf_touch", depth, W, H, *K, T, VOXEL, 8 * VOXEL, 0, keys, tags, err)
    for bad in (8 * VOXEL * (1 + 1e-12), 0.12, 16 * VOXEL):
        with pytest.raises(cnr._C.CnrError, match="-2"):
            cnr._C.call("cnr_tsdf_touch", depth, W, H, *K, T, VOXEL, bad, 0, keys, tags, err)
        with pytest.raises(ValueError, match="8 voxel"):
            cnr.utils.TSDFVolume(VOXEL, bad, device=dev)
        with pytest.raises(ValueError):
            TC.touch(np.ones((W, H), np.float32), K, np.eye(4), VOXEL, bad)


def test_unproject_pointcloud_gpu(cnr, dev):
    """utils.unproject_pointcloud takes the (H,W) depth image and T_CW, as the reference's does: the points of RC.unproject on
    the transposed frame with inv(T_CW), in its order, within the bound of test_unproject_and_accumulate_on_the_replica_fixture_gpu
    (the kernel rounds the fp64 point once to fp32: 1e-5 m below 16 m)"""
    depths, _, poses = slanted_case()
    depth_hw = np.ascontiguousarray(depths[1].T)
    depth_hw[3:6, 10:20] = 0
    T_CW = np.linalg.inv(poses[1])
    got = cnr.utils.unproject_pointcloud(depth_hw, cnr.dataset.PinholeIntrinsics(W, H, *K), T_CW, device=dev)
    sample = {"depth": np.ascontiguousarray(depth_hw.T), "obj_mask": np.ones((W, H), np.int32), "image": np.zeros((W, H, 3), np.uint8),
              "T": poses[1]}
    idx, want, _ = RC.unproject(sample, 1, *K)
    assert len(got) == len(want) == int((depth_hw > 0).sum()) > 100 and got.colors_device is None
    assert np.abs(want).max() < 16 and np.abs(got.points - want).max() < 1e-5
    assert np.abs(want - want.mean(0)).max() > 0.3            # a transposed image or a pose not inverted is far outside the bound


# ---- which pixels and voxels count ----------------------------------------------------------------------------------------
def test_pixel_validity_gpu(cnr, dev):
    """Depth 0, depth beyond max_depth, an object mask over half the image; a camera 6 cm from the surface, so that voxels of
    the units it touches lie behind it and beside its image."""
    n = np.array([0.0, 0.0, 1.0])
    poses = np.stack([TC.look_at((0.0, 0.0, -1.0), (0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)),
                      TC.look_at((0.1, 0.05, -0.06), (0.1, 0.05, 0.0), up=(0.0, 1.0, 0.0)),
                      TC.look_at((0.3, 0.0, -1.25), (0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))])
    metric, imgs = zip(*[TC.render_plane(n, 0.0, K, T, W, H) for T in poses])
    metric = np.stack(metric)
    metric[0, 5:9, 3:8] = 0
    mask = np.ones((3, W, H), np.int32)
    mask[0, :, H // 2:] = 2
    max_depth = 1.27
    want_d = np.stack([TC.depth_image(metric[f], mask[f], 1, 0.001, max_depth) for f in range(3)])
    got_d = torch.stack([cnr.utils.tsdf_depth_image(torch.from_numpy(metric[f]).to(dev), torch.from_numpy(mask[f]).to(dev), 1, 0.001,
                                                     max_depth) for f in range(3)])
    assert np.array_equal(np_(got_d), want_d)
    assert (want_d[0, :, H // 2:] == 0).all() and (want_d[0, :, :H // 2] > 0).any() and (want_d[0, 5:9, 3:8] == 0).all()
    assert ((metric[2] > max_depth) & (want_d[2] == 0)).any() and (want_d[2] > 0).any()          # some beyond, some kept
    want, vol = run_both(cnr, dev, want_d, np.stack(imgs), poses)
    # frame 1's units hold voxels behind the camera and voxels that project beside the image
    T_CW = np.linalg.inv(poses[1])
    behind = beside = False
    for u in np.flatnonzero([1 in want["frame_idx"][a:b] for a, b in zip(want["frame_ofs"][:-1], want["frame_ofs"][1:])]):
        c = TC.voxel_centres(TC.unpack(want["units"][u]), VOXEL) @ T_CW[:3, :3].T + T_CW[:3, 3]
        behind |= bool((c[:, 2] <= 0).any())
        front = c[c[:, 2] > 0]
        beside |= bool((front[:, 0] * K[0] / front[:, 2] + K[2] + 0.5 < 0).any())
    assert behind and beside
    check_tables(want, vol)
    check_blocks(want, vol)
    assert check_points(want, vol) > 0


def test_depth_image_wraps_and_drops_gpu(cnr, dev):
    """values that divide inexactly, 70 m (70000 wraps to 4464 mm), a negative depth and a NaN, with two depth scales"""
    rng = np.random.default_rng(8)
    depth = rng.uniform(0, 7, (37, 29)).astype(np.float32)
    depth[0, :4] = [70.0, -1.5, np.nan, 0.0]
    mask = rng.integers(0, 3, (37, 29)).astype(np.int32)
    mask[0, :4] = 1
    for scale, max_depth in ((0.001, 6.0), (0.00025, 3.3)):
        want = TC.depth_image(depth, mask, 1, scale, max_depth)
        got = cnr.utils.tsdf_depth_image(torch.from_numpy(depth).to(dev), torch.from_numpy(mask).to(dev), 1, scale, max_depth)
        assert np.array_equal(np_(got), want)
        assert (want[mask != 1] == 0).all() and (want > 0).any() and want.max() <= max_depth
    assert TC.depth_image(depth, mask, 1, 0.001, 6.0)[0, :4].tolist() == [np.float32(4.464), 0.0, 0.0, 0.0]


def test_stride_gpu(cnr, dev):
    """A unit that frame B sees but only frame A's strided samples touch: its weights do not count B."""
    from test_tsdf_host import stride_case
    want, vol = run_both(cnr, dev, *stride_case())
    only_a = np.flatnonzero(np.diff(want["frame_ofs"]) == 1)
    assert len(only_a) > 0 and (np.diff(want["frame_ofs"]) == 2).any()
    got_w = np_(vol.weight)
    assert all(got_w[u].max() == 1 for u in only_a) and got_w.max() == 2
    check_tables(want, vol)
    check_blocks(want, vol)
    check_points(want, vol)


def test_valid_range_gpu(cnr, dev):
    """Two frames of one pose whose depths differ by 3 cm: voxels up to 7 cm behind the first surface are updated by the second
    frame alone, down to tsdf = -1."""
    depths = np.stack([np.full((W, H), 1.0154, np.float32), np.full((W, H), 1.0454, np.float32)])
    imgs = np.stack([TC.render_plane((0, 0, 1), 1.0, K, np.eye(4), W, H)[1]] * 2)
    want, vol = run_both(cnr, dev, depths, imgs, np.stack([np.eye(4), np.eye(4)]))
    f, w = want["tsdf"], want["weight"]
    seen = w != 0
    assert (seen & (f < np.float32(-0.98))).any() and (seen & (f >= np.float32(-0.98)) & (f < 0)).any()      # around -0.98
    assert (seen & (f >= np.float32(0.98))).any() and (seen & (f < np.float32(0.98)) & (f > 0)).any()        # around +0.98
    assert (w == 1).any() and (w == 2).any()                                     # sdf <= -trunc in the first frame only
    assert (~seen).any()                                                         # ... and in both
    check_blocks(want, vol)
    assert check_points(want, vol) > 0


def test_unit_faces_gpu(cnr, dev):
    """A surface at z = 6 x 0.16 m, on a unit face: its crossings join voxels of two units through the neighbour table.  Without
    the table's +z entries nothing is emitted there."""
    depths = np.full((1, W, H), 0.96, np.float32)
    want, vol = run_both(cnr, dev, depths, np.full((1, W, H, 3), 90, np.uint8), np.eye(4)[None])
    assert set(TC.unpack(want["units"])[:, 2]) == {5, 6}
    n = check_points(want, vol)
    assert n > 0 and np.all(np.abs(want["points"][:, 2] - 0.96) < 0.005)
    nb = want["neighbours"].copy()
    nb[:, 2] = -1
    vol.neighbours = torch.from_numpy(nb).to(dev)
    p, c = vol.extract_points()
    wp, wc = TC.extract(want["units"], nb, want["tsdf"], want["weight"], want["color"], VOXEL)
    assert len(wp) == 0 and len(p) == 0 and len(c) == 0


def test_extraction_scans_more_than_1024_blocks_gpu(cnr, dev):
    """One frame, 96 x 64 at fx = 16, of a plane at 4 m = 25 x 0.16 m: every strided sample (1 m apart) touches units on both
    sides of the face, more than 1024 in all, and the crossings lie in most of them."""
    Kw = (16.0, 16.0, 47.5, 31.5)
    depths = np.full((1, 96, 64), 4.0, np.float32)
    imgs = TC.render_plane((0, 0, 1), 4.0, Kw, np.eye(4), 96, 64)[1][None]
    want, vol = run_both(cnr, dev, depths, imgs, np.eye(4)[None], K=Kw)
    assert len(want["units"]) > 1024
    check_tables(want, vol)
    check_blocks(want, vol)
    assert check_points(want, vol) > 1024


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_emitted_counts_around_wave_and_block_sizes_gpu(cnr, dev, n):
    """Hand-made blocks of two units adjacent in x with exactly n crossings along z, most in the first unit."""
    units = TC.pack(np.array([-1, 0]), np.array([2, 2]), np.array([-3, -3]))
    nb = np.array([[1, -1, -1], [-1, -1, -1]], np.int32)
    tsdf, weight = np.zeros((2, 16, 16, 16), np.float32), np.zeros((2, 16, 16, 16), np.float32)
    color = np.zeros((2, 16, 16, 16, 3), np.float32)
    rng = np.random.default_rng(n)
    first = min(n, 200)
    for u, m in ((0, first), (1, n - first)):
        i, j = np.divmod(np.arange(m), 16)
        tsdf[u, i, j, 4], tsdf[u, i, j, 5] = rng.uniform(0.1, 0.9, m), -rng.uniform(0.1, 0.9, m)
        weight[u, i, j, 4] = weight[u, i, j, 5] = 1
        color[u, i, j, 4:6] = rng.integers(0, 256, (m, 2, 3))
    tsdf, weight, color = tsdf.reshape(2, -1), weight.reshape(2, -1), color.reshape(2, -1, 3)
    wp, wc = TC.extract(units, nb, tsdf, weight, color, VOXEL)
    assert len(wp) == n
    vol = cnr.utils.TSDFVolume(VOXEL, TRUNC, device=dev)
    vol.units, vol.neighbours = torch.from_numpy(units).to(dev), torch.from_numpy(nb).to(dev)
    vol.tsdf, vol.weight, vol.color = (torch.from_numpy(a).to(dev) for a in (tsdf, weight, color))
    p, c = vol.extract_points()
    assert np.array_equal(np_(p), wp) and np.array_equal(np_(c), wc)


def test_memory_guard_and_key_range_gpu(cnr, dev):
    depths, imgs, T = np.full((1, W, H), 1.0, np.float32), np.zeros((1, W, H, 3), np.uint8), np.eye(4)[None]
    Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]])
    with pytest.raises(cnr._C.CnrError, match="max_block_bytes"):
        cnr.utils.TSDFVolume(VOXEL, TRUNC, device=dev, max_block_bytes=3 * 20 * 4096).integrate_frames(depths, imgs, Km, T)
    far = np.eye(4)[None].copy()
    far[0, 0, 3] = 0.16 * 2 ** 20
    with pytest.raises(cnr._C.CnrError, match="2\\^20"):
        cnr.utils.TSDFVolume(VOXEL, TRUNC, device=dev).integrate_frames(depths, imgs, Km, far)


# ---- radius counts -------------------------------------------------------------------------------------------------------
def _counts(cnr, dev, p, r):
    return np_(cnr.utils.radius_neighbour_counts(torch.from_numpy(p).to(dev), r))


@pytest.mark.parametrize("n", [1, 63, 65, 1000])
def test_radius_count_random_gpu(cnr, dev, n):
    p = np.random.default_rng(n).uniform(-0.2, 0.3, (n, 3)).astype(np.float32)          # negative coordinates too
    want = TC.radius_counts_brute(p, 0.05)
    assert n < 1000 or want.max() > 5
    assert np.array_equal(_counts(cnr, dev, p, 0.05), want)


def test_radius_count_one_cell_cell_faces_and_negative_gpu(cnr, dev):
    rng = np.random.default_rng(2)
    one = rng.uniform(0.01, 0.04, (200, 3)).astype(np.float32)                           # all in the cell (0, 0, 0) of edge 0.05
    assert np.array_equal(_counts(cnr, dev, one, 0.05), TC.radius_counts_brute(one, 0.05))
    r = 0.0625                                                                            # p / r is exact: points ON cell faces
    off = rng.integers(0, 2, (300, 3)) * rng.uniform(0, r, (300, 3))
    off[np.arange(300), rng.integers(0, 3, 300)] = 0                                     # at least one coordinate on a face
    faces = (rng.integers(-3, 4, (300, 3)) * r + off).astype(np.float32)
    assert (faces / np.float32(r) == np.round(faces / np.float32(r))).any(1).all()
    assert np.array_equal(_counts(cnr, dev, faces, r), TC.radius_counts_brute(faces, r))
    neg = rng.uniform(-0.4, -0.1, (500, 3)).astype(np.float32)
    assert np.array_equal(_counts(cnr, dev, neg, 0.05), TC.radius_counts_brute(neg, 0.05))


def test_remove_radius_outlier_keeps_more_than_nb_points_gpu(cnr, dev):
    """two tight clusters 1 m apart: one of nb_points + 1 points (each counts nb_points + 1: kept), one of nb_points (removed)"""
    nb = 7
    rng = np.random.default_rng(3)
    a, b = rng.uniform(0, 0.005, (nb + 1, 3)), rng.uniform(0, 0.005, (nb, 3)) + 1.0
    p = np.concatenate([b[:3], a, b[3:]]).astype(np.float32)
    cloud = cnr.utils.PointCloud(p, colors=np.abs(p) / 2, device=dev)
    counts = _counts(cnr, dev, p, 0.05)
    assert sorted(set(counts)) == [nb, nb + 1]
    kept, index = cloud.remove_radius_outlier(nb_points=nb, radius=0.05)
    assert np.array_equal(np_(index), np.arange(3, 3 + nb + 1))
    assert np.array_equal(np_(kept.points_device), p[3:3 + nb + 1]) and np.array_equal(np_(kept.colors_device), (np.abs(p) / 2).astype(np.float32)[3:3 + nb + 1])


# ---- the chain and the ScanNet fixture -------------------------------------------------------------------------------------
def restated_cloud(inst_id, frame_info, samples, Kc, depth_scale, max_depth):
    """accumulate_pointcloud_tsdf in the restatement's words -> (points (n,3) f32, fell back to the unfiltered cloud)"""
    frames = [samples[fi["frame"]] for fi in frame_info]
    depths = np.stack([TC.depth_image(s["depth"], s["obj_mask"], inst_id, depth_scale, max_depth) for s in frames])
    r = TC.fuse(depths, np.stack([s["image"] for s in frames]), np.stack([s["T"] for s in frames]), Kc, 0.01, 0.04)
    p, _, _, _ = RC.voxel_down_sample(r["points"].astype(np.float32), r["colors"].astype(np.float32), 0.01)
    p = p.astype(np.float32)
    kept = p[TC.radius_counts(p, 0.05) > 100]
    return (kept, False) if len(kept) >= 100 else (p, True)          # (kept is a strict subset when the filter removed any)


def test_accumulate_keeps_the_filtered_cloud_of_a_corrugated_surface_gpu(cnr, dev):
    """columns of pixels alternately at 1.00 m and 1.03 m: two sheets and the walls between them put more than 100 points within
    5 cm of most points, fewer at the rim, so the filter both keeps and removes and its result is returned"""
    depth = (1.0 + 0.03 * (np.arange(W)[:, None] % 2) + np.zeros((1, H))).astype(np.float32)
    samples = {0: {"depth": depth, "image": TC.render_plane((0, 0, 1), 1.0, K, np.eye(4), W, H)[1], "obj_mask": np.zeros((W, H), np.int32),
                   "T": np.eye(4), "frame_id": 0}}
    want, fell_back = restated_cloud(0, [{"frame": 0}], samples, K, 0.001, 6.0)
    assert not fell_back and len(want) > 1000
    full, _, _, _ = RC.voxel_down_sample(TC.fuse(TC.depth_image(depth, samples[0]["obj_mask"], 0)[None], samples[0]["image"][None],
                                                 np.eye(4)[None], K, VOXEL, TRUNC)["points"].astype(np.float32), None, 0.01)
    assert len(want) < len(full)                              # the filter removed points as well
    got = cnr.utils.accumulate_pointcloud_tsdf(0, [{"frame": 0}], samples, cnr.dataset.PinholeIntrinsics(W, H, *K), device=dev)
    assert np.array_equal(np_(got.points_device), want)


def test_accumulate_falls_back_when_fewer_than_100_points_survive_gpu(cnr, dev):
    depths, imgs, poses = slanted_case()
    samples = {f: {"depth": depths[f], "image": imgs[f], "obj_mask": np.zeros((W, H), np.int32), "T": poses[f], "frame_id": f}
               for f in range(3)}
    info = [{"frame": f} for f in range(3)]
    want, fell_back = restated_cloud(0, info, samples, K, 0.001, 6.0)
    assert fell_back and len(want) > 1000                     # a single thin sheet: about 78 points per 5 cm disc
    got = cnr.utils.accumulate_pointcloud_tsdf(0, info, samples, cnr.dataset.PinholeIntrinsics(W, H, *K), device=dev)
    assert np.array_equal(np_(got.points_device), want)


@pytest.fixture(scope="module")
def scannet_registered(cnr, dev, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("scannet_tsdf")
    root = str(tmp / "scannet")
    shutil.copytree(os.path.join(DS, "scannet"), root)
    cfg = _config(cnr, "scannet_refined", root=root)
    cfg.weight_root, cfg.load_pretrained, cfg.load_registration_result = str(tmp / "weights"), True, False
    cfg.data_device = str(dev)
    return cfg, root


def test_get_all_poses_scannet_equals_the_restatement_gpu(cnr, dev, scannet_registered, monkeypatch):
    cfg, root = scannet_registered
    CR = cnr.category_registration
    seen = {}
    monkeypatch.setattr(CR, "register_dataset", lambda ds, c, solver=None, tsdf=False: seen.update(tsdf=tsdf))
    ds = cnr.dataset.get_dataset(cfg, register=True, tsdf=True)
    assert seen == {"tsdf": True}
    inst = ds.inst_dict
    Kc = (cfg.fx, cfg.fy, cfg.cx, cfg.cy)
    raw = {(c, i): e["pcs"] for c, d in inst.items() if c != 0 for i, e in d.items()}
    assert len(raw) == 3 and all(len(p) > 0 for p in raw.values())
    CR.get_all_poses(inst, ds.sample_dict, ds.intrinsic_open3d, name="scannet", depth_scale=cfg.depth_scale, max_depth=cfg.max_depth,
                     tsdf=True)
    for (c, i), cloud in raw.items():
        # what the loader gathered: the object's pixels of its frames (coordinates within the bound of
        # test_unproject_and_accumulate_on_the_replica_fixture_gpu: 1e-5 m), then the restated 1 cm down-sample of exactly that
        want = np.concatenate([RC.unproject(ds.sample_dict[fi["frame"]], i, *Kc)[1] for fi in inst[c][i]["frame_info"]])
        assert len(cloud) == len(want) and np.abs(cloud.points - want).max() < 1e-5
        m, _, _, _ = RC.voxel_down_sample(np_(cloud.points_device), None, 0.01)
        assert np.array_equal(np_(inst[c][i]["pcs"].points_device), m.astype(np.float32)), (c, i)
    want_bg, fell_back = restated_cloud(0, inst[0]["frame_info"], ds.sample_dict, Kc, cfg.depth_scale, cfg.max_depth)
    assert fell_back and len(want_bg) > 1000      # thin sheets: the fixture takes the fallback (the kept branch: the corrugated case)
    assert np.array_equal(np_(inst[0]["pcs"].points_device), want_bg)
    to_box, extents = cnr.metrics.oriented_bounds(want_bg.astype(np.float64))
    from_box = np.linalg.inv(to_box)
    box = inst[0]["bbox3D"]
    assert np.array_equal(box.R, from_box[:3, :3]) and np.array_equal(box.center, from_box[:3, 3]) and np.array_equal(box.extent, extents)
    # an object the loader gathered nothing for
    inst[5][99] = {"frame_info": []}
    CR.get_all_poses({5: {99: inst[5][99]}}, ds.sample_dict, ds.intrinsic_open3d, name="scannet", tsdf=True)
    assert inst[5][99]["pcs"] is None and np.array_equal(inst[5][99]["T_obj"], np.eye(4))


def test_register_scannet_writes_a_cache_that_reloads_gpu(cnr, dev, scannet_registered):
    cfg, root = scannet_registered
    _write_checkpoints(cnr, cfg.weight_root, [3, 4, 65536], cfg.hidden_feature_size)
    with pytest.raises(NotImplementedError, match="registration"):
        cnr.dataset.get_dataset(cfg, register=True)
    plain = cnr.dataset.ScanNet.__new__(cnr.dataset.ScanNet)
    plain.name = "scannet"
    with pytest.raises(NotImplementedError, match="tsdf=True"):
        cnr.category_registration.register_dataset(plain, cfg)
    assert not os.path.exists(os.path.join(root, "inst_dict.pkl"))
    ds = cnr.dataset.get_dataset(cfg, register=True, tsdf=True)
    back = cnr.dataset.load_registration_result(os.path.join(root, "inst_dict.pkl"))
    assert list(back.keys()) == list(ds.inst_dict.keys()) and 0 in back
    n_inst = 0
    for cls_id, d in back.items():
        for inst_id, e in ([(None, d)] if cls_id == 0 else d.items()):
            n_inst += cls_id != 0
            assert "pcs" not in e and e["bbox3D"].extent.shape == (3,)
            if cls_id != 0:
                assert e["T_obj"].shape == (4, 4) and np.isfinite(e["T_obj"]).all()
                assert np.array_equal(e["T_obj"], ds.inst_dict[cls_id][inst_id]["T_obj"])
    assert n_inst == 3
