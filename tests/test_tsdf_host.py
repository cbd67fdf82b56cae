"""CPU: the numpy restatement of the TSDF contract (tests/tsdf_cpu.py) can fail for its own reasons: a plane
it must reconstruct where it is, a unit that only the frames touching it may update, and radius counts against a cKDTree."""
import numpy as np
from scipy.spatial import cKDTree

import tsdf_cpu as TC

K = (32.0, 32.0, 15.5, 11.5)
W, H, VOXEL, TRUNC = 32, 24, 0.01, 0.04


def test_a_fronto_parallel_plane_is_reconstructed_at_its_depth():
    """A plane at d = 1.000 m seen by an identity camera.  Only z crossings exist (both ends of an x or y edge lie on one side),
    and along z the stored value is (d - z) s / trunc with s the ray-length factor of the voxel's pixel.  Where both voxels of a
    crossing see the same pixel the TSDF is linear in z and the interpolation returns d -- up to the fp32 rounding of the two
    stored values (relative 2^-24 each), which moves the crossing by at most (voxel / 4) 2^-23 < voxel 2^-24, and fp64 rounding
    far below that.  Where the two voxels round to neighbouring pixels (x fx / z moves by up to 1 % of 16 px between them), s
    differs: z* - d = (z1 - d)(d - z0)(s0 - s1) / (r0 + r1) with r0 + r1 >= voxel min s >= voxel, so |z* - d| <= (voxel / 4) |s0 - s1|;
    ds/da = a / s <= |a| <= 0.5 and ds/db <= |b| <= 0.375 on this image and a, b move by 1 / fx between neighbouring pixels, so
    |s0 - s1| <= 0.875 / fx and 6.9e-5 m bounds every point."""
    d = np.float32(1.0)
    depth, img = np.full((W, H), d, np.float32), np.zeros((W, H, 3), np.uint8)
    r = TC.fuse(depth[None], img[None], np.eye(4)[None], K, VOXEL, TRUNC)
    p = r["points"]
    assert len(p) > 1000
    fx, fy, cx, cy = K
    # every point: an interpolated z between the two voxel centres 0.995 and 1.005, x and y on voxel centres
    z0, z1 = 0.995, 1.005
    assert np.all((p[:, 2] > z0) & (p[:, 2] < z1))
    pix = lambda z: (np.floor(p[:, 0] * fx / z + cx + 0.5), np.floor(p[:, 1] * fy / z + cy + 0.5))
    same = (pix(z0)[0] == pix(z1)[0]) & (pix(z0)[1] == pix(z1)[1])
    assert same.sum() > 500 and (~same).sum() > 0
    err = np.abs(p[:, 2] - 1.0)
    print("max |z - d|: same pixel %.3g, neighbouring pixels %.3g" % (err[same].max(), err[~same].max()))
    assert err[same].max() <= VOXEL * 2.0 ** -24
    assert err.max() <= VOXEL / 4 * 0.875 / fx
    # no point outside the image frustum
    uf, vf = p[:, 0] * fx / p[:, 2] + cx + 0.5, p[:, 1] * fy / p[:, 2] + cy + 0.5
    assert uf.min() >= 0 and uf.max() < W and vf.min() >= 0 and vf.max() < H
    # the colour of a black image, the weights of one frame
    assert not r["colors"].any() and set(np.unique(r["weight"])) <= {0.0, 1.0}


def stride_case():
    """frame A: a plane at 1 m.  frame B: the same pose and plane, but without depth at the strided samples of the image's left
    half -- B sees the units there, yet touches none of them."""
    depth = np.full((W, H), 1.0, np.float32)
    b = depth.copy()
    b[0:W // 2:TC.STRIDE, ::TC.STRIDE] = 0
    img = np.zeros((2, W, H, 3), np.uint8)
    img[1] = 200
    return np.stack([depth, b]), img, np.stack([np.eye(4), np.eye(4)])


def test_a_unit_is_updated_only_by_the_frames_that_touch_it():
    depths, img, T = stride_case()
    r = TC.fuse(depths, img, T, K, VOXEL, TRUNC)
    n_frames = np.diff(r["frame_ofs"])
    only_a = np.flatnonzero(n_frames == 1)
    assert len(only_a) > 0 and (n_frames == 2).any()
    assert all(r["frame_idx"][r["frame_ofs"][u]] == 0 for u in only_a)
    for u in only_a:
        w = r["weight"][u]
        assert set(np.unique(w)) <= {0.0, 1.0} and (w == 1).any()
    # the same units with B forced into their lists: B sees them (weights of 2), so the assertion above can fail
    U = len(r["units"])
    ofs, idx = np.arange(U + 1) * 2, np.tile(np.array([0, 1], np.int32), U)
    _, w2, _ = TC.integrate(r["units"], ofs, idx, depths, img, np.linalg.inv(T), K, VOXEL, TRUNC)
    assert all((w2[u] == 2).any() for u in only_a)


def test_radius_counts_equal_a_kdtree():
    rng = np.random.default_rng(5)
    r = 0.05
    for n, lo, hi in ((1, 0, 1), (300, -0.2, 0.2), (2000, -0.3, 0.5)):
        p = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
        p64 = p.astype(np.float64)
        tree = cKDTree(p64)
        assert len(tree.query_pairs(r + 1e-9)) == len(tree.query_pairs(r - 1e-9))        # no distance within 1e-9 of r
        want = np.array([len(v) for v in tree.query_ball_point(p64, r)])
        assert np.array_equal(TC.radius_counts(p, r), want)
        if n <= 300:
            assert np.array_equal(TC.radius_counts_brute(p, r), want)
    assert TC.radius_counts(np.zeros((1, 3), np.float32), r).tolist() == [1]


def test_touch_at_the_largest_truncation_emits_every_unit_of_the_range():
    """trunc = 8 voxel = half a unit: [p - trunc, p + trunc] is as long as a unit and spans two units on every axis; the 8 slots
    must hold exactly the units of [lo, hi], enumerated here without the slot structure.  Beyond it three units are possible
    (p = 0.08, trunc = 0.12, unit 0.16: floor(-0.25) = -1 .. floor(1.25) = 1), which 8 slots cannot hold: refused."""
    from itertools import product
    from test_tsdf_gpu import slanted_case
    depths, _, poses = slanted_case()
    fx, fy, cx, cy = K
    trunc, UL = 8 * VOXEL, 16.0 * VOXEL
    keys = TC.touch(depths[0], K, poses[0], VOXEL, trunc)
    n = 0
    for s, (x, y) in enumerate(product(range(0, W, TC.STRIDE), range(0, H, TC.STRIDE))):
        d = float(depths[0][x, y])
        if not d > 0:
            assert (keys[s] < 0).all()
            continue
        cam = np.array([(x - cx) * d / fx, (y - cy) * d / fy, d])
        p = [((poses[0][a, 0] * cam[0] + poses[0][a, 1] * cam[1]) + poses[0][a, 2] * cam[2]) + poses[0][a, 3] for a in range(3)]
        spans = [range(int(np.floor((c - trunc) / UL)), int(np.floor((c + trunc) / UL)) + 1) for c in p]
        want = {int(TC.pack(*u)) for u in product(*spans)}
        assert all(len(r) == 2 for r in spans) and len(want) == 8
        assert {int(k) for k in keys[s] if k >= 0} == want
        n += 1
    assert n > 20
    assert np.floor((0.08 - 0.12) / 0.16) == -1 and np.floor((0.08 + 0.12) / 0.16) == 1
    for bad in (8 * VOXEL * (1 + 1e-12), 0.12, 16 * VOXEL):
        try:
            TC.touch(depths[0], K, poses[0], VOXEL, bad)
        except ValueError:
            continue
        raise AssertionError("a truncation beyond 8 voxels was accepted")


def test_unit_tables_and_keys():
    keys = TC.touch(np.full((W, H), 1.0, np.float32), K, np.eye(4), VOXEL, TRUNC)
    assert keys.shape == (8 * 6, 8) and (keys[:, 0] >= 0).all()
    units, ofs, idx, nb = TC.unit_tables([keys, keys[:5]])
    ijk = TC.unpack(units)
    assert np.array_equal(TC.pack(*ijk.T), units) and ijk[:, 0].min() < 0 <= ijk[:, 0].max()       # x spans the origin
    assert np.all(np.diff(units) > 0) and ofs[-1] == len(idx) and set(np.diff(ofs)) <= {1, 2}
    for u in range(len(units)):
        for a in range(3):
            if nb[u, a] >= 0:
                step = np.zeros(3, np.int64)
                step[a] = 1
                assert np.array_equal(ijk[nb[u, a]], ijk[u] + step)
