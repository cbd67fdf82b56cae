"""GPU: csrc/metric.hip against float64 brute force and the numpy restatement (tests/metric_cpu.py), the public metrics against
the reference's metrics.py (tests/golden/metric/), calc_3d_metric end to end on analytic shapes, and tools/eval_3d_obj.py on a
tiny Replica-style tree."""
import glob
import json
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import mc_cpu as M
import metric_cpu as K
from conftest import ROOT

pytestmark = pytest.mark.gpu

METRIC_GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "metric", "*.npz")))


@pytest.fixture(scope="module")
def mt():
    from cnr_amd import metrics
    return metrics


def _brute(q, p):
    """float64 nearest distances by broadcasting, in query chunks of at most 2e7 pairs"""
    q64, p64 = q.double(), p.double()
    step = max(1, 20_000_000 // len(p64))
    out = []
    for i in range(0, len(q64), step):
        out.append(((q64[i:i + step, None, :] - p64[None]) ** 2).sum(-1).min(1).values.sqrt())
    return torch.cat(out)


@pytest.mark.parametrize("nq,nr", [(1, 1), (1, 63), (63, 1), (64, 64), (65, 65), (1000, 1000), (63, 1000), (1000, 65),
                                   (10000, 10000), (200000, 5000), (5000, 200000)])
def test_nn_dist_against_float64_brute_force(mt, dev, nq, nr):
    g = torch.Generator(device=dev).manual_seed(nq * 7 + nr)
    q = torch.rand(nq, 3, device=dev, generator=g) * 6 - 1        # metres, away from the origin
    p = torch.rand(nr, 3, device=dev, generator=g) * 6 - 1
    d = mt.nn_dist(q, p)
    ref = _brute(q, p)
    bar = 2e-6 * (1 + q.double().norm(dim=1))
    assert ((d.double() - ref).abs() <= bar).all(), float(((d.double() - ref).abs() - bar).max())
    again = mt.nn_dist(q, p)
    assert torch.equal(d, again)


def test_nn_dist_duplicates_and_exact_hits(mt, dev):
    g = torch.Generator(device=dev).manual_seed(3)
    p = torch.rand(3000, 3, device=dev, generator=g) * 4 + 3
    p = torch.cat([p, p[:1000], p[:10]])                            # duplicated reference points
    q = torch.cat([p[500:1500], torch.rand(700, 3, device=dev, generator=g) * 4 + 3])
    d = mt.nn_dist(q, p)
    assert (d[:1000] == 0).all()
    ref = _brute(q, p)
    assert ((d.double() - ref).abs() <= 2e-6 * (1 + q.double().norm(dim=1))).all()
    assert torch.equal(mt.nn_dist(q, q), torch.zeros(len(q), device=dev))


def test_dist_stats(mt, dev):
    """The count is exact: the kernel compares float v < float th with th rounded to fp32 as ctypes rounds a c_float argument
    (to nearest), which is np.float32(th), and numpy compares the same two fp32 numbers.  The sum: any order of n fp64
    additions of non-negative terms is within (n - 1) 2^-53 of the exact sum (math.fsum), relatively."""
    g = torch.Generator(device=dev).manual_seed(5)
    for n in (1, 255, 256, 257, 10000, 65536, 65537, 200001):
        d = torch.rand(n, device=dev, generator=g) * 0.2
        th = 0.05
        s, c = mt.dist_stats(d, th)
        dn = d.cpu().numpy()
        assert s == pytest.approx(math.fsum(dn.astype(np.float64)), rel=n * 2.0 ** -53, abs=1e-300)
        assert c == int((dn < np.float32(th)).sum())
        assert (s, c) == mt.dist_stats(d, th)


def test_dist_stats_at_the_threshold_and_non_finite(mt, dev):
    """strict <: th itself and the fp32 number above it are not counted, the one below is; inf and NaN are never counted, not
    even under th = inf; a NaN makes the sum NaN, an inf without a NaN makes it inf"""
    th = 0.05
    t32 = np.float32(th)
    up, down = np.nextafter(t32, np.float32(np.inf)), np.nextafter(t32, np.float32(-np.inf))
    assert down < t32 < up
    edge = np.array([t32, up, down, np.inf, 0.01, 0.2, down, t32], np.float32)
    rng = np.random.default_rng(8)
    body = (rng.random(70001) * 0.2).astype(np.float32)
    at = rng.permutation(len(body))[:len(edge)]
    body[at] = edge
    for base in (edge, body):
        for with_nan in (False, True):
            d = np.append(base, np.float32(np.nan)) if with_nan else base
            t = torch.from_numpy(d).to(dev)
            s, c = mt.dist_stats(t, th)
            assert c == int((d < t32).sum())
            if base is edge:
                assert c == 3                         # 0.01 and `down` twice, by hand; the NaN adds nothing
            assert math.isnan(s) if with_nan else s == float("inf")
            s2, c2 = mt.dist_stats(t, float("inf"))
            assert c2 == int(np.isfinite(d).sum()) == int((d < np.float32(np.inf)).sum())
            assert (c, c2) == (mt.dist_stats(t, th)[1], mt.dist_stats(t, float("inf"))[1])
    fin = np.where(np.isfinite(body), body, np.float32(0.1))
    s, c = mt.dist_stats(torch.from_numpy(fin).to(dev), th)
    assert s == pytest.approx(math.fsum(fin.astype(np.float64)), rel=len(fin) * 2.0 ** -53) and c == int((fin < t32).sum())


def _mc_mesh(D=48, r0=0.85, centre=(0.0, 0.0, 0.0), scale=1.0):
    from cnr_amd import vis
    m = vis.marching_cubes(M.sphere(D, r0, 4.0, centre))
    m.apply_translation([-0.5, -0.5, -0.5]).apply_scale(2.0 * scale)
    return m


def _device_mesh(mesh, dev):
    from cnr_amd.devmesh import device_mesh
    return device_mesh(mesh, dev)


def _soup_device(verts32, dev):
    """a soup (F*3,3) f32 both ways the kernels read triangles: unindexed (faces = NULL) and indexed by 0, 1, 2, ..."""
    v = torch.from_numpy(np.ascontiguousarray(verts32, np.float32)).to(dev)
    F = len(v) // 3
    return _device_mesh((v, None), dev), _device_mesh((v, torch.arange(3 * F, device=dev, dtype=torch.int32).view(F, 3)), dev)


def _sample_points(tri, cum, u, dev):
    from cnr_amd import _C
    out = torch.empty(len(u), 3, device=dev)
    _C.call("cnr_sample_surface", tri.verts, tri.faces, tri.n_faces, cum, torch.from_numpy(u).to(dev), len(u), out)
    return out


def test_sample_surface_matches_the_restatement(mt, dev):
    from cnr_amd import vis
    v, f, us = K.sampling_random_inputs()
    meshes = [_mc_mesh(33), _mc_mesh(64, 0.6, (0.2, 0.0, 0.1), 3.0), vis.Mesh(v, f)]
    for m, u in zip(meshes, us):
        tri = _device_mesh(m, dev)
        area, cum = mt._area_scan(tri)
        T = K.triangles(m.vertices, m.faces)
        np.testing.assert_allclose(area.cpu().numpy(), K.face_areas(T), rtol=1e-12, atol=0)
        face, pts, cum_r, near = K.sampling_near_boundaries(T, u)
        np.testing.assert_allclose(cum.cpu().numpy(), cum_r, rtol=1e-12)
        out = _sample_points(tri, cum, u, dev)
        got = out.cpu().numpy()
        # the same face wherever u0 * total is not within 1e-12 (relative) of a prefix boundary: that band is 2e-12 of the total
        # per boundary, 4e-3 samples are expected in it, and none of this seed's draws is (test_metrics_host.py checks the same)
        assert near.sum() == 0
        np.testing.assert_allclose(got, pts, rtol=0, atol=1e-6 * (1 + np.abs(pts).max()))
        assert torch.equal(out, _sample_points(tri, cum, u, dev))


@pytest.mark.parametrize("which", ["many", "single"])
def test_sample_surface_is_exact_on_dyadic_input(mt, dev, which):
    """Areas, prefixes, targets and points of K.dyadic_sampling_fixture are exact in fp64 however they are evaluated
    (test_metrics_host.py proves it in rational arithmetic), so everything is compared bit for bit: u0 = 0, u0 on a prefix
    boundary (the lower face; the first of equal prefixes), one ulp either side, zero-area faces, a + b == 1 and 1 + 2^-52."""
    verts, u = K.dyadic_sampling_fixture() if which == "many" else K.dyadic_single_face()
    T = K.triangles(verts)
    face, pts, cum_r = K.sample_surface(T, u)
    outs = []
    for tri in _soup_device(verts, dev):
        area, cum = mt._area_scan(tri)
        assert np.array_equal(area.cpu().numpy(), K.face_areas(T)) and np.array_equal(cum.cpu().numpy(), cum_r)
        out = _sample_points(tri, cum, u, dev)
        got = out.cpu().numpy()
        wrong = np.flatnonzero((got != pts).any(1))
        assert len(wrong) == 0, (wrong[:5], u[wrong[:5]], got[wrong[:5]], pts[wrong[:5]], face[wrong[:5]])
        assert torch.equal(out, _sample_points(tri, cum, u, dev))
        outs.append(out)
    assert torch.equal(outs[0], outs[1])


_random_box = K.random_box


def test_clip_matches_the_restatement(mt, dev):
    from cnr_amd import vis
    rng = np.random.default_rng(6)
    soup_v = rng.normal(size=(3000, 3)) * 0.5
    cases = [(_mc_mesh(48), (0.1, 0.0, -0.2), (1.2, 0.9, 1.0)), (_mc_mesh(96), (0.0, 0.3, 0.0), (0.4, 2.5, 2.5)),
             (vis.Mesh(soup_v, np.arange(3000).reshape(-1, 3)), (0.0, 0.0, 0.0), (0.7, 0.7, 0.7))]
    for m, c, e in cases:
        T, ext = _random_box(rng, c, e)
        planes = mt.box_planes(T, ext)
        tri = _device_mesh(m, dev)
        out = mt._clip(tri, planes)
        ref = K.clip_box(K.triangles(m.vertices, m.faces), planes)
        assert out is not None and len(ref)
        got = out.verts.double().cpu().numpy().reshape(-1, 3, 3)
        assert K.face_areas(got).sum() == pytest.approx(K.face_areas(ref).sum(), rel=1e-5)
        loc = got.reshape(-1, 3) @ T[:3, :3].T + T[:3, 3]
        assert (np.abs(loc) <= ext / 2 + 1e-5).all()
        again = mt._clip(tri, planes)
        assert torch.equal(out.verts, again.verts)
        # the soup itself can be clipped and sampled again
        assert mt._sample(out, 1000, np.random.default_rng(1)).shape == (1000, 3)
    # outside everything: nothing
    T, ext = _random_box(rng, (10.0, 0.0, 0.0), (0.5, 0.5, 0.5))
    assert mt._clip(_device_mesh(_mc_mesh(33), dev), mt.box_planes(T, ext)) is None


def _check_clip_rows(mt, tri_dev, tri64, planes, general=True):
    """mt._clip against K.clip_box row for row: the same triangle count, (face, fan) order and corner order.  The kernel
    evaluates each corner in fp64 and rounds once to fp32; its fp64 value differs from numpy's by a few units of 2^-53 (fused
    multiply-adds; t = da / (da - db) is well conditioned, da and db have opposite signs), so each coordinate lies within one
    fp32 spacing of float32(ref), and a rounding boundary between the two fp64 values has probability 2^-53 / 2^-24 = 2e-9:
    at most 1 coordinate in 10^4 may differ from float32(ref) at all."""
    ref, counts, closest = K.clip_box_info(tri64, planes)
    if general:
        assert closest >= 1e-9 * np.abs(tri64).max(), closest    # the kept / dropped decisions cannot differ (test_metrics_host.py)
    out = mt._clip(tri_dev, planes)
    assert out is not None and len(ref) and out.n_faces == len(ref) and out.verts.shape == (3 * len(ref), 3)
    got = out.verts.cpu().numpy().reshape(-1, 3, 3)
    ref32 = ref.astype(np.float32)
    err = np.abs(got.astype(np.float64) - ref32.astype(np.float64))
    bad = np.flatnonzero((err > np.spacing(np.abs(ref32)).astype(np.float64)).any((1, 2)))
    face_of = np.repeat(np.arange(len(counts)), counts)
    assert len(bad) == 0, (len(bad), len(ref), bad[:4], face_of[bad[:4]], got[bad[:2]], ref32[bad[:2]])
    differ = int((got != ref32).sum())
    print("clip: %d faces -> %d triangles, %d of %d coordinates off float32(ref), closest dist %.3g"
          % (len(tri64), len(ref), differ, got.size, closest))
    assert differ * 10 ** 4 <= got.size, (differ, got.size)
    again = mt._clip(tri_dev, planes)
    assert torch.equal(out.verts, again.verts)
    return out


@pytest.mark.parametrize("F,verts,T,ext", K.clip_soup_cases(), ids=["F%d" % c[0] for c in K.clip_soup_cases()])
def test_clip_rows_of_random_soups(mt, dev, F, verts, T, ext):
    planes = mt.box_planes(T, ext)
    soup, indexed = _soup_device(verts, dev)
    assert soup.n_faces == F
    out = _check_clip_rows(mt, soup, K.triangles(verts), planes)
    assert torch.equal(out.verts, _check_clip_rows(mt, indexed, K.triangles(verts), planes).verts)


def test_clip_rows_of_an_indexed_sphere(mt, dev):
    m = _mc_mesh(48)
    T, ext = K.random_box(np.random.default_rng(22), (0.1, 0.0, -0.2), (1.2, 0.9, 1.0))
    out = _check_clip_rows(mt, _device_mesh(m, dev), K.triangles(m.vertices, m.faces), mt.box_planes(T, ext))
    assert 1000 < out.n_faces < len(m.faces)


def test_clip_rows_for_every_fan_count(mt, dev):
    """faces that clip to 0, 1, ... 7 triangles (the 9-vertex polygon is constructed: K.hexagon_triangle), shuffled so that
    every bit of the per-lane count is mixed within every wave"""
    verts = K.fan_soup()
    planes = mt.box_planes(*K.UNIT_BOX)
    counts = K.clip_box_info(K.triangles(verts), planes)[1]
    assert set(counts) == set(range(8))
    for tri in _soup_device(verts, dev):
        _check_clip_rows(mt, tri, K.triangles(verts), planes)


def test_clip_rows_with_corners_exactly_on_the_planes(mt, dev):
    """dist == 0 is inside (>=).  All dists and intersections of K.on_plane_soup are exact, so the decisions are the
    restatement's; a face that only touches the box comes out as zero-area triangles, as the restatement emits them."""
    verts, counts = K.on_plane_soup()
    planes = mt.box_planes(*K.UNIT_BOX)
    for tri in _soup_device(verts, dev):
        out = _check_clip_rows(mt, tri, K.triangles(verts), planes, general=False)
        assert out.n_faces == counts.sum()
        got = out.verts.double().cpu().numpy().reshape(-1, 3, 3)
        assert np.array_equal(got, K.clip_box(K.triangles(verts), planes))       # exact input: exact output
        first = np.cumsum(counts) - counts
        assert (got[first[3]] == verts[9]).all()                                 # touched by one corner: that corner three times


def test_clip_scan_with_more_than_1024_blocks(mt, dev):
    """F > 262144 faces are more than 1024 blocks of 256: every thread of clip_scan_kernel owns a run of `per` = 2 block
    counts.  Clipping is per face, so a verified soup tiled k times gives its verified output k times, bit for bit."""
    F, verts, T, ext = K.clip_soup_cases()[-1]
    planes = mt.box_planes(T, ext)
    small = _check_clip_rows(mt, _soup_device(verts, dev)[0], K.triangles(verts), planes)
    k = 263
    assert F * k > 262144 and (F * k) % 256 != 0 and -(-F * k // 256) > 1024
    for tri in _soup_device(np.tile(verts, (k, 1)), dev):
        big = mt._clip(tri, planes)
        assert big.n_faces == k * small.n_faces
        assert torch.equal(big.verts.view(k, -1), small.verts.view(1, -1).expand(k, -1))
        assert torch.equal(big.verts, mt._clip(tri, planes).verts)


def test_face_area_scan_with_more_than_1024_blocks(mt, dev):
    """F > 1048576 faces are more than 1024 blocks of 1024: fa_blocks_scan_kernel's `per` = 2.  The areas are the small
    soup's, tiled, bit for bit; the prefix against numpy's sequential fp64 cumsum at 1e-12 (sqrt(F) 2^-53 = 1e-13 is the
    expected difference of two summation orders), and it never decreases."""
    F, verts, _, _ = K.clip_soup_cases()[-1]
    small_area, small_cum = mt._area_scan(_soup_device(verts, dev)[0])
    ref = K.face_areas(K.triangles(verts))
    np.testing.assert_allclose(small_area.cpu().numpy(), ref, rtol=1e-12, atol=0)
    np.testing.assert_allclose(small_cum.cpu().numpy(), np.cumsum(ref), rtol=1e-12, atol=0)
    k = 1049
    assert F * k > 1048576 and (F * k) % 1024 != 0 and -(-F * k // 1024) > 1024
    for tri in _soup_device(np.tile(verts, (k, 1)), dev):
        area, cum = mt._area_scan(tri)
        assert torch.equal(area.view(k, F), small_area.view(1, F).expand(k, F))
        np.testing.assert_allclose(cum.cpu().numpy(), np.cumsum(area.cpu().numpy()), rtol=1e-12, atol=0)
        assert bool((cum[1:] >= cum[:-1]).all())
        area2, cum2 = mt._area_scan(tri)
        assert torch.equal(area, area2) and torch.equal(cum, cum2)


@pytest.mark.parametrize("path", METRIC_GOLDEN, ids=[os.path.basename(p)[:-4] for p in METRIC_GOLDEN])
def test_public_metrics_match_the_reference(mt, dev, path):
    z = np.load(path)
    gt, rec = z["gt"], z["rec"]
    assert mt.accuracy(gt, rec) == pytest.approx(float(z["accuracy"]), rel=1e-5)
    assert mt.completion(gt, rec) == pytest.approx(float(z["completion"]), rel=1e-5)
    assert mt.chamfer(torch.from_numpy(gt).to(dev), rec) == pytest.approx(float(z["chamfer"]), rel=1e-5)
    assert mt.accuracy_ratio(gt, rec, float(z["th_acc"])) == pytest.approx(float(z["accuracy_ratio"]), rel=1e-5)
    assert mt.completion_ratio(gt, rec, float(z["th_comp"])) == pytest.approx(float(z["completion_ratio"]), rel=1e-5)
    assert isinstance(mt.accuracy(gt, rec), float)


# ---- end to end ----------------------------------------------------------------------------------------------------------
R0, DELTA = 0.40, 0.02


def _sphere_mesh(r, D=96):
    """a marching-cubes sphere of radius r (metres) about the origin"""
    m = _mc_mesh(D, 0.8)
    m.vertices = m.vertices * (r / 0.8)
    return m


def test_calc_3d_metric_on_concentric_spheres(mt, dev):
    rec, gt = _sphere_mesh(R0), _sphere_mesh(R0 + DELTA)
    out = mt.calc_3d_metric(rec, gt, N=200000)
    acc, comp, ratio = out[0][0], out[1][0], out[2][0]
    # the chord error of the mesh (~h^2 / 8r ~ 0.01 cm) and the sampling's tangential offset (~0.05 cm at 200k) both add
    assert DELTA * 100 - 0.05 < acc < DELTA * 100 + 0.15, out
    assert DELTA * 100 - 0.05 < comp < DELTA * 100 + 0.15, out
    assert ratio == 100.0
    assert isinstance(acc, float) and mt.calc_3d_metric(rec, gt, N=200000) == out       # seeded, deterministic
    gt_pts, rec_pts = mt.sample_surface(gt, 50000, seed=1), mt.sample_surface(rec, 50000, seed=2)
    assert mt.completion_ratio(gt_pts, rec_pts, 0.05) == 1.0
    assert mt.completion_ratio(gt_pts, rec_pts, 0.01) == 0.0
    assert mt.accuracy_ratio(gt_pts, rec_pts, 0.03) == 1.0


def test_calc_3d_metric_crops_to_a_half_sphere(mt, dev):
    from cnr_amd import vis
    rec, big = _sphere_mesh(R0), _sphere_mesh(R0 + DELTA)
    keep = (big.vertices[big.faces][:, :, 2] > 0).all(1)
    half = vis.Mesh(big.vertices, big.faces[keep])
    T, ext = mt.oriented_bounds(half)
    cut = mt.slice_box(rec, T, ext)
    assert cut.vertices[:, 2].min() > -1e-5 - 0.002                   # the half sphere's lowest vertex lies just above 0
    area = K.face_areas(K.triangles(cut.vertices, cut.faces)).sum()
    full = K.face_areas(K.triangles(rec.vertices, rec.faces)).sum()
    assert 0.45 < area / full < 0.52
    out = mt.calc_3d_metric(rec, half, N=100000)
    # accuracy on the cropped upper half stays ~delta; completion (half GT against the whole rec) too
    assert DELTA * 100 - 0.1 < out[0][0] < DELTA * 100 + 0.4, out
    assert DELTA * 100 - 0.1 < out[1][0] < DELTA * 100 + 0.3, out
    # without the crop the lower half would be ~R0 away: the uncropped accuracy is far larger
    assert mt.accuracy(mt.sample_surface(half, 50000), mt.sample_surface(rec, 50000)) * 100 > 3 * out[0][0]


def test_calc_3d_metric_with_the_box_elsewhere_is_none(mt, dev, capsys):
    rec, far = _sphere_mesh(R0), _sphere_mesh(R0)
    far.apply_translation([10.0, 0.0, 0.0])
    assert mt.calc_3d_metric(rec, far, N=1000) is None
    assert "no mesh found" in capsys.readouterr().out


# ---- the command line ----------------------------------------------------------------------------------------------------
def _write_quad_ply(path, v, quads):
    head = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(v), "property float x", "property float y",
            "property float z", "property uchar red", "property uchar green", "property uchar blue",
            "element face %d" % len(quads), "property list uchar int vertex_indices", "property int object_id", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode())
        for p in v:
            f.write(struct.pack("<3f3B", *p, 200, 100, 50))
        for q in quads:
            f.write(struct.pack("<B4ii", 4, *q, 3))


def _cube(lo, hi, n=8):
    """the surface of a box as an n x n grid of quads per face"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    verts, quads = [], []
    t = np.linspace(0, 1, n + 1)
    for ax in range(3):
        for side in (0, 1):
            a, b = [k for k in range(3) if k != ax]
            base = len(verts)
            for i in range(n + 1):
                for j in range(n + 1):
                    p = np.empty(3)
                    p[ax] = (lo if side == 0 else hi)[ax]
                    p[a] = lo[a] + t[i] * (hi[a] - lo[a])
                    p[b] = lo[b] + t[j] * (hi[b] - lo[b])
                    verts.append(p)
            for i in range(n):
                for j in range(n):
                    k = base + i * (n + 1) + j
                    quads.append([k, k + n + 1, k + n + 2, k + 1])
    return np.array(verts), np.array(quads)


def test_eval_3d_obj_cli_on_a_replica_tree(dev, tmp_path):
    from cnr_amd import vis
    data = tmp_path / "Replica"
    hab = data / "room_0" / "habitat"
    hab.mkdir(parents=True)
    boxes = {1: ([0.0, 0.0, 0.0], [0.5, 0.4, 0.3]), 2: ([1.0, 1.0, 0.0], [1.3, 1.6, 0.8])}
    (hab / "info_semantic.json").write_text(json.dumps({"objects": [{"id": 1, "class_id": 7}, {"id": 2, "class_id": 40}]}))
    logs = tmp_path / "logs"
    mdir = logs / "room_0" / "scene_mesh"
    mdir.mkdir(parents=True)
    for k, (lo, hi) in boxes.items():
        v, q = _cube(lo, hi)
        _write_quad_ply(str(hab / ("mesh_semantic.ply_%d.ply" % k)), v, q)
        rv, rq = _cube(np.array(lo) + 0.01, np.array(hi) - 0.01, 6)        # a reconstruction 1 cm in on every side
        tris = np.concatenate([rq[:, [0, 1, 2]], rq[:, [0, 2, 3]]])
        vis.Mesh(rv, tris).export(str(mdir / ("iteration_10000_obj%d.obj" % k)))
    vis.Mesh(*_cube([0, 0, 0], [1, 1, 1])[:1], np.zeros((0, 3), np.int64)).export(str(mdir / "iteration_500_obj3.obj"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_3d_obj.py"), "--data_dir", str(data),
                        "--log_dir", str(logs)], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    out = logs / "room_0" / "eval_mesh"
    per = {k: np.load(out / ("metric_obj%d.npy" % k)) for k in boxes}
    allm = np.load(out / "metrics_3D_obj.npy")
    assert allm.shape == (3, 2, 1) and not (out / "metric_obj3.npy").exists()
    for k, m in per.items():
        assert m.shape == (3, 1)
        acc, comp, ratio = m[:, 0]
        # 1 cm offset surfaces, 10k samples: about 1 cm each way (plus the sampling's spread), all within 5 cm
        assert 0.5 < acc < 2.0 and 0.5 < comp < 2.0 and ratio == 100.0, (k, m)
    np.testing.assert_array_equal(allm[:, 0], per[1])
    assert "Acc | Comp | Comp Ratio 5cm" in r.stdout
