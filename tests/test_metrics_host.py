"""CPU: the mesh-evaluation pieces that run on the host (metrics.oriented_bounds / box_planes, vis.load_mesh), the numpy
restatement of csrc/metric.hip (tests/metric_cpu.py) against analytic areas and the reference's metrics.py (golden fixtures
under tests/golden/metric/), and a warning-free build of the new kernels."""
import glob
import os
import struct
import subprocess

import numpy as np
import pytest

import metric_cpu as K
from conftest import ROOT

PKG = os.path.join(ROOT, "category-nerf-reconstruction-official_amd")
METRIC_GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "metric", "*.npz")))


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    return q


def _cuboid(ext):
    c = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], np.float64)
    return (c - 0.5) * np.asarray(ext)


def _in_box(pts, T, ext, tol):
    loc = pts @ T[:3, :3].T + T[:3, 3]
    return (np.abs(loc) <= np.asarray(ext) / 2 + tol).all()


@pytest.mark.parametrize("seed", range(8))
def test_oriented_bounds_recovers_rotated_cuboids(seed):
    from cnr_amd import metrics
    rng = np.random.default_rng(seed)
    ext = rng.uniform(0.2, 3.0, 3)
    R, t = _rotation(rng), rng.normal(size=3) * 5
    # the corners and random points inside the cuboid: the hull is the cuboid
    pts = np.concatenate([_cuboid(ext), (rng.uniform(-0.5, 0.5, (200, 3)) * ext)]) @ R.T + t
    T, e = metrics.oriented_bounds(pts)
    np.testing.assert_allclose(np.sort(e), np.sort(ext), rtol=0, atol=1e-6)
    np.testing.assert_allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-12)
    assert np.linalg.det(T[:3, :3]) > 0
    assert _in_box(pts, T, e, 1e-9)


@pytest.mark.parametrize("seed", range(6))
def test_oriented_bounds_of_random_clouds(seed):
    from cnr_amd import metrics
    rng = np.random.default_rng(100 + seed)
    pts = rng.normal(size=(300, 3)) * rng.uniform(0.3, 2.0, 3) @ _rotation(rng).T + rng.normal(size=3)
    T, e = metrics.oriented_bounds(pts)
    assert _in_box(pts, T, e, 1e-9)
    vol = np.prod(e)
    aabb = np.prod(pts.max(0) - pts.min(0))
    _, _, vt = np.linalg.svd(pts - pts.mean(0))
    loc = pts @ vt.T
    pca = np.prod(loc.max(0) - loc.min(0))
    assert vol <= aabb * (1 + 1e-12) and vol <= pca * (1 + 1e-12), (vol, aabb, pca)


def test_oriented_bounds_of_a_flat_set():
    from cnr_amd import metrics
    rng = np.random.default_rng(3)
    pts = np.concatenate([rng.uniform(-1, 1, (50, 2)), np.zeros((50, 1))], 1) @ _rotation(rng).T
    T, e = metrics.oriented_bounds(pts)
    assert np.sort(e)[0] < 1e-9 and _in_box(pts, T, e, 1e-9)


def test_box_planes_are_the_box_faces():
    from cnr_amd import metrics
    rng = np.random.default_rng(5)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = _rotation(rng), rng.normal(size=3)
    ext = np.array([0.5, 1.0, 2.0])
    P = metrics.box_planes(T, ext)
    inside = np.linalg.inv(T)[:3, :3] @ (rng.uniform(-0.49, 0.49, (100, 3)) * ext).T + np.linalg.inv(T)[:3, 3:]
    d = (inside.T[:, None, :] - P[None, :, :3]) * P[None, :, 3:]
    assert (d.sum(2) > 0).all()
    outside = np.linalg.inv(T)[:3, :3] @ np.array([[0.3, 0, 0], [0, 0.6, 0], [0, 0, -1.1]]).T + np.linalg.inv(T)[:3, 3:]
    d = ((outside.T[:, None, :] - P[None, :, :3]) * P[None, :, 3:]).sum(2)
    assert (d.min(1) < 0).all()


# ---- readers -----------------------------------------------------------------------------------------------------------
def _quad_cube():
    v = _cuboid([1.0, 1.0, 1.0]) + 0.5
    q = np.array([[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]], np.int64)
    return v, q


def _write_ply(path, v, polys, binary, count_type="uchar", index_type="int"):
    head = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "comment test",
            "element vertex %d" % len(v), "property float x", "property float y", "property float z",
            "property float nx", "property float ny", "property float nz", "property uchar red", "property uchar green",
            "property uchar blue", "element face %d" % len(polys),
            "property list %s %s vertex_indices" % (count_type, index_type), "property int object_id", "end_header"]
    fmt = {"uchar": "B", "int": "i", "uint": "I"}
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode())
        for p in v:
            if binary:
                f.write(struct.pack("<6f3B", *p, 0.0, 0.0, 1.0, 10, 20, 30))
            else:
                f.write(("%r %r %r 0 0 1 10 20 30\n" % tuple(float(x) for x in p)).encode())
        for p in polys:
            if binary:
                f.write(struct.pack("<" + fmt[count_type] + fmt[index_type] * len(p) + "i", len(p), *p, 7))
            else:
                f.write((" ".join(str(int(x)) for x in [len(p), *p, 7]) + "\n").encode())


def _fan(polys):
    return np.array([[p[0], p[k], p[k + 1]] for p in polys for k in range(1, len(p) - 1)], np.int64)


@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("kind", ["quads", "triangles", "mixed"])
def test_ply_reader(tmp_path, binary, kind):
    from cnr_amd import vis
    v, q = _quad_cube()
    polys = {"quads": [list(p) for p in q], "triangles": [list(t) for t in _fan(q)],
             "mixed": [list(q[0])] + [list(t) for t in _fan(q[1:])] + [[0, 1, 5, 7, 3]]}[kind]
    for ct, it in (("uchar", "int"), ("int", "uint")):
        p = str(tmp_path / ("m_%s_%s.ply" % (ct, it)))
        _write_ply(p, v, polys, binary, ct, it)
        m = vis.load_mesh(p)
        np.testing.assert_allclose(m.vertices, v.astype(np.float32), rtol=0, atol=0)
        assert np.array_equal(m.faces, _fan(polys))


def test_obj_reader_face_syntaxes(tmp_path):
    from cnr_amd import vis
    v, q = _quad_cube()
    lines = ["# cube", "o cube"] + ["v %r %r %r 0.5 0.5 0.5" % tuple(float(x) for x in p) for p in v] + ["vt 0 0", "vn 0 0 1"]
    forms = [lambda i: "%d" % i, lambda i: "%d/1" % i, lambda i: "%d//1" % i, lambda i: "%d/1/1" % i]
    for k, p in enumerate(q):
        lines.append("f " + " ".join(forms[k % 4](i + 1) for i in p))
    lines.append("f -8 -7 -6")                      # relative indices: vertices 0, 1, 2
    p = tmp_path / "m.obj"
    p.write_text("\n".join(lines) + "\n")
    m = vis.load_mesh(str(p))
    np.testing.assert_allclose(m.vertices, v)
    assert np.array_equal(m.faces, np.concatenate([_fan(q), [[0, 1, 2]]]))


def test_load_mesh_reads_what_mesh_export_writes(tmp_path):
    from cnr_amd import vis
    rng = np.random.default_rng(1)
    m = vis.Mesh(rng.normal(size=(30, 3)), rng.integers(0, 30, (40, 3)))
    back = vis.load_mesh(m.export(str(tmp_path / "e.obj")))
    np.testing.assert_allclose(back.vertices, m.vertices, atol=1e-8)
    assert np.array_equal(back.faces, m.faces)


# ---- the restatement ---------------------------------------------------------------------------------------------------
def _cube_surface():
    v, q = _quad_cube()
    return K.triangles(v, _fan(q))


def _aabb_planes(lo, hi):
    rows = []
    for i in range(3):
        o, n = np.zeros(3), np.zeros(3)
        o[i], n[i] = lo[i], 1.0
        rows.append(np.concatenate([o, n]))
        o, n = np.zeros(3), np.zeros(3)
        o[i], n[i] = hi[i], -1.0
        rows.append(np.concatenate([o, n]))
    return np.array(rows)


def test_clip_restatement_area_on_a_cut_cube():
    tri = _cube_surface()
    assert K.face_areas(tri).sum() == pytest.approx(6.0, rel=1e-15)
    # x in [.25, .75], y unbounded, z in [.5, 2]: half of each y face's upper part (2 x 0.25) and half of the top (0.5)
    out = K.clip_box(tri, _aabb_planes([0.25, -1.0, 0.5], [0.75, 2.0, 2.0]))
    assert K.face_areas(out).sum() == pytest.approx(1.0, rel=1e-12)
    # a box strictly inside the cube meets no face; one around it keeps all six
    assert len(K.clip_box(tri, _aabb_planes([0.1] * 3, [0.9] * 3))) == 0
    assert K.face_areas(K.clip_box(tri, _aabb_planes([-1] * 3, [2] * 3))).sum() == pytest.approx(6.0, rel=1e-15)


def test_clip_restatement_rotated_box_matches_metrics_planes():
    from cnr_amd import metrics
    tri = _cube_surface()
    # the same cut as above, as a box whose frame is a rotation that permutes and flips the axes, through metrics.box_planes
    R = np.array([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    assert np.linalg.det(R) == 1.0
    lo, hi = np.array([0.25, -1.0, 0.5]), np.array([0.75, 2.0, 2.0])
    c = (lo + hi) / 2
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, -R @ c
    out = K.clip_box(tri, metrics.box_planes(T, np.abs(R) @ (hi - lo)))
    assert K.face_areas(out).sum() == pytest.approx(1.0, rel=1e-12)
    # and a box turned 45 degrees about z through the cube's centre, half-width w across: with a = x - 1/2, b = y - 1/2 it
    # keeps |a + b| <= w / s and |b - a| <= w / s (s = sqrt(1/2))
    s = np.sqrt(0.5)
    Rz = np.array([[s, s, 0.0], [-s, s, 0.0], [0.0, 0.0, 1.0]])
    T[:3, :3], T[:3, 3] = Rz, -Rz @ np.full(3, 0.5)
    w = 0.5
    out = K.clip_box(tri, metrics.box_planes(T, [2 * w, 2 * w, 10.0]))
    side = 2 * (w / s - 0.5)                               # each side face (a = -1/2 etc.): |b| <= w / s - 1/2, height 1
    leg = 1.0 - w / s                                      # top and bottom: the unit square less four corner triangles
    cap = 1.0 - 4 * 0.5 * leg * leg
    assert K.face_areas(out).sum() == pytest.approx(4 * side + 2 * cap, rel=1e-12)


def test_sampling_restatement_is_area_weighted():
    tri = K.triangles(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [3, 0, 1], [0, 3, 1]], np.float32),
                      np.array([[0, 1, 2], [3, 4, 5]]))
    u = np.random.default_rng(0).random((40000, 3))
    face, pts, cum = K.sample_surface(tri, u)
    np.testing.assert_allclose(cum, [0.5, 5.0])
    assert abs((face == 0).mean() - 0.1) < 0.01
    # inside their triangles: barycentric coordinates in [0, 1]
    assert (pts[face == 0, :2].sum(1) <= 1 + 1e-6).all() and (pts[face == 1, :2].sum(1) <= 3 + 1e-5).all()
    assert (pts[:, :2] >= -1e-7).all()


@pytest.mark.parametrize("path", METRIC_GOLDEN, ids=[os.path.basename(p)[:-4] for p in METRIC_GOLDEN])
def test_restatement_matches_the_reference_metrics(path):
    z = np.load(path)
    gt, rec = z["gt"], z["rec"]
    assert K.accuracy(gt, rec) == pytest.approx(float(z["accuracy"]), rel=1e-12)
    assert K.completion(gt, rec) == pytest.approx(float(z["completion"]), rel=1e-12)
    assert K.chamfer(gt, rec) == pytest.approx(float(z["chamfer"]), rel=1e-12)
    assert K.accuracy_ratio(gt, rec, float(z["th_acc"])) == float(z["accuracy_ratio"])
    assert K.completion_ratio(gt, rec, float(z["th_comp"])) == float(z["completion_ratio"])


def test_golden_metric_fixtures_exist_and_stay_small():
    assert len(METRIC_GOLDEN) >= 3
    assert sum(os.path.getsize(p) for p in METRIC_GOLDEN) < 400 * 1024
    sizes = {(len(np.load(p)["gt"]), len(np.load(p)["rec"])) for p in METRIC_GOLDEN}
    assert any(a != b for a, b in sizes)


# ---- the fixtures of test_metrics_gpu.py: each condition they rest on, from the restatement alone -----------------------------
def _mc_mesh_cpu(D=48, r0=0.85, centre=(0.0, 0.0, 0.0), scale=1.0):
    """test_metrics_gpu._mc_mesh with the numpy marching cubes (the two agree to 2e-6, test_meshing_gpu.py)"""
    import mc_cpu as M
    from cnr_amd import vis
    v, n, f = M.marching_cubes(M.sphere(D, r0, 4.0, centre))
    m = vis.Mesh(v, f, n)
    m.apply_translation([-0.5, -0.5, -0.5]).apply_scale(2.0 * scale)
    return m


def _general_clip_cases():
    from cnr_amd import metrics
    for F, v, T, ext in K.clip_soup_cases():
        yield "soup%d" % F, K.triangles(v), metrics.box_planes(T, ext)
    m = _mc_mesh_cpu(48)
    T, ext = K.random_box(np.random.default_rng(22), (0.1, 0.0, -0.2), (1.2, 0.9, 1.0))
    yield "sphere", K.triangles(m.vertices, m.faces), metrics.box_planes(T, ext)
    yield "fans", K.triangles(K.fan_soup()), metrics.box_planes(*K.UNIT_BOX)


def test_general_clip_fixtures_decide_far_from_rounding():
    """Every kept / dropped decision of the general-position cases is taken at |dist| >= 1e-9 S (S the largest coordinate),
    seven orders above the 2^-53 S by which two fp64 evaluations of a dist can differ: the GPU takes the same decisions, so
    its output can be compared row for row."""
    for name, tri, planes in _general_clip_cases():
        out, counts, closest = K.clip_box_info(tri, planes)
        assert closest >= 1e-9 * np.abs(tri).max(), (name, closest)
        assert len(out) == counts.sum() > 0 and len(counts) == len(tri), name
        if name.startswith("soup") and len(tri) >= 63:
            assert (counts == 0).any() and (counts >= 3).any(), name


def test_fan_soup_has_every_triangle_count_mixed_within_a_wave():
    from cnr_amd import metrics
    tri = K.triangles(K.fan_soup())
    _, counts, _ = K.clip_box_info(tri, metrics.box_planes(*K.UNIT_BOX))
    hist = np.bincount(counts, minlength=8)
    assert len(hist) == 8 and (hist > 0).all(), hist                   # 0 .. 7, and no face beyond 9 vertices
    assert hist[7] >= 8                                                # the eight constructed hexagon cuts
    # the construction itself, unperturbed: 9 vertices
    _, c, closest = K.clip_box_info(K.hexagon_triangle()[None], metrics.box_planes(*K.UNIT_BOX))
    assert c.tolist() == [7] and closest > 1e-3
    # each of the three count bits is set in some lanes and clear in others of every full wave
    full = counts[:len(counts) // 64 * 64].reshape(-1, 64)
    for b in range(3):
        bit = (full >> b) & 1
        assert ((bit.sum(1) > 0) & (bit.sum(1) < 64)).all(), b
    assert len(counts) % 256 != 0 and len(counts) > 256


def test_on_plane_fixture_is_exact_and_touching_faces_survive_as_zero_area():
    from cnr_amd import metrics
    v, want = K.on_plane_soup()
    tri = K.triangles(v)
    planes = metrics.box_planes(*K.UNIT_BOX)
    assert np.array_equal(np.abs(planes[:, :3]).sum(1), np.full(6, 0.5)) and np.array_equal(np.abs(planes[:, 3:]).sum(1), np.ones(6))
    out, counts, closest = K.clip_box_info(tri, planes)
    assert closest == 0.0 and counts.tolist() == want.tolist()
    assert np.array_equal(out * 1024, np.round(out * 1024))            # dyadic: the same in any fp64 evaluation
    area = K.face_areas(out)
    first = np.cumsum(counts) - counts
    assert area[first[3]] == 0.0 and (out[first[3]] == tri[3][0]).all()        # touched by one corner from outside
    assert area[first[0]] == K.face_areas(tri)[0] and (area[first[1]:first[1] + 2] == 0).all()
    assert (np.abs(out) <= 0.5).all()


def _exact_sampling(verts, u):
    """the sampling of a soup in rational arithmetic -> (face, points as floats): exact, or an AssertionError"""
    from fractions import Fraction as Fr
    tri = [[[Fr(float(x)) for x in p] for p in t] for t in np.asarray(verts, np.float64).reshape(-1, 3, 3)]
    area = [abs((t[1][0] - t[0][0]) * (t[2][1] - t[0][1]) - (t[1][1] - t[0][1]) * (t[2][0] - t[0][0])) / 2 for t in tri]
    cum = [sum(area[:k + 1]) for k in range(len(area))]
    faces, pts = [], []
    for u0, a, b in u:
        target = Fr(float(u0)) * cum[-1]
        f = next(k for k in range(len(cum)) if cum[k] >= target)
        a, b = Fr(float(a)), Fr(float(b))
        if a + b > 1:
            a, b = abs(a - 1), abs(b - 1)
        t = tri[f]
        p = [(t[1][k] - t[0][k]) * a + (t[2][k] - t[0][k]) * b + t[0][k] for k in range(3)]
        faces.append(f)
        pts.append([float(x) for x in p])
        assert all(Fr(x) == y for x, y in zip(pts[-1], p))             # the point is an fp64 number
    return np.array(faces), np.array(pts), [float(c) for c in cum]


@pytest.mark.parametrize("which", ["many", "single"])
def test_dyadic_sampling_fixture_is_exact(which):
    import math
    verts, u = K.dyadic_sampling_fixture() if which == "many" else K.dyadic_single_face()
    tri = K.triangles(verts)
    area = K.face_areas(tri)
    cum = np.cumsum(area)
    assert cum.tolist() == [math.fsum(area[:k + 1]) for k in range(len(area))]
    assert math.frexp(cum[-1])[0] == 0.5                               # a power of two: u0 * total is exact
    face, pts, cum_r = K.sample_surface(tri, u)
    want_face, want_pts, want_cum = _exact_sampling(verts, u)
    assert cum_r.tolist() == want_cum and np.array_equal(face, want_face)
    assert np.array_equal(pts, want_pts.astype(np.float32))
    # what the draws cover
    assert (u[:, 0] == 0).any() and (u[:, 0] == 1.0 - 2.0 ** -53).any()
    s = u[:, 1] + u[:, 2]
    assert (s == 1.0).any() and (s == 1.0 + 2.0 ** -52).any() and (s < 1).any() and (s > 1.25).any()
    if which == "many":
        assert area[0] == 0 and area[-1] == 0 and (area[1:-1] == 0).any() and len(np.unique(cum)) < len(cum)
        target = u[:, 0] * cum[-1]
        on = np.isin(target, cum)
        assert set(target[on]) == set(cum) - {cum[-1]}                 # every boundary below the total is hit exactly ...
        assert (cum[face[on]] == target[on]).all()                     # ... and belongs to the face that ends there:
        assert (face[on] == np.searchsorted(cum, target[on], "left")).all()       # the first of equal prefixes
        assert face.max() == len(cum) - 2 and face.min() == 0          # never the trailing zero-area face; u0 = 0 -> face 0
        assert set(face) == {0} | set(np.flatnonzero(area))             # every face with an area, and no other but face 0
    else:
        assert len(tri) == 1 and (face == 0).all()


def test_random_sampling_draws_stay_off_the_prefix_boundaries():
    """The random comparison of test_metrics_gpu.py leaves out no sample: none of the committed seed's draws lies within
    1e-12 of a prefix boundary (about 4e-3 are expected to).  The marching-cubes meshes here come from the numpy restatement,
    whose vertices agree with the GPU's to 2e-6; the GPU test asserts the same on its own meshes."""
    from cnr_amd import vis
    v, f, us = K.sampling_random_inputs()
    meshes = [_mc_mesh_cpu(33), _mc_mesh_cpu(64, 0.6, (0.2, 0.0, 0.1), 3.0), vis.Mesh(v, f)]
    for m, u in zip(meshes, us):
        _, _, _, near = K.sampling_near_boundaries(K.triangles(m.vertices, m.faces), u)
        assert near.sum() == 0


# ---- build and ABI -----------------------------------------------------------------------------------------------------
def test_metric_build_is_warning_free():
    """csrc/metric.hip, compiled with the Makefile's own compiler and flags (into a temporary file), gives no warning"""
    import tempfile
    csrc = os.path.join(PKG, "csrc")
    cmd = subprocess.run(["make", "-s", "-C", csrc, "--no-print-directory", "--eval",
                          "print-compile: ; @echo $(HIPCC) $(CXXFLAGS)", "print-compile"],
                         capture_output=True, text=True, check=True).stdout.split()
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run(cmd + ["-c", os.path.join(csrc, "metric.hip"), "-o", os.path.join(d, "metric.o")],
                             capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "warning" not in (out.stdout + out.stderr).lower(), out.stderr


def test_metric_argument_errors_without_a_device():
    import cnr_amd
    lib = cnr_amd._C.load()
    assert lib.cnr_nn_workspace_bytes(0, 5) == -2 and lib.cnr_nn_workspace_bytes(5, 0) == -2
    assert lib.cnr_nn_workspace_bytes(10000, 10000) > 0
    assert lib.cnr_face_area_workspace_bytes(0) == -2 and lib.cnr_clip_box_workspace_bytes(0) == -2
    assert lib.cnr_dist_stats_workspace_bytes(0) == -2 and lib.cnr_dist_stats_workspace_bytes(1) > 0
    assert lib.cnr_nn_dist(None, 4, None, 4, None, None, None) == -1
    assert lib.cnr_dist_stats(None, 4, 0.5, None, None, None, None) == -1
    assert lib.cnr_face_area_scan(None, None, 4, None, None, None, None) == -1
    assert lib.cnr_sample_surface(None, None, 4, None, None, 4, None, None) == -1
    assert lib.cnr_clip_box_count(None, None, 4, None, None, None, None) == -1
    assert lib.cnr_clip_box_emit(None, None, 4, None, None, None, None) == -1
