"""GPU: cnr_point_mesh_dist (csrc/point_mesh.hip) bit for bit against the numpy restatement (tests/pointmesh_cpu.py) and within
the 4 K bar of float64, ties, degenerate faces, determinism, translation, the closest point; cnr_sample_faces; and the public
functions built on them: metrics.calc_3d_metric_surface on closed forms, meshops.deviation, the two tools' new flags.

The bar of a distance d whose winning face has longest edge L is 4 K 2^-24 (d + L), K = pointmesh_cpu.K_F32, which
tests/test_pointmesh_host.py measures from the restatement on the random cases used here."""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import metric_cpu as MC
import pointmesh_cpu as P
from conftest import ROOT

pytestmark = pytest.mark.gpu

BAR_K = 4 * P.K_F32


@pytest.fixture(scope="module")
def mt():
    from cnr_amd import metrics
    return metrics


@functools.lru_cache(maxsize=None)
def _case(nq, F):
    """the scene and both references, computed once and shared: (q, verts, faces, closest_f32, closest_f64)"""
    q, v, f = P.random_case(nq, F)
    ref32, ref64 = P.closest_f32(q, v, f), P.closest_f64(q, v, f)
    for arr in ref32 + ref64:
        arr.setflags(write=False)
    return q, v, f, ref32, ref64


def _run(mt, q, mesh, **kw):
    out = mt.point_mesh_distance(q, mesh, closest=True, **kw)
    return tuple(t.cpu().numpy() for t in out)


def _chunks(nq, F):
    import cnr_amd
    return P.workspace_chunks(nq, F, cnr_amd._C.load().cnr_point_mesh_workspace_bytes(nq, F))


# ---- bit equality and the bar ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,F", P.BIT_CASES)
def test_bit_equal_to_the_restatement_and_within_the_bar_of_float64(mt, dev, nq, F):
    q, v, f, ref32, ref64 = _case(nq, F)
    if (nq, F) == P.BIT_CASES[-1]:
        assert _chunks(nq, F) >= 3 and nq * F < 4e6                     # the finish pass merges at least three chunks
    for mesh in ((v, f), (P.soup(v, f), None)):
        d, face, near = _run(mt, q, mesh)
        assert d.dtype == np.float32 and face.dtype == np.int32 and near.dtype == np.float32
        assert np.array_equal(d, ref32[0]), int((d != ref32[0]).sum())
        assert np.array_equal(face, ref32[1])
        assert np.array_equal(near, ref32[2])
    d64, f64 = ref64[0], ref64[1]
    bar = P.bar(d64, P.longest_edge(v, f, f64), BAR_K)
    err = np.abs(d.astype(np.float64) - d64)
    assert (err <= bar).all(), float((err / bar).max())                 # every query, none left out
    dist_only = mt.point_mesh_distance(q, (v, f))
    assert len(dist_only) == 2 and np.array_equal(dist_only[0].cpu().numpy(), d)


def _torch_f64(q, verts, faces, step=200):
    """an independent float64 evaluation on the device, in query chunks: the plane distance where the projection lies inside
    the triangle, else the minimum over the three edge segments -> (dist, face)"""
    tri = verts.double()[faces.long()]
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    n = torch.linalg.cross(b - a, c - a)
    nn = (n * n).sum(-1)

    def seg(p, u, v):
        e = v - u
        t = (((p - u) * e).sum(-1) / (e * e).sum(-1)).clamp(0.0, 1.0)
        r = p - (u + t[..., None] * e)
        return (r * r).sum(-1)
    dist, face = [], []
    for s in range(0, len(q), step):
        p = q[s:s + step].double()[:, None, :]
        h = ((p - a) * n).sum(-1)
        proj = p - (h / nn)[..., None] * n
        inside = torch.ones_like(h, dtype=torch.bool)
        for u, v in ((a, b), (b, c), (c, a)):
            inside &= (torch.linalg.cross((v - u).expand_as(proj), proj - u) * n).sum(-1) >= 0
        d2 = torch.where(inside, h * h / nn, torch.minimum(torch.minimum(seg(p, a, b), seg(p, b, c)), seg(p, c, a)))
        m = d2.min(1)
        dist.append(m.values.sqrt())
        face.append(m.indices)
    return torch.cat(dist), torch.cat(face)


def test_large_case_within_the_bar_of_float64(mt, dev):
    nq, F = P.LARGE_CASE
    q, v, f = P.random_case(nq, F)
    qd, vd, fd = (torch.from_numpy(x).to(dev) for x in (q, v, f))
    d, face = mt.point_mesh_distance(qd, (vd, fd))
    d64, f64 = _torch_f64(qd, vd, fd)
    L = torch.from_numpy(P.longest_edge(v, f, f64.cpu().numpy())).to(dev)
    bar = BAR_K * 2.0 ** -24 * (d64 + L)
    err = (d.double() - d64).abs()
    assert (err <= bar).all(), float((err / bar).max())
    assert float((face.long() == f64).double().mean()) > 0.99             # away from near-ties the face is the same
    assert _chunks(nq, F) > 1


# ---- ties --------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lowest_face(mt, dev):
    q = P.cube_tie_queries()
    ref = P.closest_f32(q, P.CUBE_VERTS, P.CUBE_FACES)
    pairs = P._pairs(q, P.face_records(P.corners(P.CUBE_VERTS, P.CUBE_FACES, np.float32)))[0]
    lowest = np.argmax(pairs == ref[3][:, None], axis=1)
    assert ((pairs == ref[3][:, None]).sum(1) >= 2).all()
    d, face, near = _run(mt, q, (P.CUBE_VERTS, P.CUBE_FACES))
    assert np.array_equal(face, lowest) and np.array_equal(d, ref[0]) and np.array_equal(near, ref[2])
    assert face[0] == 0 and d[0] == 0                                   # cube vertex 0, shared by 6 faces: the first of them


@pytest.mark.parametrize("nq,F", [(65, 257), (100, 2000)])
def test_a_mesh_concatenated_with_itself_answers_from_its_first_half(mt, dev, nq, F):
    q, v, f, ref32, _ = _case(nq, F)
    d, face, near = _run(mt, q, (np.concatenate([v, v]), np.concatenate([f, f + len(v)])))
    assert (face < F).all()
    assert np.array_equal(face, ref32[1]) and np.array_equal(d, ref32[0]) and np.array_equal(near, ref32[2])


# ---- degenerate faces --------------------------------------------------------------------------------------------------------
def test_degenerate_faces_give_the_distance_to_their_segment_or_point(mt, dev):
    q, verts, faces, is_deg = P.degenerate_mesh()
    d, face, near = _run(mt, q, (verts, faces))
    assert np.isfinite(d).all() and np.isfinite(near).all() and ((face >= 0) & (face < len(faces))).all()
    ref32 = P.closest_f32(q, verts, faces)
    assert np.array_equal(d, ref32[0]) and np.array_equal(face, ref32[1]) and np.array_equal(near, ref32[2])
    d64, f64, _, _ = P.closest_f64(q, verts, faces)
    won = is_deg[f64]
    assert won.sum() >= 40
    t = P.corners(verts, faces)[f64[won]]
    p = q.astype(np.float64)[won]
    seg = np.stack([P._segment_d2(p[:, None], t[:, None, i], t[:, None, (i + 1) % 3])[:, 0] for i in range(3)]).min(0)
    want = np.sqrt(seg)
    bar = P.bar(want, P.longest_edge(verts, faces, f64[won]), BAR_K)
    assert (np.abs(d[won].astype(np.float64) - want) <= bar).all()
    assert (np.abs(d.astype(np.float64) - d64) <= P.bar(d64, P.longest_edge(verts, faces, f64), BAR_K)).all()


# ---- determinism and translation ---------------------------------------------------------------------------------------------
def test_two_calls_are_bit_identical(mt, dev):
    q, v, f, _, _ = _case(2049, 1000)
    a = mt.point_mesh_distance(q, (v, f), closest=True)
    b = mt.point_mesh_distance(q, (v, f), closest=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_translation_changes_no_bit(mt, dev):
    q, v = P.grid_scene()
    d0, f0, c0 = _run(mt, q, (v, None))
    d1, f1, c1 = _run(mt, q + P.GRID_SHIFT, (v + P.GRID_SHIFT, None))
    assert np.array_equal(d0, d1) and np.array_equal(f0, f1)
    ref = P.closest_f32(q, v)
    assert np.array_equal(d0, ref[0]) and np.array_equal(f0, ref[1]) and np.array_equal(c0, ref[2])
    assert (d0 == 0).sum() >= 100 and (d0 > 0).sum() >= 100


# ---- the closest point -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,F", [(63, 65), (64, 256), (65, 257), (100, 2000)])
def test_closest_point_lies_on_the_winning_face_at_the_distance(mt, dev, nq, F):
    """The point's barycentric coordinates in the winning face lie in [0,1] up to the bar: stated in metres, its float64
    distance to that face is within the bar, plus the rounding of the point itself (q + r rounded once per coordinate: half
    a spacing each, sqrt(3)/2 spacings of the largest coordinate in length).  |q - closest| equals dist within 2 such spacings."""
    q, v, f, _, _ = _case(nq, F)
    d, face, near = _run(mt, q, (v, f))
    ulp = np.spacing(np.abs(near).max(1)).astype(np.float64)
    L = P.longest_edge(v, f, face)
    off = np.array([P.closest_f64(near[i:i + 1], v, f[face[i]:face[i] + 1])[0][0] for i in range(nq)])
    assert (off <= P.bar(d.astype(np.float64), L, BAR_K) + ulp).all()
    gap = np.sqrt(((q.astype(np.float64) - near.astype(np.float64)) ** 2).sum(1))
    assert (np.abs(gap - d) <= 2 * ulp).all()


# ---- samples -----------------------------------------------------------------------------------------------------------------
def test_sample_faces_equals_the_restatement(mt, dev):
    import cnr_amd
    _C = cnr_amd._C
    verts, u_edge = MC.dyadic_sampling_fixture()
    rng = np.random.default_rng(2)
    for soup_verts, u_fixed in ((verts, u_edge), (MC.dyadic_single_face()[0], MC.dyadic_single_face()[1])):
        tri = cnr_amd.devmesh.device_mesh((soup_verts, None), dev)
        _, cum = mt._area_scan(tri)
        cum_h = cum.cpu().numpy()
        for n in (1, 255, 256, 257, 5000):
            u = np.concatenate([u_fixed, rng.random((max(n - len(u_fixed), 0), 3))])[:n]         # the boundary draws first
            if n == 1:
                u = u_fixed[-1:]                                                                 # a draw beside a prefix boundary
            face = torch.empty(n, device=dev, dtype=torch.int32)
            _C.call("cnr_sample_faces", cum, tri.n_faces, torch.from_numpy(np.ascontiguousarray(u)).to(dev), n, face)
            assert np.array_equal(face.cpu().numpy(), P.sample_faces(cum_h, u[:, 0]))
            assert np.array_equal(face.cpu().numpy(), MC.sample_surface(MC.triangles(soup_verts), u)[0])


def test_sample_surface_faces_draws_sample_surface(mt, dev):
    from cnr_amd import vis
    v, f, _ = MC.sampling_random_inputs()
    mesh = vis.Mesh(v, f)
    pts, face = mt.sample_surface_faces(mesh, 5000, seed=3)
    assert torch.equal(pts, mt.sample_surface(mesh, 5000, seed=3)) and face.dtype == torch.int32
    u = np.random.default_rng(3).random((5000, 3))
    want_face, want_pts, _ = MC.sample_surface(MC.triangles(v, f), u)
    assert np.array_equal(face.cpu().numpy(), want_face)
    d, _ = mt.point_mesh_distance(pts, mesh)                                                # the samples lie on the mesh
    L = P.longest_edge(v, f, np.arange(len(f))).max()
    assert float(d.max()) <= float(P.bar(0.0, L, BAR_K)) + 2 * np.spacing(np.float32(np.abs(v).max()))


def test_non_finite_input_is_refused(mt, dev):
    q, v, f, _, _ = _case(63, 65)
    bad_q, bad_v = q.copy(), v.copy()
    bad_q[5, 1], bad_v[7, 2] = np.nan, np.inf
    for args in ((bad_q, (v, f)), (q, (bad_v, f)), (q, (v, f + 1000))):
        with pytest.raises(ValueError):
            mt.point_mesh_distance(*args)
    with pytest.raises(ValueError):
        mt.point_mesh_distance(q, (v[:0], f[:0]))


# ---- calc_3d_metric_surface on closed forms ----------------------------------------------------------------------------------
DELTA = 2.0 ** -5


def _cube_mesh(side, R, t):
    from cnr_amd import vis
    v = (P.CUBE_VERTS.astype(np.float64) - 0.5) * side
    return vis.Mesh(v @ R.T + t, P.CUBE_FACES.astype(np.int64))


def _cube_distance(x, side):
    """the float64 distance of points (in the cube's own frame) to the surface of the centred cube of `side`"""
    e = np.abs(x) - side / 2
    outside = np.sqrt((np.maximum(e, 0) ** 2).sum(1))
    return np.where((e <= 0).all(1), -e.max(1), outside)


@functools.lru_cache(maxsize=None)
def _cube_pose():
    """the first random pose under which oriented_bounds of the ground-truth cube contains the reconstruction"""
    from cnr_amd import metrics
    for seed in range(20):
        rng = np.random.default_rng(seed)
        R = MC.random_box(rng, np.zeros(3), np.ones(3))[0][:3, :3]
        t = rng.uniform(1.0, 3.0, 3)
        planes = metrics.box_planes(*metrics.oriented_bounds(_cube_mesh(1 + 2 * DELTA, R, t)))
        rec = _cube_mesh(1.0, R, t).vertices
        if all((((rec - h[:3]) * h[3:]).sum(1) >= DELTA / 2).all() for h in planes):
            return R, t
    raise AssertionError("no pose whose oriented box holds the reconstruction")


def test_calc_3d_metric_surface_on_concentric_cubes(mt, dev):
    """Every point of the unit cube's surface is delta from the cube of side 1 + 2 delta, and every point of the larger cube
    between delta (over a face) and sqrt(3) delta (at a corner) from the unit cube.  With delta = 2^-5 the corners' sqrt(3)
    delta = 0.0541 lies beyond 0.05, so at threshold 0.05 the recall is not 1 but the fraction of the ground truth's samples
    whose closed-form distance is below it; precision is 1.  At threshold 0.06 every distance is below and fscore == 1."""
    R, t = _cube_pose()
    rec, gt = _cube_mesh(1.0, R, t), _cube_mesh(1 + 2 * DELTA, R, t)
    N = 50000
    out = mt.calc_3d_metric_surface(rec, gt, N=N, seed=1)
    L = math.sqrt(2.0) * (1 + 2 * DELTA)
    # the bar of one distance, plus the fp32 rounding of the vertices and samples (a spacing of the largest coordinate each)
    bar = float(P.bar(math.sqrt(3) * DELTA, L, BAR_K)) + 4 * float(np.spacing(np.float32(np.abs(gt.vertices).max())))
    assert abs(out["accuracy_cm"] - 100 * DELTA) <= 100 * bar
    assert 100 * DELTA - 100 * bar <= out["completion_cm"] <= 100 * math.sqrt(3) * DELTA + 100 * bar
    assert out["precision"] == 1.0
    # the closed form of the recall from the very samples: calc_3d_metric's third draw, in the cube's frame
    rng = np.random.default_rng(1)
    rng.random((N, 3)), rng.random((N, 3))
    import cnr_amd
    gt_tri = cnr_amd.devmesh.device_mesh(gt, dev)
    gt_pc = mt._sample(gt_tri, N, rng).double().cpu().numpy()
    exact = _cube_distance((gt_pc - t) @ R, 1.0)
    sure_below, sure_above = (exact < 0.05 - bar).sum(), (exact >= 0.05 + bar).sum()
    assert sure_above >= 1 and sure_below / N <= out["recall"] <= 1 - sure_above / N and out["recall"] > 0.99
    assert out["completion_ratio"] == 100 * out["recall"]
    assert out["fscore"] == 2 * out["recall"] / (1 + out["recall"])
    assert abs(out["completion_cm"] - 100 * exact.mean()) <= 100 * bar
    wide = mt.calc_3d_metric_surface(rec, gt, N=N, seed=1, threshold=0.06)
    assert wide["fscore"] == 1.0 and wide["precision"] == 1.0 and wide["recall"] == 1.0 and wide["completion_ratio"] == 100.0
    # normals: a sample of the unit cube is closest to the parallel face of the larger cube; a ground-truth sample over an
    # edge or corner of the unit cube (the frame of width delta around each face: 1 - 1 / (1 + 2 delta)^2 of the area) is
    # equally close to two or three of its faces and may be given the perpendicular one
    assert out["normal_consistency_acc"] >= 0.99
    frame = 1 - 1 / (1 + 2 * DELTA) ** 2
    assert 1 - frame - 0.01 <= out["normal_consistency_comp"] <= 1.0
    assert out["normal_consistency"] == (out["normal_consistency_acc"] + out["normal_consistency_comp"]) / 2
    assert out["normal_pairs"] == (N, N)
    # per sample the distance to a mesh cannot exceed the distance to samples of that mesh
    pts = mt.calc_3d_metric(rec, gt, N=N, seed=1)
    assert out["accuracy_cm"] <= pts[0][0] + 100 * bar and out["completion_cm"] <= pts[1][0] + 100 * bar
    assert out["completion_ratio"] >= pts[2][0]


def test_calc_3d_metric_surface_with_the_box_elsewhere_is_none(mt, dev, capsys):
    R, t = np.eye(3), np.zeros(3)
    assert mt.calc_3d_metric_surface(_cube_mesh(1.0, R, t), _cube_mesh(1.0, R, t + 10.0), N=100) is None
    assert "no mesh found" in capsys.readouterr().out


# ---- deviation ---------------------------------------------------------------------------------------------------------------
def _sheet(n=64, seed=0):
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 2) / (n - 1.0)
    v = np.concatenate([g + rng.uniform(-0.3, 0.3, g.shape) / (n - 1.0), 0.02 * rng.normal(size=(n * n, 1))], 1) + [2.0, 1.0, 3.0]
    k = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)[None]).reshape(-1)
    f = np.concatenate([np.stack([k, k + n, k + n + 1], 1), np.stack([k, k + n + 1, k + 1], 1)])
    return v.astype(np.float32), f.astype(np.int32)


def test_deviation_of_a_mesh_from_itself_is_zero(mt, dev):
    from cnr_amd import meshops
    v, f = (torch.from_numpy(x).to(dev) for x in _sheet(24))
    out = meshops.deviation(v, f, v, f, samples=0)
    assert out["a_to_b"]["max"] == 0.0 and out["b_to_a"]["max"] == 0.0 and out["hausdorff"] == 0.0
    assert out["a_to_b"]["n"] == len(v) and out["a_to_b"]["mean"] == 0.0 and out["a_to_b"]["rms"] == 0.0
    lo, hi = v.double().amin(0), v.double().amax(0)
    assert out["diag"] == pytest.approx(float((hi - lo).norm()), rel=1e-12)
    with pytest.raises(ValueError):
        meshops.deviation(v, f, v, f, samples=0, include_vertices=False)


@pytest.mark.parametrize("placement", ["quadric", "mean", "representative"])
def test_deviation_of_a_clustered_sheet_stays_within_its_cell(mt, dev, placement):
    """Clustering keeps every output vertex inside its cluster's own cell, so an input vertex whose cluster survives lies
    within the cell's diagonal sqrt(3) c of that output vertex, hence of the output mesh."""
    from cnr_amd import meshops
    v, f = (torch.from_numpy(x).to(dev) for x in _sheet(64))
    c = 0.05
    ov, of, vmap, report = meshops.simplify(v, f, cell=c, placement=placement)
    assert 0 < report["faces_out"] < len(f)
    kept = vmap >= 0
    d, _ = mt.point_mesh_distance(v[kept], (ov, of))
    L = float(P.longest_edge(ov.cpu().numpy(), of.cpu().numpy(), np.arange(len(of))).max())
    bound = math.sqrt(3) * c + float(P.bar(math.sqrt(3) * c, L, BAR_K))
    assert kept.sum() > 3000 and float(d.max()) <= bound
    out = meshops.deviation(v, f, ov, of, samples=2000, seed=1)
    assert out["a_to_b"]["n"] == len(v) + 2000 and out["b_to_a"]["n"] == len(ov) + 2000
    assert 0 < out["a_to_b"]["mean"] <= out["a_to_b"]["rms"] <= out["a_to_b"]["max"] <= out["hausdorff"]
    assert out["hausdorff"] == max(out["a_to_b"]["max"], out["b_to_a"]["max"]) and out["hausdorff"] < 3 * c
    if placement == "representative":                                   # the output vertices ARE input vertices
        dv = meshops.deviation(ov, of, v, f, samples=0)
        assert dv["a_to_b"]["max"] == 0.0


# ---- the tools ---------------------------------------------------------------------------------------------------------------
def test_simplify_mesh_tool_prints_the_deviation_only_when_asked(dev, tmp_path, capsys):
    from cnr_amd import vis
    v, f = _sheet(24)
    src = str(tmp_path / "in.obj")
    vis.Mesh(v, f, np.zeros_like(v)).export(src)
    tool = os.path.join(ROOT, "tools", "simplify_mesh.py")
    r = subprocess.run([sys.executable, tool, src, str(tmp_path / "a.obj"), "--cell", "0.1", "--deviation", "3000"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import simplify_mesh
    finally:
        sys.path.pop(0)
    capsys.readouterr()
    simplify_mesh.main([src, str(tmp_path / "b.obj"), "--cell", "0.1"])
    plain = capsys.readouterr().out
    assert "deviation" not in plain and "hausdorff" not in plain and plain.count("\n") == 3
    extra = [ln for ln in r.stdout.splitlines() if ln.startswith(("deviation", "hausdorff"))]
    assert len(extra) == 3 and "input -> output" in extra[0] and "output -> input" in extra[1] and "of the diagonal" in extra[2]
    assert "".join(ln + "\n" for ln in r.stdout.splitlines() if ln not in extra) == plain
    assert open(tmp_path / "a.obj").read() == open(tmp_path / "b.obj").read()
    h = float(extra[2].split()[1])
    assert 0 < h < 0.1 * math.sqrt(3) + 1e-3


def test_eval_3d_obj_tool_flag_adds_its_columns_only_when_asked(dev, tmp_path, capsys):
    from cnr_amd import vis
    from test_metrics_gpu import _cube, _write_quad_ply
    data, logs = tmp_path / "Replica", tmp_path / "logs"
    hab, mdir = data / "room_0" / "habitat", logs / "room_0" / "scene_mesh"
    hab.mkdir(parents=True)
    mdir.mkdir(parents=True)
    (hab / "info_semantic.json").write_text(json.dumps({"objects": [{"id": 1, "class_id": 7}]}))
    gv, gq = _cube([0.0, 0.0, 0.0], [0.5, 0.4, 0.3], 2)
    _write_quad_ply(str(hab / "mesh_semantic.ply_1.ply"), gv, gq)
    rv, rq = _cube([0.01, 0.01, 0.01], [0.49, 0.39, 0.29], 2)
    vis.Mesh(rv, np.concatenate([rq[:, [0, 1, 2]], rq[:, [0, 2, 3]]])).export(str(mdir / "iteration_10000_obj1.obj"))
    tool = os.path.join(ROOT, "tools", "eval_3d_obj.py")
    r = subprocess.run([sys.executable, tool, "--data_dir", str(data), "--log_dir", str(logs), "--surface"],
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    out = logs / "room_0" / "eval_mesh"
    with_flag = np.load(out / "metrics_3D_obj.npy")
    table = json.loads((out / "metrics_3D_obj_surface.json").read_text())
    row = table["objects"]["1"]
    assert table["mean"]["accuracy_cm"] == row["accuracy_cm"]
    # the surfaces are 1 cm apart: accuracy is 1 cm exactly (up to fp32), completion between 1 and sqrt(3) cm
    assert abs(row["accuracy_cm"] - 1.0) < 1e-3 and 1.0 - 1e-3 <= row["completion_cm"] <= math.sqrt(3) + 1e-3
    assert row["fscore"] == 1.0 and row["completion_ratio"] == 100.0 and row["normal_consistency_acc"] > 0.99
    assert row["accuracy_cm"] <= with_flag[0, 0, 0] and row["completion_cm"] <= with_flag[1, 0, 0]
    (out / "metrics_3D_obj_surface.json").unlink()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import eval_3d_obj
    finally:
        sys.path.pop(0)
    capsys.readouterr()
    eval_3d_obj.main(["--data_dir", str(data), "--log_dir", str(logs)])
    plain = capsys.readouterr().out
    assert "surface" not in plain and not (out / "metrics_3D_obj_surface.json").exists()
    np.testing.assert_array_equal(np.load(out / "metrics_3D_obj.npy"), with_flag)
    extra = [ln for ln in r.stdout.splitlines() if ln.startswith("surface ")]
    assert [ln for ln in r.stdout.splitlines() if ln not in extra] == plain.splitlines()
    assert len(extra) == 2 and extra[0].startswith("surface obj 1: accuracy_cm") and extra[1].startswith("surface mean: accuracy_cm")
