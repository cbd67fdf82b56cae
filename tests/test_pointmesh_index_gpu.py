"""GPU: the tile-box index of the point-to-mesh distance (csrc/point_mesh_index.hip, metrics.MeshIndex).  The build bit for bit
against the numpy restatement (tests/pointmesh_index_cpu.py); the query bit for bit against ``pointmesh_cpu.closest_f32`` (the
restatement the brute force is pinned to) and against the brute-force kernel itself; ties, degenerate faces, determinism,
translation, the near-planar scene aimed at the skip rule's margin; that tiles are really skipped; and the opt-in flags of
calc_3d_metric_surface, meshops.deviation and the tools."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pointmesh_cpu as P
import pointmesh_index_cpu as X
from conftest import ROOT

pytestmark = pytest.mark.gpu

TILE, GROUP = X.TILE, X.GROUP
RESULT_CASES = ((1, 1), (1, 257), (63, 65), (65, 257), (GROUP - 1, TILE), (GROUP + 1, 2 * TILE), (2049, 1000), (100, 2000))


@pytest.fixture(scope="module")
def mt():
    from cnr_amd import metrics
    assert metrics._index_params() == (TILE, GROUP)
    return metrics


@functools.lru_cache(maxsize=None)
def _case(nq, F):
    """the scene and closest_f32 of it, computed once and shared"""
    q, v, f = P.random_case(nq, F)
    ref = P.closest_f32(q, v, f)
    for arr in (q, v, f) + ref:
        arr.setflags(write=False)
    return q, v, f, ref


def _query(mt, q, mesh, **kw):
    """-> (dist, face, closest) as numpy and the stats"""
    *out, stats = mt.MeshIndex(mesh).query(q, closest=True, stats=True, **kw)
    assert stats["tile_faces"] == TILE and stats["group_queries"] == GROUP and stats["groups"] == -(-len(q) // GROUP)
    assert stats["groups"] <= stats["tiles_visited"] <= stats["groups"] * stats["tiles"]
    return tuple(t.cpu().numpy() for t in out), stats


def _equal(got, ref):
    d, face, near = got
    assert d.dtype == np.float32 and face.dtype == np.int32 and near.dtype == np.float32
    assert np.array_equal(face, ref[1]), int((face != ref[1]).sum())
    assert np.array_equal(d, ref[0]), int((d != ref[0]).sum())
    assert np.array_equal(near, ref[2])


# ---- the build ----------------------------------------------------------------------------------------------------------------
def _built(mt, dev, verts, faces):
    """the device's keys, records (F,16) and tile rows (T,8) of a mesh"""
    import cnr_amd
    ix = mt.MeshIndex((verts, faces))
    tri = cnr_amd.devmesh.device_mesh((verts, faces), dev)
    keys = torch.empty(ix.faces, device=dev, dtype=torch.int32)
    cnr_amd._C.call("cnr_pm_index_keys", tri.verts, tri.faces, tri.n_faces, ix.bbox, keys)
    raw = ix.index.cpu().numpy()
    F, T = ix.faces, ix.tiles
    assert len(raw) == X.index_bytes(F) and T == -(-F // TILE)
    rec = raw[:64 * F].view(np.float32).reshape(F, 16)
    rows = raw[P.align256(64 * F):][:32 * T].view(np.float32).reshape(T, 8)
    return keys.cpu().numpy(), rec, rows, ix.bbox.cpu().numpy()


def _build_equals_the_restatement(mt, dev, verts, faces):
    keys, rec, rows, bbox = _built(mt, dev, verts, faces)
    want = X.build(verts, faces)
    assert np.array_equal(bbox, want["bbox"]) and np.array_equal(keys, want["keys"])
    assert np.array_equal(rec[:, 15].view(np.int32), want["order"])
    a, ab, ac, e00, e01, e11, nh = want["rec"]
    flat = np.concatenate([a, ab, ac, e00[:, None], e01[:, None], e11[:, None], nh], 1)
    assert np.array_equal(rec[:, :15], flat.astype(np.float32))          # (as values: a degenerate face's unused normal may be -0)
    assert np.array_equal(rows[:, :3], want["lo"]) and np.array_equal(rows[:, 4:7], want["hi"])
    assert np.array_equal(rows[:, 3], want["lmax"]) and np.array_equal(rows[:, 7].view(np.int32), want["first"])
    return want


@pytest.mark.parametrize("F", [1, 2, TILE - 1, TILE, TILE + 1, 1000])
def test_keys_records_and_tile_table_are_the_restatement(mt, dev, F):
    _, v, f = P.random_case(8, F)
    want = _build_equals_the_restatement(mt, dev, v, f)
    _build_equals_the_restatement(mt, dev, P.soup(v, f), None)
    # Lmax is not below the fp32 length of any edge of its tile
    t = P.corners(v, f, np.float32)[want["order"]]
    e = np.stack([t[:, 1] - t[:, 0], t[:, 2] - t[:, 0], t[:, 2] - t[:, 1]], 1)
    assert (np.sqrt(P._dot(e, e)).max(1) <= np.repeat(want["lmax"], TILE)[:F]).all()


def test_a_mesh_of_coincident_vertices_and_a_mesh_of_degenerate_faces(mt, dev):
    point = np.tile(np.array([[1.5, -2.0, 0.25]], np.float32), (3 * 70, 1))                 # a zero-extent box: every key is 0
    want = _build_equals_the_restatement(mt, dev, point, None)
    assert (want["keys"] == 0).all() and (want["lmax"] == 0).all()
    q = P.random_case(130, 1)[0]
    got, _ = _query(mt, q, (point, None))
    _equal(got, P.closest_f32(q, point))
    assert (got[1] == 0).all()                                                              # 70 equal faces: the first wins
    dq, verts, faces, is_deg = P.degenerate_mesh()
    only = np.ascontiguousarray(faces[is_deg])
    _build_equals_the_restatement(mt, dev, verts, only)
    got, _ = _query(mt, dq, (verts, only))
    _equal(got, P.closest_f32(dq, verts, only))
    assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all()


def test_keys_of_an_extent_that_overflows_are_the_restatement(mt, dev):
    """hi - lo = inf on x: cell 0 on that axis on the device as in numpy, not the conversion of a NaN"""
    import cnr_amd
    big = np.float32(3e38)
    v = np.array([[-big, 0, 0], [big, 1, 0], [0, 0, 1], [big, 1, 1], [big, 0.5, 0.25], [1, 1, 1]], np.float32)
    bbox = X.bbox_of(v)
    vd, bd = torch.from_numpy(v).to(dev), torch.from_numpy(bbox).to(dev)
    keys = torch.empty(2, device=dev, dtype=torch.int32)
    cnr_amd._C.call("cnr_pm_index_keys", vd, None, 2, bd, keys)
    assert np.array_equal(keys.cpu().numpy(), X.face_keys(P.corners(v, None, np.float32), bbox))
    qk = torch.empty(len(v), device=dev, dtype=torch.int32)
    cnr_amd._C.call("cnr_pm_query_keys", vd, len(v), bd, qk)
    want = X.query_keys(v, bbox)
    assert np.array_equal(qk.cpu().numpy(), want) and (want & 0x09249249 == 0).all() and len(np.unique(want)) >= 4


def test_check_applies_to_the_points_of_a_given_index(mt, dev):
    q, v, f, _ = _case(63, 65)
    bad = q.copy()
    bad[3, 0] = np.nan
    for ix in (mt.MeshIndex((v, f)), mt.MeshIndex((v, f), check=False)):
        with pytest.raises(ValueError):
            mt.point_mesh_distance(bad, None, index=ix)                                     # check=True is the call's default
        with pytest.raises(ValueError):
            ix.query(bad, check=True)
    assert len(mt.point_mesh_distance(q, None, index=mt.MeshIndex((v, f)), check=False)) == 2
    with pytest.raises(ValueError):
        mt.MeshIndex((v, f)).query(bad)                                                     # the index's own setting


# ---- results against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,F", RESULT_CASES)
def test_query_is_bit_equal_to_closest_f32(mt, dev, nq, F):
    q, v, f, ref = _case(nq, F)
    got, stats = _query(mt, q, (v, f))
    _equal(got, ref)
    _equal(_query(mt, q, (P.soup(v, f), None))[0], ref)
    visited = X.search(q, v, f)[4]                                                          # the restated skip rule, tile for tile
    assert stats["tiles_visited"] == int(visited.sum()) and stats["tiles"] == -(-F // TILE)
    plain = mt.point_mesh_distance(q, (v, f), index=True)
    assert len(plain) == 2 and np.array_equal(plain[0].cpu().numpy(), ref[0]) and np.array_equal(plain[1].cpu().numpy(), ref[1])


def test_queries_far_outside_the_box_get_clamped_keys(mt, dev):
    q, v, f, _ = _case(65, 257)
    far = q + np.float32(100.0)
    bbox = X.bbox_of(v)
    assert len(np.unique(X.query_keys(far, bbox))) == 1                                     # every key is the far corner's
    _equal(_query(mt, far, (v, f))[0], P.closest_f32(far, v, f))
    _equal(_query(mt, -far, (v, f))[0], P.closest_f32(-far, v, f))


def test_queries_on_a_tile_box_face_have_a_zero_gap(mt, dev):
    _, v, f, _ = _case(100, 2000)
    ix = X.build(v, f)
    rng = np.random.default_rng(3)
    lo, hi = ix["lo"], ix["hi"]
    q = lo + (hi - lo) * rng.random(lo.shape).astype(np.float32)                            # inside every tile's box
    q = np.clip(q, lo, hi)
    axis = np.arange(len(q)) % 3
    q[np.arange(len(q)), axis] = np.where((np.arange(len(q)) % 2)[:, None], lo, hi)[np.arange(len(q)), axis]      # on one of its faces
    q = np.ascontiguousarray(q, np.float32)
    assert (X.box_distance(q, q, lo, hi) == 0).all()
    _equal(_query(mt, q, (v, f))[0], P.closest_f32(q, v, f))


# ---- ties ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
def test_ties_go_to_the_lowest_original_face(mt, dev, reverse):
    q = P.cube_tie_queries()
    faces = np.ascontiguousarray(P.CUBE_FACES[::-1]) if reverse else P.CUBE_FACES
    ref = P.closest_f32(q, P.CUBE_VERTS, faces)
    pairs = P._pairs(q, P.face_records(P.corners(P.CUBE_VERTS, faces, np.float32)))[0]
    assert ((pairs == ref[3][:, None]).sum(1) >= 2).all()
    got, _ = _query(mt, q, (P.CUBE_VERTS, faces))
    _equal(got, ref)
    assert np.array_equal(got[1], np.argmax(pairs == ref[3][:, None], axis=1))
    # the cube's faces mixed with small faces inside it: the faces of a tie lie in different tiles
    _, pv, pf = P.random_case(8, 3 * TILE, 4)
    verts = np.concatenate([P.CUBE_VERTS, pv * np.float32(0.05) + np.float32(0.4)])
    mixed = np.concatenate([pf + 8, faces])
    mixed = np.ascontiguousarray(mixed[np.random.default_rng(2).permutation(len(mixed))])
    _equal(_query(mt, q, (verts, mixed))[0], P.closest_f32(q, verts, mixed))


@pytest.mark.parametrize("nq,F", [(65, 257), (100, 2000)])
def test_a_doubled_mesh_answers_from_its_first_half(mt, dev, nq, F):
    q, v, f, ref = _case(nq, F)
    got, _ = _query(mt, q, (np.concatenate([v, v]), np.concatenate([f, f + len(v)])))
    assert (got[1] < F).all()
    _equal(got, ref)


def test_degenerate_faces_among_valid_ones(mt, dev):
    q, verts, faces, _ = P.degenerate_mesh()
    _equal(_query(mt, q, (verts, faces))[0], P.closest_f32(q, verts, faces))


# ---- determinism and translation ----------------------------------------------------------------------------------------------
def test_two_calls_are_bit_identical_and_an_index_is_reusable(mt, dev):
    q, v, f, ref = _case(2049, 1000)
    ix = mt.MeshIndex((v, f))
    a = ix.query(q, closest=True)
    b = ix.query(q, closest=True)
    c = mt.MeshIndex((v, f)).query(q, closest=True)
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a, b, c))
    d = mt.point_mesh_distance(q, None, closest=True, index=ix)                              # a MeshIndex is used as given
    assert all(torch.equal(x, y) for x, y in zip(a, d))
    q2, _, _, _ = _case(63, 65)
    _equal(tuple(t.cpu().numpy() for t in ix.query(q2, closest=True)), P.closest_f32(q2, v, f))


def test_translation_changes_no_bit(mt, dev):
    q, v = P.grid_scene()
    a, _ = _query(mt, q, (v, None))
    b, _ = _query(mt, q + P.GRID_SHIFT, (v + P.GRID_SHIFT, None))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    _equal(a, P.closest_f32(q, v))
    assert (a[0] == 0).sum() >= 100 and (a[0] > 0).sum() >= 100


# ---- the margin ---------------------------------------------------------------------------------------------------------------
def test_near_planar_sheets_are_bit_equal_to_closest_f32(mt, dev):
    """each sheet fills two whole tiles; the groups of low queries skip tiles, so the skip rule and its margin decide here"""
    q, v, f, sheet = X.near_planar_scene()
    ix = X.build(v, f)
    per_tile = [np.unique(sheet[ix["orig"][t * TILE:(t + 1) * TILE]]) for t in range(ix["T"])]
    assert len(f) == 4 * TILE and [len(u) for u in per_tile] == [1, 1, 1, 1] and sorted(int(u[0]) for u in per_tile) == [0, 0, 1, 1]
    assert np.abs(v[:, 2]).max() <= 1e-6 and 1e-3 <= q[:, 2].min() and q[:, 2].max() <= 1.0
    got, stats = _query(mt, q, (v, f))
    _equal(got, P.closest_f32(q, v, f))
    assert stats["tiles_visited"] == int(X.search(q, v, f)[4].sum())
    assert stats["tiles_visited"] < stats["groups"] * stats["tiles"]


def test_a_sphere_that_culls_is_bit_equal_to_closest_f32(mt, dev):
    """queries at 1.02 r of a small UV sphere: most tiles are skipped, and the result is still the restatement's"""
    q, v, f = X.sphere_scene()
    got, stats = _query(mt, q, (v, f))
    _equal(got, P.closest_f32(q, v, f))
    assert stats["tiles_visited"] == int(X.search(q, v, f)[4].sum())
    assert stats["tiles_visited"] < stats["groups"] * stats["tiles"]
    print("sphere: %d of %d tile evaluations" % (stats["tiles_visited"], stats["groups"] * stats["tiles"]))


# ---- results against the brute force ------------------------------------------------------------------------------------------
def _against_the_brute_force(mt, dev, q, v, f, what):
    qd, vd, fd = (torch.from_numpy(x).to(dev) for x in (q, v, f))
    brute = mt.point_mesh_distance(qd, (vd, fd), closest=True, check=False)
    *got, stats = mt.MeshIndex((vd, fd), check=False).query(qd, closest=True, stats=True)
    assert all(torch.equal(x, y) for x, y in zip(got, brute))
    print("%s: %d of %d tile evaluations (%.2f %%)" % (what, stats["tiles_visited"], stats["groups"] * stats["tiles"],
                                                      100.0 * stats["tiles_visited"] / (stats["groups"] * stats["tiles"])))
    return stats


def test_large_case_equals_the_brute_force(mt, dev):
    q, v, f = P.random_case(*P.LARGE_CASE)
    _against_the_brute_force(mt, dev, q, v, f, "large case")


def test_sphere_equals_the_brute_force_near_its_surface_and_at_its_centre(mt, dev):
    v, f = X.uv_sphere(64, 125)                                             # 15 750 faces
    assert 15000 <= len(f) <= 17000
    rng = np.random.default_rng(6)
    d = rng.normal(size=(8192, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    centre = np.array([0.3, -0.2, 0.5])
    _against_the_brute_force(mt, dev, (centre + 1.02 * d).astype(np.float32), v, f, "sphere, queries at 1.02 r")
    _against_the_brute_force(mt, dev, (centre + 1e-3 * rng.random((8192, 1)) * d).astype(np.float32), v, f, "sphere, queries at its centre")


# ---- culling happens ----------------------------------------------------------------------------------------------------------
def test_a_far_cluster_is_never_evaluated(mt, dev):
    """The queries lie inside the first cluster's box, so after any tile of that cluster a group's largest minimum is at most
    the box's diagonal (under 10 m), while every tile of the second cluster is more than 90 m away on every axis."""
    q, v, f = X.two_clusters()
    assert len(q) == 600 and len(f) == 2 * 512
    got, stats = _query(mt, q, (v, f))
    _equal(got, P.closest_f32(q, v, f))
    assert (got[1] < 512).all()
    assert stats["tiles"] == 2 * 512 // stats["tile_faces"]
    assert stats["tiles_visited"] <= stats["groups"] * 512 // stats["tile_faces"]


# ---- opt-in equality ----------------------------------------------------------------------------------------------------------
def test_calc_3d_metric_surface_with_the_index_is_the_default_result(mt, dev):
    from test_pointmesh_gpu import DELTA, _cube_mesh, _cube_pose
    R, t = _cube_pose()
    rec, gt = _cube_mesh(1.0, R, t), _cube_mesh(1 + 2 * DELTA, R, t)
    plain = mt.calc_3d_metric_surface(rec, gt, N=20000, seed=1)
    assert mt.calc_3d_metric_surface(rec, gt, N=20000, seed=1, index=True) == plain
    assert mt.calc_3d_metric_surface(rec, gt, N=20000, seed=1, index=False) == plain


def test_deviation_with_the_index_is_the_default_result(mt, dev):
    from cnr_amd import meshops
    from test_pointmesh_gpu import _sheet
    v, f = (torch.from_numpy(x).to(dev) for x in _sheet(40))
    ov, of, _, _ = meshops.simplify(v, f, cell=0.08)
    plain = meshops.deviation(v, f, ov, of, samples=3000, seed=2)
    assert meshops.deviation(v, f, ov, of, samples=3000, seed=2, index=True) == plain and plain["hausdorff"] > 0


def _tool(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return __import__(name)
    finally:
        sys.path.pop(0)


def test_simplify_mesh_tool_prints_the_same_deviation_with_the_index(dev, tmp_path, capsys):
    from cnr_amd import vis
    from test_pointmesh_gpu import _sheet
    v, f = _sheet(24)
    src = str(tmp_path / "in.obj")
    vis.Mesh(v, f, np.zeros_like(v)).export(src)
    tool = _tool("simplify_mesh")
    capsys.readouterr()
    tool.main([src, str(tmp_path / "a.obj"), "--cell", "0.1", "--deviation", "3000"])
    plain = capsys.readouterr().out
    tool.main([src, str(tmp_path / "b.obj"), "--cell", "0.1", "--deviation", "3000", "--index"])
    assert capsys.readouterr().out == plain and "deviation" in plain and "hausdorff" in plain
    assert open(tmp_path / "a.obj").read() == open(tmp_path / "b.obj").read()


def test_eval_3d_obj_tool_writes_the_same_table_with_the_index(dev, tmp_path, capsys):
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
    tool = _tool("eval_3d_obj")
    table = logs / "room_0" / "eval_mesh" / "metrics_3D_obj_surface.json"
    capsys.readouterr()
    tool.main(["--data_dir", str(data), "--log_dir", str(logs), "--surface"])
    plain_out, plain = capsys.readouterr().out, table.read_text()
    table.unlink()
    tool.main(["--data_dir", str(data), "--log_dir", str(logs), "--surface", "--index"])
    assert capsys.readouterr().out == plain_out and table.read_text() == plain
    assert json.loads(plain)["objects"]["1"]["fscore"] == 1.0


def test_time_pointmesh_tool_times_the_index_beside_the_brute_force(dev, tmp_path):
    out = tmp_path / "time.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "time_pointmesh.py"), "--index", "--queries", "2000", "--reps", "1",
                        "--out", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = json.loads(out.read_text())["rows"]
    assert {"mc256", "mc256_clipped", "nn_dist", "numpy_restatement_cpu"} <= set(rows)      # the tool's own rows are still there
    for name in ("index_mc256", "index_mc256_clipped", "index_mc256_centre"):
        row = rows[name]
        assert row["equal"] is True and row["queries"] == 2000 and row["tiles"] == -(-row["faces"] // TILE)
        for leg in ("brute_ms", "build_keys_ms", "build_sort_ms", "build_records_tiles_ms", "query_keys_ms", "query_sort_ms",
                    "query_kernel_ms", "query_ms"):
            assert len(row[leg]) == 3 and row[leg][1] <= row[leg][0] <= row[leg][2]
        assert row["pairs_evaluated"] == row["tiles_visited"] * TILE * GROUP and row["pairs_brute"] == 2000 * row["faces"]
        print(name, "visited share", row["visited_share"])
