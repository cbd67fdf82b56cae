"""GPU: cnr_winding_number (csrc/winding.hip) within the derived bar of the numpy restatement (tests/winding_cpu.py) at the tile
and query-block edges, indexed and soup; a large case against torch float64; closed forms, linearity, determinism,
translation, degenerate faces; and the public functions built on it: metrics.inside, signed_distance, volume_iou, the two tools.

The bar of a query (winding_cpu.bar) always comes from the restatement, or in the large case from the torch
evaluation: 2^-52 [(F + 16) sum |t| + 16 sum la lb lc / hypot(det, den)] / 2 pi."""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pointmesh_cpu as P
import winding_cpu as W
from conftest import ROOT

pytestmark = pytest.mark.gpu

CUBE_CENTRED = W.CUBE_VERTS.astype(np.float64) - 0.5
MERGE_CASE = (3, 1000)                                                # one query block, four tiles: four chunks


@pytest.fixture(scope="module")
def mt():
    from cnr_amd import metrics
    return metrics


@functools.lru_cache(maxsize=None)
def _case(nq, F):
    """the scene and the restatement with its bar, computed once and shared"""
    q, v, f = W.random_case(nq, F)
    w, bar = W.winding_f64(q, v, f, with_bar=True)
    for arr in (q, v, f, w, bar):
        arr.setflags(write=False)
    return q, v, f, w, bar


@functools.lru_cache(maxsize=None)
def _spheres():
    """(name, verts, faces, outward?) of the closed and the open sphere, each outward and flipped, and per mesh the restated
    winding number of inside_queries()"""
    v, f = W.uv_sphere()
    vo, fo = W.open_sphere()
    q = W.inside_queries()
    out = []
    for name, verts, faces, outward in (("closed", v, f, True), ("closed flipped", v, W.flipped(f), False),
                                        ("open", vo, fo, True), ("open flipped", vo, W.flipped(fo), False)):
        w = W.winding_f64(q, verts, faces)
        w.setflags(write=False)
        out.append((name, verts, faces, outward, w))
    return q, out


def _chunks(nq, F):
    import cnr_amd
    return W.workspace_chunks(nq, F, cnr_amd._C.load().cnr_winding_workspace_bytes(nq, F))


def _w(mt, q, mesh, **kw):
    w = mt.winding_number(q, mesh, **kw)
    assert w.dtype == torch.float64 and w.is_cuda and w.shape == (len(q),)
    return w.cpu().numpy()


# ---- the bar ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,F", W.BIT_CASES + (MERGE_CASE,))
def test_within_the_bar_of_the_restatement_indexed_and_soup(mt, dev, nq, F):
    q, v, f, want, bar = _case(nq, F)
    if (nq, F) == MERGE_CASE:
        assert _chunks(nq, F) >= 3 and nq * F < 4e6                     # the finish pass merges at least three chunks
    assert _chunks(nq, F) == W.chunk_count(nq, F)
    got = mt.winding_number(q, (v, f))
    soup = mt.winding_number(q, (P.soup(v, f), None))
    assert torch.equal(got, soup)                                       # same faces, same order, same operations
    err = np.abs(got.cpu().numpy() - want)
    print("(%d, %d): max error %.3g, %.4f of the bar" % (nq, F, err.max(), (err / bar).max()))
    assert got.dtype == torch.float64 and len(err) == nq and (err <= bar).all(), float((err / bar).max())


def _time_winding():
    """tools/time_winding.py as a module: its torch float64 evaluation is the independent one used here"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import time_winding
    finally:
        sys.path.pop(0)
    return time_winding


def test_large_case_against_torch_float64(mt, dev):
    nq, F = 4096, 50000
    q, v, f = W.random_case(nq, F)
    tq, tv, tf = torch.from_numpy(q).to(dev), torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    got = mt.winding_number(tq, (tv, tf))
    want, bar = _time_winding().torch_winding(tq, tv.double()[tf.long()], 64, with_bar=True)      # query chunks of 64
    ratio = (got - want).abs() / bar
    print("max error %.3g, %.4f of the bar, chunks %d" % (float((got - want).abs().max()), float(ratio.max()), _chunks(nq, F)))
    assert _chunks(nq, F) > 1 and bool((bar > 0).all()) and bool((ratio <= 1).all()), float(ratio.max())


# ---- closed forms, linearity -----------------------------------------------------------------------------------------------
def test_closed_forms_on_the_unit_cube(mt, dev):
    q = np.concatenate([W.cube_tie_queries(), np.full((1, 3), 0.5, np.float32)])
    want = np.concatenate([W.cube_expected(), [1.0]])
    w = _w(mt, q, (W.CUBE_VERTS, W.CUBE_FACES))
    assert (np.abs(w - want) <= 1e-12).all(), float(np.abs(w - want).max())
    flipped = _w(mt, q, (W.CUBE_VERTS, W.flipped(W.CUBE_FACES)))
    assert (np.abs(flipped + want) <= 1e-12).all()
    tri = np.array([[0, 0, 0.5], [4, 0, 0.5], [0, 4, 0.5]], np.float32)
    flat = _w(mt, np.array([[1, 1, 0.5], [5, 5, 0.5], [2, 2, 0.5], [0, 0, 0.5]], np.float32), (tri, None))
    assert np.array_equal(flat, np.zeros(4))                            # det == 0: exactly nothing, inside the triangle too


def test_linearity_in_the_mesh(mt, dev):
    q, v, f, want, bar = _case(65, 257)
    twice = _w(mt, q, (v, np.concatenate([f, f])))
    assert (np.abs(twice - 2 * want) <= 2 * bar).all()
    none = _w(mt, q, (v, np.concatenate([f, W.flipped(f)])))
    assert (np.abs(none) <= 2 * bar).all() and (np.abs(want) > 2 * bar).sum() > 40


# ---- determinism and translation ---------------------------------------------------------------------------------------------
def test_two_calls_are_equal_and_an_exact_translation_changes_no_bit(mt, dev):
    q, v, f, _, _ = _case(2049, 1000)
    assert torch.equal(mt.winding_number(q, (v, f)), mt.winding_number(q, (v, f)))
    gq, gv = W.grid_scene()
    a = mt.winding_number(gq, (gv, None))
    b = mt.winding_number(gq + W.GRID_SHIFT, (gv + W.GRID_SHIFT, None))
    assert torch.equal(a, b) and int((a != 0).sum()) > 100
    want, bar = W.winding_f64(gq, gv, with_bar=True)
    assert (np.abs(a.cpu().numpy() - want) <= bar).all()


def test_degenerate_faces_within_the_bar(mt, dev):
    q, v, f, is_deg = W.degenerate_mesh()
    want, bar = W.winding_f64(q, v, f, with_bar=True)
    got = _w(mt, q, (v, f))
    assert is_deg.sum() == 12 and np.isfinite(got).all() and (np.abs(got - want) <= bar).all()


# ---- inside, signed distance ---------------------------------------------------------------------------------------------------
def test_inside_flags_equal_the_restatement(mt, dev):
    q, meshes = _spheres()
    for name, verts, faces, outward, w in meshes:
        s = 1 if outward else -1
        margin = np.abs(s * w - 0.5).min()
        assert margin >= 1e-6, (name, margin)                           # over ALL queries: none is excluded below
        want = s * w > 0.5
        assert 300 < want.sum() < 2000
        assert mt.mesh_orientation((verts, faces)) == s
        for orientation in ("auto", "outward" if outward else "inward"):
            got = mt.inside(q, (verts, faces), orientation=orientation)
            assert got.dtype == torch.bool and got.is_cuda and np.array_equal(got.cpu().numpy(), want), (name, orientation)
        wrong = mt.inside(q, (verts, faces), orientation="inward" if outward else "outward")
        assert not bool(wrong.any())                                    # -w > 0.5 nowhere
    with pytest.raises(ValueError):
        mt.inside(q, (verts, faces), orientation="sideways")


def test_signed_distance_is_the_distance_with_the_restated_sign(mt, dev):
    q, meshes = _spheres()
    for name, verts, faces, outward, w in meshes[1:3]:                  # the flipped closed sphere and the open one
        flag = (w if outward else -w) > 0.5
        d32, f32, c32, _ = P.closest_f32(q, verts, faces)
        sd, face, near = (t.cpu().numpy() for t in mt.signed_distance(q, (verts, faces), closest=True))
        assert sd.dtype == np.float32 and np.array_equal(np.abs(sd), d32)
        assert np.array_equal(sd < 0, flag & (d32 > 0)) and (d32 > 0).all()
        d, fc, nr = mt.point_mesh_distance(q, (verts, faces), closest=True)
        assert np.array_equal(face, fc.cpu().numpy()) and np.array_equal(near, nr.cpu().numpy())
        assert np.array_equal(face, f32) and np.array_equal(near, c32)
        two = mt.signed_distance(q, (verts, faces))
        assert len(two) == 2 and np.array_equal(two[0].cpu().numpy(), sd)
        for index in (True, mt.MeshIndex((verts, faces))):
            si, fi, ni = (t.cpu().numpy() for t in mt.signed_distance(q, (verts, faces), closest=True, index=index))
            assert np.array_equal(si, sd) and np.array_equal(fi, face) and np.array_equal(ni, near)
        explicit = mt.signed_distance(q, (verts, faces), orientation="outward" if outward else "inward")[0]
        assert np.array_equal(explicit.cpu().numpy(), sd)


# ---- volume IoU --------------------------------------------------------------------------------------------------------------
def test_volume_iou_counts_are_the_analytic_ones(mt, dev):
    delta = 2.0 ** -5
    (va, fa), (vb, fb) = W.concentric_cubes(delta)
    p = W.iou_points()
    x = p.astype(np.float64)
    in_a = ((x > 0) & (x < 1)).all(1)
    in_b = ((x > -delta) & (x < 1 + delta)).all(1)
    r = mt.volume_iou((va, fa), (vb, fb), points=p)
    assert set(r) == {"iou", "intersection", "union", "inside_a", "inside_b", "n", "volume_a", "volume_b", "orientation_a",
                      "orientation_b"}
    assert (r["orientation_a"], r["orientation_b"]) == (1, -1) and r["n"] == 20000
    assert (r["inside_a"], r["inside_b"]) == (int(in_a.sum()), int(in_b.sum()))
    assert (r["intersection"], r["union"]) == (int((in_a & in_b).sum()), int((in_a | in_b).sum()))
    assert all(isinstance(r[k], int) for k in ("intersection", "union", "inside_a", "inside_b", "n"))
    closed = 1.0 / (1 + 2 * delta) ** 3
    sigma = math.sqrt(closed * (1 - closed) / r["union"])
    assert r["iou"] == r["intersection"] / r["union"] and abs(r["iou"] - closed) <= 4 * sigma
    wrong = mt.volume_iou((va, fa), (vb, fb), points=p, orientation=("auto", "outward"))
    assert wrong["inside_b"] == 0 and wrong["iou"] == 0.0 and wrong["union"] == r["inside_a"]
    empty = mt.volume_iou((va, fa), (vb, fb), points=p + np.float32(4.0))
    assert empty["union"] == 0 and math.isnan(empty["iou"])


def test_volume_iou_seeded_draw_equals_the_restatement(mt, dev):
    delta = 2.0 ** -5
    (va, fa), (vb, fb) = W.concentric_cubes(delta)
    N, seed = 6000, 3
    r = mt.volume_iou((va, fa), (vb, fb), N=N, seed=seed)
    p = W.box_draw(np.full(3, -delta), np.full(3, 1 + delta), N, seed)          # the box of both meshes' vertices
    wa, wb = W.winding_f64(p, va, fa), -W.winding_f64(p, vb, fb)
    assert min(np.abs(wa - 0.5).min(), np.abs(wb - 0.5).min()) >= 1e-6
    in_a, in_b = wa > 0.5, wb > 0.5
    assert (r["inside_a"], r["inside_b"], r["n"]) == (int(in_a.sum()), int(in_b.sum()), N)
    assert (r["intersection"], r["union"]) == (int((in_a & in_b).sum()), int((in_a | in_b).sum()))
    box = (1 + 2 * delta) ** 3
    assert abs(r["volume_a"] - in_a.sum() / N * box) <= 1e-12 and abs(r["volume_b"] - in_b.sum() / N * box) <= 1e-12
    assert abs(r["volume_a"] - 1.0) < 0.03 and r["inside_b"] > 0.99 * N
    # an oriented box as oriented_bounds returns it: the unit cube's own box, so everything drawn is inside the larger cube
    T = np.eye(4)
    T[:3, 3] = -0.5
    ob = mt.volume_iou((va, fa), (vb, fb), N=N, seed=seed, box=(T, np.ones(3)))
    assert ob["inside_b"] == N and ob["inside_a"] >= N - 5 and abs(ob["volume_b"] - 1.0) <= 1e-12
    # a rotated, shifted, unequal box: a cuboid that fills box_planes' box exactly holds every drawn point (a transposed or
    # non-inverted transform would put most of them outside), and a cuboid of the same size left at the origin far fewer
    T, ext = W.rotated_box()
    Ti = np.linalg.inv(T)
    local = (CUBE_CENTRED * ext).astype(np.float64)
    fill = (local @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    rb = mt.volume_iou((fill, W.CUBE_FACES), (local.astype(np.float32), W.CUBE_FACES), N=N, seed=seed, box=(T, ext))
    assert rb["inside_a"] >= N - 5 and abs(rb["volume_a"] - float(np.prod(ext))) <= 5 / N * float(np.prod(ext)) + 1e-12
    assert rb["inside_b"] < 0.5 * N


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_non_finite_inputs_and_empty_meshes_raise(mt, dev):
    q = W.cube_tie_queries()
    mesh = (W.CUBE_VERTS, W.CUBE_FACES)
    none = (W.CUBE_VERTS, np.zeros((0, 3), np.int32))
    for bad in (np.nan, np.inf):
        qb, vb = q.copy(), W.CUBE_VERTS.copy()
        qb[3, 1] = bad
        vb[5, 2] = bad
        for fn in (mt.winding_number, mt.inside, mt.signed_distance):
            with pytest.raises(ValueError):
                fn(qb, mesh)
            with pytest.raises(ValueError):
                fn(q, (vb, W.CUBE_FACES))
        with pytest.raises(ValueError):
            mt.volume_iou(mesh, (vb, W.CUBE_FACES), N=10)
        with pytest.raises(ValueError):
            mt.volume_iou(mesh, mesh, points=qb)
    for fn in (mt.winding_number, mt.inside, mt.signed_distance, mt.mesh_orientation):
        with pytest.raises(ValueError):
            fn(*((q, none) if fn is not mt.mesh_orientation else (none,)))
    with pytest.raises(ValueError):
        mt.volume_iou(mesh, none, N=10)
    with pytest.raises(ValueError):
        mt.winding_number(q, (W.CUBE_VERTS, W.CUBE_FACES + 1))          # an index outside the vertices


# ---- the tools ---------------------------------------------------------------------------------------------------------------
def test_eval_3d_obj_tool_iou_flag_adds_its_column_only_when_asked(dev, tmp_path, capsys):
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
    r = subprocess.run([sys.executable, tool, "--data_dir", str(data), "--log_dir", str(logs), "--volume", "5000"],
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    out = logs / "room_0" / "eval_mesh"
    with_flag = np.load(out / "metrics_3D_obj.npy")
    table = json.loads((out / "metrics_3D_obj_volume.json").read_text())
    row = table["objects"]["1"]
    assert table["points"] == 5000 == row["n"] and table["mean"]["iou"] == row["iou"]
    # (_cube's opposite sides are wound the same way, so these boxes are NOT consistently oriented and the value itself means
    # nothing here; test_volume_iou_* check values on oriented meshes.  The counts still have to be counts.)
    assert row["union"] == row["inside_a"] + row["inside_b"] - row["intersection"] and 0 < row["union"] <= 5000
    assert row["iou"] == row["intersection"] / row["union"] and abs(row["volume_b"] - row["inside_b"] / 5000 * 0.06) < 1e-9
    (out / "metrics_3D_obj_volume.json").unlink()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import eval_3d_obj
    finally:
        sys.path.pop(0)
    capsys.readouterr()
    eval_3d_obj.main(["--data_dir", str(data), "--log_dir", str(logs)])
    plain = capsys.readouterr().out
    assert "volume" not in plain and not (out / "metrics_3D_obj_volume.json").exists()
    np.testing.assert_array_equal(np.load(out / "metrics_3D_obj.npy"), with_flag)
    extra = [ln for ln in r.stdout.splitlines() if ln.startswith("volume ")]
    assert [ln for ln in r.stdout.splitlines() if ln not in extra] == plain.splitlines()
    assert len(extra) == 2 and extra[0].startswith("volume obj 1: iou ") and extra[1].startswith("volume mean: iou ")


def test_time_winding_tool_writes_its_rows(dev, tmp_path):
    out = tmp_path / "winding_time.json"
    tool = os.path.join(ROOT, "tools", "time_winding.py")
    r = subprocess.run([sys.executable, tool, "--queries", "2000", "--faces", "3000", "--reps", "2", "--out", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    table = json.loads(out.read_text())
    row = table["rows"]["random"]
    assert table["reps"] == 2 and (row["faces"], row["queries"], row["pairs"]) == (3000, 2000, 6000000)
    for key in ("winding_ms", "point_mesh_ms", "torch_ms"):
        assert len(row[key]) == 3 and row[key][1] <= row[key][0] <= row[key][2] and row[key][1] > 0
    for key in ("winding_pairs_per_s", "point_mesh_pairs_per_s", "torch_pairs_per_s", "winding_over_point_mesh",
                "kernel_over_torch_per_pair"):
        assert row[key] > 0
    assert row["max_abs_difference_to_torch"] < 1e-9
