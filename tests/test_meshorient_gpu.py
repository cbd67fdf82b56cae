"""GPU: orientation repair (csrc/mesh_topo.hip cnr_mesh_orient_*, cnr_amd.meshops.orient) against the
numpy restatement tests/meshorient_cpu.py, whose hand cases and fixtures' conditions tests/test_meshorient_host.py proves
without a GPU.  Every integer and boolean output is EQUAL to the restatement and signed_volume is bit-equal to it (the same
order of operations); the device err word is 0 (a set word raises)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cnr_amd
import mc_cpu as M
import meshops_cpu as R
import meshorient_cpu as OC
from conftest import ROOT

MO = cnr_amd.meshops
pytestmark = pytest.mark.gpu
FIELDS = ("faces", "flip", "face_patch", "first", "n_faces", "orientable", "closed", "inconsistent_edges", "n_flipped")
CHAIN = 100001


def _t(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)                           # a copy: the cached fixtures are read-only


def gpu_orient(v, f, dev, outward=None, with_verts=True):
    return MO.orient(_t(f, dev), len(v), _t(v, dev) if with_verts else None, outward=outward)


def assert_equal(got, ref):
    assert got.n == ref["n"]
    for k in FIELDS:
        assert np.array_equal(getattr(got, k).cpu().numpy(), ref[k]), k
    if ref["signed_volume"] is None:
        assert got.signed_volume is None
        return
    vol = got.signed_volume.cpu().numpy()
    if got.n:
        print("signed_volume: largest difference to the restatement %.3g, in bounds %.3g" % (
            np.abs(vol - ref["signed_volume"]).max(), (np.abs(vol - ref["signed_volume"]) * 6 / np.maximum(ref["s_bound"], 1e-300)).max()))
    assert np.array_equal(vol, ref["signed_volume"])                                  # bit-equal: the same order of operations


def same_direction_edges(faces, n_vertices, dev):
    """the existing components' count of interior edges both of whose faces run them the same way"""
    return int(MO.components(faces if torch.is_tensor(faces) else _t(faces, dev), n_vertices).edge_counts[:, 2].sum())


def hand_oriented(v, f, centre):
    """every face turned so that its normal points away from `centre` (convex meshes), by plain geometry"""
    p = np.asarray(v, np.float64)[f]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    return OC.flip_faces(f, (n * (p.mean(1) - centre)).sum(1) < 0)


@functools.lru_cache(maxsize=None)
def two_spheres():
    v, _, f = M.marching_cubes(M.two_spheres(64))
    comp = R.components(f, len(v))["face_component"]
    for a in (v, f, comp):
        a.setflags(write=False)
    return v, f, comp


@functools.lru_cache(maxsize=None)
def metric_cube(lo, hi):
    """test_metrics_gpu._cube -- opposite sides wound the same way -- triangulated and welded: (verts f32, faces, hand-oriented faces)"""
    from test_metrics_gpu import _cube
    cv, cq = _cube(list(lo), list(hi), 4)
    tri = np.concatenate([cq[:, [0, 1, 2]], cq[:, [0, 2, 3]]]).astype(np.int32)
    kept, f, _ = R.weld(cv.astype(np.float32), tri)
    v = cv.astype(np.float32)[kept]
    return v, f, hand_oriented(v, f, 0.5 * (np.asarray(lo) + np.asarray(hi)))


# ---- no link at all ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [0, 1, 63, 64, 65, 257])
def test_disjoint_triangles(dev, F):
    v, f = R.disjoint_triangles(F)
    f = f.copy()
    if F >= 63:
        f[5] = [f[5, 0], f[5, 1], f[5, 0]]                   # (a, b, a)
        f[40] = f[40, 0]                                     # (a, a, a)
        f[41] = [f[40, 0], f[41, 1], f[41, 2]]               # shares a vertex, not an edge
    ref = OC.orient(f, len(v), v)
    got = gpu_orient(v, f, dev)
    assert_equal(got, ref)
    assert got.n == F and np.array_equal(got.face_patch.cpu().numpy(), np.arange(F)) and not got.inconsistent_edges.any()
    if F >= 63:
        flip, vol = got.flip.cpu().numpy(), got.signed_volume.cpu().numpy()
        assert flip[5] == 0 and flip[40] == 0 and vol[5] == 0 and vol[40] == 0 and got.closed[5] and got.closed[40]
        assert np.array_equal(got.faces.cpu().numpy()[[5, 40]], f[[5, 40]])
        assert 0 < flip.sum() < F and (vol >= 0).all()       # random triangles: some had to turn
    plain = gpu_orient(v, f, dev, with_verts=False)
    assert_equal(plain, OC.orient(f, len(v)))
    assert not plain.flip.any() and plain.signed_volume is None


# ---- one long parity chain -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def strip(F, order):
    """the first F faces of a ladder, a random half flipped, in the given order -> (verts, faces, restatement)"""
    v, f = R.ladder(F // 2 + 2, "ascending")
    f, _ = OC.random_flips(f[:F], F)
    if order == "descending":
        f = f[::-1]
    elif order == "shuffled":
        f = f[np.random.default_rng(F).permutation(F)]
    f = np.ascontiguousarray(f)
    return v, f, OC.orient(f, len(v), v)


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
@pytest.mark.parametrize("F", [2, 63, 64, 65, 1025, CHAIN])
def test_ladder_strip_with_random_flips(dev, F, order):
    v, f, ref = strip(F, order)
    assert len(f) == F and ref["n"] == 1
    got = gpu_orient(v, f, dev)
    assert_equal(got, ref)
    assert got.n == 1 and bool(got.orientable[0]) and not bool(got.closed[0])
    assert same_direction_edges(got.faces, len(v), dev) == 0
    assert int(got.inconsistent_edges[0]) == same_direction_edges(f, len(v), dev)
    assert int(got.flip[0]) == 0                             # the smallest face stays: the strip is planar, s = 0
    if F >= 63:
        assert 0 < int(got.n_flipped[0]) < F


# ---- undo ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_flips_are_undone(dev, seed):
    v, f = R.icosphere(2)
    assert np.array_equal(hand_oriented(v, f, 0.0), f)       # outward as it stands
    g, mask = OC.random_flips(f, seed)
    got = gpu_orient(v, g, dev)
    assert_equal(got, OC.orient(g, len(v), v))
    assert np.array_equal(got.faces.cpu().numpy(), f) and np.array_equal(got.flip.cpu().numpy().astype(bool), mask)
    assert bool(got.closed[0]) and float(got.signed_volume[0]) > 3.9            # a little under 4 pi / 3
    for kw in (dict(outward=False), dict(with_verts=False)):
        rel = gpu_orient(v, g, dev, **kw)
        want = OC.flip_faces(f, np.ones(len(f), bool)) if mask[0] else f       # face 0 stays as it came
        assert np.array_equal(rel.faces.cpu().numpy(), want)
    mirrored = gpu_orient(v, g, dev, outward=False)
    assert_equal(mirrored, OC.orient(g, len(v), v, outward=False))
    assert (float(mirrored.signed_volume[0]) < 0) == bool(mask[0])
    # flipping twice is the identity
    again = MO.orient(got.faces, len(v), _t(v, dev))
    assert not again.flip.any() and torch.equal(again.faces, got.faces)


# ---- the cube of the metrics tests ---------------------------------------------------------------------------------------------
def test_inconsistent_cube_is_repaired_for_the_inside_tests(dev):
    from cnr_amd import metrics
    lo, hi = (0.0, 0.0, 0.0), (0.5, 0.25, 1.0)
    v, f, hand = metric_cube(lo, hi)
    assert same_direction_edges(f, len(v), dev) > 0 and same_direction_edges(hand, len(v), dev) == 0
    ref = OC.orient(f, len(v), v)
    got = gpu_orient(v, f, dev)
    assert_equal(got, ref)
    assert got.n == 1 and bool(got.closed[0]) and bool(got.orientable[0]) and same_direction_edges(got.faces, len(v), dev) == 0
    assert abs(float(got.signed_volume[0]) - 0.125) <= ref["s_bound"][0] / 6
    assert np.array_equal(got.faces.cpu().numpy(), hand)
    q = (np.random.default_rng(3).random((4000, 3)) * 1.4 - 0.2).astype(np.float32)
    want = metrics.inside(_t(q, dev), (v, hand), orientation="outward")
    assert torch.equal(metrics.inside(_t(q, dev), (v, f), orientation="repair"), want) and 0 < int(want.sum()) < len(q)
    assert not torch.equal(metrics.inside(_t(q, dev), (v, f)), want)                   # ... which the mesh as it came does not give
    sd = metrics.signed_distance(_t(q, dev), (v, f), orientation="repair")[0]
    assert torch.equal(sd, metrics.signed_distance(_t(q, dev), (v, hand), orientation="outward")[0])
    v2, f2, hand2 = metric_cube((0.25, 0.0, 0.25), (0.75, 0.5, 0.75))
    a = metrics.volume_iou((v, f), (v2, f2), N=5000, orientation=("repair", "repair"))
    b = metrics.volume_iou((v, hand), (v2, hand2), N=5000, orientation=("outward", "outward"))
    assert a == b and a["orientation_a"] == a["orientation_b"] == 1 and 0 < a["intersection"] < a["union"]
    mixed = metrics.volume_iou((v, f), (v2, hand2), N=5000, orientation=("repair", "auto"))
    assert mixed == b
    with pytest.raises(ValueError):
        metrics.inside(_t(q, dev), (v, f), orientation="sideways")


# ---- a band that cannot be oriented beside a strip that can ---------------------------------------------------------------------
def test_moebius_band_beside_a_flipped_strip(dev):
    vb, fb = OC.moebius(5)
    vs, fs = OC.quad_strip(7, False, v0=len(vb))
    g, mask = OC.random_flips(fs, 4)
    assert mask.any() and not mask.all()
    v, f = np.concatenate([vb, vs + np.float32([3, 0, 0])]), np.concatenate([fb, g])
    ref = OC.orient(f, len(v), v)
    got = gpu_orient(v, f, dev)
    assert_equal(got, ref)
    assert got.n == 2 and got.orientable.tolist() == [False, True] and got.n_flipped[0] == 0
    out = got.faces.cpu().numpy()
    assert np.array_equal(out[:len(fb)], fb) and same_direction_edges(out[len(fb):], len(v), dev) == 0
    assert same_direction_edges(out[:len(fb)], len(v), dev) == 1
    other = gpu_orient(v, np.concatenate([g, fb]), dev)                               # the band last: still found out, still untouched
    assert other.orientable.tolist() == [True, False] and np.array_equal(other.faces.cpu().numpy()[len(g):], fb)


# ---- non-manifold edges join nothing -----------------------------------------------------------------------------------------
def test_book_and_cubes_on_an_edge(dev):
    v, f = OC.book()
    got = gpu_orient(v, f, dev)
    assert_equal(got, OC.orient(f, len(v), v))
    assert got.n == 3 and not got.flip.any() and MO.components(_t(f, dev), len(v)).n == 1
    v, f = OC.cubes_on_an_edge()
    for seed in range(3):
        g, _ = OC.random_flips(f, seed)
        got = gpu_orient(v, g, dev)
        assert_equal(got, OC.orient(g, len(v), v))
        assert got.n == 2 and got.n_faces.tolist() == [12, 12] and not got.closed.any() and got.signed_volume.tolist() == [1.0, 1.0]
        assert np.array_equal(got.faces.cpu().numpy(), f)                              # both cubes outward again


@pytest.mark.parametrize("seed", [0, 1])
def test_random_binary_volume(dev, seed):
    v, _, f = M.marching_cubes(M.random_binary(24, seed))
    g, _ = OC.random_flips(f, seed)
    ref = OC.orient(g, len(v), v)
    got = gpu_orient(v, g, dev)
    assert_equal(got, ref)
    assert got.n >= R.components(f, len(v))["n"] >= 100 and not ref["closed"].all()   # a non-manifold edge cuts sheets apart
    again = MO.orient(got.faces, len(v), _t(v, dev))
    assert not again.flip.any() and not again.inconsistent_edges[again.orientable].any()
    assert torch.equal(again.orientable, got.orientable) and torch.equal(again.signed_volume, got.signed_volume)


# ---- every patch on its own ----------------------------------------------------------------------------------------------------
def test_two_spheres_one_inward(dev):
    v, f, comp = two_spheres()
    outward = OC.flip_faces(f, np.ones(len(f), bool))                                 # marching cubes' faces look inward
    g = OC.flip_faces(f, comp == 0)                                                   # sphere 0 outward, sphere 1 inward
    ref = OC.orient(g, len(v), v)
    got = gpu_orient(v, g, dev)
    assert_equal(got, ref)
    assert got.n == 2 and got.closed.all() and got.orientable.all() and (got.signed_volume > 0.02).all()
    assert np.array_equal(got.faces.cpu().numpy(), outward)
    assert got.n_flipped.tolist() == [0, int((comp == 1).sum())]
    shuffled, _ = OC.random_flips(g, 9)
    assert np.array_equal(gpu_orient(v, shuffled, dev).faces.cpu().numpy(), outward)


# ---- determinism -----------------------------------------------------------------------------------------------------------------
def test_runs_are_identical_and_a_permutation_permutes(dev):
    v, f, _ = two_spheres()
    g, _ = OC.random_flips(f, 5)
    a, b = gpu_orient(v, g, dev), gpu_orient(v, g, dev)
    for k in FIELDS + ("signed_volume",):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    perm = np.random.default_rng(6).permutation(len(g))
    c = gpu_orient(v, g[perm], dev)
    assert np.array_equal(c.flip.cpu().numpy(), a.flip.cpu().numpy()[perm])
    assert np.array_equal(c.faces.cpu().numpy(), a.faces.cpu().numpy()[perm])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_error_paths(dev):
    v, f = R.icosphere(1)
    bad = f.copy()
    bad[7, 1] = len(v)
    with pytest.raises(ValueError):
        gpu_orient(v, bad, dev)
    bad[7, 1] = -1
    with pytest.raises(ValueError):
        gpu_orient(v, bad, dev)
    with pytest.raises(ValueError):
        gpu_orient(v, f, dev, outward=True, with_verts=False)
    with pytest.raises(ValueError):
        MO.orient(_t(f, dev), len(v), _t(v[:-1], dev))
    empty = MO.orient(torch.zeros(0, 3, device=dev, dtype=torch.int32), 5, torch.zeros(5, 3, device=dev))
    assert empty.n == 0 and tuple(empty.faces.shape) == (0, 3) and len(empty.signed_volume) == 0 and empty.table().count("\n") == 0


# ---- the vis.Mesh form, clean_mesh's option and the tools ------------------------------------------------------------------------
def test_orient_mesh_and_clean_mesh_option(dev):
    v, f = R.icosphere(2)
    g, mask = OC.random_flips(f, 7)
    rng = np.random.default_rng(0)
    mesh = cnr_amd.vis.Mesh(v, g, rng.normal(size=v.shape))
    mesh.visual.vertex_colors = rng.integers(0, 256, (len(v), 3))
    out, rep = MO.orient_mesh(mesh)
    assert np.array_equal(out.faces, f) and np.array_equal(out.vertices, mesh.vertices)
    assert np.array_equal(out.vertex_normals, mesh.vertex_normals) and np.array_equal(out.visual.vertex_colors, mesh.visual.vertex_colors)
    assert rep.n == 1 and int(rep.n_flipped[0]) == int(mask.sum()) and len(rep.table().splitlines()) == 2
    cleaned, report = MO.clean_mesh(mesh, orient=True)
    assert np.array_equal(cleaned.faces, f) and report["orientation"].n == 1
    plain, report = MO.clean_mesh(mesh)
    assert np.array_equal(plain.faces, g) and "orientation" not in report
    cleaned, _ = MO.clean_mesh(mesh, **MO.parse_clean_options("keep_largest=1,orient=1"))
    assert np.array_equal(cleaned.faces, f)


def test_clean_mesh_tool_orients_an_obj(dev, tmp_path):
    v, f = R.icosphere(2)
    g, mask = OC.random_flips(f, 8)
    src, dst = str(tmp_path / "in.obj"), str(tmp_path / "out.obj")
    cnr_amd.vis.Mesh(v, g, v.astype(np.float64)).export(src)
    tool = os.path.join(ROOT, "tools", "clean_mesh.py")
    out = subprocess.run([sys.executable, tool, src, dst, "--orient"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "orientable" in out.stdout and "patches: 1  not orientable: 0  faces flipped: %d" % mask.sum() in out.stdout
    back = cnr_amd.vis.load_mesh(dst)
    assert np.array_equal(back.faces, f) and np.abs(back.vertices - cnr_amd.vis.load_mesh(src).vertices).max() <= 1e-8
    out = subprocess.run([sys.executable, tool, src, dst], capture_output=True, text=True)
    assert out.returncode == 0 and "patches" not in out.stdout and np.array_equal(cnr_amd.vis.load_mesh(dst).faces, g)


def test_eval_3d_obj_tool_repair_flag(dev, tmp_path):
    from cnr_amd import metrics, vis
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
    out = logs / "room_0" / "eval_mesh"
    gt = vis.load_mesh(str(hab / "mesh_semantic.ply_1.ply"))
    rec = vis.load_mesh(str(mdir / "iteration_10000_obj1.obj"))
    box = metrics.oriented_bounds(gt)
    tables = {}
    for flags in ((), ("--repair",)):
        r = subprocess.run([sys.executable, tool, "--data_dir", str(data), "--log_dir", str(logs), "--volume", "5000", *flags],
                           capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout + r.stderr
        tables[flags] = json.loads((out / "metrics_3D_obj_volume.json").read_text())
    # without the flag: what volume_iou gives on the meshes as they come, the keys of before
    plain = tables[()]["objects"]["1"]
    want = metrics.volume_iou(rec, gt, N=5000, box=box)
    assert plain == json.loads(json.dumps(want)) and sorted(tables[()]) == ["mean", "objects", "objects_in_mean", "points"]
    # with it: the counts of boxes oriented by hand
    hand = [(m.vertices, hand_oriented(m.vertices, m.faces.astype(np.int32), 0.5 * (m.vertices.min(0) + m.vertices.max(0))))
            for m in (rec, gt)]
    want = metrics.volume_iou(*hand, N=5000, box=box, orientation=("outward", "outward"))
    row = tables[("--repair",)]["objects"]["1"]
    for k in ("intersection", "union", "inside_a", "inside_b", "n"):
        assert row[k] == want[k], k
    assert row["iou"] == want["intersection"] / want["union"] and row["orientation_a"] == row["orientation_b"] == 1
    assert abs(row["iou"] - 0.48 * 0.38 * 0.28 / 0.06) < 0.03 and row != plain      # the volumes' ratio, within the counting noise
    r = subprocess.run([sys.executable, tool, "--data_dir", str(data), "--log_dir", str(logs), "--repair"], capture_output=True, text=True,
                       cwd=str(tmp_path))
    assert r.returncode != 0 and "--repair goes with --volume" in r.stderr


def test_time_meshorient_tool_writes_its_rows(dev, tmp_path):
    out = tmp_path / "meshorient_time.json"
    tool = os.path.join(ROOT, "tools", "time_meshorient.py")
    r = subprocess.run([sys.executable, tool, "--dims", "16", "--ladder", "300", "--reps", "2", "--out", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    table = json.loads(out.read_text())
    assert table["reps"] == 2 and [row["mesh"] for row in table["rows"]] == ["marching cubes sphere 16^3", "ladder ascending"]
    for row in table["rows"]:
        assert row["equal_to_host"] and row["orient"]["patches"] == 1 and row["ms_host_bfs"] > 0
        for part in ("orient", "components"):
            assert row[part]["ms_total"] > row[part]["ms_torch_sort"] > 0
            assert abs(sum(row[part]["stages_ms"].values()) - row[part]["ms_total"]) < 0.01
        assert set(row["orient"]["stages_ms"]) == {"check", "edge_keys", "sort_edges", "union", "flatten", "roots_assign", "check_links",
                                                   "sort_faces", "patch_stats", "apply"}
        assert row["orient_over_components_without_sort"] > 0 and row["host_over_orient"] > 0
    assert table["rows"][1]["F"] == 598 and 0 < table["rows"][1]["flipped_in"] < 598
