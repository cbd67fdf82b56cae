"""CPU: mesh simplification without a GPU -- the restatement tests/meshsimplify_cpu.py against a
brute-force dictionary implementation on every fixture the GPU tests use; each fixture's own condition (eigenvalue margin, key
margin, the rotated cube's clamped clusters and its quality bar) proved from the restatement alone; the arithmetic of
csrc/mesh_simplify_common.h in a stand-alone host program under the address and undefined-behaviour sanitizers; the option
parser and the cell search (host logic); and the C-ABI of the new entry points."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import cnr_amd
import mc_cpu as M
import meshops_cpu as R
import meshsimplify_cpu as S
from conftest import ROOT
from test_abi import assert_row_matches, declared_functions, load_library

NEW = ("cnr_simplify_check_keys", "cnr_simplify_vertex_q", "cnr_simplify_face_records", "cnr_mesh_face_normals_f64",
       "cnr_segment_sum_f64", "cnr_simplify_place", "cnr_simplify_face_rows", "cnr_mesh_normals_finish")
CSRC = os.path.join(ROOT, "category-nerf-reconstruction-official_amd", "csrc")
FANS = (15, 16, 17, 31, 32, 33, 255, 257)
CLUSTER_COUNTS = (1, 63, 64, 65, 257)


@functools.lru_cache(maxsize=None)
def fixtures():
    """name -> (verts, faces, cell) of every mesh the GPU tests simplify"""
    out = {"one_triangle": (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32), 0.25)}
    out.update({"clusters_%d" % C: S.cluster_triangles(C) + (S.CELL,) for C in CLUSTER_COUNTS})
    out.update({"fan_%d" % n: S.fan(n) + (S.CELL,) for n in FANS})
    out.update(duplicate=S.duplicate_pair() + (S.CELL,), opposite=S.duplicate_pair(True) + (S.CELL,), lattice=S.lattice_mesh())
    iv, ifc = R.icosphere(4)
    ico = ((iv + np.float32([0.37, 0.11, 0.23])).astype(np.float32), ifc)       # off the origin: see test_coordinate_floor
    out.update(ico_a=ico + (0.2,), ico_b=ico + (0.3,))
    cube = S.rotated_cube()
    out.update(cube_a=cube + (0.08,), cube_b=cube + (0.15,))
    v, _, f = M.marching_cubes(M.two_spheres(64))
    out.update(two_spheres=(v, f, 0.05))
    return out


@functools.lru_cache(maxsize=None)
def restated(name, placement="quadric"):
    v, f, cell = fixtures()[name]
    return S.simplify(v, f, cell, placement)


# ---- the restatement against dictionaries ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fixtures()))
def test_restatement_is_the_brute_force(name):
    v, f, cell = fixtures()[name]
    got, ref = restated(name), S.brute_force(v, f, cell)
    assert got["clusters"] == ref["clusters"] and got["faces_collapsed"] == ref["faces_collapsed"]
    assert np.array_equal(got["vertex_map"], ref["vertex_map"]), name
    if ref["faces"].size == 0:
        assert got["faces_out"] == 0 and got["vertices_out"] == 0 and (got["vertex_map"] == -1).all()
        return
    for k in ("cluster", "roots", "faces", "kept_clusters", "counts"):
        assert np.array_equal(got[k], ref[k]), (name, k)
    assert got["faces_duplicate"] == ref["faces_duplicate"] and got["faces_out"] == len(ref["faces"])
    assert got["faces_in"] == got["faces_collapsed"] + got["faces_duplicate"] + got["faces_out"]
    assert np.array_equal(got["representatives"], ref["roots"][ref["kept_clusters"]])
    # the sums: the fixed order against the exact sum of the same terms (the terms themselves differ in their last places)
    bound = 1e-10 * ref["abs_quadrics"].max(1, keepdims=True) + 1e-300
    assert (np.abs(got["quadrics"] - ref["quadrics"]) <= bound).all(), name
    assert (np.abs(got["possum"] - ref["possum"]) <= 1e-12 * (np.abs(ref["possum"]) + ref["counts"][:, None])).all(), name


def test_group_sum_order():
    rng = np.random.default_rng(0)
    for n in (0, 1, 15, 16, 17, 33, 1000):
        a = rng.random((n, 2)) - 0.5
        s = S.group_sum(a)
        for k in range(2):
            lanes = [sum(a[l::16, k].tolist(), 0.0) for l in range(16)]             # python's left-to-right sum per lane
            for d in (8, 4, 2, 1):
                lanes = [lanes[i] + lanes[i + d] for i in range(d)]
            assert s[k] == lanes[0]
            assert abs(s[k] - math.fsum(a[:, k])) <= n * 2.0 ** -53 * np.abs(a[:, k]).sum()
    seg = np.array([0, 0, 2, 2, 2], np.int32)                                        # an empty segment gives zeros
    out = S.segment_sums(np.arange(10.0).reshape(5, 2), np.arange(5), seg, 4)
    assert out.tolist() == [[2.0, 4.0], [0.0, 0.0], [18.0, 21.0], [0.0, 0.0]]


# ---- the fixtures' conditions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fixtures()))
def test_eigenvalue_margin(name):
    """no eigenvalue ratio within 1e-9 of tau at any cluster: round-off cannot change which eigenvalues are dropped"""
    got = restated(name)
    print(name, "smallest |lambda_i / lambda_max - tau|:", got["margin"], "clusters:", got["clusters"], "clamped:", got["clamped"])
    assert got["margin"] >= S.MARGIN, (name, got["margin"])


@pytest.mark.parametrize("name", sorted(fixtures()))
def test_coordinate_floor(name):
    """no output coordinate cancels to nearly nothing (S.coordinate_floor_ok): the icosphere stands off the origin for this"""
    got = restated(name)
    assert got["faces_out"] == 0 or S.coordinate_floor_ok(got["cluster_verts"], fixtures()[name][0]), name
    iv, ifc = R.icosphere(4)
    assert not S.coordinate_floor_ok(S.simplify(iv, ifc, 0.2)["cluster_verts"], iv)            # ... which at the origin does


def test_fixture_conditions():
    fx = fixtures()
    for C in CLUSTER_COUNTS:
        got = restated("clusters_%d" % C)
        assert got["clusters"] == C and got["faces_out"] == (C // 3 if C > 1 else 0)
        if C > 1:
            v, f, cell = fx["clusters_%d" % C]
            assert R.voxel_keys(v, cell)[1] >= 0.25
    for n in FANS:
        got = restated("fan_%d" % n)
        corners = np.bincount(got["cluster"][fx["fan_%d" % n][1].reshape(-1)], minlength=got["clusters"])
        assert corners[0] == n and corners[1:n + 1].tolist() == [2] * n and got["faces_out"] == n and got["clusters"] == n + 2
    assert restated("duplicate")["faces"].tolist() == [[3, 4, 5], [0, 1, 2]] and restated("duplicate")["faces_duplicate"] == 1
    assert restated("opposite")["faces_out"] == 3 and restated("opposite")["faces_duplicate"] == 0
    assert restated("opposite")["faces"].tolist() == [[3, 4, 5], [0, 1, 2], [0, 2, 1]]
    pts, f, cell = fx["lattice"]
    got = restated("lattice")
    assert R.voxel_keys(pts, cell)[1] > 0.25 and got["clusters"] == 6 ** 3
    assert got["faces_collapsed"] > 0 and got["faces_duplicate"] > 0 and got["faces_out"] > 0
    v, f, _ = fx["cube_a"]
    assert len(v) == 41 ** 3 - 39 ** 3 and len(f) == 6 * 40 * 40 * 2
    assert R.components(f, len(v))["watertight"].all() and np.abs(S.cube_surface_distance(v)).max() < 1e-6
    assert (np.einsum("ij,ij->i", S.vertex_normals(v, f), v - v.mean(0)) > 0).all()          # outward
    v, f, cell = fx["two_spheres"]
    assert restated("two_spheres")["faces_out"] < len(f) // 4


@pytest.mark.parametrize("name,clamped", [("cube_a", 29), ("cube_b", 19)])
def test_rotated_cube_clamps_and_quality(name, clamped):
    """the clamp path is exercised, every vertex lies in its cell, and the quadric placement is at least 4 x nearer to the cube's
    surface than the mean (the bar of the GPU test, here for the restatement)"""
    v, f, cell = fixtures()[name]
    got, mean = restated(name), restated(name, "mean")
    assert got["clamped"] == clamped, got["clamped"]
    lo, hi = S.cell_bounds(S.key_cells(got["keys"][got["roots"]]), cell)
    for r in (got, mean):
        q = r["cluster_verts"].astype(np.float64) - r["min"].astype(np.float64)
        assert ((q >= lo) & (q <= hi)).all()
    dq, dm = S.cube_surface_distance(got["verts"]).mean(), S.cube_surface_distance(mean["verts"]).mean()
    print(name, "mean distance to the surface: quadric", dq, "mean", dm, "ratio", dm / dq)
    assert dq <= dm / 4
    moved = np.linalg.norm(got["cluster_verts"][got["cluster"]].astype(np.float64) - v, axis=1)
    assert moved.max() <= math.sqrt(3) * cell * (1 + 2.0 ** -20)                                # (the bound, and fp32 positions)


def test_restated_search():
    v, f, _ = fixtures()["ico_a"]
    for target in (40, 300, len(f), 10 ** 6):
        cell, trials = S.search_cell(target, S.bbox_diag(v), lambda c: S.faces_out(v, f, c))
        assert len(trials) <= 24 and dict(trials)[cell] <= target
        assert all(n > target for c, n in trials if c < cell)
    assert S.search_cell(10 ** 6, S.bbox_diag(v), lambda c: S.faces_out(v, f, c))[1][-1][1] == len(f)      # the finest cell keeps every face
    cell, trials = cnr_amd.meshops.search_cell(300, S.bbox_diag(v), lambda c: S.faces_out(v, f, c))
    assert (cell, trials) == S.search_cell(300, S.bbox_diag(v), lambda c: S.faces_out(v, f, c))
    with pytest.raises(ValueError):
        cnr_amd.meshops.search_cell(10, 0.0, lambda c: 0)
    with pytest.raises(ValueError):
        cnr_amd.meshops.search_cell(10, 1.0, lambda c: 11)


def test_restated_vertex_normals():
    v, f = R.icosphere(3)
    n = S.vertex_normals(v, f)
    assert (np.einsum("ij,ij->i", n, v) > 0.99).all()                                          # a sphere's normals are radial
    v2 = np.concatenate([v, [[5, 5, 5]]]).astype(np.float32)
    assert S.vertex_normals(v2, f)[-1].tolist() == [0, 0, 0]                                   # an unused vertex
    both = np.concatenate([f[:1], f[:1, ::-1]])
    assert (S.vertex_normals(v, both) == 0).all()                                              # a zero sum
    mv, mn, mf = M.marching_cubes(M.two_spheres(64))                                           # the side marching cubes' normals point to
    assert (np.einsum("ij,ij->i", S.vertex_normals(mv, mf), mn) > 0).all()


# ---- the arithmetic on the host --------------------------------------------------------------------------------------------
def test_solve_in_a_host_program(tmp_path):
    """csrc/mesh_simplify_common.h compiled by the host compiler with the address and undefined-behaviour sanitizers"""
    exe = str(tmp_path / "meshsimplify_solve")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "meshsimplify_solve_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr


# ---- host logic --------------------------------------------------------------------------------------------------------------
def test_parse_simplify_options():
    parse = cnr_amd.meshops.parse_simplify_options
    assert parse("cell=0.02, placement=mean,tau=0.01") == dict(cell=0.02, placement="mean", tau=0.01)
    assert parse("target_faces=20000") == dict(target_faces=20000) and parse("") == {} and parse(None) == {}
    for bad in ("faces=3", "cell", "cell=", "cell=abc"):
        with pytest.raises(ValueError):
            parse(bad)


def test_bad_arguments_are_refused_before_the_device():
    simplify = cnr_amd.meshops.simplify
    v, f = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    for kw in (dict(), dict(cell=0.1, target_faces=5), dict(cell=0.0), dict(cell=-1.0), dict(cell=float("nan")),
               dict(cell=0.1, placement="median"), dict(cell=0.1, tau=1.0), dict(cell=0.1, tau=-0.1)):
        with pytest.raises(ValueError):
            simplify(v, f, **kw)
    with pytest.raises(ValueError):
        simplify(torch.zeros(4, 2), f, cell=0.1)
    with pytest.raises(cnr_amd._C.CnrError):
        simplify(v, f, cell=0.1)                                                               # host tensors: no CPU path
    with pytest.raises(cnr_amd._C.CnrError):
        cnr_amd.meshops.vertex_normals(v, f)


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_symbols():
    lib = load_library()
    fns = declared_functions()
    for name in NEW:
        assert name in fns and hasattr(lib, name) and name in cnr_amd._C.SIGNATURES, name
        assert_row_matches(name, cnr_amd._C.SIGNATURES[name], fns[name])
    # every new workspace query returns int64_t (this unit needs no workspace, so there is none to list)
    queries = [n for n in NEW if n.endswith("_bytes")]
    assert all(n in cnr_amd._C._RESTYPE64 for n in queries) and not any(n in cnr_amd._C._RESTYPE64 for n in NEW if n not in queries)
    for name in ("simplify", "simplify_mesh", "vertex_normals", "parse_simplify_options", "search_cell"):
        assert hasattr(cnr_amd.meshops, name), name


def test_argument_errors_are_return_codes():
    """host pointers and no GPU: sizes outside the contract are refused before anything is read or launched"""
    lib = load_library()
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 2 ** 31
    assert lib.cnr_simplify_check_keys(None, 4, p, None) == -1 and lib.cnr_simplify_check_keys(p, 0, p, None) == -2
    assert lib.cnr_simplify_check_keys(p, big, p, None) == -2
    assert lib.cnr_simplify_vertex_q(p, None, 4, p, None) == -1 and lib.cnr_simplify_vertex_q(p, p, 0, p, None) == -2
    assert lib.cnr_simplify_face_records(p, p, p, 1, 4, None, p, None) == -1
    assert lib.cnr_simplify_face_records(p, p, p, 0, 4, p, p, None) == -2 and lib.cnr_simplify_face_records(p, p, p, 1, big, p, p, None) == -2
    assert lib.cnr_mesh_face_normals_f64(p, p, 1, 4, p, None, None) == -1 and lib.cnr_mesh_face_normals_f64(p, p, big // 3 + 1, 4, p, p, None) == -2
    assert lib.cnr_segment_sum_f64(None, p, 1, p, 4, 4, 3, 2, p, p, None) == -1
    assert lib.cnr_segment_sum_f64(p, p, 1, p, 4, 4, 0, 2, p, p, None) == -2 and lib.cnr_segment_sum_f64(p, p, 1, p, 4, 4, 17, 2, p, p, None) == -2
    assert lib.cnr_segment_sum_f64(p, p, 0, p, 4, 4, 3, 2, p, p, None) == -2 and lib.cnr_segment_sum_f64(p, p, 1, p, 0, 4, 3, 2, p, p, None) == -2
    assert lib.cnr_segment_sum_f64(p, p, 1, p, 4, 4, 3, 0, p, p, None) == -2
    assert lib.cnr_segment_sum_f64(p, None, 1, p, 5, 4, 3, 2, p, p, None) == -2                 # no gather: an item per position
    ok = (p, p, p, p, p, p, p, 4, 2, 0.25, 1e-3, 0, p, p, p, p, None)
    def place(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.cnr_simplify_place(*a)
    assert place(a0=None) == -1 and place(a1=None) == -1 and place(a2=None) == -1 and place(a15=None) == -1
    assert place(a11=3) == -1 and place(a11=-1) == -1 and place(a9=0.0) == -1 and place(a9=float("inf")) == -1
    assert place(a10=1.0) == -1 and place(a10=-0.5) == -1 and place(a7=0) == -2 and place(a8=5) == -2 and place(a8=0) == -2
    assert lib.cnr_simplify_face_rows(p, 0, p, None) == -2 and lib.cnr_simplify_face_rows(p, 1, None, None) == -1
    assert lib.cnr_mesh_normals_finish(None, 4, p, None) == -1 and lib.cnr_mesh_normals_finish(p, 0, p, None) == -2
