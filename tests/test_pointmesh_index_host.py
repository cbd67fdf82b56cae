"""The tile-box index of the point-to-mesh distance without a GPU: the margin C of the skip rule measured from the numpy
restatement of the pair arithmetic (tests/pointmesh_cpu.py) alone, the restated indexed search (tests/pointmesh_index_cpu.py)
against ``closest_f32`` bit for bit, the warning-free build and the C-ABI."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cnr_amd
import pointmesh_cpu as P
import pointmesh_index_cpu as X
from conftest import ROOT
from test_abi import assert_row_matches, declared_functions, load_library

PKG = os.path.join(ROOT, "category-nerf-reconstruction-official_amd")
NEW = ("cnr_pm_index_params", "cnr_pm_index_bytes", "cnr_pm_index_keys", "cnr_pm_index_build", "cnr_pm_query_keys",
       "cnr_point_mesh_indexed_workspace_bytes", "cnr_point_mesh_dist_indexed")


# ---- the margin ---------------------------------------------------------------------------------------------------------------
def test_margin_constant_is_four_times_the_measured_excess():
    """The worst (lb - sqrt(d2_32)) / (2^-24 (lb + L)) over ALL (query, face) pairs, d2_32 from pointmesh_cpu._pairs (the
    arithmetic closest_f32 uses, never the code under test), for the per-face box, the face's tile box and the group-box
    form, on every BIT_CASES scene, with the queries shifted by 100 m and by 1000 m, and on the near-planar scene.
    Measured: 4.452 (per-face box, (2049, 1000), unshifted); the tile box 2.553, the group box never above the pair value."""
    worst = np.full(3, -np.inf)
    scenes = [P.random_case(nq, F) + ("(%d, %d)" % (nq, F),) for nq, F in P.BIT_CASES] + [X.near_planar_scene()[:3] + ("near-planar",)]
    for q, v, f, name in scenes:
        for shift in (0.0, 100.0, 1000.0) if name != "near-planar" else (0.0,):
            e = np.array(X.excess(q + np.float32(shift), v, f))
            print("%s + %g: face box %.3f, tile box %.3f, group box %.3f" % (name, shift, *e))
            worst = np.maximum(worst, e)
    print("worst: face box %.4f, tile box %.4f, group box %.4f" % tuple(worst))
    assert worst.max() <= X.C_MARGIN / 4
    assert X.C_MARGIN & (X.C_MARGIN - 1) == 0 and X.MARGIN == np.float32(X.C_MARGIN * 2.0 ** -24)
    assert 0.9 * X.MEASURED_EXCESS <= worst.max() <= X.MEASURED_EXCESS                      # the stated value is the measured one


# ---- the restated search ------------------------------------------------------------------------------------------------------
def _same(q, verts, faces=None):
    ref = P.closest_f32(q, verts, faces)
    d, face, near, d2, visited = X.search(q, verts, faces)
    assert np.array_equal(d2, ref[3]) and np.array_equal(face, ref[1]), int((face != ref[1]).sum())
    assert np.array_equal(d, ref[0]) and np.array_equal(near, ref[2])
    groups, tiles = -(-len(np.reshape(q, (-1, 3))) // X.GROUP), -(-len(P.corners(verts, faces)) // X.TILE)
    assert len(visited) == groups and (visited >= 1).all() and (visited <= tiles).all()
    return ref, visited


@pytest.mark.parametrize("nq,F", P.BIT_CASES)
def test_restated_search_equals_closest_f32_bit_for_bit(nq, F):
    q, v, f = P.random_case(nq, F)
    _same(q, v, f)
    _same(q, P.soup(v, f))


@pytest.mark.parametrize("reverse", [False, True])
def test_restated_search_keeps_the_lowest_original_face_among_ties(reverse):
    """the cube in the given face order and reversed, and mixed with small faces inside the cube so that the cube's 12 faces are spread over several
    tiles and one of the two orders meets the higher-index face of a tie in the earlier tile"""
    q = P.cube_tie_queries()
    faces = P.CUBE_FACES[::-1].copy() if reverse else P.CUBE_FACES
    ref, _ = _same(q, P.CUBE_VERTS, faces)
    pairs = P._pairs(q, P.face_records(P.corners(P.CUBE_VERTS, faces, np.float32)))[0]
    assert ((pairs == ref[3][:, None]).sum(1) >= 2).all()
    _, pv, pf = P.random_case(8, 3 * X.TILE, 4)
    verts = np.concatenate([P.CUBE_VERTS, pv * np.float32(0.05) + np.float32(0.4)])       # small faces inside the cube
    mixed = np.concatenate([pf + 8, faces])
    order = np.random.default_rng(2).permutation(len(mixed))
    ref2, _ = _same(q, verts, mixed[order])
    ix = X.build(verts, mixed[order])
    cube_pos = np.flatnonzero(np.isin(ix["orig"], np.flatnonzero(order >= len(pf))))
    assert len(np.unique(cube_pos // X.TILE)) >= 2                                         # the cube's faces lie in several tiles


def test_restated_search_on_a_doubled_mesh_answers_from_the_first_half():
    for nq, F in ((65, 257), (100, 2000)):
        q, v, f = P.random_case(nq, F)
        ref, _ = _same(q, np.concatenate([v, v]), np.concatenate([f, f + len(v)]))
        assert (ref[1] < F).all()


def test_restated_search_on_degenerate_faces_and_the_grid_scene():
    q, verts, faces, _ = P.degenerate_mesh()
    _same(q, verts, faces)
    q, v = P.grid_scene()
    a, _ = _same(q, v)
    b, _ = _same(q + P.GRID_SHIFT, v + P.GRID_SHIFT)
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[1], b[1])


def _whole_tiles_of_one_sheet(verts, faces, sheet):
    ix = X.build(verts, faces)
    per_tile = [np.unique(sheet[ix["orig"][t * X.TILE:(t + 1) * X.TILE]]) for t in range(ix["T"])]
    assert ix["T"] == 4 and [len(u) for u in per_tile] == [1, 1, 1, 1] and sorted(int(u[0]) for u in per_tile) == [0, 0, 1, 1]


def test_restated_search_on_the_near_planar_scene_skips_tiles():
    """each sheet fills two whole tiles, and the groups of low queries skip tiles: the skip rule decides here"""
    q, v, f, sheet = X.near_planar_scene()
    _whole_tiles_of_one_sheet(v, f, sheet)
    assert np.abs(v[:, 2]).max() <= 1e-6 and q[:, 2].min() >= 1e-3 and q[:, 2].max() <= 1.0 and q[:, 2].min() < 2e-3 < 0.5 < q[:, 2].max()
    _, visited = _same(q, v, f)
    print("near-planar: %d of %d tile evaluations" % (visited.sum(), len(visited) * 4))
    assert visited.sum() < len(visited) * 4 and visited.min() == 1 and visited.max() == 4


def test_restated_search_on_a_sphere_skips_tiles():
    """queries at 1.02 r: the answer is 2 % of the radius away and most of the sphere much farther, so most tiles are skipped;
    what is left must still be closest_f32's answer"""
    q, v, f = X.sphere_scene()
    _, visited = _same(q, v, f)
    tiles = -(-len(f) // X.TILE)
    print("sphere: %d of %d tile evaluations" % (visited.sum(), len(visited) * tiles))
    assert visited.sum() < len(visited) * tiles


def test_restated_search_on_the_two_clusters():
    q, v, f = X.two_clusters()
    _, visited = _same(q, v, f)
    assert len(f) == 2 * 512 and visited.sum() <= len(visited) * 512 // X.TILE             # the far cluster is never evaluated


def test_an_extent_that_overflows_gives_cell_zero():
    big = np.float32(3e38)
    v = np.array([[-big, 0, 0], [big, 1, 0], [0, 0, 1]], np.float32)
    keys = X.query_keys(np.array([[0, 1, 1], [big, 0, 0]], np.float32), X.bbox_of(v))
    assert keys.tolist() == [(0x09249249 << 1) | (0x09249249 << 2), 0]                     # x has no usable extent: its cell is 0


def test_keys_of_a_zero_extent_axis_and_of_clamped_queries():
    v = np.array([[0, 0, 1], [1, 0, 1], [0, 2, 1]], np.float32)                            # z has no extent
    bbox = X.bbox_of(v)
    keys = X.query_keys(np.array([[0, 0, 1], [1, 2, 1], [5, 5, 5], [-5, -5, -5], [0.5, 1, 9]], np.float32), bbox)
    assert keys.tolist() == [0, 0x09249249 | (0x09249249 << 1), 0x09249249 | (0x09249249 << 1), 0, int(X._spread(np.array([512]))[0]) * 3]
    assert (X.face_keys(P.corners(v, None, np.float32), bbox) == X._keys(np.array([[0.5, 1, 1]], np.float32), bbox)).all()
    assert (X.query_keys(np.ones((3, 3), np.float32), X.bbox_of(np.ones((3, 3), np.float32))) == 0).all()


# ---- build and ABI ------------------------------------------------------------------------------------------------------------
def test_point_mesh_index_build_is_warning_free():
    """csrc/point_mesh_index.hip and csrc/point_mesh.hip (which now shares point_mesh_common.h), with the Makefile's compiler and
    flags plus -Werror, into a temporary directory"""
    csrc = os.path.join(PKG, "csrc")
    cmd = subprocess.run(["make", "-s", "-C", csrc, "--no-print-directory", "--eval",
                          "print-compile: ; @echo $(HIPCC) $(CXXFLAGS)", "print-compile"],
                         capture_output=True, text=True, check=True).stdout.split()
    assert "-Wall" in cmd
    with tempfile.TemporaryDirectory() as d:
        for unit in ("point_mesh_index", "point_mesh"):
            out = subprocess.run(cmd + ["-Werror", "-c", os.path.join(csrc, unit + ".hip"), "-o", os.path.join(d, unit + ".o")],
                                 capture_output=True, text=True)
            assert out.returncode == 0, out.stderr
            assert "warning" not in (out.stdout + out.stderr).lower(), out.stderr


def test_library_exports_the_index_symbols():
    lib = load_library()
    fns = declared_functions()
    for name in NEW:
        assert name in fns and hasattr(lib, name) and name in cnr_amd._C.SIGNATURES, name
        assert_row_matches(name, cnr_amd._C.SIGNATURES[name], fns[name])
    assert {n for n in NEW if n in cnr_amd._C._RESTYPE64} == {"cnr_pm_index_bytes", "cnr_point_mesh_indexed_workspace_bytes"}
    assert hasattr(cnr_amd.metrics, "MeshIndex") and "MeshIndex" in cnr_amd.metrics.__all__
    import inspect
    for fn in (cnr_amd.metrics.point_mesh_distance, cnr_amd.metrics.calc_3d_metric_surface, cnr_amd.meshops.deviation,
               cnr_amd.meshops.deviation_mesh):
        assert not inspect.signature(fn).parameters["index"].default                       # opt-in: off by default


def test_index_argument_errors_are_return_codes():
    lib = load_library()
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 2 ** 31
    tile, group = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.cnr_pm_index_params(ctypes.byref(tile), ctypes.byref(group)) == 0
    assert (tile.value, group.value) == (X.TILE, X.GROUP)
    assert tile.value & (tile.value - 1) == 0 and 1 <= tile.value <= 512
    assert lib.cnr_pm_index_params(None, ctypes.byref(group)) == -1 and lib.cnr_pm_index_params(ctypes.byref(tile), None) == -1
    assert lib.cnr_pm_index_bytes(0) == -2 and lib.cnr_pm_index_bytes(big) == -2 and lib.cnr_pm_index_bytes(big - 1) > 0
    assert lib.cnr_point_mesh_indexed_workspace_bytes(0, 5) == -2 and lib.cnr_point_mesh_indexed_workspace_bytes(5, 0) == -2
    assert lib.cnr_point_mesh_indexed_workspace_bytes(5, big) == -2
    assert lib.cnr_pm_index_keys(None, None, 4, p, p, None) == -1 and lib.cnr_pm_index_keys(p, None, 4, None, p, None) == -1
    assert lib.cnr_pm_index_keys(p, None, 4, p, None, None) == -1
    assert lib.cnr_pm_index_keys(p, None, 0, p, p, None) == -2 and lib.cnr_pm_index_keys(p, None, big, p, p, None) == -2
    assert lib.cnr_pm_query_keys(None, 4, p, p, None) == -1 and lib.cnr_pm_query_keys(p, 4, None, p, None) == -1
    assert lib.cnr_pm_query_keys(p, 4, p, None, None) == -1 and lib.cnr_pm_query_keys(p, 0, p, p, None) == -2
    assert lib.cnr_pm_index_build(None, None, 4, p, p, p, None) == -1 and lib.cnr_pm_index_build(p, None, 4, None, p, p, None) == -1
    assert lib.cnr_pm_index_build(p, None, 4, p, None, p, None) == -1 and lib.cnr_pm_index_build(p, None, 4, p, p, None, None) == -1
    assert lib.cnr_pm_index_build(p, None, 0, p, p, p, None) == -2 and lib.cnr_pm_index_build(p, None, big, p, p, p, None) == -2
    ok = [p, 4, p, p, p, 4, p, p, None, p, None]
    for k in (0, 2, 3, 4, 6, 7, 9):                                                        # every required pointer
        args = list(ok)
        args[k] = None
        assert lib.cnr_point_mesh_dist_indexed(*args) == -1, k
    for k, bad in ((1, 0), (5, 0), (5, big)):
        args = list(ok)
        args[k] = bad
        assert lib.cnr_point_mesh_dist_indexed(*args) == -2, (k, bad)


def test_index_sizes_follow_the_documented_formulas():
    """cnr_pm_index_bytes(F) = align256(64 F) + align256(32 tiles), tiles = ceil(F / TILE); the query's workspace is
    align256(4 groups), groups = ceil(nq / GROUP)"""
    lib = load_library()
    for nq, F in P.BIT_CASES + (P.LARGE_CASE, (200000, 442700), (1, 70000), (5000000, 300), (X.GROUP + 1, X.TILE + 1)):
        assert lib.cnr_pm_index_bytes(F) == X.index_bytes(F), F
        assert lib.cnr_point_mesh_indexed_workspace_bytes(nq, F) == X.workspace_bytes(nq), nq
    assert X.index_bytes(1) == 512 and X.index_bytes(X.TILE + 1) == P.align256(64 * (X.TILE + 1)) + 256
    assert X.workspace_bytes(X.GROUP * 64 + 1) == 512
