"""CPU: mesh clean-up without a GPU -- the restatement tests/meshops_cpu.py against a brute-force
breadth-first search on every fixture the GPU tests use; each fixture's condition proved from the restatement alone; the shared
union/find of csrc/mesh_topo_common.h in a stand-alone host program under the address and undefined-behaviour sanitizers; the
component selection of clean_mesh (host logic); and the C-ABI of the new entry points."""
import ctypes
import math
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cnr_amd
import mc_cpu as M
import meshops_cpu as R
from conftest import ROOT
from test_abi import assert_row_matches, declared_functions, load_library

NEW = ("cnr_mesh_check_faces", "cnr_mesh_labels_init", "cnr_mesh_union_pairs", "cnr_mesh_union_faces", "cnr_mesh_edge_keys",
       "cnr_mesh_union_edges", "cnr_mesh_flatten_workspace_bytes", "cnr_mesh_flatten", "cnr_mesh_roots_workspace_bytes",
       "cnr_mesh_roots_count", "cnr_mesh_roots_emit", "cnr_mesh_assign", "cnr_mesh_cross_component", "cnr_mesh_edge_stats",
       "cnr_mesh_component_stats_workspace_bytes", "cnr_mesh_component_stats", "cnr_mesh_compact_workspace_bytes", "cnr_mesh_compact_count", "cnr_mesh_compact_emit",
       "cnr_weld_runs", "cnr_mesh_remap_faces")
CSRC = os.path.join(ROOT, "category-nerf-reconstruction-official_amd", "csrc")
LADDER_N = 100000
LADDER_ORDERS = ("ascending", "descending", "shuffled", "permuted")


@pytest.fixture(scope="module")
def cnr():
    assert cnr_amd.meshops.CONNECTIVITY == ("edge", "vertex")
    return cnr_amd


def mc_mesh(vol):
    v, _, f = M.marching_cubes(vol)
    return v, f


def fixtures():
    """name -> (verts, faces) of every mesh the GPU tests label"""
    out = {"triangles_%d" % F: R.disjoint_triangles(F) for F in (1, 63, 64, 65, 255, 256, 257, 1025)}
    out.update(pinch=R.pinch(), open_sheet=R.open_sheet(), fan3=R.fan3(), flipped=R.flipped_tetra(), halves=R.sphere_halves(),
               sheets=R.sheets([(1, 1), (1, 3), (2, 2), (2, 4)]), two_spheres=mc_mesh(M.two_spheres(64)))
    out.update({"random_%d" % s: mc_mesh(M.random_binary(24, s)) for s in (0, 1)})
    return out


# ---- the restatement against a breadth-first search ------------------------------------------------------------------------
def test_restated_labels_are_the_bfs_minima():
    for name, (v, f) in fixtures().items():
        for pairs, n in ((R.vertex_pairs(f), len(v)), (R.edge_pairs(f), len(f))):
            assert np.array_equal(R.labels_from_pairs(pairs, n), R.labels_bfs(pairs, n)), name


@pytest.mark.parametrize("order", LADDER_ORDERS)
def test_restated_ladder_is_one_component(order):
    v, f = R.ladder(LADDER_N, order)
    assert len(v) == 2 * LADDER_N and len(f) == 2 * (LADDER_N - 1) and len(np.unique(f)) == 2 * LADDER_N
    for pairs, n in ((R.vertex_pairs(f), len(v)), (R.edge_pairs(f), len(f))):
        lab = R.labels_from_pairs(pairs, n)
        assert (lab == 0).all()
        assert np.array_equal(lab, R.labels_bfs(pairs, n))
    if order == "ascending":                        # the chain the issue pictures: every face's lowest vertex ascends with it
        assert (np.diff(f.min(1)) >= 0).all()
    t = R.components(f, len(v), v, "edge")
    assert t["n"] == 1 and t["boundary_edges"] == 2 * LADDER_N and t["nonmanifold_edges"] == 0 and t["edge_counts"][0, 2] == 0
    assert t["area"][0] == LADDER_N - 1                      # unit quads: every partial sum is exact


def test_edge_pairs_are_the_shared_edges():
    """the neighbours of the sorted keys against a dictionary of undirected edges"""
    for name, (v, f) in fixtures().items():
        if len(f) > 3000:
            continue
        by_edge = {}
        for i, (a, b, c) in enumerate(f):
            for e in ((a, b), (b, c), (c, a)):
                if e[0] != e[1]:
                    by_edge.setdefault((min(e), max(e)), []).append(i)
        want = R.labels_bfs([(g[0], h) for g in by_edge.values() for h in g[1:]], len(f))
        assert np.array_equal(R.labels_from_pairs(R.edge_pairs(f), len(f)), want), name


# ---- the fixtures' conditions ----------------------------------------------------------------------------------------------
def test_fixture_conditions():
    fx = fixtures()
    for F in (1, 63, 64, 65, 255, 256, 257, 1025):
        v, f = fx["triangles_%d" % F]
        for conn in ("edge", "vertex"):
            t = R.components(f, len(v), v, conn)
            assert t["n"] == F and (t["vertex_component"][-2:] == -1).all() and (t["vertex_component"][:-2] >= 0).all()
            assert np.array_equal(t["face_component"], np.arange(F)) and t["boundary_edges"] == 3 * F
    v, f = fx["pinch"]
    assert R.components(f, len(v), v, "vertex")["n"] == 1
    t = R.components(f, len(v), v, "edge")
    assert t["n"] == 2 and t["watertight"].all() and t["vertex_component"][3] == 0 and t["n_vertices"].tolist() == [4, 3]
    v, f = fx["open_sheet"]
    t = R.components(f, len(v), v)
    assert t["n"] == 1 and t["boundary_edges"] == 2 * (5 + 7) and not t["watertight"][0] and t["edge_counts"][0, 2] == 0
    assert t["area"][0] == 35.0
    v, f = fx["fan3"]
    t = R.components(f, len(v), v)
    assert t["n"] == 1 and t["nonmanifold_edges"] == 1 and t["boundary_edges"] == 6
    v, f = fx["flipped"]
    t = R.components(f, len(v), v)
    assert t["n"] == 1 and t["boundary_edges"] == 0 and t["nonmanifold_edges"] == 0 and t["edge_counts"][0, 2] == 3
    assert not t["watertight"][0]
    assert R.components(R.TETRA, 4, R.TETRA_V)["watertight"].all()
    v, f = fx["two_spheres"]
    t = R.components(f, len(v), v)
    assert t["n"] == 2 and t["watertight"].all() and t["n_faces"].sum() == len(f)
    for c in range(2):
        sel = t["face_component"] == c
        assert M.euler(v, f[sel]) == 2
        assert abs(t["area"][c] - R.fsum_area(v, f, t["face_component"], c)) <= len(f) * 2.0 ** -53 * t["area"][c]
    for s in (0, 1):
        v, f = fx["random_%d" % s]
        t = R.components(f, len(v), v)
        assert t["n"] >= 100, t["n"]
        assert M.boundary_edges_on_outer_faces(v, f, 24)
        assert R.components(f, len(v), v, "vertex")["n"] <= t["n"]
    v, f = fx["halves"]
    assert R.components(f, len(v), v)["n"] == 2 and R.components(f, len(v), v)["boundary_edges"] > 0
    kept, nf, remap = R.weld(v, f)
    t = R.components(nf, len(kept), v[kept])
    assert t["n"] == 1 and t["watertight"].all() and len(kept) == len(R.icosphere()[0]) and len(nf) == len(f)
    v, f = fx["sheets"]
    t = R.components(f, len(v), v)
    assert t["area"].tolist() == [1.0, 3.0, 4.0, 8.0] and t["n_faces"].tolist() == [2, 6, 8, 16]


def test_weld_fixture_conditions():
    v, f, soup = R.exact_weld_case()
    assert np.signbit(v[:, 2]).any() and (~np.signbit(v[:, 2])).any() and (v[:, 2] == 0).all()
    assert np.isnan(soup[-1]).any() and len(soup) == len(f) + 1
    kept, nf, remap = R.weld(soup)
    # the indexed mesh comes back with its very indices; the NaN face keeps three vertices of its own
    assert np.array_equal(nf[:-1], f) and nf[-1].tolist() == [len(v), len(v) + 1, len(v) + 2] and len(kept) == len(v) + 3
    assert np.array_equal(soup.reshape(-1, 3)[kept][:len(v)], v)                      # -0 == +0 as values
    assert (np.diff(kept) > 0).all() and np.array_equal(remap[kept], np.arange(len(kept)))
    # degenerate faces
    vv = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 1, 0]], np.float32)
    ff = np.array([[0, 1, 2], [0, 1, 3]], np.int32)
    assert R.weld(vv, ff)[1].tolist() == [[0, 1, 2]] and R.weld(vv, ff, drop_degenerate=False)[1].tolist() == [[0, 1, 0], [0, 1, 2]]
    # cell > 0: no coordinate within 1e-3 cell of a boundary, so no rounding of the key arithmetic can move a point across one
    pts, ids, cell = R.jittered_lattice()
    keys, margin = R.voxel_keys(pts, cell)
    assert margin > 0.25 and (keys >= 0).all(), margin
    kept, _, remap = R.weld(pts, np.zeros((0, 3), np.int32), cell=cell)
    assert len(kept) == 6 ** 3
    for a in np.unique(ids):                                                          # same lattice point <=> same welded vertex
        assert len(np.unique(remap[ids == a])) == 1
    assert len(np.unique(remap)) == 6 ** 3
    first = np.array([np.flatnonzero(ids == a)[0] for a in np.unique(ids)])
    assert np.array_equal(np.sort(first), kept)                                       # the representative is the lowest input index


def test_restated_compaction_is_cull_mesh(cnr):
    rng = np.random.default_rng(5)
    v, f = mc_mesh(M.random_binary(12, 3))
    mesh = cnr.vis.Mesh(v, f, rng.normal(size=v.shape))
    mesh.visual.vertex_colors = rng.integers(0, 256, (len(v), 3))
    for keep in (rng.random(len(f)) < 0.3, np.zeros(len(f), bool), np.ones(len(f), bool)):
        nf, vmap, used = R.compact(f, len(v), keep)
        ref = cnr.raster.cull_mesh(mesh, keep)
        assert np.array_equal(ref.faces, nf) and np.array_equal(ref.vertices, mesh.vertices[used])
        assert np.array_equal(ref.vertex_normals, mesh.vertex_normals[used])


def test_wave_sum_order():
    rng = np.random.default_rng(0)
    for n in (1, 63, 64, 65, 1000):
        a = rng.random(n)
        s = R.wave_sum(a)
        assert abs(s - math.fsum(a)) <= n * 2.0 ** -53 * math.fsum(a)
        lanes = [sum(a[l::64].tolist(), 0.0) for l in range(64)]               # python's left-to-right sum per lane
        for d in (32, 16, 8, 4, 2, 1):
            lanes = [lanes[i] + lanes[i + d] for i in range(d)]
        assert s == lanes[0]


# ---- the union/find on the host --------------------------------------------------------------------------------------------
def test_union_find_in_a_host_program(tmp_path):
    """csrc/mesh_topo_common.h compiled by the host compiler with the address and undefined-behaviour sanitizers: unions with
    path halving and the flatten sweeps on ladders ascending, descending, shuffled and permuted, against a breadth-first search"""
    exe = str(tmp_path / "meshcc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "meshcc_unionfind_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr


# ---- clean_mesh's selection (host logic on a table) ------------------------------------------------------------------------
def _table(area, n_faces, diag):
    return SimpleNamespace(n=len(area), area=torch.tensor(area, dtype=torch.float64), diag=torch.tensor(diag, dtype=torch.float64),
                           n_faces=torch.tensor(n_faces, dtype=torch.int32))


def test_select_components(cnr):
    sel = cnr.meshops.select_components
    t = _table([1.0, 3.0, 4.0, 8.0], [2, 6, 8, 16], [1.0, 2.0, 2.5, 4.0])
    assert sel(t).tolist() == [True] * 4
    assert sel(t, min_faces=6).tolist() == [False, True, True, True]                  # exactly on the threshold: kept
    assert sel(t, min_faces=7).tolist() == [False, False, True, True]
    assert sel(t, min_area=4.0).tolist() == [False, False, True, True]
    assert sel(t, min_area=np.nextafter(4.0, 5.0)).tolist() == [False, False, False, True]
    assert sel(t, min_diag=2.5).tolist() == [False, False, True, True]
    assert sel(t, min_area_fraction=0.25).tolist() == [False, False, True, True]      # 0.25 x 16 = 4 exactly
    assert sel(t, keep_largest=1).tolist() == [False, False, False, True]
    assert sel(t, keep_largest=2, min_faces=3).tolist() == [False, False, True, True]
    assert sel(t, keep_largest=9).tolist() == [True] * 4
    assert sel(t, min_area=100.0).tolist() == [False, False, False, True]             # never empty: the largest stays
    tie = _table([4.0, 4.0, 4.0], [8, 9, 9], [1.0, 3.0, 3.0])
    assert sel(tie, keep_largest=1).tolist() == [True, False, False]                  # ties: the lower id
    assert sel(tie, keep_largest=1, largest_by="faces").tolist() == [False, True, False]
    assert sel(tie, keep_largest=2, largest_by="diag").tolist() == [False, True, True]
    assert sel(_table([], [], [])).tolist() == []
    with pytest.raises(ValueError):
        sel(t, largest_by="volume")
    with pytest.raises(ValueError):
        sel(t, keep_largest=0)
    assert cnr.meshops.parse_clean_options("keep_largest=1, min_area=0.5,weld=0,connectivity=vertex") == dict(
        keep_largest=1, min_area=0.5, weld=0.0, connectivity="vertex")
    assert cnr.meshops.parse_clean_options("") == {}
    with pytest.raises(ValueError):
        cnr.meshops.parse_clean_options("biggest=1")


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_symbols(cnr):
    lib = load_library()
    fns = declared_functions()
    for name in NEW:
        assert name in fns and hasattr(lib, name) and name in cnr._C.SIGNATURES, name
        assert_row_matches(name, cnr._C.SIGNATURES[name], fns[name])
    for name in ("weld", "components", "compact", "clean_mesh", "MeshComponents", "union_find"):
        assert hasattr(cnr.meshops, name), name


def test_argument_errors_are_return_codes():
    """host pointers and no GPU: sizes outside the contract are refused before anything is read or launched"""
    lib = load_library()
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 2 ** 31
    assert lib.cnr_mesh_check_faces(p, 0, 4, p, None) == -2 and lib.cnr_mesh_check_faces(p, 1, 0, p, None) == -2
    assert lib.cnr_mesh_check_faces(p, big // 3 + 1, 4, p, None) == -2 and lib.cnr_mesh_check_faces(p, 1, big, p, None) == -2
    assert lib.cnr_mesh_check_faces(None, 1, 4, p, None) == -1 and lib.cnr_mesh_check_faces(p, 1, 4, None, None) == -1
    assert lib.cnr_mesh_labels_init(p, 0, None) == -2 and lib.cnr_mesh_labels_init(None, 4, None) == -1
    assert lib.cnr_mesh_union_pairs(p, 0, 4, p, p, None) == -2 and lib.cnr_mesh_union_pairs(p, 1, big, p, p, None) == -2
    assert lib.cnr_mesh_union_pairs(p, 1, 4, None, p, None) == -1
    assert lib.cnr_mesh_union_faces(p, 1, 4, p, None, p, None) == -1 and lib.cnr_mesh_union_faces(p, 0, 4, p, p, p, None) == -2
    assert lib.cnr_mesh_edge_keys(p, 0, p, None) == -2 and lib.cnr_mesh_edge_keys(p, 1, None, None) == -1
    assert lib.cnr_mesh_union_edges(p, p, 0, p, p, None) == -2 and lib.cnr_mesh_union_edges(p, None, 1, p, p, None) == -1
    assert lib.cnr_mesh_flatten_workspace_bytes(0) == -2 and lib.cnr_mesh_flatten_workspace_bytes(big) == -2
    assert lib.cnr_mesh_flatten_workspace_bytes(8) == 256 and lib.cnr_mesh_flatten_workspace_bytes(big - 1) == 256
    assert lib.cnr_mesh_flatten(p, 4, None, p, None) == -1 and lib.cnr_mesh_flatten(p, 0, p, p, None) == -2
    assert lib.cnr_mesh_roots_workspace_bytes(0) == -2 and lib.cnr_mesh_roots_workspace_bytes(1025) == 512
    assert lib.cnr_mesh_roots_count(p, None, 4, p, None, None) == -1 and lib.cnr_mesh_roots_emit(p, None, 0, p, p, None) == -2
    assert lib.cnr_mesh_assign(p, None, 4, p, 0, p, p, None) == -2 and lib.cnr_mesh_assign(p, None, 4, p, 5, p, p, None) == -2
    assert lib.cnr_mesh_assign(p, None, 4, None, 1, p, p, None) == -1
    assert lib.cnr_mesh_cross_component(p, 1, 4, 2, p, p, None) == -2 and lib.cnr_mesh_cross_component(p, 1, 4, 0, None, p, None) == -1
    assert lib.cnr_mesh_edge_stats(p, p, p, 1, p, 0, p, None) == -2 and lib.cnr_mesh_edge_stats(p, p, p, 1, p, 1, None, None) == -1
    assert lib.cnr_mesh_component_stats(p, p, p, p, 1, 4, 1, p, p, p, p, None, p, p, None) == -1    # verts without area
    assert lib.cnr_mesh_component_stats(p, p, p, p, 1, 4, 1, p, None, p, p, p, p, p, None) == -1    # ... without workspace
    assert lib.cnr_mesh_component_stats(None, p, p, p, 1, 4, 0, p, None, p, p, None, None, None, None) == -2
    assert lib.cnr_mesh_component_stats_workspace_bytes(0) == -2 and lib.cnr_mesh_component_stats_workspace_bytes(33) == 512 + 1024
    assert lib.cnr_mesh_compact_workspace_bytes(0, 4) == -2 and lib.cnr_mesh_compact_workspace_bytes(1, 1) == 5 * 256
    assert lib.cnr_mesh_compact_count(p, 1, 4, None, 1, p, p, None) == -1 and lib.cnr_mesh_compact_count(p, 1, 0, p, 1, p, p, None) == -2
    assert lib.cnr_mesh_compact_emit(p, 1, 4, p, 1, p, p, None, p, None) == -1
    assert lib.cnr_weld_runs(p, p, p, 4, p, p, None) == -1 and lib.cnr_weld_runs(None, None, p, 4, p, p, None) == -1
    assert lib.cnr_weld_runs(p, None, p, 0, p, p, None) == -2
    assert lib.cnr_mesh_remap_faces(p, 0, p, 1, p, p, None) == -2 and lib.cnr_mesh_remap_faces(p, 1, None, 1, p, p, None) == -1


def test_host_tensors_and_bad_shapes_are_refused(cnr):
    with pytest.raises(cnr._C.CnrError):
        cnr.meshops.components(torch.zeros(4, 3, dtype=torch.int32), 12)
    with pytest.raises(ValueError):
        cnr.meshops.components(torch.zeros(4, 2, dtype=torch.int32), 12)
    with pytest.raises(ValueError):
        cnr.meshops.components(torch.zeros(4, 3, dtype=torch.int32), 12, connectivity="face")
    with pytest.raises(ValueError):
        cnr.meshops.weld(torch.zeros(4, 3, 2))
