"""CPU: orientation repair without a GPU -- the restatement tests/meshorient_cpu.py on hand cases whose
answers are written out here and on the fixtures' conditions; the union/find with a parity bit of csrc/mesh_topo_common.h in a
stand-alone host program under the address and undefined-behaviour sanitizers; and the C-ABI of the new entry points."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import cnr_amd
import mc_cpu as M
import meshops_cpu as R
import meshorient_cpu as OC
from conftest import ROOT
from test_abi import assert_row_matches, declared_functions, load_library

NEW = ("cnr_mesh_orient_keys", "cnr_mesh_orient_union", "cnr_mesh_orient_flatten", "cnr_mesh_orient_check",
       "cnr_mesh_orient_stats_workspace_bytes", "cnr_mesh_orient_stats", "cnr_mesh_orient_apply")
CSRC = os.path.join(ROOT, "category-nerf-reconstruction-official_amd", "csrc")


def same_direction_edges(faces, n_vertices):
    """the total of components' edge_counts[:, 2]: interior edges both of whose faces run them the same way"""
    return int(R.components(faces, n_vertices)["edge_counts"][:, 2].sum())


# ---- hand cases ------------------------------------------------------------------------------------------------------------
def test_two_triangles():
    v, f = OC.two_triangles(True)
    assert OC.links(f).tolist() == [[0, 1, 0]]
    out = OC.orient(f, len(v))
    assert out["n"] == 1 and out["faces"].tolist() == [[0, 1, 2], [1, 3, 2]] and out["flip"].tolist() == [0, 0]
    assert out["inconsistent_edges"].tolist() == [0] and out["orientable"].tolist() == [True] and out["closed"].tolist() == [False]
    assert out["n_flipped"].tolist() == [0] and out["signed_volume"] is None and out["first"].tolist() == [0]
    v, f = OC.two_triangles(False)
    assert OC.links(f).tolist() == [[0, 1, 1]]
    out = OC.orient(f, len(v))
    assert out["n"] == 1 and out["faces"].tolist() == [[0, 1, 2], [1, 3, 2]] and out["flip"].tolist() == [0, 1]
    assert out["inconsistent_edges"].tolist() == [1] and out["orientable"].tolist() == [True] and out["n_flipped"].tolist() == [1]
    assert out["face_patch"].tolist() == [0, 0] and out["n_faces"].tolist() == [2]
    # flipping twice is the identity
    assert np.array_equal(OC.flip_faces(OC.flip_faces(f, [1]), [1]), f)
    with pytest.raises(ValueError):
        OC.orient(f, len(v), outward=True)


def test_book_of_three_pages():
    v, f = OC.book()
    assert len(OC.links(f)) == 0
    out = OC.orient(f, len(v), v)
    assert out["n"] == 3 and out["face_patch"].tolist() == [0, 1, 2] and out["first"].tolist() == [0, 1, 2]
    assert np.array_equal(out["faces"], f) and not out["flip"].any() and out["n_flipped"].tolist() == [0, 0, 0]
    assert out["orientable"].all() and not out["closed"].any() and out["inconsistent_edges"].tolist() == [0, 0, 0]
    assert out["signed_volume"].tolist() == [0.0, 0.0, 0.0]                           # one planar face each
    assert R.components(f, len(v))["n"] == 1                                          # ... where components joins the sheets


def test_moebius_band_of_five_quads():
    v, f = OC.moebius(5)
    assert len(f) == 10 and len(np.unique(f)) == 10
    t = R.components(f, len(v))
    assert t["n"] == 1 and t["nonmanifold_edges"] == 0 and t["boundary_edges"] == 10          # one boundary curve of 10 edges
    assert M.euler(v, f) == 0
    out = OC.orient(f, len(v), v)
    assert out["n"] == 1 and out["orientable"].tolist() == [False] and not out["flip"].any() and np.array_equal(out["faces"], f)
    assert out["inconsistent_edges"].tolist() == [1] and out["n_flipped"].tolist() == [0] and out["closed"].tolist() == [False]
    # any flip set leaves an inconsistent edge: try them all
    for bits in range(1 << 10):
        mask = np.array([(bits >> k) & 1 for k in range(10)], bool)
        assert same_direction_edges(OC.flip_faces(f, mask), len(v)) >= 1
    # the untwisted strip of the same size is orientable, and comes back whatever was flipped
    v, f = OC.quad_strip(5, False)
    assert same_direction_edges(f, len(v)) == 0
    for seed in range(3):
        g, mask = OC.random_flips(f, seed)
        out = OC.orient(g, len(v))
        want = OC.flip_faces(f, np.ones(len(f), bool)) if mask[0] else f
        assert out["orientable"].all() and np.array_equal(out["faces"], want) and out["inconsistent_edges"][0] == same_direction_edges(g, len(v))


def test_degenerate_faces_are_patches_of_their_own():
    f = np.array([[0, 1, 2], [2, 1, 2], [1, 3, 2], [4, 4, 4], [2, 1, 0]], np.int32)
    v = np.random.default_rng(0).random((5, 3)).astype(np.float32)
    out = OC.orient(f, 5, v)
    # faces 0, 2 and 4 share the edge (1, 2): three times, no link ((2,1,2) would have made it four); 0 and 4 share two more
    assert out["n"] == 4 and out["face_patch"].tolist() == [0, 1, 2, 3, 0] and np.array_equal(out["faces"][[1, 3]], f[[1, 3]])
    assert out["flip"][[1, 3]].tolist() == [0, 0] and out["closed"].tolist() == [False, True, False, True]
    assert out["flip"][0] == out["flip"][4] and not OC.orient(f, 5)["flip"].any()
    assert out["signed_volume"][[1, 3]].tolist() == [0.0, 0.0] and out["closed"][[1, 3]].tolist() == [True, True]
    f = np.array([[0, 1, 2], [2, 1, 2], [1, 2, 3]], np.int32)
    out = OC.orient(f, 4)
    assert out["n"] == 2 and out["face_patch"].tolist() == [0, 1, 0] and out["flip"].tolist() == [0, 0, 1]


# ---- the fixtures' conditions ------------------------------------------------------------------------------------------------
def test_box_is_outward_and_its_volume_exact():
    v, f = OC.box([0, 0, 0], [0.5, 0.25, 1.0])
    out = OC.orient(f, len(v), v)
    assert out["n"] == 1 and out["closed"].all() and not out["flip"].any() and same_direction_edges(f, len(v)) == 0
    assert out["signed_volume"].tolist() == [0.125]
    out = OC.orient(OC.flip_faces(f, np.ones(12, bool)), len(v), v)
    assert out["flip"].all() and np.array_equal(out["faces"], f) and out["signed_volume"].tolist() == [0.125]
    out = OC.orient(OC.flip_faces(f, np.ones(12, bool)), len(v), v, outward=False)
    assert not out["flip"].any() and out["signed_volume"].tolist() == [-0.125]


def test_cubes_on_an_edge_are_two_patches():
    v, f = OC.cubes_on_an_edge()
    t = R.components(f, len(v))
    assert t["n"] == 1 and t["nonmanifold_edges"] == 1
    keys = R.edge_keys(f)
    assert (keys == ((6 << 32) | 7)).sum() == 4
    out = OC.orient(f, len(v), v)
    assert out["n"] == 2 and out["n_faces"].tolist() == [12, 12] and not out["closed"].any() and not out["flip"].any()
    assert out["signed_volume"].tolist() == [1.0, 1.0]


def test_sum_bound_is_small_beside_the_sums():
    """every outward decision of the GPU tests' meshes has |s| at least 1000 bounds"""
    cases = [OC.box([0, 0, 0], [0.5, 0.25, 1.0]), OC.cubes_on_an_edge(), R.icosphere(2)]
    v, _, f = M.marching_cubes(M.two_spheres(64))
    cases.append((v, f))
    for v, f in cases:
        out = OC.orient(OC.random_flips(f, 1)[0], len(v), v)
        assert (np.abs(6 * out["signed_volume"]) >= 1000 * out["s_bound"]).all() and (out["signed_volume"] > 0).all()


# ---- the union/find on the host --------------------------------------------------------------------------------------------
def test_parity_union_find_in_a_host_program(tmp_path):
    """csrc/mesh_topo_common.h compiled by the host compiler with the address and undefined-behaviour sanitizers, run as its own
    process: find_parity / unite_parity / jump_parity on a chain of 4097 faces with random rel, its links ascending, descending,
    bit-reversed and shuffled with 3 seeds, and on cycles of even and of odd total parity"""
    exe = str(tmp_path / "meshorient")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "meshorient_unionfind_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr


# ---- the C-ABI and the python surface ----------------------------------------------------------------------------------------
def test_library_exports_the_new_symbols():
    lib = load_library()
    fns = declared_functions()
    for name in NEW:
        assert name in fns and hasattr(lib, name) and name in cnr_amd._C.SIGNATURES, name
        assert_row_matches(name, cnr_amd._C.SIGNATURES[name], fns[name])
    for name in ("orient", "orient_mesh", "MeshOrientation"):
        assert hasattr(cnr_amd.meshops, name), name


def test_argument_errors_are_return_codes():
    """host pointers and no GPU: sizes outside the contract are refused before anything is read or launched"""
    lib = load_library()
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 2 ** 31
    assert lib.cnr_mesh_orient_keys(p, 0, p, None) == -2 and lib.cnr_mesh_orient_keys(p, big // 3 + 1, p, None) == -2
    assert lib.cnr_mesh_orient_keys(p, 1, None, None) == -1
    assert lib.cnr_mesh_orient_union(p, p, p, 0, p, p, None) == -2 and lib.cnr_mesh_orient_union(p, p, None, 1, p, p, None) == -1
    assert lib.cnr_mesh_orient_flatten(p, 0, p, p, p, p, None) == -2 and lib.cnr_mesh_orient_flatten(p, 4, None, p, p, p, None) == -1
    assert lib.cnr_mesh_orient_check(p, p, p, 4, p, 5, p, p, p, p, None) == -2                     # more patches than faces
    assert lib.cnr_mesh_orient_check(p, p, p, 4, p, 0, p, p, p, p, None) == -2
    assert lib.cnr_mesh_orient_check(p, p, p, 4, p, 1, p, None, p, p, None) == -1
    assert lib.cnr_mesh_orient_stats_workspace_bytes(0) == -2 and lib.cnr_mesh_orient_stats_workspace_bytes(33) == 1024 + 512 + 256
    assert lib.cnr_mesh_orient_stats(p, p, p, p, p, 4, 4, 1, p, p, 1, None, p, p, p, p, None) == -1      # without workspace
    assert lib.cnr_mesh_orient_stats(p, p, p, p, p, 4, 4, 1, p, p, 1, p, p, p, p, None, None) == -1      # verts without signed_volume
    assert lib.cnr_mesh_orient_stats(None, p, p, p, p, 4, 4, 0, p, p, 0, p, p, p, p, None, None) == -2
    assert lib.cnr_mesh_orient_apply(p, 0, p, 1, p, p, p, p, None) == -2 and lib.cnr_mesh_orient_apply(p, 4, p, 1, p, None, p, p, None) == -1


def test_host_tensors_and_bad_options_are_refused():
    with pytest.raises(cnr_amd._C.CnrError):
        cnr_amd.meshops.orient(torch.zeros(4, 3, dtype=torch.int32), 12)
    with pytest.raises(ValueError):
        cnr_amd.meshops.orient(torch.zeros(4, 2, dtype=torch.int32), 12)
    with pytest.raises(ValueError):
        cnr_amd.meshops.orient(torch.zeros(4, 3, dtype=torch.int32), 12, outward=True)
    assert cnr_amd.meshops.parse_clean_options("keep_largest=1,orient=1") == dict(keep_largest=1, orient=True)
    assert cnr_amd.meshops.parse_clean_options("orient=0") == dict(orient=False)
    with pytest.raises(ValueError):
        cnr_amd.meshops.parse_clean_options("orient=maybe")
