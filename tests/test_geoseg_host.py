"""CPU: ScanNet mask refinement without a GPU -- the restatement tests/geoseg_cpu.py against
scipy.ndimage (labelling, hole filling, morphology) and against what the reference's refine_inst_data recorded; the synthetic
scenes; the union/find helpers of csrc/ccl_common.h in a stand-alone host program; and the C-ABI of the new entry points."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import scipy.ndimage as ndi

import geoseg_cpu as G
from conftest import GOLDEN, ROOT
from test_abi import assert_row_matches, declared_functions, load_library

NEW = ("cnr_geoseg_maps", "cnr_geoseg_edge_map", "cnr_ccl", "cnr_label_counts", "cnr_geoseg_grow", "cnr_fill_holes_workspace_bytes",
       "cnr_fill_holes", "cnr_refine_vote", "cnr_refine_apply")
CSRC = os.path.join(ROOT, "category-nerf-reconstruction-official_amd", "csrc")


@pytest.fixture(scope="module")
def cnr():
    import cnr_amd
    return cnr_amd


@pytest.fixture(scope="module")
def lib():
    return load_library()


def same_partition(a, b):
    """two label images name the same components (-1 / 0 = background)"""
    fa, fb = a.ravel() >= 0, b.ravel() > 0
    if not np.array_equal(fa, fb):
        return False
    pairs = np.unique(np.stack([a.ravel()[fa], b.ravel()[fa]]), axis=1)
    return len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1]))


# ---- the restatement against scipy ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
def test_restated_labelling_is_scipys_up_to_names(connectivity):
    structure = np.ones((3, 3)) if connectivity == 8 else None
    for name, m in G.ccl_masks().items():
        got = G.ccl(m, connectivity)
        want, n = ndi.label(m, structure=structure)
        assert same_partition(got, want), name
        roots = np.unique(got[got >= 0])
        assert len(roots) == n, name
        for r in roots:                                           # the name of a component is its first pixel in raster order
            assert np.flatnonzero(got.ravel() == r)[0] == r, name
    H, W = 70, 45
    board = G.ccl_masks(H, W)["checkerboard"]
    assert len(np.unique(G.ccl(board, 8))) == 2                   # -1 and one component
    assert np.array_equal(G.ccl(board, 4).ravel()[board.ravel() != 0], np.flatnonzero(board.ravel()))     # none merged
    for name in ("spiral", "serpentine", "u_shapes", "frame_ring"):
        n = len(np.unique(G.ccl(G.ccl_masks()[name], 4))) - 1
        assert n == (2 if name == "frame_ring" else 1), (name, n)
    batch = np.stack([G.ccl_masks()[k] for k in ("spiral", "random_half", "zeros")])
    assert np.array_equal(G.ccl(batch, 8)[1], G.ccl(batch[1], 8))
    assert np.array_equal(G.label_counts(G.ccl(batch[1], 8)).ravel()[G.ccl(batch[1], 8)[batch[1] != 0]] > 0, np.ones(int(batch[1].sum()), bool))


def test_restated_fill_is_binary_fill_holes():
    masks = dict(G.fill_masks())
    masks.update({k: v for k, v in G.ccl_masks().items() if v.shape == (70, 45)})
    for name, m in masks.items():
        assert np.array_equal(G.fill_holes(m), ndi.binary_fill_holes(m)), name
    f = G.fill_masks()
    assert G.fill_holes(f["diagonal"])[1:5, 1:5].all() and not G.fill_holes(f["diagonal"])[0, 0]
    assert not G.fill_holes(f["open"])[10:25, 10:25].any()
    assert G.fill_holes(f["nested"])[2:38, 2:50].all()


def test_restated_morphology_is_scipys():
    rng = np.random.default_rng(3)
    a = rng.random((37, 29)).astype(np.float32)
    a[rng.random(a.shape) < 0.2] = 0
    assert np.array_equal(G.erode3(a), ndi.grey_erosion(a, size=(3, 3), mode="constant", cval=np.inf))
    assert np.array_equal(G.dilate3(a), ndi.grey_dilation(a, size=(3, 3), mode="constant", cval=-np.inf))
    b = (rng.random((37, 29)) < 0.6).astype(np.uint8)
    assert np.array_equal(G.erode3(b), ndi.grey_erosion(b.astype(np.float32), size=(3, 3), mode="constant", cval=np.inf).astype(np.uint8))
    assert np.array_equal(G.dilate3(b), ndi.grey_dilation(b.astype(np.float32), size=(3, 3), mode="constant", cval=-np.inf).astype(np.uint8))
    i = np.arange(-2, 9)
    assert G.reflect101(i, 7).tolist() == [2, 1, 0, 1, 2, 3, 4, 5, 6, 5, 4]


def test_colormap_is_pascal_voc(cnr):
    c = G.label_colormap()
    assert c[:6].tolist() == [[0, 0, 0], [128, 0, 0], [0, 128, 0], [128, 128, 0], [0, 0, 128], [128, 0, 128]]
    assert c[8].tolist() == [64, 0, 0] and c[255].tolist() == [224, 224, 192]
    assert np.array_equal(cnr.utils.label_colormap(), c)


# ---- the vote against the reference's recorded outputs --------------------------------------------------------------------
def test_restated_vote_equals_the_reference():
    z = np.load(os.path.join(GOLDEN, "geoseg", "refine_cases.npz"))
    cases = G.refine_cases()
    assert sorted({k.split("__")[0] for k in z.files}) == sorted(cases)
    for name, (inst, masks) in cases.items():
        assert np.array_equal(z[name + "__inst"], inst) and np.array_equal(z[name + "__masks"], masks), name
        got = G.refine_inst_data(inst, list(masks))
        assert got.dtype == z[name + "__refined"].dtype and np.array_equal(got, z[name + "__refined"]), name
    assert not z["rate_equal__refined"].any() and not z["no_objects__refined"].any()
    assert (z["rate_above__refined"] == 4).sum() == 100
    r = z["overlap_later_wins__refined"]
    assert (r[cases["overlap_later_wins"][1][1]] == 6).all()
    assert set(np.unique(z["ring_swallows_island__refined"])) == {0, 6} and 4 in z["island_after_ring__refined"]
    assert (z["diagonal_hole__refined"][1:5, 1:5] == 7).all()


# ---- the scenes ---------------------------------------------------------------------------------------------------------------
def test_scene_boxes_through_the_restatement():
    s = G.scene_boxes()
    seg = G.segmentation(s["P"], s["N"], s["depth"], G.BOXES_MIN, G.BOXES_MIN)
    assert len(seg["masks"]) == 3                                    # wall, A, B
    wall, a, b = seg["masks"]
    assert wall[0, 0] and a[30, 25] and b[40, 70]
    refined = G.refine_inst_data(s["inst"], seg["masks"])
    assert set(np.unique(refined)) <= {0, G.ID_A, G.ID_B} and (refined == G.ID_A).any() and (refined == G.ID_B).any()
    assert (s["inst"] == G.ID_POSTER).sum() >= 400 and not (refined == G.ID_POSTER).any()     # the poster is gone
    for ident, true in ((G.ID_A, s["A"]), (G.ID_B, s["B"])):
        got = refined == ident
        inner = ndi.binary_erosion(true, structure=np.ones((3, 3)), iterations=2)
        outer = ndi.binary_dilation(true, structure=np.ones((3, 3)), iterations=4)
        assert got[inner].all() and not got[~outer].any(), ident
    assert np.array_equal(seg["output"][a][0], G.label_colormap()[1]) and not seg["output"][~(wall | a | b)].any()


def test_scene_room_exercises_both_maps():
    s = G.scene_room()
    valid = s["depth"] > 0
    assert (~valid).sum() == 24
    for side in (s["depth"][0], s["depth"][-1], s["depth"][:, 0], s["depth"][:, -1]):
        assert (side > 0).sum() >= len(side) - 3                     # surfaces run off all four image borders
    disc, conv = G.maps(s["P"], s["N"], s["depth"])
    for name, m in (("disc", disc), ("conv", conv)):
        share = m[valid].mean()
        print(name, "set on", share, "of the valid pixels")
        assert 0.05 <= share <= 0.95, (name, share)
    seg = G.segmentation(s["P"], s["N"], s["depth"], G.BOXES_MIN, G.BOXES_MIN)
    assert len(seg["masks"]) >= 1 and (seg["edge"] == 0)[valid].any() and (seg["grown"] != seg["kept"]).any()


# ---- the union/find helpers on the host ------------------------------------------------------------------------------------
def test_union_find_helpers_in_a_host_program(tmp_path):
    """csrc/ccl_common.h compiled by the host compiler with the address and undefined-behaviour sanitizers: the kernels' three
    phases on adversarial masks, the per-thread work in three different orders, against a flood fill"""
    exe = str(tmp_path / "unionfind")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "geoseg_unionfind_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_symbols(cnr, lib):
    fns = declared_functions()
    for name in NEW:
        assert name in fns and hasattr(lib, name) and name in cnr._C.SIGNATURES, name
        assert_row_matches(name, cnr._C.SIGNATURES[name], fns[name])
    for name in ("geometry_segmentation", "refine_inst_data", "Segment", "connected_components", "fill_holes"):
        assert hasattr(cnr.utils, name), name


def test_argument_errors_are_return_codes(lib):
    """host pointers and no GPU: H = 0, connectivity = 5 and K < 0 are refused before anything is read or launched"""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.cnr_geoseg_maps(p, p, p, 0, 8, p, p, None) == -2
    assert lib.cnr_geoseg_maps(p, p, p, 8, 2, p, p, None) == -2            # the reflected 5x5 window needs three pixels
    assert lib.cnr_geoseg_maps(None, p, p, 8, 8, p, p, None) == -1
    assert lib.cnr_geoseg_edge_map(p, p, p, 0, 8, p, None) == -2
    assert lib.cnr_geoseg_edge_map(p, p, p, 8, 8, None, None) == -1
    assert lib.cnr_ccl(p, 1, 0, 8, 8, p, p, None) == -2
    assert lib.cnr_ccl(p, 1, 8, 8, 5, p, p, None) == -2
    assert lib.cnr_ccl(p, 0, 8, 8, 4, p, p, None) == -2
    assert lib.cnr_ccl(p, 1, 65536, 65536, 4, p, p, None) == -2            # H W beyond int32
    assert lib.cnr_ccl(p, 1, 8, 8, 8, p, None, None) == -1
    assert lib.cnr_label_counts(p, 1, 0, 8, p, None) == -2
    assert lib.cnr_label_counts(None, 1, 8, 8, p, None) == -1
    assert lib.cnr_geoseg_grow(p, p, p, p, None, 0, 0, 8, p, None) == -2
    assert lib.cnr_geoseg_grow(p, p, p, None, None, 0, 8, 8, p, None) == -1
    assert lib.cnr_fill_holes_workspace_bytes(-1, 8, 8) == -2 and lib.cnr_fill_holes_workspace_bytes(1, 0, 8) == -2
    assert lib.cnr_fill_holes_workspace_bytes(3, 10, 7) >= 3 * 70 * 5 and lib.cnr_fill_holes_workspace_bytes(0, 10, 7) == 0
    assert lib.cnr_fill_holes(None, None, p, -1, 8, 8, p, p, p, None) == -2
    assert lib.cnr_fill_holes(None, None, p, 1, 0, 8, p, p, p, None) == -2
    assert lib.cnr_fill_holes(p, p, p, 1, 8, 8, p, p, p, None) == -1         # labels AND masks
    assert lib.cnr_fill_holes(None, None, None, 1, 8, 8, p, p, p, None) == -1
    assert lib.cnr_refine_vote(p, p, p, -1, 1, 8, 8, p, None) == -2
    assert lib.cnr_refine_vote(p, p, p, 1, 1, 0, 8, p, None) == -2
    assert lib.cnr_refine_vote(p, p, p, 1, 2049, 8, 8, p, None) == -2
    assert lib.cnr_refine_vote(p, None, p, 1, 1, 8, 8, p, None) == -1
    assert lib.cnr_refine_apply(p, p, p, -1, 1, 8, 8, 0.7, p, p, None) == -2
    assert lib.cnr_refine_apply(p, p, p, 1, 1, 8, 0, 0.7, p, p, None) == -2
    assert lib.cnr_refine_apply(p, p, p, 1, 1, 8, 8, 0.7, p, None, None) == -1


def test_host_tensors_are_refused(cnr):
    import torch
    with pytest.raises(cnr._C.CnrError):
        cnr.utils.connected_components(torch.zeros(4, 4, dtype=torch.uint8))
    with pytest.raises(cnr._C.CnrError):
        cnr.utils.fill_holes(torch.zeros(4, 4, dtype=torch.uint8))
