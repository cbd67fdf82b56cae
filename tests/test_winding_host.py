"""The generalized winding number without a GPU: the numpy restatement (tests/winding_cpu.py) against the same formula in mpmath
at 40 digits, against an independent formulation and against closed forms; what a few ulp in the lengths do; the det == 0
rule; the orientation rule; the warning-free build and the C-ABI of csrc/winding.hip.

The bar of a query (winding_cpu.bar) always comes from the restatement."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import cnr_amd
import winding_cpu as W
from conftest import ROOT
from test_abi import assert_row_matches, declared_functions, load_library

PKG = os.path.join(ROOT, "category-nerf-reconstruction-official_amd")
NEW = ("cnr_winding_workspace_bytes", "cnr_winding_number")
MP_CASES = ((63, 65), (65, 257), (2049, 1000), (100, 2000))


@functools.lru_cache(maxsize=None)
def _case(nq, F):
    q, v, f = W.random_case(nq, F)
    w, bar = W.winding_f64(q, v, f, with_bar=True)
    for arr in (q, v, f, w, bar):
        arr.setflags(write=False)
    return q, v, f, w, bar


# ---- the restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,F", MP_CASES + (("degenerate", None),))
def test_restatement_is_within_the_bar_of_forty_digits(nq, F):
    pytest.importorskip("mpmath")
    if nq == "degenerate":
        q, v, f, _ = W.degenerate_mesh()
        w, bar = W.winding_f64(q, v, f, with_bar=True)
    else:
        q, v, f, w, bar = _case(nq, F)
        q, w, bar = q[:60], w[:60], bar[:60]                            # the batch's values (its chunk length), 60 of them
    err = np.abs(w - W.winding_mp(q, v, f))
    print("max |f64 - mp| %.3g, %.4f of the bar, bar <= %.3g" % (err.max(), (err / bar).max(), bar.max()))
    assert (bar > 0).all() and (err <= bar).all(), float((err / bar).max())


@pytest.mark.parametrize("nq,F", [("degenerate", None)] + [c for c in W.BIT_CASES])
def test_restatement_equals_the_independent_formulation(nq, F):
    if nq == "degenerate":
        q, v, f, _ = W.degenerate_mesh()
        w = W.winding_f64(q, v, f)
    else:
        q, v, f, w, _ = _case(nq, F)
    err = np.abs(w - W.winding_alt_f64(q, v, f))
    print("max |f64 - alt| %.3g" % err.max())
    assert np.isfinite(w).all() and (err <= 1e-11).all(), float(err.max())
    assert np.array_equal(W.winding_f64(q, W.soup(v, f)), w)


@pytest.mark.parametrize("nq,F", MP_CASES)
def test_an_ulp_in_the_three_lengths_stays_within_half_the_bar(nq, F):
    q, v, f, w, bar = _case(nq, F)
    moved = W.winding_f64(q, v, f, lengths=W.ulp_lengths(nq + F))
    ratio = np.abs(moved - w) / bar
    print("max %.4f of the bar, max |dw| %.3g" % (ratio.max(), np.abs(moved - w).max()))
    assert (moved != w).any() and (ratio <= 0.5).all(), float(ratio.max())


def test_closed_forms_on_the_unit_cube():
    q = W.cube_tie_queries()
    want = W.cube_expected()
    assert len(q) == 46 == len(want)
    w = W.winding_f64(q, W.CUBE_VERTS, W.CUBE_FACES)
    print("max error %.3g" % np.abs(w - want).max())
    assert (np.abs(w - want) <= 1e-12).all()
    centre = np.full((1, 3), 0.5, np.float32)
    assert abs(W.winding_f64(centre, W.CUBE_VERTS, W.CUBE_FACES)[0] - 1.0) <= 1e-12
    both = np.concatenate([q, centre])
    flipped = W.winding_f64(both, W.CUBE_VERTS, W.flipped(W.CUBE_FACES))
    assert (np.abs(flipped + np.concatenate([want, [1.0]])) <= 1e-12).all()
    alt = W.winding_alt_f64(both, W.CUBE_VERTS, W.CUBE_FACES)
    assert (np.abs(alt - np.concatenate([want, [1.0]])) <= 1e-12).all()


def test_a_query_in_the_plane_of_a_triangle_gets_exactly_zero():
    verts = np.array([[0, 0, 0.5], [4, 0, 0.5], [0, 4, 0.5]], np.float32)
    q = np.array([[1, 1, 0.5], [0.25, 3, 0.5], [2, 2, 0.5], [0, 0, 0.5], [2, 0, 0.5],       # inside, on an edge, on corners
                  [5, 5, 0.5], [-1, 1, 0.5], [3, 3, 0.5], [8, 0, 0.5]], np.float32)         # outside, on an edge's line
    for v in (verts, verts[::-1].copy()):
        w = W.winding_f64(q, v)
        assert np.array_equal(w, np.zeros(len(q))) and not np.signbit(w).any()
    t, det, den, _ = W.pair_terms(q.astype(np.float64), W.corners(verts))
    assert (det == 0).all() and (den[:3, 0] < 0).sum() >= 1             # atan2 alone would have said +-pi inside the triangle
    above = W.winding_f64(q[:1] + np.float32([0, 0, 2.0 ** -20]), verts)[0]
    assert abs(abs(above) - 0.5) < 1e-5                                 # a hair off the plane: half of the sphere


def test_sphere_fixture_and_its_open_form():
    v, f = W.uv_sphere()
    vo, fo = W.open_sphere()
    assert len(f) == 960 and 0 < len(fo) < 960
    w = W.winding_f64(np.array([[0, 0, 0], [0.3, -0.2, 0.5], [1.2, 0, 0]], np.float32), v, f)
    assert (np.abs(w - [1, 1, 0]) <= 1e-12).all()
    wo = W.winding_f64(np.array([[0, 0, 0], [0, 0, 3.0]], np.float32), vo, fo)
    assert 0.5 < wo[0] < 1 and abs(wo[1]) < 0.1                         # the hole lets some of the sphere out


def test_mesh_orientation_rule():
    from cnr_amd import metrics
    v, f = W.uv_sphere()
    vo, fo = W.open_sphere()
    for verts, faces, want in ((W.CUBE_VERTS, W.CUBE_FACES, 1), (W.CUBE_VERTS, W.flipped(W.CUBE_FACES), -1), (v, f, 1),
                               (vo, fo, 1), (vo, W.flipped(fo), -1), (W.soup(vo, W.flipped(fo)), None, -1)):
        assert W.mesh_orientation(verts, faces) == want
        tv = torch.from_numpy(verts)
        tf = None if faces is None else torch.from_numpy(faces)
        vol = float(metrics._signed_volume(tv, tf))                     # the package's own sum, here on host tensors
        assert (1 if vol >= 0 else -1) == want and abs(vol - W.signed_volume(verts, faces)) <= 1e-12 * abs(vol)
    assert abs(W.signed_volume(W.CUBE_VERTS, W.CUBE_FACES) - 6.0) <= 1e-12
    assert metrics._orientation_sign("outward", None) == 1 and metrics._orientation_sign("inward", None) == -1
    with pytest.raises(ValueError):
        metrics._orientation_sign("sideways", None)


def test_volume_iou_draw_is_within_four_sigma_on_the_restatement():
    """the explicit points of the GPU test, classified by the restatement: the analytic counts, and an IoU within 4 sigma"""
    delta = 2.0 ** -5
    (va, fa), (vb, fb) = W.concentric_cubes(delta)
    p = W.iou_points()
    x = p.astype(np.float64)
    in_a = ((x > 0) & (x < 1)).all(1)
    in_b = ((x > -delta) & (x < 1 + delta)).all(1)
    assert np.array_equal(W.winding_f64(p, va, fa) > 0.5, in_a)
    assert np.array_equal(-W.winding_f64(p, vb, fb) > 0.5, in_b) and W.mesh_orientation(vb, fb) == -1
    closed = 1.0 / (1 + 2 * delta) ** 3
    union = int((in_a | in_b).sum())
    sigma = np.sqrt(closed * (1 - closed) / union)
    iou = (in_a & in_b).sum() / union
    print("iou %.5f, closed form %.5f, %.2f sigma" % (iou, closed, abs(iou - closed) / sigma))
    assert abs(closed - 0.83371) < 5e-6 and abs(iou - closed) <= 4 * sigma


def test_points_drawn_in_an_oriented_box_lie_in_box_planes_half_spaces():
    """volume_iou's box=(transform, extents) is the box box_planes(transform, extents) describes: every drawn point on the inner
    side of its six planes (to fp32 rounding of a coordinate of about 1), and the draw reaches every one of them"""
    from cnr_amd import metrics
    T, ext = W.rotated_box()
    u = np.random.default_rng(4).random((4000, 3))
    p, volume = metrics._box_points(u, (T, ext), ())
    assert p.dtype == np.float32 and p.shape == (4000, 3) and abs(volume - float(np.prod(ext))) <= 1e-15
    planes = metrics.box_planes(T, ext)
    depth = ((p.astype(np.float64)[:, None, :] - planes[None, :, :3]) * planes[None, :, 3:]).sum(-1)      # (n, 6), inward
    assert (depth >= -1e-6).all(), float(depth.min())
    assert (depth.min(0) < 0.01 * np.repeat(ext, 2)).all() and (np.abs(p.mean(0) - [0.7, -0.4, 1.1]) < 0.03).all()
    # and the axis-aligned default: the box of all the meshes' vertices
    a = metrics.DeviceMesh(torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 2, 0]]), None)
    b = metrics.DeviceMesh(torch.tensor([[-1.0, 0, 0.5], [0, 0, 3], [0, 1, 0]]), None)
    p, volume = metrics._box_points(u, None, (a, b))
    assert volume == 2 * 2 * 3 and np.array_equal(p, W.box_draw([-1, 0, 0], [1, 2, 3], 4000, 4))


# ---- build and ABI -------------------------------------------------------------------------------------------------------------
def test_winding_build_is_warning_free():
    """csrc/winding.hip with the Makefile's compiler and flags plus -Werror, into a temporary directory"""
    import tempfile
    csrc = os.path.join(PKG, "csrc")
    cmd = subprocess.run(["make", "-s", "-C", csrc, "--no-print-directory", "--eval",
                          "print-compile: ; @echo $(HIPCC) $(CXXFLAGS)", "print-compile"],
                         capture_output=True, text=True, check=True).stdout.split()
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run(cmd + ["-Werror", "-c", os.path.join(csrc, "winding.hip"), "-o", os.path.join(d, "winding.o")],
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        assert "warning" not in (out.stdout + out.stderr).lower(), out.stderr


def test_library_exports_the_new_symbols():
    lib = load_library()
    fns = declared_functions()
    for name in NEW:
        assert name in fns and hasattr(lib, name) and name in cnr_amd._C.SIGNATURES, name
        assert_row_matches(name, cnr_amd._C.SIGNATURES[name], fns[name])
    assert "cnr_winding_workspace_bytes" in cnr_amd._C._RESTYPE64 and "cnr_winding_number" not in cnr_amd._C._RESTYPE64
    for name in ("winding_number", "mesh_orientation", "inside", "signed_distance", "volume_iou"):
        assert hasattr(cnr_amd.metrics, name) and name in cnr_amd.metrics.__all__, name


def test_argument_errors_are_return_codes():
    lib = load_library()
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 2 ** 31
    assert lib.cnr_winding_workspace_bytes(0, 5) == -2 and lib.cnr_winding_workspace_bytes(5, 0) == -2
    assert lib.cnr_winding_workspace_bytes(5, big) == -2 and lib.cnr_winding_workspace_bytes(5, big - 1) > 0
    assert lib.cnr_winding_number(None, 4, p, None, 4, p, p, None) == -1
    assert lib.cnr_winding_number(p, 4, None, None, 4, p, p, None) == -1
    assert lib.cnr_winding_number(p, 4, p, None, 4, None, p, None) == -1
    assert lib.cnr_winding_number(p, 4, p, None, 4, p, None, None) == -1
    assert lib.cnr_winding_number(p, 0, p, None, 4, p, p, None) == -2
    assert lib.cnr_winding_number(p, 4, p, None, 0, p, p, None) == -2
    assert lib.cnr_winding_number(p, 4, p, None, big, p, p, None) == -2


def test_workspace_size_states_the_chunk_count():
    """bytes = chunks align256(8 nq), chunks from the documented rule: query blocks of 512, tiles of 256 faces, about 2048
    workgroups"""
    lib = load_library()
    for nq, F in W.BIT_CASES + ((4096, 50000), (200000, 442700), (200000, 30258), (1, 70000), (5000000, 300)):
        got = lib.cnr_winding_workspace_bytes(nq, F)
        assert got == W.chunk_count(nq, F) * W.align256(8 * nq), (nq, F)
        assert W.workspace_chunks(nq, F, got) == W.chunk_count(nq, F)
    assert W.chunk_count(100, 2000) >= 3 and W.chunk_count(1, 1) == 1 and W.chunk_count(200000, 442700) == 6
