"""Point-to-mesh distance without a GPU: the numpy restatement (tests/pointmesh_cpu.py) against an independent formulation and
against closed forms, the fp32 error constant K that the GPU tests' bar uses, the translation property, the face search of
cnr_sample_faces against tests/metric_cpu.py's sampling, the warning-free build and the C-ABI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cnr_amd
import metric_cpu as MC
import pointmesh_cpu as P
from conftest import ROOT
from test_abi import assert_row_matches, declared_functions, load_library

PKG = os.path.join(ROOT, "category-nerf-reconstruction-official_amd")
NEW = ("cnr_point_mesh_workspace_bytes", "cnr_point_mesh_dist", "cnr_point_mesh_pass", "cnr_sample_faces")


def _agree(points, verts, faces=None):
    """closest_f64 against closest_alt_f64: 1e-12 relative to the scale of the pair, d + the winning face's longest edge (a
    distance of 1e-9 m to a face of 1 m is not known to 1e-21 m in either formulation)"""
    d, f, _, _ = P.closest_f64(points, verts, faces)
    da, fa = P.closest_alt_f64(points, verts, faces)
    L = P.longest_edge(verts, faces, f)
    assert np.isfinite(d).all() and np.isfinite(da).all()
    assert (np.abs(d - da) <= 1e-12 * (d + L)).all(), float(np.max(np.abs(d - da) / (d + L)))
    return d, f


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,F", [c for c in P.BIT_CASES if c[0] * c[1] <= 600000])
def test_f64_restatement_equals_the_independent_formulation_on_random_triangles(nq, F):
    q, v, f = P.random_case(nq, F)
    _agree(q, v, f)
    _agree(q, P.soup(v, f))


def test_f64_restatement_equals_the_independent_formulation_on_slivers():
    """needle and cap slivers down to a height of 1e-6 of the base, and exactly degenerate faces among them"""
    rng = np.random.default_rng(11)
    F = 300
    a = rng.uniform(0, 4, (F, 3))
    e = rng.normal(size=(F, 3))
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    p = np.cross(e, rng.normal(size=(F, 3)))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    h = 10.0 ** rng.uniform(-6, -1, (F, 1))
    s = rng.uniform(-0.5, 1.5, (F, 1))                                  # the apex over, before or past the base
    tri = np.stack([a, a + e, a + s * e + h * p], 1).astype(np.float32)
    q = np.concatenate([rng.uniform(-1, 5, (150, 3)), tri.astype(np.float64).mean(1)[:150] + rng.normal(size=(150, 3)) * 1e-3])
    _agree(q.astype(np.float32), tri.reshape(-1, 3))
    qd, vd, fd, _ = P.degenerate_mesh()
    _agree(qd, vd, fd)


def test_the_seven_regions_of_a_dyadic_triangle_are_exact():
    verts = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float32)
    cases = [((-3, -4, 0), (0, 0, 0), 5.0),         # vertex a
             ((7, -4, 0), (4, 0, 0), 5.0),          # vertex b
             ((-4, 7, 0), (0, 4, 0), 5.0),          # vertex c
             ((2, -3, 0), (2, 0, 0), 3.0),          # edge ab
             ((-3, 2, 0), (0, 2, 0), 3.0),          # edge ac
             ((4, 4, 1), (2, 2, 0), 3.0),           # edge bc
             ((1, 1, 2), (1, 1, 0), 2.0)]           # interior
    q = np.array([c[0] for c in cases], np.float32)
    want_c = np.array([c[1] for c in cases], np.float64)
    want_d = np.array([c[2] for c in cases])
    for fn in (P.closest_f32, P.closest_f64):
        d, f, c, d2 = fn(q, verts)
        assert np.array_equal(d.astype(np.float64), want_d) and np.array_equal(c.astype(np.float64), want_c)
        assert np.array_equal(d2.astype(np.float64), want_d ** 2) and (f == 0).all()
    da, _ = P.closest_alt_f64(q, verts)
    assert np.array_equal(da, want_d)
    # the same triangle with its corners rotated: every region once more under another name
    for k in (1, 2):
        d, _, c, _ = P.closest_f32(q, np.roll(verts, k, 0))
        assert np.array_equal(d.astype(np.float64), want_d) and np.array_equal(c.astype(np.float64), want_c)


def test_degenerate_faces_stand_for_their_segment_or_point():
    q, verts, faces, is_deg = P.degenerate_mesh()
    t = P.corners(verts, faces)
    assert is_deg.sum() == 12
    d32, f32, c32, _ = P.closest_f32(q, verts, faces)
    d64, f64, _, _ = P.closest_f64(q, verts, faces)
    assert np.isfinite(d32).all() and np.isfinite(c32).all()
    won = is_deg[f64]
    assert won.sum() >= 40 and (~won).sum() >= 10
    # the fp64 distance to the segment (or point) the face covers: the minimum over its three edge segments
    p = q.astype(np.float64)[won, None, :]
    tw = t[f64[won]]
    seg = np.minimum(np.minimum(P._segment_d2(p, tw[None, :, 0], tw[None, :, 1]), P._segment_d2(p, tw[None, :, 1], tw[None, :, 2])),
                     P._segment_d2(p, tw[None, :, 2], tw[None, :, 0]))
    want = np.sqrt(seg[np.arange(won.sum()), np.arange(won.sum())])
    L = P.longest_edge(verts, faces, f64[won])
    assert (np.abs(d64[won] - want) <= 1e-12 * (want + L)).all()
    assert (np.abs(d32[won].astype(np.float64) - want) <= P.bar(want, L, 4 * P.K_F32)).all()
    assert (d64[-36:] <= 1e-12).all() and won[-36:].all()               # the degenerate faces' own corners lie on them


# ---- the fp32 error constant -----------------------------------------------------------------------------------------------
def test_fp32_error_constant_on_the_gpu_tests_cases():
    """K = max |d32 - d64| / (2^-24 (d64 + L)) over every query of the GPU tests' random cases (L: the longest edge of the
    face that wins in fp64), measured from the restatement alone: P.K_F32 states it, the GPU bar is 4 K."""
    worst = 0.0
    for nq, F in P.BIT_CASES:
        q, v, f = P.random_case(nq, F)
        d32 = P.closest_f32(q, v, f)[0].astype(np.float64)
        d64, f64, _, _ = P.closest_f64(q, v, f)
        k = np.abs(d32 - d64) / (2.0 ** -24 * (d64 + P.longest_edge(v, f, f64)))
        print("K over (%d, %d): %.3f" % (nq, F, k.max()))
        worst = max(worst, float(k.max()))
    print("K = %.4f" % worst)
    assert 0.9 * P.K_F32 <= worst <= P.K_F32


# ---- translation -----------------------------------------------------------------------------------------------------------
def test_translation_changes_no_bit_of_the_restatement():
    q, v = P.grid_scene()
    assert np.array_equal(q * 4096, np.round(q * 4096)) and np.array_equal(v * 4096, np.round(v * 4096))
    qs, vs = q + P.GRID_SHIFT, v + P.GRID_SHIFT
    assert np.array_equal(qs.astype(np.float64), q.astype(np.float64) + P.GRID_SHIFT)       # the shift itself is exact
    a, b = P.closest_f32(q, v), P.closest_f32(qs, vs)
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])
    assert (a[3] == 0).sum() >= 100 and (a[3] > 0).sum() >= 100


def test_ties_go_to_the_lowest_face_in_the_restatement():
    q = P.cube_tie_queries()
    d, f, _, d2 = P.closest_f32(q, P.CUBE_VERTS, P.CUBE_FACES)
    pairs = P._pairs(q, P.face_records(P.corners(P.CUBE_VERTS, P.CUBE_FACES, np.float32)))[0]
    ties = (pairs == d2[:, None]).sum(1)
    assert (ties >= 2).all() and ties[0] == 6                           # vertex 0 lies on 6 faces
    assert np.array_equal(f, np.argmax(pairs == d2[:, None], axis=1))
    d_twice, f_twice, _, _ = P.closest_f32(q, np.concatenate([P.CUBE_VERTS, P.CUBE_VERTS]),
                                           np.concatenate([P.CUBE_FACES, P.CUBE_FACES + 8]))
    assert np.array_equal(f_twice, f) and np.array_equal(d_twice, d)


# ---- the face search -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["many", "one", "random"])
def test_sample_faces_is_the_face_of_the_sampling_restatement(which):
    if which == "random":
        v, f, us = MC.sampling_random_inputs()
        tri, u = MC.triangles(v, f), us[0]
    else:
        verts, u = MC.dyadic_sampling_fixture() if which == "many" else MC.dyadic_single_face()
        tri = MC.triangles(verts)
    face, _, cum = MC.sample_surface(tri, u)
    assert np.array_equal(P.sample_faces(cum, u[:, 0]), face)
    if which == "many":
        areas = MC.face_areas(tri)
        # a zero-area face is drawn by u0 = 0 alone (the fixture's first face has no area: cum[0] = 0 >= 0)
        assert (areas == 0).sum() == 5 and ((areas[face] == 0) == (u[:, 0] == 0)).all()
        on = np.isin(u[:, 0] * cum[-1], cum)
        assert on.sum() >= 8 and u[:, 0].min() == 0.0                                        # draws on the boundaries, and u0 = 0


# ---- build and ABI ---------------------------------------------------------------------------------------------------------
def test_point_mesh_build_is_warning_free():
    """csrc/point_mesh.hip and csrc/metric.hip (which gained cnr_sample_faces), with the Makefile's compiler and flags plus
    -Werror, into a temporary directory"""
    import tempfile
    csrc = os.path.join(PKG, "csrc")
    cmd = subprocess.run(["make", "-s", "-C", csrc, "--no-print-directory", "--eval",
                          "print-compile: ; @echo $(HIPCC) $(CXXFLAGS)", "print-compile"],
                         capture_output=True, text=True, check=True).stdout.split()
    with tempfile.TemporaryDirectory() as d:
        for unit in ("point_mesh", "metric"):
            out = subprocess.run(cmd + ["-Werror", "-c", os.path.join(csrc, unit + ".hip"), "-o", os.path.join(d, unit + ".o")],
                                 capture_output=True, text=True)
            assert out.returncode == 0, out.stderr
            assert "warning" not in (out.stdout + out.stderr).lower(), out.stderr


def test_library_exports_the_new_symbols():
    lib = load_library()
    fns = declared_functions()
    for name in NEW:
        assert name in fns and hasattr(lib, name) and name in cnr_amd._C.SIGNATURES, name
        assert_row_matches(name, cnr_amd._C.SIGNATURES[name], fns[name])
    assert "cnr_point_mesh_workspace_bytes" in cnr_amd._C._RESTYPE64
    assert not any(n in cnr_amd._C._RESTYPE64 for n in NEW[1:])
    for name in ("point_mesh_distance", "sample_surface_faces", "calc_3d_metric_surface"):
        assert hasattr(cnr_amd.metrics, name) and name in cnr_amd.metrics.__all__, name
    for name in ("deviation", "deviation_mesh"):
        assert hasattr(cnr_amd.meshops, name), name


def test_argument_errors_are_return_codes():
    lib = load_library()
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 2 ** 31
    assert lib.cnr_point_mesh_workspace_bytes(0, 5) == -2 and lib.cnr_point_mesh_workspace_bytes(5, 0) == -2
    assert lib.cnr_point_mesh_workspace_bytes(5, big) == -2 and lib.cnr_point_mesh_workspace_bytes(5, big - 1) > 0
    assert lib.cnr_point_mesh_dist(None, 4, p, None, 4, p, p, None, p, None) == -1
    assert lib.cnr_point_mesh_dist(p, 4, p, None, 4, p, p, None, None, None) == -1
    assert lib.cnr_point_mesh_dist(p, 0, p, None, 4, p, p, None, p, None) == -2
    assert lib.cnr_point_mesh_dist(p, 4, p, None, 0, p, p, None, p, None) == -2
    assert lib.cnr_point_mesh_dist(p, 4, p, None, big, p, p, None, p, None) == -2
    assert lib.cnr_point_mesh_pass(p, 4, p, None, 4, p, p, None, p, 0, None) == -1
    assert lib.cnr_point_mesh_pass(p, 4, p, None, 4, p, p, None, p, 4, None) == -1
    assert lib.cnr_sample_faces(None, 4, p, 4, p, None) == -1 and lib.cnr_sample_faces(p, 0, p, 4, p, None) == -2
    assert lib.cnr_sample_faces(p, big, p, 4, p, None) == -2 and lib.cnr_sample_faces(p, 4, p, -1, p, None) == -2
    assert lib.cnr_sample_faces(p, 4, p, 0, p, None) == 0                                    # nothing to do: nothing launched


def test_workspace_size_states_the_chunk_count():
    """bytes = align256(64 F) + chunks align256(8 nq), chunks from the documented rule: query blocks of 1024, tiles of 256
    faces, about 2048 workgroups"""
    lib = load_library()
    for nq, F in P.BIT_CASES + (P.LARGE_CASE, (200000, 442700), (200000, 30258), (1, 70000), (5000000, 300)):
        got = lib.cnr_point_mesh_workspace_bytes(nq, F)
        assert got == P.align256(64 * F) + P.chunk_count(nq, F) * P.align256(8 * nq), (nq, F)
        assert P.workspace_chunks(nq, F, got) == P.chunk_count(nq, F)
    assert P.chunk_count(100, 2000) >= 3 and P.chunk_count(1, 1) == 1 and P.chunk_count(200000, 442700) == 11
