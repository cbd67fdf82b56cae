"""GPU: mesh simplification (csrc/mesh_simplify.hip, cnr_amd.meshops.simplify / vertex_normals) against
the numpy restatement tests/meshsimplify_cpu.py, whose own correctness and whose fixtures' conditions
tests/test_meshsimplify_host.py proves without a GPU.  Integer outputs are EQUAL to the restatement, the quadric and position
sums and the errors of the "mean" and "representative" placements bit-equal to it (the same order of operations, contraction
off), the "quadric" positions within one fp32 unit in the last place (both sides compute in fp64, far below that; only a value
on an fp32 rounding boundary can land on either side).  Fixtures that are not built away from the cell boundaries are compared
through the device's own keys; the eigenvalue margin of every fixture is asserted before its positions are compared."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cnr_amd
import mc_cpu as M
import meshops_cpu as R
import meshsimplify_cpu as S
from conftest import ROOT
from test_meshsimplify_host import CLUSTER_COUNTS, FANS, fixtures

MO = cnr_amd.meshops
pytestmark = pytest.mark.gpu
COUNTS = ("cell", "clusters", "faces_in", "faces_collapsed", "faces_duplicate", "faces_out", "vertices_out", "clamped")
NAMES = (["one_triangle"] + ["clusters_%d" % C for C in CLUSTER_COUNTS] + ["fan_%d" % n for n in FANS] +
         ["duplicate", "opposite", "lattice", "ico_a", "ico_b", "cube_a", "cube_b", "two_spheres"])
_REF = {}


def _t(a, dev, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype)


def gpu_simplify(v, f, dev, **kw):
    out_v, out_f, vmap, report = MO.simplify(_t(v, dev), _t(f, dev), details=True, **kw)
    got = {k: (x.cpu().numpy() if torch.is_tensor(x) else x) for k, x in report.items()}
    got.update(verts=out_v.cpu().numpy(), faces=out_f.cpu().numpy(), vertex_map=vmap.cpu().numpy())
    return got


def reference(name, placement, keys):
    """the restatement on the device's keys, computed once per (fixture, placement)"""
    if (name, placement) not in _REF:
        v, f, cell = fixtures()[name]
        _REF[name, placement] = S.simplify(v, f, cell, placement, keys=keys)
    return _REF[name, placement]


def assert_integers_equal(got, ref):
    for k in COUNTS:
        assert got[k] == ref[k], k
    assert got["faces"].dtype == np.int32 and got["vertex_map"].dtype == np.int32 and got["verts"].dtype == np.float32
    assert np.array_equal(got["faces"], ref["faces"]) and np.array_equal(got["vertex_map"], ref["vertex_map"])
    assert np.array_equal(got["representatives"], ref["representatives"])
    if "cluster" in ref:
        assert np.array_equal(got["cluster"], ref["cluster"]) and np.array_equal(got["roots"], ref["roots"])
    if ref["faces_out"]:
        assert np.array_equal(got["kept_clusters"], ref["kept_clusters"])
        assert np.array_equal(got["cluster_clamped"].astype(bool), ref["cluster_clamped"])


def within_one_ulp(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))


def assert_in_cells(got, cell):
    lo, hi = S.cell_bounds(S.key_cells(got["keys"][got["roots"]]), cell)
    q = got["cluster_verts"].astype(np.float64) - got["min"].astype(np.float64)
    assert ((q >= lo) & (q <= hi)).all()


# ---- every fixture: integers, sums, positions, a second run ------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_simplify_equals_the_restatement(dev, name):
    v, f, cell = fixtures()[name]
    got = gpu_simplify(v, f, dev, cell=cell)
    ref = reference(name, "quadric", got["keys"])
    assert_integers_equal(got, ref)
    if ref["faces_out"] == 0:                                  # every vertex in one cell: empty, and nothing ran on empty tensors
        assert got["verts"].shape == (0, 3) and got["faces"].shape == (0, 3) and (got["vertex_map"] == -1).all()
        return
    assert ref["margin"] >= S.MARGIN, ref["margin"]           # the fixture's conditions, before any position is compared
    assert S.coordinate_floor_ok(ref["cluster_verts"], v)
    assert np.array_equal(got["quadrics"], ref["quadrics"]) and np.array_equal(got["possum"], ref["possum"])       # bit-equal
    same = got["cluster_verts"] == ref["cluster_verts"]
    print(name, "clusters", ref["clusters"], "coordinates that differ at all: %.3g %%" % (100.0 * (1 - same.mean())))
    assert within_one_ulp(got["cluster_verts"], ref["cluster_verts"]).all()
    assert np.array_equal(got["verts"], got["cluster_verts"][got["kept_clusters"]])
    assert_in_cells(got, cell)
    # the errors of "quadric" are fp64 at positions that differ by round-off amplified by 1 / tau = 10^3; with |q| <= 64 here the
    # terms of x^T A x - 2 b^T x + c are at most 64^2 |Q|, so 2^-52 x 10^3 x 64^2 ~ 10^-9 |Q| bounds the difference: 10^-6 holds it
    err_scale = np.abs(ref["quadrics"]).max(1) + 1e-300
    assert (np.abs(got["cluster_error"] - ref["cluster_error"]) <= 1e-6 * err_scale).all()
    again = gpu_simplify(v, f, dev, cell=cell)                 # a second run: bit-identical in every output
    for k in got:
        if isinstance(got[k], np.ndarray):
            assert np.array_equal(got[k], again[k]), k
        else:
            assert got[k] == again[k], k


@pytest.mark.parametrize("placement", ["mean", "representative"])
@pytest.mark.parametrize("name", ["fan_17", "fan_257", "lattice", "ico_b", "cube_a", "two_spheres"])
def test_mean_and_representative_are_bit_equal(dev, name, placement):
    v, f, cell = fixtures()[name]
    got = gpu_simplify(v, f, dev, cell=cell, placement=placement)
    ref = reference(name, placement, got["keys"])
    assert_integers_equal(got, ref)
    assert np.array_equal(got["cluster_verts"], ref["cluster_verts"]) and np.array_equal(got["verts"], ref["verts"])
    assert np.array_equal(got["cluster_error"], ref["cluster_error"]) and got["quadric_error"] == ref["quadric_error"]
    assert np.array_equal(got["quadrics"], ref["quadrics"])
    assert_in_cells(got, cell)
    if placement == "representative":
        assert np.array_equal(got["verts"], v[got["representatives"]]) and got["clamped"] == 0
        kept, _, remap = MO.weld(_t(v, dev), _t(f, dev), cell=cell)                       # weld's vertices, bit-exact
        assert np.array_equal(kept.cpu().numpy(), got["roots"]) and np.array_equal(remap.cpu().numpy(), got["cluster"])


def test_empty_inputs_and_one_triangle(dev):
    z = torch.zeros(0, 3, device=dev, dtype=torch.int32)
    v, f, vmap, report = MO.simplify(torch.rand(5, 3, device=dev), z, cell=0.1)
    assert v.shape == (0, 3) and f.shape == (0, 3) and vmap.tolist() == [-1] * 5 and report["faces_out"] == 0 and report["clusters"] == 0
    v, f, vmap, report = MO.simplify(torch.zeros(0, 3, device=dev), z, target_faces=10)
    assert v.shape == (0, 3) and f.shape == (0, 3) and vmap.shape == (0,) and report["search"] == []
    tri, faces, cell = fixtures()["one_triangle"]
    for placement in MO.PLACEMENT:                           # three clusters of one vertex each: the triangle comes back
        v, f, vmap, report = MO.simplify(_t(tri, dev), _t(faces, dev), cell=cell, placement=placement)
        assert np.array_equal(v.cpu().numpy(), tri) and f.tolist() == [[0, 1, 2]] and vmap.tolist() == [0, 1, 2]
        assert report["quadric_error"] == 0.0 and report["clamped"] == 0
    assert MO.vertex_normals(torch.rand(4, 3, device=dev), z).tolist() == [[0.0] * 3] * 4


def test_shuffled_faces(dev):
    """another face order: the same clusters and positions up to the order of the sums, the same set of faces"""
    v, f, cell = fixtures()["ico_b"]
    perm = np.random.default_rng(4).permutation(len(f))
    a, b = gpu_simplify(v, f, dev, cell=cell), gpu_simplify(v, f[perm], dev, cell=cell)
    assert np.array_equal(a["cluster"], b["cluster"]) and np.array_equal(a["possum"], b["possum"])
    ref = S.simplify(v, f[perm], cell, keys=b["keys"])
    assert_integers_equal(b, ref)
    assert ref["margin"] >= S.MARGIN and S.coordinate_floor_ok(ref["cluster_verts"], v)
    assert np.array_equal(b["quadrics"], ref["quadrics"]) and within_one_ulp(b["cluster_verts"], ref["cluster_verts"]).all()
    rows = lambda x: sorted(map(tuple, S.face_rows(x).tolist()))
    assert rows(a["faces"]) == rows(b["faces"]) and np.array_equal(a["vertex_map"], b["vertex_map"])
    assert np.abs(a["quadrics"] - b["quadrics"]).max() <= 1e-12 * np.abs(a["quadrics"]).max()


def test_vertices_without_a_cell_are_refused(dev):
    v, f, cell = fixtures()["ico_a"]
    bad = v.copy()
    bad[7, 1] = np.nan
    with pytest.raises(ValueError):
        MO.simplify(_t(bad, dev), _t(f, dev), cell=cell)
    bad[7, 1] = np.inf
    with pytest.raises(ValueError):
        MO.simplify(_t(bad, dev), _t(f, dev), cell=cell)
    with pytest.raises(ValueError):                          # more than 2^21 cells on an axis
        MO.simplify(_t(v, dev), _t(f, dev), cell=2.0 ** -21)
    with pytest.raises(ValueError):
        MO.simplify(_t(v, dev), torch.tensor([[0, 1, len(v)]], device=dev, dtype=torch.int32), cell=cell)


# ---- quality -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube_a", "cube_b"])
def test_quadric_placement_finds_the_cube(dev, name):
    v, f, cell = fixtures()[name]
    quad, mean = gpu_simplify(v, f, dev, cell=cell), gpu_simplify(v, f, dev, cell=cell, placement="mean")
    dq, dm = S.cube_surface_distance(quad["verts"]).mean(), S.cube_surface_distance(mean["verts"]).mean()
    print(name, "mean distance to the surface: quadric %.4g, mean %.4g, ratio %.3g; clamped %d" % (dq, dm, dm / dq, quad["clamped"]))
    assert dq <= dm / 4
    assert quad["clamped"] == {"cube_a": 29, "cube_b": 19}[name]                            # the clamp path runs
    moved = np.linalg.norm(quad["cluster_verts"][quad["cluster"]].astype(np.float64) - v, axis=1)
    assert moved.max() <= np.sqrt(3) * cell * (1 + 2.0 ** -20)


# ---- vertex normals ----------------------------------------------------------------------------------------------------------
def test_vertex_normals(dev):
    """The fp64 sums are the restatement's bit for bit (the same order); a component then takes one correctly rounded square
    root and one correctly rounded division, at most a few units of 2^-53 relative on either side, and one rounding to fp32:
    the two fp32 results are equal or neighbours -- the bar is one fp32 unit in the last place."""
    for v, f in (fixtures()["ico_a"][:2], fixtures()["cube_a"][:2], S.fan(257), R.open_sheet()):
        v = np.concatenate([v, [[9, 9, 9]]]).astype(np.float32)                             # one vertex no face uses
        got = MO.vertex_normals(_t(v, dev), _t(f, dev)).cpu().numpy()
        ref = S.vertex_normals(v, f)
        assert within_one_ulp(got, ref).all() and got[-1].tolist() == [0, 0, 0]
        print("normals that differ at all: %.3g %%" % (100.0 * (got != ref).mean()))
        assert (np.abs(np.linalg.norm(got[np.unique(f)].astype(np.float64), axis=1) - 1) < 1e-6).all()
    both = np.concatenate([f[:1], f[:1, ::-1]])
    assert (MO.vertex_normals(_t(v, dev), _t(both, dev)) == 0).all()                        # a zero sum gives zeros
    # the side marching cubes' normals point to
    mv, mn, mf = cnr_amd.vis.marching_cubes_raw(_t(M.two_spheres(64), dev).float())
    n = MO.vertex_normals(mv, mf)
    assert ((n * mn).sum(1) > 0).all()


# ---- target_faces ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", [60, 1000])
def test_target_faces(dev, target):
    v, f, _ = fixtures()["ico_a"]
    got = gpu_simplify(v, f, dev, target_faces=target)
    cell, search = got["cell"], got["search"]
    assert got["faces_out"] <= target and len(search) <= 24 and dict(search)[cell] == got["faces_out"]
    assert all(n > target for c, n in search if c < cell)
    direct = gpu_simplify(v, f, dev, cell=cell)
    for k in ("verts", "faces", "vertex_map"):
        assert np.array_equal(got[k], direct[k]), k
    ref_cell, ref_search = S.search_cell(target, S.bbox_diag(v), lambda c: S.faces_out(v, f, c))
    assert [n for _, n in search] == [n for _, n in ref_search] and cell == ref_cell
    with pytest.raises(ValueError):
        MO.simplify(_t(v, dev), _t(f, dev))
    with pytest.raises(ValueError):
        MO.simplify(_t(v, dev), _t(f, dev), cell=0.1, target_faces=10)


# ---- Trainer.meshing -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_trainer(dev):
    from scene_synth import analytic_pool, sphere_radius
    cnr = cnr_amd
    torch.manual_seed(99)
    n_obj, R_, n1, n2, L = 4, 512, 4, 28, 32
    cfg = cnr.cfg.synthetic_config(device=str(dev), latent_dim=L, n_bins_cam2surface=n1, n_bins=n2)
    gen = torch.Generator().manual_seed(11)
    tr = cnr.fused.FusedCategoryTrainer(cfg, 1, n_obj, [analytic_pool(64 * R_, n_obj, gen)], R_, dev, seed=7, generator=gen)
    tr.run(400)
    torch.cuda.synchronize()
    sd = tr.state_dicts(0)
    ids = [10 + k for k in range(n_obj)]
    t = cnr.trainer.Trainer(cfg, 3, ids)
    with torch.no_grad():
        t.fc_occ_map.load_state_dict({k: v.to(cfg.training_device) for k, v in sd["FC_state_dict"].items()})
        t.pe.B_layer.weight.copy_(sd["PE_state_dict"]["B_layer.weight"])
        t.shape_codes.weight.copy_(sd["shape_code_state_dict"]["weight"][list(range(n_obj))])
        t.texture_codes.weight.copy_(sd["texture_code_state_dict"]["weight"][list(range(n_obj))])
    t.extent_dict = {10 + k: np.full(3, 2.4 * sphere_radius(k)) for k in range(n_obj)}
    return t


def _same_mesh(a, b):
    return (np.array_equal(a.vertices, b.vertices) and np.array_equal(a.faces, b.faces) and np.array_equal(a.vertex_normals, b.vertex_normals)
            and np.array_equal(a.visual.vertex_colors, b.visual.vertex_colors))


def test_trainer_meshing_simplify(dev, small_trainer):
    t = small_trainer
    plain = t.meshing(10, grid_dim=32)
    assert plain is not None and len(plain.faces) > 0
    assert _same_mesh(t.meshing(10, grid_dim=32, simplify=None), plain)                # bit-equal to the call without it
    target = len(plain.faces) // 4
    got = t.meshing(10, grid_dim=32, simplify=dict(target_faces=target))
    report = t.last_simplify_report
    assert 0 < len(got.faces) <= target and report["faces_in"] == len(plain.faces) and report["faces_out"] == len(got.faces)
    pts = torch.from_numpy(got.vertices).float().to(dev)
    _, col = t.eval_points(pts, inst_id=10)                                            # the colours are the field's at the new vertices
    assert np.array_equal(got.visual.vertex_colors[:, :3], (col * 255).cpu().numpy().astype(np.uint8))
    want_v, want_f, _, _ = MO.simplify(_t(plain.vertices, dev, torch.float32), _t(plain.faces.astype(np.int32), dev), cell=report["cell"])
    assert np.array_equal(got.vertices, want_v.cpu().numpy().astype(np.float64)) and np.array_equal(got.faces, want_f.cpu().numpy())
    assert np.array_equal(got.vertex_normals, MO.vertex_normals(want_v, want_f).cpu().numpy().astype(np.float64))
    field = t.meshing(10, grid_dim=32, normals="field", simplify=dict(cell=report["cell"]))
    assert np.array_equal(field.vertices, got.vertices) and not np.array_equal(field.vertex_normals, got.vertex_normals)
    both = t.meshing(10, grid_dim=32, clean=dict(keep_largest=1), simplify=dict(cell=report["cell"]))        # composes with clean
    cleaned = t.meshing(10, grid_dim=32, clean=dict(keep_largest=1))
    assert 0 < len(both.faces) < len(cleaned.faces) and t.last_simplify_report["faces_in"] == len(cleaned.faces)
    assert t.last_clean_report["n_kept"] == 1


# ---- the tool --------------------------------------------------------------------------------------------------------------
def test_simplify_mesh_tool_round_trips_an_obj(dev, tmp_path):
    v, f, cell = fixtures()["ico_b"]
    mesh = cnr_amd.vis.Mesh(v, f, v)
    mesh.visual.vertex_colors = np.random.default_rng(0).integers(0, 256, (len(v), 3))
    src, dst = str(tmp_path / "in.obj"), str(tmp_path / "out.obj")
    mesh.export(src)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "simplify_mesh.py"), src, dst, "--cell", str(cell)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from clean_mesh import load
    finally:
        sys.path.pop(0)
    loaded = load(cnr_amd, src)
    want, report = MO.simplify_mesh(loaded, cell=cell)
    assert "faces %d -> %d" % (len(f), report["faces_out"]) in out.stdout and "clusters: %d" % report["clusters"] in out.stdout
    back = load(cnr_amd, dst)
    assert np.array_equal(back.faces, want.faces) and np.abs(back.vertices - want.vertices).max() <= 1e-8
    assert np.array_equal(back.visual.vertex_colors, want.visual.vertex_colors)
    assert np.array_equal(want.visual.vertex_colors, loaded.visual.vertex_colors[report["representatives"].cpu().numpy()])
    assert 0 < len(back.faces) < len(f) // 2
