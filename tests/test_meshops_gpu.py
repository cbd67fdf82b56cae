"""GPU: mesh clean-up (csrc/mesh_topo.hip, cnr_amd.meshops) against the numpy restatement
tests/meshops_cpu.py, whose own correctness and whose fixtures' conditions tests/test_meshops_host.py proves without a GPU.
Integer outputs are EQUAL to the restatement, areas bit-equal to it (and within F 2^-53 relative of math.fsum), bounding boxes
exact, the device err word 0 (a set word raises)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cnr_amd
import mc_cpu as M
import meshops_cpu as R
from conftest import ROOT

MO = cnr_amd.meshops
pytestmark = pytest.mark.gpu
INT_FIELDS = ("face_component", "vertex_component", "first", "n_faces", "n_vertices", "edge_counts", "watertight")
LADDER_N = 100000


def _t(a, dev, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype)


def gpu_components(v, f, dev, conn="edge", with_verts=True):
    return MO.components(_t(f, dev), len(v), _t(v, dev) if with_verts else None, connectivity=conn)


def assert_table_equal(got, ref, v=None, f=None):
    assert got.n == ref["n"]
    for k in INT_FIELDS:
        assert np.array_equal(getattr(got, k).cpu().numpy(), ref[k]), k
    assert got.boundary_edges == ref["boundary_edges"] and got.nonmanifold_edges == ref["nonmanifold_edges"]
    if "area" in ref:
        area = got.area.cpu().numpy()
        assert np.array_equal(area, ref["area"])                                       # bit-equal: the same order of operations
        assert np.array_equal(got.bbox_min.cpu().numpy(), ref["bbox_min"]) and np.array_equal(got.bbox_max.cpu().numpy(), ref["bbox_max"])
        assert np.array_equal(got.diag.cpu().numpy(), ref["diag"])
        if v is not None and ref["n"] <= 64:
            for c in range(ref["n"]):
                exact = R.fsum_area(v, f, ref["face_component"], c)
                assert abs(area[c] - exact) <= len(f) * 2.0 ** -53 * exact, c


@functools.lru_cache(maxsize=None)
def mc_fixture(name):
    vol = M.two_spheres(64) if name == "two_spheres" else M.random_binary(24, int(name.split("_")[1]))
    v, n, f = M.marching_cubes(vol)
    return v, n, f, {conn: R.components(f, len(v), v, conn) for conn in ("edge", "vertex")}


# ---- sizes that end inside a wave, a block and a scan run ------------------------------------------------------------------
@pytest.mark.parametrize("F", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
@pytest.mark.parametrize("conn", ["edge", "vertex"])
def test_disjoint_triangles(dev, F, conn):
    v, f = R.disjoint_triangles(F)
    got = gpu_components(v, f, dev, conn)
    assert got.n == F
    vc = got.vertex_component.cpu().numpy()
    assert (vc[-2:] == -1).all() and np.array_equal(vc[:-2], np.repeat(np.arange(F), 3))      # unreferenced vertices: -1
    assert_table_equal(got, R.components(f, len(v), v, conn), v, f)
    # ... and a second mesh where the unreferenced vertices lie in the middle and the faces are listed backwards
    if F > 1:
        f2 = (f[::-1] + (f[::-1] >= 3 * (F // 2)) * 2).astype(np.int32)
        v2 = np.insert(v[:-2], 3 * (F // 2), v[-2:], axis=0)
        assert_table_equal(gpu_components(v2, f2, dev, conn), R.components(f2, len(v2), v2, conn), v2, f2)


# ---- the ladder ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled", "permuted"])
@pytest.mark.parametrize("conn", ["edge", "vertex"])
def test_ladder_is_one_component(dev, order, conn):
    v, f = R.ladder(LADDER_N, order)
    got = gpu_components(v, f, dev, conn)
    assert got.n == 1 and int(got.first[0]) == 0
    assert int(got.labels.max()) == 0 and int(got.labels.min()) == 0                   # the label is the minimum
    assert int(got.face_component.max()) == 0 and int(got.vertex_component.min()) == 0
    assert got.n_faces.tolist() == [2 * (LADDER_N - 1)] and got.n_vertices.tolist() == [2 * LADDER_N]
    assert got.boundary_edges == 2 * LADDER_N and got.nonmanifold_edges == 0 and not bool(got.watertight[0])
    assert float(got.area[0]) == LADDER_N - 1                                          # unit quads: every partial sum is exact
    assert got.bbox_min.tolist() == [[0.0, 0.0, 0.0]] and got.bbox_max.tolist() == [[LADDER_N - 1.0, 1.0, 0.0]]


def test_union_find_over_a_pair_list(dev):
    """the pair-list entry point on the ladder's vertex pairs in four orders, and on a graph with many sets"""
    rng = np.random.default_rng(1)
    v, f = R.ladder(LADDER_N, "permuted")
    pairs = R.vertex_pairs(f)
    for p in (pairs, pairs[::-1], pairs[rng.permutation(len(pairs))]):
        lab = MO.union_find(_t(p, dev, torch.int32), len(v))
        assert int(lab.max()) == 0
    n = 5000
    p = rng.integers(0, n, (3000, 2))
    want = R.labels_from_pairs(p, n)
    assert len(np.unique(want)) > 100
    assert np.array_equal(MO.union_find(_t(p, dev, torch.int32), n).cpu().numpy(), want)
    assert np.array_equal(MO.union_find(torch.zeros(0, 2, device=dev, dtype=torch.int32), 5).cpu().numpy(), np.arange(5))
    with pytest.raises(ValueError):
        MO.union_find(torch.tensor([[0, 7]], device=dev, dtype=torch.int32), 5)


# ---- small meshes ----------------------------------------------------------------------------------------------------------
def test_pinch(dev):
    v, f = R.pinch()
    for conn, n in (("vertex", 1), ("edge", 2)):
        got = gpu_components(v, f, dev, conn)
        assert got.n == n
        assert_table_equal(got, R.components(f, len(v), v, conn), v, f)
    assert gpu_components(v, f, dev, "edge").watertight.tolist() == [True, True]


def test_edge_statistics(dev):
    v, f = R.open_sheet()
    got = gpu_components(v, f, dev)
    ref = R.components(f, len(v), v)
    assert got.boundary_edges == ref["boundary_edges"] == 24 and not bool(got.watertight[0])
    assert_table_equal(got, ref, v, f)
    v, f = R.fan3()
    got = gpu_components(v, f, dev)
    assert got.nonmanifold_edges == 1 and not bool(got.watertight[0])
    assert_table_equal(got, R.components(f, len(v), v), v, f)
    v, f = R.flipped_tetra()
    got = gpu_components(v, f, dev)
    assert got.boundary_edges == 0 and got.nonmanifold_edges == 0 and not bool(got.watertight[0])
    assert_table_equal(got, R.components(f, len(v), v), v, f)
    assert bool(gpu_components(R.TETRA_V, R.TETRA, dev).watertight[0])
    # a face with a repeated corner: its degenerate edge joins and counts nothing
    f2 = np.concatenate([R.TETRA, [[0, 0, 1]]]).astype(np.int32)
    assert_table_equal(gpu_components(R.TETRA_V, f2, dev), R.components(f2, 4, R.TETRA_V), R.TETRA_V, f2)
    assert_table_equal(gpu_components(R.TETRA_V, f2, dev, "vertex"), R.components(f2, 4, R.TETRA_V, "vertex"), R.TETRA_V, f2)
    with pytest.raises(ValueError):
        MO.components(torch.tensor([[0, 1, 4]], device=dev, dtype=torch.int32), 4)
    with pytest.raises(ValueError):
        MO.components(torch.tensor([[0, -1, 2]], device=dev, dtype=torch.int32), 4)
    t = MO.components(_t(R.TETRA, dev), 4)                                              # no verts: the counts only
    assert t.area is None and t.n_faces.tolist() == [4] and t.n_vertices.tolist() == [4]


# ---- marching cubes --------------------------------------------------------------------------------------------------------
def test_two_spheres(dev):
    v, n, f, ref = mc_fixture("two_spheres")
    got = gpu_components(v, f, dev)
    assert got.n == 2 and got.watertight.tolist() == [True, True]
    assert_table_equal(got, ref["edge"], v, f)
    assert_table_equal(gpu_components(v, f, dev, "vertex"), ref["vertex"], v, f)
    # keep_largest=1: the larger sphere (the restatement's larger area), closed, genus 0
    mesh = cnr_amd.vis.Mesh(v, f, n)
    mesh.visual.vertex_colors = np.random.default_rng(0).integers(0, 256, (len(v), 3))
    out, report = MO.clean_mesh(mesh, keep_largest=1)
    big = int(np.argmax(ref["edge"]["area"]))
    want = cnr_amd.raster.cull_mesh(mesh, ref["edge"]["face_component"] == big)
    assert report["kept"].tolist() == [c == big for c in range(2)] and report["n_components"] == 2 and report["n_kept"] == 1
    assert np.array_equal(out.vertices, want.vertices) and np.array_equal(out.faces, want.faces)
    assert np.array_equal(out.vertex_normals, want.vertex_normals)
    assert np.array_equal(out.visual.vertex_colors, want.visual.vertex_colors)
    assert M.euler(out.vertices, out.faces) == 2
    assert report["faces_out"] == len(out.faces) == ref["edge"]["n_faces"][big] and report["vertices_out"] == len(out.vertices)


@pytest.mark.parametrize("seed", [0, 1])
def test_random_binary_volume(dev, seed):
    v, n, f, ref = mc_fixture("random_%d" % seed)
    assert ref["edge"]["n"] >= 100
    got = gpu_components(v, f, dev)
    assert_table_equal(got, ref["edge"], v, f)
    assert_table_equal(gpu_components(v, f, dev, "vertex"), ref["vertex"], v, f)
    # boundary edges only on the grid's outer faces: every component that has one touches the border of [0, 1]^3
    assert M.boundary_edges_on_outer_faces(v, f, 24)
    open_c = got.edge_counts[:, 0].cpu().numpy() > 0
    touches = (got.bbox_min.cpu().numpy() == 0).any(1) | (got.bbox_max.cpu().numpy() == 1).any(1)
    assert not (open_c & ~touches).any() and got.nonmanifold_edges == 0


def test_order_independence_and_determinism(dev):
    v, n, f, ref = mc_fixture("random_0")
    perm = np.random.default_rng(9).permutation(len(f))
    for conn in ("edge", "vertex"):
        a = gpu_components(v, f, dev, conn)
        b = gpu_components(v, f[perm], dev, conn)
        if conn == "vertex":                           # components are numbered by their smallest vertex: the very same arrays
            assert torch.equal(a.vertex_component, b.vertex_component) and torch.equal(a.labels, b.labels)
            assert torch.equal(a.face_component[torch.from_numpy(perm).to(dev)], b.face_component)
            assert torch.equal(a.n_faces, b.n_faces) and torch.equal(a.edge_counts, b.edge_counts)
            assert torch.equal(a.bbox_min, b.bbox_min) and torch.equal(a.bbox_max, b.bbox_max)
        else:                                          # ... by their smallest FACE: the same partition under other numbers
            pa, pb = a.vertex_component.cpu().numpy(), b.vertex_component.cpu().numpy()
            pairs = np.unique(np.stack([pa, pb]), axis=1)
            assert len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1])) == a.n == b.n
            assert np.array_equal(np.sort(a.n_faces.cpu().numpy()), np.sort(b.n_faces.cpu().numpy()))
        c = gpu_components(v, f, dev, conn)            # a second run: bit-identical
        for k in INT_FIELDS + ("area", "bbox_min", "bbox_max", "diag", "labels"):
            assert torch.equal(getattr(a, k), getattr(c, k)), k


# ---- welding ---------------------------------------------------------------------------------------------------------------
def test_weld_exact(dev):
    v, f, soup = R.exact_weld_case()
    kept, nf, remap = MO.weld(_t(soup, dev))
    rk, rf, rr = R.weld(soup)
    assert np.array_equal(kept.cpu().numpy(), rk) and np.array_equal(nf.cpu().numpy(), rf) and np.array_equal(remap.cpu().numpy(), rr)
    assert np.array_equal(nf.cpu().numpy()[:-1], f)                                    # the original's faces, index for index
    assert nf.cpu().numpy()[-1].tolist() == [len(v), len(v) + 1, len(v) + 2]           # the NaN row welds with nothing
    assert np.array_equal(_t(soup, dev).reshape(-1, 3).index_select(0, kept.long()).cpu().numpy()[:len(v)], v)
    # indexed input; attributes are the representative's
    kept, nf, remap = MO.weld(_t(soup.reshape(-1, 3), dev), _t(np.arange(3 * len(soup), dtype=np.int32).reshape(-1, 3), dev))
    assert np.array_equal(kept.cpu().numpy(), rk) and np.array_equal(nf.cpu().numpy(), rf)
    # two NaN rows with the same bits still weld with nothing
    two = np.array([[np.nan, 1, 2], [np.nan, 1, 2], [3, 4, 5], [3, 4, 5]], np.float32)
    kept, _, remap = MO.weld(_t(two, dev), torch.zeros(0, 3, device=dev, dtype=torch.int32))
    assert kept.tolist() == [0, 1, 2] and remap.tolist() == [0, 1, 2, 2]
    assert np.array_equal(remap.cpu().numpy(), R.weld(two, np.zeros((0, 3), np.int32))[2])


def test_weld_degenerate_faces(dev):
    vv = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 1, 0]], np.float32)
    ff = np.array([[0, 1, 2], [0, 1, 3]], np.int32)
    for drop in (True, False):
        kept, nf, remap = MO.weld(_t(vv, dev), _t(ff, dev), drop_degenerate=drop)
        rk, rf, rr = R.weld(vv, ff, drop_degenerate=drop)
        assert np.array_equal(kept.cpu().numpy(), rk) and np.array_equal(nf.cpu().numpy(), rf) and np.array_equal(remap.cpu().numpy(), rr)
    assert len(R.weld(vv, ff)[1]) == 1 and len(R.weld(vv, ff, drop_degenerate=False)[1]) == 2


def test_weld_cell(dev):
    pts, ids, cell = R.jittered_lattice()
    kept, _, remap = MO.weld(_t(pts, dev), torch.zeros(0, 3, device=dev, dtype=torch.int32), cell=cell)
    rk, _, rr = R.weld(pts, np.zeros((0, 3), np.int32), cell=cell)
    assert np.array_equal(kept.cpu().numpy(), rk) and np.array_equal(remap.cpu().numpy(), rr) and len(rk) == 6 ** 3
    bad = pts.copy()
    bad[5] = np.nan                                                                    # key -1: welds with nothing
    bad[9] = np.inf
    kept, _, remap = MO.weld(_t(bad, dev), torch.zeros(0, 3, device=dev, dtype=torch.int32), cell=cell)
    rk, _, rr = R.weld(bad, np.zeros((0, 3), np.int32), cell=cell)
    assert np.array_equal(kept.cpu().numpy(), rk) and np.array_equal(remap.cpu().numpy(), rr)
    assert 5 in rk and 9 in rk


def test_weld_sphere_halves(dev):
    v, f = R.sphere_halves()
    before = gpu_components(v, f, dev)
    assert before.n == 2 and before.boundary_edges > 0
    kept, nf, remap = MO.weld(_t(v, dev), _t(f, dev))
    rk, rf, rr = R.weld(v, f)
    assert np.array_equal(kept.cpu().numpy(), rk) and np.array_equal(nf.cpu().numpy(), rf)
    after = MO.components(nf, len(kept), _t(v, dev).index_select(0, kept.long()))
    assert after.n == 1 and after.watertight.tolist() == [True] and after.boundary_edges == 0
    # the same through clean_mesh(weld=0.0), which also gathers the attributes
    mesh = cnr_amd.vis.Mesh(v, f, v)
    out, report = MO.clean_mesh(mesh, weld=0.0)
    assert report["n_components"] == 1 and np.array_equal(out.vertices, mesh.vertices[rk]) and np.array_equal(out.faces, rf)
    assert np.array_equal(out.vertex_normals, mesh.vertex_normals[rk]) and report["vertices_in"] == len(v)


# ---- compaction ------------------------------------------------------------------------------------------------------------
def test_compact_is_cull_mesh(dev):
    v, n, f, _ = mc_fixture("random_0")
    rng = np.random.default_rng(5)
    mesh = cnr_amd.vis.Mesh(v, f, n)
    mesh.visual.vertex_colors = rng.integers(0, 256, (len(v), 3))
    dv, dn, dc = _t(v, dev), _t(n, dev), _t(mesh.visual.vertex_colors, dev)
    masks = [rng.random(len(f)) < p for p in (0.02, 0.5, 0.97)] + [np.zeros(len(f), bool), np.ones(len(f), bool)]
    for keep in masks:
        nf, vmap, kept = MO.compact(_t(f, dev), len(v), _t(keep, dev))
        ref = cnr_amd.raster.cull_mesh(mesh, keep)
        idx = kept.long()
        assert np.array_equal(nf.cpu().numpy(), ref.faces)
        assert np.array_equal(dv.index_select(0, idx).cpu().numpy().astype(np.float64), ref.vertices)
        assert np.array_equal(dn.index_select(0, idx).cpu().numpy().astype(np.float64), ref.vertex_normals)
        assert np.array_equal(dc.index_select(0, idx).cpu().numpy(), ref.visual.vertex_colors)
        rf, rmap, rused = R.compact(f, len(v), keep)
        assert np.array_equal(vmap.cpu().numpy(), rmap) and np.array_equal(kept.cpu().numpy(), rused)
        assert np.array_equal(MO.compact(_t(f, dev), len(v), _t(keep, dev), reindex=False).cpu().numpy(), f[keep])
    # sizes that end inside a block of the scan
    for F in (1, 1023, 1024, 1025):
        vv, ff = R.disjoint_triangles(F)
        keep = rng.random(F) < 0.5
        nf, vmap, kept = MO.compact(_t(ff, dev), len(vv), _t(keep, dev))
        rf, rmap, rused = R.compact(ff, len(vv), keep)
        assert np.array_equal(nf.cpu().numpy(), rf) and np.array_equal(vmap.cpu().numpy(), rmap) and np.array_equal(kept.cpu().numpy(), rused)


# ---- clean_mesh ------------------------------------------------------------------------------------------------------------
def test_clean_mesh_thresholds(dev):
    v, f = R.sheets([(1, 1), (1, 3), (2, 2), (2, 4)])
    ref = R.components(f, len(v), v)
    assert ref["area"].tolist() == [1.0, 3.0, 4.0, 8.0]
    mesh = cnr_amd.vis.Mesh(v, f)

    def kept(**kw):
        out, report = MO.clean_mesh(mesh, **kw)
        want = cnr_amd.raster.cull_mesh(mesh, report["kept"][ref["face_component"]])
        assert np.array_equal(out.vertices, want.vertices) and np.array_equal(out.faces, want.faces)
        return report["kept"].tolist()
    assert kept() == [True] * 4
    assert kept(min_faces=6) == [False, True, True, True] and kept(min_faces=7) == [False, False, True, True]
    assert kept(min_area=4.0) == [False, False, True, True]                            # exactly on the threshold: kept
    assert kept(min_area=float(np.nextafter(4.0, 5.0))) == [False, False, False, True]
    assert kept(min_diag=float(ref["diag"][2])) == [bool(d >= ref["diag"][2]) for d in ref["diag"]]
    assert kept(min_diag=float(ref["diag"][2]))[2]
    assert kept(min_area_fraction=0.25) == [False, False, True, True]                  # 0.25 x 16 = 4 exactly
    assert kept(keep_largest=1) == [False, False, False, True]
    assert kept(keep_largest=2, largest_by="faces") == [False, False, True, True]
    assert kept(min_area=100.0) == [False, False, False, True]                         # never empty
    v2, f2 = R.sheets([(2, 2), (1, 4), (2, 2)])                                        # three components of area 4
    mesh2 = cnr_amd.vis.Mesh(v2, f2)
    out, report = MO.clean_mesh(mesh2, keep_largest=1)
    assert report["kept"].tolist() == [True, False, False] and len(out.faces) == 8      # ties: the lower id
    out, report = MO.clean_mesh(mesh2, keep_largest=1, largest_by="diag")
    assert report["kept"].tolist() == [False, True, False]
    empty, report = MO.clean_mesh(cnr_amd.vis.Mesh(np.zeros((0, 3)), np.zeros((0, 3), np.int64)), keep_largest=1)
    assert len(empty.faces) == 0 and len(empty.vertices) == 0 and report["n_components"] == 0


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


def test_trainer_meshing_clean(dev, small_trainer):
    t = small_trainer
    plain = t.meshing(10, grid_dim=32)
    assert plain is not None and len(plain.faces) > 0
    assert _same_mesh(t.meshing(10, grid_dim=32, clean=None), plain)                   # bit-equal to the call without it
    noop = t.meshing(10, grid_dim=32, clean={})
    assert _same_mesh(noop, plain) and t.last_clean_report["n_kept"] == t.last_clean_report["n_components"]
    got = t.meshing(10, grid_dim=32, clean=dict(keep_largest=1))
    print("components of the 32^3 mesh:", t.last_clean_report["n_components"])
    want, report = MO.clean_mesh(plain, keep_largest=1)
    assert np.array_equal(got.vertices, want.vertices) and np.array_equal(got.faces, want.faces)
    assert np.array_equal(got.vertex_normals, want.vertex_normals)
    assert report["kept"].tolist() == t.last_clean_report["kept"].tolist() and report["n_kept"] == 1
    _, col = t.eval_points(torch.from_numpy(got.vertices).float().to(dev), inst_id=10)  # the colour pass ran on the kept vertices
    assert np.array_equal(got.visual.vertex_colors[:, :3], (col * 255).cpu().numpy().astype(np.uint8))
    assert MO.components(_t(got.faces.astype(np.int32), dev), len(got.vertices)).n == 1


# ---- the tool --------------------------------------------------------------------------------------------------------------
def test_clean_mesh_tool_round_trips_an_obj(dev, tmp_path):
    v, n, f, ref = mc_fixture("two_spheres")
    mesh = cnr_amd.vis.Mesh(v, f, n)
    src, dst = str(tmp_path / "in.obj"), str(tmp_path / "out.obj")
    mesh.export(src)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "clean_mesh.py"), src, dst, "--keep_largest", "1"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "components: 2" in out.stdout and "kept: 1" in out.stdout
    back = cnr_amd.vis.load_mesh(dst)
    loaded = cnr_amd.vis.load_mesh(src)
    want, _ = MO.clean_mesh(loaded, keep_largest=1)
    assert np.array_equal(back.faces, want.faces) and np.abs(back.vertices - want.vertices).max() <= 1e-8
    assert len(back.faces) == ref["edge"]["n_faces"].max() and M.euler(back.vertices, back.faces) == 2
