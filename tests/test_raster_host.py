"""CPU: the numpy restatement of the mesh rasteriser (tests/raster_cpu.py) against a brute-force Moeller-Trumbore intersection
on every random fixture the GPU tests use, and against images written out by hand on dyadic fixtures where every quantity is
exact in fp64; cull_mesh, the depth-L1 bookkeeping and the argument errors that need no GPU."""
import numpy as np
import pytest
import torch

import raster_cpu as RC

EDGE = 1e-9


def check_against_moller_trumbore(verts, faces, T_wc, cam):
    """first: at most 0.1 % of the pixels within EDGE of an edge; then on the others the restatement's faces are
    Moeller-Trumbore's and the depths agree to 1e-12 relative.  -> the restatement's result"""
    W, H = cam["W"], cam["H"]
    dirs = RC.pinhole_dirs(W, H, cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    r = RC.rasterize(verts, faces, np.linalg.inv(T_wc), dirs, W, H, cam["zmin"], cam["zmax"])
    near = r["margin"] < EDGE
    print("pixels within 1e-9 of an edge:", int(near.sum()), "of", W * H)
    assert near.sum() <= 0.001 * W * H
    f_mt, t_mt = RC.moller_trumbore(verts, faces, T_wc, dirs, W, H, cam["zmin"], cam["zmax"])
    ok = ~near
    assert (r["face"][ok] == f_mt[ok]).all()
    hit = ok & (f_mt >= 0)
    assert hit.sum() > 0.2 * W * H
    rel = np.abs(r["t"][hit] - t_mt[hit]) / t_mt[hit]
    print("largest relative depth difference:", rel.max())
    assert rel.max() <= 1e-12
    return r


@pytest.mark.parametrize("pose", ["identity", "rigid"])
def test_soup_restatement_is_moller_trumbore(pose):
    verts, faces = RC.soup()
    T = np.eye(4) if pose == "identity" else RC.random_rigid()
    if pose == "rigid":                 # the same soup in front of the moved camera
        verts = (verts.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    r = check_against_moller_trumbore(verts, faces, T, RC.SOUP_CAM)
    z = (np.linalg.inv(T)[:3] @ np.concatenate([verts.astype(np.float64), np.ones((len(verts), 1))], 1).T)[2].reshape(-1, 3)
    assert ((z.min(1) < 0) & (z.max(1) > 0)).sum() >= 5 and (z.max(1) < 0).sum() >= 1      # the fixture is what it says
    assert len(np.unique(r["face"])) > 20


# ---- dyadic fixtures: DYADIC_CAM, identity pose, corners on dyadic coordinates ---------------------------------------------
def _tri_rule(w, h):
    """inside the pixel triangle (4,2) (4,20) (28,11), edges included"""
    return w >= 4 and 8 * h >= 16 + 3 * (w - 4) and 8 * h <= 160 - 3 * (w - 4)


def dyadic_cases():
    """-> [dict(name, verts f32, faces, cull, face (W,H) i32, depth (W,H) f32)]: the expected images by hand"""
    P = RC.dyadic_point
    W, H = RC.DYADIC_CAM["W"], RC.DYADIC_CAM["H"]
    cases = []

    # A: fill rule, tie rule, occlusion and the faces that cover nothing
    tris = [
        [P(4, 4, 2), P(12, 4, 2), P(12, 12, 2)],            # 0, 1: a quad split along the diagonal w = h, which passes through
        [P(4, 4, 2), P(12, 12, 2), P(4, 12, 2)],            #       pixel centres; corners on pixel centres
        [P(16, 2, 2), P(22, 2, 2), P(16, 8, 2)],            # 2, 3: coincident duplicates
        [P(16, 2, 2), P(22, 2, 2), P(16, 8, 2)],
        [P(16, 12, 4), P(28, 12, 4), P(16, 22, 4)],         # 4: the farther face ...
        [P(18, 13, 2), P(22, 13, 2), P(18, 17, 2)],         # 5: ... and a nearer one over it
        [P(1, 20, 2), P(1, 20, 2), P(3, 22, 2)],            # 6: zero area
        [[0.0, -0.1875, 2.0], [0.0, -0.0625, 2.0], [0.0, -0.25, 4.0]],   # 7: edge-on, in the plane x = 0 through the camera
        [[-1.0, -1.0, -2.0], [1.0, -1.0, -2.0], [0.0, 1.0, -2.0]],       # 8: wholly behind the camera
        [P(1.25, 14.25, 2), P(10.75, 14.5, 2), P(1.25, 14.75, 2)],       # 9: a sliver between the rows h = 14 and h = 15
    ]
    face, depth = np.full((W, H), -1, np.int32), np.zeros((W, H), np.float32)
    for w in range(W):
        for h in range(H):
            if 4 <= w <= 12 and 4 <= h <= 12:
                face[w, h], depth[w, h] = (0 if h <= w else 1), 2.0          # the shared diagonal goes to face 0
            elif w >= 16 and h >= 2 and (w - 16) + (h - 2) <= 6:
                face[w, h], depth[w, h] = 2, 2.0                             # not 3
            elif w >= 18 and h >= 13 and (w - 18) + (h - 13) <= 4:
                face[w, h], depth[w, h] = 5, 2.0
            elif w >= 16 and h >= 12 and 10 * (w - 16) + 12 * (h - 12) <= 120:
                face[w, h], depth[w, h] = 4, 4.0
    cases.append(dict(name="fill_tie_occlusion", tris=tris, cull=False, face=face, depth=depth))

    # B: a face from z = 4 to z = 16, cut per pixel at zmax = 8: 1 / z = 1/4 - (w - 4) / 128, so z = 128 / (36 - w) <= 8 up to
    # and including w = 20
    face, depth = np.full((W, H), -1, np.int32), np.zeros((W, H), np.float32)
    for w in range(W):
        for h in range(H):
            if _tri_rule(w, h) and w <= 20:
                face[w, h], depth[w, h] = 0, np.float32(128.0 / (36 - w))
    cases.append(dict(name="straddles_zmax", tris=[[P(4, 2, 4), P(4, 20, 4), P(28, 11, 16)]], cull=False, face=face, depth=depth))

    # C: a face from z = 1 to z = 1/4, cut per pixel at zmin = 1/2: 1 / z = 1 + (w - 4) / 8, so z = 8 / (4 + w) >= 1/2 up to and
    # including w = 12; one corner is nearer than zmin, so the tile box comes from the cut triangle
    face, depth = np.full((W, H), -1, np.int32), np.zeros((W, H), np.float32)
    for w in range(W):
        for h in range(H):
            if _tri_rule(w, h) and w <= 12:
                face[w, h], depth[w, h] = 0, np.float32(8.0 / (4 + w))
    cases.append(dict(name="straddles_zmin", tris=[[P(4, 2, 1), P(4, 20, 1), P(28, 11, 0.25)]], cull=False, face=face, depth=depth))

    # D: the same triangle twice with opposite windings; two-sided the lower index wins, culled the one with det > 0 (face 1,
    # corners clockwise as the image is displayed)
    a, b, c = P(6, 5, 2), P(20, 5, 2), P(6, 19, 2)
    for cull in (False, True):
        face, depth = np.full((W, H), -1, np.int32), np.zeros((W, H), np.float32)
        for w in range(W):
            for h in range(H):
                if w >= 6 and h >= 5 and (w - 6) + (h - 5) <= 14:
                    face[w, h], depth[w, h] = (1 if cull else 0), 2.0
        cases.append(dict(name="windings_cull" if cull else "windings", tris=[[a, c, b], [a, b, c]], cull=cull, face=face, depth=depth))

    for case in cases:
        v = np.array(case.pop("tris"), np.float64).reshape(-1, 3)
        case["verts"] = v.astype(np.float32)
        assert (case["verts"].astype(np.float64) == v).all()          # dyadic: fp32 holds them exactly
        case["faces"] = np.arange(len(v)).reshape(-1, 3)
    return cases


@pytest.mark.parametrize("case", dyadic_cases(), ids=lambda c: c["name"])
def test_dyadic_restatement_is_the_hand_written_image(case):
    cam = RC.DYADIC_CAM
    dirs = RC.pinhole_dirs(cam["W"], cam["H"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    r = RC.rasterize(case["verts"], case["faces"], np.eye(4), dirs, cam["W"], cam["H"], cam["zmin"], cam["zmax"],
                     cull_backfaces=case["cull"])
    assert (r["face"] == case["face"]).all()
    assert r["depth"].tobytes() == case["depth"].tobytes()
    assert (case["face"] >= 0).sum() > 40


def test_dyadic_fixture_touches_the_limits():
    """the depth-limit cases hold pixels exactly AT the limit, kept, and pixels of the same face beyond it, dropped"""
    cases = {c["name"]: c for c in dyadic_cases()}
    assert cases["straddles_zmax"]["depth"].max() == 8.0 and cases["straddles_zmax"]["face"][21, 11] == -1
    assert cases["straddles_zmin"]["depth"][cases["straddles_zmin"]["face"] >= 0].min() == 0.5
    assert cases["straddles_zmin"]["face"][13, 11] == -1


# ---- cull_mesh -------------------------------------------------------------------------------------------------------------
def _mesh_with_unused_vertices():
    from cnr_amd.vis import Mesh
    rng = np.random.default_rng(3)
    verts = rng.normal(size=(9, 3))
    faces = np.array([[0, 2, 4], [4, 2, 6], [6, 8, 0], [2, 8, 4]])          # the odd vertices are unused
    m = Mesh(verts, faces, rng.normal(size=(9, 3)))
    m.visual.vertex_colors = rng.integers(0, 256, (9, 3))
    return m


@pytest.mark.parametrize("keep", ["all", "none", "alternating", "indices"])
def test_cull_mesh_compacts_and_reindexes(keep):
    from cnr_amd import raster
    m = _mesh_with_unused_vertices()
    mask = {"all": np.ones(4, bool), "none": np.zeros(4, bool), "alternating": np.array([True, False, True, False]),
            "indices": np.array([3, 1])}[keep]
    out = raster.cull_mesh(m, torch.from_numpy(mask) if keep == "alternating" else mask)
    v, f, c, n = RC.cull_mesh(m.vertices, m.faces, m.visual.vertex_colors, m.vertex_normals, mask)
    assert out.faces.shape == f.shape and (out.faces == f).all()
    assert (out.vertices == v).all() and (out.vertex_normals == n).all() and (out.visual.vertex_colors == c).all()
    idx = np.nonzero(mask)[0] if mask.dtype == bool else mask
    assert (out.vertices[out.faces] == m.vertices[m.faces[idx]]).all()          # the same triangles, corner for corner
    if keep == "all":
        assert len(out.vertices) == 5 and (out.faces == m.faces // 2).all()      # by hand: 0 2 4 6 8 -> 0 1 2 3 4
    if keep == "none":
        assert len(out.vertices) == 0 and out.faces.shape == (0, 3)
    if keep == "alternating":
        assert (out.faces == [[0, 1, 2], [3, 4, 0]]).all()                      # by hand: vertices 0 2 4 6 8 all stay


def test_cull_mesh_rejects_a_wrong_mask():
    from cnr_amd import raster
    with pytest.raises(ValueError):
        raster.cull_mesh(_mesh_with_unused_vertices(), np.ones(5, bool))
    with pytest.raises(ValueError):
        raster.cull_mesh(_mesh_with_unused_vertices(), np.array([4]))


# ---- depth L1 --------------------------------------------------------------------------------------------------------------
def test_depth_l1_bookkeeping():
    from cnr_amd import metrics
    rec = np.array([[[0.0, 1.0, 2.0], [0.0, 3.0, 0.0]], [[1.5, 0.0, 4.0], [2.0, 2.0, 0.0]]], np.float32)
    gt = np.array([[[0.0, 1.25, 0.0], [5.0, 2.0, 0.0]], [[1.0, 0.0, 4.0], [0.0, 2.5, 0.0]]], np.float32)
    total, both, only_rec, only_gt, neither = metrics.depth_l1_images(torch.from_numpy(rec), torch.from_numpy(gt))
    assert (both, only_rec, only_gt, neither) == (5, 2, 1, 4)                   # counted by hand
    assert total.dtype == torch.float64 and float(total) == 0.25 + 1.0 + 0.5 + 0.0 + 0.5
    ref = RC.depth_l1(rec, gt)
    assert ref == dict(l1=2.25 / 5, both=5, only_rec=2, only_gt=1, neither=4)
    total, both, *_ = metrics.depth_l1_images(torch.zeros(2, 3), torch.ones(2, 3))
    assert both == 0 and float(total) == 0.0 and np.isnan(RC.depth_l1(np.zeros((2, 3)), np.ones((2, 3)))["l1"])
    with pytest.raises(ValueError):
        metrics.depth_l1_images(torch.zeros(2, 3), torch.zeros(3, 2))


# ---- argument errors that need no GPU ----------------------------------------------------------------------------------------
def _cpu_rasterizer():
    from cnr_amd import raster
    return raster.MeshRasterizer.from_intrinsics(50, 37, 40.0, 40.0, 24.5, 18.0, 0.1, 10.0, device="cpu")


@pytest.mark.parametrize("shape", [(3, 4), (2, 4, 3), (2, 3, 4), (0, 4, 4), (16,), (1, 2, 4, 4)])
def test_wrong_pose_shape(shape):
    r = _cpu_rasterizer()
    with pytest.raises(ValueError, match="T_wc"):
        r.render(None, np.zeros(shape))
    with pytest.raises(ValueError, match="T_wc"):
        r.visible_faces(None, torch.zeros(shape))


def test_unknown_normal_mode():
    with pytest.raises(ValueError, match="normal"):
        _cpu_rasterizer().render(None, np.eye(4), normal="smooth")


@pytest.mark.parametrize("faces", [[[0, 1, 3]], [[0, -1, 2]]])
def test_faces_out_of_range(faces):
    from cnr_amd import raster
    with pytest.raises(ValueError, match="faces"):
        raster.MeshScene([(np.zeros((3, 3), np.float32), np.array(faces))], device="cpu")


def test_scene_argument_errors():
    from cnr_amd import raster
    tri = (np.eye(3, dtype=np.float32), np.array([[0, 1, 2]]))
    with pytest.raises(ValueError, match="labels"):
        raster.MeshScene([tri, tri], labels=[1], device="cpu")
    with pytest.raises(ValueError):
        raster.MeshScene([], device="cpu")
    with pytest.raises(ValueError, match="colors"):
        raster.MeshScene([(tri[0], tri[1], np.zeros((2, 3)))], device="cpu")
    with pytest.raises(ValueError):
        raster.MeshRasterizer.from_intrinsics(50, 37, 40.0, 40.0, 24.5, 18.0, -0.1, 10.0, device="cpu")


def test_scene_concatenates_on_the_host_side():
    """offsets, labels and the colour scale, on a CPU 'device' (no kernel runs)"""
    from cnr_amd import raster
    from cnr_amd.vis import Mesh
    m = Mesh(np.eye(3), [[0, 1, 2]])
    m.visual.vertex_colors = [255, 0, 51]
    tri = (np.eye(3, dtype=np.float32) * 2, torch.tensor([[0, 1, 2], [2, 1, 0]]))
    s = raster.MeshScene([m, tri], labels=[7, 3], device="cpu")
    assert s.faces.dtype == torch.int32 and s.faces.tolist() == [[0, 1, 2], [3, 4, 5], [5, 4, 3]]
    assert s.face_label.tolist() == [7, 3, 3] and s.face_mesh.tolist() == [0, 1, 1] and s.face_offsets == [0, 1, 3]
    assert s.colors[0].tolist() == [1.0, 0.0, pytest.approx(0.2)] and s.colors[3].tolist() == [pytest.approx(0.4)] * 3
    assert raster.MeshScene(m, device="cpu").n_faces == 1 and raster.MeshScene(tri, device="cpu").n_faces == 2
    area = raster.observed_area(s, [True, False, True])
    assert area[0] == (pytest.approx(np.sqrt(3) / 2), pytest.approx(np.sqrt(3) / 2))
    assert area[1] == (pytest.approx(2 * np.sqrt(3)), pytest.approx(4 * np.sqrt(3)))


def test_entry_points_refuse_bad_arguments():
    """codes, before anything touches a device: the library loads without a GPU"""
    import cnr_amd
    lib = cnr_amd._C.load()
    # 20 items: 1600 -> 1792 B of records, 160 -> 256 B of boxes; 7 x 5 tiles x 2 views: 280 -> 512 B counts, 512 B cursors, 560 -> 768 B starts
    assert lib.cnr_raster_workspace_bytes(10, 2, 50, 37) == 1792 + 256 + 512 + 512 + 768
    for F, V, W, H in ((0, 1, 50, 37), (10, 0, 50, 37), (10, 1, 0, 37), (10, 1, 50, 40000), (1 << 31, 1, 50, 37), (1 << 30, 1 << 12, 50, 37),
                       (10, 1 << 20, 32768, 32768)):
        assert lib.cnr_raster_workspace_bytes(F, V, W, H) == -2, (F, V, W, H)
    assert lib.cnr_raster_visible_workspace_bytes(10, 3) == 256 and lib.cnr_raster_visible_workspace_bytes(0, 3) == -2
    assert lib.cnr_raster_bin_count(None, None, 10, None, 1, 50, 37, 40.0, 40.0, 24.5, 18.0, -0.1, 0, None, None, None) == -1
    assert lib.cnr_raster_bin_emit(10, 1, 50, 37, None, None, None) == -1
    assert lib.cnr_raster_tiles(None, 10, 1, 50, 37, 0.1, 10.0, None, None, None, None, None, None) == -1
    assert lib.cnr_raster_attributes(None, None, None, None, None, None, None, 10, 1, 50, 37, 0, None, None, None, None, None, None) == -1
    assert lib.cnr_raster_visible(None, None, None, 0.0, 10, 1, 50, 37, None, None, None, None) == -1
