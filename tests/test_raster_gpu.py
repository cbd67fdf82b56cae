"""GPU: the mesh rasteriser (csrc/raster.hip through cnr_amd.raster) against the numpy restatement tests/raster_cpu.py, which
tests/test_raster_host.py holds to a brute-force intersection.  ``face`` and ``instance`` must be equal everywhere and ``depth``
bit-equal to float32 of the restatement's fp64 t: both sides evaluate the same IEEE sequence.  ``bary``, ``rgb`` and ``normal``
must lie within one fp32 spacing."""
import os

import numpy as np
import pytest
import torch

import raster_cpu as RC
from test_raster_host import dyadic_cases

pytestmark = pytest.mark.gpu


def rasterizer(dev, cam):
    from cnr_amd import raster
    r = raster.MeshRasterizer.from_intrinsics(cam["W"], cam["H"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["zmin"],
                                              cam["zmax"], device=dev)
    want = RC.pinhole_dirs(cam["W"], cam["H"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    assert r.dirs().cpu().numpy().tobytes() == want.tobytes()          # the ray table both sides widen to fp64
    return r


def np_(t):
    return t.detach().cpu().numpy()


def within_one_spacing(got, ref64):
    ref64 = np.asarray(ref64, np.float64)
    return (np.abs(np_(got).astype(np.float64) - ref64) <= np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)).all()


def assert_is_restatement(res, ref):
    assert (np_(res["face"]) == ref["face"]).all()
    assert np_(res["depth"]).tobytes() == ref["depth"].tobytes()
    assert within_one_spacing(res["bary"], ref["bary"])
    assert (np_(res["opacity"]) == (ref["face"] >= 0)).all()


def restate(rast, cam, verts, faces, T_wc, **kw):
    return RC.rasterize(verts, faces, np.linalg.inv(T_wc), np_(rast.dirs()), cam["W"], cam["H"], cam["zmin"], cam["zmax"], **kw)


# ---- 1, 6: the random soup ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def soups():
    """{pose: (verts, faces, T_wc, colors, normals)}: the soup before the camera at the identity and at a random rigid pose"""
    out = {}
    rng = np.random.default_rng(23)
    for pose in ("identity", "rigid"):
        verts, faces = RC.soup()
        T = np.eye(4) if pose == "identity" else RC.random_rigid()
        if pose == "rigid":
            verts = (verts.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
        out[pose] = (verts, faces, T, rng.uniform(0, 1, verts.shape).astype(np.float32), rng.normal(size=verts.shape).astype(np.float32))
    return out


@pytest.mark.parametrize("pose", ["identity", "rigid"])
def test_soup(dev, soups, pose):
    from cnr_amd import raster
    verts, faces, T, _, _ = soups[pose]
    rast = rasterizer(dev, RC.SOUP_CAM)
    res = rast.render(raster.MeshScene((verts, faces), device=dev), T, attributes=False)
    ref = restate(rast, RC.SOUP_CAM, verts, faces, T)
    assert (ref["margin"] < 1e-9).sum() <= 0.001 * ref["face"].size
    assert_is_restatement(res, ref)
    assert (ref["face"] >= 0).mean() > 0.2 and tuple(res["depth"].shape) == (50, 37)


@pytest.mark.parametrize("mode", ["face", "vertex"])
@pytest.mark.parametrize("pose", ["identity", "rigid"])
def test_attributes(dev, soups, pose, mode):
    from cnr_amd import raster
    verts, faces, T, colors, normals = soups[pose]
    half = len(faces) // 2          # two meshes over one vertex array each: labels 5 and 9
    parts = [(verts, faces[:half], colors, normals), (verts, faces[half:], colors, normals)]
    scene = raster.MeshScene(parts, labels=[5, 9], device=dev)
    rast = rasterizer(dev, RC.SOUP_CAM)
    res = rast.render(scene, T, normal=mode)
    v2, f2 = np.concatenate([verts, verts]), np.concatenate([faces[:half], faces[half:] + len(verts)])
    label = np.array([5] * half + [9] * (len(faces) - half))
    ref = restate(rast, RC.SOUP_CAM, v2, f2, T)
    assert_is_restatement(res, ref)
    rgb, inst, nrm = RC.attributes(v2, f2, np.concatenate([colors, colors]), np.concatenate([normals, normals]), label,
                                   np.linalg.inv(T), np_(rast.dirs()), ref["face"], normal=mode)
    assert (np_(res["instance"]) == inst).all() and set(np.unique(inst)) == {-1, 5, 9}
    assert within_one_spacing(res["rgb"], rgb) and within_one_spacing(res["normal"], nrm)
    hit = ref["face"] >= 0
    n = np_(res["normal"]).astype(np.float64)
    assert np.abs(np.linalg.norm(n[hit], axis=-1) - 1).max() < 1e-6 and (n[~hit] == 0).all() and (np_(res["rgb"])[~hit] == 0).all()
    if mode == "face":              # towards the camera: n . d_world < 0
        d_world = np_(rast.dirs()).astype(np.float64).reshape(50, 37, 3) @ T[:3, :3].T
        assert ((n * d_world).sum(-1)[hit] < 0).all()


# ---- 2: dyadic cases, every quantity exact: the images are written out by hand ---------------------------------------------
@pytest.mark.parametrize("case", dyadic_cases(), ids=lambda c: c["name"])
def test_dyadic(dev, case):
    from cnr_amd import raster
    rast = rasterizer(dev, RC.DYADIC_CAM)
    res = rast.render(raster.MeshScene((case["verts"], case["faces"]), device=dev), np.eye(4), attributes=False,
                      cull_backfaces=case["cull"])
    assert (np_(res["face"]) == case["face"]).all()
    assert np_(res["depth"]).tobytes() == case["depth"].tobytes()


# ---- 3: the wall: the tile box of a face with a corner behind the camera must stay conservative ------------------------------
def test_wall(dev):
    from cnr_amd import raster
    verts = np.array([[-100, -100, 3], [100, -100, 3], [0, 100, 3],
                      [-80, 0.31, 2], [80, 0.31, 2], [0, 100, -1]], np.float32)
    faces = np.array([[0, 1, 2], [3, 4, 5]])
    rast = rasterizer(dev, RC.SOUP_CAM)
    for T in (np.eye(4), RC.look_at([0.3, -0.2, -0.5], [0.1, 0.3, 2.0], up=(0.0, -1.0, 0.2))):
        res = rast.render(raster.MeshScene((verts, faces), device=dev), T, attributes=False)
        ref = restate(rast, RC.SOUP_CAM, verts, faces, T)
        assert (ref["face"] >= 0).all() and set(np.unique(ref["face"])) == {0, 1}
        assert_is_restatement(res, ref)


# ---- min_depth = 0, as the datasets' configs carry it: the tile box cannot come from a cut at z >= 0 -----------------------------
def test_zero_min_depth(dev):
    from cnr_amd import raster
    cam = dict(RC.SOUP_CAM, zmin=0.0)
    rast = rasterizer(dev, cam)
    verts, faces = RC.soup()
    # ... and with a face in the plane z = 2^-15 + x, which every pixel sees about 2^-15 before the camera centre; the part of it
    # that can be projected (z >= 2^-13) lies beyond the image's right edge
    e = 2.0 ** -15
    near = np.array([[-1, -1, e - 1], [1, -1, e + 1], [0, 2, e]], np.float32)
    for v, f in ((verts, faces), (np.concatenate([verts, near]), np.concatenate([faces, [[360, 361, 362]]]))):
        res = rast.render(raster.MeshScene((v, f), device=dev), np.eye(4), attributes=False)
        ref = restate(rast, cam, v, f, np.eye(4))
        assert_is_restatement(res, ref)
        if len(f) > len(faces):
            assert (ref["face"] == 120).all() and 0 < ref["depth"].max() < 2.0 ** -13
        else:
            assert (ref["face"] >= 0).mean() > 0.2


# ---- 4: a tile list longer than any LDS chunk, and no multiple of it ---------------------------------------------------------
@pytest.mark.parametrize("depths", ["distinct", "equal"])
def test_long_tile_list(dev, depths):
    from cnr_amd import raster
    n = 700
    perm = np.random.default_rng(7).permutation(n)
    z = 1.0 + perm / 256.0 if depths == "distinct" else np.full(n, 2.0)
    verts = np.array([[RC.dyadic_point(15, 7, zi), RC.dyadic_point(33, 7, zi), RC.dyadic_point(15, 25, zi)] for zi in z])
    verts = verts.reshape(-1, 3).astype(np.float32)
    faces = np.arange(3 * n).reshape(n, 3)
    cam = RC.DYADIC_CAM
    rast = rasterizer(dev, cam)
    res = rast.render(raster.MeshScene((verts, faces), device=dev), np.eye(4), attributes=False)
    winner = int(np.argmin(perm)) if depths == "distinct" else 0
    face, depth = np.full((cam["W"], cam["H"]), -1, np.int32), np.zeros((cam["W"], cam["H"]), np.float32)
    for w in range(15, cam["W"]):
        for h in range(7, cam["H"]):
            if (w - 15) + (h - 7) <= 18:
                face[w, h], depth[w, h] = winner, z[winner]
    assert (face[16:24, 8:16] == winner).all()                       # the whole of tile (2, 1) lies under the stack
    assert (np_(res["face"]) == face).all() and np_(res["depth"]).tobytes() == depth.tobytes()
    assert_is_restatement(res, restate(rast, cam, verts, faces, np.eye(4)))
    assert rast.pairs >= n and n % 64 != 0


# ---- 5, 7: many (view, face) items: a marching-cubes sphere from 12 poses ----------------------------------------------------
SPHERE_CAM = dict(W=96, H=64, fx=110.0, fy=110.0, cx=47.5, cy=31.5, zmin=0.1, zmax=10.0)


def restate_blocked(dirs, cam, verts, faces, T_wc, block=16):
    """the restatement block of pixels by block of pixels, each against the faces whose bounding sphere can meet the block's
    cone of rays (angle between the face centre and the block's central ray <= the cone's half angle + the sphere's angular
    radius, with 5 % and 1e-3 rad to spare); every other face cannot cover a pixel of the block"""
    W, H = cam["W"], cam["H"]
    T_cw = np.linalg.inv(T_wc)
    p = verts.astype(np.float64)[faces] @ T_cw[:3, :3].T + T_cw[:3, 3]
    c = p.mean(1)
    rad = np.linalg.norm(p - c[:, None], axis=-1).max(1)
    dist = np.linalg.norm(c, axis=-1)
    ang_r = np.where(dist > rad, np.arcsin(np.minimum(rad / np.maximum(dist, 1e-300), 1.0)), np.pi)
    d3 = dirs.astype(np.float64).reshape(W, H, 3)
    out = dict(face=np.full((W, H), -1, np.int32), depth=np.zeros((W, H), np.float32), bary=np.zeros((W, H, 2)),
               t=np.full((W, H), np.inf), margin=np.full((W, H), np.inf))
    for w0 in range(0, W, block):
        for h0 in range(0, H, block):
            d = d3[w0:w0 + block, h0:h0 + block].reshape(-1, 3)
            u = d / np.linalg.norm(d, axis=-1, keepdims=True)
            mid = u.mean(0) / np.linalg.norm(u.mean(0))
            cone = np.arccos(np.clip(u @ mid, -1, 1)).max()
            ang_c = np.arccos(np.clip(c @ mid / np.maximum(dist, 1e-300), -1, 1))
            ids = np.nonzero(ang_c <= 1.05 * (cone + ang_r) + 1e-3)[0]
            r = RC.rasterize(verts, faces, T_cw, d.astype(np.float32), len(d), 1, cam["zmin"], cam["zmax"], face_ids=ids)
            bw, bh = min(block, W - w0), min(block, H - h0)
            for k in out:
                out[k][w0:w0 + bw, h0:h0 + bh] = r[k].reshape(bw, bh, *r[k].shape[2:])
    return out


@pytest.fixture(scope="module")
def sphere(dev):
    """the sphere mesh, its scene, 12 ring poses, the 12 views in one call and the restatement of views 0 and 7"""
    from cnr_amd import raster, vis
    with torch.cuda.device(dev):
        mesh = vis.marching_cubes(RC.sphere_volume(64, 0.47))
    poses = RC.ring_poses(12, 2.0, 0.6)
    scene = raster.MeshScene(mesh, device=dev)
    rast = rasterizer(dev, SPHERE_CAM)
    res = rast.render(scene, poses, attributes=False, views_per_launch=12)
    verts, faces = mesh.vertices.astype(np.float32), mesh.faces
    refs = {v: restate_blocked(np_(rast.dirs()), SPHERE_CAM, verts, faces, poses[v]) for v in (0, 7)}
    return dict(mesh=mesh, scene=scene, rast=rast, poses=poses, res=res, refs=refs)


def test_sphere_views_are_the_restatement(sphere):
    F = sphere["scene"].n_faces
    assert 12 * F > 262144, F                 # more items than one pass of a 1024-thread scan over blocks of 256 holds
    assert tuple(sphere["res"]["face"].shape) == (12, 96, 64)
    for v, ref in sphere["refs"].items():
        assert (ref["face"] >= 0).sum() > 1000
        assert_is_restatement({k: t[v] for k, t in sphere["res"].items()}, ref)


def test_sphere_batching_does_not_matter(sphere):
    rast, scene, poses, res = sphere["rast"], sphere["scene"], sphere["poses"], sphere["res"]
    same = lambda a, b: all(np_(a[k]).tobytes() == np_(b[k]).tobytes() for k in ("face", "depth", "bary"))
    single = [rast.render(scene, poses[v], attributes=False) for v in range(12)]
    assert tuple(single[0]["depth"].shape) == (96, 64)
    assert same({k: torch.stack([s[k] for s in single]) for k in ("face", "depth", "bary")}, res)
    for step in (1, 5, 12):                   # 12 again: a second run is bitwise the first
        assert same(rast.render(scene, poses, attributes=False, views_per_launch=step), res), step


def test_visibility(sphere):
    from cnr_amd import raster
    rast, scene, poses, res, mesh = sphere["rast"], sphere["scene"], sphere["poses"], sphere["res"], sphere["mesh"]
    F = scene.n_faces
    seen, count = rast.visible_faces(scene, poses, views_per_launch=5)
    ref_seen, ref_count = RC.visible(np_(res["face"]), np_(res["depth"]), F)
    assert seen.dtype == torch.bool and count.dtype == torch.int32
    assert (np_(seen) == ref_seen).all() and (np_(count) == ref_count).all()
    assert 0 < int(seen.sum()) < F and int(count.max()) > 1          # the far sides of the poles stay unseen
    # from the restated face images of two of the poses
    two = [0, 7]
    s2, c2 = rast.visible_faces(scene, poses[two])
    r2 = RC.visible(np.stack([sphere["refs"][v]["face"] for v in two]), np.stack([sphere["refs"][v]["depth"] for v in two]), F)
    assert (np_(s2) == r2[0]).all() and (np_(c2) == r2[1]).all()
    area = raster.observed_area(scene, seen)[0]
    assert 0 < area[0] < area[1] and abs(area[1] - 4 * np.pi * 0.47 ** 2) < 0.05 * area[1]
    # the culled mesh looks the same from the same poses
    culled = raster.cull_mesh(mesh, seen)
    assert len(culled.faces) == int(seen.sum())
    again = rast.render(raster.MeshScene(culled, device=scene.device), poses, attributes=False)
    assert np_(again["depth"]).tobytes() == np_(res["depth"]).tobytes()


def test_visibility_behind_an_occluder(sphere):
    from cnr_amd import raster
    rast, scene, poses, res = sphere["rast"], sphere["scene"], sphere["poses"], sphere["res"]
    F, three = scene.n_faces, [11, 0, 1]
    # a plate between camera 0 and the sphere, smaller than the sphere's outline; the frames' depth is the plate where it is
    # seen and a far wall elsewhere
    plate = (np.array([[1.5, 0.3, 0.5], [1.5, 0.7, 0.5], [1.5, 0.7, 0.9], [1.5, 0.3, 0.9]], np.float32), np.array([[0, 1, 2], [0, 2, 3]]))
    d_plate = rast.render(raster.MeshScene(plate, device=scene.device), poses[three], attributes=False)["depth"]
    obs = torch.where(d_plate > 0, d_plate, torch.full_like(d_plate, 9.0))
    assert int((d_plate > 0).sum()) > 100
    free_seen, free_count = rast.visible_faces(scene, poses[three])
    for tol, back in ((0.0, False), (5.0, True)):
        seen, count = rast.visible_faces(scene, poses[three], depth_obs=obs, tol=tol)
        ref = RC.visible(np_(res["face"])[three], np_(res["depth"])[three], F, depth_obs=np_(obs), tol=tol)
        assert (np_(seen) == ref[0]).all() and (np_(count) == ref[1]).all()
        if back:
            assert (seen == free_seen).all() and (count == free_count).all()
        else:
            assert int(seen.sum()) < int(free_seen.sum()) and not (seen & ~free_seen).any()
    # no observed depth at all: nothing counts
    seen, count = rast.visible_faces(scene, poses[three], depth_obs=torch.zeros_like(obs), tol=5.0)
    assert not seen.any() and not count.any()


# ---- 8: depth L1 -------------------------------------------------------------------------------------------------------------
def test_depth_l1(dev):
    from cnr_amd import metrics, vis
    cam = dict(W=48, H=32, fx=60.0, fy=60.0, cx=23.5, cy=15.5, zmin=0.1, zmax=10.0)
    rast = rasterizer(dev, cam)
    meshes = []
    with torch.cuda.device(dev):
        for r in (0.25, 0.3):             # radii 0.5 and 0.6 around the origin
            meshes.append(vis.marching_cubes(RC.sphere_volume(32, r)).apply_translation([-0.5] * 3).apply_scale(2.0))
    poses = RC.ring_poses(3, 3.0, 1.0, target=(0.0, 0.0, 0.0))
    got = metrics.depth_l1(meshes[0], meshes[1], poses, rast, views_per_launch=2)
    depth = [np.stack([restate(rast, cam, m.vertices.astype(np.float32), m.faces, T)["depth"] for T in poses]) for m in meshes]
    ref = RC.depth_l1(depth[0], depth[1])
    print("depth L1", got, "restatement", ref)
    assert {k: got[k] for k in ("both", "only_rec", "only_gt", "neither")} == {k: ref[k] for k in ("both", "only_rec", "only_gt", "neither")}
    assert ref["both"] > 300 and ref["only_gt"] > 0 and ref["only_rec"] == 0 and ref["neither"] > 0
    assert abs(got["l1"] - ref["l1"]) <= 1e-6 * ref["l1"]
    # along the central ray the spheres are 0.1 apart and every other ray crosses the shell more obliquely; the marching-cubes
    # surfaces lie within h^2 / (8 r) < 0.002 of their spheres (chord sag of the h = 2 / 31 lattice at r = 0.5), hence 0.005;
    # from above, no pixel can exceed the restatement's own largest difference, which is met towards the silhouette
    both = (depth[0] > 0) & (depth[1] > 0)
    assert 0.1 - 0.005 <= got["l1"] <= np.abs(depth[0].astype(np.float64) - depth[1])[both].max()
    # and when nothing is hit in both: nan, no exception
    away = RC.look_at([0.0, 0.0, 3.0], [0.0, 0.0, 6.0], up=(0.0, 1.0, 0.0))
    empty = metrics.depth_l1(meshes[0], meshes[1], away[None], rast)
    assert empty["both"] == 0 and np.isnan(empty["l1"]) and empty["neither"] == 48 * 32


# ---- 9: a single-view result is a SceneRenderer result -------------------------------------------------------------------------
def test_result_goes_through_the_view_tools(dev, soups, tmp_path):
    from PIL import Image
    from cnr_amd import raster, view
    verts, faces, T, colors, normals = soups["rigid"]
    rast = rasterizer(dev, RC.SOUP_CAM)
    res = rast.render(raster.MeshScene((verts, faces, colors, normals), device=dev), T)
    view.render_to_files(res, str(tmp_path))
    shade = view.shade(res, T)
    assert tuple(shade.shape) == (50, 37, 3) and float(shade.max()) > 0.1 and float(shade.min()) >= 0.0
    mm = np.array(Image.open(os.path.join(str(tmp_path), "depth.png")))
    depth = np_(res["depth"])
    assert mm.shape == (37, 50) and (mm.T == np.round(depth.astype(np.float64) * 1000)).all() and (depth > 0).sum() > 300
    for name in ("rgb.png", "instance.png", "normal.png"):
        assert Image.open(os.path.join(str(tmp_path), name)).size == (50, 37)
