"""GPU: devmesh's device-side index check at the sizes where check_faces_kernel can go wrong, and one mesh through every door
of devmesh.device_mesh into the modules that take a mesh: the results are equal bit for bit."""
import numpy as np
import pytest
import torch

import mc_cpu as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cnr():
    import cnr_amd
    return cnr_amd


# 3 F = 3, 255 and 258 straddle one 256-thread block of check_faces_kernel; 3 x 699051 = 2097153 is one entry past its grid of
# 8192 blocks, so the last entry -- the one the bad index sits in -- is read on the grid-stride loop's second trip
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("F", [1, 85, 86, 699051])
def test_device_resident_faces_are_checked_on_the_device(cnr, dev, F, dtype):
    dm = cnr.devmesh
    V = F + 2
    strip = torch.arange(F, device=dev, dtype=dtype)[:, None] + torch.arange(3, device=dev, dtype=dtype)     # face i = (i, i+1, i+2)
    assert 3 * F in (3, 255, 258, 8192 * 256 + 1) and int(strip[-1, -1]) == V - 1
    verts = torch.zeros(V, 3, device=dev)
    d = dm.device_mesh((verts, strip), what="strip")
    assert d.device == dev and d.n_faces == F and d.faces.dtype == torch.int32 and d.faces.is_contiguous()
    assert torch.equal(d.faces, strip.to(torch.int32)) and torch.equal(dm.check_faces(strip, V, "strip"), d.faces)
    bad_values = [V, -1] + ([2 ** 32] if dtype == torch.int64 else [])                 # 2^32 would wrap to 0 as int32
    for bad in bad_values:
        f = strip.clone()
        f[-1, -1] = bad
        with pytest.raises(ValueError, match="^strip: "):
            dm.device_mesh((verts, f), what="strip")
        with pytest.raises(ValueError, match="^strip: "):
            dm.check_faces(f, V, "strip")
        if bad != 2 ** 32:
            assert torch.equal(dm.device_mesh((verts, f), check=False).faces, f.to(torch.int32))


# ---- one mesh through every door ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def doors(cnr, dev):
    mesh = cnr.vis.marching_cubes(M.two_spheres(32))
    mesh.apply_translation([-0.5, -0.5, -0.5]).apply_scale(2.0)
    assert mesh.vertices.dtype == np.float64 and mesh.faces.dtype == np.int64 and len(mesh.faces) > 1000
    return mesh, dict(mesh=mesh, numpy=(mesh.vertices, mesh.faces),
                      device_tensors=(torch.from_numpy(mesh.vertices).to(dev), torch.from_numpy(mesh.faces).to(dev)),
                      device_mesh=cnr.devmesh.device_mesh(mesh, dev))


def _all_equal(results):
    first = results[0]
    for other in results[1:]:
        assert len(first) == len(other) and all(torch.equal(a, b) for a, b in zip(first, other))


def test_metrics_take_every_door(cnr, dev, doors):
    mesh, forms = doors
    mt = cnr.metrics
    g = torch.Generator(device=dev).manual_seed(4)
    q = torch.rand(3000, 3, device=dev, generator=g) * 2 - 1
    brute = [mt.point_mesh_distance(q, m, closest=True) for m in forms.values()]
    _all_equal(brute)
    indexed = [mt.point_mesh_distance(q, m, closest=True, index=True) for m in forms.values()]
    _all_equal(indexed + brute[:1])                                                    # and the index agrees with the brute force
    _all_equal([(mt.sample_surface(m, 4000, seed=3),) for m in forms.values()])
    gt = cnr.vis.Mesh(mesh.vertices * 1.02, mesh.faces)
    scores = [mt.calc_3d_metric(m, gt, N=4000, mesh_gt=(gt.vertices, gt.faces) if name != "mesh" else None)
              for name, m in forms.items()]
    assert scores[0] is not None and all(s == scores[0] for s in scores), scores


def test_mesh_scene_takes_every_door(cnr, dev, doors):
    mesh, forms = doors
    scenes = [cnr.raster.MeshScene(m, device=dev) for m in forms.values()]
    _all_equal([(s.verts, s.faces, s.colors) for s in scenes])
    assert scenes[0].n_faces == len(mesh.faces) and torch.equal(scenes[0].faces.cpu(), torch.from_numpy(mesh.faces).int())
    both = cnr.raster.MeshScene([forms["device_tensors"], forms["mesh"]], device=dev)   # offsets on the device
    V, F = len(mesh.vertices), len(mesh.faces)
    assert torch.equal(both.faces[F:], scenes[0].faces + V) and torch.equal(both.verts[V:], scenes[0].verts)


def test_clean_and_simplify_mesh_equal_the_tensor_level_calls(cnr, dev, doors):
    mesh, forms = doors
    mo, d = cnr.meshops, forms["device_mesh"]
    out, report = mo.clean_mesh(mesh, keep_largest=1, device=dev)
    faces, kept, report_d = mo.clean_device(d.verts, d.faces, keep_largest=1)
    idx = kept.cpu().numpy().astype(np.int64)
    assert report["n_components"] == report_d["n_components"] == 2 and 0 < len(out.faces) < len(mesh.faces)
    assert np.array_equal(out.faces, faces.cpu().numpy()) and np.array_equal(out.vertices, mesh.vertices[idx])
    assert np.array_equal(out.vertex_normals, mesh.vertex_normals[idx])
    cell = 4.0 / 31.0                                                                  # two voxels of the 32^3 grid
    small, rep = mo.simplify_mesh(mesh, cell=cell, device=dev)
    v, f, _, rep_d = mo.simplify(d.verts, d.faces, cell=cell)
    assert 0 < len(f) < len(mesh.faces) and rep["faces_out"] == rep_d["faces_out"] == len(f)
    assert np.array_equal(small.vertices, v.double().cpu().numpy()) and np.array_equal(small.faces, f.cpu().numpy())
    assert np.array_equal(small.vertex_normals, mo.vertex_normals(v, f).double().cpu().numpy())
