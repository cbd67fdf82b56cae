"""Host: devmesh.device_mesh on a CPU 'device' (no kernel runs) -- the same mesh through every door, the soup form, the
attributes raster.MeshScene asks for, and every refusal the host-side index check makes."""
import numpy as np
import pytest
import torch

VERTS = np.array([[0.1, 0.2, 0.3], [1.0, 0.0, 1.0 / 3.0], [0.0, 1.0, 2.0 / 3.0], [1.0, 1.0, 1e-9], [0.5, 0.5, 2.0]])   # float64
FACES = np.array([[0, 1, 2], [1, 3, 2], [2, 3, 4]], np.int64)


@pytest.fixture(scope="module")
def dm():
    from cnr_amd import devmesh
    return devmesh


def _doors():
    from cnr_amd.vis import Mesh
    return dict(mesh=Mesh(VERTS, FACES), numpy=(VERTS, FACES),
                tensor_i32=(torch.from_numpy(VERTS), torch.from_numpy(FACES.astype(np.int32))),
                tensor_i64=(torch.from_numpy(VERTS), torch.from_numpy(FACES)))


def test_every_door_gives_the_same_mesh(dm):
    assert VERTS.dtype == np.float64 and (VERTS.astype(np.float32).astype(np.float64) != VERTS).any()     # the rounding is seen
    for name, mesh in _doors().items():
        d = dm.device_mesh(mesh, device="cpu")
        assert isinstance(d, dm.DeviceMesh) and d.device == torch.device("cpu"), name
        assert d.verts.dtype == torch.float32 and d.verts.is_contiguous() and tuple(d.verts.shape) == (5, 3), name
        assert np.array_equal(d.verts.numpy(), np.float32(VERTS)), name                                  # rounded exactly once
        assert d.faces.dtype == torch.int32 and d.faces.is_contiguous() and np.array_equal(d.faces.numpy(), FACES), name
        assert d.n_faces == 3 and d.colors is None and d.normals is None, name
        assert dm.device_mesh(d, device="cpu") is d and dm.device_mesh(d) is d, name


def test_soup_and_empty_meshes(dm):
    soup = VERTS[FACES].reshape(-1, 3)
    d = dm.device_mesh((soup, None), device="cpu")
    assert d.faces is None and d.n_faces == len(soup) // 3 == 3 and np.array_equal(d.verts.numpy(), np.float32(soup))
    for empty in (np.zeros((0, 3)), np.zeros(0), np.zeros((3, 0))):
        e = dm.device_mesh((empty, np.zeros(empty.shape, np.int64)), device="cpu")
        assert tuple(e.verts.shape) == (0, 3) and tuple(e.faces.shape) == (0, 3) and e.n_faces == 0
    assert dm.device_mesh((VERTS, np.zeros((0, 3), np.int64)), device="cpu").n_faces == 0


def test_attributes(dm):
    from cnr_amd.vis import Mesh
    m = Mesh(VERTS, FACES, vertex_normals=np.tile([0.0, 0.0, 1.0], (5, 1)))
    m.visual.vertex_colors = [255, 0, 51]
    d = dm.device_mesh(m, device="cpu", attributes=True)
    assert d.colors.dtype == torch.float32 and d.normals.dtype == torch.float32
    assert np.array_equal(d.colors.numpy()[:, :2], np.tile(np.float32([1.0, 0.0]), (5, 1)))
    assert np.array_equal(d.colors.numpy()[:, 2], np.full(5, np.float32(51) / np.float32(255))) and abs(float(d.colors[0, 2]) - 0.2) < 1e-7
    assert np.array_equal(d.normals.numpy(), np.tile(np.float32([0.0, 0.0, 1.0]), (5, 1)))
    t = dm.device_mesh((VERTS, FACES), device="cpu", attributes=True)
    assert np.array_equal(t.colors.numpy(), np.full((5, 3), np.float32(102.0 / 255.0))) and not t.normals.any()
    given = dm.device_mesh((VERTS, FACES, np.full((5, 3), 0.25), None), device="cpu", attributes=True)
    assert np.array_equal(given.colors.numpy(), np.full((5, 3), np.float32(0.25))) and not given.normals.any()
    plain = dm.device_mesh((VERTS, FACES), device="cpu")
    up = dm.device_mesh(plain, device="cpu", attributes=True)            # a DeviceMesh without attributes gains the defaults
    assert up is not plain and torch.equal(up.verts, plain.verts) and torch.equal(up.colors, t.colors)
    assert dm.device_mesh(up, device="cpu", attributes=True) is up


def _with_last_corner(value, dtype=np.int64):
    f = FACES.astype(dtype)
    f[-1, -1] = value
    return f


REFUSED = {
    "index == V": lambda: (VERTS, _with_last_corner(len(VERTS))),
    "index -1": lambda: (VERTS, _with_last_corner(-1)),
    "int64 2^32 (wraps to 0 as int32)": lambda: (VERTS, _with_last_corner(2 ** 32)),
    "int64 2^32, a tensor": lambda: (torch.from_numpy(VERTS), torch.from_numpy(_with_last_corner(2 ** 32))),
    "float faces": lambda: (VERTS, FACES.astype(np.float64)),
    "float faces, a tensor": lambda: (torch.from_numpy(VERTS), torch.from_numpy(FACES).float()),
    "flat faces": lambda: (VERTS, FACES.reshape(-1)),
    "flat verts": lambda: (VERTS.reshape(-1), FACES),
    "(F,4) faces": lambda: (VERTS, np.zeros((2, 4), np.int64)),
    "a soup of 5 rows": lambda: (VERTS, None),
    "neither a mesh nor a tuple": lambda: VERTS,
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusals_are_value_errors_that_name_the_caller(dm, case):
    with pytest.raises(ValueError, match="^the caller: "):
        dm.device_mesh(REFUSED[case](), device="cpu", what="the caller")


def test_attribute_shapes_are_checked(dm):
    for bad in ((VERTS, FACES, np.zeros((4, 3))), (VERTS, FACES, None, np.zeros((5, 2))), (VERTS, FACES, np.zeros(15))):
        with pytest.raises(ValueError, match="colors"):
            dm.device_mesh(bad, device="cpu", attributes=True)


def test_check_false_skips_the_range_check_only(dm):
    for value in (len(VERTS), -1):
        f = _with_last_corner(value)
        d = dm.device_mesh((VERTS, f), device="cpu", check=False)
        assert np.array_equal(d.faces.numpy(), f) and d.faces.dtype == torch.int32
    with pytest.raises(ValueError):
        dm.device_mesh((VERTS, FACES.astype(np.float32)), device="cpu", check=False)
    with pytest.raises(ValueError):
        dm.device_mesh((VERTS, FACES.reshape(-1)), device="cpu", check=False)


def test_require_finite_and_exports(dm):
    import cnr_amd
    assert cnr_amd.devmesh is dm and set(dm.__all__) == {"DeviceMesh", "device_mesh", "check_faces", "require_finite"}
    dm.require_finite(torch.zeros(4, 3), "x")
    for bad in (float("inf"), float("nan")):
        t = torch.zeros(4, 3)
        t[3, 2] = bad
        with pytest.raises(ValueError, match="^x: "):
            dm.require_finite(t, "x")
    with pytest.raises(cnr_amd._C.CnrError):                             # the device-side check has no CPU path
        dm.check_faces(torch.zeros(4, 3, dtype=torch.int32), 12, "x")
