"""Host side of the scene view renderer's empty-space skipping: argument checks of build_grids / set_grids / render, entity
indices under edits, bit packing, and tests/viewgrid_cpu.py's float64 lookup on a hand-made 4^3 case.  No GPU."""
import numpy as np
import pytest
import torch

import view_cpu as V
import view_scene as VS
import viewgrid_cpu as VG


@pytest.fixture(scope="module")
def renderer():
    import cnr_amd as cnr
    cfg = VS.small_camera(cnr.cfg.synthetic_config(device="cpu", latent_dim=32))
    cls_dict, scene_bg = VS.make_scene(cnr, cfg, seed=2)
    return cnr, cnr.view.SceneRenderer(cls_dict, scene_bg, cfg)


@pytest.mark.parametrize("G", [0, 2, 6, 10, 130, 132, 256, 8.5])
def test_build_grids_refuses_a_bad_resolution(renderer, G):
    cnr, r = renderer
    with pytest.raises(ValueError, match="multiple of 4"):
        r.build_grids(resolution=G)


@pytest.mark.parametrize("kw", [dict(sub=0), dict(sub=5), dict(sub=1.5), dict(dilate=-1), dict(dilate=3)])
def test_build_grids_refuses_bad_sub_and_dilate(renderer, kw):
    cnr, r = renderer
    with pytest.raises(ValueError, match="sub must|dilate must"):
        r.build_grids(resolution=8, **kw)


def test_skip_empty_without_grids(renderer):
    cnr, r = renderer
    r.set_grids(None)
    assert r.grids() is None
    with pytest.raises(ValueError, match="build_grids"):
        r.render(VS.camera_pose(), n_samples=4, skip_empty=True)


def test_set_grids_refuses_wrong_shapes(renderer):
    cnr, r = renderer
    E = len(r.entities)
    assert E == 4
    r.set_grids(None)
    for shape in [(E - 1, 8, 8, 8), (E + 1, 8, 8, 8), (E, 8, 8), (E, 8, 8, 4), (E, 6, 6, 6), (E, 132, 132, 132), (E, 8, 8, 8, 1)]:
        with pytest.raises(ValueError):
            r.set_grids(torch.ones(shape, dtype=torch.bool))
    with pytest.raises(ValueError, match="bool"):
        r.set_grids(torch.ones(E, 8, 8, 8))
    with pytest.raises(ValueError):
        r.set_grids([None] * (E - 1))
    with pytest.raises(ValueError):
        r.set_grids([None] * E)
    with pytest.raises(ValueError):
        r.set_grids([torch.ones(4, 4, 4, dtype=torch.bool), torch.ones(8, 8, 8, dtype=torch.bool), None, None])
    assert r.grids() is None, "a refused call must leave no grids behind"


def test_set_grids_packs_and_grids_unpacks(renderer):
    cnr, r = renderer
    E, G = len(r.entities), 8
    bits = torch.rand(E, G, G, G, generator=torch.Generator().manual_seed(1)) < 0.5
    r.set_grids(bits)
    try:
        assert r._grids[0] == G and r._grids[1].dtype == torch.int32 and r._grids[1].shape == (E, G ** 3 // 32)
        assert np.array_equal(r._grids[1].numpy(), VG.pack(bits.numpy()))
        assert torch.equal(r.grids(), bits)
        assert torch.equal(cnr.view.unpack_grid_words(r._grids[1], G), bits)
        r.set_grids([bits[0], None, bits[2].numpy(), None])               # no grid: all set
        want = bits.clone()
        want[1], want[3] = True, True
        assert torch.equal(r.grids(), want) and r._grids[2] == [True, False, True, False]
    finally:
        r.set_grids(None)


def test_pack_puts_cell_l_at_bit_l_and_31_of_word_l_over_32():
    G = 4
    for l in (0, 1, 31, 32, 33, 63):
        bits = np.zeros(G ** 3, bool)
        bits[l] = True
        w = VG.pack(bits.reshape(G, G, G))
        want = np.zeros(2, np.uint32)
        want[l >> 5] = np.uint32(1) << np.uint32(l & 31)
        assert np.array_equal(w.view(np.uint32), want), l
        assert np.array_equal(VG.unpack(w, G).reshape(-1), bits)
    ix, iy, iz = 2, 1, 3                                                   # (ix G + iy) G + iz: z runs fastest
    bits = np.zeros((G, G, G), bool)
    bits[ix, iy, iz] = True
    assert np.nonzero(bits.reshape(-1))[0][0] == (ix * G + iy) * G + iz == 39
    assert VG.pack(bits).view(np.uint32)[1] == 1 << 7


def test_edited_keeps_entity_indices(renderer):
    cnr, r = renderer
    assert [e.index for e in r.entities] == [0, 1, 2, 3] and [e.inst_id for e in r.entities] == [0, 1, 2, 3]
    E = np.eye(4)
    E[:3, 3] = (0.3, 0.0, 0.1)
    ents = cnr.view.edited(r.entities, transforms={2: E}, hidden={1})
    assert [e.inst_id for e in ents] == [0, 2, 3] and [e.index for e in ents] == [0, 2, 3]
    assert not np.array_equal(ents[1].to_box, r.entities[2].to_box) and r.entities[2].index == 2
    ents = cnr.view.edited(r.entities, hidden={0, 3})
    assert [e.index for e in ents] == [1, 2]
    assert [e.index for e in cnr.view.edited(r.entities)] == [0, 1, 2, 3]


def test_lookup_on_a_hand_made_grid():
    """G = 4: cells are 0.5 wide in box coordinates.  One segment along the box's x axis at y = 0.25, z = -0.75, i.e. cells
    (., 2, 0); S = 4 samples between x = -1 and x = 1 at -0.75, -0.25, 0.25, 0.75: one in each cell along x."""
    G, S = 4, 4
    T = np.eye(4)
    T[:3, :3] = np.array([[0, 0, 1.0], [1.0, 0, 0], [0, 1.0, 0]])              # camera z -> world x, x -> y, y -> z
    T[:3, 3] = (-3.0, 0.25, -0.75)
    dirs = np.array([[0, 0, 1.0]], np.float32)
    to_box = np.stack([V.box_affine((0, 0, 0), np.eye(3), (1, 1, 1)), V.box_affine((0, 0, 0), np.eye(3), (1, 1, 1))])
    seg_pixel, seg_entity, seg_z = np.array([0, 0]), np.array([0, 1]), np.array([[2.0, 4.0], [2.0, 4.0]], np.float32)
    bits = np.zeros((1, G, G, G), bool)
    bits[0, 1, 2, 0] = bits[0, 3, 2, 0] = True
    bits[0, 2, 1, 0] = bits[0, 2, 2, 1] = bits[0, 0, 0, 2] = True               # neighbours in y and z: must not be hit
    active, near = VG.lookup(T, dirs, to_box, seg_pixel, seg_entity, seg_z, S, bits, np.array([0, -1]))
    assert active.tolist() == [[False, True, False, True], [True] * 4]           # the second entity has no grid
    assert not near.any()
    # a sample on a cell face is flagged; coordinates outside the box clamp to the border cells
    c, near = VG.cell_of(np.array([[0.5, 0.1, 0.1], [0.5 + 1e-6, 0.1, 0.1], [0.1, 0.1, 0.26], [-1.7, 1.3, 3.1], [-1.0, 0.99, -0.99]]), G)
    assert c.tolist() == [[3, 2, 2], [3, 2, 2], [2, 2, 2], [0, 3, 3], [0, 3, 0]]
    assert near.tolist() == [True, True, False, False, True]
    # the restated pools: a cell owns both of its faces, the dilation stops at the grid's faces
    occ = np.zeros((5, 5, 5), np.float32)
    occ[2, 0, 4] = 0.5                                                          # on the face between ix = 1 and ix = 2
    want = np.zeros((G, G, G), bool)
    want[1:3, 0, 3] = True
    assert np.array_equal(VG.cells(occ, G, 1, 0.5), want) and not VG.cells(occ, G, 1, 0.6).any()
    grown = VG.dilate(want, 1)
    assert grown.sum() == 4 * 2 * 2 and grown[0:4, 0:2, 2:4].all()
