"""GPU: ScanNet mask refinement (csrc/geoseg.hip, cnr_amd.utils.geometry_segmentation / refine_inst_data / connected_components /
fill_holes, get_dataset(cfg, refine=True)) against the restatement tests/geoseg_cpu.py, everything
array_equal; the normals by tests/test_fpfh_gpu.py's criteria.  tests/test_geoseg_host.py checks the restatement itself."""
import os
import pickle
import shutil

import numpy as np
import pytest
import torch

import fpfh_cpu as FC
import geoseg_cpu as G
from conftest import GOLDEN
from test_dataset_host import DS, _config, _frames, inst_dict_rows
from test_fpfh_host import EIGH_VS_JACOBI_ANGLE

pytestmark = pytest.mark.gpu
INTR = G.INTRINSICS


class Intrinsic:
    fx, fy, cx, cy = INTR["fx"], INTR["fy"], INTR["cx"], INTR["cy"]


@pytest.fixture(scope="module")
def cnr():
    import cnr_amd
    return cnr_amd


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _scene(name):
    build, smallest = G.SCENES[name]
    return build(), smallest


# ---- connected components -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
def test_connected_components_equal_the_restatement_gpu(dev, cnr, connectivity):
    masks = G.ccl_masks()
    for name, m in masks.items():
        got = cnr.utils.connected_components(_up(m, dev), connectivity)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), G.ccl(m, connectivity)), name
    board = cnr.utils.connected_components(_up(masks["checkerboard"], dev), connectivity).cpu().numpy()
    on = masks["checkerboard"].ravel() != 0
    if connectivity == 8:
        assert (board.ravel()[on] == 0).all()                                 # one component, named by pixel 0
    else:
        assert np.array_equal(board.ravel()[on], np.flatnonzero(on))          # none merged
    batch = np.stack([masks["spiral"], masks["random_half"], masks["u_shapes"]])
    got = cnr.utils.connected_components(_up(batch, dev), connectivity)
    assert np.array_equal(got.cpu().numpy(), G.ccl(batch, connectivity))
    assert torch.equal(got, cnr.utils.connected_components(_up(batch, dev), connectivity))
    counts = cnr.utils.label_counts(got).cpu().numpy()
    assert np.array_equal(counts, np.stack([G.label_counts(l) for l in G.ccl(batch, connectivity)]))
    with pytest.raises(cnr._C.CnrError):
        cnr.utils.connected_components(_up(masks["ones"], dev), 5)


def test_fill_holes_equal_the_restatement_gpu(dev, cnr):
    f = G.fill_masks()
    for name, m in f.items():
        got = cnr.utils.fill_holes(_up(m, dev))
        assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), G.fill_holes(m)), name
    stack = np.stack(list(f.values()))
    assert np.array_equal(cnr.utils.fill_holes(_up(stack, dev)).cpu().numpy(), np.stack([G.fill_holes(m) for m in stack]))
    for name in ("serpentine", "frame_ring", "random_dense"):
        m = G.ccl_masks()[name]
        assert np.array_equal(cnr.utils.fill_holes(_up(m, dev)).cpu().numpy(), G.fill_holes(m)), name
    # the labels form the loaders use: masks = (labels == seg_ids[k])
    labels = G.ccl(f["nested"], 4)
    ids = np.unique(labels[labels >= 0]).astype(np.int32)
    filled, err = cnr.utils._fill_holes_stack(_up(labels, dev), _up(ids, dev), None, len(ids), *labels.shape, dev)
    assert int(err.item()) == 0
    assert np.array_equal(filled.cpu().numpy() != 0, np.stack([G.fill_holes(labels == i) for i in ids]))


# ---- the image stages -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["boxes", "room"])
def test_maps_edge_and_growth_equal_the_restatement_gpu(dev, cnr, name):
    s, smallest = _scene(name)
    want = G.segmentation(s["P"], s["N"], s["depth"], smallest, smallest)
    P, N, depth = _up(s["P"], dev), _up(s["N"], dev), _up(s["depth"], dev)
    disc, conv = cnr.utils.geoseg_maps(P, N, depth)
    assert np.array_equal(disc.cpu().numpy(), want["disc"]) and np.array_equal(conv.cpu().numpy(), want["conv"])
    edge = cnr.utils.geoseg_edge_map(disc, conv, depth)
    assert np.array_equal(edge.cpu().numpy(), want["edge"])
    labels = cnr.utils.connected_components(edge, 8)
    assert np.array_equal(labels.cpu().numpy(), want["labels"])
    grown = cnr.utils.geoseg_grow(P, depth, edge, labels, cnr.utils.label_counts(labels), smallest)
    assert np.array_equal(grown.cpu().numpy(), want["grown"])
    # without the area filter, and with labels filtered beforehand: the same gather
    assert np.array_equal(cnr.utils.geoseg_grow(P, depth, edge, labels).cpu().numpy(), G.grow(s["P"], s["depth"], want["edge"], want["labels"]))
    assert np.array_equal(cnr.utils.geoseg_grow(P, depth, edge, _up(want["kept"], dev)).cpu().numpy(), want["grown"])
    assert (want["grown"] != want["kept"]).any()


def test_growth_takes_the_first_of_equal_distances_gpu(dev, cnr):
    P, depth, edge, labels = G.tie_plane()
    col = int(np.flatnonzero(edge[0] == 0)[0])
    assert np.array_equal(np.abs(P[:, col - 1, 0]), np.abs(P[:, col + 1, 0]))          # the two sides are exactly as far
    want = G.grow(P, depth, edge, labels)
    assert (want[:, col] == labels[0, col - 1]).all()                                  # the left label wins
    got = cnr.utils.geoseg_grow(_up(P, dev), _up(depth, dev), _up(edge, dev), _up(labels, dev))
    assert np.array_equal(got.cpu().numpy(), want)


# ---- the vote ---------------------------------------------------------------------------------------------------------------
def test_vote_equals_the_reference_gpu(dev, cnr):
    z = np.load(os.path.join(GOLDEN, "geoseg", "refine_cases.npz"))
    for name, (inst, masks) in G.refine_cases().items():
        got = cnr.utils.refine_inst_data(inst, list(masks), device=dev)
        want = z[name + "__refined"]
        assert isinstance(got, np.ndarray) and got.dtype == want.dtype and np.array_equal(got, want), name
    inst, masks = G.refine_cases()["overlap_later_wins"]
    assert not cnr.utils.refine_inst_data(inst, [], device=dev).any()
    assert not cnr.utils.refine_inst_data(inst, list(masks), threshold=1.0, device=dev).any()


# ---- end to end -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["boxes", "room"])
def test_geometry_segmentation_end_to_end_gpu(dev, cnr, name):
    s, smallest = _scene(name)
    normal, output, masks, segments = cnr.utils.geometry_segmentation(s["rgb"], s["depth"], Intrinsic, smallest, smallest, device=dev)
    assert normal.dtype == np.float32 and normal.shape == s["P"].shape and output.dtype == np.uint8
    valid = s["depth"] > 0
    # the normals: tests/test_fpfh_gpu.py's criteria against the restatement's, on the rows whose eigenvector is well conditioned
    pts = s["P"][valid]
    want_n, count, lam = s["normals64"], s["count"], s["eigenvalues"]
    got_n = cnr.utils.estimate_normals_device(_up(pts, dev), G.NORMAL_RADIUS, G.NORMAL_MAX_NN).cpu().numpy()
    got_n = np.where(got_n[:, 2:] > 0, -got_n, got_n)
    assert np.array_equal(normal[valid], got_n.astype(np.float32)) and not normal[~valid].any()       # the image is these, in fp32
    full = count >= 3
    ok = full & (FC.eigen_gap(lam) >= 1e-3)
    assert (full & ~ok).sum() <= 0.05 * len(pts)
    assert np.array_equal(got_n[~full], want_n[~full])
    ang = FC.angles(got_n[ok], want_n[ok])
    print(name, "largest angle to the restatement", ang.max(), "bit-equal rows", int((got_n == want_n).all(1).sum()), "of", len(pts))
    assert ang.max() <= 10 * EIGH_VS_JACOBI_ANGLE
    steep = ok & (np.abs(want_n[:, 2]) > 1e-6)
    assert ((got_n[steep] * want_n[steep]).sum(1) > 0).all() and (normal[..., 2] <= 0).all()
    # everything after the normals, from the GPU's own normal image
    want = G.segmentation(s["P"], normal, s["depth"], smallest, smallest)
    assert len(masks) == len(want["masks"]) == len(segments) and len(masks) >= (3 if name == "boxes" else 1)
    for k, (m, w) in enumerate(zip(masks, want["masks"])):
        assert m.dtype == bool and np.array_equal(m, w), k
        assert np.array_equal(segments[k].points, s["P"][w]) and np.array_equal(segments[k].normals, normal[w])
        assert np.array_equal(segments[k].rgbs, s["rgb"][w])
    assert np.array_equal(output, want["output"])
    refined = cnr.utils.refine_inst_data(s["inst"], masks, device=dev)
    assert refined.dtype == s["inst"].dtype and np.array_equal(refined, G.refine_inst_data(s["inst"], want["masks"]))
    if name == "boxes":
        assert set(np.unique(refined)) == {0, G.ID_A, G.ID_B}
    # the loaders' path, without leaving the device, with the same normals handed in
    again = cnr.utils.geometry_segmentation(s["rgb"], s["depth"], Intrinsic, smallest, smallest, device=dev, normal_image=normal)
    assert np.array_equal(again[1], output)
    frame = cnr.utils.refine_frame(_up(s["depth"], dev), _up(s["inst"], dev), Intrinsic, smallest, smallest)
    assert np.array_equal(frame.cpu().numpy(), refined)


def test_depth_beyond_the_unprojection_range_is_refused_gpu(dev, cnr):
    depth = np.full((8, 9), 9.0, np.float32)
    with pytest.raises(ValueError, match="beyond 8 m"):
        cnr.utils.geometry_segmentation(np.zeros((8, 9, 3), np.uint8), depth, Intrinsic, device=dev)
    empty = cnr.utils.geometry_segmentation(np.zeros((8, 9, 3), np.uint8), np.zeros((8, 9), np.float32), Intrinsic, device=dev)
    assert empty[2] == [] and not empty[0].any() and not empty[1].any()


# ---- the loader ---------------------------------------------------------------------------------------------------------------
def _load(cnr, cfg, **kw):
    seen, load = {}, cnr.dataset._load_inst_dict

    def spy(ds, c):
        seen["inst_dict"] = ds.inst_dict
        load(ds, c)

    cnr.dataset._load_inst_dict = spy
    try:
        return cnr.dataset.get_dataset(cfg, **kw), seen["inst_dict"]
    finally:
        cnr.dataset._load_inst_dict = load


def test_get_dataset_refines_a_missing_mask_gpu(cnr, tmp_path):
    from dataset_synth import write_registration_pickle
    root = str(tmp_path / "scannet")
    shutil.copytree(os.path.join(DS, "scannet"), root)
    write_registration_pickle(root, _frames("scannet_refined"))
    missing = os.path.join(root, "instance-refined", "3.npy")
    before = np.load(os.path.join(root, "instance-refined", "4.npy"))
    os.remove(missing)
    os.remove(os.path.join(root, "inst_to_cls", "3.pkl"))
    cfg = _config(cnr, "scannet_refined", root=root)
    with pytest.raises(NotImplementedError, match="geometry_segmentation"):
        cnr.dataset.get_dataset(cfg)
    ds, inst_dict = _load(cnr, cfg, refine=True)
    written = np.load(missing)
    assert written.dtype == np.int32 and written.shape == before.shape
    assert np.array_equal(np.load(os.path.join(root, "instance-refined", "4.npy")), before)       # the other frames' files stay
    with open(os.path.join(root, "inst_to_cls", "3.pkl"), "rb") as f:
        inst_to_cls = pickle.load(f)
    with open(os.path.join(DS, "scannet", "inst_to_cls", "3.pkl"), "rb") as f:
        recorded = pickle.load(f)
    assert inst_to_cls == recorded and [type(k) for k in inst_to_cls] == [type(k) for k in recorded]
    assert [type(v) for v in inst_to_cls.values()] == [type(v) for v in recorded.values()]
    assert set(np.unique(written)) <= set(int(k) for k in inst_to_cls)
    # the frame handed on is the written mask, and a plain reload of the tree gives the same dataset
    ds2, inst_dict2 = _load(cnr, cfg)
    assert list(ds.sample_dict) == list(ds2.sample_dict) and ds.n_img == ds2.n_img
    for f in ds.sample_dict:
        for key in ("image", "depth", "obj_mask", "T"):
            assert np.array_equal(ds.sample_dict[f][key], ds2.sample_dict[f][key]), (f, key)
        assert ds.sample_dict[f]["frame_id"] == ds2.sample_dict[f]["frame_id"]
    assert inst_dict_rows(inst_dict) == inst_dict_rows(inst_dict2)
    # the written mask is the public functions' result on the frame the loader hands on and the raw map of src/dataset.py:327-356
    from PIL import Image
    e = cfg.mw
    raw = np.asarray(Image.open(os.path.join(root, "instance-filt", "3.png"))).astype(np.int32)[e:-e, e:-e] + 1
    sem = np.asarray(Image.open(os.path.join(root, "label-filt", "3.png")))[e:-e, e:-e]
    for i in np.unique(raw):
        if sem[raw == i][0] in ds.background_cls_list:
            raw[raw == i] = 0
    sample = ds.sample_dict[2]                                  # frame 3: frame 2 has no finite pose and is skipped
    assert np.array_equal(sample["T"], ds.poses[3])
    depth = np.ascontiguousarray(sample["depth"].T)
    assert depth.shape == raw.shape == written.shape
    _, _, masks, _ = cnr.utils.geometry_segmentation(np.ascontiguousarray(sample["image"].transpose(1, 0, 2)), depth,
                                                     ds.intrinsic_open3d)
    print("frame 3:", len(masks), "segments, refined ids", np.unique(written).tolist())
    assert np.array_equal(cnr.utils.refine_inst_data(raw, masks), written)
