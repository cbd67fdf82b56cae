"""GPU: cnr_image_scores (csrc/image_metric.hip) through cnr_amd.image_metrics against the numpy restatement
(tests/imgmetric_cpu.py) at the smallest shapes at which the kernel can go wrong -- one window, none, every tile edge with and
without room for the halo --, its bit-identity across batch sizes and runs, evaluate_views on a rasterised scene, and
tools/eval_views.py.

Bars (all derived, none measured):
  counts           equal.
  se, depth_abs    relative n_terms 2^-52: sums of n_terms non-negative doubles, whatever the order.
  ssim             |sum - ref| <= n_ssim 1e-9: a moment is a 121-term sum of values in [0,1] (error about 1.4e-14), the variance
                   terms carry a few of those over denominators of at least C1 = 1e-4 and C2 = 9e-4: a few 1e-10 per pixel.
  ssim_map         1e-9 + 2^-24 (its f32 rounding); exactly 0 on the border."""
import functools
import importlib.util
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT
import imgmetric_cpu as R

pytestmark = pytest.mark.gpu

from cnr_amd import image_metrics as M  # noqa: E402

U = 2.0 ** -52
IDS = [0, 2, 3, 5, 7]                    # gaps; 5 shows nowhere; the images also hold 9, which is not listed
TW, TH = M.TILE_W, M.TILE_H
SHAPES = [(11, 11), (10, 40), (12, 11), (43, 37)] + [(w, 13) for w in (TW - 1, TW, TW + 1, TW + 1 + 2 * M.HALO)] + [
    (12, h) for h in (TH - 1, TH, TH + 1, TH + 1 + 2 * M.HALO)]


@functools.lru_cache(maxsize=None)
def case(W, H, N=3):
    """seeded inputs (numpy) and their restatement, for the f32 and the uint8 ground truth; never modified"""
    rng = np.random.default_rng(1000 * W + H)
    a = rng.random((N, W, H, 3)).astype(np.float32)
    b = np.clip(a + 0.1 * rng.standard_normal((N, W, H, 3)), 0.0, 1.0).astype(np.float32)
    b8 = np.round(b * 255.0).astype(np.uint8)
    dr = (0.5 + 3.0 * rng.random((N, W, H))).astype(np.float32) * (rng.random((N, W, H)) > 0.3)
    dg = (0.5 + 3.0 * rng.random((N, W, H))).astype(np.float32) * (rng.random((N, W, H)) > 0.3)
    for x in (dr, dg):                                       # all four hit combinations, in every image
        x[:, 0, :2] = 0.0
    dr[:, 0, 1], dg[:, 0, 0], dr[:, 0, 2], dg[:, 0, 2], dr[:, 0, 3], dg[:, 0, 3] = 1.5, 2.5, 1.25, 1.75, 0.0, 0.0
    lg = rng.choice(np.array([0, 2, 3, 7, 9], np.int32), size=(N, W, H))
    lr = np.where(rng.random((N, W, H)) < 0.7, lg, rng.choice(np.array([-1, 0, 2, 3, 7, 9], np.int32), size=(N, W, H))).astype(np.int32)
    lr[:, -1, -1] = -1
    inp = dict(a=a, b=b, b8=b8, dr=dr.astype(np.float32), dg=dg.astype(np.float32), lr=lr, lg=lg.astype(np.int32))
    ref = {k: R.scores(a, inp[k], inp["dr"], inp["dg"], lr, lg, IDS) for k in ("b", "b8")}
    return inp, ref


def run(dev, inp, gt, sl=slice(None), ids=IDS, ssim_map=True):
    t = lambda k: torch.from_numpy(inp[k][sl]).to(dev)
    return M.score_images(t("a"), t(gt), t("dr"), t("dg"), t("lr"), t("lg"), ids=ids, ssim_map=ssim_map)


def fields(s):
    out = {k: getattr(s, k).cpu().numpy() for k in M.COUNT_FIELDS + ("se", "depth_abs")}
    out["ssim"] = s.ssim_sum.cpu().numpy()
    if s.ssim_map is not None:
        out["ssim_map"] = s.ssim_map.cpu().numpy()
    return out


def assert_matches(got, ref, sl=slice(None)):
    for k in M.COUNT_FIELDS:
        assert np.array_equal(got[k], ref[k][sl]), k
    n_pix, n_both, n_ssim = (ref[k][sl].astype(np.float64) for k in ("n_pix", "n_both", "n_ssim"))
    print("max |se - ref| / ref", np.nanmax(np.abs(got["se"] - ref["se"][sl]) / np.maximum(ref["se"][sl], 1e-300)),
          "max |ssim - ref| / n_ssim", np.max(np.abs(got["ssim"] - ref["ssim"][sl]) / np.maximum(n_ssim, 1)))
    assert (np.abs(got["se"] - ref["se"][sl]) <= 3 * n_pix * U * ref["se"][sl]).all()
    assert (np.abs(got["depth_abs"] - ref["depth_abs"][sl]) <= n_both * U * ref["depth_abs"][sl]).all()
    assert (np.abs(got["ssim"] - ref["ssim"][sl]) <= n_ssim * 1e-9).all()
    if "ssim_map" in got:
        m, r = got["ssim_map"], ref["ssim_map"][sl]
        assert np.abs(m - r).max() <= 1e-9 + 2.0 ** -24
        border = np.ones(m.shape[1:], bool)
        border[M.HALO:m.shape[1] - M.HALO, M.HALO:m.shape[2] - M.HALO] = False
        assert (m[:, border] == 0).all()


def bit_equal(x, y):
    return all(np.array_equal(x[k].view(np.int64) if x[k].dtype == np.float64 else x[k], y[k].view(np.int64) if y[k].dtype == np.float64 else y[k])
               for k in x)


@pytest.mark.parametrize("W,H", SHAPES)
def test_scores_match_restatement(dev, W, H):
    inp, ref = case(W, H)
    for gt in ("b", "b8"):
        three = fields(run(dev, inp, gt))
        assert_matches(three, ref[gt])
        # an image scored alone is its row of the N = 3 launch, bit for bit; and a second run is the first
        for n in (0, 2):
            one = fields(run(dev, inp, gt, slice(n, n + 1)))
            assert bit_equal(one, {k: v[n:n + 1] for k, v in three.items()}), (gt, n)
        assert bit_equal(fields(run(dev, inp, gt)), three)
    s = ref["b"]
    windows = max(W - 10, 0) * max(H - 10, 0)
    assert (s["n_ssim"][:, -1] == windows).all() and (s["n_pix"][:, 3] == 0).all() and (s["n_pix"][:, :3] > 0).all()
    assert (s["n_both"][:, -1] > 0).all() and (s["n_only_rec"][:, -1] > 0).all() and (s["n_only_gt"][:, -1] > 0).all()
    assert (s["n_pix"][:, :-1].sum(1) < W * H).all() and (s["inter"][:, -1] < W * H).all()        # the unlisted 9, the -1


def test_no_window_is_nan(dev):
    inp, _ = case(10, 40)
    s = run(dev, inp, "b")
    assert int(s.n_ssim.sum()) == 0 and np.isnan(s.ssim()).all() and not s.ssim_map.any()
    assert np.isnan(M.ssim(inp["a"][0], inp["b"][0]))
    assert np.isnan(s.summary()["ssim"]).all() and np.isfinite(s.summary()["psnr"][-1])


def test_flat_bright_pair(dev):
    """0.9 + 1e-3 u against itself + 1e-3 u': E[a^2] - mu_a^2 cancels against C2, and moments summed in fp32 miss S by 3e-4"""
    rng = np.random.default_rng(5)
    a = (0.9 + 1e-3 * rng.random((1, 43, 37, 3))).astype(np.float32)
    b = (a + 1e-3 * rng.random((1, 43, 37, 3))).astype(np.float32)
    ref = R.scores(a, b)
    s = M.score_images(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), ssim_map=True)
    assert_matches(fields(s), ref)
    assert abs(M.ssim(a[0], b[0]) - ref["ssim"][0, 0] / ref["n_ssim"][0, 0]) <= 1e-9
    assert abs(M.psnr(a[0], b[0]) - R.psnr(ref["se"], ref["n_pix"])[0, 0]) <= 1e-9


def test_identical_images(dev):
    inp, _ = case(43, 37)
    a = torch.from_numpy(inp["a"]).to(dev)
    s = M.score_images(a, a.clone(), ssim_map=True)
    assert (s.se == 0).all() and np.isinf(s.psnr()).all() and (s.psnr() > 0).all() and M.psnr(a, a) == np.inf
    assert np.abs(s.ssim() - 1.0).max() <= 1e-9 and tuple(s.n_pix.shape) == (3, 1) and s.ids == []
    # K = 0 and no depth, no labels: one row, the absent pairs count nothing
    for k in ("n_both", "n_only_rec", "n_only_gt", "n_rec", "inter"):
        assert int(getattr(s, k).sum()) == 0, k
    assert (s.n_pix == 43 * 37).all() and (s.depth_abs == 0).all() and np.isnan(s.iou()).all() and np.isnan(s.depth_l1()).all()


def test_default_ids_and_single_image(dev):
    inp, ref = case(43, 37)
    t = lambda k: torch.from_numpy(inp[k][0]).to(dev)
    s = M.score_images(t("a"), inp["b"][0], label_rec=inp["lr"][0], label_gt=t("lg"))        # numpy and tensors mixed
    assert s.ids == [0, 2, 3, 7, 9] and tuple(s.n_pix.shape) == (1, 6)
    full = R.scores(inp["a"][:1], inp["b"][:1], None, None, inp["lr"][:1], inp["lg"][:1], s.ids)
    assert_matches(fields(s), full)
    assert int(s.n_pix[0, :5].sum()) == 43 * 37


def test_255_one_pixel_instances(dev):
    W, H = TW + 1, TH + 1                                    # 561 pixels over four tiles
    rng = np.random.default_rng(9)
    a = rng.random((2, W, H, 3)).astype(np.float32)
    b = rng.random((2, W, H, 3)).astype(np.float32)
    lg = np.full((2, W * H), 1000, np.int32)
    where = rng.permutation(W * H)[:255]
    lg[0, where] = 3 * np.arange(255) + 1                    # one pixel each, scattered over the tiles
    lg[1, :255] = 3 * np.arange(255) + 1
    lg = lg.reshape(2, W, H)
    lr = np.roll(lg, 1, axis=2)
    lr[:, ::2] = lg[:, ::2]
    ids = (3 * np.arange(255) + 1).tolist()
    ref = R.scores(a, b, None, None, lr, lg, ids)
    s = M.score_images(a, b, label_rec=lr, label_gt=lg, ids=ids)
    assert tuple(s.n_pix.shape) == (2, 256) and (ref["n_pix"][:, :255] == 1).all()
    assert_matches(fields(s), ref)
    assert 0 < ref["inter"][:, :255].sum() < 2 * 255


def test_rgb_index_past_2_31(dev):
    """One 32768 x 21900 image: its rgb has more than 2^31 elements, and the only pixels that differ from zero lie past that
    index.  Everything else is 0 against 0, where se is 0 and S is (C1 C2) / (C1 C2) = 1 exactly, so the expected sums come
    from the restatement on the 50 x 50 corner that holds the patch (20 pixels from the corner's inner edges: no window that the
    corner's own border drops sees the patch).  depth and labels stay below 2^31 elements at any shape one call allows here."""
    W, H, C = 32768, 21900, 50
    assert (W - 30) * H * 3 > 2 ** 31
    rng = np.random.default_rng(31)
    pa = rng.random((20, 20, 3)).astype(np.float32)
    pb = rng.integers(0, 256, (20, 20, 3)).astype(np.uint8)
    a = torch.zeros(1, W, H, 3, device=dev)
    b = torch.zeros(1, W, H, 3, device=dev, dtype=torch.uint8)
    a[0, W - 30:W - 10, H - 30:H - 10] = torch.from_numpy(pa).to(dev)
    b[0, W - 30:W - 10, H - 30:H - 10] = torch.from_numpy(pb).to(dev)
    s = M.score_images(a, b)
    del a, b
    ca, cb = np.zeros((1, C, C, 3), np.float32), np.zeros((1, C, C, 3), np.uint8)
    ca[0, 20:40, 20:40], cb[0, 20:40, 20:40] = pa, pb
    ref = R.scores(ca, cb)
    n_ssim = (W - 10) * (H - 10)
    assert int(s.n_pix) == W * H and int(s.n_ssim) == n_ssim
    assert abs(float(s.se) - ref["se"][0, 0]) <= 3 * 400 * U * ref["se"][0, 0]
    expected = float(n_ssim - ref["n_ssim"][0, 0]) + ref["ssim"][0, 0]
    print("ssim sum", float(s.ssim_sum), "expected", expected)
    assert abs(float(s.ssim_sum) - expected) <= n_ssim * 1e-9


def test_argument_errors_of_the_abi(dev):
    import cnr_amd
    lib = cnr_amd._C.load()
    assert lib.cnr_image_scores_workspace_bytes(1, 0, 5, 0) == -1 and lib.cnr_image_scores_workspace_bytes(1, 5, 0, 0) == -1
    assert lib.cnr_image_scores_workspace_bytes(1, 5, 5, 256) == -1 and lib.cnr_image_scores_workspace_bytes(0, 5, 5, 0) == -1
    assert lib.cnr_image_scores_workspace_bytes(1, 5, 5, 255) > 0
    a = torch.zeros(1, 5, 5, 3, device=dev)
    lab = torch.zeros(1, 5, 5, device=dev, dtype=torch.int32)
    ids = torch.arange(256, device=dev, dtype=torch.int32)
    ws, cnt, sm = torch.empty(1 << 16, device=dev, dtype=torch.uint8), torch.zeros(7, 1, 257, device=dev, dtype=torch.int64), \
        torch.zeros(3, 1, 257, device=dev, dtype=torch.float64)
    for K, W, H, has_l in ((256, 5, 5, 1), (1, 0, 5, 1), (1, 5, 0, 1), (1, 5, 5, 0)):
        with pytest.raises(cnr_amd._C.CnrError, match="argument error"):
            cnr_amd._C.call("cnr_image_scores", a, a, 0, None, None, 0, lab if has_l else None, lab if has_l else None, has_l, ids, K,
                            1, W, H, ws, None, cnt, sm)
    with pytest.raises(cnr_amd._C.CnrError, match="argument error"):           # a flag without its pointers
        cnr_amd._C.call("cnr_image_scores", a, a, 0, None, None, 1, None, None, 0, None, 0, 1, 5, 5, ws, None, cnt, sm)


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _box(lo, hi, color):
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    v = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                  [1, 5, 7], [1, 7, 3]], np.int64)
    c = np.tile(np.asarray(color, np.float32), (8, 1)) * np.linspace(0.6, 1.0, 8, dtype=np.float32)[:, None]
    return v, f, c


def test_evaluate_views_on_a_rasterised_scene(dev):
    from cnr_amd import raster
    import raster_cpu as RC
    scene = raster.MeshScene([_box((0.1, 0.1, 0.1), (0.5, 0.6, 0.7), (0.9, 0.3, 0.2)), _box((0.55, 0.3, 0.2), (0.9, 0.9, 0.5), (0.2, 0.4, 0.9))],
                             labels=[4, 11], device=dev)
    rast = raster.MeshRasterizer.from_intrinsics(24, 20, 22.0, 22.0, 11.5, 9.5, 0.1, 10.0, device=dev)
    poses = RC.ring_poses(3, 2.2, 0.8)
    render = lambda T: rast.render(scene, T)
    rng = np.random.default_rng(2)
    frames, renders = [], []
    for T in poses:
        r = {k: v.cpu().numpy() for k, v in render(T).items()}
        renders.append(r)
        img = np.round(np.clip(r["rgb"] + 0.05 * rng.standard_normal(r["rgb"].shape), 0, 1) * 255).astype(np.uint8)
        depth = (r["depth"] * np.float32(1.03) * (rng.random(r["depth"].shape) > 0.1)).astype(np.float32)
        mask = np.where(rng.random(r["instance"].shape) > 0.1, r["instance"], 4).astype(np.int32)
        frames.append(dict(image=img, depth=depth, obj_mask=mask, T=T))
    assert {4, 11} <= set(np.unique(np.stack([r["instance"] for r in renders])))
    s = M.evaluate_views(render, frames, batch=2)           # a launch of two frames and one of one
    assert s.ids == [4, 11] and len(s) == 3
    stack = lambda k: np.stack([r[k] for r in renders])
    ref = R.scores(stack("rgb"), np.stack([f["image"] for f in frames]), stack("depth"), np.stack([f["depth"] for f in frames]),
                   stack("instance"), np.stack([f["obj_mask"] for f in frames]), [4, 11])
    assert_matches(fields(s), ref)
    t = s.summary()
    assert np.abs(t["psnr"] - R.psnr(ref["se"].sum(0), ref["n_pix"].sum(0))).max() <= 1e-9
    assert np.abs(t["iou"] - R.iou(ref["n_pix"].sum(0), ref["n_rec"].sum(0), ref["inter"].sum(0))).max() <= 1e-15
    assert np.abs(t["depth_l1"] - R.ratio(ref["depth_abs"].sum(0), ref["n_both"].sum(0))).max() <= 1e-12
    # a render against itself
    same = M.evaluate_views(render, list(poses), reference_fn=render, batch=4)
    iou, p = same.iou(), same.psnr()
    assert same.ids == [4, 11] and (iou[:, -1] == 1.0).all() and ((iou == 1.0) | (same.n_pix.cpu().numpy() == 0)).all()
    assert (np.isinf(p) | (same.n_pix.cpu().numpy() == 0)).all() and np.isinf(p[:, -1]).all() and (same.depth_l1()[:, -1] == 0).all()
    assert np.nanmax(np.abs(same.ssim() - 1.0)) <= 1e-9


# ---- the tool ----------------------------------------------------------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location("eval_views_tool", os.path.join(ROOT, "tools", "eval_views.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_eval_views_tool(dev, tmp_path, monkeypatch, capsys):
    import cnr_amd as cnr
    from cnr_amd.scene_cateogries import cameraInfo, sceneCategory
    from test_dataset_gpu import DS, _tree_with_cache
    root = _tree_with_cache(tmp_path, "replica")
    with open(os.path.join(DS, "replica.json")) as f:
        c = json.load(f)
    c["dataset"]["path"] = root
    c["camera"].update(w=72, h=48, fx=60.0, fy=60.0, cx=35.5, cy=23.5)
    c["model"]["net_hyperparams"]["latent_dim"] = 32
    cfg_file = tmp_path / "cfg.json"
    cfg_file.write_text(json.dumps(c))
    cfg = cnr.cfg.Config(str(cfg_file))
    data = cnr.dataset.get_dataset(cfg)
    rays = cameraInfo(cfg).rays_dir_cache
    np.random.seed(0)
    torch.manual_seed(0)
    logdir = tmp_path / "logs"
    logdir.mkdir()
    for cls_id in data.inst_dict.keys():
        sc = sceneCategory(cfg, cls_id, data.inst_dict[cls_id], data.sample_dict, rays)
        if cls_id == 0:
            b = sc.trainer.bound                                     # a plain object, so that the file unpickles anywhere
            sc.trainer.bound = SimpleNamespace(extent=np.asarray(b.extent), center=np.asarray(b.center), R=np.asarray(b.R))
        sc.save_checkpoints(str(logdir), 5)
    tool = _tool()
    assert tool.frame_slice("0:4:2", 5) == [0, 2] and tool.frame_slice("::2", 5) == [0, 2, 4] and tool.frame_slice("-1", 5) == [4]
    n_frames = len(data.sample_dict)
    base = ["eval_views.py", "--config", str(cfg_file), "--logdir", str(logdir), "--frames", "0:2", "--samples", "16", "--allow-pickle"]
    out = tmp_path / "scores.json"
    monkeypatch.setattr(sys, "argv", base + ["--out", str(out)])
    tool.main()
    with open(out) as f:
        rec = json.load(f)
    n = min(2, n_frames)
    K = len(rec["ids"])
    assert {"ids", "frames", "n_pix", "psnr", "psnr_frame_mean", "ssim", "depth_l1", "iou", "per_frame", "against", "samples", "frame_ids"} <= set(rec)
    assert rec["against"] == "dataset frames" and K >= 1 and rec["ids"] == sorted(rec["ids"])
    assert all(len(rec[k]) == K + 1 for k in ("psnr", "ssim", "depth_l1", "iou", "n_pix", "psnr_frame_mean"))
    assert np.asarray(rec["per_frame"]["psnr"]).shape == (n, K + 1)
    assert rec["n_pix"][-1] == n * 72 * 48 and np.isfinite(rec["psnr"][-1]) and -1.0 <= rec["ssim"][-1] <= 1.0
    assert 0.0 <= rec["iou"][-1] <= 1.0
    text = capsys.readouterr().out
    assert "instance" in text and "image" in text and "psnr" in text
    # every cell set (tau 0): the skipped render is the full render bit for bit
    out2 = tmp_path / "skip.json"
    monkeypatch.setattr(sys, "argv", base + ["--skip-empty", "--grid", "8", "--tau", "0", "--against-unskipped", "--out", str(out2)])
    tool.main()
    with open(out2) as f:
        rec = json.load(f)
    assert rec["against"] == "unskipped render" and rec["psnr"][-1] == float("inf")
    assert all(p == float("inf") for row, pix in zip(rec["per_frame"]["psnr"], rec["per_frame"]["n_pix"]) for p, m in zip(row, pix) if m)
    assert abs(rec["ssim"][-1] - 1.0) <= 1e-9 and rec["iou"][-1] == 1.0
