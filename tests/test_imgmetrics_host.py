"""No GPU: the numpy restatement of the image scores (tests/imgmetric_cpu.py) against closed forms and scipy's Gaussian filter,
the host half of cnr_amd.image_metrics (ImageScores, the argument checks of score_images), and the new prototypes."""
import numpy as np
import pytest
import torch

import cnr_amd
from cnr_amd import image_metrics as M

import imgmetric_cpu as R


def _pair(W, H, seed, noise=0.1):
    rng = np.random.default_rng(seed)
    a = rng.random((W, H, 3))
    return a, np.clip(a + noise * rng.standard_normal((W, H, 3)), 0.0, 1.0)


def test_weights_sum_to_one():
    g = R.weights()
    assert g.shape == (11,) and abs(g.sum() - 1.0) <= 2.0 ** -52
    assert abs(np.outer(g, g).sum() - 1.0) <= 2.0 ** -51
    assert np.array_equal(g, g[::-1])


def test_direct_windows_equal_gaussian_filter():
    """skimage's algorithm: gaussian_filter(sigma=1.5, truncate=3.5) of x, y, xx, yy, xy per channel, crop by 5"""
    from scipy.ndimage import gaussian_filter
    a, b = _pair(23, 17, 1)
    f = lambda x: np.stack([gaussian_filter(x[..., c], sigma=1.5, truncate=3.5) for c in range(3)], -1)
    ux, uy = f(a), f(b)
    vx, vy, vxy = f(a * a) - ux * ux, f(b * b) - uy * uy, f(a * b) - ux * uy
    S = ((2 * ux * uy + R.C1) * (2 * vxy + R.C2)) / ((ux ** 2 + uy ** 2 + R.C1) * (vx + vy + R.C2))
    S = S[5:-5, 5:-5]
    got = R.ssim_windows(a, b)
    assert got.shape == S.shape == (13, 7, 3)
    assert np.abs(got - S).max() <= 1e-12


def test_closed_forms():
    a, b = _pair(15, 14, 2)
    S = R.ssim_windows(a, a)
    assert np.abs(S - 1.0).max() <= 1e-12
    s = R.scores(a[None], a[None])
    assert s["se"][0, 0] == 0.0 and R.psnr(s["se"], s["n_pix"])[0, 0] == np.inf
    c1, c2 = 0.3, 0.8
    S = R.ssim_windows(np.full((12, 13, 3), c1), np.full((12, 13, 3), c2))
    assert np.abs(S - (2 * c1 * c2 + R.C1) / (c1 * c1 + c2 * c2 + R.C1)).max() <= 1e-12
    # S(a,b) = S(b,a): the formula is symmetric, its rounding is not (E[a^2] - mu_a^2 + E[b^2] - mu_b^2 adds left to right: a
    # few 2^-53 on terms below 1, over a factor of at least C2 = 9e-4, is below 1e-12)
    assert np.abs(R.ssim_windows(a, b) - R.ssim_windows(b, a)).max() <= 1e-12
    d = 0.0625
    s = R.scores(a[None] * 0.5, (a * 0.5 + d)[None])
    assert abs(R.psnr(s["se"], s["n_pix"])[0, 0] - (-20 * np.log10(d))) <= 1e-9
    # uint8 enters as v / 255
    u = (np.arange(15 * 14 * 3) % 256).astype(np.uint8).reshape(15, 14, 3)
    assert np.array_equal(R.as_double(u), u.astype(np.float64) / 255.0)
    # below 11 x 11 there is no window
    s = R.scores(*[x[None, :10] for x in (a, b)])
    assert s["n_ssim"][0, 0] == 0 and np.isnan(R.ratio(s["ssim"], s["n_ssim"])[0, 0]) and not s["ssim_map"].any()


LABEL_GT = np.array([[1, 1, 1, 0, 0],
                     [1, 1, 1, 0, 0],
                     [4, 4, 9, 9, 0],
                     [4, 4, 9, 9, 0],
                     [7, 7, 7, 7, 7],
                     [7, 7, 7, 7, 7]], np.int32)                       # 6 x 5; 9 is not in ids
LABEL_REC = np.array([[1, 1, -1, 0, 0],
                      [1, 1, 4, 0, 0],
                      [4, 4, 4, 9, 0],
                      [1, 4, 9, 9, -1],
                      [7, 7, 7, 7, -1],
                      [-1, 7, 7, 7, 7]], np.int32)
IDS = [0, 1, 4, 5, 7]                                                   # 5 shows nowhere


def test_label_rows_by_hand():
    z = np.zeros((1, 6, 5, 3))
    s = R.scores(z, z, None, None, LABEL_REC[None], LABEL_GT[None], IDS)
    assert s["n_pix"][0].tolist() == [6, 6, 4, 0, 10, 30]
    assert s["n_rec"][0].tolist() == [5, 5, 5, 0, 8, 30]
    assert s["inter"][0].tolist() == [5, 4, 3, 0, 8, 23]
    iou = R.iou(s["n_pix"], s["n_rec"], s["inter"])[0]
    assert np.allclose(iou[[0, 1, 2, 4, 5]], [5 / 6, 4 / 7, 3 / 6, 8 / 10, 23 / 37], rtol=0, atol=1e-15) and np.isnan(iou[3])
    assert s["n_ssim"].sum() == 0


def test_depth_counts_match_depth_l1_images():
    rng = np.random.default_rng(3)
    dr = (rng.random((2, 9, 7)) * 3).astype(np.float32) * (rng.random((2, 9, 7)) > 0.3)
    dg = (rng.random((2, 9, 7)) * 3).astype(np.float32) * (rng.random((2, 9, 7)) > 0.3)
    z = np.zeros((2, 9, 7, 3))
    s = R.scores(z, z, dr, dg)
    for n in range(2):
        total, both, only_rec, only_gt, neither = cnr_amd.metrics.depth_l1_images(torch.from_numpy(dr[n]), torch.from_numpy(dg[n]))
        assert (s["n_both"][n, 0], s["n_only_rec"][n, 0], s["n_only_gt"][n, 0]) == (both, only_rec, only_gt)
        assert both and only_rec and only_gt and neither
        assert abs(s["depth_abs"][n, 0] - float(total)) <= both * 2.0 ** -52 * float(total)


def _scores(ids, **fields):
    n = np.asarray(fields["n_pix"]).shape
    get = lambda k, dt: torch.as_tensor(np.asarray(fields.get(k, np.zeros(n)), dt))
    return M.ImageScores(ids, [get(k, np.int64) for k in M.COUNT_FIELDS], [get(k, np.float64) for k in M.SUM_FIELDS])


def test_summary_pools_and_conventions():
    # rows: id 3, id 8, image; frames: 3.  id 8 is absent from frame 1; frame 2 of id 3 is perfect (se 0)
    s = _scores([3, 8], n_pix=[[10, 5, 100], [20, 0, 100], [10, 5, 100]],
                se=[[0.3, 0.15, 3.0], [0.06, 0.0, 0.3], [0.0, 1.5, 30.0]],
                n_ssim=[[4, 0, 50], [6, 0, 50], [0, 0, 50]], ssim=[[2.0, 0.0, 40.0], [3.0, 0.0, 45.0], [0.0, 0.0, 10.0]],
                n_both=[[5, 0, 10], [5, 0, 30], [0, 0, 0]], depth_abs=[[0.5, 0.0, 1.0], [1.5, 0.0, 3.0], [0.0, 0.0, 0.0]],
                n_rec=[[10, 5, 100], [10, 0, 100], [10, 0, 100]], inter=[[5, 5, 60], [10, 0, 70], [10, 0, 80]])
    p = s.psnr()
    assert p.shape == (3, 3) and p[2, 0] == np.inf and np.isnan(p[1, 1])
    assert abs(p[0, 0] - (-10 * np.log10(0.3 / 30))) < 1e-12
    assert np.isnan(s.ssim()[0, 1]) and s.ssim()[0, 0] == 0.5 and np.isnan(s.ssim()[2, 0])
    assert np.isnan(s.depth_l1()[2, 2]) and s.depth_l1()[1, 0] == 0.3
    assert s.iou()[0, 0] == 5 / 15 and np.isnan(s.iou()[1, 1]) and s.iou()[2, 1] == 0.0
    t = s.summary()
    assert t["ids"] == [3, 8] and t["frames"].tolist() == [3, 2, 3]
    assert abs(t["psnr"][0] - (-10 * np.log10(0.36 / 120))) < 1e-12
    assert abs(t["psnr"][2] - (-10 * np.log10(33.3 / 900))) < 1e-12
    assert abs(t["psnr_frame_mean"][0] - 0.5 * (p[0, 0] + p[1, 0])) < 1e-12          # the inf frame is left out
    assert abs(t["psnr_frame_mean"][1] - 0.5 * (p[0, 1] + p[2, 1])) < 1e-12          # and the absent one
    assert t["ssim"][0] == 0.5 and np.isnan(t["ssim"][1]) and abs(t["ssim"][2] - 95 / 150) < 1e-15
    assert t["depth_l1"][0] == 0.2 and np.isnan(t["depth_l1"][1]) and t["depth_l1"][2] == 0.1
    assert abs(t["iou"][0] - 25 / 45) < 1e-15 and t["iou"][1] == 0.5 and abs(t["iou"][2] - 210 / 390) < 1e-15
    # extend
    u = _scores([3, 8], n_pix=[[1, 1, 2]], se=[[0.0, 0.0, 0.0]])
    assert len(s.extend(u)) == 4 and s.n_pix[3].tolist() == [1, 1, 2] and s.summary()["frames"].tolist() == [4, 3, 4]
    with pytest.raises(ValueError):
        s.extend(_scores([3], n_pix=[[1, 2]]))
    with pytest.raises(ValueError):
        _scores([3], n_pix=[[1, 2, 3]])
    # an empty selection: all nan, nothing raised
    e = _scores([], n_pix=[[0]]).summary()
    assert np.isnan(e["psnr"][0]) and np.isnan(e["psnr_frame_mean"][0]) and e["frames"].tolist() == [0]


def test_score_images_rejects_before_the_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(cnr_amd._C, "load", boom)
    monkeypatch.setattr(cnr_amd._C, "call", boom)
    f = lambda *s: np.zeros(s, np.float32)
    i = lambda *s: np.zeros(s, np.int32)
    bad = [
        dict(rgb_rec=f(4, 5, 3), rgb_gt=f(4, 6, 3)),                                        # shapes
        dict(rgb_rec=f(2, 4, 5, 3), rgb_gt=f(4, 5, 3)),
        dict(rgb_rec=f(4, 5), rgb_gt=f(4, 5)),
        dict(rgb_rec=f(4, 5, 4), rgb_gt=f(4, 5, 4)),
        dict(rgb_rec=f(4, 5, 3).astype(np.float64), rgb_gt=f(4, 5, 3)),                     # dtypes
        dict(rgb_rec=f(4, 5, 3), rgb_gt=i(4, 5, 3)),
        dict(rgb_rec=f(4, 5, 3), rgb_gt=f(4, 5, 3), depth_rec=f(4, 5)),                     # half a pair
        dict(rgb_rec=f(4, 5, 3), rgb_gt=f(4, 5, 3), depth_gt=f(4, 5)),
        dict(rgb_rec=f(4, 5, 3), rgb_gt=f(4, 5, 3), label_rec=i(4, 5)),
        dict(rgb_rec=f(4, 5, 3), rgb_gt=f(4, 5, 3), label_gt=i(4, 5)),
        dict(rgb_rec=f(4, 5, 3), rgb_gt=f(4, 5, 3), depth_rec=f(4, 5), depth_gt=f(5, 4)),   # a pair of another shape
        dict(rgb_rec=f(4, 5, 3), rgb_gt=f(4, 5, 3), label_rec=i(4, 5), label_gt=i(2, 4, 5)),
        dict(rgb_rec=f(4, 5, 3), rgb_gt=f(4, 5, 3), label_rec=f(4, 5), label_gt=f(4, 5)),
        dict(rgb_rec=f(4, 5, 3), rgb_gt=f(4, 5, 3), label_rec=i(4, 5), label_gt=i(4, 5), ids=list(range(256))),
        dict(rgb_rec=f(4, 5, 3), rgb_gt=f(4, 5, 3), label_rec=i(4, 5), label_gt=i(4, 5), ids=[1, 3, 2]),
        dict(rgb_rec=f(4, 5, 3), rgb_gt=f(4, 5, 3), label_rec=i(4, 5), label_gt=i(4, 5), ids=[1, 1]),
        dict(rgb_rec=f(4, 5, 3), rgb_gt=f(4, 5, 3), ids=[1]),                               # ids without labels
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            M.score_images(**kw)
    with pytest.raises(ValueError):
        M.evaluate_views(lambda T: None, [])
    with pytest.raises(ValueError):
        M.evaluate_views(lambda T: None, [np.eye(4)], batch=0)


def test_header_declares_the_entry_points():
    sig = cnr_amd._C.SIGNATURES
    assert len(sig["cnr_image_scores"]) == 19 and len(sig["cnr_image_scores_workspace_bytes"]) == 4
    assert "cnr_image_scores_workspace_bytes" in cnr_amd._C._RESTYPE64
    assert (M.TILE_W, M.TILE_H, M.HALO) == (16, 32, 5)
    assert hasattr(cnr_amd, "image_metrics")
