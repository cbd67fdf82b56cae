"""numpy float64 restatement of cnr_amd.image_metrics: the sums per (image, row) that cnr_image_scores
returns and the values derived from them, written as the definitions read -- SSIM by direct 121-term windows, no separable
pass, no tiles."""
import numpy as np

C1, C2 = 1e-4, 9e-4
R = 5


def weights():
    """the 11 one-dimensional Gaussian weights, sigma 1.5, normalised"""
    i = np.arange(-R, R + 1, dtype=np.float64)
    g = np.exp(-(i * i) / (2.0 * 1.5 * 1.5))
    return g / g.sum()


def as_double(img):
    """a uint8 value v enters as v / 255.0, an f32 value as its exact double"""
    img = np.asarray(img)
    return img.astype(np.float64) / 255.0 if img.dtype == np.uint8 else img.astype(np.float64)


def ssim_windows(a, b):
    """a, b (W,H,3) float64 -> S (W-10, H-10, 3) of every window wholly inside the image (empty below 11 x 11)"""
    W, H = a.shape[:2]
    if W < 2 * R + 1 or H < 2 * R + 1:
        return np.zeros((max(W - 2 * R, 0), max(H - 2 * R, 0), 3))
    g = weights()
    w2 = (g[:, None] * g[None, :])[None, None, None]                   # (1,1,1,11,11)
    win = lambda x: np.lib.stride_tricks.sliding_window_view(x, (2 * R + 1, 2 * R + 1), axis=(0, 1))   # (W-10,H-10,3,11,11)
    A, B = win(a), win(b)
    mean = lambda x: (x * w2).sum(axis=(-2, -1))
    mu_a, mu_b, e_aa, e_bb, e_ab = mean(A), mean(B), mean(A * A), mean(B * B), mean(A * B)
    return ((2 * mu_a * mu_b + C1) * (2 * (e_ab - mu_a * mu_b) + C2)) / (
        (mu_a ** 2 + mu_b ** 2 + C1) * (e_aa - mu_a ** 2 + e_bb - mu_b ** 2 + C2))


def ssim_map(a, b):
    """(W,H) channel mean of S, 0 where the window is not inside the image"""
    out = np.zeros(a.shape[:2])
    S = ssim_windows(a, b)
    if S.size:
        out[R:a.shape[0] - R, R:a.shape[1] - R] = S.mean(-1)
    return out


def scores(rgb_rec, rgb_gt, depth_rec=None, depth_gt=None, label_rec=None, label_gt=None, ids=()):
    """stacks (N,W,H,...) -> dict of (N, K+1) arrays: n_pix, n_ssim, n_both, n_only_rec, n_only_gt, n_rec, inter (int64), se,
    ssim, depth_abs (float64), and ssim_map (N,W,H) float64"""
    ids = list(ids)
    N, W, H = rgb_rec.shape[:3]
    K = len(ids)
    ints = {k: np.zeros((N, K + 1), np.int64) for k in ("n_pix", "n_ssim", "n_both", "n_only_rec", "n_only_gt", "n_rec", "inter")}
    flt = {k: np.zeros((N, K + 1), np.float64) for k in ("se", "ssim", "depth_abs")}
    maps = np.zeros((N, W, H))
    inside = np.zeros((W, H), bool)
    if W > 2 * R and H > 2 * R:
        inside[R:W - R, R:H - R] = True
    for n in range(N):
        a, b = as_double(rgb_rec[n]), as_double(rgb_gt[n])
        se = ((a - b) ** 2).sum(-1)
        maps[n] = ssim_map(a, b)
        if depth_rec is not None:
            dr, dg = np.asarray(depth_rec[n]), np.asarray(depth_gt[n])
            hr, hg = dr > 0, dg > 0
            dabs = np.abs(dr.astype(np.float64) - dg.astype(np.float64))
        for k in range(K + 1):
            if k < K:
                m = label_gt[n] == ids[k]
                ints["n_rec"][n, k] = (label_rec[n] == ids[k]).sum()
                ints["inter"][n, k] = ((label_rec[n] == ids[k]) & m).sum()
            else:
                m = np.ones((W, H), bool)
                if label_gt is not None:
                    ints["n_rec"][n, k] = W * H
                    ints["inter"][n, k] = (label_rec[n] == label_gt[n]).sum()
            ints["n_pix"][n, k] = m.sum()
            flt["se"][n, k] = se[m].sum()
            ints["n_ssim"][n, k] = (m & inside).sum()
            flt["ssim"][n, k] = maps[n][m & inside].sum()
            if depth_rec is not None:
                ints["n_both"][n, k] = (m & hr & hg).sum()
                ints["n_only_rec"][n, k] = (m & hr & ~hg).sum()
                ints["n_only_gt"][n, k] = (m & ~hr & hg).sum()
                flt["depth_abs"][n, k] = dabs[m & hr & hg].sum()
    return dict(ssim_map=maps, **ints, **flt)


def psnr(se, n_pix):
    """-10 log10(se / (3 n_pix)); inf at se == 0, nan at n_pix == 0"""
    se, n_pix = np.asarray(se, np.float64), np.asarray(n_pix, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return -10.0 * np.log10(se / (3.0 * n_pix))


def ratio(num, den):
    """num / den, nan at den == 0"""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / den, np.nan)


def iou(n_pix, n_rec, inter):
    return ratio(inter, np.asarray(n_pix) + np.asarray(n_rec) - np.asarray(inter))
