"""Image-space view evaluation: how good a rendered view is against the sequence's frame, or against
another render of the same pose -- PSNR, SSIM, depth L1 and mask IoU, per frame and per instance, on the GPU.

``score_images`` runs ``cnr_image_scores`` (csrc/image_metric.hip) on a stack of image pairs in this project's (W,H,...)
layout and returns the SUMS per (image, row) as an ``ImageScores``: row ``k < K`` is the set of pixels whose ground-truth label
is ``ids[k]``, row ``K`` every pixel.  The ratios (``psnr``, ``ssim``, ``depth_l1``, ``iou``, ``summary``) are formed here in
float64.  ``evaluate_views`` renders and scores the frames of a dataset (or a second render function) in batches.

SSIM is Wang et al.'s with the parameters of skimage's ``structural_similarity(gaussian_weights=True, sigma=1.5,
use_sample_covariance=False, data_range=1, channel_axis=-1)``: an 11 x 11 Gaussian window, only windows wholly inside the
image, moments in float64.  skimage itself was never run beside it: tests/imgmetric_cpu.py restates the definition."""
import re

import numpy as np
import torch

from . import _C

__all__ = ["score_images", "ImageScores", "psnr", "ssim", "evaluate_views", "TILE_W", "TILE_H", "HALO", "MAX_IDS"]

COUNT_FIELDS = ("n_pix", "n_ssim", "n_both", "n_only_rec", "n_only_gt", "n_rec", "inter")
SUM_FIELDS = ("se", "ssim", "depth_abs")
HALO = 5
MAX_IDS = 255


def _tile_constants():
    """CNR_IMG_TILE_W / _H of include/cnr_hip.h: the kernel's tile, for the tests that walk its edges"""
    with open(_C.HEADER_PATH) as f:
        text = f.read()
    got = [re.search(r"#\s*define\s+CNR_IMG_TILE_%s\s+(\d+)\s*$" % a, text, flags=re.M) for a in "WH"]
    if None in got:
        raise _C.CnrError("cnr_hip.h: no #define CNR_IMG_TILE_W / CNR_IMG_TILE_H")
    return int(got[0].group(1)), int(got[1].group(1))


TILE_W, TILE_H = _tile_constants()


def _nan_div(num, den):
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.nan)


def _psnr_of(se, n_pix):
    """-10 log10(se / (3 n_pix)): inf at se == 0, nan at n_pix == 0 (and a NaN se stays NaN)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return -10.0 * np.log10(_nan_div(se, 3.0 * np.asarray(n_pix, np.float64)))


class ImageScores:
    """The sums of ``score_images``: ``n_pix, n_ssim, n_both, n_only_rec, n_only_gt, n_rec, inter`` (int64) and ``se, ssim_sum,
    depth_abs`` (float64), each an (N, K+1) tensor (on the device the scores were formed on, or the CPU), ``ids`` the K
    instance ids as a list, ``ssim_map`` (N,W,H) f32 or None.  Row K is the whole image.  ``has_labels=False``: the images
    came without labels (their counts are 0) and every IoU is nan."""

    def __init__(self, ids, counts, sums, ssim_map=None, has_labels=True):
        self.ids = [int(i) for i in ids]
        self.has_labels = bool(has_labels)
        for name, v in zip(COUNT_FIELDS, counts):
            setattr(self, name, v)
        self.se, self.ssim_sum, self.depth_abs = sums
        self.ssim_map = ssim_map
        shape = tuple(self.n_pix.shape)
        if len(shape) != 2 or shape[1] != len(self.ids) + 1:
            raise ValueError("tables of shape {} for {} ids".format(shape, len(self.ids)))
        for name in COUNT_FIELDS + ("se", "ssim_sum", "depth_abs"):
            if tuple(getattr(self, name).shape) != shape:
                raise ValueError("{} has the shape {}, not {}".format(name, tuple(getattr(self, name).shape), shape))

    def __len__(self):
        return int(self.n_pix.shape[0])

    def _np(self, name):
        return getattr(self, name).detach().cpu().numpy()

    # ---- per frame, (N, K+1) float64 numpy ---------------------------------------------------------------------------
    def psnr(self):
        return _psnr_of(self._np("se"), self._np("n_pix"))

    def ssim(self):
        return _nan_div(self._np("ssim_sum"), self._np("n_ssim"))

    def depth_l1(self):
        return _nan_div(self._np("depth_abs"), self._np("n_both"))

    def iou(self):
        n_pix, n_rec, inter = self._np("n_pix"), self._np("n_rec"), self._np("inter")
        return _nan_div(inter, (n_pix + n_rec - inter) * self.has_labels)

    # ---- pooled over the frames --------------------------------------------------------------------------------------
    def summary(self):
        """Per row (K+1 entries, the last the whole image), pooled over all frames: ``psnr`` from sum se / sum 3 n_pix,
        ``ssim`` = sum ssim / sum n_ssim, ``depth_l1`` = sum depth_abs / sum n_both, ``iou`` = sum inter / sum union;
        ``psnr_frame_mean`` the mean of the per-frame PSNR over the frames with n_pix > 0 and a finite PSNR (nan without
        one); ``frames`` the number of frames with n_pix > 0.  -> dict of ``ids`` and float64 / int64 numpy arrays."""
        n_pix, n_rec, inter = self._np("n_pix"), self._np("n_rec"), self._np("inter")
        per = self.psnr()
        ok = (n_pix > 0) & np.isfinite(per)
        cnt = ok.sum(0)
        mean = _nan_div(np.where(ok, per, 0.0).sum(0), cnt)
        return dict(ids=list(self.ids), frames=(n_pix > 0).sum(0).astype(np.int64), n_pix=n_pix.sum(0),
                    psnr=_psnr_of(self._np("se").sum(0), n_pix.sum(0)), psnr_frame_mean=mean,
                    ssim=_nan_div(self._np("ssim_sum").sum(0), self._np("n_ssim").sum(0)),
                    depth_l1=_nan_div(self._np("depth_abs").sum(0), self._np("n_both").sum(0)),
                    iou=_nan_div(inter.sum(0), (n_pix + n_rec - inter).sum(0) * self.has_labels))

    def extend(self, other):
        """appends the frames of ``other`` (equal ``ids``); returns self"""
        if list(other.ids) != list(self.ids):
            raise ValueError("cannot join scores of the ids {} and {}".format(self.ids, other.ids))
        if other.has_labels != self.has_labels:
            raise ValueError("cannot join scores with and without labels")
        for name in COUNT_FIELDS + ("se", "ssim_sum", "depth_abs"):
            a, b = getattr(self, name), getattr(other, name)
            setattr(self, name, torch.cat([a, b.to(a.device)], 0))
        if self.ssim_map is not None and other.ssim_map is not None and self.ssim_map.shape[1:] == other.ssim_map.shape[1:]:
            self.ssim_map = torch.cat([self.ssim_map, other.ssim_map.to(self.ssim_map.device)], 0)
        else:
            self.ssim_map = None
        return self

    def to_json(self):
        """the summary and the per-frame tables as plain lists (nan / inf as JSON's NaN / Infinity)"""
        s = self.summary()
        out = {k: (v if k == "ids" else np.asarray(v).tolist()) for k, v in s.items()}
        out["per_frame"] = dict(psnr=self.psnr().tolist(), ssim=self.ssim().tolist(), depth_l1=self.depth_l1().tolist(),
                                iou=self.iou().tolist(), n_pix=self._np("n_pix").tolist())
        return out


# ---- arguments -----------------------------------------------------------------------------------------------------------
def _as_tensor(x):
    return x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))


def _stack(x, tail, dtypes, what):
    """a single image (W,H,*tail) or a stack (N,W,H,*tail) of one of `dtypes` -> the stack, dtype untouched"""
    t = _as_tensor(x)
    if t.dim() == 2 + len(tail):
        t = t[None]
    if t.dim() != 3 + len(tail) or tuple(t.shape[3:]) != tuple(tail) or min(t.shape[:3]) < 1:
        raise ValueError("{} must have the shape (W,H{}) or (N,W,H{}), not {}".format(
            what, "".join(",%d" % d for d in tail), "".join(",%d" % d for d in tail), tuple(t.shape)))
    if t.dtype not in dtypes:
        raise ValueError("{} must be {}, not {}".format(what, " or ".join(str(d) for d in dtypes), t.dtype))
    return t


def _check_ids(ids):
    """-> a list of ints: strictly ascending int32 values, at most MAX_IDS of them"""
    ids = [int(i) for i in (ids.tolist() if hasattr(ids, "tolist") else ids)]
    if len(ids) > MAX_IDS:
        raise ValueError("{} ids, more than {} in one call".format(len(ids), MAX_IDS))
    if any(b <= a for a, b in zip(ids, ids[1:])):
        raise ValueError("ids must be strictly ascending")
    if ids and (ids[0] < -2 ** 31 or ids[-1] >= 2 ** 31):
        raise ValueError("ids must fit int32")
    return ids


def _prepare(rgb_rec, rgb_gt, depth_rec, depth_gt, label_rec, label_gt, ids):
    """Every check of score_images that needs no device -> (tensors in the order of the arguments, ids or None)"""
    if (depth_rec is None) != (depth_gt is None):
        raise ValueError("depth_rec and depth_gt come together or not at all")
    if (label_rec is None) != (label_gt is None):
        raise ValueError("label_rec and label_gt come together or not at all")
    a = _stack(rgb_rec, (3,), (torch.float32,), "rgb_rec")
    b = _stack(rgb_gt, (3,), (torch.float32, torch.uint8), "rgb_gt")
    if a.shape != b.shape:
        raise ValueError("rgb_rec {} and rgb_gt {} differ in shape".format(tuple(a.shape), tuple(b.shape)))
    out = [a, b]
    for rec, gt, dt, name in ((depth_rec, depth_gt, torch.float32, "depth"), (label_rec, label_gt, torch.int32, "label")):
        for x, side in ((rec, "_rec"), (gt, "_gt")):
            if x is None:
                out.append(None)
                continue
            t = _stack(x, (), (dt,), name + side)
            if t.shape != a.shape[:3]:
                raise ValueError("{}{} {} does not match the images {}".format(name, side, tuple(t.shape), tuple(a.shape[:3])))
            out.append(t)
    if ids is not None:
        ids = _check_ids(ids)
        if ids and label_gt is None:
            raise ValueError("ids without labels")
    return out, ids


def score_images(rgb_rec, rgb_gt, depth_rec=None, depth_gt=None, label_rec=None, label_gt=None, ids=None, ssim_map=False):
    """A reconstruction against a ground truth: ``rgb_rec`` f32 and ``rgb_gt`` f32 or uint8 (a byte v counts as v / 255),
    (W,H,3) or (N,W,H,3); ``depth_*`` f32 (0 = nothing there) and ``label_*`` int32 of the images' shape, each pair given
    together or not at all -- ``label_gt`` the dataset's ``obj_mask``, ``label_rec`` the renderers' ``instance`` (-1 = nothing).
    Device tensors or numpy arrays (those are uploaded to the current device).  ``ids``: the instance ids to score, strictly
    ascending, at most 255; ``None`` takes the sorted unique ``label_gt >= 0``.  ``ssim_map=True`` also returns the (N,W,H)
    map of S.  -> ``ImageScores`` with (N, K+1) tables on the device.  ValueError for every malformed argument, before the
    library is touched."""
    tens, ids = _prepare(rgb_rec, rgb_gt, depth_rec, depth_gt, label_rec, label_gt, ids)
    dev = next((t.device for t in tens if t is not None and t.is_cuda), None)
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    a, b, dr, dg, lr, lg = [None if t is None else t.to(dev).contiguous() for t in tens]
    if ids is None:
        ids = [] if lg is None else _check_ids(torch.unique(lg[lg >= 0]).cpu())
    N, W, H, K = a.shape[0], a.shape[1], a.shape[2], len(ids)
    with torch.cuda.device(dev):
        ids_t = torch.tensor(ids, dtype=torch.int32, device=dev) if K else None
        counts = torch.empty(len(COUNT_FIELDS), N, K + 1, device=dev, dtype=torch.int64)
        sums = torch.empty(len(SUM_FIELDS), N, K + 1, device=dev, dtype=torch.float64)
        smap = torch.empty(N, W, H, device=dev, dtype=torch.float32) if ssim_map else None
        ws = _C.workspace(_C.load().cnr_image_scores_workspace_bytes(N, W, H, K), dev, "cnr_image_scores")
        _C.call("cnr_image_scores", a, b, 1 if b.dtype == torch.uint8 else 0, dr, dg, 0 if dr is None else 1, lr, lg,
                0 if lr is None else 1, ids_t, K, N, W, H, ws, smap, counts, sums)
    return ImageScores(ids, list(counts.unbind(0)), list(sums.unbind(0)), smap, has_labels=lr is not None)


def psnr(a, b):
    """PSNR of two images (or stacks) with values in [0,1] (``b`` may be uint8), over all their pixels -> float"""
    s = score_images(a, b)
    return float(_psnr_of(s._np("se").sum(), s._np("n_pix").sum()))


def ssim(a, b):
    """mean SSIM of two images (or stacks) over the pixels whose window lies inside the image -> float (nan below 11 x 11)"""
    s = score_images(a, b)
    return float(_nan_div(s._np("ssim_sum").sum(), s._np("n_ssim").sum()))


# ---- rendering and scoring -------------------------------------------------------------------------------------------------
def _single(x, dtype):
    """an image of a frame as a tensor of `dtype`; a uint8 colour image stays uint8"""
    t = _as_tensor(x)
    return t if t.dtype == dtype or (dtype == torch.float32 and t.dtype == torch.uint8 and t.dim() == 3) else t.to(dtype)


def evaluate_views(render_fn, frames, ids=None, batch=4, reference_fn=None, ssim_map=False):
    """Renders and scores.  ``frames``: an iterable of ``sample_dict`` entries (``image`` (W,H,3) u8 or f32, ``depth``,
    ``obj_mask``, ``T``); ``render_fn(T_wc)`` -> a dict with ``rgb`` (W,H,3), ``depth`` (W,H), ``instance`` (W,H), as
    ``SceneRenderer.render`` returns and ``lambda T: rasterizer.render(scene, T)``.  With ``reference_fn`` the ground truth
    of a frame is ``reference_fn(T_wc)`` instead of its images, and an entry needs its ``T`` only (a bare (4,4) pose will do):
    a skipped render against the unskipped one at the same pose.  ``batch`` frames go into one launch.  ``ids=None`` takes the
    sorted unique ground-truth labels >= 0 of ALL frames, so that every batch has the same rows (with ``reference_fn`` that
    keeps every render alive until the last: name the ids for a long sequence).  -> one ``ImageScores``."""
    if isinstance(batch, bool) or int(batch) != batch or batch < 1:
        raise ValueError("batch must be a positive integer")
    frames = list(frames)
    if not frames:
        raise ValueError("no frames")
    if ids is None and reference_fn is None:
        seen = np.unique(np.concatenate([np.unique(_as_tensor(fr["obj_mask"]).cpu().numpy()) for fr in frames]))
        ids = seen[seen >= 0].tolist()
    if ids is not None:
        ids = _check_ids(ids)

    def pair(fr):
        T = fr["T"] if isinstance(fr, dict) else fr
        rec = render_fn(T)
        gt = reference_fn(T) if reference_fn is not None else dict(rgb=fr["image"], depth=fr["depth"], instance=fr["obj_mask"])
        dev = rec["rgb"].device
        return ([rec["rgb"].float(), rec["depth"].float(), rec["instance"].to(torch.int32)],
                [_single(gt["rgb"], torch.float32).to(dev), _single(gt["depth"], torch.float32).to(dev),
                 _single(gt["instance"], torch.int32).to(dev)])

    def score(part):
        rec = [torch.stack([p[0][k] for p in part]) for k in range(3)]
        gt = [torch.stack([p[1][k] for p in part]) for k in range(3)]
        return score_images(rec[0], gt[0], rec[1], gt[1], rec[2], gt[2], ids=ids, ssim_map=ssim_map)

    if ids is None:                 # two renders and no ids: the rows are known only when every reference is rendered
        pairs = [pair(fr) for fr in frames]
        seen = torch.unique(torch.cat([torch.unique(g[2]) for _, g in pairs]))
        ids = _check_ids(seen[seen >= 0].cpu().tolist())
        parts = (pairs[a:a + int(batch)] for a in range(0, len(pairs), int(batch)))
    else:
        parts = ([pair(fr) for fr in frames[a:a + int(batch)]] for a in range(0, len(frames), int(batch)))
    out = None
    for part in parts:
        s = score(part)
        out = s if out is None else out.extend(s)
    return out


def format_table(scores, names=None):
    """the per-instance table and the whole-image row of ``scores.summary()`` as text"""
    s = scores.summary()
    rows = ["{:>10} {:>7} {:>10} {:>9} {:>9} {:>8} {:>8}".format("instance", "frames", "pixels", "psnr", "ssim", "depth_l1", "iou")]
    for k in range(len(s["ids"]) + 1):
        label = "image" if k == len(s["ids"]) else str((names or {}).get(s["ids"][k], s["ids"][k]))
        rows.append("{:>10} {:>7d} {:>10d} {:>9.3f} {:>9.5f} {:>8.4f} {:>8.4f}".format(
            label, int(s["frames"][k]), int(s["n_pix"][k]), s["psnr"][k], s["ssim"][k], s["depth_l1"][k], s["iou"][k]))
    return "\n".join(rows)
