"""Times the image scores (cnr_amd.image_metrics) on the GPU at 1200 x 680 with K = 8 instances, for N = 1
and N = 8 image pairs with a uint8 ground truth, depth and labels: cnr_image_scores through the C-ABI on pre-allocated buffers
(device events over back-to-back calls after a warm-up), score_images as a user calls it, and beside them the same scores
formed with torch ops on the device -- a grouped fp64 conv2d for the five moments of the three channels, masked sums per id --,
the only yardstick there is.  Prints the agreement of the two and the bytes/s against the 31 bytes per pixel the kernel must
read (12 rgb f32 + 3 rgb u8 + 8 depths + 8 labels).

    python tools/time_imgmetrics.py [--reps 200] [--torch-reps 10] [--out profiles/imgmetrics_time.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

W, H, K = 1200, 680, 8
BYTES_PER_PIXEL = 12 + 3 + 8 + 8


def make_inputs(N, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(N, W, H, 3, generator=g)
    b8 = ((a + 0.05 * torch.randn(N, W, H, 3, generator=g)).clamp(0, 1) * 255).round().to(torch.uint8)
    dr = (0.5 + 3 * torch.rand(N, W, H, generator=g)) * (torch.rand(N, W, H, generator=g) > 0.1)
    dg = (dr * 1.02) * (torch.rand(N, W, H, generator=g) > 0.1)
    # K = 8 instances as blocks of a 4 x 3 board (ids 10, 20, ..), the other four blocks an unlisted id; the reconstruction's
    # labels are the board shifted by a few pixels, with holes
    board = torch.tensor([[10, 20, 999], [30, 999, 40], [50, 60, 999], [999, 70, 80]], dtype=torch.int32)
    lg = board.repeat_interleave(W // 4, 0).repeat_interleave(H // 3 + 1, 1)[:W, :H].expand(N, W, H).contiguous()
    lr = torch.roll(lg, (3, 2), (1, 2)).clone()
    lr[torch.rand(N, W, H, generator=g) < 0.05] = -1
    ids = [10, 20, 30, 40, 50, 60, 70, 80]
    return [t.to(dev).contiguous() for t in (a, b8, dr.float(), dg.float(), lr, lg)], ids


def torch_scores(a, b8, dr, dg, lr, lg, ids, weight):
    """the definitions with torch ops in float64 on the device -> (counts (7,N,K+1) i64, sums (3,N,K+1) f64)"""
    N = a.shape[0]
    x, y = a.double().permute(0, 3, 1, 2), b8.double().permute(0, 3, 1, 2) / 255.0
    se = ((x - y) ** 2).sum(1)
    m = torch.nn.functional.conv2d(torch.cat([x, y, x * x, y * y, x * y], 1), weight, groups=15)
    mu_a, mu_b, e_aa, e_bb, e_ab = m[:, 0:3], m[:, 3:6], m[:, 6:9], m[:, 9:12], m[:, 12:15]
    S = ((2 * mu_a * mu_b + 1e-4) * (2 * (e_ab - mu_a * mu_b) + 9e-4)) / (
        (mu_a ** 2 + mu_b ** 2 + 1e-4) * (e_aa - mu_a ** 2 + e_bb - mu_b ** 2 + 9e-4))
    smap = torch.zeros(N, W, H, dtype=torch.float64, device=a.device)
    smap[:, 5:W - 5, 5:H - 5] = S.mean(1)
    inside = torch.zeros(W, H, dtype=torch.bool, device=a.device)
    inside[5:W - 5, 5:H - 5] = True
    hr, hg = dr > 0, dg > 0
    both = hr & hg
    dabs = (dr.double() - dg.double()).abs() * both
    counts = torch.zeros(7, N, len(ids) + 1, dtype=torch.int64, device=a.device)
    sums = torch.zeros(3, N, len(ids) + 1, dtype=torch.float64, device=a.device)
    for k in range(len(ids) + 1):
        if k < len(ids):
            row, rec = lg == ids[k], lr == ids[k]
            counts[5, :, k], counts[6, :, k] = rec.sum((1, 2)), (rec & row).sum((1, 2))
        else:
            row = torch.ones_like(lg, dtype=torch.bool)
            counts[5, :, k], counts[6, :, k] = W * H, (lr == lg).sum((1, 2))
        counts[0, :, k], counts[1, :, k] = row.sum((1, 2)), (row & inside).sum((1, 2))
        counts[2, :, k], counts[3, :, k], counts[4, :, k] = (row & both).sum((1, 2)), (row & hr & ~hg).sum((1, 2)), (row & ~hr & hg).sum((1, 2))
        sums[0, :, k], sums[1, :, k], sums[2, :, k] = (se * row).sum((1, 2)), (smap * (row & inside)).sum((1, 2)), (dabs * row).sum((1, 2))
    return counts, sums


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--torch-reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from cnr_amd import _C, image_metrics as M
    assert torch.cuda.is_available(), "time_imgmetrics needs the GPU"
    dev = torch.device("cuda:0")
    g = torch.arange(-5, 6, dtype=torch.float64)
    g = torch.exp(-(g * g) / 4.5)
    g = g / g.sum()
    weight = (g[:, None] * g[None, :]).expand(15, 1, 11, 11).contiguous().to(dev)
    rows = []
    for N in (1, 8):
        inp, ids = make_inputs(N, dev)
        ids_t = torch.tensor(ids, dtype=torch.int32, device=dev)
        counts = torch.empty(7, N, K + 1, device=dev, dtype=torch.int64)
        sums = torch.empty(3, N, K + 1, device=dev, dtype=torch.float64)
        ws = _C.workspace(_C.load().cnr_image_scores_workspace_bytes(N, W, H, K), dev, "cnr_image_scores")

        def kernel():
            _C.call("cnr_image_scores", inp[0], inp[1], 1, inp[2], inp[3], 1, inp[4], inp[5], 1, ids_t, K, N, W, H, ws, None, counts, sums)
        ms_kernel = timed(kernel, a.reps)
        ms_api = timed(lambda: M.score_images(*inp, ids=ids), max(a.reps // 4, 1))
        ms_torch = timed(lambda: torch_scores(*inp, ids, weight), a.torch_reps, warmup=2)
        tc, ts = torch_scores(*inp, ids, weight)
        kernel()
        torch.cuda.synchronize()
        n_ssim = counts[1].double().clamp(min=1)
        pooled = M.ImageScores(ids, list(counts.unbind(0)), list(sums.unbind(0))).summary()
        rec = dict(N=N, W=W, H=H, K=K, gt="uint8", ms_kernel=round(ms_kernel, 4), ms_score_images=round(ms_api, 4),
                   ms_torch_formulation=round(ms_torch, 3), torch_over_kernel=round(ms_torch / ms_kernel, 1),
                   bytes_read=N * W * H * BYTES_PER_PIXEL, gbytes_per_s=round(N * W * H * BYTES_PER_PIXEL / ms_kernel / 1e6, 1),
                   workspace_bytes=int(ws.numel()), counts_equal=bool((tc == counts).all()),
                   se_max_rel_diff=float(((ts[0] - sums[0]).abs() / ts[0]).max()),
                   ssim_max_abs_diff_per_pixel=float(((ts[1] - sums[1]).abs() / n_ssim).max()),
                   depth_abs_max_rel_diff=float(((ts[2] - sums[2]).abs() / ts[2]).max()),
                   psnr_image=pooled["psnr"][-1], ssim_image=pooled["ssim"][-1])
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, torch_reps=a.torch_reps,
                           note="ms per call, device events over back-to-back calls after a warm-up; bytes_read counts "
                                "each input byte once (31 per pixel)", rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
