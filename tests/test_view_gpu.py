"""GPU: the scene view kernels (cnr_view_segments_*, cnr_view_points, cnr_view_composite) against tests/view_cpu.py, and
SceneRenderer end to end against the same restatement with oracle field values.

The comparison rule is modular_cases.check: max|kernel - fp64| <= 5 e_r + 2^-22 max|fp64|, e_r the error of the same
restatement run in float32.  Integer outputs are exact."""
import os

import numpy as np
import pytest
import torch

import view_cpu as V
import view_scene as VS
from conftest import rel_l2
from modular_cases import check

pytestmark = pytest.mark.gpu
KMAX = V.KMAX


@pytest.fixture(scope="module")
def cnr():
    import cnr_amd
    return cnr_amd


def _t(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _m7(dev, *shape, dtype=torch.int32):
    return torch.full(shape, -7, device=dev, dtype=dtype)


def gpu_segments(cnr, dev, T, dirs, to_box, n_alloc):
    """count + emit into buffers pre-filled with NaN / -7, `n_alloc` segment rows -> dict of numpy arrays"""
    _C = cnr._C
    P, E = dirs.shape[0], to_box.shape[0]
    Tg, dg, bg = _t(T, dev, torch.float32), _t(dirs, dev), _t(to_box, dev, torch.float32)
    ws = torch.empty(int(_C.load().cnr_view_segments_workspace_bytes(P, E)), device=dev, dtype=torch.uint8)
    ent_off, cnt, ovf = _m7(dev, E + 1, dtype=torch.int64), _m7(dev, 1, dtype=torch.int64), _m7(dev, 1, dtype=torch.int64)
    _C.call("cnr_view_segments_count", Tg, dg, bg, P, E, VS.ZMIN, VS.ZMAX, ws, ent_off, cnt, ovf)
    N = int(cnt.item())
    assert N <= n_alloc, (N, n_alloc)
    seg_pixel, seg_entity, seg_z = _m7(dev, n_alloc), _m7(dev, n_alloc), _nan(dev, n_alloc, 2)
    pix_segs = _m7(dev, P, KMAX)
    _C.call("cnr_view_segments_emit", Tg, dg, bg, P, E, VS.ZMIN, VS.ZMAX, ws, seg_pixel, seg_entity, seg_z, pix_segs)
    torch.cuda.synchronize()
    return dict(N=N, overflow=int(ovf.item()), entity_offset=ent_off.cpu().numpy(), seg_pixel=seg_pixel.cpu().numpy(),
                seg_entity=seg_entity.cpu().numpy(), seg_z=seg_z.cpu().numpy(), pix_segs=pix_segs.cpu().numpy(),
                dev=dict(T=Tg, dirs=dg, seg_pixel=seg_pixel, seg_entity=seg_entity, seg_z=seg_z))


def _compare_segments(got, T, dirs, to_box):
    """hit sets exact up to grazing pairs (none in the scenes here), then every array whole; -> the fp64 restatement"""
    T32, A32 = T.astype(np.float32), to_box.astype(np.float32)
    s64 = V.segments(T32, dirs, A32, VS.ZMIN, VS.ZMAX, np.float64)
    E, P = s64["hit"].shape
    N = got["N"]
    hit = np.zeros((E, P), bool)
    assert (got["seg_entity"][:N] >= 0).all() and (got["seg_pixel"][:N] >= 0).all()
    hit[got["seg_entity"][:N], got["seg_pixel"][:N]] = True
    _, zn, zf = V.slab(T32, dirs, A32, np.float64(VS.ZMIN), np.float64(VS.ZMAX), np.float64)
    grazing = np.abs(zf - zn) < 1e-4 * np.maximum(1.0, zf)
    print("hit pairs", int(s64["hit"].sum()), "kernel", int(hit.sum()), "grazing pairs left out", int(grazing.sum()))
    assert grazing.sum() <= 0.01 * E * P
    assert np.array_equal(hit | grazing, s64["hit"] | grazing)
    s64 = V.segments(T32, dirs, A32, VS.ZMIN, VS.ZMAX, np.float64, hit=hit)
    s32 = V.segments(T32, dirs, A32, VS.ZMIN, VS.ZMAX, np.float32, hit=hit)
    assert N == s64["N"]
    for k in ("seg_pixel", "seg_entity"):
        want = np.full_like(got[k], -7)
        want[:N] = s64[k]
        assert np.array_equal(got[k], want), k
    assert np.array_equal(got["entity_offset"], s64["entity_offset"])
    assert np.array_equal(got["pix_segs"], s64["pix_segs"])
    assert got["overflow"] == s64["overflow"]
    assert np.isnan(got["seg_z"][N:]).all()
    check(torch.from_numpy(got["seg_z"][:N]), torch.from_numpy(s64["seg_z"]), torch.from_numpy(s32["seg_z"]), "seg_z")
    return s64, s32


SCENES = {"A": lambda: VS.scene_a(), "A_without_bg": lambda: VS.scene_a(False), "B_axis_parallel": VS.scene_b}


@pytest.mark.parametrize("name", list(SCENES))
def test_segments_and_points(cnr, dev, name):
    T, dirs, to_box = SCENES[name]()
    n_alloc = int(V.segments(T.astype(np.float32), dirs, to_box.astype(np.float32), VS.ZMIN, VS.ZMAX, np.float64)["N"]) + 5
    got = gpu_segments(cnr, dev, T, dirs, to_box, n_alloc)
    s64, s32 = _compare_segments(got, T, dirs, to_box)
    if name == "A_without_bg":
        assert int((got["pix_segs"][:, 0] < 0).sum()) == 305
    N = got["N"]
    rng = np.random.default_rng(2)
    to_field = np.stack([V.box_affine(rng.normal(size=3), V.rot(rng.normal(size=3), rng.uniform(0, 3)), rng.uniform(0.5, 2.0) * np.ones(3))
                         for _ in range(to_box.shape[0])]).astype(np.float32)
    d = got["dev"]
    for S in (1, 5, 64, 128):
        z, pts = _nan(dev, n_alloc, S), _nan(dev, n_alloc, S, 3)
        cnr._C.call("cnr_view_points", d["T"], d["dirs"], _t(to_field, dev), d["seg_pixel"], d["seg_entity"], d["seg_z"], N, S, z, pts)
        torch.cuda.synchronize()
        assert torch.isnan(z[N:]).all() and torch.isnan(pts[N:]).all()
        # the kernel's own seg_z in, so that this step is compared on identical inputs
        args = (T.astype(np.float32), dirs, to_field, s64["seg_pixel"], s64["seg_entity"], got["seg_z"][:N], S)
        z64, p64 = V.points(*args, np.float64)
        z32, p32 = V.points(*args, np.float32)
        check(z[:N].cpu(), torch.from_numpy(z64), torch.from_numpy(z32), f"z S={S}")
        check(pts[:N].cpu(), torch.from_numpy(p64), torch.from_numpy(p32), f"pts S={S}")


def test_segments_scan_with_more_counts_than_scanning_threads(cnr, dev):
    """The scenes above have 432 pixels: 7 waves x at most 5 entities = 35 counts, one per thread of the one-workgroup scan.
    Scene A's pose and boxes at 160 x 120 give 300 waves x 5 entities = 1500 counts, so two per scanning thread: the scan's
    run loops, before and after its block scan.  Every integer output exact against the fp64 restatement."""
    T, _, to_box = VS.scene_a()
    dirs = V.pinhole_dirs(160, 120, 20 * 160 / 24, 79.5, 59.5)
    assert dirs.shape[0] == 19200 and (dirs.shape[0] + 63) // 64 * to_box.shape[0] == 1500
    N = 27388                                                       # of the restatement; _compare_segments asserts it
    got = gpu_segments(cnr, dev, T, dirs, to_box, N + 5)
    s64, _ = _compare_segments(got, T, dirs, to_box)
    assert got["N"] == s64["N"] == N and got["overflow"] == 0
    assert (got["pix_segs"][:, 0] >= 0).all()                       # no empty pixel


def test_overflow_keeps_the_nearest_eight(cnr, dev):
    T, dirs, to_box = VS.scene_nested(9)
    s64 = V.segments(T.astype(np.float32), dirs, to_box.astype(np.float32), VS.ZMIN, VS.ZMAX, np.float64)
    assert s64["overflow"] > 0
    got = gpu_segments(cnr, dev, T, dirs, to_box, s64["N"])
    assert got["overflow"] == s64["overflow"] == int((s64["hit"].sum(0) > KMAX).sum())
    _compare_segments(got, T, dirs, to_box)
    over = np.nonzero(s64["hit"].sum(0) > KMAX)[0]
    for p in over:                                                  # the kept eight are the nearest by z_near
        mine = np.nonzero(s64["seg_pixel"] == p)[0]
        kept = got["pix_segs"][p]
        dropped = np.setdiff1d(mine, kept)
        assert len(dropped) == len(mine) - KMAX and (kept >= 0).all()
        assert s64["seg_z"][dropped, 0].min() >= s64["seg_z"][kept, 0].max()


def test_render_raises_on_overflow(cnr, dev):
    cfg = VS.small_camera(cnr.cfg.synthetic_config(device=str(dev), latent_dim=32))
    cls_dict, scene_bg = VS.make_scene(cnr, cfg, seed=1, n_obj=9, spread=0.05)
    r = cnr.view.SceneRenderer(cls_dict, scene_bg, cfg)
    with pytest.raises(ValueError, match="more than 8"):
        r.render(VS.camera_pose(), n_samples=4)


# ---- the composite on synthetic arrays --------------------------------------------------------------------------------
def composite_case(K, S, regime="ordinary", P=70, seed=0):
    """P pixels with 0 .. K segments each (mixed, some with none), sigma / colour / z handed in.  One segment of every pixel is
    made the dominant one so that the two largest masses differ by at least 0.05 (asserted by the caller on the float64 result)."""
    g = torch.Generator().manual_seed(1000 * K + S + seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float32).numpy()
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32).numpy()
    n_seg = np.array([(p * 7 + 3) % (K + 1) for p in range(P)])
    n_seg[:2] = (K, 0)
    N = int(n_seg.sum())
    pix_segs = np.full((P, KMAX), -1, np.int32)
    seg_entity = np.zeros(N, np.int32)
    zn, zf = np.zeros(N, np.float32), np.zeros(N, np.float32)
    # the others together absorb about a quarter of the ray, whatever K and S; the dominant segment most of the rest
    sigma = (rn(N, S) + np.log(0.25 / (K * S))).astype(np.float32)
    s = 0
    for p in range(P):
        k = int(n_seg[p])
        if k == 0:
            continue
        idx = np.arange(s, s + k)
        pix_segs[p, :k], seg_entity[idx] = idx, np.arange(k)
        zn[idx] = 0.5 + r(k)
        zf[idx] = zn[idx] + 0.5 + 2 * r(k)                          # ranges that overlap: the merged order interleaves
        if regime == "ties":
            zn[idx], zf[idx] = zn[idx[0]], zf[idx[0]]
        dom = idx[int(r(1)[0] * k) % k]
        sigma[dom] = rn(S) * 2 + (4.0 if S == 1 else 1.0)
        s += k
    if regime == "ties":
        z = zn[:, None] + (np.arange(S, dtype=np.float32)[None] + np.float32(0.5)) * (zf - zn)[:, None] / np.float32(S)
    else:
        z = np.sort(zn[:, None] + r(N, S) * (zf - zn)[:, None], axis=1)
    z = z.astype(np.float32)
    color = r(N, S, 3)
    if regime == "saturated":                                       # the front sample of every pixel is solid
        for p in range(P):
            segs = pix_segs[p][pix_segs[p] >= 0]
            if len(segs):
                sigma[segs[np.argmin(z[segs, 0])], 0] = 200.0
    if regime == "empty":
        sigma[:] = -200.0
    inst = (10 + np.arange(KMAX)).astype(np.int32)
    return dict(sigma=sigma, color=color, z=z, pix_segs=pix_segs, seg_entity=seg_entity, inst=inst, P=P, S=S, N=N)


def gpu_composite(cnr, dev, c, thr=0.5):
    P, S = c["P"], c["S"]
    out = dict(rgb=_nan(dev, P, 3), depth=_nan(dev, P), opacity=_nan(dev, P), var=_nan(dev, P), mass=_nan(dev, P, KMAX),
               instance=_m7(dev, P))
    cnr._C.call("cnr_view_composite", _t(c["sigma"], dev), _t(c["color"], dev), _t(c["z"], dev), _t(c["pix_segs"], dev),
                _t(c["seg_entity"], dev), _t(c["inst"], dev), P, S, thr, out["rgb"], out["depth"], out["opacity"], out["var"],
                out["mass"], out["instance"])
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _check_composite(got, c, what, thr=0.5):
    args = (c["sigma"], c["color"], c["z"], c["pix_segs"], c["seg_entity"], c["inst"], thr)
    w64, w32 = V.composite(*args, np.float64), V.composite(*args, np.float32)
    for k in ("rgb", "depth", "opacity", "var", "mass"):
        check(got[k], torch.from_numpy(w64[k]), torch.from_numpy(w32[k]), f"{what} {k}")
    top = np.sort(w64["mass"], axis=1)[:, ::-1]
    live = c["pix_segs"][:, 1] >= 0
    assert (top[live, 0] - top[live, 1] >= 0.05).all() or (c["sigma"] == -200).all(), "the case must keep the two largest masses apart"
    assert (np.abs(w64["opacity"] - thr) > 1e-4).all(), "the case must keep opacity off the threshold"
    assert np.array_equal(got["instance"].numpy(), w64["instance"]) and np.array_equal(w32["instance"], w64["instance"])
    return w64


CASES = [(1, 1), (1, 64), (3, 5), (2, 33), (8, 128)]


@pytest.mark.parametrize("K,S", CASES, ids=["K%d_S%d" % c for c in CASES])
def test_composite(cnr, dev, K, S):
    c = composite_case(K, S)
    got = gpu_composite(cnr, dev, c)
    w64 = _check_composite(got, c, f"K={K} S={S}")
    none = c["pix_segs"][:, 0] < 0
    assert none.any() and (c["pix_segs"][:, K - 1] >= 0).any()
    for k in ("rgb", "depth", "opacity", "var", "mass"):
        assert not got[k][torch.from_numpy(none)].any(), k
    assert (got["instance"][torch.from_numpy(none)] == -1).all()
    assert (w64["instance"] >= 10).any()
    if (K, S) == (1, 64):             # one segment per pixel: cnr_composite_fwd on the same arrays, under the same rule
        N = c["N"]
        ray = dict(depth=_nan(dev, N), var=_nan(dev, N), rgb=_nan(dev, N, 3), opacity=_nan(dev, N))
        cnr._C.call("cnr_composite_fwd", _t(c["sigma"], dev), _t(c["color"], dev), _t(c["z"], dev), None, ray["depth"], ray["var"],
                    ray["rgb"], ray["opacity"], N, S, 0)
        torch.cuda.synchronize()
        args = (c["sigma"], c["color"], c["z"], c["pix_segs"], c["seg_entity"], c["inst"], 0.5)
        w32 = V.composite(*args, np.float32)
        pix = np.nonzero(~none)[0]
        assert np.array_equal(c["pix_segs"][pix, 0], np.arange(N))
        for k in ray:
            check(ray[k].cpu(), torch.from_numpy(w64[k][pix]), torch.from_numpy(w32[k][pix]), f"cnr_composite_fwd {k}")


@pytest.mark.parametrize("regime", ["ties", "saturated", "empty"])
@pytest.mark.parametrize("K,S", [(3, 5), (8, 128)], ids=["K3_S5", "K8_S128"])
def test_composite_regimes(cnr, dev, K, S, regime):
    c = composite_case(K, S, regime)
    got = gpu_composite(cnr, dev, c)
    w64 = _check_composite(got, c, f"{regime} K={K} S={S}")
    some = c["pix_segs"][:, 0] >= 0
    if regime == "empty":
        assert (got["opacity"] < 0.5).all() and (got["instance"] == -1).all()
    if regime == "saturated":       # all behind the solid front sample carries at most 1e-10 of its value
        for p in np.nonzero(some)[0]:
            segs = c["pix_segs"][p][c["pix_segs"][p] >= 0]
            f = int(np.argmin(c["z"][segs, 0]))
            behind = float(sum(got["mass"][p, k] for k in range(KMAX) if k != f))
            assert behind <= 1.0001e-10 * len(segs) and abs(float(got["opacity"][p]) - 1.0) <= 2.0 ** -22
            assert abs(float(got["depth"][p]) - float(c["z"][segs[f], 0])) <= 2.0 ** -22 * 8 + 1e-9
            assert int(got["instance"][p]) == 10 + f
    if regime == "ties":            # equal z across segments: the order is by segment, then sample
        assert (w64["instance"][some] >= 10).all()


# ---- end to end -------------------------------------------------------------------------------------------------------
SEED, S_E2E = 2, 16


@pytest.fixture(scope="module")
def e2e(cnr, dev):
    cfg = VS.small_camera(cnr.cfg.synthetic_config(device=str(dev), latent_dim=32))
    cls_dict, scene_bg = VS.make_scene(cnr, cfg, seed=SEED)
    r = cnr.view.SceneRenderer(cls_dict, scene_bg, cfg)
    T = VS.camera_pose()
    with torch.no_grad():
        out = r.render(T, n_samples=S_E2E)
    return cfg, cls_dict, scene_bg, r, T, out


def _against_restatement(out, ref, what):
    W, H = out["depth"].shape
    for k in ("rgb", "depth", "opacity"):
        e = rel_l2(out[k].reshape(W * H, -1), torch.from_numpy(ref[k]).reshape(W * H, -1))
        print(f"{what}: rel_l2 {k} {e:.3e}")
        assert e <= 1e-3, (what, k, e)
    top = np.sort(ref["mass"], axis=1)[:, ::-1]
    sure = (top[:, 0] - top[:, 1] >= 1e-2) & (np.abs(ref["opacity"] - 0.5) >= 1e-2)
    print(f"{what}: instance compared on {int(sure.sum())} of {len(sure)} pixels")
    assert (~sure).mean() <= 0.05
    assert np.array_equal(out["instance"].reshape(-1).cpu().numpy()[sure], ref["instance"][sure])


def test_end_to_end_against_the_restatement(cnr, dev, e2e):
    """SceneRenderer.render against tests/view_cpu.py in float64 with oracle field values.  Excluded from the instance
    comparison at SEED = 2 (top two masses closer than 1e-2, or opacity within 1e-2 of the threshold): 1 of 432 pixels
    (0.2 %), for the moved scene of test_transform_edit_against_the_restatement as well; measured with the restatement alone,
    whose float32 and float64 runs agree on every other pixel.  The scene shows the labels -1, 0, 1, 2 and 3."""
    cfg, cls_dict, scene_bg, r, T, out = e2e
    ref = VS.restated_render(r, cls_dict, scene_bg, T, S_E2E, np.float64)
    assert len(np.unique(ref["instance"])) >= 3, "the scene must show several instances"
    assert (ref["seg"]["hit"].sum(0) >= 3).any(), "the footprints must overlap"
    _against_restatement(out, ref, "e2e")


def test_chunks_do_not_change_a_bit(cnr, dev, e2e):
    cfg, cls_dict, scene_bg, r, T, out = e2e
    with torch.no_grad():
        small = r.render(T, n_samples=S_E2E, chunk=64)
    for k in ("rgb", "depth", "opacity", "var", "instance"):
        assert torch.equal(small[k], out[k]), k


def test_hidden_is_a_scene_without_the_object(cnr, dev, e2e):
    cfg, cls_dict, scene_bg, r, T, out = e2e
    with torch.no_grad():
        hid = r.render(T, n_samples=S_E2E, hidden={3})
    assert not torch.equal(hid["rgb"], out["rgb"]) and not bool((hid["instance"] == 3).any())
    without = cnr.view.SceneRenderer({10: cls_dict[10]}, scene_bg, cfg)
    with torch.no_grad():
        ref = without.render(T, n_samples=S_E2E)
    for k in ("rgb", "depth", "opacity", "var", "instance"):
        assert torch.equal(hid[k], ref[k]), k


def test_transform_edit_against_the_restatement(cnr, dev, e2e):
    cfg, cls_dict, scene_bg, r, T, out = e2e
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = 1.2 * V.rot((0, 1, 0.3), 0.5), (0.3, 0.1, -0.2)
    with torch.no_grad():
        moved = r.render(T, n_samples=S_E2E, transforms={2: E})
        again = r.render(T, n_samples=S_E2E)
    assert not torch.equal(moved["rgb"], out["rgb"])
    assert all(torch.equal(again[k], out[k]) for k in out), "an edit must leave the scene as it was"
    ref = VS.restated_render(r, cls_dict, scene_bg, T, S_E2E, np.float64, transforms={2: E})
    _against_restatement(moved, ref, "moved")


def test_return_samples_and_files(cnr, dev, e2e, tmp_path):
    from PIL import Image
    cfg, cls_dict, scene_bg, r, T, out = e2e
    with torch.no_grad():
        full = r.render(T, n_samples=S_E2E, return_samples=True)
    s = full["samples"]
    assert s["z"].shape == (s["seg_pixel"].shape[0], S_E2E) and s["pix_segs"].shape == (cfg.W * cfg.H, KMAX)
    assert torch.equal(full["rgb"], out["rgb"])
    with pytest.raises(ValueError):
        r.render(T, n_samples=S_E2E, return_samples=True, chunk=64)
    cnr.view.render_to_files(out, str(tmp_path))
    depth = np.asarray(Image.open(os.path.join(tmp_path, "depth.png")))
    assert depth.shape == (cfg.H, cfg.W) and depth.dtype == np.uint16
    want = np.round(out["depth"].double().cpu().numpy() * 1000).T
    assert np.array_equal(depth.astype(np.int64), want.astype(np.int64))
    inst = np.asarray(Image.open(os.path.join(tmp_path, "instance.png"))).astype(np.int64)
    assert np.array_equal(np.where(inst == 65535, -1, inst), out["instance"].cpu().numpy().T)
    rgb = np.asarray(Image.open(os.path.join(tmp_path, "rgb.png")))
    assert rgb.shape == (cfg.H, cfg.W, 3)
    assert np.abs(rgb.astype(np.float64) / 255 - out["rgb"].cpu().numpy().transpose(1, 0, 2)).max() <= 0.5 / 255 + 1e-6
