"""GPU: cnr_obj_train (csrc/obj_fused.hip) -- one launch = one train step of every per-object field -- and
object_fields.ObjectFieldTrainer on top of it.

Reference: tests/golden/bg_r100_s14_h32.npz (one such step as the REFERENCE computed it) and, for every other shape, objfield_cpu
in fp64, which tests/test_objfields_host.py ties to that vector.  Bars: the ones tests/test_bg_fused_gpu.py holds the hidden-128
step to against the reference -- z exact, sigma 2e-5, rgb 1e-3, loss terms 1e-3, gradient cosine 0.999, worst tensor 0.06, AdamW
update 0.02 where |g| > 2 % of max -- and rel_l2 5e-3 on the parameters after three steps (the drift bar of
test_fused_background_trainer_tracks_the_fp32_tier)."""
import os
import shutil

import numpy as np
import pytest
import torch

import objfield_cpu as OC
from conftest import Golden, rel_l2

pytestmark = pytest.mark.gpu
EPS, STOP_EPS, SCALE, LR, WD = 0.1, 0.05, 2.0, 1e-3, 0.013
DS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataset")


@pytest.fixture(scope="module")
def cnr():
    import cnr_amd
    return cnr_amd


def launch(cnr, dev, pools, theta, m, v, state, R, n1, n2, rows=None, u=None, g=None, seed=0, ids=None, eps=EPS, stop_eps=STOP_EPS,
           scale=SCALE, want=True, min_rows=None):
    """one cnr_obj_train launch on host-side pools [{rgbs, depth, dirs, T_wc}] -> dict of host tensors; theta / m / v / state are
    device tensors updated in place"""
    _C = cnr._C
    N, S = len(pools), n1 + n2
    cat = lambda k: torch.cat([p[k] for p in pools]).to(dev).contiguous()
    lens = [len(p["depth"]) for p in pools]
    off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64, device=dev)
    f = lambda *sh, dt=torch.float32: torch.zeros(*sh, device=dev, dtype=dt)
    out = dict(losses=f(3, N), flags=f(N, dt=torch.int32))
    if want:
        out.update(grad=f(N, OC.P), sigma=f(N, R, S), rgb=f(N, R, S, 3), z=f(N, R, S), rows_out=f(N, R, dt=torch.int32))
    ws = _C.workspace(_C.load().cnr_obj_workspace_bytes(max(N, 1), R, min(S, 64)), dev, "cnr_obj_train")
    dv = lambda t, dt: None if t is None else t.to(dev, dt).contiguous()
    _C.call("cnr_obj_train", cat("rgbs"), cat("depth"), cat("dirs"), cat("T_wc"), off, min(lens) if min_rows is None else min_rows,
            dv(ids, torch.int32), N, R, n1, n2, eps, stop_eps, 0.0, scale, seed, dv(rows, torch.int32), dv(u, torch.float32),
            dv(g, torch.float32), state, theta, m, v, LR, 0.9, 0.999, 1e-8, WD, 5.0, 10.0, out["losses"], out["flags"],
            out.get("grad"), out.get("sigma"), out.get("rgb"), out.get("z"), out.get("rows_out"), ws, ws.numel())
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in out.items()}


def fresh(dev, thetas):
    th = torch.stack(thetas).to(dev).contiguous()
    return th, torch.zeros_like(th), torch.zeros_like(th), torch.zeros(len(thetas), 4, device=dev, dtype=torch.int64)


def check_step(tag, got, o, ref, upd_got=None, upd_ref=None, losses=True, grad_abs=None):
    """one object's step against its reference dict (z, sigma, rgb, losses, grad) and its parameter update against the
    reference's, at the bars of the module docstring.  ``grad_abs``: the reference gradient is numerically zero (see the empty-mask
    test); the gradient is then held to that absolute bound and the update is not compared."""
    assert torch.equal(got["z"][o], ref["z"].float()), tag
    e_sig, e_rgb = rel_l2(got["sigma"][o], ref["sigma"]), rel_l2(got["rgb"][o], ref["rgb"])
    e_loss = [rel_l2(got["losses"][k, o], ref["losses"][k]) for k in range(3)]
    grad, gref = got["grad"][o].double(), ref["grad"].double()
    worst, off = 0.0, 0
    for s in OC.SHAPES + [(21, 3)]:
        k = int(np.prod(s))
        worst = max(worst, rel_l2(grad[off:off + k], gref[off:off + k]))
        off += k
    cos = float(grad @ gref / (grad.norm() * gref.norm())) if float(gref.norm()) > 0 else 1.0
    clear = gref.abs() > 0.02 * gref.abs().max()
    e_upd = rel_l2(upd_got.double()[clear], upd_ref.double()[clear]) if upd_got is not None else float("nan")
    print(f"{tag}: sigma {e_sig:.2e} rgb {e_rgb:.2e} losses {e_loss[0]:.2e} {e_loss[1]:.2e} {e_loss[2]:.2e} "
          f"cos {cos:.7f} worst {worst:.2e} update {e_upd:.2e} |grad| {float(gref.norm()):.2e} max abs err {float((grad - gref).abs().max()):.2e}")
    assert e_sig < 2e-5 and e_rgb < 1e-3, tag
    if losses:
        assert max(e_loss) < 1e-3, tag
    if grad_abs is not None:
        assert float((grad - gref).abs().max()) < grad_abs, tag
        return
    assert cos > 0.999 and worst < 0.06, tag
    if upd_got is not None:
        assert e_upd < 0.02, tag


def make_pool(cnr, n, gen):
    p = cnr.scene_cateogries.synthetic_pool(n, 1, gen, "cpu")
    return dict(rgbs=p["rgbs"], depth=p["depth"], dirs=p["dirs"], T_wc=p["T_wc"])


def draws(gen, R, n1, n2):
    return torch.rand(R, n1 + n2, generator=gen), torch.randn(R, n2, generator=gen) * (EPS / 3)


def oracle_step(orc, pool, rows, u, g):
    r = rows.long()
    return orc.step(pool["rgbs"][r], pool["depth"][r], pool["dirs"][r], pool["T_wc"][r], u, g)


# ---- 1. the reference's vector ---------------------------------------------------------------------------------------------------
def test_one_object_step_against_the_reference_vector(cnr, dev):
    g = Golden("bg_r100_s14_h32")
    R, S = g.R, g.S
    pool = dict(rgbs=g.t("pool_rgbs")[0], depth=g.t("pool_depth")[0], dirs=g.t("pool_dirs")[0], T_wc=g.t("pool_T")[0])
    theta0 = OC.flatten(g.mlp(), g.t("B")[0])
    assert theta0.numel() == int(cnr._C.load().cnr_obj_param_count()) == 11363
    ref = dict(z=g.t("z")[0], sigma=g.t("sigmas")[0].squeeze(-1), rgb=g.t("rgbs")[0],
               losses=torch.stack([g.t("loss_depth")[0], g.t("loss_color")[0], g.t("loss_opacity")[0]]),
               grad=OC.flatten(g.mlp("grad."), g.t("grad_B")[0]), theta=OC.flatten(g.mlp("new."), g.t("new_B")[0]))
    rows = torch.arange(R, dtype=torch.int32)[None]
    kw = dict(rows=rows, u=g.t("u"), g=g.t("g"), eps=g.eps, stop_eps=g.stop_eps, scale=g.scale)
    th, m, v, st = fresh(dev, [theta0])
    got = launch(cnr, dev, [pool], th, m, v, st, R, g.n1, g.n2, **kw)
    check_step("reference vector r100 s14", got, 0, ref, th[0].cpu() - theta0, ref["theta"] - theta0)
    assert st.cpu().tolist() == [[0, 1, 1, 1]]                    # 100 rows, 100 rays: the cursor wrapped, the epoch moved
    assert got["flags"].tolist() == [0] and torch.equal(got["rows_out"][0], rows[0])
    th2, m2, v2, st2 = fresh(dev, [theta0])
    got2 = launch(cnr, dev, [pool], th2, m2, v2, st2, R, g.n1, g.n2, **kw)
    assert torch.equal(th2, th) and torch.equal(m2, m) and torch.equal(v2, v)
    assert all(torch.equal(got[k], got2[k]) for k in got)


# ---- 2., 3. a ragged batch over three steps; an object alone ------------------------------------------------------------------------
R2, N1, N2 = 120, 3, 7


@pytest.fixture(scope="module")
def ragged(cnr, dev):
    gen = torch.Generator().manual_seed(11)
    pools = [make_pool(cnr, n, gen) for n in (250, 400, 1000)]
    inits = [OC.init_params(torch.Generator().manual_seed(100 + o), jitter_B=0.02) for o in range(3)]
    thetas = [OC.flatten(*i) for i in inits]
    steps = []
    for _ in range(3):
        rows = torch.stack([torch.randperm(len(p["depth"]), generator=gen)[:R2].to(torch.int32) for p in pools])
        ug = [draws(gen, R2, N1, N2) for _ in pools]
        steps.append((rows, torch.stack([a for a, _ in ug]), torch.stack([b for _, b in ug])))
    th, m, v, st = fresh(dev, thetas)
    got, after = [], []
    for rows, u, g in steps:
        got.append(launch(cnr, dev, pools, th, m, v, st, R2, N1, N2, rows=rows, u=u, g=g))
        after.append((th.cpu().clone(), m.cpu().clone(), v.cpu().clone()))
    return dict(pools=pools, inits=inits, thetas=thetas, steps=steps, got=got, after=after, state=st.cpu())


def test_ragged_batch_tracks_the_fp64_oracle_over_three_steps(cnr, dev, ragged):
    """Every step of every object against ONE fp64 step from the state the kernel's step started from (parameters, both AdamW
    moments, step count), at the per-step bars; and a second fp64 oracle that runs free from the initial parameters, for the
    drift bar after three steps.  (The per-step bars cannot be asked of the free-running oracle: a weight whose gradient is near
    1e-8, AdamW's eps, moves by lr g / (|g| + eps), which turns the last bits of g into a visible share of lr -- the parameters of
    two correct runs part by that after ONE step, in weights the loss hardly feels, and step two's sigma then differs by 3e-5
    where its own arithmetic is good to 1e-6.  That is the drift the 5e-3 bar is for.)"""
    zeros = torch.zeros(OC.P)
    for o in range(3):
        kw = dict(lr=LR, weight_decay=WD, dtype=torch.float64)
        free = OC.ObjectOracle(*ragged["inits"][o], SCALE, N1, N2, EPS, STOP_EPS, **kw)
        orc = OC.ObjectOracle(*ragged["inits"][o], SCALE, N1, N2, EPS, STOP_EPS, **kw)
        before = (ragged["thetas"][o], zeros, zeros)
        for k, (rows, u, g) in enumerate(ragged["steps"]):
            oracle_step(free, ragged["pools"][o], rows[o], u[o], g[o])
            if k:
                orc.load_state(*before, k)
            ref = oracle_step(orc, ragged["pools"][o], rows[o], u[o], g[o])
            now = tuple(t[o] for t in ragged["after"][k])
            check_step(f"object {o} step {k}", ragged["got"][k], o, ref, now[0] - before[0], ref["theta"] - before[0].double())
            before = now
        drift = rel_l2(ragged["after"][2][0][o], free.theta())
        print(f"object {o}: parameters after 3 steps rel_l2 {drift:.2e}")
        assert drift < 5e-3
    rows_o = [250, 400, 1000]
    want = [[0, 0, 0, 0]] * 3
    for _ in range(3):
        want = [cnr.object_fields.next_state(s, n, R2) for s, n in zip(want, rows_o)]
    assert ragged["state"].tolist() == want
    assert ragged["got"][2]["flags"].tolist() == [0, 0, 0]


def test_an_object_alone_equals_itself_in_the_batch_bit_for_bit(cnr, dev, ragged):
    th, m, v, st = fresh(dev, [ragged["thetas"][1]])
    for k, (rows, u, g) in enumerate(ragged["steps"]):
        got = launch(cnr, dev, [ragged["pools"][1]], th, m, v, st, R2, N1, N2, rows=rows[1:2], u=u[1:2], g=g[1:2])
        for key in ("grad", "sigma", "rgb", "z"):
            assert torch.equal(got[key][0], ragged["got"][k][key][1]), (k, key)
        assert torch.equal(got["losses"][:, 0], ragged["got"][k]["losses"][:, 1])
    for mine, batch in zip((th, m, v), ragged["after"][2]):
        assert torch.equal(mine[0].cpu(), batch[1])


# ---- 4. rays against the 64-sample tile --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,n1,n2", [(7, 3, 7), (3, 8, 56)])
def test_tiles_of_whole_rays(cnr, dev, R, n1, n2):
    """R = 7, S = 10: 70 samples = a tile of six rays and one of a single ray; R = 3, S = 64: a ray fills the tile"""
    gen = torch.Generator().manual_seed(21 + R)
    pools = [make_pool(cnr, n, gen) for n in (20, 33)]
    inits = [OC.init_params(torch.Generator().manual_seed(200 + o), jitter_B=0.02) for o in range(2)]
    thetas = [OC.flatten(*i) for i in inits]
    rows = torch.stack([torch.randperm(len(p["depth"]), generator=gen)[:R].to(torch.int32) for p in pools])
    ug = [draws(gen, R, n1, n2) for _ in pools]
    u, g = torch.stack([a for a, _ in ug]), torch.stack([b for _, b in ug])
    th, m, v, st = fresh(dev, thetas)
    got = launch(cnr, dev, pools, th, m, v, st, R, n1, n2, rows=rows, u=u, g=g)
    for o in range(2):
        orc = OC.ObjectOracle(*inits[o], SCALE, n1, n2, EPS, STOP_EPS, lr=LR, weight_decay=WD, dtype=torch.float64)
        ref = oracle_step(orc, pools[o], rows[o], u[o], g[o])
        # (z, sigma, rgb and the gradient; with 64 samples per ray the opacity is 1 to rounding, and |opacity - 1| is no number
        # a relative bar can be asked of)
        check_step(f"R {R} S {n1 + n2} object {o}", got, o, ref, losses=False)


# ---- 5. empty masks ---------------------------------------------------------------------------------------------------------------
def test_empty_masks_zero_their_terms_for_that_object_only(cnr, dev):
    gen = torch.Generator().manual_seed(31)
    pools = [make_pool(cnr, 300, gen) for _ in range(3)]
    pools[0]["depth"] = torch.zeros(300)                           # no valid depth: the depth count is zero
    pools[1]["rgbs"][:, 3] = 0                                     # every pixel another object's: depth and colour counts are zero
    inits = [OC.init_params(torch.Generator().manual_seed(300 + o), jitter_B=0.02) for o in range(3)]
    thetas = [OC.flatten(*i) for i in inits]
    rows = torch.stack([torch.randperm(300, generator=gen)[:R2].to(torch.int32) for _ in pools])
    ug = [draws(gen, R2, N1, N2) for _ in pools]
    u, g = torch.stack([a for a, _ in ug]), torch.stack([b for _, b in ug])
    th, m, v, st = fresh(dev, thetas)
    got = launch(cnr, dev, pools, th, m, v, st, R2, N1, N2, rows=rows, u=u, g=g)
    assert got["flags"].tolist() == [2, 2 | 4, 0]
    assert got["losses"][0, 0] == 0 and got["losses"][0, 1] == 0 and got["losses"][1, 1] == 0
    assert (got["losses"][1:, 0] > 0).all() and got["losses"][2, 1] > 0 and (got["losses"][:, 2] > 0).all()
    for t in list(got.values()) + [th.cpu(), m.cpu(), v.cpu()]:
        assert torch.isfinite(t.float()).all()
    refs = []
    for o in range(3):
        orc = OC.ObjectOracle(*inits[o], SCALE, N1, N2, EPS, STOP_EPS, lr=LR, weight_decay=WD, dtype=torch.float64)
        refs.append(oracle_step(orc, pools[o], rows[o], u[o], g[o]))
    # Object 1 keeps its opacity term alone, and on this pool every ray's opacity is 1 to rounding (the term is 1.0): the oracle's
    # gradient is 1e-10 of a regular object's, the derivative of a saturated product.  fp32 cannot resolve that -- the oracle
    # itself, run in fp32, is at cosine -0.3 to its fp64 self -- so no relative bar applies; what can be asked is that nothing
    # else leaks in: the gradient is zero to the rounding of a regular one, fp32's 6e-8 x 16 for the sums = 1e-6 of object 2's
    # largest element.
    tiny = 1e-6 * float(refs[2]["grad"].abs().max())
    assert float(refs[1]["grad"].abs().max()) < tiny
    for o in range(3):
        check_step(f"empty masks object {o}", got, o, refs[o], th[o].cpu() - thetas[o], refs[o]["theta"] - thetas[o].double(),
                   grad_abs=tiny if o == 1 else None)
    # object 1's colour branch gets no gradient at all: its colour count is zero
    off = sum(int(np.prod(s)) for s in OC.SHAPES[:10])
    assert float(got["grad"][1][off:off + 32 * 74 + 32 + 99].abs().max()) == 0.0
    th1, m1, v1, st1 = fresh(dev, [thetas[2]])
    solo = launch(cnr, dev, [pools[2]], th1, m1, v1, st1, R2, N1, N2, rows=rows[2:3], u=u[2:3], g=g[2:3])
    assert torch.equal(th1[0], th[2]) and torch.equal(solo["grad"][0], got["grad"][2]) and torch.equal(solo["losses"][:, 0], got["losses"][:, 2])


# ---- 6. rows, epochs and state on the device ----------------------------------------------------------------------------------------
def test_rows_epochs_and_state_in_philox_mode(cnr, dev):
    gen = torch.Generator().manual_seed(41)
    lens = [250, 1000]
    pools = [make_pool(cnr, n, gen) for n in lens]
    thetas = [OC.flatten(*OC.init_params(torch.Generator().manual_seed(400 + o))) for o in range(2)]
    th, m, v, st = fresh(dev, thetas)
    want, seen = [[0, 0, 0, 0], [0, 0, 0, 0]], [{}, {}]
    for k in range(16):                                            # two epochs of the long pool (8 steps each), eight of the short
        got = launch(cnr, dev, pools, th, m, v, st, R2, N1, N2, seed=5)
        for o in range(2):
            r = got["rows_out"][o]
            assert int(r.min()) >= 0 and int(r.max()) < lens[o]
            seen[o].setdefault(want[o][3], []).append(r)
        want = [cnr.object_fields.next_state(s, n, R2) for s, n in zip(want, lens)]
        assert st.cpu().tolist() == want, k
    assert want == [[0, 16, 16, 8], [0, 16, 16, 2]]
    for o in range(2):
        for ep, chunks in seen[o].items():
            allr = torch.cat(chunks)
            assert len(torch.unique(allr)) == len(allr), (o, ep)   # a bijection: no row twice within an epoch
        assert not torch.equal(torch.cat(seen[o][0]), torch.cat(seen[o][1]))
    assert torch.isfinite(th).all()
    # two objects with the SAME pool and parameters: their ids alone give them different rows and different draws
    th, m, v, st = fresh(dev, [thetas[0], thetas[0]])
    got = launch(cnr, dev, [pools[0], pools[0]], th, m, v, st, R2, N1, N2, seed=5, ids=torch.tensor([3, 9]))
    assert not torch.equal(got["rows_out"][0], got["rows_out"][1]) and not torch.equal(got["z"][0], got["z"][1])
    again = fresh(dev, [thetas[0], thetas[0]])
    got2 = launch(cnr, dev, [pools[0], pools[0]], *again, R2, N1, N2, seed=5, ids=torch.tensor([9, 3]))
    assert torch.equal(got2["rows_out"][0], got["rows_out"][1]) and torch.equal(got2["z"][1], got["z"][0])
    assert torch.equal(again[0][0], th[1])                          # an object's step follows its id, not its place in the launch


# ---- 7. argument errors ------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_return_codes(cnr, dev):
    gen = torch.Generator().manual_seed(51)
    pool = make_pool(cnr, 200, gen)
    theta = OC.flatten(*OC.init_params(gen))
    th, m, v, st = fresh(dev, [theta])
    err = cnr._C.CnrError
    with pytest.raises(err, match="code -1"):
        launch(cnr, dev, [pool], th, m, v, st, R2, 8, 57, want=False)                    # S = 65
    with pytest.raises(err, match="code -1"):
        launch(cnr, dev, [pool], th, m, v, st, 201, N1, N2, want=False)                  # a pool shorter than R
    with pytest.raises(err, match="code -1"):
        launch(cnr, dev, [pool], th, m, v, st, R2, N1, N2, want=False, min_rows=119)
    _C = cnr._C
    ws = torch.zeros(64, device=dev, dtype=torch.uint8)
    off = torch.zeros(1, device=dev, dtype=torch.int64)
    with pytest.raises(err, match="code -1"):                                            # N = 0
        _C.call("cnr_obj_train", pool["rgbs"].to(dev), pool["depth"].to(dev), pool["dirs"].to(dev), pool["T_wc"].to(dev), off, 200,
                None, 0, R2, N1, N2, EPS, STOP_EPS, 0.0, SCALE, 0, None, None, None, st, th, m, v, LR, 0.9, 0.999, 1e-8, WD, 5.0, 10.0,
                torch.zeros(3, 1, device=dev), torch.zeros(1, device=dev, dtype=torch.int32), None, None, None, None, None, ws,
                ws.numel())
    assert int(_C.load().cnr_obj_workspace_bytes(1, R2, 65)) == -1 and int(_C.load().cnr_obj_workspace_bytes(0, R2, 10)) == -1
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [[0, 0, 0, 0]] and torch.equal(th[0].cpu(), theta)      # nothing was launched


# ---- 8. the trainer ----------------------------------------------------------------------------------------------------------------
def _trainer(cnr, dev, seed=3):
    cfg = cnr.cfg.synthetic_config(device=str(dev), n_bins_cam2surface=3, n_bins=7)
    gen = torch.Generator().manual_seed(61)
    pools = {}
    for k, obj_id in enumerate((4, 11, 12)):
        p = make_pool(cnr, 1500 + 500 * k, gen)
        # synthetic_pool's colours are independent noise per ray, which no field can fit: one colour per object instead
        p["rgbs"][:, :3] = torch.tensor([[200, 60, 30], [20, 180, 90], [90, 40, 220]], dtype=torch.uint8)[k]
        pools[obj_id] = p
    return cfg, cnr.object_fields.ObjectFieldTrainer(cfg, pools, [4, 11, 12], rays_per_step=120, seed=seed)


def test_trainer_learns_replays_and_checkpoints(cnr, dev, tmp_path):
    cfg, tr = _trainer(cnr, dev)
    _, eager = _trainer(cnr, dev)
    assert torch.equal(tr.theta, eager.theta) and not torch.equal(tr.theta[0], tr.theta[1])
    tr.step()
    first = tr.losses.cpu().clone()
    tr.run(11)                                                     # eager warm-up, then graphs of up to 8 steps
    for _ in range(12):
        eager.step(use_graph=False)
    assert tr.steps_done == eager.steps_done == 12 and tr._sched.graphs
    assert torch.equal(tr.theta, eager.theta) and torch.equal(tr.exp_avg_sq, eager.exp_avg_sq)
    assert torch.equal(tr.d_state, eager.d_state) and torch.equal(tr.losses, eager.losses)
    tr.run(288)
    last = tr.losses.cpu()
    print("colour term, first step", first[1].tolist(), "after 300 steps", last[1].tolist())
    assert torch.isfinite(tr.theta).all() and torch.isfinite(last).all() and tr.flags.cpu().tolist() == [0, 0, 0]
    assert (last[1] < first[1]).all()
    assert tr.state() == [[s[0], 300, 300, s[3]] for s in tr.state()]
    # checkpoints: what registration loads is what the trainer holds
    files = tr.save_checkpoints(str(tmp_path), {4: "box-4", 11: "box-11", 12: "box-12"})
    assert [os.path.relpath(f, str(tmp_path)) for f in files] == [os.path.join("ckpt", str(i), "obj_%d_it_00300.pth" % i) for i in (4, 11, 12)]
    cfg.weight_root, cfg.data_device = str(tmp_path), str(dev)
    boxes, pes, fcs = {}, {}, {}
    cnr.category_registration.load_pretrained_fields({7: {4: {}, 11: {}, 12: {}}}, boxes, pes, fcs, cfg)
    z_vals = torch.rand(10000, 96, generator=torch.Generator().manual_seed(2)) * 1.2
    for obj_id in (4, 12):
        pe, fc = tr.modules(obj_id)
        assert pe.B_layer.weight.data_ptr() == tr.theta[tr.index[obj_id], 11300:].data_ptr()      # views, no copy
        a = cnr.category_registration.uncertainty_probe(pe, fc, [0.1, 0.0, -0.2], 0.6, dev, z_vals=z_vals)
        b = cnr.category_registration.uncertainty_probe(pes[7][obj_id], fcs[7][obj_id], [0.1, 0.0, -0.2], 0.6, dev, z_vals=z_vals)
        assert torch.equal(a[0], b[0]) and boxes[7][obj_id] == "box-%d" % obj_id


# ---- 9. end to end -----------------------------------------------------------------------------------------------------------------
def test_get_dataset_registers_a_raw_sequence_with_pretrain(cnr, dev, tmp_path):
    from test_dataset_host import _config
    root = str(tmp_path / "replica")
    shutil.copytree(os.path.join(DS, "replica"), root)
    cfg = _config(cnr, "replica", root=root)
    cfg.weight_root, cfg.load_pretrained, cfg.load_registration_result = str(tmp_path / "weights"), False, False
    cfg.data_device = cfg.training_device = str(dev)
    with pytest.raises(NotImplementedError, match="load_pretrained is false"):
        cnr.dataset.get_dataset(cfg, register=True)
    assert not os.path.exists(os.path.join(root, "inst_dict.pkl"))
    # (rays_per_step: the smallest crop pool of this fixture has 420 rows, tests/test_objfields_host.py)
    ds = cnr.dataset.get_dataset(cfg, register=True, pretrain=40, rays_per_step=120)
    ids = []
    for cls_id, d in ds.inst_dict.items():
        if cls_id == 0:
            continue
        for inst_id, e in d.items():
            ids.append(int(inst_id))
            assert "pcs" not in e and np.isfinite(e["T_obj"]).all() and np.linalg.det(e["T_obj"][:3, :3]) > 0
    assert sorted(ids) == [0, 3, 4, 5, 7]
    back = cnr.dataset.load_registration_result(os.path.join(root, "inst_dict.pkl"))
    assert list(back.keys()) == list(ds.inst_dict.keys())
    for i in ids:
        files = os.listdir(os.path.join(cfg.weight_root, "ckpt", str(i)))
        assert files == ["obj_%d_it_00040.pth" % i]
        ck = torch.load(os.path.join(cfg.weight_root, "ckpt", str(i), files[0]), map_location="cpu", weights_only=False)
        assert tuple(ck.keys()) == cnr.object_fields.CKPT_KEYS and ck["bbox"].extent.shape == (3,)
        assert all(torch.isfinite(t).all() for t in ck["FC_state_dict"].values())
