"""GPU: cnr_code_fit (csrc/code_fit.hip) -- one launch = one optimisation step of every candidate of a code fit -- and
code_fit.CodeFitter on top of it.

Reference: tests/golden/edge_single_obj_W.npz (a one-object class step as the REFERENCE computed it, which is exactly one fit step)
and, for every other shape, codefit_cpu in fp64, which tests/test_codefit_host.py ties to that vector.  Bars: the project's -- z
exact, sigma 2e-5, rgb 1e-3, loss terms 1e-3, AdamW update 0.02 where |g| > 2 % of max -- and, for the code gradients, a MEASURED
one: rel_l2 of codefit_cpu run in fp32 against its own fp64 run on the same case is the yardstick (what the reference's own
arithmetic is good for), and the kernel gets 4 times that for its different summation order and its fused multiply-adds.

Measured on MI355X (test 1, edge_single_obj_W): yardstick 4.07e-7, kernel 2.85e-7 (bar 1.63e-6).  Over the 25 candidates of test 2
the yardstick lies between 8.9e-7 and 1.4e-4 and the kernel between 0.15 and 3.5 times its own candidate's yardstick (the closest:
R 13, S 5, candidate 4, kernel 4.47e-6 against a yardstick of 1.26e-6); the three candidates of the empty-mask test are at 0.5 to
1.0 times theirs.  Both are single draws of a rounding error: their ratio scatters from case to case."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import codefit_cpu as FC
from conftest import Golden, rel_l2

pytestmark = pytest.mark.gpu
EPS, STOP_EPS, SCALE, LR, WD = 0.1, 0.05, 2.0, 1e-3, 0.013
DS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataset")


@pytest.fixture(scope="module")
def cnr():
    import cnr_amd
    return cnr_amd


class Case:
    """host-side description of one launch: networks [(params, B)], pools [{rgbs, depth, dirs, T}], their frames, the candidates"""

    def __init__(self, nets, pools, world, cand_net, cand_pool, codes, R, n1, n2, L, ids=None):
        self.nets, self.pools, self.world, self.cand_net, self.cand_pool = nets, pools, world, cand_net, cand_pool
        self.codes0, self.R, self.n1, self.n2, self.L, self.ids = codes.clone(), R, n1, n2, L, ids
        self.K = len(cand_net)

    def device_state(self, dev):
        c = self.codes0.to(dev).contiguous()
        return dict(codes=c, m=torch.zeros_like(c), v=torch.zeros_like(c), state=torch.zeros(self.K, 4, device=dev, dtype=torch.int64),
                    theta=torch.stack([FC.flatten_net(*n) for n in self.nets]).to(dev).contiguous())

    def oracle(self, k, reg, dtype=torch.float64):
        params, B = self.nets[self.cand_net[k]]
        return FC.FitOracle(params, B, self.codes0[k], SCALE, self.n1, self.n2, EPS, STOP_EPS, lr=LR,
                            weight_decay=WD, reg_scaling=reg, world_frame=bool(self.world[self.cand_pool[k]]), dtype=dtype)

    def oracle_step(self, orc, k, rows, u, g):
        p, r = self.pools[self.cand_pool[k]], rows.long()
        return orc.step(p["rgbs"][r], p["depth"][r], p["dirs"][r], p["T"][r], u, g)


def launch(cnr, dev, case, st, rows=None, u=None, g=None, seed=0, reg=0.0, update=1, want=True, min_rows=None, R=None, n1=None, n2=None,
           L=None, theta=None):
    """one cnr_code_fit launch -> dict of host tensors; st (Case.device_state) is updated in place"""
    _C = cnr._C
    K, R = case.K, case.R if R is None else R
    n1, n2 = case.n1 if n1 is None else n1, case.n2 if n2 is None else n2
    S, L = n1 + n2, case.L if L is None else L
    cat = lambda k: torch.cat([p[k] for p in case.pools]).to(dev).contiguous()
    lens = [len(p["depth"]) for p in case.pools]
    off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64, device=dev)
    f = lambda *sh, dt=torch.float32: torch.zeros(*sh, device=dev, dtype=dt)
    i32 = lambda v: None if v is None else torch.as_tensor(v, dtype=torch.int32).to(dev).contiguous()
    out = dict(losses=f(5, K), flags=f(K, dt=torch.int32))
    if want:
        out.update(grad=f(K, 2, L), sigma=f(K, R, S), rgb=f(K, R, S, 3), z=f(K, R, S), rows_out=f(K, R, dt=torch.int32))
    ws = _C.workspace(_C.load().cnr_code_fit_workspace_bytes(K, R, min(S, 64)), dev, "cnr_code_fit")
    dv = lambda t: None if t is None else t.to(dev, torch.float32).contiguous()
    lay = cnr.fused.ParamLayout(L, 0)
    th = st["theta"] if theta is None else theta
    _C.call("cnr_code_fit", th, lay.total, lay.trunk[0], lay.latW[0], lay.latb[0], lay.B[0], len(case.nets), L, cat("rgbs"),
            cat("depth"), cat("dirs"), cat("T"), off, min(lens) if min_rows is None else min_rows, i32(case.ids), i32(case.world),
            len(case.pools), i32(case.cand_net), i32(case.cand_pool), K, R, n1, n2, EPS, STOP_EPS, 0.0, SCALE, seed, i32(rows), dv(u),
            dv(g), st["state"], st["codes"], st["m"], st["v"], update,
            LR, 0.9, 0.999, 1e-8, WD, 5.0, 10.0, reg, out["losses"], out["flags"], out.get("grad"), out.get("sigma"), out.get("rgb"),
            out.get("z"), out.get("rows_out"), ws, ws.numel())
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in out.items()}


def check_step(tag, got, k, ref, ref32, upd_got, upd_ref):
    """Candidate k's step against its fp64 reference dict and, for the gradient's measured bar, the fp32 run of the same oracle.

    A case is ADMITTED only where the fp32 oracle's own loss terms are within 1e-4 of its fp64 ones, a tenth of the bar: on a random
    network a ray that terminates on one sample has a composite variance of ~0, and the depth term's weight 1 / (sqrt(var) + 1e-4)
    then amplifies fp32 rounding beyond any bar (the reference's own arithmetic is off by 5e-3 .. 3e-2 on such a batch).  The seeds
    of the cases below are the first of seed + 1000 j that the ORACLE admits; the kernel has no say in it."""
    assert torch.equal(got["z"][k], ref["z"].float()), tag
    admitted = max(rel_l2(ref32["losses"][i], ref["losses"][i]) for i in range(5))
    assert admitted < 1e-4, f"{tag}: not a case for a relative bar on the losses (fp32 oracle off by {admitted:.1e})"
    e_sig, e_rgb = rel_l2(got["sigma"][k], ref["sigma"]), rel_l2(got["rgb"][k], ref["rgb"])
    e_loss = [rel_l2(got["losses"][i, k], ref["losses"][i]) for i in range(5)]
    grad, gref = got["grad"][k].double(), ref["grad"].double()
    yard, e_grad = rel_l2(ref32["grad"], gref), rel_l2(grad, gref)
    clear = gref.abs() > 0.02 * gref.abs().max()
    e_upd = rel_l2(upd_got.double()[clear], upd_ref.double()[clear])
    print(f"{tag}: sigma {e_sig:.2e} rgb {e_rgb:.2e} losses {' '.join('%.2e' % e for e in e_loss)} gradient {e_grad:.2e} "
          f"(fp32 oracle {yard:.2e}, bar {4 * yard:.2e}) update {e_upd:.2e} |grad| {float(gref.norm()):.2e}")
    assert e_sig < 2e-5 and e_rgb < 1e-3, tag
    assert max(e_loss) < 1e-3, tag
    assert e_grad <= 4 * yard, tag
    assert e_upd < 0.02, tag


def make_pool(cnr, n, gen, world):
    p = cnr.scene_cateogries.synthetic_pool(n, 1, gen, "cpu")
    return dict(rgbs=p["rgbs"], depth=p["depth"], dirs=p["dirs"], T=p["T_wc"] if world else p["T_co"])


def draws(gen, R, n1, n2):
    return torch.rand(R, n1 + n2, generator=gen), torch.randn(R, n2, generator=gen) * (EPS / 3)


# ---- 1. the reference's vector ---------------------------------------------------------------------------------------------------
def test_one_candidate_against_the_reference_vector(cnr, dev):
    g = Golden("edge_single_obj_W")
    params = {k: v[0] for k, v in g.mlp().items()}
    codes = torch.stack([g.t("shape_codes")[0, 0], g.t("texture_codes")[0, 0]])
    pool = dict(rgbs=g.t("pool_rgbs")[0], depth=g.t("pool_depth")[0], dirs=g.t("pool_dirs")[0], T=g.t("pool_T")[0])
    assert (g.eps, g.stop_eps, g.scale) == (np.float32(EPS), np.float32(STOP_EPS), SCALE)
    case = Case([(params, g.t("B")[0])], [pool], [1], [0], [0], codes[None], g.R, g.n1, g.n2, g.L)
    new = torch.stack([g.t("new_shape_codes")[0, 0], g.t("new_texture_codes")[0, 0]])
    ref = dict(z=g.t("z")[0], sigma=g.t("sigmas")[0].squeeze(-1), rgb=g.t("rgbs")[0],
               losses=torch.stack([g.t("loss_depth")[0], g.t("loss_color")[0], g.t("loss_opacity")[0], codes[0].norm(), codes[1].norm()]),
               grad=torch.stack([g.t("grad_shape_codes")[0, 0], g.t("grad_texture_codes")[0, 0]]))
    rows = torch.arange(g.R, dtype=torch.int32)[None]
    kw = dict(rows=rows, u=g.t("u"), g=g.t("g"), reg=0.0)
    # the gradient's yardstick: the restatement in fp32 against itself in fp64, on this case; the reference's recorded gradient is
    # such an fp32 run, so the kernel's is measured against the fp64 one
    r64 = case.oracle_step(case.oracle(0, 0.0), 0, rows[0], g.t("u")[0], g.t("g")[0])
    r32 = case.oracle_step(case.oracle(0, 0.0, torch.float32), 0, rows[0], g.t("u")[0], g.t("g")[0])
    st = case.device_state(dev)
    got = launch(cnr, dev, case, st, **kw)
    assert torch.equal(got["z"][0], ref["z"])
    check_step("reference vector (fp64 oracle)", got, 0, r64, r32, st["codes"][0].cpu() - codes, r64["codes"] - codes.double())
    # ... and the recorded outputs, losses and update themselves at the project's bars
    assert rel_l2(got["sigma"][0], ref["sigma"]) < 2e-5 and rel_l2(got["rgb"][0], ref["rgb"]) < 1e-3
    assert max(rel_l2(got["losses"][i, 0], ref["losses"][i]) for i in range(5)) < 1e-3
    clear = ref["grad"].abs() > 0.02 * ref["grad"].abs().max()
    assert rel_l2((st["codes"][0].cpu() - codes)[clear], (new - codes)[clear]) < 0.02
    assert st["state"].cpu().tolist() == [[0, 1, 1, 1]]            # 64 rows, 64 rays: the cursor wrapped, the epoch moved
    assert got["flags"].tolist() == [0] and torch.equal(got["rows_out"][0], rows[0])
    st2 = case.device_state(dev)
    got2 = launch(cnr, dev, case, st2, **kw)
    assert all(torch.equal(st[k], st2[k]) for k in st) and all(torch.equal(got[k], got2[k]) for k in got)


# ---- 2. object frame, ragged batch, regulariser on ---------------------------------------------------------------------------------
def ragged_case(cnr, R, n1, n2, L, seed):
    gen = torch.Generator().manual_seed(seed)
    world = [0, 1, 0]
    pools = [make_pool(cnr, n, gen, w) for n, w in zip((R + 3, 2 * R + 1, 40), world)]
    nets = [FC.init_net(torch.Generator().manual_seed(seed + 100 + n), L, jitter_B=0.02) for n in range(2)]
    cand_net, cand_pool = [0, 1, 0, 1, 1], [0, 0, 1, 2, 2]
    return Case(nets, pools, world, cand_net, cand_pool, FC.init_codes(gen, L, 5), R, n1, n2, L), gen


def step_draws(case, gen):
    rows = torch.stack([torch.randperm(len(case.pools[p]["depth"]), generator=gen)[:case.R].to(torch.int32) for p in case.cand_pool])
    ug = [draws(gen, case.R, case.n1, case.n2) for _ in range(case.K)]
    return rows, torch.stack([a for a, _ in ug]), torch.stack([b for _, b in ug])


@pytest.mark.parametrize("R,n1,n2,L,seed", [(7, 1, 9, 256, 1007), (3, 0, 64, 256, 2003), (5, 1, 32, 256, 5005), (13, 1, 4, 256, 1013),
                                            (7, 1, 9, 32, 2007)])
def test_ragged_batch_in_both_frames_with_the_regulariser(cnr, dev, R, n1, n2, L, seed):
    """(7, 1, 9): six rays per tile, the last tile one ray; (3, 0, 64): one ray per tile; (5, 1, 32): S = 33, 31 idle sample slots;
    (13, 1, 4): twelve rays per tile, the second tile one ray; and L = 32.  Five candidates over three pools of unequal length in
    both frames and two networks.  (Seeds: 1000 + R + 1000 j, the first the oracle admits -- check_step.  1003 is turned away at S = 64:
    one candidate's rows are all this object's, its opacity is 1 to rounding and |opacity - 1| is no number for a relative bar.)"""
    case, gen = ragged_case(cnr, R, n1, n2, L, seed)
    rows, u, g = step_draws(case, gen)
    st = case.device_state(dev)
    got = launch(cnr, dev, case, st, rows=rows, u=u, g=g, reg=0.0005)
    assert got["flags"].tolist() == [0] * 5
    after = st["codes"].cpu()
    for k in range(5):
        r64 = case.oracle_step(case.oracle(k, 0.0005), k, rows[k], u[k], g[k])
        r32 = case.oracle_step(case.oracle(k, 0.0005, torch.float32), k, rows[k], u[k], g[k])
        check_step(f"R {R} S {n1 + n2} L {L} candidate {k}", got, k, r64, r32, after[k] - case.codes0[k], r64["codes"] - case.codes0[k].double())


# ---- 3. three steps ------------------------------------------------------------------------------------------------------------------
def test_three_steps_track_the_restatement(cnr, dev):
    """Parity mode with fresh rows and draws per step against a free-running fp64 oracle.  The bar is on the accumulated update
    codes_3 - codes_0 (the codes themselves barely move: a bar on them would pass a dead kernel), where the first step's gradient is
    clear of AdamW's eps, as the one-step update bar."""
    case, gen = ragged_case(cnr, 24, 1, 9, 256, 77)
    steps = [step_draws(case, gen) for _ in range(3)]
    st = case.device_state(dev)
    for rows, u, g in steps:
        got = launch(cnr, dev, case, st, rows=rows, u=u, g=g, reg=0.0005)
    assert got["flags"].tolist() == [0] * 5 and [s[1:3] for s in st["state"].cpu().tolist()] == [[3, 3]] * 5
    after = st["codes"].cpu()
    for k in range(5):
        orc = case.oracle(k, 0.0005)
        first = None
        for rows, u, g in steps:
            out = case.oracle_step(orc, k, rows[k], u[k], g[k])
            first = out["grad"] if first is None else first
        clear = first.abs() > 0.02 * first.abs().max()
        upd, ref = (after[k] - case.codes0[k]).double(), orc.codes() - case.codes0[k].double()
        e = rel_l2(upd[clear], ref[clear])
        print(f"candidate {k}: accumulated update rel_l2 {e:.2e}, |update| {float(ref.norm()):.2e}, |codes| {float(case.codes0[k].norm()):.2e}")
        assert float(ref[clear].norm()) > 0 and e < 0.02


# ---- 4. independence and sharing ---------------------------------------------------------------------------------------------------
def test_independence_and_sharing(cnr, dev):
    case, gen = ragged_case(cnr, 24, 1, 9, 256, 91)
    case.ids = [5, 11, 12]
    rows, u, g = step_draws(case, gen)
    st = case.device_state(dev)
    got = launch(cnr, dev, case, st, rows=rows, u=u, g=g, reg=0.0005)
    # candidate 3 alone (its network and pool kept in place) equals itself in the batch bit for bit
    solo = Case(case.nets, case.pools, case.world, [1], [2], case.codes0[3:4], 24, 1, 9, 256, ids=case.ids)
    st1 = solo.device_state(dev)
    got1 = launch(cnr, dev, solo, st1, rows=rows[3:4], u=u[3:4], g=g[3:4], reg=0.0005)
    for key in ("grad", "sigma", "rgb", "z"):
        assert torch.equal(got1[key][0], got[key][3]), key
    assert torch.equal(got1["losses"][:, 0], got["losses"][:, 3])
    assert all(torch.equal(st1[k][0], st[k][3]) for k in ("codes", "m", "v", "state"))
    # Philox mode: candidates 3 and 4 share pool 2 and network 1; with EQUAL codes they give equal bits ...
    twin = Case(case.nets, case.pools, case.world, [1, 1, 0], [2, 2, 2], case.codes0[[3, 3, 4]], 24, 1, 9, 256, ids=case.ids)
    st2 = twin.device_state(dev)
    got2 = launch(cnr, dev, twin, st2, seed=9, reg=0.0005)
    for key in ("grad", "sigma", "rgb", "z", "rows_out"):
        assert torch.equal(got2[key][0], got2[key][1]), key
    assert torch.equal(st2["codes"][0], st2["codes"][1]) and torch.equal(got2["losses"][:, 0], got2["losses"][:, 1])
    # ... and with different codes (and another network) still the same rows and the same draws
    assert torch.equal(got2["rows_out"][2], got2["rows_out"][0]) and torch.equal(got2["z"][2], got2["z"][0])
    assert not torch.equal(got2["sigma"][2], got2["sigma"][0])
    # the key is the pool's id, not its place: another id, other rows and draws
    twin.ids = [5, 11, 13]
    got3 = launch(cnr, dev, twin, twin.device_state(dev), seed=9, reg=0.0005)
    assert not torch.equal(got3["rows_out"][0], got2["rows_out"][0]) and not torch.equal(got3["z"][0], got2["z"][0])


# ---- 5. frozen means frozen --------------------------------------------------------------------------------------------------------
def test_frozen_means_frozen(cnr, dev):
    case, gen = ragged_case(cnr, 24, 1, 9, 256, 55)
    st = case.device_state(dev)
    theta0 = st["theta"].clone()
    for _ in range(20):
        got = launch(cnr, dev, case, st, seed=4, reg=0.0005, want=False)
    assert torch.equal(st["theta"], theta0)
    assert not torch.equal(st["codes"].cpu(), case.codes0) and torch.isfinite(st["codes"]).all() and got["flags"].tolist() == [0] * 5
    assert [s[1:3] for s in st["state"].cpu().tolist()] == [[20, 20]] * 5
    before = {k: t.clone() for k, t in st.items()}
    ev = launch(cnr, dev, case, st, seed=4, reg=0.0005, update=0)
    assert all(torch.equal(st[k], before[k]) for k in st)               # codes, moments, state (and theta) untouched
    up = launch(cnr, dev, case, st, seed=4, reg=0.0005, update=1)
    assert all(torch.equal(ev[k], up[k]) for k in ev)                   # the same losses, flags, gradient, outputs
    assert not torch.equal(st["codes"], before["codes"]) and torch.equal(st["theta"], theta0)


# ---- 6. empty masks ---------------------------------------------------------------------------------------------------------------
def test_empty_masks_zero_their_terms_for_that_candidate_only(cnr, dev):
    R, n1, n2, L = 24, 1, 9, 256
    gen = torch.Generator().manual_seed(1031)                      # (31 is not admitted: check_step)
    pools = [make_pool(cnr, 60, gen, 0) for _ in range(3)]
    pools[0]["depth"] = torch.zeros(60)                            # no valid depth: the depth count is zero
    pools[1]["rgbs"][:, 3] = 2                                     # every pixel "unknown": the opacity count is zero
    nets = [FC.init_net(torch.Generator().manual_seed(300), L, jitter_B=0.02)]
    case = Case(nets, pools, [0, 0, 0], [0, 0, 0], [0, 1, 2], FC.init_codes(gen, L, 3), R, n1, n2, L)
    rows, u, g = step_draws(case, gen)
    st = case.device_state(dev)
    got = launch(cnr, dev, case, st, rows=rows, u=u, g=g, reg=0.0)
    assert got["flags"].tolist() == [2, 8, 0]
    assert got["losses"][0, 0] == 0 and got["losses"][2, 1] == 0
    assert got["losses"][0, 1] > 0 and (got["losses"][1] > 0).all() and got["losses"][2, 0] > 0 and got["losses"][2, 2] > 0
    for t in list(got.values()) + [st["codes"].cpu(), st["m"].cpu(), st["v"].cpu()]:
        assert torch.isfinite(t.float()).all()
    after = st["codes"].cpu()
    for k in range(3):
        r64 = case.oracle_step(case.oracle(k, 0.0), k, rows[k], u[k], g[k])
        r32 = case.oracle_step(case.oracle(k, 0.0, torch.float32), k, rows[k], u[k], g[k])
        check_step(f"empty masks candidate {k}", got, k, r64, r32, after[k] - case.codes0[k], r64["codes"] - case.codes0[k].double())
    # (the oracle's gradient above is the gradient without the zeroed term: reduce_batch_loss returns zeros for it)  The regular
    # candidate keeps its bits beside the two
    solo = Case(nets, pools, [0, 0, 0], [0], [2], case.codes0[2:3], R, n1, n2, L)
    st1 = solo.device_state(dev)
    got1 = launch(cnr, dev, solo, st1, rows=rows[2:3], u=u[2:3], g=g[2:3], reg=0.0)
    assert torch.equal(st1["codes"][0], st["codes"][2]) and torch.equal(got1["grad"][0], got["grad"][2])
    assert torch.equal(got1["losses"][:, 0], got["losses"][:, 2]) and got1["flags"].tolist() == [0]


# ---- 7. rows, epochs and state on the device; argument errors ------------------------------------------------------------------------
def test_rows_epochs_and_state_in_philox_mode(cnr, dev):
    R, n1, n2, L = 24, 1, 9, 256
    gen = torch.Generator().manual_seed(41)
    lens = [2 * R + 1, 5 * R]
    pools = [make_pool(cnr, n, gen, 0) for n in lens]
    nets = [FC.init_net(torch.Generator().manual_seed(400), L)]
    case = Case(nets, pools, [0, 0], [0, 0], [0, 1], FC.init_codes(gen, L, 2), R, n1, n2, L, ids=[3, 8])
    st = case.device_state(dev)
    want, seen = [[0, 0, 0, 0], [0, 0, 0, 0]], [{}, {}]
    for k in range(8):                                             # 49 rows: two slices per epoch, four epochs; 120 rows: four slices, two
        got = launch(cnr, dev, case, st, seed=5)
        for o in range(2):
            r = got["rows_out"][o]
            assert int(r.min()) >= 0 and int(r.max()) < lens[o]
            seen[o].setdefault(want[o][3], []).append(r)
        want = [cnr.code_fit.next_state(s, n, R) for s, n in zip(want, lens)]
        assert st["state"].cpu().tolist() == want, k
    assert want == [[0, 8, 8, 4], [0, 8, 8, 2]]
    for o in range(2):
        for ep, chunks in seen[o].items():
            allr = torch.cat(chunks)
            assert len(torch.unique(allr)) == len(allr), (o, ep)   # a permutation slice: no row twice within an epoch
        assert not torch.equal(torch.cat(seen[o][0]), torch.cat(seen[o][1]))
    assert torch.isfinite(st["codes"]).all()


def test_skipped_candidates_and_argument_errors(cnr, dev):
    R, n1, n2, L = 24, 1, 9, 256
    gen = torch.Generator().manual_seed(51)
    pools = [make_pool(cnr, 60, gen, 0), make_pool(cnr, 20, gen, 0)]       # the second is shorter than R
    nets = [FC.init_net(torch.Generator().manual_seed(500), L)]
    case = Case(nets, pools, [0, 0], [0, 0, 1, 0, 0], [0, 1, 0, 2, -1], FC.init_codes(gen, L, 5), R, n1, n2, L)
    st = case.device_state(dev)
    got = launch(cnr, dev, case, st, seed=2, min_rows=R)           # (a host that checked the shortest pool wrongly)
    assert got["flags"].tolist() == [0, 16, 64, 64, 64]
    assert (got["losses"][:, 1:] == 0).all() and (got["losses"][:, 0] > 0).all()
    assert torch.equal(st["codes"][1:].cpu(), case.codes0[1:]) and not torch.equal(st["codes"][0].cpu(), case.codes0[0])
    assert st["state"].cpu().tolist() == [[24, 1, 1, 0]] + [[0, 0, 0, 0]] * 4 and float(st["m"][1:].abs().max()) == 0
    alone = Case(nets, pools[:1], [0], [0], [0], case.codes0[:1], R, n1, n2, L)
    st1 = alone.device_state(dev)
    launch(cnr, dev, alone, st1, seed=2)
    assert torch.equal(st1["codes"][0], st["codes"][0])            # pool ids default to the segment index
    # ---- argument errors are return codes, not launches
    err = cnr._C.CnrError
    ok = Case(nets, pools[:1], [0], [0], [0], case.codes0[:1], R, n1, n2, L)
    s0 = ok.device_state(dev)
    with pytest.raises(err, match="code -1"):
        launch(cnr, dev, ok, s0, n1=8, n2=57, want=False)                              # S = 65
    with pytest.raises(err, match="code -1"):
        launch(cnr, dev, ok, s0, R=61, want=False)                                     # the pool is shorter than R
    with pytest.raises(err, match="code -1"):
        launch(cnr, dev, ok, s0, min_rows=R - 1, want=False)
    with pytest.raises(err, match="code -1"):
        launch(cnr, dev, ok, s0, rows=torch.zeros(1, R, dtype=torch.int32), want=False)  # a partial parity set
    with pytest.raises(err, match="code -2"):
        launch(cnr, dev, ok, s0, L=48, theta=torch.zeros(1, cnr.fused.ParamLayout(48, 0).total, device=dev), want=False)
    lib, _C = cnr._C.load(), cnr._C
    assert int(lib.cnr_code_fit_workspace_bytes(1, R, 65)) == -1 and int(lib.cnr_code_fit_workspace_bytes(0, R, 10)) == -1
    assert int(lib.cnr_code_fit_workspace_bytes(3, R, 10)) == int(lib.cnr_obj_workspace_bytes(3, R, 10)) > 0
    lay = cnr.fused.ParamLayout(L, 0)
    p = {k: v.to(dev) for k, v in pools[0].items()}
    off = torch.tensor([0, 60], device=dev, dtype=torch.int64)
    zi = torch.zeros(1, device=dev, dtype=torch.int32)
    ws = _C.workspace(lib.cnr_code_fit_workspace_bytes(1, R, 10), dev, "cnr_code_fit")
    base = [s0["theta"], lay.total, 0, lay.latW[0], lay.latb[0], lay.B[0], 1, L, p["rgbs"], p["depth"], p["dirs"], p["T"], off, 60, None,
            zi, 1, zi, zi, 1, R, n1, n2, EPS, STOP_EPS, 0.0, SCALE, 0, None, None, None, s0["state"], s0["codes"], s0["m"], s0["v"], 1, LR,
            0.9, 0.999, 1e-8, WD, 5.0, 10.0, 0.0, torch.zeros(5, 1, device=dev), torch.zeros(1, device=dev, dtype=torch.int32), None, None,
            None, None, None, ws, ws.numel()]
    for idx, bad in ((0, None), (17, None), (32, None), (19, 0), (20, 0), (6, 0), (16, 0), (52, 64), (1, lay.total - 1), (3, lay.latb[0]),
                     (5, lay.total - 62), (2, lay.total - 100)):
        args = list(base)
        args[idx] = bad            # theta, cand_net, codes NULL; K, R, n_nets, P = 0; a short workspace; a row that ends before B
                                   # does, latent matrices, B or a trunk that would run past the row
        with pytest.raises(err, match="code -1"):
            _C.call("cnr_code_fit", *args)
    torch.cuda.synchronize()
    assert s0["state"].cpu().tolist() == [[0, 0, 0, 0]] and torch.equal(s0["codes"].cpu(), case.codes0[:1])      # nothing was launched


# ---- 8. the fitter ---------------------------------------------------------------------------------------------------------------
def fitter_case(cnr, device, seed=3, shipped=False):
    """A seeded random-initialised frozen category of three trained objects and two new instances whose pools have exactly R = 24
    rows, so every step is the full batch.  (synthetic_pool's colours are independent noise per ray, which no code can fit: one
    colour per instance instead.)

    The samples hug the surface (surface_eps = stop_eps = 1e-4, no free-space bin), so that the objective is a smooth function of
    the codes and hardly depends on the draws.  With the shipped 0.1 and a free-space bin, a RANDOM network -- whose x10 logits
    saturate -- makes the variance-weighted depth term heavy-tailed: a ray that terminates on one sample has variance ~0 and a
    weight of 1e4, and the term moves between 7 and 192 from one set of draws to the next (codefit_cpu, fp64).  No single
    fixed-draw score shows a descent through that; a trained network does not have the problem, a test has to avoid it."""
    cfg = cnr.cfg.synthetic_config(device=str(device), latent_dim=32, n_bins_cam2surface=1 if shipped else 0, n_bins=9 if shipped else 10)
    if not shipped:
        cfg.surface_eps = cfg.stop_eps = 1e-4
    cfg.code_learning_rate, cfg.code_weight_decay = 0.03, 0.013
    tcfg = cnr.cfg.synthetic_config(device="cpu", latent_dim=32)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1234)
        trainer = cnr.trainer.Trainer(tcfg, 3, [0, 1, 2])
    gen = torch.Generator().manual_seed(61)
    instances = []
    for k, inst_id in enumerate((40, 41)):
        p = make_pool(cnr, 24, gen, 0)
        p["rgbs"][:, :3] = torch.tensor([[200, 60, 30], [20, 180, 90]], dtype=torch.uint8)[k]
        instances.append(dict(inst_id=inst_id, cls_id=3, pool=p))
    return cfg, trainer, instances, dict(starts=["mean", ("random", 2)], rays_per_step=24, seed=seed)


def _to(trainer, dev):
    trainer.device = str(dev)
    trainer.fc_occ_map.to(dev), trainer.pe.to(dev)
    trainer.shape_codes.to(dev), trainer.texture_codes.to(dev)
    return trainer


def test_code_fitter_learns_replays_and_attaches(cnr, dev):
    """150 steps at code lr 0.03.  The same case through codefit_cpu in fp64 on the CPU (torch draws, three different seeds)
    takes the six candidates' scores from 11.4 .. 23.1 down to 2.3 .. 8.3: every candidate ends between 0.11 and 0.57 of where
    it started, the same to two digits for every seed of the draws.  That is the margin; the condition here is only "lower"."""
    cfg, trainer, instances, kw = fitter_case(cnr, dev)
    _to(trainer, dev)
    before_modules = [p.detach().clone() for p in trainer.fc_occ_map.parameters()]
    fit = cnr.code_fit.CodeFitter(cfg, {3: trainer}, instances, **kw)
    eager = cnr.code_fit.CodeFitter(cfg, {3: trainer}, instances, **kw)
    assert fit.K == 6 and fit.slices == {40: (0, 3), 41: (3, 6)} and torch.equal(fit._codes, eager._codes)
    mean = torch.stack([trainer.shape_codes.weight.data.mean(0), trainer.texture_codes.weight.data.mean(0)])
    assert torch.allclose(fit.codes(40, 0), mean) and torch.equal(fit.codes(40, 0), fit.codes(41, 0))
    assert not torch.equal(fit.codes(40, 1), fit.codes(41, 1))                     # random starts are seeded by (seed, inst_id)
    s0 = fit.score()
    assert torch.equal(s0, fit.score()) and fit.state() == [[0, 0, 0, 0]] * 6      # scoring moves nothing
    fit.step()
    fit.run(11)                                                    # eager warm-up, then graphs of up to 8 steps
    for _ in range(12):
        eager.step(use_graph=False)
    assert fit.steps_done == eager.steps_done == 12 and fit._sched.graphs
    assert torch.equal(fit._codes, eager._codes) and torch.equal(fit.exp_avg_sq, eager.exp_avg_sq)
    assert torch.equal(fit.d_state, eager.d_state) and torch.equal(fit.losses, eager.losses)
    fit.run(138)
    s1 = fit.score()
    print("scores before", s0.tolist(), "after 150 steps", s1.tolist())
    assert torch.isfinite(fit._codes).all() and fit.flags.cpu().tolist() == [0] * 6
    assert (s1 < s0).all()
    assert fit.state() == [[0, 150, 150, 150]] * 6                 # exactly R rows: every step an epoch
    for p, q in zip(trainer.fc_occ_map.parameters(), before_modules):
        assert torch.equal(p, q)                                   # the modules are never written
    k, sh, tx = fit.best(41)
    assert k == int(torch.argmin(s1[3:6])) and torch.equal(sh, fit.codes(41, k)[0]) and torch.equal(tx, fit.codes(41, k)[1])
    # attach: eval_points of the new instance equals eval_points of a trainer whose table row was set by hand to the same codes
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1234)
        hand = _to(cnr.trainer.Trainer(cnr.cfg.synthetic_config(device="cpu", latent_dim=32), 3, [0, 1, 2]), dev)
    with torch.no_grad():
        hand.shape_codes.weight[1].copy_(sh)
        hand.texture_codes.weight[1].copy_(tx)
    assert fit.attach(trainer, 41, extent=[1.0, 0.8, 1.2]) == k
    assert trainer.n_obj == 4 and trainer.inst_id_to_index[41] == 3 and torch.equal(trainer.shape_codes.weight.data[3], sh)
    pts = (torch.rand(500, 3, generator=torch.Generator().manual_seed(2)) * 2 - 1).to(dev)
    a, b = trainer.eval_points(pts, inst_id=41), hand.eval_points(pts, inst_id=1)
    assert a is not None and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError, match="already"):
        fit.attach(trainer, 41)
    mesh = trainer.meshing(41, grid_dim=16)                        # a mesh or None, never an exception
    assert mesh is None or len(mesh.vertices) > 0


def test_code_fitter_runs_at_the_shipped_sampling(cnr, dev):
    """The case of the test above with the shipped surface_eps / stop_eps and a free-space bin, through the Philox sampler and the
    graphs: no descent is asked of a fixed-draw score here (fitter_case says why), only a run that stays finite and unflagged."""
    cfg, trainer, instances, kw = fitter_case(cnr, dev, shipped=True)
    assert (cfg.surface_eps, cfg.stop_eps, cfg.n_bins_cam2surface) == (0.1, 0.05, 1)
    fit = cnr.code_fit.CodeFitter(cfg, {3: _to(trainer, dev)}, instances, **kw)
    start = fit._codes.clone()
    fit.run(20)
    assert fit.steps_done == 20 and fit._sched.graphs and fit.state() == [[0, 20, 20, 20]] * 6
    assert torch.isfinite(fit._codes).all() and torch.isfinite(fit.losses).all() and not torch.equal(fit._codes, start)
    assert fit.flags.cpu().tolist() == [0] * 6 and torch.isfinite(fit.score()).all()


# ---- 9. pools from a dataset ---------------------------------------------------------------------------------------------------------
def test_pools_from_dataset_on_restricted_frames(cnr, dev, tmp_path):
    from dataset_synth import write_registration_pickle
    from test_dataset_host import _frames
    from cnr_amd.scene_cateogries import cameraInfo
    root = str(tmp_path / "replica")
    shutil.copytree(os.path.join(DS, "replica"), root)
    write_registration_pickle(root, _frames("replica"))
    with open(os.path.join(DS, "replica.json")) as f:
        c = json.load(f)
    c["dataset"]["path"] = root
    c["camera"].update(w=72, h=48, fx=60.0, fy=60.0, cx=35.5, cy=23.5)
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps(c))
    cfg = cnr.cfg.Config(str(p))
    cfg.data_device = cfg.training_device = str(dev)
    ds = cnr.dataset.get_dataset(cfg)
    entries = {int(i): (cls, e) for cls, d in ds.inst_dict.items() if cls != 0 for i, e in d.items()}
    ids = sorted(entries)[:2]
    keys = {int(k): k for cls, d in ds.inst_dict.items() if cls != 0 for k in d}          # (the dataset's own keys: numpy int32)
    poses = {keys[i]: np.asarray(entries[i][1]["T_obj"]) for i in ids}
    all_frames = sorted({fi["frame"] for i in ids for fi in entries[i][1]["frame_info"]})
    frames = all_frames[:max(1, len(all_frames) // 2)]             # the partially observed case
    pools = cnr.code_fit.CodeFitter.pools_from_dataset(ds, cfg, poses, frames=frames)
    full = cnr.code_fit.CodeFitter.pools_from_dataset(ds, cfg, poses)
    rays = cameraInfo(cfg, device="cpu").rays_dir_cache
    assert list(pools.keys()) == [keys[i] for i in ids]
    for i in ids:
        got, info = {k: v.cpu() for k, v in pools[keys[i]].items()}, entries[i][1]
        rgbs, depth, dirs, T = [], [], [], []
        for fi in info["frame_info"]:
            if fi["frame"] not in frames:
                continue
            w0, w1, h0, h1 = (int(v) for v in fi["bbox"])
            s = ds.sample_dict[fi["frame"]]
            img, dep, msk = (torch.as_tensor(np.asarray(s[k])) for k in ("image", "depth", "obj_mask"))
            m = msk[w0:w1, h0:h1].reshape(-1)
            state = torch.where(m == i, 1, torch.where(m == -1, 2, 0)).to(torch.uint8)       # this / unknown / other
            rgbs.append(torch.cat([img[w0:w1, h0:h1].reshape(-1, 3), state[:, None]], 1))
            depth.append(dep[w0:w1, h0:h1].reshape(-1).float())
            dirs.append(rays[w0:w1, h0:h1].reshape(-1, 3))
            T_co = torch.linalg.inv(torch.as_tensor(np.asarray(s["T"]), dtype=torch.float32)) @ torch.as_tensor(poses[keys[i]], dtype=torch.float32)
            T.append(T_co[None].expand(len(m), 4, 4))
        n = sum(len(d) for d in depth)
        assert 0 < n == got["depth"].shape[0] <= full[keys[i]]["depth"].shape[0]
        assert torch.equal(got["rgbs"], torch.cat(rgbs)) and torch.equal(got["depth"], torch.cat(depth))
        assert torch.equal(got["dirs"], torch.cat(dirs))
        assert torch.allclose(got["T"], torch.cat(T), rtol=1e-5, atol=1e-6)
    assert sum(p["depth"].shape[0] for p in pools.values()) < sum(p["depth"].shape[0] for p in full.values())
    with pytest.raises(ValueError, match="no instance"):
        cnr.code_fit.CodeFitter.pools_from_dataset(ds, cfg, {99991: np.eye(4)})
