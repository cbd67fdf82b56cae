"""GPU: the sharded train step through the HIP kernels against a single-GPU step on the whole batch.

* in one process: N trainer objects play the ranks of a ray-sharded / class-sharded world (the gradient sum and the OR
  of the empty flags done by hand), compared step by step with ONE trainer on the whole batch: identical samples
  (Philox indexed by the global ray), gradients to fp32 summation order, parameters after AdamW;
* in two processes over a gloo group (both on this box's one GPU; on a node the launcher gives each rank its own GPU and
  the backend is RCCL): the product path, hipGraph replay and epoch reshuffles included, against the single-process run.
"""
import os
import socket
import subprocess
import sys

import pytest
import torch

import record_noise as rn
from conftest import ROOT, rel_l2
from mp_fused_worker import build

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cnr(dev):
    import cnr_amd
    return cnr_amd


@pytest.mark.parametrize("world", [2, 4])
def test_ray_shards_add_up_to_the_single_gpu_step(cnr, dev, world):
    """N trainers as the ranks of a ray-sharded world against ONE trainer on the whole batch, step by step.  The whole-gradient bar
    (4e-3 since the records are bf16) is the coarse backstop; the tight checks hold the difference to what the records of all
    N + 1 launches predict for their own rounding (tests/record_noise.py): exact channel (no record behind it) < 2e-5, the bar of
    the fp32 records; chi2(trunk) <= 1.25; |delta| <= 2e-5 + 4 sd; and per rank, projected on that rank's OWN share g_r of the
    gradient -- the direction of a rank-local normalisation error --, |delta_r| <= 2e-5 |g| / |g_r| + 4 sd_r.  The shards split the
    rays differently from the single trainer, so the launches round independently and chi2 sits at the null's 1.
    Measured on MI355X ("[noise]" lines; trunk chi2 | delta | sd | rho | trunk entries out of chi2 | exact channel | chi2 of B |
    delta_r / sd_r per rank):
      world 2 step 0 nwg 32/32       0.918  +2.02e-05 2.38e-05 8.38e-04 0.014  2.91e-08  0.917  -0.5 +0.6
      world 2 step 1 nwg 32/32       0.950  +1.18e-05 2.47e-05 7.77e-04 0.013  3.28e-08  1.051  -0.7 +1.2
      world 2 step 2 nwg 32/32       0.952  +3.96e-06 2.86e-05 7.04e-04 0.013  2.88e-08  0.772  -2.1 -0.5
      world 2 step 3 nwg 32/32       0.964  -8.10e-05 5.68e-05 1.24e-03 0.012  3.03e-08  0.803  -1.5 +0.1
      world 2 step 4 nwg 32/32       0.944  -2.51e-05 5.41e-05 1.18e-03 0.013  3.10e-08  0.787  -1.8 +0.9
      world 2 step 5 nwg 32/32       0.950  -5.36e-05 4.65e-05 9.42e-04 0.012  3.05e-08  1.170  -0.4 -0.6
      world 2 step 6 nwg 32/32       0.945  -1.07e-06 4.06e-05 8.89e-04 0.013  2.60e-08  1.057  -1.0 -0.6
      world 4 step 0 nwg 32/32       0.939  +4.55e-05 2.33e-05 8.27e-04 0.014  3.38e-08  1.039  -1.4 -0.8 +0.3 +1.3
      world 4 step 1 nwg 32/32       0.967  +1.20e-05 2.36e-05 7.68e-04 0.013  3.79e-08  1.050  -0.7 -0.3 -0.1 +0.8
      world 4 step 2 nwg 32/32       0.968  +5.02e-05 2.79e-05 6.94e-04 0.013  3.08e-08  1.028  +0.9 +0.7 +0.6 +1.3
      world 4 step 3 nwg 32/32       0.968  -8.68e-05 5.66e-05 1.23e-03 0.012  3.72e-08  0.744  +0.7 -0.7 -1.0 -0.5
      world 4 step 4 nwg 32/32       0.967  -5.81e-05 5.21e-05 1.16e-03 0.013  3.44e-08  0.923  -1.1 -0.9 -0.5 +1.8
      world 4 step 5 nwg 32/32       0.954  -6.27e-07 4.60e-05 9.34e-04 0.012  3.14e-08  0.991  -2.3 +1.3 -0.1 +0.9
      world 4 step 6 nwg 32/32       0.974  -2.31e-05 4.00e-05 8.80e-04 0.013  2.91e-08  1.020  +1.5 -0.9 +0.5 -1.1
    sd_r is 1.5e-4 .. 4.8e-4 (|g| / |g_r| = 1.5 .. 4.4): a rank that divided by its local count is off by 1 - 1/N >= 0.5 along
    g_r, a thousand times that bound; the whole-trunk projection resolves 1.1e-4 .. 2.5e-4."""
    C, Rg, n_obj, L = 2, 512, 4, 32
    one = build(cnr, dev, "ray", 0, 1, None, C, Rg, n_obj, L, False)
    ranks = [build(cnr, dev, "ray", r, world, None, C, Rg, n_obj, L, False) for r in range(world)]
    R = Rg // world
    E = rn.record_entries(cnr._C)
    for r, tr in enumerate(ranks):
        assert tr.grad_exchange and not tr.fused_tail and tr.R == R and tr.Rg == Rg
        assert torch.equal(tr.perm, one.perm) and torch.equal(tr.theta, one.theta)
    for step in range(7):                                   # pool of six slices: an epoch reshuffle on the way
        # every step starts from the single-GPU run's state: AdamW's first steps move each parameter by ~lr * sign(g), so
        # summation-order noise in a near-zero gradient entry becomes a 2 lr parameter difference that would compound
        for tr in ranks:
            tr.theta2.copy_(one.theta2); tr.exp_avg.copy_(one.exp_avg); tr.exp_avg_sq.copy_(one.exp_avg_sq)
        one.step()
        for tr in ranks:
            tr._pre_step()
            tr._step_front()
        g = sum(tr.grad for tr in ranks)                    # what the all-reduce leaves on every rank
        own = [tr.grad.double().cpu() for tr in ranks]      # each rank's own share, before the sum overwrites it
        for tr in ranks:
            tr.grad.copy_(g)
            tr._step_back()
            tr._post_step()
        torch.cuda.synchronize()
        for r, tr in enumerate(ranks):                      # same rays, same samples
            sl = slice(r * R, (r + 1) * R)
            for k in ("z", "pts", "gt_rgb", "gt_depth", "labels", "depth_mask", "ray_row"):
                assert torch.equal(tr.bufs[k], one.bufs[k][:, sl]), (step, r, k)
        # same parameters, same samples: the two gradients differ by fp32 summation order and -- since round 4 -- by the bf16
        # rounding of the per-workgroup records, independent in every launch (2^-9 per entry over these shapes' 8 .. 32 records:
        # measured 1.3e-3; 2e-5 with fp32 records).  Rank-local normalisation, the error this test exists for, is a 1 - 1/N effect.
        # 4e-3 is the coarse backstop; the checks below hold the difference to the noise these very records predict.
        assert rel_l2(g, one.grad) < 4e-3, (step, rel_l2(g, one.grad))
        # ---- the tight checks (tests/record_noise.py): every launch's records are still in its workspace
        lay = one.lay
        v = sum(rn.step_variance(tr.bufs["bwd_ws"], C, tr._nwg, E, n_obj, lay) for tr in [one] + ranks)
        g1 = one.grad.double().cpu()
        d = g.double().cpu() - g1
        sums = [rn.step_record_sum(tr.bufs["bwd_ws"], C, tr._nwg, E, n_obj, lay) for tr in [one] + ranks]
        d_rec, d_exact = rn.split_difference(d, sums[1:], sums[:1])
        rep = rn.noise_report(d, g1, v, rn.gradient_groups(lay, cnr.ops.TRUNK_LAYERS), d_records=d_rec)
        tag = f"ray_shards world {world} step {step} nwg {one._nwg}/{ranks[0]._nwg}"
        print(rn.format_report(tag, {k: rep[k] for k in ("trunk", "B")}))
        gn, t = float(g1.norm()), rep["trunk"]
        exact = float(d_exact.norm()) / gn
        per_rank = [rn.noise_report(d, gr, v, {"all": slice(None)})["all"] for gr in own]
        print(f"[noise] {tag} exact channel {exact:.2e}; trunk entries out of chi2 {t['left_out']:.3f}; per rank delta / sd / |g| / |g_r|: "
              + " ".join(f"{r['delta']:+.2e} / {r['sd']:.2e} / {gn / r['g2'] ** 0.5:.2f}" for r in per_rank))
        assert exact < 2e-5, (step, exact)                   # no record behind these entries: the bar of the fp32 records
        assert t["left_out"] <= 0.25, t
        assert t["chi2"] <= 1.25, (step, t)
        assert abs(t["delta"]) <= 2e-5 + 4 * t["sd"], (step, t)
        # a rank that normalised by its LOCAL count is off by a factor, along its own share of the gradient
        for r_, r in enumerate(per_rank):
            assert abs(r["delta"]) <= 2e-5 * gn / r["g2"] ** 0.5 + 4 * r["sd"], (step, r_, r)
        assert rel_l2(sum(tr.losses for tr in ranks), one.losses) < 1e-5
        for tr in ranks:
            assert torch.equal(tr.theta, ranks[0].theta)    # replicas bitwise identical
        assert rel_l2(ranks[0].theta, one.theta) < 1e-3, (step, rel_l2(ranks[0].theta, one.theta))
        assert int(ranks[1].d_state[0]) == int(one.d_state[0]) + R


def test_sixteen_classes_on_two_ranks(cnr, dev):
    """BASELINE.json configs[2] ("all categories": 16 classes x 4 objects, the survey's stand-in) split 8 + 8 over two class
    shards: same bits as the single-GPU run of all sixteen."""
    C, R, n_obj, L, world = 16, 128, 4, 32, 2
    one = build(cnr, dev, "class", 0, 1, None, C, R, n_obj, L, False)
    ranks = [build(cnr, dev, "class", r, world, None, C, R, n_obj, L, False) for r in range(world)]
    flags = torch.stack([tr.counts_tab[:, tr.C, :3] for tr in ranks]).amax(0)
    for tr in ranks:
        tr.counts_tab[:, tr.C, :3] = flags
    for _ in range(3):
        one.step()
        for tr in ranks:
            tr.step()
    torch.cuda.synchronize()
    for tr in ranks:
        assert tr.C == 8 and torch.equal(tr.theta, one.theta[tr.class_ids]) and torch.equal(tr.losses, one.losses[:, tr.class_ids])


@pytest.mark.parametrize("empty_class", [None, 2])
def test_class_shards_equal_the_single_gpu_step_bitwise(cnr, dev, empty_class):
    """Classes share nothing but the any-class-empty rule: rank r trains classes r, r + 2 with NO gradient exchange and
    ends with the very bits the single-GPU run of all four classes has -- also when one class's masks are empty, which
    zeroes the depth and colour terms of every class on every rank (src/render_rays.py:67-72)."""
    C, R, n_obj, L, world = 4, 256, 4, 32, 2
    one = build(cnr, dev, "class", 0, 1, None, C, R, n_obj, L, False, empty_class)
    ranks = [build(cnr, dev, "class", r, world, None, C, R, n_obj, L, False, empty_class) for r in range(world)]
    # the flags' OR over ranks (the trainers have no process group here; with one, _reshuffle does this)
    flags = torch.stack([tr.counts_tab[:, tr.C, :3] for tr in ranks]).amax(0)
    for tr in ranks:
        tr.counts_tab[:, tr.C, :3] = flags
        assert tr.fused_tail and not tr.grad_exchange
    assert torch.equal(flags, one.counts_tab[:, C, :3])
    if empty_class is not None:
        assert float(flags[:, :2].min()) == 1.0 and float(flags[:, 2].max()) == 0.0
    for step in range(4):                                   # within the first epoch
        one.step()
        for tr in ranks:
            tr.step()
    torch.cuda.synchronize()
    for tr in ranks:
        ids = tr.class_ids
        assert torch.equal(tr.theta, one.theta[ids]) and torch.equal(tr.losses, one.losses[:, ids])
        if empty_class is not None:
            assert float(tr.losses[:2].abs().sum()) == 0.0 and bool(((tr.flags & 6) == 6).all())


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


@pytest.mark.parametrize("mode,empty", [("ray", None), ("class", None), ("class", 1)])
def test_two_processes_match_the_single_process_run(cnr, dev, tmp_path, mode, empty):
    steps, world = 9, 2                                     # six slices per epoch: the reshuffle + its tables are crossed
    out = str(tmp_path / "res")
    port = _free_port()
    procs = []
    for rank in range(world):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank),
                   WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mp_fused_worker.py"), mode, out,
                                       str(steps), "-" if empty is None else str(empty)], env=env))
    for p in procs:
        assert p.wait(timeout=600) == 0
    one = build(cnr, dev, mode, 0, 1, None, 4, 256, 4, 32, True, empty)
    hist = []
    for _ in range(steps):
        one.step()
        hist.append(one.losses.cpu().clone())
    torch.cuda.synchronize()
    hist = torch.stack(hist)
    res = [torch.load(f"{out}.{r}") for r in range(world)]
    if mode == "ray":
        assert all(r["in_sync"] for r in res)
        assert torch.equal(res[0]["theta"], res[1]["theta"])
        # nine steps apart from the summation order of one all-reduce per step (AdamW's sign-like first steps amplify it)
        assert rel_l2(res[0]["theta"], one.theta) < 1e-3 and rel_l2(res[0]["hist"], hist) < 2e-3
    else:
        for r in res:
            assert torch.equal(r["theta"], one.theta.cpu()[r["ids"]]) and torch.equal(r["hist"], hist[:, :, r["ids"]])
