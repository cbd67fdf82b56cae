"""SHA-256 of what the trainers leave after a few epochs, for comparing two checkouts on one GPU (a refactor of the host side of
the step must leave every line as it is): `python tools/pool_hashes.py > hashes.txt` in each, then diff.  Per configuration: the
permutation after every reshuffle, the parameters, AdamW's first moment, the last step's loss terms and the device step state.
Small shapes, chosen to reach every branch of the pool code: equal pools, ragged pools with a world-frame class, ray shards (both
ranks emulated in one process), the background step in both tiers, and the whole iteration."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import cnr_amd

dev = torch.device("cuda:0")
R = 64


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


alive = []       # every trainer built here lives to the end: a captured graph must not be destroyed while another is being captured


def watch(trainer, name):
    """print the permutation after every reshuffle of ``trainer`` (the constructor's has happened: printed here)"""
    alive.append(trainer)
    count = [0]

    def show():
        print(sha(trainer.perm), "%s perm after reshuffle %d" % (name, count[0]))
        count[0] += 1
    show()
    inner = trainer._reshuffle

    def reshuffle():
        inner()
        show()
    trainer._reshuffle = reshuffle


def show_categories(tr, name):
    torch.cuda.synchronize()
    for key, t in (("theta", tr.theta), ("exp_avg", tr.exp_avg), ("losses", tr.losses), ("d_state", tr.d_state)):
        print(sha(t), name, key)


def show_background(bg, name):
    torch.cuda.synchronize()
    for key, t in (("flat", bg.flat), ("exp_avg", bg.exp_avg), ("losses", bg.losses), ("d_state", bg.d_state)):
        print(sha(t), name, key)


def config(n_bins_cam2surface=2, n_bins=8):
    cfg = cnr_amd.cfg.synthetic_config(device=str(dev), latent_dim=32, n_bins_cam2surface=n_bins_cam2surface, n_bins=n_bins)
    cfg.hidden_feature_size_bg, cfg.n_bins_cam2surface_bg = 128, 6              # background: S = 6 + 8 = 14
    return cfg


def equal_categories(name, rows=5 * R, rays=R, **kw):
    """(a): two classes of four objects, equal pools, S = 10"""
    gen = torch.Generator().manual_seed(21)
    pools = [cnr_amd.scene_cateogries.synthetic_pool(rows, 4, gen, "cpu") for _ in range(2)]
    tr = cnr_amd.fused.FusedCategoryTrainer(config(), 2, 4, pools, rays, dev, seed=1, generator=gen, **kw)
    watch(tr, name)
    return tr


def background(name, precision, rays, rows):
    torch.manual_seed(31)                                                        # module initialisation
    pool = cnr_amd.scene_cateogries.synthetic_pool(rows, 1, torch.Generator().manual_seed(12), "cpu")
    bg = cnr_amd.background.BackgroundStep(config(), pool, rays, dev, seed=5, precision=precision)
    watch(bg, name)
    return bg


# ---- a. equal pools: step() x 12 and run(12) ---------------------------------------------------------------------------------
tr = equal_categories("a/step")
for _ in range(12):
    tr.step()
show_categories(tr, "a/step")
tr = equal_categories("a/run")
tr.run(12)
show_categories(tr, "a/run")

# ---- b. ragged pools, object counts (4, 1 in the world frame, 7), 16 steps -----------------------------------------------------
gen = torch.Generator().manual_seed(22)
counts = (4, 1, 7)
pools = [cnr_amd.scene_cateogries.synthetic_pool(n, k, gen, "cpu") for n, k in zip((5 * R + 3, 3 * R, 7 * R + 1), counts)]
tr = cnr_amd.fused.FusedCategoryTrainer(config(), 3, list(counts), pools, R, dev, seed=2, generator=gen)
assert tr.ragged and tr.world_frame == [False, True, False]
watch(tr, "b/ragged")
tr.run(16)
show_categories(tr, "b/ragged")

# ---- c. ray shards, both ranks of dp_world = 2 in one process (the all-reduce done by hand), 8 steps ----------------------------
Rg = 2 * R
ranks = []
for r in range(2):
    gen = torch.Generator().manual_seed(23)
    pools = [cnr_amd.scene_cateogries.synthetic_pool(6 * Rg, 4, gen, "cpu") for _ in range(2)]
    ranks.append(cnr_amd.fused.FusedCategoryTrainer(config(), 2, 4, pools, R, dev, seed=3, generator=gen, shard="ray",
                                                    dp_rank=r, dp_world=2, use_graph=False))
    watch(ranks[r], "c/rank%d" % r)
for _ in range(8):
    for tr in ranks:
        tr._pre_step()
        tr._step_front()
    g = sum(tr.grad for tr in ranks)
    for tr in ranks:
        tr.grad.copy_(g)
        tr._step_back()
        tr._post_step()
for r, tr in enumerate(ranks):
    show_categories(tr, "c/rank%d" % r)
    print(sha(tr.slice_max), "c/rank%d slice_max" % r)
    print(sha(tr.counts_tab), "c/rank%d counts_tab" % r)

# ---- d. the background step: fused tier (hidden 128, S = 14, 12 steps) and exact fp32 tier (R = 32, 6 steps) --------------------
bg = background("d/fused", "fused", R, 5 * R)
for _ in range(12):
    bg.step()
show_background(bg, "d/fused")
bg = background("d/fp32", "fp32", 32, 5 * 32)
for _ in range(6):
    bg.step()
show_background(bg, "d/fp32")

# ---- e. the whole iteration over (a) and (d), two concurrent chains, run(12, unroll=4) ------------------------------------------
full = cnr_amd.background.FullStepTrainer(equal_categories("e/categories"), background("e/background", "fused", R, 5 * R),
                                          concurrent=True)
full.run(12, unroll=4)
show_categories(full.obj, "e/categories")
show_background(full.bg, "e/background")
