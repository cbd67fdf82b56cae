"""SHA-256 of every output of the kernels that composite a ray and form its loss terms, for comparing two checkouts (or two
libraries: CNR_HIP_LIB) on one GPU -- a refactor of csrc/render_common.h and its callers must leave every line as it is:
`python tools/render_hashes.py > hashes.txt` on each side, then diff.

Covered: cnr_composite_fwd / cnr_composite_bwd (every chunk count, both input kinds, every regime, the optional outputs and
upstream sets of tests/modular_cases.py), cnr_loss_fwd_bwd (ordinary, the three empty masks, explode), cnr_render_loss +
cnr_render_loss_finish (the shapes of test_render_loss_single_launch_equals_three_calls, and the counts_tab / d_state path),
cnr_field_fwd_render (every S, with and without packed_lo, an empty mask), and two steps each of the background step (fused
tier), ObjectFieldTrainer, CodeFitter and FusedCategoryTrainer in its two-launch forms at tools/pool_hashes.py's small shapes."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
import cnr_amd
import modular_cases as M

dev = torch.device("cuda:0")
_C = cnr_amd._C


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def show(name, **tensors):
    torch.cuda.synchronize()
    for k, t in tensors.items():
        print(sha(t), name, k)


def run_case(case, name):
    """one launch of a modular_cases case on device copies of its arguments; every output buffer is printed"""
    entry, args = case
    dargs = [a.to(dev, copy=True) if torch.is_tensor(a) else a for a in args]
    _C.call(entry, *dargs)
    show(name, **M.outputs_of(entry, dargs))


# ---- cnr_composite_fwd / cnr_composite_bwd -----------------------------------------------------------------------------------
for S in M.COMPOSITE_BWD_S:
    for NR in (1, 5):
        for occ in (0, 1):
            for regime in M.REGIMES:
                tag = "S%d NR%d occ%d %s" % (S, NR, occ, regime)
                run_case(M.composite_fwd_case(NR, S, occ, regime), "composite_fwd " + tag)
                run_case(M.composite_bwd_case(NR, S, occ, regime), "composite_bwd " + tag)
for S in (1, 65, 200):
    for occ in (0, 1):
        for outputs in ("term", "no_term"):
            run_case(M.composite_fwd_case(3, S, occ, "ordinary", outputs), "composite_fwd S%d occ%d outputs %s" % (S, occ, outputs))
for S in M.COMPOSITE_BWD_S:
    for occ in (0, 1):
        for regime in M.REGIMES:
            for upstream in M.UPSTREAMS[1:]:
                run_case(M.composite_bwd_case(3, S, occ, regime, upstream),
                         "composite_bwd S%d occ%d %s upstream %s" % (S, occ, regime, upstream))

# ---- cnr_loss_fwd_bwd --------------------------------------------------------------------------------------------------------
for C in (1, 3):
    for R in (1, 257):
        for sc in M.LOSS_SCALINGS:
            run_case(M.loss_case(C, R, sc), "loss C%d R%d scalings %s" % (C, R, sc[0]))
for variant in ("empty_depth", "empty_object", "empty_surface"):
    run_case(M.loss_case(3, 300, M.LOSS_SCALINGS[0], variant), "loss " + variant)
for C, R in ((1, 1), (3, 257)):
    run_case(M.loss_case(C, R, M.LOSS_SCALINGS[0], "explode"), "loss explode C%d R%d" % (C, R))


# ---- cnr_render_loss + cnr_render_loss_finish ----------------------------------------------------------------------------------
def render_inputs(C, R, S, empty, seed):
    gen = torch.Generator().manual_seed(seed)
    sig, col = (torch.randn(C, R, S, generator=gen) * 3).to(dev), torch.rand(C, R, S, 3, generator=gen).to(dev)
    z = (torch.rand(C, R, S, generator=gen).sort(dim=-1).values * 4 + 0.1).to(dev)
    gt_d, gt_c = (torch.rand(C, R, generator=gen) * 4).to(dev), torch.rand(C, R, 3, generator=gen).to(dev)
    labels = torch.randint(0, 3, (C, R), generator=gen).to(torch.uint8).to(dev)
    dmask = (torch.rand(C, R, generator=gen) > 0.2).to(torch.uint8).to(dev)
    if empty:
        labels[1] = 0
    return gen, sig, col, z, gt_d, gt_c, labels, dmask


def render_loss(name, C, R, S, empty, counts_tab=None, d_state=None):
    _, sig, col, z, gt_d, gt_c, labels, dmask = render_inputs(C, R, S, empty, C * 1000 + R + S)
    f = lambda *s: torch.full(s, float("nan"), device=dev)
    ws = torch.zeros(_C.render_loss_workspace_bytes(C, R), device=dev, dtype=torch.uint8)
    losses, flags = f(3, C), torch.full((C,), -1, device=dev, dtype=torch.int32)
    o = dict(d_sigma=f(C, R, S), d_color=f(C, R, S, 3), depth=f(C, R), var=f(C, R), rgb=f(C, R, 3), opacity=f(C, R))
    _C.call("cnr_render_loss", sig, col, z, gt_d, gt_c, labels, dmask, 5.0, 10.0, 0.5, o["d_sigma"], o["d_color"], o["depth"],
            o["var"], o["rgb"], o["opacity"], C, R, S, ws, ws.numel(), counts_tab, d_state)
    _C.call("cnr_render_loss_finish", ws, losses, flags, C, R, 0)
    show(name, losses=losses, flags=flags, **o)


for C, R, S, empty in [(1, 2048, 64, False), (2, 300, 16, False), (3, 130, 200, False), (2, 257, 64, True), (1, 9, 65, False),
                       (2, 5, 129, False), (1, 5, 512, False), (1, 3, 1, False), (1, 4, 63, False), (2, 3, 128, False),
                       (2, 2, 448, True)]:
    render_loss("render_loss C%d R%d S%d empty%d" % (C, R, S, empty), C, R, S, empty)
# the per-epoch table: (slices, C + 1, 4) = the three counts of every class, then the three any-class-empty flags; slice 1 is read
for S in (40, 150):
    C, R = 2, 70
    tab = torch.zeros(2, C + 1, 4)
    tab[0, :C, :3] = 1.0
    tab[1, :C, :3] = torch.tensor([[31.0, 40.0, 52.0], [17.0, 44.0, 47.0]])
    tab[1, C, 2] = 1.0 if S == 150 else 0.0
    render_loss("render_loss counts_tab S%d" % S, C, R, S, False, tab.to(dev), torch.tensor([R, 0, 0], device=dev, dtype=torch.int64))

# ---- cnr_field_fwd_render ----------------------------------------------------------------------------------------------------
for S, empty in [(S, e) for S in (32, 64, 96, 128) for e in (True, False)]:
    # (an empty mask in one class zeroes the depth and colour gradients of EVERY class: the rows without one carry all five)
    C, R, n_obj = 2, 9, 4
    gen, _, _, z, gt_d, gt_c, labels, dmask = render_inputs(C, R, S, empty, 500 + S)
    theta, lay = cnr_amd.fused.init_params(C, 32, n_obj, gen, dev)
    v = lay.views(theta)
    trunk, B = v["trunk"].contiguous(), v["B"].contiguous()
    packed = cnr_amd.ops.pack_weights(trunk)
    brows = (torch.randn(C * n_obj, 4, 32, generator=gen) * 0.1).to(dev)
    ray_row = (torch.randint(0, n_obj, (C, R), generator=gen) + torch.arange(C)[:, None] * n_obj).to(torch.int32).to(dev)
    pts = (torch.rand(C, R, S, 3, generator=gen) * 2 - 1).to(dev)
    nb = int(_C.load().cnr_field_fwd_render_blocks(R, S))
    for lo in (None, cnr_amd.ops.pack_weights_lo(trunk)):
        f = lambda *s: torch.full(s, float("nan"), device=dev)
        ws = torch.zeros(int(_C.load().cnr_field_fwd_render_workspace_bytes(C, R, S)), device=dev, dtype=torch.uint8)
        o = dict(d_sigma=f(C, R, S), d_color=f(C, R, S, 3), depth=f(C, R), var=f(C, R), rgb=f(C, R, 3), opacity=f(C, R))
        _C.call("cnr_field_fwd_render", pts, B, packed, brows, ray_row, 2.0, z, gt_d, gt_c, labels, dmask, 5.0, 10.0, 1.0,
                o["d_sigma"], o["d_color"], o["depth"], o["var"], o["rgb"], o["opacity"], C, R, S, 0, ws, ws.numel(), lo, None, None)
        losses, flags = f(3, C), torch.full((C,), -1, device=dev, dtype=torch.int32)
        _C.call("cnr_render_loss_finish", ws, losses, flags, C, R, nb)
        show("field_fwd_render S%d packed_lo%d empty%d" % (S, lo is not None, empty), losses=losses, flags=flags, **o)

# ---- two steps of every trainer whose step composites rays -----------------------------------------------------------------------
R = 64


def config(n1=2, n2=8):
    cfg = cnr_amd.cfg.synthetic_config(device=str(dev), latent_dim=32, n_bins_cam2surface=n1, n_bins=n2)
    cfg.hidden_feature_size_bg, cfg.n_bins_cam2surface_bg = 128, 6              # background: S = 6 + 8 = 14
    return cfg


torch.manual_seed(31)                                                            # module initialisation
pool = cnr_amd.scene_cateogries.synthetic_pool(5 * R, 1, torch.Generator().manual_seed(12), "cpu")
bg = cnr_amd.background.BackgroundStep(config(), pool, R, dev, seed=5, precision="fused")
for _ in range(2):
    bg.step(use_graph=False)
show("background fused", flat=bg.flat, exp_avg=bg.exp_avg, losses=bg.losses, flags=bg.fb["flags"])

gen = torch.Generator().manual_seed(0)
pools = {o: cnr_amd.scene_cateogries.synthetic_pool(4 * R, 1, gen, "cpu") for o in range(3)}
ot = cnr_amd.object_fields.ObjectFieldTrainer(config(1, 9), pools, [0, 1, 2], rays_per_step=R, seed=1)
for _ in range(2):
    ot.launch()
show("object_fields", theta=ot.theta, exp_avg=ot.exp_avg, losses=ot.losses, flags=ot.flags)

cfg = config(1, 9)
torch.manual_seed(0)
net = cnr_amd.trainer.Trainer(cfg, 1, [0, 1, 2, 3])
insts = []
for i in range(2):
    p = cnr_amd.scene_cateogries.synthetic_pool(4 * R, 1, gen, "cpu")
    insts.append(dict(inst_id=100 + i, cls_id=1, pool=dict(rgbs=p["rgbs"], depth=p["depth"], dirs=p["dirs"], T=p["T_co"])))
fit = cnr_amd.code_fit.CodeFitter(cfg, {1: net}, insts, starts=("random", 2), rays_per_step=R, seed=1)
for _ in range(2):
    fit.launch()
show("code_fit", codes=fit._codes, exp_avg=fit.exp_avg, losses=fit.losses, flags=fit.flags)

# the category trainer without the one-launch step: S = 10 -> cnr_field_fwd + cnr_render_loss (counts_tab, d_state), S = 32 ->
# cnr_field_fwd_render, each followed by the stand-alone field backward
for n1, n2 in ((2, 8), (4, 28)):
    gen = torch.Generator().manual_seed(21)
    pools = [cnr_amd.scene_cateogries.synthetic_pool(5 * R, 4, gen, "cpu") for _ in range(2)]
    tr = cnr_amd.fused.FusedCategoryTrainer(config(n1, n2), 2, 4, pools, R, dev, seed=1, generator=gen, use_graph=False,
                                            one_launch=False)
    assert not tr._ft_blocks and bool(tr._rl_blocks) == (n1 + n2 == 32)
    for _ in range(2):
        tr.step()
    show("categories two-launch S%d" % (n1 + n2), theta=tr.theta, exp_avg=tr.exp_avg, losses=tr.losses, flags=tr.flags)
