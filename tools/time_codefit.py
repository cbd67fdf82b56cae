"""Times one optimisation step of K code-fit candidates (R = 120 rays x S = 10 samples each, L = 256) on the GPU, by device events
after warm-up:

  fused     ONE cnr_code_fit launch for all K candidates (code_fit.CodeFitter.launch), and
  modular   K sequential steps of the drop-in modules: cnr_sample_rays on the candidate's slice, UniDirsEmbed, model.CodeNeRF with
            requires_grad off on the network, loss.step_batch_loss, the code-norm regulariser, autograd to the two codes, torch AdamW on
            them -- the only way to do this work without cnr_code_fit.  Every call is issued from Python; nothing is captured.

Both sides alternate inside one process; each figure is the median of `--rounds` windows of `--reps` steps, with the smallest and
the largest window beside it.  Nothing here assumes a ratio: the file holds what was measured.

    python tools/time_codefit.py [--reps 50] [--rounds 5] [--sizes 8,64,256] [--out profiles/codefit_time.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

R, N1, N2, L = 120, 1, 9, 256
VECTOR_FP32_PEAK = 157.3e12          # MI355X: 256 CUs x 128 lanes x 2 flop x 2.4 GHz


def step_flops(R, S, L):
    """multiply-adds x 2 of one candidate's step: trunk forward (13 696 weights), the backward down the activation path (seven
    32-wide products less encoding_xyz's, rgb.0, the heads), the latent layers forward and backward (4 x 32 x L each)"""
    M = R * S
    w_fwd = 32 * (87 + 32 + 119 + 32 + 32 + 74 + 32) + 16 * 32 + 32 + 48
    w_bwd = 6 * 32 * 32 + 16 * 32 + 32 + 48
    return 2 * M * (w_fwd + w_bwd) + 2 * 2 * 4 * 32 * L


def _window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


class ModularCandidate:
    """one candidate on the drop-in modules: the codes are the only leaves"""

    def __init__(self, cnr, cfg, trainer, pool, codes, seed):
        self.cnr, self.cfg, self.t, self.pool, self.seed, self.k = cnr, cfg, trainer, pool, seed, 0
        self.cs = codes[0].clone().requires_grad_()
        self.ct = codes[1].clone().requires_grad_()
        self.opt = torch.optim.AdamW([self.cs, self.ct], lr=cfg.code_learning_rate, weight_decay=cfg.code_weight_decay)
        self.rows = pool["depth"].shape[0]

    def step(self):
        cnr, cfg, p = self.cnr, self.cfg, self.pool
        a = (self.k * R) % (self.rows - R)
        sl = lambda t: t[None, a:a + R]
        b = cnr.ops.sample_rays(sl(p["rgbs"]), sl(p["depth"]), sl(p["dirs"]), sl(p["T"]), N1, N2, cfg.surface_eps, cfg.stop_eps,
                                cfg.min_depth, seed=self.seed, offset=4 * self.k)
        emb = self.t.pe(b["pts"][0])
        alpha, color = self.t.fc_occ_map(emb, self.cs.expand(R, 1, L), self.ct.expand(R, 1, L))
        loss, _, _ = cnr.loss.step_batch_loss(alpha[None], color[None], b["gt_depth"], b["gt_rgb"], b["labels"], b["depth_mask"], b["z"])
        loss = loss + 0.0005 * (torch.norm(self.cs) + torch.norm(self.ct))
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        self.opt.step()
        self.k += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="8,64,256")
    ap.add_argument("--modular-max", type=int, default=64, help="largest K whose K modular steps are timed (they are sequential)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import cnr_amd as cnr
    from cnr_amd.code_fit import CodeFitter
    assert torch.cuda.is_available(), "time_codefit needs the GPU"
    dev = torch.device("cuda:0")
    cfg = cnr.cfg.synthetic_config(device=str(dev), latent_dim=L, n_bins_cam2surface=N1, n_bins=N2)
    torch.manual_seed(0)
    trainer = cnr.trainer.Trainer(cfg, 1, [0, 1, 2, 3])
    for q in list(trainer.fc_occ_map.parameters()) + list(trainer.pe.parameters()):
        q.requires_grad_(False)
    gen = torch.Generator().manual_seed(0)
    sizes = [int(s) for s in a.sizes.split(",")]
    n_inst = max(1, max(sizes) // 4)                 # four starts per instance
    insts = []
    for i in range(n_inst):
        p = cnr.scene_cateogries.synthetic_pool(2048, 1, gen, "cpu")
        insts.append(dict(inst_id=100 + i, cls_id=1, pool=dict(rgbs=p["rgbs"], depth=p["depth"], dirs=p["dirs"], T=p["T_co"])))
    n_mod = min(max(sizes), a.modular_max)
    rows = {}
    for K in sizes:
        fit = CodeFitter(cfg, {1: trainer}, insts[:max(1, K // 4)], starts=("random", min(4, K)), rays_per_step=R, seed=1)
        assert fit.K == K, (fit.K, K)
        mods = []
        if K <= n_mod:
            for k in range(K):
                pool = {key: v.to(dev) for key, v in insts[k // 4]["pool"].items()}
                mods.append(ModularCandidate(cnr, cfg, trainer, pool, fit._codes[k], seed=k))
        for _ in range(5):
            fit.launch()
        for m in mods:
            for _ in range(3):
                m.step()
        torch.cuda.synchronize()
        fused, modular = [], []
        for _ in range(a.rounds):        # alternate the sides
            fused.append(_window(fit.launch, a.reps))
            if mods:
                modular.append(_window(lambda: [m.step() for m in mods], max(2, a.reps // 10)))
        f = statistics.median(fused)
        fl = K * step_flops(R, N1 + N2, L)
        row = dict(fused_ms=round(f, 4), fused_ms_min_max=[round(min(fused), 4), round(max(fused), 4)],
                   fused_us_per_candidate=round(1e3 * f / K, 3), flops_per_step=fl, fused_tflops=round(fl / (f * 1e-3) / 1e12, 3),
                   fused_share_of_fp32_vector_peak=round(fl / (f * 1e-3) / VECTOR_FP32_PEAK, 4), mfma_fraction=0.0,
                   finite=bool(torch.isfinite(fit._codes).all()), flags=sorted(set(fit.flags.cpu().tolist())))
        if modular:
            m = statistics.median(modular)
            row.update(modular_ms=round(m, 3), modular_ms_min_max=[round(min(modular), 3), round(max(modular), 3)],
                       modular_over_fused=round(m / f, 1))
        rows[str(K)] = row
        print(K, json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(dict(device=torch.cuda.get_device_name(0), R=R, S=N1 + N2, L=L, reps=a.reps, rounds=a.rounds, rows=rows), fo, indent=1)


if __name__ == "__main__":
    main()
