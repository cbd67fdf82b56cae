"""CPU restatement of ONE candidate's step of cnr_code_fit (TEST INFRASTRUCTURE): the reference's object step with a one-object
class and the network held fixed (train.py:123-167), put together from oracle/ref_cpu.py's functions -- origin_dirs_O / origin_dirs_W,
sample_3d_points, unidirs_embed, codenerf_forward, composite (inside step_batch_loss), step_batch_loss -- with autograd on the two
codes only and torch.optim.AdamW on them.

z comes out of the fp32 sampler whatever ``dtype`` says (it is the step's INPUT: the kernel's is held to the reference's bit for
bit).  Everything behind it -- the ray frame, the sample points, the embedding, the field, the composite, the losses, the backward, the
regulariser and the optimiser -- runs in ``dtype``: fp32 is the reference's own arithmetic, which tests/test_codefit_host.py ties to
its recorded vector; fp64 is the oracle of the GPU tests."""
import math

import torch

from oracle import ref_cpu as O

LATENT = ["shape_latent_layer_1.0", "cat_latent_layer.0", "shape_latent_layer_2.0", "texture_latent_layer_1.0"]
TRUNK = ["encoding_xyz.0", "shape_layer_1.0", "shape_layer_2.0", "cat_layer.0", "encoding_shape", "sigma.0", "encoding_viewdir.0",
         "texture_layer_1.0", "rgb.0", "rgb.2"]          # the kernel's blob order (include/cnr_hip.h)


def init_net(generator, L=256, jitter_B=0.0):
    """Trainer's initialisation of one category -> ({name.weight|bias: tensor}, B (21,3)), fp32, no class dimension"""
    p = {k: v[0] for k, v in O.init_codenerf_params(1, 32, L, generator).items()}
    B = torch.tensor(O.UNIDIRS, dtype=torch.float32).reshape(21, 3)
    return p, B + jitter_B * torch.randn(21, 3, generator=generator)


def init_codes(generator, L=256, n=1):
    """(n, 2, L): Trainer.load_codes' distribution"""
    return torch.randn(n, 2, L, generator=generator) / math.sqrt(L / 2)


def flatten_net(params, B):
    """one row of the kernel's theta: [trunk 13892 | latent W (4,32,L) | latent b (4,32) | B (21,3)] (fused.ParamLayout, no codes)"""
    parts = [t.reshape(-1) for n in TRUNK for t in (params[n + ".weight"], params[n + ".bias"])]
    parts += [params[n + ".weight"].reshape(-1) for n in LATENT] + [params[n + ".bias"].reshape(-1) for n in LATENT]
    return torch.cat(parts + [B.reshape(-1)]).float()


def next_state(state, rows, R):
    """[cursor, rng step, optimiser step, epoch] after one more step of R rays on a pool of ``rows`` rows
    (src/scene_cateogries.py:439-449)"""
    cursor, rng, opt, epoch = state
    cursor += R
    if cursor >= rows - R:
        cursor, epoch = 0, epoch + 1
    return [cursor, rng + 1, opt + 1, epoch]


class FitOracle:
    def __init__(self, params, B, codes, scale, n1, n2, eps, stop_eps, min_bound=0.0, lr=1e-3, weight_decay=0.013, reg_scaling=0.0,
                 world_frame=False, dtype=torch.float64):
        """``params`` / ``B``: the frozen category; ``codes`` (2, L): the start (shape, texture)"""
        self.dtype = dtype
        self.params = {n: t.to(dtype).clone()[None] for n, t in params.items()}          # (C = 1, ...): ref_cpu is class-batched
        self.B = B.to(dtype).clone()[None]
        self.cs = codes[0].to(dtype).clone().requires_grad_()
        self.ct = codes[1].to(dtype).clone().requires_grad_()
        self.scale, self.n1, self.n2, self.eps, self.stop_eps, self.min_bound = scale, n1, n2, eps, stop_eps, min_bound
        self.reg_scaling, self.world_frame = reg_scaling, world_frame
        self.opt = torch.optim.AdamW([self.cs, self.ct], lr=lr, weight_decay=weight_decay, betas=(0.9, 0.999), eps=1e-8)

    def load_state(self, codes, exp_avg, exp_avg_sq, steps):
        """start the next step from given codes, AdamW moments ((2, L) each) and optimiser step count"""
        with torch.no_grad():
            for k, p in enumerate((self.cs, self.ct)):
                p.copy_(codes[k].to(self.dtype))
                self.opt.state[p] = dict(step=torch.tensor(float(steps)), exp_avg=exp_avg[k].to(self.dtype).clone(),
                                         exp_avg_sq=exp_avg_sq[k].to(self.dtype).clone())

    def codes(self):
        return torch.stack([self.cs.detach(), self.ct.detach()])

    def evaluate(self, rgbs, depth, dirs, T, u, g):
        """forward and losses on the R given pool rows with the given draws; the total keeps its graph"""
        dt = self.dtype
        frame = O.origin_dirs_W if self.world_frame else O.origin_dirs_O
        o32, d32 = frame(T, dirs)
        gt_rgb, gt_depth, valid, labels, pts32, z = O.sample_3d_points(rgbs, depth, o32, d32, u, g, self.n1, self.n2, self.eps,
                                                                       self.stop_eps, self.min_bound)
        o, d = frame(T.to(dt), dirs.to(dt))
        pts = o[:, None, :] + d[:, None, :] * z.to(dt)[..., None]       # (fp32: sample_3d_points' own expression and bits)
        R = z.shape[0]
        emb = O.unidirs_embed(pts[None], self.B, self.scale)
        cs = self.cs[None, None, None, :].expand(1, R, 1, -1)
        ct = self.ct[None, None, None, :].expand(1, R, 1, -1)
        sig, col = O.codenerf_forward(self.params, emb, cs, ct)
        loss, terms, _ = O.step_batch_loss(sig, col, gt_depth.to(dt)[None], (gt_rgb.float() / 255.0).to(dt)[None], labels[None],
                                           valid[None], z.to(dt)[None])
        ns, nt = torch.norm(self.cs), torch.norm(self.ct)
        if self.reg_scaling > 0:
            loss = loss + self.reg_scaling * (ns + nt)
        return dict(z=z, pts=pts.detach(), sigma=sig.detach()[0, ..., 0], rgb=col.detach()[0], total=loss,
                    losses=torch.stack([terms["depth"][0], terms["color"][0], terms["opacity"][0], ns, nt]).detach())

    def step(self, rgbs, depth, dirs, T, u, g):
        """one step -> z, pts, sigma (R,S), rgb (R,S,3), losses (5,), grad (2,L), codes (2,L) after the update"""
        out = self.evaluate(rgbs, depth, dirs, T, u, g)
        self.opt.zero_grad(set_to_none=True)
        if out["total"].requires_grad:
            out["total"].backward()
        for p in (self.cs, self.ct):
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        out["grad"] = torch.stack([self.cs.grad, self.ct.grad]).clone()
        self.opt.step()
        out["total"] = out["total"].detach()
        out["codes"] = self.codes()
        return out
