"""CPU restatement of ONE object's step of cnr_obj_train (TEST INFRASTRUCTURE): the reference's background branch at width 32
(train.py:113-121,172-184) put together from oracle/ref_cpu.py's functions -- origin_dirs_W, sample_3d_points, unidirs_embed,
occupancy_map_forward, composite (inside step_batch_loss), step_batch_loss -- and torch.optim.AdamW.

The sampling runs in fp32 whatever ``dtype`` says (z and the sample points are the step's INPUT: the kernel's are held to the
reference's bit for bit); the field, the composite, the losses, the backward and the optimiser run in ``dtype`` (fp32: the
reference's own arithmetic, which tests/test_objfields_host.py ties to its recorded vector; fp64: the oracle of the GPU tests)."""
import math

import torch

from oracle import ref_cpu as O

NAMES = ["in_layer.0.weight", "in_layer.0.bias", "mid1.0.0.weight", "mid1.0.0.bias", "cat_layer.0.weight", "cat_layer.0.bias",
         "mid2.0.0.weight", "mid2.0.0.bias", "out_alpha.weight", "out_alpha.bias", "color_linear.0.weight",
         "color_linear.0.bias", "out_color.weight", "out_color.bias"]
SHAPES = [(32, 87), (32,), (32, 32), (32,), (32, 119), (32,), (32, 32), (32,), (1, 32), (1,), (32, 74), (32,), (3, 32), (3,)]
P = sum(math.prod(s) for s in SHAPES) + 63


def init_params(generator, jitter_B=0.0):
    """Trainer's initialisation (a10): xavier-normal weights, nn.Linear's default biases, the icosahedral B (+ jitter, so that
    objects differ in every tensor) -> ({name: tensor}, B (21,3)), fp32"""
    p = {}
    for n, s in zip(NAMES, SHAPES):
        if len(s) == 2:
            p[n] = torch.randn(s, generator=generator) * math.sqrt(2.0 / (s[0] + s[1]))
            fan_in = s[1]
        else:
            p[n] = (torch.rand(s, generator=generator) * 2 - 1) / math.sqrt(fan_in)
    B = torch.tensor(O.UNIDIRS, dtype=torch.float32).reshape(21, 3)
    return p, B + jitter_B * torch.randn(21, 3, generator=generator)


def flatten(params, B):
    """the kernel's theta layout: the 14 tensors in registration order, then B_layer.weight"""
    return torch.cat([params[n].reshape(-1) for n in NAMES] + [B.reshape(-1)])


def unflatten(theta):
    p, off = {}, 0
    for n, s in zip(NAMES, SHAPES):
        k = math.prod(s)
        p[n] = theta[off:off + k].reshape(s).clone()
        off += k
    return p, theta[off:off + 63].reshape(21, 3).clone()


class ObjectOracle:
    def __init__(self, params, B, scale, n1, n2, eps, stop_eps, min_bound=0.0, lr=1e-3, weight_decay=0.013, dtype=torch.float64):
        self.dtype = dtype
        self.params = {n: params[n].to(dtype).clone().requires_grad_() for n in NAMES}
        self.B = B.to(dtype).clone().requires_grad_()
        self.scale, self.n1, self.n2, self.eps, self.stop_eps, self.min_bound = scale, n1, n2, eps, stop_eps, min_bound
        self.opt = torch.optim.AdamW(list(self.params.values()) + [self.B], lr=lr, weight_decay=weight_decay, betas=(0.9, 0.999),
                                     eps=1e-8)

    def load_state(self, theta, exp_avg, exp_avg_sq, steps):
        """start the next step from given parameters, AdamW moments (flat, the kernel's layout) and optimiser step count"""
        leaves = [self.params[n] for n in NAMES] + [self.B]
        off = 0
        with torch.no_grad():
            for p in leaves:
                k = p.numel()
                p.copy_(theta[off:off + k].reshape(p.shape).to(self.dtype))
                self.opt.state[p] = dict(step=torch.tensor(float(steps)), exp_avg=exp_avg[off:off + k].reshape(p.shape).to(self.dtype).clone(),
                                         exp_avg_sq=exp_avg_sq[off:off + k].reshape(p.shape).to(self.dtype).clone())
                off += k

    def theta(self):
        return flatten({n: p.detach() for n, p in self.params.items()}, self.B.detach())

    def step(self, rgbs, depth, dirs, T_wc, u, g):
        """one step on the R given pool rows with the given draws -> z, pts, sigma (R,S), rgb (R,S,3), losses (3,), grad (P,),
        theta (P,) after the update"""
        dt = self.dtype
        origins, dirs_w = O.origin_dirs_W(T_wc, dirs)
        gt_rgb, gt_depth, valid, labels, pts, z = O.sample_3d_points(rgbs, depth, origins, dirs_w, u, g, self.n1, self.n2, self.eps,
                                                                     self.stop_eps, self.min_bound)
        emb = O.unidirs_embed(pts.to(dt)[None], self.B[None], self.scale)[0]
        alpha, color = O.occupancy_map_forward(self.params, emb)
        loss, terms, _ = O.step_batch_loss(alpha[None], color[None], gt_depth.to(dt)[None], (gt_rgb.float() / 255.0).to(dt)[None],
                                           labels[None], valid[None], z.to(dt)[None])
        self.opt.zero_grad(set_to_none=True)
        if loss.requires_grad:
            loss.backward()
        leaves = [self.params[n] for n in NAMES] + [self.B]
        for p in leaves:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        grad = torch.cat([p.grad.reshape(-1) for p in leaves]).clone()
        self.opt.step()
        return dict(z=z, pts=pts, sigma=alpha.detach().squeeze(-1), rgb=color.detach(),
                    losses=torch.stack([terms["depth"][0], terms["color"][0], terms["opacity"][0]]).detach(), grad=grad,
                    theta=self.theta())
