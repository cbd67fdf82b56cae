"""The fused kernels' arithmetic restated with torch ops (no kernel involved; runs on any device), and the loss restated
with it.  Shared by tests/test_fused_gpu.py, tests/test_fullsize_gpu.py and tests/test_emulation_host.py -- the last one pins
this module itself against an f64 network and the golden vectors, on the CPU.

Two pipelines (csrc/fused_common.h "Residual image", csrc/fused_fwd.hip forward_tile):

  plain f16      every MFMA operand (weights, PE features, post-ReLU activations) rounded to f16, fp32 accumulate, fp32 sigma
                 head, latent layers folded into fp32 bias rows.
  precise        the GEOMETRY branch -- encoding_xyz.0, shape_layer_1.0, both column blocks of cat_layer.0, shape_layer_2.0,
                 encoding_shape -- carries fp32 activations (the accumulators after the fp32 ReLU) and forms every product as
                     Wh xh + Wl xh + Wh xl,   Wh = f16(W), Wl = f16(W - Wh), xh = f16(x), xl = f16(x - xh)
                 (x of the first layer and of cat's E1 columns is the fp32 PE feature vector).  The ReLU masks are those of
                 that value.  The BACKWARD of such a product is the backward of f16(W) f16(x) alone: the kernels' data-gradient
                 chain and dW products read Wh and xh of the forward that was rendered, the two residual products carry no
                 gradient.  The colour branch (encoding_viewdir.0 on f16(y4) .. rgb.2) is plain f16 in both.
"""
import torch


def _ste_half(x):
    """round to f16 in the forward, identity in the backward (what an f16 MFMA operand is)."""
    return x + (x.half().float() - x).detach()


def _wt(w):
    """(C, O, K) weights -> (C, 1, K, O) right-hand matmul operand for (C, R, S, K) inputs"""
    return w.transpose(-1, -2)[:, None]


def prod3(x, W):
    """x (C,R,S,K) fp32, W (C,O,K) fp32 -> the precise branch's product: VALUE Wh xh + Wl xh + Wh xl (fp32 accumulate), GRADIENT
    of f16(W) f16(x) only (straight-through rounding); the residual products are constants of the graph."""
    out = torch.matmul(_ste_half(x), _wt(_ste_half(W)))
    with torch.no_grad():
        xh, Wh = x.half().float(), W.half().float()
        xl, Wl = (x - xh).half().float(), (W - Wh).half().float()
        extra = torch.matmul(xh, _wt(Wl)) + torch.matmul(xl, _wt(Wh))
    return out + extra


def emulated_step(latent_layers, g, dev, precise=False, exact=False):
    """Forward of the fused pipeline on the batch g (a conftest.Golden or anything with its .t / .mlp / .C / .scale); returns
    (P, B, shape, tex, sig, rgb) with P, B, shape, tex fresh leaves that require grad.  Its autograd gradient is what an
    exact-arithmetic backward of the kernels' forward returns; it shares the kernels' ReLU masks up to fp32 summation order.
    precise: the precise geometry branch (module docstring) instead of plain f16 operands.
    exact:   the same network in float64 without any rounding (the yardstick both pipelines' sigma is measured with)."""
    dt = torch.float64 if exact else torch.float32
    ident = lambda x: x
    q = ident if exact else _ste_half
    act = ident if (precise or exact) else q                  # what is kept of a geometry activation between the layers
    if exact:
        geo = lambda x, w: torch.matmul(x, _wt(w))
    elif precise:
        geo = prod3
    else:
        geo = lambda x, w: torch.matmul(q(x), _wt(q(w)))
    C = g.C
    P = {k: v.clone().to(dt).requires_grad_() for k, v in g.mlp().items()}
    B = g.t("B").clone().to(dt).requires_grad_()
    shape = g.t("shape_codes").clone().to(dt).requires_grad_()
    tex = g.t("texture_codes").clone().to(dt).requires_grad_()
    idx = g.t("indices")
    W = lambda n: P[n + ".weight"]
    b = lambda n: P[n + ".bias"][:, None, None, :]
    lin = lambda n, x: torch.matmul(x, _wt(q(W(n))))
    # differentiable PE (oracle formula, on device)
    t = g.t("pts").to(dt) / g.scale
    proj = torch.matmul(t, B.transpose(-1, -2)[:, None])
    bands = 2.0 ** torch.arange(6, device=dev, dtype=dt)
    xb = (proj[..., None, :] * bands[:, None]).reshape(*proj.shape[:-1], -1)
    e = torch.cat([t, torch.sin(xb * torch.pi)], dim=-1)
    e1, e2 = e[..., :87], q(e[..., 87:])
    zrow = {}
    for i, n in enumerate(latent_layers):
        code = tex if i == 3 else shape
        zrow[i] = torch.relu(torch.baddbmm(P[n + ".bias"][:, None, :], code, P[n + ".weight"].transpose(1, 2)))
    gather = lambda zr: torch.stack([zr[c][idx[c]] for c in range(C)])[:, :, None, :]   # (C,R,1,32)
    fold = lambda n, zr, cols=None: torch.matmul(gather(zr), _wt(W(n) if cols is None else W(n)[:, :, :cols]))
    # geometry branch
    a0 = act(torch.relu(geo(e1, W("encoding_xyz.0")) + b("encoding_xyz.0")))
    a1 = act(torch.relu(geo(a0, W("shape_layer_1.0")) + fold("shape_layer_1.0", zrow[0]) + b("shape_layer_1.0")))
    Wc = W("cat_layer.0")
    a2 = act(torch.relu(geo(a1, Wc[:, :, :32]) + geo(e1, Wc[:, :, 32:]) + fold("cat_layer.0", zrow[1], 32) + b("cat_layer.0")))
    a3 = act(torch.relu(geo(a2, W("shape_layer_2.0")) + fold("shape_layer_2.0", zrow[2]) + b("shape_layer_2.0")))
    y4 = geo(a3, W("encoding_shape")) + b("encoding_shape")
    # sigma head: fp32 dot product on the fp32 y4
    sig = (torch.matmul(y4, _wt(W("sigma.0"))) + b("sigma.0")).squeeze(-1) * 10.0
    # colour branch: plain f16
    Wv = q(W("encoding_viewdir.0"))
    a5 = q(torch.relu(torch.matmul(q(y4), _wt(Wv[:, :, :32])) + torch.matmul(e2, _wt(Wv[:, :, 32:])) + b("encoding_viewdir.0")))
    a6 = q(torch.relu(lin("texture_layer_1.0", a5) + fold("texture_layer_1.0", zrow[3]) + b("texture_layer_1.0")))
    a7 = q(torch.relu(lin("rgb.0", a6) + b("rgb.0")))
    rgb = torch.sigmoid(lin("rgb.2", a7) + b("rgb.2"))
    return P, B, shape, tex, sig, rgb


def _emulated_f16_step(cnr, g, dev, precise=False):
    """emulated_step with the package's latent-layer names (the form the GPU tests call)."""
    return emulated_step(cnr.ops.LATENT_LAYERS, g, dev, precise=precise)


def code_regulariser(shape, tex, C):
    """src/loss.py:5-15 -- the caller adds it for classes of more than one object"""
    return 0.0005 * sum(torch.norm(shape[c], dim=-1).sum() + torch.norm(tex[c], dim=-1).sum() for c in range(C))


def emulated_grads(cnr, g, dev, precise, regulariser):
    """loss and {reference tensor name: gradient} of the emulated pipeline on g; the graph is gone when this returns"""
    P, B, shape, tex, sig, rgb = _emulated_f16_step(cnr, g, dev, precise=precise)
    loss = _torch_loss(sig, rgb, g)
    if regulariser:
        loss = loss + code_regulariser(shape, tex, g.C)
    loss.backward()
    zg = lambda p: torch.zeros_like(p) if p.grad is None else p.grad
    out = {k: zg(v) for k, v in P.items()}
    out["B"], out["shape_codes"], out["texture_codes"] = zg(B), zg(shape), zg(tex)
    return loss.detach(), out


def _torch_loss(sig, rgb, g):
    """loss.py:18-74 with device tensors (plain torch; test-side restatement of the oracle's step_batch_loss)."""
    mask_obj = g.t("labels") != 0
    mask_sem = g.t("labels") != 2
    md = g.t("depth_mask") & mask_obj
    occ = torch.sigmoid(sig)
    free = torch.cat([torch.ones_like(occ[..., :1]), (1.0 - occ + 1e-10)[..., :-1]], -1)
    term = occ * torch.cumprod(free, -1)
    z = g.t("z")
    depth = (term * z).sum(-1)
    var = (term * (z - depth[..., None]) ** 2).sum(-1).detach()
    col = (term[..., None] * rgb).sum(-2)
    opa = term.sum(-1)

    def red(l, m, v=None):
        if (m.sum(-1) == 0).any():
            return torch.zeros(l.shape[0], device=l.device)
        if v is not None:
            l = l / (torch.sqrt(v) + 1e-4)
        return l.sum(-1) / (m.sum(-1) + 1e-10)
    ld = red((depth - g.t("gt_depth")).abs() * md, md, var)
    lc = red((col - g.t("gt_rgb")).abs().sum(-1) * mask_obj, mask_obj)
    lo = red((opa - mask_obj.float()).abs() * mask_sem, mask_sem)
    return (ld + 5.0 * lc + 10.0 * lo).sum()
