"""CPU: the torch emulation the GPU gradient tests compare the kernels with (tests/f16_emulation.py) is itself pinned here, on
the golden fixtures, without any kernel: a reference that is wrong would make those tests meaningless.

  * the precise geometry branch's sigma is the f64 network's to 5e-6 (measured <= 1.6e-6 on the nine fixtures; the bar leaves
    torch's summation order a factor three), and the plain pipeline is at least 100 x further away (measured 300 .. 900 x):
    the residual products are in the value;
  * the residual products are NOT in the gradient: a geometry product differentiates as f16(W) f16(x), bit for bit;
  * its colours meet north_star's 1e-3 against the golden fp32 colours (measured <= 1.3e-4);
  * its trunk gradient points along the golden fp32 gradient: cosine > 0.9999 (measured >= 0.999998).  Per tensor the distance
    is printed, not asserted (measured worst 0.097 on texture_codes of s0_c2_r64_s16_l32, 0.091 on encoding_viewdir.0.weight
    of edge_single_obj_W: flipped units of the colour branch, which stays plain f16): the baseline of the GPU tests' bars."""
import pytest
import torch

from conftest import Golden, golden_names, rel_l2
from f16_emulation import _ste_half, _wt, emulated_grads, emulated_step, prod3


@pytest.fixture(scope="module")
def cnr():
    import cnr_amd
    return cnr_amd


@pytest.mark.parametrize("name", golden_names())
def test_precise_emulation_forward_against_f64_and_golden(cnr, name):
    g = Golden(name, "cpu")
    lat = cnr.ops.LATENT_LAYERS
    with torch.no_grad():
        sig64 = emulated_step(lat, g, "cpu", exact=True)[4]
        _, _, _, _, sig_p, rgb_p = emulated_step(lat, g, "cpu", precise=True)
        sig_0 = emulated_step(lat, g, "cpu", precise=False)[4]
    assert sig64.dtype == torch.float64 and sig_p.dtype == torch.float32
    e_p, e_0 = rel_l2(sig_p, sig64), rel_l2(sig_0, sig64)
    e_rgb = rel_l2(rgb_p, g.t("rgbs"))
    print(f"[emu-host] {name}: sigma precise vs f64 {e_p:.2e}, plain vs f64 {e_0:.2e} ({e_0 / e_p:.0f} x), rgb vs golden {e_rgb:.2e}")
    assert e_p < 5e-6
    assert e_0 >= 100.0 * e_p
    assert e_rgb < 1e-3
    # the f64 network is the reference's network: its sigma is the golden fp32 sigma to fp32 rounding
    assert rel_l2(sig64, g.t("sigmas").squeeze(-1)) < 1e-5


def test_residual_products_carry_no_gradient():
    """value: three products; gradient: that of f16(W) f16(x) alone -- dW = g^T f16(x), dx = g f16(W)"""
    gen = torch.Generator().manual_seed(11)
    for K, scale in ((87, 1.0), (32, 37.0)):
        x = (torch.randn(2, 5, 7, K, generator=gen) * scale).requires_grad_()
        W = (torch.randn(2, 32, K, generator=gen) * 0.3).requires_grad_()
        up = torch.randn(2, 5, 7, 32, generator=gen)
        y = prod3(x, W)
        dx, dW = torch.autograd.grad(y, (x, W), up)
        xh, Wh = x.detach().half().float(), W.detach().half().float()
        # (by hand to fp32 summation order; a residual product that leaked would add g Wl or g^T xl: 2^-12 = 2.4e-4)
        assert rel_l2(dx, torch.matmul(up, Wh[:, None])) < 1e-6
        assert rel_l2(dW, torch.matmul(up.reshape(2, 35, 32).transpose(1, 2), xh.reshape(2, 35, K))) < 1e-6
        # ... and bit for bit autograd of the plain product, while the VALUE is not the plain product's: it is the fp32 product
        # to ~2^-22, where the plain one stops at f16 operand rounding (2^-11 per operand)
        x2, W2 = x.detach().clone().requires_grad_(), W.detach().clone().requires_grad_()
        y_plain = torch.matmul(_ste_half(x2), _wt(_ste_half(W2)))
        dx2, dW2 = torch.autograd.grad(y_plain, (x2, W2), up)
        assert torch.equal(dx, dx2) and torch.equal(dW, dW2)
        y64 = torch.matmul(x.detach().double(), _wt(W.detach().double()))
        assert rel_l2(y, y64) < 2e-6 and rel_l2(y_plain, y64) > 1e-4


@pytest.mark.parametrize("name", golden_names())
def test_precise_emulation_gradient_against_golden_fp32(cnr, name):
    g = Golden(name, "cpu")
    _, grads = emulated_grads(cnr, g, "cpu", precise=True, regulariser=g.n_obj > 1)
    ref = {k[5:]: g.t(k) for k in g.z.files if k.startswith("grad.")}
    ref["B"], ref["shape_codes"], ref["texture_codes"] = g.t("grad_B"), g.t("grad_shape_codes"), g.t("grad_texture_codes")
    assert set(ref) == set(grads)
    trunk = [n + s for n, _, _ in cnr.ops.TRUNK_LAYERS for s in (".weight", ".bias")]
    a = torch.cat([grads[k].reshape(-1) for k in trunk]).double()
    b = torch.cat([ref[k].reshape(-1) for k in trunk]).double()
    cos = float(a @ b / (a.norm() * b.norm()))
    per = {k: rel_l2(grads[k], ref[k]) for k in ref if float(ref[k].abs().sum()) > 0}
    worst = max(per, key=per.get)
    print(f"[emu-host] {name}: trunk cosine vs golden fp32 {cos:.6f}, worst tensor {worst} {per[worst]:.4f} | "
          + " ".join(f"{k}={v:.4f}" for k, v in per.items()))
    assert cos > 0.9999
