"""CPU: the host half of the code fit (code_fit.CodeFitter, cnr_code_fit): the oracle of its GPU tests against the vector the
REFERENCE recorded for one such step, the state rule, the starts, ``attach`` on CPU modules, the refusals and the header."""
import math

import numpy as np
import pytest
import torch

import codefit_cpu as FC
from conftest import Golden, rel_l2


@pytest.fixture(scope="module")
def cnr():
    import cnr_amd
    return cnr_amd


def golden_case(g):
    """(params, B, codes (2,L), pool) of a one-class, one-object fixture"""
    params = {k: v[0] for k, v in g.mlp().items()}
    codes = torch.stack([g.t("shape_codes")[0, 0], g.t("texture_codes")[0, 0]])
    pool = dict(rgbs=g.t("pool_rgbs")[0], depth=g.t("pool_depth")[0], dirs=g.t("pool_dirs")[0], T=g.t("pool_T")[0])
    return params, g.t("B")[0], codes, pool


def test_the_oracle_in_fp32_reproduces_the_reference_vector():
    """tests/golden/edge_single_obj_W.npz is a one-object class step as the reference computed it (R = 64, S = 16, L = 256, world
    frame, regulariser off): its code gradients and new codes are exactly one fit step.  codefit_cpu in fp32 is held to it at the
    bars tests/test_objfields_host.py uses for its own tie (outputs and loss 2e-6, gradients 2e-5, update 1e-6)."""
    g = Golden("edge_single_obj_W")
    assert (g.C, g.R, g.S, g.L, g.n_obj, g.single_obj) == (1, 64, 16, 256, 1, True)
    params, B, codes, pool = golden_case(g)
    orc = FC.FitOracle(params, B, codes, g.scale, g.n1, g.n2, g.eps, g.stop_eps, reg_scaling=0.0, world_frame=True, dtype=torch.float32)
    out = orc.step(pool["rgbs"], pool["depth"], pool["dirs"], pool["T"], g.t("u")[0], g.t("g")[0])
    assert torch.equal(out["z"], g.t("z")[0]) and torch.equal(out["pts"], g.t("pts")[0])
    assert rel_l2(out["sigma"], g.t("sigmas")[0].squeeze(-1)) < 2e-6 and rel_l2(out["rgb"], g.t("rgbs")[0]) < 2e-6
    for k, key in enumerate(("loss_depth", "loss_color", "loss_opacity")):
        assert rel_l2(out["losses"][k], g.t(key)[0]) < 2e-6, key
    assert rel_l2(out["grad"][0], g.t("grad_shape_codes")[0, 0]) < 2e-5 and rel_l2(out["grad"][1], g.t("grad_texture_codes")[0, 0]) < 2e-5
    assert rel_l2(out["codes"][0], g.t("new_shape_codes")[0, 0]) < 1e-6 and rel_l2(out["codes"][1], g.t("new_texture_codes")[0, 0]) < 1e-6
    # ... and the update itself, which is all of 1e-3 of the codes: a dead step would pass the bar on the codes
    for k, key in enumerate(("shape_codes", "texture_codes")):
        assert rel_l2(out["codes"][k] - codes[k], g.t("new_" + key)[0, 0] - codes[k]) < 1e-3, key


def test_flatten_net_is_the_param_layout_row(cnr):
    gen = torch.Generator().manual_seed(3)
    params, B = FC.init_net(gen, L=32, jitter_B=0.01)
    row = FC.flatten_net(params, B)
    lay = cnr.fused.ParamLayout(32, 0)
    assert row.numel() == lay.total == 13892 + 4 * 32 * 32 + 128 + 63 and lay.shape == (lay.total, lay.total)
    v = lay.views(row[None])
    assert torch.equal(v["latW"][0, 1], params["cat_latent_layer.0.weight"]) and torch.equal(v["B"][0], B)
    assert torch.equal(v["latb"][0, 3], params["texture_latent_layer_1.0.bias"])
    assert [n for n, _, _ in cnr.ops.TRUNK_LAYERS] == FC.TRUNK and cnr.ops.LATENT_LAYERS == FC.LATENT
    assert torch.equal(row[:32 * 87].reshape(32, 87), params["encoding_xyz.0.weight"])


def test_next_state_is_the_object_step_rule(cnr):
    nxt = cnr.code_fit.next_state
    s, m, starts = [0, 0, 0, 0], [0, 0, 0, 0], []
    for _ in range(7):
        starts.append((s[0], s[3]))
        s, m = nxt(s, 49, 24), FC.next_state(m, 49, 24)
        assert s == m
    assert starts == [(0, 0), (24, 0), (0, 1), (24, 1), (0, 2), (24, 2), (0, 3)]     # 2 R + 1 rows: two slices per epoch
    assert nxt([0, 0, 0, 0], 24, 24) == [0, 1, 1, 1]                                  # exactly R rows: every step the full batch


def test_starts(cnr):
    cf = cnr.code_fit
    gen = torch.Generator().manual_seed(5)
    sh, tx = torch.randn(3, 32, generator=gen), torch.randn(3, 32, generator=gen)
    mean = cf.build_starts("mean", sh, tx, 0, 7)
    assert mean.shape == (1, 2, 32) and torch.allclose(mean[0, 0], sh.mean(0)) and torch.allclose(mean[0, 1], tx.mean(0))
    objs = cf.build_starts("objects", sh, tx, 0, 7)
    assert objs.shape == (3, 2, 32) and torch.equal(objs[:, 0], sh) and torch.equal(objs[:, 1], tx)
    rnd = cf.build_starts(("random", 4), sh, tx, 0, 7)
    assert rnd.shape == (4, 2, 32) and torch.equal(rnd, cf.build_starts(("random", 4), sh, tx, 0, 7))
    assert not torch.equal(rnd, cf.build_starts(("random", 4), sh, tx, 0, 8))          # seeded by (seed, inst_id)
    assert not torch.equal(rnd, cf.build_starts(("random", 4), sh, tx, 1, 7))
    big = cf.random_codes(4000, 32, 0, 1)
    assert abs(float(big.std()) - 1 / math.sqrt(16)) < 0.01                             # Trainer.load_codes: randn / sqrt(L / 2)
    given = torch.randn(2, 2, 32, generator=gen)
    combo = cf.build_starts(["mean", ("random", 2), given, "objects"], sh, tx, 0, 7)
    assert combo.shape == (8, 2, 32) and torch.equal(combo[:1], mean) and torch.equal(combo[1:3], rnd[:2])
    assert torch.equal(combo[3:5], given) and torch.equal(combo[5:], objs)
    with pytest.raises(ValueError, match=r"\(M, 2, 32\)"):
        cf.build_starts(torch.zeros(2, 32), sh, tx, 0, 7)
    with pytest.raises(ValueError, match="unknown start"):
        cf.build_starts("median", sh, tx, 0, 7)
    with pytest.raises(ValueError, match="no start"):
        cf.build_starts([], sh, tx, 0, 7)


def _cpu_trainer(cnr, inst_ids, L=32):
    cfg = cnr.cfg.synthetic_config(device="cpu", latent_dim=L, n_bins_cam2surface=1, n_bins=9)
    return cfg, cnr.trainer.Trainer(cfg, 3, list(inst_ids))


def test_attach_on_cpu_modules(cnr):
    cfg, t = _cpu_trainer(cnr, [4, 9])
    sh0, tx0 = t.shape_codes.weight.data.clone(), t.texture_codes.weight.data.clone()
    a, b = torch.arange(32.0), -torch.arange(32.0)
    cnr.code_fit.attach_codes(t, 21, a, b, extent=[0.4, 0.2, 0.6])
    assert t.n_obj == 3 and t.inst_id_to_index == {4: 0, 9: 1, 21: 2}
    assert torch.equal(t.shape_codes.weight.data, torch.cat([sh0, a[None]])) and torch.equal(t.texture_codes.weight.data, torch.cat([tx0, b[None]]))
    assert torch.equal(t.shape_codes(torch.tensor(2)), a) and isinstance(t.shape_codes, torch.nn.Embedding)
    assert list(t.extent_dict.keys()) == [21] and np.allclose(t.extent_dict[21], [0.4, 0.2, 0.6])
    with pytest.raises(ValueError, match="instance 9 is already"):
        cnr.code_fit.attach_codes(t, 9, a, b)
    cnr.code_fit.attach_codes(t, 22, b, a)                                              # no extent: the dictionary is left alone
    assert t.n_obj == 4 and list(t.extent_dict.keys()) == [21]
    # a category of ONE instance meshes from bound_dict (world frame): a second row would break the instance it has
    _, single = _cpu_trainer(cnr, [4])
    with pytest.raises(NotImplementedError, match="single instance"):
        cnr.code_fit.attach_codes(single, 5, a, b, extent=[1.0, 1.0, 1.0])
    assert single.n_obj == 1 and single.shape_codes.weight.shape[0] == 1


def test_load_category_reads_the_reference_checkpoint_schema(cnr, tmp_path):
    cfg, t = _cpu_trainer(cnr, [4, 9])
    ck = {"global_step": 700, "PE_state_dict": t.pe.state_dict(), "FC_state_dict": t.fc_occ_map.state_dict(), "cls_id": 3,
          "instance_id_to_index": {9: 1, 4: 0}, "obj_scale": 2.0, "obj_tensor_dict": {}, "shape_code_state_dict": t.shape_codes.state_dict(),
          "texture_code_state_dict": t.texture_codes.state_dict(), "bound": {4: np.array([1.0, 2.0, 3.0]), 9: np.array([0.5, 0.5, 0.5])}}
    assert set(ck) >= set(cnr.scene_cateogries.sceneCategory.CKPT_KEYS_OBJ)
    path = str(tmp_path / "cls_3_iteration_00700.pth")
    torch.save(ck, path)
    back = cnr.code_fit.load_category(cfg, path)
    assert back.cls_id == 3 and back.n_obj == 2 and back.inst_id_to_index == {4: 0, 9: 1} and list(back.extent_dict) == [4, 9]
    assert torch.equal(back.shape_codes.weight, t.shape_codes.weight) and torch.equal(back.texture_codes.weight, t.texture_codes.weight)
    for (n, p), (_, q) in zip(back.fc_occ_map.state_dict().items(), t.fc_occ_map.state_dict().items()):
        assert torch.equal(p, q), n
    assert torch.equal(back.pe.B_layer.weight, t.pe.B_layer.weight)
    del ck["shape_code_state_dict"]
    torch.save(ck, path)
    with pytest.raises(KeyError, match="shape_code_state_dict"):
        cnr.code_fit.load_category(cfg, path)


def _pool(n):
    return dict(rgbs=torch.zeros(n, 4, dtype=torch.uint8), depth=torch.ones(n), dirs=torch.ones(n, 3), T=torch.eye(4).repeat(n, 1, 1))


def test_refusals_come_before_any_device_work(cnr):
    F = cnr.code_fit.CodeFitter
    cfg, t = _cpu_trainer(cnr, [4, 9])
    cfg.training_device = "cuda:0"
    inst = lambda i, c, n: dict(inst_id=i, cls_id=c, pool=_pool(n))
    with pytest.raises(ValueError, match="class 0"):
        F(cfg, {0: t}, [inst(1, 0, 100)], rays_per_step=24)
    with pytest.raises(ValueError, match="class 0"):
        F(cfg, {3: t}, [inst(1, 0, 100)], rays_per_step=24)
    with pytest.raises(ValueError, match="class 5, which has no network"):
        F(cfg, {3: t}, [inst(1, 5, 100)], rays_per_step=24)
    with pytest.raises(ValueError, match="instance 8 .*23 rows"):
        F(cfg, {3: t}, [inst(1, 3, 100), inst(8, 3, 23)], rays_per_step=24)
    with pytest.raises(ValueError, match="no instance"):
        F(cfg, {3: t}, [], rays_per_step=24)
    with pytest.raises(ValueError, match=r"instance id 2147483649 is outside"):      # would share rows and draws with instance 1
        F(cfg, {3: t}, [inst(1, 3, 100), inst(2 ** 31 + 1, 3, 100)], rays_per_step=24)
    with pytest.raises(ValueError, match="instance id -1"):
        F(cfg, {3: t}, [inst(-1, 3, 100)], rays_per_step=24)
    with pytest.raises(ValueError, match="seed -5"):
        F(cfg, {3: t}, [inst(1, 3, 100)], rays_per_step=24, seed=-5)
    bad = cnr.cfg.synthetic_config(device="cuda:0", latent_dim=32, n_bins_cam2surface=1, n_bins=9)
    bad.net_hyperparams = dict(bad.net_hyperparams, W=64)
    with pytest.raises(NotImplementedError, match="W 32"):
        F(bad, {3: t}, [inst(1, 3, 100)], rays_per_step=24)
    bad.net_hyperparams = dict(bad.net_hyperparams, W=32, shape_blocks=3)
    with pytest.raises(NotImplementedError, match=r"blocks \(2, 1\)"):
        F(bad, {3: t}, [inst(1, 3, 100)], rays_per_step=24)
    many = cnr.cfg.synthetic_config(device="cuda:0", latent_dim=32, n_bins_cam2surface=9, n_bins=56)
    with pytest.raises(NotImplementedError, match="64 samples"):
        F(many, {3: t}, [inst(1, 3, 100)], rays_per_step=24)
    other = cnr.cfg.synthetic_config(device="cuda:0", latent_dim=64, n_bins_cam2surface=1, n_bins=9)
    with pytest.raises(ValueError, match="codes of length 32"):
        F(other, {3: t}, [inst(1, 3, 100)], rays_per_step=24)


def test_header_declares_the_entry_points(cnr):
    _C = cnr._C
    assert {"cnr_code_fit", "cnr_code_fit_workspace_bytes"} <= set(_C.SIGNATURES)
    assert "cnr_code_fit_workspace_bytes" in _C._RESTYPE64 and "cnr_code_fit" not in _C.STRUCTS
    assert len(_C.SIGNATURES["cnr_code_fit"]) == 54                                     # positional, the stream last
    assert cnr.code_fit.LOSS_NAMES == ("depth", "color", "opacity", "shape_norm", "texture_norm")
