"""CPU: the host half of the per-object field trainer (object_fields.ObjectFieldTrainer, cnr_obj_train): the oracle of its GPU
tests against the vector the REFERENCE recorded for one such step, the cursor / epoch rule, the checkpoint schema, the argument
errors and the header."""
import os

import pytest
import torch

import objfield_cpu as OC
from conftest import Golden, rel_l2


@pytest.fixture(scope="module")
def cnr():
    import cnr_amd
    return cnr_amd


def test_the_oracle_in_fp32_reproduces_the_reference_vector():
    """tests/golden/bg_r100_s14_h32.npz is one background-branch step of the reference at width 32: objfield_cpu in fp32 is held
    to it at the bars tests/test_oracle_golden.py uses for that file (outputs and loss 2e-6, gradients 2e-5, update 1e-6)."""
    g = Golden("bg_r100_s14_h32")
    orc = OC.ObjectOracle(g.mlp(), g.t("B")[0], g.scale, g.n1, g.n2, g.eps, g.stop_eps, dtype=torch.float32)
    out = orc.step(g.t("pool_rgbs")[0], g.t("pool_depth")[0], g.t("pool_dirs")[0], g.t("pool_T")[0], g.t("u")[0], g.t("g")[0])
    assert torch.equal(out["z"], g.t("z")[0]) and torch.equal(out["pts"], g.t("pts")[0])
    assert rel_l2(out["sigma"], g.t("sigmas")[0].squeeze(-1)) < 2e-6 and rel_l2(out["rgb"], g.t("rgbs")[0]) < 2e-6
    for k, key in enumerate(("loss_depth", "loss_color", "loss_opacity")):
        assert rel_l2(out["losses"][k], g.t(key)[0]) < 2e-6, key
    grads, gB = OC.unflatten(out["grad"])
    for n in OC.NAMES:
        assert rel_l2(grads[n], g.t("grad." + n)) < 2e-5, n
    assert rel_l2(gB, g.t("grad_B")[0]) < 2e-5
    new, nB = OC.unflatten(out["theta"])
    for n in OC.NAMES:
        assert rel_l2(new[n], g.t("new." + n)) < 1e-6, n
    assert rel_l2(nB, g.t("new_B")[0]) < 1e-6
    assert out["theta"].numel() == OC.P == 11363


def test_cursor_and_epoch_rule(cnr):
    """src/scene_cateogries.py:439-449 per object: rows = 250, R = 120 -> the steps start at rows 0 and 120, then the epoch ends"""
    nxt = cnr.object_fields.next_state
    s, starts = [0, 0, 0, 0], []
    for _ in range(5):
        starts.append((s[0], s[3]))
        s = nxt(s, 250, 120)
    assert starts == [(0, 0), (120, 0), (0, 1), (120, 1), (0, 2)] and s[1:3] == [5, 5]
    assert nxt([0, 0, 0, 0], 100, 100) == [0, 1, 1, 1]           # a pool of exactly R rows: every step is an epoch
    assert nxt([0, 7, 7, 2], 1000, 120) == [120, 8, 8, 2]
    s = [0, 0, 0, 0]
    for _ in range(8):                                             # 1000 rows: eight slices, 960 >= 880 ends the epoch
        assert s[3] == 0
        s = nxt(s, 1000, 120)
    assert s == [0, 8, 8, 1]


def test_checkpoint_schema_is_what_load_pretrained_fields_reads(cnr, tmp_path):
    of = cnr.object_fields
    cfg = cnr.cfg.synthetic_config(device="cpu")
    cfg.weight_root = str(tmp_path)
    gen = torch.Generator().manual_seed(5)
    inst_dict = {0: {}, 20: {3: {}, 4: {}}}
    want = {}
    for obj_id in (3, 4):
        params, B = OC.init_params(gen, jitter_B=0.01)
        fc = cnr.model.OccupancyMap(87, 42, hidden_size=32)
        fc.load_state_dict(params)
        pe = cnr.embedding.UniDirsEmbed(max_deg=5, scale=cfg.obj_scale)
        with torch.no_grad():
            pe.B_layer.weight.copy_(B)
        path = of.checkpoint_path(cfg.weight_root, obj_id, 250)
        assert path == os.path.join(str(tmp_path), "ckpt", str(obj_id), "obj_%d_it_00250.pth" % obj_id)
        os.makedirs(os.path.dirname(path))
        ck = of.checkpoint_dict(pe, fc, cfg.obj_scale, "box-%d" % obj_id)
        assert tuple(ck.keys()) == of.CKPT_KEYS == ("FC_state_dict", "PE_state_dict", "obj_scale", "bbox")
        assert list(ck["FC_state_dict"].keys()) == OC.NAMES and set(ck["PE_state_dict"].keys()) == {"B_layer.weight", "scale"}
        torch.save(ck, path)
        want[obj_id] = (params, B)
    boxes, pes, fcs = {}, {}, {}
    cnr.category_registration.load_pretrained_fields(inst_dict, boxes, pes, fcs, cfg)
    assert list(fcs.keys()) == [20] and list(fcs[20].keys()) == [3, 4]
    for obj_id, (params, B) in want.items():
        assert boxes[20][obj_id] == "box-%d" % obj_id
        assert torch.equal(pes[20][obj_id].B_layer.weight, B) and pes[20][obj_id]._scale == cfg.obj_scale
        for n, v in fcs[20][obj_id].state_dict().items():
            assert torch.equal(v, params[n]), n


def _pool(n):
    return dict(rgbs=torch.zeros(n, 4, dtype=torch.uint8), depth=torch.ones(n), dirs=torch.ones(n, 3), T_wc=torch.eye(4).repeat(n, 1, 1))


def test_argument_errors_come_before_any_device_work(cnr):
    T = cnr.object_fields.ObjectFieldTrainer
    cfg = cnr.cfg.synthetic_config(device="cuda:0", n_bins_cam2surface=1, n_bins=9)
    with pytest.raises(ValueError, match="object 7 .*100 rows"):
        T(cfg, {3: _pool(300), 7: _pool(100)}, [3, 7], rays_per_step=120)
    with pytest.raises(ValueError, match="no object"):
        T(cfg, {}, [])
    cfg.hidden_feature_size = 128
    with pytest.raises(NotImplementedError, match="hidden_feature_size 32"):
        T(cfg, {3: _pool(300)}, [3], rays_per_step=120)
    cfg = cnr.cfg.synthetic_config(device="cuda:0", n_bins_cam2surface=9, n_bins=56)
    with pytest.raises(NotImplementedError, match="64 samples"):
        T(cfg, {3: _pool(300)}, [3], rays_per_step=120)


def test_pool_rows_of_the_replica_fixture(cnr):
    """the crop areas of the committed Replica fixture: what rays_per_step of the end-to-end GPU test must not exceed"""
    import json
    with open(os.path.join(os.path.dirname(__file__), "golden", "dataset", "replica_frames.json")) as f:
        rows = json.load(f)["inst_dict"]
    inst_dict = {e["cls"]: ({} if e["cls"] == 0 else {i["inst"]: {"frame_info": [{"frame": fr, "bbox": bb} for fr, bb in i["frame_info"]]}
                                                    for i in e["insts"]}) for e in rows}
    n = cnr.object_fields.ObjectFieldTrainer.pool_rows(inst_dict)
    assert sorted(n.keys()) == [0, 3, 4, 5, 7] and n[0] == 2 * 14 * 15 and n[3] == 5 * 24 * 24
    assert min(n.values()) >= 120


def test_header_declares_the_entry_points_and_no_sixth_struct(cnr):
    _C = cnr._C
    assert {"cnr_obj_param_count", "cnr_obj_workspace_bytes", "cnr_obj_train"} <= set(_C.SIGNATURES)
    assert _C.SIGNATURES["cnr_obj_param_count"] == [] and "cnr_obj_workspace_bytes" in _C._RESTYPE64
    assert len(_C.SIGNATURES["cnr_obj_train"]) == 40 and "cnr_obj_train" not in _C.STRUCTS      # positional, the stream last
    assert len(_C.STRUCTS) == 5 and _C.ABI_VERSION == 3
    assert cnr.object_fields.PARAM_COUNT == OC.P


def test_argument_rules_under_the_sanitizers(tmp_path):
    """tests/obj_args_main.cpp: the host-side argument rules of cnr_obj_train (csrc/obj_args.h: what runs before a launch) as a
    stand-alone program under the address and undefined-behaviour sanitizers"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "obj_args")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(root, "category-nerf-reconstruction-official_amd", "csrc"),
                    os.path.join(root, "tests", "obj_args_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
