"""GPU: TEASER's FPFH mode (csrc/fpfh.hip, utils.PointCloud.estimate_normals, category_registration.compute_fpfh_feature /
mutual_correspondences / FpfhTeaserSolver, teaser_utils) against the restatement tests/fpfh_cpu.py: the hybrid
search, SPFH, FPFH and the descriptor nearest neighbour bit for bit, the normals by angle where the eigenvector is well
conditioned, and the solver end to end.  tests/test_fpfh_host.py checks the restatement itself and the margins relied on here."""
import numpy as np
import pytest
import torch

import fpfh_cpu as FC
import registration_cpu as RC
from test_fpfh_host import EIGH_VS_JACOBI_ANGLE, RESTATEMENT_CLASS_ERRORS, RESTATEMENT_POSE_ERRORS

pytestmark = pytest.mark.gpu
NN_TILE, NN_BLOCK = 64, 256          # csrc/fpfh.hip: reference rows per LDS tile, queries per workgroup.  Few queries spread the
                                     # tiles over workgroups: (300, 1000) merges 16 chunks of one tile, (150, 170) three, nr <= 64 one
POSE_TOLERANCE = 1e-5                # tests/test_teaser_gpu.py's solver comparison (its rigid-copy test)
ETA1, ETA2, ETA3 = 0.06, 0.15, 0.12


@pytest.fixture(scope="module")
def cnr():
    import cnr_amd
    return cnr_amd


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _capacity(cnr):
    return int(cnr._C.load().cnr_hybrid_search_capacity())


@pytest.mark.parametrize("name", ["n1", "n63", "n65", "n257", "lattice", "lattice_nn128", "mixed_nn1", "mixed_nn30", "mixed_nn100",
                                  "mixed_nn128", "clump"])
def test_hybrid_search_equals_the_restatement_gpu(dev, cnr, name):
    cap = _capacity(cnr)
    p, radius, max_nn = FC.search_cases(cap)[name]
    want_idx, want_d2, want_count = FC.hybrid_search(p, radius, max_nn)
    if name == "clump":
        assert want_count.max() == max_nn and (((p[:, None, :].astype(np.float64) - p[None, :, :]) ** 2).sum(-1) < radius * radius).sum(1).max() > cap
    if name.startswith("mixed") and max_nn > 1:              # an isolated point, one with more than max_nn in range, duplicates
        assert want_count.min() == 1 and (want_count > 1).any() and ((want_d2[:, 1] == 0) & (want_count > 1)).any()
        assert (want_count == max_nn).any() == (max_nn == 30)
        assert (p < 0).any(0).all() and (p > 0).any(0).all()
    idx, d2, count = cnr.utils.hybrid_search(_up(p, dev), radius, max_nn)
    assert np.array_equal(count.cpu().numpy(), want_count)
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    assert np.array_equal(d2.cpu().numpy(), want_d2)
    again = cnr.utils.hybrid_search(_up(p, dev), radius, max_nn)
    assert torch.equal(idx, again[0]) and torch.equal(d2, again[1]) and torch.equal(count, again[2])


@pytest.mark.parametrize("name", ["jitter_300", "surface", "aniso", "sparse"])
def test_normals_equal_the_restatement_gpu(dev, cnr, name):
    """the restatement's lists go in; the angle bound is 10 x what eigh differs from the restatement's own Jacobi by"""
    p, radius, max_nn = FC.normals_cases()[name]
    idx, _, count = FC.hybrid_search(p, radius, max_nn)
    c = FC.centroid(p)
    want, lam = FC.estimate_normals(p, idx, count, c, return_eigen=True)
    got = torch.empty(len(p), 3, device=dev, dtype=torch.float64)
    cnr._C.call("cnr_estimate_normals", _up(p, dev), len(p), _up(idx, dev), _up(count, dev), max_nn, float(c[0]), float(c[1]), float(c[2]), got)
    got = got.cpu().numpy()
    full = count >= 3
    ok = full & (FC.eigen_gap(lam) >= 1e-3)
    assert (full & ~ok).sum() <= 0.05 * len(p)
    assert np.array_equal(got[~full], want[~full])
    ang = FC.angles(got[ok], want[ok])
    print(name, "largest angle to the restatement", ang.max() if ok.any() else None, "bit-equal rows", int((got == want).all(1).sum()), "of", len(p))
    if ok.any():
        assert ang.max() <= 10 * EIGH_VS_JACOBI_ANGLE
        assert ((got[ok] * want[ok]).sum(1) > 0).all()                      # the same side
    d = p.astype(np.float64) - c
    dot = (want[:, 0] * d[:, 0] + want[:, 1] * d[:, 1]) + want[:, 2] * d[:, 2]
    zero = full & (dot == 0)
    if name == "aniso":
        assert zero.sum() >= 3
    assert np.array_equal(got[zero], want[zero])                            # the rule for a dot product of exactly 0
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() < 1e-15
    # ... and through the public surface, with the kernel's own lists
    cloud = cnr.utils.PointCloud(p, device=dev).estimate_normals(radius, max_nn)
    assert cloud.normals.dtype == np.float64 and np.array_equal(cloud.normals, got)
    assert not cloud.voxel_down_sample(0.05).has_normals()


def test_a_dot_product_of_zero_turns_the_largest_component_positive_gpu(dev, cnr):
    """the centroid set to point i itself, so that n.(p_i - c) is exactly 0: rows whose raw eigenvector has a negative largest
    component must be negated, the others left (tests/test_fpfh_host.py shows the restatement does both)"""
    p, radius, max_nn = FC.normals_cases()["jitter_300"]
    idx, _, count = FC.hybrid_search(p, radius, max_nn)
    _, raw = FC.estimate_normals(p, idx, count, return_raw=True)
    negative, positive = FC.tie_rule_rows(raw, count)
    assert len(negative) == 4 and len(positive) == 4
    dp, di, dc = _up(p, dev), _up(idx, dev), _up(count, dev)
    got = torch.empty(len(p), 3, device=dev, dtype=torch.float64)
    for i in negative + positive:
        c = p[i].astype(np.float64)
        cnr._C.call("cnr_estimate_normals", dp, len(p), di, dc, max_nn, float(c[0]), float(c[1]), float(c[2]), got)
        row = got[i].cpu().numpy()
        want = FC.estimate_normals(p, idx, count, c=c)[i]
        assert np.array_equal(want, -raw[i] if i in negative else raw[i])
        assert np.array_equal(row, want), (i, row, want)


@pytest.fixture(scope="module")
def descriptors():
    p, radius, max_nn, sp = FC.descriptor_case()
    idx, d2, count = FC.hybrid_search(p, radius, max_nn)
    nrm = FC.estimate_normals(p, idx, count)
    s = FC.spfh(p, nrm, idx, count)
    return dict(p=p, radius=radius, max_nn=max_nn, sp=sp, idx=idx, d2=d2, count=count, nrm=nrm, spfh=s, fpfh=FC.fpfh(s, idx, d2, count))


def _spfh(cnr, dev, D, nrm=None):
    out = torch.empty(len(D["p"]), 33, device=dev, dtype=torch.float64)
    cnr._C.call("cnr_spfh", _up(D["p"], dev), _up(D["nrm"] if nrm is None else nrm, dev), len(D["p"]), _up(D["idx"], dev), _up(D["count"], dev),
                D["max_nn"], out)
    return out


def _fpfh(cnr, dev, D, spfh):
    out = torch.empty(len(D["p"]), 33, device=dev, dtype=torch.float64)
    cnr._C.call("cnr_fpfh", _up(spfh, dev), len(D["p"]), _up(D["idx"], dev), _up(D["d2"], dev), _up(D["count"], dev), D["max_nn"], out)
    return out


def test_spfh_equals_the_restatement_bit_for_bit_gpu(dev, cnr, descriptors):
    D, sp = descriptors, descriptors["sp"]
    got = _spfh(cnr, dev, D).cpu().numpy()
    bad = np.flatnonzero((got != D["spfh"]).any(1))
    print("rows that differ", bad[:10])
    assert np.array_equal(got, D["spfh"])
    assert not got[sp["isolated"]].any()                                                    # k <= 1
    assert np.array_equal(np.flatnonzero(got[sp["along_a"]]), [5, 16, 27])                  # |v| == 0: the zero feature's bins
    assert got[sp["dup"]][[5, 16, 27]].min() > 0                                            # d == 0: the same bins


def test_fpfh_equals_the_restatement_bit_for_bit_gpu(dev, cnr, descriptors):
    D, sp = descriptors, descriptors["sp"]
    got = _fpfh(cnr, dev, D, D["spfh"]).cpu().numpy()
    diff = np.abs(got - D["fpfh"])
    print("largest difference", diff.max(), "rows that differ", np.flatnonzero((got != D["fpfh"]).any(1))[:10])
    assert np.array_equal(got, D["fpfh"])
    assert not got[sp["isolated"]].any()
    z = D["spfh"].copy()
    z[:, 11:22] = 0.0                                                                       # a group whose weighted sum is 0
    assert np.array_equal(_fpfh(cnr, dev, D, z).cpu().numpy(), FC.fpfh(z, D["idx"], D["d2"], D["count"]))
    # the public function: its own search and normals on the same cloud; the lists are the restatement's (test above)
    cloud = cnr.utils.PointCloud(D["p"], device=dev)
    cloud.normals_device = _up(D["nrm"], dev)
    assert np.array_equal(cnr.category_registration.compute_fpfh_feature(cloud, D["radius"], D["max_nn"]).cpu().numpy(), D["fpfh"])


NN_SHAPES = [(33, 300, 1000), (33, 150, 170), (1, 40, 50), (64, 70, 90), (33, NN_BLOCK - 1, NN_TILE - 1), (33, NN_BLOCK, NN_TILE), (33, NN_BLOCK + 1, NN_TILE + 1),
             (33, 5, 1), (33, 1, 3 * NN_TILE + 5)]


@pytest.mark.parametrize("D,nq,nr", NN_SHAPES)
def test_feature_nn_equals_the_sequential_fp32_sum_gpu(dev, cnr, D, nq, nr):
    rng = np.random.default_rng(1000 * D + nq + nr)
    q, p = (rng.random((nq, D)) * 100).astype(np.float32), (rng.random((nr, D)) * 100).astype(np.float32)
    if nr >= 3:
        p[nr - 1] = p[0] = q[0]                               # duplicated rows: the lowest index wins
    want_i, want_d = FC.feature_nn(q, p)
    index, dist = cnr.category_registration.feature_nn(_up(q, dev), _up(p, dev))
    assert np.array_equal(index.cpu().numpy(), want_i) and np.array_equal(dist.cpu().numpy(), want_d)
    if nr >= 3:
        assert want_i[0] == 0 and want_d[0] == 0


def test_feature_nn_keeps_the_argmin_among_large_values_gpu(dev, cnr):
    """rows of 1e3: |q|^2 + |p|^2 - 2 q.p in fp32 has an ulp of 4 at 3.3e7 and cannot see the 33 x 0.25 between these rows"""
    q = np.full((1, 33), 1000.0, np.float32)
    p = np.concatenate([q + np.float32(0.5), q + np.float32(0.25), q + np.float32(0.25), q - np.float32(0.5)])
    want_i, want_d = FC.feature_nn(q, p)
    assert want_i[0] == 1 and want_d[0] == np.float32(33 * 0.0625)
    index, dist = cnr.category_registration.feature_nn(_up(q, dev), _up(p, dev))
    assert int(index[0]) == 1 and float(dist[0]) == float(want_d[0])


def test_mutual_correspondences_equal_the_restatement_gpu(dev, cnr):
    rng = np.random.default_rng(9)
    f0, f1 = rng.random((150, 33)) * 100, rng.random((170, 33)) * 100
    for mutual in (True, False):
        i0, i1 = cnr.category_registration.mutual_correspondences(_up(f0, dev), _up(f1, dev), mutual_filter=mutual)
        w0, w1 = FC.mutual_correspondences(f0, f1, mutual_filter=mutual)
        assert np.array_equal(i0.cpu().numpy(), w0) and np.array_equal(i1.cpu().numpy(), w1)
    h0, h1 = cnr.teaser_utils.helpers.find_correspondences(f0, f1)
    assert np.array_equal(h0, FC.mutual_correspondences(f0, f1)[0]) and np.array_equal(h1, FC.mutual_correspondences(f0, f1)[1])


# ---- end to end ----------------------------------------------------------------------------------------------------------
# The class is fpfh_cpu.e2e_case(): a plate of gentle bumps, a sibling of teaser_cpu.registration_case.  That case's spaced
# random points have no surface, hence no normals that survive 2 mm of noise, and flat boxes give every point of a face the same
# descriptor; fpfh_cpu.surface says more.
@pytest.fixture(scope="module")
def restated():
    clouds, poses, counts = FC.e2e_case()
    out = {}
    for oid in (12, 13):
        solver = FC.FpfhTeaserSolverCpu(FC.E2E_VOXEL)
        out[oid] = (solver.solve_one(clouds[oid], clouds[11]), solver.last)
    return clouds, poses, counts, out


def _pose_error(T, want):
    rot = float(np.degrees(np.arccos(np.clip((np.trace(T[:3, :3].T @ want[:3, :3]) - 1) / 2, -1, 1))))
    return rot, float(np.linalg.norm(T[:3, 3] - want[:3, 3]))


def test_fpfh_teaser_solver_equals_the_restatement_gpu(dev, cnr, restated):
    clouds, poses, _, ref = restated
    CR = cnr.category_registration
    for oid in (12, 13):
        T_ref, last = ref[oid]
        solver = CR.FpfhTeaserSolver(voxel_size=FC.E2E_VOXEL)
        R, t = solver(_up(clouds[oid].T[None].copy(), dev), _up(clouds[11].T[None].copy(), dev))
        li = solver.last_info
        assert li["n_src"] == last["n_src"] and li["n_tgt"] == last["n_tgt"]
        assert np.array_equal(li["correspondences"], last["pairs"])
        assert li["N"] == len(last["pairs"]) and li["exact"] and np.array_equal(np.sort(li["clique"]), np.sort(last["clique"]))
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R[0].numpy(), t[0].numpy().reshape(3)
        diff = float(np.abs(T - T_ref).max())
        want = poses[11] @ np.linalg.inv(poses[oid])
        rot, tr = _pose_error(T, want)
        print(oid, "largest difference to the restatement's pose", diff, "pose error", rot, tr, "restatement", RESTATEMENT_POSE_ERRORS[oid])
        assert diff <= POSE_TOLERANCE
        assert rot <= 3 * RESTATEMENT_POSE_ERRORS[oid][0] and tr <= 3 * RESTATEMENT_POSE_ERRORS[oid][1]


def test_teaser_fpfh_icp_forward_equals_the_restatement_gpu(dev, cnr, restated, capsys):
    clouds, poses, _, ref = restated
    T_ref, last = ref[12]
    tfi = cnr.teaser_utils.teaser_fpfh_icp
    source = _up(clouds[12].T[None].copy(), dev).float()
    padded = np.concatenate([clouds[11].T, np.zeros((3, 7))], 1)                 # zero padding, which forward drops
    module = tfi.TEASER_FPFH_ICP(source, voxel_size=FC.E2E_VOXEL, spc=False, visualize=True)
    R, t = module.forward(_up(padded[None].copy(), dev).float())
    assert R.shape == (1, 3, 3) and t.shape == (1, 3, 1) and R.device == source.device
    assert "FPFH generates %d putative correspondences." % len(last["pairs"]) in capsys.readouterr().out
    assert module.last_info[0]["candidates"] == len(last["pairs"])
    assert np.array_equal(module.last_info[0]["correspondences"], last["pairs"])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R[0].double().cpu().numpy(), t[0].double().cpu().numpy().reshape(3)
    diff = float(np.abs(T - T_ref.astype(np.float32)).max())      # forward returns float32, as the reference does
    rot, tr = _pose_error(T, poses[11] @ np.linalg.inv(poses[12]))
    print("forward: largest difference to the restatement's pose", diff, "pose error", rot, tr)
    assert diff <= POSE_TOLERANCE
    assert rot <= 3 * RESTATEMENT_POSE_ERRORS[12][0] and tr <= 3 * RESTATEMENT_POSE_ERRORS[12][1]


def test_fpfh_solver_registers_a_class_through_align_poses_gpu(dev, cnr, restated):
    clouds, poses, counts, _ = restated
    CR = cnr.category_registration
    inst, bbox, cnt, pe, fc = RC.build_dicts(clouds, counts, lambda p: cnr.utils.PointCloud(p, device=dev))
    solver = CR.FpfhTeaserSolver(voxel_size=FC.E2E_VOXEL)
    seen = CR.align_poses(inst, bbox, cnt, pe, fc, name="replica", eta1=ETA1, eta2=ETA2, eta3=ETA3, device=str(dev), solver=solver)
    print("chamfer", seen["chamfer"])
    assert list(inst.keys()) == [7, 107] and list(inst[107].keys()) == [15] and list(inst[7].keys()) == [11, 12, 13]
    errs = RC.pose_errors(inst, poses)
    print("pose errors (degrees, metres)", errs)
    for oid, (rot, tr) in errs.items():
        assert rot <= 3 * RESTATEMENT_CLASS_ERRORS[oid][0] and tr <= 3 * RESTATEMENT_CLASS_ERRORS[oid][1], (oid, rot, tr)


def test_bad_solver_arguments_are_value_errors_gpu(dev, cnr):
    """(mutual nearest neighbours of two non-empty sets always hold the closest pair, so the solver's own "no correspondence" error
    needs an empty cloud, which the down-sampling refuses first)"""
    pts = FC.surface(51)[:50]
    with pytest.raises(ValueError, match="max_correspondences"):
        cnr.category_registration.FpfhTeaserSolver(voxel_size=0.02, max_correspondences=0).solve_one(pts, pts, dev)
    with pytest.raises(ValueError):
        cnr.category_registration.FpfhTeaserSolver(voxel_size=0.02).solve_one(np.zeros((0, 3)), pts, dev)
    with pytest.raises(ValueError, match="no normals"):
        cnr.category_registration.compute_fpfh_feature(cnr.utils.PointCloud(pts, device=dev), 0.1, 100)
