"""kin_traj_opt_batch without a GPU: the metric table, the argument checks that precede any device work, and the
algorithm's CPU restatement (tests/trajopt_ref.py) on the reference's planning scene."""
import ctypes as C

import numpy as np
import pytest

import kinhip
import trajopt_ref as R
from kinhip import _lib as K


@pytest.mark.parametrize("n_wp", [3, 4, 10, 64])
def test_metric_inverse(n_wp):
    """kin_traj_metric_inverse = inv of the interior block of Objective(n_wp, ones).A, to 1e-10 of the identity.
    Against numpy's own inverse the bound is relative: both carry cond(A_II) eps (cond ~ 1e6 at n_wp = 64)."""
    A = kinhip.Objective(n_wp, np.ones(1)).A.toarray()
    AII = A[1:-1, 1:-1]
    M = kinhip.traj_metric_inverse(n_wp)
    assert M.shape == (n_wp - 2, n_wp - 2)
    ref = np.linalg.inv(AII)
    np.testing.assert_allclose(M, ref, rtol=0, atol=1e-9 * np.abs(ref).max())
    assert np.abs(M @ AII - np.eye(n_wp - 2)).max() < 1e-10
    assert np.array_equal(M, M.T)


def test_metric_inverse_limits():
    out = np.zeros(64 * 64)
    L = K.lib()
    for n_wp in (2, 0, -1, 65):
        assert L.kin_traj_metric_inverse(n_wp, out.ctypes.data) == K.KIN_E_UNSUPPORTED
        assert b"n_wp" in L.kin_last_error()
    assert L.kin_traj_metric_inverse(10, None) == K.KIN_E_INVALID


def _prm(**kw):
    d = dict(n_wp=10, max_iters=200, margin=0.02, band=0.03, weight=10.0, feas=1e-3, ftol=1e-6, max_step=0.5,
             dof_weights=None)
    d.update(kw)
    return K.TrajParams(*[d[k] for k, _ in K.TrajParams._fields_])


@pytest.mark.parametrize("kw,code,word", [
    (dict(n_wp=2), K.KIN_E_UNSUPPORTED, b"n_wp"),
    (dict(n_wp=65), K.KIN_E_UNSUPPORTED, b"n_wp"),
    (dict(max_iters=0), K.KIN_E_INVALID, b"max_iters"),
    (dict(weight=0.0), K.KIN_E_INVALID, b"weight"),
    (dict(weight=float("inf")), K.KIN_E_INVALID, b"weight"),
    (dict(weight=float("nan")), K.KIN_E_INVALID, b"weight"),
    (dict(max_step=-1.0), K.KIN_E_INVALID, b"max_step"),
    (dict(max_step=float("nan")), K.KIN_E_INVALID, b"max_step"),
    (dict(ftol=0.0), K.KIN_E_INVALID, b"ftol"),
    (dict(ftol=float("inf")), K.KIN_E_INVALID, b"ftol"),
    (dict(margin=float("nan")), K.KIN_E_INVALID, b"margin"),
    (dict(band=-0.1), K.KIN_E_INVALID, b"band"),
    (dict(feas=-1.0), K.KIN_E_INVALID, b"feas"),
])
def test_parameter_checks_before_device(kw, code, word):
    """Every parameter limit is refused on the host with a message, before the plan is looked at (so without a
    device); a null plan / sdf / parameter block is KIN_E_INVALID."""
    L = K.lib()
    prm = _prm(**kw)
    assert L.kin_traj_opt_batch(None, None, C.byref(prm), None, 0, 1, None, None, 0, None) == code
    assert word in L.kin_last_error()
    good = _prm()
    assert L.kin_traj_opt_batch(None, None, C.byref(good), None, 0, 1, None, None, 0, None) == K.KIN_E_INVALID
    assert b"null plan" in L.kin_last_error()
    assert L.kin_traj_opt_batch(None, None, None, None, 0, 1, None, None, 0, None) == K.KIN_E_INVALID


def test_plan_trajectory_gpu_solver_keeps_the_refusals():
    for solver in ("NLOPT", ":IPOPT", "bogus"):
        with pytest.raises(ValueError):
            kinhip.plan_trajectory(None, [], None, [], [], 10, solver=solver)
    with pytest.raises(ValueError):
        kinhip.plan_trajectory(None, [], None, [], [], 10, solver="GPU", partial_consts=[object()])


def test_union_box_sdf_matches_the_oracle():
    """The numpy box SDF of the restatement: values equal the oracle's UnionSDF, the analytic gradient its forward
    difference to O(eps) away from the kinks."""
    import oracle as O
    rng = np.random.default_rng(1)
    poses = [R._T(R.BOX_POSE), np.eye(4)]
    poses[1][:3, :3] = O.rpy_to_matrix([0.3, -0.2, 0.5])
    poses[1][:3, 3] = [0.1, 0.2, 0.3]
    widths = [R.BOX_WIDTH, (0.3, 0.2, 0.1)]
    sdf = O.OracleUnionSDF(poses, widths)
    p = rng.uniform(-0.3, 0.8, (400, 3))
    d, g = R.union_box_sdf(p, poses, widths)
    dref = np.array([sdf(x) for x in p])
    np.testing.assert_allclose(d, dref, atol=1e-14)
    gref = np.array([sdf.gradient(x) for x in p])
    assert (np.abs(g - gref).max(1) < 1e-5).mean() > 0.99
    np.testing.assert_allclose(np.linalg.norm(g, axis=1), 1.0, atol=1e-12)


@pytest.mark.parametrize("n_wp,with_base", [(3, False), (10, False), (10, True), (16, False), (33, False), (64, False)])
def test_restatement_on_the_planning_scene(n_wp, with_base):
    """The algorithm alone on Fetch + the thin box, 32 goals, 200 iterations: the merit never increases, every goal
    lies inside the joint limits, the end waypoints stay, and for n_wp in {3, 10, 16} all 32 end feasible
    (min interior distance >= margin - feas).  (33 and 64 are not asserted feasible: the penalty and smoothness
    scales do not follow n_wp.)"""
    sc = R.scene(with_base)
    assert np.all(sc.q_goals >= sc.lo[:, None]) and np.all(sc.q_goals <= sc.hi[:, None])
    out = R.full_run(n_wp, with_base)
    m = out["merits"]
    assert np.all(m[1:] <= m[:-1])
    assert np.array_equal(out["X"][:, 0], out["X0"][:, 0]) and np.array_equal(out["X"][:, -1], out["X0"][:, -1])
    X = out["X"][:, 1:-1]
    assert np.all(X >= sc.lo) and np.all(X <= sc.hi)
    feasible = out["info"][2] >= R.PARAMS["margin"] - R.PARAMS["feas"]
    started_infeasible = int((out["d0"] < R.PARAMS["margin"] - R.PARAMS["feas"]).sum())
    print(f"n_wp={n_wp} base={with_base}: straight lines infeasible {started_infeasible}/32, "
          f"end feasible {int(feasible.sum())}/32, done {int((out['iters'] <= 200).sum())}/32")
    assert started_infeasible > 0
    if n_wp in (3, 10, 16):
        assert feasible.all()
