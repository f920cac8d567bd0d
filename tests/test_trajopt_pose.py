"""kin_traj_opt_pose_batch without a device: the CPU restatement (tests/trajopt_pose_ref.py) converges on the
prototype family, its residual / Jacobian / step agree with finite differences and with the linearised constraint,
its own forward / reversed-summation spread (the GPU tests' 8-iteration bound), and the host checks of the new ABI."""
import ctypes as C

import numpy as np
import pytest
import torch

import kinhip
import trajopt_pose_ref as PR
import trajopt_ref as R
from conftest import ARM, golden
from kinhip import _lib as K

P = R.PARAMS
# Measured here (test_spread_of_the_restatement): the restatement against itself with every sum of trajopt_ref taken
# in reverse order, after 8 iterations, over the 16 first-iterate cases of tests/test_gpu_trajopt_pose.py:
# max |X - X_rev| = 9.2e-13, max |merit - merit_rev| = 1.67e-12; the larger one is taken for both.  10 x that is the GPU
# test's bound after 8 iterations (the rule of SPREAD8 in tests/test_gpu_trajopt.py; never taken from the kernel).
SPREAD8_POSE = 1.7e-12


@pytest.mark.parametrize("n_wp,rows", PR.CASES)
def test_convergence_floor(n_wp, rows):
    """The prototype family (Fetch, 32 goals, c = n_wp // 2, IK-seeded two-line guesses): at least 24 of 32 end good
    (|r_p|, |r_rot| < 1e-3, clearance >= margin - feas) within 200 iterations; the merit never increases.  The floor
    keeps the GPU comparison from being vacuous; it is not a tuning target.  Measured: 32, 28, 32 good for
    (10, 3), (10, 6), (33, 6)."""
    out = PR.full_run(n_wp, rows)
    ok = PR.good(out, P["margin"], P["feas"])
    done = out["iters"] <= P["max_iters"]
    print(f"n_wp = {n_wp}, rows = {rows}: good {int(ok.sum())}/32, done {int(done.sum())}/32, "
          f"max |r_p| {out['info'][4].max():.2e}, max |r_rot| {out['info'][5].max():.2e}")
    assert np.all(np.diff(out["merits"], axis=0) <= 0.0)
    assert np.all(ok[done])
    assert ok.sum() >= 24


def _fd_case(rows, n=6, shift=1.0):
    sc, link, c, wr, tg, X0 = PR.fetch_problem(10, rows)
    rng = np.random.default_rng(3)
    Q = np.ascontiguousarray(X0[:n, c].T + shift * rng.normal(0, 0.02, (sc.n_dof, n)))
    return sc, link, wr, tg[:, :n], Q


@pytest.mark.parametrize("rows", [3, 6])
def test_jacobian_is_the_derivative_of_the_residual(rows):
    """Forward differences, step 1e-6, bound 1e-5 (the project's forward-difference agreement): the position rows
    anywhere, the rotation rows where |r_rot| < 1e-3 (J is the derivative of -log(R* R^T) to first order in it)."""
    for shift, rot in ((1.0, False), (0.0, True)):
        sc, link, wr, tg, Q = _fd_case(rows, n=32 if rot else 6, shift=shift)
        r0, J = PR.residual(sc, link, Q, tg, wr)
        if rot:   # the IK answers that converged: |r_rot| ~ 1e-6 (the first-order term is |r_rot| |J| / 2)
            keep = np.nonzero(PR.norms(r0)[1] < 2e-6)[0][:6]
            assert keep.size == 6
            tg, Q, r0, J = tg[:, keep], np.ascontiguousarray(Q[:, keep]), r0[keep], J[keep]
            assert PR.norms(r0)[1].max() < 1e-3
        k = r0.shape[1] if rot else 3
        for d in range(sc.n_dof):
            Qd = Q.copy()
            Qd[d] += 1e-6
            fd = (PR.residual(sc, link, Qd, tg, wr)[0] - r0) / 1e-6
            assert np.abs(fd[:, :k] - J[:, :k, d]).max() < 1e-5, (d, rot)


@pytest.mark.parametrize("rows", [3, 6])
def test_step_meets_the_linearised_constraint(rows):
    """damp = 0, no clamp or scaling: J step_c = -r to 1e-6 |r|, for any raw step."""
    sc, link, wr, tg, Q = _fd_case(rows)
    n_wp, c = 10, 5
    r, J = PR.residual(sc, link, Q, tg, wr)
    rng = np.random.default_rng(4)
    raw = rng.normal(0, 0.05, (Q.shape[1], n_wp - 2, sc.n_dof))
    w = rng.uniform(0.5, 2.0, sc.n_dof)
    step = PR.projected_step(raw, R.metric_inverse(n_wp), c, r, J, 1.0 / (w * w), 0.0)
    lhs = np.einsum("tkd,td->tk", J, step[:, c - 1])
    assert np.all(np.abs(lhs + r).max(1) <= 1e-6 * np.sqrt((r * r).sum(1)))
    # away from c the correction follows the metric's column
    m = R.metric_inverse(n_wp)[:, c - 1]
    u = step[:, c - 1] - raw[:, c - 1]
    np.testing.assert_allclose(step - raw, (m / m[c - 1])[None, :, None] * u[:, None, :], atol=1e-15)


def test_rot_log_matches_the_oracle():
    """rot_log is the oracle's rot_error (the DLS IK's rotation residual), a rotation by ~pi included."""
    import oracle as O
    rng = np.random.default_rng(5)
    rpys = list(rng.uniform(-3, 3, (20, 3))) + [np.array([np.pi - 1e-9, 0, 0]), np.array([0, 0, np.pi])]
    for a in rpys:
        Ta, Tb = np.eye(4), np.eye(4)
        Ta[:3, :3] = O.rpy_to_matrix(a)
        Tb[:3, :3] = O.rpy_to_matrix(rng.uniform(-0.1, 0.1, 3))
        w = PR.rot_log(Ta[None, :3, :3], Tb[None, :3, :3])[0]
        np.testing.assert_allclose(w, O.rot_error(Ta, Tb), atol=1e-12)


def test_spread_of_the_restatement():
    """The restatement's forward / reversed-summation spread after 8 iterations over the GPU first-iterate cases
    stays within SPREAD8_POSE (the figure the GPU bound is derived from)."""
    worst = [0.0, 0.0]
    for b, rows, shape in PR.FIRST_CASES:
        f, r = PR.first_run(b, rows, shape, 8), PR.first_run(b, rows, shape, 8, rev=True)
        worst[0] = max(worst[0], np.abs(f["X"] - r["X"]).max())
        worst[1] = max(worst[1], np.abs(f["info"][0] - r["info"][0]).max())
    print(f"fwd / rev spread after 8 iterations: max |dX| = {worst[0]:.2e}, max |d merit| = {worst[1]:.2e}")
    assert max(worst) <= SPREAD8_POSE


# ------------------------------------------------------------------------------------------------ the ABI on the host
def _prm(**kw):
    d = dict(n_wp=10, max_iters=5, margin=0.02, band=0.03, weight=10.0, feas=1e-3, ftol=1e-6, max_step=0.5)
    d.update(kw)
    return K.TrajParams(d["n_wp"], d["max_iters"], d["margin"], d["band"], d["weight"], d["feas"], d["ftol"],
                        d["max_step"], None)


def _pose(wp=5, with_rot=1, n_con=1, weight=10.0, damp=1e-6, tol_pos=1e-3, tol_rot=1e-3):
    a, b = (C.c_int32 * 1)(wp), (C.c_int32 * 1)(with_rot)
    pp = K.TrajPoseParams(n_con, C.cast(a, C.c_void_p), C.cast(b, C.c_void_p), weight, damp, tol_pos, tol_rot)
    pp._keep = (a, b)
    return pp


@pytest.mark.parametrize("kw,code,word", [
    (dict(n_con=2), K.KIN_E_UNSUPPORTED, b"n_con"),
    (dict(n_con=0), K.KIN_E_UNSUPPORTED, b"n_con"),
    (dict(wp=0), K.KIN_E_INVALID, b"interior"),
    (dict(wp=9), K.KIN_E_INVALID, b"interior"),
    (dict(wp=-1), K.KIN_E_INVALID, b"interior"),
    (dict(with_rot=2), K.KIN_E_INVALID, b"with_rot"),
    (dict(weight=0.0), K.KIN_E_INVALID, b"pose weight"),
    (dict(weight=float("nan")), K.KIN_E_INVALID, b"pose weight"),
    (dict(weight=float("inf")), K.KIN_E_INVALID, b"pose weight"),
    (dict(tol_pos=0.0), K.KIN_E_INVALID, b"tol_pos"),
    (dict(tol_rot=-1.0), K.KIN_E_INVALID, b"tol_rot"),
    (dict(tol_rot=float("nan")), K.KIN_E_INVALID, b"tol_rot"),
    (dict(damp=-1e-9), K.KIN_E_INVALID, b"damp"),
    (dict(damp=float("inf")), K.KIN_E_INVALID, b"damp"),
])
def test_pose_parameter_checks_before_device(kw, code, word):
    """Every limit of kin_traj_pose_params is refused on the host with a message naming the entry point, before the
    plan is looked at; so are kin_traj_opt_batch's own limits, ldt < n_traj and null blocks."""
    L = K.lib()
    tg = np.zeros((12, 4))
    call = lambda prm, pp, ldt=4, n=4: L.kin_traj_opt_pose_batch(
        None, None, C.byref(prm) if prm else None, C.byref(pp) if pp else None, tg.ctypes.data, ldt, None, 0, n, None,
        None, 0, None)
    assert call(_prm(), _pose(**kw)) == code
    assert word in L.kin_last_error() and b"kin_traj_opt_pose_batch" in L.kin_last_error()
    assert call(_prm(), _pose()) == K.KIN_E_INVALID and b"null plan" in L.kin_last_error()
    assert call(_prm(), _pose(), ldt=3) == K.KIN_E_INVALID and b"ldt" in L.kin_last_error()
    assert call(_prm(), None) == K.KIN_E_INVALID and b"null pose parameters" in L.kin_last_error()
    assert call(None, _pose()) == K.KIN_E_INVALID
    assert call(_prm(n_wp=65), _pose()) == K.KIN_E_UNSUPPORTED and b"n_wp" in L.kin_last_error()
    assert call(_prm(ftol=0.0), _pose()) == K.KIN_E_INVALID and b"ftol" in L.kin_last_error()
    assert call(_prm(n_wp=3), _pose(wp=1)) == K.KIN_E_INVALID and b"null plan" in L.kin_last_error()


def _fetch(extra_joints=()):
    m = kinhip.parse_urdf(golden("fetch.urdf"))
    joints = [m.find_joint(n) for n in list(ARM) + list(extra_joints)]
    sscc = kinhip.SweptSphereCollisionChecker(m)
    for n in R.COLL_LINKS:
        kinhip.add_coll_links(sscc, m.find_link(n))
    return m, joints, sscc


def _serial_urdf(n):
    out = ['<robot name="serial">'] + [f'  <link name="l{k}"/>' for k in range(n + 1)]
    for k in range(n):
        out.append(f'  <joint name="j{k}" type="revolute"><parent link="l{k}"/><child link="l{k + 1}"/>'
                   f'<origin xyz="0.1 0 0.05" rpy="0 0 0"/><axis xyz="{"0 0 1" if k % 2 == 0 else "0 1 0"}"/>'
                   '<limit lower="-2" upper="2" effort="1" velocity="1"/></joint>')
    return "\n".join(out + ["</robot>"])


def test_traj_plan_create_refusals(tmp_path):
    """Refused while staging, on the host: a pose link on another branch, more than 2 pose links, no pose link, a
    chain of more than 8 steps -- by its spheres or only by the extension to the pose link."""
    m, joints, sscc = _fetch(["head_pan_joint"])
    with pytest.raises(K.KinError, match="another branch") as e:
        sscc.traj_plan(joints, [m.find_link("head_pan_link")])
    assert e.value.code == K.KIN_E_UNSUPPORTED
    gl = m.find_link("gripper_link")
    with pytest.raises(K.KinError, match="more than 2 pose links") as e:
        sscc.traj_plan(joints, [gl, m.find_link("wrist_roll_link"), m.find_link("wrist_flex_link")])
    assert e.value.code == K.KIN_E_UNSUPPORTED
    with pytest.raises(K.KinError, match="pose link") as e:
        sscc.traj_plan(joints, [])
    assert e.value.code == K.KIN_E_INVALID
    p = tmp_path / "serial.urdf"
    p.write_text(_serial_urdf(9))
    ms = kinhip.parse_urdf(str(p))
    js = [ms.find_joint(f"j{k}") for k in range(9)]
    for sphere_link in ("l4", "l9"):
        s2 = kinhip.SweptSphereCollisionChecker(ms)
        s2.add_coll_sphere(ms.find_link(sphere_link), [0.02, 0, 0], 0.05)
        with pytest.raises(K.KinError, match="more than 8 steps") as e:
            s2.traj_plan(js, [ms.find_link("l9")])
        assert e.value.code == K.KIN_E_UNSUPPORTED


def test_fetch_gripper_plan_is_staged_at_bound_8():
    """Fetch's gripper_link lies below wrist_roll_joint, past the deepest collision link: the extended chain has 8
    steps.  Staging is host work; the plan itself needs a device for its tables, so without one the call gets as far
    as the upload (KIN_E_DEVICE, after every staging refusal) and with one kin_plan_chain_bound is 8."""
    m, joints, sscc = _fetch()
    gl = m.find_link("gripper_link")
    if torch.cuda.is_available():
        assert sscc.traj_plan(joints, [gl]).chain_bound == 8
        assert sscc.traj_plan(joints, [gl, m.find_link("elbow_flex_link")]).chain_bound == 8
    else:
        with pytest.raises(K.KinError) as e:
            sscc.traj_plan(joints, [gl])
        assert e.value.code == K.KIN_E_DEVICE


def test_plan_trajectory_gpu_solver_refuses_other_partial_constraints():
    """Before sscc is touched: two constraints, a ConfigurationConstraint, a PoseConstraint look-alike with two
    links, an end waypoint."""
    class Two(kinhip.PoseConstraint):
        def __init__(self, idx_wp, n_links):
            self.idx_wp, self.move_links, self.target_poses, self.with_rots = idx_wp, [None] * n_links, [np.eye(4)], [True]

    cc = kinhip.ConfigurationConstraint(5, 8, np.zeros(8))
    for pcs in ([Two(5, 1), Two(6, 1)], [cc], [Two(5, 2)], [Two(1, 1)], [Two(10, 1)]):
        with pytest.raises(ValueError):
            kinhip.plan_trajectory(None, [], None, [], [], 10, solver="GPU", partial_consts=pcs)
