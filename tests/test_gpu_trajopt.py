"""kin_traj_opt_batch (k_traj) on the GPU against its CPU restatement (tests/trajopt_ref.py), on the reference's
planning scene: first iterates in fp64, full runs, fp32, packing independence, graph capture, the Python layer."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import trajopt_ref as R
from conftest import ARM, golden

pytestmark = pytest.mark.gpu

P = R.PARAMS
FEAS_D = P["margin"] - P["feas"]
TOL1 = 1e-9      # the project's fp64 constraint tolerance (tests/test_planning.py:91)
# Measured: the restatement against itself with every sum taken in reverse order, after 8 iterations, over all the
# cases of test_first_iterates: max |X - X_rev| = 1.3e-11, max |merit - merit_rev| = 6.9e-11 (n_wp = 64, 67
# trajectories; the larger one is taken for both).  10x that spread is the bound for the kernel after 8
# iterations (the kernel measured: max |dX| = 4.6e-11, max |d merit| = 3.1e-10, same case).
SPREAD8 = 6.9e-11
TOL8 = 10 * SPREAD8


def _T(t):
    T = np.eye(4)
    T[:3, 3] = t
    return T


@functools.lru_cache(maxsize=None)
def _setup(with_base):
    import kinhip
    m = kinhip.parse_urdf(golden("fetch.urdf"), with_base=with_base)
    joints = [m.find_joint(n) for n in ARM]
    sscc = kinhip.SweptSphereCollisionChecker(m)
    for n in R.COLL_LINKS:
        kinhip.add_coll_links(sscc, m.find_link(n))
    sdf = kinhip.UnionSDF([kinhip.BoxSDF(_T(R.BOX_POSE), R.BOX_WIDTH)])
    return m, joints, sscc, sdf


@functools.lru_cache(maxsize=None)
def _plan(with_base, dtype):
    m, joints, sscc, sdf = _setup(with_base)
    return sscc.plan(joints, dtype=dtype)


def _gpu_run(with_base, X0, max_iters, dtype=torch.float64, **over):
    """X0 [nt, n_wp, nd] (numpy) -> X [nt, n_wp, nd], iters, info (numpy, fp64)."""
    import kinhip
    _, _, _, sdf = _setup(with_base)
    prm = dict(P, max_iters=max_iters)
    prm.update(over)
    n_wp = X0.shape[1]
    X = torch.tensor(R.to_columns(X0), dtype=dtype, device="cuda")
    it, nf = kinhip.traj_opt_batch(_plan(with_base, dtype), sdf, X, n_wp, **prm)
    torch.cuda.synchronize()
    return R.from_columns(X.double().cpu().numpy(), n_wp), it.cpu().numpy(), nf.double().cpu().numpy()


def _problems(with_base, n_wp, n_traj):
    """n_traj initial guesses: the straight lines to the 32 goals, then the same lines with a smooth seeded bump."""
    sc = R.scene(with_base)
    X = R.straight_lines(sc.q_start, sc.q_goals[:, np.arange(n_traj) % R.N_GOALS], n_wp)
    rng = np.random.default_rng(7)
    bump = np.sin(np.pi * np.arange(n_wp) / (n_wp - 1))[None, :, None] * rng.normal(0, 0.05, (n_traj, 1, sc.n_dof))
    bump[:R.N_GOALS] = 0.0
    X[:, 1:-1] = np.clip(X[:, 1:-1] + bump[:, 1:-1], sc.lo, sc.hi)
    return sc, X


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("n_traj", [1, 5, 67])
@pytest.mark.parametrize("n_wp", [3, 10, 16, 33, 64])
def test_first_iterates(n_wp, n_traj, with_base):
    """fp64, max_iters = 1 and 8 (a partial segment, a partial wave, several workgroups, L = 8 / 16 / 64): after
    one iteration the trajectory, info and the accept / reject outcome equal the restatement's to 1e-9; after 8 the
    accept sequences are equal and trajectory and merit agree to TOL8 = 10 x the restatement's own spread under
    reversed summation (measured 6.9e-11, see SPREAD8).  Accept / reject outcomes and iteration counts are compared
    for the trajectories whose decisions the restatement marks as determined (trajopt_ref.run: a collision-free
    straight line has a merit of rounding noise, and its outcomes differ between the restatement's own two
    summation orders); trajectories, merits and distances are compared for all."""
    sc, X0 = _problems(with_base, n_wp, n_traj)
    kw = {k: v for k, v in P.items() if k != "max_iters"}
    ref1 = R.run(sc, X0, max_iters=1, **kw)
    X, it, nf = _gpu_run(with_base, X0, 1)
    e1 = (np.abs(X - ref1["X"]).max(), np.abs(nf[:3] - ref1["info"][:3]).max())
    print(f"1 iteration: max|dX| = {e1[0]:.2e}, max|d info| = {e1[1]:.2e}")
    det = ref1["determined"]
    print(f"determined after 1 iteration: {int(det.sum())}/{n_traj}")
    assert np.array_equal(nf[3][det], ref1["info"][3][det]) and np.array_equal(it[det], ref1["iters"][det])
    assert e1[0] <= TOL1 and e1[1] <= TOL1
    ref8 = R.run(sc, X0, max_iters=8, **kw)
    rev8 = R.run(sc, X0, max_iters=8, rev=True, **kw)
    spread = max(np.abs(ref8["X"] - rev8["X"]).max(), np.abs(ref8["info"][0] - rev8["info"][0]).max())
    nacc = [np.zeros(n_traj)]
    for k in range(1, 9):
        X, it, nf = _gpu_run(with_base, X0, k)
        nacc.append(nf[3])
    seq = np.diff(np.array(nacc), axis=0)                                  # [8, nt]: 1 accepted, 0 not
    ref_seq = np.maximum(ref8["accepts"], 0)
    ref_seq = np.vstack([ref_seq, np.zeros((8 - ref_seq.shape[0], n_traj))])
    e8 = (np.abs(X - ref8["X"]).max(), np.abs(nf[0] - ref8["info"][0]).max())
    print(f"8 iterations: max|dX| = {e8[0]:.2e}, max|d merit| = {e8[1]:.2e}, restatement fwd/rev spread {spread:.2e}")
    det = ref8["determined"]
    print(f"determined after 8 iterations: {int(det.sum())}/{n_traj}")
    assert n_traj < 67 or det.sum() >= 8   # (not vacuous: the lines through the box are determined)
    assert np.array_equal(seq[:, det], ref_seq[:, det])
    assert np.array_equal(it[det], ref8["iters"][det])
    assert e8[0] <= TOL8 and e8[1] <= TOL8


def _interior_min(with_base, X, n_wp):
    """min sphere distance over the interior waypoints per trajectory, by kin_coll_batch in fp64."""
    _, _, _, sdf = _setup(with_base)
    Q = torch.tensor(R.to_columns(X), dtype=torch.float64, device="cuda")
    _, _, mn = _plan(with_base, torch.float64).run(sdf, Q, dists=False, min_dist=True)
    return mn.cpu().numpy().reshape(-1, n_wp)[:, 1:-1].min(1)


@pytest.mark.parametrize("n_wp", [3, 10, 16, 33, 64])
def test_full_runs_fp64(n_wp):
    """200 iterations on the 32-goal set: end waypoints bit-equal to the inputs, interior waypoints within the joint
    limits, info[2] = the re-evaluated minimum distance to 1e-9; every trajectory feasible for n_wp in {3, 10, 16};
    for 33 and 64 the feasible set equals the restatement's except for trajectories whose restatement clearance is
    within 1e-6 of margin - feas (at most 2)."""
    sc = R.scene(False)
    ref = R.full_run(n_wp)
    X, it, nf = _gpu_run(False, ref["X0"], P["max_iters"])
    assert np.array_equal(X[:, 0], ref["X0"][:, 0]) and np.array_equal(X[:, -1], ref["X0"][:, -1])
    assert np.all(X[:, 1:-1] >= sc.lo) and np.all(X[:, 1:-1] <= sc.hi)
    dm = _interior_min(False, X, n_wp)
    assert np.abs(nf[2] - dm).max() <= 1e-9
    feasible = dm >= FEAS_D
    assert np.all(it[it <= P["max_iters"]] >= 1) and np.all(feasible[it <= P["max_iters"]])
    print(f"n_wp = {n_wp}: feasible {int(feasible.sum())}/32, done {int((it <= P['max_iters']).sum())}/32")
    if n_wp in (3, 10, 16):
        assert feasible.all()
    else:
        ref_d = ref["info"][2]
        near = np.abs(ref_d - FEAS_D) < 1e-6
        print(f"trajectories within 1e-6 of the threshold in the restatement: {int(near.sum())}")
        assert near.sum() <= 2
        assert np.array_equal(feasible[~near], (ref_d >= FEAS_D)[~near])


@pytest.mark.parametrize("n_wp", [10, 16])
def test_fp32(n_wp):
    """fp32 on the same set: every trajectory feasible when re-evaluated in fp64, the slack feas + 1e-6 (the fp32
    distance bound of tests/test_gpu_coll_fp32_gate.py); the merit does not increase over runs of 1, 2, 4, 8
    iterations."""
    ref = R.full_run(n_wp)
    X, it, nf = _gpu_run(False, ref["X0"], P["max_iters"], dtype=torch.float32)
    dm = _interior_min(False, X, n_wp)
    print(f"fp32 n_wp = {n_wp}: min clearance {dm.min():.6f}, done {int((it <= P['max_iters']).sum())}/32")
    assert np.all(dm >= FEAS_D - 1e-6)
    X32 = torch.tensor(R.to_columns(ref["X0"]), dtype=torch.float32)
    assert np.array_equal(X[:, 0], R.from_columns(X32.double().numpy(), n_wp)[:, 0])
    last = None
    for k in (1, 2, 4, 8):
        _, _, nk = _gpu_run(False, ref["X0"], k, dtype=torch.float32)
        if last is not None:
            assert np.all(nk[0] <= last)
        assert np.all(nk[3] <= k)
        last = nk[0]


@pytest.mark.parametrize("n_wp", [10, 33])
def test_independence_and_packing(n_wp):
    """Trajectory t of a 67-batch is bit-equal to the same trajectory run alone and in another segment position; a
    trajectory that finishes early stays as it was while its wave goes on (its result equals the run that stops at
    its own iteration count); re-running a finished trajectory from its output does not raise its merit."""
    sc, X0 = _problems(False, n_wp, 67)
    X, it, nf = _gpu_run(False, X0, 40)
    for t in (0, 5, 31, 66):
        Xa, ia, na = _gpu_run(False, X0[t:t + 1], 40)
        assert np.array_equal(Xa[0], X[t]) and ia[0] == it[t] and np.array_equal(na[:, 0], nf[:, t])
        Xb, ib, nb = _gpu_run(False, X0[[1, 2, t, 3]], 40)   # another lane position within the wave
        assert np.array_equal(Xb[2], X[t]) and ib[2] == it[t] and np.array_equal(nb[:, 2], nf[:, t])
    done = np.nonzero(it <= 40)[0]
    assert done.size > 0 and done.size < 67   # finished and unfinished trajectories share waves
    t = int(done[np.argmin(it[done])])
    Xs, is_, ns = _gpu_run(False, X0[t:t + 1], int(it[t]))
    assert np.array_equal(Xs[0], X[t]) and is_[0] == it[t] and np.array_equal(ns[:, 0], nf[:, t])
    Xr, ir, nr = _gpu_run(False, X[t:t + 1], 1)
    assert nr[0, 0] <= nf[0, t] and nf[0, t] - nr[0, 0] < P["ftol"]
    assert np.abs(Xr[0] - X[t]).max() < 1e-2


def test_capture():
    """After the plan's first (staging) call for an n_wp, a call captured in a graph replays the eager results."""
    import kinhip
    _, _, _, sdf = _setup(False)
    plan = _plan(False, torch.float64)
    ref = R.full_run(10)
    X0 = torch.tensor(R.to_columns(ref["X0"]), dtype=torch.float64, device="cuda")
    Xe = X0.clone()
    ite, nfe = kinhip.traj_opt_batch(plan, sdf, Xe, 10, **P)   # eager; also stages the table before the capture
    torch.cuda.synchronize()
    dev = X0.device
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    Xg = X0.clone()
    itg = torch.empty_like(ite)
    nfg = torch.empty_like(nfe)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            Xg.copy_(X0)
            kinhip.traj_opt_batch(plan, sdf, Xg, 10, iters=itg, info=nfg, stream=s, **P)
        for rep in range(2):
            g.replay()
            s.synchronize()
            assert torch.equal(Xg, Xe) and torch.equal(itg, ite) and torch.equal(nfg, nfe), rep


def test_limits_on_the_device():
    """The limits that need a plan: spheres on several chains, an attached scene, short arrays."""
    import kinhip
    from kinhip import _lib as K
    m, joints, sscc, sdf = _setup(False)
    prm = K.TrajParams(10, 5, 0.02, 0.03, 10.0, 1e-3, 1e-6, 0.5, None)
    X = torch.zeros((8, 20), dtype=torch.float64, device="cuda")
    L = K.lib()
    plan = _plan(False, torch.float64)
    assert L.kin_traj_opt_batch(plan._h, sdf._h, C.byref(prm), X.data_ptr(), 19, 2, None, None, 0, None) == K.KIN_E_INVALID
    assert b"ldx" in L.kin_last_error()
    nf = torch.zeros((4, 1), dtype=torch.float64, device="cuda")
    assert L.kin_traj_opt_batch(plan._h, sdf._h, C.byref(prm), X.data_ptr(), 20, 2, None, nf.data_ptr(), 1, None) \
        == K.KIN_E_INVALID
    # spheres on the arm and on the head: two chains
    m2 = kinhip.parse_urdf(golden("fetch.urdf"))
    j2 = [m2.find_joint(n) for n in ARM] + [m2.find_joint("head_pan_joint")]
    s2 = kinhip.SweptSphereCollisionChecker(m2)
    s2.add_coll_sphere(m2.find_link("wrist_flex_link"), [0, 0, 0], 0.05)
    s2.add_coll_sphere(m2.find_link("head_pan_link"), [0, 0, 0], 0.05)
    p2 = s2.plan(j2, dtype=torch.float64)
    X2 = torch.zeros((9, 20), dtype=torch.float64, device="cuda")
    assert L.kin_traj_opt_batch(p2._h, sdf._h, C.byref(prm), X2.data_ptr(), 20, 2, None, None, 0, None) \
        == K.KIN_E_UNSUPPORTED
    assert b"several chains" in L.kin_last_error()
    fr = kinhip.parse_urdf(golden("fridge.urdf"), with_base=True)
    att = kinhip.AttachedUnionSDF(fr, [fr.find_joint("door_joint")])
    assert L.kin_traj_opt_batch(plan._h, att._h, C.byref(prm), X.data_ptr(), 20, 2, None, None, 0, None) \
        == K.KIN_E_UNSUPPORTED
    assert b"attached" in L.kin_last_error()
    ik = m.plan(joints, out_links=[m.find_link("gripper_link")], jac_link=m.find_link("gripper_link"), dtype=torch.float64)
    assert L.kin_traj_opt_batch(ik._h, sdf._h, C.byref(prm), X.data_ptr(), 20, 2, None, None, 0, None) == K.KIN_E_INVALID


@pytest.mark.parametrize("with_base", [False, True])
def test_plan_trajectory_gpu_solver(with_base):
    """tests/test_planning.py::test_gpu_plan_trajectory with solver="GPU": IK goal for (0.3, -0.4, 1.2) without
    rotation, 10 waypoints around a thin box; every waypoint clears the box by more than -1e-2."""
    import kinhip
    m, joints, sscc, sdf = _setup(with_base)
    m.set_joint_angles(joints, np.zeros(8 + (3 if with_base else 0)))
    q_start = m.get_joint_angles(joints)
    gl = m.find_link("gripper_link")
    q_goal, status = kinhip.inverse_kinematics_(m, gl, joints, _T((0.3, -0.4, 1.2)), with_rot=False)
    assert status == ":FTOL_REACHED"
    n_dof = len(q_start)
    plan = m.plan(joints, out_links=[gl], jac_link=gl, jac_joints=joints, dtype=torch.float64)
    N = 256
    g = torch.Generator().manual_seed(11)
    Q0 = (torch.rand((n_dof, N), generator=g, dtype=torch.float64) * 2 - 1).cuda()
    if with_base:
        Q0[8:] = 0.0
    tgt = torch.tensor(np.repeat(_T((0.3, -0.4, 1.2))[:3, :4].T.reshape(12, 1), N, axis=1), device="cuda")
    Q, it, _ = plan.ik_dls(tgt, Q0.contiguous(), with_rot=False, max_iters=64)
    _, _, mn = sscc.plan(joints, dtype=torch.float64).run(sdf, Q, dists=False, min_dist=True)
    ok = ((it <= 64) & (mn > 0.05)).nonzero()
    assert ok.numel() > 0
    q_goal = Q[:, int(ok[0, 0])].cpu().numpy()
    q_seq, status = kinhip.plan_trajectory(sscc, joints, sdf, q_start, q_goal, 10, ftol_abs=1e-5, solver="GPU")
    assert status == ":SUCCESS"
    np.testing.assert_allclose(q_seq[:, 0], q_start, atol=1e-6)
    np.testing.assert_allclose(q_seq[:, -1], q_goal, atol=1e-6)
    for i in range(10):
        m.set_joint_angles(joints, q_seq[:, i])
        assert np.all(kinhip.compute_coll_dists(sscc, joints, sdf) > -1e-2)
    m.set_joint_angles(joints, q_start)


def test_plan_trajectories_equals_single_calls():
    """plan_trajectories on the 32 goals = 32 calls of one trajectory each, bit for bit; the straight lines built on
    the device are the restatement's."""
    import kinhip
    m, joints, sscc, sdf = _setup(False)
    sc = R.scene(False)
    plan = _plan(False, torch.float64)
    Qg = torch.tensor(sc.q_goals, dtype=torch.float64, device="cuda")
    X, it, nf = kinhip.plan_trajectories(sscc, joints, sdf, sc.q_start, Qg, 10, plan=plan, max_iters=60)
    Xl, _, _ = kinhip.plan_trajectories(sscc, joints, sdf, sc.q_start, Qg, 10, plan=plan, max_iters=1, weight=1e-9,
                                        max_step=1e-12)
    np.testing.assert_allclose(R.from_columns(Xl.cpu().numpy(), 10), R.straight_lines(sc.q_start, sc.q_goals, 10),
                               atol=1e-11)
    for t in range(R.N_GOALS):
        X1, i1, n1 = kinhip.plan_trajectories(sscc, joints, sdf, sc.q_start, sc.q_goals[:, t], 10, plan=plan,
                                              max_iters=60)
        assert torch.equal(X1, X[:, t * 10:(t + 1) * 10]) and int(i1[0]) == int(it[t]) and torch.equal(n1[:, 0], nf[:, t])
    with pytest.raises(AssertionError):   # a goal inside the box
        kinhip.plan_trajectories(sscc, joints, sdf, sc.q_start, _colliding(sc), 10, plan=plan)


def _colliding(sc):
    """A configuration of the goal set's family whose spheres touch the box: the midpoint of the straight line with
    the least clearance."""
    out = R.full_run(10)
    t = int(np.argmin(out["d0"]))
    X0 = out["X0"][t]
    d, _ = sc.distances(np.ascontiguousarray(X0.T))
    w = int(np.argmin(d.min(0)))
    assert d[:, w].min() < 0.0
    return X0[w]
