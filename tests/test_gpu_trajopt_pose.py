"""kin_traj_opt_pose_batch (k_traj's POSE variant) on the GPU against its CPU restatement (tests/trajopt_pose_ref.py):
first iterates in fp64 on Fetch, seeded random chains at chain bounds 4 and 8, full runs, fp32, packing independence,
graph capture, unchanged behaviour of the plans and the Python layer.

Bounds.  One iteration, fp64: the project's 1e-9.  Eight iterations, fp64: TOL8 = 10 x SPREAD8_POSE, the restatement's
own forward / reversed-summation spread measured on the CPU (tests/test_trajopt_pose.py; never from the kernel)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import trajopt_cases as TC
import trajopt_pose_ref as PR
import trajopt_ref as R
from conftest import ARM, golden
from test_trajopt_pose import SPREAD8_POSE

pytestmark = pytest.mark.gpu

P = R.PARAMS
KW = {k: v for k, v in P.items() if k != "max_iters"}
FEAS_D = P["margin"] - P["feas"]
TOL1 = 1e-9
TOL8 = 10 * SPREAD8_POSE
ROWS = [0, 1, 2, 4, 5]      # info rows compared with the restatement (3 = accepted steps: compared exactly)


def _T(t):
    T = np.eye(4)
    T[:3, 3] = t
    return T


def _T12(col):
    T = np.eye(4)
    T[:3, :3] = col[:9].reshape(3, 3).T
    T[:3, 3] = col[9:12]
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
    return m, joints, sscc, sdf, m.find_link("gripper_link")


@functools.lru_cache(maxsize=None)
def _plan(with_base, dtype):
    m, joints, sscc, sdf, gl = _setup(with_base)
    plan = sscc.traj_plan(joints, [gl], dtype=dtype)
    assert plan.chain_bound == 8
    return plan


def _run(plan, sdf, X0, tg, c, with_rot, max_iters, dtype=torch.float64, dof_weights=None, **over):
    """X0 [nt, n_wp, nd], tg [12, nt] (numpy) -> X [nt, n_wp, nd], iters, info [6, nt] (numpy, fp64)."""
    import kinhip
    prm = dict(KW, max_iters=max_iters)
    prm.update(over)
    n_wp = X0.shape[1]
    X = torch.tensor(R.to_columns(X0), dtype=dtype, device="cuda")
    T = torch.tensor(np.ascontiguousarray(tg), dtype=dtype, device="cuda")
    it, nf = kinhip.traj_opt_pose_batch(plan, sdf, X, n_wp, T, c, with_rot=with_rot, dof_weights=dof_weights, **prm)
    torch.cuda.synchronize()
    return R.from_columns(X.double().cpu().numpy(), n_wp), it.cpu().numpy(), nf.double().cpu().numpy()


def _gpu_run(with_base, X0, tg, c, with_rot, max_iters, dtype=torch.float64, **over):
    return _run(_plan(with_base, dtype), _setup(with_base)[3], X0, tg, c, with_rot, max_iters, dtype, **over)


@pytest.mark.parametrize("with_base,rows,shape", PR.FIRST_CASES,
                         ids=[f"{'base' if b else 'nobase'}-rows{r}-wp{s[0]}-n{s[1]}-c{s[2]}" for b, r, s in PR.FIRST_CASES])
def test_first_iterates(with_base, rows, shape):
    """fp64, Fetch, the restatement's seeded X0 (L = 8 / 16 / 64, a partial segment, several workgroups, c at the
    first and the last interior waypoint).  One iteration: X and info rows 0-2, 4, 5 within 1e-9, accepted steps and
    iteration counts equal on the determined trajectories.  max_iters = 1..8: equal accept sequences on the
    determined trajectories; after 8, X and the merit within TOL8."""
    n_wp, n_traj, c = shape
    sc, link, c, wr, tg, X0 = PR.fetch_problem(n_wp, rows, c, with_base, n_traj)
    ref1 = PR.first_run(with_base, rows, shape, 1)
    X, it, nf = _gpu_run(with_base, X0, tg, c, wr, 1)
    e1 = (np.abs(X - ref1["X"]).max(), np.abs(nf[ROWS] - ref1["info"][ROWS]).max())
    det = ref1["determined"]
    print(f"1 iteration: max|dX| = {e1[0]:.2e}, max|d info| = {e1[1]:.2e}, determined {int(det.sum())}/{n_traj}")
    assert np.array_equal(nf[3][det], ref1["info"][3][det]) and np.array_equal(it[det], ref1["iters"][det])
    assert e1[0] <= TOL1 and e1[1] <= TOL1
    ref8 = PR.first_run(with_base, rows, shape, 8)
    nacc = [np.zeros(n_traj)]
    for k in range(1, 9):
        X, it, nf = _gpu_run(with_base, X0, tg, c, wr, k)
        nacc.append(nf[3])
    seq = np.diff(np.array(nacc), axis=0)
    ref_seq = np.maximum(ref8["accepts"], 0)
    ref_seq = np.vstack([ref_seq, np.zeros((8 - ref_seq.shape[0], n_traj))])
    e8 = (np.abs(X - ref8["X"]).max(), np.abs(nf[0] - ref8["info"][0]).max())
    det = ref8["determined"]
    print(f"8 iterations: max|dX| = {e8[0]:.2e}, max|d merit| = {e8[1]:.2e}, determined {int(det.sum())}/{n_traj}")
    assert n_traj < 67 or det.sum() >= 8
    assert np.array_equal(seq[:, det], ref_seq[:, det])
    assert np.array_equal(it[det], ref8["iters"][det])
    assert e8[0] <= TOL8 and e8[1] <= TOL8


# ---------------------------------------------------------------------------------------------------- random chains
_DIR = {}
MID_POSE = np.eye(4)


@pytest.fixture(scope="module", autouse=True)
def _urdf_dir(tmp_path_factory):
    _DIR["d"] = str(tmp_path_factory.mktemp("trajposechains"))


@functools.lru_cache(maxsize=None)
def _chain_setup(key, which):
    """The case of trajopt_cases on both sides with one pose link: "leaf" (the path's leaf link) or "mid" (a new
    link on a fixed joint, turned and offset, below the link of a mid-path batch joint).  The oracle side is a
    ChainScene of its own (the cached case stays as it is)."""
    import kinhip
    import oracle as O
    from kinhip.mechanism import Link
    cs = TC.case(key)
    ch = cs.ch
    sc = R.ChainScene(ch.tree, cs.with_base, ch.q_ids, ch.held, ch.held_ang, cs.spheres, cs.sc.box_poses,
                      cs.sc.box_widths)
    p = os.path.join(_DIR["d"], f"chain{key[0]}.urdf")
    if not os.path.exists(p):
        with open(p, "w") as f:
            f.write(ch.text)
    m = kinhip.parse_urdf(p, with_base=cs.with_base)
    for j, a in zip(ch.held, ch.held_ang):
        m.set_joint_angle(m.joints[j - 1], float(a))
    joints = [m.joints[j - 1] for j in ch.q_ids]
    sscc = kinhip.SweptSphereCollisionChecker(m)
    for l, c, r in cs.spheres:
        sscc.add_coll_sphere(m.links[l - 1], c, r)
    sdf = kinhip.UnionSDF([kinhip.BoxSDF(T, w) for T, w in zip(cs.sc.box_poses, cs.sc.box_widths)])
    if which == "leaf":
        link_o, link_k = ch.leaf, m.links[ch.leaf - 1]
    else:
        on_path = [j for j in ch.path if j in ch.q_ids]
        parent = int(ch.tree.joint_clink[on_path[len(on_path) // 2] - 1])
        Tm = np.eye(4)
        Tm[:3, :3] = O.rpy_to_matrix([0.4, -0.3, 0.7])
        Tm[:3, 3] = (0.05, -0.08, 0.11)
        link_o = sc.om.add_new_link(parent, Tm)
        link_k = Link("pose_mid")
        m.add_new_link(link_k, m.links[parent - 1], Tm)
    plan = sscc.traj_plan(joints, [link_k], dtype=torch.float64)
    assert plan.chain_bound == cs.bound, (key, plan.chain_bound)
    # targets: the link's pose at a random configuration inside the limits
    rng = np.random.default_rng(6100 + 10 * key[0] + int(key[1]))
    bounded = np.isfinite(sc.lo) & np.isfinite(sc.hi)
    flo, fhi = np.where(bounded, sc.lo, -np.pi), np.where(bounded, sc.hi, np.pi)
    flo[len(ch.q_ids):], fhi[len(ch.q_ids):] = -0.5, 0.5
    q = flo[:, None] + (fhi - flo)[:, None] * rng.random((sc.n_dof, TC.N_TRAJ))
    tg = np.ascontiguousarray(sc.om.fk_batch(q, sc.ids, [link_o])[0])
    return cs, sc, link_o, plan, sdf, tg


@pytest.mark.parametrize("rows", [3, 6])
@pytest.mark.parametrize("which", ["mid", "leaf"])
@pytest.mark.parametrize("key", [(1, False), (1, True), (3, False), (3, True)], ids=TC.cid)
def test_random_chains(key, which, rows):
    """Chains 1 and 3 of trajopt_cases (chain bounds 4 and 8, without and with the base; held joints, oblique axes,
    dof_weights, rotated boxes): after one iteration X and info rows 0-2, 4, 5 equal the restatement's to 1e-9; the
    plan's chain bound is the case's."""
    cs, sc, link, plan, sdf, tg = _chain_setup(key, which)
    c = cs.n_wp // 2
    ref = PR.run(sc, link, c, rows == 6, tg, cs.X0, max_iters=1, dof_weights=cs.dof_weights, **TC.KW)
    X, it, nf = _run(plan, sdf, cs.X0, tg, c, rows == 6, 1, dof_weights=cs.dof_weights)
    e = (np.abs(X - ref["X"]).max(), np.abs(nf[ROWS] - ref["info"][ROWS]).max())
    print(f"{TC.cid(key)} {which} rows {rows} bound {cs.bound} n_wp {cs.n_wp}: max|dX| = {e[0]:.2e}, "
          f"max|d info| = {e[1]:.2e}, |r_p| up to {nf[4].max():.2f}")
    det = ref["determined"]
    assert np.array_equal(nf[3][det], ref["info"][3][det]) and np.array_equal(it[det], ref["iters"][det])
    assert np.abs(X - cs.X0).max() > 1e-3          # (the step is not a no-op)
    assert e[0] <= TOL1 and e[1] <= TOL1


# -------------------------------------------------------------------------------------------------------- full runs
def _interior_min(plan, sdf, X, n_wp):
    Q = torch.tensor(R.to_columns(X), dtype=torch.float64, device="cuda")
    _, _, mn = plan.run(sdf, Q, dists=False, min_dist=True)
    return mn.cpu().numpy().reshape(-1, n_wp)[:, 1:-1].min(1)


def _reeval(X, n_wp, rows, c, tg):
    """-> min interior clearance (kin_coll_batch, fp64), |r_p|, |r_rot| (oracle FK) of X."""
    sc = R.scene(False)
    dm = _interior_min(_plan(False, torch.float64), _setup(False)[3], X, n_wp)
    r, _ = PR.residual(sc, PR.fetch_link(), np.ascontiguousarray(X[:, c].T), tg, rows == 6)
    rp, rr = PR.norms(r)
    return dm, rp, rr


@pytest.mark.parametrize("n_wp,rows", PR.CASES)
def test_full_runs_fp64(n_wp, rows):
    """200 iterations on the 32-goal family: end waypoints bit-equal to the input, interior waypoints within the
    limits, info rows 2, 4, 5 equal a re-evaluation to 1e-9, the good set equals the restatement's except for
    trajectories whose restatement clearance or residual lies within 1e-6 of its threshold (at most 2), and for
    every good trajectory the library's PoseConstraint (rpy residual) gives |val| < 2 tol."""
    import kinhip
    sc = R.scene(False)
    ref = PR.full_run(n_wp, rows)
    c, tg = ref["c"], ref["targets"]
    X, it, nf = _gpu_run(False, ref["X0"], tg, c, rows == 6, P["max_iters"])
    assert np.array_equal(X[:, 0], ref["X0"][:, 0]) and np.array_equal(X[:, -1], ref["X0"][:, -1])
    assert np.all(X[:, 1:-1] >= sc.lo) and np.all(X[:, 1:-1] <= sc.hi)
    dm, rp, rr = _reeval(X, n_wp, rows, c, tg)
    assert np.abs(nf[2] - dm).max() <= 1e-9 and np.abs(nf[4] - rp).max() <= 1e-9 and np.abs(nf[5] - rr).max() <= 1e-9
    good = (rp < PR.TOL) & (rr < PR.TOL) & (dm >= FEAS_D)
    done = it <= P["max_iters"]
    assert np.all(good[done])
    ri = ref["info"]
    near = (np.abs(ri[2] - FEAS_D) < 1e-6) | (np.abs(ri[4] - PR.TOL) < 1e-6) | (np.abs(ri[5] - PR.TOL) < 1e-6)
    ref_good = PR.good(ref, P["margin"], P["feas"])
    print(f"n_wp = {n_wp}, rows = {rows}: good {int(good.sum())}/32 (restatement {int(ref_good.sum())}), done "
          f"{int(done.sum())}/32, near a threshold in the restatement: {int(near.sum())}")
    assert near.sum() <= 2
    assert np.array_equal(good[~near], ref_good[~near])
    m, joints, _, _, gl = _setup(False)
    pc = kinhip.PoseConstraint(c + 1, sc.n_dof, gl, np.eye(4), rows == 6, m, joints)
    Qc = torch.tensor(np.ascontiguousarray(X[:, c].T), dtype=torch.float64, device="cuda")
    V, _, _ = pc.eval_batch(0, Qc, torch.tensor(tg, dtype=torch.float64, device="cuda"))
    assert float(V[:, torch.tensor(good, device="cuda")].abs().max()) < 2 * PR.TOL


def test_fp32():
    """fp32 on (10, 6): every trajectory reported done is good when re-evaluated in fp64, with slack 1e-5 on the
    residuals and 1e-6 on the clearance (the project's fp32 pose and distance gates); at least one is done; the
    merit does not increase over runs of 1, 2, 4, 8 iterations."""
    ref = PR.full_run(10, 6)
    c, tg = ref["c"], ref["targets"]
    X, it, nf = _gpu_run(False, ref["X0"], tg, c, True, P["max_iters"], dtype=torch.float32)
    done = it <= P["max_iters"]
    dm, rp, rr = _reeval(X, 10, 6, c, tg)
    print(f"fp32: done {int(done.sum())}/32, over them max |r_p| {rp[done].max():.2e}, max |r_rot| {rr[done].max():.2e}, "
          f"min clearance {dm[done].min():.6f}")
    assert done.sum() >= 1
    assert np.all(rp[done] < PR.TOL + 1e-5) and np.all(rr[done] < PR.TOL + 1e-5) and np.all(dm[done] >= FEAS_D - 1e-6)
    last = None
    for k in (1, 2, 4, 8):
        _, _, nk = _gpu_run(False, ref["X0"], tg, c, True, k, dtype=torch.float32)
        if last is not None:
            assert np.all(nk[0] <= last)
        assert np.all(nk[3] <= k)
        last = nk[0]


def test_independence_and_packing():
    """Trajectory t of a 67-batch is bit-equal to the same trajectory run alone and in another segment position."""
    sc, link, c, wr, tg, X0 = PR.fetch_problem(10, 6, 5, False, 67)
    X, it, nf = _gpu_run(False, X0, tg, c, wr, 40)
    for t in (0, 5, 31, 66):
        Xa, ia, na = _gpu_run(False, X0[t:t + 1], tg[:, t:t + 1], c, wr, 40)
        assert np.array_equal(Xa[0], X[t]) and ia[0] == it[t] and np.array_equal(na[:, 0], nf[:, t])
        sel = [1, 2, t, 3]
        Xb, ib, nb = _gpu_run(False, X0[sel], tg[:, sel], c, wr, 40)
        assert np.array_equal(Xb[2], X[t]) and ib[2] == it[t] and np.array_equal(nb[:, 2], nf[:, t])


def test_capture():
    """After one eager call (which stages the metric table), a call captured in a graph replays the eager result."""
    import kinhip
    sdf = _setup(False)[3]
    plan = _plan(False, torch.float64)
    ref = PR.full_run(10, 6)
    X0 = torch.tensor(R.to_columns(ref["X0"]), dtype=torch.float64, device="cuda")
    tg = torch.tensor(ref["targets"], dtype=torch.float64, device="cuda")
    Xe = X0.clone()
    ite, nfe = kinhip.traj_opt_pose_batch(plan, sdf, Xe, 10, tg, 5, **P)
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
            kinhip.traj_opt_pose_batch(plan, sdf, Xg, 10, tg, 5, iters=itg, info=nfg, stream=s, **P)
        for rep in range(2):
            g.replay()
            s.synchronize()
            assert torch.equal(Xg, Xe) and torch.equal(itg, ite) and torch.equal(nfg, nfe), rep


def test_unchanged_behaviour_of_the_plans():
    """On a kin_traj_plan_create plan, kin_coll_batch and kin_traj_opt_batch give the results of the
    kin_coll_plan_create plan of the same checker, bit for bit, on the 32-goal set; kin_traj_opt_pose_batch on the
    plain collision plan is KIN_E_UNSUPPORTED."""
    import kinhip
    from kinhip import _lib as K
    m, joints, sscc, sdf, gl = _setup(False)
    tp = _plan(False, torch.float64)
    cp = sscc.plan(joints, dtype=torch.float64)
    assert tp.n_sph == cp.n_sph
    ref = R.full_run(10)
    X0 = torch.tensor(R.to_columns(ref["X0"]), dtype=torch.float64, device="cuda")
    da, ga, ma = cp.run(sdf, X0, dists=True, grads=True, min_dist=True)
    db, gb, mb = tp.run(sdf, X0, dists=True, grads=True, min_dist=True)
    assert torch.equal(da, db) and torch.equal(ga, gb) and torch.equal(ma, mb)
    Xa, Xb = X0.clone(), X0.clone()
    ia, na = kinhip.traj_opt_batch(cp, sdf, Xa, 10, **P)
    ib, nb = kinhip.traj_opt_batch(tp, sdf, Xb, 10, **P)
    torch.cuda.synchronize()
    assert torch.equal(Xa, Xb) and torch.equal(ia, ib) and torch.equal(na, nb)
    tg = torch.tensor(PR.full_run(10, 6)["targets"], dtype=torch.float64, device="cuda")
    with pytest.raises(K.KinError, match="no pose links") as e:
        kinhip.traj_opt_pose_batch(cp, sdf, X0.clone(), 10, tg, 5)
    assert e.value.code == K.KIN_E_UNSUPPORTED


# ------------------------------------------------------------------------------------------------- the Python layer
def test_plan_trajectory_gpu_solver_with_a_pose_constraint():
    """plan_trajectory(solver="GPU", partial_consts=[PoseConstraint]) on a target of the restatement's good set:
    :SUCCESS, waypoint 6 meets the constraint (axis-angle residual < 1e-3, by the oracle), every waypoint clears the
    box by more than -1e-2; two constraints, or one with two links, raise ValueError."""
    import kinhip
    m, joints, sscc, sdf, gl = _setup(False)
    sc = R.scene(False)
    ref = PR.full_run(10, 6)
    ok = np.nonzero(PR.good(ref, P["margin"], P["feas"]) & (ref["iters"] <= 100))[0]
    t = int(ok[0])
    T = _T12(ref["targets"][:, t])
    n_dof = sc.n_dof
    pc = kinhip.PoseConstraint(6, n_dof, gl, T, True, m, joints)
    q_start, q_goal = sc.q_start, sc.q_goals[:, t]
    q_seq, status = kinhip.plan_trajectory(sscc, joints, sdf, q_start, q_goal, 10, solver="GPU", partial_consts=[pc])
    assert status == ":SUCCESS"
    np.testing.assert_allclose(q_seq[:, 0], q_start, atol=1e-12)
    np.testing.assert_allclose(q_seq[:, -1], q_goal, atol=1e-12)
    r, _ = PR.residual(sc, PR.fetch_link(), np.ascontiguousarray(q_seq[:, 5:6]), ref["targets"][:, t:t + 1], True)
    rp, rr = PR.norms(r)
    assert rp[0] < PR.TOL and rr[0] < PR.TOL
    for i in range(10):
        m.set_joint_angles(joints, q_seq[:, i])
        assert np.all(kinhip.compute_coll_dists(sscc, joints, sdf) > -1e-2)
    m.set_joint_angles(joints, q_start)
    wl = m.find_link("wrist_roll_link")
    with pytest.raises(ValueError):
        kinhip.plan_trajectory(sscc, joints, sdf, q_start, q_goal, 10, solver="GPU", partial_consts=[pc, pc])
    two = kinhip.PoseConstraint(6, n_dof, [gl, wl], [T, T], [True, True], m, joints)
    with pytest.raises(ValueError):
        kinhip.plan_trajectory(sscc, joints, sdf, q_start, q_goal, 10, solver="GPU", partial_consts=[two])


def test_plan_trajectories_with_pose_equals_single_calls():
    """plan_trajectories with pose arguments on 8 goals = 8 calls of one trajectory each, bit for bit (the IK seeding
    included); its info has 6 rows."""
    import kinhip
    m, joints, sscc, sdf, gl = _setup(False)
    sc = R.scene(False)
    plan = _plan(False, torch.float64)
    ref = PR.full_run(10, 6)
    n = 8
    Qg = torch.tensor(sc.q_goals[:, :n], dtype=torch.float64, device="cuda")
    tg = torch.tensor(ref["targets"][:, :n], dtype=torch.float64, device="cuda")
    kw = dict(plan=plan, max_iters=60, pose_link=gl, pose_wp=5)
    X, it, nf = kinhip.plan_trajectories(sscc, joints, sdf, sc.q_start, Qg, 10, pose_targets=tg, **kw)
    assert nf.shape == (6, n)
    for t in range(n):
        X1, i1, n1 = kinhip.plan_trajectories(sscc, joints, sdf, sc.q_start, sc.q_goals[:, t], 10,
                                              pose_targets=tg[:, t:t + 1].contiguous(), **kw)
        assert torch.equal(X1, X[:, t * 10:(t + 1) * 10]) and int(i1[0]) == int(it[t]) and torch.equal(n1[:, 0], nf[:, t])
    # one 4x4 target for every trajectory
    X4, _, _ = kinhip.plan_trajectories(sscc, joints, sdf, sc.q_start, sc.q_goals[:, 0], 10,
                                        pose_targets=_T12(ref["targets"][:, 0]), **kw)
    assert torch.equal(X4, X[:, :10])
    with pytest.raises(ValueError):
        kinhip.plan_trajectories(sscc, joints, sdf, sc.q_start, Qg, 10, pose_link=gl, pose_wp=9, pose_targets=tg)
