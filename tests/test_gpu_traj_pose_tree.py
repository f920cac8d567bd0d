"""kin_traj_opt_pose_tree_batch (k_traj_pose_tree) on the GPU against the CPU restatement (tests/trajopt_pose_ref.py,
unchanged) on the cases of tests/trajopt_pose_tree_cases.py: a pose link held at a waypoint on the two-arm robot (the
link on either part), the PR2 with both arms and the base, a random tree whose carrying part has bound 4, and Fetch and
the PR2 at the fridge with the door swinging.

Bounds.  One iteration, fp64: the project's 1e-9.  Eight iterations, fp64: TOL8_PT = 10 x SPREAD8_PT, the restatement's
own forward / reversed spread over the cases (tests/test_trajopt_pose_tree.py, CPU).  fp32, one iteration against the
fp64 restatement: DELTA32_PT = 4 x D32_PT capped at 3e-4, D32_PT the largest such deviation of the existing k_traj_pose
fp32 kernel (not under test here) against its restatement on the single-part sub-problems of the two-arm cases and of
Fetch at the fridge frozen at one scene state (same robot, boxes and X0, one part's spheres);
test_single_parts_on_the_existing_kernel re-measures it and holds it to the recorded constant.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import test_gpu_traj_scene as GS
import test_gpu_traj_tree as GT
import trajopt_pose_ref as P
import trajopt_pose_tree_cases as PT
import trajopt_ref as R
from kinhip import _lib as K
from test_trajopt_pose_tree import SPREAD8_PT

pytestmark = pytest.mark.gpu

TOL1 = 1e-9
TOL8_PT = 10 * SPREAD8_PT
assert TOL8_PT <= 1e-10      # (beyond: a case would be ill-conditioned -- another target, not a wider bound)
D32_PT = 1.6e-5              # measured 1.578e-5 on an MI355X (s-fetch; the two-arm parts 1.4e-6 .. 3.3e-6)
DELTA32_PT = min(4 * D32_PT, 3e-4)
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _urdf_dir(tmp_path_factory):
    GT._DIR.setdefault("d", str(tmp_path_factory.mktemp("trajposetree_t")))
    GS._DIR.setdefault("d", str(tmp_path_factory.mktemp("trajposetree_s")))


def _side(cs):
    return GS if cs.scene else GT


def _sname(cs):
    return PT.SPECS[cs.name][1]


@functools.lru_cache(maxsize=None)
def _plan(name, dtype, spheres=None):
    """The TrajPlan of the case: its checker (with all spheres, or one part's) plus the pose link."""
    cs = PT.case(name)
    G, b = _side(cs), _sname(cs)
    m, joints = G._mech(b)
    sscc = G._checker(b) if spheres is None else GT._checker(b, spheres)
    plan = sscc.traj_plan(joints, [m.links[cs.link - 1]], dtype=dtype)
    if spheres is None:
        assert plan.n_parts == len(cs.base.parts) and plan.part_chain_bounds == cs.base.bounds, plan.part_chain_bounds
        assert plan.pose_link_parts == [cs.part], (name, plan.pose_link_parts)
    return plan


def _sdf(cs):
    return GS._att(_sname(cs)) if cs.scene else GT._sdf(_sname(cs))


def _gpu_run(name, max_iters, dtype=torch.float64, X0=None, targets=None, plan=None, sdf=None, SQ=None, entry=None,
             damp=None):
    """-> X [nt, n_wp, nd], iters, info [6, nt] (numpy, fp64) through kin_traj_opt_pose_tree_batch (entry: another
    function with traj_opt_pose_batch's arguments).  xi, info, iters, targets and scene_q are views with a sentinel row
    before and after and more columns than used (NaN there in xi, targets and scene_q); every run checks what the
    kernel must leave alone: the guards, the padding, the inputs, the end columns, and the joint limits."""
    import kinhip
    cs = PT.case(name)
    X0 = cs.X0 if X0 is None else X0
    tg0 = cs.targets if targets is None else targets
    nt, n_wp, nd = X0.shape
    cols = nt * n_wp
    bigx, X = GS._guarded(nd, cols, cols + PT.PAD, dtype, NAN)
    Xin = torch.tensor(R.to_columns(X0), dtype=dtype, device="cuda")
    X.copy_(Xin)
    bigi, it = GS._guarded(1, nt, nt + 3, torch.int32, int(PT.SENT - 0.75))
    bign, nf = GS._guarded(6, nt, nt + 5, dtype, PT.SENT)
    bigt, tg = GS._guarded(12, nt, nt + 4, dtype, NAN)
    tg.copy_(torch.tensor(tg0, dtype=dtype))
    kw = dict(PT.KW, max_iters=max_iters, dof_weights=cs.dof_weights, iters=it[0], info=nf, with_rot=cs.with_rot,
              damp=cs.damp if damp is None else damp)
    sdf = _sdf(cs) if sdf is None else sdf
    guards = [(bigx, nd, cols, NAN), (bigi, 1, nt, int(PT.SENT - 0.75)), (bign, 6, nt, PT.SENT), (bigt, 12, nt, NAN)]
    if isinstance(sdf, kinhip.AttachedUnionSDF):
        SQ = cs.base.SQ if SQ is None else SQ
        nc = cs.sc.n_scene_cols
        if SQ.ndim == 1:
            bigs, sq = GS._guarded(1, nc, nc + 3, dtype, PT.SENT)
            sq = sq[0]
            guards.append((bigs, 1, nc, PT.SENT))
        else:
            bigs, sq = GS._guarded(nc, cols, cols + PT.PAD + 2, dtype, NAN)
            guards.append((bigs, nc, cols, NAN))
        sq.copy_(torch.tensor(SQ, dtype=dtype))
        kw["scene_q"] = sq
    (entry or kinhip.traj_opt_pose_tree_batch)(_plan(name, dtype) if plan is None else plan, sdf, X, n_wp, tg, cs.c, **kw)
    torch.cuda.synchronize()
    for g in guards:
        assert GS._untouched(*g)
    assert torch.equal(tg, torch.tensor(tg0, dtype=dtype, device="cuda"))
    if "scene_q" in kw:
        assert torch.equal(kw["scene_q"], torch.tensor(SQ, dtype=dtype, device="cuda"))
    ends = torch.arange(nt, device="cuda") * n_wp
    assert torch.equal(X[:, ends], Xin[:, ends]) and torch.equal(X[:, ends + n_wp - 1], Xin[:, ends + n_wp - 1])
    Xo = R.from_columns(X.double().cpu().numpy(), n_wp)
    ndt = np.float32 if dtype == torch.float32 else np.float64
    assert np.all(Xo[:, 1:-1] >= cs.sc.lo.astype(ndt)) and np.all(Xo[:, 1:-1] <= cs.sc.hi.astype(ndt))
    return Xo, it[0].cpu().numpy().copy(), nf.double().cpu().numpy()


def test_the_pose_link_rides_on_either_part():
    """kin_plan_pose_link_part: l_grip on part 0 and r_grip on part 1 of the two-arm plan, the PR2's left tool frame on
    part 1, tree3's leaf on its last part (bound 4); an index out of range is KIN_E_KEY."""
    assert PT.case("twoarm-l3").part == 0 and PT.case("twoarm-r3").part == 1 and PT.case("pr2").part == 1
    assert PT.case("tree3").part == 3 and PT.case("tree3").base.bounds[3] == 4
    for name in PT.CASES:
        _plan(name, torch.float64)           # (asserts the part)
    v = C.c_int32(-5)
    h = _plan("twoarm-r3", torch.float64)._h
    for i in (-1, 1):
        assert K.lib().kin_plan_pose_link_part(h, i, C.byref(v)) == K.KIN_E_KEY and v.value == -5
    assert K.lib().kin_plan_pose_link_part(GT._plan("twoarm-nobase", torch.float64)._h, 0, C.byref(v)) == K.KIN_E_KEY


@pytest.mark.parametrize("name", PT.CASES)
def test_first_iterates(name):
    """fp64.  One iteration: X and info rows 0-2, 4, 5 equal the restatement's to 1e-9, info[3] and iters are equal on
    the determined trajectories.  max_iters = 1..8: the accept sequences are equal on the determined trajectories;
    after 8 iterations X and the merit are within TOL8_PT."""
    cs = PT.case(name)
    nt = cs.n_traj
    ref1 = PT.ref_run(name, 1)
    X, it, nf = _gpu_run(name, 1)
    rows = [0, 1, 2, 4, 5]
    e1 = (np.abs(X - ref1["X"]).max(), np.abs(nf[rows] - ref1["info"][rows]).max())
    print(f"{name} part {cs.part} n_wp {cs.n_wp}: 1 iteration max|dX| = {e1[0]:.2e}, max|d info| = {e1[1]:.2e}")
    det = ref1["determined"]
    assert np.array_equal(nf[3][det], ref1["info"][3][det]) and np.array_equal(it[det], ref1["iters"][det])
    assert e1[0] <= TOL1 and e1[1] <= TOL1
    ref8 = PT.ref_run(name, 8)
    nacc = [np.zeros(nt)]
    for k in range(1, 9):
        X, it, nf = _gpu_run(name, k)
        nacc.append(nf[3])
    seq = np.diff(np.array(nacc), axis=0)
    ref_seq = np.maximum(ref8["accepts"], 0)
    ref_seq = np.vstack([ref_seq, np.zeros((8 - ref_seq.shape[0], nt))])
    det = ref8["determined"]
    e8 = (np.abs(X - ref8["X"])[det].max(), np.abs(nf[0] - ref8["info"][0])[det].max())
    print(f"{name}: 8 iterations max|dX| = {e8[0]:.2e}, max|d merit| = {e8[1]:.2e}, determined {int(det.sum())}/{nt}")
    assert det.sum() >= min(5, nt)
    assert np.array_equal(seq[:, det], ref_seq[:, det])
    assert np.array_equal(it[det], ref8["iters"][det])
    assert e8[0] <= TOL8_PT and e8[1] <= TOL8_PT


def _single_parts():
    """(case, part's spheres or None, static scene of the restatement): the single-part sub-problems of the two-arm
    cases (the carrying part's spheres) and of s-fetch (its one part, the scene frozen at trajectory 0's middle
    waypoint)."""
    out = [(n, tuple(PT.case(n).base.parts[PT.case(n).part]), None) for n in ("twoarm-l3", "twoarm-l6", "twoarm-r3", "twoarm-r6")]
    return out + [("s-fetch", None, PT.case("s-fetch").sc.frozen(PT.case("s-fetch").base.mid_state))]


def test_single_parts_on_the_existing_kernel():
    """The input of DELTA32_PT: kin_traj_opt_pose_batch (k_traj_pose, unchanged) in fp32 on the single-part
    sub-problems against its restatement after one iteration.  Printed and held to the recorded constant."""
    import kinhip
    d32 = 0.0
    for name, sph, frozen in _single_parts():
        cs = PT.case(name)
        sc = PT.sub_scene(cs, cs.part) if frozen is None else frozen
        ref = PT.run_case(cs, 1, sc=sc)
        plan = _plan(name, torch.float32, sph)
        assert plan.n_parts == 1
        sdf = GT._sdf(_sname(cs)) if frozen is None else GS._static(frozen)
        X32, _, _ = _gpu_run(name, 1, dtype=torch.float32, plan=plan, sdf=sdf, entry=kinhip.traj_opt_pose_batch)
        e = np.abs(X32 - ref["X"]).max()
        print(f"{name} single part: k_traj_pose fp32 1 iteration |X32 - X_ref| = {e:.3e}")
        d32 = max(d32, e)
    print(f"D32_PT measured {d32:.3e} (recorded {D32_PT:.3e})")
    assert d32 <= D32_PT


@pytest.mark.parametrize("name", PT.CASES)
def test_fp32(name):
    """fp32, one iteration against the fp64 restatement: within DELTA32_PT."""
    ref = PT.ref_run(name, 1)
    X, _, nf = _gpu_run(name, 1, dtype=torch.float32)
    e = np.abs(X - ref["X"]).max()
    print(f"{name}: fp32 1 iteration |X32 - X_ref| = {e:.3e} (DELTA32_PT {DELTA32_PT:.1e})")
    assert np.isfinite(nf).all()
    assert e <= DELTA32_PT


def test_single_chain_static_plan_is_the_pose_kernel():
    """A single-chain plan against a static union through the new entry point: kin_traj_opt_pose_batch bit for bit."""
    import kinhip
    cs = PT.case("s-fetch")
    frozen = cs.sc.frozen(cs.base.mid_state)
    plan, sdf = _plan("s-fetch", torch.float64), GS._static(frozen)
    a = _gpu_run("s-fetch", 8, plan=plan, sdf=sdf)
    b = _gpu_run("s-fetch", 8, plan=plan, sdf=sdf, entry=kinhip.traj_opt_pose_batch)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_a_pose_plan_is_its_collision_plan():
    """kin_coll_batch, kin_traj_opt_tree_batch and kin_traj_opt_scene_batch on a plan with a pose link on part 1 equal
    those on the plain plan of the same desc, bit for bit (same parts, same part table)."""
    import kinhip
    for name, plain in (("twoarm-r6", GT._plan("twoarm-nobase", torch.float64)), ("s-pr2", GS._plan("pr2", torch.float64))):
        cs = PT.case(name)
        pose = _plan(name, torch.float64)
        X = torch.tensor(R.to_columns(cs.X0), dtype=torch.float64, device="cuda")
        kw = dict(PT.KW, max_iters=5, dof_weights=cs.dof_weights)
        if cs.scene:
            sq = torch.tensor(cs.base.SQ, dtype=torch.float64, device="cuda")
            outs = [(p.run(_sdf(cs), X, grads=True, min_dist=True, scene_q=sq),
                     (lambda Y: (Y,) + kinhip.traj_opt_scene_batch(p, _sdf(cs), Y, cs.n_wp, sq, **kw))(X.clone()))
                    for p in (pose, plain)]
        else:
            outs = [(p.run(_sdf(cs), X, grads=True, min_dist=True),
                     (lambda Y: (Y,) + kinhip.traj_opt_tree_batch(p, _sdf(cs), Y, cs.n_wp, **kw))(X.clone()))
                    for p in (pose, plain)]
        for u, v in zip(outs[0], outs[1]):
            for x, y in zip(u, v):
                assert torch.equal(x, y)


def test_a_far_target_changes_the_result():
    """The target moved 0.5 m further: another trajectory (a kernel that ignored the constraint would return the same)."""
    for name in ("twoarm-r3", "s-pr2"):
        cs = PT.case(name)
        far = cs.targets.copy()
        far[9:12] += 0.5
        a, b = _gpu_run(name, 4), _gpu_run(name, 4, targets=far)
        assert np.abs(a[0] - b[0]).max() > 1e-3 and np.all(b[2][4] > a[2][4])


@pytest.mark.parametrize("name", ["twoarm-r6", "pr2", "tree3", "s-fetch", "s-pr2", "s-uniform"])
def test_info_rows_are_the_returned_state(name):
    """info[2] = kin_coll_batch (static) or kin_coll_batch_scene on the returned trajectory's interior waypoints, and
    info[4..5] = the restatement's residual norms re-evaluated there, to 1e-9."""
    cs = PT.case(name)
    X, _, nf = _gpu_run(name, 8)
    Q = torch.tensor(R.to_columns(X), dtype=torch.float64, device="cuda")
    kw = {}
    if cs.scene:
        SQ = cs.base.SQ
        kw["scene_q"] = torch.tensor(SQ if SQ.ndim == 1 else np.ascontiguousarray(SQ), dtype=torch.float64, device="cuda")
    _, _, mn = _plan(name, torch.float64).run(_sdf(cs), Q, dists=False, min_dist=True, **kw)
    mn = mn.cpu().numpy().reshape(cs.n_traj, cs.n_wp)[:, 1:-1].min(1)
    r, _ = P.residual(cs.sc, cs.link, X[:, cs.c].T, cs.targets, cs.with_rot)
    rp, rr = P.norms(r)
    e = max(np.abs(nf[2] - mn).max(), np.abs(nf[4] - rp).max(), np.abs(nf[5] - rr).max())
    print(f"{name}: info rows 2, 4, 5 against a re-evaluation {e:.2e}")
    assert e <= 1e-9


@pytest.mark.parametrize("name,n", [("tree3", 8), (PT.WP64, 8)])
def test_packing_independence(name, n):
    """One trajectory alone = the same trajectory at positions 0 and 8 of 9, bit for bit."""
    cs = PT.case(name)
    X1, tg1 = cs.X0[:1], cs.targets[:, :1]
    alone = _gpu_run(name, n, X0=X1, targets=tg1)
    other = cs.X0[np.arange(1, 8) % cs.n_traj]
    X9 = np.concatenate([X1, other, X1])
    tg9 = np.concatenate([tg1, cs.targets[:, np.arange(1, 8) % cs.n_traj], tg1], 1)
    packed = _gpu_run(name, n, X0=X9, targets=tg9)
    for t in (0, 8):
        assert np.array_equal(packed[0][t], alone[0][0]) and packed[1][t] == alone[1][0]
        assert np.array_equal(packed[2][:, t], alone[2][:, 0])


def test_graph_capture_and_replay():
    """One capture and two replays on the default hardware queues (one kernel node): the eager result."""
    import kinhip
    cs = PT.case("twoarm-r3")
    plan, sdf = _plan("twoarm-r3", torch.float64), _sdf(cs)
    X0 = torch.tensor(R.to_columns(cs.X0), dtype=torch.float64, device="cuda")
    tg = torch.tensor(cs.targets, dtype=torch.float64, device="cuda")
    kw = dict(PT.KW, max_iters=8, dof_weights=cs.dof_weights, with_rot=cs.with_rot)
    Xe = X0.clone()
    ite, nfe = kinhip.traj_opt_pose_tree_batch(plan, sdf, Xe, cs.n_wp, tg, cs.c, **kw)   # (stages the metric table)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    Xg, itg, nfg = X0.clone(), torch.empty_like(ite), torch.empty_like(nfe)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            Xg.copy_(X0)
            kinhip.traj_opt_pose_tree_batch(plan, sdf, Xg, cs.n_wp, tg, cs.c, iters=itg, info=nfg, stream=s, **kw)
        for _ in range(2):
            g.replay()
    s.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(Xg, Xe) and torch.equal(itg, ite) and torch.equal(nfg, nfe)


def test_limits_on_the_device():
    """KIN_E_UNSUPPORTED / KIN_E_INVALID with xi untouched: a plan without pose links, a common bound of 16 (tree1, the
    link on its bound-8 part), scene_q with a static union, lds with a static union, no scene_q with an attached one,
    lds too small, ldt too small, n_con = 2."""
    L = K.lib()
    cs = PT.case("twoarm-r3")
    nt, n_wp, nd = cs.X0.shape
    X = torch.tensor(R.to_columns(cs.X0), dtype=torch.float64, device="cuda")
    Xin = X.clone()
    tg = torch.tensor(cs.targets, dtype=torch.float64, device="cuda")
    prm = K.TrajParams(n_wp, 5, 0.02, 0.03, 10.0, 1e-3, 1e-6, 0.5, None)
    wps, rots = (C.c_int32 * 1)(cs.c), (C.c_int32 * 1)(0)

    def pp(n_con=1):
        return K.TrajPoseParams(n_con, C.cast(wps, C.c_void_p), C.cast(rots, C.c_void_p), 10.0, 1e-6, 1e-3, 1e-3)

    def call(plan, sdf, scene_q=None, lds=0, ldt=nt, n_con=1, x=X):
        p = pp(n_con)
        rc = L.kin_traj_opt_pose_tree_batch(plan._h, sdf._h, C.byref(prm), C.byref(p), tg.data_ptr(), ldt, scene_q, lds,
                                            x.data_ptr(), x.stride(0), nt, None, None, 0, None)
        torch.cuda.synchronize()
        return rc, L.kin_last_error()

    plan, sdf = _plan("twoarm-r3", torch.float64), _sdf(cs)
    rc, msg = call(GT._plan("twoarm-nobase", torch.float64), sdf)
    assert rc == K.KIN_E_UNSUPPORTED and b"no pose links" in msg
    rc, msg = call(plan, sdf, scene_q=tg.data_ptr())
    assert rc == K.KIN_E_INVALID and b"scene_q" in msg
    rc, msg = call(plan, sdf, lds=nt * n_wp)
    assert rc == K.KIN_E_INVALID and b"lds" in msg
    rc, msg = call(plan, sdf, ldt=nt - 1)
    assert rc == K.KIN_E_INVALID and b"ldt" in msg
    rc, msg = call(plan, sdf, n_con=2)
    assert rc == K.KIN_E_UNSUPPORTED and b"n_con" in msg
    assert torch.equal(X, Xin)
    # tree1: parts of bound 12, 8, 4 -- the plan is created with the link on the bound-8 part, the call names the limit
    t1 = GT.TT.case("tree1")
    m, joints = GT._mech("tree1")
    leaf = max((t1.spheres[k][0] for k in t1.parts[1]), key=lambda l: len(PT._root_path(t1.rb.tree, l)))
    p1 = GT._checker("tree1").traj_plan(joints, [m.links[leaf - 1]], dtype=torch.float64)
    assert p1.part_chain_bounds == [12, 8, 4] and p1.pose_link_parts == [1]
    X1 = torch.tensor(R.to_columns(t1.X0[:, :n_wp]), dtype=torch.float64, device="cuda")
    X1in = X1.clone()
    rc, msg = call(p1, GT._sdf("tree1"), x=X1)
    assert rc == K.KIN_E_UNSUPPORTED and b"more than 8 steps" in msg and torch.equal(X1, X1in)
    # the attached union: scene_q is needed, lds = 0 or >= n_traj * n_wp
    sp = PT.case("s-pr2")
    plan_s, att = _plan("s-pr2", torch.float64), _sdf(sp)
    Xs = torch.tensor(R.to_columns(sp.X0), dtype=torch.float64, device="cuda")
    Xsin = Xs.clone()
    sq = torch.tensor(sp.base.SQ, dtype=torch.float64, device="cuda")
    tg = torch.tensor(sp.targets, dtype=torch.float64, device="cuda")
    rc, msg = call(plan_s, att, x=Xs)
    assert rc == K.KIN_E_INVALID and b"scene_q" in msg
    rc, msg = call(plan_s, att, scene_q=sq.data_ptr(), lds=nt * n_wp - 1, x=Xs)
    assert rc == K.KIN_E_INVALID and b"lds" in msg
    assert torch.equal(Xs, Xsin)


@pytest.mark.parametrize("lengths,with_base,bounds,groups3,what", [
    ((1, 1, 1, 1, 1), False, [4] * 5, False, b"more than 4 chains"),
    ((8, 8, 2), True, [8, 8, 4], False, b"more than 20 q columns"),
    ((4, 2), False, [4, 4], True, b"at most 2 moving groups")], ids=["5-chains", "21-columns", "3-groups"])
def test_limits_by_plan(tmp_path, lengths, with_base, bounds, groups3, what):
    """kin_traj_plan_create plans past the part loop's limits, the pose link on the last branch: a star of five one-joint
    branches ("chains"); 18 joints and the base, 21 columns ("q columns"); a union of 3 moving groups ("moving groups").
    KIN_E_UNSUPPORTED naming the limit, xi untouched."""
    import kinhip
    p = tmp_path / "branches.urdf"
    p.write_text(GT._branches_urdf(lengths))
    m = kinhip.parse_urdf(str(p), with_base=with_base)
    joints = [m.find_joint(f"j{b}_{k}") for b, n in enumerate(lengths) for k in range(n)]
    sscc = kinhip.SweptSphereCollisionChecker(m)
    for b, n in enumerate(lengths):
        sscc.add_coll_sphere(m.find_link(f"b{b}_{n - 1}"), [0.02, 0, 0], 0.05)
    last = len(lengths) - 1
    plan = sscc.traj_plan(joints, [m.find_link(f"b{last}_{lengths[last] - 1}")], dtype=torch.float64)
    assert plan.n_parts == len(lengths) and plan.part_chain_bounds == bounds and plan.pose_link_parts == [last]
    nd = len(joints) + (3 if with_base else 0)
    X = torch.full((nd, 10), 0.125, dtype=torch.float64, device="cuda")
    Xin = X.clone()
    tg = torch.zeros((12, 2), dtype=torch.float64, device="cuda")
    prm = K.TrajParams(5, 1, 0.02, 0.03, 10.0, 1e-3, 1e-6, 0.5, None)
    wps, rots = (C.c_int32 * 1)(2), (C.c_int32 * 1)(0)
    pp = K.TrajPoseParams(1, C.cast(wps, C.c_void_p), C.cast(rots, C.c_void_p), 10.0, 1e-6, 1e-3, 1e-3)
    sq, lds = None, 0
    if groups3:
        ps = tmp_path / "three.urdf"
        ps.write_text(GS.THREE_GROUPS)
        sm = kinhip.parse_urdf(str(ps))
        sdf = kinhip.AttachedUnionSDF(sm, [sm.find_joint("ja"), sm.find_joint("jb")])
        s3 = torch.zeros((2, 10), dtype=torch.float64, device="cuda")
        sq, lds = s3.data_ptr(), 10
    else:
        sdf = kinhip.UnionSDF([kinhip.BoxSDF(GT._T((2.0, 2.0, 2.0)), (0.1, 0.1, 0.1))])
    L = K.lib()
    rc = L.kin_traj_opt_pose_tree_batch(plan._h, sdf._h, C.byref(prm), C.byref(pp), tg.data_ptr(), 2, sq, lds,
                                        X.data_ptr(), 10, 2, None, None, 0, None)
    torch.cuda.synchronize()
    assert rc == K.KIN_E_UNSUPPORTED and what in L.kin_last_error(), L.kin_last_error()
    assert torch.equal(X, Xin)


# ------------------------------------------------------------------------------------------------- the Python layer
def _pr2_python(scene):
    cs = PT.case("s-pr2" if scene else "pr2")
    G, b = _side(cs), _sname(cs)
    m, joints = G._mech(b)
    return cs, m, joints, G._checker(b), _sdf(cs), m.links[cs.link - 1]


@pytest.mark.parametrize("scene", [False, True])
def test_plan_trajectories_pose_equals_the_direct_call(scene):
    """plan_trajectories_pose on the PR2 (static, and with the door swinging) with X0 given = traj_opt_pose_tree_batch
    bit for bit; seeded by the IK (no X0) the constrained waypoint starts at the target and info has 6 rows."""
    import kinhip
    cs, m, joints, sscc, sdf, link = _pr2_python(scene)
    plan = _plan(cs.name, torch.float64)
    X0 = torch.tensor(R.to_columns(cs.X0), dtype=torch.float64, device="cuda")
    tg = torch.tensor(cs.targets, dtype=torch.float64, device="cuda")
    Qs = torch.tensor(np.ascontiguousarray(cs.X0[:, 0].T), dtype=torch.float64, device="cuda")
    Qg = torch.tensor(np.ascontiguousarray(cs.X0[:, -1].T), dtype=torch.float64, device="cuda")
    kw = dict(PT.KW, max_iters=8, dof_weights=cs.dof_weights)
    skw = dict(scene_q=torch.tensor(cs.base.SQ, dtype=torch.float64, device="cuda")) if scene else {}
    Xd = X0.clone()
    itd, nfd = kinhip.traj_opt_pose_tree_batch(plan, sdf, Xd, cs.n_wp, tg, cs.c, with_rot=cs.with_rot, **kw, **skw)
    pkw = dict(pose_with_rot=cs.with_rot, plan=plan, check_ends=False, **kw, **skw)
    X, it, nf = kinhip.plan_trajectories_pose(sscc, joints, sdf, Qs, Qg, cs.n_wp, link, cs.c, tg, X0=X0, **pkw)
    assert torch.equal(X, Xd) and torch.equal(it, itd) and torch.equal(nf, nfd) and nf.shape == (6, cs.n_traj)
    X, it, nf = kinhip.plan_trajectories_pose(sscc, joints, sdf, Qs, Qg, cs.n_wp, link, cs.c, tg, **pkw)
    assert nf.shape == (6, cs.n_traj) and bool(torch.isfinite(nf).all())
    with pytest.raises(ValueError):          # plan_trajectories itself keeps refusing both
        kinhip.plan_trajectories(sscc, joints, sdf, Qs, Qg, cs.n_wp, pose_link=link, pose_wp=cs.c, pose_targets=tg,
                                 check_ends=False, **skw)


@pytest.mark.parametrize("scene", [False, True])
@pytest.mark.parametrize("rows", [3, 6])
def test_pr2_full_run(scene, rows):
    """The PR2 family, 200 iterations, static and with the door closing, rows 3 and 6: the kernel's good set equals the
    restatement's (no trajectory of the restatement lies near a threshold: clearances >= 0.01 off, residuals <= 3.5e-5
    against 1e-3); every good trajectory has the library's PoseConstraint |val| < 2e-3;
    plan_trajectory(solver="GPU", partial_consts=[PoseConstraint]) on one problem returns a status."""
    import kinhip
    full = PT.pr2_full(scene, rows)
    cs, m, joints, sscc, sdf, link = _pr2_python(scene)
    out, X0, tgn = full["out"], full["X0"], full["targets"]
    n, n_wp = X0.shape[0], X0.shape[1]
    X = torch.tensor(R.to_columns(X0), dtype=torch.float64, device="cuda")
    tg = torch.tensor(tgn, dtype=torch.float64, device="cuda")
    skw = dict(scene_q=torch.tensor(full["SQ"], dtype=torch.float64, device="cuda")) if scene else {}
    it, nf = kinhip.traj_opt_pose_tree_batch(_plan(cs.name, torch.float64), sdf, X, n_wp, tg, 5, with_rot=rows == 6,
                                             dof_weights=cs.dof_weights, **R.PARAMS, **skw)
    nf = nf.cpu().numpy()
    thr = PT.KW["margin"] - PT.KW["feas"]
    good = (nf[4] < P.TOL) & (nf[5] < P.TOL) & (nf[2] >= thr)
    ref_good = P.good(out, PT.KW["margin"], PT.KW["feas"])
    print(f"pr2 {'door' if scene else 'static'} rows {rows}: kernel good {int(good.sum())}/{n} done "
          f"{int((it.cpu().numpy() <= 200).sum())}/{n}; restatement good {int(ref_good.sum())}/{n} done "
          f"{int((out['iters'] <= 200).sum())}/{n}")
    assert np.array_equal(good, ref_good) and good.any()
    pc = kinhip.PoseConstraint(6, cs.X0.shape[2], link, np.eye(4), rows == 6, m, joints)
    Xn = R.from_columns(X.cpu().numpy(), n_wp)
    Qc = torch.tensor(np.ascontiguousarray(Xn[:, 5].T), dtype=torch.float64, device="cuda")
    V, _, _ = pc.eval_batch(0, Qc, tg)
    assert float(V[:, torch.tensor(good, device="cuda")].abs().max()) < 2 * P.TOL
    # one problem through plan_trajectory: the first trajectory whose ends are clear (the layer checks them)
    ends = np.ascontiguousarray(np.concatenate([X0[:, 0], X0[:, -1]]).T)
    if scene:
        sq = full["SQ"].reshape(-1, n, n_wp)
        d_ends = full["sc"].distances_at(ends, np.ascontiguousarray(np.concatenate([sq[:, :, 0], sq[:, :, -1]], 1)))[0]
    else:
        d_ends = full["sc"].distances(ends)[0]
    t = int(np.nonzero((d_ends.min(0).reshape(2, n) > 0).all(0))[0][0])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = tgn[:9, t].reshape(3, 3).T, tgn[9:12, t]
    pc = kinhip.PoseConstraint(6, cs.X0.shape[2], link, T, rows == 6, m, joints)
    sq1 = dict(scene_q=full["SQ"][:, t * n_wp:(t + 1) * n_wp]) if scene else {}
    q_seq, status = kinhip.plan_trajectory(sscc, joints, sdf, X0[t, 0], X0[t, -1], n_wp, solver="GPU",
                                           partial_consts=[pc], maxiter=20, **sq1)
    assert q_seq.shape == (cs.X0.shape[2], n_wp) and status in (":SUCCESS", ":MAXEVAL_REACHED")
