"""kin_traj_opt_scene_batch (k_traj_scene) on the GPU against the CPU restatement (tests/trajopt_scene_ref.py) on the
cases of tests/trajopt_scene_cases.py: Fetch and the PR2 (both arms, the base) at the fridge with its door swinging
over the waypoints and a fridge base per trajectory, a random tree with parts of bound 16 and 4 against a written
two-group scene (an oblique unnormalised revolute axis), a 19-column chain at n_wp = 64 against a drawer with 70
boxes, one scene state for the launch (lds = 0) and padded arrays (lds > n_traj * n_wp).

Bounds.  One iteration, fp64: the project's 1e-9.  Eight iterations, fp64:
    TOL8_SCENE = max(10 x SPREAD8_SCENE, 4 x D8_STATIC)
SPREAD8_SCENE is the restatement's own forward / reversed spread over the cases, measured on the CPU
(tests/test_trajopt_scene.py); D8_STATIC is the largest 8-iteration deviation from the restatement of the existing
kernels (unchanged by the scene variant: kin_traj_opt_batch's k_traj for the single-chain plans, kin_traj_opt_tree_batch's
k_traj_tree for the multi-part ones) on the frozen sub-cases -- the same robot, boxes and X0 with the scene frozen at
one state (the middle waypoint of trajectory 0, and of trajectory 1) as a static union; 4 is the project's margin on a
measured rounding figure.  fp32, one iteration: DELTA32_SCENE = 4 x D32_STATIC capped at 3e-4, D32_STATIC the same
measurement in fp32.  test_frozen_subcases_on_the_existing_kernels re-measures both and holds them to the constants
in tests/trajopt_scene_cases.py, where the measured values are recorded: D8_STATIC = 6.0e-12 (5.90e-12 measured),
D32_STATIC = 2.3e-6, so TOL8_SCENE = max(5.0e-11, 2.4e-11) = 5.0e-11 (below the 1e-10 at which the scene frames would be
doing something other than rounding) and DELTA32_SCENE = 9.2e-6.

Measured on an MI355X, kin_traj_opt_scene_batch against the restatement:
  case            fp64 1 it. (X, info)   fp64 8 it. |dX|   fp64 8 it. |d merit|   fp32 1 it. |X32 - X_ref|
  fetch                2.8e-14              5.2e-14            2.8e-14                 1.2e-6
  fetch-one            8.3e-17              7.2e-16            1.3e-16                 5.7e-8
  pr2                  1.6e-14              4.7e-15            1.2e-15                 1.3e-6
  tree0                4.2e-14              6.5e-13            1.8e-14                 3.5e-6
  wide                 3.6e-13              2.9e-12            3.4e-11                 1.9e-6
  fetch-uniform        1.1e-14              8.1e-13            6.9e-14                 1.1e-6
  fetch-padded         2.8e-14              5.2e-14            2.8e-14                 1.2e-6
wide's 3.4e-11 in the merit is 6.8 x its own forward / reversed spread (4.94e-12; merits of 50-190 over 62 interior
waypoints and 70 boxes) and 9 x the existing k_traj on its frozen sub-case (3.65e-12).  With lds = 0 against the existing
entry points on the static snapshot: fetch 4.8e-14 (X) / 4.0e-15 (merit), pr2 4.0e-15 / 7.1e-14.  The door frozen at its
first / last angle moves trajectory 0 of fetch by 0.80 / 0.24 rad after 8 iterations."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import trajopt_ref as R
import trajopt_scene_cases as SC
from trajopt_scene_cases import D8_STATIC, D32_STATIC, SPREAD8_SCENE

pytestmark = pytest.mark.gpu

TOL1 = 1e-9
TOL8_SCENE = max(10 * SPREAD8_SCENE, 4 * D8_STATIC)
DELTA32_SCENE = min(4 * D32_STATIC, 3e-4)
assert TOL8_SCENE <= 1e-10   # (beyond: the scene frames would be doing something other than rounding)
BASE_CASES = ["fetch", "fetch-one", "pr2", "tree0", "wide"]
_DIR = {}


@pytest.fixture(scope="module", autouse=True)
def _urdf_dir(tmp_path_factory):
    _DIR["d"] = str(tmp_path_factory.mktemp("trajscene"))


@functools.lru_cache(maxsize=None)
def _mech(name):
    import kinhip
    cs = SC.case(name)
    rb = cs.rb
    p = rb.path
    if p is None:
        p = os.path.join(_DIR["d"], f"{rb.name}.urdf")
        if not os.path.exists(p):
            with open(p, "w") as f:
                f.write(rb.text)
    m = kinhip.parse_urdf(p, with_base=cs.with_base)
    for j, a in zip(rb.held, rb.held_ang):
        m.set_joint_angle(m.joints[j - 1], float(a))
    return m, [m.joints[j - 1] for j in rb.q_ids]


@functools.lru_cache(maxsize=None)
def _att(name):
    import kinhip
    cs = SC.case(name)
    sm = kinhip.parse_urdf(cs.scene_path, with_base=cs.scene_base)
    att = kinhip.AttachedUnionSDF(sm, [sm.find_joint(n) for n in cs.scene_joints])
    assert att.n_scene_cols == cs.sc.n_scene_cols and len(att.links) == len(cs.sc.boxes)
    return att


def _static(sc):
    import kinhip
    return kinhip.UnionSDF([kinhip.BoxSDF(T, w) for T, w in zip(sc.box_poses, sc.box_widths)])


@functools.lru_cache(maxsize=None)
def _checker(name):
    import kinhip
    cs = SC.case(name)
    m, _ = _mech(name)
    sscc = kinhip.SweptSphereCollisionChecker(m)
    for l, c, r in cs.spheres:
        sscc.add_coll_sphere(m.links[l - 1], c, r)
    return sscc


@functools.lru_cache(maxsize=None)
def _plan(name, dtype):
    cs = SC.case(name)
    plan = _checker(name).plan(_mech(name)[1], dtype=dtype)
    assert plan.n_parts == len(cs.parts) and plan.part_chain_bounds == cs.bounds, (name, plan.part_chain_bounds)
    return plan


def _guarded(rows, cols, ld, dtype, pad):
    """A [rows, cols] view inside a [rows + 2, ld] tensor: a row of SENT before and after, the columns past `cols`
    filled with `pad`."""
    big = torch.full((rows + 2, ld), SC.SENT, dtype=dtype, device="cuda")
    big[1:rows + 1, cols:] = pad
    return big, big[1:rows + 1, :cols]


def _untouched(big, rows, cols, pad):
    sent = torch.tensor(SC.SENT).to(big.dtype)           # (as torch.full wrote it: -7 in the int32 array)
    edge = bool((big[0] == sent).all()) and bool((big[rows + 1] == sent).all())
    p = big[1:rows + 1, cols:]
    return edge and bool((torch.isnan(p) if pad != pad else p == pad).all())


def _gpu_run(name, max_iters, dtype=torch.float64, X0=None, SQ=None, nan_pad=False, static=None):
    """-> X [nt, n_wp, nd], iters, info (numpy, fp64) through kin_traj_opt_scene_batch, or with `static` (a frozen
    SceneBase) through the existing entry point for the plan (kin_traj_opt_batch / kin_traj_opt_tree_batch).  Every array
    the call touches is a view with a sentinel row before and after and PAD more columns (ldx, lds, ldi > the
    columns used; nan_pad: NaN there in xi and scene_q); every run checks what the kernel must leave alone: the guards,
    the padding, the end columns, the off-chain columns, and that the interior stays within the limits."""
    import kinhip
    cs = SC.case(name)
    X0 = cs.X0 if X0 is None else X0
    SQ = cs.SQ if SQ is None else SQ
    nt, n_wp, nd = X0.shape
    cols = nt * n_wp
    pad = float("nan") if nan_pad else SC.SENT
    bigx, X = _guarded(nd, cols, cols + SC.PAD, dtype, pad)
    Xin = torch.tensor(R.to_columns(X0), dtype=dtype, device="cuda")
    X.copy_(Xin)
    bigi, it = _guarded(1, nt, nt + 3, torch.int32, int(SC.SENT - 0.75))
    bign, nf = _guarded(4, nt, nt + 5, dtype, SC.SENT)
    plan = _plan(name, dtype)
    kw = dict(SC.KW, max_iters=max_iters, dof_weights=cs.dof_weights, iters=it[0], info=nf)
    if static is not None:
        opt = kinhip.traj_opt_tree_batch if len(cs.parts) > 1 else kinhip.traj_opt_batch
        opt(plan, _static(static), X, n_wp, **kw)
    else:
        nc = cs.sc.n_scene_cols
        if SQ.ndim == 1:
            bigs, sq = _guarded(1, nc, nc + 3, dtype, SC.SENT)
            sq = sq[0]
            sq.copy_(torch.tensor(SQ, dtype=dtype))
        else:
            bigs, sq = _guarded(nc, cols, cols + SC.PAD + 2, dtype, pad)
            sq.copy_(torch.tensor(SQ, dtype=dtype))
        kinhip.traj_opt_scene_batch(plan, _att(name), X, n_wp, sq, **kw)
        torch.cuda.synchronize()
        assert _untouched(bigs, 1 if SQ.ndim == 1 else nc, nc if SQ.ndim == 1 else cols, SC.SENT if SQ.ndim == 1 else pad)
        assert torch.equal(sq, torch.tensor(SQ, dtype=dtype, device="cuda"))
    torch.cuda.synchronize()
    assert _untouched(bigx, nd, cols, pad) and _untouched(bigi, 1, nt, int(SC.SENT - 0.75)) and _untouched(bign, 4, nt, SC.SENT)
    ends = torch.arange(nt, device="cuda") * n_wp
    assert torch.equal(X[:, ends], Xin[:, ends]) and torch.equal(X[:, ends + n_wp - 1], Xin[:, ends + n_wp - 1])
    for c in cs.off_cols:
        assert torch.equal(X[int(c)], Xin[int(c)])
    Xo = R.from_columns(X.double().cpu().numpy(), n_wp)
    ndt = np.float32 if dtype == torch.float32 else np.float64
    assert np.all(Xo[:, 1:-1] >= cs.sc.lo.astype(ndt)) and np.all(Xo[:, 1:-1] <= cs.sc.hi.astype(ndt))
    return Xo, it[0].cpu().numpy().copy(), nf.double().cpu().numpy()


def _ref_name(name):
    return "fetch" if name == "fetch-padded" else name


@pytest.mark.parametrize("name", SC.CASES)
def test_first_iterates(name):
    """fp64, the kernel from the restatement's X0.  One iteration: X and info[0:3] equal the restatement's to 1e-9,
    info[3] and iters are equal on the determined trajectories.  max_iters = 1..8: the accept sequences and the
    iteration counts are equal on the determined trajectories; after 8 iterations X and the merit are within
    TOL8_SCENE.  fetch-uniform runs with lds = 0; fetch-padded with NaN in the padding of scene_q and xi."""
    cs = SC.case(name)
    nt = cs.n_traj
    nanp = name == "fetch-padded"
    ref1 = SC.ref_run(_ref_name(name), 1)
    X, it, nf = _gpu_run(name, 1, nan_pad=nanp)
    e1 = (np.abs(X - ref1["X"]).max(), np.abs(nf[:3] - ref1["info"][:3]).max())
    print(f"{name} bounds {cs.bounds} n_wp {cs.n_wp}: 1 iteration max|dX| = {e1[0]:.2e}, max|d info| = {e1[1]:.2e}")
    det = ref1["determined"]
    assert np.array_equal(nf[3][det], ref1["info"][3][det]) and np.array_equal(it[det], ref1["iters"][det])
    assert e1[0] <= TOL1 and e1[1] <= TOL1
    ref8 = SC.ref_run(_ref_name(name), 8)
    nacc = [np.zeros(nt)]
    for k in range(1, 9):
        X, it, nf = _gpu_run(name, k, nan_pad=nanp)
        nacc.append(nf[3])
    seq = np.diff(np.array(nacc), axis=0)
    ref_seq = np.maximum(ref8["accepts"], 0)
    ref_seq = np.vstack([ref_seq, np.zeros((8 - ref_seq.shape[0], nt))])
    det = ref8["determined"]
    e8 = (np.abs(X - ref8["X"])[det].max(), np.abs(nf[0] - ref8["info"][0])[det].max())
    print(f"{name}: 8 iterations max|dX| = {e8[0]:.2e}, max|d merit| = {e8[1]:.2e}, determined {int(det.sum())}/{nt}")
    assert det.sum() >= (1 if nt == 1 else 5)
    assert np.array_equal(seq[:, det], ref_seq[:, det])
    assert np.array_equal(it[det], ref8["iters"][det])
    assert e8[0] <= TOL8_SCENE and e8[1] <= TOL8_SCENE


def test_frozen_subcases_on_the_existing_kernels():
    """The inputs of TOL8_SCENE and DELTA32_SCENE: the existing entry points (k_traj for the single-chain plans,
    k_traj_tree for pr2 and tree0) on every frozen sub-case against its own restatement -- 8 iterations in fp64
    (D8_STATIC), one in fp32 (D32_STATIC).  The measured maxima are printed and held to the recorded constants."""
    d8 = d32 = 0.0
    for name in BASE_CASES:
        cs = SC.case(name)
        for k, state in enumerate(SC.frozen_states(name)):
            fz = cs.sc.frozen(state)
            r8, r1 = SC.frozen_ref(name, k, 8), SC.frozen_ref(name, k, 1)
            det = r8["determined"]
            X, _, nf = _gpu_run(name, 8, static=fz)
            e8 = max(np.abs(X - r8["X"])[det].max(), np.abs(nf[0] - r8["info"][0])[det].max()) if det.any() else 0.0
            X32, _, _ = _gpu_run(name, 1, dtype=torch.float32, static=fz)
            e32 = np.abs(X32 - r1["X"]).max()
            print(f"{name} frozen at state {k} (bounds {cs.bounds}): fp64 8 iterations {e8:.2e} on {int(det.sum())} "
                  f"determined, fp32 1 iteration {e32:.2e}")
            d8, d32 = max(d8, e8), max(d32, e32)
    print(f"D8_STATIC measured {d8:.3e} (recorded {D8_STATIC:.3e}), D32_STATIC measured {d32:.3e} (recorded {D32_STATIC:.3e})")
    assert d8 <= D8_STATIC and d32 <= D32_STATIC


@pytest.mark.parametrize("name", SC.CASES)
def test_fp32(name):
    """fp32: after one iteration |X32 - X_ref| <= DELTA32_SCENE against the fp64 restatement; the merit does not
    increase over runs of 1, 2, 4, 8 iterations and info[3] <= k."""
    ref1 = SC.ref_run(_ref_name(name), 1)
    last = None
    for k in (1, 2, 4, 8):
        X, it, nf = _gpu_run(name, k, dtype=torch.float32, nan_pad=name == "fetch-padded")
        if k == 1:
            e = np.abs(X - ref1["X"]).max()
            print(f"{name}: fp32 1 iteration max|X32 - X_ref| = {e:.2e}")
            assert e <= DELTA32_SCENE
        if last is not None:
            assert np.all(nf[0] <= last)
        assert np.all(nf[3] <= k)
        last = nf[0]


@pytest.mark.parametrize("name", ["fetch", "pr2"])
def test_frozen_equivalence(name):
    """lds = 0: the result equals the existing entry point's (k_traj for Fetch's single chain, k_traj_tree for the
    PR2's two parts) on the static snapshot of that scene state, to 2 x TOL8_SCENE after 8 iterations on the
    determined trajectories, with equal iteration counts and accepted steps there."""
    cs = SC.case(name)
    state = SC.frozen_states(name)[0]
    det = SC.frozen_ref(name, 0, 8)["determined"]
    Xs, its, nfs = _gpu_run(name, 8, SQ=state)
    Xf, itf, nff = _gpu_run(name, 8, static=cs.sc.frozen(state))
    e = (np.abs(Xs - Xf)[det].max(), np.abs(nfs[0] - nff[0])[det].max())
    print(f"{name}: scene kernel with lds = 0 against the static snapshot: max|dX| = {e[0]:.2e}, max|d merit| = {e[1]:.2e}")
    assert det.any() and np.abs(Xs - cs.X0).max() > 1e-6
    assert np.array_equal(its[det], itf[det]) and np.array_equal(nfs[3][det], nff[3][det])
    assert e[0] <= 2 * TOL8_SCENE and e[1] <= 2 * TOL8_SCENE


def test_the_scene_is_per_waypoint():
    """fetch, 8 iterations: the result differs by more than 1e-6 from both frozen-door runs -- every trajectory's door
    held at its first angle, and at its last -- on trajectory 0, whose spheres are at the door (a kernel that
    indexes scene_q by trajectory, or by lane, returns one of them or reads another trajectory's state)."""
    cs = SC.case("fetch")
    X, _, _ = _gpu_run("fetch", 8)
    door = cs.SQ[0].reshape(cs.n_traj, cs.n_wp)
    for w in (0, cs.n_wp - 1):
        SQ = cs.SQ.copy()
        SQ[0] = np.repeat(door[:, w], cs.n_wp)
        Xw, _, _ = _gpu_run("fetch", 8, SQ=SQ)
        d = np.abs(X - Xw).max(axis=(1, 2))
        print(f"door frozen at waypoint {w}: max|dX| per trajectory {np.array2string(d, precision=2)}")
        assert d[0] > 1e-6


@pytest.mark.parametrize("name", ["fetch", "pr2", "tree0", "wide", "fetch-uniform"])
def test_info_matches_coll_batch_scene(name):
    """After 40 iterations info[2] is the minimum over the interior waypoints of kin_coll_batch_scene's min_dist on the
    returned X with the same scene_q (1e-9)."""
    cs = SC.case(name)
    X, it, nf = _gpu_run(name, 40)
    Q = torch.tensor(R.to_columns(X), dtype=torch.float64, device="cuda")
    sq = torch.tensor(cs.SQ, dtype=torch.float64, device="cuda")
    _, _, mn = _plan(name, torch.float64).run(_att(name), Q, dists=False, min_dist=True, scene_q=sq)
    dm = mn.cpu().numpy().reshape(-1, cs.n_wp)[:, 1:-1].min(1)
    assert np.abs(nf[2] - dm).max() <= 1e-9


def _subset(cs, idx):
    return cs.X0[idx], np.concatenate([cs.SQ[:, t * cs.n_wp:(t + 1) * cs.n_wp] for t in idx], axis=1)


@pytest.mark.parametrize("name", ["tree0", "wide"])
def test_packing_independence(name):
    """Parts of bound 16 and 4 at n_wp = 33, and n_wp = 64 with the halved workgroup: trajectory t of the 9-batch is
    bit-equal to the same trajectory (with its scene columns) run alone and run at another segment position."""
    cs = SC.case(name)
    X, it, nf = _gpu_run(name, 8)
    for t in (0, 4, 8):
        Xs, Ss = _subset(cs, [t])
        Xa, ia, na = _gpu_run(name, 8, X0=Xs, SQ=Ss)
        assert np.array_equal(Xa[0], X[t]) and ia[0] == it[t] and np.array_equal(na[:, 0], nf[:, t])
        Xs, Ss = _subset(cs, [1, 2, 3, 5, 6, t, 7])
        Xb, ib, nb = _gpu_run(name, 8, X0=Xs, SQ=Ss)
        assert np.array_equal(Xb[5], X[t]) and ib[5] == it[t] and np.array_equal(nb[:, 5], nf[:, t])


def test_capture():
    """After the plan's first (staging) call for an n_wp, a call captured in a graph replays the eager results bit for
    bit, twice."""
    import kinhip
    name = "pr2"
    cs = SC.case(name)
    plan, att = _plan(name, torch.float64), _att(name)
    kw = dict(SC.KW, max_iters=20, dof_weights=cs.dof_weights)
    X0 = torch.tensor(R.to_columns(cs.X0), dtype=torch.float64, device="cuda")
    sq = torch.tensor(cs.SQ, dtype=torch.float64, device="cuda")
    Xe = X0.clone()
    ite, nfe = kinhip.traj_opt_scene_batch(plan, att, Xe, cs.n_wp, sq, **kw)   # eager; also stages the table
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
            kinhip.traj_opt_scene_batch(plan, att, Xg, cs.n_wp, sq, iters=itg, info=nfg, stream=s, **kw)
        for rep in range(2):
            g.replay()
            s.synchronize()
            assert torch.equal(Xg, Xe) and torch.equal(itg, ite) and torch.equal(nfg, nfe), rep
    assert not torch.equal(Xe, X0)


def _ends_problem(cs):
    """For the start / goal asserts: trajectory 0 of fetch with its fridge base; start = its middle waypoint (a sphere
    at the door), goal = its last.  -> (q_s, q_g, base, a_bad, a_ok): at door angle a_bad the start is in collision,
    at a_ok start and goal are clear (found with the restatement on a grid of door angles)."""
    q_s, q_g = cs.X0[0, cs.n_wp // 2], cs.X0[0, -1]
    base = cs.SQ[1:, 0]
    grid = np.linspace(0.0, 2.0, 81)
    sq = np.vstack([grid, np.repeat(base[:, None], grid.size, axis=1)])
    ds = cs.sc.distances_at(np.repeat(q_s[:, None], grid.size, axis=1), sq)[0].min(0)
    dg = cs.sc.distances_at(np.repeat(q_g[:, None], grid.size, axis=1), sq)[0].min(0)
    bad, ok = np.flatnonzero((ds < -0.01) & (dg > 0.01)), np.flatnonzero((ds > 0.01) & (dg > 0.01))
    assert bad.size and ok.size
    return q_s, q_g, base, float(grid[bad[0]]), float(grid[ok[0]])


def test_python_layer():
    """plan_trajectories with an AttachedUnionSDF dispatches to kin_traj_opt_scene_batch for a single-chain plan (fetch)
    and a multi-part plan (pr2): bit-equal to the direct call, for scene_q of shape (n_scene_cols, n_traj * n_wp),
    (n_scene_cols, n_traj) (expanded per waypoint) and (n_scene_cols,).  The start / goal asserts use the scene state
    of waypoint 0 and of waypoint n_wp - 1: a door that hits the start only at waypoint 0's state raises, the same
    door angle at an interior waypoint does not.  pose_link with an attached union raises; plan_trajectory(solver=
    "GPU", scene_q=...) runs."""
    import kinhip
    for name in ("fetch", "pr2"):
        cs = SC.case(name)
        m, joints = _mech(name)
        sscc, att = _checker(name), _att(name)
        Qs, Qg = cs.X0[:, 0].T.copy(), cs.X0[:, -1].T.copy()
        kw = dict(SC.KW, max_iters=8, dof_weights=cs.dof_weights, X0=R.to_columns(cs.X0), check_ends=False,
                  plan=_plan(name, torch.float64))
        per_traj = cs.SQ.reshape(-1, cs.n_traj, cs.n_wp)[:, :, 0]
        for SQ, direct in ((cs.SQ, cs.SQ), (per_traj, np.repeat(per_traj, cs.n_wp, axis=1)), (cs.SQ[:, 0], cs.SQ[:, 0])):
            X, it, nf = kinhip.plan_trajectories(sscc, joints, att, Qs, Qg, cs.n_wp,
                                                 scene_q=torch.tensor(SQ, dtype=torch.float64, device="cuda"), **kw)
            Xd, itd, nfd = _gpu_run(name, 8, SQ=np.ascontiguousarray(direct))
            assert np.array_equal(R.from_columns(X.cpu().numpy(), cs.n_wp), Xd) and np.array_equal(it.cpu().numpy(), itd)
            assert np.array_equal(nf.cpu().numpy(), nfd)
        with pytest.raises(ValueError):
            kinhip.plan_trajectories(sscc, joints, att, Qs, Qg, cs.n_wp, **kw)                  # no scene_q
    cs = SC.case("fetch")
    m, joints = _mech("fetch")
    sscc, att = _checker("fetch"), _att("fetch")
    q_s, q_g, base, a_bad, a_ok = _ends_problem(cs)
    n_wp = cs.n_wp

    def sq_of(door):
        return torch.tensor(np.vstack([door, np.repeat(base[:, None], n_wp, axis=1)]), dtype=torch.float64, device="cuda")
    door = np.full(n_wp, a_ok)
    door[3] = a_bad                                       # an interior waypoint's state: not what the asserts look at
    X, it, nf = kinhip.plan_trajectories(sscc, joints, att, q_s, q_g, n_wp, scene_q=sq_of(door), max_iters=5)
    assert X.shape == (cs.n_dof, n_wp) and bool(torch.isfinite(nf).all())
    for w in (0, n_wp - 1):
        door = np.full(n_wp, a_ok)
        door[w] = a_bad
        qa, qb = (q_s, q_g) if w == 0 else (q_g, q_s)     # the config that a_bad hits sits at waypoint w
        with pytest.raises(AssertionError):
            kinhip.plan_trajectories(sscc, joints, att, qa, qb, n_wp, scene_q=sq_of(door), max_iters=5)
    with pytest.raises(ValueError):
        kinhip.plan_trajectories(sscc, joints, att, q_s, q_g, n_wp, scene_q=sq_of(np.full(n_wp, a_ok)),
                                 pose_link=m.find_link("gripper_link"), pose_wp=2, pose_targets=np.eye(4))
    q_seq, status = kinhip.plan_trajectory(sscc, joints, att, q_s, q_g, n_wp, solver="GPU", maxiter=20,
                                           scene_q=sq_of(np.full(n_wp, a_ok)).cpu().numpy())
    assert q_seq.shape == (cs.n_dof, n_wp) and status in (":SUCCESS", ":MAXEVAL_REACHED")
    assert np.array_equal(q_seq[:, 0], q_s) and np.array_equal(q_seq[:, -1], q_g)


THREE_GROUPS = """<robot name="three">
  <link name="root"><collision><origin xyz="2 2 2"/><geometry><box size="0.1 0.1 0.1"/></geometry></collision></link>
  <link name="a"><collision><origin xyz="2 2 2"/><geometry><box size="0.1 0.1 0.1"/></geometry></collision></link>
  <link name="b"><collision><origin xyz="2 2 2"/><geometry><box size="0.1 0.1 0.1"/></geometry></collision></link>
  <joint name="ja" type="revolute"><parent link="root"/><child link="a"/><origin xyz="0 0 0"/><axis xyz="0 0 1"/>
    <limit lower="-1" upper="1" effort="1" velocity="1"/></joint>
  <joint name="jb" type="prismatic"><parent link="root"/><child link="b"/><origin xyz="0 0 0"/><axis xyz="1 0 0"/>
    <limit lower="-1" upper="1" effort="1" velocity="1"/></joint>
</robot>
"""


def test_limits_that_need_a_plan(tmp_path):
    """A union of 3 moving groups is KIN_E_UNSUPPORTED and the message names the limit; a static union is KIN_E_INVALID
    and names kin_traj_opt_tree_batch; 0 < lds < n_traj * n_wp is KIN_E_INVALID ("lds"); a null scene_q with scene
    columns too.  X stays as given."""
    import kinhip
    from kinhip import _lib as K
    name = "fetch"
    cs = SC.case(name)
    plan = _plan(name, torch.float64)
    L = K.lib()
    prm = K.TrajParams(cs.n_wp, 5, 0.02, 0.03, 10.0, 1e-3, 1e-6, 0.5, None)
    Xin = torch.tensor(R.to_columns(cs.X0), dtype=torch.float64, device="cuda")
    X = Xin.clone()
    cols = cs.n_traj * cs.n_wp
    sq = torch.tensor(cs.SQ, dtype=torch.float64, device="cuda")
    tail = (X.data_ptr(), X.stride(0), cs.n_traj, None, None, 0, None)
    p = tmp_path / "three.urdf"
    p.write_text(THREE_GROUPS)
    sm = kinhip.parse_urdf(str(p))
    three = kinhip.AttachedUnionSDF(sm, [sm.find_joint("ja"), sm.find_joint("jb")])
    s3 = torch.zeros((2, cols), dtype=torch.float64, device="cuda")
    assert L.kin_traj_opt_scene_batch(plan._h, three._h, C.byref(prm), s3.data_ptr(), cols, *tail) == K.KIN_E_UNSUPPORTED
    assert b"at most 2 moving groups" in L.kin_last_error()
    static = _static(cs.sc.frozen(cs.mid_state))
    assert L.kin_traj_opt_scene_batch(plan._h, static._h, C.byref(prm), sq.data_ptr(), cols, *tail) == K.KIN_E_INVALID
    assert b"kin_traj_opt_tree_batch" in L.kin_last_error()
    att = _att(name)
    assert L.kin_traj_opt_scene_batch(plan._h, att._h, C.byref(prm), sq.data_ptr(), cols - 1, *tail) == K.KIN_E_INVALID
    assert b"lds" in L.kin_last_error()
    assert L.kin_traj_opt_scene_batch(plan._h, att._h, C.byref(prm), None, cols, *tail) == K.KIN_E_INVALID
    assert b"scene_q" in L.kin_last_error()
    torch.cuda.synchronize()
    assert torch.equal(X, Xin)
    assert L.kin_traj_opt_scene_batch(plan._h, att._h, C.byref(prm), sq.data_ptr(), cols, *tail) == K.KIN_OK, L.kin_last_error()
    torch.cuda.synchronize()
    assert not torch.equal(X, Xin)


def test_pr2_full_run():
    """PR2 at the fridge, both arms and the base, 6 trajectories, 200 iterations, the door closing from 2.0 to 1.2 over
    the waypoints, fp64: iteration counts equal the restatement's on the determined trajectories, the done sets are
    equal, and every done trajectory is feasible under the kin_coll_batch_scene re-evaluation (every interior waypoint at
    its own door angle: min distance >= margin - feas)."""
    cs = SC.case("pr2")
    sc, SQ, ref = SC.pr2_full()
    n = SC.N_PR2_FULL
    X, it, nf = _gpu_run("pr2", 200, X0=cs.X0[:n], SQ=SQ)
    det = ref["determined"]
    done = it <= 200
    print(f"pr2 at the closing door: done {int(done.sum())}/{n} (restatement {int((ref['iters'] <= 200).sum())}), "
          f"determined {int(det.sum())}")
    assert np.array_equal(it[det], ref["iters"][det])
    assert np.array_equal(done, ref["iters"] <= 200)
    Q = torch.tensor(R.to_columns(X), dtype=torch.float64, device="cuda")
    _, _, mn = _plan("pr2", torch.float64).run(_att("pr2"), Q, dists=False, min_dist=True,
                                               scene_q=torch.tensor(SQ, dtype=torch.float64, device="cuda"))
    dm = mn.cpu().numpy().reshape(n, cs.n_wp)[:, 1:-1].min(1)
    assert np.abs(nf[2] - dm).max() <= 1e-9
    assert done.any() and np.all(dm[done] >= SC.KW["margin"] - SC.KW["feas"])
