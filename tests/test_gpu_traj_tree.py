"""kin_traj_opt_tree_batch (k_traj_tree) on the GPU against the CPU restatement (tests/trajopt_ref.py) on the cases of
tests/trajopt_tree_cases.py: robots with spheres on two to four chains -- the two-arm robot, the PR2 with both arms
and the base (the reference's fridge_demo.jl shape) and four seeded random trees whose parts have the chain bounds
(16, 4), (12, 8, 4), (8, 8, 4, 4), (8, 4, 4, 4), asserted through kin_plan_part_count / kin_plan_part_chain_bound.

Bounds.  One iteration, fp64: the project's 1e-9.  Eight iterations, fp64:
    TOL8_TREE = max(TOL8_RC, 10 x SPREAD8_TREE, 4 x D8_PARTS)
TOL8_RC = 1.6e-13 is the existing suite's (tests/test_gpu_traj_random_chains.py); SPREAD8_TREE = 1.8e-12 is the
restatement's own forward / reversed spread over the cases, measured on the CPU (tests/test_trajopt_tree.py); D8_PARTS
is the largest 8-iteration deviation from the restatement of the existing kin_traj_opt_batch kernel (the parent
commit's code, unchanged) on the single-part sub-cases -- the same robot, boxes and X0 with one part's spheres only --
whose FK rounding the spread does not contain; 4 is the project's margin on a measured rounding figure.  That
kernel keeps 12 columns for chain bounds <= 8, so the sub-cases it can run are the six with at most 12 columns or a
bound of 12 / 16: both arms of twoarm without and with the base, the bound-16 part of tree0, the bound-12 part of
tree1.  fp32, one
iteration: DELTA32_TREE = max(DELTA32, 4 x D32_PARTS) capped at 3e-4, D32_PARTS the same single-part measurement
in fp32.  test_single_parts_on_the_existing_kernel re-measures both and holds them to the constants below.

Measured on an MI355X.  kin_traj_opt_batch on the single-part sub-cases (fp64 8 iterations, max of |dX| and
|d merit|; fp32 1 iteration |X32 - X_ref|):
  twoarm-nobase part 0 (bound 8)   3.1e-15   4.2e-7        twoarm-base part 1 (bound 8)   1.6e-15   6.0e-7
  twoarm-nobase part 1 (bound 8)   3.6e-15   4.0e-6        tree0 part 0 (bound 16)        3.5e-15   1.6e-5
  twoarm-base part 0 (bound 8)     1.8e-14   2.9e-6        tree1 part 0 (bound 12)        1.6e-13   9.0e-7
so D8_PARTS = 1.6e-13, D32_PARTS = 1.7e-5 (rounded up), TOL8_TREE = max(1.6e-13, 1.8e-11, 6.4e-13) = 1.8e-11 and
DELTA32_TREE = max(1.8e-5, 6.8e-5) = 6.8e-5.  kin_traj_opt_tree_batch against the restatement:
  case            fp64 1 it. (X, info)   fp64 8 it. |dX|   fp64 8 it. |d merit|   fp32 1 it. |X32 - X_ref|
  twoarm-nobase        1.1e-14              2.0e-15            4.9e-15                 4.1e-7
  twoarm-base          1.1e-15              8.9e-16            9.4e-16                 6.0e-7
  pr2                  2.3e-14              4.0e-14            3.1e-15                 5.4e-7
  tree0                2.1e-14              5.8e-12            7.5e-13                 1.6e-5
  tree1                3.0e-14              1.1e-14            1.5e-14                 9.9e-7
  tree2                8.2e-14              1.2e-13            2.2e-12                 1.4e-6
  tree3                1.2e-14              3.2e-15            1.6e-15                 2.8e-6
tree0's 5.8e-12 is 3.2 x its own forward / reversed spread (1.8e-12): one trajectory of that case amplifies rounding.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import trajopt_ref as R
import trajopt_tree_cases as TT
from conftest import ARM, golden
from test_gpu_traj_random_chains import DELTA32, TOL8_RC
from test_trajopt_tree import SPREAD8_TREE

pytestmark = pytest.mark.gpu

TOL1 = 1e-9
D8_PARTS = 1.6e-13      # measured 1.58e-13 (the bound-12 part of tree1)
D32_PARTS = 1.7e-5      # measured 1.61e-5 (the bound-16 part of tree0)
TOL8_TREE = max(TOL8_RC, 10 * SPREAD8_TREE, 4 * D8_PARTS)
DELTA32_TREE = min(max(DELTA32, 4 * D32_PARTS), 3e-4)
assert TOL8_TREE <= 1e-10   # (beyond: the part sum would be doing something other than rounding)
_DIR = {}


@pytest.fixture(scope="module", autouse=True)
def _urdf_dir(tmp_path_factory):
    _DIR["d"] = str(tmp_path_factory.mktemp("trajtrees"))


@functools.lru_cache(maxsize=None)
def _mech(name):
    import kinhip
    cs = TT.case(name)
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
def _sdf(name):
    import kinhip
    cs = TT.case(name)
    return kinhip.UnionSDF([kinhip.BoxSDF(T, w) for T, w in zip(cs.sc.box_poses, cs.sc.box_widths)])


@functools.lru_cache(maxsize=None)
def _checker(name, spheres=None):
    """The case's checker with all spheres, or with the given ones only (indices into cs.spheres)."""
    import kinhip
    cs = TT.case(name)
    m, _ = _mech(name)
    sscc = kinhip.SweptSphereCollisionChecker(m)
    for k in (range(len(cs.spheres)) if spheres is None else spheres):
        l, c, r = cs.spheres[k]
        sscc.add_coll_sphere(m.links[l - 1], c, r)
    return sscc


@functools.lru_cache(maxsize=None)
def _plan(name, dtype, spheres=None):
    cs = TT.case(name)
    plan = _checker(name, spheres).plan(_mech(name)[1], dtype=dtype)
    if spheres is None:
        assert plan.n_parts == len(cs.parts) and plan.part_chain_bounds == cs.bounds, (name, plan.part_chain_bounds)
    return plan


def _gpu_run(name, max_iters, dtype=torch.float64, weights=True, X0=None, spheres=None, tree=True):
    """-> X [nt, n_wp, nd], iters, info (numpy, fp64), through kin_traj_opt_tree_batch (tree) or kin_traj_opt_batch.
    X is a view into a wider tensor (ldx = n_traj * n_wp + PAD, one more row) filled with SENT; every run checks
    what the kernel must leave alone: the padding, the end columns, the off-chain columns, and that the interior
    stays within the limits."""
    import kinhip
    cs = TT.case(name)
    X0 = cs.X0 if X0 is None else X0
    nt, n_wp, nd = X0.shape
    cols = nt * n_wp
    big = torch.full((nd + 1, cols + TT.PAD), TT.SENT, dtype=dtype, device="cuda")
    X = big[:nd, :cols]
    Xin = torch.tensor(R.to_columns(X0), dtype=dtype, device="cuda")
    X.copy_(Xin)
    w = cs.dof_weights if weights else None
    opt = kinhip.traj_opt_tree_batch if tree else kinhip.traj_opt_batch
    it, nf = opt(_plan(name, dtype, spheres), _sdf(name), X, n_wp, max_iters=max_iters, dof_weights=w, **TT.KW)
    torch.cuda.synchronize()
    assert bool((big[nd] == TT.SENT).all()) and bool((big[:, cols:] == TT.SENT).all())
    ends = torch.arange(nt, device="cuda") * n_wp
    assert torch.equal(X[:, ends], Xin[:, ends]) and torch.equal(X[:, ends + n_wp - 1], Xin[:, ends + n_wp - 1])
    for c in cs.off_cols:
        assert torch.equal(X[int(c)], Xin[int(c)])
    Xo = R.from_columns(X.double().cpu().numpy(), n_wp)
    ndt = np.float32 if dtype == torch.float32 else np.float64
    assert np.all(Xo[:, 1:-1] >= cs.sc.lo.astype(ndt)) and np.all(Xo[:, 1:-1] <= cs.sc.hi.astype(ndt))
    return Xo, it.cpu().numpy(), nf.double().cpu().numpy()


@pytest.mark.parametrize("name", TT.CASES)
def test_first_iterates(name):
    """fp64.  One iteration: X and info[0:3] equal the restatement's to 1e-9, info[3] and iters are equal on the
    determined trajectories.  max_iters = 1..8: the accept sequences are equal on the determined trajectories;
    after 8 iterations X and the merit are within TOL8_TREE."""
    cs = TT.case(name)
    nt = TT.N_TRAJ
    ref1 = TT.ref_run(name, 1)
    X, it, nf = _gpu_run(name, 1)
    e1 = (np.abs(X - ref1["X"]).max(), np.abs(nf[:3] - ref1["info"][:3]).max())
    print(f"{name} bounds {cs.bounds} n_wp {cs.n_wp}: 1 iteration max|dX| = {e1[0]:.2e}, max|d info| = {e1[1]:.2e}")
    det = ref1["determined"]
    assert np.array_equal(nf[3][det], ref1["info"][3][det]) and np.array_equal(it[det], ref1["iters"][det])
    assert e1[0] <= TOL1 and e1[1] <= TOL1
    ref8 = TT.ref_run(name, 8)
    nacc = [np.zeros(nt)]
    for k in range(1, 9):
        X, it, nf = _gpu_run(name, k)
        nacc.append(nf[3])
    seq = np.diff(np.array(nacc), axis=0)
    ref_seq = np.maximum(ref8["accepts"], 0)
    ref_seq = np.vstack([ref_seq, np.zeros((8 - ref_seq.shape[0], nt))])
    e8 = (np.abs(X - ref8["X"]).max(), np.abs(nf[0] - ref8["info"][0]).max())
    det = ref8["determined"]
    print(f"{name}: 8 iterations max|dX| = {e8[0]:.2e}, max|d merit| = {e8[1]:.2e}, determined {int(det.sum())}/{nt}")
    assert det.sum() >= 4
    assert np.array_equal(seq[:, det], ref_seq[:, det])
    assert np.array_equal(it[det], ref8["iters"][det])
    assert e8[0] <= TOL8_TREE and e8[1] <= TOL8_TREE


def test_single_parts_on_the_existing_kernel():
    """The inputs of TOL8_TREE and DELTA32_TREE: kin_traj_opt_batch (k_traj, unchanged) on every single-part sub-case
    against its own restatement -- 8 iterations in fp64 (D8_PARTS), one in fp32 (D32_PARTS).  The measured maxima are
    printed and held to the recorded constants."""
    d8 = d32 = 0.0
    n_sub = 0
    for name in TT.CASES:
        cs = TT.case(name)
        for p, sph in enumerate(cs.parts):
            sph = tuple(sph)
            if cs.bounds[p] <= 8 and cs.n_dof > 12:     # kin_traj_opt_batch: at most 12 q columns for chains <= 8
                continue
            n_sub += 1
            assert _plan(name, torch.float64, sph).n_parts == 1
            r8 = TT.ref_run(name, 8, spheres=sph)
            X, _, nf = _gpu_run(name, 8, spheres=sph, tree=False)
            e8 = max(np.abs(X - r8["X"]).max(), np.abs(nf[0] - r8["info"][0]).max())
            r1 = TT.ref_run(name, 1, spheres=sph)
            X32, _, _ = _gpu_run(name, 1, dtype=torch.float32, spheres=sph, tree=False)
            e32 = np.abs(X32 - r1["X"]).max()
            print(f"{name} part {p} (bound {cs.bounds[p]}): fp64 8 iterations {e8:.2e}, fp32 1 iteration {e32:.2e}")
            d8, d32 = max(d8, e8), max(d32, e32)
    print(f"D8_PARTS measured {d8:.3e} (recorded {D8_PARTS:.3e}), D32_PARTS measured {d32:.3e} (recorded {D32_PARTS:.3e})")
    assert n_sub == 6
    assert d8 <= D8_PARTS and d32 <= D32_PARTS


@pytest.mark.parametrize("name", TT.CASES)
def test_fp32(name):
    """fp32: after one iteration |X32 - X_ref| <= DELTA32_TREE; the merit does not increase over runs of 1, 2, 4, 8
    iterations and info[3] <= k."""
    ref1 = TT.ref_run(name, 1)
    last = None
    for k in (1, 2, 4, 8):
        X, it, nf = _gpu_run(name, k, dtype=torch.float32)
        if k == 1:
            e = np.abs(X - ref1["X"]).max()
            print(f"{name}: fp32 1 iteration max|X32 - X_ref| = {e:.2e}")
            assert e <= DELTA32_TREE
        if last is not None:
            assert np.all(nf[0] <= last)
        assert np.all(nf[3] <= k)
        last = nf[0]


def test_every_part_counts():
    """twoarm, a trajectory whose right-arm spheres (the second part) are inside the band at X0: the result with all
    spheres differs by > 1e-6 from the result with the left arm's spheres only, and each equals its own
    restatement to 1e-9 (a kernel that walks part 0 only would return the second for both)."""
    name = "twoarm-nobase"
    cs = TT.case(name)
    left, right = tuple(cs.parts[0]), tuple(cs.parts[1])
    assert all(TT.TWO_ARM_SPHERES[k][0].startswith("l") for k in left)
    t = int(np.flatnonzero(TT.inside_band(cs)[1])[0])
    X0 = cs.X0[t:t + 1]
    ra = TT.run_case(cs, 1, X0=X0)
    rl = TT.run_case(cs, 1, X0=X0, spheres=left)
    Xa, _, na = _gpu_run(name, 1, X0=X0)
    Xl, _, nl = _gpu_run(name, 1, X0=X0, spheres=left)
    assert np.abs(ra["X"] - rl["X"]).max() > 1e-6 and np.abs(Xa - Xl).max() > 1e-6
    assert np.abs(Xa - ra["X"]).max() <= TOL1 and np.abs(na[:3] - ra["info"][:3]).max() <= TOL1
    assert np.abs(Xl - rl["X"]).max() <= TOL1 and np.abs(nl[:3] - rl["info"][:3]).max() <= TOL1


@pytest.mark.parametrize("name", TT.CASES)
def test_info_matches_coll_batch(name):
    """After 40 iterations info[2] is the minimum over the interior waypoints of kin_coll_batch's min_dist of the
    multi-part plan on the returned X (1e-9)."""
    cs = TT.case(name)
    X, it, nf = _gpu_run(name, 40)
    Q = torch.tensor(R.to_columns(X), dtype=torch.float64, device="cuda")
    _, _, mn = _plan(name, torch.float64).run(_sdf(name), Q, dists=False, min_dist=True)
    dm = mn.cpu().numpy().reshape(-1, cs.n_wp)[:, 1:-1].min(1)
    assert np.abs(nf[2] - dm).max() <= 1e-9


@pytest.mark.parametrize("name", [TT.MIXED_BOUNDS, TT.WP64])
def test_packing_independence(name):
    """Parts of bound 16 and 4 in one plan, and n_wp = 64: trajectory t of the 9-batch is bit-equal to the same
    trajectory run alone and run at another segment position."""
    cs = TT.case(name)
    X, it, nf = _gpu_run(name, 8)
    for t in (0, 4, 8):
        Xa, ia, na = _gpu_run(name, 8, X0=cs.X0[t:t + 1])
        assert np.array_equal(Xa[0], X[t]) and ia[0] == it[t] and np.array_equal(na[:, 0], nf[:, t])
        Xb, ib, nb = _gpu_run(name, 8, X0=cs.X0[[1, 2, 3, 5, 6, t, 7]])
        assert np.array_equal(Xb[5], X[t]) and ib[5] == it[t] and np.array_equal(nb[:, 5], nf[:, t])


def _T(t):
    T = np.eye(4)
    T[:3, 3] = t
    return T


def test_single_chain_plan_through_the_new_entry():
    """A single-chain plan (Fetch, the planning scene of tests/test_gpu_trajopt.py, 32 goals, 40 iterations): the new
    entry point runs kin_traj_opt_batch's kernel -- X, iters and info are bit-equal."""
    import kinhip
    m = kinhip.parse_urdf(golden("fetch.urdf"))
    joints = [m.find_joint(n) for n in ARM]
    sscc = kinhip.SweptSphereCollisionChecker(m)
    for n in R.COLL_LINKS:
        kinhip.add_coll_links(sscc, m.find_link(n))
    sdf = kinhip.UnionSDF([kinhip.BoxSDF(_T(R.BOX_POSE), R.BOX_WIDTH)])
    plan = sscc.plan(joints, dtype=torch.float64)
    assert plan.n_parts == 1 and plan.part_chain_bounds == [plan.chain_bound]
    X0 = torch.tensor(R.to_columns(R.full_run(10)["X0"]), dtype=torch.float64, device="cuda")
    prm = dict(R.PARAMS, max_iters=40)
    Xa, Xb = X0.clone(), X0.clone()
    ia, na = kinhip.traj_opt_batch(plan, sdf, Xa, 10, **prm)
    ib, nb = kinhip.traj_opt_tree_batch(plan, sdf, Xb, 10, **prm)
    torch.cuda.synchronize()
    assert not torch.equal(Xa, X0)
    assert torch.equal(Xa, Xb) and torch.equal(ia, ib) and torch.equal(na, nb)


def _branches_urdf(lengths):
    """Serial chains of revolute joints (alternating z / y axes) hanging off one root link, one per entry."""
    out = ['<robot name="branches">', '  <link name="root"/>']
    for b, n in enumerate(lengths):
        for k in range(n):
            out.append(f'  <link name="b{b}_{k}"/>')
            parent = "root" if k == 0 else f"b{b}_{k - 1}"
            out.append(f'  <joint name="j{b}_{k}" type="revolute"><parent link="{parent}"/><child link="b{b}_{k}"/>'
                       f'<origin xyz="0.1 {0.1 * b} 0.05" rpy="0 0 0"/><axis xyz="{"0 0 1" if k % 2 == 0 else "0 1 0"}"/>'
                       '<limit lower="-2" upper="2" effort="1" velocity="1"/></joint>')
    return "\n".join(out + ["</robot>"])


@pytest.mark.parametrize("lengths,with_base,bounds,what", [
    ((1, 1, 1, 1, 1), False, [4] * 5, b"chains"), ((9, 9), True, [12, 12], b"q columns"),
    ((17, 1), False, [32, 4], b"steps"), ((8, 2, 1, 1), True, [8, 4, 4, 4], None)],
    ids=["5-chains", "21-columns", "17-steps", "4-chains-15-columns"])
def test_limits_by_tree(tmp_path, lengths, with_base, bounds, what):
    """A star of five one-joint branches: KIN_E_UNSUPPORTED ("chains"); two 9-joint chains with the base, 21 columns:
    "q columns"; a 17-step part: "steps"; four chains with 15 columns run."""
    import kinhip
    from kinhip import _lib as K
    p = tmp_path / "branches.urdf"
    p.write_text(_branches_urdf(lengths))
    m = kinhip.parse_urdf(str(p), with_base=with_base)
    joints = [m.find_joint(f"j{b}_{k}") for b, n in enumerate(lengths) for k in range(n)]
    sscc = kinhip.SweptSphereCollisionChecker(m)
    for b, n in enumerate(lengths):
        sscc.add_coll_sphere(m.find_link(f"b{b}_{n - 1}"), [0.02, 0, 0], 0.05)
    plan = sscc.plan(joints, dtype=torch.float64)
    assert plan.n_parts == len(lengths) and plan.part_chain_bounds == bounds
    sdf = kinhip.UnionSDF([kinhip.BoxSDF(_T((2.0, 2.0, 2.0)), (0.1, 0.1, 0.1))])
    nd = len(joints) + (3 if with_base else 0)
    X = torch.zeros((nd, 10), dtype=torch.float64, device="cuda")
    prm = K.TrajParams(5, 1, 0.02, 0.03, 10.0, 1e-3, 1e-6, 0.5, None)
    L = K.lib()
    rc = L.kin_traj_opt_tree_batch(plan._h, sdf._h, C.byref(prm), X.data_ptr(), 10, 2, None, None, 0, None)
    torch.cuda.synchronize()
    if what is None:
        assert rc == K.KIN_OK, L.kin_last_error()
        assert not bool(X.any())        # a straight line at rest far from the box stays
    else:
        assert rc == K.KIN_E_UNSUPPORTED and what in L.kin_last_error()


def test_limits_on_the_union_and_the_pose_variant():
    """A union attached to a scene is refused ("attached"); kin_traj_opt_batch and kin_traj_opt_pose_batch keep
    refusing a two-chain plan ("several chains")."""
    import kinhip
    from kinhip import _lib as K
    name = "twoarm-nobase"
    cs = TT.case(name)
    plan = _plan(name, torch.float64)
    L = K.lib()
    prm = K.TrajParams(cs.n_wp, 5, 0.02, 0.03, 10.0, 1e-3, 1e-6, 0.5, None)
    X = torch.tensor(R.to_columns(cs.X0), dtype=torch.float64, device="cuda")
    fr = kinhip.parse_urdf(golden("fridge.urdf"), with_base=True)
    att = kinhip.AttachedUnionSDF(fr, [fr.find_joint("door_joint")])
    args = (X.data_ptr(), X.stride(0), TT.N_TRAJ, None, None, 0, None)
    assert L.kin_traj_opt_tree_batch(plan._h, att._h, C.byref(prm), *args) == K.KIN_E_UNSUPPORTED
    assert b"attached" in L.kin_last_error()
    assert L.kin_traj_opt_batch(plan._h, _sdf(name)._h, C.byref(prm), *args) == K.KIN_E_UNSUPPORTED
    assert b"several chains" in L.kin_last_error()
    m, joints = _mech(name)
    tplan = _checker(name).traj_plan(joints, [m.find_link("l_grip")], dtype=torch.float64)
    assert tplan.n_parts == 2
    wps, rots = (C.c_int32 * 1)(5), (C.c_int32 * 1)(0)
    pp = K.TrajPoseParams(1, C.cast(wps, C.c_void_p), C.cast(rots, C.c_void_p), 10.0, 1e-6, 1e-3, 1e-3)
    tg = torch.zeros((12, TT.N_TRAJ), dtype=torch.float64, device="cuda")
    assert L.kin_traj_opt_pose_batch(tplan._h, _sdf(name)._h, C.byref(prm), C.byref(pp), tg.data_ptr(), TT.N_TRAJ,
                                     *args) == K.KIN_E_UNSUPPORTED
    assert b"several chains" in L.kin_last_error()
    torch.cuda.synchronize()
    assert torch.equal(X, torch.tensor(R.to_columns(cs.X0), dtype=torch.float64, device="cuda"))


def test_capture():
    """After the plan's first (staging) call for an n_wp, a call captured in a graph replays the eager results."""
    import kinhip
    name = "tree3"
    cs = TT.case(name)
    plan, sdf = _plan(name, torch.float64), _sdf(name)
    kw = dict(TT.KW, max_iters=20, dof_weights=cs.dof_weights)
    X0 = torch.tensor(R.to_columns(cs.X0), dtype=torch.float64, device="cuda")
    Xe = X0.clone()
    ite, nfe = kinhip.traj_opt_tree_batch(plan, sdf, Xe, cs.n_wp, **kw)   # eager; also stages the table
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
            kinhip.traj_opt_tree_batch(plan, sdf, Xg, cs.n_wp, iters=itg, info=nfg, stream=s, **kw)
        for rep in range(2):
            g.replay()
            s.synchronize()
            assert torch.equal(Xg, Xe) and torch.equal(itg, ite) and torch.equal(nfg, nfe), rep


def test_python_layer():
    """plan_trajectories on twoarm with the base, the 9 problems of the case (its X0 as the initial guess, 40
    iterations): the set done within 40 iterations equals the restatement's on the determined trajectories.
    plan_trajectory with solver="GPU" on the straight-line problem the restatement finishes soonest: ":SUCCESS".
    pose_link on the two-chain checker: ValueError before any launch."""
    import kinhip
    name = "twoarm-base"
    cs = TT.case(name)
    m, joints = _mech(name)
    sscc, sdf = _checker(name), _sdf(name)
    ref = TT.ref_run(name, 40)
    Qs, Qg = cs.X0[:, 0].T.copy(), cs.X0[:, -1].T.copy()
    X, it, nf = kinhip.plan_trajectories(sscc, joints, sdf, Qs, Qg, cs.n_wp, max_iters=40, X0=R.to_columns(cs.X0),
                                         dof_weights=cs.dof_weights, **TT.KW)
    det = ref["determined"]
    done = (ref["iters"] <= 40)[det]
    assert det.sum() >= 4 and done.any() and not done.all()
    assert np.array_equal((it.cpu().numpy() <= 40)[det], done)
    lines = np.stack([R.straight_lines(Qs[:, t], Qg[:, t:t + 1], cs.n_wp)[0] for t in range(TT.N_TRAJ)])
    full = R.run(cs.sc, lines, max_iters=200, **TT.KW)
    good = np.flatnonzero(full["determined"] & (full["iters"] <= 200) & (full["info"][3] > 1))
    assert good.size > 0
    t = int(good[np.argmin(full["iters"][good])])
    q_seq, status = kinhip.plan_trajectory(sscc, joints, sdf, Qs[:, t], Qg[:, t], cs.n_wp, solver="GPU")
    assert status == ":SUCCESS" and q_seq.shape == (cs.n_dof, cs.n_wp)
    with pytest.raises(ValueError):
        kinhip.plan_trajectories(sscc, joints, sdf, Qs, Qg, cs.n_wp, pose_link=m.find_link("l_grip"), pose_wp=2,
                                 pose_targets=np.eye(4))


def test_pr2_full_run():
    """PR2 with both arms, the base and PR2_ARM_SPHERES, 6 trajectories from PR2_MANIP_POSE, 200 iterations, fp64:
    iters equal the restatement's on the determined trajectories, and as many trajectories are done within 200
    iterations as in the restatement (5 of 6 with the committed seed; taken from the restatement)."""
    cs = TT.case("pr2")
    ref = TT.pr2_full()
    n = TT.N_PR2_FULL
    X, it, nf = _gpu_run("pr2", 200, X0=cs.X0[:n])
    det = ref["determined"]
    print(f"pr2: done {int((it <= 200).sum())}/{n} (restatement {int((ref['iters'] <= 200).sum())}), determined "
          f"{int(det.sum())}, max|dX| on determined {np.abs(X - ref['X'])[det].max():.2e}")
    assert det.sum() >= 1
    assert np.array_equal(it[det], ref["iters"][det])
    assert int((it <= 200).sum()) == int((ref["iters"] <= 200).sum())
