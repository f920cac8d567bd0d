"""kin_traj_opt_batch (k_traj) on the seeded random chains of tests/trajopt_cases.py against the CPU restatement
(tests/trajopt_ref.py): all four chain bounds (asserted through kin_plan_chain_bound) x L = 8 / 16 / 32 / 64 in
both precisions, the 20-column register layout, the halved workgroup (WIDE), a union of 70 boxes read from global
memory (MANY_BOXES), rotated boxes, root spheres with the base, held joints, prismatic joints in mid-chain, oblique
and unnormalised axes, an off-path column, dof_weights, ldx > n_traj * n_wp and the joint-limit clamp.  All plans
are generic (k_traj is not specialised); one plan per (case, dtype).

Bounds.  One iteration, fp64: the project's 1e-9.  Eight iterations, fp64: TOL8_RC = 10 x SPREAD8_RC = 1.6e-13,
SPREAD8_RC = 1.6e-14 being the restatement's own forward / reversed-summation spread measured on the CPU in
tests/test_trajopt_random_chains.py (never from the kernel).  fp32, one iteration: DELTA32 = 4 x the largest
|X32 - X_ref| measured (the margin of tests/test_gpu_ik_random_chains.py's DELTA), capped at 3e-4.

Measured on an MI355X, the kernel against the restatement, maxima per chain bound:
  bound   fp64 1 it. (X, info)   fp64 8 it. |dX|   fp64 8 it. |d merit|   fp32 1 it. |X32 - X_ref|
    4          1.7e-14              5.2e-14            2.6e-14                 3.2e-6
    8          5.7e-14              2.4e-14            5.7e-14                 6.8e-7
   12          5.2e-15              9.3e-15            1.0e-15                 2.7e-6
   16          5.8e-14              1.5e-13            5.0e-14                 4.6e-6
The largest fp64 figure after 8 iterations, 1.52e-13 (chain7-nobase: 16 joints, n_wp = 20), is within TOL8_RC by
5 %: the spread does not contain the rounding of a 16-joint FK (the restatement's FK is the oracle's in both of its
summation orders), which the kernel's error after one iteration (2.8e-14 in that case) does.
DELTA32 = 4 x 4.56e-6 = 1.8e-5.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import trajopt_cases as TC
import trajopt_ref as R
from test_trajopt_random_chains import SPREAD8_RC, clamped

pytestmark = pytest.mark.gpu

TOL1 = 1e-9                    # the project's fp64 tolerance
TOL8_RC = 10 * SPREAD8_RC
DELTA32 = 1.8e-5               # fp32, one iteration, against the fp64 restatement (module docstring; cap 3e-4)
_DIR = {}


@pytest.fixture(scope="module", autouse=True)
def _urdf_dir(tmp_path_factory):
    _DIR["d"] = str(tmp_path_factory.mktemp("trajchains"))


@functools.lru_cache(maxsize=None)
def _setup(key):
    """The case on the library's side: mechanism (held joints set), batch joints, checker, union."""
    import kinhip
    cs = TC.case(key)
    p = os.path.join(_DIR["d"], f"chain{key[0]}.urdf")
    if not os.path.exists(p):
        with open(p, "w") as f:
            f.write(cs.ch.text)
    m = kinhip.parse_urdf(p, with_base=cs.with_base)
    for j, a in zip(cs.ch.held, cs.ch.held_ang):
        m.set_joint_angle(m.joints[j - 1], float(a))
    joints = [m.joints[j - 1] for j in cs.ch.q_ids]
    sscc = kinhip.SweptSphereCollisionChecker(m)
    for l, c, r in cs.spheres:
        sscc.add_coll_sphere(m.links[l - 1], c, r)
    sdf = kinhip.UnionSDF([kinhip.BoxSDF(T, w) for T, w in zip(cs.sc.box_poses, cs.sc.box_widths)])
    return m, joints, sscc, sdf


@functools.lru_cache(maxsize=None)
def _plan(key, dtype):
    m, joints, sscc, sdf = _setup(key)
    plan = sscc.plan(joints, dtype=dtype)
    assert plan.chain_bound == TC.case(key).bound, (key, plan.chain_bound)
    return plan


def _gpu_run(key, max_iters, dtype=torch.float64, weights=True, X0=None):
    """-> X [nt, n_wp, nd], iters, info (numpy, fp64).  X is a view into a wider tensor (ldx = n_traj * n_wp + PAD,
    one more row) filled with SENT; every run checks what the kernel must leave alone: the padding, the end
    columns, the off-path columns, and that the interior stays within the limits."""
    import kinhip
    cs = TC.case(key)
    X0 = cs.X0 if X0 is None else X0
    nt, n_wp, nd = X0.shape
    cols = nt * n_wp
    big = torch.full((nd + 1, cols + TC.PAD), TC.SENT, dtype=dtype, device="cuda")
    X = big[:nd, :cols]
    Xin = torch.tensor(R.to_columns(X0), dtype=dtype, device="cuda")
    X.copy_(Xin)
    w = cs.dof_weights if weights else None
    it, nf = kinhip.traj_opt_batch(_plan(key, dtype), _setup(key)[3], X, n_wp, max_iters=max_iters, dof_weights=w,
                                   **TC.KW)
    torch.cuda.synchronize()
    assert bool((big[nd] == TC.SENT).all()) and bool((big[:, cols:] == TC.SENT).all())
    ends = torch.arange(nt, device="cuda") * n_wp
    assert torch.equal(X[:, ends], Xin[:, ends]) and torch.equal(X[:, ends + n_wp - 1], Xin[:, ends + n_wp - 1])
    for c in cs.off_cols:
        assert torch.equal(X[int(c)], Xin[int(c)])
    Xo = R.from_columns(X.double().cpu().numpy(), n_wp)
    ndt = np.float32 if dtype == torch.float32 else np.float64     # (the kernel clamps to the limits in its dtype)
    assert np.all(Xo[:, 1:-1] >= cs.sc.lo.astype(ndt)) and np.all(Xo[:, 1:-1] <= cs.sc.hi.astype(ndt))
    return Xo, it.cpu().numpy(), nf.double().cpu().numpy()


@pytest.mark.parametrize("key", TC.CASES, ids=TC.cid)
def test_first_iterates(key):
    """fp64.  One iteration: X and info[0:3] equal the restatement's to 1e-9, info[3] and iters are equal on the
    determined trajectories.  max_iters = 1..8: the accept sequences are equal on the determined trajectories;
    after 8 iterations X and the merit are within TOL8_RC."""
    cs = TC.case(key)
    if key == TC.WIDE:
        assert cs.n_dof >= 17 and cs.n_wp == 64     # fp64: the workgroup is halved to fit LDS
    nt = TC.N_TRAJ
    ref1 = TC.ref_run(key, 1)
    X, it, nf = _gpu_run(key, 1)
    e1 = (np.abs(X - ref1["X"]).max(), np.abs(nf[:3] - ref1["info"][:3]).max())
    print(f"{TC.cid(key)} bound {cs.bound} n_wp {cs.n_wp}: 1 iteration max|dX| = {e1[0]:.2e}, max|d info| = {e1[1]:.2e}")
    det = ref1["determined"]
    assert np.array_equal(nf[3][det], ref1["info"][3][det]) and np.array_equal(it[det], ref1["iters"][det])
    assert e1[0] <= TOL1 and e1[1] <= TOL1
    ref8 = TC.ref_run(key, 8)
    nacc = [np.zeros(nt)]
    for k in range(1, 9):
        X, it, nf = _gpu_run(key, k)
        nacc.append(nf[3])
    seq = np.diff(np.array(nacc), axis=0)
    ref_seq = np.maximum(ref8["accepts"], 0)
    ref_seq = np.vstack([ref_seq, np.zeros((8 - ref_seq.shape[0], nt))])
    e8 = (np.abs(X - ref8["X"]).max(), np.abs(nf[0] - ref8["info"][0]).max())
    det = ref8["determined"]
    print(f"{TC.cid(key)}: 8 iterations max|dX| = {e8[0]:.2e}, max|d merit| = {e8[1]:.2e}, determined "
          f"{int(det.sum())}/{nt}, clamped coordinates {clamped(cs, X)}")
    assert det.sum() >= 4
    assert np.array_equal(seq[:, det], ref_seq[:, det])
    assert np.array_equal(it[det], ref8["iters"][det])
    assert e8[0] <= TOL8_RC and e8[1] <= TOL8_RC


@pytest.mark.parametrize("key", TC.CASES, ids=TC.cid)
def test_info_matches_coll_batch(key):
    """After 40 iterations info[2] is the minimum over the interior waypoints of kin_coll_batch's min_dist on the
    returned X (1e-9), and info[1] the restatement's smoothness term of the returned X with the case's
    dof_weights (1e-9 relative)."""
    cs = TC.case(key)
    X, it, nf = _gpu_run(key, 40)
    Q = torch.tensor(R.to_columns(X), dtype=torch.float64, device="cuda")
    _, _, mn = _plan(key, torch.float64).run(_setup(key)[3], Q, dists=False, min_dist=True)
    dm = mn.cpu().numpy().reshape(-1, cs.n_wp)[:, 1:-1].min(1)
    assert np.abs(nf[2] - dm).max() <= 1e-9
    W = np.ones(cs.n_dof) if cs.dof_weights is None else cs.dof_weights ** 2
    a = (X[:, :-2] - 2.0 * X[:, 1:-1]) + X[:, 2:]
    sm = (W[None, None, :] * a * a).sum((1, 2))
    assert np.all(np.abs(nf[1] - sm) <= 1e-9 * np.abs(sm))


@pytest.mark.parametrize("key", [(3, True), (7, False)], ids=TC.cid)
def test_dof_weights_change_the_step(key):
    """A bound-8 and a bound-16 case, with dof_weights = None and with the case's weights: the two results differ
    after one iteration, and each equals its own restatement to 1e-9 (weights ignored on both sides would pass
    the parity tests)."""
    assert TC.case(key).bound in (8, 16) and TC.case(key).dof_weights is not None
    Xw, _, nw = _gpu_run(key, 1)
    Xn, _, nn = _gpu_run(key, 1, weights=False)
    rw, rn = TC.ref_run(key, 1), TC.ref_run(key, 1, weights=False)
    assert np.abs(rw["X"] - rn["X"]).max() > 1e-6 and np.abs(Xw - Xn).max() > 1e-6
    assert np.abs(Xw - rw["X"]).max() <= TOL1 and np.abs(nw[:3] - rw["info"][:3]).max() <= TOL1
    assert np.abs(Xn - rn["X"]).max() <= TOL1 and np.abs(nn[:3] - rn["info"][:3]).max() <= TOL1


@pytest.mark.parametrize("key", [(1, True), (6, False), TC.WIDE], ids=TC.cid)
def test_packing_independence(key):
    """Bound 4, bound 16 and the halved workgroup: trajectory t of the 9-batch is bit-equal to the same trajectory
    run alone and run at another segment position."""
    cs = TC.case(key)
    X, it, nf = _gpu_run(key, 8)
    for t in (0, 4, 8):
        Xa, ia, na = _gpu_run(key, 8, X0=cs.X0[t:t + 1])
        assert np.array_equal(Xa[0], X[t]) and ia[0] == it[t] and np.array_equal(na[:, 0], nf[:, t])
        Xb, ib, nb = _gpu_run(key, 8, X0=cs.X0[[1, 2, 3, 5, 6, t, 7]])
        assert np.array_equal(Xb[5], X[t]) and ib[5] == it[t] and np.array_equal(nb[:, 5], nf[:, t])


@pytest.mark.parametrize("key", TC.CASES, ids=TC.cid)
def test_fp32(key):
    """fp32: after one iteration |X32 - X_ref| <= DELTA32 (the fp64 restatement from the same X0); the merit does
    not increase over runs of 1, 2, 4, 8 iterations and info[3] <= k."""
    cs = TC.case(key)
    ref1 = TC.ref_run(key, 1)
    last = None
    for k in (1, 2, 4, 8):
        X, it, nf = _gpu_run(key, k, dtype=torch.float32)
        if k == 1:
            e = np.abs(X - ref1["X"]).max()
            print(f"{TC.cid(key)} bound {cs.bound}: fp32 1 iteration max|X32 - X_ref| = {e:.2e}")
            assert e <= DELTA32
        if last is not None:
            assert np.all(nf[0] <= last)
        assert np.all(nf[3] <= k)
        last = nf[0]


def _serial_urdf(n_path, n_off):
    """A serial chain of n_path revolute joints (alternating z / y axes) below link l0, and n_off one-joint side
    branches on l0."""
    out = ['<robot name="serial">'] + [f'  <link name="l{k}"/>' for k in range(n_path + 1)]
    out += [f'  <link name="s{k}"/>' for k in range(n_off)]
    for k in range(n_path):
        out.append(f'  <joint name="j{k}" type="revolute"><parent link="l{k}"/><child link="l{k + 1}"/>'
                   f'<origin xyz="0.1 0 0.05" rpy="0 0 0"/><axis xyz="{"0 0 1" if k % 2 == 0 else "0 1 0"}"/>'
                   '<limit lower="-2" upper="2" effort="1" velocity="1"/></joint>')
    for k in range(n_off):
        out.append(f'  <joint name="o{k}" type="revolute"><parent link="l0"/><child link="s{k}"/>'
                   '<origin xyz="0 0.1 0" rpy="0 0 0"/><axis xyz="1 0 0"/>'
                   '<limit lower="-1" upper="1" effort="1" velocity="1"/></joint>')
    return "\n".join(out + ["</robot>"])


@pytest.mark.parametrize("n_path,n_off,with_base,bound,what", [
    (17, 0, False, 32, b"steps"), (8, 2, True, 8, b"q columns"), (12, 6, True, 12, b"q columns"), (8, 1, True, 8, None)],
    ids=["17-steps", "8-steps-13-columns", "12-steps-21-columns", "8-steps-12-columns"])
def test_limits_by_chain(tmp_path, n_path, n_off, with_base, bound, what):
    """A 17-step chain: KIN_E_UNSUPPORTED ("steps"); 8 steps with 13 columns (8 on the path + base + 2 off it) and
    12 steps with 21 columns: KIN_E_UNSUPPORTED ("q columns"); the 8-step chain with 12 columns runs."""
    import kinhip
    from kinhip import _lib as K
    p = tmp_path / "serial.urdf"
    p.write_text(_serial_urdf(n_path, n_off))
    m = kinhip.parse_urdf(str(p), with_base=with_base)
    joints = [m.find_joint(f"j{k}") for k in range(n_path)] + [m.find_joint(f"o{k}") for k in range(n_off)]
    sscc = kinhip.SweptSphereCollisionChecker(m)
    sscc.add_coll_sphere(m.find_link(f"l{n_path}"), [0.02, 0, 0], 0.05)
    plan = sscc.plan(joints, dtype=torch.float64)
    assert plan.chain_bound == bound
    T = np.eye(4)
    T[:3, 3] = (2.0, 2.0, 2.0)
    sdf = kinhip.UnionSDF([kinhip.BoxSDF(T, (0.1, 0.1, 0.1))])
    nd = len(joints) + (3 if with_base else 0)
    assert nd == n_path + n_off + (3 if with_base else 0)
    X = torch.zeros((nd, 10), dtype=torch.float64, device="cuda")
    prm = K.TrajParams(5, 1, 0.02, 0.03, 10.0, 1e-3, 1e-6, 0.5, None)
    L = K.lib()
    rc = L.kin_traj_opt_batch(plan._h, sdf._h, C.byref(prm), X.data_ptr(), 10, 2, None, None, 0, None)
    torch.cuda.synchronize()
    if what is None:
        assert rc == K.KIN_OK, L.kin_last_error()
        assert not bool(X.any())        # a straight line at rest far from the box stays
    else:
        assert rc == K.KIN_E_UNSUPPORTED and what in L.kin_last_error()
