"""kin_traj_opt_pose_tree_batch without a GPU: the cases of tests/trajopt_pose_tree_cases.py with the CPU restatement
(tests/trajopt_pose_ref.py, unchanged, on the multi-chain and the attached scenes) alone, the staging refusals of
kin_traj_plan_create's new placement rule (they precede any upload) and the argument checks of the new entry point.

Measured on the CPU (8 iterations, the restatement forward against itself with every sum reversed):
  case        part  n_wp  n_dof  determined  max |X - X_rev|  max |merit - merit_rev|
  twoarm-l3     0    10      9     9/9         2.3e-14          1.4e-13
  twoarm-l6     0    10      9     9/9         7.4e-14          2.6e-14
  twoarm-r3     1    10      9     9/9         2.1e-13          2.8e-13
  twoarm-r6     1    10      9     9/9         1.2e-14          1.0e-13
  base-c1       0     5     12     8/9         9.7e-15          8.3e-15
  base-c3       0     5     12     9/9         4.8e-13          6.9e-12
  pr2           1    10     17     9/9         2.1e-14          2.0e-13
  tree3         3    10     17     8/9         3.7e-13          7.2e-13
  s-fetch       0    10      8     9/9         1.2e-13          6.6e-13
  s-pr2         1    10     17     9/9         2.9e-14          4.7e-14
  s-uniform     0    10      8     9/9         2.4e-13          1.5e-12
  pr2-wp64      1    64     17     2/2         2.9e-15          2.8e-14
SPREAD8_PT = 7.0e-12 is the largest (6.92e-12, base-c3's merit, rounded up).

The PR2 family, the left tool frame at waypoint 5, 6 trajectories, 200 iterations (test_pr2_full_run_restatement):
  union                       rows   good   done
  static                        3    6/6    5/6
  static                        6    3/6    3/6
  door closing 2.0 -> 1.2       3    6/6    4/6
  door closing 2.0 -> 1.2       6    6/6    3/6
"""
import ctypes as C

import numpy as np
import pytest

import kinhip
import trajopt_pose_ref as P
import trajopt_pose_tree_cases as PT
from conftest import ARM, golden
from kinhip import _lib as K
from test_trajopt_pose import _pose, _prm

SPREAD8_PT = 7.0e-12       # the largest spread of the table above


@pytest.mark.parametrize("name", ["twoarm-r6", "pr2", "tree3", "s-pr2"])
def test_jacobian_is_the_derivative_of_the_residual(name):
    """Forward differences, step 1e-6, bound 1e-5 (as tests/test_trajopt_pose.py), on scenes with several chains and
    with the base: the position rows at waypoint c of X0 with the case's targets, the rotation rows with the targets
    at the link's own pose (|r_rot| = 0: J is the derivative of -log(R* R^T) to first order in it)."""
    cs = PT.case(name)
    sc = cs.sc
    Q = np.ascontiguousarray(cs.X0[:4, cs.c].T)
    here = sc.om.fk_batch(Q, sc.ids, [cs.link])[0]
    for tg, k in ((cs.targets[:, :4], 3), (here, 6 if cs.with_rot else 3)):
        r0, J = P.residual(sc, cs.link, Q, tg, cs.with_rot)
        assert np.abs(J).max() > 1e-2
        for d in range(sc.n_dof):
            Qd = Q.copy()
            Qd[d] += 1e-6
            fd = (P.residual(sc, cs.link, Qd, tg, cs.with_rot)[0] - r0) / 1e-6
            assert np.abs(fd[:, :k] - J[:, :k, d]).max() < 1e-5, (name, d, k)


@pytest.mark.parametrize("name", PT.CASES)
def test_case_conditions_and_spread(name):
    """The restatement alone: at least 5 of 9 trajectories (all of the 2 of pr2-wp64) determined after 8 iterations;
    forward against reversed summation within SPREAD8_PT; the merit never increases; the restated carrying part is a
    part of the plan, and part 1 for r_grip and for the PR2's left tool frame."""
    cs = PT.case(name)
    a, b = PT.ref_run(name, 8), PT.ref_run(name, 8, rev=True)
    det = a["determined"]
    sx, sf = np.abs(a["X"] - b["X"]).max(), np.abs(a["info"][0] - b["info"][0]).max()
    print(f"{name}: part {cs.part}, determined {int(det.sum())}/{cs.n_traj}, spread X {sx:.2e} merit {sf:.2e}")
    assert det.sum() >= min(5, cs.n_traj)
    assert max(sx, sf) <= SPREAD8_PT
    assert np.all(np.diff(a["merits"], axis=0) <= 0.0)
    assert 0 <= cs.part < len(cs.base.parts)
    if name in ("twoarm-r3", "twoarm-r6", "pr2", "s-pr2"):
        assert cs.part == 1
    assert np.abs(a["X"] - cs.X0).max() > 1e-3      # (the constraint and the boxes move it)


@pytest.mark.parametrize("scene", [False, True])
@pytest.mark.parametrize("rows", [3, 6])
def test_pr2_full_run_restatement(scene, rows):
    """The PR2 family within 200 iterations, static and with the door closing: the merit never increases and every
    trajectory that is done is good; the counts are printed (the table above; the GPU test pins the good sets)."""
    out = PT.pr2_full(scene, rows)["out"]
    ok = P.good(out, PT.KW["margin"], PT.KW["feas"])
    done = out["iters"] <= 200
    print(f"pr2 {'door' if scene else 'static'} rows {rows}: good {int(ok.sum())}/{ok.size}, done {int(done.sum())}/{ok.size}")
    assert np.all(np.diff(out["merits"], axis=0) <= 0.0)
    assert np.all(ok[done])


# ------------------------------------------------------------------------------------------------ the ABI on the host
@pytest.mark.parametrize("kw,code,word", [
    (dict(n_con=2), K.KIN_E_UNSUPPORTED, b"n_con"),
    (dict(wp=0), K.KIN_E_INVALID, b"interior"),
    (dict(wp=9), K.KIN_E_INVALID, b"interior"),
    (dict(with_rot=2), K.KIN_E_INVALID, b"with_rot"),
    (dict(weight=0.0), K.KIN_E_INVALID, b"pose weight"),
    (dict(tol_pos=0.0), K.KIN_E_INVALID, b"tol_pos"),
    (dict(tol_rot=float("nan")), K.KIN_E_INVALID, b"tol_rot"),
    (dict(damp=-1e-9), K.KIN_E_INVALID, b"damp"),
])
def test_parameter_checks_before_device(kw, code, word):
    """The parameter and pose-parameter limits are refused on the host under the new entry point's name before the plan
    is looked at (null plan, null arrays); then lds < 0 and the null plan."""
    L = K.lib()
    tg = np.zeros((12, 4))
    call = lambda prm, pp, ldt=4, n=4, lds=0: L.kin_traj_opt_pose_tree_batch(
        None, None, C.byref(prm) if prm else None, C.byref(pp) if pp else None, tg.ctypes.data, ldt, None, lds, None, 0,
        n, None, None, 0, None)
    assert call(_prm(), _pose(**kw)) == code
    assert word in L.kin_last_error() and b"kin_traj_opt_pose_tree_batch" in L.kin_last_error()
    assert call(_prm(), _pose()) == K.KIN_E_INVALID and b"null plan" in L.kin_last_error()
    assert call(_prm(), _pose(), lds=-1) == K.KIN_E_INVALID and b"lds" in L.kin_last_error()
    assert call(_prm(), _pose(), ldt=3) == K.KIN_E_INVALID and b"ldt" in L.kin_last_error()
    assert call(_prm(), None) == K.KIN_E_INVALID and b"null pose parameters" in L.kin_last_error()
    assert call(None, _pose()) == K.KIN_E_INVALID
    assert call(_prm(n_wp=65), _pose()) == K.KIN_E_UNSUPPORTED and b"n_wp" in L.kin_last_error()
    assert call(_prm(ftol=0.0), _pose()) == K.KIN_E_INVALID and b"ftol" in L.kin_last_error()
    v = C.c_int32()
    assert L.kin_plan_pose_link_part(None, 0, C.byref(v)) == K.KIN_E_INVALID


def _fetch_two_parts(extra):
    """Fetch with spheres on the arm and on the head (two parts) and `extra` more batch joints."""
    m = kinhip.parse_urdf(golden("fetch.urdf"))
    joints = [m.find_joint(n) for n in list(ARM) + ["head_pan_joint", "head_tilt_joint"] + list(extra)]
    sscc = kinhip.SweptSphereCollisionChecker(m)
    sscc.add_coll_sphere(m.find_link("wrist_roll_link"), [0, 0, 0], 0.05)
    sscc.add_coll_sphere(m.find_link("head_tilt_link"), [0, 0, 0], 0.05)
    return m, joints, sscc


def _two_branches(n_a, n_b):
    """Two serial chains of revolute joints (alternating z / y axes) off one root link: a0..a<n_a-1>, b0..b<n_b-1>."""
    out = ['<robot name="two">', '  <link name="root"/>']
    for b, n in (("a", n_a), ("b", n_b)):
        for k in range(n):
            parent = "root" if k == 0 else f"{b}{k - 1}"
            out.append(f'  <link name="{b}{k}"/>\n  <joint name="j{b}{k}" type="revolute"><parent link="{parent}"/>'
                       f'<child link="{b}{k}"/><origin xyz="0.1 {0.1 if b == "a" else -0.1} 0.05"/>'
                       f'<axis xyz="{"0 0 1" if k % 2 == 0 else "0 1 0"}"/>'
                       '<limit lower="-2" upper="2" effort="1" velocity="1"/></joint>')
    return "\n".join(out + ["</robot>"])


def test_staging_refusals(tmp_path):
    """Refused while staging, before any upload: a pose link comparable with no part's spine (a wheel: neither the
    arm's chain nor the head's); a carrying part of more than 8 steps after the extension, on the first part (the arm's 8
    joints and a gripper finger) and on a later one (two branches: spheres 8 joints down branch a -- part 0 -- and 7
    down branch b, the pose link 9 down branch b: it rides on part 1, whose chain then has 9 steps)."""
    p = tmp_path / "two.urdf"
    p.write_text(_two_branches(8, 9))
    m = kinhip.parse_urdf(str(p))
    joints = [m.find_joint(f"ja{k}") for k in range(8)] + [m.find_joint(f"jb{k}") for k in range(9)]
    sscc = kinhip.SweptSphereCollisionChecker(m)
    sscc.add_coll_sphere(m.find_link("a7"), [0.02, 0, 0], 0.05)
    sscc.add_coll_sphere(m.find_link("b6"), [0.02, 0, 0], 0.05)
    with pytest.raises(K.KinError, match="more than 8 steps") as e:
        sscc.traj_plan(joints, [m.find_link("b8")])
    assert e.value.code == K.KIN_E_UNSUPPORTED
    m, joints, sscc = _fetch_two_parts(["l_wheel_joint"])
    with pytest.raises(K.KinError, match="another branch") as e:
        sscc.traj_plan(joints, [m.find_link("l_wheel_link")])
    assert e.value.code == K.KIN_E_UNSUPPORTED
    m, joints, sscc = _fetch_two_parts(["r_gripper_finger_joint"])
    with pytest.raises(K.KinError, match="more than 8 steps") as e:
        sscc.traj_plan(joints, [m.find_link("r_gripper_finger_link")])
    assert e.value.code == K.KIN_E_UNSUPPORTED
