"""kin_traj_opt_scene_batch without a GPU: the argument checks that precede any device work, and the cases of
tests/trajopt_scene_cases.py with the CPU restatement (tests/trajopt_scene_ref.py: tests/trajopt_ref.py's merit and
run on boxes that ride on a scene mechanism) alone: the guard of the seeds.  Everything tests/test_gpu_traj_scene.py
relies on is shown here by the restatement.

Measured on the CPU (8 iterations, the restatement forward against itself with every sum reversed; gap = the smallest
difference between the two smallest box distances of an in-band sphere at X0):
  case            n_wp  n_dof  part bounds  boxes  determined  max |X - X_rev|  max |merit - merit_rev|  gap
  fetch             10      8  8                7    7/9        4.4e-16          7.1e-15                  5.8e-6
  fetch-one          5      8  8                7    1/1        5.6e-17          1.4e-17                  1.6e-1
  pr2               10     17  8, 8             7    9/9        1.3e-15          3.1e-16                  6.4e-5
  tree0             33     16  16, 4            5    8/9        1.1e-14          1.4e-14                  2.2e-1
  wide              64     19  16              70    9/9        3.6e-13          4.9e-12                  2.2e-5
  fetch-uniform     10      8  8                7    8/9        3.4e-15          2.7e-16                  7.5e-6
SPREAD8_SCENE = 5.0e-12 is the largest (4.94e-12, wide's merit, rounded up).  The restatement's distances equal the
oracle's coll_batch against a per-sample OracleUnionSDF to 4.4e-16; its half-gradient matches central differences to
3.1e-9.  The PR2 full run at the closing door (6 trajectories, 200 iterations): 3 of 6 done, 5 determined."""
import ctypes as C
import re

import numpy as np
import pytest

import oracle as O
import trajopt_ref as R
import trajopt_scene_cases as SC
from kinhip import _lib as K
from test_trajopt import _prm

SPREAD8_SCENE = SC.SPREAD8_SCENE
RUN_CASES = [n for n in SC.CASES if n != "fetch-padded"]      # (fetch-padded's restatement is fetch's)


def _call(L, prm, lds=0, n_traj=1):
    return L.kin_traj_opt_scene_batch(None, None, prm, None, lds, None, 0, n_traj, None, None, 0, None)


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
    """The table of tests/test_trajopt.py::test_parameter_checks_before_device through kin_traj_opt_scene_batch: every
    parameter limit is refused on the host, under the new entry point's name, before the plan is looked at; then a
    negative lds; then the null plan."""
    L = K.lib()
    assert _call(L, C.byref(_prm(**kw))) == code
    assert word in L.kin_last_error() and b"kin_traj_opt_scene_batch" in L.kin_last_error()
    good = _prm()
    assert _call(L, C.byref(good), lds=-1) == K.KIN_E_INVALID
    assert b"lds" in L.kin_last_error()
    assert _call(L, C.byref(good)) == K.KIN_E_INVALID
    assert b"null plan" in L.kin_last_error()
    assert _call(L, None) == K.KIN_E_INVALID


def test_case_generator_covers_the_paths():
    """The shapes the cases are there for: L = 8, 16, 64; a single chain of bound 8 and one of bound 16 with 19
    columns; two parts of bound 8 (17 columns) and parts of bound 16 and 4; two box groups everywhere, one of them
    moving; 70 boxes (> 64: the union is read from global memory) behind a prismatic joint; an oblique unnormalised
    revolute axis; a distinct scene value per (trajectory, waypoint); one scene state for fetch-uniform."""
    want = {"fetch": ([8], 8, 10), "fetch-one": ([8], 8, 5), "pr2": ([8, 8], 17, 10), "tree0": ([16, 4], 16, 33),
            "wide": ([16], 19, 64)}
    for name, (bounds, nd, n_wp) in want.items():
        cs = SC.case(name)
        assert cs.bounds == bounds and cs.n_dof == nd and cs.n_wp == n_wp, (name, cs.bounds, cs.n_dof)
        assert cs.X0.shape == (1 if name == "fetch-one" else SC.N_TRAJ, n_wp, nd)
        assert np.all(cs.X0 >= cs.sc.lo) and np.all(cs.X0 <= cs.sc.hi)
        assert sorted(set(cs.sc.box_group)) == [0, 1] and sorted(cs.sc.group_moves) == [False, True]
        assert cs.SQ.shape == (cs.sc.n_scene_cols, cs.n_traj * n_wp)
        assert np.unique(cs.SQ[0]).size == cs.n_traj * n_wp
    fr = SC.case("pr2")
    assert fr.sc.n_scene_cols == 4 and len(fr.sc.boxes) == 7
    bases = fr.SQ[1:].reshape(3, fr.n_traj, fr.n_wp)
    assert np.all(bases == bases[:, :, :1]) and np.unique(bases[0, :, 0]).size == fr.n_traj
    t0 = SC.case("tree0")
    st = t0.sc.scene_tree
    ax = np.array(re.search(r'<axis xyz="([^"]+)"', open(t0.scene_path).read()).group(1).split(), float)   # as written
    assert st.joint_type[st.joint_id("move") - 1] == O.REVOLUTE and abs(np.linalg.norm(ax) - 1) > 0.2 and np.abs(ax).min() > 1e-3
    assert [t0.sc.box_group.count(g) for g in (0, 1)] == [3, 2] and t0.sc.group_moves == [False, True]
    wd = SC.case("wide")
    st = wd.sc.scene_tree
    assert st.joint_type[st.joint_id("move") - 1] == O.PRISMATIC and len(wd.sc.boxes) == 70
    assert [wd.sc.box_group.count(g) for g in (0, 1)] == [35, 35]
    un = SC.case("fetch-uniform")
    assert un.SQ.shape == (4,) and np.array_equal(un.X0, SC.case("fetch").X0)
    assert np.array_equal(SC.case("fetch-padded").SQ, SC.case("fetch").SQ)


@pytest.mark.parametrize("name", ["fetch", "pr2", "tree0", "wide", "fetch-uniform"])
def test_distances_match_the_oracle(name):
    """The restatement's sphere distances at X0 equal O.coll_batch against an OracleUnionSDF built per sample from that
    sample's world box poses, to 1e-12 (wide: every 7th sample)."""
    cs = SC.case(name)
    Q = R.to_columns(cs.X0)
    SQ = cs.sc.samples_of(Q)
    d, _ = cs.sc.distances(Q)
    cols = range(0, Q.shape[1], 7 if name == "wide" else 1)
    WB = cs.sc.world_boxes(SQ)
    err = 0.0
    for n in cols:
        sdf = O.OracleUnionSDF(WB[n], np.array(cs.sc.box_widths))
        dn, _ = O.coll_batch(cs.sc.om, sdf, np.ascontiguousarray(Q[:, n:n + 1]), cs.sc.ids, cs.sc.sph, cs.sc.rad,
                             with_grad=False)
        err = max(err, np.abs(dn[:, 0] - d[:, n]).max())
    print(f"{name}: max |d - oracle| = {err:.2e} over {len(cols)} samples")
    assert err <= 1e-12


def test_half_gradient_matches_central_differences():
    """On pr2 at the fridge (two parts, the door swinging, 4 trajectories): the restatement's half-gradient g against
    central differences of its merit, (f(x + h e) - f(x - h e)) / 2h = 2 g, h = 1e-6, to 1e-5 on >= 99 % of the
    coordinates (the merit has kinks at the band's edge and on the boxes' mid-planes).  The scene is data: the
    differences move the robot only."""
    cs = SC.case("pr2")
    X0 = cs.X0[:4]
    W = cs.dof_weights ** 2
    kw = (SC.KW["margin"], SC.KW["band"], SC.KW["weight"], W)
    _, _, _, g = R.merit(cs.sc, X0, *kw)
    assert np.abs(g).max() > 1e-2
    h, err = 1e-6, []
    rng = np.random.default_rng(3)
    for w in rng.choice(np.arange(1, cs.n_wp - 1), 4, replace=False):
        for d in range(cs.n_dof):
            Xp, Xm = X0.copy(), X0.copy()
            Xp[:, w, d] += h
            Xm[:, w, d] -= h
            err.append(np.abs((R.merit(cs.sc, Xp, *kw)[0] - R.merit(cs.sc, Xm, *kw)[0]) / (4 * h) - g[:, w - 1, d]))
    err = np.array(err)
    print(f"half-gradient vs central differences: max {err.max():.2e}, within 1e-5: {(err < 1e-5).mean():.4f}")
    assert (err < 1e-5).mean() >= 0.99


@pytest.mark.parametrize("name", RUN_CASES)
def test_case_conditions(name):
    """Conditions on the inputs, met by the restatement alone: at least 5 of 9 trajectories determined after 8
    iterations (fetch-one: its one); on a determined trajectory a sphere inside the band at X0 has a box of the
    moving group as its nearest; in pr2 and tree0 every part has a sphere inside the band; the two smallest box
    distances of any in-band sphere differ by more than 1e-9 (no argmin tie); the merit does not increase."""
    cs = SC.case(name)
    ref8 = SC.ref_run(name, 8)
    det = ref8["determined"]
    c = SC.conditions(cs, det)
    print(f"{name}: determined {int(det.sum())}/{cs.n_traj}, {c}")
    assert det.sum() >= (1 if cs.n_traj == 1 else 5)
    assert c["moving"] and c["gap"] > 1e-9
    if name in SC.MULTI_PART:
        assert len(c["parts"]) == 2 and all(c["parts"])
    m = ref8["merits"]
    assert np.all(m[1:] <= m[:-1])


@pytest.mark.parametrize("name", RUN_CASES)
def test_spread(name):
    """The restatement forward against itself with every sum reversed, 8 iterations: within SPREAD8_SCENE."""
    a, b = SC.ref_run(name, 8), SC.ref_run(name, 8, rev=True)
    sx, sf = np.abs(a["X"] - b["X"]).max(), np.abs(a["info"][0] - b["info"][0]).max()
    print(f"{name}: spread X {sx:.2e} merit {sf:.2e}")
    assert max(sx, sf) <= SPREAD8_SCENE


def test_the_scene_counts_per_waypoint():
    """fetch after 8 iterations differs by more than 1e-6 from the restatement on both frozen snapshots of trajectory
    0's scene, the door at its first and at its last angle: the per-waypoint state is not a detail."""
    cs = SC.case("fetch")
    ref = SC.ref_run("fetch", 8)["X"][0]
    for w in (0, cs.n_wp - 1):
        fz = SC.run_case(cs, 8, X0=cs.X0[:1], sc=cs.sc.frozen(cs.SQ[:, w]))["X"][0]
        assert np.abs(fz - ref).max() > 1e-6


def test_pr2_full_run_restatement():
    """PR2 at the fridge, 6 trajectories, 200 iterations, the door closing from 2.0 to 1.2: the merit never increases
    and some trajectory is done (the counts are what the GPU test pins)."""
    sc, SQ, out = SC.pr2_full()
    m = out["merits"]
    assert np.all(m[1:] <= m[:-1])
    print(f"pr2 at the closing door: done {int((out['iters'] <= 200).sum())}/{SC.N_PR2_FULL}, determined "
          f"{int(out['determined'].sum())}")
    assert SQ[0, 0] == 2.0 and SQ[0, SC.case('pr2').n_wp - 1] == 1.2
    assert (out["iters"] <= 200).any()
