"""kin_traj_opt_tree_batch without a GPU: the argument checks that precede any device work, and the cases of
tests/trajopt_tree_cases.py with the CPU restatement (tests/trajopt_ref.py, which takes spheres on any links) alone:
the guard of the seeds.  Everything tests/test_gpu_traj_tree.py relies on is shown here by the restatement.

Measured on the CPU (8 iterations, the restatement forward against itself with every sum reversed):
  case            n_wp  n_dof  part bounds    determined  max |X - X_rev|  max |merit - merit_rev|
  twoarm-nobase     10      9  8, 8              9/9        1.0e-15          1.8e-15
  twoarm-base        5     12  8, 8              7/9        2.2e-16          5.6e-17
  pr2               10     17  8, 8              5/9        1.4e-14          4.2e-15
  tree0             20     16  16, 4             7/9        1.8e-12          2.3e-13
  tree1             33     14  12, 8, 4          9/9        3.6e-15          4.4e-15
  tree2             64     14  8, 8, 4, 4        9/9        9.2e-16          7.1e-15
  tree3             10     17  8, 4, 4, 4        8/9        1.4e-15          1.4e-16
SPREAD8_TREE = 1.8e-12 is the largest (1.78e-12, tree0, rounded up).  The PR2 full run (6 trajectories, 200
iterations): 5 of 6 done, 4 determined.
"""
import ctypes as C

import numpy as np
import pytest

import trajopt_ref as R
import trajopt_tree_cases as TT
from kinhip import _lib as K
from test_trajopt import _prm

SPREAD8_TREE = 1.8e-12     # the largest spread of the table above


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
    """The table of tests/test_trajopt.py::test_parameter_checks_before_device through the new entry point: every
    parameter limit is refused on the host, under the new entry point's name, before the plan is looked at."""
    L = K.lib()
    prm = _prm(**kw)
    assert L.kin_traj_opt_tree_batch(None, None, C.byref(prm), None, 0, 1, None, None, 0, None) == code
    assert word in L.kin_last_error() and b"kin_traj_opt_tree_batch" in L.kin_last_error()
    good = _prm()
    assert L.kin_traj_opt_tree_batch(None, None, C.byref(good), None, 0, 1, None, None, 0, None) == K.KIN_E_INVALID
    assert b"null plan" in L.kin_last_error()
    assert L.kin_traj_opt_tree_batch(None, None, None, None, 0, 1, None, None, 0, None) == K.KIN_E_INVALID
    v = C.c_int32()
    assert L.kin_plan_part_count(None, C.byref(v)) == K.KIN_E_INVALID
    assert L.kin_plan_part_chain_bound(None, 0, C.byref(v)) == K.KIN_E_INVALID


def _W(cs):
    return np.ones(cs.n_dof) if cs.dof_weights is None else cs.dof_weights ** 2


def test_case_generator_covers_the_paths():
    """The part counts and bounds the issue asks for (restated grouping; the GPU file asserts them on the plans): two
    arms; a plan with parts of bound 16 and 4; a bound-12 part; an off-chain column; a root sphere with the base;
    L = 8, 16, 32, 64; at most 20 columns; every part owns a box."""
    want = {"twoarm-nobase": [8, 8], "twoarm-base": [8, 8], "pr2": [8, 8], "tree0": [16, 4], "tree1": [12, 8, 4],
            "tree2": [8, 8, 4, 4], "tree3": [8, 4, 4, 4]}
    Ls = set()
    for name in TT.CASES:
        cs = TT.case(name)
        assert cs.bounds == want[name], (name, cs.bounds)
        assert sorted(k for p in cs.parts for k in p) == list(range(len(cs.spheres)))
        assert cs.n_dof <= 20 and cs.X0.shape == (TT.N_TRAJ, cs.n_wp, cs.n_dof)
        assert np.all(cs.X0 >= cs.sc.lo) and np.all(cs.X0 <= cs.sc.hi)
        assert set(cs.box_parts) == set(range(min(4, len(cs.parts))))
        for c in cs.off_cols:
            assert np.all(cs.X0[:, :, c] == cs.X0[0, 0, c])
        Ls.add(8 if cs.n_wp <= 8 else 16 if cs.n_wp <= 16 else 32 if cs.n_wp <= 32 else 64)
        if name.startswith("tree"):
            assert all(len(p) >= 1 for p in cs.parts) and 2 * len(cs.parts) <= len(cs.spheres) <= 4 * len(cs.parts) + 1
    assert Ls == {8, 16, 32, 64}
    assert TT.case("pr2").n_dof == 17 and TT.case("tree1").off_cols.size == 1 and TT.case("tree3").with_base
    assert TT.case(TT.MIXED_BOUNDS).bounds == [16, 4] and TT.case(TT.WP64).n_wp == 64
    assert sum(TT.case(n).dof_weights is None for n in TT.CASES) == 1


def test_half_gradient_matches_central_differences():
    """On tree1 (three parts, an off-chain column): the restatement's half-gradient g against central differences of
    its merit, (f(x + h e) - f(x - h e)) / 2h = 2 g, h = 1e-6, to 1e-5 (the project's finite-difference agreement,
    tests/test_trajopt_pose.py) on >= 99 % of the coordinates (the merit has kinks at the band's edge and on the
    boxes' mid-planes, as tests/test_trajopt.py::test_union_box_sdf_matches_the_oracle)."""
    cs = TT.case("tree1")
    X0 = cs.X0[:4]
    W = _W(cs)
    f0, _, _, g = R.merit(cs.sc, X0, TT.KW["margin"], TT.KW["band"], TT.KW["weight"], W)
    assert np.abs(g).max() > 1e-2
    h, err = 1e-6, []
    rng = np.random.default_rng(3)
    for w in rng.choice(np.arange(1, cs.n_wp - 1), 6, replace=False):
        for d in range(cs.n_dof):
            Xp, Xm = X0.copy(), X0.copy()
            Xp[:, w, d] += h
            Xm[:, w, d] -= h
            fp = R.merit(cs.sc, Xp, TT.KW["margin"], TT.KW["band"], TT.KW["weight"], W)[0]
            fm = R.merit(cs.sc, Xm, TT.KW["margin"], TT.KW["band"], TT.KW["weight"], W)[0]
            err.append(np.abs((fp - fm) / (4 * h) - g[:, w - 1, d]))
    err = np.array(err)
    print(f"half-gradient vs central differences: max {err.max():.2e}, within 1e-5: {(err < 1e-5).mean():.4f}")
    assert (err < 1e-5).mean() >= 0.99


@pytest.mark.parametrize("name", TT.CASES)
def test_case_conditions(name):
    """Conditions on the inputs, met by the restatement alone: at least 4 trajectories determined after 8
    iterations; every part has a sphere inside margin + band at X0 in at least one determined trajectory; the
    off-chain column stays; the merit does not increase over 40 iterations."""
    cs = TT.case(name)
    ref8 = TT.ref_run(name, 8)
    det = ref8["determined"]
    inside = TT.inside_band(cs)
    print(f"{name}: determined {int(det.sum())}/9, parts inside the band on determined trajectories "
          f"{[int((inside[p] & det).sum()) for p in range(len(cs.parts))]}")
    assert det.sum() >= 4
    assert all((inside[p] & det).any() for p in range(len(cs.parts)))
    for c in cs.off_cols:
        assert np.array_equal(ref8["X"][:, :, c], cs.X0[:, :, c])
    m = TT.ref_run(name, 40)["merits"]
    assert np.all(m[1:] <= m[:-1])


@pytest.mark.parametrize("name", TT.CASES)
def test_spread(name):
    """The restatement forward against itself with every sum reversed, 8 iterations: within SPREAD8_TREE."""
    a, b = TT.ref_run(name, 8), TT.ref_run(name, 8, rev=True)
    sx, sf = np.abs(a["X"] - b["X"]).max(), np.abs(a["info"][0] - b["info"][0]).max()
    print(f"{name}: spread X {sx:.2e} merit {sf:.2e}")
    assert max(sx, sf) <= SPREAD8_TREE


def test_pr2_full_run_restatement():
    """PR2, both arms and the base, 6 trajectories, 200 iterations: the merit never increases, and both arms are
    inside the band at X0 in some trajectory (the count done within 200 iterations is what the GPU test pins)."""
    cs = TT.case("pr2")
    out = TT.pr2_full()
    m = out["merits"]
    assert np.all(m[1:] <= m[:-1])
    print(f"pr2: done {int((out['iters'] <= 200).sum())}/{TT.N_PR2_FULL}, determined {int(out['determined'].sum())}")
    assert TT.inside_band(cs, cs.X0[:TT.N_PR2_FULL]).any(1).all()
