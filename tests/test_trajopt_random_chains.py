"""The random-chain cases of kin_traj_opt_batch (tests/trajopt_cases.py) and the CPU restatement on them, without
the kernel: the guard of CHAIN_SEED / DATA_SEED.  Everything tests/test_gpu_traj_random_chains.py relies on is
shown here by the restatement alone.

Measured on the CPU (8 iterations, the restatement forward against itself with every sum reversed; the FK and the
Jacobians are the oracle's in both, so this is the rounding freedom of the restatement's own sums):
  case               n_wp  n_dof  max |X - X_rev|  max |merit - merit_rev|
  chain0-nobase         5      3      3.3e-16         9.2e-16
  chain0-base          10      6      4.4e-16         1.2e-17
  chain1-nobase        20      4      1.3e-15         8.9e-15
  chain1-base          33      7      1.6e-14         5.8e-17
  chain2-nobase         5      6      1.5e-16         3.6e-15
  chain2-base          10      9      2.6e-15         5.3e-16
  chain3-nobase        20      8      2.2e-16         1.4e-14
  chain3-base          33     11      1.1e-15         9.9e-16
  chain4-nobase         5     10      4.4e-16         1.7e-16
  chain4-base          10     13      6.7e-16         3.8e-17
  chain5-nobase        20     12      1.1e-15         1.5e-17
  chain5-base          33     15      1.1e-14         4.0e-17
  chain6-nobase         5     14      2.2e-15         4.0e-15
  chain6-base          10     17      1.9e-15         1.2e-16
  chain7-nobase        20     16      4.5e-15         3.4e-17
  chain7-base          33     19      3.3e-15         6.9e-15
  chain7-base-wide     64     19      7.9e-15         5.3e-15
SPREAD8_RC = 1.6e-14 is the largest (1.554e-14, chain1-base, rounded up).  Over the set the restatement takes 623
accepted and 427 rejected steps in 8 iterations, and 7 cases end with coordinates on a joint limit
that X0 did not have there.
"""
import numpy as np
import pytest

import oracle as O
import trajopt_cases as TC
import trajopt_ref as R

SPREAD8_RC = 1.6e-14     # the largest spread of the table above


def _spread(key):
    a, b = TC.ref_run(key, 8), TC.ref_run(key, 8, rev=True)
    return np.abs(a["X"] - b["X"]).max(), np.abs(a["info"][0] - b["info"][0]).max()


def _W(cs):
    return np.ones(cs.n_dof) if cs.dof_weights is None else cs.dof_weights ** 2


def test_case_generator_covers_the_paths():
    """Step counts at both ends of every bound; trees carry one off-path column; every chain holds path joints out
    of the batch; oblique / unnormalised axes, prismatic joints in mid-chain and continuous joints are all there;
    every L meets every bound; the wide case has >= 17 q columns at n_wp = 64; one case has > 64 boxes, one has no
    dof_weights; with the base there is a sphere on the root link."""
    kinds, mid_prismatic = set(), 0
    for i, nb in enumerate(TC.STEPS):
        ch = TC.chain(i)
        assert int(ch.on.sum()) == nb and ch.held
        assert len(ch.q_ids) - nb == (1 if TC.is_tree(i) else 0)
        assert ch.spheres[0][0] == ch.leaf and 3 <= len(ch.spheres) <= 6
        t = ch.tree
        batch_on = [j for j, o in zip(ch.q_ids, ch.on) if o]
        for j in batch_on:
            ax = t.joint_axis[j - 1]
            kinds.add(("prismatic" if t.joint_type[j - 1] == O.PRISMATIC else
                       "continuous" if not np.isfinite(t.joint_lower[j - 1]) else "revolute",
                       "oblique" if np.count_nonzero(ax) > 1 else "aligned"))
        order = [j for j in ch.path if j in batch_on]
        mid_prismatic += any(t.joint_type[j - 1] == O.PRISMATIC for j in order[1:-1])
    assert kinds == {(k, a) for k in ("prismatic", "continuous", "revolute") for a in ("oblique", "aligned")}
    assert mid_prismatic >= 4
    seen = set()
    for key in TC.CASES:
        cs = TC.case(key)
        seen.add((cs.bound, cs.n_wp))
        assert cs.X0.shape == (TC.N_TRAJ, cs.n_wp, cs.n_dof)
        assert (cs.spheres[-1][0] == cs.ch.root) == cs.with_base
        assert np.all(cs.X0 >= cs.sc.lo) and np.all(cs.X0 <= cs.sc.hi)
        for c in cs.off_cols:
            assert np.all(cs.X0[:, :, c] == cs.X0[0, 0, c]) and cs.sc.lo[c] < cs.X0[0, 0, c] < cs.sc.hi[c]
    assert seen >= {(b, n) for b in (4, 8, 12, 16) for n in TC.N_WPS}
    wide = TC.case(TC.WIDE)
    assert wide.n_dof >= 17 and wide.n_wp == 64 and wide.bound == 16
    assert 62 * 62 * 8 + 256 * wide.n_dof * 8 > 65536       # fp64: the 256-lane workgroup does not fit LDS
    assert len(TC.case(TC.MANY_BOXES).sc.box_poses) == 70 and TC.case(TC.MANY_BOXES).bound == 8
    assert TC.case(TC.NO_WEIGHTS).dof_weights is None and TC.case(TC.NO_WEIGHTS).bound == 4
    assert sum(TC.case(k).dof_weights is None for k in TC.CASES) == 1


@pytest.mark.parametrize("key", TC.CASES, ids=TC.cid)
def test_scene_matches_the_oracle(key):
    """The generalised scene's distances equal O.coll_batch's to 1e-12 on X0; the analytic SDF gradient agrees with
    the oracle's forward difference on >= 99 % of the sphere centres (test_union_box_sdf_matches_the_oracle)."""
    cs = TC.case(key)
    sc = cs.sc
    Q = R.to_columns(cs.X0)
    d, g = sc.distances(Q)
    sdf = O.OracleUnionSDF(sc.box_poses, sc.box_widths)
    dref, _ = O.coll_batch(sc.om, sdf, Q, sc.ids, sc.sph, sc.rad, with_grad=False)
    assert np.abs(d - dref).max() <= 1e-12
    poses = sc.om.fk_batch(Q, sc.ids, sc.sph)
    C = np.transpose(poses[:, 9:12, :], (0, 2, 1)).reshape(-1, 3)
    gref = np.array([sdf.gradient(x) for x in C])
    assert (np.abs(g.reshape(-1, 3) - gref).max(1) < 1e-5).mean() >= 0.99


@pytest.mark.parametrize("key", TC.CASES, ids=TC.cid)
def test_restatement_on_the_case(key):
    """Per case: at least 4 of the 9 trajectories are determined after 8 iterations and start with a positive
    penalty; the off-path column stays; the forward / reversed spread is within SPREAD8_RC; the merit does not
    increase over 40 iterations."""
    cs = TC.case(key)
    ref8 = TC.ref_run(key, 8)
    f0, sm0, _, _ = R.merit(cs.sc, cs.X0, TC.KW["margin"], TC.KW["band"], TC.KW["weight"], _W(cs))
    good = ref8["determined"] & (f0 - sm0 > 0)
    sx, sf = _spread(key)
    print(f"{TC.cid(key)}: determined with a penalty {int(good.sum())}/9, spread X {sx:.2e} merit {sf:.2e}, "
          f"ends feasible {cs.ends_feasible}")
    assert good.sum() >= 4
    for c in cs.off_cols:
        assert np.array_equal(ref8["X"][:, :, c], cs.X0[:, :, c])
    assert max(sx, sf) <= SPREAD8_RC
    m = TC.ref_run(key, 40)["merits"]
    assert np.all(m[1:] <= m[:-1])


def clamped(cs, X):
    """Interior coordinates of X on a finite limit that X0 did not have there."""
    Xi, X0i = X[:, 1:-1], cs.X0[:, 1:-1]
    fin_lo, fin_hi = np.isfinite(cs.sc.lo), np.isfinite(cs.sc.hi)
    on = ((Xi == cs.sc.lo) & fin_lo) | ((Xi == cs.sc.hi) & fin_hi)
    return int((on & (Xi != X0i)).sum())


def test_decisions_and_clamps_over_the_set():
    """Over the set both accept and reject decisions occur, and in at least two cases the clamp is active: an
    interior coordinate of the 8-iteration result sits exactly on a finite limit (and did not in X0)."""
    acc = rej = n_clamp = 0
    for key in TC.CASES:
        ref8 = TC.ref_run(key, 8)
        acc += int((ref8["accepts"] == 1).sum())
        rej += int((ref8["accepts"] == 0).sum())
        n_clamp += clamped(TC.case(key), ref8["X"]) > 0
    print(f"accepts {acc}, rejects {rej}, cases with an active clamp {n_clamp}")
    assert acc > 0 and rej > 0 and n_clamp >= 2
