"""Cases for kin_traj_opt_pose_tree_batch (k_traj_pose_tree): a pose link held at a waypoint on robots whose spheres
hang off several chains (the scenes of tests/trajopt_tree_cases.py) and against boxes attached to a moving scene (those
of tests/trajopt_scene_cases.py).  The restatement is tests/trajopt_pose_ref.py's run(), unchanged: it takes any scene
object with om / ids / distances.  Shared by tests/test_trajopt_pose_tree.py (the restatement alone, on the CPU) and
tests/test_gpu_traj_pose_tree.py (the kernel).  Not a test module; everything here is cached and read-only.

A case takes the robot, boxes, X0 and dof_weights of its base case; its targets are the link's pose at waypoint c of
X0 moved by trajopt_pose_ref.SHIFT and, with 6 rows, turned by YAW (family_targets).  Two departures, both because the
restatement's own forward / reversed spread after 8 iterations was past 1e-11 (an ill-conditioned case, measured on the
CPU, tests/test_trajopt_pose_tree.py):
  twoarm-l6 / -r6   6 rows on a chain of 5 joints (the torso and a 4-joint arm, no base): J has 5 columns, so
                    S = J W^-1 J^T + damp I is singular but for damp and its condition number is ~ 1 / damp.  These two
                    run with damp = 1e-2 instead of 1e-6 (spread 2.3e-10 -> 7.4e-14, 9.6e-11 -> 1.0e-13).
  pr2               SHIFT and YAW halved (MOVE = 0.5): with the whole move trajectory 1 amplifies rounding to 3.2e-11
                    (the other eight stay below 7e-13); halved, the case's spread is 2.0e-13.

  name              base case (module)       link                     n_wp  c  rows  what it is for
  twoarm-l3/-l6     twoarm-nobase (tree)     l_grip                    10   5  3/6   the two arms: one of the two links
  twoarm-r3/-r6     twoarm-nobase (tree)     r_grip                    10   5  3/6   rides on part 1
  base-c1, base-c3  twoarm-base (tree)       l_grip                     5  1,3  6/3  the ends; base columns in J
  pr2               pr2 (tree)               l_gripper_tool_frame      10   5   6    two fixed joints past the wrist
  tree3             tree3 (tree)             the leaf of the last part 10   5   6    a bound-4 part: identity padding
  s-fetch           fetch (scene)            gripper_link              10   5   6    one-entry table, a door angle per waypoint
  s-pr2             pr2 (scene)              l_gripper_tool_frame      10   5   3    the door swinging, two parts
  s-uniform         fetch-uniform (scene)    gripper_link              10   5   6    lds = 0
  pr2-wp64          pr2 (tree), 2 traj.      l_gripper_tool_frame      64  32   6    fp64: the halved workgroup
pr2-wp64's X0 is the first two trajectories of pr2's, resampled linearly to 64 waypoints."""
import functools
from dataclasses import dataclass

import numpy as np

import trajopt_pose_ref as P
import trajopt_ref as R
import trajopt_scene_cases as SC
import trajopt_tree_cases as TT
from trajopt_cases import KW, PAD, SENT  # noqa: F401

DAMP = {"twoarm-l6": 1e-2, "twoarm-r6": 1e-2}      # else trajopt_pose_ref.DAMP
MOVE = {"pr2": 0.5}                                # the fraction of SHIFT / YAW the targets are moved by (else 1)
# name -> (module, base case, link name (None: tree3's leaf), c, rows)
SPECS = {
    "twoarm-l3": ("tree", "twoarm-nobase", "l_grip", 5, 3), "twoarm-l6": ("tree", "twoarm-nobase", "l_grip", 5, 6),
    "twoarm-r3": ("tree", "twoarm-nobase", "r_grip", 5, 3), "twoarm-r6": ("tree", "twoarm-nobase", "r_grip", 5, 6),
    "base-c1": ("tree", "twoarm-base", "l_grip", 1, 6), "base-c3": ("tree", "twoarm-base", "l_grip", 3, 3),
    "pr2": ("tree", "pr2", "l_gripper_tool_frame", 5, 6),
    "tree3": ("tree", "tree3", None, 5, 6),
    "s-fetch": ("scene", "fetch", "gripper_link", 5, 6),
    "s-pr2": ("scene", "pr2", "l_gripper_tool_frame", 5, 3),
    "s-uniform": ("scene", "fetch-uniform", "gripper_link", 5, 6),
    "pr2-wp64": ("tree", "pr2", "l_gripper_tool_frame", 32, 6),
}
CASES = list(SPECS)
STATIC = [n for n in CASES if SPECS[n][0] == "tree"]
SCENE = [n for n in CASES if SPECS[n][0] == "scene"]
WP64 = "pr2-wp64"
N_PR2_FULL = 6               # trajectories of the PR2 full runs (200 iterations)


@dataclass
class Case:
    name: str
    base: object         # the base case (trajopt_tree_cases.Case or trajopt_scene_cases.Case)
    scene: bool          # an attached union (base.SQ, base.scene_path, ...)
    sc: object           # the restatement's scene (ChainScene, or AttachedScene bound to (X0, SQ))
    link: int            # the pose link (link id of the robot's tree)
    c: int
    with_rot: bool
    X0: np.ndarray       # [n_traj, n_wp, n_dof]
    targets: np.ndarray  # [12, n_traj]
    part: int            # the part that carries the link (restated: the first whose spine is comparable)
    damp: float

    @property
    def n_wp(self):
        return self.X0.shape[1]

    @property
    def n_traj(self):
        return self.X0.shape[0]

    @property
    def dof_weights(self):
        return self.base.dof_weights


def _root_path(tree, x):
    pj = {int(c): k + 1 for k, c in enumerate(tree.joint_clink)}
    out = [int(x)]
    while out[-1] in pj:
        out.append(int(tree.joint_plink[pj[out[-1]] - 1]))
    return out


def carrying_part(base, link):
    """kin_traj_plan_create's rule restated: the first part, in plan order, whose spine (the anchor of its spheres with
    the most batch joints above it) is above, at or below the link's anchor (anchor: the nearest link below a batch
    joint)."""
    tree = base.rb.tree
    pj = {int(c): k + 1 for k, c in enumerate(tree.joint_clink)}
    batch = {int(j) for j in base.rb.q_ids}

    def anchor_path(x):
        path = _root_path(tree, x)
        while len(path) > 1 and pj[path[0]] not in batch:
            path = path[1:]
        return path

    def depth(path):
        return sum(pj[x] in batch for x in path[:-1])

    a = anchor_path(link)
    for p, grp in enumerate(base.parts):
        spine = max((anchor_path(base.spheres[k][0]) for k in grp), key=depth)
        if a[0] in spine or spine[0] in a:
            return p
    return -1


def _leaf_of_last_part(base):
    tree = base.rb.tree
    return max((base.spheres[k][0] for k in base.parts[-1]), key=lambda l: len(_root_path(tree, l)))


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    mod, bname, lname, c, rows = SPECS[name]
    base = (SC if mod == "scene" else TT).case(bname)
    link = _leaf_of_last_part(base) if lname is None else base.rb.tree.link_id(lname)
    X0, sc = base.X0, base.sc
    if name == WP64:
        w = np.linspace(0.0, base.n_wp - 1.0, 64)
        X0 = np.stack([np.stack([np.interp(w, np.arange(base.n_wp), base.X0[t, :, d]) for d in range(base.n_dof)], 1)
                       for t in range(2)])
        X0[:, 0], X0[:, -1] = base.X0[:2, 0], base.X0[:2, -1]
    tg = targets_of(sc, link, X0, c, rows == 6, MOVE.get(name, 1.0))
    return Case(name, base, mod == "scene", sc, link, c, rows == 6, X0, tg, carrying_part(base, link),
                DAMP.get(name, P.DAMP))


def targets_of(sc, link, X0, c, with_rot, move=1.0):
    """trajopt_pose_ref.family_targets with SHIFT and YAW scaled by `move`."""
    if move == 1.0:
        return P.family_targets(sc, link, X0, c, with_rot)
    Rm, p = P.mat_of(sc.om.fk_batch(np.ascontiguousarray(X0[:, c].T), sc.ids, [link])[0])
    if with_rot:
        cz, sz = np.cos(move * P.YAW), np.sin(move * P.YAW)
        Rm = np.einsum("ab,nbc->nac", np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]]), Rm)
    return P.pose12_of(Rm, p + move * np.asarray(P.SHIFT))


def run_case(cs, max_iters, rev=False, X0=None, targets=None, sc=None):
    """trajopt_pose_ref.run on the case (X0 / targets: a subset of its trajectories; sc: another scene for them)."""
    return P.run(cs.sc if sc is None else sc, cs.link, cs.c, cs.with_rot, cs.targets if targets is None else targets,
                 cs.X0 if X0 is None else X0, max_iters=max_iters, dof_weights=cs.dof_weights, rev=rev, damp=cs.damp,
                 **KW)


@functools.lru_cache(maxsize=None)
def ref_run(name, max_iters, rev=False):
    return run_case(case(name), max_iters, rev)


def sub_scene(cs, part):
    """The single-part sub-problem of a static case: the same robot, boxes and X0 with one part's spheres."""
    return TT.sub_scene(cs.base, tuple(cs.base.parts[part]))


@functools.lru_cache(maxsize=None)
def pr2_full(scene, rows):
    """The PR2 family, N_PR2_FULL trajectories, 200 iterations, the left tool frame at waypoint 5: static (the pr2 case
    of tests/trajopt_tree_cases.py) or with the door closing from 2.0 to 1.2 (tests/trajopt_scene_cases.py's pr2_full)
    -> dict(sc, SQ (None: static), X0, targets, out)."""
    n = N_PR2_FULL
    if scene:
        sc, SQ, _ = SC.pr2_full()
        base = SC.case("pr2")
    else:
        base, SQ = TT.case("pr2"), None
        sc = base.sc
    X0 = base.X0[:n]
    link = base.rb.tree.link_id("l_gripper_tool_frame")
    tg = P.family_targets(sc, link, X0, 5, rows == 6)
    out = P.run(sc, link, 5, rows == 6, tg, X0, max_iters=200, dof_weights=base.dof_weights, **KW)
    return dict(sc=sc, SQ=SQ, X0=X0, targets=tg, out=out, link=link, base=base)
