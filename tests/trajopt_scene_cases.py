"""Cases for kin_traj_opt_scene_batch (k_traj_scene): robots planning against boxes attached to a moving scene, every
waypoint of every trajectory with its own scene state.  Shared by tests/test_trajopt_scene.py (the cases and the
restatement alone, on the CPU) and tests/test_gpu_traj_scene.py (the kernel).  Not a test module; everything here is
cached and must be treated as read-only.

Cases (9 trajectories unless stated; dof_weights = U(0.5, 2)^n_dof; the parameters KW of tests/trajopt_cases.py):
  fetch          Fetch (the planning scene's spheres, one chain of bound 8, 8 columns) at tests/golden/fridge.urdf (its
                 base group and its door), n_wp = 10 (L = 16: four segments per wave, three waves); a distinct door
                 angle per (trajectory, waypoint) -- the door swings 0.3-0.9 rad over a trajectory -- and a fridge
                 base pose per trajectory.
  fetch-one      the same with n_traj = 1, n_wp = 5 (L = 8, invalid lanes, idle segments in the wave).
  pr2            tests/golden/pr2_two_arms.urdf with the planar base, the torso held, vcat(rarm, larm),
                 PR2_ARM_SPHERES: 17 columns, two parts of bound 8; n_wp = 10; the door swings over the waypoints and
                 the fridge base differs per trajectory.
  tree0          tree0 of tests/trajopt_tree_cases.py (parts of bound 16 and 4) against a seeded scene in the style of
                 tests/randtree.py (random origins with rpy, boxes with rotated origins on fixed child links): no
                 base, one revolute batch joint about an oblique unnormalised axis, 3 boxes on the root and 2 on the
                 child; n_wp = 33 (L = 64).  (randtree.random_urdf itself cannot be asked for a shape: the text is
                 written here with its conventions.)
  wide           the bound-16 chain with base of tests/trajopt_cases.py (19 q columns) at n_wp = 64 (fp64: the halved
                 workgroup) against a drawer: one prismatic batch joint with an unnormalised axis, 70 boxes (35 on
                 the root, 35 on the drawer; 4 of them placed, 66 scattered in a 3 m cube), so the union is read
                 from global memory.
  fetch-uniform  fetch with one scene state for the whole launch (lds = 0): that of trajectory 0's middle waypoint.
  fetch-padded   fetch with lds > n_traj * n_wp: the restatement is fetch's; the GPU test pads scene_q and xi with NaN
                 and puts sentinels around every array.

Placement.  At the fridge (a planar base is the only freedom): for trajectory t a sphere of its middle waypoint is put
0.005-0.04 outside a side face of a fridge box whose height range holds the sphere -- a door box for even t (the moving
group), a base-group box for odd t -- by the fridge's base pose (a random yaw, then x, y).  In the written scenes box
k is placed around a sphere of part k mod n_parts of trajectory k at its middle waypoint and that sample's scene
state (the sphere 0.15-0.6 half-widths off the box centre along every box axis, as tests/trajopt_cases.py), root and
child boxes alternating.

The seeds are the first (SEED0 + 10 case + 100 k) at which the restatement alone meets the conditions of
tests/test_trajopt_scene.py::test_case_conditions."""
import functools
import os
import tempfile
from dataclasses import dataclass

import numpy as np

import oracle as O
import trajopt_cases as TC
import trajopt_ref as R
import trajopt_scene_ref as SR
import trajopt_tree_cases as TT
from conftest import ARM, golden
from trajopt_cases import KW, N_TRAJ, PAD, SENT, _rot_pose  # noqa: F401

CASES = ["fetch", "fetch-one", "pr2", "tree0", "wide", "fetch-uniform", "fetch-padded"]
# (robot, robot base, n_wp, n_traj, scene)
SHAPES = {"fetch": ("fetch", False, 10, N_TRAJ, "fridge"), "fetch-one": ("fetch", False, 5, 1, "fridge"),
          "pr2": ("pr2", True, 10, N_TRAJ, "fridge"), "tree0": ("tree0", False, 33, N_TRAJ, "hinge"),
          "wide": ("wide", True, 64, N_TRAJ, "drawer")}
SEED0 = 8100
# the first data seed offset (SEED0 + 10 case + 100 k) that meets test_case_conditions, found on the CPU
SEED_K = {"fetch": 0, "fetch-one": 0, "pr2": 0, "tree0": 0, "wide": 0}
MULTI_PART = ("pr2", "tree0")
N_PR2_FULL = 6               # trajectories of the PR2 full run (200 iterations)
BAND = KW["margin"] + KW["band"]

# ---- measured (tables in tests/test_trajopt_scene.py, tests/test_gpu_traj_scene.py and DESIGN.md 4.8.3) -------------
SPREAD8_SCENE = 5.0e-12      # the restatement forward / reversed after 8 iterations, CPU: 4.94e-12 (wide's merit)
# The existing kernels (k_traj for the single-chain plans, k_traj_tree for pr2 and tree0; unchanged by the scene variant)
# on the frozen sub-cases against their own restatement, MI355X (fp64 8 iterations on the determined trajectories, max of
# |dX| and |d merit|; fp32 1 iteration |X32 - X_ref|):
#   fetch state 0       8.54e-13  6.78e-7      pr2 state 0     1.12e-13  6.86e-7      tree0 state 0   1.13e-13  2.22e-6
#   fetch state 1       6.22e-15  3.22e-7      pr2 state 1     2.09e-13  6.97e-7      tree0 state 1   5.90e-12  2.22e-6
#   fetch-one state 0   2.22e-16  9.56e-8                                              wide state 0    3.65e-12  1.11e-6
D8_STATIC = 6.0e-12          # measured 5.90e-12 (tree0 frozen at trajectory 1's middle waypoint)
D32_STATIC = 2.3e-6          # measured 2.223e-6 (tree0)
# so TOL8_SCENE = max(10 x 5.0e-12, 4 x 6.0e-12) = 5.0e-11 and DELTA32_SCENE = 4 x 2.3e-6 = 9.2e-6 (tests/test_gpu_traj_scene.py)


@functools.lru_cache(maxsize=None)
def robot(name) -> TT.Robot:
    if name == "fetch":
        import kinhip
        p = golden("fetch.urdf")
        t = O.parse_urdf_tree(p)
        sph = [(t.link_id(n), np.array(c, np.float64), float(r)) for n in R.COLL_LINKS
               for c, r in kinhip.FETCH_LINK_SPHERES[n]]
        return TT.Robot(name, None, p, t, [t.joint_id(n) for n in ARM], [], np.zeros(0), sph, np.zeros(0, int), None)
    if name == "wide":
        cs = TC.case(TC.WIDE)
        ch = cs.ch
        return TT.Robot(name, ch.text, None, ch.tree, list(ch.q_ids), list(ch.held), np.asarray(ch.held_ang), list(cs.spheres),
                        np.asarray(cs.off_cols, int), None)
    return TT.robot(name)


# ---- written scenes -----------------------------------------------------------------------------------------------
def _fmt(v):
    return " ".join(repr(float(x)) for x in v)


def _scene_text(jtype, j_xyz, j_rpy, axis, fixed, boxes):
    """root --(jtype joint "move")--> child; link b<k> fixed to the root or the child by a fixed joint with origin
    fixed[k] = (parent, xyz, rpy) and carrying box k = (size, origin xyz, origin rpy) or None."""
    out = ['<robot name="scene">', '  <link name="root"/>', '  <link name="child"/>']
    for k, bx in enumerate(boxes):
        out.append(f'  <link name="b{k}">')
        if bx is not None:
            out.append(f'    <collision><origin xyz="{_fmt(bx[1])}" rpy="{_fmt(bx[2])}"/>'
                       f'<geometry><box size="{_fmt(bx[0])}"/></geometry></collision>')
        out.append('  </link>')
    lim = '<limit lower="-3" upper="3" effort="1" velocity="1"/>'
    out.append(f'  <joint name="move" type="{jtype}"><parent link="root"/><child link="child"/>'
               f'<origin xyz="{_fmt(j_xyz)}" rpy="{_fmt(j_rpy)}"/><axis xyz="{_fmt(axis)}"/>{lim}</joint>')
    for k, (parent, xyz, rpy) in enumerate(fixed):
        out.append(f'  <joint name="f{k}" type="fixed"><parent link="{parent}"/><child link="b{k}"/>'
                   f'<origin xyz="{_fmt(xyz)}" rpy="{_fmt(rpy)}"/></joint>')
    return "\n".join(out + ["</robot>"])


def _written_scene(kind, rng, want):
    """want: [(parent, world pose 4x4 wanted, scene value at which it is wanted, size)] -> URDF text.  Two passes: the
    links' frames from the text without boxes, then every box origin = inv(link frame at that scene value) * pose."""
    axis = np.zeros(3)
    while np.abs(axis).min() < 0.2:                  # oblique: no component near 0
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
    if kind == "hinge":
        jtype, axis = "revolute", axis * rng.uniform(1.5, 2.5)                   # unnormalised (the direction counts)
    else:
        jtype, axis = "prismatic", axis * rng.uniform(0.6, 0.8)                  # unnormalised (axis * value: it counts)
    j_xyz, j_rpy = rng.uniform(-0.3, 0.3, 3), rng.uniform(-np.pi, np.pi, 3)
    fixed = [(p, rng.uniform(-0.2, 0.2, 3), rng.uniform(-np.pi, np.pi, 3) * (rng.random() < 0.7)) for p, _, _, _ in want]
    t0 = O.parse_urdf_tree(_scene_text(jtype, j_xyz, j_rpy, axis, fixed, [None] * len(want)))
    om = O.OracleMech(t0)
    vals = np.array([[v for _, _, v, _ in want]])
    fr = om.fk_batch(vals, [t0.joint_id("move")], [t0.link_id(f"b{k}") for k in range(len(want))])   # [n, 12, n]
    boxes = []
    for k, (_, pose, _, size) in enumerate(want):
        org = np.linalg.inv(SR.pose_of(fr[k][:, k:k + 1])[0]) @ pose
        boxes.append((size, org[:3, 3], O.rpy(org)))
    return _scene_text(jtype, j_xyz, j_rpy, axis, fixed, boxes)


@dataclass
class Case:
    name: str
    rb: TT.Robot
    with_base: bool
    n_wp: int
    n_traj: int
    parts: list          # sphere indices per part, plan order
    bounds: list         # chain bound per part
    sc: object           # trajopt_scene_ref.AttachedScene, bound to (X0, SQ)
    X0: np.ndarray       # [n_traj, n_wp, n_dof]
    SQ: np.ndarray       # (n_scene_cols, n_traj * n_wp), or (n_scene_cols,) for fetch-uniform
    dof_weights: object
    off_cols: np.ndarray
    scene_path: str      # URDF file of the scene
    scene_base: bool
    scene_joints: list   # names of the scene's batch joints

    @property
    def n_dof(self):
        return self.sc.n_dof

    @property
    def spheres(self):
        return self.rb.spheres

    @property
    def mid_state(self):
        """The scene state of trajectory 0's middle waypoint (the frozen sub-case; fetch-uniform's one state)."""
        return self.SQ if self.SQ.ndim == 1 else self.SQ[:, self.n_wp // 2].copy()


_TMP = tempfile.mkdtemp(prefix="trajscene")


def _fridge():
    t = O.parse_urdf_tree(golden("fridge.urdf"))
    return t, True, [t.joint_id("door_joint")], golden("fridge.urdf"), ["door_joint"]


def build(name, seed) -> Case:
    rname, with_base, n_wp, nt, scene = SHAPES[name]
    rb = robot(rname)
    rng = np.random.default_rng(seed)
    rsc = R.ChainScene(rb.tree, with_base, rb.q_ids, rb.held, rb.held_ang, rb.spheres)
    parts, bounds = TT.sphere_parts(rb.tree, rb.q_ids, [s[0] for s in rb.spheres])
    nd, nc = rsc.n_dof, len(rb.q_ids)
    bounded = np.isfinite(rsc.lo) & np.isfinite(rsc.hi)
    flo, fhi = np.where(bounded, rsc.lo, -np.pi), np.where(bounded, rsc.hi, np.pi)
    flo[nc:], fhi[nc:] = -0.5, 0.5
    off_cols = rb.off_cols
    off_val = flo[off_cols] + (fhi[off_cols] - flo[off_cols]) * rng.uniform(0.3, 0.7, off_cols.size)

    def draw(n, start=False):
        q = flo[:, None] + (fhi - flo)[:, None] * rng.random((nd, n))
        if start and rb.start is not None:                   # (pr2: every trajectory starts at the manip pose)
            q[:nc] = rb.start[:, None]
            q[nc:] = 0.0
        q[off_cols] = off_val[:, None]
        return q

    starts, goals = draw(nt, True), draw(nt)
    bump = np.sin(np.pi * np.arange(n_wp) / (n_wp - 1))[None, :, None] * rng.normal(0, 0.05, (nt, 1, nd))
    bump[:, :, off_cols] = 0.0
    X0 = np.stack([R.straight_lines(starts[:, t], goals[:, t:t + 1], n_wp)[0] for t in range(nt)])
    X0[:, 1:-1] = np.clip(X0[:, 1:-1] + bump[:, 1:-1], rsc.lo, rsc.hi)
    mid = n_wp // 2
    cen = rsc.om.fk_batch(np.ascontiguousarray(X0[:, mid].T), rsc.ids, rsc.sph)[:, 9:12, :]      # [n_sph, 3, nt]
    ramp = np.arange(n_wp) / (n_wp - 1)
    if scene == "fridge":
        stree, sbase, sids, spath, snames = _fridge()
        door = rng.uniform(0.3, 1.0, nt)[:, None] + rng.uniform(0.3, 0.9, nt)[:, None] * ramp[None, :]   # [nt, n_wp]
        probe = SR.AttachedScene(rsc, stree, sbase, sids)
        SQ = np.zeros((4, nt * n_wp))
        for t in range(nt):
            WB = probe.world_boxes(np.array([door[t, mid], 0.0, 0.0, 0.0]))[0]                  # base at the origin
            cand = [(s, k) for s in range(len(rsc.sph)) for k in range(len(probe.boxes))
                    if abs(cen[s, 2, t] - WB[k][2, 3]) < 0.5 * probe.box_widths[k][2] - 0.02]
            pick = [c for c in cand if probe.group_moves[probe.box_group[c[1]]] == (t % 2 == 0)] or cand
            Qt = np.ascontiguousarray(X0[t].T)
            for _ in range(40):      # redrawn while two boxes tie on an in-band sphere of this trajectory (the fridge's
                th = rng.uniform(-np.pi, np.pi)                       # panels share face planes with its body)
                if pick:
                    s, k = pick[int(rng.integers(0, len(pick)))]
                    h = 0.5 * np.array(probe.box_widths[k])
                    i = int(rng.integers(0, 2))
                    l = np.array([0.0, 0.0, cen[s, 2, t] - WB[k][2, 3], 1.0])
                    l[i] = rng.choice([-1.0, 1.0]) * (h[i] + rsc.rad[s] + rng.uniform(0.005, 0.04))
                    l[1 - i] = rng.uniform(-0.6, 0.6) * h[1 - i]
                    p0 = WB[k] @ l
                    xy = cen[s, :2, t] - np.array([np.cos(th) * p0[0] - np.sin(th) * p0[1],
                                                   np.sin(th) * p0[0] + np.cos(th) * p0[1]])
                else:
                    xy = cen[0, :2, t] + rng.uniform(0.5, 0.8, 2)
                sq = np.stack([door[t], np.full(n_wp, xy[0]), np.full(n_wp, xy[1]), np.full(n_wp, th)])
                srt = np.sort(probe.per_box(Qt, sq)[:, :, 1:-1], axis=0)
                if not np.any((srt[0] < BAND) & (srt[1] - srt[0] < 1e-6)):
                    break
            SQ[:, t * n_wp:(t + 1) * n_wp] = sq
    else:
        if scene == "hinge":
            val = rng.uniform(-1.0, 1.0, nt)[:, None] + (rng.uniform(0.3, 0.9, nt) * rng.choice([-1.0, 1.0], nt))[:, None] * ramp
            n_placed, n_more = 5, 0
        else:
            val = rng.uniform(-0.2, 0.2, nt)[:, None] + (rng.uniform(0.1, 0.3, nt) * rng.choice([-1.0, 1.0], nt))[:, None] * ramp
            n_placed, n_more = 4, 66
        want = []
        for k in range(n_placed):
            size = tuple(rng.uniform(0.05, 0.2, 3))
            rpy = np.zeros(3) if k % 2 == 0 else rng.uniform(-1.0, 1.0, 3)
            s = int(rng.choice(parts[k % len(parts)]))
            off = rng.uniform(0.15, 0.6, 3) * rng.choice([-1.0, 1.0], 3) * 0.5 * np.array(size)
            pose = _rot_pose(rpy, cen[s, :, k] - O.rpy_to_matrix(rpy) @ off)
            want.append(("root" if k % 2 == 0 else "child", pose, float(val[k, mid]), size))
        for k in range(n_more):                                # scattered, wanted where they are with the joint at 0
            want.append(("root" if k % 2 == 0 else "child", _rot_pose(rng.uniform(-1, 1, 3) * (k % 3 != 0), rng.uniform(-1.5, 1.5, 3)),
                         0.0, tuple(rng.uniform(0.05, 0.2, 3))))
        text = _written_scene(scene, rng, want)
        spath = os.path.join(_TMP, f"{name}_{seed}.urdf")
        with open(spath, "w") as f:
            f.write(text)
        stree, sbase, snames = O.parse_urdf_tree(text), False, ["move"]
        sids = [stree.joint_id("move")]
        SQ = val.reshape(1, nt * n_wp).copy()
    sc = SR.AttachedScene(rsc, stree, sbase, sids).bind(X0, SQ)
    w = rng.uniform(0.5, 2.0, nd)
    return Case(name, rb, bool(with_base), n_wp, nt, parts, bounds, sc, X0, SQ, w, off_cols, spath, sbase, snames)


def seed_of(name, k=None):
    return SEED0 + 10 * CASES.index(name) + 100 * (SEED_K[name] if k is None else k)


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    if name in ("fetch-uniform", "fetch-padded"):
        cs = build("fetch", seed_of("fetch"))                # (an object of its own: its scene is bound separately)
        cs.name = name
        if name == "fetch-uniform":
            cs.SQ = cs.mid_state
            cs.sc.bind(cs.X0, cs.SQ)
        return cs
    return build(name, seed_of(name))


def run_case(cs, max_iters, rev=False, X0=None, sc=None):
    """trajopt_ref.run on the case (sc: another scene for the same robot and X0, e.g. a frozen snapshot)."""
    return R.run(cs.sc if sc is None else sc, cs.X0 if X0 is None else X0, max_iters=max_iters,
                 dof_weights=cs.dof_weights, rev=rev, **KW)


@functools.lru_cache(maxsize=None)
def ref_run(name, max_iters, rev=False):
    return run_case(case(name), max_iters, rev)


@functools.lru_cache(maxsize=None)
def frozen_states(name):
    """The scene states of the frozen sub-cases: the middle waypoints of trajectories 0 and 1 (of trajectory 0 alone
    for fetch-one and for wide, whose restatement takes the longest)."""
    cs = case(name)
    if cs.SQ.ndim == 1:
        return [cs.SQ.copy()]
    return [cs.SQ[:, t * cs.n_wp + cs.n_wp // 2].copy() for t in range(1 if name == "wide" else min(2, cs.n_traj))]


@functools.lru_cache(maxsize=None)
def frozen_ref(name, k, max_iters):
    """The restatement on frozen sub-case k: the same robot, boxes and X0, the scene a static union at one state."""
    cs = case(name)
    return run_case(cs, max_iters, sc=cs.sc.frozen(frozen_states(name)[k]))


def conditions(cs, det):
    """-> dict(moving: a determined trajectory has, at X0, a sphere inside the band whose nearest box rides on the
    moving group; parts: per part, some trajectory has a sphere of it inside the band at X0; gap: the smallest
    difference between the two smallest box distances of any in-band sphere (interior waypoints of X0))."""
    nt, n_wp, _ = cs.X0.shape
    Q = R.to_columns(cs.X0)
    pb = cs.sc.per_box(Q, cs.sc.samples_of(Q))                        # [n_box, n_sph, N]
    ns = pb.shape[1]
    pb = pb.reshape(pb.shape[0], ns, nt, n_wp)[:, :, :, 1:-1]
    srt = np.sort(pb, axis=0)
    d, near = srt[0], pb.argmin(0)                                    # [n_sph, nt, ni]
    inb = d < BAND
    mv = np.array([cs.sc.group_moves[g] for g in cs.sc.box_group])[near]
    moving = bool((inb & mv).any(axis=(0, 2))[det].any())
    per_part = [bool(inb[p].any()) for p in cs.parts]
    gap = float((srt[1] - srt[0])[inb].min()) if inb.any() and pb.shape[0] > 1 else np.inf
    return dict(moving=moving, parts=per_part, gap=gap)


@functools.lru_cache(maxsize=None)
def pr2_full():
    """PR2 at the fridge, N_PR2_FULL trajectories (the pr2 case's robot, X0 and fridge bases), 200 iterations, the door
    closing from 2.0 to 1.2 over the waypoints (shared; read-only) -> (scene, SQ, restatement's run)."""
    cs = case("pr2")
    n = N_PR2_FULL
    X0 = cs.X0[:n]
    SQ = cs.SQ[:, :n * cs.n_wp].copy()
    SQ[0] = np.tile(np.linspace(2.0, 1.2, cs.n_wp), n)
    sc = SR.AttachedScene(cs.sc.robot, cs.sc.scene_tree, cs.sc.scene_base, cs.sc.scene_ids).bind(X0, SQ)
    return sc, SQ, run_case(cs, 200, X0=X0, sc=sc)
