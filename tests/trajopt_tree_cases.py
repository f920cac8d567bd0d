"""Cases for kin_traj_opt_tree_batch (k_traj_tree): robots whose collision spheres hang off several chains, shared by
tests/test_trajopt_tree.py (the cases and the restatement alone, on the CPU) and tests/test_gpu_traj_tree.py (the
kernel).  Not a test module; everything here is cached and must be treated as read-only.

Robots.
  twoarm       the two-arm robot below (a torso, two 4-joint arms), q = its 9 joints, 4 spheres per arm; without
               base at n_wp = 10 (L = 16), with base at n_wp = 5 (L = 8): two parts of bound 8.
  pr2          tests/golden/pr2_two_arms.urdf with the planar base, the torso held at 0.3, q = vcat(rarm, larm)
               (17 columns), kinhip.PR2_ARM_SPHERES, n_wp = 10, starts at PR2_MANIP_POSE: the reference's
               fridge_demo.jl shape, two parts of bound 8.
  tree0..3     seeded randtree.random_urdf trees (chain_bias 0.6) with spheres on 2, 3, 4, 4 root-to-leaf paths, each
               path its leaf sphere plus 1-3 more (on links of its own where it has any besides the leaf); the batch joints per path are chosen so that the parts' chain
               bounds are (16, 4), (12, 8, 4), (8, 8, 4, 4) and (8, 4, 4, 4); tree1 has one more batch column off
               every sphere path, tree3 the planar base and a sphere on the root link; n_wp = 20, 33, 64, 10
               (L = 32, 64, 64, 16).  The other moving joints of the paths are held at random non-zero angles.

Parts.  kin_coll_plan_create groups the spheres by chain: the spine is the remaining sphere anchor (the nearest link
below a batch joint) with the most batch joints above it, and takes every remaining sphere whose anchor is on its
root path.  sphere_parts() restates that on the CPU, so the cases know which sphere belongs to which part and the
bound each part is staged with; the GPU file asserts both through kin_plan_part_count / kin_plan_part_chain_bound.

Data per case: 9 trajectories, starts and goals inside the limits (+-pi where unbounded, base offsets +-0.5), X0 =
the straight lines plus a smooth seeded bump; 4 boxes (widths 0.05-0.2, the 2nd and 4th rotated), box k placed
around a sphere of part k mod n_parts of trajectory k at its middle waypoint (the centre 0.15-0.6 half-widths off
the box centre along every box axis, as tests/trajopt_cases.py); dof_weights = U(0.5, 2)^n_dof except None for
twoarm without base; the parameters KW of tests/trajopt_cases.py.  The seeds are the first (SEED0 + 100 k) at
which the restatement alone meets the conditions of tests/test_trajopt_tree.py::test_case_conditions."""
import functools
from dataclasses import dataclass

import numpy as np

import oracle as O
import trajopt_ref as R
from conftest import golden
from randtree import random_urdf
from trajopt_cases import KW, N_TRAJ, PAD, SENT, _path_joints, _rot_pose  # noqa: F401

TWO_ARM = """<robot name="twoarm">
  <link name="base_link"/><link name="torso"/>
  <link name="l1"/><link name="l2"/><link name="l3"/><link name="l4"/><link name="l_grip"/>
  <link name="r1"/><link name="r2"/><link name="r3"/><link name="r4"/><link name="r_grip"/>
  <joint name="torso_joint" type="prismatic"><parent link="base_link"/><child link="torso"/>
    <origin xyz="0 0 0.8"/><axis xyz="0 0 1"/><limit lower="0" upper="0.3" effort="1" velocity="1"/></joint>
  <joint name="l_j1" type="revolute"><parent link="torso"/><child link="l1"/><origin xyz="0.05 0.2 0.2"/>
    <axis xyz="0 0 1"/><limit lower="-2" upper="2" effort="1" velocity="1"/></joint>
  <joint name="l_j2" type="revolute"><parent link="l1"/><child link="l2"/><origin xyz="0.1 0 0"/>
    <axis xyz="0 1 0"/><limit lower="-1.5" upper="1.5" effort="1" velocity="1"/></joint>
  <joint name="l_j3" type="continuous"><parent link="l2"/><child link="l3"/><origin xyz="0.3 0 0"/>
    <axis xyz="1 0 0"/></joint>
  <joint name="l_j4" type="revolute"><parent link="l3"/><child link="l4"/><origin xyz="0.05 0 0"/>
    <axis xyz="0 1 0"/><limit lower="-2.2" upper="2.2" effort="1" velocity="1"/></joint>
  <joint name="l_tool" type="fixed"><parent link="l4"/><child link="l_grip"/><origin xyz="0.3 0 0"/></joint>
  <joint name="r_j1" type="revolute"><parent link="torso"/><child link="r1"/><origin xyz="0.05 -0.2 0.2"/>
    <axis xyz="0 0 1"/><limit lower="-2" upper="2" effort="1" velocity="1"/></joint>
  <joint name="r_j2" type="revolute"><parent link="r1"/><child link="r2"/><origin xyz="0.1 0 0"/>
    <axis xyz="0 1 0"/><limit lower="-1.5" upper="1.5" effort="1" velocity="1"/></joint>
  <joint name="r_j3" type="continuous"><parent link="r2"/><child link="r3"/><origin xyz="0.3 0 0"/>
    <axis xyz="1 0 0"/></joint>
  <joint name="r_j4" type="revolute"><parent link="r3"/><child link="r4"/><origin xyz="0.05 0 0"/>
    <axis xyz="0 1 0"/><limit lower="-2.2" upper="2.2" effort="1" velocity="1"/></joint>
  <joint name="r_tool" type="fixed"><parent link="r4"/><child link="r_grip"/><origin xyz="0.3 0 0"/></joint>
</robot>
"""
TWO_ARM_Q = ["r_j1", "r_j2", "r_j3", "r_j4", "torso_joint", "l_j1", "l_j2", "l_j3", "l_j4"]
TWO_ARM_SPHERES = [(side + n, c, r) for side in ("l", "r") for n, c, r in
                   (("2", (0.1, 0, 0), 0.05), ("2", (0.22, 0, 0), 0.05), ("4", (0.1, 0, 0), 0.045),
                    ("4", (0.25, 0, 0), 0.04))]

# random trees: batch joints wanted on each sphere path (the parts' chain bounds follow), n_wp, base + root sphere,
# an off-chain column
TREES = [dict(counts=(14, 3), n_wp=20, base=False, off=False),
         dict(counts=(10, 6, 3), n_wp=33, base=False, off=True),
         dict(counts=(7, 5, 3, 2), n_wp=64, base=False, off=False),
         dict(counts=(6, 4, 3, 2), n_wp=10, base=True, off=False)]
CASES = ["twoarm-nobase", "twoarm-base", "pr2", "tree0", "tree1", "tree2", "tree3"]
TREE_SEED, SEED0 = 6100, 7100
# the first data seed offset (SEED0 + 100 k) that meets test_case_conditions, found on the CPU with the restatement
SEED_K = {"twoarm-nobase": 0, "twoarm-base": 0, "pr2": 0, "tree0": 0, "tree1": 0, "tree2": 0, "tree3": 0}
NO_WEIGHTS = "twoarm-nobase"
MIXED_BOUNDS = "tree0"       # parts of bound 16 and 4 in one plan
WP64 = "tree2"
N_PR2_FULL = 6               # trajectories of the PR2 full run (200 iterations)


def chain_bound(n):
    """pick_chain_bound (kinhip_internal.h)."""
    return 4 if n <= 4 else 8 if n <= 8 else 12 if n <= 12 else 16 if n <= 16 else 32


def sphere_parts(tree, q_ids, sphere_links):
    """kin_coll_plan_create's grouping -> (parts: lists of sphere indices in plan order, their chain bounds)."""
    pj = {int(c): k + 1 for k, c in enumerate(tree.joint_clink)}        # link -> parent joint
    batch = {int(j) for j in q_ids if tree.joint_type[int(j) - 1] != O.FIXED}

    def plink(x):
        return int(tree.joint_plink[pj[x] - 1]) if x in pj else 0

    def anchor_of(x):
        while x in pj and pj[x] not in batch:
            x = plink(x)
        return x

    anchor = [anchor_of(int(l)) for l in sphere_links]
    depth = []
    for a in anchor:
        d, y = 0, a
        while y in pj:
            d += pj[y] in batch
            y = plink(y)
        depth.append(d)
    done, parts, bounds = [False] * len(anchor), [], []
    while not all(done):
        best, spine = -1, None
        for k in range(len(anchor)):
            if not done[k] and depth[k] > best:
                best, spine = depth[k], anchor[k]
        on_path, y = set(), spine
        while True:
            on_path.add(y)
            if y not in pj:
                break
            y = plink(y)
        grp = [k for k in range(len(anchor)) if not done[k] and anchor[k] in on_path]
        for k in grp:
            done[k] = True
        parts.append(grp)
        bounds.append(chain_bound(best))
    return parts, bounds


@dataclass
class Robot:
    name: str
    text: str            # URDF text (None: path)
    path: str            # URDF file (None: text)
    tree: object
    q_ids: list          # batch columns (joint ids)
    held: list
    held_ang: np.ndarray
    spheres: list        # (link id, centre [3], radius)
    off_cols: np.ndarray
    start: object        # [n_q] fixed start of every trajectory, or None (random)


@functools.lru_cache(maxsize=None)
def robot(name) -> Robot:
    if name == "twoarm":
        t, p = O.parse_urdf_tree(TWO_ARM), None
        sph = [(t.link_id(n), np.array(c, np.float64), float(r)) for n, c, r in TWO_ARM_SPHERES]
        return Robot(name, TWO_ARM, p, t, [t.joint_id(n) for n in TWO_ARM_Q], [], np.zeros(0), sph, np.zeros(0, int),
                     None)
    if name == "pr2":
        import kinhip
        p = golden("pr2_two_arms.urdf")
        t = O.parse_urdf_tree(p)
        sph = [(t.link_id(n), np.array(c, np.float64), float(r)) for n, c, r in kinhip.PR2_ARM_SPHERES]
        r, l, torso = kinhip.PR2_MANIP_POSE
        return Robot(name, None, p, t, [t.joint_id(n) for n in kinhip.PR2_RARM_JOINTS + kinhip.PR2_LARM_JOINTS],
                     [t.joint_id("torso_lift_joint")], np.array([torso]), sph, np.zeros(0, int),
                     np.deg2rad(np.array(r + l)))
    i = int(name[4:])
    return _random_tree(i)


def _random_tree(i) -> Robot:
    spec = TREES[i]
    counts = spec["counts"]
    rng = np.random.default_rng(TREE_SEED + i)
    for _ in range(4000):
        text = random_urdf(rng, int(rng.integers(30, 56)), chain_bias=0.6, box_p=0)
        t = O.parse_urdf_tree(text)
        nl = len(t.link_names)
        children = set(int(p) for p in t.joint_plink)
        leaves = [l for l in range(1, nl + 1) if l not in children]
        moving = lambda l: [j for j in _path_joints(t, l) if t.joint_type[j - 1] != O.FIXED]
        leaves.sort(key=lambda l: -len(moving(l)))
        # one leaf per wanted count, deepest first; batch joints chosen path after path: a joint decided on an earlier
        # path (batch or held) keeps its role on the later ones
        chosen, role, ok = [], {}, True
        pool = list(leaves)
        for n in counts:
            pick = None
            for l in pool:
                mv = moving(l)
                have = sum(role.get(j) == "b" for j in mv)
                free = [j for j in mv if j not in role]
                # the leaf's own parent joint is a batch joint, so that the leaf sphere is the part's deepest anchor
                if have <= n and len(free) >= n - have and (n - have >= 1) and mv and mv[-1] in free \
                        and int(t.joint_clink[mv[-1] - 1]) == l:
                    pick = (l, mv, have, free)
                    break
            if pick is None:
                ok = False
                break
            l, mv, have, free = pick
            pool.remove(l)
            take = [mv[-1]] + [int(j) for j in rng.choice([j for j in free if j != mv[-1]], n - have - 1, replace=False)]
            for j in mv:
                if j not in role:
                    role[j] = "b" if j in take else "h"
            chosen.append(l)
        if not ok:
            continue
        batch = [j for j, r in role.items() if r == "b"]
        held = [j for j, r in role.items() if r == "h"]
        off = []
        if spec["off"]:
            om = O.OracleMech(t)
            off = [j for j in range(1, len(t.joint_names) + 1) if t.joint_type[j - 1] != O.FIXED
                   and not any(om.is_relevant(j, l) for l in chosen)]
            if not off:
                continue
        if len(batch) + bool(off) + (3 if spec["base"] else 0) > 20:
            continue
        batch = [int(j) for j in rng.permutation(batch)]
        if off:
            batch.insert(int(rng.integers(0, len(batch) + 1)), int(rng.choice(off)))
        spheres, taken = [], set()
        for l in chosen:      # the path's own links (not on an earlier path) where it has any besides the leaf
            path_links = [int(t.joint_clink[j - 1]) for j in _path_joints(t, l)]
            links = [x for x in path_links[:-1] if x not in taken] or path_links[:-1]
            taken.update(path_links)
            more = [int(x) for x in rng.choice(links, min(int(rng.integers(1, 4)), len(links)), replace=False)] \
                if links else []
            spheres += [(x, rng.uniform(-0.1, 0.1, 3), float(rng.uniform(0.03, 0.08))) for x in [l] + sorted(more)]
        if spec["base"]:
            root = int(t.joint_plink[_path_joints(t, chosen[0])[0] - 1])
            spheres.append((root, rng.uniform(-0.1, 0.1, 3), float(rng.uniform(0.03, 0.08))))
        parts, bounds = sphere_parts(t, batch, [s[0] for s in spheres])
        if tuple(bounds) != tuple(chain_bound(n) for n in counts):
            continue
        held_ang = rng.uniform(0.2, 1.0, len(held)) * rng.choice([-1.0, 1.0], len(held))
        off_cols = np.array([k for k, j in enumerate(batch) if j in off], int)
        return Robot(f"tree{i}", text, None, t, batch, held, held_ang, spheres, off_cols, None)
    raise AssertionError(f"no tree for {spec}")


@dataclass
class Case:
    name: str
    rb: Robot
    with_base: bool
    n_wp: int
    parts: list          # sphere indices per part, plan order
    bounds: list         # chain bound per part
    sc: object           # trajopt_ref.ChainScene (all spheres)
    X0: np.ndarray       # [N_TRAJ, n_wp, n_dof]
    dof_weights: object
    off_cols: np.ndarray
    box_parts: list      # the part box k was placed on

    @property
    def n_dof(self):
        return self.sc.n_dof

    @property
    def spheres(self):
        return self.rb.spheres


def _shape(name):
    if name == "twoarm-nobase":
        return "twoarm", False, 10
    if name == "twoarm-base":
        return "twoarm", True, 5
    if name == "pr2":
        return "pr2", True, 10
    sp = TREES[int(name[4:])]
    return name, sp["base"], sp["n_wp"]


def build(name, seed) -> Case:
    rname, with_base, n_wp = _shape(name)
    rb = robot(rname)
    rng = np.random.default_rng(seed)
    sc = R.ChainScene(rb.tree, with_base, rb.q_ids, rb.held, rb.held_ang, rb.spheres)
    parts, bounds = sphere_parts(rb.tree, rb.q_ids, [s[0] for s in rb.spheres])
    nd, nc = sc.n_dof, len(rb.q_ids)
    bounded = np.isfinite(sc.lo) & np.isfinite(sc.hi)
    flo, fhi = np.where(bounded, sc.lo, -np.pi), np.where(bounded, sc.hi, np.pi)
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

    starts, goals = draw(N_TRAJ, True), draw(N_TRAJ)
    bump = np.sin(np.pi * np.arange(n_wp) / (n_wp - 1))[None, :, None] * rng.normal(0, 0.05, (N_TRAJ, 1, nd))
    bump[:, :, off_cols] = 0.0
    widths = [tuple(rng.uniform(0.05, 0.2, 3)) for _ in range(4)]
    rpys = [np.zeros(3) if k % 2 == 0 else rng.uniform(-1.0, 1.0, 3) for k in range(4)]
    box_parts = [k % len(parts) for k in range(4)]
    which = [int(rng.choice(parts[p])) for p in box_parts]
    offs = [rng.uniform(0.15, 0.6, 3) * rng.choice([-1.0, 1.0], 3) * 0.5 * np.array(widths[k]) for k in range(4)]
    mid = n_wp // 2
    band = KW["margin"] + KW["band"]
    for _ in range(40):
        X0 = np.stack([R.straight_lines(starts[:, t], goals[:, t:t + 1], n_wp)[0] for t in range(N_TRAJ)])
        X0[:, 1:-1] = np.clip(X0[:, 1:-1] + bump[:, 1:-1], sc.lo, sc.hi)
        sc.box_poses, sc.box_widths = [], []
        poses = sc.om.fk_batch(np.ascontiguousarray(X0[:4, mid].T), sc.ids, sc.sph)   # [n_sph, 12, 4]
        for k in range(4):
            Rk = O.rpy_to_matrix(rpys[k])
            sc.box_poses.append(_rot_pose(rpys[k], poses[which[k], 9:12, k] - Rk @ offs[k]))
            sc.box_widths.append(widths[k])
        d0, _ = sc.distances(np.ascontiguousarray(X0[:, 0].T))
        d1, _ = sc.distances(np.ascontiguousarray(X0[:, -1].T))
        bad0, bad1 = d0.min(0) < band, d1.min(0) < band
        if not (bad0.any() or bad1.any()) or (rb.start is not None and not bad1.any()):
            break
        if rb.start is None:
            starts[:, bad0] = draw(int(bad0.sum()))
        goals[:, bad1] = draw(int(bad1.sum()))
    w = None if name == NO_WEIGHTS else rng.uniform(0.5, 2.0, nd)
    return Case(name, rb, bool(with_base), n_wp, parts, bounds, sc, X0, w, off_cols, box_parts)


def seed_of(name, k=None):
    return SEED0 + 10 * CASES.index(name) + 100 * (SEED_K[name] if k is None else k)


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    return build(name, seed_of(name))


def run_case(cs, max_iters, rev=False, weights=True, spheres=None, X0=None):
    """trajopt_ref.run on the case; spheres: indices of the spheres that count (None: all)."""
    sc = cs.sc
    if spheres is not None:
        sc = sub_scene(cs, tuple(spheres))
    return R.run(sc, cs.X0 if X0 is None else X0, max_iters=max_iters, dof_weights=cs.dof_weights if weights else None,
                 rev=rev, **KW)


@functools.lru_cache(maxsize=None)
def _sub_scene(name, spheres):
    cs = case(name)
    sc = R.ChainScene(cs.rb.tree, cs.with_base, cs.rb.q_ids, cs.rb.held, cs.rb.held_ang,
                      [cs.rb.spheres[k] for k in spheres], cs.sc.box_poses, cs.sc.box_widths)
    return sc


def sub_scene(cs, spheres):
    """The case's robot, boxes and limits with only the given spheres (one part: a single-chain plan)."""
    return _sub_scene(cs.name, tuple(int(k) for k in spheres))


@functools.lru_cache(maxsize=None)
def ref_run(name, max_iters, rev=False, weights=True, spheres=None):
    return run_case(case(name), max_iters, rev, weights, spheres)


def inside_band(cs, X0=None):
    """[n_parts, n_traj]: part p has a sphere closer than margin + band at an interior waypoint of X0."""
    X0 = cs.X0 if X0 is None else X0
    nt, n_wp, _ = X0.shape
    d, _ = cs.sc.distances(R.to_columns(X0))
    d = d.reshape(len(cs.spheres), nt, n_wp)[:, :, 1:-1].min(2)
    return np.array([d[p].min(0) < KW["margin"] + KW["band"] for p in cs.parts])


@functools.lru_cache(maxsize=None)
def pr2_full():
    """200 iterations on the first N_PR2_FULL trajectories of the pr2 case (shared; read-only)."""
    cs = case("pr2")
    return run_case(cs, 200, X0=cs.X0[:N_PR2_FULL])
