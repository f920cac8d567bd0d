"""Seeded random-chain cases for kin_traj_opt_batch (k_traj), shared by tests/test_trajopt_random_chains.py (the
cases and the restatement alone, on the CPU) and tests/test_gpu_traj_random_chains.py (the kernel).  Not a test
module; everything here is cached and must be treated as read-only.

Chains.  randtree.random_urdf(..., box_p=0) robots as in tests/test_gpu_ik_random_chains.py: the path is the
root-to-leaf path with the most moving joints; the batch joints are a random subset of its moving joints in random
column order, the other path joints are held at random non-zero angles.  The number of batch joints on the path is
2, 4, 5, 8, 9, 12, 13, 16: both ends of the four chain bounds k_traj is compiled for.  A collision plan's chain
ends at the link under the deepest moving joint that carries a sphere, so every chain has one sphere on the leaf
(all the batch joints of the path are then steps) and 2 to 5 more on other links of the path: one sphere group.
The lower end of every bound is a tree (chain_bias 0.9) with one more batch column, a moving joint off the path.
Each chain runs without and with the planar base (with it: one more sphere on the root link, whose gradient has
base columns only): 16 cases, plus the bound-16 chain with base at n_wp = 64 ("wide": 19 q columns, so the fp64
workgroup is halved to fit LDS).

Data per case: 9 trajectories; n_wp cycles through 5, 10, 20, 33 within every bound (L = 8, 16, 32, 64); starts
and goals inside the limits (+-pi where unbounded, base offsets +-0.5); X0 = the straight lines plus a smooth
seeded bump; 4 boxes (widths 0.05-0.2, the 2nd and 4th rotated), box k placed around a sphere of trajectory k at
its middle waypoint (the sphere centre 0.15-0.6 half-widths off the box centre along every box axis: exactly at
the centre the sign of the SDF gradient is decided by rounding); end waypoints closer than margin + band to a box
are redrawn (Case.ends_feasible records whether that succeeded; the kernel does not require it).  The 8-joint
chain without base has 66 more boxes scattered in a 3 m cube (70 > kCollLdsBoxes: the union is read from global
memory).  dof_weights = U(0.5, 2)^n_dof, except None for the 2-joint chain without base."""
import functools
from dataclasses import dataclass

import numpy as np

import oracle as O
import trajopt_ref as R
from randtree import random_urdf

STEPS = (2, 4, 5, 8, 9, 12, 13, 16)            # batch joints on the path of chain i
BOUND = (4, 4, 8, 8, 12, 12, 16, 16)
N_WPS = (5, 10, 20, 33)
N_TRAJ = 9
PAD = 7                                        # ldx = N_TRAJ * n_wp + PAD
SENT = -7.25                                   # padding columns and the row past n_dof (exact in fp32)
CHAIN_SEED, DATA_SEED = 4100, 5100
KW = {k: v for k, v in R.PARAMS.items() if k != "max_iters"}
CASES = [(i, b) for i in range(len(STEPS)) for b in (False, True)] + [(7, True, 64)]
MANY_BOXES = (3, False)                        # 70 boxes
NO_WEIGHTS = (0, False)                        # dof_weights = None
WIDE = (7, True, 64)


def cid(c):
    return f"chain{c[0]}-{'base' if c[1] else 'nobase'}" + ("-wide" if len(c) == 3 else "")


def is_tree(i):
    return i % 2 == 0


@dataclass
class Chain:
    idx: int
    text: str
    tree: object
    leaf: int
    path: list         # moving joints root -> leaf
    q_ids: list        # batch columns (joint ids), the off-path one included
    on: np.ndarray     # per column: on the path
    held: list
    held_ang: np.ndarray
    spheres: list      # (link id, centre [3], radius), on links of the path
    root: int          # the root link of the path


def _path_joints(t, link):
    pj = {int(c): k + 1 for k, c in enumerate(t.joint_clink)}
    out = []
    while link in pj:
        j = pj[link]
        out.append(j)
        link = int(t.joint_plink[j - 1])
    return out[::-1]


@functools.lru_cache(maxsize=None)
def chain(i) -> Chain:
    nb = STEPS[i]
    rng = np.random.default_rng(CHAIN_SEED + i)
    tree_case = is_tree(i)
    for _ in range(500):
        if tree_case:
            text = random_urdf(rng, int(2.2 * nb) + 12, chain_bias=0.9, box_p=0)
        else:
            text = random_urdf(rng, int(1.25 * (nb + 1)) + 4, chain_bias=1.0, box_p=0)
        t = O.parse_urdf_tree(text)
        children = set(int(p) for p in t.joint_plink)
        leaves = [l for l in range(1, len(t.link_names) + 1) if l not in children]
        moving_on = lambda l: [j for j in _path_joints(t, l) if t.joint_type[j - 1] != O.FIXED]
        leaf = max(leaves, key=lambda l: len(moving_on(l)))
        path = moving_on(leaf)
        om = O.OracleMech(t)
        off = [j for j in range(1, len(t.joint_names) + 1)
               if t.joint_type[j - 1] != O.FIXED and not om.is_relevant(j, leaf)]
        if len(path) >= nb + 1 and (off or not tree_case):
            break
    else:
        raise AssertionError(f"no chain with {nb} batch joints for chain {i}")
    batch = [int(j) for j in rng.permutation(rng.choice(path, nb, replace=False))]
    held = [j for j in path if j not in batch]
    held_ang = rng.uniform(0.2, 1.0, len(held)) * rng.choice([-1.0, 1.0], len(held))
    if tree_case:
        batch.insert(int(rng.integers(0, nb + 1)), int(rng.choice(off)))
    on = np.array([j in path for j in batch])
    all_path = _path_joints(t, leaf)
    links = [int(t.joint_clink[j - 1]) for j in all_path]          # the path's links below the root
    n_more = int(rng.integers(2, 6))
    more = [int(l) for l in rng.choice(links[:-1], min(n_more, len(links) - 1), replace=False)]
    spheres = [(l, rng.uniform(-0.1, 0.1, 3), float(rng.uniform(0.03, 0.08))) for l in [leaf] + sorted(more)]
    return Chain(i, text, t, int(leaf), path, batch, on, held, held_ang, spheres, int(t.joint_plink[all_path[0] - 1]))


@dataclass
class Case:
    key: tuple
    ch: Chain
    with_base: bool
    n_wp: int
    bound: int
    spheres: list
    sc: object           # trajopt_ref.ChainScene
    X0: np.ndarray       # [N_TRAJ, n_wp, n_dof]
    dof_weights: object  # [n_dof] or None
    off_cols: np.ndarray
    ends_feasible: bool

    @property
    def n_dof(self):
        return self.sc.n_dof


def _rot_pose(rpy, t):
    T = np.eye(4)
    T[:3, :3] = O.rpy_to_matrix(rpy)
    T[:3, 3] = t
    return T


@functools.lru_cache(maxsize=None)
def case(key) -> Case:
    i, with_base = key[0], key[1]
    ch = chain(i)
    pos = 2 * (i % 2) + int(with_base)                       # 0..3 within the bound
    n_wp = key[2] if len(key) == 3 else N_WPS[pos]
    rng = np.random.default_rng(DATA_SEED + 10 * i + int(with_base) + (5 if len(key) == 3 else 0))
    spheres = list(ch.spheres)
    if with_base:
        spheres.append((ch.root, rng.uniform(-0.1, 0.1, 3), float(rng.uniform(0.03, 0.08))))
    sc = R.ChainScene(ch.tree, with_base, ch.q_ids, ch.held, ch.held_ang, spheres)
    nd, nc = sc.n_dof, len(ch.q_ids)
    bounded = np.isfinite(sc.lo) & np.isfinite(sc.hi)
    flo, fhi = np.where(bounded, sc.lo, -np.pi), np.where(bounded, sc.hi, np.pi)
    flo[nc:], fhi[nc:] = -0.5, 0.5
    off_cols = np.flatnonzero(~ch.on)
    off_val = flo[off_cols] + (fhi[off_cols] - flo[off_cols]) * rng.uniform(0.3, 0.7, off_cols.size)

    def draw(n):
        q = flo[:, None] + (fhi - flo)[:, None] * rng.random((nd, n))
        q[off_cols] = off_val[:, None]
        return q

    starts, goals = draw(N_TRAJ), draw(N_TRAJ)
    bump = np.sin(np.pi * np.arange(n_wp) / (n_wp - 1))[None, :, None] * rng.normal(0, 0.05, (N_TRAJ, 1, nd))
    bump[:, :, off_cols] = 0.0
    widths = [tuple(rng.uniform(0.05, 0.2, 3)) for _ in range(4)]
    rpys = [np.zeros(3) if k % 2 == 0 else rng.uniform(-1.0, 1.0, 3) for k in range(4)]
    which = rng.integers(0, len(spheres), 4)
    # the sphere sits inside its box, 0.15-0.6 half-widths off the centre along every box axis: at the centre
    # itself (and on the box's mid-planes) the sign of the SDF gradient is a matter of rounding
    offs = [rng.uniform(0.15, 0.6, 3) * rng.choice([-1.0, 1.0], 3) * 0.5 * np.array(widths[k]) for k in range(4)]
    extra_p, extra_w = [], []
    if key == MANY_BOXES:
        extra_p = [_rot_pose(rng.uniform(-1, 1, 3) * (k % 2), rng.uniform(-1.5, 1.5, 3)) for k in range(66)]
        extra_w = [tuple(rng.uniform(0.05, 0.2, 3)) for _ in range(66)]
    mid = n_wp // 2
    band = KW["margin"] + KW["band"]
    ends_ok = False
    for _ in range(40):
        X0 = np.stack([R.straight_lines(starts[:, t], goals[:, t:t + 1], n_wp)[0] for t in range(N_TRAJ)])
        X0[:, 1:-1] = np.clip(X0[:, 1:-1] + bump[:, 1:-1], sc.lo, sc.hi)
        sc.box_poses, sc.box_widths = [], []
        poses = sc.om.fk_batch(np.ascontiguousarray(X0[:4, mid].T), sc.ids, sc.sph)   # [n_sph, 12, 4]
        for k in range(4):
            Rk = O.rpy_to_matrix(rpys[k])
            sc.box_poses.append(_rot_pose(rpys[k], poses[which[k], 9:12, k] - Rk @ offs[k]))
            sc.box_widths.append(widths[k])
        sc.box_poses += extra_p
        sc.box_widths += extra_w
        d0, _ = sc.distances(np.ascontiguousarray(X0[:, 0].T))
        d1, _ = sc.distances(np.ascontiguousarray(X0[:, -1].T))
        bad0, bad1 = d0.min(0) < band, d1.min(0) < band
        if not (bad0.any() or bad1.any()):
            ends_ok = True
            break
        starts[:, bad0] = draw(int(bad0.sum()))
        goals[:, bad1] = draw(int(bad1.sum()))
    w = None if key == NO_WEIGHTS else rng.uniform(0.5, 2.0, nd)
    return Case(key, ch, bool(with_base), n_wp, BOUND[i], spheres, sc, X0, w, off_cols, ends_ok)


@functools.lru_cache(maxsize=None)
def ref_run(key, max_iters, rev=False, weights=True):
    """trajopt_ref.run on the case (weights=False: dof_weights = None whatever the case holds)."""
    cs = case(key)
    return R.run(cs.sc, cs.X0, max_iters=max_iters, dof_weights=cs.dof_weights if weights else None, rev=rev, **KW)
