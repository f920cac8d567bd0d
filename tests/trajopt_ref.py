"""CPU restatement of kin_traj_opt_batch (include/kinhip.h; the kernel is k_traj, kinhip_traj_dev.h) in numpy,
and the reference's planning scene (test/test_planning.jl) it is exercised on.

Sphere centres and 3 x n Jacobians come from the oracle (OracleMech.fk_batch / fk_jac_batch); the box SDF and its
analytic gradient are written here to the conventions of the kernel's box_gradient (the oracle's coll_batch takes a
forward difference, ~1e-5 away, which would break iterate parity).  ChainScene is the same for any robot (the
random chains of tests/trajopt_cases.py).  Not a test module: imported by tests/test_trajopt.py and
tests/test_gpu_trajopt.py, which share the runs cached here."""
import functools

import numpy as np

import oracle as O
from conftest import ARM, golden

COLL_LINKS = ["wrist_flex_link", "torso_lift_link", "upperarm_roll_link", "elbow_flex_link"]  # test_planning.jl:17-20
BOX_POSE, BOX_WIDTH = (0.4, -0.25, 0.7), (0.05, 0.05, 0.5)
TARGET = (0.3, -0.4, 1.2)
# the parameters of the 32-goal runs
PARAMS = dict(margin=0.02, band=0.03, weight=10.0, max_step=0.5, ftol=1e-6, feas=1e-3, max_iters=200)
N_GOALS = 32


def _T(t):
    T = np.eye(4)
    T[:3, 3] = t
    return T


def union_box_sdf(p, poses, widths):
    """p [N, 3] -> (d [N], grad [N, 3]) of the union of boxes (pose 4x4, full widths): the first box of minimal
    distance; outside d = |max(q, 0)| with gradient sign(l) max(q, 0) / d, inside d = max(q) with the gradient on
    the first axis of maximal q (box_gradient, kinhip_coll_dev.h), rotated to the world."""
    p = np.asarray(p, np.float64)
    best = np.full(p.shape[0], np.inf)
    grad = np.zeros_like(p)
    for pose, width in zip(poses, widths):
        R, t = pose[:3, :3], pose[:3, 3]
        l = (p - t) @ R                       # R^T (p - t)
        q = np.abs(l) - 0.5 * np.asarray(width, np.float64)
        o = np.maximum(q, 0.0)
        mx = q.max(1)
        outside = mx > 0.0
        no = np.sqrt((o * o).sum(1))
        d = np.where(outside, no, mx)
        sgn = np.where(l < 0.0, -1.0, 1.0)
        g_out = sgn * o / np.where(outside, no, 1.0)[:, None]
        im = np.where((q[:, 0] >= q[:, 1]) & (q[:, 0] >= q[:, 2]), 0, np.where(q[:, 1] >= q[:, 2], 1, 2))
        g_in = np.zeros_like(p)
        g_in[np.arange(p.shape[0]), im] = sgn[np.arange(p.shape[0]), im]
        gl = np.where(outside[:, None], g_out, g_in)
        take = d < best                       # the first minimum wins
        best = np.where(take, d, best)
        grad = np.where(take[:, None], gl @ R.T, grad)
    return best, grad


class SceneBase:
    """What merit() and run() use of a scene: om, ids, sph, rad, lo, hi, n_dof, box_poses, box_widths."""

    def distances(self, Q):
        """Q [n_dof, N] -> sphere distances [n_sph, N] and the SDF gradients at the centres [n_sph, N, 3]."""
        N = Q.shape[1]
        poses = self.om.fk_batch(Q, self.ids, self.sph)          # [n_sph, 12, N]
        C = np.transpose(poses[:, 9:12, :], (0, 2, 1)).reshape(-1, 3)
        d, g = union_box_sdf(C, self.box_poses, self.box_widths)
        return d.reshape(len(self.sph), N) - self.rad[:, None], g.reshape(len(self.sph), N, 3)


class ChainScene(SceneBase):
    """Any robot: a UrdfTree, the batch joint ids in column order (off-chain joints allowed: their Jacobian columns
    are zero), held joints at fixed angles, (link id, centre, radius) spheres and a union of boxes (4x4 poses, full
    widths).  Unbounded joints and the base columns have +-inf limits, as the library's col_lo / col_hi."""

    def __init__(self, tree, with_base, ids, held=(), held_ang=(), spheres=(), box_poses=(), box_widths=()):
        self.with_base = bool(with_base)
        self.tree = tree
        self.om = O.OracleMech(tree, with_base=with_base)
        if len(held):
            self.om.set_joint_angles(list(held), np.concatenate([np.asarray(held_ang, np.float64),
                                                                 np.zeros(3 if with_base else 0)]))
        self.sph = [self.om.add_new_link(int(l), _T(c)) for l, c, _ in spheres]
        self.rad = np.array([r for _, _, r in spheres], np.float64)
        self.ids = [int(j) for j in ids]
        nb = 3 if with_base else 0
        self.n_dof = len(self.ids) + nb
        self.lo = np.array([tree.joint_lower[j - 1] for j in self.ids] + [-np.inf] * nb, np.float64)
        self.hi = np.array([tree.joint_upper[j - 1] for j in self.ids] + [np.inf] * nb, np.float64)
        self.box_poses = [np.asarray(p, np.float64) for p in box_poses]
        self.box_widths = [tuple(w) for w in box_widths]


class Scene(SceneBase):
    """Fetch, the four collision links' spheres and the thin box, on the oracle."""

    def __init__(self, with_base):
        import kinhip
        self.with_base = bool(with_base)
        self.tree = O.parse_urdf_tree(golden("fetch.urdf"))
        self.om = O.OracleMech(self.tree, with_base=with_base)
        self.sph, self.rad = [], []
        for n in COLL_LINKS:
            for c, r in kinhip.FETCH_LINK_SPHERES[n]:
                self.sph.append(self.om.add_new_link(self.tree.link_id(n), _T(c)))
                self.rad.append(r)
        self.rad = np.asarray(self.rad, np.float64)
        self.ids = [self.tree.joint_id(n) for n in ARM]
        self.n_dof = len(self.ids) + (3 if with_base else 0)
        self.lo = np.array([self.tree.joint_lower[j - 1] for j in self.ids] + [-np.inf] * (self.n_dof - len(self.ids)))
        self.hi = np.array([self.tree.joint_upper[j - 1] for j in self.ids] + [np.inf] * (self.n_dof - len(self.ids)))
        self.box_poses, self.box_widths = [_T(BOX_POSE)], [BOX_WIDTH]

    def goals(self):
        """q_start = 0 and the first 32 collision-free (min d > 0.05) IK solutions for TARGET from
        default_rng(0).uniform(-1, 1) starts."""
        N = 512
        q0 = np.random.default_rng(0).uniform(-1, 1, (self.n_dof, N))
        if self.with_base:
            q0[8:] = 0.0
        tg = np.repeat(_T(TARGET)[:3, :4].T.reshape(12, 1), N, axis=1)
        Q, it, _ = self.om.ik_dls_batch(q0, self.ids, self.tree.link_id("gripper_link"), tg, with_rot=False, max_iters=64)
        d, _ = self.distances(Q)
        ok = np.nonzero((it <= 64) & (d.min(0) > 0.05))[0]
        assert ok.size >= N_GOALS, ok.size
        return np.zeros(self.n_dof), np.ascontiguousarray(Q[:, ok[:N_GOALS]])


def straight_lines(q_start, goals, n_wp):
    """create_straight_trajectory per goal -> X [n_traj, n_wp, n_dof] (the last waypoint is the goal itself)."""
    goals = np.asarray(goals, np.float64)
    step = (goals.T - q_start[None, :]) / (n_wp - 1)
    X = q_start[None, None, :] + step[:, None, :] * np.arange(n_wp)[None, :, None]
    X[:, n_wp - 1] = goals.T
    return X


def to_columns(X):
    """[n_traj, n_wp, n_dof] -> the C-ABI's [n_dof, n_traj * n_wp]."""
    return np.ascontiguousarray(X.reshape(-1, X.shape[2]).T)


def from_columns(Q, n_wp):
    return np.ascontiguousarray(Q.T.reshape(-1, n_wp, Q.shape[0]))


def metric_inverse(n_wp):
    """(A_sub[I,I])^-1 as the kernel's table holds it (kin_traj_metric_inverse, checked against numpy's inverse in
    tests/test_trajopt.py).  cond(A_II) grows like n_wp^4 (~1e6 at 64), so two double-precision inverses differ by
    ~1e-10 relative: with numpy's own inverse here, iterate parity at n_wp = 64 would measure that difference
    (4.5e-8 in the trajectory after 8 iterations) instead of the kernel."""
    import kinhip
    return kinhip.traj_metric_inverse(n_wp)


def _sum(a, axis, rev):
    return np.flip(a, axis).sum(axis) if rev else a.sum(axis)


def merit(sc, X, margin, band, weight, W, rev=False):
    """X [nt, n_wp, nd] -> f [nt], smoothness [nt], min interior distance [nt], half-gradient g [nt, n_wp-2, nd]."""
    nt, n_wp, nd = X.shape
    Q = to_columns(X)
    d, gw = sc.distances(Q)                                    # [ns, N], [ns, N, 3]
    ns = d.shape[0]
    r = weight * np.maximum(0.0, (margin + band) - d)
    cf = weight * r
    gp = np.zeros((nd, Q.shape[1]))
    for s in (range(ns - 1, -1, -1) if rev else range(ns)):
        if not np.any(cf[s]):
            continue
        _, J = sc.om.fk_jac_batch(Q, sc.ids, sc.sph[s], sc.ids, with_rot=False)   # [nd, 3, N]
        gp -= cf[s][None, :] * np.einsum("dkn,nk->dn", J, gw[s])
    gp = from_columns(gp, n_wp)[:, 1:-1]                       # [nt, ni, nd]
    r = r.reshape(ns, nt, n_wp)[:, :, 1:-1]
    pen = _sum(np.transpose(r * r, (1, 2, 0)), 2, rev)         # [nt, ni]
    dmin = d.reshape(ns, nt, n_wp)[:, :, 1:-1].min(axis=(0, 2))
    a = (X[:, :-2] - 2.0 * X[:, 1:-1]) + X[:, 2:]              # [nt, ni, nd]
    ap = np.zeros((nt, n_wp + 2, nd))
    ap[:, 2:-2] = a                                            # ap[w + 1] = a_w, zero outside the interior
    ax = (ap[:, 1:-3] - 2.0 * ap[:, 2:-2]) + ap[:, 3:-1]       # (A x)_w, w interior
    smw = _sum(W[None, None, :] * a * a, 2, rev)               # [nt, ni]
    f = _sum(smw + pen, 1, rev)
    return f, _sum(smw, 1, rev), dmin, W[None, None, :] * ax + gp


def run(sc, X0, max_iters, margin, band, weight, feas, ftol, max_step, dof_weights=None, rev=False):
    """The algorithm of kin_traj_opt_batch on X0 [nt, n_wp, nd] -> dict(X, iters, info [4, nt], accepts [its, nt]
    (1 accepted, 0 rejected, -1 finished before), merits [its + 1, nt], candidates [its, nt] (the merit f' of
    each iteration's candidate), determined [nt]).
    determined[t]: every decision of trajectory t was clear of rounding -- |f' - f| > 1e-9 max(|f|, |f'|) + 1e-18
    (the merit is a sum of squared residuals, each pinned to the project's 1e-9) and,
    where a step was accepted, the done test 1e-9 away from both of its thresholds.  A trajectory that starts as
    a collision-free straight line has a merit of rounding noise (~1e-31): its accept / reject outcomes are not
    a property of the algorithm, so parity tests pin the decisions of the determined trajectories only."""
    X = np.array(X0, np.float64)
    nt, n_wp, nd = X.shape
    w = np.ones(nd) if dof_weights is None else np.asarray(dof_weights, np.float64)
    W, iW = w * w, 1.0 / (w * w)
    Minv = metric_inverse(n_wp)
    f, sm, dm, g = merit(sc, X, margin, band, weight, W, rev)
    alpha = np.ones(nt)
    fin = np.zeros(nt, bool)
    iters = np.full(nt, max_iters + 1, np.int32)
    nacc = np.zeros(nt)
    accepts, merits, cands = [], [f.copy()], []
    determined = np.ones(nt, bool)
    for it in range(1, max_iters + 1):
        if fin.all():
            break
        L = np.nonzero(~fin)[0]
        gL = g[L]
        s = np.einsum("wv,tvd->twd", Minv[:, ::-1], gL[:, ::-1]) if rev else np.einsum("wv,tvd->twd", Minv, gL)
        step = -(alpha[L, None, None] * (s * iW[None, None, :]))
        mx = np.abs(step).max(axis=(1, 2))
        scale = np.where(mx > max_step, max_step / np.where(mx > 0, mx, 1.0), 1.0)
        Xn = X[L].copy()
        Xn[:, 1:-1] = np.clip(X[L][:, 1:-1] + step * scale[:, None, None], sc.lo, sc.hi)
        fn, smn, dn, gn = merit(sc, Xn, margin, band, weight, W, rev)
        acc = fn <= f[L]
        done = acc & (f[L] - fn < ftol) & (dn >= margin - feas)
        scale_f = np.maximum(np.abs(fn), np.abs(f[L]))
        clear = np.abs(fn - f[L]) > 1e-9 * scale_f + 1e-18
        clear &= ~acc | ((np.abs((f[L] - fn) - ftol) > 1e-9 * np.maximum(scale_f, ftol))
                         & (np.abs(dn - (margin - feas)) > 1e-9))
        determined[L] &= clear
        rec = np.full(nt, -1)
        rec[L] = acc
        accepts.append(rec)
        cand = np.full(nt, np.nan)
        cand[L] = fn
        cands.append(cand)
        A, R = L[acc], L[~acc]
        X[A], g[A], f[A], sm[A], dm[A] = Xn[acc], gn[acc], fn[acc], smn[acc], dn[acc]
        nacc[A] += 1
        alpha[A] = np.minimum(1.0, 2.0 * alpha[A])
        alpha[R] *= 0.25
        fin[R[alpha[R] < 1e-6]] = True
        D = L[done]
        fin[D] = True
        iters[D] = it
        merits.append(f.copy())
    return dict(X=X, iters=iters, info=np.stack([f, sm, dm, nacc]), accepts=np.array(accepts).reshape(-1, nt),
                merits=np.array(merits), candidates=np.array(cands).reshape(-1, nt), determined=determined)


@functools.lru_cache(maxsize=None)
def scene(with_base):
    sc = Scene(with_base)
    sc.q_start, sc.q_goals = sc.goals()
    return sc


@functools.lru_cache(maxsize=None)
def full_run(n_wp, with_base=False):
    """200 iterations on the 32-goal set (shared by the CPU and the GPU tests; treat as read-only)."""
    sc = scene(with_base)
    X0 = straight_lines(sc.q_start, sc.q_goals, n_wp)
    out = run(sc, X0, **PARAMS)
    out["X0"] = X0
    _, _, out["d0"], _ = merit(sc, X0, PARAMS["margin"], PARAMS["band"], PARAMS["weight"], np.ones(sc.n_dof))
    return out
