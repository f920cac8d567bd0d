"""CPU restatement of kin_traj_opt_pose_batch (include/kinhip.h; the kernel is k_traj's POSE variant,
kinhip_traj_dev.h) in numpy: trajopt_ref's algorithm plus one pose constraint per trajectory -- link `link` held at a
per-trajectory target at interior waypoint c, 3 rows (position) or 6 (position + orientation).  Reuses
trajopt_ref.merit / Scene / ChainScene; pose and geometric Jacobian come from the oracle (fk_jac_batch with
with_rot=True, rpy_jac=False).  Not a test module: imported by tests/test_trajopt_pose.py and
tests/test_gpu_trajopt_pose.py, which share the runs cached here (treat them as read-only).

    r      = [p(x_c) - p*; -log(R* R(x_c)^T)]                 (derivative: the geometric Jacobian J)
    f      = smoothness + sphere penalties + nu (|r_p| + |r_rot|)
    raw    = -alpha W^-1 Minv g,   m = Minv[:, c-1],   S = J W^-1 J^T + mu I
    v      = S^-1 (-r - J raw_c),  u = W^-1 J^T v
    step_w = raw_w + (m[w-1] / m[c-1]) u
then the scaling to max_step, the clamp and the accept / reject rule of trajopt_ref.run on f; done additionally
needs |r_p| < tol_pos and |r_rot| < tol_rot."""
import functools

import numpy as np

import trajopt_ref as R

POSE_WEIGHT, DAMP, TOL = 10.0, 1e-6, 1e-3
SHIFT, YAW = (-0.05, 0.0, 0.10), 0.3          # the target family: the straight line's pose at c, moved
CASES = [(10, 3), (10, 6), (33, 6)]            # (n_wp, rows) of the full runs, c = n_wp // 2


def rot_log(Rt, Rn):
    """[N, 3, 3] x 2 -> w [N, 3] with exp([w]) Rn = Rt (log of Rt Rn^T), by the formula of the kernels' rot_error
    (kinhip_ik_dev.h): w = v th / s, v the vector of the skew part, s = |v|, c = (tr - 1) / 2, th = atan2(s, c)."""
    E = np.einsum("nab,ncb->nac", Rt, Rn)
    v = 0.5 * np.stack([E[:, 2, 1] - E[:, 1, 2], E[:, 0, 2] - E[:, 2, 0], E[:, 1, 0] - E[:, 0, 1]], 1)
    s = np.sqrt((v * v).sum(1))
    c = 0.5 * (E[:, 0, 0] + E[:, 1, 1] + E[:, 2, 2] - 1.0)
    th = np.arctan2(s, c)
    tiny = ~(s > 1e-7)
    w = v * np.where(tiny, 1.0, th / np.where(tiny, 1.0, s))[:, None]
    for n in np.nonzero(tiny & ~(c > 0.0))[0]:          # a rotation by ~pi: the axis from the symmetric part
        d = np.diag(E[n])
        b = 0
        if d[1] > d[0]:
            b = 1
        if d[2] > d[b]:
            b = 2
        a = 0.25 * (E[n, :, b] + E[n, b, :])
        a[b] = 0.5 * (d[b] + 1.0)
        w[n] = a / np.sqrt((a * a).sum()) * th[n]
    return w


def mat_of(pose12):
    """[12, N] 3x4 column-major -> R [N, 3, 3], p [N, 3]."""
    return np.transpose(pose12[:9].T.reshape(-1, 3, 3), (0, 2, 1)), pose12[9:12].T


def pose12_of(Rm, p):
    """R [N, 3, 3], p [N, 3] -> [12, N] 3x4 column-major."""
    return np.ascontiguousarray(np.concatenate([np.transpose(Rm, (0, 2, 1)).reshape(-1, 9), p], 1).T)


def residual(sc, link, Q, targets, with_rot):
    """Q [nd, N], targets [12, N] -> r [N, k] (k = 6 or 3), J [N, k, nd]."""
    pose, J = sc.om.fk_jac_batch(np.ascontiguousarray(Q), sc.ids, link, sc.ids, with_rot=True, rpy_jac=False)
    Rn, p = mat_of(pose)
    Rt, pt = mat_of(np.asarray(targets, np.float64))
    J = np.transpose(J, (2, 1, 0))                                 # [N, 6, nd]
    if not with_rot:
        return p - pt, np.ascontiguousarray(J[:, :3])
    return np.concatenate([p - pt, -rot_log(Rt, Rn)], 1), np.ascontiguousarray(J)


def norms(r):
    """r [N, k] -> |r_p| [N], |r_rot| [N] (0 for position-only)."""
    rp = np.sqrt((r[:, :3] * r[:, :3]).sum(1))
    rr = np.sqrt((r[:, 3:] * r[:, 3:]).sum(1)) if r.shape[1] == 6 else np.zeros(r.shape[0])
    return rp, rr


def chol_solve(S, b):
    """S [N, k, k] symmetric positive definite, b [N, k] -> S^-1 b by an unpivoted Cholesky factorisation, in the
    kernel's order (column by column; a failed factorisation gives NaN, as there)."""
    N, k, _ = S.shape
    L = np.zeros_like(S)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(k):
            d = S[:, j, j].copy()
            for p in range(j):
                d -= L[:, j, p] * L[:, j, p]
            L[:, j, j] = np.sqrt(d)
            for i in range(j + 1, k):
                a = S[:, i, j].copy()
                for p in range(j):
                    a -= L[:, i, p] * L[:, j, p]
                L[:, i, j] = a / L[:, j, j]
        y = np.zeros_like(b)
        for i in range(k):
            a = b[:, i].copy()
            for p in range(i):
                a -= L[:, i, p] * y[:, p]
            y[:, i] = a / L[:, i, i]
        x = np.zeros_like(b)
        for i in range(k - 1, -1, -1):
            a = y[:, i].copy()
            for p in range(i + 1, k):
                a -= L[:, p, i] * x[:, p]
            x[:, i] = a / L[:, i, i]
    return x


def merit(sc, link, c, with_rot, targets, X, margin, band, weight, W, nu, rev=False):
    """trajopt_ref.merit plus the pose term -> f, smoothness, dmin, g (without the pose term: the projection
    annihilates it), |r_p|, |r_rot|, r [nt, k], J [nt, k, nd] at waypoint c."""
    f0, sm, dm, g = R.merit(sc, X, margin, band, weight, W, rev)
    r, J = residual(sc, link, X[:, c].T, targets, with_rot)
    rp, rr = norms(r)
    return f0 + nu * (rp + rr), sm, dm, g, rp, rr, r, J


def projected_step(raw, Minv, c, r, J, iW, damp, rev=False):
    """raw [nt, ni, nd] -> the step of the module docstring [nt, ni, nd] (before the scaling and the clamp); rev: the
    sums over the q columns and over the rows taken in reverse order."""
    k = r.shape[1]
    m = Minv[:, c - 1]
    if rev:
        out = projected_step(raw[:, :, ::-1], Minv, c, r[:, ::-1], J[:, ::-1, ::-1], iW[::-1], damp)
        return out[:, :, ::-1]
    S = np.einsum("tkd,d,tld->tkl", J, iW, J) + damp * np.eye(k)[None]
    v = chol_solve(S, -r - np.einsum("tkd,td->tk", J, raw[:, c - 1]))
    u = iW[None, :] * np.einsum("tkd,tk->td", J, v)
    return raw + (m / m[c - 1])[None, :, None] * u[:, None, :]


def run(sc, link, c, with_rot, targets, X0, max_iters, margin, band, weight, feas, ftol, max_step, dof_weights=None,
        pose_weight=POSE_WEIGHT, damp=DAMP, tol_pos=TOL, tol_rot=TOL, rev=False):
    """The algorithm of kin_traj_opt_pose_batch on X0 [nt, n_wp, nd], targets [12, nt] -> dict(X, iters,
    info [6, nt], accepts, merits, candidates, determined) as trajopt_ref.run; determined[t] also needs, where a step
    was accepted, both residual norms 1e-9 away from their tolerances."""
    X = np.array(X0, np.float64)
    nt, n_wp, nd = X.shape
    assert 1 <= c <= n_wp - 2
    w = np.ones(nd) if dof_weights is None else np.asarray(dof_weights, np.float64)
    W, iW = w * w, 1.0 / (w * w)
    Minv = R.metric_inverse(n_wp)
    targets = np.asarray(targets, np.float64)
    f, sm, dm, g, rp, rr, r, J = merit(sc, link, c, with_rot, targets, X, margin, band, weight, W, pose_weight, rev)
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
        raw = -(alpha[L, None, None] * (s * iW[None, None, :]))
        step = projected_step(raw, Minv, c, r[L], J[L], iW, damp, rev)
        mx = np.abs(step).max(axis=(1, 2))
        with np.errstate(invalid="ignore"):
            scale = np.where(mx > max_step, max_step / np.where(mx > 0, mx, 1.0), 1.0)
        Xn = X[L].copy()
        Xn[:, 1:-1] = np.clip(X[L][:, 1:-1] + step * scale[:, None, None], sc.lo, sc.hi)
        fn, smn, dn, gn, rpn, rrn, rn, Jn = merit(sc, link, c, with_rot, targets[:, L], Xn, margin, band, weight, W,
                                                  pose_weight, rev)
        acc = fn <= f[L]
        done = acc & (f[L] - fn < ftol) & (dn >= margin - feas) & (rpn < tol_pos) & (rrn < tol_rot)
        scale_f = np.maximum(np.abs(fn), np.abs(f[L]))
        clear = np.abs(fn - f[L]) > 1e-9 * scale_f + 1e-18
        clear &= ~acc | ((np.abs((f[L] - fn) - ftol) > 1e-9 * np.maximum(scale_f, ftol))
                         & (np.abs(dn - (margin - feas)) > 1e-9)
                         & (np.abs(rpn - tol_pos) > 1e-9) & ((np.abs(rrn - tol_rot) > 1e-9) | (not with_rot)))
        determined[L] &= clear
        rec = np.full(nt, -1)
        rec[L] = acc
        accepts.append(rec)
        cand = np.full(nt, np.nan)
        cand[L] = fn
        cands.append(cand)
        A, Rj = L[acc], L[~acc]
        X[A], g[A], f[A], sm[A], dm[A] = Xn[acc], gn[acc], fn[acc], smn[acc], dn[acc]
        rp[A], rr[A], r[A], J[A] = rpn[acc], rrn[acc], rn[acc], Jn[acc]
        nacc[A] += 1
        alpha[A] = np.minimum(1.0, 2.0 * alpha[A])
        alpha[Rj] *= 0.25
        fin[Rj[alpha[Rj] < 1e-6]] = True
        D = L[done]
        fin[D] = True
        iters[D] = it
        merits.append(f.copy())
    return dict(X=X, iters=iters, info=np.stack([f, sm, dm, nacc, rp, rr]),
                accepts=np.array(accepts).reshape(-1, nt), merits=np.array(merits),
                candidates=np.array(cands).reshape(-1, nt), determined=determined)


# ---------------------------------------------------------------------------------- targets and initial guesses
def family_targets(sc, link, Xline, c, with_rot):
    """The link's pose at waypoint c of the lines Xline [nt, n_wp, nd], translated by SHIFT and (with_rot) turned by
    Rz(YAW) from the left -> [12, nt]."""
    pose = sc.om.fk_batch(np.ascontiguousarray(Xline[:, c].T), sc.ids, [link])[0]
    Rm, p = mat_of(pose)
    if with_rot:
        cz, sz = np.cos(YAW), np.sin(YAW)
        Rm = np.einsum("ab,nbc->nac", np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]]), Rm)
    return pose12_of(Rm, p + np.asarray(SHIFT))


def lines(q_start, goals, n_wp):
    """trajopt_ref.straight_lines, also for one start per trajectory (q_start [nd, nt])."""
    q_start = np.asarray(q_start, np.float64)
    if q_start.ndim == 1:
        return R.straight_lines(q_start, goals, n_wp)
    return np.concatenate([R.straight_lines(q_start[:, t], np.asarray(goals)[:, t:t + 1], n_wp)
                           for t in range(q_start.shape[1])])


def two_lines(q_start, q_mid, goals, n_wp, c):
    """start -> q_mid [nd, nt] at waypoint c -> goals [nd, nt]: X [nt, n_wp, nd] (waypoints c and n_wp-1 exact)."""
    qs = np.asarray(q_start, np.float64)
    qs = (qs[:, None] if qs.ndim == 1 else qs).T[:, None, :] * np.ones((q_mid.shape[1], 1, 1))
    qm, qg = q_mid.T[:, None, :], np.asarray(goals, np.float64).T[:, None, :]
    w = np.arange(n_wp)[None, :, None]
    X = np.where(w <= c, qs + (qm - qs) * (w / c), qm + (qg - qm) * ((w - c) / (n_wp - 1 - c)))
    X[:, c], X[:, n_wp - 1] = qm[:, 0], qg[:, 0]
    return X


def seeded_guess(sc, link, q_start, goals, n_wp, c, targets, with_rot):
    """The Python layer's initial guess: the constrained waypoint by the oracle's DLS IK (64 iterations,
    tolerances 1e-6) from that waypoint of the straight line, then two_lines."""
    q0 = np.ascontiguousarray(lines(q_start, goals, n_wp)[:, c].T)
    q, _, _ = sc.om.ik_dls_batch(q0, sc.ids, link, targets, max_iters=64, tol_pos=1e-6, tol_rot=1e-6,
                                 with_rot=bool(with_rot))
    return two_lines(q_start, q, goals, n_wp, c)


def good(out, margin, feas, tol=TOL):
    """A run's trajectories that meet the constraint and clear the box: |r_p|, |r_rot| < tol, dmin >= margin - feas."""
    return (out["info"][4] < tol) & (out["info"][5] < tol) & (out["info"][2] >= margin - feas)


@functools.lru_cache(maxsize=None)
def fetch_link(with_base=False):
    return R.scene(with_base).tree.link_id("gripper_link")


@functools.lru_cache(maxsize=None)
def fetch_problem(n_wp, rows, c=None, with_base=False, n_traj=R.N_GOALS):
    """The 32-goal family (goals repeated cyclically past 32): (sc, link, c, with_rot, targets [12, nt],
    X0 [nt, n_wp, nd])."""
    sc = R.scene(with_base)
    link = fetch_link(with_base)
    c = n_wp // 2 if c is None else c
    goals = np.ascontiguousarray(sc.q_goals[:, np.arange(n_traj) % R.N_GOALS])
    line = R.straight_lines(sc.q_start, goals, n_wp)
    tg = family_targets(sc, link, line, c, rows == 6)
    X0 = seeded_guess(sc, link, sc.q_start, goals, n_wp, c, tg, rows == 6)
    return sc, link, c, rows == 6, tg, X0


# the first-iterate cases of tests/test_gpu_trajopt_pose.py: (n_wp, n_traj, c) -- L = 8 / 16 / 64, a partial segment,
# several workgroups, c at the first and the last interior waypoint (the metric column at its edge)
FIRST_SHAPES = [(5, 1, 1), (10, 67, 5), (10, 5, 8), (33, 5, 31)]
FIRST_CASES = [(b, rows, s) for b in (False, True) for rows in (3, 6) for s in FIRST_SHAPES]


@functools.lru_cache(maxsize=None)
def first_run(with_base, rows, shape, max_iters, rev=False):
    """run() of a first-iterate case (its X0 is the seeded guess of fetch_problem); read-only."""
    n_wp, n_traj, c = shape
    sc, link, c, wr, tg, X0 = fetch_problem(n_wp, rows, c, with_base, n_traj)
    kw = {k: v for k, v in R.PARAMS.items() if k != "max_iters"}
    return run(sc, link, c, wr, tg, X0, max_iters=max_iters, rev=rev, **kw)


@functools.lru_cache(maxsize=None)
def full_run(n_wp, rows):
    """200 iterations on the 32-goal family, c = n_wp // 2 (shared by the CPU and the GPU tests; read-only)."""
    sc, link, c, wr, tg, X0 = fetch_problem(n_wp, rows)
    out = run(sc, link, c, wr, tg, X0, **R.PARAMS)
    out["X0"], out["targets"], out["c"] = X0, tg, c
    return out
