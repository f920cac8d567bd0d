"""Trajectory-optimisation constraints over waypoints (src/planning.jl) on the GPU.

SURVEY.md 8f row f3.  The constraint evaluations -- the serial inner loop of
``plan_trajectory`` in the reference (one ``set_joint_angles`` +
``compute_coll_dists_and_grads`` per waypoint, src/planning.jl:59-67) -- run as
ONE batched launch over all waypoints (of one or many trajectories):

* ``IneqConst``  -> ``kin_ineq_const_batch`` (k_coll with truncation
  ``margin + 0.05`` and the ``- margin`` offset fused in);
* ``PoseConstraint`` -> ``kin_pose_const_batch`` (k_fk with rpy Jacobian +
  k_pose_residual).

The optimiser stays on the host, as the reference's does: ``Objective``,
``ConfigurationConstraint``, ``EqConst`` are small host-side assemblies and
``plan_trajectory`` drives SciPy's SLSQP (the reference's ``solver=:SCIPY``
path).  NLopt and Ipopt are not installed, so ``solver=:NLOPT`` / ``:IPOPT`` are
refused; ``solver="SLSQP_BOUNDED"`` (the default) is SciPy's SLSQP with the
joint-limit bounds the reference's NLopt path sets (src/planning.jl:364-369) --
SciPy's implementation, not NLopt's -- and reports its status as a symbol.

``plan_trajectories`` / ``plan_trajectory(..., solver="GPU")`` are the batched, device-resident
alternative: ``kin_traj_opt_batch`` runs the whole descent of many trajectories in one kernel (a
covariant projected gradient on the smoothness objective plus sphere-clearance penalties -- a
different solver from SLSQP, see include/kinhip.h).  With one ``PoseConstraint`` of one link
(``pose_link=`` ...) the same kernel's constrained variant runs (``kin_traj_opt_pose_batch``): the
link is held at a target pose at one interior waypoint.  A checker whose spheres hang off several chains
(two arms) runs ``kin_traj_opt_tree_batch`` (``traj_opt_tree_batch``; no pose constraint there).  Against an
``AttachedUnionSDF`` (boxes on a moving scene, e.g. the fridge's door) ``kin_traj_opt_scene_batch`` runs
(``traj_opt_scene_batch``): every waypoint of every trajectory has its own scene state `scene_q`.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as K
from .collision import AttachedUnionSDF, SweptSphereCollisionChecker, UnionSDF, _plan_device
from .mechanism import Link, Mechanism, _device, _same_device

_DT = {torch.float32: K.KIN_F32, torch.float64: K.KIN_F64}


# ---------------------------------------------------------------------------- host side
class Objective:
    """src/planning.jl:1-28: xi^T A xi with A = kron(A_acc, diag(w^2)) (finite-difference acceleration)."""

    def __init__(self, n_wp: int, weights):
        from scipy import sparse
        w = np.asarray(weights, np.float64)
        A_sub = np.zeros((n_wp, n_wp))
        blk = np.array([[1, -2, 1], [-2, 4, -2], [1, -2, 1]], np.float64)
        for i in range(1, n_wp - 1):
            A_sub[i - 1:i + 2, i - 1:i + 2] += blk
        self.A = sparse.csc_matrix(np.kron(A_sub, np.diag(w ** 2)))
        self.n_dim = self.A.shape[1]

    def __call__(self, xi, grad: Optional[np.ndarray] = None) -> float:
        tmp = self.A @ np.asarray(xi, np.float64)
        if grad is not None and len(grad) > 0:
            grad[:] = 2.0 * tmp
        return float(np.dot(xi, tmp))


class IneqConst:
    """src/planning.jl:32-68.  ``__call__(xi, val_vec, jac_mat)`` fills the reference's dense
    layout (val_vec [n_coll*n_wp], jac_mat [n_dof*n_wp, n_coll*n_wp], block diagonal) from one
    GPU launch over the n_wp waypoints; ``eval_batch`` is the device-resident batched form."""

    def __init__(self, sscc: SweptSphereCollisionChecker, joints, sdf: UnionSDF, n_wp: int, margin: float,
                 dtype=torch.float64):
        self.sscc, self.joints, self.sdf = sscc, list(joints), sdf
        self.n_wp = int(n_wp)
        self.n_dof = len(self.joints) + (3 if sscc.mech.with_base else 0)
        self.n_coll = len(sscc.sphere_links)
        self.n_cons = self.n_coll * self.n_wp
        self.margin = float(margin)
        self.plan = sscc.plan(self.joints, dtype=dtype)
        self.dtype = dtype
        self.jac_mat = np.zeros((self.n_dof * self.n_wp, self.n_cons))
        self.val_vec = np.zeros(self.n_cons)

    def eval_batch(self, Q: torch.Tensor, with_jac=True, stream=None):
        """Q: device [n_dof, N] (any number of waypoints / trajectories side by side) ->
        vals [n_coll, N], jac [n_coll, n_dof, N] (or None).  Async on the stream."""
        if Q.dtype != self.dtype or not Q.is_cuda or Q.dim() != 2 or Q.shape[0] != self.n_dof or Q.stride(1) != 1:
            raise ValueError(f"Q must be a CUDA {self.dtype} tensor of shape ({self.n_dof}, N)")
        N = Q.shape[1]
        V = torch.empty((self.n_coll, N), dtype=self.dtype, device=Q.device)
        G = torch.empty((self.n_coll, self.n_dof, N), dtype=self.dtype, device=Q.device) if with_jac else None
        st = (stream or torch.cuda.current_stream(Q.device)).cuda_stream
        K.check(K.lib().kin_ineq_const_batch(self.plan._h, self.sdf._h, self.margin, Q.data_ptr(), Q.stride(0), N,
                                             V.data_ptr(), N, G.data_ptr() if G is not None else None, N, st))
        return V, G

    def __call__(self, xi, val_vec: np.ndarray, jac_mat: np.ndarray):
        xi = np.asarray(xi, np.float64)
        Q = torch.tensor(xi.reshape(self.n_wp, self.n_dof).T.copy(), dtype=self.dtype, device=_device())
        V, G = self.eval_batch(Q)
        v = V.double().cpu().numpy()    # [n_coll, n_wp]
        g = G.double().cpu().numpy()    # [n_coll, n_dof, n_wp]
        nd, nc = self.n_dof, self.n_coll
        for i in range(self.n_wp):
            jac_mat[nd * i:nd * (i + 1), nc * i:nc * (i + 1)] = g[:, :, i].T
        val_vec[:] = v.T.reshape(-1)


class PartialConstraint:
    idx_wp: int
    n_dof: int
    n_cons: int


class ConfigurationConstraint(PartialConstraint):
    """src/planning.jl:72-88: q(idx_wp) == q_const."""

    def __init__(self, idx_wp: int, n_dof: int, q_const):
        self.idx_wp, self.n_dof, self.n_cons = int(idx_wp), int(n_dof), int(n_dof)
        self.q_const = np.asarray(q_const, np.float64)

    def __call__(self, q, val_vec, jac_mat):
        j0 = (self.idx_wp - 1) * self.n_dof
        jac_mat[j0:j0 + self.n_dof, :] = -np.eye(self.n_dof)
        val_vec[:] = self.q_const - np.asarray(q, np.float64)


class PoseConstraint(PartialConstraint):
    """src/planning.jl:90-138: pose of each move link at waypoint idx_wp == target
    (position, plus rpy when with_rot); Jacobian = get_jacobian!(..., rpy_jac=true)."""

    def __init__(self, idx_wp: int, n_dof: int, move_links, target_poses, with_rots, mech: Mechanism, joints,
                 dtype=torch.float64):
        if isinstance(move_links, Link):
            move_links, target_poses, with_rots = [move_links], [target_poses], [with_rots]
        self.idx_wp, self.n_dof = int(idx_wp), int(n_dof)
        self.move_links, self.with_rots = list(move_links), [bool(w) for w in with_rots]
        self.target_poses = [np.asarray(T, np.float64).reshape(4, 4) for T in target_poses]
        self.n_cons = sum(6 if w else 3 for w in self.with_rots)
        self.mech, self.joints, self.dtype = mech, list(joints), dtype
        self.plans = [mech.plan(self.joints, out_links=[l], jac_link=l, jac_joints=self.joints, with_rot=w,
                                rpy_jac=w, dtype=dtype) for l, w in zip(self.move_links, self.with_rots)]

    def eval_batch(self, k: int, Q: torch.Tensor, targets: torch.Tensor, stream=None):
        """Move link k for N configurations: Q [n_dof, N], targets [12, N] (3x4 column-major) ->
        (vals [dim, N], jac [n_dof, dim, N], poses [12, N]) on the device."""
        p = self.plans[k]
        dim = 6 if self.with_rots[k] else 3
        N = Q.shape[1]
        if Q.dtype != self.dtype or not Q.is_cuda or Q.shape[0] != self.n_dof or Q.stride(1) != 1:
            raise ValueError(f"Q must be a CUDA {self.dtype} tensor of shape ({self.n_dof}, N)")
        if targets.dtype != self.dtype or targets.shape != (12, N) or targets.stride(1) != 1:
            raise ValueError("targets must be (12, N) in the plan dtype")
        _same_device(targets, Q, "targets")
        P = torch.empty((12, N), dtype=self.dtype, device=Q.device)
        V = torch.empty((dim, N), dtype=self.dtype, device=Q.device)
        J = torch.empty((self.n_dof, dim, N), dtype=self.dtype, device=Q.device)  # zero-filled plan
        st = (stream or torch.cuda.current_stream(Q.device)).cuda_stream
        K.check(K.lib().kin_pose_const_batch(p._h, targets.data_ptr(), targets.stride(0), Q.data_ptr(), Q.stride(0),
                                             N, P.data_ptr(), N, V.data_ptr(), N, J.data_ptr(), N, st))
        return V, J, P

    def __call__(self, q, val_vec, jac_mat):
        dev = _device()
        Q = torch.tensor(np.asarray(q, np.float64), dtype=self.dtype, device=dev).reshape(-1, 1).contiguous()
        j0 = (self.idx_wp - 1) * self.n_dof
        i0 = 0
        for k, (T, w) in enumerate(zip(self.target_poses, self.with_rots)):
            tg = torch.tensor(np.concatenate([T[:3, :3].T.reshape(-1), T[:3, 3]]), dtype=self.dtype,
                              device=dev).reshape(12, 1)
            V, J, _ = self.eval_batch(k, Q, tg)
            dim = 6 if w else 3
            val_vec[i0:i0 + dim] = V[:, 0].double().cpu().numpy()
            # get_jacobian!(..., transpose(jac)): jac_mat[j0 + d, i0 + r] = J[r, d]; irrelevant
            # columns are left untouched, as get_jacobian! leaves them
            Jh = J[:, :, 0].double().cpu().numpy()  # [n_dof, dim]
            rel = [self.mech.is_relevant(j, self.move_links[k]) for j in self.joints]
            rel += [True] * (self.n_dof - len(self.joints))
            for d in range(self.n_dof):
                if rel[d]:
                    jac_mat[j0 + d, i0:i0 + dim] = Jh[d]
            i0 += dim


class EqConst:
    """src/planning.jl:140-176: stacked partial constraints."""

    def __init__(self, n_wp: int, cons_arr: Sequence[PartialConstraint]):
        self.n_dof = cons_arr[0].n_dof
        assert all(c.n_dof == self.n_dof for c in cons_arr)
        self.n_wp, self.cons_arr = int(n_wp), list(cons_arr)
        self.n_cons = sum(c.n_cons for c in cons_arr)
        self.jac_mat = np.zeros((self.n_dof * self.n_wp, self.n_cons))
        self.val_vec = np.zeros(self.n_cons)

    def __call__(self, xi, val_vec, jac_mat):
        X = np.asarray(xi, np.float64).reshape(self.n_wp, self.n_dof)
        i0 = 0
        for c in self.cons_arr:
            c(X[c.idx_wp - 1], val_vec[i0:i0 + c.n_cons], jac_mat[:, i0:i0 + c.n_cons])
            i0 += c.n_cons


def create_straight_trajectory(q_start, q_goal, n_wp: int) -> np.ndarray:
    """src/planning.jl:304-308."""
    q_start, q_goal = np.asarray(q_start, np.float64), np.asarray(q_goal, np.float64)
    step = (q_goal - q_start) / (n_wp - 1)
    return np.concatenate([q_start + step * i for i in range(n_wp)])


def construct_problem(sscc, joints, sdf, q_start, q_goal, n_wp, n_dof, margin, partial_consts=()):
    """src/planning.jl:310-330."""
    eq = [ConfigurationConstraint(1, n_dof, q_start), ConfigurationConstraint(n_wp, n_dof, q_goal)]
    eq += list(partial_consts)
    return (Objective(n_wp, np.ones(n_dof)), IneqConst(sscc, joints, sdf, n_wp, margin), EqConst(n_wp, eq),
            n_dof * n_wp)


def traj_metric_inverse(n_wp: int) -> np.ndarray:
    """kin_traj_metric_inverse: (A_sub[I,I])^-1 over the interior waypoints, [(n_wp-2), (n_wp-2)] (host)."""
    out = np.zeros((max(int(n_wp) - 2, 0), max(int(n_wp) - 2, 0)))
    K.check(K.lib().kin_traj_metric_inverse(int(n_wp), out.ctypes.data if out.size else None))
    return out


def traj_opt_batch(plan, sdf: UnionSDF, X: torch.Tensor, n_wp: int, margin=2e-2, band=3e-2, weight=10.0, feas=1e-3,
                   ftol=1e-6, max_step=0.5, max_iters=200, dof_weights=None, iters=None, info=None, stream=None):
    """kin_traj_opt_batch in place on X [n_dof, n_traj * n_wp] (column t * n_wp + w = waypoint w of trajectory t;
    the end columns of every trajectory stay as given) with a ``CollisionPlan`` -> (iters [n_traj] int32,
    info [4, n_traj]: merit, smoothness term, min interior sphere distance, accepted steps).  Async on the stream
    after the plan's first call for this n_wp (which stages the metric table)."""
    return _traj_opt(K.lib().kin_traj_opt_batch, plan, sdf, X, n_wp, margin, band, weight, feas, ftol, max_step,
                     max_iters, dof_weights, iters, info, stream)


def traj_opt_tree_batch(plan, sdf: UnionSDF, X: torch.Tensor, n_wp: int, margin=2e-2, band=3e-2, weight=10.0,
                        feas=1e-3, ftol=1e-6, max_step=0.5, max_iters=200, dof_weights=None, iters=None, info=None,
                        stream=None):
    """kin_traj_opt_tree_batch: ``traj_opt_batch`` for a ``CollisionPlan`` whose spheres hang off several chains
    (``plan.n_parts`` > 1, e.g. both arms of a two-armed robot); the same arrays and results.  A single-chain plan
    runs ``traj_opt_batch``'s kernel."""
    return _traj_opt(K.lib().kin_traj_opt_tree_batch, plan, sdf, X, n_wp, margin, band, weight, feas, ftol, max_step,
                     max_iters, dof_weights, iters, info, stream)


def _scene_columns(plan, sdf, scene_q, X, n_traj, n_wp):
    """`scene_q` of ``traj_opt_scene_batch`` -> (tensor whose storage the call reads, lds).  (n_scene_cols,): one
    state for the launch (lds = 0); (n_scene_cols, n_traj): one per trajectory, expanded over its waypoints;
    (n_scene_cols, n_traj * n_wp): one per waypoint, column t * n_wp + w."""
    if not isinstance(scene_q, torch.Tensor):
        raise ValueError("an AttachedUnionSDF needs scene_q (its scene joint values) as a tensor")
    if scene_q.dtype != plan.dtype:
        raise ValueError("scene_q must have the plan dtype")
    _same_device(scene_q, X, "scene_q")
    nc = sdf.n_scene_cols
    if scene_q.dim() == 1:
        if scene_q.shape[0] != nc or not scene_q.is_contiguous():
            raise ValueError(f"scene_q must hold {nc} values")
        return scene_q, 0
    if scene_q.dim() == 2 and scene_q.shape == (nc, n_traj) and n_wp != 1:
        scene_q = scene_q.repeat_interleave(n_wp, dim=1)
    if scene_q.dim() != 2 or scene_q.shape != (nc, n_traj * n_wp) or (scene_q.numel() and scene_q.stride(1) != 1):
        raise ValueError(f"scene_q must be ({nc},), ({nc}, n_traj) or ({nc}, n_traj * n_wp) with unit sample stride")
    return scene_q, max(scene_q.stride(0), n_traj * n_wp)


def traj_opt_scene_batch(plan, sdf: AttachedUnionSDF, X: torch.Tensor, n_wp: int, scene_q: torch.Tensor, margin=2e-2,
                         band=3e-2, weight=10.0, feas=1e-3, ftol=1e-6, max_step=0.5, max_iters=200, dof_weights=None,
                         iters=None, info=None, stream=None):
    """kin_traj_opt_scene_batch: ``traj_opt_tree_batch`` (single-chain and multi-part ``CollisionPlan``s alike)
    against an ``AttachedUnionSDF`` of at most 2 moving groups, every waypoint with its own scene state.  `scene_q`
    holds the union's scene columns (its joints, then the scene's planar base x, y, theta): (n_scene_cols,) for the
    whole launch, (n_scene_cols, n_traj) per trajectory, or (n_scene_cols, n_traj * n_wp) per waypoint (column
    t * n_wp + w, as X) -- a door that swings while the robot moves.  The scene is data, not optimised.  The same
    arrays and results as ``traj_opt_batch``; info[2] is each interior waypoint's clearance at its own scene state
    (``CollisionPlan.run(sdf, X, scene_q=...)``)."""
    if not isinstance(sdf, AttachedUnionSDF):
        raise TypeError("traj_opt_scene_batch needs an AttachedUnionSDF (a static UnionSDF: traj_opt_tree_batch)")
    if (X.dtype != plan.dtype or not X.is_cuda or X.dim() != 2 or X.shape[0] != plan.n_dof or X.stride(1) != 1
            or X.shape[1] % int(n_wp) != 0):
        raise ValueError(f"X must be a CUDA {plan.dtype} tensor of shape ({plan.n_dof}, n_traj * n_wp)")
    _plan_device(plan, X)
    _plan_device(sdf, X)
    with torch.cuda.stream(stream or torch.cuda.current_stream(X.device)):   # (the per-trajectory form is expanded)
        sq, lds = _scene_columns(plan, sdf, scene_q, X, X.shape[1] // int(n_wp), int(n_wp))

    def entry(ph, sh, prm, *rest):
        return K.lib().kin_traj_opt_scene_batch(ph, sh, prm, sq.data_ptr() if sq.numel() else None, lds, *rest)
    return _traj_opt(entry, plan, sdf, X, n_wp, margin, band, weight, feas, ftol, max_step, max_iters, dof_weights,
                     iters, info, stream)


def _traj_opt(entry, plan, sdf, X, n_wp, margin, band, weight, feas, ftol, max_step, max_iters, dof_weights, iters,
              info, stream, info_rows=4):
    if (X.dtype != plan.dtype or not X.is_cuda or X.dim() != 2 or X.shape[0] != plan.n_dof or X.stride(1) != 1
            or X.shape[1] % int(n_wp) != 0):
        raise ValueError(f"X must be a CUDA {plan.dtype} tensor of shape ({plan.n_dof}, n_traj * n_wp)")
    n_traj = X.shape[1] // int(n_wp)
    dev = X.device
    it = iters if iters is not None else torch.empty(n_traj, dtype=torch.int32, device=dev)
    nf = info if info is not None else torch.empty((info_rows, n_traj), dtype=plan.dtype, device=dev)
    if nf.shape != (info_rows, n_traj) or nf.dtype != plan.dtype or it.shape != (n_traj,) or it.dtype != torch.int32:
        raise ValueError(f"info must be ({info_rows}, {n_traj}) in the plan dtype and iters ({n_traj},) int32")
    dw = None if dof_weights is None else np.ascontiguousarray(np.asarray(dof_weights, np.float64))
    if dw is not None and dw.shape != (plan.n_dof,):
        raise ValueError(f"dof_weights must have {plan.n_dof} entries")
    prm = K.TrajParams(int(n_wp), int(max_iters), float(margin), float(band), float(weight), float(feas), float(ftol),
                       float(max_step), dw.ctypes.data if dw is not None else None)
    st = (stream or torch.cuda.current_stream(dev)).cuda_stream
    K.check(entry(plan._h, sdf._h, C.byref(prm), X.data_ptr(), X.stride(0), n_traj, it.data_ptr(), nf.data_ptr(),
                  nf.stride(0), st))
    return it, nf


def traj_opt_pose_batch(plan, sdf: UnionSDF, X: torch.Tensor, n_wp: int, targets: torch.Tensor, wp: int, with_rot=True,
                        margin=2e-2, band=3e-2, weight=10.0, feas=1e-3, ftol=1e-6, max_step=0.5, max_iters=200,
                        dof_weights=None, pose_weight=10.0, damp=1e-6, tol_pos=1e-3, tol_rot=1e-3, iters=None,
                        info=None, stream=None):
    """kin_traj_opt_pose_batch in place on X [n_dof, n_traj * n_wp] with a ``TrajPlan``: ``traj_opt_batch`` with the
    plan's pose link 0 held at targets [12, n_traj] (3x4 column-major, one column per trajectory) at the interior
    waypoint `wp` (0-based), position only (with_rot False, 3 rows) or position + orientation (6 rows)
    -> (iters [n_traj] int32, info [6, n_traj]: merit, smoothness term, min interior sphere distance, accepted
    steps, |r_p|, |r_rot| of the returned state).  X is any initial guess; ``plan_trajectories`` seeds it by IK."""
    if (X.dtype != plan.dtype or not X.is_cuda or X.dim() != 2 or X.shape[0] != plan.n_dof or X.stride(1) != 1
            or X.shape[1] % int(n_wp) != 0):
        raise ValueError(f"X must be a CUDA {plan.dtype} tensor of shape ({plan.n_dof}, n_traj * n_wp)")
    n_traj = X.shape[1] // int(n_wp)
    if (targets.dtype != plan.dtype or not targets.is_cuda or targets.dim() != 2 or targets.shape != (12, n_traj)
            or (n_traj > 1 and targets.stride(1) != 1)):
        raise ValueError(f"targets must be a CUDA {plan.dtype} tensor of shape (12, {n_traj})")
    _same_device(targets, X, "targets")
    dev = X.device
    it = iters if iters is not None else torch.empty(n_traj, dtype=torch.int32, device=dev)
    nf = info if info is not None else torch.empty((6, n_traj), dtype=plan.dtype, device=dev)
    if nf.shape != (6, n_traj) or nf.dtype != plan.dtype or it.shape != (n_traj,) or it.dtype != torch.int32:
        raise ValueError(f"info must be (6, {n_traj}) in the plan dtype and iters ({n_traj},) int32")
    dw = None if dof_weights is None else np.ascontiguousarray(np.asarray(dof_weights, np.float64))
    if dw is not None and dw.shape != (plan.n_dof,):
        raise ValueError(f"dof_weights must have {plan.n_dof} entries")
    prm = K.TrajParams(int(n_wp), int(max_iters), float(margin), float(band), float(weight), float(feas), float(ftol),
                       float(max_step), dw.ctypes.data if dw is not None else None)
    wps, rots = (C.c_int32 * 1)(int(wp)), (C.c_int32 * 1)(1 if with_rot else 0)
    pp = K.TrajPoseParams(1, C.cast(wps, C.c_void_p), C.cast(rots, C.c_void_p), float(pose_weight), float(damp),
                          float(tol_pos), float(tol_rot))
    st = (stream or torch.cuda.current_stream(dev)).cuda_stream
    K.check(K.lib().kin_traj_opt_pose_batch(plan._h, sdf._h, C.byref(prm), C.byref(pp), targets.data_ptr(),
                                            max(targets.stride(0), n_traj), X.data_ptr(), X.stride(0), n_traj,
                                            it.data_ptr(), nf.data_ptr(), nf.stride(0), st))
    return it, nf


def traj_opt_pose_tree_batch(plan, sdf: UnionSDF, X: torch.Tensor, n_wp: int, targets: torch.Tensor, wp: int,
                             scene_q=None, with_rot=True, margin=2e-2, band=3e-2, weight=10.0, feas=1e-3, ftol=1e-6,
                             max_step=0.5, max_iters=200, dof_weights=None, pose_weight=10.0, damp=1e-6, tol_pos=1e-3,
                             tol_rot=1e-3, iters=None, info=None, stream=None):
    """kin_traj_opt_pose_tree_batch: ``traj_opt_pose_batch`` for every ``TrajPlan`` -- spheres on several chains
    (``plan.n_parts`` > 1, the pose link on any of them: ``plan.pose_link_parts``) and, with an ``AttachedUnionSDF``,
    `scene_q` as in ``traj_opt_scene_batch`` (a static ``UnionSDF`` takes none).  The same arrays and results as
    ``traj_opt_pose_batch``; a single-chain plan against a static union runs that call's kernel."""
    attached = isinstance(sdf, AttachedUnionSDF)
    if attached != (scene_q is not None):
        raise ValueError("scene_q goes with an AttachedUnionSDF (and an AttachedUnionSDF needs it)")
    if (X.dtype != plan.dtype or not X.is_cuda or X.dim() != 2 or X.shape[0] != plan.n_dof or X.stride(1) != 1
            or X.shape[1] % int(n_wp) != 0):
        raise ValueError(f"X must be a CUDA {plan.dtype} tensor of shape ({plan.n_dof}, n_traj * n_wp)")
    n_traj = X.shape[1] // int(n_wp)
    if (targets.dtype != plan.dtype or not targets.is_cuda or targets.dim() != 2 or targets.shape != (12, n_traj)
            or (n_traj > 1 and targets.stride(1) != 1)):
        raise ValueError(f"targets must be a CUDA {plan.dtype} tensor of shape (12, {n_traj})")
    _same_device(targets, X, "targets")
    _plan_device(plan, X)
    _plan_device(sdf, X)
    sq, lds = None, 0
    if attached:
        with torch.cuda.stream(stream or torch.cuda.current_stream(X.device)):   # (the per-trajectory form is expanded)
            sq, lds = _scene_columns(plan, sdf, scene_q, X, n_traj, int(n_wp))
    wps, rots = (C.c_int32 * 1)(int(wp)), (C.c_int32 * 1)(1 if with_rot else 0)
    pp = K.TrajPoseParams(1, C.cast(wps, C.c_void_p), C.cast(rots, C.c_void_p), float(pose_weight), float(damp),
                          float(tol_pos), float(tol_rot))

    def entry(ph, sh, prm, *rest):
        return K.lib().kin_traj_opt_pose_tree_batch(ph, sh, prm, C.byref(pp), targets.data_ptr(),
                                                    max(targets.stride(0), n_traj),
                                                    sq.data_ptr() if sq is not None and sq.numel() else None, lds, *rest)
    return _traj_opt(entry, plan, sdf, X, n_wp, margin, band, weight, feas, ftol, max_step, max_iters, dof_weights,
                     iters, info, stream, info_rows=6)


def _pose12(T, dtype, dev):
    """4x4 -> [12, 1] 3x4 column-major on the device."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    return torch.tensor(np.concatenate([T[:3, :3].T.reshape(-1), T[:3, 3]]), dtype=dtype, device=dev).reshape(12, 1)


def _seeded_guess(sscc, joints, pose_link, Qs, Qg, n_wp, c, tg, with_rot, dtype, st):
    """The guess of a pose-constrained plan, X [n_dof, n_traj * n_wp]: waypoint c by the batched IK (kin_ik_dls_batch,
    64 iterations to 1e-6) from its place on the straight line, then start -> IK answer -> goal."""
    n_dof, n_traj = Qs.shape
    i = torch.arange(n_wp, dtype=dtype, device=Qs.device)
    step = (Qg - Qs) / (n_wp - 1)
    ikp = sscc.mech.plan(list(joints), out_links=[pose_link], jac_link=pose_link, jac_joints=list(joints), dtype=dtype)
    Qm = (Qs + step * c).contiguous()
    ikp.ik_dls(tg, Qm, max_iters=64, tol_pos=1e-6, tol_rot=1e-6, with_rot=1 if with_rot else 0, stream=st)
    a, b = (i / c)[None, None, :], ((i - c) / (n_wp - 1 - c))[None, None, :]
    X = torch.where((i <= c)[None, None, :], Qs[:, :, None] + (Qm - Qs)[:, :, None] * a,
                    Qm[:, :, None] + (Qg - Qm)[:, :, None] * b)
    X[:, :, c] = Qm
    X[:, :, n_wp - 1] = Qg
    return X.reshape(n_dof, n_traj * n_wp).contiguous()


def plan_trajectories(sscc: SweptSphereCollisionChecker, joints, sdf: UnionSDF, Q_start, Q_goal, n_wp: int,
                      margin=2e-2, band=3e-2, weight=10.0, max_iters=200, dtype=torch.float64, X0=None, stream=None,
                      feas=1e-3, ftol=1e-6, max_step=0.5, dof_weights=None, plan=None, check_ends=True,
                      pose_link=None, pose_wp=None, pose_targets=None, pose_with_rot=True, pose_weight=10.0,
                      pose_tol=1e-3, scene_q=None):
    """Many ``plan_trajectory`` problems in one launch (kin_traj_opt_batch): Q_start / Q_goal [n_dof, n_traj]
    (or one [n_dof] vector for every trajectory) -> (X [n_dof, n_traj * n_wp], iters [n_traj], info [4, n_traj]).
    Trajectory t is X[:, t * n_wp:(t + 1) * n_wp]; it is feasible (every interior sphere distance >= margin -
    feas, merit settled to ftol) when iters[t] <= max_iters.  The straight-line initial guesses
    (create_straight_trajectory) are built on the device unless X0 is given; `check_ends` evaluates every start
    and goal in one kin_coll_batch and raises if one is in collision, as the reference asserts (it reads one
    flag back: pass False to stay asynchronous).  `plan`: a ``CollisionPlan`` of (sscc, joints, dtype) to reuse
    (its metric table is staged once per n_wp).

    With `pose_link`: that link is held at `pose_targets` ([12, n_traj] 3x4 column-major on the device, or one 4x4
    for every trajectory) at the interior waypoint `pose_wp` (0-based), with its orientation unless
    `pose_with_rot` is False (kin_traj_opt_pose_batch; `plan` is then a ``TrajPlan`` of (sscc, joints, [pose_link],
    dtype)).  Unless X0 is given, the constrained waypoint is solved first by the batched IK (kin_ik_dls_batch, 64
    iterations to 1e-6, from that waypoint of the straight line) and the guess is two straight lines, start -> IK
    answer -> goal.  info then has 6 rows (4: |r_p|, 5: |r_rot|), and a trajectory with iters[t] <= max_iters also
    meets the constraint to `pose_tol`.

    With an ``AttachedUnionSDF`` as `sdf` (kin_traj_opt_scene_batch): `scene_q` holds its scene columns as a tensor
    of `dtype` on the device, (n_scene_cols,) for every waypoint of every trajectory, (n_scene_cols, n_traj) per
    trajectory or (n_scene_cols, n_traj * n_wp) per waypoint (``traj_opt_scene_batch``); `check_ends` evaluates
    the starts at the scene state of waypoint 0 and the goals at that of waypoint n_wp - 1.  `pose_link` together
    with an attached union or with spheres on several chains raises: ``plan_trajectories_pose`` takes those."""
    return _plan_trajectories(False, sscc, joints, sdf, Q_start, Q_goal, n_wp, margin, band, weight, max_iters, dtype, X0,
                              stream, feas, ftol, max_step, dof_weights, plan, check_ends, pose_link, pose_wp,
                              pose_targets, pose_with_rot, pose_weight, pose_tol, scene_q)


def plan_trajectories_pose(sscc: SweptSphereCollisionChecker, joints, sdf: UnionSDF, Q_start, Q_goal, n_wp: int,
                           pose_link, pose_wp, pose_targets, pose_with_rot=True, margin=2e-2, band=3e-2, weight=10.0,
                           max_iters=200, dtype=torch.float64, X0=None, stream=None, feas=1e-3, ftol=1e-6, max_step=0.5,
                           dof_weights=None, check_ends=True, pose_weight=10.0, pose_tol=1e-3, scene_q=None, plan=None):
    """``plan_trajectories`` with `pose_link` held at `pose_targets` at the interior waypoint `pose_wp`, for every
    plan kind: with the checker's spheres on one chain and a static union it is ``plan_trajectories(pose_link=...)``
    itself (bit-equal); with spheres on several chains (`pose_link` on any of them) and / or an ``AttachedUnionSDF``
    with its `scene_q` it takes kin_traj_opt_pose_tree_batch (``traj_opt_pose_tree_batch``).  The arguments, the
    seeding of the guess (the constrained waypoint by the batched IK, then two straight lines), `check_ends` and the
    results (info: 6 rows) are those of ``plan_trajectories``; `plan`: a ``TrajPlan`` of (sscc, joints, [pose_link],
    dtype) to reuse."""
    return _plan_trajectories(True, sscc, joints, sdf, Q_start, Q_goal, n_wp, margin, band, weight, max_iters, dtype, X0,
                              stream, feas, ftol, max_step, dof_weights, plan, check_ends, pose_link, pose_wp,
                              pose_targets, pose_with_rot, pose_weight, pose_tol, scene_q)


def _plan_trajectories(pose_any, sscc, joints, sdf, Q_start, Q_goal, n_wp, margin, band, weight, max_iters, dtype, X0,
                       stream, feas, ftol, max_step, dof_weights, plan, check_ends, pose_link, pose_wp, pose_targets,
                       pose_with_rot, pose_weight, pose_tol, scene_q):
    """``plan_trajectories`` (pose_any False: a pose link takes one sphere chain and a static union) and
    ``plan_trajectories_pose``."""
    n_wp = int(n_wp)
    dev = _device()
    attached = isinstance(sdf, AttachedUnionSDF)
    if attached and pose_link is not None and not pose_any:
        raise ValueError("pose_link with an AttachedUnionSDF: pose constraints against a moving scene are not "
                         "supported (kin_traj_opt_scene_batch takes none)")
    if attached != (scene_q is not None):
        raise ValueError("scene_q goes with an AttachedUnionSDF (and an AttachedUnionSDF needs it)")
    if pose_link is None:
        if pose_wp is not None or pose_targets is not None:
            raise ValueError("pose_wp / pose_targets need pose_link")
        plan = plan if plan is not None else sscc.plan(list(joints), dtype=dtype)
    else:
        if pose_wp is None or pose_targets is None or not 1 <= int(pose_wp) <= n_wp - 2:
            raise ValueError(f"pose_link needs pose_targets and an interior pose_wp (1..{n_wp - 2})")
        if not pose_any and (plan if plan is not None else sscc.plan(list(joints), dtype=dtype)).n_parts > 1:
            raise ValueError("pose_link: the checker's spheres hang off several chains (kin_traj_opt_pose_batch "
                             "takes one sphere chain)")
        plan = plan if plan is not None else sscc.traj_plan(list(joints), [pose_link], dtype=dtype)
        if not getattr(plan, "pose_links", None) or plan.pose_links[0].id != pose_link.id:
            raise ValueError("plan must be a TrajPlan whose first pose link is pose_link")
    if plan.dtype != dtype:
        raise ValueError("plan dtype differs from dtype")
    n_dof = plan.n_dof

    def as_cols(Q, other):
        Q = torch.as_tensor(Q, dtype=dtype).to(dev)
        if Q.dim() == 1:
            n = other.shape[1] if isinstance(other, torch.Tensor) and other.dim() == 2 else 1
            Q = Q.reshape(-1, 1).expand(-1, n)
        if Q.dim() != 2 or Q.shape[0] != n_dof:
            raise ValueError(f"Q_start / Q_goal must be ({n_dof},) or ({n_dof}, n_traj)")
        return Q.contiguous()

    Qs = as_cols(Q_start, Q_goal if isinstance(Q_goal, torch.Tensor) else torch.as_tensor(Q_goal))
    Qg = as_cols(Q_goal, Qs)
    if Qs.shape[1] == 1 and Qg.shape[1] > 1:
        Qs = Qs.expand(-1, Qg.shape[1]).contiguous()
    if Qs.shape != Qg.shape:
        raise ValueError("Q_start and Q_goal differ in shape")
    n_traj = Qs.shape[1]
    st = stream or torch.cuda.current_stream(dev)
    with torch.cuda.stream(st):
        if attached:
            if not isinstance(scene_q, torch.Tensor) or scene_q.dtype != dtype:
                raise ValueError(f"scene_q must be a {dtype} tensor")
            nc = sdf.n_scene_cols
            if scene_q.dim() == 2 and scene_q.shape == (nc, n_traj * n_wp):
                ends = scene_q.reshape(nc, n_traj, n_wp)
                sq_ends = torch.cat([ends[:, :, 0], ends[:, :, n_wp - 1]], 1).contiguous()
            elif scene_q.dim() == 2 and scene_q.shape == (nc, n_traj):
                sq_ends = torch.cat([scene_q, scene_q], 1).contiguous()
            elif scene_q.dim() == 1 and scene_q.shape[0] == nc:
                sq_ends = scene_q.contiguous()
            else:
                raise ValueError(f"scene_q must be ({nc},), ({nc}, {n_traj}) or ({nc}, {n_traj * n_wp})")
        if check_ends and attached:
            _, _, mn = plan.run(sdf, torch.cat([Qs, Qg], 1), dists=False, min_dist=True, stream=st, scene_q=sq_ends)
            if not bool((mn > 0).all()):
                raise AssertionError("start / goal in collision")
        elif check_ends:
            _, _, mn = plan.run(sdf, torch.cat([Qs, Qg], 1), dists=False, min_dist=True, stream=st)
            if not bool((mn > 0).all()):
                raise AssertionError("start / goal in collision")
        if pose_link is not None:
            if isinstance(pose_targets, torch.Tensor):
                tg = pose_targets.to(device=dev, dtype=dtype)
            else:
                tg = _pose12(pose_targets, dtype, dev).expand(-1, n_traj)
            if tg.shape != (12, n_traj):
                raise ValueError(f"pose_targets must be (12, {n_traj}) or one 4x4 pose")
            tg = tg.contiguous()
        i = torch.arange(n_wp, dtype=dtype, device=dev)
        step = (Qg - Qs) / (n_wp - 1)
        if X0 is not None:
            X = torch.as_tensor(X0, dtype=dtype).to(dev).reshape(n_dof, n_traj * n_wp).clone()
        elif pose_link is None:
            # create_straight_trajectory (src/planning.jl:304-308) per trajectory; the last waypoint is the goal itself
            X = (Qs[:, :, None] + step[:, :, None] * i[None, None, :])
            X[:, :, n_wp - 1] = Qg
            X = X.reshape(n_dof, n_traj * n_wp).contiguous()
        else:
            X = _seeded_guess(sscc, joints, pose_link, Qs, Qg, n_wp, int(pose_wp), tg, pose_with_rot, dtype, st)
        if pose_link is not None and (attached or plan.n_parts > 1):
            it, nf = traj_opt_pose_tree_batch(plan, sdf, X, n_wp, tg, int(pose_wp), scene_q=scene_q,
                                              with_rot=pose_with_rot, margin=margin, band=band, weight=weight, feas=feas,
                                              ftol=ftol, max_step=max_step, max_iters=max_iters,
                                              dof_weights=dof_weights, pose_weight=pose_weight, tol_pos=pose_tol,
                                              tol_rot=pose_tol, stream=st)
        elif attached:
            it, nf = traj_opt_scene_batch(plan, sdf, X, n_wp, scene_q, margin=margin, band=band, weight=weight, feas=feas,
                                          ftol=ftol, max_step=max_step, max_iters=max_iters, dof_weights=dof_weights,
                                          stream=st)
        elif pose_link is None:
            opt = traj_opt_tree_batch if plan.n_parts > 1 else traj_opt_batch
            it, nf = opt(plan, sdf, X, n_wp, margin=margin, band=band, weight=weight, feas=feas, ftol=ftol,
                         max_step=max_step, max_iters=max_iters, dof_weights=dof_weights, stream=st)
        else:
            it, nf = traj_opt_pose_batch(plan, sdf, X, n_wp, tg, int(pose_wp), with_rot=pose_with_rot, margin=margin,
                                         band=band, weight=weight, feas=feas, ftol=ftol, max_step=max_step,
                                         max_iters=max_iters, dof_weights=dof_weights, pose_weight=pose_weight,
                                         tol_pos=pose_tol, tol_rot=pose_tol, stream=st)
    return X, it, nf


def plan_trajectory(sscc: SweptSphereCollisionChecker, joints, sdf: UnionSDF, q_start, q_goal, n_wp: int,
                    margin=2e-2, partial_consts=(), ftol_abs=1e-3, solver="SLSQP_BOUNDED", maxiter=200, scene_q=None):
    """src/planning.jl:332-401 -> (q_seq [n_dof, n_wp], status).  Constraint evaluations on the GPU.

    ``solver``: "SLSQP_BOUNDED" (SciPy SLSQP + joint-limit bounds; status ``:SUCCESS`` /
    ``:MAXEVAL_REACHED`` / ``:FAILURE``) or "SCIPY" (the reference's :SCIPY path: no bounds, returns
    SciPy's result).  "NLOPT" and "IPOPT" raise: those libraries are not installed.  "GPU": the batched
    penalty descent of ``plan_trajectories`` on a batch of one (fp64; `partial_consts` empty or exactly one
    ``PoseConstraint`` with one move link at an interior waypoint, held by the kernel's constrained update with
    the axis-angle residual to 1e-3; status ``:SUCCESS`` when it ended feasible within `maxiter`, else
    ``:MAXEVAL_REACHED``; ``ftol_abs`` is not used).  "GPU" only: `sdf` may be an ``AttachedUnionSDF`` with
    `scene_q` its scene columns, (n_scene_cols,) or (n_scene_cols, n_wp) -- one scene state per waypoint
    (kin_traj_opt_scene_batch); a ``PoseConstraint`` with spheres on several chains or with an attached union goes
    through ``plan_trajectories_pose``."""
    from scipy.optimize import minimize
    from .collision import compute_coll_dists

    solver = str(solver).lstrip(":").upper()
    if solver == "GPU":
        pcs = list(partial_consts)   # (checked before sscc is touched)
        if len(pcs) > 1 or (pcs and not (isinstance(pcs[0], PoseConstraint) and len(pcs[0].move_links) == 1)):
            raise ValueError("solver 'GPU' takes at most one partial constraint: a PoseConstraint with one move link")
        kw = {}
        if pcs:
            pc = pcs[0]
            if not 2 <= pc.idx_wp <= int(n_wp) - 1:
                raise ValueError(f"solver 'GPU': the PoseConstraint's idx_wp must be interior (2..{int(n_wp) - 1})")
            kw = dict(pose_link=pc.move_links[0], pose_wp=pc.idx_wp - 1, pose_targets=pc.target_poses[0],
                      pose_with_rot=pc.with_rots[0])
        if scene_q is not None:
            kw["scene_q"] = torch.as_tensor(scene_q, dtype=torch.float64).to(_device())
        # (a pose constraint: every plan kind; on one sphere chain with a static union it is plan_trajectories itself)
        X, it, _ = (plan_trajectories_pose if pcs else plan_trajectories)(
            sscc, joints, sdf, np.asarray(q_start, np.float64), np.asarray(q_goal, np.float64), n_wp, margin=margin,
            max_iters=maxiter, dtype=torch.float64, **kw)
        return X.cpu().numpy(), (":SUCCESS" if int(it[0]) <= maxiter else ":MAXEVAL_REACHED")
    if solver in ("NLOPT", "IPOPT"):
        raise ValueError(f"solver :{solver} needs a library that is not installed; use 'SLSQP_BOUNDED' "
                         "(SciPy SLSQP with the joint-limit bounds) or 'SCIPY'")
    if solver not in ("SLSQP_BOUNDED", "SCIPY"):
        raise ValueError(f"unknown solver {solver!r}")
    if scene_q is not None or isinstance(sdf, AttachedUnionSDF):
        raise ValueError("an AttachedUnionSDF / scene_q needs solver='GPU'")
    m = sscc.mech
    n_dof = len(joints) + (3 if m.with_base else 0)
    assert len(q_start) == n_dof and len(q_goal) == n_dof
    for q in (q_start, q_goal):
        m.set_joint_angles(joints, q)
        assert np.all(compute_coll_dists(sscc, joints, sdf) > 0.0), "start / goal in collision"
    xi0 = create_straight_trajectory(q_start, q_goal, n_wp)
    F, G, H, n_whole = construct_problem(sscc, joints, sdf, q_start, q_goal, n_wp, n_dof, margin, partial_consts)

    def cached(cons):  # one GPU evaluation per iterate serves both fun and jac
        last = {}

        def ev(x):
            key = x.tobytes()
            if last.get("key") != key:
                cons(x, cons.val_vec, cons.jac_mat)
                last.update(key=key, val=cons.val_vec.copy(), jac=cons.jac_mat.T.copy())
            return last
        return (lambda x: ev(x)["val"]), (lambda x: ev(x)["jac"])

    g_val, g_jac = cached(G)
    h_val, h_jac = cached(H)
    grad = np.zeros(n_whole)
    cons = [{"type": "ineq", "fun": g_val, "jac": g_jac}, {"type": "eq", "fun": h_val, "jac": h_jac}]
    bounds = None
    if solver == "SLSQP_BOUNDED":
        lo = [j.lower_limit for j in joints] + ([-np.inf] * 3 if m.with_base else [])
        hi = [j.upper_limit for j in joints] + ([np.inf] * 3 if m.with_base else [])
        bounds = list(zip(lo * n_wp, hi * n_wp))
    res = minimize(lambda x: F(x, grad), xi0, jac=lambda x: (F(x, grad), grad.copy())[1], method="SLSQP",
                   bounds=bounds, constraints=cons, options={"ftol": ftol_abs, "maxiter": maxiter})
    q_seq = res.x.reshape(n_wp, n_dof).T
    if solver == "SCIPY":
        return q_seq, res
    status = ":SUCCESS" if res.success else (":MAXEVAL_REACHED" if res.status == 9 else ":FAILURE")
    return q_seq, status


def collision_aware_ik(m: Mechanism, link: Link, joints, target_pose, sscc: SweptSphereCollisionChecker,
                       sdf: UnionSDF, use_bistage=True, ftol=1e-5, with_rot=True, max_iters=200, lam=1e-2,
                       max_step=0.5, margin=0.02, solver="DLS"):
    """``inverse_kinematics!(m, link, joints, target, sscc, sdf; use_bistage)`` (src/inverse_kinematics.jl:1-21);
    see ``kinhip.inverse_kinematics_``.  -> (q, status); sets the mechanism's angles.

    ``solver="DLS"`` (default): stage 1 (use_bistage) is the collision-free solve with the reference's
    ftol_abs rule (``_dls_ik_ftol``), stage 2 the batched collision-aware kernel
    (``CollisionIKPlan.ik_coll``, kin_ik_coll_batch: the reference's rpy objective plus the
    IneqConst(sscc, joints, sdf, 1, margin) sphere rows, 3 restarts: with use_bistage the first from the
    angles stage 1 started from (kin_ik_coll_batch_alt), the others seeded draws) on a batch of one, converged
    to |dp|, |d rpy| < 1e-6 with every sphere at >= margin - 1e-6 (status ``:FTOL_REACHED``).  When no
    attempt converges (a pose the constraint forbids) the kernel returns the attempt whose end state has
    the lowest merit |dp|^2 + |d rpy|^2 + max(0, margin - min d)^2 (the penalty problem's value; ties: the
    earlier attempt, so the stage-1-seeded attempt 0 wins over equal restarts), status
    ``:MAXEVAL_REACHED``.  ``ftol`` applies to stage 1 only: stage 2 is judged on the 1e-6 rule above.
    ``solver="SLSQP"``: stage 2 by SciPy's SLSQP on the host (the reference uses NLopt's LD_SLSQP), one
    GPU evaluation per iterate, ``ftol`` as the reference's ftol_abs."""
    from .collision import CollisionIKPlan
    from .mechanism import _dls_ik_ftol

    q_start = np.asarray(m.get_joint_angles(joints), np.float64)  # stage 2's restart attempt 1 starts here
    if use_bistage:  # stage 1: the collision-free problem seeds stage 2 (src/inverse_kinematics.jl:8-13)
        _dls_ik_ftol(m, link, joints, target_pose, ftol, with_rot, max_iters, lam, max_step)
    n_dof = len(joints) + (3 if m.with_base else 0)
    T = np.asarray(target_pose, np.float64).reshape(4, 4)
    dev = _device()
    tg = torch.tensor(np.concatenate([T[:3, :3].T.reshape(-1), T[:3, 3]]), dtype=torch.float64,
                      device=dev).reshape(12, 1)
    if str(solver).upper() == "DLS":
        plan = CollisionIKPlan(sscc, link, joints, dtype=torch.float64)
        Q0 = torch.tensor(m.get_joint_angles(joints), dtype=torch.float64, device=dev).reshape(-1, 1).contiguous()
        Q = torch.empty_like(Q0)
        Qa = torch.tensor(q_start, dtype=torch.float64, device=dev).reshape(-1, 1).contiguous() if use_bistage else None
        Q, it, err = plan.ik_coll(sdf, tg.contiguous(), Q, Q0=Q0, margin=margin, with_rot=2 if with_rot else 0,
                                  max_iters=max_iters, restarts=3, lam=lam, max_step=max_step, tol_pos=1e-6,
                                  tol_rot=1e-6, Q_alt=Qa)
        q = Q[:, 0].cpu().numpy()
        m.set_joint_angles(joints, q)
        return q, (":FTOL_REACHED" if int(it[0]) <= max_iters else ":MAXEVAL_REACHED")
    if str(solver).upper() != "SLSQP":
        raise ValueError(f"unknown solver {solver!r} (DLS or SLSQP)")
    from scipy.optimize import minimize
    # objective: PoseConstraint's residual [p - p*; rpy - rpy*] and its rpy Jacobian on the GPU
    pc = PoseConstraint(1, n_dof, link, T, with_rot, m, joints, dtype=torch.float64)
    # src/inverse_kinematics.jl:16 (a checker without spheres has no constraints: the reference's own
    # PR2 test builds one, test/test_inverse_kinematics.jl:63, with an un-iterated generator)
    G = IneqConst(sscc, joints, sdf, 1, margin, dtype=torch.float64) if sscc.sphere_links else None
    rel = np.array([m.is_relevant(j, link) for j in joints] + [True] * (n_dof - len(joints)))

    def pose_eval(x):
        Q = torch.tensor(np.asarray(x, np.float64), dtype=torch.float64, device=dev).reshape(-1, 1).contiguous()
        V, J, _ = pc.eval_batch(0, Q, tg)
        v = V[:, 0].cpu().numpy()               # now - target
        Jh = J[:, :, 0].cpu().numpy() * rel[:, None]  # [n_dof, dim]
        return float(np.dot(v, v)), 2.0 * Jh @ v  # f = sum(diff.^2), grad = -2 J^T diff

    def cached(fn):
        last = {}

        def ev(x):
            k = np.asarray(x, np.float64).tobytes()
            if last.get("k") != k:
                last.update(k=k, r=fn(x))
            return last["r"]
        return ev

    fo = cached(pose_eval)

    def g_eval(x):
        G(x, G.val_vec, G.jac_mat)
        return G.val_vec + 1e-8, G.jac_mat.T.copy()  # nloptize(G) <= 1e-8  <=>  dist - margin >= -1e-8
    go = cached(g_eval)
    lo = [j.lower_limit for j in joints] + [-np.inf] * (n_dof - len(joints))
    hi = [j.upper_limit for j in joints] + [np.inf] * (n_dof - len(joints))
    x0 = np.clip(m.get_joint_angles(joints), lo, hi)
    cons = [{"type": "ineq", "fun": lambda x: go(x)[0], "jac": lambda x: go(x)[1]}] if G is not None else []
    res = minimize(lambda x: fo(x)[0], x0, jac=lambda x: fo(x)[1], method="SLSQP", bounds=list(zip(lo, hi)),
                   constraints=cons, options={"ftol": ftol, "maxiter": max_iters})  # ftol_abs, as the reference
    q = np.asarray(res.x, np.float64)
    m.set_joint_angles(joints, q)
    status = ":FTOL_REACHED" if res.success else (":MAXEVAL_REACHED" if res.status == 9 else ":FAILURE")
    return q, status
