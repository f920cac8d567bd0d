"""Throughput of the batched trajectory optimiser (kin_traj_opt_batch, kinhip.plan_trajectories) on the reference's
planning scene (test/test_planning.jl: Fetch, four collision links, a thin box; q_start = 0, 32 collision-free IK
goals for (0.3, -0.4, 1.2)), n_wp = 10, fp32 and fp64, the 32 problems replicated to 32 / 1,024 / 32,768
trajectories.  For comparison: the only way to do the same work before, kinhip.plan_trajectory (SciPy SLSQP on
the host, one GPU constraint evaluation per iterate) looped over the same 32 problems.  The two solvers differ
(a penalty descent vs SLSQP on the constrained problem): the comparison is on feasibility and time, not iterates.

    python tools/traj_bench.py [--reps 5] [--no-slsqp] [--out profiles/traj_bench.json]
    python tools/traj_bench.py --scene pr2 [--out profiles/traj_bench_pr2.json]
    python tools/traj_bench.py --scene pr2-door [--out profiles/traj_bench_scene.json]
    python tools/traj_bench.py --pose [--out profiles/traj_bench_pose_tree.json]

--scene pr2: the reference's fridge_demo.jl shape -- the PR2 (tests/golden/pr2_two_arms.urdf) with both arms and
the planar base (17 columns), kinhip.PR2_ARM_SPHERES on two chains (kin_traj_opt_tree_batch), the static fridge
union at door 2.0 and base (1.2, 0, 0), from PR2_MANIP_POSE to 32 collision-free goals at the fridge (random arm
offsets of up to +-0.6 rad, the base driven 0.2-0.7 towards the fridge, +-0.15 sideways and turned by up to +-0.3,
from default_rng(0); the first 32 with every sphere more than 0.05 clear).  straight_infeasible_of_32 counts the
problems whose straight line does not clear the fridge by margin - feas.

--scene pr2-door: the pr2 leg's robot, goals and fridge through kin_traj_opt_scene_batch (k_traj_scene), the fridge an
AttachedUnionSDF(fridge, [door_joint]): (a) "uniform", one scene state for the launch (lds = 0) at door 2.0 and base
(1.2, 0, 0) -- the same problems as the pr2 leg -- and (b) "swing", a scene state per waypoint, the door closing from
2.0 to 1.2 over the waypoints of every trajectory; beside them, in the same process and with the repeats
interleaved (static, uniform, swing, static, ...), "static": kin_traj_opt_tree_batch on the static snapshot, and
ratio_to_static = the uniform leg's median over that one's.  Feasibility is re-evaluated with kin_coll_batch_scene
at every waypoint's own scene state.

--pose: the pr2 leg's robot, goals and fridge with the left tool frame held at waypoint 5 (6 rows) through
kinhip.plan_trajectories_pose (kin_traj_opt_pose_tree_batch, k_traj_pose_tree; the IK seeding of the guess is inside the
timed call): "static" against the static union and "swing" with the door closing from 2.0 to 1.2 over the waypoints.
The target of problem t is the tool frame's pose at waypoint 5 of its straight line, moved by (-0.05, 0, 0.10) and
turned by 0.3 rad about z.  good_of_32: |r_p|, |r_rot| < 1e-3 and clearance >= margin - feas.  Beside them the only
path there was before: kinhip.plan_trajectory (SLSQP on the host) with the PoseConstraint, looped over the 32 static
problems (it cannot take the moving door).

Timing: a host clock around calls that end in a device synchronise, after a warm-up call per shape; the median of
--reps repeats and their min / max.  Iterations per second counts, per trajectory, the iterations the kernel ran
(iters, or max_iters when a trajectory did not finish; an upper bound for stalled ones); for SLSQP it is the
constraint evaluations per second (one per iterate or line-search point).  Needs a GPU: there is no CPU fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "kinematics.jl_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import kinhip  # noqa: E402

COLL_LINKS = ["wrist_flex_link", "torso_lift_link", "upperarm_roll_link", "elbow_flex_link"]
N_WP, MARGIN, FEAS, MAX_ITERS = 10, 0.02, 1e-3, 200


def scene():
    m = kinhip.parse_urdf(os.path.join(ROOT, "tests", "golden", "fetch.urdf"))
    joints = [m.find_joint(n) for n in kinhip.FETCH_ARM_JOINTS]
    sscc = kinhip.SweptSphereCollisionChecker(m)
    for n in COLL_LINKS:
        kinhip.add_coll_links(sscc, m.find_link(n))
    T = np.eye(4)
    T[:3, 3] = (0.4, -0.25, 0.7)
    sdf = kinhip.UnionSDF([kinhip.BoxSDF(T, (0.05, 0.05, 0.5))])
    return m, joints, sscc, sdf


def scene_pr2():
    m = kinhip.parse_urdf(os.path.join(ROOT, "tests", "golden", "pr2_two_arms.urdf"), with_base=True)
    joints = [m.find_joint(n) for n in kinhip.PR2_RARM_JOINTS + kinhip.PR2_LARM_JOINTS]
    m.set_joint_angles([m.find_joint("torso_lift_joint")], [kinhip.PR2_MANIP_POSE[2], 0.0, 0.0, 0.0])
    sscc = kinhip.SweptSphereCollisionChecker(m)
    for name, c, r in kinhip.PR2_ARM_SPHERES:
        sscc.add_coll_sphere(m.find_link(name), c, r)
    fridge = kinhip.parse_urdf(os.path.join(ROOT, "tests", "golden", "fridge.urdf"), with_base=True)
    return m, joints, sscc, kinhip.fridge_sdf(fridge)


def goals_pr2(joints, sscc, sdf, q_start, n=32):
    """The first n collision-free (min d > 0.05) random offsets of q_start, clipped to the joint limits."""
    N = 4096
    rng = np.random.default_rng(0)
    Q = q_start[:, None] + np.concatenate([rng.uniform(-0.6, 0.6, (14, N)), rng.uniform(0.2, 0.7, (1, N)),
                                           rng.uniform(-0.15, 0.15, (1, N)), rng.uniform(-0.3, 0.3, (1, N))])
    lo = np.array([j.lower_limit for j in joints] + [-np.inf] * 3)
    hi = np.array([j.upper_limit for j in joints] + [np.inf] * 3)
    Q = torch.tensor(np.clip(Q, lo[:, None], hi[:, None]), dtype=torch.float64, device="cuda")
    _, _, mn = sscc.plan(joints, dtype=torch.float64).run(sdf, Q, dists=False, min_dist=True)
    ok = (mn > 0.05).nonzero()[:n, 0]
    assert ok.numel() == n, int(ok.numel())
    return Q[:, ok].contiguous()


def goals(m, joints, sscc, sdf, n=32):
    """The first n collision-free (min d > 0.05) batched-IK solutions from default_rng(0).uniform(-1, 1) starts."""
    gl = m.find_link("gripper_link")
    N = 512
    Q0 = torch.tensor(np.random.default_rng(0).uniform(-1, 1, (8, N)), dtype=torch.float64, device="cuda")
    tgt = torch.tensor(np.repeat(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0.3, -0.4, 1.2]).reshape(12, 1), N, axis=1),
                       dtype=torch.float64, device="cuda")
    plan = m.plan(joints, out_links=[gl], jac_link=gl, jac_joints=joints, dtype=torch.float64)
    Q, it, _ = plan.ik_dls(tgt, Q0, with_rot=False, max_iters=64)
    _, _, mn = sscc.plan(joints, dtype=torch.float64).run(sdf, Q, dists=False, min_dist=True)
    ok = ((it <= 64) & (mn > 0.05)).nonzero()[:n, 0]
    assert ok.numel() == n
    return Q[:, ok].contiguous()


def interior_clearance(cp64, sdf, X, n_traj, scene_q=None):
    _, _, mn = cp64.run(sdf, X.double(), dists=False, min_dist=True, scene_q=scene_q)
    return mn.reshape(n_traj, N_WP)[:, 1:-1].min(1).values


def timed_interleaved(fns, reps):
    """timed() for several calls with their repeats interleaved (a, b, c, a, b, c, ...): one warm-up each."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append(time.perf_counter() - t0)
    return [(float(np.median(t)), float(min(t)), float(max(t))) for t in ts]


def door_legs(a, res, joints, sscc, sdf, q_start, G, cp64):
    """--scene pr2-door: static (k_traj_tree) / uniform (k_traj_scene, lds = 0) / swing (a scene state per waypoint)."""
    fridge = kinhip.parse_urdf(os.path.join(ROOT, "tests", "golden", "fridge.urdf"), with_base=True)
    att = kinhip.AttachedUnionSDF(fridge, [fridge.find_joint("door_joint")])
    state = [2.0, 1.2, 0.0, 0.0]                                 # door, base x, y, theta: fridge_sdf's snapshot
    for dtype in (torch.float32, torch.float64):
        cp = sscc.plan(joints, dtype=dtype)
        for n_traj in (32, 1024, 32768):
            Qg = G.repeat(1, n_traj // 32).to(dtype).contiguous()
            uni = torch.tensor(state, dtype=dtype, device="cuda")
            swing = uni[:, None].repeat(1, n_traj * N_WP)
            swing[0] = torch.linspace(2.0, 1.2, N_WP, dtype=dtype, device="cuda").repeat(n_traj)
            legs = (("static", sdf, None), ("uniform", att, uni), ("swing", att, swing))
            out = {}

            def call_of(mode, s, sq):
                def call():
                    out[mode] = kinhip.plan_trajectories(sscc, joints, s, q_start, Qg, N_WP, margin=MARGIN, feas=FEAS,
                                                         max_iters=MAX_ITERS, dtype=dtype, plan=cp, check_ends=False,
                                                         scene_q=sq)
                return call
            times = timed_interleaved([call_of(*leg) for leg in legs], a.reps)
            for (mode, s, sq), (med, lo, hi) in zip(legs, times):
                X, it, info = out[mode]
                ran = torch.clamp(it, max=MAX_ITERS).sum().item()
                d = interior_clearance(cp64, s, X, n_traj, None if sq is None else sq.double())
                feas32 = int((d[:32] >= MARGIN - FEAS - (1e-6 if dtype == torch.float32 else 0.0)).sum())
                row = {"mode": mode, "dtype": str(dtype).split(".")[-1], "n_traj": n_traj, "seconds_median": med,
                       "seconds_min": lo, "seconds_max": hi, "traj_per_s": n_traj / med, "iters_per_s": ran / med,
                       "mean_iters": ran / n_traj, "feasible_of_32": feas32,
                       "done_of_32": int((it[:32] <= MAX_ITERS).sum())}
                if mode == "uniform":
                    row["ratio_to_static"] = med / times[0][0]
                res["gpu"].append(row)
                print(json.dumps(row), flush=True)


def pose_legs(a, res, m, joints, sscc, sdf, q_start, G, cp64):
    """--pose: the left tool frame at waypoint 5, static union and swinging door (k_traj_pose_tree), then the SLSQP loop."""
    link, c = m.find_link("l_gripper_tool_frame"), 5
    fridge = kinhip.parse_urdf(os.path.join(ROOT, "tests", "golden", "fridge.urdf"), with_base=True)
    att = kinhip.AttachedUnionSDF(fridge, [fridge.find_joint("door_joint")])
    qs = torch.tensor(q_start, dtype=torch.float64, device="cuda")[:, None]
    Qc = (qs + (G - qs) * (c / (N_WP - 1))).contiguous()
    T = kinhip.get_transform_batch(m, [link], joints, Qc).double().reshape(12, 32)
    cz, sz = np.cos(0.3), np.sin(0.3)
    Rz = torch.tensor([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64, device="cuda")
    Rm = Rz @ T[:9].T.reshape(32, 3, 3).transpose(1, 2)                     # (3x4 column-major -> R, turned)
    tg32 = torch.cat([Rm.transpose(1, 2).reshape(32, 9).T, T[9:12] + torch.tensor([[-0.05], [0.0], [0.10]], device="cuda")])
    for dtype in (torch.float32, torch.float64):
        tp = sscc.traj_plan(joints, [link], dtype=dtype)
        for n_traj in (32, 1024, 32768):
            Qg = G.repeat(1, n_traj // 32).to(dtype).contiguous()
            tg = tg32.repeat(1, n_traj // 32).to(dtype).contiguous()
            swing = torch.tensor([2.0, 1.2, 0.0, 0.0], dtype=dtype, device="cuda")[:, None].repeat(1, n_traj * N_WP)
            swing[0] = torch.linspace(2.0, 1.2, N_WP, dtype=dtype, device="cuda").repeat(n_traj)
            legs = (("static", sdf, None), ("swing", att, swing))
            out = {}

            def call_of(mode, s, sq):
                def call():
                    out[mode] = kinhip.plan_trajectories_pose(sscc, joints, s, q_start, Qg, N_WP, link, c, tg,
                                                              margin=MARGIN, feas=FEAS, max_iters=MAX_ITERS, dtype=dtype,
                                                              plan=tp, check_ends=False, scene_q=sq)
                return call
            times = timed_interleaved([call_of(*leg) for leg in legs], a.reps)
            for (mode, s, sq), (med, lo, hi) in zip(legs, times):
                X, it, info = out[mode]
                ran = torch.clamp(it, max=MAX_ITERS).sum().item()
                d = interior_clearance(cp64, s, X, n_traj, None if sq is None else sq.double())
                ok = (d[:32] >= MARGIN - FEAS - (1e-6 if dtype == torch.float32 else 0.0)) \
                    & (info[4, :32] < 1e-3) & (info[5, :32] < 1e-3)
                row = {"mode": mode, "dtype": str(dtype).split(".")[-1], "n_traj": n_traj, "seconds_median": med,
                       "seconds_min": lo, "seconds_max": hi, "traj_per_s": n_traj / med, "iters_per_s": ran / med,
                       "mean_iters": ran / n_traj, "good_of_32": int(ok.sum()),
                       "done_of_32": int((it[:32] <= MAX_ITERS).sum())}
                res["gpu"].append(row)
                print(json.dumps(row), flush=True)
    if not a.no_slsqp:
        Gh, th = G.cpu().numpy(), tg32.cpu().numpy()
        t0 = time.perf_counter()
        ok = 0
        for t in range(32):
            T4 = np.eye(4)
            T4[:3, :3], T4[:3, 3] = th[:9, t].reshape(3, 3).T, th[9:12, t]
            pc = kinhip.PoseConstraint(c + 1, len(q_start), link, T4, True, m, joints)
            _, status = kinhip.plan_trajectory(sscc, joints, sdf, q_start, Gh[:, t], N_WP, margin=MARGIN, ftol_abs=1e-5,
                                               partial_consts=[pc])
            ok += int(status == ":SUCCESS")
        dt = time.perf_counter() - t0
        res["slsqp"] = {"mode": "static", "n_traj": 32, "seconds": dt, "traj_per_s": 32 / dt, "success_of_32": ok}
        print(json.dumps(res["slsqp"]), flush=True)


def timed(fn, reps):
    fn()  # warm-up: code objects, the metric table, allocator
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-slsqp", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--scene", choices=("fetch", "pr2", "pr2-door"), default="fetch")
    ap.add_argument("--pose", action="store_true", help="the left tool frame held at waypoint 5 (implies the pr2 scene)")
    a = ap.parse_args()
    if a.pose:
        a.scene = "pr2"
    if not torch.cuda.is_available():
        sys.exit("traj_bench.py needs a GPU")
    if a.scene in ("pr2", "pr2-door"):
        m, joints, sscc, sdf = scene_pr2()
        ra, la, _ = kinhip.PR2_MANIP_POSE
        q_start = np.concatenate([np.deg2rad(np.array(ra + la)), np.zeros(3)])
        G = goals_pr2(joints, sscc, sdf, q_start)
        name = "pr2, both arms + base, fridge (door 2.0, base (1.2, 0, 0)), 32 collision-free goals"
    else:
        m, joints, sscc, sdf = scene()
        G = goals(m, joints, sscc, sdf)
        q_start = np.zeros(8)
        name = "fetch + thin box, 32 IK goals"
    cp64 = sscc.plan(joints, dtype=torch.float64)
    qs = torch.tensor(q_start, dtype=torch.float64, device="cuda")[:, None, None]
    lines = qs + (G[:, :, None] - qs) * (torch.arange(N_WP, dtype=torch.float64, device="cuda") / (N_WP - 1))
    d0 = interior_clearance(cp64, sdf, lines.reshape(len(q_start), 32 * N_WP).contiguous(), 32)
    res = {"scene": name, "n_wp": N_WP, "max_iters": MAX_ITERS, "parts": cp64.n_parts,
           "straight_infeasible_of_32": int((d0 < MARGIN - FEAS).sum()), "gpu": []}
    print(json.dumps({k: v for k, v in res.items() if k != "gpu"}), flush=True)
    if a.scene == "pr2-door" or a.pose:
        (pose_legs(a, res, m, joints, sscc, sdf, q_start, G, cp64) if a.pose else
         door_legs(a, res, joints, sscc, sdf, q_start, G, cp64))
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        return
    for dtype in (torch.float32, torch.float64):
        cp = sscc.plan(joints, dtype=dtype)
        for n_traj in (32, 1024, 32768):
            Qg = G.repeat(1, n_traj // 32).to(dtype).contiguous()
            out = {}

            def call():
                out["r"] = kinhip.plan_trajectories(sscc, joints, sdf, q_start, Qg, N_WP, margin=MARGIN, feas=FEAS,
                                                    max_iters=MAX_ITERS, dtype=dtype, plan=cp, check_ends=False)
            med, lo, hi = timed(call, a.reps)
            X, it, info = out["r"]
            ran = torch.clamp(it, max=MAX_ITERS).sum().item()
            d = interior_clearance(cp64, sdf, X, n_traj)
            feas32 = int((d[:32] >= MARGIN - FEAS - (1e-6 if dtype == torch.float32 else 0.0)).sum())
            row = {"dtype": str(dtype).split(".")[-1], "n_traj": n_traj, "seconds_median": med, "seconds_min": lo,
                   "seconds_max": hi, "traj_per_s": n_traj / med, "iters_per_s": ran / med,
                   "mean_iters": ran / n_traj, "feasible_of_32": feas32, "done_of_32": int((it[:32] <= MAX_ITERS).sum())}
            res["gpu"].append(row)
            print(json.dumps(row), flush=True)
    if not a.no_slsqp:
        # the previous path: one host SLSQP per problem (its own GPU launch and copy per iterate)
        from kinhip import planning
        evals = [0]
        inner = planning.IneqConst.__call__

        def counted(self, xi, val_vec, jac_mat):  # one GPU constraint evaluation per SLSQP iterate / line-search point
            evals[0] += 1
            return inner(self, xi, val_vec, jac_mat)
        planning.IneqConst.__call__ = counted
        Gh = G.cpu().numpy()
        t0 = time.perf_counter()
        feas, ok = 0, 0
        for t in range(32):
            q_seq, status = kinhip.plan_trajectory(sscc, joints, sdf, q_start, Gh[:, t], N_WP, margin=MARGIN,
                                                   ftol_abs=1e-5)
            X = torch.tensor(np.ascontiguousarray(q_seq), dtype=torch.float64, device="cuda")
            feas += int(interior_clearance(cp64, sdf, X, 1)[0] >= MARGIN - FEAS)
            ok += int(status == ":SUCCESS")
        dt = time.perf_counter() - t0
        planning.IneqConst.__call__ = inner
        res["slsqp"] = {"n_traj": 32, "seconds": dt, "traj_per_s": 32 / dt, "constraint_evals_per_s": evals[0] / dt,
                        "mean_constraint_evals": evals[0] / 32, "feasible_of_32": feas, "success_of_32": ok}
        print(json.dumps(res["slsqp"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
