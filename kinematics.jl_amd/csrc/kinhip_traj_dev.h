// kinhip_traj_dev.h -- traj_body, the one device body of k_traj (kin_traj_opt_batch), k_traj_pose (POSE), k_traj_tree
// (TREE), k_traj_scene (SCENE) and k_traj_pose_tree (POSE and TREE, any SCENE).  Included by the kinhip_traj*.hip units
// only (no run-time specialisation: not part of the embedded sources).  gfx950 only.
//
// Many independent trajectories of n_wp waypoints per launch, one lane per waypoint, each trajectory
// in a wave segment of L = 8 / 16 / 32 / 64 lanes (the smallest L >= n_wp).  Per iteration a lane
// walks the sphere chain of its own waypoint (step_a / union_sdf / box_gradient of k_coll) and keeps
// the penalty half-gradient, the penalty sum and the minimum distance in registers; the second
// differences of the smoothness objective (src/planning.jl:1-28) come from the neighbour lanes; the
// covariant step Minv g goes through LDS; the line-search decisions are per-segment values held by
// every lane of the segment (selects, never a divergent branch around a cross-lane operation).
//
// POSE = true (kin_traj_opt_pose_batch, chain bounds 4 and 8): a pose link of the plan is held at a per-trajectory
// target at one interior waypoint.  The walk of traj_penalty also yields the link's frame; the residual norms of
// lane wp enter the merit; after the Minv g pass the segment's lanes each redo the walk at the broadcast x_wp and
// solve the 6 x 6 system of the constrained update (traj_pose_newton).  No barrier and no LDS beyond POSE = false.
//
// TREE = true (kin_traj_opt_tree_batch, common bounds 8 and 16): the POSE = false loop with the sphere sum of the merit
// and its half-gradient taken over every part of a multi-chain plan: a lane walks part after part in plan order, the
// walk state of a part dead before the next one starts.  Always ND = kTrajNdLarge columns; ndof is a kernel argument.
//
// POSE and TREE (kin_traj_opt_pose_tree_batch, k_traj_pose_tree in kinhip_traj_pose_tree.hip): the pose link rides on
// part tp.part of the table: that part's walk captures its frame, the Newton walk runs on that part's program.
//
// SCENE != 0 (kin_traj_opt_scene_batch, k_traj_scene in kinhip_traj_scene.hip; TREE only): the union's boxes are
// attached to a scene mechanism of at most SCENE moving groups and every waypoint has its own scene state: the lane
// forms its group frames once (scene_frames at its own sample offset, held in registers over the descent) and its
// spheres go through scene_union instead of union_sdf.  The scene is data: nothing is differentiated through it.
#pragma once
#include "kinhip_coll_dev.h"
#include "kinhip_ik_dev.h"  // rot_error (the POSE variant's rotation residual)

namespace kinhip {
namespace {

// q columns (+ base) a lane keeps in registers, by the chain bound of the plan
template <int MAXA>
struct TrajNd {
    static constexpr int v = MAXA <= 8 ? kTrajNdSmall : kTrajNdLarge;
};

// butterflies within a segment of L lanes (segments are L-aligned, so lane ^ m stays inside): every lane
// of the segment ends with the same bits (a + b == b + a)
template <int L, typename T>
__device__ __forceinline__ T seg_sum(T v) {
#pragma unroll
    for (int m = L / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
template <int L, typename T>
__device__ __forceinline__ T seg_min(T v) {
#pragma unroll
    for (int m = L / 2; m >= 1; m >>= 1) v = fmin(v, __shfl_xor(v, m));
    return v;
}
template <int L, typename T>
__device__ __forceinline__ T seg_max(T v) {
#pragma unroll
    for (int m = L / 2; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m));
    return v;
}

// x[c] for a uniform column c (a select chain: the array stays in registers)
template <typename T, int ND>
__device__ __forceinline__ T pick_col(const T (&x)[ND], int c) {
    T v = T(0);
#pragma unroll
    for (int k = 0; k < ND; ++k) v = (c == k) ? x[k] : v;
    return v;
}

// Penalty part of the merit at one waypoint x (all ND columns; columns past the plan's are 0):
//   pen  = sum_s r_s^2,  r_s = weight * max(0, trunc - d_s)      (0 unless `interior`)
//   g[c] = - sum_s weight * r_s * d(d_s)/d(q_c)                  (the half-gradient of pen)
//   dmin = min_s d_s                                             (+inf unless `interior`)
// d_s = sdf(centre_s) - radius_s with k_coll's analytic gradient (coll_spheres::finish's columns).
// traj_penalty's hook: called with the root (base) frame (s = -1) and with every step's post-motion frame.
// kin_traj_opt_batch's walk has none; the POSE variant captures the frame that carries its pose link.
struct TrajNoHook {
    template <typename F>
    __device__ __forceinline__ void operator()(int, const F&) const {}
};
template <typename T>
struct TrajFrameAt {
    int step;
    Fr<T>& out;
    __device__ __forceinline__ void operator()(int s, const Fr<T>& f) const {
        if (s == step) out = f;  // (uniform)
    }
};

template <typename T, int MAXA, int ND, typename Hook = TrajNoHook, int SCENE = 0>
__device__ __forceinline__ void traj_penalty(const KProg<T>& P, const KStep<T>* __restrict__ S,
                                             const KSphere<T>* __restrict__ sph, const KBox<T>* __restrict__ boxes,
                                             const KAabb<T>* __restrict__ aabb, int na, int nb,
                                             const unsigned char* smem, bool use_lds, const T (&x)[ND], bool interior,
                                             T trunc, T weight, T (&g)[ND], T& pen, T& dmin,
                                             Hook hook = Hook(),  // (by value: a reference's temporary changed k_traj's code)
                                             const SceneCtx<T, SCENE ? SCENE : 1>* sc = nullptr) {  // (SCENE != 0 only)
    const bool base = (P.flags & PF_BASE) != 0;
    T bx = T(0), by = T(0), bth = T(0);
    if (base) {
        bx = pick_col(x, P.base_col);
        by = pick_col(x, P.base_col + 1);
        bth = pick_col(x, P.base_col + 2);
    }
    T qa[MAXA];
#pragma unroll
    for (int s = 0; s < MAXA; ++s) qa[s] = S[s].qcol >= 0 ? pick_col(x, S[s].qcol) : T(0);
    Fr<T> f;
    if (base) base_frame(f, bx, by, bth);
    else set_identity(f);
    T rm[MAXA][3], rz[MAXA][3], gs[MAXA], gb[3] = {T(0), T(0), T(0)};
#pragma unroll
    for (int s = 0; s < MAXA; ++s) {
        rm[s][0] = rm[s][1] = rm[s][2] = T(0);
        rz[s][0] = rz[s][1] = rz[s][2] = T(0);
        gs[s] = T(0);
    }
    pen = T(0);
    dmin = T(INFINITY);
    auto sphere = [&](int s_last, const KSphere<T>& sp) {
        T px[1], py[1], pz[1], ds[1] = {T(0)}, gw[1][3] = {{T(0), T(0), T(0)}};
        px[0] = fma(f.r[0], sp.c[0], fma(f.r[1], sp.c[1], fma(f.r[2], sp.c[2], f.t[0])));
        py[0] = fma(f.r[3], sp.c[0], fma(f.r[4], sp.c[1], fma(f.r[5], sp.c[2], f.t[1])));
        pz[0] = fma(f.r[6], sp.c[0], fma(f.r[7], sp.c[1], fma(f.r[8], sp.c[2], f.t[2])));
        if constexpr (SCENE != 0) scene_union<T, true, 1, SCENE>(*sc, boxes, aabb, px, py, pz, ds, gw, smem, use_lds);
        else union_sdf<T, true, 1>(boxes, aabb, na, nb, px, py, pz, ds, gw, smem, use_lds);
        const T d = ds[0] - sp.r;
        const T r = interior ? weight * fmax(T(0), trunc - d) : T(0);
        dmin = interior ? fmin(dmin, d) : dmin;
        pen = fma(r, r, pen);
        const T cf = weight * r;  // 0 outside the band: the columns below add nothing
        const T g0 = gw[0][0], g1 = gw[0][1], g2 = gw[0][2];
        // column j = g . (z_j x (p - o_j)) = z_j . (p x g) - g . m_j, m_j = z_j x o_j (as k_coll)
        const T w0 = fma(py[0], g2, -(pz[0] * g1)), w1 = fma(pz[0], g0, -(px[0] * g2)), w2 = fma(px[0], g1, -(py[0] * g0));
#pragma unroll
        for (int j = 0; j < MAXA; ++j) {
            if (j <= s_last && (S[j].flags & SF_REC)) {
                T v;
                if (S[j].jkind == MOT_PRISM)
                    v = fma(g0, rz[j][0], fma(g1, rz[j][1], g2 * rz[j][2]));
                else
                    v = fma(rz[j][0], w0, fma(rz[j][1], w1, fma(rz[j][2], w2,
                            -fma(g0, rm[j][0], fma(g1, rm[j][1], g2 * rm[j][2])))));
                gs[j] = fma(-cf, v, gs[j]);
            }
        }
        if (base) {  // base columns [1 0 -y; 0 1 x; 0 0 0] (src/algorithm.jl:98-103)
            gb[0] = fma(-cf, g0, gb[0]);
            gb[1] = fma(-cf, g1, gb[1]);
            gb[2] = fma(-cf, fma(-g0, py[0] - by, g1 * (px[0] - bx)), gb[2]);
        }
    };
    hook(-1, f);
    for (int k = P.sph_root0; k < P.sph_root1; ++k) sphere(-1, sph[k]);
#pragma unroll
    for (int s = 0; s < MAXA; ++s) {
        step_a<T, KINHIP_COLL_FAST_TRIG != 0>(f, S[s], qa[s], rm[s], rz[s]);  // (fp32: k_coll's trig)
        const T o0 = rm[s][0], o1 = rm[s][1], o2 = rm[s][2];  // m_s = z_s x o_s
        rm[s][0] = fma(rz[s][1], o2, -(rz[s][2] * o1));
        rm[s][1] = fma(rz[s][2], o0, -(rz[s][0] * o2));
        rm[s][2] = fma(rz[s][0], o1, -(rz[s][1] * o0));
        for (int k = S[s].sph0; k < S[s].sph1; ++k) sphere(s, sph[k]);
        hook(s, f);
    }
    // the steps' sums to their q columns (uniform masks)
#pragma unroll
    for (int k = 0; k < ND; ++k) g[k] = T(0);
#pragma unroll
    for (int j = 0; j < MAXA; ++j) {
        const uint64_t m = (S[j].flags & SF_REC) ? S[j].colmask : 0;
#pragma unroll
        for (int k = 0; k < ND; ++k) g[k] = ((m >> k) & 1) ? g[k] + gs[j] : g[k];
    }
    if (base) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < ND; ++k) g[k] = (P.base_col + i == k) ? g[k] + gb[i] : g[k];
    }
}

// ---- the POSE variant (kin_traj_opt_pose_batch): one pose link held at a target at waypoint tp.wp ----

// Residual of the pose link carried by chain frame C: r = [p - p*; -log(R* R^T)] (rot_error, k_ik_dls's world
// axis-angle vector; rows 3..5 are 0 for a position-only constraint) and the link's position p.
// tg: the target, 3x4 column-major.
template <typename T>
__device__ __forceinline__ void traj_pose_residual(const Fr<T>& C, const TrajPose<T>& tp, const T (&tg)[12], T (&r)[6],
                                                   T (&p)[3]) {
    Fr<T> Lf;
    link_frame(Lf, C, true, tp.X);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        p[i] = Lf.t[i];
        r[i] = Lf.t[i] - tg[9 + i];
        r[3 + i] = T(0);
    }
    if (tp.with_rot) {  // uniform
        T Rt[9], w[3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) Rt[3 * a + b] = tg[a + 3 * b];
        rot_error(Rt, Lf.r, w);
#pragma unroll
        for (int i = 0; i < 3; ++i) r[3 + i] = -w[i];
    }
}

template <typename T>
__device__ __forceinline__ void traj_pose_norms(const T (&r)[6], T& rp, T& rr) {
    rp = sqrt_t(fma(r[0], r[0], fma(r[1], r[1], r[2] * r[2])));
    rr = sqrt_t(fma(r[3], r[3], fma(r[4], r[4], r[5] * r[5])));
}

// The Newton correction of the constrained waypoint: with r and the geometric Jacobian J (6 x n_dof; rotation rows
// 0 for a position-only constraint) at xc,  S = J W^-1 J^T + damp I,  v = S^-1 (-r - J rawc),  u = W^-1 J^T v.
// xc and rawc are a segment's broadcast values, so every lane of it computes the same u bit for bit.  J's columns
// [z_j x (p - o_j); z_j] ([z_j; 0] prismatic; the base columns of src/algorithm.jl:98-103) are formed on the fly
// from the walk's axis and moment vectors, as traj_penalty's sphere gradient does; S is 6 x 6 symmetric positive
// definite (its rotation block the identity for a position-only constraint): unrolled Cholesky, no pivoting.
template <typename T, int MAXA, int ND>
__device__ __forceinline__ void traj_pose_newton(const KProg<T>& P, const KStep<T>* __restrict__ S,
                                                 const TrajPose<T>& tp, const T (&tg)[12], const TrajDof& dof,
                                                 const T (&xc)[ND], const T (&rawc)[ND], T (&u)[ND]) {
    const bool base = (P.flags & PF_BASE) != 0, wr = tp.with_rot != 0;
    T bx = T(0), by = T(0), bth = T(0);
    if (base) {
        bx = pick_col(xc, P.base_col);
        by = pick_col(xc, P.base_col + 1);
        bth = pick_col(xc, P.base_col + 2);
    }
    Fr<T> f;
    if (base) base_frame(f, bx, by, bth);
    else set_identity(f);
    Fr<T> Cf = f;  // (tp.step = -1: the root frame)
    T rm[MAXA][3], rz[MAXA][3];
#pragma unroll
    for (int s = 0; s < MAXA; ++s) {
        const T qs = S[s].qcol >= 0 ? pick_col(xc, S[s].qcol) : T(0);
        step_a<T, KINHIP_COLL_FAST_TRIG != 0>(f, S[s], qs, rm[s], rz[s]);
        const T o0 = rm[s][0], o1 = rm[s][1], o2 = rm[s][2];  // m_s = z_s x o_s
        rm[s][0] = fma(rz[s][1], o2, -(rz[s][2] * o1));
        rm[s][1] = fma(rz[s][2], o0, -(rz[s][0] * o2));
        rm[s][2] = fma(rz[s][0], o1, -(rz[s][1] * o0));
        if (s == tp.step) Cf = f;  // uniform
    }
    T r[6], p[3];
    traj_pose_residual(Cf, tp, tg, r, p);
    // column of step j: z_j x p - m_j
    auto jcol = [&](int j, T (&Jc)[6]) {
        if (S[j].jkind == MOT_PRISM) {
            Jc[0] = rz[j][0]; Jc[1] = rz[j][1]; Jc[2] = rz[j][2];
            Jc[3] = Jc[4] = Jc[5] = T(0);
        } else {
            Jc[0] = fma(rz[j][1], p[2], -(rz[j][2] * p[1])) - rm[j][0];
            Jc[1] = fma(rz[j][2], p[0], -(rz[j][0] * p[2])) - rm[j][1];
            Jc[2] = fma(rz[j][0], p[1], -(rz[j][1] * p[0])) - rm[j][2];
            Jc[3] = wr ? rz[j][0] : T(0); Jc[4] = wr ? rz[j][1] : T(0); Jc[5] = wr ? rz[j][2] : T(0);
        }
    };
    auto bcol = [&](int i, T (&Jc)[6]) {  // base x, y, theta
#pragma unroll
        for (int k = 0; k < 6; ++k) Jc[k] = T(0);
        if (i == 0) Jc[0] = T(1);
        if (i == 1) Jc[1] = T(1);
        if (i == 2) {
            Jc[0] = -(p[1] - by);
            Jc[1] = p[0] - bx;
            Jc[5] = wr ? T(1) : T(0);
        }
    };
    // A: the lower triangle of S, row by row (A[i (i + 1) / 2 + j], j <= i); b = -r - J rawc
    T A[21], b[6];
#pragma unroll
    for (int k = 0; k < 21; ++k) A[k] = T(0);
#pragma unroll
    for (int i = 0; i < 6; ++i) b[i] = -r[i];
    auto accumulate = [&](const T (&Jc)[6], T wj, T rj) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const T wi = wj * Jc[i];
#pragma unroll
            for (int j = 0; j <= i; ++j) A[i * (i + 1) / 2 + j] = fma(wi, Jc[j], A[i * (i + 1) / 2 + j]);
            b[i] = fma(-Jc[i], rj, b[i]);
        }
    };
#pragma unroll
    for (int j = 0; j < MAXA; ++j) {
        if (j <= tp.step && (S[j].flags & SF_REC)) {  // uniform
            const uint64_t m = S[j].colmask;
            T wj = T(0), rj = T(0);
#pragma unroll
            for (int k = 0; k < ND; ++k) {
                wj = ((m >> k) & 1) ? wj + (T)dof.iW[k] : wj;
                rj = ((m >> k) & 1) ? rj + rawc[k] : rj;
            }
            T Jc[6];
            jcol(j, Jc);
            accumulate(Jc, wj, rj);
        }
    }
    if (base) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            T Jc[6];
            bcol(i, Jc);
            T wb = T(0);  // (a select chain: the kernel argument is never indexed by a run-time value)
#pragma unroll
            for (int k = 0; k < ND; ++k) wb = (P.base_col + i == k) ? (T)dof.iW[k] : wb;
            accumulate(Jc, wb, pick_col(rawc, P.base_col + i));
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        A[i * (i + 1) / 2 + i] += tp.damp;
        if (i >= 3 && !wr) A[i * (i + 1) / 2 + i] = T(1);  // (its rows and b are 0: v_rot = 0)
    }
    // Cholesky S = L L^T in place, then L y = b, L^T v = y
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        T d = A[j * (j + 1) / 2 + j];
#pragma unroll
        for (int q = 0; q < j; ++q) d = fma(-A[j * (j + 1) / 2 + q], A[j * (j + 1) / 2 + q], d);
        d = sqrt_t(d);
        A[j * (j + 1) / 2 + j] = d;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            T a = A[i * (i + 1) / 2 + j];
#pragma unroll
            for (int q = 0; q < j; ++q) a = fma(-A[i * (i + 1) / 2 + q], A[j * (j + 1) / 2 + q], a);
            A[i * (i + 1) / 2 + j] = a / d;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        T a = b[i];
#pragma unroll
        for (int q = 0; q < i; ++q) a = fma(-A[i * (i + 1) / 2 + q], b[q], a);
        b[i] = a / A[i * (i + 1) / 2 + i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        T a = b[i];
#pragma unroll
        for (int q = i + 1; q < 6; ++q) a = fma(-A[q * (q + 1) / 2 + i], b[q], a);
        b[i] = a / A[i * (i + 1) / 2 + i];
    }
    // u = W^-1 J^T v, the steps' dot products scattered to their q columns (uniform masks)
#pragma unroll
    for (int k = 0; k < ND; ++k) u[k] = T(0);
#pragma unroll
    for (int j = 0; j < MAXA; ++j) {
        if (j <= tp.step && (S[j].flags & SF_REC)) {  // uniform
            T Jc[6];
            jcol(j, Jc);
            const T tj = fma(Jc[0], b[0], fma(Jc[1], b[1], fma(Jc[2], b[2], fma(Jc[3], b[3], fma(Jc[4], b[4], Jc[5] * b[5])))));
            const uint64_t m = S[j].colmask;
#pragma unroll
            for (int k = 0; k < ND; ++k) u[k] = ((m >> k) & 1) ? u[k] + tj : u[k];
        }
    }
    if (base) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            T Jc[6];
            bcol(i, Jc);
            const T tj = fma(Jc[0], b[0], fma(Jc[1], b[1], Jc[5] * b[5]));
#pragma unroll
            for (int k = 0; k < ND; ++k) u[k] = (P.base_col + i == k) ? u[k] + tj : u[k];
        }
    }
#pragma unroll
    for (int k = 0; k < ND; ++k) u[k] *= (T)dof.iW[k];
}

// P, S, sph: the chain (not TREE); tp, targets, ldt: POSE only (tp->part: TREE); parts, n_parts, nd (q columns + base): TREE only;
// sa: SCENE != 0 only (its q already at the launch chunk's first sample)
template <typename T, int MAXA, int L, bool POSE = false, bool TREE = false, int SCENE = 0>
__device__ __forceinline__ void traj_body(const KProg<T>& P, const KStep<T>* __restrict__ S,
                                          const KSphere<T>* __restrict__ sph, const KBox<T>* __restrict__ boxes,
                                          const CollArgs& a, const TrajArgs& ta, const TrajDof& dof,
                                          const T* __restrict__ minvT, T* __restrict__ xi, int64_t ldx, int64_t n_traj,
                                          int32_t* __restrict__ iters, T* __restrict__ info, int64_t ldi,
                                          unsigned char* smem, const TrajPose<T>* __restrict__ tp = nullptr,
                                          const T* __restrict__ targets = nullptr, int64_t ldt = 0,
                                          const TrajPart<T>* __restrict__ parts = nullptr, int n_parts = 0, int nd = 0,
                                          const SceneArgs<T>* sa = nullptr) {
    static_assert(SCENE == 0 || TREE, "the scene variant is the part loop's");
    constexpr int ND = TREE ? kTrajNdLarge : TrajNd<MAXA>::v;
    const int n_wp = ta.n_wp, ni = n_wp - 2;
    const int ndof = TREE ? nd : P.n_jac + ((P.flags & PF_BASE) ? 3 : 0);
    // LDS: [the union's boxes (as k_coll) | Minv^T, ni x ni | g, one row of ndof per lane]
    const bool use_lds = a.n_boxes <= kCollLdsBoxes;  // uniform
    const int box_bytes = use_lds ? a.n_boxes * (int)sizeof(KBox<T>) : 0;
    T* __restrict__ mt = reinterpret_cast<T*>(smem + box_bytes);
    T* __restrict__ gl = mt + ni * ni;
    if (use_lds) {
        const int words = a.n_boxes * (int)(sizeof(KBox<T>) / 16);
        for (int w = (int)threadIdx.x; w < words; w += (int)blockDim.x)
            reinterpret_cast<uint4*>(smem)[w] = reinterpret_cast<const uint4*>(boxes)[w];
    }
    for (int k = (int)threadIdx.x; k < ni * ni; k += (int)blockDim.x) mt[k] = minvT[k];
    __syncthreads();  // the only workgroup barrier: from here on a wave works on its own LDS rows

    const int64_t gt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t t = gt / L;  // trajectory of this segment
    const int w = (int)(gt % L);
    if (__all(t >= n_traj)) return;  // (a whole wave: no lane of it has work)
    const bool valid = t < n_traj && w < n_wp;
    const bool interior = valid && w >= 1 && w <= n_wp - 2;
    const uint32_t off = valid ? (uint32_t)((t * n_wp + w) * (int64_t)sizeof(T)) : 0u;
    const KAabb<T>* aabb = reinterpret_cast<const KAabb<T>*>(boxes + a.n_boxes);
    // SCENE: this waypoint's group frames, once (the scene does not change during the solve); lanes without a
    // waypoint take sample 0 of the chunk (off = 0: in range)
    SceneCtx<T, SCENE ? SCENE : 1> sc;
    if constexpr (SCENE != 0) scene_frames(sc, *sa, off);

    const T trunc = (T)(ta.margin + ta.band), weight = (T)ta.weight;
    const T feas_d = (T)(ta.margin - ta.feas), ftol = (T)ta.ftol, max_step = (T)ta.max_step;

    T x[ND], xn[ND], g[ND], gn[ND];
#pragma unroll
    for (int k = 0; k < ND; ++k) {
        x[k] = T(0);
        if (k < ndof && valid) x[k] = ld_soa(xi, k, ldx, off);
        xn[k] = x[k];
        g[k] = T(0);
    }
    T alpha = T(1), f = T(0), fsm = T(0), dcur = T(INFINITY);
    bool fin = !(t < n_traj);  // segments without a trajectory never hold the wave in its loop
    int it_done = ta.max_iters + 1, nacc = 0;
    const int lane = (int)threadIdx.x;
    const int seg0 = lane - w;            // first lane (workgroup-relative) of this segment
    const int wi = min(max(w - 1, 0), ni - 1);  // this lane's row of Minv (clamped: masked below)
    // POSE: the segment's target, the residual norms of the accepted state (per-segment values, as f)
    T tg[12], rpc = T(0), rrc = T(0);
    if constexpr (POSE) {
#pragma unroll
        for (int k = 0; k < 12; ++k) tg[k] = t < n_traj ? targets[k * ldt + t] : T(0);
    }

    for (int it = 0;; ++it) {
        // ---- the merit and its half-gradient at xn ----
        T pen, dmin;
        T rpn = T(0), rrn = T(0);  // POSE: |r_p|, |r_rot| of the segment's candidate
        if constexpr (POSE && !TREE) {
            Fr<T> Cf;
            set_identity(Cf);
            traj_penalty<T, MAXA, ND>(P, S, sph, boxes, aabb, a.n_aabb, a.n_boxes, smem, use_lds, xn, interior, trunc,
                                      weight, gn, pen, dmin, TrajFrameAt<T>{tp->step, Cf});
            T r[6], pl[3];
            traj_pose_residual(Cf, *tp, tg, r, pl);
            traj_pose_norms(r, rpn, rrn);
            rpn = __shfl(rpn, tp->wp, L);  // lane wp of the segment holds the constrained waypoint
            rrn = __shfl(rrn, tp->wp, L);
        } else if constexpr (TREE) {
            // every part's steps are padded to MAXA in the table: the unrolled walk never reads past a staged program; each
            // part recomputes the base frame and the spheres (root-frame ones too) are disjoint: nothing is counted twice
            pen = T(0);
            dmin = T(INFINITY);
#pragma unroll
            for (int k = 0; k < ND; ++k) gn[k] = T(0);
            Fr<T> Cf;  // POSE: the frame that carries the pose link, from the walk of part tp->part
            if constexpr (POSE) set_identity(Cf);
            for (int p = 0; p < n_parts; ++p) {  // (uniform; the chain inside stays unrolled)
                const TrajPart<T>& pt = parts[p];
                const char* tab = reinterpret_cast<const char*>(parts);  // (offsets from the kernel argument: global loads)
                const KStep<T>* __restrict__ Sp = reinterpret_cast<const KStep<T>*>(tab + pt.steps_off);
                const KSphere<T>* __restrict__ sp = reinterpret_cast<const KSphere<T>*>(tab + pt.sph_off);
                T gp[ND], penp, dminp;
                if constexpr (POSE) {
                    // one call site: the hook's step is -2 (no frame of the walk) on the parts without the pose link
                    const TrajFrameAt<T> hook{p == tp->part ? tp->step : -2, Cf};  // (uniform)
                    if constexpr (SCENE != 0)
                        traj_penalty<T, MAXA, ND, TrajFrameAt<T>, SCENE>(pt.P, Sp, sp, boxes, aabb, a.n_aabb, a.n_boxes,
                                                                         smem, use_lds, xn, interior, trunc, weight, gp,
                                                                         penp, dminp, hook, &sc);
                    else
                        traj_penalty<T, MAXA, ND, TrajFrameAt<T>>(pt.P, Sp, sp, boxes, aabb, a.n_aabb, a.n_boxes, smem,
                                                                  use_lds, xn, interior, trunc, weight, gp, penp, dminp,
                                                                  hook);
                } else if constexpr (SCENE != 0)
                    traj_penalty<T, MAXA, ND, TrajNoHook, SCENE>(pt.P, Sp, sp, boxes, aabb, a.n_aabb, a.n_boxes, smem,
                                                                 use_lds, xn, interior, trunc, weight, gp, penp, dminp,
                                                                 TrajNoHook(), &sc);
                else
                    traj_penalty<T, MAXA, ND>(pt.P, Sp, sp, boxes, aabb, a.n_aabb, a.n_boxes, smem, use_lds, xn, interior,
                                              trunc, weight, gp, penp, dminp);
#pragma unroll
                for (int k = 0; k < ND; ++k) gn[k] += gp[k];
                pen += penp;
                dmin = fmin(dmin, dminp);
            }
            if constexpr (POSE) {  // once per iteration, after the part loop (the scene never enters the pose term)
                T r[6], pl[3];
                traj_pose_residual(Cf, *tp, tg, r, pl);
                traj_pose_norms(r, rpn, rrn);
                rpn = __shfl(rpn, tp->wp, L);
                rrn = __shfl(rrn, tp->wp, L);
            }
        } else {
            traj_penalty<T, MAXA, ND>(P, S, sph, boxes, aabb, a.n_aabb, a.n_boxes, smem, use_lds, xn, interior, trunc,
                                      weight, gn, pen, dmin);
        }
        T sm = T(0);
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            if (k >= ndof) continue;  // uniform
            // a_w = x_{w-1} - 2 x_w + x_{w+1} at interior waypoints (0 elsewhere); (A x)_w = a_{w-1} - 2 a_w + a_{w+1}
            const T xm = __shfl_up(xn[k], 1), xp = __shfl_down(xn[k], 1);
            const T aw = interior ? (xm - T(2) * xn[k]) + xp : T(0);
            const T am = __shfl_up(aw, 1), ap = __shfl_down(aw, 1);
            const T ax = (am - T(2) * aw) + ap;
            const T Wk = (T)dof.W[k];
            gn[k] = interior ? fma(Wk, ax, gn[k]) : T(0);
            sm = fma(Wk * aw, aw, sm);
        }
        T fl = sm + pen;
        if constexpr (POSE) fl = (w == tp->wp) ? fl + tp->nu * (rpn + rrn) : fl;  // the exact penalty, on lane wp
        const T fn = seg_sum<L>(fl);
        const T smn = seg_sum<L>(sm);
        const T dn = seg_min<L>(dmin);
        // ---- accept / reject (per segment: every lane of it holds the same values) ----
        const bool live = !fin;
        const bool acc = it == 0 ? true : (live && fn <= f);
        const bool rej = it > 0 && live && !acc;
        bool done = it > 0 && acc && (f - fn < ftol) && (dn >= feas_d);
        if constexpr (POSE) {
            done = done && rpn < tp->tol_pos && rrn < tp->tol_rot;
            rpc = acc ? rpn : rpc;
            rrc = acc ? rrn : rrc;
        }
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            x[k] = acc ? xn[k] : x[k];
            g[k] = acc ? gn[k] : g[k];
        }
        f = acc ? fn : f;
        fsm = acc ? smn : fsm;
        dcur = acc ? dn : dcur;
        if (it > 0) {
            nacc += acc ? 1 : 0;
            alpha = acc ? fmin(T(1), T(2) * alpha) : (rej ? T(0.25) * alpha : alpha);
            fin = fin || done || (rej && alpha < T(1e-6));
            it_done = done ? it : it_done;
        }
        if (it >= ta.max_iters || __all(fin)) break;
        // ---- covariant step: -alpha W^-1 Minv g over the interior waypoints, through LDS ----
#pragma unroll
        for (int k = 0; k < ND; ++k)
            if (k < ndof) gl[lane * ndof + k] = g[k];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        T st[ND];
#pragma unroll
        for (int k = 0; k < ND; ++k) st[k] = T(0);
        for (int v = 0; v < ni; ++v) {
            const T mv = mt[v * ni + wi];  // Minv[w-1][v] (symmetric), consecutive over the segment's lanes
            const T* __restrict__ gr = gl + (seg0 + 1 + v) * ndof;
#pragma unroll
            for (int k = 0; k < ND; ++k)
                if (k < ndof) st[k] = fma(mv, gr[k], st[k]);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        T mx = T(0);
        if constexpr (POSE) {
            // ---- raw step, then its projection onto the linearised constraint plus the Newton correction of the
            // constrained waypoint, spread by the metric's column wp-1 (every lane of a segment: the same u) ----
            T xc[ND], rawc[ND], u[ND];
#pragma unroll
            for (int k = 0; k < ND; ++k) {
                st[k] = interior && k < ndof ? -(alpha * (st[k] * (T)dof.iW[k])) : T(0);
                xc[k] = rawc[k] = T(0);
                if (k >= ndof) continue;  // uniform
                xc[k] = __shfl(x[k], tp->wp, L);
                rawc[k] = __shfl(st[k], tp->wp, L);
            }
            if constexpr (TREE) {  // the program of the part that carries the pose link (offsets from the kernel argument)
                const TrajPart<T>& pt = parts[tp->part];
                const KStep<T>* __restrict__ Sp =
                    reinterpret_cast<const KStep<T>*>(reinterpret_cast<const char*>(parts) + pt.steps_off);
                traj_pose_newton<T, MAXA, ND>(pt.P, Sp, *tp, tg, dof, xc, rawc, u);
            } else {
                traj_pose_newton<T, MAXA, ND>(P, S, *tp, tg, dof, xc, rawc, u);
            }
            const int ci = tp->wp - 1;
            const T ratio = mt[ci * ni + wi] / mt[ci * ni + ci];
#pragma unroll
            for (int k = 0; k < ND; ++k) st[k] = interior && k < ndof ? fma(ratio, u[k], st[k]) : T(0);
        }
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            if constexpr (!POSE) st[k] = interior && k < ndof ? -(alpha * (st[k] * (T)dof.iW[k])) : T(0);
            mx = fmax(mx, fabs(st[k]));
        }
        mx = seg_max<L>(mx);
        const T scale = mx > max_step ? max_step / mx : T(1);
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            const T c = fmin(fmax(x[k] + st[k] * scale, (T)dof.lo[k]), (T)dof.hi[k]);
            xn[k] = (interior && !fin) ? c : x[k];
        }
    }
    // ---- results: interior waypoints only (the end columns are never written) ----
    if (interior) {
#pragma unroll
        for (int k = 0; k < ND; ++k)
            if (k < ndof) st_soa(xi, k, ldx, off, x[k]);
    }
    if (valid && w == 0) {
        if (iters) iters[t] = it_done;
        if (info) {
            info[t] = f;
            info[ldi + t] = fsm;
            info[2 * ldi + t] = dcur;
            info[3 * ldi + t] = (T)nacc;
            if constexpr (POSE) {
                info[4 * ldi + t] = rpc;
                info[5 * ldi + t] = rrc;
            }
        }
    }
}

// host side of the SCENE != 0 kernels: the scene arguments of one chunk of launch_traj's loop, sample0 the chunk's
// first sample (t0 * n_wp, as xi); uniform: the scene values are one column of cols entries
template <typename T>
SceneArgs<T> traj_scene_args(const SceneLaunch& s, int64_t sample0) {
    SceneArgs<T> sa;
    sa.groups = (const KSceneGroup*)s.groups;
    sa.steps = (const KSceneStep<T>*)s.steps;
    sa.q = (const T*)s.q + (s.uniform ? 0 : sample0);
    sa.ld = s.uniform ? 1 : s.ld;
    sa.ng = s.ng;
    sa.base_col = s.base_col;
    sa.uniform = s.uniform;
    return sa;
}

}  // namespace
}  // namespace kinhip
