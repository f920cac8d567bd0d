// kinhip_traj_dev.h -- device body of k_traj: batched trajectory optimisation (kin_traj_opt_batch).
// Included by kinhip_traj.hip only (no run-time specialisation: not part of the embedded sources).
// gfx950 only.
//
// Many independent trajectories of n_wp waypoints per launch, one lane per waypoint, each trajectory
// in a wave segment of L = 8 / 16 / 32 / 64 lanes (the smallest L >= n_wp).  Per iteration a lane
// walks the sphere chain of its own waypoint (step_a / union_sdf / box_gradient of k_coll) and keeps
// the penalty half-gradient, the penalty sum and the minimum distance in registers; the second
// differences of the smoothness objective (src/planning.jl:1-28) come from the neighbour lanes; the
// covariant step Minv g goes through LDS; the line-search decisions are per-segment values held by
// every lane of the segment (selects, never a divergent branch around a cross-lane operation).
#pragma once
#include "kinhip_coll_dev.h"

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
template <typename T, int MAXA, int ND>
__device__ __forceinline__ void traj_penalty(const KProg<T>& P, const KStep<T>* __restrict__ S,
                                             const KSphere<T>* __restrict__ sph, const KBox<T>* __restrict__ boxes,
                                             const KAabb<T>* __restrict__ aabb, int na, int nb,
                                             const unsigned char* smem, bool use_lds, const T (&x)[ND], bool interior,
                                             T trunc, T weight, T (&g)[ND], T& pen, T& dmin) {
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
        union_sdf<T, true, 1>(boxes, aabb, na, nb, px, py, pz, ds, gw, smem, use_lds);
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
    for (int k = P.sph_root0; k < P.sph_root1; ++k) sphere(-1, sph[k]);
#pragma unroll
    for (int s = 0; s < MAXA; ++s) {
        step_a<T, KINHIP_COLL_FAST_TRIG != 0>(f, S[s], qa[s], rm[s], rz[s]);  // (fp32: k_coll's trig)
        const T o0 = rm[s][0], o1 = rm[s][1], o2 = rm[s][2];  // m_s = z_s x o_s
        rm[s][0] = fma(rz[s][1], o2, -(rz[s][2] * o1));
        rm[s][1] = fma(rz[s][2], o0, -(rz[s][0] * o2));
        rm[s][2] = fma(rz[s][0], o1, -(rz[s][1] * o0));
        for (int k = S[s].sph0; k < S[s].sph1; ++k) sphere(s, sph[k]);
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

template <typename T, int MAXA, int L>
__device__ __forceinline__ void traj_body(const KProg<T>& P, const KStep<T>* __restrict__ S,
                                          const KSphere<T>* __restrict__ sph, const KBox<T>* __restrict__ boxes,
                                          const CollArgs& a, const TrajArgs& ta, const TrajDof& dof,
                                          const T* __restrict__ minvT, T* __restrict__ xi, int64_t ldx, int64_t n_traj,
                                          int32_t* __restrict__ iters, T* __restrict__ info, int64_t ldi,
                                          unsigned char* smem) {
    constexpr int ND = TrajNd<MAXA>::v;
    const int n_wp = ta.n_wp, ni = n_wp - 2;
    const int ndof = P.n_jac + ((P.flags & PF_BASE) ? 3 : 0);
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

    for (int it = 0;; ++it) {
        // ---- the merit and its half-gradient at xn ----
        T pen, dmin;
        traj_penalty<T, MAXA, ND>(P, S, sph, boxes, aabb, a.n_aabb, a.n_boxes, smem, use_lds, xn, interior, trunc, weight,
                                  gn, pen, dmin);
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
        const T fn = seg_sum<L>(sm + pen);
        const T smn = seg_sum<L>(sm);
        const T dn = seg_min<L>(dmin);
        // ---- accept / reject (per segment: every lane of it holds the same values) ----
        const bool live = !fin;
        const bool acc = it == 0 ? true : (live && fn <= f);
        const bool rej = it > 0 && live && !acc;
        const bool done = it > 0 && acc && (f - fn < ftol) && (dn >= feas_d);
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
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            st[k] = interior && k < ndof ? -(alpha * (st[k] * (T)dof.iW[k])) : T(0);
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
        }
    }
}

}  // namespace
}  // namespace kinhip
