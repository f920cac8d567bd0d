// kinhip_trajopt.cpp -- C-ABI of the batched trajectory optimiser: kin_traj_opt_batch (k_traj,
// kinhip_traj.hip), kin_traj_opt_pose_batch (its POSE variant: one pose link held at a waypoint),
// kin_traj_opt_tree_batch (k_traj_tree: spheres on several chains), kin_traj_opt_scene_batch (k_traj_scene: the
// union attached to a scene, one scene state per waypoint), kin_traj_opt_pose_tree_batch (k_traj_pose_tree: the pose
// link on either of the two) and their metric table.
//
// Reference semantics restated here (host side):
//   Objective's A_sub (finite-difference accelerations)    src/planning.jl:1-28
//   the two end ConfigurationConstraints of a problem      src/planning.jl:310-330
#include <cmath>
#include <functional>
#include <string>
#include <vector>

#include "kinhip_plan.h"

namespace kinhip {
namespace {

// (A_sub[I,I])^-1 for n_wp waypoints, I the interior ones: Gauss-Jordan on the symmetric positive
// definite pentadiagonal block (no pivoting needed), accumulated in long double
void traj_metric_inverse(int n_wp, double* out) {
    const int n = n_wp - 2;
    std::vector<long double> A((size_t)n_wp * n_wp, 0.0L);
    const long double blk[3] = {1.0L, -2.0L, 1.0L};
    for (int i = 1; i < n_wp - 1; ++i)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) A[(size_t)(i - 1 + r) * n_wp + (i - 1 + c)] += blk[r] * blk[c];
    std::vector<long double> M((size_t)n * 2 * n, 0.0L);  // [A_II | 1]
    for (int r = 0; r < n; ++r) {
        for (int c = 0; c < n; ++c) M[(size_t)r * 2 * n + c] = A[(size_t)(r + 1) * n_wp + (c + 1)];
        M[(size_t)r * 2 * n + n + r] = 1.0L;
    }
    for (int p = 0; p < n; ++p) {
        const long double ip = 1.0L / M[(size_t)p * 2 * n + p];
        for (int c = 0; c < 2 * n; ++c) M[(size_t)p * 2 * n + c] *= ip;
        for (int r = 0; r < n; ++r) {
            if (r == p) continue;
            const long double fct = M[(size_t)r * 2 * n + p];
            if (fct == 0.0L) continue;
            for (int c = 0; c < 2 * n; ++c) M[(size_t)r * 2 * n + c] -= fct * M[(size_t)p * 2 * n + c];
        }
    }
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c)  // symmetrised: the kernel reads the table as its own transpose
            out[(size_t)r * n + c] = (double)(0.5L * (M[(size_t)r * 2 * n + n + c] + M[(size_t)c * 2 * n + n + r]));
}

// the plan's device table for n_wp (dtype of the plan); the first call for an n_wp stages it (synchronous)
int traj_metric_table(const kin_plan* p, int32_t n_wp, void* stream, const std::string& fn, const void** out) {
    std::lock_guard<std::mutex> lk(p->traj_mu);
    const auto it = p->traj_minv.find(n_wp);
    if (it != p->traj_minv.end()) {
        *out = it->second;
        return KIN_OK;
    }
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess) cs = hipStreamCaptureStatusNone;
    if (cs == hipStreamCaptureStatusActive)
        return set_error(KIN_E_INVALID, fn + ": the plan's first call for this n_wp stages its metric "
                                        "table and cannot run inside a stream capture (make one call outside the "
                                        "capture first)");
    const size_t n = (size_t)(n_wp - 2) * (n_wp - 2);
    std::vector<double> h(n ? n : 1);
    traj_metric_inverse(n_wp, h.data());
    std::vector<float> hf(h.begin(), h.end());
    void* d = nullptr;
    const bool f32 = p->dtype == KIN_F32;
    const int rc = upload(&d, {{f32 ? (const void*)hf.data() : (const void*)h.data(), h.size() * (f32 ? 4 : 8), 0}},
                          fn.c_str());
    if (rc != KIN_OK) {
        if (d) (void)hipFree(d);
        return rc;
    }
    p->traj_minv.emplace(n_wp, d);
    *out = d;
    return KIN_OK;
}

}  // namespace
}  // namespace kinhip

extern "C" {

int kin_traj_metric_inverse(int32_t n_wp, double* out) {
    if (!out) return set_error(KIN_E_INVALID, "kin_traj_metric_inverse: null out");
    if (n_wp < 3 || n_wp > kTrajMaxWp)
        return set_error(KIN_E_UNSUPPORTED, "kin_traj_metric_inverse: n_wp must be in 3.." + std::to_string(kTrajMaxWp));
    traj_metric_inverse(n_wp, out);
    return KIN_OK;
}

namespace {
using Bad = std::function<int(int, const std::string&)>;

// the parameter block: needs no plan and no device
int traj_check_params(const Bad& bad, const kin_traj_params* prm) {
    if (!prm) return bad(KIN_E_INVALID, "null parameters");
    if (prm->n_wp < 3 || prm->n_wp > kTrajMaxWp)
        return bad(KIN_E_UNSUPPORTED, "n_wp must be in 3.." + std::to_string(kTrajMaxWp) + " (one lane per waypoint of a wave)");
    if (prm->max_iters < 1) return bad(KIN_E_INVALID, "max_iters must be >= 1");
    if (!(prm->weight > 0) || !std::isfinite(prm->weight)) return bad(KIN_E_INVALID, "weight must be finite and > 0");
    if (!(prm->max_step > 0) || !std::isfinite(prm->max_step)) return bad(KIN_E_INVALID, "max_step must be finite and > 0");
    if (!(prm->ftol > 0) || !std::isfinite(prm->ftol)) return bad(KIN_E_INVALID, "ftol must be finite and > 0");
    if (!std::isfinite(prm->margin) || !(prm->band >= 0) || !std::isfinite(prm->band) || !(prm->feas >= 0) ||
        !std::isfinite(prm->feas))
        return bad(KIN_E_INVALID, "margin must be finite, band and feas finite and >= 0");
    return KIN_OK;
}

// the pose parameter block and the targets (after traj_check_params): need no plan and no device either
int traj_check_pose(const Bad& bad, const kin_traj_params* prm, const kin_traj_pose_params* pose, const void* targets,
                    int64_t ldt, int64_t n_traj) {
    if (!pose) return bad(KIN_E_INVALID, "null pose parameters");
    if (pose->n_con != 1) return bad(KIN_E_UNSUPPORTED, "n_con must be 1 (one pose constraint per trajectory)");
    if (!pose->wp || !pose->with_rot) return bad(KIN_E_INVALID, "null wp / with_rot");
    if (pose->wp[0] < 1 || pose->wp[0] > prm->n_wp - 2)
        return bad(KIN_E_INVALID, "wp must be an interior waypoint, 1.." + std::to_string(prm->n_wp - 2));
    if (pose->with_rot[0] != 0 && pose->with_rot[0] != 1) return bad(KIN_E_INVALID, "with_rot must be 0 or 1");
    if (!(pose->weight > 0) || !std::isfinite(pose->weight))
        return bad(KIN_E_INVALID, "pose weight must be finite and > 0");
    if (!(pose->tol_pos > 0) || !std::isfinite(pose->tol_pos) || !(pose->tol_rot > 0) || !std::isfinite(pose->tol_rot))
        return bad(KIN_E_INVALID, "tol_pos and tol_rot must be finite and > 0");
    if (!(pose->damp >= 0) || !std::isfinite(pose->damp)) return bad(KIN_E_INVALID, "damp must be finite and >= 0");
    if (n_traj > 0 && (!targets || ldt < n_traj)) return bad(KIN_E_INVALID, "bad targets / ldt (ldt >= n_traj)");
    return KIN_OK;
}

// what follows the plan's own limits: joint limits, dof_weights, the arrays, the devices, the metric table
// (*minv stays null for n_traj == 0: nothing to launch)
int traj_check_arrays(const Bad& bad, const std::string& fn, const kin_plan* p, const kin_sdf* sdf,
                      const kin_traj_params* prm, const void* xi, int64_t ldx, int64_t n_traj, const void* info,
                      int64_t ldi, void* stream, const void** minv) {
    *minv = nullptr;
    if ((int)p->col_lo.size() != p->n_q) return bad(KIN_E_INVALID, "plan without joint limits");
    const double* dw = prm->dof_weights;
    for (int k = 0; dw && k < p->nqcols; ++k)
        if (!(dw[k] > 0) || !std::isfinite(dw[k])) return bad(KIN_E_INVALID, "dof_weights must be finite and > 0");
    if (n_traj < 0) return bad(KIN_E_INVALID, "n_traj < 0");
    if (n_traj == 0) return KIN_OK;
    if (n_traj > (int64_t(1) << 40) / prm->n_wp) return bad(KIN_E_INVALID, "n_traj * n_wp too large");
    const int64_t cols = n_traj * prm->n_wp;
    if (!xi || ldx < cols) return bad(KIN_E_INVALID, "bad xi / ldx (ldx >= n_traj * n_wp)");
    if (info && ldi < n_traj) return bad(KIN_E_INVALID, "ldi < n_traj");
    if (const int rc = check_device(p->device, fn.c_str(), "the plan")) return rc;
    if (const int rc = check_device(sdf->device, fn.c_str(), "the kin_sdf")) return rc;
    return traj_metric_table(p, prm->n_wp, stream, fn, minv);
}

TrajDof traj_dof(const kin_plan* p, const double* dw) {
    TrajDof dof;
    for (int k = 0; k < kTrajNdLarge; ++k) {
        dof.W[k] = dof.iW[k] = 0.0;
        dof.lo[k] = -INFINITY;
        dof.hi[k] = INFINITY;
    }
    for (int k = 0; k < p->nqcols; ++k) {
        const double w = dw ? dw[k] : 1.0;
        dof.W[k] = w * w;
        dof.iW[k] = 1.0 / (w * w);
        if (k < p->n_q) {
            dof.lo[k] = p->col_lo[k];
            dof.hi[k] = p->col_hi[k];
        }
    }
    return dof;
}

TrajArgs traj_args(const kin_traj_params* prm) {
    return TrajArgs{prm->n_wp, prm->max_iters, prm->margin, prm->band, prm->weight, prm->feas, prm->ftol, prm->max_step};
}

CollArgs traj_coll_args(const kin_sdf* sdf) {
    return CollArgs{INFINITY, 0.0, sdf->n_boxes, sdf->n_aabb, 0, 0, {sdf->bc[0], sdf->bc[1], sdf->bc[2]},
                    {sdf->bh[0], sdf->bh[1], sdf->bh[2]}};
}

// the plan checks of every entry point; one_chain: kin_traj_opt_batch and kin_traj_opt_pose_batch refuse a plan with parts
int traj_check_plan(const Bad& bad, const kin_plan* p, const kin_sdf* sdf, bool one_chain) {
    if (!p || !sdf) return bad(KIN_E_INVALID, "null plan / sdf");
    if (!p->is_coll || p->is_coll_ik) return bad(KIN_E_INVALID, "plan was not made by kin_coll_plan_create");
    if (one_chain && !p->parts.empty())
        return bad(KIN_E_UNSUPPORTED, "the plan's spheres hang off several chains (one sphere group only)");
    if (sdf->attached) return bad(KIN_E_UNSUPPORTED, "the kin_sdf is attached to a scene (a static union only)");
    return KIN_OK;
}

// every entry point's tail: the arrays, then launch_traj (k_traj_tree for a plan with parts, k_traj_pose with pose, else k_traj)
int traj_run(const Bad& bad, const std::string& fn, const kin_plan* p, const kin_sdf* sdf, const kin_traj_params* prm,
             const kin_traj_pose_params* pose, const void* targets, int64_t ldt, void* xi, int64_t ldx, int64_t n_traj,
             int32_t* iters, void* info, int64_t ldi, void* stream, const SceneLaunch* scene = nullptr) {
    const void* minv = nullptr;
    if (const int rc = traj_check_arrays(bad, fn, p, sdf, prm, xi, ldx, n_traj, info, ldi, stream, &minv)) return rc;
    if (n_traj == 0) return KIN_OK;
    const bool tree = scene || !p->parts.empty();  // (the scene kernel: a single-chain plan's one-entry table)
    const hipError_t e = by_dtype(p->dtype, [&](auto t) {
        using T = decltype(t);
        const KProg<T>& P = p->prog<T>();
        TrajPose<T> tp{};
        if (pose) {
            const kin_plan::PoseLink& pl = p->pose_links[0];  // constraint i refers to pose link i
            to_row12<T>(pl.X, tp.X);
            tp.nu = (T)pose->weight;
            tp.damp = (T)pose->damp;
            tp.tol_pos = (T)pose->tol_pos;
            tp.tol_rot = (T)pose->tol_rot;
            tp.step = pl.step;
            tp.wp = pose->wp[0];
            tp.with_rot = pose->with_rot[0];
            tp.part = pl.part;
        }
        // the chain, its bound and ndof (tree: the common bound, the plan's q columns), the pose arguments, the part table
        TrajLaunch<T> d{&P, p->steps<T>(), p->sph<T>(), tree ? p->traj_tree_maxA : p->geom.maxA,
                        tree ? p->nqcols : P.n_jac + ((P.flags & PF_BASE) ? 3 : 0), pose ? &tp : nullptr, (const T*)targets, ldt,
                        tree ? (const TrajPart<T>*)p->d_traj_parts : nullptr,
                        tree ? std::max(1, (int)p->parts.size()) : 0, scene};
        return launch_traj<T>(d, sdf->boxes<T>(), traj_coll_args(sdf), traj_args(prm), traj_dof(p, prm->dof_weights),
                              (const T*)minv, (T*)xi, ldx, n_traj, iters, (T*)info, ldi, (hipStream_t)stream);
    });
    if (e != hipSuccess)
        return set_error(KIN_E_DEVICE, std::string(tree && pose ? "k_traj_pose_tree launch: " : scene ? "k_traj_scene launch: "
                                                   : tree       ? "k_traj_tree launch: "
                                                                : "k_traj launch: ") +
                                           hipGetErrorString(e));
    return KIN_OK;
}

// kin_traj_opt_batch (pose == null) and kin_traj_opt_pose_batch; fn names the entry point in the messages
int traj_opt(const std::string& fn, const kin_plan* p, const kin_sdf* sdf, const kin_traj_params* prm,
             const kin_traj_pose_params* pose, bool with_pose, const void* targets, int64_t ldt, void* xi, int64_t ldx,
             int64_t n_traj, int32_t* iters, void* info, int64_t ldi, void* stream) {
    const Bad bad = [&](int code, const std::string& w) { return set_error(code, fn + ": " + w); };
    // the parameters first (they need no plan), then the plan and the union, then the arrays
    if (const int rc = traj_check_params(bad, prm)) return rc;
    if (with_pose)
        if (const int rc = traj_check_pose(bad, prm, pose, targets, ldt, n_traj)) return rc;
    if (const int rc = traj_check_plan(bad, p, sdf, true)) return rc;
    if (p->geom.maxA > kTrajMaxChain)
        return bad(KIN_E_UNSUPPORTED, "the sphere chain has more than " + std::to_string(kTrajMaxChain) + " steps");
    if (with_pose && p->pose_links.empty())
        return bad(KIN_E_UNSUPPORTED, "the plan has no pose links (kin_traj_plan_create)");
    if (with_pose && p->geom.maxA > kTrajPoseMaxChain)
        return bad(KIN_E_UNSUPPORTED, "the chain has more than " + std::to_string(kTrajPoseMaxChain) + " steps");
    const int nd_max = p->geom.maxA <= 8 ? kTrajNdSmall : kTrajNdLarge;
    if (p->nqcols > nd_max)
        return bad(KIN_E_UNSUPPORTED, "more than " + std::to_string(nd_max) + " q columns (+ base) for this chain");
    return traj_run(bad, fn, p, sdf, prm, with_pose ? pose : nullptr, targets, ldt, xi, ldx, n_traj, iters, info, ldi,
                    stream);
}

// the part-table entry points' tail (k_traj_tree, k_traj_scene, k_traj_pose_tree): the limits of the part loop with
// max_chain steps per part, the scene arrays of an attached union, then traj_run
int traj_parts_run(const Bad& bad, const std::string& fn, const kin_plan* p, const kin_sdf* sdf, const kin_traj_params* prm,
                   int max_chain, const kin_traj_pose_params* pose, const void* targets, int64_t ldt, const void* scene_q,
                   int64_t lds, void* xi, int64_t ldx, int64_t n_traj, int32_t* iters, void* info, int64_t ldi,
                   void* stream) {
    if (sdf->attached && sdf->n_groups > kTrajSceneGroups)
        return bad(KIN_E_UNSUPPORTED, "the union has " + std::to_string(sdf->n_groups) + " moving groups (at most " +
                                          std::to_string(kTrajSceneGroups) + " moving groups)");
    if ((int)p->parts.size() > kTrajMaxParts)
        return bad(KIN_E_UNSUPPORTED, "the plan's spheres hang off more than " + std::to_string(kTrajMaxParts) +
                                          " chains (parts)");
    bool ok = p->parts.empty() ? p->geom.maxA <= max_chain : true;
    for (const auto& s : p->parts) ok = ok && s->geom.maxA <= max_chain;
    if (!ok) return bad(KIN_E_UNSUPPORTED, "a sphere chain has more than " + std::to_string(max_chain) + " steps");
    if (p->nqcols > kTrajNdLarge)
        return bad(KIN_E_UNSUPPORTED, "more than " + std::to_string(kTrajNdLarge) + " q columns (+ base)");
    if (!p->d_traj_parts) return bad(KIN_E_INVALID, "plan without a part table");
    if (!sdf->attached)
        return traj_run(bad, fn, p, sdf, prm, pose, targets, ldt, xi, ldx, n_traj, iters, info, ldi, stream);
    if (n_traj > 0 && n_traj <= (int64_t(1) << 40) / prm->n_wp && sdf->scene_cols > 0 &&
        (!scene_q || (lds != 0 && lds < n_traj * prm->n_wp)))
        return bad(KIN_E_INVALID, "bad scene_q / lds (lds = 0: one scene state, else lds >= n_traj * n_wp)");
    const void* sc = p->dtype == KIN_F32 ? sdf->d_scene_f32 : sdf->d_scene_f64;
    const SceneLaunch sl{sc, (const char*)sc + sdf->scene_steps_off, scene_q, lds, sdf->n_groups, sdf->scene_base_col,
                         lds == 0 ? 1 : 0};
    return traj_run(bad, fn, p, sdf, prm, pose, targets, ldt, xi, ldx, n_traj, iters, info, ldi, stream, &sl);
}

}  // namespace

int kin_traj_opt_batch(const kin_plan* p, const kin_sdf* sdf, const kin_traj_params* prm, void* xi, int64_t ldx,
                       int64_t n_traj, int32_t* iters, void* info, int64_t ldi, void* stream) {
    return traj_opt("kin_traj_opt_batch", p, sdf, prm, nullptr, false, nullptr, 0, xi, ldx, n_traj, iters, info, ldi,
                    stream);
}

int kin_traj_opt_pose_batch(const kin_plan* p, const kin_sdf* sdf, const kin_traj_params* prm,
                            const kin_traj_pose_params* pose, const void* targets, int64_t ldt, void* xi, int64_t ldx,
                            int64_t n_traj, int32_t* iters, void* info, int64_t ldi, void* stream) {
    return traj_opt("kin_traj_opt_pose_batch", p, sdf, prm, pose, true, targets, ldt, xi, ldx, n_traj, iters, info, ldi,
                    stream);
}

// a single-chain plan runs kin_traj_opt_batch's own path (the same k_traj instantiation)
int kin_traj_opt_tree_batch(const kin_plan* p, const kin_sdf* sdf, const kin_traj_params* prm, void* xi, int64_t ldx,
                            int64_t n_traj, int32_t* iters, void* info, int64_t ldi, void* stream) {
    const std::string fn = "kin_traj_opt_tree_batch";
    const Bad bad = [&](int code, const std::string& w) { return set_error(code, fn + ": " + w); };
    if (const int rc = traj_check_params(bad, prm)) return rc;
    if (const int rc = traj_check_plan(bad, p, sdf, false)) return rc;
    if (p->parts.empty())  // (its remaining checks; the ones above pass again)
        return traj_opt(fn, p, sdf, prm, nullptr, false, nullptr, 0, xi, ldx, n_traj, iters, info, ldi, stream);
    return traj_parts_run(bad, fn, p, sdf, prm, kTrajMaxChain, nullptr, nullptr, 0, nullptr, 0, xi, ldx, n_traj, iters, info,
                          ldi, stream);
}

// k_traj_scene: every plan through the part loop (a single-chain plan's one-entry table), the union attached to a scene
int kin_traj_opt_scene_batch(const kin_plan* p, const kin_sdf* sdf, const kin_traj_params* prm, const void* scene_q,
                             int64_t lds, void* xi, int64_t ldx, int64_t n_traj, int32_t* iters, void* info, int64_t ldi,
                             void* stream) {
    const std::string fn = "kin_traj_opt_scene_batch";
    const Bad bad = [&](int code, const std::string& w) { return set_error(code, fn + ": " + w); };
    if (const int rc = traj_check_params(bad, prm)) return rc;
    if (lds < 0) return bad(KIN_E_INVALID, "lds < 0");
    if (!p || !sdf) return bad(KIN_E_INVALID, "null plan / sdf");
    if (!p->is_coll || p->is_coll_ik) return bad(KIN_E_INVALID, "plan was not made by kin_coll_plan_create");
    if (!sdf->attached)
        return bad(KIN_E_INVALID, "the kin_sdf is not attached to a scene (a static union: kin_traj_opt_tree_batch)");
    return traj_parts_run(bad, fn, p, sdf, prm, kTrajMaxChain, nullptr, nullptr, 0, scene_q, lds, xi, ldx, n_traj, iters,
                          info, ldi, stream);
}

// k_traj_pose_tree: the pose link on a multi-part plan (static union) or on any plan against an attached union; a
// single-chain plan against a static union runs kin_traj_opt_pose_batch's own path (the same k_traj_pose instantiation)
int kin_traj_opt_pose_tree_batch(const kin_plan* p, const kin_sdf* sdf, const kin_traj_params* prm,
                                 const kin_traj_pose_params* pose, const void* targets, int64_t ldt, const void* scene_q,
                                 int64_t lds, void* xi, int64_t ldx, int64_t n_traj, int32_t* iters, void* info,
                                 int64_t ldi, void* stream) {
    const std::string fn = "kin_traj_opt_pose_tree_batch";
    const Bad bad = [&](int code, const std::string& w) { return set_error(code, fn + ": " + w); };
    if (const int rc = traj_check_params(bad, prm)) return rc;
    if (const int rc = traj_check_pose(bad, prm, pose, targets, ldt, n_traj)) return rc;
    if (lds < 0) return bad(KIN_E_INVALID, "lds < 0");
    if (!p || !sdf) return bad(KIN_E_INVALID, "null plan / sdf");
    if (!p->is_coll || p->is_coll_ik) return bad(KIN_E_INVALID, "plan was not made by kin_coll_plan_create");
    if (!sdf->attached && (scene_q || lds != 0))
        return bad(KIN_E_INVALID, "scene_q / lds with a static kin_sdf (scene_q must be NULL and lds 0)");
    if (!sdf->attached && p->parts.empty())  // (its remaining checks; the ones above pass again)
        return traj_opt(fn, p, sdf, prm, pose, true, targets, ldt, xi, ldx, n_traj, iters, info, ldi, stream);
    if (p->pose_links.empty()) return bad(KIN_E_UNSUPPORTED, "the plan has no pose links (kin_traj_plan_create)");
    return traj_parts_run(bad, fn, p, sdf, prm, kTrajPoseMaxChain, pose, targets, ldt, scene_q, lds, xi, ldx, n_traj, iters,
                          info, ldi, stream);
}

}  // extern "C"
