// kinhip_internal.h -- host-side launch entry points of the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "kinhip_ik_sched.h"
#include "kinhip_prog.h"

namespace kinhip {

// A/B knobs (schedules, occupancy, trig / atan variants, extra compiler options) are read from the
// environment only by the tools build (`make ab` -> lib/libkinhip_ab.so, -DKINHIP_AB_KNOBS=1,
// driven by tools/ab.py).  The product library never reads them: a stray environment variable
// cannot change a drop-in library's schedule or arithmetic.
#ifndef KINHIP_AB_KNOBS
#define KINHIP_AB_KNOBS 0
#endif
inline const char* ab_env(const char* name) {
#if KINHIP_AB_KNOBS
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}
inline int ab_env_int(const char* name, int dflt) {
    const char* e = ab_env(name);
    return e ? atoi(e) : dflt;
}

// phase-A chain bounds compiled into the kernels (kinhip_device.h KIN_MAXA_DISPATCH)
inline int pick_chain_bound(int n) { return n <= 4 ? 4 : n <= 8 ? 8 : n <= 12 ? 12 : n <= 16 ? 16 : 32; }

struct LaunchGeom {
    int block;      // threads per workgroup (multiple of 64)
    size_t lds;     // dynamic LDS bytes
    int maxA;       // phase-A steps as compiled (4 / 8 / 12 / 16 / 32); the program is padded to it
};

// Tiled SoA (kin_plan_run_tiled): element (i, r) of an array at (i / tile) * ts + r * ld + i % tile.
// tile >= n is the plain SoA of kin_plan_run (one tile, ts unused).
struct TileArgs {
    int64_t tile;
    int64_t tsq, tsp, tsj;  // tile strides (elements) of q, poses / dists, jac / grads
    int64_t tsm = 0;        // min_dist (k_coll)
};
inline TileArgs plain_soa(int64_t n) { return TileArgs{n, 0, 0, 0, 0}; }

// Plan-specialised kernels of one plan (kinhip_jit.cpp); a null entry means
// the generic kernel runs.
struct JitFns {
    hipFunction_t fk = nullptr;
    hipFunction_t fk_stride = nullptr;  // the same, grid-strided with prefetched angles (launch_fk)
    hipFunction_t ik[3][4] = {};  // [0: rows 3, 1: rows 6 axis-angle, 2: rows 6 rpy objective][log2 of lanes per target]
    hipFunction_t ik2[3][4] = {};  // the same without the fp64 solve (phase 2 of launch_ik_dls; G >= 2 only)
    hipFunction_t nakamura = nullptr;
    hipFunction_t coll[2] = {};   // [with gradients]
    hipFunction_t coll_scene[2][2] = {};  // the same over an attached union [with gradients][up to 2 | 4 groups]
    // the same with one attached union's tables compiled in (kin_plan_specialize_scene) [with gradients]
    hipFunction_t coll_scene_c[2] = {};
    // collision-aware IK (k_ik_tree) [rows == 6][lanes: 0 = 1 x 1, 1 = 1 sphere lane x 4 attempt groups,
    // 2 = 16 sphere lanes x 1, 3 = 16 x 4] (kIktVariants)
    hipFunction_t ikt[2][4] = {};
    hipFunction_t ikts[2][4] = {};  // the same over a union attached to a scene of at most 2 moving groups
};
// (kIktVariants, kIktS, kIktG: kinhip_ik_sched.h)

// jf: the plan-specialised kernels (kinhip_jit.cpp) or null for the generic one
template <typename T>
hipError_t launch_fk(const KProg<T>& P, const KStep<T>* steps, const LaunchGeom& g, const T* q, int64_t ldq,
                     int64_t n, T* poses, int64_t ldp, T* jac, int64_t ldj, const TileArgs& ta, const JitFns* jf,
                     hipStream_t st);

struct IkArgs {
    int32_t max_iters;
    double lambda, tol_pos, tol_rot, max_step;
    int32_t with_rot;
    int32_t restarts;
    uint64_t seed;
    int32_t lanes;  // 0 auto
    int64_t index_base;  // global index of target 0 (restart draws)
    double damp_err;     // error-scaled damping (k_ik_dls only)
    void* trace = nullptr;  // kin_ik_dls_batch_trace: [2 (max_iters + 1)][trace_ld] residual norms per iterate
    int64_t trace_ld = 0;
    const void* q_alt = nullptr;  // kin_ik_coll_batch_alt: attempt 1's start pose (same layout as q), or null
};

// restart schedule of kin_ik_params: attempt length L (0: no restarts) and the attempts it reaches
inline void ik_attempts(const IkArgs& a, int* L, int* natt) {
    *L = a.restarts > 0 ? a.max_iters / (a.restarts + 1) : 0;
    *natt = (*L > 0 && a.max_iters > 0) ? 1 + (a.max_iters - 1) / *L : 1;
}

// Device scratch of the two-phase IK schedule (launch_ik_dls): the list of targets attempt 0 did
// not solve and its length, for batches of up to `cap` targets (null: single phase only)
struct IkScratch {
    int32_t* fail_list = nullptr;  // kIkSubRings rings of ring_cap entries (IkArgsT)
    int32_t* fail_aux = nullptr;   // per ring entry: the handed-over active set (IkArgsT::p1_cut)
    uint32_t* fail_ctl = nullptr;  // per ring 3 control words on a 128-byte line, zero at allocation
    int64_t cap = 0;               // targets per call the rings can take (a chunk of at most cap runs two-phase)
    int64_t ring_cap = 0;          // entries per ring, a power of two
};

// true when some chunk of an n-target kin_ik_dls_batch call runs the two-phase schedule (only then
// does the call need the plan's scratch ring)
bool ik_wants_two_phase(const IkArgs& a, int64_t n, int64_t cap);
// true when the last launch_ik_dls of this thread failed after its phase 1 had been launched (the
// targets phase 1 did not solve then keep undefined outputs)
bool ik_last_call_partial();

template <typename T>
hipError_t launch_ik_dls(const KProg<T>& P, const KStep<T>* steps, const LaunchGeom& g, const IkArgs& a,
                         const T* target, int64_t ldt, const T* q0, T* q, int64_t ldq, int64_t n, int32_t* iters,
                         T* err, int64_t lde, const JitFns* jf, const IkScratch& scr, hipStream_t st);

// collision-aware IK (k_ik_tree, kinhip_ikt_dev.h): sphere-distance bound and penalty rows
struct IkcArgs {
    double margin, band, weight, feas;
};
struct SceneLaunch;

// scene: boxes attached to a scene mechanism, scene joint values per target (null: a static union)
template <typename T>
hipError_t launch_ik_tree(const KIkcProg<T>& P, const KIkcStep<T>* steps, const KSphere<T>* sph, const KBox<T>* boxes,
                          const CollArgs& ca, const SceneLaunch* scene, const IkcArgs& c, const IkArgs& a,
                          const T* target, int64_t ldt, const T* q0, T* q, int64_t ldq, int64_t n, int32_t* iters,
                          T* err, int64_t lde, const JitFns* jf, hipStream_t st);

template <typename T>
hipError_t launch_nakamura(const KProg<T>& P, const KStep<T>* steps, const LaunchGeom& g, const T* pts,
                           int64_t ldpt, T* q, int64_t ldq, int64_t n, const JitFns* jf, hipStream_t st);


template <typename T>
hipError_t launch_coll(const KProg<T>& P, const KStep<T>* steps, const KSphere<T>* sph, const KBox<T>* boxes,
                       const LaunchGeom& g, const CollArgs& a, const T* q, int64_t ldq, int64_t n, T* dists,
                       int64_t ldd, T* grads, int64_t ldg, T* min_dist, const TileArgs& ta, const JitFns* jf,
                       hipStream_t st);

// kin_coll_batch_scene: the scene side of k_coll_scene (device tables of the kin_sdf, scene columns)
struct SceneLaunch {
    const void* groups;  // KSceneGroup[ng]
    const void* steps;   // KSceneStep<T>[]
    const void* q;       // scene columns [cols][ld]
    int64_t ld;
    int32_t ng, base_col, uniform;
};
template <typename T>
hipError_t launch_coll_scene(const KProg<T>& P, const KStep<T>* steps, const KSphere<T>* sph, const KBox<T>* boxes,
                             const LaunchGeom& g, const CollArgs& a, const SceneLaunch& sl, const T* q, int64_t ldq,
                             int64_t n, T* dists, int64_t ldd, T* grads, int64_t ldg, T* min_dist, const JitFns* jf,
                             const JitFns* jfs, hipStream_t st);

// k_traj (kin_traj_opt_batch, kinhip_traj_dev.h): a lane keeps its waypoint's q columns (+ base) in registers,
// kTrajNdSmall of them for chain bounds <= 8, kTrajNdLarge for 12 / 16; chains of 32 steps are refused
constexpr int kTrajNdSmall = 12, kTrajNdLarge = 20, kTrajMaxChain = 16, kTrajMaxWp = 64;
struct TrajArgs {
    int32_t n_wp, max_iters;
    double margin, band, weight, feas, ftol, max_step;
};
// per q column (unused columns: W = iW = 0, lo = -inf, hi = +inf)
struct TrajDof {
    double W[kTrajNdLarge], iW[kTrajNdLarge];  // dof_weights^2 and its reciprocal
    double lo[kTrajNdLarge], hi[kTrajNdLarge];  // joint limits (base columns unbounded)
};
// k_traj's POSE variant (kin_traj_opt_pose_batch): one pose link of a kin_traj_plan_create plan held at a
// per-trajectory target at waypoint wp; compiled for chain bounds 4 and 8
constexpr int kTrajMaxPoseLinks = 2, kTrajPoseMaxChain = 8;
template <typename T>
struct TrajPose {
    T X[12];          // link frame = frame(step) * X (row-major 3x4)
    T nu, damp, tol_pos, tol_rot;
    int32_t step;     // chain step whose post-motion frame carries the link (-1: the root / base frame)
    int32_t wp;       // the constrained waypoint (0-based, interior)
    int32_t with_rot;  // 0: 3 rows, 1: 6 rows
    int32_t part;     // k_traj_pose_tree: the part of the table that carries the link (k_traj_pose: unused)
};
// k_traj_tree (kin_traj_opt_tree_batch): the spheres of every part of a multi-chain collision plan.  The parts
// reach the kernel as one device table, staged with the top plan (kin_coll_plan_create): per part the program
// header, a copy of its steps padded to the plan's common bound (8 or 16: the largest part bound rounded up) and a
// copy of its spheres, addressed by byte offsets from the table's start (offsets from the kernel argument, not
// pointers read from memory: the kernel's loads stay global, tests/test_isa.py).
constexpr int kTrajMaxParts = 4;
// k_traj_scene (kin_traj_opt_scene_batch): k_traj_tree against a union attached to a scene of at most this many
// moving groups (the lane's group frames stay in registers over the descent, 12 per group)
constexpr int kTrajSceneGroups = 2;
template <typename T>
struct TrajPart {
    KProg<T> P;
    int64_t steps_off;  // KStep<T>[common bound] (identity steps past the part's own program)
    int64_t sph_off;    // KSphere<T>[P.n_sph]
};
// One launcher for the kernels; the descriptor says which one and carries what only that one takes (tp with parts:
// k_traj_pose_tree, with or without scene).
template <typename T>
struct TrajLaunch {
    const KProg<T>* P;  // the chain (k_traj, k_traj_pose; unused by k_traj_tree)
    const KStep<T>* steps;
    const KSphere<T>* sph;
    int maxA;  // the chain bound (tree: the common bound, 8 or 16); one the variant is not compiled for is refused
    int ndof;  // the plan's q columns (+ base); tree: at most kTrajNdLarge
    const TrajPose<T>* tp = nullptr;  // k_traj_pose (else null): targets [12][ldt], one column per trajectory; info [6][ldi]
    const T* targets = nullptr;
    int64_t ldt = 0;
    const TrajPart<T>* parts = nullptr;  // k_traj_tree (else null)
    int n_parts = 0;
    // k_traj_scene (else null; with parts, a single-chain plan's one-entry table included): the union's scene tables
    // and scene_q [cols][ld], sample t * n_wp + w = waypoint w of trajectory t (uniform: one set for the launch)
    const SceneLaunch* scene = nullptr;
};
// one chunk of launch_traj's loop for k_traj_scene (kinhip_traj_scene.hip) and k_traj_pose_tree; called by launch_traj only
template <typename T>
struct TrajSceneChunk {
    dim3 grid, block;
    size_t lds;
    hipStream_t st;
    const TrajPart<T>* parts;
    int n_parts, ndof;
    const KBox<T>* boxes;
    const CollArgs* a;
    const TrajArgs* ta;
    const TrajDof* dof;
    const T* minvT;
    const SceneLaunch* scene;
    int64_t sample0;  // the chunk's first sample of scene_q
    T* xi;
    int64_t ldx, n_traj;
    int32_t* iters;
    T* info;
    int64_t ldi;
};
template <typename T>
bool launch_traj_scene_chunk(int maxA, int L, const TrajSceneChunk<T>& k);
// the same for k_traj_pose_tree (kinhip_traj_pose_tree.hip): tp with its part, the chunk's first target column;
// k.scene null for a static union (k.sample0 is then unused)
template <typename T>
bool launch_traj_pose_tree_chunk(int maxA, int L, const TrajSceneChunk<T>& k, TrajPose<T> tp, const T* targets,
                                 int64_t ldt);
// minv: (A_sub[I,I])^-1 of n_wp waypoints on the device, row-major (symmetric, so also its transpose)
template <typename T>
hipError_t launch_traj(const TrajLaunch<T>& d, const KBox<T>* boxes, const CollArgs& a, const TrajArgs& ta,
                       const TrajDof& dof, const T* minv, T* xi, int64_t ldx, int64_t n_traj, int32_t* iters, T* info,
                       int64_t ldi, hipStream_t st);

template <typename T>
hipError_t launch_pose_residual(const T* poses, int64_t ldp, const T* target, int64_t ldt, int64_t n, int rows, T* vals,
                                int64_t ldv, hipStream_t st);

}  // namespace kinhip
