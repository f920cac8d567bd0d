// kinhip_plan.h -- the objects behind the C-ABI handles (kin_model, kin_sdf, kin_plan) and what the host
// translation units share: models (kinhip_model.cpp), staging (kinhip_stage.cpp), signed-distance
// unions (kinhip_sdf.cpp), plans and launches (kinhip_host.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "kinhip.h"
#include "kinhip_host.h"
#include "kinhip_ik_sets.h"
#include "kinhip_internal.h"
#include "kinhip_m34.h"

namespace kinhip {

// f(T{}) with T = float or double, by a kin_dtype
template <typename F>
auto by_dtype(int32_t dtype, F&& f) {
    return dtype == KIN_F32 ? f(float{}) : f(double{});
}

// the runtime calls of the IK scratch-set scheduler (kinhip_ik_sets.h)
struct HipIkBackend {
    using Event = hipEvent_t;
    using Error = hipError_t;
    static constexpr Error kSuccess = hipSuccess, kNotReady = hipErrorNotReady;
    static Error event_create(Event* e) { return hipEventCreateWithFlags(e, hipEventDisableTiming); }
    static void event_destroy(Event e) { (void)hipEventDestroy(e); }
    static Error event_query(Event e) { return hipEventQuery(e); }
    static Error event_synchronize(Event e) { return hipEventSynchronize(e); }
    static Error event_record(Event e, void* st) { return hipEventRecord(e, (hipStream_t)st); }
    static void stream_synchronize(void* st) { (void)hipStreamSynchronize((hipStream_t)st); }
    static bool is_per_thread(void* st) { return (hipStream_t)st == hipStreamPerThread; }
    static Error alloc_zeroed(void** p, size_t bytes) {
        Error e = hipMalloc(p, bytes);
        if (e == hipSuccess) e = hipMemset(*p, 0, bytes);
        if (e != hipSuccess && *p) (void)hipFree(*p);
        return e;
    }
    static void free(void* p) { (void)hipFree(p); }
    static Error clear_last_error() { return hipGetLastError(); }
};
using IkSets = IkScratchSets<HipIkBackend>;

}  // namespace kinhip

using namespace kinhip;  // (the handle types are the C-ABI's, at file scope)

struct kin_plan;

struct kin_model {
    int32_t n_links = 0;
    std::vector<int32_t> jtype, jplink, jclink;  // 1-based link ids
    std::vector<double> jpose;                    // [J][16] column-major
    std::vector<double> jaxis;                    // [J][3]
    std::vector<double> jlo, jhi;
    std::vector<int32_t> link_pjoint;               // 0-based joint, -1 root
    std::vector<std::vector<int32_t>> child_joints;  // per link, 0-based joints in joint order
    std::vector<double> angles;                      // m.angles
    bool with_base = false;
    uint64_t version = 0;
    std::mutex mu;
    std::map<std::string, kin_plan*> cache;

    int32_t n_joints() const { return (int32_t)jtype.size(); }
    int32_t plink(int32_t l) const { return link_pjoint[l] < 0 ? -1 : jplink[link_pjoint[l]] - 1; }
    M34 pose(int32_t j) const { return m_from_col16(&jpose[16 * j]); }
    // joint motion at a constant angle (the right factor of joint_transform)
    M34 motion_at(int32_t j, double a) const {
        if (jtype[j] == KIN_JOINT_FIXED || a == 0.0) return m_identity();
        const double* ax = &jaxis[3 * j];
        if (jtype[j] == KIN_JOINT_REVOLUTE) {
            const double s = sin(0.5 * a), c = cos(0.5 * a);
            return m_quat(c, ax[0] * s, ax[1] * s, ax[2] * s);
        }
        M34 m = m_identity();
        m.t[0] = ax[0] * a; m.t[1] = ax[1] * a; m.t[2] = ax[2] * a;
        return m;
    }
    // joint_transform(joint, angle), src/mechanism.jl:90-103
    M34 joint_tf(int32_t j, double a) const {
        if (jtype[j] == KIN_JOINT_FIXED || a == 0.0) return pose(j);
        return m_mul(pose(j), motion_at(j, a));
    }
    bool relevant(int32_t j, int32_t l) const {  // rptable[j][l]: l in subtree of j's child
        const int32_t c = jclink[j] - 1;
        for (int32_t x = l, guard = 0; x >= 0 && guard <= n_links; x = plink(x), ++guard)
            if (x == c) return true;
        return false;
    }
};

struct kin_sdf {
    int device = -1;        // HIP device holding the box tables (current device at creation)
    // boxes attached to a scene mechanism (kin_sdf_create_attached): group table + scene steps
    bool attached = false;
    int32_t n_groups = 0, scene_cols = 0, scene_base_col = -1;
    void* d_scene_f32 = nullptr;  // KSceneGroup[n_groups], then KSceneStep<float>[] at scene_steps_off
    void* d_scene_f64 = nullptr;
    size_t scene_steps_off = 0;
    int32_t n_boxes = 0;
    int32_t n_aabb = 0;     // the first n_aabb boxes are axis-aligned (KAabb table after the KBox array)
    double bc[3] = {0, 0, 0}, bh[3] = {0, 0, 0};  // world-aligned box enclosing every box (broad phase, coll_body)
    void* d_f32 = nullptr;
    void* d_f64 = nullptr;
    template <typename T>
    const KBox<T>* boxes() const { return (const KBox<T>*)(sizeof(T) == 4 ? d_f32 : d_f64); }
    // host copies of an attached union's tables (kin_plan_specialize_scene compiles them in), and an id that
    // is never reused (the plans' scene-specialised kernels are keyed by it)
    uint64_t uid = 0;
    std::vector<KSceneGroup> h_groups;
    std::vector<KSceneStep<float>> h_ssf;
    std::vector<KSceneStep<double>> h_ssd;
    std::vector<KBox<float>> h_bf;
    std::vector<KBox<double>> h_bd;
    std::vector<KAabb<float>> h_af;
    std::vector<KAabb<double>> h_ad;
    template <typename T>
    auto host_tables() const {  // scene steps, boxes, axis-aligned boxes of element type T
        if constexpr (sizeof(T) == 4) return std::tie(h_ssf, h_bf, h_af);
        else return std::tie(h_ssd, h_bd, h_ad);
    }
    ~kin_sdf() {
        if (d_f32) (void)hipFree(d_f32);
        if (d_f64) (void)hipFree(d_f64);
        if (d_scene_f32) (void)hipFree(d_scene_f32);
        if (d_scene_f64) (void)hipFree(d_scene_f64);
    }
};

struct kin_plan {
    int device = -1;  // HIP device holding the staged program (current device at creation); runs must match
    int32_t dtype = KIN_F32;
    int32_t nqcols = 0, rows = 0, ncols = 0, n_q = 0, n_out = 0;
    bool has_jac = false, with_base = false, has_rpy = false;
    bool ik_ok = false;
    int32_t out_link0 = 0, jac_link = 0;  // first output link / Jacobian link (kin_pose_const_batch)
    std::string ik_why;
    void* d_steps = nullptr;
    KProg<float> pf{};
    KProg<double> pd{};
    LaunchGeom geom{256, 0, 8};
    // the program of element type T = the plan's dtype (by_dtype)
    template <typename T>
    const KProg<T>& prog() const {
        if constexpr (sizeof(T) == 4) return pf;
        else return pd;
    }
    template <typename T>
    KProg<T>& prog() { return const_cast<KProg<T>&>(std::as_const(*this).prog<T>()); }
    template <typename T>
    const KStep<T>* steps() const { return (const KStep<T>*)d_steps; }
    template <typename T>
    const KStep<T>* host_steps() const { return (const KStep<T>*)h_steps.data(); }
    template <typename T>
    const KSphere<T>* sph() const { return (const KSphere<T>*)d_sph; }
    // collision plans (kin_coll_plan_create); is_coll_ik: also an IK plan of the spheres' chain
    // (kin_coll_ik_plan_create: kin_ik_dls_batch, kin_ik_coll_batch, kin_coll_batch)
    bool is_coll = false;
    bool is_coll_ik = false;
    int32_t n_sph = 0;
    void* d_sph = nullptr;
    // spheres on several chains: one staged program per chain (kin_coll_plan_create)
    std::vector<std::unique_ptr<kin_plan>> parts;
    // host copy of the staged program (plan specialisation, kinhip_jit.cpp)
    std::vector<unsigned char> h_steps, h_sph;
    int32_t n_steps = 0;
    JitKernels* jit = nullptr;
    uint32_t jit_mask = 0;
    // two-phase IK schedule scratch sets and their scheduler (kinhip_ik_sets.h)
    mutable IkSets ik_sets;
    // collision-aware IK program (kin_coll_ik_plan_create, k_ik_tree): the needed tree, host copies
    // (plan specialisation) and one device allocation [KIkcStep<T> steps | KSphere<T> spheres]
    KIkcProg<float> ikf{};
    KIkcProg<double> ikd{};
    template <typename T>
    const KIkcProg<T>& ikc() const {
        if constexpr (sizeof(T) == 4) return ikf;
        else return ikd;
    }
    template <typename T>
    KIkcProg<T>& ikc() { return const_cast<KIkcProg<T>&>(std::as_const(*this).ikc<T>()); }
    std::vector<unsigned char> h_ikc_steps, h_ikc_sph;
    void* d_ikc = nullptr;
    size_t ikc_sph_off = 0;
    // kin_plan_specialize_scene: k_coll_scene kernels with one attached union compiled in, by kin_sdf uid
    mutable std::mutex scene_mu;
    std::map<uint64_t, JitKernels*> scene_jit;
    const JitFns* scene_fns(uint64_t uid) const {
        std::lock_guard<std::mutex> lk(scene_mu);
        const auto it = scene_jit.find(uid);
        return it == scene_jit.end() ? nullptr : jit_fns(it->second);
    }
    // kin_traj_opt_batch: the q columns' joint limits (base columns unbounded; kin_coll_plan_create) and the
    // metric tables (A_sub[I,I])^-1 on the device, in the plan's dtype, by n_wp (staged on first use)
    std::vector<double> col_lo, col_hi;
    mutable std::mutex traj_mu;
    mutable std::map<int32_t, void*> traj_minv;
    // kin_traj_plan_create: the pose links of kin_traj_opt_pose_batch (fp64 on the host; a kernel argument, never
    // part of the sphere table): the chain step whose post-motion frame carries the link (-1: the root / base
    // frame) and the static transform from that frame to the link; part: the part whose chain that is (the top plan's
    // table; 0 for a single-chain plan)
    struct PoseLink {
        int32_t step;
        M34 X;
        int32_t part = 0;
    };
    std::vector<PoseLink> pose_links;
    // kin_traj_opt_tree_batch: the part table of a multi-chain plan on the device, [TrajPart<T>[n_parts] | every
    // part's steps padded to traj_tree_maxA | every part's spheres] (kin_coll_plan_create; null when the plan is
    // past k_traj_tree's limits)
    void* d_traj_parts = nullptr;
    int32_t traj_tree_maxA = 0;
    ~kin_plan() {
        if (d_traj_parts) (void)hipFree(d_traj_parts);
        for (auto& kv : traj_minv) (void)hipFree(kv.second);
        for (auto& kv : scene_jit) jit_destroy(kv.second);
        if (d_ikc) (void)hipFree(d_ikc);
        jit_destroy(jit);
        if (d_steps) (void)hipFree(d_steps);
        if (d_sph) (void)hipFree(d_sph);
    }
};

namespace kinhip {
// staging (kinhip_stage.cpp): fills the plan's host program and headers, calls no runtime; coll / sph_out:
// the spheres of a collision plan and their global indices (null: none / their own order); pose_ids: the
// n_pose pose links of a kin_traj_plan_create plan (P.pose_links)
int stage_plan(const kin_model& m, const kin_plan_desc& d, const kin_coll_desc* coll, const int32_t* sph_out,
               kin_plan& P, int32_t n_pose = 0, const int32_t* pose_ids = nullptr);
int stage_ikc_tree(const kin_model& m, const kin_coll_desc* c, int32_t link_id, kin_plan& P);

// kinhip_host.cpp
int check_device(int owner, const char* fn, const char* what);
int plan_create(const kin_model* m, const kin_plan_desc* d, kin_plan** out);
// Host spans (each at its byte offset) into one fresh device allocation; *dst is null on failure.  The
// KIN_E_DEVICE message names the failing runtime call, or fn where the entry point reports under its own name.
struct HostSpan {
    const void* data;
    size_t bytes, offset;
};
int upload(void** dst, std::initializer_list<HostSpan> spans, const char* fn = nullptr);
}  // namespace kinhip
