// kinhip_host.cpp -- C-ABI of libkinhip.so: plans (creation, upload, specialisation) and launches.
// Models are in kinhip_model.cpp, staging in kinhip_stage.cpp, kin_sdf in kinhip_sdf.cpp.
//
// Reference semantics restated here (host side):
//   get_jacobian! column relevance / errors    src/algorithm.jl:83-106
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "kinhip_plan.h"

namespace kinhip {

// A plan's program (and its specialised module) lives on the device that was current when it was
// created; launching it from another device would read that memory through the wrong context.
int check_device(int owner, const char* fn, const char* what) {
    int cur = -1;
    const hipError_t e = hipGetDevice(&cur);
    if (e != hipSuccess) return set_error(KIN_E_DEVICE, std::string(fn) + ": hipGetDevice: " + hipGetErrorString(e));
    if (cur != owner)
        return set_error(KIN_E_INVALID, std::string(fn) + ": " + what + " lives on HIP device " + std::to_string(owner) +
                                            " but the current device is " + std::to_string(cur));
    return KIN_OK;
}

int upload(void** dst, std::initializer_list<HostSpan> spans, const char* fn) {
    auto fail = [&](const char* call, hipError_t e) {
        return set_error(KIN_E_DEVICE, std::string(fn ? fn : call) + ": " + hipGetErrorString(e));
    };
    size_t bytes = 0;
    for (const HostSpan& s : spans) bytes = std::max(bytes, s.offset + s.bytes);
    hipError_t e = hipMalloc(dst, bytes);
    if (e != hipSuccess) {
        *dst = nullptr;
        return fail("hipMalloc", e);
    }
    for (const HostSpan& s : spans) {
        if (!s.bytes) continue;
        e = hipMemcpy((char*)*dst + s.offset, s.data, s.bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail("hipMemcpy", e);
    }
    return KIN_OK;
}

// the staged program (and a collision plan's spheres) to the current device
static int upload_plan(kin_plan& P) {
    const hipError_t e = hipGetDevice(&P.device);
    if (e != hipSuccess) return set_error(KIN_E_DEVICE, std::string("hipGetDevice: ") + hipGetErrorString(e));
    if (const int rc = upload(&P.d_steps, {{P.h_steps.data(), P.h_steps.size(), 0}})) return rc;
    return P.is_coll ? upload(&P.d_sph, {{P.h_sph.data(), P.h_sph.size(), 0}}) : KIN_OK;
}

int plan_create(const kin_model* m, const kin_plan_desc* d, kin_plan** out) {
    if (!m || !d || !out) return set_error(KIN_E_INVALID, "kin_plan_create: null argument");
    auto P = std::make_unique<kin_plan>();
    if (const int rc = stage_plan(*m, *d, nullptr, nullptr, *P)) return rc;
    if (const int rc = upload_plan(*P)) return rc;
    *out = P.release();
    return KIN_OK;
}

}  // namespace kinhip

namespace {
bool dev_ptr_ok(const void* p) { return p != nullptr; }
}  // namespace

extern "C" {

int kin_plan_create(const kin_model* m, const kin_plan_desc* d, kin_plan** out) { return plan_create(m, d, out); }

int kin_plan_destroy(kin_plan* p) {
    delete p;
    return KIN_OK;
}

int kin_plan_shape(const kin_plan* p, int32_t* nq, int32_t* rows, int32_t* cols) {
    if (!p) return set_error(KIN_E_INVALID, "null plan");
    if (nq) *nq = p->nqcols;
    if (rows) *rows = p->has_jac ? p->rows : 0;
    if (cols) *cols = p->ncols;
    return KIN_OK;
}

int kin_plan_chain_bound(const kin_plan* p, int32_t* out) {
    if (!p || !out) return set_error(KIN_E_INVALID, "kin_plan_chain_bound: null plan / out");
    *out = p->geom.maxA;
    return KIN_OK;
}

int kin_plan_part_count(const kin_plan* p, int32_t* out) {
    if (!p || !out) return set_error(KIN_E_INVALID, "kin_plan_part_count: null plan / out");
    *out = p->parts.empty() ? 1 : (int32_t)p->parts.size();
    return KIN_OK;
}

int kin_plan_part_chain_bound(const kin_plan* p, int32_t part, int32_t* out) {
    if (!p || !out) return set_error(KIN_E_INVALID, "kin_plan_part_chain_bound: null plan / out");
    const int32_t np = p->parts.empty() ? 1 : (int32_t)p->parts.size();
    if (part < 0 || part >= np) return set_error(KIN_E_INVALID, "kin_plan_part_chain_bound: part out of range");
    *out = p->parts.empty() ? p->geom.maxA : p->parts[part]->geom.maxA;
    return KIN_OK;
}

int kin_plan_pose_link_part(const kin_plan* p, int32_t i, int32_t* part) {
    if (!p || !part) return set_error(KIN_E_INVALID, "kin_plan_pose_link_part: null plan / part");
    if (i < 0 || i >= (int32_t)p->pose_links.size())
        return set_error(KIN_E_KEY, "kin_plan_pose_link_part: pose link index out of range");
    *part = p->pose_links[i].part;
    return KIN_OK;
}

namespace {
int plan_run(const kin_plan* p, const void* q, int64_t ldq, int64_t n, void* poses, int64_t ldp, void* jac,
             int64_t ldj, const TileArgs& ta, void* stream, const char* fn) {
    auto bad = [&](const char* what) { return set_error(KIN_E_INVALID, std::string(fn) + ": " + what); };
    if (!p) return bad("null plan");
    if (n < 0) return bad("n < 0");
    if (n == 0) return KIN_OK;
    if (const int rc = check_device(p->device, fn, "the plan")) return rc;
    const int64_t span = std::min(ta.tile, n);  // configurations along one row of one tile
    if (p->nqcols > 0 && (!dev_ptr_ok(q) || ldq < span)) return bad("bad q / ldq");
    if (p->n_out > 0 && !poses) return bad("null poses");
    if (poses && ldp < span) return bad("ldp < tile");
    if (p->has_jac && (!jac || ldj < span)) return bad("bad jac / ldj");
    const hipError_t e = by_dtype(p->dtype, [&](auto t) {
        using T = decltype(t);
        return launch_fk<T>(p->prog<T>(), p->steps<T>(), p->geom, (const T*)q, ldq, n, (T*)poses, ldp, (T*)jac, ldj, ta,
                            jit_fns(p->jit), (hipStream_t)stream);
    });
    if (e != hipSuccess) return set_error(KIN_E_DEVICE, std::string("k_fk launch: ") + hipGetErrorString(e));
    return KIN_OK;
}
}  // namespace

int kin_plan_run(const kin_plan* p, const void* q, int64_t ldq, int64_t n, void* poses, int64_t ldp, void* jac,
                 int64_t ldj, void* stream) {
    return plan_run(p, q, ldq, n, poses, ldp, jac, ldj, plain_soa(n), stream, "kin_plan_run");
}

int kin_plan_run_tiled(const kin_plan* p, int64_t tile, const void* q, int64_t ldq, int64_t tsq, int64_t n,
                       void* poses, int64_t ldp, int64_t tsp, void* jac, int64_t ldj, int64_t tsj, void* stream) {
    auto bad = [&](const char* what) { return set_error(KIN_E_INVALID, std::string("kin_plan_run_tiled: ") + what); };
    if (!p) return bad("null plan");
    if (tile < 256 || tile % 256 != 0 || tile > (int64_t(1) << 26)) return bad("tile must be a multiple of 256 <= 2^26");
    if (n > tile) {  // several tiles: their strides must not overlap a tile's rows
        if (p->nqcols > 0 && tsq < (int64_t)p->nqcols * ldq) return bad("tsq < n_qcols * ldq");
        if (p->n_out > 0 && tsp < (int64_t)p->n_out * 12 * ldp) return bad("tsp < n_out * 12 * ldp");
        if (p->has_jac && tsj < (int64_t)p->ncols * p->rows * ldj) return bad("tsj < cols * rows * ldj");
    }
    return plan_run(p, q, ldq, n, poses, ldp, jac, ldj, TileArgs{tile, tsq, tsp, tsj}, stream, "kin_plan_run_tiled");
}

namespace {
int specialize_one(kin_plan* p, uint32_t kernels) {
    if ((p->jit_mask & kernels) == kernels) return KIN_OK;
    kernels |= p->jit_mask;
    JitKernels* k = nullptr;
    const bool ikc = p->is_coll_ik;
    const int rc = by_dtype(p->dtype, [&](auto t) {
        using T = decltype(t);
        return jit_build<T>(p->prog<T>(), p->host_steps<T>(), p->n_steps, p->geom.maxA,
                            p->h_sph.empty() ? nullptr : p->h_sph.data(), p->n_sph, ikc ? &p->ikc<T>() : nullptr,
                            p->h_ikc_steps.data(), p->h_ikc_sph.data(), kernels, &k);
    });
    if (rc != KIN_OK) return rc;
    jit_destroy(p->jit);
    p->jit = k;
    p->jit_mask = kernels;
    return KIN_OK;
}
}  // namespace

int kin_plan_specialize(kin_plan* p, uint32_t kernels) {
    if (!p) return set_error(KIN_E_INVALID, "kin_plan_specialize: null plan");
    if (const int rc = check_device(p->device, "kin_plan_specialize", "the plan")) return rc;
    uint32_t applies = 0;
    if (p->is_coll_ik) {
        applies = KIN_SPEC_IK | KIN_SPEC_IK_COLL | KIN_SPEC_IK_COLL_SCENE;
    } else if (p->is_coll) {
        applies = KIN_SPEC_COLL;
    } else {
        applies = KIN_SPEC_FK;
        if (p->ik_ok) applies |= KIN_SPEC_IK;
        if (p->ik_ok && !p->with_base) applies |= KIN_SPEC_NAKAMURA;
    }
    if (kernels == 0) kernels = applies;
    if (kernels & ~applies) return set_error(KIN_E_UNSUPPORTED, "kin_plan_specialize: kernel kind does not apply");
    if (p->parts.empty()) return specialize_one(p, kernels);
    for (auto& part : p->parts) {  // multi-chain collision plans: every chain program
        const int rc = specialize_one(part.get(), kernels);
        if (rc != KIN_OK) return rc;
    }
    p->jit_mask = kernels;
    return KIN_OK;
}

int kin_jit_selfcheck(void) { return jit_selfcheck(); }

int kin_plan_specialize_scene(kin_plan* p, const kin_sdf* sdf) {
    auto bad = [](int code, const std::string& w) { return set_error(code, "kin_plan_specialize_scene: " + w); };
    if (!p || !sdf) return bad(KIN_E_INVALID, "null plan / sdf");
    if (!p->is_coll || p->is_coll_ik) return bad(KIN_E_UNSUPPORTED, "plan was not made by kin_coll_plan_create");
    if (!sdf->attached) return bad(KIN_E_INVALID, "the kin_sdf is not attached to a scene");
    if (const int rc = check_device(p->device, "kin_plan_specialize_scene", "the plan")) return rc;
    if (const int rc = check_device(sdf->device, "kin_plan_specialize_scene", "the kin_sdf")) return rc;
    auto one = [&](kin_plan* s) -> int {
        {
            std::lock_guard<std::mutex> lk(s->scene_mu);
            if (s->scene_jit.count(sdf->uid)) return KIN_OK;
        }
        JitKernels* k = nullptr;
        const int rc = by_dtype(s->dtype, [&](auto t) {
            using T = decltype(t);
            const auto& [ss, b, a] = sdf->host_tables<T>();
            const JitScene js{sdf->h_groups.data(), (int)sdf->h_groups.size(), ss.data(), (int)ss.size(), b.data(),
                              (int)b.size(), a.data(), (int)a.size(), sdf->scene_base_col};
            return jit_build_scene<T>(s->prog<T>(), s->host_steps<T>(), s->n_steps, s->geom.maxA,
                                      s->h_sph.empty() ? nullptr : s->h_sph.data(), s->n_sph, js, &k);
        });
        if (rc != KIN_OK) return rc;
        std::lock_guard<std::mutex> lk(s->scene_mu);
        if (!s->scene_jit.emplace(sdf->uid, k).second) jit_destroy(k);
        return KIN_OK;
    };
    if (p->parts.empty()) return one(p);
    for (auto& part : p->parts)
        if (const int rc = one(part.get())) return rc;
    return KIN_OK;
}

int kin_plan_specialized(const kin_plan* p, uint32_t* kernels) {
    if (!p || !kernels) return set_error(KIN_E_INVALID, "kin_plan_specialized: null argument");
    *kernels = p->jit_mask;
    return KIN_OK;
}

namespace {
// The part table of k_traj_tree (kin_traj_opt_tree_batch) for a multi-chain plan within its limits -- and, with one
// entry, of a single-chain plan (kin_traj_opt_scene_batch runs every plan through the part loop) -- one device
// allocation [TrajPart<T>[n_parts] | steps | spheres]: the parts' program headers, copies of their phase-A steps
// padded with identity steps to the common bound (so that the kernel's unrolled walk stays inside every staged
// program) and copies of their sphere tables.  What kin_coll_batch launches for a part (its own steps at its own
// bound) is untouched.
int upload_traj_parts(kin_plan& top, const std::string& fn) {
    std::vector<const kin_plan*> parts;
    for (const auto& s : top.parts) parts.push_back(s.get());
    if (parts.empty()) parts.push_back(&top);
    const size_t np = parts.size();
    int maxA = 0;
    for (const kin_plan* s : parts) maxA = std::max(maxA, s->geom.maxA);
    if (np > (size_t)kTrajMaxParts || maxA > kTrajMaxChain) return KIN_OK;  // (refused at the call)
    const int bound = maxA <= 8 ? 8 : 16;
    return by_dtype(top.dtype, [&](auto t) -> int {
        using T = decltype(t);
        const size_t steps_off = (np * sizeof(TrajPart<T>) + 255) / 256 * 256;
        size_t bytes = steps_off + np * bound * sizeof(KStep<T>);
        std::vector<size_t> sph_off(np);
        for (size_t k = 0; k < np; ++k) {
            sph_off[k] = bytes;
            bytes += parts[k]->h_sph.size();
        }
        std::vector<unsigned char> h(bytes, 0);
        KStep<T> pad;
        memset(&pad, 0, sizeof(pad));
        to_row12<T>(m_identity(), pad.F);
        to_row12<T>(m_identity(), pad.X);
        pad.lo = (T)-INFINITY;
        pad.hi = (T)INFINITY;
        pad.kind = pad.jkind = MOT_NONE;
        pad.qcol = pad.out = pad.save = -1;
        pad.load = LOAD_NONE;
        for (size_t k = 0; k < np; ++k) {
            const kin_plan& s = *parts[k];
            TrajPart<T>* tp = reinterpret_cast<TrajPart<T>*>(h.data()) + k;
            KStep<T>* hs = reinterpret_cast<KStep<T>*>(h.data() + steps_off) + k * bound;
            tp->P = s.prog<T>();
            tp->steps_off = (int64_t)(steps_off + k * bound * sizeof(KStep<T>));
            tp->sph_off = (int64_t)sph_off[k];
            for (int i = 0; i < bound; ++i) hs[i] = i < s.geom.maxA ? s.host_steps<T>()[i] : pad;
            memcpy(h.data() + sph_off[k], s.h_sph.data(), s.h_sph.size());
        }
        if (const int rc = upload(&top.d_traj_parts, {{h.data(), bytes, 0}}, fn.c_str())) {
            if (top.d_traj_parts) (void)hipFree(top.d_traj_parts);
            top.d_traj_parts = nullptr;
            return rc;
        }
        top.traj_tree_maxA = bound;
        return KIN_OK;
    });
}

// kin_coll_plan_create, and with pose links kin_traj_plan_create (fn names the entry point in the messages)
int coll_plan_create(const kin_model* m, const kin_coll_desc* c, int32_t n_pose, const int32_t* pose_ids, kin_plan** out,
                     const std::string& fn) {
    if (!m || !c || !out) return set_error(KIN_E_INVALID, fn + ": null argument");
    if (c->n_spheres < 1 || !c->sphere_link_ids || !c->radii)
        return set_error(KIN_E_INVALID, fn + ": need >= 1 sphere with link ids and radii");
    if (c->n_q < 0 || (c->n_q && !c->q_joint_ids)) return set_error(KIN_E_INVALID, fn + ": bad q");
    const int32_t L = m->n_links, J = m->n_joints();
    std::vector<char> moving(J, 0);
    for (int32_t k = 0; k < c->n_q; ++k) {
        const int32_t j = c->q_joint_ids[k] - 1;
        if (j < 0 || j >= J) return set_error(KIN_E_KEY, fn + ": q joint id out of range");
        moving[j] = m->jtype[j] != KIN_JOINT_FIXED;
    }
    // Group the spheres by chain: the spine of a group is the remaining sphere anchor (nearest link
    // below a moving joint) with the most moving joints above it; the group takes every remaining
    // sphere whose anchor lies on the spine's root path.  One staged program per group.
    const auto anchor_of = [&](int32_t x) {
        while (x >= 0 && m->link_pjoint[x] >= 0 && !moving[m->link_pjoint[x]]) x = m->plink(x);
        return x;
    };
    std::vector<int32_t> anchor(c->n_spheres), depth(c->n_spheres);
    for (int32_t k = 0; k < c->n_spheres; ++k) {
        int32_t x = c->sphere_link_ids[k] - 1;
        if (x < 0 || x >= L) return set_error(KIN_E_KEY, fn + ": sphere link id out of range");
        x = anchor_of(x);
        int dd = 0;
        for (int32_t y = x; y >= 0 && m->link_pjoint[y] >= 0; y = m->plink(y)) dd += moving[m->link_pjoint[y]];
        anchor[k] = x;
        depth[k] = dd;
    }
    for (int32_t k = 0; k < n_pose; ++k)
        if (pose_ids[k] < 1 || pose_ids[k] > L) return set_error(KIN_E_KEY, fn + ": pose link id out of range");
    std::vector<char> done(c->n_spheres, 0);
    std::vector<std::unique_ptr<kin_plan>> parts;
    // pose link k rides on the first part, in this order, whose spine is above, at or below its anchor; (part, index
    // among that part's pose links), part -1: none yet
    std::vector<std::pair<int32_t, int32_t>> pose_at(n_pose, {-1, 0});
    int32_t left = c->n_spheres;
    while (left > 0) {
        int32_t spine = -1, best = -1;
        for (int32_t k = 0; k < c->n_spheres; ++k)
            if (!done[k] && depth[k] > best) { best = depth[k]; spine = anchor[k]; }
        std::vector<int32_t> pose_here;
        for (int32_t k = 0; k < n_pose; ++k) {  // the links on this chain or its extension: it reaches the deepest of them
            if (pose_at[k].first >= 0) continue;
            const int32_t a = anchor_of(pose_ids[k] - 1);
            bool above = false, below = false;  // a above (or at) the spine / the spine above a
            for (int32_t y = spine; y >= 0 && !above; y = m->plink(y)) above = y == a;
            for (int32_t y = a; y >= 0 && !below; y = m->plink(y)) below = y == spine;
            if (!above && !below) continue;  // (another branch than this chain: a later part's, or none's)
            if (!above) spine = a;
            pose_at[k] = {(int32_t)parts.size(), (int32_t)pose_here.size()};
            pose_here.push_back(pose_ids[k]);
        }
        const bool with_pose = !pose_here.empty();
        std::vector<char> on_path(L, 0);
        for (int32_t y = spine; y >= 0; y = m->plink(y)) on_path[y] = 1;
        std::vector<int32_t> ids, outs;
        std::vector<double> cen, rad;
        for (int32_t k = 0; k < c->n_spheres; ++k) {
            if (done[k] || !on_path[anchor[k]]) continue;
            done[k] = 1;
            --left;
            ids.push_back(c->sphere_link_ids[k]);
            outs.push_back(k);
            rad.push_back(c->radii[k]);
            for (int i = 0; i < 3; ++i) cen.push_back(c->centers ? c->centers[3 * k + i] : 0.0);
        }
        kin_coll_desc sub{c->dtype, c->n_q, c->q_joint_ids, (int32_t)ids.size(), ids.data(), cen.data(), rad.data()};
        kin_plan_desc d{c->dtype, c->n_q, c->q_joint_ids, 0, nullptr, spine + 1, c->n_q, c->q_joint_ids, 0};
        auto P = std::make_unique<kin_plan>();
        if (const int rc = stage_plan(*m, d, &sub, outs.data(), *P, (int32_t)pose_here.size(), pose_here.data())) return rc;
        if (with_pose && P->geom.maxA > kTrajPoseMaxChain)
            return set_error(KIN_E_UNSUPPORTED, fn + ": the chain to the deepest sphere / pose link has more than " +
                                                    std::to_string(kTrajPoseMaxChain) + " steps");
        parts.push_back(std::move(P));
    }
    for (int32_t k = 0; k < n_pose; ++k)
        if (pose_at[k].first < 0)
            return set_error(KIN_E_UNSUPPORTED, fn + ": pose link " + std::to_string(k) +
                                                    " is on another branch than the sphere chain");
    // the top plan's pose links in the caller's order, each with the part that carries it (staged above, part by part)
    std::vector<kin_plan::PoseLink> pose_links;
    for (int32_t k = 0; k < n_pose; ++k) {
        kin_plan::PoseLink pl = parts[pose_at[k].first]->pose_links[pose_at[k].second];
        pl.part = pose_at[k].first;
        pose_links.push_back(pl);
    }
    for (auto& P : parts)  // (nothing was uploaded before the last refusal above)
        if (const int rc = upload_plan(*P)) return rc;
    std::unique_ptr<kin_plan> top;
    if (parts.size() == 1) {
        top = std::move(parts[0]);
        if (const int rc = upload_traj_parts(*top, fn)) return rc;
    } else {
        top = std::make_unique<kin_plan>();
        top->dtype = parts[0]->dtype;
        top->nqcols = parts[0]->nqcols;
        top->with_base = parts[0]->with_base;
        top->n_q = parts[0]->n_q;
        top->is_coll = true;
        top->device = parts[0]->device;
        top->n_sph = c->n_spheres;
        top->parts = std::move(parts);
        if (const int rc = upload_traj_parts(*top, fn)) return rc;
    }
    top->n_sph = c->n_spheres;
    top->pose_links = std::move(pose_links);
    for (int32_t k = 0; k < c->n_q; ++k) {  // (kin_traj_opt_batch clamps to these)
        top->col_lo.push_back(m->jlo[c->q_joint_ids[k] - 1]);
        top->col_hi.push_back(m->jhi[c->q_joint_ids[k] - 1]);
    }
    *out = top.release();
    return KIN_OK;
}
}  // namespace

int kin_coll_plan_create(const kin_model* m, const kin_coll_desc* c, kin_plan** out) {
    return coll_plan_create(m, c, 0, nullptr, out, "kin_coll_plan_create");
}

int kin_traj_plan_create(const kin_model* m, const kin_coll_desc* c, int32_t n_pose_links, const int32_t* pose_link_ids,
                         kin_plan** out) {
    if (n_pose_links < 1 || !pose_link_ids)
        return set_error(KIN_E_INVALID, "kin_traj_plan_create: need >= 1 pose link (kin_coll_plan_create otherwise)");
    if (n_pose_links > kTrajMaxPoseLinks)
        return set_error(KIN_E_UNSUPPORTED, "kin_traj_plan_create: more than " + std::to_string(kTrajMaxPoseLinks) +
                                                " pose links");
    return coll_plan_create(m, c, n_pose_links, pose_link_ids, out, "kin_traj_plan_create");
}

namespace {
// the staged tree program to the device: [steps | spheres] in one allocation
int upload_ikc_tree(kin_plan& P) {
    P.ikc_sph_off = (P.h_ikc_steps.size() + 255) / 256 * 256;
    return upload(&P.d_ikc, {{P.h_ikc_steps.data(), P.h_ikc_steps.size(), 0},
                             {P.h_ikc_sph.data(), P.h_ikc_sph.size(), P.ikc_sph_off}});
}
}  // namespace

int kin_coll_ik_plan_create(const kin_model* m, const kin_coll_desc* c, int32_t link_id, kin_plan** out) {
    if (!m || !c || !out) return set_error(KIN_E_INVALID, "kin_coll_ik_plan_create: null argument");
    if (c->n_spheres < 0 || (c->n_spheres && (!c->sphere_link_ids || !c->radii)))
        return set_error(KIN_E_INVALID, "kin_coll_ik_plan_create: spheres need link ids and radii");
    if (c->n_q < 1 || !c->q_joint_ids) return set_error(KIN_E_INVALID, "kin_coll_ik_plan_create: no q joints");
    const int32_t out_ids[1] = {link_id};
    // an IK plan of `link` over the q joints (stage 1: get_jacobian! over them, geometric rows) ...
    kin_plan_desc d{c->dtype, c->n_q, c->q_joint_ids, 1, out_ids, link_id, c->n_q, c->q_joint_ids, KIN_WITH_ROT};
    auto P = std::make_unique<kin_plan>();
    // ... and the tree of the target link and every sphere (stage 2, k_ik_tree; staged on the host first)
    int rc = stage_ikc_tree(*m, c, link_id, *P);
    if (rc != KIN_OK) return rc;
    rc = stage_plan(*m, d, nullptr, nullptr, *P);
    if (rc != KIN_OK) return rc;
    if (!P->ik_ok) return set_error(KIN_E_INVALID, "kin_coll_ik_plan_create: " + P->ik_why);
    rc = upload_plan(*P);
    if (rc != KIN_OK) return rc;
    rc = upload_ikc_tree(*P);
    if (rc != KIN_OK) return rc;
    P->is_coll_ik = true;
    P->n_sph = c->n_spheres;
    *out = P.release();
    return KIN_OK;
}

namespace {
int ik_coll_batch(const kin_plan* p, const kin_sdf* sdf, const kin_ik_params* prm, const kin_ik_coll_params* cp,
                  const void* target, int64_t ldt, const void* scene_q, int64_t lds, bool scene, const void* q0,
                  const void* q_alt, void* q, int64_t ldq, int64_t n, int32_t* iters, void* err, int64_t lde, void* stream,
                  const char* fn) {
    auto bad = [&](int code, const std::string& w) { return set_error(code, std::string(fn) + ": " + w); };
    if (!p || !sdf || !prm || !cp) return bad(KIN_E_INVALID, "null argument");
    if (!p->is_coll_ik) return bad(KIN_E_INVALID, "plan was not made by kin_coll_ik_plan_create");
    if (sdf->attached && !scene) return bad(KIN_E_INVALID, "the kin_sdf is attached to a scene: use kin_ik_coll_batch_scene");
    if (!sdf->attached && scene) return bad(KIN_E_INVALID, "the kin_sdf is not attached to a scene (use kin_ik_coll_batch)");
    if (n < 0) return bad(KIN_E_INVALID, "n < 0");
    if (n == 0) return KIN_OK;
    if (!target || ldt < n || !q || ldq < n || (err && lde < n)) return bad(KIN_E_INVALID, "bad pointer / stride");
    if (scene && sdf->scene_cols > 0 && (!scene_q || (lds != 0 && lds < n))) return bad(KIN_E_INVALID, "bad scene_q / lds");
    if (const int rc = check_device(p->device, fn, "the plan")) return rc;
    if (const int rc = check_device(sdf->device, fn, "the kin_sdf")) return rc;
    if (prm->max_iters < 0 || !(prm->lambda > 0) || !(prm->max_step > 0) || prm->restarts < 0 ||
        prm->with_rot < 0 || prm->with_rot > 2 || prm->index_base < 0)
        return bad(KIN_E_INVALID, "bad IK parameters (lambda must be > 0)");
    if (prm->damp_err != 0.0) return bad(KIN_E_INVALID, "kin_ik_params.damp_err must be 0 for the collision-aware IK");
    if (!std::isfinite(cp->margin) || !(cp->band >= 0) || !(cp->weight > 0) || !(cp->feas >= 0))
        return bad(KIN_E_INVALID, "bad collision parameters");
    if (prm->lanes != 0 && prm->lanes != 1 && prm->lanes != 2 && prm->lanes != 4 && prm->lanes != 8 &&
        prm->lanes != 16 && prm->lanes != 64)
        return bad(KIN_E_INVALID, "kin_ik_params.lanes must be 0 (auto), 1, 2, 4, 8, 16 or 64");
    IkArgs a{prm->max_iters, prm->lambda, prm->tol_pos, prm->tol_rot, prm->max_step, prm->with_rot,
             prm->restarts, prm->seed, prm->lanes, prm->index_base, 0.0};
    a.q_alt = q_alt;
    const IkcArgs c{cp->margin, cp->band, cp->weight, cp->feas};
    const CollArgs ca{INFINITY, 0.0, sdf->n_boxes, sdf->n_aabb, 0, 0, {sdf->bc[0], sdf->bc[1], sdf->bc[2]},
                      {sdf->bh[0], sdf->bh[1], sdf->bh[2]}};
    const bool f32 = p->dtype == KIN_F32;
    const void* sc = f32 ? sdf->d_scene_f32 : sdf->d_scene_f64;
    const SceneLaunch sl{sc, sc ? (const char*)sc + sdf->scene_steps_off : nullptr, scene_q, lds, sdf->n_groups,
                         sdf->scene_base_col, lds == 0 ? 1 : 0};
    const JitFns* jf = jit_fns(p->jit);  // (the specialised kernels take the static union only)
    const void* st = p->d_ikc;
    const void* sp = (const char*)p->d_ikc + p->ikc_sph_off;
    const hipError_t e = by_dtype(p->dtype, [&](auto t) {
        using T = decltype(t);
        return launch_ik_tree<T>(p->ikc<T>(), (const KIkcStep<T>*)st, (const KSphere<T>*)sp, sdf->boxes<T>(), ca,
                                 scene ? &sl : nullptr, c, a, (const T*)target, ldt, (const T*)(q0 == q ? nullptr : q0),
                                 (T*)q, ldq, n, iters, (T*)err, lde, jf, (hipStream_t)stream);
    });
    if (e != hipSuccess) return set_error(KIN_E_DEVICE, std::string("k_ik_tree launch: ") + hipGetErrorString(e));
    return KIN_OK;
}
}  // namespace

int kin_ik_coll_batch(const kin_plan* p, const kin_sdf* sdf, const kin_ik_params* prm, const kin_ik_coll_params* cp,
                      const void* target, int64_t ldt, const void* q0, void* q, int64_t ldq, int64_t n, int32_t* iters,
                      void* err, int64_t lde, void* stream) {
    return ik_coll_batch(p, sdf, prm, cp, target, ldt, nullptr, 0, false, q0, nullptr, q, ldq, n, iters, err, lde,
                         stream, "kin_ik_coll_batch");
}

int kin_ik_coll_batch_scene(const kin_plan* p, const kin_sdf* sdf, const kin_ik_params* prm,
                            const kin_ik_coll_params* cp, const void* target, int64_t ldt, const void* scene_q,
                            int64_t lds, const void* q0, void* q, int64_t ldq, int64_t n, int32_t* iters, void* err,
                            int64_t lde, void* stream) {
    return ik_coll_batch(p, sdf, prm, cp, target, ldt, scene_q, lds, true, q0, nullptr, q, ldq, n, iters, err, lde,
                         stream, "kin_ik_coll_batch_scene");
}

int kin_ik_coll_batch_alt(const kin_plan* p, const kin_sdf* sdf, const kin_ik_params* prm,
                          const kin_ik_coll_params* cp, const void* target, int64_t ldt, const void* scene_q,
                          int64_t lds, const void* q0, const void* q_alt, void* q, int64_t ldq, int64_t n,
                          int32_t* iters, void* err, int64_t lde, void* stream) {
    return ik_coll_batch(p, sdf, prm, cp, target, ldt, scene_q, lds, sdf && sdf->attached, q0, q_alt, q, ldq, n,
                         iters, err, lde, stream, "kin_ik_coll_batch_alt");
}

namespace {
// k_coll over every chain program of a collision plan; min_dist accumulates after the first
int coll_launch(const kin_plan* p, const kin_sdf* sdf, CollArgs a, const void* q, int64_t ldq, int64_t n, void* dists,
                int64_t ldd, void* grads, int64_t ldg, void* min_dist, const TileArgs& ta, void* stream) {
    const size_t np = p->parts.empty() ? 1 : p->parts.size();
    // the specialised kernels address rows through the scalar offset (KINHIP_COLL_SOFF): every row
    // offset plus the lane span must stay below 2^31 bytes, else the generic kernels run
    const int64_t esz = p->dtype == KIN_F32 ? 4 : 8;
    const bool tiled = ta.tile < n;
    const int64_t span = tiled ? ta.tile : std::min<int64_t>(n, kChunk);
    const auto fits = [&](int64_t rows, int64_t ld) { return ((rows + 1) * (tiled ? ta.tile : ld) + span) * esz < (int64_t(1) << 31); };
    const bool soff = fits(p->nqcols, ldq) && (!dists || fits(p->n_sph, ldd)) &&
                      (!grads || fits((int64_t)p->n_sph * p->nqcols, ldg));
    for (size_t k = 0; k < np; ++k) {
        const kin_plan* s = p->parts.empty() ? p : p->parts[k].get();
        a.accumulate = k > 0;
        const JitFns* jf = soff ? jit_fns(s->jit) : nullptr;
        const hipError_t e = by_dtype(s->dtype, [&](auto t) {
            using T = decltype(t);
            return launch_coll<T>(s->prog<T>(), s->steps<T>(), s->sph<T>(), sdf->boxes<T>(), s->geom, a, (const T*)q, ldq,
                                  n, (T*)dists, ldd, (T*)grads, ldg, (T*)min_dist, ta, jf, (hipStream_t)stream);
        });
        if (e != hipSuccess) return set_error(KIN_E_DEVICE, std::string("k_coll launch: ") + hipGetErrorString(e));
    }
    return KIN_OK;
}

CollArgs coll_args(const kin_sdf* sdf, double truncation, double offset) {
    return CollArgs{truncation, offset, sdf->n_boxes, sdf->n_aabb, 0, 0, {sdf->bc[0], sdf->bc[1], sdf->bc[2]},
                    {sdf->bh[0], sdf->bh[1], sdf->bh[2]}};
}

// shared checks of the collision entry points; ta.tile >= n is the plain layout
int coll_check(const kin_plan* p, const kin_sdf* sdf, const void* q, int64_t ldq, int64_t tsq, int64_t n,
               const void* out1, int64_t ld1, int64_t ts1, int rows1, const void* out2, int64_t ld2, int64_t ts2,
               int rows2, const TileArgs& ta, const char* fn) {
    auto bad = [&](const char* what) { return set_error(KIN_E_INVALID, std::string(fn) + ": " + what); };
    if (!p || !sdf) return bad("null plan / sdf");
    if (!p->is_coll) return bad("plan was not made by kin_coll_plan_create");
    if (sdf->attached) return bad("the kin_sdf is attached to a scene: use kin_coll_batch_scene");
    if (n < 0) return bad("n < 0");
    if (n == 0) return KIN_OK;
    if (const int rc = check_device(p->device, fn, "the plan")) return rc;
    if (const int rc = check_device(sdf->device, fn, "the kin_sdf")) return rc;
    const int64_t span = std::min(ta.tile, n);
    if ((p->nqcols > 0 && (!q || ldq < span)) || (out1 && ld1 < span) || (out2 && ld2 < span))
        return bad("bad pointer / stride");
    if (ta.tile < n) {
        if (ta.tile < 256 || ta.tile % 256 || ta.tile > (int64_t(1) << 26)) return bad("tile must be a multiple of 256 <= 2^26");
        if ((p->nqcols > 0 && tsq < p->nqcols * ldq) || (out1 && ts1 < rows1 * ld1) || (out2 && ts2 < rows2 * ld2))
            return bad("tile strides overlap");
    }
    return KIN_OK;
}
}  // namespace

int kin_coll_batch(const kin_plan* p, const kin_sdf* sdf, double truncation, const void* q, int64_t ldq, int64_t n,
                   void* dists, int64_t ldd, void* grads, int64_t ldg, void* min_dist, void* stream) {
    const TileArgs ta = plain_soa(n);
    const int rc = coll_check(p, sdf, q, ldq, 0, n, dists, ldd, 0, 0, grads, ldg, 0, 0, ta, "kin_coll_batch");
    if (rc != KIN_OK || n == 0) return rc;
    return coll_launch(p, sdf, coll_args(sdf, truncation, 0.0), q, ldq, n, dists, ldd, grads, ldg, min_dist, ta,
                       stream);
}

int kin_coll_batch_scene(const kin_plan* p, const kin_sdf* sdf, double truncation, const void* q, int64_t ldq,
                         const void* scene_q, int64_t lds, int64_t n, void* dists, int64_t ldd, void* grads, int64_t ldg,
                         void* min_dist, void* stream) {
    auto bad = [](const std::string& w) { return set_error(KIN_E_INVALID, "kin_coll_batch_scene: " + w); };
    if (!p || !sdf) return bad("null plan / sdf");
    if (!p->is_coll) return bad("plan was not made by kin_coll_plan_create");
    if (!sdf->attached) return bad("the kin_sdf is not attached to a scene (use kin_coll_batch)");
    if (n < 0) return bad("n < 0");
    if (n == 0) return KIN_OK;
    if (sdf->scene_cols > 0 && (!scene_q || (lds != 0 && lds < n))) return bad("bad scene_q / lds");
    if ((p->nqcols > 0 && (!q || ldq < n)) || (dists && ldd < n) || (grads && ldg < n)) return bad("bad pointer / stride");
    if (const int rc = check_device(p->device, "kin_coll_batch_scene", "the plan")) return rc;
    if (const int rc = check_device(sdf->device, "kin_coll_batch_scene", "the kin_sdf")) return rc;
    CollArgs a = coll_args(sdf, truncation, 0.0);
    const size_t np = p->parts.empty() ? 1 : p->parts.size();
    // the specialised kernels' soffset row addressing (as coll_launch): every row offset plus the lane
    // span below 2^31 bytes, else the generic kernels
    const int64_t esz = p->dtype == KIN_F32 ? 4 : 8, span = std::min<int64_t>(n, kChunk);
    const auto fits = [&](int64_t rows, int64_t ld) { return ((rows + 1) * ld + span) * esz < (int64_t(1) << 31); };
    const bool soff = fits(p->nqcols, ldq) && (!dists || fits(p->n_sph, ldd)) &&
                      (!grads || fits((int64_t)p->n_sph * p->nqcols, ldg));
    for (size_t k = 0; k < np; ++k) {
        const kin_plan* s = p->parts.empty() ? p : p->parts[k].get();
        a.accumulate = k > 0;
        const JitFns* jf = soff ? jit_fns(s->jit) : nullptr;
        const JitFns* jfs = soff ? s->scene_fns(sdf->uid) : nullptr;  // (kin_plan_specialize_scene)
        const void* sc = s->dtype == KIN_F32 ? sdf->d_scene_f32 : sdf->d_scene_f64;
        const SceneLaunch sl{sc, (const char*)sc + sdf->scene_steps_off, scene_q, lds, sdf->n_groups,
                             sdf->scene_base_col, lds == 0 ? 1 : 0};
        const hipError_t e = by_dtype(s->dtype, [&](auto t) {
            using T = decltype(t);
            return launch_coll_scene<T>(s->prog<T>(), s->steps<T>(), s->sph<T>(), sdf->boxes<T>(), s->geom, a, sl,
                                        (const T*)q, ldq, n, (T*)dists, ldd, (T*)grads, ldg, (T*)min_dist, jf, jfs,
                                        (hipStream_t)stream);
        });
        if (e != hipSuccess) return set_error(KIN_E_DEVICE, std::string("k_coll_scene launch: ") + hipGetErrorString(e));
    }
    return KIN_OK;
}

int kin_ineq_const_batch(const kin_plan* p, const kin_sdf* sdf, double margin, const void* q, int64_t ldq, int64_t n,
                         void* vals, int64_t ldv, void* jac, int64_t ldj, void* stream) {
    if (!std::isfinite(margin)) return set_error(KIN_E_INVALID, "kin_ineq_const_batch: margin must be finite");
    if (!vals) return set_error(KIN_E_INVALID, "kin_ineq_const_batch: null vals");
    const TileArgs ta = plain_soa(n > 0 ? n : 1);
    const int ndof = p ? p->nqcols : 0;
    const int rc = coll_check(p, sdf, q, ldq, 0, n, vals, ldv, 0, p ? p->n_sph : 0, jac, ldj, 0,
                              p ? p->n_sph * ndof : 0, ta, "kin_ineq_const_batch");
    if (rc != KIN_OK || n == 0) return rc;
    // src/planning.jl:56, :66: truncation_dist = margin + 0.05; val = dist - margin
    return coll_launch(p, sdf, coll_args(sdf, margin + 0.05, margin), q, ldq, n, vals, ldv, jac, ldj, nullptr, ta,
                       stream);
}

int kin_pose_const_batch(const kin_plan* p, const void* target, int64_t ldt, const void* q, int64_t ldq, int64_t n,
                         void* poses, int64_t ldp, void* vals, int64_t ldv, void* jac, int64_t ldj, void* stream) {
    if (!p) return set_error(KIN_E_INVALID, "kin_pose_const_batch: null plan");
    if (p->is_coll || p->n_out != 1 || !p->has_jac || p->out_link0 != p->jac_link)
        return set_error(KIN_E_INVALID, "kin_pose_const_batch: plan needs n_out = 1 and a Jacobian of that same link");
    if (p->rows == 6 && !p->has_rpy)
        return set_error(KIN_E_INVALID, "kin_pose_const_batch: with_rot plans need KIN_RPY_JAC (rpy_jac=true)");
    if (n < 0) return set_error(KIN_E_INVALID, "n < 0");
    if (n == 0) return KIN_OK;
    if (!target || ldt < n || !vals || ldv < n) return set_error(KIN_E_INVALID, "kin_pose_const_batch: bad target / vals");
    int rc = kin_plan_run(p, q, ldq, n, poses, ldp, jac, ldj, stream);
    if (rc != KIN_OK) return rc;
    const hipError_t e = by_dtype(p->dtype, [&](auto t) {
        using T = decltype(t);
        return launch_pose_residual<T>((const T*)poses, ldp, (const T*)target, ldt, n, p->rows, (T*)vals, ldv,
                                       (hipStream_t)stream);
    });
    if (e != hipSuccess) return set_error(KIN_E_DEVICE, std::string("k_pose_residual launch: ") + hipGetErrorString(e));
    return KIN_OK;
}

// One scratch set's layout: kIkSubRings rings of 2 * cap / kIkSubRings entries (a phase-1 launch spreads its
// hand-overs over the rings by wave; twice the even share covers the uneven last waves), list + aux, and the
// rings' control words (one 128-byte line each)
constexpr int64_t kIkRingCap = 2 * IkSets::kIkScratchCap / kIkSubRings;
constexpr size_t kIkCtlBytes = sizeof(uint32_t) * kIkCtlStride * kIkSubRings;
constexpr size_t kIkSetBytes = kIkCtlBytes + 2 * sizeof(int32_t) * (size_t)(kIkRingCap * kIkSubRings);
static IkScratch ik_scratch_at(unsigned char* base) {
    IkScratch scr;
    scr.fail_ctl = (uint32_t*)base;
    scr.fail_list = (int32_t*)(base + kIkCtlBytes);
    scr.fail_aux = scr.fail_list + kIkRingCap * kIkSubRings;
    scr.cap = IkSets::kIkScratchCap;
    scr.ring_cap = kIkRingCap;
    return scr;
}

// kin_last_error / status of a failed IkSets::acquire
static int ik_sets_error(const IkSets::Lease& l) {
    switch (l.fail) {
    case IkSets::kFirstCallInCapture:
        return set_error(KIN_E_INVALID, "kin_ik_dls_batch: the plan's first two-phase call allocates its "
                                        "scratch and cannot run inside a stream capture (make one call "
                                        "outside the capture first, or pass lanes > 0)");
    case IkSets::kAlloc: return set_error(KIN_E_DEVICE, std::string("hipMalloc: ") + hipGetErrorString(l.error));
    case IkSets::kEventCreate:
        return set_error(KIN_E_DEVICE, std::string("kin_ik_dls_batch: two-phase scratch set: ") + hipGetErrorString(l.error));
    default:
        return set_error(KIN_E_DEVICE, std::string("kin_ik_dls_batch: two-phase scratch ordering: ") + hipGetErrorString(l.error));
    }
}

static int ik_dls_batch(const kin_plan* p, const kin_ik_params* prm, const void* target, int64_t ldt, const void* q0,
                        void* q, int64_t ldq, int64_t n, int32_t* iters, void* err, int64_t lde, void* stream,
                        void* trace = nullptr, int64_t ldtr = 0) {
    if (!p || !prm) return set_error(KIN_E_INVALID, "kin_ik_dls_batch: null argument");
    if (!p->ik_ok) return set_error(KIN_E_INVALID, "kin_ik_dls_batch: plan not usable for IK: " + p->ik_why);
    if (n < 0) return set_error(KIN_E_INVALID, "n < 0");
    if (n == 0) return KIN_OK;
    if (!target || ldt < n || !q || ldq < n || (err && lde < n)) return set_error(KIN_E_INVALID, "bad pointer / stride");
    if (const int rc = check_device(p->device, "kin_ik_dls_batch", "the plan")) return rc;
    if (prm->max_iters < 0 || !(prm->lambda >= 0) || !(prm->max_step > 0) || prm->restarts < 0)
        return set_error(KIN_E_INVALID, "bad IK parameters");
    if (prm->with_rot < 0 || prm->with_rot > 2)
        return set_error(KIN_E_INVALID, "kin_ik_params.with_rot must be 0, 1 or 2 (reference rpy objective)");
    if (prm->lanes != 0 && prm->lanes != 1 && prm->lanes != 2 && prm->lanes != 4 && prm->lanes != 8)
        return set_error(KIN_E_INVALID, "kin_ik_params.lanes must be 0 (auto), 1, 2, 4 or 8");
    if (prm->index_base < 0) return set_error(KIN_E_INVALID, "kin_ik_params.index_base < 0");
    if (!(prm->damp_err >= 0) || !std::isfinite(prm->damp_err))
        return set_error(KIN_E_INVALID, "kin_ik_params.damp_err must be finite and >= 0");
    IkArgs a{prm->max_iters, prm->lambda, prm->tol_pos, prm->tol_rot, prm->max_step, prm->with_rot,
             prm->restarts, prm->seed, prm->lanes, prm->index_base, prm->damp_err};
    if (trace) {  // kin_ik_dls_batch_trace: one lane per target, attempts in sequence (rows by iteration)
        if (ldtr < n) return set_error(KIN_E_INVALID, "kin_ik_dls_batch_trace: ldtr < n");
        a.lanes = 1;
        a.trace = trace;
        a.trace_ld = ldtr;
    }
    // the specialised IK kernels address rows with 32-bit offsets (ldn_soa): every lane offset of a
    // launch chunk plus rows * ld must stay below 2^31 bytes, else the generic kernel runs
    const int64_t esz = p->dtype == KIN_F32 ? 4 : 8;
    const int64_t span = std::min<int64_t>(n, kIkChunk);
    const bool narrow = (12 * ldt + span) * esz < (int64_t(1) << 31) && (p->nqcols * ldq + span) * esz < (int64_t(1) << 31) &&
                        (2 * lde + span) * esz < (int64_t(1) << 31);
    const JitFns* jf = narrow ? jit_fns(p->jit) : nullptr;
    // two-phase schedule scratch (small batches with restarts; launch_ik_dls): only a call that runs
    // that schedule touches it, so every other call stays allocation-free (capture-safe)
    IkScratch scr;
    IkSets::Lease lease;  // the scratch set taken by this call (released after the launch)
    if (ik_wants_two_phase(a, n, IkSets::kIkScratchCap)) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess) cs = hipStreamCaptureStatusNone;
        lease = p->ik_sets.acquire(stream, cs == hipStreamCaptureStatusActive, kIkSetBytes);
        if (lease.fail) return ik_sets_error(lease);
        if (lease.set() >= 0) scr = ik_scratch_at(lease.base());  // (no set left: one phase)
    }
    const hipError_t e = by_dtype(p->dtype, [&](auto t) {
        using T = decltype(t);
        return launch_ik_dls<T>(p->prog<T>(), p->steps<T>(), p->geom, a, (const T*)target, ldt, (const T*)q0, (T*)q, ldq,
                                n, iters, (T*)err, lde, jf, scr, (hipStream_t)stream);
    });
    lease.commit(stream);
    if (e != hipSuccess)
        return set_error(KIN_E_DEVICE, std::string("k_ik_dls launch: ") + hipGetErrorString(e) +
                                           (ik_last_call_partial() ? " (phase 2 failed to launch after phase 1: the "
                                                                     "outputs of the targets phase 1 did not solve are "
                                                                     "undefined)"
                                                                   : ""));
    return KIN_OK;
}

int kin_ik_dls_batch(const kin_plan* p, const kin_ik_params* prm, const void* target, int64_t ldt, void* q,
                     int64_t ldq, int64_t n, int32_t* iters, void* err, int64_t lde, void* stream) {
    return ik_dls_batch(p, prm, target, ldt, nullptr, q, ldq, n, iters, err, lde, stream);
}

int kin_ik_dls_batch_from(const kin_plan* p, const kin_ik_params* prm, const void* target, int64_t ldt, const void* q0,
                          void* q, int64_t ldq, int64_t n, int32_t* iters, void* err, int64_t lde, void* stream) {
    if (!q0) return set_error(KIN_E_INVALID, "kin_ik_dls_batch_from: null q0");
    return ik_dls_batch(p, prm, target, ldt, q0 == q ? nullptr : q0, q, ldq, n, iters, err, lde, stream);
}

int kin_ik_dls_batch_trace(const kin_plan* p, const kin_ik_params* prm, const void* target, int64_t ldt,
                           const void* q0, void* q, int64_t ldq, int64_t n, int32_t* iters, void* trace, int64_t ldtr,
                           void* stream) {
    if (!q0 || !trace) return set_error(KIN_E_INVALID, "kin_ik_dls_batch_trace: null q0 / trace");
    return ik_dls_batch(p, prm, target, ldt, q0 == q ? nullptr : q0, q, ldq, n, iters, nullptr, 0, stream, trace, ldtr);
}

int kin_plan_ik_sched_stats(const kin_plan* p, kin_ik_sched_stats* out) {
    if (!p || !out) return set_error(KIN_E_INVALID, "kin_plan_ik_sched_stats: null plan / out");
    *out = p->ik_sets.stats();
    return KIN_OK;
}

int kin_point_ik_nakamura_batch(const kin_plan* p, const void* pts, int64_t ldpt, void* q, int64_t ldq, int64_t n,
                                void* stream) {
    if (!p) return set_error(KIN_E_INVALID, "null plan");
    if (!p->ik_ok || p->with_base)
        return set_error(KIN_E_INVALID, "kin_point_ik_nakamura_batch: plan needs jac joints == q joints, no base");
    if (n < 0) return set_error(KIN_E_INVALID, "n < 0");
    if (n == 0) return KIN_OK;
    if (!pts || ldpt < n || !q || ldq < n) return set_error(KIN_E_INVALID, "bad pointer / stride");
    if (const int rc = check_device(p->device, "kin_point_ik_nakamura_batch", "the plan")) return rc;
    const hipError_t e = by_dtype(p->dtype, [&](auto t) {
        using T = decltype(t);
        return launch_nakamura<T>(p->prog<T>(), p->steps<T>(), p->geom, (const T*)pts, ldpt, (T*)q, ldq, n,
                                  jit_fns(p->jit), (hipStream_t)stream);
    });
    if (e != hipSuccess) return set_error(KIN_E_DEVICE, std::string("k_nakamura launch: ") + hipGetErrorString(e));
    return KIN_OK;
}

}  // extern "C"
