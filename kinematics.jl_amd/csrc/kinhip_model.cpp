// kinhip_model.cpp -- models (Mechanism trees) behind the C-ABI: tree validation, rptable, add_link,
// the per-model plan cache and the kin_model_* / kin_get_*_batch entry points.
//
// Reference semantics restated here (host side):
//   Mechanism / create_rptable / is_relevant   src/mechanism.jl:117-181, 277
//   joint_transform (static parts, fp64)       src/mechanism.jl:90-103
//   set_joint_angles column layout             src/mechanism.jl:223-231
//   add_new_link                                src/mechanism.jl:238-267
#include <algorithm>
#include <cmath>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "kinhip_plan.h"

namespace kinhip {

static thread_local std::string g_err;

int set_error(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

}  // namespace kinhip

namespace {

int validate_tree(const kin_tree_desc* d) {
    if (!d) return set_error(KIN_E_INVALID, "kin_model_create: null desc");
    if (d->n_links < 1 || d->n_joints < 0) return set_error(KIN_E_INVALID, "kin_model_create: bad sizes");
    if (d->n_joints > 0 && (!d->joint_type || !d->joint_plink || !d->joint_clink || !d->joint_pose || !d->joint_axis))
        return set_error(KIN_E_INVALID, "kin_model_create: null joint arrays");
    std::vector<int> parents(d->n_links, 0);
    for (int32_t j = 0; j < d->n_joints; ++j) {
        const int32_t t = d->joint_type[j];
        if (t != KIN_JOINT_FIXED && t != KIN_JOINT_REVOLUTE && t != KIN_JOINT_PRISMATIC)
            return set_error(KIN_E_INVALID, "kin_model_create: joint " + std::to_string(j + 1) + " has unknown type");
        const int32_t p = d->joint_plink[j], c = d->joint_clink[j];
        if (p < 1 || p > d->n_links || c < 1 || c > d->n_links)
            return set_error(KIN_E_KEY, "kin_model_create: joint " + std::to_string(j + 1) + " link id out of range");
        if (++parents[c - 1] > 1)
            return set_error(KIN_E_INVALID, "kin_model_create: link " + std::to_string(c) + " has two parent joints");
    }
    return KIN_OK;
}

int finish_model(kin_model* m) {
    const int32_t L = m->n_links, J = m->n_joints();
    m->link_pjoint.assign(L, -1);
    m->child_joints.assign(L, {});
    for (int32_t j = 0; j < J; ++j) {
        m->link_pjoint[m->jclink[j] - 1] = j;
        m->child_joints[m->jplink[j] - 1].push_back(j);
    }
    for (int32_t l = 0; l < L; ++l) {  // cycle check
        int32_t x = l, guard = 0;
        while (x >= 0) {
            if (++guard > L + 1) return set_error(KIN_E_INVALID, "kin_model_create: the joint graph has a cycle");
            x = m->plink(x);
        }
    }
    return KIN_OK;
}

std::string cache_key(const kin_model* m, const kin_plan_desc& d) {
    std::ostringstream k;
    int dev = -1;
    (void)hipGetDevice(&dev);  // one cached plan per device (kin_get_*_batch from several devices)
    k << dev << '#' << m->version << '|' << d.dtype << '|' << d.jac_link_id << '|' << d.jac_flags << "|q";
    for (int32_t c = 0; c < d.n_q; ++c) k << ',' << d.q_joint_ids[c];
    k << "|o";
    for (int32_t c = 0; c < d.n_out; ++c) k << ',' << d.out_link_ids[c];
    k << "|j";
    for (int32_t c = 0; c < d.n_jac; ++c) k << ',' << d.jac_joint_ids[c];
    return k.str();
}

int cached_plan(kin_model* m, const kin_plan_desc& d, kin_plan** out) {
    const std::string key = cache_key(m, d);
    std::lock_guard<std::mutex> g(m->mu);
    auto it = m->cache.find(key);
    if (it != m->cache.end()) {
        *out = it->second;
        return KIN_OK;
    }
    kin_plan* p = nullptr;
    const int rc = plan_create(m, &d, &p);
    if (rc != KIN_OK) return rc;
    m->cache[key] = p;
    *out = p;
    return KIN_OK;
}

void clear_cache(kin_model* m) {
    std::lock_guard<std::mutex> g(m->mu);
    for (auto& kv : m->cache) delete kv.second;
    m->cache.clear();
}

}  // namespace

extern "C" {

int kin_abi_version(void) { return KINHIP_ABI_VERSION; }

const char* kin_last_error(void) { return g_err.c_str(); }

int kin_limits(int32_t* max_chain, int32_t* max_jac_cols, int32_t* max_slots) {
    if (max_chain) *max_chain = kMaxChain;
    if (max_jac_cols) *max_jac_cols = kMaxJacCols;
    if (max_slots) *max_slots = kMaxSlots;
    return KIN_OK;
}

int kin_model_create(const kin_tree_desc* d, kin_model** out) {
    if (!out) return set_error(KIN_E_INVALID, "kin_model_create: null out");
    int rc = validate_tree(d);
    if (rc != KIN_OK) return rc;
    auto m = std::make_unique<kin_model>();
    const int32_t J = d->n_joints;
    m->n_links = d->n_links;
    m->jtype.assign(d->joint_type, d->joint_type + J);
    m->jplink.assign(d->joint_plink, d->joint_plink + J);
    m->jclink.assign(d->joint_clink, d->joint_clink + J);
    m->jpose.assign(d->joint_pose, d->joint_pose + 16 * (size_t)J);
    m->jaxis.assign(d->joint_axis, d->joint_axis + 3 * (size_t)J);
    m->jlo.resize(J);
    m->jhi.resize(J);
    for (int32_t j = 0; j < J; ++j) {
        m->jlo[j] = d->joint_lower ? d->joint_lower[j] : -INFINITY;
        m->jhi[j] = d->joint_upper ? d->joint_upper[j] : INFINITY;
    }
    m->angles.assign(J, 0.0);
    m->with_base = d->with_base != 0;
    rc = finish_model(m.get());
    if (rc != KIN_OK) return rc;
    *out = m.release();
    return KIN_OK;
}

int kin_model_destroy(kin_model* m) {
    if (!m) return KIN_OK;
    clear_cache(m);
    delete m;
    return KIN_OK;
}

int kin_model_num_links(const kin_model* m, int32_t* out) {
    if (!m || !out) return set_error(KIN_E_INVALID, "null argument");
    *out = m->n_links;
    return KIN_OK;
}

int kin_model_num_joints(const kin_model* m, int32_t* out) {
    if (!m || !out) return set_error(KIN_E_INVALID, "null argument");
    *out = m->n_joints();
    return KIN_OK;
}

int kin_model_set_angles(kin_model* m, const double* angles) {
    if (!m) return set_error(KIN_E_INVALID, "null model");
    if (angles) m->angles.assign(angles, angles + m->n_joints());
    else m->angles.assign(m->n_joints(), 0.0);
    clear_cache(m);
    m->version++;
    return KIN_OK;
}

int kin_model_is_relevant(const kin_model* m, int32_t joint_id, int32_t link_id, int32_t* out) {
    if (!m || !out) return set_error(KIN_E_INVALID, "null argument");
    if (joint_id < 1 || joint_id > m->n_joints()) return set_error(KIN_E_KEY, "joint id out of range");
    if (link_id < 1 || link_id > m->n_links) return set_error(KIN_E_KEY, "link id out of range");
    *out = m->relevant(joint_id - 1, link_id - 1) ? 1 : 0;
    return KIN_OK;
}

int kin_model_add_link(kin_model* m, int32_t parent, const double* pose16, int32_t* new_id) {
    if (!m || !pose16) return set_error(KIN_E_INVALID, "null argument");
    if (parent < 1 || parent > m->n_links) return set_error(KIN_E_KEY, "parent link id out of range");
    m->n_links += 1;
    m->jtype.push_back(KIN_JOINT_FIXED);
    m->jplink.push_back(parent);
    m->jclink.push_back(m->n_links);
    m->jpose.insert(m->jpose.end(), pose16, pose16 + 16);
    const double ax[3] = {1, 0, 0};
    m->jaxis.insert(m->jaxis.end(), ax, ax + 3);
    m->jlo.push_back(-INFINITY);
    m->jhi.push_back(INFINITY);
    m->angles.push_back(0.0);
    const int rc = finish_model(m);
    if (rc != KIN_OK) return rc;
    clear_cache(m);
    m->version++;
    if (new_id) *new_id = m->n_links;
    return KIN_OK;
}

int kin_get_transform_batch(kin_model* m, int32_t dtype, int32_t n_q, const int32_t* qids, const void* q,
                            int64_t ldq, int64_t n, int32_t n_out, const int32_t* out_ids, void* poses, int64_t ldp,
                            void* stream) {
    if (!m) return set_error(KIN_E_INVALID, "null model");
    kin_plan_desc d{dtype, n_q, qids, n_out, out_ids, 0, 0, nullptr, 0};
    kin_plan* p;
    const int rc = cached_plan(m, d, &p);
    if (rc != KIN_OK) return rc;
    if (n_out > 0 && !poses) return set_error(KIN_E_INVALID, "null poses");
    return kin_plan_run(p, q, ldq, n, poses, ldp, nullptr, 0, stream);
}

int kin_get_jacobian_batch(kin_model* m, int32_t dtype, int32_t link_id, int32_t n_joints, const int32_t* jids,
                           uint32_t flags, const void* q, int64_t ldq, int64_t n, void* pose, int64_t ldp, void* jac,
                           int64_t ldj, void* stream) {
    if (!m) return set_error(KIN_E_INVALID, "null model");
    if (link_id == 0) return set_error(KIN_E_KEY, "link id 0");
    const int32_t out_ids[1] = {link_id};
    kin_plan_desc d{dtype, n_joints, jids, pose ? 1 : 0, out_ids, link_id, n_joints, jids, flags};
    kin_plan* p;
    const int rc = cached_plan(m, d, &p);
    if (rc != KIN_OK) return rc;
    return kin_plan_run(p, q, ldq, n, pose, ldp, jac, ldj, stream);
}

}  // extern "C"
