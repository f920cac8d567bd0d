// kinhip_sdf.cpp -- signed-distance unions of boxes behind the C-ABI (kin_sdf): static boxes and boxes
// attached to a scene mechanism.
#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "kinhip_plan.h"

namespace {
// Signed axis permutation test for a box rotation (columns of R = box axes in
// the world).  perm[i] = world axis of box axis i.
bool axis_permutation(const double* pose16, int perm[3]) {
    int used = 0;
    for (int i = 0; i < 3; ++i) {
        perm[i] = -1;
        for (int j = 0; j < 3; ++j) {
            const double a = std::fabs(pose16[4 * i + j]);  // column-major: R[j][i]
            if (a > 1e-12 && std::fabs(a - 1.0) > 1e-12) return false;
            if (a > 0.5) {
                if (perm[i] >= 0) return false;
                perm[i] = j;
            }
        }
        if (perm[i] < 0 || (used & (1 << perm[i]))) return false;
        used |= 1 << perm[i];
    }
    return true;
}

// [KBox<T> boxes | KAabb<T> axis-aligned boxes] in one device allocation
template <typename T>
int upload_boxes(void** dst, const std::vector<KBox<T>>& b, const std::vector<KAabb<T>>& a, const char* fn) {
    const size_t nb = sizeof(KBox<T>) * b.size();
    return upload(dst, {{b.data(), nb, 0}, {a.data(), sizeof(KAabb<T>) * a.size(), nb}}, fn);
}
}  // namespace

extern "C" {

int kin_sdf_create_boxes(int32_t n_boxes, const double* poses16, const double* widths3, kin_sdf** out) {
    if (!out || n_boxes < 1 || !poses16 || !widths3)
        return set_error(KIN_E_INVALID, "kin_sdf_create_boxes: need >= 1 box and non-null arrays");
    for (int32_t k = 0; k < 3 * n_boxes; ++k)
        if (!(widths3[k] >= 0)) return set_error(KIN_E_INVALID, "kin_sdf_create_boxes: negative / NaN width");
    auto sd = std::make_unique<kin_sdf>();
    sd->n_boxes = n_boxes;
    // axis-aligned boxes first (their own order), then the rotated ones
    std::vector<int32_t> order;
    std::vector<std::array<int, 3>> perms(n_boxes);
    for (int32_t k = 0; k < n_boxes; ++k)
        if (axis_permutation(poses16 + 16 * k, perms[k].data())) order.push_back(k);
    sd->n_aabb = (int32_t)order.size();
    for (int32_t k = 0; k < n_boxes; ++k)
        if (!axis_permutation(poses16 + 16 * k, perms[k].data())) order.push_back(k);
    std::vector<KBox<float>> bf(n_boxes);
    std::vector<KBox<double>> bd(n_boxes);
    std::vector<KAabb<float>> af(sd->n_aabb);
    std::vector<KAabb<double>> ad(sd->n_aabb);
    for (int32_t o = 0; o < n_boxes; ++o) {
        const int32_t k = order[o];
        const double* P = poses16 + 16 * k;
        const M34 inv = m_rigid_inverse(m_from_col16(P));  // BoxSDF.inv_pose (src/sdf.jl:60)
        to_row12<float>(inv, bf[o].inv);
        to_row12<double>(inv, bd[o].inv);
        for (int i = 0; i < 3; ++i) {
            bf[o].half[i] = (float)(0.5 * widths3[3 * k + i]);
            bd[o].half[i] = 0.5 * widths3[3 * k + i];
        }
        bf[o].pad = 0;
        bd[o].pad = 0;
        if (o < sd->n_aabb) {
            for (int i = 0; i < 3; ++i) {
                const int j = perms[k][i];  // box axis i lies along world axis j
                ad[o].c[i] = P[12 + i];
                af[o].c[i] = (float)P[12 + i];
                ad[o].half[j] = 0.5 * widths3[3 * k + i];
                af[o].half[j] = (float)(0.5 * widths3[3 * k + i]);
            }
            ad[o].pad[0] = ad[o].pad[1] = 0;
            af[o].pad[0] = af[o].pad[1] = 0;
        }
    }
    {  // enclosing world-aligned box of all box corners
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        std::vector<std::array<double, 3>> corners;
        for (int32_t k = 0; k < n_boxes; ++k) {
            const double* P = poses16 + 16 * k;  // column-major 4x4
            for (int c = 0; c < 8; ++c) {
                const double l[3] = {(c & 1 ? 0.5 : -0.5) * widths3[3 * k], (c & 2 ? 0.5 : -0.5) * widths3[3 * k + 1],
                                     (c & 4 ? 0.5 : -0.5) * widths3[3 * k + 2]};
                std::array<double, 3> w;
                for (int i = 0; i < 3; ++i) {
                    w[i] = P[12 + i] + P[i] * l[0] + P[4 + i] * l[1] + P[8 + i] * l[2];
                    lo[i] = std::min(lo[i], w[i]);
                    hi[i] = std::max(hi[i], w[i]);
                }
                corners.push_back(w);
            }
        }
        for (int i = 0; i < 3; ++i) {
            sd->bc[i] = 0.5 * (lo[i] + hi[i]);
            sd->bh[i] = 0.5 * (hi[i] - lo[i]) * (1.0 + 1e-12) + 1e-12;
        }
    }
    const char* fn = "kin_sdf_create_boxes";
    const hipError_t e = hipGetDevice(&sd->device);
    if (e != hipSuccess) return set_error(KIN_E_DEVICE, std::string(fn) + ": " + hipGetErrorString(e));
    if (const int rc = upload_boxes(&sd->d_f32, bf, af, fn)) return rc;
    if (const int rc = upload_boxes(&sd->d_f64, bd, ad, fn)) return rc;
    *out = sd.release();
    return KIN_OK;
}

int kin_sdf_destroy(kin_sdf* s) {
    delete s;
    return KIN_OK;
}

int kin_sdf_create_attached(const kin_model* scene, int32_t n_q, const int32_t* q_joint_ids, int32_t n_boxes,
                            const int32_t* link_ids, const double* origins16, const double* widths3, kin_sdf** out) {
    auto bad = [](int code, const std::string& w) { return set_error(code, "kin_sdf_create_attached: " + w); };
    if (!scene || !out || n_boxes < 1 || !link_ids || !origins16 || !widths3 || n_q < 0 || (n_q && !q_joint_ids))
        return bad(KIN_E_INVALID, "null argument / no boxes");
    const kin_model& m = *scene;
    const int32_t J = m.n_joints(), L = m.n_links;
    std::vector<int32_t> qcol(J, -1);
    for (int32_t c = 0; c < n_q; ++c) {
        const int32_t j = q_joint_ids[c] - 1;
        if (j < 0 || j >= J) return bad(KIN_E_KEY, "scene joint id out of range");
        if (m.jtype[j] != KIN_JOINT_FIXED) qcol[j] = c;
    }
    for (int32_t k = 0; k < 3 * n_boxes; ++k)
        if (!(widths3[k] >= 0)) return bad(KIN_E_INVALID, "negative / NaN width");
    // per box: the group (last batch joint on its root path, -1: the root / base frame) and its pose in
    // the group frame (static joints at the scene's angles folded in, fp64, as joint_transform does)
    struct BoxS { int32_t group; M34 pose; int32_t src; };
    std::vector<BoxS> bs(n_boxes);
    std::vector<int32_t> group_key;  // joint (0-based) or -1
    for (int32_t k = 0; k < n_boxes; ++k) {
        const int32_t l = link_ids[k] - 1;
        if (l < 0 || l >= L) return bad(KIN_E_KEY, "box link id out of range");
        std::vector<int32_t> path;  // joints root .. l
        for (int32_t x = l; x >= 0 && m.link_pjoint[x] >= 0; x = m.plink(x)) path.push_back(m.link_pjoint[x]);
        std::reverse(path.begin(), path.end());
        int32_t last = -1;
        for (size_t p = 0; p < path.size(); ++p)
            if (qcol[path[p]] >= 0) last = (int32_t)p;
        M34 S = m_identity();
        for (size_t p = last + 1; p < path.size(); ++p) S = m_mul(S, m.joint_tf(path[p], m.angles[path[p]]));
        const int32_t key = last >= 0 ? path[last] : -1;
        auto it = std::find(group_key.begin(), group_key.end(), key);
        if (it == group_key.end()) {
            group_key.push_back(key);
            it = group_key.end() - 1;
        }
        bs[k] = BoxS{(int32_t)(it - group_key.begin()), m_mul(S, m_from_col16(origins16 + 16 * k)), k};
    }
    if ((int)group_key.size() > kMaxSceneGroups)
        return bad(KIN_E_UNSUPPORTED, "boxes ride on " + std::to_string(group_key.size()) + " moving frames (max " +
                                          std::to_string(kMaxSceneGroups) + ")");
    // group chains: static products up to each batch joint, then its motion (joint_transform)
    std::vector<KSceneGroup> groups(group_key.size());
    struct StepS { M34 F; double axis[3]; int32_t kind, qcol; };
    std::vector<StepS> steps;
    for (size_t g = 0; g < group_key.size(); ++g) {
        groups[g].step0 = (int32_t)steps.size();
        const int32_t key = group_key[g];
        if (key >= 0) {
            std::vector<int32_t> path;
            for (int32_t x = m.jclink[key] - 1; x >= 0 && m.link_pjoint[x] >= 0; x = m.plink(x)) path.push_back(m.link_pjoint[x]);
            std::reverse(path.begin(), path.end());
            M34 S = m_identity();
            for (int32_t j : path) {
                if (qcol[j] >= 0) {
                    StepS st;
                    st.F = m_mul(S, m.pose(j));
                    const double* ax = &m.jaxis[3 * j];
                    const double nn = sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
                    for (int i = 0; i < 3; ++i) st.axis[i] = nn > 0 ? ax[i] / nn : 0.0;
                    st.kind = m.jtype[j] == KIN_JOINT_PRISMATIC ? MOT_PRISM : MOT_REV;
                    st.qcol = qcol[j];
                    if (st.kind == MOT_PRISM) for (int i = 0; i < 3; ++i) st.axis[i] = ax[i];  // axis * q, unnormalised
                    steps.push_back(st);
                    S = m_identity();
                } else {
                    S = m_mul(S, m.joint_tf(j, m.angles[j]));
                }
            }
        }
        groups[g].step1 = (int32_t)steps.size();
    }
    // boxes sorted by group, axis-aligned ones first within a group
    std::vector<int32_t> order;
    std::vector<std::array<int, 3>> perms(n_boxes);
    std::vector<char> aa(n_boxes, 0);
    for (int32_t k = 0; k < n_boxes; ++k) {
        double P16[16] = {0};
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) P16[i + 4 * j] = bs[k].pose.r[3 * i + j];
            P16[12 + i] = bs[k].pose.t[i];
        }
        P16[15] = 1;
        aa[k] = axis_permutation(P16, perms[k].data());
    }
    std::vector<KBox<float>> bf;
    std::vector<KBox<double>> bd;
    std::vector<KAabb<float>> af;
    std::vector<KAabb<double>> ad;
    for (size_t g = 0; g < groups.size(); ++g) {
        groups[g].box0 = (int32_t)bf.size();
        groups[g].aabb0 = (int32_t)af.size();
        std::vector<int32_t> mem;
        for (int32_t k = 0; k < n_boxes; ++k)
            if (bs[k].group == (int32_t)g && aa[k]) mem.push_back(k);
        groups[g].na = (int32_t)mem.size();
        for (int32_t k = 0; k < n_boxes; ++k)
            if (bs[k].group == (int32_t)g && !aa[k]) mem.push_back(k);
        groups[g].nb = (int32_t)mem.size();
        {  // the group frame's box enclosing its boxes (|R| h around t), rounded outward to float
            double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (int32_t k : mem)
                for (int i = 0; i < 3; ++i) {
                    double e = 0;
                    for (int j = 0; j < 3; ++j) e += fabs(bs[k].pose.r[3 * i + j]) * 0.5 * widths3[3 * k + j];
                    lo[i] = std::min(lo[i], bs[k].pose.t[i] - e);
                    hi[i] = std::max(hi[i], bs[k].pose.t[i] + e);
                }
            for (int i = 0; i < 3; ++i) {
                const double c = 0.5 * (lo[i] + hi[i]), h = 0.5 * (hi[i] - lo[i]);
                groups[g].bc[i] = (float)c;
                groups[g].bh[i] = (float)(h + 1e-6 * (fabs(c) + h) + 1e-6);
            }
        }
        for (size_t o = 0; o < mem.size(); ++o) {
            const int32_t k = mem[o];
            const M34 inv = m_rigid_inverse(bs[k].pose);
            KBox<float> xf{};
            KBox<double> xd{};
            to_row12<float>(inv, xf.inv);
            to_row12<double>(inv, xd.inv);
            for (int i = 0; i < 3; ++i) {
                xf.half[i] = (float)(0.5 * widths3[3 * k + i]);
                xd.half[i] = 0.5 * widths3[3 * k + i];
            }
            bf.push_back(xf);
            bd.push_back(xd);
            if ((int32_t)o < groups[g].na) {
                KAabb<float> yf{};
                KAabb<double> yd{};
                for (int i = 0; i < 3; ++i) {
                    const int j = perms[k][i];
                    yd.c[i] = bs[k].pose.t[i];
                    yf.c[i] = (float)bs[k].pose.t[i];
                    yd.half[j] = 0.5 * widths3[3 * k + i];
                    yf.half[j] = (float)(0.5 * widths3[3 * k + i]);
                }
                af.push_back(yf);
                ad.push_back(yd);
            }
        }
    }
    auto sd = std::make_unique<kin_sdf>();
    sd->attached = true;
    sd->n_boxes = n_boxes;
    sd->n_aabb = 0;
    sd->n_groups = (int32_t)groups.size();
    sd->scene_cols = n_q + (m.with_base ? 3 : 0);
    sd->scene_base_col = m.with_base ? n_q : -1;
    sd->scene_steps_off = ((sizeof(KSceneGroup) * groups.size() + 255) / 256) * 256;
    const char* fn = "kin_sdf_create_attached";
    // [KSceneGroup groups | KSceneStep<T> steps at scene_steps_off] in one device allocation
    auto upload_scene = [&](auto tag, void** dst) -> int {
        using T = decltype(tag);
        std::vector<KSceneStep<T>> hs(std::max<size_t>(1, steps.size()));
        memset(hs.data(), 0, sizeof(KSceneStep<T>) * hs.size());
        for (size_t k = 0; k < steps.size(); ++k) {
            to_row12<T>(steps[k].F, hs[k].F);
            for (int i = 0; i < 3; ++i) hs[k].axis[i] = (T)steps[k].axis[i];
            hs[k].kind = steps[k].kind;
            hs[k].qcol = steps[k].qcol;
        }
        if constexpr (sizeof(T) == 4) sd->h_ssf.assign(hs.begin(), hs.begin() + steps.size());
        else sd->h_ssd.assign(hs.begin(), hs.begin() + steps.size());
        return upload(dst, {{groups.data(), sizeof(KSceneGroup) * groups.size(), 0},
                            {hs.data(), sizeof(KSceneStep<T>) * hs.size(), sd->scene_steps_off}}, fn);
    };
    sd->h_groups = groups;
    sd->h_bf = bf;
    sd->h_bd = bd;
    sd->h_af = af;
    sd->h_ad = ad;
    static std::atomic<uint64_t> sdf_uids{0};
    sd->uid = ++sdf_uids;
    const hipError_t e = hipGetDevice(&sd->device);
    if (e != hipSuccess) return bad(KIN_E_DEVICE, hipGetErrorString(e));
    if (const int rc = upload_boxes(&sd->d_f32, bf, af, fn)) return rc;
    if (const int rc = upload_boxes(&sd->d_f64, bd, ad, fn)) return rc;
    if (const int rc = upload_scene(float(), &sd->d_scene_f32)) return rc;
    if (const int rc = upload_scene(double(), &sd->d_scene_f64)) return rc;
    *out = sd.release();
    return KIN_OK;
}

}  // extern "C"
