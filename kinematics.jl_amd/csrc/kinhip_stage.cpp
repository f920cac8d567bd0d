// kinhip_stage.cpp -- plan staging: a model and a plan description into the host copy of the device
// program (kinhip_prog.h).  Host arithmetic only: no runtime call, the caller uploads (kinhip_host.cpp).
//
// Reference semantics restated here (host side):
//   joint_transform (static parts, fp64)       src/mechanism.jl:90-103
//   set_joint_angles column layout             src/mechanism.jl:223-231
//   get_jacobian! column relevance / errors    src/algorithm.jl:83-106
#include <algorithm>
#include <functional>
#include <map>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "kinhip_plan.h"

namespace {

// rotation A with A e_z = unit axis (exact for signed basis axes)
M34 align_z(const double* a, double* scale) {
    const double n = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    *scale = n;
    if (n == 0.0) return m_identity();
    const double z[3] = {a[0] / n, a[1] / n, a[2] / n};
    if (z[0] == 0.0 && z[1] == 0.0 && z[2] == 1.0) return m_identity();
    double h[3] = {0, 0, 1};
    if (fabs(z[2]) >= 0.9) { h[0] = 1; h[2] = 0; }
    double u[3] = {h[1] * z[2] - h[2] * z[1], h[2] * z[0] - h[0] * z[2], h[0] * z[1] - h[1] * z[0]};
    const double un = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    for (double& v : u) v /= un;
    const double v[3] = {z[1] * u[2] - z[2] * u[1], z[2] * u[0] - z[0] * u[2], z[0] * u[1] - z[1] * u[0]};
    M34 A{};
    for (int i = 0; i < 3; ++i) {
        A.r[3 * i + 0] = u[i];
        A.r[3 * i + 1] = v[i];
        A.r[3 * i + 2] = z[i];
    }
    return A;
}

struct SD {  // staged step, fp64
    M34 F, X;
    bool hasX = false;
    double scale = 1, lo = -INFINITY, hi = INFINITY;
    int32_t kind = MOT_NONE, jkind = MOT_NONE, qcol = -1, flags = 0, out = -1, load = LOAD_NONE, save = -1;
    int32_t sph0 = 0, sph1 = 0;
    uint64_t colmask = 0;
};

struct SphD {  // staged collision sphere
    int32_t step;  // phase-A step whose frame carries it (-1: root frame)
    double c[3];   // centre in that (canonical) frame
    double r;
    int32_t out;
};

struct Stager {
    const kin_model& m;
    const kin_plan_desc& d;
    std::vector<int32_t> qcol;
    std::vector<char> moving, rec, needed, node;
    std::vector<uint64_t> colmask;
    std::vector<std::vector<int32_t>> outs_of, cchildren;  // per link
    std::vector<M34> Xinv;
    std::vector<char> hasX;
    std::vector<SD> steps;
    uint64_t zmask = 0;
    std::vector<int32_t> chain, chain_step;  // phase-A nodes root..spine and their edge steps (-1: none)
    // collision plans
    const kin_coll_desc* coll = nullptr;
    const int32_t* sph_out = nullptr;  // global sphere index of each desc sphere (multi-chain plans)
    std::vector<SphD> spheres;
    int32_t sph_root0 = 0, sph_root1 = 0;
    int32_t n_pose = 0;  // kin_traj_plan_create: pose links (1-based ids)
    const int32_t* pose_ids = nullptr;
    // a static last edge into the spine folded into Xlast (no step): the spine link and the
    // transform from the previous chain node's canonical frame to it (spheres on the spine, k_ik_coll)
    int32_t fold_spine = -1;
    M34 fold_X = m_identity();
    // LDS slots
    std::vector<int> slot_of_link, slot_refs;
    std::vector<int> free_slots;
    int n_slots = 0;

    Stager(const kin_model& m_, const kin_plan_desc& d_) : m(m_), d(d_) {}

    int alloc_slot() {
        if (!free_slots.empty()) {
            int s = free_slots.back();
            free_slots.pop_back();
            return s;
        }
        slot_refs.push_back(0);
        return n_slots++;
    }
    void consume(int slot) {
        if (slot >= 0 && --slot_refs[slot] == 0) free_slots.push_back(slot);
    }

    int32_t cparent(int32_t v) const {  // nearest node ancestor (compressed parent), -1 for roots
        for (int32_t x = m.plink(v); x >= 0; x = m.plink(x))
            if (node[x]) return x;
        return -1;
    }

    // edge u -> v (v a node); appends the edge step and duplicate-output steps
    void emit_edge(int32_t v, int32_t load) {
        SD st;
        st.load = load;
        std::vector<int32_t> path;  // joints from cparent(v) down to v
        for (int32_t x = v; x >= 0 && !(x != v && node[x]); x = m.plink(x))
            if (m.link_pjoint[x] >= 0) path.push_back(m.link_pjoint[x]);
        const int32_t u = cparent(v);
        if (u < 0 || path.empty()) {  // v is a root: pseudo-step on the root frame
            st.F = m_identity();
            Xinv[v] = m_identity();
            hasX[v] = 0;
        } else {
            M34 S = hasX[u] ? Xinv[u] : m_identity();
            for (size_t k = path.size() - 1; k >= 1; --k) S = m_mul(S, m.joint_tf(path[k], m.angles[path[k]]));
            const int32_t jm = path[0];
            if (moving[jm] || rec[jm]) {
                double scale;
                const M34 A = align_z(&m.jaxis[3 * jm], &scale);
                st.F = m_mul(m_mul(S, m.pose(jm)), A);
                st.scale = scale;
                st.jkind = m.jtype[jm] == KIN_JOINT_PRISMATIC ? MOT_PRISM : MOT_REV;
                st.lo = m.jlo[jm];
                st.hi = m.jhi[jm];
                if (rec[jm]) {
                    st.flags |= SF_REC;
                    st.colmask = colmask[jm];
                }
                if (moving[jm]) {
                    st.kind = st.jkind;
                    st.qcol = qcol[jm];
                    if (st.kind == MOT_REV && scale != 1.0) st.flags |= SF_SCALE;
                    Xinv[v] = m_rot_transpose(A);
                } else {
                    Xinv[v] = m_mul(m_rot_transpose(A), m.motion_at(jm, m.angles[jm]));
                }
                hasX[v] = !m_is_identity(Xinv[v]);
            } else {
                st.F = m_mul(S, m.joint_tf(jm, m.angles[jm]));
                Xinv[v] = m_identity();
                hasX[v] = 0;
            }
        }
        st.X = Xinv[v];
        st.hasX = hasX[v];
        if (st.hasX) st.flags |= SF_HAS_X;
        const auto& o = outs_of[v];
        st.out = o.empty() ? -1 : o[0];
        steps.push_back(st);
        for (size_t k = 1; k < o.size(); ++k) {  // same link requested again: identity pseudo-steps
            SD dup;
            dup.F = m_identity();
            dup.X = st.X;
            dup.hasX = st.hasX;
            dup.flags = st.hasX ? SF_HAS_X : 0;
            dup.out = o[k];
            steps.push_back(dup);
        }
    }

    void emit_subtree(int32_t v, int32_t load) {
        emit_edge(v, load);
        const size_t edge_step = steps.size() - 1 - (outs_of[v].size() > 1 ? outs_of[v].size() - 1 : 0);
        const auto& ch = cchildren[v];
        if (ch.empty()) return;
        int slot = -1;
        if (ch.size() >= 2) {
            slot = alloc_slot();
            slot_refs[slot] = (int)ch.size() - 1;
            steps[edge_step].save = slot;
        }
        emit_subtree(ch[0], LOAD_NONE);
        for (size_t k = 1; k < ch.size(); ++k) {
            emit_subtree_loaded(ch[k], slot);
        }
    }
    void emit_subtree_loaded(int32_t v, int slot) {
        emit_subtree(v, slot);
        consume(slot);
    }

    // spheres = links (src/collision.jl:39-49), each carried by the nearest chain node above it;
    // the static path from that node (and the node's canonical-frame correction) is folded into
    // the centre, in fp64
    // The chain frame carrying link lk (0-based): its phase-A step (-1: the root frame) and S, the static
    // transform from that (canonical) frame down to lk.  `what` names the link in the messages.
    int carrier(int32_t lk, int32_t sroot, const std::string& what, int32_t* step, M34* S_out) {
        const int32_t L = m.n_links;
        std::vector<int32_t> on_chain(L, -1);
        for (size_t k = 0; k < chain.size(); ++k) on_chain[chain[k]] = (int32_t)k;
        std::vector<int32_t> path;
        int32_t x = lk;
        while (x >= 0 && on_chain[x] < 0) {
            const int32_t j = m.link_pjoint[x];
            if (j < 0) break;
            if (moving[j])
                return set_error(KIN_E_UNSUPPORTED, "coll plan: " + what + " hangs off a moving joint outside the chain");
            path.push_back(j);
            x = m.plink(x);
        }
        if (x < 0 || on_chain[x] < 0) return set_error(KIN_E_UNSUPPORTED, "coll plan: " + what + " is on another tree");
        M34 S = hasX[x] ? Xinv[x] : m_identity();
        if (x == fold_spine) {  // the spine has no step: carried by the node above it
            S = fold_X;
            x = chain[on_chain[x] - 1];
        }
        for (size_t pi = path.size(); pi-- > 0;) S = m_mul(S, m.joint_tf(path[pi], m.angles[path[pi]]));
        *step = (x == sroot) ? -1 : chain_step[on_chain[x]];
        if (x != sroot && *step < 0) return set_error(KIN_E_INVALID, "coll plan: internal (no step)");
        *S_out = S;
        return KIN_OK;
    }

    // kin_traj_plan_create's pose links: a table of their own (kin_plan::pose_links), never pseudo-spheres
    int stage_pose_links(int32_t sroot, kin_plan& P) {
        for (int32_t k = 0; k < n_pose; ++k) {
            const int32_t lk = pose_ids[k] - 1;
            if (lk < 0 || lk >= m.n_links) return set_error(KIN_E_KEY, "traj plan: pose link id out of range");
            kin_plan::PoseLink pl;
            if (const int rc = carrier(lk, sroot, "pose link " + std::to_string(k), &pl.step, &pl.X)) return rc;
            P.pose_links.push_back(pl);
        }
        return KIN_OK;
    }

    int stage_spheres(int32_t sroot) {
        const int32_t L = m.n_links;
        for (int32_t k = 0; k < coll->n_spheres; ++k) {
            const int32_t lk = coll->sphere_link_ids[k] - 1;
            if (lk < 0 || lk >= L) return set_error(KIN_E_KEY, "coll plan: sphere link id out of range");
            int32_t cstep = -1;
            M34 S;
            if (const int rc = carrier(lk, sroot, "sphere " + std::to_string(k), &cstep, &S)) return rc;
            SphD sd;
            const double c0 = coll->centers ? coll->centers[3 * k] : 0.0;
            const double c1 = coll->centers ? coll->centers[3 * k + 1] : 0.0;
            const double c2 = coll->centers ? coll->centers[3 * k + 2] : 0.0;
            for (int i = 0; i < 3; ++i) sd.c[i] = S.r[3 * i] * c0 + S.r[3 * i + 1] * c1 + S.r[3 * i + 2] * c2 + S.t[i];
            sd.r = coll->radii[k];
            sd.out = sph_out ? sph_out[k] : k;
            sd.step = cstep;
            spheres.push_back(sd);
        }
        std::stable_sort(spheres.begin(), spheres.end(), [](const SphD& a, const SphD& b) { return a.step < b.step; });
        for (size_t k = 0; k < spheres.size(); ++k) {
            const int32_t st = spheres[k].step;
            if (st < 0) {
                sph_root1 = (int32_t)k + 1;
            } else {
                if (steps[st].sph1 == 0) steps[st].sph0 = (int32_t)k;
                steps[st].sph1 = (int32_t)k + 1;
            }
        }
        return KIN_OK;
    }

    int run(kin_plan& P) {
        const int32_t L = m.n_links, J = m.n_joints();
        if (d.dtype != KIN_F32 && d.dtype != KIN_F64) return set_error(KIN_E_INVALID, "plan: bad dtype");
        if (d.n_q < 0 || d.n_out < 0 || d.n_jac < 0) return set_error(KIN_E_INVALID, "plan: negative count");
        if ((d.n_q && !d.q_joint_ids) || (d.n_out && !d.out_link_ids) || (d.n_jac && !d.jac_joint_ids))
            return set_error(KIN_E_INVALID, "plan: null id array");
        qcol.assign(J, -1);
        for (int32_t c = 0; c < d.n_q; ++c) {
            const int32_t j = d.q_joint_ids[c] - 1;
            if (j < 0 || j >= J) return set_error(KIN_E_KEY, "plan: q joint id " + std::to_string(j + 1) + " out of range");
            qcol[j] = c;  // set_joint_angles: a repeated joint keeps the last value
        }
        moving.assign(J, 0);
        for (int32_t j = 0; j < J; ++j) moving[j] = qcol[j] >= 0 && m.jtype[j] != KIN_JOINT_FIXED;
        rec.assign(J, 0);
        colmask.assign(J, 0);
        const int32_t jl = d.jac_link_id - 1;
        const bool has_jac = d.jac_link_id != 0;
        if (has_jac) {
            if (jl < 0 || jl >= L) return set_error(KIN_E_KEY, "plan: jac link id out of range");
            if (d.n_jac > kMaxJacCols)
                return set_error(KIN_E_UNSUPPORTED, "plan: more than 64 Jacobian columns");
            for (int32_t c = 0; c < d.n_jac; ++c) {
                const int32_t j = d.jac_joint_ids[c] - 1;
                if (j < 0 || j >= J) return set_error(KIN_E_KEY, "plan: jac joint id out of range");
                if (m.relevant(j, jl)) {
                    if (m.jtype[j] == KIN_JOINT_FIXED)
                        return set_error(KIN_E_METHOD, "MethodError: no joint_jacobian! method for fixed joint " +
                                                           std::to_string(j + 1));
                    rec[j] = 1;
                    colmask[j] |= 1ull << c;
                } else {
                    zmask |= 1ull << c;
                }
            }
        } else if (d.n_jac) {
            return set_error(KIN_E_INVALID, "plan: Jacobian joints without a Jacobian link");
        }
        outs_of.assign(L, {});
        for (int32_t o = 0; o < d.n_out; ++o) {
            const int32_t l = d.out_link_ids[o] - 1;
            if (l < 0 || l >= L) return set_error(KIN_E_KEY, "plan: output link id out of range");
            outs_of[l].push_back(o);
        }
        needed.assign(L, 0);
        auto mark = [&](int32_t l) {
            for (int32_t x = l; x >= 0 && !needed[x]; x = m.plink(x)) needed[x] = 1;
        };
        for (int32_t o = 0; o < d.n_out; ++o) mark(d.out_link_ids[o] - 1);
        if (has_jac) mark(jl);
        // spine = the chain evaluated straight-line in registers (phase A): the
        // Jacobian link, else the needed link with the most moving joints above it
        int32_t spine = has_jac ? jl : -1;
        if (!has_jac) {
            int best = -1, best_depth = -1;
            for (int32_t o = 0; o < d.n_out; ++o) {
                const int32_t l = d.out_link_ids[o] - 1;
                int mv = 0, depth = 0;
                for (int32_t x = l; m.link_pjoint[x] >= 0; x = m.plink(x)) {
                    mv += moving[m.link_pjoint[x]];
                    ++depth;
                }
                if (mv > best || (mv == best && depth > best_depth)) {
                    best = mv;
                    best_depth = depth;
                    spine = l;
                }
            }
        }
        // nodes: links whose frame is materialised (roots, children of moving or
        // recorded joints, outputs, the spine); static branch points are folded
        node.assign(L, 0);
        for (int32_t l = 0; l < L; ++l) {
            if (!needed[l]) continue;
            const int32_t pj = m.link_pjoint[l];
            node[l] = pj < 0 || moving[pj] || rec[pj] || !outs_of[l].empty() || l == spine;
        }
        // compressed children in tree (joint) order
        cchildren.assign(L, {});
        std::vector<int32_t> roots;
        for (int32_t l = 0; l < L; ++l)
            if (needed[l] && m.link_pjoint[l] < 0) roots.push_back(l);
        for (int32_t r : roots) {
            std::vector<std::pair<int32_t, int32_t>> work{{r, -1}};  // (link, nearest node ancestor)
            while (!work.empty()) {
                auto [x, anc] = work.back();
                work.pop_back();
                if (node[x] && anc >= 0) cchildren[anc].push_back(x);
                const int32_t a2 = node[x] ? x : anc;
                const auto& cj = m.child_joints[x];
                for (auto it = cj.rbegin(); it != cj.rend(); ++it) {
                    const int32_t c = m.jclink[*it] - 1;
                    if (needed[c]) work.push_back({c, a2});
                }
            }
        }
        Xinv.assign(L, m_identity());
        hasX.assign(L, 0);

        // ---- phase A: root -> spine, straight-line, no loads ----
        std::vector<std::pair<int32_t, int32_t>> pending;  // (child node, parent node)
        int32_t sroot = -1;
        int32_t nA = 0, spine_out = -1;
        M34 Xl = m_identity();
        int32_t lhx = 0;
        slot_of_link.assign(L, -1);
        if (spine >= 0) {
            chain.clear();  // nodes root..spine
            for (int32_t x = spine; x >= 0; x = cparent(x)) chain.push_back(x);
            std::reverse(chain.begin(), chain.end());
            sroot = chain[0];
            const size_t K = chain.size() - 1;
            // a static last edge into a leaf spine folds into Xlast (no step)
            bool fold = false;
            if (K >= 1 && cchildren[spine].empty() && outs_of[spine].size() <= 1) {
                const int32_t pj = m.link_pjoint[spine];
                fold = !(moving[pj] || rec[pj]);
            }
            std::vector<int32_t> edge_step(chain.size(), -1);
            for (size_t k = 0; k < chain.size(); ++k) {
                const int32_t v = chain[k];
                if (k == K && fold) {
                    const int32_t u = chain[k - 1];
                    Xl = hasX[u] ? Xinv[u] : m_identity();
                    std::vector<int32_t> path;
                    for (int32_t x = v; x != u; x = m.plink(x)) path.push_back(m.link_pjoint[x]);
                    for (size_t p = path.size(); p-- > 0;) Xl = m_mul(Xl, m.joint_tf(path[p], m.angles[path[p]]));
                    lhx = !m_is_identity(Xl);
                    spine_out = outs_of[v].empty() ? -1 : outs_of[v][0];
                    fold_spine = v;
                    fold_X = Xl;
                } else if (k > 0 || !outs_of[v].empty()) {
                    edge_step[k] = (int32_t)steps.size();
                    emit_edge(v, LOAD_NONE);
                }
                const int32_t next = k < K ? chain[k + 1] : -1;
                for (int32_t c : cchildren[v])
                    if (c != next) pending.push_back({c, v});
            }
            if (!fold) {
                Xl = Xinv[spine];
                lhx = hasX[spine];
            }
            chain_step = edge_step;
            nA = (int32_t)steps.size();
            if (nA > kMaxChain)
                return set_error(KIN_E_UNSUPPORTED, "plan: root -> spine chain has " + std::to_string(nA) +
                                                        " steps (max " + std::to_string(kMaxChain) + ")");
            // slots for chain nodes with pending children (the root frame needs none)
            std::map<int32_t, int> cnt;
            for (auto& pc : pending) cnt[pc.second]++;
            for (size_t k = 0; k < chain.size(); ++k) {
                const int32_t v = chain[k];
                auto it = cnt.find(v);
                if (it == cnt.end() || v == sroot) continue;
                const int s = alloc_slot();
                slot_refs[s] = it->second;
                slot_of_link[v] = s;
                steps[edge_step[k]].save = s;
            }
            // pad to the compiled chain bound with identity steps
            const int32_t bound = pick_chain_bound(nA);
            while ((int32_t)steps.size() < bound) {
                SD pad;
                pad.F = m_identity();
                pad.X = m_identity();
                pad.scale = 0.0;
                steps.push_back(pad);
            }
            nA = bound;
        }
        if (coll) {
            const int rc = stage_spheres(sroot);
            if (rc != KIN_OK) return rc;
        }
        if (n_pose > 0) {
            const int rc = stage_pose_links(sroot, P);
            if (rc != KIN_OK) return rc;
        }
        // ---- phase B ----
        for (auto& pc : pending) {
            const int32_t v = pc.first, u = pc.second;
            if (u == sroot) {
                emit_subtree(v, LOAD_ROOT);
            } else {
                const int s = slot_of_link[u];
                emit_subtree(v, s);
                consume(s);
            }
        }
        for (int32_t r : roots) {
            if (r == sroot) continue;
            if (!outs_of[r].empty()) emit_edge(r, LOAD_ROOT);
            for (int32_t c : cchildren[r]) emit_subtree(c, LOAD_ROOT);
        }
        if (n_slots > kMaxSlots)
            return set_error(KIN_E_UNSUPPORTED, "plan: needs " + std::to_string(n_slots) + " LDS branch slots (max 8)");

        // ---- finalize ----
        P.dtype = d.dtype;
        P.with_base = m.with_base;
        P.n_q = d.n_q;
        P.n_out = d.n_out;
        P.nqcols = d.n_q + (m.with_base ? 3 : 0);
        P.has_jac = has_jac;
        P.rows = (d.jac_flags & KIN_WITH_ROT) ? 6 : 3;
        P.ncols = has_jac ? d.n_jac + (m.with_base ? 3 : 0) : 0;
        P.has_rpy = (d.jac_flags & KIN_RPY_JAC) != 0;
        P.out_link0 = d.n_out > 0 ? d.out_link_ids[0] : 0;
        P.jac_link = has_jac ? d.jac_link_id : 0;
        int32_t pflags = 0;
        if (has_jac) pflags |= PF_JAC;
        if (d.jac_flags & KIN_WITH_ROT) pflags |= PF_WITH_ROT;
        if (d.jac_flags & KIN_RPY_JAC) pflags |= PF_RPY;
        if (d.jac_flags & KIN_ZERO_FILL) pflags |= PF_ZERO;
        if (m.with_base) pflags |= PF_BASE;
        const size_t esz = d.dtype == KIN_F32 ? sizeof(float) : sizeof(double);
        int block = 256;
        while (block > 64 && (size_t)n_slots * 12 * block * esz > 64 * 1024) block /= 2;
        P.geom.block = block;
        P.geom.lds = (size_t)n_slots * 12 * block * esz;  // per-lane branch slots
        P.geom.maxA = nA;
        by_dtype(d.dtype, [&](auto t) {
            using T = decltype(t);
            P.h_steps.assign(std::max<size_t>(1, steps.size()) * sizeof(KStep<T>), 0);
            KProg<T>& K = P.prog<T>();
            KStep<T>* host = reinterpret_cast<KStep<T>*>(P.h_steps.data());
            K.nA = nA;
            K.nS = (int32_t)steps.size();
            K.n_slots = n_slots;
            K.rows = P.rows;
            K.n_jac = d.n_jac;
            K.flags = pflags;
            K.base_col = d.n_q;
            K.last_has_x = lhx;
            K.spine_out = spine_out;
            K.zmask = zmask;
            K.n_sph = (int32_t)spheres.size();
            K.sph_root0 = sph_root0;
            K.sph_root1 = sph_root1;
            to_row12<T>(Xl, K.Xlast);
            for (size_t s = 0; s < steps.size(); ++s) {
                const SD& a = steps[s];
                auto& b = host[s];
                memset(&b, 0, sizeof(b));
                to_row12<T>(a.F, b.F);
                to_row12<T>(a.X, b.X);
                b.scale = (T)a.scale;
                b.lo = (T)a.lo;
                b.hi = (T)a.hi;
                b.kind = a.kind;
                b.jkind = a.jkind;
                b.qcol = a.qcol;
                b.flags = a.flags;
                b.out = a.out;
                b.load = a.load;
                b.save = a.save;
                b.sph0 = a.sph0;
                b.sph1 = a.sph1;
                b.colmask = a.colmask;
            }
        });
        P.n_steps = (int32_t)steps.size();
        if (coll) {
            P.is_coll = true;
            P.n_sph = (int32_t)spheres.size();
            by_dtype(d.dtype, [&](auto t) {
                using TS = KSphere<decltype(t)>;
                P.h_sph.assign(sizeof(TS) * std::max<size_t>(1, spheres.size()), 0);
                TS* hs = reinterpret_cast<TS*>(P.h_sph.data());
                for (size_t k = 0; k < spheres.size(); ++k) {
                    for (int i = 0; i < 3; ++i) hs[k].c[i] = spheres[k].c[i];
                    hs[k].r = spheres[k].r;
                    hs[k].out = spheres[k].out;
                }
            });
        }

        // IK eligibility: Jacobian joints == q joints (same order, no repeats), no rpy rows
        P.ik_ok = has_jac && d.n_jac == d.n_q && !(d.jac_flags & KIN_RPY_JAC);
        if (P.ik_ok) {
            std::vector<char> seen(J, 0);
            for (int32_t c = 0; c < d.n_q; ++c) {
                if (d.q_joint_ids[c] != d.jac_joint_ids[c]) { P.ik_ok = false; P.ik_why = "jac joints != q joints"; }
                if (seen[d.q_joint_ids[c] - 1]++) { P.ik_ok = false; P.ik_why = "repeated joint"; }
            }
        } else {
            P.ik_why = "IK needs a Jacobian over the q joints without rpy rows";
        }
        return KIN_OK;
    }
};

// The collision-aware IK program (kinhip_prog.h KIkcProg / KIkcStep): every moving joint above the target
// link or above a sphere link, depth first in joint order; static chains folded on the host in fp64 as
// joint_transform does (src/mechanism.jl:90-103), frames canonical (joint axis on local z, as the Stager).
struct IkcStepD {
    M34 F;
    double scale = 1;
    int32_t kind = MOT_NONE, flags = 0, var = -1, parent_step = -1, save = -1, sph0 = 0, sph1 = 0;
    uint32_t anc = 0;
};
struct IkcSphD {
    int32_t step;  // carrier step (-1: root frame)
    double c[3], r;
    int32_t out;
};

}  // namespace

int kinhip::stage_plan(const kin_model& m, const kin_plan_desc& d, const kin_coll_desc* coll, const int32_t* sph_out,
                       kin_plan& P, int32_t n_pose, const int32_t* pose_ids) {
    Stager st(m, d);
    st.coll = coll;
    st.sph_out = sph_out;
    st.n_pose = n_pose;
    st.pose_ids = pose_ids;
    return st.run(P);
}

int kinhip::stage_ikc_tree(const kin_model& m, const kin_coll_desc* c, int32_t link_id, kin_plan& P) {
    const int32_t L = m.n_links, J = m.n_joints();
    const int32_t tl = link_id - 1;
    if (tl < 0 || tl >= L) return set_error(KIN_E_KEY, "kin_coll_ik_plan_create: link id out of range");
    const int32_t nq = c->n_q, base_col = m.with_base ? nq : -1;
    const int32_t nv = nq + (m.with_base ? 3 : 0);
    if (nv > kIkcMaxVars)
        return set_error(KIN_E_UNSUPPORTED, "kin_coll_ik_plan_create: " + std::to_string(nv) + " variables (q columns + base; max " +
                                                std::to_string(kIkcMaxVars) + ")");
    if (c->n_spheres > kIkcMaxSpheres)
        return set_error(KIN_E_UNSUPPORTED, "kin_coll_ik_plan_create: more than " + std::to_string(kIkcMaxSpheres) + " spheres");
    std::vector<int32_t> qcol(J, -1);
    for (int32_t k = 0; k < nq; ++k) {
        const int32_t j = c->q_joint_ids[k] - 1;
        if (j < 0 || j >= J) return set_error(KIN_E_KEY, "kin_coll_ik_plan_create: q joint id out of range");
        qcol[j] = k;  // set_joint_angles: a repeated joint keeps the last column
    }
    std::vector<char> needed(L, 0);
    auto mark = [&](int32_t l) {
        for (int32_t x = l; x >= 0 && !needed[x]; x = m.plink(x)) needed[x] = 1;
    };
    mark(tl);
    std::vector<std::vector<int32_t>> sph_of(L);
    for (int32_t k = 0; k < c->n_spheres; ++k) {
        const int32_t lk = c->sphere_link_ids[k] - 1;
        if (lk < 0 || lk >= L) return set_error(KIN_E_KEY, "kin_coll_ik_plan_create: sphere link id out of range");
        mark(lk);
        sph_of[lk].push_back(k);
    }
    const uint32_t base_bits = m.with_base ? (7u << base_col) : 0u;
    std::vector<IkcStepD> steps;
    std::vector<IkcSphD> spheres;
    int32_t tgt_step = kIkcRoot;
    M34 Xt = m_identity();
    uint32_t prism = 0, joints = 0;
    // depth first from every root: `carrier` = step whose post-motion canonical frame carries link x,
    // S = that frame -> link x (static)
    std::function<int(int32_t, int32_t, const M34&, uint32_t)> visit = [&](int32_t x, int32_t carrier, const M34& S,
                                                                            uint32_t anc) -> int {
        if (x == tl) {
            tgt_step = carrier < 0 ? kIkcRoot : carrier;
            Xt = S;
        }
        for (int32_t k : sph_of[x]) {
            IkcSphD sd;
            const double c0 = c->centers ? c->centers[3 * k] : 0.0;
            const double c1 = c->centers ? c->centers[3 * k + 1] : 0.0;
            const double c2 = c->centers ? c->centers[3 * k + 2] : 0.0;
            for (int i = 0; i < 3; ++i) sd.c[i] = S.r[3 * i] * c0 + S.r[3 * i + 1] * c1 + S.r[3 * i + 2] * c2 + S.t[i];
            sd.r = c->radii[k];
            sd.out = k;
            sd.step = carrier;
            spheres.push_back(sd);
        }
        for (int32_t j : m.child_joints[x]) {
            const int32_t ch = m.jclink[j] - 1;
            if (!needed[ch]) continue;
            const bool moving = qcol[j] >= 0 && m.jtype[j] != KIN_JOINT_FIXED;
            if (!moving) {  // static: folded (joint held at m.angles)
                const int rc = visit(ch, carrier, m_mul(S, m.joint_tf(j, m.angles[j])), anc);
                if (rc != KIN_OK) return rc;
                continue;
            }
            if ((int32_t)steps.size() >= kIkcMaxSteps)
                return set_error(KIN_E_UNSUPPORTED, "kin_coll_ik_plan_create: more than " + std::to_string(kIkcMaxSteps) +
                                                        " moving joints on the needed tree");
            double scale;
            const M34 A = align_z(&m.jaxis[3 * j], &scale);
            IkcStepD st;
            st.F = m_mul(m_mul(S, m.pose(j)), A);
            st.scale = scale;
            st.kind = m.jtype[j] == KIN_JOINT_PRISMATIC ? MOT_PRISM : MOT_REV;
            if (st.kind == MOT_REV && scale != 1.0) st.flags |= SF_SCALE;
            st.var = qcol[j];
            st.parent_step = carrier;
            st.anc = anc | (1u << qcol[j]);
            joints |= 1u << qcol[j];
            if (st.kind == MOT_PRISM) prism |= 1u << qcol[j];
            const int32_t s = (int32_t)steps.size();
            steps.push_back(st);
            const int rc = visit(ch, s, m_rot_transpose(A), st.anc);
            if (rc != KIN_OK) return rc;
        }
        return KIN_OK;
    };
    for (int32_t l = 0; l < L; ++l)
        if (needed[l] && m.link_pjoint[l] < 0) {
            const int rc = visit(l, -1, m_identity(), base_bits);
            if (rc != KIN_OK) return rc;
        }
    // spheres in carrier order (root first, then the walk's step order), the caller's order inside a carrier
    std::stable_sort(spheres.begin(), spheres.end(), [](const IkcSphD& a, const IkcSphD& b) { return a.step < b.step; });
    int32_t sph_root0 = 0, sph_root1 = 0;
    for (size_t k = 0; k < spheres.size(); ++k) {
        const int32_t s = spheres[k].step;
        if (s < 0) {
            sph_root1 = (int32_t)k + 1;
        } else {
            if (steps[s].sph1 == 0) steps[s].sph0 = (int32_t)k;
            steps[s].sph1 = (int32_t)k + 1;
        }
    }
    // branch frames: a step whose frame a later, non-adjacent step starts from is saved into a slot, live
    // from the step to its last such child
    const int32_t ns = (int32_t)steps.size();
    std::vector<int32_t> last_use(ns, -1);
    for (int32_t s = 0; s < ns; ++s) {
        const int32_t p = steps[s].parent_step;
        if (p >= 0 && p != s - 1) last_use[p] = std::max(last_use[p], s);
    }
    std::vector<int32_t> slot_of(ns, -1), slot_free_at(kIkcMaxSlots, -1);
    for (int32_t s = 0; s < ns; ++s) {
        if (last_use[s] < 0) continue;
        int sl = -1;
        for (int k = 0; k < kIkcMaxSlots && sl < 0; ++k)
            if (slot_free_at[k] <= s) sl = k;
        if (sl < 0)
            return set_error(KIN_E_UNSUPPORTED, "kin_coll_ik_plan_create: the tree needs more than " +
                                                    std::to_string(kIkcMaxSlots) + " saved branch frames");
        slot_of[s] = sl;
        slot_free_at[sl] = last_use[s];
        steps[s].save = sl;
    }
    uint32_t tgt_mask = tgt_step == kIkcRoot ? base_bits : steps[tgt_step].anc;
    uint32_t free_mask = tgt_mask;
    for (const IkcSphD& sd : spheres) free_mask |= sd.step < 0 ? base_bits : steps[sd.step].anc;
    by_dtype(c->dtype, [&](auto t) {
        using T = decltype(t);
        P.h_ikc_steps.assign(std::max<size_t>(1, ns) * sizeof(KIkcStep<T>), 0);
        P.h_ikc_sph.assign(std::max<size_t>(1, spheres.size()) * sizeof(KSphere<T>), 0);
        KIkcProg<T>& K = P.ikc<T>();
        KIkcStep<T>* st_out = reinterpret_cast<KIkcStep<T>*>(P.h_ikc_steps.data());
        KSphere<T>* sp_out = reinterpret_cast<KSphere<T>*>(P.h_ikc_sph.data());
        K = {};
        K.nS = ns;
        K.nv = nv;
        K.n_q = nq;
        K.base_col = base_col;
        K.n_sph = (int32_t)spheres.size();
        K.sph_root0 = sph_root0;
        K.sph_root1 = sph_root1;
        K.tgt_step = tgt_step;
        K.has_xt = !m_is_identity(Xt);
        K.tgt_mask = tgt_mask;
        K.free_mask = free_mask;
        K.joint_mask = joints;
        K.prism_mask = prism;
        to_row12<T>(Xt, K.Xt);
        for (int v = 0; v < kIkcMaxVars; ++v) {
            K.vlo[v] = (T)-INFINITY;
            K.vhi[v] = (T)INFINITY;
        }
        for (int32_t j = 0; j < J; ++j)
            if (qcol[j] >= 0 && ((joints >> qcol[j]) & 1u)) {
                K.vlo[qcol[j]] = (T)m.jlo[j];
                K.vhi[qcol[j]] = (T)m.jhi[j];
            }
        // the normal equations' structure: entry (v, c) gets terms from the pose rows when both move the
        // target, from a sphere's row when both move that sphere
        auto add_block = [&](uint32_t mask) {
            for (int v = 0; v < nv; ++v)
                if ((mask >> v) & 1u) K.nzrow[v] |= mask & ((2u << v) - 1u);
        };
        add_block(tgt_mask);
        for (const IkcSphD& sd : spheres) add_block(sd.step < 0 ? base_bits : steps[sd.step].anc);
        for (int32_t s = 0; s < ns; ++s) {
            const IkcStepD& a = steps[s];
            auto& b = st_out[s];
            memset(&b, 0, sizeof(b));
            to_row12<T>(a.F, b.F);
            b.scale = (T)a.scale;
            b.kind = a.kind;
            b.flags = a.flags;
            b.var = a.var;
            b.parent = a.parent_step < 0 ? kIkcRoot : a.parent_step == s - 1 ? kIkcPrev : slot_of[a.parent_step];
            b.save = a.save;
            b.sph0 = a.sph0;
            b.sph1 = a.sph1;
            b.anc = a.anc;
        }
        for (size_t k = 0; k < spheres.size(); ++k) {
            auto& b = sp_out[k];
            memset(&b, 0, sizeof(b));
            for (int i = 0; i < 3; ++i) b.c[i] = (T)spheres[k].c[i];
            b.r = (T)spheres[k].r;
            b.out = spheres[k].out;
            b.anc = spheres[k].step < 0 ? base_bits : steps[spheres[k].step].anc;
        }
    });
    return KIN_OK;
}
