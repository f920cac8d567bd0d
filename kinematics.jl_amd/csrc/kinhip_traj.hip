// kinhip_traj.hip -- k_traj: batched trajectory optimisation, the whole descent of many trajectories in
// one launch (kin_traj_opt_batch; the reference plans one trajectory at a time, src/planning.jl:332-401); k_traj_pose
// (kin_traj_opt_pose_batch) and k_traj_tree (kin_traj_opt_tree_batch: spheres on several chains).
// (gfx950 only; device body in kinhip_traj_dev.h)
#include "kinhip_traj_dev.h"

namespace kinhip {
namespace {

template <typename T, int MAXA, int L>
__global__ __launch_bounds__(256) void k_traj(const KProg<T> P, const KStep<T>* __restrict__ S,
                                              const KSphere<T>* __restrict__ sph, const KBox<T>* __restrict__ boxes,
                                              const CollArgs a, const TrajArgs ta, const TrajDof dof,
                                              const T* __restrict__ minvT, T* __restrict__ xi, int64_t ldx,
                                              int64_t n_traj, int32_t* __restrict__ iters, T* __restrict__ info,
                                              int64_t ldi) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    traj_body<T, MAXA, L>(P, S, sph, boxes, a, ta, dof, minvT, xi, ldx, n_traj, iters, info, ldi, smem);
}

// the POSE variant (kin_traj_opt_pose_batch): tp and the targets [12][ldt] besides k_traj's arguments; info has 6 rows
template <typename T, int MAXA, int L>
__global__ __launch_bounds__(256) void k_traj_pose(const KProg<T> P, const KStep<T>* __restrict__ S,
                                                   const KSphere<T>* __restrict__ sph, const KBox<T>* __restrict__ boxes,
                                                   const CollArgs a, const TrajArgs ta, const TrajDof dof,
                                                   const TrajPose<T> tp, const T* __restrict__ minvT,
                                                   const T* __restrict__ targets, int64_t ldt, T* __restrict__ xi,
                                                   int64_t ldx, int64_t n_traj, int32_t* __restrict__ iters,
                                                   T* __restrict__ info, int64_t ldi) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    traj_body<T, MAXA, L, true>(P, S, sph, boxes, a, ta, dof, minvT, xi, ldx, n_traj, iters, info, ldi, smem, &tp, targets,
                                ldt);
}

// the multi-chain variant (kin_traj_opt_tree_batch): the plan's part table instead of one program
template <typename T, int MAXA, int L>
__global__ __launch_bounds__(256) void k_traj_tree(const TrajPart<T>* __restrict__ parts, int n_parts, int ndof,
                                                   const KBox<T>* __restrict__ boxes, const CollArgs a,
                                                   const TrajArgs ta, const TrajDof dof, const T* __restrict__ minvT,
                                                   T* __restrict__ xi, int64_t ldx, int64_t n_traj,
                                                   int32_t* __restrict__ iters, T* __restrict__ info, int64_t ldi) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    traj_body<T, MAXA, L, false, true>(KProg<T>{}, nullptr, nullptr, boxes, a, ta, dof, minvT, xi, ldx, n_traj, iters, info,
                                       ldi, smem, nullptr, nullptr, 0, parts, n_parts, ndof);
}

}  // namespace

int traj_segment(int n_wp) { return n_wp <= 8 ? 8 : n_wp <= 16 ? 16 : n_wp <= 32 ? 32 : 64; }

template <typename T>
size_t traj_lds_bytes(int n_boxes, int n_wp, int ndof, int block) {
    const size_t box = n_boxes <= kCollLdsBoxes ? (size_t)n_boxes * sizeof(KBox<T>) : 0;
    return box + sizeof(T) * ((size_t)(n_wp - 2) * (n_wp - 2) + (size_t)block * ndof);
}

namespace {

// f(m, l), two std::integral_constant, for the chain bound of the list that equals maxA and the segment size L
// (one of traj_segment's); false if the list has no such bound
template <int... MA, typename F>
bool traj_dispatch(int maxA, int L, F&& f) {
    const auto at = [&](auto m) {
        switch (L) {
        case 8: f(m, std::integral_constant<int, 8>{}); break;
        case 16: f(m, std::integral_constant<int, 16>{}); break;
        case 32: f(m, std::integral_constant<int, 32>{}); break;
        default: f(m, std::integral_constant<int, 64>{}); break;
        }
        return true;
    };
    return (... || (maxA == MA && at(std::integral_constant<int, MA>{})));
}

}  // namespace

// d.tp selects k_traj_pose, d.parts k_traj_tree (with d.scene: k_traj_scene), both k_traj_pose_tree, neither k_traj;
// each with the chain bounds it is compiled for
template <typename T>
hipError_t launch_traj(const TrajLaunch<T>& d, const KBox<T>* boxes, const CollArgs& a, const TrajArgs& ta,
                       const TrajDof& dof, const T* minvT, T* xi, int64_t ldx, int64_t n_traj, int32_t* iters, T* info,
                       int64_t ldi, hipStream_t st) {
    if (d.scene && !d.parts) return hipErrorInvalidValue;
    if (d.parts && (d.n_parts < 1 || d.n_parts > kTrajMaxParts || d.ndof > kTrajNdLarge)) return hipErrorInvalidValue;
    const int L = traj_segment(ta.n_wp);
    // the largest workgroup (whole waves) whose LDS stays within 64 KiB
    int block = 256;
    while (block > 64 && traj_lds_bytes<T>(a.n_boxes, ta.n_wp, d.ndof, block) > 65536) block /= 2;
    const size_t lds = traj_lds_bytes<T>(a.n_boxes, ta.n_wp, d.ndof, block);
    if (lds > 65536) return hipErrorInvalidValue;
    // chunks of trajectories: every lane byte offset (column * sizeof(T)) below 2^31
    const int64_t chunk = kChunk / 64;
    for (int64_t t0 = 0; t0 < n_traj; t0 += chunk) {
        const int64_t c = std::min(chunk, n_traj - t0);
        const dim3 grid(grid_of(c * L, block)), blk(block);
        T* xc = xi + t0 * ta.n_wp;
        const T* tc = d.targets ? d.targets + t0 : d.targets;
        int32_t* ic = iters ? iters + t0 : iters;
        T* fc = info ? info + t0 : info;
        bool compiled;  // (the entry points refuse the chain bounds a variant is not compiled for)
        if (!d.tp && !d.parts)
            compiled = traj_dispatch<4, 8, 12, 16>(d.maxA, L, [&](auto m, auto l) {
                hipLaunchKernelGGL((k_traj<T, decltype(m)::value, decltype(l)::value>), grid, blk, lds, st, *d.P, d.steps,
                                   d.sph, boxes, a, ta, dof, minvT, xc, ldx, c, ic, fc, ldi);
            });
        else if (d.parts && (d.scene || d.tp)) {
            const TrajSceneChunk<T> k{grid, blk, lds, st, d.parts, d.n_parts, d.ndof, boxes, &a, &ta, &dof, minvT, d.scene,
                                      t0 * ta.n_wp, xc, ldx, c, ic, fc, ldi};
            compiled = d.tp ? launch_traj_pose_tree_chunk<T>(d.maxA, L, k, *d.tp, tc, d.ldt)
                            : launch_traj_scene_chunk<T>(d.maxA, L, k);
        } else if (d.tp)
            compiled = traj_dispatch<4, 8>(d.maxA, L, [&](auto m, auto l) {
                hipLaunchKernelGGL((k_traj_pose<T, decltype(m)::value, decltype(l)::value>), grid, blk, lds, st, *d.P,
                                   d.steps, d.sph, boxes, a, ta, dof, *d.tp, minvT, tc, d.ldt, xc, ldx, c, ic, fc, ldi);
            });
        else
            compiled = traj_dispatch<8, 16>(d.maxA, L, [&](auto m, auto l) {
                hipLaunchKernelGGL((k_traj_tree<T, decltype(m)::value, decltype(l)::value>), grid, blk, lds, st, d.parts,
                                   d.n_parts, d.ndof, boxes, a, ta, dof, minvT, xc, ldx, c, ic, fc, ldi);
            });
        if (!compiled) return hipErrorInvalidValue;
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template hipError_t launch_traj<float>(const TrajLaunch<float>&, const KBox<float>*, const CollArgs&, const TrajArgs&,
                                       const TrajDof&, const float*, float*, int64_t, int64_t, int32_t*, float*, int64_t,
                                       hipStream_t);
template hipError_t launch_traj<double>(const TrajLaunch<double>&, const KBox<double>*, const CollArgs&, const TrajArgs&,
                                        const TrajDof&, const double*, double*, int64_t, int64_t, int32_t*, double*,
                                        int64_t, hipStream_t);

}  // namespace kinhip
