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
    traj_tree_body<T, MAXA, L>(parts, n_parts, ndof, boxes, a, ta, dof, minvT, xi, ldx, n_traj, iters, info, ldi, smem);
}

}  // namespace

int traj_segment(int n_wp) { return n_wp <= 8 ? 8 : n_wp <= 16 ? 16 : n_wp <= 32 ? 32 : 64; }

template <typename T>
size_t traj_lds_bytes(int n_boxes, int n_wp, int ndof, int block) {
    const size_t box = n_boxes <= kCollLdsBoxes ? (size_t)n_boxes * sizeof(KBox<T>) : 0;
    return box + sizeof(T) * ((size_t)(n_wp - 2) * (n_wp - 2) + (size_t)block * ndof);
}

template <typename T>
hipError_t launch_traj(const KProg<T>& P, const KStep<T>* steps, const KSphere<T>* sph, const KBox<T>* boxes,
                       const LaunchGeom& g, const CollArgs& a, const TrajArgs& ta, const TrajDof& dof, const T* minvT,
                       T* xi, int64_t ldx, int64_t n_traj, int32_t* iters, T* info, int64_t ldi, hipStream_t st) {
    const int L = traj_segment(ta.n_wp);
    const int ndof = P.n_jac + ((P.flags & PF_BASE) ? 3 : 0);
    // the largest workgroup (whole waves) whose LDS stays within 64 KiB
    int block = 256;
    while (block > 64 && traj_lds_bytes<T>(a.n_boxes, ta.n_wp, ndof, block) > 65536) block /= 2;
    const size_t lds = traj_lds_bytes<T>(a.n_boxes, ta.n_wp, ndof, block);
    if (lds > 65536) return hipErrorInvalidValue;
    // chunks of trajectories: every lane byte offset (column * sizeof(T)) below 2^31
    const int64_t chunk = kChunk / 64;
    for (int64_t t0 = 0; t0 < n_traj; t0 += chunk) {
        const int64_t c = std::min(chunk, n_traj - t0);
        const dim3 grid(grid_of(c * L, block)), blk(block);
        T* xc = xi + t0 * ta.n_wp;
        int32_t* ic = iters ? iters + t0 : iters;
        T* fc = info ? info + t0 : info;
#define KIN_TR_LAUNCH_L(MA, LL) \
        hipLaunchKernelGGL((k_traj<T, MA, LL>), grid, blk, lds, st, P, steps, sph, boxes, a, ta, dof, minvT, xc, ldx, c, ic, fc, ldi)
#define KIN_TR_LAUNCH(MA)                      \
        switch (L) {                           \
        case 8: KIN_TR_LAUNCH_L(MA, 8); break;   \
        case 16: KIN_TR_LAUNCH_L(MA, 16); break; \
        case 32: KIN_TR_LAUNCH_L(MA, 32); break; \
        default: KIN_TR_LAUNCH_L(MA, 64); break; \
        }
        switch (g.maxA) {
        case 4: KIN_TR_LAUNCH(4); break;
        case 8: KIN_TR_LAUNCH(8); break;
        case 12: KIN_TR_LAUNCH(12); break;
        case 16: KIN_TR_LAUNCH(16); break;
        default: return hipErrorInvalidValue;  // (kin_traj_opt_batch refuses longer chains)
        }
#undef KIN_TR_LAUNCH
#undef KIN_TR_LAUNCH_L
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <typename T>
hipError_t launch_traj_pose(const KProg<T>& P, const KStep<T>* steps, const KSphere<T>* sph, const KBox<T>* boxes,
                            const LaunchGeom& g, const CollArgs& a, const TrajArgs& ta, const TrajDof& dof,
                            const TrajPose<T>& tp, const T* minvT, const T* targets, int64_t ldt, T* xi, int64_t ldx,
                            int64_t n_traj, int32_t* iters, T* info, int64_t ldi, hipStream_t st) {
    const int L = traj_segment(ta.n_wp);
    const int ndof = P.n_jac + ((P.flags & PF_BASE) ? 3 : 0);
    int block = 256;  // as launch_traj: the same LDS layout
    while (block > 64 && traj_lds_bytes<T>(a.n_boxes, ta.n_wp, ndof, block) > 65536) block /= 2;
    const size_t lds = traj_lds_bytes<T>(a.n_boxes, ta.n_wp, ndof, block);
    if (lds > 65536) return hipErrorInvalidValue;
    const int64_t chunk = kChunk / 64;
    for (int64_t t0 = 0; t0 < n_traj; t0 += chunk) {
        const int64_t c = std::min(chunk, n_traj - t0);
        const dim3 grid(grid_of(c * L, block)), blk(block);
        T* xc = xi + t0 * ta.n_wp;
        const T* tc = targets + t0;
        int32_t* ic = iters ? iters + t0 : iters;
        T* fc = info ? info + t0 : info;
#define KIN_TRP_LAUNCH_L(MA, LL)                                                                                    \
        hipLaunchKernelGGL((k_traj_pose<T, MA, LL>), grid, blk, lds, st, P, steps, sph, boxes, a, ta, dof, tp, minvT, tc, \
                           ldt, xc, ldx, c, ic, fc, ldi)
#define KIN_TRP_LAUNCH(MA)                        \
        switch (L) {                              \
        case 8: KIN_TRP_LAUNCH_L(MA, 8); break;   \
        case 16: KIN_TRP_LAUNCH_L(MA, 16); break; \
        case 32: KIN_TRP_LAUNCH_L(MA, 32); break; \
        default: KIN_TRP_LAUNCH_L(MA, 64); break; \
        }
        switch (g.maxA) {
        case 4: KIN_TRP_LAUNCH(4); break;
        case 8: KIN_TRP_LAUNCH(8); break;
        default: return hipErrorInvalidValue;  // (kin_traj_opt_pose_batch refuses longer chains)
        }
#undef KIN_TRP_LAUNCH
#undef KIN_TRP_LAUNCH_L
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <typename T>
hipError_t launch_traj_tree(const TrajPart<T>* parts, int n_parts, int maxA, int ndof, const KBox<T>* boxes,
                            const CollArgs& a, const TrajArgs& ta, const TrajDof& dof, const T* minvT, T* xi, int64_t ldx,
                            int64_t n_traj, int32_t* iters, T* info, int64_t ldi, hipStream_t st) {
    if (n_parts < 1 || n_parts > kTrajMaxParts || ndof > kTrajNdLarge) return hipErrorInvalidValue;
    const int L = traj_segment(ta.n_wp);
    int block = 256;  // as launch_traj: the same LDS layout
    while (block > 64 && traj_lds_bytes<T>(a.n_boxes, ta.n_wp, ndof, block) > 65536) block /= 2;
    const size_t lds = traj_lds_bytes<T>(a.n_boxes, ta.n_wp, ndof, block);
    if (lds > 65536) return hipErrorInvalidValue;
    const int64_t chunk = kChunk / 64;
    for (int64_t t0 = 0; t0 < n_traj; t0 += chunk) {
        const int64_t c = std::min(chunk, n_traj - t0);
        const dim3 grid(grid_of(c * L, block)), blk(block);
        T* xc = xi + t0 * ta.n_wp;
        int32_t* ic = iters ? iters + t0 : iters;
        T* fc = info ? info + t0 : info;
#define KIN_TRT_LAUNCH_L(MA, LL)                                                                                     \
        hipLaunchKernelGGL((k_traj_tree<T, MA, LL>), grid, blk, lds, st, parts, n_parts, ndof, boxes, a, ta, dof, minvT, \
                           xc, ldx, c, ic, fc, ldi)
#define KIN_TRT_LAUNCH(MA)                        \
        switch (L) {                              \
        case 8: KIN_TRT_LAUNCH_L(MA, 8); break;   \
        case 16: KIN_TRT_LAUNCH_L(MA, 16); break; \
        case 32: KIN_TRT_LAUNCH_L(MA, 32); break; \
        default: KIN_TRT_LAUNCH_L(MA, 64); break; \
        }
        switch (maxA) {
        case 8: KIN_TRT_LAUNCH(8); break;
        case 16: KIN_TRT_LAUNCH(16); break;
        default: return hipErrorInvalidValue;  // (kin_traj_opt_tree_batch refuses longer chains)
        }
#undef KIN_TRT_LAUNCH
#undef KIN_TRT_LAUNCH_L
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

#define KIN_INSTANTIATE(T)                                                                                       \
    template hipError_t launch_traj<T>(const KProg<T>&, const KStep<T>*, const KSphere<T>*, const KBox<T>*,      \
                                       const LaunchGeom&, const CollArgs&, const TrajArgs&, const TrajDof&,     \
                                       const T*, T*, int64_t, int64_t, int32_t*, T*, int64_t, hipStream_t);    \
    template hipError_t launch_traj_pose<T>(const KProg<T>&, const KStep<T>*, const KSphere<T>*, const KBox<T>*, \
                                            const LaunchGeom&, const CollArgs&, const TrajArgs&, const TrajDof&, \
                                            const TrajPose<T>&, const T*, const T*, int64_t, T*, int64_t,       \
                                            int64_t, int32_t*, T*, int64_t, hipStream_t);               \
    template hipError_t launch_traj_tree<T>(const TrajPart<T>*, int, int, int, const KBox<T>*, const CollArgs&,  \
                                            const TrajArgs&, const TrajDof&, const T*, T*, int64_t, int64_t,     \
                                            int32_t*, T*, int64_t, hipStream_t);
KIN_INSTANTIATE(float)
KIN_INSTANTIATE(double)

}  // namespace kinhip
