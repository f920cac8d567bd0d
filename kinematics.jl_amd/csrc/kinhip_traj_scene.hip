// kinhip_traj_scene.hip -- k_traj_scene (kin_traj_opt_scene_batch): k_traj_tree with the union's boxes attached to
// a scene mechanism, one scene state per waypoint (per lane).  A unit of its own so that the 16 instantiations
// compile beside kinhip_traj.hip's; reached only through launch_traj (kinhip_traj.hip).
// (gfx950 only; device body in kinhip_traj_dev.h)
#include "kinhip_traj_dev.h"

namespace kinhip {
namespace {

// unions of at most kTrajSceneGroups moving groups (the lane's group frames: 12 registers per group)
template <typename T, int MAXA, int L>
__global__ __launch_bounds__(256) void k_traj_scene(const TrajPart<T>* __restrict__ parts, int n_parts, int ndof,
                                                    const KBox<T>* __restrict__ boxes, const CollArgs a,
                                                    const TrajArgs ta, const TrajDof dof, const T* __restrict__ minvT,
                                                    const SceneArgs<T> sa, T* __restrict__ xi, int64_t ldx,
                                                    int64_t n_traj, int32_t* __restrict__ iters, T* __restrict__ info,
                                                    int64_t ldi) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    traj_body<T, MAXA, L, false, true, kTrajSceneGroups>(KProg<T>{}, nullptr, nullptr, boxes, a, ta, dof, minvT, xi, ldx,
                                                         n_traj, iters, info, ldi, smem, nullptr, nullptr, 0, parts,
                                                         n_parts, ndof, &sa);
}

template <typename T, int MAXA>
bool scene_at(int L, const TrajSceneChunk<T>& k, const SceneArgs<T>& sa) {
    const auto go = [&](auto l) {
        hipLaunchKernelGGL((k_traj_scene<T, MAXA, decltype(l)::value>), k.grid, k.block, k.lds, k.st, k.parts, k.n_parts,
                           k.ndof, k.boxes, *k.a, *k.ta, *k.dof, k.minvT, sa, k.xi, k.ldx, k.n_traj, k.iters, k.info,
                           k.ldi);
    };
    switch (L) {
    case 8: go(std::integral_constant<int, 8>{}); break;
    case 16: go(std::integral_constant<int, 16>{}); break;
    case 32: go(std::integral_constant<int, 32>{}); break;
    default: go(std::integral_constant<int, 64>{}); break;
    }
    return true;
}

}  // namespace

// one chunk of launch_traj's loop; false: a chain bound the kernel is not compiled for
template <typename T>
bool launch_traj_scene_chunk(int maxA, int L, const TrajSceneChunk<T>& k) {
    if (k.scene->ng < 1 || k.scene->ng > kTrajSceneGroups) return false;
    const SceneArgs<T> sa = traj_scene_args<T>(*k.scene, k.sample0);
    return maxA == 8 ? scene_at<T, 8>(L, k, sa) : maxA == 16 ? scene_at<T, 16>(L, k, sa) : false;
}

template bool launch_traj_scene_chunk<float>(int, int, const TrajSceneChunk<float>&);
template bool launch_traj_scene_chunk<double>(int, int, const TrajSceneChunk<double>&);

}  // namespace kinhip
