// kinhip_traj_pose_tree.hip -- k_traj_pose_tree (kin_traj_opt_pose_tree_batch): k_traj_pose's constrained update on
// the part loop of k_traj_tree (SCENE = 0) or k_traj_scene (SCENE = kTrajSceneGroups), common bound 8 only.  A unit of
// its own so that the 16 instantiations compile beside the other units'; reached only through launch_traj
// (kinhip_traj.hip).
// (gfx950 only; device body in kinhip_traj_dev.h)
#include "kinhip_traj_dev.h"

namespace kinhip {
namespace {

// sa: SCENE != 0 only (a static union passes an empty one)
template <typename T, int L, int SCENE>
__global__ __launch_bounds__(256) void k_traj_pose_tree(const TrajPart<T>* __restrict__ parts, int n_parts, int ndof,
                                                        const KBox<T>* __restrict__ boxes, const CollArgs a,
                                                        const TrajArgs ta, const TrajDof dof, const TrajPose<T> tp,
                                                        const T* __restrict__ minvT, const T* __restrict__ targets,
                                                        int64_t ldt, const SceneArgs<T> sa, T* __restrict__ xi,
                                                        int64_t ldx, int64_t n_traj, int32_t* __restrict__ iters,
                                                        T* __restrict__ info, int64_t ldi) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    traj_body<T, 8, L, true, true, SCENE>(KProg<T>{}, nullptr, nullptr, boxes, a, ta, dof, minvT, xi, ldx, n_traj, iters,
                                          info, ldi, smem, &tp, targets, ldt, parts, n_parts, ndof, &sa);
}

template <typename T, int SCENE>
void pose_tree_at(int L, const TrajSceneChunk<T>& k, const TrajPose<T>& tp, const T* targets, int64_t ldt,
                  const SceneArgs<T>& sa) {
    const auto go = [&](auto l) {
        hipLaunchKernelGGL((k_traj_pose_tree<T, decltype(l)::value, SCENE>), k.grid, k.block, k.lds, k.st, k.parts,
                           k.n_parts, k.ndof, k.boxes, *k.a, *k.ta, *k.dof, tp, k.minvT, targets, ldt, sa, k.xi, k.ldx,
                           k.n_traj, k.iters, k.info, k.ldi);
    };
    switch (L) {
    case 8: go(std::integral_constant<int, 8>{}); break;
    case 16: go(std::integral_constant<int, 16>{}); break;
    case 32: go(std::integral_constant<int, 32>{}); break;
    default: go(std::integral_constant<int, 64>{}); break;
    }
}

}  // namespace

// one chunk of launch_traj's loop; k.scene null: a static union; false: a chain bound the kernel is not compiled for
template <typename T>
bool launch_traj_pose_tree_chunk(int maxA, int L, const TrajSceneChunk<T>& k, TrajPose<T> tp, const T* targets,
                                 int64_t ldt) {
    if (maxA != kTrajPoseMaxChain || tp.part < 0 || tp.part >= k.n_parts) return false;
    if (!k.scene) {
        pose_tree_at<T, 0>(L, k, tp, targets, ldt, SceneArgs<T>{});
        return true;
    }
    if (k.scene->ng < 1 || k.scene->ng > kTrajSceneGroups) return false;
    pose_tree_at<T, kTrajSceneGroups>(L, k, tp, targets, ldt, traj_scene_args<T>(*k.scene, k.sample0));
    return true;
}

template bool launch_traj_pose_tree_chunk<float>(int, int, const TrajSceneChunk<float>&, TrajPose<float>, const float*,
                                                 int64_t);
template bool launch_traj_pose_tree_chunk<double>(int, int, const TrajSceneChunk<double>&, TrajPose<double>,
                                                  const double*, int64_t);

}  // namespace kinhip
