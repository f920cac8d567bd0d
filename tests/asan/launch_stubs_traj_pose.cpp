// Test-only: the stand-in of k_traj's POSE launcher (kin_traj_opt_pose_batch) for the host sanitizer harness
// (see launch_stubs.cpp).
#include "kinhip_internal.h"

namespace kinhip {
template <typename T>
hipError_t launch_traj_pose(const KProg<T>&, const KStep<T>*, const KSphere<T>*, const KBox<T>*, const LaunchGeom&,
                            const CollArgs&, const TrajArgs&, const TrajDof&, const TrajPose<T>&, const T*, const T*,
                            int64_t, T*, int64_t, int64_t, int32_t*, T*, int64_t, hipStream_t) {
    return hipErrorNoDevice;
}
#define KIN_STUBS_TRAJ_POSE(T)                                                                                   \
    template hipError_t launch_traj_pose<T>(const KProg<T>&, const KStep<T>*, const KSphere<T>*, const KBox<T>*, \
                                            const LaunchGeom&, const CollArgs&, const TrajArgs&, const TrajDof&, \
                                            const TrajPose<T>&, const T*, const T*, int64_t, T*, int64_t,       \
                                            int64_t, int32_t*, T*, int64_t, hipStream_t);
KIN_STUBS_TRAJ_POSE(float)
KIN_STUBS_TRAJ_POSE(double)
#undef KIN_STUBS_TRAJ_POSE
}  // namespace kinhip
