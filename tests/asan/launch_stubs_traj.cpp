// Test-only: the stand-in of the batched trajectory optimiser's launcher (k_traj, k_traj_pose, k_traj_tree) for the
// host sanitizer harness (see launch_stubs.cpp).
#include "kinhip_internal.h"

namespace kinhip {
template <typename T>
hipError_t launch_traj(const TrajLaunch<T>&, const KBox<T>*, const CollArgs&, const TrajArgs&, const TrajDof&, const T*,
                       T*, int64_t, int64_t, int32_t*, T*, int64_t, hipStream_t) {
    return hipErrorNoDevice;
}
#define KIN_STUBS_TRAJ(T)                                                                                     \
    template hipError_t launch_traj<T>(const TrajLaunch<T>&, const KBox<T>*, const CollArgs&, const TrajArgs&, \
                                       const TrajDof&, const T*, T*, int64_t, int64_t, int32_t*, T*, int64_t, \
                                       hipStream_t);
KIN_STUBS_TRAJ(float)
KIN_STUBS_TRAJ(double)
#undef KIN_STUBS_TRAJ
}  // namespace kinhip
