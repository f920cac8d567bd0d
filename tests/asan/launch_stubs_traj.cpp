// Test-only: the k_traj launcher's stand-in for the host sanitizer harness (see launch_stubs.cpp).
#include "kinhip_internal.h"

namespace kinhip {
template <typename T>
hipError_t launch_traj(const KProg<T>&, const KStep<T>*, const KSphere<T>*, const KBox<T>*, const LaunchGeom&,
                       const CollArgs&, const TrajArgs&, const TrajDof&, const T*, T*, int64_t, int64_t, int32_t*, T*,
                       int64_t, hipStream_t) {
    return hipErrorNoDevice;
}
#define KIN_STUBS_TRAJ(T)                                                                                      \
    template hipError_t launch_traj<T>(const KProg<T>&, const KStep<T>*, const KSphere<T>*, const KBox<T>*,    \
                                       const LaunchGeom&, const CollArgs&, const TrajArgs&, const TrajDof&,   \
                                       const T*, T*, int64_t, int64_t, int32_t*, T*, int64_t, hipStream_t);
KIN_STUBS_TRAJ(float)
KIN_STUBS_TRAJ(double)
}  // namespace kinhip
