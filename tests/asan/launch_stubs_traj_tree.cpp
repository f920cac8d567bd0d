// Test-only: the stand-in of k_traj_tree's launcher (kin_traj_opt_tree_batch) for the host sanitizer harness
// (see launch_stubs.cpp).
#include "kinhip_internal.h"

namespace kinhip {
template <typename T>
hipError_t launch_traj_tree(const TrajPart<T>*, int, int, int, const KBox<T>*, const CollArgs&, const TrajArgs&,
                            const TrajDof&, const T*, T*, int64_t, int64_t, int32_t*, T*, int64_t, hipStream_t) {
    return hipErrorNoDevice;
}
#define KIN_STUBS_TRAJ_TREE(T)                                                                                  \
    template hipError_t launch_traj_tree<T>(const TrajPart<T>*, int, int, int, const KBox<T>*, const CollArgs&, \
                                            const TrajArgs&, const TrajDof&, const T*, T*, int64_t, int64_t,    \
                                            int32_t*, T*, int64_t, hipStream_t);
KIN_STUBS_TRAJ_TREE(float)
KIN_STUBS_TRAJ_TREE(double)
#undef KIN_STUBS_TRAJ_TREE
}  // namespace kinhip
