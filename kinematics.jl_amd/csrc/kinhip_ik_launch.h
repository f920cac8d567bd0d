// kinhip_ik_launch.h -- what the IK launchers (kinhip_ik.hip, kinhip_ikt.hip) share on the host side.  Not among
// the device headers: the run-time compiled sources do not carry it.
#pragma once
#include "kinhip_ik_dev.h"

namespace kinhip {

// The kernels' arguments of a call, before its schedule: one phase (att0 = 0, no list), chunk fields unset.
// (k_ik_tree calls carry no damping by error and no trace: kin_ik_coll_batch refuses the one and never sets the other.)
template <typename T>
IkArgsT<T> ik_args(const IkArgs& a) {
    int L, natt;
    ik_attempts(a, &L, &natt);
    IkArgsT<T> at{};
    at.max_iters = a.max_iters;
    at.lam2 = T(a.lambda * a.lambda);
    at.tol_pos = T(a.tol_pos);
    at.tol_rot = T(a.tol_rot);
    at.max_step = T(a.max_step);
    at.attempt_len = L;
    at.n_attempts = natt;
    at.seed = a.seed;
    at.rpy_obj = a.with_rot == 2;
    at.damp_err = T(a.damp_err);
    at.trace = (T*)a.trace;
    at.trace_ld = a.trace_ld;
    return at;
}

}  // namespace kinhip
