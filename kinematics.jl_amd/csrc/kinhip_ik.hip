// kinhip_ik.hip -- k_ik_dls (batched DLS IK with restarts) and k_nakamura.
// (gfx950 only; shared helpers in kinhip_device.h)
#include "kinhip_ik_dev.h"
#include "kinhip_ik_launch.h"

namespace kinhip {
namespace {

// --------------------------------------------------------------------------
// generic kernels (the staged program is read from device memory)
// --------------------------------------------------------------------------
#ifndef KINHIP_IK_WAVES
#define KINHIP_IK_WAVES 1
#endif
template <typename T, int MAXA, int ROWS, int G>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(KINHIP_IK_WAVES))) void k_ik_dls(
    const KProg<T> P, const KStep<T>* __restrict__ S, const IkArgsT<T> a, const T* __restrict__ tgt, int64_t ldt,
    T* __restrict__ q, int64_t ldq, int64_t n, int32_t* __restrict__ iters, T* __restrict__ err, int64_t lde,
    int64_t chunk) {
    ik_body<T, MAXA, ROWS, G>(P, S, a, tgt, ldt, q, ldq, n, iters, err, lde, chunk);
}

template <typename T, int MAXA>
__global__ __launch_bounds__(256) void k_nakamura(const KProg<T> P, const KStep<T>* __restrict__ S,
                                                  const T* __restrict__ pts, int64_t ldpt, T* __restrict__ q,
                                                  int64_t ldq, int64_t n) {
    nakamura_body<T, MAXA>(P, S, pts, ldpt, q, ldq, n);
}

}  // namespace

// The schedule of a call is decided in kinhip_ik_sched.h; here are its knobs (A/B build only) and the device.
static const IkKnobs& ik_knobs() {
    static const IkKnobs knobs = [] {
        IkKnobs k;
        k.group = ab_env_int("KINHIP_IK_GROUP", k.group);
        k.resident = ab_env_int("KINHIP_IK_RESIDENT", k.resident);
        k.two_phase = ab_env_int("KINHIP_IK_TWO_PHASE", k.two_phase);
        k.p1_cut = ab_env_int("KINHIP_IK_P1_CUT", k.p1_cut);
        k.queue = ab_env_int("KINHIP_IK_QUEUE", k.queue);
        k.tp_queue = ab_env_int("KINHIP_IK_TP_QUEUE", k.tp_queue);
        k.p2_block = ab_env_int("KINHIP_IK_P2_BLOCK", k.p2_block);
        k.p2_spread = ab_env_int("KINHIP_IK_P2_SPREAD", k.p2_spread);
        return k;
    }();
    return knobs;
}

static int ik_cus() {
    static const int cus = [] {
        int dev = 0, c = 0;
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev);
        return c > 0 ? c : 256;
    }();
    return cus;
}

// the policy's inputs that a call fixes (n, c and the per-plan ones are the launcher's)
static IkSchedIn ik_sched_in(const IkArgs& a, int64_t n, int64_t cap) {
    IkSchedIn in;
    in.n = n;
    ik_attempts(a, &in.L, &in.natt);
    in.lanes = a.lanes;
    in.cap = cap;
    in.cus = ik_cus();
    in.damped = a.damp_err != 0.0;
    return in;
}

bool ik_wants_two_phase(const IkArgs& a, int64_t n, int64_t cap) {
    return ik_wants_two_phase(ik_knobs(), ik_sched_in(a, n, cap));
}

thread_local bool g_ik_partial = false;
bool ik_last_call_partial() { return g_ik_partial; }

// Plan the chunk, fill the arguments, launch.  Two phases (ik_two_phase): phase 1 runs attempt 0 of every
// target on one lane and writes the solved ones; phase 2 runs attempts 1, 2, ... (and attempt 0 resumed, after a
// hand-over) side by side for the ones attempt 0 did not solve, packed densely (fail_list, a ring: IkArgsT).
// Each attempt's arithmetic is unchanged and the lowest converged attempt is still the one written: results are
// identical for every schedule.
template <typename T>
hipError_t launch_ik_dls(const KProg<T>& P, const KStep<T>* steps, const LaunchGeom& g, const IkArgs& a,
                         const T* target, int64_t ldt, const T* q0, T* q, int64_t ldq, int64_t n, int32_t* iters,
                         T* err, int64_t lde, const JitFns* jf, const IkScratch& scr, hipStream_t st) {
    g_ik_partial = false;
    IkArgsT<T> at = ik_args<T>(a);
    const int vr = a.with_rot == 2 ? 2 : a.with_rot ? 1 : 0;
    auto one = [&](IkArgsT<T>& ar, const IkGrid& gr, int64_t s0, int64_t c, bool no_f64 = false) -> hipError_t {
        const int bs = gr.block;
        const int64_t per_wave = gr.per_wave;
        const dim3 grid((unsigned)((gr.waves * 64 + bs - 1) / bs)), block(bs);
        const T* tc = target + s0;
        T* qc = q + s0;
        int32_t* ic = iters ? iters + s0 : iters;
        T* ec = err ? err + s0 : err;
        if (at.trace) ar.trace = at.trace + s0;
        const int vg = ik_lane_index(gr.G);
        // (no_f64: the phase-2 kernel without the fp64 solve, where the launch never takes it)
        const hipFunction_t jk = !jf ? nullptr : no_f64 && jf->ik2[vr][vg] ? jf->ik2[vr][vg] : jf->ik[vr][vg];
        if (jk) {
            int64_t cc = c, pw = per_wave;
            void* args[] = {(void*)&ar, (void*)&tc, (void*)&ldt, (void*)&qc, (void*)&ldq, (void*)&cc,
                            (void*)&ic, (void*)&ec, (void*)&lde, (void*)&pw};
            return hipModuleLaunchKernel(jk, grid.x, 1, 1, (unsigned)bs, 1, 1, 0, st, args, nullptr);
        }
#define KIN_IK_G(MA, R, GX) \
        hipLaunchKernelGGL((k_ik_dls<T, MA, R, GX>), grid, block, 0, st, P, steps, ar, tc, ldt, qc, ldq, c, ic, ec, lde, per_wave)
#define KIN_IK6(MA) \
        switch (gr.G) { case 2: KIN_IK_G(MA, 6, 2); break; case 4: KIN_IK_G(MA, 6, 4); break; \
                        case 8: KIN_IK_G(MA, 6, 8); break; default: KIN_IK_G(MA, 6, 1); }
#define KIN_IK3(MA) \
        switch (gr.G) { case 2: KIN_IK_G(MA, 3, 2); break; case 4: KIN_IK_G(MA, 3, 4); break; \
                        case 8: KIN_IK_G(MA, 3, 8); break; default: KIN_IK_G(MA, 3, 1); }
        if (a.with_rot) {
            KIN_MAXA_DISPATCH(g.maxA, KIN_IK6)
        } else {
            KIN_MAXA_DISPATCH(g.maxA, KIN_IK3)
        }
#undef KIN_IK6
#undef KIN_IK3
#undef KIN_IK_G
        return hipGetLastError();
    };
    // resident workgroups per CU of the plan's specialised G-lane kernel (asked only where the policy needs it)
    auto occupancy = [&](int G) {
        const hipFunction_t f = jf->ik[vr][ik_lane_index(G)];
        int nb = 0;
        return f && hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&nb, f, 256, 0) == hipSuccess ? nb : 0;
    };
    IkSchedIn in = ik_sched_in(a, n, scr.fail_list ? scr.cap : 0);
    in.esz = (int)sizeof(T);
    in.f64_iters = KINHIP_IK_F64_ITERS;
    in.lam2_small = at.lam2 < T(KINHIP_IK_F32SOLVE_MIN_LAM2);
    in.handover_ok = P.flags & PF_BASE ? q0 != nullptr : true;
    in.spec = jf != nullptr;
    // lane byte offsets i * sizeof(T) stay below 2^32; with a scratch set, chunks of at most its capacity
    const int64_t chunk = ik_chunk(in.natt, in.lanes, in.cap);
    for (int64_t s0 = 0; s0 < n; s0 += chunk) {
        at.ibase = a.index_base + s0;
        at.q0 = q0 ? q0 + s0 : nullptr;
        const int64_t c = in.c = std::min(chunk, n - s0);
        const IkSched s = ik_schedule(ik_knobs(), in, occupancy);
        hipError_t e;
        if (!s.two) {
            if ((e = one(at, s.g1, s0, c)) != hipSuccess) return e;
            continue;
        }
        // the ring's control words carry over from the previous call (no reset launch)
        IkArgsT<T> a1 = at;  // phase 1: attempt 0, one lane per target
        a1.n_attempts = 1;
        a1.phase1 = 1;
        a1.fail_list = scr.fail_list;
        a1.fail_ctl = scr.fail_ctl;
        a1.fail_mask = (uint32_t)(scr.ring_cap - 1);
        a1.fail_aux = scr.fail_aux;
        a1.p1_cut = s.p1_cut;
        if ((e = one(a1, s.g1, s0, c)) != hipSuccess) return e;
        IkArgsT<T> a2 = at;  // phase 2: attempts 1.. (0 resumed, after a hand-over) of the listed targets
        a2.att0 = s.att0;
        a2.cont = s.cont;
        a2.p1_cut = s.p1_cut;
        a2.fail_aux = scr.fail_aux;
        a2.idx = scr.fail_list;
        a2.p2_spread = s.p2_spread;
        a2.fail_ctl = scr.fail_ctl;
        a2.fail_mask = (uint32_t)(scr.ring_cap - 1);
        if ((e = one(a2, s.g2, s0, c, s.no_f64)) != hipSuccess) {
            // phase 1 ran but phase 2 did not move the next call's start mark: restart the ring;
            // the targets phase 1 did not solve keep undefined outputs (kin_ik_dls_batch says so)
            (void)hipMemsetAsync(scr.fail_ctl, 0, sizeof(uint32_t) * kIkCtlStride * kIkSubRings, st);
            g_ik_partial = true;
            return e;
        }
    }
    return hipSuccess;
}

template <typename T>
hipError_t launch_nakamura(const KProg<T>& P, const KStep<T>* steps, const LaunchGeom& g, const T* pts,
                           int64_t ldpt, T* q, int64_t ldq, int64_t n, const JitFns* jf, hipStream_t st) {
    for (int64_t s0 = 0; s0 < n; s0 += kChunk) {
        const int64_t c = std::min(kChunk, n - s0);
        const dim3 grid(grid_of(c, 256)), block(256);
        const T* pc = pts + s0;
        T* qc = q + s0;
        if (jf && jf->nakamura) {
            int64_t cc = c;
            void* args[] = {(void*)&pc, (void*)&ldpt, (void*)&qc, (void*)&ldq, (void*)&cc};
            const hipError_t e = hipModuleLaunchKernel(jf->nakamura, grid.x, 1, 1, 256, 1, 1, 0, st, args, nullptr);
            if (e != hipSuccess) return e;
            continue;
        }
#define KIN_NK_LAUNCH(MA) hipLaunchKernelGGL((k_nakamura<T, MA>), grid, block, 0, st, P, steps, pc, ldpt, qc, ldq, c)
        KIN_MAXA_DISPATCH(g.maxA, KIN_NK_LAUNCH)
#undef KIN_NK_LAUNCH
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

#define KIN_INSTANTIATE(T)                                                                                    \
    template hipError_t launch_ik_dls<T>(const KProg<T>&, const KStep<T>*, const LaunchGeom&, const IkArgs&, \
                                         const T*, int64_t, const T*, T*, int64_t, int64_t, int32_t*, T*, int64_t, \
                                         const JitFns*, const IkScratch&, hipStream_t);                                         \
    template hipError_t launch_nakamura<T>(const KProg<T>&, const KStep<T>*, const LaunchGeom&, const T*,    \
                                           int64_t, T*, int64_t, int64_t, const JitFns*, hipStream_t);
KIN_INSTANTIATE(float)
KIN_INSTANTIATE(double)

}  // namespace kinhip
