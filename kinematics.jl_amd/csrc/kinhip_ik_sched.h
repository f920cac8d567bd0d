// kinhip_ik_sched.h -- how an IK call is laid out on the chip: the schedule of a kin_ik_dls_batch chunk
// (launch_ik_dls) and the lanes of a collision-aware IK target (launch_ik_tree).
//
// Host only and pure: no runtime call, no environment read, no device code.  The launchers fill the knobs
// once and the inputs per chunk, and launch what the decision says; the occupancy of a specialised kernel
// reaches the policy as a callback, asked only where a rule needs it.  So the policy also builds with the
// host compiler alone and is asserted case by case in tests/host/ik_sched_check.cpp
// (tests/test_ik_sched_host.py, `make ik-sched-check`).
#pragma once
#include <stdint.h>

#include <algorithm>

#include "kinhip_prog.h"

namespace kinhip {

// The A/B knobs of the schedule (tools/ab.py's list) with the product's values; the launchers overwrite
// them from the environment in the A/B build only (ab_env_int).
struct IkKnobs {
    int group = 0;       // KINHIP_IK_GROUP=<1|2|4|8>: lanes per target (0: automatic)
    int resident = 0;    // KINHIP_IK_RESIDENT=<waves per CU that count as resident> (0: 8)
    int two_phase = -1;  // KINHIP_IK_TWO_PHASE=<0|1> (-1: automatic)
    int p1_cut = -1;     // KINHIP_IK_P1_CUT=<iterations> (0 disables the hand-over; -1: automatic)
    int queue = -1;      // KINHIP_IK_QUEUE=<0|1>: wave-local queues (-1: automatic)
    int tp_queue = -1;   // KINHIP_IK_TP_QUEUE=<0|1>: phase 1 of a large batch on queues (-1: automatic)
    int p2_block = 256;  // KINHIP_IK_P2_BLOCK=<64|256>: phase 2's workgroup
    int p2_spread = 0;   // KINHIP_IK_P2_SPREAD=<0 never | 1 kernels of <= 2 resident workgroups per CU | 2 always |
                         // 3 whole grid>
    int ikt_s = 0;       // KINHIP_IKT_S / KINHIP_IKT_G: sphere lanes / attempt groups of k_ik_tree (0: automatic)
    int ikt_g = 0;
};

// What the policy reads of one chunk of a call.
struct IkSchedIn {
    int64_t n = 0;         // targets of the whole call
    int64_t c = 0;         // targets of this chunk
    int L = 0, natt = 1;   // attempt length and attempts (ik_attempts)
    int lanes = 0;         // kin_ik_params.lanes (0: automatic; trace calls force 1)
    int64_t cap = 0;       // targets the call's scratch set takes (0: no scratch set)
    int cus = 256;         // compute units of the device
    int esz = 4;           // bytes per element: 4 (fp32) or 8
    int f64_iters = 0;     // KINHIP_IK_F64_ITERS: iterations of attempt 0 the fp32 kernels solve in fp64
    bool lam2_small = false;   // lambda^2, in the plan's type, below KINHIP_IK_F32SOLVE_MIN_LAM2
    bool damped = false;       // error-scaled damping (damp_err > 0)
    bool handover_ok = true;   // false: an in-place call of a based plan (the hand-over would overwrite the start
                               // pose that attempts 1, 2, ... begin from)
    bool spec = false;         // the plan has specialised kernels (only their occupancy can be asked)
};

// One launch: G lanes per target, `waves` waves that each work through `per_wave` targets, workgroups of `block`.
struct IkGrid {
    int G = 1;
    int64_t per_wave = 0, waves = 0;
    int block = 256;
};

struct IkSched {
    bool two = false;
    IkGrid g1;  // the one-phase launch, or phase 1 (attempt 0, one lane per target)
    // two-phase only
    int p1_cut = 0;          // IkArgsT::p1_cut of both phases (0: phase 1 runs the whole attempt)
    IkGrid g2;               // phase 2: attempts att0.. of the listed targets side by side
    int att0 = 0, cont = 0;  // 0 / 1 after a hand-over (attempt 0 resumes on slot 0), else 1 / 0
    int p2_spread = 0;       // IkArgsT::p2_spread
    bool no_f64 = false;     // phase 2 runs the kernels compiled without the fp64 solve
};

// index of a G-lane kernel in JitFns::ik / ik2 (log2 of the lanes per target)
inline int ik_lane_index(int G) { return G == 1 ? 0 : G == 2 ? 1 : G == 4 ? 2 : 3; }

// Lanes per IK target (parallel restart attempts): enough to put ~8 waves on every SIMD for small batches,
// never more than the attempts the schedule has.
inline int ik_group(const IkKnobs& k, int64_t n, int natt, int lanes) {
    const int forced = lanes ? lanes : k.group;
    if (forced == 1 || forced == 2 || forced == 4 || forced == 8) return forced;
    int g = 1;
    while (g < natt && g < 8 && n * g * 2 <= (int64_t(1) << 19)) g *= 2;
    return g;
}

// waves that stay resident: 2 per SIMD for the generic kernels (~190-240 VGPRs)
inline int64_t ik_resident_waves(const IkKnobs& k, int cus) { return (int64_t)cus * (k.resident > 0 ? k.resident : 8); }

// Launch chunk of a call: kIkChunk (32-bit lane offsets), and with restarts at most the two-phase scratch
// capacity, so that a batch larger than one list still runs the two-phase schedule chunk by chunk (in stream
// order on the call's scratch set).  2M targets: 1.20 ms on the one-phase queue before.
inline int64_t ik_chunk(int natt, int lanes, int64_t cap) {
    return natt > 1 && lanes == 0 && cap > 0 ? std::min<int64_t>(kIkChunk, cap) : kIkChunk;
}

// Two phases for a chunk when the caller left the lanes to the engine, there are restart attempts, the chunk
// fits the scratch set and it needs more than one round of resident waves at the one-phase schedule's lanes
// per target: small batches fill the chip only by running a target's attempts side by side, and a wave then
// lasts as long as any of its targets' attempts.
inline bool ik_two_phase(const IkKnobs& k, const IkSchedIn& in) {
    if (in.natt <= 1 || in.c > in.cap || in.lanes != 0) return false;
    const int64_t ng = 64 / ik_group(k, in.n, in.natt, in.lanes);
    const int64_t plain = (in.c + ng - 1) / ng;
    return k.two_phase >= 0 ? k.two_phase != 0 : plain > ik_resident_waves(k, in.cus);
}

// true when some chunk of the call runs two phases (only then does the call need a scratch set); in.c is ignored
inline bool ik_wants_two_phase(const IkKnobs& k, IkSchedIn in) {
    const int64_t chunk = ik_chunk(in.natt, in.lanes, in.cap);
    for (int64_t s0 = 0; s0 < in.n; s0 += chunk) {
        in.c = std::min<int64_t>(chunk, in.n - s0);
        if (ik_two_phase(k, in)) return true;
    }
    return false;
}

// Phase-1 hand-over point: 5/8 of an attempt.  Config 4 (L = 16): 23% of the targets are still unsolved after
// 10 iterations (46% after 8, 4% after 16; oracle histogram), so phase 2 keeps about one wave per SIMD:
// 0.081 ms vs 0.089 (no hand-over), 0.092 (cut 8), 0.084 (cut 12) fp32 and 0.165 / 0.179 / 0.236 / 0.170 ms
// fp64 (profiles/r03_ik_handover.txt).  With error-scaled damping attempt 0 converges sooner (93% within 10
// iterations) and half an attempt is the faster cut: config 4 damped 0.079 ms at cut 8 vs 0.088 at 10 (fixed
// lambda: 0.141 vs 0.082; profiles/r04_ik_p1_cut_ab.txt).  0 when not allowed or not shorter than L.
inline int ik_p1_cut(const IkKnobs& k, int L, bool allowed, bool damped) {
    const int cut = k.p1_cut >= 0 ? k.p1_cut : damped ? L / 2 : (5 * L) / 8;
    return allowed && cut > 0 && cut < L ? cut : 0;
}

// The schedule of one chunk.  occ(G): the workgroups of 256 per CU that the plan's specialised G-lane kernel
// keeps resident, 0 when there is none or the runtime cannot tell; asked at most once per phase.
template <class Occ>
IkSched ik_schedule(const IkKnobs& k, const IkSchedIn& in, Occ&& occ) {
    const int64_t resident = ik_resident_waves(k, in.cus);
    // waves of the chunk at one target per group of G lanes
    const auto plain = [&](int G) { return (in.c + 64 / G - 1) / (64 / G); };
    // wave-local queues once that is more than two rounds of resident waves
    const auto queue_at = [&](int G) { return k.queue >= 0 ? k.queue != 0 : plain(G) > 2 * resident; };
    // one target per group (no refill), or a queue: as many waves as stay resident, each working through its share
    const auto grid = [&](int G, bool queue) {
        const int64_t w = queue ? std::min(resident, plain(G)) : plain(G);
        IkGrid g;
        g.G = G;
        g.per_wave = (in.c + w - 1) / w;
        g.waves = (in.c + g.per_wave - 1) / g.per_wave;
        return g;
    };
    IkSched s;
    s.two = ik_two_phase(k, in);
    if (!s.two) {
        const int G = ik_group(k, in.n, in.natt, in.lanes);
        s.g1 = grid(G, queue_at(G));
        return s;
    }
    const bool knobs_auto = k.tp_queue < 0 && k.queue < 0;
    // Early hand-over: phase 1 lasts `cut` iterations instead of L, and phase 2 (16 targets per wave at G = 4)
    // absorbs the handed-over targets at no extra latency while it stays within ~2 waves per SIMD (one wave
    // alone issues every other VALU slot).  Only while phase 1 is one round of resident waves: a larger batch is
    // throughput-bound, and the hand-over would add the speculative attempts 1, 2, ... of every handed-over
    // target that attempt 0 still solves (1M targets: 0.55 -> 0.59 ms).
    const int64_t plain1 = (in.c + 63) / 64;
    s.p1_cut = plain1 <= resident ? ik_p1_cut(k, in.L, in.handover_ok, in.damped) : 0;
    // Phase 1 shares out targets like the one-phase schedule, with two exceptions.
    bool q1 = k.tp_queue != 0 && queue_at(1);
    // The fp32 kernels solve attempt 0's first f64_iters iterations in fp64: on a queue a lane group that takes
    // its next target runs those while the rest of the wave is in fp32, so nearly every wave iteration pays both
    // solves.  The plain grid starts a wave's targets together (1M targets: 0.607 -> 0.502 ms, identical
    // results; profiles/r05_ik_1m_queue_ab.txt).
    if (in.esz == 4 && in.f64_iters > 0 && knobs_auto) q1 = false;
    // A queue of `resident` waves must not run fewer waves per CU than the kernel could hold: where the hardware
    // keeps more (the fp32 specialised kernel, 3 per SIMD), the full grid backfilled by the dispatcher is faster
    // (profiles/r02_ik_queue_ab.txt).
    if (q1 && knobs_auto && in.spec && (int64_t)occ(1) * 4 * in.cus > resident) q1 = false;
    s.g1 = grid(1, q1);
    s.att0 = s.p1_cut ? 0 : 1;
    s.cont = s.p1_cut ? 1 : 0;
    const int na2 = in.natt - s.att0;
    s.g2.G = na2 <= 1 ? 1 : na2 <= 2 ? 2 : na2 <= 4 ? 4 : 8;
    s.g2.per_wave = 64 / s.g2.G;  // (the grid of a list of the whole chunk)
    s.g2.waves = plain(s.g2.G);
    s.g2.block = k.p2_block == 64 ? 64 : 256;
    // Phase 2's list fills only the first waves of its grid (one wave per SIMD or less).  With p2_spread its
    // waves are dealt slot-major over the workgroups the chip holds at once (the phase-2 kernel's resident
    // workgroups), so a short list spreads over every CU and never reaches a workgroup that waits for a slot.
    // Off by default (block-major, round 3's order): measured in round 5 (profiles/r05_ik_p2_ab2.txt) the
    // spread costs the fp32 kernels (config 4 fixed lambda 0.071 -> 0.089 ms, damped 0.072 -> 0.084) and fp64 at
    // fixed lambda (0.154 -> 0.163), and helps only damped fp64 (0.171 -> 0.158).  Value 3 is round 4's form,
    // the spread over the WHOLE grid: the fp64 kernel, two resident workgroups
    // per CU, then ran a 1,000-wave list in two rounds of one busy wave per workgroup (config 4 fp64 0.145 ->
    // 0.365 ms, BENCH_r04; A/B profiles/r05_ik_p2_ab.txt).
    if (k.p2_spread != 0 && s.g2.block == 256 && in.spec) {
        const int nb = occ(s.g2.G);
        if (nb > 0 && (nb <= 2 || k.p2_spread > 1))
            s.p2_spread = k.p2_spread == 3 ? (int)((s.g2.waves * 64 + 255) / 256) : nb * in.cus;
    }
    // Phase 2 never takes the fp32 kernels' fp64 solve (ik_body: attempt 0 before iteration f64_iters, or a small
    // lambda^2) when attempt 0 resumes at or past that iteration and lambda is not below the threshold: the form
    // compiled without that code, the same arithmetic, then runs -- config 4 0.072-0.074 -> 0.070 ms on one box,
    // identical results (profiles/r06_ik_p2_nof64_ab.txt).
    s.no_f64 = in.esz == 4 && !in.lam2_small && (s.p1_cut == 0 || s.p1_cut >= in.f64_iters);
    return s;
}

// Collision-aware IK (k_ik_tree).  Sphere lanes S and attempt groups G of the specialised kernels, by
// JitFns::ikt index: G groups run a target's restart attempts side by side, S sphere lanes per group share
// out its spheres -- identical results for every (S, G).
constexpr int kIktVariants = 4;
constexpr int kIktS[kIktVariants] = {1, 1, 16, 16};
constexpr int kIktG[kIktVariants] = {1, 4, 1, 4};

// The specialised kernel of a call.  Small batches fill the chip only with more lanes per target (the bistage
// solve's few thousand targets are a fraction of a wave per SIMD): G = 4 while there are restart attempts and
// up to 2^16 targets, S = 16 while the whole batch stays within ~4 waves per SIMD (n * G * 16 <= 2^18 lanes),
// else S = 1.  kin_ik_params.lanes forces a form: 1 = one lane, 2 / 4 / 8 = 4 attempt groups of one lane,
// 16 = 16 sphere lanes x 1, 64 = 16 x 4.
inline int ikt_variant(const IkKnobs& k, int64_t n, int natt, int lanes) {
    if (lanes == 1) return 0;
    if (lanes == 2 || lanes == 4 || lanes == 8) return 1;
    if (lanes == 16) return 2;
    if (lanes == 64) return 3;
    int G = natt >= 2 && n <= (int64_t(1) << 16) ? 4 : 1;
    int S = n * G * 16 <= (int64_t(1) << 18) ? 16 : 1;
    if (k.ikt_s) S = k.ikt_s;
    if (k.ikt_g) G = k.ikt_g;
    for (int v = 0; v < kIktVariants; ++v)
        if (kIktS[v] == S && kIktG[v] == G) return v;
    return 0;
}

// attempt groups of the generic kernel: side by side only when the caller asks for them (lanes 2 / 4 / 8);
// wide trees (more than 12 variables) run one lane group
inline int ikt_generic_groups(int lanes, int natt, int nv) {
    return (lanes == 2 || lanes == 4 || lanes == 8) && natt > 1 && nv <= 12 ? 4 : 1;
}

}  // namespace kinhip
