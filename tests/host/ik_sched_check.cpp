// Test-only: the IK launch schedule (kinematics.jl_amd/csrc/kinhip_ik_sched.h) on the host alone: which schedule a
// kin_ik_dls_batch chunk gets and which kernel form a collision-aware IK call gets, field by field, for
// hand-derived cases.  Built by `make -C kinematics.jl_amd/csrc ik-sched-check` under ASan + UBSan
// (tests/test_ik_sched_host.py); no HIP, no device code.  Exit status 0: every check held.
//
// The cases take 256 CUs, hence 2,048 resident waves, and the product's knobs unless they say otherwise.
#include <cstdint>
#include <cstdio>

#include "kinhip_ik_sched.h"

using namespace kinhip;

namespace {

int g_failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            ++g_failures;                                                            \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                            \
    } while (0)
#define CHECK_GRID(g, G_, per_wave_, waves_, block_)                                                        \
    do {                                                                                                    \
        const IkGrid& g_ = (g);                                                                             \
        if (g_.G != (G_) || g_.per_wave != (per_wave_) || g_.waves != (waves_) || g_.block != (block_)) {   \
            ++g_failures;                                                                                   \
            fprintf(stderr, "%s:%d: %s = {G %d, per_wave %lld, waves %lld, block %d}, expected {%s, %s, %s, %s}\n", \
                    __FILE__, __LINE__, #g, g_.G, (long long)g_.per_wave, (long long)g_.waves, g_.block, #G_, \
                    #per_wave_, #waves_, #block_);                                                          \
        }                                                                                                   \
    } while (0)

constexpr int64_t kCap = int64_t(1) << 20;  // a scratch set's capacity (IkScratchSets::kIkScratchCap)

// the occupancy callback: answers `answer` and counts the questions
struct Occ {
    int answer = 0, calls = 0, last_G = 0;
    int operator()(int G) {
        ++calls;
        last_G = G;
        return answer;
    }
};

// The first chunk of an n-target call of bench config 4's shape: max_iters 64, restarts 3 (L = 16, natt = 4),
// lambda^2 = 1e-4, fixed damping, a specialised fp32 plan, a scratch set.
IkSchedIn call(int64_t n, int natt = 4, int lanes = 0, int64_t cap = kCap) {
    IkSchedIn in;
    in.n = n;
    in.L = natt > 1 ? 16 : 0;
    in.natt = natt;
    in.lanes = lanes;
    in.cap = cap;
    in.cus = 256;
    in.esz = 4;
    in.f64_iters = 3;
    in.lam2_small = false;
    in.damped = false;
    in.handover_ok = true;
    in.spec = true;
    in.c = std::min(n, ik_chunk(natt, lanes, cap));
    return in;
}

IkSched plan(const IkKnobs& k, const IkSchedIn& in, Occ& occ) { return ik_schedule(k, in, occ); }
IkSched plan(const IkKnobs& k, const IkSchedIn& in) {
    Occ occ;
    const IkSched s = ik_schedule(k, in, occ);
    CHECK(occ.calls == 0);  // (cases that expect a question pass their own Occ)
    return s;
}

void knob_defaults() {
    const IkKnobs k;
    CHECK(k.group == 0 && k.resident == 0 && k.two_phase == -1 && k.p1_cut == -1 && k.queue == -1 &&
          k.tp_queue == -1 && k.p2_block == 256 && k.p2_spread == 0 && k.ikt_s == 0 && k.ikt_g == 0);
    CHECK(ik_resident_waves(k, 256) == 2048);
    CHECK(kIkChunk == int64_t(1) << 24);
}

void bench_config_4() {
    const IkKnobs k;
    IkSchedIn in = call(65536);
    // lanes: 65,536 * 4 * 2 = 2^19 still fits, and natt = 4 stops the doubling
    CHECK(ik_group(k, in.n, in.natt, 0) == 4);
    // 4,096 waves at 16 targets each > 2,048 resident: two phases
    IkSched s = plan(k, in);
    CHECK(s.two);
    // hand-over at 5/8 of L = 16 (phase 1 is 1,024 waves, one round)
    CHECK(s.p1_cut == 10);
    // phase 1: one lane per target, 1,024 waves <= two rounds: plain grid, nobody asks for the occupancy
    CHECK_GRID(s.g1, 1, 64, 1024, 256);
    // phase 2: attempt 0 resumed beside 1..3 -> 4 lanes, a grid for the whole chunk, block-major, and no fp64 solve
    // (cut 10 >= 3 fp64 iterations, lambda^2 not small)
    CHECK(s.att0 == 0 && s.cont == 1);
    CHECK_GRID(s.g2, 4, 16, 4096, 256);
    CHECK(s.p2_spread == 0);
    CHECK(s.no_f64);

    // error-scaled damping: half an attempt
    in.damped = true;
    s = plan(k, in);
    CHECK(s.two && s.p1_cut == 8 && s.att0 == 0 && s.cont == 1 && s.no_f64);
    in.damped = false;

    // in-place call of a based plan: no hand-over; phase 2 runs attempts 1..3 (still 4 lanes) and never meets
    // attempt 0, so it still drops the fp64 solve
    in.handover_ok = false;
    s = plan(k, in);
    CHECK(s.two && s.p1_cut == 0 && s.att0 == 1 && s.cont == 0 && s.no_f64);
    CHECK_GRID(s.g1, 1, 64, 1024, 256);
    CHECK_GRID(s.g2, 4, 16, 4096, 256);
    in.handover_ok = true;

    // lambda^2 below the fp32 solve's threshold: phase 2 keeps the fp64 solve
    in.lam2_small = true;
    CHECK(!plan(k, in).no_f64);
    in.lam2_small = false;

    // fp64 plans have no such form
    in.esz = 8;
    s = plan(k, in);
    CHECK(s.two && s.p1_cut == 10 && !s.no_f64);
    CHECK_GRID(s.g1, 1, 64, 1024, 256);
    CHECK_GRID(s.g2, 4, 16, 4096, 256);
}

void one_million_targets() {
    const IkKnobs k;
    IkSchedIn in = call(int64_t(1) << 20);
    // lanes: 2^20 * 1 * 2 > 2^19
    CHECK(ik_group(k, in.n, in.natt, 0) == 1);
    // the chunk is the scratch capacity
    CHECK(ik_chunk(in.natt, in.lanes, in.cap) == kCap && in.c == kCap);
    // fp32: 16,384 waves > 2,048: two phases; phase 1 is more than one round, so no hand-over; more than two
    // rounds would mean queues, but the fp32 kernels' fp64 iterations keep the plain grid -- without a question
    IkSched s = plan(k, in);
    CHECK(s.two && s.p1_cut == 0 && s.att0 == 1 && s.cont == 0);
    CHECK_GRID(s.g1, 1, 64, 16384, 256);
    // phase 2: attempts 1..3 -> 4 lanes
    CHECK_GRID(s.g2, 4, 16, 65536, 256);
    CHECK(s.no_f64 && s.p2_spread == 0);

    // fp32 kernels built without fp64 iterations fall under the occupancy rule like fp64
    {
        IkSchedIn v = in;
        v.f64_iters = 0;
        Occ occ{3};
        s = plan(k, v, occ);
        CHECK(occ.calls == 1 && occ.last_G == 1);
        CHECK_GRID(s.g1, 1, 64, 16384, 256);
    }

    // fp64 specialised: one question about the one-lane kernel; more than 2 workgroups per CU (> 2,048 waves
    // resident): plain grid
    in.esz = 8;
    {
        Occ occ{3};
        s = plan(k, in, occ);
        CHECK(occ.calls == 1 && occ.last_G == 1);
        CHECK(s.two && s.p1_cut == 0 && !s.no_f64);
        CHECK_GRID(s.g1, 1, 64, 16384, 256);
        CHECK_GRID(s.g2, 4, 16, 65536, 256);
    }
    // 1 or 2 workgroups per CU (or no answer): the queue of 2,048 resident waves, 512 targets each
    for (int nb = 0; nb <= 2; ++nb) {
        Occ occ{nb};
        s = plan(k, in, occ);
        CHECK(occ.calls == 1 && occ.last_G == 1);
        CHECK_GRID(s.g1, 1, 512, 2048, 256);
    }
    // fp64 generic (no specialised kernels): the queue, and nothing to ask
    in.spec = false;
    s = plan(k, in);
    CHECK(s.two);
    CHECK_GRID(s.g1, 1, 512, 2048, 256);
}

void boundaries() {
    const IkKnobs k;
    // lanes with natt = 4: n * G * 2 <= 2^19
    CHECK(ik_group(k, int64_t(1) << 18, 4, 0) == 2);
    CHECK(ik_group(k, (int64_t(1) << 18) + 1, 4, 0) == 1);
    CHECK(ik_group(k, int64_t(1) << 17, 4, 0) == 4);
    CHECK(ik_group(k, (int64_t(1) << 17) + 1, 4, 0) == 2);
    // a tiny batch: the power of two that covers the attempts, at most 8
    const int want[10] = {0, 1, 2, 4, 4, 8, 8, 8, 8, 8};
    for (int natt = 1; natt <= 9; ++natt) CHECK(ik_group(k, 1, natt, 0) == want[natt]);
    CHECK(ik_group(k, 1, 64, 0) == 8);
    // the caller's lanes win over everything
    CHECK(ik_group(k, int64_t(1) << 20, 4, 8) == 8 && ik_group(k, 1, 4, 1) == 1);

    // two-phase threshold, natt = 4 (G = 4): 2^15 targets are 2,048 waves, exactly one round
    IkSched s = plan(k, call(int64_t(1) << 15));
    CHECK(!s.two);
    CHECK_GRID(s.g1, 4, 16, 2048, 256);
    s = plan(k, call((int64_t(1) << 15) + 1));
    CHECK(s.two && s.p1_cut == 10);
    CHECK_GRID(s.g1, 1, 64, 513, 256);
    CHECK_GRID(s.g2, 4, 16, 2049, 256);

    // one-phase queue (no restarts, one lane): from more than two rounds = 4,096 waves
    s = plan(k, call(4096 * 64, 1));
    CHECK(!s.two);
    CHECK_GRID(s.g1, 1, 64, 4096, 256);
    s = plan(k, call(4096 * 64 + 1, 1));
    CHECK(!s.two);
    CHECK_GRID(s.g1, 1, 129, 2033, 256);  // 2,048 waves share 262,145 targets: 129 each, 2,033 waves cover them

    // the waves share the chunk evenly: 65 targets on 2 waves are 33 each, not 64 + 1
    s = plan(k, call(65, 1));
    CHECK_GRID(s.g1, 1, 33, 2, 256);

    // no restarts: one phase however large
    CHECK(!plan(k, call(int64_t(1) << 20, 1)).two);
    // the caller chose the lanes: one phase at those lanes
    s = plan(k, call(65536, 4, 4));
    CHECK(!s.two);
    CHECK_GRID(s.g1, 4, 16, 4096, 256);
    // a trace call (lanes forced to 1): one phase, one lane
    s = plan(k, call(65536, 4, 1));
    CHECK(!s.two);
    CHECK_GRID(s.g1, 1, 64, 1024, 256);
    // a chunk larger than the capacity: one phase
    {
        IkSchedIn in = call(kCap + 1);
        in.c = kCap + 1;
        CHECK(!plan(k, in).two);
    }

    // a call larger than the capacity with restarts: chunks of the capacity, each two-phase
    {
        IkSchedIn in = call(int64_t(1) << 21);
        CHECK(in.c == kCap && ik_chunk(in.natt, in.lanes, in.cap) == kCap);
        s = plan(k, in);
        CHECK(s.two && s.p1_cut == 0);
        CHECK_GRID(s.g1, 1, 64, 16384, 256);
        CHECK(ik_wants_two_phase(k, in));
        // ... and a short last chunk that alone is one phase (at the whole call's lanes: 1)
        in.n = (int64_t(1) << 21) + 5;
        in.c = 5;
        s = plan(k, in);
        CHECK(!s.two);
        CHECK_GRID(s.g1, 1, 5, 1, 256);
        CHECK(ik_wants_two_phase(k, in));
        // the other way round: only the last chunk would be two-phase -- impossible, every earlier chunk is larger
    }
    // wants: exactly the calls with a two-phase chunk
    CHECK(!ik_wants_two_phase(k, call(int64_t(1) << 15)));
    CHECK(ik_wants_two_phase(k, call((int64_t(1) << 15) + 1)));
    CHECK(!ik_wants_two_phase(k, call(int64_t(1) << 20, 1)));
    CHECK(!ik_wants_two_phase(k, call(int64_t(1) << 20, 4, 1)));

    // no scratch set (capacity 0): chunks of kIkChunk, all one phase
    {
        IkSchedIn in = call(kIkChunk + 3, 4, 0, 0);
        CHECK(ik_chunk(in.natt, in.lanes, in.cap) == kIkChunk && in.c == kIkChunk);
        CHECK(!ik_wants_two_phase(k, in));
        s = plan(k, in);
        CHECK(!s.two);
        CHECK_GRID(s.g1, 1, 8192, 2048, 256);  // the queue: 2,048 waves of 2^24 / 2^11 targets
        in.c = 3;
        s = plan(k, in);
        CHECK(!s.two);
        CHECK_GRID(s.g1, 1, 3, 1, 256);
    }
    // without restarts or with the caller's lanes the capacity does not bound the chunk
    CHECK(ik_chunk(1, 0, kCap) == kIkChunk && ik_chunk(4, 2, kCap) == kIkChunk);
}

void knobs() {
    // KINHIP_IK_GROUP forces the lanes: config 4 at 2 lanes is 2,048 waves -- one phase
    {
        IkKnobs k;
        k.group = 2;
        CHECK(ik_group(k, 65536, 4, 0) == 2 && ik_group(k, 65536, 4, 8) == 8);
        IkSched s = plan(k, call(65536));
        CHECK(!s.two);
        CHECK_GRID(s.g1, 2, 32, 2048, 256);
        k.group = 8;  // 8,192 waves: two phases, and phase 2's lanes follow the attempts, not the knob
        s = plan(k, call(65536));
        CHECK(s.two);
        CHECK_GRID(s.g2, 4, 16, 4096, 256);
        k.group = 3;  // not a kernel form: ignored
        CHECK(ik_group(k, 65536, 4, 0) == 4);
    }
    // KINHIP_IK_RESIDENT = 4 waves per CU: 1,024 resident waves rescale both thresholds
    {
        IkKnobs k;
        k.resident = 4;
        CHECK(ik_resident_waves(k, 256) == 1024);
        CHECK(!plan(k, call(int64_t(1) << 14)).two);  // 1,024 waves at 4 lanes
        IkSched s = plan(k, call((int64_t(1) << 14) + 1));
        CHECK(s.two && s.p1_cut == 10);
        CHECK(!plan(IkKnobs{}, call((int64_t(1) << 14) + 1)).two);
        s = plan(k, call(2048 * 64, 1));  // one-phase queue from more than 2,048 waves
        CHECK_GRID(s.g1, 1, 64, 2048, 256);
        s = plan(k, call(2048 * 64 + 1, 1));
        CHECK_GRID(s.g1, 1, 129, 1017, 256);
        // the hand-over needs phase 1 within 1,024 waves
        CHECK(plan(k, call(65536)).p1_cut == 10 && plan(k, call(65536 + 1)).p1_cut == 0);
    }
    // KINHIP_IK_TWO_PHASE = 0 / 1
    {
        IkKnobs k;
        k.two_phase = 0;
        IkSched s = plan(k, call(65536));
        CHECK(!s.two && !ik_wants_two_phase(k, call(65536)));
        CHECK_GRID(s.g1, 4, 16, 4096, 256);
        k.two_phase = 1;
        s = plan(k, call(64));
        CHECK(s.two && s.p1_cut == 10 && s.att0 == 0 && s.cont == 1 && ik_wants_two_phase(k, call(64)));
        CHECK_GRID(s.g1, 1, 64, 1, 256);
        CHECK_GRID(s.g2, 4, 16, 4, 256);
        // ... but never without restarts, with the caller's lanes or without a scratch set
        CHECK(!plan(k, call(64, 1)).two && !plan(k, call(64, 4, 2)).two && !plan(k, call(64, 4, 0, 0)).two);
    }
    // KINHIP_IK_P1_CUT
    {
        IkKnobs k;
        k.p1_cut = 0;  // no hand-over
        IkSched s = plan(k, call(65536));
        CHECK(s.two && s.p1_cut == 0 && s.att0 == 1 && s.cont == 0 && s.no_f64);
        k.p1_cut = 12;
        s = plan(k, call(65536));
        CHECK(s.p1_cut == 12 && s.att0 == 0 && s.cont == 1 && s.no_f64);
        k.p1_cut = 2;  // attempt 0 resumes inside its fp64 iterations: phase 2 keeps the fp64 solve
        s = plan(k, call(65536));
        CHECK(s.p1_cut == 2 && !s.no_f64);
        k.p1_cut = 16;  // not shorter than the attempt
        CHECK(plan(k, call(65536)).p1_cut == 0);
        k.p1_cut = 12;  // still only while phase 1 is one round, and only where allowed
        CHECK(plan(k, call(int64_t(1) << 20)).p1_cut == 0);
        IkSchedIn in = call(65536);
        in.handover_ok = false;
        CHECK(plan(k, in).p1_cut == 0);
    }
    // KINHIP_IK_QUEUE = 0 / 1: both schedules, and no occupancy question
    {
        IkKnobs k;
        k.queue = 1;
        IkSched s = plan(k, call(int64_t(1) << 18, 1));  // 4,096 waves: no queue by default
        CHECK_GRID(s.g1, 1, 128, 2048, 256);
        CHECK_GRID(plan(IkKnobs{}, call(int64_t(1) << 18, 1)).g1, 1, 64, 4096, 256);
        s = plan(k, call(int64_t(1) << 20));  // phase 1 of the fp32 1M leg on queues
        CHECK(s.two);
        CHECK_GRID(s.g1, 1, 512, 2048, 256);
        k.queue = 0;
        s = plan(k, call((int64_t(1) << 18) + 1, 1));  // 4,097 waves: a queue by default
        CHECK_GRID(s.g1, 1, 64, 4097, 256);
        IkSchedIn in = call(int64_t(1) << 20);
        in.esz = 8;
        s = plan(k, in);  // fp64 1M leg
        CHECK(s.two);
        CHECK_GRID(s.g1, 1, 64, 16384, 256);
    }
    // KINHIP_IK_TP_QUEUE = 0: phase 1 never on queues (the fp64 generic 1M leg has them by default), no question
    {
        IkKnobs k;
        k.tp_queue = 0;
        IkSchedIn in = call(int64_t(1) << 20);
        in.esz = 8;
        in.spec = false;
        CHECK_GRID(plan(k, in).g1, 1, 64, 16384, 256);
        in.spec = true;
        CHECK_GRID(plan(k, in).g1, 1, 64, 16384, 256);
        k.tp_queue = 1;  // forced on: the fp32 1M leg takes the queue, unasked
        CHECK_GRID(plan(k, call(int64_t(1) << 20)).g1, 1, 512, 2048, 256);
    }
    // KINHIP_IK_P2_BLOCK = 64: phase 2 in workgroups of one wave; disables the spread (nothing is asked)
    {
        IkKnobs k;
        k.p2_block = 64;
        k.p2_spread = 2;
        IkSched s = plan(k, call(65536));
        CHECK_GRID(s.g1, 1, 64, 1024, 256);
        CHECK_GRID(s.g2, 4, 16, 4096, 64);
        CHECK(s.p2_spread == 0);
        k.p2_block = 128;  // anything but 64 is 256
        Occ occ{2};
        CHECK(plan(k, call(65536), occ).g2.block == 256 && occ.calls == 1);
    }
    // KINHIP_IK_P2_SPREAD: one question about the phase-2 kernel (4 lanes) per chunk
    {
        IkKnobs k;
        const IkSchedIn in = call(65536);
        k.p2_spread = 1;  // kernels of <= 2 resident workgroups per CU: over those workgroups
        for (int nb = 0; nb <= 3; ++nb) {
            Occ occ{nb};
            const IkSched s = plan(k, in, occ);
            CHECK(occ.calls == 1 && occ.last_G == 4);
            CHECK(s.p2_spread == (nb == 1 ? 256 : nb == 2 ? 512 : 0));
        }
        k.p2_spread = 2;  // every kernel
        for (int nb = 0; nb <= 3; ++nb) {
            Occ occ{nb};
            const IkSched s = plan(k, in, occ);
            CHECK(occ.calls == 1 && occ.last_G == 4);
            CHECK(s.p2_spread == nb * 256);
        }
        k.p2_spread = 3;  // the whole phase-2 grid: 4,096 waves in 1,024 workgroups (still needs an answer)
        {
            Occ occ{3};
            CHECK(plan(k, in, occ).p2_spread == 1024 && occ.calls == 1 && occ.last_G == 4);
            Occ none{0};
            CHECK(plan(k, in, none).p2_spread == 0 && none.calls == 1);
        }
        // generic kernels have no occupancy to ask for: no spread
        IkSchedIn gen = in;
        gen.spec = false;
        CHECK(plan(k, gen).p2_spread == 0);
        // the 1M fp64 leg asks twice: phase 1's one-lane kernel, then phase 2's
        IkSchedIn big = call(int64_t(1) << 20);
        big.esz = 8;
        k.p2_spread = 2;
        Occ occ{2};
        const IkSched s = plan(k, big, occ);
        CHECK(occ.calls == 2 && occ.last_G == 4 && s.p2_spread == 512);
        CHECK_GRID(s.g1, 1, 512, 2048, 256);
    }
}

void collision_ik() {
    const IkKnobs k;
    // the table the variants index
    CHECK(kIktVariants == 4);
    CHECK(kIktS[0] == 1 && kIktG[0] == 1 && kIktS[1] == 1 && kIktG[1] == 4);
    CHECK(kIktS[2] == 16 && kIktG[2] == 1 && kIktS[3] == 16 && kIktG[3] == 4);
    // kin_ik_params.lanes forces a form
    const int lanes[6] = {1, 2, 4, 8, 16, 64}, variant[6] = {0, 1, 1, 1, 2, 3};
    for (int i = 0; i < 6; ++i) CHECK(ikt_variant(k, 1000, 4, lanes[i]) == variant[i]);
    // automatic with restarts: 4 groups up to 2^16 targets, 16 sphere lanes while n * G * 16 <= 2^18
    CHECK(ikt_variant(k, int64_t(1) << 12, 2, 0) == 3);        // 16 x 4
    CHECK(ikt_variant(k, (int64_t(1) << 12) + 1, 2, 0) == 1);  // 1 x 4
    CHECK(ikt_variant(k, int64_t(1) << 16, 2, 0) == 1);
    CHECK(ikt_variant(k, (int64_t(1) << 16) + 1, 2, 0) == 0);  // G = 1, and far too many for S = 16
    // one group (no restarts): S = 16 while n <= 2^14
    CHECK(ikt_variant(k, int64_t(1) << 14, 1, 0) == 2);
    CHECK(ikt_variant(k, (int64_t(1) << 14) + 1, 1, 0) == 0);
    CHECK(ikt_variant(k, 1, 1, 0) == 2);
    // KINHIP_IKT_S / KINHIP_IKT_G override the automatic choice only
    IkKnobs ks;
    ks.ikt_s = 16;
    CHECK(ikt_variant(ks, int64_t(1) << 20, 2, 0) == 2 && ikt_variant(ks, 1 << 16, 2, 0) == 3);
    CHECK(ikt_variant(ks, int64_t(1) << 20, 2, 1) == 0);
    IkKnobs kg;
    kg.ikt_g = 1;
    CHECK(ikt_variant(kg, int64_t(1) << 12, 2, 0) == 2);  // S was chosen for G = 4
    kg.ikt_g = 4;
    CHECK(ikt_variant(kg, 1, 1, 0) == 3 && ikt_variant(kg, int64_t(1) << 20, 1, 0) == 1);
    // a pair no kernel has: the one-lane form
    IkKnobs ku;
    ku.ikt_s = 8;
    CHECK(ikt_variant(ku, 1, 2, 0) == 0);
    ku.ikt_s = 0;
    ku.ikt_g = 2;
    CHECK(ikt_variant(ku, 1, 2, 0) == 0);
    // generic kernel: 4 groups only for lanes 2 / 4 / 8 with restarts and at most 12 variables
    const int all_lanes[7] = {0, 1, 2, 4, 8, 16, 64};
    for (int l : all_lanes) {
        const bool asked = l == 2 || l == 4 || l == 8;
        CHECK(ikt_generic_groups(l, 4, 8) == (asked ? 4 : 1));
        CHECK(ikt_generic_groups(l, 2, 12) == (asked ? 4 : 1));
        CHECK(ikt_generic_groups(l, 1, 8) == 1);
        CHECK(ikt_generic_groups(l, 4, 13) == 1);
    }
}

}  // namespace

int main() {
    knob_defaults();
    bench_config_4();
    one_million_targets();
    boundaries();
    knobs();
    collision_ik();
    if (g_failures) {
        fprintf(stderr, "ik_sched_check: %d checks failed\n", g_failures);
        return 1;
    }
    printf("ik_sched_check: ok\n");
    return 0;
}
