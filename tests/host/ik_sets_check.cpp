// Test-only: the IK scratch-set scheduler (kinematics.jl_amd/csrc/kinhip_ik_sets.h) on the host alone, with a
// fake runtime backend whose events the test completes, fails, or lets a background "device" thread complete.
// Built by `make -C kinematics.jl_amd/csrc ik-sets-check` once under ThreadSanitizer and once under ASan + UBSan
// (tests/test_ik_sets_host.py); no HIP, no device code.  Exit status 0: every check held.
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

#include "kinhip_ik_sets.h"

namespace {

int g_failures = 0;
std::mutex g_fail_mu;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::lock_guard<std::mutex> lk_(g_fail_mu);                     \
            ++g_failures;                                                   \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                   \
    } while (0)

struct FakeEvent {
    std::atomic<uint64_t> recorded{0}, completed{0};  // complete once completed >= recorded
    std::atomic<int> query_error{0};
    bool done() const { return completed.load() >= recorded.load(); }
    void complete() { completed.store(recorded.load()); }
};

constexpr int kCapturedEvent = 907;
void* const kPerThread = (void*)2;
void* stream_handle(int k) { return (void*)(uintptr_t)(0x1000 + 16 * k); }

struct Fake {
    using Event = FakeEvent*;
    using Error = int;
    static constexpr Error kSuccess = 0, kNotReady = 600;

    // counters and switches of one case (reset())
    static inline std::atomic<int> creates{0}, destroys{0}, records{0}, syncs{0}, drains{0}, allocs{0}, frees{0};
    static inline std::atomic<int> last_error{0}, fail_record{0};
    static inline std::atomic<FakeEvent*> last_synced{nullptr};
    // the set whose lease the calling thread is about to commit, and per set the event / stream of its last
    // commit.  Plain (not atomic) on purpose: only the scheduler orders one holder of a set after the previous
    // one, so ThreadSanitizer reports a scheduler that lets two calls overlap on a set.
    static inline thread_local int committing = -1;
    static inline FakeEvent* set_event[8] = {};
    static inline void* set_stream[8] = {};
    // the "device": completes recorded events in order after a short delay (threaded case)
    static inline std::atomic<bool> device_on{false};
    static inline std::mutex dev_mu;
    static inline std::condition_variable dev_cv;
    static inline std::deque<std::pair<FakeEvent*, uint64_t>> dev_queue;

    static void reset() {
        creates = destroys = records = syncs = drains = allocs = frees = 0;
        last_error = fail_record = 0;
        last_synced = nullptr;
        for (auto& e : set_event) e = nullptr;
        for (auto& s : set_stream) s = nullptr;
    }

    static Error event_create(Event* e) {
        *e = new FakeEvent;
        ++creates;
        return kSuccess;
    }
    static void event_destroy(Event e) {
        delete e;
        ++destroys;
    }
    static Error event_query(Event e) {
        if (const int err = e->query_error.load()) {
            last_error = err;
            return err;
        }
        return e->done() ? kSuccess : kNotReady;
    }
    static Error event_synchronize(Event e) {
        ++syncs;
        last_synced = e;
        if (device_on) {
            while (!e->done()) std::this_thread::yield();
        } else {
            e->complete();  // (a real wait ends when the work does)
        }
        return kSuccess;
    }
    static Error event_record(Event e, void* stream) {
        if (fail_record) return last_error = 1;
        ++records;
        const uint64_t gen = ++e->recorded;
        if (committing >= 0) {
            set_event[committing] = e;
            set_stream[committing] = stream;
        }
        if (device_on) {
            std::lock_guard<std::mutex> lk(dev_mu);
            dev_queue.emplace_back(e, gen);
            dev_cv.notify_one();
        }
        return kSuccess;
    }
    static void stream_synchronize(void*) { ++drains; }
    static bool is_per_thread(void* stream) { return stream == kPerThread; }
    static Error alloc_zeroed(void** p, size_t bytes) {
        *p = calloc(1, bytes);
        ++allocs;
        return kSuccess;
    }
    static void free(void* p) {
        ::free(p);
        ++frees;
    }
    static Error clear_last_error() { return last_error.exchange(0); }
};

using Sets = kinhip::IkScratchSets<Fake>;
static_assert(Sets::kIkEagerSets == 4 && Sets::kIkScratchSets == 8, "the cases below are written for 4 + 4 sets");
constexpr size_t kSetBytes = 256;

// acquire / "launch" / commit on `stream`; returns the set
int call(Sets& s, void* stream) {
    Sets::Lease l = s.acquire(stream, false, kSetBytes);
    CHECK(l.fail == Sets::kOk && l.set() >= 0 && l.set() < Sets::kIkEagerSets && l.base());
    Fake::committing = l.set();
    const int set = l.set();
    l.commit(stream);
    Fake::committing = -1;
    return set;
}

void case_a() {  // one explicit handle: the same set every time, ordered by the stream alone
    Fake::reset();
    Sets s;
    const int first = call(s, stream_handle(1));
    for (int k = 1; k < 6; ++k) CHECK(call(s, stream_handle(1)) == first);
    const kin_ik_sched_stats st = s.stats();
    CHECK(st.set_waits == 0 && Fake::syncs == 0 && st.two_phase_calls == 6 && Fake::allocs == 1);
}

void case_b() {  // two explicit handles alternating: one set each, no waits
    Fake::reset();
    Sets s;
    const int s1 = call(s, stream_handle(1)), s2 = call(s, stream_handle(2));
    CHECK(s1 != s2);
    for (int k = 0; k < 3; ++k) CHECK(call(s, stream_handle(1)) == s1 && call(s, stream_handle(2)) == s2);
    CHECK(s.stats().set_waits == 0 && Fake::syncs == 0 && s.stats().busy_waits == 0);
}

void case_c() {  // the per-thread handle never matches by handle
    // Present behaviour; ADVICE r06 item 2 intends to change it (the same-thread host wait of call 5): the
    // next pull request may edit the assertions of this case.
    Fake::reset();
    Sets s;
    bool seen[4] = {};
    int first = -1;
    for (int k = 0; k < 4; ++k) {
        const int set = call(s, kPerThread);
        if (k == 0) first = set;
        CHECK(!seen[set]);
        seen[set] = true;
    }
    FakeEvent* lru_event = Fake::set_event[first];
    CHECK(Fake::syncs == 0);
    CHECK(call(s, kPerThread) == first);  // the least recently taken set
    CHECK(Fake::syncs == 1 && Fake::last_synced == lru_event && s.stats().set_waits == 1);
}

void case_d() {  // as c with set 2's call finished: that set, no wait
    Fake::reset();
    Sets s;
    for (int k = 0; k < 4; ++k) CHECK(call(s, kPerThread) == k);
    Fake::set_event[2]->complete();
    CHECK(call(s, kPerThread) == 2);
    CHECK(Fake::syncs == 0 && s.stats().set_waits == 0);
}

void case_e() {  // captures: refused before the first allocation, then sets 4..7 for good, then one phase
    Fake::reset();
    Sets s;
    {
        Sets::Lease l = s.acquire(stream_handle(1), true, kSetBytes);
        CHECK(l.fail == Sets::kFirstCallInCapture && l.set() < 0 && Fake::allocs == 0);
    }
    call(s, stream_handle(1));
    for (int k = 0; k < 4; ++k) {
        Sets::Lease l = s.acquire(stream_handle(1), true, kSetBytes);
        CHECK(l.fail == Sets::kOk && l.set() == 4 + k && l.base());
        l.commit(stream_handle(1));  // (nothing to record for a graph's set)
    }
    CHECK(s.stats().captured_calls == 4 && Fake::records == 1);
    {
        Sets::Lease l = s.acquire(stream_handle(1), true, kSetBytes);
        CHECK(l.fail == Sets::kOk && l.set() < 0 && !l.base());
    }
    CHECK(s.stats().captured_calls == 4 && s.stats().captured_one_phase == 1);
    for (int k = 0; k < 8; ++k) call(s, k % 2 ? kPerThread : stream_handle(2 + k));  // (call() checks set < 4)
    CHECK(s.stats().two_phase_calls == 9 && s.stats().one_phase_fallbacks == 0);
}

void case_f() {  // a per-thread set whose event reports an error: complete, event replaced, error cleared
    Fake::reset();
    Sets s;
    CHECK(call(s, kPerThread) == 0);
    Fake::set_event[0]->query_error = kCapturedEvent;
    const int creates = Fake::creates, destroys = Fake::destroys;
    CHECK(call(s, kPerThread) == 0);
    CHECK(Fake::creates == creates + 1 && Fake::destroys == destroys + 1 && Fake::last_error == 0);
    CHECK(Fake::syncs == 0 && s.stats().set_waits == 0);
}

void case_g() {  // the same error on an explicit handle's set: returned, and the set is free again
    Fake::reset();
    Sets s;
    for (int k = 0; k < 4; ++k) CHECK(call(s, stream_handle(k)) == k);
    FakeEvent* e0 = Fake::set_event[0];
    e0->query_error = kCapturedEvent;
    {
        Sets::Lease l = s.acquire(stream_handle(9), false, kSetBytes);  // least recently used: set 0
        CHECK(l.fail == Sets::kOrdering && l.error == kCapturedEvent && l.set() < 0);
    }
    e0->query_error = 0;
    e0->complete();
    CHECK(call(s, stream_handle(9)) == 0);  // at once: not left busy
    CHECK(s.stats().busy_waits == 0);
}

void case_h() {  // a lease dropped without commit: the set is free, nothing recorded
    Fake::reset();
    Sets s;
    {
        Sets::Lease l = s.acquire(stream_handle(1), false, kSetBytes);
        CHECK(l.fail == Sets::kOk && l.set() == 0);
    }
    CHECK(Fake::records == 0);
    CHECK(call(s, stream_handle(2)) == 0);
    CHECK(Fake::records == 1 && s.stats().busy_waits == 0);
}

void case_i() {  // a failed event record drains the stream
    Fake::reset();
    Sets s;
    Fake::fail_record = 1;
    call(s, stream_handle(1));
    CHECK(Fake::drains == 1);
    Fake::fail_record = 0;
    call(s, stream_handle(1));
    CHECK(Fake::drains == 1);
}

// 6 threads on the per-thread handle and 2 on explicit handles against a device thread
void case_threads(int rounds) {
    Fake::reset();
    Sets s;
    std::atomic<int> holder[Sets::kIkEagerSets] = {};
    static int scribble[Sets::kIkEagerSets];  // plain: the "launch" writes the set it holds
    std::atomic<bool> stop{false};
    Fake::device_on = true;
    std::thread device([&] {
        std::unique_lock<std::mutex> lk(Fake::dev_mu);
        for (;;) {
            Fake::dev_cv.wait(lk, [&] { return stop || !Fake::dev_queue.empty(); });
            if (Fake::dev_queue.empty()) return;
            const auto [e, gen] = Fake::dev_queue.front();
            Fake::dev_queue.pop_front();
            lk.unlock();
            std::this_thread::sleep_for(std::chrono::microseconds(5));
            e->completed.store(gen);
            lk.lock();
        }
    });
    auto worker = [&](void* stream) {
        for (int r = 0; r < rounds; ++r) {
            Sets::Lease l = s.acquire(stream, false, kSetBytes);
            CHECK(l.fail == Sets::kOk && l.set() >= 0 && l.set() < Sets::kIkEagerSets);
            const int set = l.set();
            CHECK(holder[set].exchange(1) == 0);  // no set is held by two leases
            // the "launch" starts after the set's previous call finished, unless the stream itself orders them
            const FakeEvent* prev = Fake::set_event[set];
            CHECK(!prev || prev->done() || (stream != kPerThread && Fake::set_stream[set] == stream));
            ++scribble[set];
            std::this_thread::yield();
            holder[set] = 0;
            Fake::committing = set;
            l.commit(stream);
            Fake::committing = -1;
        }
    };
    std::vector<std::thread> th;
    for (int k = 0; k < 6; ++k) th.emplace_back(worker, kPerThread);
    for (int k = 0; k < 2; ++k) th.emplace_back(worker, stream_handle(k));
    for (auto& t : th) t.join();
    {
        std::lock_guard<std::mutex> lk(Fake::dev_mu);
        stop = true;
    }
    Fake::dev_cv.notify_one();
    device.join();
    Fake::device_on = false;
    const kin_ik_sched_stats st = s.stats();
    CHECK(st.two_phase_calls == uint64_t(8) * rounds && st.one_phase_fallbacks == 0);
    int total = 0;
    for (int v : scribble) total += v;
    CHECK(total == 8 * rounds);
    printf("threads: %d rounds x 8, set_waits %llu busy_waits %llu\n", rounds, (unsigned long long)st.set_waits,
           (unsigned long long)st.busy_waits);
}

}  // namespace

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 300;
    case_a();
    case_b();
    case_c();
    case_d();
    case_e();
    case_f();
    case_g();
    case_h();
    case_i();
    CHECK(Fake::creates == Fake::destroys && Fake::allocs == Fake::frees);  // (of the last case: all released)
    case_threads(rounds);
    if (g_failures) {
        fprintf(stderr, "%d check(s) failed\n", g_failures);
        return 1;
    }
    printf("ik_sets_check: ok\n");
    return 0;
}
