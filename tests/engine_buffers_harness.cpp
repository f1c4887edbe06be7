// tests/engine_buffers_harness.cpp — TEST INFRASTRUCTURE: the out-of-memory rules of denseflow_amd/csrc/engine_buffers.h
// (what every engine's set_size() and ensure_frame_slots() do with a failed allocation) run on the CPU against an
// allocator that fails on command.  tests/test_engine_buffers_cpu.py runs the cases one by one through eb_run(); main()
// runs the same cases, for a stand-alone build under the host sanitizers.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "../denseflow_amd/csrc/engine_buffers.h"

namespace {

// The allocator policy: device memory comes out of a byte budget, the k-th allocation from now (and the n - 1 after it)
// can be told to fail, and every live allocation is on record.
struct FakeAlloc {
    struct Live {
        size_t bytes;
        bool pinned;
    };
    std::map<void *, Live> live;
    size_t budget = (size_t)1 << 40, dev_bytes = 0, peak = 0;
    int calls = 0, fail_from = 0, fail_n = 0; // allocations so far; calls fail_from .. fail_from + fail_n - 1 fail
    bool no_free_bytes = false;
    size_t failed_bytes = 0;
    int failed_code = 0, failures = 0;
    std::string bad; // what the allocator itself saw go wrong (a free of something not live)

    void fail(int k, int n = 1) { fail_from = calls + k, fail_n = n; }
    int get(void **p, size_t bytes, bool pinned) {
        ++calls;
        *p = nullptr;
        if (calls >= fail_from && calls < fail_from + fail_n)
            return 2;
        if (!pinned && dev_bytes + bytes > budget)
            return 2;
        *p = std::malloc(bytes ? bytes : 1);
        live[*p] = Live{bytes, pinned};
        if (!pinned)
            peak = std::max(peak, dev_bytes += bytes);
        return 0;
    }
    void put(void *p, bool pinned) {
        auto it = live.find(p);
        if (it == live.end() || it->second.pinned != pinned) {
            bad = "free of a pointer that is not live, or of the wrong kind";
            return;
        }
        if (!pinned)
            dev_bytes -= it->second.bytes;
        live.erase(it);
        std::free(p);
    }
    int dev(void **p, size_t bytes) { return get(p, bytes, false); }
    int pinned(void **p, size_t bytes) { return get(p, bytes, true); }
    void free_dev(void *p) { put(p, false); }
    void free_pinned(void *p) { put(p, true); }
    int free_bytes(size_t *out) {
        *out = budget - dev_bytes;
        return no_free_bytes ? 1 : 0;
    }
    void failed(size_t bytes, int code) { failed_bytes = bytes, failed_code = code, ++failures; }
    size_t holds(const void *p) const { // bytes of the live allocation at p
        auto it = live.find(const_cast<void *>(p));
        return it == live.end() ? 0 : it->second.bytes;
    }
};

std::string g_msg;
#define CHECK(cond)                                                                                             \
    do {                                                                                                        \
        if (!(cond)) {                                                                                          \
            if (g_msg.empty())                                                                                  \
                g_msg = std::string(#cond) + " (line " + std::to_string(__LINE__) + ")";                        \
            return;                                                                                             \
        }                                                                                                       \
    } while (0)

template <class T> void release(FakeAlloc &a, T *&p, size_t &cap) {
    if (p)
        a.free_dev(p);
    p = nullptr, cap = 0;
}

// ---- the grow-only buffer ---------------------------------------------------------------------------------------
void grow_large_enough_is_untouched(FakeAlloc &a) {
    float *p = nullptr;
    size_t cap = 0;
    CHECK(dfx_grow(a, p, cap, 4096) == DFX_OK && cap == 4096 && a.holds(p) == 4096);
    float *const was = p;
    const int calls = a.calls;
    CHECK(dfx_grow(a, p, cap, 4096) == DFX_OK && dfx_grow(a, p, cap, 100) == DFX_OK && dfx_grow(a, p, cap, 0) == DFX_OK);
    CHECK(p == was && cap == 4096 && a.calls == calls);
    release(a, p, cap);
}

void grow_frees_the_old_buffer_first(FakeAlloc &a) {
    float *p = nullptr;
    size_t cap = 0;
    CHECK(dfx_grow(a, p, cap, 6000) == DFX_OK);
    a.budget = 10000; // old and new together do not fit
    CHECK(dfx_grow(a, p, cap, 9000) == DFX_OK && cap == 9000 && a.holds(p) == 9000);
    CHECK(a.peak == 9000 && a.live.size() == 1 && a.failures == 0);
    release(a, p, cap);
}

void grow_failure_restores_the_old_size(FakeAlloc &a) {
    float *p = nullptr;
    size_t cap = 0;
    CHECK(dfx_grow(a, p, cap, 6000) == DFX_OK);
    a.fail(1);
    CHECK(dfx_grow(a, p, cap, 9000) == DFX_ERR_HIP);
    CHECK(p != nullptr && cap == 6000 && a.holds(p) == 6000 && a.live.size() == 1);
    CHECK(a.failures == 1 && a.failed_bytes == 9000 && a.failed_code == 2 && a.peak == 6000);
    a.budget = 8000; // the same through the budget
    CHECK(dfx_grow(a, p, cap, 9000) == DFX_ERR_HIP && cap == 6000 && a.holds(p) == 6000 && a.peak == 6000);
    release(a, p, cap);
}

void grow_failure_without_restore_leaves_nothing(FakeAlloc &a) {
    float *p = nullptr;
    size_t cap = 0;
    CHECK(dfx_grow(a, p, cap, 6000) == DFX_OK);
    a.fail(1, 2); // the new size and the old size again
    CHECK(dfx_grow(a, p, cap, 9000) == DFX_ERR_HIP);
    CHECK(p == nullptr && cap == 0 && a.live.empty() && a.failures == 1 && a.failed_bytes == 9000);
    a.fail(1); // an empty buffer has no old size to come back to: one allocation, no second attempt
    const int calls = a.calls;
    CHECK(dfx_grow(a, p, cap, 100) == DFX_ERR_HIP && p == nullptr && cap == 0 && a.calls == calls + 1);
    CHECK(dfx_grow(a, p, cap, 100) == DFX_OK && cap == 100);
    release(a, p, cap);
}

// ---- the device + pinned table ----------------------------------------------------------------------------------
void table_grow(FakeAlloc &a, int fail_k) { // fail_k = 0: success; 1: the device array fails; 2: the pinned one
    DfxTable<int> t;
    CHECK(dfx_grow_tables(a, 5, t) && t.cap == 5 && a.holds(t.dev) == 20 && a.holds(t.host) == 20);
    const int src[5] = {4, 3, 2, 1, 0};
    t.stage(src, 5);
    CHECK(t.host[0] == 4 && t.host[4] == 0);
    int *const dev = t.dev, *const host = t.host;
    const int calls = a.calls;
    CHECK(dfx_grow_tables(a, 5, t) && dfx_grow_tables(a, 2, t) && a.calls == calls && t.dev == dev); // large enough
    if (fail_k) {
        a.fail(fail_k);
        CHECK(!dfx_grow_tables(a, 9, t));
        CHECK(t.dev == dev && t.host == host && t.cap == 5 && a.live.size() == 2 && a.holds(dev) == 20 && a.holds(host) == 20);
        CHECK(t.host[0] == 4 && t.new_dev == nullptr && t.new_host == nullptr);
    } else {
        CHECK(dfx_grow_tables(a, 9, t) && t.cap == 9 && a.live.size() == 2 && a.holds(t.dev) == 36 && a.holds(t.host) == 36);
        CHECK(a.holds(dev) == 0 && a.holds(host) == 0 && t.dev != dev && t.host != host); // exactly the old pair went
    }
    t.release(a);
    CHECK(t.cap == 0 && t.dev == nullptr && t.host == nullptr);
}
void table_grow_succeeds(FakeAlloc &a) { table_grow(a, 0); }
void table_device_failure_keeps_the_old_pair(FakeAlloc &a) { table_grow(a, 1); }
void table_pinned_failure_keeps_the_old_pair(FakeAlloc &a) { table_grow(a, 2); }

// TVL1's per-pair arrays: five tables, one of them device-only, nine allocations, all or nothing
struct PairTables {
    DfxTable<double> state{1, false};
    DfxTable<long long> pairs;
    DfxTable<int> iters{160}, checks{32};
    DfxTable<long long> work{32};
    template <class A> bool grow(A &a, int n) { return dfx_grow_tables(a, n, state, pairs, iters, checks, work); }
    template <class A> void release(A &a) { state.release(a), pairs.release(a), iters.release(a), checks.release(a), work.release(a); }
    std::vector<const void *> pointers() const {
        return {state.dev, state.host, pairs.dev, pairs.host, iters.dev, iters.host, checks.dev, checks.host, work.dev, work.host};
    }
};

void per_pair_tables_grow_all_or_nothing(FakeAlloc &a) {
    PairTables t;
    CHECK(t.grow(a, 3) && a.live.size() == 9 && t.state.host == nullptr && t.pairs.cap == 3);
    CHECK(a.holds(t.iters.dev) == 3 * 160 * sizeof(int) && a.holds(t.work.host) == 3 * 32 * sizeof(long long));
    const std::vector<const void *> old = t.pointers();
    for (int k = 1; k <= 9; ++k) {
        a.fail(k);
        const int calls = a.calls;
        CHECK(!t.grow(a, 8));
        CHECK(a.calls == calls + k && t.pointers() == old && a.live.size() == 9); // it stopped there, and nothing leaked
        for (const void *p : old)
            CHECK(p == nullptr || a.holds(p) > 0); // none of the old arrays was freed
        CHECK(t.state.cap == 3 && t.pairs.cap == 3 && t.iters.cap == 3 && t.checks.cap == 3 && t.work.cap == 3);
    }
    CHECK(t.grow(a, 8) && a.live.size() == 9 && t.pairs.cap == 8 && t.work.cap == 8);
    for (const void *p : old)
        CHECK(a.holds(p) == 0);
    t.release(a);
}

// ---- fit_pair_slots ---------------------------------------------------------------------------------------------
void fit_halves_the_batch_until_it_fits(FakeAlloc &a) {
    float *planes = nullptr;
    size_t cap = 0;
    int B = 7, nB = -1;
    a.budget = (size_t)40 << 20; // 129 + 2, 64 + 2 and 32 + 2 pairs of 1 MiB are more than half of 40 MiB, 16 + 2 are not
    CHECK(dfx_fit_pair_slots(a, 129, (size_t)1 << 20, 1000, 0, planes, cap, B, nB) == DFX_OK);
    CHECK(nB == 16 && cap == 16000 && a.holds(planes) == 16000 && B == 7);
    // what the engine holds counts as free: 16000 bytes held make the difference between 4 and 8 pairs
    CHECK(dfx_fit_pair_slots(a, 8, (size_t)2 << 20, 1000, 0, planes, cap, B, nB) == DFX_OK && nB == 4);
    CHECK(dfx_fit_pair_slots(a, 8, (size_t)2 << 20, 1000, 16000, planes, cap, B, nB) == DFX_OK && nB == 8);
    // it never goes below one pair, whatever the memory
    CHECK(dfx_fit_pair_slots(a, 129, (size_t)1 << 30, 1000, 0, planes, cap, B, nB) == DFX_OK && nB == 1);
    CHECK(cap == 16000 && a.live.size() == 1 && B == 7 && a.failures == 0);
    release(a, planes, cap);
}

void fit_falls_back_to_the_held_allocation(FakeAlloc &a) {
    float *planes = nullptr;
    size_t cap = 0;
    int B = 0, nB = -1;
    CHECK(dfx_fit_pair_slots(a, 10, 1, 1000, 0, planes, cap, B, nB) == DFX_OK && nB == 10 && cap == 10000);
    B = nB;
    a.fail(1); // larger frames: ten slots of 3000 bytes cannot be had, the 10000 bytes it held come back
    CHECK(dfx_fit_pair_slots(a, 10, 1, 3000, cap, planes, cap, B, nB) == DFX_OK);
    CHECK(nB == 3 && cap == 10000 && a.holds(planes) == 10000 && B == 10 && a.failed_bytes == 30000);
    a.fail(1); // whole slots only
    CHECK(dfx_fit_pair_slots(a, 4, 1, 2501, cap, planes, cap, B, nB) == DFX_OK && nB == 3);
    a.fail(1);
    CHECK(dfx_fit_pair_slots(a, 2, 1, 5001, cap, planes, cap, B, nB) == DFX_OK && nB == 1);
    CHECK(cap == 10000 && a.holds(planes) == 10000 && B == 10 && a.failures == 3);
    // a plan that fits what it holds allocates nothing
    const int calls = a.calls;
    CHECK(dfx_fit_pair_slots(a, 2, 1, 5000, cap, planes, cap, B, nB) == DFX_OK && nB == 2 && a.calls == calls);
    release(a, planes, cap);
}

void fit_fails_when_not_one_slot_is_held(FakeAlloc &a) {
    float *planes = nullptr;
    size_t cap = 0;
    int B = 0, nB = -1;
    CHECK(dfx_fit_pair_slots(a, 10, 1, 1000, 0, planes, cap, B, nB) == DFX_OK);
    B = nB;
    a.fail(1); // the old array comes back, but a slot is now larger than all of it
    CHECK(dfx_fit_pair_slots(a, 10, 1, 10001, cap, planes, cap, B, nB) == DFX_ERR_HIP);
    CHECK(cap == 10000 && a.holds(planes) == 10000 && B == 10); // the batch in force stands: the old size still runs
    release(a, planes, cap);
}

void fit_reports_batch_0_exactly_when_nothing_came_back(FakeAlloc &a) {
    float *planes = nullptr;
    size_t cap = 0;
    int B = 0, nB = -1;
    CHECK(dfx_fit_pair_slots(a, 10, 1, 1000, 0, planes, cap, B, nB) == DFX_OK);
    B = nB;
    a.fail(1, 2);
    CHECK(dfx_fit_pair_slots(a, 10, 1, 3000, cap, planes, cap, B, nB) == DFX_ERR_HIP);
    CHECK(B == 0 && cap == 0 && planes == nullptr && a.live.empty());
    // a first set_size that fails has nothing to lose either
    B = 0;
    a.fail(1);
    CHECK(dfx_fit_pair_slots(a, 10, 1, 1000, 0, planes, cap, B, nB) == DFX_ERR_HIP && B == 0 && cap == 0);
    // no free-memory figure: nothing is touched
    CHECK(dfx_fit_pair_slots(a, 10, 1, 1000, 0, planes, cap, B, nB) == DFX_OK && cap == 10000);
    B = nB;
    a.no_free_bytes = true;
    const int calls = a.calls;
    CHECK(dfx_fit_pair_slots(a, 10, 1, 3000, cap, planes, cap, B, nB) == DFX_ERR_HIP && a.calls == calls && cap == 10000 && B == 10);
    release(a, planes, cap);
}

// ---- the frame-slot rule ----------------------------------------------------------------------------------------
// An engine's frame-slot half: buffers of mul[i] * (elems or plane) floats per slot, one of them (cond) only with `with_cond`,
// the slot-id table, and the two calls as the engines write them.
struct SlotEngine {
    FakeAlloc &a;
    int n_bufs;
    int mul[4];
    bool by_plane[4]; // the buffer is sized by the scratch plane, not by the frame's elements
    int cond;         // index of the conditional buffer, -1: none
    bool with_cond;
    float *p[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t cap[4] = {0, 0, 0, 0};
    DfxTable<int> ids;
    long long elems = 0, plane = 0; // the geometry in force
    int n_frame_slots = 0;

    size_t each(int i, long long e, long long pl) const { return (size_t)mul[i] * (size_t)(by_plane[i] ? pl : e) * sizeof(float); }
    DfxSlotBufs bufs(long long e, long long pl) {
        DfxSlotBufs s;
        for (int i = 0; i < n_bufs; ++i)
            if (i != cond || with_cond)
                s.add(p[i], cap[i], each(i, e, pl));
        return s;
    }
    int held() { return dfx_frame_slots_held(bufs(elems, plane), ids.cap); }
    int grow(int need, long long e, long long pl) {
        if (const int rc = dfx_grow_slot_bufs(a, bufs(e, pl), need))
            return rc;
        return dfx_grow_tables(a, need, ids) ? DFX_OK : DFX_ERR_HIP;
    }
    int set_size(int need, long long e, long long pl) { // the frame-slot steps of an engine's set_size
        const int rc = grow(need, e, pl);
        if (rc == DFX_OK)
            elems = e, plane = pl;
        dfx_settle_frame_slots(n_frame_slots, rc, held());
        return rc;
    }
    int ensure(int need) {
        if (need <= n_frame_slots)
            return DFX_OK;
        const int rc = grow(need, elems, plane);
        dfx_settle_frame_slots(n_frame_slots, rc, held());
        return rc;
    }
    // what the allocations really hold at the geometry in force, from the allocator's own records
    int truly_held() const {
        size_t n = std::min(a.holds(ids.dev), a.holds(ids.host)) / sizeof(int);
        for (int i = 0; i < n_bufs; ++i)
            if (i != cond || with_cond)
                n = each(i, elems, plane) ? std::min(n, a.holds(p[i]) / each(i, elems, plane)) : 0;
        return (int)n;
    }
    void release() {
        for (int i = 0; i < n_bufs; ++i)
            ::release(a, p[i], cap[i]);
        ids.release(a);
    }
};

// From one starting state, every allocation of a growth fails in turn, alone (the old size comes back) and together with
// the allocation after it (a buffer's old size does not come back either); `resize`: the growth is a set_size to another
// geometry, otherwise an ensure_frame_slots.  Then a call that succeeds.
void slot_rule_walk(FakeAlloc &a, SlotEngine proto, bool resize) {
    const int n_allocs = (proto.cond >= 0 && !proto.with_cond ? proto.n_bufs - 1 : proto.n_bufs) + 2;
    for (int k = 1; k <= n_allocs; ++k)
        for (int n_fail = 1; n_fail <= 2; ++n_fail) {
            SlotEngine e = proto;
            CHECK(e.set_size(5, 1000, 300) == DFX_OK && e.n_frame_slots == 5 && e.truly_held() == 5);
            CHECK(e.ensure(7) == DFX_OK && e.n_frame_slots == 7 && e.truly_held() == 7);
            // a smaller geometry inside the same buffers: more slots than the id table has entries for
            CHECK(e.set_size(6, 500, 100) == DFX_OK && e.n_frame_slots == 7 && e.truly_held() == 7);
            CHECK(e.set_size(4, 1000, 300) == DFX_OK && e.n_frame_slots == 7 && e.truly_held() == 7);
            const int before = e.n_frame_slots;
            a.fail(k, n_fail);
            const int rc = resize ? e.set_size(9, 1500, 700) : e.ensure(12);
            a.fail(0, 0); // a table stops at its first failure: nothing of the order is left over for the next call
            CHECK(rc == DFX_ERR_HIP);
            CHECK(e.elems == 1000 && e.plane == 300);                                        // the geometry in force stands
            CHECK(e.n_frame_slots <= e.truly_held() && e.n_frame_slots <= before);            // never more than is there
            CHECK(e.n_frame_slots == std::min(before, e.truly_held()));                       // and no less than it may keep
            const bool lost = n_fail == 2 && k < n_allocs - 1;                               // a buffer did not come back
            CHECK(e.n_frame_slots == (lost ? 0 : before));
            // the next call finds the memory: what the buffers hold at the new geometry, however far the failed one got
            const int later = resize ? e.set_size(9, 1500, 700) : e.ensure(12);
            CHECK(later == DFX_OK && e.n_frame_slots == e.held() && e.n_frame_slots == e.truly_held());
            CHECK(e.n_frame_slots == (resize ? 9 : 12));
            if (resize)
                CHECK(e.elems == 1500 && e.plane == 700);
            e.release();
            CHECK(a.live.empty());
        }
}

SlotEngine three_equal_buffers(FakeAlloc &a) { // TVL1: I, Ix, Iy
    return SlotEngine{a, 3, {1, 1, 1, 0}, {false, false, false, false}, -1, false};
}
SlotEngine four_unequal_buffers(FakeAlloc &a, bool with_cond) { // Farneback: R, f32 (conditional), tmpv, pyr
    return SlotEngine{a, 4, {1, 1, 2, 1}, {false, true, true, true}, 1, with_cond};
}
void slot_rule_three_equal_buffers_ensure(FakeAlloc &a) { slot_rule_walk(a, three_equal_buffers(a), false); }
void slot_rule_three_equal_buffers_set_size(FakeAlloc &a) { slot_rule_walk(a, three_equal_buffers(a), true); }
void slot_rule_four_unequal_buffers_ensure(FakeAlloc &a) { slot_rule_walk(a, four_unequal_buffers(a, true), false); }
void slot_rule_four_unequal_buffers_set_size(FakeAlloc &a) { slot_rule_walk(a, four_unequal_buffers(a, true), true); }
void slot_rule_without_the_conditional_buffer(FakeAlloc &a) {
    SlotEngine e = four_unequal_buffers(a, false);
    CHECK(e.set_size(5, 1000, 300) == DFX_OK && e.p[1] == nullptr && e.cap[1] == 0 && e.n_frame_slots == 5); // and it is not counted
    e.release();
    slot_rule_walk(a, four_unequal_buffers(a, false), false);
    slot_rule_walk(a, four_unequal_buffers(a, false), true);
}

// A failed set_size may leave a buffer larger than the slots in force need: the count stays, and an engine that has no
// geometry yet counts nothing.
void slot_rule_counts_nothing_new_on_failure(FakeAlloc &a) {
    SlotEngine e = four_unequal_buffers(a, true);
    CHECK(e.held() == 0 && e.truly_held() == 0);
    a.fail(2); // the first set_size fails behind its first buffer
    CHECK(e.set_size(5, 1000, 300) == DFX_ERR_HIP && e.n_frame_slots == 0 && e.cap[0] == 5 * 4000 && e.elems == 0);
    CHECK(e.set_size(5, 1000, 300) == DFX_OK && e.n_frame_slots == 5);
    a.fail(3); // R grows to 9 slots of the new geometry = 13 of the old one, tmpv fails
    CHECK(e.set_size(9, 1500, 700) == DFX_ERR_HIP && e.cap[0] == 9 * 6000 && e.n_frame_slots == 5 && e.truly_held() == 5);
    e.release();
    // The buffers that limit the count grow and a later one fails: more slots are there than are counted.  The count does
    // not rise on a failure; the next call that asks for more gets them without an allocation.
    SlotEngine f = four_unequal_buffers(a, true);
    CHECK(f.set_size(5, 1000, 600) == DFX_OK && f.set_size(20, 250, 75) == DFX_OK && f.n_frame_slots == 20);
    CHECK(f.set_size(4, 1000, 300) == DFX_OK && f.n_frame_slots == 5 && f.truly_held() == 5); // R holds 5, the planes 10
    a.fail(3);
    CHECK(f.set_size(9, 1500, 700) == DFX_ERR_HIP && f.truly_held() == 10 && f.n_frame_slots == 5);
    const int calls = a.calls;
    CHECK(f.ensure(8) == DFX_OK && a.calls == calls && f.n_frame_slots == 10);
    f.release();
}

struct Case {
    const char *name;
    void (*run)(FakeAlloc &);
};
#define CASE(f) Case{#f, f}
const Case kCases[] = {
    CASE(grow_large_enough_is_untouched),
    CASE(grow_frees_the_old_buffer_first),
    CASE(grow_failure_restores_the_old_size),
    CASE(grow_failure_without_restore_leaves_nothing),
    CASE(table_grow_succeeds),
    CASE(table_device_failure_keeps_the_old_pair),
    CASE(table_pinned_failure_keeps_the_old_pair),
    CASE(per_pair_tables_grow_all_or_nothing),
    CASE(fit_halves_the_batch_until_it_fits),
    CASE(fit_falls_back_to_the_held_allocation),
    CASE(fit_fails_when_not_one_slot_is_held),
    CASE(fit_reports_batch_0_exactly_when_nothing_came_back),
    CASE(slot_rule_three_equal_buffers_ensure),
    CASE(slot_rule_three_equal_buffers_set_size),
    CASE(slot_rule_four_unequal_buffers_ensure),
    CASE(slot_rule_four_unequal_buffers_set_size),
    CASE(slot_rule_without_the_conditional_buffer),
    CASE(slot_rule_counts_nothing_new_on_failure),
};
constexpr int kCaseCount = (int)(sizeof kCases / sizeof kCases[0]);

} // namespace

extern "C" {

int eb_case_count() { return kCaseCount; }
const char *eb_case_name(int i) { return i >= 0 && i < kCaseCount ? kCases[i].name : ""; }

// Runs case i on a fresh allocator: 0, or 1 with the first failed check (or what was still allocated at the end) in msg.
int eb_run(int i, char *msg, int cap) {
    if (i < 0 || i >= kCaseCount)
        return -1;
    FakeAlloc a;
    g_msg.clear();
    kCases[i].run(a);
    if (g_msg.empty() && !a.bad.empty())
        g_msg = a.bad;
    if (g_msg.empty() && !a.live.empty())
        g_msg = std::to_string(a.live.size()) + " allocations are live after tear-down";
    for (auto &l : a.live) // a failed check returns before its tear-down
        std::free(l.first);
    if (msg && cap > 0)
        snprintf(msg, (size_t)cap, "%s", g_msg.c_str());
    return g_msg.empty() ? 0 : 1;
}
}

int main() {
    int failed = 0;
    for (int i = 0; i < kCaseCount; ++i) {
        char msg[512];
        const int rc = eb_run(i, msg, (int)sizeof msg);
        printf("%-55s %s%s\n", kCases[i].name, rc ? "FAILED: " : "ok", rc ? msg : "");
        failed += rc != 0;
    }
    return failed ? 1 : 0;
}
