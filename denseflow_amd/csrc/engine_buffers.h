// engine_buffers.h — the capacity half of every engine's set_size() and ensure_frame_slots(): how a buffer grows, what a
// failed growth leaves behind and how many pair and frame slots the engine may then count on.  Pure host logic (no HIP),
// like engine_plan.h: the memory comes from an allocator policy `A`, an object with
//     int  dev(void **p, size_t bytes)      device memory: 0, or the allocator's error code with *p = nullptr
//     int  pinned(void **p, size_t bytes)   page-locked host memory, likewise
//     void free_dev(void *p), free_pinned(void *p)
//     int  free_bytes(size_t *out)          free device memory: 0, or non-zero once it has recorded why not
//     void failed(size_t bytes, int code)   dfx_grow could not get `bytes`: record the error text
// The engines pass DfxHipAlloc (dfx_internal.h); tests/engine_buffers_harness.cpp passes one that fails on command
// (tests/test_engine_buffers_cpu.py).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstring>

#include "../../include/dfx.h"
#include "engine_plan.h"

// Slots of `each` bytes that a buffer of `bytes` holds, as an int.
inline int dfx_slots_in(size_t bytes, size_t each) {
    return each ? (int)std::min<size_t>(bytes / each, (size_t)1 << 30) : 0;
}

// A device buffer that only grows: `cap` is what p holds, in bytes.  Large enough: untouched.  Otherwise the old buffer is
// freed first (a pair-slot array is most of a handle's memory: two of them may not fit) and, should the new allocation
// fail, allocated again at its old size, so that the owner can go on at the size it had; if not even that comes back,
// cap is 0.  Nothing may be using the buffer.
template <class A, class T> inline int dfx_grow(A &a, T *&p, size_t &cap, size_t need) {
    if (need <= cap)
        return DFX_OK;
    if (p)
        a.free_dev(p);
    p = nullptr;
    const int e = a.dev((void **)&p, need);
    if (e == 0) {
        cap = need;
        return DFX_OK;
    }
    if (cap > 0 && a.dev((void **)&p, cap) != 0)
        cap = 0;
    a.failed(need, e);
    return DFX_ERR_HIP;
}

// A small device array of `per` elements of T per entry and (twin) its page-locked copy, which the host fills and
// uploads.  It grows through dfx_grow_tables only: the new arrays first, the old ones freed once every allocation of the
// call has succeeded, so a failure leaves the table as it was.
template <class T> struct DfxTable {
    size_t per = 1;
    bool twin = true;
    T *dev = nullptr, *host = nullptr;
    int cap = 0;                               // entries dev and host hold
    T *new_dev = nullptr, *new_host = nullptr; // inside dfx_grow_tables only

    size_t bytes(int n) const { return sizeof(T) * per * (size_t)n; }
    void stage(const T *src, int n) { std::memcpy(host, src, bytes(n)); }
    template <class A> bool reserve(A &a, int need) {
        return a.dev((void **)&new_dev, bytes(need)) == 0 && (!twin || a.pinned((void **)&new_host, bytes(need)) == 0);
    }
    template <class A> void commit(A &a, int need) {
        release(a);
        dev = new_dev, host = new_host, cap = need;
        new_dev = new_host = nullptr;
    }
    template <class A> void abandon(A &a) { drop(a, new_dev, new_host); }
    template <class A> void release(A &a) {
        drop(a, dev, host);
        cap = 0;
    }

  private:
    template <class A> static void drop(A &a, T *&d, T *&h) {
        if (d)
            a.free_dev(d);
        if (h)
            a.free_pinned(h);
        d = h = nullptr;
    }
};

// Tables that hold the same entries (TVL1's per-pair arrays) grow together, all or nothing.
template <class A, class... Ts> inline bool dfx_grow_tables(A &a, int need, Ts &...t) {
    if (((need <= t.cap) && ...))
        return true;
    const bool ok = (t.reserve(a, need) && ...);
    if (ok)
        (t.commit(a, need), ...);
    else
        (t.abandon(a), ...);
    return ok;
}

// The pair slots of set_size: the planned batch, halved until it fits the memory that is free now plus what the engine
// holds (`held_bytes`) and would give back, then the pair-slot array grown to it.  If that fails the engine goes on in the
// array it had: nB is what that holds at the new slot size, DFX_ERR_HIP if not even one slot.  B, the batch in force, is
// only touched when not even the old array came back: 0, and no FlowBuffer runs until a dfx_set_size succeeds.
template <class A, class T>
inline int dfx_fit_pair_slots(A &a, int batch, size_t per_pair, size_t slot_bytes, size_t held_bytes, T *&planes,
                              size_t &planes_cap, int &B, int &nB) {
    size_t free_b = 0;
    if (a.free_bytes(&free_b) != 0)
        return DFX_ERR_HIP;
    nB = dfx_plan_fit_batch(batch, per_pair, free_b + held_bytes);
    if (dfx_grow(a, planes, planes_cap, slot_bytes * nB) != DFX_OK) {
        if (planes_cap == 0)
            B = 0;
        if (planes_cap < slot_bytes)
            return DFX_ERR_HIP;
        nB = (int)std::min<size_t>(planes_cap / slot_bytes, (size_t)nB); // what the allocation it had holds
    }
    return DFX_OK;
}

// The buffers a frame slot needs, each with the bytes it takes per slot at one geometry.  An engine lists them once per
// geometry; growing and counting both walk the list, so they cannot disagree.
struct DfxSlotBufs {
    struct Buf {
        float **p;
        size_t *cap, each;
    } b[4];
    int n = 0;
    void add(float *&p, size_t &cap, size_t each) { b[n++] = Buf{&p, &cap, each}; }
};

// Every buffer of the list holds `need` frame slots; stops at the first that fails, which dfx_grow leaves at least as
// large as it was, or gone.
template <class A> inline int dfx_grow_slot_bufs(A &a, const DfxSlotBufs &s, int need) {
    for (int i = 0; i < s.n; ++i)
        if (const int rc = dfx_grow(a, *s.b[i].p, *s.b[i].cap, (size_t)need * s.b[i].each))
            return rc;
    return DFX_OK;
}

// Frame slots the buffers hold at the list's geometry, capped by the entries of the slot-id table.
inline int dfx_frame_slots_held(const DfxSlotBufs &s, int slot_ids) {
    int n = slot_ids;
    for (int i = 0; i < s.n; ++i)
        n = std::min(n, dfx_slots_in(*s.b[i].cap, s.b[i].each));
    return n;
}

// The frame-slot count after an attempt (status rc) to grow the frame-slot buffers.  Success: what they hold at the new
// geometry, committed by then.  Failure: the engine goes on at the geometry in force, on no more slots than it counted
// and no more than the buffers still hold there (one of them may be gone).
inline void dfx_settle_frame_slots(int &n_frame_slots, int rc, int held) {
    n_frame_slots = rc == DFX_OK ? held : std::min(n_frame_slots, held);
}
