// The pinned staging ring between pageable host memory and the device, without the device: the ring's arithmetic and
// the two transfer loops, in a form the host compiler takes (tests/test_staging_ring.py runs them with g++ under TSan
// and ASan / UBSan against a fake device).  The only thing that knows HIP is the `Dev` the loops are given
// (transfer.hip has the real one):
//   bool enqueue(i, slot, slot_mem, off, n)   a copy of n bytes between slot_mem and byte `off` of the device range
//   bool record(i, slot)                      the slot's event, behind that copy
//   bool wait(slot)                           until the slot's event, as last recorded, has passed
//   bool prepare_worker()                     once on every copy thread that will wait for events
//   bool drain()                              until everything enqueued is done
// each false on failure.
//
// Host -> device: copy threads (8; SITATOR_COPY_THREADS) fill 4 MB slots, each slot leaves by DMA as soon as it is
// staged - the pieces alternating between TWO streams - and is reused once its DMA has finished.  Measured on the MI355X
// box (scratch/ring_probe.hip, 1.38 GB): a plain hipMemcpy of pageable memory 56 GB/s (but it holds the runtime's lock
// against other threads' launches while it runs); this ring with ONE stream 46 GB/s whatever the slots, piece size,
// threads, pinned-memory flags or way of waiting (36-40 GB/s beside the fit's kernels: until round 4 the fit was the
// longer leg and nobody noticed); with two streams 55 GB/s.
// Device -> host: the DMA of a slot is enqueued on one stream, copy threads move finished slots to their place.  A plain
// hipMemcpy of 0.9 GB into a fresh numpy array runs at 18 GB/s (one thread copies out of the runtime's staging buffer
// and takes the page faults of the new array); eight threads (SITATOR_D2H_THREADS) share both: the page faults of the
// fresh destination are the cost (C3: 0.092 -> 0.070 s from four).
#pragma once

#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>
#include <vector>

#define RING_SLOTS 16
#define RING_SLOT_BYTES ((size_t)4 << 20)

// `slots` slots `stride` bytes apart; chunk i of a copy is `chunk` bytes (the last one what is left) at the front of
// slot i % slots
struct RingGeometry {
    size_t slots, stride, chunk;
    size_t chunks(size_t bytes) const { return (bytes + chunk - 1) / chunk; }
    size_t offset(size_t i) const { return i * chunk; }
    size_t length(size_t i, size_t bytes) const { return std::min(chunk, bytes - i * chunk); }
    size_t slot(size_t i) const { return i % slots; }
    size_t slot_offset(size_t i) const { return slot(i) * stride; }
};

// an integer from the environment, read at every call (a getenv beside a copy of megabytes costs nothing, and a test
// can set it): `dflt` when unset or outside [lo, hi]
inline long long ring_env(const char *name, long long lo, long long hi, long long dflt)
{
    const char *v = getenv(name);
    const long long n = v && *v ? atoll(v) : lo - 1;
    return n >= lo && n <= hi ? n : dflt;
}
inline int ring_threads(const char *name) { return (int)ring_env(name, 1, 32, 8); }

template <class Ready>
inline void ring_poll(Ready ready)
{
    while (!ready()) std::this_thread::sleep_for(std::chrono::microseconds(10));
}

// Up to `want_threads` copy threads run start() and then per_chunk(i) for the chunks they claim, in order, while this
// thread runs issue().  Returns when all of them have joined: issue() and per_chunk must let every chunk through,
// whatever failed, because they hold references to the caller's stack.
template <class Start, class PerChunk, class Issue>
inline void ring_run(int want_threads, size_t nchunks, Start start, PerChunk per_chunk, Issue issue)
{
    std::atomic<size_t> next(0);
    std::vector<std::thread> pool;
    for (size_t t = 0; t < std::min((size_t)want_threads, nchunks); t++)
        pool.emplace_back([&]() {
            start();
            for (size_t i; (i = next.fetch_add(1)) < nchunks;) per_chunk(i);
        });
    issue();
    for (auto &t : pool) t.join();
}

// src[0, bytes) to the device range of `dev`.  The copy threads stage chunk i once `released` > i; this thread sends the
// staged chunks in order and hands a slot back after waiting for the event of the chunk issued half a ring earlier, so
// staging runs at most one ring ahead of the DMA that has finished.  A failure is sticky: nothing more is enqueued, the
// events recorded until then are still waited for (no slot is refilled under a DMA), and the loop runs to the end so
// that every copy thread gets through its chunks.  Returns when the whole range has arrived.
template <class Dev>
inline bool ring_upload(const RingGeometry &g, char *ring, const char *src, size_t bytes, int want_threads, Dev &dev)
{
    const size_t nchunks = g.chunks(bytes), lag = g.slots / 2;
    std::vector<std::atomic<int>> staged(nchunks);
    for (auto &f : staged) f.store(0);
    std::atomic<size_t> released(g.slots);
    bool ok = true;
    size_t recorded = 0;                                        // chunks enqueued with their event
    ring_run(want_threads, nchunks, [] {},
        [&](size_t i) {
            ring_poll([&] { return released.load(std::memory_order_acquire) > i; });
            memcpy(ring + g.slot_offset(i), src + g.offset(i), g.length(i, bytes));
            staged[i].store(1, std::memory_order_release);
        },
        [&]() {
            for (size_t i = 0; i < nchunks; i++) {
                ring_poll([&] { return staged[i].load(std::memory_order_acquire) != 0; });
                if (ok) {
                    ok = dev.enqueue(i, g.slot(i), ring + g.slot_offset(i), g.offset(i), g.length(i, bytes)) && dev.record(i, g.slot(i));
                    if (ok) recorded = i + 1;
                }
                if (i + 1 >= lag) {                             // the slot of the oldest chunk in flight is handed back once its DMA is done
                    const size_t done = i + 1 - lag;
                    if (done < recorded && !dev.wait(g.slot(done))) ok = false;
                    released.store(done + 1 + g.slots, std::memory_order_release);
                }
            }
        });
    return dev.drain() && ok;
}

// The device range of `dev` to dst[0, bytes).  This thread waits until the chunk that had the slot a ring earlier has
// been copied out (`freed`), enqueues, records and publishes `issued`; the copy threads wait for the slot's event and
// copy out.  A failure is sticky: nothing more is enqueued or copied, every chunk still counts as issued and freed so
// that the copy threads get through the list, and what was enqueued is drained before the return.  Returns when
// everything has arrived.
template <class Dev>
inline bool ring_download(const RingGeometry &g, char *ring, char *dst, size_t bytes, int want_threads, Dev &dev)
{
    const size_t nchunks = g.chunks(bytes);
    std::vector<std::atomic<int>> freed(nchunks);
    for (auto &f : freed) f.store(0);
    std::atomic<size_t> issued(0);
    std::atomic<int> failed(0);
    ring_run(want_threads, nchunks, [&] { if (!dev.prepare_worker()) failed.store(1); },
        [&](size_t i) {
            ring_poll([&] { return issued.load(std::memory_order_acquire) > i || failed.load(); });
            if (!failed.load() && !dev.wait(g.slot(i))) failed.store(1);
            if (!failed.load()) memcpy(dst + g.offset(i), ring + g.slot_offset(i), g.length(i, bytes));
            freed[i].store(1, std::memory_order_release);
        },
        [&]() {
            for (size_t i = 0; i < nchunks && !failed.load(); i++) {
                if (i >= g.slots) ring_poll([&] { return freed[i - g.slots].load(std::memory_order_acquire) != 0; });
                if (!dev.enqueue(i, g.slot(i), ring + g.slot_offset(i), g.offset(i), g.length(i, bytes)) || !dev.record(i, g.slot(i)))
                    failed.store(1);
                issued.store(i + 1, std::memory_order_release);
            }
        });
    if (failed.load()) { (void)dev.drain(); return false; }
    return true;
}
