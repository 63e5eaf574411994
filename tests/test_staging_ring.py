"""CPU-only: the flow control of the pinned staging ring (sitator_amd/csrc/staging_ring.h) compiled with the host compiler,
the way test_clamp_point.py builds its probe, once under TSan and once under ASan / UBSan, and run against a fake device:
two "DMA" threads, one per lane, execute their queues in order with a short pseudo-random delay per copy and signal
per-slot events.  The fake keeps a state per slot and checks the slot's bytes against the truth, and aborts when
  * a DMA is issued from a slot that is not staged (upload) or into a slot that has not been copied out (download),
  * a slot is written while its DMA is pending (upload: the DMA then finds other bytes than were issued),
  * a slot is reused before the event of its previous DMA was waited for, or an event is waited for that nobody recorded.
A small geometry (16 slots, chunks of a few hundred bytes) takes a thousand chunks round the ring in milliseconds.  Every
run has a timeout, so a deadlock fails the test instead of hanging it."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = 16

# probe geom <bytes> <chunk> <stride>: prints the number of chunks, then "offset length slot slot_offset" per chunk.
# probe up|down <bytes> <chunk> <stride> <threads> <fail_at>: one transfer; fail_at >= 0: the fake's copy of that chunk fails.
# Exit 0: the transfer did what was expected (arrived byte for byte with the guard intact, or returned the failure).
PROBE = r"""
#include <stdio.h>
#include <condition_variable>
#include <deque>
#include <mutex>
#include "staging_ring.h"

#define DIE(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); abort(); } while (0)

enum { FREE, IN_FLIGHT, DONE };
static const unsigned char POISON = 0xFF;                       // the truth never holds it

struct Fake {
    struct Op { size_t slot; char *slot_mem; size_t off, n, seq; };   // slot_mem == nullptr: the event of the slot
    struct Lane { std::deque<Op> q; std::thread t; };
    bool upload;
    RingGeometry g;
    char *device;                                               // the device range
    const char *truth;                                          // what the range holds (download) or must receive (upload)
    const char *host_dst;                                       // download: where the copy threads put the chunks
    size_t bytes;
    long long fail_at;
    std::mutex m;                                               // queues, events, counters
    std::condition_variable cv;
    Lane lane[2];
    bool stop = false;
    size_t seq = 0, pushed = 0, finished = 0, recorded[RING_SLOTS] = {0}, passed[RING_SLOTS] = {0};
    std::atomic<int> state[RING_SLOTS];
    std::atomic<int> prepared{0};

    Fake(bool up, const RingGeometry &geo, char *dev, const char *tr, const char *hd, size_t b, long long fail)
        : upload(up), g(geo), device(dev), truth(tr), host_dst(hd), bytes(b), fail_at(fail)
    {
        for (auto &s : state) s.store(FREE);
        for (int l = 0; l < 2; l++) lane[l].t = std::thread([this, l] { run(l); });
    }
    ~Fake()
    {
        { std::lock_guard<std::mutex> k(m); stop = true; }
        cv.notify_all();
        for (auto &l : lane) l.t.join();
    }
    void run(int l)
    {
        unsigned r = 2463534242u + (unsigned)l;
        for (;;) {
            Op op;
            {
                std::unique_lock<std::mutex> k(m);
                cv.wait(k, [&] { return stop || !lane[l].q.empty(); });
                if (lane[l].q.empty()) return;
                op = lane[l].q.front();
                lane[l].q.pop_front();
            }
            if (op.slot_mem) {
                r ^= r << 13; r ^= r >> 17; r ^= r << 5;
                if (r % 4 == 0) std::this_thread::sleep_for(std::chrono::microseconds(r % 40)); else std::this_thread::yield();
                if (upload) {
                    if (memcmp(op.slot_mem, truth + op.off, op.n)) DIE("slot %zu was written while its DMA was pending", op.slot);
                    memcpy(device + op.off, op.slot_mem, op.n);
                    memset(op.slot_mem, POISON, op.n);
                } else memcpy(op.slot_mem, device + op.off, op.n);
                if (state[op.slot].exchange(DONE) != IN_FLIGHT) DIE("slot %zu: DMA done on a slot not in flight", op.slot);
            }
            { std::lock_guard<std::mutex> k(m); if (!op.slot_mem) passed[op.slot] = op.seq; finished++; }
            cv.notify_all();
        }
    }
    void push(int l, const Op &op)
    {
        { std::lock_guard<std::mutex> k(m); lane[l].q.push_back(op); pushed++; }
        cv.notify_all();
    }
    int lane_of(size_t i) const { return upload ? (int)(i & 1) : 0; }

    bool enqueue(size_t i, size_t slot, char *slot_mem, size_t off, size_t n)
    {
        if ((long long)i == fail_at) return false;
        if (slot != g.slot(i) || off != g.offset(i) || n != g.length(i, bytes) || n == 0) DIE("chunk %zu: wrong arithmetic", i);
        if (state[slot].exchange(IN_FLIGHT) != FREE) DIE("slot %zu reused before the event of its previous DMA was waited for", slot);
        if (upload) { if (memcmp(slot_mem, truth + off, n)) DIE("DMA of chunk %zu issued from a slot that is not staged", i); }
        else if (i >= g.slots && memcmp(host_dst + g.offset(i - g.slots), truth + g.offset(i - g.slots), g.chunk))
            DIE("DMA of chunk %zu issued into a slot that has not been copied out", i);
        push(lane_of(i), {slot, slot_mem, off, n, 0});
        return true;
    }
    bool record(size_t i, size_t slot)
    {
        size_t s;
        { std::lock_guard<std::mutex> k(m); s = recorded[slot] = ++seq; }
        push(lane_of(i), {slot, nullptr, 0, 0, s});
        return true;
    }
    bool wait(size_t slot)
    {
        std::unique_lock<std::mutex> k(m);
        const size_t target = recorded[slot];
        if (!target) DIE("slot %zu: wait for an event that was never recorded", slot);
        cv.wait(k, [&] { return passed[slot] >= target; });
        if (state[slot].exchange(FREE) != DONE) DIE("slot %zu: event passed but the DMA is not done", slot);
        return true;
    }
    bool prepare_worker() { prepared++; return true; }
    bool drain()
    {
        std::unique_lock<std::mutex> k(m);
        cv.wait(k, [&] { return finished == pushed; });
        return true;
    }
};

static int threads_now()
{
    FILE *f = fopen("/proc/self/status", "r");
    char line[256];
    int n = -1;
    while (f && fgets(line, sizeof(line), f)) if (sscanf(line, "Threads: %d", &n) == 1) break;
    if (f) fclose(f);
    return n;
}

int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    const size_t bytes = (size_t)atoll(argv[2]);
    const RingGeometry g = {RING_SLOTS, (size_t)atoll(argv[4]), (size_t)atoll(argv[3])};
    if (!strcmp(argv[1], "geom")) {
        printf("%zu\n", g.chunks(bytes));
        for (size_t i = 0; i < g.chunks(bytes); i++) printf("%zu %zu %zu %zu\n", g.offset(i), g.length(i, bytes), g.slot(i), g.slot_offset(i));
        return 0;
    }
    if (argc < 7) return 2;
    const bool up = !strcmp(argv[1], "up");
    const int threads = atoi(argv[5]);
    const long long fail_at = atoll(argv[6]);
    const size_t guard = 64;
    std::vector<char> src(bytes), dst(bytes + guard, (char)0xA5), ring(g.slots * g.stride, (char)POISON);
    for (size_t k = 0; k < bytes; k++) src[k] = (char)(((unsigned)k * 2654435761u >> 13) % 251);
    bool ok;
    {
        // upload: src is the host buffer, dst the device range; download: src the device range, dst the host buffer
        Fake dev(up, g, up ? dst.data() : src.data(), src.data(), dst.data(), bytes, fail_at);
        const int threads_before = threads_now();              // with the fake's two lanes
        ok = up ? ring_upload(g, ring.data(), src.data(), bytes, threads, dev) : ring_download(g, ring.data(), dst.data(), bytes, threads, dev);
        // nothing of the ring's is running when the call is back (a joined thread can take a moment to leave the list)
        for (int tries = 0; threads_now() != threads_before; tries++) {
            if (tries == 1000) DIE("%d threads before the call, %d after it", threads_before, threads_now());
            std::this_thread::sleep_for(std::chrono::microseconds(100));
        }
        if (!up && ok && dev.prepared.load() != (int)std::min((size_t)threads, g.chunks(bytes))) DIE("copy threads not prepared");
    }
    for (size_t k = bytes; k < bytes + guard; k++) if (dst[k] != (char)0xA5) DIE("guard byte %zu overwritten", k - bytes);
    if (fail_at >= 0) {
        if (ok) DIE("the failure of chunk %lld was not returned", fail_at);
        return 0;
    }
    if (!ok) DIE("the transfer failed");
    if (memcmp(dst.data(), src.data(), bytes)) DIE("destination differs from source");
    return 0;
}
"""

BUILDS = {"tsan": ["-fsanitize=thread"], "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
# (chunk, stride): chunks that fill their slot, and chunks at the front of a wider slot (SITATOR_RING_CHUNK_KB)
GEOMETRIES = [(320, 320), (200, 512)]


def sizes(chunk):
    """1 byte; one chunk; one lap; one lap and a chunk; 3 laps + 1 chunks with a partial tail; not a multiple of 8; and a
    thousand chunks."""
    return [1, chunk, SLOTS * chunk, (SLOTS + 1) * chunk, 3 * SLOTS * chunk + 123, 5 * chunk + 13, 1000 * chunk + 7]


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    td = tmp_path_factory.mktemp("staging_ring")
    src = td / "probe.cpp"
    src.write_text(PROBE)
    exes = {}
    for name, flags in BUILDS.items():
        exes[name] = str(td / ("probe_" + name))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-pthread"] + flags
                              + ["-I", os.path.join(ROOT, "sitator_amd", "csrc"), str(src), "-o", exes[name]])
    return exes


def run(exe, *args):
    p = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0 and not p.stderr, "%s: exit %d\n%s" % (" ".join(str(a) for a in args), p.returncode, p.stderr.decode()[-3000:])
    return p.stdout.decode()


def test_chunk_arithmetic(probes):
    for chunk, stride in GEOMETRIES:
        for b in sizes(chunk):
            out = run(probes["asan_ubsan"], "geom", b, chunk, stride).split("\n")
            n = -(-b // chunk)
            assert int(out[0]) == n
            got = np.array([line.split() for line in out[1:1 + n]], dtype=np.int64)
            i = np.arange(n)
            assert np.array_equal(got, np.stack([i * chunk, np.minimum(chunk, b - i * chunk), i % SLOTS, i % SLOTS * stride], axis=1))


@pytest.mark.parametrize("threads", [1, 8])
@pytest.mark.parametrize("direction", ["up", "down"])
@pytest.mark.parametrize("build", list(BUILDS))
def test_every_byte_arrives_and_nothing_beyond(probes, build, direction, threads):
    for chunk, stride in GEOMETRIES:
        for b in sizes(chunk):
            run(probes[build], direction, b, chunk, stride, threads, -1)


@pytest.mark.parametrize("threads", [1, 8])
@pytest.mark.parametrize("direction", ["up", "down"])
@pytest.mark.parametrize("build", list(BUILDS))
def test_a_failed_copy_is_returned_after_every_thread_has_joined(probes, build, direction, threads):
    """The fake's copy fails at the first chunk, in the second lap and at the last chunk (a host-side fault of the fake):
    the call returns the failure, the copy threads are gone, no sanitizer has anything to say."""
    chunk, stride = GEOMETRIES[0]
    b = 3 * SLOTS * chunk + 123
    for fail_at in (0, 20, 3 * SLOTS):
        run(probes[build], direction, b, chunk, stride, threads, fail_at)
