// Large copies between pageable host memory and the device: the HIP side of the pinned staging ring (staging_ring.h
// has the flow control and why it is the way it is).  One ring per process, shared by the contexts of every device and
// held for the length of a copy; its slot events belong to a device, so there is a set per device, created at the
// device's first staged copy and kept.
#include "sit_internal.h"
#include "staging_ring.h"

#include <array>
#include <mutex>

static std::mutex g_ring_mutex;
static char *g_ring = nullptr;
static std::vector<std::array<hipEvent_t, RING_SLOTS>> g_slot_ev;       // [device]

// with g_ring_mutex held and c->device current
static bool ring_ready(sit_ctx *c)
{
    if (!g_ring && hipHostMalloc((void **)&g_ring, RING_SLOTS * RING_SLOT_BYTES) != hipSuccess) { g_ring = nullptr; return false; }
    if (g_slot_ev.size() <= (size_t)c->device) g_slot_ev.resize((size_t)c->device + 1, std::array<hipEvent_t, RING_SLOTS>{});
    for (hipEvent_t &e : g_slot_ev[(size_t)c->device])
        if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { e = nullptr; return false; }
    return true;
}

// SITATOR_RING_CHUNK_KB (tests and diagnostics): chunks shorter than a slot, so that a small copy goes round the ring
static RingGeometry ring_geometry()
{
    return {RING_SLOTS, RING_SLOT_BYTES, (size_t)ring_env("SITATOR_RING_CHUNK_KB", 1, (long long)(RING_SLOT_BYTES >> 10), (long long)(RING_SLOT_BYTES >> 10)) << 10};
}

// The one size policy: is this copy big enough to stage?  Below, the runtime's own pageable copy is as good.
static bool staged(hipMemcpyKind kind, size_t bytes)
{
    if (kind == hipMemcpyHostToDevice) return bytes >= ring_geometry().chunk;
    return bytes >= (size_t)ring_env("SITATOR_STAGED_D2H_MB", 0, 1ll << 40, 64) << 20;
}

struct HipRing {
    sit_ctx *c;
    hipMemcpyKind kind;
    char *device_range;
    hipStream_t lane[2];                                        // chunk i goes on lane[i & 1]
    bool enqueue(size_t i, size_t, char *slot_mem, size_t off, size_t n)
    {
        char *d = device_range + off;
        return hipMemcpyAsync(kind == hipMemcpyHostToDevice ? d : slot_mem, kind == hipMemcpyHostToDevice ? slot_mem : d, n, kind, lane[i & 1]) == hipSuccess;
    }
    bool record(size_t i, size_t slot) { return hipEventRecord(g_slot_ev[(size_t)c->device][slot], lane[i & 1]) == hipSuccess; }
    bool wait(size_t slot) { return hipEventSynchronize(g_slot_ev[(size_t)c->device][slot]) == hipSuccess; }
    bool prepare_worker() { return hipSetDevice(c->device) == hipSuccess; }
    bool drain()
    {
        const bool ok = hipStreamSynchronize(lane[0]) == hipSuccess;
        return (lane[1] == lane[0] || hipStreamSynchronize(lane[1]) == hipSuccess) && ok;
    }
};

// Part of the trajectory for sit_upload_fill_fit's helper thread: on the two copy streams, c->stream is left alone, and
// c->msg too (the other thread owns it).  Returns when the range has arrived.
int upload_range(sit_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (bytes == 0) return SIT_OK;
    std::lock_guard<std::mutex> lock(g_ring_mutex);
    if (!ring_ready(c)) return SIT_ERR_HIP;
    HipRing dev = {c, hipMemcpyHostToDevice, (char *)dst, {c->copy_stream, c->copy_stream2}};
    return ring_upload(ring_geometry(), g_ring, (const char *)src, bytes, ring_threads("SITATOR_COPY_THREADS"), dev) ? SIT_OK : SIT_ERR_HIP;
}

// A pageable host buffer to the device, complete on return.
int copy_to_device(sit_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (bytes == 0) return SIT_OK;
    if (!staged(hipMemcpyHostToDevice, bytes)) {
        HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return SIT_OK;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));                 // whatever read dst before is done
    const int rc = upload_range(c, dst, src, bytes);
    if (rc) c->msg = "staged host-to-device copy failed";
    return rc;
}

// The device to a pageable host buffer, ordered behind the work on c->stream.  On return the copy is either complete
// (staged) or enqueued on c->stream (small): the caller's hipStreamSynchronize(c->stream) finishes it either way.
int copy_to_host(sit_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (bytes == 0) return SIT_OK;
    if (!staged(hipMemcpyDeviceToHost, bytes)) {
        HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
        return SIT_OK;
    }
    std::lock_guard<std::mutex> lock(g_ring_mutex);
    if (!ring_ready(c)) { c->msg = "pinned staging ring"; return SIT_ERR_HIP; }
    HipRing dev = {c, hipMemcpyDeviceToHost, (char *)src, {c->stream, c->stream}};
    if (ring_download(ring_geometry(), g_ring, (char *)dst, bytes, ring_threads("SITATOR_D2H_THREADS"), dev)) return SIT_OK;
    c->msg = "staged device-to-host copy failed";
    return SIT_ERR_HIP;
}
