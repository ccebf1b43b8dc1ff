// What the device's text writers share (flatten_device.hip: FASTA and BED; print_device.hip: GFA text; bed_device.hip: the
// intersect lines): the small device functions of a tile of output bytes, and the pieces on their way to the sink.  HIP only;
// templates and inline functions, so all of them include it.  DESIGN.md sections 15, 19 and 21.
//
// The tile shape is flatten's (flatten_device.hpp): kFlatThreads lanes own kFlatTile consecutive output bytes, form them in
// LDS and store them with 16-byte vector stores; a piece of kFlatPieceBytes is what one launch writes and one copy takes to
// the host.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>

#include "../../include/flatgfa.h"
#include "device_common.hpp"
#include "device_scan.hpp"
#include "flatten_device.hpp"
#include "host_copy.hpp"

namespace fgfa_dev {

static_assert(kFlatTile % (16 * kFlatThreads) == 0, "every lane stores whole 16-byte vectors of a tile");
static_assert(kFlatPieceBytes % kFlatTile == 0 && 2 * kFlatPieceBytes <= kStagingBytes, "two pieces share a staging buffer");
// clipped copies of more than kFlatLongName bytes are disjoint stretches of one tile
constexpr uint32_t kLongCap = kFlatTile / (kFlatLongName + 1) + 2;

// the last index of [lo, hi] whose value is at or before x (a[lo] <= x holds)
__device__ __forceinline__ uint64_t last_at_or_before(const uint64_t *__restrict__ a, uint64_t lo, uint64_t hi, uint64_t x) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo + 1) >> 1);
        if (a[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ uint32_t digits10(uint64_t x) {
    uint32_t n = 1;
    for (uint64_t p = 10; n < 20 && x >= p; p *= 10) ++n;
    return n;
}

// a stretch of a tile that the whole workgroup copies
struct LongCopy {
    const uint8_t *src;
    uint32_t dst, len;
};

// The copy stream, the events and the two piece buffers of a job that delivers text.
struct PieceBufs {
    hipStream_t st = nullptr, copy = nullptr;  // the caller's work stream; the job's own copy stream
    hipEvent_t made[2] = {}, copied[2] = {};   // piece b is formatted / has arrived
    uint8_t *out[2] = {};                      // kFlatPieceBytes each
};

// made once per job; the buffers are `mem`'s.  `who` starts the error's sentence ("flatten: ").
inline int pieces_ready(PieceBufs *j, DeviceMem *mem, hipStream_t st, const char *who) {
    j->st = st;
    mem->st = st;
    if (j->copy) return FLATGFA_OK;
    FGFA_HIP(who, hipStreamCreateWithFlags(&j->copy, hipStreamNonBlocking));
    for (int b = 0; b < 2; ++b) {
        FGFA_HIP(who, hipEventCreateWithFlags(&j->made[b], hipEventDisableTiming));
        FGFA_HIP(who, hipEventCreateWithFlags(&j->copied[b], hipEventDisableTiming));
        FGFA_HIP(who, mem->alloc(&j->out[b], kFlatPieceBytes));
    }
    return FLATGFA_OK;
}

// waits for both streams; the events and the copy stream go (the buffers go with their DeviceMem)
inline void pieces_free(PieceBufs *j) {
    if (j->st) (void)hipStreamSynchronize(j->st);
    if (j->copy) (void)hipStreamSynchronize(j->copy);
    for (hipEvent_t e : {j->made[0], j->made[1], j->copied[0], j->copied[1]})
        if (e) (void)hipEventDestroy(e);
    if (j->copy) (void)hipStreamDestroy(j->copy);
}

// The pieces on their way out.  Piece k is formatted into device buffer k & 1 on the work stream, copied into half k & 1 of
// the borrowed staging buffer on the copy stream, and piece k - 1 is handed to the sink while it travels.
struct Pipe {
    PieceBufs *j;
    FlatSink sink;
    void *ctx;
    const char *who;
    char *pin = nullptr;
    std::unique_lock<std::mutex> lock;
    uint64_t k = 0;
    size_t len[2] = {};
    Pipe(PieceBufs *job, FlatSink s, void *c, const char *w) : j(job), sink(s), ctx(c), who(w) { lock = borrow_staging(&pin); }
    ~Pipe() {  // nothing may still travel into the staging buffer when it goes back
        (void)hipStreamSynchronize(j->st);
        (void)hipStreamSynchronize(j->copy);
    }
    int give(const char *p, size_t n) {
        if (n && sink(ctx, p, n)) {
            set_error(std::string(who) + "the sink stopped the call");
            return FLATGFA_ERR_IO;
        }
        return FLATGFA_OK;
    }
    int retire(int b) {
        FGFA_HIP(who, hipEventSynchronize(j->copied[b]));
        return give(pin + (size_t)b * kFlatPieceBytes, len[b]);
    }
    // launch(out) enqueues on the work stream the kernel that writes the piece's `bytes` bytes to out
    template <class Launch>
    int push(size_t bytes, const Launch &launch) {
        const int b = (int)(k & 1);
        launch(j->out[b]);
        FGFA_HIP(who, hipGetLastError());
        FGFA_HIP(who, hipEventRecord(j->made[b], j->st));
        FGFA_HIP(who, hipStreamWaitEvent(j->copy, j->made[b], 0));
        FGFA_HIP(who, hipMemcpyAsync(pin + (size_t)b * kFlatPieceBytes, j->out[b], bytes, hipMemcpyDeviceToHost, j->copy));
        FGFA_HIP(who, hipEventRecord(j->copied[b], j->copy));
        len[b] = bytes;
        const int rc = k ? retire(b ^ 1) : FLATGFA_OK;  // (whose buffers piece k + 1 takes)
        ++k;
        return rc;
    }
    int finish() { return k ? retire((int)((k - 1) & 1)) : FLATGFA_OK; }
    // `bytes` bytes of tiles, piece by piece: launch(out, first tile, tiles)
    template <class Launch>
    int tiles(uint64_t bytes, const Launch &launch) {
        for (uint64_t at = 0; at < bytes; at += kFlatPieceBytes) {
            const uint64_t n = std::min<uint64_t>(kFlatPieceBytes, bytes - at);
            const uint64_t tile0 = at / kFlatTile;
            const uint32_t nt = (uint32_t)blocks(n, kFlatTile);
            if (int rc = push((size_t)n, [&](uint8_t *out) { launch(out, tile0, nt); })) return rc;
        }
        return FLATGFA_OK;
    }
};

}  // namespace fgfa_dev
