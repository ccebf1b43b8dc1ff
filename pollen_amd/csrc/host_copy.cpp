// The process's pinned staging pool and the copies that go through it (host_copy.hpp).
#include "host_copy.hpp"
#include <sys/mman.h>
#include <unistd.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

namespace fgfa_dev {
namespace {
constexpr size_t kMiB = (size_t)1 << 20;
constexpr int kMaxThreads = 16, kMaxDevices = 64;

int staging_threads() {
    static const int n = [] {
        const char *e = getenv("FLATGFA_UPLOAD_THREADS");
        return std::min(std::max(e ? atoi(e) : 4, 1), kMaxThreads);
    }();
    return n;
}

// Two buffers per staging thread, made when first wanted and kept (portable: any device copies through them): allocating and
// freeing them per copy cost 2.9 + 3.8 ms of the 17 ms a cfg-L graph took to become resident.  Events belong to a device.
struct Pool {
    std::mutex mu;  // held for the whole of a staged copy, and by a borrower
    char *buf[2 * kMaxThreads] = {};
    hipEvent_t ev[kMaxDevices][2 * kMaxThreads] = {};
    hipError_t ensure(int device, int n) {  // the first n buffers, and device's events for them (device < 0: none)
        for (int i = 0; i < n; ++i) {
            hipError_t e;
            if (!buf[i] && (e = hipHostMalloc((void **)&buf[i], kStagingBytes, hipHostMallocPortable)) != hipSuccess) return buf[i] = nullptr, e;
            if (device >= 0 && !ev[device][i] && (e = hipEventCreateWithFlags(&ev[device][i], hipEventDisableTiming)) != hipSuccess)
                return ev[device][i] = nullptr, e;
        }
        return hipSuccess;
    }
};
Pool &pool() {
    static Pool *p = new Pool();  // never destroyed: the HIP runtime may be gone by the time static destructors run
    return *p;
}

hipError_t plain_copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t stream) {
    if (!stream) return hipMemcpy(dst, src, bytes, kind);
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, stream);
    return e != hipSuccess ? e : hipStreamSynchronize(stream);
}
}  // namespace

hipError_t staged_copy(void *dst_, const void *src_, size_t bytes, hipMemcpyKind kind, hipStream_t stream) {
    if (bytes == 0) return hipSuccess;
    const bool up = kind == hipMemcpyHostToDevice;
    if (bytes < 4 * kMiB || (!up && kind != hipMemcpyDeviceToHost)) return plain_copy(dst_, src_, bytes, kind, stream);
    const bool timing = up && getenv("FLATGFA_TIMING") != nullptr;  // diagnostic: where a large upload spends its time
    const auto t0 = std::chrono::steady_clock::now();
    const auto since = [t0] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    double t_last = 0;
    const auto tick = [&](const char *what) {
        if (timing) fprintf(stderr, "upload: %-31s %8.2f ms\n", what, since() - t_last);
        t_last = since();
    };
    int device = 0;
    hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess) return e;
    if (device < 0 || device >= kMaxDevices) return plain_copy(dst_, src_, bytes, kind, stream);
    const int threads = bytes >= 32 * kMiB ? staging_threads() : 1;
    // (one thread: four-megabyte chunks, so that a copy of a few of them still overlaps the staging with the transfer)
    const size_t chunk = threads == 1 ? 4 * kMiB : kStagingBytes, n_chunks = (bytes + chunk - 1) / chunk;
    Pool &p = pool();
    std::lock_guard<std::mutex> lk(p.mu);
    if (p.ensure(device, 2 * threads) != hipSuccess) {
        (void)hipGetLastError();
        return plain_copy(dst_, src_, bytes, kind, stream);
    }
    tick("pinned buffers + events");

    // Thread t moves chunks t, t + threads, ... through buffers 2t and 2t + 1 in turn.
    char *const dst = (char *)dst_, *const *buf = p.buf;
    const char *const src = (const char *)src_;
    hipEvent_t *const ev = p.ev[device];
    bool busy[2 * kMaxThreads] = {};  // a copy through the buffer is queued and not yet waited for (each written by its thread alone)
    std::atomic<int> failed{hipSuccess};
    const auto fail = [&](hipError_t x) {
        int none = hipSuccess;
        failed.compare_exchange_strong(none, (int)x);  // (the first error is the one reported)
        return false;
    };
    const auto len = [&](size_t c) { return std::min(chunk, bytes - c * chunk); };
    const auto wait = [&](int b) -> hipError_t {
        if (threads > 1) return hipEventSynchronize(ev[b]);
        // one thread: polled, not slept on -- a chunk travels for a tenth of a millisecond, and plan creation waits on these
        hipError_t q;
        while ((q = hipEventQuery(ev[b])) == hipErrorNotReady) {}
        (void)hipGetLastError();  // ("not ready" must not be what a later check of the launches finds)
        return q;
    };
    const auto settle = [&](int b) {
        const hipError_t x = wait(b);
        if (x != hipSuccess) return fail(x);
        busy[b] = false;
        return true;
    };
    const auto queue = [&](size_t c, int b) {
        hipError_t x = up ? hipMemcpyAsync(dst + c * chunk, buf[b], len(c), kind, stream) : hipMemcpyAsync(buf[b], src + c * chunk, len(c), kind, stream);
        if (x == hipSuccess) x = hipEventRecord(ev[b], stream);
        if (x != hipSuccess) return fail(x);
        busy[b] = true;
        return true;
    };
    const auto h2d = [&](int t) {
        int round = 0;
        for (size_t c = (size_t)t; c < n_chunks && !failed; c += threads, ++round) {
            const int b = 2 * t + (round & 1);
            const double t_w = since();
            if (busy[b] && !settle(b)) return;  // the buffer's previous copy is done
            const double t_a = since();
#ifdef MADV_POPULATE_READ
            // a freshly mapped file: let the kernel map the chunk's pages in one go instead of taking a fault per
            // page inside the memcpy (on anonymous memory it only maps what the copy would touch anyway)
            static const uintptr_t page = (uintptr_t)sysconf(_SC_PAGESIZE);
            const uintptr_t a0 = ((uintptr_t)src + c * chunk) & ~(page - 1);
            (void)madvise((void *)a0, ((uintptr_t)src + c * chunk + len(c)) - a0, MADV_POPULATE_READ);
#endif
            memcpy(buf[b], src + c * chunk, len(c));
            const double t_b = since();
            if (!queue(c, b)) return;
            if (timing && t == 0 && round < 3)
                fprintf(stderr, "upload: worker 0 chunk %2d at %6.2f ms (set device %.2f): waited %.2f, fault + stage %.2f, queue %.2f ms\n",
                        round, t_w, 0.0, t_a - t_w, t_b - t_a, since() - t_b);
        }
    };
    const auto d2h = [&](int t) {  // (the chunk before this one is moved out of the other buffer while this one travels)
        int round = 0;
        for (size_t c = (size_t)t; !failed; c += threads, ++round) {
            const int b = 2 * t + (round & 1);
            if (c < n_chunks && !queue(c, b)) return;
            if (round > 0) {
                if (!settle(b ^ 1)) return;
                memcpy(dst + (c - threads) * chunk, buf[b ^ 1], len(c - threads));
            }
            if (c >= n_chunks) return;
        }
    };
    const auto work = [&](int t) {
        if (up) h2d(t);
        else d2h(t);
    };
    std::vector<std::thread> workers;
    for (int t = 1; t < threads; ++t)
        workers.emplace_back([&, t] {
            const hipError_t x = hipSetDevice(device);
            if (x != hipSuccess) fail(x);
            else work(t);
        });
    work(0);
    for (auto &w : workers) w.join();
    tick("workers: fault in, stage, queue");
    // Nothing may still travel through a buffer once the lock is released: every copy queued is waited for, whatever failed.
    e = (hipError_t)failed.load();
    for (int b = 0; b < 2 * threads; ++b) {
        const hipError_t x = busy[b] ? wait(b) : hipSuccess;
        if (e == hipSuccess) e = x;
    }
    if (e != hipSuccess) (void)hipStreamSynchronize(stream);  // (a copy queued without its event)
    tick("copies drained");
    return e;
}

std::unique_lock<std::mutex> borrow_staging(char **buf) {
    Pool &p = pool();
    std::unique_lock<std::mutex> lk(p.mu);
    const bool ok = p.ensure(-1, 1) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    *buf = ok ? p.buf[0] : nullptr;
    return lk;
}

hipError_t warm_staging(int device) {
    if (device < 0 || device >= kMaxDevices) return hipErrorInvalidDevice;
    Pool &p = pool();
    std::lock_guard<std::mutex> lk(p.mu);
    return p.ensure(device, 2 * staging_threads());
}

}  // namespace fgfa_dev
