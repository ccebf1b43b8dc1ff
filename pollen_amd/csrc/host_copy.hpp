// Copies between the host's pageable (or file-mapped) memory and the device: the one place that decides how they travel.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstddef>
#include <mutex>

namespace fgfa_dev {

// A copy that returns when the bytes have arrived, ordered behind the work already queued on `stream` (nullptr: the null
// stream).  From four megabytes up it goes through the process's own pinned staging buffers: the runtime would otherwise pin
// the caller's pages for the transfer, and pages registered with the GPU that the kernel then moves or unmaps cost the
// process's queues the next dispatch (profiles/NOTES.md R6.6c).  From 32 MB up FLATGFA_UPLOAD_THREADS threads, the caller's
// among them, move the chunks, which reaches the PCIe rate; below that the caller's thread alone.  Kinds other than
// host -> device and device -> host are a plain hipMemcpy.
hipError_t staged_copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t stream);

// One of the staging buffers (kStagingBytes of pinned memory) in *buf, the caller's while it holds the returned lock: for a
// device result that is read straight out of pinned memory.  *buf is null when the buffer could not be made.
constexpr size_t kStagingBytes = (size_t)8 << 20;
std::unique_lock<std::mutex> borrow_staging(char **buf);

// Makes all of the staging buffers and `device`'s events for them, so that the first large copy does not.
hipError_t warm_staging(int device);

}  // namespace fgfa_dev
