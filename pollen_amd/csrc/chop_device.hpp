// Chop on the device (chop_device.hip), as the C ABI (capi.cpp, and the flatgfa_dev_chop_* entries) drives it.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace fgfa_dev {

// The graph a chop reads, all in device memory of the current device.  seq_start and links are optional (the host entry
// needs them for the new segment records and links; the device entry does not).
struct ChopIn {
    const uint32_t *steps = nullptr;
    uint64_t n_steps = 0;
    const uint32_t *path_begin = nullptr, *path_end = nullptr;
    uint32_t n_paths = 0;
    uint32_t n_segs = 0;
    const uint32_t *seg_len = nullptr;
    const uint32_t *seq_start = nullptr;  // u32[n_segs]: Segment.seq.start
    const uint32_t *links = nullptr;      // the Link records (16 bytes each: from, to, overlap)
    uint64_t n_links = 0;
};

// What a fill writes (device memory).  Any pointer may be NULL where its array is not wanted.
struct ChopOut {
    uint32_t *steps = nullptr;       // u32[n_new_steps]
    uint32_t *path_begin = nullptr;  // u32[n_paths]
    uint32_t *path_end = nullptr;    // u32[n_paths]
    uint32_t *seg_len = nullptr;     // u32[n_new_segs]
    uint32_t *seg_recs = nullptr;    // Segment records, 24 bytes each: name = id + 1, seq span in the old seq_data, optional (0,0)
    uint32_t *links = nullptr;       // Link records, 16 bytes each: the n_new_segs - n_segs forward links, then the old links remapped
};

// One chop: count() checks the graph, scans the piece counts, waits for the totals (its one host synchronization), checks
// them and enqueues the write of seg_first; fill() enqueues the rest.  Both return FLATGFA_* codes (flatgfa_last_error).
// The job is an Expansion (expand_kernels.hpp, the driver chop and inject share) and c; chop_free waits for the last stream
// the job was used on, then frees its scratch.
struct ChopJob;
ChopJob *chop_new();
void chop_free(ChopJob *j);
int chop_count(ChopJob *j, const ChopIn &in, uint64_t max_size, bool links, uint32_t *seg_first, hipStream_t stream,
               uint64_t *n_new_segs, uint64_t *n_new_steps, uint64_t *n_new_links);
int chop_fill(ChopJob *j, const ChopOut &out, hipStream_t stream);

}  // namespace fgfa_dev
