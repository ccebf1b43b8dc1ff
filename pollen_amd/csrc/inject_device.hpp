// Inject on the device (inject_device.hip), as the C ABI (capi.cpp, and the flatgfa_dev_inject_* entries)
// drives it.  The graph it reads and the image it writes are chop's (chop_device.hpp).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "chop_device.hpp"

namespace fgfa_dev {

// The BED lines, in device memory: line l is bases [start[l], end[l]) of path path_id[l].
struct InjectLines {
    const uint32_t *path_id = nullptr;
    const uint64_t *start = nullptr, *end = nullptr;
    uint64_t n = 0;
};

// One inject: count() checks the graph and the lines, locates the cuts, builds the cut table, scans the piece counts and the new
// paths' lengths, waits for the totals (its one host synchronization), checks them and enqueues the write of seg_first; fill()
// enqueues the rest.  A fill writes ChopOut with path_begin / path_end of n_paths + n entries: the old paths, then one new
// path per line.  Both return FLATGFA_* codes (flatgfa_last_error).  The job is an Expansion (expand_kernels.hpp, the driver
// chop and inject share) plus the lines, the cut table and the lines' scan; inject_free waits and frees as chop_free does.
struct InjectJob;
InjectJob *inject_new();
void inject_free(InjectJob *j);
int inject_count(InjectJob *j, const ChopIn &in, const InjectLines &lines, bool links, uint32_t *seg_first, hipStream_t stream,
                 uint64_t *n_new_segs, uint64_t *n_new_steps, uint64_t *n_new_links);
int inject_fill(InjectJob *j, const ChopOut &out, hipStream_t stream);

}  // namespace fgfa_dev
