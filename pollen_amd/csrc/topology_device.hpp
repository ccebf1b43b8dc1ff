// Validate and degree on the device (topology_device.hip), as the C ABI (capi.cpp) drives them.  DESIGN.md section 13.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "../../include/flatgfa.h"

namespace fgfa_dev {

// The link index of one graph, all in device memory of one device: the links as the set of their canonical keys
// (min of (from << 32 | to) and (flip(to) << 32 | flip(from))), in CSR over the 2 * n_segs handles -- row h holds the low
// halves of the keys whose high half is h, to[row[h] .. row[h + 1]).  Rows longer than the linear-probe threshold are sorted.
struct TopoIndex {
    void *mem = nullptr;      // the one allocation behind the three arrays
    uint32_t *row = nullptr;  // u32[2 * n_segs + 1]
    uint32_t *to = nullptr;   // u32[n_links]
    uint32_t *deg = nullptr;  // u32[n_segs]: link ends per segment (degree.py:11-16)
    uint32_t n_segs = 0;
    uint64_t n_links = 0;
};

// The steps a validate reads: path p walks steps[pbegin[p] .. pbegin[p] + (pstart[p + 1] - pstart[p])).  The spans may
// overlap or leave gaps; pstart numbers the steps of all paths one behind another (n_lin of them).
struct TopoSteps {
    const uint32_t *steps = nullptr;
    const uint32_t *pstart = nullptr;  // u32[n_paths + 1]
    const uint32_t *pbegin = nullptr;  // u32[n_paths]
    uint32_t n_paths = 0;
    uint64_t n_lin = 0;
};

// Every call enqueues on `stream` and returns a FLATGFA_* code (flatgfa_last_error).  Those that hand something to the host
// wait for it; nothing else synchronizes.
// `links` are the Link records in device memory.  A link naming a segment >= n_segs: FLATGFA_ERR_BOUNDS, and *out stays empty.
int topo_index_build(const uint32_t *links, uint64_t n_links, uint32_t n_segs, hipStream_t stream, TopoIndex *out);
void topo_index_free(TopoIndex *ix);
// deg widened into out[n_segs] (host memory).
int topo_degree(const TopoIndex &ix, hipStream_t stream, uint64_t *out);

struct ValidateJob;
ValidateJob *validate_new();
void validate_free(ValidateJob *j);
// validate.py:9-24: *n = the consecutive step pairs no link supports.  A step naming a segment >= n_segs: FLATGFA_ERR_BOUNDS.
int validate_count(ValidateJob *j, const TopoIndex &ix, const TopoSteps &sp, hipStream_t stream, uint64_t *n);
// The *n records of the count, in path order then step order, into host memory.
int validate_fill(ValidateJob *j, flatgfa_missing_link_t *out);

}  // namespace fgfa_dev
