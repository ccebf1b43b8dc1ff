// Interval and window depth over many paths on the device (interval_device.hip), as the C ABI (capi.cpp) drives it.
// DESIGN.md section 14.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace fgfa_dev {

// The graph an interval job reads.  The pools are device memory of the current device; `depth` is the node depth as the
// handle's d_depth holds it.  Path p walks steps[begin[p] .. end[p]): the spans (they may overlap or leave gaps) are HOST
// memory -- the batches are planned from them, and a batch's spans travel with its plan.
struct IntervalGraph {
    const uint32_t *steps = nullptr;
    uint64_t n_steps = 0;
    const uint32_t *begin = nullptr, *end = nullptr;  // u32[n_paths], host memory
    uint32_t n_paths = 0;
    const uint32_t *seg_len = nullptr;  // u32[n_segs]
    const uint32_t *depth = nullptr;    // u32[n_segs]
    uint32_t n_segs = 0;
};

// The intervals, in device memory: interval k is [start[k], end[k]) on path path_id[k].  A group is a maximal run of equal
// path ids: one interval_depth call of the reference (window_depth.rs:116-147), with a cursor of its own.
struct IntervalList {
    const uint32_t *path_id = nullptr;
    const uint64_t *start = nullptr, *end = nullptr;
    uint64_t n = 0;
};

// What a job holds of step end positions at a time (8 bytes each): the groups are cut into batches whose paths' steps fit.
// One path longer than this is a batch of its own.
constexpr uint64_t kIntervalScratchSteps = (uint64_t)1 << 27;
// Intervals of up to this many steps are summed by one lane each, longer ones by one wave each.
constexpr uint32_t kIntervalLaneCut = 8;

struct IntervalJob;
// (the two parameters are for the tests and the measurement: they change which launches run, never a result)
IntervalJob *interval_new(uint64_t scratch_steps = kIntervalScratchSteps, uint32_t lane_cut = kIntervalLaneCut);
void interval_free(IntervalJob *j);
// out[k] (device memory, f64[iv.n]) = what the reference's interval_depth gives interval k within its group.  host_path_id is
// iv.path_id in host memory, for the plan.  Enqueues on `stream`; waits for every batch's plan to arrive and, at the end, for
// the flag word.  A path id >= n_paths, a span outside the steps or a step naming a segment >= n_segs: FLATGFA_ERR_BOUNDS.
int interval_depth(IntervalJob *j, const IntervalGraph &g, const IntervalList &iv, const uint32_t *host_path_id, hipStream_t stream,
                   double *out);
// how many batches the last call ran
uint64_t interval_batches(const IntervalJob *j);

}  // namespace fgfa_dev
