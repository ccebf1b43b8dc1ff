// The GAF lookup of gaf_lookup_device.hip, as the C ABI (capi.cpp, and the flatgfa_dev_gaf_* entries) drives it.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "gaf_device.hpp"

namespace fgfa_dev {

// What a lookup reads of the graph, all in device memory of the current device.
struct GafGraph {
    GafNameTable names;
    const uint32_t *seg_seq = nullptr;  // u32[2 * n_segs]: Segment.seq.start, Segment::len() per segment
    const uint8_t *seq_data = nullptr;
};

// What count() found in one piece of text.  The bad_* words are ~0 when no line is bad, else the lowest `base` + offset of
// a line that is malformed (parse), names a segment the graph lacks (name), or has a range that cannot be sliced (slice).
struct GafTotals {
    uint64_t n_lines = 0, n_events = 0, seq_bytes = 0;
    uint64_t bad_parse = ~0ull, bad_name = ~0ull, bad_slice = ~0ull;
};

// The arrays a counted job holds (device memory, the job's own), valid until the next count() or the job's end.
struct GafArrays {
    const uint64_t *line_end = nullptr;    // [n_lines]: the offset of each line's '\n' in the text
    const uint64_t *name_len = nullptr;    // [n_lines]: the length of field 0 (it starts where the line does)
    const uint64_t *line_first = nullptr;  // [n_lines + 1]: the line's first event
    const uint32_t *handle = nullptr;      // [n_events]: (id << 1) | backward
    const uint8_t *kind = nullptr;         // [n_events]: 0 none, 1 all, 2 partial
    const uint64_t *a = nullptr, *b = nullptr;  // [n_events]: Partial(a, b); 0, len for All; 0, 0 for None
};

// One lookup over d_text[0, len) (whole lines: what follows the last '\n' is ignored): count() indexes the lines, parses them,
// forms every event and -- with `seqs` -- lays the `-s` text out, waiting for `stream` to read the totals; gather() enqueues
// bytes [begin, end) of that text into d_out.  Both return FLATGFA_* codes (flatgfa_last_error).
struct GafLookupJob;
GafLookupJob *gaf_lookup_new();
void gaf_lookup_free(GafLookupJob *j);
int gaf_lookup_count(GafLookupJob *j, const uint8_t *d_text, size_t len, const GafGraph &g, bool seqs, uint64_t base,
                     hipStream_t stream, GafTotals *totals);
const GafArrays &gaf_lookup_arrays(const GafLookupJob *j);
int gaf_lookup_gather(GafLookupJob *j, uint64_t begin, uint64_t end, uint8_t *d_out, hipStream_t stream);
// Work that reads the job's arrays was enqueued on `stream` (any stream): the next count(), and the job's end, wait for it.
int gaf_lookup_used_on(GafLookupJob *j, hipStream_t stream);

}  // namespace fgfa_dev
