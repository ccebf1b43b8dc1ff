// The GAF scan of gaf_device.hip, as the C ABI (capi.cpp) drives it.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace fgfa_dev {

// A graph's NameMap on the device (namemap.rs): names up to `seq_max` are id = name - 1, the others are found in `keys`
// (sorted; `ids` beside them).
struct GafNameTable {
    const uint64_t *keys = nullptr;
    const uint32_t *ids = nullptr;
    uint32_t n_others = 0;
    uint32_t n_segs = 0;
    uint64_t seq_max = 0;
};

// u64 words of scratch a scan of `len` bytes at `d_text` takes (one summary per tile, and one more word).
size_t gaf_scratch_words(const void *d_text, size_t len);

// Enqueues on `stream`: the segments named by the counted lines of the whole lines in d_text[0, len) are OR-ed into d_row
// (bit s & 63 of word s >> 6); a name the graph does not have lowers *d_first_bad to base + the offset of its line.
hipError_t gaf_scan(const uint8_t *d_text, size_t len, const GafNameTable &names, uint64_t *d_row, uint64_t *d_first_bad,
                    uint64_t base, uint64_t *scratch, hipStream_t stream);

}  // namespace fgfa_dev
