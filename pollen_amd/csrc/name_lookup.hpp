// NameMap::get (namemap.rs:27-33) on the device, over the table NameMap::export_sorted leaves (GafNameTable): the one lookup
// of the GAF scan, the GAF lookup and the GFA parser.  HIP only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace fgfa_dev {

// Names up to seq_max are id = name - 1 (name 0 wraps to u32::MAX); the others are found in `keys` (sorted, `ids` beside
// them) by bisection.  0xFFFFFFFF: the map does not have the name.
__device__ __forceinline__ uint32_t name_map_get(uint64_t num, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ ids,
                                                 uint32_t n_others, uint64_t seq_max) {
    if (num <= seq_max) return (uint32_t)(num - 1);
    uint32_t lo = 0, hi = n_others;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] < num) lo = mid + 1;
        else hi = mid;
    }
    return lo < n_others && keys[lo] == num ? ids[lo] : 0xFFFFFFFFu;
}

}  // namespace fgfa_dev
