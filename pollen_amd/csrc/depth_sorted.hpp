// The one function depth_sorted.hip takes from depth_sorted_sort.hip (which alone includes rocprim's merge sort).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace fgfa_dev {

// Sorts n (key, record) pairs by their keys, ascending and stable, on `stream`.
// scratch == nullptr: *scratch_bytes is set to what the sort asks for and nothing is enqueued.
bool sorted_sort_pairs(void *scratch, size_t *scratch_bytes, const uint64_t *keys_in, uint64_t *keys_out, const uint32_t *recs_in, uint32_t *recs_out, uint32_t n,
                       hipStream_t stream);

}  // namespace fgfa_dev
