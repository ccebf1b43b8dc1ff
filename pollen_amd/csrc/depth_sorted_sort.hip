// The sort of the sorted record image (depth_sorted.hip): rocprim's device merge sort over (64-bit key, 32-bit record) pairs.
// A translation unit of its own: the header is large and nothing else of the project needs it.  Not the radix sort: its
// one-sweep kernel for this box keeps 80 bytes of scratch memory per lane, for which the runtime sets aside some 40 MB of device
// memory per process from the first launch on -- more than the image of a small graph, and never given back.  The merge sort's
// kernels use none; the image is sorted once per set of plans, so its few milliseconds more do not show in any call.
#include <hip/hip_runtime.h>

#include <cstring>

#include <rocprim/device/device_merge_sort.hpp>

#include "depth_sorted.hpp"

namespace fgfa_dev {

// scratch == nullptr: *scratch_bytes is set to what the sort asks for, nothing is enqueued
bool sorted_sort_pairs(void *scratch, size_t *scratch_bytes, const uint64_t *keys_in, uint64_t *keys_out, const uint32_t *recs_in, uint32_t *recs_out, uint32_t n,
                       hipStream_t stream) {
    const hipError_t e = rocprim::merge_sort(scratch, *scratch_bytes, keys_in, keys_out, recs_in, recs_out, (size_t)n, rocprim::less<uint64_t>(), stream);
    if (e != hipSuccess) (void)hipGetLastError();
    return e == hipSuccess;
}

}  // namespace fgfa_dev
