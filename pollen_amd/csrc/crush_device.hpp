// Crush on the device (crush_device.hip): every run of N inside a segment's sequence becomes one N
// (slow_odgi/slow_odgi/crush.py), as the C ABI (capi.cpp, and the flatgfa_dev_crush_* entries) drives it.  DESIGN.md section 17.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace fgfa_dev {

// The bases are walked in the coordinates of the segments laid end to end (flatten's legend), a tile of kCrushTile bytes at a
// time by one workgroup of kCrushThreads lanes; the tiles are dealt to at most kCrushGrid workgroups in equal contiguous
// ranges, so that neither the grid nor the scratch depends on a total the host does not know yet.
constexpr int kCrushThreads = 256;
constexpr uint32_t kCrushTile = 16384;
constexpr uint32_t kCrushGrid = 2048;
// The three-launch scans (device_scan.hpp) of the old lengths, the new lengths and the ranges' kept counts.
constexpr uint32_t kCrushScanPer = 4;

// What a crush reads, all device memory of the current device: Segment.seq.start and Segment::len() per segment (two words
// each, as the GAF lookup keeps them) and seq_data.  The spans may be out of order, overlap, alias or be empty.
struct CrushIn {
    const uint32_t *seg_seq = nullptr;  // u32[2 * n_segs]
    const uint8_t *seq_data = nullptr;
    uint64_t seq_len = 0;
    uint32_t n_segs = 0;
};

// One crush.  count() checks the spans, lays the segments end to end, counts what every range of tiles keeps and what every
// segment drops, waits for the totals (its one host synchronization) and checks them; only then does it enqueue the write of
// seg_len_out (u32[n_segs]: the new lengths).  fill() enqueues the new pool -- the crushed segments one behind another in
// segment order -- into seq_out (u8[*bytes_out], at any alignment) and the new spans into seg_seq_out (u32[2 * n_segs]:
// start, length; a segment's start is the sum of the new lengths before it, whether it is empty or not); it does not wait.
// Both return FLATGFA_* codes (flatgfa_last_error).
struct CrushJob;
CrushJob *crush_new();
void crush_free(CrushJob *j);
int crush_count(CrushJob *j, const CrushIn &in, uint32_t *seg_len_out, hipStream_t stream, uint64_t *bytes_out, uint64_t *dropped_out);
int crush_fill(CrushJob *j, uint8_t *seq_out, uint32_t *seg_seq_out, hipStream_t stream);

}  // namespace fgfa_dev
