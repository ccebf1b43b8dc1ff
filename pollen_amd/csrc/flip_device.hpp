// Flip on the device (flip_device.hip): a path that walks more bases backward than forward is turned around, and the links its
// new steps need are added to the old ones, de-duplicated (slow_odgi/slow_odgi/flip.py), as the C ABI (capi.cpp, and the
// flatgfa_dev_flip_* entries) drives it.  DESIGN.md section 22.
//
// mygfa keys paths by their old name, so of several paths with one name only one survives there; this store keeps every
// path, as the project's other transformers do.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace fgfa_dev {

// The steps are walked in the coordinates of the paths laid one behind another (TopoSteps' numbering), a tile of kFlipTile
// steps at a time by one workgroup of kFlipThreads lanes; the tiles are dealt round robin to at most kFlipGrid workgroups.
constexpr int kFlipThreads = 256;
constexpr uint32_t kFlipPer = 8;
constexpr uint32_t kFlipTile = kFlipThreads * kFlipPer;
constexpr uint32_t kFlipGrid = 2048;
// The three-launch scans (device_scan.hpp) of the candidate counts, the rows and the keep flags.
constexpr uint32_t kFlipScanPer = 4;
// A row of the key table (all keys with one high handle) of up to kFlipShortRow entries is sorted by one wave in registers;
// a longer one by a workgroup, in LDS up to kFlipLdsRow entries and in place beyond.
constexpr uint32_t kFlipShortRow = 64;
constexpr uint32_t kFlipLdsRow = 4096;
// The key table is worked in rounds where its keys -- at most one per old link and per step -- are more than two rounds'
// worth: round r scatters, sorts and decides the rows that begin at key offsets [r, r + 1) * kFlipRoundKeys, in scratch for
// twice as many keys.  (1 GiB; a row of more keys than one round then has no place: FLATGFA_ERR_TOO_LARGE.)
constexpr uint64_t kFlipRoundKeys = (uint64_t)1 << 26;

// What a flip reads, all device memory of the current device.  Path p walks steps[pbegin[p] .. pbegin[p] + n_p) with
// n_p = pstart[p + 1] - pstart[p]; the spans may be out of order, overlap or leave gaps, and pstart numbers the steps of all
// paths one behind another (n_lin of them) -- which is where the output has them.  links are the Link records (four words:
// from, to, overlap.start, overlap.end) and alignment the pool their overlaps point into.
struct FlipIn {
    const uint32_t *steps = nullptr;
    uint64_t n_steps = 0;
    const uint32_t *pstart = nullptr;  // u32[n_paths + 1]
    const uint32_t *pbegin = nullptr;  // u32[n_paths]
    uint32_t n_paths = 0;
    uint64_t n_lin = 0;
    const uint32_t *seg_len = nullptr;  // u32[n_segs]
    uint32_t n_segs = 0;
    const uint32_t *links = nullptr;  // u32[4 * n_links]
    uint64_t n_links = 0;
    const uint32_t *alignment = nullptr;  // u32[n_align]
    uint64_t n_align = 0;
};

// One flip.  count() checks the ids and spans, weighs the paths, forms the candidate links of the turned ones, groups old
// links and candidates by canonical key and decides which are kept, then waits for the totals (its one host
// synchronization).  fill() enqueues the new steps (u32[n_lin], the paths one behind another), the turned flags (u32[n_paths],
// 0 or 1) and the kept Link records (u32[4 * links_out]; a new link's overlap is the span [n_align, n_align + 1): the one 0M
// op the caller appends to its alignment pool when *links_new is not zero); it does not wait.  Both return FLATGFA_* codes
// (flatgfa_last_error).
struct FlipJob;
// (round_keys is for the tests and the measurement: it changes where the rounds are cut, never a link of the answer)
FlipJob *flip_new(uint64_t round_keys = kFlipRoundKeys);
void flip_free(FlipJob *j);
int flip_count(FlipJob *j, const FlipIn &in, hipStream_t stream, uint64_t *n_turned, uint64_t *links_out, uint64_t *links_new);
int flip_fill(FlipJob *j, uint32_t *steps_out, uint32_t *turned_out, uint32_t *links_out, hipStream_t stream);
// the turned flags of a counted job, in device memory (u32[n_paths]; the host route names the paths from them)
const uint32_t *flip_turned(const FlipJob *j);

}  // namespace fgfa_dev
