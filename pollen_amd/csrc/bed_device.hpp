// BED intersection on the device (bed_device.hip): which intervals of one BED file lie under the intervals of another, as
// flatgfa/src/cli/cmds.rs:392-413 and FlatBED::get_intersects (flatbed.rs:37-57) print them -- in the reference's order, but
// not by its double loop over all pairs -- as the C ABI (capi.cpp, and the flatgfa_dev_bed_* entries) drives it.
// DESIGN.md section 21.
//
// The host has parsed both texts, given every name of B a dense id and laid B out grouped by id, file order kept inside a
// group.  On the device:
//   groups      one pass over B: where every group begins, whether it is SORTED (no entry starts before its predecessor in
//               the group; equal starts count as sorted), and runmax_end[i], the running maximum of `end` over the group's
//               entries up to i (a segmented inclusive max-scan on the three-launch scan of device_scan.hpp).
//   candidates  per A entry a range [lo, hi) of its name's group: in a sorted group lo is the first i with
//               runmax_end[i] > a.start and hi the first i with start[i] >= a.end, both by bisection; everything left of lo
//               ends at or before a.start and everything from hi on starts at or after a.end, so no hit is dropped.  An
//               UNSORTED group is walked whole: the result is the same, and the work is that of the reference's double loop
//               restricted to one name.  (No sort by start with a re-ordering of the hits is built.)  The counts hi - lo are
//               scanned into a u64 prefix; their sum is the number of candidates.
//   rounds      the candidates laid one behind another -- A entry after A entry, inside an entry in B's grouped order: the
//               reference's loop order restricted to one name -- are processed kBedRoundCands at a time: the exact test
//               (e > s) counted per tile of kBedCandTile candidates, the counts scanned, the hits compacted in order into
//               records (A entry, B entry, s, e, the line's bytes), the lines' lengths scanned, and the text written by tile
//               of output bytes and delivered piece by piece (text_tiles.hpp).  The scratch of a round is sized by the
//               round, never by the number of candidates or hits.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "flatten_device.hpp"

namespace fgfa_dev {

constexpr int kBedThreads = 256;
// A workgroup of the count and fill kernels owns this many consecutive candidates, kBedThreads at a step.
constexpr uint32_t kBedCandTile = 1024;
// The three-launch scans (device_scan.hpp): kBedThreads * kBedScanPer elements a tile.
constexpr uint32_t kBedScanPer = 4;
// The candidates of one round: what the round's scratch (36 bytes a candidate) is sized by.
constexpr uint64_t kBedRoundCands = (uint64_t)1 << 22;
// The id of an A entry whose name B does not have.
constexpr uint32_t kBedNone = 0xFFFFFFFFu;

static_assert(kBedCandTile % kBedThreads == 0, "a tile is whole steps of the workgroup");

// One side, all device memory: entry i has name id[i] and the interval [start[i], end[i]).
struct BedSide {
    const uint32_t *id = nullptr;
    const uint64_t *start = nullptr, *end = nullptr;
    uint64_t n = 0;  // below 2^32 - 1
};

// What the intersection reads.  A's ids are below n_groups or kBedNone; B's ids are below n_groups and never decrease (B is
// grouped); bed_begin refuses anything else with FLATGFA_ERR_BOUNDS.  names / gname are for the text only: group g's name is
// names[gname[2 g], gname[2 g] + gname[2 g + 1]).
struct BedInput {
    BedSide a, b;
    uint32_t n_groups = 0;
    const uint8_t *names = nullptr;
    const uint32_t *gname = nullptr;  // u32[2 * n_groups], or null: records only
};

// The hits of one round, caller's or the job's device memory, room for the round's candidates each; len may be null.
struct BedHits {
    uint32_t *a = nullptr, *b = nullptr;  // the A entry; the B entry in grouped order
    uint64_t *s = nullptr, *e = nullptr;  // max of the starts, min of the ends
    uint32_t *len = nullptr;              // name_len + digits10(s) + digits10(e) + 3 (needs gname)
};

struct BedTotals {
    uint64_t lines = 0, bytes = 0, candidates = 0, unsorted_groups = 0;
};

struct BedJob;
// (round_cands is for the tests and the measurement: it changes where the rounds are cut, never a byte of the text)
BedJob *bed_new(uint64_t round_cands = kBedRoundCands);
void bed_free(BedJob *j);

// Groups and candidate ranges; waits for `stream` once.  in's arrays stay as they are until the job is freed.
int bed_begin(BedJob *j, const BedInput &in, hipStream_t stream, uint64_t *candidates, uint64_t *unsorted_groups);
uint64_t bed_rounds(const BedJob *j);
// The hit records of round r (below bed_rounds) into `out`; waits for the stream, for *n_hits.
int bed_round(BedJob *j, uint64_t r, const BedHits &out, uint64_t *n_hits);
// Every round without the text: the totals.
int bed_count(BedJob *j, BedTotals *t);
// Every round with its text, to the sink in order, each piece copied out while the next is formed.  A sink that returns
// nonzero: FLATGFA_ERR_IO, nothing more delivered.  With no hit the sink is never called.
int bed_emit(BedJob *j, FlatSink sink, void *ctx, BedTotals *t);

}  // namespace fgfa_dev
