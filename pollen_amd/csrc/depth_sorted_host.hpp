// The sorted record image of a bucketed depth plan (DESIGN.md sections 3.2, 3.3; depth_sorted.hip): the records of the plan's
// items, once per plan, sorted by (window, path, window-relative start) and cut into chunks of kSortedChunk records, each
// with a carry word -- an index for pass 2 (k_accum_sorted), never an answer.  Here: what the host decides about it, as
// functions over plain data -- the sort key and how many bits it takes, where every window's chunks lie, what the build needs
// of the device's memory and when that is refused.  No HIP runtime call and no environment variable in here;
// tests/host_check/sorted_check.cpp runs these functions without a GPU.  At the end: the sweep's arithmetic per lane, one text for
// k_accum_sorted and for tests/host_check/sorted_group_check.cpp, and the packed cells it adds into with unique depth -- the
// pack values, the unpack, and the rule under which a plan may use them (tests/host_check/packed_cells_check.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define FGFA_SORTED_HD __host__ __device__
#else
#define FGFA_SORTED_HD
#endif

namespace fgfa_dev {

constexpr uint32_t kSortedK = 1;                    // records a lane holds per chunk (fixed at build time)
constexpr uint32_t kSortedChunk = 64u * kSortedK;   // records per chunk
// A record of the image: today's low 23 bits -- window-relative start | (length - 1) << wb -- and
constexpr uint32_t kSortedFirst = 1u << 23;         // ... the first record of its path in its window
constexpr uint32_t kSortedPad = 1u << 31;           // ... a record that counts nothing (a window is padded to whole chunks)
constexpr uint32_t kSortedEndBits = 14;             // a record's end is at most 8192: the sweep's scan keeps it below its path's ordinal
constexpr uint32_t kSortedOrdShift = 24;            // ... bits 24..30: how many of the chunk's records up to this one are the first of their path (0..64; 0: the path was under way when the chunk began)
constexpr uint32_t kSortedOrdMask = 0x7Fu;
constexpr uint32_t kSortedGroup = 4;                // consecutive chunks of a window the sweep takes in one step: a lane holds four consecutive records
constexpr uint32_t kSortedQShift = kSortedEndBits + 7;  // the sweep's key: chunk within the group | ordinal | end, from the top
static_assert(kSortedOrdShift + 7 == 31 && kSortedQShift + 2 <= 24, "the ordinal lies between the first-of-path flag and the padding flag; the key fits a word");

inline uint32_t bits_for(uint64_t n_values) {  // bits that hold 0 .. n_values - 1
    uint32_t b = 0;
    while (b < 64 && (n_values - 1) >> b && n_values > 1) ++b;
    return b;
}

// key = window | path id | window-relative start, from the top: a plain ascending sort then groups a window's records by path and
// orders a path's by start, which is all the sweep asks of the order.  One definition for the host's checks and the kernels
// (sorted_image_emit packs with it, sorted_image_finalise takes window and path out with it).
struct SortedKey {
    uint32_t wb = 0, path_bits = 0, win_bits = 0;
    FGFA_SORTED_HD uint32_t bits() const { return wb + path_bits + win_bits; }  // the bits in use: an image whose key would not fit 64 is refused ("size")
    FGFA_SORTED_HD uint64_t pack(uint32_t win, uint32_t path, uint32_t rel) const { return ((((uint64_t)win << path_bits) | path) << wb) | rel; }
    FGFA_SORTED_HD uint32_t path(uint64_t key) const { return (uint32_t)((key >> wb) & ((1ull << path_bits) - 1ull)); }
    FGFA_SORTED_HD uint32_t win(uint64_t key) const { return (uint32_t)(key >> (wb + path_bits)); }
    FGFA_SORTED_HD uint32_t rel(uint64_t key) const { return (uint32_t)(key & ((1ull << wb) - 1ull)); }
};
inline SortedKey sorted_key(uint32_t wb, uint32_t n_paths, uint32_t n_win) {
    SortedKey k;
    k.wb = wb;
    k.path_bits = std::max(1u, bits_for(n_paths));
    k.win_bits = std::max(1u, bits_for(n_win));
    return k;
}

// Where every window's records lie in the sorted pairs, and its chunks in the image.
struct SortedLayout {
    std::vector<uint32_t> rec_off;    // [n_win + 1] a window's records in the sorted pairs
    std::vector<uint32_t> win_chunk;  // [n_win + 1] a window's chunks in the image
    uint64_t n_records = 0, n_chunks = 0;
    bool fits = true;                 // ... in the 32 bits the kernels count records and chunks in
};
inline SortedLayout sorted_layout(const uint32_t *win_count, uint32_t n_win) {
    SortedLayout l;
    l.rec_off.resize((size_t)n_win + 1);
    l.win_chunk.resize((size_t)n_win + 1);
    for (uint32_t w = 0; w < n_win; ++w) {
        l.rec_off[w] = (uint32_t)l.n_records;
        l.win_chunk[w] = (uint32_t)l.n_chunks;
        l.n_records += win_count[w];
        l.n_chunks += ((uint64_t)win_count[w] + kSortedChunk - 1) / kSortedChunk;
        if (l.n_records >= (1ull << 31) || l.n_chunks * kSortedChunk >= (1ull << 31)) l.fits = false;
    }
    l.rec_off[n_win] = (uint32_t)l.n_records;
    l.win_chunk[n_win] = (uint32_t)l.n_chunks;
    return l;
}

// Device memory: what the plan keeps (4 bytes a record slot, 4 a chunk, the windows' table) and what the build needs beside it
// until it is done (the pairs in and out of the sort, the sort's own scratch, the windows' offsets).
inline uint64_t sorted_kept_bytes(uint64_t n_chunks, uint32_t n_win) { return n_chunks * kSortedChunk * 4 + n_chunks * 4 + ((uint64_t)n_win + 1) * 4; }
inline uint64_t sorted_transient_bytes(uint64_t n_records, uint32_t n_win, uint64_t sort_scratch) {
    return n_records * (8 + 4) * 2 + sort_scratch + ((uint64_t)n_win + 1) * 4 + 16;
}
// The refusal rule: the build must leave `reserve` bytes free while it runs (the hook waives it).
inline bool sorted_memory_refused(uint64_t transient, uint64_t kept, uint64_t free_bytes, uint64_t reserve, bool waived) {
    return !waived && transient + kept + reserve > free_bytes;
}

// Which plans get the image (beside the rule of the run image, which they passed): nullptr, or the reason pass 2 keeps its walk.
inline const char *sorted_refused(int hook, uint32_t acc_parts, uint32_t n_groups, uint32_t n_more, uint32_t wb, bool keeps_records) {
    if (hook == 0) return "hook";
    if (!keeps_records) return "rewritten";
    if (acc_parts != 1) return "parts";
    if (n_groups > 1 || n_more) return "ranges";
    if (wb < 11 || wb > 13) return "windows";
    return nullptr;
}

// ---- the sweep's arithmetic per lane (k_accum_sorted; tests/host_check/sorted_group_check.cpp runs the same text) ----
// A step of the sweep takes a group of kSortedGroup consecutive chunks of a window; lane L holds records 4L .. 4L+3 of the
// group, all of chunk q = L >> 4.  A record's key x = q | its ordinal in its chunk | its end, from the top, never falls along
// the group's records of one path and rises from path to path and chunk to chunk; so with p the largest key among the records
// before it -- and the chunk's seed, its carry word as a record of ordinal 0 before the chunk's first -- a record revisits cells
// exactly if p >= x - len (the same chunk, the same path, an earlier end beyond its start), and the stretch ends at the smaller
// of the two ends.  CHECKED: the build for the one group of a window that may hold padding (key 0: it counts nothing).
FGFA_SORTED_HD inline uint32_t sorted_umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
FGFA_SORTED_HD inline uint32_t sorted_umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
FGFA_SORTED_HD inline uint32_t sorted_seed(uint32_t q, uint32_t carry) { return (q << kSortedQShift) | carry; }

struct SortedLane {
    uint32_t s[kSortedGroup], len[kSortedGroup], x[kSortedGroup];  // start, length - 1, key (0: padding)
    uint32_t t;                                                      // the largest of the lane's keys and its chunk's seed
};
template <bool CHECKED>
FGFA_SORTED_HD inline void sorted_lane_keys(const uint32_t (&rec)[kSortedGroup], uint32_t q, uint32_t wb, uint32_t seed, SortedLane &ln) {
    ln.t = seed;  // (at every lane of the chunk: the seed stands before all of them, and a maximum takes it twice as once)
    for (uint32_t k = 0; k < kSortedGroup; ++k) {
        ln.s[k] = rec[k] & ((1u << wb) - 1u);
        ln.len[k] = (rec[k] >> wb) & 1023u;
        const uint32_t x = ((rec[k] >> (kSortedOrdShift - kSortedEndBits)) & (kSortedOrdMask << kSortedEndBits)) | ((q << kSortedQShift) + ln.s[k] + ln.len[k] + 1u);
        ln.x[k] = CHECKED && (rec[k] & kSortedPad) ? 0u : x;
        ln.t = sorted_umax(ln.t, ln.x[k]);
    }
}
// One record against p, the largest key before it (the lane's first starts from the larger of the wave's exclusive prefix
// maximum of t and the seed): whether it revisits cells, and where that stretch [s, end) ends; p takes the record in.
template <bool CHECKED>
FGFA_SORTED_HD inline bool sorted_record_step(uint32_t &p, uint32_t x, uint32_t len, uint32_t &end) {
    const bool hit = (!CHECKED || x != 0u) && p >= x - len;
    end = sorted_umin(x, p) & ((1u << kSortedEndBits) - 1u);
    p = sorted_umax(p, x);
    return hit;
}

// ---- packed cells (k_accum_sorted<true, ...>; tests/host_check/packed_cells_check.cpp runs the same text) ----
// With unique depth a record adds to the difference arrays of depth and of revisits, and a revisiting record adds to the SAME
// cell s of both.  So one array W: a cell holds dD + 65536 dR mod 2^32, depth's difference in the low half and the revisits'
// in the high half; a record is two adds, and a third only where its revisits end before it does.  Unpacking is exact while
// both halves stay inside 16 signed bits, and they do under the rule below: |dD[c]| <= max(starts(c), ends(c)), counting the
// window's records that start or end at cell c; and |dR[c]| <= max(starts(c), 2 ends(c)), because a revisit's end is the
// record's own end or an earlier end M of its path, and a path cuts at one value of M once -- the record that does raises M
// beyond it -- so the cuts at c are no more than the paths with a record ending at c.
constexpr uint32_t kSortedPackRevisit = 1u << 16;  // one revisit, in a cell
constexpr uint32_t kSortedPackLimit = 1u << 14;    // the rule: fewer starts and fewer ends than this at every cell of every window
FGFA_SORTED_HD inline uint32_t sorted_pack(int32_t dD, int32_t dR) { return (uint32_t)dD + ((uint32_t)dR << 16); }
FGFA_SORTED_HD inline void sorted_unpack(uint32_t w, int32_t &dD, int32_t &dR) {
    dD = (int32_t)(int16_t)(uint16_t)(w & 0xFFFFu);
    dR = (int32_t)(int16_t)(uint16_t)((w - (uint32_t)dD) >> 16);  // (a negative low half borrowed from the high one)
}
FGFA_SORTED_HD inline uint32_t sorted_pack_start(bool hit) { return 1u + (hit ? kSortedPackRevisit : 0u); }         // what W[s] takes
FGFA_SORTED_HD inline uint32_t sorted_pack_end(bool hit_to_e) { return 1u + (hit_to_e ? kSortedPackRevisit : 0u); }  // what W[e] gives: the revisits end with the record
// One record of a lane, as sorted_record_step sees it, into the cells: add(cell, value) adds mod 2^32.
template <bool CHECKED, class Add>
FGFA_SORTED_HD inline void sorted_record_packed(uint32_t &p, uint32_t s, uint32_t len, uint32_t x, Add add) {
    uint32_t end;
    const bool hit = sorted_record_step<CHECKED>(p, x, len, end);
    if (CHECKED && x == 0u) return;  // padding
    const uint32_t e = s + len + 1u;  // (e <= window size; that cell is a sink)
    add(s, sorted_pack_start(hit));
    add(e, 0u - sorted_pack_end(hit && end == e));
    if (hit && end != e) add(end, 0u - kSortedPackRevisit);
}
// The rule, from the largest number of records that start at one cell of one window and that end at one (sorted_image_cell_max:
// a histogram maximum of the image, an index and not an answer).  No maximum (an image nobody measured): not known.
inline bool sorted_cells_fit(uint32_t max_starts, uint32_t max_ends) { return max_starts != 0u && max_starts < kSortedPackLimit && max_ends < kSortedPackLimit; }
// What FastPlan::sorted_cells says; 0 is "not known", which sweeps wide cells.
constexpr uint32_t kSortedCellsUnknown = 0, kSortedCellsPacked = 1, kSortedCellsWideRule = 2, kSortedCellsWideHook = 3;
// (hook: FLATGFA_SORTED_CELLS as it was when the image was installed -- 0: wide, 1: packed, which never overrides the rule; -1: unset)
inline uint32_t sorted_cells_choice(int hook, uint32_t max_starts, uint32_t max_ends) {
    if (max_starts == 0u) return kSortedCellsUnknown;
    if (!sorted_cells_fit(max_starts, max_ends)) return kSortedCellsWideRule;
    return hook == 0 ? kSortedCellsWideHook : kSortedCellsPacked;
}
inline const char *sorted_cells_name(uint32_t cells) {
    return cells == kSortedCellsPacked ? "packed" : cells == kSortedCellsWideRule ? "wide(rule)" : cells == kSortedCellsWideHook ? "wide(hook)" : "wide(unknown)";
}

}  // namespace fgfa_dev
