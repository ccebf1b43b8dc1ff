// The sorted record image of a bucketed depth plan (DESIGN.md sections 3.2, 3.3; depth_sorted.hip): the records of the plan's
// items, once per plan, sorted by (window, path, window-relative start) and cut into chunks of kSortedChunk records, each
// with a carry word -- an index for pass 2 (k_accum_sorted), never an answer.  Here: what the host decides about it, as
// functions over plain data -- the sort key and how many bits it takes, where every window's chunks lie, what the build needs
// of the device's memory and when that is refused.  No HIP runtime call and no environment variable in here;
// tests/host_check/sorted_check.cpp runs these functions without a GPU.
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

}  // namespace fgfa_dev
