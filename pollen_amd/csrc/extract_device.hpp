// Extract and position on the device (extract_device.hip), as the C ABI (capi.cpp) drives them.  DESIGN.md section 12.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <vector>

namespace fgfa_dev {

// The graph an extract reads, all in device memory of the current device.  The paths' steps lie one behind another:
// path p walks steps[pstart[p] .. pstart[p + 1]).
struct ExtractGraph {
    const uint32_t *steps = nullptr;
    uint64_t n_steps = 0;
    const uint32_t *pstart = nullptr;  // u32[n_paths + 1]
    uint32_t n_paths = 0;
    const uint32_t *seg_seq = nullptr;  // u32[2 * n_segs]: Segment.seq.start, Segment::len()
    uint32_t n_segs = 0;
    const uint32_t *links = nullptr;  // the Link records (16 bytes each: from, to, overlap)
    uint64_t n_links = 0;
    uint64_t n_align = 0;  // the length of the alignment pool the links' overlap spans point into
};

// One record per subpath (extract.rs:56-61, 102-134), as the step pass writes it.
struct SubpathRec {
    uint64_t path, start, end, step_begin, step_end;
};

struct ExtractTotals {
    uint64_t steps = 0, paths = 0, links = 0, ops = 0;
};

struct ExtractOut {
    uint32_t *steps = nullptr;   // u32[totals.steps]
    SubpathRec *recs = nullptr;  // [totals.paths]
    uint32_t *links = nullptr;   // Link records [totals.links]
    uint32_t *align = nullptr;   // u32[totals.ops], gathered from `align_src` (the old alignment pool, device memory)
    const uint32_t *align_src = nullptr;
};

// Every call enqueues on the job's stream and returns a FLATGFA_* code (flatgfa_last_error).  Those that hand something to the
// host wait for it; nothing else synchronizes.
struct ExtractJob;
ExtractJob *extract_new();
void extract_free(ExtractJob *j);
// Scratch for the graph; the links are checked (a segment id out of range: FLATGFA_ERR_BOUNDS).
int extract_begin(ExtractJob *j, const ExtractGraph &g, hipStream_t stream);
// extract.rs:159-178.  `order` receives the old ids of the neighbourhood in new-id order (the origin first).
int extract_bfs(ExtractJob *j, uint32_t origin, uint64_t dist, std::vector<uint32_t> *order);
// Base position of every step in its path; a step naming a segment out of range: FLATGFA_ERR_BOUNDS.
int extract_positions(ExtractJob *j);
// plen[p] = how many of path p's steps start at a position <= max_dist (the prefix merge_subpaths can act on).
int extract_prefix_lens(ExtractJob *j, uint64_t max_dist, uint32_t *plen);
// merge_subpaths (extract.rs:65-98) for every path in order, the sweep repeated `iterations` times (:181-185), on the host: path p
// walks steps[pbegin[p] .. pbegin[p] + plen[p]), its prefix of steps that start at or before max_distance_subpaths -- a fill
// happens only on re-entry at such a step.  `order` holds the map (old ids in new-id order) and receives the filled segments.
// Every step must name a segment below n_segs.  A sweep that adds nothing ends the sweeps: so would every later one.
inline void extract_merge_host(const uint32_t *steps, const uint32_t *pbegin, const uint32_t *plen, size_t n_paths, size_t n_segs,
                               uint64_t iterations, std::vector<uint32_t> *order) {
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    std::vector<uint32_t> map(n_segs, kNone);
    for (size_t k = 0; k < order->size(); ++k) map[(*order)[k]] = (uint32_t)k;
    for (uint64_t it = 0; it < iterations; ++it) {
        const size_t before = order->size();
        for (size_t p = 0; p < n_paths; ++p) {
            const uint32_t *s = steps + pbegin[p];
            bool open = true, ignore = true;  // cur_subpath_start = Some(0), ignore_path = true
            size_t start = 0;
            for (size_t idx = 0, n = plen[p]; idx < n; ++idx) {
                const bool in = map[s[idx] >> 1] != kNone;
                if (open && in) {
                    if (!ignore)
                        for (size_t k = start; k < idx; ++k) {
                            const uint32_t sg = s[k] >> 1;
                            if (map[sg] == kNone) {
                                map[sg] = (uint32_t)order->size();
                                order->push_back(sg);
                            }
                        }
                    open = false;
                    ignore = false;
                } else if (!open && !in) {
                    open = true;
                    start = idx;
                }
            }
        }
        if (order->size() == before) break;
    }
}
// Segments segs[0 .. n) join the map with new ids base, base + 1, ...
int extract_add(ExtractJob *j, const uint32_t *segs, uint64_t n, uint64_t base);
// The sizes of what fill() writes.  A link whose overlap leaves the alignment pool: FLATGFA_ERR_BOUNDS.
int extract_count(ExtractJob *j, ExtractTotals *t);
int extract_fill(ExtractJob *j, const ExtractOut &out);

// dst[dst_off[k] + x] = src[src_start[k] + x] for the n items laid out by dst_off (ascending; item k ends where k + 1 starts,
// the last at total), every workgroup writing one tile of the output.  All pointers are device memory.
int gather_bytes(const uint8_t *src, uint64_t src_len, const uint32_t *src_start, const uint32_t *dst_off, uint64_t n, uint64_t total,
                 uint8_t *dst, hipStream_t stream);
int gather_u32(const uint32_t *src, uint64_t src_len, const uint32_t *src_start, const uint32_t *dst_off, uint64_t n, uint64_t total,
               uint32_t *dst, hipStream_t stream);

// ops/position.rs over steps[0 .. n) (device memory): *index = the first step with offset < its end position, n when none.
int position_find(const uint32_t *steps, uint64_t n, const uint32_t *seg_seq, uint32_t n_segs, uint64_t offset, hipStream_t stream,
                  uint64_t *index, uint64_t *step_start);

}  // namespace fgfa_dev
