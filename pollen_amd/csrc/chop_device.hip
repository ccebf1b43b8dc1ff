// Chop on gfx950 (flatgfa/src/ops/chop.rs).
//
// A segment of length len becomes k = pieces(len) = (len <= c ? 1 : ceil(len / c)) new segments, numbered in segment order
// from seg_first[s] (an exclusive scan of the piece counts).  A step of s becomes k steps, and the new steps pool is the
// concatenation of the paths' expansions.  Everything is a scan and a variable-length expansion: the kernels, and the driver
// that launches them (the Expansion: count, read the totals, check them against the u32 id space, and only then write), are
// in expand_kernels.hpp, which inject shares.  What is chop's own is below: where a segment's piece count comes from (its
// length and c) and how long a piece is.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/flatgfa.h"
#include "chop_device.hpp"
#include "device_common.hpp"
#include "device_scan.hpp"
#include "expand_kernels.hpp"
#include "prof.hpp"

namespace fgfa_dev {
namespace {

__device__ __forceinline__ uint64_t pieces(uint32_t len, uint64_t c) { return len <= c ? 1u : ((uint64_t)len - 1) / c + 1; }

struct ChopPieces {
    const uint32_t *len;
    uint64_t c;
    __device__ uint64_t operator()(uint32_t s) const { return pieces(len[s], c); }
};

struct SegLoad {
    const uint32_t *len, *seq_start;
    uint64_t c;
    __device__ void operator()(uint64_t i, uint32_t *cnt, uint32_t *a, uint32_t *b) const {
        const uint32_t L = len[i];
        *cnt = (uint32_t)pieces(L, c);
        *a = L;
        *b = seq_start ? seq_start[i] : 0u;
    }
};
struct SegEmit {  // new segment jj is piece p of k of old segment i (length a, sequence from b)
    uint64_t c;
    uint32_t *recs, *links;
    __device__ uint32_t operator()(uint64_t jj, uint64_t i, uint32_t a, uint32_t b, uint32_t p, uint32_t k) const {
        const uint64_t plen = p + 1 < k ? c : (uint64_t)a - (uint64_t)(k - 1) * c;
        write_piece(recs, links, jj, i, (uint32_t)((uint64_t)b + (uint64_t)p * c), plen, p, k);
        return (uint32_t)plen;
    }
};

constexpr ExpandNames kChop{"chop: ", "chopped graph", "k_chop_reduce_segs", "k_chop_reduce_steps", "k_chop_reduce_paths",
                            "k_chop_expand_steps", "k_chop_expand_paths", "k_chop_expand_segs"};

}  // namespace

struct ChopJob {
    Expansion x;
    uint64_t c = 0;
};

ChopJob *chop_new() { return new ChopJob(); }
void chop_free(ChopJob *j) { delete j; }

int chop_count(ChopJob *j, const ChopIn &in, uint64_t c, bool links, uint32_t *seg_first, hipStream_t st, uint64_t *n_new_segs,
               uint64_t *n_new_steps, uint64_t *n_new_links) {
    if (c == 0) return expand_refuse(kChop, "the maximum segment size must be at least 1", FLATGFA_ERR_ARG);
    Expansion &x = j->x;
    if (int rc = expand_check_args(kChop, in, links, seg_first, false)) return rc;
    if (int rc = expand_begin(x, kChop, in, links, seg_first, st)) return rc;
    j->c = c;
    if (int rc = expand_check_graph(x, kChop, st)) return rc;
    const ChopPieces pc{in.seg_len, c};
    expand_reduce(x, kChop, pc, st);
    return expand_totals(x, kChop, pc, st, n_new_segs, n_new_steps, n_new_links);
}

int chop_fill(ChopJob *j, const ChopOut &out, hipStream_t st) {
    Expansion &x = j->x;
    return expand_fill(x, kChop, SegLoad{x.in.seg_len, x.in.seq_start, j->c}, SegEmit{j->c, out.seg_recs, x.links ? out.links : nullptr}, out, 0, st);
}

}  // namespace fgfa_dev

// ---- the device-level C ABI (include/flatgfa.h Part 3) ----
struct flatgfa_dev_chop : fgfa_dev::ChopJob {};

extern "C" {

int flatgfa_dev_chop_count(const flatgfa_dev_graph_t *g, uint64_t max_size, uint32_t *seg_first, void *stream, flatgfa_dev_chop_t **job,
                           uint64_t *n_segs_out, uint64_t *n_steps_out) {
    if (job) *job = nullptr;
    if (!g || !job || !n_segs_out || !n_steps_out) { fgfa_dev::set_error("flatgfa_dev_chop_count: NULL argument"); return FLATGFA_ERR_ARG; }
    if (!g->seg_len) { fgfa_dev::set_error("flatgfa_dev_chop_count: the graph has no seg_len"); return FLATGFA_ERR_ARG; }
    auto *h = new flatgfa_dev_chop();
    const int rc = fgfa_dev::chop_count(h, fgfa_dev::chop_in_of(*g), max_size, false, seg_first, (hipStream_t)stream, n_segs_out, n_steps_out, nullptr);
    if (rc) {
        delete h;
        return rc;
    }
    *job = h;
    return FLATGFA_OK;
}

int flatgfa_dev_chop_fill(flatgfa_dev_chop_t *job, uint32_t *steps, uint32_t *path_begin, uint32_t *path_end, uint32_t *seg_len, void *stream) {
    if (!job) { fgfa_dev::set_error("flatgfa_dev_chop_fill: NULL job"); return FLATGFA_ERR_ARG; }
    return fgfa_dev::chop_fill(job, fgfa_dev::chop_out_of(steps, path_begin, path_end, seg_len), (hipStream_t)stream);
}

void flatgfa_dev_chop_free(flatgfa_dev_chop_t *job) { delete job; }

}  // extern "C"
