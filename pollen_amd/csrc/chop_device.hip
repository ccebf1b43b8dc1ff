// Chop on gfx950 (flatgfa/src/ops/chop.rs).
//
// A segment of length len becomes k = pieces(len) = (len <= c ? 1 : ceil(len / c)) new segments, numbered in segment order
// from seg_first[s] (an exclusive scan of the piece counts).  A step of s becomes k steps, and the new steps pool is the
// concatenation of the paths' expansions.  Everything is a scan and a variable-length expansion:
//
//   k_reduce     one workgroup per 16 tiles of 256 elements: each tile's sum of piece counts (u64), the workgroup's sum; the
//                last workgroup to finish (a ticket) scans the workgroup sums and writes the total.  The host reads the totals
//                -- new segments, new steps -- checks them against the u32 id space, and only then is anything written.
//   k_prefix     each tile's exclusive prefix, from its workgroup's and the tile sums before it in the workgroup.
//   k_offsets    a tile's elements' exclusive prefixes (seg_first; the new path spans when they are laid out per path).
//   k_map        for each output tile of 2048 items, the source tile its first item comes from (a binary search of the prefixes).
//   k_expand     one workgroup per output tile: the source tiles that cover it (at most 10: every element has at least one
//                piece) are scanned again into LDS, each lane finds its first source element by a binary search there and
//                emits 8 consecutive items, and the tile goes out through LDS in coalesced rows.  Every workgroup writes
//                2048 items whatever the lengths: a 5 Mbp segment at c = 1 is 2 442 tiles spread over the whole chip.
//   k_path_spans a wave per path: the new span [O(begin), O(end)) where O(v) = prefix of v's tile + the pieces of the at most
//                255 steps before v in it.
//
// Path spans that do not tile the steps pool in order (the types allow any spans, overlapping ones included) are expanded per
// path instead: k_path_lens sums each path's pieces, k_offsets lays the paths out, k_expand_paths writes each path with one
// workgroup (all its lanes on a long step).  Kernels never trap: a bad span, step or link raises a bit of the flag word.
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

// The kernels listed above are in expand_kernels.hpp, which inject shares; what is chop's own is where a segment's piece
// count comes from (its length and c) and how long a piece is.
__device__ __forceinline__ uint64_t pieces(uint32_t len, uint64_t c) { return len <= c ? 1u : ((uint64_t)len - 1) / c + 1; }

struct ChopPieces {
    const uint32_t *len;
    uint64_t c;
    __device__ uint64_t operator()(uint32_t s) const { return pieces(len[s], c); }
};
using SegCount = SegCountT<ChopPieces>;
using StepCount = StepCountT<ChopPieces>;

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

}  // namespace

struct ChopJob {
    ChopIn in;
    uint64_t c = 0;
    bool links = false, counted = false, tiling = true;
    uint32_t *seg_first = nullptr;
    uint64_t S2 = 0, N2 = 0, L2 = 0;
    uint64_t *mem = nullptr;
    uint32_t *maps = nullptr;
    uint64_t *hdr = nullptr;  // [0] flags, [1] new segments, [2] new steps (tiling), [3] new steps (per path)
    uint64_t *plen = nullptr;
    ScanBuf seg, step, path;
    hipStream_t last = nullptr;
    ~ChopJob() {
        if (last) (void)hipStreamSynchronize(last);
        if (mem) (void)hipFree(mem);
        if (maps) (void)hipFree(maps);
    }
};

ChopJob *chop_new() { return new ChopJob(); }
void chop_free(ChopJob *j) { delete j; }
const ChopIn &chop_input(const ChopJob *j) { return j->in; }

#define CHOP_HIP(expr) FGFA_HIP("chop: ", expr)

int chop_count(ChopJob *j, const ChopIn &in, uint64_t c, bool links, uint32_t *seg_first, hipStream_t st, uint64_t *n_new_segs,
               uint64_t *n_new_steps, uint64_t *n_new_links) {
    if (c == 0) { set_error("chop: the maximum segment size must be at least 1"); return FLATGFA_ERR_ARG; }
    if ((in.n_segs && (!in.seg_len || !seg_first)) || (in.n_steps && !in.steps) || (in.n_paths && (!in.path_begin || !in.path_end)) ||
        (links && in.n_links && !in.links)) {
        set_error("chop: NULL argument");
        return FLATGFA_ERR_ARG;
    }
    if (in.n_steps > 0xFFFFFFFFull || in.n_segs > 0x80000000u) { set_error("chop: graph too large for 32-bit ids"); return FLATGFA_ERR_TOO_LARGE; }
    if (j->counted) { set_error("chop: this job was counted already"); return FLATGFA_ERR_ARG; }
    j->in = in;
    j->c = c;
    j->links = links;
    j->seg_first = seg_first;
    j->last = st;
    // one allocation for the scans' scratch: header, segments, steps, paths, per-path lengths
    const size_t words = 8 + ScanBuf::words_for(in.n_segs) + ScanBuf::words_for(in.n_steps) + ScanBuf::words_for(in.n_paths) + in.n_paths;
    CHOP_HIP(hipMalloc(&j->mem, words * 8));
    CHOP_HIP(hipMemsetAsync(j->mem, 0, words * 8, st));
    uint64_t *p = j->mem;
    j->hdr = p;
    p += 8;
    j->seg.place(in.n_segs, p);
    j->step.place(in.n_steps, p);
    j->path.place(in.n_paths, p);
    j->plen = p;
    uint32_t *flags = reinterpret_cast<uint32_t *>(j->hdr);
    if (in.n_paths == 0) CHOP_HIP(hipMemsetAsync(flags, kNonTiling, 1, st));  // (no path: the pool is not walked)
    if (in.n_paths)
        hipLaunchKernelGGL(k_check_spans, dim3((uint32_t)blocks(in.n_paths, kThreads)), dim3(kThreads), 0, st, in.path_begin, in.path_end, in.n_paths,
                           in.n_steps, flags);
    if (links && in.n_links)
        hipLaunchKernelGGL(k_check_links<kThreads>, dim3((uint32_t)blocks(in.n_links, kThreads)), dim3(kThreads), 0, st, in.links, in.n_links, in.n_segs,
                           flags, kBadLink);
    launch_reduce(j->seg, SegCount{ChopPieces{in.seg_len, c}}, j->hdr + 1, st, "k_chop_reduce_segs");
    launch_reduce(j->step, StepCount{in.steps, in.n_segs, ChopPieces{in.seg_len, c}, flags}, j->hdr + 2, st, "k_chop_reduce_steps");
    if (in.n_paths) {
        hipLaunchKernelGGL(k_path_lens<ChopPieces>, dim3(std::min<uint32_t>(in.n_paths, 4096)), dim3(kThreads), 0, st, in.steps, in.path_begin,
                           in.path_end, in.n_paths, in.n_steps, ChopPieces{in.seg_len, c}, in.n_segs, flags, j->plen);
        launch_reduce(j->path, ArrCount{j->plen}, j->hdr + 3, st, "k_chop_reduce_paths");
    }
    CHOP_HIP(hipGetLastError());
    uint64_t h[4];
    CHOP_HIP(hipMemcpyAsync(h, j->hdr, sizeof h, hipMemcpyDeviceToHost, st));
    CHOP_HIP(hipStreamSynchronize(st));
    const uint32_t f = (uint32_t)h[0];
    if (f & kBadSpan) { set_error("chop: a path has a step span outside the steps pool"); return FLATGFA_ERR_BOUNDS; }
    if (f & kBadStep) { set_error("chop: a step refers to a segment id that is out of range"); return FLATGFA_ERR_BOUNDS; }
    if (f & kBadLink) { set_error("chop: a link refers to a segment id that is out of range"); return FLATGFA_ERR_BOUNDS; }
    j->tiling = !(f & kNonTiling);
    j->S2 = h[1];
    j->N2 = j->tiling ? h[2] : h[3];
    j->L2 = links ? j->S2 - in.n_segs + in.n_links : 0;
    // a handle is seg << 1 | orient in a u32; steps and links are counted in u32 (chop.rs through pool.rs Id)
    if (j->S2 >= 0x80000000ull || j->N2 > 0xFFFFFFFFull || j->L2 > 0xFFFFFFFFull) {
        set_error("chop: the chopped graph would have " + std::to_string(j->S2) + " segments, " + std::to_string(j->N2) + " steps and " +
                  std::to_string(j->L2) + " links: more than 32-bit ids hold");
        return FLATGFA_ERR_TOO_LARGE;
    }
    // the tile maps of the two expansions
    j->seg.n_out_tiles = (j->S2 + kOutTile - 1) / kOutTile;
    j->step.n_out_tiles = j->tiling ? (j->N2 + kOutTile - 1) / kOutTile : 0;
    const uint64_t mw = j->seg.n_out_tiles + j->step.n_out_tiles;
    if (mw) {
        CHOP_HIP(hipMalloc(&j->maps, mw * 4));
        j->seg.map = j->maps;
        j->step.map = j->maps + j->seg.n_out_tiles;
    }
    // seg_first, now that it fits
    if (in.n_segs) {
        launch_prefix(j->seg, st);
        hipLaunchKernelGGL((k_offsets<SegCount, SegFirstWriter>), dim3((uint32_t)j->seg.n_tiles), dim3(kThreads), 0, st, SegCount{ChopPieces{in.seg_len, c}},
                           (uint64_t)in.n_segs, j->seg.prefix, SegFirstWriter{seg_first});
    } else if (seg_first) {
        CHOP_HIP(hipMemsetAsync(seg_first, 0, 4, st));
    }
    CHOP_HIP(hipGetLastError());
    j->counted = true;
    *n_new_segs = j->S2;
    *n_new_steps = j->N2;
    if (n_new_links) *n_new_links = j->L2;
    return FLATGFA_OK;
}

int chop_fill(ChopJob *j, const ChopOut &out, hipStream_t st) {
    if (!j->counted) { set_error("chop: fill before a successful count"); return FLATGFA_ERR_ARG; }
    const ChopIn &in = j->in;
    if ((j->N2 && !out.steps) || (in.n_paths && (!out.path_begin || !out.path_end)) || (j->links && j->L2 && !out.links)) {
        set_error("chop: NULL output");
        return FLATGFA_ERR_ARG;
    }
    j->last = st;
    if (j->tiling) {
        launch_prefix(j->step, st);
        launch_map(j->step, st);
        if (j->N2) {
            ProfScope ps("k_chop_expand_steps", st);
            hipLaunchKernelGGL((k_expand<StepLoad, StepEmit>), dim3((uint32_t)j->step.n_out_tiles), dim3(kThreads), 0, st,
                               StepLoad{in.steps, j->seg_first, in.n_segs}, StepEmit{}, in.n_steps, j->step.prefix, j->step.n_tiles, j->step.map,
                               j->N2, out.steps);
        }
        if (in.n_paths)
            hipLaunchKernelGGL(k_path_spans, dim3((uint32_t)blocks(in.n_paths, kThreads / 64)), dim3(kThreads), 0, st, in.steps, in.path_begin, in.path_end,
                               in.n_paths, in.n_steps, j->seg_first, in.n_segs, j->step.prefix, out.path_begin, out.path_end);
    } else if (in.n_paths) {
        launch_prefix(j->path, st);
        hipLaunchKernelGGL((k_offsets<ArrCount, PathWriter>), dim3((uint32_t)j->path.n_tiles), dim3(kThreads), 0, st, ArrCount{j->plen},
                           (uint64_t)in.n_paths, j->path.prefix, PathWriter{out.path_begin, out.path_end});
        ProfScope ps("k_chop_expand_paths", st);
        hipLaunchKernelGGL(k_expand_paths, dim3(std::min<uint32_t>(in.n_paths, 4096)), dim3(kThreads), 0, st, in.steps, in.path_begin,
                           in.path_end, in.n_paths, in.n_steps, j->seg_first, in.n_segs, out.path_begin, out.steps);
    }
    if (j->S2) {
        launch_map(j->seg, st);
        ProfScope ps("k_chop_expand_segs", st);
        hipLaunchKernelGGL((k_expand<SegLoad, SegEmit>), dim3((uint32_t)j->seg.n_out_tiles), dim3(kThreads), 0, st,
                           SegLoad{in.seg_len, in.seq_start, j->c}, SegEmit{j->c, out.seg_recs, j->links ? out.links : nullptr}, (uint64_t)in.n_segs,
                           j->seg.prefix, j->seg.n_tiles, j->seg.map, j->S2, out.seg_len);
    }
    if (j->links && in.n_links)
        hipLaunchKernelGGL(k_links, dim3((uint32_t)blocks(in.n_links, kThreads)), dim3(kThreads), 0, st, in.links, in.n_links, j->seg_first, in.n_segs,
                           out.links + (j->S2 - in.n_segs) * 4);
    CHOP_HIP(hipGetLastError());
    return FLATGFA_OK;
}

}  // namespace fgfa_dev

// ---- the device-level C ABI (include/flatgfa.h Part 3) ----
struct flatgfa_dev_chop {
    fgfa_dev::ChopJob *job = nullptr;
    ~flatgfa_dev_chop() { fgfa_dev::chop_free(job); }
};

extern "C" {

int flatgfa_dev_chop_count(const flatgfa_dev_graph_t *g, uint64_t max_size, uint32_t *seg_first, void *stream, flatgfa_dev_chop_t **job,
                           uint64_t *n_segs_out, uint64_t *n_steps_out) {
    if (job) *job = nullptr;
    if (!g || !job || !n_segs_out || !n_steps_out) { fgfa_dev::set_error("flatgfa_dev_chop_count: NULL argument"); return FLATGFA_ERR_ARG; }
    if (!g->seg_len) { fgfa_dev::set_error("flatgfa_dev_chop_count: the graph has no seg_len"); return FLATGFA_ERR_ARG; }
    fgfa_dev::ChopIn in;
    in.steps = g->steps;
    in.n_steps = g->n_steps;
    in.path_begin = g->path_begin;
    in.path_end = g->path_end;
    in.n_paths = g->n_paths;
    in.n_segs = g->n_segs;
    in.seg_len = g->seg_len;
    auto *h = new flatgfa_dev_chop();
    h->job = fgfa_dev::chop_new();
    const int rc = fgfa_dev::chop_count(h->job, in, max_size, false, seg_first, (hipStream_t)stream, n_segs_out, n_steps_out, nullptr);
    if (rc) {
        delete h;
        return rc;
    }
    *job = h;
    return FLATGFA_OK;
}

int flatgfa_dev_chop_fill(flatgfa_dev_chop_t *job, uint32_t *steps, uint32_t *path_begin, uint32_t *path_end, uint32_t *seg_len, void *stream) {
    if (!job) { fgfa_dev::set_error("flatgfa_dev_chop_fill: NULL job"); return FLATGFA_ERR_ARG; }
    fgfa_dev::ChopOut out;
    out.steps = steps;
    out.path_begin = path_begin;
    out.path_end = path_end;
    out.seg_len = seg_len;
    return fgfa_dev::chop_fill(job->job, out, (hipStream_t)stream);
}

void flatgfa_dev_chop_free(flatgfa_dev_chop_t *job) { delete job; }

}  // extern "C"
