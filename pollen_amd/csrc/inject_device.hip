// Inject on gfx950 (slow_odgi/inject.py, `odgi inject`).
//
// Every BED line "path low high name" cuts the segments under its two ends so that both fall on segment seams, and adds a path
// that walks exactly the interval.  The reference does this a line at a time on the graph the line before left; here it is one
// pass, which gives the same graph because base positions along a path never change and a cut only ever inserts a seam:
//
//   positions     one u64 scan (k_scan + k_spine) of seg_len[step >> 1] over the steps pool: pre[i] = the bases before step i
//                 of the pool.  A step's walk -- the bases before it on its path -- is pre[i] - pre[begin], for any spans.
//   k_locate      one lane per line end x: a bisection of the path's span of pre for the first step with walk + len > x.  No such
//                 step, or walk == x: the end is on a seam already.  Else the cut is at o = x - walk of the step: position o
//                 of a forward step's segment, len - o of a backward one's.  The segment's raw count goes up by one.
//   cut table     the raw rows (a u32 scan of the counts, a scatter behind a cursor per row) hold (segment, position) keys;
//                 k_sort_short sorts the rows of up to 16 keys by one lane and lists the longer ones, k_sort_long sorts each
//                 listed row with a workgroup (bitonic, in place), a scan of the "differs from the key before" flags
//                 compacts them: cut_row[s] .. cut_row[s + 1] are the distinct sorted cuts of s, seg_first[s] = s + cut_row[s].
//   expansion     the kernels and the driver that chop uses too (expand_kernels.hpp: the Expansion and its expand_* functions,
//                 called in order below with inject's launches between them), with the piece count of a segment taken from
//                 the table: k + 1.
//   new paths     noff[i] = the new steps before old step i of the pool (a u32 scan); k_line_spans finds each line's
//                 [n_lo, n_hi) relative to its path's new begin -- the old step that holds low or high, plus the pieces before
//                 the cut within it (reversed for a backward step) -- a scan of the lengths lays the new paths out behind the old
//                 ones, and k_copy_lines writes them, one workgroup per 2048 output steps whatever the lines' lengths.
//
// Scratch: 12 bytes a step (pre and noff over the whole pool), 24 bytes a line end.  Kernels never trap: a bad span, step,
// link or path id raises a bit of the flag word that the count reads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/flatgfa.h"
#include "device_common.hpp"
#include "device_scan.hpp"
#include "expand_kernels.hpp"
#include "inject_device.hpp"
#include "prof.hpp"

namespace fgfa_dev {
namespace {

constexpr uint32_t kPer = 4;         // consecutive elements per lane of the tiled scans
constexpr uint32_t kScanTile = kThreads * kPer;
constexpr uint32_t kLinear = 16;     // cut rows up to this long are sorted by one lane
constexpr uint32_t kMaxGrid = 2048;  // workgroups of a grid-stride launch
constexpr uint32_t kNone = 0xFFFFFFFFu;

// the pieces of a segment: one more than its distinct cuts
struct CutPieces {
    const uint32_t *cut_row;
    __device__ uint64_t operator()(uint32_t s) const { return (uint64_t)(cut_row[s + 1] - cut_row[s]) + 1; }
};

// ---- positions ----
struct PosOp {  // pre[i] = the lengths of the steps before i (a step that names no segment has none); i runs to n inclusive
    const uint32_t *steps, *len;
    uint32_t n_segs;
    uint64_t n;
    uint64_t *pre;
    __device__ Sum<uint64_t> load(uint64_t i) const {
        if (i >= n) return Sum<uint64_t>{0};
        const uint32_t s = steps[i] >> 1;
        return Sum<uint64_t>{s < n_segs ? len[s] : 0u};
    }
    __device__ void store(uint64_t i, uint64_t before, const Sum<uint64_t> &) const { pre[i] = before; }
};
struct NoffOp {  // noff[i] = the new steps of the steps before i, modulo 2^32 (differences within a path are exact)
    const uint32_t *steps;
    uint32_t n_segs;
    uint64_t n;
    CutPieces pc;
    uint32_t *noff;
    __device__ Sum<uint32_t> load(uint64_t i) const {
        if (i >= n) return Sum<uint32_t>{0};
        const uint32_t s = steps[i] >> 1;
        return Sum<uint32_t>{s < n_segs ? (uint32_t)pc(s) : 1u};
    }
    __device__ void store(uint64_t i, uint32_t before, const Sum<uint32_t> &) const { noff[i] = before; }
};
struct RowOp {  // data[i] becomes the sum of data[0 .. i), in place
    uint32_t *data;
    __device__ Sum<uint32_t> load(uint64_t i) const { return Sum<uint32_t>{data[i]}; }
    __device__ void store(uint64_t i, uint32_t before, const Sum<uint32_t> &) const { data[i] = before; }
};
struct DistinctOp {  // dpos[i] = the distinct keys before raw key i; i runs to m inclusive, keys at or past *total count nothing
    const uint64_t *raw;
    const uint32_t *total;
    uint64_t m;
    uint32_t *dpos;
    __device__ Sum<uint32_t> load(uint64_t i) const {
        if (i >= m || i >= *total) return Sum<uint32_t>{0};
        return Sum<uint32_t>{(i == 0 || raw[i] != raw[i - 1]) ? 1u : 0u};
    }
    __device__ void store(uint64_t i, uint32_t before, const Sum<uint32_t> &) const { dpos[i] = before; }
};

// the first step i of [b, e) with pre[i + 1] - pre[b] > x, the step that holds base x of the path; e when there is none
__device__ __forceinline__ uint64_t step_holding(const uint64_t *pre, uint64_t b, uint64_t e, uint64_t x) {
    const uint64_t base = pre[b];
    uint64_t lo = b, hi = e;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (pre[mid + 1] - base > x) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// ---- locate ----
// inject.py:24-46 (where_chop, handle_pos).  Line end e = 2 l + side: end_step[e] = the step that holds x (the path's end when
// none does), end_seg[e] / end_pos[e] = the cut, or kNone when x is on a seam already.
__global__ __launch_bounds__(kThreads) void k_locate(const uint32_t *__restrict__ line_path, const uint64_t *__restrict__ line_lo,
                                                     const uint64_t *__restrict__ line_hi, uint64_t n_ends, const uint32_t *__restrict__ pb,
                                                     const uint32_t *__restrict__ pe, uint32_t n_paths, const uint32_t *__restrict__ steps,
                                                     uint64_t n_steps, const uint32_t *__restrict__ len, uint32_t n_segs,
                                                     const uint64_t *__restrict__ pre, uint32_t *__restrict__ end_step,
                                                     uint32_t *__restrict__ end_seg, uint32_t *__restrict__ end_pos, uint32_t *raw_cnt,
                                                     uint32_t *flags) {
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= n_ends) return;
    const uint64_t l = t >> 1;
    const uint32_t p = line_path[l];
    uint32_t at = 0, seg = kNone, pos = 0;
    if (p >= n_paths) {
        atomicOr(flags, kBadPath);
    } else {
        const uint64_t x = (t & 1) ? line_hi[l] : line_lo[l];
        uint64_t b, e;
        clamp_span(pb[p], pe[p], n_steps, &b, &e);
        const uint64_t i = step_holding(pre, b, e, x);
        at = (uint32_t)i;
        if (i < e) {
            const uint64_t walk = pre[i] - pre[b];
            if (walk < x) {  // (walk + len > x: the step has bases, so it names a segment)
                const uint32_t h = steps[i], s = h >> 1, o = (uint32_t)(x - walk);
                seg = s;
                pos = (h & 1u) ? len[s] - o : o;
                atomicAdd(raw_cnt + s, 1u);
            }
        }
    }
    end_step[t] = at;
    end_seg[t] = seg;
    end_pos[t] = pos;
}

// ---- the cut table ----
__global__ __launch_bounds__(kThreads) void k_cut_scatter(const uint32_t *__restrict__ end_seg, const uint32_t *__restrict__ end_pos, uint64_t n_ends,
                                                          const uint32_t *__restrict__ raw_row, uint32_t *cursor, uint64_t *__restrict__ raw) {
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= n_ends) return;
    const uint32_t s = end_seg[t];
    if (s == kNone) return;
    const uint64_t at = (uint64_t)raw_row[s] + atomicAdd(cursor + s, 1u);
    if (at < raw_row[s + 1]) raw[at] = ((uint64_t)s << 32) | end_pos[t];
}

// rows of up to kLinear keys: an insertion sort by one lane; longer ones are listed for k_sort_long
__global__ __launch_bounds__(kThreads) void k_sort_short(const uint32_t *__restrict__ raw_row, uint32_t n_segs, uint64_t *raw, uint32_t *list,
                                                         uint32_t cap, uint32_t *count) {
    for (uint64_t s = (uint64_t)blockIdx.x * kThreads + threadIdx.x; s < n_segs; s += (uint64_t)gridDim.x * kThreads) {
        const uint32_t r0 = raw_row[s], n = raw_row[s + 1] - r0;
        if (n < 2) continue;
        if (n > kLinear) {
            const uint32_t k = atomicAdd(count, 1u);
            if (k < cap) list[k] = (uint32_t)s;
            continue;
        }
        uint64_t *v = raw + r0;
        for (uint32_t a = 1; a < n; ++a) {
            const uint64_t x = v[a];
            uint32_t q = a;
            while (q > 0 && v[q - 1] > x) {
                v[q] = v[q - 1];
                --q;
            }
            v[q] = x;
        }
    }
}

// One workgroup per listed row, as topology_device.hip's k_sort_rows: compare-exchanges (i, l) with i < l always leave the
// smaller at i, and an l at or past the row's end stands for +infinity and is already in place.
__global__ __launch_bounds__(kThreads) void k_sort_long(const uint32_t *__restrict__ raw_row, uint64_t *raw, const uint32_t *__restrict__ list,
                                                        uint32_t cap, const uint32_t *__restrict__ count) {
    const uint32_t n_list = min(*count, cap);
    for (uint32_t r = blockIdx.x; r < n_list; r += gridDim.x) {
        const uint32_t s = list[r];
        uint64_t *v = raw + raw_row[s];
        const uint64_t n = raw_row[s + 1] - raw_row[s];
        uint64_t pow2 = 1;
        while (pow2 < n) pow2 <<= 1;
        for (uint64_t k = 2; k <= pow2; k <<= 1) {
            for (uint64_t j = k >> 1; j > 0; j >>= 1) {
                const uint64_t mask = j == (k >> 1) ? k - 1 : j;  // the first step of a merge flips, the rest disperse
                for (uint64_t i = threadIdx.x; i < n; i += kThreads) {
                    const uint64_t l = i ^ mask;
                    if (l > i && l < n) {
                        const uint64_t x = v[i], y = v[l];
                        if (x > y) v[i] = y, v[l] = x;
                    }
                }
                __syncthreads();
            }
        }
    }
}

// the distinct keys, compacted: cuts[dpos[i]] = the position of raw key i when it differs from the key before it
__global__ __launch_bounds__(kThreads) void k_cut_compact(const uint64_t *__restrict__ raw, const uint32_t *__restrict__ total,
                                                          const uint32_t *__restrict__ dpos, uint32_t *__restrict__ cuts) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= *total) return;
    if (i == 0 || raw[i] != raw[i - 1]) cuts[dpos[i]] = (uint32_t)raw[i];
}
__global__ __launch_bounds__(kThreads) void k_cut_rows(const uint32_t *__restrict__ raw_row, const uint32_t *__restrict__ dpos, uint64_t n_rows1,
                                                       uint32_t *__restrict__ cut_row) {
    const uint64_t s = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (s < n_rows1) cut_row[s] = dpos[raw_row[s]];
}

// ---- new segments ----
struct CutSegLoad {
    const uint32_t *len, *cut_row;
    __device__ void operator()(uint64_t i, uint32_t *cnt, uint32_t *a, uint32_t *b) const {
        *cnt = cut_row[i + 1] - cut_row[i] + 1;
        *a = len[i];
        *b = cut_row[i];
    }
};
struct CutSegEmit {  // new segment jj is piece p of k of old segment i (length a, cuts from row b): inject.py:70-75
    const uint32_t *cuts, *seq_start;
    uint32_t *recs, *links;
    __device__ uint32_t operator()(uint64_t jj, uint64_t i, uint32_t a, uint32_t b, uint32_t p, uint32_t k) const {
        const uint32_t lo = p ? cuts[b + p - 1] : 0u, hi = p + 1 < k ? cuts[b + p] : a;
        write_piece(recs, links, jj, i, (seq_start ? seq_start[i] : 0u) + lo, hi - lo, p, k);
        return hi - lo;
    }
};

// ---- new paths ----
// The piece of a step that starts at its cut `pos` (a position of segment s), counted along the step: the pieces of a backward
// step are walked in reverse (chop.py:55).
__device__ __forceinline__ uint32_t piece_at_cut(const uint32_t *cut_row, const uint32_t *cuts, uint32_t s, uint32_t pos, bool backward) {
    const uint32_t r0 = cut_row[s], k = cut_row[s + 1] - r0;
    uint32_t lo = 0, hi = k;  // the rank of pos among the k cuts of s
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cuts[r0 + mid] < pos) lo = mid + 1;
        else hi = mid;
    }
    return backward ? k - lo : lo + 1;
}

// inject.py:6-21 (track_path) on the cut path: the new steps from the first with start >= low up to the first with end > high.
// line_rel[l] = the first of them, counted from the path's new begin; line_len[l] = how many.
__global__ __launch_bounds__(kThreads) void k_line_spans(const uint32_t *__restrict__ line_path, const uint64_t *__restrict__ line_lo, uint64_t n_lines,
                                                         const uint32_t *__restrict__ pb, const uint32_t *__restrict__ pe, uint32_t n_paths,
                                                         const uint32_t *__restrict__ steps, uint64_t n_steps, const uint64_t *__restrict__ pre,
                                                         const uint32_t *__restrict__ noff, const uint32_t *__restrict__ end_step,
                                                         const uint32_t *__restrict__ end_seg, const uint32_t *__restrict__ end_pos,
                                                         const uint32_t *__restrict__ cut_row, const uint32_t *__restrict__ cuts,
                                                         uint32_t *__restrict__ line_rel, uint64_t *__restrict__ line_len) {
    const uint64_t l = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (l >= n_lines) return;
    const uint32_t p = line_path[l];
    uint32_t rel[2] = {0, 0};
    if (p < n_paths) {  // (else reported by k_locate)
        uint64_t b, e;
        clamp_span(pb[p], pe[p], n_steps, &b, &e);
        const uint32_t nb = noff[b];
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const uint64_t t = 2 * l + side;
            const uint32_t s = end_seg[t];
            uint64_t i = end_step[t];
            uint32_t w = 0;
            if (s != kNone) {
                w = piece_at_cut(cut_row, cuts, s, end_pos[t], steps[i] & 1u);
            } else if (side == 0) {  // the first step with walk >= low (a step of no bases at low is inside)
                const uint64_t low = line_lo[l], base = pre[b];
                uint64_t lo = b, hi = e;
                while (lo < hi) {
                    const uint64_t mid = lo + ((hi - lo) >> 1);
                    if (pre[mid] - base >= low) hi = mid;
                    else lo = mid + 1;
                }
                i = lo;
            }
            rel[side] = noff[i] - nb + w;
        }
    }
    line_rel[l] = rel[0];
    line_len[l] = rel[1] > rel[0] ? rel[1] - rel[0] : 0u;
}

struct NewPathWriter {  // new path l lies at base + the lengths of the lines before it
    uint32_t *begin, *end;
    uint64_t base;
    __device__ void operator()(uint64_t i, uint64_t, uint64_t ex, uint64_t cnt) const {
        begin[i] = (uint32_t)(base + ex);
        end[i] = (uint32_t)(base + ex + cnt);
    }
};

// One workgroup per kOutTile steps of the new paths, [base, total) of the new pool: each lane finds the line its first step
// belongs to (the last line that begins at or before it: lines of no steps share their begin with the next) and copies kItems
// consecutive steps from where the line's path was expanded to.
__global__ __launch_bounds__(kThreads) void k_copy_lines(uint32_t *steps, uint64_t base, uint64_t total, const uint32_t *__restrict__ new_begin,
                                                         const uint32_t *__restrict__ new_end, uint64_t n_lines,
                                                         const uint32_t *__restrict__ line_path, const uint32_t *__restrict__ line_rel,
                                                         const uint32_t *__restrict__ path_begin) {
    const uint64_t j0 = base + (uint64_t)blockIdx.x * kOutTile + (uint64_t)threadIdx.x * kItems;
    if (j0 >= total) return;
    uint64_t lo = 0, hi = n_lines - 1;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo + 1) >> 1);
        if (new_begin[mid] <= j0) lo = mid;
        else hi = mid - 1;
    }
    uint64_t l = lo;
    uint32_t nb = new_begin[l], ne = new_end[l];
    uint64_t src = (uint64_t)path_begin[line_path[l]] + line_rel[l];
    for (uint32_t q = 0; q < kItems && j0 + q < total; ++q) {
        const uint64_t j = j0 + q;
        while (j >= ne && l + 1 < n_lines) {
            ++l;
            nb = new_begin[l];
            ne = new_end[l];
            src = (uint64_t)path_begin[line_path[l]] + line_rel[l];
        }
        steps[j] = steps[src + (j - nb)];
    }
}

constexpr ExpandNames kInject{"inject: ", "graph", "k_inject_reduce_segs", "k_inject_reduce_steps", "k_inject_reduce_paths",
                              "k_inject_expand_steps", "k_inject_expand_paths", "k_inject_expand_segs"};

}  // namespace

struct InjectJob {
    Expansion x;  // (N_add: the new paths' steps)
    InjectLines lines;
    uint64_t *line_len = nullptr;
    uint32_t *cut_row = nullptr, *cuts = nullptr, *line_rel = nullptr;
    ScanBuf line;
};

InjectJob *inject_new() { return new InjectJob(); }
void inject_free(InjectJob *j) { delete j; }

#define INJ_HIP(expr) FGFA_HIP("inject: ", expr)

int inject_count(InjectJob *j, const ChopIn &in, const InjectLines &ln, bool links, uint32_t *seg_first, hipStream_t st, uint64_t *n_new_segs,
                 uint64_t *n_new_steps, uint64_t *n_new_links) {
    if (int rc = expand_check_args(kInject, in, links, seg_first, ln.n && (!ln.path_id || !ln.start || !ln.end))) return rc;
    if (ln.n >= 0x7FFFFFFFull || (uint64_t)in.n_paths + ln.n > 0xFFFFFFFFull) {
        set_error("inject: " + std::to_string(ln.n) + " lines: more paths than 32-bit ids hold");
        return FLATGFA_ERR_TOO_LARGE;
    }
    Expansion &x = j->x;
    const uint64_t N = in.n_steps, S = in.n_segs, n = ln.n, M = 2 * n;
    // behind the driver's scratch, in its one block: the lines' scan and their lengths
    uint64_t *p = nullptr;
    if (int rc = expand_begin(x, kInject, in, links, seg_first, st, ScanBuf::words_for(n) + n, &p)) return rc;
    j->lines = ln;
    j->line.place(n, p);
    j->line_len = p;
    uint32_t *flags = reinterpret_cast<uint32_t *>(x.hdr);
    // positions, line ends, the cut table
    uint64_t *pre = nullptr, *raw = nullptr;
    uint32_t *noff = nullptr, *end_step = nullptr, *end_seg = nullptr, *end_pos = nullptr, *raw_row = nullptr, *cursor = nullptr, *list = nullptr,
             *dpos = nullptr, *words4 = nullptr;
    const uint64_t list_cap = M / (kLinear + 1) + 1;  // (a listed row holds more than kLinear of the M keys)
    const uint64_t n_pos = n ? N + 1 : 0;  // (no line: no position is asked for, and the copy of the graph costs no 12 bytes a step)
    INJ_HIP(x.dm.alloc(&pre, n_pos));
    INJ_HIP(x.dm.alloc(&noff, n_pos));
    INJ_HIP(x.dm.alloc(&end_step, 3 * M));
    end_seg = end_step + M;
    end_pos = end_seg + M;
    INJ_HIP(x.dm.alloc(&raw_row, 2 * (S + 2)));  // the raw rows, then the rows of distinct cuts
    j->cut_row = raw_row + (S + 2);
    INJ_HIP(x.dm.alloc(&cursor, S));
    INJ_HIP(x.dm.alloc(&list, list_cap));
    INJ_HIP(x.dm.alloc(&raw, M));
    INJ_HIP(x.dm.alloc(&dpos, M + 1));
    INJ_HIP(x.dm.alloc(&j->cuts, M));
    INJ_HIP(x.dm.alloc(&j->line_rel, n));
    INJ_HIP(x.dm.alloc(&words4, 4));  // the long-row count
    Spine<Sum<uint64_t>> sp;  // (one spine for the scans below, which run one behind another)
    INJ_HIP(sp.alloc(&x.dm, blocks(std::max<uint64_t>(std::max(n_pos, M), S) + 2, kScanTile)));
    INJ_HIP(hipMemsetAsync(raw_row, 0, 2 * (S + 2) * 4, st));
    INJ_HIP(hipMemsetAsync(cursor, 0, std::max<uint64_t>(S, 1) * 4, st));
    INJ_HIP(hipMemsetAsync(words4, 0, 16, st));
    INJ_HIP(hipMemsetAsync(dpos, 0, 4, st));
    if (int rc = expand_check_graph(x, kInject, st)) return rc;
    const Spine<Sum<uint32_t>> sp32{sp.aggr, sp.prefix, sp.total};
    if (n) {
        ProfScope ps("k_inject_positions", st);
        const PosOp op{in.steps, in.seg_len, in.n_segs, N, pre};
        scan_count<kThreads, kPer>(op, N + 1, sp, st);
        scan_apply<kThreads, kPer>(op, N + 1, sp, st);
    }
    if (M) {
        {
            ProfScope ps("k_inject_locate", st);
            hipLaunchKernelGGL(k_locate, dim3((uint32_t)blocks(M, kThreads)), dim3(kThreads), 0, st, ln.path_id, ln.start, ln.end, M, in.path_begin,
                               in.path_end, in.n_paths, in.steps, N, in.seg_len, in.n_segs, pre, end_step, end_seg, end_pos, raw_row, flags);
        }
        ProfScope ps("k_inject_cut_table", st);
        const RowOp rows{raw_row};
        scan_count<kThreads, kPer>(rows, S + 1, sp32, st);
        scan_apply<kThreads, kPer>(rows, S + 1, sp32, st);
        hipLaunchKernelGGL(k_cut_scatter, dim3((uint32_t)blocks(M, kThreads)), dim3(kThreads), 0, st, end_seg, end_pos, M, raw_row, cursor, raw);
        if (S) {
            hipLaunchKernelGGL(k_sort_short, dim3(stride_blocks(S, kThreads, kMaxGrid)), dim3(kThreads), 0, st, raw_row, in.n_segs, raw, list,
                               (uint32_t)list_cap, words4);
            hipLaunchKernelGGL(k_sort_long, dim3((uint32_t)std::min<uint64_t>(list_cap, kMaxGrid)), dim3(kThreads), 0, st, raw_row, raw, list,
                               (uint32_t)list_cap, words4);
        }
        const DistinctOp dop{raw, raw_row + S, M, dpos};
        scan_count<kThreads, kPer>(dop, M + 1, sp32, st);
        scan_apply<kThreads, kPer>(dop, M + 1, sp32, st);
        hipLaunchKernelGGL(k_cut_compact, dim3((uint32_t)blocks(M, kThreads)), dim3(kThreads), 0, st, raw, raw_row + S, dpos, j->cuts);
        hipLaunchKernelGGL(k_cut_rows, dim3((uint32_t)blocks(S + 1, kThreads)), dim3(kThreads), 0, st, raw_row, dpos, S + 1, j->cut_row);
    }
    // the piece counts, from the table
    const CutPieces pc{j->cut_row};
    expand_reduce(x, kInject, pc, st);
    // the new paths' lengths
    if (n) {
        ProfScope ps("k_inject_line_spans", st);
        const NoffOp nop{in.steps, in.n_segs, N, pc, noff};
        scan_count<kThreads, kPer>(nop, N + 1, sp32, st);
        scan_apply<kThreads, kPer>(nop, N + 1, sp32, st);
        hipLaunchKernelGGL(k_line_spans, dim3((uint32_t)blocks(n, kThreads)), dim3(kThreads), 0, st, ln.path_id, ln.start, n, in.path_begin, in.path_end,
                           in.n_paths, in.steps, N, pre, noff, end_step, end_seg, end_pos, j->cut_row, j->cuts, j->line_rel, j->line_len);
        launch_reduce(j->line, ArrCount{j->line_len}, x.hdr + 4, st, "k_inject_reduce_lines");
    }
    return expand_totals(x, kInject, pc, st, n_new_segs, n_new_steps, n_new_links);
}

int inject_fill(InjectJob *j, const ChopOut &out, hipStream_t st) {
    Expansion &x = j->x;
    const ChopIn &in = x.in;
    const uint64_t n = j->lines.n;
    if (int rc = expand_fill(x, kInject, CutSegLoad{in.seg_len, j->cut_row},
                             CutSegEmit{j->cuts, in.seq_start, out.seg_recs, x.links ? out.links : nullptr}, out, n, st))
        return rc;
    // the new paths, behind the old ones
    if (n) {
        uint32_t *nb = out.path_begin + in.n_paths, *ne = out.path_end + in.n_paths;
        launch_prefix(j->line, st);
        hipLaunchKernelGGL((k_offsets<ArrCount, NewPathWriter>), dim3((uint32_t)j->line.n_tiles), dim3(kThreads), 0, st, ArrCount{j->line_len}, n,
                           j->line.prefix, NewPathWriter{nb, ne, x.N_old2});
        if (x.N_add) {
            ProfScope ps("k_inject_copy_lines", st);
            hipLaunchKernelGGL(k_copy_lines, dim3((uint32_t)blocks(x.N_add, kOutTile)), dim3(kThreads), 0, st, out.steps, x.N_old2, x.N2(), nb, ne, n,
                               j->lines.path_id, j->line_rel, out.path_begin);
        }
    }
    INJ_HIP(hipGetLastError());
    return FLATGFA_OK;
}

}  // namespace fgfa_dev

// ---- the device-level C ABI (include/flatgfa.h Part 3) ----
struct flatgfa_dev_inject : fgfa_dev::InjectJob {};

extern "C" {

int flatgfa_dev_inject_count(const flatgfa_dev_graph_t *g, const uint32_t *d_path_id, const uint64_t *d_start, const uint64_t *d_end, uint64_t n,
                             uint32_t *seg_first, void *stream, flatgfa_dev_inject_t **job, uint64_t *n_segs_out, uint64_t *n_steps_out,
                             uint64_t *n_paths_out) {
    if (job) *job = nullptr;
    if (!g || !job || !n_segs_out || !n_steps_out || !n_paths_out) { fgfa_dev::set_error("flatgfa_dev_inject_count: NULL argument"); return FLATGFA_ERR_ARG; }
    if (!g->seg_len) { fgfa_dev::set_error("flatgfa_dev_inject_count: the graph has no seg_len"); return FLATGFA_ERR_ARG; }
    fgfa_dev::InjectLines ln;
    ln.path_id = d_path_id;
    ln.start = d_start;
    ln.end = d_end;
    ln.n = n;
    auto *h = new flatgfa_dev_inject();
    const int rc = fgfa_dev::inject_count(h, fgfa_dev::chop_in_of(*g), ln, false, seg_first, (hipStream_t)stream, n_segs_out, n_steps_out, nullptr);
    if (rc) {
        delete h;
        return rc;
    }
    *n_paths_out = (uint64_t)g->n_paths + n;
    *job = h;
    return FLATGFA_OK;
}

int flatgfa_dev_inject_fill(flatgfa_dev_inject_t *job, uint32_t *steps, uint32_t *path_begin, uint32_t *path_end, uint32_t *seg_len, void *stream) {
    if (!job) { fgfa_dev::set_error("flatgfa_dev_inject_fill: NULL job"); return FLATGFA_ERR_ARG; }
    return fgfa_dev::inject_fill(job, fgfa_dev::chop_out_of(steps, path_begin, path_end, seg_len), (hipStream_t)stream);
}

void flatgfa_dev_inject_free(flatgfa_dev_inject_t *job) { delete job; }

}  // extern "C"
