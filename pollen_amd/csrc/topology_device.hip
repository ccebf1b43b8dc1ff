// Validate and degree on gfx950 (slow_odgi/slow_odgi/validate.py, degree.py over mygfa/preprocess.py:23-43).
//
//   k_link_count    one pass over the links: the row of every link's canonical key is counted (a link and its reverse
//                   complement share one key, so a step pair needs one lookup), and so are the two link ends per segment
//                   (the degree).  A link naming a segment out of range raises a flag bit and is left out.
//   k_scan          (device_scan.hpp, over RowOp) the exclusive scan of the row counts, in place, in three launches (tile
//                   sums, k_spine, tiles again).
//   k_link_scatter  the low half of every key goes into its row, behind a cursor per row.
//   k_sort_rows     rows longer than kLinear are sorted, one workgroup per row (a bitonic network in which every compare
//                   points upwards, so the padding to a power of two stays virtual); shorter rows are probed linearly.
//   k_steps         the one read of the steps: tiles of kTile consecutive steps of the paths laid one behind another, dealt
//                   to at most kMaxGrid workgroups.  Every step but a path's last forms a pair with its successor, whichever
//                   lane, wave or workgroup reads that one, so a pair is checked exactly once, by the owner of its first
//                   step.  Count launch: missing pairs per tile.  k_spine.  Fill launch: the tiles that have any write their
//                   records at their prefix, in step order -- no atomics on the data path, so the order is the reference's.
// Kernels never trap: a bad step or link raises a bit of the flag word.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/flatgfa.h"
#include "device_common.hpp"
#include "device_scan.hpp"
#include "host_copy.hpp"
#include "topology_device.hpp"

namespace fgfa_dev {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kPer = 4;  // consecutive elements per lane
constexpr uint32_t kTile = kThreads * kPer;
constexpr uint32_t kMaxGrid = 2048;  // workgroups of a grid-stride launch
constexpr uint32_t kLinear = 16;     // rows up to this long are probed linearly (one 64-byte line), longer ones are sorted

// flag word bits
constexpr uint32_t kBadStep = 1, kBadLink = 2;

__device__ __forceinline__ uint64_t canon(uint32_t from, uint32_t to) {
    const uint64_t x = ((uint64_t)from << 32) | to, y = ((uint64_t)(to ^ 1u) << 32) | (from ^ 1u);
    return x < y ? x : y;
}

// The row scan: data[i] becomes the sum of data[0 .. i), in place (k_scan holds a lane's elements before it stores any).
struct RowOp {
    uint32_t *data;
    __device__ Sum<uint32_t> load(uint64_t i) const { return Sum<uint32_t>{data[i]}; }
    __device__ void store(uint64_t i, uint32_t before, const Sum<uint32_t> &) const { data[i] = before; }
};

// preprocess.py:39-41: every link adds one entry to outs[from] and one to ins[to] -- here one key, and two link ends.
__global__ __launch_bounds__(kThreads) void k_link_count(const uint32_t *__restrict__ links, uint64_t n_links, uint32_t n_segs, uint32_t *row,
                                                         uint32_t *deg, uint32_t *flags) {
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n_links; i += (uint64_t)gridDim.x * kThreads) {
        const uint32_t f = links[i * 4], t = links[i * 4 + 1];
        if ((f >> 1) >= n_segs || (t >> 1) >= n_segs) {
            atomicOr(flags, kBadLink);
            continue;
        }
        atomicAdd(row + (canon(f, t) >> 32), 1u);
        atomicAdd(deg + (f >> 1), 1u);
        atomicAdd(deg + (t >> 1), 1u);
    }
}

__global__ __launch_bounds__(kThreads) void k_link_scatter(const uint32_t *__restrict__ links, uint64_t n_links, uint32_t n_segs,
                                                           const uint32_t *__restrict__ row, uint32_t *cursor, uint32_t *__restrict__ to) {
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n_links; i += (uint64_t)gridDim.x * kThreads) {
        const uint32_t f = links[i * 4], t = links[i * 4 + 1];
        if ((f >> 1) >= n_segs || (t >> 1) >= n_segs) continue;
        const uint64_t key = canon(f, t);
        const uint32_t h = (uint32_t)(key >> 32);
        const uint64_t at = (uint64_t)row[h] + atomicAdd(cursor + h, 1u);
        if (at < row[h + 1]) to[at] = (uint32_t)key;
    }
}

__global__ __launch_bounds__(kThreads) void k_long_rows(const uint32_t *__restrict__ row, uint64_t n_rows, uint32_t *list, uint32_t cap,
                                                        uint32_t *count) {
    for (uint64_t h = (uint64_t)blockIdx.x * kThreads + threadIdx.x; h < n_rows; h += (uint64_t)gridDim.x * kThreads) {
        if (row[h + 1] - row[h] <= kLinear) continue;
        const uint32_t k = atomicAdd(count, 1u);
        if (k < cap) list[k] = (uint32_t)h;
    }
}

// One workgroup per listed row.  Compare-exchanges (i, l) with i < l always leave the smaller at i: an l at or past the row's
// end stands for +infinity and is already in place.
__global__ __launch_bounds__(kThreads) void k_sort_rows(const uint32_t *__restrict__ row, uint32_t *to, const uint32_t *__restrict__ list,
                                                        uint32_t n_list) {
    for (uint32_t r = blockIdx.x; r < n_list; r += gridDim.x) {
        const uint32_t h = list[r];
        uint32_t *v = to + row[h];
        const uint64_t n = row[h + 1] - row[h];
        uint64_t pow2 = 1;
        while (pow2 < n) pow2 <<= 1;
        for (uint64_t k = 2; k <= pow2; k <<= 1) {
            for (uint64_t j = k >> 1; j > 0; j >>= 1) {
                const uint64_t mask = j == (k >> 1) ? k - 1 : j;  // the first step of a merge flips, the rest disperse
                for (uint64_t i = threadIdx.x; i < n; i += kThreads) {
                    const uint64_t l = i ^ mask;
                    if (l > i && l < n) {
                        const uint32_t x = v[i], y = v[l];
                        if (x > y) v[i] = y, v[l] = x;
                    }
                }
                __syncthreads();
            }
        }
    }
}

struct IndexView {
    const uint32_t *row, *to;
    uint32_t n_segs;
};

// Is (a, b) a link or the reverse complement of one (validate.py:16-19)?  Both handles name segments below n_segs.
__device__ __forceinline__ bool supported(const IndexView &ix, uint32_t a, uint32_t b) {
    const uint64_t key = canon(a, b);
    const uint32_t h = (uint32_t)(key >> 32), want = (uint32_t)key;
    uint32_t lo = ix.row[h], hi = ix.row[h + 1];
    if (hi - lo <= kLinear) {
        for (; lo < hi; ++lo)
            if (ix.to[lo] == want) return true;
        return false;
    }
    while (lo < hi) {  // the first entry at or above want
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (ix.to[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    return lo < ix.row[h + 1] && ix.to[lo] == want;
}

template <bool kApply>
__global__ __launch_bounds__(kThreads) void k_steps(IndexView ix, TopoSteps sp, uint64_t n_tiles, Sum<uint64_t> *aggr, const uint64_t *__restrict__ prefix,
                                                    uint4 *__restrict__ recs, uint32_t *flags) {
    __shared__ Sum<uint32_t> sh[kThreads];
    __shared__ uint32_t ends[2];
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        if (kApply && !aggr[tile].v) continue;  // (the same for every lane)
        const uint64_t t0 = tile * kTile, t1 = min(t0 + kTile, sp.n_lin);
        if (threadIdx.x < 2) ends[threadIdx.x] = last_start_at_or_before(sp.pstart, 0, sp.n_paths - 1, threadIdx.x ? t1 - 1 : t0);
        __syncthreads();
        const uint64_t base = t0 + (uint64_t)threadIdx.x * kPer;
        uint4 rec[kPer];
        uint32_t miss = 0;  // bit q: this lane's step q has an unsupported pair
        if (base < t1) {
            uint32_t p = last_start_at_or_before(sp.pstart, ends[0], ends[1], base);
            uint64_t ps = sp.pstart[p], pe = sp.pstart[p + 1], pb = sp.pbegin[p];
#pragma unroll
            for (uint32_t q = 0; q < kPer; ++q) {
                const uint64_t j = base + q;
                if (j >= t1) break;
                while (j >= pe) {  // (j < n_lin = pstart[n_paths]: this ends at a path that is not empty)
                    ++p;
                    ps = pe, pe = sp.pstart[p + 1], pb = sp.pbegin[p];
                }
                const uint64_t at = pb + (j - ps);
                const uint32_t a = sp.steps[at];
                if ((a >> 1) >= ix.n_segs) {
                    atomicOr(flags, kBadStep);
                    continue;
                }
                if (j + 1 >= pe) continue;  // the path's last step: no pair, and none with the next path's first
                const uint32_t b = sp.steps[at + 1];
                if ((b >> 1) >= ix.n_segs) continue;  // (flagged by its own lane)
                if (!supported(ix, a, b)) {
                    rec[q] = make_uint4(p, (uint32_t)(j - ps), a, b);
                    miss |= 1u << q;
                }
            }
        }
        block_scan<kThreads>(sh, Sum<uint32_t>{(uint32_t)__popc(miss)});
        if (!kApply) {
            if (threadIdx.x == kThreads - 1) aggr[tile].v = sh[kThreads - 1].v;
        } else {
            uint64_t at = prefix[tile] + (threadIdx.x ? sh[threadIdx.x - 1].v : 0u);
#pragma unroll
            for (uint32_t q = 0; q < kPer; ++q)
                if ((miss >> q) & 1u) recs[at++] = rec[q];
        }
        __syncthreads();  // (sh and ends are written again in the next round)
    }
}

}  // namespace

#define TP_HIP(expr) FGFA_HIP("topology: ", expr)

void topo_index_free(TopoIndex *ix) {
    if (ix->mem) (void)hipFree(ix->mem);
    *ix = TopoIndex();
}

int topo_index_build(const uint32_t *links, uint64_t L, uint32_t S, hipStream_t st, TopoIndex *out) {
    *out = TopoIndex();
    if (L > 0xFFFFFFFFull || S > 0x7FFFFFFFu) {
        set_error("topology: graph too large for 32-bit ids");
        return FLATGFA_ERR_TOO_LARGE;
    }
    const uint64_t n_rows = 2 * (uint64_t)S, n_scan = n_rows + 1, tiles = blocks(n_scan, kTile);
    // row[2 S + 1] (and one word of padding), to[L], deg[S]: one allocation, kept with the handle
    const uint64_t words = (n_scan + 1) + std::max<uint64_t>(L, 1) + std::max<uint64_t>(S, 1);
    uint32_t *mem = nullptr;
    TP_HIP(hipMalloc((void **)&mem, words * 4));
    TopoIndex ix;
    ix.mem = mem;
    ix.row = mem;
    ix.to = mem + (n_scan + 1);
    ix.deg = ix.to + std::max<uint64_t>(L, 1);
    ix.n_segs = S;
    ix.n_links = L;
    struct Guard {  // (the index goes back unless it is handed out)
        TopoIndex *ix;
        ~Guard() { if (ix) topo_index_free(ix); }
    } guard{&ix};
    DeviceMem sc;
    sc.st = st;
    uint32_t *cursor = nullptr, *list = nullptr, *words4 = nullptr;
    Spine<Sum<uint32_t>> rows;
    const uint64_t list_cap = L / (kLinear + 1) + 1;  // (a listed row holds more than kLinear of the L entries)
    TP_HIP(sc.alloc(&cursor, n_rows));
    TP_HIP(sc.alloc(&list, list_cap));
    TP_HIP(sc.alloc(&words4, 4));  // flags, long-row count
    TP_HIP(rows.alloc(&sc, tiles));
    TP_HIP(hipMemsetAsync(mem, 0, words * 4, st));
    TP_HIP(hipMemsetAsync(cursor, 0, std::max<uint64_t>(n_rows, 1) * 4, st));
    TP_HIP(hipMemsetAsync(words4, 0, 16, st));
    if (L) hipLaunchKernelGGL(k_link_count, dim3(stride_blocks(L, kThreads, kMaxGrid)), dim3(kThreads), 0, st, links, L, S, ix.row, ix.deg, words4);
    scan_count<kThreads, kPer>(RowOp{ix.row}, n_scan, rows, st);
    scan_apply<kThreads, kPer>(RowOp{ix.row}, n_scan, rows, st);
    if (L) {
        hipLaunchKernelGGL(k_link_scatter, dim3(stride_blocks(L, kThreads, kMaxGrid)), dim3(kThreads), 0, st, links, L, S, ix.row, cursor, ix.to);
        hipLaunchKernelGGL(k_long_rows, dim3(stride_blocks(n_rows, kThreads, kMaxGrid)), dim3(kThreads), 0, st, ix.row, n_rows, list, (uint32_t)list_cap,
                           words4 + 1);
    }
    TP_HIP(hipGetLastError());
    uint32_t host[4] = {0, 0, 0, 0};
    TP_HIP(staged_copy(host, words4, 16, hipMemcpyDeviceToHost, st));
    if (host[0] & kBadLink) {
        set_error("topology: a link refers to a segment id that is out of range");
        return FLATGFA_ERR_BOUNDS;
    }
    const uint32_t n_long = (uint32_t)std::min<uint64_t>(host[1], list_cap);
    if (n_long) {
        hipLaunchKernelGGL(k_sort_rows, dim3(std::min(n_long, kMaxGrid)), dim3(kThreads), 0, st, ix.row, ix.to, list, n_long);
        TP_HIP(hipGetLastError());
        TP_HIP(hipStreamSynchronize(st));
    }
    *out = ix;
    guard.ix = nullptr;
    return FLATGFA_OK;
}

int topo_degree(const TopoIndex &ix, hipStream_t st, uint64_t *out) {
    if (!ix.n_segs) return FLATGFA_OK;
    std::vector<uint32_t> d(ix.n_segs);
    TP_HIP(staged_copy(d.data(), ix.deg, (size_t)ix.n_segs * 4, hipMemcpyDeviceToHost, st));
    for (size_t s = 0; s < d.size(); ++s) out[s] = d[s];
    return FLATGFA_OK;
}

struct ValidateJob {
    DeviceMem sc;
    IndexView ix{};
    TopoSteps sp;
    uint64_t tiles = 0, total = 0;
    Spine<Sum<uint32_t>> pairs;  // missing pairs per tile of steps
    uint32_t *flags = nullptr;
    bool counted = false;
};

ValidateJob *validate_new() { return new ValidateJob(); }
void validate_free(ValidateJob *j) { delete j; }

int validate_count(ValidateJob *j, const TopoIndex &ix, const TopoSteps &sp, hipStream_t st, uint64_t *n) {
    *n = 0;
    j->sc.st = st;
    j->ix = IndexView{ix.row, ix.to, ix.n_segs};
    j->sp = sp;
    j->tiles = blocks(sp.n_lin, kTile);
    j->total = 0;
    j->counted = !sp.n_lin;
    if (!sp.n_lin) return FLATGFA_OK;  // (no path has a step)
    TP_HIP(j->pairs.alloc(&j->sc, j->tiles));
    TP_HIP(j->sc.alloc(&j->flags, 1));
    TP_HIP(hipMemsetAsync(j->flags, 0, 4, st));
    hipLaunchKernelGGL((k_steps<false>), dim3(stride_blocks(j->tiles, 1, kMaxGrid)), dim3(kThreads), 0, st, j->ix, sp, j->tiles, j->pairs.aggr,
                       j->pairs.prefix, (uint4 *)nullptr, j->flags);
    hipLaunchKernelGGL((k_spine<Sum<uint64_t>, kThreads>), dim3(1), dim3(kThreads), 0, st, j->pairs.aggr, j->tiles, j->pairs.prefix, j->pairs.total);
    TP_HIP(hipGetLastError());
    uint32_t f = 0;
    TP_HIP(staged_copy(&f, j->flags, 4, hipMemcpyDeviceToHost, st));
    TP_HIP(staged_copy(&j->total, j->pairs.total, 8, hipMemcpyDeviceToHost, st));
    if (f & kBadStep) {
        set_error("topology: a step refers to a segment id that is out of range");
        return FLATGFA_ERR_BOUNDS;
    }
    j->counted = true;
    *n = j->total;
    return FLATGFA_OK;
}

int validate_fill(ValidateJob *j, flatgfa_missing_link_t *out) {
    if (!j->counted) { set_error("topology: fill before a successful count"); return FLATGFA_ERR_ARG; }
    if (!j->total) return FLATGFA_OK;
    if (!out) { set_error("topology: NULL output"); return FLATGFA_ERR_ARG; }
    static_assert(sizeof(flatgfa_missing_link_t) == sizeof(uint4), "a record is four words");
    hipStream_t st = j->sc.st;
    uint4 *recs = nullptr;
    TP_HIP(j->sc.alloc(&recs, j->total));
    hipLaunchKernelGGL((k_steps<true>), dim3(stride_blocks(j->tiles, 1, kMaxGrid)), dim3(kThreads), 0, st, j->ix, j->sp, j->tiles, j->pairs.aggr, j->pairs.prefix, recs,
                       j->flags);
    TP_HIP(hipGetLastError());
    TP_HIP(staged_copy(out, recs, (size_t)j->total * sizeof(uint4), hipMemcpyDeviceToHost, st));
    return FLATGFA_OK;
}

}  // namespace fgfa_dev
