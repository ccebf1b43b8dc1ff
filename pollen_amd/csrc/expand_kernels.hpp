// The count / scan / expansion kernels that chop (chop_device.hip) and inject (inject_device.hip, section
// 16) share: a piece count per element, a ticketed reduction, tile prefixes, and an expansion load-balanced by output tile.
// The two features differ in one thing only, where the piece count of a segment comes from: a functor Pc with
// pc(s) = the pieces of segment s (chop: from its length and c; inject: from its row of the cut table).
//
//   k_reduce     one workgroup per 16 tiles of 256 elements: each tile's sum of piece counts (u64), the workgroup's sum; the
//                last workgroup to finish (a ticket) scans the workgroup sums and writes the total.
//   k_prefix     each tile's exclusive prefix, from its workgroup's and the tile sums before it in the workgroup.
//   k_offsets    a tile's elements' exclusive prefixes (seg_first; the new path spans when they are laid out per path).
//   k_map        for each output tile of 2048 items, the source tile its first item comes from (a binary search of the prefixes).
//   k_expand     one workgroup per output tile: the source tiles that cover it (at most 10: every element has at least one
//                piece) are scanned again into LDS, each lane finds its first source element by a binary search there and
//                emits 8 consecutive items, and the tile goes out through LDS in coalesced rows.
//   k_path_spans a wave per path: the new span [O(begin), O(end)) where O(v) = prefix of v's tile + the pieces of the at most
//                255 steps before v in it.
//   k_path_lens, k_expand_paths   the per-path route for spans that do not tile the steps pool in order (the types allow any
//                spans, overlapping ones included): k_path_lens sums each path's pieces, k_offsets lays the paths out,
//                k_expand_paths writes each path with one workgroup (all its lanes on a long step).
//
// The host code that drives them is here too, once ("the expansion driver", below the kernels): the Expansion that a job of
// either feature holds and the functions that check the arguments, lay out the scratch, launch the reduces, read the totals
// (the host reads them -- new segments, new steps -- checks them against the u32 id space, and only then is anything written)
// and fill; templated on Pc and on the pair Load / Emit that makes the new segments' records.  A feature's .hip file says
// what is its own and calls them in order.
//
// Everything is in an unnamed namespace: each .hip file that includes this gets its own kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "chop_device.hpp"
#include "device_common.hpp"
#include "device_scan.hpp"
#include "prof.hpp"

namespace fgfa_dev {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTile = 256;           // source elements per tile
constexpr uint32_t kTilesPerWg = 16;      // tiles per k_reduce workgroup
constexpr uint32_t kItems = 8;            // output items per lane of k_expand
constexpr uint32_t kOutTile = kThreads * kItems;
constexpr uint32_t kRMax = kOutTile / kTile + 2;  // source tiles that can cover one output tile

// flag word bits
constexpr uint32_t kNonTiling = 1, kBadSpan = 2, kBadStep = 4, kBadLink = 8, kBadPath = 16;  // (kBadPath: inject's lines)

// ---- piece counts ----
template <class Pc>
struct SegCountT {
    Pc pc;
    __device__ uint64_t operator()(uint64_t i) const { return pc((uint32_t)i); }
};
template <class Pc>
struct StepCountT {  // the steps pool as one sequence (the spans tile it); nothing when they do not
    const uint32_t *steps;
    uint32_t n_segs;
    Pc pc;
    uint32_t *flags;
    __device__ uint64_t operator()(uint64_t i) const {
        if (*flags & kNonTiling) return 0;
        const uint32_t s = steps[i] >> 1;
        if (s >= n_segs) {
            atomicOr(flags, kBadStep);
            return 1;
        }
        return pc(s);
    }
};
struct ArrCount {
    const uint64_t *a;
    __device__ uint64_t operator()(uint64_t i) const { return a[i]; }
};

template <class Src>
__global__ __launch_bounds__(kThreads) void k_reduce(Src src, uint64_t n, uint64_t *__restrict__ tile_sum, uint64_t *wg, uint32_t n_wg,
                                                     uint32_t *ticket, uint64_t *total_out) {
    __shared__ uint64_t ts[kTilesPerWg];
    __shared__ uint32_t last;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t n_tiles = (n + kTile - 1) / kTile;
    for (uint32_t r = wave; r < kTilesPerWg; r += kThreads / 64) {
        const uint64_t t = (uint64_t)blockIdx.x * kTilesPerWg + r, base = t * kTile;
        uint64_t s = 0;
#pragma unroll
        for (uint32_t q = 0; q < kTile / 64; ++q) {
            const uint64_t i = base + q * 64 + lane;
            if (i < n) s += src(i);
        }
        s = wave_sum(s);
        if (lane == 0) {
            ts[r] = s;
            if (t < n_tiles) tile_sum[t] = s;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t s = 0;
        for (uint32_t r = 0; r < kTilesPerWg; ++r) s += ts[r];
        // Workgroups sit on different XCDs, whose L2s do not see each other's lines within a kernel: the sums are written and read
        // with device-scope accesses, the write is waited for, and only then is the ticket taken (as depth_accum.hip's pairs do).
        __hip_atomic_store(wg + blockIdx.x, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == n_wg - 1;
    }
    __syncthreads();
    if (!last) return;
    uint64_t carry = 0;
    for (uint32_t b = 0; b < n_wg; b += kThreads) {
        const uint32_t i = b + threadIdx.x;
        const uint64_t v = i < n_wg ? __hip_atomic_load(wg + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        uint64_t tot;
        const uint64_t ex = block_excl_scan<uint64_t, kThreads>(v, &tot);
        if (i < n_wg) wg[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) {
        wg[n_wg] = carry;
        *total_out = carry;
        *ticket = 0;
    }
}

__global__ __launch_bounds__(kThreads) void k_prefix(const uint64_t *__restrict__ tile_sum, const uint64_t *__restrict__ wg, uint64_t n_tiles,
                                                     uint32_t n_wg, uint64_t *__restrict__ prefix) {
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= n_tiles) return;
    const uint64_t w = t / kTilesPerWg;
    uint64_t s = wg[w];
    for (uint64_t u = w * kTilesPerWg; u < t; ++u) s += tile_sum[u];
    prefix[t] = s;
    if (t == n_tiles - 1) prefix[n_tiles] = wg[n_wg];
}

template <class Src, class Writer>
__global__ __launch_bounds__(kThreads) void k_offsets(Src src, uint64_t n, const uint64_t *__restrict__ prefix, Writer wr) {
    const uint64_t i = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    const uint64_t cnt = i < n ? src(i) : 0;
    uint64_t tot;
    const uint64_t ex = block_excl_scan<uint64_t, kThreads>(cnt, &tot);
    if (i < n) wr(i, n, prefix[blockIdx.x] + ex, cnt);
}
struct SegFirstWriter {
    uint32_t *seg_first;
    __device__ void operator()(uint64_t i, uint64_t n, uint64_t ex, uint64_t cnt) const {
        seg_first[i] = (uint32_t)ex;
        if (i == n - 1) seg_first[n] = (uint32_t)(ex + cnt);
    }
};
struct PathWriter {
    uint32_t *begin, *end;
    __device__ void operator()(uint64_t i, uint64_t, uint64_t ex, uint64_t cnt) const {
        begin[i] = (uint32_t)ex;
        end[i] = (uint32_t)(ex + cnt);
    }
};

__global__ __launch_bounds__(kThreads) void k_map(const uint64_t *__restrict__ prefix, uint64_t n_tiles, uint64_t n_out_tiles,
                                                  uint32_t *__restrict__ map) {
    const uint64_t o = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (o >= n_out_tiles) return;
    const uint64_t j0 = o * kOutTile;
    uint64_t lo = 0, hi = n_tiles;  // the last tile whose prefix is <= j0
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (prefix[mid] <= j0) lo = mid;
        else hi = mid;
    }
    map[o] = (uint32_t)lo;
}

// ---- expansion ----
// New segment jj is piece p of k of old segment i: its record (sequence [start, start + plen) of the old seq_data) and, when it
// is not the last piece, the forward link behind it.  Either array may be NULL.
__device__ __forceinline__ void write_piece(uint32_t *recs, uint32_t *links, uint64_t jj, uint64_t i, uint32_t start, uint64_t plen, uint32_t p,
                                            uint32_t k) {
    if (recs) {
        uint32_t *r = recs + jj * 6;  // Segment: name u64, seq span, optional span (chop.rs:29-35, 45-58)
        r[0] = (uint32_t)(jj + 1);
        r[1] = 0;
        r[2] = start;
        r[3] = (uint32_t)(start + plen);
        r[4] = 0;
        r[5] = 0;
    }
    if (links && p + 1 < k) {  // link_forward (chop.rs:14-22): link jj - i, among the S' - S of them
        uint32_t *l = links + (jj - i) * 4;
        l[0] = (uint32_t)jj << 1;
        l[1] = (uint32_t)(jj + 1) << 1;
        l[2] = 0;
        l[3] = 0;
    }
}
struct StepLoad {
    const uint32_t *steps, *seg_first;
    uint32_t n_segs;
    __device__ void operator()(uint64_t i, uint32_t *cnt, uint32_t *a, uint32_t *b) const {
        const uint32_t h = steps[i], s = h >> 1;
        uint32_t base = 0, k = 1;  // (an id out of range was reported by the count; it takes one item here)
        if (s < n_segs) {
            base = seg_first[s];
            k = seg_first[s + 1] - base;
        }
        *cnt = k;
        *a = h;
        *b = base;
    }
};
struct StepEmit {  // chop.rs:80-101: forward first..first+k, backward the same ids reversed
    __device__ uint32_t operator()(uint64_t, uint64_t, uint32_t h, uint32_t base, uint32_t p, uint32_t k) const {
        return (h & 1u) ? (((base + k - 1 - p) << 1) | 1u) : ((base + p) << 1);
    }
};

template <class Load, class Emit>
__global__ __launch_bounds__(kThreads) void k_expand(Load ld, Emit em, uint64_t n, const uint64_t *__restrict__ prefix, uint64_t n_tiles,
                                                     const uint32_t *__restrict__ map, uint64_t total, uint32_t *__restrict__ dst) {
    __shared__ uint32_t off[kRMax * kTile], pa[kRMax * kTile], pb[kRMax * kTile];
    __shared__ uint32_t stage[kThreads * (kItems + 1)];
    const uint64_t j0 = (uint64_t)blockIdx.x * kOutTile, j1 = min(j0 + kOutTile, total);
    const uint64_t t0 = map[blockIdx.x];
    uint32_t R = 1;
    while (R < kRMax && t0 + R < n_tiles && prefix[t0 + R] < j1) ++R;
    for (uint32_t r = 0; r < R; ++r) {
        const uint64_t i = (t0 + r) * kTile + threadIdx.x;
        uint32_t cnt = 0, a = 0, b = 0;
        if (i < n) ld(i, &cnt, &a, &b);
        uint32_t tot;
        const uint32_t ex = block_excl_scan<uint32_t, kThreads>(cnt, &tot);
        off[r * kTile + threadIdx.x] = (uint32_t)prefix[t0 + r] + ex;
        pa[r * kTile + threadIdx.x] = a;
        pb[r * kTile + threadIdx.x] = b;
    }
    const uint32_t m = (uint32_t)min<uint64_t>((uint64_t)R * kTile, n - t0 * kTile);
    const uint32_t off_end = (uint32_t)prefix[t0 + R];
    __syncthreads();
    const uint64_t j = j0 + (uint64_t)threadIdx.x * kItems;
    uint32_t vals[kItems];
#pragma unroll
    for (uint32_t q = 0; q < kItems; ++q) vals[q] = 0;
    if (j < j1) {
        const uint32_t jr = (uint32_t)j;  // (every offset is below 2^32: the count checked the total)
        uint32_t lo = 0, hi = m;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (off[mid] <= jr) lo = mid;
            else hi = mid;
        }
        uint32_t e = lo;
#pragma unroll
        for (uint32_t q = 0; q < kItems; ++q) {
            const uint32_t jj = jr + q;
            if (j + q < j1) {
                while (e + 1 < m && off[e + 1] <= jj) ++e;
                const uint32_t next = e + 1 < m ? off[e + 1] : off_end;
                vals[q] = em(j + q, t0 * kTile + e, pa[e], pb[e], jj - off[e], next - off[e]);
            }
        }
    }
    if (!dst) return;
#pragma unroll
    for (uint32_t q = 0; q < kItems; ++q) stage[threadIdx.x * (kItems + 1) + q] = vals[q];
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < kItems; ++q) {
        const uint32_t x = q * kThreads + threadIdx.x;
        if (j0 + x < j1) dst[j0 + x] = stage[(x / kItems) * (kItems + 1) + x % kItems];
    }
}

// ---- paths ----
__global__ __launch_bounds__(kThreads) void k_check_spans(const uint32_t *__restrict__ pb, const uint32_t *__restrict__ pe, uint32_t n_paths,
                                                          uint64_t n_steps, uint32_t *flags) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n_paths) return;
    const uint32_t b = pb[p], e = pe[p];
    uint32_t f = 0;
    if (b > e || e > n_steps) f |= kBadSpan;
    if (b != (p ? pe[p - 1] : 0u) || (p == n_paths - 1 && e != n_steps)) f |= kNonTiling;
    if (f) atomicOr(flags, f);
}

// a span clamped into the pool (a bad one was reported by k_check_spans)
__device__ __forceinline__ void clamp_span(uint32_t b, uint32_t e, uint64_t n, uint64_t *cb, uint64_t *ce) {
    *cb = min<uint64_t>(b, n);
    *ce = max<uint64_t>(*cb, min<uint64_t>(e, n));
}

// pieces of the steps [b, e) of a path, by one workgroup (non-tiling spans only)
template <class Pc>
__global__ __launch_bounds__(kThreads) void k_path_lens(const uint32_t *__restrict__ steps, const uint32_t *__restrict__ pb,
                                                        const uint32_t *__restrict__ pe, uint32_t n_paths, uint64_t n_steps, Pc pc,
                                                        uint32_t n_segs, uint32_t *flags, uint64_t *__restrict__ plen) {
    if (!(*flags & kNonTiling)) return;
    __shared__ uint64_t ws[kThreads / 64];
    for (uint32_t p = blockIdx.x; p < n_paths; p += gridDim.x) {
        uint64_t b, e;
        clamp_span(pb[p], pe[p], n_steps, &b, &e);
        uint64_t s = 0;
        bool bad = false;
        for (uint64_t i = b + threadIdx.x; i < e; i += kThreads) {
            const uint32_t sg = steps[i] >> 1;
            if (sg < n_segs) s += pc(sg);
            else bad = true, s += 1;
        }
        if (bad) atomicOr(flags, kBadStep);
        s = wave_sum(s);
        if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) plen[p] = ws[0] + ws[1] + ws[2] + ws[3];
        __syncthreads();
    }
}

__device__ __forceinline__ uint32_t step_pieces(const uint32_t *steps, const uint32_t *seg_first, uint32_t n_segs, uint64_t i) {
    const uint32_t s = steps[i] >> 1;
    return s < n_segs ? seg_first[s + 1] - seg_first[s] : 1u;
}

// new spans of tiling paths: [O(begin), O(end)), a wave per path
__global__ __launch_bounds__(kThreads) void k_path_spans(const uint32_t *__restrict__ steps, const uint32_t *__restrict__ pb,
                                                         const uint32_t *__restrict__ pe, uint32_t n_paths, uint64_t n_steps,
                                                         const uint32_t *__restrict__ seg_first, uint32_t n_segs,
                                                         const uint64_t *__restrict__ prefix, uint32_t *__restrict__ out_b,
                                                         uint32_t *__restrict__ out_e) {
    const uint32_t p = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= n_paths) return;
    uint64_t b, e;
    clamp_span(pb[p], pe[p], n_steps, &b, &e);
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const uint64_t v = side ? e : b, t = v / kTile;
        uint64_t s = 0;
        for (uint64_t i = t * kTile + lane; i < v; i += 64) s += step_pieces(steps, seg_first, n_segs, i);
        s = wave_sum(s);
        if (lane == 0) (side ? out_e : out_b)[p] = (uint32_t)(prefix[t] + s);
    }
}

// non-tiling paths: one workgroup per path writes its expansion at out_b[p]
__global__ __launch_bounds__(kThreads) void k_expand_paths(const uint32_t *__restrict__ steps, const uint32_t *__restrict__ pb,
                                                           const uint32_t *__restrict__ pe, uint32_t n_paths, uint64_t n_steps,
                                                           const uint32_t *__restrict__ seg_first, uint32_t n_segs,
                                                           const uint32_t *__restrict__ out_b, uint32_t *__restrict__ dst) {
    __shared__ uint32_t off[kTile], pa[kTile], pbase[kTile];
    const StepEmit em;
    for (uint32_t p = blockIdx.x; p < n_paths; p += gridDim.x) {
        uint64_t b, e;
        clamp_span(pb[p], pe[p], n_steps, &b, &e);
        uint32_t obase = out_b[p];
        for (uint64_t cb = b; cb < e; cb += kTile) {
            const uint64_t i = cb + threadIdx.x;
            uint32_t cnt = 0, h = 0, base = 0;
            if (i < e) StepLoad{steps, seg_first, n_segs}(i, &cnt, &h, &base);
            uint32_t tot;
            const uint32_t ex = block_excl_scan<uint32_t, kThreads>(cnt, &tot);
            off[threadIdx.x] = ex;
            pa[threadIdx.x] = h;
            pbase[threadIdx.x] = base;
            const uint32_t m = (uint32_t)min<uint64_t>(kTile, e - cb);
            __syncthreads();
            // 64-bit: tot reaches 2^32 - 1, and a u32 ob would wrap from 2^32 - kOutTile to 0 and never end
            for (uint64_t ob = 0; ob < tot; ob += kOutTile) {
                const uint64_t j64 = ob + threadIdx.x * kItems;
                if (j64 < tot) {
                    const uint32_t j = (uint32_t)j64;
                    uint32_t lo = 0, hi = m;
                    while (hi - lo > 1) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if (off[mid] <= j) lo = mid;
                        else hi = mid;
                    }
                    uint32_t e2 = lo;
                    for (uint32_t q = 0; q < kItems && j64 + q < tot; ++q) {
                        const uint32_t jj = j + q;
                        while (e2 + 1 < m && off[e2 + 1] <= jj) ++e2;
                        const uint32_t next = e2 + 1 < m ? off[e2 + 1] : tot;
                        dst[(uint64_t)obase + jj] = em(0, 0, pa[e2], pbase[e2], jj - off[e2], next - off[e2]);
                    }
                }
            }
            obase += tot;
            __syncthreads();
        }
    }
}

// chop.rs:106-134: an old link remapped, behind the S' - S forward links
__global__ __launch_bounds__(kThreads) void k_links(const uint32_t *__restrict__ links, uint64_t n_links, const uint32_t *__restrict__ seg_first,
                                                    uint32_t n_segs, uint32_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_links) return;
    const uint32_t f = links[i * 4], t = links[i * 4 + 1], fs = f >> 1, tsg = t >> 1;
    uint32_t nf = 0, nt = 0;
    if (fs < n_segs && tsg < n_segs) {  // (else reported by the count)
        const uint32_t fseg = (f & 1u) ? seg_first[fs] : seg_first[fs + 1] - 1;
        const uint32_t tseg = (t & 1u) ? seg_first[tsg + 1] - 1 : seg_first[tsg];
        nf = (fseg << 1) | (f & 1u);
        nt = (tseg << 1) | (t & 1u);
    }
    out[i * 4] = nf;
    out[i * 4 + 1] = nt;
    out[i * 4 + 2] = 0;  // the empty alignment (flatgfa.rs:494-500)
    out[i * 4 + 3] = 0;
}

// ---- host side ----
struct ScanBuf {
    uint64_t n = 0, n_tiles = 0;
    uint32_t n_wg = 0;
    uint64_t *tile_sum = nullptr, *wg = nullptr, *prefix = nullptr;
    uint32_t *ticket = nullptr;
    uint32_t *map = nullptr;
    uint64_t n_out_tiles = 0;
    static size_t words_for(uint64_t count) {
        const uint64_t t = (count + kTile - 1) / kTile, w = (t + kTilesPerWg - 1) / kTilesPerWg;
        return t + (w + 1) + (t + 1) + 1;
    }
    size_t words() const { return words_for(n); }
    void place(uint64_t count, uint64_t *&p) {
        n = count;
        n_tiles = (n + kTile - 1) / kTile;
        n_wg = (uint32_t)((n_tiles + kTilesPerWg - 1) / kTilesPerWg);
        tile_sum = p;
        wg = tile_sum + n_tiles;
        prefix = wg + n_wg + 1;
        ticket = reinterpret_cast<uint32_t *>(prefix + n_tiles + 1);
        p += words();
    }
};

template <class Src>
void launch_reduce(const ScanBuf &sb, Src src, uint64_t *total_out, hipStream_t st, const char *name) {
    if (!sb.n) return;  // (the total stays 0 from the memset)
    ProfScope ps(name, st);
    hipLaunchKernelGGL(k_reduce<Src>, dim3(sb.n_wg), dim3(kThreads), 0, st, src, sb.n, sb.tile_sum, sb.wg, sb.n_wg, sb.ticket, total_out);
}
void launch_prefix(const ScanBuf &sb, hipStream_t st) {
    if (!sb.n) return;  // (prefix[0] = 0 from the memset)
    hipLaunchKernelGGL(k_prefix, dim3((uint32_t)blocks(sb.n_tiles, kThreads)), dim3(kThreads), 0, st, sb.tile_sum, sb.wg, sb.n_tiles, sb.n_wg, sb.prefix);
}
void launch_map(const ScanBuf &sb, hipStream_t st) {
    if (!sb.n_out_tiles) return;
    hipLaunchKernelGGL(k_map, dim3((uint32_t)blocks(sb.n_out_tiles, kThreads)), dim3(kThreads), 0, st, sb.prefix, sb.n_tiles, sb.n_out_tiles, sb.map);
}

// ---- the expansion driver ----
// What a feature is called in its messages and in the profile (literals: ProfRec keeps the pointers).
struct ExpandNames {
    const char *prefix, *noun;  // "chop: ", "chopped graph"
    const char *reduce_segs, *reduce_steps, *reduce_paths, *expand_steps, *expand_paths, *expand_segs;
};

// One count-and-fill job over a graph: what chop and inject both hold.  A feature's count calls expand_check_args,
// expand_begin, expand_check_graph, expand_reduce<Pc> and expand_totals<Pc> in this order, and its fill calls
// expand_fill<Load, Emit>, with the launches of its own between them (inject: the cut table before the reduces, the lines'
// lengths behind them, the new paths behind the fill).  The count waits for its stream once, in expand_totals; nothing else
// waits.  Kernels never trap: a bad span, step, link or path id raises a bit of the flag word that expand_totals reads.
struct Expansion {
    ChopIn in;
    bool links = false, counted = false, tiling = true;
    uint32_t *seg_first = nullptr;
    uint64_t S2 = 0, N_old2 = 0, N_add = 0, L2 = 0;  // new segments, the old paths' new steps, the added paths' steps, new links
    DeviceMem dm;                                    // (waits for the last stream used, then frees)
    uint64_t *hdr = nullptr;  // [0] flags, [1] new segments, [2] old paths' new steps (tiling), [3] (per path), [4] the added paths' steps
    uint64_t *plen = nullptr;
    uint32_t *maps = nullptr;
    ScanBuf seg, step, path;
    uint64_t N2() const { return N_old2 + N_add; }
};

inline int expand_refuse(const ExpandNames &nm, const char *what, int code) {
    set_error(std::string(nm.prefix) + what);
    return code;
}

// `own_null`: an argument of the feature's own is missing
int expand_check_args(const ExpandNames &nm, const ChopIn &in, bool links, const uint32_t *seg_first, bool own_null) {
    if ((in.n_segs && (!in.seg_len || !seg_first)) || (in.n_steps && !in.steps) || (in.n_paths && (!in.path_begin || !in.path_end)) ||
        (links && in.n_links && !in.links) || own_null)
        return expand_refuse(nm, "NULL argument", FLATGFA_ERR_ARG);
    if (in.n_steps > 0xFFFFFFFFull || in.n_segs > 0x80000000u) return expand_refuse(nm, "graph too large for 32-bit ids", FLATGFA_ERR_TOO_LARGE);
    return FLATGFA_OK;
}

// One zeroed allocation for the scans' scratch: header, segments, steps, paths, per-path lengths, then `extra_words` of the
// feature's own, at *extra.
int expand_begin(Expansion &x, const ExpandNames &nm, const ChopIn &in, bool links, uint32_t *seg_first, hipStream_t st, size_t extra_words = 0,
                 uint64_t **extra = nullptr) {
    if (x.counted) return expand_refuse(nm, "this job was counted already", FLATGFA_ERR_ARG);
    x.in = in;
    x.links = links;
    x.seg_first = seg_first;
    x.dm.st = st;
    const size_t words = 8 + ScanBuf::words_for(in.n_segs) + ScanBuf::words_for(in.n_steps) + ScanBuf::words_for(in.n_paths) + in.n_paths + extra_words;
    uint64_t *p = nullptr;
    FGFA_HIP(nm.prefix, x.dm.alloc(&p, words));
    FGFA_HIP(nm.prefix, hipMemsetAsync(p, 0, words * 8, st));
    x.hdr = p;
    p += 8;
    x.seg.place(in.n_segs, p);
    x.step.place(in.n_steps, p);
    x.path.place(in.n_paths, p);
    x.plen = p;
    if (extra) *extra = p + in.n_paths;
    return FLATGFA_OK;
}

// the spans and the links
int expand_check_graph(Expansion &x, const ExpandNames &nm, hipStream_t st) {
    const ChopIn &in = x.in;
    uint32_t *flags = reinterpret_cast<uint32_t *>(x.hdr);
    if (in.n_paths == 0) FGFA_HIP(nm.prefix, hipMemsetAsync(flags, kNonTiling, 1, st));  // (no path: the pool is not walked)
    if (in.n_paths)
        hipLaunchKernelGGL(k_check_spans, dim3((uint32_t)blocks(in.n_paths, kThreads)), dim3(kThreads), 0, st, in.path_begin, in.path_end, in.n_paths,
                           in.n_steps, flags);
    if (x.links && in.n_links)
        hipLaunchKernelGGL(k_check_links<kThreads>, dim3((uint32_t)blocks(in.n_links, kThreads)), dim3(kThreads), 0, st, in.links, in.n_links, in.n_segs,
                           flags, kBadLink);
    return FLATGFA_OK;
}

// the piece counts of the segments, of the steps pool and (for spans that do not tile it) of each path
template <class Pc>
void expand_reduce(Expansion &x, const ExpandNames &nm, const Pc &pc, hipStream_t st) {
    const ChopIn &in = x.in;
    uint32_t *flags = reinterpret_cast<uint32_t *>(x.hdr);
    launch_reduce(x.seg, SegCountT<Pc>{pc}, x.hdr + 1, st, nm.reduce_segs);
    launch_reduce(x.step, StepCountT<Pc>{in.steps, in.n_segs, pc, flags}, x.hdr + 2, st, nm.reduce_steps);
    if (in.n_paths) {
        hipLaunchKernelGGL(k_path_lens<Pc>, dim3(std::min<uint32_t>(in.n_paths, 4096)), dim3(kThreads), 0, st, in.steps, in.path_begin, in.path_end,
                           in.n_paths, in.n_steps, pc, in.n_segs, flags, x.plen);
        launch_reduce(x.path, ArrCount{x.plen}, x.hdr + 3, st, nm.reduce_paths);
    }
}

// Waits for the totals (the count's one host synchronization), checks the flags and then the totals against the u32 id
// space, and only then allocates the tile maps of the two expansions and enqueues the write of seg_first.
template <class Pc>
int expand_totals(Expansion &x, const ExpandNames &nm, const Pc &pc, hipStream_t st, uint64_t *n_new_segs, uint64_t *n_new_steps,
                  uint64_t *n_new_links) {
    const ChopIn &in = x.in;
    FGFA_HIP(nm.prefix, hipGetLastError());
    uint64_t h[5];
    FGFA_HIP(nm.prefix, hipMemcpyAsync(h, x.hdr, sizeof h, hipMemcpyDeviceToHost, st));
    FGFA_HIP(nm.prefix, hipStreamSynchronize(st));
    const uint32_t f = (uint32_t)h[0];
    if (f & kBadSpan) return expand_refuse(nm, "a path has a step span outside the steps pool", FLATGFA_ERR_BOUNDS);
    if (f & kBadPath) return expand_refuse(nm, "a line names a path id that is out of range", FLATGFA_ERR_BOUNDS);
    if (f & kBadStep) return expand_refuse(nm, "a step refers to a segment id that is out of range", FLATGFA_ERR_BOUNDS);
    if (f & kBadLink) return expand_refuse(nm, "a link refers to a segment id that is out of range", FLATGFA_ERR_BOUNDS);
    x.tiling = !(f & kNonTiling);
    x.S2 = h[1];
    x.N_old2 = x.tiling ? h[2] : h[3];
    x.N_add = h[4];
    x.L2 = x.links ? x.S2 - in.n_segs + in.n_links : 0;
    // a handle is seg << 1 | orient in a u32; steps and links are counted in u32 (chop.rs through pool.rs Id)
    if (x.S2 >= 0x80000000ull || x.N_old2 > 0xFFFFFFFFull || x.N2() > 0xFFFFFFFFull || x.L2 > 0xFFFFFFFFull) {
        set_error(std::string(nm.prefix) + "the " + nm.noun + " would have " + std::to_string(x.S2) + " segments, " + std::to_string(x.N2()) +
                  " steps and " + std::to_string(x.L2) + " links: more than 32-bit ids hold");
        return FLATGFA_ERR_TOO_LARGE;
    }
    x.seg.n_out_tiles = (x.S2 + kOutTile - 1) / kOutTile;
    x.step.n_out_tiles = x.tiling ? (x.N_old2 + kOutTile - 1) / kOutTile : 0;
    const uint64_t mw = x.seg.n_out_tiles + x.step.n_out_tiles;
    if (mw) {
        FGFA_HIP(nm.prefix, x.dm.alloc(&x.maps, mw));
        x.seg.map = x.maps;
        x.step.map = x.maps + x.seg.n_out_tiles;
    }
    // seg_first, now that it fits
    if (in.n_segs) {
        launch_prefix(x.seg, st);
        hipLaunchKernelGGL((k_offsets<SegCountT<Pc>, SegFirstWriter>), dim3((uint32_t)x.seg.n_tiles), dim3(kThreads), 0, st, SegCountT<Pc>{pc},
                           (uint64_t)in.n_segs, x.seg.prefix, SegFirstWriter{x.seg_first});
    } else if (x.seg_first) {
        FGFA_HIP(nm.prefix, hipMemsetAsync(x.seg_first, 0, 4, st));
    }
    FGFA_HIP(nm.prefix, hipGetLastError());
    x.counted = true;
    *n_new_segs = x.S2;
    *n_new_steps = x.N2();
    if (n_new_links) *n_new_links = x.L2;
    return FLATGFA_OK;
}

// The old paths' steps and spans (by output tile when the spans tile the pool, per path when they do not), the new segments
// through the feature's Load / Emit pair, and the old links remapped.  `n_added`: the paths the feature writes behind the old.
template <class Load, class Emit>
int expand_fill(Expansion &x, const ExpandNames &nm, const Load &ld, const Emit &em, const ChopOut &out, uint64_t n_added, hipStream_t st) {
    if (!x.counted) return expand_refuse(nm, "fill before a successful count", FLATGFA_ERR_ARG);
    const ChopIn &in = x.in;
    if ((x.N2() && !out.steps) || ((in.n_paths || n_added) && (!out.path_begin || !out.path_end)) || (x.links && x.L2 && !out.links))
        return expand_refuse(nm, "NULL output", FLATGFA_ERR_ARG);
    x.dm.st = st;
    if (x.tiling) {
        launch_prefix(x.step, st);
        launch_map(x.step, st);
        if (x.N_old2) {
            ProfScope ps(nm.expand_steps, st);
            hipLaunchKernelGGL((k_expand<StepLoad, StepEmit>), dim3((uint32_t)x.step.n_out_tiles), dim3(kThreads), 0, st,
                               StepLoad{in.steps, x.seg_first, in.n_segs}, StepEmit{}, in.n_steps, x.step.prefix, x.step.n_tiles, x.step.map, x.N_old2,
                               out.steps);
        }
        if (in.n_paths)
            hipLaunchKernelGGL(k_path_spans, dim3((uint32_t)blocks(in.n_paths, kThreads / 64)), dim3(kThreads), 0, st, in.steps, in.path_begin, in.path_end,
                               in.n_paths, in.n_steps, x.seg_first, in.n_segs, x.step.prefix, out.path_begin, out.path_end);
    } else if (in.n_paths) {
        launch_prefix(x.path, st);
        hipLaunchKernelGGL((k_offsets<ArrCount, PathWriter>), dim3((uint32_t)x.path.n_tiles), dim3(kThreads), 0, st, ArrCount{x.plen},
                           (uint64_t)in.n_paths, x.path.prefix, PathWriter{out.path_begin, out.path_end});
        ProfScope ps(nm.expand_paths, st);
        hipLaunchKernelGGL(k_expand_paths, dim3(std::min<uint32_t>(in.n_paths, 4096)), dim3(kThreads), 0, st, in.steps, in.path_begin, in.path_end,
                           in.n_paths, in.n_steps, x.seg_first, in.n_segs, out.path_begin, out.steps);
    }
    if (x.S2) {
        launch_map(x.seg, st);
        ProfScope ps(nm.expand_segs, st);
        hipLaunchKernelGGL((k_expand<Load, Emit>), dim3((uint32_t)x.seg.n_out_tiles), dim3(kThreads), 0, st, ld, em, (uint64_t)in.n_segs, x.seg.prefix,
                           x.seg.n_tiles, x.seg.map, x.S2, out.seg_len);
    }
    if (x.links && in.n_links)
        hipLaunchKernelGGL(k_links, dim3((uint32_t)blocks(in.n_links, kThreads)), dim3(kThreads), 0, st, in.links, in.n_links, x.seg_first, in.n_segs,
                           out.links + (x.S2 - in.n_segs) * 4);
    FGFA_HIP(nm.prefix, hipGetLastError());
    return FLATGFA_OK;
}

// ---- the device-level C ABI's arguments (include/flatgfa.h Part 3) ----
inline ChopIn chop_in_of(const flatgfa_dev_graph_t &g) {
    ChopIn in;
    in.steps = g.steps;
    in.n_steps = g.n_steps;
    in.path_begin = g.path_begin;
    in.path_end = g.path_end;
    in.n_paths = g.n_paths;
    in.n_segs = g.n_segs;
    in.seg_len = g.seg_len;
    return in;
}
inline ChopOut chop_out_of(uint32_t *steps, uint32_t *path_begin, uint32_t *path_end, uint32_t *seg_len) {
    ChopOut out;
    out.steps = steps;
    out.path_begin = path_begin;
    out.path_end = path_end;
    out.seg_len = seg_len;
    return out;
}

}  // namespace
}  // namespace fgfa_dev
