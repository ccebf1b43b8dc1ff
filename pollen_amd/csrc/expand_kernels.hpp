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
//   k_path_lens, k_expand_paths   the per-path route for spans that do not tile the steps pool in order.
//
// Everything is in an unnamed namespace: each .hip file that includes this gets its own kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

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
constexpr uint32_t kNonTiling = 1, kBadSpan = 2, kBadStep = 4, kBadLink = 8;

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

}  // namespace
}  // namespace fgfa_dev
