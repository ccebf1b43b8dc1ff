// BED intersection on the device: bed_device.hpp says what is computed and why the pruning drops no hit.  DESIGN.md section 21.
//
//   k_bed_groups   one lane per B entry: where the groups begin, which of them are unsorted, and that B is grouped at all
//   RunMaxOp       runmax_end, the segmented inclusive max-scan (k_scan over MaxV: the maximum and a head flag)
//   k_bed_ranges   one lane per A entry: its candidate range [lo, lo + cand) by two bisections, or the whole group
//   k_bed_hits     one workgroup per tile of consecutive candidates, once to count the hits and once, behind the scan of the
//                  tiles' counts, to compact them in order (block_excl_scan, coalesced stores, no atomics)
//   k_bed_tiles    one workgroup per tile of output bytes: "name \t s \t e \n" per hit, formed in LDS, 16-byte stores
//
// The only atomics are the ORs of k_bed_groups and k_bed_ranges into the flag words.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/flatgfa.h"
#include "bed_device.hpp"
#include "device_common.hpp"
#include "device_scan.hpp"
#include "host_copy.hpp"
#include "prof.hpp"
#include "text_tiles.hpp"

namespace fgfa_dev {
namespace {

#define BED_HIP(expr) FGFA_HIP("bed: ", expr)

enum : uint32_t { kBadB = 1u, kBadA = 2u };

// ---- groups ----

// gstart is zeroed before (an empty B leaves it so); unsorted[g] != 0: group g has an entry that starts before its predecessor
__global__ __launch_bounds__(kBedThreads) void k_bed_groups(BedSide b, uint32_t n_groups, uint32_t *__restrict__ gstart,
                                                            uint32_t *__restrict__ unsorted, uint32_t *flags) {
    const uint64_t i = (uint64_t)blockIdx.x * kBedThreads + threadIdx.x;
    if (i >= b.n) return;
    const uint32_t id = b.id[i];
    if (id >= n_groups) {
        atomicOr(flags, kBadB);
        return;
    }
    if (i) {
        const uint32_t prev = b.id[i - 1];
        if (prev > id) {  // (B is not grouped; a predecessor at or past n_groups is flagged by its own lane)
            atomicOr(flags, kBadB);
            return;
        }
        for (uint32_t g = prev + 1; g <= id && prev != id; ++g) gstart[g] = (uint32_t)i;  // (the empty groups in between too)
        if (prev == id && b.start[i] < b.start[i - 1]) atomicOr(&unsorted[id], 1u);
    }
    if (i == b.n - 1)
        for (uint64_t g = (uint64_t)id + 1; g <= n_groups; ++g) gstart[g] = (uint32_t)b.n;
}

// a maximum, and whether a group's head lies in the stretch it covers: combined the way extract's SV is
struct MaxV {
    using Carry = uint64_t;
    using Wide = MaxV;
    uint64_t m;
    uint32_t f;
    __device__ __forceinline__ static MaxV zero() { return MaxV{0, 0u}; }
    __device__ __forceinline__ static MaxV comb(const MaxV &x, const MaxV &y) {
        if (y.f) return MaxV{y.m, 1u};
        return MaxV{x.m > y.m ? x.m : y.m, x.f};
    }
    __device__ __forceinline__ uint64_t carry() const { return m; }
    __device__ __forceinline__ static MaxV widen(const MaxV &x) { return x; }
    __device__ __forceinline__ static MaxV after(uint64_t c) { return MaxV{c, 0u}; }
};
struct RunMaxOp {
    BedSide b;
    uint64_t *runmax;
    __device__ __forceinline__ MaxV load(uint64_t i) const { return MaxV{b.end[i], (i == 0 || b.id[i] != b.id[i - 1]) ? 1u : 0u}; }
    __device__ __forceinline__ void store(uint64_t i, uint64_t before, const MaxV &me) const {
        runmax[i] = me.f || me.m > before ? me.m : before;
    }
};

// ---- candidates ----

struct Groups {
    const uint32_t *gstart, *unsorted;
    const uint64_t *runmax;
};

// the first i of [lo, hi) with a[i] > x (kAbove) or a[i] >= x; hi if there is none.  a does not decrease there.
template <bool kAbove>
__device__ __forceinline__ uint32_t first_past(const uint64_t *__restrict__ a, uint32_t lo, uint32_t hi, uint64_t x) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (kAbove ? a[mid] > x : a[mid] >= x) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(kBedThreads) void k_bed_ranges(BedInput in, Groups gr, uint32_t *__restrict__ lo_out, uint32_t *__restrict__ cand,
                                                            uint32_t *flags) {
    const uint64_t a = (uint64_t)blockIdx.x * kBedThreads + threadIdx.x;
    if (a >= in.a.n) return;
    const uint32_t id = in.a.id[a];
    const uint64_t as = in.a.start[a], ae = in.a.end[a];
    uint32_t lo = 0, n = 0;
    if (id != kBedNone && id >= in.n_groups) {
        atomicOr(flags, kBadA);
    } else if (id != kBedNone && as < ae) {
        const uint32_t g0 = gr.gstart[id], g1 = gr.gstart[id + 1];
        uint32_t hi = g1;
        lo = g0;
        if (!gr.unsorted[id]) {
            lo = first_past<true>(gr.runmax, g0, g1, as);
            hi = first_past<false>(in.b.start, g0, g1, ae);
        }
        n = hi > lo ? hi - lo : 0;  // (entries with start >= end may stand between hi and lo)
    }
    lo_out[a] = lo;
    cand[a] = n;
}

struct CandOp {
    const uint32_t *cand;
    uint64_t *prefix;
    __device__ __forceinline__ Sum<uint64_t> load(uint64_t a) const { return Sum<uint64_t>{cand[a]}; }
    __device__ __forceinline__ void store(uint64_t a, uint64_t before, const Sum<uint64_t> &) const { prefix[a] = before; }
};
struct UnsortedOp {
    const uint32_t *unsorted;
    __device__ __forceinline__ Sum<uint32_t> load(uint64_t g) const { return Sum<uint32_t>{unsorted[g] ? 1u : 0u}; }
    __device__ __forceinline__ void store(uint64_t, uint32_t, const Sum<uint32_t> &) const {}
};

// ---- rounds ----

// The tile of candidates [c0 + block * kBedCandTile, ...) of the round [c0, c0 + n).  !kFill: tile_hits[block] = its hits.
// kFill: the hits' records, in order, from tile_off[block] on.
template <bool kFill>
__global__ __launch_bounds__(kBedThreads) void k_bed_hits(BedInput in, const uint64_t *__restrict__ prefix, const uint32_t *__restrict__ lo,
                                                          uint64_t c0, uint64_t n, uint32_t *__restrict__ tile_hits,
                                                          const uint64_t *__restrict__ tile_off, BedHits out) {
    __shared__ uint64_t s_a[2];
    const uint64_t first = (uint64_t)blockIdx.x * kBedCandTile;
    const uint32_t tile_n = (uint32_t)min((uint64_t)kBedCandTile, n - first);
    const uint64_t base = c0 + first;
    if (threadIdx.x == 0) {  // the A entries that own the tile's first and last candidate
        s_a[0] = last_at_or_before(prefix, 0, in.a.n - 1, base);
        s_a[1] = last_at_or_before(prefix, s_a[0], in.a.n - 1, base + tile_n - 1);
    }
    __syncthreads();
    const uint64_t a0 = s_a[0], a1 = s_a[1];
    uint64_t running = kFill ? tile_off[blockIdx.x] : 0;
#pragma unroll 1
    for (uint32_t q = 0; q < kBedCandTile / kBedThreads; ++q) {
        const uint32_t k = q * kBedThreads + threadIdx.x;
        uint32_t hit = 0, bi = 0;
        uint64_t a = 0, s = 0, e = 0;
        if (k < tile_n) {
            const uint64_t c = base + k;
            a = last_at_or_before(prefix, a0, a1, c);  // (an entry without candidates is never the last at or before c)
            bi = lo[a] + (uint32_t)(c - prefix[a]);
            const uint64_t as = in.a.start[a], ae = in.a.end[a], bs = in.b.start[bi], be = in.b.end[bi];
            s = bs < as ? as : bs;
            e = ae < be ? ae : be;
            hit = e > s ? 1u : 0u;
        }
        uint32_t total = 0;
        const uint32_t at = block_excl_scan<uint32_t, kBedThreads>(hit, &total);
        if (kFill && hit) {
            const uint64_t w = running + at;
            out.a[w] = (uint32_t)a, out.b[w] = bi, out.s[w] = s, out.e[w] = e;
            if (out.len) out.len[w] = in.gname[2 * (uint64_t)in.b.id[bi] + 1] + digits10(s) + digits10(e) + 3;
        }
        running += total;
    }
    if (!kFill && threadIdx.x == 0) tile_hits[blockIdx.x] = (uint32_t)running;
}

struct TileOp {
    const uint32_t *tile_hits;
    uint64_t *tile_off;
    __device__ __forceinline__ Sum<uint64_t> load(uint64_t t) const { return Sum<uint64_t>{tile_hits[t]}; }
    __device__ __forceinline__ void store(uint64_t t, uint64_t before, const Sum<uint64_t> &) const { tile_off[t] = before; }
};
struct LenOp {
    const uint32_t *len;
    uint64_t *off;
    __device__ __forceinline__ Sum<uint64_t> load(uint64_t i) const { return Sum<uint64_t>{len[i]}; }
    __device__ __forceinline__ void store(uint64_t i, uint64_t before, const Sum<uint64_t> &) const { off[i] = before; }
};

// The tile [B0, B0 + tlen) of a round of n hits and `bytes` bytes; positions are kept relative to B0, so a line that began
// in an earlier tile has a negative one.
__global__ __launch_bounds__(kFlatThreads) void k_bed_tiles(BedInput in, BedHits h, uint64_t n, const uint64_t *__restrict__ off, uint64_t bytes,
                                                            uint64_t tile0, uint8_t *__restrict__ out) {
    __shared__ uint4 tile4[kFlatTile / 16];
    __shared__ LongCopy longs[kLongCap];
    __shared__ uint32_t n_long;
    __shared__ uint64_t s_range[2];
    uint8_t *tile = reinterpret_cast<uint8_t *>(tile4);
    const uint32_t lane = threadIdx.x;
    const uint64_t B0 = (tile0 + blockIdx.x) * kFlatTile;
    const int64_t tlen = (int64_t)min((uint64_t)kFlatTile, bytes - B0);
    for (uint32_t v = lane; v < kFlatTile / 16; v += kFlatThreads) tile4[v] = uint4{0, 0, 0, 0};
    if (lane == 0) {
        n_long = 0;
        s_range[0] = last_at_or_before(off, 0, n - 1, B0);  // the lines that have a byte in the tile
        s_range[1] = last_at_or_before(off, s_range[0], n - 1, B0 + (uint64_t)tlen - 1);
    }
    __syncthreads();
    const auto put = [&](int64_t at, uint8_t ch) {
        if (at >= 0 && at < tlen) tile[at] = ch;
    };
    const auto put_num = [&](int64_t at, uint64_t x, uint32_t nd) {  // nd digits, the last at at + nd - 1
        if (at >= tlen || at + nd <= 0) return;
        int64_t d = at + nd - 1;
        for (; d >= at && (x >> 32); --d) {
            put(d, (uint8_t)('0' + x % 10));
            x /= 10;
        }
        for (uint32_t y = (uint32_t)x; d >= at; --d) {
            put(d, (uint8_t)('0' + y % 10));
            y /= 10;
        }
    };
    const auto put_bytes = [&](int64_t at, const uint8_t *src, uint32_t len) {
        const int64_t lo = max((int64_t)0, -at), hi = min((int64_t)len, tlen - at);
        if (lo >= hi) return;
        if (hi - lo > (int64_t)kFlatLongName) {
            const uint32_t e = atomicAdd(&n_long, 1u);  // (LDS: which slot of the tile's list, not data)
            if (e < kLongCap) {
                longs[e] = LongCopy{src + lo, (uint32_t)(at + lo), (uint32_t)(hi - lo)};
                return;
            }
        }
        for (int64_t k = lo; k < hi; ++k) tile[at + k] = src[k];
    };
    const uint64_t l0 = s_range[0], l1 = s_range[1];
    for (uint64_t l = l0 + lane; l <= l1; l += kFlatThreads) {
        const uint32_t g = in.b.id[h.b[l]];
        const uint32_t name_at = in.gname[2 * (uint64_t)g], name_len = in.gname[2 * (uint64_t)g + 1];
        const uint64_t s = h.s[l], e = h.e[l];
        int64_t at = (int64_t)(off[l] - B0);
        put_bytes(at, in.names + name_at, name_len), at += name_len;
        put(at++, '\t');
        const uint32_t ds = digits10(s), de = digits10(e);
        put_num(at, s, ds), at += ds;
        put(at++, '\t');
        put_num(at, e, de), at += de;
        put(at, '\n');
    }
    __syncthreads();
    const uint32_t nl = min(n_long, kLongCap);
    for (uint32_t c = 0; c < nl; ++c) {
        const LongCopy lc = longs[c];
        for (uint32_t k = lane; k < lc.len; k += kFlatThreads) tile[lc.dst + k] = lc.src[k];
    }
    __syncthreads();
    uint4 *dst = reinterpret_cast<uint4 *>(out + (uint64_t)blockIdx.x * kFlatTile);
    for (uint32_t v = lane; v < kFlatTile / 16; v += kFlatThreads) dst[v] = tile4[v];
}

}  // namespace

// ---- host side ----

struct BedJob : PieceBufs {
    uint64_t round_cands = kBedRoundCands;
    BedInput in;
    hipStream_t work = nullptr;
    bool begun = false;
    uint64_t cands = 0, unsorted_groups = 0;
    uint32_t *gstart = nullptr, *unsorted = nullptr, *lo = nullptr, *cand = nullptr, *flags = nullptr;
    uint64_t *runmax = nullptr, *prefix = nullptr;
    // a round's scratch: sized by the round
    uint64_t room = 0;
    uint32_t *tile_hits = nullptr;
    uint64_t *tile_off = nullptr, *off = nullptr;
    Spine<Sum<uint64_t>> tile_sp, len_sp;
    BedHits own;
    DeviceMem mem;
};

BedJob *bed_new(uint64_t round_cands) {
    BedJob *j = new BedJob();
    j->round_cands = std::max<uint64_t>(round_cands, 1);
    return j;
}

void bed_free(BedJob *j) {
    if (!j) return;
    if (j->work) (void)hipStreamSynchronize(j->work);
    pieces_free(j);
    delete j;  // (the device memory goes with mem)
}

uint64_t bed_rounds(const BedJob *j) { return j && j->begun ? blocks(j->cands, j->round_cands) : 0; }

int bed_begin(BedJob *j, const BedInput &in, hipStream_t st, uint64_t *candidates, uint64_t *unsorted_groups) {
    if (!j || !candidates || !unsorted_groups) { set_error("bed: NULL argument"); return FLATGFA_ERR_ARG; }
    if (j->begun || j->flags) { set_error("bed: a job begins once"); return FLATGFA_ERR_ARG; }
    *candidates = *unsorted_groups = 0;
    if (in.a.n >= 0xFFFFFFFFull || in.b.n >= 0xFFFFFFFFull) { set_error("bed: a file has 2^32 - 1 entries or more"); return FLATGFA_ERR_BOUNDS; }
    if ((in.a.n && (!in.a.id || !in.a.start || !in.a.end)) || (in.b.n && (!in.b.id || !in.b.start || !in.b.end))) {
        set_error("bed: NULL argument");
        return FLATGFA_ERR_ARG;
    }
    j->in = in;
    j->work = st;
    j->mem.st = st;
    const uint64_t nA = in.a.n, nB = in.b.n, G = in.n_groups;
    BED_HIP(j->mem.alloc(&j->flags, 1));
    BED_HIP(hipMemsetAsync(j->flags, 0, 4, st));
    if (!nA || !nB) {  // no pair: no candidate
        j->begun = true;
        return FLATGFA_OK;
    }
    BED_HIP(j->mem.alloc(&j->gstart, G + 1));
    BED_HIP(j->mem.alloc(&j->unsorted, G));
    BED_HIP(j->mem.alloc(&j->runmax, nB));
    BED_HIP(j->mem.alloc(&j->lo, nA));
    BED_HIP(j->mem.alloc(&j->cand, nA));
    BED_HIP(j->mem.alloc(&j->prefix, nA + 1));
    BED_HIP(hipMemsetAsync(j->gstart, 0, (G + 1) * 4, st));
    BED_HIP(hipMemsetAsync(j->unsorted, 0, std::max<uint64_t>(G, 1) * 4, st));
    uint32_t flags = 0;
    {
        ProfScope prof("bed_groups", st);
        hipLaunchKernelGGL(k_bed_groups, dim3((uint32_t)blocks(nB, kBedThreads)), dim3(kBedThreads), 0, st, in.b, in.n_groups, j->gstart, j->unsorted,
                           j->flags);
    }
    BED_HIP(hipGetLastError());
    BED_HIP(hipMemcpyAsync(&flags, j->flags, 4, hipMemcpyDeviceToHost, st));
    BED_HIP(hipStreamSynchronize(st));
    if (flags & kBadB) {  // (the ranges would read group bounds that were never written)
        set_error("bed: the second file's entries are not grouped by ids below the group count");
        return FLATGFA_ERR_BOUNDS;
    }
    {
        Spine<MaxV> sp;
        BED_HIP(sp.alloc(&j->mem, blocks(nB, kBedThreads * kBedScanPer)));
        const RunMaxOp op{in.b, j->runmax};
        ProfScope prof("bed_runmax", st);
        scan_count<kBedThreads, kBedScanPer, MaxV>(op, nB, sp, st);
        scan_apply<kBedThreads, kBedScanPer, MaxV>(op, nB, sp, st);
    }
    BED_HIP(hipGetLastError());
    {
        ProfScope prof("bed_ranges", st);
        hipLaunchKernelGGL(k_bed_ranges, dim3((uint32_t)blocks(nA, kBedThreads)), dim3(kBedThreads), 0, st, in, Groups{j->gstart, j->unsorted, j->runmax},
                           j->lo, j->cand, j->flags);
    }
    BED_HIP(hipGetLastError());
    uint64_t got[2] = {0, 0};
    {
        Spine<Sum<uint64_t>> sp;
        Spine<Sum<uint32_t>> usp;
        BED_HIP(sp.alloc(&j->mem, blocks(nA, kBedThreads * kBedScanPer)));
        BED_HIP(usp.alloc(&j->mem, blocks(G, kBedThreads * kBedScanPer)));
        const CandOp op{j->cand, j->prefix};
        {
            ProfScope prof("bed_cand_scan", st);
            scan_count<kBedThreads, kBedScanPer, Sum<uint64_t>>(op, nA, sp, st);
            scan_apply<kBedThreads, kBedScanPer, Sum<uint64_t>>(op, nA, sp, st);
            scan_count<kBedThreads, kBedScanPer, Sum<uint32_t>>(UnsortedOp{j->unsorted}, G, usp, st);
        }
        BED_HIP(hipGetLastError());
        BED_HIP(hipMemcpyAsync(j->prefix + nA, sp.total, 8, hipMemcpyDeviceToDevice, st));
        BED_HIP(hipMemcpyAsync(&got[0], sp.total, 8, hipMemcpyDeviceToHost, st));
        BED_HIP(hipMemcpyAsync(&got[1], usp.total, 8, hipMemcpyDeviceToHost, st));
        BED_HIP(hipMemcpyAsync(&flags, j->flags, 4, hipMemcpyDeviceToHost, st));
        BED_HIP(hipStreamSynchronize(st));
    }
    if (flags & kBadA) { set_error("bed: an entry of the first file has an id at or past the group count"); return FLATGFA_ERR_BOUNDS; }
    j->cands = *candidates = got[0];
    j->unsorted_groups = *unsorted_groups = got[1];
    j->begun = true;
    return FLATGFA_OK;
}

namespace {

// the scratch every round needs: the tiles' counts and their scan
int round_scratch(BedJob *j) {
    if (j->room) return FLATGFA_OK;
    const uint64_t room = std::min(j->round_cands, std::max<uint64_t>(j->cands, 1)), tiles = blocks(room, kBedCandTile);
    BED_HIP(j->mem.alloc(&j->tile_hits, tiles));
    BED_HIP(j->mem.alloc(&j->tile_off, tiles));
    BED_HIP(j->tile_sp.alloc(&j->mem, blocks(tiles, kBedThreads * kBedScanPer)));
    j->room = room;
    return FLATGFA_OK;
}

// ... and the job's own records, their line offsets and that scan, for the calls that keep the hits to themselves
int own_records(BedJob *j) {
    if (int rc = round_scratch(j)) return rc;
    if (j->own.a) return FLATGFA_OK;
    BED_HIP(j->mem.alloc(&j->own.a, j->room));
    BED_HIP(j->mem.alloc(&j->own.b, j->room));
    BED_HIP(j->mem.alloc(&j->own.s, j->room));
    BED_HIP(j->mem.alloc(&j->own.e, j->room));
    BED_HIP(j->mem.alloc(&j->own.len, j->room));
    BED_HIP(j->mem.alloc(&j->off, j->room));
    BED_HIP(j->len_sp.alloc(&j->mem, blocks(j->room, kBedThreads * kBedScanPer)));
    return FLATGFA_OK;
}

// count, scan, fill; waits for the stream
int run_round(BedJob *j, uint64_t r, const BedHits &out, uint64_t *n_hits) {
    const hipStream_t st = j->work;
    const uint64_t c0 = r * j->round_cands, n = std::min(j->round_cands, j->cands - c0);
    const uint32_t tiles = (uint32_t)blocks(n, kBedCandTile);
    const TileOp op{j->tile_hits, j->tile_off};
    {
        ProfScope prof("bed_count", st);
        hipLaunchKernelGGL(k_bed_hits<false>, dim3(tiles), dim3(kBedThreads), 0, st, j->in, j->prefix, j->lo, c0, n, j->tile_hits, j->tile_off, out);
    }
    {
        ProfScope prof("bed_tile_scan", st);
        scan_count<kBedThreads, kBedScanPer, Sum<uint64_t>>(op, tiles, j->tile_sp, st);
        scan_apply<kBedThreads, kBedScanPer, Sum<uint64_t>>(op, tiles, j->tile_sp, st);
    }
    {
        ProfScope prof("bed_fill", st);
        hipLaunchKernelGGL(k_bed_hits<true>, dim3(tiles), dim3(kBedThreads), 0, st, j->in, j->prefix, j->lo, c0, n, j->tile_hits, j->tile_off, out);
    }
    BED_HIP(hipGetLastError());
    BED_HIP(hipMemcpyAsync(n_hits, j->tile_sp.total, 8, hipMemcpyDeviceToHost, st));
    BED_HIP(hipStreamSynchronize(st));
    return FLATGFA_OK;
}

// the round's line offsets (emit) and their sum; waits for the stream
int scan_lines(BedJob *j, uint64_t n_hits, bool apply, uint64_t *bytes) {
    const hipStream_t st = j->work;
    const LenOp op{j->own.len, j->off};
    {
        ProfScope prof("bed_line_scan", st);
        scan_count<kBedThreads, kBedScanPer, Sum<uint64_t>>(op, n_hits, j->len_sp, st);
        if (apply) scan_apply<kBedThreads, kBedScanPer, Sum<uint64_t>>(op, n_hits, j->len_sp, st);
    }
    BED_HIP(hipGetLastError());
    BED_HIP(hipMemcpyAsync(bytes, j->len_sp.total, 8, hipMemcpyDeviceToHost, st));
    BED_HIP(hipStreamSynchronize(st));
    return FLATGFA_OK;
}

int ready(const BedJob *j, bool text) {
    if (!j) { set_error("bed: NULL argument"); return FLATGFA_ERR_ARG; }
    if (!j->begun) { set_error("bed: a round before a successful begin"); return FLATGFA_ERR_ARG; }
    if (text && j->cands && !j->in.gname) { set_error("bed: the lines' lengths need the names"); return FLATGFA_ERR_ARG; }
    return FLATGFA_OK;
}

}  // namespace

int bed_round(BedJob *j, uint64_t r, const BedHits &out, uint64_t *n_hits) {
    if (int rc = ready(j, out.len != nullptr)) return rc;
    if (!n_hits || !out.a || !out.b || !out.s || !out.e) { set_error("bed: NULL argument"); return FLATGFA_ERR_ARG; }
    *n_hits = 0;
    if (r >= bed_rounds(j)) { set_error("bed: no such round"); return FLATGFA_ERR_BOUNDS; }
    if (int rc = round_scratch(j)) return rc;
    return run_round(j, r, out, n_hits);
}

int bed_count(BedJob *j, BedTotals *t) {
    if (int rc = ready(j, true)) return rc;
    if (!t) { set_error("bed: NULL argument"); return FLATGFA_ERR_ARG; }
    *t = BedTotals();
    t->candidates = j->cands, t->unsorted_groups = j->unsorted_groups;
    if (!j->cands) return FLATGFA_OK;
    if (int rc = own_records(j)) return rc;
    for (uint64_t r = 0, n = bed_rounds(j); r < n; ++r) {
        uint64_t hits = 0, bytes = 0;
        if (int rc = run_round(j, r, j->own, &hits)) return rc;
        if (int rc = scan_lines(j, hits, false, &bytes)) return rc;
        t->lines += hits, t->bytes += bytes;
    }
    return FLATGFA_OK;
}

int bed_emit(BedJob *j, FlatSink sink, void *ctx, BedTotals *t) {
    if (int rc = ready(j, true)) return rc;
    if (!sink) { set_error("bed: NULL argument"); return FLATGFA_ERR_ARG; }
    BedTotals tot;
    tot.candidates = j->cands, tot.unsorted_groups = j->unsorted_groups;
    if (t) *t = tot;
    if (!j->cands) return FLATGFA_OK;
    if (int rc = pieces_ready(j, &j->mem, j->work, "bed: ")) return rc;
    if (int rc = own_records(j)) return rc;
    Pipe pipe(j, sink, ctx, "bed: ");
    if (!pipe.pin) { set_error("bed: no pinned staging buffer"); return FLATGFA_ERR_HIP; }
    const hipStream_t st = j->work;
    for (uint64_t r = 0, n = bed_rounds(j); r < n; ++r) {
        // (behind the pieces of the round before: the records and offsets are theirs until they are formatted)
        uint64_t hits = 0, bytes = 0;
        if (int rc = run_round(j, r, j->own, &hits)) return rc;
        if (!hits) continue;
        if (int rc = scan_lines(j, hits, true, &bytes)) return rc;
        tot.lines += hits, tot.bytes += bytes;
        if (int rc = pipe.tiles(bytes, [&](uint8_t *out, uint64_t tile0, uint32_t nt) {
                ProfScope prof("bed_tiles", st);
                hipLaunchKernelGGL(k_bed_tiles, dim3(nt), dim3(kFlatThreads), 0, st, j->in, j->own, hits, j->off, bytes, tile0, out);
            }))
            return rc;
    }
    if (t) *t = tot;
    return pipe.finish();
}

}  // namespace fgfa_dev

// ---- the device-level C ABI (include/flatgfa.h Part 3) ----
struct flatgfa_dev_bed {
    fgfa_dev::BedJob *job = nullptr;
    ~flatgfa_dev_bed() { fgfa_dev::bed_free(job); }
};

extern "C" {

int flatgfa_dev_bed_begin(const uint32_t *a_id, const uint64_t *a_start, const uint64_t *a_end, uint64_t n_a, const uint32_t *b_id,
                          const uint64_t *b_start, const uint64_t *b_end, uint64_t n_b, uint32_t n_groups, uint64_t round_cands, void *stream,
                          flatgfa_dev_bed_t **job, uint64_t *candidates, uint64_t *rounds, uint64_t *unsorted_groups) {
    if (job) *job = nullptr;
    if (!job || !candidates || !rounds || !unsorted_groups) { fgfa_dev::set_error("flatgfa_dev_bed_begin: NULL argument"); return FLATGFA_ERR_ARG; }
    *candidates = *rounds = *unsorted_groups = 0;
    if ((n_a && (!a_id || !a_start || !a_end)) || (n_b && (!b_id || !b_start || !b_end))) {
        fgfa_dev::set_error("flatgfa_dev_bed_begin: NULL argument");
        return FLATGFA_ERR_ARG;
    }
    fgfa_dev::BedInput in;
    in.a = fgfa_dev::BedSide{a_id, a_start, a_end, n_a};
    in.b = fgfa_dev::BedSide{b_id, b_start, b_end, n_b};
    in.n_groups = n_groups;
    auto *h = new flatgfa_dev_bed();
    h->job = fgfa_dev::bed_new(round_cands ? round_cands : fgfa_dev::kBedRoundCands);
    const int rc = fgfa_dev::bed_begin(h->job, in, (hipStream_t)stream, candidates, unsorted_groups);
    if (rc) {
        delete h;
        return rc;
    }
    *rounds = fgfa_dev::bed_rounds(h->job);
    *job = h;
    return FLATGFA_OK;
}

int flatgfa_dev_bed_round(flatgfa_dev_bed_t *job, uint64_t round, uint32_t *a_index, uint32_t *b_index, uint64_t *start, uint64_t *end,
                          uint64_t *n_hits) {
    if (!job) { fgfa_dev::set_error("flatgfa_dev_bed_round: NULL job"); return FLATGFA_ERR_ARG; }
    fgfa_dev::BedHits out;
    out.a = a_index, out.b = b_index, out.s = start, out.e = end;
    return fgfa_dev::bed_round(job->job, round, out, n_hits);
}

void flatgfa_dev_bed_free(flatgfa_dev_bed_t *job) { delete job; }

}  // extern "C"
