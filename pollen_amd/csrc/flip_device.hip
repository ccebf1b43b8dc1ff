// Flip on gfx950 (slow_odgi/slow_odgi/flip.py over mygfa/gfa.py): a path that walks more bases backward
// than forward is turned around -- its steps reversed, every orientation toggled -- and for every consecutive pair of a turned
// path's new steps a link with the overlap 0M joins the old links, which are then de-duplicated: a link and its reverse
// complement with equal overlaps are one link, and the first of each class stays, in input order.
//
// The steps are walked in the coordinates of the paths laid one behind another, never in the pool's: spans that are out of
// order, overlap or leave gaps then need no special case, and the work is dealt by steps, not by paths.
//
//   k_flip_check    every path span lies inside the steps, every link names segments and has an overlap span inside the
//                   alignment pool, else a bit of the flag word (and no later kernel of the count reads through them)
//   k_flip_weigh    a workgroup per tile of kFlipTile laid-out steps: Segment::len() of every step, summed in 64 bits into
//                   fwd and rev of its path.  A tile inside one path is a plain workgroup reduction; a tile in which paths
//                   begin sums in LDS, one slot for the path that runs into the tile and one per step at which a path may
//                   begin (a wave whose lanes share a path adds once).  What a tile holds of the path that runs into it goes
//                   to part[tile], what it holds of a path that begins in it to head[path]: no global atomics.
//   k_flip_decide   a wave per path: head[path] plus the part[] of the tiles it runs into; turned = rev > fwd
//   scans           (device_scan.hpp) the turned paths, and max(n - 1, 0) per turned path into cand_start: a turned path's
//                   candidate i is the link from its new step i to its new step i + 1, and candidate c of the whole has the
//                   ordinal n_links + c behind the old links' 0 .. n_links
//   k_flip_keys     twice.  Every old link and every candidate (by tile of steps again: the new steps are read from the old
//                   ones, reversed) forms its canonical key, min of (from << 32 | to) and (flip(to) << 32 | flip(from)), as
//                   topology_device.hip does.  First launch: the keys are counted by their high handle.  k_scan of the rows.
//                   Second launch: (low half << 32 | ordinal) goes into its row behind a cursor.
//   rounds          the two launches below and the second one above run once per round of kFlipRoundKeys key offsets, on the
//                   rows that begin there, in scratch for two rounds' keys: one round where all keys fit that scratch
//   k_flip_short    a wave takes 64 rows at a time.  A row of one entry is kept as it is.  A row of up to kFlipShortRow
//                   entries is sorted in the wave's registers (a bitonic network through shuffles) and decided there; a
//                   longer one is listed.
//   k_flip_long     a workgroup per listed row: the same network in LDS (up to kFlipLdsRow entries) or in place, then the
//                   same decision.
//                   The decision: sorted, a class of equal keys is a run with the ordinals ascending, so the old links of a
//                   run stand before its candidates.  A candidate behind another candidate of its run is dropped -- one
//                   look at the entry before it, whatever the run's length.  The first candidate of a run is kept unless an
//                   old link of the run has the overlap 0M; an old link is kept unless an earlier old link of the run has
//                   an equal overlap, op for op: both walk back over the run's old links, which is quadratic in the old
//                   links of one class and in nothing else.
//   scans           the keep flags of the old links and of the candidates, in ordinal order; the host reads the totals
//   k_flip_rewrite  (fill) by tile of output steps: out[j] = turned ? in[end - 1 - i] ^ 1 : in[begin + i]; a reversed tile
//                   is still one contiguous read
//   scans, again    (fill) with the stores: a kept old link is copied to its place, a kept candidate is made there
// Kernels never trap: whatever is out of range raises a bit of the flag word.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/flatgfa.h"
#include "device_common.hpp"
#include "device_scan.hpp"
#include "flip_device.hpp"
#include "prof.hpp"

namespace fgfa_dev {
namespace {

#define FL_HIP(expr) FGFA_HIP("flip: ", expr)

// flag word bits
constexpr uint32_t kBadStep = 1, kBadLink = 2, kBadSpan = 4, kBadOverlap = 8, kLongRow = 16;

constexpr uint32_t kWaves = kFlipThreads / 64;
static_assert(kFlipShortRow == 64, "a short row is one entry per lane of a wave");
static_assert((kFlipLdsRow & (kFlipLdsRow - 1)) == 0, "the LDS network is padded to a power of two");

__device__ __forceinline__ uint64_t canon(uint32_t from, uint32_t to) {
    const uint64_t x = ((uint64_t)from << 32) | to, y = ((uint64_t)(to ^ 1u) << 32) | (from ^ 1u);
    return x < y ? x : y;
}

struct FlipSteps {
    const uint32_t *steps;
    const uint32_t *pstart, *pbegin;
    uint32_t n_paths;
    uint64_t n_lin, n_steps;
};

// the paths of a tile's first and last step, for all lanes (contains a barrier, and one before it: `ends` may still be read)
__device__ __forceinline__ void tile_paths(const FlipSteps &g, uint64_t t0, uint64_t t1, uint32_t *ends) {
    __syncthreads();
    if (threadIdx.x < 2) ends[threadIdx.x] = last_start_at_or_before(g.pstart, 0, g.n_paths - 1, threadIdx.x ? t1 - 1 : t0);
    __syncthreads();
}

__global__ __launch_bounds__(kFlipThreads) void k_flip_check(FlipSteps g, const uint32_t *__restrict__ links, uint64_t n_links, uint32_t n_segs,
                                                             uint64_t n_align, uint32_t *flags) {
    const uint64_t n = max((uint64_t)g.n_paths, n_links);
    for (uint64_t i = (uint64_t)blockIdx.x * kFlipThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kFlipThreads) {
        if (i < g.n_paths) {  // pstart rises from 0 to n_lin, and every span lies inside the steps
            const uint64_t ps = g.pstart[i], pe = g.pstart[i + 1];
            if (pe < ps || pe > g.n_lin || (i == 0 && ps != 0) || (i + 1 == g.n_paths && pe != g.n_lin) || (uint64_t)g.pbegin[i] + (pe - ps) > g.n_steps)
                atomicOr(flags, kBadSpan);
        }
        if (i < n_links) {
            if ((links[i * 4] >> 1) >= n_segs || (links[i * 4 + 1] >> 1) >= n_segs) atomicOr(flags, kBadLink);
            if (links[i * 4 + 2] > links[i * 4 + 3] || links[i * 4 + 3] > n_align) atomicOr(flags, kBadOverlap);
        }
    }
}

// ---- weigh ----

__global__ __launch_bounds__(kFlipThreads) void k_flip_weigh(FlipSteps g, const uint32_t *__restrict__ seg_len, uint32_t n_segs, uint64_t n_tiles,
                                                             uint64_t *__restrict__ part, uint64_t *__restrict__ head, uint32_t *flags) {
    __shared__ unsigned long long s_f[kFlipTile + 1], s_r[kFlipTile + 1];  // slot 0: the path that runs into the tile; 1 + i: one that begins at its step i
    __shared__ uint64_t s_w[2 * kWaves];
    __shared__ uint32_t ends[2], s_bad;
    const uint32_t t = threadIdx.x, lane = t & 63;
    if (t == 0) s_bad = *flags;  // (what k_flip_check found; one read, so that every lane takes the same way while this launch raises bits too)
    __syncthreads();
    if (s_bad) return;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t t0 = tile * kFlipTile, t1 = min(t0 + kFlipTile, g.n_lin);
        tile_paths(g, t0, t1, ends);
        const uint32_t e0 = ends[0], e1 = ends[1];
        const bool one = e0 == e1;  // (the same for every lane)
        if (!one) {
            for (uint32_t i = t; i <= kFlipTile; i += kFlipThreads) s_f[i] = 0, s_r[i] = 0;
            __syncthreads();
        }
        uint64_t f = 0, r = 0;
        uint32_t p = e0, head_of[kFlipPer];
        uint64_t ps = g.pstart[e0], pb = g.pbegin[e0];
#pragma unroll
        for (uint32_t q = 0; q < kFlipPer; ++q) {
            const uint64_t j = t0 + (uint64_t)q * kFlipThreads + t;
            const bool active = j < t1;
            uint64_t len = 0;
            bool fwd = true;
            head_of[q] = 0xFFFFFFFFu;
            if (active) {
                if (!one) {
                    p = last_start_at_or_before(g.pstart, e0, e1, j);
                    ps = g.pstart[p], pb = g.pbegin[p];
                    if (j == ps) head_of[q] = p;
                }
                const uint64_t at = pb + (j - ps);
                if (at < g.n_steps) {
                    const uint32_t h = g.steps[at];
                    if ((h >> 1) < n_segs) len = seg_len[h >> 1], fwd = !(h & 1u);
                    else atomicOr(flags, kBadStep);
                } else {
                    atomicOr(flags, kBadSpan);
                }
            }
            if (one) {
                if (fwd) f += len;
                else r += len;
            } else {
                const uint32_t slot = !active ? 0xFFFFFFFFu : ps < t0 ? 0u : 1u + (uint32_t)(ps - t0);
                const uint32_t slot0 = (uint32_t)__shfl((int)slot, 0, 64);  // (lane 0 idle: so are the lanes above it)
                if (__all(slot == slot0 || slot == 0xFFFFFFFFu)) {
                    const uint64_t wf = wave_sum(fwd ? len : 0), wr = wave_sum(fwd ? 0 : len);
                    if (lane == 0 && slot0 != 0xFFFFFFFFu) {
                        if (wf) atomicAdd(&s_f[slot0], (unsigned long long)wf);
                        if (wr) atomicAdd(&s_r[slot0], (unsigned long long)wr);
                    }
                } else if (active && len) {
                    atomicAdd(fwd ? &s_f[slot] : &s_r[slot], (unsigned long long)len);
                }
            }
        }
        if (one) {
            f = wave_sum(f), r = wave_sum(r);
            if (lane == 0) s_w[2 * (t >> 6)] = f, s_w[2 * (t >> 6) + 1] = r;
            __syncthreads();
            if (t == 0) {
                uint64_t af = 0, ar = 0;
                for (uint32_t w = 0; w < kWaves; ++w) af += s_w[2 * w], ar += s_w[2 * w + 1];
                const bool runs_in = ps < t0;  // (else the path begins with the tile)
                part[2 * tile] = runs_in ? af : 0, part[2 * tile + 1] = runs_in ? ar : 0;
                if (!runs_in) head[2 * (uint64_t)e0] = af, head[2 * (uint64_t)e0 + 1] = ar;
            }
        } else {
            __syncthreads();
            if (t == 0) part[2 * tile] = s_f[0], part[2 * tile + 1] = s_r[0];
#pragma unroll
            for (uint32_t q = 0; q < kFlipPer; ++q) {
                if (head_of[q] == 0xFFFFFFFFu) continue;
                const uint32_t at = 1u + q * kFlipThreads + t;
                head[2 * (uint64_t)head_of[q]] = s_f[at], head[2 * (uint64_t)head_of[q] + 1] = s_r[at];
            }
        }
    }
}

__global__ __launch_bounds__(kFlipThreads) void k_flip_decide(const uint32_t *__restrict__ pstart, uint32_t n_paths, const uint64_t *__restrict__ part,
                                                              const uint64_t *__restrict__ head, uint32_t *__restrict__ turned, const uint32_t *flags) {
    if (*flags) return;
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t p = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); p < n_paths; p += (uint64_t)gridDim.x * kWaves) {
        const uint64_t ps = pstart[p], pe = pstart[p + 1];
        uint64_t f = 0, r = 0;
        if (pe > ps) {
            // the tiles behind the one the path begins in hold it in part[]: it runs into each of them
            for (uint64_t tile = ps / kFlipTile + 1 + lane; tile <= (pe - 1) / kFlipTile; tile += 64) f += part[2 * tile], r += part[2 * tile + 1];
            f = wave_sum(f) + head[2 * p], r = wave_sum(r) + head[2 * p + 1];
        }
        if (lane == 0) turned[p] = r > f ? 1u : 0u;  // flip.py:16: strictly
    }
}

// ---- the scans' operands ----
struct TurnOp {  // the turned paths (counted only)
    const uint32_t *turned;
    __device__ __forceinline__ Sum<uint32_t> load(uint64_t i) const { return Sum<uint32_t>{turned[i]}; }
    __device__ __forceinline__ void store(uint64_t, uint32_t, const Sum<uint32_t> &) const {}
};
struct CandOp {  // flip.py:61-67: a turned path of n steps gives n - 1 links; over n_paths + 1 elements, so that the last start is the total
    const uint32_t *turned, *pstart;
    uint32_t n_paths;
    uint32_t *cand_start;
    __device__ __forceinline__ Sum<uint32_t> load(uint64_t i) const {
        if (i >= n_paths || !turned[i]) return Sum<uint32_t>{0};
        const uint32_t n = pstart[i + 1] - pstart[i];
        return Sum<uint32_t>{n ? n - 1 : 0};
    }
    __device__ __forceinline__ void store(uint64_t i, uint32_t before, const Sum<uint32_t> &) const { cand_start[i] = before; }
};
struct RowOp {  // the row counts -> where each row begins, in place
    uint32_t *data;
    __device__ __forceinline__ Sum<uint32_t> load(uint64_t i) const { return Sum<uint32_t>{data[i]}; }
    __device__ __forceinline__ void store(uint64_t i, uint32_t before, const Sum<uint32_t> &) const { data[i] = before; }
};

// new steps i and i + 1 of turned path p
struct NewPair {
    uint32_t a, b;
};
__device__ __forceinline__ NewPair new_pair(const FlipSteps &g, uint32_t p, uint64_t i) {
    const uint64_t last = (uint64_t)g.pbegin[p] + (g.pstart[p + 1] - g.pstart[p]) - 1;
    return NewPair{g.steps[last - i] ^ 1u, g.steps[last - i - 1] ^ 1u};
}

// ---- keys ----

// A round's rows: those that begin at key offsets [lo, hi) and end inside the scratch of `room` keys that begins at lo.
struct Window {
    uint64_t lo, hi, room;
    __device__ __forceinline__ bool begins(uint64_t r0) const { return r0 >= lo && r0 < hi; }
    __device__ __forceinline__ bool holds(uint64_t r0, uint64_t r1) const { return begins(r0) && r1 - lo <= room; }
};

template <bool kScatter>
__global__ __launch_bounds__(kFlipThreads) void k_flip_keys(FlipSteps g, const uint32_t *__restrict__ links, uint64_t n_links, uint64_t n_tiles,
                                                            const uint32_t *__restrict__ turned, const uint32_t *__restrict__ cand_start, uint32_t *row,
                                                            uint32_t *cursor, uint64_t *__restrict__ items, Window w, const uint32_t *flags) {
    __shared__ uint32_t ends[2];
    if (*flags) return;
    const auto put = [&](uint64_t key, uint64_t ordinal) {
        const uint32_t h = (uint32_t)(key >> 32);
        if (!kScatter) {
            atomicAdd(row + h, 1u);
        } else if (w.holds(row[h], row[h + 1])) {
            items[(uint64_t)row[h] - w.lo + atomicAdd(cursor + h, 1u)] = (key << 32) | ordinal;
        }
    };
    for (uint64_t i = (uint64_t)blockIdx.x * kFlipThreads + threadIdx.x; i < n_links; i += (uint64_t)gridDim.x * kFlipThreads)
        put(canon(links[i * 4], links[i * 4 + 1]), i);
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t t0 = tile * kFlipTile, t1 = min(t0 + kFlipTile, g.n_lin);
        tile_paths(g, t0, t1, ends);
        const uint32_t e0 = ends[0], e1 = ends[1];
        if (e0 == e1 && !turned[e0]) continue;  // (the same for every lane)
        for (uint32_t q = 0; q < kFlipPer; ++q) {
            const uint64_t j = t0 + (uint64_t)q * kFlipThreads + threadIdx.x;
            if (j >= t1) break;
            const uint32_t p = last_start_at_or_before(g.pstart, e0, e1, j);
            if (!turned[p] || j + 1 >= g.pstart[p + 1]) continue;  // (a path's last step begins no pair)
            const uint64_t i = j - g.pstart[p];
            const NewPair np = new_pair(g, p, i);
            put(canon(np.a, np.b), n_links + cand_start[p] + i);
        }
    }
}

// ---- the decision ----
struct KeepCtx {
    const uint32_t *links, *alignment;
    uint64_t n_links;
    uint32_t *keep;  // by ordinal
};
__device__ __forceinline__ bool zero_m(const KeepCtx &c, uint32_t i) {
    const uint32_t s = c.links[4 * (uint64_t)i + 2], e = c.links[4 * (uint64_t)i + 3];
    return e - s == 1 && c.alignment[s] == 0;  // one op: length 0, match
}
__device__ __forceinline__ bool same_overlap(const KeepCtx &c, uint32_t i, uint32_t k) {
    const uint32_t s1 = c.links[4 * (uint64_t)i + 2], e1 = c.links[4 * (uint64_t)i + 3];
    const uint32_t s2 = c.links[4 * (uint64_t)k + 2], e2 = c.links[4 * (uint64_t)k + 3];
    if (e1 - s1 != e2 - s2) return false;
    if (s1 == s2) return true;
    for (uint32_t x = 0; x < e1 - s1; ++x)
        if (c.alignment[s1 + x] != c.alignment[s2 + x]) return false;
    return true;
}
// does the old link `other`, of the same class and before `mine`, make `mine` a duplicate?
__device__ __forceinline__ bool dup_of(const KeepCtx &c, uint32_t mine, uint32_t other) {
    return mine >= c.n_links ? zero_m(c, other) : same_overlap(c, mine, other);
}

__global__ __launch_bounds__(kFlipThreads) void k_flip_short(KeepCtx c, const uint32_t *__restrict__ row, uint64_t n_rows, const uint64_t *__restrict__ items,
                                                             Window w, uint32_t *list, uint32_t cap, uint32_t *count, uint32_t *flags) {
    __shared__ uint32_t s_bad;
    if (threadIdx.x == 0) s_bad = *flags;  // (one read: this launch raises a bit too)
    __syncthreads();
    if (s_bad) return;
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t base = ((uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6)) * 64; base < n_rows; base += (uint64_t)gridDim.x * kWaves * 64) {
        const uint64_t h = base + lane;
        uint32_t r0 = 0, n = 0;
        if (h < n_rows && w.begins(row[h])) {
            n = row[h + 1] - row[h];
            if (w.holds(row[h], row[h + 1])) r0 = (uint32_t)(row[h] - w.lo);
            else atomicOr(flags, kLongRow), n = 0;  // (nothing of it was scattered)
        }
        if (n == 1) c.keep[(uint32_t)items[r0]] = 1;
        if (n > kFlipShortRow) {
            const uint32_t k = atomicAdd(count, 1u);
            if (k < cap) list[k] = (uint32_t)h;
        }
        uint64_t todo = __ballot(n >= 2 && n <= kFlipShortRow);
        while (todo) {  // (the same for every lane)
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const uint32_t rn = (uint32_t)__shfl((int)n, src, 64), rr0 = (uint32_t)__shfl((int)r0, src, 64);
            uint64_t item = lane < rn ? items[(uint64_t)rr0 + lane] : ~0ull;  // (no entry is all ones: an ordinal is below 2^32 - 1)
#pragma unroll
            for (uint32_t k = 2; k <= 64; k <<= 1) {
#pragma unroll
                for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                    const uint64_t o = shfl_xor_u64(item, (int)j);
                    const bool want_min = ((lane & j) == 0) == ((lane & k) == 0);
                    item = want_min == (o < item) ? o : item;
                }
            }
            const uint64_t prev = shfl_up_u64(item, 1);
            const bool valid = lane < rn, same = valid && lane > 0 && (prev >> 32) == (item >> 32);
            const uint32_t ord = (uint32_t)item;
            bool kept = true;
            if (same && (uint32_t)prev >= c.n_links) kept = false;  // a candidate behind a candidate
            bool walk = same && kept;                               // the entry before is an old link of the run
            if (__any(walk)) {
                for (uint32_t d = 1; d < rn; ++d) {
                    const uint64_t o = shfl_up_u64(item, (int)d);
                    if (walk && lane >= d) {
                        if ((o >> 32) != (item >> 32)) walk = false;
                        else if (dup_of(c, ord, (uint32_t)o)) kept = false, walk = false;
                    }
                }
            }
            if (valid) c.keep[ord] = kept ? 1u : 0u;
        }
    }
}

// One workgroup per listed row.  Compare-exchanges (i, l) with i < l always leave the smaller at i: an l at or past the row's
// end stands for +infinity and is already in place (as k_sort_rows of topology_device.hip).
__global__ __launch_bounds__(kFlipThreads) void k_flip_long(KeepCtx c, const uint32_t *__restrict__ row, uint64_t *items, Window w,
                                                            const uint32_t *__restrict__ list, uint32_t cap, const uint32_t *count, const uint32_t *flags) {
    __shared__ uint64_t s_v[kFlipLdsRow];
    if (*flags) return;
    const uint32_t n_list = min(*count, cap);
    for (uint32_t r = blockIdx.x; r < n_list; r += gridDim.x) {
        const uint32_t h = list[r];
        uint64_t *v = items + (row[h] - w.lo);
        const uint64_t n = row[h + 1] - row[h];
        if (n <= kFlipLdsRow) {
            for (uint64_t i = threadIdx.x; i < n; i += kFlipThreads) s_v[i] = v[i];
            v = s_v;
        }
        __syncthreads();
        uint64_t pow2 = 1;
        while (pow2 < n) pow2 <<= 1;
        for (uint64_t k = 2; k <= pow2; k <<= 1) {
            for (uint64_t j = k >> 1; j > 0; j >>= 1) {
                const uint64_t mask = j == (k >> 1) ? k - 1 : j;  // the first step of a merge flips, the rest disperse
                for (uint64_t i = threadIdx.x; i < n; i += kFlipThreads) {
                    const uint64_t l = i ^ mask;
                    if (l > i && l < n) {
                        const uint64_t x = v[i], y = v[l];
                        if (x > y) v[i] = y, v[l] = x;
                    }
                }
                __syncthreads();
            }
        }
        for (uint64_t i = threadIdx.x; i < n; i += kFlipThreads) {
            const uint64_t item = v[i];
            const uint32_t ord = (uint32_t)item;
            bool kept = true;
            if (i > 0 && (v[i - 1] >> 32) == (item >> 32)) {
                if ((uint32_t)v[i - 1] >= c.n_links) {
                    kept = false;  // a candidate behind a candidate
                } else {
                    for (uint64_t x = i; x-- > 0;) {  // the old links of the run
                        const uint64_t o = v[x];
                        if ((o >> 32) != (item >> 32)) break;
                        if (dup_of(c, ord, (uint32_t)o)) {
                            kept = false;
                            break;
                        }
                    }
                }
            }
            c.keep[ord] = kept ? 1u : 0u;
        }
        __syncthreads();  // (s_v is the next row's)
    }
}

// ---- the kept links ----
struct OldOp {  // the old links' keep flags; the store copies a kept one to its place
    const uint32_t *keep, *links;
    uint32_t *out;
    __device__ __forceinline__ Sum<uint32_t> load(uint64_t i) const { return Sum<uint32_t>{keep[i]}; }
    __device__ __forceinline__ void store(uint64_t i, uint32_t before, const Sum<uint32_t> &me) const {
        if (!me.v) return;
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w) out[4 * (uint64_t)before + w] = links[4 * i + w];
    }
};
struct NewOp {  // the candidates' keep flags, over n_lin elements (the first cand_start[n_paths] are candidates); the store makes a kept one
    const uint32_t *keep;  // (of the first candidate)
    const uint32_t *cand_start;
    FlipSteps g;
    const uint64_t *old_kept;
    uint32_t zero_m_at;
    uint32_t *out;
    __device__ __forceinline__ Sum<uint32_t> load(uint64_t c) const { return Sum<uint32_t>{c < cand_start[g.n_paths] ? keep[c] : 0u}; }
    __device__ __forceinline__ void store(uint64_t c, uint32_t before, const Sum<uint32_t> &me) const {
        if (!me.v) return;
        const uint32_t p = last_start_at_or_before(cand_start, 0, g.n_paths - 1, c);
        const NewPair np = new_pair(g, p, c - cand_start[p]);
        uint32_t *o = out + 4 * (*old_kept + before);
        o[0] = np.a, o[1] = np.b, o[2] = zero_m_at, o[3] = zero_m_at + 1;  // flip.py:56
    }
};

// ---- rewrite ----
__global__ __launch_bounds__(kFlipThreads) void k_flip_rewrite(FlipSteps g, uint64_t n_tiles, const uint32_t *__restrict__ turned, uint32_t *__restrict__ out) {
    __shared__ uint32_t ends[2];
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t t0 = tile * kFlipTile, t1 = min(t0 + kFlipTile, g.n_lin);
        tile_paths(g, t0, t1, ends);
        const uint32_t e0 = ends[0], e1 = ends[1];
        const bool one = e0 == e1;
        uint32_t p = e0;
        uint64_t ps = g.pstart[e0], pe = g.pstart[e0 + 1], pb = g.pbegin[e0];
        bool tn = turned[e0] != 0;
#pragma unroll
        for (uint32_t q = 0; q < kFlipPer; ++q) {
            const uint64_t j = t0 + (uint64_t)q * kFlipThreads + threadIdx.x;
            if (j >= t1) break;
            if (!one) {
                p = last_start_at_or_before(g.pstart, e0, e1, j);
                ps = g.pstart[p], pe = g.pstart[p + 1], pb = g.pbegin[p], tn = turned[p] != 0;
            }
            out[j] = tn ? g.steps[pb + (pe - 1 - j)] ^ 1u : g.steps[pb + (j - ps)];  // flip.py:25-26
        }
    }
}

}  // namespace

struct FlipJob {
    FlipIn in;
    FlipSteps g{};
    bool counted = false;
    uint64_t tiles = 0, n_rows = 0;
    uint32_t *flags = nullptr, *turned = nullptr, *cand_start = nullptr, *row = nullptr, *cursor = nullptr, *list = nullptr, *keep = nullptr;
    uint64_t *part = nullptr, *head = nullptr, *items = nullptr;
    uint32_t list_cap = 0;
    uint64_t round_keys = kFlipRoundKeys;
    Spine<Sum<uint32_t>> path_sp, cand_sp, row_sp, old_sp, new_sp;
    uint64_t n_turned = 0, old_kept = 0, new_kept = 0;
    DeviceMem mem;  // (waits for the last stream used before it frees)
};

FlipJob *flip_new(uint64_t round_keys) {
    FlipJob *j = new FlipJob();
    j->round_keys = std::max<uint64_t>(round_keys, 1);
    return j;
}
void flip_free(FlipJob *j) { delete j; }
const uint32_t *flip_turned(const FlipJob *j) { return j && j->counted ? j->turned : nullptr; }

int flip_count(FlipJob *j, const FlipIn &in, hipStream_t st, uint64_t *n_turned, uint64_t *links_out, uint64_t *links_new) {
    if (!j || !n_turned || !links_out || !links_new || !in.pstart || (in.n_paths && !in.pbegin) || (in.n_lin && (!in.steps || !in.seg_len)) ||
        (in.n_links && !in.links) || (in.n_align && !in.alignment)) {
        set_error("flip: NULL argument");
        return FLATGFA_ERR_ARG;
    }
    if (in.n_segs > 0x7FFFFFFFu || in.n_paths > 0xFFFFFFFEu || in.n_steps > 0xFFFFFFFFull || in.n_align > 0xFFFFFFFEull) {
        set_error("flip: graph too large for 32-bit ids");
        return FLATGFA_ERR_TOO_LARGE;
    }
    // every step of a turned path but its last may add a link: the ordinals of old links and candidates are 32 bits wide
    if (in.n_links + in.n_lin > 0xFFFFFFFEull) {
        set_error("flip: " + std::to_string(in.n_links) + " links and " + std::to_string(in.n_lin) + " steps: more than 2^32 - 1 links may be kept");
        return FLATGFA_ERR_TOO_LARGE;
    }
    if (j->counted) { set_error("flip: this job was counted already"); return FLATGFA_ERR_ARG; }
    j->in = in;
    j->mem.st = st;
    const uint32_t P = in.n_paths, S = in.n_segs;
    const uint64_t L = in.n_links, N = in.n_lin, most = L + N;
    j->g = FlipSteps{in.steps, in.pstart, in.pbegin, P, N, in.n_steps};
    j->tiles = blocks(N, kFlipTile);
    j->n_rows = 2 * (uint64_t)S;
    const uint64_t n_scan = j->n_rows + 1;
    j->list_cap = (uint32_t)(most / (kFlipShortRow + 1) + 1);  // (a listed row holds more than kFlipShortRow of the entries)
    FL_HIP(j->mem.alloc(&j->flags, 4));  // the flag word, the listed rows
    FL_HIP(j->mem.alloc(&j->turned, P));
    FL_HIP(j->mem.alloc(&j->cand_start, (uint64_t)P + 1));
    FL_HIP(j->mem.alloc(&j->part, 2 * j->tiles));
    FL_HIP(j->mem.alloc(&j->head, 2 * (uint64_t)P));
    FL_HIP(j->mem.alloc(&j->row, 2 * n_scan + 1));
    j->cursor = j->row + n_scan + 1;
    FL_HIP(j->mem.alloc(&j->list, j->list_cap));
    // one round where all keys fit the scratch of two rounds; else a round per kFlipRoundKeys key offsets
    const uint64_t R = j->round_keys, room = std::min(most, 2 * R), rounds = most <= 2 * R ? 1 : blocks(most, R);
    FL_HIP(j->mem.alloc(&j->items, room));
    FL_HIP(j->mem.alloc(&j->keep, most));
    constexpr uint64_t kScanTile = (uint64_t)kFlipThreads * kFlipScanPer;
    FL_HIP(j->path_sp.alloc(&j->mem, blocks(P, kScanTile)));
    FL_HIP(j->cand_sp.alloc(&j->mem, blocks((uint64_t)P + 1, kScanTile)));
    FL_HIP(j->row_sp.alloc(&j->mem, blocks(n_scan, kScanTile)));
    FL_HIP(j->old_sp.alloc(&j->mem, blocks(L, kScanTile)));
    FL_HIP(j->new_sp.alloc(&j->mem, blocks(N, kScanTile)));
    FL_HIP(hipMemsetAsync(j->flags, 0, 16, st));
    FL_HIP(hipMemsetAsync(j->row, 0, (2 * n_scan + 1) * 4, st));
    const FlipSteps &g = j->g;
    const uint32_t tile_grid = stride_blocks(j->tiles, 1, kFlipGrid);
    if (P || L) {
        hipLaunchKernelGGL(k_flip_check, dim3(stride_blocks(std::max<uint64_t>(P, L), kFlipThreads, kFlipGrid)), dim3(kFlipThreads), 0, st, g, in.links, L, S,
                           in.n_align, j->flags);
    }
    {
        ProfScope prof("flip_weigh", st);
        if (N) hipLaunchKernelGGL(k_flip_weigh, dim3(tile_grid), dim3(kFlipThreads), 0, st, g, in.seg_len, S, j->tiles, j->part, j->head, j->flags);
        if (P) hipLaunchKernelGGL(k_flip_decide, dim3(stride_blocks(P, kWaves, kFlipGrid)), dim3(kFlipThreads), 0, st, in.pstart, P, j->part, j->head, j->turned, j->flags);
        scan_count<kFlipThreads, kFlipScanPer, Sum<uint32_t>>(TurnOp{j->turned}, P, j->path_sp, st);
        const CandOp op{j->turned, in.pstart, P, j->cand_start};
        scan_count<kFlipThreads, kFlipScanPer, Sum<uint32_t>>(op, (uint64_t)P + 1, j->cand_sp, st);
        scan_apply<kFlipThreads, kFlipScanPer, Sum<uint32_t>>(op, (uint64_t)P + 1, j->cand_sp, st);
    }
    FL_HIP(hipGetLastError());
    const KeepCtx kc{in.links, in.alignment, L, j->keep};
    {
        ProfScope prof("flip_group", st);
        const uint32_t key_grid = std::max(tile_grid, stride_blocks(L, kFlipThreads, kFlipGrid));
        if (most) {
            hipLaunchKernelGGL((k_flip_keys<false>), dim3(key_grid), dim3(kFlipThreads), 0, st, g, in.links, L, j->tiles, j->turned, j->cand_start, j->row, j->cursor,
                               j->items, Window{0, 0, 0}, j->flags);
        }
        scan_count<kFlipThreads, kFlipScanPer, Sum<uint32_t>>(RowOp{j->row}, n_scan, j->row_sp, st);
        scan_apply<kFlipThreads, kFlipScanPer, Sum<uint32_t>>(RowOp{j->row}, n_scan, j->row_sp, st);
        for (uint64_t r = 0; most && r < rounds; ++r) {
            const Window w{r * R, rounds == 1 ? most + 1 : (r + 1) * R, room};
            if (r) FL_HIP(hipMemsetAsync(j->flags + 1, 0, 4, st));  // (the listed rows of the round before)
            hipLaunchKernelGGL((k_flip_keys<true>), dim3(key_grid), dim3(kFlipThreads), 0, st, g, in.links, L, j->tiles, j->turned, j->cand_start, j->row, j->cursor,
                               j->items, w, j->flags);
            hipLaunchKernelGGL(k_flip_short, dim3(stride_blocks(j->n_rows, (uint64_t)kWaves * 64, kFlipGrid)), dim3(kFlipThreads), 0, st, kc, j->row, j->n_rows,
                               j->items, w, j->list, j->list_cap, j->flags + 1, j->flags);
            hipLaunchKernelGGL(k_flip_long, dim3(std::min(j->list_cap, kFlipGrid)), dim3(kFlipThreads), 0, st, kc, j->row, j->items, w, j->list, j->list_cap,
                               j->flags + 1, j->flags);
        }
    }
    FL_HIP(hipGetLastError());
    {  // (after a refusal keep[] is unwritten: the scans then add up whatever it holds, and nobody reads the sums)
        ProfScope prof("flip_compact_count", st);
        scan_count<kFlipThreads, kFlipScanPer, Sum<uint32_t>>(OldOp{j->keep, in.links, nullptr}, L, j->old_sp, st);
        scan_count<kFlipThreads, kFlipScanPer, Sum<uint32_t>>(NewOp{j->keep + L, j->cand_start, g, j->old_sp.total, (uint32_t)in.n_align, nullptr}, N, j->new_sp, st);
    }
    FL_HIP(hipGetLastError());
    uint32_t flags = 0;
    FL_HIP(hipMemcpyAsync(&flags, j->flags, 4, hipMemcpyDeviceToHost, st));
    FL_HIP(hipMemcpyAsync(&j->n_turned, j->path_sp.total, 8, hipMemcpyDeviceToHost, st));
    FL_HIP(hipMemcpyAsync(&j->old_kept, j->old_sp.total, 8, hipMemcpyDeviceToHost, st));
    FL_HIP(hipMemcpyAsync(&j->new_kept, j->new_sp.total, 8, hipMemcpyDeviceToHost, st));
    FL_HIP(hipStreamSynchronize(st));
    if (flags & kBadSpan) { set_error("flip: a path has a step span outside the steps pool"); return FLATGFA_ERR_BOUNDS; }
    if (flags & kBadStep) { set_error("flip: a step refers to a segment id that is out of range"); return FLATGFA_ERR_BOUNDS; }
    if (flags & kBadLink) { set_error("flip: a link refers to a segment id that is out of range"); return FLATGFA_ERR_BOUNDS; }
    if (flags & kBadOverlap) { set_error("flip: a link has an overlap span outside the alignment pool"); return FLATGFA_ERR_BOUNDS; }
    if (flags & kLongRow) {
        set_error("flip: more than " + std::to_string(j->round_keys) + " links and step pairs share one handle: more than a round of the key table holds");
        return FLATGFA_ERR_TOO_LARGE;
    }
    j->counted = true;
    *n_turned = j->n_turned;
    *links_out = j->old_kept + j->new_kept;
    *links_new = j->new_kept;
    return FLATGFA_OK;
}

int flip_fill(FlipJob *j, uint32_t *steps_out, uint32_t *turned_out, uint32_t *links_out, hipStream_t st) {
    if (!j || !j->counted) { set_error("flip: fill before a successful count"); return FLATGFA_ERR_ARG; }
    const FlipIn &in = j->in;
    if ((in.n_lin && !steps_out) || (in.n_paths && !turned_out) || (j->old_kept + j->new_kept && !links_out)) {
        set_error("flip: NULL output");
        return FLATGFA_ERR_ARG;
    }
    j->mem.st = st;
    if (in.n_lin) {
        ProfScope prof("flip_rewrite", st);
        hipLaunchKernelGGL(k_flip_rewrite, dim3(stride_blocks(j->tiles, 1, kFlipGrid)), dim3(kFlipThreads), 0, st, j->g, j->tiles, j->turned, steps_out);
    }
    if (in.n_paths) FL_HIP(hipMemcpyAsync(turned_out, j->turned, (uint64_t)in.n_paths * 4, hipMemcpyDeviceToDevice, st));
    {
        ProfScope prof("flip_compact", st);
        if (j->old_kept) scan_apply<kFlipThreads, kFlipScanPer, Sum<uint32_t>>(OldOp{j->keep, in.links, links_out}, in.n_links, j->old_sp, st);
        if (j->new_kept) {
            scan_apply<kFlipThreads, kFlipScanPer, Sum<uint32_t>>(NewOp{j->keep + in.n_links, j->cand_start, j->g, j->old_sp.total, (uint32_t)in.n_align, links_out},
                                                                  in.n_lin, j->new_sp, st);
        }
    }
    FL_HIP(hipGetLastError());
    return FLATGFA_OK;
}

}  // namespace fgfa_dev

// ---- the device-level C ABI (include/flatgfa.h Part 3) ----
struct flatgfa_dev_flip {
    fgfa_dev::FlipJob *job = nullptr;
    ~flatgfa_dev_flip() { fgfa_dev::flip_free(job); }
};

extern "C" {

int flatgfa_dev_flip_count(const uint32_t *steps, uint64_t n_steps, const uint32_t *path_start, const uint32_t *path_begin, uint32_t n_paths,
                           uint64_t n_lin, const uint32_t *seg_len, uint32_t n_segs, const uint32_t *links, uint64_t n_links, const uint32_t *alignment, uint64_t n_align,
                           uint64_t round_keys, void *stream, flatgfa_dev_flip_t **job, uint64_t *n_turned, uint64_t *links_out, uint64_t *links_new) {
    if (job) *job = nullptr;
    if (!job || !n_turned || !links_out || !links_new || !path_start) { fgfa_dev::set_error("flatgfa_dev_flip_count: NULL argument"); return FLATGFA_ERR_ARG; }
    fgfa_dev::FlipIn in;
    in.steps = steps, in.n_steps = n_steps;
    in.pstart = path_start, in.pbegin = path_begin, in.n_paths = n_paths, in.n_lin = n_lin;
    in.seg_len = seg_len, in.n_segs = n_segs;
    in.links = links, in.n_links = n_links;
    in.alignment = alignment, in.n_align = n_align;
    auto *h = new flatgfa_dev_flip();
    h->job = fgfa_dev::flip_new(round_keys ? round_keys : fgfa_dev::kFlipRoundKeys);
    const int rc = fgfa_dev::flip_count(h->job, in, (hipStream_t)stream, n_turned, links_out, links_new);
    if (rc) {
        delete h;
        return rc;
    }
    *job = h;
    return FLATGFA_OK;
}

int flatgfa_dev_flip_fill(flatgfa_dev_flip_t *job, uint32_t *steps_out, uint32_t *turned_out, uint32_t *links_out, void *stream) {
    if (!job) { fgfa_dev::set_error("flatgfa_dev_flip_fill: NULL job"); return FLATGFA_ERR_ARG; }
    return fgfa_dev::flip_fill(job->job, steps_out, turned_out, links_out, (hipStream_t)stream);
}

void flatgfa_dev_flip_free(flatgfa_dev_flip_t *job) { delete job; }

}  // extern "C"
