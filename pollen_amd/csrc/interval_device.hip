// Interval and window depth over many paths on gfx950 (flatgfa/src/ops/window_depth.rs:84-147).
//
// The reference's two-pointer loop over (steps of a path, intervals) has a closed form per interval: with step j of the path
// on [r0_j, r1_j) and M = the largest end among the intervals before this one in its group (0 for the group's first),
//   out = the sum, in increasing j from +0.0, over the steps with min(end, r1_j) > max(start, r0_j) and r1_j >= M of
//         ((f64)(depth_j * len_j) * ((f64)(o1 - o0) / (f64)len_j)) / (f64)(end - start).
// Those steps are one contiguous range, which starts at the first step with r1_j >= max(start + 1, M).
//
//   k_scan         (device_scan.hpp) twice: over the intervals, the running maximum of the ends that restarts at every group's
//                  first interval (MaxOp), and per batch over the steps of the paths the batch names, laid one behind another,
//                  the sum of the segment lengths that restarts at every path's first step (PosOp): the step end positions r1,
//                  8 bytes a step.  r0_j is r1 of the step before (0 at a path's first), len_j their difference.
//   k_slots        the batch's paths get their slots: where a path's end positions lie and where its steps begin.
//   k_intervals    one lane per interval: the binary search for the first step, then the walk -- up to lane_cut steps; an
//                  interval that has more goes to the list of long ones with its first step.
//   k_long         one wave per long interval: 64 consecutive steps per round, one per lane (coalesced end positions and steps,
//                  gathered depths), 64 terms, added in lane order by every lane alike.
// The terms are computed in any order; the additions are made in step order, one at a time: f64 addition is not associative.
// Kernels never trap: a bad step raises a bit of the flag word and counts as a step of no length.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/flatgfa.h"
#include "device_common.hpp"
#include "device_scan.hpp"
#include "flatgfa_core.hpp"
#include "host_copy.hpp"
#include "interval_device.hpp"
#include "prof.hpp"

// IEEE double throughout: no contraction into fma, no reassociation (HIP device code defaults to -ffp-contract=fast).
#pragma clang fp contract(off)

namespace fgfa_dev {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kPer = 4;  // consecutive elements per lane
constexpr uint32_t kTile = kThreads * kPer;
constexpr uint32_t kMaxGrid = 2048;   // workgroups of a grid-stride launch
constexpr uint32_t kLongGrid = 1024;  // ... of k_long: four waves each

// flag word bits
constexpr uint32_t kBadStep = 1;

// A segmented scan value (device_scan.hpp): F over the stretch, and whether a head lies in it (a head restarts F).
template <class F>
struct Seg {
    using Carry = uint64_t;
    using Wide = Seg;
    uint64_t v;
    uint32_t f;
    __device__ __forceinline__ static Seg zero() { return Seg{0, 0u}; }  // (0 is the identity of both F below)
    __device__ __forceinline__ static Seg comb(const Seg &x, const Seg &y) {
        if (y.f) return Seg{y.v, 1u};
        return Seg{F::op(x.v, y.v), x.f};
    }
    __device__ __forceinline__ uint64_t carry() const { return v; }
    __device__ __forceinline__ static Seg widen(const Seg &x) { return x; }
    __device__ __forceinline__ static Seg after(uint64_t c) { return Seg{c, 0u}; }
};
struct AddF {
    __device__ __forceinline__ static uint64_t op(uint64_t a, uint64_t b) { return a + b; }
};
struct MaxF {
    __device__ __forceinline__ static uint64_t op(uint64_t a, uint64_t b) { return a > b ? a : b; }
};
using SegSum = Seg<AddF>;
using SegMax = Seg<MaxF>;

// The paths a batch names, one slot each: slot k holds path path[k], whose end positions are pos[pstart[k] .. pstart[k + 1])
// and whose steps begin at steps[sbegin[k]].
struct Slots {
    const uint32_t *path = nullptr;    // u32[n]
    const uint32_t *pstart = nullptr;  // u32[n + 1]
    const uint32_t *sbegin = nullptr;  // u32[n]
    uint32_t *tile_slot = nullptr;     // u32[tiles + 1]: the slot of every scan tile's first step
    uint32_t n = 0;
};

// ---- M: mprev[i] = the largest end among the intervals before i in its group, 0 for the group's first ----
struct MaxOp {
    const uint32_t *path_id;
    const uint64_t *end;
    uint64_t *mprev;
    __device__ SegMax load(uint64_t i) const { return SegMax{end[i], i == 0 || path_id[i] != path_id[i - 1] ? 1u : 0u}; }
    __device__ void store(uint64_t i, uint64_t before, const SegMax &me) const { mprev[i] = me.f ? 0 : before; }
};

// ---- step end positions: an inclusive scan of the steps' segment lengths that restarts at every slot's first step ----
struct PosOp {
    const uint32_t *steps, *seg_len;
    uint32_t n_segs;
    Slots sl;
    uint32_t *flags;
    uint64_t *pos;
    __device__ SegSum load(uint64_t j) const {
        const uint64_t t = j / kTile;
        const uint32_t k = last_start_at_or_before(sl.pstart, sl.tile_slot[t], sl.tile_slot[t + 1], j);
        const uint32_t s = steps[(uint64_t)sl.sbegin[k] + (j - sl.pstart[k])] >> 1;
        uint64_t len = 0;
        if (s < n_segs) len = seg_len[s];
        else atomicOr(flags, kBadStep);
        return SegSum{len, j == sl.pstart[k] ? 1u : 0u};
    }
    __device__ void store(uint64_t j, uint64_t before, const SegSum &me) const { pos[j] = (me.f ? 0 : before) + me.v; }
};

__global__ __launch_bounds__(kThreads) void k_slots(Slots sl, uint32_t *__restrict__ slot_of) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k < sl.n) slot_of[sl.path[k]] = k;
}

__global__ __launch_bounds__(kThreads) void k_tile_slots(Slots sl, uint64_t tiles) {
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t > tiles) return;
    sl.tile_slot[t] = t < tiles ? last_start_at_or_before(sl.pstart, 0, sl.n - 1, t * kTile) : sl.n - 1;
}

struct View {
    const uint32_t *steps, *depth;
    uint32_t n_segs;
    const uint32_t *path_id;
    const uint64_t *start, *end, *mprev;
    const uint32_t *slot_of, *pstart, *sbegin;
    const uint64_t *pos;
};

// What step j of a path (end positions e0 before it and e1 at it, handle h) adds to the interval [ws, we): false when nothing.
__device__ __forceinline__ bool term_of(const View &v, uint32_t h, uint64_t e0, uint64_t e1, uint64_t ws, uint64_t we, double *term) {
    const uint64_t o0 = ws > e0 ? ws : e0, o1 = we < e1 ? we : e1;
    if (o1 <= o0) return false;  // (a step of no length among them)
    const uint32_t s = h >> 1;
    const uint64_t len = e1 - e0, d = s < v.n_segs ? v.depth[s] : 0;  // (a bad step was flagged by the scan)
    const double sdepth = (double)(d * len);                           // weighted_depths, window_depth.rs:93-100
    const double amt = (double)(o1 - o0) / (double)len;                // assign_depths, :130-133
    *term = (sdepth * amt) / (double)(we - ws);
    return true;
}

__global__ __launch_bounds__(kThreads) void k_intervals(View v, uint64_t i0, uint64_t i1, uint32_t lane_cut, uint2 *__restrict__ list,
                                                        uint32_t *count, double *__restrict__ out) {
    for (uint64_t i = i0 + (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < i1; i += (uint64_t)gridDim.x * kThreads) {
        const uint64_t ws = v.start[i], we = v.end[i];
        const uint32_t k = v.slot_of[v.path_id[i]];
        const uint32_t lo = v.pstart[k], hi = v.pstart[k + 1];
        double sum = 0.0;
        bool is_long = false;
        uint32_t first = lo;
        if (we > ws && hi > lo) {
            const uint64_t m = v.mprev[i], want = ws + 1 > m ? ws + 1 : m;  // (ws < we: no wrap)
            uint32_t a = lo, b = hi;
            while (a < b) {  // the first step that ends at or past `want`
                const uint32_t mid = a + ((b - a) >> 1);
                if (v.pos[mid] < want) a = mid + 1;
                else b = mid;
            }
            first = a;
            const uint32_t *steps = v.steps + v.sbegin[k];
            uint64_t e0 = first > lo ? v.pos[first - 1] : 0;
            uint32_t walked = 0;
            for (uint32_t j = first; j < hi && e0 < we; ++j, ++walked) {
                if (walked == lane_cut) {
                    is_long = true;
                    break;
                }
                const uint64_t e1 = v.pos[j];
                double term;
                if (term_of(v, steps[j - lo], e0, e1, ws, we, &term)) sum += term;
                e0 = e1;
            }
        }
        if (is_long) list[atomicAdd(count, 1u)] = make_uint2((uint32_t)(i - i0), first);
        else out[i] = sum;
    }
}

__global__ __launch_bounds__(kThreads) void k_long(View v, uint64_t i0, const uint2 *__restrict__ list, const uint32_t *__restrict__ count,
                                                   double *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63, n = *count;
    const uint32_t waves = gridDim.x * (kThreads / 64);
    for (uint32_t w = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); w < n; w += waves) {  // (the same for a wave's lanes)
        const uint2 rec = list[w];
        const uint64_t i = i0 + rec.x, ws = v.start[i], we = v.end[i];
        const uint32_t k = v.slot_of[v.path_id[i]];
        const uint32_t lo = v.pstart[k], hi = v.pstart[k + 1];
        const uint32_t *steps = v.steps + v.sbegin[k];
        double sum = 0.0;
        for (uint64_t base = rec.y; base < hi; base += 64) {
            const uint64_t j = base + lane;
            bool live = false, has = false;
            double term = 0.0;
            if (j < hi) {
                const uint64_t e0 = j > lo ? v.pos[j - 1] : 0;
                live = e0 < we;
                if (live) has = term_of(v, steps[j - lo], e0, v.pos[j], ws, we, &term);
            }
            unsigned long long todo = __ballot(has);
            while (todo) {  // in lane order, which is step order
                const int l = __ffsll(todo) - 1;
                sum += __shfl(term, l, 64);
                todo &= todo - 1;
            }
            if (!((__ballot(live) >> 63) & 1ull)) break;  // the round's last step lies past the interval, or past the path
        }
        if (lane == 0) out[i] = sum;
    }
}

}  // namespace

#define IV_HIP(expr) FGFA_HIP("interval depth: ", expr)

struct IntervalJob {
    uint64_t scratch_steps = kIntervalScratchSteps;
    uint32_t lane_cut = kIntervalLaneCut;
    uint64_t batches = 0;
};

IntervalJob *interval_new(uint64_t scratch_steps, uint32_t lane_cut) {
    IntervalJob *j = new IntervalJob();
    j->scratch_steps = std::min<uint64_t>(std::max<uint64_t>(scratch_steps, 1), 0xFFFFFFFFull);  // (a batch's steps are numbered in 32 bits)
    j->lane_cut = lane_cut;
    return j;
}
void interval_free(IntervalJob *j) { delete j; }
uint64_t interval_batches(const IntervalJob *j) { return j->batches; }

int interval_depth(IntervalJob *job, const IntervalGraph &g, const IntervalList &iv, const uint32_t *h_path, hipStream_t st, double *out) {
    job->batches = 0;
    const uint64_t n = iv.n;
    if (!n) return FLATGFA_OK;
    if (n > 0xFFFFFFFFull) {
        set_error("interval depth: more than 2^32 - 1 intervals in one call");
        return FLATGFA_ERR_TOO_LARGE;
    }
    // ---- the plan: whole groups, in order, as long as their paths' steps fit the scratch ----
    std::vector<uint32_t> paths;  // the batches' slots, one batch behind another
    std::vector<fgfa::IntervalBatch> plan;
    std::string err;
    if (!fgfa::plan_interval_batches(h_path, n, g.begin, g.end, g.n_paths, g.n_steps, job->scratch_steps, &paths, &plan, &err)) {
        set_error("interval depth: " + err);
        return FLATGFA_ERR_BOUNDS;
    }
    uint64_t max_lin = 0;
    size_t max_slots = 0;
    for (const fgfa::IntervalBatch &b : plan) {
        max_lin = std::max(max_lin, b.n_steps);
        max_slots = std::max(max_slots, b.s1 - b.s0);
    }
    if (max_lin > 0xFFFFFFFFull) {  // (one path has fewer; a batch of several holds at most scratch_steps)
        set_error("interval depth: a batch of more than 2^32 - 1 steps");
        return FLATGFA_ERR_TOO_LARGE;
    }
    // ---- scratch ----
    DeviceMem mem;
    mem.st = st;
    const uint64_t max_tiles = blocks(max_lin, kTile);
    uint64_t *mprev = nullptr, *pos = nullptr;
    uint32_t *slot_of = nullptr, *up = nullptr, *tile_slot = nullptr, *words = nullptr;
    uint2 *list = nullptr;
    Spine<SegMax> m_sp;
    Spine<SegSum> p_sp;
    IV_HIP(mem.alloc(&mprev, n));
    IV_HIP(mem.alloc(&pos, max_lin));
    IV_HIP(mem.alloc(&slot_of, g.n_paths));
    IV_HIP(mem.alloc(&up, 3 * max_slots + 1));  // a batch's paths, then its pstart, then where its paths' steps begin
    IV_HIP(mem.alloc(&tile_slot, max_tiles + 1));
    IV_HIP(mem.alloc(&words, 4));  // flags, long intervals
    IV_HIP(mem.alloc(&list, n));
    IV_HIP(m_sp.alloc(&mem, blocks(n, kTile)));
    IV_HIP(p_sp.alloc(&mem, max_tiles));
    IV_HIP(hipMemsetAsync(words, 0, 16, st));
    {
        ProfScope prof("interval_max_scan", st);
        const MaxOp op{iv.path_id, iv.end, mprev};
        scan_count<kThreads, kPer>(op, n, m_sp, st);
        scan_apply<kThreads, kPer>(op, n, m_sp, st);
    }
    IV_HIP(hipGetLastError());
    std::vector<uint32_t> h_up;
    for (const fgfa::IntervalBatch &b : plan) {
        const uint32_t ns = (uint32_t)(b.s1 - b.s0);
        h_up.assign(paths.begin() + b.s0, paths.begin() + b.s1);
        uint64_t at = 0;
        for (uint32_t k = 0; k < ns; ++k) {
            h_up.push_back((uint32_t)at);
            at += g.end[paths[b.s0 + k]] - g.begin[paths[b.s0 + k]];
        }
        h_up.push_back((uint32_t)at);
        for (uint32_t k = 0; k < ns; ++k) h_up.push_back(g.begin[paths[b.s0 + k]]);
        IV_HIP(staged_copy(up, h_up.data(), h_up.size() * 4, hipMemcpyHostToDevice, st));
        Slots sl;
        sl.path = up, sl.pstart = up + ns, sl.sbegin = up + 2 * ns + 1, sl.tile_slot = tile_slot, sl.n = ns;
        const uint64_t tiles = blocks(b.n_steps, kTile);
        {
            ProfScope prof("interval_positions", st);
            hipLaunchKernelGGL(k_slots, dim3((uint32_t)blocks(ns, kThreads)), dim3(kThreads), 0, st, sl, slot_of);
            if (b.n_steps) {
                hipLaunchKernelGGL(k_tile_slots, dim3((uint32_t)blocks(tiles + 1, kThreads)), dim3(kThreads), 0, st, sl, tiles);
                const PosOp op{g.steps, g.seg_len, g.n_segs, sl, words, pos};
                scan_count<kThreads, kPer>(op, b.n_steps, p_sp, st);
                scan_apply<kThreads, kPer>(op, b.n_steps, p_sp, st);
            }
        }
        IV_HIP(hipGetLastError());
        const View v{g.steps, g.depth, g.n_segs, iv.path_id, iv.start, iv.end, mprev, slot_of, sl.pstart, sl.sbegin, pos};
        const uint64_t ni = b.i1 - b.i0;
        {
            ProfScope prof("interval_depth", st);
            IV_HIP(hipMemsetAsync(words + 1, 0, 4, st));
            hipLaunchKernelGGL(k_intervals, dim3(stride_blocks(ni, kThreads, kMaxGrid)), dim3(kThreads), 0, st, v, b.i0, b.i1, job->lane_cut, list,
                               words + 1, out);
            hipLaunchKernelGGL(k_long, dim3(stride_blocks(ni, kThreads / 64, kLongGrid)), dim3(kThreads), 0, st, v, b.i0, list, words + 1, out);
        }
        IV_HIP(hipGetLastError());
        ++job->batches;
    }
    uint32_t f = 0;
    IV_HIP(staged_copy(&f, words, 4, hipMemcpyDeviceToHost, st));
    if (f & kBadStep) {
        set_error("interval depth: a step refers to a segment id that is out of range");
        return FLATGFA_ERR_BOUNDS;
    }
    return FLATGFA_OK;
}

}  // namespace fgfa_dev
