// Pass 1 from a run-length image of the steps: the image's kernels (which steps start a run, how many
// per aligned block of 1024 steps, where they go), the entries a plan's items read, and k_scan_runs, which turns entries into
// the records k_scan makes of the steps themselves.  Plain HIP: no landing registers, no run queue.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "depth_fast_kernels.hpp"
#include "device_scan.hpp"
#include "prof.hpp"
#include "host_copy.hpp"

namespace fgfa_dev {

// The image of one resident step array.  An entry is the first step of a maximal run: consecutive steps whose segment ids go
// up by exactly one, or down by exactly one, cut at every path's begin and end and at every aligned block of kRunBlock steps
// (which is also the most a record's length field holds with 8192-segment windows).  A run's length is the distance to the
// next entry; entry n_ent closes the last run.
struct RunImage {
    uint2 *ent = nullptr;        // [n_ent + 1] {first id | runs down << 31, position in the step array}
    uint32_t *index = nullptr;   // [n_blocks + 1] the first entry of every aligned block; [n_blocks] = n_ent
    uint64_t n_ent = 0, n_blocks = 0, n_steps = 0;
    const uint32_t *steps = nullptr;
    // while it is being made
    uint32_t *cuts = nullptr;    // a bit per step: a path begins or ends here
    uint32_t *blk = nullptr;     // [n_blocks + 1] run starts per block (the last: none)
    Sum<uint32_t>::Wide *aggr = nullptr;
    uint64_t *prefix = nullptr;  // the tiles' prefixes of the scan, and the total behind them
    uint64_t tiles = 0;
    hipEvent_t done = nullptr;
    int phase = 0;               // 1: counted and scanned (enqueued), 2: written (enqueued), 3: there, -1: not to be had
    const char *why = "";        // ... because of this
};

namespace {

constexpr uint32_t kRunBlock = 1024, kRunBlockBits = 10;
constexpr int kImgThreads = 1024;
constexpr uint32_t kScanPer = 4;

__global__ __launch_bounds__(256) void k_run_cuts(const uint32_t *__restrict__ pbeg, const uint32_t *__restrict__ pend, uint32_t n_paths, uint64_t n_steps,
                                                   uint32_t *__restrict__ cuts) {
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n_paths; p += gridDim.x * 256u) {
        const uint32_t b = pbeg[p], e = pend[p];
        if (b < n_steps) atomicOr(&cuts[b >> 5], 1u << (b & 31u));
        if (e < n_steps) atomicOr(&cuts[e >> 5], 1u << (e & 31u));
    }
}

// The later of two marks (block_scan's monoid): a step where the question "does a run start here" has an answer of its own
// carries (position << 1 | answer) + 1 -- a cut or a jump in the ids: yes; the same unit step as before: no -- and a step
// that turns round (up after down, down after up) starts a run exactly if the step before it did not: the answer alternates
// from the last mark on.
struct LastMark {
    uint32_t v;
    __device__ __forceinline__ static LastMark comb(const LastMark &x, const LastMark &y) { return LastMark{max(x.v, y.v)}; }
};

// One workgroup per aligned block, a step per thread.  WRITE: the entries, at index[block] on; else the block's count.
template <bool WRITE>
__global__ __launch_bounds__(kImgThreads) void k_run_starts(const uint32_t *__restrict__ steps, uint64_t n_steps, const uint32_t *__restrict__ cuts, uint64_t n_blocks,
                                                            uint32_t *__restrict__ blk, const uint32_t *__restrict__ index, uint2 *__restrict__ ent, uint64_t n_ent) {
    __shared__ LastMark sh[kImgThreads];
    const uint32_t tid = threadIdx.x;
    if (WRITE && blockIdx.x == 0 && tid == 0) ent[n_ent] = make_uint2(0u, (uint32_t)n_steps);
    for (uint64_t bk = blockIdx.x; bk < n_blocks; bk += gridDim.x) {
        const uint64_t t = bk * kRunBlock + tid;
        const bool in = t < n_steps;
        const uint32_t id = in ? steps[t] >> 1 : 0u;
        const uint32_t idp = in && tid >= 1u ? steps[t - 1] >> 1 : 0u, idpp = in && tid >= 2u ? steps[t - 2] >> 1 : 0u;
        const bool cut = tid == 0u || !in || ((cuts[t >> 5] >> (t & 31u)) & 1u);
        const bool up = id == idp + 1u, down = id + 1u == idp, up_before = idp == idpp + 1u;
        const bool fresh = cut || !(up || down);          // a run starts here whatever came before
        const bool same = !fresh && up == up_before;      // (looked at only where the step before continued a run: it was a unit step then)
        const uint32_t key = fresh ? ((tid << 1) | 1u) + 1u : same ? (tid << 1) + 1u : 0u;
        block_scan<kImgThreads>(sh, LastMark{key});
        const uint32_t m = sh[tid].v - 1u;  // (thread 0 is a mark: never zero)
        bool start = ((m & 1u) ^ ((tid - (m >> 1)) & 1u)) != 0u;
        // (`same` after a step that started a run continues that run, whichever way the step before went: the mark says "no")
        start = start && in;
        if (!WRITE) {
            const int n = __syncthreads_count(start);
            if (tid == 0) blk[bk] = (uint32_t)n;
        } else {
            uint32_t total;
            const uint32_t rank = block_excl_scan<uint32_t, kImgThreads>(start ? 1u : 0u, &total);
            if (start) {
                const bool dn = t + 1 < n_steps && (steps[t + 1] >> 1) + 1u == id;  // (read only where the next step continues the run)
                const uint64_t at = (uint64_t)index[bk] + rank;  // (below n_ent unless the steps changed between the count and this)
                if (at < n_ent) ent[at] = make_uint2(id | (dn ? 0x80000000u : 0u), (uint32_t)t);
            }
        }
        __syncthreads();
    }
}

struct IndexOp {
    const uint32_t *blk;
    uint32_t *index;
    __device__ __forceinline__ Sum<uint32_t> load(uint64_t i) const { return Sum<uint32_t>{blk[i]}; }
    __device__ __forceinline__ void store(uint64_t i, uint32_t before, const Sum<uint32_t> &) const { index[i] = before; }
};

// the entries of the aligned blocks an item's steps lie in: [x, y) of the image
__global__ __launch_bounds__(256) void k_item_entries(const uint4 *__restrict__ items, uint32_t n_items, const uint32_t *__restrict__ index, uint2 *__restrict__ out) {
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < n_items; j += gridDim.x * 256u) {
        const uint4 d = items[j];
        const uint32_t lo = index[d.x >> kRunBlockBits];
        out[j] = make_uint2(lo, d.y > d.x ? index[((uint64_t)d.y + kRunBlock - 1u) >> kRunBlockBits] : lo);
    }
}

// ============================================================ pass 1 from the image ===

// Which item a workgroup walks in its r-th turn: the items are sorted longest first and dealt in snake order (0 .. G-1, then
// G-1 .. 0, ...), and run_wg_of is the other way round.
__host__ __device__ __forceinline__ uint32_t run_item_of(uint32_t round, uint32_t wg, uint32_t n_wg) { return round * n_wg + ((round & 1u) ? n_wg - 1u - wg : wg); }
__host__ __device__ __forceinline__ uint32_t run_wg_of(uint32_t item, uint32_t n_wg) { return ((item / n_wg) & 1u) ? n_wg - 1u - item % n_wg : item % n_wg; }

// How many records k_scan_runs will put into every (window, workgroup) sub-bucket: the same arithmetic as emit_chunk, a
// workgroup per item.  fill: [n_win][n_slots], zeroed; k_run_room_max leaves the fullest in *most.
__global__ __launch_bounds__(256) void k_run_room(const uint4 *__restrict__ items, const uint2 *__restrict__ item_ent, uint32_t n_items, const uint2 *__restrict__ ent,
                                                   uint32_t n_wg, uint32_t n_slots, uint32_t n_segs, uint32_t wb, uint32_t *__restrict__ fill) {
    const uint32_t wmask = (1u << wb) - 1u;
    for (uint32_t j = blockIdx.x; j < n_items; j += gridDim.x) {
        const uint4 d = items[j];
        const uint2 er = item_ent[j];
        const uint32_t wg = run_wg_of(j, n_wg);
        for (uint32_t i = er.x + threadIdx.x; i < er.y; i += 256u) {
            const uint2 en = ent[i];
            const uint32_t s = max(en.y, d.x), t = min(ent[i + 1u].y, d.y);
            if (s >= t) continue;
            const uint32_t skip = s - en.y, lenm1 = t - s - 1u;
            const bool dn = (en.x >> 31) != 0u;
            const uint32_t first = (en.x & 0x7FFFFFFFu) + (dn ? 0u - skip : skip);
            const uint32_t id = dn ? first - lenm1 : first;
            if (id + lenm1 >= n_segs) continue;
            const uint32_t win = id >> wb;
            atomicAdd(&fill[(size_t)win * n_slots + wg], 1u);
            if ((id & wmask) + lenm1 > wmask) atomicAdd(&fill[(size_t)(win + 1u) * n_slots + wg], 1u);
        }
    }
}
__global__ __launch_bounds__(256) void k_run_room_max(const uint32_t *__restrict__ fill, uint64_t n, uint32_t *__restrict__ most) {
    uint32_t m = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) m = max(m, fill[i]);
    if (m) atomicMax(most, m);
}

struct RunScanArgs {
    const uint2 *ent;       // the image's entries
    const uint2 *item_ent;  // [n_items] which of them each item reads
    uint32_t n_ent;
    uint32_t *counts_kept;  // [n_win][n_slots] a second copy of the cursors this call leaves (FastPlan::counts_kept), or null
};

struct RunsWave {
    uint32_t vm[3];  // (put() counts its stores for k_scan's landing registers: nobody looks here)
};

constexpr int kRunsWide = 4;  // chunks of 64 entries a wave takes at a time
// The kernel needs 17 KB of LDS and 50 registers: two of its workgroups fit a CU, and where the dispatcher puts two on one, both
// run at half speed -- with a fixed deal nobody takes their items off them.  It asks for more than half a CU's LDS instead:
// one workgroup per CU, as k_scan (cfg-L, three calls in flight, same box: 0.0704-0.0747 -> 0.0687-0.0702 ms per call).
#ifndef FGFA_RUNS_LDS_MIN
#define FGFA_RUNS_LDS_MIN (84 * 1024)
#endif
constexpr uint32_t kRunsLdsMin = FGFA_RUNS_LDS_MIN;  // dynamic LDS asked for at least

template <bool NT>
__device__ __forceinline__ uint2 load_entry(const uint2 *p) {
    const unsigned long long *q = reinterpret_cast<const unsigned long long *>(p);
    const unsigned long long v = NT ? __builtin_nontemporal_load(q) : *q;
    return make_uint2((uint32_t)v, (uint32_t)(v >> 32));
}

__device__ __forceinline__ uint32_t runs_epoch(uint32_t *ctl) { return __hip_atomic_load(ctl + kCtlEpoch, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP); }

// kRunsWide * 64 consecutive entries from `base` on (those below `hi` count) and the position that closes the last of them
template <bool NT>
__device__ __forceinline__ void load_chunk(const RunScanArgs &R, uint32_t base, int lane, uint2 (&en)[kRunsWide], uint32_t &tail) {
#pragma unroll
    for (int k = 0; k < kRunsWide; ++k) en[k] = load_entry<NT>(R.ent + min(base + 64u * (uint32_t)k + (uint32_t)lane, R.n_ent));
    tail = load_entry<NT>(R.ent + min(base + 64u * (uint32_t)kRunsWide, R.n_ent)).y;
}

// One record per entry (two where the run crosses a window's edge), as k_scan's emit_raw makes them of its queue: the run's
// part inside the item's steps [b, e), from its low end.
template <bool BIG>
__device__ __forceinline__ void emit_chunk(const ScanArgs &A, RunsWave &w, uint32_t *bcur, uint32_t *mine, int lane, uint32_t base, uint32_t hi, uint32_t b, uint32_t e,
                                           uint32_t tagc, const uint2 (&en)[kRunsWide], uint32_t tail) {
    const uint32_t wb = A.wb, wmask = (1u << wb) - 1u;
    bool valid[kRunsWide], cross[kRunsWide];
    uint32_t win[kRunsWide], rel[kRunsWide], lenm1[kRunsWide], pos[kRunsWide];
    bool bad = false, any_cross = false;
#pragma unroll
    for (int k = 0; k < kRunsWide; ++k) {
        uint32_t next = (uint32_t)__shfl_down((int)en[k].y, 1, 64);
        const uint32_t after = k + 1 < kRunsWide ? (uint32_t)__shfl((int)en[k + 1 < kRunsWide ? k + 1 : k].y, 0, 64) : tail;
        next = lane == 63 ? after : next;
        const uint32_t s = max(en[k].y, b), t = min(next, e);
        valid[k] = base + 64u * (uint32_t)k + (uint32_t)lane < hi && s < t;
        const uint32_t skip = valid[k] ? s - en[k].y : 0u;
        lenm1[k] = valid[k] ? t - s - 1u : 0u;
        const bool dn = (en[k].x >> 31) != 0u;
        const uint32_t first = (en[k].x & 0x7FFFFFFFu) + (dn ? 0u - skip : skip);
        const uint32_t id = dn ? first - lenm1[k] : first;  // (a run that goes down by one a step never goes below its last id)
        const bool out = valid[k] && id + lenm1[k] >= A.n_segs;
        bad |= out;
        valid[k] = valid[k] && !out;
        win[k] = id >> wb;
        rel[k] = id & wmask;
        cross[k] = valid[k] && rel[k] + lenm1[k] > wmask;
        any_cross |= cross[k];
    }
    flag_if_any(A, bad, kStBounds);
#pragma unroll
    for (int k = 0; k < kRunsWide; ++k) pos[k] = take_slots(bcur, lane, valid[k], win[k]);
    bool ovf = false;
#pragma unroll
    for (int k = 0; k < kRunsWide; ++k) {
        const uint32_t l1 = cross[k] ? wmask - rel[k] : lenm1[k];
        ovf |= put<false, BIG, false>(A, w, mine, valid[k], pos[k], win[k], rel[k] | (l1 << wb) | tagc);
    }
    if (__builtin_amdgcn_ballot_w64(any_cross)) {
#pragma unroll
        for (int k = 0; k < kRunsWide; ++k) {
            const uint32_t pos2 = cross[k] ? atomicAdd(&bcur[win[k] + 1u], 1u) : 0u;
            ovf |= put<false, BIG, false>(A, w, mine, cross[k], pos2, win[k] + 1u, ((lenm1[k] - (wmask - rel[k]) - 1u) << wb) | tagc);
        }
    }
    flag_if_any(A, ovf, kStOverflow);
}

// Tagged calls of plans whose every path is an item of k_scan.  What it shares with k_scan<kModePlain, true>: the persistent
// workgroups, the tags, the
// gate (a wave appends for its workgroup's item r once every wave has left item r - kTagSlots), the cursors it leaves and
// `taken`.  The waves of a workgroup take chunks of the current item's entries off an LDS counter, a chunk ahead of the one
// they emit; LDS holds the cursors and the control words, nothing else.
template <bool BIG, bool NT>
__global__ __launch_bounds__(kThreads) void k_scan_runs(const ScanArgs A, const RunScanArgs R) {
    constexpr uint32_t kRing = kCtlRing - 1u;
    constexpr uint32_t kPer = 64u * kRunsWide;
    extern __shared__ uint32_t lds[];
    uint32_t *bcur = lds, *ctl = lds + A.nwp;
    const int lane = threadIdx.x & 63;
    uint32_t *mine = A.buckets + (size_t)blockIdx.x * A.cap;
    RunsWave w;
    w.vm[0] = w.vm[1] = w.vm[2] = 0;
    if (A.zero_a) {  // small graphs: pass 2 adds to the outputs (AccArgs::parts)
        for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < A.n_segs; i += gridDim.x * kThreads) {
            A.zero_a[i] = 0u;
            if (A.zero_b) A.zero_b[i] = 0u;
        }
    }
    for (uint32_t i = threadIdx.x; i < A.nwp; i += kThreads) bcur[i] = i < A.n_win ? A.counts[(size_t)i * A.n_slots + blockIdx.x] : 0u;
    if (threadIdx.x < kCtlWords) ctl[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t n_items = A.n_items;
    uint32_t rr = 0, job = run_item_of(0u, blockIdx.x, gridDim.x);
    uint4 d = make_uint4(0u, 0u, 0u, 0u);
    uint2 er = make_uint2(0u, 0u);
    if (job < n_items) {
        d = A.items[job];
        er = R.item_ent[job];
    }
    while (job < n_items) {
        // The workgroup's next item.  The deal is FIXED (sorted items in snake order, run_item_of): which records meet in which
        // sub-bucket is then the same in every call, and the plan has counted, when it installed the image, that they fit
        // (k_run_room) -- a deal that follows the workgroups' speed, as k_scan's does, fills the sub-buckets differently from call
        // to call, and this kernel's workgroups differ more in speed than k_scan's: now and then a sub-bucket sized on k_scan's
        // calls ran over, with hundreds of calls enqueued behind it.
        const uint32_t next_job = rr + 1u < A.tag_limit ? run_item_of(rr + 1u, blockIdx.x, gridDim.x) : n_items;
        const uint32_t next_job_s = __builtin_amdgcn_readfirstlane(next_job);
        uint4 next_d = make_uint4(0u, 0u, 0u, 0u);
        uint2 next_er = make_uint2(0u, 0u);
        if (next_job_s < n_items) {  // (asked for now, looked at behind this item's chunks)
            next_d = A.items[next_job_s];
            next_er = R.item_ent[next_job_s];
        }
        const uint32_t need = rr >= kTagSlots ? rr - (kTagSlots - 1u) : 0u;
        while (runs_epoch(ctl) < need) __builtin_amdgcn_s_sleep(2);
        const uint32_t shared = (d.z & ~kItemNoClaim) >> 1;
        const uint32_t tagc = (uint32_t)__builtin_amdgcn_readfirstlane((d.z >> 31) ? kTagNoClaim : shared ? kTagCount - 1u - shared : rr) << kTagShift;
        const uint32_t b = __builtin_amdgcn_readfirstlane(d.x), e = __builtin_amdgcn_readfirstlane(d.y);
        const uint32_t lo = __builtin_amdgcn_readfirstlane(er.x), hi = __builtin_amdgcn_readfirstlane(er.y);
        uint32_t *next_chunk = &ctl[kCtlNext + (rr & kRing)];
        const auto take = [&]() -> uint32_t {
            uint32_t c = 0;
            if (lane == 0) c = atomicAdd(next_chunk, 1u);
            c = __builtin_amdgcn_readfirstlane(c);
            return c < (hi - lo + kPer - 1u) / kPer ? lo + c * kPer : hi;
        };
        uint32_t base = take();
        uint2 en[kRunsWide];
        uint32_t tail = 0;
        if (base < hi) load_chunk<NT>(R, base, lane, en, tail);
        while (base < hi) {
            const uint32_t base2 = take();
            uint2 en2[kRunsWide];
            uint32_t tail2 = 0;
            if (base2 < hi) load_chunk<NT>(R, base2, lane, en2, tail2);
            emit_chunk<BIG>(A, w, bcur, mine, lane, base, hi, b, e, tagc, en, tail);
#pragma unroll
            for (int k = 0; k < kRunsWide; ++k) en[k] = en2[k];
            tail = tail2;
            base = base2;
        }
        // the last wave to leave the item counts it off
        uint32_t old = 0;
        if (lane == 0) old = __hip_atomic_fetch_add(&ctl[kCtlArrive + (rr & kRing)], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
        old = __builtin_amdgcn_readfirstlane(old);
        if (old == kWaves - 1u) {
            if (lane == 0) {
                ctl[kCtlArrive + (rr & kRing)] = 0u;
                ctl[kCtlNext + (rr & kRing)] = 0u;
            }
            __hip_atomic_store(ctl + kCtlEpoch, rr + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);  // (items complete in order)
        }
        rr += 1u;
        job = next_job_s;
        d = next_d;
        er = next_er;
    }
    __syncthreads();
    // (the cursors twice: pass 2 zeroes `counts` as it reads them, the kept copy stays for the calls that run pass 2 alone)
    for (uint32_t wdw = threadIdx.x; wdw < A.n_win; wdw += kThreads) {
        A.counts[(size_t)wdw * A.n_slots + blockIdx.x] = bcur[wdw];
        if (R.counts_kept) R.counts_kept[(size_t)wdw * A.n_slots + blockIdx.x] = bcur[wdw];
    }
    if (threadIdx.x == 0) {
        A.taken[blockIdx.x] = rr;
        if (run_item_of(rr, blockIdx.x, gridDim.x) < n_items) atomicOr(A.status, kStBackOverflow);  // (out of private tags with items left: the plan's rule keeps such plans away)
    }
}

void image_release_scratch(RunImage *im) {
    for (void **p : {(void **)&im->cuts, (void **)&im->blk, (void **)&im->aggr, (void **)&im->prefix}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
}

bool image_fail(RunImage *im, const char *why) {
    (void)hipGetLastError();
    im->phase = -1;
    im->why = why;
    return false;
}

}  // namespace

RunImage *run_image_start(const flatgfa_dev_graph_t &g, hipStream_t side) {
    auto *im = new RunImage();
    im->steps = g.steps;
    im->n_steps = g.n_steps;
    im->n_blocks = (g.n_steps + kRunBlock - 1) / kRunBlock;
    im->tiles = blocks(im->n_blocks + 1, kImgThreads * kScanPer);
    const uint64_t cut_words = g.n_steps / 32 + 1;
    hipError_t e = hipMalloc(&im->cuts, cut_words * 4);
    if (e == hipSuccess) e = hipMalloc(&im->blk, (im->n_blocks + 1) * 4);
    if (e == hipSuccess) e = hipMalloc(&im->index, (im->n_blocks + 1) * 4);
    if (e == hipSuccess) e = hipMalloc(&im->aggr, std::max<uint64_t>(im->tiles, 1) * sizeof(*im->aggr));
    if (e == hipSuccess) e = hipMalloc(&im->prefix, (im->tiles + 1) * 8);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&im->done, hipEventDisableTiming);
    if (e != hipSuccess) {
        image_fail(im, "memory");
        return im;
    }
    int dev = 0;
    (void)hipGetDevice(&dev);
    const uint32_t cus = (uint32_t)device_cu_count(dev);
    {
        ProfScope ps("run_image_count", side);
        e = hipMemsetAsync(im->cuts, 0, cut_words * 4, side);
        if (e == hipSuccess) e = hipMemsetAsync(im->blk + im->n_blocks, 0, 4, side);
        if (e != hipSuccess) {
            image_fail(im, "error");
            return im;
        }
        if (g.n_paths) hipLaunchKernelGGL(k_run_cuts, dim3(stride_blocks(g.n_paths, 256, cus * 8u)), dim3(256), 0, side, g.path_begin, g.path_end, g.n_paths, g.n_steps, im->cuts);
        if (im->n_blocks)
            hipLaunchKernelGGL((k_run_starts<false>), dim3(stride_blocks(im->n_blocks, 1, cus * 2u)), dim3(kImgThreads), 0, side, g.steps, g.n_steps, im->cuts, im->n_blocks,
                               im->blk, (const uint32_t *)nullptr, (uint2 *)nullptr, (uint64_t)0);
        Spine<Sum<uint32_t>> sp;
        sp.aggr = im->aggr;
        sp.prefix = im->prefix;
        sp.total = im->prefix + im->tiles;
        const IndexOp op{im->blk, im->index};
        scan_count<kImgThreads, kScanPer, Sum<uint32_t>>(op, im->n_blocks + 1, sp, side);
        scan_apply<kImgThreads, kScanPer, Sum<uint32_t>>(op, im->n_blocks + 1, sp, side);
    }
    if (hipEventRecord(im->done, side) != hipSuccess || hipGetLastError() != hipSuccess) {
        (void)hipStreamSynchronize(side);
        image_fail(im, "error");
        return im;
    }
    im->phase = 1;
    return im;
}

int run_image_poll(RunImage *im, hipStream_t side, bool wait, uint64_t reserve, bool any_ratio) {
    for (;;) {
        if (im->phase == 3) return 1;
        if (im->phase < 1) return -1;
        if (wait) {
            if (hipEventSynchronize(im->done) != hipSuccess) { image_fail(im, "error"); return -1; }
        } else {
            const hipError_t q = hipEventQuery(im->done);
            if (q != hipSuccess) {
                (void)hipGetLastError();
                return 0;
            }
        }
        if (im->phase == 2) {
            image_release_scratch(im);
            im->phase = 3;
            return 1;
        }
        // counted: how many entries, and whether that is worth having -- at most one for four steps, and what the device has room for
        uint64_t total = 0;
        if (staged_copy(&total, im->prefix + im->tiles, 8, hipMemcpyDeviceToHost, nullptr) != hipSuccess) { image_fail(im, "error"); return -1; }
        im->n_ent = total;
        if ((!any_ratio && (total + 1) * 8 > im->n_steps * 2) || total >= (1ull << 32) - 4096) {  // (k_scan_runs counts entries in 32 bits)
            image_release_scratch(im);
            image_fail(im, "runs");
            return -1;
        }
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
            (void)hipGetLastError();
            free_b = 0;
        }
        if ((total + 1) * 8 + reserve > free_b) {
            image_release_scratch(im);
            image_fail(im, "memory");
            return -1;
        }
        if (hipMalloc(&im->ent, (total + 1) * 8) != hipSuccess) {
            image_release_scratch(im);
            image_fail(im, "memory");
            return -1;
        }
        int dev = 0;
        (void)hipGetDevice(&dev);
        const uint32_t cus = (uint32_t)device_cu_count(dev);
        {
            ProfScope ps("run_image_write", side);
            hipLaunchKernelGGL((k_run_starts<true>), dim3(stride_blocks(im->n_blocks, 1, cus * 2u)), dim3(kImgThreads), 0, side, im->steps, im->n_steps, im->cuts, im->n_blocks,
                               (uint32_t *)nullptr, im->index, im->ent, total);
        }
        if (hipEventRecord(im->done, side) != hipSuccess || hipGetLastError() != hipSuccess) {
            (void)hipStreamSynchronize(side);
            image_release_scratch(im);
            image_fail(im, "error");
            return -1;
        }
        im->phase = 2;
    }
}

const char *run_image_why(const RunImage *im) { return im->why; }
uint64_t run_image_bytes(const RunImage *im) { return im->phase == 3 ? (im->n_ent + 1) * 8 + (im->n_blocks + 1) * 4 : 0; }

void run_image_free(RunImage *im, hipStream_t side) {
    if (!im) return;
    if (im->phase == 1 || im->phase == 2) (void)hipStreamSynchronize(side);
    image_release_scratch(im);
    if (im->ent) (void)hipFree(im->ent);
    if (im->index) (void)hipFree(im->index);
    if (im->done) (void)hipEventDestroy(im->done);
    delete im;
}

bool run_items_start(const FastPlan &fp, const RunImage *im, hipStream_t side, void **item_ent, void **room, hipEvent_t *done) {
    *item_ent = *room = nullptr;
    *done = nullptr;
    if (im->phase != 3 || !fp.n_items) return false;
    const uint64_t n_fill = (uint64_t)fp.n_win * fp.n_slots;
    const auto fail = [&]() {
        (void)hipGetLastError();
        if (*item_ent) (void)hipFree(*item_ent);
        if (*room) (void)hipFree(*room);
        if (*done) (void)hipEventDestroy(*done);
        *item_ent = *room = nullptr;
        *done = nullptr;
        return false;
    };
    if (hipMalloc(item_ent, (size_t)fp.n_items * sizeof(uint2)) != hipSuccess || hipMalloc(room, (n_fill + 1) * 4) != hipSuccess ||
        hipEventCreateWithFlags(done, hipEventDisableTiming) != hipSuccess || hipMemsetAsync(*room, 0, (n_fill + 1) * 4, side) != hipSuccess)
        return fail();
    const uint4 *items = reinterpret_cast<const uint4 *>(fp.items);
    uint32_t *fill = reinterpret_cast<uint32_t *>(*room);
    hipLaunchKernelGGL(k_item_entries, dim3(stride_blocks(fp.n_items, 256, fp.n_cus * 8u)), dim3(256), 0, side, items, fp.n_items, im->index, reinterpret_cast<uint2 *>(*item_ent));
    // ... and the room its records will need with k_scan_runs' fixed deal on the plan's workgroups (run_range's grid)
    const uint32_t n_wg = std::min<uint32_t>(fp.n_items, fp.n_slots);
    hipLaunchKernelGGL(k_run_room, dim3(std::min<uint32_t>(fp.n_items, fp.n_cus * 8u)), dim3(256), 0, side, items, reinterpret_cast<const uint2 *>(*item_ent), fp.n_items,
                       im->ent, n_wg, fp.n_slots, fp.n_range, fp.wb, fill);
    hipLaunchKernelGGL(k_run_room_max, dim3(stride_blocks(n_fill, 256, fp.n_cus * 4u)), dim3(256), 0, side, fill, n_fill, fill + n_fill);
    if (hipEventRecord(*done, side) != hipSuccess || hipGetLastError() != hipSuccess) {
        (void)hipStreamSynchronize(side);
        return fail();
    }
    return true;
}

// the fullest sub-bucket k_run_room counted (behind run_items_start's event); ~0 on an error
uint32_t run_room_needed(const FastPlan &fp, const void *room) {
    uint32_t most = ~0u;
    if (staged_copy(&most, reinterpret_cast<const uint32_t *>(room) + (uint64_t)fp.n_win * fp.n_slots, 4, hipMemcpyDeviceToHost, nullptr) != hipSuccess) {
        (void)hipGetLastError();
        return ~0u;
    }
    return most;
}

void run_image_install(FastPlan *fp, const RunImage *im, void *item_ent, bool nt) {
    fp->run_ent = im->ent;
    fp->run_n_ent = (uint32_t)im->n_ent;
    fp->run_item_ent = item_ent;
    fp->run_nt = nt;
}

void launch_scan_runs(const FastPlan &fp, const ScanArgs &sa, uint32_t grid, hipStream_t stream) {
    const dim3 g(grid), b(kThreads);
    const uint32_t lds = std::max<uint32_t>((fp.nwp + kCtlWords) * 4u, kRunsLdsMin);
    if (lds > 64u * 1024u) {
        static OncePerDevice once;
        (void)once([] {
            bool good = true;
            for (const void *k : {(const void *)k_scan_runs<true, true>, (const void *)k_scan_runs<true, false>, (const void *)k_scan_runs<false, true>, (const void *)k_scan_runs<false, false>})
                good = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit) == hipSuccess && good;
            return good;
        });
    }
    const RunScanArgs ra{reinterpret_cast<const uint2 *>(fp.run_ent), reinterpret_cast<const uint2 *>(fp.run_item_ent), fp.run_n_ent, fp.counts_kept};
    if (sa.big && fp.run_nt) hipLaunchKernelGGL((k_scan_runs<true, true>), g, b, lds, stream, sa, ra);
    else if (sa.big) hipLaunchKernelGGL((k_scan_runs<true, false>), g, b, lds, stream, sa, ra);
    else if (fp.run_nt) hipLaunchKernelGGL((k_scan_runs<false, true>), g, b, lds, stream, sa, ra);
    else hipLaunchKernelGGL((k_scan_runs<false, false>), g, b, lds, stream, sa, ra);
}

}  // namespace fgfa_dev
