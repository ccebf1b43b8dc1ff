// Extract and position on gfx950 (flatgfa/src/ops/extract.rs, ops/position.rs).
//
//   k_bfs_level   one pass over the links per level: a link with one end in the frontier and the other outside the map offers
//                 the outside segment the key (rank of the frontier segment << 32 | link index) by a 64-bit atomicMin; the
//                 first offer to a segment also appends it to the level's candidate list.  The candidates come back with their
//                 keys, are ordered by key (the order in which the reference's LIFO walk meets them) and committed with their
//                 new ids and their ranks for the next level.
//   k_scan        (device_scan.hpp) the one scan all the rest is built from: a tile of 1024 elements per workgroup, a pair of
//                 64-bit sums and a head flag per element (SV; a head restarts the sums: the segmented scan), in three launches
//                 -- the tiles' aggregates, k_spine over the aggregates, the tiles again with their prefixes.  PosOp: base positions of
//                 the steps per path.  StepOp: member steps and run starts, writing the translated steps and one record per
//                 subpath.  LinkOp: kept links and their alignment ops, writing the translated links.
//   k_gather      variable-length copies by output tile (sequences, optional data, alignment ops, paths laid out one behind another):
//                 every workgroup writes 4096 consecutive output elements whatever the items' lengths.
// Kernels never trap: a bad step, link or span raises a bit of the flag word.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/flatgfa.h"
#include "device_common.hpp"
#include "device_scan.hpp"
#include "extract_device.hpp"
#include "host_copy.hpp"

namespace fgfa_dev {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kPer = 4;  // consecutive elements per lane
constexpr uint32_t kTile = kThreads * kPer;
constexpr uint32_t kMaxGrid = 256 * 8;  // workgroups of a grid-stride launch
constexpr uint32_t kGatherPer = 16;
constexpr uint32_t kGatherTile = kThreads * kGatherPer;
constexpr uint32_t kNoRank = 0xFFFFFFFFu;
constexpr uint64_t kNoKey = ~0ull;

// flag word bits
constexpr uint32_t kBadStep = 1, kBadLink = 2, kBadSpan = 4;

struct U2 {
    uint64_t a, b;
};
struct SV {  // a scan value (device_scan.hpp): two sums, and whether a head lies in the stretch they cover
    using Carry = U2;
    using Wide = SV;
    U2 v;
    uint32_t f;
    __device__ __forceinline__ static SV zero() { return SV{{0, 0}, 0u}; }
    __device__ __forceinline__ static SV comb(const SV &x, const SV &y) {
        if (y.f) return SV{y.v, 1u};
        return SV{{x.v.a + y.v.a, x.v.b + y.v.b}, x.f};
    }
    __device__ __forceinline__ U2 carry() const { return v; }
    __device__ __forceinline__ static SV widen(const SV &x) { return x; }
    __device__ __forceinline__ static SV after(const U2 &c) { return SV{c, 0u}; }
};

__device__ __forceinline__ bool head_at(const uint32_t *heads, uint64_t i) { return (heads[i >> 5] >> (i & 31)) & 1u; }

// ---- positions: an exclusive scan of the steps' segment lengths that restarts at every path's first step ----
struct PosOp {
    const uint32_t *steps, *heads, *seg_seq;
    uint32_t n_segs;
    uint32_t *flags;
    uint64_t *pos;
    __device__ SV load(uint64_t i) const {
        const uint32_t s = steps[i] >> 1;
        uint64_t len = 0;
        if (s < n_segs) len = seg_seq[2 * (uint64_t)s + 1];
        else atomicOr(flags, kBadStep);
        return SV{{len, 0}, heads && head_at(heads, i) ? 1u : 0u};
    }
    __device__ void store(uint64_t i, const U2 &before, const SV &me) const { pos[i] = me.f ? 0 : before.a; }
};

// ---- subpaths (find_subpaths, extract.rs:102-134): a = member steps, b = run starts ----
struct StepOp {
    const uint32_t *steps, *heads, *state, *seg_seq, *pstart;
    const uint64_t *pos;
    uint32_t n_paths;
    uint64_t n;
    uint32_t *out_steps;
    SubpathRec *recs;
    __device__ bool member(uint64_t i) const { return state[steps[i] >> 1] != 0; }
    __device__ SV load(uint64_t i) const {
        const bool m = member(i);
        const bool s = m && (i == 0 || head_at(heads, i) || !member(i - 1));
        return SV{{m ? 1u : 0u, s ? 1u : 0u}, 0u};
    }
    __device__ void store(uint64_t i, const U2 &before, const SV &me) const {
        if (!me.v.a) return;
        const uint32_t h = steps[i], s = h >> 1;
        out_steps[before.a] = ((state[s] - 1) << 1) | (h & 1u);  // tr_handle, extract.rs:137-140
        if (me.v.b) {
            SubpathRec &r = recs[before.b];
            r.path = last_start_at_or_before(pstart, 0, n_paths - 1, i);  // (n_steps = pstart[n_paths]: where there is a step there is a path)
            r.start = pos[i];
            r.step_begin = before.a;
        }
        if (i + 1 == n || head_at(heads, i + 1) || !member(i + 1)) {
            SubpathRec &r = recs[before.b + me.v.b - 1];
            r.end = pos[i] + seg_seq[2 * (uint64_t)s + 1];
            r.step_end = before.a + 1;
        }
    }
};

// ---- links (extract.rs:188-192, include_link :48-53): a = kept links, b = their alignment ops ----
struct LinkOp {
    const uint32_t *links, *state;
    uint64_t n_align;
    uint32_t *flags;
    uint32_t *out_links, *al_src, *al_dst;
    __device__ SV load(uint64_t i) const {
        const uint32_t *l = links + i * 4;
        if (!state[l[0] >> 1] || !state[l[1] >> 1]) return SV::zero();
        if (l[2] > l[3] || l[3] > n_align) {
            atomicOr(flags, kBadSpan);
            return SV{{1, 0}, 0u};
        }
        return SV{{1, (uint64_t)(l[3] - l[2])}, 0u};
    }
    __device__ void store(uint64_t i, const U2 &before, const SV &me) const {
        if (!me.v.a) return;
        const uint32_t *l = links + i * 4;
        uint32_t *o = out_links + before.a * 4;
        o[0] = ((state[l[0] >> 1] - 1) << 1) | (l[0] & 1u);
        o[1] = ((state[l[1] >> 1] - 1) << 1) | (l[1] & 1u);
        o[2] = (uint32_t)before.b;
        o[3] = (uint32_t)(before.b + me.v.b);
        al_src[before.a] = l[2];
        al_dst[before.a] = (uint32_t)before.b;
    }
};

__global__ __launch_bounds__(kThreads) void k_heads(const uint32_t *__restrict__ pstart, uint32_t n_paths, uint32_t *heads) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n_paths) return;
    const uint32_t b = pstart[p];
    if (b < pstart[p + 1]) atomicOr(heads + (b >> 5), 1u << (b & 31));
}

// Link::incident_seg (flatgfa.rs:137-145) for every frontier segment at once.  A self-loop offers nothing.
__global__ __launch_bounds__(kThreads) void k_bfs_level(const uint32_t *__restrict__ links, uint64_t n_links, const uint32_t *__restrict__ state,
                                                        const uint32_t *__restrict__ rank, unsigned long long *key, uint32_t *cand,
                                                        uint32_t *count) {
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n_links; i += (uint64_t)gridDim.x * kThreads) {
        const uint32_t f = links[i * 4] >> 1, t = links[i * 4 + 1] >> 1;
        if (f == t) continue;
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const uint32_t p = side ? t : f, o = side ? f : t;
            const uint32_t r = rank[p];
            if (r == kNoRank || state[o]) continue;
            const unsigned long long k = ((unsigned long long)r << 32) | (uint32_t)i;
            if (atomicMin(key + o, k) == kNoKey) cand[atomicAdd(count, 1u)] = o;
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_collect(const uint32_t *__restrict__ cand, uint32_t n, const unsigned long long *__restrict__ key,
                                                      U2 *__restrict__ pairs) {
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
    if (j < n) pairs[j] = U2{key[cand[j]], cand[j]};
}

// list[j] takes new id base + j; with_rank: it is also the next frontier, popped from the back (extract.rs:166)
__global__ __launch_bounds__(kThreads) void k_commit(const uint32_t *__restrict__ list, uint64_t n, uint64_t base, uint32_t *state, uint32_t *rank,
                                                     bool with_rank) {
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= n) return;
    state[list[j]] = (uint32_t)(base + j + 1);
    if (with_rank) rank[list[j]] = (uint32_t)(n - 1 - j);
}

__global__ __launch_bounds__(kThreads) void k_clear_rank(const uint32_t *__restrict__ list, uint64_t n, uint32_t *rank) {
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j < n) rank[list[j]] = kNoRank;
}

// positions ascend along a path: the steps that start at or before max_dist are a prefix
__global__ __launch_bounds__(kThreads) void k_prefix_len(const uint64_t *__restrict__ pos, const uint32_t *__restrict__ pstart, uint32_t n_paths,
                                                         uint64_t max_dist, uint32_t *__restrict__ plen) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n_paths) return;
    uint64_t lo = pstart[p], hi = pstart[p + 1];
    const uint64_t b = lo;
    while (lo < hi) {  // the first step whose position is past max_dist
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (pos[mid] <= max_dist) lo = mid + 1;
        else hi = mid;
    }
    plen[p] = (uint32_t)(lo - b);
}

template <class T>
__global__ __launch_bounds__(kThreads) void k_gather(const T *__restrict__ src, uint64_t src_len, const uint32_t *__restrict__ src_start,
                                                     const uint32_t *__restrict__ dst_off, uint64_t n, uint64_t total, T *__restrict__ dst) {
    const uint64_t j0 = (uint64_t)blockIdx.x * kGatherTile + threadIdx.x;
    uint64_t k = 0;
#pragma unroll 1
    for (uint32_t q = 0; q < kGatherPer; ++q) {
        const uint64_t j = j0 + (uint64_t)q * kThreads;
        if (j >= total) break;
        uint64_t lo = k, hi = n;  // the last item at or behind k that starts at or before j
        while (hi - lo > 1) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (dst_off[mid] <= j) lo = mid;
            else hi = mid;
        }
        k = lo;
        const uint64_t s = (uint64_t)src_start[k] + (j - dst_off[k]);
        if (s < src_len) dst[j] = src[s];
    }
}

__global__ __launch_bounds__(kThreads) void k_find_pos(const uint64_t *__restrict__ pos, const uint32_t *__restrict__ steps,
                                                       const uint32_t *__restrict__ seg_seq, uint32_t n_segs, uint64_t n, uint64_t offset,
                                                       unsigned long long *result) {
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kThreads) {
        const uint32_t s = steps[i] >> 1;
        if (s < n_segs && offset < pos[i] + seg_seq[2 * (uint64_t)s + 1]) atomicMin(result, (unsigned long long)i);
    }
}

}  // namespace

#define EX_HIP(expr) FGFA_HIP("extract: ", expr)

struct ExtractJob {
    ExtractGraph g;
    hipStream_t st = nullptr;
    DeviceMem mem;
    uint32_t *state = nullptr, *rank = nullptr, *cand = nullptr, *list[2] = {nullptr, nullptr}, *heads = nullptr, *words = nullptr;
    unsigned long long *key = nullptr;
    U2 *pairs = nullptr;
    uint64_t *pos = nullptr;
    Spine<SV> step_sp, link_sp;
    uint32_t *al_src = nullptr, *al_dst = nullptr;
    ExtractTotals tot;
    bool counted = false;
    int flags_error(uint32_t *f) {
        EX_HIP(staged_copy(f, words, 4, hipMemcpyDeviceToHost, st));
        return FLATGFA_OK;
    }
};

ExtractJob *extract_new() { return new ExtractJob(); }
void extract_free(ExtractJob *j) { delete j; }

int extract_begin(ExtractJob *j, const ExtractGraph &g, hipStream_t st) {
    if (g.n_steps > 0xFFFFFFFFull || g.n_links > 0xFFFFFFFFull || g.n_segs > 0x80000000u) {
        set_error("extract: graph too large for 32-bit ids");
        return FLATGFA_ERR_TOO_LARGE;
    }
    j->g = g;
    j->st = j->mem.st = st;
    const uint64_t S = g.n_segs, N = g.n_steps;
    EX_HIP(j->mem.alloc(&j->state, S));
    EX_HIP(j->mem.alloc(&j->rank, S));
    EX_HIP(j->mem.alloc(&j->key, S));
    EX_HIP(j->mem.alloc(&j->cand, S));
    EX_HIP(j->mem.alloc(&j->list[0], S));
    EX_HIP(j->mem.alloc(&j->list[1], S));
    EX_HIP(j->mem.alloc(&j->pairs, S));
    EX_HIP(j->mem.alloc(&j->heads, N / 32 + 2));
    EX_HIP(j->mem.alloc(&j->pos, N));
    EX_HIP(j->mem.alloc(&j->words, 4));
    EX_HIP(j->step_sp.alloc(&j->mem, blocks(N, kTile)));
    EX_HIP(j->link_sp.alloc(&j->mem, blocks(g.n_links, kTile)));
    EX_HIP(hipMemsetAsync(j->state, 0, std::max<uint64_t>(S, 1) * 4, st));
    EX_HIP(hipMemsetAsync(j->rank, 0xFF, std::max<uint64_t>(S, 1) * 4, st));
    EX_HIP(hipMemsetAsync(j->key, 0xFF, std::max<uint64_t>(S, 1) * 8, st));
    EX_HIP(hipMemsetAsync(j->heads, 0, (N / 32 + 2) * 4, st));
    EX_HIP(hipMemsetAsync(j->words, 0, 16, st));
    if (g.n_links) {
        hipLaunchKernelGGL(k_check_links<kThreads>, dim3((uint32_t)blocks(g.n_links, kThreads)), dim3(kThreads), 0, st, g.links, g.n_links, g.n_segs,
                           j->words, kBadLink);
        EX_HIP(hipGetLastError());
        uint32_t f = 0;
        if (int rc = j->flags_error(&f)) return rc;
        if (f & kBadLink) { set_error("extract: a link refers to a segment id that is out of range"); return FLATGFA_ERR_BOUNDS; }
    }
    return FLATGFA_OK;
}

int extract_add(ExtractJob *j, const uint32_t *segs, uint64_t n, uint64_t base) {
    if (!n) return FLATGFA_OK;
    uint32_t *d = nullptr;
    EX_HIP(hipMalloc((void **)&d, n * 4));
    hipError_t e = staged_copy(d, segs, n * 4, hipMemcpyHostToDevice, j->st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_commit, dim3((uint32_t)blocks(n, kThreads)), dim3(kThreads), 0, j->st, d, n, base, j->state, j->rank, false);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(j->st);
    }
    (void)hipFree(d);
    EX_HIP(e);
    return FLATGFA_OK;
}

int extract_bfs(ExtractJob *j, uint32_t origin, uint64_t dist, std::vector<uint32_t> *order) {
    const ExtractGraph &g = j->g;
    hipStream_t st = j->st;
    if (origin >= g.n_segs) { set_error("extract: the origin segment is out of range"); return FLATGFA_ERR_BOUNDS; }
    order->assign(1, origin);
    EX_HIP(staged_copy(j->list[0], order->data(), 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_commit, dim3(1), dim3(kThreads), 0, st, j->list[0], (uint64_t)1, (uint64_t)0, j->state, j->rank, true);
    uint64_t n_front = 1;
    int cur = 0;
    uint32_t *count = j->words + 1;
    std::vector<U2> pairs;
    std::vector<uint32_t> next;
    for (uint64_t lvl = 0; lvl < dist && n_front && g.n_links; ++lvl) {
        EX_HIP(hipMemsetAsync(count, 0, 4, st));
        hipLaunchKernelGGL(k_bfs_level, dim3(stride_blocks(g.n_links, kThreads, kMaxGrid)), dim3(kThreads), 0, st, g.links, g.n_links, j->state, j->rank, j->key,
                           j->cand, count);
        hipLaunchKernelGGL(k_clear_rank, dim3((uint32_t)blocks(n_front, kThreads)), dim3(kThreads), 0, st, j->list[cur], n_front, j->rank);
        EX_HIP(hipGetLastError());
        uint32_t c = 0;
        EX_HIP(staged_copy(&c, count, 4, hipMemcpyDeviceToHost, st));
        if (!c) break;  // (nothing new: every later level finds an empty frontier)
        hipLaunchKernelGGL(k_collect, dim3((uint32_t)blocks(c, kThreads)), dim3(kThreads), 0, st, j->cand, c, j->key, j->pairs);
        EX_HIP(hipGetLastError());
        pairs.resize(c);
        EX_HIP(staged_copy(pairs.data(), j->pairs, (size_t)c * sizeof(U2), hipMemcpyDeviceToHost, st));
        std::sort(pairs.begin(), pairs.end(), [](const U2 &x, const U2 &y) { return x.a < y.a; });
        next.resize(c);
        for (uint32_t k = 0; k < c; ++k) next[k] = (uint32_t)pairs[k].b;
        cur ^= 1;
        EX_HIP(staged_copy(j->list[cur], next.data(), (size_t)c * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_commit, dim3((uint32_t)blocks(c, kThreads)), dim3(kThreads), 0, st, j->list[cur], (uint64_t)c, (uint64_t)order->size(),
                           j->state, j->rank, true);
        order->insert(order->end(), next.begin(), next.end());
        n_front = c;
    }
    EX_HIP(hipGetLastError());
    return FLATGFA_OK;
}

int extract_positions(ExtractJob *j) {
    const ExtractGraph &g = j->g;
    hipStream_t st = j->st;
    if (g.n_paths) hipLaunchKernelGGL(k_heads, dim3((uint32_t)blocks(g.n_paths, kThreads)), dim3(kThreads), 0, st, g.pstart, g.n_paths, j->heads);
    const PosOp op{g.steps, j->heads, g.seg_seq, g.n_segs, j->words, j->pos};
    scan_count<kThreads, kPer>(op, g.n_steps, j->step_sp, st);
    scan_apply<kThreads, kPer>(op, g.n_steps, j->step_sp, st);
    EX_HIP(hipGetLastError());
    uint32_t f = 0;
    if (int rc = j->flags_error(&f)) return rc;
    if (f & kBadStep) { set_error("extract: a step refers to a segment id that is out of range"); return FLATGFA_ERR_BOUNDS; }
    return FLATGFA_OK;
}

int extract_prefix_lens(ExtractJob *j, uint64_t max_dist, uint32_t *plen) {
    const ExtractGraph &g = j->g;
    if (!g.n_paths) return FLATGFA_OK;
    uint32_t *d = nullptr;
    EX_HIP(j->mem.alloc(&d, g.n_paths));
    hipLaunchKernelGGL(k_prefix_len, dim3((uint32_t)blocks(g.n_paths, kThreads)), dim3(kThreads), 0, j->st, j->pos, g.pstart, g.n_paths, max_dist, d);
    EX_HIP(hipGetLastError());
    EX_HIP(staged_copy(plen, d, (size_t)g.n_paths * 4, hipMemcpyDeviceToHost, j->st));
    return FLATGFA_OK;
}

int extract_count(ExtractJob *j, ExtractTotals *t) {
    const ExtractGraph &g = j->g;
    hipStream_t st = j->st;
    const StepOp sop{g.steps, j->heads, j->state, g.seg_seq, g.pstart, j->pos, g.n_paths, g.n_steps, nullptr, nullptr};
    const LinkOp lop{g.links, j->state, g.n_align, j->words, nullptr, nullptr, nullptr};
    scan_count<kThreads, kPer>(sop, g.n_steps, j->step_sp, st);
    scan_count<kThreads, kPer>(lop, g.n_links, j->link_sp, st);
    EX_HIP(hipGetLastError());
    U2 a, b;
    uint32_t f = 0;
    EX_HIP(staged_copy(&a, j->step_sp.total, sizeof a, hipMemcpyDeviceToHost, st));
    EX_HIP(staged_copy(&b, j->link_sp.total, sizeof b, hipMemcpyDeviceToHost, st));
    if (int rc = j->flags_error(&f)) return rc;
    if (f & kBadSpan) { set_error("extract: a link has an overlap span outside the alignment pool"); return FLATGFA_ERR_BOUNDS; }
    j->tot = ExtractTotals{a.a, a.b, b.a, b.b};
    if (b.b > 0xFFFFFFFFull) {
        set_error("extract: the subgraph's links would hold " + std::to_string(b.b) + " alignment ops: more than 32-bit ids hold");
        return FLATGFA_ERR_TOO_LARGE;
    }
    j->counted = true;
    *t = j->tot;
    return FLATGFA_OK;
}

int extract_fill(ExtractJob *j, const ExtractOut &out) {
    if (!j->counted) { set_error("extract: fill before a successful count"); return FLATGFA_ERR_ARG; }
    const ExtractGraph &g = j->g;
    const ExtractTotals &t = j->tot;
    hipStream_t st = j->st;
    if ((t.steps && (!out.steps || !out.recs)) || (t.links && !out.links) || (t.ops && (!out.align || !out.align_src))) {
        set_error("extract: NULL output");
        return FLATGFA_ERR_ARG;
    }
    if (t.steps) {
        const StepOp sop{g.steps, j->heads, j->state, g.seg_seq, g.pstart, j->pos, g.n_paths, g.n_steps, out.steps, out.recs};
        scan_apply<kThreads, kPer>(sop, g.n_steps, j->step_sp, st);
    }
    if (t.links) {
        EX_HIP(j->mem.alloc(&j->al_src, t.links));
        EX_HIP(j->mem.alloc(&j->al_dst, t.links));
        const LinkOp lop{g.links, j->state, g.n_align, j->words, out.links, j->al_src, j->al_dst};
        scan_apply<kThreads, kPer>(lop, g.n_links, j->link_sp, st);
        if (t.ops)
            hipLaunchKernelGGL(k_gather<uint32_t>, dim3((uint32_t)blocks(t.ops, kGatherTile)), dim3(kThreads), 0, st, out.align_src, g.n_align, j->al_src,
                               j->al_dst, t.links, t.ops, out.align);
    }
    EX_HIP(hipGetLastError());
    return FLATGFA_OK;
}

int gather_bytes(const uint8_t *src, uint64_t src_len, const uint32_t *src_start, const uint32_t *dst_off, uint64_t n, uint64_t total,
                 uint8_t *dst, hipStream_t st) {
    if (!total || !n) return FLATGFA_OK;
    hipLaunchKernelGGL(k_gather<uint8_t>, dim3((uint32_t)blocks(total, kGatherTile)), dim3(kThreads), 0, st, src, src_len, src_start, dst_off, n, total, dst);
    EX_HIP(hipGetLastError());
    return FLATGFA_OK;
}

int gather_u32(const uint32_t *src, uint64_t src_len, const uint32_t *src_start, const uint32_t *dst_off, uint64_t n, uint64_t total,
               uint32_t *dst, hipStream_t st) {
    if (!total || !n) return FLATGFA_OK;
    hipLaunchKernelGGL(k_gather<uint32_t>, dim3((uint32_t)blocks(total, kGatherTile)), dim3(kThreads), 0, st, src, src_len, src_start, dst_off, n, total, dst);
    EX_HIP(hipGetLastError());
    return FLATGFA_OK;
}

int position_find(const uint32_t *steps, uint64_t n, const uint32_t *seg_seq, uint32_t n_segs, uint64_t offset, hipStream_t st, uint64_t *index,
                  uint64_t *step_start) {
    *index = n;
    *step_start = 0;
    if (!n) return FLATGFA_OK;
    DeviceMem mem;
    mem.st = st;
    uint64_t *pos = nullptr;
    unsigned long long *res = nullptr;
    uint32_t *flags = nullptr;
    Spine<SV> sp;
    EX_HIP(mem.alloc(&pos, n));
    EX_HIP(mem.alloc(&res, 1));
    EX_HIP(mem.alloc(&flags, 1));
    EX_HIP(sp.alloc(&mem, blocks(n, kTile)));
    EX_HIP(hipMemsetAsync(res, 0xFF, 8, st));
    EX_HIP(hipMemsetAsync(flags, 0, 4, st));
    const PosOp op{steps, nullptr, seg_seq, n_segs, flags, pos};
    scan_count<kThreads, kPer>(op, n, sp, st);
    scan_apply<kThreads, kPer>(op, n, sp, st);
    hipLaunchKernelGGL(k_find_pos, dim3(stride_blocks(n, kThreads, kMaxGrid)), dim3(kThreads), 0, st, pos, steps, seg_seq, n_segs, n, offset, res);
    EX_HIP(hipGetLastError());
    uint32_t f = 0;
    unsigned long long r = 0;
    EX_HIP(staged_copy(&f, flags, 4, hipMemcpyDeviceToHost, st));
    EX_HIP(staged_copy(&r, res, 8, hipMemcpyDeviceToHost, st));
    if (f & kBadStep) { set_error("position: a step refers to a segment id that is out of range"); return FLATGFA_ERR_BOUNDS; }
    if (r < n) {
        *index = r;
        EX_HIP(staged_copy(step_start, pos + r, 8, hipMemcpyDeviceToHost, st));
    }
    return FLATGFA_OK;
}

}  // namespace fgfa_dev
