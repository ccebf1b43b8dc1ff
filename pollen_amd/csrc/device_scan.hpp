// What the count-scan-fill features share (chop, GAF lookup, extract / position, validate / degree):
// wave and workgroup scans, the one tiled scan, and the small pieces around them.  HIP only.  Templates and inline functions
// (the kernels are static templates: every translation unit that launches one gets its own), so any number of .hip files may
// include it; each passes its own kThreads / kPer.
//
//   k_scan + k_spine   a scan of any length in three launches -- the tiles' aggregates, one workgroup over the aggregates, the
//                      tiles again with their prefixes -- over a value type V and an Op with load(i) and store(i, before, me).
//                      Sum<T> is the plain sum (topology's row scan in place and its missing-pair counts on 4-byte values, the
//                      spine on 8-byte ones); extract's SV (two sums and a head flag: the segmented scan) lives in
//                      extract_device.hip.
//
// NOT built on it, on purpose: chop's ticketed k_reduce / k_prefix / k_offsets and lookup's recursive scan_u64
// (k_lk_scan_local, k_lk_scan_add).  They use block_excl_scan and the wave helpers from here and nothing else.  Moving them
// onto the three-launch scan would change launch counts and memory passes on paths with published timings
// (profiles/chop_bench.json, profiles/gaf_lookup_bench.json): a performance change, to be made with its own measurement.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/flatgfa.h"
#include "device_common.hpp"

namespace fgfa_dev {

// ---- waves ----
__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int d) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int d) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += shfl_xor_u64(v, d);
    return v;
}
__device__ __forceinline__ uint64_t wave_incl_scan(uint64_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t u = shfl_up_u64(v, d);
        if (lane >= d) v += u;
    }
    return v;
}

// ---- workgroups ----

// Exclusive scan over the workgroup's kThreads lanes; *total = the sum.  Contains barriers: every lane calls it.
// (A u32 goes through the u64 shuffle too.)
template <class T, int kThreads>
__device__ __forceinline__ T block_excl_scan(T v, T *total) {
    __shared__ T wsum[kThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T u = (T)shfl_up_u64((uint64_t)incl, d);
        if (lane >= d) incl += u;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
        if (w < wave) before += wsum[w];
        all += wsum[w];
    }
    __syncthreads();  // (wsum is reused by the next call)
    *total = all;
    return before + incl - v;
}

// A scan value V is a plain struct with
//   V::zero(), V::comb(x, y)   the monoid (comb need not commute: x lies before y)
//   V::Carry, x.carry()        what of the values before an element its store sees
//   V::Wide                    the value type of the tiles' aggregates, with V::widen(x), and V::after(c) for the value that
//                              stands for a Wide::Carry c, a tile's prefix, in front of the tile
template <class T>
struct Sum {
    using Carry = T;
    using Wide = Sum<uint64_t>;
    T v;
    __device__ __forceinline__ static Sum zero() { return Sum{0}; }
    __device__ __forceinline__ static Sum comb(const Sum &x, const Sum &y) { return Sum{(T)(x.v + y.v)}; }
    __device__ __forceinline__ T carry() const { return v; }
    __device__ __forceinline__ static Wide widen(const Sum &x) { return Wide{x.v}; }
    __device__ __forceinline__ static Sum after(uint64_t c) { return Sum{(T)c}; }  // (rows are u32 below a u64 spine)
};

// Inclusive scan of one value per lane over the workgroup, left in sh.  Contains barriers: every lane calls it.
template <int kThreads, class V>
__device__ __forceinline__ void block_scan(V *sh, V mine) {
    const uint32_t t = threadIdx.x;
    sh[t] = mine;
    __syncthreads();
    for (uint32_t d = 1; d < kThreads; d <<= 1) {
        V x = sh[t];
        if (t >= d) x = V::comb(sh[t - d], x);
        __syncthreads();
        sh[t] = x;
        __syncthreads();
    }
}

// ---- the tiled scan ----

// A tile of kThreads * kPer elements per workgroup.  Every lane holds its kPer elements in registers before any is stored, so
// an Op may store where it loads.  !kApply: the tile's aggregate.  kApply: the stores, behind prefix[tile].
template <class V, class Op, int kThreads, uint32_t kPer, bool kApply>
static __global__ __launch_bounds__(kThreads) void k_scan(Op op, uint64_t n, typename V::Wide *__restrict__ aggr,
                                                          const typename V::Wide::Carry *__restrict__ prefix) {
    __shared__ V sh[kThreads];
    const uint64_t base = (uint64_t)blockIdx.x * (kThreads * kPer) + (uint64_t)threadIdx.x * kPer;
    V item[kPer];
    V acc = V::zero();
#pragma unroll
    for (uint32_t q = 0; q < kPer; ++q) {
        item[q] = base + q < n ? op.load(base + q) : V::zero();
        acc = V::comb(acc, item[q]);
    }
    block_scan<kThreads>(sh, acc);
    if (!kApply) {
        if (threadIdx.x == kThreads - 1) aggr[blockIdx.x] = V::widen(sh[kThreads - 1]);
        return;
    }
    V run = V::comb(V::after(prefix[blockIdx.x]), threadIdx.x ? sh[threadIdx.x - 1] : V::zero());
#pragma unroll
    for (uint32_t q = 0; q < kPer; ++q) {
        if (base + q < n) op.store(base + q, run.carry(), item[q]);
        run = V::comb(run, item[q]);
    }
}

// One workgroup: the exclusive scan of the tiles' aggregates, and the total.
template <class V, int kThreads>
static __global__ __launch_bounds__(kThreads) void k_spine(const V *__restrict__ aggr, uint64_t n_tiles, typename V::Carry *__restrict__ prefix,
                                                           typename V::Carry *total) {
    __shared__ V sh[kThreads];
    V carry = V::zero();
    for (uint64_t b = 0; b < n_tiles; b += kThreads) {
        const uint64_t i = b + threadIdx.x;
        block_scan<kThreads>(sh, i < n_tiles ? aggr[i] : V::zero());
        if (i < n_tiles) prefix[i] = V::comb(carry, threadIdx.x ? sh[threadIdx.x - 1] : V::zero()).carry();
        carry = V::comb(carry, sh[kThreads - 1]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry.carry();
}

// ---- small kernels and device functions ----

// a link that names a segment at or past n_segs raises `bit` of the flag word
template <int kThreads>
static __global__ __launch_bounds__(kThreads) void k_check_links(const uint32_t *__restrict__ links, uint64_t n_links, uint32_t n_segs,
                                                                 uint32_t *flags, uint32_t bit) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_links) return;
    if ((links[i * 4] >> 1) >= n_segs || (links[i * 4 + 1] >> 1) >= n_segs) atomicOr(flags, bit);
}

// the last path of [lo, hi] that starts at or before step j of the paths laid one behind another: the one that holds it
__device__ __forceinline__ uint32_t last_start_at_or_before(const uint32_t *pstart, uint32_t lo, uint32_t hi, uint64_t j) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1) >> 1);
        if (pstart[mid] <= j) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// ---- host side ----

inline uint64_t blocks(uint64_t n, uint64_t per) { return (n + per - 1) / per; }
// workgroups of a grid-stride launch: at least one, at most max_grid
inline uint32_t stride_blocks(uint64_t n, uint64_t per, uint32_t max_grid) {
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(blocks(n, per), 1), max_grid);
}

// device allocations given back on every way out, behind the work queued on `st`
struct DeviceMem {
    std::vector<void *> mem;
    hipStream_t st = nullptr;
    DeviceMem() = default;
    DeviceMem(const DeviceMem &) = delete;
    DeviceMem &operator=(const DeviceMem &) = delete;
    ~DeviceMem() {
        if (mem.empty()) return;
        if (st) (void)hipStreamSynchronize(st);
        for (void *p : mem) (void)hipFree(p);
    }
    template <class T>
    hipError_t alloc(T **p, uint64_t count) {  // (at least one element)
        *p = nullptr;
        const hipError_t e = hipMalloc((void **)p, std::max<uint64_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) mem.push_back(*p);
        return e;
    }
};

// the scratch of one scan over values V: room for blocks(n, kThreads * kPer) tiles
template <class V>
struct Spine {
    typename V::Wide *aggr = nullptr;
    typename V::Wide::Carry *prefix = nullptr, *total = nullptr;
    hipError_t alloc(DeviceMem *m, uint64_t tiles) {
        hipError_t e = m->alloc(&aggr, tiles);
        if (e == hipSuccess) e = m->alloc(&prefix, tiles + 1);
        total = prefix ? prefix + tiles : nullptr;
        return e;
    }
};
// tiles, then spine
template <int kThreads, uint32_t kPer, class V, class Op>
void scan_count(const Op &op, uint64_t n, const Spine<V> &sp, hipStream_t st) {
    const uint32_t tiles = (uint32_t)blocks(n, kThreads * kPer);
    if (tiles) hipLaunchKernelGGL((k_scan<V, Op, kThreads, kPer, false>), dim3(tiles), dim3(kThreads), 0, st, op, n, sp.aggr, sp.prefix);
    hipLaunchKernelGGL((k_spine<typename V::Wide, kThreads>), dim3(1), dim3(kThreads), 0, st, sp.aggr, (uint64_t)tiles, sp.prefix, sp.total);
}
template <int kThreads, uint32_t kPer, class V, class Op>
void scan_apply(const Op &op, uint64_t n, const Spine<V> &sp, hipStream_t st) {
    const uint32_t tiles = (uint32_t)blocks(n, kThreads * kPer);
    if (tiles) hipLaunchKernelGGL((k_scan<V, Op, kThreads, kPer, true>), dim3(tiles), dim3(kThreads), 0, st, op, n, sp.aggr, sp.prefix);
}

}  // namespace fgfa_dev
