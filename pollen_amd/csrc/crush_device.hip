// Crush on gfx950 (slow_odgi/slow_odgi/crush.py): within each segment's sequence every run of N becomes
// one N.  Byte k of a segment is dropped iff it is N, k > 0 and byte k - 1 of the same segment is N -- a stream compaction over
// the bases, segmented by the segments' seams.
//
// The bases are walked in the coordinates of the segments laid end to end (flatten's legend), never in the pool's: spans that
// are out of order, overlap or alias one another then need no special case, and the work is dealt by bytes, not by segments.
// The host does not know how many bytes that is before the one wait of a count, so neither the grid nor the scratch may
// depend on it: the tiles of kCrushTile laid-out bytes are dealt to kCrushGrid workgroups in equal contiguous ranges, which
// every workgroup works out from the legend's total on the device.
//
//   k_crush_check   every span lies inside the pool, else bit 0 of the flag word (and no later kernel reads a base)
//   legend          an exclusive u64 scan of the old lengths (the three-launch scan of device_scan.hpp)
//   k_crush_count   a workgroup per range of tiles; a wave walks a quarter of a tile 64 lane-consecutive bytes a round.  The tile's
//                   first segment comes from a binary search in the legend, as in k_flat_fasta; inside a step of four rounds the lanes load
//                   the next 64 legend entries together and each finds its bytes' segments among them through shuffles.  A lane
//                   takes the byte before its own from the lane below (lane 0: from the pool -- a read, so neither rounds nor
//                   tiles carry anything to one another), and a ballot gives the round's 64 keep flags.  The range's kept count goes to cnt[]; the
//                   dropped bytes go to drop[segment], one atomic add per segment and round that drops any.
//   scan            cnt[] in u64, the same scan: where each range's output begins, and the total, which the host reads once
//   k_crush_lens    seg_len_out = old length - drop, once the total is known to fit a Span
//   starts          (fill) an exclusive scan of the new lengths into the new spans: a segment begins where the kept bytes of
//                   the segments before it end, whether it is empty or not
//   k_crush_fill    the same walk, a tile at a time: bytes and keep flags into LDS, a workgroup scan of the 256 waves' counts,
//                   the kept bytes compacted in LDS at the destination's offset within 16 bytes, and the tile stored with
//                   16-byte vector stores, bytewise at its two ragged ends.
// Steps, paths and links are neither read nor checked: the reference does not look at them either.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/flatgfa.h"
#include "crush_device.hpp"
#include "device_common.hpp"
#include "device_scan.hpp"
#include "prof.hpp"

namespace fgfa_dev {
namespace {

#define CR_HIP(expr) FGFA_HIP("crush: ", expr)

static_assert(kCrushTile / 64 == kCrushThreads, "the tile's scan has one lane per wave-sized chunk of 64 bytes");
static_assert(kCrushTile % 16 == 0, "a tile is whole 16-byte vectors");

// the last index of [lo, hi] whose value is at or before x (a[lo] <= x holds); as flatten's
__device__ __forceinline__ uint64_t last_at_or_before(const uint64_t *__restrict__ a, uint64_t lo, uint64_t hi, uint64_t x) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo + 1) >> 1);
        if (a[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kCrushThreads) void k_crush_check(const uint32_t *__restrict__ seg_seq, uint32_t n_segs, uint64_t seq_len,
                                                               uint32_t *flags) {
    const uint64_t i = (uint64_t)blockIdx.x * kCrushThreads + threadIdx.x;
    if (i < n_segs && (uint64_t)seg_seq[2 * i] + seg_seq[2 * i + 1] > seq_len) atomicOr(flags, 1u);
}

// ---- the scans' operands ----
struct LegendOp {  // the old lengths -> the legend
    const uint32_t *seg_seq;
    uint64_t *legend;
    __device__ __forceinline__ Sum<uint64_t> load(uint64_t i) const { return Sum<uint64_t>{seg_seq[2 * i + 1]}; }
    __device__ __forceinline__ void store(uint64_t i, uint64_t before, const Sum<uint64_t> &) const { legend[i] = before; }
};
struct RangeOp {  // the ranges' kept counts -> where each range's output begins
    const uint64_t *cnt;
    uint64_t *pre;
    __device__ __forceinline__ Sum<uint64_t> load(uint64_t i) const { return Sum<uint64_t>{cnt[i]}; }
    __device__ __forceinline__ void store(uint64_t i, uint64_t before, const Sum<uint64_t> &) const { pre[i] = before; }
};
struct StartOp {  // the new lengths -> the new spans (the total fits 32 bits: crush_count saw to that)
    const uint32_t *seg_seq, *drop;
    uint32_t *out;
    __device__ __forceinline__ Sum<uint64_t> load(uint64_t i) const { return Sum<uint64_t>{seg_seq[2 * i + 1] - drop[i]}; }
    __device__ __forceinline__ void store(uint64_t i, uint64_t before, const Sum<uint64_t> &me) const {
        out[2 * i] = (uint32_t)before;
        out[2 * i + 1] = (uint32_t)me.v;
    }
};

__global__ __launch_bounds__(kCrushThreads) void k_crush_lens(const uint32_t *__restrict__ seg_seq, const uint32_t *__restrict__ drop,
                                                              uint32_t n_segs, uint32_t *__restrict__ seg_len_out) {
    const uint64_t i = (uint64_t)blockIdx.x * kCrushThreads + threadIdx.x;
    if (i < n_segs) seg_len_out[i] = seg_seq[2 * i + 1] - drop[i];
}

// ---- the walk ----
struct CrushWalk {
    const uint64_t *legend;   // u64[n_segs + 1]
    const uint32_t *seg_seq;  // u32[2 * n_segs]
    const uint8_t *seq_data;
    uint32_t n_segs;
    const uint32_t *flags;  // nonzero: a span leaves the pool, nothing is read
};

// the tiles [*t0, *t1) of this workgroup: the tiles of `total` laid-out bytes in gridDim.x equal contiguous ranges
__device__ __forceinline__ void my_tiles(uint64_t total, uint64_t *t0, uint64_t *t1) {
    const uint64_t tiles = (total + kCrushTile - 1) / kCrushTile, per = (tiles + gridDim.x - 1) / gridDim.x;
    *t0 = min((uint64_t)blockIdx.x * per, tiles);
    *t1 = min(*t0 + per, tiles);
}

// the segments of a tile's first and last byte, for all lanes (contains a barrier)
__device__ __forceinline__ void tile_segments(const CrushWalk &g, uint64_t q0, uint32_t tlen, uint64_t *s_range) {
    if (threadIdx.x == 0) {
        s_range[0] = last_at_or_before(g.legend, 0, g.n_segs - 1, q0);
        s_range[1] = last_at_or_before(g.legend, s_range[0], g.n_segs - 1, q0 + tlen - 1);
    }
    __syncthreads();
}

// A wave walks a quarter of the tile, 64 lane-consecutive bytes a round: round after round of one stretch of the laid-out order,
// so that the segment of a round's first byte is the one the round before ended in.
constexpr uint32_t kWaveBytes = kCrushTile / (kCrushThreads / 64);

// One step of a wave: kRounds rounds of 64 lane-consecutive bytes, the nb <= 64 kRounds bytes from laid-out offset `base` on;
// byte 64 j + lane is lane's byte of round j (every lane of the wave calls this: it shuffles).  *ws is a segment that begins at
// or before `base`; it becomes the segment of the step's last byte.  The lanes load the 64 legend entries from *ws on -- one
// coalesced load for the whole step -- and each finds its bytes' segments among them by binary searches through shuffles; a
// byte that may lie past them (64 segments or more begin inside the step: short or empty ones) is looked up in the legend
// itself.  The rounds' loads do not depend on one another.  The byte before a lane's own is the lane below's, for lane 0 the
// round before's last, and for lane 0 of the step's first round it is read from the pool -- from the byte's own segment's span,
// which is where the laid-out order has it.  keep[j]: whether crush keeps the byte.
constexpr uint32_t kRounds = 4;
static_assert(kWaveBytes % (64 * kRounds) == 0, "a wave's stretch is whole steps");
struct StepBytes {
    uint8_t ch[kRounds];
    bool first[kRounds], keep[kRounds];
    uint64_t seg[kRounds];
};
__device__ __forceinline__ void crush_step(const CrushWalk &g, uint64_t *ws, uint64_t base, uint32_t nb, StepBytes *o) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t idx = *ws + lane;
    const uint64_t v = idx <= g.n_segs ? g.legend[idx] : ~0ull;  // (legend[n_segs], the total, is past every byte)
    const uint64_t v0 = shfl_u64(v, 0);
    uint64_t at[kRounds];
#pragma unroll
    for (uint32_t j = 0; j < kRounds; ++j) {
        const uint64_t b = base + 64 * j + lane;
        uint32_t lo = 0;
        uint64_t begin = v0;
#pragma unroll
        for (uint32_t step = 32; step; step >>= 1) {
            const uint64_t vv = shfl_u64(v, (int)(lo + step));
            if (vv <= b) lo += step, begin = vv;
        }
        uint64_t s = *ws + lo;
        o->ch[j] = 0, o->first[j] = true, at[j] = 0;
        if (64 * j + lane < nb) {
            if (lo == 63) {
                s = last_at_or_before(g.legend, s, g.n_segs - 1, b);
                begin = g.legend[s];
            }
            at[j] = (uint64_t)g.seg_seq[2 * s] + (b - begin);
            o->ch[j] = g.seq_data[at[j]];
            o->first[j] = b == begin;
        }
        o->seg[j] = s;
    }
#pragma unroll
    for (uint32_t j = 0; j < kRounds; ++j) {
        uint8_t prev = (uint8_t)__shfl_up((int)o->ch[j], 1, 64);
        if (j) {
            const uint8_t last = (uint8_t)__shfl((int)o->ch[j - 1], 63, 64);
            if (lane == 0) prev = last;
        } else if (lane == 0 && nb && !o->first[0] && o->ch[0] == 'N') {
            prev = g.seq_data[at[0] - 1];
        }
        o->keep[j] = !(o->ch[j] == 'N' && !o->first[j] && prev == 'N');
        if (j == (nb - 1) >> 6) *ws = shfl_u64(o->seg[j], (int)((nb - 1) & 63));
    }
}

__global__ __launch_bounds__(kCrushThreads) void k_crush_count(CrushWalk g, uint32_t *__restrict__ drop, uint64_t *__restrict__ cnt) {
    __shared__ uint64_t s_range[2];
    __shared__ uint64_t s_wave[kCrushThreads / 64];
    if (*g.flags) return;
    const uint32_t t = threadIdx.x, lane = t & 63, w0 = (t >> 6) * kWaveBytes;
    const uint64_t total = g.legend[g.n_segs];
    uint64_t t0, t1;
    my_tiles(total, &t0, &t1);
    uint64_t kept = 0;  // (lane 0 of each wave counts for it)
    for (uint64_t tile = t0; tile < t1; ++tile) {
        const uint64_t q0 = tile * kCrushTile;
        const uint32_t tlen = (uint32_t)min((uint64_t)kCrushTile, total - q0);
        tile_segments(g, q0, tlen, s_range);
        if (w0 < tlen) {
            uint64_t ws = last_at_or_before(g.legend, s_range[0], s_range[1], q0 + w0);
            const uint32_t w1 = min(tlen, w0 + kWaveBytes);
            for (uint32_t k0 = w0; k0 < w1; k0 += 64 * kRounds) {
                const uint32_t nb = min(64 * kRounds, w1 - k0);
                StepBytes sb;
                crush_step(g, &ws, q0 + k0, nb, &sb);
#pragma unroll
                for (uint32_t j = 0; j < kRounds; ++j) {
                    if (64 * j >= nb) break;
                    const bool active = 64 * j + lane < nb;
                    const uint64_t keepm = __ballot(active && sb.keep[j]), dropm = __ballot(active && !sb.keep[j]);
                    if (lane == 0) kept += (uint64_t)__popcll(keepm);
                    if (dropm) {
                        // the round's bytes in runs of one segment each: a run begins at lane 0 and at every first byte, and
                        // the lane it begins at adds what it drops to its segment
                        const uint64_t headm = __ballot(active && sb.first[j]) | 1ull;
                        if ((headm >> lane) & 1) {
                            const uint64_t above = headm & ~((2ull << lane) - 1);
                            const int end = above ? __ffsll((long long)above) - 1 : 64;
                            const uint64_t upto = end == 64 ? ~0ull : (1ull << end) - 1;
                            const uint32_t d = (uint32_t)__popcll(dropm & upto & ~((1ull << lane) - 1));
                            if (d) atomicAdd(&drop[sb.seg[j]], d);
                        }
                    }
                }
            }
        }
        __syncthreads();  // (s_range is the next tile's)
    }
    if (lane == 0) s_wave[t >> 6] = kept;
    __syncthreads();
    if (t == 0) {
        uint64_t all = 0;
        for (int w = 0; w < kCrushThreads / 64; ++w) all += s_wave[w];
        cnt[blockIdx.x] = all;
    }
}

// out[pre[workgroup] ...): what the workgroup's tiles keep, tile after tile
__global__ __launch_bounds__(kCrushThreads) void k_crush_fill(CrushWalk g, const uint64_t *__restrict__ pre, uint8_t *__restrict__ out) {
    __shared__ uint4 out4[kCrushTile / 16 + 1];  // the kept bytes, from byte `shift` on: vector v goes to an aligned address
    __shared__ uint8_t raw[kCrushTile];
    __shared__ uint64_t s_keep[kCrushThreads];  // the keep flags of chunk c: bytes [64 c, 64 c + 64) of the tile
    __shared__ uint32_t s_off[kCrushThreads];   // what the chunks before c keep
    __shared__ uint64_t s_range[2];
    uint8_t *outb = reinterpret_cast<uint8_t *>(out4);
    const uint32_t t = threadIdx.x, lane = t & 63, w0 = (t >> 6) * kWaveBytes;
    const uint64_t total = g.legend[g.n_segs];
    uint64_t t0, t1;
    my_tiles(total, &t0, &t1);
    uint64_t run = pre[blockIdx.x];
    for (uint64_t tile = t0; tile < t1; ++tile) {
        const uint64_t q0 = tile * kCrushTile;
        const uint32_t tlen = (uint32_t)min((uint64_t)kCrushTile, total - q0);
        tile_segments(g, q0, tlen, s_range);
        if (w0 < tlen) {
            uint64_t ws = last_at_or_before(g.legend, s_range[0], s_range[1], q0 + w0);
            const uint32_t w1 = min(tlen, w0 + kWaveBytes);
            for (uint32_t k0 = w0; k0 < w1; k0 += 64 * kRounds) {
                const uint32_t nb = min(64 * kRounds, w1 - k0);
                StepBytes sb;
                crush_step(g, &ws, q0 + k0, nb, &sb);
#pragma unroll
                for (uint32_t j = 0; j < kRounds; ++j) {
                    if (64 * j >= nb) break;
                    const bool active = 64 * j + lane < nb;
                    const uint64_t keepm = __ballot(active && sb.keep[j]);
                    if (active) raw[k0 + 64 * j + lane] = sb.ch[j];
                    if (lane == 0) s_keep[(k0 >> 6) + j] = keepm;
                }
            }
        }
        __syncthreads();
        uint32_t tile_kept = 0;  // (chunk t was written by a round above iff it has a byte)
        const uint32_t before = block_excl_scan<uint32_t, kCrushThreads>(t * 64 < tlen ? (uint32_t)__popcll(s_keep[t]) : 0u, &tile_kept);
        s_off[t] = before;
        __syncthreads();
        const uintptr_t dst = reinterpret_cast<uintptr_t>(out) + run;
        const uint32_t shift = (uint32_t)(dst & 15);
        for (uint32_t k = t; k < tlen; k += kCrushThreads) {
            const uint64_t m = s_keep[k >> 6];
            if ((m >> (k & 63)) & 1) outb[shift + s_off[k >> 6] + (uint32_t)__popcll(m & ((1ull << (k & 63)) - 1))] = raw[k];
        }
        __syncthreads();
        // bytes [shift, end) of outb go to dst - shift + [shift, end): whole vectors where all 16 bytes are the tile's
        const uint32_t end = shift + tile_kept;
        for (uint32_t v = t; v * 16 < end; v += kCrushThreads) {
            const uint32_t lo = v * 16, hi = lo + 16;
            if (lo >= shift && hi <= end) {
                *reinterpret_cast<uint4 *>(dst - shift + lo) = out4[v];
            } else {
                for (uint32_t x = max(lo, shift); x < min(hi, end); ++x) *reinterpret_cast<uint8_t *>(dst - shift + x) = outb[x];
            }
        }
        run += tile_kept;
        __syncthreads();  // (the LDS is the next tile's)
    }
}

}  // namespace

struct CrushJob {
    CrushIn in;
    bool counted = false;
    uint32_t *flags = nullptr, *drop = nullptr;
    uint64_t *legend = nullptr, *cnt = nullptr, *pre = nullptr;
    Spine<Sum<uint64_t>> seg_sp, range_sp;
    uint64_t total = 0, kept = 0;
    DeviceMem mem;  // (waits for the last stream used before it frees)
};

CrushJob *crush_new() { return new CrushJob(); }
void crush_free(CrushJob *j) { delete j; }

int crush_count(CrushJob *j, const CrushIn &in, uint32_t *seg_len_out, hipStream_t st, uint64_t *bytes_out, uint64_t *dropped_out) {
    if (!j || !bytes_out || !dropped_out || (in.n_segs && (!in.seg_seq || !seg_len_out)) || (in.seq_len && !in.seq_data)) {
        set_error("crush: NULL argument");
        return FLATGFA_ERR_ARG;
    }
    if (in.n_segs > 0x80000000u) { set_error("crush: graph too large for 32-bit ids"); return FLATGFA_ERR_TOO_LARGE; }
    if (j->counted) { set_error("crush: this job was counted already"); return FLATGFA_ERR_ARG; }
    j->in = in;
    j->mem.st = st;
    const uint32_t S = in.n_segs;
    CR_HIP(j->mem.alloc(&j->flags, 2));
    CR_HIP(j->mem.alloc(&j->legend, (uint64_t)S + 1));
    CR_HIP(j->mem.alloc(&j->drop, S));
    CR_HIP(j->mem.alloc(&j->cnt, 2 * (uint64_t)kCrushGrid));
    j->pre = j->cnt + kCrushGrid;
    CR_HIP(j->seg_sp.alloc(&j->mem, blocks(S, kCrushThreads * kCrushScanPer)));
    CR_HIP(j->range_sp.alloc(&j->mem, blocks(kCrushGrid, kCrushThreads * kCrushScanPer)));
    CR_HIP(hipMemsetAsync(j->flags, 0, 8, st));
    CR_HIP(hipMemsetAsync(j->drop, 0, std::max<uint64_t>(S, 1) * 4, st));
    CR_HIP(hipMemsetAsync(j->cnt, 0, (uint64_t)kCrushGrid * 8, st));
    const CrushWalk g{j->legend, in.seg_seq, in.seq_data, S, j->flags};
    if (S) hipLaunchKernelGGL(k_crush_check, dim3((uint32_t)blocks(S, kCrushThreads)), dim3(kCrushThreads), 0, st, in.seg_seq, S, in.seq_len, j->flags);
    {
        ProfScope prof("crush_legend", st);
        const LegendOp op{in.seg_seq, j->legend};
        scan_count<kCrushThreads, kCrushScanPer, Sum<uint64_t>>(op, S, j->seg_sp, st);
        scan_apply<kCrushThreads, kCrushScanPer, Sum<uint64_t>>(op, S, j->seg_sp, st);
    }
    CR_HIP(hipGetLastError());
    CR_HIP(hipMemcpyAsync(j->legend + S, j->seg_sp.total, 8, hipMemcpyDeviceToDevice, st));
    {
        ProfScope prof("crush_count", st);
        hipLaunchKernelGGL(k_crush_count, dim3(kCrushGrid), dim3(kCrushThreads), 0, st, g, j->drop, j->cnt);
    }
    {
        ProfScope prof("crush_range_scan", st);
        const RangeOp op{j->cnt, j->pre};
        scan_count<kCrushThreads, kCrushScanPer, Sum<uint64_t>>(op, kCrushGrid, j->range_sp, st);
        scan_apply<kCrushThreads, kCrushScanPer, Sum<uint64_t>>(op, kCrushGrid, j->range_sp, st);
    }
    CR_HIP(hipGetLastError());
    uint32_t flags = 0;
    CR_HIP(hipMemcpyAsync(&flags, j->flags, 4, hipMemcpyDeviceToHost, st));
    CR_HIP(hipMemcpyAsync(&j->total, j->legend + S, 8, hipMemcpyDeviceToHost, st));
    CR_HIP(hipMemcpyAsync(&j->kept, j->range_sp.total, 8, hipMemcpyDeviceToHost, st));
    CR_HIP(hipStreamSynchronize(st));
    if (flags) { set_error("crush: a segment has a sequence span outside seq_data"); return FLATGFA_ERR_BOUNDS; }
    if (j->kept > 0xFFFFFFFFull) {  // (a Span is two u32)
        set_error("crush: the crushed sequences would take " + std::to_string(j->kept) + " bytes: more than a 32-bit span holds");
        return FLATGFA_ERR_TOO_LARGE;
    }
    if (S) hipLaunchKernelGGL(k_crush_lens, dim3((uint32_t)blocks(S, kCrushThreads)), dim3(kCrushThreads), 0, st, in.seg_seq, j->drop, S, seg_len_out);
    CR_HIP(hipGetLastError());
    j->counted = true;
    *bytes_out = j->kept;
    *dropped_out = j->total - j->kept;
    return FLATGFA_OK;
}

int crush_fill(CrushJob *j, uint8_t *seq_out, uint32_t *seg_seq_out, hipStream_t st) {
    if (!j || !j->counted) { set_error("crush: fill before a successful count"); return FLATGFA_ERR_ARG; }
    const CrushIn &in = j->in;
    if ((j->kept && !seq_out) || (in.n_segs && !seg_seq_out)) { set_error("crush: NULL output"); return FLATGFA_ERR_ARG; }
    j->mem.st = st;
    if (in.n_segs) {
        ProfScope prof("crush_starts", st);
        const StartOp op{in.seg_seq, j->drop, seg_seq_out};
        scan_count<kCrushThreads, kCrushScanPer, Sum<uint64_t>>(op, in.n_segs, j->seg_sp, st);
        scan_apply<kCrushThreads, kCrushScanPer, Sum<uint64_t>>(op, in.n_segs, j->seg_sp, st);
    }
    if (j->kept) {
        ProfScope prof("crush_fill", st);
        const CrushWalk g{j->legend, in.seg_seq, in.seq_data, in.n_segs, j->flags};
        hipLaunchKernelGGL(k_crush_fill, dim3(kCrushGrid), dim3(kCrushThreads), 0, st, g, j->pre, seq_out);
    }
    CR_HIP(hipGetLastError());
    return FLATGFA_OK;
}

}  // namespace fgfa_dev

// ---- the device-level C ABI (include/flatgfa.h Part 3) ----
struct flatgfa_dev_crush {
    fgfa_dev::CrushJob *job = nullptr;
    ~flatgfa_dev_crush() { fgfa_dev::crush_free(job); }
};

extern "C" {

int flatgfa_dev_crush_count(const uint32_t *seg_seq, const uint8_t *seq_data, uint64_t seq_len, uint32_t n_segs, uint32_t *seg_len_out, void *stream,
                            flatgfa_dev_crush_t **job, uint64_t *bytes_out, uint64_t *dropped_out) {
    if (job) *job = nullptr;
    if (!job || !bytes_out || !dropped_out) { fgfa_dev::set_error("flatgfa_dev_crush_count: NULL argument"); return FLATGFA_ERR_ARG; }
    fgfa_dev::CrushIn in;
    in.seg_seq = seg_seq;
    in.seq_data = seq_data;
    in.seq_len = seq_len;
    in.n_segs = n_segs;
    auto *h = new flatgfa_dev_crush();
    h->job = fgfa_dev::crush_new();
    const int rc = fgfa_dev::crush_count(h->job, in, seg_len_out, (hipStream_t)stream, bytes_out, dropped_out);
    if (rc) {
        delete h;
        return rc;
    }
    *job = h;
    return FLATGFA_OK;
}

int flatgfa_dev_crush_fill(flatgfa_dev_crush_t *job, uint8_t *seq_out, uint32_t *seg_seq_out, void *stream) {
    if (!job) { fgfa_dev::set_error("flatgfa_dev_crush_fill: NULL job"); return FLATGFA_ERR_ARG; }
    return fgfa_dev::crush_fill(job->job, seq_out, seg_seq_out, (hipStream_t)stream);
}

void flatgfa_dev_crush_free(flatgfa_dev_crush_t *job) { delete job; }

}  // extern "C"
