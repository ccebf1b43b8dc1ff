// GAF lookup on gfx950 (flatgfa/src/ops/gaf.rs).
//
// For every line of GAF text -- the bytes before a '\n', none skipped -- the read's path field is walked through the graph: each
// token `>N` / `<N` is a handle, `pos` is the sum of the lengths of the segments before it, and the read's [start, end) says
// which stretch of the segment it covers (gaf.rs:200-243).  As `pos` never decreases, the reference's walk with its two flags
// is a rule per token (with next = pos + len):
//
//     start >= next                          None      (not started)
//     start >= pos   (the first started)     Partial(start - pos, end < next ? end - pos : len)
//     end < pos                              None      (ended before)
//     end < next                             Partial(0, end - pos)
//     otherwise                              All
//
// so an event needs its token's `pos` and nothing else of its line: a segmented prefix sum.
//
//   k_lk_nl_count    '\n' per tile of 16 KiB; a scan of the counts places every tile's lines.
//   k_lk_nl_scatter  the offset of every '\n', in order: line l is (line_end[l - 1], line_end[l]).
//   k_lk_parse       a wave per line, 64 bytes a step: tabs 1 and 5 .. 9 from ballots, `start` and `end` as digit runs (each
//                    lane a digit times its power of ten, wrapping), the end of the clean token prefix of the path field --
//                    the first byte outside [<>0-9], a '<' or '>' with no digit behind it, a first byte that is a digit --
//                    as the first set bit of a ballot, and the tokens before it.  A scan of the counts is line_first.
//   k_lk_events      a wave per line, 64 bytes a step: a lane on a '<' or '>' reads its digits, finds the id by the bisection of
//                    namemap.rs:27-33, and a wave scan of the segment lengths plus the carry of the steps before gives `pos`.
//                    With `-s` it also writes the copy list: per line the name and its tab, one item per event, the '\n'.
//   k_lk_gather      the `-s` text, tiled by OUTPUT bytes: a workgroup owns 16 KiB of it whatever the events are, bisects the
//                    scanned item lengths for its first and last item, and each lane fills 16 bytes at a time from the text
//                    or the sequence pool (one 16-byte load where they lie in one item, bytes across item ends), reversed
//                    and complemented for a backward handle.  A read through a 5 Mbp segment is
//                    320 workgroups.
//
// Every offset, count and length is a u64.  Kernels never trap: a bad line lowers one of three words to its offset.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/flatgfa.h"
#include "device_common.hpp"
#include "device_scan.hpp"
#include "gaf_lookup_device.hpp"
#include "name_lookup.hpp"
#include "prof.hpp"

namespace fgfa_dev {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kLaneBytes = 64;                     // consecutive text bytes per lane of the line index
constexpr uint32_t kNlTile = kThreads * kLaneBytes;     // text bytes per workgroup of the line index
constexpr uint32_t kScanItems = 8;
constexpr uint32_t kScanTile = kThreads * kScanItems;   // elements per workgroup of a scan
constexpr uint32_t kOutRows = 4;
constexpr uint32_t kOutTile = kThreads * 16 * kOutRows;  // output bytes per workgroup of the gather
constexpr uint64_t kRev = 1ull << 63, kFromText = 1ull << 62, kSrcMask = kFromText - 1;
constexpr uint64_t kBadLine = ~0ull;                    // m_pb of a line the parser rejects

// 0x80 in every byte of w equal to c (exact: no borrow runs between bytes)
__device__ __forceinline__ uint32_t eq_bytes(uint32_t w, uint32_t c) {
    const uint32_t t = w ^ (c * 0x01010101u);
    return ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t) & 0x80808080u;
}

// ---- scans (u64, exclusive, in place) ----

__global__ __launch_bounds__(kThreads) void k_lk_scan_local(uint64_t *__restrict__ a, uint64_t n, uint64_t *__restrict__ block_sum) {
    const uint64_t first = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanItems;
    uint64_t v[kScanItems], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < kScanItems; ++k) {
        v[k] = first + k < n ? a[first + k] : 0;
        sum += v[k];
    }
    uint64_t total;
    uint64_t run = block_excl_scan<uint64_t, kThreads>(sum, &total);
#pragma unroll
    for (uint32_t k = 0; k < kScanItems; ++k) {
        if (first + k < n) a[first + k] = run;
        run += v[k];
    }
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void k_lk_scan_add(uint64_t *__restrict__ a, uint64_t n, const uint64_t *__restrict__ block_off) {
    const uint64_t first = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanItems, add = block_off[blockIdx.x];
#pragma unroll
    for (uint32_t k = 0; k < kScanItems; ++k)
        if (first + k < n) a[first + k] += add;
}

uint64_t scan_blocks(uint64_t n) { return (n + kScanTile - 1) / kScanTile; }
// u64 words of scratch a scan of n elements takes
uint64_t scan_scratch_words(uint64_t n) {
    uint64_t w = 0;
    for (uint64_t nb = scan_blocks(n);; nb = scan_blocks(nb)) {
        w += nb;
        if (nb <= 1) return w;
    }
}
void scan_u64(uint64_t *a, uint64_t n, uint64_t *scratch, hipStream_t stream) {
    const uint64_t nb = scan_blocks(n);
    hipLaunchKernelGGL(k_lk_scan_local, dim3((uint32_t)nb), dim3(kThreads), 0, stream, a, n, scratch);
    if (nb <= 1) return;
    scan_u64(scratch, nb, scratch + nb, stream);
    hipLaunchKernelGGL(k_lk_scan_add, dim3((uint32_t)nb), dim3(kThreads), 0, stream, a, n, scratch);
}

// ---- the line index ----

// The 16 bytes at `vpos` (a multiple of 16, counted from the 16-byte boundary `abase` below the text), those outside [lo, hi) as 0.
__device__ __forceinline__ uint4 load16(const uint8_t *__restrict__ abase, uint64_t vpos, uint64_t lo, uint64_t hi) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (vpos >= hi || vpos + 16 <= lo) return v;
    v = *reinterpret_cast<const uint4 *>(abase + vpos);
    if (vpos < lo || vpos + 16 > hi) {
        const uint32_t a = vpos < lo ? (uint32_t)(lo - vpos) : 0u, b = (uint32_t)min<uint64_t>(16, hi - vpos);
        uint32_t m[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k)
            if (k >= a && k < b) m[k >> 2] |= 0xFFu << ((k & 3) * 8);
        v.x &= m[0];
        v.y &= m[1];
        v.z &= m[2];
        v.w &= m[3];
    }
    return v;
}

__global__ __launch_bounds__(kThreads) void k_lk_nl_count(const uint8_t *__restrict__ abase, uint64_t lead, uint64_t vend,
                                                           uint64_t *__restrict__ tile_cnt) {
    const uint64_t p = (uint64_t)blockIdx.x * kNlTile + (uint64_t)threadIdx.x * kLaneBytes;
    uint32_t c = 0;
#pragma unroll
    for (uint32_t k = 0; k < kLaneBytes / 16; ++k) {
        const uint4 v = load16(abase, p + 16u * k, lead, vend);
        c += (uint32_t)__builtin_popcount(eq_bytes(v.x, '\n')) + (uint32_t)__builtin_popcount(eq_bytes(v.y, '\n')) +
             (uint32_t)__builtin_popcount(eq_bytes(v.z, '\n')) + (uint32_t)__builtin_popcount(eq_bytes(v.w, '\n'));
    }
    uint64_t total;
    (void)block_excl_scan<uint64_t, kThreads>(c, &total);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void k_lk_nl_scatter(const uint8_t *__restrict__ abase, uint64_t lead, uint64_t vend,
                                                             const uint64_t *__restrict__ tile_first, uint64_t *__restrict__ line_end) {
    const uint64_t p = (uint64_t)blockIdx.x * kNlTile + (uint64_t)threadIdx.x * kLaneBytes;
    uint4 v[kLaneBytes / 16];
    uint32_t c = 0;
#pragma unroll
    for (uint32_t k = 0; k < kLaneBytes / 16; ++k) {
        v[k] = load16(abase, p + 16u * k, lead, vend);
        c += (uint32_t)__builtin_popcount(eq_bytes(v[k].x, '\n')) + (uint32_t)__builtin_popcount(eq_bytes(v[k].y, '\n')) +
             (uint32_t)__builtin_popcount(eq_bytes(v[k].z, '\n')) + (uint32_t)__builtin_popcount(eq_bytes(v[k].w, '\n'));
    }
    uint64_t total;
    uint64_t at = tile_first[blockIdx.x] + block_excl_scan<uint64_t, kThreads>(c, &total);
    if (!c) return;
#pragma unroll
    for (uint32_t k = 0; k < kLaneBytes / 16; ++k) {
        const uint32_t w[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            for (uint32_t m = eq_bytes(w[j], '\n'); m; m &= m - 1)
                line_end[at++] = p + 16u * k + 4u * j + ((uint32_t)__builtin_ctz(m) >> 3) - lead;
    }
}

// ---- lines ----

struct LineOut {
    uint64_t *name_len, *pb, *stop, *start, *end;  // per line
    uint64_t *ntok;                                // per line: becomes line_first by a scan
};

// The digits text[a, b) as a u64, wrapping (gaf.rs:264-285); *ok is cleared where the field is empty or holds another byte.
__device__ __forceinline__ uint64_t digits_u64(const uint8_t *__restrict__ text, uint64_t a, uint64_t b, int lane, bool *ok) {
    if (a >= b) *ok = false;
    uint64_t num = 0;
    for (uint64_t p = a; p < b; p += 64) {
        const uint32_t cnt = (uint32_t)min<uint64_t>(64, b - p);
        uint64_t term = 0;
        bool bad = false;
        if ((uint32_t)lane < cnt) {
            const uint32_t d = (uint32_t)text[p + lane] - '0';
            bad = d >= 10u;
            uint64_t w = d;
            for (uint32_t k = lane + 1; k < cnt; ++k) w *= 10u;
            term = w;
        }
        if (__builtin_amdgcn_ballot_w64(bad)) *ok = false;
        uint64_t shift = 1;
        if (num)
            for (uint32_t k = 0; k < cnt; ++k) shift *= 10u;
        term = wave_incl_scan(term, lane);
        num = num * shift + shfl_u64(term, 63);
    }
    return num;
}

__global__ __launch_bounds__(kThreads) void k_lk_parse(const uint8_t *__restrict__ text, const uint64_t *__restrict__ line_end,
                                                        uint64_t n_lines, LineOut o, unsigned long long *__restrict__ bad_parse,
                                                        uint64_t base) {
    const int lane = threadIdx.x & 63;
    const uint64_t l = (uint64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (l >= n_lines) return;
    const uint64_t ls = l ? line_end[l - 1] + 1 : 0, le = line_end[l];
    // tabs 1, 5, 6, 7, 8, 9 (gaf.rs:50-70: field 0 is the name, 5 the path, 7 and 8 the coordinates)
    uint64_t t1 = 0, t5 = 0, t6 = 0, t7 = 0, t8 = 0, t9 = 0;
    uint32_t seen = 0;
    for (uint64_t p = ls; p < le && seen < 9; p += 64) {
        const bool tab = p + lane < le && text[p + lane] == '\t';
        for (unsigned long long m = __builtin_amdgcn_ballot_w64(tab); m && seen < 9; m &= m - 1) {
            const uint64_t at = p + (uint64_t)__builtin_ctzll(m);
            ++seen;
            if (seen == 1) t1 = at;
            else if (seen == 5) t5 = at;
            else if (seen == 6) t6 = at;
            else if (seen == 7) t7 = at;
            else if (seen == 8) t8 = at;
            else if (seen == 9) t9 = at;
        }
    }
    bool ok = seen >= 9;
    uint64_t start = 0, end = 0;
    if (ok) {
        start = digits_u64(text, t7 + 1, t8, lane, &ok);
        end = digits_u64(text, t8 + 1, t9, lane, &ok);
    }
    if (!ok) {  // where the reference panics
        if (lane == 0) {
            atomicMin(bad_parse, (unsigned long long)(base + ls));
            o.pb[l] = kBadLine;
            o.stop[l] = kBadLine;
            o.name_len[l] = 0;
            o.start[l] = 0;
            o.end[l] = 0;
            o.ntok[l] = 0;
        }
        return;
    }
    // the clean token prefix of the path field (gaf.rs:287-308) and the tokens in it
    const uint64_t pb = t5 + 1, pe = t6;
    uint64_t count = 0, stop = pe;
    for (uint64_t p = pb; p < pe; p += 64) {
        const uint64_t i = p + lane;
        const bool valid = i < pe;
        const uint32_t c = valid ? text[i] : 0u, nx = i + 1 < pe ? text[i + 1] : 0u;
        const bool dir = c == '>' || c == '<', dig = c - '0' < 10u;
        const bool bad = valid && ((!dir && !dig) || (dir && nx - '0' >= 10u) || (i == pb && !dir));
        const unsigned long long mb = __builtin_amdgcn_ballot_w64(bad), md = __builtin_amdgcn_ballot_w64(valid && dir);
        if (mb) {
            const int f = __builtin_ctzll(mb);
            count += (uint64_t)__builtin_popcountll(md & ((1ull << f) - 1ull));
            stop = p + (uint64_t)f;
            break;
        }
        count += (uint64_t)__builtin_popcountll(md);
    }
    if (lane == 0) {
        o.pb[l] = pb;
        o.stop[l] = stop;
        o.name_len[l] = t1 - ls;
        o.start[l] = start;
        o.end[l] = end;
        o.ntok[l] = count;
    }
}

// ---- events ----

struct Graph {
    const uint64_t *keys;  // the NameMap's `others`, sorted by name
    const uint32_t *ids;
    uint32_t n_others;
    uint32_t n_segs;
    uint64_t seq_max;
    const uint32_t *seg_seq;
};

// NameMap::get (namemap.rs:27-33); an id >= n_segs is where the reference panics
__device__ __forceinline__ uint32_t name_id(uint64_t num, const Graph &g) {
    return name_map_get(num, g.keys, g.ids, g.n_others, g.seq_max);
}

struct EventOut {
    uint32_t *handle;
    uint8_t *kind;
    uint64_t *a, *b;
    uint64_t *g_len, *g_src;  // the copy list of the `-s` text, or NULL
};

__global__ __launch_bounds__(kThreads) void k_lk_events(const uint8_t *__restrict__ text, const uint64_t *__restrict__ line_end,
                                                         uint64_t n_lines, LineOut in, Graph g, EventOut o,
                                                         unsigned long long *__restrict__ bad_name,
                                                         unsigned long long *__restrict__ bad_slice, uint64_t base) {
    const int lane = threadIdx.x & 63;
    const uint64_t l = (uint64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (l >= n_lines) return;
    const uint64_t ls = l ? line_end[l - 1] + 1 : 0, le = line_end[l];
    const uint64_t first = in.ntok[l], ntok = in.ntok[l + 1] - first;  // (scanned: ntok[l] is the line's first event)
    const uint64_t pb = in.pb[l], stop = in.stop[l], start = in.start[l], end = in.end[l];
    const bool bad_line = pb == kBadLine;
    if (o.g_len && lane == 0) {  // name and tab before the events, the '\n' behind them: both are bytes of the text
        const uint64_t ib = first + 2 * l;
        o.g_len[ib] = bad_line ? 0 : in.name_len[l] + 1;
        o.g_src[ib] = kFromText | ls;
        o.g_len[ib + 1 + ntok] = bad_line ? 0 : 1;
        o.g_src[ib + 1 + ntok] = kFromText | le;
    }
    if (bad_line) return;
    uint64_t carry_pos = 0, carry_cnt = 0;
    for (uint64_t p = pb; p < stop; p += 64) {
        const uint64_t i = p + lane;
        const uint32_t c = i < stop ? text[i] : 0u;
        const bool tok = c == '>' || c == '<';
        uint32_t id = 0xFFFFFFFFu, len = 0, seq0 = 0;
        bool known = false;
        if (tok) {
            uint64_t num = 0;
            for (uint64_t q = i + 1; q < stop; ++q) {  // (the prefix is clean: digits up to the next token or `stop`)
                const uint32_t d = (uint32_t)text[q] - '0';
                if (d >= 10u) break;
                num = num * 10u + d;
            }
            id = name_id(num, g);
            known = id < g.n_segs;
            if (known) {
                seq0 = g.seg_seq[2 * (uint64_t)id];
                len = g.seg_seq[2 * (uint64_t)id + 1];
            } else {
                atomicMin(bad_name, (unsigned long long)(base + ls));
            }
        }
        const uint64_t incl = wave_incl_scan(len, lane);
        const uint64_t next = carry_pos + incl, pos = next - len;
        const unsigned long long mt = __builtin_amdgcn_ballot_w64(tok);
        const uint64_t k = first + carry_cnt + (uint64_t)__builtin_popcountll(mt & ((1ull << lane) - 1ull));
        if (tok) {
            uint32_t kind = 0;
            uint64_t a = 0, b = 0;
            if (!known || !(start < next)) {
                // not started (gaf.rs:229-231)
            } else if (!(start < pos)) {  // starts here (gaf.rs:213-222)
                kind = 2;
                a = start - pos;
                b = end < next ? end - pos : (uint64_t)len;
            } else if (end < pos) {
                // ended before
            } else if (end < next) {  // ends here (gaf.rs:223-226)
                kind = 2;
                b = end - pos;
            } else {  // gaf.rs:227-228
                kind = 1;
                b = len;
            }
            const uint32_t back = c == '<';
            o.handle[k] = known ? (id << 1) | back : 0xFFFFFFFFu;
            o.kind[k] = (uint8_t)kind;
            o.a[k] = a;
            o.b[k] = b;
            if (o.g_len) {
                uint64_t bytes = 0, src = 0;
                if (kind && (a > b || b > len)) {  // the slice the reference panics on (flatgfa.rs:295-345)
                    atomicMin(bad_slice, (unsigned long long)(base + ls));
                } else if (kind && b > a) {
                    bytes = b - a;
                    // backward: seq[len - b .. len - a] read from its last byte down
                    src = back ? kRev | ((uint64_t)seq0 + len - a - 1) : (uint64_t)seq0 + a;
                }
                o.g_len[k + 2 * l + 1] = bytes;
                o.g_src[k + 2 * l + 1] = src;
            }
        }
        carry_pos += shfl_u64(incl, 63);
        carry_cnt += (uint64_t)__builtin_popcountll(mt);
    }
}

// ---- the `-s` text ----

// flatgfa.rs:327-345: ACGT and acgt swap in pairs, every other byte stays
__device__ __forceinline__ uint32_t complement(uint32_t c) {
    switch (c) {
        case 'A': return 'T';
        case 'C': return 'G';
        case 'G': return 'C';
        case 'T': return 'A';
        case 'a': return 't';
        case 'c': return 'g';
        case 'g': return 'c';
        case 't': return 'a';
        default: return c;
    }
}

__device__ __forceinline__ uint64_t complement8(uint64_t w) {
    uint64_t r = 0;
#pragma unroll
    for (uint32_t k = 0; k < 64; k += 8) r |= (uint64_t)complement((uint32_t)(w >> k) & 0xFFu) << k;
    return r;
}

// the last item in [lo, hi] whose first output byte is at or before `at` (off[lo] <= at): the one that holds byte `at`
__device__ __forceinline__ uint64_t item_of(const uint64_t *__restrict__ off, uint64_t lo, uint64_t hi, uint64_t at) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo + 1) >> 1);
        if (off[mid] <= at) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kThreads) void k_lk_gather(const uint64_t *__restrict__ off, const uint64_t *__restrict__ src,
                                                         uint64_t n_items, const uint8_t *__restrict__ text,
                                                         const uint8_t *__restrict__ seq, uint64_t begin, uint64_t end,
                                                         uint8_t *__restrict__ out, int aligned) {
    __shared__ uint64_t span[2];
    const uint64_t t0 = begin + (uint64_t)blockIdx.x * kOutTile, t1 = min(end, t0 + kOutTile);
    if (threadIdx.x < 2) span[threadIdx.x] = item_of(off, 0, n_items - 1, threadIdx.x ? t1 - 1 : t0);
    __syncthreads();
    const uint64_t hi = span[1];
#pragma unroll 1
    for (uint32_t r = 0; r < kOutRows; ++r) {
        const uint64_t o0 = t0 + ((uint64_t)r * kThreads + threadIdx.x) * 16u;
        if (o0 >= t1) break;
        const uint64_t o1 = min(o0 + 16, t1);
        uint64_t w0 = 0, w1 = 0, lo = span[0];
        for (uint64_t cur = o0; cur < o1;) {
            const uint64_t it = item_of(off, lo, hi, cur);
            const uint64_t run = min(o1, off[it + 1]) - cur, skip = cur - off[it], s = src[it];
            const uint8_t *from = (s & kFromText) ? text : seq;
            const uint64_t at = s & kSrcMask;
            if (run == 16) {  // the lane's 16 bytes lie in one item: one 16-byte load (any alignment), turned round in registers
                uint64_t v[2];
                __builtin_memcpy(v, (s & kRev) ? from + (at - skip - 15) : from + (at + skip), 16);
                if (s & kRev) {
                    w0 = complement8(__builtin_bswap64(v[1]));
                    w1 = complement8(__builtin_bswap64(v[0]));
                } else {
                    w0 = v[0];
                    w1 = v[1];
                }
                break;
            }
            for (uint64_t j = 0; j < run; ++j) {
                const uint64_t c = (s & kRev) ? complement(from[at - skip - j]) : from[at + skip + j];
                const uint32_t k = (uint32_t)(cur + j - o0);
                if (k < 8) w0 |= c << (8u * k);
                else w1 |= c << (8u * (k - 8u));
            }
            cur += run;
            lo = it + 1 <= hi ? it + 1 : hi;
        }
        uint8_t *dst = out + (o0 - begin);
        if (aligned && o1 - o0 == 16) {
            *reinterpret_cast<uint4 *>(dst) = make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
        } else {
            for (uint32_t k = 0; k < (uint32_t)(o1 - o0); ++k) dst[k] = (uint8_t)((k < 8 ? w0 >> (8u * k) : w1 >> (8u * (k - 8u))) & 0xFFu);
        }
    }
}

// A device buffer that grows and is never shrunk.
struct Buf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = bytes + bytes / 4 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    ~Buf() {
        if (p) (void)hipFree(p);
    }
};

}  // namespace

struct GafLookupJob {
    Buf tiles, lines, events, items, words;
    const uint8_t *text = nullptr;
    const uint8_t *seq = nullptr;
    uint64_t n_items = 0;
    uint64_t *g_off = nullptr, *g_src = nullptr;
    GafArrays arr;
    hipStream_t last = nullptr;
    bool used = false;
    hipEvent_t reader = nullptr;  // behind the last reader of the arrays on a stream other than `last`
    bool reader_set = false;
    void wait() {
        if (used) (void)hipStreamSynchronize(last);
        if (reader_set) (void)hipEventSynchronize(reader);
        reader_set = false;
    }
    ~GafLookupJob() {
        if (reader) (void)hipEventDestroy(reader);
    }
};

GafLookupJob *gaf_lookup_new() { return new GafLookupJob(); }
void gaf_lookup_free(GafLookupJob *j) {
    if (!j) return;
    j->wait();
    delete j;
}
const GafArrays &gaf_lookup_arrays(const GafLookupJob *j) { return j->arr; }

#define LK_HIP(expr) FGFA_HIP("", expr)

int gaf_lookup_count(GafLookupJob *j, const uint8_t *d_text, size_t len, const GafGraph &g, bool seqs, uint64_t base,
                     hipStream_t stream, GafTotals *totals) {
    *totals = GafTotals();
    j->arr = GafArrays();
    j->n_items = 0;
    j->text = d_text;
    j->seq = g.seq_data;
    if (len == 0) return FLATGFA_OK;
    j->wait();  // (a gather or a copy of the last count may still read what is made again here)
    j->last = stream;
    j->used = true;
    const uint8_t *abase = reinterpret_cast<const uint8_t *>((uintptr_t)d_text & ~(uintptr_t)15);
    const uint64_t lead = (uint64_t)(d_text - abase), vend = lead + len;
    const uint64_t tiles = (vend + kNlTile - 1) / kNlTile;
    if (tiles > 0x7FFFFFFFull) { set_error("gaf lookup: a piece of text beyond 2^45 bytes"); return FLATGFA_ERR_TOO_LARGE; }

    // 1. lines
    LK_HIP(j->words.ensure(64));
    unsigned long long *bad = static_cast<unsigned long long *>(j->words.p);  // parse, name, slice
    LK_HIP(hipMemsetAsync(bad, 0xFF, 24, stream));
    LK_HIP(j->tiles.ensure((tiles + 1 + scan_scratch_words(tiles + 1)) * 8));
    uint64_t *tile_first = static_cast<uint64_t *>(j->tiles.p);
    LK_HIP(hipMemsetAsync(tile_first + tiles, 0, 8, stream));
    {
        ProfScope ps("k_lk_nl_count", stream);
        hipLaunchKernelGGL(k_lk_nl_count, dim3((uint32_t)tiles), dim3(kThreads), 0, stream, abase, lead, vend, tile_first);
    }
    scan_u64(tile_first, tiles + 1, tile_first + tiles + 1, stream);
    uint64_t host[4] = {0, 0, 0, 0};
    LK_HIP(hipMemcpyAsync(host, tile_first + tiles, 8, hipMemcpyDeviceToHost, stream));
    LK_HIP(hipStreamSynchronize(stream));
    const uint64_t L = host[0];
    totals->n_lines = L;
    if (L == 0) return FLATGFA_OK;
    if ((L + 3) / 4 > 0x7FFFFFFFull) { set_error("gaf lookup: more than 2^33 lines in one piece of text"); return FLATGFA_ERR_TOO_LARGE; }

    // 2. fields and token counts
    const uint64_t line_words = 7 * L + 1 + scan_scratch_words(L + 1);
    LK_HIP(j->lines.ensure(line_words * 8));
    uint64_t *w = static_cast<uint64_t *>(j->lines.p);
    uint64_t *line_end = w, *line_first = w + L;  // (L + 1 words)
    LineOut lo{w + 2 * L + 1, w + 3 * L + 1, w + 4 * L + 1, w + 5 * L + 1, w + 6 * L + 1, line_first};
    uint64_t *scan_scratch = w + 7 * L + 1;
    {
        ProfScope ps("k_lk_nl_scatter", stream);
        hipLaunchKernelGGL(k_lk_nl_scatter, dim3((uint32_t)tiles), dim3(kThreads), 0, stream, abase, lead, vend, tile_first, line_end);
    }
    const uint32_t line_grid = (uint32_t)((L + kThreads / 64 - 1) / (kThreads / 64));
    LK_HIP(hipMemsetAsync(line_first + L, 0, 8, stream));
    {
        ProfScope ps("k_lk_parse", stream);
        hipLaunchKernelGGL(k_lk_parse, dim3(line_grid), dim3(kThreads), 0, stream, d_text, line_end, L, lo, bad, base);
    }
    scan_u64(line_first, L + 1, scan_scratch, stream);
    LK_HIP(hipMemcpyAsync(host, line_first + L, 8, hipMemcpyDeviceToHost, stream));
    LK_HIP(hipStreamSynchronize(stream));
    const uint64_t E = host[0];
    totals->n_events = E;

    // 3. events, and the layout of the `-s` text
    LK_HIP(j->events.ensure(E * 21 + 64));
    uint8_t *ev = static_cast<uint8_t *>(j->events.p);
    EventOut eo{};
    eo.a = reinterpret_cast<uint64_t *>(ev);
    eo.b = eo.a + E;
    eo.handle = reinterpret_cast<uint32_t *>(eo.b + E);
    eo.kind = reinterpret_cast<uint8_t *>(eo.handle + E);
    const uint64_t I = E + 2 * L;
    if (seqs) {
        LK_HIP(j->items.ensure((2 * I + 1 + scan_scratch_words(I + 1)) * 8));
        j->g_off = static_cast<uint64_t *>(j->items.p);
        j->g_src = j->g_off + I + 1;
        eo.g_len = j->g_off;
        eo.g_src = j->g_src;
        LK_HIP(hipMemsetAsync(j->g_off + I, 0, 8, stream));
    }
    const Graph dg{g.names.keys, g.names.ids, g.names.n_others, g.names.n_segs, g.names.seq_max, g.seg_seq};
    {
        ProfScope ps("k_lk_events", stream);
        hipLaunchKernelGGL(k_lk_events, dim3(line_grid), dim3(kThreads), 0, stream, d_text, line_end, L, lo, dg, eo, bad + 1, bad + 2,
                           base);
    }
    if (seqs) {
        scan_u64(j->g_off, I + 1, j->g_src + I, stream);
        LK_HIP(hipMemcpyAsync(host + 3, j->g_off + I, 8, hipMemcpyDeviceToHost, stream));
    }
    LK_HIP(hipMemcpyAsync(host, bad, 24, hipMemcpyDeviceToHost, stream));
    LK_HIP(hipStreamSynchronize(stream));
    LK_HIP(hipGetLastError());
    totals->bad_parse = host[0];
    totals->bad_name = host[1];
    totals->bad_slice = host[2];
    totals->seq_bytes = seqs ? host[3] : 0;
    j->n_items = seqs ? I : 0;
    j->arr.line_end = line_end;
    j->arr.name_len = lo.name_len;
    j->arr.line_first = line_first;
    j->arr.handle = eo.handle;
    j->arr.kind = eo.kind;
    j->arr.a = eo.a;
    j->arr.b = eo.b;
    return FLATGFA_OK;
}

int gaf_lookup_gather(GafLookupJob *j, uint64_t begin, uint64_t end, uint8_t *d_out, hipStream_t stream) {
    if (begin >= end) return FLATGFA_OK;
    if (!j->n_items || !d_out) { set_error("gaf lookup: nothing was laid out to gather"); return FLATGFA_ERR_ARG; }
    const uint64_t tiles = (end - begin + kOutTile - 1) / kOutTile;
    if (tiles > 0x7FFFFFFFull) { set_error("gaf lookup: a gather beyond 2^45 bytes"); return FLATGFA_ERR_TOO_LARGE; }
    j->last = stream;
    {
        ProfScope ps("k_lk_gather", stream);
        hipLaunchKernelGGL(k_lk_gather, dim3((uint32_t)tiles), dim3(kThreads), 0, stream, j->g_off, j->g_src, j->n_items, j->text, j->seq,
                           begin, end, d_out, ((uintptr_t)d_out & 15u) == 0 ? 1 : 0);
    }
    LK_HIP(hipGetLastError());
    return FLATGFA_OK;
}

int gaf_lookup_used_on(GafLookupJob *j, hipStream_t stream) {
    if (!j->reader) LK_HIP(hipEventCreateWithFlags(&j->reader, hipEventDisableTiming));
    LK_HIP(hipEventRecord(j->reader, stream));
    j->reader_set = true;
    return FLATGFA_OK;
}

}  // namespace fgfa_dev
