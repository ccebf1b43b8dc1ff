// The GFA parser on gfx950 (flatgfa/src/parse.rs:24-126, gfaline.rs): the inverse of print_device.hip.
//
// The text is uploaded once and stays in device memory for the call.  The kernels judge the PLAIN grammar only (see
// parse_device.hpp and DESIGN.md): whatever else they meet raises a bit of the not-plain word -- grammar, name or limit --
// and the caller hands the same bytes to the host parser, whose handle or error is then the call's.  No kernel takes an
// index from the text: every position is a byte offset below n, every rank comes from a scan of counts made from the same
// bytes, and every read is of [0, n).
//
//   k_nl_count / k_line_fill   per tile of 4 KiB: the '\n' count, scanned over the tiles, then every line's start (u64) and
//                              kind byte (the line_order pool as it stands).  An empty line, another kind, no tab at byte 1:
//                              grammar.  Compacting scans over the kinds give the segment lines and the deferred lines (L and P
//                              in file order, or L then P for parse_stream), and a scan over those each one's link / path rank.
//   k_s_count / k_s_fill       a wave per S line: the name (wrapping u64), the first tab behind it by ballots, the sequence and
//                              the optional bytes copied 64 bytes a step.
//   k_lp_count / k_lp_fill     a wave per deferred line.  L: the head read by every lane alike, the CIGAR by the wave (wave_cigar:
//                              every byte is classified against its predecessor, an op letter walks back over its digits, ranks
//                              are ballot prefixes).  P: tab 2 from the front and the last tab from the back by ballots, the
//                              overlaps by wave_cigar with commas, the name copied 64 bytes a step.
//   k_steps<count / fill>      the hot path, by tile of text bytes, 16 bytes a lane.  A tile finds the step fields it overlaps
//                              by bisection over the fields' starts; a byte inside a field is classified against its
//                              predecessor (digit after digit, comma or field start; sign after digit; comma after sign; field
//                              end after sign or field start); signs are counted, the counts scanned over lanes and tiles, and
//                              each sign walks back over its digits, resolves the name (name_lookup.hpp) and stores
//                              steps[rank].  Ranks ascend with byte position, so the store is coalesced and needs no atomic.
//                              The lanes that own a field's first byte and the byte behind its last write the path's span.
//
// Between the count and the fill passes the S names go to the host, where NameMap::insert builds the map in segment order
// (exact for duplicates, name 0, the sequential prefix, names out of order), and its export_sorted table comes back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/flatgfa.h"
#include "device_common.hpp"
#include "device_scan.hpp"
#include "host_copy.hpp"
#include "name_lookup.hpp"
#include "parse_device.hpp"

namespace fgfa_dev {
namespace {

constexpr int kT = kParseThreads;
constexpr uint32_t kTile = kParseTile;
constexpr uint32_t kWin = kParseWindow;
enum : uint32_t { fGrammar = 1, fName = 2, fLimit = 4 };
constexpr uint8_t kBadKind = 0xFF;

__device__ __forceinline__ bool is_digit(uint8_t c) { return (uint8_t)(c - '0') < 10; }
__device__ __forceinline__ bool is_sign(uint8_t c) { return c == '+' || c == '-'; }
__device__ __forceinline__ bool is_op(uint8_t c) { return c == 'M' || c == 'N' || c == 'D' || c == 'I'; }
// gfaline.rs:178-184 with flatgfa.rs:213-221
__device__ __forceinline__ uint32_t op_code(uint8_t c) { return c == 'M' ? 0u : c == 'N' ? 1u : c == 'I' ? 2u : 3u; }
// a byte outside the text reads as a line end
__device__ __forceinline__ uint8_t rd(const uint8_t *__restrict__ t, uint64_t n, uint64_t p) { return p < n ? t[p] : (uint8_t)'\n'; }

// the 16 bytes at p0 (a multiple of 16; the text starts on an allocation's boundary), those at or past n as '\n'
__device__ __forceinline__ void load16(const uint8_t *__restrict__ t, uint64_t n, uint64_t p0, uint8_t b[16]) {
    if (p0 + 16 <= n) {
        const uint4 v = *reinterpret_cast<const uint4 *>(t + p0);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 16; ++q) b[q] = (uint8_t)(w[q >> 2] >> ((q & 3) * 8));
    } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) b[q] = rd(t, n, p0 + q);
    }
}

// ---- the line index ----

__global__ __launch_bounds__(kT) void k_nl_count(const uint8_t *__restrict__ text, uint64_t n, uint64_t *__restrict__ tile_cnt) {
    const uint64_t p0 = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * 16u;
    uint8_t b[16];
    load16(text, n, p0, b);
    uint32_t c = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) c += (p0 + q < n && b[q] == '\n') ? 1u : 0u;
    uint32_t total;
    (void)block_excl_scan<uint32_t, kT>(c, &total);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

// the kind of the line that starts at s: the line_order byte (flatgfa.rs:262-269), or kBadKind with the grammar bit
__device__ __forceinline__ void write_kind(const uint8_t *__restrict__ text, uint64_t n, uint64_t line, uint64_t s, uint8_t *__restrict__ kind,
                                           uint32_t *flags) {
    const uint8_t c0 = rd(text, n, s), c1 = rd(text, n, s + 1);
    uint8_t k = c0 == 'H' ? 0 : c0 == 'S' ? 1 : c0 == 'P' ? 2 : c0 == 'L' ? 3 : kBadKind;
    if (c1 != '\t') k = kBadKind;
    if (k == kBadKind) atomicOr(flags, fGrammar);
    kind[line] = k;
}

// starts[k] for every line k, and starts[n_lines] = one past the last line's end + 1: line k is [starts[k], starts[k + 1] - 1)
__global__ __launch_bounds__(kT) void k_line_fill(const uint8_t *__restrict__ text, uint64_t n, const uint64_t *__restrict__ tile_first,
                                                  uint64_t n_lines, int virt, uint64_t *__restrict__ starts, uint8_t *__restrict__ kind,
                                                  uint32_t *flags) {
    const uint64_t p0 = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * 16u;
    uint8_t b[16];
    load16(text, n, p0, b);
    uint32_t c = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) c += (p0 + q < n && b[q] == '\n') ? 1u : 0u;
    uint32_t total;
    uint64_t j = tile_first[blockIdx.x] + block_excl_scan<uint32_t, kT>(c, &total);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        if (p0 + q < n && b[q] == '\n') {
            if (j + 1 <= n_lines) starts[j + 1] = p0 + q + 1;
            if (j + 1 < n_lines) write_kind(text, n, j + 1, p0 + q + 1, kind, flags);
            ++j;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        starts[0] = 0;
        if (n_lines) write_kind(text, n, 0, 0, kind, flags);
        if (virt) starts[n_lines] = n + 1;  // (the unterminated last line of parse_stream ends at n)
    }
}

// ---- the scans' ops (device_scan.hpp) ----

using SumU = Sum<uint64_t>;

// an exclusive scan in place
struct InPlaceOp {
    uint64_t *a;
    __device__ __forceinline__ SumU load(uint64_t i) const { return SumU{a[i]}; }
    __device__ __forceinline__ void store(uint64_t i, uint64_t before, const SumU &) const { a[i] = before; }
};
// the lines of one kind (or of L and P together), compacted in order behind list[off]
struct KindOp {
    const uint8_t *kind;
    uint32_t *list;
    uint64_t off;
    uint8_t want;
    bool lp;
    __device__ __forceinline__ SumU load(uint64_t i) const {
        const uint8_t k = kind[i];
        return SumU{(lp ? (k == 2 || k == 3) : k == want) ? 1ull : 0ull};
    }
    __device__ __forceinline__ void store(uint64_t i, uint64_t before, const SumU &me) const {
        if (me.v) list[off + before] = (uint32_t)i;
    }
};
// the links before every deferred line
struct LinkRankOp {
    const uint8_t *kind;
    const uint32_t *dl;
    uint32_t *lrank;
    __device__ __forceinline__ SumU load(uint64_t d) const { return SumU{kind[dl[d]] == 3 ? 1ull : 0ull}; }
    __device__ __forceinline__ void store(uint64_t d, uint64_t before, const SumU &) const { lrank[d] = (uint32_t)before; }
};

// ---- numbers and CIGARs ----

// parse_num (gfaline.rs:153-158) at *p, before e: *v (wrapping) and *p behind the digits.  fGrammar: no digit.  More than kWin
// digits: the limit bit in *soft, and the line is read on, so that a grammar fault behind it is still seen.
__device__ __forceinline__ uint32_t read_num(const uint8_t *__restrict__ text, uint64_t *p, uint64_t e, uint64_t *v, uint32_t *soft) {
    uint64_t x = 0, q = *p;
    uint32_t nd = 0;
    while (q < e && is_digit(text[q])) {
        x = x * 10 + (uint64_t)(text[q] - '0');
        ++q;
        ++nd;
    }
    if (!nd) return fGrammar;
    if (nd > kWin) *soft |= fLimit;
    *p = q;
    *v = x;
    return 0;
}
__device__ __forceinline__ bool eat(const uint8_t *__restrict__ text, uint64_t *p, uint64_t e, uint8_t c) {
    if (*p >= e || text[*p] != c) return false;
    ++*p;
    return true;
}

// the first tab of [a, e), or e: the whole wave calls it
__device__ __forceinline__ uint64_t wave_find_tab(const uint8_t *__restrict__ text, uint64_t a, uint64_t e, int lane) {
    for (uint64_t b = a; b < e; b += 64) {
        const uint64_t i = b + (uint64_t)lane;
        const unsigned long long m = __ballot(i < e && text[i] == '\t');
        if (m) return b + (uint64_t)(__ffsll((long long)m) - 1);
    }
    return e;
}
// the last tab of [a, e), or e
__device__ __forceinline__ uint64_t wave_find_last_tab(const uint8_t *__restrict__ text, uint64_t a, uint64_t e, int lane) {
    for (uint64_t hi = e; hi > a;) {
        const uint64_t lo = hi - a >= 64 ? hi - 64 : a, i = lo + (uint64_t)lane;
        const unsigned long long m = __ballot(i < hi && text[i] == '\t');
        if (m) return lo + (uint64_t)(63 - __clzll((long long)m));
        hi = lo;
    }
    return e;
}
// dst[0, len) = text[src, src + len), 64 bytes a step
__device__ __forceinline__ void wave_copy(uint8_t *__restrict__ dst, const uint8_t *__restrict__ text, uint64_t src, uint64_t len, int lane) {
    for (uint64_t i = (uint64_t)lane; i < len; i += 64) dst[i] = text[src + i];
}

struct CigarCount {
    uint32_t ops, cigars;
};
// The CIGARs of text[a, e) -- (<digits>[MNDI])+ separated by single commas where `commas`, one (<digits>[MNDI])* where not --
// by the whole wave, 64 bytes a step.  Counting, every byte is judged against its predecessor; filling, an op letter of rank
// r writes align[abase + r] and a comma closes its CIGAR's span in ov (u32 pairs, from CIGAR obase on; null: no spans).
template <bool kFill>
__device__ __forceinline__ CigarCount wave_cigar(const uint8_t *__restrict__ text, uint64_t a, uint64_t e, bool commas, int lane, uint32_t *flags,
                                                 uint32_t *__restrict__ align, uint64_t abase, uint32_t *__restrict__ ov, uint64_t obase) {
    uint32_t run_ops = 0, run_c = 0;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (uint64_t b = a; b < e; b += 64) {
        const uint64_t i = b + (uint64_t)lane;
        const bool in = i < e;
        const uint8_t c = in ? text[i] : 0, prev = in && i > a ? text[i - 1] : 0;
        const bool first = i == a, op = in && is_op(c), com = in && c == ',';
        uint64_t v = 0;
        if (op) {
            uint64_t k = i, mul = 1;
            uint32_t nd = 0;
            while (k > a && nd < kWin && is_digit(text[k - 1])) {
                v += (uint64_t)(text[k - 1] - '0') * mul;
                mul *= 10;
                --k;
                ++nd;
            }
            if (!kFill) {
                if (nd == kWin && k > a && is_digit(text[k - 1])) atomicOr(flags, fLimit);
                else if ((v & 0xFFFFFFFFull) > 255) atomicOr(flags, fGrammar);  // flatgfa.rs:228
            }
        }
        if (!kFill && in) {
            bool ok;
            if (is_digit(c)) ok = first || is_digit(prev) || is_op(prev) || (commas && prev == ',');
            else if (op) ok = !first && is_digit(prev);
            else if (com) ok = commas && !first && is_op(prev);
            else ok = false;
            if (!ok) atomicOr(flags, fGrammar);
        }
        const unsigned long long opmask = __ballot(op), cmask = __ballot(com);
        if (kFill) {
            const uint32_t my_ops = run_ops + (uint32_t)__popcll(opmask & lt), my_c = run_c + (uint32_t)__popcll(cmask & lt);
            if (op) align[abase + my_ops] = (((uint32_t)v & 0xFFu) << 8) | op_code(c);
            if (com && ov) {
                ov[2 * (obase + my_c) + 1] = (uint32_t)(abase + my_ops);
                ov[2 * (obase + my_c + 1)] = (uint32_t)(abase + my_ops);
            }
        }
        run_ops += (uint32_t)__popcll(opmask);
        run_c += (uint32_t)__popcll(cmask);
    }
    if (e > a && lane == 0) {
        if (!kFill && !is_op(text[e - 1])) atomicOr(flags, fGrammar);
        if (kFill && ov) {
            ov[2 * obase] = (uint32_t)abase;
            ov[2 * (obase + run_c) + 1] = (uint32_t)(abase + run_ops);
        }
    }
    return CigarCount{run_ops, e > a ? run_c + 1 : 0u};
}

// ---- S lines ----

struct SegArrays {
    uint64_t *name, *pos;  // the name; where the sequence starts in the text
    uint64_t *seq, *opt;   // [segments + 1]: the lengths, then (scanned in place) the offsets into seq_data / optional_data
};

__global__ __launch_bounds__(kT) void k_s_count(const uint8_t *__restrict__ text, const uint64_t *__restrict__ starts,
                                                const uint32_t *__restrict__ idx_s, uint64_t n_segs, SegArrays o, uint32_t *flags) {
    const uint64_t s = ((uint64_t)blockIdx.x * kT + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (s >= n_segs) return;
    const uint64_t line = idx_s[s], a = starts[line], e = starts[line + 1] - 1;
    uint64_t p = a + 2, name = 0, seq_len = 0, opt_len = 0;
    uint32_t soft = 0;
    uint32_t bad = read_num(text, &p, e, &name, &soft);
    if (!bad && !eat(text, &p, e, '\t')) bad = fGrammar;
    if (!bad) {
        const uint64_t tab = wave_find_tab(text, p, e, lane);
        seq_len = tab - p;
        opt_len = tab < e ? e - tab - 1 : 0;
    }
    if (lane == 0) {
        if (bad | soft) atomicOr(flags, bad | soft);
        o.name[s] = name;
        o.pos[s] = p;
        o.seq[s] = seq_len;
        o.opt[s] = opt_len;
    }
}

__global__ __launch_bounds__(kT) void k_s_fill(const uint8_t *__restrict__ text, uint64_t n_segs, SegArrays o, uint32_t *__restrict__ segs,
                                               uint8_t *__restrict__ seq_data, uint8_t *__restrict__ optional_data) {
    const uint64_t s = ((uint64_t)blockIdx.x * kT + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (s >= n_segs) return;
    const uint64_t p = o.pos[s], s0 = o.seq[s], s1 = o.seq[s + 1], o0 = o.opt[s], o1 = o.opt[s + 1];
    wave_copy(seq_data + s0, text, p, s1 - s0, lane);
    wave_copy(optional_data + o0, text, p + (s1 - s0) + 1, o1 - o0, lane);  // (behind the tab; nothing where there is none)
    if (lane == 0) {
        const uint64_t name = o.name[s];
        uint32_t *g = segs + 6 * s;
        g[0] = (uint32_t)name;
        g[1] = (uint32_t)(name >> 32);
        g[2] = (uint32_t)s0;
        g[3] = (uint32_t)s1;
        g[4] = (uint32_t)o0;
        g[5] = (uint32_t)o1;
    }
}

// ---- L and P lines, in deferred order ----

struct DeferArrays {
    const uint32_t *dl;     // the deferred lines
    const uint32_t *lrank;  // the links before each: line d is link lrank[d] or path d - lrank[d]
    uint64_t *ops;          // [deferred + 1]: the ops of each line, then the offsets into alignment
    uint64_t *cig;          // where each line's CIGAR / overlaps field starts
    uint64_t *l_names;      // [2 * links]
    uint8_t *l_orient;      // bit 0: from is backward, bit 1: to is
    uint64_t *fs, *fe;      // [paths]: the step field
    uint64_t *p_name;       // [paths + 1]: name lengths, then offsets into name_data
    uint64_t *p_ovl;        // [paths + 1]: overlaps, then offsets into the overlaps pool
};

__global__ __launch_bounds__(kT) void k_lp_count(const uint8_t *__restrict__ text, const uint64_t *__restrict__ starts,
                                                 const uint8_t *__restrict__ kind, uint64_t n_defer, DeferArrays o, uint32_t *flags) {
    const uint64_t d = ((uint64_t)blockIdx.x * kT + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (d >= n_defer) return;
    const uint64_t line = o.dl[d], a = starts[line], e = starts[line + 1] - 1;
    uint64_t p = a + 2;
    if (kind[line] == 3) {
        const uint64_t li = o.lrank[d];
        uint64_t from = 0, to = 0;
        uint32_t orient = 0;
        uint32_t soft = 0;
        uint32_t bad = read_num(text, &p, e, &from, &soft);
        if (!bad && !eat(text, &p, e, '\t')) bad = fGrammar;
        if (!bad && p < e && is_sign(text[p])) orient |= text[p++] == '-' ? 1u : 0u;
        else if (!bad) bad = fGrammar;
        if (!bad && !eat(text, &p, e, '\t')) bad = fGrammar;
        if (!bad) bad = read_num(text, &p, e, &to, &soft);
        if (!bad && !eat(text, &p, e, '\t')) bad = fGrammar;
        if (!bad && p < e && is_sign(text[p])) orient |= text[p++] == '-' ? 2u : 0u;
        else if (!bad) bad = fGrammar;
        if (!bad && !eat(text, &p, e, '\t')) bad = fGrammar;
        CigarCount cc{0, 0};
        if (!bad) cc = wave_cigar<false>(text, p, e, false, lane, flags, nullptr, 0, nullptr, 0);
        if (lane == 0) {
            if (bad | soft) atomicOr(flags, bad | soft);
            o.ops[d] = cc.ops;
            o.cig[d] = p;
            o.l_names[2 * li] = from;
            o.l_names[2 * li + 1] = to;
            o.l_orient[li] = (uint8_t)orient;
        }
        return;
    }
    const uint64_t pi = d - o.lrank[d];
    // tab 2 from the front, the tab before the overlaps from the back: what lies between is the step field, tabs and all
    const uint64_t tab2 = wave_find_tab(text, p, e, lane);
    const uint64_t last = tab2 < e ? wave_find_last_tab(text, tab2 + 1, e, lane) : e;
    const bool bad = tab2 == e || last == e;  // (no steps column, or no overlaps column)
    CigarCount cc{0, 0};
    if (!bad) {
        const uint64_t q = last + 1;
        if (q == e) {
            if (lane == 0) atomicOr(flags, fGrammar);  // an empty overlaps field
        } else if (!(e - q == 1 && text[q] == '*')) {
            cc = wave_cigar<false>(text, q, e, true, lane, flags, nullptr, 0, nullptr, 0);
        }
    }
    if (lane == 0) {
        if (bad) atomicOr(flags, fGrammar);
        o.ops[d] = cc.ops;
        o.cig[d] = bad ? e : last + 1;
        o.fs[pi] = bad ? e : tab2 + 1;
        o.fe[pi] = bad ? e : last;
        o.p_name[pi] = bad ? 0 : tab2 - p;
        o.p_ovl[pi] = cc.cigars;
    }
}

struct NameTab {
    const uint64_t *keys;
    const uint32_t *ids;
    uint32_t n_others;
    uint64_t seq_max;
};
// the handle of `name` with `backward`; a name without a segment, name 0 or an id >= 2^31 (flatgfa.rs:194): the name bit
__device__ __forceinline__ uint32_t handle_of(uint64_t name, bool backward, const NameTab &nm, uint32_t *flags) {
    const uint32_t id = name_map_get(name, nm.keys, nm.ids, nm.n_others, nm.seq_max);
    if (id & 0x80000000u) {
        atomicOr(flags, fName);
        return 0;
    }
    return (id << 1) | (backward ? 1u : 0u);
}

struct Pools {
    uint32_t *segs, *paths, *links, *steps, *overlaps, *alignment;
    uint8_t *seq_data, *name_data, *optional_data;
};

__global__ __launch_bounds__(kT) void k_lp_fill(const uint8_t *__restrict__ text, const uint64_t *__restrict__ starts,
                                                const uint8_t *__restrict__ kind, uint64_t n_defer, DeferArrays o, NameTab nm, Pools g,
                                                uint32_t *flags) {
    const uint64_t d = ((uint64_t)blockIdx.x * kT + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (d >= n_defer) return;
    const uint64_t line = o.dl[d], a = starts[line], e = starts[line + 1] - 1;
    const uint64_t a0 = o.ops[d], a1 = o.ops[d + 1], q = o.cig[d];
    if (kind[line] == 3) {
        const uint64_t li = o.lrank[d];
        wave_cigar<true>(text, q, e, false, lane, flags, g.alignment, a0, nullptr, 0);
        if (lane == 0) {
            const uint32_t orient = o.l_orient[li];
            uint32_t *l = g.links + 4 * li;
            l[0] = handle_of(o.l_names[2 * li], orient & 1u, nm, flags);
            l[1] = handle_of(o.l_names[2 * li + 1], orient & 2u, nm, flags);
            l[2] = (uint32_t)a0;
            l[3] = (uint32_t)a1;
        }
        return;
    }
    const uint64_t pi = d - o.lrank[d];
    const uint64_t n0 = o.p_name[pi], n1 = o.p_name[pi + 1], v0 = o.p_ovl[pi], v1 = o.p_ovl[pi + 1];
    wave_copy(g.name_data + n0, text, a + 2, n1 - n0, lane);
    if (v1 > v0) wave_cigar<true>(text, q, e, true, lane, flags, g.alignment, a0, g.overlaps, v0);
    if (lane == 0) {
        uint32_t *p = g.paths + 6 * pi;  // (the steps span is k_steps')
        p[0] = (uint32_t)n0;
        p[1] = (uint32_t)n1;
        p[4] = (uint32_t)v0;
        p[5] = (uint32_t)v1;
    }
}

// ---- steps ----

// the first field of [lo, hi) that starts behind x, or hi
__device__ __forceinline__ uint32_t first_field_after(const uint64_t *__restrict__ fs, uint32_t lo, uint32_t hi, uint64_t x) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (fs[mid] > x) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// What a lane's walk over its bytes starts from: the field that holds p0 or lies before it (cur; -1: none), the next one.
struct FieldCursor {
    int64_t cur;
    uint32_t nxt;
    uint64_t cfs, cfe, nfs;
};

// kMode 0: the signs inside step fields, every byte judged; 1: the signs; 2: the steps and the spans, from rank `rank` on
template <int kMode>
__device__ __forceinline__ uint32_t walk_steps(const uint8_t *__restrict__ text, uint64_t n, const uint8_t b[16], uint64_t p0, FieldCursor f,
                                               const uint64_t *__restrict__ fs, const uint64_t *__restrict__ fe, uint32_t n_paths, uint32_t rank,
                                               const NameTab &nm, uint32_t *__restrict__ steps, uint32_t *__restrict__ paths, uint32_t *flags) {
    uint32_t cnt = 0;
    bool bad = false;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const uint64_t p = p0 + q;
        if (p >= n) break;
        if (p == f.nfs) {  // (field starts ascend strictly: at most one at a byte)
            f.cur = f.nxt++;
            f.cfs = p;
            f.cfe = fe[f.cur];
            f.nfs = f.nxt < n_paths ? fs[f.nxt] : ~0ull;
            if (kMode == 2) paths[6 * (uint64_t)f.cur + 2] = rank + cnt;
        }
        if (f.cur < 0) continue;
        if (p == f.cfe) {
            if (kMode == 2) paths[6 * (uint64_t)f.cur + 3] = rank + cnt;
            if (kMode == 0 && f.cfe > f.cfs && !is_sign(q ? b[q - 1] : text[p - 1])) bad = true;
        } else if (p >= f.cfs && p < f.cfe) {
            const uint8_t c = b[q];
            if (kMode == 0) {
                const bool first = p == f.cfs;
                const uint8_t prev = first ? 0 : (q ? b[q - 1] : text[p - 1]);
                bool ok;
                if (is_digit(c)) ok = first || is_digit(prev) || prev == ',';
                else if (is_sign(c)) ok = !first && is_digit(prev);
                else if (c == ',') ok = !first && is_sign(prev);
                else ok = false;
                bad |= !ok;
            }
            if (is_sign(c)) {
                if (kMode == 2) {
                    uint64_t k = p, v = 0, mul = 1;
                    uint32_t nd = 0;
                    while (k > f.cfs && nd < kWin && is_digit(text[k - 1])) {
                        v += (uint64_t)(text[k - 1] - '0') * mul;
                        mul *= 10;
                        --k;
                        ++nd;
                    }
                    if (nd == kWin && k > f.cfs && is_digit(text[k - 1])) atomicOr(flags, fLimit);
                    else steps[rank + cnt] = handle_of(v, c == '-', nm, flags);
                }
                ++cnt;
            }
        }
    }
    if (kMode == 0 && bad) atomicOr(flags, fGrammar);
    return cnt;
}

// count: tile_cnt[tile] = the tile's steps.  fill: tile_cnt holds the steps before each tile.
template <bool kFill>
__global__ __launch_bounds__(kT) void k_steps(const uint8_t *__restrict__ text, uint64_t n, const uint64_t *__restrict__ fs,
                                              const uint64_t *__restrict__ fe, uint32_t n_paths, uint64_t *__restrict__ tile_cnt, NameTab nm,
                                              uint32_t *__restrict__ steps, uint32_t *__restrict__ paths, uint32_t *flags) {
    __shared__ uint32_t s_lo, s_hi;
    const uint64_t t0 = (uint64_t)blockIdx.x * kTile, p0 = t0 + (uint64_t)threadIdx.x * 16u;
    if (threadIdx.x == 0) {  // the fields that start in the tile are [s_lo, s_hi)
        s_lo = t0 ? first_field_after(fs, 0, n_paths, t0 - 1) : 0;
        s_hi = first_field_after(fs, s_lo, n_paths, t0 + kTile - 1);
    }
    __syncthreads();
    FieldCursor f;
    f.nxt = p0 ? first_field_after(fs, s_lo, s_hi, p0 - 1) : 0;  // the first field that starts at or behind p0
    f.cur = (int64_t)f.nxt - 1;
    f.cfs = f.cur >= 0 ? fs[f.cur] : 0;
    f.cfe = f.cur >= 0 ? fe[f.cur] : 0;
    f.nfs = f.nxt < n_paths ? fs[f.nxt] : ~0ull;
    uint8_t b[16];
    load16(text, n, p0, b);
    if (!kFill) {
        const uint32_t c = walk_steps<0>(text, n, b, p0, f, fs, fe, n_paths, 0, nm, steps, paths, flags);
        uint32_t total;
        (void)block_excl_scan<uint32_t, kT>(c, &total);
        if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
    } else {
        const uint32_t c = walk_steps<1>(text, n, b, p0, f, fs, fe, n_paths, 0, nm, steps, paths, flags);
        uint32_t total;
        const uint32_t rank = (uint32_t)tile_cnt[blockIdx.x] + block_excl_scan<uint32_t, kT>(c, &total);
        (void)walk_steps<2>(text, n, b, p0, f, fs, fe, n_paths, rank, nm, steps, paths, flags);
    }
}

// ---- host side ----

template <class Op>
void scan_total(const Op &op, uint64_t n, const Spine<SumU> &sp, hipStream_t st) {
    scan_count<kT, kParseScanPer, SumU>(op, n, sp, st);
}
template <class Op>
void scan_all(const Op &op, uint64_t n, const Spine<SumU> &sp, hipStream_t st) {
    scan_count<kT, kParseScanPer, SumU>(op, n, sp, st);
    scan_apply<kT, kParseScanPer, SumU>(op, n, sp, st);
}
uint32_t wave_grid(uint64_t items) { return (uint32_t)blocks(items * 64, kT); }

int not_plain(ParseInfo *info, uint32_t flags) {
    info->device_route = 0;
    info->reason = (flags & fGrammar) ? kParseGrammar : (flags & fLimit) ? kParseLimit : kParseName;
    return FLATGFA_OK;
}

double ms_since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

#define PARSE_HIP(expr) FGFA_HIP("device GFA parser: ", expr)

// The events of one call: mark() records one on the stream; the marks come in pairs around device work, and ms() adds up
// what lies between the two of every pair in [first, first + n).
struct Marks {
    hipStream_t st;
    std::vector<hipEvent_t> ev;
    explicit Marks(hipStream_t s) : st(s) {}
    Marks(const Marks &) = delete;
    Marks &operator=(const Marks &) = delete;
    ~Marks() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    hipError_t mark() {
        hipEvent_t e = nullptr;
        hipError_t rc = hipEventCreate(&e);
        if (rc != hipSuccess) return rc;
        ev.push_back(e);
        return hipEventRecord(e, st);
    }
    hipError_t ms(size_t first, size_t n, double *out) const {
        *out = 0;
        for (size_t i = first; i + 1 < first + n && i + 1 < ev.size(); i += 2) {
            float f = 0;
            const hipError_t rc = hipEventElapsedTime(&f, ev[i], ev[i + 1]);
            if (rc != hipSuccess) return rc;
            *out += (double)f;
        }
        return hipSuccess;
    }
};

}  // namespace

int parse_device(const uint8_t *text, size_t n, bool stream_mode, uint64_t item_limit, hipStream_t st, fgfa::Store *out, ParseInfo *info) {
    *out = fgfa::Store();
    *info = ParseInfo();
    const uint64_t tiles = blocks(n, kTile);
    info->tiles = tiles;
    info->device_route = 1;
    if (n == 0) return FLATGFA_OK;  // (no line: every pool is empty)
    if (tiles > 0x7FFFFFFFull) return not_plain(info, fLimit);
    const auto t_begin = std::chrono::steady_clock::now();
    DeviceMem m;
    m.st = st;
    uint8_t *d_text = nullptr;
    uint32_t *d_flags = nullptr;
    PARSE_HIP(m.alloc(&d_text, n));
    PARSE_HIP(m.alloc(&d_flags, 1));
    PARSE_HIP(staged_copy(d_text, text, n, hipMemcpyHostToDevice, st));
    PARSE_HIP(hipMemsetAsync(d_flags, 0, 4, st));
    info->upload_ms = ms_since(t_begin);
    const auto t_device = std::chrono::steady_clock::now();
    Marks all(st), steps_only(st);  // every kernel and scan of the call; the two step kernels

    // ---- the line index ----
    uint64_t *d_tile = nullptr;  // [tiles + 1]: the lines, later the steps, before each tile
    PARSE_HIP(m.alloc(&d_tile, tiles + 1));
    Spine<SumU> sp;  // (one spine for every scan: they run one behind another on the stream)
    PARSE_HIP(sp.alloc(&m, blocks(tiles + 1, kParseScanTile)));
    PARSE_HIP(hipMemsetAsync(d_tile + tiles, 0, 8, st));
    PARSE_HIP(all.mark());
    hipLaunchKernelGGL(k_nl_count, dim3((uint32_t)tiles), dim3(kT), 0, st, d_text, (uint64_t)n, d_tile);
    scan_all(InPlaceOp{d_tile}, tiles + 1, sp, st);
    PARSE_HIP(all.mark());
    uint64_t n_nl = 0;
    PARSE_HIP(hipMemcpyAsync(&n_nl, d_tile + tiles, 8, hipMemcpyDeviceToHost, st));
    PARSE_HIP(hipStreamSynchronize(st));
    const int virt = stream_mode && text[n - 1] != '\n' ? 1 : 0;  // parse_stream keeps the unterminated last line (parse.rs:32)
    const uint64_t n_lines = n_nl + (uint64_t)virt;
    if (n_lines > item_limit) return not_plain(info, fLimit);
    if (n_lines == 0) return FLATGFA_OK;
    uint64_t *d_starts = nullptr;
    uint8_t *d_kind = nullptr;
    PARSE_HIP(m.alloc(&d_starts, n_lines + 1));
    PARSE_HIP(m.alloc(&d_kind, n_lines));
    Spine<SumU> spl;
    PARSE_HIP(spl.alloc(&m, blocks(n_lines + 1, kParseScanTile)));
    PARSE_HIP(all.mark());
    hipLaunchKernelGGL(k_line_fill, dim3((uint32_t)tiles), dim3(kT), 0, st, d_text, (uint64_t)n, d_tile, n_lines, virt, d_starts, d_kind, d_flags);
    uint64_t n_kind[4] = {0, 0, 0, 0};  // H, S, P, L
    for (int k = 0; k < 4; ++k) {
        scan_total(KindOp{d_kind, nullptr, 0, (uint8_t)k, false}, n_lines, spl, st);
        PARSE_HIP(hipMemcpyAsync(&n_kind[k], spl.total, 8, hipMemcpyDeviceToHost, st));
    }
    PARSE_HIP(all.mark());
    uint32_t flags = 0;
    PARSE_HIP(hipMemcpyAsync(&flags, d_flags, 4, hipMemcpyDeviceToHost, st));
    PARSE_HIP(hipStreamSynchronize(st));
    if (flags) return not_plain(info, flags);
    const uint64_t n_h = n_kind[0], n_segs = n_kind[1], n_paths = n_kind[2], n_links = n_kind[3], n_defer = n_paths + n_links;
    if (n_h > 1) return not_plain(info, fGrammar);  // flatgfa.rs:444 (the host parser judges what an empty first header means)
    if (n_segs > item_limit || n_paths > item_limit || n_links > item_limit) return not_plain(info, fLimit);

    uint32_t *d_idx_h = nullptr, *d_idx_s = nullptr, *d_dl = nullptr, *d_lrank = nullptr;
    PARSE_HIP(m.alloc(&d_idx_h, 1));
    PARSE_HIP(m.alloc(&d_idx_s, n_segs));
    PARSE_HIP(m.alloc(&d_dl, n_defer));
    PARSE_HIP(m.alloc(&d_lrank, n_defer));
    PARSE_HIP(all.mark());
    if (n_h) scan_all(KindOp{d_kind, d_idx_h, 0, 0, false}, n_lines, spl, st);
    if (n_segs) scan_all(KindOp{d_kind, d_idx_s, 0, 1, false}, n_lines, spl, st);
    if (n_defer) {
        if (stream_mode) {  // parse_stream unwinds the links, then the paths (parse.rs:63-72)
            scan_all(KindOp{d_kind, d_dl, 0, 3, false}, n_lines, spl, st);
            scan_all(KindOp{d_kind, d_dl, n_links, 2, false}, n_lines, spl, st);
        } else {
            scan_all(KindOp{d_kind, d_dl, 0, 0, true}, n_lines, spl, st);
        }
        scan_all(LinkRankOp{d_kind, d_dl, d_lrank}, n_defer, spl, st);
    }
    PARSE_HIP(all.mark());
    uint64_t hdr[2] = {0, 0};
    if (n_h) {
        uint32_t hl = 0;
        PARSE_HIP(hipMemcpyAsync(&hl, d_idx_h, 4, hipMemcpyDeviceToHost, st));
        PARSE_HIP(hipStreamSynchronize(st));
        PARSE_HIP(hipMemcpyAsync(hdr, d_starts + hl, 16, hipMemcpyDeviceToHost, st));
    }

    // ---- the count passes ----
    SegArrays sa{};
    PARSE_HIP(m.alloc(&sa.name, n_segs));
    PARSE_HIP(m.alloc(&sa.pos, n_segs));
    PARSE_HIP(m.alloc(&sa.seq, n_segs + 1));
    PARSE_HIP(m.alloc(&sa.opt, n_segs + 1));
    PARSE_HIP(hipMemsetAsync(sa.seq + n_segs, 0, 8, st));
    PARSE_HIP(hipMemsetAsync(sa.opt + n_segs, 0, 8, st));
    DeferArrays da{};
    da.dl = d_dl;
    da.lrank = d_lrank;
    PARSE_HIP(m.alloc(&da.ops, n_defer + 1));
    PARSE_HIP(m.alloc(&da.cig, n_defer));
    PARSE_HIP(m.alloc(&da.l_names, 2 * n_links));
    PARSE_HIP(m.alloc(&da.l_orient, n_links));
    PARSE_HIP(m.alloc(&da.fs, n_paths));
    PARSE_HIP(m.alloc(&da.fe, n_paths));
    PARSE_HIP(m.alloc(&da.p_name, n_paths + 1));
    PARSE_HIP(m.alloc(&da.p_ovl, n_paths + 1));
    PARSE_HIP(hipMemsetAsync(da.ops + n_defer, 0, 8, st));
    PARSE_HIP(hipMemsetAsync(da.p_name + n_paths, 0, 8, st));
    PARSE_HIP(hipMemsetAsync(da.p_ovl + n_paths, 0, 8, st));
    PARSE_HIP(hipMemsetAsync(d_tile + tiles, 0, 8, st));
    PARSE_HIP(all.mark());  // (every allocation of the pass lies before it: the events time the device's work alone)
    if (n_segs) hipLaunchKernelGGL(k_s_count, dim3(wave_grid(n_segs)), dim3(kT), 0, st, d_text, d_starts, d_idx_s, n_segs, sa, d_flags);
    scan_all(InPlaceOp{sa.seq}, n_segs + 1, spl, st);
    scan_all(InPlaceOp{sa.opt}, n_segs + 1, spl, st);
    if (n_defer) hipLaunchKernelGGL(k_lp_count, dim3(wave_grid(n_defer)), dim3(kT), 0, st, d_text, d_starts, d_kind, n_defer, da, d_flags);
    scan_all(InPlaceOp{da.ops}, n_defer + 1, spl, st);
    scan_all(InPlaceOp{da.p_name}, n_paths + 1, spl, st);
    scan_all(InPlaceOp{da.p_ovl}, n_paths + 1, spl, st);
    const NameTab no_names{nullptr, nullptr, 0, 0};
    PARSE_HIP(steps_only.mark());
    hipLaunchKernelGGL((k_steps<false>), dim3((uint32_t)tiles), dim3(kT), 0, st, d_text, (uint64_t)n, da.fs, da.fe, (uint32_t)n_paths, d_tile, no_names,
                       (uint32_t *)nullptr, (uint32_t *)nullptr, d_flags);
    PARSE_HIP(steps_only.mark());
    scan_all(InPlaceOp{d_tile}, tiles + 1, sp, st);
    PARSE_HIP(all.mark());
    uint64_t tot[6] = {0, 0, 0, 0, 0, 0};  // seq_data, optional_data, alignment, name_data, overlaps, steps
    PARSE_HIP(hipMemcpyAsync(&tot[0], sa.seq + n_segs, 8, hipMemcpyDeviceToHost, st));
    PARSE_HIP(hipMemcpyAsync(&tot[1], sa.opt + n_segs, 8, hipMemcpyDeviceToHost, st));
    PARSE_HIP(hipMemcpyAsync(&tot[2], da.ops + n_defer, 8, hipMemcpyDeviceToHost, st));
    PARSE_HIP(hipMemcpyAsync(&tot[3], da.p_name + n_paths, 8, hipMemcpyDeviceToHost, st));
    PARSE_HIP(hipMemcpyAsync(&tot[4], da.p_ovl + n_paths, 8, hipMemcpyDeviceToHost, st));
    PARSE_HIP(hipMemcpyAsync(&tot[5], d_tile + tiles, 8, hipMemcpyDeviceToHost, st));
    PARSE_HIP(hipMemcpyAsync(&flags, d_flags, 4, hipMemcpyDeviceToHost, st));
    PARSE_HIP(hipStreamSynchronize(st));
    if (flags) return not_plain(info, flags);
    for (uint64_t t : tot)
        if (t > item_limit) return not_plain(info, fLimit);
    if (n_h && hdr[1] - 1 - (hdr[0] + 2) > item_limit) return not_plain(info, fLimit);

    // ---- the name map, made on the host in segment order (namemap.rs) ----
    NameTab nm{nullptr, nullptr, 0, 0};
    {
        std::vector<uint64_t> names(n_segs);
        if (n_segs) PARSE_HIP(staged_copy(names.data(), sa.name, n_segs * 8, hipMemcpyDeviceToHost, st));
        fgfa::NameMap map;
        for (uint64_t i = 0; i < n_segs; ++i) map.insert(names[i], (uint32_t)i);
        std::vector<std::pair<uint64_t, uint32_t>> others;
        map.export_sorted(&nm.seq_max, &others);
        std::vector<uint64_t> keys(others.size());
        std::vector<uint32_t> ids(others.size());
        for (size_t i = 0; i < others.size(); ++i) keys[i] = others[i].first, ids[i] = others[i].second;
        uint64_t *d_keys = nullptr;
        uint32_t *d_ids = nullptr;
        PARSE_HIP(m.alloc(&d_keys, keys.size()));
        PARSE_HIP(m.alloc(&d_ids, ids.size()));
        if (!keys.empty()) {
            PARSE_HIP(staged_copy(d_keys, keys.data(), keys.size() * 8, hipMemcpyHostToDevice, st));
            PARSE_HIP(staged_copy(d_ids, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, st));
        }
        nm.keys = d_keys;
        nm.ids = d_ids;
        nm.n_others = (uint32_t)others.size();
    }

    // ---- the fill passes ----
    Pools g{};
    PARSE_HIP(m.alloc(&g.segs, 6 * n_segs));
    PARSE_HIP(m.alloc(&g.paths, 6 * n_paths));
    PARSE_HIP(m.alloc(&g.links, 4 * n_links));
    PARSE_HIP(m.alloc(&g.steps, tot[5]));
    PARSE_HIP(m.alloc(&g.overlaps, 2 * tot[4]));
    PARSE_HIP(m.alloc(&g.alignment, tot[2]));
    PARSE_HIP(m.alloc(&g.seq_data, tot[0]));
    PARSE_HIP(m.alloc(&g.name_data, tot[3]));
    PARSE_HIP(m.alloc(&g.optional_data, tot[1]));
    PARSE_HIP(all.mark());
    if (n_segs) hipLaunchKernelGGL(k_s_fill, dim3(wave_grid(n_segs)), dim3(kT), 0, st, d_text, n_segs, sa, g.segs, g.seq_data, g.optional_data);
    if (n_defer) hipLaunchKernelGGL(k_lp_fill, dim3(wave_grid(n_defer)), dim3(kT), 0, st, d_text, d_starts, d_kind, n_defer, da, nm, g, d_flags);
    PARSE_HIP(steps_only.mark());
    hipLaunchKernelGGL((k_steps<true>), dim3((uint32_t)tiles), dim3(kT), 0, st, d_text, (uint64_t)n, da.fs, da.fe, (uint32_t)n_paths, d_tile, nm, g.steps,
                       g.paths, d_flags);
    PARSE_HIP(steps_only.mark());
    PARSE_HIP(all.mark());
    PARSE_HIP(hipMemcpyAsync(&flags, d_flags, 4, hipMemcpyDeviceToHost, st));
    PARSE_HIP(hipStreamSynchronize(st));
    PARSE_HIP(hipGetLastError());
    if (flags) return not_plain(info, flags);
    PARSE_HIP(steps_only.ms(0, 4, &info->step_ms));
    PARSE_HIP(all.ms(0, all.ev.size(), &info->kernel_ms));
    info->device_ms = ms_since(t_device);

    // ---- the pools ----
    const auto t_down = std::chrono::steady_clock::now();
    const auto fetch = [&](void *dst, const void *src, uint64_t bytes) {
        return bytes ? staged_copy(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
    };
    if (n_h) out->header.assign(text + hdr[0] + 2, text + hdr[1] - 1);
    out->segs.resize(n_segs);
    out->paths.resize(n_paths);
    out->links.resize(n_links);
    out->steps.resize(tot[5]);
    out->seq_data.resize(tot[0]);
    out->overlaps.resize(tot[4]);
    out->alignment.resize(tot[2]);
    out->name_data.resize(tot[3]);
    out->optional_data.resize(tot[1]);
    out->line_order.resize(n_lines);
    PARSE_HIP(fetch(out->segs.data(), g.segs, n_segs * 24));
    PARSE_HIP(fetch(out->paths.data(), g.paths, n_paths * 24));
    PARSE_HIP(fetch(out->links.data(), g.links, n_links * 16));
    PARSE_HIP(fetch(out->steps.data(), g.steps, tot[5] * 4));
    PARSE_HIP(fetch(out->seq_data.data(), g.seq_data, tot[0]));
    PARSE_HIP(fetch(out->overlaps.data(), g.overlaps, tot[4] * 8));
    PARSE_HIP(fetch(out->alignment.data(), g.alignment, tot[2] * 4));
    PARSE_HIP(fetch(out->name_data.data(), g.name_data, tot[3]));
    PARSE_HIP(fetch(out->optional_data.data(), g.optional_data, tot[1]));
    PARSE_HIP(fetch(out->line_order.data(), d_kind, n_lines));
    info->download_ms = ms_since(t_down);
    return FLATGFA_OK;
}

}  // namespace fgfa_dev
