// Pangenotype rows from GAF text on gfx950 (flatgfa/src/ops/pangenotype.rs:11-70).
//
// A segment id s is covered by a piece of GAF text when some line of it -- the bytes before a '\n', the line not empty and not
// starting with '#' -- names s in its path field: the bytes after the line's 5th tab.  Inside that field every '>' or '<' starts
// a token whose digits are read into a u64 (wrapping) and looked up in the graph's NameMap.  Put per byte: a '>' or '<' counts
// when exactly five tabs precede it in its line, and its line neither starts with '#' nor lacks its '\n'.
//
// The state a byte needs -- "tabs since the line began, saturated at 6" and "offset of the line's first byte" -- composes
// associatively, and is packed into one u64 (bit 3: a '\n' was seen, bits 0-2: tabs, bits 4-63: where the current line starts).
//
//   k_gaf_tiles  one workgroup per tile of 32 KiB: the tile's summary (the state it leaves behind, as if it started a line) and
//                atomicMax of one past its last '\n' into `eff_end` -- the bytes behind the text's last '\n' are not a line.
//   k_gaf_rows   one workgroup per tile.  Wave 0 takes the state the tile starts in from the summaries before it, 64 at a time,
//                back to the nearest tile with a '\n' (or until six tabs settle it); those summaries were written by the
//                previous launch, so no workgroup waits on another.  Then 4 KiB at a time: a 16-byte load per lane, the lanes'
//                states by a workgroup scan, and a lane with a '>' or '<' walks its 16 bytes, reading a token's digits on past
//                its own bytes where the token runs on.  A name sets its bit (read first: the same segments recur millions of
//                times); a name the graph does not have lowers `first_bad` to its line's offset.
//
// Text at any address: positions are counted from the 16-byte boundary below it (`lead` bytes early), and bytes outside
// [lead, end) read as 0, which is none of the bytes that matter.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/flatgfa.h"
#include "device_common.hpp"
#include "gaf_device.hpp"
#include "name_lookup.hpp"
#include "prof.hpp"

namespace fgfa_dev {
namespace {

constexpr int kGafThreads = 256;
constexpr uint32_t kGafSub = kGafThreads * 16;  // bytes per step of a workgroup
constexpr uint32_t kGafSteps = 8;
constexpr uint32_t kGafTile = kGafSub * kGafSteps;

constexpr uint64_t kNl = 8;  // the packed state's "a '\n' was seen" bit

// a then b, over consecutive bytes
__device__ __forceinline__ uint64_t compose(uint64_t a, uint64_t b) {
    if (b & kNl) return b;
    return (a & ~(uint64_t)7) | (uint64_t)min((uint32_t)(a & 7) + (uint32_t)(b & 7), 6u);
}

// 0x80 in every byte of w equal to c (exact: no borrow runs between bytes)
__device__ __forceinline__ uint32_t eq_bytes(uint32_t w, uint32_t c) {
    const uint32_t t = w ^ (c * 0x01010101u);
    return ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t) & 0x80808080u;
}

// the 16 bytes at `vpos` (a multiple of 16), those outside [lo, hi) as 0
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

// The state a lane's 16 bytes leave behind, as if they started a line (the identity is 0).
__device__ __forceinline__ uint64_t lane_state(const uint32_t w[4], uint64_t vpos) {
    uint64_t st = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t nl = eq_bytes(w[j], '\n'), tab = eq_bytes(w[j], '\t');
        uint32_t after = tab;
        if (nl) {
            const uint32_t hb = 31u - (uint32_t)__builtin_clz(nl);  // the high bit of the last '\n'
            after = hb >= 31u ? 0u : tab & ~((2u << hb) - 1u);
            st = ((vpos + 4u * j + (hb >> 3) + 1u) << 4) | kNl;
        }
        st = (st & ~(uint64_t)7) | (uint64_t)min((uint32_t)(st & 7) + (uint32_t)__builtin_popcount(after), 6u);
    }
    return st;
}

__device__ __forceinline__ uint64_t shfl_up64(uint64_t x, int d) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)x, d, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(x >> 32), d, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl64(uint64_t x, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)x, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(x >> 32), src, 64);
    return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(kGafThreads) void k_gaf_tiles(const uint8_t *__restrict__ abase, uint64_t lead, uint64_t vend,
                                                            uint64_t *__restrict__ summary, unsigned long long *__restrict__ eff_end) {
    __shared__ uint64_t part[kGafThreads / 64];
    const uint64_t t0 = (uint64_t)blockIdx.x * kGafTile;
    uint4 v[kGafSteps];
#pragma unroll
    for (uint32_t k = 0; k < kGafSteps; ++k) v[k] = load16(abase, t0 + k * kGafSub + threadIdx.x * 16u, lead, vend);
    uint64_t st = 0;
#pragma unroll
    for (uint32_t k = 0; k < kGafSteps; ++k) {
        const uint32_t w[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
        st = compose(st, lane_state(w, t0 + k * kGafSub + threadIdx.x * 16u));
    }
    // The lanes' states are not in byte order (lane l holds 16 bytes of every 4 KiB), so the tile's state is put together from
    // two reductions: the last '\n' (the largest line start), then the tabs behind it.
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t ls = (st & kNl) ? (st >> 4) : 0;
    for (int d = 32; d >= 1; d >>= 1) ls = max(ls, shfl64(ls, lane ^ d));
    if (lane == 0) part[wave] = ls;
    __syncthreads();
    ls = max(max(part[0], part[1]), max(part[2], part[3]));
    __syncthreads();
    uint32_t tabs = 0;
#pragma unroll
    for (uint32_t k = 0; k < kGafSteps; ++k) {
        const uint32_t w[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
        const uint64_t p = t0 + k * kGafSub + threadIdx.x * 16u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t tab = eq_bytes(w[j], '\t');
            const uint64_t b = p + 4u * j;  // byte 0 of the word; byte i is at b + i, and counts when b + i >= ls
            if (b + 4 <= ls) tab = 0;
            else if (b < ls) tab &= ~0u << (8u * (uint32_t)(ls - b));
            tabs += (uint32_t)__builtin_popcount(tab);
        }
    }
    for (int d = 32; d >= 1; d >>= 1) tabs += (uint32_t)__shfl_xor((int)tabs, d, 64);
    if (lane == 0) part[wave] = tabs;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t t = min((uint32_t)(part[0] + part[1] + part[2] + part[3]), 6u);
        summary[blockIdx.x] = ls ? ((ls << 4) | kNl | t) : (uint64_t)t;
        if (ls) atomicMax(eff_end, (unsigned long long)ls);
    }
}

struct Names {
    const uint64_t *keys;  // the NameMap's `others`, sorted by name
    const uint32_t *ids;
    uint32_t n_others;
    uint32_t n_segs;
    uint64_t seq_max;
};

__device__ __forceinline__ void emit(uint64_t num, const Names &nm, unsigned long long *row,
                                     unsigned long long *first_bad, uint64_t report) {
    const uint32_t id = name_map_get(num, nm.keys, nm.ids, nm.n_others, nm.seq_max);
    if (id >= nm.n_segs) {  // the reference panics: a missing key, or an index past the row
        atomicMin(first_bad, (unsigned long long)report);
        return;
    }
    const unsigned long long bit = 1ull << (id & 63u);
    if (!(row[id >> 6] & bit)) atomicOr(&row[id >> 6], bit);
}

__global__ __launch_bounds__(kGafThreads) void k_gaf_rows(const uint8_t *__restrict__ abase, uint64_t lead,
                                                           const uint64_t *__restrict__ summary,
                                                           const unsigned long long *__restrict__ eff_end, Names nm,
                                                           unsigned long long *row, unsigned long long *first_bad,
                                                           uint64_t base) {
    __shared__ uint64_t wave_total[kGafThreads / 64];
    __shared__ uint64_t carry_s;
    const uint64_t vend = *eff_end;  // one past the last '\n': what lies behind it is not a line
    const uint64_t t0 = (uint64_t)blockIdx.x * kGafTile;
    if (t0 >= vend) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint4 v[kGafSteps];
#pragma unroll
    for (uint32_t k = 0; k < kGafSteps; ++k) v[k] = load16(abase, t0 + k * kGafSub + threadIdx.x * 16u, lead, vend);
    if (wave == 0) {
        // the state at the tile's first byte: back over the tiles before it to the nearest one with a '\n'
        uint64_t ls = lead;
        uint32_t tabs = 0;
        for (int64_t t = (int64_t)blockIdx.x - 1; t >= 0; t -= 64) {
            const int64_t j = t - lane;
            const uint64_t s = j >= 0 ? summary[j] : 0;
            const unsigned long long nl = __builtin_amdgcn_ballot_w64((s & kNl) != 0);
            const int first = nl ? __builtin_ctzll(nl) : 64;
            uint32_t mine = lane <= first ? (uint32_t)(s & 7) : 0u;
            for (int d = 32; d >= 1; d >>= 1) mine += (uint32_t)__shfl_xor((int)mine, d, 64);
            tabs += mine;
            if (nl) {
                ls = shfl64(s, first) >> 4;
                break;
            }
            if (tabs >= 6) break;  // six tabs: nothing before the tile's first '\n' counts, wherever its line began
        }
        if (lane == 0) carry_s = (ls << 4) | kNl | min(tabs, 6u);
    }
    __syncthreads();
    uint64_t carry = carry_s;
    for (uint32_t k = 0; k < kGafSteps; ++k) {
        const uint64_t p = t0 + k * kGafSub + threadIdx.x * 16u;
        const uint32_t w[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
        const uint64_t own = lane_state(w, p);
        uint64_t incl = own;
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t o = shfl_up64(incl, d);
            if (lane >= d) incl = compose(o, incl);
        }
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        uint64_t before = carry;
        for (int q = 0; q < wave; ++q) before = compose(before, wave_total[q]);
        const uint64_t up = shfl_up64(incl, 1);
        const uint64_t st = lane ? compose(before, up) : before;  // the state at this lane's first byte
        uint64_t next = carry;
        for (int q = 0; q < kGafThreads / 64; ++q) next = compose(next, wave_total[q]);
        __syncthreads();
        carry = next;
        uint32_t tok = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) tok |= eq_bytes(w[j], '>') | eq_bytes(w[j], '<');
        if (!tok || p >= vend) continue;  // (a token begun in an earlier lane is finished by that lane)
        uint32_t tabs = (uint32_t)(st & 7);
        uint64_t ls = st >> 4;
        uint64_t hash_ls = ~0ull;  // the line whose first byte was looked at last, and whether it was '#'
        bool hash = false;
        bool in_num = false, ok = false;
        uint64_t num = 0, tok_ls = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t c = (w[i >> 2] >> ((i & 3) * 8)) & 0xFFu;
            const uint64_t at = p + (uint64_t)i;
            if (in_num) {
                if (c - '0' < 10u) {
                    num = num * 10u + (c - '0');
                    continue;
                }
                if (ok) emit(num, nm, row, first_bad, tok_ls - lead + base);
                in_num = false;
            }
            if (c == '\n') {
                tabs = 0;
                ls = at + 1;
            } else if (c == '\t') {
                tabs = min(tabs + 1u, 6u);
            } else if ((c == '>' || c == '<') && tabs == 5u) {
                if (hash_ls != ls) {
                    hash_ls = ls;
                    hash = abase[ls] == '#';  // (ls < at < vend: the line's first byte is text)
                }
                in_num = true;
                ok = !hash;
                num = 0;
                tok_ls = ls;
            }
        }
        if (in_num) {  // the digits run on past this lane's bytes (they end at the line's '\n' at the latest, before vend)
            for (uint64_t q = p + 16; q < vend; ++q) {
                const uint32_t c = abase[q];
                if (c - '0' >= 10u) break;
                num = num * 10u + (c - '0');
            }
            if (ok) emit(num, nm, row, first_bad, tok_ls - lead + base);
        }
    }
}

}  // namespace

size_t gaf_scratch_words(const void *d_text, size_t len) {
    const uint64_t vend = (uint64_t)((uintptr_t)d_text & 15u) + len;
    return (size_t)((vend + kGafTile - 1) / kGafTile) + 1;
}

hipError_t gaf_scan(const uint8_t *d_text, size_t len, const GafNameTable &names, uint64_t *d_row, uint64_t *d_first_bad,
                    uint64_t base, uint64_t *scratch, hipStream_t stream) {
    if (len == 0) return hipSuccess;
    const uint8_t *abase = reinterpret_cast<const uint8_t *>((uintptr_t)d_text & ~(uintptr_t)15);
    const uint64_t lead = (uint64_t)(d_text - abase), vend = lead + len;
    const uint64_t tiles = (vend + kGafTile - 1) / kGafTile;
    if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    uint64_t *eff_end = scratch + tiles;
    hipError_t e = hipMemsetAsync(eff_end, 0, 8, stream);
    if (e != hipSuccess) return e;
    {
        ProfScope ps("k_gaf_tiles", stream);
        hipLaunchKernelGGL(k_gaf_tiles, dim3((uint32_t)tiles), dim3(kGafThreads), 0, stream, abase, lead, vend, scratch,
                           reinterpret_cast<unsigned long long *>(eff_end));
    }
    const Names nm{names.keys, names.ids, names.n_others, names.n_segs, names.seq_max};
    {
        ProfScope ps("k_gaf_rows", stream);
        hipLaunchKernelGGL(k_gaf_rows, dim3((uint32_t)tiles), dim3(kGafThreads), 0, stream, abase, lead, scratch,
                           reinterpret_cast<const unsigned long long *>(eff_end), nm, reinterpret_cast<unsigned long long *>(d_row),
                           reinterpret_cast<unsigned long long *>(d_first_bad), base);
    }
    return hipGetLastError();
}

}  // namespace fgfa_dev
