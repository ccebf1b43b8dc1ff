// The packed-sequence codec on gfx950 (flatgfa/src/packedseq.rs): nucleotide text to two bases a byte
// (`seq-export`) and back (`seq-import`).  Pack is a stream compaction whose output unit is half a byte: whitespace out,
// anything but A C T G an error, base 2k into the low nibble of byte k and base 2k + 1 into the high one.
//
// The text is walked in the coordinates of the aligned 16-byte vectors it lies in: position p of that walk is text byte
// p - mis, mis = text & 15, and positions outside [mis, mis + n) are masked -- they share an aligned vector with a text byte, so
// reading them is a read of the same page.  Every load is then a whole aligned vector at any alignment of the text.  The tiles
// of kSeqTile positions are dealt to the grid in equal contiguous ranges, as crush's are.
//
//   k_seq_count   a workgroup per range; a lane classifies 16 bytes a load.  Per range: the kept bases (cnt[]) and the code of
//                 the first one (first[], 0xFF: none).  The smallest offset of a byte that is neither whitespace nor a
//                 nucleotide, with the byte, goes into one word by atomicMin: the same answer whichever workgroup finds what.
//   scan          cnt[] in u64 (the three-launch scan of device_scan.hpp): the kept bases before each range, and the total
//   k_seq_fill    the same walk, a tile at a time: the bytes through LDS, a lane takes 64 consecutive ones, a workgroup scan of
//                 the lanes' counts, the kept codes scattered into LDS a byte each -- laid so that the codes of output byte
//                 x of the tile's aligned destination vectors are at 2x and 2x + 1 -- and a lane packs 32 codes into one 16-byte
//                 store, bytewise at the tile's two ragged ends.
//
// Who writes which byte.  The logical stream is the carry, if there is one, then the kept bases.  An output byte belongs to
// the workgroup that holds its low-nibble base (the carry is workgroup 0's).  Inside a range a tile with an odd number of
// bases to place leaves its last one pending, and the next tile begins with it.  A range that begins at an odd logical index
// skips its first kept base: that base is the high nibble of a byte of an earlier range, which takes the code from first[] --
// going past ranges that keep nothing -- when it ends with a base pending, and writes that one byte; where nothing follows the
// high nibble is 0.  So every byte is written once, by one workgroup, with both nibbles final: no zeroed output, no atomics
// on it, no read-modify-write.
//
//   k_seq_unpack  a lane takes 16 packed bytes a step and writes 32 letters; nibbles above 3 among the first n_bases are
//                 min-reduced into one word as pack's bad bytes are.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>

#include "../../include/flatgfa.h"
#include "device_common.hpp"
#include "device_scan.hpp"
#include "prof.hpp"
#include "seq_device.hpp"

namespace fgfa_dev {
namespace {

#define SEQ_HIP(expr) FGFA_HIP("seq: ", expr)

static_assert(kSeqTile == 64u * kSeqThreads, "fill: a lane takes 64 consecutive bytes of the tile");
static_assert(kSeqTile % (16 * kSeqThreads) == 0, "a tile is whole rounds of one 16-byte vector a lane");
constexpr uint32_t kVecRounds = kSeqTile / (16 * kSeqThreads);
constexpr uint64_t kNone = ~0ull;

struct SeqText {
    const uint4 *vec;   // the aligned vectors the text lies in
    uint64_t mis, end;  // text byte i is position mis + i; end = mis + n
};

// the tiles [*t0, *t1) of this workgroup: the tiles of `total` positions in gridDim.x equal contiguous ranges
__device__ __forceinline__ void my_tiles(uint64_t total, uint64_t *t0, uint64_t *t1) {
    const uint64_t tiles = (total + kSeqTile - 1) / kSeqTile, per = (tiles + gridDim.x - 1) / gridDim.x;
    *t0 = min((uint64_t)blockIdx.x * per, tiles);
    *t1 = min(*t0 + per, tiles);
}

__device__ __forceinline__ bool is_space(uint32_t b) {  // u8::is_ascii_whitespace: space, \t, \n, \x0C, \r -- not \x0B
    return b == 0x20 || (b >= 0x09 && b <= 0x0D && b != 0x0B);
}
// A = 0x41, C = 0x43, T = 0x54, G = 0x47: bits 1 and 2 are the reference's codes A 0, C 1, T 2, G 3
__device__ __forceinline__ uint32_t code_of(uint32_t b) { return (b >> 1) & 3; }

__device__ __forceinline__ uint32_t byte_of(const uint4 &w, uint32_t k) {  // byte k of 16 (selects: no indexed registers)
    const uint32_t word = k < 8 ? (k < 4 ? w.x : w.y) : (k < 12 ? w.z : w.w);
    return (word >> (8 * (k & 3))) & 0xFF;
}

// Four bytes a word at a time: a byte a compare each is what bounds these kernels, not the memory.
// 0x80 in every byte of v that is zero -- exact, nothing carries from one byte into the next
__device__ __forceinline__ uint32_t zero_bytes(uint32_t v) { return ~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v | 0x7F7F7F7Fu); }
// bits 7, 15, 23, 31 as bits 0..3
__device__ __forceinline__ uint32_t flags4(uint32_t z) {
    const uint32_t m = (z >> 7) & 0x01010101u;
    return (m | (m >> 7) | (m >> 14) | (m >> 21)) & 0xF;
}
// which of a word's four bytes are A C T G.  b ^ 0x41 is 0, 2, 6 for A, C, G -- the values without a bit outside 0x06, but
// for 4, which is E -- and 0x15 for T.
__device__ __forceinline__ uint32_t base_flags(uint32_t w) {
    const uint32_t y = w ^ 0x41414141u;
    return flags4((zero_bytes(y & 0xF9F9F9F9u) & ~zero_bytes(y ^ 0x04040404u)) | zero_bytes(y ^ 0x15151515u));
}

// The 16 bytes of one vector at position p0: which are kept bases, and which are neither those nor bases (whitespace and bad
// bytes).  Positions outside [x.mis, x.end) are in neither mask.
__device__ __forceinline__ void classify(const SeqText &x, uint64_t p0, const uint4 &w, uint32_t *basem, uint32_t *otherm) {
    const uint32_t lo = p0 < x.mis ? (uint32_t)min((uint64_t)16, x.mis - p0) : 0u;
    const uint32_t hi = (uint32_t)min((uint64_t)16, x.end - p0);  // (p0 < x.end holds)
    const uint32_t valid = ((1u << hi) - 1) & ~((1u << lo) - 1);
    const uint32_t bm = base_flags(w.x) | (base_flags(w.y) << 4) | (base_flags(w.z) << 8) | (base_flags(w.w) << 12);
    *basem = bm & valid;
    *otherm = ~bm & valid;
}
// of the bytes in otherm (few: a newline a line), those that are not whitespace
__device__ __forceinline__ uint32_t bad_of(const uint4 &w, uint32_t otherm) {
    uint32_t badm = 0;
    while (otherm) {
        const uint32_t k = (uint32_t)__ffs((int)otherm) - 1;
        otherm &= otherm - 1;
        if (!is_space(byte_of(w, k))) badm |= 1u << k;
    }
    return badm;
}

__device__ __forceinline__ uint64_t wave_min(uint64_t v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v = min(v, shfl_xor_u64(v, d));
    return v;
}

__global__ __launch_bounds__(kSeqThreads) void k_seq_count(SeqText x, uint64_t *__restrict__ cnt, uint8_t *__restrict__ first,
                                                           unsigned long long *err) {
    __shared__ uint64_t s_kept[kSeqThreads / 64], s_first[kSeqThreads / 64], s_bad[kSeqThreads / 64];
    const uint32_t t = threadIdx.x, lane = t & 63;
    uint64_t t0, t1;
    my_tiles(x.end, &t0, &t1);
    // a lane's positions only grow, so the first kept base and the first bad byte it meets are its smallest
    uint64_t kept = 0, first_key = kNone, bad_key = kNone;  // position << 2 | code;  offset << 8 | byte
    for (uint64_t tile = t0; tile < t1; ++tile) {
        const uint64_t q0 = tile * kSeqTile;
#pragma unroll
        for (uint32_t i = 0; i < kVecRounds; ++i) {
            const uint64_t p0 = q0 + 16ull * (t + kSeqThreads * i);
            if (p0 >= x.end) continue;
            const uint4 w = x.vec[p0 >> 4];
            uint32_t basem, otherm;
            classify(x, p0, w, &basem, &otherm);
            const uint32_t badm = bad_of(w, otherm);
            kept += (uint32_t)__popc(basem);
            if (basem && first_key == kNone) {
                const uint32_t k = (uint32_t)__ffs((int)basem) - 1;
                first_key = ((p0 + k) << 2) | code_of(byte_of(w, k));
            }
            if (badm && bad_key == kNone) {
                const uint32_t k = (uint32_t)__ffs((int)badm) - 1;
                bad_key = ((p0 + k - x.mis) << 8) | byte_of(w, k);
            }
        }
    }
    kept = wave_sum(kept), first_key = wave_min(first_key), bad_key = wave_min(bad_key);
    if (lane == 0) s_kept[t >> 6] = kept, s_first[t >> 6] = first_key, s_bad[t >> 6] = bad_key;
    __syncthreads();
    if (t == 0) {
        uint64_t all = 0, f = kNone, b = kNone;
        for (int w = 0; w < kSeqThreads / 64; ++w) all += s_kept[w], f = min(f, s_first[w]), b = min(b, s_bad[w]);
        cnt[blockIdx.x] = all;
        first[blockIdx.x] = f == kNone ? (uint8_t)0xFF : (uint8_t)(f & 3);
        if (b != kNone) atomicMin(err, (unsigned long long)b);
    }
}

struct RangeOp {  // the ranges' kept counts -> the kept bases before each range
    const uint64_t *cnt;
    uint64_t *pre;
    __device__ __forceinline__ Sum<uint64_t> load(uint64_t i) const { return Sum<uint64_t>{cnt[i]}; }
    __device__ __forceinline__ void store(uint64_t i, uint64_t before, const Sum<uint64_t> &) const { pre[i] = before; }
};

// four codes, a byte each, to two packed bytes
__device__ __forceinline__ uint32_t pack4(uint32_t w) {
    const uint32_t f = (w | (w >> 4)) & 0x00FF00FFu;
    return (f | (f >> 8)) & 0xFFFFu;
}

// carry: a code 0..3 in front of the kept bases, or kSeqNoCarry
__global__ __launch_bounds__(kSeqThreads) void k_seq_fill(SeqText x, const uint64_t *__restrict__ pre, const uint64_t *__restrict__ cnt,
                                                          const uint8_t *__restrict__ first, int carry, uint8_t *__restrict__ out) {
    __shared__ uint4 raw4[kSeqTile / 16];
    __shared__ uint4 code4[kSeqTile / 16 + 4];  // codes, a byte each: those of byte x of the destination's aligned vectors at 2x, 2x + 1
    uint8_t *codeb = reinterpret_cast<uint8_t *>(code4);
    const uint32_t t = threadIdx.x;
    uint64_t t0, t1;
    my_tiles(x.end, &t0, &t1);
    const uint64_t run = (carry >= 0 ? 1u : 0u) + pre[blockIdx.x];  // the logical index of this range's first kept base
    // uniform over the workgroup: a base waiting for its high nibble; whether the next kept base is an earlier range's; the next output byte
    bool has_pend = blockIdx.x == 0 && carry >= 0, skip = !has_pend && (run & 1);
    uint32_t pend = has_pend ? (uint32_t)carry : 0u;
    uint64_t ob = has_pend ? 0 : (run + 1) / 2;
    for (uint64_t tile = t0; tile < t1; ++tile) {
        const uint64_t q0 = tile * kSeqTile;
#pragma unroll
        for (uint32_t i = 0; i < kVecRounds; ++i) {
            const uint32_t v = t + kSeqThreads * i;
            const uint64_t p0 = q0 + 16ull * v;
            raw4[v] = p0 < x.end ? x.vec[p0 >> 4] : make_uint4(0, 0, 0, 0);
        }
        __syncthreads();
        // bytes [64 t, 64 t + 64) of the tile: the keep flags, and the two bits of each code
        uint64_t keepm = 0, c0 = 0, c1 = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint64_t p0 = q0 + 64ull * t + 16 * k;
            if (p0 >= x.end) break;
            const uint4 w = raw4[4 * t + k];
            uint32_t basem, otherm;
            classify(x, p0, w, &basem, &otherm);
            // bits 1 and 2 of every byte (code_of), sixteen at a time
            const uint32_t b0 = flags4(w.x << 6) | (flags4(w.y << 6) << 4) | (flags4(w.z << 6) << 8) | (flags4(w.w << 6) << 12);
            const uint32_t b1 = flags4(w.x << 5) | (flags4(w.y << 5) << 4) | (flags4(w.z << 5) << 8) | (flags4(w.w << 5) << 12);
            keepm |= (uint64_t)basem << (16 * k), c0 |= (uint64_t)b0 << (16 * k), c1 |= (uint64_t)b1 << (16 * k);
        }
        uint32_t tile_kept = 0;
        const uint32_t before = block_excl_scan<uint32_t, kSeqThreads>((uint32_t)__popcll(keepm), &tile_kept);
        const uint32_t lead = has_pend ? 1u : 0u, sk = skip && tile_kept ? 1u : 0u;
        const uint32_t len = lead + tile_kept - sk;  // the codes this tile places: the pending one, then its own but a skipped first
        const uintptr_t dst = reinterpret_cast<uintptr_t>(out) + ob;
        const uint32_t shift = (uint32_t)(dst & 15);
        if (t == 0 && lead) codeb[2 * shift] = (uint8_t)pend;
        {
            uint64_t m = keepm;
            uint32_t r = before;
            while (m) {
                const uint32_t b = (uint32_t)__ffsll((long long)m) - 1;
                m &= m - 1;
                if (r >= sk) codeb[2 * shift + lead + r - sk] = (uint8_t)(((c0 >> b) & 1) | (((c1 >> b) & 1) << 1));
                ++r;
            }
        }
        __syncthreads();
        const uint32_t nb = len >> 1;
        has_pend = len & 1;
        if (has_pend) pend = codeb[2 * shift + len - 1];
        if (sk) skip = false;
        // bytes [shift, end) of the aligned vectors at dst - shift: whole vectors where all 16 bytes are the tile's
        const uint32_t end = shift + nb;
        for (uint32_t v = t; v * 16 < end; v += kSeqThreads) {
            const uint32_t lo = v * 16, hi = lo + 16;
            const uint4 a = code4[2 * v], b = code4[2 * v + 1];
            const uint4 o = make_uint4(pack4(a.x) | (pack4(a.y) << 16), pack4(a.z) | (pack4(a.w) << 16), pack4(b.x) | (pack4(b.y) << 16),
                                       pack4(b.z) | (pack4(b.w) << 16));
            if (lo >= shift && hi <= end) {
                *reinterpret_cast<uint4 *>(dst - shift + lo) = o;
            } else {
                for (uint32_t k = max(lo, shift); k < min(hi, end); ++k) *reinterpret_cast<uint8_t *>(dst - shift + k) = (uint8_t)byte_of(o, k - lo);
            }
        }
        ob += nb;
        __syncthreads();  // (the LDS is the next tile's)
    }
    if (has_pend && t == 0) {
        // the range ends with a base pending: its high nibble is the first base kept after it, which its range skips
        uint32_t hi = 0;
        for (uint32_t r = blockIdx.x + 1; r < gridDim.x; ++r)
            if (cnt[r]) {
                hi = first[r];
                break;
            }
        out[ob] = (uint8_t)(pend | (hi << 4));
    }
}

// eight nibbles of a word to eight letters: "ACTG"[nibble & 3]
__device__ __forceinline__ void letters8(uint32_t w, uint32_t *lo, uint32_t *hi) {
    constexpr uint32_t kLetters = 0x47544341u;  // 'A' 'C' 'T' 'G', low byte first
    uint32_t a = 0, b = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        a |= ((kLetters >> (8 * ((w >> (4 * q)) & 3))) & 0xFF) << (8 * q);
        b |= ((kLetters >> (8 * ((w >> (4 * q + 16)) & 3))) & 0xFF) << (8 * q);
    }
    *lo = a, *hi = b;
}

// vectors: both pointers are 16-byte aligned
__global__ __launch_bounds__(kSeqThreads) void k_seq_unpack(const uint8_t *__restrict__ packed, uint64_t n_bases, uint8_t *__restrict__ text_out,
                                                            unsigned long long *err, bool vectors) {
    const uint64_t n_bytes = n_bases / 2 + (n_bases & 1), groups = (n_bytes + 15) / 16;
    uint64_t bad_key = kNone;  // base index << 4 | nibble; a lane's groups only grow
    for (uint64_t g = (uint64_t)blockIdx.x * kSeqThreads + threadIdx.x; g < groups; g += (uint64_t)gridDim.x * kSeqThreads) {
        const uint64_t b0 = g * 16;
        if (vectors && b0 + 16 <= n_bytes && 2 * (b0 + 16) <= n_bases) {
            const uint4 w = *reinterpret_cast<const uint4 *>(packed + b0);
            const uint32_t words[4] = {w.x, w.y, w.z, w.w};
            if (((w.x | w.y | w.z | w.w) & 0xCCCCCCCCu) && bad_key == kNone) {
#pragma unroll
                for (uint32_t q = 0; q < 32; ++q) {
                    const uint32_t nib = (words[q >> 3] >> (4 * (q & 7))) & 0xF;
                    if (nib > 3 && bad_key == kNone) bad_key = ((2 * b0 + q) << 4) | nib;
                }
            }
            uint4 o0, o1;
            letters8(w.x, &o0.x, &o0.y), letters8(w.y, &o0.z, &o0.w), letters8(w.z, &o1.x, &o1.y), letters8(w.w, &o1.z, &o1.w);
            uint4 *dst = reinterpret_cast<uint4 *>(text_out + 2 * b0);
            dst[0] = o0, dst[1] = o1;
        } else {
            constexpr uint32_t kLetters = 0x47544341u;
            for (uint64_t k = b0; k < min(b0 + 16, n_bytes); ++k) {
                const uint32_t by = packed[k];
#pragma unroll
                for (uint32_t h = 0; h < 2; ++h) {
                    const uint64_t base = 2 * k + h;
                    if (base >= n_bases) break;  // (the unused high nibble of an odd sequence's last byte)
                    const uint32_t nib = (by >> (4 * h)) & 0xF;
                    if (nib > 3 && bad_key == kNone) bad_key = (base << 4) | nib;
                    text_out[base] = (uint8_t)(kLetters >> (8 * (nib & 3)));
                }
            }
        }
    }
    if (bad_key != kNone) atomicMin(err, (unsigned long long)bad_key);
}

}  // namespace

struct SeqPackJob {
    SeqText x{nullptr, 0, 0};
    uint32_t grid = kSeqGrid;
    bool counted = false;
    uint64_t *cnt = nullptr, *pre = nullptr;
    unsigned long long *err = nullptr;
    uint8_t *first = nullptr;
    Spine<Sum<uint64_t>> range_sp;
    uint64_t kept = 0;
    DeviceMem mem;  // (waits for the last stream used before it frees)
};

// FLATGFA_SEQ_GRID (a test hook): fewer workgroups than kSeqGrid, so that a small text has ranges of several tiles
SeqPackJob *seq_pack_new() {
    SeqPackJob *j = new SeqPackJob();
    if (const char *h = test_hook("FLATGFA_SEQ_GRID")) j->grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(strtoull(h, nullptr, 10), 1), kSeqGrid);
    return j;
}
void seq_pack_free(SeqPackJob *j) { delete j; }

int seq_pack_count(SeqPackJob *j, const uint8_t *text, uint64_t n, uint64_t base_offset, hipStream_t st, uint64_t *n_bases) {
    if (!j || !n_bases || (n && !text)) { set_error("seq-export: NULL argument"); return FLATGFA_ERR_ARG; }
    if (n >= kSeqMaxText) { set_error("seq-export: more than 2^56 bytes of text"); return FLATGFA_ERR_TOO_LARGE; }
    if (j->counted) { set_error("seq-export: this job was counted already"); return FLATGFA_ERR_ARG; }
    const uint64_t mis = n ? (uint64_t)(reinterpret_cast<uintptr_t>(text) & 15) : 0;
    j->x = SeqText{n ? reinterpret_cast<const uint4 *>(text - mis) : nullptr, mis, mis + n};
    j->mem.st = st;
    const uint32_t G = j->grid;
    SEQ_HIP(j->mem.alloc(&j->cnt, 2 * (uint64_t)G));
    j->pre = j->cnt + G;
    SEQ_HIP(j->mem.alloc(&j->first, G));
    SEQ_HIP(j->mem.alloc(&j->err, 1));
    SEQ_HIP(j->range_sp.alloc(&j->mem, blocks(G, kSeqThreads * kSeqScanPer)));
    SEQ_HIP(hipMemsetAsync(j->err, 0xFF, 8, st));
    {
        ProfScope prof("seq_pack_count", st);
        hipLaunchKernelGGL(k_seq_count, dim3(G), dim3(kSeqThreads), 0, st, j->x, j->cnt, j->first, j->err);
    }
    {
        ProfScope prof("seq_pack_scan", st);
        const RangeOp op{j->cnt, j->pre};
        scan_count<kSeqThreads, kSeqScanPer, Sum<uint64_t>>(op, G, j->range_sp, st);
        scan_apply<kSeqThreads, kSeqScanPer, Sum<uint64_t>>(op, G, j->range_sp, st);
    }
    SEQ_HIP(hipGetLastError());
    unsigned long long err = 0;
    SEQ_HIP(hipMemcpyAsync(&err, j->err, 8, hipMemcpyDeviceToHost, st));
    SEQ_HIP(hipMemcpyAsync(&j->kept, j->range_sp.total, 8, hipMemcpyDeviceToHost, st));
    SEQ_HIP(hipStreamSynchronize(st));
    if (err != kNone) {
        char msg[96];
        snprintf(msg, sizeof msg, "seq-export: byte 0x%02x at offset %llu is not a nucleotide", (unsigned)(err & 0xFF),
                 (unsigned long long)(base_offset + (err >> 8)));
        set_error(msg);
        return FLATGFA_ERR_PARSE;
    }
    j->counted = true;
    *n_bases = j->kept;
    return FLATGFA_OK;
}

int seq_pack_fill(SeqPackJob *j, int carry, uint8_t *out, hipStream_t st) {
    if (!j || !j->counted) { set_error("seq-export: fill before a successful count"); return FLATGFA_ERR_ARG; }
    if (carry != kSeqNoCarry && (carry < 0 || carry > 3)) { set_error("seq-export: the carry is -1 (none) or a code 0..3"); return FLATGFA_ERR_ARG; }
    const uint64_t logical = j->kept + (carry >= 0 ? 1 : 0);
    if (logical && !out) { set_error("seq-export: NULL output"); return FLATGFA_ERR_ARG; }
    j->mem.st = st;
    if (logical) {
        ProfScope prof("seq_pack_fill", st);
        hipLaunchKernelGGL(k_seq_fill, dim3(j->grid), dim3(kSeqThreads), 0, st, j->x, j->pre, j->cnt, j->first, carry, out);
    }
    SEQ_HIP(hipGetLastError());
    return FLATGFA_OK;
}

int seq_unpack(const uint8_t *packed, uint64_t n_bases, uint64_t base_offset, uint8_t *text_out, hipStream_t st) {
    if (n_bases && (!packed || !text_out)) { set_error("seq-import: NULL argument"); return FLATGFA_ERR_ARG; }
    if (n_bases >= (1ull << 60)) { set_error("seq-import: more than 2^60 bases"); return FLATGFA_ERR_TOO_LARGE; }
    if (!n_bases) return FLATGFA_OK;
    DeviceMem mem;
    mem.st = st;
    unsigned long long *d_err = nullptr, err = 0;
    SEQ_HIP(mem.alloc(&d_err, 1));
    SEQ_HIP(hipMemsetAsync(d_err, 0xFF, 8, st));
    const bool vectors = ((reinterpret_cast<uintptr_t>(packed) | reinterpret_cast<uintptr_t>(text_out)) & 15) == 0;
    {
        ProfScope prof("seq_unpack", st);
        const uint64_t groups = blocks(seq_packed_bytes(n_bases), 16);
        hipLaunchKernelGGL(k_seq_unpack, dim3(stride_blocks(groups, kSeqThreads, kSeqUnpackGrid)), dim3(kSeqThreads), 0, st, packed, n_bases, text_out,
                           d_err, vectors);
    }
    SEQ_HIP(hipGetLastError());
    SEQ_HIP(hipMemcpyAsync(&err, d_err, 8, hipMemcpyDeviceToHost, st));
    SEQ_HIP(hipStreamSynchronize(st));
    if (err != kNone) {
        set_error("seq-import: nibble " + std::to_string(err & 0xF) + " at base " + std::to_string(base_offset + (err >> 4)) + " is not a nucleotide");
        return FLATGFA_ERR_PARSE;
    }
    return FLATGFA_OK;
}

}  // namespace fgfa_dev

// ---- the device-level C ABI (include/flatgfa.h Part 3) ----
struct flatgfa_dev_seq_pack {
    fgfa_dev::SeqPackJob *job = nullptr;
    ~flatgfa_dev_seq_pack() { fgfa_dev::seq_pack_free(job); }
};

extern "C" {

int flatgfa_dev_seq_pack_count(const uint8_t *text, uint64_t n, void *stream, flatgfa_dev_seq_pack_t **job, uint64_t *n_bases) {
    if (job) *job = nullptr;
    if (!job || !n_bases) { fgfa_dev::set_error("flatgfa_dev_seq_pack_count: NULL argument"); return FLATGFA_ERR_ARG; }
    auto *h = new flatgfa_dev_seq_pack();
    h->job = fgfa_dev::seq_pack_new();
    const int rc = fgfa_dev::seq_pack_count(h->job, text, n, 0, (hipStream_t)stream, n_bases);
    if (rc) {
        delete h;
        return rc;
    }
    *job = h;
    return FLATGFA_OK;
}

int flatgfa_dev_seq_pack_fill(flatgfa_dev_seq_pack_t *job, int carry, uint8_t *out, void *stream) {
    if (!job) { fgfa_dev::set_error("flatgfa_dev_seq_pack_fill: NULL job"); return FLATGFA_ERR_ARG; }
    return fgfa_dev::seq_pack_fill(job->job, carry, out, (hipStream_t)stream);
}

void flatgfa_dev_seq_pack_free(flatgfa_dev_seq_pack_t *job) { delete job; }

int flatgfa_dev_seq_unpack(const uint8_t *packed, uint64_t n_bases, uint8_t *text_out, void *stream) {
    return fgfa_dev::seq_unpack(packed, n_bases, 0, text_out, (hipStream_t)stream);
}

}  // extern "C"
