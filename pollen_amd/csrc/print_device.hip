// The GFA printer (flatgfa/src/print.rs:99-153) on the device, both orders.  DESIGN.md section 19.
//
//   lines    line k of the text has a kind (H, S, P, L) and an index within its kind: closed forms of k in normalized order,
//            line_order[k] and the count of that kind before k -- one scan that sums the three counts side by side -- in a
//            preserved one.  LineOf is the one functor every kernel asks.
//   items    an H, S or L line is one item, a P line of n steps is n: its first carries "P\t{name}\t", its last the overlaps
//            field and the newline, and every one "{segment name}{+|-}" and a ',' (a tab after the last).  The lines' item
//            counts are scanned once (u64 a line); an item finds its line by binary search in them.
//   text     per chunk of items: a scan of the item lengths (k_scan over ItemLen), then k_print_tiles, one workgroup per
//            tile of the chunk's bytes: its first and last item by binary search in the item offsets, one lane per item --
//            digits by division by ten, copies of more than kFlatLongName bytes (bases, optional fields, long path names)
//            left to the whole workgroup -- into LDS, the tile stored with 16-byte vector stores.
//
// The text leaves in pieces as flatten's does (Pipe in text_tiles.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/flatgfa.h"
#include "device_common.hpp"
#include "device_scan.hpp"
#include "host_copy.hpp"
#include "print_device.hpp"
#include "prof.hpp"
#include "text_tiles.hpp"

namespace fgfa_dev {
namespace {

#define PR_HIP(expr) FGFA_HIP("print: ", expr)

enum : uint32_t { kH = 0, kS = 1, kP = 2, kL = 3 };  // flatgfa.rs:262-269

// Which line is k: its kind and its index within the kind.
struct LineOf {
    const uint8_t *order = nullptr;  // a preserved order, with idx; else the closed forms
    const uint32_t *idx = nullptr;
    uint64_t h = 0, s = 0, p = 0;
    __device__ __forceinline__ void operator()(uint64_t k, uint32_t *kind, uint32_t *i) const {
        if (order) {
            *kind = order[k], *i = idx[k];
            return;
        }
        if (k < h) *kind = kH, *i = 0;
        else if (k < h + s) *kind = kS, *i = (uint32_t)(k - h);
        else if (k < h + s + p) *kind = kP, *i = (uint32_t)(k - h - s);
        else *kind = kL, *i = (uint32_t)(k - h - s - p);
    }
};

// the graph, its lines and their items
struct Text {
    PrintGraph g;
    LineOf line;
    const uint64_t *item0 = nullptr;  // u64[n_lines + 1]: the items before each line
    uint64_t n_items = 0;
};

// ---- the lines of a preserved order ----

// the counts of S, P and L lines side by side
struct Kinds {
    using Carry = Kinds;
    using Wide = Kinds;
    uint32_t s, p, l;
    __device__ __forceinline__ static Kinds zero() { return Kinds{0, 0, 0}; }
    __device__ __forceinline__ static Kinds comb(const Kinds &x, const Kinds &y) { return Kinds{x.s + y.s, x.p + y.p, x.l + y.l}; }
    __device__ __forceinline__ Kinds carry() const { return *this; }
    __device__ __forceinline__ static Kinds widen(const Kinds &x) { return x; }
    __device__ __forceinline__ static Kinds after(const Kinds &c) { return c; }
};
struct KindOp {
    const uint8_t *order;
    uint32_t *idx;
    __device__ __forceinline__ Kinds load(uint64_t k) const {
        const uint32_t kind = order[k];
        return Kinds{kind == kS, kind == kP, kind == kL};
    }
    __device__ __forceinline__ void store(uint64_t k, const Kinds &before, const Kinds &me) const {
        idx[k] = me.s ? before.s : me.p ? before.p : me.l ? before.l : 0;
    }
};

// ---- items ----

struct ItemCount {
    PrintGraph g;
    LineOf line;
    uint64_t *item0;
    __device__ __forceinline__ Sum<uint64_t> load(uint64_t k) const {
        uint32_t kind, i;
        line(k, &kind, &i);
        return Sum<uint64_t>{kind == kP ? (uint64_t)(g.paths[6 * (uint64_t)i + 3] - g.paths[6 * (uint64_t)i + 2]) : 1};
    }
    __device__ __forceinline__ void store(uint64_t k, uint64_t before, const Sum<uint64_t> &) const { item0[k] = before; }
};

// item `rank` of the `n` of line (kind, idx); a P line's item is its step `rank`, whose handle is `handle`
struct Item {
    uint32_t kind, idx, rank, n, handle;
};
// item i, whose line lies in [lo, hi]
__device__ __forceinline__ Item item_at(const Text &t, uint64_t i, uint64_t lo, uint64_t hi) {
    const uint64_t k = last_at_or_before(t.item0, lo, hi, i);
    Item it;
    t.line(k, &it.kind, &it.idx);
    const uint64_t first = t.item0[k];
    it.rank = (uint32_t)(i - first), it.n = (uint32_t)(t.item0[k + 1] - first), it.handle = 0;
    if (it.kind == kP) it.handle = t.g.steps[(uint64_t)t.g.paths[6 * (uint64_t)it.idx + 2] + it.rank];
    return it;
}

// print.rs:13-34: "0M" for an empty span, else {length}{letter} per op
__device__ __forceinline__ uint64_t align_len(const PrintGraph &g, uint32_t a0, uint32_t a1) {
    if (a0 == a1) return 2;
    uint64_t n = 0;
    for (uint32_t a = a0; a < a1; ++a) n += digits10(g.alignment[a] >> 8) + 1;
    return n;
}

// the bytes of an item (a P item's handle names a segment)
__device__ __forceinline__ uint64_t item_len(const PrintGraph &g, const Item &it) {
    if (it.kind == kH) return 3 + (uint64_t)g.header_len;  // "H\t", the header, the newline
    if (it.kind == kS) {                                   // "S\t{name}\t{bases}[\t{optional}]\n"
        const PrintSeg s = g.segs[it.idx];
        return 4 + (uint64_t)digits10(s.name) + (s.seq1 - s.seq0) + (s.opt1 != s.opt0 ? 1 + (uint64_t)(s.opt1 - s.opt0) : 0);
    }
    if (it.kind == kL) {  // "L\t{from}\t{+|-}\t{to}\t{+|-}\t{overlap}\n"
        const uint32_t *l = g.links + 4 * (uint64_t)it.idx;
        return 9 + (uint64_t)digits10(g.segs[l[0] >> 1].name) + digits10(g.segs[l[1] >> 1].name) + align_len(g, l[2], l[3]);
    }
    const uint32_t *p = g.paths + 6 * (uint64_t)it.idx;
    uint64_t n = digits10(g.segs[it.handle >> 1].name) + 2;  // the name, the orientation, ',' or a tab
    if (it.rank == 0) n += 3 + (uint64_t)(p[1] - p[0]);      // "P\t{name}\t"
    if (it.rank == it.n - 1) {                               // the overlaps field and the newline
        if (p[4] == p[5]) {
            n += 2;
        } else {
            for (uint32_t o = p[4]; o < p[5]; ++o) n += align_len(g, g.overlaps[2 * (uint64_t)o], g.overlaps[2 * (uint64_t)o + 1]) + 1;
        }
    }
    return n;
}

// every step printed names a segment (else bit 0 of *flag), and *total += the bytes of all items
__global__ __launch_bounds__(kFlatThreads) void k_print_check(Text t, uint64_t *total, uint32_t *flag) {
    uint64_t sum = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kFlatThreads + threadIdx.x; i < t.n_items; i += (uint64_t)gridDim.x * kFlatThreads) {
        const Item it = item_at(t, i, 0, t.g.n_lines - 1);
        if (it.kind == kP && (it.handle >> 1) >= t.g.n_segs) {
            atomicOr(flag, 1u);
            continue;
        }
        sum += item_len(t.g, it);
    }
    uint64_t all = 0;
    (void)block_excl_scan<uint64_t, kFlatThreads>(sum, &all);
    if (threadIdx.x == 0 && all) atomicAdd(reinterpret_cast<unsigned long long *>(total), (unsigned long long)all);
}

// the lengths of the chunk's items [i0, i0 + n), scanned into their offsets within the chunk
struct ItemLen {
    Text t;
    uint64_t i0;
    uint64_t *off;
    __device__ __forceinline__ Sum<uint64_t> load(uint64_t i) const { return Sum<uint64_t>{item_len(t.g, item_at(t, i0 + i, 0, t.g.n_lines - 1))}; }
    __device__ __forceinline__ void store(uint64_t i, uint64_t before, const Sum<uint64_t> &) const { off[i] = before; }
};

// The tile [B0, B0 + tlen) of a chunk of n items and `bytes` bytes; positions are kept relative to B0, so an item that began
// in an earlier tile has a negative one.
__global__ __launch_bounds__(kFlatThreads) void k_print_tiles(Text t, uint64_t i0, uint64_t n, const uint64_t *__restrict__ off, uint64_t bytes,
                                                              uint64_t tile0, uint8_t *__restrict__ out) {
    __shared__ uint4 tile4[kFlatTile / 16];
    __shared__ LongCopy longs[kLongCap];
    __shared__ uint32_t n_long;
    __shared__ uint64_t s_range[4];
    uint8_t *tile = reinterpret_cast<uint8_t *>(tile4);
    const uint32_t lane = threadIdx.x;
    const PrintGraph &g = t.g;
    const uint64_t B0 = (tile0 + blockIdx.x) * kFlatTile;
    const int64_t tlen = (int64_t)min((uint64_t)kFlatTile, bytes - B0);
    for (uint32_t v = lane; v < kFlatTile / 16; v += kFlatThreads) tile4[v] = uint4{0, 0, 0, 0};
    if (lane == 0) {
        n_long = 0;
        // the items that have a byte in the tile, and the lines they belong to
        const uint64_t l0 = last_at_or_before(off, 0, n - 1, B0), l1 = last_at_or_before(off, l0, n - 1, B0 + (uint64_t)tlen - 1);
        const uint64_t k0 = last_at_or_before(t.item0, 0, g.n_lines - 1, i0 + l0);
        s_range[0] = l0, s_range[1] = l1, s_range[2] = k0, s_range[3] = last_at_or_before(t.item0, k0, g.n_lines - 1, i0 + l1);
    }
    __syncthreads();
    const auto put = [&](int64_t at, uint8_t ch) {
        if (at >= 0 && at < tlen) tile[at] = ch;
    };
    const auto put_num = [&](int64_t at, uint64_t x, uint32_t nd) {  // nd digits, the last at at + nd - 1
        if (at >= tlen || at + nd <= 0) return;
        int64_t d = at + nd - 1;
        for (; d >= at && (x >> 32); --d) {
            put(d, (uint8_t)('0' + x % 10));
            x /= 10;
        }
        for (uint32_t y = (uint32_t)x; d >= at; --d) {
            put(d, (uint8_t)('0' + y % 10));
            y /= 10;
        }
    };
    const auto put_bytes = [&](int64_t at, const uint8_t *src, uint32_t len) {
        const int64_t lo = max((int64_t)0, -at), hi = min((int64_t)len, tlen - at);
        if (lo >= hi) return;
        if (hi - lo > (int64_t)kFlatLongName) {
            const uint32_t e = atomicAdd(&n_long, 1u);
            if (e < kLongCap) {
                longs[e] = LongCopy{src + lo, (uint32_t)(at + lo), (uint32_t)(hi - lo)};
                return;
            }
        }
        for (int64_t k = lo; k < hi; ++k) tile[at + k] = src[k];
    };
    const auto put_name = [&](int64_t at, uint32_t handle) {  // a segment's name; returns where it ends
        const uint64_t name = g.segs[handle >> 1].name;
        const uint32_t nd = digits10(name);
        put_num(at, name, nd);
        return at + nd;
    };
    const auto put_align = [&](int64_t at, uint32_t a0, uint32_t a1) {  // print.rs:13-34; returns where it ends
        if (a0 == a1) {
            put(at, '0'), put(at + 1, 'M');
            return at + 2;
        }
        for (uint32_t a = a0; a < a1 && at < tlen; ++a) {
            const uint32_t op = g.alignment[a], nd = digits10(op >> 8);
            put_num(at, op >> 8, nd), at += nd;
            put(at++, (uint8_t)("MNDI"[op & 3]));
        }
        return at;
    };
    const uint64_t l0 = s_range[0], l1 = s_range[1], k0 = s_range[2], k1 = s_range[3];
    for (uint64_t l = l0 + lane; l <= l1; l += kFlatThreads) {
        const Item it = item_at(t, i0 + l, k0, k1);
        int64_t at = (int64_t)(off[l] - B0);
        if (it.kind == kH) {
            put(at++, 'H'), put(at++, '\t');
            put_bytes(at, g.header, g.header_len), at += g.header_len;
            put(at, '\n');
        } else if (it.kind == kS) {
            const PrintSeg s = g.segs[it.idx];
            put(at++, 'S'), put(at++, '\t');
            at = put_name(at, it.idx << 1);
            put(at++, '\t');
            put_bytes(at, g.seq_data + s.seq0, s.seq1 - s.seq0), at += s.seq1 - s.seq0;
            if (s.opt1 != s.opt0) {
                put(at++, '\t');
                put_bytes(at, g.optional_data + s.opt0, s.opt1 - s.opt0), at += s.opt1 - s.opt0;
            }
            put(at, '\n');
        } else if (it.kind == kL) {
            const uint32_t *ln = g.links + 4 * (uint64_t)it.idx;
            put(at++, 'L'), put(at++, '\t');
            at = put_name(at, ln[0]);
            put(at++, '\t'), put(at++, (ln[0] & 1u) ? '-' : '+'), put(at++, '\t');
            at = put_name(at, ln[1]);
            put(at++, '\t'), put(at++, (ln[1] & 1u) ? '-' : '+'), put(at++, '\t');
            at = put_align(at, ln[2], ln[3]);
            put(at, '\n');
        } else {
            const uint32_t *p = g.paths + 6 * (uint64_t)it.idx;
            if (it.rank == 0) {
                put(at++, 'P'), put(at++, '\t');
                put_bytes(at, g.name_data + p[0], p[1] - p[0]), at += p[1] - p[0];
                put(at++, '\t');
            }
            at = put_name(at, it.handle);
            put(at++, (it.handle & 1u) ? '-' : '+');
            if (it.rank != it.n - 1) {
                put(at, ',');
            } else {
                put(at++, '\t');
                if (p[4] == p[5]) put(at++, '*');
                for (uint32_t o = p[4]; o < p[5] && at < tlen; ++o) {
                    if (o != p[4]) put(at++, ',');
                    at = put_align(at, g.overlaps[2 * (uint64_t)o], g.overlaps[2 * (uint64_t)o + 1]);
                }
                put(at, '\n');  // (clipped where a loop above stopped at the tile's end)
            }
        }
    }
    __syncthreads();
    const uint32_t nl = min(n_long, kLongCap);
    for (uint32_t e = 0; e < nl; ++e) {
        const LongCopy c = longs[e];
        for (uint32_t k = lane; k < c.len; k += kFlatThreads) tile[c.dst + k] = c.src[k];
    }
    __syncthreads();
    uint4 *dst = reinterpret_cast<uint4 *>(out + (uint64_t)blockIdx.x * kFlatTile);
    for (uint32_t v = lane; v < kFlatTile / 16; v += kFlatThreads) dst[v] = tile4[v];
}

}  // namespace

// ---- host side ----

struct PrintJob : PieceBufs {
    uint64_t chunk_items = kPrintChunkItems;
    uint64_t chunks = 0;
    uint64_t *off = nullptr;    // u64[chunk_items]: item offsets within the chunk
    uint64_t *total = nullptr;  // the check's byte count, then its flag word
    Spine<Sum<uint64_t>> sp;    // the chunk's scan
    Text t;
    bool begun = false;
    DeviceMem mem;
};

PrintJob *print_new(uint64_t chunk_items) {
    PrintJob *j = new PrintJob();
    j->chunk_items = std::max<uint64_t>(chunk_items, 1);
    return j;
}

void print_free(PrintJob *j) {
    if (!j) return;
    pieces_free(j);
    delete j;  // (the device memory goes with mem)
}

uint64_t print_chunks(const PrintJob *j) { return j->chunks; }

int print_begin(PrintJob *j, const PrintGraph &g, hipStream_t st, uint64_t *bytes) {
    if (!j || !bytes) { set_error("print: NULL argument"); return FLATGFA_ERR_ARG; }
    j->begun = false;
    *bytes = 0;
    if (int rc = pieces_ready(j, &j->mem, st, "print: ")) return rc;
    Text &t = j->t;
    t = Text();
    t.g = g;
    t.line.h = g.header_lines, t.line.s = g.seg_lines, t.line.p = g.path_lines;
    if (!g.n_lines) {  // an empty graph: no text
        j->begun = true;
        return FLATGFA_OK;
    }
    if (!j->total) {
        PR_HIP(j->mem.alloc(&j->total, 2));
        PR_HIP(j->mem.alloc(&j->off, j->chunk_items));
        PR_HIP(j->sp.alloc(&j->mem, blocks(j->chunk_items, kFlatThreads * kFlatScanPer)));
    }
    const uint64_t line_tiles = blocks(g.n_lines, kFlatThreads * kFlatScanPer);
    if (g.line_order) {  // each line's index within its kind
        uint32_t *idx = nullptr;
        Spine<Kinds> sp;
        PR_HIP(j->mem.alloc(&idx, g.n_lines));
        PR_HIP(sp.alloc(&j->mem, line_tiles));
        const KindOp op{g.line_order, idx};
        ProfScope prof("print_order", st);
        scan_count<kFlatThreads, kFlatScanPer, Kinds>(op, g.n_lines, sp, st);
        scan_apply<kFlatThreads, kFlatScanPer, Kinds>(op, g.n_lines, sp, st);
        PR_HIP(hipGetLastError());
        t.line.order = g.line_order, t.line.idx = idx;
    }
    uint64_t *item0 = nullptr;
    {
        Spine<Sum<uint64_t>> sp;
        PR_HIP(j->mem.alloc(&item0, g.n_lines + 1));
        PR_HIP(sp.alloc(&j->mem, line_tiles));
        const ItemCount op{g, t.line, item0};
        ProfScope prof("print_items", st);
        scan_count<kFlatThreads, kFlatScanPer, Sum<uint64_t>>(op, g.n_lines, sp, st);
        scan_apply<kFlatThreads, kFlatScanPer, Sum<uint64_t>>(op, g.n_lines, sp, st);
        PR_HIP(hipGetLastError());
        PR_HIP(hipMemcpyAsync(item0 + g.n_lines, sp.total, 8, hipMemcpyDeviceToDevice, st));
        PR_HIP(hipMemcpyAsync(&t.n_items, sp.total, 8, hipMemcpyDeviceToHost, st));
        PR_HIP(hipStreamSynchronize(st));
    }
    t.item0 = item0;
    uint64_t got[2] = {0, 0};
    PR_HIP(hipMemsetAsync(j->total, 0, 16, st));
    {
        const uint32_t grid = stride_blocks(t.n_items, kFlatThreads * 8, 1u << 16);
        ProfScope prof("print_check", st);
        hipLaunchKernelGGL(k_print_check, dim3(grid), dim3(kFlatThreads), 0, st, t, j->total, reinterpret_cast<uint32_t *>(j->total + 1));
    }
    PR_HIP(hipGetLastError());
    PR_HIP(hipMemcpyAsync(got, j->total, 16, hipMemcpyDeviceToHost, st));
    PR_HIP(hipStreamSynchronize(st));
    if (got[1]) {
        set_error("print: a step refers to a segment id that is out of range");
        return FLATGFA_ERR_BOUNDS;
    }
    *bytes = got[0];
    j->begun = true;
    return FLATGFA_OK;
}

int print_emit(PrintJob *j, FlatSink sink, void *ctx) {
    if (!j || !sink) { set_error("print: NULL argument"); return FLATGFA_ERR_ARG; }
    if (!j->begun) { set_error("print: emit before a successful begin"); return FLATGFA_ERR_ARG; }
    j->chunks = 0;
    const Text &t = j->t;
    if (!t.n_items) return FLATGFA_OK;
    Pipe pipe(j, sink, ctx, "print: ");
    if (!pipe.pin) { set_error("print: no pinned staging buffer"); return FLATGFA_ERR_HIP; }
    const hipStream_t st = j->st;
    for (uint64_t i0 = 0; i0 < t.n_items; i0 += j->chunk_items, ++j->chunks) {
        const uint64_t n = std::min<uint64_t>(j->chunk_items, t.n_items - i0);
        const ItemLen op{t, i0, j->off};
        {
            ProfScope prof("print_item_scan", st);
            scan_count<kFlatThreads, kFlatScanPer, Sum<uint64_t>>(op, n, j->sp, st);
            scan_apply<kFlatThreads, kFlatScanPer, Sum<uint64_t>>(op, n, j->sp, st);
        }
        PR_HIP(hipGetLastError());
        uint64_t bytes = 0;  // (behind the pieces of the chunk before: the offsets are theirs until they are formatted)
        PR_HIP(hipMemcpyAsync(&bytes, j->sp.total, 8, hipMemcpyDeviceToHost, st));
        PR_HIP(hipStreamSynchronize(st));
        if (int rc = pipe.tiles(bytes, [&](uint8_t *out, uint64_t tile0, uint32_t nt) {
                ProfScope prof("print_tiles", st);
                hipLaunchKernelGGL(k_print_tiles, dim3(nt), dim3(kFlatThreads), 0, st, t, i0, n, j->off, bytes, tile0, out);
            }))
            return rc;
    }
    return pipe.finish();
}

}  // namespace fgfa_dev
