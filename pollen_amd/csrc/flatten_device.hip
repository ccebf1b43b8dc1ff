// Flatten (slow_odgi/slow_odgi/flatten.py) on the device: the legend, the FASTA record and the BED table.  DESIGN.md section 15.
//
//   legend   an exclusive u64 scan of the segment lengths (the three-launch scan of device_scan.hpp)
//   FASTA    k_flat_fasta, one workgroup per tile of output bytes: the tile's first segment by binary search in the legend,
//            the bases gathered into LDS with the newline rule applied (lane-consecutive bytes, so lane-consecutive reads of
//            seq_data inside a segment), the tile stored with 16-byte vector stores.  Reads no step.
//   BED      per chunk of lines: a scan of the line lengths (k_scan over FlatLineLen), then k_flat_bed, one workgroup per
//            tile of the chunk's bytes: its first and last line by binary search in the line offsets, one lane per line --
//            digits by division by ten, names of more than kFlatLongName bytes left to the whole workgroup -- into LDS, the
//            tile stored with 16-byte vector stores.  Reads no base.
//
// Both texts leave in pieces of kFlatPieceBytes: a piece is formatted into one of two device buffers, copied into one half
// of a borrowed staging buffer on the job's copy stream, and handed to the sink while the next piece travels (Pipe in
// text_tiles.hpp, which the GFA printer shares).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/flatgfa.h"
#include "device_common.hpp"
#include "device_scan.hpp"
#include "flatten_device.hpp"
#include "host_copy.hpp"
#include "prof.hpp"
#include "text_tiles.hpp"

namespace fgfa_dev {
namespace {

#define FL_HIP(expr) FGFA_HIP("flatten: ", expr)

constexpr uint32_t kBedFixed = 7;  // five tabs, the strand, the newline
const char kBedHeader[] = "#name\tstart\tend\tpath.name\tstrand\tstep.rank\n";

// ---- the legend ----
struct LegendOp {
    const uint32_t *len;
    uint64_t *out;
    __device__ __forceinline__ Sum<uint64_t> load(uint64_t i) const { return Sum<uint64_t>{len[i]}; }
    __device__ __forceinline__ void store(uint64_t i, uint64_t before, const Sum<uint64_t> &) const { out[i] = before; }
};

// ---- FASTA ----

// Byte q of the body is '\n' when q % 81 == 80 or q is the last byte, else base q - q / 81.
__global__ __launch_bounds__(kFlatThreads) void k_flat_fasta(FlatSeqs g, uint64_t body, uint64_t tile0, uint8_t *__restrict__ out) {
    __shared__ uint4 tile4[kFlatTile / 16];
    __shared__ uint64_t s_range[2];
    uint8_t *tile = reinterpret_cast<uint8_t *>(tile4);
    const uint32_t t = threadIdx.x;
    const uint64_t q0 = (tile0 + blockIdx.x) * kFlatTile;
    const uint32_t tlen = (uint32_t)min((uint64_t)kFlatTile, body - q0);
    for (uint32_t v = t; v < kFlatTile / 16; v += kFlatThreads) tile4[v] = uint4{0, 0, 0, 0};
    if (t == 0 && g.total) {  // the segments of the tile's first and last base (a newline's position gives the base behind it)
        const uint64_t q1 = q0 + tlen - 1;
        const uint64_t b0 = min(q0 - q0 / (kFlatWrap + 1), g.total - 1), b1 = min(q1 - q1 / (kFlatWrap + 1), g.total - 1);
        s_range[0] = last_at_or_before(g.legend, 0, g.n_segs - 1, b0);
        s_range[1] = last_at_or_before(g.legend, s_range[0], g.n_segs - 1, b1);
    }
    __syncthreads();
    uint64_t s = 0, s_hi = 0, seg_begin = 0, seg_end = 0;  // the lane's current segment: bases [seg_begin, seg_end)
    uint32_t src = 0;
    if (g.total) s = s_range[0], s_hi = s_range[1], seg_begin = g.legend[s], seg_end = g.legend[s + 1], src = g.seg_seq[2 * s];
    for (uint32_t k = t; k < tlen; k += kFlatThreads) {
        const uint64_t q = q0 + k, line = q / (kFlatWrap + 1);
        uint8_t ch = '\n';
        if (q - line * (kFlatWrap + 1) != kFlatWrap && q != body - 1) {
            const uint64_t b = q - line;
            if (b >= seg_end) {  // the next segment, or -- past a run of empty ones, or many short ones -- a search
                ++s;
                if (b >= g.legend[s + 1]) s = last_at_or_before(g.legend, s, s_hi, b);
                seg_begin = g.legend[s], seg_end = g.legend[s + 1], src = g.seg_seq[2 * s];
            }
            ch = g.seq_data[src + (b - seg_begin)];
        }
        tile[k] = ch;
    }
    __syncthreads();
    uint4 *dst = reinterpret_cast<uint4 *>(out + (uint64_t)blockIdx.x * kFlatTile);
    for (uint32_t v = t; v < kFlatTile / 16; v += kFlatThreads) dst[v] = tile4[v];
}

// ---- BED ----

// Line j: "NAME\t{start}\t{end}\t{path name}\t{+|-}\t{rank}\n"
struct BedLine {
    uint64_t start, end;
    uint32_t rank, name_begin, name_len, handle;
    uint32_t d_start, d_end, d_rank;
};
__device__ __forceinline__ uint32_t line_handle(const FlatPaths &g, uint64_t j, BedLine *ln) {
    const uint32_t p = (uint32_t)last_at_or_before(g.pstart, 0, g.n_paths - 1, j);
    ln->rank = (uint32_t)(j - g.pstart[p]);
    ln->name_begin = g.prec[3 * p + 1], ln->name_len = g.prec[3 * p + 2];
    return ln->handle = g.steps[(uint64_t)g.prec[3 * p] + ln->rank];
}
// (the handle names a segment: flatten_bed_begin saw to that)
__device__ __forceinline__ uint64_t line_fields(const FlatPaths &g, uint32_t name_len, BedLine *ln) {
    const uint32_t seg = ln->handle >> 1;
    ln->start = g.legend[seg], ln->end = g.legend[seg + 1];
    ln->d_start = digits10(ln->start), ln->d_end = digits10(ln->end), ln->d_rank = digits10(ln->rank);
    return (uint64_t)name_len + ln->name_len + ln->d_start + ln->d_end + ln->d_rank + kBedFixed;
}

// every handle names a segment (else bit 0 of *flag), and *total += the bytes of all lines
__global__ __launch_bounds__(kFlatThreads) void k_flat_check(FlatPaths g, uint32_t name_len, uint64_t *total, uint32_t *flag) {
    uint64_t sum = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * kFlatThreads + threadIdx.x; j < g.n_lines; j += (uint64_t)gridDim.x * kFlatThreads) {
        BedLine ln;
        if ((line_handle(g, j, &ln) >> 1) >= g.n_segs) {
            atomicOr(flag, 1u);
            continue;
        }
        sum += line_fields(g, name_len, &ln);
    }
    uint64_t all = 0;
    (void)block_excl_scan<uint64_t, kFlatThreads>(sum, &all);
    if (threadIdx.x == 0 && all) atomicAdd(reinterpret_cast<unsigned long long *>(total), (unsigned long long)all);
}

// the lengths of the chunk's lines [j0, j0 + n), scanned into their offsets within the chunk
struct FlatLineLen {
    FlatPaths g;
    uint32_t name_len;
    uint64_t j0;
    uint64_t *off;
    __device__ __forceinline__ Sum<uint64_t> load(uint64_t i) const {
        BedLine ln;
        (void)line_handle(g, j0 + i, &ln);
        return Sum<uint64_t>{line_fields(g, name_len, &ln)};
    }
    __device__ __forceinline__ void store(uint64_t i, uint64_t before, const Sum<uint64_t> &) const { off[i] = before; }
};

// The tile [B0, B0 + tlen) of a chunk of n lines and `bytes` bytes; positions are kept relative to B0, so a line that began in
// an earlier tile has a negative one.
__global__ __launch_bounds__(kFlatThreads) void k_flat_bed(FlatPaths g, const uint8_t *__restrict__ name, uint32_t name_len, uint64_t j0, uint64_t n,
                                                           const uint64_t *__restrict__ off, uint64_t bytes, uint64_t tile0,
                                                           uint8_t *__restrict__ out) {
    __shared__ uint4 tile4[kFlatTile / 16];
    __shared__ LongCopy longs[kLongCap];
    __shared__ uint32_t n_long;
    uint8_t *tile = reinterpret_cast<uint8_t *>(tile4);
    const uint32_t t = threadIdx.x;
    const uint64_t B0 = (tile0 + blockIdx.x) * kFlatTile;
    const int64_t tlen = (int64_t)min((uint64_t)kFlatTile, bytes - B0);
    for (uint32_t v = t; v < kFlatTile / 16; v += kFlatThreads) tile4[v] = uint4{0, 0, 0, 0};
    if (t == 0) n_long = 0;
    __syncthreads();
    const auto put = [&](int64_t at, uint8_t ch) {
        if (at >= 0 && at < tlen) tile[at] = ch;
    };
    const auto put_num = [&](int64_t at, uint64_t x, uint32_t nd) {  // nd digits, the last at at + nd - 1
        for (int64_t d = at + nd - 1; d >= at; --d) {
            put(d, (uint8_t)('0' + x % 10));
            x /= 10;
        }
    };
    const auto put_name = [&](int64_t at, const uint8_t *src, uint32_t len) {
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
    // the lines that have a byte in the tile
    const uint64_t l0 = last_at_or_before(off, 0, n - 1, B0), l1 = last_at_or_before(off, l0, n - 1, B0 + (uint64_t)tlen - 1);
    for (uint64_t l = l0 + t; l <= l1; l += kFlatThreads) {
        BedLine ln;
        (void)line_handle(g, j0 + l, &ln);
        (void)line_fields(g, name_len, &ln);
        int64_t at = (int64_t)(off[l] - B0);
        put_name(at, name, name_len), at += name_len;
        put(at++, '\t');
        put_num(at, ln.start, ln.d_start), at += ln.d_start;
        put(at++, '\t');
        put_num(at, ln.end, ln.d_end), at += ln.d_end;
        put(at++, '\t');
        put_name(at, g.name_data + ln.name_begin, ln.name_len), at += ln.name_len;
        put(at++, '\t');
        put(at++, (ln.handle & 1u) ? '-' : '+');
        put(at++, '\t');
        put_num(at, ln.rank, ln.d_rank), at += ln.d_rank;
        put(at, '\n');
    }
    __syncthreads();
    const uint32_t nl = min(n_long, kLongCap);
    for (uint32_t e = 0; e < nl; ++e) {
        const LongCopy c = longs[e];
        for (uint32_t k = t; k < c.len; k += kFlatThreads) tile[c.dst + k] = c.src[k];
    }
    __syncthreads();
    uint4 *dst = reinterpret_cast<uint4 *>(out + (uint64_t)blockIdx.x * kFlatTile);
    for (uint32_t v = t; v < kFlatTile / 16; v += kFlatThreads) dst[v] = tile4[v];
}

}  // namespace

// ---- host side ----

int flatten_legend(const uint32_t *seg_len, uint32_t n_segs, uint64_t *offset_out, hipStream_t st) {
    if (!offset_out || (n_segs && !seg_len)) { set_error("flatten: NULL argument"); return FLATGFA_ERR_ARG; }
    DeviceMem mem;
    mem.st = st;
    Spine<Sum<uint64_t>> sp;
    FL_HIP(sp.alloc(&mem, blocks(n_segs, kFlatThreads * kFlatScanPer)));
    const LegendOp op{seg_len, offset_out};
    ProfScope prof("flatten_legend", st);
    scan_count<kFlatThreads, kFlatScanPer, Sum<uint64_t>>(op, n_segs, sp, st);
    scan_apply<kFlatThreads, kFlatScanPer, Sum<uint64_t>>(op, n_segs, sp, st);
    FL_HIP(hipGetLastError());
    FL_HIP(hipMemcpyAsync(offset_out + n_segs, sp.total, 8, hipMemcpyDeviceToDevice, st));
    FL_HIP(hipStreamSynchronize(st));
    return FLATGFA_OK;
}

struct FlatJob : PieceBufs {  // (the streams, the events and the two piece buffers: text_tiles.hpp)
    uint64_t chunk_lines = kFlatChunkLines;
    uint64_t chunks = 0;
    uint64_t *off = nullptr;                   // u64[chunk_lines]: line offsets within the chunk
    uint64_t *total = nullptr;                 // the check's byte count, then its flag word
    uint8_t *name = nullptr;
    size_t name_len = 0;
    Spine<Sum<uint64_t>> sp;
    FlatPaths g;
    bool begun = false;
    DeviceMem mem;
};

FlatJob *flatten_new(uint64_t chunk_lines) {
    FlatJob *j = new FlatJob();
    j->chunk_lines = std::max<uint64_t>(chunk_lines, 1);
    return j;
}

void flatten_free(FlatJob *j) {
    if (!j) return;
    pieces_free(j);
    delete j;  // (the device memory goes with mem)
}

uint64_t flatten_chunks(const FlatJob *j) { return j->chunks; }

uint64_t flatten_fasta_bytes(uint64_t total_bases, size_t name_len) {
    const uint64_t body = total_bases ? total_bases + (total_bases + kFlatWrap - 1) / kFlatWrap : 1;
    return 2 + (uint64_t)name_len + body;
}

int flatten_fasta(FlatJob *j, const FlatSeqs &g, const uint8_t *name, size_t name_len, hipStream_t st, FlatSink sink, void *ctx) {
    if (!j || !sink || (name_len && !name)) { set_error("flatten: NULL argument"); return FLATGFA_ERR_ARG; }
    if (int rc = pieces_ready(j, &j->mem, st, "flatten: ")) return rc;
    Pipe pipe(j, sink, ctx, "flatten: ");
    if (!pipe.pin) { set_error("flatten: no pinned staging buffer"); return FLATGFA_ERR_HIP; }
    std::string head = ">";
    head.append((const char *)name, name_len).push_back('\n');
    if (int rc = pipe.give(head.data(), head.size())) return rc;
    const uint64_t body = flatten_fasta_bytes(g.total, name_len) - head.size();
    if (int rc = pipe.tiles(body, [&](uint8_t *out, uint64_t tile0, uint32_t nt) {
            ProfScope prof("flatten_fasta", st);
            hipLaunchKernelGGL(k_flat_fasta, dim3(nt), dim3(kFlatThreads), 0, st, g, body, tile0, out);
        }))
        return rc;
    return pipe.finish();
}

int flatten_bed_begin(FlatJob *j, const FlatPaths &g, const uint8_t *name, size_t name_len, hipStream_t st, uint64_t *bytes) {
    if (!j || !bytes || (name_len && !name)) { set_error("flatten: NULL argument"); return FLATGFA_ERR_ARG; }
    if (name_len > 0xFFFFFFFFull) { set_error("flatten: the name is longer than 2^32 - 1 bytes"); return FLATGFA_ERR_TOO_LARGE; }
    j->begun = false;
    if (int rc = pieces_ready(j, &j->mem, st, "flatten: ")) return rc;
    if (!j->total) {
        FL_HIP(j->mem.alloc(&j->total, 2));
        FL_HIP(j->mem.alloc(&j->off, j->chunk_lines));
        FL_HIP(j->sp.alloc(&j->mem, blocks(j->chunk_lines, kFlatThreads * kFlatScanPer)));
    }
    FL_HIP(j->mem.alloc(&j->name, name_len));  // (a job serves few calls: the names before this one go with the job)
    if (name_len) FL_HIP(staged_copy(j->name, name, name_len, hipMemcpyHostToDevice, st));
    j->name_len = name_len;
    j->g = g;
    uint64_t got[2] = {0, 0};
    if (g.n_lines) {
        FL_HIP(hipMemsetAsync(j->total, 0, 16, st));
        const uint32_t grid = stride_blocks(g.n_lines, kFlatThreads * 8, 1u << 16);
        {
            ProfScope prof("flatten_check", st);
            hipLaunchKernelGGL(k_flat_check, dim3(grid), dim3(kFlatThreads), 0, st, g, (uint32_t)name_len, j->total,
                               reinterpret_cast<uint32_t *>(j->total + 1));
        }
        FL_HIP(hipGetLastError());
        FL_HIP(hipMemcpyAsync(got, j->total, 16, hipMemcpyDeviceToHost, st));
        FL_HIP(hipStreamSynchronize(st));
    }
    if (got[1]) {
        set_error("flatten: a step refers to a segment id that is out of range");
        return FLATGFA_ERR_BOUNDS;
    }
    *bytes = sizeof kBedHeader - 1 + got[0];
    j->begun = true;
    return FLATGFA_OK;
}

int flatten_bed_emit(FlatJob *j, FlatSink sink, void *ctx) {
    if (!j || !sink) { set_error("flatten: NULL argument"); return FLATGFA_ERR_ARG; }
    if (!j->begun) { set_error("flatten: emit before a successful begin"); return FLATGFA_ERR_ARG; }
    j->chunks = 0;
    Pipe pipe(j, sink, ctx, "flatten: ");
    if (!pipe.pin) { set_error("flatten: no pinned staging buffer"); return FLATGFA_ERR_HIP; }
    if (int rc = pipe.give(kBedHeader, sizeof kBedHeader - 1)) return rc;
    const FlatPaths &g = j->g;
    const hipStream_t st = j->st;
    const uint32_t name_len = (uint32_t)j->name_len;
    for (uint64_t j0 = 0; j0 < g.n_lines; j0 += j->chunk_lines, ++j->chunks) {
        const uint64_t n = std::min<uint64_t>(j->chunk_lines, g.n_lines - j0);
        const FlatLineLen op{g, name_len, j0, j->off};
        {
            ProfScope prof("flatten_line_scan", st);
            scan_count<kFlatThreads, kFlatScanPer, Sum<uint64_t>>(op, n, j->sp, st);
            scan_apply<kFlatThreads, kFlatScanPer, Sum<uint64_t>>(op, n, j->sp, st);
        }
        FL_HIP(hipGetLastError());
        uint64_t bytes = 0;  // (behind the pieces of the chunk before: the offsets are theirs until they are formatted)
        FL_HIP(hipMemcpyAsync(&bytes, j->sp.total, 8, hipMemcpyDeviceToHost, st));
        FL_HIP(hipStreamSynchronize(st));
        if (int rc = pipe.tiles(bytes, [&](uint8_t *out, uint64_t tile0, uint32_t nt) {
                ProfScope prof("flatten_bed", st);
                hipLaunchKernelGGL(k_flat_bed, dim3(nt), dim3(kFlatThreads), 0, st, g, j->name, name_len, j0, n, j->off, bytes, tile0, out);
            }))
            return rc;
    }
    return pipe.finish();
}

}  // namespace fgfa_dev

// ---- the device-level entry (include/flatgfa.h, Part 3) ----
extern "C" int flatgfa_dev_flatten_legend(const flatgfa_dev_graph_t *g, uint64_t *d_offset_out, void *stream) {
    if (!g || !d_offset_out) { fgfa_dev::set_error("flatgfa_dev_flatten_legend: NULL argument"); return FLATGFA_ERR_ARG; }
    if (!g->seg_len) { fgfa_dev::set_error("flatgfa_dev_flatten_legend: the graph has no seg_len"); return FLATGFA_ERR_ARG; }
    return fgfa_dev::flatten_legend(g->seg_len, g->n_segs, d_offset_out, (hipStream_t)stream);
}
