// Flatten on the device (flatten_device.hip): the graph in linear coordinates, as slow_odgi/slow_odgi/flatten.py prints it -- a
// FASTA record of every segment's bases and a BED line per path step -- as the C ABI (capi.cpp) drives it.  DESIGN.md section 15.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace fgfa_dev {

// Both texts are written by output tile: one workgroup of kFlatThreads lanes owns kFlatTile consecutive output bytes, forms
// them in LDS and stores them with 16-byte vector stores.  A piece is what one launch writes and one copy takes to the host:
// half a staging buffer (host_copy.hpp), so that one half travels while the host hands the other to the sink.
constexpr int kFlatThreads = 256;
constexpr uint32_t kFlatTile = 16384;
constexpr uint64_t kFlatPieceBytes = (uint64_t)4 << 20;
// The three-launch scans (device_scan.hpp) of the legend and of the line lengths: kFlatThreads * kFlatScanPer elements a tile.
constexpr uint32_t kFlatScanPer = 4;
// BED lines are laid out a chunk at a time: the scratch (8 bytes a line) is sized by this and never by the step count.
constexpr uint64_t kFlatChunkLines = (uint64_t)1 << 20;
// A name longer than this inside one tile is copied by the whole workgroup, a shorter one by the line's own lane.
constexpr uint32_t kFlatLongName = 64;
// FASTA lines hold this many bases (flatten.py:44-46).
constexpr uint32_t kFlatWrap = 80;

// The legend (flatten.py:13-19): offset_out[s] = the bases of the segments before s, offset_out[n_segs] = all of them.
// seg_len u32[n_segs] and offset_out u64[n_segs + 1] are device memory.  Enqueues on `stream` and waits for it (the scan's
// scratch goes before the call returns).
int flatten_legend(const uint32_t *seg_len, uint32_t n_segs, uint64_t *offset_out, hipStream_t stream);

// What the FASTA reads, all device memory: the legend, Segment.seq.start and Segment::len() per segment (two words each, as
// the GAF lookup keeps them) and seq_data.  Every span lies inside seq_data (the host checks that).  Never the steps.
struct FlatSeqs {
    const uint64_t *legend = nullptr;   // u64[n_segs + 1]
    const uint32_t *seg_seq = nullptr;  // u32[2 * n_segs]
    const uint8_t *seq_data = nullptr;
    uint32_t n_segs = 0;
    uint64_t total = 0;  // legend[n_segs]
};

// What the BED reads, all device memory: the legend, the steps, and per path where its steps begin and where its name lies
// in name_data.  Line j of the paths laid one behind another belongs to the last path p with pstart[p] <= j and is its step
// j - pstart[p]; the spans may overlap, alias or be empty.  Never seq_data.
struct FlatPaths {
    const uint64_t *legend = nullptr;  // u64[n_segs + 1]
    uint32_t n_segs = 0;
    const uint32_t *steps = nullptr;
    const uint64_t *pstart = nullptr;  // u64[n_paths + 1]
    const uint32_t *prec = nullptr;    // u32[3 * n_paths]: first step, first name byte, name length
    const uint8_t *name_data = nullptr;
    uint32_t n_paths = 0;
    uint64_t n_lines = 0;  // pstart[n_paths]
};

// Receives the text in order, a piece at a time; nonzero stops the call (flatgfa_sink_t).
using FlatSink = int (*)(void *ctx, const char *bytes, size_t n);

struct FlatJob;
// (chunk_lines is for the tests and the measurement: it changes where the chunks are cut, never a byte of the text)
FlatJob *flatten_new(uint64_t chunk_lines = kFlatChunkLines);
void flatten_free(FlatJob *j);

// The bytes of the FASTA record for a name of name_len bytes: ">" name "\n", the bases, a newline after every kFlatWrap of
// them and one at the end (flatten.py:51-55).
uint64_t flatten_fasta_bytes(uint64_t total_bases, size_t name_len);
// The record, to the sink.  Enqueues on `stream`, copies on a stream of the job's and waits for both.  A sink that
// returns nonzero: FLATGFA_ERR_IO, nothing more delivered.
int flatten_fasta(FlatJob *j, const FlatSeqs &g, const uint8_t *name, size_t name_len, hipStream_t stream, FlatSink sink, void *ctx);

// The BED table (flatten.py:23-41) in two calls.  flatten_bed_begin takes `name` (host memory) to the device, reads every
// line's handle -- one that names a segment >= n_segs: FLATGFA_ERR_BOUNDS -- and adds up the table's bytes, header line
// included; it waits for `stream`.  flatten_bed_emit delivers the table: per chunk of lines a scan of their lengths, then
// tile by tile the text, each piece copied out while the next is formatted.  g's arrays stay as they are in between.
int flatten_bed_begin(FlatJob *j, const FlatPaths &g, const uint8_t *name, size_t name_len, hipStream_t stream, uint64_t *bytes);
int flatten_bed_emit(FlatJob *j, FlatSink sink, void *ctx);
// how many chunks the last flatten_bed_emit ran
uint64_t flatten_chunks(const FlatJob *j);

}  // namespace fgfa_dev
