// The GFA printer on the device (print_device.hip): the text of flatgfa/src/print.rs:99-153, in either order, as the C ABI
// (capi.cpp) drives it.  DESIGN.md section 19.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "flatten_device.hpp"

namespace fgfa_dev {

// The text is cut into items -- an H, S or L line is one, a P line of n steps is n -- and the items' lengths are scanned a
// chunk at a time: the scratch (8 bytes an item) is sized by this and never by the step count.  Tiles and pieces are
// flatten's (kFlatTile, kFlatPieceBytes).
constexpr uint64_t kPrintChunkItems = (uint64_t)1 << 20;

// A segment as the segs pool holds it (flatgfa.rs:71-82); the device copy of the pool starts on an 8-byte boundary.
struct PrintSeg {
    uint64_t name;
    uint32_t seq0, seq1, opt0, opt1;
};

// What the printer reads, all device memory: the pools as the container holds them.  The lines in print order: with
// line_order, line k is of kind line_order[k] and the next of its kind (print.rs:99-131); without, the header if there is
// one, then seg_lines segments, path_lines paths, link_lines links (print.rs:134-150).  The host has seen to it that every
// line exists, that every path printed has a step, that every span read lies in its pool and that every link names two
// segments; the steps' handles are print_begin's to check.
struct PrintGraph {
    const uint8_t *header = nullptr;
    uint32_t header_len = 0;
    const PrintSeg *segs = nullptr;
    uint32_t n_segs = 0;
    const uint32_t *paths = nullptr;  // u32[6 * paths]: the name, steps and overlaps spans
    const uint32_t *links = nullptr;  // u32[4 * links]: from, to, the overlap's span
    const uint32_t *steps = nullptr;
    const uint32_t *overlaps = nullptr;   // u32[2 * n]: spans into alignment
    const uint32_t *alignment = nullptr;  // length << 8 | opcode
    const uint8_t *seq_data = nullptr, *name_data = nullptr, *optional_data = nullptr;
    const uint8_t *line_order = nullptr;  // null: normalized order
    uint64_t n_lines = 0;
    uint64_t header_lines = 0, seg_lines = 0, path_lines = 0, link_lines = 0;  // how many of each kind are printed
};

struct PrintJob;
// (chunk_items is for the tests and the measurement: it changes where the chunks are cut, never a byte of the text)
PrintJob *print_new(uint64_t chunk_items = kPrintChunkItems);
void print_free(PrintJob *j);

// The text in two calls.  print_begin numbers the lines within their kinds (a preserved order only), scans the lines' item
// counts, reads every step's handle -- one that names a segment >= n_segs: FLATGFA_ERR_BOUNDS -- and adds up the text's
// bytes; it waits for `stream`.  print_emit delivers the text: per chunk of items a scan of their lengths, then tile by tile
// the bytes, each piece copied out while the next is formatted.  A sink that returns nonzero: FLATGFA_ERR_IO, nothing more
// delivered.  g's arrays stay as they are in between.
int print_begin(PrintJob *j, const PrintGraph &g, hipStream_t stream, uint64_t *bytes);
int print_emit(PrintJob *j, FlatSink sink, void *ctx);
// how many chunks the last print_emit ran
uint64_t print_chunks(const PrintJob *j);

}  // namespace fgfa_dev
