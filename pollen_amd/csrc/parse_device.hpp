// The GFA parser on the device (parse_device.hip): the pools of Parser::parse_mem / parse_stream (flatgfa/src/parse.rs:77-126,
// 24-74) from GFA text of the plain grammar, as the C ABI (capi.cpp) drives it.  DESIGN.md section 20.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "flatgfa_core.hpp"

namespace fgfa_dev {

// The step kernels work by tile of text bytes: 256 lanes of 16 bytes.
constexpr int kParseThreads = 256;
constexpr uint32_t kParseLaneBytes = 16;
constexpr uint32_t kParseTile = kParseThreads * kParseLaneBytes;
// The digits of one number -- a segment name, a CIGAR length -- the kernels read: a longer run is not theirs to judge.
constexpr uint32_t kParseWindow = 32;
// the elements of one tile of the scans the parser runs (device_scan.hpp's k_scan)
constexpr uint32_t kParseScanPer = 4;
constexpr uint32_t kParseScanTile = kParseThreads * kParseScanPer;

// Why a text is not the device's to parse.  Grammar: a line that is not of the plain forms.  Name: a link or a step names
// no segment, name 0, or a segment id >= 2^31.  Limit: a number of more than kParseWindow digits, or a pool past the item limit.
enum ParseReason : int { kParsePlain = 0, kParseGrammar = 1, kParseName = 2, kParseLimit = 3 };

struct ParseInfo {
    int device_route = 0;  // 1: `out` holds the pools; 0: the text is the host parser's, for `reason`
    int reason = kParsePlain;
    uint64_t tile_bytes = kParseTile, tiles = 0;
    // milliseconds of the call: the text's upload, everything between upload and download (the kernels, the scans' totals
    // read back, the name map made on the host), the pools' download; and by HIP events every kernel and scan of the call,
    // and of those the two step kernels alone
    double upload_ms = 0, device_ms = 0, download_ms = 0, kernel_ms = 0, step_ms = 0;
};

// The pools of text[0, n) into *out, on `stream` of the current device; waits for it.  stream_mode: parse_stream's rules (an
// unterminated last line counts, links come before paths in the alignment pool).  item_limit: what no pool may pass
// (2^32 - 1).  FLATGFA_OK with info->device_route = 0 where the text is not plain: *out is then unspecified.  Anything else
// is an error of the device (an allocation that failed among them), with the thread's message set.
int parse_device(const uint8_t *text, size_t n, bool stream_mode, uint64_t item_limit, hipStream_t stream, fgfa::Store *out,
                 ParseInfo *info);

}  // namespace fgfa_dev
