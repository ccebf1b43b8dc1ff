// The packed-sequence codec on the device (seq_device.hip): nucleotide text to two bases a byte and back
// (flatgfa/src/packedseq.rs, `fgfa seq-export` / `seq-import`), as the C ABI (capi.cpp, and the flatgfa_dev_seq_* entries)
// drives it.  DESIGN.md section 18.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace fgfa_dev {

// The text is walked a tile of kSeqTile bytes at a time by one workgroup of kSeqThreads lanes, in the coordinates of the
// 16-byte vectors the text lies in (a text that does not begin on a 16-byte boundary begins inside its first tile); the tiles
// are dealt to at most kSeqGrid workgroups in equal contiguous ranges, so that the scratch does not depend on the text.
constexpr int kSeqThreads = 256;
constexpr uint32_t kSeqTile = 16384;
constexpr uint32_t kSeqGrid = 1024;
// The three-launch scan (device_scan.hpp) of the ranges' kept counts.
constexpr uint32_t kSeqScanPer = 4;
// Unpack: 16 packed bytes (32 bases) a lane and step, a grid-stride walk of at most kSeqUnpackGrid workgroups.
constexpr uint32_t kSeqUnpackGrid = 4096;
// A text byte's offset travels with the byte in one 64-bit word (the min-reduction of the first byte that is no nucleotide).
constexpr uint64_t kSeqMaxText = 1ull << 56;

constexpr int kSeqNoCarry = -1;

// One pack.  count() classifies every byte of text[0, n) -- whitespace (Rust's u8::is_ascii_whitespace) is dropped, A C T G
// are kept, anything else is an error -- counts what every range of tiles keeps, notes every range's first kept base, scans
// the counts and waits for the total and the smallest offending offset: its one host synchronization.  A bad byte:
// FLATGFA_ERR_PARSE, flatgfa_last_error names the byte and base_offset + its offset.  fill() enqueues the packed bytes of the
// logical stream "carry (a code 0..3, or kSeqNoCarry), then the kept bases" into out, u8[seq_packed_bytes(*n_bases + carry)]
// at any alignment: base 2k in the low nibble of byte k, base 2k + 1 in the high one, the unused last high nibble 0.  Every
// byte is written once, by one workgroup, with both nibbles final; fill does not wait.  All device memory of the current device.
struct SeqPackJob;
SeqPackJob *seq_pack_new();
void seq_pack_free(SeqPackJob *j);
int seq_pack_count(SeqPackJob *j, const uint8_t *text, uint64_t n, uint64_t base_offset, hipStream_t stream, uint64_t *n_bases);
int seq_pack_fill(SeqPackJob *j, int carry, uint8_t *out, hipStream_t stream);
inline uint64_t seq_packed_bytes(uint64_t n_bases) { return n_bases / 2 + (n_bases & 1); }

// text_out[i] = "ACTG"[nibble i of packed] for i < n_bases; the unused high nibble of an odd sequence's last byte is not
// looked at.  Waits for the stream once, for the smallest base index whose nibble is above 3: FLATGFA_ERR_PARSE then, and
// flatgfa_last_error names base_offset + that index (text_out holds no answer).  Both pointers at any alignment; the 16-byte
// loads and stores are taken where both are 16-byte aligned.
int seq_unpack(const uint8_t *packed, uint64_t n_bases, uint64_t base_offset, uint8_t *text_out, hipStream_t stream);

}  // namespace fgfa_dev
