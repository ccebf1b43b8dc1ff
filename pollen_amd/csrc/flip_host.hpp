// The host's stages of flatgfa_flip (capi.cpp), as pure functions over the pools: how the paths are laid
// one behind another for the device, what the pools must satisfy before anything is uploaded, the names of the turned paths,
// and the assembly of the new store from what the device hands back.  No HIP: tests/host_check/flip_host_check.cpp drives
// them under the sanitizers.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "flatgfa_core.hpp"

namespace fgfa_flip {

constexpr char kSuffix[] = "_inv";  // flip.py:27
constexpr uint32_t kZeroM = 0;      // flip.py:56: one alignment op, length 0 (above the low byte), match (opcode 0)

enum class Verdict { kOk, kBounds, kTooLarge };

// The paths' steps numbered one behind another, whatever their spans do in the pool: path p is [pstart[p], pstart[p + 1]) of
// that order and begins at pbegin[p] of the pool (pbegin has one spare entry, so that it is never empty).
struct Lay {
    std::vector<uint32_t> pstart, pbegin;
    uint64_t n_lin = 0;
};

// What flip reads on the host or lets a kernel index by: the pools' sizes against the 32-bit ids, every path's step span and
// name span, every segment's sequence span.  (Step and link ids and the links' overlap spans are the kernels' to check.)
inline Verdict check_and_lay(const fgfa::View &v, Lay *lay, std::string *why) {
    const size_t P = v.paths.len, N = v.steps.len, S = v.segs.len;
    if (N > 0xFFFFFFFFull || P > 0xFFFFFFFEull || S > 0x7FFFFFFFull || v.links.len > 0xFFFFFFFFull || v.alignment.len > 0xFFFFFFFEull) {
        *why = "graph too large for 32-bit ids";
        return Verdict::kTooLarge;
    }
    for (size_t s = 0; s < S; ++s) {
        const fgfa::Span sp = v.segs[s].seq;
        if (sp.start > sp.end || sp.end > v.seq_data.len) {
            *why = "segment " + std::to_string(s) + " has a sequence span outside seq_data";
            return Verdict::kBounds;
        }
    }
    lay->pstart.assign(P + 1, 0);
    lay->pbegin.assign(P + 1, 0);
    lay->n_lin = 0;
    for (size_t p = 0; p < P; ++p) {
        const fgfa::Span sp = v.paths[p].steps, nm = v.paths[p].name;
        if (sp.start > sp.end || sp.end > N) {
            *why = "path " + std::to_string(p) + " has a step span outside the steps pool";
            return Verdict::kBounds;
        }
        if (nm.start > nm.end || nm.end > v.name_data.len) {
            *why = "path " + std::to_string(p) + " has a name span outside name_data";
            return Verdict::kBounds;
        }
        lay->pbegin[p] = sp.start;
        lay->n_lin += sp.len();
        if (lay->n_lin > 0xFFFFFFFFull) {
            *why = "the paths hold more than 2^32 - 1 steps";
            return Verdict::kTooLarge;
        }
        lay->pstart[p + 1] = (uint32_t)lay->n_lin;
    }
    return Verdict::kOk;
}

// the bytes of the new name pool: every path's name, the turned ones' with the suffix
inline uint64_t names_bytes(const fgfa::View &v, const uint32_t *turned) {
    uint64_t n = 0;
    for (size_t p = 0; p < v.paths.len; ++p) n += (uint64_t)v.paths[p].name.len() + (turned[p] ? sizeof kSuffix - 1 : 0);
    return n;
}

// The new name pool and the spans into it: the names one behind another in path order (names_bytes of them, which fit a span).
inline void rebuild_names(const fgfa::View &v, const uint32_t *turned, std::vector<uint8_t> *name_data, std::vector<fgfa::Span> *spans) {
    name_data->clear();
    name_data->reserve((size_t)names_bytes(v, turned));
    spans->resize(v.paths.len);
    for (size_t p = 0; p < v.paths.len; ++p) {
        const fgfa::Span nm = v.paths[p].name;
        const uint32_t at = (uint32_t)name_data->size();
        name_data->insert(name_data->end(), v.name_data.data + nm.start, v.name_data.data + nm.end);
        if (turned[p]) name_data->insert(name_data->end(), kSuffix, kSuffix + sizeof kSuffix - 1);
        (*spans)[p] = fgfa::Span{at, (uint32_t)name_data->size()};
    }
}

// The new store.  `steps` are the new steps (lay.n_lin of them, the paths one behind another), `links` the kept records; the
// new ones among them (any_new: there are some) point at op v.alignment.len, which is appended here.
inline void assemble(const fgfa::View &v, const Lay &lay, const uint32_t *turned, std::vector<fgfa::Handle> &&steps, std::vector<fgfa::Link> &&links,
                     bool any_new, fgfa::Store *h) {
    h->header.assign(v.header.begin(), v.header.end());
    h->seq_data.assign(v.seq_data.begin(), v.seq_data.end());
    h->segs.resize(v.segs.len);
    for (size_t s = 0; s < v.segs.len; ++s) h->segs[s] = fgfa::Segment{v.segs[s].name, v.segs[s].seq, fgfa::Span{0, 0}};
    h->steps = std::move(steps);
    h->links = std::move(links);
    h->alignment.resize(v.alignment.len + (any_new ? 1 : 0));
    if (v.alignment.len) memcpy(h->alignment.data(), v.alignment.data, v.alignment.len * 4);
    if (any_new) h->alignment[v.alignment.len] = kZeroM;
    std::vector<fgfa::Span> names;
    rebuild_names(v, turned, &h->name_data, &names);
    h->paths.resize(v.paths.len);
    for (size_t p = 0; p < v.paths.len; ++p) h->paths[p] = fgfa::Path{names[p], fgfa::Span{lay.pstart[p], lay.pstart[p + 1]}, fgfa::Span{0, 0}};  // flip.py:27, 29
    h->overlaps.clear();
    h->optional_data.clear();
    h->line_order.clear();
}

}  // namespace fgfa_flip
