// The host's decisions about one call of a bucketed node-depth plan (depth_fast.hip: run_range) and about the status word
// behind it (depth_device.hip: flatgfa_dev_status), as functions over plain data: which launches a call is made of, how
// large, who zeroes what, which build of k_scan runs, and what a status word asks for.  No HIP runtime call and no
// environment variable in here: run_range reads the hooks once and hands them in, and tests/host_check/call_check.cpp
// runs these functions over every combination of the facts they read, without a GPU.
#pragma once
#include <algorithm>
#include <cstdint>

#include "depth_fast.hpp"

namespace fgfa_dev {

// The test and measurement hooks of a call, read once at its top (per call, not per plan: tests set them between calls).
struct CallHooks {
    bool scan_always = false;         // FLATGFA_SCAN_ALWAYS: k_scan is launched even where it has nothing to do
    const char *scan_time = nullptr;  // FLATGFA_SCAN_TIME[=<file>]: when k_scan's workgroups start, run dry and end
    bool no_plain = false;            // FLATGFA_NO_PLAIN (measurements): pass 2 is not told how many items each workgroup took
    bool acc_time = false;            // FLATGFA_ACC_TIME: where the waves of pass 2 spend their time (calls with unique depth)
    const char *acc_skip = nullptr;   // FLATGFA_ACC_SKIP=<mask> (measurement builds): pass 2 without parts of its work
};
struct CallWants {
    bool uniq = false;                     // unique depth beside depth
    bool psum = false, psum_clear = false;  // path sums ride on the call (PathSums), and the call zeroes them first
    bool count_only = false;               // the counting call of a packed plan: pass 1 alone
};
struct GraphFacts {
    uint32_t n_segs;
    bool has_seg_len;
};
enum class Zeroes { nobody, k_scan, memset };  // who clears a vector the call adds to: k_scan as its first act, or memsets where it does not run
struct CallShape {
    const char *refusal = nullptr;  // FLATGFA_ERR_ARG with this message; nothing is enqueued
    bool has_pre = false;           // there are wave-per-path lists
    bool scan_skip = false;         // ... and k_scan has no items of its own and nothing can come back: its launch is left out
    uint32_t grid = 0;              // k_scan's (or k_scan_runs'): one persistent workgroup per sub-bucket; 0 = no launch
    uint32_t grid_tiny = 0, grid_short = 0, grid_medium = 0;  // the wave-per-path kernels'; 0 = the list is empty
    bool tagged = false, ranged = false, big = false, cflags = false;
    bool from_image = false;  // pass 1 reads the steps' run-length image (k_scan_runs)
    bool kept = false;        // ... whose records of the call before are still there: pass 1 is left out
    bool sorted = false;      // ... and pass 2 sweeps the plan's sorted record image (k_accum_sorted) instead of walking the kept records
    uint32_t sorted_solo_lds = 0;  // ... launched with this much dynamic LDS: one sweep workgroup to a CU (a pipeline lane); 0: two share it
    uint32_t has_pre2 = 0;    // pass 2: 0 = all records are k_scan's, 1 = the wave-per-path kernels' lie before them, 2 = there are no others
    uint32_t max_back = 0;    // paths that may be handed back to k_scan, as both passes see it
    Zeroes outputs = Zeroes::nobody, sums = Zeroes::nobody;
    bool scans() const { return grid && !kept; }  // pass 1 for the items: a launch of k_scan, k_scan_dense or k_scan_runs
};

// ---- which build of k_scan a call runs ----
constexpr int kModeDense = -1, kModeRefused = -2;  // (beside depth_fast.hpp's kMode*: k_scan_dense; no build takes such a call)
struct ScanMode {
    int mode;
    bool tagged;
};
inline ScanMode scan_mode(const FastPlan &fp, const CallShape &s) {
    if (fp.dense) return {kModeDense, false};
#ifdef FGFA_MEASURE
    if (fp.dbg) return {kModeDbg, false};
#endif
    const bool flags = s.cflags && s.tagged && !s.ranged;
    if (flags && fp.packed) return {kModePackedFlags, true};  // (a packed call's offsets are its region's: `big` is not its business)
    if (flags && !s.big) return {kModePlainFlags, true};
    if (fp.packed) return {s.ranged ? kModePackedRanged : kModePacked, true};
    if (s.big && !s.tagged) return {kModeRefused, false};
    if (s.big) return {s.ranged ? kModeRangedBig : kModeBig, true};
    if (s.ranged) return {kModeRanged, s.tagged};
    return {s.tagged && fp.narrow_emit ? kModePlainNarrow : kModePlain, s.tagged};
}

// ---- pipeline lanes: one sweep workgroup to a CU ----
// Two sweeps queued by two lanes start side by side on the same CUs, share the LDS pipe that bounds both and reach their clears
// and epilogues together; launched with enough dynamic LDS that static plus dynamic exceeds half a CU's, the lanes' sweeps
// follow each other on every CU instead.  hook: FLATGFA_SORTED_SOLO as it was when the image was installed (0, 1; -1: unset);
// lanes: the calls in flight of the pipeline that made the plan (0: a plan on its own, which keeps two workgroups to a CU).
constexpr bool kSortedLanesSoloDefault = false;  // (profiles/NOTES.md R7.6: which setting measured faster)
inline bool sorted_lanes_solo(int hook, uint32_t lanes) { return hook >= 0 ? hook == 1 : kSortedLanesSoloDefault && lanes >= 2u; }
inline uint32_t sorted_solo_lds(int hook, uint32_t lanes, uint32_t cu_lds_bytes) { return sorted_lanes_solo(hook, lanes) ? cu_lds_bytes / 2u : 0u; }

// ---- the shape of a call ----
inline uint32_t wave_list_grid(uint32_t n, uint32_t per_wg, uint32_t n_slots) { return std::min<uint32_t>((n + per_wg - 1) / per_wg, n_slots); }

inline CallShape decide_call(const FastPlan &fp, const GraphFacts &g, const CallWants &w, const CallHooks &hooks, bool records_use) {
    CallShape s;
    if (w.psum && (w.uniq || fp.wb != 12 || !g.has_seg_len || !fp.psum_part || fp.n_range != g.n_segs)) {
        s.refusal = "fast_seg_depth: path sums ride on seg_depth with 4096-segment windows only";
        return s;
    }
    // Tagged: k_scan's records name their items, pass 2 walks whole sub-buckets.  Path sums ride on
    // the directory walk (an item's records have to be found again once the window's depth is final).
    const bool tagged = fp.tagged && !w.psum;
    if (fp.packed && !tagged) {
        s.refusal = "fast_seg_depth: a plan with packed buckets runs tagged calls only";
        return s;
    }
    s.tagged = tagged;
    s.has_pre = fp.n_short || fp.n_medium || fp.n_tiny;
    // one persistent workgroup per CU; k_scan may be handed short paths back, so it gets a full grid when there are any
    // (and whenever the wave-per-path kernels ran: it saves their cursors for pass 2)
    // -- unless it has no items of its own and nothing can come back (the run counts of the lists are
    // exact): then the launch is left out, every record is one of the wave-per-path kernels', and a
    // path that does not fit after all (steps changed behind the plan) raises kStBackOverflow.
    s.scan_skip = s.has_pre && fp.n_items == 0 && fp.exact_short && !fp.dbg && !hooks.scan_always;
    s.grid = s.scan_skip ? 0u : s.has_pre ? fp.n_slots : std::min<uint32_t>(fp.n_items, fp.n_slots);
    s.has_pre2 = s.scan_skip ? 2u : s.has_pre ? 1u : 0u;
    s.max_back = s.scan_skip ? 0u : fp.max_back;
    s.ranged = fp.seg_base != 0 || fp.n_range != g.n_segs;
    const uint32_t stride = fp.n_slots * fp.cap;
    s.big = ((uint64_t)fp.n_win + 1) * stride >= (1ull << 30);
    s.cflags = tagged && fp.cflags;
    // (a tagged call of a plan with the steps' run-length image installed reads that: no plan that is given one has dense
    // pass 1, packed buckets, ranges, marks or wave-per-path lists)
    s.from_image = s.grid && tagged && fp.run_ent && fp.run_item_ent && !w.count_only && !fp.dense && !fp.packed && !s.ranged && !s.cflags && !s.has_pre && !fp.dbg;
    // ... and where the records of the image call before this one are still in the scratch (RecordsUse: the handle knows), it
    // would write the same records into the same slots: pass 1 is left out, pass 2 reads the kept cursors and leaves them.
    s.kept = s.from_image && records_use && fp.counts_kept;
    // ... and exactly those calls, once the plan's sorted record image is installed (one pass-2 workgroup per window, the window
    // widths it has builds for), sweep that.  Pass 1 runs wherever it ran: whatever drops the kept records brings it back.
    s.sorted = s.kept && fp.sorted_rec && fp.sorted_carry && fp.sorted_win_chunk && fp.acc_parts == 1 && fp.wb >= 11 && fp.wb <= 13;
    s.sorted_solo_lds = s.sorted ? fp.sorted_solo_lds : 0u;
    if (s.scans() && !s.from_image && scan_mode(fp, s).mode == kModeRefused) {
        CallShape no;
        no.refusal = "fast_seg_depth: a bucket array this large needs a tagged call";
        return no;
    }
    if (fp.n_tiny) s.grid_tiny = wave_list_grid(fp.n_tiny, kWaves, fp.n_slots);  // paths a wave holds whole (at most 128 steps)
    if (fp.n_short) s.grid_short = wave_list_grid(fp.n_short, kShortWaves, fp.n_slots);
    if (fp.n_medium) s.grid_medium = wave_list_grid(fp.n_medium, kMediumPaired ? kMediumWaves / 2 : kMediumWaves, fp.n_slots);  // (paths a workgroup walks at a time)
    // What pass 2 (several workgroups per window) and k_path_reduce add to starts at zero: k_scan's first act, or memsets
    // where it does not run.  (A later group of paths adds to what is there.)
    const Zeroes who = s.scans() ? Zeroes::k_scan : Zeroes::memset;
    if (fp.acc_parts > 1 && !fp.accumulate && !w.count_only) s.outputs = who;
    if (w.psum && w.psum_clear) s.sums = s.grid ? Zeroes::k_scan : Zeroes::memset;
    return s;
}

// ---- what a status word asks for (flatgfa_dev_status keeps the copies, the memsets, the messages and the loop) ----
enum class StatusVerdict {
    fine,            // nothing (left) to do
    bounds, stale, internal, several_calls,  // the four errors
    redo_grown,      // the last call again, with four times the room (through the atomic kernels if the plan cannot grow)
    redo_atomic,     // ... through the atomic kernels right away, which later calls take too (a full hand-back list)
    unresolved,      // there is no last call to run again, or it has been tried too often
};
struct StatusAction {
    StatusVerdict verdict;
    bool grow_ahead;  // first: a sub-bucket was more than half full and nothing overflowed -- make room ahead of need (an eligible plan)
};
// st3: the flags; -; the fullest sub-bucket beyond half of the capacity.  `attempt`: how often the loop has come round.
inline StatusAction status_verdict(const uint32_t st3[3], uint32_t calls, int attempt, bool last_fast, bool has_last_call) {
    const uint32_t st = st3[0], over = kStOverflow | kStBackOverflow;
    StatusAction a{StatusVerdict::fine, st3[2] != 0 && !(st & over)};
    if (st & kStBounds) a.verdict = StatusVerdict::bounds;
    else if (st & kStStale) a.verdict = StatusVerdict::stale;
    else if (st & kStInternal) a.verdict = StatusVerdict::internal;
    else if (!(st & over)) a.verdict = StatusVerdict::fine;
    // Several calls were enqueued since the last status and (at least) one of them ran out of
    // scratch room: which one is not recorded, and only the last one's outputs are known here.
    else if (attempt == 0 && calls > 1) a.verdict = StatusVerdict::several_calls;
    else if (!last_fast || !has_last_call || attempt > 8) a.verdict = StatusVerdict::unresolved;
    else a.verdict = (st & kStBackOverflow) ? StatusVerdict::redo_atomic : StatusVerdict::redo_grown;  // (a full hand-back list is not a matter of bucket room)
    return a;
}

}  // namespace fgfa_dev
