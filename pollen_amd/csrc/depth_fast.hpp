// The bucketed node-depth path (depth_fast.hip); see DESIGN.md "Kernels".
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <mutex>

#include "../../include/flatgfa.h"

namespace fgfa_dev {

// The runtime keeps a kernel's attributes (hipFuncSetAttribute: more than 64 KB of dynamic LDS) per DEVICE, and one process
// may drive several (flatgfa_sharded_create: a plan per shard on its own device and host thread; Python: graphs on cuda:1 and
// up).  `fn` runs once per device that is current when a plan is made there; devices beyond the mask's 64 run it every time.
struct OncePerDevice {
    std::mutex mu;
    uint64_t done = 0;
    template <class F>
    bool operator()(F fn) {
        int dev = -1;
        if (hipGetDevice(&dev) != hipSuccess) return false;
        std::lock_guard<std::mutex> lk(mu);
        if (dev >= 0 && dev < 64 && ((done >> dev) & 1ull)) return true;
        if (!fn()) return false;
        if (dev >= 0 && dev < 64) done |= 1ull << dev;
        return true;
    }
};

// multiProcessorCount of a device, asked for once per device (depth_device.hip)
int device_cu_count(int device);
// the LDS of a CU of the current device, in bytes (depth_accum.hip; 0: not known)
uint32_t device_cu_lds_bytes();
// FLATGFA_TIMING=1: prints what the calling thread spent since its last tick (the device drained first), to stderr; `what` == nullptr restarts the clock
void plan_tick(const char *what);

// ---- what the plan and a call decide by (depth_plan_host.hpp, depth_call_host.hpp); the kernels' own constants are in depth_fast_kernels.hpp ----
constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
// status word bits (flatgfa_dev_status)
constexpr uint32_t kStBounds = 1u, kStDebug = 2u, kStOverflow = 4u, kStInternal = 8u, kStBackOverflow = 16u, kStStale = 32u;  // (32: FLATGFA_CHECK_NO_CLAIM=1 found the step values changed behind the plan)  // (16: more short paths handed back than the list holds: larger buckets would not help, the atomic kernels complete the call)  // (8: an invariant between the two passes did not hold -- a bug, reported as an error rather than as counts)
// The medium-path variant of k_scan_short: hash sets of 2048 entries, for paths whose run count (known to the plan) fits
// one -- seven sets and fourteen waves per workgroup, two waves per path (eight and eight, one wave per
// path, when built with -DFGFA_MEDIUM_PAIRED=0).
#ifndef FGFA_MEDIUM_PAIRED
#define FGFA_MEDIUM_PAIRED 1
#endif
constexpr bool kMediumPaired = FGFA_MEDIUM_PAIRED != 0;  // two waves per path and hash set (k_scan_short<..., PAIRED>)
constexpr int kMediumHash = 11, kMediumWaves = kMediumPaired ? 14 : 8;
#ifndef FGFA_SHORT_WAVES
#define FGFA_SHORT_WAVES 16
#endif
constexpr int kShortWaves = FGFA_SHORT_WAVES;  // waves of a k_scan_short workgroup (measurements: fewer = lower occupancy)
// k_scan's builds: plain, diagnostic (FLATGFA_DEBUG_SKIP), ranged (one of several walks of a graph beyond 16 M segments)
constexpr int kModePlain = 0, kModeDbg = 1, kModeRanged = 2, kModeBig = 3, kModeRangedBig = 4, kModePacked = 5, kModePackedRanged = 6, kModePlainFlags = 7, kModePackedFlags = 8, kModePlainNarrow = 9;  // (...Flags: the plain and the packed build for plans with per-block no-claim flags, ScanArgs::cflags)  // (Big: builds of their own for bucket arrays of 2^30 records or more, see put(); Packed: sub-buckets of exactly the size their records need, items dealt in a fixed order)
constexpr bool mode_ranged(int m) { return m == kModeRanged || m == kModeRangedBig || m == kModePackedRanged; }
constexpr bool mode_big(int m) { return m == kModeBig || m == kModeRangedBig; }
constexpr bool mode_packed(int m) { return m == kModePacked || m == kModePackedRanged || m == kModePackedFlags; }
constexpr bool mode_flags(int m) { return m == kModePlainFlags || m == kModePackedFlags; }
constexpr bool mode_plain(int m) { return m == kModePlain || m == kModePlainNarrow; }
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
constexpr uint32_t kAccWaves = 16;         // waves of a pass-2 workgroup
constexpr uint32_t kShortMax = 2048;       // steps; longer paths go through k_scan (or the medium variant)
constexpr uint32_t kTinyMax = 128;         // steps: a wave holds the whole path (k_scan_tiny)
#ifndef FGFA_QCAP
#define FGFA_QCAP 416
#endif
constexpr uint32_t kQCap = FGFA_QCAP;  // at least 64 left over + up to 257 from sixteen lanes of a block; a short path has at most kQCap - 16 runs, hence bitset words: its 512-entry hash set must not fill up
constexpr uint32_t kMediumRuns = 1500;
constexpr uint32_t kMaxHandBack = 4096;    // short paths k_scan_short may hand back to k_scan per call
constexpr uint32_t kTagCount = 512;        // tags a record can carry (depth_fast_kernels.hpp: kTagShift)
constexpr uint32_t kItemNoClaim = 0x80000000u;  // items[].z: the item's path is strictly monotone in the segment ids
constexpr uint32_t kTagSlots = 4;
constexpr uint32_t kMaxShared = 128;      // bitsets of split paths pass 2 has LDS for (4096-segment windows)
constexpr uint32_t kMaxWin = 2048;        // windows per launch (LDS tables: the cursors and their snapshots per item)
constexpr uint32_t kMaxWinTagged = 4096;  // ... of a plan whose calls are always tagged: k_scan keeps no snapshots then

struct FastPlan {
    bool eligible = false;
    bool cap_forced = false;   // FLATGFA_BUCKET_CAP (tests): the capacity must not grow
    // A plan covers the segments [seg_base, seg_base + n_range).  A graph beyond 16 M segments gets
    // several (`more`: a heap array of n_more further plans); each call then walks the steps once
    // per range, every walk keeping only the part of each run that falls into its range.
    uint32_t seg_base = 0, n_range = 0;
    FastPlan *more = nullptr;
    uint32_t n_more = 0;
    uint32_t n_cus = 256;
    bool tagged = false;       // k_scan's records can carry their item's tag: pass 2 then walks whole sub-buckets and needs no directory (depth_fast.hip: kTagShift)
    uint32_t tag_limit = 0;    // tagged: items a k_scan workgroup may take (its private tags; at most 512 less the split paths; FLATGFA_TAG_LIMIT shrinks it for tests)
    uint32_t n_shared = 0;     // paths cut into pieces (their bitsets are shared by all waves of a pass-2 workgroup in a tagged call)
    bool big_groups = false;   // pass 2 looks for steps that lie inside one item (worth it when a path has hundreds of records per window; the plan's creator times both)
    bool dense_maybe = false;  // between one and nine records for ten steps: the plan's creator times k_scan_dense against k_scan
    bool dense = false;        // nearly every step starts a run: pass 1 partitions the steps themselves (k_scan_dense)
    bool narrow_emit = false;  // fewer than a record for eight steps: the plain tagged build of k_scan that emits two chunks side by side, not four (kModePlainNarrow)
    uint32_t acc_parts = 1;  // workgroups per window in pass 2 (small graphs: fewer windows than CUs)
    uint64_t est_records = 0;  // records k_scan will make of its items (counted when the plan is made)
    bool acc_pair = false;     // tagged calls with unique depth run two workgroups per window, both resident on a CU (k_accum_pair)
    uint32_t acc_slots = 4;    // private bitsets per wave of the tagged walk
    bool acc_own = false;      // ... which keeps track of their owners (k_accum<..., OWN>): sub-buckets of sparse tags
    uint32_t *pair_part = nullptr, *pair_flag = nullptr;  // their halves of the result vectors, and how many are there
    // Packed buckets: every (window, workgroup) sub-bucket has exactly the room its records need (counted once when the
    // plan is made, k_scan dealing its items in a fixed order from then on), a workgroup's sub-buckets back to back.
    uint64_t mall_steps = 0;       // the steps below this index are read without the nt hint: they stay in the Infinity Cache from call to call (plan_create decides)
    bool packed = false;
    bool can_pack = false;         // create_range: the plan could have packed buckets (tagged, all records k_scan's, ...): whether making it again for them can lead anywhere
    uint32_t *pk_off = nullptr;    // u32[n_slots][n_win + 1] sub-bucket starts within the workgroup's region; the last entry is its sink
    uint64_t *pk_base = nullptr;   // u64[n_slots] where each workgroup's region starts
    void *pk = nullptr;            // uint2[n_win][n_slots] {start in the array, room} for pass 2
    uint64_t bucket_records = 0;   // records the bucket array has room for (what flatgfa_dev_plan_describe reports as scratch)
    uint32_t n_slots = 0;      // sub-buckets per window = persistent workgroups of pass 1
    uint32_t n_win = 0;        // accumulation windows
    uint32_t wb = 12;          // log2 of the window size (4096 segments, 8192 beyond 4 M segments)
    uint32_t nwp = 0;          // n_win rounded up to a multiple of 64
    uint32_t cap = 0;          // records per (window, sub-bucket)
    uint32_t lds_bytes_scan = 0;
    uint32_t dbg = 0;          // FLATGFA_DEBUG_SKIP ablation mask (diagnostics only)
    uint32_t *counts = nullptr;    // u32[n_win * n_slots] cursors, zero between calls (pass 2 resets)
    uint32_t *counts0 = nullptr;   // u32[n_win * n_slots] the cursors k_scan started from
    uint32_t *buckets = nullptr;   // u32[(n_win + 1) * n_slots * cap]
    void *dir = nullptr;           // uint2[n_win * dstride] {cursor before, after} each item, per window, in pass 2's walk order
    uint32_t *islot = nullptr;     // u32[dstride] per position of pass 2's walk order: the sub-bucket that holds the item's records | first of its path << 31
    uint32_t *perm = nullptr;      // u32[n_items] where item j stands in pass 2's walk order | first of its path << 31
    uint32_t dstride = 0;          // n_items + max_back + 1
    uint32_t *lists_slab = nullptr;  // one allocation behind perm, elist, wave_off, fat_off and fat_woff
    uint32_t *elist = nullptr;     // k_scan's items in pass 2's order (grouped by path, split among its waves)
    uint32_t *wave_off = nullptr;  // u32[16 * acc_parts + 1] the stretch of elist each wave of pass 2 walks
    uint32_t *fat_off = nullptr;   // u32[acc_parts + 1] the long paths each of a window's workgroups walks with all its waves
    uint32_t *fat_woff = nullptr;  // u32[n_fat][17] the stretch of elist each wave walks of such a path's items
    uint32_t n_fat = 0;
    void *items = nullptr;         // uint4[n_items + max_back] whole paths and pieces of long paths, longest first,
                                   // with room for the short paths k_scan_short hands back
    uint32_t n_items = 0;
    uint32_t n_noclaim = 0;        // items whose path walks the segment ids strictly one way (their records skip pass 2's claim: depth_fast.hip kTagNoClaim)
    uint32_t *cflags = nullptr;    // a bit per 16 steps of the step array, of which the one of a k_scan block's FIRST chunk counts: every chunk of the block
                                   // lies in windows its path enters once and walks one way, and the block makes no-claim records too (k_visit_bits,
                                   // k_chunk_flags, k_block_flags); nullptr: none
    uint64_t n_flag_chunks = 0;    // how many chunks say so
    bool marks_wanted = false;     // create_range: this plan may gain from such marks (tagged, one range, items that claim) -- they are made off the
                                   // critical path (fast_marks_start on a side stream, fast_marks_finish installs them between two calls)
    uint64_t item_steps = 0;       // steps of k_scan's items (what the marks' share is measured against)
    uint32_t max_back = 0;
    bool accumulate = false;       // a group of paths behind the first (see fast_plan_create): pass 2 adds to the outputs
    bool too_many_items = false;   // create_range's verdict: only the number of items (or of split paths) per k_scan workgroup stands between this range and a tagged plan
    bool want_wb12 = false;        // ... or only the split paths' bitsets, for which pass 2 has LDS with 4096-segment windows
    uint32_t n_groups = 1;         // (of the first plan) path groups the ranges of `more` belong to
    bool exact_short = false;      // the wave-per-path lists hold only paths that fit: nothing is handed back to k_scan
    void *short_items = nullptr;   // uint4[n_short] paths every wave walks on its own (k_scan_short): first those read from the graph's
                                   // steps, then n_short_rev paths that walk the ids downwards, read from rev_steps (their
                                   // steps in reverse order: a wave-per-path kernel only knows runs that go up)
    uint32_t n_short = 0, n_short_rev = 0;
    // the paths of a wave-per-path list that walk the segment ids strictly one way -- no segment twice, so no claim --
    // lie at [mono_lo, mono_lo + mono_n) of their list, on both sides of the boundary to the reversed ones
    uint32_t short_mono_lo = 0, short_mono_n = 0, medium_mono_lo = 0, medium_mono_n = 0, tiny_mono_lo = 0, tiny_mono_n = 0;
    uint32_t *rev_steps = nullptr; // the reversed copies, every path at a multiple of 16
    uint32_t n_rev_steps = 0;
    uint32_t lds_bytes_short = 0;
    void *medium_items = nullptr;  // uint4[n_medium] longer paths with few enough runs for a 2048-entry hash set
    uint32_t n_medium = 0, n_medium_rev = 0;  // (laid out like short_items)
    uint32_t lds_bytes_medium = 0;
    void *tiny_items = nullptr;    // uint4[n_tiny] paths of at most 128 steps: a wave holds one whole (k_scan_tiny)
    uint32_t n_tiny = 0;
    uint64_t class_steps[4] = {0, 0, 0, 0};  // steps walked by k_scan / k_scan_short / k_scan_medium / k_scan_tiny (flatgfa_dev_plan_describe)
    uint32_t lds_bytes_tiny = 0;
    uint32_t *taken = nullptr;         // u32[n_slots] items each workgroup of the last tagged k_scan took
    uint32_t *work_counter = nullptr;  // how many short paths were handed back in this call
    void *psum_part = nullptr;         // ulonglong2[n_win * dstride] per-window path sums of k_scan's items (on first use)
    uint32_t *other_ids = nullptr;     // u32[n_other] the paths k_scan_short walks (their sums need k_path_sums)
    uint32_t n_other = 0;
    // The run-length image of the step array, once it is installed (run_image_install): tagged calls then run k_scan_runs on
    // the image's entries, not k_scan on the steps.  The entries are the image's (shared by the plans of one step array), the
    // items' stretches of them are the plan's handle's; neither is freed by fast_plan_destroy.
    const void *run_ent = nullptr;       // uint2[run_n_ent + 1]
    const void *run_item_ent = nullptr;  // uint2[n_items] the entries each item reads
    uint32_t run_n_ent = 0;
    bool run_nt = false;                 // the entries are read past the caches (they do not fit the Infinity Cache beside the records)
    // u32[n_win * n_slots] the cursors k_scan_runs left, a second time: pass 2 zeroes `counts` behind every call, a call that
    // runs on the records of the image call before it (RecordsUse) reads these and leaves them.  nullptr: records are never kept.
    uint32_t *counts_kept = nullptr;
    // The plan's sorted record image, once it is installed (sorted_image_install): the same records in the
    // order pass 2 sweeps them in, a carry word per chunk of them, and every window's chunks.  The calls that would run pass 2
    // alone on the kept records run k_accum_sorted on these.  The plan's handle's; not freed by fast_plan_destroy.
    const uint32_t *sorted_rec = nullptr, *sorted_carry = nullptr, *sorted_win_chunk = nullptr;
    bool sorted_nt = false;              // read past the caches (image and results do not fit the Infinity Cache)
    // which cells the sweep for unique depth adds into (depth_sorted_host.hpp, kSortedCells...): packed where the image's build
    // found the rule to hold; 0: not known, which sweeps wide cells
    uint32_t sorted_cells = 0;
    // dynamic LDS, in bytes, the sweep is launched with so that no second sweep workgroup fits its CU (a pipeline lane's plan,
    // depth_call_host.hpp: sorted_solo_lds); 0: two workgroups share a CU
    uint32_t sorted_solo_lds = 0;
};

// What a plan's handle tells a call about the records in the plan's scratch, and what the call tells it back.  k_scan_runs'
// deal of the items is fixed and so is the image, so an image call writes the same records into the same slots as the image
// call before it: where nothing else has written to the scratch since (the handle's business), pass 1 is left out.
struct RecordsUse {
    bool use = false;         // in: buckets, `taken` and counts_kept are those of a complete image call of this plan
    bool from_image = false;  // out: this call was an image call of a plan with counts_kept -- they are (still) there behind it
};

// A plan's ranges and path groups, one after the other: the first plan itself, then more[0 .. n_more).  `Plan` is FastPlan or
// const FastPlan, and fn takes a reference to the same.
template <class Plan, class Fn>
inline void for_each_range(Plan &fp, Fn fn) {
    fn(fp);
    for (uint32_t r = 0; r < fp.n_more; ++r) {
        Plan &q = fp.more[r];
        fn(q);
    }
}
// ... and whether `pred` holds for all of them / for at least one
template <class Pred>
inline bool all_ranges(const FastPlan &fp, Pred pred) {
    bool all = true;
    for_each_range(fp, [&](const FastPlan &q) { all = all && pred(q); });
    return all;
}
template <class Pred>
inline bool any_range(const FastPlan &fp, Pred pred) {
    return !all_ranges(fp, [&](const FastPlan &q) { return !pred(q); });
}

// The per-block no-claim marks of a plan (k_visit_bits, k_chunk_flags, k_block_flags: three more reads of the steps) are
// not on the way to the first answer: a job enqueues them on a stream of its own; once they are there they are looked
// at on the host (do enough blocks qualify?) and installed between two calls.
struct MarksJob {
    bool active = false;
    uint32_t *vis = nullptr, *pbeg = nullptr, *chunks = nullptr, *flags = nullptr;
    unsigned long long *cnt = nullptr;
    hipEvent_t done = nullptr;
};
// Enqueues the job's kernels on `side` (which must not be a stream a call of the plan runs on).  `host_path_begin`: the
// spans the plan was made with (P entries, alive until the job is finished).  False on a HIP error (the plan then
// simply has no marks).  A plan that does not want marks (fp.marks_wanted) gets no job: job->active stays false.
bool fast_marks_start(const FastPlan &fp, const flatgfa_dev_graph_t &g, const uint32_t *host_path_begin, hipStream_t side, MarksJob *job);
// Has the job finished?  (never blocks)
bool fast_marks_ready(const MarksJob &job);
// Waits for the job, releases its scratch and installs the marks in `fp` if enough blocks qualify (no call of the plan
// may be enqueued concurrently from another thread; calls already running are not affected: their arguments were
// copied when they were launched).
void fast_marks_finish(FastPlan *fp, MarksJob *job);
// Debug (FLATGFA_CHECK_NO_CLAIM=1): re-derives, on `stream` and before a call's kernels, the facts about the step values
// that the plan relies on without re-checking them per call -- items and short paths found strictly monotone, the
// per-block marks, the reversed copies -- and raises status bit kStStale where one no longer holds.
int fast_check_plan_facts(const FastPlan &fp, const flatgfa_dev_graph_t &g, const uint32_t *host_path_begin, const uint32_t *host_path_end, uint32_t *status,
                          hipStream_t stream);

// The run-length image of a resident step array (depth_scan_runs.hip): one 8-byte entry per maximal
// run of consecutive segment ids, made by a few kernels on `side` in two stages with the host in between (it has to know how
// many entries there are before it gives them room).
struct RunImage;
// Enqueues the first stage (count, scan).  Never null; an image that cannot be had says so when it is polled.
RunImage *run_image_start(const flatgfa_dev_graph_t &g, hipStream_t side);
// Moves the image on as far as it can without blocking (`wait`: until it is there): 1 = there, 0 = not yet, -1 = not to be had
// (run_image_why: "runs" -- more than an entry for four steps, unless any_ratio --, "memory" -- it would leave less than `reserve` bytes of device memory free --, "error").
int run_image_poll(RunImage *im, hipStream_t side, bool wait, uint64_t reserve, bool any_ratio);
const char *run_image_why(const RunImage *im);
uint64_t run_image_bytes(const RunImage *im);  // entries and index, once it is there
void run_image_free(RunImage *im, hipStream_t side);
// The entries each of the plan's items reads (uint2[n_items], the caller's to free) and, in *room (the caller's to free), how many
// records k_scan_runs -- whose deal of the items is fixed -- will put into each sub-bucket, computed on `side`; *done is recorded behind it.
bool run_items_start(const FastPlan &fp, const RunImage *im, hipStream_t side, void **item_ent, void **room, hipEvent_t *done);
// ... the fullest of them (once *done has happened): the image is installed in a plan whose sub-buckets hold that many
uint32_t run_room_needed(const FastPlan &fp, const void *room);
// From the plan's next tagged call on, pass 1 reads the image.  (No call of the plan may be enqueued concurrently from another thread.)
void run_image_install(FastPlan *fp, const RunImage *im, void *item_ent, bool nt);

// The sorted record image of a plan whose run image is installed (depth_sorted.hip): made on `side` in two
// stages with the host in between -- the records are counted per window, then emitted as (key, record) pairs, sorted, and
// finalised into chunks.  Never null; one that cannot be had says so when it is polled.
struct SortedImage;
SortedImage *sorted_image_start(const FastPlan &fp, uint32_t n_paths, hipStream_t side);
// 1 = there, 0 = not yet, -1 = not to be had (sorted_image_why: "bounds" -- a record was dropped, pass 1 has an error to raise --,
// "memory" -- the build would leave less than `reserve` bytes free, unless `waived` --, "size", "error")
int sorted_image_poll(SortedImage *si, const FastPlan &fp, hipStream_t side, bool wait, uint64_t reserve, bool waived);
const char *sorted_image_why(const SortedImage *si);
uint64_t sorted_image_bytes(const SortedImage *si);      // what the plan keeps, once it is there
uint64_t sorted_image_transient(const SortedImage *si);  // what the build held beside that (the description reports both)
int sorted_image_phase(const SortedImage *si);           // 1: counted (enqueued), 2: emitted, sorted, finalised (enqueued), 3: there, -1: not to be had
void sorted_image_install(FastPlan *fp, const SortedImage *si, bool nt);
void sorted_image_free(SortedImage *si, hipStream_t side);

// Decides eligibility (16-byte aligned steps, directories that stay small next to the steps) and
// allocates the scratch: one range of at most 2048 windows, or several.  Returns false only on a HIP error.
// `scan_workgroups`: how many persistent workgroups pass 1 runs (= sub-buckets per window); 0 = one per CU.  A plan that
// is one lane of a pipeline (calls in flight) takes fewer, so that another call's kernels share the chip with its pass 1.
// `prefer_packed`: record buckets laid out to the count wherever the plan allows it (by default only where the even layout
// would take gigabytes from the start).
bool fast_plan_create(const flatgfa_dev_graph_t &g, const uint32_t *host_path_begin, const uint32_t *host_path_end,
                      FastPlan *fp, uint32_t scan_workgroups = 0, bool prefer_packed = false);
void fast_plan_destroy(FastPlan *fp);
// After a call whose records did not fit their sub-buckets (status bit 4): quadruple the capacity.
// Returns false -- and marks the plan ineligible -- when that is not possible.
// gives back the bucket arrays kept for the next plan (one per device)
void fast_release_scratch();
bool fast_plan_grow(FastPlan *fp, bool ahead_of_need = false);  // ahead_of_need: a plan that cannot grow stays eligible
// Per-path sums of measure_path (depth.rs:116-131), accumulated by pass 2 of a seg_depth call for
// the paths k_scan walks (plan.other_ids lists the rest): u64[n_paths] each, zeroed by the caller.
struct PathSums {
    uint64_t *len_out, *weighted_out;  // one per path of the graph
    bool clear = false;                // the call zeroes them first (inside k_scan where it runs)
};
// Allocates (once) the scratch `ps` needs; false = not possible for this plan.
bool fast_plan_want_path_sums(FastPlan *fp);
// Enqueues the kernels, one range after the other.  uniq_out may be NULL (seg_depth); `ps` only with uniq_out == NULL and
// after fast_plan_want_path_sums.  `records`: see RecordsUse; nullptr = pass 1 runs, and the caller must take its
// scratch for overwritten.  What a call is made of is decided first (depth_call_host.hpp: decide_call -- which launches, how
// large, who zeroes what, which build of k_scan); a call it refuses (FLATGFA_ERR_ARG: path sums outside their precondition, a
// packed plan or a bucket array of 2^30 records called untagged) has enqueued nothing for the range that refused it.
int fast_seg_depth(const FastPlan &fp, const flatgfa_dev_graph_t &g, uint32_t *depth_out, uint32_t *uniq_out,
                   uint32_t *status, hipStream_t stream, const PathSums *ps = nullptr, RecordsUse *records = nullptr);

}  // namespace fgfa_dev
