// The host's decisions about one call of a bucketed depth plan and about the status word behind it
// (pollen_amd/csrc/depth_call_host.hpp: decide_call, scan_mode, status_verdict) on their own, without a GPU: every
// combination of the facts they read, and for each what the kernels and the handle rely on.
// Built twice by `make -C pollen_amd/csrc call_check call_check_asan`; tests/test_host_sanitized_call.py runs both.
//
// The space: every boolean of FastPlan the functions read (as pointers where they are pointers), a ranged plan, a big bucket
// array, each count in {0, 1, several}, FLATGFA_SCAN_ALWAYS, records_use, and the call kinds (unique depth, depth, the
// counting call, path sums with and without `clear`).  What a kind does not read is not multiplied in: the path sums'
// precondition (wb in {11, 12, 13}, the sums' scratch, seg_len, the whole graph) is run through all its values for the two
// path-sum kinds, over the plan's booleans, and holds for the rest of their space; the four hooks decide_call does not decide
// by (they belong to the arguments and the diagnostics) and n_more (which only the description reads) go round with the
// case number, so that every value of them meets every property.
#include <cstdio>
#include <cstdlib>

#include "depth_call_host.hpp"

using namespace fgfa_dev;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

static const uint32_t kCounts[3] = {0, 1, 7};
static const uint32_t kSlots = 4;  // fewer than "several": both arms of every min() are reached
static uint32_t g_dummy[4];        // what the plan's pointers point at (never read)

struct Kind {
    const char *name;
    CallWants w;
};
static const Kind kKinds[5] = {{"uniq", {true, false, false, false}}, {"depth", {false, false, false, false}}, {"count", {false, false, false, true}},
                               {"sums+clear", {false, true, true, false}}, {"sums", {false, true, false, false}}};

struct Tally {
    unsigned long long cases = 0, refused = 0, skipped = 0, image = 0, kept = 0, narrow = 0, by_kscan = 0, by_memset = 0;
};

// bits of `b`: the plan's booleans
enum : uint32_t { bTagged = 1, bPacked = 2, bDense = 4, bNarrow = 8, bExact = 16, bAccumulate = 32, bDbg = 64, bCflags = 128, bKept = 256, bRanged = 512, bBig = 1024, bAll = 2048 };

static FastPlan plan_of(uint32_t b, int image, uint32_t n_items, uint32_t n_short, uint32_t n_medium, uint32_t n_tiny, uint32_t acc_parts, uint32_t wb, bool psum_part, bool whole) {
    FastPlan fp;
    fp.eligible = true;
    fp.tagged = b & bTagged;
    fp.packed = b & bPacked;
    fp.dense = b & bDense;
    fp.narrow_emit = b & bNarrow;
    fp.exact_short = b & bExact;
    fp.accumulate = b & bAccumulate;
    fp.dbg = (b & bDbg) ? 32u : 0u;
    fp.cflags = (b & bCflags) ? g_dummy : nullptr;
    fp.counts_kept = (b & bKept) ? g_dummy : nullptr;
    fp.n_range = whole ? 8192 : 4096;  // (of a graph of 8192 segments)
    fp.seg_base = (b & bRanged) ? 4096 : 0;
    fp.n_slots = kSlots;
    fp.n_win = 2;
    fp.cap = (b & bBig) ? (1u << 28) : 1024u;  // three windows of four sub-buckets: 3 * 2^30 records, or 12288
    fp.run_ent = image >= 1 ? g_dummy : nullptr;
    fp.run_item_ent = image >= 2 ? g_dummy : nullptr;
    fp.n_items = n_items;
    fp.n_short = n_short;
    fp.n_medium = n_medium;
    fp.n_tiny = n_tiny;
    fp.acc_parts = acc_parts;
    fp.wb = wb;
    fp.psum_part = psum_part ? g_dummy : nullptr;
    fp.max_back = 5;
    return fp;
}

static bool registered(ScanMode m) {  // depth_scan.hip: scan_kernels_setup
    switch (m.mode) {
    case kModeDense: return true;
    case kModePlain: case kModeRanged: return true;  // (both builds)
    case kModeBig: case kModeRangedBig: case kModePacked: case kModePackedRanged: case kModePlainFlags: case kModePackedFlags: case kModePlainNarrow: return m.tagged;
    default: return false;
    }
}

static void check_case(const FastPlan &fp, const GraphFacts &g, const Kind &k, const CallHooks &hooks, bool records_use, Tally *t) {
    const CallWants &w = k.w;
    const CallShape s = decide_call(fp, g, w, hooks, records_use);
    t->cases += 1;
    const bool whole = fp.seg_base == 0 && fp.n_range == g.n_segs;
    const bool sums_ok = !w.psum || (!w.uniq && fp.wb == 12 && g.has_seg_len && fp.psum_part && fp.n_range == g.n_segs);
    const bool tagged = fp.tagged && !w.psum, has_pre = fp.n_short || fp.n_medium || fp.n_tiny;
    const bool big = 3ull * kSlots * fp.cap >= (1ull << 30);
    const bool skipped = has_pre && !fp.n_items && fp.exact_short && !fp.dbg && !hooks.scan_always;
    const bool pass1 = !skipped && (has_pre || fp.n_items);  // a launch for the items, unless their records are kept
    // the refusals: path sums outside their precondition, a packed plan called untagged, k_scan on a big array untagged
    const bool refuse = !sums_ok || (fp.packed && !tagged) || (big && !tagged && !fp.dense && pass1);
    CHECK((s.refusal != nullptr) == refuse);
    if (s.refusal) {  // ... which carry no launches
        CHECK(!s.grid && !s.grid_tiny && !s.grid_short && !s.grid_medium && !s.scans() && s.outputs == Zeroes::nobody && s.sums == Zeroes::nobody);
        t->refused += 1;
        return;
    }
    CHECK(s.tagged == tagged && s.has_pre == has_pre && s.ranged == !whole && s.big == big && s.scan_skip == skipped);
    if (w.psum) CHECK(!s.tagged);
    // k_scan's grid and what the two passes are told about the wave-per-path kernels
    if (s.scan_skip) CHECK(s.grid == 0 && s.max_back == 0 && s.has_pre2 == 2);
    else if (!has_pre) CHECK(s.grid == std::min(fp.n_items, fp.n_slots) && s.has_pre2 == 0 && s.max_back == fp.max_back);
    else CHECK(s.grid == fp.n_slots && s.has_pre2 == 1 && s.max_back == fp.max_back);
    CHECK((s.grid > 0) == pass1);
    // the wave-per-path grids: a launch iff the list has paths, never more workgroups than sub-buckets, all paths covered
    const uint32_t n[3] = {fp.n_tiny, fp.n_short, fp.n_medium}, grids[3] = {s.grid_tiny, s.grid_short, s.grid_medium};
    const uint32_t per_wg[3] = {(uint32_t)kWaves, (uint32_t)kShortWaves, (uint32_t)(kMediumPaired ? kMediumWaves / 2 : kMediumWaves)};
    for (int i = 0; i < 3; ++i) {
        CHECK((grids[i] > 0) == (n[i] > 0) && grids[i] <= fp.n_slots);
        CHECK(grids[i] == fp.n_slots || (uint64_t)grids[i] * per_wg[i] >= n[i]);
    }
    // the run image and the kept records
    if (s.kept) CHECK(s.from_image && records_use && fp.counts_kept);
    if (s.from_image) {
        CHECK(s.tagged && s.grid > 0 && !fp.dense && !fp.packed && !s.ranged && !s.cflags && !has_pre && !fp.dbg && !w.count_only);
        CHECK(fp.run_ent && fp.run_item_ent);
        t->image += 1;
    }
    t->kept += s.kept;
    t->skipped += s.scan_skip;
    // who zeroes what pass 2 and k_path_reduce add to: exactly one party, k_scan iff it runs
    const Zeroes who = s.grid > 0 && !s.kept ? Zeroes::k_scan : Zeroes::memset;
    CHECK(s.scans() == (who == Zeroes::k_scan));
    CHECK(s.outputs == (fp.acc_parts > 1 && !fp.accumulate && !w.count_only ? who : Zeroes::nobody));
    CHECK(s.sums == (w.psum && w.psum_clear ? who : Zeroes::nobody));
    t->by_kscan += (s.outputs == Zeroes::k_scan) + (s.sums == Zeroes::k_scan);
    t->by_memset += (s.outputs == Zeroes::memset) + (s.sums == Zeroes::memset);
    // the build of k_scan, where it is k_scan that runs
    if (!s.scans() || s.from_image) return;
    const ScanMode m = scan_mode(fp, s);
    CHECK(registered(m));
    if (m.mode == kModeDense) {
        CHECK(fp.dense);
        return;
    }
    CHECK(!fp.dense && m.tagged == s.tagged);
    if (!m.tagged) CHECK(m.mode == kModePlain || m.mode == kModeRanged);
    if (mode_flags(m.mode)) CHECK(fp.cflags && s.cflags);
    CHECK(mode_packed(m.mode) == fp.packed);
    CHECK(mode_ranged(m.mode) == s.ranged);
    if (!fp.packed) CHECK(mode_big(m.mode) == s.big);  // (a packed call's offsets are its region's)
    // the narrow build only where the plan's description says emit=two_chunks (of a plan of one range)
    if (m.mode == kModePlainNarrow) {
        CHECK(fp.narrow_emit && fp.tagged && !fp.packed && !fp.dense && !(fp.cflags && s.tagged));
        t->narrow += 1;
    }
}

static void check_shapes() {
    Tally t;
    unsigned long long round = 0;
    for (uint32_t b = 0; b < bAll; ++b)
        for (int image = 0; image < 3; ++image)
            for (uint32_t n_items : kCounts)
                for (uint32_t n_short : kCounts)
                    for (uint32_t n_medium : kCounts)
                        for (uint32_t n_tiny : kCounts)
                            for (uint32_t acc_parts : kCounts) {
                                FastPlan fp = plan_of(b, image, n_items, n_short, n_medium, n_tiny, acc_parts, 12, true, !(b & bRanged));
                                for (int always = 0; always < 2; ++always)
                                    for (int use = 0; use < 2; ++use)
                                        for (const Kind &k : kKinds) {
                                            round += 1;
                                            CallHooks hooks;
                                            hooks.scan_always = always;
                                            hooks.no_plain = round & 1;
                                            hooks.acc_time = round & 2;
                                            hooks.scan_time = (round & 4) ? "x" : nullptr;
                                            hooks.acc_skip = (round & 8) ? "64" : nullptr;
                                            fp.n_more = kCounts[(round >> 4) % 3];
                                            check_case(fp, {8192, true}, k, hooks, use, &t);
                                        }
                            }
    std::printf("shapes ok: %llu cases, %llu refused, %llu without k_scan, %llu from the image (%llu on kept records), %llu narrow, zeroed by k_scan %llu / by memsets %llu\n",
                t.cases, t.refused, t.skipped, t.image, t.kept, t.narrow, t.by_kscan, t.by_memset);
    // the path sums' precondition, through all its values
    Tally p;
    for (uint32_t b = 0; b < bAll; ++b)
        for (uint32_t wb = 11; wb <= 13; ++wb)
            for (int part = 0; part < 2; ++part)
                for (int len = 0; len < 2; ++len)
                    for (int whole = 0; whole < 2; ++whole)
                        for (const Kind &k : kKinds) {
                            const FastPlan fp = plan_of(b & ~bRanged, 2, 7, 0, 0, 0, 1, wb, part, whole && !(b & bRanged));
                            check_case(fp, {8192, len != 0}, k, CallHooks(), false, &p);
                        }
    std::printf("path sums ok: %llu cases, %llu refused\n", p.cases, p.refused);
}

static void check_status() {
    unsigned long long n = 0, by[8] = {};
    const uint32_t over = kStOverflow | kStBackOverflow, errs = kStBounds | kStStale | kStInternal;
    for (uint32_t st = 0; st < 64; ++st)
        for (uint32_t full = 0; full < 2; ++full)
            for (uint32_t calls = 0; calls < 3; ++calls)
                for (int attempt : {0, 1, 9})
                    for (int last_fast = 0; last_fast < 2; ++last_fast)
                        for (int has_last = 0; has_last < 2; ++has_last) {
                            const uint32_t st3[3] = {st, 77, full};
                            const StatusAction a = status_verdict(st3, calls, attempt, last_fast, has_last);
                            const StatusVerdict v = a.verdict;
                            n += 1;
                            CHECK((int)v >= 0 && (int)v < 8);
                            by[(int)v] += 1;
                            // bounds before stale before internal before overflow
                            if (st & kStBounds) CHECK(v == StatusVerdict::bounds);
                            else if (st & kStStale) CHECK(v == StatusVerdict::stale);
                            else if (st & kStInternal) CHECK(v == StatusVerdict::internal);
                            else if (!(st & over)) CHECK(v == StatusVerdict::fine);  // (nothing, or a diagnostic's sentinel)
                            else {
                                // several calls: the "call it after every call" error, on attempt 0 only
                                const bool several = attempt == 0 && calls > 1;
                                CHECK((v == StatusVerdict::several_calls) == several);
                                if (!several) {
                                    const bool can = last_fast && has_last && attempt <= 8;
                                    CHECK((v == StatusVerdict::unresolved) == !can);
                                    if (can) CHECK(v == ((st & kStBackOverflow) ? StatusVerdict::redo_atomic : StatusVerdict::redo_grown));
                                }
                            }
                            if (st & errs) CHECK(v != StatusVerdict::redo_grown && v != StatusVerdict::redo_atomic);
                            if (st & kStBackOverflow) CHECK(v != StatusVerdict::redo_grown && !a.grow_ahead);  // bit 16 never grows
                            CHECK(a.grow_ahead == (full && !(st & over)));
                        }
    std::printf("status ok: %llu cases: fine %llu, errors %llu %llu %llu %llu, redo grown %llu, redo atomic %llu, unresolved %llu\n", n, by[0], by[1], by[2], by[3], by[4], by[5],
                by[6], by[7]);
}

int main() {
    check_shapes();
    check_status();
    std::printf("all ok\n");
    return 0;
}
