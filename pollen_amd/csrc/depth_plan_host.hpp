// The host's decisions about a bucketed node-depth plan (depth_fast.hip: create_range), as functions over plain data:
// which kernel walks which path, how long paths are cut and dealt, whether records are tagged, the order pass 2
// walks the items in, how packed buckets are laid out.  No HIP runtime call and no environment variable in here:
// create_range reads the test hooks, runs the device steps and hands their results in, and
// tests/host_check/plan_check.cpp runs these stages without a GPU and asserts what the kernels rely on.
#pragma once
#include <algorithm>
#include <cstdint>
#include <functional>
#include <numeric>
#include <queue>
#include <utility>
#include <vector>

#include "depth_fast.hpp"
#include "temp_arena.hpp"

namespace fgfa_dev {

struct LongerItem {  // (a type, not a function: the sorts inline it)
    bool operator()(const uint4 &a, const uint4 &b) const { return a.y - a.x > b.y - b.x; }
};
inline uint64_t steps_of(const Vec<uint4> &v) {
    uint64_t n = 0;
    for (const uint4 &d : v) n += d.y - d.x;
    return n;
}

// ---- which kernel walks which path ----
// A wave-per-path list: the paths read from the graph's steps, then those read from their reversed copies; of
// either kind the ones that need no claim lie next to the boundary, so that one stretch of the list names them
// all: [claim][no claim | no claim, reversed][claim, reversed], each part longest first.
struct WaveList {
    Vec<uint4> items;
    uint32_t n_rev = 0, mono_lo = 0, mono_n = 0;
};
struct PathClasses {
    Vec<uint4> whole;      // k_scan's paths, as {first step, one past the last, kNoSlot, path}
    Vec<uint4> rev_list;   // {first step, one past the last, where the reversed copy starts, path}
    uint64_t rev_len = 0;  // steps the reversed copies take (every copy starts at a multiple of 16)
    WaveList shorts, mediums, tiny;
};
struct ClassifyIn {
    const uint32_t *hb, *he;  // the spans the plan walks
    uint32_t n_paths;
    uint64_t n_steps;                        // the step array's
    uint64_t short_max;                      // 0: the wave-per-path kernels are not to be had, everything is k_scan's
    const uint32_t *runs, *runs_down, *mono;  // k_count_runs' (read only with short_max)
    bool short_any, no_rev, no_tiny;          // hooks: FLATGFA_SHORT_ANY, FLATGFA_NO_REVERSED_COPIES, FLATGFA_NO_TINY
};
// A wave-per-path kernel only knows runs that go up.  A path that walks the ids downwards (a
// contig on the reverse strand) has far fewer runs when it is read backwards, and the order of a
// path's steps does not matter to the counts: such a path is walked from a reversed copy of its steps.
// (the *_mono lists: paths that walk the ids strictly one way -- the wave-per-path kernels skip their claims)
inline PathClasses classify_paths(const ClassifyIn &in) {
    PathClasses c;
    Vec<uint4> short_mono, short_rev_mono, short_rev, medium_mono, medium_rev_mono, medium_rev, tiny_mono;
    const uint64_t short_max = in.short_max;
    for (uint32_t p = 0; p < in.n_paths; ++p) {
        const uint64_t b = in.hb[p], e = in.he[p], n = e - b;
        if (n == 0) continue;
        const bool in_reach = ((e + 15) & ~15ull) <= in.n_steps;  // the last block must not read past the step array
        const bool down = short_max && !in.no_rev && in.runs_down[p] < in.runs[p] && c.rev_len + n + 2048 < 0xFFFFFFFFull;
        const uint32_t rn = short_max ? (down ? in.runs_down[p] : in.runs[p]) : 0u;
        const bool is_tiny = n <= std::min<uint64_t>(short_max, kTinyMax) && !in.no_tiny;  // (k_scan_tiny: a wave holds the whole path)
        const bool is_short = !is_tiny && n <= short_max && (down || in_reach) && (rn + 16 <= kQCap || in.short_any);
        const bool is_medium = !is_tiny && !is_short && short_max && (down || in_reach) && rn <= kMediumRuns;
        const bool mn = short_max && in.mono[p] != 0u;
        const uint4 it = make_uint4((uint32_t)b, (uint32_t)e, kNoSlot, p);
        if (is_tiny) {
            (mn ? tiny_mono : c.tiny.items).push_back(it);
        } else if ((is_short || is_medium) && down) {
            const uint32_t at = (uint32_t)c.rev_len;
            c.rev_list.push_back(make_uint4((uint32_t)b, (uint32_t)e, at, p));
            (is_short ? (mn ? short_rev_mono : short_rev) : (mn ? medium_rev_mono : medium_rev)).push_back(make_uint4(at, at + (uint32_t)n, kNoSlot, p));
            c.rev_len += (n + 15) & ~15ull;
        } else if (is_short) {
            (mn ? short_mono : c.shorts.items).push_back(it);
        } else if (is_medium) {
            (mn ? medium_mono : c.mediums.items).push_back(it);
        } else {
            c.whole.push_back(it);
        }
    }
    const auto lay_out = [](WaveList *l, Vec<uint4> *fwd_mono, Vec<uint4> *rev_mono, Vec<uint4> *rev) {
        for (Vec<uint4> *v : {&l->items, fwd_mono, rev_mono, rev}) std::stable_sort(v->begin(), v->end(), LongerItem());
        l->mono_lo = (uint32_t)l->items.size();
        l->mono_n = (uint32_t)(fwd_mono->size() + rev_mono->size());
        l->n_rev = (uint32_t)(rev_mono->size() + rev->size());
        for (Vec<uint4> *v : {fwd_mono, rev_mono, rev}) l->items.insert(l->items.end(), v->begin(), v->end());
    };
    lay_out(&c.shorts, &short_mono, &short_rev_mono, &short_rev);
    lay_out(&c.mediums, &medium_mono, &medium_rev_mono, &medium_rev);
    c.tiny.mono_lo = (uint32_t)c.tiny.items.size();  // (in path order: a wave takes them as they come)
    c.tiny.mono_n = (uint32_t)tiny_mono.size();
    c.tiny.items.insert(c.tiny.items.end(), tiny_mono.begin(), tiny_mono.end());
    return c;
}

// Paths of equal length -- the ties of the items' sort -- are walked in the order of where they
// start: k_scan's workgroups take the items one after the other, so neighbours in the list go to
// different workgroups, and it is the paths that start near each other that meet in a window.  A
// sub-bucket then holds one path's records of its window, not those of the five or six that
// chance gave one workgroup (the capacity every sub-bucket gets is the fullest one's, §2).
// first[i]: the segment whole[i] starts at.
inline void order_whole_paths(Vec<uint4> *whole, const Vec<uint32_t> &first) {
    Vec<uint32_t> order(whole->size());
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return first[a] < first[b]; });
    Vec<uint4> sorted(whole->size());
    for (size_t i = 0; i < whole->size(); ++i) sorted[i] = (*whole)[order[i]];
    whole->swap(sorted);
}

// ---- the cut and the deals ----
// k_scan's work items: whole paths, except that a path longer than `piece` steps is cut into equal pieces, appended to
// `out`; returns how many paths were cut.  (z: bit 0 = the item walks the ids downwards, set by k_item_dirs; from bit 1
// up, 1 + the ordinal of the split path the item is a piece of, or 0 for a whole path)
inline uint32_t cut_paths(const Vec<uint4> &whole, uint64_t piece, Vec<uint4> *out) {
    uint32_t n_split = 0;
    for (const uint4 &w : whole) {
        const uint64_t b = w.x, n = (uint64_t)w.y - w.x;
        const uint32_t k = (uint32_t)((n + piece - 1) / piece);
        const uint32_t z = k > 1 ? (++n_split) << 1 : 0u;
        for (uint32_t j = 0; j < k; ++j)
            out->push_back(make_uint4((uint32_t)(b + n * j / k), (uint32_t)(b + n * (j + 1) / k), z, w.w));
    }
    return n_split;
}
// ... and the items themselves, longest first (ties as the paths stand); returns the number of split paths
inline uint32_t make_items(const Vec<uint4> &whole, uint64_t piece, Vec<uint4> *items) {
    const uint32_t n_shared = cut_paths(whole, piece ? piece : 32768, items);
    std::stable_sort(items->begin(), items->end(), LongerItem());
    return n_shared;
}

// `n` things dealt one after the other, each to the least loaded hand (the lowest of equals); load[h] and taken[h] are what
// the hands hold before and after.
template <class CostOf>
inline void deal_to_least_loaded(Vec<uint64_t> *load, Vec<uint32_t> *taken, uint64_t first, uint64_t n, CostOf cost_of) {
    using Hand = std::pair<uint64_t, uint32_t>;
    std::priority_queue<Hand, Vec<Hand>, std::greater<Hand>> hands;
    for (uint32_t i = 0; i < load->size(); ++i) hands.push({(*load)[i], i});
    for (uint64_t j = first; j < n; ++j) {
        const uint32_t i = hands.top().second;
        hands.pop();
        (*load)[i] += cost_of(j);
        (*taken)[i] += 1;
        hands.push({(*load)[i], i});
    }
}

// The workgroups take the items, longest first, in a fixed snake order (item_of): with a hundred paths of a million steps
// and pieces of N / (2 CUs), three pieces fall to some workgroups and two to most (+28 % on the
// longest).  So the deal is played through on the host for a few piece sizes, every item charged
// a few blocks' worth for its turnaround, and the size with the shortest longest hand is taken
// (the largest such size: for 1000 paths of 100 k steps, no cutting at all).  0: none.
inline uint64_t choose_piece(const Vec<uint4> &whole, uint32_t n_slots, uint32_t wb, bool keep_cuts) {
    constexpr uint64_t kTurnaround = 8192;  // steps a workgroup could have walked while it changes items
    const uint64_t long_steps = steps_of(whole);
    uint64_t piece = 0, best = ~0ull;
    for (const uint32_t twice_m : {4u, 5u, 6u, 8u, 10u, 12u, 16u, 20u, 24u}) {  // pieces of N / (m CUs), m = 2 .. 12
        uint64_t cand = std::max<uint64_t>(32768, (2 * long_steps + (uint64_t)twice_m * n_slots - 1) / ((uint64_t)twice_m * n_slots));
        cand = (cand + 255) & ~255ull;
        Vec<uint4> trial;
        cut_paths(whole, cand, &trial);
        std::stable_sort(trial.begin(), trial.end(), LongerItem());
        Vec<uint64_t> hand(n_slots, 0);
        for (size_t i = 0; i < trial.size(); ++i) {
            const size_t round = i / n_slots, pos = i % n_slots;
            hand[(round & 1) ? n_slots - 1 - pos : pos] += (uint64_t)(trial[i].y - trial[i].x) + kTurnaround;
        }
        const uint64_t longest = *std::max_element(hand.begin(), hand.end());
        if (longest + longest / 64 < best) {  // smaller pieces have to win by more than 1.5 %
            best = longest;
            piece = cand;
        }
        if (cand == 32768) break;
    }
    // Cutting has a price beyond the turnaround where pass 2 cannot give all split paths a bitset
    // of their own kind -- none at all with 8192-segment windows, 128 with smaller ones: the plan
    // then takes smaller windows, more ranges, or walks the paths in groups (fast_plan_create).  A
    // graph of thousands of paths rarely needs its long ones cut: k_scan's workgroups take the
    // items longest first as they get to them, and if whole paths dealt that way (to the least
    // loaded workgroup each) leave the longest hand within a tenth of the best cut's, they stay whole.
    if (piece && !keep_cuts) {
        Vec<uint4> trial;
        if (cut_paths(whole, piece, &trial) > (wb <= 12 ? kMaxShared : 0u)) {
            Vec<uint64_t> lens, load(n_slots, 0);
            Vec<uint32_t> taken(n_slots, 0u);
            for (const uint4 &w : whole) lens.push_back((uint64_t)w.y - w.x);
            std::sort(lens.begin(), lens.end(), std::greater<uint64_t>());
            deal_to_least_loaded(&load, &taken, 0, lens.size(), [&](uint64_t j) { return lens[j] + kTurnaround; });
            const uint64_t longest = *std::max_element(load.begin(), load.end());
            if (longest <= best + best / 10) piece = ~0ull >> 1;  // (longer than any path)
        }
    }
    return piece;
}

// ---- tagged or not ----
// Tagged calls (records say whose they are; see kTagShift): every workgroup's items -- the handed-back
// ones included -- must have tags of their own next to the split paths', and pass 2 needs LDS for a
// bitset per split path (none to spare with 8192-segment windows; a window shared by several
// workgroups cannot share bitsets).
struct TagIn {
    uint32_t n_slots, wb, acc_parts, max_back, n_shared;
    bool wave_lists;       // some paths are walked by the wave-per-path kernels
    bool dbg;              // the diagnostic build: never tagged
    bool tagged_off;       // FLATGFA_TAGGED=0 keeps the directory (tests, measurements)
    uint32_t limit_asked;  // FLATGFA_TAG_LIMIT: fewer tags (tests); 0 = not set
    bool mean_only;        // FLATGFA_TAG_MEAN_ONLY: the deal is not played through
};
struct TagVerdict {
    bool tagged = false;
    uint32_t tag_limit = 0;
    // what fast_plan_create may do about a plan that is not: walk the paths in groups (fewer items, fewer
    // split paths per group), or take 4096-segment windows (pass 2 then has LDS for split paths' bitsets)
    bool too_many_items = false, want_wb12 = false;
};
inline TagVerdict tag_verdict(const Vec<uint4> &items, const TagIn &in) {
    TagVerdict v;
    const uint32_t n_items = (uint32_t)items.size();
    const uint32_t grid = in.wave_lists ? in.n_slots : std::min<uint32_t>(n_items, in.n_slots);
    const uint64_t per_wg = grid ? ((uint64_t)n_items + in.max_back + grid - 1) / grid : 0;
    const uint32_t shared_cap = in.wb <= 12 ? kMaxShared : 0u;
    const bool base_ok = !in.dbg && !in.tagged_off && (in.n_shared == 0 || in.acc_parts == 1);
    const bool taggable = base_ok && in.n_shared <= shared_cap;
    // A workgroup's private tags: what the split paths leave of the 512.
    // k_scan deals the items out as its workgroups get to them, so it is not the mean that has to
    // fit but the most any workgroup takes: the deal is played through here (its first two items
    // are fixed, every further one goes to whoever is done first), with some room to spare --
    // a workgroup that does run out of tags stops taking items (k_scan) and the others go on.
    uint32_t limit = in.n_shared + 1u < kTagCount ? kTagCount - 1u - in.n_shared : 0u;  // (the highest tag says "no claim")
    if (in.limit_asked) limit = std::min<uint32_t>(limit, std::max(2u, in.limit_asked));
    v.tag_limit = limit;
    uint64_t most = per_wg;
    if (taggable && grid && per_wg <= limit && n_items + in.max_back > 2ull * grid && !in.mean_only) {
        constexpr uint64_t kTurn = 2048;  // steps' worth an item costs beyond its steps
        Vec<uint64_t> load(grid, 0);
        Vec<uint32_t> taken(grid, 0u);
        for (uint32_t i = 0; i < grid; ++i)
            for (uint32_t k = 0; k < 2; ++k)
                if (i + k * grid < n_items) load[i] += (uint64_t)(items[i + k * grid].y - items[i + k * grid].x) + kTurn, taken[i] += 1;
        deal_to_least_loaded(&load, &taken, 2ull * grid, (uint64_t)n_items + in.max_back,
                             [&](uint64_t j) { return (j < n_items ? (uint64_t)(items[j].y - items[j].x) : kShortMax) + kTurn; });
        most = *std::max_element(taken.begin(), taken.end());
        most += most / 4;  // (the workgroups do not run at one speed)
    }
    v.tagged = taggable && per_wg <= limit && most <= limit;
    v.too_many_items = base_ok && !v.tagged && in.acc_parts == 1 && !in.wave_lists && (taggable || (in.wb <= 12 && in.n_shared > shared_cap));
    v.want_wb12 = base_ok && !v.tagged && in.wb == 13 && in.n_shared > 0 && in.acc_parts == 1;
    return v;
}

// ---- pass 2's lists ----
// Pass 2 walks k_scan's items grouped by path (the pieces of a split path share a bitset),
// each of its waves a contiguous stretch of the list: paths are dealt to the waves longest
// first, each to the wave with the least steps so far.
// (the five lists in one slab, for one allocation and one copy, every one on a 256-byte boundary: an allocation and a copy
// each cost a tenth of what the first answer costs)
struct Pass2Lists {
    Vec<uint32_t> slab;
    size_t o_fat_off = 0, o_fat_woff = 0, o_perm = 0, o_elist = 0, o_wave_off = 0;  // words into the slab
    uint32_t n_fat = 0;
};
inline Pass2Lists pass2_lists(const Vec<uint4> &items, uint32_t n_paths, uint32_t acc_parts, bool no_fat) {
    Pass2Lists out;
    const uint32_t n_items = (uint32_t)items.size(), acc_waves = acc_parts * kAccWaves;
    Vec<Vec<uint32_t>> by_path;  // item indices per path that has items
    Vec<uint64_t> path_steps;
    Vec<int64_t> slot_of(n_paths, -1);
    for (uint32_t j = 0; j < n_items; ++j) {
        const uint32_t p = items[j].w;
        if (slot_of[p] < 0) {
            slot_of[p] = (int64_t)by_path.size();
            by_path.emplace_back();
            path_steps.push_back(0);
        }
        by_path[(size_t)slot_of[p]].push_back(j);
        path_steps[(size_t)slot_of[p]] += items[j].y - items[j].x;
    }
    Vec<uint32_t> order(by_path.size());
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return path_steps[a] > path_steps[b]; });
    // A path with more than half a wave's even share of the steps would hold its wave up (four
    // paths of 25 M steps: four waves busy out of sixteen, pass 2 2.6 times slower).  Such
    // paths go to the window's workgroups whole -- to the one with the least so far -- and
    // their pieces to its sixteen waves in turn; the others are dealt to single waves as before.
    uint64_t total_steps = 0;
    for (uint64_t v : path_steps) total_steps += v;
    const uint64_t fat_min = total_steps / (2ull * acc_waves) + 1;
    Vec<Vec<uint32_t>> per_wave(acc_waves), fat_of_part(acc_parts);
    Vec<uint64_t> load(acc_waves, 0), part_load(acc_parts, 0);
    for (uint32_t gi : order) {
        if (path_steps[gi] < fat_min || by_path[gi].size() < kAccWaves / 2 || no_fat) continue;  // (fewer pieces than half the waves: better one wave busy all the time than three)
        const uint32_t q = (uint32_t)(std::min_element(part_load.begin(), part_load.end()) - part_load.begin());
        part_load[q] += path_steps[gi];
        fat_of_part[q].push_back(gi);
    }
    for (uint32_t q = 0; q < acc_parts; ++q)
        for (uint32_t wv = 0; wv < kAccWaves; ++wv) load[q * kAccWaves + wv] = part_load[q] / kAccWaves;
    std::vector<bool> is_fat(by_path.size(), false);
    for (const auto &v : fat_of_part)
        for (uint32_t gi : v) is_fat[gi] = true;
    for (uint32_t gi : order) {
        if (is_fat[gi]) continue;
        const uint32_t wv = (uint32_t)(std::min_element(load.begin(), load.end()) - load.begin());
        load[wv] += path_steps[gi] + 64;
        bool first = true;
        for (uint32_t j : by_path[gi]) {
            per_wave[wv].push_back(j | (first ? 0x80000000u : 0u));
            first = false;
        }
    }
    Vec<uint32_t> elist, wave_off(acc_waves + 1, 0);
    for (uint32_t wv = 0; wv < acc_waves; ++wv) {
        wave_off[wv] = (uint32_t)elist.size();
        elist.insert(elist.end(), per_wave[wv].begin(), per_wave[wv].end());
    }
    wave_off[acc_waves] = (uint32_t)elist.size();
    Vec<uint32_t> fat_off(acc_parts + 1, 0), fat_woff;
    for (uint32_t q = 0; q < acc_parts; ++q) {
        fat_off[q] = out.n_fat;
        for (uint32_t gi : fat_of_part[q]) {
            const Vec<uint32_t> &its = by_path[gi];
            for (uint32_t wv = 0; wv < kAccWaves; ++wv) {
                fat_woff.push_back((uint32_t)elist.size());
                bool first = true;
                for (size_t k = wv; k < its.size(); k += kAccWaves) {
                    elist.push_back(its[k] | (first ? 0x80000000u : 0u));
                    first = false;
                }
            }
            fat_woff.push_back((uint32_t)elist.size());
            out.n_fat += 1;
        }
    }
    fat_off[acc_parts] = out.n_fat;
    // k_scan leaves an item's cursors and sub-bucket at the item's place in this order
    Vec<uint32_t> perm(n_items + 1, 0);
    for (size_t at = 0; at < elist.size(); ++at) perm[elist[at] & 0x7FFFFFFFu] = (uint32_t)at | (elist[at] & 0x80000000u);
    const auto padded = [](size_t words) { return (words + 63) & ~(size_t)63; };
    out.o_fat_off = 0;
    out.o_fat_woff = out.o_fat_off + padded(fat_off.size());
    out.o_perm = out.o_fat_woff + padded(fat_woff.size() + 1);
    out.o_elist = out.o_perm + padded(perm.size());
    out.o_wave_off = out.o_elist + padded(elist.size() + 1);
    out.slab.assign(out.o_wave_off + padded(wave_off.size()), 0u);
    std::copy(fat_off.begin(), fat_off.end(), out.slab.begin() + (ptrdiff_t)out.o_fat_off);
    std::copy(fat_woff.begin(), fat_woff.end(), out.slab.begin() + (ptrdiff_t)out.o_fat_woff);
    std::copy(perm.begin(), perm.end(), out.slab.begin() + (ptrdiff_t)out.o_perm);
    std::copy(elist.begin(), elist.end(), out.slab.begin() + (ptrdiff_t)out.o_elist);
    std::copy(wave_off.begin(), wave_off.end(), out.slab.begin() + (ptrdiff_t)out.o_wave_off);
    return out;
}

// ---- what is known of the items ----
struct ItemFacts {
    unsigned long long records = 0;  // the records k_scan will make of the items (but for window crossings)
    unsigned long long against = 0;  // their steps against the grain (what spoils a window for the per-block no-claim marks)
    uint32_t n_noclaim = 0;
};
// No path cut into pieces, and the counting kernel's facts at hand (`ext`, six words per path: k_count_runs): an item is a
// whole path, and what k_item_dirs would find out about it -- which way it mostly runs, whether it runs strictly one way,
// how many records it makes, how many of its steps go against its grain -- is known.  `claim_all` (FLATGFA_NO_CLAIM=0:
// tests and measurements): every item claims, monotone or not.
inline ItemFacts item_facts_from_ext(Vec<uint4> *items, const Vec<uint32_t> &ext, bool claim_all) {
    ItemFacts f;
    for (uint4 &it : *items) {
        const uint32_t *x = &ext[6 * (size_t)it.w];
        const uint32_t n = it.y - it.x, pairs = n - 1u;  // (an item has at least one step)
        const uint32_t state = (x[0] == pairs ? 1u : 0u) | (x[1] == pairs ? 2u : 0u);
        it.z = (it.z & ~1u) | (x[3] > x[2] ? 1u : 0u);
        if (state && !claim_all) {
            it.z |= kItemNoClaim;
            f.n_noclaim += 1;
        }
        f.records += (unsigned long long)n - std::max(x[2], x[3]);
        f.against += std::min(x[0], x[1]);
    }
    return f;
}
// The pieces of a split path: the path never meets a segment twice when every piece runs strictly one way,
// all of them the same way, and each piece starts beyond (below) where the piece before it ended.  `items` as k_item_dirs
// left them, mono[j] = what it found of item j {1 up / 2 down / 3 a single step / 0 neither, first id, last id, -}.
// True when some items gained kItemNoClaim.
inline bool mark_noclaim_pieces(Vec<uint4> *items, const Vec<uint4> &mono, uint32_t n_shared) {
    Vec<Vec<uint32_t>> pieces(n_shared);
    for (uint32_t j = 0; j < items->size(); ++j) {
        const uint32_t sh = ((*items)[j].z & ~kItemNoClaim) >> 1;
        if (sh) pieces[sh - 1].push_back(j);
    }
    bool any = false;
    for (Vec<uint32_t> &pc : pieces) {
        std::sort(pc.begin(), pc.end(), [&](uint32_t a, uint32_t b) { return (*items)[a].x < (*items)[b].x; });
        uint32_t way = 3u;  // the ways all pieces so far can be read: 1 upwards, 2 downwards
        for (size_t k = 0; k < pc.size() && way; ++k) {
            way &= mono[pc[k]].x;
            if (k) {
                const uint32_t last = mono[pc[k - 1]].z, first = mono[pc[k]].y;
                way &= (first > last ? 1u : 0u) | (first < last ? 2u : 0u);
            }
        }
        if (way && !pc.empty()) {
            for (uint32_t j : pc) (*items)[j].z |= kItemNoClaim;
            any = true;
        }
    }
    return any;
}

// ---- packed buckets ----
// Every (window, workgroup) sub-bucket with the room its records need -- cnt[w * n_slots + g], the counting call's cursors --
// a workgroup's sub-buckets back to back, a 64-record sink behind each workgroup's region.
struct PackedLayout {
    Vec<uint32_t> off;   // [n_slots][n_win + 1] sub-bucket starts within the region; the last entry is its sink
    Vec<uint64_t> base;  // [n_slots] where each region starts
    Vec<uint2> pk;       // [n_win][n_slots] {start in the array, room}
    uint64_t total = 0, deepest = 0;
    bool fits = true;    // false: the even layout, if it can be had, with `cap` records per sub-bucket
    uint64_t cap = 0;
};
// `countable`: the counting call's queues held (blocks without any runs do not fit a packed call's: the even layout).
// `ask_first`: the call was only asked how deep the deepest sub-bucket is; an even layout with headroom -- three times that
// for every sub-bucket: a call deals the items as they come, so its fullest sub-bucket is not the counted one, and what ends
// up more than half full is doubled (flatgfa_dev_plan_create; twice the deepest was kept even, doubled there, and made again
// packed after all) -- that stays within even_limit bytes is kept: its k_scan keeps one table less in LDS.
inline PackedLayout packed_layout(const Vec<uint32_t> &cnt, uint32_t n_win, uint32_t n_slots, bool countable, bool ask_first, uint64_t even_limit,
                                  uint64_t cap) {
    PackedLayout l;
    const size_t row = (size_t)n_win + 1;
    const uint64_t slots = (uint64_t)n_win * n_slots;
    l.off.resize(row * n_slots);
    l.base.resize(n_slots);
    l.pk.resize(slots);
    l.cap = cap;
    for (uint32_t gq = 0; gq < n_slots; ++gq) {
        uint64_t o = 0;
        l.base[gq] = l.total;
        for (uint32_t wq = 0; wq < n_win; ++wq) {
            const uint64_t room = ((uint64_t)cnt[(size_t)wq * n_slots + gq] + 3) & ~3ull;  // (sub-buckets start on 16 bytes: pass 2 reads four records at a time)
            l.off[gq * row + wq] = (uint32_t)o;
            l.pk[(size_t)wq * n_slots + gq] = make_uint2((uint32_t)(l.total + o), (uint32_t)room);
            l.deepest = std::max(l.deepest, room);
            o += room;
        }
        l.off[gq * row + n_win] = (uint32_t)o;  // the region's sink
        o += 64;
        l.fits = l.fits && o < (1ull << 30);    // (a region's byte offsets take 32 bits)
        l.total += o;
    }
    l.fits = l.fits && countable && l.total < (1ull << 32);
    if (l.fits && ask_first && (slots + n_slots) * std::max<uint64_t>(3 * l.deepest, 4) * 4 <= even_limit) {
        l.fits = false;
        l.cap = std::max<uint64_t>(cap, 3 * l.deepest);
    }
    return l;
}

}  // namespace fgfa_dev
