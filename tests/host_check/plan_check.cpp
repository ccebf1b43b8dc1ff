// The host stages of the bucketed depth plan (pollen_amd/csrc/depth_plan_host.hpp) on their own, without a GPU: what the
// kernels rely on -- every item once in pass 2's list, `perm` its inverse, sub-buckets on 16 bytes, regions disjoint, the
// wave-per-path lists laid out as their kernels read them -- asserted at the smallest shapes that reach each branch.
// Built twice by `make -C pollen_amd/csrc plan_check plan_check_asan`; tests/test_host_sanitized_plan.py runs both.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>

#include "depth_plan_host.hpp"

using namespace fgfa_dev;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

// whole paths of the given lengths, one behind the other from step 0
static Vec<uint4> paths_of(const std::vector<uint32_t> &lens) {
    Vec<uint4> whole;
    uint32_t at = 0;
    for (uint32_t p = 0; p < lens.size(); ++p) {
        whole.push_back(make_uint4(at, at + lens[p], kNoSlot, p));
        at += lens[p];
    }
    return whole;
}

static void check_cut() {
    const std::vector<uint32_t> lens{1, 255, 256, 257, 513, 769};
    const uint64_t piece = 256;
    const Vec<uint4> whole = paths_of(lens);
    Vec<uint4> cut;
    const uint32_t n_split = cut_paths(whole, piece, &cut);
    CHECK(n_split == 3);
    size_t at = 0;
    uint32_t split = 0;
    for (const uint4 &w : whole) {
        const uint32_t n = w.y - w.x, k = (uint32_t)((n + piece - 1) / piece);
        const uint32_t z = k > 1 ? (++split) << 1 : 0u;
        uint32_t pos = w.x;
        for (uint32_t j = 0; j < k; ++j, ++at) {
            CHECK(at < cut.size());
            const uint4 &it = cut[at];
            CHECK(it.x == pos && it.y > it.x && it.y - it.x <= piece);  // non-empty, contiguous, no longer than a piece
            CHECK(it.z == z && it.w == w.w);
            pos = it.y;
        }
        CHECK(pos == w.y);  // [b, e) exactly
    }
    CHECK(at == cut.size() && split == n_split);
    // the item list: longest first, ties as the cut left them
    Vec<uint4> items;
    CHECK(make_items(whole, piece, &items) == n_split && items.size() == cut.size());
    std::map<std::pair<uint32_t, uint32_t>, size_t> place;
    for (size_t i = 0; i < cut.size(); ++i) place[{cut[i].x, cut[i].y}] = i;
    for (size_t i = 0; i < items.size(); ++i) {
        CHECK(place.count({items[i].x, items[i].y}) == 1);
        if (!i) continue;
        const uint32_t a = items[i - 1].y - items[i - 1].x, b = items[i].y - items[i].x;
        CHECK(a >= b);
        if (a == b) CHECK((place[{items[i - 1].x, items[i - 1].y}] < place[{items[i].x, items[i].y}]));
    }
    // piece 0: the default, nothing here is that long
    Vec<uint4> uncut;
    CHECK(make_items(whole, 0, &uncut) == 0 && uncut.size() == whole.size());
    // the piece chosen: a multiple of 256 steps of at least 32768, or longer than any path
    for (const uint32_t wb : {12u, 13u}) {
        const uint64_t chosen = choose_piece(paths_of(std::vector<uint32_t>(300, 100000u)), 256, wb, false);
        CHECK(chosen == ~0ull >> 1 || (chosen >= 32768 && chosen % 256 == 0));
        std::printf("cut: 300 paths of 100000 steps, 256 workgroups, wb %u: piece %llu\n", wb, (unsigned long long)chosen);
    }
    std::printf("cut ok: %zu items of %zu paths\n", items.size(), whole.size());
}

struct PathCase {
    uint32_t len, runs, runs_down, mono;
    char list;  // t tiny, s short, m medium, w whole, - none
    bool rev;
};
static void check_wave_list(const WaveList &l, char name, const std::vector<PathCase> &cases, const PathClasses &c, std::set<uint32_t> *seen) {
    CHECK(l.mono_lo + l.mono_n <= l.items.size() && l.n_rev <= l.items.size());
    std::map<uint32_t, uint4> copy_of;
    for (const uint4 &r : c.rev_list) copy_of[r.w] = r;
    const size_t rev_lo = l.items.size() - l.n_rev;
    CHECK(l.mono_lo <= rev_lo || l.mono_n == 0);
    for (size_t i = 0; i < l.items.size(); ++i) {
        const uint4 &it = l.items[i];
        const PathCase &pc = cases[it.w];
        CHECK(seen->insert(it.w).second);  // a path is in one list, once
        CHECK(pc.list == name && it.z == kNoSlot && it.y - it.x == pc.len);
        const bool rev = i >= rev_lo, mono = i >= l.mono_lo && i < l.mono_lo + l.mono_n;
        CHECK(rev == pc.rev && mono == (pc.mono != 0));  // [claim][mono | mono reversed][claim reversed]
        if (rev) CHECK(copy_of.count(it.w) == 1 && copy_of[it.w].z == it.x && copy_of[it.w].y - copy_of[it.w].x == pc.len);
        else CHECK(copy_of.count(it.w) == 0);
        // each of the four parts longest first
        if (i && name != 't' && (i - 1 >= rev_lo) == rev && (i - 1 >= l.mono_lo && i - 1 < l.mono_lo + l.mono_n) == mono)
            CHECK(l.items[i - 1].y - l.items[i - 1].x >= it.y - it.x);
    }
}
static void check_classes() {
    const uint32_t q = kQCap - 16;
    std::vector<PathCase> cases{
        {kTinyMax, 3, 3, 0, 't', false},           {kTinyMax, 3, 3, 1, 't', false},          {kTinyMax + 1, 3, 3, 0, 's', false},
        {kShortMax, q, q, 0, 's', false},          {kShortMax, q + 1, q + 1, 0, 'm', false}, {kShortMax + 1, kMediumRuns, kMediumRuns, 0, 'm', false},
        {kShortMax + 1, kMediumRuns + 1, kMediumRuns + 1, 0, 'w', false},                    {kShortMax, 9, 9, 1, 's', false},
        {900, 50, 4, 0, 's', true},                {1000, 50, 4, 1, 's', true},              {700, 50, 4, 0, 's', true},
        {5000, 900, 800, 0, 'm', true},            {5001, 900, 800, 1, 'm', true},           {4000, 10, 10, 1, 'm', false},
        {0, 0, 0, 0, '-', false},                  {300, q + 1, q, 0, 's', true},            {kShortMax + 7, kMediumRuns + 2, kMediumRuns + 1, 0, 'w', false},
        {133, 5, 5, 0, 'w', false},  // the pool's last path: its last block would reach past the pool
    };
    std::vector<uint32_t> hb, he, runs, runs_down, mono;
    uint32_t at = 0;
    for (const PathCase &pc : cases) {
        hb.push_back(at);
        he.push_back(at += pc.len);
        runs.push_back(pc.runs), runs_down.push_back(pc.runs_down), mono.push_back(pc.mono);
    }
    const uint64_t n_steps = at;
    CHECK(n_steps % 16 != 0);
    // ... and the same span again, read reversed: within reach
    cases.push_back({133, 5, 4, 0, 's', true});
    hb.push_back(hb.back()), he.push_back(he.back()), runs.push_back(5), runs_down.push_back(4), mono.push_back(0);
    const uint32_t np = (uint32_t)cases.size();
    const PathClasses c = classify_paths({hb.data(), he.data(), np, n_steps, kShortMax, runs.data(), runs_down.data(), mono.data(), false, false, false});
    std::set<uint32_t> seen;
    check_wave_list(c.tiny, 't', cases, c, &seen);
    check_wave_list(c.shorts, 's', cases, c, &seen);
    check_wave_list(c.mediums, 'm', cases, c, &seen);
    CHECK(c.tiny.n_rev == 0);
    for (const uint4 &w : c.whole) {
        CHECK(seen.insert(w.w).second && cases[w.w].list == 'w' && w.x == hb[w.w] && w.y == he[w.w] && w.z == kNoSlot);
    }
    for (uint32_t p = 0; p < np; ++p) CHECK(seen.count(p) == (cases[p].list != '-'));
    // reversed copies: at multiples of 16, one behind the other
    uint64_t end = 0;
    for (const uint4 &r : c.rev_list) {
        CHECK(r.z % 16 == 0 && r.z >= end && r.x == hb[r.w] && r.y == he[r.w] && cases[r.w].rev);
        end = (uint64_t)r.z + (r.y - r.x);
    }
    CHECK(c.rev_len >= end && c.rev_len % 16 == 0);
    // the hooks: any run count is short (FLATGFA_SHORT_ANY), no tiny list, no reversed copies
    const PathClasses any = classify_paths({hb.data(), he.data(), np, n_steps, kShortMax, runs.data(), runs_down.data(), mono.data(), true, false, false});
    CHECK(any.shorts.items.size() == c.shorts.items.size() + 1);  // (the path of kQCap - 15 runs)
    const PathClasses no_tiny = classify_paths({hb.data(), he.data(), np, n_steps, kShortMax, runs.data(), runs_down.data(), mono.data(), false, false, true});
    CHECK(no_tiny.tiny.items.empty() && no_tiny.shorts.items.size() == c.shorts.items.size() + c.tiny.items.size());
    const PathClasses no_rev = classify_paths({hb.data(), he.data(), np, n_steps, kShortMax, runs.data(), runs_down.data(), mono.data(), false, true, false});
    CHECK(no_rev.rev_list.empty() && no_rev.rev_len == 0 && no_rev.shorts.n_rev == 0 && no_rev.mediums.n_rev == 0);
    // short_max 0: everything is k_scan's, and the run counts are not looked at
    const PathClasses none = classify_paths({hb.data(), he.data(), np, n_steps, 0, nullptr, nullptr, nullptr, false, false, false});
    CHECK(none.whole.size() == np - 1 && none.tiny.items.empty() && none.shorts.items.empty() && none.mediums.items.empty() && none.rev_list.empty());
    // the order of whole paths: by first id, ties as they stood
    Vec<uint4> whole = paths_of({10, 10, 10, 10});
    order_whole_paths(&whole, Vec<uint32_t>{7u, 3u, 7u, 1u});
    CHECK(whole[0].w == 3 && whole[1].w == 1 && whole[2].w == 0 && whole[3].w == 2);
    std::printf("classes ok: %zu tiny, %zu short (%u reversed, %u mono), %zu medium (%u reversed, %u mono), %zu whole, %llu reversed steps\n", c.tiny.items.size(),
                c.shorts.items.size(), c.shorts.n_rev, c.shorts.mono_n, c.mediums.items.size(), c.mediums.n_rev, c.mediums.mono_n, c.whole.size(),
                (unsigned long long)c.rev_len);
}

static void check_tags() {
    const auto items_of = [](uint32_t n, uint32_t len) {
        Vec<uint4> items;
        for (uint32_t j = 0; j < n; ++j) items.push_back(make_uint4(j * len, (j + 1) * len, 0u, j));
        return items;
    };
    TagIn in{256, 12, 1, 0, kMaxShared, false, false, false, 0, false};
    // split paths: as many as pass 2 has shared bitsets for, and one more
    TagVerdict v = tag_verdict(items_of(2 * kMaxShared, 1000), in);
    CHECK(v.tagged && !v.too_many_items && !v.want_wb12 && v.tag_limit == kTagCount - 1 - kMaxShared);
    in.n_shared = kMaxShared + 1;
    v = tag_verdict(items_of(2 * in.n_shared, 1000), in);
    CHECK(!v.tagged && v.too_many_items && !v.want_wb12);
    // 8192-segment windows have no LDS for any: the plan asks for 4096-segment ones
    in.n_shared = 1, in.wb = 13;
    v = tag_verdict(items_of(2, 1000), in);
    CHECK(!v.tagged && v.want_wb12 && !v.too_many_items);
    in.n_shared = 0;
    CHECK(tag_verdict(items_of(2, 1000), in).tagged);
    // a window's workgroups cannot share a split path's bitset
    in = TagIn{256, 12, 2, 0, 1, false, false, false, 0, false};
    v = tag_verdict(items_of(2, 1000), in);
    CHECK(!v.tagged && !v.too_many_items && !v.want_wb12);
    in.n_shared = 0;
    CHECK(tag_verdict(items_of(2, 1000), in).tagged);
    // items per workgroup at the tag limit and one past it: the mean alone ...
    in = TagIn{8, 12, 1, 0, 0, false, false, false, 4, true};
    v = tag_verdict(items_of(32, 1000), in);
    CHECK(v.tagged && v.tag_limit == 4);
    v = tag_verdict(items_of(33, 1000), in);
    CHECK(!v.tagged && v.too_many_items);
    // ... and the deal played through, a quarter on top of the most any workgroup takes
    in.mean_only = false, in.limit_asked = 5;
    CHECK(tag_verdict(items_of(32, 1000), in).tagged);   // four each: 4 + 1
    CHECK(!tag_verdict(items_of(40, 1000), in).tagged);  // five each: 5 + 1
    // handed-back paths take tags too; the other switches
    in = TagIn{8, 12, 1, 8, 0, true, false, false, 4, true};
    CHECK(tag_verdict(items_of(24, 1000), in).tagged && !tag_verdict(items_of(25, 1000), in).tagged);
    CHECK(!tag_verdict(items_of(25, 1000), in).too_many_items);  // (the wave-per-path lists stand in the way of path groups)
    in.tagged_off = true;
    CHECK(!tag_verdict(items_of(8, 1000), in).tagged);
    in.tagged_off = false, in.dbg = true;
    CHECK(!tag_verdict(items_of(8, 1000), in).tagged);
    // the one deal helper: each to the least loaded hand, the lowest of equals
    Vec<uint64_t> load(3, 0);
    Vec<uint32_t> taken(3, 0u);
    const uint64_t cost[5] = {5, 3, 3, 1, 4};
    deal_to_least_loaded(&load, &taken, 0, 5, [&](uint64_t j) { return cost[j]; });
    CHECK(load[0] == 5 && load[1] == 3 + 1 && load[2] == 3 + 4 && taken[0] == 1 && taken[1] == 2 && taken[2] == 2);
    std::printf("tags ok\n");
}

static void check_lists(const Vec<uint4> &whole, uint64_t piece, uint32_t acc_parts, uint32_t want_fat) {
    Vec<uint4> items;
    make_items(whole, piece, &items);
    const uint32_t n_items = (uint32_t)items.size(), n_paths = (uint32_t)whole.size(), acc_waves = acc_parts * kAccWaves;
    const Pass2Lists l = pass2_lists(items, n_paths, acc_parts, false);
    CHECK(l.n_fat == want_fat);
    // the five lists: on 64 words, one behind the other
    const size_t offs[6] = {l.o_fat_off, l.o_fat_woff, l.o_perm, l.o_elist, l.o_wave_off, l.slab.size()};
    const size_t lens[5] = {acc_parts + 1, (size_t)17 * l.n_fat, (size_t)n_items + 1, n_items, acc_waves + 1};
    for (int k = 0; k < 5; ++k) CHECK(offs[k] % 64 == 0 && offs[k] + lens[k] <= offs[k + 1]);
    const uint32_t *fat_off = &l.slab[l.o_fat_off], *fat_woff = &l.slab[l.o_fat_woff], *perm = &l.slab[l.o_perm], *elist = &l.slab[l.o_elist],
                   *wave_off = &l.slab[l.o_wave_off];
    std::vector<uint32_t> times(n_items, 0);
    for (uint32_t at = 0; at < n_items; ++at) {
        const uint32_t j = elist[at] & 0x7FFFFFFFu;
        CHECK(j < n_items);
        times[j] += 1;
        CHECK(perm[j] == (at | (elist[at] & 0x80000000u)));
    }
    for (uint32_t j = 0; j < n_items; ++j) CHECK(times[j] == 1);
    // the waves' stretches: a path's items together, the first of them flagged
    std::set<uint32_t> paths_seen;
    for (uint32_t wv = 0; wv < acc_waves; ++wv) {
        CHECK(wave_off[wv] <= wave_off[wv + 1] && wave_off[wv + 1] <= n_items);
        for (uint32_t at = wave_off[wv]; at < wave_off[wv + 1]; ++at) {
            const uint32_t p = items[elist[at] & 0x7FFFFFFFu].w;
            if (elist[at] >> 31) CHECK(paths_seen.insert(p).second);
            else CHECK(at > wave_off[wv] && items[elist[at - 1] & 0x7FFFFFFFu].w == p);
        }
    }
    CHECK(wave_off[0] == 0);
    // fat paths: behind the waves' stretches, 17 offsets each, the pieces to the sixteen waves in turn
    uint32_t at = wave_off[acc_waves];
    for (uint32_t q = 0; q < acc_parts; ++q) CHECK(fat_off[q] <= fat_off[q + 1]);
    CHECK(fat_off[0] == 0 && fat_off[acc_parts] == l.n_fat);
    for (uint32_t f = 0; f < l.n_fat; ++f) {
        const uint32_t *w = fat_woff + 17 * f;
        CHECK(w[0] == at && w[0] < w[1]);
        const uint32_t p = items[elist[w[0]] & 0x7FFFFFFFu].w;
        CHECK(paths_seen.insert(p).second);
        std::vector<uint32_t> its;
        for (uint32_t j = 0; j < n_items; ++j)
            if (items[j].w == p) its.push_back(j);
        CHECK(its.size() >= kAccWaves / 2);
        for (uint32_t wv = 0; wv < kAccWaves; ++wv) {
            size_t k = wv;
            for (uint32_t i = w[wv]; i < w[wv + 1]; ++i, k += kAccWaves) CHECK(k < its.size() && elist[i] == (its[k] | (i == w[wv] ? 0x80000000u : 0u)));
            CHECK(k >= its.size());
        }
        at = w[kAccWaves];
    }
    CHECK(at == n_items);
    std::printf("lists ok: %u items of %u paths, %u workgroups per window, %u fat\n", n_items, n_paths, acc_parts, l.n_fat);
}

static void check_layout() {
    const uint32_t n_win = 3, n_slots = 8;
    const size_t row = n_win + 1;
    Vec<uint32_t> cnt((size_t)n_win * n_slots);
    for (uint32_t w = 0; w < n_win; ++w)
        for (uint32_t g = 0; g < n_slots; ++g) cnt[(size_t)w * n_slots + g] = (w * 7 + g * 3) % 11;
    PackedLayout l = packed_layout(cnt, n_win, n_slots, true, false, 0, 300);
    CHECK(l.fits && l.cap == 300);
    uint64_t end = 0, deepest = 0;
    for (uint32_t g = 0; g < n_slots; ++g) {
        CHECK(l.base[g] == end && l.off[g * row] == 0);
        for (uint32_t w = 0; w < n_win; ++w) {
            const uint2 pk = l.pk[(size_t)w * n_slots + g];
            CHECK(pk.y % 4 == 0 && pk.y >= cnt[(size_t)w * n_slots + g] && pk.y < cnt[(size_t)w * n_slots + g] + 4);
            CHECK(pk.x == l.base[g] + l.off[g * row + w] && pk.x % 4 == 0);
            CHECK(l.off[g * row + w + 1] == l.off[g * row + w] + pk.y);  // back to back; the last entry is the sink
            deepest = std::max<uint64_t>(deepest, pk.y);
        }
        end = l.base[g] + l.off[g * row + n_win] + 64;  // (a 64-record sink behind the region)
    }
    CHECK(l.total == end && l.deepest == deepest);
    CHECK(!packed_layout(cnt, n_win, n_slots, false, false, 0, 300).fits);  // (the counting call's queues did not hold)
    // asked first: the even layout is kept exactly when three times the deepest fits the limit, and takes that capacity
    const uint64_t even = ((uint64_t)n_win * n_slots + n_slots) * 3 * deepest * 4;
    l = packed_layout(cnt, n_win, n_slots, true, true, even, 7);
    CHECK(!l.fits && l.cap == 3 * deepest);
    l = packed_layout(cnt, n_win, n_slots, true, true, even, 1000);
    CHECK(!l.fits && l.cap == 1000);
    l = packed_layout(cnt, n_win, n_slots, true, true, even - 1, 7);
    CHECK(l.fits && l.cap == 7);
    // a region of 2^30 records; a total of 2^32
    Vec<uint32_t> one(n_slots, 0u);
    one[5] = 1u << 30;
    CHECK(!packed_layout(one, 1, n_slots, true, false, 0, 4).fits);
    one[5] = (1u << 30) - 128;
    CHECK(packed_layout(one, 1, n_slots, true, false, 0, 4).fits);
    const PackedLayout big = packed_layout(Vec<uint32_t>(n_slots, 1u << 29), 1, n_slots, true, false, 0, 4);
    CHECK(!big.fits && big.total >= 1ull << 32);
    CHECK(packed_layout(Vec<uint32_t>(n_slots - 1, 1u << 29), 1, n_slots - 1, true, false, 0, 4).fits);
    std::printf("layout ok: %llu records, deepest %llu\n", (unsigned long long)end, (unsigned long long)deepest);
}

static void check_item_facts() {
    // ext per path: {ascents, descents, steps that follow upwards, downwards, first id, last id}
    const Vec<uint32_t> ext{9, 0, 9, 0, 1, 10, /**/ 0, 9, 0, 9, 10, 1, /**/ 5, 4, 3, 2, 1, 4, /**/ 0, 0, 0, 0, 7, 7, /**/ 9, 0, 2, 0, 1, 30};
    const auto fresh = [] {
        Vec<uint4> items = paths_of({10, 10, 10, 1, 10});
        for (uint4 &it : items) it.z = 0;
        return items;
    };
    Vec<uint4> items = fresh();
    ItemFacts f = item_facts_from_ext(&items, ext, false);
    CHECK(items[0].z == kItemNoClaim && items[1].z == (kItemNoClaim | 1u) && items[2].z == 0 && items[3].z == kItemNoClaim && items[4].z == kItemNoClaim);
    CHECK(f.n_noclaim == 4 && f.records == 1 + 1 + 7 + 1 + 8 && f.against == 4);
    items = fresh();
    f = item_facts_from_ext(&items, ext, true);  // every item claims
    CHECK(items[0].z == 0 && items[1].z == 1u && items[2].z == 0 && items[3].z == 0 && items[4].z == 0);
    CHECK(f.n_noclaim == 0 && f.records == 18 && f.against == 4);
    // the pieces of split paths: 1 = up and onwards, 2 = up but the second piece starts where the first ended, 3 = down and onwards, 4 = one piece turns
    Vec<uint4> pieces;
    for (uint32_t k = 1; k <= 4; ++k)
        for (uint32_t j = 0; j < 2; ++j) pieces.push_back(make_uint4((2 * k + j) * 100, (2 * k + j + 1) * 100, k << 1, k));
    pieces.push_back(make_uint4(0, 50, 0, 0));  // a whole path, as the kernel marked it
    pieces.back().z |= kItemNoClaim;
    const Vec<uint4> mono{make_uint4(1, 10, 20, 0), make_uint4(1, 21, 30, 0), make_uint4(1, 10, 20, 0), make_uint4(1, 20, 30, 0),
                          make_uint4(2, 90, 80, 0), make_uint4(2, 79, 60, 0), make_uint4(1, 10, 20, 0), make_uint4(0, 21, 30, 0), make_uint4(1, 1, 9, 0)};
    CHECK(mark_noclaim_pieces(&pieces, mono, 4));
    const bool want[9] = {true, true, false, false, true, true, false, false, true};
    for (int j = 0; j < 9; ++j) CHECK((pieces[j].z >> 31 != 0) == want[j]);
    Vec<uint4> none(pieces.begin() + 2, pieces.begin() + 4);
    none[0].z = none[1].z = 1u << 1;
    CHECK(!mark_noclaim_pieces(&none, Vec<uint4>(mono.begin() + 2, mono.begin() + 4), 1));
    std::printf("item facts ok\n");
}

int main() {
    check_cut();
    check_classes();
    check_tags();
    std::vector<uint32_t> plain, fat{16000};
    for (uint32_t i = 0; i < 40; ++i) plain.push_back(100 + 7 * (i % 9));
    for (uint32_t i = 0; i < 10; ++i) fat.push_back(50 + i);
    for (const uint32_t acc_parts : {1u, 2u}) {
        check_lists(paths_of(plain), 0, acc_parts, 0);
        check_lists(paths_of(fat), 1000, acc_parts, 1);   // one path in sixteen pieces, nearly all the steps
        check_lists(paths_of(fat), 2500, acc_parts, 0);   // in seven: fewer than half the waves
        check_lists(paths_of({769, 513, 257, 1}), 256, acc_parts, 0);
    }
    check_layout();
    check_item_facts();
    std::printf("all ok\n");
    return 0;
}
