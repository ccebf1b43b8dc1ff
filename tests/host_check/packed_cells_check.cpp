// The packed cells of the sweep over the sorted record image (pollen_amd/csrc/depth_sorted_host.hpp: sorted_pack, sorted_unpack,
// sorted_record_packed, sorted_cells_fit, sorted_cells_choice -- the text k_accum_sorted runs), without a GPU: a cell holds the
// depth difference in its low half and the revisit difference in its high half, mod 2^32.  Here: that packing and unpacking
// agree wherever both halves stay inside 16 signed bits; what the rule says at its edge; a host model of the packed sweep --
// the finaliser's image, swept group by group in shuffled order, the group with the window's last chunk through the build that
// checks for padding -- against brute force with a visited set per path; and, by brute force over the same records, the bounds
// the rule rests on: |dD[c]| <= max(starts(c), ends(c)) and |dR[c]| <= max(starts(c), 2 ends(c)).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#include "depth_sorted_host.hpp"

using namespace fgfa_dev;

#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #c); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

static int check_round_trip() {
    const int32_t top = (1 << 15) - 1;
    const int32_t edge[] = {-top, -top + 1, -2, -1, 0, 1, 2, top - 1, top};
    unsigned n = 0;
    for (int32_t d : edge)
        for (int32_t r : edge) {  // (every sign of one half under every sign of the other: the borrow out of a negative low half)
            int32_t dd = 12345, dr = 12345;
            sorted_unpack(sorted_pack(d, r), dd, dr);
            CHECK(dd == d && dr == r);
            ++n;
        }
    // ... and as the sweep makes a cell: one add after the other, mod 2^32, in any order
    std::mt19937 rng(99);
    for (int round = 0; round < 2000; ++round) {
        const int32_t d = (int32_t)(rng() % (2u * top + 1u)) - top, r = (int32_t)(rng() % (2u * top + 1u)) - top;
        uint32_t w = 0;
        int32_t dl = d, rl = r;
        while (dl || rl) {
            const bool hit = rl > 0, back = rl < 0, up = dl > 0, down = dl < 0;
            switch (rng() % 3) {
            case 0:
                if (up) w += sorted_pack_start(hit), --dl, rl -= hit;
                break;
            case 1:
                if (down) w -= sorted_pack_end(back), ++dl, rl += back;
                break;
            default:
                if (back) w -= kSortedPackRevisit, ++rl;
                else if (hit && !up) w += kSortedPackRevisit, --rl;  // (what a start adds beyond the depth's one, on its own)
            }
        }
        int32_t dd, dr;
        sorted_unpack(w, dd, dr);
        CHECK(dd == d && dr == r);
    }
    printf("round trip ok: %u edge pairs, 2000 random cells\n", n);
    return 0;
}

static int check_rule() {
    const uint32_t lim = 1u << 14;
    CHECK(kSortedPackLimit == lim);
    CHECK(sorted_cells_fit(lim - 1u, lim - 1u) && sorted_cells_fit(1u, 0u) && sorted_cells_fit(lim - 1u, 1u));
    CHECK(!sorted_cells_fit(lim, 1u) && !sorted_cells_fit(1u, lim) && !sorted_cells_fit(lim, lim) && !sorted_cells_fit(~0u, 1u));
    CHECK(!sorted_cells_fit(0u, 0u));  // (no maximum: not known)
    // the bounds the rule gives stay inside a half: max(starts, 2 ends) < 2^15
    CHECK(std::max(lim - 1u, 2u * (lim - 1u)) < (1u << 15));
    // the hook: `packed` never overrides the rule, `wide` always holds
    CHECK(sorted_cells_choice(-1, lim - 1u, lim - 1u) == kSortedCellsPacked && sorted_cells_choice(1, lim - 1u, lim - 1u) == kSortedCellsPacked);
    CHECK(sorted_cells_choice(0, 5u, 5u) == kSortedCellsWideHook);
    CHECK(sorted_cells_choice(-1, lim, 5u) == kSortedCellsWideRule && sorted_cells_choice(1, lim, 5u) == kSortedCellsWideRule && sorted_cells_choice(1, 5u, lim) == kSortedCellsWideRule);
    CHECK(sorted_cells_choice(-1, 0u, 0u) == kSortedCellsUnknown && sorted_cells_choice(1, 0u, 0u) == kSortedCellsUnknown);
    CHECK(kSortedCellsUnknown == 0u);  // (a plan that never heard of the bound sweeps wide cells)
    printf("rule ok\n");
    return 0;
}

struct Rec {
    uint32_t path, s, e;  // [s, e) inside one window
};
struct Window {
    std::vector<uint32_t> rec, carry;
};
// sorted_image_finalise, one window: records sorted by path, then start
static Window finalise(const std::vector<Rec> &sorted, uint32_t wb) {
    Window w;
    const size_t nc = (sorted.size() + kSortedChunk - 1) / kSortedChunk;
    w.rec.assign(nc * kSortedChunk, kSortedPad);
    w.carry.assign(nc, 0u);
    uint32_t m = 0, ord = 0;
    for (size_t i = 0; i < sorted.size(); ++i) {
        const bool first = i == 0 || sorted[i].path != sorted[i - 1].path;
        if (i % kSortedChunk == 0) ord = 0;
        if (first) m = 0, ++ord;
        if (i % kSortedChunk == 0) w.carry[i / kSortedChunk] = first ? 0u : m;
        w.rec[i] = sorted[i].s | ((sorted[i].e - sorted[i].s - 1u) << wb) | (first ? kSortedFirst : 0u) | (ord << kSortedOrdShift);
        m = std::max(m, sorted[i].e);
    }
    return w;
}

// k_accum_sorted's packed sweep of one group, the wave's lanes one after the other; how many third adds it made
template <bool CHECKED>
static void sweep_group(const Window &w, size_t g, uint32_t wb, std::vector<uint32_t> &W, unsigned long long &adds) {
    const size_t nc = w.carry.size();
    uint32_t before = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint32_t q = lane >> 4;
        const size_t ck = g * kSortedGroup + q;
        const bool in = ck < nc;
        const size_t at = std::min((g * kSortedGroup) * kSortedChunk + (size_t)lane * kSortedGroup, nc * kSortedChunk - kSortedGroup);
        const uint32_t carry = w.carry[std::min(ck, nc - 1)];
        const uint32_t pad = CHECKED && !in ? kSortedPad : 0u;
        const uint32_t rec[kSortedGroup] = {w.rec[at] | pad, w.rec[at + 1] | pad, w.rec[at + 2] | pad, w.rec[at + 3] | pad};
        const uint32_t seed = CHECKED && !in ? 0u : sorted_seed(q, carry);
        SortedLane ln;
        sorted_lane_keys<CHECKED>(rec, q, wb, seed, ln);
        uint32_t p = sorted_umax(seed, before);
        for (uint32_t k = 0; k < kSortedGroup; ++k)
            sorted_record_packed<CHECKED>(p, ln.s[k], ln.len[k], ln.x[k], [&](uint32_t cell, uint32_t v) {
                W.at(cell) += v;
                ++adds;
            });
        before = sorted_umax(before, ln.t);
    }
}

static unsigned long long g_adds = 0, g_records = 0;

static int check_one(std::vector<Rec> recs, uint32_t n_paths, uint32_t wb, std::mt19937 &rng, bool must_fit = true) {
    const uint32_t Wn = 1u << wb;
    const SortedKey k = sorted_key(wb, n_paths, 1);
    std::stable_sort(recs.begin(), recs.end(), [&](const Rec &a, const Rec &b) { return k.pack(0, a.path, a.s) < k.pack(0, b.path, b.s); });
    // brute force: counts with a visited set per path (the records are grouped by path: one array of stamps), and the cells'
    // differences -- dD from the records' two ends, dR as the difference of the revisit counts of neighbouring cells
    std::vector<uint32_t> depth(Wn + 1, 0), revisits(Wn + 1, 0), seen(Wn, 0), starts(Wn + 1, 0), ends(Wn + 1, 0);
    for (const Rec &r : recs) {
        ++starts[r.s];
        ++ends[r.e];
        for (uint32_t i = r.s; i < r.e; ++i) {
            ++depth[i];
            if (seen[i] == r.path + 1u) ++revisits[i];
            seen[i] = r.path + 1u;
        }
    }
    const uint32_t ms = *std::max_element(starts.begin(), starts.end()), me = *std::max_element(ends.begin(), ends.end());
    if (recs.empty()) return 0;
    CHECK(!must_fit || sorted_cells_fit(ms, me));
    const Window w = finalise(recs, wb);
    const size_t ng = (w.carry.size() + kSortedGroup - 1) / kSortedGroup;
    std::vector<uint32_t> W(Wn + 1, 0u);
    std::vector<size_t> order(ng);
    std::iota(order.begin(), order.end(), 0);
    std::shuffle(order.begin(), order.end(), rng);  // groups are independent
    for (size_t g : order) {
        if (g + 1 == ng) sweep_group<true>(w, g, wb, W, g_adds);
        else sweep_group<false>(w, g, wb, W, g_adds);
    }
    g_records += recs.size();
    long long d = 0, r = 0;
    for (uint32_t i = 0; i <= Wn; ++i) {
        int32_t dd, dr;
        sorted_unpack(W[i], dd, dr);
        // (the prefix sums of the sweep's differences are the counts at every cell, so a cell's difference is the counts': the
        // sink cell at the window's end takes back what is left)
        const long long want_d = (long long)depth[i] - (i ? (long long)depth[i - 1] : 0), want_r = (long long)revisits[i] - (i ? (long long)revisits[i - 1] : 0);
        if (sorted_cells_fit(ms, me)) {
            CHECK(dd == want_d && dr == want_r);
            CHECK((uint32_t)std::llabs(want_d) <= std::max(starts[i], ends[i]));
            CHECK((uint32_t)std::llabs(want_r) <= std::max(starts[i], 2u * ends[i]));
        }
        d += dd;
        r += dr;
        if (sorted_cells_fit(ms, me) && i < Wn) CHECK(d == (long long)depth[i] && r == (long long)revisits[i]);
    }
    if (sorted_cells_fit(ms, me)) CHECK(d == 0 && r == 0);
    return 0;
}

static int check_sweep() {
    std::mt19937 rng(4712);
    unsigned long long sets = 0;
    for (uint32_t wb : {11u, 12u, 13u}) {
        const uint32_t W = 1u << wb;
        for (uint32_t round = 0; round < 601 + 60; ++round) {
            const uint32_t n = round <= 600 ? round : 601 + rng() % 800;  // every count up to 600: every tail of one to four chunks, full and not
            const uint32_t kinds[] = {1, 2, 5, 64, 700};
            const uint32_t n_paths = 1 + rng() % kinds[round % 5];
            const uint32_t max_len = round % 7 == 0 ? 1024 : round % 3 == 0 ? 64 : 6;
            const uint32_t span = round % 2 ? std::min(W, 16u + max_len) : W;  // (a narrow stretch: everything overlaps, cells take many starts and ends)
            std::vector<Rec> recs(n);
            for (Rec &r : recs) {
                r.path = round % 11 == 5 ? (uint32_t)(&r - recs.data()) % n_paths : rng() % n_paths;
                r.s = rng() % span;
                r.e = std::min(W, r.s + 1u + (uint32_t)(rng() % max_len));
            }
            if (n > 4) {  // identical, abutting, one cell of overlap, a record up to the window's last cell (its end is the sink)
                recs[1] = recs[0];
                recs[2] = {recs[0].path, recs[0].e < W ? recs[0].e : 0, std::min(W, (recs[0].e < W ? recs[0].e : 0) + 3)};
                recs[3] = {recs[0].path, recs[0].e - 1, std::min(W, recs[0].e + 2)};
                recs[4] = {recs[0].path, W - std::min(max_len, 1000u), W};
            }
            if (check_one(recs, n_paths, wb, rng)) {
                fprintf(stderr, "wb %u, %u records, %u paths, lengths up to %u\n", wb, n, n_paths, max_len);
                return 1;
            }
            ++sets;
        }
    }
    printf("sweep ok: %llu record sets, %llu records against brute force\n", sets, g_records);
    return 0;
}

// One path's records laid so that a cell takes as many revisit ends as it can: the bound on |dR|, and what the rule makes of
// a cell with 2^14 - 1 and with 2^14 starts and ends.
static int check_bound() {
    std::mt19937 rng(7);
    const uint32_t wb = 12, W = 1u << wb;
    unsigned sets = 0;
    for (uint32_t n : {1u, 2u, 3u, 5u, 64u, 65u, 300u}) {
        std::vector<Rec> nested, same, abut, back, borrow;
        for (uint32_t i = 0; i < n; ++i) {
            nested.push_back({0, 100 + i, 1100 - i});          // each inside the one before: every end a revisit's own end
            same.push_back({0, 500, 600});                     // identical: n starts and n ends on two cells, n - 1 revisits
            abut.push_back({0, 10 * i, 10 * i + 10});          // abutting: no revisit, a cell takes a start and an end
            back.push_back({0, 200 + 6 * i, 200 + 6 * i + 10});  // stepping back by four: each cut at the earlier end, then on past it
            // more records end at 900 than start there while the revisits there are positive: the low half borrows from the high
            borrow.push_back({0, 900 - (i % 7u) - 1u, 900});
        }
        borrow.push_back({0, 880, 1000});
        borrow.push_back({0, 900, 950});
        for (auto *set : {&nested, &same, &abut, &back, &borrow}) {
            if (check_one(*set, 1, wb, rng)) return 1;
            // ... and the same as three paths' records, and with every record twice
            std::vector<Rec> three = *set;
            for (size_t i = 0; i < three.size(); ++i) three[i].path = (uint32_t)(i % 3);
            if (check_one(three, 3, wb, rng)) return 1;
            std::vector<Rec> twice = *set;
            twice.insert(twice.end(), set->begin(), set->end());
            if (check_one(twice, 1, wb, rng)) return 1;
            sets += 3;
        }
    }
    // the rule's edge: one path going to and fro between two far-apart cells
    for (uint32_t n : {(1u << 14) - 1u, 1u << 14}) {
        std::vector<Rec> recs;
        for (uint32_t i = 0; i < n; ++i) {
            recs.push_back({0, 7, 8});
            recs.push_back({0, W - 9, W - 8});
        }
        if (check_one(recs, 1, wb, rng, n < (1u << 14))) return 1;
        uint32_t ms = n, me = n;
        CHECK(sorted_cells_fit(ms, me) == (n < (1u << 14)));
        ++sets;
    }
    printf("bound ok: %u record sets\n", sets);
    return 0;
}

int main() {
    if (check_round_trip() || check_rule() || check_sweep() || check_bound()) return 1;
    printf("LDS adds a record in these sets: %.2f\n", (double)g_adds / (double)g_records);
    printf("all ok\n");
    return 0;
}
