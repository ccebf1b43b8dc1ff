// The sweep over groups of four chunks of the sorted record image (pollen_amd/csrc/depth_sorted_host.hpp: sorted_lane_keys,
// sorted_record_step, sorted_seed -- the text k_accum_sorted runs), without a GPU: a window's image as sorted_image_finalise
// defines it (first-of-path flags, the ordinals in bits 24..30, padding to whole chunks, a carry word per chunk), swept group by
// group in shuffled order, a wave's 64 lanes one after the other with the exclusive prefix maximum the DPP scan gives them --
// the group with the window's last chunk through the build that checks for padding, every other one through the build that
// checks nothing -- against brute force with a visited set per path: every cell a path covers c times counts c - 1 revisits.
#include <algorithm>
#include <cstdio>
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

// k_accum_sorted's sweep_group<true, wb, CHECKED>, the wave's lanes one after the other.  Lanes whose chunk lies behind the
// window's last read the window's last four records and its last carry, as the kernel's clamped addresses do.
template <bool CHECKED>
static void sweep_group(const Window &w, size_t g, uint32_t wb, std::vector<int> &D, std::vector<int> &R) {
    const size_t nc = w.carry.size();
    uint32_t before = 0;  // the largest t over the lanes before: what wave_shr:1 and the inclusive scan leave in the lane
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
        for (uint32_t k = 0; k < kSortedGroup; ++k) {
            uint32_t end;
            const bool hit = sorted_record_step<CHECKED>(p, ln.x[k], ln.len[k], end);
            if (!CHECKED || ln.x[k] != 0u) {
                D[ln.s[k]] += 1;
                D[ln.s[k] + ln.len[k] + 1u] -= 1;
            }
            if (hit) {
                R[ln.s[k]] += 1;
                R[end] -= 1;
            }
        }
        before = sorted_umax(before, ln.t);
    }
}

static int check_record_word() {
    // the ordinal's bits are free at every width, between the first-of-path flag and the padding flag
    for (uint32_t wb : {11u, 12u, 13u}) {
        const uint32_t low = ((1u << wb) - 1u) | (1023u << wb);
        CHECK(low < kSortedFirst && (kSortedFirst << 1) == (1u << kSortedOrdShift));
        CHECK(((64u << kSortedOrdShift) & (low | kSortedFirst | kSortedPad)) == 0u && (64u << kSortedOrdShift) < kSortedPad);
    }
    CHECK(kSortedChunk == 64u && kSortedGroup == 4u && kSortedOrdMask >= kSortedChunk);
    // a key holds chunk | ordinal | end without one running into the other: the largest end is the window's size
    CHECK((8192u >> kSortedEndBits) == 0u && ((64u << kSortedEndBits) >> kSortedQShift) == 0u && ((kSortedGroup - 1u) << kSortedQShift) >> kSortedQShift == kSortedGroup - 1u);
    printf("record word ok\n");
    return 0;
}

static int check_one(std::vector<Rec> recs, uint32_t n_paths, uint32_t wb, std::mt19937 &rng) {
    const uint32_t W = 1u << wb;
    const SortedKey k = sorted_key(wb, n_paths, 1);
    std::stable_sort(recs.begin(), recs.end(), [&](const Rec &a, const Rec &b) { return k.pack(0, a.path, a.s) < k.pack(0, b.path, b.s); });
    // brute force: the records are grouped by path, so one array of stamps is every path's visited set in turn
    std::vector<uint32_t> depth(W, 0), revisits(W, 0), seen(W, 0);
    for (const Rec &r : recs)
        for (uint32_t i = r.s; i < r.e; ++i) {
            ++depth[i];
            if (seen[i] == r.path + 1u) ++revisits[i];
            seen[i] = r.path + 1u;
        }
    const Window w = finalise(recs, wb);
    const size_t ng = (w.carry.size() + kSortedGroup - 1) / kSortedGroup;
    std::vector<int> D(W + 1, 0), R(W + 1, 0);
    std::vector<size_t> order(ng);
    std::iota(order.begin(), order.end(), 0);
    std::shuffle(order.begin(), order.end(), rng);  // groups are independent
    for (size_t g : order) {
        if (g + 1 == ng) sweep_group<true>(w, g, wb, D, R);
        else sweep_group<false>(w, g, wb, D, R);
    }
    int d = 0, r = 0;
    for (uint32_t i = 0; i < W; ++i) {
        d += D[i];
        r += R[i];
        CHECK(d == (int)depth[i] && r == (int)revisits[i]);
    }
    return 0;
}

static int check_groups() {
    std::mt19937 rng(4711);
    unsigned long long sets = 0, records = 0;
    for (uint32_t wb : {11u, 12u, 13u}) {
        const uint32_t W = 1u << wb;
        for (uint32_t round = 0; round < 601 + 90; ++round) {
            const uint32_t n = round <= 600 ? round : 601 + rng() % 800;  // every count up to 600: every tail of one to four chunks, full and not
            const uint32_t kinds[] = {1, 2, 5, 64, 700};
            const uint32_t n_paths = 1 + rng() % kinds[round % 5];
            const uint32_t max_len = round % 7 == 0 ? 1024 : round % 3 == 0 ? 64 : 6;
            const uint32_t span = round % 2 ? std::min(W, 16u + max_len) : W;  // (a narrow stretch: everything overlaps)
            std::vector<Rec> recs(n);
            for (Rec &r : recs) {
                r.path = round % 11 == 5 ? (uint32_t)(&r - recs.data()) % n_paths : rng() % n_paths;
                r.s = rng() % span;
                r.e = std::min(W, r.s + 1u + (uint32_t)(rng() % max_len));
            }
            if (n > 4) {  // identical, abutting, one cell of overlap, a record up to the window's last cell
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
            records += n;
        }
        // a path per record: every record a first, the ordinal reaches 64
        for (uint32_t n : {64u, 256u, 257u, 700u}) {
            std::vector<Rec> recs(n);
            for (uint32_t i = 0; i < n; ++i) recs[i] = {i, (i * 7u) % 100u, (i * 7u) % 100u + 1u + i % 50u};
            if (check_one(recs, n, wb, rng)) return 1;
            ++sets;
            records += n;
        }
    }
    printf("groups ok: %llu record sets, %llu records against brute force\n", sets, records);
    return 0;
}

int main() {
    if (check_record_word() || check_groups()) return 1;
    printf("all ok\n");
    return 0;
}
