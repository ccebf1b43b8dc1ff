// The host's side of the sorted record image (pollen_amd/csrc/depth_sorted_host.hpp), without a GPU: the sort key and its bits
// in use, the layout of windows and chunks, the memory rule, which plans get an image -- and a host model of what the
// finaliser and the sweep do with a window's sorted records (first-of-path flags, padding, a carry word per chunk, chunks taken
// in any order), against brute force: every cell a path covers c times counts c - 1 revisits.
#include <algorithm>
#include <cassert>
#include <cstdio>
#include <cstring>
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

// What sorted_image_finalise leaves of one window (records sorted by path, then start) ...
struct Window {
    std::vector<uint32_t> rec, carry;
};
static Window finalise(const std::vector<Rec> &sorted, uint32_t wb) {
    Window w;
    const size_t nc = (sorted.size() + kSortedChunk - 1) / kSortedChunk;
    w.rec.assign(nc * kSortedChunk, kSortedPad);
    w.carry.assign(nc, 0u);
    uint32_t m = 0;
    for (size_t i = 0; i < sorted.size(); ++i) {
        const bool first = i == 0 || sorted[i].path != sorted[i - 1].path;
        if (first) m = 0;
        if (i % kSortedChunk == 0) w.carry[i / kSortedChunk] = first ? 0u : m;
        w.rec[i] = sorted[i].s | ((sorted[i].e - sorted[i].s - 1u) << wb) | (first ? kSortedFirst : 0u);
        m = std::max(m, sorted[i].e);
    }
    return w;
}
// ... and what k_accum_sorted makes of one chunk of it, lane by lane as the wave's scan does: the prefix maximum of
// (ordinal << kSortedEndBits | end) over the lanes before, the carry for the path under way.
static void sweep_chunk(const uint32_t *rec, uint32_t carry, uint32_t wb, std::vector<int> &D, std::vector<int> &R) {
    const uint32_t wmask = (1u << wb) - 1u;
    uint32_t ord = 0, before = 0;
    for (uint32_t lane = 0; lane < kSortedChunk; ++lane) {
        const uint32_t r = rec[lane];
        const bool valid = !(r & kSortedPad);
        if (valid && (r & kSortedFirst)) ++ord;
        const uint32_t s = r & wmask, e = s + ((r >> wb) & 1023u) + 1u;
        if (valid) {
            D[s] += 1;
            D[e] -= 1;
            uint32_t M = (before >> kSortedEndBits) == ord ? before & ((1u << kSortedEndBits) - 1u) : 0u;
            if (ord == 0) M = std::max(M, carry);
            if (M > s) {
                R[s] += 1;
                R[std::min(e, M)] -= 1;
            }
        }
        before = std::max(before, valid ? (ord << kSortedEndBits) | e : 0u);
    }
}

static int check_key() {
    CHECK(bits_for(1) == 0 && bits_for(2) == 1 && bits_for(3) == 2 && bits_for(4) == 2 && bits_for(5) == 3 && bits_for(1ull << 32) == 32);
    for (uint32_t wb : {11u, 12u, 13u}) {
        for (uint32_t n_paths : {1u, 2u, 100u, 1000u, 65536u, 0xFFFFFFFFu}) {
            for (uint32_t n_win : {1u, 2u, 300u, 2048u, 1u << 19}) {
                const SortedKey k = sorted_key(wb, n_paths, n_win);
                CHECK(k.bits() <= 64);
                const uint32_t win = n_win - 1, path = n_paths - 1, rel = (1u << wb) - 1u;
                const uint64_t key = k.pack(win, path, rel);
                CHECK(k.win(key) == win && k.path(key) == path && k.rel(key) == rel);
                CHECK(k.bits() == 64 || (key >> k.bits()) == 0);  // nothing above the bits the sort looks at
                // the order: window first, then path, then start
                if (win) CHECK(k.pack(win - 1, path, rel) < k.pack(win, 0, 0));
                if (path) CHECK(k.pack(win, path - 1, rel) < k.pack(win, path, 0));
                CHECK(k.pack(win, path, rel - 1) < key);
            }
        }
    }
    printf("key ok\n");
    return 0;
}

static int check_layout() {
    const uint32_t C = kSortedChunk;
    const std::vector<uint32_t> cnt = {0, 1, C - 1, C, C + 1, 2 * C, 2 * C + 1, 0};
    const SortedLayout l = sorted_layout(cnt.data(), (uint32_t)cnt.size());
    CHECK(l.fits && l.rec_off.size() == cnt.size() + 1 && l.win_chunk.size() == cnt.size() + 1);
    uint64_t recs = 0, chunks = 0;
    for (size_t w = 0; w < cnt.size(); ++w) {
        CHECK(l.rec_off[w] == recs && l.win_chunk[w] == chunks);
        recs += cnt[w];
        chunks += (cnt[w] + C - 1) / C;
        CHECK((uint64_t)(l.win_chunk[w + 1] - l.win_chunk[w]) * C >= cnt[w] && (uint64_t)(l.win_chunk[w + 1] - l.win_chunk[w]) * C < cnt[w] + C);
    }
    CHECK(l.n_records == recs && l.n_chunks == chunks && l.rec_off.back() == recs && l.win_chunk.back() == chunks);
    const std::vector<uint32_t> huge(3, 0x40000000u);
    CHECK(!sorted_layout(huge.data(), 3).fits);
    CHECK(sorted_layout(nullptr, 0).n_records == 0);
    printf("layout ok: %llu records in %llu chunks of %u\n", (unsigned long long)recs, (unsigned long long)chunks, C);
    return 0;
}

static int check_rules() {
    CHECK(sorted_kept_bytes(10, 4) == 10ull * kSortedChunk * 4 + 40 + 20);
    const uint64_t tr = sorted_transient_bytes(1000, 4, 4096);
    CHECK(tr >= 1000ull * 24 + 4096);
    CHECK(!sorted_memory_refused(tr, 100, tr + 100 + (1ull << 30), 1ull << 30, false));
    CHECK(sorted_memory_refused(tr, 100, tr + 99 + (1ull << 30), 1ull << 30, false));
    CHECK(!sorted_memory_refused(tr, 100, 0, 1ull << 30, true));  // the hook waives the rule
    CHECK(sorted_refused(-1, 1, 1, 0, 12, true) == nullptr && sorted_refused(1, 1, 1, 0, 11, true) == nullptr && sorted_refused(-1, 1, 1, 0, 13, true) == nullptr);
    CHECK(!strcmp(sorted_refused(0, 1, 1, 0, 12, true), "hook"));
    CHECK(!strcmp(sorted_refused(-1, 2, 1, 0, 12, true), "parts"));
    CHECK(!strcmp(sorted_refused(-1, 1, 2, 0, 12, true), "ranges") && !strcmp(sorted_refused(-1, 1, 1, 1, 12, true), "ranges"));
    CHECK(!strcmp(sorted_refused(-1, 1, 1, 0, 10, true), "windows") && !strcmp(sorted_refused(-1, 1, 1, 0, 14, true), "windows"));
    CHECK(!strcmp(sorted_refused(1, 1, 1, 0, 12, false), "rewritten"));
    printf("rules ok\n");
    return 0;
}

static int check_sweep() {
    std::mt19937 rng(12345);
    int sets = 0;
    for (uint32_t wb : {11u, 12u, 13u}) {
        const uint32_t W = 1u << wb;
        for (int round = 0; round < 120; ++round) {
            const uint32_t n_paths = 1 + rng() % (round % 3 == 0 ? 200 : 5);
            const uint32_t n = rng() % (round % 4 == 0 ? 5 * kSortedChunk : 2 * kSortedChunk + 2);
            const uint32_t span = round % 2 ? 64 : W;  // (a narrow window: everything overlaps)
            std::vector<Rec> recs(n);
            for (Rec &r : recs) {
                r.path = rng() % n_paths;
                r.s = rng() % span;
                r.e = std::min(W, r.s + 1u + (uint32_t)(rng() % (round % 5 == 0 ? 1024 : 12)));
            }
            if (n > 3) {  // identical, abutting, nested, one cell of overlap
                recs[1] = recs[0];
                recs[2] = {recs[0].path, recs[0].e < W ? recs[0].e : 0, std::min(W, (recs[0].e < W ? recs[0].e : 0) + 3)};
                recs[3] = {recs[0].path, recs[0].e - 1, std::min(W, recs[0].e + 2)};
            }
            // brute force: per path, how often it covers each cell
            std::vector<uint32_t> depth(W, 0), revisits(W, 0);
            for (uint32_t p = 0; p < n_paths; ++p) {
                std::vector<uint32_t> c(W, 0);
                for (const Rec &r : recs)
                    if (r.path == p)
                        for (uint32_t i = r.s; i < r.e; ++i) ++c[i];
                for (uint32_t i = 0; i < W; ++i) {
                    depth[i] += c[i];
                    revisits[i] += c[i] ? c[i] - 1 : 0;
                }
            }
            const SortedKey k = sorted_key(wb, n_paths, 1);
            std::stable_sort(recs.begin(), recs.end(), [&](const Rec &a, const Rec &b) { return k.pack(0, a.path, a.s) < k.pack(0, b.path, b.s); });
            const Window w = finalise(recs, wb);
            std::vector<int> D(W + 1, 0), R(W + 1, 0);
            std::vector<size_t> order(w.carry.size());
            std::iota(order.begin(), order.end(), 0);
            std::shuffle(order.begin(), order.end(), rng);  // chunks are independent
            for (size_t c : order) sweep_chunk(w.rec.data() + c * kSortedChunk, w.carry[c], wb, D, R);
            int d = 0, r = 0;
            for (uint32_t i = 0; i < W; ++i) {
                d += D[i];
                r += R[i];
                CHECK(d == (int)depth[i] && r == (int)revisits[i]);
            }
            ++sets;
        }
    }
    printf("sweep ok: %d record sets against brute force\n", sets);
    return 0;
}

int main() {
    if (check_key() || check_layout() || check_rules() || check_sweep()) return 1;
    printf("all ok\n");
    return 0;
}
