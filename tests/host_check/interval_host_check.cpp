// Drives the host side of interval depth over many paths (flatgfa_core.cpp: plan_interval_batches, make_paths_windows,
// window_table_cuts, bed_entry_paths, with parse_bed and emit_interval_depth around them -- what flatgfa_intervals_depth and the two tables on
// it do before and after the device's part) for the sanitizer build of pollen_amd/csrc/Makefile (interval_host_check,
// interval_host_asan).  CPU only.
//
//   interval_host_check FILE.gfa ...   for every fixture: the windows of all paths at sizes 1, 4 and 2^64 - 1 (lengths from a host
//                                      walk); where each listed path's windows begin, and the cuts of a window table between two
//                                      listed copies of one path (window_table_cuts) against their definition; a BED that names every path in shuffled blocks, and one with a name the graph does
//                                      not have; the batch plan of the BED's groups at budgets 0, 1, the longest path and no
//                                      limit, checked here for what a plan must hold; path ids and spans out of range, which the
//                                      plan must refuse without reading past anything.  Prints one line per fixture and a digest;
//                                      the sanitized build prints the same.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../pollen_amd/csrc/flatgfa_core.hpp"

using namespace fgfa;

static uint64_t fnv(uint64_t h, const void *p, size_t n) {
    const uint8_t *b = (const uint8_t *)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

[[noreturn]] static void fail(const char *what, const char *file) {
    fprintf(stderr, "interval_host_check: %s (%s)\n", what, file);
    exit(1);
}

// what every plan must hold: the batches tile the intervals at group boundaries, name each of their paths once, and none but
// a batch of one path is over the budget
static void check_plan(const std::vector<uint32_t> &ids, const std::vector<uint32_t> &begin, const std::vector<uint32_t> &end, uint64_t budget,
                       const std::vector<uint32_t> &paths, const std::vector<IntervalBatch> &plan, const char *file) {
    if (ids.empty()) {
        if (!plan.empty()) fail("a plan of no intervals has a batch", file);
        return;
    }
    uint64_t at = 0;
    size_t slot = 0;
    for (const IntervalBatch &b : plan) {
        if (b.i0 != at || b.i1 <= b.i0 || b.s0 != slot || b.s1 <= b.s0) fail("the batches do not tile", file);
        if (b.i0 && ids[b.i0] == ids[b.i0 - 1]) fail("a batch begins inside a group", file);
        std::vector<uint32_t> named(paths.begin() + b.s0, paths.begin() + b.s1);
        uint64_t steps = 0;
        for (uint32_t p : named) steps += end[p] - begin[p];
        if (steps != b.n_steps || (named.size() > 1 && steps > budget)) fail("a batch is over the budget", file);
        std::sort(named.begin(), named.end());
        if (std::adjacent_find(named.begin(), named.end()) != named.end()) fail("a batch names a path twice", file);
        for (uint64_t i = b.i0; i < b.i1; ++i)
            if (!std::binary_search(named.begin(), named.end(), ids[i])) fail("an interval's path is not in its batch", file);
        at = b.i1, slot = b.s1;
    }
    if (at != ids.size() || slot != paths.size()) fail("the batches do not cover the intervals", file);
}

// window_table_cuts against its definition, entry by entry: a cut lies exactly where two neighbouring entries belong to two
// listed copies of one path.  Returns the number of such seams.
static size_t check_cuts(const View &v, const std::vector<uint32_t> &list, const std::vector<uint64_t> &lens, uint64_t size, const char *file) {
    Bed bed;
    std::vector<uint32_t> entry_path;
    std::vector<size_t> path_entry, cuts;
    make_paths_windows(v, list.data(), list.size(), lens.data(), size, &bed, &entry_path, &path_entry);
    const size_t n = bed.entries.size();
    if (path_entry.size() != list.size() + 1 || path_entry[0] != 0 || path_entry.back() != n) fail("path_entry does not span the entries", file);
    std::vector<size_t> owner(n);
    for (size_t k = 0; k < list.size(); ++k) {
        if (path_entry[k + 1] < path_entry[k]) fail("path_entry goes back", file);
        if ((path_entry[k + 1] > path_entry[k]) != (lens[k] > 0)) fail("a path's windows are not where path_entry says", file);
        for (size_t e = path_entry[k]; e < path_entry[k + 1]; ++e) {
            owner[e] = k;
            if (entry_path[e] != list[k] || (e == path_entry[k] ? bed.entries[e].start != 0 : bed.entries[e].start != bed.entries[e - 1].end))
                fail("an entry is not its path's next window", file);
        }
        if (path_entry[k + 1] > path_entry[k] && bed.entries[path_entry[k + 1] - 1].end != lens[k]) fail("a path's windows stop short", file);
    }
    std::vector<size_t> want(1, 0);
    for (size_t e = 1; e < n; ++e)
        if (owner[e] != owner[e - 1] && list[owner[e]] == list[owner[e - 1]]) want.push_back(e);
    if (n) want.push_back(n);
    window_table_cuts(list.data(), list.size(), path_entry, &cuts);
    if (cuts != want) fail("the cuts are not the seams between copies of one path", file);
    return want.size() - (n ? 2 : 1);
}

int main(int argc, char **argv) {
    uint64_t all = 1469598103934665603ull;
    for (int k = 1; k < argc; ++k) {
        std::ifstream f(argv[k], std::ios::binary);
        std::string t((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        Store st;
        std::string err;
        if (!parse_gfa((const uint8_t *)t.data(), t.size(), &st, &err, false)) {
            all = fnv(all, err.data(), err.size());
            continue;
        }
        const View v = st.view();
        if (!validate_step_ids(v)) continue;
        const size_t P = v.paths.len;
        std::vector<uint32_t> all_ids(P), begin(P), end(P);
        std::vector<uint64_t> lens(P);
        uint64_t longest = 0;
        for (size_t p = 0; p < P; ++p) {
            all_ids[p] = (uint32_t)p;
            begin[p] = v.paths[p].steps.start, end[p] = v.paths[p].steps.end;
            lens[p] = path_length(v, (uint32_t)p);
            longest = std::max<uint64_t>(longest, end[p] - begin[p]);
        }
        // ---- windows ----
        size_t n_windows = 0;
        for (uint64_t size : {(uint64_t)1, (uint64_t)4, ~(uint64_t)0}) {
            Bed bed;
            std::vector<uint32_t> entry_path;
            std::vector<size_t> path_entry;
            make_paths_windows(v, all_ids.data(), P, lens.data(), size, &bed, &entry_path, &path_entry);
            if (path_entry.size() != P + 1) fail("path_entry has not one value per listed path and one more", argv[k]);
            if (entry_path.size() != bed.entries.size()) fail("windows without a path", argv[k]);
            size_t at = 0;
            for (size_t p = 0; p < P; ++p) {  // the same entries as one make_windows per path
                if (path_entry[p] != at) fail("a path's entries begin elsewhere", argv[k]);
                const Path &path = v.paths[p];
                Bed one;
                make_windows(v.name_data.data + path.name.start, path.name.len(), 0, lens[p], size, &one);
                for (const BedEntry &e : one.entries) {
                    if (at >= bed.entries.size()) fail("too few windows", argv[k]);
                    const BedEntry &g = bed.entries[at];
                    const std::string a((const char *)bed.name_data.data() + g.name_start, g.name_end - g.name_start),
                        b((const char *)one.name_data.data() + e.name_start, e.name_end - e.name_start);
                    if (g.start != e.start || g.end != e.end || a != b || entry_path[at] != p) fail("a window differs", argv[k]);
                    ++at;
                }
            }
            if (at != bed.entries.size() || path_entry[P] != at) fail("too many windows", argv[k]);
            n_windows += at;
            std::vector<double> depths(bed.entries.size(), 1.5);
            std::string table;
            emit_interval_depth(bed, depths.data(), &table);
            all = fnv(all, table.data(), table.size());
        }
        // ---- lists that name a path again: no seam (all paths, and none), every path twice in a row, thrice, the first path
        // again behind all the others -- as they are, and with the others' lengths taken as 0 -- and a lone path of no length ----
        size_t n_seams = 0;
        for (uint64_t size : {(uint64_t)1, (uint64_t)4, ~(uint64_t)0}) {
            n_seams += check_cuts(v, all_ids, lens, size, argv[k]);
            n_seams += check_cuts(v, {}, {}, size, argv[k]);
            for (size_t times : {2, 3}) {
                std::vector<uint32_t> list;
                std::vector<uint64_t> ll;
                for (size_t p = 0; p < P; ++p) list.insert(list.end(), times, (uint32_t)p), ll.insert(ll.end(), times, lens[p]);
                n_seams += check_cuts(v, list, ll, size, argv[k]);
            }
            if (P) {
                std::vector<uint32_t> list = all_ids;
                std::vector<uint64_t> ll = lens;
                list.push_back(0), ll.push_back(lens[0]);
                n_seams += check_cuts(v, list, ll, size, argv[k]);
                std::fill(ll.begin() + 1, ll.end() - 1, 0);
                n_seams += check_cuts(v, list, ll, size, argv[k]);
                n_seams += check_cuts(v, {0, 0}, {0, 0}, size, argv[k]);
            }
        }
        // ---- a BED that names every path in shuffled blocks ----
        std::string text = "#name\tstart\tend\n";
        uint64_t x = 88172645463325252ull + (uint64_t)k;
        std::vector<uint32_t> want;
        for (size_t r = 0; r < 3 * P; ++r) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            const uint32_t p = (uint32_t)(x % P);
            const Path &path = v.paths[p];
            for (uint64_t e = 0; e <= x % 3; ++e) {
                text.append((const char *)v.name_data.data + path.name.start, path.name.len());
                text += "\t" + std::to_string((x >> 8) % 7 + e) + "\t" + std::to_string((x >> 16) % 11) + "\n";
                want.push_back((uint32_t)v.find_path(v.name_data.data + path.name.start, path.name.len()));  // (names may repeat: the first)
            }
        }
        Bed bed;
        if (!parse_bed((const uint8_t *)text.data(), text.size(), &bed, &err)) fail("the BED does not parse", argv[k]);
        std::vector<uint32_t> ids;
        size_t bad = 0;
        if (!bed_entry_paths(v, bed, &ids, &bad) || ids != want) fail("BED names resolve to other paths", argv[k]);
        const std::string stray = text + "no such path\t0\t1\n";
        Bed bed2;
        std::vector<uint32_t> ids2;
        if (!parse_bed((const uint8_t *)stray.data(), stray.size(), &bed2, &err)) fail("the BED does not parse", argv[k]);
        const bool refused = P && !bed_entry_paths(v, bed2, &ids2, &bad) && bad == bed2.entries.size() - 1;
        // ---- the plan ----
        size_t n_batches = 0;
        for (uint64_t budget : {(uint64_t)0, (uint64_t)1, longest, ~(uint64_t)0}) {
            std::vector<uint32_t> paths;
            std::vector<IntervalBatch> plan;
            if (!plan_interval_batches(ids.data(), ids.size(), begin.data(), end.data(), (uint32_t)P, v.steps.len, budget, &paths, &plan, &err))
                fail("a plan is refused", argv[k]);
            check_plan(ids, begin, end, budget, paths, plan, argv[k]);
            n_batches += plan.size();
        }
        int refusals = 0;
        if (P) {
            std::vector<uint32_t> paths;
            std::vector<IntervalBatch> plan;
            std::vector<uint32_t> bad_ids = {0, (uint32_t)P, 0};
            refusals += plan_interval_batches(bad_ids.data(), 3, begin.data(), end.data(), (uint32_t)P, v.steps.len, 8, &paths, &plan, &err) ? 0 : 1;
            std::vector<uint32_t> e2 = end;
            e2[P - 1] = (uint32_t)v.steps.len + 1;
            const uint32_t last = (uint32_t)P - 1;
            refusals += plan_interval_batches(&last, 1, begin.data(), e2.data(), (uint32_t)P, v.steps.len, 8, &paths, &plan, &err) ? 0 : 1;
            std::vector<uint32_t> b2 = begin;
            b2[0] = end[0] + 1;
            const uint32_t zero = 0;
            refusals += plan_interval_batches(&zero, 1, b2.data(), end.data(), (uint32_t)P, v.steps.len, 8, &paths, &plan, &err) ? 0 : 1;
            refusals += plan_interval_batches(nullptr, 0, begin.data(), end.data(), (uint32_t)P, v.steps.len, 8, &paths, &plan, &err) && plan.empty() ? 1 : 0;
        }
        printf("%s windows=%zu seams=%zu bed=%zu refused=%d batches=%zu refusals=%d\n", argv[k], n_windows, n_seams, ids.size(), (int)refused, n_batches,
               refusals);
        all = fnv(all, ids.data(), ids.size() * 4);
    }
    printf("all %016llx\n", (unsigned long long)all);
    return 0;
}
