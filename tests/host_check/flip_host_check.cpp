// Drives the host's stages of flatgfa_flip (pollen_amd/csrc/flip_host.hpp: check_and_lay, names_bytes, rebuild_names,
// assemble) for the sanitizer build of pollen_amd/csrc/Makefile (flip_host_check, flip_host_check_asan).  CPU only.
//
//   flip_host_check FILE.gfa ...   for every fixture: the paths laid out; what the device would hand back -- the turned flags,
//                                  the new steps, the kept links -- made by a plain host walk of the rules; the new store
//                                  assembled from it and laid out again (nothing turns twice).  Then pools that must be
//                                  refused: spans that leave their pools, counts past the 32-bit ids (no memory behind them:
//                                  the verdict comes before any is read).  Prints one line per fixture and one digest; the
//                                  sanitized build prints the same.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../../pollen_amd/csrc/flatgfa_core.hpp"
#include "../../pollen_amd/csrc/flip_host.hpp"

using namespace fgfa;
using fgfa_flip::Lay;
using fgfa_flip::Verdict;

static uint64_t fnv(uint64_t h, const void *p, size_t n) {
    const uint8_t *b = (const uint8_t *)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

using Key = std::tuple<uint32_t, uint32_t, std::vector<uint32_t>>;

// flip.py on a view that passed check_and_lay and whose ids are in range: what the device hands the host
static void walk(const View &v, const Lay &lay, std::vector<uint32_t> *turned, std::vector<Handle> *steps, std::vector<Link> *links, bool *any_new) {
    const size_t P = v.paths.len;
    turned->assign(P + 1, 0);
    steps->clear();
    std::vector<std::pair<uint32_t, uint32_t>> cand;
    for (size_t p = 0; p < P; ++p) {
        const Span sp = v.paths[p].steps;
        uint64_t fwd = 0, rev = 0;
        for (uint32_t i = sp.start; i < sp.end; ++i) (v.steps[i].is_forward() ? fwd : rev) += v.segs[v.steps[i].segment()].seq.len();
        (*turned)[p] = rev > fwd;
        const size_t at = steps->size();
        if (rev > fwd) {
            for (uint32_t i = sp.end; i-- > sp.start;) steps->push_back(Handle{v.steps[i].bits ^ 1u});
            for (size_t i = at; i + 1 < steps->size(); ++i) cand.emplace_back((*steps)[i].bits, (*steps)[i + 1].bits);
        } else {
            for (uint32_t i = sp.start; i < sp.end; ++i) steps->push_back(v.steps[i]);
        }
        if (at != lay.pstart[p] || steps->size() != lay.pstart[p + 1]) std::abort();
    }
    std::set<Key> seen;
    links->clear();
    *any_new = false;
    const uint32_t A = (uint32_t)v.alignment.len;
    const auto take = [&](uint32_t from, uint32_t to, std::vector<uint32_t> ops, const Link &rec, bool is_new) {
        if (seen.count(Key{from, to, ops}) || seen.count(Key{to ^ 1u, from ^ 1u, ops})) return;
        seen.insert(Key{from, to, std::move(ops)});
        links->push_back(rec);
        *any_new = *any_new || is_new;
    };
    for (size_t i = 0; i < v.links.len; ++i) {
        const Link l = v.links[i];
        std::vector<uint32_t> ops;
        for (uint32_t x = l.overlap.start; x < l.overlap.end; ++x) ops.push_back(v.alignment[x].bits);
        take(l.from, l.to, std::move(ops), l, false);
    }
    for (const auto &c : cand) take(c.first, c.second, {fgfa_flip::kZeroM}, Link{c.first, c.second, Span{A, A + 1}}, true);
}

static bool ids_in_range(const View &v) {
    if (!validate_step_ids(v)) return false;
    for (size_t i = 0; i < v.links.len; ++i) {
        const Link l = v.links[i];
        if ((l.from >> 1) >= v.segs.len || (l.to >> 1) >= v.segs.len || l.overlap.start > l.overlap.end || l.overlap.end > v.alignment.len) return false;
    }
    return true;
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
        Lay lay;
        std::string why;
        if (fgfa_flip::check_and_lay(v, &lay, &why) != Verdict::kOk || !ids_in_range(v)) {
            printf("%s refused: %s\n", argv[k], why.c_str());
            continue;
        }
        std::vector<uint32_t> turned;
        std::vector<Handle> steps;
        std::vector<Link> links;
        bool any_new = false;
        walk(v, lay, &turned, &steps, &links, &any_new);
        const uint64_t name_bytes = fgfa_flip::names_bytes(v, turned.data());
        Store out;
        fgfa_flip::assemble(v, lay, turned.data(), std::move(steps), std::move(links), any_new, &out);
        const View w = out.view();
        // the new store is a graph of the same kind: laid out already, and nothing of it turns
        Lay lay2;
        int again = fgfa_flip::check_and_lay(w, &lay2, &why) == Verdict::kOk && ids_in_range(w) && lay2.pstart == lay.pstart &&
                    std::equal(lay2.pbegin.begin(), lay2.pbegin.end() - 1, lay.pstart.begin());
        if (again) {
            std::vector<uint32_t> turned2;
            std::vector<Handle> steps2;
            std::vector<Link> links2;
            bool new2 = false;
            walk(w, lay2, &turned2, &steps2, &links2, &new2);
            again = !new2 && links2.size() == w.links.len && std::count(turned2.begin(), turned2.end(), 1u) == 0 && steps2.size() == w.steps.len &&
                    (steps2.empty() || !memcmp(steps2.data(), w.steps.data, steps2.size() * 4));
        }
        const long n_turned = (long)std::count(turned.begin(), turned.end(), 1u);
        printf("%s paths=%zu turned=%ld steps=%zu links=%zu names=%llu alignment=%zu again=%d\n", argv[k], w.paths.len, n_turned, w.steps.len, w.links.len,
               (unsigned long long)name_bytes, w.alignment.len, again);
        if (name_bytes != w.name_data.len) return 1;
        for (int ix = 0; ix < 11; ++ix) all = fnv(all, w.pool_data(ix), w.pool_len(ix) * kPoolElemSize[ix]);
    }
    // ---- what must be refused ----
    int refused = 0;
    {
        Store st;
        st.seq_data.assign(4, 'A');
        st.segs = {Segment{1, Span{0, 4}, Span{0, 0}}};
        st.steps = {Handle{0}, Handle{1}};
        st.name_data = {'x'};
        st.paths = {Path{Span{0, 1}, Span{0, 2}, Span{0, 0}}};
        Lay lay;
        std::string why;
        if (fgfa_flip::check_and_lay(st.view(), &lay, &why) != Verdict::kOk || lay.n_lin != 2) return 2;
        const auto bad = [&](const Store &s, Verdict want) {
            Lay l;
            std::string w;
            refused += fgfa_flip::check_and_lay(s.view(), &l, &w) == want && !w.empty();
        };
        Store s = st;
        s.segs[0].seq = Span{1, 5};  // past seq_data
        bad(s, Verdict::kBounds);
        s = st;
        s.segs[0].seq = Span{3, 2};  // ends before it begins
        bad(s, Verdict::kBounds);
        s = st;
        s.paths[0].steps = Span{1, 3};  // past the steps
        bad(s, Verdict::kBounds);
        s = st;
        s.paths[0].name = Span{0, 2};  // past name_data
        bad(s, Verdict::kBounds);
        s = st;  // 65537 paths over 65536 steps each: 2^32 + 2^16 steps laid out
        s.steps.assign(65536, Handle{0});
        s.paths.assign(65537, Path{Span{0, 1}, Span{0, 65536}, Span{0, 0}});
        bad(s, Verdict::kTooLarge);
        // counts past the ids, with no memory behind them
        View v = st.view();
        const auto big = [&](View x) {
            Lay l;
            std::string w;
            refused += fgfa_flip::check_and_lay(x, &l, &w) == Verdict::kTooLarge;
        };
        View x = v;
        x.steps.len = 1ull << 32;
        big(x);
        x = v;
        x.segs.len = 1ull << 31;
        big(x);
        x = v;
        x.paths.len = 0xFFFFFFFFull;
        big(x);
        x = v;
        x.links.len = 1ull << 32;
        big(x);
        x = v;
        x.alignment.len = 0xFFFFFFFFull;
        big(x);
    }
    printf("all %016llx refused=%d\n", (unsigned long long)all, refused);
    return refused == 10 ? 0 : 3;
}
