// Drives the host side of validate and degree (flatgfa_core.cpp: emit_missing_links, emit_degree -- what
// flatgfa_validate_table and flatgfa_degree_table format from the device's records) for the sanitizer builds of
// pollen_amd/csrc/Makefile (topology_check, topology_asan, topology_tsan).  CPU only.
//
//   topology_check FILE.gfa ...   for every fixture: the records a host walk of the paths finds (validate.py:9-24 over a
//                                 sorted key vector), formatted; the degrees, formatted; and records that name paths or
//                                 segments the graph does not have, which the formatter must refuse without reading them.
//                                 Prints the two tables' sizes per fixture and one digest; the sanitized builds print the same.
#include <algorithm>
#include <cstdint>
#include <cstdio>
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

static uint64_t canon(uint32_t a, uint32_t b) {
    const uint64_t x = ((uint64_t)a << 32) | b, y = ((uint64_t)(b ^ 1u) << 32) | (a ^ 1u);
    return std::min(x, y);
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
        std::vector<uint64_t> keys, deg(v.segs.len + 1, 0);
        for (size_t i = 0; i < v.links.len; ++i) {
            const Link l = v.links[i];
            if ((l.from >> 1) >= v.segs.len || (l.to >> 1) >= v.segs.len) continue;
            keys.push_back(canon(l.from, l.to));
            ++deg[l.from >> 1], ++deg[l.to >> 1];
        }
        std::sort(keys.begin(), keys.end());
        std::vector<MissingLink> recs;
        for (size_t p = 0; p < v.paths.len; ++p) {
            const Span sp = v.paths[p].steps;
            for (uint32_t i = sp.start; i + 1 < sp.end; ++i) {
                const uint32_t a = v.steps[i].bits, b = v.steps[i + 1].bits;
                if (!std::binary_search(keys.begin(), keys.end(), canon(a, b))) recs.push_back(MissingLink{(uint32_t)p, i - sp.start, a, b});
            }
        }
        std::string table, dtab, none;
        const bool ok = emit_missing_links(v, recs.data(), recs.size(), &table);
        emit_degree(v, deg.data(), &dtab);
        const bool empty_ok = emit_missing_links(v, nullptr, 0, &none);
        // records that name nothing: refused, whatever else they hold
        const MissingLink bad[3] = {{(uint32_t)v.paths.len, 0, 0, 0}, {0, 0, (uint32_t)(v.segs.len << 1), 0}, {0, 0, 0, 0xFFFFFFFFu}};
        int refused = 0;
        for (const MissingLink &r : bad) {
            std::string scratch;
            refused += emit_missing_links(v, &r, 1, &scratch) ? 0 : 1;
        }
        printf("%s validate=%zu degree=%zu ok=%d empty=%d refused=%d\n", argv[k], table.size(), dtab.size(), (int)ok, (int)(empty_ok && none.empty()), refused);
        all = fnv(all, table.data(), table.size());
        all = fnv(all, dtab.data(), dtab.size());
    }
    printf("all %016llx\n", (unsigned long long)all);
    return 0;
}
