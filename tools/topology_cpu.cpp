// A single-thread restatement of slow_odgi's validate (validate.py:5-25) and degree (degree.py:5-18) over a .flatgfa file,
// for tools/topology_bench.py: what one core does with the same work.  The links become a sorted vector of canonical keys
// (min of from << 32 | to and flip(to) << 32 | flip(from)); every consecutive step pair of a path is one binary search.
// usage: topology_cpu FILE.flatgfa [REPEATS]
// prints one JSON line: the number of records, a weighted sum of them and of the degrees, and the best times in milliseconds
// (index: sort of the keys and the degree count; steps: the walk over the paths).
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#pragma pack(push, 1)
struct Span { uint32_t start, end; };
struct Path { Span name, steps, overlaps; };
struct Link { uint32_t from, to; Span overlap; };
#pragma pack(pop)
struct Rec { uint32_t path, step, from, to; };
static const size_t kElem[11] = {1, 24, 24, 16, 4, 1, 8, 4, 1, 1, 1};

static uint64_t canon(uint32_t a, uint32_t b) {
    const uint64_t x = ((uint64_t)a << 32) | b, y = ((uint64_t)(b ^ 1u) << 32) | (a ^ 1u);
    return std::min(x, y);
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: topology_cpu FILE.flatgfa [REPEATS]\n"); return 2; }
    const int fd = open(argv[1], O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb)) { perror(argv[1]); return 1; }
    const uint8_t *m = (const uint8_t *)mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE | MAP_POPULATE, fd, 0);
    if (m == MAP_FAILED) { perror("mmap"); return 1; }
    const uint8_t *pool[11];
    uint64_t len[11];
    size_t off = 8 + 11 * 16;
    for (int k = 0; k < 11; ++k) {  // file.rs:29-38: magic, then (len, capacity) per pool; the pools follow by capacity
        uint64_t cap;
        memcpy(&len[k], m + 8 + k * 16, 8);
        memcpy(&cap, m + 16 + k * 16, 8);
        pool[k] = m + off;
        off += cap * kElem[k];
    }
    const Path *paths = (const Path *)pool[2];
    const Link *links = (const Link *)pool[3];
    const uint32_t *steps = (const uint32_t *)pool[4];
    const uint64_t S = len[1], P = len[2], L = len[3];
    const int repeats = argc > 2 ? atoi(argv[2]) : 1;
    double best_index = 1e300, best_steps = 1e300;
    std::vector<Rec> recs;
    std::vector<uint64_t> keys, deg;
    for (int r = 0; r < repeats; ++r) {
        auto t0 = std::chrono::steady_clock::now();
        keys.assign(L, 0);
        deg.assign(S, 0);
        for (uint64_t i = 0; i < L; ++i) {
            keys[i] = canon(links[i].from, links[i].to);
            ++deg[links[i].from >> 1], ++deg[links[i].to >> 1];
        }
        std::sort(keys.begin(), keys.end());
        auto t1 = std::chrono::steady_clock::now();
        recs.clear();
        for (uint64_t p = 0; p < P; ++p) {
            const Span sp = paths[p].steps;
            for (uint32_t i = sp.start; i + 1 < sp.end; ++i)
                if (!std::binary_search(keys.begin(), keys.end(), canon(steps[i], steps[i + 1])))
                    recs.push_back(Rec{(uint32_t)p, i - sp.start, steps[i], steps[i + 1]});
        }
        auto t2 = std::chrono::steady_clock::now();
        best_index = std::min(best_index, std::chrono::duration<double, std::milli>(t1 - t0).count());
        best_steps = std::min(best_steps, std::chrono::duration<double, std::milli>(t2 - t1).count());
    }
    uint64_t h = 0, hd = 0;
    for (size_t k = 0; k < recs.size(); ++k) h += (uint64_t)(k + 1) * (recs[k].path + 3ull * recs[k].step + 5ull * recs[k].from + 7ull * recs[k].to);
    for (size_t s = 0; s < deg.size(); ++s) hd += (uint64_t)(s + 1) * deg[s];
    printf("{\"records\": %zu, \"checksum\": \"%016llx\", \"degree_checksum\": \"%016llx\", \"index_ms\": %.3f, \"steps_ms\": %.3f}\n", recs.size(),
           (unsigned long long)h, (unsigned long long)hd, best_index, best_steps);
    return 0;
}
