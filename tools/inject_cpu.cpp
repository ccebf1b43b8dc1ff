// A single-thread C++ restatement of the one-pass inject (slow_odgi/inject.py, without links) over a
// .flatgfa file and a BED file, for tools/inject_bench.py and tests/test_inject_cpu_tool.py: prints the new step count, segment
// count, path count, the steps' checksum (as chop_bench.py's) and the same checksum over the new segments' lengths and over the
// paths' begins and ends, then the seconds the work took without reading the inputs.  The refused cases are not looked for.
//   g++ -O3 -std=c++17 tools/inject_cpu.cpp -o inject_cpu && ./inject_cpu G.flatgfa LINES.bed
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
#include <string>
#include <unordered_map>
#include <vector>

static const uint8_t *map_file(const char *path, size_t *n) {
    const int fd = open(path, O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb)) { fprintf(stderr, "inject_cpu: cannot open %s\n", path); exit(1); }
    *n = (size_t)sb.st_size;
    return *n ? (const uint8_t *)mmap(nullptr, *n, PROT_READ, MAP_PRIVATE, fd, 0) : (const uint8_t *)"";
}
static uint32_t u32_at(const uint8_t *p) {
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}
template <class T>
static uint64_t checksum(const std::vector<T> &v) {
    uint64_t sum = 0;
    for (size_t i = 0; i < v.size(); ++i) sum ^= (uint64_t)v[i] * 0x9E3779B97F4A7C15ull + i;
    return sum;
}

struct Line {
    uint32_t path;
    uint64_t lo, hi;
};

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: inject_cpu G.flatgfa LINES.bed\n"); return 2; }
    size_t mn = 0, bn = 0;
    const uint8_t *m = map_file(argv[1], &mn);
    const char *bed = (const char *)map_file(argv[2], &bn);
    // file.rs:14-38: magic, 11 x {len, capacity}, then the pools at their capacities
    uint64_t toc[23];
    memcpy(toc, m, sizeof toc);
    static const size_t es[11] = {1, 24, 24, 16, 4, 1, 8, 4, 1, 1, 1};
    const uint8_t *pool[11];
    size_t at = sizeof toc;
    for (int i = 0; i < 11; ++i) pool[i] = m + at, at += toc[2 + 2 * i] * es[i];
    const uint64_t S = toc[3], P = toc[5], N = toc[9];
    const uint8_t *steps = pool[4], *names = pool[8];
    std::vector<uint32_t> len(S), pb(P), pe(P);
    for (uint64_t s = 0; s < S; ++s) len[s] = u32_at(pool[1] + s * 24 + 12) - u32_at(pool[1] + s * 24 + 8);
    std::unordered_map<std::string, uint32_t> by_name;
    for (uint64_t p = 0; p < P; ++p) {
        const uint32_t a = u32_at(pool[2] + p * 24), b = u32_at(pool[2] + p * 24 + 4);
        pb[p] = u32_at(pool[2] + p * 24 + 8);
        pe[p] = u32_at(pool[2] + p * 24 + 12);
        by_name.emplace(std::string((const char *)names + a, b - a), (uint32_t)p);
    }
    // the BED: path, start, end, new name; '#' and empty lines skipped; a line on a path the graph lacks is skipped (inject.py:87)
    std::vector<Line> lines;
    for (size_t pos = 0; pos < bn;) {
        const char *nl = (const char *)memchr(bed + pos, '\n', bn - pos), *p = bed + pos, *e = nl ? nl : bed + bn;
        pos = (size_t)(e - bed) + 1;
        if (p == e || *p == '#') continue;
        const char *t1 = (const char *)memchr(p, '\t', (size_t)(e - p));
        if (!t1) { fprintf(stderr, "inject_cpu: bad BED line\n"); return 1; }
        char *q = nullptr;
        const uint64_t lo = strtoull(t1 + 1, &q, 10), hi = strtoull(q + 1, &q, 10);
        const auto it = by_name.find(std::string(p, (size_t)(t1 - p)));
        if (it != by_name.end()) lines.push_back(Line{it->second, lo, hi});
    }
    const auto t0 = std::chrono::steady_clock::now();
    const size_t n = lines.size();
    // positions: pre[i] = the bases before step i of the pool
    std::vector<uint64_t> pre(N + 1);
    for (uint64_t i = 0; i < N; ++i) pre[i + 1] = pre[i] + len[u32_at(steps + i * 4) >> 1];
    // locate (inject.py:24-46): the step that holds x, and the cut when x is inside it
    struct End {
        uint64_t step;
        uint32_t seg, pos;
        bool cut;
    };
    std::vector<End> ends(2 * n);
    std::vector<uint64_t> keys;
    for (size_t l = 0; l < n; ++l)
        for (int side = 0; side < 2; ++side) {
            const uint64_t b = pb[lines[l].path], e = pe[lines[l].path], x = side ? lines[l].hi : lines[l].lo;
            const uint64_t i = (uint64_t)(std::upper_bound(pre.begin() + b + 1, pre.begin() + e + 1, pre[b] + x) - pre.begin()) - 1;
            End en{i, 0, 0, false};
            if (i < e && pre[i] - pre[b] < x) {
                const uint32_t h = u32_at(steps + i * 4), o = (uint32_t)(x - (pre[i] - pre[b]));
                en.seg = h >> 1;
                en.pos = (h & 1) ? len[en.seg] - o : o;
                en.cut = true;
                keys.push_back(((uint64_t)en.seg << 32) | en.pos);
            }
            ends[2 * l + side] = en;
        }
    // the cut table: the distinct cuts of every segment, sorted
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    std::vector<uint32_t> cut_row(S + 1, 0);
    for (uint64_t k : keys) ++cut_row[(k >> 32) + 1];
    for (uint64_t s = 0; s < S; ++s) cut_row[s + 1] += cut_row[s];
    std::vector<uint32_t> seg_len;
    seg_len.reserve(S + keys.size());
    for (uint64_t s = 0; s < S; ++s) {
        uint32_t last = 0;
        for (uint32_t c = cut_row[s]; c < cut_row[s + 1]; ++c) seg_len.push_back((uint32_t)keys[c] - last), last = (uint32_t)keys[c];
        seg_len.push_back(len[s] - last);
    }
    // old paths (chop.py:46-58), and noff[i] = the new steps before step i of the pool
    std::vector<uint64_t> noff(N + 1);
    for (uint64_t i = 0; i < N; ++i) {
        const uint32_t s = u32_at(steps + i * 4) >> 1;
        noff[i + 1] = noff[i] + (cut_row[s + 1] - cut_row[s] + 1);
    }
    std::vector<uint32_t> out, nb(P + n), ne(P + n);
    for (uint64_t p = 0; p < P; ++p) {
        nb[p] = (uint32_t)out.size();
        for (uint32_t i = pb[p]; i < pe[p]; ++i) {
            const uint32_t h = u32_at(steps + (size_t)i * 4), s = h >> 1, a = s + cut_row[s], z = s + 1 + cut_row[s + 1];
            if (h & 1)
                for (uint32_t k = z; k-- > a;) out.push_back((k << 1) | 1);
            else
                for (uint32_t k = a; k < z; ++k) out.push_back(k << 1);
        }
        ne[p] = (uint32_t)out.size();
    }
    // new paths (inject.py:6-21): from the first new step that starts at or after low up to the first that ends after high
    for (size_t l = 0; l < n; ++l) {
        const uint64_t b = pb[lines[l].path], e = pe[lines[l].path];
        uint64_t rel[2];
        for (int side = 0; side < 2; ++side) {
            const End &en = ends[2 * l + side];
            uint64_t i = en.step, w = 0;
            if (en.cut) {
                const uint32_t r0 = cut_row[en.seg], k = cut_row[en.seg + 1] - r0;
                const uint32_t r = (uint32_t)(std::lower_bound(keys.begin() + r0, keys.begin() + r0 + k, ((uint64_t)en.seg << 32) | en.pos) - keys.begin()) - r0;
                w = (u32_at(steps + i * 4) & 1) ? k - r : r + 1;
            } else if (side == 0) {
                i = (uint64_t)(std::lower_bound(pre.begin() + b, pre.begin() + e, pre[b] + lines[l].lo) - pre.begin());
            }
            rel[side] = noff[i] - noff[b] + w;
        }
        const uint64_t cnt = rel[1] > rel[0] ? rel[1] - rel[0] : 0, src = nb[lines[l].path] + rel[0];
        nb[P + l] = (uint32_t)out.size();
        out.resize(out.size() + cnt);  // (not insert from itself: the vector may move)
        memcpy(out.data() + nb[P + l], out.data() + src, cnt * 4);
        ne[P + l] = (uint32_t)out.size();
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    nb.insert(nb.end(), ne.begin(), ne.end());
    printf("%zu %zu %zu %llu %llu %llu %.6f\n", out.size(), seg_len.size(), (size_t)(P + n), (unsigned long long)checksum(out),
           (unsigned long long)checksum(seg_len), (unsigned long long)checksum(nb), secs);
    return 0;
}
