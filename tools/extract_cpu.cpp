// A single-thread restatement of the reference's extract (flatgfa/src/ops/extract.rs) over a .flatgfa file, for
// tools/extract_bench.py: what one core does with the same work.  Two forms of the neighbourhood walk:
//   literal    every popped frontier segment reads all links (extract.rs:166-175)
//   levelwise  one pass over the links per level, the candidates ordered by (rank of the frontier segment, link index) --
//              the same ids; here so that a speed-up is not credited to the reference's quadratic walk
// usage: extract_cpu FILE.flatgfa ORIGIN_ID DIST MAX_DISTANCE ITERATIONS literal|levelwise [REPEATS]
// prints one JSON line: the new graph's sizes, a weighted sum of its pools and the best time in milliseconds.
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
#include <vector>

#pragma pack(push, 1)
struct Span { uint32_t start, end; };
struct Segment { uint64_t name; Span seq, optional; };
struct Path { Span name, steps, overlaps; };
struct Link { uint32_t from, to; Span overlap; };
#pragma pack(pop)

struct Graph {
    const uint8_t *pool[11];
    uint64_t len[11];
};
static const size_t kElem[11] = {1, 24, 24, 16, 4, 1, 8, 4, 1, 1, 1};

struct Out {
    std::vector<Segment> segs;
    std::vector<Path> paths;
    std::vector<Link> links;
    std::vector<uint32_t> steps, alignment;
    std::vector<uint8_t> seq, opt, names;
};

static void extract(const Graph &g, uint32_t origin, uint64_t dist, uint64_t max_dist, uint64_t iters, bool literal, Out *o) {
    const Segment *segs = (const Segment *)g.pool[1];
    const Path *paths = (const Path *)g.pool[2];
    const Link *links = (const Link *)g.pool[3];
    const uint32_t *steps = (const uint32_t *)g.pool[4];
    const uint64_t S = g.len[1], P = g.len[2], L = g.len[3];
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    std::vector<uint32_t> map(S, kNone), order;
    auto include = [&](uint32_t s) { map[s] = (uint32_t)order.size(); order.push_back(s); };
    include(origin);
    std::vector<uint32_t> frontier{origin}, next;
    if (literal) {
        for (uint64_t lvl = 0; lvl < dist && !frontier.empty(); ++lvl) {
            while (!frontier.empty()) {
                const uint32_t p = frontier.back();
                frontier.pop_back();
                for (uint64_t i = 0; i < L; ++i) {
                    const uint32_t f = links[i].from >> 1, t = links[i].to >> 1;
                    const uint32_t other = f == p ? t : t == p ? f : kNone;
                    if (other != kNone && map[other] == kNone) { include(other); next.push_back(other); }
                }
            }
            std::swap(frontier, next);
        }
    } else {
        std::vector<uint32_t> rank(S, kNone);
        std::vector<uint64_t> key(S, ~0ull);
        std::vector<std::pair<uint64_t, uint32_t>> cand;
        for (uint64_t lvl = 0; lvl < dist && !frontier.empty(); ++lvl) {
            for (size_t k = 0; k < frontier.size(); ++k) rank[frontier[k]] = (uint32_t)(frontier.size() - 1 - k);
            cand.clear();
            for (uint64_t i = 0; i < L; ++i) {
                const uint32_t f = links[i].from >> 1, t = links[i].to >> 1;
                if (f == t) continue;
                for (int side = 0; side < 2; ++side) {
                    const uint32_t p = side ? t : f, other = side ? f : t;
                    if (rank[p] == kNone || map[other] != kNone) continue;
                    const uint64_t k = ((uint64_t)rank[p] << 32) | i;
                    if (key[other] == ~0ull) cand.emplace_back(0, other);
                    key[other] = std::min(key[other], k);
                }
            }
            for (uint32_t s : frontier) rank[s] = kNone;
            for (auto &c : cand) c.first = key[c.second];
            std::sort(cand.begin(), cand.end());
            frontier.clear();
            for (auto &c : cand) { include(c.second); frontier.push_back(c.second); }
        }
    }
    auto seg_len = [&](uint32_t h) { return (uint64_t)(segs[h >> 1].seq.end - segs[h >> 1].seq.start); };
    for (uint64_t it = 0; it < iters; ++it)  // merge_subpaths, extract.rs:65-98
        for (uint64_t p = 0; p < P; ++p) {
            bool open = true, ignore = true;
            uint64_t start = 0, length = 0;
            const uint32_t *st = steps + paths[p].steps.start;
            for (uint64_t idx = 0, n = paths[p].steps.end - paths[p].steps.start; idx < n; ++idx) {
                const bool in = map[st[idx] >> 1] != kNone;
                if (open && in) {
                    if (!ignore && length <= max_dist)
                        for (uint64_t k = start; k < idx; ++k)
                            if (map[st[k] >> 1] == kNone) include(st[k] >> 1);
                    open = false, ignore = false;
                } else if (!open && !in) {
                    open = true, start = idx;
                }
                length += seg_len(st[idx]);
            }
        }
    for (uint32_t s : order) {  // include_seg
        const Segment &sg = segs[s];
        const uint32_t a = (uint32_t)o->seq.size(), b = (uint32_t)o->opt.size();
        o->seq.insert(o->seq.end(), g.pool[5] + sg.seq.start, g.pool[5] + sg.seq.end);
        o->opt.insert(o->opt.end(), g.pool[9] + sg.optional.start, g.pool[9] + sg.optional.end);
        o->segs.push_back(Segment{sg.name, {a, (uint32_t)o->seq.size()}, {b, (uint32_t)o->opt.size()}});
    }
    auto tr = [&](uint32_t h) { return (map[h >> 1] << 1) | (h & 1u); };
    const uint32_t *al = (const uint32_t *)g.pool[7];
    for (uint64_t i = 0; i < L; ++i)
        if (map[links[i].from >> 1] != kNone && map[links[i].to >> 1] != kNone) {
            const uint32_t a = (uint32_t)o->alignment.size();
            o->alignment.insert(o->alignment.end(), al + links[i].overlap.start, al + links[i].overlap.end);
            o->links.push_back(Link{tr(links[i].from), tr(links[i].to), {a, (uint32_t)o->alignment.size()}});
        }
    for (uint64_t p = 0; p < P; ++p) {  // find_subpaths, extract.rs:102-134
        bool in_run = false;
        uint64_t pos = 0, run_pos = 0;
        uint32_t run_step = 0;
        auto close = [&](uint64_t end_pos) {
            const uint32_t a = (uint32_t)o->names.size();
            o->names.insert(o->names.end(), g.pool[8] + paths[p].name.start, g.pool[8] + paths[p].name.end);
            const std::string tail = ":" + std::to_string(run_pos) + "-" + std::to_string(end_pos);
            o->names.insert(o->names.end(), tail.begin(), tail.end());
            o->paths.push_back(Path{{a, (uint32_t)o->names.size()}, {run_step, (uint32_t)o->steps.size()}, {0, 0}});
        };
        for (uint32_t i = paths[p].steps.start; i < paths[p].steps.end; ++i) {
            const bool in = map[steps[i] >> 1] != kNone;
            if (in_run && !in) { close(pos); in_run = false; }
            else if (!in_run && in) { in_run = true; run_pos = pos; run_step = (uint32_t)o->steps.size(); }
            if (in) o->steps.push_back(tr(steps[i]));
            pos += seg_len(steps[i]);
        }
        if (in_run) close(pos);
    }
}

// sum of v[i] * (i + 1) mod 2^64: what tools/extract_bench.py forms of the library's pools with numpy
template <class T>
static uint64_t wsum(const T *v, size_t n) {
    uint64_t h = 0;
    for (size_t i = 0; i < n; ++i) h += (uint64_t)v[i] * (uint64_t)(i + 1);
    return h;
}

int main(int argc, char **argv) {
    if (argc < 7) { fprintf(stderr, "usage: extract_cpu FILE.flatgfa ORIGIN_ID DIST MAX_DISTANCE ITERATIONS literal|levelwise [REPEATS]\n"); return 2; }
    const int fd = open(argv[1], O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb)) { perror(argv[1]); return 1; }
    const uint8_t *m = (const uint8_t *)mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE | MAP_POPULATE, fd, 0);
    if (m == MAP_FAILED) { perror("mmap"); return 1; }
    Graph g;
    size_t off = 8 + 11 * 16;
    for (int k = 0; k < 11; ++k) {  // file.rs:29-38: magic, then (len, capacity) per pool; the pools follow by capacity
        uint64_t len, cap;
        memcpy(&len, m + 8 + k * 16, 8);
        memcpy(&cap, m + 16 + k * 16, 8);
        g.pool[k] = m + off;
        g.len[k] = len;
        off += cap * kElem[k];
    }
    const uint32_t origin = (uint32_t)strtoul(argv[2], nullptr, 10);
    const uint64_t dist = strtoull(argv[3], nullptr, 10), max_dist = strtoull(argv[4], nullptr, 10), iters = strtoull(argv[5], nullptr, 10);
    const bool literal = !strcmp(argv[6], "literal");
    const int reps = argc > 7 ? atoi(argv[7]) : 1;
    if (origin >= g.len[1]) { fprintf(stderr, "origin out of range\n"); return 1; }
    double best = 1e300;
    Out last;
    for (int r = 0; r < reps; ++r) {
        Out o;
        const auto t0 = std::chrono::steady_clock::now();
        extract(g, origin, dist, max_dist, iters, literal, &o);
        best = std::min(best, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        last = std::move(o);
    }
    std::vector<uint64_t> names(last.segs.size());
    for (size_t i = 0; i < names.size(); ++i) names[i] = last.segs[i].name;
    const uint64_t h = wsum(last.steps.data(), last.steps.size()) + wsum(names.data(), names.size()) + wsum(last.names.data(), last.names.size()) +
                       wsum(last.seq.data(), last.seq.size()) + wsum((const uint32_t *)last.links.data(), last.links.size() * 4);
    printf("{\"form\": \"%s\", \"segs\": %zu, \"paths\": %zu, \"links\": %zu, \"steps\": %zu, \"seq_bytes\": %zu, \"checksum\": \"%016llx\", \"ms\": %.3f}\n",
           argv[6], last.segs.size(), last.paths.size(), last.links.size(), last.steps.size(), last.seq.size(), (unsigned long long)h, best);
    return 0;
}
