// A single-thread C++ restatement of flip (slow_odgi/slow_odgi/flip.py) over a graph image as the
// device-level entry takes it, for tools/flip_bench.py and tests/test_flip_cpu_tool.py.  STEPS holds u32 handles, SPANS u32 pairs
// (begin, end) per path into them, SEGLEN a u32 per segment, LINKS four u32 per link (from, to, overlap.start, overlap.end) and
// ALIGN the u32 ops the overlaps point into.  A path turns iff its backward steps cover strictly more bases (64-bit sums); the
// new steps go to OUT_STEPS, the paths one behind another; the turned flags (a byte per path) to OUT_TURNED; the kept links
// -- first of each class, in order, the classes held in a hash set keyed by the canonical pair and the overlap's ops; a new
// one's overlap is [n_align, n_align + 1) -- to OUT_LINKS.  Prints the turned paths, the links kept, the new ones among them and
// the seconds the work took without reading or writing the files.  An id or span out of range: exit status 3.
//   g++ -O3 -std=c++17 tools/flip_cpu.cpp -o flip_cpu && ./flip_cpu STEPS SPANS SEGLEN LINKS ALIGN OUT_STEPS OUT_TURNED OUT_LINKS
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unordered_set>
#include <vector>

static std::vector<uint32_t> read_words(const char *path) {
    const int fd = open(path, O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb)) { fprintf(stderr, "flip_cpu: cannot open %s\n", path); exit(1); }
    std::vector<uint32_t> v((size_t)sb.st_size / 4);
    size_t got = 0;
    while (got < v.size() * 4) {
        const ssize_t r = read(fd, (char *)v.data() + got, v.size() * 4 - got);
        if (r <= 0) { fprintf(stderr, "flip_cpu: cannot read %s\n", path); exit(1); }
        got += (size_t)r;
    }
    close(fd);
    return v;
}

static void write_bytes(const char *path, const void *p, size_t n) {
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(p, 1, n, f) != n || fclose(f)) { fprintf(stderr, "flip_cpu: cannot write %s\n", path); exit(1); }
}

static const uint32_t *g_align;
static const uint32_t kZeroM = 0;  // flip.py:56: one op, length 0, match

struct Cls {  // a link's class: the smaller of the pair and its reverse complement, and the overlap's ops
    uint64_t key;
    const uint32_t *ops;
    uint32_t n_ops;
    bool operator==(const Cls &o) const { return key == o.key && n_ops == o.n_ops && !memcmp(ops, o.ops, (size_t)n_ops * 4); }
};
struct ClsHash {
    size_t operator()(const Cls &c) const {
        uint64_t h = c.key * 0x9E3779B97F4A7C15ull;
        for (uint32_t i = 0; i < c.n_ops; ++i) h = (h ^ c.ops[i]) * 0x100000001B3ull;
        return (size_t)(h ^ (h >> 29));
    }
};
static uint64_t canon(uint32_t a, uint32_t b) {
    const uint64_t x = ((uint64_t)a << 32) | b, y = ((uint64_t)(b ^ 1u) << 32) | (a ^ 1u);
    return x < y ? x : y;
}

int main(int argc, char **argv) {
    if (argc != 9) { fprintf(stderr, "usage: flip_cpu STEPS SPANS SEGLEN LINKS ALIGN OUT_STEPS OUT_TURNED OUT_LINKS\n"); return 2; }
    const std::vector<uint32_t> steps = read_words(argv[1]), spans = read_words(argv[2]), seg_len = read_words(argv[3]), links = read_words(argv[4]),
                                align = read_words(argv[5]);
    g_align = align.data();
    const size_t P = spans.size() / 2, L = links.size() / 4, S = seg_len.size(), A = align.size();
    uint64_t n_lin = 0;
    for (size_t p = 0; p < P; ++p) {
        if (spans[2 * p] > spans[2 * p + 1] || spans[2 * p + 1] > steps.size()) { fprintf(stderr, "flip_cpu: path %zu has a span outside the steps\n", p); return 3; }
        for (uint32_t i = spans[2 * p]; i < spans[2 * p + 1]; ++i)
            if ((steps[i] >> 1) >= S) { fprintf(stderr, "flip_cpu: a step names no segment\n"); return 3; }
        n_lin += spans[2 * p + 1] - spans[2 * p];
    }
    for (size_t l = 0; l < L; ++l)
        if ((links[4 * l] >> 1) >= S || (links[4 * l + 1] >> 1) >= S || links[4 * l + 2] > links[4 * l + 3] || links[4 * l + 3] > A) {
            fprintf(stderr, "flip_cpu: link %zu is out of range\n", l);
            return 3;
        }
    std::vector<uint32_t> out(n_lin ? n_lin : 1), kept;  // (touched before the clock starts)
    memset(out.data(), 0, out.size() * 4);
    kept.reserve(4 * (L + n_lin));
    std::vector<uint8_t> turned(P ? P : 1, 0);
    const auto t0 = std::chrono::steady_clock::now();
    std::unordered_set<Cls, ClsHash> seen;
    seen.reserve(L + n_lin / 2);
    for (size_t l = 0; l < L; ++l) {  // flip.py:33-40 over the old links
        const uint32_t *r = &links[4 * l];
        if (seen.insert(Cls{canon(r[0], r[1]), g_align + r[2], r[3] - r[2]}).second) kept.insert(kept.end(), r, r + 4);
    }
    const size_t old_kept = kept.size() / 4;
    uint64_t at = 0, n_turned = 0;
    for (size_t p = 0; p < P; ++p) {
        const uint32_t b = spans[2 * p], e = spans[2 * p + 1];
        uint64_t fwd = 0, rev = 0;
        for (uint32_t i = b; i < e; ++i) ((steps[i] & 1u) ? rev : fwd) += seg_len[steps[i] >> 1];  // flip.py:6-16
        uint32_t *o = out.data() + at;
        if (rev > fwd) {
            turned[p] = 1, ++n_turned;
            for (uint32_t i = 0; i < e - b; ++i) o[i] = steps[e - 1 - i] ^ 1u;  // flip.py:24-26
            for (uint32_t i = 0; i + 1 < e - b; ++i)                            // flip.py:61-67
                if (seen.insert(Cls{canon(o[i], o[i + 1]), &kZeroM, 1}).second) {
                    const uint32_t rec[4] = {o[i], o[i + 1], (uint32_t)A, (uint32_t)A + 1};
                    kept.insert(kept.end(), rec, rec + 4);
                }
        } else if (e > b) {
            memcpy(o, steps.data() + b, (size_t)(e - b) * 4);
        }
        at += e - b;
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    write_bytes(argv[6], out.data(), (size_t)n_lin * 4);
    write_bytes(argv[7], turned.data(), P);
    write_bytes(argv[8], kept.data(), kept.size() * 4);
    printf("%llu %zu %zu %.6f\n", (unsigned long long)n_turned, kept.size() / 4, kept.size() / 4 - old_kept, sec);
    return 0;
}
