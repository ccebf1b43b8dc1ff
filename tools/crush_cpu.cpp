// A single-thread C++ restatement of crush (slow_odgi/slow_odgi/crush.py) over a sequence pool and its
// segments' spans as the device-level entry takes them, for tools/crush_bench.py and tests/test_crush_cpu_tool.py: SPANS holds
// u32 pairs (start, length), POOL the bases; the crushed segments are written one behind another in segment order to OUT, and
// the kept bytes, the dropped bytes, a checksum of the new lengths (as chop_bench.py's) and the seconds the work took without
// reading or writing the files are printed.  A span that leaves the pool: exit status 3.
//   g++ -O3 -std=c++17 tools/crush_cpu.cpp -o crush_cpu && ./crush_cpu SPANS.bin POOL.bin OUT.bin
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static const uint8_t *map_file(const char *path, size_t *n) {
    const int fd = open(path, O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb)) { fprintf(stderr, "crush_cpu: cannot open %s\n", path); exit(1); }
    *n = (size_t)sb.st_size;
    const void *m = *n ? mmap(nullptr, *n, PROT_READ, MAP_PRIVATE | MAP_POPULATE, fd, 0) : (const void *)"";
    if (m == MAP_FAILED) { fprintf(stderr, "crush_cpu: cannot map %s\n", path); exit(1); }
    return (const uint8_t *)m;
}

int main(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "usage: crush_cpu SPANS.bin POOL.bin OUT.bin\n"); return 2; }
    size_t sn = 0, pn = 0;
    const uint8_t *sp = map_file(argv[1], &sn);
    const uint8_t *pool = map_file(argv[2], &pn);
    const size_t S = sn / 8;
    std::vector<uint32_t> spans(2 * S);
    if (S) memcpy(spans.data(), sp, 2 * S * 4);
    uint64_t total = 0;
    for (size_t s = 0; s < S; ++s) {
        if ((uint64_t)spans[2 * s] + spans[2 * s + 1] > pn) { fprintf(stderr, "crush_cpu: segment %zu has a span outside the pool\n", s); return 3; }
        total += spans[2 * s + 1];
    }
    std::vector<uint8_t> out(total ? total : 1);  // (never more than the input; touched before the clock starts)
    memset(out.data(), 0, out.size());
    std::vector<uint32_t> len(S);
    const auto t0 = std::chrono::steady_clock::now();
    uint8_t *o = out.data();
    for (size_t s = 0; s < S; ++s) {  // crush.py:5-17
        const uint8_t *b = pool + spans[2 * s], *e = b + spans[2 * s + 1];
        uint8_t *const o0 = o;
        bool in_n = false;
        for (; b != e; ++b) {
            const bool n = *b == 'N';
            if (!(n && in_n)) *o++ = *b;
            in_n = n;
        }
        len[s] = (uint32_t)(o - o0);
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const uint64_t kept = (uint64_t)(o - out.data());
    uint64_t sum = 0;
    for (size_t i = 0; i < S; ++i) sum ^= (uint64_t)len[i] * 0x9E3779B97F4A7C15ull + i;
    FILE *f = fopen(argv[3], "wb");
    if (!f || fwrite(out.data(), 1, kept, f) != kept || fclose(f)) { fprintf(stderr, "crush_cpu: cannot write %s\n", argv[3]); return 1; }
    printf("%llu %llu %llu %.6f\n", (unsigned long long)kept, (unsigned long long)(total - kept), (unsigned long long)sum, sec);
    return 0;
}
