// A single-thread C++ restatement of chop (flatgfa/src/ops/chop.rs, without links) over a .flatgfa file, for
// tools/chop_bench.py: prints the new step count, segment count and the steps' checksum (as chop_bench.py's).
//   g++ -O3 -std=c++17 tools/chop_cpu.cpp -o chop_cpu && ./chop_cpu G.flatgfa C
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: chop_cpu G.flatgfa C\n"); return 2; }
    const uint64_t c = strtoull(argv[2], nullptr, 10);
    const int fd = open(argv[1], O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) || c == 0) return 1;
    const uint8_t *m = (const uint8_t *)mmap(nullptr, sb.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    // file.rs:14-38: magic, 11 x {len, capacity}, then the pools at their capacities
    uint64_t toc[23];
    memcpy(toc, m, sizeof toc);
    static const size_t es[11] = {1, 24, 24, 16, 4, 1, 8, 4, 1, 1, 1};
    const uint8_t *pool[11];
    size_t at = sizeof toc;
    for (int i = 0; i < 11; ++i) pool[i] = m + at, at += toc[2 + 2 * i] * es[i];
    const uint64_t S = toc[3], P = toc[5];
    std::vector<uint32_t> first(S + 1);  // chop.rs:25-66
    for (uint64_t s = 0; s < S; ++s) {
        uint32_t b, e;
        memcpy(&b, pool[1] + s * 24 + 8, 4);
        memcpy(&e, pool[1] + s * 24 + 12, 4);
        const uint64_t len = e - b;
        first[s + 1] = first[s] + (uint32_t)(len <= c ? 1 : (len - 1) / c + 1);
    }
    std::vector<uint32_t> out;  // chop.rs:68-104
    for (uint64_t p = 0; p < P; ++p) {
        uint32_t b, e;
        memcpy(&b, pool[2] + p * 24 + 8, 4);
        memcpy(&e, pool[2] + p * 24 + 12, 4);
        for (uint32_t i = b; i < e; ++i) {
            uint32_t h;
            memcpy(&h, pool[4] + (size_t)i * 4, 4);
            const uint32_t s = h >> 1, a = first[s], z = first[s + 1];
            if (h & 1)
                for (uint32_t k = z; k-- > a;) out.push_back((k << 1) | 1);
            else
                for (uint32_t k = a; k < z; ++k) out.push_back(k << 1);
        }
    }
    uint64_t sum = 0;
    for (size_t i = 0; i < out.size(); ++i) sum ^= (uint64_t)out[i] * 0x9E3779B97F4A7C15ull + i;
    printf("%zu %u %llu\n", out.size(), first[S], (unsigned long long)sum);
    return 0;
}
