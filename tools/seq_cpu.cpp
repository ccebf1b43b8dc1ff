// A single-thread C++ restatement of the packed-sequence codec (flatgfa/src/packedseq.rs) for
// tools/seq_bench.py and tests/test_seq_cpu_tool.py.
//   seq_cpu export TEXT OUT    the file image `fgfa seq-export` writes for TEXT; prints the bases and the seconds the packing
//                              took, memory to memory, without reading or writing the files.  A byte that is neither
//                              whitespace nor one of A C T G: exit status 3, its offset on stderr, no OUT.
//   seq_cpu import FILE OUT    the bases of a packed file (no newline); prints the bases and the seconds.  A malformed header
//                              or a nibble above 3: exit status 3.
//   g++ -O3 -std=c++17 tools/seq_cpu.cpp -o seq_cpu
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
    if (fd < 0 || fstat(fd, &sb)) { fprintf(stderr, "seq_cpu: cannot open %s\n", path); exit(1); }
    *n = (size_t)sb.st_size;
    const void *m = *n ? mmap(nullptr, *n, PROT_READ, MAP_PRIVATE | MAP_POPULATE, fd, 0) : (const void *)"";
    if (m == MAP_FAILED) { fprintf(stderr, "seq_cpu: cannot map %s\n", path); exit(1); }
    return (const uint8_t *)m;
}

static void put_le64(uint8_t *p, uint64_t v) {
    for (int k = 0; k < 8; ++k) p[k] = (uint8_t)(v >> (8 * k));
}
static uint64_t get_le64(const uint8_t *p) {
    uint64_t v = 0;
    for (int k = 0; k < 8; ++k) v |= (uint64_t)p[k] << (8 * k);
    return v;
}

static int write_out(const char *path, const uint8_t *p, size_t n) {
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(p, 1, n, f) != n || fclose(f)) { fprintf(stderr, "seq_cpu: cannot write %s\n", path); return 1; }
    return 0;
}

static double since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

int main(int argc, char **argv) {
    if (argc != 4 || (strcmp(argv[1], "export") && strcmp(argv[1], "import"))) {
        fprintf(stderr, "usage: seq_cpu export TEXT OUT | seq_cpu import FILE OUT\n");
        return 2;
    }
    size_t n = 0;
    const uint8_t *in = map_file(argv[2], &n);
    if (!strcmp(argv[1], "export")) {
        int8_t code[256];  // -1: not a nucleotide, -2: whitespace
        memset(code, -1, sizeof code);
        code['A'] = 0, code['C'] = 1, code['T'] = 2, code['G'] = 3;
        for (const char *w = " \t\n\x0c\r"; *w; ++w) code[(uint8_t)*w] = -2;
        std::vector<uint8_t> out(25 + n / 2 + 1);  // (touched before the clock starts)
        memset(out.data(), 0, out.size());
        const auto t0 = std::chrono::steady_clock::now();
        uint8_t *data = out.data() + 25;
        uint64_t bases = 0;
        for (size_t i = 0; i < n; ++i) {  // packedseq.rs:293-304, a push a nucleotide
            const int c = code[in[i]];
            if (c == -2) continue;
            if (c < 0) { fprintf(stderr, "seq_cpu: byte 0x%02x at offset %zu is not a nucleotide\n", in[i], i); return 3; }
            if (bases & 1) data[bases >> 1] |= (uint8_t)(c << 4);
            else data[bases >> 1] = (uint8_t)c;
            ++bases;
        }
        const double sec = since(t0);
        const uint64_t len = bases / 2 + (bases & 1);
        put_le64(out.data(), 0x12), put_le64(out.data() + 8, len), put_le64(out.data() + 16, len);
        out[24] = bases & 1 ? 0 : 1;
        if (write_out(argv[3], out.data(), 25 + len)) return 1;
        printf("%llu %.6f\n", (unsigned long long)bases, sec);
        return 0;
    }
    if (n < 25) { fprintf(stderr, "seq_cpu: shorter than the header\n"); return 3; }
    const uint64_t magic = get_le64(in), len = get_le64(in + 8), cap = get_le64(in + 16);
    const uint8_t hne = in[24];
    if (magic != 0x12 || hne > 1 || cap < len || cap > n - 25 || (len == 0 && hne == 0)) { fprintf(stderr, "seq_cpu: malformed header\n"); return 3; }
    const uint64_t bases = 2 * len - (1 - hne);
    std::vector<uint8_t> out(bases ? bases : 1);
    memset(out.data(), 0, out.size());
    const auto t0 = std::chrono::steady_clock::now();
    const uint8_t *data = in + 25;
    for (uint64_t i = 0; i < bases; ++i) {  // packedseq.rs:199-206, a get a nucleotide
        const uint8_t nib = i & 1 ? data[i >> 1] >> 4 : data[i >> 1] & 0xF;
        if (nib > 3) { fprintf(stderr, "seq_cpu: nibble %u at base %llu is not a nucleotide\n", nib, (unsigned long long)i); return 3; }
        out[i] = (uint8_t)"ACTG"[nib];
    }
    const double sec = since(t0);
    if (write_out(argv[3], out.data(), bases)) return 1;
    printf("%llu %.6f\n", (unsigned long long)bases, sec);
    return 0;
}
