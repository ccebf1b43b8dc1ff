// A single-thread C++ restatement of the reference's pangenotype matrix (flatgfa/src/ops/pangenotype.rs:11-70 with
// flatgfa/src/namemap.rs), the CPU baseline of tools/pangenotype_bench.py.
//
//   pangenotype_cpu NAMES.u64 GAF   -> the bytes `fgfa matrix GAF` prints
//
// NAMES.u64: the graph's segment names in id order, little-endian u64.  Exit status 101 where the reference panics.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

static const uint8_t *map_file(const char *path, size_t *n) {
    const int fd = open(path, O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) != 0) { fprintf(stderr, "cannot open %s\n", path); exit(1); }
    *n = (size_t)sb.st_size;
    void *m = *n ? mmap(nullptr, *n, PROT_READ, MAP_PRIVATE, fd, 0) : nullptr;
    close(fd);
    if (m == MAP_FAILED) { fprintf(stderr, "cannot map %s\n", path); exit(1); }
    return (const uint8_t *)m;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: pangenotype_cpu NAMES.u64 GAF\n"); return 2; }
    size_t nb = 0, n = 0;
    const uint8_t *nm = map_file(argv[1], &nb);
    const size_t S = nb / 8;
    // NameMap::build (namemap.rs:17-42)
    uint64_t seq_max = 0;
    std::unordered_map<uint64_t, uint32_t> others;
    for (size_t i = 0; i < S; ++i) {
        uint64_t name;
        memcpy(&name, nm + 8 * i, 8);
        if (name - 1 == seq_max && name - 1 == i) ++seq_max;
        else others[name] = (uint32_t)i;
    }
    std::vector<uint8_t> row(S, 0);
    const uint8_t *t = map_file(argv[2], &n);
    size_t start = 0;
    while (start < n) {
        const void *q = memchr(t + start, '\n', n - start);
        if (!q) break;
        const size_t line_end = (size_t)((const uint8_t *)q - t);
        const uint8_t *line = t + start;
        const size_t len = line_end - start;
        start = line_end + 1;
        if (len == 0 || line[0] == '#') continue;
        size_t tabs = 0, idx = 0;
        while (idx < len && tabs < 5) {
            if (line[idx] == '\t') ++tabs;
            ++idx;
        }
        if (tabs < 5 || idx >= len) continue;
        size_t end = idx;
        while (end < len && line[end] != '\t') ++end;
        for (size_t p = idx; p < end;) {
            const uint8_t b = line[p];
            if (b == '>' || b == '<') {
                ++p;
                uint64_t num = 0;
                while (p < end && line[p] >= '0' && line[p] <= '9') num = num * 10 + (uint64_t)(line[p++] - '0');
                uint32_t id;
                if (num <= seq_max) {
                    id = (uint32_t)(num - 1);
                } else {
                    auto it = others.find(num);
                    if (it == others.end()) { fprintf(stderr, "panic: name %llu not in the graph\n", (unsigned long long)num); return 101; }
                    id = it->second;
                }
                if (id >= S) { fprintf(stderr, "panic: index %u out of bounds\n", id); return 101; }
                row[id] = 1;
            } else {
                ++p;
            }
        }
    }
    std::string out(S + 1, '\n');
    for (size_t s = 0; s < S; ++s) out[s] = row[s] ? '1' : '0';
    fwrite(out.data(), 1, out.size(), stdout);
    return 0;
}
