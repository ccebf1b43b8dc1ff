// A single-thread restatement of the reference's GAF lookup (flatgfa/src/ops/gaf.rs, `fgfa gaf GAF -s` / `-b`,
// cli/cmds.rs:311-376), the stand-in for the Rust binary in tools/gaf_lookup_bench.py.  Build: g++ -O3 -march=native.
//
//   gaf_lookup_cpu NAMES.u64 SEQ_START.u32 SEQ_LEN.u32 SEQ_DATA GAF (-s OUT | -b)
//
// -s writes name, tab, bases, newline per read to OUT; -b prints the number of events.  The seconds from the first line to the
// last byte of the answer in memory go to stderr (the files are mapped and read once before, so neither side pays for the disk).
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <string>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <unordered_map>
#include <vector>

struct Map {
    const uint8_t *p = nullptr;
    size_t n = 0;
};
static Map map_file(const char *path) {
    Map m;
    const int fd = open(path, O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) != 0) { fprintf(stderr, "cannot open %s\n", path); exit(1); }
    m.n = (size_t)sb.st_size;
    m.p = m.n ? (const uint8_t *)mmap(nullptr, m.n, PROT_READ, MAP_PRIVATE | MAP_POPULATE, fd, 0) : nullptr;
    close(fd);
    return m;
}

static uint8_t comp[256];

int main(int argc, char **argv) {
    if (argc < 7) { fprintf(stderr, "usage: gaf_lookup_cpu NAMES SEQ_START SEQ_LEN SEQ_DATA GAF (-s OUT | -b)\n"); return 2; }
    const Map names = map_file(argv[1]), st = map_file(argv[2]), ln = map_file(argv[3]), seq = map_file(argv[4]), gaf = map_file(argv[5]);
    const bool count_only = !strcmp(argv[6], "-b");
    const size_t S = names.n / 8;
    const uint64_t *name = (const uint64_t *)names.p;
    const uint32_t *seq_start = (const uint32_t *)st.p, *seq_len = (const uint32_t *)ln.p;
    // NameMap::build (namemap.rs:36-42)
    uint64_t seq_max = 0;
    std::unordered_map<uint64_t, uint32_t> others;
    for (size_t i = 0; i < S; ++i) {
        if (name[i] - 1 == seq_max && name[i] - 1 == i) ++seq_max;
        else others[name[i]] = (uint32_t)i;
    }
    for (int c = 0; c < 256; ++c) comp[c] = (uint8_t)c;
    const char *from = "ACGTacgt", *to = "TGCAtgca";
    for (int k = 0; k < 8; ++k) comp[(uint8_t)from[k]] = (uint8_t)to[k];
    uint64_t sink = 0;
    for (size_t i = 0; i < gaf.n; i += 4096) sink += gaf.p[i];  // (touched once before the clock starts)

    const auto t0 = std::chrono::steady_clock::now();
    std::string out;
    if (!count_only) out.reserve(gaf.n);
    uint64_t events = 0;
    const uint8_t *p = gaf.p, *end = gaf.p + gaf.n;
    auto digits = [](const uint8_t *&q, const uint8_t *e, uint64_t *v) {  // gaf.rs:264-285
        const uint8_t *b = q;
        uint64_t n = 0;
        while (q < e && (unsigned)(*q - '0') < 10u) n = n * 10 + (*q++ - '0');
        *v = n;
        return q > b;
    };
    while (p < end) {
        const uint8_t *nl = (const uint8_t *)memchr(p, '\n', (size_t)(end - p));
        if (!nl) break;  // memfile.rs:51-63: what follows the last '\n' is not a line
        const uint8_t *f[10];
        const uint8_t *q = p;
        int tabs = 0;
        while (tabs < 9) {
            const uint8_t *t = (const uint8_t *)memchr(q, '\t', (size_t)(nl - q));
            if (!t) break;
            f[tabs++] = t;
            q = t + 1;
        }
        uint64_t start = 0, stop = 0;
        const uint8_t *a = tabs >= 9 ? f[6] + 1 : nl, *b = tabs >= 9 ? f[7] + 1 : nl;
        if (tabs < 9 || !digits(a, nl, &start) || a != f[7] || !digits(b, nl, &stop) || b != f[8]) {
            fprintf(stderr, "malformed line at %zu\n", (size_t)(p - gaf.p));
            return 1;
        }
        if (!count_only) out.append((const char *)p, (size_t)(f[0] - p + 1));  // the name and its tab
        uint64_t pos = 0;
        bool started = false, ended = false;
        for (const uint8_t *t = f[4] + 1; t < f[5];) {  // gaf.rs:287-308
            const uint8_t dir = *t++;
            if (dir != '>' && dir != '<') break;
            uint64_t nm;
            if (!digits(t, f[5], &nm)) break;
            uint32_t id;
            if (nm <= seq_max) id = (uint32_t)(nm - 1);
            else {
                auto it = others.find(nm);
                id = it == others.end() ? 0xFFFFFFFFu : it->second;
            }
            if (id >= S) { fprintf(stderr, "unknown name at %zu\n", (size_t)(p - gaf.p)); return 1; }
            const uint64_t len = seq_len[id], next = pos + len;
            uint64_t ra = 0, rb = 0;  // gaf.rs:200-243
            if (!started && start < next) {
                started = true;
                ra = start - pos;
                if (stop < next) { ended = true; rb = stop - pos; } else rb = len;
            } else if (started && !ended && stop < next) {
                ended = true;
                rb = stop - pos;
            } else if (started && !ended) {
                rb = len;
            }
            pos = next;
            ++events;
            if (count_only || ra == rb) continue;
            if (ra > rb || rb > len) { fprintf(stderr, "bad range at %zu\n", (size_t)(p - gaf.p)); return 1; }
            const uint8_t *sq = seq.p + seq_start[id];
            if (dir == '>') out.append((const char *)sq + ra, (size_t)(rb - ra));
            else {
                const size_t at = out.size();
                out.resize(at + (size_t)(rb - ra));
                char *o = &out[at];
                for (uint64_t k = 0; k < rb - ra; ++k) o[k] = (char)comp[sq[len - ra - 1 - k]];
            }
        }
        if (!count_only) out.push_back('\n');
        p = nl + 1;
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    fprintf(stderr, "lookup_seconds=%.6f\n", s + (double)(sink & 0));
    if (count_only) printf("%llu\n", (unsigned long long)events);
    else {
        FILE *o = fopen(argv[7], "wb");
        if (!o || fwrite(out.data(), 1, out.size(), o) != out.size()) { fprintf(stderr, "cannot write %s\n", argv[7]); return 1; }
        fclose(o);
    }
    return 0;
}
