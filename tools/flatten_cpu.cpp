// A single-thread C++ restatement of slow_odgi/slow_odgi/flatten.py over the FlatGFA pools, for tools/flatten_bench.py: the
// comparison the GPU flatten is timed beside, never the code under test.  Built by the tool as a shared object
// (g++ -O3 -march=native -shared -fPIC) and called through ctypes; memory to memory, one thread, its own seconds measured inside.
//
//   legend  flatten.py:13-19   FASTA  flatten.py:44-46, 51-55   BED  flatten.py:23-41
#include <charconv>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {
double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
char *put(char *p, uint64_t x) { return std::to_chars(p, p + 20, x).ptr; }
}  // namespace

extern "C" {

// Every output is malloc'd (flatten_cpu_free); returns 0, or 1 when memory runs out.
int flatten_cpu(const uint32_t *seq_start, const uint32_t *seq_len, uint64_t n_segs, const uint8_t *seq, const uint32_t *steps,
                const uint32_t *pbegin, const uint32_t *pend, const uint32_t *name_start, const uint32_t *name_end, uint64_t n_paths,
                const uint8_t *name_data, const char *name, size_t name_len, char **fasta, size_t *fasta_len, char **bed, size_t *bed_len,
                double *fasta_s, double *bed_s) {
    // get_fasta_legend (flatten.py:5-20)
    double t0 = now();
    std::vector<uint64_t> legend(n_segs + 1, 0);
    for (uint64_t s = 0; s < n_segs; ++s) legend[s + 1] = legend[s] + seq_len[s];
    const uint64_t total = legend[n_segs];
    char *glued = (char *)malloc(total + 1);
    if (!glued) return 1;
    for (uint64_t s = 0; s < n_segs; ++s) memcpy(glued + legend[s], seq + seq_start[s], seq_len[s]);
    // ">" name, insert_newlines (flatten.py:44-46), print's newline
    const uint64_t lines = (total + 79) / 80;
    char *fa = (char *)malloc(name_len + 2 + total + lines + 2), *p = fa;
    if (!fa) return 1;
    *p++ = '>';
    memcpy(p, name, name_len), p += name_len;
    *p++ = '\n';
    for (uint64_t i = 0; i < total; i += 80) {
        const uint64_t n = total - i < 80 ? total - i : 80;
        if (i) *p++ = '\n';
        memcpy(p, glued + i, n), p += n;
    }
    *p++ = '\n';
    free(glued);
    *fasta = fa, *fasta_len = (size_t)(p - fa);
    *fasta_s = now() - t0;

    // print_bed (flatten.py:23-41)
    t0 = now();
    static const char head[] = "#name\tstart\tend\tpath.name\tstrand\tstep.rank\n";
    uint64_t cap = sizeof head;
    for (uint64_t k = 0; k < n_paths; ++k) cap += (uint64_t)(pend[k] - pbegin[k]) * (name_len + (name_end[k] - name_start[k]) + 20 + 20 + 10 + 7);
    char *b = (char *)malloc(cap + 1), *q = b;
    if (!b) return 1;
    memcpy(q, head, sizeof head - 1), q += sizeof head - 1;
    for (uint64_t k = 0; k < n_paths; ++k) {
        const uint8_t *pname = name_data + name_start[k];
        const size_t pn = name_end[k] - name_start[k];
        for (uint32_t i = pbegin[k]; i < pend[k]; ++i) {
            const uint32_t h = steps[i];
            memcpy(q, name, name_len), q += name_len;
            *q++ = '\t';
            q = put(q, legend[h >> 1]);
            *q++ = '\t';
            q = put(q, legend[(h >> 1) + 1]);
            *q++ = '\t';
            memcpy(q, pname, pn), q += pn;
            *q++ = '\t';
            *q++ = (h & 1) ? '-' : '+';
            *q++ = '\t';
            q = put(q, i - pbegin[k]);
            *q++ = '\n';
        }
    }
    *bed = b, *bed_len = (size_t)(q - b);
    *bed_s = now() - t0;
    return 0;
}

void flatten_cpu_free(char *p) { free(p); }
}
