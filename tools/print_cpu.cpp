// A single-thread restatement of the GFA printer (flatgfa/src/print.rs:99-153) over the eleven pools, memory to memory: the
// yardstick of tools/print_bench.py.  Stand-alone: it includes nothing of the library.
//
//   g++ -O3 -march=native -std=c++17 -shared -fPIC tools/print_cpu.cpp -o print_cpu.so
//
// The pools come in the container's order and layout (file.rs:14-27): header, segs (u64 name, the sequence span, the
// optional span: 24 bytes), paths (name, steps, overlaps spans: 24 bytes), links (from, to, the overlap's span: 16 bytes),
// steps, seq_data, overlaps (spans), alignment, name_data, optional_data, line_order.  The spans are trusted (the library
// has checked them when it loaded the graph).  The text is sized first and written second, so that no buffer grows; the
// seconds are those of both passes.
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace {

struct Graph {
    const uint8_t *header, *seq, *names, *opt, *order;
    const uint8_t *segs, *paths, *links;
    const uint32_t *steps, *overlaps, *align;
    uint64_t n_header, n_segs, n_paths, n_links, n_order;
};

inline uint32_t u32_at(const uint8_t *p) {
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}
inline uint64_t u64_at(const uint8_t *p) {
    uint64_t v;
    memcpy(&v, p, 8);
    return v;
}
inline unsigned digits(uint64_t x) {
    unsigned n = 1;
    while (x >= 10) x /= 10, ++n;
    return n;
}

// Writes when kWrite, else only advances: one body for the sizing pass and the writing pass.
template <bool kWrite>
struct Out {
    char *base;
    size_t at = 0;
    void ch(char c) {
        if (kWrite) base[at] = c;
        ++at;
    }
    void bytes(const uint8_t *s, size_t n) {
        if (kWrite) memcpy(base + at, s, n);
        at += n;
    }
    void num(uint64_t x) {
        const unsigned n = digits(x);
        if (kWrite)
            for (char *p = base + at, *q = p + n; q != p; x /= 10) *--q = (char)('0' + x % 10);
        at += n;
    }
};

template <bool kWrite>
void alignment(const Graph &g, uint32_t a0, uint32_t a1, Out<kWrite> &o) {
    if (a0 == a1) o.ch('0'), o.ch('M');  // print.rs:26-28
    for (uint32_t a = a0; a < a1; ++a) o.num(g.align[a] >> 8), o.ch("MNDI"[g.align[a] & 3]);  // print.rs:29-31, :16-19
}
template <bool kWrite>
void handle(const Graph &g, uint32_t h, Out<kWrite> &o) {
    o.num(u64_at(g.segs + 24 * (uint64_t)(h >> 1))), o.ch((h & 1) ? '-' : '+');  // print.rs:41-43
}
template <bool kWrite>
void segment(const Graph &g, uint64_t i, Out<kWrite> &o) {  // print.rs:89-94
    const uint8_t *s = g.segs + 24 * i;
    o.ch('S'), o.ch('\t'), o.num(u64_at(s)), o.ch('\t');
    o.bytes(g.seq + u32_at(s + 8), u32_at(s + 12) - u32_at(s + 8));
    if (u32_at(s + 16) != u32_at(s + 20)) o.ch('\t'), o.bytes(g.opt + u32_at(s + 16), u32_at(s + 20) - u32_at(s + 16));
    o.ch('\n');
}
template <bool kWrite>
bool path(const Graph &g, uint64_t i, Out<kWrite> &o) {  // print.rs:48-66
    const uint8_t *r = g.paths + 24 * i;
    const uint32_t s0 = u32_at(r + 8), s1 = u32_at(r + 12), o0 = u32_at(r + 16), o1 = u32_at(r + 20);
    o.ch('P'), o.ch('\t'), o.bytes(g.names + u32_at(r), u32_at(r + 4) - u32_at(r)), o.ch('\t');
    if (s0 == s1) return false;  // steps[0]
    for (uint32_t k = s0; k < s1; ++k) {
        if (k != s0) o.ch(',');
        handle(g, g.steps[k], o);
    }
    o.ch('\t');
    if (o0 == o1) o.ch('*');
    for (uint32_t k = o0; k < o1; ++k) {
        if (k != o0) o.ch(',');
        alignment(g, g.overlaps[2 * (uint64_t)k], g.overlaps[2 * (uint64_t)k + 1], o);
    }
    o.ch('\n');
    return true;
}
template <bool kWrite>
void link(const Graph &g, uint64_t i, Out<kWrite> &o) {  // print.rs:70-84
    const uint8_t *r = g.links + 16 * i;
    const uint32_t from = u32_at(r), to = u32_at(r + 4);
    o.ch('L'), o.ch('\t'), o.num(u64_at(g.segs + 24 * (uint64_t)(from >> 1))), o.ch('\t'), o.ch((from & 1) ? '-' : '+'), o.ch('\t');
    o.num(u64_at(g.segs + 24 * (uint64_t)(to >> 1))), o.ch('\t'), o.ch((to & 1) ? '-' : '+'), o.ch('\t');
    alignment(g, u32_at(r + 8), u32_at(r + 12), o);
    o.ch('\n');
}
template <bool kWrite>
void header(const Graph &g, Out<kWrite> &o) {
    o.ch('H'), o.ch('\t'), o.bytes(g.header, g.n_header), o.ch('\n');  // print.rs:108, :130
}

template <bool kWrite>
bool print(const Graph &g, Out<kWrite> &o) {
    if (!g.n_order) {  // write_normalized, print.rs:128-142
        if (g.n_header) header(g, o);
        for (uint64_t i = 0; i < g.n_segs; ++i) segment(g, i, o);
        for (uint64_t i = 0; i < g.n_paths; ++i)
            if (!path(g, i, o)) return false;
        for (uint64_t i = 0; i < g.n_links; ++i) link(g, i, o);
        return true;
    }
    uint64_t si = 0, pi = 0, li = 0;  // write_preserved, print.rs:99-125
    for (uint64_t k = 0; k < g.n_order; ++k) {
        switch (g.order[k]) {
            case 0:
                if (!g.n_header) return false;
                header(g, o);
                break;
            case 1:
                if (si >= g.n_segs) return false;
                segment(g, si++, o);
                break;
            case 2:
                if (pi >= g.n_paths || !path(g, pi++, o)) return false;
                break;
            case 3:
                if (li >= g.n_links) return false;
                link(g, li++, o);
                break;
            default:
                return false;
        }
    }
    return true;
}

}  // namespace

// pools[11], lens[11] (elements) in the container's order.  0: *text is malloc'd (print_cpu_free), *n its length, *seconds the
// time of both passes.  1: the reference would have panicked.  2: out of memory.
extern "C" int print_cpu(const void *const *pools, const uint64_t *lens, char **text, size_t *n, double *seconds) {
    Graph g;
    g.header = (const uint8_t *)pools[0], g.n_header = lens[0];
    g.segs = (const uint8_t *)pools[1], g.n_segs = lens[1];
    g.paths = (const uint8_t *)pools[2], g.n_paths = lens[2];
    g.links = (const uint8_t *)pools[3], g.n_links = lens[3];
    g.steps = (const uint32_t *)pools[4], g.seq = (const uint8_t *)pools[5], g.overlaps = (const uint32_t *)pools[6];
    g.align = (const uint32_t *)pools[7], g.names = (const uint8_t *)pools[8], g.opt = (const uint8_t *)pools[9];
    g.order = (const uint8_t *)pools[10], g.n_order = lens[10];
    const auto t0 = std::chrono::steady_clock::now();
    Out<false> size{nullptr};
    if (!print(g, size)) return 1;
    const size_t bytes = size.at;
    char *buf = (char *)malloc(bytes + 1);
    if (!buf) return 2;
    Out<true> out{buf};
    (void)print(g, out);
    *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    *text = buf, *n = bytes;
    return 0;
}

extern "C" void print_cpu_free(char *text) { free(text); }
