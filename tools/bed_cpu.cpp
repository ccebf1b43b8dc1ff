// `fgfa bed -a A -b B` on one CPU thread, with the SAME method as the device (pollen_amd/csrc/bed_device.hpp): B's names
// interned and B grouped by name, stably; per group whether its starts never decrease, and the running maximum of `end`; per
// A entry two bisections for its candidate range, or the whole group where the group is not sorted; then the exact test and
// the line.  What tools/bed_bench.py times the GPU route against -- not the reference's double loop over all pairs -- and
// what tests/test_bed_cpu_tool.py holds against tests/bed_model.py.
//
//   g++ -O3 -march=native -std=c++17 -shared -fPIC tools/bed_cpu.cpp -o bed_cpu.so
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string_view>
#include <unordered_map>
#include <vector>

namespace {

struct Entry {
    std::string_view name;
    uint64_t start, end;
};

// flatbed.rs:125-158 over memfile.rs:51-63; false where the reference panics
bool parse(const uint8_t *buf, size_t n, std::vector<Entry> *out) {
    size_t pos = 0;
    while (pos < n) {
        const uint8_t *nl = (const uint8_t *)memchr(buf + pos, '\n', n - pos);
        if (!nl) break;  // an unterminated last line is dropped
        const uint8_t *p = buf + pos, *e = nl;
        pos = (size_t)(nl - buf) + 1;
        if (p < e && *p == '#') continue;
        const uint8_t *t = (const uint8_t *)memchr(p, '\t', (size_t)(e - p));
        const uint8_t *name_end = t ? t : e, *q = t ? t + 1 : e, *s = q;
        uint64_t start = 0, end = 0;
        while (s < e && *s >= '0' && *s <= '9') start = start * 10 + (uint64_t)(*s++ - '0');
        if (s == q || s >= e) return false;
        const uint8_t *r = ++s;
        while (s < e && *s >= '0' && *s <= '9') end = end * 10 + (uint64_t)(*s++ - '0');
        if (s == r) return false;
        out->push_back(Entry{std::string_view((const char *)p, (size_t)(name_end - p)), start, end});
    }
    return true;
}

struct Text {
    char *buf = nullptr;
    size_t cap = 0, at = 0;
    bool room(size_t n) {
        if (n <= cap - at) return true;
        const size_t want = cap * 2 > at + n ? cap * 2 : at + n + (1 << 20);
        char *p = (char *)realloc(buf, want);
        if (!p) return false;
        buf = p, cap = want;
        return true;
    }
    void number(uint64_t x) {
        char tmp[20];
        int k = 0;
        do tmp[k++] = (char)('0' + x % 10);
        while (x /= 10);
        while (k) buf[at++] = tmp[--k];
    }
};

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

// stats: lines, bytes, candidates, unsorted groups.  secs: parse, intern and group, intersect and print.
// 0, or 1 where a text does not parse, 2 out of memory.  *text is malloc'd (bed_cpu_free).
extern "C" int bed_cpu(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, char **text, size_t *len, uint64_t *stats, double *secs) {
    *text = nullptr, *len = 0;
    const double t0 = now();
    std::vector<Entry> A, B;
    if (!parse(a, a_len, &A) || !parse(b, b_len, &B)) return 1;
    const double t1 = now();
    std::unordered_map<std::string_view, uint32_t> ids;
    std::vector<uint32_t> bid(B.size()), gstart(1, 0);
    {
        std::string_view last;
        uint32_t last_id = 0;
        for (size_t i = 0; i < B.size(); ++i) {
            if (!i || B[i].name != last) {
                const auto got = ids.emplace(B[i].name, (uint32_t)ids.size());
                if (got.second) gstart.push_back(0);
                last = B[i].name, last_id = got.first->second;
            }
            bid[i] = last_id;
            ++gstart[last_id + 1];
        }
    }
    const size_t G = ids.size();
    for (size_t g = 0; g < G; ++g) gstart[g + 1] += gstart[g];
    std::vector<uint64_t> bs(B.size()), be(B.size()), runmax(B.size());
    std::vector<std::string_view> gname(G);
    std::vector<uint8_t> unsorted(G, 0);
    {
        std::vector<uint32_t> next(gstart.begin(), gstart.end() - 1);
        for (size_t i = 0; i < B.size(); ++i) {
            const uint32_t at = next[bid[i]]++;
            bs[at] = B[i].start, be[at] = B[i].end;
            gname[bid[i]] = B[i].name;
        }
    }
    uint64_t n_unsorted = 0;
    for (size_t g = 0; g < G; ++g) {
        for (uint32_t i = gstart[g]; i < gstart[g + 1]; ++i) {
            const bool head = i == gstart[g];
            if (!head && bs[i] < bs[i - 1]) unsorted[g] = 1;
            runmax[i] = head || be[i] > runmax[i - 1] ? be[i] : runmax[i - 1];
        }
        n_unsorted += unsorted[g];
    }
    const double t2 = now();
    Text out;
    uint64_t lines = 0, cands = 0;
    std::string_view last;
    uint32_t g = 0;
    bool have = false;
    for (size_t i = 0; i < A.size(); ++i) {
        if (!i || A[i].name != last) {
            const auto it = ids.find(A[i].name);
            last = A[i].name, have = it != ids.end(), g = have ? it->second : 0;
        }
        const uint64_t as = A[i].start, ae = A[i].end;
        if (!have || as >= ae) continue;
        uint32_t lo = gstart[g], hi = gstart[g + 1];
        if (!unsorted[g]) {
            uint32_t l = lo, h = hi;
            while (l < h) {  // the first entry whose running maximum of `end` is past a.start
                const uint32_t mid = l + ((h - l) >> 1);
                if (runmax[mid] > as) h = mid;
                else l = mid + 1;
            }
            const uint32_t first = l;
            l = lo, h = hi;
            while (l < h) {  // the first entry that starts at or past a.end
                const uint32_t mid = l + ((h - l) >> 1);
                if (bs[mid] >= ae) h = mid;
                else l = mid + 1;
            }
            lo = first, hi = l;
        }
        if (hi <= lo) continue;
        cands += hi - lo;
        const std::string_view nm = gname[g];
        for (uint32_t x = lo; x < hi; ++x) {
            const uint64_t s = bs[x] < as ? as : bs[x], e = ae < be[x] ? ae : be[x];
            if (e <= s) continue;
            if (!out.room(nm.size() + 43)) {
                free(out.buf);
                return 2;
            }
            memcpy(out.buf + out.at, nm.data(), nm.size());
            out.at += nm.size();
            out.buf[out.at++] = '\t';
            out.number(s);
            out.buf[out.at++] = '\t';
            out.number(e);
            out.buf[out.at++] = '\n';
            ++lines;
        }
    }
    const double t3 = now();
    stats[0] = lines, stats[1] = out.at, stats[2] = cands, stats[3] = n_unsorted;
    secs[0] = t1 - t0, secs[1] = t2 - t1, secs[2] = t3 - t2;
    *text = out.buf, *len = out.at;
    return 0;
}

extern "C" void bed_cpu_free(char *text) { free(text); }

// The bench's synthetic BED text (tools/bed_bench.py), memory to memory: per name "chr1" .. "chr<names>", first the one
// interval [0, front_end) if front_end != 0, then per_name intervals [at + i * step, at + i * step + width).  Returns the
// bytes written; out == NULL: the bytes needed, at most.
extern "C" size_t bed_synth(char *out, uint32_t names, uint64_t per_name, uint64_t at, uint64_t step, uint64_t width, uint64_t front_end) {
    if (!out) return (size_t)names * (per_name + 1) * 50;
    Text t;
    t.buf = out, t.cap = (size_t)-1;
    for (uint32_t n = 1; n <= names; ++n) {
        for (uint64_t i = front_end ? 0 : 1; i <= per_name; ++i) {
            const uint64_t s = i ? at + (i - 1) * step : 0, e = i ? s + width : front_end;
            memcpy(t.buf + t.at, "chr", 3);
            t.at += 3;
            t.number(n);
            t.buf[t.at++] = '\t';
            t.number(s);
            t.buf[t.at++] = '\t';
            t.number(e);
            t.buf[t.at++] = '\n';
        }
    }
    return t.at;
}
