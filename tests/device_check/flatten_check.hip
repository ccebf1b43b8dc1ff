// Runs the legend and the BED of pollen_amd/csrc/flatten_device.hpp on its own, on segment lengths that no host handle can
// hold: the BED reads no base, so four lengths that add up to more than 2^32 need no sequence pool behind them.
// `make -C pollen_amd/csrc flatten_check` builds it for gfx950 from the feature's source and the staged copies (host_copy.cpp);
// tests/test_gpu_flatten_large.py drives it.
//
//   flatten_check INPUT OUTPUT [CHUNK_LINES]
//
//   INPUT   text.  Line 1: NAME.  Line 2: the segment lengths, decimal, blank-separated.  Every further line: a path's name,
//           then its step handles ((segment << 1) | backward), decimal, blank-separated.
//   OUTPUT  "legend" and the legend's S + 1 offsets on one line, blank-separated; then the BED table as the sink received it.
//
// The program judges nothing: it writes what the device left and exits 0.  A HIP call or a flatten call that fails ends it at
// once with a non-zero status.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../pollen_amd/csrc/device_common.hpp"
#include "../../pollen_amd/csrc/flatten_device.hpp"
#include "../../pollen_amd/csrc/prof.hpp"

namespace fgfa_dev {
static std::string g_error;
void set_error(const std::string &s) { g_error = s; }
const char *last_error() { return g_error.c_str(); }
bool prof_enabled() { return false; }
void prof_push(const ProfRec &) {}
hipEvent_t prof_event_get() { return nullptr; }
void prof_event_put(hipEvent_t) {}
}  // namespace fgfa_dev

using namespace fgfa_dev;

[[noreturn]] static void fail(const std::string &what) {
    std::fprintf(stderr, "flatten_check: %s\n", what.c_str());
    std::exit(1);
}
#define CK(expr)                                                                      \
    do {                                                                              \
        hipError_t _e = (expr);                                                       \
        if (_e != hipSuccess) fail(std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

template <class T>
static T *to_device(const std::vector<T> &v) {
    T *d = nullptr;
    CK(hipMalloc((void **)&d, (v.size() ? v.size() : 1) * sizeof(T)));
    if (!v.empty()) CK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}

static int take(void *ctx, const char *bytes, size_t n) {
    static_cast<std::string *>(ctx)->append(bytes, n);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 3 && argc != 4) fail("usage: flatten_check INPUT OUTPUT [CHUNK_LINES]");
    std::ifstream in(argv[1]);
    if (!in) fail(std::string("cannot read ") + argv[1]);
    std::string name, line;
    if (!std::getline(in, name) || !std::getline(in, line)) fail("the input has no name and lengths");
    std::vector<uint32_t> seg_len, steps, prec;
    {
        std::istringstream ls(line);
        for (uint64_t x; ls >> x;) seg_len.push_back((uint32_t)x);
    }
    std::vector<uint64_t> pstart{0};
    std::vector<uint8_t> names;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ls(line);
        std::string pname;
        ls >> pname;
        prec.insert(prec.end(), {(uint32_t)steps.size(), (uint32_t)names.size(), (uint32_t)pname.size()});
        names.insert(names.end(), pname.begin(), pname.end());
        for (uint64_t h; ls >> h;) {
            if ((h >> 1) >= seg_len.size()) fail("a step names no segment");  // (the refusal is the library tests' business)
            steps.push_back((uint32_t)h);
        }
        pstart.push_back(steps.size());
    }
    const uint32_t S = (uint32_t)seg_len.size();
    hipStream_t st = nullptr;
    CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    uint32_t *d_len = to_device(seg_len);
    uint64_t *d_legend = nullptr;
    CK(hipMalloc((void **)&d_legend, (S + 1) * 8));
    if (flatten_legend(d_len, S, d_legend, st)) fail(last_error());
    std::vector<uint64_t> legend(S + 1);
    CK(hipMemcpy(legend.data(), d_legend, (S + 1) * 8, hipMemcpyDeviceToHost));

    FlatPaths g;
    g.legend = d_legend, g.n_segs = S;
    g.steps = to_device(steps), g.pstart = to_device(pstart), g.prec = to_device(prec), g.name_data = to_device(names);
    g.n_paths = (uint32_t)(pstart.size() - 1), g.n_lines = pstart.back();
    FlatJob *job = flatten_new(argc == 4 ? strtoull(argv[3], nullptr, 10) : kFlatChunkLines);
    uint64_t bytes = 0;
    std::string bed;
    if (flatten_bed_begin(job, g, (const uint8_t *)name.data(), name.size(), st, &bytes)) fail(last_error());
    if (flatten_bed_emit(job, take, &bed)) fail(last_error());
    if (bed.size() != bytes) fail("the table is not as long as it was counted");
    flatten_free(job);

    std::ofstream o(argv[2], std::ios::binary);
    o << "legend";
    for (uint64_t x : legend) o << ' ' << x;
    o << '\n' << bed;
    o.close();
    if (!o) fail(std::string("cannot write ") + argv[2]);
    for (const void *d : {(const void *)d_len, (const void *)d_legend, (const void *)g.steps, (const void *)g.pstart, (const void *)g.prec,
                          (const void *)g.name_data})
        CK(hipFree(const_cast<void *>(d)));
    CK(hipStreamDestroy(st));
    std::printf("flatten_check: %u segments, %llu lines, %llu bytes\n", S, (unsigned long long)g.n_lines, (unsigned long long)bytes);
    return 0;
}
