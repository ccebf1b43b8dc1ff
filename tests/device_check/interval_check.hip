// Runs the interval job of pollen_amd/csrc/interval_device.hip on its own, with the two parameters no public entry passes:
// the batch budget (how many step end positions the scratch holds at a time) and the lane / wave cut.
// `make -C pollen_amd/csrc interval_check` builds it for gfx950 from the job's source, the host plan (flatgfa_core.cpp) and the
// staged copies (host_copy.cpp); tests/test_gpu_interval_depth.py drives it.
//
//   interval_check MANIFEST    one case per line: INPUT OUTPUT.  Every case runs in this one process on one stream.  The program
//                              judges nothing: it writes what the job left and exits 0.  A HIP call that fails or an input that
//                              does not hold what its header says ends the program at once with a non-zero status.
//
//   INPUT   u64[6]: n_segs, n_steps, n_paths, n_intervals, budget, lane_cut; then u32 seg_len[n_segs], u32 depth[n_segs],
//           u32 steps[n_steps], u32 begin[n_paths], u32 end[n_paths], u32 path_id[n_intervals] (padded to 8 bytes),
//           u64 start[n_intervals], u64 end[n_intervals]
//   OUTPUT  i64 return code, u64 batches, f64[n_intervals + 64]: the results, then a guard of 0xA5 bytes
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "../../pollen_amd/csrc/device_common.hpp"
#include "../../pollen_amd/csrc/interval_device.hpp"
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
    std::fprintf(stderr, "interval_check: %s\n", what.c_str());
    std::exit(1);
}
#define CK(expr)                                                                      \
    do {                                                                              \
        hipError_t _e = (expr);                                                       \
        if (_e != hipSuccess) fail(std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

namespace {
constexpr uint64_t kGuard = 64;
constexpr uint64_t kMaxN = 1ull << 26;  // (no case comes near)

template <class T>
T *to_device(const uint8_t *src, uint64_t n) {
    T *d = nullptr;
    CK(hipMalloc((void **)&d, (n ? n : 1) * sizeof(T)));
    if (n) CK(hipMemcpy(d, src, n * sizeof(T), hipMemcpyHostToDevice));
    return d;
}

void run_case(const std::string &in_path, const std::string &out_path, hipStream_t st) {
    std::ifstream f(in_path, std::ios::binary);
    if (!f) fail("cannot read " + in_path);
    const std::string buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (buf.size() < 48) fail(in_path + ": no header");
    uint64_t h[6];
    memcpy(h, buf.data(), 48);
    const uint64_t S = h[0], N = h[1], P = h[2], n = h[3], budget = h[4], cut = h[5];
    if (S > kMaxN || N > kMaxN || P > kMaxN || n > kMaxN) fail(in_path + ": a count out of range");
    const uint64_t n_pad = (n + 1) & ~1ull;
    if (buf.size() != 48 + 4 * (2 * S + N + 2 * P + n_pad) + 16 * n) fail(in_path + ": the size is not what the header says");
    const uint8_t *p = (const uint8_t *)buf.data() + 48;
    const uint8_t *p_len = p, *p_depth = p_len + 4 * S, *p_steps = p_depth + 4 * S, *p_begin = p_steps + 4 * N, *p_end = p_begin + 4 * P,
                  *p_ids = p_end + 4 * P, *p_st = p_ids + 4 * n_pad, *p_en = p_st + 8 * n;
    std::vector<uint32_t> begin(P), end(P), ids(n);
    if (P) memcpy(begin.data(), p_begin, 4 * P), memcpy(end.data(), p_end, 4 * P);
    if (n) memcpy(ids.data(), p_ids, 4 * n);
    IntervalGraph g;
    g.steps = to_device<uint32_t>(p_steps, N), g.n_steps = N;
    g.begin = begin.data(), g.end = end.data(), g.n_paths = (uint32_t)P;
    g.seg_len = to_device<uint32_t>(p_len, S), g.depth = to_device<uint32_t>(p_depth, S), g.n_segs = (uint32_t)S;
    IntervalList iv;
    iv.path_id = to_device<uint32_t>(p_ids, n), iv.start = to_device<uint64_t>(p_st, n), iv.end = to_device<uint64_t>(p_en, n), iv.n = n;
    double *d_out = nullptr;
    CK(hipMalloc((void **)&d_out, (n + kGuard) * 8));
    CK(hipMemset(d_out, 0xA5, (n + kGuard) * 8));
    IntervalJob *job = interval_new(budget, (uint32_t)cut);
    const int64_t rc = interval_depth(job, g, iv, ids.data(), st, d_out);
    CK(hipStreamSynchronize(st));
    const uint64_t batches = interval_batches(job);
    interval_free(job);
    std::vector<double> out(n + kGuard);
    CK(hipMemcpy(out.data(), d_out, out.size() * 8, hipMemcpyDeviceToHost));
    std::ofstream o(out_path, std::ios::binary);
    o.write((const char *)&rc, 8);
    o.write((const char *)&batches, 8);
    o.write((const char *)out.data(), (std::streamsize)(out.size() * 8));
    if (!o) fail("cannot write " + out_path);
    for (const void *d : {(const void *)g.steps, (const void *)g.seg_len, (const void *)g.depth, (const void *)iv.path_id, (const void *)iv.start,
                          (const void *)iv.end, (const void *)d_out})
        CK(hipFree(const_cast<void *>(d)));
}
}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) fail("usage: interval_check MANIFEST");
    std::ifstream m(argv[1]);
    if (!m) fail(std::string("cannot read ") + argv[1]);
    hipStream_t st = nullptr;
    CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    std::string line;
    int cases = 0;
    while (std::getline(m, line)) {
        if (line.empty()) continue;
        std::istringstream ls(line);
        std::string in, out;
        if (!(ls >> in >> out)) fail("bad manifest line: " + line);
        run_case(in, out, st);
        ++cases;
    }
    CK(hipStreamDestroy(st));
    std::printf("interval_check: %d cases\n", cases);
    return 0;
}
