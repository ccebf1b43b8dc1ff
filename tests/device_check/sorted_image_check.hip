// Builds the sorted record image of pollen_amd/csrc/depth_sorted.hip on its own, from a hand-made FastPlan: the four arrays and
// five scalars the build reads and nothing else -- no graph, no depth buffers, no plan.  So the cases reach what no public entry
// point does with a few hundred records: n_cus of 1 (the grid stride of count and emit), more than 8192 windows (the count
// straight into memory), every refusal, and what the finaliser leaves in memory that no answer depends on.
// `make -C pollen_amd/csrc sorted_image_check` builds it for gfx950 from depth_sorted.hip, depth_sorted_sort.hip and the staged
// copies (host_copy.cpp), linked against nothing of the library; tests/test_gpu_sorted_image.py drives it over the cases of
// tests/sorted_image_cases.py.
//
//   sorted_image_check MANIFEST   one case per line: INPUT OUTPUT.  Every case runs in this one process on one stream.  The
//                                 program judges nothing: it writes what the build left and exits 0.  A HIP call of its own that
//                                 fails or an input that does not hold what its header says ends it at once with a non-zero status.
//
//   INPUT   u64[10]: wb, n_range, n_win, n_paths, n_cus, reserve, waived, n_items, n_ent, second; then u32 items[n_items][4]
//           (.x, .y the item's steps [b, e), .w its path id), u32 item_ent[n_items][2] (the entries the item reads),
//           u32 ent[n_ent + 1][2] (first id | downward << 31, step position; the last one closes the last run) and, where
//           `second` is 1, u32 ent2[n_ent + 1][2]: copied over the entries between sorted_image_start (and a stream synchronise
//           behind it) and the first sorted_image_poll -- the steps changed while the image was made.
//   OUTPUT  i64[8]: polls made, the last poll's return, sorted_image_phase, sorted_image_bytes, sorted_image_transient,
//           n_chunks (0 unless built), n_win, 0; char why[16]; i64 returns[polls]; and where the last return is 1:
//           u32 win_chunk[n_win + 1], u32 rec[n_chunks * 64], u32 carry[n_chunks] as sorted_image_install left them in the plan.
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

#include "../../pollen_amd/csrc/depth_fast.hpp"
#include "../../pollen_amd/csrc/depth_sorted_host.hpp"
#include "../../pollen_amd/csrc/device_common.hpp"
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
    std::fprintf(stderr, "sorted_image_check: %s\n", what.c_str());
    std::exit(1);
}
#define CK(expr)                                                                      \
    do {                                                                              \
        hipError_t _e = (expr);                                                       \
        if (_e != hipSuccess) fail(std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

namespace {
constexpr uint64_t kMaxN = 1ull << 24;  // (no case comes near)
constexpr int kMaxPolls = 8;            // (a waiting poll settles the build in one)

uint32_t *to_device(const uint8_t *src, uint64_t n_words) {
    uint32_t *d = nullptr;
    CK(hipMalloc((void **)&d, (n_words ? n_words : 4) * 4));
    if (n_words) CK(hipMemcpy(d, src, n_words * 4, hipMemcpyHostToDevice));
    return d;
}

void run_case(const std::string &in_path, const std::string &out_path, hipStream_t st) {
    std::ifstream f(in_path, std::ios::binary);
    if (!f) fail("cannot read " + in_path);
    const std::string buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (buf.size() < 80) fail(in_path + ": no header");
    uint64_t h[10];
    memcpy(h, buf.data(), 80);
    const uint64_t wb = h[0], n_range = h[1], n_win = h[2], n_paths = h[3], n_cus = h[4], reserve = h[5], waived = h[6], n_items = h[7], n_ent = h[8], second = h[9];
    if (wb > 16 || n_range >> 32 || n_win > kMaxN || n_paths >> 32 || !n_cus || n_cus > 1024 || waived > 1 || n_items > kMaxN || n_ent > kMaxN || second > 1)
        fail(in_path + ": a header field out of range");
    const uint64_t ent_words = 2 * (n_ent + 1);
    if (buf.size() != 80 + 4 * (4 * n_items + 2 * n_items + ent_words * (1 + second))) fail(in_path + ": the size is not what the header says");
    const uint8_t *p_items = (const uint8_t *)buf.data() + 80, *p_item_ent = p_items + 16 * n_items, *p_ent = p_item_ent + 8 * n_items, *p_ent2 = p_ent + 4 * ent_words;
    uint32_t *d_items = to_device(p_items, 4 * n_items), *d_item_ent = to_device(p_item_ent, 2 * n_items), *d_ent = to_device(p_ent, ent_words);

    FastPlan fp;
    fp.wb = (uint32_t)wb, fp.n_range = (uint32_t)n_range, fp.n_win = (uint32_t)n_win, fp.n_cus = (uint32_t)n_cus;
    fp.items = d_items, fp.n_items = (uint32_t)n_items;
    fp.run_item_ent = d_item_ent, fp.run_ent = d_ent, fp.run_n_ent = (uint32_t)n_ent;

    SortedImage *si = sorted_image_start(fp, (uint32_t)n_paths, st);
    if (second) {
        CK(hipStreamSynchronize(st));
        CK(hipMemcpy(d_ent, p_ent2, ent_words * 4, hipMemcpyHostToDevice));
    }
    std::vector<int64_t> polls;
    int rc = 0;
    while (rc == 0 && (int)polls.size() < kMaxPolls) {
        rc = sorted_image_poll(si, fp, st, true, reserve, waived != 0);
        polls.push_back(rc);
    }
    CK(hipStreamSynchronize(st));
    std::vector<uint32_t> win_chunk, rec, carry;
    if (rc == 1) {
        sorted_image_install(&fp, si, false);
        win_chunk.resize(n_win + 1);
        CK(hipMemcpy(win_chunk.data(), fp.sorted_win_chunk, win_chunk.size() * 4, hipMemcpyDeviceToHost));
        const uint64_t n_chunks = win_chunk[n_win];
        if (n_chunks > kMaxN) fail(in_path + ": win_chunk's last entry is out of range");
        rec.resize(n_chunks * kSortedChunk), carry.resize(n_chunks);
        if (n_chunks) {
            CK(hipMemcpy(rec.data(), fp.sorted_rec, rec.size() * 4, hipMemcpyDeviceToHost));
            CK(hipMemcpy(carry.data(), fp.sorted_carry, carry.size() * 4, hipMemcpyDeviceToHost));
        }
    }
    const int64_t head[8] = {(int64_t)polls.size(), rc, sorted_image_phase(si), (int64_t)sorted_image_bytes(si), (int64_t)sorted_image_transient(si),
                             (int64_t)carry.size(), (int64_t)n_win, 0};
    char why[16] = {0};
    std::strncpy(why, sorted_image_why(si), sizeof why - 1);
    sorted_image_free(si, st);
    (void)hipGetLastError();  // (a refusal may leave a status behind that is not this program's)

    std::ofstream o(out_path, std::ios::binary);
    o.write((const char *)head, sizeof head);
    o.write(why, sizeof why);
    o.write((const char *)polls.data(), (std::streamsize)(polls.size() * 8));
    o.write((const char *)win_chunk.data(), (std::streamsize)(win_chunk.size() * 4));
    o.write((const char *)rec.data(), (std::streamsize)(rec.size() * 4));
    o.write((const char *)carry.data(), (std::streamsize)(carry.size() * 4));
    if (!o) fail("cannot write " + out_path);
    for (void *d : {(void *)d_items, (void *)d_item_ent, (void *)d_ent}) CK(hipFree(d));
}
}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) fail("usage: sorted_image_check MANIFEST");
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
    std::printf("sorted_image_check: %d cases\n", cases);
    return 0;
}
