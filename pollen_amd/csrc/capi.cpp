// extern "C" surface of libflatgfa.so: the flatgfa-c drop-in (Part 1 of include/flatgfa.h)
// plus the additive loaders, the depth queries and the host routes of the other features (Part 2).  The kernels live in the
// .hip files -- depth_device.hip and its kin for depth, gaf_device.hip, gaf_lookup_device.hip, chop_device.hip,
// extract_device.hip, topology_device.hip, flatten_device.hip, crush_device.hip, flip_device.hip, seq_device.hip, print_device.hip for the rest -- and are reached through their headers; this file uses the HIP runtime
// API only.  Every host route that is not a depth query holds what it has on the device in one DevScope (below).
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <sys/mman.h>
#include <fcntl.h>
#include <unistd.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <string_view>
#include <unordered_set>
#include <vector>

#include <malloc.h>

#include <climits>
#include <cstring>

#include "../../include/flatgfa.h"
#include "device_common.hpp"
#include "temp_arena.hpp"
#include "host_copy.hpp"
#include "flatgfa_core.hpp"
#include "gaf_device.hpp"
#include "chop_device.hpp"
#include "inject_device.hpp"
#include "gaf_lookup_device.hpp"
#include "extract_device.hpp"
#include "topology_device.hpp"
#include "interval_device.hpp"
#include "flatten_device.hpp"
#include "crush_device.hpp"
#include "flip_device.hpp"
#include "flip_host.hpp"
#include "seq_device.hpp"
#include "print_device.hpp"
#include "parse_device.hpp"
#include "bed_device.hpp"

using fgfa_dev::set_error;

// A handle's stream comes from a per-device pool of the process and goes back to it idle when the handle is freed: creating a stream
// costs half a millisecond on this runtime, which is a third of what a resident graph's first answer costs.
namespace {
std::mutex g_stream_pool_mu;
std::vector<hipStream_t> g_stream_pool[64];
hipError_t stream_acquire(int device, hipStream_t *out) {
    {
        std::lock_guard<std::mutex> lk(g_stream_pool_mu);
        if (device >= 0 && device < 64 && !g_stream_pool[device].empty()) {
            *out = g_stream_pool[device].back();
            g_stream_pool[device].pop_back();
            return hipSuccess;
        }
    }
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}
void stream_release(int device, hipStream_t st) {
    if (!st) return;
    if (hipStreamSynchronize(st) != hipSuccess || device < 0 || device >= 64) {
        (void)hipGetLastError();
        (void)hipStreamDestroy(st);
        return;
    }
    std::lock_guard<std::mutex> lk(g_stream_pool_mu);
    if (g_stream_pool[device].size() < 8) g_stream_pool[device].push_back(st);
    else (void)hipStreamDestroy(st);
}
}  // namespace

// The opaque store (flatgfa-c/src/lib.rs:16-28): either a heap store built by the parser /
// generator, or a borrowed view of a memory-mapped .flatgfa file.
struct CStore {
    fgfa::Store heap;
    std::unique_ptr<fgfa::MappedFile> file;
    fgfa::View view;

    // Resident device image (structure of arrays), created on first use.
    std::mutex op_mu;   // one depth query at a time per handle
    std::mutex dev_mu;
    bool on_device = false;
    int device = 0;
    uint32_t *d_steps = nullptr;
    uint32_t *d_small = nullptr;  // one allocation behind the five arrays below
    uint32_t *d_path_begin = nullptr, *d_path_end = nullptr, *d_seg_len = nullptr;
    uint32_t *d_depth = nullptr, *d_uniq = nullptr;
    uint64_t *d_sums = nullptr;  // [2 * paths] scratch of flatgfa_path_depth (inside d_small)
    double h2d_ms = 0, plan_ms = 0;  // what becoming resident took: the copies, and the plan's creation (flatgfa_residency_ms)
    // The plan's creation is the first query (flatgfa_dev_plan_create_first): d_depth / d_uniq hold seg_depth_with_uniq of the
    // graph until another query overwrites them, and the first node-depth call of the handle takes them as they are.
    bool first_answer = false;
    int first_rc = 0;
    std::vector<uint32_t> h_path_begin, h_path_end;
    std::vector<uint32_t> h_soa;  // the host image of the small arrays (spans, segment lengths) that was uploaded: kept, not unmapped behind the upload
    flatgfa_dev_plan_t *plan = nullptr;
    hipStream_t stream = nullptr;
    // the prepared query of the last flatgfa_seg_depth_subset call, reused while the subset is the same
    std::vector<uint32_t> sub_ids;
    flatgfa_dev_plan_t *sub_plan = nullptr;
    uint32_t *d_sub_spans = nullptr;  // the subset's begin[] then end[]
    std::atomic<int> steps_ok{-1};  // -1 = not checked yet: do all step handles name a segment? (host-side walks index by them)
    // pangenotype: the graph's NameMap on one device (made on first use; it needs the segments only, never the steps), and
    // the scratch of flatgfa_dev_pangenotype_row with the event after its last use
    int gaf_device = -1;
    uint64_t *d_gaf_names = nullptr;  // the `others` names, sorted, then their ids
    fgfa_dev::GafNameTable gaf_names;
    int gaf_scratch_device = -1;
    uint64_t *d_gaf_scratch = nullptr;
    size_t gaf_scratch_words = 0;
    hipEvent_t gaf_ev = nullptr;
    // GAF lookup: the sequence pool on one device (made on first use: Segment.seq.start and Segment::len() per segment,
    // then seq_data), freed with the handle as the name table is
    int gaf_seq_device = -1;
    uint32_t *d_gaf_seg_seq = nullptr;
    uint8_t *d_gaf_seq_data = nullptr;
    // validate, degree: the link index on one device (made on the first validate or degree call, never for a graph that is not asked)
    int topo_device = -1;
    fgfa_dev::TopoIndex topo;
    // flatten: the legend on one device (made on the first flatten call), and the bases it adds up to
    int flat_device = -1;
    uint64_t *d_flat_legend = nullptr;
    uint64_t flat_total = 0;

    ~CStore() {
        if (plan) flatgfa_dev_plan_destroy(plan);
        if (sub_plan) flatgfa_dev_plan_destroy(sub_plan);
        if (d_sub_spans) (void)hipFree(d_sub_spans);
        for (uint32_t *p : {d_steps, d_small})
            if (p) (void)hipFree(p);
        if (gaf_ev) (void)hipEventSynchronize(gaf_ev);
        for (uint64_t *p : {d_gaf_names, d_gaf_scratch})
            if (p) (void)hipFree(p);
        if (gaf_ev) (void)hipEventDestroy(gaf_ev);
        if (d_gaf_seg_seq) (void)hipFree(d_gaf_seg_seq);
        fgfa_dev::topo_index_free(&topo);
        if (d_flat_legend) (void)hipFree(d_flat_legend);
        stream_release(device, stream);
    }
};

// Host code that follows step handles into the segment pool (path lengths, the GFA printer, the
// interval walk) asks this first; the kernels check the ids themselves.
static bool steps_name_segments(CStore *cs) {
    if (cs->steps_ok < 0) cs->steps_ok = fgfa::validate_step_ids(cs->view) ? 1 : 0;
    if (!cs->steps_ok) set_error("a step refers to a segment id that is out of range");
    return cs->steps_ok == 1;
}

// (sharded.hip reads the pools of a handle)
const fgfa::View &flatgfa_capi_view(flatgfa_t gfa) { return gfa->view; }

#define CAPI_HIP(expr) FGFA_HIP("", expr)

namespace {
// How many HIP devices there are; none is the error of every entry that needs one, which names itself in `who` ("chop has",
// "the depth queries have").
int count_devices(const std::string &who, int *ndev) {
    *ndev = 0;
    if (hipGetDeviceCount(ndev) != hipSuccess || *ndev <= 0) {
        set_error("no HIP device is visible; " + who + " no CPU fallback");
        return FLATGFA_ERR_NO_DEVICE;
    }
    return FLATGFA_OK;
}

// What one host call of a route -- pangenotype, GAF lookup, chop, extract, position, validate, degree, flatten, crush, flip, seq-export, seq-import, the GFA printer, bed -- holds on the device,
// given back on every way out: the work stream is waited for, then the job, the events and the memory go, then the streams
// return to the pool.  A thread that still copies on one of the streams is joined first: its joiner is declared after the scope.
struct DevScope {
    int device = 0;
    bool resident = false;         // the graph has an image on `device`, which the call may read in place
    hipStream_t stream = nullptr;  // the work stream: the first one taken
    std::vector<hipStream_t> streams;
    std::vector<hipEvent_t> events;
    std::vector<void *> mem;
    void *job = nullptr;  // the feature's job object (no route has two) and how it is freed
    void (*job_free)(void *) = nullptr;
    DevScope() = default;
    DevScope(const DevScope &) = delete;
    DevScope &operator=(const DevScope &) = delete;
    ~DevScope() {
        if (stream) (void)hipStreamSynchronize(stream);
        if (job) job_free(job);
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        for (void *p : mem) (void)hipFree(p);
        for (hipStream_t s : streams) stream_release(device, s);
    }
    hipError_t take_stream(hipStream_t *out) {
        *out = nullptr;
        const hipError_t e = stream_acquire(device, out);
        if (e == hipSuccess) streams.push_back(*out);
        return e;
    }
    hipError_t make_event(hipEvent_t *out) {
        *out = nullptr;
        const hipError_t e = hipEventCreateWithFlags(out, hipEventDisableTiming);
        if (e == hipSuccess) events.push_back(*out);
        return e;
    }
    template <class J, void (*Free)(J *)>
    J *hold(J *j) {
        job = j;
        job_free = [](void *p) { Free(static_cast<J *>(p)); };
        return j;
    }
    template <class T>
    hipError_t alloc(T **p, size_t count) {  // (at least one element)
        *p = nullptr;
        const hipError_t e = hipMalloc((void **)p, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) mem.push_back(*p);
        return e;
    }
    // a device copy of host memory
    template <class T>
    hipError_t upload(T **p, const void *src, size_t count) {
        hipError_t e = alloc(p, count);
        if (e == hipSuccess && count) e = fgfa_dev::staged_copy(*p, src, count * sizeof(T), hipMemcpyHostToDevice, stream);
        return e;
    }
    // one allocation given back early (NULL: nothing)
    hipError_t release(void *p) {
        if (!p) return hipSuccess;
        mem.erase(std::remove(mem.begin(), mem.end(), p), mem.end());
        return hipFree(p);
    }
};

// The device a call on `gfa` runs on (the one it is resident on, else 0), made current, with the work stream.  A route that
// reads no graph (the packed-sequence codec) passes null: device 0, nothing resident.
int open_scope(CStore *gfa, DevScope *sc, const char *what) {
    if (gfa) {
        std::lock_guard<std::mutex> lk(gfa->dev_mu);
        if (gfa->on_device) sc->device = gfa->device, sc->resident = true;  // (beside the graph; it is not made resident)
    }
    int ndev = 0;
    if (int rc = count_devices(std::string(what) + " has", &ndev)) return rc;
    CAPI_HIP(hipSetDevice(sc->device));
    CAPI_HIP(sc->take_stream(&sc->stream));
    return FLATGFA_OK;
}

struct Joiner {
    std::thread &t;
    ~Joiner() { if (t.joinable()) t.join(); }
};

// The size GAF text is cut to for the device (fgfa::cut_lines): 64 MiB, or what the tests ask for.
size_t gaf_chunk_bytes() {
    if (const char *h = test_hook("FLATGFA_GAF_CHUNK_BYTES")) return std::max<size_t>(1, strtoull(h, nullptr, 10));
    return (size_t)64 << 20;
}
}  // namespace

extern "C" {

const char *flatgfa_last_error(void) { return fgfa_dev::last_error(); }

// ------------------------------------------------------------- Part 1 ---

static flatgfa_t parse_common(const uint8_t *data, size_t len, bool stream_mode) {
    auto cs = std::make_unique<CStore>();
    std::string err;
    if (!fgfa::parse_gfa(data ? data : (const uint8_t *)"", len, &cs->heap, &err, stream_mode)) {
        set_error(err);
        return nullptr;
    }
    cs->view = cs->heap.view();
    return cs.release();
}

flatgfa_t flatgfa_parse_bytes(const uint8_t *data, size_t len) { return parse_common(data, len, false); }
flatgfa_t flatgfa_parse_stream_bytes(const uint8_t *data, size_t len) { return parse_common(data, len, true); }

flatgfa_t flatgfa_parse(const char *filename) {
    if (!filename) { set_error("flatgfa_parse: NULL filename"); return nullptr; }
    fgfa::MappedFile f;
    std::string err;
    if (!f.open(filename, &err)) { set_error(err); return nullptr; }
    return flatgfa_parse_bytes(f.data, f.size);
}

// ---- GFA text parsed on the device ----

extern "C++" {
namespace {
struct ParseRecord {
    bool any = false;
    uint64_t info[4] = {0, 0, 0, 0};
    double ms[4] = {0, 0, 0, 0};
};
thread_local ParseRecord t_parse_record;

// What no pool may pass on the device route: 2^32 - 1 items, or what the tests ask for.
uint64_t parse_device_limit() {
    if (const char *h = test_hook("FLATGFA_PARSE_DEVICE_LIMIT")) return strtoull(h, nullptr, 10);
    return 0xFFFFFFFFull;
}

flatgfa_t parse_device_common(const uint8_t *data, size_t len, bool stream_mode) {
    auto cs = std::make_unique<CStore>();
    fgfa_dev::ParseInfo info;
    {
        DevScope sc;
        if (open_scope(nullptr, &sc, "the device GFA parser")) return nullptr;
        if (fgfa_dev::parse_device(data ? data : (const uint8_t *)"", len, stream_mode, parse_device_limit(), sc.stream, &cs->heap, &info))
            return nullptr;
    }
    ParseRecord &r = t_parse_record;
    r.any = true;
    r.info[0] = (uint64_t)info.device_route;
    r.info[1] = (uint64_t)info.reason;
    r.info[2] = info.tile_bytes;
    r.info[3] = info.tiles;
    r.ms[0] = info.upload_ms, r.ms[1] = info.kernel_ms, r.ms[2] = info.step_ms, r.ms[3] = info.download_ms;
    if (!info.device_route) {  // not the plain grammar: the host parser's handle, or its error, on the same bytes
        r.ms[0] = r.ms[1] = r.ms[2] = r.ms[3] = 0;
        return parse_common(data, len, stream_mode);
    }
    cs->view = cs->heap.view();
    return cs.release();
}
}  // namespace
}  // extern "C++"

flatgfa_t flatgfa_parse_bytes_device(const uint8_t *data, size_t len, int from_stream) {
    if (!data && len) { set_error("flatgfa_parse_bytes_device: NULL data with a length"); return nullptr; }
    return parse_device_common(data, len, from_stream != 0);
}

flatgfa_t flatgfa_parse_device(const char *filename) {
    if (!filename) { set_error("flatgfa_parse_device: NULL filename"); return nullptr; }
    fgfa::MappedFile f;
    std::string err;
    if (!f.open(filename, &err)) { set_error(err); return nullptr; }
    return parse_device_common(f.data, f.size, false);
}

int flatgfa_parse_device_info(uint64_t out[4]) {
    if (!out || !t_parse_record.any) { set_error("flatgfa_parse_device_info: NULL argument, or no device parse on this thread yet"); return FLATGFA_ERR_ARG; }
    for (int i = 0; i < 4; ++i) out[i] = t_parse_record.info[i];
    return FLATGFA_OK;
}

int flatgfa_parse_device_times(double out[4]) {
    if (!out || !t_parse_record.any) { set_error("flatgfa_parse_device_times: NULL argument, or no device parse on this thread yet"); return FLATGFA_ERR_ARG; }
    for (int i = 0; i < 4; ++i) out[i] = t_parse_record.ms[i];
    return FLATGFA_OK;
}

flatgfa_t flatgfa_load(const char *filename) {
    if (!filename) { set_error("flatgfa_load: NULL filename"); return nullptr; }
    auto cs = std::make_unique<CStore>();
    cs->file = std::make_unique<fgfa::MappedFile>();
    std::string err;
    if (!cs->file->open(filename, &err) || !fgfa::view_flatgfa(cs->file->data, cs->file->size, &cs->view, &err)) {
        set_error(err);
        return nullptr;
    }
    return cs.release();
}

flatgfa_t flatgfa_synth(uint64_t seed, uint32_t n_segs, uint32_t n_paths, uint32_t steps_per_path, int model,
                        bool with_seq) {
    if (n_segs == 0 || (model < 0 || model > 4) || (uint64_t)n_paths * steps_per_path > 0xFFFFFFFFull ||
        n_segs > 0x7FFFFFFFu) {
        set_error("flatgfa_synth: bad shape");
        return nullptr;
    }
    auto cs = std::make_unique<CStore>();
    fgfa::synth_store(seed, n_segs, n_paths, steps_per_path, model, with_seq, &cs->heap);
    cs->view = cs->heap.view();
    return cs.release();
}

void flatgfa_free(flatgfa_t gfa) { delete gfa; }

uint32_t flatgfa_get_segment_count(flatgfa_t gfa) { return (uint32_t)gfa->view.segs.len; }

flatgfa_string_t flatgfa_get_seq(flatgfa_t gfa, uint32_t segment_id) {
    flatgfa_string_t s{nullptr, 0};
    const fgfa::View &v = gfa->view;
    if (segment_id >= v.segs.len) return s;
    fgfa::Span sp = v.segs[segment_id].seq;
    s.data = v.seq_data.data + sp.start;
    s.len = (int)sp.len();
    return s;
}

uint32_t flatgfa_path_count(flatgfa_t gfa) { return (uint32_t)gfa->view.paths.len; }

flatgfa_string_t flatgfa_get_path_name(flatgfa_t gfa, uint32_t path_index) {
    flatgfa_string_t s{nullptr, 0};
    const fgfa::View &v = gfa->view;
    if (path_index >= v.paths.len) return s;
    fgfa::Span sp = v.paths[path_index].name;
    s.data = v.name_data.data + sp.start;
    s.len = (int)sp.len();
    return s;
}

uint32_t flatgfa_get_path_step_count(flatgfa_t gfa, uint32_t path_index) {
    const fgfa::View &v = gfa->view;
    if (path_index >= v.paths.len) return UINT32_MAX;
    return v.paths[path_index].steps.len();
}

bool flatgfa_get_step(flatgfa_t gfa, uintptr_t path_index, uintptr_t step_index, flatgfa_handle_t *out) {
    const fgfa::View &v = gfa->view;
    if (path_index >= v.paths.len) return false;
    fgfa::Span sp = v.paths[path_index].steps;
    if (step_index >= sp.len()) return false;
    fgfa::Handle h = v.steps[sp.start + step_index];
    out->segment_id = h.segment();
    out->is_forward = h.is_forward();
    return true;
}

// ------------------------------------------------------------- Part 2 ---

int flatgfa_pool(flatgfa_t gfa, int ix, const void **data, uint64_t *len, uint64_t *elem_size) {
    if (!gfa || ix < 0 || ix > 10) { set_error("flatgfa_pool: bad argument"); return FLATGFA_ERR_ARG; }
    if (data) *data = gfa->view.pool_data(ix);
    if (len) *len = gfa->view.pool_len(ix);
    if (elem_size) *elem_size = fgfa::kPoolElemSize[ix];
    return FLATGFA_OK;
}

int64_t flatgfa_find_path(flatgfa_t gfa, const uint8_t *name, size_t len) {
    if (!gfa) return -1;
    return gfa->view.find_path(name, len);
}

int flatgfa_write_flatgfa(flatgfa_t gfa, const char *filename) {
    if (!gfa || !filename) { set_error("flatgfa_write_flatgfa: NULL argument"); return FLATGFA_ERR_ARG; }
    size_t n = fgfa::flatgfa_file_size(gfa->view);
    std::vector<uint8_t> buf(n);
    fgfa::dump_flatgfa(gfa->view, buf.data());
    FILE *f = fopen(filename, "wb");
    if (!f) { set_error(std::string("cannot create ") + filename); return FLATGFA_ERR_IO; }
    size_t w = fwrite(buf.data(), 1, n, f);
    if (fclose(f) != 0 || w != n) { set_error(std::string("short write to ") + filename); return FLATGFA_ERR_IO; }
    return FLATGFA_OK;
}

int flatgfa_write_flatgfa_prealloc(flatgfa_t gfa, const char *filename, const uint8_t *gfa_text, size_t text_len, uint32_t factor) {
    if (!gfa || !filename || (text_len && !gfa_text)) { set_error("flatgfa_write_flatgfa_prealloc: NULL argument"); return FLATGFA_ERR_ARG; }
    uint64_t cap[11];
    std::string err;
    if (gfa_text) {
        if (!fgfa::estimate_toc(gfa_text, text_len, cap, &err)) { set_error(err); return FLATGFA_ERR_BOUNDS; }
    } else {
        fgfa::guess_toc(factor, cap);
    }
    size_t n = 0;
    if (!fgfa::prealloc_file_size(gfa->view, cap, &n, &err)) { set_error(err); return FLATGFA_ERR_BOUNDS; }
    // The file is the sum of the CAPACITIES (up to 2^46 bytes; `-p 1000` is already gigabytes), most of it
    // never written: made sparse with ftruncate, then the table of contents and each pool's `len`
    // entries written at their offsets -- what the reference's map_new_file + file::init amount to
    // (memfile.rs:12-33, file.rs:255-272).  A fresh file reads as zeros behind what is written.
    const int fd = open(filename, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) { set_error(std::string("cannot create ") + filename); return FLATGFA_ERR_IO; }
    bool ok = ftruncate(fd, (off_t)n) == 0;
    const auto put = [&](const void *p, size_t bytes, uint64_t at) {
        const char *c = (const char *)p;
        while (ok && bytes) {
            const ssize_t w = pwrite(fd, c, bytes, (off_t)at);
            if (w <= 0) { ok = false; break; }
            c += w;
            at += (uint64_t)w;
            bytes -= (size_t)w;
        }
    };
    fgfa::Toc toc;
    toc.magic = fgfa::kMagic;
    for (int i = 0; i < 11; ++i) toc.pool[i] = fgfa::TocSize{gfa->view.pool_len(i), cap[i]};
    put(&toc, sizeof toc, 0);
    uint64_t off = sizeof toc;
    for (int i = 0; i < 11; ++i) {
        put(gfa->view.pool_data(i), gfa->view.pool_len(i) * fgfa::kPoolElemSize[i], off);
        off += cap[i] * fgfa::kPoolElemSize[i];
    }
    if (close(fd) != 0 || !ok) { set_error(std::string("short write to ") + filename); return FLATGFA_ERR_IO; }
    return FLATGFA_OK;
}

static int give_text(const std::string &s, char **text, size_t *len) {
    char *p = (char *)malloc(s.size() + 1);
    if (!p) { set_error("out of memory"); return FLATGFA_ERR_IO; }
    memcpy(p, s.data(), s.size());
    p[s.size()] = 0;
    *text = p;
    if (len) *len = s.size();
    return FLATGFA_OK;
}

int flatgfa_translate_prealloc(const uint8_t *gfa_text, size_t text_len, int from_stream, const char *filename, uint32_t factor) {
    if (!filename || (text_len && !gfa_text)) { set_error("flatgfa_translate_prealloc: NULL argument"); return FLATGFA_ERR_ARG; }
    const uint8_t *text = gfa_text ? gfa_text : (const uint8_t *)"";
    uint64_t cap[11];
    std::string err;
    if (from_stream) {
        fgfa::guess_toc(factor, cap);
    } else if (!fgfa::estimate_toc(text, text_len, cap, &err)) {
        set_error(err);
        return FLATGFA_ERR_BOUNDS;
    }
    size_t n = 0;
    if (!fgfa::toc_file_size(cap, &n, &err)) { set_error(err); return FLATGFA_ERR_BOUNDS; }
    // memfile::map_new_file (memfile.rs:24-33): created, sized (sparse: it reads as zeros), mapped shared
    const int fd = open(filename, O_RDWR | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) { set_error(std::string("cannot create ") + filename); return FLATGFA_ERR_IO; }
    if (ftruncate(fd, (off_t)n) != 0) {
        close(fd);
        set_error(std::string("cannot size ") + filename);
        return FLATGFA_ERR_IO;
    }
    void *m = mmap(nullptr, n, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (m == MAP_FAILED) { set_error(std::string("cannot map ") + filename); return FLATGFA_ERR_IO; }
    const bool ok = fgfa::parse_gfa_prealloc(text, text_len, from_stream != 0, cap, (uint8_t *)m, &err);
    const bool flushed = msync(m, n, MS_SYNC) == 0;  // (mmap.flush())
    munmap(m, n);
    if (!ok) {
        set_error(err);
        return err.rfind("preallocated flatgfa:", 0) == 0 ? FLATGFA_ERR_BOUNDS : FLATGFA_ERR_PARSE;
    }
    if (!flushed) { set_error(std::string("cannot flush ") + filename); return FLATGFA_ERR_IO; }
    return FLATGFA_OK;
}

int flatgfa_print_gfa(flatgfa_t gfa, char **text, size_t *len) {
    if (!gfa || !text) { set_error("flatgfa_print_gfa: NULL argument"); return FLATGFA_ERR_ARG; }
    if (!steps_name_segments(gfa)) return FLATGFA_ERR_BOUNDS;
    std::string out, err;
    if (!fgfa::print_gfa(gfa->view, &out, &err)) { set_error(err); return FLATGFA_ERR_BOUNDS; }
    return give_text(out, text, len);
}

void flatgfa_free_text(char *text) { free(text); }

int flatgfa_format_float(double x, int digits, char *out, int cap) {
    std::string s = fgfa::format_float(x, digits);
    int n = (int)std::min<size_t>(s.size(), cap > 0 ? (size_t)cap : 0);
    memcpy(out, s.data(), (size_t)n);
    return n;
}

// ---- device residency ----

int flatgfa_keep_host_memory(int on) {
#ifdef __GLIBC__
    // (never map: large blocks come from the heap and go back to its free lists; never trim: the heap's top stays)
    (void)mallopt(M_MMAP_MAX, on ? 0 : 65536);
    (void)mallopt(M_TRIM_THRESHOLD, on ? INT_MAX : 128 * 1024);
#else
    (void)on;
#endif
    return FLATGFA_OK;
}

int flatgfa_warm_device(int device) {
    int ndev = 0;
    if (int rc = count_devices("the depth queries have", &ndev)) return rc;
    if (device < 0 || device >= ndev) { set_error("device index out of range"); return FLATGFA_ERR_ARG; }
    CAPI_HIP(hipSetDevice(device));
    CAPI_HIP(fgfa_dev::warm_staging(device));  // (the staging buffers and this device's events, kept by the process)
    {   // the process's first asynchronous copy and first launch (queues, the library's code object)
        char *pinned = nullptr;
        const auto lk = fgfa_dev::borrow_staging(&pinned);
        uint32_t *d = nullptr;
        hipStream_t s = nullptr;
        CAPI_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        hipError_t e = hipMalloc(&d, 4096);
        if (e == hipSuccess) e = hipMemcpyAsync(d, pinned, 4096, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) {
            fgfa_dev::warm_launch(s);  // (loads the library's code object)
            e = hipStreamSynchronize(s);
        }
        if (d) (void)hipFree(d);
        (void)hipStreamDestroy(s);
        CAPI_HIP(e);
    }
    return FLATGFA_OK;
}

static int ensure_device(CStore *cs, int device) {
    std::lock_guard<std::mutex> lk(cs->dev_mu);
    if (cs->on_device) {
        if (device >= 0 && device != cs->device) { set_error("graph is already resident on another device"); return FLATGFA_ERR_ARG; }
        CAPI_HIP(hipSetDevice(cs->device));
        return FLATGFA_OK;
    }
    if (device < 0) device = 0;
    int ndev = 0;
    if (int rc = count_devices("the depth queries have", &ndev)) return rc;
    if (device >= ndev) { set_error("device index out of range"); return FLATGFA_ERR_ARG; }
    const fgfa::View &v = cs->view;
    if (v.steps.len > 0xFFFFFFFFull || v.segs.len > 0x80000000ull || v.paths.len > 0xFFFFFFFFull) {
        set_error("graph too large for 32-bit ids");
        return FLATGFA_ERR_TOO_LARGE;
    }
    const bool timing = getenv("FLATGFA_TIMING") != nullptr;  // diagnostic: where making a graph resident spends its time
    const auto t_enter = std::chrono::steady_clock::now();
    auto tick = [t = t_enter, timing](const char *what) mutable {
        if (!timing) return;
        const auto n = std::chrono::steady_clock::now();
        fprintf(stderr, "to_device: %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count());
        t = n;
    };
    // reversed or overlong step spans: where the reference would panic on the slice index (pool.rs:341-347)
    const size_t N = v.steps.len, P = v.paths.len, S = v.segs.len;
    for (size_t i = 0; i < P; ++i) {
        const fgfa::Span sp = v.paths[i].steps;
        if (sp.start > sp.end || (size_t)sp.end > N) {
            set_error("path " + std::to_string(i) + " has a step span outside the steps pool");
            return FLATGFA_ERR_BOUNDS;
        }
    }
    CAPI_HIP(hipSetDevice(device));
    // Everything is built into locals and handed to the handle only when all of it exists: a
    // failure half way (out of memory, say) leaves the handle as it was, and releases the rest.
    struct Image {
        int device = 0;
        hipStream_t stream = nullptr;
        uint32_t *steps = nullptr, *small = nullptr;
        uint32_t *pb = nullptr, *pe = nullptr, *seg_len = nullptr, *depth = nullptr, *uniq = nullptr, *sums = nullptr;  // inside `small`
        flatgfa_dev_plan_t *plan = nullptr;
        bool keep = false;
        ~Image() {
            if (keep) return;
            if (plan) flatgfa_dev_plan_destroy(plan);
            for (uint32_t *p : {steps, small})
                if (p) (void)hipFree(p);
            stream_release(device, stream);
        }
    } im;
    im.device = device;
    CAPI_HIP(stream_acquire(device, &im.stream));
    tick("device + stream");
    // AoS (packed, align-1) -> SoA.  Byte copies only: the file regions may be unaligned.  The
    // small arrays -- path spans, segment lengths, the two result vectors -- share one device
    // allocation and one copy: a hipMalloc costs about a millisecond whatever its size.
    const size_t Pa = (P + 63) & ~(size_t)63, Sa = (S + 63) & ~(size_t)63;  // 256-byte aligned sub-arrays
    std::vector<uint32_t> host(2 * Pa + Sa);
    uint32_t *h_pb = host.data(), *h_pe = host.data() + Pa, *h_len = host.data() + 2 * Pa;
    // (on a thread of its own, beside the upload of the steps: a million segments' lengths out of a freshly mapped file are a
    // millisecond of page faults that the link need not wait for)
    std::thread soa([&] {
        for (size_t i = 0; i < P; ++i) {
            h_pb[i] = v.paths[i].steps.start;
            h_pe[i] = v.paths[i].steps.end;
        }
        for (size_t i = 0; i < S; ++i) h_len[i] = v.segs[i].seq.len();
    });
    struct Joiner {
        std::thread &t;
        ~Joiner() { if (t.joinable()) t.join(); }
    } joiner{soa};
    if (N) {
        CAPI_HIP(hipMalloc(&im.steps, N * 4));
        tick("steps: hipMalloc");
        CAPI_HIP(fgfa_dev::staged_copy(im.steps, v.steps.data, N * 4, hipMemcpyHostToDevice, im.stream));
    }
    tick("steps: upload");
    soa.join();
    tick("span arrays on the host (beside the upload)");
    if (P || S) {
        CAPI_HIP(hipMalloc(&im.small, (2 * Pa + 3 * Sa + 4 * Pa) * 4));  // (the last 4 * Pa words: two u64 sums per path)
        CAPI_HIP(fgfa_dev::staged_copy(im.small, host.data(), host.size() * 4, hipMemcpyHostToDevice, nullptr));
        im.pb = im.small;
        im.pe = im.small + Pa;
        im.seg_len = im.small + 2 * Pa;
        im.depth = im.seg_len + Sa;
        im.uniq = im.depth + Sa;
        im.sums = im.uniq + Sa;  // (256-byte aligned: every sub-array is)
    }
    flatgfa_dev_graph_t g{im.steps, (uint64_t)N, im.pb, im.pe, (uint32_t)P, (uint32_t)S, im.seg_len};
    tick("paths, segments, outputs");
    const auto t_plan = std::chrono::steady_clock::now();
    int first_rc = FLATGFA_OK;
    im.plan = S ? flatgfa_dev_plan_create_first(&g, h_pb, h_pe, im.depth, im.uniq, &first_rc) : flatgfa_dev_plan_create(&g, h_pb, h_pe);
    const auto t_done = std::chrono::steady_clock::now();
    tick("plan (scratch + item lists)");
    if (!im.plan) return FLATGFA_ERR_HIP;  // the spans were checked above: what is left is the HIP runtime (see flatgfa_last_error)
    im.keep = true;
    cs->h2d_ms = std::chrono::duration<double, std::milli>(t_plan - t_enter).count();
    cs->plan_ms = std::chrono::duration<double, std::milli>(t_done - t_plan).count();
    cs->device = device;
    cs->stream = im.stream;
    cs->d_steps = im.steps;
    cs->d_small = im.small;
    cs->d_path_begin = im.pb;
    cs->d_path_end = im.pe;
    cs->d_seg_len = im.seg_len;
    cs->d_depth = im.depth;
    cs->d_uniq = im.uniq;
    cs->d_sums = reinterpret_cast<uint64_t *>(im.sums);
    cs->h_path_begin.assign(h_pb, h_pb + P);
    cs->h_path_end.assign(h_pe, h_pe + P);
    cs->h_soa.swap(host);  // (kept until the handle goes: four megabytes unmapped here would be ten milliseconds on the first query's copy)
    cs->plan = im.plan;
    cs->first_answer = S != 0;
    cs->first_rc = first_rc;
    cs->on_device = true;
    return FLATGFA_OK;
}

int flatgfa_to_device(flatgfa_t gfa, int device) {
    if (!gfa) { set_error("flatgfa_to_device: NULL handle"); return FLATGFA_ERR_ARG; }
    return ensure_device(gfa, device);
}

int flatgfa_residency_ms(flatgfa_t gfa, double *h2d_ms, double *plan_ms) {
    if (!gfa) { set_error("flatgfa_residency_ms: NULL handle"); return FLATGFA_ERR_ARG; }
    std::lock_guard<std::mutex> lk(gfa->dev_mu);
    if (!gfa->on_device) { set_error("flatgfa_residency_ms: the graph is not resident"); return FLATGFA_ERR_ARG; }
    if (h2d_ms) *h2d_ms = gfa->h2d_ms;
    if (plan_ms) *plan_ms = gfa->plan_ms;
    return FLATGFA_OK;
}

// Runs the node-depth kernels and leaves u32 results in cs->d_depth / cs->d_uniq.
static int run_seg_depth(CStore *cs, bool want_uniq) {
    int rc = ensure_device(cs, -1);
    if (rc) return rc;
    if (cs->first_answer) {  // (the query that sized the plan left both vectors here: the reference's consumers ask once per graph, cmds.rs:234-285)
        cs->first_answer = false;
        if (cs->first_rc) set_error("a step refers to a segment id (or a query to a path id) that is out of range");
        return cs->first_rc;
    }
    rc = flatgfa_dev_seg_depth(cs->plan, cs->d_depth, want_uniq ? cs->d_uniq : nullptr, cs->stream);
    if (rc) return rc;
    return flatgfa_dev_status(cs->plan, cs->stream);
}

static int fetch_widen(CStore *cs, const uint32_t *dev, uint64_t *out) {
    const size_t S = cs->view.segs.len;
    std::vector<uint32_t> tmp(S);
    if (S) CAPI_HIP(hipMemcpy(tmp.data(), dev, S * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < S; ++i) out[i] = tmp[i];  // Vec<usize>
    return FLATGFA_OK;
}

// Both result vectors as the device left them (u32; they lie next to each other in the handle's allocation, 256-byte aligned), fetched
// in ONE copy -- through one of the process's pinned staging buffers where they fit one: the link's rate, a pageable target gets a third
// of it -- and handed to `use(depth32, uniq32)`.
extern "C++" {
template <class F>
static int with_both_u32(CStore *gfa, F use) {
    const size_t S = gfa->view.segs.len, gap = (size_t)(gfa->d_uniq - gfa->d_depth);
    if ((gap + S) * 4 <= fgfa_dev::kStagingBytes) {
        char *pinned = nullptr;
        const auto lk = fgfa_dev::borrow_staging(&pinned);
        if (pinned) {
            CAPI_HIP(hipMemcpyAsync(pinned, gfa->d_depth, (gap + S) * 4, hipMemcpyDeviceToHost, gfa->stream));
            CAPI_HIP(hipStreamSynchronize(gfa->stream));
            const uint32_t *src = reinterpret_cast<const uint32_t *>(pinned);
            return use(src, src + gap);
        }
    }
    std::unique_ptr<uint32_t[]> tmp(new uint32_t[gap + S]);
    CAPI_HIP(hipMemcpy(tmp.get(), gfa->d_depth, (gap + S) * 4, hipMemcpyDeviceToHost));
    return use(tmp.get(), tmp.get() + gap);
}
}  // extern "C++"

int flatgfa_seg_depth(flatgfa_t gfa, uint64_t *depth_out, uint64_t *uniq_out) {
    if (!gfa || (!depth_out && gfa->view.segs.len)) { set_error("flatgfa_seg_depth: NULL argument"); return FLATGFA_ERR_ARG; }
    std::lock_guard<std::mutex> op(gfa->op_mu);
    int rc = run_seg_depth(gfa, uniq_out != nullptr);
    if (rc) return rc;
    if (!uniq_out) return fetch_widen(gfa, gfa->d_depth, depth_out);
    const size_t S = gfa->view.segs.len;
    if (!S) return FLATGFA_OK;
    return with_both_u32(gfa, [&](const uint32_t *d32, const uint32_t *u32) {  // widened to Vec<usize> on a few threads
        // (the caller's vectors are as a rule fresh pages: 16 MB of first touches for a million segments, which is what the threads share)
        const unsigned per = S >= (1u << 18) ? 4u : 1u;
        std::vector<std::thread> others;
        const auto widen = [&](unsigned k) {
            const uint32_t *src = k < per ? d32 : u32;
            uint64_t *dst = k < per ? depth_out : uniq_out;
            const unsigned j = k % per;
            for (size_t i = S * j / per, e = S * (j + 1) / per; i < e; ++i) dst[i] = src[i];
        };
        for (unsigned k = 1; k < 2 * per; ++k) others.emplace_back(widen, k);
        widen(0);
        for (auto &t : others) t.join();
        return (int)FLATGFA_OK;
    });
}

int flatgfa_path_depth(flatgfa_t gfa, const uint32_t *path_ids, uint32_t n_ids, uint64_t *length_out,
                       double *mean_out) {
    if (!gfa || (n_ids && (!path_ids || !length_out || !mean_out))) {
        set_error("flatgfa_path_depth: NULL argument");
        return FLATGFA_ERR_ARG;
    }
    for (uint32_t k = 0; k < n_ids; ++k)
        if (path_ids[k] >= gfa->view.paths.len) { set_error("flatgfa_path_depth: path id out of range"); return FLATGFA_ERR_BOUNDS; }
    // pass 1 over ALL paths (depth.rs:94-99), pass 2 over the requested ones (:104-108).  The device
    // forms every path's two sums in the pass that accumulates node depth (one read of the
    // steps); the requested ones are picked here.
    std::lock_guard<std::mutex> op(gfa->op_mu);
    int rc = ensure_device(gfa, -1);
    if (rc) return rc;
    const size_t P = gfa->view.paths.len;
    if (n_ids == 0 || P == 0) return run_seg_depth(gfa, false);
    uint64_t *d_sums = gfa->d_sums;  // (the handle's own: a hipMalloc per call cost five times the kernels it bracketed)
    std::vector<uint64_t> sums(P * 2);
    gfa->first_answer = false;  // (d_depth is written again)
    rc = flatgfa_dev_path_depth_all(gfa->plan, gfa->d_depth, d_sums, d_sums + P, gfa->stream);
    if (!rc) rc = flatgfa_dev_status(gfa->plan, gfa->stream);
    if (!rc && hipMemcpy(sums.data(), d_sums, P * 16, hipMemcpyDeviceToHost) != hipSuccess) rc = FLATGFA_ERR_HIP;
    if (rc) return rc;
    for (uint32_t k = 0; k < n_ids; ++k) {
        const uint64_t ln = sums[path_ids[k]], ws = sums[P + path_ids[k]];
        length_out[k] = ln;
        // the one floating-point operation on this path: depth.rs:129
        mean_out[k] = (double)ws / (double)ln;
    }
    return FLATGFA_OK;
}

int flatgfa_depth_table(flatgfa_t gfa, char **text, size_t *len) {
    if (!gfa || !text) { set_error("flatgfa_depth_table: NULL argument"); return FLATGFA_ERR_ARG; }
    const size_t S = gfa->view.segs.len;
    if (!S) {
        std::string out;
        fgfa::emit_seg_depth(gfa->view, nullptr, nullptr, &out);
        return give_text(out, text, len);
    }
    // the table straight from the device's 32-bit counts into the buffer the caller gets: no widened vectors, no intermediate string
    std::lock_guard<std::mutex> op(gfa->op_mu);
    int rc = run_seg_depth(gfa, true);
    if (rc) return rc;
    return with_both_u32(gfa, [&](const uint32_t *d32, const uint32_t *u32) {
        size_t n = 0;
        char *p = fgfa::emit_seg_depth_u32_malloc(gfa->view, d32, u32, &n);
        if (!p) { set_error("out of memory"); return (int)FLATGFA_ERR_IO; }
        *text = p;
        if (len) *len = n;
        return (int)FLATGFA_OK;
    });
}

int flatgfa_path_depth_table(flatgfa_t gfa, const uint32_t *path_ids, uint32_t n_ids, char **text, size_t *len) {
    if (!gfa || !text) { set_error("flatgfa_path_depth_table: NULL argument"); return FLATGFA_ERR_ARG; }
    std::vector<uint32_t> all;
    if (!path_ids) {
        all.resize(gfa->view.paths.len);
        for (size_t i = 0; i < all.size(); ++i) all[i] = (uint32_t)i;
        path_ids = all.data();
        n_ids = (uint32_t)all.size();
    }
    std::vector<uint64_t> lens(n_ids);
    std::vector<double> means(n_ids);
    int rc = flatgfa_path_depth(gfa, path_ids, n_ids, lens.data(), means.data());
    if (rc) return rc;
    std::string out;
    fgfa::emit_path_depth(gfa->view, path_ids, n_ids, lens.data(), means.data(), &out);
    return give_text(out, text, len);
}

int flatgfa_path_depth_bed(flatgfa_t gfa, const uint32_t *path_ids, uint32_t n_ids, char **text, size_t *len) {
    if (!gfa || !text) { set_error("flatgfa_path_depth_bed: NULL argument"); return FLATGFA_ERR_ARG; }
    std::vector<uint32_t> all;
    if (!path_ids) {
        all.resize(gfa->view.paths.len);
        for (size_t i = 0; i < all.size(); ++i) all[i] = (uint32_t)i;
        path_ids = all.data();
        n_ids = (uint32_t)all.size();
    }
    // as_bed keeps what path_depth computed as `lengths` (depth.rs:104-108, 173-183): same call, depths dropped
    std::vector<uint64_t> lens(n_ids);
    std::vector<double> means(n_ids);
    int rc = flatgfa_path_depth(gfa, path_ids, n_ids, lens.data(), means.data());
    if (rc) return rc;
    std::string out;
    for (uint32_t k = 0; k < n_ids; ++k) {
        const fgfa::Path &p = gfa->view.paths[path_ids[k]];
        out.append((const char *)gfa->view.name_data.data + p.name.start, p.name.len());
        out += "\t0\t" + std::to_string(lens[k]) + "\n";
    }
    return give_text(out, text, len);
}

// ---- f1: path-pair overlap (slow_odgi/overlap.py) ----

int flatgfa_path_overlaps(flatgfa_t gfa, const uint32_t *query_ids, uint32_t n_q, uint8_t *touch_out) {
    if (!gfa || (n_q && (!query_ids || !touch_out))) { set_error("flatgfa_path_overlaps: NULL argument"); return FLATGFA_ERR_ARG; }
    const size_t P = gfa->view.paths.len;
    for (uint32_t k = 0; k < n_q; ++k)
        if (query_ids[k] >= P) { set_error("flatgfa_path_overlaps: path id out of range"); return FLATGFA_ERR_BOUNDS; }
    if (n_q == 0 || P == 0) return FLATGFA_OK;
    std::lock_guard<std::mutex> op(gfa->op_mu);
    int rc = ensure_device(gfa, -1);
    if (rc) return rc;
    uint32_t *d_q = nullptr;
    uint8_t *d_t = nullptr;
    CAPI_HIP(hipMalloc(&d_q, (size_t)n_q * 4));
    if (hipMalloc(&d_t, (size_t)n_q * P) != hipSuccess) { (void)hipFree(d_q); set_error("hipMalloc failed"); return FLATGFA_ERR_HIP; }
    rc = FLATGFA_OK;
    if (hipMemcpyAsync(d_q, query_ids, (size_t)n_q * 4, hipMemcpyHostToDevice, gfa->stream) != hipSuccess) rc = FLATGFA_ERR_HIP;
    if (!rc) rc = flatgfa_dev_path_overlaps(gfa->plan, d_q, n_q, d_t, gfa->stream);
    if (!rc) rc = flatgfa_dev_status(gfa->plan, gfa->stream);
    if (!rc && hipMemcpy(touch_out, d_t, (size_t)n_q * P, hipMemcpyDeviceToHost) != hipSuccess) rc = FLATGFA_ERR_HIP;
    (void)hipFree(d_q);
    (void)hipFree(d_t);
    return rc;
}

int flatgfa_overlap_table(flatgfa_t gfa, const uint32_t *query_ids, uint32_t n_q, char **text, size_t *len) {
    if (!gfa || !text) { set_error("flatgfa_overlap_table: NULL argument"); return FLATGFA_ERR_ARG; }
    const size_t P = gfa->view.paths.len;
    std::vector<uint8_t> touch((size_t)n_q * P);
    int rc = flatgfa_path_overlaps(gfa, query_ids, n_q, touch.data());
    if (rc) return rc;
    if (!steps_name_segments(gfa)) return FLATGFA_ERR_BOUNDS;
    std::vector<uint64_t> plen(n_q);  // len(pathseq[ip]): the path's length in base pairs
    for (uint32_t k = 0; k < n_q; ++k) plen[k] = fgfa::path_length(gfa->view, query_ids[k]);
    std::string out;
    fgfa::emit_overlap(gfa->view, query_ids, n_q, plen.data(), touch.data(), &out);
    return give_text(out, text, len);
}

// ---- f2: window / interval depth (ops/window_depth.rs) ----

int flatgfa_interval_depth(flatgfa_t gfa, uint32_t path_index, const uint64_t *starts, const uint64_t *ends,
                           uint64_t n, double *depth_out) {
    if (!gfa || (n && (!starts || !ends || !depth_out))) { set_error("flatgfa_interval_depth: NULL argument"); return FLATGFA_ERR_ARG; }
    if (path_index >= gfa->view.paths.len) { set_error("flatgfa_interval_depth: path id out of range"); return FLATGFA_ERR_BOUNDS; }
    std::vector<uint64_t> depth(gfa->view.segs.len);
    int rc = flatgfa_seg_depth(gfa, depth.data(), nullptr);  // interval_depth calls seg_depth, window_depth.rs:177
    if (rc) return rc;
    std::vector<fgfa::BedEntry> win(n);
    for (uint64_t i = 0; i < n; ++i) win[i] = fgfa::BedEntry{0u, 0u, starts[i], ends[i]};
    fgfa::interval_depth(gfa->view, depth.data(), path_index, win.data(), n, depth_out);
    return FLATGFA_OK;
}

static int bed_depth_common(flatgfa_t gfa, uint32_t path_index, const fgfa::Bed &bed, char **text, size_t *len) {
    std::vector<uint64_t> depth(gfa->view.segs.len);
    int rc = flatgfa_seg_depth(gfa, depth.data(), nullptr);
    if (rc) return rc;
    std::vector<double> out(bed.entries.size());
    fgfa::interval_depth(gfa->view, depth.data(), path_index, bed.entries.data(), bed.entries.size(), out.data());
    std::string s;
    fgfa::emit_interval_depth(bed, out.data(), &s);
    return give_text(s, text, len);
}

int flatgfa_window_depth_table(flatgfa_t gfa, uint32_t path_index, uint64_t window, char **text, size_t *len) {
    if (!gfa || !text) { set_error("flatgfa_window_depth_table: NULL argument"); return FLATGFA_ERR_ARG; }
    if (path_index >= gfa->view.paths.len) { set_error("window depth: path not found"); return FLATGFA_ERR_BOUNDS; }
    if (window == 0) { set_error("window depth: window size must be positive"); return FLATGFA_ERR_ARG; }  // div_ceil by zero panics
    if (!steps_name_segments(gfa)) return FLATGFA_ERR_BOUNDS;
    const fgfa::Path &p = gfa->view.paths[path_index];
    fgfa::Bed bed;
    fgfa::make_windows(gfa->view.name_data.data + p.name.start, p.name.len(), 0, fgfa::path_length(gfa->view, path_index),
                       window, &bed);
    return bed_depth_common(gfa, path_index, bed, text, len);
}

int flatgfa_bed_depth_table(flatgfa_t gfa, const uint8_t *bed_text, size_t bed_len, char **text, size_t *len) {
    if (!gfa || !text || (bed_len && !bed_text)) { set_error("flatgfa_bed_depth_table: NULL argument"); return FLATGFA_ERR_ARG; }
    fgfa::Bed bed;
    std::string err;
    if (!fgfa::parse_bed(bed_text, bed_len, &bed, &err)) { set_error(err); return FLATGFA_ERR_BOUNDS; }
    if (bed.entries.empty()) { set_error("BED: no intervals"); return FLATGFA_ERR_BOUNDS; }  // entries.all()[0] panics
    // all intervals are taken to lie on the path named by the first entry (window_depth.rs:204-210)
    const fgfa::BedEntry &e0 = bed.entries[0];
    int64_t path = gfa->view.find_path(bed.name_data.data() + e0.name_start, e0.name_end - e0.name_start);
    if (path < 0) { set_error("BED: path not found in graph"); return FLATGFA_ERR_BOUNDS; }
    return bed_depth_common(gfa, (uint32_t)path, bed, text, len);
}

// ---- f2 on many paths: the interval walk on the device too (interval_device.hip) ----

extern "C++" {
namespace {
// depth_out[k] for interval k on path ids[k], under the handle's op_mu.  Node depth goes into d_depth first unless the
// caller has just left it there (depth_ready); it stays on the device, and only the n doubles come back.
int intervals_depth_locked(CStore *gfa, DevScope *sc, const uint32_t *ids, const uint64_t *starts, const uint64_t *ends, uint64_t n,
                           bool depth_ready, double *depth_out) {
    if (!depth_ready)
        if (int rc = run_seg_depth(gfa, false)) return rc;
    CAPI_HIP(hipStreamSynchronize(gfa->stream));  // (the job runs on the scope's stream)
    const fgfa::View &v = gfa->view;
    fgfa_dev::IntervalGraph g;
    g.steps = gfa->d_steps, g.n_steps = v.steps.len;
    g.begin = gfa->h_path_begin.data(), g.end = gfa->h_path_end.data(), g.n_paths = (uint32_t)v.paths.len;
    g.seg_len = gfa->d_seg_len, g.depth = gfa->d_depth, g.n_segs = (uint32_t)v.segs.len;
    uint32_t *d_ids = nullptr;
    uint64_t *d_starts = nullptr, *d_ends = nullptr;
    double *d_out = nullptr;
    CAPI_HIP(sc->upload(&d_ids, ids, n));
    CAPI_HIP(sc->upload(&d_starts, starts, n));
    CAPI_HIP(sc->upload(&d_ends, ends, n));
    CAPI_HIP(sc->alloc(&d_out, n));
    uint32_t cut = fgfa_dev::kIntervalLaneCut;
    if (const char *h = test_hook("FLATGFA_INTERVAL_LANE_CUT")) cut = (uint32_t)strtoul(h, nullptr, 10);
    fgfa_dev::IntervalJob *job = sc->hold<fgfa_dev::IntervalJob, fgfa_dev::interval_free>(fgfa_dev::interval_new(fgfa_dev::kIntervalScratchSteps, cut));
    const fgfa_dev::IntervalList iv{d_ids, d_starts, d_ends, n};
    if (int rc = fgfa_dev::interval_depth(job, g, iv, ids, sc->stream, d_out)) return rc;
    CAPI_HIP(fgfa_dev::staged_copy(depth_out, d_out, n * sizeof(double), hipMemcpyDeviceToHost, sc->stream));
    return FLATGFA_OK;
}

// the table of `bed`'s entries, entry k on path ids[k]: one job, or one per stretch of `cuts` (window_table_cuts), so that no
// group reaches across a cut
int intervals_table_locked(CStore *gfa, DevScope *sc, const fgfa::Bed &bed, const std::vector<uint32_t> &ids, bool depth_ready, char **text,
                           size_t *len, const std::vector<size_t> *cuts = nullptr) {
    const size_t n = bed.entries.size();
    std::vector<uint64_t> starts(n), ends(n);
    for (size_t k = 0; k < n; ++k) starts[k] = bed.entries[k].start, ends[k] = bed.entries[k].end;
    std::vector<double> out(n);
    const std::vector<size_t> whole = {0, n};
    if (!cuts) cuts = &whole;
    for (size_t s = 0; s + 1 < cuts->size(); ++s) {
        const size_t a = (*cuts)[s], b = (*cuts)[s + 1];
        if (b <= a) continue;  // (no entries)
        // (the first job leaves d_depth as it found or made it)
        if (int rc = intervals_depth_locked(gfa, sc, ids.data() + a, starts.data() + a, ends.data() + a, b - a, depth_ready || s, out.data() + a)) return rc;
    }
    std::string s;
    fgfa::emit_interval_depth(bed, out.data(), &s);
    return give_text(s, text, len);
}
}  // namespace
}  // extern "C++"

int flatgfa_intervals_depth(flatgfa_t gfa, const uint32_t *path_ids, const uint64_t *starts, const uint64_t *ends, uint64_t n_intervals,
                            double *depth_out) {
    if (!gfa || (n_intervals && (!path_ids || !starts || !ends || !depth_out))) {
        set_error("flatgfa_intervals_depth: NULL argument");
        return FLATGFA_ERR_ARG;
    }
    if (!n_intervals) return FLATGFA_OK;
    for (uint64_t k = 0; k < n_intervals; ++k)
        if (path_ids[k] >= gfa->view.paths.len) { set_error("flatgfa_intervals_depth: path id out of range"); return FLATGFA_ERR_BOUNDS; }
    std::lock_guard<std::mutex> op(gfa->op_mu);
    DevScope sc;
    if (int rc = open_scope(gfa, &sc, "interval depth")) return rc;
    if (int rc = ensure_device(gfa, -1)) return rc;
    return intervals_depth_locked(gfa, &sc, path_ids, starts, ends, n_intervals, false, depth_out);
}

int flatgfa_window_depth_paths_table(flatgfa_t gfa, const uint32_t *path_ids, uint32_t n_ids, uint64_t window, char **text, size_t *len) {
    if (text) *text = nullptr;
    if (len) *len = 0;
    if (!gfa || !text) { set_error("flatgfa_window_depth_paths_table: NULL argument"); return FLATGFA_ERR_ARG; }
    if (window == 0) { set_error("window depth: window size must be positive"); return FLATGFA_ERR_ARG; }
    const size_t P = gfa->view.paths.len;
    std::vector<uint32_t> all;
    if (!path_ids) {
        all.resize(P);
        for (size_t i = 0; i < P; ++i) all[i] = (uint32_t)i;
        path_ids = all.data();
        n_ids = (uint32_t)P;
    }
    for (uint32_t k = 0; k < n_ids; ++k)
        if (path_ids[k] >= P) { set_error("window depth: path not found"); return FLATGFA_ERR_BOUNDS; }
    std::lock_guard<std::mutex> op(gfa->op_mu);
    DevScope sc;
    if (int rc = open_scope(gfa, &sc, "window depth")) return rc;
    if (int rc = ensure_device(gfa, -1)) return rc;
    fgfa::Bed bed;
    std::vector<uint32_t> ids;
    if (!n_ids) return intervals_table_locked(gfa, &sc, bed, ids, false, text, len);
    // every path's length comes out of the pass that forms the node depth (flatgfa_path_depth's): one read of the steps for
    // both, and d_depth is left where the interval job reads it
    gfa->first_answer = false;  // (d_depth is written again)
    int rc = flatgfa_dev_path_depth_all(gfa->plan, gfa->d_depth, gfa->d_sums, gfa->d_sums + P, gfa->stream);
    if (!rc) rc = flatgfa_dev_status(gfa->plan, gfa->stream);
    if (rc) return rc;
    std::vector<uint64_t> plen(P), lens(n_ids);
    CAPI_HIP(fgfa_dev::staged_copy(plen.data(), gfa->d_sums, P * 8, hipMemcpyDeviceToHost, gfa->stream));
    for (uint32_t k = 0; k < n_ids; ++k) lens[k] = plen[path_ids[k]];
    // a path listed again behind itself (paths without windows in between or not) is a table of its own, not more intervals of
    // one group: the job runs once per stretch without such a seam -- once, for a list that has none
    std::vector<size_t> path_entry, cuts;
    fgfa::make_paths_windows(gfa->view, path_ids, n_ids, lens.data(), window, &bed, &ids, &path_entry);
    fgfa::window_table_cuts(path_ids, n_ids, path_entry, &cuts);
    return intervals_table_locked(gfa, &sc, bed, ids, true, text, len, &cuts);
}

int flatgfa_bed_depth_paths_table(flatgfa_t gfa, const uint8_t *bed_text, size_t bed_len, char **text, size_t *len) {
    if (text) *text = nullptr;
    if (len) *len = 0;
    if (!gfa || !text || (bed_len && !bed_text)) { set_error("flatgfa_bed_depth_paths_table: NULL argument"); return FLATGFA_ERR_ARG; }
    fgfa::Bed bed;
    std::string err;
    if (!fgfa::parse_bed(bed_text, bed_len, &bed, &err)) { set_error(err); return FLATGFA_ERR_BOUNDS; }
    if (bed.entries.empty()) { set_error("BED: no intervals"); return FLATGFA_ERR_BOUNDS; }
    std::vector<uint32_t> ids;
    size_t bad = 0;
    if (!fgfa::bed_entry_paths(gfa->view, bed, &ids, &bad)) {
        set_error("BED: entry " + std::to_string(bad) + " names a path that is not in the graph");
        return FLATGFA_ERR_BOUNDS;
    }
    std::lock_guard<std::mutex> op(gfa->op_mu);
    DevScope sc;
    if (int rc = open_scope(gfa, &sc, "interval depth")) return rc;
    if (int rc = ensure_device(gfa, -1)) return rc;
    return intervals_table_locked(gfa, &sc, bed, ids, false, text, len);
}

// ---- f3: node depth over a subset of paths (odgi depth -d -s) ----

int flatgfa_seg_depth_subset(flatgfa_t gfa, const uint32_t *path_ids, uint32_t n_ids, uint64_t *depth_out,
                             uint64_t *uniq_out) {
    if (!gfa || (n_ids && !path_ids) || (!depth_out && gfa->view.segs.len)) {
        set_error("flatgfa_seg_depth_subset: NULL argument");
        return FLATGFA_ERR_ARG;
    }
    const size_t P = gfa->view.paths.len, S = gfa->view.segs.len;
    for (uint32_t k = 0; k < n_ids; ++k)
        if (path_ids[k] >= P) { set_error("flatgfa_seg_depth_subset: path id out of range"); return FLATGFA_ERR_BOUNDS; }
    std::lock_guard<std::mutex> op(gfa->op_mu);
    int rc = ensure_device(gfa, -1);
    if (rc) return rc;
    // A prepared query over the same resident steps, with only the chosen paths' spans.  It is kept:
    // asking again for the same subset (a table after the vectors, say) costs the kernels alone.
    const bool same = gfa->sub_plan && gfa->sub_ids.size() == n_ids &&
                      std::equal(gfa->sub_ids.begin(), gfa->sub_ids.end(), path_ids);
    if (!same) {
        if (gfa->sub_plan) flatgfa_dev_plan_destroy(gfa->sub_plan);
        if (gfa->d_sub_spans) (void)hipFree(gfa->d_sub_spans);
        gfa->sub_plan = nullptr;
        gfa->d_sub_spans = nullptr;
        gfa->sub_ids.clear();
        std::vector<uint32_t> span(2 * (size_t)n_ids);
        for (uint32_t k = 0; k < n_ids; ++k) {
            span[k] = gfa->h_path_begin[path_ids[k]];
            span[n_ids + k] = gfa->h_path_end[path_ids[k]];
        }
        if (n_ids) {
            CAPI_HIP(hipMalloc(&gfa->d_sub_spans, span.size() * 4));
            if (hipMemcpy(gfa->d_sub_spans, span.data(), span.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
                (void)hipFree(gfa->d_sub_spans);
                gfa->d_sub_spans = nullptr;
                set_error("flatgfa_seg_depth_subset: copying the path spans to the device failed");
                return FLATGFA_ERR_HIP;
            }
        }
        flatgfa_dev_graph_t g{gfa->d_steps, (uint64_t)gfa->view.steps.len, gfa->d_sub_spans,
                              gfa->d_sub_spans ? gfa->d_sub_spans + n_ids : nullptr, n_ids, (uint32_t)S, gfa->d_seg_len};
        gfa->sub_plan = flatgfa_dev_plan_create(&g, span.data(), span.data() + n_ids);
        if (!gfa->sub_plan) return FLATGFA_ERR_HIP;
        gfa->sub_ids.assign(path_ids, path_ids + n_ids);
    }
    gfa->first_answer = false;  // (the handle's result buffers now hold the subset's counts)
    rc = flatgfa_dev_seg_depth(gfa->sub_plan, gfa->d_depth, uniq_out ? gfa->d_uniq : nullptr, gfa->stream);
    if (!rc) rc = flatgfa_dev_status(gfa->sub_plan, gfa->stream);
    if (!rc) rc = fetch_widen(gfa, gfa->d_depth, depth_out);
    if (!rc && uniq_out) rc = fetch_widen(gfa, gfa->d_uniq, uniq_out);
    return rc;
}

// ---- pangenotype matrix from GAF text (ops/pangenotype.rs) ----

// The handle's name table on `device` (the current device), made once: NameMap::build over the segments (namemap.rs:36-42).
static int ensure_gaf_names(CStore *cs, int device) {
    if (cs->gaf_device == device) return FLATGFA_OK;
    const fgfa::View &v = cs->view;
    if (v.segs.len > 0x80000000ull) { set_error("pangenotype: more than 2^31 segments"); return FLATGFA_ERR_TOO_LARGE; }
    fgfa::NameMap names;
    for (size_t i = 0; i < v.segs.len; ++i) names.insert(v.segs[i].name, (uint32_t)i);
    uint64_t seq_max = 0;
    std::vector<std::pair<uint64_t, uint32_t>> others;
    names.export_sorted(&seq_max, &others);
    const size_t n = others.size();
    std::vector<uint64_t> host(n + (n + 1) / 2, 0);
    uint32_t *ids = reinterpret_cast<uint32_t *>(host.data() + n);
    for (size_t i = 0; i < n; ++i) {
        host[i] = others[i].first;
        ids[i] = others[i].second;
    }
    uint64_t *d = nullptr;
    if (n) {
        CAPI_HIP(hipMalloc(&d, host.size() * 8));
        if (hipMemcpy(d, host.data(), host.size() * 8, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(d);
            set_error("pangenotype: copying the name table to the device failed");
            return FLATGFA_ERR_HIP;
        }
    }
    if (cs->d_gaf_names) {
        if (cs->gaf_ev) (void)hipEventSynchronize(cs->gaf_ev);  // (a device-entry call may still read the old one)
        (void)hipFree(cs->d_gaf_names);
    }
    cs->d_gaf_names = d;
    cs->gaf_names.keys = d;
    cs->gaf_names.ids = d ? reinterpret_cast<const uint32_t *>(d + n) : nullptr;
    cs->gaf_names.n_others = (uint32_t)n;
    cs->gaf_names.n_segs = (uint32_t)v.segs.len;
    cs->gaf_names.seq_max = seq_max;
    cs->gaf_device = device;
    return FLATGFA_OK;
}

static int gaf_bad_line(uint32_t file, uint64_t offset) {
    set_error("pangenotype: GAF file " + std::to_string(file) + ": the line at byte offset " + std::to_string(offset) +
              " names a segment that is not in the graph");
    return FLATGFA_ERR_BOUNDS;
}

int flatgfa_pangenotype_matrix(flatgfa_t gfa, const uint8_t *const *gaf, const size_t *gaf_len, uint32_t n_files,
                               uint64_t *bits_out) {
    if (!gfa || (n_files && (!gaf || !gaf_len || !bits_out))) { set_error("flatgfa_pangenotype_matrix: NULL argument"); return FLATGFA_ERR_ARG; }
    for (uint32_t f = 0; f < n_files; ++f)
        if (gaf_len[f] && !gaf[f]) { set_error("flatgfa_pangenotype_matrix: NULL text with a length"); return FLATGFA_ERR_ARG; }
    if (n_files == 0) return FLATGFA_OK;
    std::lock_guard<std::mutex> op(gfa->op_mu);
    DevScope sc;
    if (int rc = open_scope(gfa, &sc, "the pangenotype matrix")) return rc;
    int rc = ensure_gaf_names(gfa, sc.device);
    if (rc) return rc;
    const size_t S = gfa->view.segs.len, W = (S + 63) / 64;

    // Every file's chunks (fgfa::cut_lines), one file behind another; the bytes behind a file's last '\n' are dropped.
    std::vector<std::pair<size_t, size_t>> pieces;
    std::vector<size_t> first(n_files + 1, 0);  // file f's pieces are [first[f], first[f + 1])
    const size_t target = gaf_chunk_bytes();
    for (uint32_t f = 0; f < n_files; ++f) {
        fgfa::cut_lines(gaf[f], gaf_len[f], target, &pieces);
        first[f + 1] = pieces.size();
    }
    size_t cap = 16;
    for (const auto &pc : pieces) cap = std::max(cap, pc.second - pc.first);
    cap = (cap + 255) & ~(size_t)255;
    const size_t scratch_words = fgfa_dev::gaf_scratch_words(nullptr, cap);  // (the text buffers are 256-byte aligned)

    // One allocation: two text buffers and their scratch, the row, the first bad offset.
    uint8_t *block = nullptr;
    const size_t per = (cap + scratch_words * 8 + 255) & ~(size_t)255;
    CAPI_HIP(sc.alloc(&block, 2 * per + W * 8 + 8));
    hipStream_t ks = sc.stream, cs = nullptr;
    hipEvent_t done[2] = {nullptr, nullptr};
    CAPI_HIP(sc.take_stream(&cs));
    for (int i = 0; i < 2; ++i) CAPI_HIP(sc.make_event(&done[i]));
    uint8_t *d_text[2] = {block, block + per};
    uint64_t *d_scratch[2] = {reinterpret_cast<uint64_t *>(block + cap), reinterpret_cast<uint64_t *>(block + per + cap)};
    uint64_t *d_row = reinterpret_cast<uint64_t *>(block + 2 * per), *d_bad = d_row + W;
    bool used[2] = {false, false};
    size_t k = 0;  // the next piece
    std::vector<uint64_t> bad(1);
    for (uint32_t f = 0; f < n_files; ++f) {
        if (W) CAPI_HIP(hipMemsetAsync(d_row, 0, W * 8, ks));
        CAPI_HIP(hipMemsetAsync(d_bad, 0xFF, 8, ks));
        for (; k < first[f + 1]; ++k) {
            const int b = (int)(k & 1);
            if (used[b]) CAPI_HIP(hipEventSynchronize(done[b]));  // the scan that read this buffer is over
            const size_t len = pieces[k].second - pieces[k].first;
            CAPI_HIP(fgfa_dev::staged_copy(d_text[b], gaf[f] + pieces[k].first, len, hipMemcpyHostToDevice, cs));  // (beside the scan of the piece before, on ks)
            CAPI_HIP(fgfa_dev::gaf_scan(d_text[b], len, gfa->gaf_names, d_row, d_bad, pieces[k].first, d_scratch[b], ks));
            CAPI_HIP(hipEventRecord(done[b], ks));
            used[b] = true;
        }
        if (W) CAPI_HIP(hipMemcpyAsync(bits_out + (size_t)f * W, d_row, W * 8, hipMemcpyDeviceToHost, ks));
        CAPI_HIP(hipMemcpyAsync(bad.data(), d_bad, 8, hipMemcpyDeviceToHost, ks));
        CAPI_HIP(hipStreamSynchronize(ks));
        if (bad[0] != ~0ull) return gaf_bad_line(f, bad[0]);
    }
    return FLATGFA_OK;
}

int flatgfa_pangenotype_table(flatgfa_t gfa, const uint8_t *const *gaf, const size_t *gaf_len, uint32_t n_files, char **text,
                              size_t *len) {
    if (!gfa || !text) { set_error("flatgfa_pangenotype_table: NULL argument"); return FLATGFA_ERR_ARG; }
    const size_t S = gfa->view.segs.len, W = (S + 63) / 64;
    std::vector<uint64_t> bits((size_t)n_files * W);
    const int rc = flatgfa_pangenotype_matrix(gfa, gaf, gaf_len, n_files, bits.empty() ? nullptr : bits.data());
    if (rc) return rc;
    // cmds.rs:466-474: a '1' or '0' per segment, a newline per file
    const size_t n = (size_t)n_files * (S + 1);
    char *p = (char *)malloc(n + 1);
    if (!p) { set_error("out of memory"); return FLATGFA_ERR_IO; }
    for (uint32_t f = 0; f < n_files; ++f) {
        char *o = p + (size_t)f * (S + 1);
        const uint64_t *row = bits.data() + (size_t)f * W;
        for (size_t s = 0; s < S; ++s) o[s] = (char)('0' + ((row[s >> 6] >> (s & 63)) & 1u));
        o[S] = '\n';
    }
    p[n] = 0;
    *text = p;
    if (len) *len = n;
    return FLATGFA_OK;
}

int flatgfa_dev_pangenotype_row(flatgfa_t gfa, const uint8_t *d_text, size_t len, uint64_t *d_row, uint64_t *d_first_bad,
                                void *stream_) {
    if (!gfa || (len && (!d_text || !d_first_bad)) || (len && gfa->view.segs.len && !d_row)) {
        set_error("flatgfa_dev_pangenotype_row: NULL argument");
        return FLATGFA_ERR_ARG;
    }
    if (len == 0) return FLATGFA_OK;
    hipStream_t stream = (hipStream_t)stream_;
    std::lock_guard<std::mutex> op(gfa->op_mu);
    int device = 0;
    CAPI_HIP(hipGetDevice(&device));
    int rc = ensure_gaf_names(gfa, device);
    if (rc) return rc;
    const size_t words = fgfa_dev::gaf_scratch_words(d_text, len);
    if (gfa->gaf_scratch_device != device || gfa->gaf_scratch_words < words) {
        if (gfa->gaf_ev) {  // the last call's kernels may still read the old scratch
            (void)hipEventSynchronize(gfa->gaf_ev);
            (void)hipEventDestroy(gfa->gaf_ev);
            gfa->gaf_ev = nullptr;
        }
        if (gfa->d_gaf_scratch) (void)hipFree(gfa->d_gaf_scratch);
        gfa->d_gaf_scratch = nullptr;
        gfa->gaf_scratch_words = 0;
        gfa->gaf_scratch_device = -1;
        CAPI_HIP(hipMalloc(&gfa->d_gaf_scratch, words * 8));
        gfa->gaf_scratch_words = words;
        gfa->gaf_scratch_device = device;
        CAPI_HIP(hipEventCreateWithFlags(&gfa->gaf_ev, hipEventDisableTiming));
    } else {
        CAPI_HIP(hipStreamWaitEvent(stream, gfa->gaf_ev, 0));  // (the scratch is free once the last call on any stream is done)
    }
    CAPI_HIP(fgfa_dev::gaf_scan(d_text, len, gfa->gaf_names, d_row, d_first_bad, 0, gfa->d_gaf_scratch, stream));
    CAPI_HIP(hipEventRecord(gfa->gaf_ev, stream));
    return FLATGFA_OK;
}

// ---- GAF lookup (ops/gaf.rs) ----

// The handle's sequence pool on `device` (the current device), made once.  A span that leaves seq_data, where the reference
// panics on the slice, is refused here: the gather reads what the spans say.
static int ensure_gaf_seqs(CStore *cs, int device) {
    if (cs->gaf_seq_device == device) return FLATGFA_OK;
    const fgfa::View &v = cs->view;
    const size_t S = v.segs.len, n_seq = v.seq_data.len;
    std::vector<uint32_t> seg_seq(2 * S + 2, 0);
    for (size_t i = 0; i < S; ++i) {
        const fgfa::Span sp = v.segs[i].seq;
        if (sp.start > sp.end || sp.end > n_seq) {
            set_error("gaf: segment " + std::to_string(i) + " has a sequence span outside seq_data");
            return FLATGFA_ERR_BOUNDS;
        }
        seg_seq[2 * i] = sp.start;
        seg_seq[2 * i + 1] = sp.end - sp.start;
    }
    const size_t head = (seg_seq.size() * 4 + 255) & ~(size_t)255;
    uint8_t *d = nullptr;
    CAPI_HIP(hipMalloc(&d, head + n_seq + 16));
    hipError_t e = fgfa_dev::staged_copy(d, seg_seq.data(), seg_seq.size() * 4, hipMemcpyHostToDevice, nullptr);
    if (e == hipSuccess && n_seq) e = fgfa_dev::staged_copy(d + head, v.seq_data.data, n_seq, hipMemcpyHostToDevice, nullptr);
    if (e != hipSuccess) {
        (void)hipFree(d);
        set_error(std::string("gaf: copying the sequence pool to the device failed: ") + hipGetErrorString(e));
        return FLATGFA_ERR_HIP;
    }
    if (cs->d_gaf_seg_seq) (void)hipFree(cs->d_gaf_seg_seq);  // (the handle moved to another device; hipFree waits for the memory's users)
    cs->d_gaf_seg_seq = reinterpret_cast<uint32_t *>(d);
    cs->d_gaf_seq_data = d + head;
    cs->gaf_seq_device = device;
    return FLATGFA_OK;
}

static int ensure_gaf_graph(CStore *cs, int device, fgfa_dev::GafGraph *g) {
    int rc = ensure_gaf_names(cs, device);
    if (!rc) rc = ensure_gaf_seqs(cs, device);
    if (rc) return rc;
    g->names = cs->gaf_names;
    g->seg_seq = cs->d_gaf_seg_seq;
    g->seq_data = cs->d_gaf_seq_data;
    return FLATGFA_OK;
}

// Which of a piece's bad lines decides (the one at the lowest offset), as a FLATGFA_* code with its message; 0 when none is bad.
static int gaf_lookup_verdict(const fgfa_dev::GafTotals &t, bool seqs) {
    const uint64_t bounds = std::min<uint64_t>(t.bad_name, seqs ? t.bad_slice : ~0ull);
    if (t.bad_parse == ~0ull && bounds == ~0ull) return FLATGFA_OK;
    if (t.bad_parse < bounds) {
        set_error("gaf: the line at byte offset " + std::to_string(t.bad_parse) +
                  " is not a GAF record (nine tabs, digits in fields 7 and 8)");
        return FLATGFA_ERR_PARSE;
    }
    set_error("gaf: the line at byte offset " + std::to_string(bounds) +
              (t.bad_name <= bounds ? " names a segment that is not in the graph" : " ends before it starts: its range cannot be sliced"));
    return FLATGFA_ERR_BOUNDS;
}

namespace {
enum GafMode { kGafCount, kGafSeqs, kGafEvents };
struct GafResult {
    uint64_t n_lines = 0, n_events = 0;
    char *text = nullptr;  // kGafSeqs: malloc'd
    uint64_t text_len = 0, text_cap = 0;
    std::vector<uint64_t> line_first, name_off, name_len, a, b;  // kGafEvents
    std::vector<uint32_t> handle;
    std::vector<uint8_t> kind;
    ~GafResult() { free(text); }
};
}  // namespace

// One lookup over host text: chunks cut after a '\n' go to the device through the pinned staging, each is counted, checked and
// -- when nothing in it is bad -- its answer comes back through the same staging, the `-s` text in pieces of a bounded size.
static int gaf_lookup_host(flatgfa_t gfa, const uint8_t *gaf, size_t len, GafMode mode, GafResult *res) {
    std::lock_guard<std::mutex> op(gfa->op_mu);
    DevScope sc;
    if (int rc = open_scope(gfa, &sc, "the GAF lookup")) return rc;
    const int device = sc.device;
    fgfa_dev::GafGraph graph;
    int rc = ensure_gaf_graph(gfa, device, &graph);
    if (rc) return rc;
    if (mode == kGafEvents) res->line_first.push_back(0);

    size_t out_bound = (size_t)64 << 20;
    if (const char *h = test_hook("FLATGFA_GAF_OUT_BYTES")) out_bound = std::max<size_t>(1, strtoull(h, nullptr, 10));  // tests
    std::vector<std::pair<size_t, size_t>> pieces;  // the chunks (what follows the last '\n' is not a line)
    fgfa::cut_lines(gaf, len, gaf_chunk_bytes(), &pieces);
    if (pieces.empty()) return FLATGFA_OK;
    size_t text_cap = 16;
    for (const auto &pc : pieces) text_cap = std::max(text_cap, pc.second - pc.first);
    text_cap = (text_cap + 255) & ~(size_t)255;

    // Two text buffers: the chunk behind the one being looked up travels to the device meanwhile, on a thread and a stream of
    // its own (a staged copy returns when the bytes have arrived).
    hipError_t up_err = hipSuccess;  // (declared before the thread that writes it is: it outlives the join)
    std::thread up;
    Joiner joiner{up};  // (declared after the scope: the copy is over before the scope gives its buffer and stream back)
    const hipStream_t st = sc.stream;
    hipStream_t cs = nullptr;
    CAPI_HIP(sc.take_stream(&cs));
    fgfa_dev::GafLookupJob *job = sc.hold<fgfa_dev::GafLookupJob, fgfa_dev::gaf_lookup_free>(fgfa_dev::gaf_lookup_new());
    uint8_t *d_texts = nullptr, *d_out = nullptr;
    CAPI_HIP(sc.alloc(&d_texts, (pieces.size() > 1 ? 2 : 1) * text_cap));
    size_t out_cap = 0;
    up_err = fgfa_dev::staged_copy(d_texts, gaf + pieces[0].first, pieces[0].second - pieces[0].first, hipMemcpyHostToDevice, cs);
    for (size_t k = 0; k < pieces.size(); ++k) {
        if (up.joinable()) up.join();
        CAPI_HIP(up_err);
        const size_t b = pieces[k].first, n = pieces[k].second - b;
        uint8_t *d_text = d_texts + (k & 1) * text_cap;
        if (k + 1 < pieces.size()) {  // (its buffer was read by chunk k - 1, which is done: every count and copy-back waited)
            uint8_t *d_next = d_texts + ((k + 1) & 1) * text_cap;
            const uint8_t *src = gaf + pieces[k + 1].first;
            const size_t bytes = pieces[k + 1].second - pieces[k + 1].first;
            up = std::thread([=, &up_err] {
                up_err = hipSetDevice(device);
                if (up_err == hipSuccess) up_err = fgfa_dev::staged_copy(d_next, src, bytes, hipMemcpyHostToDevice, cs);
            });
        }
        fgfa_dev::GafTotals t;
        rc = fgfa_dev::gaf_lookup_count(job, d_text, n, graph, mode == kGafSeqs, b, st, &t);
        if (!rc) rc = gaf_lookup_verdict(t, mode == kGafSeqs);  // (chunks go in text order: the first bad chunk holds the lowest offset)
        if (rc) return rc;
        const fgfa_dev::GafArrays &ar = fgfa_dev::gaf_lookup_arrays(job);
        const uint64_t L = t.n_lines, E = t.n_events;
        if (mode == kGafSeqs) {
            if (res->text_len + t.seq_bytes + 1 > res->text_cap) {
                const uint64_t cap = std::max<uint64_t>(res->text_len + t.seq_bytes + 1, res->text_cap + res->text_cap / 2);
                char *p = (char *)realloc(res->text, cap);
                if (!p) { set_error("out of memory"); return FLATGFA_ERR_IO; }
                res->text = p;
                res->text_cap = cap;
            }
            for (uint64_t o = 0; o < t.seq_bytes;) {  // the chunk's text, a bounded piece at a time
                const uint64_t m = std::min<uint64_t>(out_bound, t.seq_bytes - o);
                if (m > out_cap) {  // (at most a few times a call: it grows to twice what was needed, up to the bound)
                    uint8_t *old = d_out;
                    d_out = nullptr;
                    CAPI_HIP(sc.release(old));
                    out_cap = std::min<uint64_t>(out_bound, 2 * std::max<uint64_t>(m, t.seq_bytes));
                    CAPI_HIP(sc.alloc(&d_out, out_cap + 16));
                }
                rc = fgfa_dev::gaf_lookup_gather(job, o, o + m, d_out, st);
                if (rc) return rc;
                CAPI_HIP(fgfa_dev::staged_copy(res->text + res->text_len, d_out, m, hipMemcpyDeviceToHost, st));
                res->text_len += m;
                o += m;
            }
        } else if (mode == kGafEvents && L) {
            const uint64_t L0 = res->n_lines, E0 = res->n_events;
            res->line_first.resize(L0 + L + 1);
            res->name_off.resize(L0 + L);
            res->name_len.resize(L0 + L);
            // (line_first[L0] of this chunk is 0 on the device and E0 here: copied from the chunk's second entry on)
            CAPI_HIP(fgfa_dev::staged_copy(&res->line_first[L0 + 1], ar.line_first + 1, L * 8, hipMemcpyDeviceToHost, st));
            CAPI_HIP(fgfa_dev::staged_copy(&res->name_off[L0], ar.line_end, L * 8, hipMemcpyDeviceToHost, st));
            CAPI_HIP(fgfa_dev::staged_copy(&res->name_len[L0], ar.name_len, L * 8, hipMemcpyDeviceToHost, st));
            for (uint64_t l = L; l-- > 0;) {  // a line starts behind the '\n' of the one before
                res->name_off[L0 + l] = b + (l ? res->name_off[L0 + l - 1] + 1 : 0);
                res->line_first[L0 + l + 1] += E0;
            }
            res->handle.resize(E0 + E);
            res->kind.resize(E0 + E);
            res->a.resize(E0 + E);
            res->b.resize(E0 + E);
            if (E) {
                CAPI_HIP(fgfa_dev::staged_copy(&res->handle[E0], ar.handle, E * 4, hipMemcpyDeviceToHost, st));
                CAPI_HIP(fgfa_dev::staged_copy(&res->kind[E0], ar.kind, E, hipMemcpyDeviceToHost, st));
                CAPI_HIP(fgfa_dev::staged_copy(&res->a[E0], ar.a, E * 8, hipMemcpyDeviceToHost, st));
                CAPI_HIP(fgfa_dev::staged_copy(&res->b[E0], ar.b, E * 8, hipMemcpyDeviceToHost, st));
            }
        }
        res->n_lines += L;
        res->n_events += E;
    }
    return FLATGFA_OK;
}

static int gaf_args(const char *what, flatgfa_t gfa, const uint8_t *gaf, size_t len, const void *out) {
    if (!gfa || !out || (len && !gaf)) { set_error(std::string(what) + ": NULL argument"); return FLATGFA_ERR_ARG; }
    return FLATGFA_OK;
}

int flatgfa_gaf_count(flatgfa_t gfa, const uint8_t *gaf, size_t len, uint64_t *events, uint64_t *lines) {
    if (int rc = gaf_args("flatgfa_gaf_count", gfa, gaf, len, events)) return rc;
    GafResult res;
    if (int rc = gaf_lookup_host(gfa, gaf, len, kGafCount, &res)) return rc;
    *events = res.n_events;
    if (lines) *lines = res.n_lines;
    return FLATGFA_OK;
}

int flatgfa_gaf_seqs(flatgfa_t gfa, const uint8_t *gaf, size_t len, char **text, size_t *text_len) {
    if (int rc = gaf_args("flatgfa_gaf_seqs", gfa, gaf, len, text)) return rc;
    *text = nullptr;
    GafResult res;
    if (int rc = gaf_lookup_host(gfa, gaf, len, kGafSeqs, &res)) return rc;
    if (!res.text && !(res.text = (char *)malloc(1))) { set_error("out of memory"); return FLATGFA_ERR_IO; }
    res.text[res.text_len] = 0;
    *text = res.text;
    res.text = nullptr;
    if (text_len) *text_len = (size_t)res.text_len;
    return FLATGFA_OK;
}

int flatgfa_gaf_events(flatgfa_t gfa, const uint8_t *gaf, size_t len, flatgfa_gaf_events_t **out) {
    if (int rc = gaf_args("flatgfa_gaf_events", gfa, gaf, len, out)) return rc;
    *out = nullptr;
    GafResult res;
    if (int rc = gaf_lookup_host(gfa, gaf, len, kGafEvents, &res)) return rc;
    const uint64_t L = res.n_lines, E = res.n_events;
    // one block: the struct, then the u64 arrays, the u32 array, the bytes
    const size_t bytes = sizeof(flatgfa_gaf_events_t) + ((L + 1) + 2 * L + 2 * E) * 8 + E * 4 + E + 8;
    char *blk = (char *)malloc(bytes);
    if (!blk) { set_error("out of memory"); return FLATGFA_ERR_IO; }
    flatgfa_gaf_events_t *ev = reinterpret_cast<flatgfa_gaf_events_t *>(blk);
    uint64_t *w = reinterpret_cast<uint64_t *>(blk + sizeof(flatgfa_gaf_events_t));
    ev->n_lines = L;
    ev->n_events = E;
    ev->line_first = w;
    ev->name_off = w + L + 1;
    ev->name_len = ev->name_off + L;
    ev->a = ev->name_len + L;
    ev->b = ev->a + E;
    ev->handle = reinterpret_cast<uint32_t *>(ev->b + E);
    ev->kind = reinterpret_cast<uint8_t *>(ev->handle + E);
    memcpy(ev->line_first, res.line_first.data(), (L + 1) * 8);
    if (L) {
        memcpy(ev->name_off, res.name_off.data(), L * 8);
        memcpy(ev->name_len, res.name_len.data(), L * 8);
    }
    if (E) {
        memcpy(ev->a, res.a.data(), E * 8);
        memcpy(ev->b, res.b.data(), E * 8);
        memcpy(ev->handle, res.handle.data(), E * 4);
        memcpy(ev->kind, res.kind.data(), E);
    }
    *out = ev;
    return FLATGFA_OK;
}

void flatgfa_gaf_events_free(flatgfa_gaf_events_t *ev) { free(ev); }

int flatgfa_gaf_table(flatgfa_t gfa, const uint8_t *gaf, size_t len, char **text, size_t *text_len) {
    if (int rc = gaf_args("flatgfa_gaf_table", gfa, gaf, len, text)) return rc;
    *text = nullptr;
    flatgfa_gaf_events_t *ev = nullptr;
    if (int rc = flatgfa_gaf_events(gfa, gaf, len, &ev)) return rc;
    // cmds.rs:367-374, gaf.rs:167-197: the name and a newline, then the events with nothing between or behind them
    const fgfa::View &v = gfa->view;
    std::string s;
    for (uint64_t l = 0; l < ev->n_lines; ++l) {
        s.append(reinterpret_cast<const char *>(gaf) + ev->name_off[l], ev->name_len[l]);
        s.push_back('\n');
        for (uint64_t k = ev->line_first[l]; k < ev->line_first[l + 1]; ++k) {
            s += std::to_string(k - ev->line_first[l]);
            if (ev->kind[k] == 0) {
                s += ": (skipped)";
                continue;
            }
            const fgfa::Segment seg = v.segs[ev->handle[k] >> 1];
            s += ": " + std::to_string(seg.name) + ((ev->handle[k] & 1u) ? "-, " : "+, ");
            if (ev->kind[k] == 1) s += std::to_string(seg.seq.len()) + "bp";
            else s += std::to_string(ev->a[k]) + "-" + std::to_string(ev->b[k]) + "bp";
        }
    }
    flatgfa_gaf_events_free(ev);
    char *p = (char *)malloc(s.size() + 1);
    if (!p) { set_error("out of memory"); return FLATGFA_ERR_IO; }
    memcpy(p, s.data(), s.size());
    p[s.size()] = 0;
    *text = p;
    if (text_len) *text_len = s.size();
    return FLATGFA_OK;
}

struct flatgfa_dev_gaf {
    fgfa_dev::GafLookupJob *job = nullptr;
    fgfa_dev::GafTotals totals;
    ~flatgfa_dev_gaf() { fgfa_dev::gaf_lookup_free(job); }
};

int flatgfa_dev_gaf_count(flatgfa_t gfa, const uint8_t *d_text, size_t len, int seqs, void *stream, flatgfa_dev_gaf_t **job,
                          uint64_t *n_lines, uint64_t *n_events, uint64_t *seq_bytes) {
    if (!gfa || !job || !n_lines || !n_events || (len && !d_text)) { set_error("flatgfa_dev_gaf_count: NULL argument"); return FLATGFA_ERR_ARG; }
    std::lock_guard<std::mutex> op(gfa->op_mu);
    int device = 0;
    CAPI_HIP(hipGetDevice(&device));
    fgfa_dev::GafGraph graph;
    int rc = ensure_gaf_graph(gfa, device, &graph);
    if (rc) return rc;
    flatgfa_dev_gaf_t *h = *job ? *job : new flatgfa_dev_gaf();  // (a job given is used again: its scratch stays)
    if (!h->job) h->job = fgfa_dev::gaf_lookup_new();
    rc = fgfa_dev::gaf_lookup_count(h->job, d_text, len, graph, seqs != 0, 0, (hipStream_t)stream, &h->totals);
    if (!rc) rc = gaf_lookup_verdict(h->totals, seqs != 0);
    if (rc) {
        if (!*job) delete h;
        return rc;
    }
    *job = h;
    *n_lines = h->totals.n_lines;
    *n_events = h->totals.n_events;
    if (seq_bytes) *seq_bytes = h->totals.seq_bytes;
    return FLATGFA_OK;
}

int flatgfa_dev_gaf_fill(flatgfa_dev_gaf_t *job, uint64_t *line_first, uint64_t *line_end, uint64_t *name_len, uint32_t *handle,
                         uint8_t *kind, uint64_t *a, uint64_t *b, uint8_t *seq_text, void *stream_) {
    if (!job || !job->job) { set_error("flatgfa_dev_gaf_fill: NULL job"); return FLATGFA_ERR_ARG; }
    hipStream_t stream = (hipStream_t)stream_;
    const fgfa_dev::GafArrays &ar = fgfa_dev::gaf_lookup_arrays(job->job);
    const uint64_t L = job->totals.n_lines, E = job->totals.n_events;
    if (L) {
        if (line_first) CAPI_HIP(hipMemcpyAsync(line_first, ar.line_first, (L + 1) * 8, hipMemcpyDeviceToDevice, stream));
        if (line_end) CAPI_HIP(hipMemcpyAsync(line_end, ar.line_end, L * 8, hipMemcpyDeviceToDevice, stream));
        if (name_len) CAPI_HIP(hipMemcpyAsync(name_len, ar.name_len, L * 8, hipMemcpyDeviceToDevice, stream));
    }
    if (E) {
        if (handle) CAPI_HIP(hipMemcpyAsync(handle, ar.handle, E * 4, hipMemcpyDeviceToDevice, stream));
        if (kind) CAPI_HIP(hipMemcpyAsync(kind, ar.kind, E, hipMemcpyDeviceToDevice, stream));
        if (a) CAPI_HIP(hipMemcpyAsync(a, ar.a, E * 8, hipMemcpyDeviceToDevice, stream));
        if (b) CAPI_HIP(hipMemcpyAsync(b, ar.b, E * 8, hipMemcpyDeviceToDevice, stream));
    }
    int rc = FLATGFA_OK;
    if (seq_text && job->totals.seq_bytes) rc = fgfa_dev::gaf_lookup_gather(job->job, 0, job->totals.seq_bytes, seq_text, stream);
    if (!rc) rc = fgfa_dev::gaf_lookup_used_on(job->job, stream);  // (the next count, or the free, waits for these copies)
    return rc;
}

void flatgfa_dev_gaf_free(flatgfa_dev_gaf_t *job) { delete job; }

// ---- chop (ops/chop.rs) ----

// What chop and inject read of `gfa` on the scope's device: the steps, spans and lengths (the resident image's, when there is
// one), the seq starts, the links when they are wanted; and room for seg_first.
static int upload_chop_input(CStore *gfa, DevScope &sc, bool links, fgfa_dev::ChopIn *in_out, uint32_t **seg_first_out) {
    const fgfa::View &v = gfa->view;
    const size_t N = v.steps.len, P = v.paths.len, S = v.segs.len, L = links ? v.links.len : 0;
    const bool resident = sc.resident;  // (its image is read in place)
    // (an array of no elements stays NULL below, which chop_fill reads as "not wanted": sc.alloc would make it one element long)
    const size_t Pa = (P + 63) & ~(size_t)63, Sa = (S + 63) & ~(size_t)63;
    std::vector<uint32_t> host((resident ? 0 : 2 * Pa + Sa) + Sa + 1);
    uint32_t *h_start = host.data();
    for (size_t i = 0; i < S; ++i) h_start[i] = v.segs[i].seq.start;
    fgfa_dev::ChopIn in;
    in.n_steps = N;
    in.n_paths = (uint32_t)P;
    in.n_segs = (uint32_t)S;
    in.n_links = L;
    uint32_t *d_small = nullptr;
    CAPI_HIP(sc.alloc(&d_small, host.size() + S + 1));
    uint32_t *d_seg_first = d_small + host.size();
    in.seq_start = d_small;
    if (resident) {
        in.steps = gfa->d_steps;
        in.path_begin = gfa->d_path_begin;
        in.path_end = gfa->d_path_end;
        in.seg_len = gfa->d_seg_len;
    } else {
        uint32_t *h_pb = host.data() + Sa, *h_pe = h_pb + Pa, *h_len = h_pe + Pa;
        for (size_t i = 0; i < P; ++i) {
            h_pb[i] = v.paths[i].steps.start;
            h_pe[i] = v.paths[i].steps.end;
        }
        for (size_t i = 0; i < S; ++i) h_len[i] = v.segs[i].seq.len();
        in.path_begin = d_small + Sa;
        in.path_end = in.path_begin + Pa;
        in.seg_len = in.path_end + Pa;
        uint32_t *d_steps = nullptr;
        if (N) CAPI_HIP(sc.upload(&d_steps, v.steps.data, N));
        in.steps = d_steps;
    }
    CAPI_HIP(fgfa_dev::staged_copy(d_small, host.data(), host.size() * 4, hipMemcpyHostToDevice, nullptr));
    if (L) {
        uint32_t *d_links = nullptr;
        CAPI_HIP(sc.alloc(&d_links, L * 4));
        CAPI_HIP(fgfa_dev::staged_copy(d_links, v.links.data, L * 16, hipMemcpyHostToDevice, nullptr));
        in.links = d_links;
    }
    *in_out = in;
    *seg_first_out = d_seg_first;
    return FLATGFA_OK;
}

// the pools that chop and inject number in u32 (`links`: whether the links are read at all)
static bool chop_input_too_large(const fgfa::View &v, bool links) {
    return v.steps.len > 0xFFFFFFFFull || v.segs.len > 0x80000000ull || v.paths.len > 0xFFFFFFFFull || (links && v.links.len > 0xFFFFFFFFull);
}

// What chop and inject do once the count has the sizes (S2 segments, N2 steps, L2 links, P2 >= P paths): the image is
// allocated on the device, filled (the feature's fill on the scope's stream) and downloaded into a new CStore: the header,
// seq_data and name_data (with room for name_bytes) copied, the old P path records made from the new spans.  *spans_out holds
// the P2 spans, begins in its first half and ends in its second, for the paths the caller adds behind the old ones.
static int download_expanded(CStore *gfa, DevScope &sc, const std::function<int(const fgfa_dev::ChopOut &)> &fill, size_t P2, uint64_t S2, uint64_t N2,
                             uint64_t L2, size_t name_bytes, std::unique_ptr<CStore> *cs_out, std::vector<uint32_t> *spans_out) {
    const fgfa::View &v = gfa->view;
    const size_t P = v.paths.len, Pa = (P2 + 63) & ~(size_t)63;
    hipStream_t st = sc.stream;
    // the outputs, now that their sizes are known to fit
    fgfa_dev::ChopOut o;
    if (N2) CAPI_HIP(sc.alloc(&o.steps, N2));
    if (Pa) CAPI_HIP(sc.alloc(&o.path_begin, 2 * Pa));
    o.path_end = o.path_begin ? o.path_begin + Pa : nullptr;
    if (S2) CAPI_HIP(sc.alloc(&o.seg_recs, S2 * 6));
    if (L2) CAPI_HIP(sc.alloc(&o.links, L2 * 4));
    if (int rc = fill(o)) return rc;
    auto cs = std::make_unique<CStore>();
    fgfa::Store &h = cs->heap;
    // (the host pools are allocated beside the kernels; the largest, the steps, on a thread of its own)
    std::thread alloc([&] { h.steps.resize(N2); });
    Joiner joiner{alloc};
    h.header.assign(v.header.begin(), v.header.end());
    h.seq_data.assign(v.seq_data.begin(), v.seq_data.end());
    h.name_data.reserve(name_bytes);
    h.name_data.assign(v.name_data.begin(), v.name_data.end());
    h.segs.resize(S2);
    h.links.resize(L2);
    std::vector<uint32_t> &spans = *spans_out;
    spans.resize(2 * Pa);
    CAPI_HIP(fgfa_dev::staged_copy(h.segs.data(), o.seg_recs, S2 * 24, hipMemcpyDeviceToHost, st));
    CAPI_HIP(fgfa_dev::staged_copy(h.links.data(), o.links, L2 * 16, hipMemcpyDeviceToHost, st));
    CAPI_HIP(fgfa_dev::staged_copy(spans.data(), o.path_begin, 2 * Pa * 4, hipMemcpyDeviceToHost, st));
    alloc.join();
    CAPI_HIP(fgfa_dev::staged_copy(h.steps.data(), o.steps, N2 * 4, hipMemcpyDeviceToHost, st));
    h.paths.resize(P2);
    for (size_t i = 0; i < P; ++i) h.paths[i] = fgfa::Path{v.paths[i].name, fgfa::Span{spans[i], spans[Pa + i]}, fgfa::Span{0, 0}};  // chop.rs:104, chop.py:56
    *cs_out = std::move(cs);
    return FLATGFA_OK;
}

int flatgfa_chop(flatgfa_t gfa, uint64_t max_size, int links, flatgfa_t *out) {
    if (out) *out = nullptr;
    if (!gfa || !out) { set_error("flatgfa_chop: NULL argument"); return FLATGFA_ERR_ARG; }
    if (max_size == 0) { set_error("flatgfa_chop: the maximum segment size must be at least 1"); return FLATGFA_ERR_ARG; }
    std::lock_guard<std::mutex> op(gfa->op_mu);
    const fgfa::View &v = gfa->view;
    if (chop_input_too_large(v, links != 0)) { set_error("flatgfa_chop: graph too large for 32-bit ids"); return FLATGFA_ERR_TOO_LARGE; }
    DevScope sc;
    if (int rc = open_scope(gfa, &sc, "chop")) return rc;
    fgfa_dev::ChopIn in;
    uint32_t *d_seg_first = nullptr;
    if (int rc = upload_chop_input(gfa, sc, links != 0, &in, &d_seg_first)) return rc;
    fgfa_dev::ChopJob *job = sc.hold<fgfa_dev::ChopJob, fgfa_dev::chop_free>(fgfa_dev::chop_new());
    uint64_t S2 = 0, N2 = 0, L2 = 0;
    if (int rc = fgfa_dev::chop_count(job, in, max_size, links != 0, d_seg_first, sc.stream, &S2, &N2, &L2)) return rc;
    std::unique_ptr<CStore> cs;
    std::vector<uint32_t> spans;
    const auto fill = [&](const fgfa_dev::ChopOut &o) { return fgfa_dev::chop_fill(job, o, sc.stream); };
    if (int rc = download_expanded(gfa, sc, fill, v.paths.len, S2, N2, L2, v.name_data.len, &cs, &spans)) return rc;
    cs->view = cs->heap.view();
    *out = cs.release();
    return FLATGFA_OK;
}

// ---- inject (slow_odgi/inject.py) ----

namespace {
// The three cases a batch refuses (the reference updates its path dictionary in place, line by line): new name l equals a path
// name of the graph, or an earlier line's new name.  `by_name` holds the graph's path names; line_no[l] is what line l is called
// in the message (the line of the BED text, counted from 1), l + 1 when there is none.
int inject_check_names(const std::unordered_map<std::string, uint32_t> &by_name, const char *const *names, const size_t *name_lens, uint64_t n,
                       const size_t *line_no) {
    std::unordered_set<std::string> fresh;
    for (uint64_t l = 0; l < n; ++l) {
        std::string nm(names[l] ? names[l] : "", name_lens[l]);
        const std::string where = "inject: line " + std::to_string(line_no ? line_no[l] : l + 1);
        if (by_name.count(nm)) {
            set_error(where + ": the new name '" + nm + "' is a path of the graph already");
            return FLATGFA_ERR_ARG;
        }
        if (!fresh.insert(std::move(nm)).second) {
            set_error(where + ": the new name was given by an earlier line");
            return FLATGFA_ERR_ARG;
        }
    }
    return FLATGFA_OK;
}

void path_names(const fgfa::View &v, std::unordered_map<std::string, uint32_t> *out) {
    std::unordered_map<std::string, uint32_t> &m = *out;
    m.reserve(v.paths.len);
    for (size_t i = 0; i < v.paths.len; ++i) {  // (the first path of a name, as View::find_path)
        const fgfa::Span s = v.paths[i].name;
        m.emplace(std::string((const char *)v.name_data.data + s.start, s.len()), (uint32_t)i);
    }
}

// chop's route with the lines beside the graph; the names were checked
int inject_locked(CStore *gfa, const uint32_t *path_ids, const uint64_t *starts, const uint64_t *ends, const char *const *names,
                  const size_t *name_lens, uint64_t n, int links, flatgfa_t *out) {
    const fgfa::View &v = gfa->view;
    const size_t P = v.paths.len;
    size_t name_bytes = v.name_data.len;
    for (uint64_t l = 0; l < n; ++l) name_bytes += name_lens[l];
    if (chop_input_too_large(v, links != 0) || P + n > 0xFFFFFFFFull || n >= 0x7FFFFFFFull || name_bytes > 0xFFFFFFFFull) {
        set_error("flatgfa_inject: graph too large for 32-bit ids");
        return FLATGFA_ERR_TOO_LARGE;
    }
    DevScope sc;
    if (int rc = open_scope(gfa, &sc, "inject")) return rc;
    fgfa_dev::ChopIn in;
    uint32_t *d_seg_first = nullptr;
    if (int rc = upload_chop_input(gfa, sc, links != 0, &in, &d_seg_first)) return rc;
    fgfa_dev::InjectLines ln;
    ln.n = n;
    if (n) {
        uint32_t *d_ids = nullptr;
        uint64_t *d_lo = nullptr, *d_hi = nullptr;
        CAPI_HIP(sc.upload(&d_ids, path_ids, n));
        CAPI_HIP(sc.upload(&d_lo, starts, n));
        CAPI_HIP(sc.upload(&d_hi, ends, n));
        ln.path_id = d_ids;
        ln.start = d_lo;
        ln.end = d_hi;
    }
    fgfa_dev::InjectJob *job = sc.hold<fgfa_dev::InjectJob, fgfa_dev::inject_free>(fgfa_dev::inject_new());
    uint64_t S2 = 0, N2 = 0, L2 = 0;
    if (int rc = fgfa_dev::inject_count(job, in, ln, links != 0, d_seg_first, sc.stream, &S2, &N2, &L2)) return rc;
    std::unique_ptr<CStore> cs;
    std::vector<uint32_t> spans;
    const auto fill = [&](const fgfa_dev::ChopOut &o) { return fgfa_dev::inject_fill(job, o, sc.stream); };
    if (int rc = download_expanded(gfa, sc, fill, P + n, S2, N2, L2, name_bytes, &cs, &spans)) return rc;
    fgfa::Store &h = cs->heap;
    const size_t Pa = spans.size() / 2;
    for (size_t l = 0; l < n; ++l) {  // inject.py:91-92
        const uint32_t at = (uint32_t)h.name_data.size();
        h.name_data.insert(h.name_data.end(), (const uint8_t *)names[l], (const uint8_t *)names[l] + name_lens[l]);
        h.paths[P + l] = fgfa::Path{fgfa::Span{at, (uint32_t)h.name_data.size()}, fgfa::Span{spans[P + l], spans[Pa + P + l]}, fgfa::Span{0, 0}};
    }
    cs->view = h.view();
    *out = cs.release();
    return FLATGFA_OK;
}
}  // namespace

int flatgfa_inject(flatgfa_t gfa, const uint32_t *path_ids, const uint64_t *starts, const uint64_t *ends, const char *const *names,
                   const size_t *name_lens, uint64_t n, int links, flatgfa_t *out) {
    if (out) *out = nullptr;
    if (!gfa || !out || (n && (!path_ids || !starts || !ends || !names || !name_lens))) { set_error("flatgfa_inject: NULL argument"); return FLATGFA_ERR_ARG; }
    for (uint64_t l = 0; l < n; ++l) {
        if (!names[l] && name_lens[l]) { set_error("flatgfa_inject: NULL argument"); return FLATGFA_ERR_ARG; }
        if (!name_lens[l]) { set_error("inject: line " + std::to_string(l + 1) + ": the new name is empty"); return FLATGFA_ERR_ARG; }
    }
    std::lock_guard<std::mutex> op(gfa->op_mu);
    std::unordered_map<std::string, uint32_t> by_name;
    path_names(gfa->view, &by_name);
    if (int rc = inject_check_names(by_name, names, name_lens, n, nullptr)) return rc;
    return inject_locked(gfa, path_ids, starts, ends, names, name_lens, n, links, out);
}

int flatgfa_inject_bed(flatgfa_t gfa, const char *bed, size_t bed_len, int links, flatgfa_t *out) {
    if (out) *out = nullptr;
    if (!gfa || !out || (bed_len && !bed)) { set_error("flatgfa_inject_bed: NULL argument"); return FLATGFA_ERR_ARG; }
    std::vector<fgfa::InjectBedLine> lines;
    std::string err;
    if (!fgfa::parse_inject_bed((const uint8_t *)bed, bed_len, &lines, &err)) { set_error(err); return FLATGFA_ERR_ARG; }
    std::lock_guard<std::mutex> op(gfa->op_mu);
    std::unordered_map<std::string, uint32_t> by_name;
    path_names(gfa->view, &by_name);
    // inject.py:87: a line whose path the graph does not have is skipped -- unless an earlier line made a path of that name
    std::vector<uint32_t> ids;
    std::vector<uint64_t> lo, hi;
    std::vector<const char *> names;
    std::vector<size_t> name_lens, line_no;
    std::unordered_set<std::string> fresh;
    for (size_t l = 0; l < lines.size(); ++l) {
        const fgfa::InjectBedLine &b = lines[l];
        const std::string path(bed + b.path_off, b.path_len);
        const auto it = by_name.find(path);
        if (it == by_name.end()) {
            if (fresh.count(path)) {
                set_error("inject: line " + std::to_string(b.line) + " names the path '" + path + "' that an earlier line injects");
                return FLATGFA_ERR_ARG;
            }
            continue;
        }
        fresh.emplace(bed + b.name_off, b.name_len);
        ids.push_back(it->second);
        lo.push_back(b.start);
        hi.push_back(b.end);
        names.push_back(bed + b.name_off);
        name_lens.push_back(b.name_len);
        line_no.push_back(b.line);
    }
    if (int rc = inject_check_names(by_name, names.data(), name_lens.data(), ids.size(), line_no.data())) return rc;
    return inject_locked(gfa, ids.data(), lo.data(), hi.data(), names.data(), name_lens.data(), ids.size(), links, out);
}

// ---- crush (slow_odgi/crush.py) ----

int flatgfa_crush(flatgfa_t gfa, flatgfa_t *out) {
    if (out) *out = nullptr;
    if (!gfa || !out) { set_error("flatgfa_crush: NULL argument"); return FLATGFA_ERR_ARG; }
    std::lock_guard<std::mutex> op(gfa->op_mu);
    const fgfa::View &v = gfa->view;
    const size_t S = v.segs.len, n_seq = v.seq_data.len;
    if (S > 0x80000000ull) { set_error("flatgfa_crush: graph too large for 32-bit ids"); return FLATGFA_ERR_TOO_LARGE; }
    // (before any device work: the kernels check the spans again, as the device-level entry needs them to)
    std::vector<uint32_t> seg_seq(2 * S);
    for (size_t i = 0; i < S; ++i) {
        const fgfa::Span sp = v.segs[i].seq;
        if (sp.start > sp.end || sp.end > n_seq) {
            set_error("crush: segment " + std::to_string(i) + " has a sequence span outside seq_data");
            return FLATGFA_ERR_BOUNDS;
        }
        seg_seq[2 * i] = sp.start;
        seg_seq[2 * i + 1] = sp.end - sp.start;
    }
    DevScope sc;
    if (int rc = open_scope(gfa, &sc, "crush")) return rc;
    hipStream_t st = sc.stream;
    fgfa_dev::CrushIn in;
    in.seq_len = n_seq;
    in.n_segs = (uint32_t)S;
    if (gfa->gaf_seq_device == sc.device) {  // the pool the handle keeps on this device, read in place
        in.seg_seq = gfa->d_gaf_seg_seq;
        in.seq_data = gfa->d_gaf_seq_data;
    } else {
        uint32_t *d_seg_seq = nullptr;
        uint8_t *d_seq = nullptr;
        CAPI_HIP(sc.upload(&d_seg_seq, seg_seq.data(), 2 * S));
        CAPI_HIP(sc.upload(&d_seq, v.seq_data.data, n_seq));
        in.seg_seq = d_seg_seq;
        in.seq_data = d_seq;
    }
    uint32_t *d_out = nullptr;  // the new lengths, then the new spans
    CAPI_HIP(sc.alloc(&d_out, 3 * S));
    fgfa_dev::CrushJob *job = sc.hold<fgfa_dev::CrushJob, fgfa_dev::crush_free>(fgfa_dev::crush_new());
    uint64_t kept = 0, dropped = 0;
    if (int rc = fgfa_dev::crush_count(job, in, d_out, st, &kept, &dropped)) return rc;
    // the new pool, now that its size is known to fit
    uint8_t *d_seq_out = nullptr;
    CAPI_HIP(sc.alloc(&d_seq_out, kept));
    if (int rc = fgfa_dev::crush_fill(job, d_seq_out, d_out + S, st)) return rc;
    auto cs = std::make_unique<CStore>();
    fgfa::Store &h = cs->heap;
    // (the host pools are made beside the kernels)
    h.header.assign(v.header.begin(), v.header.end());
    h.name_data.assign(v.name_data.begin(), v.name_data.end());
    h.steps.assign(v.steps.begin(), v.steps.end());
    h.links.assign(v.links.begin(), v.links.end());
    h.alignment.resize(v.alignment.len);
    if (v.alignment.len) memcpy(h.alignment.data(), v.alignment.data, v.alignment.len * 4);
    h.seq_data.resize(kept);
    std::vector<uint32_t> spans(2 * S);
    CAPI_HIP(fgfa_dev::staged_copy(spans.data(), d_out + S, 2 * S * 4, hipMemcpyDeviceToHost, st));
    CAPI_HIP(fgfa_dev::staged_copy(h.seq_data.data(), d_seq_out, kept, hipMemcpyDeviceToHost, st));
    h.segs.resize(S);
    for (size_t i = 0; i < S; ++i) h.segs[i] = fgfa::Segment{v.segs[i].name, fgfa::Span{spans[2 * i], spans[2 * i] + spans[2 * i + 1]}, fgfa::Span{0, 0}};
    h.paths.resize(v.paths.len);
    for (size_t i = 0; i < v.paths.len; ++i) h.paths[i] = fgfa::Path{v.paths[i].name, v.paths[i].steps, fgfa::Span{0, 0}};  // crush.py:27
    cs->view = h.view();
    *out = cs.release();
    return FLATGFA_OK;
}

// ---- flip (slow_odgi/flip.py) ----

extern "C++" {
namespace {
// How many keys of the link table a round takes: kFlipRoundKeys, or what the tests ask for.
uint64_t flip_round_keys() {
    if (const char *h = test_hook("FLATGFA_FLIP_ROUND_KEYS")) return std::max<uint64_t>(1, strtoull(h, nullptr, 10));
    return fgfa_dev::kFlipRoundKeys;
}

// The count (always) and the new store (where cs_out is given): the pools are checked and the paths laid out on the host
// (flip_host.hpp), steps, spans, lengths, links and alignment go up -- the steps and lengths of a resident graph are read in
// place -- and the device does the rest (flip_device.hip); the names are made on the host from the turned flags.
int flip_locked(CStore *gfa, uint64_t *n_turned_out, uint64_t *n_links_out, std::unique_ptr<CStore> *cs_out) {
    const fgfa::View &v = gfa->view;
    fgfa_flip::Lay lay;
    std::string why;
    switch (fgfa_flip::check_and_lay(v, &lay, &why)) {
        case fgfa_flip::Verdict::kBounds: set_error("flip: " + why); return FLATGFA_ERR_BOUNDS;
        case fgfa_flip::Verdict::kTooLarge: set_error("flip: " + why); return FLATGFA_ERR_TOO_LARGE;
        case fgfa_flip::Verdict::kOk: break;
    }
    const size_t P = v.paths.len, N = v.steps.len, S = v.segs.len, L = v.links.len, A = v.alignment.len;
    DevScope sc;
    if (int rc = open_scope(gfa, &sc, "flip")) return rc;
    hipStream_t st = sc.stream;
    fgfa_dev::FlipIn in;
    uint32_t *d_pstart = nullptr, *d_pbegin = nullptr, *d_steps = nullptr, *d_seg_len = nullptr, *d_links = nullptr, *d_align = nullptr;
    CAPI_HIP(sc.upload(&d_pstart, lay.pstart.data(), P + 1));
    CAPI_HIP(sc.upload(&d_pbegin, lay.pbegin.data(), P + 1));
    if (sc.resident) {  // (read in place)
        d_steps = gfa->d_steps;
        d_seg_len = gfa->d_seg_len;
    } else {
        std::vector<uint32_t> seg_len(S);
        for (size_t s = 0; s < S; ++s) seg_len[s] = v.segs[s].seq.len();
        CAPI_HIP(sc.upload(&d_steps, v.steps.data, N));
        CAPI_HIP(sc.upload(&d_seg_len, seg_len.data(), S));
    }
    CAPI_HIP(sc.alloc(&d_links, L * 4));
    if (L) CAPI_HIP(fgfa_dev::staged_copy(d_links, v.links.data, L * 16, hipMemcpyHostToDevice, st));
    CAPI_HIP(sc.alloc(&d_align, A));
    if (A) CAPI_HIP(fgfa_dev::staged_copy(d_align, v.alignment.data, A * 4, hipMemcpyHostToDevice, st));
    in.steps = d_steps, in.n_steps = N;
    in.pstart = d_pstart, in.pbegin = d_pbegin, in.n_paths = (uint32_t)P, in.n_lin = lay.n_lin;
    in.seg_len = d_seg_len, in.n_segs = (uint32_t)S;
    in.links = d_links, in.n_links = L;
    in.alignment = d_align, in.n_align = A;
    fgfa_dev::FlipJob *job = sc.hold<fgfa_dev::FlipJob, fgfa_dev::flip_free>(fgfa_dev::flip_new(flip_round_keys()));
    uint64_t n_turned = 0, links_out = 0, links_new = 0;
    if (int rc = fgfa_dev::flip_count(job, in, st, &n_turned, &links_out, &links_new)) return rc;
    if (n_turned_out) *n_turned_out = n_turned;
    if (n_links_out) *n_links_out = links_out;
    if (!cs_out) return FLATGFA_OK;
    // the names are the host's: their size is known, and checked, before any output is allocated
    std::vector<uint32_t> turned(P + 1, 0);
    if (P) CAPI_HIP(fgfa_dev::staged_copy(turned.data(), fgfa_dev::flip_turned(job), P * 4, hipMemcpyDeviceToHost, st));
    if (fgfa_flip::names_bytes(v, turned.data()) > 0xFFFFFFFFull) {
        set_error("flip: the names of the turned paths would take name_data past 2^32 - 1 bytes");
        return FLATGFA_ERR_TOO_LARGE;
    }
    uint32_t *d_steps_out = nullptr, *d_turned_out = nullptr, *d_links_out = nullptr;
    CAPI_HIP(sc.alloc(&d_steps_out, (size_t)lay.n_lin));
    CAPI_HIP(sc.alloc(&d_turned_out, P));
    CAPI_HIP(sc.alloc(&d_links_out, (size_t)links_out * 4));
    if (int rc = fgfa_dev::flip_fill(job, d_steps_out, d_turned_out, d_links_out, st)) return rc;
    // (the host pools are made beside the kernels)
    std::vector<fgfa::Handle> steps((size_t)lay.n_lin);
    std::vector<fgfa::Link> links((size_t)links_out);
    CAPI_HIP(fgfa_dev::staged_copy(steps.data(), d_steps_out, (size_t)lay.n_lin * 4, hipMemcpyDeviceToHost, st));
    CAPI_HIP(fgfa_dev::staged_copy(links.data(), d_links_out, (size_t)links_out * 16, hipMemcpyDeviceToHost, st));
    auto cs = std::make_unique<CStore>();
    fgfa_flip::assemble(v, lay, turned.data(), std::move(steps), std::move(links), links_new != 0, &cs->heap);
    cs->view = cs->heap.view();
    *cs_out = std::move(cs);
    return FLATGFA_OK;
}
}  // namespace
}  // extern "C++"

int flatgfa_flip(flatgfa_t gfa, flatgfa_t *out) {
    if (out) *out = nullptr;
    if (!gfa || !out) { set_error("flatgfa_flip: NULL argument"); return FLATGFA_ERR_ARG; }
    std::lock_guard<std::mutex> op(gfa->op_mu);
    std::unique_ptr<CStore> cs;
    if (int rc = flip_locked(gfa, nullptr, nullptr, &cs)) return rc;
    *out = cs.release();
    return FLATGFA_OK;
}

int flatgfa_flip_count(flatgfa_t gfa, uint64_t *n_turned, uint64_t *n_links_out) {
    if (n_turned) *n_turned = 0;
    if (n_links_out) *n_links_out = 0;
    if (!gfa) { set_error("flatgfa_flip_count: NULL argument"); return FLATGFA_ERR_ARG; }
    std::lock_guard<std::mutex> op(gfa->op_mu);
    return flip_locked(gfa, n_turned, n_links_out, nullptr);
}

// ---- the packed-sequence codec (packedseq.rs, cli/cmds.rs:415-452) ----

extern "C++" {
namespace {
// The size text and packed bytes are cut to for the device: 64 MiB, or what the tests ask for.
size_t seq_chunk_bytes() {
    if (const char *h = test_hook("FLATGFA_SEQ_CHUNK_BYTES")) return std::max<size_t>(1, strtoull(h, nullptr, 10));
    return (size_t)64 << 20;
}

struct FreeBytes {
    void operator()(void *p) const { free(p); }
};
struct FreePackJob {
    void operator()(fgfa_dev::SeqPackJob *j) const { fgfa_dev::seq_pack_free(j); }
};

// The file image of `text` into a malloc'd buffer.  The text travels a chunk at a time, cut anywhere: a chunk that ends on a
// low nibble (its bases and the carry in front of them are an odd number) and is not the last keeps its final byte back, and
// that byte's low nibble is the carry in front of the next chunk.  The packed bytes land where they stay.
int seq_export_image(const uint8_t *text, size_t n, uint8_t **image, size_t *image_len) {
    DevScope sc;
    if (int rc = open_scope(nullptr, &sc, "seq-export")) return rc;
    hipStream_t st = sc.stream;
    const size_t chunk = seq_chunk_bytes(), room = std::min(n, chunk);
    uint8_t *d_text = nullptr, *d_out = nullptr;
    CAPI_HIP(sc.alloc(&d_text, room));
    CAPI_HIP(sc.alloc(&d_out, room / 2 + 2));
    std::unique_ptr<uint8_t, FreeBytes> buf((uint8_t *)malloc(fgfa::kPackedSeqHeader + n / 2 + 2));
    if (!buf) { set_error("seq-export: out of memory"); return FLATGFA_ERR_IO; }
    size_t at = fgfa::kPackedSeqHeader;
    uint64_t bases = 0;
    int carry = fgfa_dev::kSeqNoCarry;
    for (size_t a = 0; a < n;) {
        const size_t m = std::min(chunk, n - a);
        const bool last = a + m == n;
        CAPI_HIP(fgfa_dev::staged_copy(d_text, text + a, m, hipMemcpyHostToDevice, st));
        std::unique_ptr<fgfa_dev::SeqPackJob, FreePackJob> job(fgfa_dev::seq_pack_new());
        uint64_t kept = 0;
        if (int rc = fgfa_dev::seq_pack_count(job.get(), d_text, m, a, st, &kept)) return rc;
        if (int rc = fgfa_dev::seq_pack_fill(job.get(), carry, d_out, st)) return rc;
        const uint64_t logical = kept + (carry >= 0 ? 1 : 0), bytes = fgfa_dev::seq_packed_bytes(logical);
        if (bytes) CAPI_HIP(fgfa_dev::staged_copy(buf.get() + at, d_out, bytes, hipMemcpyDeviceToHost, st));
        if (!last && (logical & 1)) {
            carry = buf.get()[at + bytes - 1] & 0xF;
            at += bytes - 1;
        } else {
            carry = fgfa_dev::kSeqNoCarry;
            at += bytes;
        }
        bases += kept;
        a += m;
    }
    if (at != fgfa::kPackedSeqHeader + fgfa_dev::seq_packed_bytes(bases)) {
        set_error("seq-export: internal: the packed bytes are not as many as the bases counted");
        return FLATGFA_ERR_HIP;
    }
    fgfa::packed_seq_header(bases, buf.get());
    *image = buf.release();
    *image_len = at;
    return FLATGFA_OK;
}

// The bases of a packed file in device memory (*d_text, the scope's): the header is checked before any device work, the data
// travel a chunk at a time, cut on even base indices, and every nibble is checked before a base is delivered.
int seq_import_device(const uint8_t *file, size_t n, DevScope *sc, uint8_t **d_text, uint64_t *n_bases) {
    size_t off = 0;
    std::string err;
    if (!fgfa::parse_packed_seq(file, n, n_bases, &off, &err)) { set_error(err); return FLATGFA_ERR_PARSE; }
    if (int rc = open_scope(nullptr, sc, "seq-import")) return rc;
    const uint64_t n_bytes = fgfa_dev::seq_packed_bytes(*n_bases);
    const size_t chunk = seq_chunk_bytes();
    uint8_t *d_packed = nullptr;
    CAPI_HIP(sc->alloc(&d_packed, std::min<uint64_t>(n_bytes, chunk)));
    CAPI_HIP(sc->alloc(d_text, *n_bases));
    for (uint64_t a = 0; a < n_bytes;) {
        const uint64_t m = std::min<uint64_t>(chunk, n_bytes - a), here = std::min<uint64_t>(2 * m, *n_bases - 2 * a);
        CAPI_HIP(fgfa_dev::staged_copy(d_packed, file + off + a, m, hipMemcpyHostToDevice, sc->stream));
        if (int rc = fgfa_dev::seq_unpack(d_packed, here, 2 * a, *d_text + 2 * a, sc->stream)) return rc;
        a += m;
    }
    return FLATGFA_OK;
}
}  // namespace
}  // extern "C++"

int flatgfa_seq_packed_info(const uint8_t *file, size_t n, uint64_t *n_bases, uint64_t *data_offset) {
    if ((!file && n) || !n_bases || !data_offset) { set_error("flatgfa_seq_packed_info: NULL argument"); return FLATGFA_ERR_ARG; }
    size_t off = 0;
    std::string err;
    if (!fgfa::parse_packed_seq(file ? file : (const uint8_t *)"", n, n_bases, &off, &err)) { set_error(err); return FLATGFA_ERR_PARSE; }
    *data_offset = off;
    return FLATGFA_OK;
}

int flatgfa_seq_export(const uint8_t *text, size_t n, uint8_t **file_image, size_t *file_len) {
    if (file_image) *file_image = nullptr;
    if (file_len) *file_len = 0;
    if ((!text && n) || !file_image || !file_len) { set_error("flatgfa_seq_export: NULL argument"); return FLATGFA_ERR_ARG; }
    return seq_export_image(text, n, file_image, file_len);
}

int flatgfa_seq_export_file(const uint8_t *text, size_t n, const char *filename) {
    if ((!text && n) || !filename) { set_error("flatgfa_seq_export_file: NULL argument"); return FLATGFA_ERR_ARG; }
    uint8_t *image = nullptr;
    size_t len = 0;
    if (int rc = seq_export_image(text, n, &image, &len)) return rc;  // (no file then)
    std::unique_ptr<uint8_t, FreeBytes> hold(image);
    FILE *f = fopen(filename, "wb");
    if (!f || fwrite(image, 1, len, f) != len || fclose(f)) {
        set_error(std::string("seq-export: cannot write ") + filename);
        return FLATGFA_ERR_IO;
    }
    return FLATGFA_OK;
}

int flatgfa_seq_import(const uint8_t *file, size_t n, char **text, size_t *text_len) {
    if (text) *text = nullptr;
    if (text_len) *text_len = 0;
    if ((!file && n) || !text || !text_len) { set_error("flatgfa_seq_import: NULL argument"); return FLATGFA_ERR_ARG; }
    DevScope sc;
    uint8_t *d_text = nullptr;
    uint64_t bases = 0;
    if (int rc = seq_import_device(file ? file : (const uint8_t *)"", n, &sc, &d_text, &bases)) return rc;
    std::unique_ptr<char, FreeBytes> buf((char *)malloc(bases + 1));
    if (!buf) { set_error("seq-import: out of memory"); return FLATGFA_ERR_IO; }
    if (bases) CAPI_HIP(fgfa_dev::staged_copy(buf.get(), d_text, bases, hipMemcpyDeviceToHost, sc.stream));
    buf.get()[bases] = 0;
    *text = buf.release();
    *text_len = bases;
    return FLATGFA_OK;
}

int flatgfa_seq_import_stream(const uint8_t *file, size_t n, flatgfa_sink_t sink, void *ctx) {
    if ((!file && n) || !sink) { set_error("flatgfa_seq_import_stream: NULL argument"); return FLATGFA_ERR_ARG; }
    DevScope sc;
    uint8_t *d_text = nullptr;
    uint64_t bases = 0;
    if (int rc = seq_import_device(file ? file : (const uint8_t *)"", n, &sc, &d_text, &bases)) return rc;
    std::vector<char> piece(std::min<uint64_t>(bases, std::min<size_t>(seq_chunk_bytes(), (size_t)64 << 20)));
    for (uint64_t a = 0; a < bases; a += piece.size()) {
        const size_t m = std::min<uint64_t>(piece.size(), bases - a);
        CAPI_HIP(fgfa_dev::staged_copy(piece.data(), d_text + a, m, hipMemcpyDeviceToHost, sc.stream));
        if (sink(ctx, piece.data(), m)) { set_error("seq-import: the sink stopped the stream"); return FLATGFA_ERR_IO; }
    }
    return FLATGFA_OK;
}

// ---- extract (ops/extract.rs) and position (ops/position.rs) ----

int64_t flatgfa_find_seg(flatgfa_t gfa, uint64_t name) {
    if (!gfa) { set_error("flatgfa_find_seg: NULL handle"); return -1; }
    const fgfa::View &v = gfa->view;
    for (size_t i = 0; i < v.segs.len; ++i)  // flatgfa.rs:380-384: the first one
        if (v.segs[i].name == name) return (int64_t)i;
    return -1;
}

int flatgfa_extract(flatgfa_t gfa, uint32_t origin_seg, uint64_t link_distance, uint64_t max_distance_subpaths, uint64_t num_iterations,
                    flatgfa_t *out) {
    if (out) *out = nullptr;
    if (!gfa || !out) { set_error("flatgfa_extract: NULL argument"); return FLATGFA_ERR_ARG; }
    std::lock_guard<std::mutex> op(gfa->op_mu);
    const fgfa::View &v = gfa->view;
    const size_t N = v.steps.len, P = v.paths.len, S = v.segs.len, L = v.links.len, A = v.alignment.len;
    if (N > 0xFFFFFFFFull || S > 0x80000000ull || P > 0xFFFFFFFEull || L > 0xFFFFFFFFull || A > 0xFFFFFFFFull) {
        set_error("flatgfa_extract: graph too large for 32-bit ids");
        return FLATGFA_ERR_TOO_LARGE;
    }
    if (origin_seg >= S) { set_error("flatgfa_extract: the origin segment is out of range"); return FLATGFA_ERR_BOUNDS; }
    // the paths' steps one behind another: as they lie in the pool when the spans tile it in path order (what the parser makes)
    std::vector<uint32_t> pstart(P + 1, 0), pbegin(P);
    bool tiling = true;
    uint64_t n_lin = 0;
    for (size_t p = 0; p < P; ++p) {
        const fgfa::Span sp = v.paths[p].steps;
        if (sp.start > sp.end || sp.end > N) { set_error("flatgfa_extract: a path has a step span outside the steps pool"); return FLATGFA_ERR_BOUNDS; }
        tiling = tiling && sp.start == n_lin;
        pbegin[p] = sp.start;
        n_lin += sp.len();
        if (n_lin > 0xFFFFFFFFull) { set_error("flatgfa_extract: the paths hold more than 2^32 - 1 steps"); return FLATGFA_ERR_TOO_LARGE; }
        pstart[p + 1] = (uint32_t)n_lin;
    }
    for (size_t i = 0; i < S; ++i) {
        const fgfa::Span o = v.segs[i].optional;
        if (o.start > o.end || o.end > v.optional_data.len) {
            set_error("flatgfa_extract: segment " + std::to_string(i) + " has an optional-data span outside optional_data");
            return FLATGFA_ERR_BOUNDS;
        }
    }
    DevScope sc;
    if (int rc = open_scope(gfa, &sc, "extract")) return rc;
    hipStream_t st = sc.stream;
    if (int rc = ensure_gaf_seqs(gfa, sc.device)) return rc;  // (lengths and sequences, kept with the handle)

    fgfa_dev::ExtractGraph g;
    g.n_steps = n_lin;
    g.n_paths = (uint32_t)P;
    g.n_segs = (uint32_t)S;
    g.seg_seq = gfa->d_gaf_seg_seq;
    g.n_links = L;
    g.n_align = A;
    uint32_t *d_pstart = nullptr, *d_links = nullptr, *d_steps = nullptr;
    CAPI_HIP(sc.upload(&d_pstart, pstart.data(), P + 1));
    CAPI_HIP(sc.upload(&d_links, v.links.data, L * 4));
    g.pstart = d_pstart;
    g.links = d_links;
    if (sc.resident) d_steps = gfa->d_steps;  // (used in place)
    else CAPI_HIP(sc.upload(&d_steps, v.steps.data, N));
    if (!tiling) {
        uint32_t *d_pb = nullptr, *d_lin = nullptr;
        CAPI_HIP(sc.upload(&d_pb, pbegin.data(), P));
        CAPI_HIP(sc.alloc(&d_lin, n_lin));
        if (int rc = fgfa_dev::gather_u32(d_steps, N, d_pb, d_pstart, P, n_lin, d_lin, st)) return rc;
        d_steps = d_lin;
    }
    g.steps = d_steps;

    fgfa_dev::ExtractJob *job = sc.hold<fgfa_dev::ExtractJob, fgfa_dev::extract_free>(fgfa_dev::extract_new());
    int rc = fgfa_dev::extract_begin(job, g, st);
    if (rc) return rc;
    std::vector<uint32_t> order;  // old ids in new-id order (seg_map, extract.rs:9, inverted)
    if ((rc = fgfa_dev::extract_bfs(job, origin_seg, link_distance, &order))) return rc;
    if ((rc = fgfa_dev::extract_positions(job))) return rc;

    // merge_subpaths (extract.rs:65-98, 181-185), on the host over each path's prefix of steps that start at or before
    // max_distance_subpaths: a fill happens only on re-entry at such a step, and the paths and sweeps depend on one another in order
    if (num_iterations && P) {
        std::vector<uint32_t> plen(P);
        if ((rc = fgfa_dev::extract_prefix_lens(job, max_distance_subpaths, plen.data()))) return rc;
        const size_t n_bfs = order.size();
        fgfa_dev::extract_merge_host(reinterpret_cast<const uint32_t *>(v.steps.data), pbegin.data(), plen.data(), P, S, num_iterations, &order);
        if ((rc = fgfa_dev::extract_add(job, order.data() + n_bfs, order.size() - n_bfs, n_bfs))) return rc;
    }

    fgfa_dev::ExtractTotals tot;
    if ((rc = fgfa_dev::extract_count(job, &tot))) return rc;
    // the new segments, and where their sequences and optional data go
    const size_t S2 = order.size();
    std::vector<uint32_t> lay(4 * S2);  // seq src, seq dst, optional src, optional dst
    uint32_t *seq_src = lay.data(), *seq_dst = seq_src + S2, *opt_src = seq_dst + S2, *opt_dst = opt_src + S2;
    uint64_t n_seq = 0, n_opt = 0;
    for (size_t k = 0; k < S2; ++k) {
        const fgfa::Segment sg = v.segs[order[k]];
        seq_src[k] = sg.seq.start, seq_dst[k] = (uint32_t)n_seq, opt_src[k] = sg.optional.start, opt_dst[k] = (uint32_t)n_opt;
        n_seq += sg.seq.len();
        n_opt += sg.optional.len();
        if (n_seq > 0xFFFFFFFFull || n_opt > 0xFFFFFFFFull) {
            set_error("flatgfa_extract: the subgraph's sequences or optional data pass 2^32 - 1 bytes");
            return FLATGFA_ERR_TOO_LARGE;
        }
    }
    uint32_t *d_lay = nullptr;
    uint8_t *d_seq2 = nullptr, *d_opt = nullptr, *d_opt2 = nullptr;
    fgfa_dev::ExtractOut o;
    uint32_t *d_align = nullptr;
    CAPI_HIP(sc.upload(&d_lay, lay.data(), lay.size()));
    CAPI_HIP(sc.alloc(&d_seq2, n_seq));
    CAPI_HIP(sc.alloc(&o.steps, tot.steps));
    CAPI_HIP(sc.alloc(&o.recs, tot.paths));
    CAPI_HIP(sc.alloc(&o.links, tot.links * 4));
    CAPI_HIP(sc.alloc(&o.align, tot.ops));
    if (tot.ops) CAPI_HIP(sc.upload(&d_align, v.alignment.data, A));
    o.align_src = d_align;
    if ((rc = fgfa_dev::extract_fill(job, o))) return rc;
    if ((rc = fgfa_dev::gather_bytes(gfa->d_gaf_seq_data, v.seq_data.len, d_lay, d_lay + S2, S2, n_seq, d_seq2, st))) return rc;
    if (n_opt) {
        CAPI_HIP(sc.upload(&d_opt, v.optional_data.data, v.optional_data.len));
        CAPI_HIP(sc.alloc(&d_opt2, n_opt));
        if ((rc = fgfa_dev::gather_bytes(d_opt, v.optional_data.len, d_lay + 2 * S2, d_lay + 3 * S2, S2, n_opt, d_opt2, st))) return rc;
    }

    auto cs = std::make_unique<CStore>();
    fgfa::Store &h = cs->heap;
    std::vector<fgfa_dev::SubpathRec> recs(tot.paths);
    CAPI_HIP(fgfa_dev::staged_copy(recs.data(), o.recs, tot.paths * sizeof(fgfa_dev::SubpathRec), hipMemcpyDeviceToHost, st));
    // include_subpath (extract.rs:56-61): "{name}:{start}-{end}"
    uint64_t n_name = 0;
    for (const auto &r : recs) {
        if (r.path >= P) { set_error("flatgfa_extract: internal: a subpath names no path"); return FLATGFA_ERR_HIP; }
        n_name += v.paths[r.path].name.len() + 2 + std::to_string(r.start).size() + std::to_string(r.end).size();
    }
    if (n_name > 0xFFFFFFFFull) {
        set_error("flatgfa_extract: the subpaths' names would take " + std::to_string(n_name) + " bytes: more than 32-bit spans hold");
        return FLATGFA_ERR_TOO_LARGE;
    }
    h.header.assign(v.header.begin(), v.header.end());
    h.segs.resize(S2);
    for (size_t k = 0; k < S2; ++k) {
        const fgfa::Segment sg = v.segs[order[k]];
        h.segs[k] = fgfa::Segment{sg.name, fgfa::Span{seq_dst[k], seq_dst[k] + sg.seq.len()}, fgfa::Span{opt_dst[k], opt_dst[k] + sg.optional.len()}};
    }
    h.name_data.reserve(n_name);
    h.paths.resize(tot.paths);
    for (size_t k = 0; k < recs.size(); ++k) {
        const fgfa_dev::SubpathRec &r = recs[k];
        const fgfa::Span nm = v.paths[r.path].name;
        const uint32_t b = (uint32_t)h.name_data.size();
        h.name_data.insert(h.name_data.end(), v.name_data.data + nm.start, v.name_data.data + nm.end);
        const std::string tail = ":" + std::to_string(r.start) + "-" + std::to_string(r.end);
        h.name_data.insert(h.name_data.end(), tail.begin(), tail.end());
        h.paths[k] = fgfa::Path{fgfa::Span{b, (uint32_t)h.name_data.size()}, fgfa::Span{(uint32_t)r.step_begin, (uint32_t)r.step_end}, fgfa::Span{0, 0}};
    }
    h.steps.resize(tot.steps);
    h.links.resize(tot.links);
    h.alignment.resize(tot.ops);
    h.seq_data.resize(n_seq);
    h.optional_data.resize(n_opt);
    CAPI_HIP(fgfa_dev::staged_copy(h.steps.data(), o.steps, tot.steps * 4, hipMemcpyDeviceToHost, st));
    CAPI_HIP(fgfa_dev::staged_copy(h.links.data(), o.links, tot.links * 16, hipMemcpyDeviceToHost, st));
    CAPI_HIP(fgfa_dev::staged_copy(h.alignment.data(), o.align, tot.ops * 4, hipMemcpyDeviceToHost, st));
    CAPI_HIP(fgfa_dev::staged_copy(h.seq_data.data(), d_seq2, n_seq, hipMemcpyDeviceToHost, st));
    if (n_opt) CAPI_HIP(fgfa_dev::staged_copy(h.optional_data.data(), d_opt2, n_opt, hipMemcpyDeviceToHost, st));
    cs->view = h.view();
    *out = cs.release();
    return FLATGFA_OK;
}

int flatgfa_position(flatgfa_t gfa, uint32_t path, uint64_t offset, uint32_t *handle_out, uint64_t *seg_offset_out, int *found) {
    if (found) *found = 0;
    if (!gfa || !handle_out || !seg_offset_out || !found) { set_error("flatgfa_position: NULL argument"); return FLATGFA_ERR_ARG; }
    std::lock_guard<std::mutex> op(gfa->op_mu);
    const fgfa::View &v = gfa->view;
    if (path >= v.paths.len) { set_error("flatgfa_position: the path index is out of range"); return FLATGFA_ERR_BOUNDS; }
    const fgfa::Span sp = v.paths[path].steps;
    if (sp.start > sp.end || sp.end > v.steps.len) { set_error("flatgfa_position: the path has a step span outside the steps pool"); return FLATGFA_ERR_BOUNDS; }
    if (v.segs.len > 0x80000000ull) { set_error("flatgfa_position: graph too large for 32-bit ids"); return FLATGFA_ERR_TOO_LARGE; }
    DevScope sc;
    if (int rc = open_scope(gfa, &sc, "position")) return rc;
    if (int rc = ensure_gaf_seqs(gfa, sc.device)) return rc;
    const uint32_t *d_steps = nullptr;
    if (sc.resident) {
        d_steps = gfa->d_steps + sp.start;
    } else {
        uint32_t *d = nullptr;
        CAPI_HIP(sc.upload(&d, v.steps.data + sp.start, sp.len()));
        d_steps = d;
    }
    uint64_t index = 0, start = 0;
    if (int rc = fgfa_dev::position_find(d_steps, sp.len(), gfa->d_gaf_seg_seq, (uint32_t)v.segs.len, offset, sc.stream, &index, &start)) return rc;
    if (index < sp.len()) {
        *handle_out = v.steps[sp.start + index].bits;
        *seg_offset_out = offset - start;
        *found = 1;
    }
    return FLATGFA_OK;
}

int flatgfa_position_table(flatgfa_t gfa, const uint8_t *triple, size_t len, char **text, size_t *n) {
    if (text) *text = nullptr;
    if (n) *n = 0;
    if (!gfa || !text || !n || (len && !triple)) { set_error("flatgfa_position_table: NULL argument"); return FLATGFA_ERR_ARG; }
    // cmds.rs:114-132, with its messages
    const std::string arg((const char *)triple, len);
    std::vector<std::string> parts(1);
    for (char c : arg) {
        if (c == ',') parts.emplace_back();
        else parts.back().push_back(c);
    }
    if (parts.size() != 3) { set_error("position must be path_name,offset,orientation"); return FLATGFA_ERR_ARG; }
    uint64_t offset = 0;
    {   // usize::from_str: an optional '+', then digits only, within 64 bits
        const std::string &t = parts[1];
        size_t k = !t.empty() && t[0] == '+' ? 1 : 0;
        bool ok = k < t.size();
        for (; ok && k < t.size(); ++k) {
            if (t[k] < '0' || t[k] > '9') { ok = false; break; }
            const uint64_t d = (uint64_t)(t[k] - '0');
            if (offset > (UINT64_MAX - d) / 10) { ok = false; break; }
            offset = offset * 10 + d;
        }
        if (!ok) { set_error("offset must be a number"); return FLATGFA_ERR_ARG; }
    }
    if (parts[2] != "+" && parts[2] != "-") { set_error("orientation must be + or -"); return FLATGFA_ERR_ARG; }
    const int64_t path = gfa->view.find_path((const uint8_t *)parts[0].data(), parts[0].size());
    if (path < 0) { set_error("path not found"); return FLATGFA_ERR_ARG; }
    if (parts[2] != "+") { set_error("only + is implemented so far"); return FLATGFA_ERR_ARG; }
    uint32_t handle = 0;
    uint64_t seg_off = 0;
    int found = 0;
    if (int rc = flatgfa_position(gfa, (uint32_t)path, offset, &handle, &seg_off, &found)) return rc;
    std::string out;
    if (found) {  // cmds.rs:136-149
        out = "#source.path.pos\ttarget.graph.pos\n" + parts[0] + "," + std::to_string(offset) + ",+\t" +
              std::to_string(gfa->view.segs[handle >> 1].name) + "," + std::to_string(seg_off) + "," + ((handle & 1u) ? "-" : "+") + "\n";
    }
    char *buf = (char *)malloc(out.size() + 1);
    if (!buf) { set_error("flatgfa_position_table: out of memory"); return FLATGFA_ERR_ARG; }
    memcpy(buf, out.data(), out.size());
    buf[out.size()] = 0;
    *text = buf;
    *n = out.size();
    return FLATGFA_OK;
}

// ---- validate (slow_odgi/validate.py) and degree (slow_odgi/degree.py) ----

extern "C++" {
namespace {
// The handle's link index on `device` (the current device), made once: the links are uploaded for the build only.
int ensure_topo(CStore *cs, DevScope *sc) {
    if (cs->topo_device == sc->device) return FLATGFA_OK;
    const fgfa::View &v = cs->view;
    if (v.links.len > 0xFFFFFFFFull || v.segs.len > 0x7FFFFFFFull) {
        set_error("topology: graph too large for 32-bit ids");
        return FLATGFA_ERR_TOO_LARGE;
    }
    uint32_t *d_links = nullptr;
    CAPI_HIP(hipMalloc((void **)&d_links, std::max<size_t>(v.links.len, 1) * 16));
    hipError_t e = hipSuccess;
    if (v.links.len) e = fgfa_dev::staged_copy(d_links, v.links.data, v.links.len * 16, hipMemcpyHostToDevice, sc->stream);
    fgfa_dev::TopoIndex ix;
    int rc = FLATGFA_OK;
    if (e == hipSuccess) rc = fgfa_dev::topo_index_build(d_links, v.links.len, (uint32_t)v.segs.len, sc->stream, &ix);
    (void)hipStreamSynchronize(sc->stream);
    (void)hipFree(d_links);
    CAPI_HIP(e);
    if (rc) return rc;
    fgfa_dev::topo_index_free(&cs->topo);  // (the handle moved to another device)
    cs->topo = ix;
    cs->topo_device = sc->device;
    return FLATGFA_OK;
}
}  // namespace
}  // extern "C++"

int flatgfa_validate(flatgfa_t gfa, flatgfa_missing_link_t **out, uint64_t *n) {
    if (out) *out = nullptr;
    if (n) *n = 0;
    if (!gfa || !n) { set_error("flatgfa_validate: NULL argument"); return FLATGFA_ERR_ARG; }
    std::lock_guard<std::mutex> op(gfa->op_mu);
    const fgfa::View &v = gfa->view;
    const size_t N = v.steps.len, P = v.paths.len;
    if (N > 0xFFFFFFFFull || P > 0xFFFFFFFEull) { set_error("flatgfa_validate: graph too large for 32-bit ids"); return FLATGFA_ERR_TOO_LARGE; }
    // the paths' steps numbered one behind another, whatever their spans do in the pool (they may overlap or leave gaps)
    std::vector<uint32_t> pstart(P + 1, 0), pbegin(P + 1, 0);
    uint64_t n_lin = 0;
    for (size_t p = 0; p < P; ++p) {
        const fgfa::Span sp = v.paths[p].steps;
        if (sp.start > sp.end || sp.end > N) { set_error("flatgfa_validate: a path has a step span outside the steps pool"); return FLATGFA_ERR_BOUNDS; }
        pbegin[p] = sp.start;
        n_lin += sp.len();
        if (n_lin > 0xFFFFFFFFull) { set_error("flatgfa_validate: the paths hold more than 2^32 - 1 steps"); return FLATGFA_ERR_TOO_LARGE; }
        pstart[p + 1] = (uint32_t)n_lin;
    }
    DevScope sc;
    if (int rc = open_scope(gfa, &sc, "validate")) return rc;
    if (int rc = ensure_topo(gfa, &sc)) return rc;
    fgfa_dev::TopoSteps ts;
    uint32_t *d_pstart = nullptr, *d_pbegin = nullptr, *d_steps = nullptr;
    CAPI_HIP(sc.upload(&d_pstart, pstart.data(), P + 1));
    CAPI_HIP(sc.upload(&d_pbegin, pbegin.data(), P + 1));
    if (sc.resident) d_steps = gfa->d_steps;  // (read in place)
    else CAPI_HIP(sc.upload(&d_steps, v.steps.data, N));
    ts.steps = d_steps, ts.pstart = d_pstart, ts.pbegin = d_pbegin, ts.n_paths = (uint32_t)P, ts.n_lin = n_lin;
    fgfa_dev::ValidateJob *job = sc.hold<fgfa_dev::ValidateJob, fgfa_dev::validate_free>(fgfa_dev::validate_new());
    uint64_t count = 0;
    if (int rc = fgfa_dev::validate_count(job, gfa->topo, ts, sc.stream, &count)) return rc;
    *n = count;
    if (!out || !count) return FLATGFA_OK;
    flatgfa_missing_link_t *recs = (flatgfa_missing_link_t *)malloc((size_t)count * sizeof *recs);
    if (!recs) { set_error("flatgfa_validate: out of memory"); return FLATGFA_ERR_IO; }
    if (int rc = fgfa_dev::validate_fill(job, recs)) {
        free(recs);
        return rc;
    }
    *out = recs;
    return FLATGFA_OK;
}

void flatgfa_missing_links_free(flatgfa_missing_link_t *p) { free(p); }

int flatgfa_validate_table(flatgfa_t gfa, char **text, size_t *len) {
    if (text) *text = nullptr;
    if (len) *len = 0;
    if (!gfa || !text) { set_error("flatgfa_validate_table: NULL argument"); return FLATGFA_ERR_ARG; }
    flatgfa_missing_link_t *recs = nullptr;
    uint64_t n = 0;
    if (int rc = flatgfa_validate(gfa, &recs, &n)) return rc;
    // the text is made on the host: a graph worth validating has few or no missing links
    static_assert(sizeof(fgfa::MissingLink) == sizeof(flatgfa_missing_link_t), "one record layout");
    std::string out;
    const bool ok = fgfa::emit_missing_links(gfa->view, reinterpret_cast<const fgfa::MissingLink *>(recs), (size_t)n, &out);
    flatgfa_missing_links_free(recs);
    if (!ok) { set_error("flatgfa_validate_table: internal: a record names no path or segment"); return FLATGFA_ERR_HIP; }
    return give_text(out, text, len);
}

int flatgfa_degree(flatgfa_t gfa, uint64_t *degree_out) {
    if (!gfa || !degree_out) { set_error("flatgfa_degree: NULL argument"); return FLATGFA_ERR_ARG; }
    std::lock_guard<std::mutex> op(gfa->op_mu);
    DevScope sc;
    if (int rc = open_scope(gfa, &sc, "degree")) return rc;
    if (int rc = ensure_topo(gfa, &sc)) return rc;
    return fgfa_dev::topo_degree(gfa->topo, sc.stream, degree_out);
}

int flatgfa_degree_table(flatgfa_t gfa, char **text, size_t *len) {
    if (text) *text = nullptr;
    if (len) *len = 0;
    if (!gfa || !text) { set_error("flatgfa_degree_table: NULL argument"); return FLATGFA_ERR_ARG; }
    std::vector<uint64_t> deg(gfa->view.segs.len + 1, 0);
    if (int rc = flatgfa_degree(gfa, deg.data())) return rc;
    std::string out;
    fgfa::emit_degree(gfa->view, deg.data(), &out);
    return give_text(out, text, len);
}

// ---- flatten (slow_odgi/flatten.py) ----

extern "C++" {
namespace {
// How many BED lines a chunk holds: kFlatChunkLines, or what the tests ask for.
uint64_t flatten_chunk_lines() {
    if (const char *h = test_hook("FLATGFA_FLATTEN_CHUNK_LINES")) return std::max<uint64_t>(1, strtoull(h, nullptr, 10));
    return fgfa_dev::kFlatChunkLines;
}

// The handle's legend on `device` (the current device), made once from the segments' spans.  A span that leaves seq_data,
// where the reference could not have read the segment, is refused here.
int ensure_flat_legend(CStore *cs, DevScope *sc) {
    if (cs->flat_device == sc->device) return FLATGFA_OK;
    const fgfa::View &v = cs->view;
    const size_t S = v.segs.len;
    if (S > 0x80000000ull) { set_error("flatten: graph too large for 32-bit ids"); return FLATGFA_ERR_TOO_LARGE; }
    std::vector<uint32_t> len(S);
    for (size_t i = 0; i < S; ++i) {
        const fgfa::Span sp = v.segs[i].seq;
        if (sp.start > sp.end || sp.end > v.seq_data.len) {
            set_error("flatten: segment " + std::to_string(i) + " has a sequence span outside seq_data");
            return FLATGFA_ERR_BOUNDS;
        }
        len[i] = sp.end - sp.start;
    }
    uint32_t *d_len = nullptr;
    uint64_t *d_legend = nullptr;
    CAPI_HIP(sc->upload(&d_len, len.data(), S));
    CAPI_HIP(hipMalloc((void **)&d_legend, (S + 1) * 8));
    int rc = fgfa_dev::flatten_legend(d_len, (uint32_t)S, d_legend, sc->stream);
    uint64_t total = 0;
    if (!rc && hipMemcpy(&total, d_legend + S, 8, hipMemcpyDeviceToHost) != hipSuccess) {
        set_error("flatten: reading the legend's total failed");
        rc = FLATGFA_ERR_HIP;
    }
    (void)sc->release(d_len);
    if (rc) {
        (void)hipFree(d_legend);
        return rc;
    }
    if (cs->d_flat_legend) (void)hipFree(cs->d_flat_legend);  // (the handle moved to another device)
    cs->d_flat_legend = d_legend;
    cs->flat_total = total;
    cs->flat_device = sc->device;
    return FLATGFA_OK;
}

// One flatten call between its two halves: everything is checked and counted (open) before a byte is delivered (emit).
struct FlatCall {
    DevScope sc;
    fgfa_dev::FlatJob *job = nullptr;
    fgfa_dev::FlatSeqs seqs;
    const uint8_t *name = nullptr;
    size_t name_len = 0;
    int what = 0;
    uint64_t fasta_bytes = 0, bed_bytes = 0;
};

int flat_open(CStore *gfa, FlatCall *c, const char *name, size_t name_len, int what) {
    c->name = (const uint8_t *)name, c->name_len = name_len, c->what = what;
    const fgfa::View &v = gfa->view;
    const size_t N = v.steps.len, P = v.paths.len;
    // the paths' steps numbered one behind another, whatever their spans do in the pool (they may overlap, alias or be empty)
    std::vector<uint64_t> pstart;
    std::vector<uint32_t> prec;
    if (what & 2) {
        if (N > 0xFFFFFFFFull || P > 0xFFFFFFFEull) { set_error("flatten: graph too large for 32-bit ids"); return FLATGFA_ERR_TOO_LARGE; }
        pstart.assign(P + 1, 0), prec.assign(3 * P, 0);
        for (size_t p = 0; p < P; ++p) {
            const fgfa::Span sp = v.paths[p].steps, nm = v.paths[p].name;
            if (sp.start > sp.end || sp.end > N) { set_error("flatten: a path has a step span outside the steps pool"); return FLATGFA_ERR_BOUNDS; }
            if (nm.start > nm.end || nm.end > v.name_data.len) { set_error("flatten: a path has a name span outside name_data"); return FLATGFA_ERR_BOUNDS; }
            prec[3 * p] = sp.start, prec[3 * p + 1] = nm.start, prec[3 * p + 2] = nm.len();
            pstart[p + 1] = pstart[p] + sp.len();
        }
    }
    DevScope &sc = c->sc;
    if (int rc = open_scope(gfa, &sc, "flatten")) return rc;
    if (int rc = ensure_flat_legend(gfa, &sc)) return rc;
    c->job = sc.hold<fgfa_dev::FlatJob, fgfa_dev::flatten_free>(fgfa_dev::flatten_new(flatten_chunk_lines()));
    if (what & 1) {
        if (int rc = ensure_gaf_seqs(gfa, sc.device)) return rc;  // (starts and bases, kept with the handle)
        c->seqs.legend = gfa->d_flat_legend, c->seqs.seg_seq = gfa->d_gaf_seg_seq, c->seqs.seq_data = gfa->d_gaf_seq_data;
        c->seqs.n_segs = (uint32_t)v.segs.len, c->seqs.total = gfa->flat_total;
        c->fasta_bytes = fgfa_dev::flatten_fasta_bytes(gfa->flat_total, name_len);
    }
    if (what & 2) {
        fgfa_dev::FlatPaths g;
        uint64_t *d_pstart = nullptr;
        uint32_t *d_prec = nullptr, *d_steps = nullptr;
        uint8_t *d_names = nullptr;
        CAPI_HIP(sc.upload(&d_pstart, pstart.data(), P + 1));
        CAPI_HIP(sc.upload(&d_prec, prec.data(), 3 * P));
        CAPI_HIP(sc.upload(&d_names, v.name_data.data, v.name_data.len));
        if (sc.resident) d_steps = gfa->d_steps;  // (read in place)
        else CAPI_HIP(sc.upload(&d_steps, v.steps.data, N));
        g.legend = gfa->d_flat_legend, g.n_segs = (uint32_t)v.segs.len, g.steps = d_steps, g.pstart = d_pstart, g.prec = d_prec;
        g.name_data = d_names, g.n_paths = (uint32_t)P, g.n_lines = pstart[P];
        if (int rc = fgfa_dev::flatten_bed_begin(c->job, g, c->name, name_len, sc.stream, &c->bed_bytes)) return rc;
    }
    return FLATGFA_OK;
}

int flat_emit(FlatCall *c, flatgfa_sink_t sink, void *ctx) {
    if (c->what & 1)
        if (int rc = fgfa_dev::flatten_fasta(c->job, c->seqs, c->name, c->name_len, c->sc.stream, sink, ctx)) return rc;
    if (c->what & 2)
        if (int rc = fgfa_dev::flatten_bed_emit(c->job, sink, ctx)) return rc;
    return FLATGFA_OK;
}

int flat_args(const char *who, flatgfa_t gfa, const char *name, size_t name_len, const void *a, const void *b) {
    if (gfa && a && b && (name || !name_len)) return FLATGFA_OK;
    set_error(std::string(who) + ": NULL argument");
    return FLATGFA_ERR_ARG;
}

// the stream into a malloc'd buffer of the size flat_open counted
struct TextSink {
    char *buf;
    size_t cap, at;
    static int take(void *ctx, const char *bytes, size_t n) {
        TextSink *t = static_cast<TextSink *>(ctx);
        if (n > t->cap - t->at) return 1;
        memcpy(t->buf + t->at, bytes, n);
        t->at += n;
        return 0;
    }
};

int flat_text(const char *who, flatgfa_t gfa, const char *name, size_t name_len, int what, char **text, size_t *len) {
    if (text) *text = nullptr;
    if (len) *len = 0;
    if (int rc = flat_args(who, gfa, name, name_len, text, len)) return rc;
    std::lock_guard<std::mutex> op(gfa->op_mu);
    FlatCall c;
    if (int rc = flat_open(gfa, &c, name, name_len, what)) return rc;
    TextSink t{nullptr, (size_t)(c.fasta_bytes + c.bed_bytes), 0};
    t.buf = (char *)malloc(t.cap + 1);
    if (!t.buf) { set_error(std::string(who) + ": out of memory"); return FLATGFA_ERR_IO; }
    int rc = flat_emit(&c, TextSink::take, &t);
    if (!rc && t.at != t.cap) { set_error(std::string(who) + ": internal: the text is not as long as it was counted"); rc = FLATGFA_ERR_HIP; }
    if (rc) {
        free(t.buf);
        return rc;
    }
    t.buf[t.cap] = 0;
    *text = t.buf;
    *len = t.cap;
    return FLATGFA_OK;
}
}  // namespace
}  // extern "C++"

int flatgfa_flatten_legend(flatgfa_t gfa, uint64_t *offset_out) {
    if (!gfa || !offset_out) { set_error("flatgfa_flatten_legend: NULL argument"); return FLATGFA_ERR_ARG; }
    std::lock_guard<std::mutex> op(gfa->op_mu);
    DevScope sc;
    if (int rc = open_scope(gfa, &sc, "flatten")) return rc;
    if (int rc = ensure_flat_legend(gfa, &sc)) return rc;
    CAPI_HIP(fgfa_dev::staged_copy(offset_out, gfa->d_flat_legend, (gfa->view.segs.len + 1) * 8, hipMemcpyDeviceToHost, sc.stream));
    return FLATGFA_OK;
}

int flatgfa_flatten_fasta(flatgfa_t gfa, const char *name, size_t name_len, char **text, size_t *len) {
    return flat_text("flatgfa_flatten_fasta", gfa, name, name_len, 1, text, len);
}

int flatgfa_flatten_bed(flatgfa_t gfa, const char *name, size_t name_len, char **text, size_t *len) {
    return flat_text("flatgfa_flatten_bed", gfa, name, name_len, 2, text, len);
}

int flatgfa_flatten_stream(flatgfa_t gfa, const char *name, size_t name_len, int what, flatgfa_sink_t sink, void *ctx) {
    if (int rc = flat_args("flatgfa_flatten_stream", gfa, name, name_len, (const void *)sink, (const void *)sink)) return rc;
    if (what < 1 || what > 3) { set_error("flatgfa_flatten_stream: `what` is 1 (FASTA), 2 (BED) or 3 (both)"); return FLATGFA_ERR_ARG; }
    std::lock_guard<std::mutex> op(gfa->op_mu);
    FlatCall c;
    if (int rc = flat_open(gfa, &c, name, name_len, what)) return rc;
    return flat_emit(&c, sink, ctx);
}

// ---- the GFA printer on the device (flatgfa/src/print.rs:99-153) ----

extern "C++" {
namespace {
static_assert(sizeof(fgfa_dev::PrintSeg) == sizeof(fgfa::Segment), "the segs pool is read as it is");

// How many items a chunk holds: kPrintChunkItems, or what the tests ask for.
uint64_t print_chunk_items() {
    if (const char *h = test_hook("FLATGFA_PRINT_CHUNK_ITEMS")) return std::max<uint64_t>(1, strtoull(h, nullptr, 10));
    return fgfa_dev::kPrintChunkItems;
}

int print_refuse(const char *what, int rc = FLATGFA_ERR_BOUNDS) {
    set_error(what);
    return rc;
}
bool span_in(fgfa::Span sp, size_t pool_len) { return sp.start <= sp.end && sp.end <= pool_len; }

// One print call between its two halves: everything is checked and counted (open) before a byte is delivered (emit).
struct PrintCall {
    DevScope sc;
    fgfa_dev::PrintJob *job = nullptr;
    uint64_t bytes = 0;
};

int print_open(CStore *gfa, PrintCall *c) {
    const fgfa::View &v = gfa->view;
    const size_t S = v.segs.len, P = v.paths.len, L = v.links.len, N = v.steps.len;
    if (N > 0xFFFFFFFFull || S > 0x80000000ull || P > 0xFFFFFFFFull || L > 0xFFFFFFFFull)
        return print_refuse("print: graph too large for 32-bit ids", FLATGFA_ERR_TOO_LARGE);
    // The lines, and what print_gfa stops at first (flatgfa_core.cpp, print.rs:99-150): one pass, no device.
    fgfa_dev::PrintGraph g;
    if (!v.line_order.len) {
        g.header_lines = v.header.len ? 1 : 0, g.seg_lines = S, g.path_lines = P, g.link_lines = L;
        for (size_t p = 0; p < P; ++p)
            if (v.paths[p].steps.start == v.paths[p].steps.end) return print_refuse("print: path with no steps");
    } else {
        for (size_t k = 0; k < v.line_order.len; ++k) {
            switch (v.line_order[k]) {
                case fgfa::kHeader:
                    if (!v.header.len) return print_refuse("print: empty header");
                    ++g.header_lines;
                    break;
                case fgfa::kSegment:
                    if (g.seg_lines >= S) return print_refuse("print: too few segments");
                    ++g.seg_lines;
                    break;
                case fgfa::kPath:
                    if (g.path_lines >= P) return print_refuse("print: too few paths");
                    if (v.paths[g.path_lines].steps.start == v.paths[g.path_lines].steps.end) return print_refuse("print: path with no steps");
                    ++g.path_lines;
                    break;
                case fgfa::kLink:
                    if (g.link_lines >= L) return print_refuse("print: too few links");
                    ++g.link_lines;
                    break;
                default:
                    return print_refuse("print: bad line kind");
            }
        }
    }
    g.n_lines = g.header_lines + g.seg_lines + g.path_lines + g.link_lines;
    // Refused where the host printer would read outside a pool: the spans and link handles of the lines that are printed.
    for (size_t i = 0; i < g.seg_lines; ++i) {
        if (!span_in(v.segs[i].seq, v.seq_data.len)) return print_refuse("print: a segment has a sequence span outside seq_data");
        if (!span_in(v.segs[i].optional, v.optional_data.len)) return print_refuse("print: a segment has an optional span outside optional_data");
    }
    for (size_t i = 0; i < g.path_lines; ++i) {
        const fgfa::Path &p = v.paths[i];
        if (!span_in(p.name, v.name_data.len)) return print_refuse("print: a path has a name span outside name_data");
        if (!span_in(p.steps, N)) return print_refuse("print: a path has a step span outside the steps pool");
        if (!span_in(p.overlaps, v.overlaps.len)) return print_refuse("print: a path has an overlaps span outside the overlaps pool");
        for (uint32_t o = p.overlaps.start; o < p.overlaps.end; ++o)
            if (!span_in(v.overlaps[o], v.alignment.len)) return print_refuse("print: a path overlap has a span outside the alignment pool");
    }
    for (size_t i = 0; i < g.link_lines; ++i) {
        const fgfa::Link &l = v.links[i];
        if ((l.from >> 1) >= S || (l.to >> 1) >= S) return print_refuse("print: a link refers to a segment id that is out of range");
        if (!span_in(l.overlap, v.alignment.len)) return print_refuse("print: a link has an overlap span outside the alignment pool");
    }
    DevScope &sc = c->sc;
    if (int rc = open_scope(gfa, &sc, "the device GFA printer")) return rc;
    c->job = sc.hold<fgfa_dev::PrintJob, fgfa_dev::print_free>(fgfa_dev::print_new(print_chunk_items()));
    if (!g.n_lines) return fgfa_dev::print_begin(c->job, g, sc.stream, &c->bytes);  // (no text: nothing to upload)
    // the pools as they are (the segment names in full: u64, as the pool holds them)
    uint8_t *d_header = nullptr, *d_seq = nullptr, *d_names = nullptr, *d_opt = nullptr, *d_order = nullptr;
    fgfa_dev::PrintSeg *d_segs = nullptr;
    uint32_t *d_paths = nullptr, *d_links = nullptr, *d_steps = nullptr, *d_overlaps = nullptr, *d_align = nullptr;
    CAPI_HIP(sc.upload(&d_header, v.header.data, v.header.len));
    CAPI_HIP(sc.upload(&d_segs, v.segs.data, S));
    CAPI_HIP(sc.upload(&d_paths, v.paths.data, 6 * P));
    CAPI_HIP(sc.upload(&d_links, v.links.data, 4 * L));
    CAPI_HIP(sc.upload(&d_overlaps, v.overlaps.data, 2 * v.overlaps.len));
    CAPI_HIP(sc.upload(&d_align, v.alignment.data, v.alignment.len));
    CAPI_HIP(sc.upload(&d_seq, v.seq_data.data, v.seq_data.len));
    CAPI_HIP(sc.upload(&d_names, v.name_data.data, v.name_data.len));
    CAPI_HIP(sc.upload(&d_opt, v.optional_data.data, v.optional_data.len));
    if (v.line_order.len) CAPI_HIP(sc.upload(&d_order, v.line_order.data, v.line_order.len));
    if (sc.resident) d_steps = gfa->d_steps;  // (read in place)
    else CAPI_HIP(sc.upload(&d_steps, v.steps.data, N));
    g.header = d_header, g.header_len = (uint32_t)v.header.len, g.segs = d_segs, g.n_segs = (uint32_t)S, g.paths = d_paths, g.links = d_links;
    g.steps = d_steps, g.overlaps = d_overlaps, g.alignment = d_align, g.seq_data = d_seq, g.name_data = d_names, g.optional_data = d_opt;
    g.line_order = d_order;
    return fgfa_dev::print_begin(c->job, g, sc.stream, &c->bytes);
}
}  // namespace
}  // extern "C++"

int flatgfa_print_gfa_bytes(flatgfa_t gfa, uint64_t *bytes) {
    if (!gfa || !bytes) { set_error("flatgfa_print_gfa_bytes: NULL argument"); return FLATGFA_ERR_ARG; }
    *bytes = 0;
    std::lock_guard<std::mutex> op(gfa->op_mu);
    PrintCall c;
    if (int rc = print_open(gfa, &c)) return rc;
    *bytes = c.bytes;
    return FLATGFA_OK;
}

int flatgfa_print_gfa_device(flatgfa_t gfa, char **text, size_t *len) {
    if (text) *text = nullptr;
    if (len) *len = 0;
    if (!gfa || !text || !len) { set_error("flatgfa_print_gfa_device: NULL argument"); return FLATGFA_ERR_ARG; }
    std::lock_guard<std::mutex> op(gfa->op_mu);
    PrintCall c;
    if (int rc = print_open(gfa, &c)) return rc;
    TextSink t{nullptr, (size_t)c.bytes, 0};
    t.buf = (char *)malloc(t.cap + 1);
    if (!t.buf) { set_error("flatgfa_print_gfa_device: out of memory"); return FLATGFA_ERR_IO; }
    int rc = fgfa_dev::print_emit(c.job, TextSink::take, &t);
    if (!rc && t.at != t.cap) { set_error("flatgfa_print_gfa_device: internal: the text is not as long as it was counted"); rc = FLATGFA_ERR_HIP; }
    if (rc) {
        free(t.buf);
        return rc;
    }
    t.buf[t.cap] = 0;
    *text = t.buf;
    *len = t.cap;
    return FLATGFA_OK;
}

int flatgfa_print_gfa_stream(flatgfa_t gfa, flatgfa_sink_t sink, void *ctx) {
    if (!gfa || !sink) { set_error("flatgfa_print_gfa_stream: NULL argument"); return FLATGFA_ERR_ARG; }
    std::lock_guard<std::mutex> op(gfa->op_mu);
    PrintCall c;
    if (int rc = print_open(gfa, &c)) return rc;
    return fgfa_dev::print_emit(c.job, sink, ctx);
}

// ---- BED intersection (cli/cmds.rs:392-413, flatbed.rs:37-57) ----

extern "C++" {
namespace {
// How many candidates a round holds: kBedRoundCands, or what the tests ask for.
uint64_t bed_round_cands() {
    if (const char *h = test_hook("FLATGFA_BED_ROUND_CANDS")) return std::max<uint64_t>(1, strtoull(h, nullptr, 10));
    return fgfa_dev::kBedRoundCands;
}

int bed_refuse(const char *what) {
    set_error(what);
    return FLATGFA_ERR_BOUNDS;
}

// One side as the device takes it.
struct BedColumns {
    std::vector<uint32_t> id;
    std::vector<uint64_t> start, end;
};

// One intersect call: the texts parsed, B's names interned and B grouped on the host -- all of it O(lines), all of it before
// a device is asked for -- then the entries on the device with the groups and candidate ranges found (bed_begin).
struct BedCall {
    DevScope sc;
    fgfa_dev::BedJob *job = nullptr;
    uint64_t candidates = 0, unsorted_groups = 0;
};

int bed_open(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, BedCall *c) {
    // (parse_bed keeps name offsets in 32 bits; decided before a byte is read)
    if ((uint64_t)a_len >= (1ull << 32) || (uint64_t)b_len >= (1ull << 32)) return bed_refuse("bed: a text of 2^32 bytes or more is not taken");
    fgfa::Bed A, B;
    std::string err;
    if (!fgfa::parse_bed(a ? a : (const uint8_t *)"", a_len, &A, &err) || !fgfa::parse_bed(b ? b : (const uint8_t *)"", b_len, &B, &err)) {
        set_error(err);
        return FLATGFA_ERR_BOUNDS;  // (flatgfa_bed_depth_table's code)
    }
    const size_t nA = A.entries.size(), nB = B.entries.size();
    if (nA >= 0xFFFFFFFFull || nB >= 0xFFFFFFFFull) return bed_refuse("bed: a file of 2^32 - 1 entries or more is not taken");
    // B's names get dense ids in the order they first appear; A's names are looked up in the same table
    const auto name_of = [](const fgfa::Bed &bed, const fgfa::BedEntry &e) {
        return std::string_view((const char *)bed.name_data.data() + e.name_start, e.name_end - e.name_start);
    };
    std::unordered_map<std::string_view, uint32_t> ids;
    std::vector<uint32_t> b_id(nB), gname, group_start(1, 0);
    std::vector<uint8_t> names;
    {
        std::string_view last;
        uint32_t last_id = 0;
        for (size_t i = 0; i < nB; ++i) {
            const std::string_view nm = name_of(B, B.entries[i]);
            if (!i || nm != last) {  // (a file sorted by name asks the table once a name)
                const auto got = ids.emplace(nm, (uint32_t)ids.size());
                if (got.second) {
                    gname.push_back((uint32_t)names.size());
                    gname.push_back((uint32_t)nm.size());
                    names.insert(names.end(), nm.begin(), nm.end());
                    group_start.push_back(0);
                }
                last = nm, last_id = got.first->second;
            }
            b_id[i] = last_id;
            ++group_start[last_id + 1];
        }
    }
    const uint32_t G = (uint32_t)ids.size();
    for (uint32_t g = 0; g < G; ++g) group_start[g + 1] += group_start[g];
    BedColumns ca, cb;  // B grouped by id, stably: file order is kept inside a group
    cb.id.resize(nB), cb.start.resize(nB), cb.end.resize(nB);
    {
        std::vector<uint32_t> next(group_start.begin(), group_start.end() - 1);
        for (size_t i = 0; i < nB; ++i) {
            const uint32_t at = next[b_id[i]]++;
            cb.id[at] = b_id[i], cb.start[at] = B.entries[i].start, cb.end[at] = B.entries[i].end;
        }
    }
    ca.id.resize(nA), ca.start.resize(nA), ca.end.resize(nA);
    {
        std::string_view last;
        uint32_t last_id = fgfa_dev::kBedNone;
        for (size_t i = 0; i < nA; ++i) {
            const std::string_view nm = name_of(A, A.entries[i]);
            if (!i || nm != last) {
                const auto it = ids.find(nm);
                last = nm, last_id = it == ids.end() ? fgfa_dev::kBedNone : it->second;
            }
            ca.id[i] = last_id, ca.start[i] = A.entries[i].start, ca.end[i] = A.entries[i].end;
        }
    }
    DevScope &sc = c->sc;
    if (int rc = open_scope(nullptr, &sc, "bed")) return rc;
    fgfa_dev::BedInput in;
    uint32_t *d_aid = nullptr, *d_bid = nullptr, *d_gname = nullptr;
    uint64_t *d_as = nullptr, *d_ae = nullptr, *d_bs = nullptr, *d_be = nullptr;
    uint8_t *d_names = nullptr;
    CAPI_HIP(sc.upload(&d_aid, ca.id.data(), nA));
    CAPI_HIP(sc.upload(&d_as, ca.start.data(), nA));
    CAPI_HIP(sc.upload(&d_ae, ca.end.data(), nA));
    CAPI_HIP(sc.upload(&d_bid, cb.id.data(), nB));
    CAPI_HIP(sc.upload(&d_bs, cb.start.data(), nB));
    CAPI_HIP(sc.upload(&d_be, cb.end.data(), nB));
    CAPI_HIP(sc.upload(&d_gname, gname.data(), gname.size()));
    CAPI_HIP(sc.upload(&d_names, names.data(), names.size()));
    in.a = fgfa_dev::BedSide{d_aid, d_as, d_ae, nA};
    in.b = fgfa_dev::BedSide{d_bid, d_bs, d_be, nB};
    in.n_groups = G, in.names = d_names, in.gname = d_gname;
    c->job = sc.hold<fgfa_dev::BedJob, fgfa_dev::bed_free>(fgfa_dev::bed_new(bed_round_cands()));
    return fgfa_dev::bed_begin(c->job, in, sc.stream, &c->candidates, &c->unsorted_groups);
}

// a malloc'd text that grows as the pieces arrive
struct GrowSink {
    char *buf = nullptr;
    size_t cap = 0, at = 0;
    static int take(void *ctx, const char *bytes, size_t n) {
        GrowSink *t = static_cast<GrowSink *>(ctx);
        if (n > t->cap - t->at) {
            const size_t cap = std::max(t->at + n, 2 * t->cap);
            char *p = (char *)realloc(t->buf, cap + 1);
            if (!p) return 1;
            t->buf = p, t->cap = cap;
        }
        memcpy(t->buf + t->at, bytes, n);
        t->at += n;
        return 0;
    }
};
}  // namespace
}  // extern "C++"

int flatgfa_bed_intersect(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, char **text, size_t *len) {
    if (text) *text = nullptr;
    if (len) *len = 0;
    if ((!a && a_len) || (!b && b_len) || !text || !len) { set_error("flatgfa_bed_intersect: NULL argument"); return FLATGFA_ERR_ARG; }
    BedCall c;
    if (int rc = bed_open(a, a_len, b, b_len, &c)) return rc;
    GrowSink t;
    t.buf = (char *)malloc(1);
    if (!t.buf) { set_error("flatgfa_bed_intersect: out of memory"); return FLATGFA_ERR_IO; }
    const int rc = fgfa_dev::bed_emit(c.job, GrowSink::take, &t, nullptr);
    if (rc == FLATGFA_ERR_IO) set_error("flatgfa_bed_intersect: out of memory");  // (the one reason this sink stops)
    if (rc) {
        free(t.buf);
        return rc;
    }
    t.buf[t.at] = 0;
    *text = t.buf;
    *len = t.at;
    return FLATGFA_OK;
}

int flatgfa_bed_intersect_stream(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, flatgfa_sink_t sink, void *ctx) {
    if ((!a && a_len) || (!b && b_len) || !sink) { set_error("flatgfa_bed_intersect_stream: NULL argument"); return FLATGFA_ERR_ARG; }
    BedCall c;
    if (int rc = bed_open(a, a_len, b, b_len, &c)) return rc;
    return fgfa_dev::bed_emit(c.job, sink, ctx, nullptr);
}

int flatgfa_bed_intersect_count(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint64_t *lines, uint64_t *bytes,
                                uint64_t *candidates, uint64_t *unsorted_groups) {
    if ((!a && a_len) || (!b && b_len) || !lines || !bytes || !candidates || !unsorted_groups) {
        set_error("flatgfa_bed_intersect_count: NULL argument");
        return FLATGFA_ERR_ARG;
    }
    *lines = *bytes = *candidates = *unsorted_groups = 0;
    BedCall c;
    if (int rc = bed_open(a, a_len, b, b_len, &c)) return rc;
    fgfa_dev::BedTotals t;
    if (int rc = fgfa_dev::bed_count(c.job, &t)) return rc;
    *lines = t.lines, *bytes = t.bytes, *candidates = t.candidates, *unsorted_groups = t.unsorted_groups;
    return FLATGFA_OK;
}

}  // extern "C"
