// Runs the pieces of pollen_amd/csrc/device_scan.hpp on their own, away from the four features built on them (chop, GAF
// lookup, extract / position, validate / degree), so that a failing feature test can be told from a failing scan.
// `make -C pollen_amd/csrc scan_check` builds it for gfx950; tests/test_gpu_device_scan.py drives it.
//
//   scan_check MANIFEST      one case per line: KIND POINT N INPUT OUTPUT.  Every case runs in this one process on one stream;
//                            INPUT and OUTPUT are raw little-endian arrays (layouts below, restated in
//                            tests/device_scan_cases.py).  The program judges nothing: it writes what the device code left
//                            and exits 0.  A HIP call that fails, or a manifest or input that does not hold what its kind
//                            needs, is printed and ends the program at once with a non-zero status.
//
// Every output array has `guard` elements behind what the case may write, filled with 0xA5 bytes before the launch and written
// back with the rest: a store past the end shows as a changed byte.
//
//   KIND        POINT          INPUT                                          OUTPUT (guard)
//   sum32       kThreads x kPer  u32[n]                                       u32[n + tile] scanned in place, u64 total
//   sum64       kThreads x kPer  u64[n]                                       u64[n + tile], u64 total
//   affine      kThreads x kPer  {u64 a, b}[n]                                {u64 a, b}[n + tile], {u64 a, b} total
//   block_excl  u32|u64 x kThreads  T[2 kThreads]: the lanes' values of two calls   T[5 kThreads]: results 1, results 2, totals 1, totals 2 (per lane), guard
//   wave        -              u64[512]: 256 values, 256 source lanes         u64[6 * 256]: wave_sum, wave_incl_scan, shfl_u64 from lane 0, from
//                                                                             lane 63, from the lane's source lane, guard
//   last_start  -              u64[3 + m + n]: m, lo, hi, pstart[m], j[n]      u32[n + 256]
//   check_links -              u32[3 + 4n]: n_segs, bit, flags before, links  u32[1 + 256]: flags after
//   blocks      -              u64[3n]: n, per, max_grid                      u64[2n]: blocks, stride_blocks (host only)
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

#ifndef SCAN_HEADER
#define SCAN_HEADER "../../pollen_amd/csrc/device_scan.hpp"
#endif
#include SCAN_HEADER

namespace fgfa_dev {
void set_error(const std::string &s) { std::fprintf(stderr, "scan_check: %s\n", s.c_str()); }
}  // namespace fgfa_dev

using namespace fgfa_dev;

[[noreturn]] static void fail(const std::string &what) {
    std::fprintf(stderr, "scan_check: %s\n", what.c_str());
    std::exit(1);
}
#define CK(expr)                                                                      \
    do {                                                                              \
        hipError_t _e = (expr);                                                       \
        if (_e != hipSuccess) fail(std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

namespace {

constexpr uint8_t kGuardByte = 0xA5;
constexpr uint64_t kMaxN = 1ull << 23;  // (no case comes near: a manifest that asks for more is a mistake)

struct P2 {
    uint64_t a, b;
};
// x -> a * x + b over u64; comb(x, y) is "x, then y"
struct Aff {
    using Carry = P2;
    using Wide = Aff;
    uint64_t a, b;
    __device__ __forceinline__ static Aff zero() { return Aff{1, 0}; }
    __device__ __forceinline__ static Aff comb(const Aff &x, const Aff &y) { return Aff{y.a * x.a, y.a * x.b + y.b}; }
    __device__ __forceinline__ P2 carry() const { return P2{a, b}; }
    __device__ __forceinline__ static Aff widen(const Aff &x) { return x; }
    __device__ __forceinline__ static Aff after(const P2 &c) { return Aff{c.a, c.b}; }
};

struct RowOp {  // in place, as topology's
    uint32_t *data;
    __device__ Sum<uint32_t> load(uint64_t i) const { return Sum<uint32_t>{data[i]}; }
    __device__ void store(uint64_t i, uint32_t before, const Sum<uint32_t> &) const { data[i] = before; }
};
struct WideOp {
    const uint64_t *in;
    uint64_t *out;
    __device__ Sum<uint64_t> load(uint64_t i) const { return Sum<uint64_t>{in[i]}; }
    __device__ void store(uint64_t i, uint64_t before, const Sum<uint64_t> &) const { out[i] = before; }
};
struct AffOp {
    const P2 *in;
    P2 *out;
    __device__ Aff load(uint64_t i) const { return Aff{in[i].a, in[i].b}; }
    __device__ void store(uint64_t i, const P2 &before, const Aff &) const { out[i] = before; }
};

template <class T, int kThreads>
__global__ __launch_bounds__(kThreads) void k_block_excl(const T *__restrict__ in, T *__restrict__ out) {
    const uint32_t t = threadIdx.x;
    T tot1, tot2;
    const T r1 = block_excl_scan<T, kThreads>(in[t], &tot1);
    const T r2 = block_excl_scan<T, kThreads>(in[kThreads + t], &tot2);
    out[t] = r1;
    out[kThreads + t] = r2;
    out[2 * kThreads + t] = tot1;
    out[3 * kThreads + t] = tot2;
}

constexpr int kWaveThreads = 256;  // four waves
__global__ __launch_bounds__(kWaveThreads) void k_wave(const uint64_t *__restrict__ in, uint64_t *__restrict__ out) {
    const uint32_t t = threadIdx.x;
    const uint64_t v = in[t];
    const int src = (int)(in[kWaveThreads + t] & 63);
    out[t] = wave_sum(v);
    out[kWaveThreads + t] = wave_incl_scan(v, (int)(t & 63));
    out[2 * kWaveThreads + t] = shfl_u64(v, 0);
    out[3 * kWaveThreads + t] = shfl_u64(v, 63);
    out[4 * kWaveThreads + t] = shfl_u64(v, src);
}

__global__ __launch_bounds__(256) void k_last_start(const uint32_t *__restrict__ pstart, uint32_t lo, uint32_t hi, const uint64_t *__restrict__ j,
                                                    uint64_t n, uint32_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = last_start_at_or_before(pstart, lo, hi, j[i]);
}

std::string read_file(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) fail("cannot read " + path);
    return std::string((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

struct Out {
    std::ofstream f;
    explicit Out(const std::string &path) : f(path, std::ios::binary) {
        if (!f) fail("cannot write " + path);
    }
    void put(const void *p, size_t bytes) { f.write((const char *)p, (std::streamsize)bytes); }
    void done(const std::string &path) {
        f.close();
        if (!f) fail("write failed: " + path);
    }
};

// a device array of `count` elements behind which `guard` more are filled with the guard byte
template <class T>
struct Guarded {
    T *d = nullptr;
    uint64_t count, guard;
    Guarded(uint64_t count_, uint64_t guard_, hipStream_t st) : count(count_), guard(guard_) {
        CK(hipMalloc((void **)&d, (count + guard) * sizeof(T)));
        CK(hipMemsetAsync(d, kGuardByte, (count + guard) * sizeof(T), st));
    }
    Guarded(const Guarded &) = delete;
    Guarded &operator=(const Guarded &) = delete;
    ~Guarded() { (void)hipFree(d); }
    void upload(const void *src, uint64_t n, hipStream_t st) {
        if (n > count) fail("internal: upload past the array");
        if (n) CK(hipMemcpyAsync(d, src, n * sizeof(T), hipMemcpyHostToDevice, st));
    }
    void write_back(Out *o, hipStream_t st) {
        std::vector<T> h(count + guard);
        CK(hipMemcpyAsync(h.data(), d, (count + guard) * sizeof(T), hipMemcpyDeviceToHost, st));
        CK(hipStreamSynchronize(st));
        o->put(h.data(), h.size() * sizeof(T));
    }
};

template <class T>
void put_scalar(Out *o, const T *d, hipStream_t st) {
    T h;
    CK(hipMemcpyAsync(&h, d, sizeof(T), hipMemcpyDeviceToHost, st));
    CK(hipStreamSynchronize(st));
    o->put(&h, sizeof(T));
}

// scan_count, scan_apply over n elements; the output array and the total
template <int kThreads, uint32_t kPer, class V, class E, class MakeOp>
void tiled(const std::string &in, uint64_t n, Out *o, hipStream_t st, MakeOp make_op, bool in_place) {
    constexpr uint64_t tile = (uint64_t)kThreads * kPer;
    if (in.size() != n * sizeof(E)) fail("input size does not match n");
    Guarded<E> out(n, tile, st);
    E *d_in = nullptr;
    if (in_place) out.upload(in.data(), n, st);
    else {
        CK(hipMalloc((void **)&d_in, (n ? n : 1) * sizeof(E)));
        if (n) CK(hipMemcpyAsync(d_in, in.data(), n * sizeof(E), hipMemcpyHostToDevice, st));
    }
    {
        DeviceMem mem;
        mem.st = st;
        Spine<V> sp;
        CK(sp.alloc(&mem, blocks(n, tile)));
        const auto op = make_op(d_in, out.d);
        scan_count<kThreads, kPer>(op, n, sp, st);
        CK(hipGetLastError());
        scan_apply<kThreads, kPer>(op, n, sp, st);
        CK(hipGetLastError());
        CK(hipStreamSynchronize(st));
        out.write_back(o, st);
        put_scalar(o, sp.total, st);
    }
    if (d_in) CK(hipFree(d_in));
}

template <int kThreads, uint32_t kPer>
void tiled_kind(const std::string &kind, const std::string &in, uint64_t n, Out *o, hipStream_t st) {
    if (kind == "sum32")
        tiled<kThreads, kPer, Sum<uint32_t>, uint32_t>(in, n, o, st, [](uint32_t *, uint32_t *out) { return RowOp{out}; }, true);
    else if (kind == "sum64")
        tiled<kThreads, kPer, Sum<uint64_t>, uint64_t>(in, n, o, st, [](uint64_t *src, uint64_t *out) { return WideOp{src, out}; }, false);
    else
        tiled<kThreads, kPer, Aff, P2>(in, n, o, st, [](P2 *src, P2 *out) { return AffOp{src, out}; }, false);
}

template <class T, int kThreads>
void block_excl(const std::string &in, Out *o, hipStream_t st) {
    if (in.size() != 2 * kThreads * sizeof(T)) fail("block_excl: the input is not two values per lane");
    Guarded<T> src(2 * kThreads, 0, st), out(4 * kThreads, kThreads, st);
    src.upload(in.data(), 2 * kThreads, st);
    hipLaunchKernelGGL((k_block_excl<T, kThreads>), dim3(1), dim3(kThreads), 0, st, src.d, out.d);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(st));
    out.write_back(o, st);
}

template <class T>
void block_excl_threads(int threads, const std::string &in, Out *o, hipStream_t st) {
    if (threads == 64) block_excl<T, 64>(in, o, st);
    else if (threads == 256) block_excl<T, 256>(in, o, st);
    else if (threads == 1024) block_excl<T, 1024>(in, o, st);
    else fail("block_excl: no such point");
}

void wave(const std::string &in, Out *o, hipStream_t st) {
    if (in.size() != 2 * kWaveThreads * 8) fail("wave: the input is not a value and a source lane per lane");
    Guarded<uint64_t> src(2 * kWaveThreads, 0, st), out(5 * kWaveThreads, kWaveThreads, st);
    src.upload(in.data(), 2 * kWaveThreads, st);
    hipLaunchKernelGGL(k_wave, dim3(1), dim3(kWaveThreads), 0, st, src.d, out.d);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(st));
    out.write_back(o, st);
}

void last_start(const std::string &in, uint64_t n, Out *o, hipStream_t st) {
    if (in.size() < 24 || in.size() % 8) fail("last_start: short input");
    const uint64_t *w = (const uint64_t *)in.data();
    const uint64_t m = w[0], lo = w[1], hi = w[2];
    if (!m || m > kMaxN || in.size() != (3 + m + n) * 8 || lo > hi || hi >= m) fail("last_start: the input does not hold m, lo <= hi < m, pstart[m], j[n]");
    std::vector<uint32_t> ps(m);
    for (uint64_t k = 0; k < m; ++k) {
        if (w[3 + k] > 0xFFFFFFFFull) fail("last_start: a start past 32 bits");
        ps[k] = (uint32_t)w[3 + k];
    }
    Guarded<uint32_t> pstart(m, 0, st), out(n, 256, st);
    Guarded<uint64_t> j(n ? n : 1, 0, st);
    pstart.upload(ps.data(), m, st);
    j.upload(w + 3 + m, n, st);
    if (n) hipLaunchKernelGGL(k_last_start, dim3((uint32_t)blocks(n, 256)), dim3(256), 0, st, pstart.d, (uint32_t)lo, (uint32_t)hi, j.d, n, out.d);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(st));
    out.write_back(o, st);
}

void check_links(const std::string &in, uint64_t n, Out *o, hipStream_t st) {
    if (in.size() != (3 + 4 * n) * 4) fail("check_links: the input does not hold n_segs, bit, flags, links[4 n]");
    const uint32_t *w = (const uint32_t *)in.data();
    Guarded<uint32_t> links(n ? 4 * n : 1, 0, st), flags(1, 256, st);
    links.upload(w + 3, 4 * n, st);
    flags.upload(w + 2, 1, st);
    if (n) hipLaunchKernelGGL(k_check_links<256>, dim3((uint32_t)blocks(n, 256)), dim3(256), 0, st, links.d, n, w[0], flags.d, w[1]);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(st));
    flags.write_back(o, st);
}

// host only
void host_blocks(const std::string &in, uint64_t n, Out *o) {
    if (in.size() != n * 24) fail("blocks: the input does not hold n, per, max_grid per case");
    const uint64_t *w = (const uint64_t *)in.data();
    for (uint64_t k = 0; k < n; ++k) {
        if (!w[3 * k + 1] || w[3 * k + 2] > 0xFFFFFFFFull) fail("blocks: per is 0 or max_grid past 32 bits");
        const uint64_t r[2] = {blocks(w[3 * k], w[3 * k + 1]), stride_blocks(w[3 * k], w[3 * k + 1], (uint32_t)w[3 * k + 2])};
        o->put(r, sizeof r);
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) fail("usage: scan_check MANIFEST");
    std::istringstream manifest(read_file(argv[1]));
    hipStream_t st = nullptr;
    std::string line;
    int done = 0;
    while (std::getline(manifest, line)) {
        if (line.empty()) continue;
        std::istringstream ls(line);
        std::string kind, point, in_path, out_path;
        uint64_t n = 0;
        if (!(ls >> kind >> point >> n >> in_path >> out_path) || n > kMaxN) fail("bad manifest line: " + line);
        const std::string in = read_file(in_path);
        Out o(out_path);
        if (kind == "blocks") {
            host_blocks(in, n, &o);
        } else {
            if (!st) CK(hipStreamCreate(&st));  // (the host-only kind needs no device)
            if (kind == "sum32" || kind == "sum64" || kind == "affine") {
                if (point == "256x4") tiled_kind<256, 4>(kind, in, n, &o, st);
                else if (point == "256x8") tiled_kind<256, 8>(kind, in, n, &o, st);
                else if (point == "64x1") tiled_kind<64, 1>(kind, in, n, &o, st);
                else if (point == "1024x2") tiled_kind<1024, 2>(kind, in, n, &o, st);
                else fail("no such point: " + line);
            } else if (kind == "block_excl") {
                if (point.compare(0, 4, "u32x") == 0) block_excl_threads<uint32_t>(std::atoi(point.c_str() + 4), in, &o, st);
                else if (point.compare(0, 4, "u64x") == 0) block_excl_threads<uint64_t>(std::atoi(point.c_str() + 4), in, &o, st);
                else fail("no such point: " + line);
            } else if (kind == "wave") {
                wave(in, &o, st);
            } else if (kind == "last_start") {
                last_start(in, n, &o, st);
            } else if (kind == "check_links") {
                check_links(in, n, &o, st);
            } else {
                fail("no such kind: " + line);
            }
        }
        o.done(out_path);
        ++done;
    }
    if (st) {
        CK(hipStreamSynchronize(st));
        CK(hipStreamDestroy(st));
    }
    std::printf("scan_check: %d cases\n", done);
    return 0;
}
