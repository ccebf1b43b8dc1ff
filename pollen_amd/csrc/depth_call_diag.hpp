// The diagnostics of a bucketed node-depth call (depth_fast.hip: run_range): each takes its buffer when its hook is set, reports
// to stderr behind the call's launches (the stream drained first), and frees the buffer on every way out of the call.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "depth_fast_kernels.hpp"
#include "host_copy.hpp"

namespace fgfa_dev {

struct ScanTimeDiag {  // FLATGFA_SCAN_TIME: when the workgroups of k_scan start, when their first wave runs out of work, when they end
    unsigned long long *buf = nullptr;
    const char *const where;
    const size_t n;
    ScanTimeDiag(const char *hook, uint32_t n_slots) : where(hook), n(kTprofRow * (size_t)n_slots) {
        if (!hook) return;
        if (hipMalloc(&buf, n * 8) == hipSuccess) (void)hipMemset(buf, 0, n * 8);
        else buf = nullptr;
    }
    ScanTimeDiag(const ScanTimeDiag &) = delete;
    ~ScanTimeDiag() { if (buf) (void)hipFree(buf); }
    void report(uint32_t grid, bool tagged, hipStream_t stream) const {
        if (!buf) return;
        constexpr size_t kRow = kTprofRow;
        std::vector<unsigned long long> raw(n);
        (void)hipStreamSynchronize(stream);
        (void)staged_copy(raw.data(), buf, raw.size() * 8, hipMemcpyDeviceToHost, nullptr);
        unsigned long long t0 = ~0ull;
        for (uint32_t i = 0; i < grid; ++i) t0 = std::min(t0, raw[kRow * i]);
        std::vector<double> st, fw, lw, en;
        for (uint32_t i = 0; i < grid; ++i) {
            st.push_back((raw[kRow * i] - t0) / 100.0);
            en.push_back((raw[kRow * i + 1] - t0) / 100.0);
            unsigned long long a = ~0ull, b = 0;
            for (size_t k = 0; k < kWaves; ++k) {
                a = std::min(a, raw[kRow * i + 4 + k]);
                b = std::max(b, raw[kRow * i + 4 + k]);
            }
            fw.push_back((a - t0) / 100.0);
            lw.push_back((b - t0) / 100.0);
        }
        const auto pct = [](std::vector<double> v, double q) { std::sort(v.begin(), v.end()); return v[(size_t)(q * (v.size() - 1))]; };
        fprintf(stderr, "k_scan%s workgroups (us since the first one started): start p50 %.1f max %.1f | first wave out of work p5 %.1f p50 %.1f p95 %.1f | last wave p5 %.1f p50 %.1f p95 %.1f max %.1f | end p50 %.1f max %.1f\n",
                tagged ? " [tagged]" : "", pct(st, 0.5), pct(st, 1.0), pct(fw, 0.05), pct(fw, 0.5), pct(fw, 0.95), pct(lw, 0.05), pct(lw, 0.5), pct(lw, 0.95), pct(lw, 1.0), pct(en, 0.5), pct(en, 1.0));
        // FLATGFA_SCAN_TIME=<file>: one line per workgroup and call -- call, workgroup, XCC, HW_ID, items, start, first / last wave out of work, end (us)
        static int call_no = 0;
        if (strchr(where, '/')) {
            if (FILE *f = fopen(where, "a")) {
                for (uint32_t i = 0; i < grid; ++i)
                    fprintf(f, "%d,%u,%u,0x%08x,%u,%.2f,%.2f,%.2f,%.2f\n", call_no, i, (unsigned)(raw[kRow * i + 2] >> 32) & 15u, (unsigned)raw[kRow * i + 2],
                            (unsigned)raw[kRow * i + 3], st[i], fw[i], lw[i], en[i]);
                fclose(f);
            }
        }
        call_no += 1;
    }
};
struct AccTimeDiag {  // FLATGFA_ACC_TIME: where the waves of pass 2 spend their time
    uint32_t *buf = nullptr;
    const size_t words;
    AccTimeDiag(bool on, size_t words_) : words(words_) {
        if (on && hipMalloc(&buf, words * 4) != hipSuccess) buf = nullptr;
    }
    AccTimeDiag(const AccTimeDiag &) = delete;
    ~AccTimeDiag() { if (buf) (void)hipFree(buf); }
    void report(bool tagged, hipStream_t stream) const {
        if (!buf) return;
        std::vector<uint32_t> raw(words);
        (void)hipStreamSynchronize(stream);
        (void)staged_copy(raw.data(), buf, words * 4, hipMemcpyDeviceToHost, nullptr);
        const size_t waves = words / 16;
        double sum[16] = {}, mx[16] = {};
        for (size_t w = 0; w < waves; ++w)
            for (int k = 0; k < 16; ++k) {
                sum[k] += raw[w * 16 + k];
                mx[k] = std::max<double>(mx[k], raw[w * 16 + k]);
            }
        static const char *names[5] = {"setup", "flat", "walk", "barrier", "scan+store"};
        fprintf(stderr, "k_accum%s per wave, us avg (max):", tagged ? " [tagged]" : "");
        for (int k = 0; k < 5; ++k) fprintf(stderr, "  %s %.2f (%.2f)", names[k], sum[k] / waves / 100.0, mx[k] / 100.0);
        fprintf(stderr, "  | per wave avg (max): steps %.1f (%.0f) rounds %.1f flushes %.1f (%.0f)\n", sum[8] / waves, mx[8], sum[9] / waves, sum[10] / waves, mx[10]);
    }
};
// kDbgTime (measurement builds): where the waves of k_scan spend their cycles -- read from the status words, nothing to hold
inline void report_scan_cycles(uint32_t *status, uint32_t grid, hipStream_t stream) {
    unsigned long long acc[8] = {};
    (void)hipStreamSynchronize(stream);
    (void)staged_copy(acc, status + 8, sizeof acc, hipMemcpyDeviceToHost, nullptr);
    (void)hipMemset(status + 8, 0, sizeof acc);
    const double waves = (double)grid * kWaves;
    fprintf(stderr, "k_scan cycles per wave: wait_block %.0f  epoch_wait %.0f  passA+B %.0f  drain %.0f  other %.0f  item switch %.0f\n",
            acc[0] / waves, acc[1] / waves, acc[2] / waves, acc[3] / waves, acc[4] / waves, acc[5] / waves);
}

}  // namespace fgfa_dev
