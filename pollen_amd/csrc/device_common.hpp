// Shared between the C-ABI translation unit and the HIP translation unit.
#pragma once
#include <cstdlib>
#include <string>

// Environment variables reach this library in two kinds.  The handful a user may set -- FLATGFA_DEPTH_PATH, FLATGFA_MALL_MB,
// FLATGFA_PACKED, FLATGFA_BUCKET_GB, FLATGFA_UPLOAD_THREADS, FLATGFA_PARSE_THREADS, FLATGFA_TIMING, FLATGFA_CHECK_NO_CLAIM,
// FLATGFA_SHARD_FORCE_RCCL, FLATGFA_NO_WARM, FLATGFA_KEEP_HOST_MEMORY (the CLI and the Python package): INTEGRATION.md section 6 -- are read with getenv where they apply; none of them
// changes a result.  Everything else is a TEST HOOK: the parity suite forces every device path of the shipped library
// (tests/test_gpu_depth.py: `device_path`, tools/fuzz_gpu.py: ENVS) by shaping the plan -- piece sizes, window sizes, bucket
// capacities, which kernel walks which path -- and reads two diagnostics (FLATGFA_SCAN_TIME, FLATGFA_ACC_TIME).  They go through
// this one function so that they can be told apart (and found: `grep test_hook`); they change which kernels run, never
// what they count.
#ifndef FGFA_TEST_HOOK_DEFINED
#define FGFA_TEST_HOOK_DEFINED
inline const char *test_hook(const char *name) { return std::getenv(name); }
#endif

namespace fgfa_dev {
void set_error(const std::string &s);
const char *last_error();
}  // namespace fgfa_dev

// The one HIP check: where expr fails, "<prefix><expr>: <what HIP says>" becomes the thread's error and `fail_stmt` runs (a
// return, or a block that cleans up first).  For code that has HIP's runtime header and flatgfa.h before it: every user,
// host or device side.  FGFA_HIP_OR is the form without a prefix; FGFA_HIP returns FLATGFA_ERR_HIP.
#define FGFA_HIP_CHECK(prefix, expr, fail_stmt)                                                   \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            fgfa_dev::set_error(std::string(prefix) + #expr + ": " + hipGetErrorString(_e));      \
            fail_stmt;                                                                            \
        }                                                                                         \
    } while (0)
#define FGFA_HIP_OR(expr, fail_stmt) FGFA_HIP_CHECK("", expr, fail_stmt)
#define FGFA_HIP(prefix, expr) FGFA_HIP_CHECK(prefix, expr, return FLATGFA_ERR_HIP)

// The calling thread's current device is its own business: whatever an entry point switches to, it switches back.  Saves
// the current device when it is made and restores it when it goes; switch_to leaves a device that is current already alone.
namespace fgfa_dev {
struct DeviceGuard {
    int dev = -1;
    DeviceGuard() { if (hipGetDevice(&dev) != hipSuccess) dev = -1; }
    ~DeviceGuard() { if (dev >= 0) (void)hipSetDevice(dev); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
    bool switch_to(int device) {
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur == device) return true;
        return hipSetDevice(device) == hipSuccess;
    }
};
}  // namespace fgfa_dev

// An empty launch on `stream`: what makes the runtime load this library's code object (flatgfa_warm_device).
namespace fgfa_dev {
void warm_launch(void *stream);
}
