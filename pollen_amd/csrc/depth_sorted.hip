// The sorted record image of a bucketed depth plan (DESIGN.md sections 3.2, 3.3; depth_sorted_host.hpp): the records
// k_scan_runs makes of the plan's items, made once more with k_run_room's arithmetic, as (key, record) pairs -- key = window |
// path | window-relative start --, sorted by rocprim's merge sort (depth_sorted_sort.hip, which says why not the radix sort),
// and finalised into chunks of kSortedChunk records that k_accum_sorted sweeps in any order.  An index, never an answer: the
// same intervals in another order; every depth update and every revisit decision is made in every call.  Plain HIP; no
// kernel of the build uses scratch memory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "depth_fast_kernels.hpp"
#include "depth_sorted.hpp"
#include "depth_sorted_host.hpp"
#include "device_scan.hpp"
#include "host_copy.hpp"
#include "prof.hpp"

namespace fgfa_dev {

struct SortedImage {
    // what the plan keeps
    uint32_t *rec = nullptr;        // [n_chunks * kSortedChunk]
    uint32_t *carry = nullptr;      // [n_chunks]
    uint32_t *win_chunk = nullptr;  // [n_win + 1]
    // while it is being made
    uint32_t *cnt = nullptr;        // [n_win] records per window; [n_win]: records dropped for bounds; [n_win + 1]: pairs emitted; [n_win + 2]: a pair in the wrong window;
                                    // [n_win + 3], [n_win + 4]: the most records that start at one cell of one window, and that end at one
    uint32_t *rec_off = nullptr;    // [n_win + 1]
    uint64_t *keys = nullptr;       // [2 n]: in, out
    uint32_t *recs = nullptr;       // [2 n]
    void *scratch = nullptr;
    uint32_t n_win = 0;
    SortedKey key;
    SortedLayout lay;
    uint64_t transient = 0;
    uint32_t cell_max[2] = {0u, 0u};  // (sorted_image_cell_max; 0: not known)
    hipEvent_t done = nullptr;
    int phase = 0;                  // 1: counted (enqueued), 2: emitted, sorted, finalised (enqueued), 3: there, -1: not to be had
    const char *why = "";
};

namespace {

constexpr uint32_t kSortedHistWindows = 8192;  // windows the counting kernel counts in LDS (32 KB)

// One record (two where the run crosses a window's edge) per entry of the item's stretch of the run image, clipped to the item's
// steps [b, e): k_run_room's arithmetic, which is emit_chunk's.  fn(window, window-relative start, length - 1); returns false
// where the record is dropped for bounds.
template <class Fn>
__device__ __forceinline__ bool sorted_records_of(const uint2 *__restrict__ ent, uint32_t i, const uint4 &d, uint32_t n_segs, uint32_t wb, Fn fn) {
    const uint32_t wmask = (1u << wb) - 1u;
    const uint2 en = ent[i];
    const uint32_t s = max(en.y, d.x), t = min(ent[i + 1u].y, d.y);
    if (s >= t) return true;
    const uint32_t skip = s - en.y, lenm1 = t - s - 1u;
    const bool dn = (en.x >> 31) != 0u;
    const uint32_t first = (en.x & 0x7FFFFFFFu) + (dn ? 0u - skip : skip);
    const uint32_t id = dn ? first - lenm1 : first;
    if (id + lenm1 >= n_segs || id + lenm1 < id) return false;
    const uint32_t win = id >> wb, rel = id & wmask;
    if (rel + lenm1 > wmask) {
        fn(win, rel, wmask - rel);
        fn(win + 1u, 0u, lenm1 - (wmask - rel) - 1u);
    } else {
        fn(win, rel, lenm1);
    }
    return true;
}

__global__ __launch_bounds__(256) void sorted_image_count(const uint4 *__restrict__ items, const uint2 *__restrict__ item_ent, uint32_t n_items,
                                                           const uint2 *__restrict__ ent, uint32_t n_segs, uint32_t wb, uint32_t n_win, uint32_t *__restrict__ cnt) {
    // (a few hundred windows take millions of records: counted in LDS per workgroup where the windows fit it -- straight into
    // memory the same kernel took forty times as long at cfg-L)
    __shared__ uint32_t hist[kSortedHistWindows];
    const bool local = n_win <= kSortedHistWindows;
    for (uint32_t w = threadIdx.x; local && w < n_win; w += 256u) hist[w] = 0u;
    __syncthreads();
    for (uint32_t j = blockIdx.x; j < n_items; j += gridDim.x) {
        const uint4 d = items[j];
        const uint2 er = item_ent[j];
        for (uint32_t i = er.x + threadIdx.x; i < er.y; i += 256u) {
            const bool ok = sorted_records_of(ent, i, d, n_segs, wb, [&](uint32_t win, uint32_t, uint32_t) {
                if (win >= n_win) return;
                if (local) atomicAdd(&hist[win], 1u);
                else atomicAdd(&cnt[win], 1u);
            });
            if (!ok) atomicAdd(&cnt[n_win], 1u);
        }
    }
    __syncthreads();
    for (uint32_t w = threadIdx.x; local && w < n_win; w += 256u)
        if (hist[w]) atomicAdd(&cnt[w], hist[w]);
}

__global__ __launch_bounds__(256) void sorted_image_emit(const uint4 *__restrict__ items, const uint2 *__restrict__ item_ent, uint32_t n_items,
                                                          const uint2 *__restrict__ ent, uint32_t n_segs, const SortedKey key, uint32_t n_win,
                                                          uint32_t n_records, uint32_t *__restrict__ cursor, uint64_t *__restrict__ keys, uint32_t *__restrict__ recs) {
    const uint32_t wb = key.wb;
    for (uint32_t j = blockIdx.x; j < n_items; j += gridDim.x) {
        const uint4 d = items[j];
        const uint2 er = item_ent[j];
        const uint32_t path = d.w & (uint32_t)((1ull << key.path_bits) - 1ull);
        for (uint32_t i = er.x + threadIdx.x; i < er.y; i += 256u) {
            (void)sorted_records_of(ent, i, d, n_segs, wb, [&](uint32_t win, uint32_t rel, uint32_t lenm1) {
                if (win >= n_win) return;
                const uint32_t at = atomicAdd(cursor, 1u);
                if (at >= n_records) return;  // (the steps changed behind the count: the finaliser sees the cursor and the image is not installed)
                keys[at] = key.pack(win, path, rel);
                recs[at] = rel | (lenm1 << wb);
            });
        }
    }
}

// One wave per window walks the window's sorted pairs a chunk at a time: the first record of every path gets its flag, every
// record the ordinal of its path among its chunk's records (kSortedOrdShift: what the sweep's keys are made of), the
// window is padded to whole chunks, and every chunk gets its carry word -- the largest end among the earlier records, in this
// window, of the path the chunk begins with; 0 where the chunk begins a path.
__global__ __launch_bounds__(64) void sorted_image_finalise(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ recs, const uint32_t *__restrict__ rec_off,
                                                            const uint32_t *__restrict__ win_chunk, uint32_t n_win, const SortedKey sk,
                                                            uint32_t *__restrict__ img, uint32_t *__restrict__ carry, uint32_t *__restrict__ wrong) {
    static_assert(kSortedChunk == 64u, "one record per lane and chunk");
    const int lane = threadIdx.x;
    const uint32_t wb = sk.wb, wmask = (1u << wb) - 1u;
    for (uint32_t w = blockIdx.x; w < n_win; w += gridDim.x) {
        const uint32_t off = rec_off[w], cnt = rec_off[w + 1u] - off, c0 = win_chunk[w], nc = win_chunk[w + 1u] - c0;
        uint32_t carry_m = 0u, carry_path = 0u;
        for (uint32_t c = 0; c < nc; ++c) {
            const uint32_t k = c * kSortedChunk + (uint32_t)lane;
            const bool have = k < cnt;
            const uint64_t key = have ? keys[off + k] : 0ull;
            const uint32_t rec = have ? recs[off + k] : 0u;
            if (have && sk.win(key) != w) atomicOr(wrong, 1u);
            const uint32_t path = sk.path(key);
            const uint32_t up = (uint32_t)__shfl_up((int)path, 1, 64);
            const uint32_t prev = lane == 0 ? carry_path : up;
            const bool first = have && (k == 0u || path != prev);
            const unsigned long long fm = __builtin_amdgcn_ballot_w64(first);
            const uint32_t ord = (uint32_t)__builtin_popcountll(fm & (~0ull >> (63 - lane)));
            const uint32_t e = (rec & wmask) + ((rec >> wb) & 1023u) + 1u;
            const uint32_t incl = wave_scan_max(have ? (ord << kSortedEndBits) | e : 0u);
            // (the record carries its path's ordinal in its chunk, so the sweep reads it and does not count flags: an index, as the flag is)
            img[(size_t)(c0 + c) * kSortedChunk + lane] = have ? rec | (first ? kSortedFirst : 0u) | (ord << kSortedOrdShift) : kSortedPad;
            if (lane == 0) carry[c0 + c] = first ? 0u : carry_m;
            // what the next chunk starts from: the last record's path, and the largest end of that path's records so far
            const uint32_t last = min(cnt - c * kSortedChunk, kSortedChunk) - 1u;
            const uint32_t incl_l = __builtin_amdgcn_readlane(incl, last), ord_l = __builtin_amdgcn_readlane(ord, last);
            const uint32_t m = incl_l & ((1u << kSortedEndBits) - 1u);
            carry_m = ord_l == 0u ? max(carry_m, m) : m;
            carry_path = __builtin_amdgcn_readlane(path, last);
        }
    }
}

// The bound the sweep's packed cells rest on (depth_sorted_host.hpp, sorted_cells_fit): one workgroup per window counts, over the
// window's finished chunks, the records that start at every cell and then those that end at every cell, and the largest of each
// goes out.  A histogram maximum of the image; nothing of it reaches a result.
constexpr uint32_t kSortedMaxWb = 13;
__global__ __launch_bounds__(256) void sorted_image_cell_max(const uint32_t *__restrict__ img, const uint32_t *__restrict__ win_chunk, uint32_t wb, uint32_t *__restrict__ out) {
    __shared__ uint32_t hist[(1u << kSortedMaxWb) + 1u];
    __shared__ uint32_t top;
    const uint32_t w = blockIdx.x, wmask = (1u << wb) - 1u, n_cells = (1u << wb) + 1u;  // (wb <= kSortedMaxWb: the host's business)
    const uint32_t r0 = win_chunk[w] * kSortedChunk, r1 = win_chunk[w + 1u] * kSortedChunk;
    for (uint32_t pass = 0; pass < 2u; ++pass) {
        for (uint32_t i = threadIdx.x; i < n_cells; i += 256u) hist[i] = 0u;
        if (threadIdx.x == 0) top = 0u;
        __syncthreads();
        for (uint32_t i = r0 + threadIdx.x; i < r1; i += 256u) {
            const uint32_t rec = img[i];
            const uint32_t s = rec & wmask, cell = pass ? s + ((rec >> wb) & 1023u) + 1u : s;
            if (!(rec & kSortedPad) && cell < n_cells) atomicAdd(&hist[cell], 1u);
        }
        __syncthreads();
        uint32_t m = 0u;
        for (uint32_t i = threadIdx.x; i < n_cells; i += 256u) m = max(m, hist[i]);
        if (m) atomicMax(&top, m);
        __syncthreads();
        if (threadIdx.x == 0 && top) atomicMax(&out[pass], top);
        __syncthreads();
    }
}

void sorted_release_scratch(SortedImage *si) {
    for (void **p : {(void **)&si->cnt, (void **)&si->rec_off, (void **)&si->keys, (void **)&si->recs, &si->scratch}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
}

int sorted_fail(SortedImage *si, const char *why) {
    (void)hipGetLastError();
    sorted_release_scratch(si);
    for (void **p : {(void **)&si->rec, (void **)&si->carry, (void **)&si->win_chunk}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    si->phase = -1;
    si->why = why;
    return -1;
}

}  // namespace

SortedImage *sorted_image_start(const FastPlan &fp, uint32_t n_paths, hipStream_t side) {
    auto *si = new SortedImage();
    si->n_win = fp.n_win;
    si->key = sorted_key(fp.wb, n_paths, fp.n_win);
    if (!fp.run_ent || !fp.run_item_ent || !fp.n_items || !fp.n_win) {
        sorted_fail(si, "error");
        return si;
    }
    if (si->key.bits() > 64) {
        sorted_fail(si, "size");
        return si;
    }
    const size_t cnt_bytes = ((size_t)fp.n_win + 5) * 4;
    if (hipMalloc(&si->cnt, cnt_bytes) != hipSuccess || hipEventCreateWithFlags(&si->done, hipEventDisableTiming) != hipSuccess) {
        sorted_fail(si, "memory");
        return si;
    }
    {
        ProfScope ps("sorted_image_count", side);
        if (hipMemsetAsync(si->cnt, 0, cnt_bytes, side) != hipSuccess) {
            sorted_fail(si, "error");
            return si;
        }
        hipLaunchKernelGGL(sorted_image_count, dim3(std::min<uint32_t>(fp.n_items, fp.n_cus * 8u)), dim3(256), 0, side, reinterpret_cast<const uint4 *>(fp.items),
                           reinterpret_cast<const uint2 *>(fp.run_item_ent), fp.n_items, reinterpret_cast<const uint2 *>(fp.run_ent), fp.n_range, fp.wb, fp.n_win, si->cnt);
    }
    if (hipEventRecord(si->done, side) != hipSuccess || hipGetLastError() != hipSuccess) {
        (void)hipStreamSynchronize(side);
        sorted_fail(si, "error");
        return si;
    }
    si->phase = 1;
    return si;
}

int sorted_image_poll(SortedImage *si, const FastPlan &fp, hipStream_t side, bool wait, uint64_t reserve, bool waived) {
    for (;;) {
        if (si->phase == 3) return 1;
        if (si->phase < 1) return -1;
        if (wait) {
            if (hipEventSynchronize(si->done) != hipSuccess) return sorted_fail(si, "error");
        } else if (hipEventQuery(si->done) != hipSuccess) {
            (void)hipGetLastError();
            return 0;
        }
        if (si->phase == 2) {
            uint32_t end[4] = {0u, 1u, 0u, 0u};  // pairs emitted; a pair in the wrong window; the most starts at a cell, the most ends
            if (staged_copy(end, si->cnt + si->n_win + 1, 16, hipMemcpyDeviceToHost, nullptr) != hipSuccess) return sorted_fail(si, "error");
            if (end[0] != si->lay.n_records || end[1]) return sorted_fail(si, "stale");  // (the steps changed while it was made)
            si->cell_max[0] = end[2];
            si->cell_max[1] = end[3];
            sorted_release_scratch(si);
            si->phase = 3;
            return 1;
        }
        // counted: the layout, what it takes, and whether that is to be had
        std::vector<uint32_t> cnt((size_t)si->n_win + 1);
        if (staged_copy(cnt.data(), si->cnt, cnt.size() * 4, hipMemcpyDeviceToHost, nullptr) != hipSuccess) return sorted_fail(si, "error");
        if (cnt[si->n_win]) return sorted_fail(si, "bounds");  // (pass 1 has an error to raise: the calls keep running it)
        si->lay = sorted_layout(cnt.data(), si->n_win);
        if (!si->lay.fits || !si->lay.n_records) return sorted_fail(si, "size");
        const uint32_t n = (uint32_t)si->lay.n_records;
        size_t scratch_bytes = 0;
        if (!sorted_sort_pairs(nullptr, &scratch_bytes, nullptr, nullptr, nullptr, nullptr, n, side)) return sorted_fail(si, "error");
        si->transient = sorted_transient_bytes(n, si->n_win, scratch_bytes);
        const uint64_t kept = sorted_kept_bytes(si->lay.n_chunks, si->n_win);
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
            (void)hipGetLastError();
            free_b = 0;
        }
        if (sorted_memory_refused(si->transient, kept, free_b, reserve, waived)) return sorted_fail(si, "memory");
        if (hipMalloc(&si->keys, (size_t)n * 16) != hipSuccess || hipMalloc(&si->recs, (size_t)n * 8) != hipSuccess ||
            hipMalloc(&si->scratch, std::max<size_t>(scratch_bytes, 16)) != hipSuccess || hipMalloc(&si->rec_off, ((size_t)si->n_win + 1) * 4) != hipSuccess ||
            hipMalloc(&si->rec, si->lay.n_chunks * kSortedChunk * 4) != hipSuccess || hipMalloc(&si->carry, si->lay.n_chunks * 4) != hipSuccess ||
            hipMalloc(&si->win_chunk, ((size_t)si->n_win + 1) * 4) != hipSuccess)
            return sorted_fail(si, "memory");
        if (staged_copy(si->rec_off, si->lay.rec_off.data(), ((size_t)si->n_win + 1) * 4, hipMemcpyHostToDevice, side) != hipSuccess ||
            staged_copy(si->win_chunk, si->lay.win_chunk.data(), ((size_t)si->n_win + 1) * 4, hipMemcpyHostToDevice, side) != hipSuccess)
            return sorted_fail(si, "error");
        const uint4 *items = reinterpret_cast<const uint4 *>(fp.items);
        {
            ProfScope ps("sorted_image_emit", side);
            hipLaunchKernelGGL(sorted_image_emit, dim3(std::min<uint32_t>(fp.n_items, fp.n_cus * 8u)), dim3(256), 0, side, items, reinterpret_cast<const uint2 *>(fp.run_item_ent),
                               fp.n_items, reinterpret_cast<const uint2 *>(fp.run_ent), fp.n_range, si->key, fp.n_win, n, si->cnt + si->n_win + 1, si->keys, si->recs);
        }
        {
            ProfScope ps("sorted_image_sort", side);
            if (!sorted_sort_pairs(si->scratch, &scratch_bytes, si->keys, si->keys + n, si->recs, si->recs + n, n, side)) {
                (void)hipStreamSynchronize(side);
                return sorted_fail(si, "error");
            }
        }
        {
            ProfScope ps("sorted_image_finalise", side);
            hipLaunchKernelGGL(sorted_image_finalise, dim3(fp.n_win), dim3(64), 0, side, si->keys + n, si->recs + n, si->rec_off, si->win_chunk, fp.n_win, si->key,
                               si->rec, si->carry, si->cnt + si->n_win + 2);
        }
        if (fp.wb <= kSortedMaxWb) {  // (wider windows: the words stay 0, "not known")
            ProfScope ps("sorted_image_cell_max", side);
            hipLaunchKernelGGL(sorted_image_cell_max, dim3(fp.n_win), dim3(256), 0, side, si->rec, si->win_chunk, fp.wb, si->cnt + si->n_win + 3);
        }
        if (hipEventRecord(si->done, side) != hipSuccess || hipGetLastError() != hipSuccess) {
            (void)hipStreamSynchronize(side);
            return sorted_fail(si, "error");
        }
        si->phase = 2;
    }
}

const char *sorted_image_why(const SortedImage *si) { return si->why; }
int sorted_image_phase(const SortedImage *si) { return si->phase; }
uint64_t sorted_image_bytes(const SortedImage *si) { return si->phase == 3 ? sorted_kept_bytes(si->lay.n_chunks, si->n_win) : 0; }
uint64_t sorted_image_transient(const SortedImage *si) { return si->transient; }

void sorted_image_install(FastPlan *fp, const SortedImage *si, bool nt) {
    fp->sorted_rec = si->rec;
    fp->sorted_carry = si->carry;
    fp->sorted_win_chunk = si->win_chunk;
    fp->sorted_nt = nt;
    // FLATGFA_SORTED_CELLS=wide|packed (a test hook, read here): one form of the cells for unique depth -- packed only where the rule allows it
    // (any other value is no hook at all)
    const char *hook = std::getenv("FLATGFA_SORTED_CELLS");
    const int forced = !hook ? -1 : !strcmp(hook, "packed") ? 1 : !strcmp(hook, "wide") ? 0 : -1;
    fp->sorted_cells = sorted_cells_choice(forced, si->cell_max[0], si->cell_max[1]);
}

void sorted_image_free(SortedImage *si, hipStream_t side) {
    if (!si) return;
    if (si->phase == 1 || si->phase == 2) (void)hipStreamSynchronize(side);
    sorted_release_scratch(si);
    for (void *p : {(void *)si->rec, (void *)si->carry, (void *)si->win_chunk})
        if (p) (void)hipFree(p);
    if (si->done) (void)hipEventDestroy(si->done);
    delete si;
}

}  // namespace fgfa_dev
