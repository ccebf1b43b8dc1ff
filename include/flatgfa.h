/*
 * flatgfa.h -- C ABI of the MI355X-native FlatGFA depth engine (libflatgfa.so).
 *
 * Part 1 is a drop-in for the reference's `flatgfa-c` crate (cucapra/pollen,
 * flatgfa-c/src/lib.rs; its header is cbindgen-generated, flatgfa-c/build.rs:6-12):
 * identical type names, function names, signatures, ownership and in-band error
 * sentinels.  Part 2 is additive: the reference exposes its depth queries only
 * as Rust functions (flatgfa/src/ops/depth.rs), so the entry points a binding
 * for them would need are declared here, each citing the Rust item it replaces.
 * Part 3 is the device-level surface used when the caller already owns HBM
 * buffers (e.g. a torch tensor's data_ptr) and a HIP stream.
 *
 * All depth entry points run on the GPU through hand-written HIP kernels for
 * gfx950.  There is no CPU fallback: without a usable HIP device they return
 * FLATGFA_ERR_NO_DEVICE.
 */
#ifndef FLATGFA_H
#define FLATGFA_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libflatgfa.so is built with -fvisibility=hidden; only this header's functions are exported. */
#pragma GCC visibility push(default)

/* ------------------------------------------------------------------------ */
/* Part 1 -- the flatgfa-c surface                                          */
/* ------------------------------------------------------------------------ */

/* flatgfa-c/src/lib.rs:16,31 -- opaque store, handed out as a raw pointer. */
typedef struct CStore CStore;
typedef CStore *flatgfa_t;

/* flatgfa-c/src/lib.rs:36-40 -- borrowed, NOT NUL-terminated. */
typedef struct flatgfa_string_t {
    const uint8_t *data;
    int len;
} flatgfa_string_t;

/* flatgfa-c/src/lib.rs:140-144 */
typedef struct flatgfa_handle_t {
    uint32_t segment_id;
    bool is_forward;
} flatgfa_handle_t;

/* lib.rs:63 -- parse a GFA text file.  Where the reference aborts (missing or
 * malformed file) this returns NULL and sets flatgfa_last_error(). */
flatgfa_t flatgfa_parse(const char *filename);
/* lib.rs:72 -- NULL-safe; also releases any device buffers the handle owns. */
void flatgfa_free(flatgfa_t gfa);
/* lib.rs:80 */
uint32_t flatgfa_get_segment_count(flatgfa_t gfa);
/* lib.rs:92 -- {NULL,0} when segment_id is out of range. */
flatgfa_string_t flatgfa_get_seq(flatgfa_t gfa, uint32_t segment_id);
/* lib.rs:105 */
uint32_t flatgfa_path_count(flatgfa_t gfa);
/* lib.rs:118 -- {NULL,0} when path_index is out of range. */
flatgfa_string_t flatgfa_get_path_name(flatgfa_t gfa, uint32_t path_index);
/* lib.rs:130 -- UINT32_MAX when path_index is out of range. */
uint32_t flatgfa_get_path_step_count(flatgfa_t gfa, uint32_t path_index);
/* lib.rs:149-154 -- false when either index is out of range. */
bool flatgfa_get_step(flatgfa_t gfa, uintptr_t path_index, uintptr_t step_index, flatgfa_handle_t *out);

/* ------------------------------------------------------------------------ */
/* Part 2 -- additive: loaders, writers, and the depth queries              */
/* ------------------------------------------------------------------------ */

enum {
    FLATGFA_OK = 0,
    FLATGFA_ERR_ARG = -1,       /* NULL handle / bad argument */
    FLATGFA_ERR_BOUNDS = -2,    /* a span or segment id is out of range (the reference panics) */
    FLATGFA_ERR_NO_DEVICE = -3, /* no usable HIP device; there is no CPU fallback */
    FLATGFA_ERR_HIP = -4,       /* a HIP runtime call failed; see flatgfa_last_error() */
    FLATGFA_ERR_IO = -5,
    FLATGFA_ERR_TOO_LARGE = -6, /* more than 2^32-1 steps, or a size past an operation's own limit (path overlaps: 2^28 segments) */
    FLATGFA_ERR_PARSE = -7,     /* GFA text the reference's parser panics on (flatgfa_translate_prealloc; the parse calls that return a handle return NULL) */
    FLATGFA_ERR_STALE_PLAN = -8 /* FLATGFA_CHECK_NO_CLAIM=1 only: the step values changed behind a device plan (flatgfa_dev_plan_steps_changed) */
};

/* Thread-local description of the last failure in this thread ("" if none). */
const char *flatgfa_last_error(void);

/* Parser::parse_mem on a caller buffer (flatgfa/src/parse.rs:77; flatgfa-py/src/lib.rs parse_bytes). */
flatgfa_t flatgfa_parse_bytes(const uint8_t *data, size_t len);
/* Parser::parse_stream semantics (parse.rs:24-74; what `fgfa` uses for stdin, cli/main.rs:110-113):
 * an unterminated last line is kept and links are added before paths. */
flatgfa_t flatgfa_parse_stream_bytes(const uint8_t *data, size_t len);
/* file::view on a memory-mapped `.flatgfa` file, zero-copy (flatgfa/src/file.rs:185; cli/main.rs:99-100). */
flatgfa_t flatgfa_load(const char *flatgfa_filename);
/* file::dump (flatgfa/src/file.rs:290; cli/main.rs:197-201). */
int flatgfa_write_flatgfa(flatgfa_t gfa, const char *filename);
/* The preallocated ("in-place") container of `fgfa -m -p FACTOR -o OUT [-I GFA]`
 * (cli/main.rs:216-248, file.rs:255-272): every pool's region is `capacity` items long, `len` of
 * them in use.  With the GFA text the graph was parsed from, the capacities are the reference's
 * estimates from it (parse.rs:176-216, file.rs:136-158); with gfa_text == NULL, file.rs:117-132's
 * guess from `factor`.  FLATGFA_ERR_BOUNDS where a pool does not fit its capacity (the reference's
 * fixed-capacity store panics there).  flatgfa_load reads such files as it reads any other. */
int flatgfa_write_flatgfa_prealloc(flatgfa_t gfa, const char *filename, const uint8_t *gfa_text, size_t text_len, uint32_t factor);
/* prealloc_translate itself (cli/main.rs:216-248): GFA text -> preallocated container with no graph
 * in between.  The output file is created at the size its capacities add up to and mapped
 * (memfile::map_new_file, memfile.rs:24-33), file::init (file.rs:255-272) writes the empty table of
 * contents, the parser pushes straight into the file's regions (Parser::for_slice, parse.rs:170-174)
 * and the table's lengths are set at the end (Toc::for_fixed_store).  from_stream == 0: the text of
 * `-I GFA` (capacities estimated from it, Parser::parse_mem); != 0: the text came from stdin
 * (capacities guessed from `factor`, Parser::parse_stream).  Byte for byte the file that
 * flatgfa_parse_bytes + flatgfa_write_flatgfa_prealloc leave.  FLATGFA_ERR_BOUNDS where a pool
 * does not fit (the reference panics with the file as it then is: capacities in the table, every
 * length 0 -- so it is left here), FLATGFA_ERR_PARSE where the text does not parse. */
int flatgfa_translate_prealloc(const uint8_t *gfa_text, size_t text_len, int from_stream, const char *filename, uint32_t factor);
/* GFA text (flatgfa/src/print.rs:99-153).  *text is malloc'd; release with flatgfa_free_text. */
int flatgfa_print_gfa(flatgfa_t gfa, char **text, size_t *len);
void flatgfa_free_text(char *text);
/* Deterministic synthetic graph; model 0 = pangenome walk, 1 = uniform,
 * 2 = chromosome (paths walk along the graph, every other one downwards; one step in a hundred
 * jumps anywhere), 3 = haplotype (the same without those jumps: one step in 1600 skips up to 1087
 * segments), 4 = repeats (a haplotype walk that, one step in 6400, goes 16 .. 271 segments back and
 * walks them again). */
flatgfa_t flatgfa_synth(uint64_t seed, uint32_t n_segs, uint32_t n_paths, uint32_t steps_per_path, int model,
                        bool with_seq);

/* Raw pool access in `.flatgfa` order (file.rs:14-27): 0 header, 1 segs, 2 paths, 3 links,
 * 4 steps, 5 seq_data, 6 overlaps, 7 alignment, 8 name_data, 9 optional_data, 10 line_order.
 * *data borrows from the handle and may be unaligned (the reference's PODs are repr(packed)). */
int flatgfa_pool(flatgfa_t gfa, int pool_index, const void **data, uint64_t *len, uint64_t *elem_size);
/* FlatGFA::find_path (flatgfa.rs:387): first path with this name, or -1. */
int64_t flatgfa_find_path(flatgfa_t gfa, const uint8_t *name, size_t len);

/* Number of visible HIP devices (0 if none). */
int flatgfa_device_count(void);
/* Start the HIP runtime on `device` ahead of need: the runtime's own start-up (a tenth of a second
 * and more on a cold process), the pinned staging buffers large copies go through, the first copy and
 * the first kernel launch of the process.  Meant to be called from a helper thread while the caller
 * maps or parses its graph (`fgfa` does); everything it does would otherwise happen inside the
 * first flatgfa_to_device.  Returns 0, or FLATGFA_ERR_NO_DEVICE / FLATGFA_ERR_HIP. */
int flatgfa_warm_device(int device);
/* Host memory policy of the PROCESS (glibc's malloc; a no-op elsewhere): with `on`, freed host memory stays with the process --
 * nothing is unmapped, the heap is not trimmed -- instead of going back to the system.  Why a GPU library has this: on the
 * amdgpu/KFD driver a process that unmaps host memory has its GPU queues quiesced and restored by a delayed work item, and
 * the next kernel launch or copy then waits 10-30 ms (in steps of the kernel's timer tick; a second now and then) where it
 * would take 0.1 -- measured: a first query 20 ms instead of 0.9, a plan over a million paths 49 ms instead of 12
 * (profiles/NOTES.md R6.6c).  The library keeps its own large temporaries; what the host application frees around its
 * queries -- a parsed GFA, result vectors, a table -- is the application's to keep, or this switch's.  Not applied by the
 * library itself: `fgfa` and the Python package call it at start-up (FLATGFA_KEEP_HOST_MEMORY=0 in the environment keeps
 * them from it).  Returns 0. */
int flatgfa_keep_host_memory(int on);
/* Copy the graph's structure-of-arrays image (steps, path spans, segment lengths) into the
 * HBM of `device` and keep it resident until flatgfa_free.  Depth calls do this lazily on
 * device 0 if it has not been done. */
int flatgfa_to_device(flatgfa_t gfa, int device);
/* What that took on this handle, in milliseconds of host time: the host-to-device copies (SoA
 * conversion and allocation included) and the creation of the depth plan (scratch, item lists,
 * the timing of kernel variants).  An error before the graph is resident. */
int flatgfa_residency_ms(flatgfa_t gfa, double *h2d_ms, double *plan_ms);

/* seg_depth_with_uniq (ops/depth.rs:15-39) when uniq_out != NULL, seg_depth (depth.rs:45-56)
 * when it is NULL.  Outputs are indexed by segment id, one uint64_t (Rust usize) each. */
int flatgfa_seg_depth(flatgfa_t gfa, uint64_t *depth_out, uint64_t *uniq_out);
/* path_depth + measure_path (ops/depth.rs:88-131) for the given path ids, in order.  Every path's two
 * sums -- its length and sum of depth * segment length -- must stay below 2^64 (the reference's usize:
 * beyond it a release build wraps and a debug build panics); the mean is (weighted as f64) / (length
 * as f64), each total rounded to nearest-even once, and NaN for a path of no bases. */
int flatgfa_path_depth(flatgfa_t gfa, const uint32_t *path_ids, uint32_t n_ids, uint64_t *length_out,
                       double *mean_depth_out);
/* The bytes `fgfa depth -d` prints: SegDepth::emit (ops/depth.rs:67-82; cli/cmds.rs:237-245). */
int flatgfa_depth_table(flatgfa_t gfa, char **text, size_t *len);
/* The bytes `fgfa depth [-r NAME]...` prints: PathDepth::emit (ops/depth.rs:143-160;
 * cli/cmds.rs:256-284).  path_ids == NULL means all paths, in order. */
int flatgfa_path_depth_table(flatgfa_t gfa, const uint32_t *path_ids, uint32_t n_ids, char **text, size_t *len);
/* PathDepth::as_bed (ops/depth.rs:173-183): the same paths as a BED store -- one entry
 * {path name, 0, path length in base pairs} each, the depths dropped -- rendered as three-column
 * BED text (`name\t0\tlength\n`).  path_ids == NULL means all paths, in order. */
int flatgfa_path_depth_bed(flatgfa_t gfa, const uint32_t *path_ids, uint32_t n_ids, char **text, size_t *len);
/* odgi-style node depth restricted to a subset of paths (`odgi depth -d -s FILE`,
 * slow_odgi/slow_odgi/depth.py:12; tests/turnt.toml:31-44).  The reference's Rust `-d` ignores
 * `-r`; this closes that gap.  path_ids may repeat: each occurrence counts as its own path. */
int flatgfa_seg_depth_subset(flatgfa_t gfa, const uint32_t *path_ids, uint32_t n_ids, uint64_t *depth_out,
                             uint64_t *uniq_out);
/* Path-pair overlap (slow_odgi/slow_odgi/overlap.py:6-32; `odgi overlap -R FILE`):
 * touch_out[k * path_count + j] = 1 iff path j touches query path query_ids[k]. */
int flatgfa_path_overlaps(flatgfa_t gfa, const uint32_t *query_ids, uint32_t n_q, uint8_t *touch_out);
/* The bytes `slow_odgi overlap --paths FILE` prints for these query paths (overlap.py:17-32). */
int flatgfa_overlap_table(flatgfa_t gfa, const uint32_t *query_ids, uint32_t n_q, char **text, size_t *len);
/* interval_depth (flatgfa/src/ops/window_depth.rs:176-180): mean depth of each [start,end) interval
 * (base pairs along path `path_index`, sorted) -- node depth from the GPU, the f64 accumulation of
 * assign_depths (:116-147) on the host in the reference's order. */
int flatgfa_interval_depth(flatgfa_t gfa, uint32_t path_index, const uint64_t *starts, const uint64_t *ends,
                           uint64_t n_intervals, double *depth_out);
/* The bytes `fgfa window-depth PATH SIZE` prints (window_depth.rs:183-200, cli/cmds.rs:488-496). */
int flatgfa_window_depth_table(flatgfa_t gfa, uint32_t path_index, uint64_t window, char **text, size_t *len);
/* The pangenotype matrix (flatgfa/src/ops/pangenotype.rs:11-70; flatgfa-py's make_pangenotype_matrix):
 * row f says, for every segment id s, whether some line of GAF text gaf[f][0, gaf_len[f]) names s in its
 * path field.  A line is the bytes before a '\n' (what follows the last '\n' is not one); empty lines and
 * lines that start with '#' are skipped; the path field is what follows the 5th tab, up to the next tab;
 * every '>' or '<' in it starts a name, its digits read as a u64 (wrapping) and looked up in the graph's
 * NameMap.  bits_out holds n_files rows of ceil(S / 64) words: bit s & 63 of word s >> 6 of row f is
 * segment s (np.unpackbits(..., bitorder="little") order).  Each buffer goes to the device in chunks cut
 * after a '\n', through the process's pinned staging, copies overlapping the scan of the chunk before;
 * device memory is two chunks and one row, all freed before the call returns.  A name the graph does not
 * have (name 0 included: a '>' with no digits), where the reference panics: FLATGFA_ERR_BOUNDS, and
 * flatgfa_last_error() names the file's index and the byte offset of the first such line.  The graph need
 * not be resident, and this does not make it so. */
int flatgfa_pangenotype_matrix(flatgfa_t gfa, const uint8_t *const *gaf, const size_t *gaf_len, uint32_t n_files,
                               uint64_t *bits_out);
/* The bytes `fgfa matrix GAF` prints (cli/cmds.rs:465-474) for these files: one line per file, a '0' or
 * '1' per segment id.  *text is malloc'd; release with flatgfa_free_text. */
int flatgfa_pangenotype_table(flatgfa_t gfa, const uint8_t *const *gaf, const size_t *gaf_len, uint32_t n_files,
                              char **text, size_t *len);
/* The GAF lookup (flatgfa/src/ops/gaf.rs; `fgfa gaf GAF [-s] [-b]`, cli/cmds.rs:311-376; flatgfa-py's all_reads and
 * print_gaf_lookup): every line of gaf[0, len) -- the bytes before a '\n', none skipped; what follows the last '\n' is not
 * a line -- is a read.  Field 0 is its name, field 5 its path, fields 7 and 8 its start and end along that path (digits,
 * read wrapping).  The path's tokens (`>N` forward, `<N` backward, up to the first byte that continues neither) are looked
 * up in the graph's NameMap and give one event each: the stretch of the segment that [start, end) covers
 * (gaf.rs:200-243) -- none of it, all of it, or Partial(a, b).  The text goes to the device in chunks cut after a '\n'
 * through the process's pinned staging and the answers come back the same way; the name table and the sequence pool are
 * uploaded on first use and kept with the handle.  The graph need not be resident, and this does not make it so.
 * Where the reference panics: a line without nine tabs or without digits, each run followed by a tab, in fields 7 and 8
 * gives FLATGFA_ERR_PARSE; a name the graph does not have gives FLATGFA_ERR_BOUNDS; and so does, where bases are asked
 * for (flatgfa_gaf_seqs), a Partial(a, b) that cannot be sliced (an end below the start).  flatgfa_last_error() names the
 * byte offset of the first such line, and the line at the lowest offset decides the code.  Nothing is returned then. */
/* `fgfa gaf GAF -b`: the number of events (and of lines, when `lines` is not NULL); every name is still looked up. */
int flatgfa_gaf_count(flatgfa_t gfa, const uint8_t *gaf, size_t len, uint64_t *events, uint64_t *lines);
/* The bytes `fgfa gaf GAF -s` prints (cmds.rs:349-357): per read its name, a tab, the bases its events cover as the graph
 * spells them (a backward handle reversed and complemented: ACGTacgt to TGCAtgca, every other byte itself), a newline.
 * *text is malloc'd; release with flatgfa_free_text. */
int flatgfa_gaf_seqs(flatgfa_t gfa, const uint8_t *gaf, size_t len, char **text, size_t *text_len);
/* The bytes `fgfa gaf GAF` prints (cmds.rs:367-374, gaf.rs:167-197): per read its name and a newline, then per event
 * "{index}: {segment name}{+|-}, {a}-{b}bp", "{index}: {segment name}{+|-}, {length}bp" or "{index}: (skipped)" with nothing
 * between or behind them.  Formatted on the host from flatgfa_gaf_events. */
int flatgfa_gaf_table(flatgfa_t gfa, const uint8_t *gaf, size_t len, char **text, size_t *text_len);
/* The events themselves, in host memory (one block: release with flatgfa_gaf_events_free).  Line l's events are
 * [line_first[l], line_first[l + 1]); its name is gaf[name_off[l], name_off[l] + name_len[l]). */
typedef struct flatgfa_gaf_events_t {
    uint64_t n_lines;
    uint64_t n_events;
    uint64_t *line_first; /* [n_lines + 1] */
    uint64_t *name_off;   /* [n_lines] */
    uint64_t *name_len;   /* [n_lines] */
    uint32_t *handle;     /* [n_events]: (segment id << 1) | backward */
    uint8_t *kind;        /* [n_events]: 0 none, 1 all, 2 partial */
    uint64_t *a;          /* [n_events]: Partial(a, b); 0 and the segment's length for all; 0, 0 for none */
    uint64_t *b;
} flatgfa_gaf_events_t;
int flatgfa_gaf_events(flatgfa_t gfa, const uint8_t *gaf, size_t len, flatgfa_gaf_events_t **out);
void flatgfa_gaf_events_free(flatgfa_gaf_events_t *ev);
/* chop (flatgfa/src/ops/chop.rs; `fgfa chop -c max_size [-l]`, cli/main.rs:139-159): every segment longer
 * than max_size becomes ceil(len / max_size) segments -- max_size bases each, the remainder last -- numbered in
 * segment order and named id + 1; a step becomes the steps of its pieces (reversed, all backward, for a backward
 * step); paths keep their names and lose their overlaps.  links != 0: the forward links between the pieces of each
 * chopped segment, then every old link remapped to the pieces it touches (from: the last piece of a forward handle,
 * the first of a backward one; to: the other way round), all with an empty alignment; links == 0: no links.  *out is a
 * new heap handle that owns copies of what it keeps of `gfa` (header, seq_data, name_data), so it outlives `gfa`.
 * The counts, scans and expansion run on the GPU (the device `gfa` is resident on, else device 0); `gfa` is not
 * made resident, and a resident one is only read.  max_size == 0 (where the reference loops forever):
 * FLATGFA_ERR_ARG; a span, step or link naming something out of range: FLATGFA_ERR_BOUNDS; 2^31 or more new
 * segments, or more than 2^32 - 1 new steps or links: FLATGFA_ERR_TOO_LARGE, found before any output is allocated. */
int flatgfa_chop(flatgfa_t gfa, uint64_t max_size, int links, flatgfa_t *out);
/* inject (slow_odgi/inject.py, `odgi inject`; `fgfa inject -b BED [-l]`): line l -- bases [starts[l], ends[l]) of path
 * path_ids[l], to be called names[l] (name_lens[l] bytes) -- cuts the segments under its two ends so that both fall on
 * segment seams and adds a path that walks exactly the interval.  All lines are handled in one pass, which gives what the
 * reference gives line by line: a segment with k distinct cuts becomes k + 1 segments, numbered in old-segment order and by
 * position and named id + 1 (seq spans into the old seq_data, no optional fields); an old path keeps its name, loses its
 * overlaps, and walks the pieces of its steps (reversed, all backward, for a backward step); the new paths follow the old
 * ones in line order, each the steps of its path after cutting from the first that starts at or after `start` up to, but not
 * including, the first that ends after `end` (none when start >= end or start is at or past the path's end).  links as
 * flatgfa_chop's.  *out is a new heap handle that owns its pools.  The work runs on the GPU (the device `gfa` is resident
 * on, else device 0); `gfa` is not made resident, and a resident one is only read.
 * Refused with FLATGFA_ERR_ARG before any device work, flatgfa_last_error naming the line, where the reference's
 * line-by-line dictionary update does what one pass cannot: a new name that is a path of `gfa` already (the reference
 * replaces that path), a new name an earlier line gave (the later wins there), and -- flatgfa_inject_bed only -- a line on a
 * path that `gfa` lacks but an earlier line injects.  A path id, span, step or link out of range: FLATGFA_ERR_BOUNDS; 2^31
 * or more new segments, or more than 2^32 - 1 new steps, links or paths: FLATGFA_ERR_TOO_LARGE, found before any output is
 * allocated.  n == 0: a copy of the graph with no cuts.
 * flatgfa_inject_bed reads BED text: "path<TAB>start<TAB>end<TAB>new_name" lines ('#' lines and empty lines skipped; a line
 * with fewer than four columns, with an empty new name, or without a number in the second or third: FLATGFA_ERR_ARG; a number
 * past 2^64 - 1 wraps, as the --bed-paths reader's does); a line whose path `gfa` does not have is skipped silently, as the
 * reference does.  The line a message names is counted from 1 over every line of the text, comments and empty lines too. */
int flatgfa_inject(flatgfa_t gfa, const uint32_t *path_ids, const uint64_t *starts, const uint64_t *ends, const char *const *names,
                   const size_t *name_lens, uint64_t n, int links, flatgfa_t *out);
int flatgfa_inject_bed(flatgfa_t gfa, const char *bed, size_t bed_len, int links, flatgfa_t *out);
/* crush (slow_odgi/crush.py, `odgi crush`; `fgfa crush`): within each segment's sequence every maximal run of the byte 'N'
 * (0x4E, and no other: 'n' and '*' are ordinary bytes) becomes a single N; runs never join across segments.  *out is a new
 * heap handle that owns its pools and outlives `gfa`: seq_data is the crushed segments one behind another in segment order,
 * whatever the input spans were (they may be out of order, overlap, alias or be empty), and every segment's span points into
 * it -- an empty segment's at the place where the next segment begins; segments keep their names and lose their optional
 * fields, paths keep their names and steps and lose their overlaps; header, steps, links, alignment and name_data are copies
 * of the input's; overlaps, optional_data and line_order are empty (the text comes out in normalized order).  The steps are
 * neither read nor checked.  The count, the scans and the compaction run on the GPU (the device `gfa` is resident on, else
 * device 0), on the sequence pool the handle keeps there when it has one, else on a copy made for the call; `gfa` is only
 * read.  A segment span that leaves seq_data: FLATGFA_ERR_BOUNDS, before any device work; more than 2^32 - 1 kept bytes:
 * FLATGFA_ERR_TOO_LARGE, found before any output is allocated. */
int flatgfa_crush(flatgfa_t gfa, flatgfa_t *out);
/* flip (slow_odgi/flip.py, `odgi flip`; `fgfa flip`): a path whose backward steps cover more bases than its forward steps
 * (64-bit sums of Segment::len(); strictly more: a tie, an empty path or a path of empty segments stays) is turned around --
 * its steps in reverse order, each orientation toggled -- and gets `_inv` appended to its name; for every consecutive pair
 * (a, b) of a turned path's new steps the link a -> b with the overlap 0M joins the links, behind the old ones, in path order
 * then step order; then the links are de-duplicated: two links are one when their overlaps are equal op for op and they have
 * the same (from, to) or one is the other's reverse complement (flip(to), flip(from)), and the first of each class stays, in
 * that order -- among the old links too, and whether or not any path turns.  *out is a new heap handle that owns its pools and
 * outlives `gfa`: the steps are the paths one behind another in path order, whatever the input spans were (they may be out of
 * order, overlap or leave gaps); name_data is the paths' names one behind another; kept old links keep their overlap spans,
 * and the new ones share one 0M op appended to the alignment pool (appended only when a new link is kept); paths lose their
 * overlaps and segments their optional fields; header, segments and seq_data are copies of the input's; overlaps,
 * optional_data and line_order are empty (the text comes out in normalized order), as flatgfa_crush leaves them.  Every path
 * is kept, also where several share a name (the reference keys paths by name and keeps one).  The weighing, the rewrite, the
 * grouping of the links by canonical key, the decisions and the compaction run on the GPU (the device `gfa` is resident on,
 * else device 0), on the steps the handle keeps there when it has them; `gfa` is only read.  A step or link that names a
 * segment >= the segment count, a path span that leaves the steps, a segment span that leaves seq_data, a link whose overlap
 * span leaves the alignment pool: FLATGFA_ERR_BOUNDS; more links and steps together than 2^32 - 2 (every step may add a link,
 * and the ordinals are 32 bits wide), more than 2^32 - 1 bytes of names, or -- where links and steps together are more than
 * 2^27 -- more than 2^26 links and step pairs on one handle: FLATGFA_ERR_TOO_LARGE; all before any output exists.  flatgfa_flip_count is the count alone: how many paths would turn and how many links the output would have (either
 * pointer may be NULL). */
int flatgfa_flip(flatgfa_t gfa, flatgfa_t *out);
int flatgfa_flip_count(flatgfa_t gfa, uint64_t *n_turned, uint64_t *n_links_out);
/* extract (flatgfa/src/ops/extract.rs; `fgfa extract -n NAME -c DIST [-d N] [-e N]`, cli/cmds.rs:174-215): the subgraph
 * around one segment.  flatgfa_find_seg is FlatGFA::find_seg (flatgfa.rs:380-384): the id of the first segment with that
 * name, or -1.  The new graph holds the old header; the origin as segment 0 and every segment within link_distance links
 * of it, numbered in the order the reference's walk meets them (each level pops its frontier from the back and reads all
 * links in link order); the segments of every gap between two visits of a path to the subgraph that re-enters at a base
 * position of at most max_distance_subpaths, swept over all paths num_iterations times (the reference CLI's defaults:
 * 300000 and 6); every link between two kept segments with its alignment; and per path one new path
 * "{name}:{start}-{end}" for each maximal run of steps on kept segments, without overlaps.  line_order is empty, so the
 * graph prints in normalized order.  *out is a new heap handle that owns all its pools and outlives `gfa`.  The walk
 * over the links, the positions, the subpaths, the link filter and the gathers run on the GPU (the device `gfa` is
 * resident on, else device 0); a resident graph's steps are read in place, and `gfa` is not made resident (its sequence
 * pool is kept on the device with the handle, as for the GAF lookup).  An origin, step, link or span naming something out
 * of range: FLATGFA_ERR_BOUNDS; totals past 32-bit ids or spans: FLATGFA_ERR_TOO_LARGE, before any output is allocated. */
int64_t flatgfa_find_seg(flatgfa_t gfa, uint64_t name);
int flatgfa_extract(flatgfa_t gfa, uint32_t origin_seg, uint64_t link_distance, uint64_t max_distance_subpaths,
                    uint64_t num_iterations, flatgfa_t *out);
/* position (flatgfa/src/ops/position.rs; `fgfa position -p path,offset,+`, cli/cmds.rs:105-152): the step of a path that
 * holds base `offset` -- the first whose end position is past it -- as *handle_out (segment << 1 | backward) and the
 * offset into that step, with *found = 1; *found = 0 when the path is no longer than `offset`.  A segmented scan of the
 * path's segment lengths and a search on the GPU.  flatgfa_position_table takes the CLI's argument and returns the bytes
 * the reference prints (nothing when not found; free with flatgfa_free_text); a malformed triple, an unknown path or the
 * orientation "-" give FLATGFA_ERR_ARG with the reference's own message in flatgfa_last_error(). */
int flatgfa_position(flatgfa_t gfa, uint32_t path, uint64_t offset, uint32_t *handle_out, uint64_t *seg_offset_out, int *found);
int flatgfa_position_table(flatgfa_t gfa, const uint8_t *triple, size_t len, char **text, size_t *n);
/* validate (slow_odgi/slow_odgi/validate.py:5-25; `fgfa validate`): do the links support the paths?  Every path is walked
 * in path order and every pair of consecutive steps (a, b) of one path in step order -- a path of fewer than two steps has
 * none (validate.py:11-12), and a path's last step forms none with the next path's first.  The pair is supported when a link
 * has (from, to) == (a, b) or == (flip(b), flip(a)) (validate.py:16-19 over the `outs` lists of mygfa/preprocess.py:23-43).
 * One record per unsupported pair, in that order: the path's index, the index of `a` within the path, and the two handles
 * (segment << 1 | backward).  *out is malloc'd (release with flatgfa_missing_links_free) and may be NULL when *n == 0;
 * out == NULL with n != NULL returns the count only.  flatgfa_validate_table returns the bytes the reference prints, one
 * line per record (validate.py:20-24; nothing for a valid graph; free with flatgfa_free_text), formatted on the host.
 * The links become an index on the GPU -- built on the first validate or degree call, kept with the handle and freed by
 * flatgfa_free -- and one pass over the steps looks every pair up in it (the device `gfa` is resident on, else device 0;
 * a resident graph's steps are read in place, and `gfa` is not made resident).  A link or a step naming a segment out of
 * range, or a path whose span leaves the steps pool: FLATGFA_ERR_BOUNDS; NULL arguments: FLATGFA_ERR_ARG. */
typedef struct { uint32_t path, step, from, to; } flatgfa_missing_link_t;
int flatgfa_validate(flatgfa_t gfa, flatgfa_missing_link_t **out, uint64_t *n);
void flatgfa_missing_links_free(flatgfa_missing_link_t *p);
int flatgfa_validate_table(flatgfa_t gfa, char **text, size_t *len);
/* degree (slow_odgi/slow_odgi/degree.py:5-18; `fgfa degree`): degree_out[s] = the number of link ends on segment s -- the
 * links whose `from` names it plus those whose `to` does, whatever the orientations (degree.py:11-16: the four lists of
 * preprocess.py:31-41), so a self-loop counts 2 and a duplicate link counts again.  Counted on the GPU in the pass that
 * builds the link index.  flatgfa_degree_table: "#node.id\tnode.degree\n", then "{name}\t{degree}\n" per segment in pool
 * order (degree.py:7, 17; free with flatgfa_free_text). */
int flatgfa_degree(flatgfa_t gfa, uint64_t *degree_out /* [segment_count] */);
int flatgfa_degree_table(flatgfa_t gfa, char **text, size_t *len);
/* The bytes `fgfa depth -b FILE.bed` prints (window_depth.rs:203-211, cli/cmds.rs:246-255); the BED
 * text is parsed as flatbed.rs:125-158 does. */
int flatgfa_bed_depth_table(flatgfa_t gfa, const uint8_t *bed, size_t bed_len, char **text, size_t *len);
/* Interval and window depth over many paths in one call, the interval walk on the GPU as well (the three entries above
 * take one path per call and walk it on the host; their results are these, path by path).  Interval k lies on path
 * path_ids[k]; a group is a maximal run of equal path_ids, and each group is one interval_depth of the reference
 * (window_depth.rs:116-147) with a cursor of its own: within a group the intervals may be unsorted, overlapping or inverted
 * and get what the reference's loop gives them, bit for bit; the same path in two separate runs is two groups.  Node depth
 * stays on the device; only the n_intervals doubles come back.  A path id >= flatgfa_path_count: FLATGFA_ERR_BOUNDS, nothing
 * written.  n_intervals == 0: FLATGFA_OK. */
int flatgfa_intervals_depth(flatgfa_t gfa, const uint32_t *path_ids, const uint64_t *starts, const uint64_t *ends,
                            uint64_t n_intervals, double *depth_out);
/* The concatenation, in order, of what `fgfa window-depth P SIZE` prints for each listed path (`fgfa window-depth-all SIZE`);
 * path_ids == NULL: all paths.  A path may be listed any number of times, in a row or apart: every listing is a table of its
 * own (not one group of flatgfa_intervals_depth).  window == 0: FLATGFA_ERR_ARG. */
int flatgfa_window_depth_paths_table(flatgfa_t gfa, const uint32_t *path_ids, uint32_t n_ids, uint64_t window,
                                     char **text, size_t *len);
/* `fgfa depth -b`, except that every entry is looked up by its own name (`fgfa depth --bed-paths FILE`): consecutive
 * entries on one path are a group.  A name the graph does not have: FLATGFA_ERR_BOUNDS, and flatgfa_last_error names the
 * entry's index.  No entries: FLATGFA_ERR_BOUNDS. */
int flatgfa_bed_depth_paths_table(flatgfa_t gfa, const uint8_t *bed_text, size_t bed_len, char **text, size_t *len);
/* flatten (slow_odgi/slow_odgi/flatten.py:5-57; `fgfa flatten [-n NAME] [-f FASTA] [-b BED]`, `odgi flatten -f -b`,
 * tests/turnt.toml:46-49): the graph in linear coordinates.  `name` is name_len bytes of the caller's (not NUL-terminated).
 * The FASTA (flatten.py:51-55): ">" name "\n", then the bases of every segment in pool order -- segment s is
 * seq_data[seq.start, seq.end), gathered: the spans need not be in order, disjoint or contiguous -- with a newline after every
 * 80 of them (insert_newlines, flatten.py:44-46) and one at the end (print's); with no bases the body is that one newline.
 * The BED (flatten.py:23-41): "#name\tstart\tend\tpath.name\tstrand\tstep.rank\n", then for every path in pool order and
 * every step of its span in order (rank i from 0) "{name}\t{start}\t{end}\t{path name}\t{+|-}\t{i}\n": start is the legend
 * (flatten.py:13-19) of the step's segment -- the lengths of the segments before it in pool order -- and end = start + its
 * length, '+' a forward handle; plain decimal, offsets 64-bit.  Path spans may overlap, alias or be empty, and paths of one
 * name are emitted as often as they occur.
 * The legend is an exclusive scan on the GPU, made on the first flatten call and kept with the handle (freed by
 * flatgfa_free); both texts are formed on the GPU by tile of output bytes -- the BED a fixed number of lines at a time, so
 * device memory beyond the graph does not grow with the step count -- and leave through the process's pinned staging while
 * the next piece is formed.  The device `gfa` is resident on, else device 0; a resident graph's steps are read in place, and
 * `gfa` is not made resident (its sequence pool is kept on the device with the handle, as for the GAF lookup, once a FASTA is
 * asked for).  A step naming a segment out of range, or a span that leaves its pool: FLATGFA_ERR_BOUNDS, nothing delivered.
 * Without a device: FLATGFA_ERR_NO_DEVICE.  NULL arguments, name == NULL with name_len != 0: FLATGFA_ERR_ARG. */
/* flatten.py:13-19: offset_out[s] = the bases before segment s; offset_out[segment_count] = all bases. */
int flatgfa_flatten_legend(flatgfa_t gfa, uint64_t *offset_out /* [segment_count + 1] */);
/* flatten.py:51-55 and :23-41, each into a malloc'd buffer (release with flatgfa_free_text): the stream below into memory. */
int flatgfa_flatten_fasta(flatgfa_t gfa, const char *name, size_t name_len, char **text, size_t *len);
int flatgfa_flatten_bed(flatgfa_t gfa, const char *name, size_t name_len, char **text, size_t *len);
/* flatten.py:49-57 as a stream: the bytes in order, in pieces of whatever size the chunks give, each handed to `sink` (the
 * pointer is the library's and holds until the sink returns).  what: 1 the FASTA, 2 the BED, 3 both, the FASTA first (what
 * `slow_odgi flatten` prints, __main__.py:178); anything else, or a NULL sink: FLATGFA_ERR_ARG.  A sink that returns nonzero
 * ends the call with FLATGFA_ERR_IO, and nothing more is delivered. */
typedef int (*flatgfa_sink_t)(void *ctx, const char *bytes, size_t n); /* nonzero: stop */
int flatgfa_flatten_stream(flatgfa_t gfa, const char *name, size_t name_len, int what, flatgfa_sink_t sink, void *ctx);
/* The packed-sequence codec (flatgfa/src/packedseq.rs; `fgfa seq-export INPUT OUTPUT`, `fgfa seq-import FILE`,
 * cli/cmds.rs:415-452).  No graph is read.  The file: a 25-byte header without padding -- u64 magic 0x12, u64 len, u64
 * capacity (the writer's equals len), u8 high_nibble_end (1: an even number of bases, zero included), little-endian -- then
 * len data bytes of two bases each, base 2k in the low nibble of byte k and base 2k + 1 in the high one, A = 0, C = 1, T = 2,
 * G = 3; the unused high nibble of an odd sequence's last byte is written as 0 and never read.
 * flatgfa_seq_export packs `text` on the GPU (device 0) into a malloc'd file image (release with flatgfa_free_text):
 * whitespace -- space, \t, \n, \x0C, \r; not \x0B -- is dropped and every other byte must be one of A C T G, else
 * FLATGFA_ERR_PARSE with flatgfa_last_error naming the smallest offending offset and its byte ("seq-export: byte 0x6e at offset
 * 12 is not a nucleotide"), *file_image left NULL and, for flatgfa_seq_export_file, no file made.  flatgfa_seq_import unpacks a
 * file image into the bases, without a newline, in a malloc'd buffer (release with flatgfa_free_text); flatgfa_seq_import_stream
 * hands the same bytes to `sink` in pieces (a sink that returns nonzero: FLATGFA_ERR_IO).  FLATGFA_ERR_PARSE, before any
 * device work, for a file shorter than the header, a wrong magic, high_nibble_end not 0 or 1, capacity < len, fewer than
 * capacity bytes behind the header, or len == 0 with high_nibble_end == 0; and, with nothing delivered, for a nibble above 3
 * among the bases, flatgfa_last_error naming the smallest such base index.  Bytes behind the data are ignored.
 * flatgfa_seq_packed_info is the header check alone, on the host: the base count and where the data begin.  n == 0 is valid
 * with a NULL pointer.  Text and packed bytes travel in chunks of 64 MiB; the result does not depend on where they are cut.
 * Without a device the export and import calls return FLATGFA_ERR_NO_DEVICE; NULL arguments: FLATGFA_ERR_ARG. */
int flatgfa_seq_export(const uint8_t *text, size_t n, uint8_t **file_image, size_t *file_len);
int flatgfa_seq_export_file(const uint8_t *text, size_t n, const char *filename);
int flatgfa_seq_import(const uint8_t *file, size_t n, char **text, size_t *text_len);
int flatgfa_seq_import_stream(const uint8_t *file, size_t n, flatgfa_sink_t sink, void *ctx);
int flatgfa_seq_packed_info(const uint8_t *file, size_t n, uint64_t *n_bases, uint64_t *data_offset);
/* The GFA text of flatgfa_print_gfa (flatgfa/src/print.rs:99-153, either order), formatted on the GPU: the same bytes
 * (`fgfa print`).  flatgfa_print_gfa stays the route for a machine without a device.  Everything is
 * checked and counted before a byte is delivered.  What stops flatgfa_print_gfa stops these with its code and sentence,
 * FLATGFA_ERR_BOUNDS, found on the host before any device is asked for, the first of them in line order: "print: empty
 * header", "print: too few segments", "print: too few paths", "print: too few links", "print: bad line kind", "print: path
 * with no steps".  Where the host printer would read outside a pool -- a sequence, optional, name, steps, overlaps or
 * alignment span that leaves its pool, a step or link that names no segment -- FLATGFA_ERR_BOUNDS, flatgfa_last_error naming
 * the pool.  More than 2^32 - 1 steps or more than 2^31 segments: FLATGFA_ERR_TOO_LARGE.  Without a device:
 * FLATGFA_ERR_NO_DEVICE; NULL arguments: FLATGFA_ERR_ARG, answered without one.  A resident handle's steps are read in place.
 * An empty graph is zero bytes, and the sink is never called. */
/* the size of the text, nothing delivered */
int flatgfa_print_gfa_bytes(flatgfa_t gfa, uint64_t *bytes);
/* the text in a malloc'd buffer (release with flatgfa_free_text) */
int flatgfa_print_gfa_device(flatgfa_t gfa, char **text, size_t *len);
/* the text in order, a piece at a time; a sink that returns nonzero ends the call with FLATGFA_ERR_IO, nothing more is
 * delivered, and the handle answers as before */
int flatgfa_print_gfa_stream(flatgfa_t gfa, flatgfa_sink_t sink, void *ctx);
/* Which lines of BED text `b` lie under the intervals of BED text `a` (`fgfa bed -a FILE -b FILE`; cli/cmds.rs:392-413,
 * flatbed.rs:37-57): byte for byte what the reference prints.  Both texts are read as flatgfa_bed_depth_table
 * reads its BED text (flatbed.rs:125-158: an unterminated last line is dropped, `#` lines are skipped, the name is the bytes
 * before the first tab, numbers are u64 and wrap, columns after the third are ignored), and what stops it stops these with
 * its code and sentence.  The entries of `a` are taken in file order, and for each the entries x of `b` in file order: with
 * s = max(x.start, a.start) and e = min(x.end, a.end), "name \t s \t e \n" is printed where the two names are equal byte for
 * byte and e > s.  Duplicates are kept.  No graph is read.  The pairs are not all tried: the entries of `b` are grouped by
 * name, and where a group's starts never decrease in file order an entry of `a` meets only the stretch of the group that
 * can overlap it; a group that is not so sorted is walked whole for each entry of `a` of its name (the same text, at the cost
 * of the reference's double loop restricted to that name).
 * A text of 2^32 bytes or more, or a file of 2^32 - 1 entries or more: FLATGFA_ERR_BOUNDS and a sentence that starts "bed: ",
 * the former before a byte of the text is read.  NULL arguments (a text may be NULL only with length 0): FLATGFA_ERR_ARG,
 * answered without a device; so are the parse errors and the refusals.  Without a device: FLATGFA_ERR_NO_DEVICE. */
/* the text in a malloc'd, NUL-terminated buffer (release with flatgfa_free_text) */
int flatgfa_bed_intersect(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, char **text, size_t *len);
/* the text in order, a piece at a time; a sink that returns nonzero ends the call with FLATGFA_ERR_IO, nothing more is
 * delivered; with no line to print the sink is never called */
int flatgfa_bed_intersect_stream(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, flatgfa_sink_t sink, void *ctx);
/* the same work without the text: how many lines and bytes the text has, how many pairs were tried (*candidates), and how
 * many of b's name groups were walked whole (*unsorted_groups) */
int flatgfa_bed_intersect_count(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint64_t *lines, uint64_t *bytes,
                                uint64_t *candidates, uint64_t *unsorted_groups);
/* GFA text parsed on the GPU (`fgfa -D`): a handle whose pools are byte for byte those of
 * flatgfa_parse_bytes (from_stream == 0) or flatgfa_parse_stream_bytes (from_stream != 0) on the same text.  The device
 * judges the plain grammar only -- one H line at most, `S <digits> <seq> [<rest>]`, `L <digits> [+-] <digits> [+-] <cigar>`,
 * `P <name> <steps> <overlaps>` with single commas, every number of at most 32 digits, every name one a segment has --
 * and hands every other text, the same bytes, to the host parser: that parser's handle, or NULL with its message, is then
 * the call's.  flatgfa_parse_device maps the file, as flatgfa_parse does.  NULL with "no HIP device is visible; the device
 * GFA parser has no CPU fallback" without a device (flatgfa_parse_bytes stays the route there); NULL data with len > 0, or a
 * NULL filename: NULL with a message, answered without a device; a device allocation that fails: NULL with HIP's message. */
flatgfa_t flatgfa_parse_bytes_device(const uint8_t *data, size_t len, int from_stream);
flatgfa_t flatgfa_parse_device(const char *filename);
/* The calling thread's last flatgfa_parse_bytes_device / flatgfa_parse_device call that reached a device: out[0] = the
 * route (1: the device made the pools, 0: the host parser), out[1] = why (one of the codes below), out[2] = the bytes of a
 * text tile of the step kernels, out[3] = the tiles of the call's text.  FLATGFA_ERR_ARG for NULL or before such a call. */
enum {
    FLATGFA_PARSE_PLAIN = 0,   /* the device route */
    FLATGFA_PARSE_GRAMMAR = 1, /* a line that is not of the plain forms */
    FLATGFA_PARSE_NAME = 2,    /* a link or a step names no segment, name 0, or a segment id >= 2^31 */
    FLATGFA_PARSE_LIMIT = 3    /* a number of more than 32 digits, or a pool past 2^32 - 1 items */
};
int flatgfa_parse_device_info(uint64_t out[4]);
/* ... and that call's milliseconds: the text's upload; every kernel and scan of the call, by HIP events; of those the two
 * step kernels alone; the pools' download.  What is left of the whole call is the host's: totals read back, allocations,
 * the name map.  Zeros on the host route. */
int flatgfa_parse_device_times(double out[4]);
/* format_float (ops/depth.rs:192-197); returns bytes written (no NUL). */
int flatgfa_format_float(double x, int digits, char *out, int cap);

/* ---- one graph sharded over the GPUs of a node by ONE process ----
 * The reference has no counterpart (it is single-threaded, flatgfa/src/ops/depth.rs:15-39); the
 * semantics are those of the functions above, the sharding is invisible in the results.
 * The graph's steps are cut into n_shards contiguous stretches of near-equal size -- at path
 * boundaries where one lies within an eighth of a shard's share of the even cut, inside a path
 * where none does (fewer paths than shards; a path longer than a shard's share) -- and shard i is
 * made resident on HIP device devices[i] (NULL: shard i on device i mod the device count), with a
 * depth plan, a stream and a host thread of its own.  A query is the local HIP kernels on every
 * shard, ONE all-reduce of the fused [depth | uniq | per-cut-path touch] u32 vector over RCCL
 * (ncclAllReduce, ncclUint32, ncclSum; communicators from ncclCommInitAll), and a fix-up of
 * unique depth for the paths that were cut (depth.rs:30-34 counts a path once per segment however
 * many of its pieces touch it).  librccl.so is loaded on the first create with more than one
 * shard.  Devices may repeat: shards that share a device exchange by device-side adds instead (so
 * does FLATGFA_SHARD_NO_RCCL).  The handle borrows `gfa`, which must outlive it.
 * flags: */
enum {
    FLATGFA_SHARD_WHOLE_PATHS = 1, /* never cut inside a path (shards may then be uneven, or empty) */
    FLATGFA_SHARD_NO_RCCL = 2      /* exchange by peer copies and device-side adds */
};
typedef struct flatgfa_sharded flatgfa_sharded_t;
flatgfa_sharded_t *flatgfa_sharded_create(flatgfa_t gfa, const int *devices, int n_shards, unsigned flags);
void flatgfa_sharded_free(flatgfa_sharded_t *sh);
/* What shard `shard` holds (any out pointer may be NULL): its device, its stretch of the steps
 * pool, the first path it has steps of, how many paths or pieces of paths it walks, how many paths
 * the whole handle cuts, and whether the exchange is RCCL's. */
int flatgfa_sharded_layout(flatgfa_sharded_t *sh, int shard, int *device, uint64_t *step_begin, uint64_t *step_end,
                           uint32_t *first_path, uint32_t *n_pieces, uint32_t *n_split_paths, int *uses_rccl);
/* Bytes every shard contributes to the one collective of a call: 4 per segment for node depth alone;
 * with unique depth 8, plus 4 per segment for every 32 / bits(n_shards) paths that were cut (their
 * touch counters share words: with eight shards, 12 bytes per segment whatever was cut). */
uint64_t flatgfa_sharded_collective_bytes(flatgfa_sharded_t *sh, int with_uniq);
/* seg_depth_with_uniq (depth.rs:15-39) / seg_depth (:45-56) over all shards: results as
 * flatgfa_seg_depth's. */
int flatgfa_sharded_seg_depth(flatgfa_sharded_t *sh, uint64_t *depth_out, uint64_t *uniq_out);
/* path_depth (depth.rs:88-131) for the given path ids: every shard measures its paths (and
 * pieces) against the reduced node depth; the host adds the pieces of a cut path up and divides. */
int flatgfa_sharded_path_depth(flatgfa_sharded_t *sh, const uint32_t *path_ids, uint32_t n_ids, uint64_t *length_out,
                               double *mean_depth_out);
/* The same query in three steps, for callers that time it or overlap it with other work:
 * enqueue (local kernels + collective on every shard's stream; returns without waiting), sync
 * (waits for every shard; FLATGFA_ERR_BOUNDS as flatgfa_dev_status), fetch (the reduced vectors
 * as held by shard `shard` -- every shard holds them). */
int flatgfa_sharded_enqueue(flatgfa_sharded_t *sh, int with_uniq);
int flatgfa_sharded_sync(flatgfa_sharded_t *sh);
int flatgfa_sharded_fetch(flatgfa_sharded_t *sh, int shard, uint64_t *depth_out, uint64_t *uniq_out);
/* How many ranks the handle's exchange really spans: every shard contributes a one to an all-reduce over the
 * handle's communicator (RCCL), or -- shards that exchange by adds -- to the same copies and adds its vectors go
 * through, and every shard reads back its own copy of the sum (FLATGFA_ERR_HIP if they disagree).  Equals
 * n_shards on a handle that works; negative = an error code. */
int flatgfa_sharded_ranks_seen(flatgfa_sharded_t *sh);
/* Where flatgfa_sharded_create would cut a graph whose paths, in path order, have path_steps[p] steps (host only: no
 * device is touched).  cuts_out[r], r = 0 .. n_shards, counts path steps along the path order: shard r walks
 * [cuts_out[r], cuts_out[r + 1]).  Cut r lies at the path boundary nearest to the even cut (total * r / n_shards) when
 * that is within an eighth of a shard's share of it -- or always, with FLATGFA_SHARD_WHOLE_PATHS -- and inside the path
 * otherwise.  This is flatgfa_sharded_create's rule for a graph whose paths' step spans lie in path order in the steps pool
 * (every path's steps behind those of the path before it: what the parser emits, flatgfa/src/parse.rs:149-159); where they do
 * not -- the types allow arbitrary spans -- flatgfa_sharded_create cuts at path boundaries only, as with
 * FLATGFA_SHARD_WHOLE_PATHS.  The rule is computed exactly for any lengths whose total is below 2^64; lengths that add up
 * to 2^64 or more have no u64 cut points and are refused with FLATGFA_ERR_TOO_LARGE. */
int flatgfa_shard_cuts(const uint64_t *path_steps, uint32_t n_paths, int n_shards, unsigned flags, uint64_t *cuts_out);

/* ------------------------------------------------------------------------ */
/* Part 3 -- device-level entry points (caller-owned HBM buffers)           */
/* ------------------------------------------------------------------------ */

/* The graph image the kernels read, all pointers in device memory:
 *   steps       u32[n_steps]   Handle bits, (segment << 1) | orient   (flatgfa.rs:186-209)
 *   path_begin  u32[n_paths]   Path.steps.start                        (flatgfa.rs:106)
 *   path_end    u32[n_paths]   Path.steps.end
 *   seg_len     u32[n_segs]    Segment::len() = seq.end - seq.start    (flatgfa.rs:86-88); may be
 *                              NULL for node depth                                              */
typedef struct flatgfa_dev_graph_t {
    const uint32_t *steps;
    uint64_t n_steps;
    const uint32_t *path_begin;
    const uint32_t *path_end;
    uint32_t n_paths;
    uint32_t n_segs;
    const uint32_t *seg_len;
} flatgfa_dev_graph_t;

/* A prepared depth query over one resident graph image: owns the launch plan (how paths are cut
 * into work items) and the scratch HBM the kernels need, on the device that is current when it
 * is created.  `host_path_begin/host_path_end` are host copies of the span arrays (P entries each);
 * pass NULL to have them copied back from the device.  Returns NULL on failure
 * (flatgfa_last_error()); spans that are reversed or exceed n_steps are rejected here, where the
 * reference would panic on the slice index (pool.rs:341-347).  The plan is laid out for the path
 * spans and the step values it was created with (how many runs each path has decides which
 * kernel walks it; a path that walks the segment ids strictly one way is counted without the
 * per-path "seen" set, and so are the stretches of a path in windows it enters once and walks one way,
 * flatgfa_dev_plan_describe: no_claim_items / no_claim_paths / no_claim_chunks): neither may change while it
 * lives.  Every call still checks the step values against n_segs and its scratch against what the
 * steps need, and reports an error -- or completes the call through the simple kernels -- rather
 * than a wrong answer when they no longer fit; what it does not re-check per step is that a path
 * the plan found strictly monotone still is (a compare per step: 12-18 % of the step scan on a
 * graph of such paths, profiles/NOTES.md R5.8), that a no-claim mark still holds, that the
 * reversed copy of a short downward path still mirrors it, or -- for a plan that reads the steps'
 * run-length image (its description names run_image=<MiB> ... records=kept) -- that the steps are
 * those the image and the run records were made of: such a plan turns the image into records in
 * the first of a row of node-depth calls and counts the calls behind it from those records without
 * reading the steps at all (no answer is kept: every call counts anew, into the caller's buffers;
 * another kind of call, a status that reports anything, or changed steps end the row).  Device memory such a
 * plan holds beside its record buckets: its share of the image (8 bytes a run, one copy for all plans of a
 * step array), 8 bytes an item, and -- where its description says pass2=sorted -- the same records once more,
 * sorted by window, path and start for pass 2 (4 bytes a record and 4 a chunk of 64: sorted_image=<MiB>, 40 at
 * a million segments and 100 M steps; about nine times that transiently while it is made, behind the first
 * answer; plans of one step array over the same paths, a pipeline's lanes among them, share one).  A caller that DOES change step values
 * under a live plan says so with flatgfa_dev_plan_steps_changed (below), which makes the plan
 * again from the steps as they are; FLATGFA_CHECK_NO_CLAIM=1 in the environment (read when a plan
 * is made; a debugging aid, three more reads of the steps per call) re-derives those facts before
 * every call and has flatgfa_dev_status return FLATGFA_ERR_STALE_PLAN where one no longer holds.
 * Creation runs the query a few times into scratch outputs: once to size the record buckets for
 * this graph (so that no later call runs out of room), and, up to 8 M steps, to time the bucketed
 * kernels against the atomic ones and keep the faster.  A graph beyond 16 M segments is walked in
 * ranges of at most 16 M (one pass over the steps per range and call).  What is not needed for the
 * first answer -- the per-block no-claim marks, three more reads of the steps -- is made on a
 * side stream by the first call behind the plan's creation and used from the first call after it
 * is there (flatgfa_dev_plan_describe waits for it; a caller that only wants the first answer never
 * pays for it).
 * Calls on one plan must not overlap in time. */
typedef struct flatgfa_dev_plan flatgfa_dev_plan_t;
flatgfa_dev_plan_t *flatgfa_dev_plan_create(const flatgfa_dev_graph_t *g, const uint32_t *host_path_begin,
                                            const uint32_t *host_path_end);
/* The same, and the first answer with it: the reference's consumers ask ONE depth query per graph
 * (flatgfa/src/cli/cmds.rs:234-285, flatgfa-sh/src/eval/instr.rs:27-72; bench/config.toml:29-32 times
 * a process per query), and the query that sizes the plan's scratch is a whole query -- here it
 * writes the caller's buffers.  depth_out u32[n_segs] (required) and uniq_out u32[n_segs] (or
 * NULL: node depth alone) are device memory and hold seg_depth_with_uniq (ops/depth.rs:15-39) of
 * the graph when the function returns (the device is synchronized).  *first_status (may be NULL):
 * FLATGFA_OK, or FLATGFA_ERR_BOUNDS when a step named a segment id out of range (the counts are
 * then those of the other steps, as after flatgfa_dev_seg_depth + flatgfa_dev_status). */
flatgfa_dev_plan_t *flatgfa_dev_plan_create_first(const flatgfa_dev_graph_t *g, const uint32_t *host_path_begin,
                                                  const uint32_t *host_path_end, uint32_t *depth_out, uint32_t *uniq_out,
                                                  int *first_status);
void flatgfa_dev_plan_destroy(flatgfa_dev_plan_t *plan);
/* A plan that goes leaves its record buckets (the one large device allocation it had: half a gigabyte at cfg-L) with the library for
 * the next plan of the device to take, because allocating and freeing gigabytes of device memory in a row is what the driver does worst
 * (a plan made beside five that stay: 5 ms, or every other time 80-300 ms; with the array kept 4.8 ms every time).  One array per
 * device, the largest seen, at most 8 GB.  This gives them back to the device; call it when no plan will be made for a while. */
void flatgfa_dev_release_scratch(void);
/* The step values (not the spans) of the plan's graph image were changed by the caller: waits for
 * `stream` (the plan's), then makes the plan's launch plan and scratch again from the steps as they
 * are -- which kernel walks which path, the reversed copies, which paths and blocks need no claim,
 * the record buckets' sizes, the overlap query's bitmaps -- at the cost of creating it.  The
 * reference's pools are immutable while a query runs (flatgfa/src/ops/depth.rs:30-34 reads them
 * as they are); this is how a caller who owns the HBM buffers keeps that true of a plan. */
int flatgfa_dev_plan_steps_changed(flatgfa_dev_plan_t *plan, void *stream);

/* Node depth on device: seg_depth_with_uniq (ops/depth.rs:15-39) when uniq_out != NULL, seg_depth
 * (depth.rs:45-56) when NULL.  depth_out / uniq_out are u32[n_segs] in device memory.  Enqueues on
 * `stream` (a hipStream_t; NULL = the default stream) and returns without synchronizing. */
int flatgfa_dev_seg_depth(flatgfa_dev_plan_t *plan, uint32_t *depth_out, uint32_t *uniq_out, void *stream);
/* Per-path sums on device given depth u32[n_segs] (measure_path, ops/depth.rs:116-131):
 * length_out[k] = sum seg_len, weighted_out[k] = sum depth*seg_len over the steps of path
 * path_ids[k] (u32[n_ids], device memory), both u64 wrapping like Rust usize.  The single f64
 * division per path is left to the host. */
int flatgfa_dev_path_sums(flatgfa_dev_plan_t *plan, const uint32_t *path_ids, uint32_t n_ids, const uint32_t *depth,
                          uint64_t *length_out, uint64_t *weighted_out, void *stream);
/* path_depth for ALL paths of the plan in one go (ops/depth.rs:88-111 with every path requested --
 * what `fgfa depth` prints, cmds.rs:256-262): node depth into depth_out u32[n_segs], and per path
 * the two integer sums of measure_path into length_out / weighted_out u64[n_paths] (device
 * memory), indexed by path.  The sums of the paths the step-scan kernel walks are formed in the
 * same pass that accumulates node depth -- a run of segments contributes two differences of
 * window-local prefix sums -- so the steps are read once.  As with flatgfa_path_depth, every path's
 * sums must stay below 2^64; the 64-bit intermediate values (a window's prefix sums over all paths
 * among them) wrap and their differences stay exact. */
int flatgfa_dev_path_depth_all(flatgfa_dev_plan_t *plan, uint32_t *depth_out, uint64_t *length_out,
                               uint64_t *weighted_out, void *stream);
/* Path-pair overlap on device (slow_odgi/slow_odgi/overlap.py:6-14): touch_out[k * n_paths + j] = 1
 * iff path j is a different path from path_ids[k] and the two share at least one ORIENTED handle.
 * query_ids u32[n_q] and touch_out u8[n_q * n_paths] are device memory.  A coarse bitmap per path
 * (one bit per 2048 handles) is built on the first call and kept with the plan; exact handle
 * bitsets are built for the query paths only, per call -- memory follows the queries, not the
 * number of paths.  A graph of more than 2^28 segments (n_segs > 268435456) is refused with
 * FLATGFA_ERR_TOO_LARGE before anything is written; one of 0 segments gives all zeros. */
int flatgfa_dev_path_overlaps(flatgfa_dev_plan_t *plan, const uint32_t *query_ids, uint32_t n_q, uint8_t *touch_out,
                              void *stream);
/* One pangenotype row on device (as flatgfa_pangenotype_matrix, for one piece of text): d_text[0, len) is
 * GAF text in device memory of the current device, made of whole lines (what follows its last '\n' is
 * ignored).  The segments it names are OR-ed into d_row (ceil(S / 64) u64 words, bit s & 63 of word s >> 6),
 * so a caller may feed a file in pieces of its own; a name the graph does not have lowers *d_first_bad
 * (atomic min) to the offset of its line in d_text.  The graph's name table is built on the first call
 * for the device and kept with the handle.  Enqueued on `stream`; returns without waiting. */
int flatgfa_dev_pangenotype_row(flatgfa_t gfa, const uint8_t *d_text, size_t len, uint64_t *d_row, uint64_t *d_first_bad,
                                void *stream);
/* The GAF lookup on device text (as flatgfa_gaf_events and flatgfa_gaf_seqs, for one piece of text), in two calls.
 * flatgfa_dev_gaf_count: d_text[0, len) is GAF text in device memory of the current device, at any alignment, made of
 * whole lines (what follows its last '\n' is ignored).  It indexes the lines, parses them, forms every event and, with
 * seqs != 0, lays out the `-s` text; it waits for `stream` to read the totals -- *n_lines, *n_events and *seq_bytes (the
 * length of the `-s` text; 0 without seqs) -- and checks them: errors as flatgfa_gaf_events' (and, with seqs,
 * flatgfa_gaf_seqs'), offsets counted in d_text.  *job must be NULL, or a job of an earlier call whose scratch is then
 * used again.  flatgfa_dev_gaf_fill enqueues on `stream` the copies into caller memory (device; any pointer may be NULL):
 * line_first u64[n_lines + 1], line_end u64[n_lines] (the offset of each line's '\n': a line, and its name, start behind
 * the one before), name_len u64[n_lines], handle u32 / kind u8 / a, b u64 [n_events], and the gather of the `-s` text
 * into seq_text u8[seq_bytes].  d_text must stay as it is until the fill is done.  The graph's name table and sequence
 * pool are made on the first call for the device and kept with the handle.  flatgfa_dev_gaf_free waits for the job's
 * stream and releases its scratch. */
typedef struct flatgfa_dev_gaf flatgfa_dev_gaf_t;
int flatgfa_dev_gaf_count(flatgfa_t gfa, const uint8_t *d_text, size_t len, int seqs, void *stream, flatgfa_dev_gaf_t **job,
                          uint64_t *n_lines, uint64_t *n_events, uint64_t *seq_bytes);
int flatgfa_dev_gaf_fill(flatgfa_dev_gaf_t *job, uint64_t *line_first, uint64_t *line_end, uint64_t *name_len, uint32_t *handle,
                         uint8_t *kind, uint64_t *a, uint64_t *b, uint8_t *seq_text, void *stream);
void flatgfa_dev_gaf_free(flatgfa_dev_gaf_t *job);
/* chop (flatgfa_chop, without links) of a graph image in device memory, in two stream-ordered calls.
 * flatgfa_dev_chop_count checks the image (g->seg_len is required: FLATGFA_ERR_ARG when NULL), scans the piece
 * counts, waits for `stream` once to read the totals -- *n_segs_out new segments, *n_steps_out new steps -- and, when
 * they fit 32-bit ids, enqueues seg_first u32[n_segs + 1] (device memory: old segment s became the new segments
 * [seg_first[s], seg_first[s + 1])) and returns a job in *job; errors as flatgfa_chop's, with no job.
 * flatgfa_dev_chop_fill enqueues on `stream` the chopped image into caller memory: steps u32[*n_steps_out],
 * path_begin / path_end u32[n_paths] and seg_len u32[*n_segs_out] -- together a flatgfa_dev_graph_t of n_paths
 * paths and *n_segs_out segments that flatgfa_dev_plan_create takes.  Path spans may be any spans (overlapping ones
 * too); the new steps are the paths' expansions in path order.  g's arrays and seg_first must stay as they are until
 * the fill is done.  flatgfa_dev_chop_free waits for the job's stream and releases its scratch. */
typedef struct flatgfa_dev_chop flatgfa_dev_chop_t;
int flatgfa_dev_chop_count(const flatgfa_dev_graph_t *g, uint64_t max_size, uint32_t *seg_first, void *stream, flatgfa_dev_chop_t **job,
                           uint64_t *n_segs_out, uint64_t *n_steps_out);
int flatgfa_dev_chop_fill(flatgfa_dev_chop_t *job, uint32_t *steps, uint32_t *path_begin, uint32_t *path_end, uint32_t *seg_len,
                          void *stream);
void flatgfa_dev_chop_free(flatgfa_dev_chop_t *job);
/* inject (flatgfa_inject, without links or names) of a graph image in device memory, in two stream-ordered calls modelled on
 * the chop pair.  d_path_id u32[n], d_start / d_end u64[n] are the lines, in device memory.  flatgfa_dev_inject_count
 * checks the image (g->seg_len is required) and the lines, builds the cut table, waits for `stream` once to read the totals
 * -- *n_segs_out new segments, *n_steps_out new steps, *n_paths_out = g->n_paths + n paths -- and, when they fit 32-bit
 * ids, enqueues seg_first u32[n_segs + 1] and returns a job; errors as flatgfa_inject's, with no job.
 * flatgfa_dev_inject_fill enqueues the new image into caller memory: steps u32[*n_steps_out], path_begin / path_end
 * u32[*n_paths_out] (the old paths, then one per line) and seg_len u32[*n_segs_out] -- a flatgfa_dev_graph_t that
 * flatgfa_dev_plan_create takes.  g's arrays, the lines and seg_first must stay as they are until the fill is done; nothing is
 * held per call outside the job.  flatgfa_dev_inject_free waits for the job's stream and releases its scratch. */
typedef struct flatgfa_dev_inject flatgfa_dev_inject_t;
int flatgfa_dev_inject_count(const flatgfa_dev_graph_t *g, const uint32_t *d_path_id, const uint64_t *d_start, const uint64_t *d_end, uint64_t n,
                             uint32_t *seg_first, void *stream, flatgfa_dev_inject_t **job, uint64_t *n_segs_out, uint64_t *n_steps_out,
                             uint64_t *n_paths_out);
int flatgfa_dev_inject_fill(flatgfa_dev_inject_t *job, uint32_t *steps, uint32_t *path_begin, uint32_t *path_end, uint32_t *seg_len,
                            void *stream);
void flatgfa_dev_inject_free(flatgfa_dev_inject_t *job);
/* crush (flatgfa_crush) of a sequence pool in device memory, in two stream-ordered calls modelled on the chop pair.  seg_seq
 * u32[2 * n_segs] holds each segment's start in seq_data and its length, as the GAF lookup keeps them; seq_data u8[seq_len].
 * n_segs == 0 and seq_len == 0 are valid (the pointers may then be NULL).  flatgfa_dev_crush_count checks the spans, counts
 * what is kept, waits for `stream` once to read the totals -- *bytes_out kept bytes, *dropped_out dropped ones -- and, when
 * the kept bytes fit a 32-bit span, enqueues seg_len_out u32[n_segs] (the new lengths: put in place of a
 * flatgfa_dev_graph_t's seg_len they give the crushed graph's image, the steps and path spans shared) and returns a job in
 * *job; a span that leaves seq_data: FLATGFA_ERR_BOUNDS, more than 2^32 - 1 kept bytes: FLATGFA_ERR_TOO_LARGE, both with no
 * job and nothing written.  flatgfa_dev_crush_fill enqueues on `stream` the new pool into seq_out u8[*bytes_out] (at any
 * alignment) and the new spans into seg_seq_out u32[2 * n_segs] (start, length; segment s starts at the sum of the new
 * lengths before s, empty or not), and does not wait.  seg_seq and seq_data must stay as they are until the fill is done.
 * flatgfa_dev_crush_free waits for the job's stream and releases its scratch. */
typedef struct flatgfa_dev_crush flatgfa_dev_crush_t;
int flatgfa_dev_crush_count(const uint32_t *seg_seq, const uint8_t *seq_data, uint64_t seq_len, uint32_t n_segs, uint32_t *seg_len_out,
                            void *stream, flatgfa_dev_crush_t **job, uint64_t *bytes_out, uint64_t *dropped_out);
int flatgfa_dev_crush_fill(flatgfa_dev_crush_t *job, uint8_t *seq_out, uint32_t *seg_seq_out, void *stream);
void flatgfa_dev_crush_free(flatgfa_dev_crush_t *job);
/* flip (flatgfa_flip) of a graph image in device memory, in two stream-ordered calls modelled on the crush pair.  Path p walks
 * steps[path_begin[p] .. path_begin[p] + n_p) of steps u32[n_steps], n_p = path_start[p + 1] - path_start[p]: path_start
 * u32[n_paths + 1] numbers the steps of all paths one behind another, from 0 to n_lin, while the spans themselves may be out
 * of order, overlap or leave gaps.  seg_len u32[n_segs]; links u32[4 * n_links] are the Link records (from, to,
 * overlap.start, overlap.end) and alignment u32[n_align] the pool their overlaps point into.  Empty pools may be NULL.
 * flatgfa_dev_flip_count checks ids and spans, weighs the paths, forms and de-duplicates the links, waits for `stream` once
 * to read the totals -- *n_turned turned paths, *links_out links kept, *links_new of them new -- and returns a job in *job;
 * an id or span out of range: FLATGFA_ERR_BOUNDS, n_links + n_lin > 2^32 - 2: FLATGFA_ERR_TOO_LARGE, both with no job.
 * round_keys is 0 (2^26) or, for tests and measurements, how many keys of the link table a round takes: where n_links + n_lin
 * is more than two rounds' keys, the table is grouped and decided a round at a time in scratch for two rounds' keys -- the
 * answer is the same -- and more links and step pairs on one handle than a round holds are FLATGFA_ERR_TOO_LARGE.
 * flatgfa_dev_flip_fill enqueues on `stream` the new steps into steps_out u32[n_lin] (path p at [path_start[p],
 * path_start[p + 1]): with path_start as begins and ends it is a flatgfa_dev_graph_t's image), the flags into turned_out
 * u32[n_paths] (0 or 1) and the kept Link records into links_out u32[4 * *links_out] -- the old ones first, with their
 * spans; a new one's overlap is [n_align, n_align + 1), the 0M op (the word 0) that the caller appends to its alignment pool
 * when *links_new is not 0 -- and does not wait.  The inputs must stay as they are until the fill is done.
 * flatgfa_dev_flip_free waits for the job's stream and releases its scratch. */
typedef struct flatgfa_dev_flip flatgfa_dev_flip_t;
int flatgfa_dev_flip_count(const uint32_t *steps, uint64_t n_steps, const uint32_t *path_start, const uint32_t *path_begin, uint32_t n_paths,
                           uint64_t n_lin, const uint32_t *seg_len, uint32_t n_segs, const uint32_t *links, uint64_t n_links,
                           const uint32_t *alignment, uint64_t n_align, uint64_t round_keys, void *stream, flatgfa_dev_flip_t **job, uint64_t *n_turned,
                           uint64_t *links_out, uint64_t *links_new);
int flatgfa_dev_flip_fill(flatgfa_dev_flip_t *job, uint32_t *steps_out, uint32_t *turned_out, uint32_t *links_out, void *stream);
void flatgfa_dev_flip_free(flatgfa_dev_flip_t *job);
/* The packed-sequence codec (flatgfa_seq_export, flatgfa_seq_import) on text and packed bytes in device memory; offsets and
 * counts are 64-bit throughout.  flatgfa_dev_seq_pack_count classifies text[0, n) (at any alignment; n == 0 with NULL is
 * valid), counts the kept bases, waits for `stream` once and returns a job in *job and the count in *n_bases; a byte that is
 * neither whitespace nor one of A C T G: FLATGFA_ERR_PARSE with no job, flatgfa_last_error naming the smallest such offset.
 * flatgfa_dev_seq_pack_fill enqueues on `stream` the packed bytes of "the carry, then the kept bases" into out (at any
 * alignment): carry is -1 for none or a code 0..3 that takes the first low nibble (what a caller who cuts its text in pieces
 * holds back from the piece before); out is u8[(*n_bases + (carry >= 0) + 1) / 2], every byte of it written exactly once,
 * the unused last high nibble as 0, and nothing beside it.  It does not wait; the text must stay as it was until it has run.
 * flatgfa_dev_seq_pack_free waits for the job's stream and releases its scratch.  flatgfa_dev_seq_unpack writes the letters of
 * the first n_bases nibbles of `packed` into text_out u8[n_bases] (any alignment; 16-byte loads and stores where both are
 * 16-byte aligned) and waits for `stream` once: a nibble above 3 among them is FLATGFA_ERR_PARSE, flatgfa_last_error naming
 * the smallest such base index; the unused high nibble of an odd count's last byte is not looked at. */
typedef struct flatgfa_dev_seq_pack flatgfa_dev_seq_pack_t;
int flatgfa_dev_seq_pack_count(const uint8_t *text, uint64_t n, void *stream, flatgfa_dev_seq_pack_t **job, uint64_t *n_bases);
int flatgfa_dev_seq_pack_fill(flatgfa_dev_seq_pack_t *job, int carry, uint8_t *out, void *stream);
void flatgfa_dev_seq_pack_free(flatgfa_dev_seq_pack_t *job);
int flatgfa_dev_seq_unpack(const uint8_t *packed, uint64_t n_bases, uint8_t *text_out, void *stream);
/* BED intersection (flatgfa_bed_intersect, without names or text) of entries in device memory.  Entry i of a side has the
 * name id id[i] and the interval [start[i], end[i]).  b's ids are below n_groups and never decrease (b is grouped by name,
 * file order kept inside a group); a's ids are below n_groups, or 0xFFFFFFFF for a name b does not have; anything else:
 * FLATGFA_ERR_BOUNDS, with no job.  Either side may be empty (its pointers may then be NULL); 2^32 - 1 entries or more on a
 * side: FLATGFA_ERR_BOUNDS.  flatgfa_dev_bed_begin finds the groups and every a entry's candidate range, waits for `stream`
 * once and returns a job in *job, the number of candidate pairs, the number of rounds they are cut into -- round_cands
 * candidates each, 0 for the library's own size -- and the number of groups that are walked whole.  flatgfa_dev_bed_round
 * writes the hits of round `round` in the reference's order into caller memory with room for min(round_cands, *candidates)
 * records each -- a_index and b_index (the entries' indices as given), start = max of the starts, end = min of the ends --
 * and waits for the job's stream to return their number in *n_hits.  Rounds may be asked for in any order, one at a time.
 * The sides' arrays must stay as they are until the job is freed.  flatgfa_dev_bed_free waits for the job's stream and
 * releases its scratch. */
typedef struct flatgfa_dev_bed flatgfa_dev_bed_t;
int flatgfa_dev_bed_begin(const uint32_t *a_id, const uint64_t *a_start, const uint64_t *a_end, uint64_t n_a, const uint32_t *b_id,
                          const uint64_t *b_start, const uint64_t *b_end, uint64_t n_b, uint32_t n_groups, uint64_t round_cands, void *stream,
                          flatgfa_dev_bed_t **job, uint64_t *candidates, uint64_t *rounds, uint64_t *unsorted_groups);
int flatgfa_dev_bed_round(flatgfa_dev_bed_t *job, uint64_t round, uint32_t *a_index, uint32_t *b_index, uint64_t *start, uint64_t *end,
                          uint64_t *n_hits);
void flatgfa_dev_bed_free(flatgfa_dev_bed_t *job);
/* The legend of flatten (flatten.py:13-19; flatgfa_flatten_legend) of a graph image in device memory: d_offset_out[s] = the
 * sum of g->seg_len before s, d_offset_out[n_segs] = the sum of all, in 64 bits (g->seg_len is required: FLATGFA_ERR_ARG when
 * NULL; the steps and spans are not read).  Enqueued on `stream`, which is waited for: the scan's scratch goes before the
 * call returns. */
int flatgfa_dev_flatten_legend(const flatgfa_dev_graph_t *g, uint64_t *d_offset_out /* device, [n_segs + 1] */, void *stream);
/* Synchronizes `stream`, then returns FLATGFA_OK, or FLATGFA_ERR_BOUNDS if any kernel since the
 * last call saw a segment id >= n_segs or a path id >= n_paths.  Plans size their scratch for the
 * graph when they are created; should a node-depth call nevertheless have run out of scratch room
 * (the step values changed behind the plan's back), this call runs it again on a larger plan
 * before it returns, into the same output buffers -- which therefore must not have been
 * modified in between.  Only the last call can be completed that way: if several node-depth calls
 * were enqueued since the last status and one of them ran out of room, this returns
 * FLATGFA_ERR_HIP (call status after every call where step values may change behind a plan).
 * A plan belongs to ONE stream: every call of the plan, and this one, must be enqueued on the same
 * stream (this call may release and reallocate the plan's scratch once that stream is idle). */
int flatgfa_dev_status(flatgfa_dev_plan_t *plan, void *stream);

/* Calls in flight.  A plan's calls run one after the other on its one stream, and a call is two kernels with
 * opposite needs: pass 1 is bound by the memory system, pass 2 by instruction issue, each wants the whole chip, and
 * each leaves compute units idle at its end.  A pipeline is `calls_in_flight` plans of ONE resident graph (they share
 * the graph image and its claim on the Infinity Cache; each has its own record scratch) on as many internal streams,
 * taken in turn, and each lane's pass 1 runs on fewer persistent workgroups than there are compute units (half of
 * them with three calls in flight or more on graphs of up to 2^28 steps, eleven sixteenths otherwise), so that the
 * other calls' kernels share the chip with it all the time, not only at its tail (1 M segments / 100 M steps: 0.133 ms
 * per call one at a time, 0.114 with two in flight, 0.107 with three; a fourth loses).  A lane's plan alone would be
 * slower than flatgfa_dev_plan_create's.  Every call is a whole query into the caller's buffers,
 * which must not be reused before the call that wrote them is known to be done (join, or status).
 *   flatgfa_dev_pipeline_seg_depth   as flatgfa_dev_seg_depth, on the pipeline's next lane; returns without waiting.
 *                                    The call first waits for everything enqueued so far on `after_stream` (the
 *                                    stream that filled the graph image or consumed the buffers' previous contents;
 *                                    NULL = the default stream), or for nothing when after_stream is (void *)-1.
 *   flatgfa_dev_pipeline_path_depth_all   as flatgfa_dev_path_depth_all (what `fgfa depth` prints), likewise.
 *   flatgfa_dev_pipeline_join        makes `stream` wait for every call enqueued so far (events; no host wait).
 *   flatgfa_dev_pipeline_status      waits for every lane; FLATGFA_ERR_BOUNDS etc. as flatgfa_dev_status. */
typedef struct flatgfa_dev_pipeline flatgfa_dev_pipeline_t;
flatgfa_dev_pipeline_t *flatgfa_dev_pipeline_create(const flatgfa_dev_graph_t *g, const uint32_t *host_path_begin,
                                                    const uint32_t *host_path_end, int calls_in_flight);
void flatgfa_dev_pipeline_destroy(flatgfa_dev_pipeline_t *p);
int flatgfa_dev_pipeline_seg_depth(flatgfa_dev_pipeline_t *p, uint32_t *depth_out, uint32_t *uniq_out, void *after_stream);
int flatgfa_dev_pipeline_path_depth_all(flatgfa_dev_pipeline_t *p, uint32_t *depth_out, uint64_t *length_out, uint64_t *weighted_out,
                                        void *after_stream);
int flatgfa_dev_pipeline_join(flatgfa_dev_pipeline_t *p, void *stream);
int flatgfa_dev_pipeline_status(flatgfa_dev_pipeline_t *p);
/* flatgfa_dev_plan_steps_changed for every lane (waits for all of them first). */
int flatgfa_dev_pipeline_steps_changed(flatgfa_dev_pipeline_t *p);
int flatgfa_dev_pipeline_describe(flatgfa_dev_pipeline_t *p, char *out, int cap);

/* Which kernels this plan's calls run -- the choices made when it was created, some of them by
 * timing on the graph -- as a line of `key=value` words; returns the bytes written (NUL excluded). */
int flatgfa_dev_plan_describe(flatgfa_dev_plan_t *plan, char *out, int cap);

/* Kernel-level timing for bench.py: when enabled, every kernel the library launches is bracketed
 * by HIP events on its own stream; flatgfa_dev_profile_read synchronizes and returns, for up to
 * `cap` kernels since the last read, the kernel name and elapsed milliseconds. */
void flatgfa_dev_profile_enable(int on);
int flatgfa_dev_profile_read(const char **names, float *ms, int cap);
/* What such an event pair reads around a kernel that does nothing, launched with `n_workgroups`
 * workgroups of 1024 threads and `lds_bytes` of dynamic LDS (median of `reps`; < 0 on error):
 * the part of a profiled kernel's time that rocprofv3's dispatch duration does not contain. */
float flatgfa_dev_profile_overhead_ms(int n_workgroups, int lds_bytes, int reps, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* FLATGFA_H */
