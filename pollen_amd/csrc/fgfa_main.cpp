// `fgfa` -- the slice of the reference CLI that sits on the depth path
// (cucapra/pollen flatgfa/src/cli/main.rs:9-55, cmds.rs:16-97,217-285), built on the C ABI:
//
//   fgfa [-i FILE.flatgfa | -I FILE.gfa] [-D] [-o OUT.flatgfa] [-O OUT.gfa] [COMMAND]
//   COMMAND: toc [-b] | paths | stats -S | depth [-d] [-r NAME]... [-b FILE.bed] [--bed-paths FILE.bed] [-s PATHS]
//            | window-depth PATH SIZE | window-depth-all SIZE | overlap --paths FILE | matrix GAF | gaf GAF [-s] [-b] [-p] | chop -c N [-l] | inject -b BED [-l] | crush | flip
//            | extract -n NAME -c DIST [-d N] [-e N] | position -p PATH,OFFSET,+ | validate | degree
//            | flatten [-n NAME] [-f FASTA] [-b BED] | print [-O OUT.gfa]
//   fgfa seq-export INPUT OUTPUT | fgfa seq-import FILE | fgfa bed -a FILE -b FILE        (no graph is read)
//
// With no -i/-I the GFA text is read from stdin; with -D that text, or -I's, is parsed on the GPU (the same graph; a text that
// is not of the plain grammar goes to the host parser; without a device: an error); with no COMMAND the graph is written out
// (-o binary, -O text, otherwise text on stdout).  `depth` output is byte-identical to the
// reference's and is computed on the GPU, as are `matrix` (cmds.rs:453-475), `position` (cmds.rs:105-152), and `chop`
// (cli/main.rs:139-159) and `extract` (cmds.rs:174-215), whose graph is written out as the input graph would be; `validate` and `degree` print what slow_odgi's validate.py and
// degree.py print, `crush` writes out the graph of its crush.py, `flip` that of its flip.py, `flatten` what its flatten.py prints (or, with -f / -b, what `odgi flatten` writes to those files).
// `seq-export` and `seq-import` (cmds.rs:415-452) are the packed-sequence codec of packedseq.rs, on the GPU as well; like the
// reference's they take files, not a graph, and stdin is never read.  So does `bed` (cmds.rs:378-413, bed-intersect): the lines
// of -b that lie under the intervals of -a, found and printed on the GPU.  Of the reference CLI that leaves `bench`.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/flatgfa.h"

static inline const char *test_hook(const char *name) { return getenv(name); }  // (a test hook, not a user-facing switch: device_common.hpp)

static int die(const char *what) {
    fprintf(stderr, "fgfa: %s: %s\n", what, flatgfa_last_error());
    return 1;
}

// One name per line (blank lines skipped), as slow_odgi's parse_paths does.
static bool read_names(const char *file, std::vector<std::string> *out) {
    FILE *f = fopen(file, "rb");
    if (!f) return false;
    std::string cur;
    int c;
    while ((c = fgetc(f)) != EOF) {
        if (c == '\n') {
            if (!cur.empty()) out->push_back(cur);
            cur.clear();
        } else if (c != '\r') {
            cur.push_back((char)c);
        }
    }
    if (!cur.empty()) out->push_back(cur);
    fclose(f);
    return true;
}

// flatgfa_sink_t over a file descriptor (ctx: the int); a short or failed write stops the call
static int write_fd(void *ctx, const char *p, size_t n) {
    while (n) {
        const ssize_t w = write(*static_cast<int *>(ctx), p, n);
        if (w <= 0) return 1;
        p += w;
        n -= (size_t)w;
    }
    return 0;
}

// flatgfa_sink_t of the GFA text: stdout, or a file that is made when the first piece arrives -- the text has been checked by
// then, so that a print error leaves no file behind
struct TextOut {
    const char *file;
    int fd = -1;
    bool failed = false;
};
static int write_text(void *ctx, const char *p, size_t n) {
    TextOut *o = static_cast<TextOut *>(ctx);
    if (o->fd < 0 && (o->fd = o->file ? open(o->file, O_WRONLY | O_CREAT | O_TRUNC, 0666) : STDOUT_FILENO) < 0) o->failed = true;
    if (o->fd < 0 || write_fd(&o->fd, p, n)) return o->failed = true, 1;
    return 0;
}

static void write_all(const char *p, size_t n) {
    while (n) {
        ssize_t w = write(STDOUT_FILENO, p, n);
        if (w <= 0) exit(1);
        p += w;
        n -= (size_t)w;
    }
}

int main(int argc, char **argv) {
    const char *in_flat = nullptr, *in_gfa = nullptr, *out_flat = nullptr, *out_gfa = nullptr, *prealloc = nullptr;
    bool device_parse = false;  // -D: the text of -I FILE, or of stdin, is parsed on the device
    bool mutate = false;  // -m: with -o, write the preallocated container (cli/main.rs:88-96); with -i, open for mutation (read the same way here)
    int i = 1;
    for (; i < argc; ++i) {
        std::string a = argv[i];
        auto need = [&](const char **dst) {
            if (i + 1 >= argc) { fprintf(stderr, "fgfa: %s needs a value\n", a.c_str()); exit(2); }
            *dst = argv[++i];
        };
        if (a == "-i") need(&in_flat);
        else if (a == "-I") need(&in_gfa);
        else if (a == "-o") need(&out_flat);
        else if (a == "-O") need(&out_gfa);
        else if (a == "-m") mutate = true;
        else if (a == "-D") device_parse = true;
        else if (a == "-p") need(&prealloc);
        else break;
    }
    std::string cmd = i < argc ? argv[i++] : "";
    if (device_parse && in_flat) {
        fprintf(stderr, "usage: fgfa -D parses GFA text (-I FILE, or stdin): it does not go with -i\n");
        return 2;
    }

    // The special case the reference's main starts with (cli/main.rs:61-66): `-m -o OUT` with no command and
    // no -i is prealloc_translate -- GFA text (the mapped -I file, or stdin) parsed straight into the mapped,
    // preallocated output; no graph is built.
    if (mutate && cmd.empty() && !in_flat && out_flat) {
        const uint32_t factor = prealloc ? (uint32_t)strtoul(prealloc, nullptr, 10) : 32u;
        int rc;
        if (in_gfa) {
            const int fd = open(in_gfa, O_RDONLY);
            struct stat sb;
            if (fd < 0 || fstat(fd, &sb) != 0) { fprintf(stderr, "fgfa: cannot open %s\n", in_gfa); return 1; }
            void *m = sb.st_size ? mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, fd, 0) : nullptr;
            close(fd);
            if (m == MAP_FAILED) { fprintf(stderr, "fgfa: cannot map %s\n", in_gfa); return 1; }
            rc = flatgfa_translate_prealloc((const uint8_t *)m, (size_t)sb.st_size, 0, out_flat, factor);
            if (m) munmap(m, (size_t)sb.st_size);
        } else {
            std::string buf;
            char tmp[1 << 16];
            ssize_t r;
            while ((r = read(STDIN_FILENO, tmp, sizeof tmp)) > 0) buf.append(tmp, (size_t)r);
            rc = flatgfa_translate_prealloc((const uint8_t *)buf.data(), buf.size(), 1, out_flat, factor);
        }
        return rc ? die("write") : 0;
    }

    // A one-shot query is mostly start-up: the HIP runtime takes a tenth of a second and more to come
    // up in a cold process, the staging buffers, the first copy and the first launch another thirty
    // milliseconds.  All of that starts now, on a thread of its own, while this one maps or parses
    // the graph (and, for a mapped file, has the kernel map the step pool's pages in).
    const bool wants_device = device_parse || cmd == "depth" || cmd == "window-depth" || cmd == "window-depth-all" || cmd == "overlap" || cmd == "matrix" || cmd == "gaf" || cmd == "chop" || cmd == "inject" || cmd == "crush" || cmd == "flip" || cmd == "extract" || cmd == "position" || cmd == "validate" || cmd == "degree" || cmd == "flatten" || cmd == "print" || cmd == "seq-export" || cmd == "seq-import" || cmd == "bed";
    // (`fgfa` only ever uses device 0: on a node with several GPUs the runtime need not bring the others up.  Set
    // before the first HIP call; a caller's or scheduler's own choice of visible devices -- by any of the variables the
    // HIP runtime honours: CUDA_VISIBLE_DEVICES and GPU_DEVICE_ORDINAL index into what ROCr exposes, so narrowing
    // ROCr to device 0 under them would hide the assigned GPU -- is left alone.)
    bool pinned = false;
    for (const char *v : {"ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "GPU_DEVICE_ORDINAL"}) pinned = pinned || getenv(v) != nullptr;
    if (wants_device && !pinned) (void)setenv("ROCR_VISIBLE_DEVICES", "0", 0);
    // (freed host memory stays with the process: an unmapped buffer costs the next launch or copy 10-30 ms on this driver, flatgfa.h)
    if (const char *k = getenv("FLATGFA_KEEP_HOST_MEMORY"); !(k && k[0] == '0')) (void)flatgfa_keep_host_memory(1);
    std::thread warm;
    if (wants_device && !getenv("FLATGFA_NO_WARM")) warm = std::thread([] { (void)flatgfa_warm_device(0); });

    // cli/cmds.rs:415-452: fgfa seq-export INPUT OUTPUT, fgfa seq-import FILE -- before any graph is loaded: neither reads one
    if (cmd == "seq-export" || cmd == "seq-import") {
        const bool exporting = cmd == "seq-export";
        int rc = 0;
        if (argc - i != (exporting ? 2 : 1)) {
            fprintf(stderr, exporting ? "usage: fgfa seq-export INPUT OUTPUT\n" : "usage: fgfa seq-import FILE\n");
            rc = 2;
        } else {
            const int fd = open(argv[i], O_RDONLY);
            struct stat sb;
            void *m = nullptr;
            size_t n = 0;
            if (fd < 0 || fstat(fd, &sb) != 0) {
                fprintf(stderr, "fgfa: cannot open %s\n", argv[i]);
                rc = 1;
            } else if ((n = (size_t)sb.st_size) && (m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0)) == MAP_FAILED) {
                fprintf(stderr, "fgfa: cannot map %s\n", argv[i]);
                rc = 1;
            }
            if (fd >= 0) close(fd);
            if (!rc && m) (void)madvise(m, n, MADV_SEQUENTIAL);
            if (!rc && exporting) {
                if (flatgfa_seq_export_file((const uint8_t *)m, n, argv[i + 1])) rc = die("seq-export");
            } else if (!rc) {
                // the bases, then one newline (cmds.rs:427-429); checked whole before a byte is printed
                char *text = nullptr;
                size_t len = 0;
                if (flatgfa_seq_import((const uint8_t *)m, n, &text, &len)) {
                    rc = die("seq-import");
                } else {
                    write_all(text, len);
                    write_all("\n", 1);
                }
                flatgfa_free_text(text);
            }
        }
        if (warm.joinable()) warm.join();
        fflush(stdout);
        fflush(stderr);
        if (!test_hook("FLATGFA_SLOW_EXIT")) _exit(rc);
        return rc;
    }

    // cli/cmds.rs:378-413: fgfa bed -a FILE -b FILE -- before any graph is loaded too; both files are mapped, the text goes to
    // stdout as it streams
    if (cmd == "bed") {
        const char *file[2] = {nullptr, nullptr};
        bool bad = false;
        for (; i < argc; ++i) {
            const int k = !strcmp(argv[i], "-a") ? 0 : !strcmp(argv[i], "-b") ? 1 : -1;
            if (k < 0 || i + 1 >= argc || file[k]) { bad = true; break; }
            file[k] = argv[++i];
        }
        int rc = 0;
        void *m[2] = {nullptr, nullptr};
        size_t n[2] = {0, 0};
        if (bad || !file[0] || !file[1]) {
            fprintf(stderr, "usage: fgfa bed -a FILE -b FILE\n");
            rc = 2;
        }
        for (int k = 0; k < 2 && !rc; ++k) {
            const int fd = open(file[k], O_RDONLY);
            struct stat sb;
            if (fd < 0 || fstat(fd, &sb) != 0) {
                fprintf(stderr, "fgfa: cannot open %s\n", file[k]);
                rc = 1;
            } else if ((n[k] = (size_t)sb.st_size) && (m[k] = mmap(nullptr, n[k], PROT_READ, MAP_PRIVATE, fd, 0)) == MAP_FAILED) {
                fprintf(stderr, "fgfa: cannot map %s\n", file[k]);
                rc = 1;
            }
            if (fd >= 0) close(fd);
            if (!rc && m[k]) (void)madvise(m[k], n[k], MADV_SEQUENTIAL);
        }
        if (warm.joinable()) warm.join();
        int out = STDOUT_FILENO;
        if (!rc && flatgfa_bed_intersect_stream((const uint8_t *)m[0], n[0], (const uint8_t *)m[1], n[1], write_fd, &out)) rc = die("bed");
        fflush(stdout);
        fflush(stderr);
        if (!test_hook("FLATGFA_SLOW_EXIT")) _exit(rc);
        return rc;
    }

    flatgfa_t g;
    if (in_flat) {
        g = flatgfa_load(in_flat);
    } else if (in_gfa) {
        g = device_parse ? flatgfa_parse_device(in_gfa) : flatgfa_parse(in_gfa);
    } else {
        std::string buf;
        char tmp[1 << 16];
        ssize_t r;
        while ((r = read(STDIN_FILENO, tmp, sizeof tmp)) > 0) buf.append(tmp, (size_t)r);
        g = device_parse ? flatgfa_parse_bytes_device((const uint8_t *)buf.data(), buf.size(), 1)
                         : flatgfa_parse_stream_bytes((const uint8_t *)buf.data(), buf.size());
    }
    if (!g) {
        if (warm.joinable()) warm.join();
        return die("cannot load graph");
    }
#ifdef MADV_POPULATE_READ
    if (wants_device && in_flat && cmd != "matrix" && cmd != "gaf") {  // (chop uploads the steps too)  // (a freshly mapped file: one call instead of a fault per page inside the upload's copies)
        const void *steps = nullptr;
        uint64_t n = 0, es = 0;
        if (flatgfa_pool(g, 4, &steps, &n, &es) == 0 && n) {
            const uintptr_t page = (uintptr_t)sysconf(_SC_PAGESIZE), a0 = (uintptr_t)steps & ~(page - 1);
            (void)madvise((void *)a0, ((uintptr_t)steps + n * es) - a0, MADV_POPULATE_READ);
        }
    }
#endif
    if (warm.joinable()) warm.join();

    // the GFA text through the device printer, as it streams: to `file`, else to stdout
    auto print_stream = [&](flatgfa_t gr, const char *file) -> int {
        TextOut o{file};
        int r = 0;
        if (flatgfa_print_gfa_stream(gr, write_text, &o)) {
            if (o.failed) fprintf(stderr, "fgfa: cannot write %s\n", file ? file : "the output");
            else die("print");
            r = 1;
        } else if (file && o.fd < 0 && (o.fd = open(file, O_WRONLY | O_CREAT | O_TRUNC, 0666)) < 0) {  // (no text: an empty file)
            fprintf(stderr, "fgfa: cannot write %s\n", file);
            r = 1;
        }
        if (file && o.fd >= 0 && close(o.fd) && !r) { fprintf(stderr, "fgfa: cannot write %s\n", file); r = 1; }
        return r;
    };

    // dump (cli/main.rs:192-212): -o FILE as .flatgfa, else -O FILE as GFA text, else GFA text on stdout.  The text of a
    // command that has brought the device up (chop, inject, crush, flip, extract) is formatted there; a bare `fgfa` prints on the
    // host, where a small graph does not pay for the HIP runtime coming up.
    auto dump = [&](flatgfa_t gr) -> int {
        if (out_flat) return flatgfa_write_flatgfa(gr, out_flat) ? die("write") : 0;
        if (wants_device) return print_stream(gr, out_gfa);
        char *text = nullptr;
        size_t n = 0;
        int r = 0;
        if (flatgfa_print_gfa(gr, &text, &n)) {
            r = die("print");
        } else if (out_gfa) {
            FILE *f = fopen(out_gfa, "wb");
            if (!f || fwrite(text, 1, n, f) != n || fclose(f)) { fprintf(stderr, "fgfa: cannot write %s\n", out_gfa); r = 1; }
        } else {
            write_all(text, n);
        }
        flatgfa_free_text(text);
        return r;
    };

    int rc = 0;
    if (cmd.empty()) {
        rc = dump(g);
    } else if (cmd == "chop") {
        // cli/cmds.rs:286-307: fgfa chop -c N [-l]
        uint64_t count = 0;
        bool links = false, bad = false;
        for (; i < argc; ++i) {
            std::string a = argv[i];
            if ((a == "-c" || a == "--count") && i + 1 < argc) {
                char *end = nullptr;
                count = strtoull(argv[++i], &end, 10);
                bad = bad || !*argv[i] || *end;
            } else if (a == "-l" || a == "--links") {
                links = true;
            } else {
                bad = true;
            }
        }
        if (bad || count == 0) {
            fprintf(stderr, "usage: fgfa chop -c N [-l]   (N >= 1: the maximum segment size)\n");
            flatgfa_free(g);
            return 2;
        }
        flatgfa_t chopped = nullptr;
        if (flatgfa_chop(g, count, links ? 1 : 0, &chopped)) rc = die("chop");
        else rc = dump(chopped);
    } else if (cmd == "inject") {
        // slow_odgi inject --bed BED (`odgi inject -b`): fgfa inject -b BED [-l]
        const char *bed_path = nullptr;
        bool links = false, bad = false;
        for (; i < argc; ++i) {
            std::string a = argv[i];
            if ((a == "-b" || a == "--bed") && i + 1 < argc) bed_path = argv[++i];
            else if (a == "-l" || a == "--links") links = true;
            else bad = true;
        }
        if (bad || !bed_path) {
            fprintf(stderr, "usage: fgfa inject -b BED [-l]   (BED: path<TAB>start<TAB>end<TAB>new_name lines)\n");
            flatgfa_free(g);
            return 2;
        }
        std::string bed;
        if (FILE *f = fopen(bed_path, "rb")) {
            char tmp[1 << 16];
            size_t r;
            while ((r = fread(tmp, 1, sizeof tmp, f)) > 0) bed.append(tmp, r);
            fclose(f);
        } else {
            fprintf(stderr, "fgfa: cannot open %s\n", bed_path);
            flatgfa_free(g);
            return 1;
        }
        flatgfa_t injected = nullptr;
        if (flatgfa_inject_bed(g, bed.data(), bed.size(), links ? 1 : 0, &injected)) rc = die("inject");
        else rc = dump(injected);
    } else if (cmd == "crush") {
        // slow_odgi crush (`odgi crush`): every run of N in a segment becomes one N; the graph is written out as chop's is
        if (i != argc) {
            fprintf(stderr, "usage: fgfa crush\n");
            flatgfa_free(g);
            return 2;
        }
        flatgfa_t crushed = nullptr;
        if (flatgfa_crush(g, &crushed)) rc = die("crush");
        else rc = dump(crushed);
    } else if (cmd == "flip") {
        // slow_odgi flip (`odgi flip`): reverse-heavy paths are turned around and the links they need added; written out as chop's is
        if (i != argc) {
            fprintf(stderr, "usage: fgfa flip\n");
            flatgfa_free(g);
            return 2;
        }
        flatgfa_t flipped = nullptr;
        if (flatgfa_flip(g, &flipped)) rc = die("flip");
        else rc = dump(flipped);
    } else if (cmd == "extract") {
        // cli/cmds.rs:174-215: fgfa extract -n NAME -c DIST [-d N] [-e N]
        uint64_t name = 0, dist = 0, max_dist = 300000, iters = 6;
        bool have_n = false, have_c = false, bad = false;
        for (; i < argc; ++i) {
            const std::string a = argv[i];
            uint64_t *dst = nullptr;
            if (a == "-n" || a == "--seg-name") dst = &name, have_n = true;
            else if (a == "-c" || a == "--link-distance") dst = &dist, have_c = true;
            else if (a == "-d" || a == "--max-distance-subpaths") dst = &max_dist;
            else if (a == "-e" || a == "--max-merging-iterations") dst = &iters;
            if (!dst || i + 1 >= argc) { bad = true; break; }
            char *end = nullptr;
            const char *val = argv[++i];
            *dst = strtoull(val, &end, 10);
            bad = bad || *val < '0' || *val > '9' || *end;
        }
        if (bad || !have_n || !have_c) {
            fprintf(stderr, "usage: fgfa extract -n NAME -c DIST [-d MAX_DISTANCE_SUBPATHS] [-e MAX_MERGING_ITERATIONS]\n");
            flatgfa_free(g);
            return 2;
        }
        const int64_t origin = flatgfa_find_seg(g, name);
        flatgfa_t sub = nullptr;
        if (origin < 0) { fprintf(stderr, "Error: \"segment not found\"\n"); rc = 1; }  // (main's Err, cli/main.rs:132-133)
        else if (flatgfa_extract(g, (uint32_t)origin, dist, max_dist, iters, &sub)) rc = die("extract");
        else rc = dump(sub);
    } else if (cmd == "position") {
        // cli/cmds.rs:105-152: fgfa position -p PATH,OFFSET,+
        if (i + 2 != argc || (strcmp(argv[i], "-p") && strcmp(argv[i], "--path-pos"))) {
            fprintf(stderr, "usage: fgfa position -p PATH,OFFSET,+\n");
            flatgfa_free(g);
            return 2;
        }
        char *text = nullptr;
        size_t n = 0;
        const int prc = flatgfa_position_table(g, (const uint8_t *)argv[i + 1], strlen(argv[i + 1]), &text, &n);
        if (prc == FLATGFA_ERR_ARG) { fprintf(stderr, "Error: \"%s\"\n", flatgfa_last_error()); rc = 1; }  // (the reference's Err)
        else if (prc) rc = die("position");
        else write_all(text, n);
        flatgfa_free_text(text);
    } else if (cmd == "validate" || cmd == "degree") {
        // slow_odgi validate (validate.py:5-25), slow_odgi degree (degree.py:5-18): no arguments; the exit status is 0 whatever validate finds
        if (i != argc) {
            fprintf(stderr, "usage: fgfa %s\n", cmd.c_str());
            flatgfa_free(g);
            return 2;
        }
        char *text = nullptr;
        size_t n = 0;
        if (cmd == "validate" ? flatgfa_validate_table(g, &text, &n) : flatgfa_degree_table(g, &text, &n)) rc = die(cmd.c_str());
        else write_all(text, n);
        flatgfa_free_text(text);
    } else if (cmd == "flatten") {
        // slow_odgi flatten (flatten.py:49-57, __main__.py:178): FASTA then BED on stdout; with -f / -b each goes to its file and
        // nothing to stdout, as `odgi flatten -f -b` (tests/turnt.toml:46-49).  Written as it streams, never held whole.
        const char *name = nullptr, *fasta = nullptr, *bed = nullptr;
        bool bad = false;
        for (; i < argc; ++i) {
            const std::string a = argv[i];
            const char **dst = a == "-n" ? &name : a == "-f" ? &fasta : a == "-b" ? &bed : nullptr;
            if (!dst || i + 1 >= argc) { bad = true; break; }
            *dst = argv[++i];
        }
        if (bad) {
            fprintf(stderr, "usage: fgfa flatten [-n NAME] [-f FASTA] [-b BED]\n");
            flatgfa_free(g);
            return 2;
        }
        // the default name: the input's file name with its last extension cut and ".og" in its place (for x.gfa the
        // reference's G[:-4] + ".og")
        std::string nm = name ? name : "";
        if (!name) {
            nm = in_flat ? in_flat : in_gfa ? in_gfa : "-";
            const size_t dot = nm.rfind('.'), slash = nm.rfind('/');
            if (dot != std::string::npos && (slash == std::string::npos || dot > slash)) nm.resize(dot);
            nm += ".og";
        }
        const auto to = [&](const char *file, int what) -> int {
            int fd = STDOUT_FILENO;
            if (file && (fd = open(file, O_WRONLY | O_CREAT | O_TRUNC, 0666)) < 0) { fprintf(stderr, "fgfa: cannot write %s\n", file); return 1; }
            const int r = flatgfa_flatten_stream(g, nm.data(), nm.size(), what, write_fd, &fd) ? die("flatten") : 0;
            if (file && close(fd) && !r) { fprintf(stderr, "fgfa: cannot write %s\n", file); return 1; }
            return r;
        };
        if (!fasta && !bed) rc = to(nullptr, 3);
        if (fasta) rc = to(fasta, 1);
        if (bed && !rc) rc = to(bed, 2);
    } else if (cmd == "print") {
        // the graph as GFA text (cli/main.rs:192-212 with no command), formatted on the GPU: fgfa print [-O FILE]
        bool bad = false;
        for (; i < argc; ++i) {
            if (!strcmp(argv[i], "-O") && i + 1 < argc) out_gfa = argv[++i];
            else bad = true;
        }
        if (bad) {
            fprintf(stderr, "usage: fgfa [-i FILE | -I FILE] print\n");
            flatgfa_free(g);
            return 2;
        }
        rc = print_stream(g, out_gfa);
    } else if (cmd == "toc") {
        bool bytes = i < argc && !strcmp(argv[i], "-b");
        static const char *names[11] = {"header", "segs", "paths", "links", "steps", "seq_data",
                                        "overlaps", "alignment", "name_data", "optional_data", "line_order"};
        for (int k = 0; k < 11; ++k) {
            uint64_t len = 0, es = 0;
            flatgfa_pool(g, k, nullptr, &len, &es);
            printf("%s: %llu\n", names[k], (unsigned long long)(bytes ? len * es : len));
        }
    } else if (cmd == "paths") {
        uint32_t n = flatgfa_path_count(g);
        for (uint32_t k = 0; k < n; ++k) {
            flatgfa_string_t s = flatgfa_get_path_name(g, k);
            printf("%.*s\n", s.len, (const char *)s.data);
        }
    } else if (cmd == "stats") {
        if (i < argc && !strcmp(argv[i], "-S")) {
            uint64_t len[11];
            for (int k = 0; k < 11; ++k) flatgfa_pool(g, k, nullptr, &len[k], nullptr);
            printf("#length\tnodes\tedges\tpaths\tsteps\n%llu\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)len[5],
                   (unsigned long long)len[1], (unsigned long long)len[3], (unsigned long long)len[2],
                   (unsigned long long)len[4]);
        }
    } else if (cmd == "depth") {
        bool seg_depth = false;
        std::vector<std::string> names;
        const char *bed = nullptr, *subset = nullptr;
        bool bed_paths = false;  // --bed-paths: every entry on the path it names (-b: all on the first entry's)
        for (; i < argc; ++i) {
            std::string a = argv[i];
            if (a == "-d" || a == "--graph-depth-table") seg_depth = true;
            else if (a == "-r" && i + 1 < argc) names.push_back(argv[++i]);
            else if ((a == "-b" || a == "--bed-input") && i + 1 < argc) bed = argv[++i], bed_paths = false;
            else if (a == "--bed-paths" && i + 1 < argc) bed = argv[++i], bed_paths = true;
            else if ((a == "-s" || a == "--subset-paths") && i + 1 < argc) subset = argv[++i];  // odgi depth -d -s
            else { fprintf(stderr, "fgfa: depth: unknown option %s\n", a.c_str()); flatgfa_free(g); return 2; }
        }
        char *text = nullptr;
        size_t n = 0;
        if (seg_depth && subset) {
            // node depth over the listed paths only (slow_odgi depth --paths, depth.py:12)
            std::vector<std::string> want;
            if (!read_names(subset, &want)) { fprintf(stderr, "fgfa: cannot read %s\n", subset); flatgfa_free(g); return 1; }
            std::vector<uint32_t> ids;
            for (auto &nm : want) {
                int64_t id = flatgfa_find_path(g, (const uint8_t *)nm.data(), nm.size());
                if (id >= 0) ids.push_back((uint32_t)id);
            }
            uint32_t S = flatgfa_get_segment_count(g);
            std::vector<uint64_t> d(S), u(S);
            uint32_t dummy = 0;
            rc = flatgfa_seg_depth_subset(g, ids.empty() ? &dummy : ids.data(), (uint32_t)ids.size(), d.data(), u.data());
            if (!rc) {
                std::string out = "#node.id\tdepth\tdepth.uniq\n";
                const void *segs;
                uint64_t ns;
                flatgfa_pool(g, 1, &segs, &ns, nullptr);
                char line[96];
                for (uint32_t k = 0; k < S; ++k) {
                    uint64_t name;
                    memcpy(&name, (const char *)segs + (size_t)k * 24, 8);
                    out.append(line, (size_t)snprintf(line, sizeof line, "%u\t%llu\t%llu\n", (uint32_t)name,
                                                      (unsigned long long)d[k], (unsigned long long)u[k]));
                }
                write_all(out.data(), out.size());
            }
        } else if (seg_depth) {
            rc = flatgfa_depth_table(g, &text, &n);
        } else if (bed) {
            std::string btext;
            FILE *bf = fopen(bed, "rb");
            if (!bf) { fprintf(stderr, "fgfa: cannot open %s\n", bed); flatgfa_free(g); return 1; }
            char tmp[1 << 16];
            size_t r;
            while ((r = fread(tmp, 1, sizeof tmp, bf)) > 0) btext.append(tmp, r);
            fclose(bf);
            rc = bed_paths ? flatgfa_bed_depth_paths_table(g, (const uint8_t *)btext.data(), btext.size(), &text, &n)
                           : flatgfa_bed_depth_table(g, (const uint8_t *)btext.data(), btext.size(), &text, &n);
        } else if (names.empty()) {
            rc = flatgfa_path_depth_table(g, nullptr, 0, &text, &n);
        } else {
            // cmds.rs:270-274: names that do not resolve are silently dropped
            std::vector<uint32_t> ids;
            for (auto &nm : names) {
                int64_t id = flatgfa_find_path(g, (const uint8_t *)nm.data(), nm.size());
                if (id >= 0) ids.push_back((uint32_t)id);
            }
            uint32_t dummy = 0;
            rc = flatgfa_path_depth_table(g, ids.empty() ? &dummy : ids.data(), (uint32_t)ids.size(), &text, &n);
        }
        if (rc) rc = die("depth");
        else write_all(text, n);
        flatgfa_free_text(text);
    } else if (cmd == "window-depth") {
        // cli/cmds.rs:477-496: fgfa window-depth PATH SIZE
        if (i + 1 >= argc) { fprintf(stderr, "usage: fgfa window-depth PATH SIZE\n"); flatgfa_free(g); return 2; }
        std::string pname = argv[i];
        int64_t id = flatgfa_find_path(g, (const uint8_t *)pname.data(), pname.size());
        char *text = nullptr;
        size_t n = 0;
        if (id < 0) { fprintf(stderr, "fgfa: path not found\n"); rc = 1; }
        else if (flatgfa_window_depth_table(g, (uint32_t)id, strtoull(argv[i + 1], nullptr, 10), &text, &n)) rc = die("window-depth");
        else write_all(text, n);
        flatgfa_free_text(text);
    } else if (cmd == "window-depth-all") {
        // fgfa window-depth-all SIZE: what `window-depth P SIZE` prints, for every path in order (a name of its own, so that
        // a path may be called anything)
        if (i >= argc) { fprintf(stderr, "usage: fgfa window-depth-all SIZE\n"); flatgfa_free(g); return 2; }
        char *text = nullptr;
        size_t n = 0;
        if (flatgfa_window_depth_paths_table(g, nullptr, 0, strtoull(argv[i], nullptr, 10), &text, &n)) rc = die("window-depth-all");
        else write_all(text, n);
        flatgfa_free_text(text);
    } else if (cmd == "overlap") {
        // slow_odgi overlap --paths FILE (slow_odgi/__main__.py:93-101)
        if (i + 1 >= argc || strcmp(argv[i], "--paths")) { fprintf(stderr, "usage: fgfa overlap --paths FILE\n"); flatgfa_free(g); return 2; }
        std::vector<std::string> want;
        if (!read_names(argv[i + 1], &want)) { fprintf(stderr, "fgfa: cannot read %s\n", argv[i + 1]); flatgfa_free(g); return 1; }
        std::vector<uint32_t> ids;
        for (auto &nm : want) {
            int64_t id = flatgfa_find_path(g, (const uint8_t *)nm.data(), nm.size());
            if (id < 0) { fprintf(stderr, "fgfa: overlap: path %s is not in the graph\n", nm.c_str()); flatgfa_free(g); return 1; }
            ids.push_back((uint32_t)id);
        }
        char *text = nullptr;
        size_t n = 0;
        uint32_t dummy = 0;
        if (flatgfa_overlap_table(g, ids.empty() ? &dummy : ids.data(), (uint32_t)ids.size(), &text, &n)) rc = die("overlap");
        else write_all(text, n);
        flatgfa_free_text(text);
    } else if (cmd == "matrix") {
        // cli/cmds.rs:453-475: fgfa matrix GAF -- exactly one GAF file
        if (i + 1 != argc) { fprintf(stderr, "usage: fgfa matrix GAF\n"); flatgfa_free(g); return 2; }
        const char *gaf = argv[i];
        const int fd = open(gaf, O_RDONLY);
        struct stat sb;
        if (fd < 0 || fstat(fd, &sb) != 0) {
            fprintf(stderr, "fgfa: cannot open %s\n", gaf);
            if (fd >= 0) close(fd);
            flatgfa_free(g);
            return 1;
        }
        const size_t n = (size_t)sb.st_size;
        void *m = n ? mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0) : nullptr;
        close(fd);
        if (m == MAP_FAILED) { fprintf(stderr, "fgfa: cannot map %s\n", gaf); flatgfa_free(g); return 1; }
        if (m) (void)madvise(m, n, MADV_SEQUENTIAL);  // (read once, front to back; the copies fault the pages in chunk by chunk)
        const uint8_t *text_in = (const uint8_t *)m;
        char *text = nullptr;
        size_t len = 0;
        if (flatgfa_pangenotype_table(g, &text_in, &n, 1, &text, &len)) rc = die("matrix");
        else write_all(text, len);
        flatgfa_free_text(text);
    } else if (cmd == "gaf") {
        // cli/cmds.rs:311-376: fgfa gaf GAF [-s] [-b] [-p] -- one GAF file; -p without -b is unimplemented!() in the reference
        const char *gaf = nullptr;
        bool seqs = false, bench = false, parallel = false, bad = false;
        for (; i < argc; ++i) {
            const std::string a = argv[i];
            if (a == "-s") seqs = true;
            else if (a == "-b") bench = true;
            else if (a == "-p") parallel = true;
            else if (a[0] != '-' && !gaf) gaf = argv[i];
            else bad = true;
        }
        if (bad || !gaf || (parallel && !bench)) {
            fprintf(stderr, "usage: fgfa gaf GAF [-s] [-b [-p]]\n");
            flatgfa_free(g);
            return 2;
        }
        const int fd = open(gaf, O_RDONLY);
        struct stat sb;
        if (fd < 0 || fstat(fd, &sb) != 0) {
            fprintf(stderr, "fgfa: cannot open %s\n", gaf);
            if (fd >= 0) close(fd);
            flatgfa_free(g);
            return 1;
        }
        const size_t n = (size_t)sb.st_size;
        void *m = n ? mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0) : nullptr;
        close(fd);
        if (m == MAP_FAILED) { fprintf(stderr, "fgfa: cannot map %s\n", gaf); flatgfa_free(g); return 1; }
        if (m) (void)madvise(m, n, MADV_SEQUENTIAL);
        const uint8_t *text_in = (const uint8_t *)m;
        if (bench) {  // cmds.rs:325-347: the events are counted, nothing else is printed
            uint64_t events = 0;
            if (flatgfa_gaf_count(g, text_in, n, &events, nullptr)) rc = die("gaf");
            else printf("%llu\n", (unsigned long long)events);
        } else {
            char *text = nullptr;
            size_t len = 0;
            if (seqs ? flatgfa_gaf_seqs(g, text_in, n, &text, &len) : flatgfa_gaf_table(g, text_in, n, &text, &len)) rc = die("gaf");
            else write_all(text, len);
            flatgfa_free_text(text);
        }
    } else {
        fprintf(stderr, "fgfa: command '%s' is outside the depth path this build covers\n", cmd.c_str());
        rc = 2;
    }
    // (no tear-down: the process is over, and unloading the HIP runtime takes longer than the query did)
    fflush(stdout);
    fflush(stderr);
    if (!test_hook("FLATGFA_SLOW_EXIT")) _exit(rc);
    flatgfa_free(g);
    return rc;
}
