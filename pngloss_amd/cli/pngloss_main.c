/*
 * pngloss_main.c -- `pngloss [options] -- pngfile [pngfile ...]` on an MI355X: files, threads and the calls into the library.
 *
 * Same command line, messages and exit codes as the reference tool (/root/reference/src/pngloss.c:28-165 usage and
 * argument checks), but the per-file loop of pngloss_main_internal (pngloss.c:168-223), which handles one file at a
 * time, is replaced by a three-stage batch:
 *
 *     decode all inputs (libpng, worker threads)  ->  ONE batched call into libpngloss_hip.so  ->  encode (threads)
 *
 * The GPU call also returns the filtered scanlines of every image (colour type re-detected, per-row filters applied),
 * so the encode stage only deflates and frames chunks (png_stream_writer.c) -- libpng is used for decoding only.
 *
 * All files of a call go to the GPU together, so that a GPU with 256 compute units works on up to 256 images at once
 * (one workgroup per image).  Files are processed in windows so that memory stays bounded.  Per-file semantics are
 * unchanged: output naming (--ext / -o), the overwrite rule, temp-file + atomic rename, --skip-if-larger, --strip,
 * stdin/stdout with "-", and the exit code is the error of the last failing file.  Verbose messages are buffered per
 * file and printed in file order.
 *
 * What is decided without I/O lives beside this file and is tested on the CPU: the command line and its rules
 * (cli_options.c), what a library answer means for one file (cli_outcome.h), the lines about a file (cli_report.c).
 */
#include <pthread.h>
#include <stdarg.h>
#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include "../../include/pngloss_hip.h"
#include "../../include/pngloss_hip_indexed.h"
#include "../../include/pngloss_hip_index_depth.h"
#include "../../include/pngloss_hip_quant.h"
#include "../../include/pngloss_hip_dither.h"
#include "../../include/pngloss_hip_quant_target.h"
#include "../../include/pngloss_hip_quant_space.h"
#include "cli_options.h"
#include "cli_outcome.h"
#include "cli_report.h"
#include "png_bridge.h"
#include "png_stream_reader.h"
#include "png_stream_writer.h"

#define PNGLOSS_VERSION "1.0.1-mi355x"
#define WINDOW_FILES window_files()      /* images per GPU batch (one workgroup each): 256, or $PNGLOSS_WINDOW_FILES */
static size_t window_files(void);

static void print_version_banner(FILE *f)
{
    fprintf(f, "pngloss, %s, filter+quantise path on AMD MI355X (%s).\n", PNGLOSS_VERSION, pngloss_hip_version());
    rwpng_version_info(f);
    fputs("\n", f);
}

/* ------------------------------------------------------------------------------------------- per-file job */

struct job {
    const char *in_name;      /* "stdin" for the pipe */
    char *out_name;           /* malloc'ed unless it aliases options.output_path */
    bool own_out_name;
    pngloss_error status;
    png24_image in, out;
    unsigned char *filters;
    unsigned char *line_types, *lines;   /* filtered scanlines from the GPU: type byte per row, width*4-pitched rows */
    size_t zsize;                        /* --gpu-deflate: `lines` holds the finished zlib stream of zsize bytes instead */
    int color_type;
    char *log;                /* buffered stderr text */
    size_t log_len;
    pngloss_hip_result gpu;
    pngloss_hip_size_report size;        /* --target-size: what the search found for this file */
    size_t size_budget;                  /* ... and the file's budget in bytes */
    pngloss_hip_target_report target;    /* --target-psnr / --max-error: the strength the search chose for this file */
    pngloss_hip_distortion distortion;   /* --distortion: the optimised pixels against the decoded input's (have_distortion: the library had a record) */
    bool have_distortion;
    pngloss_hip_ssim ssim;               /* --ssim: the same pair's structural similarity (have_ssim: the library had a record) */
    bool have_ssim;
    pngloss_hip_palette palette;         /* --indexed: what the library decided for this file (color_type 3: the PLTE / tRNS payloads of the written file) */
    bool have_palette;
    pngloss_hip_index_depth depth;       /* --index-depth: the bit depth of the stream the library kept (have_depth: the library had a record) */
    bool have_depth;
    pngloss_hip_quant_report quant;      /* --colors: what the quantiser did to this file (have_quant: it ran) */
    bool have_quant;
    pngloss_hip_quant_target_report chosen;   /* --colors-psnr / --colors-max-error: what the colour-count search did (have_chosen: it ran) */
    bool have_chosen;
    png_stream_source src;    /* --gpu-read: inflated scanlines waiting for the device (src.scanlines != NULL) */
};

static void say(struct job *j, const char *fmt, ...)
{
    char line[1024];
    va_list ap;
    va_start(ap, fmt);
    int n = vsnprintf(line, sizeof line, fmt, ap);
    va_end(ap);
    if (n <= 0) return;
    if ((size_t)n >= sizeof line) n = (int)sizeof line - 1;
    char *grown = realloc(j->log, j->log_len + (size_t)n + 1);
    if (!grown) return;
    memcpy(grown + j->log_len, line, (size_t)n + 1);
    j->log = grown;
    j->log_len += (size_t)n;
}

static void flush_log(struct job *j)
{
    if (j->log) fputs(j->log, stderr);
    free(j->log);
    j->log = NULL;
    j->log_len = 0;
}

static const char *leaf(const char *path)
{
    const char *s = strrchr(path, '/');
    return s ? s + 1 : path;
}

static char *with_extension(const char *name, const char *ext)
{
    size_t n = strlen(name);
    char *out = malloc(n + strlen(ext) + 1);
    if (!out) return NULL;
    memcpy(out, name, n + 1);
    if (n > 4 && (memcmp(out + n - 4, ".png", 4) == 0 || memcmp(out + n - 4, ".PNG", 4) == 0)) n -= 4;
    strcpy(out + n, ext);
    return out;
}

static bool exists(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (f) fclose(f);
    return f != NULL;
}

/* the private output copy of a decoded image (pngloss.c:471-484 of the reference) */
static void finish_decode(struct job *j, const struct cli_options *o)
{
    if (j->status != SUCCESS) return;
    if (o->verbose) {
        say(j, "  read %luKB file\n", (unsigned long)((j->in.file_size + 500UL) / 1000UL));
        if (j->in.input_color == RWPNG_SRGB) say(j, "  passing sRGB tag from the input\n");
        else if (j->in.gamma != 0.45455) say(j, "  converted image from gamma %2.1f to gamma 2.2\n", 1.0 / j->in.gamma);
    }
    const size_t W = j->in.width, H = j->in.height;
    j->out.width = j->in.width;
    j->out.height = j->in.height;
    j->out.gamma = j->in.gamma;
    j->out.output_color = j->in.output_color;
    const size_t bytes = W * H * 4;
    j->out.rgba_data = malloc(bytes > 0 ? bytes : 1);
    j->out.row_pointers = malloc((H ? H : 1) * sizeof(unsigned char *));
    j->filters = malloc(H ? H : 1);
    j->line_types = malloc(H ? H : 1);
    j->lines = malloc(o->gpu_deflate ? pngloss_hip_zlib_bound((uint32_t)W, (uint32_t)H) : (bytes > 0 ? bytes : 1));
    if (!j->out.rgba_data || !j->out.row_pointers || !j->filters || !j->line_types || !j->lines) { j->status = OUT_OF_MEMORY_ERROR; return; }
    for (size_t y = 0; y < H; y++) {
        j->out.row_pointers[y] = j->out.rgba_data + y * W * 4;
        memcpy(j->out.row_pointers[y], j->in.row_pointers[y], W * 4);
    }
}

/* --gpu-read, host half: chunk walk + inflate (png_stream_reader.c); the image header fields the libpng path would have set
 * (rwpng.c:260-277: sRGB tag, else gAMA inside (0, 1], else the default) and the RGBA buffer the device will fill */
static bool decode_job_stream(struct job *j)
{
    if (!png_stream_read(j->in_name, &j->src)) return false;
    png24_image *im = &j->in;
    im->width = j->src.width; im->height = j->src.height; im->file_size = j->src.file_size;
    double gamma = 0.45455;
    if (j->src.has_srgb) im->input_color = im->output_color = RWPNG_SRGB;
    else {
        if (j->src.has_gama) gamma = j->src.gamma;
        if (gamma > 0 && gamma <= 1.0) im->input_color = im->output_color = RWPNG_GAMA_ONLY;
        else {
            say(j, "pngloss readpng:  ignored out-of-range gamma %f\n", gamma);
            im->input_color = im->output_color = RWPNG_NONE;
            gamma = 0.45455;
        }
    }
    im->gamma = gamma;
    const size_t W = im->width, H = im->height;
    im->rgba_data = malloc(W * H * 4);
    im->row_pointers = malloc(H * sizeof(unsigned char *));
    if (!im->rgba_data || !im->row_pointers) { free(j->src.scanlines); j->src.scanlines = NULL; j->status = OUT_OF_MEMORY_ERROR; return true; }
    for (size_t y = 0; y < H; y++) im->row_pointers[y] = im->rgba_data + y * W * 4;
    return true;
}

/* stage 1: open + decode + private output copy (pngloss.c:433-484 of the reference) */
static void decode_job(struct job *j, const struct cli_options *o)
{
    if (j->status != SUCCESS) return;
    if (o->verbose) say(j, "%s:\n", j->in_name);
    if (o->gpu_read && !o->from_stdin && decode_job_stream(j)) return;       /* pixels follow from the device (decode_window_on_device) */
    FILE *f = o->from_stdin ? stdin : fopen(j->in_name, "rb");
    if (!f) {
        say(j, "  error: cannot open %s for reading\n", j->in_name);
        j->status = READ_ERROR;
        return;
    }
    pngloss_error rc = rwpng_read_image24(f, &j->in, o->strip, o->verbose);
    if (!o->from_stdin) fclose(f);
    if (rc != SUCCESS) {
        say(j, "  error: cannot decode image %s\n", o->from_stdin ? "from stdin" : leaf(j->in_name));
        j->status = rc;
        return;
    }
    finish_decode(j, o);
}

/* what the stream writer takes from a decoded image: size, gamma, colour tags (rwpng.c:508-516 of the reference) and the chunks to pass through.
 * Colour type 6 without rows: callers that write fill in theirs by name */
static png_stream_image stream_image_of(const png24_image *img, const struct rwpng_chunk *chunks)
{
    return (png_stream_image){ .width = img->width, .height = img->height, .color_type = 6, .gamma = img->gamma,
                               .tag_gamma = img->output_color != RWPNG_GAMA_ONLY && img->output_color != RWPNG_NONE,
                               .tag_srgb = img->output_color == RWPNG_SRGB, .chunks = chunks };
}

/* stage 3: encode to "<out>.tmp", rename over the destination (pngloss.c:379-431 of the reference) */
static pngloss_error encode_to(struct job *j, png24_image *img, unsigned char *filters, const struct cli_options *o)
{
    FILE *f;
    char *tmp = NULL;
    if (o->to_stdout) {
        f = stdout;
        if (o->verbose) say(j, "  writing compressed image to stdout\n");
    } else {
        tmp = malloc(strlen(j->out_name) + 5);
        if (!tmp) return OUT_OF_MEMORY_ERROR;
        sprintf(tmp, "%s.tmp", j->out_name);
        f = fopen(tmp, "wb");
        if (!f) {
            say(j, "  error: cannot open '%s' for writing\n", tmp);
            free(tmp);
            return CANT_WRITE_ERROR;
        }
        if (o->verbose) say(j, "  writing compressed image as %s\n", leaf(j->out_name));
    }
    pngloss_error rc;
    if (filters) {
        /* the optimised image: scanlines were filtered on the GPU, only deflate + chunk framing happen here */
        png_stream_image si = stream_image_of(img, img->chunks);
        si.color_type = j->color_type;
        si.filter_ids = j->line_types;
        si.rows = j->lines;
        si.pitch = (size_t)img->width * 4;
        si.maximum_file_size = img->maximum_file_size;
        if (o->gpu_deflate) { si.zdata = j->lines; si.zsize = j->zsize; }
        if (j->color_type == 3) {
            si.palette = &j->palette.rgb[0][0]; si.palette_entries = j->palette.entries;
            si.trns = j->palette.alpha; si.trns_entries = j->palette.trns_entries;
            if (j->have_depth) si.index_bits = j->depth.bit_depth;
        }
        rc = png_stream_write(f, &si, &img->file_size, &img->metadata_size);
    } else {
        rc = rwpng_write_image24(f, img, NULL);     /* the untouched original (pipe fallback): plain libpng */
    }
    if (!o->to_stdout) {
        fclose(f);
        if (rc == SUCCESS && rename(tmp, j->out_name) != 0) rc = CANT_WRITE_ERROR;
        if (rc != SUCCESS) unlink(tmp);
    }
    free(tmp);
    if (rc != SUCCESS && rc != TOO_LARGE_FILE)
        say(j, "  error: failed writing image to %s (%d)\n", o->to_stdout ? "stdout" : j->out_name, (int)rc);
    return rc;
}

/* --distortion and --ssim: the lines of a written file (cli_report.c) */
static void say_distortion(struct job *j, const struct cli_options *o)
{
    char line[256];
    /* (--colors-visible: the record is the quantiser's, which that switch makes the visible-mode one) */
    cli_report_distortion(line, sizeof line, &j->distortion, j->gpu.bytes_per_pixel, o->visible || o->colors_visible);
    say(j, "%s", line);
}

static void say_ssim(struct job *j, const struct cli_options *o)
{
    char line[256];
    cli_report_ssim(line, sizeof line, j->have_ssim ? &j->ssim : NULL, o->search, j->gpu.bytes_per_pixel, o->visible);
    say(j, "%s", line);
}

static void encode_job(struct job *j, const struct cli_options *o)
{
    if (j->status != SUCCESS) return;
    char line[1024];
    if (o->verbose && o->search != CLI_SEARCH_NONE) {
        if (o->search == CLI_SEARCH_SIZE) cli_report_strength(line, sizeof line, j->size.strength, j->size.probes);
        else cli_report_strength(line, sizeof line, j->target.strength, j->target.probes);
        say(j, "%s", line);
    }
    if (o->verbose) say(j, "  compression complete\n  used %u unique symbols\n", j->gpu.unique_symbols);
    if (o->verbose && j->have_quant) {
        cli_report_quant(line, sizeof line, &j->quant);
        say(j, "%s", line);
        if (o->colors_visible) {
            cli_report_colors_space(line, sizeof line, &j->quant);
            say(j, "%s", line);
        }
        if (j->have_chosen) {
            cli_report_chosen_colors(line, sizeof line, &j->chosen, (unsigned)o->colors);
            say(j, "%s", line);
        }
        if (o->dither) {
            cli_report_dither(line, sizeof line, &j->quant);
            say(j, "%s", line);
        }
    }
    if (o->verbose && j->color_type == 3) {
        cli_report_indexed(line, sizeof line, &j->palette);
        say(j, "%s", line);
        if (j->have_depth) {
            cli_report_index_depth(line, sizeof line, &j->depth);
            say(j, "%s", line);
        }
    }
    if (o->skip_if_larger) j->out.maximum_file_size = j->in.file_size - 1;
    j->out.chunks = j->in.chunks;          /* metadata travels to the output */
    j->in.chunks = NULL;
    pngloss_error rc = encode_to(j, &j->out, j->filters, o);
    /* a colour target that even --colors M does not reach: the file was written at M colours; one line says so, the exit status stays */
    if (j->have_chosen && rc == SUCCESS && !j->chosen.reached) {
        cli_report_colors_missed(line, sizeof line, j->in_name, (unsigned)o->colors);
        say(j, "%s", line);
    }
    /* a budget that was not reached (or is smaller than the container alone): the file was written at -s; one line says so, the exit status stays */
    if (o->search == CLI_SEARCH_SIZE && rc == SUCCESS && (!j->size.reached || j->out.file_size > j->size_budget)) {
        cli_report_budget_missed(line, sizeof line, j->in_name, j->size_budget, j->out.file_size, j->size.strength);
        say(j, "%s", line);
    }
    if (o->distortion && rc == SUCCESS && j->have_distortion) say_distortion(j, o);
    if (o->ssim && rc == SUCCESS) say_ssim(j, o);
    if (o->verbose) {
        if (rc == SUCCESS) {
            say(j, "  wrote %luKB file (%.1f%% of original)\n", (unsigned long)((j->out.file_size + 500UL) / 1000UL),
                100.0f * (float)j->out.file_size / (float)j->in.file_size);
            if (j->out.metadata_size > 0) say(j, "  copied %dKB of additional PNG metadata\n", (int)(j->out.metadata_size + 500) / 1000);
        } else if (rc == TOO_LARGE_FILE) {
            say(j, "  file exceeded maximum size of %luKB\n", (unsigned long)((j->out.maximum_file_size + 500UL) / 1000UL));
        }
    }
    if (o->to_stdout && (rc == TOO_LARGE_FILE || rc == TOO_LOW_QUALITY)) {
        /* never leave a pipe empty: fall back to the decoded original */
        pngloss_error again = encode_to(j, &j->in, NULL, o);
        if (again != SUCCESS) rc = again;
    }
    j->status = rc;
}

/* ------------------------------------------------------------------------------------------- tiny parallel-for */

struct crew { struct job *jobs; size_t n, next; const struct cli_options *o; void (*work)(struct job *, const struct cli_options *); pthread_mutex_t mu; };

static void *crew_member(void *arg)
{
    struct crew *c = arg;
    for (;;) {
        pthread_mutex_lock(&c->mu);
        size_t i = c->next++;
        pthread_mutex_unlock(&c->mu);
        if (i >= c->n) return NULL;
        c->work(&c->jobs[i], c->o);
    }
}

static void for_each_job(struct job *jobs, size_t n, const struct cli_options *o, void (*work)(struct job *, const struct cli_options *))
{
    long cores = sysconf(_SC_NPROCESSORS_ONLN);
    size_t threads = cores > 1 ? (size_t)cores : 1;
    if (threads > n) threads = n;
    if (threads > 64) threads = 64;
    if (o->from_stdin || o->to_stdout) threads = 1;
    struct crew c = { jobs, n, 0, o, work, PTHREAD_MUTEX_INITIALIZER };
    if (threads <= 1) { crew_member(&c); return; }
    pthread_t tid[64];
    size_t started = 0;
    for (; started < threads; started++)
        if (pthread_create(&tid[started], NULL, crew_member, &c) != 0) break;
    if (!started) crew_member(&c);
    for (size_t t = 0; t < started; t++) pthread_join(tid[t], NULL);
}

/* ------------------------------------------------------------------------------------------- the batch driver */

static double now_s(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

static size_t window_files(void)
{
    const char *e = getenv("PNGLOSS_WINDOW_FILES");
    const long v = e ? atol(e) : 0;
    return v > 0 ? (size_t)v : 256;
}

/* stage 1 of a window, possibly running in the background while the previous window is on the GPU */
struct decode_ahead { struct job *jobs; size_t n; const struct cli_options *o; pthread_t thread; bool running; double seconds; };

/* --gpu-read, device half: every file of the window whose scanlines were inflated, as ONE batch (its own context: the optimiser's
 * contexts may be busy with the previous window) */
static pngloss_hip_ctx *g_read_ctx = NULL;
static void decode_window_on_device(struct job *jobs, size_t n, const struct cli_options *o)
{
    size_t m = 0;
    for (size_t i = 0; i < n; i++) if (jobs[i].src.scanlines && jobs[i].status == SUCCESS) m++;
    if (m) {
        pngloss_hip_png_source *src = calloc(m, sizeof *src);
        size_t *who = calloc(m, sizeof *who);
        int rc = src && who ? PNGLOSS_SUCCESS : PNGLOSS_OUT_OF_MEMORY_ERROR;
        if (rc == PNGLOSS_SUCCESS && !g_read_ctx) { g_read_ctx = pngloss_hip_create(-1); if (!g_read_ctx) rc = PNGLOSS_HIP_ERROR; }
        size_t k = 0;
        for (size_t i = 0; i < n && rc == PNGLOSS_SUCCESS; i++) {
            struct job *j = &jobs[i];
            if (!j->src.scanlines || j->status != SUCCESS) continue;
            src[k] = (pngloss_hip_png_source){ j->src.scanlines, j->src.width, j->src.height, j->src.color_type, j->src.bit_depth, j->src.interlace,
                                               j->src.palette_entries ? j->src.palette : NULL, j->src.palette_entries,
                                               j->src.has_trns ? j->src.trns : NULL, j->src.trns_bytes, j->in.rgba_data };
            who[k++] = i;
        }
        /* a status per file: a damaged file fails alone, like under the reference's one-file-at-a-time loop (pngloss.c:196-204) */
        int *st = calloc(m, sizeof *st);
        if (!st && rc == PNGLOSS_SUCCESS) rc = PNGLOSS_OUT_OF_MEMORY_ERROR;
        int brc = rc;
        if (rc == PNGLOSS_SUCCESS) brc = pngloss_hip_png_decode_batch_host_status(g_read_ctx, src, m, st);
        bool explained = false;
        for (size_t q = 0; q < k && rc == PNGLOSS_SUCCESS; q++) if (st[q]) explained = true;
        for (size_t q = 0; q < k; q++) {
            const int one = cli_status_after_device_read(rc, brc, st ? st[q] : 0, explained);
            if (one != PNGLOSS_SUCCESS) { say(&jobs[who[q]], "  error: cannot decode image %s on the GPU (%d)\n", leaf(jobs[who[q]].in_name), one); jobs[who[q]].status = (pngloss_error)one; }
        }
        free(src); free(who); free(st);
    }
    for (size_t i = 0; i < n; i++) {
        if (!jobs[i].src.scanlines) continue;
        free(jobs[i].src.scanlines); jobs[i].src.scanlines = NULL;
        finish_decode(&jobs[i], o);
    }
}

static void *decode_ahead_main(void *arg)
{
    struct decode_ahead *d = arg;
    const double t0 = now_s();
    for_each_job(d->jobs, d->n, d->o, decode_job);
    if (d->o->gpu_read) decode_window_on_device(d->jobs, d->n, d->o);
    d->seconds = now_s() - t0;
    return NULL;
}

static void *warm_up_main(void *arg)
{
    (void)arg;
    if (pngloss_hip_device_count() > 0) {                    /* runtime, device context, code objects */
        pngloss_hip_ctx *c = pngloss_hip_create(-1);
        if (c) pngloss_hip_destroy(c);
    }
    return NULL;
}

static void decode_ahead_start(struct decode_ahead *d, struct job *jobs, size_t n, const struct cli_options *o)
{
    d->jobs = jobs; d->n = n; d->o = o; d->seconds = 0;
    d->running = n && pthread_create(&d->thread, NULL, decode_ahead_main, d) == 0;
    if (n && !d->running) decode_ahead_main(d);              /* no thread: decode right here */
}

static void decode_ahead_wait(struct decode_ahead *d)
{
    if (d->running) pthread_join(d->thread, NULL);
    d->running = false;
}

/* The per-image arrays of one GPU batch, indexed alike: what goes into the library call and what comes back.  Entry k is job who[k]. */
struct window_batch {
    size_t m;                          /* entries in use */
    size_t *who;
    pngloss_hip_host_image *imgs;
    pngloss_hip_scanlines *lines;
    pngloss_hip_zstream *zs;
    pngloss_hip_result *res;
    pngloss_hip_target_report *rep;    /* the quality search: the strength chosen and the distortion record ... */
    pngloss_hip_ssim *sm;              /* ... and with --target-ssim the SSIM records of what was written */
    pngloss_hip_size_report *srep;     /* the size search */
    uint64_t *budget;                  /* the size search: the largest zlib stream of each file */
};

static void window_batch_free(struct window_batch *b)
{
    free(b->who); free(b->imgs); free(b->lines); free(b->zs); free(b->res); free(b->rep); free(b->sm); free(b->srep); free(b->budget);
}

static bool window_batch_alloc(struct window_batch *b, size_t n)
{
    if (!n) n = 1;
    *b = (struct window_batch){ .who = calloc(n, sizeof *b->who), .imgs = calloc(n, sizeof *b->imgs), .lines = calloc(n, sizeof *b->lines),
                                .zs = calloc(n, sizeof *b->zs), .res = calloc(n, sizeof *b->res), .rep = calloc(n, sizeof *b->rep),
                                .sm = calloc(n, sizeof *b->sm), .srep = calloc(n, sizeof *b->srep), .budget = calloc(n, sizeof *b->budget) };
    if (b->who && b->imgs && b->lines && b->zs && b->res && b->rep && b->sm && b->srep && b->budget) return true;
    window_batch_free(b);
    return false;
}

/* every decoded image of the window */
static void collect_decoded(struct window_batch *b, struct job *jobs, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        struct job *j = &jobs[i];
        if (j->status != SUCCESS) continue;
        b->imgs[b->m] = (pngloss_hip_host_image){ j->out.rgba_data, j->filters, j->out.width, j->out.height };
        b->lines[b->m] = (pngloss_hip_scanlines){ j->line_types, j->lines, (size_t)j->out.width * 4, -1 };
        b->zs[b->m] = (pngloss_hip_zstream){ j->lines, pngloss_hip_zlib_bound(j->out.width, j->out.height), 0, -1, { 0, 0, 0 },
                                             PNGLOSS_HIP_Z_STREAM_ONLY };     /* the file is written from the stream alone */
        b->who[b->m++] = i;
    }
}

/* --gpu-deflate: the device encoder addresses one image's scanlines with 32-bit positions (include/pngloss_hip.h); larger images fail here and
 * leave the batch */
static void refuse_too_large(struct window_batch *b, struct job *jobs)
{
    size_t keep = 0;
    for (size_t k = 0; k < b->m; k++) {
        if (((uint64_t)b->imgs[k].width * 4 + 1) * b->imgs[k].height > ((uint64_t)1 << 30)) {
            say(&jobs[b->who[k]], "  error: image too large for --gpu-deflate (more than 1 GiB of scanlines); run it without the option\n");
            jobs[b->who[k]].status = INVALID_ARGUMENT;
            continue;
        }
        b->imgs[keep] = b->imgs[k]; b->lines[keep] = b->lines[k]; b->zs[keep] = b->zs[k]; b->who[keep++] = b->who[k];
    }
    b->m = keep;
}

/* Every GPU of the node ($PNGLOSS_DEVICES restricts or repeats them; the files of a window are dealt out by size), with the options of this call.
 * NULL: no context, or the library refused an option the call cannot do without */
static pngloss_hip_multi *open_contexts(const struct cli_options *o)
{
    /* a context (device initialisation, events, arenas) only on as many GPUs as the call has files for */
    const char *envd = getenv("PNGLOSS_DEVICES");
    const int ndev = pngloss_hip_device_count();
    pngloss_hip_multi *ctx;
    if ((envd && *envd) || ndev <= 1 || (size_t)ndev <= o->num_files) ctx = pngloss_hip_multi_create(NULL);
    else {
        char list[256]; size_t at = 0;
        for (size_t d = 0; d < o->num_files && at + 8 < sizeof list; d++) at += (size_t)snprintf(list + at, sizeof list - at, d ? ",%zu" : "%zu", d);
        ctx = pngloss_hip_multi_create(list);
    }
    if (!ctx) return NULL;
    /* (with --colors the record is the quantiser's: strength 0 changes no pixel behind it) */
    if (o->distortion && !o->have_colors && pngloss_hip_multi_set_option(ctx, "distortion", "on") != PNGLOSS_SUCCESS)
        fputs("  warning: the library refused the option \"distortion\"; no distortion lines\n", stderr);
    if (o->ssim && pngloss_hip_multi_set_option(ctx, "ssim", "on") != PNGLOSS_SUCCESS)
        fputs("  warning: the library refused the option \"ssim\"; no ssim lines\n", stderr);
    if (o->indexed && pngloss_hip_multi_set_option(ctx, "indexed", "on") != PNGLOSS_SUCCESS)
        fputs("  warning: the library refused the option \"indexed\"; every file is written as truecolour\n", stderr);
    /* (a library that refuses it stays at 8 bits, and its record says so) */
    if (o->have_index_depth && pngloss_hip_multi_set_option(ctx, "index_depth", o->index_depth) != PNGLOSS_SUCCESS)
        fputs("  warning: the library refused the option \"index_depth\"; palette files are written at 8 bits\n", stderr);
    /* --visible: what those two and the searches measure.  A library that refuses it would measure something else than the lines say */
    if (o->visible && pngloss_hip_multi_set_option(ctx, "measure", "visible") != PNGLOSS_SUCCESS) {
        fputs("  error: the library refused the option \"measure\"\n", stderr);
        pngloss_hip_multi_destroy(ctx);
        return NULL;
    }
    return ctx;
}

/* --target-size: each file's budget for the WRITTEN FILE, turned into the largest zlib stream that fits it (png_stream_writer.c knows the
 * container) */
static void compute_budgets(struct window_batch *b, struct job *jobs, const struct cli_options *o)
{
    for (size_t k = 0; k < b->m; k++) {
        struct job *j = &jobs[b->who[k]];
        j->size_budget = cli_file_budget(o->size_percent, o->size_value, j->in.file_size);
        const png_stream_image si = stream_image_of(&j->out, j->in.chunks);
        b->budget[k] = cli_stream_budget(png_stream_largest_stream(&si, j->size_budget, PNG_STREAM_GPU_IDAT_SLICE));
    }
}

/* --colors: every image of the batch to at most N colours, where it lies (it is the encoder's private copy of the decoded input).  An error fails
 * every file of the batch, which then has nothing left to optimise */
static void quantise_batch(pngloss_hip_multi *ctx, struct window_batch *b, struct job *jobs, const struct cli_options *o)
{
    const pngloss_hip_quant_params params = { (uint32_t)o->colors, PNGLOSS_HIP_QUANT_DEFAULT_ROUNDS };
    const pngloss_hip_quant_params2 dithered = { params.max_colors, params.rounds, PNGLOSS_HIP_DITHER_FLOYD_STEINBERG, 0 };
    const bool searched = o->have_colors_psnr || o->have_colors_max_error;
    const pngloss_hip_quant_params2 plain = { params.max_colors, params.rounds, PNGLOSS_HIP_DITHER_NONE, 0 };
    /* --colors-visible: the same call in the premultiplied space */
    const pngloss_hip_quant_params3 visible = { params.max_colors, params.rounds, o->dither ? PNGLOSS_HIP_DITHER_FLOYD_STEINBERG : PNGLOSS_HIP_DITHER_NONE,
                                                PNGLOSS_HIP_QUANT_SPACE_VISIBLE };
    const pngloss_hip_quant_target target = { o->have_colors_psnr ? o->colors_psnr : 0.0, o->have_colors_max_error ? (uint32_t)o->colors_max_error : 0, 0 };
    pngloss_hip_quant_report *reports = calloc(b->m ? b->m : 1, sizeof *reports);
    pngloss_hip_quant_target_report *chosen = searched ? calloc(b->m ? b->m : 1, sizeof *chosen) : NULL;
    int rc = !ctx ? PNGLOSS_HIP_ERROR : !reports || (searched && !chosen) ? PNGLOSS_OUT_OF_MEMORY_ERROR
           : searched && o->colors_visible ? pngloss_hip_multi_quantize_batch_host_target3(ctx, b->imgs, b->m, &visible, &target, chosen)
           : o->colors_visible ? pngloss_hip_multi_quantize_batch_host3(ctx, b->imgs, b->m, &visible, reports)
           : searched ? pngloss_hip_multi_quantize_batch_host_target(ctx, b->imgs, b->m, o->dither ? &dithered : &plain, &target, chosen)
           : o->dither ? pngloss_hip_multi_quantize_batch_host2(ctx, b->imgs, b->m, &dithered, reports)
                       : pngloss_hip_multi_quantize_batch_host(ctx, b->imgs, b->m, &params, reports);
    for (size_t k = 0; k < b->m; k++) {
        struct job *j = &jobs[b->who[k]];
        if (rc == PNGLOSS_SUCCESS && searched) { j->chosen = chosen[k]; j->have_chosen = true; reports[k] = chosen[k].quant; }
        if (rc == PNGLOSS_SUCCESS) { j->quant = reports[k]; j->have_quant = true; continue; }
        say(j, "  error: GPU colour quantisation failed (%d)\n", rc);
        j->status = (pngloss_error)rc;
    }
    if (rc != PNGLOSS_SUCCESS) b->m = 0;
    free(reports);
    free(chosen);
}

/* The one call into the library.  In a search the library finds a strength per file, -s bounds it, and the records come back in the reports */
static int optimise_batch(pngloss_hip_multi *ctx, struct window_batch *b, const struct cli_options *o)
{
    if (!ctx) return PNGLOSS_HIP_ERROR;
    pngloss_hip_scanlines *lines = o->gpu_deflate ? NULL : b->lines;
    pngloss_hip_zstream *zs = o->gpu_deflate ? b->zs : NULL;
    switch (o->search) {
    case CLI_SEARCH_SIZE: {
        const pngloss_hip_size_target target = { b->budget, (uint32_t)o->strength, 0 };
        return pngloss_hip_multi_optimize_batch_host_size(ctx, b->imgs, b->m, &target, (long)o->bleed, b->res, NULL, b->zs, b->srep);
    }
    case CLI_SEARCH_QUALITY:
        if (o->have_target_ssim) {
            const pngloss_hip_target2 target = { o->target_psnr, (uint32_t)o->max_error, (uint32_t)o->strength, o->target_ssim };
            return pngloss_hip_multi_optimize_batch_host_target2(ctx, b->imgs, b->m, &target, (long)o->bleed, b->res, lines, zs, b->rep, b->sm);
        } else {
            const pngloss_hip_target target = { o->target_psnr, (uint32_t)o->max_error, (uint32_t)o->strength };
            return pngloss_hip_multi_optimize_batch_host_target(ctx, b->imgs, b->m, &target, (long)o->bleed, b->res, lines, zs, b->rep);
        }
    default:
        return pngloss_hip_multi_optimize_batch_host(ctx, b->imgs, b->m, (unsigned)o->strength, (long)o->bleed, b->res, lines, zs);
    }
}

/* what the call answered for entry k of the batch: the records that are valid (cli_outcome.h), and the file's status */
static void take_answer(struct job *j, const struct window_batch *b, size_t k, const struct cli_options *o, pngloss_hip_multi *ctx, int rc)
{
    bool last_distortion = false, last_ssim = false, last_palette = false;
    j->gpu = b->res[k];
    j->color_type = o->gpu_deflate ? b->zs[k].color_type : b->lines[k].color_type;
    j->zsize = b->zs[k].size;
    switch (o->search) {
    case CLI_SEARCH_SIZE:
        j->size = b->srep[k];
        j->distortion = b->srep[k].distortion;
        break;
    case CLI_SEARCH_QUALITY:
        j->target = b->rep[k];
        j->distortion = b->rep[k].distortion;
        j->ssim = b->sm[k];
        break;
    default:     /* the plain call keeps the records in the context */
        if (j->have_quant) { j->distortion = j->quant.distortion; last_distortion = o->distortion; }
        else last_distortion = o->distortion && ctx && pngloss_hip_multi_last_distortion(ctx, k, &j->distortion) == PNGLOSS_SUCCESS;
        last_ssim = o->ssim && ctx && pngloss_hip_multi_last_ssim(ctx, k, &j->ssim) == PNGLOSS_SUCCESS;
        last_palette = o->indexed && ctx && pngloss_hip_multi_last_palette(ctx, k, &j->palette) == PNGLOSS_SUCCESS;
        j->have_depth = o->have_index_depth && last_palette && pngloss_hip_multi_last_index_depth(ctx, k, &j->depth) == PNGLOSS_SUCCESS;
        break;
    }
    j->have_distortion = cli_have_distortion(o->search, o->distortion, rc, last_distortion);
    j->have_ssim = cli_have_ssim(o->search, o->ssim, o->have_target_ssim, rc, last_ssim);
    j->have_palette = cli_have_palette(o->search, o->indexed, last_palette);
    if (o->have_index_depth && j->have_palette && !j->have_depth && j->color_type == 3 && rc == PNGLOSS_SUCCESS) {
        say(j, "  error: the library returned an indexed stream without its bit depth\n");
        j->status = (pngloss_error)PNGLOSS_HIP_ERROR;
    }
    if (cli_indexed_without_palette(j->color_type, j->have_palette, rc)) {
        say(j, "  error: the library returned an indexed stream without its palette\n");
        j->status = (pngloss_error)PNGLOSS_HIP_ERROR;
    }
    if (cli_status_after_optimise(rc, b->res[k].status) != PNGLOSS_SUCCESS) {
        say(j, "  error: GPU optimisation failed (%d)\n", rc);
        j->status = (pngloss_error)rc;
    }
}

/* stages 2 and 3 of a window whose files are decoded already: every decoded image in one GPU batch, then encode (threads) */
static void run_window(struct job *jobs, size_t n, const struct cli_options *o, pngloss_hip_multi **ctx, double decode_seconds)
{
    const bool timing = getenv("PNGLOSS_TIMING") != NULL;
    const double t1 = now_s(), t0 = t1 - decode_seconds;
    struct window_batch b;
    if (!window_batch_alloc(&b, n)) return;
    collect_decoded(&b, jobs, n);
    if (o->gpu_deflate) refuse_too_large(&b, jobs);
    if (b.m) {
        const double tc0 = now_s();
        if (!*ctx) *ctx = open_contexts(o);
        if (timing) fprintf(stderr, "  [timing] GPU contexts ready after %.3f s\n", now_s() - tc0);
        if (o->search == CLI_SEARCH_SIZE) compute_budgets(&b, jobs, o);
        if (o->have_colors) quantise_batch(*ctx, &b, jobs, o);
        const int rc = b.m ? optimise_batch(*ctx, &b, o) : PNGLOSS_SUCCESS;
        for (size_t k = 0; k < b.m; k++) take_answer(&jobs[b.who[k]], &b, k, o, *ctx, rc);
    }
    window_batch_free(&b);
    const double t2 = now_s();

    for_each_job(jobs, n, o, encode_job);
    if (timing) fprintf(stderr, "  [timing] %zu files: decode %.2f s, gpu batch %.2f s, encode %.2f s\n", n, t1 - t0, t2 - t1, now_s() - t2);
}

/* every file of the call, window by window; the exit code is the error of the last failing file */
static pngloss_error run_files(const struct cli_options *o)
{
    const size_t total = o->num_files;
    struct job *jobs = calloc(total ? total : 1, sizeof *jobs);
    if (!jobs) return OUT_OF_MEMORY_ERROR;
    for (size_t i = 0; i < total; i++) {
        struct job *j = &jobs[i];
        j->in_name = o->from_stdin ? "stdin" : o->files[i];
        if (!o->to_stdout) {
            if (o->output_path) j->out_name = (char *)o->output_path;
            else { j->out_name = with_extension(j->in_name, o->extension ? o->extension : CLI_DEFAULT_EXTENSION); j->own_out_name = true; }
            if (!j->out_name) j->status = OUT_OF_MEMORY_ERROR;
            else if (!o->force && exists(j->out_name)) {
                say(j, "  error: '%s' exists; not overwriting\n", j->out_name);
                j->status = NOT_OVERWRITING_ERROR;
            }
        }
    }

    pngloss_hip_multi *ctx = NULL;
    pngloss_error latest = SUCCESS;
    unsigned errors = 0, skipped = 0;
    /* windows of up to WINDOW_FILES files: decoded (threads), optimised as ONE GPU batch, encoded (threads).  The next
     * window is decoded in the background while the current one is on the GPU (pngloss.c:173 is a sequential loop). */
    struct decode_ahead ahead;
    memset(&ahead, 0, sizeof ahead);
    /* the HIP runtime needs a quarter of a second for its first call: let it be made while the first window is read and decoded */
    pthread_t warm;
    const bool warming = total && pthread_create(&warm, NULL, warm_up_main, NULL) == 0;
    decode_ahead_start(&ahead, jobs, total < WINDOW_FILES ? total : WINDOW_FILES, o);
    for (size_t start = 0; start < total;) {
        size_t n = total - start < WINDOW_FILES ? total - start : WINDOW_FILES;
        decode_ahead_wait(&ahead);
        if (warming && start == 0) pthread_join(warm, NULL);
        const double decode_seconds = ahead.seconds;
        const size_t next = start + n, next_n = total - next < WINDOW_FILES ? total - next : WINDOW_FILES;
        if (next < total) decode_ahead_start(&ahead, jobs + next, next_n, o);
        run_window(jobs + start, n, o, &ctx, decode_seconds);
        for (size_t i = start; i < start + n; i++) {
            struct job *j = &jobs[i];
            flush_log(j);
            if (j->status != SUCCESS) {
                latest = j->status;
                if (j->status == TOO_LOW_QUALITY || j->status == TOO_LARGE_FILE) skipped++;
                else errors++;
            }
            rwpng_free_image24(&j->in);
            rwpng_free_image24(&j->out);
            free(j->filters);
            free(j->line_types);
            free(j->lines);
            if (j->own_out_name) free(j->out_name);
        }
        start += n;
    }
    if (ctx) pngloss_hip_multi_destroy(ctx);
    if (o->verbose) {
        const unsigned files = (unsigned)total;
        if (errors) fprintf(stderr, "There were errors compressing %d file%s out of a total of %d file%s.\n", errors, errors == 1 ? "" : "s", files, files == 1 ? "" : "s");
        if (skipped) fprintf(stderr, "Skipped %d file%s out of a total of %d file%s.\n", skipped, skipped == 1 ? "" : "s", files, files == 1 ? "" : "s");
        if (!skipped && !errors) fprintf(stderr, "Compressed %d image%s.\n", files, files == 1 ? "" : "s");
    }
    free(jobs);
    return latest;
}

int main(int argc, char **argv)
{
    struct cli_options o;
    pngloss_error rc = cli_options_parse(argc, argv, &o, stderr);
    if (rc != SUCCESS) return rc;
    if (o.version) { puts(PNGLOSS_VERSION); return SUCCESS; }
    if (o.missing) { print_version_banner(stderr); fputs(cli_usage_text, stderr); return MISSING_ARGUMENT; }
    if (o.help) { print_version_banner(stdout); fputs(cli_usage_text, stdout); return SUCCESS; }
    rc = cli_options_check(&o, stderr);
    if (rc == MISSING_ARGUMENT) {
        if (o.verbose) print_version_banner(stderr);
        fputs(cli_usage_text, stderr);
    }
    if (rc != SUCCESS) return rc;
    return run_files(&o);
}
