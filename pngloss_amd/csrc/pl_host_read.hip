/*
 * pl_host_read.hip -- the host side of the PNG read path (pl_pngread, pl_inflate): scanlines or zlib streams up, decoded RGBA8 down or left on the
 * device for the optimiser (pl_host_ctx.h has the map of the host files).  Where everything lies is pl_layout.h's (pl_read_layout).
 */
#include "pl_host_ctx.h"

/* `interlace` sits where both source structs had padding: their size and every other member's offset are what they were before it */
static_assert(sizeof(pngloss_hip_png_source) == 64 && offsetof(pngloss_hip_png_source, interlace) == 18 && offsetof(pngloss_hip_png_source, palette) == 24 &&
              offsetof(pngloss_hip_png_source, palette_entries) == 32 && offsetof(pngloss_hip_png_source, trns) == 40 &&
              offsetof(pngloss_hip_png_source, trns_bytes) == 48 && offsetof(pngloss_hip_png_source, rgba) == 56, "pngloss_hip_png_source layout");
static_assert(sizeof(pngloss_hip_png_zsource) == 64 && offsetof(pngloss_hip_png_zsource, interlace) == 26 && offsetof(pngloss_hip_png_zsource, palette) == 32 &&
              offsetof(pngloss_hip_png_zsource, palette_entries) == 40 && offsetof(pngloss_hip_png_zsource, trns) == 48 &&
              offsetof(pngloss_hip_png_zsource, trns_bytes) == 56, "pngloss_hip_png_zsource layout");
namespace {
/* d_out == nullptr: the decoded images are downloaded to src[i].rgba.  Else they STAY on the device, in the context's frame arena (apart
 * from the workspace the optimiser carves up), and d_out[i] receives their device pointers. */
/* zs != nullptr: src[i].scanlines is not used; the scanlines are INFLATED ON THE DEVICE from zs[i] (the concatenated IDAT payloads), one wave per file */
struct ZRef { const unsigned char *z; size_t bytes; };
/* per_image: set once the batch as a whole went through -- from there on the return value is the worst PER-IMAGE status and status[] explains it.
 * A return before that point is a failure of the WHOLE batch (bad argument, allocation, copy, launch, device fault): png_decode_common then
 * writes that code into every status[i], so that a caller who looks at status[] alone never takes an undecoded image for a decoded one. */
int png_decode_body(pngloss_hip_ctx *ctx, const pngloss_hip_png_source *src, size_t n, int *status, void **d_out, hipStream_t stream, const ZRef *zs, bool &per_image)
{
    if (!ctx || (!src && n)) return PNGLOSS_INVALID_ARGUMENT;
    if (status) for (size_t i = 0; i < n; i++) status[i] = PNGLOSS_SUCCESS;
    if (d_out) for (size_t i = 0; i < n; i++) d_out[i] = nullptr;
    if (!n) { per_image = true; return PNGLOSS_SUCCESS; }
    if (batch_in_flight_refused(ctx)) return PNGLOSS_INVALID_ARGUMENT;       /* (the workspace this call carves up belongs to the batch in flight) */
    PL_CHECK(hipSetDevice(ctx->device));
    std::vector<PrFormat> fmt(n);
    std::vector<PlReadIn> in(n);
    static const unsigned char bad_stream[6] = { 0, 0, 0, 0, 0, 0 };       /* (CMF 0: not deflate) */
    std::vector<ZRef> zsub(zs ? n : 0);
    for (size_t i = 0; i < n; i++) {
        if ((!zs && !src[i].scanlines) || (zs && !zs[i].z) || (!d_out && !src[i].rgba)) return PNGLOSS_INVALID_ARGUMENT;
        if (src[i].interlace > 1) {
            std::fprintf(stderr, "pngloss_hip: image %zu: interlace method %d (0 = none, 1 = Adam7; the struct has to be zero-initialised)\n", i, src[i].interlace);
            return PNGLOSS_INVALID_ARGUMENT;
        }
        /* a stream too short to be zlib's (header + one block + Adler-32) or beyond the inflater's 32-bit positions is THAT file's problem: it gets
         * status 25 like any other stream the inflater refuses (it is handed a six-byte stream with an invalid header), the batch goes on */
        if (zs && (zs[i].bytes < 6 || zs[i].bytes > 0xFFFFFFF0u)) zsub[i] = ZRef{ bad_stream, sizeof bad_stream };
        else if (zs) zsub[i] = zs[i];
        PrFormat &F = fmt[i];
        if (!pr_format(F, src[i].width, src[i].height, src[i].color_type, src[i].bit_depth, src[i].palette, src[i].palette_entries, src[i].trns, src[i].trns_bytes)) {
            std::fprintf(stderr, "pngloss_hip: image %zu: colour type %d with bit depth %d (or an empty image / a palette image without PLTE) is not a PNG format\n", i, src[i].color_type, src[i].bit_depth);
            return PNGLOSS_INVALID_ARGUMENT;
        }
        if (zs && pr_scanline_bytes(F.width, F.height, F.color_type, F.bit_depth, src[i].interlace) > 0xFFFFFFF0u) return PNGLOSS_INVALID_ARGUMENT;     /* (32-bit positions in the inflater) */
        in[i] = PlReadIn{ F.width, F.height, F.color_type, F.bit_depth, src[i].interlace, zs ? (uint64_t)zsub[i].bytes : PL_READ_NO_STREAM };
    }
    /* where everything lies (pl_layout.h): the tables in front -- jobs, then the status words of the decode and of the inflate and the progress words
     * (zeroed by one memset), then the inflate's streams --, the files' data behind them.  (Every job carries its format, palette included: 1.1 KB a
     * pass.  A first version whose jobs pointed at one format per file had a table 4.6 MB smaller at 768 interlaced files, but a kernel 13 % slower
     * on plain files: DESIGN.md section 9.2) */
    const PlReadLayout lay = pl_read_layout(in, d_out != nullptr, sizeof(PrJob), sizeof(PliStream));
    const size_t m = lay.job.size(), total = lay.total, ftotal = lay.ftotal;
    const auto tr0 = std::chrono::steady_clock::now();
    auto ms_since = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tr0).count(); };
    int rc = ctx->d_ws.grow(total, 4);
    if (rc == PNGLOSS_SUCCESS && d_out) rc = ctx->d_frames.grow(ftotal, 4);
    if (rc) return rc;
    const double ms_ws = ms_since();
    /* offsets into pointers: here and nowhere else */
    char *const b = ctx->d_ws.p, *const fb = d_out ? ctx->d_frames.p : b;
    int32_t *d_status = reinterpret_cast<int32_t *>(b + lay.status), *d_zstatus = reinterpret_cast<int32_t *>(b + lay.zstatus);
    uint32_t *d_prog = reinterpret_cast<uint32_t *>(b + lay.prog);
    PliStream *d_zjobs = reinterpret_cast<PliStream *>(b + lay.zjobs);
    auto d_raw = [&](size_t i) { return reinterpret_cast<uint8_t *>(b + lay.file[i].raw); };
    auto d_z = [&](size_t i) { return reinterpret_cast<uint8_t *>(b + lay.file[i].z); };
    auto d_rgba = [&](size_t i) { return fb + lay.file[i].out; };
    std::vector<PrJob> jobs(m);
    for (size_t k = 0; k < m; k++) {
        const PlReadJob &a = lay.job[k];
        PrJob &j = jobs[k];
        j.F = fmt[a.file];                                                    /* (a pass: the file's format with the pass's geometry) */
        j.F.width = a.width; j.F.height = a.height; j.F.rowbytes = a.rowbytes;
        j.ox = a.ox; j.oy = a.oy; j.sx = a.sx; j.sy = a.sy; j.pitch = a.pitch;
        j.nbands = a.nbands; j.lastpitch = a.lastpitch;
        j.raw = reinterpret_cast<const uint8_t *>(b + a.raw);
        j.rgba = reinterpret_cast<uint32_t *>(d_rgba(a.file));
        j.lastrow = reinterpret_cast<uint8_t *>(b + a.last);
        j.progress = d_prog + a.prog;
        j.status = d_status + a.file;
    }
    std::vector<PliStream> zjobs(zs ? n : 0);
    PL_CHECK(hipMemsetAsync(d_status, 0, lay.zeroed, stream));
    for (size_t i = 0; i < n; i++) {
        /* (from pinned memory -- pngloss_hip_pinned_alloc -- this is one DMA; from pageable memory the runtime stages it: 33 ms against 1.3 for 64 MiB) */
        if (zs) {
            PL_CHECK(hipMemcpyAsync(d_z(i), zsub[i].z, zsub[i].bytes, hipMemcpyHostToDevice, stream));
            zjobs[i].z = d_z(i); zjobs[i].zbytes = (uint32_t)zsub[i].bytes;
            zjobs[i].out = d_raw(i); zjobs[i].expect = (uint32_t)lay.file[i].raw_bytes;
            zjobs[i].status = d_zstatus + i;
        } else
        PL_CHECK(hipMemcpyAsync(d_raw(i), src[i].scanlines, lay.file[i].raw_bytes, hipMemcpyHostToDevice, stream));
    }
    PL_CHECK(hipMemcpyAsync(b, jobs.data(), sizeof(PrJob) * m, hipMemcpyHostToDevice, stream));
    if (zs) {
        PL_CHECK(hipMemcpyAsync(d_zjobs, zjobs.data(), sizeof(PliStream) * n, hipMemcpyHostToDevice, stream));
        PL_CHECK(pl_launch_inflate(d_zjobs, n, stream));
    }
    const bool seam_dbg = ctx->hooks.debug_seam;
    double ms_up = 0, ms_k = 0;
    if (seam_dbg) { PL_CHECK(hipStreamSynchronize(stream)); ms_up = ms_since(); }
    PL_CHECK(pl_launch_png_decode(reinterpret_cast<const PrJob *>(b), m, lay.max_bands, stream));
    if (seam_dbg) { PL_CHECK(hipStreamSynchronize(stream)); ms_k = ms_since(); }
    std::vector<int32_t> st(n), zst(n, 0);
    if (zs) PL_CHECK(hipMemcpyAsync(zst.data(), d_zstatus, sizeof(int32_t) * n, hipMemcpyDeviceToHost, stream));
    if (!d_out)
        for (size_t i = 0; i < n; i++)
            PL_CHECK(hipMemcpyAsync(src[i].rgba, d_rgba(i), (size_t)src[i].width * src[i].height * 4, hipMemcpyDeviceToHost, stream));
    PL_CHECK(hipMemcpyAsync(st.data(), d_status, sizeof(int32_t) * n, hipMemcpyDeviceToHost, stream));
    PL_CHECK(hipStreamSynchronize(stream));
    if (seam_dbg) std::fprintf(stderr, "pngloss_hip: read side: %zu files, workspace %zu MB ready after %.1f ms, upload %.1f ms, unfilter + expand %.1f ms, %s %.1f ms\n", n, (total + ftotal) >> 20, ms_ws, ms_up - ms_ws, ms_k - ms_up, d_out ? "status (the frames stay on the device)" : "download", ms_since() - ms_k);
    /* every image has been decoded (and downloaded); the ones that failed say so -- one damaged file does not take the window with it */
    per_image = true;
    int worst = PNGLOSS_SUCCESS;
    for (size_t i = 0; i < n; i++) {
        if (d_out) d_out[i] = d_rgba(i);
        if (zst[i]) {
            /* the stream is not one the device inflater takes (damaged, or beyond what it checks): the caller reads the file on the host */
            std::fprintf(stderr, "pngloss_hip: image %zu: the device inflater stopped (code %d): corrupt or unusual zlib stream\n", i, zst[i]);
            if (status) status[i] = 25;
            if (worst == PNGLOSS_SUCCESS) worst = 25;
            continue;
        }
        if (!st[i]) continue;
        const int code = st[i] == 25 ? 25 : PNGLOSS_HIP_ERROR;
        if (st[i] == 25) std::fprintf(stderr, "pngloss_hip: image %zu: a scanline has a filter type beyond 4 (corrupt stream)\n", i);
        else std::fprintf(stderr, "pngloss_hip: image %zu: the row bands of the decoder lost step (internal error %d)\n", i, st[i]);
        if (status) status[i] = code;
        if (worst == PNGLOSS_SUCCESS || code == PNGLOSS_HIP_ERROR) worst = code;
    }
    return worst;
}
int png_decode_common(pngloss_hip_ctx *ctx, const pngloss_hip_png_source *src, size_t n, int *status, void **d_out, hipStream_t stream, const ZRef *zs = nullptr)
{
    bool per_image = false;
    const int rc = png_decode_body(ctx, src, n, status, d_out, stream, zs, per_image);
    if (!per_image && rc != PNGLOSS_SUCCESS) {
        /* the batch as a whole failed: nothing in rgba / d_out is a decoded image */
        if (status) for (size_t i = 0; i < n; i++) status[i] = rc;
        if (d_out) for (size_t i = 0; i < n; i++) d_out[i] = nullptr;
    }
    return rc;
}
} // namespace

extern "C" {

int pngloss_hip_png_decode_batch_host(pngloss_hip_ctx *ctx, const pngloss_hip_png_source *src, size_t n)
{
    return pngloss_hip_png_decode_batch_host_status(ctx, src, n, nullptr);
}

int pngloss_hip_png_decode_batch_host_status(pngloss_hip_ctx *ctx, const pngloss_hip_png_source *src, size_t n, int *status)
{
    return png_decode_common(ctx, src, n, status, nullptr, nullptr);
}

int pngloss_hip_png_decode_batch_device(pngloss_hip_ctx *ctx, const pngloss_hip_png_source *src, size_t n, void **d_rgba, int *status, void *stream)
{
    if (!d_rgba && n) return PNGLOSS_INVALID_ARGUMENT;
    return png_decode_common(ctx, src, n, status, d_rgba, static_cast<hipStream_t>(stream));
}

int pngloss_hip_png_decode_batch_device_z(pngloss_hip_ctx *ctx, const pngloss_hip_png_zsource *zsrc, size_t n, void **d_rgba, int *status, void *stream)
{
    if ((!d_rgba || !zsrc) && n) return PNGLOSS_INVALID_ARGUMENT;
    std::vector<pngloss_hip_png_source> src(n);
    std::vector<ZRef> zs(n);
    for (size_t i = 0; i < n; i++) {
        src[i] = pngloss_hip_png_source{ nullptr, zsrc[i].width, zsrc[i].height, zsrc[i].color_type, zsrc[i].bit_depth, zsrc[i].interlace, zsrc[i].palette, zsrc[i].palette_entries, zsrc[i].trns, zsrc[i].trns_bytes, nullptr };
        zs[i] = ZRef{ zsrc[i].zstream, zsrc[i].zbytes };
    }
    return png_decode_common(ctx, src.data(), n, status, d_rgba, static_cast<hipStream_t>(stream), zs.data());
}

} /* extern "C" */
