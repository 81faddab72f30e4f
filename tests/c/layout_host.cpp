/*
 * layout_host.cpp -- TEST INFRASTRUCTURE: the memory layouts of the host shim (pngloss_amd/csrc/pl_layout.h, the header pl_host.hip carries out)
 * behind a thin C ABI, so that the CPU suite proves alignment and disjointness and pins every offset without a GPU (tests/test_layout_host.py).
 * Everything goes out as int64.
 *
 *   layout_host_batch(w, h, n, use_rows, seg_list, nseg, n_wg, nsp, seeded, job_bytes, segjob_bytes, img[n][14], tables[4], seg[nseg][2])
 *       img: base, then WsLayout in its order (flags .. rowstat, total); tables: seg_jobs, seg_params, sel, total; seg: base, PlSegLayout::total
 *   layout_host_seg_total(width, nsp, seeded) -> pl_seg_layout(..).total      layout_host_seg_params_bytes() -> sizeof(SegParams)
 *   layout_host_rowstat_bytes(height)
 *   layout_host_window(w, h, filters, emit, n, im[n][7], tot[2])     im: px, img, flt, span, ids, rows, pitch; tot: mirrored, total
 *   layout_host_read(in[n][6], n, frames, job_bytes, stream_bytes, head[9], files[n][4], jobs[7 n][14]) -> jobs
 *       in: width, height, colour type, bit depth, interlace, zbytes (-1: no stream); head: status, zstatus, prog, zjobs, zeroed, max_bands, nprog, total, ftotal;
 *       files: raw_bytes, raw, z, out; jobs: file, raw, last, prog, ox, oy, sx, sy, pitch, nbands, lastpitch, width, height, rowbytes
 *   layout_host_adam7_pass(p, W, H, colour type, depth, out[8])      pr_adam7_pass: x0, y0, dx, dy, width, height, rowbytes, bytes
 *   layout_host_grow(need, have, divisor)    layout_host_color_type(flags)    layout_host_emit_bpp(flags)    layout_host_band_rows() -> PR_ROWS
 *   layout_host_pack(slots, packed, width, bpp)    layout_host_unpack(packed, slots, width, bpp)
 */
#include "../../pngloss_amd/csrc/pl_layout.h"

extern "C" {

void layout_host_batch(const uint32_t *w, const uint32_t *h, size_t n, int use_rows, const uint32_t *seg_list, size_t nseg, size_t n_wg, uint32_t nsp,
                       int seeded, size_t job_bytes, size_t segjob_bytes, int64_t *img, int64_t *tables, int64_t *seg)
{
    const PlBatchLayout b = pl_batch_layout(std::vector<uint32_t>(w, w + n), std::vector<uint32_t>(h, h + n), use_rows != 0,
                                            std::vector<uint32_t>(seg_list, seg_list + nseg), n_wg, nsp, seeded != 0, job_bytes, segjob_bytes);
    for (size_t i = 0; i < n; i++) {
        const WsLayout &l = b.ws[i];
        const size_t v[14] = { b.image[i], l.flags, l.orig_hist, l.orig_rank, l.cand, l.err0, l.err1, l.old_above, l.final_hist, l.result, l.row_ids, l.out_flags, l.rowstat, l.total };
        for (int k = 0; k < 14; k++) img[14 * i + k] = (int64_t)v[k];
    }
    tables[0] = (int64_t)b.seg_jobs; tables[1] = (int64_t)b.seg_params; tables[2] = (int64_t)b.sel; tables[3] = (int64_t)b.total;
    for (size_t k = 0; k < b.seg.size(); k++) { seg[2 * k] = (int64_t)b.seg_image[k]; seg[2 * k + 1] = (int64_t)b.seg[k].total; }
}

int64_t layout_host_seg_total(uint32_t width, uint32_t nsp, int seeded) { return (int64_t)pl_seg_layout(width, nsp, seeded != 0).total; }
int64_t layout_host_seg_params_bytes(void) { return (int64_t)sizeof(SegParams); }
int64_t layout_host_rowstat_bytes(uint32_t height) { return (int64_t)pl_rowstat_bytes(height); }

void layout_host_window(const uint32_t *w, const uint32_t *h, const uint8_t *filters, const uint8_t *emit, size_t n, int64_t *im, int64_t *tot)
{
    std::vector<PlWindowIn> in(n);
    for (size_t i = 0; i < n; i++) in[i] = PlWindowIn{ w[i], h[i], filters[i] != 0, emit[i] != 0 };
    const PlWindowLayout l = pl_window_layout(in);
    for (size_t i = 0; i < n; i++) {
        const PlWindowImage &m = l.im[i];
        const size_t v[7] = { m.px, m.img, m.flt, m.span, m.ids, m.rows, m.pitch };
        for (int k = 0; k < 7; k++) im[7 * i + k] = (int64_t)v[k];
    }
    tot[0] = (int64_t)l.mirrored; tot[1] = (int64_t)l.total;
}

int64_t layout_host_read(const int64_t *in, size_t n, int frames, size_t job_bytes, size_t stream_bytes, int64_t *head, int64_t *files, int64_t *jobs)
{
    std::vector<PlReadIn> f(n);
    for (size_t i = 0; i < n; i++) {
        const int64_t *s = in + 6 * i;
        f[i] = PlReadIn{ (uint32_t)s[0], (uint32_t)s[1], (int)s[2], (int)s[3], (int)s[4], s[5] < 0 ? PL_READ_NO_STREAM : (uint64_t)s[5] };
    }
    const PlReadLayout r = pl_read_layout(f, frames != 0, job_bytes, stream_bytes);
    const size_t hv[9] = { r.status, r.zstatus, r.prog, r.zjobs, r.zeroed, r.max_bands, r.nprog, r.total, r.ftotal };
    for (int k = 0; k < 9; k++) head[k] = (int64_t)hv[k];
    for (size_t i = 0; i < n; i++) {
        const PlReadFile &o = r.file[i];
        files[4 * i] = (int64_t)o.raw_bytes; files[4 * i + 1] = (int64_t)o.raw; files[4 * i + 2] = (int64_t)o.z; files[4 * i + 3] = (int64_t)o.out;
    }
    for (size_t k = 0; k < r.job.size(); k++) {
        const PlReadJob &j = r.job[k];
        const size_t v[14] = { j.file, j.raw, j.last, j.prog, j.ox, j.oy, j.sx, j.sy, j.pitch, j.nbands, j.lastpitch, j.width, j.height, j.rowbytes };
        for (int q = 0; q < 14; q++) jobs[14 * k + q] = (int64_t)v[q];
    }
    return (int64_t)r.job.size();
}

void layout_host_adam7_pass(int p, uint32_t W, uint32_t H, int color_type, int depth, int64_t *out)
{
    const PrPass s = pr_adam7_pass(p, W, H, color_type, depth);
    const uint64_t v[8] = { s.x0, s.y0, s.dx, s.dy, s.width, s.height, s.rowbytes, s.bytes };
    for (int k = 0; k < 8; k++) out[k] = (int64_t)v[k];
}

int64_t layout_host_grow(size_t need, size_t have, size_t divisor) { return (int64_t)pl_grow_bytes(need, have, divisor); }
int layout_host_color_type(uint32_t flags) { return pl_color_type_of(flags); }
int layout_host_emit_bpp(uint32_t flags) { return (int)pl_emit_bpp_of(flags); }
int layout_host_band_rows(void) { return PR_ROWS; }
void layout_host_pack(uint32_t *slots, const unsigned char *packed, uint32_t width, uint32_t bpp) { pl_pack_row(slots, packed, width, bpp); }
void layout_host_unpack(unsigned char *packed, const uint32_t *slots, uint32_t width, uint32_t bpp) { pl_unpack_row(packed, slots, width, bpp); }

} /* extern "C" */
