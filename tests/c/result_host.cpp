/*
 * result_host.cpp -- TEST INFRASTRUCTURE: the per-image result record (pngloss_amd/csrc/pl_result.h: the slots the kernels write and the one decoder
 * that pl_host.hip's finish() and pngloss_hip_last_engine_info call) behind a thin C ABI, so that the CPU suite pins what the library reports for
 * a record without a GPU (tests/test_result_host.py).  That no two slots of an engine overlap is first the header's static_asserts, checked
 * when this file compiles.
 *
 *   result_host_words()                                  -> PLR_WORDS
 *   result_host_decode(r[PLR_WORDS], engine, res[5], info[PLR_INFO_WORDS])
 *   result_host_layout(engine, ranges[2 * PLR_WORDS])    -> the number of {base, count} pairs of the engine's table, or -1
 */
#include "../../pngloss_amd/csrc/pl_result.h"

extern "C" {

int result_host_words(void) { return PLR_WORDS; }

void result_host_decode(const int32_t *r, int engine, uint32_t *res, int32_t *info)
{
    pngloss_hip_result d;
    pl_result_decode(r, engine, &d, info);
    res[0] = (uint32_t)d.status; res[1] = d.bytes_per_pixel; res[2] = d.unique_symbols; res[3] = d.retried_rows; res[4] = d.repaired_pixels;
}

int result_host_layout(int engine, int32_t *ranges)
{
    auto put = [&](const auto &table) {
        int k = 0;
        for (const PlrRange &x : table) { ranges[2 * k] = x.base; ranges[2 * k + 1] = x.count; k++; }
        return k;
    };
    if (engine == PLR_ENGINE_WG) return put(PLR_LAYOUT_WG);
    if (engine == PLR_ENGINE_SEG) return put(PLR_LAYOUT_SEG);
    if (engine == PLR_ENGINE_ROWS) return put(PLR_LAYOUT_ROWS);
    return -1;
}

} /* extern "C" */
