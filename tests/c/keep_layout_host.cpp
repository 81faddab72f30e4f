/*
 * keep_layout_host.cpp -- TEST INFRASTRUCTURE: the keep arena of the distortion measurement (pl_keep_layout, pngloss_amd/csrc/pl_layout.h) behind a
 * thin C ABI, as tests/c/layout_host.cpp does for the other layouts of the host shim (tests/test_keep_layout_host.py).  Everything goes out as int64.
 *
 *   keep_layout_host(w, h, n, originals, job_bytes, record_bytes, image[n], tables[3])     tables: jobs, records, total
 */
#include "../../pngloss_amd/csrc/pl_layout.h"

extern "C" void keep_layout_host(const uint32_t *w, const uint32_t *h, size_t n, int originals, size_t job_bytes, size_t record_bytes, int64_t *image, int64_t *tables)
{
    const PlKeepLayout k = pl_keep_layout(std::vector<uint32_t>(w, w + n), std::vector<uint32_t>(h, h + n), originals != 0, job_bytes, record_bytes);
    for (size_t i = 0; i < n; i++) image[i] = (int64_t)k.image[i];
    tables[0] = (int64_t)k.jobs; tables[1] = (int64_t)k.records; tables[2] = (int64_t)k.total;
}
