/*
 * pl_move_core.h -- the thread loop of pl_move (pl_target.hip): a batched copy of byte ranges that need not be aligned (an image's pixels are, its
 * row filters are `height` bytes wherever the caller put them).  Shared with tests/c/target_host.cpp, which runs it on the CPU under the sanitizers.
 * As pl_keep: 16 bytes per lane and step where both sides start on a 16-byte boundary, then words, then bytes.
 */
#ifndef PL_MOVE_CORE_H
#define PL_MOVE_CORE_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PLM_HD __host__ __device__ __forceinline__
#else
#define PLM_HD inline
#endif

/* one job: `bytes` bytes from src to dst (device memory; the ranges of one launch do not overlap) */
struct PlMoveJob {
    const void *src;
    void *dst;
    uint64_t bytes;
};

struct alignas(16) PlmQuad { uint32_t w[4]; };

/* the share of thread `tid` of `nthreads` */
PLM_HD void plm_thread(const void *src, void *dst, size_t bytes, size_t tid, size_t nthreads)
{
    const uintptr_t both = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst);
    size_t done = 0;
    if (!(both & 15u)) {
        const size_t n16 = bytes / 16;
        const PlmQuad *s = static_cast<const PlmQuad *>(src);
        PlmQuad *d = static_cast<PlmQuad *>(dst);
        for (size_t i = tid; i < n16; i += nthreads) d[i] = s[i];
        done = n16 * 16;
    }
    if (!(both & 3u)) {
        const size_t n4 = (bytes - done) / 4;
        const uint32_t *s = reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(src) + done);
        uint32_t *d = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(dst) + done);
        for (size_t i = tid; i < n4; i += nthreads) d[i] = s[i];
        done += n4 * 4;
    }
    const uint8_t *s = static_cast<const uint8_t *>(src);
    uint8_t *d = static_cast<uint8_t *>(dst);
    for (size_t i = done + tid; i < bytes; i += nthreads) d[i] = s[i];
}

#endif
