// ubench_headtrips.hip -- what ONE scalar round trip at the head of a kernel costs the segment engine (gfx950, one MI355X).
// A chain of dependent launches on one stream, with the enumeration's grid (800 workgroups of 512 threads): every kernel does N DEPENDENT scalar
// loads (each address is the word the one before returned, every step in another 128-byte line) from a record that the launch in front of it
// wrote, then exits; workgroup 0 writes the record's other copy for the launch behind it.  N = 0, 1, 2, 4, 6.
// Build both ways (the second takes the kernel's arguments in SGPRs at wave launch, as pl_seg.hip is built):
//   hipcc -O3 --offload-arch=gfx950 -o tools/ubench_headtrips tools/ubench_headtrips.hip
//   hipcc -O3 --offload-arch=gfx950 -mllvm -amdgpu-kernarg-preload-count=8 -DPRELOAD=1 -o tools/ubench_headtrips_preload tools/ubench_headtrips.hip
// Prints us per launch (HIP events over LAUNCHES back-to-back launches; minimum and median of REPS repetitions).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)
#ifndef PRELOAD
#define PRELOAD 0
#endif

#define REC_WORDS 256u          /* one copy of the record: 8 lines of 128 bytes */
#define STEP_WORDS 32u          /* a step of the chain: the next line */

typedef const __attribute__((address_space(4))) uint32_t *const_words;

template <int N>
__global__ __launch_bounds__(512) void k_head(uint32_t *rec, unsigned turn, uint32_t *sink)
{
    const_words c = (const_words)(uintptr_t)(rec + (turn & 1u) * REC_WORDS);
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < N; i++) o = c[o & (REC_WORDS - 1u)];        /* s_load_dword, s_waitcnt, N times; the mask keeps any word inside the record */
    if (blockIdx.x == 0 && threadIdx.x < REC_WORDS) rec[((turn + 1u) & 1u) * REC_WORDS + threadIdx.x] = (threadIdx.x + STEP_WORDS) & (REC_WORDS - 1u);
    if (o == 0xdeadbeefu) sink[0] = o;                              /* (never: the loads must not be dropped) */
}

template <int N>
static void run(uint32_t *rec, uint32_t *sink, hipEvent_t e0, hipEvent_t e1)
{
    const int LAUNCHES = 2000, REPS = 7;
    float us[REPS];
    for (int r = -1; r < REPS; r++) {            /* (r = -1: warm-up) */
        CK(hipEventRecord(e0, 0));
        for (int i = 0; i < LAUNCHES; i++) hipLaunchKernelGGL(k_head<N>, dim3(800), dim3(512), 0, 0, rec, (unsigned)i, sink);
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (r >= 0) us[r] = ms * 1000.0f / LAUNCHES;
    }
    std::sort(us, us + REPS);
    printf("%s  %d dependent scalar loads at the head: %.3f us per launch (median %.3f, max %.3f)\n", PRELOAD ? "arguments preloaded" : "arguments loaded   ", N, us[0], us[REPS / 2], us[REPS - 1]);
}

int main()
{
    uint32_t *rec, *sink;
    CK(hipMalloc(&rec, 2 * REC_WORDS * 4));
    CK(hipMalloc(&sink, 64));
    uint32_t h[2 * REC_WORDS];
    for (unsigned i = 0; i < 2 * REC_WORDS; i++) h[i] = ((i % REC_WORDS) + STEP_WORDS) & (REC_WORDS - 1u);
    CK(hipMemcpy(rec, h, sizeof h, hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    run<0>(rec, sink, e0, e1);
    run<1>(rec, sink, e0, e1);
    run<2>(rec, sink, e0, e1);
    run<4>(rec, sink, e0, e1);
    run<6>(rec, sink, e0, e1);
    run<0>(rec, sink, e0, e1);      /* (again: drift over the run) */
    CK(hipDeviceSynchronize());
    return 0;
}
