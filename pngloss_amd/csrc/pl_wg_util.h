/*
 * pl_wg_util.h -- workgroup engine (pl_engine.hip), part 1: what every stage uses -- DPP and wave reductions, single instructions the compiler does not pick
 * by itself, and the pointer types that keep an address space.  A part of pl_engine.hip: included inside its anonymous namespace, not a header of its own.
 */
#ifndef PL_WG_UTIL_H
#define PL_WG_UTIL_H

/* ---- DPP helpers (wave64, 16-lane rows) ---------------------------------------------------------------- */
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}
/* max over the 16 lanes of a DPP row, result in every lane of the row: row_ror 8,4,2,1 butterfly */
__device__ __forceinline__ uint32_t rowmax_u32(uint32_t v)
{
    v = max(v, dpp_u32<0x128>(v));
    v = max(v, dpp_u32<0x124>(v));
    v = max(v, dpp_u32<0x122>(v));
    v = max(v, dpp_u32<0x121>(v));
    return v;
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float recip_up(int d)
{
    /* smallest float strictly above the correctly rounded 1/d: see pl_truncdiv_f */
    return __uint_as_float(__float_as_uint(1.0f / (float)d) + 2u);   /* +2 ulp: safe even if the device division were 1 ulp low */
}


/* LDS pointers keep their address space across the (non-inlined) per-filter chain functions, so the compiler emits
 * ds_* instead of flat_* accesses */
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) u32x2 lds_uint2;
typedef __attribute__((address_space(3))) u32x4 lds_uint4;
typedef __attribute__((address_space(3))) uint32_t lds_u32;
/* pointers loaded from the job table are generic; accesses through them would be FLAT instructions, which count in
 * lgkmcnt and make every wait for an LDS result also wait for outstanding global stores.  Name the address space. */
typedef __attribute__((address_space(1))) uint32_t glb_u32;
typedef __attribute__((address_space(1))) const uint32_t glb_cu32;
typedef __attribute__((address_space(1))) const u32x2 glb_cu32x2;

__device__ __forceinline__ uint32_t sad_u32(uint32_t a, uint32_t b)
{
    uint32_t r;
    asm("v_sad_u32 %0, %1, %2, 0" : "=v"(r) : "v"(a), "v"(b));   /* |a - b| */
    return r;
}

__device__ __forceinline__ int med3_i32(int v, int lo, int hi)
{
    int r;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(v), "v"(lo), "v"(hi));
    return r;
}

/* max over an aligned group of GL (16 or 8) lanes, result in every lane of the group */
template <int GL>
__device__ __forceinline__ uint32_t groupmax_u32(uint32_t v)
{
    if (GL == 16) return rowmax_u32(v);
    v = max(v, dpp_u32<0xB1>(v));    /* quad_perm [1,0,3,2] */
    v = max(v, dpp_u32<0x4E>(v));    /* quad_perm [2,3,0,1] */
    v = max(v, dpp_u32<0x141>(v));   /* row_half_mirror     */
    return v;
}

#endif
