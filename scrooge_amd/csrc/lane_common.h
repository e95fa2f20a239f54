// lane_common.h — what the one-pair-per-lane aligner kernels with the table in registers share (genasm_lane_kernel.hip,
// genasm_lane_wide_kernel.hip, genasm_lane_parts_kernel.hip): the truth tables and instruction helpers of their tables and
// walks, and the wavefront priority rotation.  (Helpers that the GenASM-row kernels use as well are in genasm_device.h.)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "genasm_kernels.h"
#include "genasm_device.h"

namespace scrg {

// truth tables (inputs a, b, c in that order)
// (two-input operations are left to plain and/or/xor: 4-byte encodings, a v_bitop3_b32 takes 8)
constexpr int TT_XH  = bitop3_table([](int sum, int pv, int eq) { return (sum ^ pv) | eq; });
constexpr int TT_PH  = bitop3_table([](int mv, int xh, int pv) { return mv | ~(xh | pv); });
constexpr int TT_PVN = bitop3_table([](int mhs, int xv, int phs) { return mhs | ~(xv | phs); });
constexpr int TT_NOR3 = bitop3_table([](int a, int b, int c) { return ~(a | b | c); });
constexpr int TT_NIV  = bitop3_table([](int nv1, int v0, int stop) { return nv1 | ~v0 | stop; });     // not (insertion), or the stop row
constexpr int TT_ANDN = bitop3_table([](int a, int b, int) { return a & ~b; });
constexpr int TT_BFI = bitop3_table([](int a, int b, int c) { return (a & c) | (b & ~c); });       // bits of a where c is set, else b
constexpr int TT_ANDOR = bitop3_table([](int a, int b, int c) { return (a & b) | c; });
constexpr int TT_V0  = bitop3_table([](int pvn, int ph, int xh) { return pvn | ~(ph | xh); });

// LDS accesses by 32-bit LDS address (no generic-pointer arithmetic in front of the ds instruction)
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) u32x2_t lds_u32x2_t;
__device__ __forceinline__ uint2 lds_read64(uint32_t addr)
{
    const u32x2_t v = *reinterpret_cast<const lds_u32x2_t*>((uintptr_t)addr);
    return make_uint2(v.x, v.y);
}
__device__ __forceinline__ void lds_write64(uint32_t addr, uint2 v)
{
    u32x2_t w;
    w.x = v.x;
    w.y = v.y;
    *reinterpret_cast<lds_u32x2_t*>((uintptr_t)addr) = w;
}

__device__ __forceinline__ uint32_t ffbh_u32(uint32_t v)      // count leading zeros; 0xffffffff for v == 0
{
    uint32_t r;
    asm("v_ffbh_u32 %0, %1" : "=v"(r) : "v"(v));
    return r;
}

__device__ __forceinline__ uint32_t ffbl_u32(uint32_t v)      // count trailing zeros; 0xffffffff for v == 0
{
    uint32_t r;
    asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(v));
    return r;
}

// q + 2 * bit as ONE instruction, and as written (the optimiser otherwise sums the bits of an iteration first and rebuilds every
// slot offset from the offset at the start of the iteration: one more instruction per slot)
__device__ __forceinline__ uint32_t add_twice(uint32_t q, uint32_t bit)
{
    uint32_t r;
    asm("v_lshl_add_u32 %0, %1, 1, %2" : "=v"(r) : "v"(bit), "v"(q));
    return r;
}

__device__ __forceinline__ uint32_t mad24(uint32_t a, uint32_t b, uint32_t c)      // a * b + c for a, b < 2^24, as written (v_mad_u32_u24)
{
    uint32_t r;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(b), "v"(c));
    return r;
}

__device__ __forceinline__ uint32_t add3(uint32_t a, uint32_t b, uint32_t c)       // a + b + c (c wave-uniform), as written (v_add3_u32)
{
    uint32_t r;
    asm("v_add3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c));
    return r;
}

__device__ __forceinline__ uint64_t shl64(uint64_t v, uint32_t s)      // one v_lshlrev_b64 (count modulo 64)
{
    uint64_t r;
    asm("v_lshlrev_b64 %0, %1, %2" : "=v"(r) : "v"(s), "v"(v));
    return r;
}
__device__ __forceinline__ uint64_t shr64(uint64_t v, uint32_t s)
{
    uint64_t r;
    asm("v_lshrrev_b64 %0, %1, %2" : "=v"(r) : "v"(s), "v"(v));
    return r;
}
__device__ __forceinline__ uint32_t clz64(uint64_t v)                  // 64 for v == 0 (through 0xffffffff + 32 -> min)
{
    return min(ffbh_u32((uint32_t)(v >> 32)), ffbh_u32((uint32_t)v) + 32u);
}

// hardware wave slot on my SIMD (HW_ID bits 3:0)
__device__ __forceinline__ uint32_t hw_wave_slot()
{
    return __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 4);
}

// The SIMD's arbiter issues oldest-wave-first: left alone, the first wavefront on a SIMD runs at the speed of a lone wave and
// the last one finishes 2.7x later, with the SIMD half idle at the end of a launch.  Rotating the priorities (one step per
// round, starting from the wave slot: a different wavefront is on top from round to round) lets the wavefronts of a SIMD
// progress, and finish, together.  (Until round 4 the rotation was keyed on the clock: s_memtime and the wait for it — which
// is a wait for every LDS operation in flight as well — cost a wavefront that has its SIMD to itself ~1 000 cycles per round:
// one launch of 100 k pairs 2.45 -> 2.30 ms without it.)
__device__ __forceinline__ void rotate_priority(uint32_t round)
{
    const uint32_t pr = round & 3u;
    if (pr == 0) __builtin_amdgcn_s_setprio(0);
    else if (pr == 1) __builtin_amdgcn_s_setprio(1);
    else if (pr == 2) __builtin_amdgcn_s_setprio(2);
    else __builtin_amdgcn_s_setprio(3);
}

}  // namespace scrg
