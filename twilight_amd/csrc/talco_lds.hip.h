// twilight_amd/csrc/talco_lds.hip.h -- the LDS primitives of talco_lean_kernel (talco_nuc.hip.h): loads and stores at a byte address kept in a
// register, ds atomics on (address register + immediate offset), the workgroup barrier that waits for LDS traffic only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace twl {

typedef float nuc_f4 __attribute__((ext_vector_type(4)));
typedef float nuc_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float4 lds_ld128(unsigned addr)      // one ds_read_b128 at a byte address kept in a register
{
    const nuc_f4 v = *reinterpret_cast<const __attribute__((address_space(3))) nuc_f4 *>((const __attribute__((address_space(3))) char *)nullptr + addr);
    return make_float4(v.x, v.y, v.z, v.w);
}
typedef int nuc_i2 __attribute__((ext_vector_type(2)));
typedef int nuc_i4 __attribute__((ext_vector_type(4)));
template <class T>
__device__ __forceinline__ T lds_ld(unsigned addr)
{
    return *reinterpret_cast<const __attribute__((address_space(3))) T *>((const __attribute__((address_space(3))) char *)nullptr + addr);
}
template <class T>
__device__ __forceinline__ void lds_st(unsigned addr, T v)
{
    *reinterpret_cast<__attribute__((address_space(3))) T *>((__attribute__((address_space(3))) char *)nullptr + addr) = v;
}
template <int OFF>
__device__ __forceinline__ void lds_max_u32_off(unsigned addr, unsigned v) { asm volatile("ds_max_u32 %0, %1 offset:%2" ::"v"(addr), "v"(v), "n"(OFF) : "memory"); }
template <int OFF>
__device__ __forceinline__ void lds_max_f32_off(unsigned addr, float v) { asm volatile("ds_max_f32 %0, %1 offset:%2" ::"v"(addr), "v"(v), "n"(OFF) : "memory"); }
// ds atomics on (address register + immediate offset)
#define TWL_LDS_ATOM(NAME)                                                                                                     \
    template <int OFF>                                                                                                         \
    __device__ __forceinline__ void NAME##_off(unsigned addr, int v) { asm volatile(#NAME " %0, %1 offset:%2" ::"v"(addr), "v"(v), "n"(OFF) : "memory"); }
TWL_LDS_ATOM(ds_min_i32)
TWL_LDS_ATOM(ds_max_i32)
TWL_LDS_ATOM(ds_or_b32)
#undef TWL_LDS_ATOM
// Workgroup barrier that waits for this wave's LDS traffic only.  __syncthreads() also drains the vector-memory counter, which
// makes every eighth diagonal wait for the round trip of its traceback store; those stores are only read after the tile's
// final __syncthreads().
__device__ __forceinline__ void wg_barrier_lds() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ void lds_max_u32(unsigned addr, unsigned v) { asm volatile("ds_max_u32 %0, %1" ::"v"(addr), "v"(v) : "memory"); }
__device__ __forceinline__ void lds_max_f32(unsigned addr, float v) { asm volatile("ds_max_f32 %0, %1" ::"v"(addr), "v"(v) : "memory"); }

}  // namespace twl
