// nfk_mfma.h -- the MFMA and LDS-DMA primitives every fp16-split kernel uses.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma16(h8 a, h8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// the tail step: K = 16 over the packed (hi, hi, lo, 0) x (a_hi, a_lo, a_hi, -) groups
__device__ __forceinline__ f32x4 mfma16k16(h4 a, h4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0);
}

// LDS-DMA is issued through inline asm and waited for by hand: the compiler
// cannot prove that a DMA into one slot does not alias reads of the other, so
// with the builtin it drains every DMA (vmcnt(0)) before the first ds_read of
// each phase -- serialising the copy of phase p+1 with the compute of phase p.
// Invariant instead: a DMA issued right after the barrier that ends phase p
// is waited for (vmcnt(0)) at the barrier that ends phase p+1, and the kernel
// issues no other VGPR-destination global loads while DMAs are in flight.
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)p;
}

// one 16-byte LDS-DMA per lane (m0 = the LDS base of the wave's 1-KiB block)
__device__ __forceinline__ void dma16(const float* gsrc, uint32_t lds) {
    uint32_t saved;  // m0 is reserved by the compiler: restore it
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %2, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(saved)
                 : "s"(__builtin_amdgcn_readfirstlane(lds)), "v"(gsrc)
                 : "memory");
}
