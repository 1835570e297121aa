// What the kernels that stage operands global -> LDS directly share (gemm_nt.hip, gemm_tn.hip; joint_fused.hip takes the
// hand-off alone): the DMA request, the LDS-only hand-off between waves and the developer builds' knock-outs of the bf16
// split and the MFMA.  (The zero chunk a dead lane fetches from stays one per unit: a __device__ variable shared between
// units needs relocatable device code.)
#pragma once
#include "common.h"

typedef __attribute__((address_space(3))) void* lptr_t;

// 64 lanes x 16 B from per-lane global addresses to LDS [lds_addr + 16 * lane].  In-order with every
// other vector-memory operation of the wave (vmcnt), so compiler-placed waits stay correct (at worst
// they wait for this too); the data is visible after s_waitcnt vmcnt(0) + a workgroup barrier.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void dma16(const float* gsrc, unsigned lds_addr) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gsrc), "s"(lds_addr) : "memory", "m0");
}
#pragma clang diagnostic pop

// LDS-only hand-off between waves: no global-memory fence (a __syncthreads() would also wait for
// this wave's outstanding C stores and for the next stage's DMA)
__device__ __forceinline__ void lds_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// developer builds (scripts/dev/nt_decompose.sh; WRONG results, right instruction mix): -DPC_EXP_NO_SPLIT (and
// -DPC_EXP_NO_LDSREAD) fragments used unsplit, -DPC_EXP_NO_MFMA products replaced by a register keep-alive
#if defined(PC_EXP_NO_SPLIT) || defined(PC_EXP_NO_LDSREAD)
#define PC_SPLIT(LO, HI) Split3{__builtin_bit_cast(bf16x8, LO), __builtin_bit_cast(bf16x8, HI), __builtin_bit_cast(bf16x8, LO)}
#else
#define PC_SPLIT(LO, HI) split3(LO, HI)
#endif
#if defined(PC_EXP_NO_MFMA)
#define PC_MFMA(A, B, C) ([&]() { asm volatile("" ::"v"(A), "v"(B)); return C; }())
#else
#define PC_MFMA(A, B, C) mfma_bf16(A, B, C)
#endif
