// Device helpers shared by the LDS-DMA kernels (conv3x3_tile.hip, conv3x3_wreg.hip, gemm_dma.hip).
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(2))) float egm_f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 egm_bf16x2;

// two fp32 -> one dword of two bf16 (round to nearest even): ONE v_cvt_pk_bf16_f32 (the scalar casts were paired crosswise by the
// vectoriser and re-shuffled with and / shift / or: 6 instructions per 4 values instead of 2)
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    egm_f32x2 v; v.x = lo; v.y = hi;
    const egm_bf16x2 b = __builtin_convertvector(v, egm_bf16x2);
    return *reinterpret_cast<const uint32_t*>(&b);
}

// global -> LDS, 16 bytes per lane (global_load_lds_dwordx4): M0 = wave-uniform LDS base; lane l lands at base + 16 l.
// The DMA is issued from inline asm on purpose: through the builtin the compiler treats it as an LDS store that may alias the
// fragment reads and drains it (s_waitcnt vmcnt(0)) in front of the first ds_read, which serialises copy and MFMA.  Ordering is the
// caller's instead: a counted s_waitcnt vmcnt and a barrier before anybody reads the image just filled.
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_byte_addr) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_byte_addr));
}
