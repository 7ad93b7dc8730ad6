// Internal interface of csrc/gemm_dma.hip (the 8-wave LDS-DMA bf16 GEMM behind egm_gemm, csrc/vit.hip).
#pragma once
#include "common.h"

struct GemmDmaArgs {
    const void* A; const void* B; void* C; const float* bias; const void* R;      // bf16 A [M][K], B [N][K], C [M][N], R [M][N]; fp32 bias [N]
    int lda, ldb, ldc, ldr, M, N, K, act;
    float alpha;
};
// The form of the LDS-DMA kernel a product takes: nt = 32-column blocks per wave (tile 256 x 64 nt; 0: not taken -- shape, alignment, too
// few tiles to fill the chip, EGM_GEMM_DMA = 0), nw = waves per workgroup (8, or 4 under egm_gemm_dma_mode 2).  The ONE decision: the
// launch and the planner query (egm_gemm_kernel_name, csrc/vit.hip) both read it.
struct GemmDmaPlan { int nt, nw; };
GemmDmaPlan egm_gemm_dma_plan(const GemmDmaArgs& a);
inline int egm_gemm_dma_ok(const GemmDmaArgs& a) { return egm_gemm_dma_plan(a).nt != 0; }
int egm_gemm_dma_launch(const GemmDmaArgs& a, hipStream_t st);
