// 3x3 convolution (stride 1, dilation 1) for the NARROW layers -- Cout = 32, Cin = 32 or 64 -- at 512^2 / 256^2: weights in registers.
//
//   y[n,oy,ox,co] = bias[co] + sum_{r,s,ci} x[n, oy+r-1, ox+s-1, ci] * w[r*3+s][co][ci]
//
// in_conv.3, up4.conv.3, up4.conv.0, up3.conv.3 of the U-Net stacks (src/EGM-UNet.py:49,52,893,899) and the data gradients of
// in_conv.3 / down1.1.0 / up4.conv.3: 38-77 GFLOP over 270-400 MB per launch, i.e. MFMA time ~ memory time ~ 20-25 us.  Neither
// conv_igemm_pipe_kernel<1,3,3,4> (62-130 us) nor the 32-cout tiles of conv3x3_tile.hip (70-150 us) overlaps the two: both re-stage the
// weights per stage and run the epilogue (half the instructions of such a tile) with the matrix pipe idle.
//
// This kernel:
//   * ONE workgroup of 8 waves per CU, persistent over 16-row x 32-pixel tiles; wave w owns rows 2w, 2w+1 x all 32 couts
//     (2 accumulator tiles of v_mfma_f32_32x32x16_bf16; A = weights: rows = couts, B = patch: columns = pixels).
//   * the WHOLE weight set of the wave's 32 couts lives in registers for the whole kernel: 9 taps x (Cin/16) k-steps fragments
//     (72 VGPRs for Cin = 32, 144 for Cin = 64), loaded once from the chunk-major pack.  The MFMA phase reads only patch-row fragments
//     from LDS: 24 ds_read_b128 per 36 MFMAs, no weight traffic at all.
//   * a stage = the 18 x 34 halo patch of 32 channels (39 KB, whole 64-byte segments per pixel), global -> LDS by LDS-DMA, THREE
//     buffers: two stages (78 KB) in flight per CU behind a counted s_waitcnt vmcnt, one raw s_barrier per stage.  LDS slot of
//     (pixel p of a row, 16-byte channel group g) = 4p + (g ^ (p>>2 & 3)): conflict-free ds_read_b128 for all three column shifts.
//   * TWO accumulator sets, and the two wave groups run the iteration in opposite order: waves 0-3 store tile t-1 (epilogue: VALU,
//     LDS, stores) and then multiply tile t; waves 4-7 multiply tile t first and store tile t-1 afterwards.  Each SIMD hosts one wave
//     of either group, so the epilogue of one always sits beside the MFMA phase of the other ("two accumulator sets so
//     tile i's epilogue overlaps tile i+1's first stages").
//   * zero page for out-of-image lanes, XCD-aware block map, epilogue and BatchNorm partial sums as in conv3x3_tile.hip.
#include "common.h"
#include "conv_plan.h"
#include "lds_dma.h"
#include "group.h"
#include "bn_elem.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;

__device__ uint4 egm_dump_wreg[64];                   // where the stores of lanes outside the image go (never read)
__device__ uint4 egm_zero_page_wreg[4];               // zero-initialised: source of DMA lanes outside the image (device symbols are per code object)

namespace {

constexpr int TW = 32, PW = TW + 2, R = 2, TROWS = 16, PH = TROWS + 2, NBUF = 3;
constexpr int PSLOTS = PH * PW * 4;                   // 16-byte slots of one stage (32 channels = 4 slots per pixel)
constexpr int NPI = (PSLOTS + 63) / 64;               // 39 DMA instructions
constexpr int KT = (NPI + 7) / 8;                     // 5 per wave (the 40th is padding)
constexpr int STAGE = KT * 8 * 1024;                  // 40 KB
constexpr int OROW = 64 + 16;                         // out-tile row: 32 couts bf16 + pad
constexpr int SMEM = NBUF * STAGE + 8 * R * 32 * OROW; // 120 KB + 40 KB: a wave's two output rows cross the LDS together
static_assert(SMEM <= 160 * 1024, "LDS budget");
static_assert(KT <= 6, "DMA slots of a stage");

struct WregParams {
    const bf16_t* x; const bf16_t* w; const float* bias; bf16_t* y; float* stats;
    int ldx, ldy, N, H, W, Cin, Cout, bias_n;
    int tiles_y, tiles_x, npt, G;
};

template <int CH>         // CH = Cin / 32 (only 1 is offered: Cin = 64 needs 144 weight registers)
__global__ __launch_bounds__(512, 2) void conv3x3_wreg_kernel(WregParams p) {
    constexpr int ACT = EGM_ACT_NONE;
#include "conv3x3_wreg_body.h"
}
// the same with an activation in the epilogue (egm_conv_fwd_act)
template <int CH, int ACT>
__global__ __launch_bounds__(512, 2) void conv3x3_wreg_act_kernel(WregParams p) {
#include "conv3x3_wreg_body.h"
}

template <int CH, int ACT = EGM_ACT_NONE>
int launch_wreg(const WregParams& p, hipStream_t st) {
    constexpr auto kern = [] { if constexpr (ACT == EGM_ACT_NONE) return &conv3x3_wreg_kernel<CH>; else return &conv3x3_wreg_act_kernel<CH, ACT>; }();
    if (int rc = egm_allow_max_lds<kern>("conv3x3_wreg")) return rc;
    hipLaunchKernelGGL(kern, dim3(p.G), dim3(512), SMEM, st, p);
    EGM_CHECK_LAUNCH("conv3x3_wreg");
    return EGM_OK;
}
}  // namespace

// Plan: 1 when the shape takes this kernel (then *G_out = pixel groups = BatchNorm statistics rows)
int egm_conv_wreg_plan(int dtype, int N, int H, int W, int Cin, int Cout, int KH, int KW, int dil, int* G_out) {
    if (dtype != EGM_BF16 || KH != 3 || KW != 3 || dil != 1 || Cout != 32 || Cin != 32) return 0;      // (Cin = 64: 144 weight registers + two accumulator sets spill)
    if (egm_group_recording()) return 0;
    if (!(egm_conv_tile_mode(-1) & 4)) return 0;
    const long long npt = (long long)N * egm_cdiv(H, TROWS) * egm_cdiv(W, TW);
    if (npt < 512) return 0;                                  // at least two tiles per workgroup: the epilogue overlap needs a next tile
    *G_out = 256;
    return 1;
}
const char* egm_conv_wreg_name(int Cin) { (void)Cin; return "conv3x3_wreg_kernel<1>"; }

int egm_conv_wreg_launch(const void* x, int ldx, const void* wf, const float* bias, int bias_n, void* y, int ldy, float* stats, int N, int H,
                         int W, int Cin, int Cout, int G, egm_stream_t s, int act) {
    WregParams p;
    p.x = (const bf16_t*)x; p.w = (const bf16_t*)wf; p.bias = bias; p.y = (bf16_t*)y; p.stats = stats;
    p.ldx = ldx; p.ldy = ldy; p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.bias_n = bias ? bias_n : 0;
    p.tiles_y = egm_cdiv(H, TROWS); p.tiles_x = egm_cdiv(W, TW); p.npt = N * p.tiles_y * p.tiles_x; p.G = G;
    EGM_REQUIRE((long long)(PH + 1) * W * ldx < (1LL << 31), "conv3x3_wreg: halo window offsets exceed 32 bits");
    return egm_with_act(act, [&](auto a) { return launch_wreg<1, decltype(a)::value>(p, (hipStream_t)s); });
}
