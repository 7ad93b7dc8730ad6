// 3x3 convolution (stride 1, dilation 1, 'same' padding) for NHWC bf16 activations on CDNA4: the wide-tile LDS-DMA kernel.
//
//   y[n,oy,ox,co] = bias[co] + sum_{r,s,ci} x[n, oy+r-1, ox+s-1, ci] * w[r*3+s][co][ci]
//
// The 3x3 convs of the U-Net stacks (src/EGM-UNet.py:49,52,893,899: DoubleConv / DoubleConv1; src/unet.py:12,15) forward and, with
// the flipped pack `wd`, their data gradients.  Round 3's replacement for the 4-wave register-staged kernel
// (conv_igemm_pipe_kernel<*,3,3,*>) on every layer that fills the chip with the larger tile.
//
// Structure (one workgroup = 8 waves = WR x WC, one workgroup per CU, 2 waves per SIMD, <= 256 VGPRs):
//   * tile = (WR*R) rows x 32 pixels x (WC*NT*32) couts; wave (wr, wc) owns R rows x NT cout blocks = R*NT accumulator tiles of
//     v_mfma_f32_32x32x16_bf16 (A = weights: rows = couts, B = patch: columns = pixels, so a lane ends with 4 consecutive couts of one
//     pixel per register quad).
//   * K loop = 16-channel chunks.  A stage = the (rows+2) x 34 halo patch of the chunk + the 9 x NC weight rows of the chunk.  Both go
//     global -> LDS by LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave-instruction, no staging registers, no LDS write pass): every
//     wave issues KT of the stage's instructions.  The weight image is read from the chunk-major operand pack
//     [tap][Cin/16][Cout][16] (egm_conv_pack, common.h WLayout), so a weight instruction reads 1 KiB of contiguous memory; a patch
//     instruction reads 32 pixels x 32 B.
//   * the LDS image is 16-byte slots in DMA order (slot = wave-uniform base + lane): WHICH (pixel, channel half) a slot holds is
//     chosen by the lane's source address, so the bank swizzle costs nothing: slot(pixel p of a row, half h) = 2p + (h ^ (p>>3 & 1))
//     makes every ds_read_b128 fragment read (32 consecutive pixels or couts, one half) conflict-free for all three column shifts.
//   * NBUF stage buffers, ONE barrier per stage: iteration t issues stage t+NBUF-1, multiplies stage t, then waits
//     (s_waitcnt vmcnt, counted when NBUF = 3) and passes a raw s_barrier.  A stage is 9*R*NT MFMAs per wave (72 for R*NT = 8).
//   * lanes whose pixel lies outside the image read a 64-byte zero page instead (zero padding of the conv), so every wave issues
//     the same number of DMA instructions per stage whatever the tile: the vmcnt counts are compile-time constants.
//   * persistent over pixel tiles (stage list = (tile, chunk) pairs, the next tile's first stages stream in during the epilogue);
//     epilogue of tile i runs after the barrier, behind the DMA issue of the next stage: accumulators -> bf16 -> wave-private LDS
//     tile -> whole 16-byte channel vectors -> coalesced stores (+bias), BatchNorm partial sums in registers over all tiles.
//   * XCD-aware block -> (pixel group, cout tile) map as in conv_igemm.hip.
#include "common.h"
#include "conv_plan.h"
#include "lds_dma.h"
#include "group.h"
#include "bn_elem.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;

__device__ uint4 egm_zero_page[4];          // zero-initialised: the source of every DMA lane that must deliver zeros

#ifndef EGM_TILE_DMA_EVERY
#define EGM_TILE_DMA_EVERY 1      // one LDS-DMA instruction after every n-th fragment group of the MFMA phase
#endif

namespace {

constexpr int TW = 32, PW = TW + 2, KC = 16;

struct TileParams {
    const bf16_t* x; const bf16_t* w; const float* bias; bf16_t* y; float* stats;
    bf16_t* y2; int ldy2, csplit;    // split output: couts >= csplit go to y2[..., c - csplit] (pixel stride ldy2); csplit = 0: one output
    int ldx, ldy, N, H, W, Cin, Cout, bias_n;
    int tiles_y, tiles_x, npt, nct, G;
    int dbg;        // ablation switches for tools/conv_tile_diag.py (0 in production): 1 = no DMA, 2 = no MFMA phase, 4 = no epilogue, 8 = no static priority
};

template <int R, int NT, int WR, int WC, int NBUF> struct TileGeom {
    static constexpr int TROWS = WR * R, PH = TROWS + 2, NC = WC * NT * 32;
    static constexpr int PSLOTS = PH * PW * 2, WSLOTS = 9 * NC * 2;          // 16-byte slots
    static constexpr int NPI = (PSLOTS + 63) / 64, NWI = WSLOTS / 64;       // DMA instructions (64 slots each)
    static constexpr int KT = (NPI + NWI + 7) / 8;                          // per wave and stage (the last few may be padding)
    static constexpr int STAGE_BYTES = KT * 8 * 1024;
    static constexpr int WOFF = NPI * 1024;                                 // weight image behind the patch image
    static constexpr int OROW = NT * 64 + 16;                               // out-tile row: NT*32 couts bf16 + pad
    static constexpr int OUT_BYTES = 8 * 32 * OROW;
    static constexpr int SMEM = NBUF * STAGE_BYTES + OUT_BYTES;
    static_assert(WSLOTS % 64 == 0, "weight image must be whole DMA instructions");
    static_assert(SMEM <= 160 * 1024, "LDS budget");
    static_assert(9 * NC * 32 + 64 * 32 < 65536, "ds_read immediate offsets");
};

template <int R, int NT, int WR, int WC, int NBUF>
__global__ __launch_bounds__(512, 2) void conv3x3_tile_kernel(TileParams p) {
    constexpr int ACT = EGM_ACT_NONE;
#include "conv3x3_tile_body.h"
}
// the same with an activation in the epilogue (egm_conv_fwd_act)
template <int R, int NT, int WR, int WC, int NBUF, int ACT>
__global__ __launch_bounds__(512, 2) void conv3x3_tile_act_kernel(TileParams p) {
#include "conv3x3_tile_body.h"
}

template <int R, int NT, int WR, int WC, int NBUF, int ACT = EGM_ACT_NONE>
int launch_tile(const TileParams& p, hipStream_t st) {
    using Gm = TileGeom<R, NT, WR, WC, NBUF>;
    constexpr auto kern = [] {
        if constexpr (ACT == EGM_ACT_NONE) return &conv3x3_tile_kernel<R, NT, WR, WC, NBUF>;
        else return &conv3x3_tile_act_kernel<R, NT, WR, WC, NBUF, ACT>;
    }();
    if (int rc = egm_allow_max_lds<kern>("conv3x3_tile")) return rc;
    const int grid = ((p.G + 7) / 8) * 8 * p.nct;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), Gm::SMEM, st, p);
    EGM_CHECK_LAUNCH("conv3x3_tile");
    return EGM_OK;
}

// tile shapes: {rows per wave, cout blocks per wave, wave rows, wave columns}
struct TileCfg { int id, rows, nc; };
constexpr TileCfg kCfgs[] = {
    {0, 16, 128},   // A: R4 NT2 WR4 WC2
    {1, 8, 128},    // B: R2 NT2 WR4 WC2
    {2, 32, 64},    // D: R4 NT2 WR8 WC1
    {3, 16, 64},    // E: R2 NT2 WR8 WC1
    {4, 32, 32},    // F: R4 NT1 WR8 WC1
    {5, 16, 32},    // G: R2 NT1 WR8 WC1
};
}  // namespace

// bits: 1 = 8-wave tile kernel (>= 64-cout tiles), 2 = also its 32-cout tiles (measured slower: tests / A-B runs only), 4 = weights-in-
// registers kernel for the 32 -> 32 layers (conv3x3_wreg.hip).  -1: not read yet (env EGM_CONV_TILE, default 5); 0 = 4-wave kernel only
static int g_tile_mode = -1;
extern "C" int egm_conv_tile_mode(int mode) {
    if (g_tile_mode < 0) g_tile_mode = egm_env_int("EGM_CONV_TILE", 5);
    const int old = g_tile_mode;
    if (mode >= 0) g_tile_mode = mode;
    return old;
}

static int g_tile_dbg = 0;
/* ablation switches of the tile kernel (diagnostics only; results are wrong while set): 1 = no DMA, 2 = no MFMA phase, 4 = no epilogue */
extern "C" int egm_conv_tile_debug(int dbg) { const int old = g_tile_dbg; if (dbg >= 0) g_tile_dbg = dbg; return old; }

// Plan: returns 0 when the shape does not take this kernel, else 1 with the tile configuration, grid decomposition and the number of
// BatchNorm statistics rows (= pixel groups).
int egm_conv_tile_plan(int dtype, int N, int H, int W, int Cin, int Cout, int KH, int KW, int dil, int* cfg_out, int* nct_out, int* G_out) {
    if (dtype != EGM_BF16 || KH != 3 || KW != 3 || dil != 1) return 0;
    if (!egm_w_chunk16(dtype, KH, KW, Cin, Cout)) return 0;
    if (Cout % 32 != 0) return 0;
    if (egm_group_recording()) return 0;                     // merged launches of small sibling convs stay on the 4-wave kernel
    if (!(egm_conv_tile_mode(-1) & 1)) return 0;
    if (Cin < 16) return 0;              // (r04: 32-channel inputs on the 4-wave kernel instead, i.e. 64 here: step 12.07 -> 12.11 ms, not kept)
    const int tx = egm_cdiv(W, TW);
    int best = -1, best_nct = 0, best_npt = 0;
    long long best_score = -1;
    for (const TileCfg& c : kCfgs) {
        if (Cout % c.nc != 0) continue;
        // 32-cout tiles (the HBM-bound 32-cout layers at 512^2 / 256^2, and 128-cout layers cut four ways): measured 3-25 % slower
        // than the 4-wave kernel's tall tiles (two resident workgroups keep more bytes in flight than one stage ahead of one
        // workgroup): only offered under mode bit 2 (tools/conv_tile_bench.py)
        if (c.nc == 32 && !(egm_conv_tile_mode(-1) & 2)) continue;
        const int nct = Cout / c.nc;
        const int npt = N * egm_cdiv(H, c.rows) * tx;
        const long long wgs = (long long)npt * nct;
        if (wgs < 192) continue;                             // one workgroup per CU: fewer than ~3/4 of the chip is not worth it
        // prefer the configuration with the most work per workgroup that still fills the chip in whole rounds
        const long long rounds = (wgs + 255) / 256;
        const long long eff = wgs * 1000 / (rounds * 256);    // fill of the last round, per mille
        const long long score = eff * 4 + (long long)c.rows * c.nc / 128;   // fill first, then tile size
        if (score > best_score) { best_score = score; best = c.id; best_nct = nct; best_npt = npt; }
    }
    if (best < 0) return 0;
    int g = (256 / best_nct) / 8 * 8;
    if (g < 8) g = 8;
    if (g > best_npt) g = best_npt;
    *cfg_out = best; *nct_out = best_nct; *G_out = g;
    return 1;
}

const char* egm_conv_tile_name(int cfg) {
    switch (cfg) {
        case 0: return "conv3x3_tile_kernel<4, 2, 4, 2, 2>";
        case 1: return "conv3x3_tile_kernel<2, 2, 4, 2, 2>";
        case 2: return "conv3x3_tile_kernel<4, 2, 8, 1, 2>";
        case 3: return "conv3x3_tile_kernel<2, 2, 8, 1, 2>";
        case 4: return "conv3x3_tile_kernel<4, 1, 8, 1, 2>";
        default: return "conv3x3_tile_kernel<2, 1, 8, 1, 2>";
    }
}

int egm_conv_tile_launch(const void* x, int ldx, const void* wf, const float* bias, int bias_n, void* y, int ldy, float* stats, int N, int H,
                         int W, int Cin, int Cout, int cfg, int nct, int G, egm_stream_t s, void* y2, int ldy2, int csplit, int act) {
    TileParams p;
    p.x = (const bf16_t*)x; p.w = (const bf16_t*)wf; p.bias = bias; p.y = (bf16_t*)y; p.stats = stats;
    p.y2 = (bf16_t*)y2; p.ldy2 = ldy2; p.csplit = y2 ? csplit : 0;
    p.ldx = ldx; p.ldy = ldy; p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.bias_n = bias ? bias_n : 0;
    p.dbg = g_tile_dbg;
    const int rows = kCfgs[cfg].rows;
    p.tiles_y = egm_cdiv(H, rows); p.tiles_x = egm_cdiv(W, TW); p.npt = N * p.tiles_y * p.tiles_x; p.nct = nct; p.G = G;
    EGM_REQUIRE((long long)(rows + 2) * W * ldx < (1LL << 31), "conv3x3_tile: halo window offsets exceed 32 bits");
    hipStream_t st = (hipStream_t)s;
    // every configuration has an instantiation per activation: egm_conv_fwd_act takes the plan of egm_conv_fwd under every tile mode,
    // the 32-cout configurations of mode bit 2 included (test_gpu_conv_epilogue.py runs them)
    auto any = [&](auto a) {
        constexpr int ACT = decltype(a)::value;
        switch (cfg) {
            case 0: return launch_tile<4, 2, 4, 2, 2, ACT>(p, st);
            case 1: return launch_tile<2, 2, 4, 2, 2, ACT>(p, st);
            case 2: return launch_tile<4, 2, 8, 1, 2, ACT>(p, st);
            case 3: return launch_tile<2, 2, 8, 1, 2, ACT>(p, st);
            case 4: return launch_tile<4, 1, 8, 1, 2, ACT>(p, st);
            default: return launch_tile<2, 1, 8, 1, 2, ACT>(p, st);
        }
    };
    if (act != EGM_ACT_NONE) {
        EGM_REQUIRE(y2 == nullptr, "conv3x3_tile: no activation with a split output");
        EGM_REQUIRE(act >= EGM_ACT_RELU && act <= EGM_ACT_SILU, "conv3x3_tile: unknown activation %d", act);
        return egm_with_act(act, any);
    }
    return any(std::integral_constant<int, EGM_ACT_NONE>());
}
