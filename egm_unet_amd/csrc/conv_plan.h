// The convolution kernel families as conv_igemm.hip's conv_plan() / conv_fwd_impl() and conv_wgrad.hip's wgrad_plan() /
// egm_conv_wgrad() see them: per family a *_plan that says whether it takes a shape (and with what decomposition), a *_launch, and
// where egm_conv_kernel_name needs it a *_name.  Every conv .hip includes this header, the defining files too, so a signature
// cannot drift from its users.
#pragma once
#include "common.h"

// conv_direct.hip: 1x1 / dilated convolutions without an LDS activation tile.  Plan: 0 = not taken; else NT, nct, G (= statistics
// tiles) and the dynamic LDS size describe the launch.
int egm_conv_direct_plan(int dtype, int N, int H, int W, int Cin, int Cout, int KH, int KW, int dil, int* NT_out, int* nct_out, int* G_out,
                         size_t* smem_out);
int egm_conv_direct_launch(const void* x, int ldx, const void* wf, const float* bias, int bias_n, void* y, int ldy, float* stats, int N, int H,
                           int W, int Cin, int Cout, int KH, int KW, int dil, int NT, int nct, int G, size_t smem, egm_stream_t s,
                           int act = EGM_ACT_NONE);

// conv3x3_tile.hip: 8-wave LDS-DMA 3x3 kernel (the throughput path of the 3x3 stacks).  Plan: 0 = not taken; else the tile
// configuration, the cout tiles and G = pixel groups = statistics rows.  y2 != nullptr: split output (egm_conv_fwd_split).
int egm_conv_tile_plan(int dtype, int N, int H, int W, int Cin, int Cout, int KH, int KW, int dil, int* cfg_out, int* nct_out, int* G_out);
const char* egm_conv_tile_name(int cfg);
int egm_conv_tile_launch(const void* x, int ldx, const void* wf, const float* bias, int bias_n, void* y, int ldy, float* stats, int N, int H,
                         int W, int Cin, int Cout, int cfg, int nct, int G, egm_stream_t s, void* y2 = nullptr, int ldy2 = 0, int csplit = 0,
                         int act = EGM_ACT_NONE);

// conv3x3_wreg.hip: weights-in-registers 3x3 kernel for the 32 -> 32 layers.  Plan: 1 when taken (then *G_out = statistics rows).
int egm_conv_wreg_plan(int dtype, int N, int H, int W, int Cin, int Cout, int KH, int KW, int dil, int* G_out);
const char* egm_conv_wreg_name(int Cin);
int egm_conv_wreg_launch(const void* x, int ldx, const void* wf, const float* bias, int bias_n, void* y, int ldy, float* stats, int N, int H,
                         int W, int Cin, int Cout, int G, egm_stream_t s, int act = EGM_ACT_NONE);

// conv7x7_c16.hip: weights-in-registers kernels for 16 -> 16 channels: the 7x7 conv (FusionConv's merged multi-scale conv at the
// 64-channel level; no statistics epilogue) and the dilated 3x3 conv (plan = statistics rows, 0 = not taken), and their weight
// gradients (plan = workgroups = slabs, 0 = not taken).
int egm_conv_c7_plan(int dtype, int N, int H, int W, int Cin, int Cout, int KH, int KW, int dil);
int egm_conv_c7_launch(const void* x, int ldx, const void* wf, const float* bias, int bias_n, void* y, int ldy, int N, int H, int W,
                       egm_stream_t s, int act = EGM_ACT_NONE);
int egm_conv_c16d_plan(int dtype, int N, int H, int W, int Cin, int Cout, int KH, int KW, int dil);
int egm_conv_c16d_launch(const void* x, int ldx, const void* wf, const float* bias, int bias_n, void* y, int ldy, float* stats, int N, int H,
                         int W, int dil, egm_stream_t s, int act = EGM_ACT_NONE);
int egm_conv_c7_wgrad_plan(int dtype, int N, int H, int W, int Cin, int Cout, int KH, int KW, int dil);
int egm_conv_c7_wgrad_launch(const void* x, int ldx, const void* dy, int lddy, float* slab, int nslab, int N, int H, int W, egm_stream_t s);
int egm_conv_c16d_wgrad_plan(int dtype, int N, int H, int W, int Cin, int Cout, int KH, int KW, int dil);
int egm_conv_c16d_wgrad_launch(const void* x, int ldx, const void* dy, int lddy, float* slab, int nslab, int N, int H, int W, int dil,
                               egm_stream_t s);
