// The fused logit of the CLIPSeg (+) UNet ensemble (predict_CLIPseg.py:501-525), shared by every kernel that evaluates it
// (ensemble_score.hip: egm_ensemble_fuse, egm_ensemble_alpha_hist; ensemble_pipe.hip: egm_ensemble_mask_u8), so that all of them produce the
// same bits: fused = bilinear(clip_logits -> HxW, align_corners=False) + alpha * unet_logits, argmax with ties to the lowest class.
#pragma once
#include "common.h"

__device__ __forceinline__ void bilin_src(int dst, int in_size, int out_size, int& i0, int& i1, float& w1) {
    const float scale = (float)in_size / (float)out_size;
    float src = ((float)dst + 0.5f) * scale - 0.5f;            // torch area_pixel_compute_source_index, align_corners=False
    if (src < 0.f) src = 0.f;
    i0 = (int)src; if (i0 > in_size - 1) i0 = in_size - 1;
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    w1 = src - (float)i0;
}
__device__ __forceinline__ float bilin_at(const float* __restrict__ m, int wc, int y0, int y1, float wy, int x0, int x1, float wx) {
    const float a = m[(long long)y0 * wc + x0], b = m[(long long)y0 * wc + x1], c = m[(long long)y1 * wc + x0], d = m[(long long)y1 * wc + x1];
    return (1.f - wy) * ((1.f - wx) * a + wx * b) + wy * ((1.f - wx) * c + wx * d);
}
// argmax_c (up(clip)[n][c] + alpha * unet[n][c]) at UNet pixel (y, x) of image n; fused (optional, [N][C][H][W]) receives the logits
__device__ __forceinline__ int ensemble_fused_argmax(const float* __restrict__ clip, const float* __restrict__ unet, float alpha, int n, int C,
                                                     int hc, int wc, int H, int W, int y, int x, float* __restrict__ fused) {
    const long long HW = (long long)H * W, pix = (long long)y * W + x;
    int y0, y1, x0, x1; float wy, wx;
    bilin_src(y, hc, H, y0, y1, wy); bilin_src(x, wc, W, x0, x1, wx);
    int best = 0; float m = -INFINITY;
    for (int c = 0; c < C; ++c) {
        const float v = bilin_at(clip + ((long long)n * C + c) * hc * wc, wc, y0, y1, wy, x0, x1, wx) + alpha * unet[((long long)n * C + c) * HW + pix];
        if (fused) fused[((long long)n * C + c) * HW + pix] = v;
        if (v > m) { m = v; best = c; }
    }
    return best;
}
