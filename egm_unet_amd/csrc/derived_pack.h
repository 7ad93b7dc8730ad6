// The derived FusionConv weights, one packed element at a time: the one copy of the fold2 / merge357 expressions, shared by the
// stand-alone launches (fold2_pack_kernel / merge357_pack_kernel, blocks.hip) and the model-wide prepack (conv_pack_multi_kernel,
// conv_igemm.hip).  i indexes the packed forward image [tap][CoutP][CinP]; layouts as egm_conv_pack's for a 1x1 / 7x7 weight (never
// chunk-major: that is for 3x3 only): wf [tap][CoutP][CinP], wd [tap flipped][CinP][CoutP], zeros in the padding.
#pragma once
#include "common.h"

// down conv on cat([x, x]): W[:, :K] + W[:, K:] of the real [rows][2K] weight -> out fp32 [rows][K] and its packs
template <typename T>
__device__ __forceinline__ void fold2_pack_elem(int i, const float* __restrict__ w, float* __restrict__ out, T* __restrict__ wf,
                                                T* __restrict__ wd, int rows, int K, int CoutP, int CinP) {
    const int co = i / CinP, ci = i - co * CinP;
    float v = 0.f;
    if (co < rows && ci < K) {
        v = w[(long long)co * 2 * K + ci] + w[(long long)co * 2 * K + K + ci];
        out[co * K + ci] = v;
    }
    wf[i] = from_f32<T>(v);
    wd[(long long)ci * CoutP + co] = from_f32<T>(v);
}

// conv3 + conv5 + conv7 of one input: the 7x7 weight with the zero-padded kernels summed -> w fp32 [Co][Ci][7][7], its packs, and
// (elements i < Co) the summed bias b
template <typename T>
__device__ __forceinline__ void merge357_pack_elem(int i, const float* __restrict__ w3, const float* __restrict__ w5,
                                                   const float* __restrict__ w7, const float* __restrict__ b3,
                                                   const float* __restrict__ b5, const float* __restrict__ b7, float* __restrict__ w,
                                                   float* __restrict__ b, T* __restrict__ wf, T* __restrict__ wd, int Co, int Ci, int CoutP,
                                                   int CinP) {
    const int ci = i % CinP, co = (i / CinP) % CoutP, t = i / (CinP * CoutP), r = t / 7, sx = t % 7;
    float v = 0.f;
    if (co < Co && ci < Ci) {
        const int oc = co * Ci + ci;
        v = w7[oc * 49 + t];
        if (r >= 1 && r <= 5 && sx >= 1 && sx <= 5) v += w5[oc * 25 + (r - 1) * 5 + (sx - 1)];
        if (r >= 2 && r <= 4 && sx >= 2 && sx <= 4) v += w3[oc * 9 + (r - 2) * 3 + (sx - 2)];
        w[oc * 49 + t] = v;
    }
    wf[i] = from_f32<T>(v);
    wd[((long long)(48 - t) * CinP + ci) * CoutP + co] = from_f32<T>(v);
    if (i < Co) b[i] = b3[i] + b5[i] + b7[i];
}
