// Source coordinate and weights of the bilinear x2 upsample (align_corners=True) of Up.forward (src/EGM-UNet.py:937-947): the ONE
// definition every kernel that interpolates uses (pool_up.hip, bn_stencil_fused.hip).
#pragma once
#include "common.h"

struct Lerp { int i0, i1; float w0, w1; };
// a product that is rounded on its own wherever the call is inlined: without the contract flag the compiler cannot fuse it into
// the operation that consumes it
__device__ __forceinline__ float egm_mul_rounded(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
// ROUNDED: scale*dst is rounded before i0 is subtracted (torch's own form).  The forward kernels (upcat_fwd_kernel and the fused
// bn_act_upcat_fwd_kernel, which must agree bit for bit) ask for it, so their weights are the same floats by definition and not by
// what the compiler makes of the code around each call: left alone it contracts the pair into fma(scale, dst, -i0) where the product
// has no other use, which moves the last bit of w1 for about one coordinate in three.  The backward gather keeps the default form
// it has always compiled with.
template <bool ROUNDED = false>
__device__ __forceinline__ Lerp lerp_coord(int dst, int in_size, int out_size) {
    // torch upsample_bilinear2d, align_corners=True: scale = (in-1)/(out-1) (0 when out == 1), all in fp32
    const float scale = out_size > 1 ? (float)(in_size - 1) / (float)(out_size - 1) : 0.f;
    const float src = ROUNDED ? egm_mul_rounded(scale, (float)dst) : scale * (float)dst;
    Lerp l;
    l.i0 = (int)src;
    l.i1 = l.i0 + (l.i0 < in_size - 1 ? 1 : 0);
    l.w1 = src - (float)l.i0;
    l.w0 = 1.f - l.w1;
    return l;
}
