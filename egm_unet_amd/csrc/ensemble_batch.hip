// The UNet end of batched ensemble inference: B decoded uint8 photos of one size [B][H][W][3] -> transforms.Resize(base_size) of the
// PIL image (Pillow BILINEAR with antialias, two separable passes on bytes) -> ToTensor -> Normalize, fp32 [B][3][oh][ow].
// The batched form of egm_resample_u8 (axis 1, then axis 0) followed by egm_augment_u8 without flips and with a full crop; per output
// element the expressions are theirs (csrc/data.hip), so image b of the result equals the per-image chain bit for bit.
//   horizontal  rows are independent, so the pass runs over the B * H rows of the batch: uint8 [B*H][ow][3], one thread per pixel
//   vertical    one thread per output pixel and image: the bytes of the second pass are normalised in registers and written as
//               planar fp32, which saves the second uint8 tensor and the augment launch
// A pass whose table is NULL is the identity (ow == W or oh == H) and is skipped: at most two launches, whatever B.
// Streaming kernels without reuse beyond the 3..7 taps, which L1/L2 serve; the byte rows of a [.][ow][3] tensor start at any
// alignment (ow * 3 is odd for odd ow), so loads are per byte and lanes are adjacent pixels (a wave reads 192 contiguous bytes per
// tap); the fp32 planes are written 256 contiguous bytes per wave.
#include "common.h"

namespace {

constexpr int kPrecisionBits = 32 - 8 - 2;      // Pillow Resample.c, as in data.hip

__device__ __forceinline__ int clip8(int v) {
    v >>= kPrecisionBits;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// out[r][xo][c] = clip8(2^21 + sum_j src[r][x0 + j][c] * coefs[xo][j]) for the rows r of the whole batch
__global__ __launch_bounds__(256) void unet_hresample_rows_kernel(const unsigned char* __restrict__ src, long long rows, int W,
                                                                  unsigned char* __restrict__ dst, int OW, const int* __restrict__ bounds,
                                                                  const int* __restrict__ coefs, int ksize) {
    const long long total = rows * OW;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int xo = (int)(i % OW);
        const long long r = i / OW;
        int x0 = bounds[xo * 2], n = bounds[xo * 2 + 1];
        x0 = x0 < 0 ? 0 : (x0 > W - 1 ? W - 1 : x0);                             // no table can make the kernel leave the row
        n = n < 0 ? 0 : min(n, min(ksize, W - x0));
        const unsigned char* p = src + (r * W + x0) * 3;
        const int* k = coefs + (long long)xo * ksize;
        int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
        for (int j = 0; j < n; ++j) {
            const int c = k[j];
            a0 += (int)p[j * 3] * c; a1 += (int)p[j * 3 + 1] * c; a2 += (int)p[j * 3 + 2] * c;
        }
        unsigned char* q = dst + i * 3;
        q[0] = (unsigned char)clip8(a0); q[1] = (unsigned char)clip8(a1); q[2] = (unsigned char)clip8(a2);
    }
}

// src uint8 [B][H][W][3] -> out fp32 [B][3][OH][W]: the vertical pass (bounds == nullptr: none, OH == H) and ToTensor / Normalize
__global__ __launch_bounds__(256) void unet_vresample_norm_kernel(const unsigned char* __restrict__ src, int B, int H, int W,
                                                                  float* __restrict__ out, int OH, const int* __restrict__ bounds,
                                                                  const int* __restrict__ coefs, int ksize, float m0, float m1, float m2,
                                                                  float s0, float s1, float s2) {
    const long long plane = (long long)OH * W, total = (long long)B * plane;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long b = i / plane, o = i - b * plane;
        const int x = (int)(o % W), yo = (int)(o / W);
        int p0, p1, p2;
        if (bounds != nullptr) {
            int y0 = bounds[yo * 2], n = bounds[yo * 2 + 1];
            y0 = y0 < 0 ? 0 : (y0 > H - 1 ? H - 1 : y0);
            n = n < 0 ? 0 : min(n, min(ksize, H - y0));
            const unsigned char* p = src + ((b * H + y0) * W + x) * 3;
            const int* k = coefs + (long long)yo * ksize;
            const long long pitch = (long long)W * 3;
            int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
            for (int j = 0; j < n; ++j) {
                const int c = k[j];
                const unsigned char* q = p + j * pitch;
                a0 += (int)q[0] * c; a1 += (int)q[1] * c; a2 += (int)q[2] * c;
            }
            p0 = clip8(a0); p1 = clip8(a1); p2 = clip8(a2);
        } else {
            const unsigned char* p = src + ((b * H + yo) * W + x) * 3;
            p0 = p[0]; p1 = p[1]; p2 = p[2];
        }
        float* d = out + b * 3 * plane + o;
        d[0] = ((float)p0 / 255.0f - m0) / s0;                                  // augment_kernel's expression
        d[plane] = ((float)p1 / 255.0f - m1) / s1;
        d[2 * plane] = ((float)p2 / 255.0f - m2) / s2;
    }
}

}  // namespace

extern "C" int egm_unet_preprocess_batch_u8(const void* imgs_bhwc3, int B, int H, int W, float* out_bchw, int oh, int ow, const int* xbounds,
                                            const int* xcoefs, int xksize, const int* ybounds, const int* ycoefs, int yksize,
                                            const float* mean3_host, const float* std3_host, void* tmp_bhwc3, egm_stream_t s) {
    EGM_REQUIRE(imgs_bhwc3 && out_bchw && mean3_host && std3_host, "unet_preprocess_batch_u8: null pointer");
    EGM_REQUIRE(B > 0 && H > 0 && W > 0 && oh > 0 && ow > 0, "unet_preprocess_batch_u8: bad shape");
    EGM_REQUIRE((xbounds != nullptr) == (xcoefs != nullptr) && (ybounds != nullptr) == (ycoefs != nullptr),
                "unet_preprocess_batch_u8: bounds and coefficients of a pass come together");
    EGM_REQUIRE(xbounds ? (xksize > 0 && tmp_bhwc3 != nullptr) : ow == W,
                "unet_preprocess_batch_u8: a horizontal pass needs its tables and tmp; without one ow must equal W");
    EGM_REQUIRE(ybounds ? yksize > 0 : oh == H, "unet_preprocess_batch_u8: a vertical pass needs its tables; without one oh must equal H");
    EGM_REQUIRE(std3_host[0] != 0.f && std3_host[1] != 0.f && std3_host[2] != 0.f, "unet_preprocess_batch_u8: zero std");
    const unsigned char* src = (const unsigned char*)imgs_bhwc3;
    if (xbounds) {
        const long long rows = (long long)B * H;
        hipLaunchKernelGGL(unet_hresample_rows_kernel, dim3(egm_stream_grid(rows * ow)), dim3(256), 0, (hipStream_t)s, src, rows, W,
                           (unsigned char*)tmp_bhwc3, ow, xbounds, xcoefs, xksize);
        EGM_CHECK_LAUNCH("unet_preprocess_batch_u8 (horizontal)");
        src = (const unsigned char*)tmp_bhwc3;
    }
    hipLaunchKernelGGL(unet_vresample_norm_kernel, dim3(egm_stream_grid((long long)B * oh * ow)), dim3(256), 0, (hipStream_t)s, src, B, H, ow, out_bchw,
                       oh, ybounds, ycoefs, yksize, mean3_host[0], mean3_host[1], mean3_host[2], std3_host[0], std3_host[1], std3_host[2]);
    EGM_CHECK_LAUNCH("unet_preprocess_batch_u8 (vertical)");
    return EGM_OK;
}
