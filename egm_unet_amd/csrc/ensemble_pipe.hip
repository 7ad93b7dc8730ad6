// The two ends of the per-image ensemble pipeline (predict_CLIPseg.py:447-451 and :525-534) around the models:
//   egm_clip_preprocess_u8: decoded uint8 photo [H][W][3] -> ToTensor -> Normalize -> Resize((Sh, Sw)) of the float tensor, fp32 [3][Sh][Sw]
//   egm_ensemble_mask_u8:   fused-logit argmax at the UNet's size -> cv2.resize(INTER_NEAREST) to the photo's size -> colour map, uint8
//
// The preprocess is the pipeline's one pass over the full photo, so it is built as a streaming kernel.  The separable filter runs
// horizontally first (uint8 rows -> fp32 [3][H][Sw], the only kernel that touches the photo), then vertically over that intermediate,
// where the normalisation is applied (the weights sum to one, so filtering the raw bytes and normalising the result differs from the
// reference's order by rounding only).  Horizontal first whatever the aspect, because it is the pass whose reads are contiguous
// 16-byte loads of the uint8 rows; it is not always the fewest bytes: the fp32 intermediate is 12 * H * Sw bytes against 3 * H * W of
// the photo, 2.8x smaller at 4000 -> 352 columns (12.7 against 36 MB) but larger at 1024 -> 352 (3.2 against 2.4 MB).
// Horizontal pass: a workgroup owns 64 output columns (one per lane) and a band of rows; the 64 columns' weights are staged once in
// LDS as [tap][lane] (conflict-free); each wave then owns rows of its own: it stages the bytes of a row's input span with aligned
// 16-byte loads into its own LDS buffer and every lane runs its taps out of it, synchronised within the wave only.  Lane l starts at
// tap (l mod n) and wraps: with every lane on the same tap the 64 byte addresses are 3*scale bytes apart, which at an even scale lands
// them on a few banks; the rotation makes the stride 3*(scale+1).
#include "common.h"
#include "ensemble_fuse.h"

namespace {

constexpr int kClipMaxTaps = 64;          // ksize limit of both axes (antialiased scale up to 31.5)
constexpr int kClipRows = 16;             // rows per workgroup of the horizontal pass (4 waves x 4 rows)
constexpr int kClipMaxLds = 64 * 1024;

// One wave's LDS accesses execute in program order, so a buffer only that wave touches needs no workgroup barrier: this keeps the
// compiler from moving LDS accesses across the point and lets the wave's lanes meet there.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(256) void clip_hfilter_u8_kernel(const unsigned char* __restrict__ img, int H, int W, float* __restrict__ tmp, int Sw,
                                                              const int* __restrict__ bounds, const float* __restrict__ wts, int ksize,
                                                              int cap_px, int rowbuf) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* wl = reinterpret_cast<float*>(smem);                               // [ksize][64]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned char* row = smem + (size_t)ksize * 256 + (size_t)wv * rowbuf;      // this wave's row span, 16-byte aligned
    const int xo0 = blockIdx.x * 64, xo = xo0 + lane;
    const int nout = min(64, Sw - xo0);
    for (int i = threadIdx.x; i < nout * ksize; i += 256) {                     // contiguous in global memory, transposed into LDS
        const int l = i / ksize, j = i - l * ksize;
        wl[j * 64 + l] = wts[(long long)xo0 * ksize + i];
    }
    // this lane's taps, clamped so that no table can make the kernel read outside the row or outside its LDS span
    const int span0 = clampi(bounds[xo0 * 2], 0, W - 1);
    int b0 = span0, n = 0;
    if (xo < Sw) {
        b0 = clampi(bounds[xo * 2], span0, W - 1);
        n = max(0, min(min(bounds[xo * 2 + 1], ksize), min(W - b0, span0 + cap_px - b0)));
    }
    int span_end = n > 0 ? b0 + n : span0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) span_end = max(span_end, __shfl_xor(span_end, o, 64));
    const int span_bytes = (span_end - span0) * 3;                              // <= cap_px * 3
    const uintptr_t img_lo = reinterpret_cast<uintptr_t>(img), img_hi = img_lo + (uintptr_t)H * W * 3;
    const int start = n > 0 ? lane % n : 0;
    __syncthreads();
    for (int r = wv; r < kClipRows; r += 4) {
        const int y = blockIdx.y * kClipRows + r;
        int shift = 0;
        if (y < H) {
            const uintptr_t g0 = img_lo + ((uintptr_t)y * W + span0) * 3, a0 = g0 & ~(uintptr_t)15;
            shift = (int)(g0 - a0);
            const int chunks = (shift + span_bytes + 15) >> 4;                  // chunks * 16 <= rowbuf
            for (int k = lane; k < chunks; k += 64) {
                const uintptr_t a = a0 + (uintptr_t)k * 16;
                uint4 v;
                const long long off = (long long)(a - img_lo);                  // (negative in front of an unaligned image)
                if (a >= img_lo && a + 16 <= img_hi) {
                    v = *reinterpret_cast<const uint4*>(img + off);
                } else {                                                        // the image's first / last bytes: never read outside it
                    unsigned int w4[4] = {0u, 0u, 0u, 0u};
                    for (int b = 0; b < 16; ++b)
                        if (a + b >= img_lo && a + b < img_hi) w4[b >> 2] |= (unsigned int)img[off + b] << ((b & 3) * 8);
                    v = make_uint4(w4[0], w4[1], w4[2], w4[3]);
                }
                *reinterpret_cast<uint4*>(row + k * 16) = v;
            }
        }
        wave_lds_sync();
        if (y < H && n > 0) {
            const unsigned char* p = row + shift + (b0 - span0) * 3;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f;
            int jj = start;
            for (int j = 0; j < n; ++j) {
                const float w = wl[jj * 64 + lane];
                const unsigned char* q = p + jj * 3;
                a0 += w * (float)q[0]; a1 += w * (float)q[1]; a2 += w * (float)q[2];
                if (++jj == n) jj = 0;
            }
            const long long plane = (long long)H * Sw, o = (long long)y * Sw + xo;
            tmp[o] = a0; tmp[plane + o] = a1; tmp[2 * plane + o] = a2;
        }
        wave_lds_sync();
    }
}

// Vertical pass over the fp32 intermediate + ToTensor / Normalize, blockIdx.z is the image:
//   out[b][c][yo][x] = (sum_j w[yo][j] * tmp[c][b][b0 + j][x] / 255 - mean) / std
// The horizontal pass ran over the B * H rows of the whole batch, so the intermediate is [3][B][H][Sw] (one plane set per image inside
// each channel); a single photo is B = 1.
__global__ __launch_bounds__(256) void clip_vfilter_norm_batch_kernel(const float* __restrict__ tmp, int B, int H, int Sw, float* __restrict__ out,
                                                                      int Sh, const int* __restrict__ bounds, const float* __restrict__ wts,
                                                                      int ksize, float m0, float m1, float m2, float s0, float s1, float s2) {
    __shared__ float wl[kClipMaxTaps];
    const int yo = blockIdx.y, b = blockIdx.z;
    const int b0 = clampi(bounds[yo * 2], 0, H - 1);
    const int n = clampi(bounds[yo * 2 + 1], 0, min(ksize, H - b0));
    if ((int)threadIdx.x < n) wl[threadIdx.x] = wts[(long long)yo * ksize + threadIdx.x];
    __syncthreads();
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= Sw) return;
    const long long plane = (long long)B * H * Sw;
    const float* p = tmp + ((long long)b * H + b0) * Sw + x;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int j = 0; j < n; ++j) {
        const float w = wl[j];
        const float* q = p + (long long)j * Sw;
        a0 += w * q[0]; a1 += w * q[plane]; a2 += w * q[2 * plane];
    }
    const long long oplane = (long long)Sh * Sw, o = (long long)b * 3 * oplane + (long long)yo * Sw + x;
    out[o] = (a0 / 255.0f - m0) / s0;
    out[oplane + o] = (a1 / 255.0f - m1) / s1;
    out[2 * oplane + o] = (a2 / 255.0f - m2) / s2;
}

// One lane per 16-byte group of an output row.  The groups are cut at 16-byte boundaries of the row's ADDRESS: group 0 is the row's
// unaligned head (byte stores, empty when the row starts aligned), every further group is one aligned 16-byte store, and the last one
// of a row falls back to byte stores when it is short; so any width and any alignment of `out` stores vectors in the interior.
// At the usual 4-6x enlargement consecutive pixels map to the same UNet pixel, so the fused argmax is evaluated only when xidx
// changes: about 16 / scale + 1 times per lane.
__global__ __launch_bounds__(256) void ensemble_mask_u8_kernel(const float* __restrict__ clip, const float* __restrict__ unet,
                                                               const float* __restrict__ alpha_dev, int N, int C, int hc, int wc, int H, int W,
                                                               const int* __restrict__ yidx, const int* __restrict__ xidx,
                                                               const unsigned char* __restrict__ lut, unsigned char* __restrict__ out, int H0,
                                                               int W0) {
    const float alpha = *alpha_dev;
    const int gpr = ((W0 + 15) >> 4) + 1;                                      // groups per row, the head included
    const long long total = (long long)N * H0 * gpr;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        long long r; int g; egm_divmod(i, gpr, r, g);
        long long nn; int y; egm_divmod(r, H0, nn, y);
        const int n = (int)nn;
        unsigned char* rowp = out + ((long long)n * H0 + y) * W0;
        const int head = min(W0, (int)((16 - (reinterpret_cast<uintptr_t>(rowp) & 15)) & 15));
        const int x0 = g == 0 ? 0 : head + (g - 1) * 16, x1 = g == 0 ? head : min(W0, x0 + 16);
        if (x0 >= x1) continue;
        const int uy = clampi(yidx[y], 0, H - 1);
        unsigned long long lo = 0ull, hi = 0ull;                               // the group's output bytes
        int last = -1; unsigned long long cur = 0ull;
        for (int k = 0; k < x1 - x0; ++k) {
            const int ux = clampi(xidx[x0 + k], 0, W - 1);
            if (ux != last) {
                const int best = ensemble_fused_argmax(clip, unet, alpha, n, C, hc, wc, H, W, uy, ux, nullptr);
                cur = lut ? (unsigned long long)lut[best & 255] : (unsigned long long)(best & 255);
                last = ux;
            }
            if (k < 8) lo |= cur << (k * 8); else hi |= cur << ((k - 8) * 8);
        }
        unsigned char* dst = rowp + x0;
        if (g > 0 && x1 - x0 == 16) {
            *reinterpret_cast<uint4*>(dst) = make_uint4((unsigned int)lo, (unsigned int)(lo >> 32), (unsigned int)hi, (unsigned int)(hi >> 32));
        } else {
            for (int k = 0; k < x1 - x0; ++k) dst[k] = (unsigned char)((k < 8 ? lo >> (k * 8) : hi >> ((k - 8) * 8)) & 255ull);
        }
    }
}

}  // namespace

// Both CLIP preprocess entry points (`who` names the one that was called).  The horizontal kernel is row-independent and bounds its
// aligned 16-byte staging by the buffer it is given, so it runs over the B * H rows of the batch as over one tall image (image b
// starts b*H*W*3 bytes in, at any alignment); only the vertical pass needs the image index.  Two launches whatever B.
static int clip_preprocess_launch(const char* who, const void* imgs_bhwc3, int B, int H, int W, float* out_bchw, int Sh, int Sw,
                                  const int* xbounds, const float* xweights, int xksize, const int* ybounds, const float* yweights, int yksize,
                                  const float* mean3_host, const float* std3_host, float* tmp_cbhw, egm_stream_t s) {
    EGM_REQUIRE(imgs_bhwc3 && out_bchw && xbounds && xweights && ybounds && yweights && mean3_host && std3_host && tmp_cbhw,
                "%s: null pointer", who);
    EGM_REQUIRE(B > 0 && H > 0 && W > 0 && Sh > 0 && Sw > 0 && xksize > 0 && yksize > 0, "%s: bad shape", who);
    EGM_REQUIRE((long long)B * H * W * 3 < (1ll << 31) && (long long)B * H * Sw * 3 < (1ll << 31) && (long long)B * 3 * Sh * Sw < (1ll << 31),
                "%s: input too large", who);
    EGM_REQUIRE(B <= 65535 && Sh <= 65535 && egm_cdiv((long long)B * H, kClipRows) <= 65535, "%s: too many rows for one launch", who);
    EGM_REQUIRE(xksize <= kClipMaxTaps && yksize <= kClipMaxTaps,
                "%s: %d x %d filter taps, at most %d per axis are supported (an antialiased reduction by up to 31.5)", who, yksize, xksize,
                kClipMaxTaps);
    EGM_REQUIRE(std3_host[0] != 0.f && std3_host[1] != 0.f && std3_host[2] != 0.f, "%s: zero std", who);
    // input pixels the 64 output columns of a workgroup can span: 63 steps of the scale plus one window (both table rules)
    long long cap = (63ll * W + Sw - 1) / Sw + xksize + 2;
    if (cap > W) cap = W;
    const long long rowbuf = (cap * 3 + 15 + 15) & ~15ll;
    const long long lds = (long long)xksize * 256 + 4 * rowbuf;
    EGM_REQUIRE(lds <= kClipMaxLds, "%s: a reduction of %d -> %d columns needs %lld bytes of LDS per workgroup, at most %d are supported", who, W,
                Sw, lds, kClipMaxLds);
    const int rows = B * H;
    hipLaunchKernelGGL(clip_hfilter_u8_kernel, dim3(egm_cdiv(Sw, 64), egm_cdiv(rows, kClipRows)), dim3(256), (size_t)lds, (hipStream_t)s,
                       (const unsigned char*)imgs_bhwc3, rows, W, tmp_cbhw, Sw, xbounds, xweights, xksize, (int)cap, (int)rowbuf);
    EGM_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(clip_vfilter_norm_batch_kernel, dim3(egm_cdiv(Sw, 256), Sh, B), dim3(256), 0, (hipStream_t)s, (const float*)tmp_cbhw, B, H,
                       Sw, out_bchw, Sh, ybounds, yweights, yksize, mean3_host[0], mean3_host[1], mean3_host[2], std3_host[0], std3_host[1],
                       std3_host[2]);
    EGM_CHECK_LAUNCH(who);
    return EGM_OK;
}

extern "C" int egm_clip_preprocess_u8(const void* img_hwc3, int H, int W, float* out_chw, int Sh, int Sw, const int* xbounds, const float* xweights,
                                      int xksize, const int* ybounds, const float* yweights, int yksize, const float* mean3_host,
                                      const float* std3_host, float* tmp_chw, egm_stream_t s) {
    return clip_preprocess_launch("clip_preprocess_u8", img_hwc3, 1, H, W, out_chw, Sh, Sw, xbounds, xweights, xksize, ybounds, yweights, yksize,
                                  mean3_host, std3_host, tmp_chw, s);
}

extern "C" int egm_clip_preprocess_batch_u8(const void* imgs_bhwc3, int B, int H, int W, float* out_bchw, int Sh, int Sw, const int* xbounds,
                                            const float* xweights, int xksize, const int* ybounds, const float* yweights, int yksize,
                                            const float* mean3_host, const float* std3_host, float* tmp_cbhw, egm_stream_t s) {
    return clip_preprocess_launch("clip_preprocess_batch_u8", imgs_bhwc3, B, H, W, out_bchw, Sh, Sw, xbounds, xweights, xksize, ybounds, yweights,
                                  yksize, mean3_host, std3_host, tmp_cbhw, s);
}

extern "C" int egm_ensemble_mask_u8(const float* clip_logits, const float* unet_logits, const float* alpha_dev, int N, int C, int hc, int wc, int H,
                                    int W, const int* yidx, const int* xidx, const unsigned char* lut, unsigned char* out, int H0, int W0,
                                    egm_stream_t s) {
    EGM_REQUIRE(clip_logits && unet_logits && alpha_dev && yidx && xidx && out, "ensemble_mask_u8: null pointer");
    EGM_REQUIRE(N > 0 && C > 0 && C <= 256 && hc > 0 && wc > 0 && H > 0 && W > 0 && H0 > 0 && W0 > 0, "ensemble_mask_u8: bad shape (C <= 256)");
    const long long groups = (long long)N * H0 * ((W0 + 15) / 16 + 1);
    long long grid = (groups + 255) / 256;
    if (grid > 8192) grid = 8192;
    hipLaunchKernelGGL(ensemble_mask_u8_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)s, clip_logits, unet_logits, alpha_dev, N, C, hc, wc, H, W,
                       yidx, xidx, lut, out, H0, W0);
    EGM_CHECK_LAUNCH("ensemble_mask_u8");
    return EGM_OK;
}
