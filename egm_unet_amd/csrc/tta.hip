// Test-time augmentation: the mirrored and rescaled views of an fp32 NCHW batch, and the merge of the model's outputs on
// those views back in the image's frame.
//   egm_tta_views_f32  dst[f * N + n] = flip_f(resize(src[n] -> h x w)), the F views of one scale in one launch
//   egm_tta_merge_f32  out = mean_v sample_v (or mean_v softmax_c sample_v) per pixel over the V views, and / or lut[argmax_c out]
// A resize is bilinear, align_corners=False, no antialias.  Its taps come from host-made tables (egm_unet_amd.tta.resize_axis, integer
// arithmetic): per output pixel of an axis the two source pixels (i0, i1) and the weight l1 of i1.  The device never computes a
// coordinate.  The arithmetic of a sample is fixed so that a numpy float32 restatement gives the same bits (tests/tta_oracle.py):
//   l0 = 1 - l1,  top = lx0 * a + lx1 * b,  bot = lx0 * c + lx1 * d,  val = ly0 * top + ly1 * bot
// one rounding per operation, no contraction into an FMA; the mean is acc = acc + val in ascending v and one correctly rounded division.
//   shape   a lane owns kStripLanePix consecutive output pixels of one row, a wave kStripCols columns of ONE row, a workgroup kStripRows
//           rows: the row taps (and the view descriptor) are wave-uniform, the column taps differ per lane.  Both kernels are gathers: no
//           atomics, no lane depends on another.  In the merge's mean mode the classes are the outermost loop with a running best, so C costs
//           no registers; in prob mode a view's samples of every class stay in registers (kProbMaxC).
//   memory  taps are gathers (dword loads; at scale 1 consecutive lanes read consecutive addresses); the outputs leave as 16-byte
//           non-temporal stores where the row length is a multiple of 4 and the base is aligned (common.h, EGM_STORE_MODE), else as
//           dwords.
// Every index read from a table is clamped into [0, side - 1] of the tensor it addresses and a flip code is read & 3, so the reads
// stay inside [N][C][h][w] (as the call or the descriptor states it) whatever the tables hold.
#include <math.h>
#include "strip_out.h"

// No multiply of this file may be fused with the add behind it (as csrc/tiles.hip: the pragma governs the operators written below
// it; the __fmul_rn / __fadd_rn wrappers are plain operators inside a header compiled under the default mode, and were fused).  So
// strip_out.h, the frame shared with tiles.hip (the lane's pixels, the running argmax, the stores, the entry points' geometry), holds
// no arithmetic on samples: the taps, acc + val, the softmax and acc / fV stay here, below the pragma.
#pragma clang fp contract(off)

namespace {

constexpr int kTtaMaxV = 4096;
constexpr int kProbMaxC = 8;                           // prob mode: acc and the samples, kProbMaxC x kStripLanePix registers each

// the two taps and weights of one axis for output pixel p, the indices clamped into [0, side - 1] and mirrored for a flipped axis
struct Taps { int i0, i1; float l0, l1; };
__device__ __forceinline__ Taps load_taps(const int* __restrict__ idx, const float* __restrict__ l, int p, int side, bool flipped) {
    Taps t;
    t.i0 = clampi(idx[2 * p], 0, side - 1);
    t.i1 = clampi(idx[2 * p + 1], 0, side - 1);
    if (flipped) { t.i0 = side - 1 - t.i0; t.i1 = side - 1 - t.i1; }
    t.l1 = l[p];
    t.l0 = 1.f - t.l1;
    return t;
}

// rows r0 / r1 of one plane, already at their first column (plain operators: the pragma above governs them, one rounding each)
__device__ __forceinline__ float bilinear(const float* __restrict__ r0, const float* __restrict__ r1, const Taps& ty, const Taps& tx) {
    const float a = r0[tx.i0], b = r0[tx.i1], c = r1[tx.i0], d = r1[tx.i1];
    const float ta = tx.l0 * a, tb = tx.l1 * b, tc = tx.l0 * c, td = tx.l1 * d;
    const float top = ta + tb, bot = tc + td;
    const float vt = ty.l0 * top, vb = ty.l1 * bot;
    return vt + vb;
}

__global__ __launch_bounds__(256) void tta_views_kernel(const float* __restrict__ src, int N, int C, int H, int W, int h, int w,
                                                        const int* __restrict__ yi, const float* __restrict__ yl,
                                                        const int* __restrict__ xi, const float* __restrict__ xl,
                                                        const int* __restrict__ flips, long long rows, float* __restrict__ dst, int vec) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long row = blockIdx.x * (long long)kStripRows + wave;   // row y of class c of view f of image n: dst[f * N + n][c][y]
    if (row >= rows) return;                                   // (a whole wave; the kernel has no barrier)
    long long q, k, f;
    int y, c, n;
    egm_divmod(row, h, q, y);
    egm_divmod(q, C, k, c);
    egm_divmod(k, N, f, n);
    const int flip = flips[f] & 3;
    const Taps ty = load_taps(yi, yl, (flip & 2) ? h - 1 - y : y, H, false);   // the mirror is in which table row a pixel reads
    const float* plane = src + ((long long)n * C + c) * H * W;
    const float* r0 = plane + (long long)ty.i0 * W;
    const float* r1 = plane + (long long)ty.i1 * W;
    float* d = dst + row * w;
    for (int x = lane * kStripLanePix; x < w; x += kStripCols) {
        float out[kStripLanePix];
#pragma unroll
        for (int e = 0; e < kStripLanePix; ++e) {
            out[e] = 0.f;
            if (x + e < w) {
                const Taps tx = load_taps(xi, xl, (flip & 1) ? w - 1 - (x + e) : x + e, W, false);
                out[e] = bilinear(r0, r1, ty, tx);
            }
        }
        store_row4(d + x, out, x, w, vec);
    }
}

// mean: out_c = (sum_v sample_v) / V.  The classes are the outermost loop.
__global__ __launch_bounds__(256) void tta_merge_mean_kernel(const egm_tta_view* __restrict__ views, int V, int C, int H, int W,
                                                             const unsigned char* __restrict__ lut, float* __restrict__ logits,
                                                             unsigned char* __restrict__ mask, int nrg, int ncg, int vec_logits,
                                                             int vec_mask) {
    const auto [n, y, x, outside] = strip_pos(nrg, ncg, H, W);
    if (outside) return;
    const float fV = (float)V;
    StripArgmax top;
    for (int c = 0; c < C; ++c) {
        float acc[kStripLanePix];
#pragma unroll
        for (int e = 0; e < kStripLanePix; ++e) acc[e] = 0.f;
        for (int v = 0; v < V; ++v) {
            const egm_tta_view& d = views[v];                  // wave-uniform
            const int h = max(d.h, 1), w = max(d.w, 1), flip = d.flip & 3;
            const Taps ty = load_taps(d.yi, d.yl, y, h, flip & 2);
            const float* plane = d.logits + ((long long)n * C + c) * h * w;
            const float* r0 = plane + (long long)ty.i0 * w;
            const float* r1 = plane + (long long)ty.i1 * w;
#pragma unroll
            for (int e = 0; e < kStripLanePix; ++e) {
                if (x + e < W) {
                    const Taps tx = load_taps(d.xi, d.xl, x + e, w, flip & 1);
                    const float val = bilinear(r0, r1, ty, tx);
                    acc[e] = acc[e] + val;
                }
            }
        }
        float out[kStripLanePix];
#pragma unroll
        for (int e = 0; e < kStripLanePix; ++e) {
            out[e] = acc[e] / fV;                               // correctly rounded: hipcc's default for fp32 division
            top.take(c, e, out[e]);
        }
        if (logits) store_row4(logits + (((long long)n * C + c) * H + y) * W + x, out, x, W, vec_logits);
    }
    if (mask) top.store_mask(mask + ((long long)n * H + y) * W + x, lut, x, W, vec_mask);
}

// prob: out_c = (sum_v softmax_c(sample_v)) / V.  The views are the outermost loop; acc and one view's samples stay in registers, every
// index into them a compile-time constant (the loops over the classes are unrolled to kProbMaxC and guarded by the wave-uniform C).
__global__ __launch_bounds__(256) void tta_merge_prob_kernel(const egm_tta_view* __restrict__ views, int V, int C, int H, int W,
                                                             const unsigned char* __restrict__ lut, float* __restrict__ logits,
                                                             unsigned char* __restrict__ mask, int nrg, int ncg, int vec_logits,
                                                             int vec_mask) {
    const auto [n, y, x, outside] = strip_pos(nrg, ncg, H, W);
    if (outside) return;
    const float fV = (float)V;
    float acc[kProbMaxC][kStripLanePix];
#pragma unroll
    for (int c = 0; c < kProbMaxC; ++c)
#pragma unroll
        for (int e = 0; e < kStripLanePix; ++e) acc[c][e] = 0.f;
    for (int v = 0; v < V; ++v) {
        const egm_tta_view& d = views[v];                      // wave-uniform
        const int h = max(d.h, 1), w = max(d.w, 1), flip = d.flip & 3;
        const Taps ty = load_taps(d.yi, d.yl, y, h, flip & 2);
        Taps tx[kStripLanePix];
#pragma unroll
        for (int e = 0; e < kStripLanePix; ++e) tx[e] = load_taps(d.xi, d.xl, min(x + e, W - 1), w, flip & 1);
        float s[kProbMaxC][kStripLanePix];
#pragma unroll
        for (int c = 0; c < kProbMaxC; ++c) {
            if (c < C) {
                const float* plane = d.logits + ((long long)n * C + c) * h * w;
                const float* r0 = plane + (long long)ty.i0 * w;
                const float* r1 = plane + (long long)ty.i1 * w;
#pragma unroll
                for (int e = 0; e < kStripLanePix; ++e) s[c][e] = bilinear(r0, r1, ty, tx[e]);
            }
        }
#pragma unroll
        for (int e = 0; e < kStripLanePix; ++e) {
            float m = s[0][e];
#pragma unroll
            for (int c = 1; c < kProbMaxC; ++c)
                if (c < C) m = fmaxf(m, s[c][e]);
            float z = 0.f;
#pragma unroll
            for (int c = 0; c < kProbMaxC; ++c) {
                if (c < C) {
                    s[c][e] = expf(s[c][e] - m);                // the accurate expf, not the exp2-based intrinsic
                    z = z + s[c][e];
                }
            }
#pragma unroll
            for (int c = 0; c < kProbMaxC; ++c) {
                if (c < C) {
                    const float p = s[c][e] / z;                // correctly rounded
                    acc[c][e] = acc[c][e] + p;
                }
            }
        }
    }
    StripArgmax top;
#pragma unroll
    for (int c = 0; c < kProbMaxC; ++c) {
        if (c < C) {
            float out[kStripLanePix];
#pragma unroll
            for (int e = 0; e < kStripLanePix; ++e) {
                out[e] = acc[c][e] / fV;
                top.take(c, e, out[e]);
            }
            if (logits) store_row4(logits + (((long long)n * C + c) * H + y) * W + x, out, x, W, vec_logits);
        }
    }
    if (mask) top.store_mask(mask + ((long long)n * H + y) * W + x, lut, x, W, vec_mask);
}

}  // namespace

extern "C" int egm_tta_views_f32(const float* src, int N, int C, int H, int W, int h, int w, const int* yi_dev, const float* yl_dev,
                                 const int* xi_dev, const float* xl_dev, const int* flips_dev, int F, float* dst, egm_stream_t s) {
    const char* name = "tta_views_f32";
    EGM_REQUIRE(src && dst, "%s: null pointer", name);
    EGM_REQUIRE(yi_dev && yl_dev && xi_dev && xl_dev && flips_dev, "%s: null pointer (the four axis tables and the flip codes are required)",
                name);
    EGM_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "%s: bad shape N=%d C=%d H=%d W=%d", name, N, C, H, W);
    EGM_REQUIRE(h > 0 && w > 0 && F > 0, "%s: bad views: %d flips of %d x %d pixels", name, F, h, w);
    EGM_REQUIRE(H <= kStripMaxSide && W <= kStripMaxSide && h <= kStripMaxSide && w <= kStripMaxSide,
                "%s: %d x %d -> %d x %d pixels, at most %d rows and columns are supported", name, H, W, h, w, kStripMaxSide);
    const long long rows = (long long)F * N * C * h;
    StripRows g;
    if (const int rc = strip_rows_check(name, rows, w, dst, &g); rc != EGM_OK) return rc;
    hipLaunchKernelGGL(tta_views_kernel, dim3(g.groups), dim3(256), 0, (hipStream_t)s, src, N, C, H, W, h, w, yi_dev, yl_dev, xi_dev, xl_dev,
                       flips_dev, rows, dst, g.vec);
    EGM_CHECK_LAUNCH("tta_views_f32");
    return EGM_OK;
}

extern "C" int egm_tta_merge_f32(const egm_tta_view* views_dev, int V, int N, int C, int H, int W, int mode, const unsigned char* lut,
                                 float* logits_out, unsigned char* mask_out, egm_stream_t s) {
    const char* name = "tta_merge_f32";
    EGM_REQUIRE(views_dev, "%s: null pointer (the table of view descriptors is required)", name);
    StripGrid g;
    if (const int rc = strip_check(name, N, C, H, W, logits_out, mask_out, &g); rc != EGM_OK) return rc;
    EGM_REQUIRE(V > 0 && V <= kTtaMaxV, "%s: %d views, between 1 and %d are supported", name, V, kTtaMaxV);
    EGM_REQUIRE(mode == 0 || mode == 1, "%s: bad mode %d (0 = mean of the samples, 1 = mean of their softmax probabilities)", name, mode);
    EGM_REQUIRE(mode == 0 || C <= kProbMaxC, "%s: %d classes, mode 1 (prob) keeps the samples in registers and holds at most %d", name, C,
                kProbMaxC);
    hipLaunchKernelGGL(mode == 0 ? tta_merge_mean_kernel : tta_merge_prob_kernel, dim3((unsigned)g.items), dim3(256), 0, (hipStream_t)s,
                       views_dev, V, C, H, W, lut, logits_out, mask_out, g.nrg, g.ncg, g.vec_logits, g.vec_mask);
    EGM_CHECK_LAUNCH("tta_merge_f32");
    return EGM_OK;
}
