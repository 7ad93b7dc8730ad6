// The ensemble's tail at the UNet's size and its scoring at the ground truth's size (the evaluation half of the ensemble workflow):
//   egm_ensemble_fuse:          clip + alpha * unet -> argmax (and the fused logits), predict_CLIPseg.py:501-525
//   egm_ensemble_alpha_hist:    the alpha grid search against labels at the UNet's size, one confusion matrix per alpha
//   egm_ensemble_miou:          mean IoU of every alpha's matrix
//   egm_mask_confusion_u8:      confusion matrix of a predicted uint8 mask against a ground-truth uint8 mask (evaluating_indicator.py:
//                               347-417, compute_mIoU's fast_hist), one streaming pass over both images
//   egm_ensemble_alpha_hist_u8: the alpha grid search with the UNet-size argmax resized to the label's size by cv2.resize(INTER_NEAREST)
//                               (eval_CLIPseg.py:682-711), one confusion matrix per alpha
//
// Counts are exact integers.  The two _u8 kernels keep 32-bit partial counts on chip and add them to the uint64 matrices with at most one 64-bit
// atomic per cell and workgroup; the launchers refuse sizes at which a 32-bit partial could wrap (see each launcher).
#include "common.h"
#include "ensemble_fuse.h"

namespace {

constexpr int kScoreMaxC = 4;                  // classes, as egm_ensemble_alpha_hist
constexpr int kScoreCells = kScoreMaxC * kScoreMaxC;
constexpr int kScoreMaxAlphas = 128;
constexpr int kConfMaxGrid = 2048;             // 8 workgroups of 256 per CU
constexpr int kConfUnroll = 4;                 // 16-byte chunk pairs in flight per lane

// Byte -> cell tables in LDS: lt[b] = label class * C, pt[b] = predicted class, 16 for a dropped byte; a pixel's cell is
// min(lt[l] + pt[p], 16), and cell 16 is a counter row nobody reads, so a dropped pixel needs no branch.  Every lane owns one 32-bit
// counter per cell, cnt[cell][lane] (lanes of a wave on different banks: an LDS add without conflicts and without a returned value).
struct ConfLds {
    unsigned int cnt[kScoreCells + 1][256];
    unsigned char lt[256], pt[256];
};

__device__ __forceinline__ void conf_count(ConfLds& L, unsigned int p, unsigned int l) {
    const int cell = min((int)L.lt[l] + (int)L.pt[p], kScoreCells);
    atomicAdd(&L.cnt[cell][threadIdx.x], 1u);
}
__device__ __forceinline__ void conf_count16(ConfLds& L, const uint4& p, const uint4& l) {
    const unsigned int pw[4] = {p.x, p.y, p.z, p.w}, lw[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int b = 0; b < 4; ++b) conf_count(L, (pw[w] >> (b * 8)) & 255u, (lw[w] >> (b * 8)) & 255u);
}

// Pixels [0, head) in front of the prediction's first 16-byte boundary and the tail behind the last whole chunk go byte by byte
// (workgroup 0); the body is nchunks chunks of 16 pixels, grid-strided, kConfUnroll chunk pairs loaded before any is counted.  The
// label's alignment is whatever it is once the chunks are cut at the prediction's 16-byte boundaries: load16_any.
__global__ __launch_bounds__(256) void mask_confusion_u8_kernel(const unsigned char* __restrict__ pred, const unsigned char* __restrict__ label,
                                                                long long npix, const unsigned char* __restrict__ pred_cls,
                                                                const unsigned char* __restrict__ label_cls, int C,
                                                                unsigned long long* __restrict__ hist) {
    __shared__ ConfLds L;
    {
        const unsigned int pc = pred_cls[threadIdx.x], lc = label_cls[threadIdx.x];
        L.pt[threadIdx.x] = (unsigned char)(pc < (unsigned)C ? pc : kScoreCells);
        L.lt[threadIdx.x] = (unsigned char)(lc < (unsigned)C ? lc * C : kScoreCells);
        for (int k = 0; k <= kScoreCells; ++k) L.cnt[k][threadIdx.x] = 0u;
    }
    __syncthreads();
    long long head = (long long)((16 - (reinterpret_cast<uintptr_t>(pred) & 15)) & 15);
    if (head > npix) head = npix;
    const long long nchunks = (npix - head) >> 4, tail0 = head + (nchunks << 4);
    const unsigned char* pb = pred + head;
    const unsigned char* lb = label + head;
    const long long stride = (long long)gridDim.x * 256;
    long long c = blockIdx.x * 256LL + threadIdx.x;
    for (; c + (kConfUnroll - 1) * stride < nchunks; c += kConfUnroll * stride) {
        uint4 pv[kConfUnroll], lv[kConfUnroll];
#pragma unroll
        for (int k = 0; k < kConfUnroll; ++k) {
            pv[k] = *reinterpret_cast<const uint4*>(pb + ((c + k * stride) << 4));
            lv[k] = load16_any(lb + ((c + k * stride) << 4));
        }
#pragma unroll
        for (int k = 0; k < kConfUnroll; ++k) conf_count16(L, pv[k], lv[k]);
    }
    for (; c < nchunks; c += stride) conf_count16(L, *reinterpret_cast<const uint4*>(pb + (c << 4)), load16_any(lb + (c << 4)));
    if (blockIdx.x == 0) {
        for (long long i = threadIdx.x; i < head; i += 256) conf_count(L, pred[i], label[i]);
        for (long long i = tail0 + threadIdx.x; i < npix; i += 256) conf_count(L, pred[i], label[i]);
    }
    __syncthreads();
    // 64-bit sums of the 256 lanes' counters: wave w takes cells w, w + 4, ...
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int cell = wv; cell < C * C; cell += 4) {
        unsigned long long v = 0ull;
#pragma unroll
        for (int k = 0; k < 4; ++k) v += L.cnt[cell][lane + 64 * k];
        v = wave_sum_u64(v);
        if (lane == 0 && v) atomicAdd(&hist[cell], v);
    }
}

// A workgroup takes tiles of 256 UNet pixels ("source pixels") of image n, in two phases per tile.
// Phase 1, one lane per source pixel: the label pixels that cv2.resize(INTER_NEAREST) fills from it are the rectangle
// [ybeg[y], ybeg[y+1]) x [xbeg[x], xbeg[x+1]) (possibly empty); their classes are counted once, the bilinear CLIPSeg value and the UNet
// logit of every class are evaluated once, and all of it goes to LDS.
// Phase 2, one lane per ALPHA (two per lane when na > 64): every wave walks 64 of the tile's pixels, whose values all lanes read from
// one LDS address (a broadcast), runs its alphas' argmax and adds the pixel's class counts to matrices it keeps in registers.  No lane
// shares a matrix with another, so nothing is atomic until the end, where with one lane per pixel all 64 lanes of a wave would add
// to the same two or three LDS words per alpha.
// The fused value is the expression of ensemble_fused_argmax (ensemble_fuse.h): bilin_at(..) + alpha * unet, the first maximum wins.
template <int C>
__global__ __launch_bounds__(256) void ensemble_alpha_hist_u8_kernel(const float* __restrict__ clip, const float* __restrict__ unet,
                                                                     const unsigned char* __restrict__ labels,
                                                                     const unsigned char* __restrict__ label_cls,
                                                                     const float* __restrict__ alphas, int na, int N, int hc, int wc, int H, int W,
                                                                     int Hl, int Wl, const int* __restrict__ ybeg,
                                                                     const int* __restrict__ xbeg, unsigned long long* __restrict__ hist) {
    __shared__ unsigned int lh[kScoreMaxAlphas * C * C];          // [na][C][C]
    __shared__ float s_cv[C][256], s_uv[C][256];
    __shared__ unsigned int s_cnt[C][256];
    __shared__ unsigned char lt[256];
    for (int i = threadIdx.x; i < na * C * C; i += 256) lh[i] = 0u;
    lt[threadIdx.x] = label_cls[threadIdx.x];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float al[2];
    unsigned int acc[2][C][C];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        al[k] = lane + 64 * k < na ? alphas[lane + 64 * k] : 0.f;
#pragma unroll
        for (int t = 0; t < C; ++t)
#pragma unroll
            for (int p = 0; p < C; ++p) acc[k][t][p] = 0u;
    }
    __syncthreads();
    const long long HW = (long long)H * W, total = (long long)N * HW, tiles = (total + 255) >> 8;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long i = (tile << 8) + threadIdx.x;
        unsigned int cnt[C];
#pragma unroll
        for (int t = 0; t < C; ++t) cnt[t] = 0u;
        if (i < total) {
            int n, y, x;
            egm_pix_nyx(i, H, W, n, y, x);
            // the tables are clamped, so none can make the kernel read outside the label
            const int Y0 = clampi(ybeg[y], 0, Hl), Y1 = clampi(ybeg[y + 1], Y0, Hl);
            const int X0 = clampi(xbeg[x], 0, Wl), X1 = clampi(xbeg[x + 1], X0, Wl);
            const unsigned char* lab = labels + (long long)n * Hl * Wl;
            for (int Y = Y0; Y < Y1; ++Y) {
                const unsigned char* row = lab + (long long)Y * Wl;
                for (int X = X0; X < X1; ++X) {
                    const int t = lt[row[X]];
#pragma unroll
                    for (int k = 0; k < C; ++k) cnt[k] += (t == k) ? 1u : 0u;
                }
            }
            int y0, y1, x0, x1; float wy, wx;
            bilin_src(y, hc, H, y0, y1, wy); bilin_src(x, wc, W, x0, x1, wx);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                s_cv[c][threadIdx.x] = bilin_at(clip + ((long long)n * C + c) * hc * wc, wc, y0, y1, wy, x0, x1, wx);
                s_uv[c][threadIdx.x] = unet[((long long)n * C + c) * HW + (i - n * HW)];
            }
        }
#pragma unroll
        for (int t = 0; t < C; ++t) s_cnt[t][threadIdx.x] = cnt[t];              // (zeros behind the last pixel: skipped below)
        __syncthreads();
        for (int j = wv * 64; j < wv * 64 + 64; ++j) {
            unsigned int pc[C], any = 0u;
#pragma unroll
            for (int t = 0; t < C; ++t) { pc[t] = s_cnt[t][j]; any |= pc[t]; }
            if (!any) continue;                                                  // the same for every lane
            float cv[C], uv[C];
#pragma unroll
            for (int c = 0; c < C; ++c) { cv[c] = s_cv[c][j]; uv[c] = s_uv[c][j]; }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (k * 64 >= na) break;
                const float alpha = al[k];
                int best = 0; float m = -INFINITY;
#pragma unroll
                for (int c = 0; c < C; ++c) { const float v = cv[c] + alpha * uv[c]; if (v > m) { m = v; best = c; } }
#pragma unroll
                for (int t = 0; t < C; ++t)
#pragma unroll
                    for (int p = 0; p < C; ++p) acc[k][t][p] += (best == p) ? pc[t] : 0u;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int a = lane + 64 * k;
        if (a < na) {
#pragma unroll
            for (int t = 0; t < C; ++t)
#pragma unroll
                for (int p = 0; p < C; ++p) if (acc[k][t][p]) atomicAdd(&lh[(a * C + t) * C + p], acc[k][t][p]);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < na * C * C; i += 256) if (lh[i]) atomicAdd(&hist[i], (unsigned long long)lh[i]);
}

// ---- CLIPSeg (+) UNet ensemble tail (predict_CLIPseg.py:501-525, eval_CLIPseg.py:656-723) ------------------------------------
// fused = bilinear(clip_logits -> HxW, align_corners=False) + alpha * unet_logits ; prediction = argmax_c fused.
// One lane per output pixel; the alpha grid search evaluates every alpha of the grid in the same pass and accumulates one
// confusion matrix per alpha (LDS pre-aggregation, integer atomics).
// (bilin_src, bilin_at and the fused argmax live in ensemble_fuse.h: egm_ensemble_mask_u8 evaluates the same expression)
// pred[n][y][x] = argmax_c (up(clip)[n][c] + alpha * unet[n][c]); fused (optional) receives the fused logits
__global__ void ensemble_fuse_kernel(const float* __restrict__ clip, const float* __restrict__ unet, float alpha, int N, int C, int hc, int wc,
                                     int H, int W, long long* __restrict__ pred, float* __restrict__ fused) {
    const long long HW = (long long)H * W, total = (long long)N * HW;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int x = (int)(i % W), y = (int)((i / W) % H), n = (int)(i / HW);
        const int best = ensemble_fused_argmax(clip, unet, alpha, n, C, hc, wc, H, W, y, x, fused);
        if (pred) pred[i] = best;
    }
}
// The fused logits alone with alpha read from the device (a captured graph follows its value), bit for bit ensemble_fuse_kernel's.  That
// kernel's expression is compiled under the default contracting mode, and which multiply goes into which FMA is the optimiser's choice
// there: a second kernel written with the same operators was vectorised and fused differently.  So this one states the form the kernel
// above has on gfx950 with explicit fmaf under contract(off), which leaves the optimiser no choice (tests/test_gpu_guided.py compares):
//   src = fma(dst + 0.5, in / out, -0.5);  top = fma(1 - wx, a, wx * b), bot = fma(1 - wx, c, wx * d);
//   fused = fma(alpha, unet, fma(1 - wy, top, wy * bot))
__global__ void ensemble_fuse_dev_kernel(const float* __restrict__ clip, const float* __restrict__ unet, const float* __restrict__ alpha_dev,
                                         int N, int C, int hc, int wc, int H, int W, float* __restrict__ fused) {
#pragma clang fp contract(off)
    const float alpha = alpha_dev[0];
    const float sy = (float)hc / (float)H, sx = (float)wc / (float)W;
    const long long HW = (long long)H * W, total = (long long)N * HW;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int x = (int)(i % W), y = (int)((i / W) % H), n = (int)(i / HW);
        float fy = fmaf((float)y + 0.5f, sy, -0.5f), fx = fmaf((float)x + 0.5f, sx, -0.5f);
        if (fy < 0.f) fy = 0.f;
        if (fx < 0.f) fx = 0.f;
        int y0 = (int)fy, x0 = (int)fx;
        if (y0 > hc - 1) y0 = hc - 1;
        if (x0 > wc - 1) x0 = wc - 1;
        const int y1 = y0 + (y0 < hc - 1 ? 1 : 0), x1 = x0 + (x0 < wc - 1 ? 1 : 0);
        const float wy = fy - (float)y0, wx = fx - (float)x0, uy = 1.f - wy, ux = 1.f - wx;
        for (int c = 0; c < C; ++c) {
            const float* m = clip + ((long long)n * C + c) * hc * wc;
            const float a = m[(long long)y0 * wc + x0], b = m[(long long)y0 * wc + x1], cc = m[(long long)y1 * wc + x0], d = m[(long long)y1 * wc + x1];
            const float top = fmaf(ux, a, wx * b), bot = fmaf(ux, cc, wx * d);
            const long long o = ((long long)n * C + c) * HW + (i - (long long)n * HW);
            fused[o] = fmaf(alpha, unet[o], fmaf(uy, top, wy * bot));
        }
    }
}
// hist[a][t][p] += 1 for every alpha a of the grid (C <= 4, na <= 128)
__global__ __launch_bounds__(256) void ensemble_alpha_hist_kernel(const float* __restrict__ clip, const float* __restrict__ unet,
                                                                  const long long* __restrict__ target, const float* __restrict__ alphas, int na,
                                                                  int N, int C, int hc, int wc, int H, int W,
                                                                  unsigned long long* __restrict__ hist) {
    extern __shared__ unsigned int lh[];                         // [na][C][C]
    for (int i = threadIdx.x; i < na * C * C; i += 256) lh[i] = 0;
    __syncthreads();
    const long long HW = (long long)H * W, total = (long long)N * HW;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int x = (int)(i % W), y = (int)((i / W) % H), n = (int)(i / HW);
        const long long t = target[i];
        if (t < 0 || t >= C) continue;
        int y0, y1, x0, x1; float wy, wx;
        bilin_src(y, hc, H, y0, y1, wy); bilin_src(x, wc, W, x0, x1, wx);
        float cv[4], uv[4];
        for (int c = 0; c < C; ++c) {
            cv[c] = bilin_at(clip + ((long long)n * C + c) * hc * wc, wc, y0, y1, wy, x0, x1, wx);
            uv[c] = unet[((long long)n * C + c) * HW + (i - n * HW)];
        }
        for (int a = 0; a < na; ++a) {
            const float al = alphas[a];
            int best = 0; float m = cv[0] + al * uv[0];
            for (int c = 1; c < C; ++c) { const float v = cv[c] + al * uv[c]; if (v > m) { m = v; best = c; } }
            atomicAdd(&lh[(a * C + (int)t) * C + best], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < na * C * C; i += 256) if (lh[i]) atomicAdd(&hist[i], (unsigned long long)lh[i]);
}
// miou[a] = mean_c IoU_c of hist[a]  (ConfusionMatrix.compute, float arithmetic as the reference)
__global__ void ensemble_miou_kernel(const unsigned long long* __restrict__ hist, int na, int C, float* __restrict__ miou) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= na) return;
    float acc = 0.f;
    for (int i = 0; i < C; ++i) {
        float row = 0.f, col = 0.f;
        for (int j = 0; j < C; ++j) { row += (float)hist[(a * C + i) * C + j]; col += (float)hist[(a * C + j) * C + i]; }
        const float dg = (float)hist[(a * C + i) * C + i];
        acc += dg / (row + col - dg);
    }
    miou[a] = acc / (float)C;
}

}  // namespace

// Partial counts: 32 bits per lane and cell, summed in 64 bits per workgroup.  A lane counts at most 16 * ceil(chunks / (grid * 256))
// pixels plus the 30 of head and tail; the grid is min(ceil(chunks / (256 * 4)), 2048): a lane has 4 chunks (one pass of the unrolled
// body) up to 33.5 M pixels and more beyond, and npix <= 2^40 keeps it below 2^22 pixels.
extern "C" int egm_mask_confusion_u8(const unsigned char* pred, const unsigned char* label, long long npix, const unsigned char* pred_cls,
                                     const unsigned char* label_cls, int C, unsigned long long* hist, egm_stream_t s) {
    EGM_REQUIRE(pred && label && pred_cls && label_cls && hist, "mask_confusion_u8: null pointer");
    EGM_REQUIRE(C > 0 && C <= kScoreMaxC, "mask_confusion_u8: %d classes, between 1 and %d are supported", C, kScoreMaxC);
    EGM_REQUIRE(npix > 0 && npix <= (1ll << 40), "mask_confusion_u8: %lld pixels, between 1 and 2^40 are supported", npix);
    long long grid = ((npix >> 4) + 256 * kConfUnroll - 1) / (256 * kConfUnroll);   // kConfUnroll chunks per lane, so the unrolled body runs
    if (grid > kConfMaxGrid) grid = kConfMaxGrid;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(mask_confusion_u8_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)s, pred, label, npix, pred_cls, label_cls, C, hist);
    EGM_CHECK_LAUNCH("mask_confusion_u8");
    return EGM_OK;
}

// Partial counts: 32 bits per lane, alpha and cell, then per workgroup.  Either is at most the call's label pixels, N * Hl * Wl, so
// the call is refused from 2^32 label pixels on (357 photos of 3000 x 4000); split such a batch over several calls.
extern "C" int egm_ensemble_alpha_hist_u8(const float* clip_logits, const float* unet_logits, const unsigned char* labels,
                                          const unsigned char* label_cls, const float* alphas, int na, int N, int C, int hc, int wc, int H,
                                          int W, int Hl, int Wl, const int* ybeg, const int* xbeg, unsigned long long* hist, egm_stream_t s) {
    EGM_REQUIRE(clip_logits && unet_logits && labels && label_cls && alphas && ybeg && xbeg && hist, "ensemble_alpha_hist_u8: null pointer");
    EGM_REQUIRE(na > 0 && na <= kScoreMaxAlphas && C > 0 && C <= kScoreMaxC && N > 0 && hc > 0 && wc > 0 && H > 0 && W > 0 && Hl > 0 && Wl > 0,
                "ensemble_alpha_hist_u8: bad shape (na<=128, C<=4)");
    EGM_REQUIRE((long long)N <= ((1ll << 32) - 1) / ((long long)Hl * Wl),
                "ensemble_alpha_hist_u8: %d labels of %d x %d in one call, fewer than 2^32 label pixels are supported", N, Hl, Wl);
    long long grid = ((long long)N * H * W + 255) / 256;                       // tiles of 256 source pixels
    if (grid > 2048) grid = 2048;                                              // (565 x 753 is 1662 tiles: one each)
#define EGM_ALPHA_HIST_U8(CC) hipLaunchKernelGGL(ensemble_alpha_hist_u8_kernel<CC>, dim3((int)grid), dim3(256), 0, (hipStream_t)s, clip_logits, \
                                                 unet_logits, labels, label_cls, alphas, na, N, hc, wc, H, W, Hl, Wl, ybeg, xbeg, hist)
    switch (C) {
        case 1: EGM_ALPHA_HIST_U8(1); break;
        case 2: EGM_ALPHA_HIST_U8(2); break;
        case 3: EGM_ALPHA_HIST_U8(3); break;
        default: EGM_ALPHA_HIST_U8(4); break;
    }
#undef EGM_ALPHA_HIST_U8
    EGM_CHECK_LAUNCH("ensemble_alpha_hist_u8");
    return EGM_OK;
}

extern "C" int egm_ensemble_fuse(const float* clip_logits, const float* unet_logits, float alpha, int N, int C, int hc, int wc, int H, int W,
                                 long long* pred, float* fused, egm_stream_t s) {
    EGM_REQUIRE(clip_logits && unet_logits && (pred || fused) && N > 0 && C > 0 && hc > 0 && wc > 0 && H > 0 && W > 0, "ensemble_fuse: bad args");
    const long long total = (long long)N * H * W;
    int grid = (int)((total + 255) / 256); if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(ensemble_fuse_kernel, dim3(grid), dim3(256), 0, (hipStream_t)s, clip_logits, unet_logits, alpha, N, C, hc, wc, H, W, pred, fused);
    EGM_CHECK_LAUNCH("ensemble_fuse");
    return EGM_OK;
}
extern "C" int egm_ensemble_fuse_dev_f32(const float* clip_logits, const float* unet_logits, const float* alpha_dev, int N, int C, int hc,
                                         int wc, int H, int W, float* fused, egm_stream_t s) {
    EGM_REQUIRE(clip_logits && unet_logits && alpha_dev && fused, "ensemble_fuse_dev_f32: null pointer");
    EGM_REQUIRE(N > 0 && C > 0 && hc > 0 && wc > 0 && H > 0 && W > 0, "ensemble_fuse_dev_f32: bad shape N=%d C=%d hc=%d wc=%d H=%d W=%d", N, C, hc,
                wc, H, W);
    const long long total = (long long)N * H * W;
    int grid = (int)((total + 255) / 256); if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(ensemble_fuse_dev_kernel, dim3(grid), dim3(256), 0, (hipStream_t)s, clip_logits, unet_logits, alpha_dev, N, C, hc, wc, H, W,
                       fused);
    EGM_CHECK_LAUNCH("ensemble_fuse_dev_f32");
    return EGM_OK;
}
/* hist: zeroed [na][C][C] uint64 (accumulates across calls = across images); miou: fp32 [na] */
extern "C" int egm_ensemble_alpha_hist(const float* clip_logits, const float* unet_logits, const long long* target, const float* alphas, int na,
                                       int N, int C, int hc, int wc, int H, int W, unsigned long long* hist, egm_stream_t s) {
    EGM_REQUIRE(clip_logits && unet_logits && target && alphas && hist, "ensemble_alpha_hist: null pointer");
    EGM_REQUIRE(na > 0 && na <= 128 && C > 0 && C <= 4 && N > 0 && hc > 0 && wc > 0 && H > 0 && W > 0, "ensemble_alpha_hist: bad shape (na<=128, C<=4)");
    const long long total = (long long)N * H * W;
    int grid = (int)((total + 255) / 256); if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(ensemble_alpha_hist_kernel, dim3(grid), dim3(256), (size_t)na * C * C * sizeof(unsigned int), (hipStream_t)s, clip_logits,
                       unet_logits, target, alphas, na, N, C, hc, wc, H, W, hist);
    EGM_CHECK_LAUNCH("ensemble_alpha_hist");
    return EGM_OK;
}
extern "C" int egm_ensemble_miou(const unsigned long long* hist, int na, int C, float* miou, egm_stream_t s) {
    EGM_REQUIRE(hist && miou && na > 0 && C > 0, "ensemble_miou: bad args");
    hipLaunchKernelGGL(ensemble_miou_kernel, dim3((na + 63) / 64), dim3(64), 0, (hipStream_t)s, hist, na, C, miou);
    EGM_CHECK_LAUNCH("ensemble_miou");
    return EGM_OK;
}
