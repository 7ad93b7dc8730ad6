// CLIPSeg visual prompts: the support image of a one-shot query, built from a decoded photo and its mask on the device.
//   egm_vprompt_mask_f32   uint8 masks [K][H][W] -> coverage m [K][S][S] in [0, 1]: the antialiased triangle filter of the photo's
//                          resize on the 0/1 indicator (two launches); the second one also resets the K box records
//   egm_vprompt_blend_f32  x [K][3][S][S], m -> the mode's blend of x, m and the Gaussian-blurred x; the same launch finds each image's
//                          bounding box of m > 0 (one launch)
//   egm_vprompt_crop_f32   the square window around the box, read from the record on the device, resampled to S x S (one launch)
//   egm_cond_mix_f32       out[g] = w * text[g] + (1 - w) * mean(vis[group g]) (one launch)
// All arithmetic is fp32 with one rounding per operation written below and a fixed order, so that a numpy float32 restatement gives the
// same bits (tests/vprompt_oracle.py):
//   resample  acc = w[0] * v[0];  acc = acc + w[j] * v[j]  for j = 1 ..   (both axes; columns first);  m = min(acc, 1)
//   blur      the same form over the 15 taps, rows first, then columns; reflect-101 at the border (index -i reads i, S-1+i reads S-1-i)
//   blend     t = x * m;  u = (bg * xb) * (1 - m);  out = (t + u) - sub
//   crop      value = (1-fy) * ((1-fx) * a00 + fx * a01) + fy * ((1-fx) * a10 + fx * a11), taps and weights from integers (see the kernel)
//   mix       s = vis[first]; s = s + vis[next] ..;  mean = s / n;  out = w * text + (1 - w) * mean
//   shape   blend: a workgroup owns a kTile x kTile tile of one image.  With a blur it stages the tile of x with its 7-pixel halo on every
//           side (46 x 46 per channel, borders reflected: the only reads of x for the blur) in LDS, fills an LDS strip
//           [3][kTile + 14][kTile] with the row-blurred values of the tile's rows and the 7 above and below, then every lane runs the
//           column taps of its 4 pixels out of the strip (consecutive lanes, consecutive banks).  Without a blur both are skipped.
//           mask, horizontal: see the kernel; mask vertical / crop / mix: one lane per output element, no LDS beyond the filter weights.
//   box     every lane holds m of its 4 pixels; the extents of m > 0 are reduced over the wave with shuffles and lane 0 issues at most
//           four vector atomics (atomicMin / atomicMax on int32) into the image's record {y0, y1, x0, x1}.  The record is reset by
//           egm_vprompt_mask_f32 and read by egm_vprompt_crop_f32: stream order is the only synchronisation, nothing returns to the host.
// Every index read from a table or from the box record is clamped before it addresses memory.
#include "common.h"

// No multiply of this file may be fused with the add behind it (as csrc/tta.hip).
#pragma clang fp contract(off)

namespace {

constexpr int kTile = 32;                       // tile width and height of the blend kernel (tests/test_gpu_vprompt.py restates these)
constexpr int kRadius = 7;                      // 15 taps
constexpr int kTaps = 2 * kRadius + 1;
constexpr int kStripRows = kTile + 2 * kRadius;
constexpr int kXtStride = kStripRows + 1;       // row stride of the staged x tile
constexpr int kPix = kTile * kTile / 256;       // pixels per lane: rows ly, ly + 8, ly + 16, ly + 24 of one column
constexpr int kVpMaxSide = 8192;                // the crop's integer arithmetic stays inside int32
constexpr int kVpMaxTaps = 64;                  // as the photo's resize (csrc/ensemble_pipe.hip)
constexpr int kModes = 7;
constexpr int kMaskRows = 16;                   // rows per workgroup of the mask's horizontal pass (4 waves x 4 rows)
constexpr int kVpMaxLds = 64 * 1024;

struct Taps15 { float t[kTaps]; };
struct Lut256 { unsigned int w[8]; };           // bit v set: mask value v is object

__device__ __forceinline__ int reflect101(int i, int S) {
    if (i < 0) i = -i;
    if (i > S - 1) i = 2 * (S - 1) - i;
    return clampi(i, 0, S - 1);                // (only rows / columns of a tile's overhang past the image need the clamp)
}

// ---- mask -> coverage ------------------------------------------------------------------------------------------------------------------
// One wave's LDS accesses execute in program order, so a buffer only that wave touches needs no workgroup barrier (as
// csrc/ensemble_pipe.hip): this keeps the compiler from moving LDS accesses across the point and lets the wave's lanes meet there.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// horizontal: tmp[r][xo] = sum_j w[xo][j] * ind(mask[r][b0 + j]) over the K * H rows of the batch, the structure of the photo's
// horizontal pass: a workgroup owns 64 output columns (one per lane) and kMaskRows rows; the columns' weights are staged once as
// [tap][lane]; each wave then takes rows of its own, stages the bytes of the row's input span as 0 / 1 indicators into its own LDS
// buffer with aligned dword loads (the only reads of the mask, coalesced) and every lane runs its taps out of it in ascending order.
__global__ __launch_bounds__(256) void vp_mask_h_kernel(const unsigned char* __restrict__ mask, long long rows, int W, float* __restrict__ tmp,
                                                        int S, const int* __restrict__ bounds, const float* __restrict__ wts, int ksize,
                                                        Lut256 lut, int cap_px, int rowbuf) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* wl = reinterpret_cast<float*>(smem);                               // [ksize][64]
    unsigned int* lutl = reinterpret_cast<unsigned int*>(smem + (size_t)ksize * 256);       // [8]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned char* row = smem + (size_t)ksize * 256 + 32 + (size_t)wv * rowbuf;  // this wave's row span, 16-byte aligned
    const int xo0 = blockIdx.y * 64, xo = xo0 + lane;
    const int nout = min(64, S - xo0);
    for (int i = threadIdx.x; i < nout * ksize; i += 256) {                     // contiguous in global memory, transposed into LDS
        const int l = i / ksize, j = i - l * ksize;
        wl[j * 64 + l] = wts[(long long)xo0 * ksize + i];
    }
    if (threadIdx.x < 8) lutl[threadIdx.x] = lut.w[threadIdx.x];
    // this lane's taps, clamped so that no table can make the kernel read outside the row or outside its LDS span
    const int span0 = clampi(bounds[xo0 * 2], 0, W - 1);
    int b0 = span0, n = 0;
    if (xo < S) {
        b0 = clampi(bounds[xo * 2], span0, W - 1);
        n = max(0, min(min(bounds[xo * 2 + 1], ksize), min(W - b0, span0 + cap_px - b0)));
    }
    int span_end = n > 0 ? b0 + n : span0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) span_end = max(span_end, __shfl_xor(span_end, o, 64));
    const int span_bytes = span_end - span0;                                    // <= cap_px
    const uintptr_t lo = reinterpret_cast<uintptr_t>(mask), hi = lo + (uintptr_t)rows * W;
    __syncthreads();
    for (int r = wv; r < kMaskRows; r += 4) {
        const long long y = blockIdx.x * (long long)kMaskRows + r;
        int shift = 0;
        if (y < rows) {
            const uintptr_t g0 = lo + (uintptr_t)y * W + span0, a0 = g0 & ~(uintptr_t)3;
            shift = (int)(g0 - a0);
            const int words = (shift + span_bytes + 3) >> 2;                    // words * 4 <= rowbuf
            for (int k = lane; k < words; k += 64) {
                const uintptr_t a = a0 + (uintptr_t)k * 4;
                const long long off = (long long)(a - lo);                      // (negative in front of an unaligned buffer)
                unsigned int v = 0u;
                if (a >= lo && a + 4 <= hi) {
                    v = *reinterpret_cast<const unsigned int*>(mask + off);
                } else {                                                        // the buffer's first / last bytes: never read outside it
                    for (int b = 0; b < 4; ++b)
                        if (a + b >= lo && a + b < hi) v |= (unsigned int)mask[off + b] << (b * 8);
                }
                unsigned int ind = 0u;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const unsigned int byte = (v >> (b * 8)) & 255u;
                    ind |= ((lutl[byte >> 5] >> (byte & 31)) & 1u) << (b * 8);
                }
                reinterpret_cast<unsigned int*>(row)[k] = ind;
            }
        }
        wave_lds_sync();
        if (y < rows && xo < S) {
            const unsigned char* p = row + shift + (b0 - span0);
            float acc = 0.f;
            for (int j = 0; j < n; ++j) {
                const float prod = wl[j * 64 + lane] * (float)p[j];             // the indicator is 0 or 1: the product is exact
                acc = j == 0 ? prod : acc + prod;
            }
            tmp[y * S + xo] = acc;
        }
        wave_lds_sync();
    }
}

// vertical: m[k][yo][x] = min(sum_j w[yo][j] * tmp[k][b0 + j][x], 1); workgroup (0, 0, k) resets box record k to the empty box
__global__ __launch_bounds__(256) void vp_mask_v_kernel(const float* __restrict__ tmp, int H, int S, float* __restrict__ m,
                                                        const int* __restrict__ bounds, const float* __restrict__ wts, int ksize,
                                                        int* __restrict__ box) {
    __shared__ float wl[kVpMaxTaps];
    const int yo = blockIdx.y, k = blockIdx.z;
    const int b0 = clampi(bounds[yo * 2], 0, H - 1);
    const int n = clampi(bounds[yo * 2 + 1], 0, min(min(ksize, kVpMaxTaps), H - b0));
    if ((int)threadIdx.x < n) wl[threadIdx.x] = wts[(long long)yo * ksize + threadIdx.x];
    if (blockIdx.x == 0 && yo == 0 && threadIdx.x < 4) box[k * 4 + threadIdx.x] = (threadIdx.x & 1) ? 0 : S;      // {y0, y1, x0, x1}
    __syncthreads();
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= S) return;
    const float* p = tmp + ((long long)k * H + b0) * S + x;
    float acc = 0.f;
    for (int j = 0; j < n; ++j) {
        const float prod = wl[j] * p[(long long)j * S];
        acc = j == 0 ? prod : acc + prod;
    }
    m[((long long)k * S + yo) * S + x] = fminf(acc, 1.f);
}

// ---- blend + box -----------------------------------------------------------------------------------------------------------------------
// modes: 0 overlay, 1 highlight, 2 highlight2, 3 shape, 4 image_only, 5 image_black, 6 blur blend
__device__ __forceinline__ float blend_px(int mode, float x, float xb, float m, float bg, float sub) {
    switch (mode) {
    case 0: return x * m;
    case 1: { const float a = x * m, b = a * 0.85f, c = 0.15f * x; return b + c; }
    case 2: { const float h = x / 2.f, a = h + 0.1f, b = a * m, c = 0.3f * h; return b + c; }
    case 3: return m;
    case 4: return x;
    case 5: return x * 0.f;
    default: { const float t = x * m, g = bg * xb, om = 1.f - m, u = g * om, r = t + u; return r - sub; }
    }
}

template <bool BLUR>
__global__ __launch_bounds__(256) void vp_blend_kernel(const float* __restrict__ x, const float* __restrict__ m, float* __restrict__ out,
                                                       int* __restrict__ box, int S, int mode, Taps15 taps, float bg, float sub) {
    __shared__ float strip[BLUR ? 3 * kStripRows * kTile : 1];
    __shared__ float xt[BLUR ? 3 * kStripRows * kXtStride : 1];
    const int k = blockIdx.z, x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
    const long long plane = (long long)S * S;
    const float* xi = x + (long long)k * 3 * plane;
    if (BLUR) {
        for (int e = threadIdx.x; e < 3 * kStripRows * kStripRows; e += 256) {  // the tile of x with its halo, borders reflected
            const int cx = e % kStripRows, rc = e / kStripRows, r = rc % kStripRows, c = rc / kStripRows;
            xt[(c * kStripRows + r) * kXtStride + cx] =
                xi[c * plane + (long long)reflect101(y0 - kRadius + r, S) * S + reflect101(x0 - kRadius + cx, S)];
        }
        __syncthreads();
        for (int e = threadIdx.x; e < 3 * kStripRows * kTile; e += 256) {       // rows: a wave reads two rows, each half its own banks
            const int lx = e % kTile, rc = e / kTile;
            const float* row = xt + rc * kXtStride + lx;
            float acc = taps.t[0] * row[0];
#pragma unroll
            for (int j = 1; j < kTaps; ++j) {
                const float prod = taps.t[j] * row[j];
                acc = acc + prod;
            }
            strip[e] = acc;
        }
        __syncthreads();
    }
    const int lx = threadIdx.x % kTile, ly = threadIdx.x / kTile, px = x0 + lx;
    int bymin = S, bymax = 0, bxmin = S, bxmax = 0;
    if (px < S) {
#pragma unroll
        for (int i = 0; i < kPix; ++i) {
            const int ty = ly + i * (256 / kTile), py = y0 + ty;
            if (py >= S) break;
            const long long o = (long long)py * S + px;
            const float mv = m[(long long)k * plane + o];
            if (mv > 0.f) { bymin = min(bymin, py); bymax = max(bymax, py + 1); bxmin = min(bxmin, px); bxmax = max(bxmax, px + 1); }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float xv = xi[c * plane + o];
                float xb = xv;
                if (BLUR) {
                    const float* col = strip + (c * kStripRows + ty) * kTile + lx;
                    float acc = taps.t[0] * col[0];
#pragma unroll
                    for (int j = 1; j < kTaps; ++j) {
                        const float prod = taps.t[j] * col[j * kTile];
                        acc = acc + prod;
                    }
                    xb = acc;
                }
                out[((long long)k * 3 + c) * plane + o] = blend_px(mode, xv, xb, mv, bg, sub);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        bymin = min(bymin, __shfl_xor(bymin, o, 64)); bymax = max(bymax, __shfl_xor(bymax, o, 64));
        bxmin = min(bxmin, __shfl_xor(bxmin, o, 64)); bxmax = max(bxmax, __shfl_xor(bxmax, o, 64));
    }
    if ((threadIdx.x & 63) == 0 && bymax > 0) {
        atomicMin(box + k * 4 + 0, bymin); atomicMax(box + k * 4 + 1, bymax);
        atomicMin(box + k * 4 + 2, bxmin); atomicMax(box + k * 4 + 3, bxmax);
    }
}

// ---- crop ------------------------------------------------------------------------------------------------------------------------------
// One axis of the window [lo, lo + L) resampled to S pixels: output o reads taps i, i + 1 (clamped into the window, then offset by lo)
// with weight f of the second, n = (2o + 1) L - S, i = floor(n / 2S), f = (n - i 2S) / 2S.
struct CropTap { int i0, i1; float f; };
__device__ __forceinline__ CropTap crop_tap(int o, int L, int S, int lo) {
    const int n = (2 * o + 1) * L - S, i = n < 0 ? -1 : n / (2 * S);            // n > -2S: floor(n / 2S) is -1 for every negative n
    CropTap t;
    t.f = (float)(n - i * 2 * S) / (float)(2 * S);
    t.i0 = clampi(i, 0, L - 1) + lo;
    t.i1 = clampi(i + 1, 0, L - 1) + lo;
    return t;
}

__global__ __launch_bounds__(256) void vp_crop_kernel(const float* __restrict__ src, const int* __restrict__ box, float* __restrict__ out, int S,
                                                      int cnum) {
    const int k = blockIdx.z, oy = blockIdx.y, ox = blockIdx.x * 256 + threadIdx.x;
    if (ox >= S) return;
    const int by0 = clampi(box[k * 4 + 0], 0, S), by1 = clampi(box[k * 4 + 1], 0, S);
    const int bx0 = clampi(box[k * 4 + 2], 0, S), bx1 = clampi(box[k * 4 + 3], 0, S);
    int top = 0, left = 0, L = S;
    if (by1 > by0 && bx1 > bx0) {
        const int side = max(by1 - by0, bx1 - bx0), pad = (side * cnum + 1023) >> 10;
        L = side + 2 * pad;
        top = (by0 + by1 - L) >> 1;                                              // floor, also of a negative numerator
        left = (bx0 + bx1 - L) >> 1;
    }
    const CropTap ty = crop_tap(oy, L, S, top), tx = crop_tap(ox, L, S, left);
    const bool y0in = ty.i0 >= 0 && ty.i0 < S, y1in = ty.i1 >= 0 && ty.i1 < S, x0in = tx.i0 >= 0 && tx.i0 < S, x1in = tx.i1 >= 0 && tx.i1 < S;
    const long long plane = (long long)S * S;
    const float wy0 = 1.f - ty.f, wx0 = 1.f - tx.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* p = src + ((long long)k * 3 + c) * plane;
        const float a00 = y0in && x0in ? p[(long long)ty.i0 * S + tx.i0] : 0.f, a01 = y0in && x1in ? p[(long long)ty.i0 * S + tx.i1] : 0.f;
        const float a10 = y1in && x0in ? p[(long long)ty.i1 * S + tx.i0] : 0.f, a11 = y1in && x1in ? p[(long long)ty.i1 * S + tx.i1] : 0.f;
        const float t0 = wx0 * a00, t1 = tx.f * a01, b0 = wx0 * a10, b1 = tx.f * a11;
        const float tt = t0 + t1, bb = b0 + b1;
        const float vt = wy0 * tt, vb = ty.f * bb;
        out[((long long)k * 3 + c) * plane + (long long)oy * S + ox] = vt + vb;
    }
}

// ---- conditional mix -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cond_mix_kernel(float* __restrict__ out, const float* __restrict__ vis, const int* __restrict__ group_off,
                                                       const float* __restrict__ text, float w, int G, int K, int D) {
    const long long total = (long long)G * D;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        long long g; int d;
        egm_divmod(i, D, g, d);
        const int a = clampi(group_off[g], 0, K), b = clampi(group_off[g + 1], a, K);
        float mean = 0.f;
        if (b > a) {
            float s = vis[(long long)a * D + d];
            for (int r = a + 1; r < b; ++r) s = s + vis[(long long)r * D + d];
            mean = s / (float)(b - a);                                           // correctly rounded: hipcc's default for fp32 division
        }
        if (text != nullptr) {
            const float t = w * text[i], om = 1.f - w, v = om * mean;
            mean = t + v;
        }
        out[i] = mean;
    }
}

inline int vp_grid(long long n) { long long b = (n + 255) / 256; if (b > 8192) b = 8192; return (int)(b < 1 ? 1 : b); }

}  // namespace

extern "C" int egm_vprompt_mask_f32(const void* masks_khw, int K, int H, int W, float* m_kss, int S, const int* xbounds, const float* xweights,
                                    int xksize, const int* ybounds, const float* yweights, int yksize, const unsigned int* lut8_host,
                                    float* tmp_khs, int* box_k4, egm_stream_t s) {
    const char* name = "vprompt_mask_f32";
    EGM_REQUIRE(masks_khw && m_kss && xbounds && xweights && ybounds && yweights && lut8_host && tmp_khs && box_k4, "%s: null pointer", name);
    EGM_REQUIRE(K >= 1, "%s: K = %d, at least one mask is required", name, K);
    EGM_REQUIRE(S >= 8, "%s: S = %d, at least 8 is required (the blur's radius of 7 reflects once)", name, S);
    EGM_REQUIRE(S <= kVpMaxSide, "%s: S = %d, at most %d is supported", name, S, kVpMaxSide);
    EGM_REQUIRE(H > 0 && W > 0, "%s: bad shape H=%d W=%d", name, H, W);
    EGM_REQUIRE(xksize > 0 && yksize > 0 && xksize <= kVpMaxTaps && yksize <= kVpMaxTaps,
                "%s: %d x %d filter taps, between 1 and %d per axis are supported", name, yksize, xksize, kVpMaxTaps);
    EGM_REQUIRE((long long)K * H * W < (1ll << 31) && (long long)K * H * S < (1ll << 31) && (long long)K * S * S < (1ll << 31),
                "%s: input too large (K * H * W, K * H * S and K * S * S must stay below 2^31 elements)", name);
    EGM_REQUIRE(K <= 65535, "%s: K = %d, at most 65535 images per launch", name, K);
    Lut256 lut;
    memcpy(lut.w, lut8_host, sizeof(lut.w));
    const long long rows = (long long)K * H;
    // input pixels the 64 output columns of a workgroup can span: 63 steps of the scale plus one window (as the photo's pass)
    long long cap = (63ll * W + S - 1) / S + xksize + 2;
    if (cap > W) cap = W;
    const long long rowbuf = (cap + 6 + 15) & ~15ll;                            // up to 3 bytes of alignment in front, 3 behind
    const long long lds = (long long)xksize * 256 + 32 + 4 * rowbuf;
    EGM_REQUIRE(lds <= kVpMaxLds, "%s: a reduction of %d -> %d columns needs %lld bytes of LDS per workgroup, at most %d are supported", name, W,
                S, lds, kVpMaxLds);
    hipLaunchKernelGGL(vp_mask_h_kernel, dim3(egm_cdiv(rows, kMaskRows), egm_cdiv(S, 64)), dim3(256), (size_t)lds, (hipStream_t)s,
                       (const unsigned char*)masks_khw, rows, W, tmp_khs, S, xbounds, xweights, xksize, lut, (int)cap, (int)rowbuf);
    EGM_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(vp_mask_v_kernel, dim3(egm_cdiv(S, 256), S, K), dim3(256), 0, (hipStream_t)s, (const float*)tmp_khs, H, S, m_kss, ybounds,
                       yweights, yksize, box_k4);
    EGM_CHECK_LAUNCH(name);
    return EGM_OK;
}

extern "C" int egm_vprompt_blend_f32(const float* x_k3ss, const float* m_kss, float* out_k3ss, int* box_k4, int K, int S, int mode,
                                     const float* taps15_host, int blur, float bg_fac, float sub, egm_stream_t s) {
    const char* name = "vprompt_blend_f32";
    EGM_REQUIRE(x_k3ss && m_kss && out_k3ss && box_k4 && taps15_host, "%s: null pointer", name);
    EGM_REQUIRE(K >= 1, "%s: K = %d, at least one image is required", name, K);
    EGM_REQUIRE(S >= 8, "%s: S = %d, at least 8 is required (the blur's radius of 7 reflects once)", name, S);
    EGM_REQUIRE(S <= kVpMaxSide, "%s: S = %d, at most %d is supported", name, S, kVpMaxSide);
    EGM_REQUIRE(mode >= 0 && mode < kModes, "%s: bad mode %d (0 .. %d)", name, mode, kModes - 1);
    EGM_REQUIRE((long long)K * 3 * S * S < (1ll << 31), "%s: input too large (K * 3 * S * S must stay below 2^31 elements)", name);
    EGM_REQUIRE(K <= 65535, "%s: K = %d, at most 65535 images per launch", name, K);
    Taps15 taps;
    memcpy(taps.t, taps15_host, sizeof(taps.t));
    const dim3 grid(egm_cdiv(S, kTile), egm_cdiv(S, kTile), K);
    if (blur && mode == 6)
        hipLaunchKernelGGL((vp_blend_kernel<true>), grid, dim3(256), 0, (hipStream_t)s, x_k3ss, m_kss, out_k3ss, box_k4, S, mode, taps, bg_fac, sub);
    else
        hipLaunchKernelGGL((vp_blend_kernel<false>), grid, dim3(256), 0, (hipStream_t)s, x_k3ss, m_kss, out_k3ss, box_k4, S, mode, taps, bg_fac, sub);
    EGM_CHECK_LAUNCH(name);
    return EGM_OK;
}

extern "C" int egm_vprompt_crop_f32(const float* src_k3ss, const int* box_k4, float* out_k3ss, int K, int S, int cnum, egm_stream_t s) {
    const char* name = "vprompt_crop_f32";
    EGM_REQUIRE(src_k3ss && box_k4 && out_k3ss, "%s: null pointer", name);
    EGM_REQUIRE(src_k3ss != out_k3ss, "%s: the crop cannot run in place", name);
    EGM_REQUIRE(K >= 1, "%s: K = %d, at least one image is required", name, K);
    EGM_REQUIRE(S >= 8, "%s: S = %d, at least 8 is required", name, S);
    EGM_REQUIRE(S <= kVpMaxSide, "%s: S = %d, at most %d is supported", name, S, kVpMaxSide);
    EGM_REQUIRE(cnum >= 0 && cnum <= 1024, "%s: center_context * 1024 = %d, between 0 and 1024 is supported", name, cnum);
    EGM_REQUIRE((long long)K * 3 * S * S < (1ll << 31), "%s: input too large (K * 3 * S * S must stay below 2^31 elements)", name);
    EGM_REQUIRE(K <= 65535, "%s: K = %d, at most 65535 images per launch", name, K);
    hipLaunchKernelGGL(vp_crop_kernel, dim3(egm_cdiv(S, 256), S, K), dim3(256), 0, (hipStream_t)s, src_k3ss, box_k4, out_k3ss, S, cnum);
    EGM_CHECK_LAUNCH(name);
    return EGM_OK;
}

extern "C" int egm_cond_mix_f32(float* out_gd, const float* vis_kd, const int* group_off, const float* text_gd, float w, int G, int K, int D,
                                egm_stream_t s) {
    const char* name = "cond_mix_f32";
    EGM_REQUIRE(out_gd && vis_kd && group_off, "%s: null pointer", name);
    EGM_REQUIRE(K >= 1 && G >= 1 && G <= K && D >= 1, "%s: bad shape G=%d K=%d D=%d (1 <= G <= K, every group holds a vector)", name, G, K, D);
    EGM_REQUIRE((long long)K * D < (1ll << 31), "%s: input too large (K * D must stay below 2^31 elements)", name);
    hipLaunchKernelGGL(cond_mix_kernel, dim3(vp_grid((long long)G * D)), dim3(256), 0, (hipStream_t)s, out_gd, vis_kd, group_off, text_gd, w, G, K, D);
    EGM_CHECK_LAUNCH(name);
    return EGM_OK;
}
