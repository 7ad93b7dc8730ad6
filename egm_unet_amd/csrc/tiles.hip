// Sliding-window inference: cut an fp32 NCHW batch into overlapping windows, and blend the windows' logits back with a
// separable weight that fades towards the window's edge.
//   egm_tile_gather_f32  dst[k] = tile min(t0 + k, T - 1) of src, one launch whatever count is
//   egm_tile_blend_f32   out = sum_t wt_t * tile_t / sum_t wt_t per pixel over the tiles that cover it, and / or lut[argmax_c out]
// Tile t = (n * ny + i) * nx + j covers rows ys[i] .. ys[i] + h - 1 and columns xs[j] .. xs[j] + w - 1 of image n; ys and xs ascend.
// The blend is a gather: a lane owns kBlendLanePix consecutive pixels of one row and visits the tiles that cover each of them in
// ascending t (i outside, j inside).  No atomics and no lane depends on another, so the result does not depend on scheduling.  The
// arithmetic is fixed so that a numpy float32 restatement gives the same bits (tests/tile_oracle.py): wt = wy * wx, p = wt * v,
// acc = acc + p, wsum = wsum + wt, one rounding each and no contraction into an FMA, then one correctly rounded division.
//   shape   a wave owns kBlendCols columns of ONE row, a workgroup kBlendRows rows: the row range of covering tiles is wave-uniform (a
//           scalar loop), the column range differs per lane (a divergent loop, two tiles at the usual overlap).  The classes are the
//           outermost loop with a running best, so C costs no registers.
//   memory  T*C*h*w*4 bytes read once or (in the overlaps) a few times from neighbouring workgroups, N*C*H*W*4 (+ N*H*W) written once:
//           the logits leave as 16-byte non-temporal stores where W % 4 == 0 and the base is aligned (common.h, EGM_STORE_MODE),
//           else as dwords.  A tile row starts at any x0: where x0 and w are multiples of 4 (window 480 at overlap 0.25: every tile
//           but a clamped last one) the lane's four pixels are one 16-byte load of the tile and one of wx, else dwords (consecutive
//           lanes, consecutive addresses).  Both forms do the same arithmetic per pixel.
// Every tile read is at (t, c, y - y0, x - x0) with 0 <= y - y0 < h and 0 <= x - x0 < w checked in the kernel: inside [T][C][h][w]
// whatever the tables hold.  The gather clamps a tile's origin into the image for the same reason.
#include "common.h"

// No multiply of this file may be fused with the add behind it.  The pragma governs the operators written below it; the __fmul_rn /
// __fadd_rn wrappers are plain operators inside a header compiled under the default (contracting) mode, and were fused.
#pragma clang fp contract(off)

namespace {

constexpr int kBlendRows = 4;                          // rows per workgroup, one per wave (tests/test_gpu_tiled.py restates both)
constexpr int kBlendLanePix = 4;                       // consecutive pixels per lane
constexpr int kBlendCols = 64 * kBlendLanePix;         // columns per wave
constexpr int kTileMaxSide = 32767;
constexpr int kTileMaxC = 256;                         // a class index fits the mask's byte

// the first index of an ascending table whose tile reaches p: starts[i] + size > p (n when none does)
__device__ __forceinline__ int first_cover(const int* __restrict__ starts, int n, int size, int p) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (starts[mid] + size > p) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void tile_gather_kernel(const float* __restrict__ src, int C, int H, int W, const int* __restrict__ ys,
                                                          int ny, const int* __restrict__ xs, int nx, int h, int w, int T, int t0,
                                                          long long rows, float* __restrict__ dst, int vec) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long row = blockIdx.x * 4LL + wave;             // row r of class c of dst[k]
    if (row >= rows) return;                                   // (a whole wave; the kernel has no barrier)
    long long q, k, ti, n;
    int r, c, i, j;
    egm_divmod(row, h, q, r);
    egm_divmod(q, C, k, c);
    const long long t = min((long long)t0 + k, (long long)T - 1);
    egm_divmod(t, nx, ti, j);
    egm_divmod(ti, ny, n, i);
    const int y0 = min(max(ys[i], 0), H - h), x0 = min(max(xs[j], 0), W - w);
    const float* s = src + ((n * C + c) * H + y0 + r) * W + x0;
    float* d = dst + row * w;
    const bool wide = vec && (reinterpret_cast<uintptr_t>(s) & 15) == 0;       // this row of the image happens to be aligned: 16-byte loads too
    for (int x = lane * kBlendLanePix; x < w; x += kBlendCols) {
        if (vec) {                                             // w % 4 == 0 and dst aligned: the lane's four columns are inside
            float4 v;
            if (wide) v = *reinterpret_cast<const float4*>(s + x);
            else v = make_float4(s[x], s[x + 1], s[x + 2], s[x + 3]);
            egm_u32x4 a;
            a.x = __float_as_uint(v.x); a.y = __float_as_uint(v.y); a.z = __float_as_uint(v.z); a.w = __float_as_uint(v.w);
            egm_store16_as<EGM_STORE_MODE>(d + x, a);
        } else {
#pragma unroll
            for (int e = 0; e < kBlendLanePix; ++e)
                if (x + e < w) d[x + e] = s[x + e];
        }
    }
}

__global__ __launch_bounds__(256) void tile_blend_kernel(const float* __restrict__ tiles, int C, int H, int W, const int* __restrict__ ys,
                                                         int ny, const int* __restrict__ xs, int nx, int h, int w,
                                                         const float* __restrict__ wy, const float* __restrict__ wx,
                                                         const unsigned char* __restrict__ lut, float* __restrict__ logits,
                                                         unsigned char* __restrict__ mask, int nrg, int ncg, int vec_tiles, int vec_logits,
                                                         int vec_mask) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x;
    const int cg = b % ncg, rn = b / ncg, rg = rn % nrg, n = rn / nrg;
    const int y = rg * kBlendRows + wave;
    const int x = cg * kBlendCols + lane * kBlendLanePix;
    if (y >= H || x >= W) return;                              // (the kernel has no barrier)
    const int i0 = first_cover(ys, ny, h, y);                  // wave-uniform
    const int j0 = first_cover(xs, nx, w, x);                  // per lane: no tile before j0 reaches x, x + 1, ...
    const long long plane = (long long)h * w;
    float best[kBlendLanePix];
    int arg[kBlendLanePix];
#pragma unroll
    for (int e = 0; e < kBlendLanePix; ++e) { best[e] = 0.f; arg[e] = 0; }
    for (int c = 0; c < C; ++c) {
        float acc[kBlendLanePix], wsum[kBlendLanePix];
#pragma unroll
        for (int e = 0; e < kBlendLanePix; ++e) acc[e] = wsum[e] = 0.f;
        for (int i = i0; i < ny; ++i) {
            const int dy = y - ys[i];
            if (dy < 0) break;
            if (dy >= h) continue;
            const float fy = wy[dy];
            const float* trow = tiles + ((((long long)n * ny + i) * nx) * C + c) * plane + (long long)dy * w;
            for (int j = j0; j < nx; ++j) {
                const int x0 = xs[j];
                if (x0 > x + kBlendLanePix - 1) break;
                const float* row = trow + (long long)j * C * plane;
                if (vec_tiles && (x0 & 3) == 0) {              // x, x0 and w are multiples of 4: the lane's four pixels are inside the
                    const int dx = x - x0;                     // tile or outside it together, and 16-byte aligned in its row and in wx
                    if (dx < 0 || dx >= w) continue;
                    const float4 fx = *reinterpret_cast<const float4*>(wx + dx), v = *reinterpret_cast<const float4*>(row + dx);
                    const float f[kBlendLanePix] = {fx.x, fx.y, fx.z, fx.w}, u[kBlendLanePix] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int e = 0; e < kBlendLanePix; ++e) {
                        const float wt = fy * f[e];
                        const float p = wt * u[e];
                        acc[e] = acc[e] + p;
                        wsum[e] = wsum[e] + wt;
                    }
                    continue;
                }
#pragma unroll
                for (int e = 0; e < kBlendLanePix; ++e) {
                    const int dx = x + e - x0;
                    if (dx < 0 || dx >= w) continue;
                    const float wt = fy * wx[dx];                  // (plain operators: the pragma above governs them, one rounding each)
                    const float p = wt * row[dx];
                    acc[e] = acc[e] + p;
                    wsum[e] = wsum[e] + wt;
                }
            }
        }
        float out[kBlendLanePix];
#pragma unroll
        for (int e = 0; e < kBlendLanePix; ++e) {
            out[e] = acc[e] / wsum[e];                          // correctly rounded: hipcc's default for fp32 division
            if (c == 0 || out[e] > best[e]) { best[e] = out[e]; arg[e] = c; }      // ties to the lowest class, as egm_argmax_u8
        }
        if (logits) {
            float* o = logits + (((long long)n * C + c) * H + y) * W + x;
            if (vec_logits) {                                  // W % 4 == 0: the lane's four pixels are inside the row
                egm_u32x4 a;
                a.x = __float_as_uint(out[0]); a.y = __float_as_uint(out[1]); a.z = __float_as_uint(out[2]); a.w = __float_as_uint(out[3]);
                egm_store16_as<EGM_STORE_MODE>(o, a);
            } else {
#pragma unroll
                for (int e = 0; e < kBlendLanePix; ++e)
                    if (x + e < W) o[e] = out[e];
            }
        }
    }
    if (mask) {
        unsigned char* o = mask + ((long long)n * H + y) * W + x;
        unsigned int m[kBlendLanePix];
#pragma unroll
        for (int e = 0; e < kBlendLanePix; ++e) m[e] = lut ? lut[arg[e]] : (unsigned int)arg[e];
        if (vec_mask) {
            *reinterpret_cast<unsigned int*>(o) = m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24);
        } else {
#pragma unroll
            for (int e = 0; e < kBlendLanePix; ++e)
                if (x + e < W) o[e] = (unsigned char)m[e];
        }
    }
}

// the checks both entry points share; T = the plan's number of tiles
int tile_plan_check(const char* name, int N, int C, int H, int W, const void* ys, int ny, const void* xs, int nx, int h, int w, long long* T) {
    EGM_REQUIRE(ys && xs, "%s: null pointer (the tables of tile origins are required)", name);
    EGM_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "%s: bad shape N=%d C=%d H=%d W=%d", name, N, C, H, W);
    EGM_REQUIRE(H <= kTileMaxSide && W <= kTileMaxSide, "%s: %d x %d pixels, at most %d rows and columns are supported", name, H, W,
                kTileMaxSide);
    EGM_REQUIRE(ny > 0 && nx > 0 && h > 0 && w > 0 && h <= H && w <= W, "%s: bad plan: %d x %d tiles of %d x %d in an image of %d x %d", name,
                ny, nx, h, w, H, W);
    EGM_REQUIRE((long long)ny * h >= H && (long long)nx * w >= W,
                "%s: %d x %d tiles of %d x %d cannot cover %d x %d pixels (a stride above the window leaves gaps)", name, ny, nx, h, w, H, W);
    *T = (long long)N * ny * nx;
    EGM_REQUIRE(*T < (1ll << 31), "%s: %lld tiles, fewer than 2^31 are supported", name, *T);
    return EGM_OK;
}

}  // namespace

extern "C" int egm_tile_gather_f32(const float* src, int N, int C, int H, int W, const int* ys_dev, int ny, const int* xs_dev, int nx, int h,
                                   int w, int t0, int count, float* dst, egm_stream_t s) {
    const char* name = "tile_gather_f32";
    EGM_REQUIRE(src && dst, "%s: null pointer", name);
    long long T;
    const int rc = tile_plan_check(name, N, C, H, W, ys_dev, ny, xs_dev, nx, h, w, &T);
    if (rc != EGM_OK) return rc;
    EGM_REQUIRE(t0 >= 0 && t0 < T && count > 0, "%s: bad range: %d tiles from tile %d of %lld", name, count, t0, T);
    const long long rows = (long long)count * C * h;
    EGM_REQUIRE(rows < (1ll << 32), "%s: %lld rows in one call, fewer than 2^32 are supported", name, rows);
    const int vec = (w % kBlendLanePix == 0) && egm_aligned16(dst);
    hipLaunchKernelGGL(tile_gather_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)s, src, C, H, W, ys_dev, ny, xs_dev, nx,
                       h, w, (int)T, t0, rows, dst, vec);
    EGM_CHECK_LAUNCH("tile_gather_f32");
    return EGM_OK;
}

extern "C" int egm_tile_blend_f32(const float* tiles, int N, int C, int H, int W, const int* ys_dev, int ny, const int* xs_dev, int nx, int h,
                                  int w, const float* wy_dev, const float* wx_dev, const unsigned char* lut, float* logits_out,
                                  unsigned char* mask_out, egm_stream_t s) {
    const char* name = "tile_blend_f32";
    EGM_REQUIRE(tiles && wy_dev && wx_dev, "%s: null pointer (the tiles and both weight profiles are required)", name);
    EGM_REQUIRE(logits_out || mask_out, "%s: null pointer (no output: logits_out and mask_out are both NULL)", name);
    long long T;
    const int rc = tile_plan_check(name, N, C, H, W, ys_dev, ny, xs_dev, nx, h, w, &T);
    if (rc != EGM_OK) return rc;
    EGM_REQUIRE(!mask_out || C <= kTileMaxC, "%s: %d classes, a mask holds at most %d", name, C, kTileMaxC);
    const int nrg = egm_cdiv(H, kBlendRows), ncg = egm_cdiv(W, kBlendCols);
    const long long items = (long long)N * nrg * ncg;
    EGM_REQUIRE(items < (1ll << 31), "%s: %lld workgroups of %d x %d pixels, fewer than 2^31 are supported", name, items, kBlendRows, kBlendCols);
    const int vec_tiles = (w % kBlendLanePix == 0) && egm_aligned16(tiles) && egm_aligned16(wx_dev);
    const int vec_logits = logits_out && (W % kBlendLanePix == 0) && egm_aligned16(logits_out);
    const int vec_mask = mask_out && (W % kBlendLanePix == 0) && (reinterpret_cast<uintptr_t>(mask_out) & 3) == 0;
    hipLaunchKernelGGL(tile_blend_kernel, dim3((unsigned)items), dim3(256), 0, (hipStream_t)s, tiles, C, H, W, ys_dev, ny, xs_dev, nx, h, w,
                       wy_dev, wx_dev, lut, logits_out, mask_out, nrg, ncg, vec_tiles, vec_logits, vec_mask);
    EGM_CHECK_LAUNCH("tile_blend_f32");
    return EGM_OK;
}
