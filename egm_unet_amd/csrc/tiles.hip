// Sliding-window inference: cut an fp32 NCHW batch into overlapping windows, and blend the windows' logits back with a
// separable weight that fades towards the window's edge.
//   egm_tile_gather_f32  dst[k] = tile min(t0 + k, T - 1) of src, one launch whatever count is
//   egm_tile_blend_f32   out = sum_t wt_t * tile_t / sum_t wt_t per pixel over the tiles that cover it, and / or lut[argmax_c out]
// Tile t = (n * ny + i) * nx + j covers rows ys[i] .. ys[i] + h - 1 and columns xs[j] .. xs[j] + w - 1 of image n; ys and xs ascend.
// The blend is a gather: a lane owns kStripLanePix consecutive pixels of one row and visits the tiles that cover each of them in
// ascending t (i outside, j inside).  No atomics and no lane depends on another, so the result does not depend on scheduling.  The
// arithmetic is fixed so that a numpy float32 restatement gives the same bits (tests/tile_oracle.py): wt = wy * wx, p = wt * v,
// acc = acc + p, wsum = wsum + wt, one rounding each and no contraction into an FMA, then one correctly rounded division.
//   shape   a wave owns kStripCols columns of ONE row, a workgroup kStripRows rows (strip_out.h, the frame shared with tta.hip): the row
//           range of covering tiles is wave-uniform (a scalar loop), the column range differs per lane (a divergent loop, two tiles at
//           the usual overlap).  The classes are the outermost loop with a running best, so C costs no registers.
//   memory  T*C*h*w*4 bytes read once or (in the overlaps) a few times from neighbouring workgroups, N*C*H*W*4 (+ N*H*W) written once:
//           the logits leave as 16-byte non-temporal stores where W % 4 == 0 and the base is aligned (common.h, EGM_STORE_MODE),
//           else as dwords.  A tile row starts at any x0: where x0 and w are multiples of 4 (window 480 at overlap 0.25: every tile
//           but a clamped last one) the lane's four pixels are one 16-byte load of the tile and one of wx, else dwords (consecutive
//           lanes, consecutive addresses).  Both forms do the same arithmetic per pixel.
// Every tile read is at (t, c, y - y0, x - x0) with 0 <= y - y0 < h and 0 <= x - x0 < w checked in the kernel: inside [T][C][h][w]
// whatever the tables hold.  The gather clamps a tile's origin into the image for the same reason.
#include "strip_out.h"

// No multiply of this file may be fused with the add behind it.  The pragma governs the operators written below it; the __fmul_rn /
// __fadd_rn wrappers are plain operators inside a header compiled under the default (contracting) mode, and were fused.  So strip_out.h
// (the lane's pixels, the running argmax, the stores, the entry points' geometry) holds no arithmetic on samples: wt * v, acc + p and
// acc / wsum stay here, below the pragma.
#pragma clang fp contract(off)

namespace {

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
    const long long row = blockIdx.x * (long long)kStripRows + wave;   // row r of class c of dst[k]
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
    for (int x = lane * kStripLanePix; x < w; x += kStripCols) {
        float out[kStripLanePix];
        if (vec) {                                             // w % 4 == 0 and dst aligned: the lane's four columns are inside
            float4 v;
            if (wide) v = *reinterpret_cast<const float4*>(s + x);
            else v = make_float4(s[x], s[x + 1], s[x + 2], s[x + 3]);
            out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
            store_row4(d + x, out, x, w, 1);                   // (a store per branch compiles closest to the loop as it was: DESIGN.md 6.26)
        } else {
#pragma unroll
            for (int e = 0; e < kStripLanePix; ++e) out[e] = x + e < w ? s[x + e] : 0.f;
            store_row4(d + x, out, x, w, 0);
        }
    }
}

__global__ __launch_bounds__(256) void tile_blend_kernel(const float* __restrict__ tiles, int C, int H, int W, const int* __restrict__ ys,
                                                         int ny, const int* __restrict__ xs, int nx, int h, int w,
                                                         const float* __restrict__ wy, const float* __restrict__ wx,
                                                         const unsigned char* __restrict__ lut, float* __restrict__ logits,
                                                         unsigned char* __restrict__ mask, int nrg, int ncg, int vec_tiles, int vec_logits,
                                                         int vec_mask) {
    const auto [n, y, x, outside] = strip_pos(nrg, ncg, H, W);
    if (outside) return;
    const int i0 = first_cover(ys, ny, h, y);                  // wave-uniform
    const int j0 = first_cover(xs, nx, w, x);                  // per lane: no tile before j0 reaches x, x + 1, ...
    const long long plane = (long long)h * w;
    StripArgmax top;
    for (int c = 0; c < C; ++c) {
        float acc[kStripLanePix], wsum[kStripLanePix];
#pragma unroll
        for (int e = 0; e < kStripLanePix; ++e) acc[e] = wsum[e] = 0.f;
        for (int i = i0; i < ny; ++i) {
            const int dy = y - ys[i];
            if (dy < 0) break;
            if (dy >= h) continue;
            const float fy = wy[dy];
            const float* trow = tiles + ((((long long)n * ny + i) * nx) * C + c) * plane + (long long)dy * w;
            for (int j = j0; j < nx; ++j) {
                const int x0 = xs[j];
                if (x0 > x + kStripLanePix - 1) break;
                const float* row = trow + (long long)j * C * plane;
                if (vec_tiles && (x0 & 3) == 0) {              // x, x0 and w are multiples of 4: the lane's four pixels are inside the
                    const int dx = x - x0;                     // tile or outside it together, and 16-byte aligned in its row and in wx
                    if (dx < 0 || dx >= w) continue;
                    const float4 fx = *reinterpret_cast<const float4*>(wx + dx), v = *reinterpret_cast<const float4*>(row + dx);
                    const float f[kStripLanePix] = {fx.x, fx.y, fx.z, fx.w}, u[kStripLanePix] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int e = 0; e < kStripLanePix; ++e) {
                        const float wt = fy * f[e];
                        const float p = wt * u[e];
                        acc[e] = acc[e] + p;
                        wsum[e] = wsum[e] + wt;
                    }
                    continue;
                }
#pragma unroll
                for (int e = 0; e < kStripLanePix; ++e) {
                    const int dx = x + e - x0;
                    if (dx < 0 || dx >= w) continue;
                    const float wt = fy * wx[dx];                  // (plain operators: the pragma above governs them, one rounding each)
                    const float p = wt * row[dx];
                    acc[e] = acc[e] + p;
                    wsum[e] = wsum[e] + wt;
                }
            }
        }
        float out[kStripLanePix];
#pragma unroll
        for (int e = 0; e < kStripLanePix; ++e) {
            out[e] = acc[e] / wsum[e];                          // correctly rounded: hipcc's default for fp32 division
            top.take(c, e, out[e]);
        }
        if (logits) store_row4(logits + (((long long)n * C + c) * H + y) * W + x, out, x, W, vec_logits);
    }
    if (mask) top.store_mask(mask + ((long long)n * H + y) * W + x, lut, x, W, vec_mask);
}

// the checks both entry points share; T = the plan's number of tiles
int tile_plan_check(const char* name, int N, int C, int H, int W, const void* ys, int ny, const void* xs, int nx, int h, int w, long long* T) {
    EGM_REQUIRE(ys && xs, "%s: null pointer (the tables of tile origins are required)", name);
    const int rc = strip_shape_check(name, N, C, H, W);
    if (rc != EGM_OK) return rc;
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
    int rc = tile_plan_check(name, N, C, H, W, ys_dev, ny, xs_dev, nx, h, w, &T);
    if (rc != EGM_OK) return rc;
    EGM_REQUIRE(t0 >= 0 && t0 < T && count > 0, "%s: bad range: %d tiles from tile %d of %lld", name, count, t0, T);
    const long long rows = (long long)count * C * h;
    StripRows g;
    if ((rc = strip_rows_check(name, rows, w, dst, &g)) != EGM_OK) return rc;
    hipLaunchKernelGGL(tile_gather_kernel, dim3(g.groups), dim3(256), 0, (hipStream_t)s, src, C, H, W, ys_dev, ny, xs_dev, nx, h, w, (int)T, t0,
                       rows, dst, g.vec);
    EGM_CHECK_LAUNCH("tile_gather_f32");
    return EGM_OK;
}

extern "C" int egm_tile_blend_f32(const float* tiles, int N, int C, int H, int W, const int* ys_dev, int ny, const int* xs_dev, int nx, int h,
                                  int w, const float* wy_dev, const float* wx_dev, const unsigned char* lut, float* logits_out,
                                  unsigned char* mask_out, egm_stream_t s) {
    const char* name = "tile_blend_f32";
    EGM_REQUIRE(tiles && wy_dev && wx_dev, "%s: null pointer (the tiles and both weight profiles are required)", name);
    StripGrid g;
    long long T;
    int rc = strip_check(name, N, C, H, W, logits_out, mask_out, &g);
    if (rc == EGM_OK) rc = tile_plan_check(name, N, C, H, W, ys_dev, ny, xs_dev, nx, h, w, &T);
    if (rc != EGM_OK) return rc;
    const int vec_tiles = (w % kStripLanePix == 0) && egm_aligned16(tiles) && egm_aligned16(wx_dev);
    hipLaunchKernelGGL(tile_blend_kernel, dim3((unsigned)g.items), dim3(256), 0, (hipStream_t)s, tiles, C, H, W, ys_dev, ny, xs_dev, nx, h, w,
                       wy_dev, wx_dev, lut, logits_out, mask_out, g.nrg, g.ncg, vec_tiles, g.vec_logits, g.vec_mask);
    EGM_CHECK_LAUNCH("tile_blend_f32");
    return EGM_OK;
}
