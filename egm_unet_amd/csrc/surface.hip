// Surface distances of uint8 masks at their own size, all in integers: for every contour pixel p of a side and class the
// exact squared Euclidean distance d2(p) = min |p - q|^2 over the contour pixels q of the OTHER side's same class, and per image, class
// and direction the statistics that the Hausdorff distance, its percentiles, the average surface distances and the surface Dice are
// made of.  The contour is contour.hip's (4-neighbours inside the image); nothing here is truncated: where contour.hip keeps a row
// distance in a byte and asks "within r?", this file keeps it in 16 bits (H, W <= 32767) and takes the minimum.
//   egm_surface_workspace     bytes of the planes the row pass leaves for the column pass
//   egm_mask_surface_dist_u8  counts [N][C][2][260] (n, sum of floor(256 d), sum of d2, max d2, 256 bins of ceil(d)) and the d2 maps
// Two launches per call whatever the content, N, C and the distances:
//   rows    contour_rows_kernel<16> of mask_scan.h, the row pass of contour.hip's F counts with 16-bit cells: a wave walks a row in
//           chunks of 1024 pixels twice, left to right and right to left (a scan of marked columns per lane, one shuffle scan over
//           the wave, a carry from chunk to chunk).  It leaves the contour bits of the pixel (bit k pred, bit 4 + k label) in a byte
//           plane and per side and class a 16-bit plane g = the distance to the nearest contour pixel of that class in the row,
//           0xFFFF = the row has none.
//   columns a wave owns 256 columns (4 per lane) of kSurfaceRows rows.  Per direction, class and group of kRowGroup rows in which some
//           lane holds an asking pixel (a wave-uniform skip otherwise) it walks the rows outwards from the group, dy = 0, 1, 2, ...
//           on both sides inside the image, and keeps best = min(dy^2 + g^2) per asking pixel.  Rows t or more away can only give
//           t^2 or more, so the walk ends when t^2 reaches the largest best of the wave (one ballot), and at the image's first and
//           last row at the latest: at most H steps, O(true distance) where the contours are close.  A pixel whose best is still
//           "none" then has no contour of the other side in its image and is counted in n only.
//           Statistics: n, the sums and the maximum stay in registers per lane, one shuffle reduction and one 64-bit atomic per wave
//           and non-zero cell; the histogram is collected in LDS (256 bins per wave: the four waves of a workgroup may be in
//           different images) and its non-zero bins are flushed once per direction and class.
// No workgroup waits for another and no wave waits for another wave; a wave never leaves its image: every row index is inside
// [0, H) of image n.
// mask_scan.h holds what this file shares with boundary.hip and contour.hip: the row pass, the column pass's tile and the host checks.
#include "common.h"
#include "mask_scan.h"

namespace {

constexpr int kSurfaceRows = 16;               // column pass: image rows per wave (tests/test_gpu_surface.py restates it)
static_assert(kSurfaceRows % kRowGroup == 0, "a tile is a whole number of row groups");
constexpr int kSurfaceMaxSide = 32767;         // d2 < 2^31 and a row distance fits 16 bits beside 0xFFFF
constexpr int kSurfaceFields = 4 + 256;        // n, sum_q, sum_d2, max_d2, bins of ceil(d) (the last one: 255 or more)
constexpr unsigned int kNoRow = Cells<16>::kCap;       // g: no contour pixel in the row (W <= 32767: no true distance reaches the cap)
constexpr unsigned int kNoDist = 0x7FFFFFFFu;  // g^2 of such a row: larger than every d2 (at most 2 * 32766^2), and + dy^2 fits 32 bits

// g^2 of a lane's four columns of one row (kNoDist where the row has no contour pixel), from the 8 bytes of its 16-bit plane
__device__ __forceinline__ void row_squares(const unsigned short* g, long long at, unsigned int (&sq)[kColLanePix]) {
    const uint2 v = *reinterpret_cast<const uint2*>(g + at);
    const unsigned int h[kColLanePix] = {v.x & 0xFFFFu, v.x >> 16, v.y & 0xFFFFu, v.y >> 16};
#pragma unroll
    for (int i = 0; i < kColLanePix; ++i) sq[i] = h[i] == kNoRow ? kNoDist : h[i] * h[i];
}

// floor(256 * sqrt(d2)) = isqrt(d2 << 16) for d2 < 2^31: a float seed (off by a few units at most), corrected in 64-bit integers
__device__ __forceinline__ unsigned int isqrt_q8(unsigned int d2) {
    const unsigned long long n = (unsigned long long)d2 << 16;
    unsigned long long q = (unsigned long long)(__fsqrt_rn((float)d2) * 256.0f);
    while (q * q > n) --q;
    while ((q + 1) * (q + 1) <= n) ++q;
    return (unsigned int)q;
}

// ---- columns: rows [y0, y0 + kSurfaceRows) x columns [x0, x0 + 256) of image n; one wave per item
__global__ __launch_bounds__(256) void surface_cols_kernel(int H, int W, int pitch, int C, const unsigned char* __restrict__ contour,
                                                           const unsigned short* __restrict__ g_planes, long long plane, int nrc, int ncg,
                                                           long long items, unsigned long long* __restrict__ counts,
                                                           int* __restrict__ d2_pred, int* __restrict__ d2_label) {
    __shared__ unsigned int hist_all[4][256];
    const long long item = blockIdx.x * 4LL + (threadIdx.x >> 6);
    if (item >= items) return;                                 // (a whole wave; the kernel has no barrier)
    unsigned int* hist = hist_all[threadIdx.x >> 6];           // this wave's own bins: lane l zeroes and flushes bins 4 l .. 4 l + 3
    const ColTile tile(item, ncg, nrc, H, pitch, kSurfaceRows);
    const long long n = tile.n, img = tile.img;
    const int lane = tile.lane, x0 = tile.x0, y0 = tile.y0, yend = tile.yend;
    const bool live = tile.live;
    int* maps[2] = {d2_pred, d2_label};
#pragma unroll
    for (int s = 0; s < 2; ++s) {                              // -1 everywhere first; the asking pixels overwrite their own below
        if (!maps[s] || !live) continue;
        for (int y = y0; y < yend; ++y) {
            int* row = maps[s] + (n * H + y) * W;
#pragma unroll
            for (int i = 0; i < kColLanePix; ++i)
                if (x0 + i < W) row[x0 + i] = -1;
        }
    }
    for (int ks = 0; ks < 2 * C; ++ks) {                       // direction s (0: pred asks label, 1: label asks pred), class k
        const int s = ks / C, k = ks - s * C;
        const unsigned short* g = g_planes + ((1 - s) * C + k) * plane;
        unsigned int cnt = 0u, dmax = 0u;
        unsigned long long sum_q = 0ull, sum_d2 = 0ull;
        if (counts) {
#pragma unroll
            for (int i = 0; i < 4; ++i) hist[4 * lane + i] = 0u;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");             // the zeroes before any lane's adds
            __builtin_amdgcn_wave_barrier();
        }
        for (int y = y0; y < yend; y += kRowGroup) {           // rows y .. y + kRowGroup - 1 share one walk
            unsigned int ask[kRowGroup], any_ask = 0u;
#pragma unroll
            for (int j = 0; j < kRowGroup; ++j) {
                const unsigned int kb = (live && y + j < yend) ? *reinterpret_cast<const unsigned int*>(contour + img + (long long)(y + j) * pitch) : 0u;
                ask[j] = (kb >> (4 * s + k)) & 0x01010101u;
                cnt += __popc(ask[j]);
                any_ask |= ask[j];
            }
            if (!__any(any_ask != 0u)) continue;               // no lane of the wave has such a pixel in these rows
            unsigned int best[kRowGroup][kColLanePix];         // 0 where nobody asks: it never holds the walk up
#pragma unroll
            for (int j = 0; j < kRowGroup; ++j)
#pragma unroll
                for (int i = 0; i < kColLanePix; ++i) best[j][i] = ((ask[j] >> (8 * i)) & 1u) ? 0xFFFFFFFFu : 0u;
#pragma unroll
            for (int jj = 0; jj < kRowGroup; ++jj) {           // the group's own rows: dy = |j - jj|
                if (y + jj >= yend) break;
                unsigned int sq[kColLanePix];
                row_squares(g, img + (long long)(y + jj) * pitch, sq);
#pragma unroll
                for (int j = 0; j < kRowGroup; ++j)
#pragma unroll
                    for (int i = 0; i < kColLanePix; ++i) best[j][i] = min(best[j][i], sq[i] + (unsigned int)((j - jj) * (j - jj)));
            }
            for (int t = 1; t < H; ++t) {                      // rows y - t and y + kRowGroup - 1 + t: dy >= t for every row of the group
                unsigned int lmax = 0u;
#pragma unroll
                for (int j = 0; j < kRowGroup; ++j)
#pragma unroll
                    for (int i = 0; i < kColLanePix; ++i) lmax = max(lmax, best[j][i]);
                const int ya = y - t, yb = y + kRowGroup - 1 + t;
                if (!__any((unsigned int)(t * t) < lmax) || (ya < 0 && yb >= H)) break;         // nothing nearer is left, or no row is
                if (ya >= 0) {
                    unsigned int sq[kColLanePix];
                    row_squares(g, img + (long long)ya * pitch, sq);
#pragma unroll
                    for (int j = 0; j < kRowGroup; ++j)
#pragma unroll
                        for (int i = 0; i < kColLanePix; ++i) best[j][i] = min(best[j][i], sq[i] + (unsigned int)((t + j) * (t + j)));
                }
                if (yb < H) {
                    unsigned int sq[kColLanePix];
                    row_squares(g, img + (long long)yb * pitch, sq);
#pragma unroll
                    for (int j = 0; j < kRowGroup; ++j)
#pragma unroll
                        for (int i = 0; i < kColLanePix; ++i)
                            best[j][i] = min(best[j][i], sq[i] + (unsigned int)((t + kRowGroup - 1 - j) * (t + kRowGroup - 1 - j)));
                }
            }
#pragma unroll
            for (int j = 0; j < kRowGroup; ++j)
#pragma unroll
                for (int i = 0; i < kColLanePix; ++i) {
                    const unsigned int d2 = best[j][i];
                    if (!((ask[j] >> (8 * i)) & 1u) || d2 >= kNoDist) continue;                 // not asking, or the other contour is empty
                    if (maps[s]) maps[s][(n * H + y + j) * W + x0 + i] = (int)d2;               // (an asking pixel is inside the image)
                    if (!counts) continue;
                    const unsigned int q = isqrt_q8(d2), r = q >> 8, up = r + (r * r < d2 ? 1u : 0u);
                    sum_q += q;
                    sum_d2 += d2;
                    dmax = max(dmax, d2);
                    atomicAdd(&hist[min(up, 255u)], 1u);
                }
        }
        if (!counts) continue;
        unsigned long long* cell = counts + ((n * C + k) * 2 + s) * kSurfaceFields;
        const unsigned int wn = wave_sum_u32(cnt), wmax = wave_max_u32(dmax);
        const unsigned long long wq = wave_sum_u64(sum_q), wd2 = wave_sum_u64(sum_d2);
        if (lane == 0) {
            if (wn) atomicAdd(&cell[0], (unsigned long long)wn);
            if (wq) atomicAdd(&cell[1], wq);
            if (wd2) atomicAdd(&cell[2], wd2);
            if (wmax) atomicMax(&cell[3], (unsigned long long)wmax);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // the wave's own LDS adds, before its lanes read the bins back
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned int v = hist[4 * lane + i];
            if (v) atomicAdd(&cell[4 + 4 * lane + i], (unsigned long long)v);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // ... and those reads before the next direction's zeroes
        __builtin_amdgcn_wave_barrier();
    }
}

// a row distance fits 16 bits beside 0xFFFF
inline int surface_side_check(const char* name, int H, int W) {
    EGM_REQUIRE(H <= kSurfaceMaxSide && W <= kSurfaceMaxSide, "%s: %d x %d pixels, at most %d rows and columns are supported", name, H, W,
                kSurfaceMaxSide);
    return EGM_OK;
}

}  // namespace

extern "C" long long egm_surface_workspace(int N, int H, int W, int C) {
    if (mask_shape_check("surface_workspace", N, H, W, C) != EGM_OK || surface_side_check("surface_workspace", H, W) != EGM_OK) return EGM_ERR_ARG;
    return (long long)(1 + 4 * C) * N * H * boundary_pitch(W) + 16;            // (+16: the planes start at the first 16-byte boundary)
}

extern "C" int egm_mask_surface_dist_u8(const unsigned char* pred, const unsigned char* label, int N, int H, int W,
                                        const unsigned char* pred_cls, const unsigned char* label_cls, int C, void* workspace,
                                        unsigned long long* counts, int* d2_pred, int* d2_label, egm_stream_t s) {
    const char* name = "mask_surface_dist_u8";
    MaskGrid g;
    if (mask_check(name, pred, pred_cls, workspace, N, H, W, C, kSurfaceRows, g) != EGM_OK || surface_side_check(name, H, W) != EGM_OK)
        return EGM_ERR_ARG;
    EGM_REQUIRE(label && label_cls, "%s: null pointer (both images and both class tables are required)", name);
    EGM_REQUIRE(counts || d2_pred || d2_label, "%s: null pointer (no output: counts and both d2 maps are NULL)", name);
    const long long plane = g.nrows * g.pitch;
    unsigned char* contour = mask_align(workspace);
    unsigned char* g_planes = contour + plane;                 // (plane is a multiple of 16 bytes)
    hipLaunchKernelGGL(contour_rows_kernel<16>, g.row_blocks(), dim3(256), 0, (hipStream_t)s, pred, label, g.nrows, H, W, g.pitch, pred_cls,
                       label_cls, C, 1, contour, g_planes);
    EGM_CHECK_LAUNCH("mask_surface_dist_u8 (rows)");
    hipLaunchKernelGGL(surface_cols_kernel, g.col_blocks(), dim3(256), 0, (hipStream_t)s, H, W, g.pitch, C, contour,
                       reinterpret_cast<const unsigned short*>(g_planes), plane, g.nrc, g.ncg, g.items, counts, d2_pred, d2_label);
    EGM_CHECK_LAUNCH("mask_surface_dist_u8 (columns)");
    return EGM_OK;
}
