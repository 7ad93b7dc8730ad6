// Surface distances of uint8 masks at their own size, all in integers: for every contour pixel p of a side and class the
// exact squared Euclidean distance d2(p) = min |p - q|^2 over the contour pixels q of the OTHER side's same class, and per image, class
// and direction the statistics that the Hausdorff distance, its percentiles, the average surface distances and the surface Dice are
// made of.  The contour is contour.hip's (4-neighbours inside the image); nothing here is truncated: where contour.hip keeps a row
// distance in a byte and asks "within r?", this file keeps it in 16 bits (H, W <= 32767) and takes the minimum.
//   egm_surface_workspace     bytes of the planes the row pass leaves for the column pass
//   egm_mask_surface_dist_u8  counts [N][C][2][260] (n, sum of floor(256 d), sum of d2, max d2, 256 bins of ceil(d)) and the d2 maps
// Two launches per call whatever the content, N, C and the distances:
//   rows    contour_f_rows_kernel's shape: a wave walks a row in chunks of 1024 pixels twice, left to right and right to left (a scan
//           of marked columns per lane, one shuffle scan over the wave, a carry from chunk to chunk).  It leaves the contour bits of
//           the pixel (bit k pred, bit 4 + k label) in a byte plane and per side and class a 16-bit plane g = the distance to the
//           nearest contour pixel of that class in the row, 0xFFFF = the row has none.
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
#include "common.h"
#include "mask_scan.h"

namespace {

constexpr int kSurfaceRows = 16;               // column pass: image rows per wave (tests/test_gpu_surface.py restates it)
constexpr int kRowGroup = 4;                   //              rows that share one walk and its loads
static_assert(kSurfaceRows % kRowGroup == 0, "a tile is a whole number of row groups");
constexpr int kColLanePix = 4;                 // column pass: columns per lane
constexpr int kColWave = 64 * kColLanePix;     //              and per wave
constexpr int kSurfaceMaxSide = 32767;         // d2 < 2^31 and a row distance fits 16 bits beside 0xFFFF
constexpr int kSurfaceFields = 4 + 256;        // n, sum_q, sum_d2, max_d2, bins of ceil(d) (the last one: 255 or more)
constexpr unsigned int kNoRow = 0xFFFFu;       // g: no contour pixel in the row
constexpr unsigned int kNoDist = 0x7FFFFFFFu;  // g^2 of such a row: larger than every d2 (at most 2 * 32766^2), and + dy^2 fits 32 bits
constexpr int kNoMarkLeft = -(1 << 20);        // "no marked pixel so far": farther than 0xFFFF from every column >= 0
constexpr int kNoMarkRight = 1 << 22;          // the same to the right of every column of a padded row (W <= 32767)

// Distance from each of a lane's 16 pixels [p0, p0 + 16) to the nearest marked pixel at or left of it, capped at 0xFFFF, as 16
// halfwords.  marks: bit i = pixel p0 + i is marked.  carry = the last marked column of the chunks before, moved on.
__device__ __forceinline__ void dist_left16(unsigned int marks, int p0, int& carry, unsigned int (&out)[8]) {
    const int lane = threadIdx.x & 63;
    int inc = marks ? p0 + 31 - __clz((int)marks) : kNoMarkLeft;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc = max(inc, t);
    }
    int cur = __shfl_up(inc, 1, 64);
    if (lane == 0) cur = kNoMarkLeft;
    cur = max(cur, carry);
#pragma unroll
    for (int i = 0; i < kRowLanePix; ++i) {
        if ((marks >> i) & 1u) cur = p0 + i;
        out[i >> 1] |= (unsigned int)min(p0 + i - cur, (int)kNoRow) << (16 * (i & 1));
    }
    carry = max(carry, __shfl(inc, 63, 64));
}

// The mirror image: nearest marked pixel at or right of each pixel; io holds dist_left16's halfwords and leaves the smaller of the two.
__device__ __forceinline__ void dist_right_min16(unsigned int marks, int p0, int& carry, unsigned int (&io)[8]) {
    const int lane = threadIdx.x & 63;
    int inc = marks ? p0 + __ffs((int)marks) - 1 : kNoMarkRight;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_down(inc, o, 64);
        if (lane + o < 64) inc = min(inc, t);
    }
    int cur = __shfl_down(inc, 1, 64);
    if (lane == 63) cur = kNoMarkRight;
    cur = min(cur, carry);
    unsigned int res[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = kRowLanePix - 1; i >= 0; --i) {
        if ((marks >> i) & 1u) cur = p0 + i;
        const int left = (int)((io[i >> 1] >> (16 * (i & 1))) & 0xFFFFu);
        res[i >> 1] |= (unsigned int)min(min(cur - (p0 + i), (int)kNoRow), left) << (16 * (i & 1));
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) io[j] = res[j];
    carry = min(carry, __shfl(inc, 0, 64));
}

__device__ __forceinline__ void load32(const unsigned short* p, unsigned int (&v)[8]) {
    const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void store32(unsigned short* p, const unsigned int (&v)[8]) {
    reinterpret_cast<uint4*>(p)[0] = make_uint4(v[0], v[1], v[2], v[3]);
    reinterpret_cast<uint4*>(p)[1] = make_uint4(v[4], v[5], v[6], v[7]);
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned int wave_max_u32(unsigned int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned int)__shfl_xor((int)v, o, 64));
    return v;
}

// ---- rows: contour[row][p] = bit k: p is a contour pixel of pred class k, bit 4 + k: of label class k (0 behind W);
// g[s * C + k][row][p] = the distance to the nearest contour pixel of side s and class k in the row, 0xFFFF = none
__global__ __launch_bounds__(256) void surface_rows_kernel(const unsigned char* __restrict__ pred, const unsigned char* __restrict__ label,
                                                           long long nrows, int H, int W, int pitch,
                                                           const unsigned char* __restrict__ pred_cls,
                                                           const unsigned char* __restrict__ label_cls, int C,
                                                           unsigned char* __restrict__ contour, unsigned short* __restrict__ g_planes) {
    __shared__ unsigned char pt[256], lt[256];
    boundary_tables(pt, lt, pred_cls, label_cls, C);
    const int lane = threadIdx.x & 63;
    const long long row = blockIdx.x * 4LL + (threadIdx.x >> 6);
    if (row >= nrows) return;                                  // (a whole wave, behind the only barrier)
    const int y = (int)(row % H);
    const bool has_up = y > 0, has_dn = y + 1 < H;             // the neighbours above and below, inside this image only
    const unsigned char* rows[2] = {pred + row * W, label + row * W};
    const unsigned char* tabs[2] = {pt, lt};
    unsigned char* krow = contour + row * pitch;
    const long long plane = nrows * pitch;
    unsigned short* grow = g_planes + row * pitch;
    unsigned int left_cls[2] = {kNoClass, kNoClass};
    int carry[2 * kBoundaryMaxC];
#pragma unroll
    for (int t = 0; t < 2 * kBoundaryMaxC; ++t) carry[t] = kNoMarkLeft;
    for (int base = 0; base < pitch; base += kRowChunk) {      // left to right
        const int p0 = base + lane * kRowLanePix;
        unsigned int kbits[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            unsigned int c[kRowLanePix], up[kRowLanePix], dn[kRowLanePix];
            row_classes(rows[s], p0, W, tabs[s], c);
            row_classes(has_up ? rows[s] - W : nullptr, p0, W, tabs[s], up);
            row_classes(has_dn ? rows[s] + W : nullptr, p0, W, tabs[s], dn);
            unsigned int before = __shfl_up(c[kRowLanePix - 1], 1, 64), after = __shfl_down(c[0], 1, 64);
            if (lane == 0) before = left_cls[s];
            if (lane == 63) after = p0 + kRowLanePix < W ? (unsigned int)tabs[s][rows[s][p0 + kRowLanePix]] : kNoClass;
            left_cls[s] = __shfl(c[kRowLanePix - 1], 63, 64);
#pragma unroll
            for (int i = 0; i < kRowLanePix; ++i) {
                const int p = p0 + i;
                const unsigned int me = c[i], l = i ? c[i - 1] : before, r = i + 1 < kRowLanePix ? c[i + 1] : after;
                const bool edge = (p > 0 && l != me) || (p + 1 < W && r != me) || (has_up && up[i] != me) || (has_dn && dn[i] != me);
                if (me < (unsigned)kBoundaryMaxC && edge) kbits[i >> 2] |= (1u << me) << (8 * (i & 3) + 4 * s);
            }
        }
        if (p0 < pitch) *reinterpret_cast<uint4*>(krow + p0) = make_uint4(kbits[0], kbits[1], kbits[2], kbits[3]);
#pragma unroll
        for (int t = 0; t < 2 * kBoundaryMaxC; ++t) {          // bit t of the contour byte: side t / 4, class t % 4 -> plane side * C + class
            if ((t & 3) >= C) continue;
            unsigned int marks = 0u, g[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < kRowLanePix; ++i) marks |= ((kbits[i >> 2] >> (8 * (i & 3) + t)) & 1u) << i;
            dist_left16(marks, p0, carry[t], g);
            if (p0 < pitch) store32(grow + ((t >> 2) * C + (t & 3)) * plane + p0, g);
        }
    }
#pragma unroll
    for (int t = 0; t < 2 * kBoundaryMaxC; ++t) carry[t] = kNoMarkRight;
    for (int base = ((pitch - 1) / kRowChunk) * kRowChunk; base >= 0; base -= kRowChunk) {     // right to left
        const int p0 = base + lane * kRowLanePix;
        unsigned int kbits[4] = {0u, 0u, 0u, 0u};
        if (p0 < pitch) {
            const uint4 v = *reinterpret_cast<const uint4*>(krow + p0);
            kbits[0] = v.x; kbits[1] = v.y; kbits[2] = v.z; kbits[3] = v.w;
        }
#pragma unroll
        for (int t = 0; t < 2 * kBoundaryMaxC; ++t) {
            if ((t & 3) >= C) continue;
            unsigned short* gt = grow + ((t >> 2) * C + (t & 3)) * plane + p0;
            unsigned int marks = 0u, g[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < kRowLanePix; ++i) marks |= ((kbits[i >> 2] >> (8 * (i & 3) + t)) & 1u) << i;
            if (p0 < pitch) load32(gt, g);
            dist_right_min16(marks, p0, carry[t], g);
            if (p0 < pitch) store32(gt, g);
        }
    }
}

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
    const int lane = threadIdx.x & 63;
    const long long item = blockIdx.x * 4LL + (threadIdx.x >> 6);
    if (item >= items) return;                                 // (a whole wave; the kernel has no barrier)
    unsigned int* hist = hist_all[threadIdx.x >> 6];           // this wave's own bins: lane l zeroes and flushes bins 4 l .. 4 l + 3
    const int cg = (int)(item % ncg), rc = (int)((item / ncg) % nrc);
    const long long n = item / ncg / nrc;
    const int x0 = cg * kColWave + lane * kColLanePix;
    const bool live = x0 < pitch;                              // (pitch is a multiple of 16: a lane's columns are inside or outside as a whole)
    const int xl = live ? x0 : 0;
    const int y0 = rc * kSurfaceRows, yend = min(y0 + kSurfaceRows, H);
    const long long img = n * H * pitch + xl;
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

int surface_check(const void* pred, const void* label, int N, int H, int W, const void* pred_cls, const void* label_cls, int C,
                  const void* workspace, const void* counts, const void* d2_pred, const void* d2_label) {
    const char* name = "mask_surface_dist_u8";
    EGM_REQUIRE(pred && label && pred_cls && label_cls && workspace, "%s: null pointer (both images and both class tables are required)", name);
    EGM_REQUIRE(counts || d2_pred || d2_label, "%s: null pointer (no output: counts and both d2 maps are NULL)", name);
    EGM_REQUIRE(C > 0 && C <= kBoundaryMaxC, "%s: %d classes, between 1 and %d are supported", name, C, kBoundaryMaxC);
    EGM_REQUIRE(N > 0 && H > 0 && W > 0, "%s: bad shape %d x %d x %d", name, N, H, W);
    EGM_REQUIRE(H <= kSurfaceMaxSide && W <= kSurfaceMaxSide, "%s: %d x %d pixels, at most %d rows and columns are supported", name, H, W,
                kSurfaceMaxSide);
    EGM_REQUIRE((long long)H * W <= kBoundaryMaxPix, "%s: %d x %d pixels per image, at most 2^30 are supported", name, H, W);
    EGM_REQUIRE((long long)N * H <= (1ll << 31), "%s: %d images of %d rows in one call, at most 2^31 rows are supported", name, N, H);
    const long long items = (long long)N * egm_cdiv(H, kSurfaceRows) * egm_cdiv(W, kColWave);
    EGM_REQUIRE(items <= (1ll << 32), "%s: %lld tiles of %d x %d, at most 2^32 are supported", name, items, kSurfaceRows, kColWave);
    return EGM_OK;
}

}  // namespace

extern "C" long long egm_surface_workspace(int N, int H, int W, int C) {
    EGM_REQUIRE(N > 0 && H > 0 && W > 0, "surface_workspace: bad shape %d x %d x %d", N, H, W);
    EGM_REQUIRE(C > 0 && C <= kBoundaryMaxC, "surface_workspace: %d classes, between 1 and %d are supported", C, kBoundaryMaxC);
    EGM_REQUIRE(H <= kSurfaceMaxSide && W <= kSurfaceMaxSide, "surface_workspace: %d x %d pixels, at most %d rows and columns are supported", H, W,
                kSurfaceMaxSide);
    EGM_REQUIRE((long long)H * W <= kBoundaryMaxPix, "surface_workspace: %d x %d pixels per image, at most 2^30 are supported", H, W);
    return (long long)(1 + 4 * C) * N * H * boundary_pitch(W) + 16;            // (+16: the planes start at the first 16-byte boundary)
}

extern "C" int egm_mask_surface_dist_u8(const unsigned char* pred, const unsigned char* label, int N, int H, int W,
                                        const unsigned char* pred_cls, const unsigned char* label_cls, int C, void* workspace,
                                        unsigned long long* counts, int* d2_pred, int* d2_label, egm_stream_t s) {
    const int rc = surface_check(pred, label, N, H, W, pred_cls, label_cls, C, workspace, counts, d2_pred, d2_label);
    if (rc != EGM_OK) return rc;
    const long long nrows = (long long)N * H;
    const int pitch = boundary_pitch(W);
    const long long plane = nrows * pitch;
    unsigned char* contour = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(workspace) + 15) & ~(uintptr_t)15);
    unsigned short* g_planes = reinterpret_cast<unsigned short*>(contour + plane);              // (plane is a multiple of 16 bytes)
    const int nrc = egm_cdiv(H, kSurfaceRows), ncg = egm_cdiv(W, kColWave);
    const long long items = (long long)N * nrc * ncg;
    hipLaunchKernelGGL(surface_rows_kernel, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, (hipStream_t)s, pred, label, nrows, H, W, pitch,
                       pred_cls, label_cls, C, contour, g_planes);
    EGM_CHECK_LAUNCH("mask_surface_dist_u8 (rows)");
    hipLaunchKernelGGL(surface_cols_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, (hipStream_t)s, H, W, pitch, C, contour, g_planes,
                       plane, nrc, ncg, items, counts, d2_pred, d2_label);
    EGM_CHECK_LAUNCH("mask_surface_dist_u8 (columns)");
    return EGM_OK;
}
