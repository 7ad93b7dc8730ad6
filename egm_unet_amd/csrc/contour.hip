// Contour scores of uint8 masks at their own size, all in integers: the Boundary IoU band under a EUCLIDEAN distance
// and the counts of the boundary F-measure.  Both ask one question per pixel: is there a pixel of a set S within distance r, i.e. is
// the pixel inside S dilated by a disc?  The disc is cut into rows: S reaches (y, x) iff for some |dy| <= r row y + dy has a pixel of S
// within w[|dy|] = isqrt(r^2 - dy^2) columns of x.
//   egm_contour_workspace        bytes of the planes the row passes leave for the column passes
//   egm_mask_boundary_euclid_u8  bands of both sides (optionally written out, bit k = class k) and {inter, npred, ngt} per image and class
//   egm_mask_contour_f_u8        contours of both sides (optionally written out) and {mp, |Kp|, mg, |Kg|} per image and class
// Two launches per call whatever the content, N, C and radius:
//   rows    a wave walks a row in chunks of 1024 pixels (16 per lane, 16-byte loads and stores) twice: left to right for the distance
//           to the nearest marked pixel at or before p (a max-scan of marked columns: each lane over its 16 pixels, one shuffle scan
//           over the wave, a carry from chunk to chunk), then right to left for the nearest at or after p (the mirrored min-scan); the
//           second sweep reads the first one's bytes back (each lane its own) and leaves g = min of the two, capped at 255 = "none".
//           band: a pixel has one class, so per side ONE plane whatever C: marks are the starts and ends of the runs of equal classes
//                 and g = the distance to the nearest pixel of the row (or the first column outside it) whose class differs from the
//                 pixel's own.  A third plane holds the classes of both sides (a nibble each, 15 = in no class).
//           F:    the contour bits of the pixel (4-neighbours, read from the rows above and below; bit k pred, bit 4 + k label) go to
//                 one plane, and per side and class one plane g = the distance to the nearest contour pixel of that class in the row.
//   columns a wave owns 256 columns (4 per lane, one 4-byte word per plane and row) of kContourRows rows.  Per group of kRowGroup
//           rows it walks the rows within r of the group inside the image once and ORs up "g <= w[|dy|]" for each row of the group and
//           the four columns at once: with the bytes spread over two words of 16-bit fields, bit 8 of (256 + w) - g says g <= w.  w
//           comes from a table in LDS that the prologue fills in integers; beyond r its entries never say "near".
//           band: row y + dy is near at once where its class differs from the pixel's own; rows outside the image are all "not k".
//           F:    only contour pixels ask, so a row group in which no lane holds a contour pixel of the class and side at hand is
//                 not walked (a wave-uniform skip).
//           Counts stay in 32-bit registers per lane (at most 4 * kContourRows pixels), one shuffle reduction per cell, one 64-bit
//           atomic per wave and non-zero cell.
// No workgroup waits for another; a wave never leaves its image: every row index is clamped to [0, H) of image n.
// mask_scan.h holds what this file shares with boundary.hip and surface.hip: the packed cells and the two scans of the row passes, the
// F row pass itself (contour_rows_kernel<8>; surface.hip runs it with 16-bit cells), the column passes' tile and the host checks.
#include "common.h"
#include "mask_scan.h"

namespace {

constexpr int kContourRows = 16;               // column passes: image rows per wave (tests/test_gpu_contour.py restates it)
constexpr int kContourMaxRadius = 254;         // a row distance fits a byte, 255 = none
static_assert(kContourRows % kRowGroup == 0, "a tile is a whole number of row groups");
constexpr unsigned int kOutside = 256u;        // the class of a column outside the row: equal to no class, the dropped one included

// a lane's 16 classes with kOutside behind the row's end
__device__ __forceinline__ void row_classes_outside(const unsigned char* row, int p0, int W, const unsigned char* tab,
                                                    unsigned int (&cls)[kRowLanePix]) {
    row_classes(row, p0, W, tab, cls);
    if (p0 + kRowLanePix > W) {
#pragma unroll
        for (int i = 0; i < kRowLanePix; ++i)
            if (p0 + i >= W) cls[i] = kOutside;
    }
}

// ---- band, rows: cls[row][p] = pred class | label class << 4 (15 = none, 0xff behind W); gp / gl[row][p] = the distance to the nearest
// column of the row whose class on that side differs from p's (column -1 and column W differ from everything), capped at 255
__global__ __launch_bounds__(256) void contour_band_rows_kernel(const unsigned char* __restrict__ pred, const unsigned char* __restrict__ label,
                                                                long long nrows, int W, int pitch,
                                                                const unsigned char* __restrict__ pred_cls,
                                                                const unsigned char* __restrict__ label_cls, int C,
                                                                unsigned char* __restrict__ cls_plane, unsigned char* __restrict__ gp_plane,
                                                                unsigned char* __restrict__ gl_plane) {
    __shared__ unsigned char pt[256], lt[256];
    boundary_tables(pt, lt, pred_cls, label_cls, C);
    const int lane = threadIdx.x & 63;
    const long long row = blockIdx.x * 4LL + (threadIdx.x >> 6);
    if (row >= nrows) return;                                  // (a whole wave, behind the only barrier)
    const unsigned char* prow = pred + row * W;
    const unsigned char* lrow = label ? label + row * W : nullptr;
    unsigned char* crow = cls_plane + row * pitch;
    unsigned char* grow[2] = {gp_plane + row * pitch, gl_plane + row * pitch};
    unsigned int edge_cls[2] = {kOutside, kOutside};           // the class next to the chunk, per side
    int carry[2] = {kNoMarkLeft, kNoMarkLeft};
    for (int base = 0; base < pitch; base += kRowChunk) {      // left to right: run starts
        const int p0 = base + lane * kRowLanePix;
        unsigned int c[2][kRowLanePix];
        Cells<8> both;
        row_classes_outside(prow, p0, W, pt, c[0]);
        row_classes_outside(lrow, p0, W, lt, c[1]);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            unsigned int q = __shfl_up(c[s][kRowLanePix - 1], 1, 64), marks = 0u;
            if (lane == 0) q = edge_cls[s];
#pragma unroll
            for (int i = 0; i < kRowLanePix; ++i) {
                marks |= (c[s][i] != q ? 1u : 0u) << i;
                q = c[s][i];
                both.put(i, (c[s][i] < (unsigned)kBoundaryMaxC ? c[s][i] : 15u) << (4 * s));
            }
            const Cells<8> g = dist_left<8>(marks, p0, 1, carry[s]);
            edge_cls[s] = __shfl(c[s][kRowLanePix - 1], 63, 64);
            if (p0 < pitch) g.store(grow[s] + p0);
        }
        if (p0 < pitch) both.store(crow + p0);
    }
    edge_cls[0] = edge_cls[1] = kOutside;
    carry[0] = carry[1] = kNoMarkRight;
    for (int base = ((pitch - 1) / kRowChunk) * kRowChunk; base >= 0; base -= kRowChunk) {     // right to left: run ends
        const int p0 = base + lane * kRowLanePix;
        unsigned int c[2][kRowLanePix];
        row_classes_outside(prow, p0, W, pt, c[0]);
        row_classes_outside(lrow, p0, W, lt, c[1]);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            unsigned int q = __shfl_down(c[s][0], 1, 64), marks = 0u;
            if (lane == 63) q = edge_cls[s];
#pragma unroll
            for (int i = kRowLanePix - 1; i >= 0; --i) {
                marks |= (c[s][i] != q ? 1u : 0u) << i;
                q = c[s][i];
            }
            Cells<8> g;
            if (p0 < pitch) g.load(grow[s] + p0);
            dist_right_min(marks, p0, 1, carry[s], g);
            edge_cls[s] = __shfl(c[s][0], 0, 64);
            if (p0 < pitch) g.store(grow[s] + p0);
        }
    }
}

// kw[j] = (256 + w[j]) in both 16-bit fields for j <= radius, w[j] = isqrt(radius^2 - j^2) by bits: (256 + w) - g has bit 8 set iff
// g <= w.  Beyond the radius (a row group walks up to kRowGroup - 1 rows more) 255 in both fields: 255 - g never has bit 8 set.
__device__ __forceinline__ void disc_table(unsigned int* kw, int radius) {
    const int j = threadIdx.x;
    unsigned int v = 0x00ff00ffu;
    if (j <= radius) {
        const int rest = radius * radius - j * j;
        int s = 0;
#pragma unroll
        for (int b = 128; b > 0; b >>= 1)
            if ((s | b) * (s | b) <= rest) s |= b;
        v = (256u + (unsigned int)s) * 0x00010001u;
    }
    kw[j] = v;
    if (j < kRowGroup) kw[256 + j] = 0x00ff00ffu;
    __syncthreads();
}

// bit 0 of byte j = column j is near, from the two ORed words of 16-bit fields (even and odd columns)
__device__ __forceinline__ unsigned int near_bytes(unsigned int near_e, unsigned int near_o) {
    return ((near_e >> 8) & 0x00010001u) | (((near_o >> 8) & 0x00010001u) << 8);
}

// ---- band, columns: rows [y0, y0 + kContourRows) x columns [x0, x0 + 256) of image n; one wave per item
__global__ __launch_bounds__(256) void contour_band_cols_kernel(int H, int W, int pitch, int radius, int C,
                                                                const unsigned char* __restrict__ cls_plane,
                                                                const unsigned char* __restrict__ gp_plane,
                                                                const unsigned char* __restrict__ gl_plane, int nrc, int ncg, long long items,
                                                                unsigned long long* __restrict__ counts, unsigned char* __restrict__ band_pred,
                                                                unsigned char* __restrict__ band_label) {
    __shared__ unsigned int kw[256 + kRowGroup];
    disc_table(kw, radius);
    const long long item = blockIdx.x * 4LL + (threadIdx.x >> 6);
    if (item >= items) return;                                 // (a whole wave, behind the only barrier)
    const ColTile tile(item, ncg, nrc, H, pitch, kContourRows);
    const long long n = tile.n, img = tile.img;
    const int x0 = tile.x0, y0 = tile.y0, yend = tile.yend;
    const bool live = tile.live;
    unsigned int cnt[kBoundaryMaxC][3];
#pragma unroll
    for (int k = 0; k < kBoundaryMaxC; ++k) cnt[k][0] = cnt[k][1] = cnt[k][2] = 0u;
    for (int y = y0; y < yend; y += kRowGroup) {               // rows y .. y + kRowGroup - 1 share one walk
        unsigned int own[kRowGroup], diff[kRowGroup], pe[kRowGroup], po[kRowGroup], le[kRowGroup], lod[kRowGroup];
#pragma unroll
        for (int j = 0; j < kRowGroup; ++j) {
            own[j] = (live && y + j < yend) ? *reinterpret_cast<const unsigned int*>(cls_plane + img + (long long)(y + j) * pitch) : 0xffffffffu;
            diff[j] = pe[j] = po[j] = le[j] = lod[j] = 0u;
        }
        const int lo = max(y - radius, 0), hi = min(y + kRowGroup - 1 + radius, H - 1);
        for (int yy = lo; yy <= hi; ++yy) {
            const long long at = img + (long long)yy * pitch;
            const unsigned int c = *reinterpret_cast<const unsigned int*>(cls_plane + at);
            const unsigned int gp = *reinterpret_cast<const unsigned int*>(gp_plane + at);
            const unsigned int gl = *reinterpret_cast<const unsigned int*>(gl_plane + at);
            const unsigned int gpe = gp & 0x00ff00ffu, gpo = (gp >> 8) & 0x00ff00ffu, gle = gl & 0x00ff00ffu, glo = (gl >> 8) & 0x00ff00ffu;
#pragma unroll
            for (int j = 0; j < kRowGroup; ++j) {
                const int dy = yy > y + j ? yy - (y + j) : y + j - yy;          // at most radius + kRowGroup - 1
                const unsigned int k2 = kw[dy], in_reach = dy <= radius ? 0xffffffffu : 0u;
                diff[j] |= (c ^ own[j]) & in_reach;
                pe[j] |= k2 - gpe;
                po[j] |= k2 - gpo;
                le[j] |= k2 - gle;
                lod[j] |= k2 - glo;
            }
        }
#pragma unroll
        for (int j = 0; j < kRowGroup; ++j) {
            const int yj = y + j;
            if (yj >= yend) break;
            const unsigned int frame = (yj - radius < 0 || yj + radius > H - 1) ? 0x01010101u : 0u;    // a row outside the image is in reach
            const unsigned int near_p = near_bytes(pe[j], po[j]) | ((((diff[j] & 0x0f0f0f0fu) + 0x0f0f0f0fu) >> 4) & 0x01010101u) | frame;
            const unsigned int near_l = near_bytes(le[j], lod[j]) | (((((diff[j] >> 4) & 0x0f0f0f0fu) + 0x0f0f0f0fu) >> 4) & 0x01010101u) | frame;
            unsigned int bp = 0u, bl = 0u;
#pragma unroll
            for (int i = 0; i < kColLanePix; ++i) {
                const unsigned int cp = (own[j] >> (8 * i)) & 15u, cl = (own[j] >> (8 * i + 4)) & 15u;
                if (cp < (unsigned)C && ((near_p >> (8 * i)) & 1u)) bp |= (1u << cp) << (8 * i);
                if (cl < (unsigned)C && ((near_l >> (8 * i)) & 1u)) bl |= (1u << cl) << (8 * i);
            }
#pragma unroll
            for (int k = 0; k < kBoundaryMaxC; ++k) {
                if (k >= C) break;
                const unsigned int m = 0x01010101u << k;
                cnt[k][0] += __popc(bp & bl & m);
                cnt[k][1] += __popc(bp & m);
                cnt[k][2] += __popc(bl & m);
            }
            if (band_pred) store4_row(band_pred + (n * H + yj) * W, x0, W, bp);
            if (band_label) store4_row(band_label + (n * H + yj) * W, x0, W, bl);
        }
    }
    if (!counts) return;
    for (int k = 0; k < C; ++k)
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const unsigned int v = wave_sum_u32(cnt[k][t]);    // at most 64 * 4 * kContourRows
            if (tile.lane == 0 && v) atomicAdd(&counts[(n * C + k) * 3 + t], (unsigned long long)v);
        }
}

// ---- F, rows: contour_rows_kernel<8> of mask_scan.h (255 = no contour pixel of the side and class within 254 columns)
// ---- F, columns: per contour pixel of side s and class k, is a contour pixel of the OTHER side's class k within the tolerance?
__global__ __launch_bounds__(256) void contour_f_cols_kernel(int H, int W, int pitch, int radius, int C, const unsigned char* __restrict__ contour,
                                                             const unsigned char* __restrict__ g_planes, long long plane, int nrc, int ncg,
                                                             long long items, unsigned long long* __restrict__ counts,
                                                             unsigned char* __restrict__ contour_pred, unsigned char* __restrict__ contour_label) {
    __shared__ unsigned int kw[256 + kRowGroup];
    disc_table(kw, radius);
    const long long item = blockIdx.x * 4LL + (threadIdx.x >> 6);
    if (item >= items) return;                                 // (a whole wave, behind the only barrier)
    const ColTile tile(item, ncg, nrc, H, pitch, kContourRows);
    const long long n = tile.n, img = tile.img;
    const int x0 = tile.x0, y0 = tile.y0, yend = tile.yend;
    const bool live = tile.live;
    unsigned int cnt[kBoundaryMaxC][4];
#pragma unroll
    for (int k = 0; k < kBoundaryMaxC; ++k) cnt[k][0] = cnt[k][1] = cnt[k][2] = cnt[k][3] = 0u;
    for (int y = y0; y < yend; y += kRowGroup) {               // rows y .. y + kRowGroup - 1 share one walk
        unsigned int kb[kRowGroup];
#pragma unroll
        for (int j = 0; j < kRowGroup; ++j) {
            kb[j] = (live && y + j < yend) ? *reinterpret_cast<const unsigned int*>(contour + img + (long long)(y + j) * pitch) : 0u;
            if (y + j < yend) {
                if (contour_pred) store4_row(contour_pred + (n * H + y + j) * W, x0, W, kb[j] & 0x0f0f0f0fu);
                if (contour_label) store4_row(contour_label + (n * H + y + j) * W, x0, W, (kb[j] >> 4) & 0x0f0f0f0fu);
            }
        }
        if (!counts) continue;
        const int lo = max(y - radius, 0), hi = min(y + kRowGroup - 1 + radius, H - 1);
#pragma unroll
        for (int k = 0; k < kBoundaryMaxC; ++k) {
            if (k >= C) break;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                unsigned int ask[kRowGroup], ne[kRowGroup], no[kRowGroup], any_ask = 0u;
#pragma unroll
                for (int j = 0; j < kRowGroup; ++j) {
                    ask[j] = (kb[j] >> (4 * s + k)) & 0x01010101u;
                    cnt[k][2 * s + 1] += __popc(ask[j]);
                    any_ask |= ask[j];
                    ne[j] = no[j] = 0u;
                }
                if (!__any(any_ask != 0u)) continue;           // no lane of the wave has such a pixel in these rows
                const unsigned char* g = g_planes + ((1 - s) * C + k) * plane + img;
                for (int yy = lo; yy <= hi; ++yy) {
                    const unsigned int gv = *reinterpret_cast<const unsigned int*>(g + (long long)yy * pitch);
                    const unsigned int ge = gv & 0x00ff00ffu, go = (gv >> 8) & 0x00ff00ffu;
#pragma unroll
                    for (int j = 0; j < kRowGroup; ++j) {
                        const unsigned int k2 = kw[yy > y + j ? yy - (y + j) : y + j - yy];      // (255s beyond the radius: never near)
                        ne[j] |= k2 - ge;
                        no[j] |= k2 - go;
                    }
                }
#pragma unroll
                for (int j = 0; j < kRowGroup; ++j) cnt[k][2 * s] += __popc(ask[j] & near_bytes(ne[j], no[j]));
            }
        }
    }
    if (!counts) return;
    for (int k = 0; k < C; ++k)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const unsigned int v = wave_sum_u32(cnt[k][t]);    // at most 64 * 4 * kContourRows
            if (tile.lane == 0 && v) atomicAdd(&counts[(n * C + k) * 4 + t], (unsigned long long)v);
        }
}

inline int contour_planes(int C) { return 2 * C + 1 > 3 ? 2 * C + 1 : 3; }      // F: contour + a g plane per side and class; band: 3

// mask_check, then the rules of this file's two entry points: one-sided calls and the radius; -> EGM_OK or EGM_ERR_ARG with the message set
int contour_args(const char* name, const void* pred, const void* label, int N, int H, int W, int radius, const void* pred_cls,
                 const void* label_cls, int C, const void* workspace, const void* counts, const void* out_pred, const void* out_label,
                 const char* what, MaskGrid& g) {
    if (mask_check(name, pred, pred_cls, workspace, N, H, W, C, kContourRows, g) != EGM_OK) return EGM_ERR_ARG;
    EGM_REQUIRE(label ? label_cls != nullptr : (!counts && !out_label),
                "%s: null pointer (a label needs its class table; without a label there are no counts and no label %s)", name, what);
    EGM_REQUIRE(counts || out_pred || out_label, "%s: null pointer (no output: counts and both %s outputs are NULL)", name, what);
    EGM_REQUIRE(radius >= 1 && radius <= kContourMaxRadius, "%s: radius %d, between 1 and %d are supported", name, radius, kContourMaxRadius);
    return EGM_OK;
}

}  // namespace

extern "C" long long egm_contour_workspace(int N, int H, int W, int C) {
    if (mask_shape_check("contour_workspace", N, H, W, C) != EGM_OK) return EGM_ERR_ARG;
    return (long long)contour_planes(C) * N * H * boundary_pitch(W) + 16;      // (+16: the planes start at the first 16-byte boundary)
}

extern "C" int egm_mask_boundary_euclid_u8(const unsigned char* pred, const unsigned char* label, int N, int H, int W, int radius,
                                           const unsigned char* pred_cls, const unsigned char* label_cls, int C, void* workspace,
                                           unsigned long long* counts, unsigned char* band_pred, unsigned char* band_label, egm_stream_t s) {
    MaskGrid g;
    const int rc = contour_args("mask_boundary_euclid_u8", pred, label, N, H, W, radius, pred_cls, label_cls, C, workspace, counts, band_pred,
                                band_label, "band", g);
    if (rc != EGM_OK) return rc;
    unsigned char* cls_plane = mask_align(workspace);
    unsigned char* gp_plane = cls_plane + g.nrows * g.pitch;
    unsigned char* gl_plane = gp_plane + g.nrows * g.pitch;
    hipLaunchKernelGGL(contour_band_rows_kernel, g.row_blocks(), dim3(256), 0, (hipStream_t)s, pred, label, g.nrows, W, g.pitch, pred_cls,
                       label_cls, C, cls_plane, gp_plane, gl_plane);
    EGM_CHECK_LAUNCH("mask_boundary_euclid_u8 (rows)");
    hipLaunchKernelGGL(contour_band_cols_kernel, g.col_blocks(), dim3(256), 0, (hipStream_t)s, H, W, g.pitch, radius, C, cls_plane, gp_plane,
                       gl_plane, g.nrc, g.ncg, g.items, counts, band_pred, band_label);
    EGM_CHECK_LAUNCH("mask_boundary_euclid_u8 (columns)");
    return EGM_OK;
}

extern "C" int egm_mask_contour_f_u8(const unsigned char* pred, const unsigned char* label, int N, int H, int W, int radius,
                                     const unsigned char* pred_cls, const unsigned char* label_cls, int C, void* workspace,
                                     unsigned long long* counts, unsigned char* contour_pred, unsigned char* contour_label, egm_stream_t s) {
    MaskGrid g;
    const int rc = contour_args("mask_contour_f_u8", pred, label, N, H, W, radius, pred_cls, label_cls, C, workspace, counts, contour_pred,
                                contour_label, "contour", g);
    if (rc != EGM_OK) return rc;
    const long long plane = g.nrows * g.pitch;
    unsigned char* contour = mask_align(workspace);
    unsigned char* g_planes = contour + plane;
    hipLaunchKernelGGL(contour_rows_kernel<8>, g.row_blocks(), dim3(256), 0, (hipStream_t)s, pred, label, g.nrows, H, W, g.pitch, pred_cls,
                       label_cls, C, counts ? 1 : 0, contour, g_planes);
    EGM_CHECK_LAUNCH("mask_contour_f_u8 (rows)");
    hipLaunchKernelGGL(contour_f_cols_kernel, g.col_blocks(), dim3(256), 0, (hipStream_t)s, H, W, g.pitch, radius, C, contour, g_planes, plane,
                       g.nrc, g.ncg, g.items, counts, contour_pred, contour_label);
    EGM_CHECK_LAUNCH("mask_contour_f_u8 (columns)");
    return EGM_OK;
}
