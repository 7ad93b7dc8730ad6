// Boundary IoU counts of uint8 masks at their own size: IoU restricted to the band of mask pixels within `radius` of
// the mask's contour (Cheng et al., CVPR 2021; mask_to_boundary = the mask minus its erosion by a (2 radius + 1)^2 box, zero outside).
//   egm_boundary_workspace: bytes of the two planes the row pass leaves for the column pass
//   egm_mask_boundary_u8:   bands of both sides (optionally written out, bit k = class k) and {inter, npred, ngt} per image and class
//
// A pixel has one class per side, so a box window full of class k is a window of ONE value: per side a single run length says
// everything, whatever C.  Two launches whatever the content:
//   rows    a wave walks a row in chunks of 1024 pixels (16 per lane, 16-byte loads).  start(p) = the column at which the run of equal
//           classes that holds p begins: a max-scan (each lane over its 16 pixels, one shuffle scan over the wave, a carry from chunk
//           to chunk).  The flag byte of column p gets bit k (pred) / bit 4 + k (label) when p's class is k and p - start(p) >= 2 radius,
//           i.e. when the window CENTRED at p - radius is full: the plane is written where the scan is (aligned 16-byte stores into
//           rows padded to a multiple of 16, zero behind W) and read radius columns to the right.  A second plane of the same layout
//           holds the pixel's own class bits (bit k / bit 4 + k), so the column pass needs neither the images nor the tables.
//   columns a wave owns 256 columns (4 per lane, one 4-byte word per plane and row) of kBoundaryRows rows and walks down from `radius`
//           rows above its chunk to `radius` rows below it: per column and side the row at which the flag nibble last changed.  Flag row r
//           decides image row r - radius: eroded iff the nibble is non-zero and has lasted 2 radius + 1 rows; the band of the four
//           columns is member & ~eroded on the word.  Band bytes are written if asked; counts stay in 32-bit registers per lane (at
//           most 4 * kBoundaryRows pixels), one shuffle reduction per cell, one 64-bit atomic per wave and cell.
// When 2 radius + 1 exceeds H or W nothing is eroded: the column pass then ignores the flags and walks its own rows only.
// No workgroup waits for another and no loop depends on the data.
// mask_scan.h holds what this file shares with contour.hip and surface.hip: the class tables, the column pass's tile and the host
// checks.
#include "common.h"
#include "mask_scan.h"

namespace {

constexpr int kBoundaryRows = 128;             // column pass: image rows per wave (tests/test_gpu_boundary.py restates it)
constexpr int kColUnroll = 8;                  //              rows loaded before any is used

// One side of the row pass for a lane's 16 pixels [p0, p0 + 16): cls = their classes, prev_cls / carry_start = the class of pixel
// p0 - 1 of the chunk before (256 in front of the row: equal to no class) and the latest run start so far.  -> bit (1 << class) per pixel
// whose run of equal classes reaches back 2 radius columns or more, in 16 bytes shifted left by `shift`; the carries move on.
__device__ __forceinline__ void row_side(const unsigned int (&cls)[kRowLanePix], int p0, int d2, int shift, unsigned int& prev_cls,
                                         int& carry_start, unsigned int (&out)[4], unsigned int (&mem)[4]) {
    const int lane = threadIdx.x & 63;
    unsigned int before = __shfl_up(cls[kRowLanePix - 1], 1, 64);
    if (lane == 0) before = prev_cls;
    int last = -1;                                             // the last run start among this lane's pixels
    {
        unsigned int q = before;
#pragma unroll
        for (int i = 0; i < kRowLanePix; ++i) { if (cls[i] != q) last = p0 + i; q = cls[i]; }
    }
    int inc = last;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc = max(inc, t);
    }
    int cur = __shfl_up(inc, 1, 64);
    if (lane == 0) cur = -1;
    cur = max(cur, carry_start);
    unsigned int q = before;
#pragma unroll
    for (int i = 0; i < kRowLanePix; ++i) {
        if (cls[i] != q) cur = p0 + i;
        q = cls[i];
        const unsigned int own = cls[i] < (unsigned)kBoundaryMaxC ? (1u << (cls[i] & 3u)) << shift : 0u;
        mem[i >> 2] |= own << (8 * (i & 3));
        out[i >> 2] |= (p0 + i - cur >= d2 ? own : 0u) << (8 * (i & 3));
    }
    carry_start = max(carry_start, __shfl(inc, 63, 64));
    prev_cls = __shfl(cls[kRowLanePix - 1], 63, 64);
}

// flags[row][p]: bit k = pred class k fills columns [p - 2 radius, p] of the row, bit 4 + k = the label's; member[row][p]: the class
// bits of pixel p itself; one wave per row
__global__ __launch_bounds__(256) void boundary_rows_kernel(const unsigned char* __restrict__ pred, const unsigned char* __restrict__ label,
                                                            long long nrows, int W, int pitch, int d2,
                                                            const unsigned char* __restrict__ pred_cls,
                                                            const unsigned char* __restrict__ label_cls, int C,
                                                            unsigned char* __restrict__ flags, unsigned char* __restrict__ member) {
    __shared__ unsigned char pt[256], lt[256];
    boundary_tables(pt, lt, pred_cls, label_cls, C);
    const int lane = threadIdx.x & 63;
    const long long row = blockIdx.x * 4LL + (threadIdx.x >> 6);
    if (row >= nrows) return;                                  // (a whole wave, behind the only barrier)
    const unsigned char* prow = pred + row * W;
    const unsigned char* lrow = label ? label + row * W : nullptr;
    unsigned char* frow = flags + row * pitch;
    unsigned char* mrow = member + row * pitch;
    unsigned int prev_p = 256u, prev_l = 256u;
    int start_p = -1, start_l = -1;
    for (int base = 0; base < pitch; base += kRowChunk) {
        const int p0 = base + lane * kRowLanePix;
        unsigned int cp[kRowLanePix], cl[kRowLanePix], out[4] = {0u, 0u, 0u, 0u}, mem[4] = {0u, 0u, 0u, 0u};
        row_classes(prow, p0, W, pt, cp);
        row_classes(lrow, p0, W, lt, cl);
        row_side(cp, p0, d2, 0, prev_p, start_p, out, mem);
        row_side(cl, p0, d2, 4, prev_l, start_l, out, mem);
        if (p0 < pitch) {
            *reinterpret_cast<uint4*>(frow + p0) = make_uint4(out[0], out[1], out[2], out[3]);
            *reinterpret_cast<uint4*>(mrow + p0) = make_uint4(mem[0], mem[1], mem[2], mem[3]);
        }
    }
}

// The bands of rows [y0, y0 + kBoundaryRows) x columns [x0, x0 + 256) of image n from the two planes of the row pass; one wave per item.
// Per column and side, begin = the row at which the flag nibble last changed; a non-zero nibble that has lasted 2 radius + 1 rows at
// flag row r erodes image row r - radius.  Four columns are one 4-byte word: band = member & ~eroded.
__global__ __launch_bounds__(256) void boundary_cols_kernel(int H, int W, int pitch, int radius, int dead, int C,
                                                            const unsigned char* __restrict__ flags, const unsigned char* __restrict__ member,
                                                            int nrc, int ncg, long long items, unsigned long long* __restrict__ counts,
                                                            unsigned char* __restrict__ band_pred, unsigned char* __restrict__ band_label) {
    const long long item = blockIdx.x * 4LL + (threadIdx.x >> 6);
    if (item >= items) return;                                 // (a whole wave; the kernel has no barrier)
    const ColTile tile(item, ncg, nrc, H, pitch, kBoundaryRows);  // (x0 may lie behind the pitch: load4_row and store4_row bound every access)
    const long long n = tile.n;
    const int x0 = tile.x0, y0 = tile.y0, yend = tile.yend;
    const int dv = dead ? 0 : radius, d2 = 2 * radius;         // (radius <= 2^29)
    const int rbeg = max(y0 - dv, 0), rend = yend + dv;        // flag rows walked; row r decides image row r - dv
    const unsigned char* fimg = flags + n * H * pitch;
    const unsigned char* mimg = member + n * H * pitch;
    unsigned int prevf = 0u, cnt[kBoundaryMaxC][3];
    int beg_p[kColLanePix], beg_l[kColLanePix];
#pragma unroll
    for (int j = 0; j < kColLanePix; ++j) beg_p[j] = beg_l[j] = rbeg;
#pragma unroll
    for (int k = 0; k < kBoundaryMaxC; ++k) cnt[k][0] = cnt[k][1] = cnt[k][2] = 0u;
    for (int r = rbeg; r < rend; r += kColUnroll) {
        unsigned int f[kColUnroll], mv[kColUnroll];
#pragma unroll
        for (int u = 0; u < kColUnroll; ++u) {
            const int rr = r + u, y = rr - dv;
            f[u] = mv[u] = 0u;
            if (rr >= rend) continue;
            if (!dead && rr < H) f[u] = load4_row(fimg + (long long)rr * pitch, x0 + radius, pitch);
            if (y >= y0) mv[u] = load4_row(mimg + (long long)y * pitch, x0, pitch);
        }
#pragma unroll
        for (int u = 0; u < kColUnroll; ++u) {
            const int rr = r + u, y = rr - dv;
            if (rr >= rend) continue;
            const unsigned int changed = f[u] ^ prevf;
            prevf = f[u];
#pragma unroll
            for (int j = 0; j < kColLanePix; ++j) {
                if ((changed >> (8 * j)) & 15u) beg_p[j] = rr;
                if ((changed >> (8 * j + 4)) & 15u) beg_l[j] = rr;
            }
            if (y < y0) continue;                              // still above the chunk: only the run lengths matter
            unsigned int lasted = 0u;                          // 0x0f / 0xf0 per column whose nibble has lasted 2 radius + 1 rows
#pragma unroll
            for (int j = 0; j < kColLanePix; ++j)
                lasted |= ((rr - beg_p[j] >= d2 ? 0x0fu : 0u) | (rr - beg_l[j] >= d2 ? 0xf0u : 0u)) << (8 * j);
            const unsigned int band = mv[u] & ~(f[u] & lasted);
            const unsigned int bp = band & 0x0f0f0f0fu, bl = (band >> 4) & 0x0f0f0f0fu;
#pragma unroll
            for (int k = 0; k < kBoundaryMaxC; ++k) {
                if (k >= C) break;
                const unsigned int m = 0x01010101u << k;
                cnt[k][0] += __popc(bp & bl & m);
                cnt[k][1] += __popc(bp & m);
                cnt[k][2] += __popc(bl & m);
            }
            if (band_pred) store4_row(band_pred + (n * H + y) * W, x0, W, bp);
            if (band_label) store4_row(band_label + (n * H + y) * W, x0, W, bl);
        }
    }
    if (!counts) return;
    for (int k = 0; k < C; ++k)
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const unsigned int v = wave_sum_u32(cnt[k][t]);    // at most 64 * 4 * kBoundaryRows
            if (tile.lane == 0 && v) atomicAdd(&counts[(n * C + k) * 3 + t], (unsigned long long)v);
        }
}

}  // namespace

extern "C" long long egm_boundary_workspace(int N, int H, int W) {
    if (mask_shape_check("boundary_workspace", N, H, W, 1) != EGM_OK) return EGM_ERR_ARG;      // (the planes do not depend on C)
    return 2LL * N * H * boundary_pitch(W) + 16;               // (two planes; +16: they start at the first 16-byte boundary)
}

extern "C" int egm_mask_boundary_u8(const unsigned char* pred, const unsigned char* label, int N, int H, int W, int radius,
                                    const unsigned char* pred_cls, const unsigned char* label_cls, int C, void* workspace,
                                    unsigned long long* counts, unsigned char* band_pred, unsigned char* band_label, egm_stream_t s) {
    MaskGrid g;
    if (mask_check("mask_boundary_u8", pred, pred_cls, workspace, N, H, W, C, kBoundaryRows, g) != EGM_OK) return EGM_ERR_ARG;
    EGM_REQUIRE(label ? label_cls != nullptr : (!counts && !band_label),
                "mask_boundary_u8: null pointer (a label needs its class table; without a label there are no counts and no label band)");
    EGM_REQUIRE(counts || band_pred || band_label, "mask_boundary_u8: null pointer (no output: counts, band_pred and band_label are all NULL)");
    EGM_REQUIRE(radius >= 1, "mask_boundary_u8: radius %d, at least 1 is required", radius);
    const int d = radius < (1 << 29) ? radius : (1 << 29);     // 2 d >= 2^30 >= H, W: as empty an erosion as any larger radius gives
    const int dead = (2LL * d + 1 > H || 2LL * d + 1 > W) ? 1 : 0;
    unsigned char* flags = mask_align(workspace);
    unsigned char* member = flags + g.nrows * g.pitch;
    hipLaunchKernelGGL(boundary_rows_kernel, g.row_blocks(), dim3(256), 0, (hipStream_t)s, pred, label, g.nrows, W, g.pitch, 2 * d, pred_cls,
                       label_cls, C, flags, member);
    EGM_CHECK_LAUNCH("mask_boundary_u8 (rows)");
    hipLaunchKernelGGL(boundary_cols_kernel, g.col_blocks(), dim3(256), 0, (hipStream_t)s, H, W, g.pitch, d, dead, C, flags, member, g.nrc, g.ncg,
                       g.items, counts, band_pred, band_label);
    EGM_CHECK_LAUNCH("mask_boundary_u8 (columns)");
    return EGM_OK;
}
