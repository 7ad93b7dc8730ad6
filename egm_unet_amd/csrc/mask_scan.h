// What the mask passes of boundary.hip, contour.hip and surface.hip share.
//   rows     the byte -> class tables in LDS, a lane's 16 classes of a row from one 16-byte load, Cells<BITS> (a lane's 16 row distances,
//            packed), the two scans dist_left / dist_right_min over marked columns, and contour_rows_kernel<BITS>: the row pass of the
//            boundary F-measure (BITS = 8) and of the surface distances (BITS = 16)
//   columns  ColTile (which columns and rows of which image a wave owns) and row-bounded 4-byte accesses
//   host     the argument checks every entry point makes (mask_shape_check, mask_check), the launch geometry they imply (MaskGrid),
//            the padded row pitch and the alignment of the workspace planes
#pragma once
#include "common.h"

namespace {

constexpr int kBoundaryMaxC = 4;
constexpr unsigned int kNoClass = 255u;        // a byte that belongs to no class (table entry >= C), also the padding behind a row
constexpr int kRowLanePix = 16;                // row pass: pixels per lane
constexpr int kRowChunk = 64 * kRowLanePix;    //           and per wave and step
constexpr int kColLanePix = 4;                 // column pass: columns per lane
constexpr int kColWave = 64 * kColLanePix;     //              and per wave
constexpr int kRowGroup = 4;                   //              rows of a tile decided by one walk (contour.hip, surface.hip): they share its loads
// "No marked pixel so far" for the scans, to the left and to the right: farther than 0xFFFF, the largest cap, from every column of a
// padded row of at most 2^30 pixels (and from the up to 1023 columns behind it that a wave's last step covers), while every
// p - cur + add and cur - p + add stays below 2^31.
constexpr int kNoMarkLeft = -(1 << 20);
constexpr int kNoMarkRight = (1 << 30) + (1 << 17);

__device__ __forceinline__ unsigned int load4_any(const unsigned char* p) {
    unsigned int v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
// bytes [x0, x0 + 4) of a row of `width` bytes, 0 behind its end
__device__ __forceinline__ unsigned int load4_row(const unsigned char* row, int x0, int width) {
    if (x0 + 4 <= width) return load4_any(row + x0);
    unsigned int v = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (x0 + j < width) v |= (unsigned int)row[x0 + j] << (8 * j);
    return v;
}
__device__ __forceinline__ void store4_row(unsigned char* row, int x0, int width, unsigned int v) {
    if (x0 + 4 <= width) { __builtin_memcpy(row + x0, &v, 4); return; }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (x0 + j < width) row[x0 + j] = (unsigned char)(v >> (8 * j));
}

// byte -> class tables in LDS, kNoClass for a dropped byte (and for every byte of a side that is not there)
__device__ __forceinline__ void boundary_tables(unsigned char* pt, unsigned char* lt, const unsigned char* pred_cls, const unsigned char* label_cls,
                                                int C) {
    const unsigned int pc = pred_cls[threadIdx.x], lc = label_cls ? label_cls[threadIdx.x] : kNoClass;
    pt[threadIdx.x] = (unsigned char)(pc < (unsigned)C ? pc : kNoClass);
    lt[threadIdx.x] = (unsigned char)(lc < (unsigned)C ? lc : kNoClass);
    __syncthreads();
}

__device__ __forceinline__ void row_classes(const unsigned char* row, int p0, int W, const unsigned char* tab, unsigned int (&cls)[kRowLanePix]) {
    if (row && p0 + kRowLanePix <= W) {
        const uint4 v = load16_any(row + p0);
        const unsigned int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < kRowLanePix; ++i) cls[i] = tab[(w[i >> 2] >> (8 * (i & 3))) & 255u];
    } else {
#pragma unroll
        for (int i = 0; i < kRowLanePix; ++i) cls[i] = (row && p0 + i < W) ? (unsigned int)tab[row[p0 + i]] : kNoClass;
    }
}

// ---------------------------------------------------------------- rows: packed cells and the scans over marked columns
// A lane's 16 pixels of a row with BITS bits each, as the plane holds them: 16 or 32 bytes, moved with 16-byte vectors (the planes'
// rows are padded to 16 pixels and start at a 16-byte boundary).  kCap, the largest value, stands for "none".
template <int BITS>
struct Cells {
    static_assert(BITS == 8 || BITS == 16, "a cell is a byte or a halfword");
    static constexpr int kPerWord = 32 / BITS, kWords = kRowLanePix / kPerWord, kBytes = BITS / 8, kCap = (1 << BITS) - 1;
    unsigned int w[kWords];
    __device__ __forceinline__ Cells() {
#pragma unroll
        for (int j = 0; j < kWords; ++j) w[j] = 0u;
    }
    __device__ __forceinline__ unsigned int get(int i) const { return (w[i / kPerWord] >> (BITS * (i % kPerWord))) & (unsigned int)kCap; }
    __device__ __forceinline__ unsigned int bit(int i, int t) const { return (w[i / kPerWord] >> (BITS * (i % kPerWord) + t)) & 1u; }
    __device__ __forceinline__ void put(int i, unsigned int v) { w[i / kPerWord] |= v << (BITS * (i % kPerWord)); }    // ORed into the cell
    __device__ __forceinline__ void load(const unsigned char* p) {
#pragma unroll
        for (int j = 0; j < kWords; j += 4) {
            const uint4 v = *reinterpret_cast<const uint4*>(p + 4 * j);
            w[j] = v.x; w[j + 1] = v.y; w[j + 2] = v.z; w[j + 3] = v.w;
        }
    }
    __device__ __forceinline__ void store(unsigned char* p) const {
#pragma unroll
        for (int j = 0; j < kWords; j += 4) *reinterpret_cast<uint4*>(p + 4 * j) = make_uint4(w[j], w[j + 1], w[j + 2], w[j + 3]);
    }
};

// -> distance from each of a lane's 16 pixels [p0, p0 + 16) to the nearest marked pixel at or left of it, plus `add`, capped.
// marks: bit i = pixel p0 + i is marked.  carry = the last marked column of the chunks before, moved on.
template <int BITS>
__device__ __forceinline__ Cells<BITS> dist_left(unsigned int marks, int p0, int add, int& carry) {
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
    Cells<BITS> out;
#pragma unroll
    for (int i = 0; i < kRowLanePix; ++i) {
        if ((marks >> i) & 1u) cur = p0 + i;
        out.put(i, (unsigned int)min(p0 + i - cur + add, Cells<BITS>::kCap));
    }
    carry = max(carry, __shfl(inc, 63, 64));
    return out;
}

// The mirror image: nearest marked pixel at or right of each pixel; io holds dist_left's cells and leaves the smaller of the two.
// carry = the first marked column of the chunks to the right.
template <int BITS>
__device__ __forceinline__ void dist_right_min(unsigned int marks, int p0, int add, int& carry, Cells<BITS>& io) {
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
    Cells<BITS> res;
#pragma unroll
    for (int i = kRowLanePix - 1; i >= 0; --i) {
        if ((marks >> i) & 1u) cur = p0 + i;
        res.put(i, (unsigned int)min(min(cur - (p0 + i) + add, Cells<BITS>::kCap), (int)io.get(i)));
    }
    io = res;
    carry = min(carry, __shfl(inc, 0, 64));
}

// bit i = bit t of cell i
__device__ __forceinline__ unsigned int gather_bit(const Cells<8>& c, int t) {
    unsigned int marks = 0u;
#pragma unroll
    for (int i = 0; i < kRowLanePix; ++i) marks |= c.bit(i, t) << i;
    return marks;
}

// The row pass of the boundary F-measure and of the surface distances, one wave per row, which walks its row in chunks of 1024 pixels
// twice.  contour[row][p] = bit k: p is a contour pixel (4-neighbours inside the image) of pred class k, bit 4 + k: of label class k
// (0 behind W; label may be NULL: no such bits).  With want_g, g[s * C + k][row][p] = the distance to the nearest contour pixel of
// side s and class k in the row, Cells<BITS>::kCap = none that near, in planes of BITS / 8 bytes per pixel.
template <int BITS>
__global__ __launch_bounds__(256) void contour_rows_kernel(const unsigned char* __restrict__ pred, const unsigned char* __restrict__ label,
                                                           long long nrows, int H, int W, int pitch,
                                                           const unsigned char* __restrict__ pred_cls,
                                                           const unsigned char* __restrict__ label_cls, int C, int want_g,
                                                           unsigned char* __restrict__ contour, unsigned char* __restrict__ g_planes) {
    constexpr int kBytes = Cells<BITS>::kBytes;
    __shared__ unsigned char pt[256], lt[256];
    boundary_tables(pt, lt, pred_cls, label_cls, C);
    const int lane = threadIdx.x & 63;
    const long long row = blockIdx.x * 4LL + (threadIdx.x >> 6);
    if (row >= nrows) return;                                  // (a whole wave, behind the only barrier)
    const int y = (int)(row % H);
    const bool has_up = y > 0, has_dn = y + 1 < H;             // the neighbours above and below, inside this image only
    const unsigned char* rows[2] = {pred + row * W, label ? label + row * W : nullptr};
    const unsigned char* tabs[2] = {pt, lt};
    unsigned char* krow = contour + row * pitch;
    const long long plane = nrows * pitch * kBytes;
    unsigned char* grow = g_planes + row * pitch * kBytes;
    unsigned int left_cls[2] = {kNoClass, kNoClass};           // (never read at p == 0)
    int carry[2 * kBoundaryMaxC];
#pragma unroll
    for (int t = 0; t < 2 * kBoundaryMaxC; ++t) carry[t] = kNoMarkLeft;
    for (int base = 0; base < pitch; base += kRowChunk) {      // left to right
        const int p0 = base + lane * kRowLanePix;
        Cells<8> kbits;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            unsigned int c[kRowLanePix], up[kRowLanePix], dn[kRowLanePix];
            row_classes(rows[s], p0, W, tabs[s], c);
            row_classes(rows[s] && has_up ? rows[s] - W : nullptr, p0, W, tabs[s], up);
            row_classes(rows[s] && has_dn ? rows[s] + W : nullptr, p0, W, tabs[s], dn);
            unsigned int before = __shfl_up(c[kRowLanePix - 1], 1, 64), after = __shfl_down(c[0], 1, 64);
            if (lane == 0) before = left_cls[s];
            if (lane == 63) after = (rows[s] && p0 + kRowLanePix < W) ? (unsigned int)tabs[s][rows[s][p0 + kRowLanePix]] : kNoClass;
            left_cls[s] = __shfl(c[kRowLanePix - 1], 63, 64);
#pragma unroll
            for (int i = 0; i < kRowLanePix; ++i) {
                const int p = p0 + i;
                const unsigned int me = c[i], l = i ? c[i - 1] : before, r = i + 1 < kRowLanePix ? c[i + 1] : after;
                const bool edge = (p > 0 && l != me) || (p + 1 < W && r != me) || (has_up && up[i] != me) || (has_dn && dn[i] != me);
                if (me < (unsigned)kBoundaryMaxC && edge) kbits.put(i, (1u << me) << (4 * s));
            }
        }
        if (p0 < pitch) kbits.store(krow + p0);
        if (!want_g) continue;
#pragma unroll
        for (int t = 0; t < 2 * kBoundaryMaxC; ++t) {          // bit t of the contour byte: side t / 4, class t % 4 -> plane side * C + class
            if ((t & 3) >= C) continue;
            const Cells<BITS> g = dist_left<BITS>(gather_bit(kbits, t), p0, 0, carry[t]);
            if (p0 < pitch) g.store(grow + ((t >> 2) * C + (t & 3)) * plane + p0 * kBytes);
        }
    }
    if (!want_g) return;
#pragma unroll
    for (int t = 0; t < 2 * kBoundaryMaxC; ++t) carry[t] = kNoMarkRight;
    for (int base = ((pitch - 1) / kRowChunk) * kRowChunk; base >= 0; base -= kRowChunk) {     // right to left
        const int p0 = base + lane * kRowLanePix;
        Cells<8> kbits;
        if (p0 < pitch) kbits.load(krow + p0);
#pragma unroll
        for (int t = 0; t < 2 * kBoundaryMaxC; ++t) {
            if ((t & 3) >= C) continue;
            unsigned char* gt = grow + ((t >> 2) * C + (t & 3)) * plane + p0 * kBytes;
            Cells<BITS> g;
            if (p0 < pitch) g.load(gt);
            dist_right_min(gather_bit(kbits, t), p0, 0, carry[t], g);
            if (p0 < pitch) g.store(gt);
        }
    }
}

// ---------------------------------------------------------------- columns
// The tile of a column pass's work item: columns [x0, x0 + 4) of this lane and rows [y0, yend) of image n, one wave per item.  A lane
// whose columns lie behind the padded row (pitch is a multiple of 16: inside or outside as a whole) is not live and reads column 0
// instead; img = the lane's offset into a byte plane at row 0 of its image.
struct ColTile {
    int lane, x0, xl, y0, yend;
    bool live;
    long long n, img;
    __device__ __forceinline__ ColTile(long long item, int ncg, int nrc, int H, int pitch, int rows_per_wave) {
        const int cg = (int)(item % ncg), rc = (int)((item / ncg) % nrc);
        lane = threadIdx.x & 63;
        n = item / ncg / nrc;
        x0 = cg * kColWave + lane * kColLanePix;
        live = x0 < pitch;
        xl = live ? x0 : 0;
        y0 = rc * rows_per_wave;
        yend = min(y0 + rows_per_wave, H);
        img = n * H * pitch + xl;
    }
};

// (The {inter, npred, ngt} popcounts and the tail that adds a wave's counts to the caller's stay written out in each column kernel:
// handing the counter array to a helper, even an inlined one, changes how the compiler keeps it, and the Euclidean band's column
// pass measured 0.7 - 1.4 % slower for it)

// ---------------------------------------------------------------- host
constexpr long long kBoundaryMaxPix = 1ll << 30;
inline int boundary_pitch(int W) { return (W + 15) & ~15; }
// the planes start at the first 16-byte boundary of the workspace (the workspace sizes include the 16 bytes)
inline unsigned char* mask_align(void* workspace) {
    return reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(workspace) + 15) & ~(uintptr_t)15);
}

// what the workspace-size entry points check, and mask_check with them; -> EGM_OK or EGM_ERR_ARG with the message set
inline int mask_shape_check(const char* name, int N, int H, int W, int C) {
    EGM_REQUIRE(C > 0 && C <= kBoundaryMaxC, "%s: %d classes, between 1 and %d are supported", name, C, kBoundaryMaxC);
    EGM_REQUIRE(N > 0 && H > 0 && W > 0, "%s: bad shape %d x %d x %d", name, N, H, W);
    EGM_REQUIRE((long long)H * W <= kBoundaryMaxPix, "%s: %d x %d pixels per image, at most 2^30 are supported", name, H, W);
    return EGM_OK;
}

// the launch geometry of a rows / columns kernel pair: a wave per row, then a wave per tile of rows_per_wave x kColWave pixels
struct MaskGrid {
    long long nrows, items;
    int pitch, nrc, ncg;
    dim3 row_blocks() const { return dim3((unsigned)((nrows + 3) / 4)); }
    dim3 col_blocks() const { return dim3((unsigned)((items + 3) / 4)); }
};

// what all four entry points check before they launch, and the geometry that passed
inline int mask_check(const char* name, const void* pred, const void* pred_cls, const void* workspace, int N, int H, int W, int C,
                      int rows_per_wave, MaskGrid& g) {
    EGM_REQUIRE(pred && pred_cls && workspace, "%s: null pointer", name);
    if (mask_shape_check(name, N, H, W, C) != EGM_OK) return EGM_ERR_ARG;
    g.nrows = (long long)N * H;
    EGM_REQUIRE(g.nrows <= (1ll << 31), "%s: %d images of %d rows in one call, at most 2^31 rows are supported", name, N, H);
    g.pitch = boundary_pitch(W);
    g.nrc = egm_cdiv(H, rows_per_wave);
    g.ncg = egm_cdiv(W, kColWave);
    g.items = (long long)N * g.nrc * g.ncg;
    EGM_REQUIRE(g.items <= (1ll << 32), "%s: %lld tiles of %d x %d, at most 2^32 are supported", name, g.items, rows_per_wave, kColWave);
    return EGM_OK;
}

}  // namespace
