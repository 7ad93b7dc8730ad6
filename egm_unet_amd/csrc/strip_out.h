// The frame of the "strip" kernels of tiles.hip and tta.hip: a lane owns kStripLanePix consecutive pixels of one row, a
// wave kStripCols columns of ONE row, a workgroup kStripRows rows; the classes of a pixel go by one at a time with a running best.
//   device  strip_pos (blockIdx.x -> image, row, first column), StripArgmax (the running best and the lut[arg] mask store), store_row4
//   host    the argument checks and the launch geometry of the blend and the merge (strip_check) and of the two row-per-wave kernels
// NO floating-point multiply, add or subtract may stand in this file, only compares, moves, integer arithmetic and stores: it is compiled
// under the default contracting mode, ahead of the .hip files' #pragma clang fp contract(off), and arithmetic written in a header was
// fused into FMAs.  The kernels hand finished values over.
#pragma once
#include "common.h"

namespace {

constexpr int kStripRows = 4;                          // rows per workgroup, one per wave (the GPU tests restate these two)
constexpr int kStripLanePix = 4;                       // consecutive pixels per lane
constexpr int kStripCols = 64 * kStripLanePix;         // columns per wave
constexpr int kStripMaxSide = 32767;                   // (a tap weight's numerator and denominator are exact in float32)
constexpr int kStripMaxC = 256;                        // a class index fits the mask's byte

// the lane's pixels: x .. x + kStripLanePix - 1 of row y of image n; outside: none of them is in the image (the kernels have no barrier)
struct StripPos { int n, y, x; bool outside; };
__device__ __forceinline__ StripPos strip_pos(int nrg, int ncg, int H, int W) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x;
    const int cg = b % ncg, rn = b / ncg, rg = rn % nrg, n = rn / nrg;
    const int y = rg * kStripRows + wave;
    const int x = cg * kStripCols + lane * kStripLanePix;
    return {n, y, x, y >= H || x >= W};
}

// four values of one row, o at the first of them: one 16-byte store (vec: the row length % 4 == 0 and the base aligned, so they are
// inside the row) or the dwords before column W
__device__ __forceinline__ void store_row4(float* o, const float (&out)[kStripLanePix], int x, int W, int vec) {
    if (vec) {
        egm_u32x4 a;
        a.x = __float_as_uint(out[0]); a.y = __float_as_uint(out[1]); a.z = __float_as_uint(out[2]); a.w = __float_as_uint(out[3]);
        egm_store16_as<EGM_STORE_MODE>(o, a);
    } else {
#pragma unroll
        for (int e = 0; e < kStripLanePix; ++e)
            if (x + e < W) o[e] = out[e];
    }
}

// the best class so far of the lane's pixels; ties go to the lowest class, as egm_argmax_u8.  take is per pixel so that a kernel calls it
// right behind the pixel's division: taking four values after four divisions compiles to another schedule
struct StripArgmax {
    float best[kStripLanePix] = {};
    int arg[kStripLanePix] = {};
    __device__ __forceinline__ void take(int c, int e, float v) {
        if (c == 0 || v > best[e]) { best[e] = v; arg[e] = c; }
    }
    // lut[arg] (arg without a lut) to o, the mask at the lane's first pixel: one packed store (vec: W % 4 == 0, the base 4-byte aligned)
    __device__ __forceinline__ void store_mask(unsigned char* o, const unsigned char* __restrict__ lut, int x, int W, int vec) const {
        unsigned int m[kStripLanePix];
#pragma unroll
        for (int e = 0; e < kStripLanePix; ++e) m[e] = lut ? lut[arg[e]] : (unsigned int)arg[e];
        if (vec) {
            *reinterpret_cast<unsigned int*>(o) = m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24);
        } else {
#pragma unroll
            for (int e = 0; e < kStripLanePix; ++e)
                if (x + e < W) o[e] = (unsigned char)m[e];
        }
    }
};

int strip_shape_check(const char* name, int N, int C, int H, int W) {
    EGM_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "%s: bad shape N=%d C=%d H=%d W=%d", name, N, C, H, W);
    EGM_REQUIRE(H <= kStripMaxSide && W <= kStripMaxSide, "%s: %d x %d pixels, at most %d rows and columns are supported", name, H, W,
                kStripMaxSide);
    return EGM_OK;
}

// the blend and the merge: a launch of `items` workgroups over [N][H][W]; vec_*: that output takes the vector store
struct StripGrid { int nrg, ncg, vec_logits, vec_mask; long long items; };
int strip_check(const char* name, int N, int C, int H, int W, const float* logits_out, const unsigned char* mask_out, StripGrid* g) {
    EGM_REQUIRE(logits_out || mask_out, "%s: null pointer (no output: logits_out and mask_out are both NULL)", name);
    const int rc = strip_shape_check(name, N, C, H, W);
    if (rc != EGM_OK) return rc;
    EGM_REQUIRE(!mask_out || C <= kStripMaxC, "%s: %d classes, a mask holds at most %d", name, C, kStripMaxC);
    const int nrg = egm_cdiv(H, kStripRows), ncg = egm_cdiv(W, kStripCols), vec = W % kStripLanePix == 0;
    const long long items = (long long)N * nrg * ncg;
    EGM_REQUIRE(items < (1ll << 31), "%s: %lld workgroups of %d x %d pixels, fewer than 2^31 are supported", name, items, kStripRows, kStripCols);
    *g = {nrg, ncg, logits_out && vec && egm_aligned16(logits_out), mask_out && vec && (reinterpret_cast<uintptr_t>(mask_out) & 3) == 0, items};
    return EGM_OK;
}

// the gather and the views: a launch of one wave per row of w floats at dst; vec: the rows take the vector store
struct StripRows { unsigned int groups; int vec; };
int strip_rows_check(const char* name, long long rows, int w, const float* dst, StripRows* g) {
    EGM_REQUIRE(rows < (1ll << 32), "%s: %lld rows in one call, fewer than 2^32 are supported", name, rows);
    *g = {(unsigned int)((rows + kStripRows - 1) / kStripRows), (w % kStripLanePix == 0) && egm_aligned16(dst)};
    return EGM_OK;
}

}  // namespace
