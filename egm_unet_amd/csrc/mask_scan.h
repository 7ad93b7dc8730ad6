// What the mask passes of boundary.hip and contour.hip share: the byte -> class tables in LDS, a lane's 16 classes of a row from one
// 16-byte load, unaligned and row-bounded 4-byte accesses, the wave sum and the padded row pitch of the workspace planes.
#pragma once
#include "common.h"

namespace {

constexpr int kBoundaryMaxC = 4;
constexpr unsigned int kNoClass = 255u;        // a byte that belongs to no class (table entry >= C), also the padding behind a row
constexpr int kRowLanePix = 16;                // row pass: pixels per lane
constexpr int kRowChunk = 64 * kRowLanePix;    //           and per wave and step

__device__ __forceinline__ unsigned int wave_sum_u32(unsigned int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint4 load16_any(const unsigned char* p) {
    uint4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}
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

constexpr long long kBoundaryMaxPix = 1ll << 30;
inline int boundary_pitch(int W) { return (W + 15) & ~15; }

}  // namespace
