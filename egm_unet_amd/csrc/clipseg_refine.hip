// CLIPSeg refined decoder head, complex_trans_conv=True (models/clipseg.py:401-414):
//   Conv2d(rd, rd, 3, padding 1) -> ReLU -> ConvTranspose2d(rd, rd/2, 4, stride 4) -> ReLU -> ConvTranspose2d(rd/2, 1, 4, stride 4)
// on the g x g token grid of the decoder output a [B][Ltot][rd] (tok_off leading tokens, the class token, skipped).
// Both transposed convolutions have kernel == stride, so token (ty, tx) owns the disjoint 16 x 16 output patch at (16 ty, 16 tx):
//   h      = relu(b0 + conv3x3(a)[ty, tx])                         rd values; the only step that reads neighbouring tokens
//   z[p]   = relu(b1 + W1[:, :, p]^T h)                            p = (i1, j1), 16 positions x rd/2; never written to memory
//   out    = b2 + W2[:, q]^T z[p]  at (16 ty + 4 i1 + i2, 16 tx + 4 j1 + j2),  q = (i2, j2)
// Forward: ONE launch, a workgroup per (image, token row), writing 16 whole output rows.  Backward: three launches
//   1. dh (masked by h > 0) per token row  ||  per-(position, token slice) slabs of dW1, db1, dW2, db2 (z recomputed from h)
//   2. da per token row (3x3 with flipped taps)  ||  per-(tap, token slice) slabs of dW0 (+ db0)
//   3. the slab sums in fixed slice order (bitwise reproducible, no atomics)
// The products run on the vector ALU with fp32 accumulation; in the bf16 path h and z are rounded to bf16 before the next product.
#include "common.h"

namespace {

constexpr int NT = 256;        // threads per workgroup
constexpr int GMAX = 32;       // largest token grid side
constexpr int TC = 16;         // tokens per chunk of the per-token products

template <typename T> __device__ __forceinline__ float rnd(float x) { return to_f32(from_f32<T>(x)); }

// packed operand image (elements, in the activation dtype), see egm_refine_pack
__host__ __device__ constexpr long long off_w0f(int rd) { return 0; }
__host__ __device__ constexpr long long off_w0d(int rd) { return 9LL * rd * rd; }
__host__ __device__ constexpr long long off_w1f(int rd) { return 18LL * rd * rd; }
__host__ __device__ constexpr long long off_w1d(int rd) { return 26LL * rd * rd; }
__host__ __device__ constexpr long long off_w2(int rd) { return 34LL * rd * rd; }
__host__ __device__ constexpr long long packed_elems(int rd) { return 34LL * rd * rd + 8LL * rd; }

// backward slabs per token slice: S = number of slices, a slice = TPS tokens (a multiple of TC)
struct Slices { int S, tps; };
static inline Slices slices_for(long long T) {
    long long S = (T + 255) / 256;
    if (S > 32) S = 32;
    if (S < 1) S = 1;
    long long tps = (T + S - 1) / S;
    tps = (tps + TC - 1) / TC * TC;
    return Slices{(int)((T + tps - 1) / tps), (int)tps};
}
__host__ __device__ constexpr long long slab1_elems(int rd) { return (long long)rd * (rd / 2) + rd / 2 + (rd / 2) * 16 + 16; }
struct WsLayout { long long dh, s0, sb0, s1, total; };       // float offsets into the workspace
static inline WsLayout ws_layout(int B, int g, int rd) {
    const long long T = (long long)B * g * g;
    const Slices sl = slices_for(T);
    WsLayout w;
    w.dh = 0;
    w.s0 = (T * rd + 63) / 64 * 64;
    w.sb0 = w.s0 + (long long)sl.S * 9 * rd * rd;
    w.s1 = w.sb0 + (long long)sl.S * rd;
    w.total = w.s1 + (long long)sl.S * 16 * slab1_elems(rd);
    return w;
}

// ---- 3x3 conv of one token row --------------------------------------------------------------------------------------------
// src element (b, y, x, c) at src[(b*Ltot + tok_off + y*g + x)*RD + c]; xs [3][GMAX+2][RD] fp32 gets rows ty-1..ty+1 with a zero halo.
template <typename TI, int RD>
__device__ __forceinline__ void stage_rows(const TI* __restrict__ src, int tok_off, int Ltot, int b, int ty, int g, float* xs) {
    const int n = 3 * (g + 2) * RD;
    for (int i = threadIdx.x; i < n; i += NT) {
        const int c = i % RD, xx = (i / RD) % (g + 2), r = i / (RD * (g + 2));
        const int y = ty + r - 1, x = xx - 1;
        float v = 0.f;
        if (y >= 0 && y < g && x >= 0 && x < g) v = to_f32(src[((long long)b * Ltot + tok_off + y * g + x) * RD + c]);
        xs[(r * (GMAX + 2) + xx) * RD + c] = v;
    }
}
// acc[k] = sum_{tap, c} w[(tap*RD + c)*RD + co] * xs[tap_y][tx + tap_x][c] for co = tid % RD, tx = tid / RD + k * (NT / RD) < g
template <typename TW, int RD>
__device__ __forceinline__ void conv3x3_row(const float* xs, const TW* __restrict__ w, int g, float (&acc)[GMAX * RD / NT]) {
    constexpr int NG = NT / RD, MAXT = GMAX / NG;
    const int co = threadIdx.x % RD, grp = threadIdx.x / RD;
#pragma unroll
    for (int k = 0; k < MAXT; ++k) acc[k] = 0.f;
    for (int tap = 0; tap < 9; ++tap) {
        const float* xr = xs + ((tap / 3) * (GMAX + 2) + tap % 3) * RD;
        const TW* wt = w + (long long)tap * RD * RD + co;
        for (int c = 0; c < RD; c += 4) {
            const float w0 = to_f32(wt[(c + 0) * RD]), w1 = to_f32(wt[(c + 1) * RD]);
            const float w2 = to_f32(wt[(c + 2) * RD]), w3 = to_f32(wt[(c + 3) * RD]);
#pragma unroll
            for (int k = 0; k < MAXT; ++k) {
                const int tx = grp + NG * k;
                if (tx < g) {
                    const float4 v = *reinterpret_cast<const float4*>(xr + tx * RD + c);
                    acc[k] = fmaf(w3, v.w, fmaf(w2, v.z, fmaf(w1, v.y, fmaf(w0, v.x, acc[k]))));
                }
            }
        }
    }
}

// z for TC tokens (rows hs[tok(t)]) at the NPZ (position, channel) pairs o = tid + NT*j of thread tid: p = o / R2, c2 = tid % R2
template <typename T, int RD>
__device__ __forceinline__ void z_chunk(const float* hs, const int (&tok)[TC], const T* __restrict__ w1f, const float* __restrict__ b1,
                                        float (&z)[16 * RD / 2 / NT][TC]) {
    constexpr int R2 = RD / 2, NPZ = 16 * R2 / NT;
    const float bias = b1[threadIdx.x % R2];
#pragma unroll
    for (int j = 0; j < NPZ; ++j)
#pragma unroll
        for (int t = 0; t < TC; ++t) z[j][t] = bias;
    for (int c = 0; c < RD; ++c) {
        float hv[TC];
#pragma unroll
        for (int t = 0; t < TC; ++t) hv[t] = hs[tok[t] * RD + c];
#pragma unroll
        for (int j = 0; j < NPZ; ++j) {
            const float w = to_f32(w1f[(long long)c * 8 * RD + threadIdx.x + NT * j]);
#pragma unroll
            for (int t = 0; t < TC; ++t) z[j][t] = fmaf(w, hv[t], z[j][t]);
        }
    }
#pragma unroll
    for (int j = 0; j < NPZ; ++j)
#pragma unroll
        for (int t = 0; t < TC; ++t) z[j][t] = rnd<T>(fmaxf(z[j][t], 0.f));
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
template <typename T, int RD>
__global__ __launch_bounds__(NT) void refine_fwd_kernel(const T* __restrict__ a, int tok_off, int Ltot, const T* __restrict__ pk,
                                                        const float* __restrict__ b0, const float* __restrict__ b1,
                                                        const float* __restrict__ b2, T* __restrict__ hout, float* __restrict__ out, int g) {
    constexpr int R2 = RD / 2, NG = NT / RD, MAXT = GMAX / NG, NPZ = 16 * R2 / NT, ZLD = R2 + 1;
    constexpr int XS = 3 * (GMAX + 2) * RD, ZS = TC * 16 * ZLD;
    __shared__ __align__(16) float xz[XS > ZS ? XS : ZS];          // staged input rows, then z of a token chunk
    __shared__ float hs[GMAX * RD];
    __shared__ float w2s[R2 * 16];
    const int tid = threadIdx.x, b = blockIdx.x / g, ty = blockIdx.x % g;
    stage_rows<T, RD>(a, tok_off, Ltot, b, ty, g, xz);
    for (int i = tid; i < R2 * 16; i += NT) w2s[i] = to_f32(pk[off_w2(RD) + i]);
    __syncthreads();
    {
        float acc[MAXT];
        conv3x3_row<T, RD>(xz, pk + off_w0f(RD), g, acc);
        const int co = tid % RD, grp = tid / RD;
        const float bias = b0[co];
#pragma unroll
        for (int k = 0; k < MAXT; ++k) {
            const int tx = grp + NG * k;
            if (tx < g) {
                const float hv = rnd<T>(fmaxf(acc[k] + bias, 0.f));
                hs[tx * RD + co] = hv;
                if (hout) hout[((long long)b * g * g + ty * g + tx) * RD + co] = from_f32<T>(hv);
            }
        }
    }
    __syncthreads();
    const int W = 16 * g;
    const float bias2 = b2[0];
    const int tl = tid >> 4, j1 = (tid >> 2) & 3, j2 = tid & 3;
    for (int t0 = 0; t0 < g; t0 += TC) {
        int tok[TC];
#pragma unroll
        for (int t = 0; t < TC; ++t) tok[t] = min(t0 + t, g - 1);          // past the row end: a valid row, result never stored
        float z[NPZ][TC];
        z_chunk<T, RD>(hs, tok, pk + off_w1f(RD), b1, z);
#pragma unroll
        for (int j = 0; j < NPZ; ++j) {
            const int p = (tid + NT * j) / R2, c2 = tid % R2;
#pragma unroll
            for (int t = 0; t < TC; ++t) xz[(t * 16 + p) * ZLD + c2] = z[j][t];
        }
        __syncthreads();
        // thread -> (token tl, j1, j2), all 16 (i1, i2) rows: a row of 16 tokens x 16 pixels is 256 consecutive floats
        float o[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] = bias2;
        for (int c2 = 0; c2 < R2; ++c2) {
            float zv[4], wv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { zv[i] = xz[(tl * 16 + i * 4 + j1) * ZLD + c2]; wv[i] = w2s[c2 * 16 + i * 4 + j2]; }
#pragma unroll
            for (int i1 = 0; i1 < 4; ++i1)
#pragma unroll
                for (int i2 = 0; i2 < 4; ++i2) o[i1 * 4 + i2] = fmaf(zv[i1], wv[i2], o[i1 * 4 + i2]);
        }
        const int tx = t0 + tl;
        if (tx < g) {
            float* ob = out + ((long long)b * W + 16 * ty) * W + 16 * tx + 4 * j1 + j2;
#pragma unroll
            for (int i = 0; i < 16; ++i) ob[(long long)i * W] = o[i];
        }
        __syncthreads();
    }
}

// ---- backward, launch 1 ------------------------------------------------------------------------------------------------------
// role A (blockIdx < B*g): dh of token row ty (masked by h > 0), fp32 into the workspace
// role B: slabs of (dW1, db1, dW2, db2) for position p over token slice s (blockIdx - B*g = s*16 + p)
template <typename T, int RD>
__global__ __launch_bounds__(NT) void refine_bwd1_kernel(const float* __restrict__ dout, const T* __restrict__ h, const T* __restrict__ pk,
                                                         const float* __restrict__ b1, float* __restrict__ dh, float* __restrict__ slab1,
                                                         int B, int g, int tps) {
    constexpr int R2 = RD / 2, NG = NT / RD, NPZ = 16 * R2 / NT;
    constexpr int SH = GMAX * RD + TC * 256 + TC * 8 * RD;
    __shared__ __align__(16) float sm[SH];
    __shared__ float w2s[R2 * 16];
    const int tid = threadIdx.x, W = 16 * g, gg = g * g;
    const long long T_ = (long long)B * gg;
    for (int i = tid; i < R2 * 16; i += NT) w2s[i] = to_f32(pk[off_w2(RD) + i]);
    if ((int)blockIdx.x < B * g) {
        float* hs = sm;                        // [GMAX][RD]
        float* dos = hs + GMAX * RD;           // [TC][p][q]
        float* dzs = dos + TC * 256;           // [TC][p*R2 + c2]
        const int b = blockIdx.x / g, ty = blockIdx.x % g;
        const T* hr = h + ((long long)b * gg + ty * g) * RD;
        for (int i = tid; i < g * RD; i += NT) hs[i] = to_f32(hr[i]);
        const int tl = tid >> 4, j1 = (tid >> 2) & 3, j2 = tid & 3;
        for (int t0 = 0; t0 < g; t0 += TC) {
            __syncthreads();
            {
                const int tx = t0 + tl;
                const float* ob = dout + ((long long)b * W + 16 * ty) * W + 16 * tx + 4 * j1 + j2;
#pragma unroll
                for (int i = 0; i < 16; ++i) {                  // i = i1*4 + i2
                    float v = 0.f;
                    if (tx < g) v = ob[(long long)i * W];
                    dos[tl * 256 + ((i >> 2) * 4 + j1) * 16 + (i & 3) * 4 + j2] = v;
                }
            }
            __syncthreads();
            int tok[TC];
#pragma unroll
            for (int t = 0; t < TC; ++t) tok[t] = min(t0 + t, g - 1);
            float z[NPZ][TC];
            z_chunk<T, RD>(hs, tok, pk + off_w1f(RD), b1, z);
            const int c2 = tid % R2;
            float w2r[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) w2r[q] = w2s[c2 * 16 + q];
#pragma unroll
            for (int j = 0; j < NPZ; ++j) {
                const int o = tid + NT * j, p = o / R2;
#pragma unroll
                for (int t = 0; t < TC; ++t) {
                    float d = 0.f;
#pragma unroll
                    for (int q = 0; q < 16; ++q) d = fmaf(w2r[q], dos[t * 256 + p * 16 + q], d);
                    dzs[t * 8 * RD + o] = z[j][t] > 0.f ? d : 0.f;
                }
            }
            __syncthreads();
            // dh[t][co] = (h > 0) * sum_o W1d[o][co] dz[t][o]
            constexpr int TPT = TC / NG;
            const int co = tid % RD, grp = tid / RD;
            float acc[TPT];
#pragma unroll
            for (int k = 0; k < TPT; ++k) acc[k] = 0.f;
            const T* w1d = pk + off_w1d(RD) + co;
            for (int o = 0; o < 8 * RD; o += 4) {
                const float w0 = to_f32(w1d[(o + 0) * RD]), w1 = to_f32(w1d[(o + 1) * RD]);
                const float w2 = to_f32(w1d[(o + 2) * RD]), w3 = to_f32(w1d[(o + 3) * RD]);
#pragma unroll
                for (int k = 0; k < TPT; ++k) {
                    const float4 v = *reinterpret_cast<const float4*>(dzs + (grp + NG * k) * 8 * RD + o);
                    acc[k] = fmaf(w3, v.w, fmaf(w2, v.z, fmaf(w1, v.y, fmaf(w0, v.x, acc[k]))));
                }
            }
#pragma unroll
            for (int k = 0; k < TPT; ++k) {
                const int tx = t0 + grp + NG * k;
                if (tx < g) dh[((long long)b * gg + ty * g + tx) * RD + co] = hs[tx * RD + co] > 0.f ? acc[k] : 0.f;
            }
        }
        return;
    }
    // role B
    const int idx = blockIdx.x - B * g, p = idx % 16, s = idx / 16, pi1 = p >> 2, pj1 = p & 3;
    float* hs = sm;                  // [TC][RD]
    float* dop = hs + TC * RD;       // [TC][16]
    float* zs = dop + TC * 16;       // [TC][R2]
    float* dzs = zs + TC * R2;       // [TC][R2]
    constexpr int CT = RD / 16, C2T = R2 / 16, NW2 = R2 * 16 / NT, NGZ = NT / R2, TPZ = TC / NGZ;
    const int cb = tid / 16, c2b = tid % 16;
    float aw1[CT][C2T], aw2[NW2], ab1 = 0.f, ab2 = 0.f;
#pragma unroll
    for (int i = 0; i < CT; ++i)
#pragma unroll
        for (int j = 0; j < C2T; ++j) aw1[i][j] = 0.f;
#pragma unroll
    for (int j = 0; j < NW2; ++j) aw2[j] = 0.f;
    const int zc2 = tid % R2, zgrp = tid / R2;
    const float bz = b1[zc2];
    const T* w1f = pk + off_w1f(RD) + p * R2 + zc2;
    const long long tbeg = (long long)s * tps, tend = min(T_, tbeg + tps);
    for (long long t0 = tbeg; t0 < tend; t0 += TC) {
        __syncthreads();
        for (int i = tid; i < TC * RD; i += NT) {
            const long long t = t0 + i / RD;
            hs[i] = t < tend ? to_f32(h[t * RD + i % RD]) : 0.f;
        }
        {
            const long long t = t0 + tid / 16;
            const int q = tid % 16;
            float v = 0.f;
            if (t < tend) {
                const int bb = (int)(t / gg), r = (int)(t % gg), ty = r / g, tx = r % g;
                v = dout[((long long)bb * W + 16 * ty + 4 * pi1 + (q >> 2)) * W + 16 * tx + 4 * pj1 + (q & 3)];
            }
            dop[tid] = v;
        }
        __syncthreads();
        {
            float zz[TPZ];
#pragma unroll
            for (int k = 0; k < TPZ; ++k) zz[k] = bz;
            for (int c = 0; c < RD; ++c) {
                const float w = to_f32(w1f[(long long)c * 8 * RD]);
#pragma unroll
                for (int k = 0; k < TPZ; ++k) zz[k] = fmaf(w, hs[(zgrp + NGZ * k) * RD + c], zz[k]);
            }
#pragma unroll
            for (int k = 0; k < TPZ; ++k) {
                const int t = zgrp + NGZ * k;
                const float zv = rnd<T>(fmaxf(zz[k], 0.f));
                float d = 0.f;
#pragma unroll
                for (int q = 0; q < 16; ++q) d = fmaf(w2s[zc2 * 16 + q], dop[t * 16 + q], d);
                zs[t * R2 + zc2] = zv;
                dzs[t * R2 + zc2] = zv > 0.f ? d : 0.f;
            }
        }
        __syncthreads();
        for (int t = 0; t < TC; ++t) {
            float hv[CT], dv[C2T];
#pragma unroll
            for (int i = 0; i < CT; ++i) hv[i] = hs[t * RD + cb * CT + i];
#pragma unroll
            for (int j = 0; j < C2T; ++j) dv[j] = dzs[t * R2 + c2b * C2T + j];
#pragma unroll
            for (int i = 0; i < CT; ++i)
#pragma unroll
                for (int j = 0; j < C2T; ++j) aw1[i][j] = fmaf(hv[i], dv[j], aw1[i][j]);
#pragma unroll
            for (int j = 0; j < NW2; ++j) {
                const int o = tid + NT * j;
                aw2[j] = fmaf(zs[t * R2 + o / 16], dop[t * 16 + o % 16], aw2[j]);
            }
            if (tid < R2) ab1 += dzs[t * R2 + tid];
            if (tid < 16) ab2 += dop[t * 16 + tid];
        }
    }
    float* sl = slab1 + ((long long)s * 16 + p) * slab1_elems(RD);
#pragma unroll
    for (int i = 0; i < CT; ++i)
#pragma unroll
        for (int j = 0; j < C2T; ++j) sl[(cb * CT + i) * R2 + c2b * C2T + j] = aw1[i][j];
    if (tid < R2) sl[RD * R2 + tid] = ab1;
#pragma unroll
    for (int j = 0; j < NW2; ++j) sl[RD * R2 + R2 + tid + NT * j] = aw2[j];
    if (tid < 16) sl[RD * R2 + R2 + R2 * 16 + tid] = ab2;
}

// ---- backward, launch 2 ------------------------------------------------------------------------------------------------------
// role A (blockIdx < B*g): da of token row ty = 3x3 of dh with flipped taps and swapped channels (W0d); the rows outside the grid
//   (class token, tok_off) are written as zeros by the first / last row's workgroup
// role B: slab of dW0[:, :, tap] over token slice s (blockIdx - B*g = s*9 + tap); the centre tap also sums db0
template <typename T, int RD>
__global__ __launch_bounds__(NT) void refine_bwd2_kernel(const T* __restrict__ a, int tok_off, int Ltot, const float* __restrict__ dh,
                                                         const T* __restrict__ pk, T* __restrict__ da, float* __restrict__ slab0,
                                                         float* __restrict__ sb0, int B, int g, int tps) {
    constexpr int NG = NT / RD, MAXT = GMAX / NG;
    __shared__ __align__(16) float sm[3 * (GMAX + 2) * RD];
    const int tid = threadIdx.x, gg = g * g;
    if ((int)blockIdx.x < B * g) {
        const int b = blockIdx.x / g, ty = blockIdx.x % g;
        stage_rows<float, RD>(dh, 0, gg, b, ty, g, sm);
        __syncthreads();
        float acc[MAXT];
        conv3x3_row<T, RD>(sm, pk + off_w0d(RD), g, acc);
        const int co = tid % RD, grp = tid / RD;
#pragma unroll
        for (int k = 0; k < MAXT; ++k) {
            const int tx = grp + NG * k;
            if (tx < g) da[((long long)b * Ltot + tok_off + ty * g + tx) * RD + co] = from_f32<T>(acc[k]);
        }
        T* db = da + (long long)b * Ltot * RD;
        if (ty == 0)
            for (int i = tid; i < tok_off * RD; i += NT) db[i] = from_f32<T>(0.f);
        if (ty == g - 1)
            for (int i = (tok_off + gg) * RD + tid; i < Ltot * RD; i += NT) db[i] = from_f32<T>(0.f);
        return;
    }
    const int idx = blockIdx.x - B * g, tap = idx % 9, s = idx / 9, dy = tap / 3 - 1, dx = tap % 3 - 1;
    float* ds = sm;              // [TC][RD] dh
    float* as = ds + TC * RD;    // [TC][RD] a at the tap's neighbour
    constexpr int CT = RD / 16;
    const int ob = tid / 16, ib = tid % 16;
    float acc[CT][CT], ab0 = 0.f;
#pragma unroll
    for (int i = 0; i < CT; ++i)
#pragma unroll
        for (int j = 0; j < CT; ++j) acc[i][j] = 0.f;
    const long long T_ = (long long)B * gg, tbeg = (long long)s * tps, tend = min(T_, tbeg + tps);
    for (long long t0 = tbeg; t0 < tend; t0 += TC) {
        __syncthreads();
        for (int i = tid; i < TC * RD; i += NT) {
            const long long t = t0 + i / RD;
            const int c = i % RD;
            float dv = 0.f, av = 0.f;
            if (t < tend) {
                dv = dh[t * RD + c];
                const int bb = (int)(t / gg), r = (int)(t % gg), y = r / g + dy, x = r % g + dx;
                if (y >= 0 && y < g && x >= 0 && x < g) av = to_f32(a[((long long)bb * Ltot + tok_off + y * g + x) * RD + c]);
            }
            ds[i] = dv;
            as[i] = av;
        }
        __syncthreads();
        for (int t = 0; t < TC; ++t) {
            float dv[CT], av[CT];
#pragma unroll
            for (int i = 0; i < CT; ++i) { dv[i] = ds[t * RD + ob * CT + i]; av[i] = as[t * RD + ib * CT + i]; }
#pragma unroll
            for (int i = 0; i < CT; ++i)
#pragma unroll
                for (int j = 0; j < CT; ++j) acc[i][j] = fmaf(dv[i], av[j], acc[i][j]);
            if (tap == 4 && tid < RD) ab0 += ds[t * RD + tid];
        }
    }
    float* sl = slab0 + ((long long)s * 9 + tap) * RD * RD;
#pragma unroll
    for (int i = 0; i < CT; ++i)
#pragma unroll
        for (int j = 0; j < CT; ++j) sl[(ob * CT + i) * RD + ib * CT + j] = acc[i][j];
    if (tap == 4 && tid < RD) sb0[(long long)s * RD + tid] = ab0;
}

// ---- backward, launch 3: fixed-order slab sums into the parameter-shaped gradients ---------------------------------------------
__global__ __launch_bounds__(NT) void refine_reduce_kernel(const float* __restrict__ slab0, const float* __restrict__ sb0,
                                                           const float* __restrict__ slab1, int S, int RD, float* __restrict__ dw0,
                                                           float* __restrict__ db0, float* __restrict__ dw1, float* __restrict__ db1,
                                                           float* __restrict__ dw2, float* __restrict__ db2) {
    const int R2 = RD / 2;
    const long long RR = (long long)RD * RD, SL1 = slab1_elems(RD);
    long long e = (long long)blockIdx.x * NT + threadIdx.x;
    if (e < 9 * RR) {                                       // slab order (tap, co, c) -> OIHW [co][c][tap]
        const int tap = (int)(e / RR), co = (int)((e / RD) % RD), c = (int)(e % RD);
        float v = 0.f;
        for (int s = 0; s < S; ++s) v += slab0[((long long)s * 9 + tap) * RR + (long long)co * RD + c];
        dw0[((long long)co * RD + c) * 9 + tap] = v;
        return;
    }
    e -= 9 * RR;
    if (e < RD) {
        float v = 0.f;
        for (int s = 0; s < S; ++s) v += sb0[(long long)s * RD + e];
        db0[e] = v;
        return;
    }
    e -= RD;
    if (e < 8 * RR) {                                       // slab order (p, c, c2) -> [c][c2][i1][j1]
        const int p = (int)(e / (RD * R2)), r = (int)(e % (RD * R2));
        float v = 0.f;
        for (int s = 0; s < S; ++s) v += slab1[((long long)s * 16 + p) * SL1 + r];
        dw1[(long long)r * 16 + p] = v;
        return;
    }
    e -= 8 * RR;
    if (e < R2) {
        float v = 0.f;
        for (int s = 0; s < S; ++s)
            for (int p = 0; p < 16; ++p) v += slab1[((long long)s * 16 + p) * SL1 + RD * R2 + e];
        db1[e] = v;
        return;
    }
    e -= R2;
    if (e < R2 * 16) {                                      // [c2][q] = [c2][0][i2][j2]
        float v = 0.f;
        for (int s = 0; s < S; ++s)
            for (int p = 0; p < 16; ++p) v += slab1[((long long)s * 16 + p) * SL1 + RD * R2 + R2 + e];
        dw2[e] = v;
        return;
    }
    e -= R2 * 16;
    if (e == 0) {
        float v = 0.f;
        for (int s = 0; s < S; ++s)
            for (int p = 0; p < 16; ++p)
                for (int q = 0; q < 16; ++q) v += slab1[((long long)s * 16 + p) * SL1 + RD * R2 + R2 + R2 * 16 + q];
        db2[0] = v;
    }
}

// ---- weight pack ----------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void refine_pack_kernel(const float* __restrict__ w0, const float* __restrict__ w1, const float* __restrict__ w2,
                                   T* __restrict__ pk, int RD) {
    const long long RR = (long long)RD * RD, n = packed_elems(RD);
    const int R2 = RD / 2;
    for (long long e = blockIdx.x * (long long)NT + threadIdx.x; e < n; e += (long long)gridDim.x * NT) {
        float v;
        if (e < off_w0d(RD)) {                              // W0f[tap][c][co] = W0[co][c][tap]
            const int tap = (int)(e / RR), c = (int)((e / RD) % RD), co = (int)(e % RD);
            v = w0[((long long)co * RD + c) * 9 + tap];
        } else if (e < off_w1f(RD)) {                       // W0d[tap'][co][c] = W0[co][c][8 - tap']  (da = flipped 3x3 of dh)
            const long long f = e - off_w0d(RD);
            const int tap = (int)(f / RR), co = (int)((f / RD) % RD), c = (int)(f % RD);
            v = w0[((long long)co * RD + c) * 9 + 8 - tap];
        } else if (e < off_w1d(RD)) {                       // W1f[c][p][c2] = W1[c][c2][p]
            const long long f = e - off_w1f(RD);
            const int c = (int)(f / (8 * RD)), p = (int)((f % (8 * RD)) / R2), c2 = (int)(f % R2);
            v = w1[((long long)c * R2 + c2) * 16 + p];
        } else if (e < off_w2(RD)) {                        // W1d[p][c2][c] = W1[c][c2][p]
            const long long f = e - off_w1d(RD);
            const int p = (int)(f / (R2 * (long long)RD)), c2 = (int)((f / RD) % R2), c = (int)(f % RD);
            v = w1[((long long)c * R2 + c2) * 16 + p];
        } else {                                            // W2[c2][q] as it lies
            v = w2[e - off_w2(RD)];
        }
        pk[e] = from_f32<T>(v);
    }
}

int check_shape(int rd, int patch, int g) {
    if (patch != 16)
        EGM_FAIL(EGM_ERR_UNSUPPORTED, "refine: patch %d unsupported (the refined head is built for ViT-B/16: patch 16, 4x4 transposed "
                                      "convolutions)", patch);
    if (rd != 64 && rd != 128) EGM_FAIL(EGM_ERR_UNSUPPORTED, "refine: reduce_dim %d unsupported (64 or 128)", rd);
    if (g < 1 || g > GMAX) EGM_FAIL(EGM_ERR_UNSUPPORTED, "refine: token grid %d x %d unsupported (1 .. %d)", g, g, GMAX);
    return EGM_OK;
}

#define EGM_RD(rd, ...) do { if ((rd) == 64) { constexpr int RD = 64; __VA_ARGS__; } else { constexpr int RD = 128; __VA_ARGS__; } } while (0)

}  // namespace

extern "C" long long egm_refine_packed_elems(int rd, int patch) {
    const int rc = check_shape(rd, patch, 1);
    return rc != EGM_OK ? rc : packed_elems(rd);
}

extern "C" long long egm_refine_bwd_workspace(int B, int g, int rd, int patch) {
    const int rc = check_shape(rd, patch, g);
    if (rc != EGM_OK) return rc;
    if (B < 1) EGM_FAIL(EGM_ERR_ARG, "refine_bwd_workspace: bad batch %d", B);
    return ws_layout(B, g, rd).total * 4;
}

extern "C" int egm_refine_pack(int dtype, const float* w0, const float* w1, const float* w2, void* packed, int rd, int patch,
                               egm_stream_t s) {
    const int rc = check_shape(rd, patch, 1);
    if (rc != EGM_OK) return rc;
    EGM_REQUIRE(w0 && w1 && w2 && packed, "refine_pack: null pointer");
    const int grid = egm_cdiv(packed_elems(rd), NT);
    EGM_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((refine_pack_kernel<T>), dim3(grid), dim3(NT), 0, (hipStream_t)s, w0, w1, w2, (T*)packed, rd));
    EGM_CHECK_LAUNCH("refine_pack");
    return EGM_OK;
}

extern "C" int egm_refine_fwd(int dtype, const void* a, int tok_off, int Ltot, const void* packed, const float* b0, const float* b1,
                              const float* b2, void* h, float* out, int B, int g, int rd, int patch, egm_stream_t s) {
    const int rc = check_shape(rd, patch, g);
    if (rc != EGM_OK) return rc;
    EGM_REQUIRE(a && packed && b0 && b1 && b2 && out && B > 0 && tok_off >= 0 && Ltot >= tok_off + g * g, "refine_fwd: bad args");
    EGM_DISPATCH_DTYPE(dtype, EGM_RD(rd, hipLaunchKernelGGL((refine_fwd_kernel<T, RD>), dim3(B * g), dim3(NT), 0, (hipStream_t)s, (const T*)a,
                                                            tok_off, Ltot, (const T*)packed, b0, b1, b2, (T*)h, out, g)));
    EGM_CHECK_LAUNCH("refine_fwd");
    return EGM_OK;
}

extern "C" int egm_refine_bwd(int dtype, const float* dout, const void* a, int tok_off, int Ltot, const void* h, const void* packed,
                              const float* b1, void* da, float* dw0, float* db0, float* dw1, float* db1, float* dw2, float* db2,
                              void* workspace, int B, int g, int rd, int patch, egm_stream_t s) {
    const int rc = check_shape(rd, patch, g);
    if (rc != EGM_OK) return rc;
    EGM_REQUIRE(dout && a && h && packed && b1 && da && dw0 && db0 && dw1 && db1 && dw2 && db2 && workspace && B > 0 && tok_off >= 0 &&
                Ltot >= tok_off + g * g, "refine_bwd: bad args");
    const Slices sl = slices_for((long long)B * g * g);
    const WsLayout wl = ws_layout(B, g, rd);
    float* ws = (float*)workspace;
    EGM_DISPATCH_DTYPE(dtype, EGM_RD(rd, {
        hipLaunchKernelGGL((refine_bwd1_kernel<T, RD>), dim3(B * g + 16 * sl.S), dim3(NT), 0, (hipStream_t)s, dout, (const T*)h,
                           (const T*)packed, b1, ws + wl.dh, ws + wl.s1, B, g, sl.tps);
        hipLaunchKernelGGL((refine_bwd2_kernel<T, RD>), dim3(B * g + 9 * sl.S), dim3(NT), 0, (hipStream_t)s, (const T*)a, tok_off, Ltot,
                           ws + wl.dh, (const T*)packed, (T*)da, ws + wl.s0, ws + wl.sb0, B, g, sl.tps);
    }));
    const long long nout = 17LL * rd * rd + rd + (rd / 2) * 17 + 1;
    hipLaunchKernelGGL(refine_reduce_kernel, dim3(egm_cdiv(nout, NT)), dim3(NT), 0, (hipStream_t)s, ws + wl.s0, ws + wl.sb0, ws + wl.s1, sl.S,
                       rd, dw0, db0, dw1, db1, dw2, db2);
    EGM_CHECK_LAUNCH("refine_bwd");
    return EGM_OK;
}
