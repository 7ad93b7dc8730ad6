// The two loop frames of the BatchNorm kernel family (bn.hip, bn_fused.hip, bn_dz_fused.hip, pool_fused.hip): the per-channel
// partial-sum pass and the streaming apply pass.  A kernel supplies what differs -- its loads, its element arithmetic, its stores --
// as functors marked __attribute__((always_inline)); the frame owns the geometry: coefficient staging, the item loop, the write-back.
//
// No floating-point arithmetic lives here except the fixed-order column sum of bn_partials.  HIP contracts multiplies and adds across
// statements, so arithmetic shared through a header could fuse differently per call site; every formula stays in the .hip file that
// uses it, built from bn_elem.h (the rule of strip_out.h).
#pragma once
#include "common.h"

// Partial sums of a per-channel reduction: block = 256 threads = (256 / ncv) item rows x ncv channel vectors; out[blk][2][C].
// (bid, nb) = this block's index among the nb blocks working on the tensor: blockIdx / gridDim for the single-tensor kernels, a slice
// of the grid for the multi-tensor ones.  red: the caller's 2 * 256 * 8 floats of LDS.
// STAGE: the four coefficient rows scale | shift | mean | rstd go through red[] once per block and the thread's 8 channels of each
// into registers (C <= 1024); without it f sees zeros.
// f(item, cv, sc, sh, mu, rs, s, q) loads what it needs of `item` (a pixel, or a 2x2 window) and accumulates into s[] and q[].
template <bool STAGE, typename F>
__device__ __forceinline__ void bn_partials(float* red, const float* __restrict__ scale, const float* __restrict__ shift,
                                            const float* __restrict__ mean, const float* __restrict__ rstd, long long n, int C,
                                            float* __restrict__ out, int bid, int nb, F f) {
    const int ncv = C >> 3, rows = 256 / ncv;
    const int tid = threadIdx.x, cv = tid % ncv, row = tid / ncv;
    float s[8], q[8], sc[8], sh[8], mu[8], rs[8];
    zero8(s); zero8(q); zero8(sc); zero8(sh); zero8(mu); zero8(rs);
    if (STAGE) {                                               // stage the per-channel coefficients once per block
        for (int c = tid; c < C; c += 256) { red[c] = scale[c]; red[C + c] = shift[c]; red[2 * C + c] = mean[c]; red[3 * C + c] = rstd[c]; }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) { sc[j] = red[cv * 8 + j]; sh[j] = red[C + cv * 8 + j]; mu[j] = red[2 * C + cv * 8 + j]; rs[j] = red[3 * C + cv * 8 + j]; }
        __syncthreads();                                       // red[] is reused for the reduction below
    }
    if (row < rows) {
        for (long long i = (long long)bid * rows + row; i < n; i += (long long)nb * rows) f(i, cv, sc, sh, mu, rs, s, q);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) { red[tid * 8 + j] = s[j]; red[(256 + tid) * 8 + j] = q[j]; }
    __syncthreads();
    // thread t < 2*C sums column t over the `rows` item rows (fixed order)
    for (int t = tid; t < 2 * C; t += 256) {
        const int which = t / C, c = t - which * C, ccv = c >> 3, j = c & 7;
        float v = 0.f;
        for (int r = 0; r < rows; ++r) v += red[(which * 256 + r * ncv + ccv) * 8 + j];
        out[((long long)bid * 2 + which) * C + c] = v;
    }
}

// Streaming pass over [npix][C]: when C/8 divides 256 a thread keeps the same 8 channels for its whole grid-stride loop, so the NR
// per-channel coefficient rows are staged once per block through cf[] (the caller's NR * C floats of LDS: every thread of every block
// reading the same few global lines serialises on one L2 channel) and then live in registers; the loop body is 16-byte loads and
// stores with two pixels in flight, issued as  ld a; ld b; op a; op b; st a; st b.  Any other C / 8 takes the generic path behind it:
// an item -> (pixel, vector) division and the coefficients from global memory per vector.
//   coef(c, r)       -> r[NR], the coefficients of channel c (fills the LDS rows, and the registers of the generic path)
//   ld(p, cv, v)        loads vector cv of pixel p into v (a V: the kernel's per-pixel registers)
//   op(v, k)            the arithmetic, k[NR][8] = the coefficient rows of the thread's 8 channels
//   st(p, cv, v)        stores the results
template <typename V, int NR, typename Coef, typename Ld, typename Op, typename St>
__device__ __forceinline__ void bn_stream(long long npix, int C, int bid, int nb, float* cf, Coef coef, Ld ld, Op op, St st) {
    const int ncv = C >> 3;
    float k[NR][8];
    if (256 % ncv == 0) {
        for (int c = threadIdx.x; c < C; c += 256) {
            float r[NR];
            coef(c, r);
#pragma unroll
            for (int i = 0; i < NR; ++i) cf[i * C + c] = r[i];
        }
        __syncthreads();
        const int cv = threadIdx.x % ncv, ppb = 256 / ncv;
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int i = 0; i < NR; ++i) k[i][j] = cf[i * C + cv * 8 + j];
        const long long stride = (long long)nb * ppb;
        long long p = (long long)bid * ppb + threadIdx.x / ncv;
        for (; p + stride < npix; p += 2 * stride) {              // two independent pixels in flight
            V a, b;
            ld(p, cv, a); ld(p + stride, cv, b);
            op(a, k); op(b, k);
            st(p, cv, a); st(p + stride, cv, b);
        }
        if (p < npix) { V a; ld(p, cv, a); op(a, k); st(p, cv, a); }
        return;
    }
    const long long total = npix * ncv;
    for (long long i = bid * 256LL + threadIdx.x; i < total; i += (long long)nb * 256) {
        const long long p = i / ncv; const int cv = (int)(i - p * ncv);
        V a;
        ld(p, cv, a);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float r[NR];
            coef(cv * 8 + j, r);
#pragma unroll
            for (int i = 0; i < NR; ++i) k[i][j] = r[i];
        }
        op(a, k);
        st(p, cv, a);
    }
}
