// Per-channel reductions, train/eval BatchNorm + activation forward and backward for NHWC activations.
// Replaces nn.BatchNorm2d(+nn.ReLU / nn.Sigmoid) at src/EGM-UNet.py:50-51,53-54,878-879,894-895,900-901,966-973.
// All of these are HBM-bound streaming kernels: 16-byte (bf16) / 32-byte (fp32) vectors of 8 channels per lane,
// channel-contiguous so a wave reads whole pixels; reductions are two-stage with plain stores (deterministic).
#include "common.h"
#include "bn_elem.h"
#include "bn_frames.h"
#include <stdlib.h>

namespace {


// block = 256 threads = (256 / ncv) pixel rows x ncv channel-vectors; out[blk][2][C]
// MODE 0: (x, x^2).  MODE 1 (BN backward): (dzp, dzp*xhat) with dzp = dz*act'(y*scale+shift), xhat = (y-mean)*rstd.
// (bid, nb) = this block's index among the nb blocks working on the tensor: blockIdx / gridDim for the single-tensor kernels, a
// slice of the grid for the multi-tensor ones (several BatchNorms of independent branches in one launch)
template <typename T, int MODE>
__device__ __forceinline__ void channel_partials_body(const T* __restrict__ a, int lda, const T* __restrict__ y, int ldy,
                                                      const float* __restrict__ scale, const float* __restrict__ shift,
                                                      const float* __restrict__ mean, const float* __restrict__ rstd,
                                                      int act, long long npix, int C, float* __restrict__ out, int bid, int nb) {
    __shared__ float red[2 * 256 * 8];
    bn_partials<MODE == 1>(red, scale, shift, mean, rstd, npix, C, out, bid, nb,
        [&](long long p, int cv, const float (&sc)[8], const float (&sh)[8], const float (&mu)[8], const float (&rs)[8], float (&s)[8],
            float (&q)[8]) __attribute__((always_inline)) {
            float v[8];
            load8(a + p * lda + cv * 8, v);
            if (MODE == 0) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { s[j] += v[j]; q[j] += v[j] * v[j]; }
            } else {
                float yv[8];
                load8(y + p * ldy + cv * 8, yv);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float g = v[j] * act_grad<sizeof(T) == 2>(fmaf(yv[j], sc[j], sh[j]), act);
                    s[j] += g; q[j] += g * (yv[j] - mu[j]) * rs[j];
                }
            }
        });
}
template <typename T, int MODE>
__global__ __launch_bounds__(256) void channel_partials_kernel(const T* __restrict__ a, int lda, const T* __restrict__ y, int ldy,
                                                               const float* __restrict__ scale, const float* __restrict__ shift,
                                                               const float* __restrict__ mean, const float* __restrict__ rstd,
                                                               int act, long long npix, int C, float* __restrict__ out) {
    channel_partials_body<T, MODE>(a, lda, y, ldy, scale, shift, mean, rstd, act, npix, C, out, blockIdx.x, gridDim.x);
}

// sums [ntiles][2][C] -> out [2][C] in double, fixed order.  grid = C/8 blocks of 1024 threads (8 channels x 128 tile lanes).
__device__ __forceinline__ void tiles_reduce(const float* __restrict__ st, int ntiles, int C, int c0, double& s_out, double& q_out,
                                             double* red) {
    const int tid = threadIdx.x, j = tid & 7, tl = tid >> 3;       // 128 tile lanes
    const int c = c0 + j;
    double s = 0.0, q = 0.0;
    if (c < C) {
        for (int t = tl; t < ntiles; t += 128) {
            s += (double)st[((long long)t * 2 + 0) * C + c];
            q += (double)st[((long long)t * 2 + 1) * C + c];
        }
    }
    red[tid] = s; red[1024 + tid] = q;
    __syncthreads();
    for (int stride = 64; stride > 0; stride >>= 1) {
        if (tl < stride) { red[tid] += red[tid + stride * 8]; red[1024 + tid] += red[1024 + tid + stride * 8]; }
        __syncthreads();
    }
    s_out = red[j]; q_out = red[1024 + j];
}

__global__ __launch_bounds__(1024) void reduce_tiles_kernel(const float* __restrict__ st, int ntiles, int C, float* __restrict__ out) {
    __shared__ double red[2048];
    double s, q;
    st += (long long)blockIdx.y * ntiles * 2 * C;                 // batched: one independent reduction per blockIdx.y
    out += (long long)blockIdx.y * 2 * C;
    tiles_reduce(st, ntiles, C, blockIdx.x * 8, s, q, red);
    const int c = blockIdx.x * 8 + (threadIdx.x & 7);
    if (threadIdx.x < 8 && c < C) { out[c] = (float)s; out[C + c] = (float)q; }
}

__device__ __forceinline__ void bn_finalize_body(const float* __restrict__ st, int ntiles, double count,
                                                 const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                 float momentum, float* __restrict__ rmean, float* __restrict__ rvar,
                                                 float* __restrict__ scale, float* __restrict__ shift,
                                                 float* __restrict__ save_mean, float* __restrict__ save_rstd, int C,
                                                 int Creal, int bid) {
    __shared__ double red[2048];
    double s, q;
    tiles_reduce(st, ntiles, C, bid * 8, s, q, red);
    const int c = bid * 8 + (threadIdx.x & 7);
    if (threadIdx.x < 8 && c >= Creal && c < C) { scale[c] = 0.f; shift[c] = 0.f; save_mean[c] = 0.f; save_rstd[c] = 0.f; }
    if (threadIdx.x < 8 && c < Creal) {
        const double mean = s / count;
        double var = q / count - mean * mean;               // biased (normalisation) variance
        if (var < 0.0) var = 0.0;
        const float rstd = (float)(1.0 / sqrt(var + (double)eps));
        const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
        scale[c] = g * rstd;
        shift[c] = b - (float)mean * g * rstd;
        save_mean[c] = (float)mean;
        save_rstd[c] = rstd;
        if (rmean != nullptr) {
            const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
            rmean[c] = (1.f - momentum) * rmean[c] + momentum * (float)mean;
            rvar[c] = (1.f - momentum) * rvar[c] + momentum * (float)unbiased;
        }
    }
}
#ifdef EGM_DIAG_EXTRA_LAUNCHES
__global__ __launch_bounds__(1024) void diag_tiny_kernel(const float* __restrict__ st, float* __restrict__ scale) {
    if (st[0] == 12345.678f && threadIdx.x == 2000) scale[0] = 0.f;       // reads one line, writes nothing
}
#endif
__global__ __launch_bounds__(1024) void bn_finalize_kernel(const float* __restrict__ st, int ntiles, double count,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                           float momentum, float* __restrict__ rmean, float* __restrict__ rvar,
                                                           float* __restrict__ scale, float* __restrict__ shift,
                                                           float* __restrict__ save_mean, float* __restrict__ save_rstd, int C,
                                                           int Creal) {
    bn_finalize_body(st, ntiles, count, gamma, beta, eps, momentum, rmean, rvar, scale, shift, save_mean, save_rstd, C, Creal, blockIdx.x);
}

// BatchNorm backward, second stage: partial tiles [ntiles][2][C] of (sum dzp, sum dzp*xhat) -> sums [2][C] (= dbeta | dgamma) and the
// coefficient rows cf [4][C] = scale | shift | cb | cc with dy = scale*dzp + cb + cc*y (bn_elem.h): one launch instead of a reduce_tiles
// launch plus per-element mean arithmetic in the apply passes that follow.
__device__ __forceinline__ void bn_bwd_coefs_body(const float* __restrict__ st, int ntiles, float inv_count,
                                                  const float* __restrict__ scale, const float* __restrict__ shift,
                                                  const float* __restrict__ mean, const float* __restrict__ rstd, int train,
                                                  float* __restrict__ sums, float* __restrict__ cf, int C, int bid) {
    __shared__ double red[2048];
    double s, q;
    tiles_reduce(st, ntiles, C, bid * 8, s, q, red);
    const int c = bid * 8 + (threadIdx.x & 7);
    if (threadIdx.x < 8 && c < C) {
        const float s0 = (float)s, s1 = (float)q;
        sums[c] = s0; sums[C + c] = s1;
        const float scv = scale[c];
        float cbv = 0.f, ccv = 0.f;
        if (train) bn_bwd_cb_cc(scv, s0, s1, inv_count, mean[c], rstd[c], cbv, ccv);
        cf[c] = scv; cf[C + c] = shift[c]; cf[2 * C + c] = cbv; cf[3 * C + c] = ccv;
    }
}
__global__ __launch_bounds__(1024) void bn_bwd_coefs_kernel(const float* __restrict__ st, int ntiles, float inv_count,
                                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd, int train,
                                                            float* __restrict__ sums, float* __restrict__ cf, int C) {
    bn_bwd_coefs_body(st, ntiles, inv_count, scale, shift, mean, rstd, train, sums, cf, C, blockIdx.x);
}

__global__ void bn_eval_coeffs_kernel(const float* gamma, const float* beta, const float* rm, const float* rv, float eps,
                                      float* scale, float* shift, float* save_mean, float* save_rstd, int C, int Creal) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= Creal && c < C) { scale[c] = 0.f; shift[c] = 0.f; if (save_mean) { save_mean[c] = 0.f; save_rstd[c] = 0.f; } }
    if (c < Creal) {
        const float rstd = 1.f / sqrtf(rv[c] + eps);
        const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
        scale[c] = g * rstd; shift[c] = b - rm[c] * g * rstd;
        if (save_mean) { save_mean[c] = rm[c]; save_rstd[c] = rstd; }
    }
}

// Streaming kernels below: when C/8 divides 256 a thread keeps the same 8 channels for its whole grid-stride loop, so the
// per-channel coefficients are loaded once into registers and the loop body is pure 16-byte loads/stores.
template <typename T>
__device__ __forceinline__ void bn_act_fwd_body(const T* __restrict__ y, int ldy, const float* __restrict__ scale,
                                                const float* __restrict__ shift, int act, T* __restrict__ z, int ldz,
                                                long long npix, int C, int bid, int nb) {
    __shared__ float cf[2 * 2048];
    struct V { float v[8]; };
    bn_stream<V, 2>(npix, C, bid, nb, cf,
        [&](int c, float (&r)[2]) __attribute__((always_inline)) { r[0] = scale[c]; r[1] = shift[c]; },
        [&](long long p, int cv, V& a) __attribute__((always_inline)) { load8(y + p * ldy + cv * 8, a.v); },
        [&](V& a, const float (&k)[2][8]) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < 8; ++j) a.v[j] = bn_fwd_elem<sizeof(T) == 2>(a.v[j], k[0][j], k[1][j], act);
        },
        [&](long long p, int cv, V& a) __attribute__((always_inline)) { store8(z + p * ldz + cv * 8, a.v); });
}
template <typename T>
__global__ __launch_bounds__(256) void bn_act_fwd_kernel(const T* __restrict__ y, int ldy, const float* __restrict__ scale,
                                                         const float* __restrict__ shift, int act, T* __restrict__ z, int ldz,
                                                         long long npix, int C) {
    bn_act_fwd_body<T>(y, ldy, scale, shift, act, z, ldz, npix, C, blockIdx.x, gridDim.x);
}

// dy = scale * (dzp - mean(dzp) - xhat * mean(dzp*xhat))   (train)   |   dy = scale * dzp   (eval)
//    = ca*dzp + cb + cc*y   with per-channel ca = scale, cb = -scale*(m0 - mean*rstd*m1), cc = -scale*rstd*m1   (train)
template <typename T>
__device__ __forceinline__ void bn_act_bwd_apply_body(const T* __restrict__ dz, int lddz, const T* __restrict__ y, int ldy,
                                                      const float* __restrict__ scale, const float* __restrict__ shift,
                                                      const float* __restrict__ mean, const float* __restrict__ rstd, int act,
                                                      int train, const float* __restrict__ sums, float inv_count,
                                                      T* __restrict__ dy, int lddy, long long npix, int C, int bid, int nb) {
    __shared__ float cf[4 * 2048];                         // scale | shift | cb | cc, computed once per block
    struct V { float g[8], y[8]; };
    bn_stream<V, 4>(npix, C, bid, nb, cf,
        [&](int c, float (&r)[4]) __attribute__((always_inline)) {
            r[0] = scale[c]; r[1] = shift[c]; r[2] = 0.f; r[3] = 0.f;
            if (train) bn_bwd_cb_cc(r[0], sums[c], sums[C + c], inv_count, mean[c], rstd[c], r[2], r[3]);
        },
        [&](long long p, int cv, V& a) __attribute__((always_inline)) { load8(dz + p * lddz + cv * 8, a.g); load8(y + p * ldy + cv * 8, a.y); },
        [&](V& a, const float (&k)[4][8]) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < 8; ++j) a.g[j] = bn_bwd_elem<sizeof(T) == 2>(a.g[j], a.y[j], k[0][j], k[1][j], k[2][j], k[3][j], act);
        },
        [&](long long p, int cv, V& a) __attribute__((always_inline)) { store8(dy + p * lddy + cv * 8, a.g); });
}
template <typename T>
__global__ __launch_bounds__(256) void bn_act_bwd_apply_kernel(const T* __restrict__ dz, int lddz, const T* __restrict__ y, int ldy,
                                                               const float* __restrict__ scale, const float* __restrict__ shift,
                                                               const float* __restrict__ mean, const float* __restrict__ rstd, int act,
                                                               int train, const float* __restrict__ sums, float inv_count,
                                                               T* __restrict__ dy, int lddy, long long npix, int C) {
    bn_act_bwd_apply_body<T>(dz, lddz, y, ldy, scale, shift, mean, rstd, act, train, sums, inv_count, dy, lddy, npix, C, blockIdx.x, gridDim.x);
}


// ---- multi-tensor forms: the BatchNorm passes of up to EGM_BN_MULTI_MAX INDEPENDENT layers (the parallel branches of
// EdgeEnhancedGRFB, src/EGM-UNet.py:1256-1278: 8-32 channel tensors whose passes are launch-latency bound) in ONE launch each.
// The descriptors travel by value as a kernel argument; a block finds its tensor by the cumulative block counts (blk0).
struct BnMulti { egm_bn_desc e[EGM_BN_MULTI_MAX]; int blk0[EGM_BN_MULTI_MAX + 1]; int n; };

__device__ __forceinline__ int multi_entry(const BnMulti& m, int& bid, int& nb) {
    int k = 0;
#pragma unroll
    for (int i = 1; i < EGM_BN_MULTI_MAX; ++i) if (i < m.n && (int)blockIdx.x >= m.blk0[i]) k = i;
    bid = blockIdx.x - m.blk0[k]; nb = m.blk0[k + 1] - m.blk0[k];
    return k;
}
__global__ __launch_bounds__(1024) void bn_finalize_multi_kernel(BnMulti m) {
    int bid, nb; const egm_bn_desc& d = m.e[multi_entry(m, bid, nb)];
    bn_finalize_body(d.stats, d.ntiles, (double)d.npix, d.gamma, d.beta, d.eps, d.momentum, d.running_mean, d.running_var, d.coef,
                     d.coef + d.C, d.coef + 2 * d.C, d.coef + 3 * d.C, d.C, d.C_real, bid);
}
template <typename T>
__global__ __launch_bounds__(256) void bn_act_fwd_multi_kernel(BnMulti m) {
    int bid, nb; const egm_bn_desc& d = m.e[multi_entry(m, bid, nb)];
    bn_act_fwd_body<T>((const T*)d.y, d.ldy, d.coef, d.coef + d.C, d.act, (T*)d.z, d.ldz, d.npix, d.C, bid, nb);
}
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_reduce_multi_kernel(BnMulti m) {
    int bid, nb; const egm_bn_desc& d = m.e[multi_entry(m, bid, nb)];
    channel_partials_body<T, 1>((const T*)d.dz, d.lddz, (const T*)d.y, d.ldy, d.coef, d.coef + d.C, d.coef + 2 * d.C, d.coef + 3 * d.C, d.act,
                                d.npix, d.C, d.partials, bid, nb);
}
__global__ __launch_bounds__(1024) void bn_bwd_coefs_multi_kernel(BnMulti m) {
    int bid, nb; const egm_bn_desc& d = m.e[multi_entry(m, bid, nb)];
    bn_bwd_coefs_body(d.partials, d.nblocks, 1.f / (float)d.npix, d.coef, d.coef + d.C, d.coef + 2 * d.C, d.coef + 3 * d.C, d.train, d.sums,
                      d.cf4, d.C, bid);
}
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_multi_kernel(BnMulti m) {
    int bid, nb; const egm_bn_desc& d = m.e[multi_entry(m, bid, nb)];
    bn_act_bwd_apply_body<T>((const T*)d.dz, d.lddz, (const T*)d.y, d.ldy, d.coef, d.coef + d.C, d.coef + 2 * d.C, d.coef + 3 * d.C, d.act,
                             d.train, d.sums, 1.f / (float)d.npix, (T*)d.dy, d.lddy, d.npix, d.C, bid, nb);
}

// which: 0 finalize, 1 fwd apply, 2 bwd reduce, 3 bwd coefs, 4 bwd apply -> blocks a tensor gets (the single-tensor launch geometry)
int multi_blocks(const egm_bn_desc& d, int which) {
    switch (which) {
        case 0: case 3: return (d.C + 7) / 8;
        case 2: return egm_partial_blocks(d.npix, d.C);
        default: return egm_stream_grid(d.npix * (d.C >> 3));
    }
}
int multi_build(const egm_bn_desc* descs, int n, int which, BnMulti* m) {
    if (!descs || n < 1 || n > EGM_BN_MULTI_MAX) return -1;
    m->n = n; m->blk0[0] = 0;
    for (int i = 0; i < n; ++i) {
        const egm_bn_desc& d = descs[i];
        if (d.C <= 0 || d.C % 8 || d.C > 1024 || d.npix <= 0 || !d.coef) return -1;
        m->e[i] = d;
        m->blk0[i + 1] = m->blk0[i] + multi_blocks(d, which);
    }
    for (int i = n; i < EGM_BN_MULTI_MAX; ++i) m->blk0[i + 1] = m->blk0[n];
    return m->blk0[n];
}

}  // namespace


extern "C" int egm_channel_partials_blocks(long long npix, int C) {
    if (C <= 0 || C % 8 || C > 2048) return -1;
    return egm_partial_blocks(npix, C);
}

extern "C" int egm_channel_sums(int dtype, const void* x, int ld, long long npix, int C, float* partials, egm_stream_t s) {
    EGM_REQ_VEC("channel_sums", x, ld, C);
    EGM_REQUIRE(partials && npix > 0 && C <= 2048, "channel_sums: bad args");
    const int nb = egm_partial_blocks(npix, C);
    EGM_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((channel_partials_kernel<T, 0>), dim3(nb), dim3(256), 0, (hipStream_t)s, (const T*)x,
                                                 ld, (const T*)nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, npix, C, partials));
    EGM_CHECK_LAUNCH("channel_sums");
    return EGM_OK;
}

/* ---- the bias gradients of a whole backward pass as two launches (db = sum over pixels of dy, nn.Conv2d biases that no BatchNorm follows:
 * src/EGM-UNet.py:1256-1313 branch heads / tails, 1362-1390 attention convs, 1499 classifier).  One by one they were ~25 pairs of
 * egm_channel_sums + egm_reduce_tiles per step, 5 us each for tensors that take 1-2 us to read; here every tensor keeps the block count,
 * the per-block pixel set and the summation order of that pair (channel_partials_body<T, 0> and tiles_reduce are the same code), so the
 * result is bit-identical to it.
 * table: device array of 2n egm_bsum_entry -- entries [0, n) carry chunk0 = first stage-1 block of the tensor (nblk blocks each),
 * entries [n, 2n) the same tensors with chunk0 = first stage-2 block (C/8 blocks each). */
typedef egm_bsum_entry BsumEntry;
static_assert(sizeof(BsumEntry) == 56, "egm_bsum_entry layout");

template <typename T>
__global__ __launch_bounds__(256) void channel_sums_multi_kernel(const BsumEntry* __restrict__ tab, int n) {
    const int k = egm_find_entry(tab, n, (long long)blockIdx.x);
    const BsumEntry e = tab[k];
    channel_partials_body<T, 0>((const T*)e.x, e.ld, (const T*)nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, e.npix, e.C, e.part,
                                (int)blockIdx.x - e.chunk0, e.nblk);
}
__global__ __launch_bounds__(1024) void bias_reduce_multi_kernel(const BsumEntry* __restrict__ tab, int n) {
    __shared__ double red[2048];
    const int k = egm_find_entry(tab, n, (long long)blockIdx.x);
    const BsumEntry e = tab[k];
    const int c0 = ((int)blockIdx.x - e.chunk0) * 8;
    double s, q;
    tiles_reduce(e.part, e.nblk, e.C, c0, s, q, red);
    const int c = c0 + (threadIdx.x & 7);
    if (threadIdx.x < 8 && c < e.Cout) e.out[c] = (float)s;
}

extern "C" int egm_bias_grad_multi(int dtype, const void* table_dev, int n, long long blocks1, long long blocks2, egm_stream_t s) {
    EGM_REQUIRE(table_dev && n > 0 && blocks1 > 0 && blocks2 > 0 && blocks1 < (1LL << 30) && blocks2 < (1LL << 30), "bias_grad_multi: bad args");
    const BsumEntry* tab = (const BsumEntry*)table_dev;
    EGM_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((channel_sums_multi_kernel<T>), dim3((unsigned)blocks1), dim3(256), 0, (hipStream_t)s, tab, n));
    EGM_CHECK_LAUNCH("bias_grad_multi (partials)");
    hipLaunchKernelGGL(bias_reduce_multi_kernel, dim3((unsigned)blocks2), dim3(1024), 0, (hipStream_t)s, tab + n, n);
    EGM_CHECK_LAUNCH("bias_grad_multi (reduce)");
    return EGM_OK;
}

extern "C" int egm_reduce_tiles_batched(const float* tiles, int batch, int ntiles, int C, float* out, egm_stream_t s) {
    EGM_REQUIRE(tiles && out && batch > 0 && ntiles > 0 && C > 0, "reduce_tiles_batched: bad args");
    hipLaunchKernelGGL(reduce_tiles_kernel, dim3((C + 7) / 8, batch), dim3(1024), 0, (hipStream_t)s, tiles, ntiles, C, out);
    EGM_CHECK_LAUNCH("reduce_tiles_batched");
    return EGM_OK;
}
extern "C" int egm_reduce_tiles(const float* tiles, int ntiles, int C, float* out, egm_stream_t s) {
    EGM_REQUIRE(tiles && out && ntiles > 0 && C > 0, "reduce_tiles: bad args");
    hipLaunchKernelGGL(reduce_tiles_kernel, dim3((C + 7) / 8, 1), dim3(1024), 0, (hipStream_t)s, tiles, ntiles, C, out);
    EGM_CHECK_LAUNCH("reduce_tiles");
    return EGM_OK;
}

extern "C" int egm_bn_finalize(const float* stats, int ntiles, long long count, const float* gamma, const float* beta, float eps,
                               float momentum, float* running_mean, float* running_var, float* scale, float* shift,
                               float* save_mean, float* save_rstd, int C, int C_real, egm_stream_t s) {
    EGM_REQUIRE(stats && scale && shift && save_mean && save_rstd && ntiles > 0 && count > 0 && C > 0 && C_real > 0 && C_real <= C,
                "bn_finalize: bad args");
    EGM_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "bn_finalize: running stats must come in pairs");
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 7) / 8), dim3(1024), 0, (hipStream_t)s, stats, ntiles, (double)count, gamma, beta,
                       eps, momentum, running_mean, running_var, scale, shift, save_mean, save_rstd, C, C_real);
    EGM_CHECK_LAUNCH("bn_finalize");
#ifdef EGM_DIAG_EXTRA_LAUNCHES
    // diagnostic build (profiles/r04_ab_runs.md): what ONE more tiny dependent launch costs inside the captured step -- k extra kernels of
    // the finalize kernel's geometry that only read their arguments, behind each of the 30 egm_bn_finalize calls of a step
    {
        static int extra = -1;
        if (extra < 0) extra = getenv("EGM_EXTRA_LAUNCHES") ? atoi(getenv("EGM_EXTRA_LAUNCHES")) : 0;
        for (int i = 0; i < extra; ++i)
            hipLaunchKernelGGL(diag_tiny_kernel, dim3((C + 7) / 8), dim3(1024), 0, (hipStream_t)s, stats, scale);
    }
#endif
    return EGM_OK;
}

extern "C" int egm_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                                  float eps, float* scale, float* shift, float* save_mean, float* save_rstd, int C, int C_real,
                                  egm_stream_t s) {
    EGM_REQUIRE(running_mean && running_var && scale && shift && C > 0 && C_real > 0 && C_real <= C, "bn_eval_coeffs: bad args");
    hipLaunchKernelGGL(bn_eval_coeffs_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)s, gamma, beta, running_mean,
                       running_var, eps, scale, shift, save_mean, save_rstd, C, C_real);
    EGM_CHECK_LAUNCH("bn_eval_coeffs");
    return EGM_OK;
}

extern "C" int egm_bn_act_fwd(int dtype, const void* y, int ldy, const float* scale, const float* shift, int act, void* z, int ldz,
                              long long npix, int C, egm_stream_t s) {
    EGM_REQ_VEC("bn_act_fwd", y, ldy, C);
    EGM_REQ_VEC("bn_act_fwd", z, ldz, C);
    EGM_REQUIRE(scale && shift && npix > 0, "bn_act_fwd: bad args");
    const int grid = egm_stream_grid(npix * (C >> 3));
    EGM_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((bn_act_fwd_kernel<T>), dim3(grid), dim3(256), 0, (hipStream_t)s, (const T*)y, ldy,
                                                 scale, shift, act, (T*)z, ldz, npix, C));
    EGM_CHECK_LAUNCH("bn_act_fwd");
    return EGM_OK;
}

extern "C" int egm_bn_act_bwd_reduce(int dtype, const void* dz, int lddz, const void* y, int ldy, const float* scale,
                                     const float* shift, const float* save_mean, const float* save_rstd, int act, float* partials,
                                     long long npix, int C, egm_stream_t s) {
    EGM_REQ_VEC("bn_act_bwd_reduce", dz, lddz, C);
    EGM_REQ_VEC("bn_act_bwd_reduce", y, ldy, C);
    EGM_REQUIRE(scale && shift && save_mean && save_rstd && partials && npix > 0 && C <= 1024, "bn_act_bwd_reduce: bad args (C <= 1024)");
    const int nb = egm_partial_blocks(npix, C);
    EGM_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((channel_partials_kernel<T, 1>), dim3(nb), dim3(256), 0, (hipStream_t)s, (const T*)dz,
                                                 lddz, (const T*)y, ldy, scale, shift, save_mean, save_rstd, act, npix, C, partials));
    EGM_CHECK_LAUNCH("bn_act_bwd_reduce");
    return EGM_OK;
}

extern "C" int egm_bn_bwd_coefs(const float* partials, int ntiles, long long count, const float* scale, const float* shift,
                                const float* save_mean, const float* save_rstd, int train, float* sums, float* cf, int C,
                                egm_stream_t s) {
    EGM_REQUIRE(partials && scale && shift && save_mean && save_rstd && sums && cf && ntiles > 0 && count > 0 && C > 0 && C % 8 == 0,
                "bn_bwd_coefs: bad args");
    hipLaunchKernelGGL(bn_bwd_coefs_kernel, dim3((C + 7) / 8), dim3(1024), 0, (hipStream_t)s, partials, ntiles, 1.f / (float)count,
                       scale, shift, save_mean, save_rstd, train, sums, cf, C);
    EGM_CHECK_LAUNCH("bn_bwd_coefs");
    return EGM_OK;
}

extern "C" int egm_bn_act_bwd_apply(int dtype, const void* dz, int lddz, const void* y, int ldy, const float* scale,
                                    const float* shift, const float* save_mean, const float* save_rstd, int act, int train,
                                    const float* sums, void* dy, int lddy, long long npix, int C, egm_stream_t s) {
    EGM_REQ_VEC("bn_act_bwd_apply", dz, lddz, C);
    EGM_REQ_VEC("bn_act_bwd_apply", y, ldy, C);
    EGM_REQ_VEC("bn_act_bwd_apply", dy, lddy, C);
    EGM_REQUIRE(scale && shift && save_mean && save_rstd && sums && npix > 0, "bn_act_bwd_apply: bad args");
    const int grid = egm_stream_grid(npix * (C >> 3));
    EGM_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((bn_act_bwd_apply_kernel<T>), dim3(grid), dim3(256), 0, (hipStream_t)s, (const T*)dz,
                                                 lddz, (const T*)y, ldy, scale, shift, save_mean, save_rstd, act, train, sums,
                                                 1.f / (float)npix, (T*)dy, lddy, npix, C));
    EGM_CHECK_LAUNCH("bn_act_bwd_apply");
    return EGM_OK;
}

// ---- multi-tensor entry points (descs: HOST array of n <= EGM_BN_MULTI_MAX descriptors, copied into the kernel argument) ----------
extern "C" int egm_bn_multi(int dtype, int which, const egm_bn_desc* descs, int n, egm_stream_t s) {
    BnMulti m;
    const int grid = multi_build(descs, n, which, &m);
    EGM_REQUIRE(grid > 0, "bn_multi: bad descriptors (n=%d, 1..%d tensors, C %% 8 == 0, C <= 1024)", n, EGM_BN_MULTI_MAX);
    // every activation tensor a pass reads or writes: what EGM_REQ_VEC asks of the single-tensor entry points (16-byte vectors)
    auto vec = [](const void* p, int ld, int C) { return p != nullptr && egm_aligned16(p) && ld >= C && ld % 8 == 0; };
    for (int i = 0; i < n; ++i) {
        const egm_bn_desc& d = descs[i];
        switch (which) {
            case EGM_BN_MULTI_FINALIZE: EGM_REQUIRE(d.stats && d.ntiles > 0 && d.C_real > 0 && d.C_real <= d.C, "bn_multi finalize: bad entry %d", i); break;
            case EGM_BN_MULTI_FWD: EGM_REQUIRE(vec(d.y, d.ldy, d.C) && vec(d.z, d.ldz, d.C), "bn_multi fwd: bad entry %d", i); break;
            case EGM_BN_MULTI_BWD_REDUCE: EGM_REQUIRE(vec(d.dz, d.lddz, d.C) && vec(d.y, d.ldy, d.C) && d.partials, "bn_multi bwd reduce: bad entry %d", i); break;
            case EGM_BN_MULTI_BWD_COEFS: EGM_REQUIRE(d.partials && d.nblocks > 0 && d.sums && d.cf4, "bn_multi bwd coefs: bad entry %d", i); break;
            case EGM_BN_MULTI_BWD_APPLY: EGM_REQUIRE(vec(d.dz, d.lddz, d.C) && vec(d.y, d.ldy, d.C) && vec(d.dy, d.lddy, d.C) && d.sums, "bn_multi bwd apply: bad entry %d", i); break;
            default: EGM_FAIL(EGM_ERR_ARG, "bn_multi: unknown pass %d", which);
        }
    }
    hipStream_t st = (hipStream_t)s;
    switch (which) {
        case EGM_BN_MULTI_FINALIZE: hipLaunchKernelGGL(bn_finalize_multi_kernel, dim3(grid), dim3(1024), 0, st, m); break;
        case EGM_BN_MULTI_BWD_COEFS: hipLaunchKernelGGL(bn_bwd_coefs_multi_kernel, dim3(grid), dim3(1024), 0, st, m); break;
        case EGM_BN_MULTI_FWD: EGM_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((bn_act_fwd_multi_kernel<T>), dim3(grid), dim3(256), 0, st, m)); break;
        case EGM_BN_MULTI_BWD_REDUCE: EGM_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((bn_bwd_reduce_multi_kernel<T>), dim3(grid), dim3(256), 0, st, m)); break;
        case EGM_BN_MULTI_BWD_APPLY: EGM_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((bn_bwd_apply_multi_kernel<T>), dim3(grid), dim3(256), 0, st, m)); break;
    }
    EGM_CHECK_LAUNCH("bn_multi");
    return EGM_OK;
}
