// Knowledge distillation against a frozen teacher (Hinton et al. 2015), on the device (train_utils/distill_loss.py):
//   egm_distill_workspace, egm_distill_fwd, egm_distill_bwd    the temperature-scaled KL term and its gradient
//   egm_pseudo_target_i64                                      hard labels of the teacher where it is confident
//   egm_renorm_resize_f32                                      the student's normalised crop -> the teacher CLIPSeg's input
//
// The loss passes are the boundary loss's streaming frame (csrc/sdf.hip): one image per blockIdx.y, kDistillBlocks workgroups per
// image in a grid-stride loop over its pixels, four pixels per lane through vector loads where every plane allows it (up to four
// channels) and one otherwise, channel templates 2 / 4 / 16, plain-store partial sums per workgroup that one workgroup sums in a
// fixed order in double with the counts in integers.  No float atomics: loss and gradient have the same bits from run to run.  The backward recomputes both
// softmaxes from the logits; nothing per pixel lives between the passes.  Bandwidth-bound, no MFMA.
#include "common.h"

namespace {

constexpr int kDistillBlocks = 256;           // workgroups per image of the loss passes = partial sums per image
constexpr int kDistillMaxC = 16;
constexpr int kResizeMaxTaps = 64;            // kClipMaxTaps of csrc/ensemble_pipe.hip: the same limit, the same message

__device__ __forceinline__ float distill_f32(float v) { return v; }
__device__ __forceinline__ float distill_f32(unsigned short v) { return __uint_as_float((unsigned int)v << 16); }      // bf16 bits

// V consecutive values of T from p (V = 4: one load of 4 * sizeof(T) bytes; the launcher has checked the alignment)
template <int V, typename T>
__device__ __forceinline__ void distill_load(const T* __restrict__ p, float (&v)[V]) {
    if constexpr (V == 1) {
        v[0] = distill_f32(p[0]);
    } else {
        T raw[V];
        __builtin_memcpy(raw, __builtin_assume_aligned(p, V * sizeof(T)), V * sizeof(T));
#pragma unroll
        for (int i = 0; i < V; ++i) v[i] = distill_f32(raw[i]);
    }
}

// log-softmax of a[c] * inv_t over the channels in the max-subtracted form: a[c][v] becomes log softmax, pr[c][v] the softmax itself.
// Student and teacher go through this one function, so equal logits give equal bits and a KL term of exactly 0.
template <int CB, int V>
__device__ __forceinline__ void distill_log_softmax(float (&a)[CB][V], int C, float inv_t, float (&pr)[CB][V]) {
    float mx[V], se[V];
#pragma unroll
    for (int v = 0; v < V; ++v) { mx[v] = -INFINITY; se[v] = 0.f; }
#pragma unroll
    for (int c = 0; c < CB; ++c)
        if (c < C) {
#pragma unroll
            for (int v = 0; v < V; ++v) { a[c][v] *= inv_t; mx[v] = fmaxf(mx[v], a[c][v]); }
        }
#pragma unroll
    for (int c = 0; c < CB; ++c)
        if (c < C) {
#pragma unroll
            for (int v = 0; v < V; ++v) { a[c][v] -= mx[v]; pr[c][v] = expf(a[c][v]); se[v] += pr[c][v]; }
        }
#pragma unroll
    for (int v = 0; v < V; ++v) { mx[v] = logf(se[v]); se[v] = 1.f / se[v]; }
#pragma unroll
    for (int c = 0; c < CB; ++c)
        if (c < C) {
#pragma unroll
            for (int v = 0; v < V; ++v) { a[c][v] -= mx[v]; pr[c][v] *= se[v]; }
        }
}

// The teacher's confidence max_c softmax(z)_c at temperature 1 = 1 / sum_c exp(z_c - max z), and the first channel that holds the max
template <int CB>
__device__ __forceinline__ float distill_confidence(const float (&z)[CB], int C, int& best) {
    float mz = -INFINITY;
    best = 0;
#pragma unroll
    for (int c = 0; c < CB; ++c)
        if (c < C && z[c] > mz) { mz = z[c]; best = c; }
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < CB; ++c)
        if (c < C) s += expf(z[c] - mz);
    return 1.f / s;
}

// The V pixels from p of image planes lg (student) and zt (teacher): lq / q = log softmax and softmax of x / T, lp / pp of z / T;
// ok[v] = the pixel is valid (target not ignored, teacher confident)
template <int CB, int V, typename TZ>
__device__ __forceinline__ void distill_pixel(const float* __restrict__ lg, const TZ* __restrict__ zt, const long long* __restrict__ tg,
                                              long long HW, long long p, int C, int has_ignore, long long ignore_index, float inv_t,
                                              float tau, float (&lq)[CB][V], float (&q)[CB][V], float (&lp)[CB][V], float (&pp)[CB][V],
                                              bool (&ok)[V]) {
#pragma unroll
    for (int c = 0; c < CB; ++c)
        if (c < C) {
            distill_load<V>(lg + c * HW + p, lq[c]);
            distill_load<V>(zt + c * HW + p, lp[c]);
        }
#pragma unroll
    for (int v = 0; v < V; ++v) {
        ok[v] = !(tg && has_ignore) || tg[p + v] != ignore_index;
        if (tau > 0.f) {                                       // (uniform: tau is one device scalar)
            float zc[CB];
#pragma unroll
            for (int c = 0; c < CB; ++c) zc[c] = c < C ? lp[c][v] : 0.f;
            int best;
            ok[v] = ok[v] && distill_confidence<CB>(zc, C, best) >= tau;
        }
    }
    distill_log_softmax<CB, V>(lq, C, inv_t, q);
    distill_log_softmax<CB, V>(lp, C, inv_t, pp);
}

// psum[n][b] = this workgroup's sum over its valid pixels of sum_c p_c (log p_c - log q_c), pcnt[n][b] = their count; plain stores
template <int CB, int V, typename TZ>
__global__ __launch_bounds__(256) void distill_fwd_kernel(const float* __restrict__ logits, const TZ* __restrict__ teacher,
                                                          const long long* __restrict__ target, int C, long long HW, int has_ignore,
                                                          long long ignore_index, float inv_t, const float* __restrict__ tau_dev,
                                                          float* __restrict__ psum, unsigned int* __restrict__ pcnt) {
    __shared__ float red_s[4];
    __shared__ unsigned int red_c[4];
    const int n = blockIdx.y;
    const float* lg = logits + (long long)n * C * HW;
    const TZ* zt = teacher + (long long)n * C * HW;
    const long long* tg = target ? target + (long long)n * HW : nullptr;
    const float tau = tau_dev[0];
    float acc = 0.f;
    unsigned int cnt = 0u;
    for (long long p = (blockIdx.x * 256LL + threadIdx.x) * V; p < HW; p += (long long)gridDim.x * 256 * V) {
        float lq[CB][V], q[CB][V], lp[CB][V], pp[CB][V];
        bool ok[V];
        distill_pixel<CB, V, TZ>(lg, zt, tg, HW, p, C, has_ignore, ignore_index, inv_t, tau, lq, q, lp, pp, ok);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            float kl = 0.f;
#pragma unroll
            for (int c = 0; c < CB; ++c)
                if (c < C) kl += pp[c][v] * (lp[c][v] - lq[c][v]);     // (p_c = 0 after an underflow: 0 * finite, the logs never overflow)
            acc += ok[v] ? kl : 0.f;
            cnt += ok[v] ? 1u : 0u;
        }
    }
    acc = wave_sum(acc);
    cnt = wave_sum_u32(cnt);
    if ((threadIdx.x & 63) == 0) { red_s[threadIdx.x >> 6] = acc; red_c[threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        psum[(long long)n * gridDim.x + blockIdx.x] = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
        pcnt[(long long)n * gridDim.x + blockIdx.x] = red_c[0] + red_c[1] + red_c[2] + red_c[3];
    }
}

// one workgroup: the partial sums in a fixed order in double, the count in integers -> out = {w L_KD, L_KD}, valid = V,
// inv_v[0] = 1 / max(1, V)
__global__ __launch_bounds__(1024) void distill_finalize_kernel(const float* __restrict__ psum, const unsigned int* __restrict__ pcnt,
                                                                int nparts, float t2, const float* __restrict__ w_dev,
                                                                float* __restrict__ inv_v, float* __restrict__ out,
                                                                long long* __restrict__ valid) {
    __shared__ double red_s[16];
    __shared__ unsigned long long red_c[16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double s = 0.0;
    unsigned long long c = 0ull;
    for (int b = threadIdx.x; b < nparts; b += 1024) { s += (double)psum[b]; c += pcnt[b]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    c = wave_sum_u64(c);
    if (lane == 0) { red_s[wv] = s; red_c[wv] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        s = 0.0;
        c = 0ull;
        for (int i = 0; i < 16; ++i) { s += red_s[i]; c += red_c[i]; }
        const double d = (double)(c > 0ull ? c : 1ull);
        const float l = c > 0ull ? (float)((double)t2 * s / d) : 0.f;
        inv_v[0] = (float)(1.0 / d);
        out[0] = w_dev[0] * l;
        out[1] = l;
        if (valid) valid[0] = (long long)c;
    }
}

// dlogits[c] = go w T / max(1, V) * (q_c - p_c) at a valid pixel, 0 elsewhere; every element written
template <int CB, int V, typename TZ>
__global__ __launch_bounds__(256) void distill_bwd_kernel(const float* __restrict__ logits, const TZ* __restrict__ teacher,
                                                          const long long* __restrict__ target, int C, long long HW, int has_ignore,
                                                          long long ignore_index, float inv_t, float t, const float* __restrict__ tau_dev,
                                                          const float* __restrict__ inv_v, const float* __restrict__ gout,
                                                          const float* __restrict__ w_dev, float* __restrict__ dlogits) {
    const int n = blockIdx.y;
    const float* lg = logits + (long long)n * C * HW;
    const TZ* zt = teacher + (long long)n * C * HW;
    const long long* tg = target ? target + (long long)n * HW : nullptr;
    float* dl = dlogits + (long long)n * C * HW;
    const float tau = tau_dev[0];
    const float scale = (gout ? gout[0] : 1.f) * w_dev[0] * t * inv_v[0];
    for (long long p = (blockIdx.x * 256LL + threadIdx.x) * V; p < HW; p += (long long)gridDim.x * 256 * V) {
        float lq[CB][V], q[CB][V], lp[CB][V], pp[CB][V];
        bool ok[V];
        distill_pixel<CB, V, TZ>(lg, zt, tg, HW, p, C, has_ignore, ignore_index, inv_t, tau, lq, q, lp, pp, ok);
#pragma unroll
        for (int c = 0; c < CB; ++c)
            if (c < C) {
                float g[V];
#pragma unroll
                for (int v = 0; v < V; ++v) g[v] = ok[v] ? scale * (q[c][v] - pp[c][v]) : 0.f;
                if constexpr (V == 1) {                        // the element-wise kernels' store policy (common.h, EGM_STORE_MODE)
                    __builtin_nontemporal_store(g[0], dl + c * HW + p);
                } else {
                    egm_u32x4 a;
                    a.x = __float_as_uint(g[0]); a.y = __float_as_uint(g[1]); a.z = __float_as_uint(g[2]); a.w = __float_as_uint(g[3]);
                    egm_store16_as<EGM_STORE_MODE>(dl + c * HW + p, a);
                }
            }
    }
}

// out[i] = the teacher's argmax class (ties to the lowest class) where its confidence is >= tau and the existing target, if any, is
// not ignored; ignore_index elsewhere
template <typename TZ>
__global__ __launch_bounds__(256) void pseudo_target_kernel(const TZ* __restrict__ teacher, const long long* __restrict__ existing, int C,
                                                            long long HW, long long total, long long ignore_index,
                                                            const float* __restrict__ tau_dev, long long* __restrict__ out) {
    const float tau = tau_dev[0];
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        long long n; long long p;
        n = i / HW; p = i - n * HW;
        const TZ* z = teacher + n * C * HW + p;
        float zc[kDistillMaxC];
#pragma unroll
        for (int c = 0; c < kDistillMaxC; ++c) zc[c] = c < C ? distill_f32(z[c * HW]) : 0.f;
        int best;
        const float conf = distill_confidence<kDistillMaxC>(zc, C, best);
        const bool keep = conf >= tau && !(existing && existing[i] == ignore_index);
        out[i] = keep ? (long long)best : ignore_index;
    }
}

// ---- renorm_resize: horizontal pass.  tmp[n][c][y][xo] = sum_j wx[xo][j] * fmaf(x[n][c][y][b0 + j], a_c, b_c), the taps in table
// order, every step one fmaf into the running sum (DESIGN.md 6.35 fixes this order)
__global__ __launch_bounds__(256) void renorm_hfilter_kernel(const float* __restrict__ x, long long rows, int H, int W,
                                                             float* __restrict__ tmp, int Sw, const int* __restrict__ bounds,
                                                             const float* __restrict__ wts, int ksize, float a0, float a1, float a2,
                                                             float b0, float b1, float b2) {
    const long long total = rows * Sw;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        long long r; int xo; egm_divmod(i, Sw, r, xo);
        long long nc; int y; egm_divmod(r, H, nc, y);
        const int c = (int)(nc % 3);
        const float a = c == 0 ? a0 : (c == 1 ? a1 : a2), b = c == 0 ? b0 : (c == 1 ? b1 : b2);
        const int first = clampi(bounds[xo * 2], 0, W - 1);
        const int n = clampi(bounds[xo * 2 + 1], 0, min(ksize, W - first));         // no table can make the kernel read outside the row
        const float* src = x + r * W + first;
        const float* w = wts + (long long)xo * ksize;
        float acc = 0.f;
        for (int j = 0; j < n; ++j) acc = fmaf(w[j], fmaf(src[j], a, b), acc);
        tmp[i] = acc;
    }
}

// vertical pass: out[n][c][yo][x] = sum_j wy[yo][j] * tmp[n][c][b0 + j][x], the same form
__global__ __launch_bounds__(256) void renorm_vfilter_kernel(const float* __restrict__ tmp, long long planes, int H, int Sw,
                                                             float* __restrict__ out, int Sh, const int* __restrict__ bounds,
                                                             const float* __restrict__ wts, int ksize) {
    const long long total = planes * Sh * Sw;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        long long r; int xo; egm_divmod(i, Sw, r, xo);
        long long pl; int yo; egm_divmod(r, Sh, pl, yo);
        const int first = clampi(bounds[yo * 2], 0, H - 1);
        const int n = clampi(bounds[yo * 2 + 1], 0, min(ksize, H - first));
        const float* src = tmp + (pl * H + first) * Sw + xo;
        const float* w = wts + (long long)yo * ksize;
        float acc = 0.f;
        for (int j = 0; j < n; ++j) acc = fmaf(w[j], src[(long long)j * Sw], acc);
        out[i] = acc;
    }
}

// ---------------------------------------------------------------- host
inline int distill_shape_check(const char* name, int N, int C, int H, int W) {
    EGM_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C <= kDistillMaxC, "%s: bad shape %d x %d x %d x %d (at most %d channels)", name, N, C, H,
                W, kDistillMaxC);
    EGM_REQUIRE(N <= 65535, "%s: %d images in one call, at most 65535 are supported", name, N);
    return EGM_OK;
}
inline int distill_common_check(const char* name, int teacher_dtype, float temperature) {
    EGM_REQUIRE(teacher_dtype == EGM_F32 || teacher_dtype == EGM_BF16, "%s: teacher dtype %d, float32 (0) or bfloat16 (1) expected", name,
                teacher_dtype);
    EGM_REQUIRE(temperature > 0.f && temperature <= 3.0e38f, "%s: temperature %g, a finite value > 0 is expected", name, (double)temperature);
    return EGM_OK;
}
// four pixels per lane where every channel plane of every image starts at a boundary of its four-pixel load (16 bytes of fp32, 8 of
// bf16).  The 16-channel template always takes one: sixteen channels of four pixels of both models are 128 registers of logits alone,
// and the compiler's report shows that form at 256 VGPRs with spills to scratch, one wave per SIMD.
inline bool distill_vec4(long long HW, const void* logits, const void* teacher, int teacher_dtype, const void* dlogits) {
    const uintptr_t zmask = teacher_dtype == EGM_BF16 ? 7 : 15;
    return HW % 4 == 0 && egm_aligned16(logits) && (reinterpret_cast<uintptr_t>(teacher) & zmask) == 0 && (!dlogits || egm_aligned16(dlogits));
}

}  // namespace

extern "C" int egm_distill_blocks(void) { return kDistillBlocks; }

extern "C" long long egm_distill_workspace(int N, int C, int H, int W) {
    if (distill_shape_check("distill_workspace", N, C, H, W) != EGM_OK) return EGM_ERR_ARG;
    return ((long long)2 * N * kDistillBlocks + 4) * 4;        // partial sums, counts, 1 / max(1, V)
}

#define EGM_DISTILL_LAUNCH_T(kernel, TZ, ...)                                                                                     \
    do {                                                                                                                          \
        const dim3 grid_(kDistillBlocks, N), block_(256);                                                                         \
        if (vec4 && C <= 4) {                                                                                                     \
            if (C <= 2) hipLaunchKernelGGL((kernel<2, 4, TZ>), grid_, block_, 0, (hipStream_t)s, __VA_ARGS__);                    \
            else hipLaunchKernelGGL((kernel<4, 4, TZ>), grid_, block_, 0, (hipStream_t)s, __VA_ARGS__);                           \
        } else {                                                                                                                  \
            if (C <= 2) hipLaunchKernelGGL((kernel<2, 1, TZ>), grid_, block_, 0, (hipStream_t)s, __VA_ARGS__);                    \
            else if (C <= 4) hipLaunchKernelGGL((kernel<4, 1, TZ>), grid_, block_, 0, (hipStream_t)s, __VA_ARGS__);               \
            else hipLaunchKernelGGL((kernel<kDistillMaxC, 1, TZ>), grid_, block_, 0, (hipStream_t)s, __VA_ARGS__);                \
        }                                                                                                                         \
    } while (0)

extern "C" int egm_distill_fwd(const float* logits, const void* teacher, int teacher_dtype, const long long* target, int N, int C, int H,
                               int W, int has_ignore, long long ignore_index, float temperature, const float* w_dev, const float* tau_dev,
                               void* workspace, float* out2, long long* valid_out, egm_stream_t s) {
    const char* name = "distill_fwd";
    if (distill_shape_check(name, N, C, H, W) != EGM_OK || distill_common_check(name, teacher_dtype, temperature) != EGM_OK) return EGM_ERR_ARG;
    EGM_REQUIRE(logits && teacher && w_dev && tau_dev && workspace && out2, "%s: null pointer", name);
    EGM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "%s: the workspace must be 4-byte aligned", name);
    const long long HW = (long long)H * W;
    float* psum = reinterpret_cast<float*>(workspace);
    unsigned int* pcnt = reinterpret_cast<unsigned int*>(psum + (long long)N * kDistillBlocks);
    float* inv_v = psum + (long long)2 * N * kDistillBlocks;
    const float inv_t = 1.0f / temperature;
    const bool vec4 = distill_vec4(HW, logits, teacher, teacher_dtype, nullptr);
    if (teacher_dtype == EGM_BF16)
        EGM_DISTILL_LAUNCH_T(distill_fwd_kernel, unsigned short, logits, (const unsigned short*)teacher, target, C, HW, has_ignore, ignore_index,
                             inv_t, tau_dev, psum, pcnt);
    else
        EGM_DISTILL_LAUNCH_T(distill_fwd_kernel, float, logits, (const float*)teacher, target, C, HW, has_ignore, ignore_index, inv_t, tau_dev,
                             psum, pcnt);
    EGM_CHECK_LAUNCH("distill_fwd");
    hipLaunchKernelGGL(distill_finalize_kernel, dim3(1), dim3(1024), 0, (hipStream_t)s, psum, pcnt, N * kDistillBlocks,
                       temperature * temperature, w_dev, inv_v, out2, valid_out);
    EGM_CHECK_LAUNCH("distill_fwd (finalize)");
    return EGM_OK;
}

extern "C" int egm_distill_bwd(const float* logits, const void* teacher, int teacher_dtype, const long long* target, int N, int C, int H,
                               int W, int has_ignore, long long ignore_index, float temperature, const float* w_dev, const float* tau_dev,
                               const void* workspace, const float* grad_out, float* dlogits, egm_stream_t s) {
    const char* name = "distill_bwd";
    if (distill_shape_check(name, N, C, H, W) != EGM_OK || distill_common_check(name, teacher_dtype, temperature) != EGM_OK) return EGM_ERR_ARG;
    EGM_REQUIRE(logits && teacher && w_dev && tau_dev && workspace && dlogits, "%s: null pointer", name);
    const long long HW = (long long)H * W;
    const float* inv_v = reinterpret_cast<const float*>(workspace) + (long long)2 * N * kDistillBlocks;
    const float inv_t = 1.0f / temperature;
    const bool vec4 = distill_vec4(HW, logits, teacher, teacher_dtype, dlogits);
    if (teacher_dtype == EGM_BF16)
        EGM_DISTILL_LAUNCH_T(distill_bwd_kernel, unsigned short, logits, (const unsigned short*)teacher, target, C, HW, has_ignore, ignore_index,
                             inv_t, temperature, tau_dev, inv_v, grad_out, w_dev, dlogits);
    else
        EGM_DISTILL_LAUNCH_T(distill_bwd_kernel, float, logits, (const float*)teacher, target, C, HW, has_ignore, ignore_index, inv_t,
                             temperature, tau_dev, inv_v, grad_out, w_dev, dlogits);
    EGM_CHECK_LAUNCH("distill_bwd");
    return EGM_OK;
}
#undef EGM_DISTILL_LAUNCH_T

extern "C" int egm_pseudo_target_i64(const void* teacher, int teacher_dtype, const long long* existing, int N, int C, int H, int W,
                                     long long ignore_index, const float* tau_dev, long long* out, egm_stream_t s) {
    const char* name = "pseudo_target_i64";
    if (distill_shape_check(name, N, C, H, W) != EGM_OK || distill_common_check(name, teacher_dtype, 1.f) != EGM_OK) return EGM_ERR_ARG;
    EGM_REQUIRE(teacher && tau_dev && out, "%s: null pointer", name);
    const long long HW = (long long)H * W, total = (long long)N * HW;
    if (teacher_dtype == EGM_BF16)
        hipLaunchKernelGGL(pseudo_target_kernel<unsigned short>, dim3(egm_stream_grid(total)), dim3(256), 0, (hipStream_t)s,
                           (const unsigned short*)teacher, existing, C, HW, total, ignore_index, tau_dev, out);
    else
        hipLaunchKernelGGL(pseudo_target_kernel<float>, dim3(egm_stream_grid(total)), dim3(256), 0, (hipStream_t)s, (const float*)teacher,
                           existing, C, HW, total, ignore_index, tau_dev, out);
    EGM_CHECK_LAUNCH(name);
    return EGM_OK;
}

extern "C" int egm_renorm_resize_f32(const float* x_nchw, int N, int H, int W, float* out_nchw, int Sh, int Sw, const int* xbounds,
                                     const float* xweights, int xksize, const int* ybounds, const float* yweights, int yksize,
                                     const float* a3_host, const float* b3_host, float* tmp_nchw, egm_stream_t s) {
    const char* who = "renorm_resize_f32";
    EGM_REQUIRE(x_nchw && out_nchw && xbounds && xweights && ybounds && yweights && a3_host && b3_host && tmp_nchw, "%s: null pointer", who);
    EGM_REQUIRE(N > 0 && H > 0 && W > 0 && Sh > 0 && Sw > 0 && xksize > 0 && yksize > 0, "%s: bad shape", who);
    EGM_REQUIRE((long long)N * H * W * 3 < (1ll << 31) && (long long)N * H * Sw * 3 < (1ll << 31) && (long long)N * 3 * Sh * Sw < (1ll << 31),
                "%s: input too large", who);
    EGM_REQUIRE(xksize <= kResizeMaxTaps && yksize <= kResizeMaxTaps,
                "%s: %d x %d filter taps, at most %d per axis are supported (an antialiased reduction by up to 31.5)", who, yksize, xksize,
                kResizeMaxTaps);
    const long long planes = (long long)N * 3, rows = planes * H;
    hipLaunchKernelGGL(renorm_hfilter_kernel, dim3(egm_stream_grid(rows * Sw)), dim3(256), 0, (hipStream_t)s, x_nchw, rows, H, W, tmp_nchw, Sw,
                       xbounds, xweights, xksize, a3_host[0], a3_host[1], a3_host[2], b3_host[0], b3_host[1], b3_host[2]);
    EGM_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(renorm_vfilter_kernel, dim3(egm_stream_grid(planes * Sh * Sw)), dim3(256), 0, (hipStream_t)s, (const float*)tmp_nchw,
                       planes, H, Sw, out_nchw, Sh, ybounds, yweights, yksize);
    EGM_CHECK_LAUNCH(who);
    return EGM_OK;
}
