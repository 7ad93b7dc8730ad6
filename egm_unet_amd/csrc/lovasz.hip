// Lovasz-Softmax loss (Berman, Triki, Blaschko, CVPR 2018) on the device: the convex extension of the Jaccard loss of
// K classes of fp32 logits [N][C][H][W] against an int64 target with an ignore value, on the stable radix sort of sort.hip.
//   egm_lovasz_workspace, egm_lovasz_errors, egm_lovasz_coefs, egm_lovasz_fwd, egm_lovasz_bwd
// A segment is the whole batch (S = 1, L = N H W) or one image (per_image: S = N, L = H W); the planes of the K classes are K S sort
// segments [k][s] of L elements, which is the layout [K][N][H][W] itself.
//   errors    one streaming launch for all classes: softmax over C, e = |fg - p_c| (0 at an ignored pixel) ->
//             key = (~bits(e) & 0x3FFFFFFF) | fg << 30 | valid << 31, payload = the pixel's index in its segment.  e lies in [0, 1], so
//             bits(e) <= 0x3F800000 fits 30 bits: the sort runs over bits 0..29 and carries the two flags along in the bits it never reads
//   sort      egm_sort_pairs_u32 over bits [0, 30): descending e, ties by ascending pixel index
//   counts    per tile of kLovTile sorted elements the number of foreground and of valid ones (plain stores)
//   scan      one workgroup per segment: exclusive prefix of the tile counts in place, and the segment's totals {G, V}
//   apply     per tile: the inclusive counts F_j, V_j of every element from a wave scan of (fg | valid << 16), the wave and tile
//             offsets; g_j = J(F_j, V_j) - J(F_j - fg_j, V_j - 1) in double, rounded once; coef = sign(p_c - fg) g scattered to the
//             pixel's own place in the coef plane; one double partial of e g per workgroup
//   finalize  one workgroup: the partials per (class, segment) in a fixed order in double, which classes count (present: G > 0, decided
//             here from the scan's totals), L_s, L -> out = {w L, L}; scale[k][s] = 1 / (S P_s) for a counted class, 0 otherwise
//   backward  one streaming launch: softmax again, dlogits[j] = go w sum_k scale_k coef_k p_ck ([c_k == j] - p_j), non-temporal stores
// The forward is 4 * 3 + 5 launches whatever N, K, the content and per_image.  No workgroup waits for another, every loop is bounded by
// the arguments, no atomics on global memory; each element makes g from its own two counts, so no neighbour's value is read.
// counts, scan, apply and finalize are lovasz_core.h's, shared with the Lovasz hinge (lovasz_hinge.hip), on the key layout LovKeySoftmax.
#include "lovasz_core.h"

namespace {

constexpr int kLovMaxC = 16;                   // channels, and classes per call
constexpr unsigned int kLovErrMask = LovKeySoftmax::kErrMask, kLovFg = LovKeySoftmax::kFg, kLovValid = LovKeySoftmax::kValid;

struct LovClasses { int id[kLovMaxC]; };

// softmax over the C channels of V pixels, as bloss_pixel (sdf.hip) does it: e[c][v] = the probabilities
template <int CB, int V>
__device__ __forceinline__ void lov_softmax(const float* __restrict__ lg, long long HW, long long p, int C, float (&e)[CB][V]) {
    float mx[V], se[V];
#pragma unroll
    for (int v = 0; v < V; ++v) { mx[v] = -INFINITY; se[v] = 0.f; }
#pragma unroll
    for (int c = 0; c < CB; ++c)
        if (c < C) {
            lov_load<V>(lg + c * HW + p, e[c]);
#pragma unroll
            for (int v = 0; v < V; ++v) mx[v] = fmaxf(mx[v], e[c][v]);
        }
#pragma unroll
    for (int c = 0; c < CB; ++c)
        if (c < C) {
#pragma unroll
            for (int v = 0; v < V; ++v) { e[c][v] = expf(e[c][v] - mx[v]); se[v] += e[c][v]; }
        }
#pragma unroll
    for (int v = 0; v < V; ++v) se[v] = 1.f / se[v];
#pragma unroll
    for (int c = 0; c < CB; ++c)
        if (c < C) {
#pragma unroll
            for (int v = 0; v < V; ++v) e[c][v] *= se[v];
        }
}

// planes [K][N][HW]: keys, vals and (when not null) e_out
template <int CB, int V>
__global__ __launch_bounds__(256) void lovasz_errors_kernel(const float* __restrict__ logits, const long long* __restrict__ target,
                                                            LovClasses cls, int K, int C, long long HW, long long NHW,
                                                            long long ignore_index, int per_image, unsigned int* __restrict__ keys,
                                                            unsigned int* __restrict__ vals, float* __restrict__ e_out) {
    const int n = blockIdx.y;
    const float* lg = logits + (long long)n * C * HW;
    const long long* tg = target + (long long)n * HW;
    const long long img = (long long)n * HW, first = per_image ? 0 : img;
    for (long long p = (blockIdx.x * 256LL + threadIdx.x) * V; p < HW; p += (long long)gridDim.x * 256 * V) {
        float e[CB][V];
        lov_softmax<CB, V>(lg, HW, p, C, e);
        long long t[V];
#pragma unroll
        for (int v = 0; v < V; ++v) t[v] = tg[p + v];
        for (int k = 0; k < K; ++k) {
            const int id = cls.id[k];
            unsigned int key[V], val[V], eb[V];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                float q = 0.f;
#pragma unroll
                for (int c = 0; c < CB; ++c) q = (c < C && c == id) ? e[c][v] : q;
                const bool valid = t[v] != ignore_index, fg = valid && t[v] == (long long)id;
                const float err = valid ? fabsf((fg ? 1.f : 0.f) - q) : 0.f;
                eb[v] = __float_as_uint(err);
                key[v] = (~eb[v] & kLovErrMask) | (fg ? kLovFg : 0u) | (valid ? kLovValid : 0u);
                val[v] = (unsigned int)(first + p + v);
            }
            const long long at = k * NHW + img + p;
            lov_store<V>(keys + at, key);
            lov_store<V>(vals + at, val);
            if (e_out) lov_store<V>(reinterpret_cast<unsigned int*>(e_out) + at, eb);
        }
    }
}

// dlogits[j] = go w (own_j - p_j A), a_k = scale_k coef_k p_ck, A = sum_k a_k, own_j = a_k of the class k with id j; 0 at an ignored
// pixel because every coef is 0 there
template <int CB, int V>
__global__ __launch_bounds__(256) void lovasz_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ coef, LovClasses cls,
                                                         int K, int C, long long HW, long long NHW, int S, int per_image,
                                                         const float* __restrict__ scale, const float* __restrict__ gout,
                                                         const float* __restrict__ w_dev, float* __restrict__ dlogits) {
    const int n = blockIdx.y;
    const float* lg = logits + (long long)n * C * HW;
    float* dl = dlogits + (long long)n * C * HW;
    const float go = (gout ? gout[0] : 1.f) * w_dev[0];
    const int s = per_image ? n : 0;
    for (long long p = (blockIdx.x * 256LL + threadIdx.x) * V; p < HW; p += (long long)gridDim.x * 256 * V) {
        float e[CB][V], own[CB][V], A[V];
        lov_softmax<CB, V>(lg, HW, p, C, e);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            A[v] = 0.f;
#pragma unroll
            for (int c = 0; c < CB; ++c) own[c][v] = 0.f;
        }
        for (int k = 0; k < K; ++k) {
            const int id = cls.id[k];
            const float sc = scale[k * S + s];
            float cf[V];
            lov_load<V>(coef + k * NHW + (long long)n * HW + p, cf);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                float q = 0.f;
#pragma unroll
                for (int c = 0; c < CB; ++c) q = (c < C && c == id) ? e[c][v] : q;
                const float a = sc * cf[v] * q;
                A[v] += a;
#pragma unroll
                for (int c = 0; c < CB; ++c) own[c][v] = c == id ? a : own[c][v];
            }
        }
#pragma unroll
        for (int c = 0; c < CB; ++c)
            if (c < C) {
                float g[V];
#pragma unroll
                for (int v = 0; v < V; ++v) g[v] = go * (own[c][v] - e[c][v] * A[v]);
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

// ---------------------------------------------------------------- host
struct LovShape {
    int S, ntiles;
    long long L, NHW, HW;
};
inline int lov_shape_check(const char* name, int N, int C, int H, int W, int K, int per_image, LovShape& sh) {
    EGM_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C <= kLovMaxC, "%s: bad shape %d x %d x %d x %d (at most %d channels)", name, N, C, H, W,
                kLovMaxC);
    EGM_REQUIRE(N <= 65535, "%s: %d images in one call, at most 65535 are supported", name, N);
    EGM_REQUIRE(K >= 1 && K <= kLovMaxC, "%s: %d classes, between 1 and %d are supported", name, K, kLovMaxC);
    sh.HW = (long long)H * W;
    sh.NHW = sh.HW * N;
    EGM_REQUIRE(sh.NHW < (1ll << 31), "%s: %d x %d x %d pixels, S * L must stay below 2^31", name, N, H, W);
    sh.S = per_image ? N : 1;
    sh.L = per_image ? sh.HW : sh.NHW;
    sh.ntiles = (int)((sh.L + kLovTile - 1) / kLovTile);
    EGM_REQUIRE((long long)K * sh.S <= 65535, "%s: %d classes x %d segments, at most 65535 planes are supported", name, K, sh.S);
    return EGM_OK;
}
inline int lov_classes_check(const char* name, const int* classes, int K, int C, LovClasses& cls) {
    EGM_REQUIRE(classes, "%s: null pointer (classes)", name);
    for (int k = 0; k < kLovMaxC; ++k) cls.id[k] = -1;
    for (int k = 0; k < K; ++k) {
        EGM_REQUIRE(classes[k] >= 0 && classes[k] < C, "%s: class id %d outside [0, %d)", name, classes[k], C);
        for (int j = 0; j < k; ++j) EGM_REQUIRE(classes[j] != classes[k], "%s: class id %d is repeated", name, classes[k]);
        cls.id[k] = classes[k];
    }
    return EGM_OK;
}
inline LovPlanes lov_planes(void* workspace, const LovShape& sh, int K) { return lov_planes(workspace, K, sh.S, sh.L, sh.ntiles); }
inline bool lov_vec4(long long HW, const void* a, const void* b, const void* c, const void* d) {
    return HW % 4 == 0 && egm_aligned16(a) && egm_aligned16(b) && (!c || egm_aligned16(c)) && (!d || egm_aligned16(d));
}

#define EGM_LOV_LAUNCH(kernel, ...)                                                                                               \
    do {                                                                                                                          \
        const dim3 grid_(kLovBlocks, N), block_(256);                                                                             \
        if (vec4) {                                                                                                               \
            if (C <= 2) hipLaunchKernelGGL((kernel<2, 4>), grid_, block_, 0, (hipStream_t)s, __VA_ARGS__);                        \
            else if (C <= 4) hipLaunchKernelGGL((kernel<4, 4>), grid_, block_, 0, (hipStream_t)s, __VA_ARGS__);                   \
            else hipLaunchKernelGGL((kernel<kLovMaxC, 4>), grid_, block_, 0, (hipStream_t)s, __VA_ARGS__);                        \
        } else {                                                                                                                  \
            if (C <= 2) hipLaunchKernelGGL((kernel<2, 1>), grid_, block_, 0, (hipStream_t)s, __VA_ARGS__);                        \
            else if (C <= 4) hipLaunchKernelGGL((kernel<4, 1>), grid_, block_, 0, (hipStream_t)s, __VA_ARGS__);                   \
            else hipLaunchKernelGGL((kernel<kLovMaxC, 1>), grid_, block_, 0, (hipStream_t)s, __VA_ARGS__);                        \
        }                                                                                                                         \
    } while (0)

inline int lov_errors_launch(const float* logits, const long long* target, const LovClasses& cls, int K, int N, int C, const LovShape& sh,
                             long long ignore_index, int per_image, unsigned int* keys, unsigned int* vals, float* e_out,
                             egm_stream_t s) {
    const bool vec4 = lov_vec4(sh.HW, logits, keys, vals, e_out);
    EGM_LOV_LAUNCH(lovasz_errors_kernel, logits, target, cls, K, C, sh.HW, sh.NHW, ignore_index, per_image, keys, vals, e_out);
    EGM_CHECK_LAUNCH("lovasz_errors");
    return EGM_OK;
}

// errors, sort, counts, scan, apply: everything of the forward but the finalize
inline int lov_coefs_run(const char* name, const float* logits, const long long* target, const LovClasses& cls, int K, int N, int C,
                         const LovShape& sh, long long ignore_index, int per_image, const LovPlanes& pl, float* e_out, float* coef,
                         egm_stream_t s) {
    if (lov_errors_launch(logits, target, cls, K, N, C, sh, ignore_index, per_image, pl.keys, pl.vals, e_out, s) != EGM_OK) return EGM_ERR_LAUNCH;
    return lov_rank_run<LovKeySoftmax>(name, K * sh.S, sh.L, sh.ntiles, pl, coef, s);
}

}  // namespace

extern "C" long long egm_lovasz_workspace(int N, int C, int H, int W, int K, int per_image) {
    LovShape sh;
    if (lov_shape_check("lovasz_workspace", N, C, H, W, K, per_image, sh) != EGM_OK) return EGM_ERR_ARG;
    return lov_planes(nullptr, sh, K).bytes;
}

extern "C" int egm_lovasz_errors(const float* logits, const long long* target, const int* classes, int K, int N, int C, int H, int W,
                                 long long ignore_index, int per_image, unsigned int* keys, unsigned int* vals, float* e_out,
                                 egm_stream_t s) {
    const char* name = "lovasz_errors";
    LovShape sh;
    LovClasses cls;
    if (lov_shape_check(name, N, C, H, W, K, per_image, sh) != EGM_OK || lov_classes_check(name, classes, K, C, cls) != EGM_OK)
        return EGM_ERR_ARG;
    EGM_REQUIRE(logits && target && keys && vals, "%s: null pointer", name);
    return lov_errors_launch(logits, target, cls, K, N, C, sh, ignore_index, per_image, keys, vals, e_out, s);
}

extern "C" int egm_lovasz_coefs(const float* logits, const long long* target, const int* classes, int K, int N, int C, int H, int W,
                                long long ignore_index, int per_image, void* workspace, float* e_out, float* coef, egm_stream_t s) {
    const char* name = "lovasz_coefs";
    LovShape sh;
    LovClasses cls;
    if (lov_shape_check(name, N, C, H, W, K, per_image, sh) != EGM_OK || lov_classes_check(name, classes, K, C, cls) != EGM_OK)
        return EGM_ERR_ARG;
    EGM_REQUIRE(logits && target && workspace && coef, "%s: null pointer", name);
    EGM_REQUIRE(egm_aligned16(workspace), "%s: the workspace must be 16-byte aligned", name);
    return lov_coefs_run(name, logits, target, cls, K, N, C, sh, ignore_index, per_image, lov_planes(workspace, sh, K), e_out, coef, s);
}

extern "C" int egm_lovasz_fwd(const float* logits, const long long* target, const int* classes, int K, int N, int C, int H, int W,
                              long long ignore_index, int per_image, int present, const float* w_dev, void* workspace, float* coef,
                              float* out2, egm_stream_t s) {
    const char* name = "lovasz_fwd";
    LovShape sh;
    LovClasses cls;
    if (lov_shape_check(name, N, C, H, W, K, per_image, sh) != EGM_OK || lov_classes_check(name, classes, K, C, cls) != EGM_OK)
        return EGM_ERR_ARG;
    EGM_REQUIRE(logits && target && w_dev && workspace && coef && out2, "%s: null pointer", name);
    EGM_REQUIRE(egm_aligned16(workspace), "%s: the workspace must be 16-byte aligned", name);
    const LovPlanes pl = lov_planes(workspace, sh, K);
    const int rc = lov_coefs_run(name, logits, target, cls, K, N, C, sh, ignore_index, per_image, pl, nullptr, coef, s);
    if (rc != EGM_OK) return rc;
    return lov_finalize_run("lovasz_fwd (finalize)", K, sh.S, sh.ntiles, present, w_dev, pl, out2, s);
}

extern "C" int egm_lovasz_bwd(const float* logits, const float* coef, const int* classes, int K, int N, int C, int H, int W,
                              int per_image, const void* workspace, const float* grad_out, const float* w_dev, float* dlogits,
                              egm_stream_t s) {
    const char* name = "lovasz_bwd";
    LovShape sh;
    LovClasses cls;
    if (lov_shape_check(name, N, C, H, W, K, per_image, sh) != EGM_OK || lov_classes_check(name, classes, K, C, cls) != EGM_OK)
        return EGM_ERR_ARG;
    EGM_REQUIRE(logits && coef && w_dev && workspace && dlogits, "%s: null pointer", name);
    EGM_REQUIRE(egm_aligned16(workspace), "%s: the workspace must be 16-byte aligned", name);
    const LovPlanes pl = lov_planes(const_cast<void*>(workspace), sh, K);
    const bool vec4 = lov_vec4(sh.HW, logits, coef, dlogits, nullptr);
    EGM_LOV_LAUNCH(lovasz_bwd_kernel, logits, coef, cls, K, C, sh.HW, sh.NHW, sh.S, per_image, pl.scale, grad_out, w_dev, dlogits);
    EGM_CHECK_LAUNCH("lovasz_bwd");
    return EGM_OK;
}
#undef EGM_LOV_LAUNCH
