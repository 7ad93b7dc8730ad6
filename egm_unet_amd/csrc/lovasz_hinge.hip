// Lovasz hinge loss (Berman, Triki, Blaschko, CVPR 2018: lovasz_hinge) on the device: the convex extension of the
// Jaccard loss of one binary score map per image, on the stable radix sort of sort.hip and the rank passes of lovasz_core.h.
//   egm_lovasz_hinge_workspace, egm_lovasz_hinge_errors, egm_lovasz_hinge_coefs, egm_lovasz_hinge_fwd, egm_lovasz_hinge_bwd
// Score forms (those of sweep.hip).  C == 1: logits fp32 [N][H][W], every map one image, s = x[n][p] (the caller folds [N][K][H][W] into
// N K images).  C >= 2: logits fp32 [N][C][H][W], s = x[n][c_pos][p] - x[n][c_neg][p], one fp32 subtraction; each n one image.
// Target, of the score's shape [N][H][W].  fp32: ignored iff t == (float)ignore_index, tested first; else positive iff t > 0.5.
// int64: ignored iff t == ignore_index; positive iff t == positive; every other value negative.  use_ignore == 0 ignores nothing.
// A segment is one image (per_image: S = N, L = H W) or all of them (S = 1, L = N H W); S L < 2^31.
//   errors    one streaming launch: sigma = +1 at a positive pixel, -1 otherwise; e = 1 - s sigma in fp32 (s sigma is exact, so e is one
//             rounding); r = e where the pixel is valid and e > 0, else +0; key = (~bits(r) & 0x7FFFFFFF) | fg << 31 with fg = valid and
//             positive; payload = the pixel's index in its segment; e_out (on request) = e, of every pixel
//   sort      egm_sort_pairs_u32 over bits [0, 31): descending r, ties by ascending pixel index.  An element with r = 0 (well
//             classified or ignored) sorts after every element with r > 0, has coef 0 and adds 0 to the loss, so the order taken on r
//             gives the official loss and gradient, no valid flag has to travel (V_j = j for every element whose g is used), and G,
//             the count of fg, is the number of valid positive pixels
//   counts, scan, apply, finalize    lovasz_core.h on LovKeyHinge, one plane: g_j = J(F_j, j) - J(F_j - fg_j, j - 1) in double, rounded
//             once; coef = -sigma g where r > 0, else 0, at the pixel's own place; L_s = sum r g in double in a fixed order;
//             L = (1 / S) sum_s L_s; out = {w L, L}
//   backward  one streaming launch: m = (grad_out * w) * (1.0f / S) (fp32 products in this order; grad_out NULL is 1);
//             C == 1: dx = m coef; C >= 2: dx[c_pos] = m coef, dx[c_neg] = -(m coef), every other channel +0.  Every element is
//             written, non-temporal stores.  There are no additions: nothing can be contracted
// The forward is 4 * 3 + 5 launches whatever N, the content and per_image (segments are a grid dimension).  No workgroup waits for
// another, every loop is bounded by the arguments, no atomics on global memory.  NaN or infinite logits are outside the specification;
// the sort takes any bits and the scatter's store is guarded.
#include "lovasz_core.h"

namespace {

// planes [N][HW]: keys, vals and (when not null) e_out.  TT: float or long long
template <int V, typename TT>
__global__ __launch_bounds__(256) void lovasz_hinge_errors_kernel(const float* __restrict__ logits, const TT* __restrict__ target, int C,
                                                                  int c_pos, int c_neg, long long HW, long long positive,
                                                                  long long ignore_index, int use_ignore, int per_image,
                                                                  unsigned int* __restrict__ keys, unsigned int* __restrict__ vals,
                                                                  float* __restrict__ e_out) {
    const int n = blockIdx.y;
    const float* xp = logits + ((long long)n * C + (C > 1 ? c_pos : 0)) * HW;
    const float* xn = C > 1 ? logits + ((long long)n * C + c_neg) * HW : nullptr;
    const long long img = (long long)n * HW, first = per_image ? 0 : img;
    const TT* tg = target + img;
    const float ign_f = (float)ignore_index;
    for (long long p = (blockIdx.x * 256LL + threadIdx.x) * V; p < HW; p += (long long)gridDim.x * 256 * V) {
        float sc[V];
        lov_load<V>(xp + p, sc);
        if (xn) {
            float b[V];
            lov_load<V>(xn + p, b);
#pragma unroll
            for (int v = 0; v < V; ++v) sc[v] = sc[v] - b[v];
        }
        TT t[V];
        if constexpr (sizeof(TT) == 4) {
            lov_load<V>(tg + p, t);
        } else {
#pragma unroll
            for (int v = 0; v < V; ++v) t[v] = tg[p + v];
        }
        unsigned int key[V], val[V], eb[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            bool valid, pos;
            if constexpr (sizeof(TT) == 4) {
                valid = !(use_ignore && t[v] == ign_f);
                pos = t[v] > 0.5f;
            } else {
                valid = !(use_ignore && t[v] == ignore_index);
                pos = t[v] == positive;
            }
            const bool fg = valid && pos;
            const float e = fg ? 1.f - sc[v] : 1.f + sc[v];    // 1 - s sigma: s sigma is s or -s, exact
            const float r = (valid && e > 0.f) ? e : 0.f;
            eb[v] = __float_as_uint(e);
            key[v] = (~__float_as_uint(r) & LovKeyHinge::kErrMask) | (fg ? LovKeyHinge::kFg : 0u);
            val[v] = (unsigned int)(first + p + v);
        }
        lov_store<V>(keys + img + p, key);
        lov_store<V>(vals + img + p, val);
        if (e_out) lov_store<V>(reinterpret_cast<unsigned int*>(e_out) + img + p, eb);
    }
}

// C == 1: dx[n][p] = m coef[n][p].  C >= 2: dx[n][c_pos] = m coef, dx[n][c_neg] = -(m coef), the other channels +0
template <int V>
__global__ __launch_bounds__(256) void lovasz_hinge_bwd_kernel(const float* __restrict__ coef, int C, int c_pos, int c_neg, long long HW,
                                                               float inv_s, const float* __restrict__ gout,
                                                               const float* __restrict__ w_dev, float* __restrict__ dlogits) {
    const int n = blockIdx.y;
    const float* cf = coef + (long long)n * HW;
    float* dl = dlogits + (long long)n * C * HW;
    const float m = ((gout ? gout[0] : 1.f) * w_dev[0]) * inv_s;
    for (long long p = (blockIdx.x * 256LL + threadIdx.x) * V; p < HW; p += (long long)gridDim.x * 256 * V) {
        float c4[V], g[V];
        lov_load<V>(cf + p, c4);
#pragma unroll
        for (int v = 0; v < V; ++v) g[v] = m * c4[v];
        if (C == 1) {
            lov_store_stream<V>(dl + p, g);
        } else {
            for (int c = 0; c < C; ++c) {
                float o[V];
#pragma unroll
                for (int v = 0; v < V; ++v) o[v] = c == c_pos ? g[v] : (c == c_neg ? -g[v] : 0.f);
                lov_store_stream<V>(dl + c * HW + p, o);
            }
        }
    }
}

// ---------------------------------------------------------------- host
struct HingeShape {
    int S, ntiles;
    long long L, NHW, HW;
};

inline int hinge_shape_check(const char* name, int N, int H, int W, int per_image, HingeShape& sh) {
    EGM_REQUIRE(N > 0 && H > 0 && W > 0, "%s: bad shape %d x %d x %d", name, N, H, W);
    EGM_REQUIRE(N <= 65535, "%s: %d images in one call, at most 65535 are supported", name, N);
    sh.HW = (long long)H * W;
    sh.NHW = sh.HW * N;
    EGM_REQUIRE(sh.NHW < (1ll << 31), "%s: %d x %d x %d pixels, S * L must stay below 2^31", name, N, H, W);
    sh.S = per_image ? N : 1;
    sh.L = per_image ? sh.HW : sh.NHW;
    sh.ntiles = (int)((sh.L + kLovTile - 1) / kLovTile);
    return EGM_OK;
}
inline int hinge_channels_check(const char* name, int C, int c_pos, int c_neg) {
    EGM_REQUIRE(C >= 1, "%s: %d channels", name, C);
    if (C > 1) {
        EGM_REQUIRE(c_pos >= 0 && c_pos < C && c_neg >= 0 && c_neg < C, "%s: channels (%d, %d) outside [0, %d)", name, c_pos, c_neg, C);
        EGM_REQUIRE(c_pos != c_neg, "%s: the positive and the negative channel are both %d", name, c_pos);
    }
    return EGM_OK;
}
inline bool hinge_vec4(long long HW, const void* a, const void* b, const void* c, const void* d, const void* e) {
    return HW % 4 == 0 && egm_aligned16(a) && (!b || egm_aligned16(b)) && (!c || egm_aligned16(c)) && (!d || egm_aligned16(d)) &&
           (!e || egm_aligned16(e));
}

inline int hinge_errors_launch(const float* logits, const void* target, int target_f32, int N, int C, int c_pos, int c_neg,
                               const HingeShape& sh, long long positive, long long ignore_index, int use_ignore, int per_image,
                               unsigned int* keys, unsigned int* vals, float* e_out, egm_stream_t s) {
    // an fp32 target is read four at a time too; an int64 one element by element
    const bool vec4 = hinge_vec4(sh.HW, logits, keys, vals, e_out, target_f32 ? target : nullptr);
    const dim3 grid(kLovBlocks, N), block(256);
#define EGM_HINGE_ERRORS(V, TT)                                                                                                          \
    hipLaunchKernelGGL((lovasz_hinge_errors_kernel<V, TT>), grid, block, 0, (hipStream_t)s, logits, reinterpret_cast<const TT*>(target), \
                       C, c_pos, c_neg, sh.HW, positive, ignore_index, use_ignore ? 1 : 0, per_image ? 1 : 0, keys, vals, e_out)
    if (target_f32) {
        if (vec4) EGM_HINGE_ERRORS(4, float);
        else EGM_HINGE_ERRORS(1, float);
    } else {
        if (vec4) EGM_HINGE_ERRORS(4, long long);
        else EGM_HINGE_ERRORS(1, long long);
    }
#undef EGM_HINGE_ERRORS
    EGM_CHECK_LAUNCH("lovasz_hinge_errors");
    return EGM_OK;
}

}  // namespace

extern "C" long long egm_lovasz_hinge_workspace(int N, int H, int W, int per_image) {
    HingeShape sh;
    if (hinge_shape_check("lovasz_hinge_workspace", N, H, W, per_image, sh) != EGM_OK) return EGM_ERR_ARG;
    return lov_planes(nullptr, 1, sh.S, sh.L, sh.ntiles).bytes;
}

extern "C" int egm_lovasz_hinge_errors(const float* logits, const void* target, int target_f32, int N, int C, int c_pos, int c_neg, int H,
                                       int W, long long positive, long long ignore_index, int use_ignore, int per_image,
                                       unsigned int* keys, unsigned int* vals, float* e_out, egm_stream_t s) {
    const char* name = "lovasz_hinge_errors";
    HingeShape sh;
    if (hinge_shape_check(name, N, H, W, per_image, sh) != EGM_OK || hinge_channels_check(name, C, c_pos, c_neg) != EGM_OK) return EGM_ERR_ARG;
    EGM_REQUIRE(logits && target && keys && vals, "%s: null pointer", name);
    return hinge_errors_launch(logits, target, target_f32, N, C, c_pos, c_neg, sh, positive, ignore_index, use_ignore, per_image, keys, vals,
                               e_out, s);
}

extern "C" int egm_lovasz_hinge_coefs(const float* logits, const void* target, int target_f32, int N, int C, int c_pos, int c_neg, int H,
                                      int W, long long positive, long long ignore_index, int use_ignore, int per_image, void* workspace,
                                      float* e_out, float* coef, egm_stream_t s) {
    const char* name = "lovasz_hinge_coefs";
    HingeShape sh;
    if (hinge_shape_check(name, N, H, W, per_image, sh) != EGM_OK || hinge_channels_check(name, C, c_pos, c_neg) != EGM_OK) return EGM_ERR_ARG;
    EGM_REQUIRE(logits && target && workspace && coef, "%s: null pointer", name);
    EGM_REQUIRE(egm_aligned16(workspace), "%s: the workspace must be 16-byte aligned", name);
    const LovPlanes pl = lov_planes(workspace, 1, sh.S, sh.L, sh.ntiles);
    const int rc = hinge_errors_launch(logits, target, target_f32, N, C, c_pos, c_neg, sh, positive, ignore_index, use_ignore, per_image,
                                       pl.keys, pl.vals, e_out, s);
    if (rc != EGM_OK) return rc;
    return lov_rank_run<LovKeyHinge>(name, sh.S, sh.L, sh.ntiles, pl, coef, s);
}

extern "C" int egm_lovasz_hinge_fwd(const float* logits, const void* target, int target_f32, int N, int C, int c_pos, int c_neg, int H,
                                    int W, long long positive, long long ignore_index, int use_ignore, int per_image, const float* w_dev,
                                    void* workspace, float* coef, float* out2, egm_stream_t s) {
    const char* name = "lovasz_hinge_fwd";
    HingeShape sh;
    if (hinge_shape_check(name, N, H, W, per_image, sh) != EGM_OK || hinge_channels_check(name, C, c_pos, c_neg) != EGM_OK) return EGM_ERR_ARG;
    EGM_REQUIRE(logits && target && w_dev && workspace && coef && out2, "%s: null pointer", name);
    EGM_REQUIRE(egm_aligned16(workspace), "%s: the workspace must be 16-byte aligned", name);
    const LovPlanes pl = lov_planes(workspace, 1, sh.S, sh.L, sh.ntiles);
    int rc = hinge_errors_launch(logits, target, target_f32, N, C, c_pos, c_neg, sh, positive, ignore_index, use_ignore, per_image, pl.keys,
                                 pl.vals, nullptr, s);
    if (rc != EGM_OK) return rc;
    rc = lov_rank_run<LovKeyHinge>(name, sh.S, sh.L, sh.ntiles, pl, coef, s);
    if (rc != EGM_OK) return rc;
    return lov_finalize_run("lovasz_hinge_fwd (finalize)", 1, sh.S, sh.ntiles, 0, w_dev, pl, out2, s);
}

extern "C" int egm_lovasz_hinge_bwd(const float* coef, int N, int C, int c_pos, int c_neg, int H, int W, int per_image,
                                    const float* grad_out, const float* w_dev, float* dlogits, egm_stream_t s) {
    const char* name = "lovasz_hinge_bwd";
    HingeShape sh;
    if (hinge_shape_check(name, N, H, W, per_image, sh) != EGM_OK || hinge_channels_check(name, C, c_pos, c_neg) != EGM_OK) return EGM_ERR_ARG;
    EGM_REQUIRE(coef && w_dev && dlogits, "%s: null pointer", name);
    const float inv_s = 1.0f / (float)sh.S;
    const dim3 grid(kLovBlocks, N), block(256);
    if (hinge_vec4(sh.HW, coef, dlogits, nullptr, nullptr, nullptr))
        hipLaunchKernelGGL(lovasz_hinge_bwd_kernel<4>, grid, block, 0, (hipStream_t)s, coef, C, c_pos, c_neg, sh.HW, inv_s, grad_out, w_dev,
                           dlogits);
    else
        hipLaunchKernelGGL(lovasz_hinge_bwd_kernel<1>, grid, block, 0, (hipStream_t)s, coef, C, c_pos, c_neg, sh.HW, inv_s, grad_out, w_dev,
                           dlogits);
    EGM_CHECK_LAUNCH(name);
    return EGM_OK;
}
