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
#include "common.h"

namespace {

constexpr int kLovMaxC = 16;                   // channels, and classes per call
constexpr int kLovBlocks = 256;                // workgroups per image of the streaming passes
constexpr int kLovItems = 8;
constexpr int kLovTile = 256 * kLovItems;      // sorted elements per workgroup of the count and apply passes
constexpr int kLovEndBit = 30;                 // the keys of e in [0, 1] vary in bits 0..29
constexpr unsigned int kLovErrMask = 0x3FFFFFFFu, kLovFg = 1u << 30, kLovValid = 1u << 31;

struct LovClasses { int id[kLovMaxC]; };

template <int V, typename T>
__device__ __forceinline__ void lov_load(const T* __restrict__ p, T (&v)[V]) {
    static_assert(V == 1 || (V == 4 && sizeof(T) == 4), "one value, or four of four bytes");
    if constexpr (V == 1) v[0] = p[0];
    else __builtin_memcpy(v, __builtin_assume_aligned(p, 16), 16);
}
template <int V>
__device__ __forceinline__ void lov_store(unsigned int* __restrict__ p, const unsigned int (&v)[V]) {
    if constexpr (V == 1) p[0] = v[0];
    else *reinterpret_cast<uint4*>(p) = make_uint4(v[0], v[1], v[2], v[3]);
}

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

// counts[seg][tile] = {foreground, valid} elements of the tile
__global__ __launch_bounds__(256) void lovasz_counts_kernel(const unsigned int* __restrict__ skeys, int L, int ntiles,
                                                            uint2* __restrict__ counts) {
    __shared__ unsigned int red[4];
    const int tile = blockIdx.x, seg = blockIdx.y;
    const unsigned int* k = skeys + (long long)seg * L;
    unsigned int x = 0u;                                       // fg | valid << 16: at most 2048 of each
#pragma unroll
    for (int i = 0; i < kLovItems; ++i) {
        const long long idx = (long long)tile * kLovTile + i * 256 + threadIdx.x;
        const unsigned int key = idx < L ? k[idx] : 0u;
        x += ((key >> 30) & 1u) + ((key >> 31) << 16);
    }
    x = wave_sum_u32(x);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        x = red[0] + red[1] + red[2] + red[3];
        counts[(long long)seg * ntiles + tile] = make_uint2(x & 0xFFFFu, x >> 16);
    }
}

// exclusive prefix of a segment's tile counts in place; totals[seg] = {G, V}
__global__ __launch_bounds__(1024) void lovasz_scan_kernel(uint2* __restrict__ counts, int ntiles, uint2* __restrict__ totals) {
    __shared__ uint2 wsum[16];
    uint2* c = counts + (long long)blockIdx.x * ntiles;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint2 carry = make_uint2(0u, 0u);
    for (int base = 0; base < ntiles; base += 1024) {
        const int at = base + threadIdx.x;
        const uint2 own = at < ntiles ? c[at] : make_uint2(0u, 0u);
        uint2 x = own;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned int yx = __shfl_up(x.x, o, 64), yy = __shfl_up(x.y, o, 64);
            if (lane >= o) { x.x += yx; x.y += yy; }
        }
        if (lane == 63) wsum[wv] = x;
        __syncthreads();
        uint2 before = make_uint2(0u, 0u), total = make_uint2(0u, 0u);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint2 w = wsum[i];
            if (i < wv) { before.x += w.x; before.y += w.y; }
            total.x += w.x; total.y += w.y;
        }
        if (at < ntiles) c[at] = make_uint2(carry.x + before.x + x.x - own.x, carry.y + before.y + x.y - own.y);
        carry.x += total.x; carry.y += total.y;
        __syncthreads();
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// the Jaccard index of the extension after F foreground among V valid elements, G foreground in all
__device__ __forceinline__ double lov_jaccard(unsigned int G, unsigned int F, unsigned int V) {
    return 1.0 - (double)(G - F) / ((double)G + (double)V - (double)F);
}

__global__ __launch_bounds__(256) void lovasz_apply_kernel(const unsigned int* __restrict__ skeys, const unsigned int* __restrict__ svals,
                                                           int L, int ntiles, const uint2* __restrict__ counts,
                                                           const uint2* __restrict__ totals, float* __restrict__ coef,
                                                           double* __restrict__ partials) {
    __shared__ unsigned int wtot[4];
    __shared__ double red[4];
    const int tile = blockIdx.x, seg = blockIdx.y;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long off = (long long)seg * L;
    const long long base = (long long)tile * kLovTile + wv * (64 * kLovItems) + lane;     // (wave, round, lane): the sorted order
    unsigned int key[kLovItems], val[kLovItems], inc[kLovItems];
    unsigned int run = 0u;                                     // fg | valid << 16 of the wave's earlier rounds
#pragma unroll
    for (int i = 0; i < kLovItems; ++i) {
        const long long idx = base + i * 64;
        key[i] = idx < L ? skeys[off + idx] : 0u;
        val[i] = idx < L ? svals[off + idx] : 0u;
        unsigned int x = ((key[i] >> 30) & 1u) + ((key[i] >> 31) << 16);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned int y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        inc[i] = run + x;
        run += __shfl(x, 63, 64);
    }
    if (lane == 0) wtot[wv] = run;
    __syncthreads();
    unsigned int before = 0u;
#pragma unroll
    for (int w = 0; w < 4; ++w) before += w < wv ? wtot[w] : 0u;
    const uint2 t0 = counts[(long long)seg * ntiles + tile];
    const unsigned int G = totals[seg].x;
    const unsigned int f0 = t0.x + (before & 0xFFFFu), v0 = t0.y + (before >> 16);
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < kLovItems; ++i) {
        const long long idx = base + i * 64;
        if (idx >= L) continue;
        const unsigned int fg = (key[i] >> 30) & 1u, valid = key[i] >> 31;
        const unsigned int F = f0 + (inc[i] & 0xFFFFu), V = v0 + (inc[i] >> 16);
        const float e = __uint_as_float(~key[i] & kLovErrMask);
        float g = 0.f;
        if (valid) {
            const double j1 = lov_jaccard(G, F, V);
            const double j0 = V == 1u ? 0.0 : lov_jaccard(G, F - fg, V - 1u);
            g = (float)(j1 - j0);
        }
        acc += (double)e * (double)g;
        const float cf = e == 0.f ? 0.f : (fg ? -g : g);      // sign(p_c - fg) g: p_c <= 1 = fg, or p_c >= 0 = fg
        if (val[i] < (unsigned int)L) coef[off + val[i]] = cf;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) red[wv] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[(long long)seg * ntiles + tile] = (red[0] + red[1]) + (red[2] + red[3]);
}

// one workgroup.  lsk[k S + s] = L_{s,k}, lseg[s] = L_s, scale[k S + s] = 1 / (S P_s) where class k counts in segment s, else 0
__global__ __launch_bounds__(1024) void lovasz_finalize_kernel(const double* __restrict__ partials, const uint2* __restrict__ totals,
                                                               int ntiles, int K, int S, int present, const float* __restrict__ w_dev,
                                                               double* __restrict__ lsk, double* __restrict__ lseg,
                                                               float* __restrict__ scale, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int pair = wv; pair < K * S; pair += 16) {
        double s = 0.0;
        for (int i = lane; i < ntiles; i += 64) s += partials[(long long)pair * ntiles + i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) lsk[pair] = s;
    }
    __syncthreads();
    for (int s = threadIdx.x; s < S; s += 1024) {
        int P = 0;
        double acc = 0.0;
        for (int k = 0; k < K; ++k)
            if (!present || totals[k * S + s].x > 0u) { ++P; acc += lsk[k * S + s]; }
        lseg[s] = P ? acc / (double)P : 0.0;
        const float inv = P ? (float)(1.0 / ((double)S * (double)P)) : 0.f;
        for (int k = 0; k < K; ++k) scale[k * S + s] = (!present || totals[k * S + s].x > 0u) ? inv : 0.f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double l = 0.0;
        for (int s = 0; s < S; ++s) l += lseg[s];
        const float lf = (float)(l / (double)S);
        out[0] = w_dev[0] * lf;
        out[1] = lf;
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
struct LovPlanes {                                             // the workspace, every plane at a 16-byte boundary
    unsigned int *keys, *vals, *skeys, *svals;
    unsigned char* sort_ws;
    uint2 *counts, *totals;
    double *partials, *lsk, *lseg;
    float* scale;
    long long bytes;
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
inline long long lov_up16(long long b) { return (b + 15) / 16 * 16; }
inline LovPlanes lov_planes(void* workspace, const LovShape& sh, int K) {
    LovPlanes pl;
    unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
    const long long plane = lov_up16((long long)K * sh.NHW * 4), pairs = (long long)K * sh.S;
    const long long sort_bytes = lov_up16(egm_sort_pairs_workspace((int)pairs, sh.L));
    long long at = 0;
    pl.keys = reinterpret_cast<unsigned int*>(w + at); at += plane;
    pl.vals = reinterpret_cast<unsigned int*>(w + at); at += plane;
    pl.skeys = reinterpret_cast<unsigned int*>(w + at); at += plane;
    pl.svals = reinterpret_cast<unsigned int*>(w + at); at += plane;
    pl.sort_ws = w + at; at += sort_bytes;
    pl.counts = reinterpret_cast<uint2*>(w + at); at += lov_up16(pairs * sh.ntiles * 8);
    pl.totals = reinterpret_cast<uint2*>(w + at); at += lov_up16(pairs * 8);
    pl.partials = reinterpret_cast<double*>(w + at); at += lov_up16(pairs * sh.ntiles * 8);
    pl.lsk = reinterpret_cast<double*>(w + at); at += lov_up16(pairs * 8);
    pl.lseg = reinterpret_cast<double*>(w + at); at += lov_up16((long long)sh.S * 8);
    pl.scale = reinterpret_cast<float*>(w + at); at += lov_up16(pairs * 4);
    pl.bytes = at;
    return pl;
}
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
    const int pairs = K * sh.S;
    const int rc = egm_sort_pairs_u32(pl.keys, pl.vals, pairs, sh.L, 0, kLovEndBit, pl.sort_ws, pl.skeys, pl.svals, s);
    if (rc != EGM_OK) return rc;
    const dim3 grid(sh.ntiles, pairs);
    hipLaunchKernelGGL(lovasz_counts_kernel, grid, dim3(256), 0, (hipStream_t)s, pl.skeys, (int)sh.L, sh.ntiles, pl.counts);
    EGM_CHECK_LAUNCH("lovasz (counts)");
    hipLaunchKernelGGL(lovasz_scan_kernel, dim3(pairs), dim3(1024), 0, (hipStream_t)s, pl.counts, sh.ntiles, pl.totals);
    EGM_CHECK_LAUNCH("lovasz (scan)");
    hipLaunchKernelGGL(lovasz_apply_kernel, grid, dim3(256), 0, (hipStream_t)s, pl.skeys, pl.svals, (int)sh.L, sh.ntiles, pl.counts, pl.totals,
                       coef, pl.partials);
    EGM_CHECK_LAUNCH("lovasz (apply)");
    (void)name;
    return EGM_OK;
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
    hipLaunchKernelGGL(lovasz_finalize_kernel, dim3(1), dim3(1024), 0, (hipStream_t)s, pl.partials, pl.totals, sh.ntiles, K, sh.S,
                       present ? 1 : 0, w_dev, pl.lsk, pl.lseg, pl.scale, out2);
    EGM_CHECK_LAUNCH("lovasz_fwd (finalize)");
    return EGM_OK;
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
