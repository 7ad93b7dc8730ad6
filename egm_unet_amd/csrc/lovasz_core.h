// What the two Lovasz losses share (lovasz.hip: Lovasz-Softmax; lovasz_hinge.hip: the Lovasz hinge):
// everything between the sort and the backward.  Along the stably sorted (key, payload) pairs of every segment
//   counts    per tile of kLovTile sorted elements the number of foreground and of valid ones (plain stores)
//   scan      one workgroup per segment: exclusive prefix of the tile counts in place, and the segment's totals {G, V}
//   apply     per tile: the inclusive counts F_j, V_j of every element from a wave scan of (fg | valid << 16), the wave and tile
//             offsets; g_j = J(F_j, V_j) - J(F_j - fg_j, V_j - 1) in double, rounded once; coef = -g on foreground, +g elsewhere (0 where
//             the error is 0) scattered to the element's own place in the coef plane; one double partial of e g per workgroup
//   finalize  one workgroup: the partials per (class, segment) in a fixed order in double, which classes count, L_s, L -> out = {w L, L}
// The losses differ in what a key holds; a key layout KL names it:
//   KL::kEndBit       the sort runs over key bits [0, kEndBit): ~bits(e) of the error, so ascending keys are descending errors
//   KL::flags(key)    fg | valid << 16 of an element
//   KL::error(key)    the fp32 error the key was made from
// No workgroup waits for another, every loop is bounded by the arguments, no atomics on global memory; each element makes g from its
// own two counts, so no neighbour's value is read.
#pragma once
#include "common.h"

namespace {

constexpr int kLovBlocks = 256;                // workgroups per image of the streaming passes
constexpr int kLovItems = 8;
constexpr int kLovTile = 256 * kLovItems;      // sorted elements per workgroup of the count and apply passes

// Lovasz-Softmax: e in [0, 1], so bits(e) <= 0x3F800000 fits 30 bits; fg in bit 30, valid in bit 31
struct LovKeySoftmax {
    static constexpr int kEndBit = 30;
    static constexpr unsigned int kErrMask = 0x3FFFFFFFu, kFg = 1u << 30, kValid = 1u << 31;
    static __device__ __forceinline__ unsigned int flags(unsigned int key) { return ((key >> 30) & 1u) + ((key >> 31) << 16); }
    static __device__ __forceinline__ float error(unsigned int key) { return __uint_as_float(~key & kErrMask); }
};
// Lovasz hinge: r = max(e, +0) at a valid pixel, +0 at an ignored one: any non-negative float, 31 bits; fg in bit 31.  Every element
// counts as valid: one with r > 0 has only valid ones in front of it (V_j = j), and one with r = 0 has coef 0 and adds 0 to the loss
struct LovKeyHinge {
    static constexpr int kEndBit = 31;
    static constexpr unsigned int kErrMask = 0x7FFFFFFFu, kFg = 1u << 31;
    static __device__ __forceinline__ unsigned int flags(unsigned int key) { return (key >> 31) + (1u << 16); }
    static __device__ __forceinline__ float error(unsigned int key) { return __uint_as_float(~key & kErrMask); }
};

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
// the element-wise kernels' store policy (common.h, EGM_STORE_MODE)
template <int V>
__device__ __forceinline__ void lov_store_stream(float* __restrict__ p, const float (&g)[V]) {
    if constexpr (V == 1) {
        __builtin_nontemporal_store(g[0], p);
    } else {
        egm_u32x4 a;
        a.x = __float_as_uint(g[0]); a.y = __float_as_uint(g[1]); a.z = __float_as_uint(g[2]); a.w = __float_as_uint(g[3]);
        egm_store16_as<EGM_STORE_MODE>(p, a);
    }
}

// counts[seg][tile] = {foreground, valid} elements of the tile
template <class KL>
__global__ __launch_bounds__(256) void lovasz_counts_kernel(const unsigned int* __restrict__ skeys, int L, int ntiles,
                                                            uint2* __restrict__ counts) {
    __shared__ unsigned int red[4];
    const int tile = blockIdx.x, seg = blockIdx.y;
    const unsigned int* k = skeys + (long long)seg * L;
    unsigned int x = 0u;                                       // fg | valid << 16: at most 2048 of each
#pragma unroll
    for (int i = 0; i < kLovItems; ++i) {
        const long long idx = (long long)tile * kLovTile + i * 256 + threadIdx.x;
        x += idx < L ? KL::flags(k[idx]) : 0u;
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

template <class KL>
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
    unsigned int key[kLovItems], val[kLovItems], inc[kLovItems], own[kLovItems];
    unsigned int run = 0u;                                     // fg | valid << 16 of the wave's earlier rounds
#pragma unroll
    for (int i = 0; i < kLovItems; ++i) {
        const long long idx = base + i * 64;
        key[i] = idx < L ? skeys[off + idx] : 0u;
        val[i] = idx < L ? svals[off + idx] : 0u;
        own[i] = idx < L ? KL::flags(key[i]) : 0u;
        unsigned int x = own[i];
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
        const unsigned int fg = own[i] & 1u, valid = own[i] >> 16;
        const unsigned int F = f0 + (inc[i] & 0xFFFFu), V = v0 + (inc[i] >> 16);
        const float e = KL::error(key[i]);
        float g = 0.f;
        if (valid) {
            const double j1 = lov_jaccard(G, F, V);
            const double j0 = V == 1u ? 0.0 : lov_jaccard(G, F - fg, V - 1u);
            g = (float)(j1 - j0);
        }
        acc += (double)e * (double)g;
        // softmax: sign(p_c - fg) g with p_c <= 1 = fg, or p_c >= 0 = fg; hinge: -sigma g
        const float cf = e == 0.f ? 0.f : (fg ? -g : g);
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

// ---------------------------------------------------------------- host
struct LovPlanes {                                             // the workspace, every plane at a 16-byte boundary
    unsigned int *keys, *vals, *skeys, *svals;
    unsigned char* sort_ws;
    uint2 *counts, *totals;
    double *partials, *lsk, *lseg;
    float* scale;
    long long bytes;
};

inline long long lov_up16(long long b) { return (b + 15) / 16 * 16; }
// K planes of S segments of L elements each
inline LovPlanes lov_planes(void* workspace, int K, int S, long long L, int ntiles) {
    LovPlanes pl;
    unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
    const long long plane = lov_up16((long long)K * S * L * 4), pairs = (long long)K * S;
    const long long sort_bytes = lov_up16(egm_sort_pairs_workspace((int)pairs, L));
    long long at = 0;
    pl.keys = reinterpret_cast<unsigned int*>(w + at); at += plane;
    pl.vals = reinterpret_cast<unsigned int*>(w + at); at += plane;
    pl.skeys = reinterpret_cast<unsigned int*>(w + at); at += plane;
    pl.svals = reinterpret_cast<unsigned int*>(w + at); at += plane;
    pl.sort_ws = w + at; at += sort_bytes;
    pl.counts = reinterpret_cast<uint2*>(w + at); at += lov_up16(pairs * ntiles * 8);
    pl.totals = reinterpret_cast<uint2*>(w + at); at += lov_up16(pairs * 8);
    pl.partials = reinterpret_cast<double*>(w + at); at += lov_up16(pairs * ntiles * 8);
    pl.lsk = reinterpret_cast<double*>(w + at); at += lov_up16(pairs * 8);
    pl.lseg = reinterpret_cast<double*>(w + at); at += lov_up16((long long)S * 8);
    pl.scale = reinterpret_cast<float*>(w + at); at += lov_up16(pairs * 4);
    pl.bytes = at;
    return pl;
}

// the sort of pl.keys / pl.vals over the bits the layout's errors vary in, then counts, scan, apply: 4 * 3 + 3 launches
template <class KL>
inline int lov_rank_run(const char* name, int pairs, long long L, int ntiles, const LovPlanes& pl, float* coef, egm_stream_t s) {
    const int rc = egm_sort_pairs_u32(pl.keys, pl.vals, pairs, L, 0, KL::kEndBit, pl.sort_ws, pl.skeys, pl.svals, s);
    if (rc != EGM_OK) return rc;
    const dim3 grid(ntiles, pairs);
    hipLaunchKernelGGL(lovasz_counts_kernel<KL>, grid, dim3(256), 0, (hipStream_t)s, pl.skeys, (int)L, ntiles, pl.counts);
    EGM_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(lovasz_scan_kernel, dim3(pairs), dim3(1024), 0, (hipStream_t)s, pl.counts, ntiles, pl.totals);
    EGM_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(lovasz_apply_kernel<KL>, grid, dim3(256), 0, (hipStream_t)s, pl.skeys, pl.svals, (int)L, ntiles, pl.counts, pl.totals,
                       coef, pl.partials);
    EGM_CHECK_LAUNCH(name);
    return EGM_OK;
}
inline int lov_finalize_run(const char* name, int K, int S, int ntiles, int present, const float* w_dev, const LovPlanes& pl, float* out2,
                            egm_stream_t s) {
    hipLaunchKernelGGL(lovasz_finalize_kernel, dim3(1), dim3(1024), 0, (hipStream_t)s, pl.partials, pl.totals, ntiles, K, S, present ? 1 : 0,
                       w_dev, pl.lsk, pl.lseg, pl.scale, out2);
    EGM_CHECK_LAUNCH(name);
    return EGM_OK;
}

}  // namespace
