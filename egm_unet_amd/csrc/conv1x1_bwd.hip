// 1x1 convolution backward: data gradient + weight-gradient slabs in ONE pass over dy and x.
//
// dx = dy W and dW = dy^T x of a 1x1 convolution both read dy; as two kernels (the data-gradient conv and the weight-gradient slab
// kernel) dy is pulled from memory twice and each launch pays its own start-up on tensors that take 10-30 us at the roofline.  Here a
// wave stages its 32-pixel tile of x and dy once (coalesced 16-byte loads, next tile prefetched into registers), multiplies
// dx = wd . dy from row reads of the dy image and accumulates dW += dy^T x from transposing reads of both images; no element-wise work
// at all.  Every wave is an independent stream processor: it multiplies from its own LDS images and stores dx through its own
// transposition tile; the weights are staged once per workgroup, so the tile loop contains no workgroup barrier.
// grid.y = 64-channel blocks of Cin: a workgroup owns the dx channels and the dW columns of its block and reads only those x channels.
// One slab [CoutP][CinP] per workgroup column (waves summed through LDS in wave order: bitwise reproducible), laid out like
// conv_wgrad.hip's slabs, so the deferred multi-conv reduction (egm_wgrad_reduce_multi) finishes them.
// Templated on the storage type: bf16 = v_mfma_f32_32x32x16_bf16, fp32 = v_mfma_f32_32x32x2_f32 (exact).
// Limits: padded Cin, Cout <= 128, <= 4 convolutions per launch.
#include "common.h"
#include <algorithm>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((ext_vector_type(8))) short s16x8_t;

namespace {

constexpr int C1_MAXP = 4, C1_MAXC = 128;                   // convolutions per launch, padded channels per side
constexpr int C1_LDS_BUDGET = 150 * 1024;

__host__ __device__ inline int r32(int v) { return (v + 31) & ~31; }

// ---------------------------------------------------------------- element traits
template <typename T> struct Pw;
template <> struct Pw<bf16_t> {
    static constexpr int ESZ = 2, VEC = 8, BLK = 2048, ROW = 64;
    struct Frag { bf16x8_t v; };
    // byte offset, inside an image of [32-ch block][32 pixels][32 ch], of the 16-byte slot holding channels [c, c + 8) of pixel p.  The
    // slot index is XOR-swizzled with (p >> 2) & 3: the row reads (16 B per lane, 16 lanes = pixels {0-3, 12-15, 20-27} per LDS cycle)
    // and the transposing reads (four consecutive rows of 64 B per 32 lanes) are both bank-conflict free.
    static __device__ __forceinline__ int slot_off(int p, int c) { return (c >> 5) * BLK + p * ROW + ((((c & 31) >> 3) ^ ((p >> 2) & 3)) << 4); }
    static __device__ __forceinline__ Frag row_frag(const unsigned char* img, int p, int c) {
        Frag f; f.v = *reinterpret_cast<const bf16x8_t*>(img + slot_off(p, c)); return f;
    }
    static __device__ __forceinline__ Frag lin_frag(const unsigned char* row, int c) {           // unswizzled row-major image (weights)
        Frag f; f.v = *reinterpret_cast<const bf16x8_t*>(row + c * 2); return f;
    }
    // rows (channels of block blk) lane & 31, k = pixels pix0 + 8 * (lane >> 5) + 0..7   (ds_read_b64_tr_b16, as conv_wgrad.hip)
    static __device__ __forceinline__ Frag col_frag(const unsigned char* blk, int pix0, int lane) {
        const int gq = lane >> 4, t = lane & 15;
        const int r0 = pix0 + 8 * (gq >> 1) + (t >> 2), r1 = r0 + 4;
        const int slot = (gq & 1) * 2 + ((t & 3) >> 1), ins = (t & 1) * 8;
        typedef __attribute__((address_space(3))) s16x4_t* lds_ptr_t;
        s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr_t)(blk + r0 * ROW + ((slot ^ ((r0 >> 2) & 3)) << 4) + ins));
        s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr_t)(blk + r1 * ROW + ((slot ^ ((r1 >> 2) & 3)) << 4) + ins));
        s16x8_t v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        Frag f; f.v = __builtin_bit_cast(bf16x8_t, v); return f;
    }
    static __device__ __forceinline__ f32x16_t mma(const Frag& a, const Frag& b, f32x16_t c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, b.v, c, 0, 0, 0);
    }
    static __device__ __forceinline__ void put4(unsigned char* dst, float a, float b, float c, float d) {
        uint2 v;
        v.x = (uint32_t)f32_to_bf16(a) | ((uint32_t)f32_to_bf16(b) << 16);
        v.y = (uint32_t)f32_to_bf16(c) | ((uint32_t)f32_to_bf16(d) << 16);
        *reinterpret_cast<uint2*>(dst) = v;
    }
};
template <> struct Pw<float> {
    static constexpr int ESZ = 4, VEC = 4, BLK = 4096, ROW = 128;
    struct Frag { float v[8]; };
    static __device__ __forceinline__ int slot_off(int p, int c) { return (c >> 5) * BLK + p * ROW + (c & 31) * 4; }
    static __device__ __forceinline__ Frag row_frag(const unsigned char* img, int p, int c) {
        Frag f;
        const float4 a = *reinterpret_cast<const float4*>(img + slot_off(p, c)), b = *reinterpret_cast<const float4*>(img + slot_off(p, c + 4));
        f.v[0] = a.x; f.v[1] = a.y; f.v[2] = a.z; f.v[3] = a.w; f.v[4] = b.x; f.v[5] = b.y; f.v[6] = b.z; f.v[7] = b.w;
        return f;
    }
    static __device__ __forceinline__ Frag lin_frag(const unsigned char* row, int c) {
        Frag f;
        const float4 a = *reinterpret_cast<const float4*>(row + c * 4), b = *reinterpret_cast<const float4*>(row + c * 4 + 16);
        f.v[0] = a.x; f.v[1] = a.y; f.v[2] = a.z; f.v[3] = a.w; f.v[4] = b.x; f.v[5] = b.y; f.v[6] = b.z; f.v[7] = b.w;
        return f;
    }
    static __device__ __forceinline__ Frag col_frag(const unsigned char* blk, int pix0, int lane) {
        Frag f;
#pragma unroll
        for (int j = 0; j < 8; ++j) f.v[j] = *reinterpret_cast<const float*>(blk + (pix0 + 8 * (lane >> 5) + j) * ROW + (lane & 31) * 4);
        return f;
    }
    // k-slot (lane >> 5) of MFMA j stands for k = 8 * (lane >> 5) + j in BOTH operands: eight 32x32x2 steps = one 16-deep product
    static __device__ __forceinline__ f32x16_t mma(const Frag& a, const Frag& b, f32x16_t c) {
#pragma unroll
        for (int j = 0; j < 8; ++j) c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.v[j], b.v[j], c, 0, 0, 0);
        return c;
    }
    static __device__ __forceinline__ void put4(unsigned char* dst, float a, float b, float c, float d) {
        *reinterpret_cast<float4*>(dst) = make_float4(a, b, c, d);
    }
};

__device__ __forceinline__ void wave_fence() {           // same-wave LDS traffic is in order; this only stops the compiler from reordering it
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

// ---------------------------------------------------------------- staging of one 32-pixel x nc-channel tile (channels [c_lo, c_lo + nc))
// K = 16-byte vectors per lane (compile time); vector v = it * 64 + lane -> (pixel v / nvec, channel vector v % nvec).  The per-lane
// offsets are computed ONCE (StageMap) -- the divisions and the swizzle are not part of the tile loop.
template <int K> struct StageMap { int goff[K]; int loff[K]; int px[K]; };     // global element offset, LDS byte offset, pixel (32 = none)
template <typename T, int K>
__device__ __forceinline__ void stage_map(StageMap<K>& m, int ldx, int c_lo, int nc, int Cin, int lane) {
    constexpr int VEC = Pw<T>::VEC;
    const int nvec = nc / VEC;
#pragma unroll
    for (int it = 0; it < K; ++it) {
        const int v = it * 64 + lane;
        const int px = v / nvec, cv = v - px * nvec;
        const bool ok = px < 32 && c_lo + cv * VEC < Cin;
        m.px[it] = ok ? px : 32;
        m.goff[it] = px * ldx + c_lo + cv * VEC;
        m.loff[it] = px < 32 ? Pw<T>::slot_off(px, cv * VEC) : -1;
    }
}
template <typename T, int K>
__device__ __forceinline__ void tile_load(uint4 (&r)[K], const T* __restrict__ x, int ldx, long long pix0, long long npix, const StageMap<K>& m) {
    const T* base = x + pix0 * ldx;
    const int left = (int)(npix - pix0 < 32 ? npix - pix0 : 32);
#pragma unroll
    for (int it = 0; it < K; ++it) {
        r[it] = make_uint4(0, 0, 0, 0);
        if (m.px[it] < left) r[it] = *reinterpret_cast<const uint4*>(base + m.goff[it]);
    }
}
template <typename T, int K>
__device__ __forceinline__ void tile_store(const uint4 (&r)[K], unsigned char* img, const StageMap<K>& m) {
#pragma unroll
    for (int it = 0; it < K; ++it)
        if (m.loff[it] >= 0) *reinterpret_cast<uint4*>(img + m.loff[it]) = r[it];
}
template <typename T> __device__ __forceinline__ void image_zero(unsigned char* img, int nblk, int lane) {
    for (int i = lane; i < nblk * Pw<T>::BLK / 16; i += 64) reinterpret_cast<uint4*>(img)[i] = make_uint4(0, 0, 0, 0);
}

__device__ __forceinline__ int pow2_ge(int v) { int p = 1; while (p < v) p <<= 1; return p; }

// ================================================================= the kernel
// blk0: first workgroup (x index) of a problem in a merged launch; nparts: its waves, the stride of a wave's tile loop
struct C1Prob { const void* x; const void* dy; const void* wd; void* dx; float* slab; long long npix; int ldx, lddy, lddx, Cin, Cout, ntiles, nparts, blk0; };
struct C1Launch { int n, nw; C1Prob p[C1_MAXP]; };
struct C1Geom { int Cout32, WDRB, wd_bytes, wave_off, x_bytes, dy_bytes, tile_rb, tile_bytes, wave_bytes; };
template <typename T>
__host__ __device__ inline C1Geom c1_geom(int Cout) {
    constexpr int ESZ = Pw<T>::ESZ;
    C1Geom g;
    g.Cout32 = r32(Cout);
    g.WDRB = g.Cout32 * ESZ + 16;
    g.wd_bytes = 64 * g.WDRB;
    g.wave_off = g.wd_bytes;
    g.x_bytes = 2 * Pw<T>::BLK;
    g.dy_bytes = g.Cout32 / 32 * Pw<T>::BLK;
    g.tile_rb = 64 * ESZ + 16;
    g.tile_bytes = 32 * g.tile_rb;
    g.wave_bytes = g.x_bytes + g.dy_bytes + g.tile_bytes;
    return g;
}

template <typename T, int K, int NI>
__global__ __launch_bounds__(256) void conv1x1_bwd_kernel(const C1Launch L) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using P = Pw<T>;
    constexpr int VEC = P::VEC, ESZ = P::ESZ;
    int k = 0;
#pragma unroll
    for (int i = 1; i < C1_MAXP; ++i) if (i < L.n && (int)blockIdx.x >= L.p[i].blk0) k = i;
    const C1Prob& q = L.p[k];
    const int cb = blockIdx.y, c_lo = cb * 64;
    if (c_lo >= q.Cin) return;
    const int c_n = q.Cin - c_lo < 64 ? q.Cin - c_lo : 64;         // x / dx channels of this block
    const C1Geom g = c1_geom<T>(q.Cout);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r31 = lane & 31, h = lane >> 5;
    unsigned char* wdimg = smem;                                    // [64 cin rows of the block][Cout32], zero beyond Cin / Cout
    unsigned char* ximg = smem + g.wave_off + wv * g.wave_bytes;
    unsigned char* dyimg = ximg + g.x_bytes;
    unsigned char* tile = dyimg + g.dy_bytes;
    {
        const int nvr = g.Cout32 / VEC;
        const T* wd = reinterpret_cast<const T*>(q.wd);
        for (int i = threadIdx.x; i < 64 * nvr; i += blockDim.x) {
            const int row = i / nvr, v = i - row * nvr, c = v * VEC;
            uint4 val = make_uint4(0, 0, 0, 0);
            if (c_lo + row < q.Cin && c < q.Cout) val = *reinterpret_cast<const uint4*>(wd + (long long)(c_lo + row) * q.Cout + c);
            *reinterpret_cast<uint4*>(wdimg + row * g.WDRB + c * ESZ) = val;
        }
    }
    image_zero<T>(ximg, 2, lane);
    image_zero<T>(dyimg, g.Cout32 / 32, lane);
    __syncthreads();
    const T* __restrict__ xg = reinterpret_cast<const T*>(q.x);
    const T* __restrict__ dyg = reinterpret_cast<const T*>(q.dy);
    T* __restrict__ dxg = reinterpret_cast<T*>(q.dx);
    const int nwaves = q.nparts, nkc = g.Cout32 / 16;
    int t = ((int)blockIdx.x - q.blk0) * L.nw + wv;
    StageMap<K> smx, smd;
    stage_map<T, K>(smx, q.ldx, c_lo, 64, q.Cin, lane);
    stage_map<T, K>(smd, q.lddy, 0, q.Cout, q.Cout, lane);
    const int nvi = c_n / VEC, nvip = pow2_ge(nvi), slotsi = 64 / nvip, cvi = lane % nvip, sloti = lane / nvip;
    const int ni = g.Cout32 / 32;                                   // cout blocks in use (<= NI)
    const bool two_b = c_n > 32;
    f32x16_t am[NI][2];
#pragma unroll
    for (int a = 0; a < NI; ++a)
#pragma unroll
        for (int i = 0; i < 16; ++i) { am[a][0][i] = 0.f; am[a][1][i] = 0.f; }
    uint4 rx[K], rd[K];
    if (t < q.ntiles) {
        tile_load<T, K>(rx, xg, q.ldx, (long long)t * 32, q.npix, smx);
        tile_load<T, K>(rd, dyg, q.lddy, (long long)t * 32, q.npix, smd);
    }
    for (; t < q.ntiles; t += nwaves) {
        wave_fence();
        tile_store<T, K>(rx, ximg, smx);
        tile_store<T, K>(rd, dyimg, smd);
        const int tn = t + nwaves;
        if (tn < q.ntiles) {
            tile_load<T, K>(rx, xg, q.ldx, (long long)tn * 32, q.npix, smx);
            tile_load<T, K>(rd, dyg, q.lddy, (long long)tn * 32, q.npix, smd);
        }
        wave_fence();
        if (dxg != nullptr) {
            // dx[cin][pixel] = sum_cout wd[cin][cout] dy[cout][pixel]
            typename P::Frag db[K];
#pragma unroll
            for (int ks = 0; ks < K; ++ks) if (ks < nkc) db[ks] = P::row_frag(dyimg, r31, ks * 16 + 8 * h);
#pragma unroll
            for (int cit = 0; cit < 2; ++cit) {
                if (cit == 1 && !two_b) break;
                f32x16_t acc;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0.f;
                const unsigned char* wrow = wdimg + (cit * 32 + r31) * g.WDRB;
                typename P::Frag a[K];
#pragma unroll
                for (int ks = 0; ks < K; ++ks) if (ks < nkc) a[ks] = P::lin_frag(wrow, ks * 16 + 8 * h);
#pragma unroll
                for (int ks = 0; ks < K; ++ks) if (ks < nkc) acc = P::mma(a[ks], db[ks], acc);
#pragma unroll
                for (int gq = 0; gq < 4; ++gq)
                    P::put4(tile + r31 * g.tile_rb + (cit * 32 + gq * 8 + 4 * h) * ESZ, acc[gq * 4 + 0], acc[gq * 4 + 1], acc[gq * 4 + 2], acc[gq * 4 + 3]);
            }
            wave_fence();
            if (cvi < nvi) {
                const int left = (int)(q.npix - (long long)t * 32 < 32 ? q.npix - (long long)t * 32 : 32);
                T* ob = dxg + (long long)t * 32 * q.lddx + c_lo + cvi * VEC;
#pragma unroll
                for (int it = 0; it < K; ++it) {
                    const int px = sloti + it * slotsi;
                    if (px < left) *reinterpret_cast<uint4*>(ob + (long long)px * q.lddx) = *reinterpret_cast<const uint4*>(tile + px * g.tile_rb + cvi * VEC * ESZ);
                }
            }
        }
        // dW[cout][cin] += dy^T x over the 32 pixels (K = pixels, both operands transposing reads)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const typename P::Frag b0 = P::col_frag(ximg, ks * 16, lane);
            typename P::Frag b1 = b0;
            if (two_b) b1 = P::col_frag(ximg + P::BLK, ks * 16, lane);
#pragma unroll
            for (int a = 0; a < NI; ++a) {
                if (a < ni) {
                    const typename P::Frag fa = P::col_frag(dyimg + a * P::BLK, ks * 16, lane);
                    am[a][0] = P::mma(fa, b0, am[a][0]);
                    if (two_b) am[a][1] = P::mma(fa, b1, am[a][1]);
                }
            }
        }
    }
    // ---- one slab per workgroup: the waves' accumulators are added through LDS in wave order (fixed order), then stored
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);                   // [NI * 32][64]
    for (int r = 0; r < L.nw; ++r) {
        if (wv == r) {
#pragma unroll
            for (int a = 0; a < NI; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int idx = (a * 32 + (i & 3) + 8 * (i >> 2) + 4 * h) * 64 + b * 32 + r31;
                        red[idx] = (r == 0 ? 0.f : red[idx]) + am[a][b][i];
                    }
        }
        __syncthreads();
    }
    float* out = q.slab + (long long)((int)blockIdx.x - q.blk0) * q.Cout * q.Cin;
    for (int i = threadIdx.x; i < q.Cout * 64; i += blockDim.x) {
        const int row = i >> 6, col = i & 63;
        if (col < c_n) out[(long long)row * q.Cin + c_lo + col] = red[row * 64 + col];
    }
}

// ================================================================= host side
struct Plan { int nw, smem; };
int waves_for(long long ntiles, int cap) {
    long long w = (ntiles + 3) / 4;              // >= 4 tiles per wave where there are that many
    if (w > cap) w = cap;
    if (w < 1) w = 1;
    return (int)w;
}

// vectors per lane of a tile of `nc` channels
template <typename T> int cv_of(int nc) { return (32 * (nc / Pw<T>::VEC) + 63) / 64; }
// iterations of the element-wise side for nc channels: lanes = (64 / nvp pixel slots) x nvp vectors
template <typename T> int np_of(int nc) { int nv = nc / Pw<T>::VEC, nvp = 1; while (nvp < nv) nvp <<= 1; return nvp >= 2 ? nvp / 2 : 1; }

// one slab per workgroup, a function of the pixel count alone (the slab buffer is sized by egm_conv1x1_bwd_slabs)
constexpr int C1_WAVES = 1024;
int c1_wgs(long long npix) { return (waves_for((npix + 31) / 32, C1_WAVES) + 3) / 4; }
template <typename T> Plan c1_plan(int Cout) {
    const C1Geom g = c1_geom<T>(Cout);
    Plan p;
    const int red = r32(Cout) * 64 * 4;
    for (p.nw = 4; p.nw >= 1; p.nw >>= 1) {
        p.smem = g.wave_off + p.nw * g.wave_bytes;
        if (p.smem < red) p.smem = red;
        if (p.smem <= C1_LDS_BUDGET) return p;
    }
    p.nw = 0; p.smem = 0;
    return p;
}
template <typename T>
int conv1x1_bwd_t(const egm_conv1x1_bwd_desc* d, int n, egm_stream_t s) {
    C1Launch L; L.n = n; L.nw = 4;
    int smem = 0, kk = 1, ni = 1, gy = 1, blk = 0;
    for (int i = 0; i < n; ++i) {
        const Plan p = c1_plan<T>(d[i].Cout);
        EGM_REQUIRE(p.nw > 0, "conv1x1_bwd: shape does not fit the LDS");
        if (p.nw < L.nw) L.nw = p.nw;
    }
    for (int i = 0; i < n; ++i) {
        C1Prob& q = L.p[i];
        q.x = d[i].x; q.dy = d[i].dy; q.wd = d[i].wd; q.dx = d[i].dx; q.slab = d[i].slabs; q.npix = d[i].npix; q.ldx = d[i].ldx; q.lddy = d[i].lddy;
        q.lddx = d[i].lddx; q.Cin = d[i].Cin; q.Cout = d[i].Cout; q.ntiles = (int)((d[i].npix + 31) / 32);
        const int wgs = c1_wgs(d[i].npix);
        q.nparts = wgs * L.nw; q.blk0 = blk; blk += wgs;
        const C1Geom g = c1_geom<T>(q.Cout);
        int sm = g.wave_off + L.nw * g.wave_bytes;
        if (sm < r32(q.Cout) * 64 * 4) sm = r32(q.Cout) * 64 * 4;
        smem = std::max(smem, sm);
        kk = std::max(kk, std::max(cv_of<T>(64), std::max(cv_of<T>(q.Cout), np_of<T>(64))));
        ni = std::max(ni, r32(q.Cout) / 32);
        gy = std::max(gy, (q.Cin + 63) / 64);
    }
#define C1_LAUNCH(KV, NIV) do { if (int rc = egm_allow_max_lds<conv1x1_bwd_kernel<T, KV, NIV>>("conv1x1_bwd")) return rc; \
        hipLaunchKernelGGL((conv1x1_bwd_kernel<T, KV, NIV>), dim3(blk, gy), dim3(64 * L.nw), smem, (hipStream_t)s, L); } while (0)
    if (ni <= 2) { if (kk <= 4) C1_LAUNCH(4, 2); else if (kk <= 8) C1_LAUNCH(8, 2); else C1_LAUNCH(16, 2); }
    else { if (kk <= 8) C1_LAUNCH(8, 4); else C1_LAUNCH(16, 4); }
#undef C1_LAUNCH
    EGM_CHECK_LAUNCH("conv1x1_bwd");
    return EGM_OK;
}
}  // namespace

extern "C" int egm_conv1x1_bwd_supported(int dtype, int Cin, int Cout) {
    if (!(Cin > 0 && Cin % 8 == 0 && Cin <= C1_MAXC && Cout > 0 && Cout % 8 == 0 && Cout <= C1_MAXC)) return 0;
    if (dtype == EGM_BF16) return c1_plan<bf16_t>(Cout).nw > 0 ? 1 : 0;
    if (dtype == EGM_F32) return c1_plan<float>(Cout).nw > 0 ? 1 : 0;
    return 0;
}
extern "C" int egm_conv1x1_bwd_slabs(long long npix) { return npix > 0 ? c1_wgs(npix) : -1; }
extern "C" int egm_conv1x1_bwd(int dtype, const egm_conv1x1_bwd_desc* descs, int n, egm_stream_t s) {
    EGM_REQUIRE(descs && n > 0 && n <= C1_MAXP, "conv1x1_bwd: 1..%d convolutions per call", C1_MAXP);
    for (int i = 0; i < n; ++i) {
        const egm_conv1x1_bwd_desc& e = descs[i];
        EGM_REQUIRE(egm_conv1x1_bwd_supported(dtype, e.Cin, e.Cout), "conv1x1_bwd: unsupported channels %d -> %d (entry %d)", e.Cin, e.Cout, i);
        EGM_REQUIRE(e.x && e.dy && e.wd && e.slabs && egm_aligned16(e.x) && egm_aligned16(e.dy) && egm_aligned16(e.wd) && e.npix > 0 && e.ldx >= e.Cin &&
                    e.ldx % 8 == 0 && e.lddy >= e.Cout && e.lddy % 8 == 0 && (e.dx == nullptr || (egm_aligned16(e.dx) && e.lddx >= e.Cin && e.lddx % 8 == 0)),
                    "conv1x1_bwd: bad entry %d", i);
    }
    return dtype == EGM_BF16 ? conv1x1_bwd_t<bf16_t>(descs, n, s) : conv1x1_bwd_t<float>(descs, n, s);
}
