// CLIPSeg baseline decoder head, CLIPDenseBaseline (models/clipseg.py:529-590), per token t of the layer-9 activation x [B][Ltot][768]
// (tok_off leading rows, the class token, skipped):
//   u  = x_t W_red^T + b_red                  768 -> rd
//   f  = mul[b] * u + add[b]                  FiLM (mul / add = film_mul(cond), film_add(cond): [B][rd], precomputed)
//   h  = relu(f W1^T + b1)                    rd -> rd2   (reduce2[0], reduce2[1])
//   a3 = h W2^T + b2                          rd2 -> rd   (reduce2[2])
//   y  = a3 Wt + bt                           ConvTranspose2d(rd -> 1, 16, stride 16): token (ty, tx) owns the 16 x 16 patch at (16 ty, 16 tx)
// No product reads another token, so the head is a chain of four GEMMs over a tile of tokens.
//
// Layout.  A wave owns a tile of 16 tokens of ONE image (consecutive in raster order, so neighbours in a grid row are neighbours in the
// wave); a workgroup is 4 such waves.  Every product runs on v_mfma_f32_16x16x32_bf16 with the tokens as the 16 columns (lane & 15) and
// the features as rows, so a product's fp32 accumulator tile is the B operand of the next product without any lane movement (two
// 16-row tiles = one 32-deep k-step; the k order inside a step is permuted, and the weight images of egm_baseline_pack follow it).
//   * reduce: x is read straight from memory into B fragments (each lane 2 x 16 B of its token's row per 64-feature chunk: four lanes
//     cover 128 contiguous bytes); W_red streams through LDS in 64-feature chunks shared by the workgroup's 4 waves.
//   * W1, W2 and Wt stay resident in LDS.
//   * The epilogue adds bt and writes fp32 NCHW directly: a lane holds all 16 pixels of one patch row (4 x 16-byte stores, 64 B).
// rd and rd2 are padded to NP = the next multiple of 32 of max(rd, rd2) with zero weights; pad rows stay 0 through the chain.
//
// Rounding (bf16 path): products accumulate in fp32.  u is rounded to bf16 (it is what the training form saves, so the backward
// recomputes exactly the forward's f); f, h and a3 are rounded to bf16 where they become MFMA operands (h is also what is saved);
// y leaves in fp32.  Backward: dy, da3, dh are rounded to bf16 as operands, df stays fp32, du = bf16(df * mul).
//
// Backward: two launches, no atomics, bitwise reproducible.
//   1. per workgroup (64 tokens): dy from dout (pixel unshuffle inside the load), da3 = dy Wt^T, recompute f (from u) and a3 (from h),
//      dh = (da3 W2) * [h > 0], df = dh W1, du = df * mul -> bf16.  Per wave tile: dmul, dadd partial rows.  Per workgroup: fp32 slabs of
//      dWt, dW2, dW1 (MFMA over the 64 tokens, operands transposed through LDS), db2, db1, dbt.
//   2. slab sums in fixed order (4 interleaved partial sums per output, combined as a tree).
// reduce's own weight gradient (768 x rd over all tokens) is left to the caller (du is the gradient of u).
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

constexpr int NT = 256;          // threads per workgroup = 4 waves
constexpr int TT = 16;           // tokens per wave tile
constexpr int WT = NT / 64;      // wave tiles per workgroup
constexpr int DX = 768;          // activation width (ViT-B)
constexpr int PP = 256;          // pixels per token (patch 16)
constexpr int TS = WT * TT + 8;  // row stride (elements) of the transposed [feature][token] LDS images of the backward

__host__ __device__ constexpr int np_for(int rd, int rd2) { return ((rd > rd2 ? rd : rd2) + 31) / 32 * 32; }

// packed operand image (bf16 elements); every region is [tile][k-step][lane 64][8]
__host__ __device__ constexpr long long off_wr(int) { return 0; }                                             // W_red   768 NP
__host__ __device__ constexpr long long off_w1f(int np) { return 768LL * np; }                              // W1  fwd NP^2
__host__ __device__ constexpr long long off_w2f(int np) { return 768LL * np + 1LL * np * np; }              // W2  fwd NP^2
__host__ __device__ constexpr long long off_wtf(int np) { return 768LL * np + 2LL * np * np; }              // Wt  fwd 256 NP
__host__ __device__ constexpr long long off_wtb(int np) { return 1024LL * np + 2LL * np * np; }             // Wt  bwd 256 NP
__host__ __device__ constexpr long long off_w2b(int np) { return 1280LL * np + 2LL * np * np; }             // W2  bwd NP^2
__host__ __device__ constexpr long long off_w1b(int np) { return 1280LL * np + 3LL * np * np; }             // W1  bwd NP^2
__host__ __device__ constexpr long long packed_elems(int np) { return 1280LL * np + 4LL * np * np; }

// k-slot j of lane group q in a 32-deep k-step over an accumulator-derived operand -> row inside the step (two 16-row tiles)
__host__ __device__ constexpr int kperm(int q, int j) { return j < 4 ? 4 * q + j : 16 + 4 * q + (j - 4); }

// weight-gradient slab of one backward workgroup (floats)
__host__ __device__ constexpr long long sl_w2(int np) { return 256LL * np; }
__host__ __device__ constexpr long long sl_w1(int np) { return 256LL * np + 1LL * np * np; }
__host__ __device__ constexpr long long sl_b2(int np) { return 256LL * np + 2LL * np * np; }
__host__ __device__ constexpr long long sl_b1(int np) { return 256LL * np + 2LL * np * np + np; }
__host__ __device__ constexpr long long sl_bt(int np) { return 256LL * np + 2LL * np * np + 2 * np; }
__host__ __device__ constexpr long long slab_elems(int np) { return (256LL * np + 2LL * np * np + 2 * np + 1 + 3) / 4 * 4; }

struct Tiles { long long ntpi, nwt, nwg; };
static inline Tiles tiles_for(int B, int g) {
    Tiles t;
    t.ntpi = ((long long)g * g + TT - 1) / TT;
    t.nwt = (long long)B * t.ntpi;
    t.nwg = (t.nwt + WT - 1) / WT;
    return t;
}

__device__ __forceinline__ float rnd(float x) { return bf16_to_f32(f32_to_bf16(x)); }
__device__ __forceinline__ bf16x8_t pack2(const f32x4_t& a, const f32x4_t& b) {
    bf16x8_t r;
    r[0] = (__bf16)a[0]; r[1] = (__bf16)a[1]; r[2] = (__bf16)a[2]; r[3] = (__bf16)a[3];
    r[4] = (__bf16)b[0]; r[5] = (__bf16)b[1]; r[6] = (__bf16)b[2]; r[7] = (__bf16)b[3];
    return r;
}
__device__ __forceinline__ bf16x8_t frag(const bf16_t* p) { return *reinterpret_cast<const bf16x8_t*>(p); }
__device__ __forceinline__ bf16x8_t zero8() { bf16x8_t r; for (int j = 0; j < 8; ++j) r[j] = (__bf16)0.f; return r; }
__device__ __forceinline__ f32x4_t mfma(const bf16x8_t& a, const bf16x8_t& b, const f32x4_t& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// 4 consecutive bf16 (8 bytes) <-> floats
__device__ __forceinline__ f32x4_t load4(const bf16_t* p) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    return (f32x4_t){bf16_to_f32(v.x & 0xffff), bf16_to_f32(v.x >> 16), bf16_to_f32(v.y & 0xffff), bf16_to_f32(v.y >> 16)};
}
__device__ __forceinline__ void store4(bf16_t* p, const f32x4_t& v) {
    uint2 o;
    o.x = (uint32_t)f32_to_bf16(v[0]) | ((uint32_t)f32_to_bf16(v[1]) << 16);
    o.y = (uint32_t)f32_to_bf16(v[2]) | ((uint32_t)f32_to_bf16(v[3]) << 16);
    *reinterpret_cast<uint2*>(p) = o;
}
// sum over the 16 token lanes of a lane group (fixed butterfly order)
__device__ __forceinline__ float sum16(float v) {
    v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
    return v;
}
// copy n16 16-byte units global -> LDS with the whole workgroup
__device__ __forceinline__ void stage(bf16_t* dst, const bf16_t* src, int n16) {
    for (int i = threadIdx.x; i < n16; i += NT) reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
}

// What both forward kernels start with: the wave's token tile (image b, token t of lane column col, tv: the token exists), W1 / W2 / Wt
// staged into s_res, and acc = x W_red^T, the 768-deep product, with W_red streaming through s_wr in 64-feature chunks.
template <int NP>
__device__ __forceinline__ void reduce_product(const bf16_t* __restrict__ x, int tok_off, int Ltot, const bf16_t* __restrict__ pk, int g,
                                               long long nwt, long long ntpi, bf16_t* s_wr, bf16_t* s_res, int& b, int& t, bool& tv,
                                               f32x4_t (&acc)[NP / 16]) {
    constexpr int MT = NP / 16;
    const int tid = threadIdx.x, lane = tid & 63, q = lane >> 4, col = lane & 15;
    const long long wt = (long long)blockIdx.x * WT + (tid >> 6);
    const bool has = wt < nwt;
    b = has ? (int)(wt / ntpi) : 0;
    t = has ? (int)(wt % ntpi) * TT + col : 0;
    tv = has && t < g * g;
    // the token's 768 activations as B fragments: chunk c, step s -> features 64c + 16q + 8s .. +7
    bf16x8_t xf[24];
    {
        const bf16_t* xr = x + ((long long)b * Ltot + tok_off + (tv ? t : 0)) * DX + 16 * q;
#pragma unroll
        for (int c = 0; c < 12; ++c)
#pragma unroll
            for (int s = 0; s < 2; ++s) xf[2 * c + s] = tv ? frag(xr + 64 * c + 8 * s) : zero8();
    }
    stage(s_res, pk + off_w1f(NP), (2 * NP * NP + PP * NP) / 8);
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < 12; ++c) {
        stage(s_wr, pk + off_wr(NP) + 64LL * NP * c, 64 * NP / 8);
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m] = mfma(frag(s_wr + ((m * 2 + s) * 64 + lane) * 8), xf[2 * c + s], acc[m]);
        __syncthreads();
    }
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
template <int NP>
__global__ __launch_bounds__(NT) void baseline_fwd_kernel(const bf16_t* __restrict__ x, int tok_off, int Ltot, const bf16_t* __restrict__ mul,
                                                          const bf16_t* __restrict__ add, const bf16_t* __restrict__ pk,
                                                          const float* __restrict__ b_red, const float* __restrict__ b1,
                                                          const float* __restrict__ b2, const float* __restrict__ bt,
                                                          bf16_t* __restrict__ u_out, bf16_t* __restrict__ h_out, float* __restrict__ out,
                                                          int g, int rd, int rd2, long long nwt, long long ntpi) {
    constexpr int MT = NP / 16, KS = NP / 32;
    __shared__ __align__(16) bf16_t s_wr[64 * NP];                   // one 64-feature chunk of W_red
    __shared__ __align__(16) bf16_t s_res[2 * NP * NP + PP * NP];    // W1 fwd | W2 fwd | Wt fwd
    const int lane = threadIdx.x & 63, q = lane >> 4;
    int b, t;
    bool tv;
    f32x4_t acc[MT];
    reduce_product<NP>(x, tok_off, Ltot, pk, g, nwt, ntpi, s_wr, s_res, b, t, tv, acc);
    // u (rounded, saved) -> f
    const long long trow = (long long)b * g * g + t;
    bf16x8_t fb[KS];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int r0 = 16 * m + 4 * q;
        f32x4_t u, f;
        for (int r = 0; r < 4; ++r) {
            const bool ok = r0 + r < rd;
            u[r] = ok ? rnd(acc[m][r] + b_red[r0 + r]) : 0.f;
            f[r] = ok ? fmaf(to_f32(mul[(long long)b * rd + r0 + r]), u[r], to_f32(add[(long long)b * rd + r0 + r])) : 0.f;
        }
        if (u_out && tv && r0 < rd) store4(u_out + trow * rd + r0, u);
        acc[m] = f;
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) fb[s] = pack2(acc[2 * s], acc[2 * s + 1]);
    // h = relu(W1 f + b1)
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int r0 = 16 * m + 4 * q;
        for (int r = 0; r < 4; ++r) acc[m][r] = r0 + r < rd2 ? b1[r0 + r] : 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s) acc[m] = mfma(frag(s_res + ((m * KS + s) * 64 + lane) * 8), fb[s], acc[m]);
        for (int r = 0; r < 4; ++r) acc[m][r] = rnd(fmaxf(acc[m][r], 0.f));
        if (h_out && tv && r0 < rd2) store4(h_out + trow * rd2 + r0, acc[m]);
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) fb[s] = pack2(acc[2 * s], acc[2 * s + 1]);
    // a3 = W2 h + b2
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int r0 = 16 * m + 4 * q;
        for (int r = 0; r < 4; ++r) acc[m][r] = r0 + r < rd ? b2[r0 + r] : 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s) acc[m] = mfma(frag(s_res + NP * NP + ((m * KS + s) * 64 + lane) * 8), fb[s], acc[m]);
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) fb[s] = pack2(acc[2 * s], acc[2 * s + 1]);
    // y = Wt^T a3 + bt: tile i = 4a + cc holds pixel row 4a + q, columns 4cc .. 4cc + 3 of the lane's token
    const float bias = bt[0];
    const int G16 = 16 * g, ty = t / g, tx = t % g;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        f32x4_t y[4];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            y[cc] = (f32x4_t){bias, bias, bias, bias};
#pragma unroll
            for (int s = 0; s < KS; ++s) y[cc] = mfma(frag(s_res + 2 * NP * NP + (((4 * a + cc) * KS + s) * 64 + lane) * 8), fb[s], y[cc]);
        }
        if (tv) {
            float* o = out + ((long long)b * G16 + 16 * ty + 4 * a + q) * G16 + 16 * tx;
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) *reinterpret_cast<f32x4_t*>(o + 4 * cc) = y[cc];
        }
    }
}

// ---- forward, K prompts on the same activation (CLIPDenseBase.forward_multi) ------------------------------------------------------
// u = x W_red^T + b_red (the 768-deep product, the head's largest) is computed ONCE per token tile and kept in registers; the prompts
// k0 .. k1 - 1 of this workgroup's group (blockIdx.y) then each run FiLM -> W1 -> ReLU -> W2 -> Wt from the LDS-resident weights and
// store out[b*K + k].  Per prompt the instruction sequence and rounding points are those of baseline_fwd_kernel with mul[k] / add[k], so
// every prompt's mask equals egm_baseline_fwd's bit for bit.  The prompt groups exist for small B: a grid of token tiles alone is ~8
// workgroups at B = 1, so u is recomputed per group to fill the GPU.
template <int NP>
__global__ __launch_bounds__(NT) void baseline_fwd_multi_kernel(const bf16_t* __restrict__ x, int tok_off, int Ltot, const bf16_t* __restrict__ mul,
                                                                const bf16_t* __restrict__ add, const bf16_t* __restrict__ pk,
                                                                const float* __restrict__ b_red, const float* __restrict__ b1,
                                                                const float* __restrict__ b2, const float* __restrict__ bt, float* __restrict__ out,
                                                                int g, int rd, int rd2, long long nwt, long long ntpi, int K, int kpg) {
    constexpr int MT = NP / 16, KS = NP / 32;
    __shared__ __align__(16) bf16_t s_wr[64 * NP];                   // one 64-feature chunk of W_red
    __shared__ __align__(16) bf16_t s_res[2 * NP * NP + PP * NP];    // W1 fwd | W2 fwd | Wt fwd
    const int lane = threadIdx.x & 63, q = lane >> 4;
    int b, t;
    bool tv;
    f32x4_t acc[MT];
    reduce_product<NP>(x, tok_off, Ltot, pk, g, nwt, ntpi, s_wr, s_res, b, t, tv, acc);
    f32x4_t u[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int r0 = 16 * m + 4 * q;
        for (int r = 0; r < 4; ++r) u[m][r] = r0 + r < rd ? rnd(acc[m][r] + b_red[r0 + r]) : 0.f;
    }
    const float bias = bt[0];
    const int G16 = 16 * g, ty = t / g, tx = t % g;
    const int k0 = blockIdx.y * kpg, k1 = k0 + kpg < K ? k0 + kpg : K;
    for (int k = k0; k < k1; ++k) {
        // compiler-only fence: keeps the LDS weight fragments from being hoisted out of the prompt loop (they would not fit in registers)
        asm volatile("" ::: "memory");
        const bf16_t* mk = mul + (long long)k * rd;
        const bf16_t* ak = add + (long long)k * rd;
        bf16x8_t fb[KS];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int r0 = 16 * m + 4 * q;
            for (int r = 0; r < 4; ++r) acc[m][r] = r0 + r < rd ? fmaf(to_f32(mk[r0 + r]), u[m][r], to_f32(ak[r0 + r])) : 0.f;
        }
#pragma unroll
        for (int s = 0; s < KS; ++s) fb[s] = pack2(acc[2 * s], acc[2 * s + 1]);
        // h = relu(W1 f + b1)
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int r0 = 16 * m + 4 * q;
            for (int r = 0; r < 4; ++r) acc[m][r] = r0 + r < rd2 ? b1[r0 + r] : 0.f;
#pragma unroll
            for (int s = 0; s < KS; ++s) acc[m] = mfma(frag(s_res + ((m * KS + s) * 64 + lane) * 8), fb[s], acc[m]);
            for (int r = 0; r < 4; ++r) acc[m][r] = rnd(fmaxf(acc[m][r], 0.f));
        }
#pragma unroll
        for (int s = 0; s < KS; ++s) fb[s] = pack2(acc[2 * s], acc[2 * s + 1]);
        // a3 = W2 h + b2
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int r0 = 16 * m + 4 * q;
            for (int r = 0; r < 4; ++r) acc[m][r] = r0 + r < rd ? b2[r0 + r] : 0.f;
#pragma unroll
            for (int s = 0; s < KS; ++s) acc[m] = mfma(frag(s_res + NP * NP + ((m * KS + s) * 64 + lane) * 8), fb[s], acc[m]);
        }
#pragma unroll
        for (int s = 0; s < KS; ++s) fb[s] = pack2(acc[2 * s], acc[2 * s + 1]);
        // y = Wt^T a3 + bt -> out[b*K + k]
        float* ok = out + ((long long)b * K + k) * G16 * G16;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            f32x4_t y[4];
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                y[cc] = (f32x4_t){bias, bias, bias, bias};
#pragma unroll
                for (int s = 0; s < KS; ++s) y[cc] = mfma(frag(s_res + 2 * NP * NP + (((4 * a + cc) * KS + s) * 64 + lane) * 8), fb[s], y[cc]);
            }
            if (tv) {
                float* o = ok + (16LL * ty + 4 * a + q) * G16 + 16 * tx;
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) *reinterpret_cast<f32x4_t*>(o + 4 * cc) = y[cc];
            }
        }
    }
}

// ---- backward 1: per-token data gradients + per-workgroup slabs ---------------------------------------------------------------
template <int NP>
__global__ __launch_bounds__(NT) void baseline_bwd_kernel(const float* __restrict__ dout, const bf16_t* __restrict__ u_in,
                                                          const bf16_t* __restrict__ h_in, const bf16_t* __restrict__ mul,
                                                          const bf16_t* __restrict__ add, const bf16_t* __restrict__ pk,
                                                          const float* __restrict__ b2, bf16_t* __restrict__ du, int tok_off, int Ltot,
                                                          float* __restrict__ slabs, float* __restrict__ film, int g, int rd, int rd2,
                                                          long long nwt, long long ntpi) {
    constexpr int MT = NP / 16, KS = NP / 32;
    // transposed [feature][token slot] images of this workgroup's 64 tokens (bf16): dy, a3, da3, h, dh, f
    __shared__ __align__(16) bf16_t s_tr[(PP + 5 * NP) * TS];
    __shared__ float s_red[WT][2 * NP + 1];
    bf16_t* tr_dy = s_tr;
    bf16_t* tr_a3 = s_tr + PP * TS;
    bf16_t* tr_da3 = tr_a3 + NP * TS;
    bf16_t* tr_h = tr_da3 + NP * TS;
    bf16_t* tr_dh = tr_h + NP * TS;
    bf16_t* tr_f = tr_dh + NP * TS;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, col = lane & 15, slot = wave * TT + col;
    const long long wt = (long long)blockIdx.x * WT + wave;
    const bool has = wt < nwt;
    const int b = has ? (int)(wt / ntpi) : 0;
    const int t = has ? (int)(wt % ntpi) * TT + col : 0;
    const bool tv = has && t < g * g;
    const long long trow = (long long)b * g * g + t;
    auto put = [&](bf16_t* img, int row, float v) { img[row * TS + slot] = from_f32<bf16_t>(v); };

    // dy: step s, lane group q -> pixels 32s + 8q .. +7 = patch row 2s + (q >> 1), columns 8 (q & 1) .. +7
    bf16x8_t dyf[8];
    float sdy = 0.f;
    {
        const int G16 = 16 * g, ty = t / g, tx = t % g;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            f32x4_t v0 = (f32x4_t){0.f, 0.f, 0.f, 0.f}, v1 = v0;
            if (tv) {
                const float* p = dout + ((long long)b * G16 + 16 * ty + 2 * s + (q >> 1)) * G16 + 16 * tx + 8 * (q & 1);
                v0 = *reinterpret_cast<const f32x4_t*>(p);
                v1 = *reinterpret_cast<const f32x4_t*>(p + 4);
            }
            sdy += ((v0[0] + v0[1]) + (v0[2] + v0[3])) + ((v1[0] + v1[1]) + (v1[2] + v1[3]));
            dyf[s] = pack2(v0, v1);
#pragma unroll
            for (int j = 0; j < 8; ++j) tr_dy[(32 * s + 8 * q + j) * TS + slot] = from_f32<bf16_t>((float)dyf[s][j]);
        }
    }
    // da3 = Wt dy  (rows c)
    f32x4_t da3[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        da3[m] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 8; ++s) da3[m] = mfma(frag(pk + off_wtb(NP) + ((m * 8 + s) * 64 + lane) * 8), dyf[s], da3[m]);
    }
    // recompute f (from u) and a3 (from h); keep u and h in fp32
    f32x4_t u[MT], h[MT], tmp[MT];
    bf16x8_t fb[KS], hb[KS], ab[KS];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int r0 = 16 * m + 4 * q;
        u[m] = (tv && r0 < rd) ? load4(u_in + trow * rd + r0) : (f32x4_t){0.f, 0.f, 0.f, 0.f};
        h[m] = (tv && r0 < rd2) ? load4(h_in + trow * rd2 + r0) : (f32x4_t){0.f, 0.f, 0.f, 0.f};
        for (int r = 0; r < 4; ++r)
            tmp[m][r] = r0 + r < rd ? fmaf(to_f32(mul[(long long)b * rd + r0 + r]), u[m][r], to_f32(add[(long long)b * rd + r0 + r])) : 0.f;
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) { fb[s] = pack2(tmp[2 * s], tmp[2 * s + 1]); hb[s] = pack2(h[2 * s], h[2 * s + 1]); }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int r0 = 16 * m + 4 * q;
        for (int r = 0; r < 4; ++r) tmp[m][r] = r0 + r < rd ? b2[r0 + r] : 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s) tmp[m] = mfma(frag(pk + off_w2f(NP) + ((m * KS + s) * 64 + lane) * 8), hb[s], tmp[m]);
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) ab[s] = pack2(tmp[2 * s], tmp[2 * s + 1]);
    // transposed operand images for the weight gradients: a3, h, f (as rounded operands) and da3
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int row = 32 * s + kperm(q, j);
            put(tr_a3, row, (float)ab[s][j]);
            put(tr_h, row, (float)hb[s][j]);
            put(tr_f, row, (float)fb[s][j]);
        }
    // dh = (W2^T da3) * [h > 0]
    bf16x8_t db[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) db[s] = pack2(da3[2 * s], da3[2 * s + 1]);
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) put(tr_da3, 32 * s + kperm(q, j), (float)db[s][j]);
    float* red = s_red[wave];
#pragma unroll
    for (int m = 0; m < MT; ++m)
        for (int r = 0; r < 4; ++r) {
            const float v = sum16(da3[m][r]);
            if (col == 0) red[16 * m + 4 * q + r] = v;                                          // db2 of this wave
        }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        tmp[m] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) tmp[m] = mfma(frag(pk + off_w2b(NP) + ((m * KS + s) * 64 + lane) * 8), db[s], tmp[m]);
        for (int r = 0; r < 4; ++r) {
            tmp[m][r] = h[m][r] > 0.f ? tmp[m][r] : 0.f;
            const float v = sum16(tmp[m][r]);
            if (col == 0) red[NP + 16 * m + 4 * q + r] = v;                                     // db1 of this wave
        }
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) db[s] = pack2(tmp[2 * s], tmp[2 * s + 1]);
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) put(tr_dh, 32 * s + kperm(q, j), (float)db[s][j]);
    // df = W1^T dh;  du = df * mul;  dmul, dadd partial rows of this wave tile
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int r0 = 16 * m + 4 * q;
        f32x4_t df = (f32x4_t){0.f, 0.f, 0.f, 0.f}, o;
#pragma unroll
        for (int s = 0; s < KS; ++s) df = mfma(frag(pk + off_w1b(NP) + ((m * KS + s) * 64 + lane) * 8), db[s], df);
        for (int r = 0; r < 4; ++r) {
            o[r] = r0 + r < rd ? df[r] * to_f32(mul[(long long)b * rd + r0 + r]) : 0.f;
            const float dm = sum16(df[r] * u[m][r]), da = sum16(df[r]);
            if (has && col == 0) {
                film[wt * 2 * NP + r0 + r] = dm;
                film[wt * 2 * NP + NP + r0 + r] = da;
            }
        }
        if (tv && r0 < rd) store4(du + ((long long)b * Ltot + tok_off + t) * rd + r0, o);
    }
    if (has && wt % ntpi == 0)                                     // the class-token rows of du: 0
        for (int i = lane; i < tok_off * rd; i += 64) du[(long long)b * Ltot * rd + i] = from_f32<bf16_t>(0.f);
    {
        float v = sdy;
        v += __shfl_xor(v, 32); v += __shfl_xor(v, 16); v = sum16(v);
        if (lane == 0) red[2 * NP] = v;                                                         // dbt of this wave
    }
    __syncthreads();
    float* slab = slabs + (long long)blockIdx.x * slab_elems(NP);
    for (int i = tid; i < 2 * NP + 1; i += NT) slab[sl_b2(NP) + i] = (s_red[0][i] + s_red[1][i]) + (s_red[2][i] + s_red[3][i]);
    // weight gradients over the workgroup's 64 tokens: dWt = a3^T dy, dW2 = da3^T h, dW1 = dh^T f  (16 x 16 output tiles)
    constexpr int T1 = MT * 16, T2 = MT * MT;
    for (int i = wave; i < T1 + 2 * T2; i += WT) {
        const bf16_t *A, *Bm;
        float* dst;
        int ld, mi, ni;
        if (i < T1) { A = tr_a3; Bm = tr_dy; mi = i / 16; ni = i % 16; dst = slab; ld = PP; }
        else if (i < T1 + T2) { A = tr_da3; Bm = tr_h; mi = (i - T1) / MT; ni = (i - T1) % MT; dst = slab + sl_w2(NP); ld = NP; }
        else { A = tr_dh; Bm = tr_f; mi = (i - T1 - T2) / MT; ni = (i - T1 - T2) % MT; dst = slab + sl_w1(NP); ld = NP; }
        f32x4_t c = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 2; ++s)
            c = mfma(frag(A + (16 * mi + col) * TS + 32 * s + 8 * q), frag(Bm + (16 * ni + col) * TS + 32 * s + 8 * q), c);
        for (int r = 0; r < 4; ++r) dst[(long long)(16 * mi + 4 * q + r) * ld + 16 * ni + col] = c[r];
    }
}

// ---- backward 2: slab sums in fixed order ----------------------------------------------------------------------------------
template <int NP>
__global__ __launch_bounds__(NT) void baseline_reduce_kernel(const float* __restrict__ slabs, long long nslab, const float* __restrict__ film,
                                                             long long ntpi, int B, int rd, int rd2, float* __restrict__ dwt,
                                                             float* __restrict__ dbt, float* __restrict__ dw2, float* __restrict__ db2,
                                                             float* __restrict__ dw1, float* __restrict__ db1, bf16_t* __restrict__ dmul,
                                                             bf16_t* __restrict__ dadd) {
    __shared__ float part[4][64];
    const int tid = threadIdx.x, p = tid >> 6;
    const long long nwts = (long long)rd * PP, nw2 = (long long)rd * rd2, nw1 = nw2;
    const long long o = (long long)blockIdx.x * 64 + (tid & 63);
    const long long e0 = nwts, e1 = e0 + 1, e2 = e1 + nw2, e3 = e2 + rd, e4 = e3 + nw1, e5 = e4 + rd2, e6 = e5 + 2LL * B * rd;
    const float* src = nullptr;
    long long n = 0, stride = 0;
    if (o < e0) { src = slabs + (o / PP) * PP + o % PP; n = nslab; stride = slab_elems(NP); }
    else if (o < e1) { src = slabs + sl_bt(NP); n = nslab; stride = slab_elems(NP); }
    else if (o < e2) { const long long k = o - e1; src = slabs + sl_w2(NP) + (k / rd2) * NP + k % rd2; n = nslab; stride = slab_elems(NP); }
    else if (o < e3) { src = slabs + sl_b2(NP) + (o - e2); n = nslab; stride = slab_elems(NP); }
    else if (o < e4) { const long long k = o - e3; src = slabs + sl_w1(NP) + (k / rd) * NP + k % rd; n = nslab; stride = slab_elems(NP); }
    else if (o < e5) { src = slabs + sl_b1(NP) + (o - e4); n = nslab; stride = slab_elems(NP); }
    else if (o < e6) {
        const long long k = o - e5, which = k / ((long long)B * rd), bb = (k / rd) % B, c = k % rd;
        src = film + bb * ntpi * 2 * NP + which * NP + c; n = ntpi; stride = 2 * NP;
    }
    float v = 0.f;
    if (src)
        for (long long w = p; w < n; w += 4) v += src[w * stride];
    part[p][tid & 63] = v;
    __syncthreads();
    if (p != 0 || o >= e6) return;
    v = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
    if (o < e0) dwt[o] = v;
    else if (o < e1) dbt[0] = v;
    else if (o < e2) dw2[o - e1] = v;
    else if (o < e3) db2[o - e2] = v;
    else if (o < e4) dw1[o - e3] = v;
    else if (o < e5) db1[o - e4] = v;
    else {
        const long long k = o - e5;
        (k < (long long)B * rd ? dmul[k] : dadd[k - (long long)B * rd]) = from_f32<bf16_t>(v);
    }
}

// ---- weight pack ----------------------------------------------------------------------------------------------------------
__global__ void baseline_pack_kernel(const float* __restrict__ w_red, const float* __restrict__ w1, const float* __restrict__ w2,
                                     const float* __restrict__ wt, bf16_t* __restrict__ pk, int rd, int rd2, int np) {
    const long long n = packed_elems(np);
    const int KS = np / 32;
    for (long long e = blockIdx.x * (long long)NT + threadIdx.x; e < n; e += (long long)gridDim.x * NT) {
        const int j = (int)(e % 8), l = (int)((e / 8) % 64), lr = l & 15, q = l >> 4;
        float v = 0.f;
        if (e < off_w1f(np)) {                                  // [chunk][mt][s 2]: W_red[16mt + lr][64 chunk + 16q + 8s + j]
            const long long blk = e / 512;
            const int s = (int)(blk % 2), mt = (int)((blk / 2) % (np / 16)), c = (int)(blk / 2 / (np / 16));
            const int row = 16 * mt + lr;
            if (row < rd) v = w_red[(long long)row * DX + 64 * c + 16 * q + 8 * s + j];
        } else if (e < off_wtf(np)) {                           // [mt][KS]: W1[n][c] / W2[c][n], k permuted
            const bool is2 = e >= off_w2f(np);
            const long long blk = (e - (is2 ? off_w2f(np) : off_w1f(np))) / 512;
            const int row = 16 * (int)(blk / KS) + lr, k = 32 * (int)(blk % KS) + kperm(q, j);
            if (!is2 && row < rd2 && k < rd) v = w1[(long long)row * rd + k];
            if (is2 && row < rd && k < rd2) v = w2[(long long)row * rd2 + k];
        } else if (e < off_wtb(np)) {                           // [i 16][KS]: Wt[c][pixel(i, lr)], c permuted
            const long long blk = (e - off_wtf(np)) / 512;
            const int i = (int)(blk / KS), c = 32 * (int)(blk % KS) + kperm(q, j);
            const int pix = 16 * (4 * (i >> 2) + (lr >> 2)) + 4 * (i & 3) + (lr & 3);
            if (c < rd) v = wt[(long long)c * PP + pix];
        } else if (e < off_w2b(np)) {                           // [mt][s 8]: Wt[16mt + lr][32s + 8q + j]
            const long long blk = (e - off_wtb(np)) / 512;
            const int c = 16 * (int)(blk / 8) + lr, pix = 32 * (int)(blk % 8) + 8 * q + j;
            if (c < rd) v = wt[(long long)c * PP + pix];
        } else {                                                // [mt][KS]: W2^T (rows n, k = c) / W1^T (rows c, k = n), k permuted
            const bool is1 = e >= off_w1b(np);
            const long long blk = (e - (is1 ? off_w1b(np) : off_w2b(np))) / 512;
            const int row = 16 * (int)(blk / KS) + lr, k = 32 * (int)(blk % KS) + kperm(q, j);
            if (!is1 && row < rd2 && k < rd) v = w2[(long long)k * rd2 + row];
            if (is1 && row < rd && k < rd2) v = w1[(long long)k * rd + row];
        }
        pk[e] = from_f32<bf16_t>(v);
    }
}

bool supported(int rd, int rd2, int patch) {
    return patch == 16 && rd >= 16 && rd <= 128 && rd % 16 == 0 && rd2 >= 16 && rd2 <= 128 && rd2 % 16 == 0;
}

int check(int dtype, int rd, int rd2, int patch) {
    if (!supported(rd, rd2, patch))
        EGM_FAIL(EGM_ERR_UNSUPPORTED, "baseline head: reduce_dim %d, reduce2_dim %d, patch %d unsupported (patch 16; both dims multiples of "
                                      "16 in 16 .. 128)", rd, rd2, patch);
    if (dtype != EGM_BF16) EGM_FAIL(EGM_ERR_UNSUPPORTED, "baseline head: bf16 only (dtype %d)", dtype);
    return EGM_OK;
}

#define EGM_NP(np, ...) do { switch (np) { \
    case 32: { constexpr int NP = 32; __VA_ARGS__; } break; case 64: { constexpr int NP = 64; __VA_ARGS__; } break; \
    case 96: { constexpr int NP = 96; __VA_ARGS__; } break; default: { constexpr int NP = 128; __VA_ARGS__; } break; } } while (0)

}  // namespace

extern "C" int egm_baseline_supported(int rd, int rd2, int patch) { return supported(rd, rd2, patch) ? 1 : 0; }

extern "C" long long egm_baseline_packed_elems(int rd, int rd2, int patch) {
    const int rc = check(EGM_BF16, rd, rd2, patch);
    return rc != EGM_OK ? rc : packed_elems(np_for(rd, rd2));
}

extern "C" long long egm_baseline_bwd_workspace(int B, int g, int rd, int rd2, int patch) {
    const int rc = check(EGM_BF16, rd, rd2, patch);
    if (rc != EGM_OK) return rc;
    if (B < 1 || g < 1) EGM_FAIL(EGM_ERR_ARG, "baseline_bwd_workspace: bad batch %d / grid %d", B, g);
    const Tiles tl = tiles_for(B, g);
    const int np = np_for(rd, rd2);
    return (tl.nwg * slab_elems(np) + tl.nwt * 2 * np) * 4;
}

extern "C" int egm_baseline_pack(int dtype, const float* w_red, const float* w1, const float* w2, const float* wt, void* packed, int rd,
                                 int rd2, int patch, egm_stream_t s) {
    const int rc = check(dtype, rd, rd2, patch);
    if (rc != EGM_OK) return rc;
    EGM_REQUIRE(w_red && w1 && w2 && wt && packed, "baseline_pack: null pointer");
    const int np = np_for(rd, rd2);
    hipLaunchKernelGGL(baseline_pack_kernel, dim3(egm_cdiv(packed_elems(np), NT)), dim3(NT), 0, (hipStream_t)s, w_red, w1, w2, wt,
                       (bf16_t*)packed, rd, rd2, np);
    EGM_CHECK_LAUNCH("baseline_pack");
    return EGM_OK;
}

extern "C" int egm_baseline_fwd(int dtype, const void* x, int tok_off, int Ltot, const void* mul, const void* add, const void* packed,
                                const float* b_red, const float* b1, const float* b2, const float* bt, void* u, void* h, float* out, int B,
                                int g, int rd, int rd2, int patch, egm_stream_t s) {
    const int rc = check(dtype, rd, rd2, patch);
    if (rc != EGM_OK) return rc;
    EGM_REQUIRE(x && mul && add && packed && b_red && b1 && b2 && bt && out && B > 0 && g > 0 && tok_off >= 0 &&
                Ltot >= tok_off + g * g && (u == nullptr) == (h == nullptr), "baseline_fwd: bad args");
    const Tiles tl = tiles_for(B, g);
    EGM_NP(np_for(rd, rd2), hipLaunchKernelGGL((baseline_fwd_kernel<NP>), dim3(tl.nwg), dim3(NT), 0, (hipStream_t)s, (const bf16_t*)x, tok_off,
                                               Ltot, (const bf16_t*)mul, (const bf16_t*)add, (const bf16_t*)packed, b_red, b1, b2, bt,
                                               (bf16_t*)u, (bf16_t*)h, out, g, rd, rd2, tl.nwt, tl.ntpi));
    EGM_CHECK_LAUNCH("baseline_fwd");
    return EGM_OK;
}

extern "C" int egm_baseline_fwd_multi(int dtype, const void* x, int tok_off, int Ltot, const void* mul, const void* add, const void* packed,
                                      const float* b_red, const float* b1, const float* b2, const float* bt, float* out, int B, int K, int g,
                                      int rd, int rd2, int patch, int prompts_per_group, egm_stream_t s) {
    const int rc = check(dtype, rd, rd2, patch);
    if (rc != EGM_OK) return rc;
    EGM_REQUIRE(x && mul && add && packed && b_red && b1 && b2 && bt && out && B > 0 && K > 0 && g > 0 && tok_off >= 0 &&
                Ltot >= tok_off + g * g, "baseline_fwd_multi: bad args");
    const Tiles tl = tiles_for(B, g);
    int kpg = prompts_per_group;
    if (kpg <= 0) {                        // automatic: enough prompt groups that the grid covers the 256 CUs once
        long long ng = 256 / tl.nwg;
        ng = ng < 1 ? 1 : (ng > K ? K : ng);
        kpg = egm_cdiv(K, ng);
    }
    if (kpg > K) kpg = K;
    const int ngroups = egm_cdiv(K, kpg);
    EGM_REQUIRE(ngroups < 65536, "baseline_fwd_multi: %d prompt groups", ngroups);
    EGM_NP(np_for(rd, rd2), hipLaunchKernelGGL((baseline_fwd_multi_kernel<NP>), dim3(tl.nwg, ngroups), dim3(NT), 0, (hipStream_t)s,
                                               (const bf16_t*)x, tok_off, Ltot, (const bf16_t*)mul, (const bf16_t*)add, (const bf16_t*)packed,
                                               b_red, b1, b2, bt, out, g, rd, rd2, tl.nwt, tl.ntpi, K, kpg));
    EGM_CHECK_LAUNCH("baseline_fwd_multi");
    return EGM_OK;
}

extern "C" int egm_baseline_bwd(int dtype, const float* dout, const void* u, const void* h, const void* mul, const void* add,
                                const void* packed, const float* b2, void* du, int tok_off, int Ltot, float* dwt, float* dbt, float* dw2,
                                float* db2, float* dw1, float* db1, void* dmul, void* dadd, void* workspace, int B, int g, int rd, int rd2,
                                int patch, egm_stream_t s) {
    const int rc = check(dtype, rd, rd2, patch);
    if (rc != EGM_OK) return rc;
    EGM_REQUIRE(dout && u && h && mul && add && packed && b2 && du && dwt && dbt && dw2 && db2 && dw1 && db1 && dmul && dadd && workspace &&
                B > 0 && g > 0 && tok_off >= 0 && Ltot == tok_off + g * g, "baseline_bwd: bad args");
    const Tiles tl = tiles_for(B, g);
    const int np = np_for(rd, rd2);
    float* slabs = (float*)workspace;
    float* film = slabs + tl.nwg * slab_elems(np);
    const long long nout = (long long)rd * PP + 1 + 2LL * rd * rd2 + rd + rd2 + 2LL * B * rd;
    EGM_NP(np, {
        hipLaunchKernelGGL((baseline_bwd_kernel<NP>), dim3(tl.nwg), dim3(NT), 0, (hipStream_t)s, dout, (const bf16_t*)u, (const bf16_t*)h,
                           (const bf16_t*)mul, (const bf16_t*)add, (const bf16_t*)packed, b2, (bf16_t*)du, tok_off, Ltot, slabs, film, g, rd,
                           rd2, tl.nwt, tl.ntpi);
        hipLaunchKernelGGL((baseline_reduce_kernel<NP>), dim3(egm_cdiv(nout, 64)), dim3(NT), 0, (hipStream_t)s, slabs, tl.nwg, film, tl.ntpi,
                           B, rd, rd2, dwt, dbt, dw2, db2, dw1, db1, (bf16_t*)dmul, (bf16_t*)dadd);
    });
    EGM_CHECK_LAUNCH("baseline_bwd");
    return EGM_OK;
}
