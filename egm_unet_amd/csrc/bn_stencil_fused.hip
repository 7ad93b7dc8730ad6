// BatchNorm apply (+activation) fused into the small stencil behind it (bf16; forward only).  Two producer / consumer pairs of the
// training step were an element-wise egm_bn_act_fwd followed by a per-pixel gather kernel that read its result straight back:
//   DoubleConv1 tail -> EdgeEnhancedGRFB entry   src/EGM-UNet.py:894-901 -> :872-886   egm_bn_act_fwd + egm_highpass3
//   Up block tail -> the next Up's concat        src/EGM-UNet.py:952-956 -> :937-947   egm_bn_act_fwd + egm_upcat_fwd
// Neither holds a reduction, so the fused forms are bit-identical: a workgroup stages a pixel tile of one 32-channel chunk in LDS with
// z = round_T(bn_fwd_elem(y)) applied once per staged element (bn_elem.h, rounded as egm_bn_act_fwd stores it) and forms the stencil
// from LDS in the order of the stand-alone kernel (blocks.hip highpass3_kernel, pool_up.hip upcat_fwd_kernel).  The raw conv output is
// read once (halo elements come out of L2) and the intermediate tensor is written once (high-pass: z is still needed by the other
// consumers) or never (upsample: the low-resolution activation has no other reader).
// Workgroups take (tile, chunk) items in the XCD-contiguous order of common.h: the chunks of one 128-byte line meet in one L2.
#include "bn_elem.h"
#include "lerp.h"

namespace {

// the thread's 8 channels are fixed for the whole kernel (256 % 4 == 0 -> vector = tid & 3): coefficients live in registers
__device__ __forceinline__ void load_coef8(const float* __restrict__ scale, const float* __restrict__ shift, int c, bool ok, float (&sc)[8],
                                           float (&sh)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { sc[j] = ok ? scale[c + j] : 0.f; sh[j] = ok ? shift[c + j] : 0.f; }
}

// ---- z = act(scale*y + shift) AND edge = z - avgpool3x3(z) -----------------------------------------------------------------------
// A workgroup owns an 8 x 16 pixel tile of a 32-channel chunk (the halo, 29 % of the staged elements, comes out of L2).  Measured inside
// the benchmarked step against 16 x 32 tiles (halo 16 %): 53.7 / 26.9 / 15.4 / 7.7 us at the four levels against 58.4 / 34.7 / 25.0 /
// 18.5 us -- the large tile leaves CUs idle on the small maps and, with its ten staging loads per thread held in registers, runs at
// half the occupancy on the large ones.
constexpr int HP_TY = 8, HP_TX = 16, HP_CB = 32;
__global__ __launch_bounds__(256) void bn_act_hp_fwd_kernel(const bf16_t* __restrict__ y, int ldy, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, int act, bf16_t* __restrict__ z, int ldz,
                                                            bf16_t* __restrict__ edge, int lde, int N, int H, int W, int C, int tiles_x,
                                                            int tiles_y, int nchunk) {
    constexpr int TY = HP_TY, TX = HP_TX, NB = 3;
    constexpr int PY = TY + 2, PX = TX + 2, NST = PY * PX * 4, NS = (NST + 255) / 256;
    __shared__ __attribute__((aligned(16))) bf16_t sz[PY * PX * HP_CB];            // z of the tile + 1-pixel halo; zeros outside the image
    const int tid = threadIdx.x, vt = tid & 3;
    int b = xcd_contiguous_item(blockIdx.x, gridDim.x);
    const int chunk = b % nchunk; b /= nchunk;
    const int tx = b % tiles_x; b /= tiles_x;
    const int ty = b % tiles_y; const int n = b / tiles_y;
    const int y0 = ty * TY, x0 = tx * TX, c0 = chunk * HP_CB;
    const int nvec = (C - c0 < HP_CB ? C - c0 : HP_CB) >> 3;
    const bool okv = vt < nvec;
    const int c = c0 + vt * 8;
    const long long img = (long long)n * H * W;
    float sc[8], sh[8];
    load_coef8(scale, shift, c, okv, sc, sh);
    // all loads of the thread (NS = 3) are issued before its first LDS store
    static_assert(NS == NB, "one batch");
#pragma unroll
    for (int k0 = 0; k0 < NS; k0 += NB) {
        uint4 raw[NB];
#pragma unroll
        for (int kk = 0; kk < NB; ++kk) {
            const int i = tid + (k0 + kk) * 256, pix = i >> 2, ry = pix / PX, rx = pix - ry * PX;
            const int gy = y0 + ry - 1, gx = x0 + rx - 1;
            raw[kk] = make_uint4(0, 0, 0, 0);
            if (i < NST && okv && gy >= 0 && gy < H && gx >= 0 && gx < W)
                raw[kk] = *reinterpret_cast<const uint4*>(y + (img + (long long)gy * W + gx) * ldy + c);
        }
#pragma unroll
        for (int kk = 0; kk < NB; ++kk) {
            const int i = tid + (k0 + kk) * 256, pix = i >> 2, ry = pix / PX, rx = pix - ry * PX;
            const int gy = y0 + ry - 1, gx = x0 + rx - 1;
            if (i >= NST) break;
            bf16_t* dst = sz + pix * HP_CB + vt * 8;
            if (okv && gy >= 0 && gy < H && gx >= 0 && gx < W) {
                float a[8];
                load8(raw[kk], a);
#pragma unroll
                for (int j = 0; j < 8; ++j) a[j] = bn_fwd_elem<true>(a[j], sc[j], sh[j], act);
                store8_lds(dst, a);
                if (ry >= 1 && ry <= TY && rx >= 1 && rx <= TX)                     // the tile's own pixels: z goes out here
                    store8(z + (img + (long long)gy * W + gx) * ldz + c, a);
            } else {
                *reinterpret_cast<uint4*>(dst) = make_uint4(0, 0, 0, 0);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < TY * TX * 4; i += 256) {
        const int pix = i >> 2, ly = pix / TX, lx = pix - ly * TX;
        const int yy = y0 + ly, xx = x0 + lx;
        if (!okv || yy >= H || xx >= W) continue;
        const bf16_t* base = sz + ((ly + 1) * PX + lx + 1) * HP_CB + vt * 8;
        float s[8], cc[8], v[8];
        zero8(s);
        load8(base, cc);
        // highpass3_kernel's order: r outer, q inner, out-of-image taps skipped
#pragma unroll
        for (int r = -1; r <= 1; ++r)
#pragma unroll
            for (int q = -1; q <= 1; ++q) {
                if (yy + r < 0 || yy + r >= H || xx + q < 0 || xx + q >= W) continue;
                load8(base + (r * PX + q) * HP_CB, v);
#pragma unroll
                for (int j = 0; j < 8; ++j) s[j] += v[j];
            }
#pragma unroll
        for (int j = 0; j < 8; ++j) cc[j] -= s[j] * (1.f / 9.f);
        store8(edge + (img + (long long)yy * W + xx) * lde + c, cc);
    }
}

// ---- out[..., Cs:Cs+Cl] = pad(bilinear_x2_align_corners(act(scale*y_low + shift)))  (+ the skip copy) -----------------------------
// (Lerp, lerp_coord<true>: lerp.h -- the form upcat_fwd_kernel uses, so the weights are the same floats)
// The window a TY x TX output tile reads fits UF_LR x UF_LC low-resolution pixels.  scale = fl((in - 1)/(2 in - 1)) <= 1/2 (rounding is
// monotone and 1/2 is a float), so over the T - 1 steps of a tile the rounded source coordinate grows by less than T/2 (the products
// are below 2^16, their rounding errors below 2^-8), its integer part i0 by at most T/2, and i1 adds one: T/2 + 2 rows / columns
// at most, one fewer than the buffer holds.
constexpr int UF_TY = 16, UF_TX = 32, UF_CB = 32, UF_LR = UF_TY / 2 + 3, UF_LC = UF_TX / 2 + 3;
__global__ __launch_bounds__(256) void bn_act_upcat_fwd_kernel(const bf16_t* __restrict__ skip, int lds, const bf16_t* __restrict__ low, int ldl,
                                                               const float* __restrict__ scale, const float* __restrict__ shift, int act,
                                                               bf16_t* __restrict__ out, int ldo, int N, int Hs, int Ws, int Cs, int Hl, int Wl,
                                                               int Cl, int tiles_x, int tiles_y, int nsc, int nlc) {
    __shared__ __attribute__((aligned(16))) bf16_t sl[UF_LR * UF_LC * UF_CB];      // act(BatchNorm(low)) of the rows / columns the tile reads
    __shared__ Lerp sly[UF_TY], slx[UF_TX];                                        // interpolation of the tile's rows / columns (indices relative
                                                                                   // to the staged window), once per workgroup
    const int tid = threadIdx.x, vt = tid & 3;
    int b = xcd_contiguous_item(blockIdx.x, gridDim.x);
    const int nchunk = nsc + nlc;
    const int chunk = b % nchunk; b /= nchunk;
    const int tx = b % tiles_x; b /= tiles_x;
    const int ty = b % tiles_y; const int n = b / tiles_y;
    const int y0 = ty * UF_TY, x0 = tx * UF_TX;
    const long long img = (long long)n * Hs * Ws;
    if (chunk < nsc) {                                                             // a chunk of the skip tensor: plain copy
        const int c0 = chunk * UF_CB, nvec = (Cs - c0 < UF_CB ? Cs - c0 : UF_CB) >> 3;
        for (int i = tid; i < UF_TY * UF_TX * 4; i += 256) {
            const int pix = i >> 2, ly = pix / UF_TX, lx = pix - ly * UF_TX;
            const int yy = y0 + ly, xx = x0 + lx;
            if (vt >= nvec || yy >= Hs || xx >= Ws) continue;
            const long long p = img + (long long)yy * Ws + xx;
            float v[8];
            load8(skip + p * lds + c0 + vt * 8, v);
            store8(out + p * ldo + c0 + vt * 8, v);
        }
        return;
    }
    const int c0 = (chunk - nsc) * UF_CB, nvec = (Cl - c0 < UF_CB ? Cl - c0 : UF_CB) >> 3;
    const bool okv = vt < nvec;
    const int c = c0 + vt * 8;
    const int Hu = 2 * Hl, Wu = 2 * Wl, py = (Hs - Hu) / 2, px = (Ws - Wu) / 2;
    // the up-sampled rows / columns this tile covers (the rest of it is the zero pad border or lies outside the image)
    const int yend = y0 + UF_TY < Hs ? y0 + UF_TY : Hs, xend = x0 + UF_TX < Ws ? x0 + UF_TX : Ws;
    const int uy_lo = y0 - py > 0 ? y0 - py : 0, uy_hi = yend - 1 - py < Hu - 1 ? yend - 1 - py : Hu - 1;
    const int ux_lo = x0 - px > 0 ? x0 - px : 0, ux_hi = xend - 1 - px < Wu - 1 ? xend - 1 - px : Wu - 1;
    const bool any = uy_lo <= uy_hi && ux_lo <= ux_hi;
    int r0 = 0, nr = 0, q0 = 0, nq = 0;
    if (any) {
        r0 = lerp_coord<true>(uy_lo, Hl, Hu).i0; nr = lerp_coord<true>(uy_hi, Hl, Hu).i1 - r0 + 1;
        q0 = lerp_coord<true>(ux_lo, Wl, Wu).i0; nq = lerp_coord<true>(ux_hi, Wl, Wu).i1 - q0 + 1;
    }
    if (tid < UF_TY) {
        const int uy = y0 + tid - py;
        Lerp l; l.i0 = 0; l.i1 = 0; l.w0 = 0.f; l.w1 = 0.f;
        if (uy >= uy_lo && uy <= uy_hi) { l = lerp_coord<true>(uy, Hl, Hu); l.i0 -= r0; l.i1 -= r0; }
        sly[tid] = l;
    } else if (tid >= 64 && tid < 64 + UF_TX) {
        const int ux = x0 + tid - 64 - px;
        Lerp l; l.i0 = 0; l.i1 = 0; l.w0 = 0.f; l.w1 = 0.f;
        if (ux >= ux_lo && ux <= ux_hi) { l = lerp_coord<true>(ux, Wl, Wu); l.i0 -= q0; l.i1 -= q0; }
        slx[tid - 64] = l;
    }
    float sc[8], sh[8];
    load_coef8(scale, shift, c, okv, sc, sh);
    const bf16_t* __restrict__ lowb = low + (long long)n * Hl * Wl * ldl + c;
    for (int i = tid; i < nr * nq * 4; i += 256) {
        const int pix = i >> 2, rr = pix / nq, qq = pix - rr * nq;
        if (!okv) continue;
        float a[8];
        load8(lowb + ((long long)(r0 + rr) * Wl + q0 + qq) * ldl, a);
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = bn_fwd_elem<true>(a[j], sc[j], sh[j], act);
        store8_lds(sl + (rr * UF_LC + qq) * UF_CB + vt * 8, a);
    }
    __syncthreads();
    for (int i = tid; i < UF_TY * UF_TX * 4; i += 256) {
        const int pix = i >> 2, ly = pix / UF_TX, lx = pix - ly * UF_TX;
        const int yy = y0 + ly, xx = x0 + lx;
        if (!okv || yy >= Hs || xx >= Ws) continue;
        const int uy = yy - py, ux = xx - px;
        float v[8];
        zero8(v);
        if (uy >= 0 && uy < Hu && ux >= 0 && ux < Wu) {
            const Lerp ay = sly[ly], ax = slx[lx];
            const bf16_t* sb = sl + vt * 8;
            float a[8];
            // upcat_fwd_kernel's order: (i0,i0), (i0,i1), (i1,i0), (i1,i1), each as v += wy*wx*a
            load8(sb + (ay.i0 * UF_LC + ax.i0) * UF_CB, a);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] += ay.w0 * ax.w0 * a[j];
            load8(sb + (ay.i0 * UF_LC + ax.i1) * UF_CB, a);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] += ay.w0 * ax.w1 * a[j];
            load8(sb + (ay.i1 * UF_LC + ax.i0) * UF_CB, a);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] += ay.w1 * ax.w0 * a[j];
            load8(sb + (ay.i1 * UF_LC + ax.i1) * UF_CB, a);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] += ay.w1 * ax.w1 * a[j];
        }
        store8(out + (img + (long long)yy * Ws + xx) * ldo + Cs + c, v);
    }
}

}  // namespace

extern "C" int egm_bn_act_hp_fwd(int dtype, const void* y, int ldy, const float* scale, const float* shift, int act, void* z, int ldz,
                                 void* edge, int lde, int N, int H, int W, int C, egm_stream_t s) {
    EGM_REQUIRE(dtype == EGM_BF16, "bn_act_hp_fwd: bf16 only (dtype %d); other types take egm_bn_act_fwd + egm_highpass3", dtype);
    EGM_REQ_VEC("bn_act_hp_fwd", y, ldy, C); EGM_REQ_VEC("bn_act_hp_fwd", z, ldz, C); EGM_REQ_VEC("bn_act_hp_fwd", edge, lde, C);
    EGM_REQUIRE(scale && shift && N > 0 && H > 0 && W > 0 && act >= EGM_ACT_NONE && act <= EGM_ACT_SILU, "bn_act_hp_fwd: bad args");
    const int nchunk = egm_cdiv(C, HP_CB);
    const int tiles_y = egm_cdiv(H, HP_TY), tiles_x = egm_cdiv(W, HP_TX);
    const long long grid = (long long)N * tiles_y * tiles_x * nchunk;
    EGM_REQUIRE(grid < (1ll << 31), "bn_act_hp_fwd: tensor too large");
    hipLaunchKernelGGL(bn_act_hp_fwd_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)s, (const bf16_t*)y, ldy, scale, shift, act,
                       (bf16_t*)z, ldz, (bf16_t*)edge, lde, N, H, W, C, tiles_x, tiles_y, nchunk);
    EGM_CHECK_LAUNCH("bn_act_hp_fwd");
    return EGM_OK;
}

extern "C" int egm_bn_act_upcat_fwd(int dtype, const void* skip, int lds, const void* low, int ldl, const float* scale, const float* shift,
                                    int act, void* out, int ldo, int N, int Hs, int Ws, int Cs, int Hl, int Wl, int Cl, egm_stream_t s) {
    EGM_REQUIRE(dtype == EGM_BF16, "bn_act_upcat_fwd: bf16 only (dtype %d); other types take egm_bn_act_fwd + egm_upcat_fwd", dtype);
    if (skip != nullptr) EGM_REQ_VEC("bn_act_upcat_fwd", skip, lds, Cs);
    EGM_REQUIRE(Cs > 0 && Cs % 8 == 0, "bn_act_upcat_fwd: bad Cs %d", Cs);
    EGM_REQ_VEC("bn_act_upcat_fwd", low, ldl, Cl);
    EGM_REQ_VEC("bn_act_upcat_fwd", out, ldo, Cs + Cl);
    EGM_REQUIRE(scale && shift && act >= EGM_ACT_NONE && act <= EGM_ACT_SILU, "bn_act_upcat_fwd: bad args");
    EGM_REQUIRE(N > 0 && Hl > 0 && Wl > 0 && Hs >= 2 * Hl && Ws >= 2 * Wl, "bn_act_upcat_fwd: skip must be at least 2x the low-res size");
    const int tiles_y = egm_cdiv(Hs, UF_TY), tiles_x = egm_cdiv(Ws, UF_TX);
    const int nsc = skip ? egm_cdiv(Cs, UF_CB) : 0, nlc = egm_cdiv(Cl, UF_CB);
    const long long grid = (long long)N * tiles_y * tiles_x * (nsc + nlc);
    EGM_REQUIRE(grid < (1ll << 31), "bn_act_upcat_fwd: tensor too large");
    hipLaunchKernelGGL(bn_act_upcat_fwd_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)s, (const bf16_t*)skip, lds, (const bf16_t*)low,
                       ldl, scale, shift, act, (bf16_t*)out, ldo, N, Hs, Ws, Cs, Hl, Wl, Cl, tiles_x, tiles_y, nsc, nlc);
    EGM_CHECK_LAUNCH("bn_act_upcat_fwd");
    return EGM_OK;
}
