// Guided upsampling: the fast guided filter (He, Sun, Tang 2013 / 2015) with a colour guide.  At the model's size the
// scores are fitted as a local linear function of the photo's three colours, the coefficients are smoothed, and the linear function is
// evaluated on the full-resolution photo, so the mask's edge follows the photo's colour edge instead of the model's grid.
//   egm_guided_coefs_f32  guide [N][3][h][w] and scores [N][C][h][w] (or a uint8 class map read as one-hot scores) -> A [N][h][w][4C]
//                         launch 1: box means of the 9 + 4C moments, the 3 x 3 solve per pixel -> unsmoothed (a0, a1, a2, b) per class
//                         launch 2: the box mean of those 4C channels -> A
//   egm_guided_apply_u8   photos uint8 [N][H0][W0][3] and A -> mask uint8 [N][H0][W0] (and q fp32 [N][C][H0][W0]): A sampled bilinearly
//                         from host-made integer taps (egm_unet_amd.tta.resize_axis), q_c = a . I + b, mask = lut[argmax_c q_c]
// The arithmetic is fixed so that a numpy float32 restatement gives the same bits (tests/guided_oracle.py): every multiply, add,
// subtract and divide is one fp32 rounding in the order written here, and none is contracted into an FMA.
//   box mean  of a channel X at (y, x), the window clipped to the image: t[y'][x] = X[y'][xlo], t = t + X[y'][k] for k ascending to xhi;
//             u = t[ylo][x], u = u + t[k][x] for k ascending to yhi; mean = u / float(rows * columns of the window)
//   shape     coefficients: a workgroup owns a kGfTile x kGfTile tile of one image and stages the guide and the scores with an r-pixel
//             clipped halo in LDS; a pass runs the row sums of up to four channels (products formed on the fly) into an LDS strip,
//             then the column sums out of it, every thread keeping the means of its own pixel.  Grid dimensions carry the tiles and N
//             (and, in launch 2, the class): two launches whatever N and C.
//             apply: the strip frame of strip_out.h, a lane owns 4 consecutive photo pixels of one row.  Its 12 RGB bytes are three
//             dwords where the row's address allows it, the mask leaves as one non-temporal dword; ragged ends go by bytes.  A
//             workgroup's strip needs a few rows of A and about w / W0 of 256 columns: that span is staged in LDS once per strip
//             where it fits kGfStageLimit (measured: 56 us against 73 us of gathers at 3000 x 4000), else gathered.
// Every index read from a table is clamped into [0, side - 1] before it addresses memory.  No atomics.
#include <math.h>
#include "strip_out.h"

// (as csrc/tta.hip: the pragma governs the operators written below it, so all arithmetic on samples stays in this file)
#pragma clang fp contract(off)

namespace {

constexpr int kGfTile = 16;                            // tile side of the two coefficient launches (the GPU tests restate it)
constexpr int kGfMaxR = 16;
constexpr int kGfMaxC = 8;
constexpr int kGfLdsLimit = 160 * 1024;                // the LDS of a CU
constexpr int kGfThreads = kGfTile * kGfTile;
constexpr int kGfStageLimit = 32 * 1024;               // bytes of A a strip of the apply launch stages in LDS at most (the GPU tests restate it)

struct GfTile { int n, y0, x0, P; };                   // the tile's image and origin; P = kGfTile + 2 r, the staged side
__device__ __forceinline__ GfTile gf_tile(int w, int r) {
    const int tx = (w + kGfTile - 1) / kGfTile;
    return {(int)blockIdx.z, (int)(blockIdx.x / tx) * kGfTile, (int)(blockIdx.x % tx) * kGfTile, kGfTile + 2 * r};
}

// The box means of K channels at the thread's own pixel (py, px) of the tile.  val(i, v) gives the K channel values at staged index
// i = ly * P + lx.  strip: K * P * kGfTile floats.  Every thread of the workgroup calls it (two barriers); a thread whose pixel is
// outside the image gets zeros.
template <int K, typename F>
__device__ __forceinline__ void box_means(const GfTile& t, int h, int w, int r, float* __restrict__ strip, F val, float (&mean)[K]) {
    const int P = t.P;
    __syncthreads();                                           // the strip's readers of the pass before are done
    for (int item = threadIdx.x; item < P * kGfTile; item += kGfThreads) {
        const int ly = item / kGfTile, lx = item % kGfTile;
        const int gy = t.y0 - r + ly, gx = t.x0 + lx;
        if (gy < 0 || gy >= h || gx >= w) continue;
        const int lo = max(0, gx - r) - (t.x0 - r), hi = min(w - 1, gx + r) - (t.x0 - r);
        float acc[K], v[K];
        val(ly * P + lo, acc);
        for (int k = lo + 1; k <= hi; ++k) {
            val(ly * P + k, v);
#pragma unroll
            for (int c = 0; c < K; ++c) acc[c] = acc[c] + v[c];
        }
#pragma unroll
        for (int c = 0; c < K; ++c) strip[(c * P + ly) * kGfTile + lx] = acc[c];
    }
    __syncthreads();
    const int py = threadIdx.x / kGfTile, px = threadIdx.x % kGfTile;
    const int gy = t.y0 + py, gx = t.x0 + px;
#pragma unroll
    for (int c = 0; c < K; ++c) mean[c] = 0.f;
    if (gy >= h || gx >= w) return;
    const int ylo = max(0, gy - r), yhi = min(h - 1, gy + r), xlo = max(0, gx - r), xhi = min(w - 1, gx + r);
    const int lo = ylo - (t.y0 - r), hi = yhi - (t.y0 - r);
    const float cnt = (float)((yhi - ylo + 1) * (xhi - xlo + 1));
#pragma unroll
    for (int c = 0; c < K; ++c) {
        float u = strip[(c * P + lo) * kGfTile + px];
        for (int k = lo + 1; k <= hi; ++k) u = u + strip[(c * P + k) * kGfTile + px];
        mean[c] = u / cnt;                                      // correctly rounded: hipcc's default for fp32 division
    }
}

struct Eps3 { float e[3]; };

// launch 1: moments -> covariance -> the solve by cofactors -> ab [N][h][w][4C], unsmoothed
__global__ __launch_bounds__(kGfThreads) void guided_fit_kernel(const float* __restrict__ guide, const float* __restrict__ scores,
                                                                const unsigned char* __restrict__ cls, int C, int h, int w, int r, Eps3 eps,
                                                                float* __restrict__ ab) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const GfTile t = gf_tile(w, r);
    const int P = t.P, PP = P * P;
    float* g = lds;                                            // [3][P][P]
    float* sc = lds + 3 * PP;                                  // [C][P][P]
    float* strip = sc + C * PP;                                // [4][P][kGfTile]
    const long long hw = (long long)h * w;
    for (int i = threadIdx.x; i < PP; i += kGfThreads) {
        const int gy = t.y0 - r + i / P, gx = t.x0 - r + i % P;
        const bool in = gy >= 0 && gy < h && gx >= 0 && gx < w;
        const long long pix = in ? (long long)gy * w + gx : 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c * PP + i] = in ? guide[((long long)t.n * 3 + c) * hw + pix] : 0.f;
        if (scores) {
            for (int c = 0; c < C; ++c) sc[c * PP + i] = in ? scores[((long long)t.n * C + c) * hw + pix] : 0.f;
        } else {
            const int k = in ? cls[(long long)t.n * hw + pix] : -1;
            for (int c = 0; c < C; ++c) sc[c * PP + i] = k == c ? 1.f : 0.f;
        }
    }
    const float *g0 = g, *g1 = g + PP, *g2 = g + 2 * PP;
    float m1[4], m2[4], m3[1];                                  // (G0, G1, G2, G0 G0), (G0 G1, G0 G2, G1 G1, G1 G2), (G2 G2)
    box_means<4>(t, h, w, r, strip, [&](int i, float (&v)[4]) { v[0] = g0[i]; v[1] = g1[i]; v[2] = g2[i]; v[3] = g0[i] * g0[i]; }, m1);
    box_means<4>(t, h, w, r, strip, [&](int i, float (&v)[4]) { v[0] = g0[i] * g1[i]; v[1] = g0[i] * g2[i]; v[2] = g1[i] * g1[i];
                                                                 v[3] = g1[i] * g2[i]; }, m2);
    box_means<1>(t, h, w, r, strip, [&](int i, float (&v)[1]) { v[0] = g2[i] * g2[i]; }, m3);
    const float mg0 = m1[0], mg1 = m1[1], mg2 = m1[2];
    const float s00 = (m1[3] - mg0 * mg0) + eps.e[0], s01 = m2[0] - mg0 * mg1, s02 = m2[1] - mg0 * mg2;
    const float s11 = (m2[2] - mg1 * mg1) + eps.e[1], s12 = m2[3] - mg1 * mg2, s22 = (m3[0] - mg2 * mg2) + eps.e[2];
    const float c00 = s11 * s22 - s12 * s12, c01 = s02 * s12 - s01 * s22, c02 = s01 * s12 - s02 * s11;
    const float c11 = s00 * s22 - s02 * s02, c12 = s01 * s02 - s00 * s12, c22 = s00 * s11 - s01 * s01;
    const float det = (s00 * c00 + s01 * c01) + s02 * c02;
    const int gy = t.y0 + threadIdx.x / kGfTile, gx = t.x0 + threadIdx.x % kGfTile;
    for (int c = 0; c < C; ++c) {                               // (uniform: box_means has barriers)
        const float* s = sc + c * PP;
        float m[4];                                             // (S, G0 S, G1 S, G2 S)
        box_means<4>(t, h, w, r, strip, [&](int i, float (&v)[4]) { v[0] = s[i]; v[1] = g0[i] * s[i]; v[2] = g1[i] * s[i]; v[3] = g2[i] * s[i]; },
                     m);
        if (gy >= h || gx >= w) continue;
        const float v0 = m[1] - mg0 * m[0], v1 = m[2] - mg1 * m[0], v2 = m[3] - mg2 * m[0];
        const float a0 = ((c00 * v0 + c01 * v1) + c02 * v2) / det;
        const float a1 = ((c01 * v0 + c11 * v1) + c12 * v2) / det;
        const float a2 = ((c02 * v0 + c12 * v1) + c22 * v2) / det;
        const float b = ((m[0] - a0 * mg0) - a1 * mg1) - a2 * mg2;
        *reinterpret_cast<float4*>(ab + (((long long)t.n * h + gy) * w + gx) * (4 * C) + 4 * c) = make_float4(a0, a1, a2, b);
    }
}

// launch 2: A = the box mean of ab, one class (four channels, one 16-byte element per pixel) per workgroup
__global__ __launch_bounds__(kGfThreads) void guided_smooth_kernel(const float* __restrict__ ab, int C, int h, int w, int r,
                                                                   float* __restrict__ A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const GfTile t = gf_tile(w, r);
    const int P = t.P, PP = P * P, c = blockIdx.y;
    float4* st = reinterpret_cast<float4*>(lds);               // [P][P]
    float* strip = lds + 4 * PP;                               // [4][P][kGfTile]
    for (int i = threadIdx.x; i < PP; i += kGfThreads) {
        const int gy = t.y0 - r + i / P, gx = t.x0 - r + i % P;
        const bool in = gy >= 0 && gy < h && gx >= 0 && gx < w;
        st[i] = in ? *reinterpret_cast<const float4*>(ab + (((long long)t.n * h + gy) * w + gx) * (4 * C) + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float m[4];
    box_means<4>(t, h, w, r, strip, [&](int i, float (&v)[4]) { const float4 e = st[i]; v[0] = e.x; v[1] = e.y; v[2] = e.z; v[3] = e.w; }, m);
    const int gy = t.y0 + threadIdx.x / kGfTile, gx = t.x0 + threadIdx.x % kGfTile;
    if (gy >= h || gx >= w) return;
    *reinterpret_cast<float4*>(A + (((long long)t.n * h + gy) * w + gx) * (4 * C) + 4 * c) = make_float4(m[0], m[1], m[2], m[3]);
}

// the two taps and weights of one axis for output pixel p, the indices clamped into [0, side - 1] (as csrc/tta.hip)
struct GfTaps { int i0, i1; float l0, l1; };
__device__ __forceinline__ GfTaps gf_taps(const int* __restrict__ idx, const float* __restrict__ l, int p, int side) {
    GfTaps t;
    t.i0 = clampi(idx[2 * p], 0, side - 1);
    t.i1 = clampi(idx[2 * p + 1], 0, side - 1);
    t.l1 = l[p];
    t.l0 = 1.f - t.l1;
    return t;
}
__device__ __forceinline__ float gf_bilinear(float a, float b, float c, float d, const GfTaps& ty, const GfTaps& tx) {
    const float ta = tx.l0 * a, tb = tx.l1 * b, tc = tx.l0 * c, td = tx.l1 * d;
    const float top = ta + tb, bot = tc + td;
    const float vt = ty.l0 * top, vb = ty.l1 * bot;
    return vt + vb;
}

struct Affine3 { float scale[3], offset[3]; };

// The span of A that the workgroup's strip (kStripRows rows x kStripCols columns of the photo) reads: rows [r_lo, r_lo + rspan) and columns
// [c_lo, c_lo + cspan), r_lo / c_lo the first taps of the strip's first row / column.  With the taps of resize_axis the strip's rows reach
// at most floor((kStripRows - 1) h / H0) + 2 rows past r_lo (the columns likewise): the host sizes the span by that, and a tap is clamped
// into the span, so a wrong table gives wrong pixels, never an access outside it.
struct GfSpan { int rspan, cspan; };

// STAGE: the span is copied into LDS once per strip and the taps are LDS reads; otherwise (a span too large for LDS: ratios near 1 and
// below with many classes) the taps are gathers from global memory.  The arithmetic is the same code.
template <bool STAGE>
__global__ __launch_bounds__(256) void guided_apply_kernel(const unsigned char* __restrict__ imgs, int H0, int W0, const float* __restrict__ A,
                                                           int C, int h, int w, const int* __restrict__ yi, const float* __restrict__ yl,
                                                           const int* __restrict__ xi, const float* __restrict__ xl, Affine3 aff,
                                                           const unsigned char* __restrict__ lut, unsigned char* __restrict__ mask,
                                                           float* __restrict__ q_out, int nrg, int ncg, int vec_q, GfSpan span) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const float4* st = reinterpret_cast<const float4*>(lds);   // [rspan][cspan][C]
    const auto [n, y, x, outside] = strip_pos(nrg, ncg, H0, W0);
    int r_lo = 0, c_lo = 0;
    if (STAGE) {                                               // every thread of the workgroup, the ones outside the image too
        const int cg = blockIdx.x % ncg, rg = (blockIdx.x / ncg) % nrg;
        r_lo = clampi(yi[2 * (rg * kStripRows)], 0, h - 1);
        c_lo = clampi(xi[2 * (cg * kStripCols)], 0, w - 1);
        float4* dst = reinterpret_cast<float4*>(lds);
        const int per_row = span.cspan * C, last = w * C - 1;     // a row of the span is one run of 16-byte elements of A's row
        for (int rr = 0; rr < span.rspan; ++rr) {
            const float4* arow = reinterpret_cast<const float4*>(A) + ((long long)n * h + min(r_lo + rr, h - 1)) * w * C;
            for (int k = threadIdx.x; k < per_row; k += 256) dst[rr * per_row + k] = arow[min(c_lo * C + k, last)];
        }
        __syncthreads();
    }
    if (outside) return;
    const bool whole = x + kStripLanePix <= W0;                // the lane's four pixels are all in the row
    // the photo's bytes: the row's own address decides, image n starts n * H0 * W0 * 3 bytes in at whatever alignment that is
    const unsigned char* row = imgs + ((long long)n * H0 + y) * W0 * 3;
    unsigned int px[3 * kStripLanePix];
    if (whole && (reinterpret_cast<uintptr_t>(row) & 3) == 0) {
        const unsigned int* p = reinterpret_cast<const unsigned int*>(row + 3 * x);
        const unsigned int d0 = __builtin_nontemporal_load(p), d1 = __builtin_nontemporal_load(p + 1), d2 = __builtin_nontemporal_load(p + 2);
#pragma unroll
        for (int k = 0; k < 4; ++k) { px[k] = (d0 >> (8 * k)) & 255u; px[4 + k] = (d1 >> (8 * k)) & 255u; px[8 + k] = (d2 >> (8 * k)) & 255u; }
    } else {
#pragma unroll
        for (int k = 0; k < 3 * kStripLanePix; ++k) px[k] = x + k / 3 < W0 ? row[3 * x + k] : 0u;
    }
    float I[kStripLanePix][3];
#pragma unroll
    for (int e = 0; e < kStripLanePix; ++e)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float f = (float)px[3 * e + i] * aff.scale[i];
            I[e][i] = f + aff.offset[i];
        }
    const GfTaps ty = gf_taps(yi, yl, y, h);                   // wave-uniform
    GfTaps tx[kStripLanePix];
#pragma unroll
    for (int e = 0; e < kStripLanePix; ++e) tx[e] = gf_taps(xi, xl, min(x + e, W0 - 1), w);
    // the taps' places in 16-byte elements: of the staged span, or of image n's part of A (below 2^29, checked by the launcher)
    const float4* src = STAGE ? st : reinterpret_cast<const float4*>(A) + (long long)n * h * w * C;
    const int pitch = STAGE ? span.cspan * C : w * C;
    const int ry0 = STAGE ? clampi(ty.i0 - r_lo, 0, span.rspan - 1) : ty.i0, ry1 = STAGE ? clampi(ty.i1 - r_lo, 0, span.rspan - 1) : ty.i1;
    int o0[kStripLanePix], o1[kStripLanePix];
#pragma unroll
    for (int e = 0; e < kStripLanePix; ++e) {
        o0[e] = (STAGE ? clampi(tx[e].i0 - c_lo, 0, span.cspan - 1) : tx[e].i0) * C;
        o1[e] = (STAGE ? clampi(tx[e].i1 - c_lo, 0, span.cspan - 1) : tx[e].i1) * C;
    }
    const float4* r0 = src + ry0 * pitch;
    const float4* r1 = src + ry1 * pitch;
    StripArgmax top;
    for (int c = 0; c < C; ++c) {
        float q[kStripLanePix];
#pragma unroll
        for (int e = 0; e < kStripLanePix; ++e) {
            const float4 ta = r0[o0[e] + c], tb = r0[o1[e] + c], tc = r1[o0[e] + c], td = r1[o1[e] + c];
            const float a0 = gf_bilinear(ta.x, tb.x, tc.x, td.x, ty, tx[e]), a1 = gf_bilinear(ta.y, tb.y, tc.y, td.y, ty, tx[e]);
            const float a2 = gf_bilinear(ta.z, tb.z, tc.z, td.z, ty, tx[e]), b = gf_bilinear(ta.w, tb.w, tc.w, td.w, ty, tx[e]);
            const float p0 = a0 * I[e][0], p1 = a1 * I[e][1], p2 = a2 * I[e][2];
            q[e] = ((p0 + p1) + p2) + b;
            top.take(c, e, q[e]);
        }
        if (q_out) store_row4(q_out + (((long long)n * C + c) * H0 + y) * W0 + x, q, x, W0, vec_q);
    }
    unsigned int m[kStripLanePix];
#pragma unroll
    for (int e = 0; e < kStripLanePix; ++e) m[e] = lut ? lut[top.arg[e]] : (unsigned int)top.arg[e];
    unsigned char* o = mask + ((long long)n * H0 + y) * W0 + x;
    if (whole && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        __builtin_nontemporal_store(m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24), reinterpret_cast<unsigned int*>(o));
    } else {
#pragma unroll
        for (int e = 0; e < kStripLanePix; ++e)
            if (x + e < W0) __builtin_nontemporal_store((unsigned char)m[e], o + e);
    }
}

// the bytes of LDS the two coefficient launches stage for radius r and C classes
constexpr size_t fit_lds(int r, int C) { const size_t P = kGfTile + 2 * r; return ((3 + C) * P * P + 4 * P * kGfTile) * sizeof(float); }
constexpr size_t smooth_lds(int r) { const size_t P = kGfTile + 2 * r; return (4 * P * P + 4 * P * kGfTile) * sizeof(float); }
// The host's choice of the tile from r and C is one tile for all of them: kGfTile fits a CU's LDS at the largest rule (111 KiB at r = 16,
// C = 8; a 32 x 32 tile would need 176 KiB), and the coefficient launches are not what bounds the tail at the small ones.
static_assert(fit_lds(kGfMaxR, kGfMaxC) <= (size_t)kGfLdsLimit && smooth_lds(kGfMaxR) <= (size_t)kGfLdsLimit,
              "guided.hip: kGfTile does not fit the LDS at the largest radius and class count");

int guided_shape_check(const char* name, int N, int C, int h, int w) {
    EGM_REQUIRE(N > 0 && h > 0 && w > 0, "%s: bad shape N=%d h=%d w=%d", name, N, h, w);
    EGM_REQUIRE(C >= 1 && C <= kGfMaxC, "%s: %d classes, between 1 and %d are supported", name, C, kGfMaxC);
    EGM_REQUIRE(h <= kStripMaxSide && w <= kStripMaxSide, "%s: %d x %d pixels, at most %d rows and columns are supported", name, h, w,
                kStripMaxSide);
    EGM_REQUIRE(N <= 65535, "%s: %d images in one call, at most 65535 are supported", name, N);
    return EGM_OK;
}

template <typename K>
int raise_lds(const char* name, K kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return EGM_OK;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) EGM_FAIL(EGM_ERR_LAUNCH, "%s: hipFuncSetAttribute: %s", name, hipGetErrorString(e));
    return EGM_OK;
}

}  // namespace

extern "C" long long egm_guided_workspace(int N, int C, int h, int w) {
    if (const int rc = guided_shape_check("guided_workspace", N, C, h, w); rc != EGM_OK) return rc;
    return (long long)N * h * w * 4 * C * (long long)sizeof(float);
}

extern "C" int egm_guided_coefs_f32(const float* guide, const float* scores, const unsigned char* cls, int N, int C, int h, int w, int r,
                                    float eps0, float eps1, float eps2, float* A_out, void* workspace, egm_stream_t s) {
    const char* name = "guided_coefs_f32";
    EGM_REQUIRE(guide && A_out && workspace, "%s: null pointer", name);
    EGM_REQUIRE(scores || cls, "%s: null pointer (neither scores nor a class map: exactly one is required)", name);
    EGM_REQUIRE(!(scores && cls), "%s: both scores and a class map: exactly one is required", name);
    if (const int rc = guided_shape_check(name, N, C, h, w); rc != EGM_OK) return rc;
    EGM_REQUIRE(r >= 1 && r <= kGfMaxR, "%s: radius %d, between 1 and %d is supported", name, r, kGfMaxR);
    const float eps[3] = {eps0, eps1, eps2};
    for (int i = 0; i < 3; ++i) EGM_REQUIRE(isfinite(eps[i]) && eps[i] > 0.f, "%s: eps[%d] = %g, a finite number above 0 expected", name, i, eps[i]);
    EGM_REQUIRE(egm_aligned16(A_out) && egm_aligned16(workspace), "%s: A_out and the workspace must be 16-byte aligned", name);
    const size_t lds1 = fit_lds(r, C), lds2 = smooth_lds(r);        // (within kGfLdsLimit for every r and C let through above)
    const long long tiles = (long long)egm_cdiv(h, kGfTile) * egm_cdiv(w, kGfTile);
    if (const int rc = raise_lds(name, guided_fit_kernel, lds1); rc != EGM_OK) return rc;
    if (const int rc = raise_lds(name, guided_smooth_kernel, lds2); rc != EGM_OK) return rc;
    float* ab = static_cast<float*>(workspace);
    hipLaunchKernelGGL(guided_fit_kernel, dim3((unsigned)tiles, 1, N), dim3(kGfThreads), lds1, (hipStream_t)s, guide, scores, cls, C, h, w, r,
                       Eps3{{eps0, eps1, eps2}}, ab);
    EGM_CHECK_LAUNCH("guided_coefs_f32 (fit)");
    hipLaunchKernelGGL(guided_smooth_kernel, dim3((unsigned)tiles, C, N), dim3(kGfThreads), lds2, (hipStream_t)s, ab, C, h, w, r, A_out);
    EGM_CHECK_LAUNCH("guided_coefs_f32 (smooth)");
    return EGM_OK;
}

extern "C" int egm_guided_apply_u8(const unsigned char* imgs, int N, int H0, int W0, const float* A, int C, int h, int w, const int* yi_dev,
                                   const float* yl_dev, const int* xi_dev, const float* xl_dev, float scale0, float scale1, float scale2,
                                   float offset0, float offset1, float offset2, const unsigned char* lut, unsigned char* mask_out,
                                   float* q_out, egm_stream_t s) {
    const char* name = "guided_apply_u8";
    EGM_REQUIRE(imgs && A && mask_out, "%s: null pointer", name);
    EGM_REQUIRE(yi_dev && yl_dev && xi_dev && xl_dev, "%s: null pointer (the four axis tables are required)", name);
    if (const int rc = guided_shape_check(name, N, C, h, w); rc != EGM_OK) return rc;
    StripGrid g;
    if (const int rc = strip_check(name, N, C, H0, W0, q_out, mask_out, &g); rc != EGM_OK) return rc;
    EGM_REQUIRE(egm_aligned16(A), "%s: A must be 16-byte aligned", name);
    EGM_REQUIRE((long long)h * w * C < (1ll << 31) / 4, "%s: %d x %d coefficients of %d classes per image, fewer than 2^29 are supported", name, h, w, C);
    // the span of A behind one strip of the photo (GfSpan), staged in LDS where it fits kGfStageLimit bytes
    const GfSpan span = {(int)min((long long)h, (long long)(kStripRows - 1) * h / H0 + 3), (int)min((long long)w, (long long)(kStripCols - 1) * w / W0 + 3)};
    const size_t staged = (size_t)span.rspan * span.cspan * C * 16;
    const bool stage = staged <= (size_t)kGfStageLimit;
    hipLaunchKernelGGL(stage ? guided_apply_kernel<true> : guided_apply_kernel<false>, dim3((unsigned)g.items), dim3(256), stage ? staged : 0,
                       (hipStream_t)s, imgs, H0, W0, A, C, h, w, yi_dev, yl_dev, xi_dev, xl_dev,
                       Affine3{{scale0, scale1, scale2}, {offset0, offset1, offset2}}, lut, mask_out, q_out, g.nrg, g.ncg, g.vec_logits, span);
    EGM_CHECK_LAUNCH("guided_apply_u8");
    return EGM_OK;
}
