// Boundary loss of Kervadec et al. on the device: the signed squared Euclidean distance of every pixel of an int64
// target to the contour of K of its classes, all in integers, and the loss term that weights the softmax by the distance map.
//   egm_sdf_workspace     bytes of the planes the row pass leaves for the column pass
//   egm_target_sdf_i64    s [N][K][H][W] int32: -min |p - q|^2 over the valid q outside class k for a pixel of class k, +min |p - q|^2
//                         over the q of class k for a valid pixel outside it, 0 for an ignored pixel and for a pixel without such a q
//   egm_bloss_workspace, egm_bloss_fwd, egm_bloss_bwd
//                         L_B = (1/D) sum phi_k(p) softmax(x)[class k], phi made from s on the fly, and its gradient
// The distance transform is two launches whatever the content, N, K and the distances:
//   rows    one wave per row, in chunks of 1024 pixels (mask_scan.h).  A lane reads its 16 int64 labels and leaves the "ask byte" of each
//           pixel (bit k: the pixel is of class k, bit 4 + k: it is valid and not of class k; 0 for an ignored pixel and behind W) and,
//           per bit, a 16-bit plane g = the distance to the nearest pixel of the row with that bit, 0xFFFF = the row has none.  A row of
//           one chunk keeps the marks in registers and runs both scans before its only store; a longer one sweeps left to right, then
//           right to left over what it stored (contour_rows_kernel's scheme).
//   columns a wave owns 256 columns (4 per lane) of kSdfRows rows.  Per class and side (the class pixels ask the plane of bit 4 + k, the
//           valid pixels outside ask the plane of bit k; a side no lane of the wave has is skipped) it walks the rows outwards, two steps
//           on each side per iteration, and keeps best = min(dy^2 + g^2).  Rows t or more away can only give t^2 or more, so the walk
//           ends when t^2 reaches the largest best of the wave, and at the image's first and last row at the latest.
// The flat rule needs no flag: a pixel's minimum is undefined exactly when the set it asks is empty in its image, and then the set of
// pixels that would ask the other plane of (n, k) is empty as well (no class pixel: everything valid asks for one and finds none; no
// valid pixel outside: only class pixels ask, and find none), so "still none -> 0" makes the whole plane 0.
// No workgroup waits for another and no wave waits for another wave; a wave never leaves its image: every row index is clamped into
// [0, H) of image n.  No atomics at all: the loss's partial sums are plain stores, summed in a fixed order in double.
#include "common.h"
#include "mask_scan.h"

namespace {

constexpr int kSdfMaxK = kBoundaryMaxC;        // classes per call: bit k and bit 4 + k of the ask byte
constexpr int kSdfRows = kRowGroup;            // column pass: image rows per wave (tests/test_gpu_boundary_loss.py restates it)
static_assert(kSdfRows % kRowGroup == 0, "a tile is a whole number of row groups");
constexpr int kSdfMaxSide = 32767;             // |s| < 2^31 and a row distance fits 16 bits beside 0xFFFF
constexpr unsigned int kSdfNoRow = Cells<16>::kCap;
constexpr unsigned int kSdfNoDist = 0x7FFFFFFFu;       // g^2 of a row without a marked pixel: above every d2, and + dy^2 fits 32 bits
constexpr int kBlossBlocks = 256;              // workgroups per image of the loss passes = partial sums per image
constexpr int kBlossMaxC = 16;

struct SdfClasses { int id[kSdfMaxK]; };

// ---------------------------------------------------------------- rows
// the ask bytes of a lane's 16 pixels [p0, p0 + 16) of a row of W int64 labels
__device__ __forceinline__ Cells<8> target_bits(const long long* __restrict__ row, int p0, int W, const SdfClasses& cls, int K,
                                                long long ignore_index) {
    long long t[kRowLanePix];
    if (p0 + kRowLanePix <= W) {
#pragma unroll
        for (int i = 0; i < kRowLanePix; i += 2) __builtin_memcpy(&t[i], row + p0 + i, 16);
    } else {
#pragma unroll
        for (int i = 0; i < kRowLanePix; ++i) t[i] = p0 + i < W ? row[p0 + i] : ignore_index;
    }
    Cells<8> bits;
#pragma unroll
    for (int i = 0; i < kRowLanePix; ++i) {
        unsigned int b = 0u;
#pragma unroll
        for (int k = 0; k < kSdfMaxK; ++k)
            if (k < K) b |= (t[i] == (long long)cls.id[k] ? 1u : 16u) << k;
        bits.put(i, (t[i] != ignore_index && p0 + i < W) ? b : 0u);
    }
    return bits;
}

__global__ __launch_bounds__(256) void sdf_rows_kernel(const long long* __restrict__ target, long long nrows, int W, int pitch,
                                                       SdfClasses cls, int K, long long ignore_index, unsigned char* __restrict__ ask,
                                                       unsigned char* __restrict__ g_planes) {
    const int lane = threadIdx.x & 63;
    const long long row = blockIdx.x * 4LL + (threadIdx.x >> 6);
    if (row >= nrows) return;                                  // (a whole wave; the kernel has no barrier)
    const long long* trow = target + row * W;
    unsigned char* krow = ask + row * pitch;
    const long long plane = nrows * pitch * 2;                 // bytes of a 16-bit plane
    unsigned char* grow = g_planes + row * pitch * 2;
    const bool one_chunk = pitch <= kRowChunk;                 // both scans from the marks in registers
    int carry[2 * kSdfMaxK];
#pragma unroll
    for (int t = 0; t < 2 * kSdfMaxK; ++t) carry[t] = kNoMarkLeft;
    for (int base = 0; base < pitch; base += kRowChunk) {      // left to right
        const int p0 = base + lane * kRowLanePix;
        const Cells<8> kbits = target_bits(trow, p0, W, cls, K, ignore_index);
        if (p0 < pitch) kbits.store(krow + p0);
#pragma unroll
        for (int t = 0; t < 2 * kSdfMaxK; ++t) {               // bit t of the ask byte -> plane (t / 4) * K + t % 4
            if ((t & 3) >= K) continue;
            const unsigned int marks = gather_bit(kbits, t);
            Cells<16> g = dist_left<16>(marks, p0, 0, carry[t]);
            if (one_chunk) {
                int none = kNoMarkRight;
                dist_right_min(marks, p0, 0, none, g);
            }
            if (p0 < pitch) g.store(grow + ((t >> 2) * K + (t & 3)) * plane + p0 * 2);
        }
    }
    if (one_chunk) return;
#pragma unroll
    for (int t = 0; t < 2 * kSdfMaxK; ++t) carry[t] = kNoMarkRight;
    for (int base = ((pitch - 1) / kRowChunk) * kRowChunk; base >= 0; base -= kRowChunk) {     // right to left
        const int p0 = base + lane * kRowLanePix;
        Cells<8> kbits;
        if (p0 < pitch) kbits.load(krow + p0);
#pragma unroll
        for (int t = 0; t < 2 * kSdfMaxK; ++t) {
            if ((t & 3) >= K) continue;
            unsigned char* gt = grow + ((t >> 2) * K + (t & 3)) * plane + p0 * 2;
            Cells<16> g;
            if (p0 < pitch) g.load(gt);
            dist_right_min(gather_bit(kbits, t), p0, 0, carry[t], g);
            if (p0 < pitch) g.store(gt);
        }
    }
}

// ---------------------------------------------------------------- columns
// g^2 of a lane's four columns of one row, kSdfNoDist where the row has no marked pixel or `inside` is false (surface.hip's row_squares
// with the row's own guard: the caller clamps the row index and says whether the row exists)
__device__ __forceinline__ void sdf_row_squares(const unsigned short* g, long long at, bool inside, unsigned int (&sq)[kColLanePix]) {
    const uint2 v = *reinterpret_cast<const uint2*>(g + at);
    const unsigned int h[kColLanePix] = {v.x & 0xFFFFu, v.x >> 16, v.y & 0xFFFFu, v.y >> 16};
#pragma unroll
    for (int i = 0; i < kColLanePix; ++i) sq[i] = (h[i] == kSdfNoRow || !inside) ? kSdfNoDist : h[i] * h[i];
}

// rows [y0, y0 + kSdfRows) x columns [x0, x0 + 256) of image n; one wave per item
__global__ __launch_bounds__(256) void sdf_cols_kernel(int H, int W, int pitch, int K, const unsigned char* __restrict__ ask,
                                                       const unsigned short* __restrict__ g_planes, long long plane, int nrc, int ncg,
                                                       long long items, int vec, int* __restrict__ s_out) {
    const long long item = blockIdx.x * 4LL + (threadIdx.x >> 6);
    if (item >= items) return;                                 // (a whole wave; the kernel has no barrier)
    const ColTile tile(item, ncg, nrc, H, pitch, kSdfRows);
    const long long n = tile.n, img = tile.img;
    const int x0 = tile.x0, y0 = tile.y0, yend = tile.yend;
    const bool live = tile.live;
    for (int k = 0; k < K; ++k) {
        for (int y = y0; y < yend; y += kRowGroup) {           // rows y .. y + kRowGroup - 1 share one walk
            unsigned int kb[kRowGroup];
#pragma unroll
            for (int j = 0; j < kRowGroup; ++j)
                kb[j] = (live && y + j < yend) ? *reinterpret_cast<const unsigned int*>(ask + img + (long long)(y + j) * pitch) : 0u;
            int res[kRowGroup][kColLanePix];
#pragma unroll
            for (int j = 0; j < kRowGroup; ++j)
#pragma unroll
                for (int i = 0; i < kColLanePix; ++i) res[j][i] = 0;
#pragma unroll
            for (int s = 0; s < 2; ++s) {                      // 0: the class pixels ask for a valid pixel outside, 1: the other way round
                unsigned int want[kRowGroup], any_want = 0u;
#pragma unroll
                for (int j = 0; j < kRowGroup; ++j) {
                    want[j] = (kb[j] >> (4 * s + k)) & 0x01010101u;
                    any_want |= want[j];
                }
                if (!__any(any_want != 0u)) continue;          // no lane of the wave has such a pixel in these rows
                const unsigned short* g = g_planes + ((1 - s) * K + k) * plane;
                unsigned int best[kRowGroup][kColLanePix];     // 0 where nobody asks: it never holds the walk up
#pragma unroll
                for (int j = 0; j < kRowGroup; ++j)
#pragma unroll
                    for (int i = 0; i < kColLanePix; ++i) best[j][i] = ((want[j] >> (8 * i)) & 1u) ? 0xFFFFFFFFu : 0u;
#pragma unroll
                for (int jj = 0; jj < kRowGroup; ++jj) {       // the group's own rows: dy = |j - jj|
                    unsigned int sq[kColLanePix];
                    sdf_row_squares(g, img + (long long)min(y + jj, H - 1) * pitch, y + jj < H, sq);
#pragma unroll
                    for (int j = 0; j < kRowGroup; ++j)
#pragma unroll
                        for (int i = 0; i < kColLanePix; ++i) best[j][i] = min(best[j][i], sq[i] + (unsigned int)((j - jj) * (j - jj)));
                }
                // rows y - t, y - t - 1 above and y + kRowGroup - 1 + t, + t + 1 below per iteration: four loads in flight; the second
                // row of a side is a candidate like any other, so taking it before its own bound is checked leaves the minimum exact
                for (int t = 1; t < H; t += 2) {
                    unsigned int lmax = 0u;
#pragma unroll
                    for (int j = 0; j < kRowGroup; ++j)
#pragma unroll
                        for (int i = 0; i < kColLanePix; ++i) lmax = max(lmax, best[j][i]);
                    const int ya = y - t, yb = y + kRowGroup - 1 + t;
                    if (!__any((unsigned int)(t * t) < lmax) || (ya < 0 && yb >= H)) break;     // nothing nearer is left, or no row is
                    unsigned int sq[4][kColLanePix];
                    const int r[4] = {ya, ya - 1, yb, yb + 1};
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        sdf_row_squares(g, img + (long long)clampi(r[q], 0, H - 1) * pitch, r[q] >= 0 && r[q] < H, sq[q]);
#pragma unroll
                    for (int j = 0; j < kRowGroup; ++j) {
                        const int dy[4] = {t + j, t + 1 + j, t + kRowGroup - 1 - j, t + kRowGroup - j};
#pragma unroll
                        for (int q = 0; q < 4; ++q)
#pragma unroll
                            for (int i = 0; i < kColLanePix; ++i) best[j][i] = min(best[j][i], sq[q][i] + (unsigned int)(dy[q] * dy[q]));
                    }
                }
#pragma unroll
                for (int j = 0; j < kRowGroup; ++j)
#pragma unroll
                    for (int i = 0; i < kColLanePix; ++i) {
                        const unsigned int d2 = best[j][i];
                        if (((want[j] >> (8 * i)) & 1u) && d2 < kSdfNoDist) res[j][i] = s ? (int)d2 : -(int)d2;
                    }
            }
            if (!live) continue;
#pragma unroll
            for (int j = 0; j < kRowGroup; ++j) {              // every pixel of the tile is written, 0 where nothing is defined
                if (y + j >= yend) break;
                int* row = s_out + ((n * K + k) * H + y + j) * W + x0;
                if (vec && x0 + kColLanePix <= W) {
                    *reinterpret_cast<int4*>(row) = make_int4(res[j][0], res[j][1], res[j][2], res[j][3]);
                } else {
#pragma unroll
                    for (int i = 0; i < kColLanePix; ++i)
                        if (x0 + i < W) row[i] = res[j][i];
                }
            }
        }
    }
}

// ---------------------------------------------------------------- the loss term
// phi of the official one_hot2dist from the signed squared distance: sqrt(s) outside, -(sqrt(-s) - 1) inside, 0 where s is 0; the
// correctly rounded fp32 root of the int -> float conversion, which numpy's float32 restates bit for bit.  sqrtf, not __fsqrt_rn: the
// intrinsic compiles to a bare v_sqrt_f32 (1 ulp) here, sqrtf to v_sqrt_f32 plus the one-ulp correction by fma residuals
__device__ __forceinline__ float sdf_phi(int s) {
    const float r = sqrtf((float)abs(s));
    return s > 0 ? r : (s < 0 ? -(r - 1.f) : 0.f);
}

// phi as a tensor, for inspection and tests (the loss passes never store it)
__global__ __launch_bounds__(256) void sdf_phi_kernel(const int* __restrict__ s, long long n, float* __restrict__ phi) {
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256) phi[i] = sdf_phi(s[i]);
}

// V consecutive values of T from p (V = 4: one 16-byte load; the launcher has checked the alignment)
template <int V, typename T>
__device__ __forceinline__ void load_run(const T* __restrict__ p, T (&v)[V]) {
    static_assert(V == 1 || (V == 4 && sizeof(T) == 4), "one value, or four of four bytes");
    if constexpr (V == 1) v[0] = p[0];
    else __builtin_memcpy(v, __builtin_assume_aligned(p, 16), 16);
}

// softmax over the C channels of V pixels and phi of their K planes -> pk[k][v] = the probability of class k, ph[k][v] = phi_k;
// e[c][v] = the probabilities of all channels
template <int CB, int V>
__device__ __forceinline__ void bloss_pixel(const float* __restrict__ lg, const int* __restrict__ sd, long long HW, long long p, int C,
                                            const SdfClasses& cls, int K, float (&e)[CB][V], float (&pk)[kSdfMaxK][V],
                                            float (&ph)[kSdfMaxK][V]) {
    float mx[V], se[V];
#pragma unroll
    for (int v = 0; v < V; ++v) { mx[v] = -INFINITY; se[v] = 0.f; }
#pragma unroll
    for (int c = 0; c < CB; ++c)
        if (c < C) {
            load_run<V>(lg + c * HW + p, e[c]);
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
#pragma unroll
    for (int k = 0; k < kSdfMaxK; ++k) {
        int sv[V];
        if (k < K) {
            load_run<V>(sd + k * HW + p, sv);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                ph[k][v] = sdf_phi(sv[v]);
                float q = 0.f;
#pragma unroll
                for (int c = 0; c < CB; ++c) q = (c < C && c == cls.id[k]) ? e[c][v] : q;
                pk[k][v] = q;
            }
        } else {
#pragma unroll
            for (int v = 0; v < V; ++v) { ph[k][v] = 0.f; pk[k][v] = 0.f; }
        }
    }
}

// psum[n][b] = this workgroup's sum of phi_k p_k, pcnt[n][b] = its count of valid pixels; plain stores
template <int CB, int V>
__global__ __launch_bounds__(256) void bloss_fwd_kernel(const float* __restrict__ logits, const int* __restrict__ sdf,
                                                        const long long* __restrict__ target, SdfClasses cls, int K, int C, long long HW,
                                                        long long ignore_index, float* __restrict__ psum, unsigned int* __restrict__ pcnt) {
    __shared__ float red_s[4];
    __shared__ unsigned int red_c[4];
    const int n = blockIdx.y;
    const float* lg = logits + (long long)n * C * HW;
    const int* sd = sdf + (long long)n * K * HW;
    const long long* tg = target + (long long)n * HW;
    float acc = 0.f;
    unsigned int cnt = 0u;
    for (long long p = (blockIdx.x * 256LL + threadIdx.x) * V; p < HW; p += (long long)gridDim.x * 256 * V) {
        float e[CB][V], pk[kSdfMaxK][V], ph[kSdfMaxK][V];
        bloss_pixel<CB, V>(lg, sd, HW, p, C, cls, K, e, pk, ph);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            cnt += tg[p + v] != ignore_index ? 1u : 0u;
#pragma unroll
            for (int k = 0; k < kSdfMaxK; ++k) acc += ph[k][v] * pk[k][v];     // (phi is 0 at an ignored pixel and beyond K)
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

// one workgroup: the partial sums in a fixed order in double, the count in integers -> out = {w L_B, L_B}, inv_d[0] = 1 / D.  1024
// threads, so that a batch of 8 images is two loads per thread: one wave walking 2048 partials paid 32 dependent round trips
__global__ __launch_bounds__(1024) void bloss_finalize_kernel(const float* __restrict__ psum, const unsigned int* __restrict__ pcnt,
                                                              int nparts, int K, const float* __restrict__ w_dev,
                                                              float* __restrict__ inv_d, float* __restrict__ out) {
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
        const double d = (double)K * (double)(c > 0ull ? c : 1ull);
        const float lb = (float)(s / d);
        inv_d[0] = (float)(1.0 / d);
        out[0] = w_dev[0] * lb;
        out[1] = lb;
    }
}

// dlogits[j] = go w / D * p_j * ([j in classes] phi_j - sum_k phi_k p_k); 0 at an ignored pixel because every phi is 0 there
template <int CB, int V>
__global__ __launch_bounds__(256) void bloss_bwd_kernel(const float* __restrict__ logits, const int* __restrict__ sdf, SdfClasses cls, int K,
                                                        int C, long long HW, const float* __restrict__ inv_d,
                                                        const float* __restrict__ gout, const float* __restrict__ w_dev,
                                                        float* __restrict__ dlogits) {
    const int n = blockIdx.y;
    const float* lg = logits + (long long)n * C * HW;
    const int* sd = sdf + (long long)n * K * HW;
    float* dl = dlogits + (long long)n * C * HW;
    const float scale = (gout ? gout[0] : 1.f) * w_dev[0] * inv_d[0];
    for (long long p = (blockIdx.x * 256LL + threadIdx.x) * V; p < HW; p += (long long)gridDim.x * 256 * V) {
        float e[CB][V], pk[kSdfMaxK][V], ph[kSdfMaxK][V], dot[V];
        bloss_pixel<CB, V>(lg, sd, HW, p, C, cls, K, e, pk, ph);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            dot[v] = 0.f;
#pragma unroll
            for (int k = 0; k < kSdfMaxK; ++k) dot[v] += ph[k][v] * pk[k][v];
        }
#pragma unroll
        for (int c = 0; c < CB; ++c)
            if (c < C) {
                float g[V];
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    float own = 0.f;
#pragma unroll
                    for (int k = 0; k < kSdfMaxK; ++k) own = (k < K && c == cls.id[k]) ? ph[k][v] : own;
                    g[v] = scale * (e[c][v] * (own - dot[v]));
                }
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
// K, the class ids among themselves and (C > 0) against the channel count; -> EGM_OK or EGM_ERR_ARG with the message set
inline int sdf_classes_check(const char* name, const int* classes, int K, int C, SdfClasses& cls) {
    EGM_REQUIRE(K >= 1 && K <= kSdfMaxK, "%s: %d classes, between 1 and %d are supported", name, K, kSdfMaxK);
    EGM_REQUIRE(classes, "%s: null pointer (classes)", name);
    for (int k = 0; k < kSdfMaxK; ++k) cls.id[k] = -1;
    for (int k = 0; k < K; ++k) {
        EGM_REQUIRE(classes[k] >= 0 && (C <= 0 || classes[k] < C), "%s: class id %d outside [0, %d)", name, classes[k], C > 0 ? C : 0x7FFFFFFF);
        for (int j = 0; j < k; ++j) EGM_REQUIRE(classes[j] != classes[k], "%s: class id %d is repeated", name, classes[k]);
        cls.id[k] = classes[k];
    }
    return EGM_OK;
}
inline int sdf_side_check(const char* name, int H, int W) {
    EGM_REQUIRE(H <= kSdfMaxSide && W <= kSdfMaxSide, "%s: %d x %d pixels, at most %d rows and columns are supported", name, H, W, kSdfMaxSide);
    return EGM_OK;
}
inline int bloss_shape_check(const char* name, int N, int C, int H, int W) {
    EGM_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C <= kBlossMaxC, "%s: bad shape %d x %d x %d x %d (at most %d channels)", name, N, C, H, W,
                kBlossMaxC);
    EGM_REQUIRE(N <= 65535, "%s: %d images in one call, at most 65535 are supported", name, N);
    return EGM_OK;
}
// four pixels per lane where every channel plane of every image starts at a 16-byte boundary
inline bool bloss_vec4(long long HW, const void* a, const void* b, const void* c) {
    return HW % 4 == 0 && egm_aligned16(a) && egm_aligned16(b) && (!c || egm_aligned16(c));
}

}  // namespace

extern "C" long long egm_sdf_workspace(int N, int H, int W, int K) {
    EGM_REQUIRE(K >= 1 && K <= kSdfMaxK, "sdf_workspace: %d classes, between 1 and %d are supported", K, kSdfMaxK);
    if (mask_shape_check("sdf_workspace", N, H, W, K) != EGM_OK || sdf_side_check("sdf_workspace", H, W) != EGM_OK) return EGM_ERR_ARG;
    return (long long)(1 + 4 * K) * N * H * boundary_pitch(W) + 16;            // (+16: the planes start at the first 16-byte boundary)
}

extern "C" int egm_target_sdf_i64(const long long* target, int N, int H, int W, const int* classes, int K, long long ignore_index,
                                  void* workspace, int* s_out, egm_stream_t s) {
    const char* name = "target_sdf_i64";
    SdfClasses cls;
    if (sdf_classes_check(name, classes, K, 0, cls) != EGM_OK) return EGM_ERR_ARG;
    EGM_REQUIRE(target && workspace && s_out, "%s: null pointer", name);
    if (mask_shape_check(name, N, H, W, K) != EGM_OK || sdf_side_check(name, H, W) != EGM_OK) return EGM_ERR_ARG;
    const long long nrows = (long long)N * H;
    const int pitch = boundary_pitch(W), nrc = egm_cdiv(H, kSdfRows), ncg = egm_cdiv(W, kColWave);
    const long long items = (long long)N * nrc * ncg, plane = nrows * pitch;
    EGM_REQUIRE(nrows <= (1ll << 31) && items <= (1ll << 32), "%s: %d images of %d x %d in one call are too many", name, N, H, W);
    unsigned char* ask = mask_align(workspace);
    unsigned char* g_planes = ask + plane;                     // (plane is a multiple of 16 bytes)
    hipLaunchKernelGGL(sdf_rows_kernel, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, (hipStream_t)s, target, nrows, W, pitch, cls, K,
                       ignore_index, ask, g_planes);
    EGM_CHECK_LAUNCH("target_sdf_i64 (rows)");
    hipLaunchKernelGGL(sdf_cols_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, (hipStream_t)s, H, W, pitch, K, ask,
                       reinterpret_cast<const unsigned short*>(g_planes), plane, nrc, ncg, items, (W % 4 == 0 && egm_aligned16(s_out)) ? 1 : 0,
                       s_out);
    EGM_CHECK_LAUNCH("target_sdf_i64 (columns)");
    return EGM_OK;
}

extern "C" int egm_sdf_phi_f32(const int* sdf, long long n, float* phi, egm_stream_t s) {
    EGM_REQUIRE(sdf && phi && n > 0, "sdf_phi_f32: null pointer or no element");
    hipLaunchKernelGGL(sdf_phi_kernel, dim3(egm_stream_grid(n)), dim3(256), 0, (hipStream_t)s, sdf, n, phi);
    EGM_CHECK_LAUNCH("sdf_phi_f32");
    return EGM_OK;
}

extern "C" long long egm_bloss_workspace(int N, int C, int H, int W) {
    if (bloss_shape_check("bloss_workspace", N, C, H, W) != EGM_OK) return EGM_ERR_ARG;
    return ((long long)2 * N * kBlossBlocks + 4) * 4;          // partial sums, counts, 1 / D
}

#define EGM_BLOSS_LAUNCH(kernel, ...)                                                                                             \
    do {                                                                                                                          \
        const dim3 grid_(kBlossBlocks, N), block_(256);                                                                           \
        if (vec4) {                                                                                                               \
            if (C <= 2) hipLaunchKernelGGL((kernel<2, 4>), grid_, block_, 0, (hipStream_t)s, __VA_ARGS__);                        \
            else if (C <= 4) hipLaunchKernelGGL((kernel<4, 4>), grid_, block_, 0, (hipStream_t)s, __VA_ARGS__);                   \
            else hipLaunchKernelGGL((kernel<kBlossMaxC, 4>), grid_, block_, 0, (hipStream_t)s, __VA_ARGS__);                      \
        } else {                                                                                                                  \
            if (C <= 2) hipLaunchKernelGGL((kernel<2, 1>), grid_, block_, 0, (hipStream_t)s, __VA_ARGS__);                        \
            else if (C <= 4) hipLaunchKernelGGL((kernel<4, 1>), grid_, block_, 0, (hipStream_t)s, __VA_ARGS__);                   \
            else hipLaunchKernelGGL((kernel<kBlossMaxC, 1>), grid_, block_, 0, (hipStream_t)s, __VA_ARGS__);                      \
        }                                                                                                                         \
    } while (0)

extern "C" int egm_bloss_fwd(const float* logits, const int* sdf, const long long* target, const int* classes, int K, int N, int C, int H,
                             int W, long long ignore_index, const float* w_dev, void* workspace, float* out2, egm_stream_t s) {
    const char* name = "bloss_fwd";
    SdfClasses cls;
    if (bloss_shape_check(name, N, C, H, W) != EGM_OK || sdf_classes_check(name, classes, K, C, cls) != EGM_OK) return EGM_ERR_ARG;
    EGM_REQUIRE(logits && sdf && target && w_dev && workspace && out2, "%s: null pointer", name);
    EGM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "%s: the workspace must be 4-byte aligned", name);
    const long long HW = (long long)H * W;
    float* psum = reinterpret_cast<float*>(workspace);
    unsigned int* pcnt = reinterpret_cast<unsigned int*>(psum + (long long)N * kBlossBlocks);
    float* inv_d = psum + (long long)2 * N * kBlossBlocks;
    const bool vec4 = bloss_vec4(HW, logits, sdf, nullptr);
    EGM_BLOSS_LAUNCH(bloss_fwd_kernel, logits, sdf, target, cls, K, C, HW, ignore_index, psum, pcnt);
    EGM_CHECK_LAUNCH("bloss_fwd");
    hipLaunchKernelGGL(bloss_finalize_kernel, dim3(1), dim3(1024), 0, (hipStream_t)s, psum, pcnt, N * kBlossBlocks, K, w_dev, inv_d, out2);
    EGM_CHECK_LAUNCH("bloss_fwd (finalize)");
    return EGM_OK;
}

extern "C" int egm_bloss_bwd(const float* logits, const int* sdf, const int* classes, int K, int N, int C, int H, int W,
                             const void* workspace, const float* grad_out, const float* w_dev, float* dlogits, egm_stream_t s) {
    const char* name = "bloss_bwd";
    SdfClasses cls;
    if (bloss_shape_check(name, N, C, H, W) != EGM_OK || sdf_classes_check(name, classes, K, C, cls) != EGM_OK) return EGM_ERR_ARG;
    EGM_REQUIRE(logits && sdf && w_dev && workspace && dlogits, "%s: null pointer", name);
    const long long HW = (long long)H * W;
    const float* inv_d = reinterpret_cast<const float*>(workspace) + (long long)2 * N * kBlossBlocks;
    const bool vec4 = bloss_vec4(HW, logits, sdf, dlogits);
    EGM_BLOSS_LAUNCH(bloss_bwd_kernel, logits, sdf, cls, K, C, HW, inv_d, grad_out, w_dev, dlogits);
    EGM_CHECK_LAUNCH("bloss_bwd");
    return EGM_OK;
}
#undef EGM_BLOSS_LAUNCH
