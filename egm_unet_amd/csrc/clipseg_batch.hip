// The training batch of the CLIPSeg decoder on the device (egm_unet_amd/clipseg_data.py): B ragged uint8 photos
// [H_b][W_b][3] with their masks [H_b][W_b] -> the object-aware square crop, the bilinear align_corners=True resize to S x S with the
// nearest resize of the mask, / 255, ColorJitter, Normalize -> fp32 [B][3][S][S] and fp32 [B][1][S][S].  Everything that differs between
// the images sits in one device table of egm_clipseg_batch_desc rows followed by int32 / fp32 tables (include/egm_hip.h); blockIdx.y
// (blockIdx.x in the choice) is the image, so the launch count does not depend on B:
//   egm_mask_profile_u8   per image the counts of nonzero mask bytes per line of the slide axis (per column when W > H, else per row)
//   egm_clipseg_choose    a prefix sum over the counts, the window sum of every candidate offset, the first one over the threshold or
//                         the earliest largest one -> choice [B][3] = (off_y, off_x, exceed)
//   egm_clipseg_batch_u8  reads the choice on the device, gathers the four taps of every output pixel inside the window, applies the
//                         jitter operations in front of the contrast and writes one double partial of the gray sum per tile; without
//                         a jitter it writes the finished, normalised batch
//   egm_color_jitter_f32  the contrast mean from the partials, the remaining operations and Normalize, in place
// Nothing waits for the device, for another workgroup or for a flag; no atomics; stream order is the only synchronisation.
// The arithmetic of a sample is fixed, one fp32 rounding per operation, so that a numpy float32 restatement gives the same bits
// (tests/clipseg_batch_oracle.py):
//   resize      l0 = 1 - l1;  top = lx0 * a + lx1 * b;  bot = lx0 * c + lx1 * d;  v = (ly0 * top + ly1 * bot) / 255
//   gray        g = (0.2989 R + 0.587 G) + 0.114 B
//   brightness  clamp(r x);  saturation  clamp(r x + q g);  contrast  clamp(r x + q mean);  hue  rgb -> hsv, h = (h + f) mod 1, hsv -> rgb
//   mean        a tile is 1024 consecutive pixels of the plane, 4 per lane: ((g0 + g1) + g2) + g3 in double, the xor butterfly 32 .. 1
//               over the wave, ((w0 + w1) + w2) + w3 over the waves; the tiles in ascending order; / (H W) in double, rounded once
//   normalize   (x - mean_c) / std_c
//   shape   a lane owns 4 consecutive pixels of a plane (one row where S is a multiple of 4), a workgroup a tile of 1024.  The resample
//           is a gather: one dword at the byte address of each of the four tap pixels, served by L1 / L2 (the window of a photo is read about
//           once); the fp32
//           planes leave as 16-byte non-temporal stores where the plane is a multiple of 4 pixels and the base is aligned, else as dwords.
//           The mask is read as dwords at byte addresses (columns 4 lane .. 4 lane + 3 of a row), per byte at a row's ragged end.
// The device-chosen offset is clamped into [0, long - m], every tap and nearest index into its window and the window into the photo, a
// candidate offset into [0, long - m] and a jitter operation id is read & 3: a wrong row gives wrong pixels, never a read outside the
// buffers it names.
#include <limits.h>
#include <math.h>
#include "common.h"

static_assert(sizeof(egm_clipseg_batch_desc) == 80, "egm_clipseg_batch_desc is packed by the host (egm_unet_amd/clipseg_data.py: CLIPSEG_DESC)");

// No multiply of this file may be fused with the add behind it (as csrc/tta.hip): the sample arithmetic below is written with plain
// operators, which this pragma governs; common.h holds none of it.
#pragma clang fp contract(off)

namespace {

constexpr int kLanePix = 4;
constexpr int kTilePix = 256 * kLanePix;
constexpr int kMaxSide = 32767;

struct Norm { float m[3], s[3]; int on; };

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

__device__ __forceinline__ float gray_of(const float (&p)[3]) {
    const float a = 0.2989f * p[0], b = 0.587f * p[1], c = 0.114f * p[2];
    const float ab = a + b;
    return ab + c;
}

// x - trunc(x) is fmod(x, 1) exactly (the fraction of a float is a float)
__device__ __forceinline__ float fmod1(float x) { return x - truncf(x); }

__device__ __forceinline__ void hue_op(float f, float (&p)[3]) {
    const float r = p[0], g = p[1], b = p[2];
    const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
    const bool eqc = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eqc ? 1.f : maxc);
    const float dv = eqc ? 1.f : cr;
    const float rc = (maxc - r) / dv, gc = (maxc - g) / dv, bc = (maxc - b) / dv;
    float h;
    if (maxc == r) h = bc - gc;
    else if (maxc == g) { const float t = 2.f + rc; h = t - bc; }
    else { const float t = 4.f + gc; h = t - rc; }
    h = h / 6.f;
    h = h + 1.f;
    h = fmod1(h);
    h = h + f;
    float m = fmod1(h);                                   // remainder(h, 1): fmod, then + 1 where it is negative
    if (m < 0.f) m = m + 1.f;
    const float h6 = m * 6.f;
    const float fl = floorf(h6);
    const float ff = h6 - fl;
    const int i = (int)fl % 6;
    const float v = maxc;
    const float one_s = 1.f - s, sf = s * ff, one_f = 1.f - ff;
    const float one_sf = 1.f - sf, s1f = s * one_f;
    const float one_s1f = 1.f - s1f;
    const float pp = clamp01(v * one_s), qq = clamp01(v * one_sf), tt = clamp01(v * one_s1f);
    //            i:  0   1   2   3   4   5
    // R              v   q   p   p   t   v
    // G              t   v   v   q   p   p
    // B              p   p   t   v   v   q
    p[0] = (i == 0 || i == 5) ? v : (i == 1 ? qq : (i == 4 ? tt : pp));
    p[1] = (i == 1 || i == 2) ? v : (i == 0 ? tt : (i == 3 ? qq : pp));
    p[2] = (i == 3 || i == 4) ? v : (i == 2 ? tt : (i == 5 ? qq : pp));
}

// one jitter operation on one pixel: 0 brightness, 1 contrast, 2 saturation, 3 hue; fac = r[0..3], q[0..3] of the image
__device__ __forceinline__ void jitter_op(int op, const float* __restrict__ fac, float mean, float (&p)[3]) {
    const float r = fac[op], q = fac[4 + op];
    if (op == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = clamp01(r * p[c]);
    } else if (op == 3) {
        hue_op(r, p);
    } else {
        const float other = op == 1 ? mean : gray_of(p);
        const float qo = q * other;
#pragma unroll
        for (int c = 0; c < 3; ++c) { const float rx = r * p[c]; p[c] = clamp01(rx + qo); }
    }
}

// index of the contrast in the image's order (4: the order holds none, every operation runs in front)
__device__ __forceinline__ int contrast_at(const int* __restrict__ ord) {
    int k = 4;
#pragma unroll
    for (int j = 3; j >= 0; --j) if ((ord[j] & 3) == 1) k = j;
    return k;
}

// the tile's double partial of its lanes' gray values; `red` = 4 doubles of LDS; every thread of the workgroup calls it
__device__ __forceinline__ void tile_partial(const float (&g)[kLanePix], double* red, double* __restrict__ dst) {
    double s = (double)g[0];
    s = s + (double)g[1]; s = s + (double)g[2]; s = s + (double)g[3];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = red[0] + red[1];
        t = t + red[2]; t = t + red[3];
        *dst = t;
    }
}

// 4 consecutive floats of a plane at pixel p0 (n valid): one 16-byte non-temporal store where vec, else dwords
__device__ __forceinline__ void store_run(float* __restrict__ q, const float (&v)[kLanePix], int n, int vec) {
    if (vec && n == kLanePix) {
        egm_u32x4 a;
        a.x = __float_as_uint(v[0]); a.y = __float_as_uint(v[1]); a.z = __float_as_uint(v[2]); a.w = __float_as_uint(v[3]);
        egm_store16_as<EGM_STORE_MODE>(q, a);
    } else {
        for (int k = 0; k < n; ++k) q[k] = v[k];
    }
}

__device__ __forceinline__ float normalize(float x, const Norm& nm, int c) {
    if (!nm.on) return x;
    const float d = x - nm.m[c];
    return d / nm.s[c];
}

// ---- line counts ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned load_mask4(const unsigned char* __restrict__ p, int n) {     // n = bytes left in the row, >= 1
    unsigned v = 0u;
    if (n >= 4) __builtin_memcpy(&v, p, 4);
    else for (int k = 0; k < n; ++k) v |= (unsigned)p[k] << (8 * k);
    return v;
}

__global__ __launch_bounds__(256) void cs_profile_kernel(const egm_clipseg_batch_desc* __restrict__ tab, int* __restrict__ profile) {
    __shared__ unsigned red[4][256];
    const egm_clipseg_batch_desc d = tab[blockIdx.y];
    if (d.axis < 0) return;
    const unsigned char* mask = static_cast<const unsigned char*>(d.mask);
    int* prof = profile + d.prof_off;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, H = d.H, W = d.W;
    if (d.axis == 1) {                                                          // columns: a workgroup owns 256 of them, a wave every 4th row
        const int units = (W + 255) >> 8;
        for (int u = blockIdx.x; u < units; u += gridDim.x) {
            const int c = u * 256 + lane * 4;
            unsigned n0 = 0, n1 = 0, n2 = 0, n3 = 0;
            if (c < W) {
#pragma unroll 4
                for (int y = wave; y < H; y += 4) {
                    const unsigned v = load_mask4(mask + (long long)y * W + c, W - c);
                    n0 += (v & 0xffu) != 0u; n1 += (v & 0xff00u) != 0u; n2 += (v & 0xff0000u) != 0u; n3 += (v & 0xff000000u) != 0u;
                }
            }
            red[wave][lane * 4] = n0; red[wave][lane * 4 + 1] = n1; red[wave][lane * 4 + 2] = n2; red[wave][lane * 4 + 3] = n3;
            __syncthreads();
            const int col = u * 256 + threadIdx.x;
            if (col < W) prof[col] = (int)(red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
            __syncthreads();
        }
    } else {                                                                    // rows: a wave per row
        const int units = (H + 3) >> 2;
        for (int u = blockIdx.x; u < units; u += gridDim.x) {
            const int y = u * 4 + wave;
            if (y >= H) continue;                                               // (a whole wave; this branch has no barrier)
            unsigned n = 0;
            for (int c = lane * 4; c < W; c += 256) {
                const unsigned v = load_mask4(mask + (long long)y * W + c, W - c);
                n += ((v & 0xffu) != 0u) + ((v & 0xff00u) != 0u) + ((v & 0xff0000u) != 0u) + ((v & 0xff000000u) != 0u);
            }
            n = wave_sum_u32(n);
            if (lane == 0) prof[y] = (int)n;
        }
    }
}

// ---- choice --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cs_choose_kernel(const egm_clipseg_batch_desc* __restrict__ tab, int* __restrict__ profile,
                                                        int* __restrict__ choice) {
    __shared__ int s_a[256], s_b[256], s_c[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const egm_clipseg_batch_desc d = tab[b];
    if (d.axis < 0 || d.ncand <= 0) {
        if (tid < 3) choice[b * 3 + tid] = 0;
        return;
    }
    const int L = d.axis == 1 ? d.W : d.H;
    const int m = clampi(d.axis == 1 ? d.win_w : d.win_h, 1, L);
    const int* counts = profile + d.prof_off;
    int* prefix = profile + d.prof_off + L;                                     // [L + 1]
    const int per = (L + 255) >> 8;
    const int lo = min(tid * per, L), hi = min(lo + per, L);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += counts[i];
    s_a[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) { const int v = s_a[t]; s_a[t] = run; run += v; }
    }
    __syncthreads();
    int run = s_a[tid];
    for (int i = lo; i < hi; ++i) { prefix[i] = run; run += counts[i]; }
    if (tid == 255) prefix[L] = run;                                            // thread 255's run ends at L: the total
    __threadfence_block();
    __syncthreads();
    const int* cand = reinterpret_cast<const int*>(tab) + d.cand_off;
    int first = INT_MAX, best = -1, best_i = INT_MAX;
    for (int c = tid; c < d.ncand; c += 256) {                                  // ascending per thread: strictly greater keeps the earliest
        const int o = clampi(cand[c], 0, L - m);
        const int sum = prefix[o + m] - prefix[o];
        if (sum > d.thresh && first == INT_MAX) first = c;
        if (sum > best) { best = sum; best_i = c; }
    }
    s_a[tid] = first; s_b[tid] = best; s_c[tid] = best_i;
    __syncthreads();
    if (tid == 0) {
        for (int t = 1; t < 256; ++t) {
            first = min(first, s_a[t]);
            if (s_b[t] > best || (s_b[t] == best && s_c[t] < best_i)) { best = s_b[t]; best_i = s_c[t]; }
        }
        const int exceed = first == INT_MAX;
        const int idx = exceed ? best_i : first;
        const int o = clampi(cand[clampi(idx, 0, d.ncand - 1)], 0, L - m);
        choice[b * 3] = d.axis == 0 ? o : 0;
        choice[b * 3 + 1] = d.axis == 1 ? o : 0;
        choice[b * 3 + 2] = exceed;
    }
}

// ---- resample (+ the jitter in front of the contrast, + the gray partials) --------------------------------------------------------------
// the three bytes of pixel `pix` of an [H][W][3] photo in bits 0 .. 23: one dword at the pixel's byte address (its fourth byte belongs
// to the next pixel and is not looked at); per byte at the photo's last pixel, where that dword would end outside the buffer
__device__ __forceinline__ unsigned load_rgb(const unsigned char* __restrict__ img, int pix, int last_pix) {
    const unsigned char* p = img + (long long)pix * 3;
    unsigned v;
    if (pix < last_pix) __builtin_memcpy(&v, p, 4);
    else v = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
    return v;
}

template <bool JIT>
__global__ __launch_bounds__(256) void cs_resample_kernel(const egm_clipseg_batch_desc* __restrict__ tab, int S, const int* __restrict__ choice,
                                                          const int* __restrict__ order, const float* __restrict__ factors,
                                                          float* __restrict__ out_img, float* __restrict__ out_seg,
                                                          double* __restrict__ partials, Norm nm, int vec) {
    __shared__ double red[4];
    const int b = blockIdx.y, tile = blockIdx.x, tiles = gridDim.x;
    const egm_clipseg_batch_desc d = tab[b];
    const int* tb = reinterpret_cast<const int*>(tab);
    const float* tf = reinterpret_cast<const float*>(tab);
    const int* yi = tb + d.yi_off; const float* yl = tf + d.yl_off;
    const int* xi = tb + d.xi_off; const float* xl = tf + d.xl_off;
    const int* ynn = tb + d.ynn_off; const int* xnn = tb + d.xnn_off;
    const unsigned char* img = static_cast<const unsigned char*>(d.img);
    const unsigned char* mask = static_cast<const unsigned char*>(d.mask);
    const int H = d.H, W = d.W, wh = clampi(d.win_h, 1, H), ww = clampi(d.win_w, 1, W);
    int oy = 0, ox = 0;
    if (d.axis == 0) oy = clampi(choice[b * 3], 0, H - wh);
    if (d.axis == 1) ox = clampi(choice[b * 3 + 1], 0, W - ww);
    const int plane = S * S, last_pix = H * W - 1;
    const int p0 = (tile * 256 + (int)threadIdx.x) * kLanePix;
    const int n = clampi(plane - p0, 0, kLanePix);
    int ord[4] = {0, 0, 0, 0}, kc = 0;
    const float* fac = factors;
    if (JIT) {
#pragma unroll
        for (int j = 0; j < 4; ++j) ord[j] = order[b * 4 + j] & 3;
        kc = contrast_at(ord);
        fac = factors + b * 8;
    }
    float v[3][kLanePix], sg[kLanePix], g[kLanePix];
#pragma unroll
    for (int k = 0; k < kLanePix; ++k) {
        v[0][k] = v[1][k] = v[2][k] = 0.f; sg[k] = 0.f; g[k] = 0.f;
        if (k < n) {
            const int p = p0 + k, y = p / S, x = p - y * S;
            const int y0 = oy + clampi(yi[2 * y], 0, wh - 1), y1 = oy + clampi(yi[2 * y + 1], 0, wh - 1);
            const int x0 = ox + clampi(xi[2 * x], 0, ww - 1), x1 = ox + clampi(xi[2 * x + 1], 0, ww - 1);
            const float ly1 = yl[y], lx1 = xl[x];
            const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
            const unsigned ua = load_rgb(img, y0 * W + x0, last_pix), ub = load_rgb(img, y0 * W + x1, last_pix);
            const unsigned uc = load_rgb(img, y1 * W + x0, last_pix), ud = load_rgb(img, y1 * W + x1, last_pix);
            float px[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float a = (float)((ua >> (8 * c)) & 255u), bb = (float)((ub >> (8 * c)) & 255u);
                const float cc = (float)((uc >> (8 * c)) & 255u), dd = (float)((ud >> (8 * c)) & 255u);
                const float ta = lx0 * a, tbb = lx1 * bb, tc = lx0 * cc, td = lx1 * dd;
                const float top = ta + tbb, bot = tc + td;
                const float vt = ly0 * top, vb = ly1 * bot;
                const float s = vt + vb;
                px[c] = s / 255.0f;
            }
            const int my = oy + clampi(ynn[y], 0, wh - 1), mx = ox + clampi(xnn[x], 0, ww - 1);
            sg[k] = (!d.negative && mask[(long long)my * W + mx] != 0) ? 1.f : 0.f;
            if (JIT) {
                for (int j = 0; j < kc; ++j) jitter_op(ord[j], fac, 0.f, px);
                g[k] = gray_of(px);
                v[0][k] = px[0]; v[1][k] = px[1]; v[2][k] = px[2];
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][k] = normalize(px[c], nm, c);
            }
        }
    }
    if (n > 0) {
        float* oi = out_img + (long long)b * 3 * plane + p0;
        store_run(oi, v[0], n, vec); store_run(oi + plane, v[1], n, vec); store_run(oi + 2ll * plane, v[2], n, vec);
        store_run(out_seg + (long long)b * plane + p0, sg, n, vec);
    }
    if (JIT) tile_partial(g, red, partials + (long long)b * tiles + tile);
}

// ---- the jitter on an fp32 batch: the operations in front of the contrast out of place, the rest in place -------------------------------
__global__ __launch_bounds__(256) void cs_jitter_pre_kernel(const float* x, float* out, int plane,
                                                            const int* __restrict__ order, const float* __restrict__ factors,
                                                            double* __restrict__ partials, int vec) {
    __shared__ double red[4];
    const int b = blockIdx.y, tile = blockIdx.x, tiles = gridDim.x;
    const int p0 = (tile * 256 + (int)threadIdx.x) * kLanePix;
    const int n = clampi(plane - p0, 0, kLanePix);
    int ord[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ord[j] = order[b * 4 + j] & 3;
    const int kc = contrast_at(ord);
    const float* fac = factors + b * 8;
    const float* xi = x + (long long)b * 3 * plane + p0;
    float v[3][kLanePix], g[kLanePix];
#pragma unroll
    for (int k = 0; k < kLanePix; ++k) {
        v[0][k] = v[1][k] = v[2][k] = 0.f; g[k] = 0.f;
        if (k < n) {
            float px[3] = {xi[k], xi[plane + k], xi[2ll * plane + k]};
            for (int j = 0; j < kc; ++j) jitter_op(ord[j], fac, 0.f, px);
            g[k] = gray_of(px);
            v[0][k] = px[0]; v[1][k] = px[1]; v[2][k] = px[2];
        }
    }
    if (n > 0) {
        float* oi = out + (long long)b * 3 * plane + p0;
        store_run(oi, v[0], n, vec); store_run(oi + plane, v[1], n, vec); store_run(oi + 2ll * plane, v[2], n, vec);
    }
    tile_partial(g, red, partials + (long long)b * tiles + tile);
}

// a workgroup takes kPostTiles tiles in turn, so the sum of the image's partials is made once per 4096 pixels
constexpr int kPostTiles = 4;

__global__ __launch_bounds__(256) void cs_jitter_post_kernel(float* __restrict__ out, int plane, int tiles, const int* __restrict__ order,
                                                             const float* __restrict__ factors, const double* __restrict__ partials,
                                                             Norm nm, int vec) {
    const int b = blockIdx.y;
    int ord[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ord[j] = order[b * 4 + j] & 3;
    const int kc = contrast_at(ord);
    const float* fac = factors + b * 8;
    double sum = 0.0;
    for (int t = 0; t < tiles; ++t) sum = sum + partials[(long long)b * tiles + t];          // uniform: every lane adds in tile order
    const float mean = (float)(sum / (double)plane);
    for (int i = 0; i < kPostTiles; ++i) {
        const int tile = blockIdx.x * kPostTiles + i;
        const int p0 = (tile * 256 + (int)threadIdx.x) * kLanePix;
        const int n = clampi(plane - p0, 0, kLanePix);
        if (tile >= tiles || n <= 0) return;                                    // (the kernel has no barrier)
        float* oi = out + (long long)b * 3 * plane + p0;
        float v[3][kLanePix];
        if (vec && n == kLanePix) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float4 t = *reinterpret_cast<const float4*>(oi + (long long)c * plane);
                v[c][0] = t.x; v[c][1] = t.y; v[c][2] = t.z; v[c][3] = t.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < kLanePix; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][k] = k < n ? oi[(long long)c * plane + k] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < kLanePix; ++k) {
            if (k < n) {
                float px[3] = {v[0][k], v[1][k], v[2][k]};
                for (int j = kc; j < 4; ++j) jitter_op(ord[j], fac, mean, px);
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][k] = normalize(px[c], nm, c);
            }
        }
        store_run(oi, v[0], n, vec); store_run(oi + plane, v[1], n, vec); store_run(oi + 2ll * plane, v[2], n, vec);
    }
}

inline bool make_norm(const float* mean3, const float* std3, Norm& nm) {
    nm.on = mean3 != nullptr && std3 != nullptr;
    for (int c = 0; c < 3; ++c) { nm.m[c] = nm.on ? mean3[c] : 0.f; nm.s[c] = nm.on ? std3[c] : 1.f; }
    return !nm.on || (nm.s[0] != 0.f && nm.s[1] != 0.f && nm.s[2] != 0.f);
}

inline int tiles_of(long long plane) { return (int)((plane + kTilePix - 1) / kTilePix); }

}  // namespace

extern "C" int egm_color_jitter_tiles(int H, int W) {
    EGM_REQUIRE(H > 0 && W > 0 && H <= kMaxSide && W <= kMaxSide, "color_jitter_tiles: sides must be in 1 .. 32767");
    return tiles_of((long long)H * W);
}

extern "C" int egm_mask_profile_u8(const egm_clipseg_batch_desc* table_dev, int B, int max_units, int* profile_dev, egm_stream_t s) {
    EGM_REQUIRE(table_dev && profile_dev, "mask_profile_u8: null pointer");
    EGM_REQUIRE(B > 0 && B <= 65535 && max_units > 0, "mask_profile_u8: bad batch or unit count");
    hipLaunchKernelGGL(cs_profile_kernel, dim3(max_units < 1024 ? max_units : 1024, B), dim3(256), 0, (hipStream_t)s, table_dev, profile_dev);
    EGM_CHECK_LAUNCH("mask_profile_u8");
    return EGM_OK;
}

extern "C" int egm_clipseg_choose(const egm_clipseg_batch_desc* table_dev, int B, int* profile_dev, int* choice_b3, egm_stream_t s) {
    EGM_REQUIRE(table_dev && choice_b3, "clipseg_choose: null pointer");
    EGM_REQUIRE(B > 0 && B <= 65535, "clipseg_choose: bad batch");
    hipLaunchKernelGGL(cs_choose_kernel, dim3(B), dim3(256), 0, (hipStream_t)s, table_dev, profile_dev, choice_b3);
    EGM_CHECK_LAUNCH("clipseg_choose");
    return EGM_OK;
}

extern "C" int egm_clipseg_batch_u8(const egm_clipseg_batch_desc* table_dev, int B, int S, const int* choice_b3, const int* order_dev,
                                    const float* factors_dev, float* out_img_b3ss, float* out_seg_b1ss, double* partials,
                                    const float* mean3_host, const float* std3_host, egm_stream_t s) {
    EGM_REQUIRE(table_dev && choice_b3 && out_img_b3ss && out_seg_b1ss && mean3_host && std3_host, "clipseg_batch_u8: null pointer");
    EGM_REQUIRE(B > 0 && B <= 65535 && S >= 2 && S <= kMaxSide, "clipseg_batch_u8: bad batch or size");
    EGM_REQUIRE((long long)B * 3 * S * S < (1ll << 31), "clipseg_batch_u8: B*3*S*S must stay below 2^31");
    const bool jit = order_dev != nullptr || factors_dev != nullptr;
    EGM_REQUIRE(!jit || (order_dev && factors_dev && partials), "clipseg_batch_u8: a jitter needs order, factors and partials");
    Norm nm;
    EGM_REQUIRE(make_norm(mean3_host, std3_host, nm), "clipseg_batch_u8: zero std");
    const int plane = S * S, tiles = tiles_of(plane);
    const int vec = plane % 4 == 0 && egm_aligned16(out_img_b3ss) && egm_aligned16(out_seg_b1ss);
    if (jit)
        hipLaunchKernelGGL(cs_resample_kernel<true>, dim3(tiles, B), dim3(256), 0, (hipStream_t)s, table_dev, S, choice_b3, order_dev,
                           factors_dev, out_img_b3ss, out_seg_b1ss, partials, nm, vec);
    else
        hipLaunchKernelGGL(cs_resample_kernel<false>, dim3(tiles, B), dim3(256), 0, (hipStream_t)s, table_dev, S, choice_b3, order_dev,
                           factors_dev, out_img_b3ss, out_seg_b1ss, partials, nm, vec);
    EGM_CHECK_LAUNCH("clipseg_batch_u8");
    return EGM_OK;
}

extern "C" int egm_color_jitter_f32(const float* x_b3hw, float* out_b3hw, int B, int H, int W, const int* order_dev,
                                    const float* factors_dev, double* partials, const float* mean3_host, const float* std3_host,
                                    int stages, egm_stream_t s) {
    EGM_REQUIRE(out_b3hw && order_dev && factors_dev && partials, "color_jitter_f32: null pointer");
    EGM_REQUIRE(stages >= 1 && stages <= 3 && (!(stages & 1) || x_b3hw), "color_jitter_f32: stages is 1 (front), 2 (rest) or 3, the front needs x");
    EGM_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && H <= kMaxSide && W <= kMaxSide, "color_jitter_f32: bad batch or size");
    EGM_REQUIRE((long long)B * 3 * H * W < (1ll << 31), "color_jitter_f32: B*3*H*W must stay below 2^31");
    EGM_REQUIRE((mean3_host == nullptr) == (std3_host == nullptr), "color_jitter_f32: mean and std come together");
    Norm nm;
    EGM_REQUIRE(make_norm(mean3_host, std3_host, nm), "color_jitter_f32: zero std");
    const int plane = H * W, tiles = tiles_of(plane);
    const int vec = plane % 4 == 0 && egm_aligned16(out_b3hw);
    if (stages & 1) {
        hipLaunchKernelGGL(cs_jitter_pre_kernel, dim3(tiles, B), dim3(256), 0, (hipStream_t)s, x_b3hw, out_b3hw, plane, order_dev,
                           factors_dev, partials, vec);
        EGM_CHECK_LAUNCH("color_jitter_f32 (front)");
    }
    if (stages & 2) {
        hipLaunchKernelGGL(cs_jitter_post_kernel, dim3((tiles + kPostTiles - 1) / kPostTiles, B), dim3(256), 0, (hipStream_t)s,
                           out_b3hw, plane, tiles, order_dev, factors_dev, (const double*)partials, nm, vec);
        EGM_CHECK_LAUNCH("color_jitter_f32 (rest)");
    }
    return EGM_OK;
}
