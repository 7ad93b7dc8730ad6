// Body of conv_igemm's kernel, included by conv_igemm.hip into two kernels: the egm_conv_fwd kernel (ACT = EGM_ACT_NONE: unchanged
// name and code) and its egm_conv_fwd_act twin (ACT a template argument).  No include guard: included once per kernel.
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using M = Mma<T>;
    constexpr int VEC = 16 / sizeof(T);               // elements per 16-byte vector
    constexpr int NVPP = KC / VEC;                    // vectors per LDS row
    constexpr int PS = M::kPixStride;

    // ---- block -> (pixel tile, cout tile), XCD-aware
    const int b = blockIdx.x, q = b >> 3;
    const int ct = q % p.nct;
    const int pt = (q / p.nct) * 8 + (b & 7);
    if (pt >= p.npt) return;
    const int tpi = p.tiles_y * p.tiles_x;
    const int n = pt / tpi, trem = pt - n * tpi;
    const int oy0 = (trem / p.tiles_x) * TH, ox0 = (trem % p.tiles_x) * TW;
    const int co0 = ct * NT * 32;

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r31 = lane & 31, h = lane >> 5;
    const T* __restrict__ xg = reinterpret_cast<const T*>(p.x);
    const T* __restrict__ wg = reinterpret_cast<const T*>(p.w);

    const bool halo = (p.dil == 1);
    const int ngroups = halo ? 1 : p.KH * p.KW;
    const int wh = halo ? p.KH : 1, ww = halo ? p.KW : 1;
    const int PH = TH + wh - 1, PW = TW + ww - 1;
    unsigned char* patch = smem;
    unsigned char* wts = smem + p.patch_bytes;
    const int rows_per_stage = halo ? p.wrows_per_stage : 1;

    f32x16_t acc[2][NT];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[m][t][i] = 0.f;

    for (int g = 0; g < ngroups; ++g) {
        int offy, offx, tapbase;
        if (halo) { offy = -(p.KH / 2); offx = -(p.KW / 2); tapbase = 0; }
        else {
            offy = (g / p.KW - p.KH / 2) * p.dil; offx = (g % p.KW - p.KW / 2) * p.dil; tapbase = g;
            // shifted tile entirely outside the image -> contributes only zeros (block-uniform test)
            if (oy0 + offy >= p.H || oy0 + offy + TH <= 0 || ox0 + offx >= p.W || ox0 + offx + TW <= 0) continue;
        }
        for (int c0 = 0; c0 < p.Cin; c0 += KC) {
            const int kc = min(KC, p.Cin - c0);
            const int nks = (kc + M::kStep - 1) / M::kStep;
            __syncthreads();                                   // everyone done reading the previous patch/weights
            // ---- stage the input patch (zero-filled outside the image / beyond Cin)
            for (int i = tid; i < PH * PW * NVPP; i += 256) {
                const int pix = i / NVPP, v = i - pix * NVPP;
                const int py = pix / PW, px = pix - py * PW;
                const int iy = oy0 + offy + py, ix = ox0 + offx + px, c = c0 + v * VEC;
                const bool ok = (iy >= 0) && (iy < p.H) && (ix >= 0) && (ix < p.W) && (c < p.Cin);
                const long long pixoff = (long long)(n * p.H + iy) * p.W + ix;
                const T* src = xg + pixoff * p.ldx + c;
                M::stage16(patch + pix * PS + v * 16, src, ok);
            }
            for (int wr0 = 0; wr0 < wh; wr0 += rows_per_stage) {
                const int nrows = min(rows_per_stage, wh - wr0);
                const int ntaps = nrows * ww;
                if (wr0 > 0) __syncthreads();                  // previous weight stage consumed
                // ---- stage weights of taps [wr0*ww, wr0*ww+ntaps) x NT*32 couts x KC
                for (int i = tid; i < ntaps * NT * 32 * NVPP; i += 256) {
                    const int row = i / NVPP, v = i - row * NVPP;
                    const int t = row / (NT * 32), j = row - t * (NT * 32);
                    const int co = co0 + j, c = c0 + v * VEC;
                    const int tap = tapbase + wr0 * ww + t;
                    const bool ok = (co < p.Cout) && (c < p.Cin);
                    const T* src = wg + egm_w_off(p.wl, tap, co, c, p.Cout, p.Cin);
                    M::stage16(wts + row * PS + v * 16, src, ok);
                }
                __syncthreads();
                // ---- MFMA over the staged taps
                for (int t = 0; t < ntaps; ++t) {
                    const int wr = wr0 + t / ww, ws = t - (t / ww) * ww;
                    const unsigned char* a0 = patch + ((2 * wv + 0 + wr) * PW + r31 + ws) * PS;
                    const unsigned char* a1 = patch + ((2 * wv + 1 + wr) * PW + r31 + ws) * PS;
                    const unsigned char* b0 = wts + (t * NT * 32 + r31) * PS;
                    for (int ks = 0; ks < nks; ++ks) {
                        const typename M::Frag fa0 = M::load(a0, ks, h), fa1 = M::load(a1, ks, h);
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) {
                            const typename M::Frag fb = M::load(b0 + nt * 32 * PS, ks, h);
                            acc[0][nt] = M::mma(fa0, fb, acc[0][nt]);
                            acc[1][nt] = M::mma(fa1, fb, acc[1][nt]);
                        }
                    }
                }
            }
        }
    }

    // ---- epilogue: C/D layout of 32x32 MFMA: col (cout) = lane&31, row (pixel) = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
    T* __restrict__ yg = reinterpret_cast<T*>(p.y);
    float ssum[NT], ssq[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) { ssum[nt] = 0.f; ssq[nt] = 0.f; }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int co = co0 + nt * 32 + r31;
        const bool cok = co < p.Cout;
        const float bv = (p.bias != nullptr && co < p.bias_n) ? p.bias[co] : 0.f;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int oy = oy0 + 2 * wv + m;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int ox = ox0 + (i & 3) + 8 * (i >> 2) + 4 * h;
                if (cok && oy < p.H && ox < p.W) {
                    const T o = from_f32<T>(conv_epi_act<ACT, sizeof(T) == 2>(acc[m][nt][i] + bv));
                    yg[((long long)(n * p.H + oy) * p.W + ox) * p.ldy + co] = o;
                    const float f = to_f32(o);
                    ssum[nt] += f; ssq[nt] += f * f;
                }
            }
        }
    }
    if (p.stats != nullptr) {
        __syncthreads();                                       // LDS is free again
        float* red = reinterpret_cast<float*>(smem);           // [4 waves][2][NT*32]
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const float s = ssum[nt] + __shfl_xor(ssum[nt], 32, 64);
            const float qq = ssq[nt] + __shfl_xor(ssq[nt], 32, 64);
            if (h == 0) {
                red[(wv * 2 + 0) * NT * 32 + nt * 32 + r31] = s;
                red[(wv * 2 + 1) * NT * 32 + nt * 32 + r31] = qq;
            }
        }
        __syncthreads();
        if (tid < 2 * NT * 32) {
            const int which = tid / (NT * 32), j = tid - which * NT * 32;
            const int co = co0 + j;
            if (co < p.Cout) {
                float v = 0.f;
                for (int w4 = 0; w4 < 4; ++w4) v += red[(w4 * 2 + which) * NT * 32 + j];
                p.stats[((long long)pt * 2 + which) * p.Cout + co] = v;
            }
        }
    }
