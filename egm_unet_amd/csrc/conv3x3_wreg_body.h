// Body of conv3x3_wreg's kernel, included by conv3x3_wreg.hip into two kernels: the egm_conv_fwd kernel (ACT = EGM_ACT_NONE: unchanged
// name and code) and its egm_conv_fwd_act twin (ACT a template argument).  No include guard: included once per kernel.
    static_assert(CH == 1, "one 32-channel stage per tile");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    typedef __attribute__((address_space(3))) unsigned char* lds_p;
    const int grp = blockIdx.x;                                       // one cout tile: the block index is the pixel group
    if (grp >= p.G) return;
    const int tid = threadIdx.x, lane = tid & 63, r31 = lane & 31, h = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tpi = p.tiles_y * p.tiles_x;
    const unsigned smem_lds = (unsigned)(unsigned long long)(lds_p)smem;
    const void* const zp = reinterpret_cast<const void*>(egm_zero_page_wreg);
    const bool late = wv >= 4;                                        // waves 4-7: multiply first, store the previous tile afterwards

    // ---- per-lane DMA sources: instruction k of this wave is stage instruction j = wv + 8k, slots 64j + lane
    int rel[KT];            // element offset from the tile's halo origin; -1: the slot lies behind the patch (padding of the last instruction)
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        const int j = wv + 8 * k;
        const int slot = j * 64 + lane, pix = slot >> 2, prow = pix / PW, col = pix - prow * PW;
        const int cg = (slot & 3) ^ ((col >> 2) & 3);
        rel[k] = (j < NPI && pix < PH * PW) ? (prow * p.W + col) * p.ldx + cg * 8 : -1;
    }
    // tile walk pt = grp, grp + G, ...: (image, tile row, tile column) advance by constant steps with carries -- a decode by division
    // costs ~500 clk per tile here (two iterators, three runtime divisions each), a tenth of a 16 x 32 tile's budget
    struct Tile { int pt, n, ty, tx; };
    const int d_n = p.G / tpi, d_rem = p.G - d_n * tpi, d_y = d_rem / p.tiles_x, d_x = d_rem - d_y * p.tiles_x;
    auto first_tile = [&](Tile& t) {
        t.pt = grp; t.n = grp / tpi; const int trem = grp - t.n * tpi;
        t.ty = trem / p.tiles_x; t.tx = trem - t.ty * p.tiles_x;
    };
    auto next_tile = [&](Tile& t) {
        t.pt += p.G;
        t.tx += d_x; if (t.tx >= p.tiles_x) { t.tx -= p.tiles_x; t.ty += 1; }
        t.ty += d_y; if (t.ty >= p.tiles_y) { t.ty -= p.tiles_y; t.n += 1; }
        t.n += d_n;
    };
    struct Src { const bf16_t* xb; int oy0, ox0; unsigned lds; bool interior; };
    auto make_src = [&](const Tile& t, int bufi) {
        Src q;
        q.oy0 = t.ty * TROWS; q.ox0 = t.tx * TW;
        q.xb = p.x + ((long long)(t.n * p.H + q.oy0 - 1) * p.W + (q.ox0 - 1)) * p.ldx;
        q.interior = q.oy0 >= 1 && q.oy0 + TROWS + 1 <= p.H && q.ox0 >= 1 && q.ox0 + TW + 1 <= p.W;      // whole halo window inside the image
        q.lds = smem_lds + bufi * STAGE + wv * 1024;
        return q;
    };
    auto dma = [&](const Src& q, int k) __attribute__((always_inline)) {
        bool ok = rel[k] >= 0;
        if (!q.interior) {                                            // border tiles (wave-uniform branch): the slot's pixel from its index
            const int pix = ((wv + 8 * k) * 64 + lane) >> 2, prow = pix / PW, col = pix - prow * PW;
            ok = ok && (unsigned)(q.oy0 - 1 + prow) < (unsigned)p.H && (unsigned)(q.ox0 - 1 + col) < (unsigned)p.W;
        }
        const void* src = ok ? reinterpret_cast<const void*>(q.xb + rel[k]) : zp;
        glds16(src, q.lds + k * 8192);
    };

    // ---- first stages on their way before anything else
    const int ntl = (p.npt - grp + p.G - 1) / p.G;                   // tiles = stages of this workgroup
    Tile it; first_tile(it);
#pragma unroll
    for (int i = 0; i < NBUF - 1; ++i) {
        if (i < ntl) {
            const Src q = make_src(it, i);
#pragma unroll
            for (int k = 0; k < KT; ++k) dma(q, k);
            next_tile(it);
        }
    }

    // ---- the wave's weights: fragment (tap, ks): rows = couts r31, k = channels 16ks + 8h .. +7 (chunk-major pack)
    bf16x8_t wr[9][2];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
            wr[tap][ks] = *reinterpret_cast<const bf16x8_t*>(p.w + ((long long)(tap * 2 + ks) * p.Cout + r31) * 16 + h * 8);
    // fragment read addresses (bytes inside a stage buffer): column shift s, k-step ks
    int pb[3][2];
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int col = r31 + s, cg = 2 * ks + h;
            pb[s][ks] = ((R * wv) * PW + col) * 64 + ((cg ^ ((col >> 2) & 3)) * 16);
        }

    float ssum[8], ssq[8];
    zero8(ssum); zero8(ssq);
    unsigned char* ot = smem + NBUF * STAGE + wv * (R * 32 * OROW);   // wave-private out tile: R rows x 32 pixels x 32 couts
    unsigned char* dump = reinterpret_cast<unsigned char*>(egm_dump_wreg) + lane * 16;
    f32x16_t acc[R];

    auto compute = [&](int bufi, bool with_dma, const Src& q) __attribute__((always_inline)) {
        const unsigned char* sb = smem + bufi * STAGE;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                bf16x8_t fb[R + 2];                                   // the group's four patch-row fragments in flight together
#pragma unroll
                for (int rho = 0; rho < R + 2; ++rho) fb[rho] = *reinterpret_cast<const bf16x8_t*>(sb + pb[s][ks] + rho * (PW * 64));
#pragma unroll
                for (int rho = 0; rho < R + 2; ++rho) {
#pragma unroll
                    for (int m = 0; m < R; ++m) {
                        const int r = rho - m;
                        if (r >= 0 && r < 3) acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wr[r * 3 + s][ks], fb[rho], acc[m], 0, 0, 0);
                    }
                }
                const int gi = ks * 3 + s;                            // 6 groups per stage carry the KT = 5 DMA instructions
                if (gi < KT) {
                    if (with_dma) dma(q, gi);
                }
            }
    };
    // epilogue, first half: accumulators -> bf16 -> the wave's LDS tile (both rows); runs right behind the MFMA phase, so the
    // transposition's LDS latency passes while the workgroup crosses the barrier
    auto park = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int m = 0; m < R; ++m)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                if (p.bias != nullptr) {                              // rare; in fp32, before the ONE rounding to bf16
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int co = gq * 8 + h * 4 + j;
                        acc[m][gq * 4 + j] += co < p.bias_n ? p.bias[co] : 0.f;
                    }
                }
                if constexpr (ACT != EGM_ACT_NONE) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[m][gq * 4 + j] = conv_epi_act<ACT, true>(acc[m][gq * 4 + j]);
                }
                uint2 v;
                v.x = pack_bf16x2(acc[m][gq * 4 + 0], acc[m][gq * 4 + 1]);
                v.y = pack_bf16x2(acc[m][gq * 4 + 2], acc[m][gq * 4 + 3]);
                *reinterpret_cast<uint2*>(ot + (m * 32 + r31) * OROW + (gq * 8 + h * 4) * 2) = v;
            }
    };
    // second half, one iteration later: whole channel vectors back from LDS, coalesced stores, BatchNorm partial sums.  EXACTLY
    // R*2 store instructions per call whatever the tile (lanes outside the image write a dump line): the counted vmcnt of waves 4-7
    // depends on it.
    auto store_tile = [&](const Tile& t) __attribute__((always_inline)) {
        const int cv = lane & 3, slot = lane >> 2;                    // 4 channel vectors per pixel, 16 pixel slots
        const int oy0 = t.ty * TROWS, ox0 = t.tx * TW;
        uint4 raw[R][2];
#pragma unroll
        for (int m = 0; m < R; ++m)
#pragma unroll
            for (int i2 = 0; i2 < 2; ++i2) raw[m][i2] = *reinterpret_cast<const uint4*>(ot + (m * 32 + i2 * 16 + slot) * OROW + cv * 16);
#pragma unroll
        for (int m = 0; m < R; ++m) {
            const int oy = oy0 + R * wv + m;                          // wave-uniform
            bf16_t* yrow = p.y + ((long long)(t.n * p.H + oy) * p.W + ox0) * p.ldy + cv * 8;
#pragma unroll
            for (int i2 = 0; i2 < 2; ++i2) {
                const int pl = i2 * 16 + slot;
                const bool ok = oy < p.H && ox0 + pl < p.W;
                uint4 rw = raw[m][i2];
                if (!ok) rw = make_uint4(0, 0, 0, 0);
                unsigned char* dst = ok ? reinterpret_cast<unsigned char*>(yrow + (long long)pl * p.ldy) : dump;
                egm_store16_conv(dst, rw);
                float v[8];
                v[0] = __uint_as_float(rw.x << 16); v[1] = __uint_as_float(rw.x & 0xffff0000u);
                v[2] = __uint_as_float(rw.y << 16); v[3] = __uint_as_float(rw.y & 0xffff0000u);
                v[4] = __uint_as_float(rw.z << 16); v[5] = __uint_as_float(rw.z & 0xffff0000u);
                v[6] = __uint_as_float(rw.w << 16); v[7] = __uint_as_float(rw.w & 0xffff0000u);
#pragma unroll
                for (int j = 0; j < 8; ++j) { ssum[j] += v[j]; ssq[j] = fmaf(v[j], v[j], ssq[j]); }
            }
        }
    };

#ifdef EGM_TILE_TIMING
    long long tph[6] = {0, 0, 0, 0, 0, 0};
    __builtin_amdgcn_sched_barrier(0);
    long long tmark = __builtin_amdgcn_s_memtime();
    const long long treal0 = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_sched_barrier(0);
#define EGM_TICK(i) do { __builtin_amdgcn_sched_barrier(0); const long long t_ = __builtin_amdgcn_s_memtime(); \
                         __builtin_amdgcn_s_waitcnt(0xC07F); __builtin_amdgcn_sched_barrier(0); tph[i] += t_ - tmark; tmark = t_; } while (0)
#else
#define EGM_TICK(i) do { } while (0)
#endif
    // ---- pipeline.  Tile t uses buffer t % NBUF; iteration t issues tile t + NBUF - 1, multiplies tile t, stores tile t - 1.
    // Waves 0-3 run [store t-1 | multiply t | park t], waves 4-7 [multiply t | store t-1 | park t]: each SIMD hosts one wave of either
    // group, so a store phase (VALU, LDS, memory) always sits beside the partner's MFMA phase.
    // vmcnt bookkeeping (loads, stores and LDS-DMA retire in issue order): at the end of iteration t a wave must have its share of tile
    // t+1 in LDS; younger than those DMAs are, for waves 0-3, only this iteration's KT DMAs (their stores came first) -> vmcnt(KT);
    // for waves 4-7 this iteration's KT DMAs AND its R*2 stores -> vmcnt(KT + R*2), except in iteration 0 (nothing to store yet).
    if (ntl > 1) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(KT) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    EGM_TICK(5);
    int bc = 0, bi = NBUF - 1;
    Tile cu; first_tile(cu);
    Tile prev = cu;
    for (int t = 0; t < ntl; ++t) {
        const bool more = t + NBUF - 1 < ntl;
        const Src q = make_src(it, bi);
        if (more) next_tile(it);
        EGM_TICK(0);
        if (t > 0 && !late) store_tile(prev);
        EGM_TICK(1);
#pragma unroll
        for (int m = 0; m < R; ++m)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[m][i] = 0.f;
        compute(bc, more, q);
        EGM_TICK(2);
        if (t > 0 && late) store_tile(prev);
        park();
        EGM_TICK(1);
        if (!more) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else if (late && t > 0) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(KT + R * 2) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" :: "n"(KT) : "memory");
        EGM_TICK(3);
        __builtin_amdgcn_s_barrier();
        EGM_TICK(4);
        prev = cu; next_tile(cu);
        bc = (bc + 1 == NBUF) ? 0 : bc + 1;
        bi = (bi + 1 == NBUF) ? 0 : bi + 1;
    }
    store_tile(prev);
    EGM_TICK(1);
#ifdef EGM_TILE_TIMING
    if (p.stats != nullptr) {       // [grp][wave][8]: issue, epilogue, mfma, vmcnt wait, barrier, prologue, stages, 100 MHz ticks
        const long long treal = __builtin_amdgcn_s_memrealtime() - treal0;
        if (lane == 0) {
            float* o = p.stats + ((long long)grp * 8 + wv) * 8;
            for (int i = 0; i < 6; ++i) o[i] = (float)tph[i];
            o[6] = (float)ntl; o[7] = (float)treal;
        }
        return;
    }
#endif

    if (p.stats != nullptr) {
        // lanes with equal cv (lane & 3) hold partial sums of the same 8 channels
#pragma unroll
        for (int j = 0; j < 8; ++j)
            for (int o = 4; o < 64; o <<= 1) { ssum[j] += __shfl_xor(ssum[j], o, 64); ssq[j] += __shfl_xor(ssq[j], o, 64); }
        float* red = reinterpret_cast<float*>(smem);                  // [8 waves][2][32]; the stage buffers are idle now
        if (lane < 4) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { red[(wv * 2 + 0) * 32 + lane * 8 + j] = ssum[j]; red[(wv * 2 + 1) * 32 + lane * 8 + j] = ssq[j]; }
        }
        __syncthreads();
        if (tid < 64) {
            const int which = tid >> 5, j = tid & 31;
            float v = 0.f;
#pragma unroll
            for (int w8 = 0; w8 < 8; ++w8) v += red[(w8 * 2 + which) * 32 + j];
            p.stats[((long long)grp * 2 + which) * p.Cout + j] = v;
        }
    }
