// Exact ranking scores of binary logits on the device sort: step-wise average precision with one threshold per
// distinct score, the exact AUROC numerator and the best foreground IoU over every distinct score, per segment (an evaluation set or
// one image).
//   egm_rank_keys       one streaming launch over the scores and targets in egm_sweep_hist's forms -> (key, val) uint32 pairs
//   egm_rank_workspace  bytes of the sorted planes, the sort's workspace and the per-tile tables
//   egm_rank_scores     egm_sort_pairs_u32 over all 32 key bits, then along the sorted order of every segment
//     tile      per tile of kRankTile sorted elements: positives, kept elements, and (positives, index) up to the tile's last group end
//     scan      one workgroup per segment: the exclusive prefix of the positives and, as an exclusive maximum, the (TP, V) of the last
//               group end in front of every tile; the segment's totals {P, kept}
//     apply     per tile: F_j of every element (wave scan + offsets), V_j = j + 1; at every group end the previous group end's (TP, V)
//               from an exclusive max-scan, and from the two the AP term (double), the auc2 term (uint64) and the best-IoU candidate
//               (uint64 cross-multiplication); one partial of each per workgroup
//     finalize  one workgroup: the partials of a segment in a fixed order -> out_u64[s][8], out_f64[s]
// The key is the complement of the order-preserving map of the fp32 score (-0 -> +0, NaN -> -inf first), so ascending keys are
// descending scores, kept keys are <= 0xFF800000 and a dropped pixel's 0xFFFFFFFF sorts last: the kept elements of a segment are a
// prefix of its sorted order, hence V_j = j + 1, and equal scores are equal keys, next to each other.
// An element is a group end when its successor is missing, not kept or has another key: a decision about two neighbours, so a group
// of any length (one group over every tile of a segment included) costs what any other content costs.  What a group end needs from
// the groups in front of it is the (TP, V) of the previous group end; both counts never decrease along the order, so "the last one in
// front" is a maximum, and a maximum scans like a sum.
// As in lovasz_core.h: no workgroup waits for another, every loop is bounded by the arguments, no atomics on global memory, nothing
// allocates or waits for the device; 4 * 3 + 4 launches whatever S, L and the content.
#include "common.h"

namespace {

constexpr int kRankItems = 8;
constexpr int kRankTile = 256 * kRankItems;    // sorted elements per workgroup of the tile and apply passes (tests restate it)
constexpr unsigned int kRankDropped = 0xFFFFFFFFu;

// ---------------------------------------------------------------- keys
__device__ __forceinline__ unsigned int rank_key(float s) {
    if (!(s == s)) s = -__builtin_inff();                      // NaN ranks with -inf (the sweep's "NaN: bin 0")
    if (s == 0.f) s = 0.f;                                     // -0 -> +0
    const unsigned int b = __float_as_uint(s);
    return (b & 0x80000000u) ? b : (~b & 0x7FFFFFFFu);         // ~(negative ? ~b : b | 0x80000000)
}

template <bool TWO, bool TF32>
__global__ __launch_bounds__(256) void rank_keys_kernel(const float* __restrict__ scores, const void* __restrict__ target,
                                                        const unsigned char* __restrict__ target_cls, int C, int c_pos, int c_neg,
                                                        long long HW, unsigned int* __restrict__ keys, unsigned int* __restrict__ vals) {
    const long long n = blockIdx.y, p0 = (long long)blockIdx.x * kRankTile + threadIdx.x;
    const float* sp = scores + (n * C + (TWO ? c_pos : 0)) * HW;
    const float* sn = scores + (n * C + c_neg) * HW;          // (read only when TWO)
    const float* tf = reinterpret_cast<const float*>(target) + n * HW;
    const unsigned char* tb = reinterpret_cast<const unsigned char*>(target) + n * HW;
    float s[kRankItems];
    unsigned int cls[kRankItems];                              // 0 negative, 1 positive, anything else dropped
#pragma unroll
    for (int i = 0; i < kRankItems; ++i) {                     // every load first
        const long long p = p0 + i * 256;
        s[i] = 0.f;
        cls[i] = 2u;
        if (p < HW) {
            s[i] = sp[p];
            if (TWO) s[i] -= sn[p];
            cls[i] = TF32 ? (tf[p] > 0.5f ? 1u : 0u) : (unsigned int)target_cls[tb[p]];
        }
    }
#pragma unroll
    for (int i = 0; i < kRankItems; ++i) {
        const long long p = p0 + i * 256;
        if (p < HW) {
            const bool kept = cls[i] <= 1u;
            keys[n * HW + p] = kept ? rank_key(s[i]) : kRankDropped;
            vals[n * HW + p] = kept ? (cls[i] | 2u) : 0u;
        }
    }
}

// ---------------------------------------------------------------- along the sorted order
__device__ __forceinline__ unsigned int rank_kept(unsigned int val) { return (val >> 1) & 1u; }
__device__ __forceinline__ unsigned int rank_pos(unsigned int val) { return val & (val >> 1) & 1u; }

// element idx of a segment (idx < L) is a group end: it is kept and its successor is missing, not kept or has another key
__device__ __forceinline__ bool rank_group_end(const unsigned int* __restrict__ k, const unsigned int* __restrict__ v, long long idx, int L,
                                               unsigned int key, unsigned int val) {
    if (!rank_kept(val)) return false;
    if (idx + 1 >= L) return true;
    return !rank_kept(v[idx + 1]) || k[idx + 1] != key;
}

// tiles[seg][tile] = {positives, kept, positives up to and including the tile's last group end, its tile-local index + 1 (0: none)}
__global__ __launch_bounds__(256) void rank_tile_kernel(const unsigned int* __restrict__ skeys, const unsigned int* __restrict__ svals, int L,
                                                        int ntiles, uint4* __restrict__ tiles) {
    __shared__ unsigned int red_cnt[4], red_end[4], red_pos[4];
    const int tile = blockIdx.x, seg = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned int* k = skeys + (long long)seg * L;
    const unsigned int* v = svals + (long long)seg * L;
    unsigned int cnt = 0u, last = 0u, posbits = 0u;            // positives | kept << 16: at most 2048 of each
#pragma unroll
    for (int i = 0; i < kRankItems; ++i) {
        const int local = i * 256 + threadIdx.x;
        const long long idx = (long long)tile * kRankTile + local;
        if (idx < L) {
            const unsigned int key = k[idx], val = v[idx];
            cnt += rank_pos(val) + (rank_kept(val) << 16);
            posbits |= rank_pos(val) << i;
            if (rank_group_end(k, v, idx, L, key, val)) last = (unsigned int)local + 1u;     // (local ascends with i)
        }
    }
    cnt = wave_sum_u32(cnt);
    last = wave_max_u32(last);
    if (lane == 0) { red_cnt[wv] = cnt; red_end[wv] = last; }
    __syncthreads();
    cnt = red_cnt[0] + red_cnt[1] + red_cnt[2] + red_cnt[3];
    last = max(max(red_end[0], red_end[1]), max(red_end[2], red_end[3]));
    unsigned int upto = 0u;
#pragma unroll
    for (int i = 0; i < kRankItems; ++i) upto += (unsigned int)(i * 256 + (int)threadIdx.x) < last ? (posbits >> i) & 1u : 0u;
    upto = wave_sum_u32(upto);
    if (lane == 0) red_pos[wv] = upto;
    __syncthreads();
    if (threadIdx.x == 0)
        tiles[(long long)seg * ntiles + tile] = make_uint4(cnt & 0xFFFFu, cnt >> 16, red_pos[0] + red_pos[1] + red_pos[2] + red_pos[3], last);
}

// pre[seg][tile] = {positives in front of the tile, TP and V of the last group end in front of it (0, 0: none), 0}; totals[seg] = {P, kept}
__global__ __launch_bounds__(1024) void rank_scan_kernel(const uint4* __restrict__ tiles, int ntiles, uint4* __restrict__ pre,
                                                         uint2* __restrict__ totals) {
    __shared__ uint2 wsum[16], wmax[16];
    const uint4* c = tiles + (long long)blockIdx.x * ntiles;
    uint4* o = pre + (long long)blockIdx.x * ntiles;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint2 carry = make_uint2(0u, 0u), cmax = make_uint2(0u, 0u);
    for (int base = 0; base < ntiles; base += 1024) {
        const int at = base + threadIdx.x;
        const uint4 own = at < ntiles ? c[at] : make_uint4(0u, 0u, 0u, 0u);
        uint2 x = make_uint2(own.x, own.y);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned int yx = __shfl_up(x.x, d, 64), yy = __shfl_up(x.y, d, 64);
            if (lane >= d) { x.x += yx; x.y += yy; }
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
        const unsigned int pref = carry.x + before.x + x.x - own.x;
        // the tile's last group end in the segment's counts; V = its index + 1 (the kept elements are a prefix of the order)
        uint2 m = own.w ? make_uint2(pref + own.z, (unsigned int)at * (unsigned int)kRankTile + own.w) : make_uint2(0u, 0u);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned int yx = __shfl_up(m.x, d, 64), yy = __shfl_up(m.y, d, 64);
            if (lane >= d) { m.x = max(m.x, yx); m.y = max(m.y, yy); }
        }
        if (lane == 63) wmax[wv] = m;
        uint2 ex = make_uint2(__shfl_up(m.x, 1, 64), __shfl_up(m.y, 1, 64));
        if (lane == 0) ex = make_uint2(0u, 0u);
        __syncthreads();
        uint2 mb = cmax, mt = cmax;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint2 w = wmax[i];
            if (i < wv) { mb.x = max(mb.x, w.x); mb.y = max(mb.y, w.y); }
            mt.x = max(mt.x, w.x); mt.y = max(mt.y, w.y);
        }
        if (at < ntiles) o[at] = make_uint4(pref, max(mb.x, ex.x), max(mb.y, ex.y), 0u);
        carry.x += total.x; carry.y += total.y;
        cmax = mt;
        __syncthreads();
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// A best-IoU candidate: the group end with TP true and FP false positives at position V (1-based), key its score.  TP / (P + FP) is
// compared by cross-multiplication: TP < 2^31 and P + FP < 2^32, so a product stays below 2^63.  Equal ratios: the lower position
// (the higher score) wins, which makes the choice independent of the order of the reduction.  V = 0xFFFFFFFF: no candidate.
struct RankBest {
    unsigned int tp, fp, v, key;
};
__device__ __forceinline__ RankBest rank_best_none() { return RankBest{0u, 0u, 0xFFFFFFFFu, 0u}; }
__device__ __forceinline__ RankBest rank_better(const RankBest& a, const RankBest& b, unsigned int P) {
    const unsigned long long qa = (unsigned long long)a.tp * ((unsigned long long)P + b.fp);
    const unsigned long long qb = (unsigned long long)b.tp * ((unsigned long long)P + a.fp);
    return (qb > qa || (qb == qa && b.v < a.v)) ? b : a;
}
__device__ __forceinline__ RankBest rank_best_wave(RankBest a, unsigned int P) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        RankBest b;
        b.tp = __shfl_xor(a.tp, o, 64); b.fp = __shfl_xor(a.fp, o, 64); b.v = __shfl_xor(a.v, o, 64); b.key = __shfl_xor(a.key, o, 64);
        a = rank_better(a, b, P);
    }
    return a;
}

// The tile's elements in the order (wave w, round i, lane l) = tile element w * 512 + i * 64 + l, as lovasz_apply_kernel takes them.
__global__ __launch_bounds__(256) void rank_apply_kernel(const unsigned int* __restrict__ skeys, const unsigned int* __restrict__ svals, int L,
                                                         int ntiles, const uint4* __restrict__ pre, const uint2* __restrict__ totals,
                                                         unsigned int* __restrict__ tp_out, double* __restrict__ part_ap,
                                                         unsigned long long* __restrict__ part_u64, uint4* __restrict__ part_best) {
    __shared__ unsigned int wtot[4];
    __shared__ uint2 wend[4];
    __shared__ double red_ap[4];
    __shared__ unsigned long long red_auc[4];
    __shared__ unsigned int red_groups[4];
    __shared__ uint4 red_best[4];
    const int tile = blockIdx.x, seg = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long off = (long long)seg * L;
    const unsigned int* k = skeys + off;
    const unsigned int* v = svals + off;
    const long long base = (long long)tile * kRankTile + wv * (64 * kRankItems) + lane;
    unsigned int key[kRankItems], inc[kRankItems];
    unsigned int ends = 0u, run = 0u;                          // bit i: the lane's element of round i is a group end
#pragma unroll
    for (int i = 0; i < kRankItems; ++i) {
        const long long idx = base + i * 64;
        unsigned int x = 0u;
        key[i] = 0u;
        if (idx < L) {
            key[i] = k[idx];
            const unsigned int val = v[idx];
            x = rank_pos(val);
            ends |= (rank_group_end(k, v, idx, L, key[i], val) ? 1u : 0u) << i;
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned int y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        inc[i] = run + x;
        run += __shfl(x, 63, 64);
    }
    if (lane == 0) wtot[wv] = run;
    __syncthreads();
    unsigned int before = 0u;
#pragma unroll
    for (int w = 0; w < 4; ++w) before += w < wv ? wtot[w] : 0u;
    const uint4 pr = pre[(long long)seg * ntiles + tile];
    const unsigned int P = totals[seg].x;
    const unsigned int f0 = pr.x + before;
    // the (TP, V) of the last group end in front of every element: an exclusive max-scan of the group ends' own (F, V)
    unsigned int ptp[kRankItems], pv[kRankItems];
    uint2 mrun = make_uint2(0u, 0u);
#pragma unroll
    for (int i = 0; i < kRankItems; ++i) {
        const long long idx = base + i * 64;
        inc[i] += f0;                                          // F_j
        if (tp_out && idx < L) tp_out[off + idx] = inc[i];
        const bool e = (ends >> i) & 1u;
        uint2 m = e ? make_uint2(inc[i], (unsigned int)idx + 1u) : make_uint2(0u, 0u);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned int yx = __shfl_up(m.x, d, 64), yy = __shfl_up(m.y, d, 64);
            if (lane >= d) { m.x = max(m.x, yx); m.y = max(m.y, yy); }
        }
        const unsigned int ex = __shfl_up(m.x, 1, 64), ey = __shfl_up(m.y, 1, 64);
        ptp[i] = max(mrun.x, lane ? ex : 0u);
        pv[i] = max(mrun.y, lane ? ey : 0u);
        mrun.x = max(mrun.x, __shfl(m.x, 63, 64));
        mrun.y = max(mrun.y, __shfl(m.y, 63, 64));
    }
    if (lane == 0) wend[wv] = mrun;
    __syncthreads();
    uint2 cin = make_uint2(pr.y, pr.z);                        // the tile's carry-in and the waves in front
#pragma unroll
    for (int w = 0; w < 4; ++w)
        if (w < wv) { cin.x = max(cin.x, wend[w].x); cin.y = max(cin.y, wend[w].y); }
    double ap = 0.0;
    unsigned long long auc = 0ull;
    unsigned int groups = 0u;
    RankBest best = rank_best_none();
#pragma unroll
    for (int i = 0; i < kRankItems; ++i) {
        if (!((ends >> i) & 1u)) continue;
        const unsigned int tp = inc[i], vv = (unsigned int)(base + i * 64) + 1u, fp = vv - tp;
        const unsigned int tp0 = max(cin.x, ptp[i]), v0 = max(cin.y, pv[i]), fp0 = v0 - tp0;
        ap += (double)(tp - tp0) * (double)tp / (double)vv;
        auc += (unsigned long long)(fp - fp0) * ((unsigned long long)tp0 + tp);
        ++groups;
        best = rank_better(best, RankBest{tp, fp, vv, key[i]}, P);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ap += __shfl_xor(ap, o, 64);
    auc = wave_sum_u64(auc);
    groups = wave_sum_u32(groups);
    best = rank_best_wave(best, P);
    if (lane == 0) {
        red_ap[wv] = ap; red_auc[wv] = auc; red_groups[wv] = groups;
        red_best[wv] = make_uint4(best.tp, best.fp, best.v, best.key);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const long long at = (long long)seg * ntiles + tile;
        RankBest b = rank_best_none();
#pragma unroll
        for (int w = 0; w < 4; ++w) b = rank_better(b, RankBest{red_best[w].x, red_best[w].y, red_best[w].z, red_best[w].w}, P);
        part_ap[at] = (red_ap[0] + red_ap[1]) + (red_ap[2] + red_ap[3]);
        part_u64[2 * at] = red_auc[0] + red_auc[1] + red_auc[2] + red_auc[3];
        part_u64[2 * at + 1] = (unsigned long long)(red_groups[0] + red_groups[1] + red_groups[2] + red_groups[3]);
        part_best[at] = make_uint4(b.tp, b.fp, b.v, b.key);
    }
}

// one workgroup, a wave per segment at a time: out_u64[s] = {P, Nn, groups, auc2, best_tp, best_fp, best_key, 0}, out_f64[s] = ap
__global__ __launch_bounds__(1024) void rank_finalize_kernel(const double* __restrict__ part_ap, const unsigned long long* __restrict__ part_u64,
                                                             const uint4* __restrict__ part_best, const uint2* __restrict__ totals, int ntiles,
                                                             int S, unsigned long long* __restrict__ out_u64, double* __restrict__ out_f64) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int seg = wv; seg < S; seg += 16) {
        const uint2 tot = totals[seg];
        const unsigned int P = tot.x;
        double ap = 0.0;
        unsigned long long auc = 0ull, groups = 0ull;
        RankBest best = rank_best_none();
        for (int i = lane; i < ntiles; i += 64) {
            const long long at = (long long)seg * ntiles + i;
            ap += part_ap[at];
            auc += part_u64[2 * at];
            groups += part_u64[2 * at + 1];
            const uint4 b = part_best[at];
            best = rank_better(best, RankBest{b.x, b.y, b.z, b.w}, P);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ap += __shfl_xor(ap, o, 64);
        auc = wave_sum_u64(auc);
        groups = wave_sum_u64(groups);
        best = rank_best_wave(best, P);
        if (P == 0u) best = RankBest{0u, 0u, 0u, 0u};          // no positives: no best group
        if (lane < 8) {
            unsigned long long w = 0ull;
            switch (lane) {
                case 0: w = P; break;
                case 1: w = tot.y - P; break;
                case 2: w = groups; break;
                case 3: w = auc; break;
                case 4: w = best.tp; break;
                case 5: w = best.fp; break;
                case 6: w = best.key; break;
                default: break;
            }
            out_u64[(long long)seg * 8 + lane] = w;
        }
        if (lane == 0) out_f64[seg] = P ? ap / (double)P : 0.0;
    }
}

// ---------------------------------------------------------------- host
inline long long rank_up16(long long b) { return (b + 15) / 16 * 16; }
inline int rank_ntiles(long long L) { return (int)((L + kRankTile - 1) / kRankTile); }

struct RankPlanes {                                            // the workspace, every plane at a 16-byte boundary
    unsigned int *skeys, *svals;
    unsigned char* sort_ws;
    uint4 *tiles, *pre, *part_best;
    uint2* totals;
    double* part_ap;
    unsigned long long* part_u64;
    long long bytes;
};
inline RankPlanes rank_planes(void* workspace, int S, long long L) {
    RankPlanes pl;
    unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
    const long long plane = rank_up16((long long)S * L * 4), cells = (long long)S * rank_ntiles(L);
    long long at = 0;
    pl.skeys = reinterpret_cast<unsigned int*>(w + at); at += plane;
    pl.svals = reinterpret_cast<unsigned int*>(w + at); at += plane;
    pl.sort_ws = w + at; at += rank_up16(egm_sort_pairs_workspace(S, L));
    pl.tiles = reinterpret_cast<uint4*>(w + at); at += cells * 16;
    pl.pre = reinterpret_cast<uint4*>(w + at); at += cells * 16;
    pl.part_best = reinterpret_cast<uint4*>(w + at); at += cells * 16;
    pl.part_u64 = reinterpret_cast<unsigned long long*>(w + at); at += cells * 16;
    pl.part_ap = reinterpret_cast<double*>(w + at); at += rank_up16(cells * 8);
    pl.totals = reinterpret_cast<uint2*>(w + at); at += rank_up16((long long)S * 8);
    pl.bytes = at;
    return pl;
}
inline int rank_shape_check(const char* name, int S, long long L) {
    EGM_REQUIRE(S >= 1 && S <= 65535, "%s: %d segments, between 1 and 65535 are supported", name, S);
    EGM_REQUIRE(L >= 1 && L < (1ll << 31), "%s: segments of %lld elements, 1 <= L < 2^31 is supported", name, L);
    return EGM_OK;
}

}  // namespace

extern "C" int egm_rank_keys(const float* scores, int N, int C, int c_pos, int c_neg, long long HW, const void* target, int target_f32,
                             const unsigned char* target_cls, unsigned int* keys, unsigned int* vals, long long offset, egm_stream_t s) {
    EGM_REQUIRE(scores && target && keys && vals && (target_f32 || target_cls), "rank_keys: null pointer");
    EGM_REQUIRE(N >= 1 && N <= 65535, "rank_keys: %d samples, between 1 and 65535 are supported", N);
    EGM_REQUIRE(HW >= 1 && HW < (1ll << 31), "rank_keys: %lld pixels per sample, 1 <= HW < 2^31 is supported", HW);
    EGM_REQUIRE(C >= 1 && C <= 65535, "rank_keys: %d channels, between 1 and 65535 are supported", C);
    if (C > 1)
        EGM_REQUIRE(c_pos >= 0 && c_pos < C && c_neg >= 0 && c_neg < C && c_pos != c_neg,
                    "rank_keys: channels (%d, %d) must be two different channels of the %d", c_pos, c_neg, C);
    EGM_REQUIRE(offset >= 0, "rank_keys: element offset %lld is negative", offset);
    const dim3 grid((unsigned)rank_ntiles(HW), (unsigned)N);
#define EGM_RANK_LAUNCH(TWO, TF32) \
    hipLaunchKernelGGL((rank_keys_kernel<TWO, TF32>), grid, dim3(256), 0, (hipStream_t)s, scores, target, target_cls, C, c_pos, c_neg, HW, \
                       keys + offset, vals + offset)
    if (C > 1) { if (target_f32) EGM_RANK_LAUNCH(true, true); else EGM_RANK_LAUNCH(true, false); }
    else       { if (target_f32) EGM_RANK_LAUNCH(false, true); else EGM_RANK_LAUNCH(false, false); }
#undef EGM_RANK_LAUNCH
    EGM_CHECK_LAUNCH("rank_keys");
    return EGM_OK;
}

extern "C" long long egm_rank_workspace(int S, long long L) {
    if (rank_shape_check("rank_workspace", S, L) != EGM_OK) return EGM_ERR_ARG;
    return rank_planes(nullptr, S, L).bytes;
}

extern "C" int egm_rank_scores(const unsigned int* keys, const unsigned int* vals, int S, long long L, void* workspace,
                               unsigned long long* out_u64, double* out_f64, unsigned int* skeys_out, unsigned int* tp_out, egm_stream_t s) {
    const char* name = "rank_scores";
    EGM_REQUIRE(keys && vals && workspace && out_u64 && out_f64, "%s: null pointer", name);
    if (rank_shape_check(name, S, L) != EGM_OK) return EGM_ERR_ARG;
    EGM_REQUIRE(egm_aligned16(workspace), "%s: the workspace must be 16-byte aligned", name);
    EGM_REQUIRE(skeys_out != keys, "%s: skeys_out must not be the input keys", name);
    const RankPlanes pl = rank_planes(workspace, S, L);
    unsigned int* skeys = skeys_out ? skeys_out : pl.skeys;
    const int rc = egm_sort_pairs_u32(keys, vals, S, L, 0, 32, pl.sort_ws, skeys, pl.svals, s);
    if (rc != EGM_OK) return rc;
    const int ntiles = rank_ntiles(L);
    const dim3 grid(ntiles, S);
    hipLaunchKernelGGL(rank_tile_kernel, grid, dim3(256), 0, (hipStream_t)s, skeys, pl.svals, (int)L, ntiles, pl.tiles);
    EGM_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(rank_scan_kernel, dim3(S), dim3(1024), 0, (hipStream_t)s, pl.tiles, ntiles, pl.pre, pl.totals);
    EGM_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(rank_apply_kernel, grid, dim3(256), 0, (hipStream_t)s, skeys, pl.svals, (int)L, ntiles, pl.pre, pl.totals, tp_out,
                       pl.part_ap, pl.part_u64, pl.part_best);
    EGM_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(rank_finalize_kernel, dim3(1), dim3(1024), 0, (hipStream_t)s, pl.part_ap, pl.part_u64, pl.part_best, pl.totals, ntiles, S,
                       out_u64, out_f64);
    EGM_CHECK_LAUNCH(name);
    return EGM_OK;
}
