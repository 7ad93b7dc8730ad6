// Threshold-swept scores of binary logits:
//   egm_sweep_hist:    hist[n][g][b] += 1 for every kept pixel of sample n with truth g and bin b(s) = #{i : s > cuts[i]}, one streaming
//                      pass over the scores and the targets
//   egm_score_mask_u8: out = s > cut ? v_fg : v_bg, where a threshold chosen from the sweep is applied
// The score s is one fp32 map, or the fp32 difference x[n][c_pos] - x[n][c_neg] of an NCHW tensor (one subtraction, then the same path).
// Every decision is an fp32 `>` against a cut the host made: no transcendental runs here, NaN compares false everywhere (bin 0, never
// foreground), -0.0 and +0.0 are one value.  Counts are exact integers, so the result does not depend on scheduling.
//
// What decides the speed, and what was chosen (measurements: DESIGN.md 6.24):
//   * Segmentation logits are saturated: a wave sees one (truth, bin) key in all 64 lanes, or two or three where its 256 pixels cross
//     an object's edge, and 64 LDS adds to one word serialise.  So a wave first counts two keys whole: the first uncounted lane's key
//     is broadcast, a ballot marks the lanes that hold it, and that one lane adds the ballot's population count; then the same for the
//     lanes that are left.  After two rounds a saturated wave has only the few pixels of the transition left, and a wave of spread
//     scores nearly all of its lanes, on many addresses; either way the rest takes one LDS add per lane.  The rounds are straight-line
//     code over a lane's 17 pixels at once, so their scalar chains (find lane, read lane, ballot, count) overlap.  A wave adds into one
//     of four copies of the histogram, 2 T + 1 words each (8 KiB at T = 256: no per-lane copy is needed to keep the largest table on
//     chip); with four waves per workgroup every wave has a copy of its own.
//   * A workgroup owns one chunk of kSweepChunk pixels of one sample, cut at the scores' 16-byte boundaries: 16-byte score loads, the
//     targets read at whatever alignment falls out (4 bytes per lane for uint8, 16 for fp32); the up to three pixels in front of the
//     first boundary and behind the last whole vector go element by element.  All of a lane's loads are issued first, in front of the
//     table set-up and its barrier, so the chunk's one trip to memory overlaps the tables': at these sizes (20 MB, 3 us at the streaming
//     rate) the kernel is a chain of latencies, not a stream.
//   * The bin is a branch-free binary search of the cut table in LDS, log2(P) compares for P = the power of two >= T; entries past T
//     hold +inf, which no score exceeds, so padding cannot move a bin.  A lane's 17 searches advance in lockstep, so a step's LDS reads
//     are independent and the chain is log2(P) reads long, not 17 log2(P).
//   * The flush adds the four copies and issues at most one 64-bit atomic per non-zero cell and workgroup.
#include "common.h"

namespace {

#ifndef EGM_SWEEP_THREADS
#define EGM_SWEEP_THREADS 256                  // lanes per workgroup (a multiple of 256; A/B builds: DESIGN.md 6.24)
#endif
constexpr int kSweepThreads = EGM_SWEEP_THREADS;
static_assert(kSweepThreads % 256 == 0 && kSweepThreads <= 1024, "the tables are loaded by the first 256 lanes");
constexpr int kSweepVecs = 4;                  // 16-byte score loads per lane
constexpr int kSweepChunk = kSweepThreads * 4 * kSweepVecs;          // pixels per workgroup
constexpr int kSweepMaxT = 256;
constexpr int kSweepCells = 2 * kSweepMaxT + 1;          // [truth][bin] and one cell for dropped pixels that nobody reads

// The pixels [p0, p0 + len) of a sample that one workgroup owns, cut at the 16-byte boundaries of `base` (the first score of the range).
struct SweepSpan {
    int head, nvec, tail0, len;
};
__device__ __forceinline__ SweepSpan sweep_span(const float* base, long long p0, long long HW) {
    SweepSpan s;
    const long long left = HW - p0;
    s.len = left < kSweepChunk ? (int)left : kSweepChunk;
    s.head = (int)(((16 - (reinterpret_cast<uintptr_t>(base) & 15)) & 15) >> 2);
    if (s.head > s.len) s.head = s.len;
    s.nvec = (s.len - s.head) >> 2;
    s.tail0 = s.head + (s.nvec << 2);
    return s;
}
__device__ __forceinline__ float4 load_f4_any(const float* p) {
    float4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}

struct SweepLds {
    float cut[kSweepMaxT];
    unsigned int cnt[4][kSweepCells];
    unsigned short row[256];                   // target byte -> 0 (negative), T (positive), 2 T (dropped)
};

constexpr int kSweepSlots = 4 * kSweepVecs + 1;          // a lane's pixels: its vectors' and one of the chunk's head or tail
constexpr int kSweepPeelRounds = 2;

template <bool TWO, bool TF32>
__global__ __launch_bounds__(kSweepThreads) void sweep_hist_kernel(const float* __restrict__ scores, const void* __restrict__ target,
                                                         const unsigned char* __restrict__ target_cls, const float* __restrict__ cuts, int T,
                                                         int P, int C, int c_pos, int c_neg, long long HW,
                                                         unsigned long long* __restrict__ hist) {
    __shared__ SweepLds L;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long n = blockIdx.y, p0 = (long long)blockIdx.x * kSweepChunk;
    const float* sp = scores + (n * C + (TWO ? c_pos : 0)) * HW + p0;
    const float* sn = scores + (n * C + c_neg) * HW + p0;          // (read only when TWO)
    const float* tf = reinterpret_cast<const float*>(target) + n * HW + p0;               // the chunk's first target, either type
    const unsigned char* tb = reinterpret_cast<const unsigned char*>(target) + n * HW + p0;
    const SweepSpan span = sweep_span(sp, p0, HW);

    // every load of the lane: score s, and row = the target's byte (uint8) or its row 0 / T (fp32); slots nobody owns hold zeros and are not counted
    float s[kSweepSlots];
    int row[kSweepSlots];
    bool valid[kSweepSlots];
#pragma unroll
    for (int k = 0; k < kSweepVecs; ++k) {
        const int v = tid + kSweepThreads * k, e = span.head + (v << 2);
        valid[4 * k] = valid[4 * k + 1] = valid[4 * k + 2] = valid[4 * k + 3] = v < span.nvec;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        unsigned int w = 0u;
        float4 t = a;
        if (v < span.nvec) {
            a = *reinterpret_cast<const float4*>(sp + e);
            if (TWO) {
                const float4 m = load_f4_any(sn + e);
                a.x -= m.x; a.y -= m.y; a.z -= m.z; a.w -= m.w;
            }
            if (TF32) t = load_f4_any(tf + e);
            else __builtin_memcpy(&w, tb + e, 4);
        }
        s[4 * k] = a.x; s[4 * k + 1] = a.y; s[4 * k + 2] = a.z; s[4 * k + 3] = a.w;
        if (TF32) {
            row[4 * k] = t.x > 0.5f ? T : 0; row[4 * k + 1] = t.y > 0.5f ? T : 0;
            row[4 * k + 2] = t.z > 0.5f ? T : 0; row[4 * k + 3] = t.w > 0.5f ? T : 0;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) row[4 * k + j] = (int)((w >> (8 * j)) & 255u);
        }
    }
    {   // the chunk's head (lanes 0..2) and tail (lanes 64..66), at most three pixels each
        constexpr int X = kSweepSlots - 1;
        const int nt = span.len - span.tail0;
        int e = -1;
        if (tid < span.head) e = tid;
        else if (tid >= 64 && tid - 64 < nt) e = span.tail0 + (tid - 64);
        valid[X] = e >= 0;
        s[X] = 0.f;
        row[X] = 0;
        if (e >= 0) {
            s[X] = sp[e];
            if (TWO) s[X] -= sn[e];
            row[X] = TF32 ? (tf[e] > 0.5f ? T : 0) : (int)tb[e];
        }
    }

    // tables and the wave histograms
    if (tid < 256) {
        L.cut[tid] = tid < T ? cuts[tid] : __builtin_inff();
        if (!TF32) {
            const unsigned int c = target_cls[tid];
            L.row[tid] = (unsigned short)(c == 0 ? 0 : (c == 1 ? T : 2 * T));
        }
    }
    for (int cell = tid; cell <= 2 * T; cell += kSweepThreads)     // only the cells this table uses
        L.cnt[0][cell] = L.cnt[1][cell] = L.cnt[2][cell] = L.cnt[3][cell] = 0u;
    __syncthreads();

    // b(s) = #{i : s > cut[i]} for a table that is ascending and ends in +inf: cut[b + step - 1] is read at indices <= P - 2
    int bin[kSweepSlots];
#pragma unroll
    for (int i = 0; i < kSweepSlots; ++i) bin[i] = 0;
    for (int step = P >> 1; step > 0; step >>= 1) {
#pragma unroll
        for (int i = 0; i < kSweepSlots; ++i)
            if (s[i] > L.cut[bin[i] + step - 1]) bin[i] += step;
    }
    unsigned int* cnt = L.cnt[wv & 3];
    int key[kSweepSlots];
    bool mine[kSweepSlots];                                         // the lane's pixel in this slot is still to be counted
#pragma unroll
    for (int i = 0; i < kSweepSlots; ++i) {
        const int r = TF32 ? row[i] : (int)L.row[row[i]];
        // min(bin, T - 1) is a no-op for the tables the launcher admits and keeps a foreign table inside its rows; a dropped pixel's
        // key is the cell 2 T that nobody reads
        key[i] = min(r + min(bin[i], T - 1), 2 * T);
        mine[i] = valid[i];
    }
    // A key at a time, every slot in step (the slots' chains are independent): the first uncounted lane's key is broadcast, a ballot
    // marks the lanes that hold it and that lane adds their number.  No branch depends on the data.
#pragma unroll
    for (int r = 0; r < kSweepPeelRounds; ++r) {
#pragma unroll
        for (int i = 0; i < kSweepSlots; ++i) {
            const unsigned long long todo = __ballot(mine[i]);
            const int leader = todo ? __ffsll((long long)todo) - 1 : 0;
            const int first = __builtin_amdgcn_readlane(key[i], leader);
            const bool hit = mine[i] && key[i] == first;
            const unsigned long long m = __ballot(hit);
            if (hit && lane == leader) atomicAdd(&cnt[first], (unsigned int)__popcll(m));
            mine[i] = mine[i] && !hit;
        }
    }
#pragma unroll
    for (int i = 0; i < kSweepSlots; ++i)
        if (mine[i]) atomicAdd(&cnt[key[i]], 1u);
    __syncthreads();
    // flush: a cell's four copies summed (at most kSweepChunk, far from 2^32), one 64-bit atomic per non-zero cell
    unsigned long long* h = hist + n * 2 * T;
    for (int cell = tid; cell < 2 * T; cell += kSweepThreads) {
        const unsigned int v = L.cnt[0][cell] + L.cnt[1][cell] + L.cnt[2][cell] + L.cnt[3][cell];
        if (v) atomicAdd(&h[cell], (unsigned long long)v);
    }
}

template <bool TWO>
__global__ __launch_bounds__(kSweepThreads) void score_mask_u8_kernel(const float* __restrict__ scores, int C, int c_pos, int c_neg, long long HW,
                                                            float cut, unsigned int v_bg, unsigned int v_fg, unsigned char* __restrict__ out) {
    const int tid = threadIdx.x;
    const long long n = blockIdx.y, p0 = (long long)blockIdx.x * kSweepChunk;
    const float* sp = scores + (n * C + (TWO ? c_pos : 0)) * HW + p0;
    const float* sn = scores + (n * C + c_neg) * HW + p0;
    unsigned char* op = out + n * HW + p0;
    const SweepSpan sp_ = sweep_span(sp, p0, HW);
#pragma unroll
    for (int k = 0; k < kSweepVecs; ++k) {
        const int v = tid + kSweepThreads * k;
        if (v < sp_.nvec) {
            const int e = sp_.head + (v << 2);
            float4 s = *reinterpret_cast<const float4*>(sp + e);
            if (TWO) {
                const float4 m = load_f4_any(sn + e);
                s.x -= m.x; s.y -= m.y; s.z -= m.z; s.w -= m.w;
            }
            const unsigned int w = (s.x > cut ? v_fg : v_bg) | ((s.y > cut ? v_fg : v_bg) << 8) | ((s.z > cut ? v_fg : v_bg) << 16) |
                                   ((s.w > cut ? v_fg : v_bg) << 24);
            __builtin_memcpy(op + e, &w, 4);
        }
    }
    const int nt = sp_.len - sp_.tail0;
    int e = -1;
    if (tid < sp_.head) e = tid;
    else if (tid >= 64 && tid - 64 < nt) e = sp_.tail0 + (tid - 64);
    if (e >= 0) {
        float s = sp[e];
        if (TWO) s -= sn[e];
        op[e] = (unsigned char)(s > cut ? v_fg : v_bg);
    }
}

// The shapes both entry points admit.  A workgroup counts at most kSweepChunk pixels in 32 bits, so no partial can wrap at any size;
// what bounds the sizes is the grid: chunks of a sample in x (HW <= 2^40 keeps it below 2^31), samples in y (N <= 65535).
int sweep_shape_check(const char* who, const float* scores, int N, int C, int c_pos, int c_neg, long long HW) {
    EGM_REQUIRE(scores, "%s: null pointer", who);
    EGM_REQUIRE(N >= 1 && N <= 65535, "%s: %d samples, between 1 and 65535 are supported", who, N);
    EGM_REQUIRE(HW >= 1 && HW <= (1ll << 40), "%s: %lld pixels per sample, between 1 and 2^40 are supported", who, HW);
    EGM_REQUIRE(C >= 1 && C <= 65535, "%s: %d channels, between 1 and 65535 are supported", who, C);
    if (C > 1)
        EGM_REQUIRE(c_pos >= 0 && c_pos < C && c_neg >= 0 && c_neg < C && c_pos != c_neg,
                    "%s: channels (%d, %d) must be two different channels of the %d", who, c_pos, c_neg, C);
    return EGM_OK;
}
dim3 sweep_grid(int N, long long HW) { return dim3((unsigned)((HW + kSweepChunk - 1) / kSweepChunk), (unsigned)N); }

}  // namespace

extern "C" long long egm_sweep_chunk(void) { return kSweepChunk; }

extern "C" int egm_sweep_hist(const float* scores, int N, int C, int c_pos, int c_neg, long long HW, const void* target, int target_f32,
                              const unsigned char* target_cls, const float* cuts_host, const float* cuts_dev, int T,
                              unsigned long long* hist, egm_stream_t s) {
    EGM_REQUIRE(scores && target && cuts_host && cuts_dev && hist && (target_f32 || target_cls), "sweep_hist: null pointer");
    EGM_REQUIRE(T >= 2 && T <= kSweepMaxT, "sweep_hist: %d thresholds, between 2 and %d are supported", T, kSweepMaxT);
    for (int i = 0; i < T; ++i) {
        EGM_REQUIRE(cuts_host[i] == cuts_host[i], "sweep_hist: cut %d is NaN", i);
        EGM_REQUIRE(i == 0 || cuts_host[i - 1] < cuts_host[i], "sweep_hist: the cuts must ascend strictly (cut %d = %g after %g)", i,
                    (double)cuts_host[i], (double)cuts_host[i - 1]);
    }
    EGM_REQUIRE(cuts_host[T - 1] == __builtin_inff(), "sweep_hist: the last cut must be +inf (threshold 1), so that the bins are 0..%d", T - 1);
    if (sweep_shape_check("sweep_hist", scores, N, C, c_pos, c_neg, HW) != EGM_OK) return EGM_ERR_ARG;
    int P = 2;
    while (P < T) P <<= 1;
    const dim3 grid = sweep_grid(N, HW);
#define EGM_SWEEP_LAUNCH(TWO, TF32) \
    hipLaunchKernelGGL((sweep_hist_kernel<TWO, TF32>), grid, dim3(kSweepThreads), 0, (hipStream_t)s, scores, target, target_cls, cuts_dev, T, P, C, c_pos, \
                       c_neg, HW, hist)
    if (C > 1) { if (target_f32) EGM_SWEEP_LAUNCH(true, true); else EGM_SWEEP_LAUNCH(true, false); }
    else       { if (target_f32) EGM_SWEEP_LAUNCH(false, true); else EGM_SWEEP_LAUNCH(false, false); }
#undef EGM_SWEEP_LAUNCH
    EGM_CHECK_LAUNCH("sweep_hist");
    return EGM_OK;
}

extern "C" int egm_score_mask_u8(const float* scores, int N, int C, int c_pos, int c_neg, long long HW, float cut, int v_bg, int v_fg,
                                 unsigned char* out, egm_stream_t s) {
    EGM_REQUIRE(scores && out, "score_mask_u8: null pointer");
    EGM_REQUIRE(cut == cut, "score_mask_u8: the cut is NaN");
    EGM_REQUIRE(v_bg >= 0 && v_bg <= 255 && v_fg >= 0 && v_fg <= 255, "score_mask_u8: mask values (%d, %d) must be bytes", v_bg, v_fg);
    if (sweep_shape_check("score_mask_u8", scores, N, C, c_pos, c_neg, HW) != EGM_OK) return EGM_ERR_ARG;
    const dim3 grid = sweep_grid(N, HW);
    if (C > 1)
        hipLaunchKernelGGL(score_mask_u8_kernel<true>, grid, dim3(kSweepThreads), 0, (hipStream_t)s, scores, C, c_pos, c_neg, HW, cut, (unsigned)v_bg,
                           (unsigned)v_fg, out);
    else
        hipLaunchKernelGGL(score_mask_u8_kernel<false>, grid, dim3(kSweepThreads), 0, (hipStream_t)s, scores, C, c_pos, c_neg, HW, cut, (unsigned)v_bg,
                           (unsigned)v_fg, out);
    EGM_CHECK_LAUNCH("score_mask_u8");
    return EGM_OK;
}
