// A stable LSD radix sort of (uint32 key, uint32 value) pairs on the device: S independent segments of equal length L,
// ascending on the key bits [begin_bit, end_bit), equal keys in their input order.  The primitive under the Lovasz-Softmax loss
// (lovasz.hip), with entry points of its own:
//   egm_sort_pairs_workspace   bytes of the ping-pong planes and the count table
//   egm_sort_pairs_u32         kSortBits bits per pass, three launches per pass whatever the content, S and L
// A pass over the digit d = (key >> shift) & mask:
//   hist     one workgroup per tile of kSortTile elements and segment: the tile's digit histogram (integer LDS atomics: counts are exact
//            whatever the order) -> table[segment][digit][tile]
//   scan     one wave per (segment, digit): the exclusive prefix sum of the digit's tile counts in place, kScanTiles tiles per sweep,
//            the carry in a register, and the digit's total -> totals[segment][digit].  The prefix over the digits is left to the
//            scatter: 256 totals, one per thread.  The elements of the segment with a smaller digit + those with digit d in the tiles
//            before t = where tile t's first element of digit d goes
//   scatter  one workgroup per tile and segment.  The tile's elements are taken in the order (wave w, round i, lane l) = tile element
//            w * 512 + i * 64 + l.  In a round a lane finds the lanes of its wave with its digit from kSortBits __ballot masks (64 bits):
//            its rank among them is the number of lower such lanes, on top of the wave's running count of that digit, which lives in LDS
//            (one row of 256 counters per wave, read by the lanes of a match and advanced by its highest lane; a wave's LDS operations
//            execute in program order, no other wave touches the row).  After the rounds a row holds the wave's histogram; thread d adds
//            the digits before d, the table's entry and the rows of the waves before: waves taken in order.  destination = that base + the rank.
// The rank depends on the element's position and the digits alone, never on the order in which anything executes: two runs give the
// same bits.  No workgroup waits for another (no look-back, no flags, no grid barrier; launches are ordered by the stream); every loop
// is bounded by the arguments; no atomics on global memory.  A destination is below L by construction (the table is the histogram of
// the very keys the scatter reads); the store is guarded all the same.
#include "common.h"

namespace {

constexpr int kSortBits = 8;                   // digit width
constexpr int kSortRadix = 1 << kSortBits;
constexpr int kSortThreads = 256;              // = kSortRadix: thread d owns digit d
constexpr int kSortWaves = kSortThreads / 64;
constexpr int kSortItems = 8;                  // rounds: elements per lane
constexpr int kSortTile = kSortThreads * kSortItems;          // 2048 (tests/test_gpu_sort.py restates it)
constexpr int kScanTiles = 64;                 // the table scan: one wave per (segment, digit), a tile count per lane and sweep
static_assert(kSortThreads == kSortRadix, "one thread per digit");

__device__ __forceinline__ unsigned int sort_digit(unsigned int key, int shift, unsigned int mask) { return (key >> shift) & mask; }

// tiles per segment as the table stores them: padded to a multiple of 4, so that every row starts at a 16-byte boundary
inline long long sort_tile_pitch(long long L) { return ((L + kSortTile - 1) / kSortTile + 3) / 4 * 4; }

__global__ __launch_bounds__(kSortThreads) void sort_hist_kernel(const unsigned int* __restrict__ keys, int L, int tp, int shift,
                                                                 unsigned int mask, unsigned int* __restrict__ table) {
    __shared__ unsigned int hist[kSortRadix];
    const int tile = blockIdx.x, seg = blockIdx.y;
    hist[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned int* k = keys + (long long)seg * L;
    const long long base = (long long)tile * kSortTile + threadIdx.x;      // (a padding tile starts at or behind L: it counts nothing)
#pragma unroll
    for (int i = 0; i < kSortItems; ++i) {
        const long long idx = base + i * kSortThreads;
        if (idx < L) atomicAdd(&hist[sort_digit(k[idx], shift, mask)], 1u);
    }
    __syncthreads();
    table[((long long)seg * kSortRadix + threadIdx.x) * tp + tile] = hist[threadIdx.x];
}

// inclusive scan of x over the 64 lanes of a wave
__device__ __forceinline__ unsigned int sort_wave_scan(unsigned int x, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    return x;
}

// one wave per row (segment, digit) of tp tile counts: the row's exclusive prefix in place, its total -> totals[row]
__global__ __launch_bounds__(256) void sort_scan_kernel(unsigned int* __restrict__ table, int tp, long long rows,
                                                        unsigned int* __restrict__ totals) {
    const long long row = blockIdx.x * 4LL + (threadIdx.x >> 6);
    if (row >= rows) return;                                   // (a whole wave; the kernel has no barrier)
    const int lane = threadIdx.x & 63;
    unsigned int* t = table + row * tp;
    unsigned int carry = 0u;
    for (int base = 0; base < tp; base += kScanTiles) {
        const int at = base + lane;
        const unsigned int own = at < tp ? t[at] : 0u;
        const unsigned int x = sort_wave_scan(own, lane);
        if (at < tp) t[at] = carry + x - own;
        carry += __shfl(x, 63, 64);
    }
    if (lane == 0) totals[row] = carry;
}

__global__ __launch_bounds__(kSortThreads) void sort_scatter_kernel(const unsigned int* __restrict__ keys,
                                                                    const unsigned int* __restrict__ vals, int L, int tp, int shift,
                                                                    unsigned int mask, const unsigned int* __restrict__ table,
                                                                    const unsigned int* __restrict__ totals,
                                                                    unsigned int* __restrict__ keys_out,
                                                                    unsigned int* __restrict__ vals_out) {
    __shared__ unsigned int cnt_s[kSortWaves][kSortRadix];
    __shared__ unsigned int dsum[kSortWaves];
    volatile unsigned int (*cnt)[kSortRadix] = cnt_s;          // every access is a real LDS operation, in program order
    const int tile = blockIdx.x, seg = blockIdx.y;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int w = 0; w < kSortWaves; ++w) cnt[w][threadIdx.x] = 0u;
    // thread d: the elements of the segment with a digit below d, from the 256 totals
    const unsigned int dtot = totals[(long long)seg * kSortRadix + threadIdx.x];
    const unsigned int dinc = sort_wave_scan(dtot, lane);
    if (lane == 63) dsum[wv] = dinc;
    __syncthreads();
    unsigned int dbase = dinc - dtot;
#pragma unroll
    for (int w = 0; w < kSortWaves; ++w) dbase += w < wv ? dsum[w] : 0u;
    const long long off = (long long)seg * L;
    const long long base = (long long)tile * kSortTile + wv * (64 * kSortItems) + lane;
    unsigned int k[kSortItems], v[kSortItems], rank[kSortItems];
#pragma unroll
    for (int i = 0; i < kSortItems; ++i) {
        const long long idx = base + i * 64;
        k[i] = idx < L ? keys[off + idx] : 0u;
        v[i] = idx < L ? vals[off + idx] : 0u;
    }
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int i = 0; i < kSortItems; ++i) {
        const bool ok = base + i * 64 < L;
        const unsigned int d = sort_digit(k[i], shift, mask);
        unsigned long long same = __ballot(ok);                // the lanes of this round that hold an element with my digit
#pragma unroll
        for (int b = 0; b < kSortBits; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long has = __ballot(bit);
            same &= bit ? has : ~has;
        }
        const unsigned int before = ok ? cnt[wv][d] : 0u;
        __builtin_amdgcn_wave_barrier();
        rank[i] = before + (unsigned int)__popcll(same & below);
        if (ok && (same >> lane) == 1ull) cnt[wv][d] = before + (unsigned int)__popcll(same);      // the highest lane of the match
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {                                                          // thread d: the table's entry, then the waves in order
        unsigned int run = dbase + table[((long long)seg * kSortRadix + threadIdx.x) * tp + tile];
#pragma unroll
        for (int w = 0; w < kSortWaves; ++w) {
            const unsigned int c = cnt[w][threadIdx.x];
            cnt[w][threadIdx.x] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kSortItems; ++i) {
        if (base + i * 64 >= L) continue;
        const unsigned int pos = cnt[wv][sort_digit(k[i], shift, mask)] + rank[i];
        if (pos < (unsigned int)L) {
            keys_out[off + pos] = k[i];
            vals_out[off + pos] = v[i];
        }
    }
}

inline int sort_shape_check(const char* name, int S, long long L) {
    EGM_REQUIRE(S >= 1 && S <= 65535 && L >= 1, "%s: %d segments of %lld elements (1..65535 segments of at least one)", name, S, L);
    EGM_REQUIRE(L < (1ll << 31), "%s: segments of %lld elements, L must stay below 2^31", name, L);
    return EGM_OK;
}

}  // namespace

extern "C" long long egm_sort_pairs_workspace(int S, long long L) {
    if (sort_shape_check("sort_pairs_workspace", S, L) != EGM_OK) return EGM_ERR_ARG;
    const long long plane = ((long long)S * L * 4 + 15) / 16 * 16;
    return 2 * plane + (long long)S * kSortRadix * (sort_tile_pitch(L) + 1) * 4 + 16;       // (+16: the planes start at a 16-byte boundary)
}

extern "C" int egm_sort_pairs_u32(const unsigned int* keys, const unsigned int* vals, int S, long long L, int begin_bit, int end_bit,
                                  void* workspace, unsigned int* keys_out, unsigned int* vals_out, egm_stream_t s) {
    const char* name = "sort_pairs_u32";
    if (sort_shape_check(name, S, L) != EGM_OK) return EGM_ERR_ARG;
    EGM_REQUIRE(keys && vals && workspace && keys_out && vals_out, "%s: null pointer", name);
    EGM_REQUIRE(0 <= begin_bit && begin_bit < end_bit && end_bit <= 32, "%s: bits [%d, %d) must be a non-empty range inside [0, 32)", name,
                begin_bit, end_bit);
    EGM_REQUIRE(keys != keys_out && vals != vals_out, "%s: the outputs must not be the inputs", name);
    EGM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "%s: the workspace must be 4-byte aligned", name);
    unsigned char* w = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(workspace) + 15) & ~(uintptr_t)15);
    const long long plane = ((long long)S * L * 4 + 15) / 16 * 16;
    unsigned int* tmp_k = reinterpret_cast<unsigned int*>(w);
    unsigned int* tmp_v = reinterpret_cast<unsigned int*>(w + plane);
    unsigned int* table = reinterpret_cast<unsigned int*>(w + 2 * plane);
    const int tp = (int)sort_tile_pitch(L);
    unsigned int* totals = table + (long long)S * kSortRadix * tp;
    const long long rows = (long long)S * kSortRadix;
    const int passes = (end_bit - begin_bit + kSortBits - 1) / kSortBits;
    const unsigned int* src_k = keys;
    const unsigned int* src_v = vals;
    const dim3 grid(tp, S), block(kSortThreads);
    for (int p = 0; p < passes; ++p) {                         // the last pass lands in the outputs
        const int shift = begin_bit + p * kSortBits;
        const int bits = end_bit - shift < kSortBits ? end_bit - shift : kSortBits;
        const unsigned int mask = (1u << bits) - 1u;
        const bool to_out = (passes - 1 - p) % 2 == 0;
        unsigned int* dst_k = to_out ? keys_out : tmp_k;
        unsigned int* dst_v = to_out ? vals_out : tmp_v;
        hipLaunchKernelGGL(sort_hist_kernel, grid, block, 0, (hipStream_t)s, src_k, (int)L, tp, shift, mask, table);
        EGM_CHECK_LAUNCH("sort_pairs_u32 (hist)");
        hipLaunchKernelGGL(sort_scan_kernel, dim3((unsigned)(rows / 4)), dim3(256), 0, (hipStream_t)s, table, tp, rows, totals);
        EGM_CHECK_LAUNCH("sort_pairs_u32 (scan)");
        hipLaunchKernelGGL(sort_scatter_kernel, grid, block, 0, (hipStream_t)s, src_k, src_v, (int)L, tp, shift, mask, table, totals, dst_k, dst_v);
        EGM_CHECK_LAUNCH("sort_pairs_u32 (scatter)");
        src_k = dst_k;
        src_v = dst_v;
    }
    return EGM_OK;
}
