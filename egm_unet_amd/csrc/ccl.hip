// Connected-component labelling of uint8 class maps and the mask clean-up built on it.
//   egm_ccl_label_u8:  canonical labels (raster index of the component's first pixel) and areas, foreground and background alike
//   egm_mask_clean_u8: stage 1 fills small enclosed background components, stage 2 drops small foreground components and / or keeps
//                      the largest one per class; the last pass writes the photo-size mask through the nearest-neighbour tables.
//
// Labelling is three launches whatever the content (union-find of csrc/ccl_core.h):
//   tile    a workgroup labels a 16 x 64 tile in LDS (links to the left / up / diagonal neighbours inside the tile), then writes every
//           pixel's tile root as a global raster index; the pixels of a tile component are counted in LDS and the count (with the
//           border bit) is left in the area word of the tile root, 0 in every other word
//   seam    the pixels on a tile's first row, first and last column link to their backward neighbours in other tiles with atomicMin on
//           the global array
//   flatten every pixel walks to its root and stores it; a tile root that is not the root hands its count over with one atomicAdd (and
//           an atomicOr of the border bit), so the largest component costs one atomic per tile it covers.  (A first version counted in
//           this pass, one atomicAdd per run of equal roots in a wave: 6.6 k adds to the background's one word made it 444 us.)
// No workgroup ever waits for another: separate launches are the only ordering between workgroups, and every loop has a trip bound
// (ccl_core.h); a loop that runs out ORs a bit into the status word at the start of the workspace.
#include "common.h"
#include "ccl_core.h"

namespace {

struct GlobalForest {            // one image's labels in global memory
    int* p;
    __device__ int load(int i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ int fetch_min(int i, int v) const { return atomicMin(p + i, v); }
    __device__ void store(int i, int v) const { p[i] = v; }
};
struct GlobalAreas {             // one image's area words
    int* p;
    __device__ int load(int i) const { return p[i]; }
    __device__ void store(int i, int v) const { p[i] = v; }
    __device__ void add(int i, int v) const { atomicAdd(p + i, v); }
    __device__ void or_bits(int i, int v) const { atomicOr(p + i, v); }
};
struct TileForest {              // one tile's labels in LDS
    int* p;
    __device__ int load(int i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ int fetch_min(int i, int v) const { return atomicMin(p + i, v); }
    __device__ void store(int i, int v) const { p[i] = v; }
};

// params (device): {min_area, keep_largest, max_hole}.  A labelling pass of a stage that is switched off returns at once, so the
// launches of a captured graph stay the same while the numbers change.  params == nullptr: egm_ccl_label_u8, always on.
__device__ __forceinline__ bool stage_off(const int* __restrict__ params, int stage) {
    if (!params) return false;
    return stage == 1 ? !ccl_stage1_on(params[2]) : !ccl_stage2_on(params[0], params[1]);
}

__global__ __launch_bounds__(256) void ccl_tile_kernel(const unsigned char* __restrict__ cls, int H, int W, int tilesX, int tilesY,
                                                       long long tiles, int connectivity, int* __restrict__ labels, int* __restrict__ areas,
                                                       int border, const int* __restrict__ params, int stage, int* __restrict__ status) {
    if (stage_off(params, stage)) return;
    __shared__ int lab[kCclTilePix];
    __shared__ short val[kCclTilePix];
    __shared__ int cnt[kCclTilePix];
    int st = 0;
    for (long long b = blockIdx.x; b < tiles; b += gridDim.x) {                  // (one tile per workgroup below kMaxGrid tiles)
    const int tix = (int)(b % tilesX), tiy = (int)((b / tilesX) % tilesY), n = (int)(b / tilesX / tilesY);
    const int y0 = tiy * kCclTileH, x0 = tix * kCclTileW;
    const long long base = (long long)n * H * W;
#pragma unroll
    for (int k = 0; k < kCclTilePix / 256; ++k) {
        const int l = threadIdx.x + k * 256, y = y0 + l / kCclTileW, x = x0 + l % kCclTileW;
        val[l] = (y < H && x < W) ? (short)cls[base + y * W + x] : (short)-1;
        lab[l] = l;
        cnt[l] = 0;
    }
    __syncthreads();
    const TileForest f{lab};
#pragma unroll
    for (int k = 0; k < kCclTilePix / 256; ++k) ccl_link_tile_pixel(f, val, threadIdx.x + k * 256, connectivity, st);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kCclTilePix / 256; ++k) {
        const int l = threadIdx.x + k * 256, y = y0 + l / kCclTileW, x = x0 + l % kCclTileW;
        if (y < H && x < W) {
            const int root = ccl_find(f, l, kCclTilePix, st);
            labels[base + y * W + x] = (y0 + root / kCclTileW) * W + x0 + root % kCclTileW;
            if (areas) {
                atomicAdd(&cnt[root], 1);
                if (border && ccl_on_border(y, x, H, W)) atomicOr(&cnt[root], kCclBorder);
            }
        }
    }
    __syncthreads();
    if (areas) {
#pragma unroll
        for (int k = 0; k < kCclTilePix / 256; ++k) {
            const int l = threadIdx.x + k * 256, y = y0 + l / kCclTileW, x = x0 + l % kCclTileW;
            if (y < H && x < W) areas[base + y * W + x] = cnt[l];              // the tile component's count at its tile root, 0 elsewhere
        }
    }
    __syncthreads();
    }
    if (st) atomicOr(status, st);
}

__global__ __launch_bounds__(256) void ccl_seam_kernel(const unsigned char* __restrict__ cls, int H, int W, int chunks, long long blocks,
                                                       int connectivity, int* labels, const int* __restrict__ params, int stage,
                                                       int* __restrict__ status) {
    if (stage_off(params, stage)) return;
    int st = 0;
    for (long long b = blockIdx.x; b < blocks; b += gridDim.x) {
        const long long n = b / chunks;
        const int i = (int)(b - n * chunks) * 256 + threadIdx.x;
        if (i >= H * W) continue;
        const int y = i / W, x = i - y * W;
        if (!ccl_on_seam(y, x)) continue;
        const long long base = n * H * W;
        ccl_link_seam_pixel(GlobalForest{labels + base}, cls + base, H, W, y, x, connectivity, st);
    }
    if (st) atomicOr(status, st);
}

__global__ __launch_bounds__(256) void ccl_flatten_kernel(int H, int W, int chunks, long long blocks, int* labels, int* areas,
                                                          const int* __restrict__ params, int stage, int* __restrict__ status) {
    if (stage_off(params, stage)) return;
    int st = 0;
    for (long long b = blockIdx.x; b < blocks; b += gridDim.x) {
        const long long n = b / chunks, base = n * H * W;
        const int i = (int)(b - n * chunks) * 256 + threadIdx.x;
        if (i >= H * W) continue;
        const GlobalAreas a{areas + base};
        ccl_flatten_pixel(GlobalForest{labels + base}, areas ? &a : nullptr, i, H * W, st);
    }
    if (st) atomicOr(status, st);
}

// Stage 1 applied: cls1 = cls with the enclosed background components of at most max_hole pixels set to the byte left of their first
// pixel (a foreground pixel of the same row: the component touches no border, and the dual connectivity would have joined a background
// one).  With the stage off a copy.  Also zeroes the per-class maxima of stage 2.
__global__ __launch_bounds__(256) void clean_fill_kernel(const unsigned char* __restrict__ cls, long long total, int HW, const int* __restrict__ labels,
                                                         const int* __restrict__ areas, const int* __restrict__ params,
                                                         unsigned char* __restrict__ cls1, unsigned long long* __restrict__ best, int nbest) {
    const int max_hole = params[2];
    const long long stride = (long long)gridDim.x * 256, t0 = blockIdx.x * 256LL + threadIdx.x;
    for (long long j = t0; j < nbest; j += stride) best[j] = 0ull;
    for (long long i = t0; i < total; i += stride) {
        int v = cls[i];
        if (v == 0 && ccl_stage1_on(max_hole)) {
            const long long base = egm_udiv(i, HW) * HW;
            const int root = labels[i];
            if (root > 0 && root < HW && ccl_hole_fills(areas[base + root], max_hole)) v = cls[base + root - 1];
        }
        cls1[i] = (unsigned char)v;
    }
}

// Stage 2, per-class maxima: every foreground root offers its (area, -first index) key.
__global__ __launch_bounds__(256) void clean_rank_kernel(const unsigned char* __restrict__ cls1, long long total, int HW, const int* __restrict__ labels,
                                                         const int* __restrict__ areas, const int* __restrict__ params,
                                                         unsigned long long* __restrict__ best) {
    if (!params[1]) return;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int v = cls1[i];
        if (v == 0) continue;
        const long long n = egm_udiv(i, HW);
        const int p = (int)(i - n * HW);
        if (labels[i] == p) atomicMax(best + n * 256 + v, ccl_rank_key(areas[i] & kCclAreaMask, p));
    }
}

struct CleanRule {
    const unsigned char* cls1; const int* labels; const int* areas; const unsigned long long* best;
    int HW, min_area, keep_largest; bool on;
    __device__ __forceinline__ int at(int n, int p) const {          // the cleaned class of pixel p of image n
        const long long i = (long long)n * HW + p;
        const int v = cls1[i];
        if (v == 0 || !on) return v;
        const int root = min(max(labels[i], 0), HW - 1);
        const int area = areas[(long long)n * HW + root] & kCclAreaMask;
        return ccl_component_kept(area, root, min_area, keep_largest, best[n * 256 + v]) ? v : 0;
    }
};

// The last pass.  Items [0, groups): 16-byte groups of the photo-size rows, cut as in ensemble_mask_u8_kernel (group 0 of a row is its
// unaligned head, the others are one aligned 16-byte store each), out = lut[cleaned[yidx[y]][xidx[x]]]; the rule runs once per run of
// equal xidx.  Items [groups, groups + N*H*W): the cleaned map itself, when asked for.
__global__ __launch_bounds__(256) void clean_apply_kernel(CleanRule rule_in, const int* __restrict__ params, int N, int H, int W,
                                                          unsigned char* __restrict__ out_cls, const int* __restrict__ yidx,
                                                          const int* __restrict__ xidx, const unsigned char* __restrict__ lut,
                                                          unsigned char* __restrict__ out, int H0, int W0, long long groups, long long total) {
    CleanRule rule = rule_in;
    rule.min_area = params[0]; rule.keep_largest = params[1]; rule.on = ccl_stage2_on(params[0], params[1]);
    const int gpr = ((W0 + 15) >> 4) + 1;
    for (long long it = blockIdx.x * 256LL + threadIdx.x; it < total; it += (long long)gridDim.x * 256) {
        if (it >= groups) {
            const long long i = it - groups, n = egm_udiv(i, rule.HW);
            out_cls[i] = (unsigned char)rule.at((int)n, (int)(i - n * rule.HW));
            continue;
        }
        long long r; int g; egm_divmod(it, gpr, r, g);
        long long nn; int y; egm_divmod(r, H0, nn, y);
        const int n = (int)nn;
        unsigned char* rowp = out + ((long long)n * H0 + y) * W0;
        const int head = min(W0, (int)((16 - (reinterpret_cast<uintptr_t>(rowp) & 15)) & 15));
        const int x0 = g == 0 ? 0 : head + (g - 1) * 16, x1 = g == 0 ? head : min(W0, x0 + 16);
        if (x0 >= x1) continue;
        const int uy = min(max(yidx[y], 0), H - 1);
        unsigned long long lo = 0ull, hi = 0ull;
        int last = -1; unsigned long long cur = 0ull;
        for (int k = 0; k < x1 - x0; ++k) {
            const int ux = min(max(xidx[x0 + k], 0), W - 1);
            if (ux != last) {
                const int v = rule.at(n, uy * W + ux);
                cur = lut ? (unsigned long long)lut[v & 255] : (unsigned long long)(v & 255);
                last = ux;
            }
            if (k < 8) lo |= cur << (k * 8); else hi |= cur << ((k - 8) * 8);
        }
        unsigned char* dst = rowp + x0;
        if (g > 0 && x1 - x0 == 16) {
            *reinterpret_cast<uint4*>(dst) = make_uint4((unsigned int)lo, (unsigned int)(lo >> 32), (unsigned int)hi, (unsigned int)(hi >> 32));
        } else {
            for (int k = 0; k < x1 - x0; ++k) dst[k] = (unsigned char)((k < 8 ? lo >> (k * 8) : hi >> ((k - 8) * 8)) & 255ull);
        }
    }
}

constexpr long long kStatusBytes = 256;              // the status word and padding, in front of everything else

struct Shape { int tilesX, tilesY, chunks; long long tiles, blocks; };

// One workgroup per tile / per 256 pixels up to kMaxGrid workgroups, a uniform loop beyond (a launch's thread count must fit 32 bits).
constexpr long long kMaxGrid = 1ll << 22;
unsigned grid_of(long long items) { return (unsigned)(items < kMaxGrid ? items : kMaxGrid); }

// The checks both compute entry points share.
int check_shape(const char* who, int N, int H, int W, int connectivity, Shape& sh) {
    EGM_REQUIRE(N > 0 && H > 0 && W > 0, "%s: bad shape", who);
    EGM_REQUIRE(connectivity == 4 || connectivity == 8, "%s: connectivity %d (4 or 8)", who, connectivity);
    EGM_REQUIRE((long long)H * W <= kCclMaxPixels, "%s: %d x %d pixels, at most 2^30 per image are supported", who, H, W);
    sh.tilesX = egm_cdiv(W, kCclTileW); sh.tilesY = egm_cdiv(H, kCclTileH); sh.chunks = egm_cdiv((long long)H * W, 256);
    sh.tiles = (long long)N * sh.tilesX * sh.tilesY; sh.blocks = (long long)N * sh.chunks;
    EGM_REQUIRE((long long)N * H * W < (1ll << 40), "%s: batch of %d images of %d x %d is too large", who, N, H, W);
    return EGM_OK;
}

int label_launch(const char* who, const unsigned char* cls, int H, int W, int connectivity, const Shape& sh, int* labels, int* areas, int border,
                 const int* params, int stage, int* status, hipStream_t s) {
    hipLaunchKernelGGL(ccl_tile_kernel, dim3(grid_of(sh.tiles)), dim3(256), 0, s, cls, H, W, sh.tilesX, sh.tilesY, sh.tiles, connectivity, labels, areas,
                       border, params, stage, status);
    EGM_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(ccl_seam_kernel, dim3(grid_of(sh.blocks)), dim3(256), 0, s, cls, H, W, sh.chunks, sh.blocks, connectivity, labels, params, stage, status);
    EGM_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(ccl_flatten_kernel, dim3(grid_of(sh.blocks)), dim3(256), 0, s, H, W, sh.chunks, sh.blocks, labels, areas, params, stage, status);
    EGM_CHECK_LAUNCH(who);
    return EGM_OK;
}

long long pad16(long long v) { return (v + 15) & ~15ll; }

}  // namespace

extern "C" long long egm_ccl_workspace(int N, int H, int W) {
    Shape sh;
    const int rc = check_shape("ccl_workspace", N, H, W, 8, sh);
    if (rc != EGM_OK) return rc;
    const long long px = (long long)N * H * W;
    return kStatusBytes + (long long)N * 256 * 8 + 2 * pad16(px * 4) + pad16(px);
}

extern "C" int egm_ccl_label_u8(const unsigned char* cls, int N, int H, int W, int connectivity, int* labels, int* areas, void* workspace,
                                egm_stream_t s) {
    EGM_REQUIRE(cls && labels && workspace, "ccl_label_u8: null pointer");
    Shape sh;
    const int rc = check_shape("ccl_label_u8", N, H, W, connectivity, sh);
    if (rc != EGM_OK) return rc;
    return label_launch("ccl_label_u8", cls, H, W, connectivity, sh, labels, areas, 0, nullptr, 0, (int*)workspace, (hipStream_t)s);
}

extern "C" int egm_mask_clean_u8(const unsigned char* cls, int N, int H, int W, int connectivity, const int* params_dev, void* workspace,
                                 unsigned char* out_cls, const int* yidx, const int* xidx, const unsigned char* lut, unsigned char* out, int H0,
                                 int W0, egm_stream_t s) {
    EGM_REQUIRE(cls && params_dev && workspace, "mask_clean_u8: null pointer");
    EGM_REQUIRE(out_cls || out, "mask_clean_u8: null pointer (out_cls and out)");
    EGM_REQUIRE(!out || (yidx && xidx), "mask_clean_u8: null pointer (yidx / xidx with out)");
    Shape sh;
    const int rc = check_shape("mask_clean_u8", N, H, W, connectivity, sh);
    if (rc != EGM_OK) return rc;
    EGM_REQUIRE(!out || (H0 > 0 && W0 > 0), "mask_clean_u8: bad output shape");
    const int HW = H * W;
    const long long px = (long long)N * HW;
    char* ws = (char*)workspace;
    int* status = (int*)ws;
    unsigned long long* best = (unsigned long long*)(ws + kStatusBytes);
    int* labels = (int*)(ws + kStatusBytes + (long long)N * 256 * 8);
    int* areas = (int*)((char*)labels + pad16(px * 4));
    unsigned char* cls1 = (unsigned char*)areas + pad16(px * 4);
    hipStream_t st = (hipStream_t)s;
    const int stream_grid = (int)((px + 255) / 256 > 8192 ? 8192 : (px + 255) / 256);
    int r = label_launch("mask_clean_u8", cls, H, W, connectivity, sh, labels, areas, 1, params_dev, 1, status, st);
    if (r != EGM_OK) return r;
    hipLaunchKernelGGL(clean_fill_kernel, dim3(stream_grid), dim3(256), 0, st, cls, px, HW, (const int*)labels, (const int*)areas, params_dev, cls1,
                       best, N * 256);
    EGM_CHECK_LAUNCH("mask_clean_u8");
    r = label_launch("mask_clean_u8", cls1, H, W, connectivity, sh, labels, areas, 0, params_dev, 2, status, st);
    if (r != EGM_OK) return r;
    hipLaunchKernelGGL(clean_rank_kernel, dim3(stream_grid), dim3(256), 0, st, (const unsigned char*)cls1, px, HW, (const int*)labels,
                       (const int*)areas, params_dev, best);
    EGM_CHECK_LAUNCH("mask_clean_u8");
    const long long groups = out ? (long long)N * H0 * ((W0 + 15) / 16 + 1) : 0;
    const long long total = groups + (out_cls ? px : 0);
    long long grid = (total + 255) / 256;
    if (grid > 8192) grid = 8192;
    CleanRule rule{cls1, labels, areas, best, HW, 0, 0, false};
    hipLaunchKernelGGL(clean_apply_kernel, dim3((int)grid), dim3(256), 0, st, rule, params_dev, N, H, W, out_cls, yidx, xidx, lut, out, H0, W0, groups,
                       total);
    EGM_CHECK_LAUNCH("mask_clean_u8");
    return EGM_OK;
}
