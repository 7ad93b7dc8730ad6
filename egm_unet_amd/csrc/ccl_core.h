// Connected-component labelling: the union-find core shared by the kernels of ccl.hip and the host check of tools/ccl_host_check.cpp
// (which runs exactly this code on the CPU under sanitizers).  No HIP header is needed to read it.
//
// A label array holds a forest: label[i] <= i always, label[i] == i marks a root.  Links only ever go from a larger index to a smaller
// one, so every path strictly descends (no cycle can form, whatever the interleaving), and the root of a finished component is its
// smallest index = its first pixel in raster order: the canonical label comes out without a renumbering pass.
//
// `Mem` is the view of one image's label array: int load(int i) (a relaxed atomic load), int fetch_min(int i, int v) (atomic min,
// returns the old value), void store(int i, int v).  On the device a load may return an OLDER value of the word than another
// workgroup's atomic has since written (the per-XCD L2s are not coherent for plain reads).  That is harmless here: an older value is a former parent, which is
// still a member of the same component with an index >= the current parent, so find still descends inside the component; only
// fetch_min decides whether a link was made, and it is exact.
//
// Every loop carries a trip bound; a loop that runs out sets a bit in `status` and leaves.  With a sound array neither bound can be
// reached: find descends at most `bound` = H*W times, and every failed fetch_min of unite strictly lowers a + b.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CCL_HD __host__ __device__ inline
#else
#define CCL_HD inline
#endif

constexpr int kCclTileH = 16, kCclTileW = 64, kCclTilePix = kCclTileH * kCclTileW;   // the LDS tile of the first pass
constexpr int kCclBorder = (int)0x80000000u;         // bit of an area word: the component touches the image border
constexpr int kCclAreaMask = 0x7fffffff;
constexpr long long kCclMaxPixels = 1ll << 30;       // H*W limit: indices and areas fit 31 bits
enum { CCL_ST_FIND = 1, CCL_ST_UNION = 2 };          // status bits: a find / a union ran into its trip bound

template <class Mem>
CCL_HD int ccl_find(const Mem& m, int x, int bound, int& status) {
    for (int k = 0; k <= bound; ++k) {
        const int p = m.load(x);
        if (p >= x || p < 0) return x;               // a root (anything but a smaller index ends the walk: never an index out of range)
        x = p;
    }
    status |= CCL_ST_FIND;
    return x;
}

template <class Mem>
CCL_HD void ccl_unite(const Mem& m, int a, int b, int bound, int& status) {
    for (unsigned k = 0; k <= 2u * (unsigned)bound; ++k) {
        a = ccl_find(m, a, bound, status);
        b = ccl_find(m, b, bound, status);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = m.fetch_min(a, b);           // link the larger root under the smaller one
        if (old == a) return;                        // a was a root: linked
        if (old > a || old < 0) break;               // (cannot happen with a sound array)
        a = old;                                     // a had a parent meanwhile (now min(old, b)): go on with that parent, old < a
    }
    status |= CCL_ST_UNION;
}

// Pixels are joined when they hold the same byte and are neighbours under their class's connectivity: `connectivity` (8 or 4) for
// foreground, the dual for background (byte 0).
CCL_HD bool ccl_conn8(int v, int connectivity) { return (v != 0) == (connectivity == 8); }

// The four backward neighbours a pixel links to: 0 left, 1 up, 2 up-left, 3 up-right (2 and 3 under 8-connectivity only).
CCL_HD void ccl_backward(int k, int& dy, int& dx) {
    dy = k == 0 ? 0 : -1;
    dx = k == 0 || k == 2 ? -1 : (k == 3 ? 1 : 0);
}

// First pass, one pixel of a tile: vals[kCclTilePix] holds the tile's bytes (-1 outside the image), m the tile's local forest over
// indices ty * kCclTileW + tx.  A diagonal link is left out where an equal left / up neighbour already implies it.
template <class Mem, class Val>
CCL_HD void ccl_link_tile_pixel(const Mem& m, const Val* vals, int l, int connectivity, int& status) {
    const int v = vals[l];
    if (v < 0) return;
    const int ty = l / kCclTileW, tx = l % kCclTileW;
    const bool left = tx > 0 && vals[l - 1] == v, up = ty > 0 && vals[l - kCclTileW] == v;
    if (left) ccl_unite(m, l, l - 1, kCclTilePix, status);
    if (up) ccl_unite(m, l, l - kCclTileW, kCclTilePix, status);
    if (!ccl_conn8(v, connectivity) || ty == 0 || up) return;
    if (!left && tx > 0 && vals[l - kCclTileW - 1] == v) ccl_unite(m, l, l - kCclTileW - 1, kCclTilePix, status);
    if (tx + 1 < kCclTileW && vals[l - kCclTileW + 1] == v) ccl_unite(m, l, l - kCclTileW + 1, kCclTilePix, status);
}

// Only these pixels have a backward neighbour in another tile.
CCL_HD bool ccl_on_seam(int y, int x) {
    const int tx = x % kCclTileW;
    return y % kCclTileH == 0 || tx == 0 || tx == kCclTileW - 1;
}

// Second pass, one pixel of an image: the links to backward neighbours that lie in ANOTHER tile, on the image's global forest.
template <class Mem>
CCL_HD void ccl_link_seam_pixel(const Mem& m, const unsigned char* cls, int H, int W, int y, int x, int connectivity, int& status) {
    const int i = y * W + x, v = cls[i];
    const bool left = x > 0 && cls[i - 1] == v, up = y > 0 && cls[i - W] == v;
    const bool c8 = ccl_conn8(v, connectivity);
    for (int k = 0; k < (c8 ? 4 : 2); ++k) {
        int dy, dx;
        ccl_backward(k, dy, dx);
        const int yy = y + dy, xx = x + dx;
        if (yy < 0 || xx < 0 || xx >= W) continue;
        if (yy / kCclTileH == y / kCclTileH && xx / kCclTileW == x / kCclTileW) continue;      // same tile: the first pass did it
        if ((k >= 2 && up) || (k == 2 && left)) continue;                                      // implied by two other links
        const int j = yy * W + xx;
        if (cls[j] == v) ccl_unite(m, i, j, H * W, status);
    }
}

CCL_HD bool ccl_on_border(int y, int x, int H, int W) { return y == 0 || x == 0 || y == H - 1 || x == W - 1; }

// Third pass, one pixel: walk to the root and store it (a walk that passes through i meanwhile reads the old parent or the root: both
// descend).  Areas: the first pass left at every TILE root the pixel count of its tile component (| kCclBorder when one of those
// pixels is on the image border) and 0 elsewhere; a tile root that is not its component's root hands its word over to the root, so a
// component costs one atomic per tile it covers, not one per pixel.  Nobody adds to a word that is handed over: only roots receive.
// `Area`: int load(int i), void store(int i, int v), void add(int i, int v), void or_bits(int i, int v) on the image's area words.
template <class Mem, class Area>
CCL_HD int ccl_flatten_pixel(const Mem& m, const Area* areas, int i, int bound, int& status) {
    const int root = ccl_find(m, i, bound, status);
    m.store(i, root);
    if (areas && root != i) {
        const int w = areas->load(i);
        if (w != 0) {
            areas->add(root, w & kCclAreaMask);
            if (w & kCclBorder) areas->or_bits(root, kCclBorder);
            areas->store(i, 0);
        }
    }
    return root;
}

// ---- the clean-up rules on labelled maps ---------------------------------------------------------------------------------------
// Stage 1: a background component fills when it touches no border and has at most max_hole pixels (area_word = area | border bit).
CCL_HD bool ccl_hole_fills(int area_word, int max_hole) { return max_hole > 0 && area_word >= 0 && area_word <= max_hole; }

// Stage 2: the largest component of a class is the one with the greatest (area, -first index): one 64-bit maximum.
CCL_HD unsigned long long ccl_rank_key(int area, int first) {
    return ((unsigned long long)(unsigned)area << 32) | (unsigned long long)(0xffffffffu - (unsigned)first);
}
CCL_HD bool ccl_stage1_on(int max_hole) { return max_hole > 0; }
CCL_HD bool ccl_stage2_on(int min_area, int keep_largest) { return min_area > 1 || keep_largest != 0; }
CCL_HD bool ccl_component_kept(int area, int first, int min_area, int keep_largest, unsigned long long best_of_class) {
    if (area < min_area) return false;
    return !keep_largest || best_of_class == ccl_rank_key(area, first);
}
