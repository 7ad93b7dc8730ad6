// Host check of the connected-component core: runs the find / union / link / decision code of egm_unet_amd/csrc/ccl_core.h (the code
// the kernels of csrc/ccl.hip run) on the CPU, in the kernels' pass structure (tile, seam, flatten, fill, rank, apply) and in several
// pixel orders, over the test patterns, against a breadth-first reference written here.  Meant to be built with sanitizers:
//     g++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/ccl_host_check.cpp -o ccl_host_check && ./ccl_host_check
// Prints one line per group and "ccl_host_check: ok"; exit status 1 on any mismatch or any status bit.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <queue>
#include <string>
#include <vector>

#include "../egm_unet_amd/csrc/ccl_core.h"

namespace {

typedef std::vector<unsigned char> Map;

struct HostForest {
    int* p;
    int load(int i) const { return p[i]; }
    int fetch_min(int i, int v) const { const int old = p[i]; if (v < old) p[i] = v; return old; }
    void store(int i, int v) const { p[i] = v; }
};
struct HostAreas {
    int* p;
    int load(int i) const { return p[i]; }
    void store(int i, int v) const { p[i] = v; }
    void add(int i, int v) const { p[i] += v; }
    void or_bits(int i, int v) const { p[i] |= v; }
};

// pixel visiting orders: the result may not depend on which thread runs first
std::vector<int> order_of(int n, int mode) {
    std::vector<int> o(n);
    for (int i = 0; i < n; ++i) o[i] = i;
    if (mode == 1) std::reverse(o.begin(), o.end());
    if (mode == 2) { unsigned s = 12345u; for (int i = n - 1; i > 0; --i) { s = s * 1664525u + 1013904223u; std::swap(o[i], o[(s >> 8) % (unsigned)(i + 1)]); } }
    return o;
}

// ---- the kernels' passes, sequentially
void label_core(const Map& cls, int H, int W, int conn, int mode, bool border, std::vector<int>& labels, std::vector<int>& areas, int& status) {
    labels.assign((size_t)H * W, -1);
    areas.assign((size_t)H * W, 0);
    const std::vector<int> tord = order_of(kCclTilePix, mode);
    for (int y0 = 0; y0 < H; y0 += kCclTileH)
        for (int x0 = 0; x0 < W; x0 += kCclTileW) {
            short val[kCclTilePix];
            int lab[kCclTilePix];
            for (int l = 0; l < kCclTilePix; ++l) {
                const int y = y0 + l / kCclTileW, x = x0 + l % kCclTileW;
                val[l] = (y < H && x < W) ? (short)cls[(size_t)y * W + x] : (short)-1;
                lab[l] = l;
            }
            const HostForest f{lab};
            for (int l : tord) ccl_link_tile_pixel(f, val, l, conn, status);
            for (int l = 0; l < kCclTilePix; ++l) {
                const int y = y0 + l / kCclTileW, x = x0 + l % kCclTileW;
                if (y < H && x < W) {
                    const int root = ccl_find(f, l, kCclTilePix, status);
                    const int g = (y0 + root / kCclTileW) * W + x0 + root % kCclTileW;
                    labels[(size_t)y * W + x] = g;
                    areas[g] += 1;                                      // (the kernel counts in LDS and writes the word at the tile root)
                    if (border && ccl_on_border(y, x, H, W)) areas[g] |= kCclBorder;
                }
            }
        }
    const std::vector<int> ord = order_of(H * W, mode);
    const HostForest g{labels.data()};
    for (int i : ord)
        if (ccl_on_seam(i / W, i % W)) ccl_link_seam_pixel(g, cls.data(), H, W, i / W, i % W, conn, status);
    const HostAreas ar{areas.data()};
    for (int i : ord) ccl_flatten_pixel(g, &ar, i, H * W, status);
}

Map clean_core(const Map& cls, int H, int W, int conn, int min_area, int keep_largest, int max_hole, int mode, int& status) {
    const int HW = H * W;
    std::vector<int> labels, areas;
    Map cls1 = cls;
    if (ccl_stage1_on(max_hole)) {
        label_core(cls, H, W, conn, mode, true, labels, areas, status);
        for (int i = 0; i < HW; ++i)
            if (cls[i] == 0 && labels[i] > 0 && ccl_hole_fills(areas[labels[i]], max_hole)) cls1[i] = cls[labels[i] - 1];
    }
    if (!ccl_stage2_on(min_area, keep_largest)) return cls1;
    label_core(cls1, H, W, conn, mode, false, labels, areas, status);
    std::vector<unsigned long long> best(256, 0ull);
    for (int i = 0; i < HW; ++i)
        if (cls1[i] && labels[i] == i) best[cls1[i]] = std::max(best[cls1[i]], ccl_rank_key(areas[i] & kCclAreaMask, i));
    Map out = cls1;
    for (int i = 0; i < HW; ++i)
        if (cls1[i] && !ccl_component_kept(areas[labels[i]] & kCclAreaMask, labels[i], min_area, keep_largest, best[cls1[i]])) out[i] = 0;
    return out;
}

// ---- the reference: breadth-first search in raster order, the rules spelt out
void label_ref(const Map& cls, int H, int W, int conn, std::vector<int>& labels, std::vector<int>& areas, std::vector<char>& touches) {
    labels.assign((size_t)H * W, -1);
    areas.assign((size_t)H * W, 0);
    touches.assign((size_t)H * W, 0);
    for (int s = 0; s < H * W; ++s) {
        if (labels[s] >= 0) continue;
        const int v = cls[s];
        const bool c8 = v ? conn == 8 : conn == 4;
        std::queue<int> q;
        q.push(s);
        labels[s] = s;
        while (!q.empty()) {
            const int i = q.front(); q.pop();
            const int y = i / W, x = i % W;
            areas[s] += 1;
            if (y == 0 || x == 0 || y == H - 1 || x == W - 1) touches[s] = 1;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    if ((!dy && !dx) || (!c8 && dy && dx)) continue;
                    const int yy = y + dy, xx = x + dx;
                    if (yy < 0 || xx < 0 || yy >= H || xx >= W) continue;
                    const int j = yy * W + xx;
                    if (labels[j] < 0 && cls[j] == v) { labels[j] = s; q.push(j); }
                }
        }
    }
}

Map clean_ref(const Map& cls, int H, int W, int conn, int min_area, int keep_largest, int max_hole) {
    std::vector<int> labels, areas;
    std::vector<char> touches;
    Map m = cls;
    if (max_hole > 0) {
        label_ref(cls, H, W, conn, labels, areas, touches);
        for (int i = 0; i < H * W; ++i)
            if (cls[i] == 0 && !touches[labels[i]] && areas[labels[i]] <= max_hole) m[i] = cls[labels[i] - 1];
    }
    if (!(min_area > 1 || keep_largest)) return m;
    label_ref(m, H, W, conn, labels, areas, touches);
    std::vector<int> winner(256, -1);
    for (int i = 0; i < H * W; ++i)
        if (m[i] && labels[i] == i && (winner[m[i]] < 0 || areas[i] > areas[winner[m[i]]])) winner[m[i]] = i;     // ties: the first stays
    Map out = m;
    for (int i = 0; i < H * W; ++i)
        if (m[i] && (areas[labels[i]] < min_area || (keep_largest && winner[m[i]] != labels[i]))) out[i] = 0;
    return out;
}

// ---- patterns
struct Case { std::string name; int H, W; Map m; };

Map blank(int H, int W, int v = 0) { return Map((size_t)H * W, (unsigned char)v); }

void rect(Map& m, int W, int y0, int x0, int y1, int x1, int v) {          // [y0, y1) x [x0, x1)
    for (int y = y0; y < y1; ++y) for (int x = x0; x < x1; ++x) m[(size_t)y * W + x] = (unsigned char)v;
}

Map spiral(int S) {                                                        // one-pixel-wide square spiral walked inwards from (0, 0)
    Map m = blank(S, S);
    const int D[4][2] = {{0, 1}, {1, 0}, {0, -1}, {-1, 0}};
    auto inb = [S](int y, int x) { return y >= 0 && x >= 0 && y < S && x < S; };
    int y = 0, x = 0, d = 0;
    bool turned = false;
    m[0] = 1;
    for (;;) {                                                             // forward while the cell after the next one is free
        const int ny = y + D[d][0], nx = x + D[d][1], my = ny + D[d][0], mx = nx + D[d][1];
        if (inb(ny, nx) && !m[(size_t)ny * S + nx] && (!inb(my, mx) || !m[(size_t)my * S + mx])) {
            y = ny; x = nx; m[(size_t)y * S + x] = 1; turned = false;
        } else if (!turned) {
            d = (d + 1) % 4; turned = true;
        } else {
            break;
        }
    }
    return m;
}

std::vector<Case> cases() {
    std::vector<Case> cs;
    const int sizes[][2] = {{1, 1}, {1, 70}, {70, 1}, {64, 64}, {33, 65}, {129, 131}};
    unsigned seed = 99u;
    for (auto& hw : sizes) {
        const int H = hw[0], W = hw[1];
        const std::string tag = std::to_string(H) + "x" + std::to_string(W);
        cs.push_back({"empty " + tag, H, W, blank(H, W)});
        cs.push_back({"full " + tag, H, W, blank(H, W, 1)});
        Map c = blank(H, W);
        for (int i = 0; i < H * W; ++i) c[i] = ((i / W + i % W) & 1) ? 0 : 1;
        cs.push_back({"checker " + tag, H, W, c});
        for (double d : {0.3, 0.5, 0.62, 0.8}) {
            Map r = blank(H, W);
            for (auto& p : r) { seed = seed * 1664525u + 1013904223u; p = ((seed >> 8) & 0xffff) < d * 65536 ? 1 : 0; }
            cs.push_back({"random " + std::to_string(d) + " " + tag, H, W, r});
            for (auto& p : r) { seed = seed * 1664525u + 1013904223u; if (p && (seed >> 20) % 3 == 0) p = 2; }
            cs.push_back({"random 2 classes " + tag, H, W, r});
        }
        if (H >= 33 && W >= 33) {
            Map r = blank(H, W);                                          // ring, hole, ring, hole; a one-pixel hole; a diagonal leak
            rect(r, W, 2, 2, 31, 31, 1); rect(r, W, 5, 5, 28, 28, 0); rect(r, W, 9, 9, 24, 24, 2); rect(r, W, 13, 13, 20, 20, 0);
            r[(size_t)10 * W + 10] = 0;
            cs.push_back({"rings " + tag, H, W, r});
            Map k = blank(H, W);                                          // a hole that reaches the border only through a diagonal step
            rect(k, W, 0, 0, 12, 12, 1); rect(k, W, 1, 1, 6, 6, 0); k[0] = 0;
            rect(k, W, 16, 16, 30, 30, 1); rect(k, W, 18, 18, 22, 22, 0); k[(size_t)22 * W + 22] = 0; k[(size_t)23 * W + 23] = 0;
            rect(k, W, 24, 24, 30, 30, 0);
            cs.push_back({"diagonal leak " + tag, H, W, k});
            Map t = blank(H, W);                                          // comb: vertical teeth joined along the bottom row
            for (int x = 0; x < W; x += 2) rect(t, W, 1, x, H, x + 1, 1);
            rect(t, W, H - 1, 0, H, W, 1);
            cs.push_back({"comb " + tag, H, W, t});
            Map q = blank(H, W);                                          // three class values side by side; equal ones merge
            rect(q, W, 3, 0, 20, W / 3, 1); rect(q, W, 3, W / 3, 20, 2 * W / 3, 2); rect(q, W, 3, 2 * W / 3, 20, W, 1);
            rect(q, W, 20, 0, 23, W, 1); rect(q, W, 26, 4, 30, 9, 3);
            cs.push_back({"three classes " + tag, H, W, q});
        }
    }
    cs.push_back({"spiral 67x67", 67, 67, spiral(67)});
    return cs;
}

}  // namespace

int main() {
    const int param_sets[][3] = {{0, 0, 0}, {2, 0, 0}, {5, 0, 3}, {0, 1, 0}, {5, 1, 3}, {0, 0, 1 << 30}};     // min_area, keep_largest, max_hole
    int failures = 0, checks = 0;
    size_t ncase = 0;
    for (const Case& c : cases()) {
        int bad = 0;
        ++ncase;
        for (int conn : {4, 8}) {
            std::vector<int> rl, ra, labels, areas;
            std::vector<char> rt;
            label_ref(c.m, c.H, c.W, conn, rl, ra, rt);
            std::vector<Map> want;
            for (auto& ps : param_sets) want.push_back(clean_ref(c.m, c.H, c.W, conn, ps[0], ps[1], ps[2]));
            for (int mode = 0; mode < 3; ++mode) {
                int status = 0;
                label_core(c.m, c.H, c.W, conn, mode, false, labels, areas, status);
                bad += (labels != rl) + (areas != ra) + (status != 0);
                if (mode == 2) {                                           // the border bit of the area words
                    label_core(c.m, c.H, c.W, conn, mode, true, labels, areas, status);
                    for (int i = 0; i < c.H * c.W; ++i)
                        bad += (areas[i] & kCclAreaMask) != ra[i] || ((areas[i] & kCclBorder) != 0) != (rt[i] != 0);
                }
                for (size_t k = 0; k < want.size(); ++k) {
                    if ((int)((k + ncase) % 3) != mode) continue;          // the labellings above ran in every order; one order per rule here
                    status = 0;
                    const int* ps = param_sets[k];
                    bad += (clean_core(c.m, c.H, c.W, conn, ps[0], ps[1], ps[2], mode, status) != want[k]) + (status != 0);
                    ++checks;
                }
            }
        }
        std::printf("%-28s %s\n", c.name.c_str(), bad ? "MISMATCH" : "ok");
        failures += bad != 0;
    }
    {   // the facts the test patterns rely on
        const int S = 67;
        for (const Case& c : cases())
            if (c.name == "spiral 67x67") {
                std::vector<int> l, a; std::vector<char> t;
                label_ref(c.m, S, S, 4, l, a, t);
                int comps = 0, fg = 0, fgcomps = 0;
                for (int i = 0; i < S * S; ++i) { comps += l[i] == i; fg += c.m[i] != 0; fgcomps += l[i] == i && c.m[i]; }
                std::printf("spiral: %d foreground pixels, %d foreground and %d background components at connectivity 4\n", fg, fgcomps, comps - fgcomps);
                failures += !(fg == 2311 && fgcomps == 1 && comps == 2);
            }
    }
    if (failures) { std::printf("ccl_host_check: %d pattern(s) FAILED\n", failures); return 1; }
    std::printf("ccl_host_check: ok (%d clean-up checks)\n", checks);
    return 0;
}
