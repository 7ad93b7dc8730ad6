// The training end of the device data path for a whole batch of ragged photos: B decoded uint8 photos [H_b][W_b][3] with their
// masks [H_b][W_b] -> RandomResize -> flips -> pad_if_smaller -> RandomCrop -> ToTensor -> Normalize -> collate slot, i.e. what
// egm_resample_u8 (axis 1, then axis 0), egm_gather_u8, egm_augment_u8 and collate_fn compute per image (csrc/data.hip), written
// straight into fp32 [B][3][slot_h][slot_w] / int64 [B][slot_h][slot_w].  Per output element the expressions are theirs, so image b of
// the result equals the per-image chain bit for bit.  Everything that differs between the images of a batch sits in one device table
// of egm_train_desc rows (include/egm_hip.h), blockIdx.y is the image: two launches whatever B, one when no image is resized in x.
//   horizontal  only what the crop can see: the source rows [r0, r0 + nr) that the vertical taps of the visible output rows touch
//               and the resized columns [c0, c0 + nc) inside the crop window after the flip, uint8 [nr][nc][3] in the workspace.
//               At the large sizes of the 565 / 480 preset that is less than half of the resized photo.
//   vertical    one thread per pixel of the slot: vertical taps over the intermediate (or over the photo where the horizontal pass is
//               the identity), flip, pad, crop, normalise; the target is read from the source mask through the two nearest-index
//               tables, so no resized mask exists.
// Byte-streaming kernels without reuse beyond the 3..7 taps, which L1/L2 serve.  Rows of a [.][nc][3] tensor start at any alignment, so
// loads are per byte and lanes are adjacent pixels (a wave reads 192 contiguous bytes per tap, backwards under hflip); the fp32 planes
// are written 256 and the int64 plane 512 contiguous bytes per wave.  The descriptor is uniform per workgroup (scalar loads).
#include "common.h"

static_assert(sizeof(egm_train_desc) == 120, "egm_train_desc is packed by the host (egm_unet_amd/data.py: TRAIN_DESC)");

namespace {

constexpr int kPrecisionBits = 32 - 8 - 2;      // Pillow Resample.c, as in data.hip

__device__ __forceinline__ int clip8(int v) {
    v >>= kPrecisionBits;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// ws[ws_off + (r * nc + xi) * 3 + c] = clip8(2^21 + sum_j img[r0 + r][x0 + j][c] * coefs[xi][j]), (x0, n) = bounds[xi], xi = xx - c0
__global__ __launch_bounds__(256) void train_hpass_kernel(const egm_train_desc* __restrict__ tab, unsigned char* __restrict__ ws) {
    const egm_train_desc d = tab[blockIdx.y];
    if (d.xksize <= 0) return;                                                   // identity: the vertical pass reads the photo itself
    const int* bounds = reinterpret_cast<const int*>(tab) + d.xb_off;
    const int* coefs = reinterpret_cast<const int*>(tab) + d.xc_off;
    const unsigned char* src = static_cast<const unsigned char*>(d.img);
    unsigned char* dst = ws + d.ws_off;
    const unsigned total = (unsigned)d.nr * (unsigned)d.nc, nc = (unsigned)d.nc;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const unsigned r = i / nc, xi = i - r * nc;
        int x0 = bounds[xi * 2], n = bounds[xi * 2 + 1];
        x0 = clampi(x0, 0, d.W - 1);                                             // no table can make the kernel leave the row
        n = n < 0 ? 0 : min(n, min(d.xksize, d.W - x0));
        const unsigned char* p = src + ((long long)(d.r0 + (int)r) * d.W + x0) * 3;
        const int* k = coefs + (long long)xi * d.xksize;
        int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
        for (int j = 0; j < n; ++j) {
            const int c = k[j];
            a0 += (int)p[j * 3] * c; a1 += (int)p[j * 3 + 1] * c; a2 += (int)p[j * 3 + 2] * c;
        }
        unsigned char* q = dst + (long long)i * 3;
        q[0] = (unsigned char)clip8(a0); q[1] = (unsigned char)clip8(a1); q[2] = (unsigned char)clip8(a2);
    }
}

__global__ __launch_bounds__(256) void train_vpass_kernel(const egm_train_desc* __restrict__ tab, const unsigned char* __restrict__ ws,
                                                          float* __restrict__ out_img, long long* __restrict__ out_tgt, int slot_h,
                                                          int slot_w, float m0, float m1, float m2, float s0, float s1, float s2) {
    const egm_train_desc d = tab[blockIdx.y];
    const int* tb = reinterpret_cast<const int*>(tab);
    const int* ybounds = tb + d.yb_off;
    const int* ycoefs = tb + d.yc_off;
    const int* xnn = tb + d.xnn_off;
    const int* ynn = tb + d.ynn_off;
    const unsigned char* mask = static_cast<const unsigned char*>(d.mask);
    // the rows [r0, r0 + nr) x columns [c0, c0 + nc) of the horizontally resized photo: the intermediate, or the photo where ow == W
    const bool hp = d.xksize > 0;
    const unsigned char* base = hp ? ws + d.ws_off : static_cast<const unsigned char*>(d.img);
    const int pitch = hp ? d.nc : d.W, rbase = hp ? d.r0 : 0, cbase = hp ? d.c0 : 0;
    const int rlast = d.r0 + d.nr - 1, clast = d.c0 + d.nc - 1, ylast = d.y0 + d.ny - 1;
    const unsigned plane = (unsigned)slot_h * (unsigned)slot_w, sw = (unsigned)slot_w;
    float* oi = out_img + (long long)blockIdx.y * 3 * plane;
    long long* ot = out_tgt + (long long)blockIdx.y * plane;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < plane; i += gridDim.x * 256u) {
        const unsigned yu = i / sw;
        const int y = (int)yu, x = (int)(i - yu * sw);
        float v0 = 0.f, v1 = 0.f, v2 = 0.f;
        long long t = 255;                                                       // collate_fn's fill outside the crop
        if (y < d.crop_h && x < d.crop_w) {
            const int sy = y + d.top, sx = x + d.left;                           // coordinates in the flipped (and zero-padded) image
            int p0 = 0, p1 = 0, p2 = 0; t = 0;
            if (sy < d.oh && sx < d.ow) {
                int yy = d.vflip ? d.oh - 1 - sy : sy, xx = d.hflip ? d.ow - 1 - sx : sx;
                yy = clampi(yy, d.y0, ylast); xx = clampi(xx, d.c0, clast);      // the plan's windows hold both; a wrong row reads in bounds
                const int yi = yy - d.y0, xi = xx - d.c0;
                if (d.yksize > 0) {
                    int r = ybounds[yi * 2], n = ybounds[yi * 2 + 1];
                    r = clampi(r, d.r0, rlast);
                    n = n < 0 ? 0 : min(n, min(d.yksize, rlast + 1 - r));
                    const long long step = (long long)pitch * 3;
                    const unsigned char* p = base + ((long long)(r - rbase) * pitch + (xx - cbase)) * 3;
                    const int* k = ycoefs + (long long)yi * d.yksize;
                    int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
                    for (int j = 0; j < n; ++j) {
                        const int c = k[j];
                        const unsigned char* q = p + j * step;
                        a0 += (int)q[0] * c; a1 += (int)q[1] * c; a2 += (int)q[2] * c;
                    }
                    p0 = clip8(a0); p1 = clip8(a1); p2 = clip8(a2);
                } else {
                    const int r = clampi(yy, d.r0, rlast);
                    const unsigned char* p = base + ((long long)(r - rbase) * pitch + (xx - cbase)) * 3;
                    p0 = p[0]; p1 = p[1]; p2 = p[2];
                }
                t = mask[(long long)clampi(ynn[yi], 0, d.H - 1) * d.W + clampi(xnn[xi], 0, d.W - 1)];
            }
            v0 = ((float)p0 / 255.0f - m0) / s0;                                 // augment_kernel's expression
            v1 = ((float)p1 / 255.0f - m1) / s1;
            v2 = ((float)p2 / 255.0f - m2) / s2;
        }
        oi[i] = v0; oi[plane + i] = v1; oi[2ll * plane + i] = v2;
        ot[i] = t;
    }
}

inline int batch_grid_x(long long n, int B) {
    long long b = (n + 255) / 256, cap = 8192 / B;
    if (cap < 64) cap = 64;
    if (b > cap) b = cap;
    return (int)(b < 1 ? 1 : b);
}

}  // namespace

extern "C" int egm_train_batch_u8(const egm_train_desc* table_dev, int B, int slot_h, int slot_w, int max_crop_h, int max_crop_w,
                                  float* out_img_bchw, long long* out_target_bhw, const float* mean3_host, const float* std3_host,
                                  void* workspace, long long workspace_bytes, long long max_hpass_pixels, egm_stream_t s) {
    EGM_REQUIRE(table_dev && out_img_bchw && out_target_bhw && mean3_host && std3_host, "train_batch_u8: null pointer");
    EGM_REQUIRE(B > 0 && B <= 65535 && slot_h > 0 && slot_w > 0, "train_batch_u8: bad batch or slot");
    EGM_REQUIRE(max_crop_h > 0 && max_crop_w > 0 && slot_h >= max_crop_h && slot_w >= max_crop_w, "train_batch_u8: slot smaller than a crop");
    EGM_REQUIRE(std3_host[0] != 0.f && std3_host[1] != 0.f && std3_host[2] != 0.f, "train_batch_u8: zero std");
    EGM_REQUIRE(workspace_bytes >= 0 && max_hpass_pixels >= 0 && max_hpass_pixels * 3 <= workspace_bytes,
                "train_batch_u8: workspace smaller than an intermediate");
    EGM_REQUIRE(max_hpass_pixels == 0 || workspace != nullptr, "train_batch_u8: a horizontal pass needs the workspace");
    EGM_REQUIRE((long long)B * 3 * slot_h * slot_w < (1ll << 31) && workspace_bytes < (1ll << 31),
                "train_batch_u8: B*3*slot_h*slot_w and the workspace must stay below 2^31");
    if (max_hpass_pixels > 0) {
        hipLaunchKernelGGL(train_hpass_kernel, dim3(batch_grid_x(max_hpass_pixels, B), B), dim3(256), 0, (hipStream_t)s, table_dev,
                           (unsigned char*)workspace);
        EGM_CHECK_LAUNCH("train_batch_u8 (horizontal)");
    }
    hipLaunchKernelGGL(train_vpass_kernel, dim3(batch_grid_x((long long)slot_h * slot_w, B), B), dim3(256), 0, (hipStream_t)s, table_dev,
                       (const unsigned char*)workspace, out_img_bchw, out_target_bhw, slot_h, slot_w, mean3_host[0], mean3_host[1],
                       mean3_host[2], std3_host[0], std3_host[1], std3_host[2]);
    EGM_CHECK_LAUNCH("train_batch_u8 (vertical)");
    return EGM_OK;
}
