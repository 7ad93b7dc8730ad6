// Inference-only kernels of the folded eval path (egm_unet_amd/infer.py):
//
//   * egm_conv_fold_pack_multi: every conv -> BatchNorm pair of a model folded in ONE launch.  With s = gamma / sqrt(running_var + eps)
//     per output channel, the forward operand pack of w*s (the `wf` layout of egm_conv_pack, compute dtype) and the fp32 bias
//     (b - running_mean)*s + beta; the product is formed in fp32 on the fp32 master weights and rounded once.  nn.BatchNorm2d in eval
//     mode behind nn.Conv2d (src/EGM-UNet.py:44-55, 888-904, 958-975; src/unet.py:7-18) is then the convolution alone, and the
//     activation goes into its epilogue (egm_conv_fwd_act).
//   * egm_argmax_u8: NCHW fp32 logits -> uint8 class ids (predict.py: output.argmax(1), then the color_map LUT).
#include "common.h"

namespace {

// device table entry of egm_conv_fold_pack_multi (include/egm_hip.h documents the byte layout)
struct FoldEntry {
    const float* w; const float* b; const float* gamma; const float* beta; const float* mean; const float* var;
    void* wf; float* bias;
    float eps; int Cout, Cin, CoutP, CinP, KH, KW, groups, chunk0, pad;
};
static_assert(sizeof(FoldEntry) == 104, "egm_fold_entry layout");
constexpr int kFoldChunk = 1024;

__device__ __forceinline__ float fold_scale(const FoldEntry& e, int co) {
    const float rstd = 1.f / sqrtf(e.var[co] + e.eps);                 // as egm_bn_eval_coeffs
    return (e.gamma ? e.gamma[co] : 1.f) * rstd;
}

template <typename T>
__global__ __launch_bounds__(256) void conv_fold_pack_multi_kernel(const FoldEntry* __restrict__ tab, int n) {
    const int s_t = egm_find_entry(tab, n, (long long)blockIdx.x);
    const int s_c = (int)((long long)blockIdx.x - (long long)tab[s_t].chunk0);
    const FoldEntry e = tab[s_t];
    if (s_c == 0) {                                                     // the entry's first workgroup also writes the folded bias
        for (int co = threadIdx.x; co < e.CoutP; co += 256) {
            float v = 0.f;
            if (co < e.Cout) {
                const float s = fold_scale(e, co);
                v = ((e.b ? e.b[co] : 0.f) - e.mean[co]) * s + (e.beta ? e.beta[co] : 0.f);
            }
            e.bias[co] = v;
        }
    }
    const long long total = (long long)e.KH * e.KW * e.CoutP * e.CinP;
    const int cin_g = e.Cin / e.groups, cout_g = e.Cout / e.groups;
    T* wf = reinterpret_cast<T*>(e.wf);
    const WLayout lf = egm_w_layout(TypeInfo<T>::kDtype, e.KH, e.KW, e.CinP, e.CoutP);
#pragma unroll
    for (int k = 0; k < kFoldChunk / 256; ++k) {
        const long long i = (long long)s_c * kFoldChunk + k * 256 + threadIdx.x;
        if (i >= total) break;
        const int ci = (int)(i % e.CinP), co = (int)((i / e.CinP) % e.CoutP), tap = (int)(i / ((long long)e.CinP * e.CoutP));
        float v = 0.f;
        if (co < e.Cout && ci < e.Cin && (co / cout_g) == (ci / cin_g)) {
            const int r = tap / e.KW, sx = tap % e.KW;
            v = e.w[(((long long)co * cin_g + (ci % cin_g)) * e.KH + r) * e.KW + sx] * fold_scale(e, co);
        }
        wf[egm_w_off(lf, tap, co, ci, e.CoutP, e.CinP)] = from_f32<T>(v);
    }
}

// one thread per pixel; ties go to the lowest class index (torch.argmax)
__global__ __launch_bounds__(256) void argmax_u8_kernel(const float* __restrict__ logits, int C, long long HW, long long total,
                                                        const unsigned char* __restrict__ lut, unsigned char* __restrict__ out) {
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long nimg = i / HW, px = i - nimg * HW;
        const float* l = logits + nimg * C * HW + px;
        float best = l[0];
        int arg = 0;
        for (int c = 1; c < C; ++c) {
            const float v = l[(long long)c * HW];
            if (v > best) { best = v; arg = c; }
        }
        out[i] = lut ? lut[arg] : (unsigned char)arg;
    }
}

}  // namespace

extern "C" int egm_conv_fold_chunk(void) { return kFoldChunk; }

extern "C" int egm_conv_fold_pack_multi(int dtype, const void* table_dev, int n, long long total_chunks, egm_stream_t s) {
    EGM_REQUIRE(table_dev && n > 0 && total_chunks > 0 && total_chunks < (1LL << 30), "conv_fold_pack_multi: bad args");
    EGM_REQUIRE(egm_aligned16(table_dev), "conv_fold_pack_multi: table must be 16-byte aligned");
    EGM_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((conv_fold_pack_multi_kernel<T>), dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)s,
                                                 (const FoldEntry*)table_dev, n));
    EGM_CHECK_LAUNCH("conv_fold_pack_multi");
    return EGM_OK;
}

extern "C" int egm_argmax_u8(const float* logits, const unsigned char* lut, unsigned char* out, int N, int C, int H, int W, egm_stream_t s) {
    EGM_REQUIRE(logits && out, "argmax_u8: null pointer");
    EGM_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C <= 256, "argmax_u8: bad shape N=%d C=%d H=%d W=%d (C <= 256)", N, C, H, W);
    const long long HW = (long long)H * W, total = (long long)N * HW;
    const long long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(argmax_u8_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, (hipStream_t)s, logits, C, HW, total,
                       lut, out);
    EGM_CHECK_LAUNCH("argmax_u8");
    return EGM_OK;
}
