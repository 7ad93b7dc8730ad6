// CLIPSeg multi-prompt inference (CLIPDenseBase.forward_multi): B images, K prompts, one backbone pass per image.  The decoder's
// sequences are b-major, s = b*K + k, so the heads' [B*K][1][H][W] output is [B][K][H][W] as it stands.
//   film_fanout    out[b*K + k][t][:] = mul[k][:] * r[b][t][:] + add[k][:]      (FiLM at cond_layer, B -> B*K sequences)
//   bcast_add      a[b*K + k][t][:] += r[b][t][:]                              (reduce_i(act_i) of the later layers, computed on B*L rows)
//   sigmoid_affine x[n][c][:] = offset + scale[c] * sigmoid(x[n][c][:])        (CLIPSegMultiLabel, models/clipseg.py:608-619)
// Rounding: each output is computed in fp32 from the stored operands and rounded once, with the expression of egm_film (vit.hip), so
// the fan-out reproduces the single-prompt FiLM bit for bit.  All three are bandwidth kernels: 4 elements per thread, grid-stride.
#include "common.h"

namespace {

constexpr int NT = 256;

inline int grid_for(long long n) {
    long long b = (n + NT - 1) / NT;
    if (b > 8192) b = 8192;
    return (int)(b < 1 ? 1 : b);
}

template <typename T> struct V4;
template <> struct V4<float> {
    static __device__ __forceinline__ void load(const float* p, float* v) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
    static __device__ __forceinline__ void store(float* p, const float* v) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};
template <> struct V4<bf16_t> {
    static __device__ __forceinline__ void load(const bf16_t* p, float* v) {
        const uint2 q = *reinterpret_cast<const uint2*>(p);
        v[0] = bf16_to_f32(q.x & 0xffff); v[1] = bf16_to_f32(q.x >> 16); v[2] = bf16_to_f32(q.y & 0xffff); v[3] = bf16_to_f32(q.y >> 16);
    }
    static __device__ __forceinline__ void store(bf16_t* p, const float* v) {
        uint2 q;
        q.x = (uint32_t)f32_to_bf16(v[0]) | ((uint32_t)f32_to_bf16(v[1]) << 16);
        q.y = (uint32_t)f32_to_bf16(v[2]) | ((uint32_t)f32_to_bf16(v[3]) << 16);
        *reinterpret_cast<uint2*>(p) = q;
    }
};

// one thread per 4 consecutive features of one (sequence, token) row; D % 4 == 0
template <typename T>
__global__ __launch_bounds__(NT) void film_fanout_kernel(const T* __restrict__ r, const T* __restrict__ mul, const T* __restrict__ add,
                                                         T* __restrict__ out, int K, int L, int D) {
    const int D4 = D / 4;
    const long long per_b = (long long)K * L * D4;                      // blockIdx.y = b
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < per_b; i += (long long)gridDim.x * NT) {
        const int d = (int)(i % D4) * 4;
        const int t = (int)((i / D4) % L);
        const int k = (int)(i / ((long long)L * D4));
        const long long b = blockIdx.y;
        float rv[4], m[4], a[4], o[4];
        V4<T>::load(r + (b * L + t) * D + d, rv);
        V4<T>::load(mul + (long long)k * D + d, m);
        V4<T>::load(add + (long long)k * D + d, a);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = rv[j] * m[j] + a[j];
        V4<T>::store(out + ((b * K + k) * L + t) * D + d, o);
    }
}

template <typename T>
__global__ __launch_bounds__(NT) void bcast_add_kernel(T* __restrict__ a, const T* __restrict__ r, int K, int L, int D) {
    const int D4 = D / 4;
    const long long per_b = (long long)K * L * D4;
    const long long b = blockIdx.y;
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < per_b; i += (long long)gridDim.x * NT) {
        const int d = (int)(i % D4) * 4;
        const int t = (int)((i / D4) % L);
        const int k = (int)(i / ((long long)L * D4));
        T* pa = a + ((b * K + k) * L + t) * D + d;
        float av[4], rv[4];
        V4<T>::load(pa, av);
        V4<T>::load(r + (b * L + t) * D + d, rv);
#pragma unroll
        for (int j = 0; j < 4; ++j) av[j] = av[j] + rv[j];
        V4<T>::store(pa, av);
    }
}

// x [N][C][HW] fp32, HW % 4 == 0
__global__ __launch_bounds__(NT) void sigmoid_affine_kernel(float* __restrict__ x, const float* __restrict__ scale, float offset, int C,
                                                            long long HW, long long total4) {
    const long long HW4 = HW / 4;
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < total4; i += (long long)gridDim.x * NT) {
        const int c = (int)((i / HW4) % C);
        const float sc = scale[c];
        float v[4];
        V4<float>::load(x + 4 * i, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = offset + sc * (1.f / (1.f + expf(-v[j])));
        V4<float>::store(x + 4 * i, v);
    }
}

int check_seq(const char* name, const void* p0, const void* p1, int B, int K, int L, int D) {
    if (!(p0 && p1 && B > 0 && K > 0 && L > 0 && D > 0 && D % 4 == 0 && B < 65536))
        EGM_FAIL(EGM_ERR_ARG, "%s: bad args (B %d, K %d, L %d, D %d; D must be a multiple of 4)", name, B, K, L, D);
    return EGM_OK;
}

}  // namespace

extern "C" int egm_film_fanout(int dtype, const void* r, const void* mul, const void* add, void* out, int B, int K, int L, int D,
                               egm_stream_t s) {
    const int rc = check_seq("film_fanout", r, out, B, K, L, D);
    if (rc != EGM_OK) return rc;
    EGM_REQUIRE(mul && add && egm_aligned16(r) && egm_aligned16(mul) && egm_aligned16(add) && egm_aligned16(out),
                "film_fanout: null or misaligned pointer");
    const dim3 grid(grid_for((long long)K * L * D / 4), B);
    EGM_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((film_fanout_kernel<T>), grid, dim3(NT), 0, (hipStream_t)s, (const T*)r, (const T*)mul,
                                                 (const T*)add, (T*)out, K, L, D));
    EGM_CHECK_LAUNCH("film_fanout");
    return EGM_OK;
}

extern "C" int egm_bcast_add(int dtype, void* a, const void* r, int B, int K, int L, int D, egm_stream_t s) {
    const int rc = check_seq("bcast_add", a, r, B, K, L, D);
    if (rc != EGM_OK) return rc;
    EGM_REQUIRE(egm_aligned16(a) && egm_aligned16(r), "bcast_add: misaligned pointer");
    const dim3 grid(grid_for((long long)K * L * D / 4), B);
    EGM_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((bcast_add_kernel<T>), grid, dim3(NT), 0, (hipStream_t)s, (T*)a, (const T*)r, K, L, D));
    EGM_CHECK_LAUNCH("bcast_add");
    return EGM_OK;
}

extern "C" int egm_sigmoid_affine(float* x, const float* scale, float offset, int N, int C, long long HW, egm_stream_t s) {
    EGM_REQUIRE(x && scale && N > 0 && C > 0 && HW > 0 && HW % 4 == 0 && egm_aligned16(x), "sigmoid_affine: bad args (HW must be a multiple of 4)");
    const long long total4 = (long long)N * C * HW / 4;
    hipLaunchKernelGGL(sigmoid_affine_kernel, dim3(grid_for(total4)), dim3(NT), 0, (hipStream_t)s, x, scale, offset, C, HW, total4);
    EGM_CHECK_LAUNCH("sigmoid_affine");
    return EGM_OK;
}
