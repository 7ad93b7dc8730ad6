// CLIPSeg multi-prompt inference (CLIPDenseBase.forward_multi): B images, K prompts, one backbone pass per image.  The decoder's
// sequences are b-major, s = b*K + k, so the heads' [B*K][1][H][W] output is [B][K][H][W] as it stands.
//   film_fanout    out[b*K + k][t][:] = mul[k][:] * r[b][t][:] + add[k][:]      (FiLM at cond_layer, B -> B*K sequences)
//   bcast_add      a[b*K + k][t][:] += r[b][t][:]                              (reduce_i(act_i) of the later layers, computed on B*L rows)
//   sigmoid_affine x[n][c][:] = offset + scale[c] * sigmoid(x[n][c][:])        (CLIPSegMultiLabel, models/clipseg.py:608-619)
// Rounding: each output is computed in fp32 from the stored operands and rounded once, with the expression of egm_film (vit.hip), so
// the fan-out reproduces the single-prompt FiLM bit for bit.  All three are bandwidth kernels: 4 elements per thread, grid-stride.
// Decoder training on K prompts (CLIPDenseBase.forward_multi_train, clip/train_ops.py FilmFanoutFn / BcastAddFn):
//   bcast_add_out  out[b*K + k][t][:] = a[b*K + k][t][:] + r[b][t][:]          (bcast_add out of place: autograd has saved a)
//   group_sum      out[b][t][:] = sum_k g[b*K + k][t][:]                       (gradient of the broadcast operand, k ascending)
//   film_fanout_bwd  dr[b][t][:] = sum_k g[b*K + k][t][:] * mul[k][:];  dmul[k][:] = sum_{b,t} g * r;  dadd[k][:] = sum_{b,t} g
// fp32 accumulation, one rounding per output, no atomics: the sums over (b, t) are per-workgroup partials added in block order.
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

// out may be a itself (egm_bcast_add): every element is read and written by the same thread
template <typename T>
__global__ __launch_bounds__(NT) void bcast_add_kernel(const T* a, const T* __restrict__ r, T* out, int K, int L, int D) {
    const int D4 = D / 4;
    const long long per_b = (long long)K * L * D4;
    const long long b = blockIdx.y;
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < per_b; i += (long long)gridDim.x * NT) {
        const int d = (int)(i % D4) * 4;
        const int t = (int)((i / D4) % L);
        const int k = (int)(i / ((long long)L * D4));
        const long long o = ((b * K + k) * L + t) * D + d;
        float av[4], rv[4];
        V4<T>::load(a + o, av);
        V4<T>::load(r + (b * L + t) * D + d, rv);
#pragma unroll
        for (int j = 0; j < 4; ++j) av[j] = av[j] + rv[j];
        V4<T>::store(out + o, av);
    }
}

// N consecutive features per thread: 4 as above, or 8 bf16 (16 bytes) where D % 8 == 0
template <typename T, int N> struct VN : V4<T> {};
template <> struct VN<bf16_t, 8> {
    static __device__ __forceinline__ void load(const bf16_t* p, float* v) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        v[0] = bf16_to_f32(q.x & 0xffff); v[1] = bf16_to_f32(q.x >> 16); v[2] = bf16_to_f32(q.y & 0xffff); v[3] = bf16_to_f32(q.y >> 16);
        v[4] = bf16_to_f32(q.z & 0xffff); v[5] = bf16_to_f32(q.z >> 16); v[6] = bf16_to_f32(q.w & 0xffff); v[7] = bf16_to_f32(q.w >> 16);
    }
    static __device__ __forceinline__ void store(bf16_t* p, const float* v) {
        uint4 q;
        q.x = (uint32_t)f32_to_bf16(v[0]) | ((uint32_t)f32_to_bf16(v[1]) << 16);
        q.y = (uint32_t)f32_to_bf16(v[2]) | ((uint32_t)f32_to_bf16(v[3]) << 16);
        q.z = (uint32_t)f32_to_bf16(v[4]) | ((uint32_t)f32_to_bf16(v[5]) << 16);
        q.w = (uint32_t)f32_to_bf16(v[6]) | ((uint32_t)f32_to_bf16(v[7]) << 16);
        *reinterpret_cast<uint4*>(p) = q;
    }
};
inline int vec_for(int dtype, int D) { return dtype == EGM_BF16 && D % 8 == 0 ? 8 : 4; }

// out[b][t][:] = sum_k g[b*K + k][t][:], k ascending in fp32: one thread per VEC features of one (image, token) row
template <typename T, int VEC>
__global__ __launch_bounds__(NT) void group_sum_kernel(const T* __restrict__ g, T* __restrict__ out, int K, int L, int D, long long total) {
    const int DV = D / VEC;
    const long long LD = (long long)L * D;
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const long long bt = i / DV;                                     // b*L + t
        const int d = (int)(i - bt * DV) * VEC;
        const long long b = bt / L;
        const T* pg = g + b * K * LD + (bt - b * L) * D + d;
        float acc[VEC], gv[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
        for (int k = 0; k < K; ++k) {
            VN<T, VEC>::load(pg + k * LD, gv);
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] += gv[e];
        }
        VN<T, VEC>::store(out + bt * D + d, acc);
    }
}

// Backward of film_fanout.  One workgroup per (image, token tile): threads are laid out [rw rows][cw column vectors] (cw = min(D / VEC,
// NT)), a thread owns FAN_TPT tokens (rows row, row + rw, ...) of its column vector, keeps their r and the running dr in registers and
// walks the K prompts: g is read once, r once per (b, t, d).  Per prompt the rows' sums of g * r and g are added through LDS in row order
// and written as this workgroup's partial part[block][2][K][D]; fan_finalize_kernel adds the partials in block order.
constexpr int FAN_TPT = 2;
struct FanTile { int cw, rw, tiles; };
inline FanTile fan_tile(int L, int D, int vec) {
    FanTile f;
    const int dv = D / vec;
    f.cw = dv < NT ? dv : NT;
    f.rw = NT / f.cw;
    f.tiles = (L + f.rw * FAN_TPT - 1) / (f.rw * FAN_TPT);
    return f;
}

template <typename T, int VEC>
__global__ __launch_bounds__(NT) void film_fanout_bwd_kernel(const T* __restrict__ g, const T* __restrict__ r, const T* __restrict__ mul,
                                                             T* __restrict__ dr, float* __restrict__ part, int K, int L, int D, int cw, int rw,
                                                             int tiles) {
    __shared__ float red[2][NT * VEC];
    const int DV = D / VEC;
    const long long b = blockIdx.x / tiles;
    const int t0 = (blockIdx.x % tiles) * rw * FAN_TPT;
    const int col = threadIdx.x % cw, row = threadIdx.x / cw;
    float* pm = part + (long long)blockIdx.x * 2 * K * D;
    float* pa = pm + (long long)K * D;
    for (int c0 = 0; c0 < DV; c0 += cw) {                                // one pass unless D / VEC > NT
        const int d = (c0 + col) * VEC;
        const bool colok = row < rw && c0 + col < DV;
        float rv[FAN_TPT][VEC], acc[FAN_TPT][VEC];
        bool ok[FAN_TPT];
#pragma unroll
        for (int j = 0; j < FAN_TPT; ++j) {
            const int t = t0 + row + j * rw;
            ok[j] = colok && t < L;
#pragma unroll
            for (int e = 0; e < VEC; ++e) { rv[j][e] = 0.f; acc[j][e] = 0.f; }
            if (ok[j]) VN<T, VEC>::load(r + (b * L + t) * D + d, rv[j]);
        }
        for (int k = 0; k < K; ++k) {
            float m[VEC], s1[VEC], s2[VEC], gv[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) { m[e] = 0.f; s1[e] = 0.f; s2[e] = 0.f; }
            if (colok) VN<T, VEC>::load(mul + (long long)k * D + d, m);
#pragma unroll
            for (int j = 0; j < FAN_TPT; ++j) {
                if (ok[j]) {
                    VN<T, VEC>::load(g + ((b * K + k) * L + t0 + row + j * rw) * D + d, gv);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) { acc[j][e] += gv[e] * m[e]; s1[e] += gv[e] * rv[j][e]; s2[e] += gv[e]; }
                }
            }
            if (row < rw) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) { red[0][threadIdx.x * VEC + e] = s1[e]; red[1][threadIdx.x * VEC + e] = s2[e]; }
            }
            __syncthreads();
            // one thread per feature of this pass (x = col * VEC + e) and sum: the rows' values lie cw * VEC apart
            for (int x = threadIdx.x; x < 2 * cw * VEC; x += NT) {
                const int which = x >= cw * VEC, f = x - which * cw * VEC;
                if (c0 * VEC + f < D) {
                    float t = 0.f;
                    for (int rr = 0; rr < rw; ++rr) t += red[which][rr * cw * VEC + f];
                    (which ? pa : pm)[(long long)k * D + c0 * VEC + f] = t;
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < FAN_TPT; ++j)
            if (ok[j]) VN<T, VEC>::store(dr + (b * L + t0 + row + j * rw) * D + d, acc[j]);
    }
}

// dmul / dadd [K][D] = the workgroups' partials [nblk][2][K][D] added in ascending block order
template <typename T>
__global__ __launch_bounds__(NT) void fan_finalize_kernel(const float* __restrict__ part, T* __restrict__ dmul, T* __restrict__ dadd, int nblk,
                                                          int KD) {
    const int i = blockIdx.x * NT + threadIdx.x;                          // element of [2][K][D]: dmul, then dadd
    if (i >= 2 * KD) return;
    float s = 0.f;
#pragma unroll 8
    for (int blk = 0; blk < nblk; ++blk) s += part[(long long)blk * 2 * KD + i];
    if (i < KD) dmul[i] = from_f32<T>(s);
    else dadd[i - KD] = from_f32<T>(s);
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
    EGM_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((bcast_add_kernel<T>), grid, dim3(NT), 0, (hipStream_t)s, (const T*)a, (const T*)r, (T*)a, K, L,
                                                 D));
    EGM_CHECK_LAUNCH("bcast_add");
    return EGM_OK;
}

extern "C" int egm_bcast_add_out(int dtype, const void* a, const void* r, void* out, int B, int K, int L, int D, egm_stream_t s) {
    const int rc = check_seq("bcast_add_out", a, r, B, K, L, D);
    if (rc != EGM_OK) return rc;
    EGM_REQUIRE(out && egm_aligned16(a) && egm_aligned16(r) && egm_aligned16(out), "bcast_add_out: null or misaligned pointer");
    const dim3 grid(grid_for((long long)K * L * D / 4), B);
    EGM_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((bcast_add_kernel<T>), grid, dim3(NT), 0, (hipStream_t)s, (const T*)a, (const T*)r, (T*)out, K,
                                                 L, D));
    EGM_CHECK_LAUNCH("bcast_add_out");
    return EGM_OK;
}

extern "C" int egm_group_sum(int dtype, const void* g, void* out, int B, int K, int L, int D, egm_stream_t s) {
    const int rc = check_seq("group_sum", g, out, B, K, L, D);
    if (rc != EGM_OK) return rc;
    EGM_REQUIRE(egm_aligned16(g) && egm_aligned16(out), "group_sum: misaligned pointer");
    const int vec = vec_for(dtype, D);
    const long long total = (long long)B * L * (D / vec);
    if (vec == 8)
        hipLaunchKernelGGL((group_sum_kernel<bf16_t, 8>), dim3(grid_for(total)), dim3(NT), 0, (hipStream_t)s, (const bf16_t*)g, (bf16_t*)out, K, L,
                           D, total);
    else
        EGM_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((group_sum_kernel<T, 4>), dim3(grid_for(total)), dim3(NT), 0, (hipStream_t)s, (const T*)g,
                                                     (T*)out, K, L, D, total));
    EGM_CHECK_LAUNCH("group_sum");
    return EGM_OK;
}

extern "C" long long egm_film_fanout_bwd_workspace(int dtype, int B, int K, int L, int D) {
    if (!(B > 0 && K > 0 && L > 0 && D > 0 && D % 4 == 0 && B < 65536 && (dtype == EGM_F32 || dtype == EGM_BF16)))
        EGM_FAIL(EGM_ERR_ARG, "film_fanout_bwd_workspace: bad args (B %d, K %d, L %d, D %d; D must be a multiple of 4)", B, K, L, D);
    const FanTile f = fan_tile(L, D, vec_for(dtype, D));
    return (long long)B * f.tiles * 2 * K * D * (long long)sizeof(float);
}

extern "C" int egm_film_fanout_bwd(int dtype, const void* g, const void* r, const void* mul, void* dr, void* dmul, void* dadd, void* ws, int B,
                                   int K, int L, int D, egm_stream_t s) {
    const int rc = check_seq("film_fanout_bwd", g, r, B, K, L, D);
    if (rc != EGM_OK) return rc;
    EGM_REQUIRE(mul && dr && dmul && dadd && ws && egm_aligned16(g) && egm_aligned16(r) && egm_aligned16(mul) && egm_aligned16(dr) &&
                egm_aligned16(ws), "film_fanout_bwd: null or misaligned pointer");
    const int vec = vec_for(dtype, D);
    const FanTile f = fan_tile(L, D, vec);
    const long long nblk = (long long)B * f.tiles;
    EGM_REQUIRE(nblk < (1ll << 31) && 2ll * K * D < (1ll << 31), "film_fanout_bwd: too many tiles (B %d, L %d) or K * D too large", B, L);
    if (vec == 8)
        hipLaunchKernelGGL((film_fanout_bwd_kernel<bf16_t, 8>), dim3((unsigned)nblk), dim3(NT), 0, (hipStream_t)s, (const bf16_t*)g,
                           (const bf16_t*)r, (const bf16_t*)mul, (bf16_t*)dr, (float*)ws, K, L, D, f.cw, f.rw, f.tiles);
    else
        EGM_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((film_fanout_bwd_kernel<T, 4>), dim3((unsigned)nblk), dim3(NT), 0, (hipStream_t)s,
                                                     (const T*)g, (const T*)r, (const T*)mul, (T*)dr, (float*)ws, K, L, D, f.cw, f.rw, f.tiles));
    EGM_CHECK_LAUNCH("film_fanout_bwd");
    EGM_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((fan_finalize_kernel<T>), dim3(egm_cdiv(2ll * K * D, NT)), dim3(NT), 0, (hipStream_t)s,
                                                 (const float*)ws, (T*)dmul, (T*)dadd, (int)nblk, K * D));
    EGM_CHECK_LAUNCH("film_fanout_bwd finalize");
    return EGM_OK;
}

extern "C" int egm_sigmoid_affine(float* x, const float* scale, float offset, int N, int C, long long HW, egm_stream_t s) {
    EGM_REQUIRE(x && scale && N > 0 && C > 0 && HW > 0 && HW % 4 == 0 && egm_aligned16(x), "sigmoid_affine: bad args (HW must be a multiple of 4)");
    const long long total4 = (long long)N * C * HW / 4;
    hipLaunchKernelGGL(sigmoid_affine_kernel, dim3(grid_for(total4)), dim3(NT), 0, (hipStream_t)s, x, scale, offset, C, HW, total4);
    EGM_CHECK_LAUNCH("sigmoid_affine");
    return EGM_OK;
}
