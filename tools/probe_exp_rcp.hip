// Accuracy of v_exp_f32 and v_rcp_f32 on the device at hand, over the argument ranges of the fast logistic function of
// csrc/bn_elem.h (logistic<true>: rcp(1 + exp2(-log2(e) * v))) for |v| <= 8.5, against float64 on the host.  The bound `delta` in
// tests/test_gpu_conv_epilogue.py (section C) is derived from TWICE the maxima this prints; it runs no kernel of the library.
//
//   hipcc --offload-arch=gfx950 -O2 tools/probe_exp_rcp.hip -o probe_exp_rcp && ./probe_exp_rcp
//
// exp2: 2^24 evenly spaced arguments in [-12.5, 12.5] (|log2(e) * 8.5| = 12.27).  rcp: 2^24 arguments 1 + 2^t for evenly spaced t in the
// same range, which is every magnitude the logistic's denominator takes, and 2^23 consecutive floats from 1.0 (one whole binade: the
// reciprocal's error depends on the significand alone).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#define CHECK(e)                                                                                   \
    do {                                                                                           \
        hipError_t rc_ = (e);                                                                      \
        if (rc_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(rc_)); return 1; } \
    } while (0)

__global__ void probe(const float* in, float* out, int n, int what) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = what == 0 ? __builtin_amdgcn_exp2f(in[i]) : __builtin_amdgcn_rcpf(in[i]);
}

static int run(const char* name, const std::vector<float>& in, int what) {
    const int n = (int)in.size();
    float *din = nullptr, *dout = nullptr;
    CHECK(hipMalloc(&din, n * sizeof(float)));
    CHECK(hipMalloc(&dout, n * sizeof(float)));
    CHECK(hipMemcpy(din, in.data(), n * sizeof(float), hipMemcpyHostToDevice));
    probe<<<(n + 255) / 256, 256>>>(din, dout, n, what);
    CHECK(hipGetLastError());
    std::vector<float> out(n);
    CHECK(hipMemcpy(out.data(), dout, n * sizeof(float), hipMemcpyDeviceToHost));
    CHECK(hipFree(din));
    CHECK(hipFree(dout));
    double worst = 0, worst_ulp = 0, at = 0;
    for (int i = 0; i < n; ++i) {
        const double want = what == 0 ? exp2((double)in[i]) : 1.0 / (double)in[i];
        const double rel = fabs((double)out[i] - want) / want;
        int e;
        frexp(want, &e);
        const double ulp = fabs((double)out[i] - want) / ldexp(1.0, e - 24);
        if (rel > worst) { worst = rel; at = in[i]; }
        if (ulp > worst_ulp) worst_ulp = ulp;
    }
    printf("%s: %d arguments, max relative error %.4g (at %.9g), max error %.3f ulp\n", name, n, worst, at, worst_ulp);
    return 0;
}

int main() {
    const int n = 1 << 24;
    std::vector<float> t(n), d(n), b(1 << 23);
    for (int i = 0; i < n; ++i) {
        t[i] = (float)(-12.5 + 25.0 * i / (n - 1));
        d[i] = 1.f + (float)exp2((double)t[i]);
    }
    for (int i = 0; i < (1 << 23); ++i) {
        const unsigned u = 0x3f800000u + (unsigned)i;
        memcpy(&b[i], &u, 4);
    }
    if (run("v_exp_f32", t, 0)) return 1;
    if (run("v_rcp_f32 (1 + 2^t)", d, 1)) return 1;
    if (run("v_rcp_f32 (binade [1, 2))", b, 1)) return 1;
    return 0;
}
