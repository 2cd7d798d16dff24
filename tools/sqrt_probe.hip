// Accuracy of v_sqrt_f32 and v_rsq_f32 on gfx950, exhaustively over every float32 in [1, 4): all 2^24 mantissa /
// exponent-parity combinations; the relative error of both repeats every two binades.  Each result is compared with the
// float64 sqrt (1 / sqrt) of the same argument, in ulp of the float32 result's binade.  The worst values are recorded as
// SQRT_MEASURED_ULP and RSQ_MEASURED_ULP (tests/bn_pair_reference.py).
// Build: hipcc -O2 --offload-arch=gfx950 -ffp-contract=off tools/sqrt_probe.hip -o tools/sqrt_probe
// Run:   timeout -k 10 120 tools/sqrt_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

constexpr uint32_t kFirst = 0x3f800000u;  // 1.0f
constexpr uint32_t kCount = 1u << 24;     // up to, not including, 4.0f

__global__ __launch_bounds__(256) void probe_kernel(float *__restrict__ out_sqrt, float *__restrict__ out_rsq) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= kCount) return;
    const float x = __uint_as_float(kFirst + i);
    out_sqrt[i] = __builtin_amdgcn_sqrtf(x);
    out_rsq[i] = __builtin_amdgcn_rsqf(x);
}

#define HIP_OK(call)                                                                   \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) {                                                        \
            std::fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_));            \
            return 1;                                                                  \
        }                                                                              \
    } while (0)

static void report(const char *name, const std::vector<float> &got, bool reciprocal) {
    double worst_ulp = 0.0, worst_rel = 0.0;
    float worst_x = 0.f;
    size_t inexact = 0;
    for (uint32_t i = 0; i < kCount; i++) {
        const uint32_t bits = kFirst + i;
        float x;
        std::memcpy(&x, &bits, 4);
        const double ref = reciprocal ? 1.0 / std::sqrt((double)x) : std::sqrt((double)x);
        // ulp of the binade the exact result lies in: sqrt in [1, 2) -> 2^-23; 1/sqrt in (0.5, 1] -> 2^-24 (2^-23 at 1)
        int e;
        std::frexp(ref, &e);  // ref = f 2^e, f in [0.5, 1)
        const double ulp = std::ldexp(1.0, e - 24);
        const double err = std::fabs((double)got[i] - ref);
        if ((float)ref != got[i]) inexact++;
        if (err / ulp > worst_ulp) {
            worst_ulp = err / ulp;
            worst_rel = err / ref;
            worst_x = x;
        }
    }
    std::printf("%s: worst %.4f ulp at x = %.9g (relative error %.4f u, u = 2^-24); %zu of %u results are not the "
                "correctly rounded value\n",
                name, worst_ulp, (double)worst_x, worst_rel * 16777216.0, inexact, kCount);
}

int main() {
    float *d_sqrt = nullptr, *d_rsq = nullptr;
    HIP_OK(hipMalloc(&d_sqrt, (size_t)kCount * sizeof(float)));
    HIP_OK(hipMalloc(&d_rsq, (size_t)kCount * sizeof(float)));
    hipLaunchKernelGGL(probe_kernel, dim3(kCount / 256), dim3(256), 0, 0, d_sqrt, d_rsq);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    std::vector<float> h_sqrt(kCount), h_rsq(kCount);
    HIP_OK(hipMemcpy(h_sqrt.data(), d_sqrt, (size_t)kCount * sizeof(float), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(h_rsq.data(), d_rsq, (size_t)kCount * sizeof(float), hipMemcpyDeviceToHost));
    report("v_sqrt_f32", h_sqrt, false);
    report("v_rsq_f32", h_rsq, true);
    HIP_OK(hipFree(d_sqrt));
    HIP_OK(hipFree(d_rsq));
    return 0;
}
