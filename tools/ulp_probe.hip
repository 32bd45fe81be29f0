// Worst observed ULP error of the device's expf / logf / powf / sqrtf / division against double, at the arguments the loss, target and
// ROI-loss kernels of csrc/ore_train.hip feed them (tests/trainloss_ref.py charges twice these figures, rounded up, per call).
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tools/ulp_probe.hip -o tools/bin/ulp_probe && tools/bin/ulp_probe
// (the flags of csrc/Makefile for ore_train: nothing relaxes division or sqrtf).  One line per sweep: worst error in ULPs of the fp32
// result and the argument it was seen at.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

enum Fn { F_EXP, F_LOG, F_POW, F_SQRT, F_DIV, F_SIGMOID };

__global__ void k_eval(int fn, const float* __restrict__ x, float e, float* __restrict__ y, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    float r = 0.f;
    switch (fn) {
        case F_EXP: r = expf(v); break;
        case F_LOG: r = logf(v); break;
        case F_POW: r = powf(v, e); break;
        case F_SQRT: r = sqrtf(v); break;
        case F_DIV: r = e / v; break;
        case F_SIGMOID: r = 1.0f / (1.0f + expf(-v)); break;
    }
    y[i] = r;
}

static double ref_of(int fn, double v, double e) {
    switch (fn) {
        case F_EXP: return std::exp(v);
        case F_LOG: return std::log(v);
        case F_POW: return std::pow(v, e);
        case F_SQRT: return std::sqrt(v);
        case F_DIV: return e / v;
        default: return 1.0 / (1.0 + std::exp(-v));
    }
}

static double ulp_of(double r) {           // spacing of fp32 at |r| (normal range)
    int ex;
    std::frexp(std::fabs(r), &ex);         // |r| = f * 2^ex, f in [0.5, 1)
    return std::ldexp(1.0, ex - 24);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double urand() {                    // xorshift64*, [0, 1)
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}

static int sweep(const char* name, int fn, double lo, double hi, bool logu, float e) {
    const int n = 1 << 22;
    std::vector<float> x(n), y(n);
    for (int i = 0; i < n; ++i) {
        const double t = urand();
        x[i] = (float)(logu ? std::exp(std::log(lo) + t * (std::log(hi) - std::log(lo))) : lo + t * (hi - lo));
    }
    float *dx = nullptr, *dy = nullptr;
    if (hipMalloc(&dx, n * sizeof(float)) != hipSuccess || hipMalloc(&dy, n * sizeof(float)) != hipSuccess) return 1;
    if (hipMemcpy(dx, x.data(), n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return 1;
    hipLaunchKernelGGL(k_eval, dim3((n + 255) / 256), dim3(256), 0, 0, fn, dx, e, dy, n);
    if (hipMemcpy(y.data(), dy, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    (void)hipFree(dx); (void)hipFree(dy);
    double worst = 0.0, at = 0.0;
    for (int i = 0; i < n; ++i) {
        const double r = ref_of(fn, (double)x[i], (double)e);
        if (r == 0.0 || !std::isfinite(r) || std::fabs(r) < 1.2e-38) continue;
        const double err = std::fabs((double)y[i] - r) / ulp_of(r);
        if (!(err <= worst)) { worst = err; at = x[i]; }
    }
    printf("%-34s worst %.4f ulp at %.9g\n", name, worst, at);
    return 0;
}

int main() {
    int rc = 0;
    rc |= sweep("expf   [-87, 88]", F_EXP, -87.0, 88.0, false, 0.f);
    rc |= sweep("expf   [-20, 20]", F_EXP, -20.0, 20.0, false, 0.f);
    rc |= sweep("expf   [-1, 0]", F_EXP, -1.0, 0.0, false, 0.f);
    rc |= sweep("logf   [1e-5, 16] log-uniform", F_LOG, 1e-5, 16.0, true, 0.f);
    rc |= sweep("logf   [0.5, 2]", F_LOG, 0.5, 2.0, false, 0.f);
    rc |= sweep("logf   [0.99, 1.01]", F_LOG, 0.99, 1.01, false, 0.f);
    const float es[] = {1.0f, 2.0f, 4.0f};
    for (float e : es) {
        char nm[64];
        snprintf(nm, sizeof nm, "powf(x, %g) [0, 1]", e);
        rc |= sweep(nm, F_POW, 0.0, 1.0, false, e);
        snprintf(nm, sizeof nm, "powf(x, %g) [1e-5, 1] log-uniform", e);
        rc |= sweep(nm, F_POW, 1e-5, 1.0, true, e);
    }
    rc |= sweep("sqrtf  [1e-3, 1e7] log-uniform", F_SQRT, 1e-3, 1e7, true, 0.f);
    rc |= sweep("1 / x  [1e-6, 1e6] log-uniform", F_DIV, 1e-6, 1e6, true, 1.0f);
    rc |= sweep("3.7 / x [1e-6, 1e6] log-uniform", F_DIV, 1e-6, 1e6, true, 3.7f);
    rc |= sweep("1 / (1 + expf(-x)) [-20, 20]", F_SIGMOID, -20.0, 20.0, false, 0.f);
    return rc;
}
