// Host parts of csrc/ore_optim.hip under AddressSanitizer / UBSan, as a stand-alone program: argument checking of the entry points,
// the partial tables of ore_grad_norm_plan and their sizing.  No kernel is launched (every call below returns before its launch), so
// it runs on a machine without a GPU.  Build and run from the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Iinclude \
//         faster-orefsdet_amd/csrc/ore_optim.hip -x hip faster-orefsdet_amd/csrc/ore_util.cpp tools/optim_host_check.cpp \
//         -o optim_host_check -ldl && ./optim_host_check
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "ore_hip.h"

#define CHECK(c)                                                             \
    do {                                                                     \
        if (!(c)) {                                                          \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c);   \
            return 1;                                                        \
        }                                                                    \
    } while (0)

int main() {
    int32_t G = 0, W = 0;
    CHECK(ore_grad_norm_geometry(nullptr, &W) == ORE_EINVAL);
    CHECK(ore_grad_norm_geometry(&G, &W) == ORE_OK && G > 0 && W > 0);
    // tables: every size class of the kernels' geometry, and a few thousand one-element parameters
    std::vector<int64_t> numel = {1, 255, 256, 257, 256ll * G, 256ll * G + 1, 256ll * G * W + 1, 3, 43};
    for (int i = 0; i < 3000; ++i) numel.push_back(1 + (i * 7919) % 5000);
    const int32_t P = (int32_t)numel.size();
    int64_t nc = 0, np = 0;
    CHECK(ore_grad_norm_plan(numel.data(), P, nullptr, nullptr, 0, &nc, &np) == ORE_OK);
    int64_t wc = 0, wp = 0;
    for (int64_t n : numel) {
        const int64_t c = (n + 255) / 256;
        wc += c;
        wp += (c + G - 1) / G;
    }
    CHECK(nc == wc && np == wp);
    // heap blocks of exactly the planned size: a write past either end is an ASan report
    std::vector<int32_t> part0((size_t)P + 1, -1), part_param((size_t)np, -1);
    CHECK(ore_grad_norm_plan(numel.data(), P, part0.data(), part_param.data(), np, &nc, &np) == ORE_OK);
    CHECK(part0[0] == 0 && part0[P] == np);
    for (int32_t i = 0; i < P; ++i) {
        const int64_t c = (numel[i] + 255) / 256;
        CHECK(part0[i + 1] - part0[i] == (c + G - 1) / G);
        for (int32_t q = part0[i]; q < part0[i + 1]; ++q) CHECK(part_param[q] == i);
    }
    // a table one entry short is refused, not overrun
    std::vector<int32_t> shorter((size_t)np - 1, -1);
    CHECK(ore_grad_norm_plan(numel.data(), P, part0.data(), shorter.data(), np - 1, &nc, &np) == ORE_EINVAL);
    CHECK(ore_grad_norm_plan(numel.data(), P, nullptr, shorter.data(), -1, &nc, &np) == ORE_EINVAL);
    CHECK(ore_grad_norm_plan(nullptr, P, nullptr, nullptr, 0, &nc, &np) == ORE_EINVAL);
    CHECK(ore_grad_norm_plan(numel.data(), 0, nullptr, nullptr, 0, &nc, &np) == ORE_EINVAL);
    CHECK(ore_grad_norm_plan(numel.data(), P, nullptr, nullptr, 0, nullptr, &np) == ORE_EINVAL);
    std::vector<int64_t> bad = {5, 0, 7};
    CHECK(ore_grad_norm_plan(bad.data(), 3, nullptr, nullptr, 0, &nc, &np) == ORE_EINVAL);
    bad[1] = -3;
    CHECK(ore_grad_norm_plan(bad.data(), 3, nullptr, nullptr, 0, &nc, &np) == ORE_EINVAL);
    std::vector<int64_t> huge(3, (1ll << 38) - 1);                       // 3 x 2^30 chunks: past the 2^31 a grid can index
    CHECK(ore_grad_norm_plan(huge.data(), 3, nullptr, nullptr, 0, &nc, &np) == ORE_EINVAL);
    huge[0] = 1ll << 38;
    CHECK(ore_grad_norm_plan(huge.data(), 1, nullptr, nullptr, 0, &nc, &np) == ORE_EINVAL);
    // the launching entry points refuse what they can check on the host, before any launch (the pointers are never dereferenced here)
    float* f = reinterpret_cast<float*>(0x1000);
    const int64_t* t64 = reinterpret_cast<const int64_t*>(0x1000);
    const int32_t* t32 = reinterpret_cast<const int32_t*>(0x1000);
    CHECK(ore_grad_norm_fwd(nullptr, P, t64, t64, t32, t32, np, 2, 0, 1.f, 1.f, f, f, f, f, f, nullptr) == ORE_EINVAL);
    CHECK(ore_grad_norm_fwd(f, P, t64, t64, t32, t32, np, 2, 0, 1.f, 1.f, f, f, f, nullptr, f, nullptr) == ORE_EINVAL);
    CHECK(ore_grad_norm_fwd(f, 0, t64, t64, t32, t32, np, 2, 0, 1.f, 1.f, f, f, f, f, f, nullptr) == ORE_EINVAL);
    CHECK(ore_grad_norm_fwd(f, P, t64, t64, t32, t32, P - 1, 2, 0, 1.f, 1.f, f, f, f, f, f, nullptr) == ORE_EINVAL);
    CHECK(ore_grad_norm_fwd(f, P, t64, t64, t32, t32, 1ll << 31, 2, 0, 1.f, 1.f, f, f, f, f, f, nullptr) == ORE_EINVAL);
    CHECK(ore_grad_norm_fwd(f, P, t64, t64, t32, t32, np, 3, 0, 1.f, 1.f, f, f, f, f, f, nullptr) == ORE_EINVAL);
    CHECK(ore_grad_norm_fwd(f, P, t64, t64, t32, t32, np, 2, 1, 1.f, 1.f, f, f, f, f, nullptr, nullptr) == ORE_EINVAL);
    CHECK(ore_sgd_step_clipnorm_fwd(nullptr, f, f, nc, f, f, t32, t64, t64, f, nullptr, 1.f, .9f, 1.f, 1.f, 0, nullptr) == ORE_EINVAL);
    CHECK(ore_sgd_step_clipnorm_fwd(f, f, f, 0, f, f, t32, t64, t64, f, nullptr, 1.f, .9f, 1.f, 1.f, 0, nullptr) == ORE_EINVAL);
    CHECK(ore_sgd_step_clipnorm_fwd(f, f, f, 1ll << 31, f, f, t32, t64, t64, f, nullptr, 1.f, .9f, 1.f, 1.f, 0, nullptr) == ORE_EINVAL);
    CHECK(ore_sgd_step_clipnorm_fwd(f, f, f, nc, f, f, nullptr, t64, t64, f, nullptr, 1.f, .9f, 1.f, 1.f, 0, nullptr) == ORE_EINVAL);
    CHECK(ore_sgd_step_clipnorm_fwd(f, f, f, nc, f, f, t32, t64, t64, f, nullptr, 1.f, 0.f, 1.f, 1.f, 1, nullptr) == ORE_EINVAL);
    CHECK(ore_last_error() != nullptr && ore_last_error()[0] != 0);
    printf("optim_host_check: %d parameters, %lld chunks, %lld partials, G=%d W=%d: ok\n", P, (long long)nc, (long long)np, G, W);
    return 0;
}
