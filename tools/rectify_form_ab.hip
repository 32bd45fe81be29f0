// A/B of the rectify kernel's forms (a measurement aid, not part of the library): A the direct gather of csrc/ore_rectify.hip,
// B the same arithmetic with the source reads replaced by register values (the VALU floor), C the workgroup's source footprint staged
// in LDS and the taps read from there.  hipEvents over `launches` launches, median of 5 rounds; A and C are compared byte for byte.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

constexpr int RP = 4, RTX = 16, RTY = 16;
constexpr int LDS_BYTES = 32768;

struct Args {
    const uint8_t* src; uint8_t* dst;
    int32_t hs, ws, ho, wo;
    float m[9];
    uint32_t fill;
};

__device__ __forceinline__ uint64_t row_taps(const Args& a, int y, int xa, int xb, size_t total) {
    const size_t o = ((size_t)y * a.ws + xa) * 3;
    if (xb == xa + 1 && o + 8 <= total) {
        uint64_t v;
        __builtin_memcpy(&v, a.src + o, 8);
        return v;
    }
    const uint8_t* p = a.src + o;
    const uint8_t* q = a.src + ((size_t)y * a.ws + xb) * 3;
    return (uint64_t)p[0] | (uint64_t)p[1] << 8 | (uint64_t)p[2] << 16 | (uint64_t)q[0] << 24 | (uint64_t)q[1] << 32 | (uint64_t)q[2] << 40;
}

struct Stage { const uint8_t* lds; int x0, y0, x1, y1, pitch; bool on; };

__device__ __forceinline__ uint64_t lds_taps(const Stage& s, int y, int xa, int xb) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(s.lds);
    auto six = [&](int x) {
        const int pos = (y - s.y0) * s.pitch + (x - s.x0) * 3, k = pos >> 2, sh = (pos & 3) * 8;
        const uint64_t lo = (uint64_t)w[k + 1] << 32 | w[k];
        const uint64_t v = sh ? (lo >> sh | (uint64_t)w[k + 2] << (64 - sh)) : lo;
        return v;
    };
    if (xb == xa + 1) return six(xa);
    return (six(xa) & 0xFFFFFF) | (six(xb) & 0xFFFFFF) << 24;
}

template <int FORM>
__device__ __forceinline__ uint32_t pixel(const Args& a, int i, int j, size_t total, const Stage& st) {
    const float xo = (float)j + 0.5f, yo = (float)i + 0.5f;
    const float X = (a.m[0] * xo + a.m[1] * yo) + a.m[2];
    const float Y = (a.m[3] * xo + a.m[4] * yo) + a.m[5];
    const float Z = (a.m[6] * xo + a.m[7] * yo) + a.m[8];
    const float u = X / Z - 0.5f, v = Y / Z - 0.5f;
    const bool inside = __builtin_isfinite(X) && __builtin_isfinite(Y) && __builtin_isfinite(Z) && Z > 0.0f && u >= -0.5f &&
                        u <= (float)a.ws - 0.5f && v >= -0.5f && v <= (float)a.hs - 0.5f;
    if (!inside) return a.fill;
    const int U = (int)floorf(u * 256.0f + 0.5f), V = (int)floorf(v * 256.0f + 0.5f);
    const int x0 = U >> 8, y0 = V >> 8;
    const uint32_t fx = U & 255, fy = V & 255;
    const int xa = min(max(x0, 0), a.ws - 1), xb = min(max(x0 + 1, 0), a.ws - 1);
    const int ya = min(max(y0, 0), a.hs - 1), yb = min(max(y0 + 1, 0), a.hs - 1);
    uint64_t t, b;
    if (FORM == 1) {
        t = (uint64_t)(uint32_t)(xa * 2654435761u) << 16 | (uint32_t)ya;
        b = (uint64_t)(uint32_t)(xb * 2246822519u) << 16 | (uint32_t)yb;
    } else if (FORM == 2 && st.on && xa >= st.x0 && xb <= st.x1 && ya >= st.y0 && yb <= st.y1) {
        t = lds_taps(st, ya, xa, xb);
        b = lds_taps(st, yb, xa, xb);
    } else {
        t = row_taps(a, ya, xa, xb, total);
        b = row_taps(a, yb, xa, xb, total);
    }
    uint32_t out = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t pa = (uint32_t)(t >> (8 * c)) & 255, pb = (uint32_t)(t >> (8 * c + 24)) & 255;
        const uint32_t pc = (uint32_t)(b >> (8 * c)) & 255, pd = (uint32_t)(b >> (8 * c + 24)) & 255;
        const uint32_t top = pa * (256 - fx) + pb * fx, bot = pc * (256 - fx) + pd * fx;
        out |= ((top * (256 - fy) + bot * fy + 32768) >> 16) << (8 * c);
    }
    return out;
}

__device__ __forceinline__ bool corner(const Args& a, int i, int j, float& u, float& v) {
    const float xo = (float)j + 0.5f, yo = (float)i + 0.5f;
    const float X = (a.m[0] * xo + a.m[1] * yo) + a.m[2];
    const float Y = (a.m[3] * xo + a.m[4] * yo) + a.m[5];
    const float Z = (a.m[6] * xo + a.m[7] * yo) + a.m[8];
    u = X / Z - 0.5f;
    v = Y / Z - 0.5f;
    return __builtin_isfinite(u) && __builtin_isfinite(v) && Z > 0.0f && fabsf(u) < 1e6f && fabsf(v) < 1e6f;
}

template <int FORM>
__global__ __launch_bounds__(256) void k_rectify(const Args a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[FORM == 2 ? LDS_BYTES + 16 : 16];
    const size_t total = (size_t)a.hs * a.ws * 3;
    Stage st{lds, 0, 0, -1, -1, 0, false};
    if (FORM == 2) {
        const int ti = blockIdx.y * RTY, tj = blockIdx.x * RTX * RP;
        const int i1 = min(ti + RTY, a.ho) - 1, j1 = min(tj + RTX * RP, a.wo) - 1;
        float u[4], v[4];
        bool ok = corner(a, ti, tj, u[0], v[0]);
        ok &= corner(a, ti, j1, u[1], v[1]);
        ok &= corner(a, i1, tj, u[2], v[2]);
        ok &= corner(a, i1, j1, u[3], v[3]);
        if (ok) {
            const float ulo = fminf(fminf(u[0], u[1]), fminf(u[2], u[3])), uhi = fmaxf(fmaxf(u[0], u[1]), fmaxf(u[2], u[3]));
            const float vlo = fminf(fminf(v[0], v[1]), fminf(v[2], v[3])), vhi = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
            st.x0 = min(max((int)floorf(ulo) - 1, 0), a.ws - 1);
            st.x1 = min(max((int)floorf(uhi) + 2, 0), a.ws - 1);
            st.y0 = min(max((int)floorf(vlo) - 1, 0), a.hs - 1);
            st.y1 = min(max((int)floorf(vhi) + 2, 0), a.hs - 1);
            const int bw = st.x1 - st.x0 + 1, bh = st.y1 - st.y0 + 1;
            st.pitch = (bw * 3 + 3) / 4 * 4 + 4;                       // a row's words, and one more for the funnel's third read
            st.on = (size_t)st.pitch * bh + 8 <= LDS_BYTES;
        }
        if (st.on) {
            const int wpr = st.pitch / 4, bh = st.y1 - st.y0 + 1;
            uint32_t* w = reinterpret_cast<uint32_t*>(lds);
            for (int idx = threadIdx.x; idx < wpr * bh; idx += 256) {
                const int r = idx / wpr, k = idx - r * wpr;
                const size_t o = ((size_t)(st.y0 + r) * a.ws + st.x0) * 3 + (size_t)k * 4;
                uint32_t val = 0;
                if (o + 4 <= total) __builtin_memcpy(&val, a.src + o, 4);
                else
                    for (int q = 0; q < 4; ++q)
                        if (o + q < total) val |= (uint32_t)a.src[o + q] << (8 * q);
                w[idx] = val;
            }
            if (threadIdx.x < 2) w[wpr * bh + threadIdx.x] = 0;
        }
        __syncthreads();
    }
    const int tx = threadIdx.x % RTX, ty = threadIdx.x / RTX;
    const int i = blockIdx.y * RTY + ty, j0 = (blockIdx.x * RTX + tx) * RP;
    if (i >= a.ho || j0 >= a.wo) return;
    const int np = min(RP, a.wo - j0);
    uint32_t px[RP];
#pragma unroll
    for (int k = 0; k < RP; ++k) px[k] = k < np ? pixel<FORM>(a, i, j0 + k, total, st) : 0u;
    const uint32_t w[4] = {px[0] | px[1] << 24, px[1] >> 8 | px[2] << 16, px[2] >> 16 | px[3] << 8, 0u};
    uint8_t* d = a.dst + ((size_t)i * a.wo + j0) * 3;
    const int nb = np * 3, mis = (int)((uintptr_t)d & 3);
    if (mis == 0 && np == RP) {
#pragma unroll
        for (int q = 0; q < 3; ++q) reinterpret_cast<uint32_t*>(d)[q] = w[q];
        return;
    }
    const int head = min((4 - mis) & 3, nb);
    const int words = (nb - head) >> 2;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (k < head) d[k] = (uint8_t)(w[0] >> (8 * k));
#pragma unroll
    for (int q = 0; q < 3; ++q)
        if (q < words) {
            const uint64_t pair = (uint64_t)w[q + 1] << 32 | w[q];
            *reinterpret_cast<uint32_t*>(d + head + 4 * q) = (uint32_t)(pair >> (8 * head));
        }
    const int done = head + 4 * words;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int at = done + k;
        if (at < nb) {
            const uint32_t lo = at < 4 ? w[0] : (at < 8 ? w[1] : w[2]);
            d[at] = (uint8_t)(lo >> (8 * (at & 3)));
        }
    }
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s -> %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

template <int FORM>
static int timed(const Args& a, int launches, double* med_us) {
    const dim3 grid((a.wo + RTX * RP - 1) / (RTX * RP), (a.ho + RTY - 1) / RTY);
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (int k = 0; k < 50; ++k) k_rectify<FORM><<<grid, 256>>>(a);
    CK(hipDeviceSynchronize());
    std::vector<double> per;
    for (int r = 0; r < 5; ++r) {
        CK(hipEventRecord(e0));
        for (int k = 0; k < launches; ++k) k_rectify<FORM><<<grid, 256>>>(a);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        per.push_back(ms * 1e3 / launches);
    }
    CK(hipGetLastError());
    std::sort(per.begin(), per.end());
    *med_us = per[2];
    printf("    rounds %.2f .. %.2f us\n", per[0], per[4]);
    return 0;
}

int main() {
    const float M[2][9] = {{0.416666657f, -0.510638297f, 560.f, 0.f, 0.116233252f, 300.f, 0.f, -0.000531914877f, 1.f},
                           {0.416666657f, -0.510638297f, 1120.f, 0.f, 0.116233252f, 600.f, 0.f, -0.000265957438f, 1.f}};
    for (int s = 0; s < 2; ++s) {
        const int h = 1080 << s, w = 1920 << s;
        const size_t n = (size_t)h * w * 3;
        std::vector<uint8_t> host(n), outA(n), outC(n);
        uint32_t x = 12345u + s;
        for (size_t k = 0; k < n; ++k) { x = x * 1664525u + 1013904223u; host[k] = (uint8_t)(x >> 24); }
        uint8_t *src, *dst;
        CK(hipMalloc(&src, n));
        CK(hipMalloc(&dst, n));
        CK(hipMemcpy(src, host.data(), n, hipMemcpyHostToDevice));
        Args a{src, dst, h, w, h, w, {}, 0x030201u};
        memcpy(a.m, M[s], sizeof(a.m));
        double us[3];
        printf("%dx%d -> %dx%d\n", h, w, h, w);
        printf("  A direct gather\n");
        if (timed<0>(a, 200, &us[0])) return 2;
        CK(hipMemcpy(outA.data(), dst, n, hipMemcpyDeviceToHost));
        printf("  B no source reads (VALU floor; wrong bytes by design)\n");
        if (timed<1>(a, 200, &us[1])) return 2;
        CK(hipMemset(dst, 0, n));
        printf("  C LDS-staged footprint\n");
        if (timed<2>(a, 200, &us[2])) return 2;
        CK(hipMemcpy(outC.data(), dst, n, hipMemcpyDeviceToHost));
        const bool same = memcmp(outA.data(), outC.data(), n) == 0;
        printf("  median us: A %.2f  B %.2f  C %.2f   C equals A: %s\n", us[0], us[1], us[2], same ? "yes" : "NO");
        CK(hipFree(src));
        CK(hipFree(dst));
        if (!same) return 1;
    }
    return 0;
}
