// Rectification of an oblique camera frame into the belt plane (contract "rectify v1", include/ore_hip.h): one launch on the caller's
// stream, the nine coefficients of the homography as kernel arguments, no table, no workspace, no host synchronisation.
//   k_rectify_u8  a workgroup renders a 64 x 16 tile of the output, so its source footprint is a compact quadrilateral for L2; a thread
//                 renders RP consecutive pixels of one row (12 bytes) and stores them as aligned 4-byte words with a byte head and tail
//                 where the row's byte offset is no multiple of 4.  The source is gathered directly: the two taps of a source row are 6
//                 consecutive bytes and come with one 8-byte load where those 8 bytes lie inside the frame, byte by byte where not.
// Compiled with -ffp-contract=off, correctly rounded division: every fp32 operation is rounded on its own, as numpy rounds them.
#include <math.h>
#include "ore_common.h"

namespace {

constexpr int RP = 4;                              // pixels per thread
constexpr int RTX = 16, RTY = 16;                  // threads of a workgroup: RTX * RP = 64 pixels by RTY rows
static_assert(RTX * RTY == 256, "one workgroup is 256 threads");
static_assert(RP * 3 % 4 == 0, "a thread's bytes are whole 4-byte words");

struct RectifyArgs {
    const uint8_t* src; uint8_t* dst;
    int32_t hs, ws, ho, wo;
    float m[9];
    uint32_t fill;                                 // byte c = channel c
};

// the two horizontal taps of source row y, three channels each, as 6 bytes in the low 48 bits
__device__ __forceinline__ uint64_t row_taps(const RectifyArgs& a, int y, int xa, int xb, size_t total) {
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

// the three bytes of output pixel (i, j) in bits 0 .. 23
__device__ __forceinline__ uint32_t rectify_pixel(const RectifyArgs& a, int i, int j, size_t total) {
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
    const uint64_t t = row_taps(a, ya, xa, xb, total), b = row_taps(a, yb, xa, xb, total);
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

// grid (ceil(wo / 64), ceil(ho / 16))
__global__ __launch_bounds__(256) void k_rectify_u8(const RectifyArgs a) {
    const int tx = threadIdx.x % RTX, ty = threadIdx.x / RTX;
    const int i = blockIdx.y * RTY + ty, j0 = (blockIdx.x * RTX + tx) * RP;
    if (i >= a.ho || j0 >= a.wo) return;
    const int np = min(RP, a.wo - j0);
    const size_t total = (size_t)a.hs * a.ws * 3;
    uint32_t px[RP];
#pragma unroll
    for (int k = 0; k < RP; ++k) px[k] = k < np ? rectify_pixel(a, i, j0 + k, total) : 0u;
    // 12 bytes, little endian: w[0] = bytes 0 .. 3 and so on; w[3] = 0 pads the funnel below
    const uint32_t w[4] = {px[0] | px[1] << 24, px[1] >> 8 | px[2] << 16, px[2] >> 16 | px[3] << 8, 0u};
    uint8_t* d = a.dst + ((size_t)i * a.wo + j0) * 3;
    const int nb = np * 3, mis = (int)((uintptr_t)d & 3);
    if (mis == 0 && np == RP) {
#pragma unroll
        for (int q = 0; q < 3; ++q) reinterpret_cast<uint32_t*>(d)[q] = w[q];
        return;
    }
    const int head = min((4 - mis) & 3, nb);                  // bytes in front of the first aligned word
    const int words = (nb - head) >> 2;                       // whole aligned words behind them: at most 3
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (k < head) d[k] = (uint8_t)(w[0] >> (8 * k));
#pragma unroll
    for (int q = 0; q < 3; ++q)
        if (q < words) {
            const uint64_t pair = (uint64_t)w[q + 1] << 32 | w[q];
            *reinterpret_cast<uint32_t*>(d + head + 4 * q) = (uint32_t)(pair >> (8 * head));
        }
    const int done = head + 4 * words;                        // the tail: at most 3 bytes
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int at = done + k;
        if (at < nb) {
            const uint32_t lo = at < 4 ? w[0] : (at < 8 ? w[1] : w[2]);
            d[at] = (uint8_t)(lo >> (8 * (at & 3)));
        }
    }
}

}  // namespace

extern "C" int ore_rectify_u8_fwd(const uint8_t* src, int32_t hs, int32_t ws, const float m9_host[9], uint8_t* dst, int32_t ho, int32_t wo,
                                  int32_t fill_rgb, void* stream) {
    ORE_CHECK_ARG(src && dst && m9_host, "ore_rectify_u8_fwd: null pointer");
    ORE_CHECK_ARG(hs >= 1 && hs <= ORE_RECTIFY_MAX_SIDE && ws >= 1 && ws <= ORE_RECTIFY_MAX_SIDE && ho >= 1 && ho <= ORE_RECTIFY_MAX_SIDE &&
                      wo >= 1 && wo <= ORE_RECTIFY_MAX_SIDE,
                  "ore_rectify_u8_fwd: source %dx%d, output %dx%d (sides 1 .. %d)", hs, ws, ho, wo, ORE_RECTIFY_MAX_SIDE);
    for (int k = 0; k < 9; ++k)
        ORE_CHECK_ARG(isfinite(m9_host[k]), "ore_rectify_u8_fwd: coefficient %d is %g (finite)", k, (double)m9_host[k]);
    ORE_CHECK_ARG(fill_rgb >= 0 && fill_rgb <= 0xFFFFFF, "ore_rectify_u8_fwd: fill 0x%x (0 .. 0xFFFFFF)", (unsigned)fill_rgb);
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (size_t)hs * ws * 3, d0 = (uintptr_t)dst, d1 = d0 + (size_t)ho * wo * 3;
    ORE_CHECK_ARG(d1 <= s0 || s1 <= d0, "ore_rectify_u8_fwd: dst overlaps src");
    RectifyArgs a{src, dst, hs, ws, ho, wo, {}, (uint32_t)fill_rgb};
    for (int k = 0; k < 9; ++k) a.m[k] = m9_host[k];
    k_rectify_u8<<<dim3(ceil_div(wo, RTX * RP), ceil_div(ho, RTY)), 256, 0, (hipStream_t)stream>>>(a);
    return ore_launch_status("k_rectify_u8");
}
