// Window arithmetic of the 8-bit antialiased BILINEAR resample (Pillow's ImagingResample), shared by the host planner
// (ore_resize_plan.cpp) and the launcher (ore_resize.hip), which sizes a tile's LDS from the first and last window of the tile.
// Also what the whole-image kernels (ore_resize.hip) and the support-crop kernels (ore_support.hip, ore_support_plan.cpp) have in
// common: the side range, the layout of a size pair's tables, the tile, its block width and its LDS sizing, the 16-byte staging
// address, the guarded granule, the tap loops, the final clip, the word-or-bytes store and the horizontal pass of the workspace form.
// The two fused tile kernels (k_resize_fused, k_support_fused) string the same leaves together but stay two bodies: every shared
// form of them that was measured made the resize of 1080x1920 -> 562x1000 slower than its own body (profiles/EXPERIMENTS.md).
#pragma once
#include <stddef.h>
#include <stdint.h>

#define ORE_RESIZE_PREC 22           // fractional bits of the fixed-point coefficients
#define ORE_RESIZE_MAX_SIDE 8192
#define ORE_RESIZE_TW 64             // output tile of a one-launch block: 16 rows x 64 columns
#define ORE_RESIZE_TH 16
// threads of a one-launch block: a tile of a 3x reduction stages ~60 source rows, and with 1080x1920 -> 320x569 only 180 tiles exist for
// 256 CUs, so the block's own width is what hides its latencies (measured 14.3 / 9.7 / 8.1 us at 256 / 512 / 1024; profiles/EXPERIMENTS.md)
#define ORE_RESIZE_NTF 1024
#define ORE_RESIZE_LDS_BYTES (64 * 1024)   // dynamic LDS a launch may ask for without opting in to more

// a side of a frame, a rectangle, an output or a canvas
static inline bool ore_resize_side_ok(int32_t n) { return n >= 1 && n <= ORE_RESIZE_MAX_SIDE; }

struct ore_resize_axis {
    double scale, filterscale, support;
    int32_t ksize;
};

static inline ore_resize_axis ore_resize_axis_of(int32_t in, int32_t out) {
    ore_resize_axis a;
    a.scale = (double)in / out;
    a.filterscale = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = 1.0 * a.filterscale;                     // the triangle filter's support is 1
    a.ksize = (int32_t)__builtin_ceil(a.support) * 2 + 1;
    return a;
}

// window of output index xx: source indices [xmin, xmin + count), 1 <= count <= ksize, inside [0, in).  Both ends are
// non-decreasing in xx, so a run of outputs reads the sources from its first window's xmin to its last window's end.
static inline void ore_resize_window(const ore_resize_axis& a, int32_t in, int32_t xx, int32_t* xmin, int32_t* count) {
    const double center = (xx + 0.5) * a.scale;
    int32_t lo = (int32_t)(center - a.support + 0.5);
    if (lo < 0) lo = 0;
    int32_t hi = (int32_t)(center + a.support + 0.5);
    if (hi > in) hi = in;
    *xmin = lo;
    *count = hi - lo;
}

// widest source span (last window's end - first window's start) of any run of outputs that one tile covers.  The first tile holds
// the outputs [0, first), every later one the next `tile`: first == tile for tiles that start at output 0 (the whole-image resize);
// a support crop's tiles are cut on its canvas, so the first one of its destination rectangle is a partial one.
static inline int32_t ore_resize_max_tile_span(int32_t in, int32_t out, int32_t tile, int32_t first) {
    const ore_resize_axis ax = ore_resize_axis_of(in, out);
    int32_t worst = 0;
    for (int32_t t0 = 0, t1 = first; t0 < out; t0 = t1, t1 += tile) {
        const int32_t last = (t1 < out ? t1 : out) - 1;
        int32_t lo, n0, lo1, n1;
        ore_resize_window(ax, in, t0, &lo, &n0);
        ore_resize_window(ax, in, last, &lo1, &n1);
        if (lo1 + n1 - lo > worst) worst = lo1 + n1 - lo;
    }
    return worst;
}

// LDS of a one-launch block: R = source / intermediate rows held, S = bytes of one staged source row (a multiple of 16), bytes = the
// whole carve: x coefficients [TW][ksx rounded up to 4] | y coefficients [TH][ksy] | x bounds | y bounds | intermediate [3][R][TW] |
// staged rows [R][S] + 32 bytes a last row's padded taps may read.
struct ore_resize_fused_lds { int32_t R, S; size_t bytes; };

static inline ore_resize_fused_lds ore_resize_fused_lds_of(int32_t h, int32_t w, int32_t nh, int32_t nw, int32_t first_y, int32_t first_x) {
    const int32_t TW = ORE_RESIZE_TW, TH = ORE_RESIZE_TH;
    const int32_t ksx = ore_resize_axis_of(w, nw).ksize, ksy = ore_resize_axis_of(h, nh).ksize;
    ore_resize_fused_lds l;
    l.R = ore_resize_max_tile_span(h, nh, TH, first_y);
    l.S = ((ore_resize_max_tile_span(w, nw, TW, first_x) * 3 + 15 + 15) & ~15);       // a row starts up to 15 bytes into its first granule
    l.bytes = (size_t)(TW * ((ksx + 3) & ~3) + ((TH * ksy + 3) & ~3) + TW * 2 + TH * 2) * 4 + (size_t)3 * l.R * TW + (size_t)l.R * l.S + 32;
    return l;
}

// the same for a resample whose output lands at (dy0, dx0) of a canvas that is cut into tiles from its own corner (a support crop)
static inline ore_resize_fused_lds ore_resize_fused_lds_at(int32_t h, int32_t w, int32_t nh, int32_t nw, int32_t dy0, int32_t dx0) {
    return ore_resize_fused_lds_of(h, w, nh, nw, ORE_RESIZE_TH - dy0 % ORE_RESIZE_TH, ORE_RESIZE_TW - dx0 % ORE_RESIZE_TW);
}

// The tables of one size pair, one run of int32 words: x bounds [nw][2] | y bounds [nh][2] | x coefficients [nw][ksx] | y coefficients
// [nh][ksy].  xb .. ky are the word offsets of the four inside the run, total its length.
struct ore_resize_layout { int32_t ksx, ksy; size_t xb, yb, kx, ky, total; };

static inline ore_resize_layout ore_resize_layout_of(int32_t h, int32_t w, int32_t nh, int32_t nw) {
    ore_resize_layout t;
    t.ksx = ore_resize_axis_of(w, nw).ksize, t.ksy = ore_resize_axis_of(h, nh).ksize;
    t.xb = 0, t.yb = t.xb + (size_t)nw * 2, t.kx = t.yb + (size_t)nh * 2, t.ky = t.kx + (size_t)nw * t.ksx;
    t.total = t.ky + (size_t)nh * t.ksy;
    return t;
}

#ifdef __HIPCC__
__device__ __forceinline__ uint32_t ore_resize_clip8(int32_t acc) {
    const int32_t v = acc >> ORE_RESIZE_PREC;
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// the four bytes src[p .. p + 4) as a word; bytes outside [lo, hi) read as 0 without being touched
__device__ __forceinline__ uint32_t ore_resize_guarded_word(const uint8_t* src, int64_t p, int64_t lo, int64_t hi) {
    uint32_t wd = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (p + b >= lo && p + b < hi) wd |= (uint32_t)src[p + b] << (b * 8);
    return wd;
}

// Staging a run of source bytes that starts at offset row_lo of a buffer whose base lies `al` bytes into a 16-byte granule: the v-th
// granule of the run is the 16 bytes at this offset (of the base), which is 16-byte aligned as an address, so that the run's first
// byte lands (row_lo + al) & 15 bytes into its staged row.
__device__ __forceinline__ int64_t ore_resize_granule_at(int64_t row_lo, int al, int v) {
    return ((row_lo + al) & ~(int64_t)15) - al + (int64_t)v * 16;
}

// the 16 bytes at offset p of src; only the bytes inside [lo, hi) are touched, the others read as 0
__device__ __forceinline__ uint4 ore_resize_granule_load(const uint8_t* src, int64_t p, int64_t lo, int64_t hi) {
    if (p >= lo && p + 16 <= hi) return *reinterpret_cast<const uint4*>(src + p);
    return make_uint4(ore_resize_guarded_word(src, p, lo, hi), ore_resize_guarded_word(src, p + 4, lo, hi),
                      ore_resize_guarded_word(src, p + 8, lo, hi), ore_resize_guarded_word(src, p + 12, lo, hi));
}

// Horizontal taps of one output pixel from a staged row in LDS: the window is `groups` * 4 taps = groups * 12 contiguous bytes that
// start at byte `at` of s_src.  They are read as aligned words, shifted to the window's first byte (v_alignbyte), and consumed four
// taps = three words at a time against four coefficients; k is zero past the window's count, whatever bytes lie there.
__device__ __forceinline__ void ore_resize_htaps_lds(const uint8_t* s_src, int at, int groups, const int32_t* k, int32_t& acc0, int32_t& acc1,
                                                     int32_t& acc2) {
    const int sh = at & 3;
    const uint32_t* q = reinterpret_cast<const uint32_t*>(s_src + (at - sh));
    acc0 = acc1 = acc2 = 1 << (ORE_RESIZE_PREC - 1);
    uint32_t lo = q[0];
    for (int g = 0; g < groups; ++g) {
        const uint32_t w1 = q[3 * g + 1], w2 = q[3 * g + 2], w3 = q[3 * g + 3];
        const uint32_t d0 = __builtin_amdgcn_alignbyte(w1, lo, sh), d1 = __builtin_amdgcn_alignbyte(w2, w1, sh),
                       d2 = __builtin_amdgcn_alignbyte(w3, w2, sh);
        lo = w3;
        const int4 kk = *reinterpret_cast<const int4*>(k + 4 * g);
        acc0 += (int32_t)(d0 & 255) * kk.x + (int32_t)(d0 >> 24) * kk.y + (int32_t)((d1 >> 16) & 255) * kk.z + (int32_t)((d2 >> 8) & 255) * kk.w;
        acc1 += (int32_t)((d0 >> 8) & 255) * kk.x + (int32_t)(d1 & 255) * kk.y + (int32_t)(d1 >> 24) * kk.z + (int32_t)((d2 >> 16) & 255) * kk.w;
        acc2 += (int32_t)((d0 >> 16) & 255) * kk.x + (int32_t)((d1 >> 8) & 255) * kk.y + (int32_t)(d2 & 255) * kk.z + (int32_t)(d2 >> 24) * kk.w;
    }
}

// Vertical taps of four neighbouring columns of one plane of the LDS intermediate (rows `stride` bytes apart, col 4-byte aligned)
__device__ __forceinline__ void ore_resize_vtaps_lds(const uint8_t* col, int stride, int cnt, const int32_t* k, int32_t& a0, int32_t& a1,
                                                     int32_t& a2, int32_t& a3) {
    a0 = a1 = a2 = a3 = 1 << (ORE_RESIZE_PREC - 1);
    for (int t = 0; t < cnt; ++t) {
        const uint32_t wd = *reinterpret_cast<const uint32_t*>(col + t * stride);
        const int32_t kk = k[t];
        a0 += (int32_t)(wd & 255) * kk;
        a1 += (int32_t)((wd >> 8) & 255) * kk;
        a2 += (int32_t)((wd >> 16) & 255) * kk;
        a3 += (int32_t)(wd >> 24) * kk;
    }
}

// Taps of one pixel's three interleaved channels straight from memory: tap t is the three bytes at p + t * step
__device__ __forceinline__ void ore_resize_taps_mem(const uint8_t* p, size_t step, int cnt, const int32_t* k, int32_t& acc0, int32_t& acc1,
                                                    int32_t& acc2) {
    acc0 = acc1 = acc2 = 1 << (ORE_RESIZE_PREC - 1);
    for (int t = 0; t < cnt; ++t) {
        const int32_t kk = k[t];
        const uint8_t* q = p + (size_t)t * step;
        acc0 += (int32_t)q[0] * kk;
        acc1 += (int32_t)q[1] * kk;
        acc2 += (int32_t)q[2] * kk;
    }
}

// four neighbouring bytes of an output row, as one word where the address allows; n = how many of them the row still has
__device__ __forceinline__ void ore_resize_store4(uint8_t* o, int n, uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3) {
    if (n >= 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        *reinterpret_cast<uint32_t*>(o) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
    } else {
        o[0] = (uint8_t)b0;
        if (n > 1) o[1] = (uint8_t)b1;
        if (n > 2) o[2] = (uint8_t)b2;
        if (n > 3) o[3] = (uint8_t)b3;
    }
}

// Workspace form, horizontal pass: output column x of one source row of a rectangle (`row` = its first pixel, sw = its pixels) -> the
// three bytes at o.  A window that leaves the row (tables of another size pair) writes nothing.  It takes a row and the tables as plain
// arguments: a kernel that took a whole descriptor struct as its argument was 0.3 us slower on 1080 rows (profiles/EXPERIMENTS.md).
__device__ __forceinline__ void ore_resize_hpass_mem(const uint8_t* row, int sw, const int32_t* xb, const int32_t* kx, int ksx, int x, uint8_t* o) {
    const int xmin = xb[2 * x], cnt = xb[2 * x + 1];
    if (xmin < 0 || cnt < 0 || cnt > ksx || xmin + cnt > sw) return;
    int32_t acc0, acc1, acc2;
    ore_resize_taps_mem(row + (size_t)xmin * 3, 3, cnt, kx + (size_t)x * ksx, acc0, acc1, acc2);
    o[0] = (uint8_t)ore_resize_clip8(acc0);
    o[1] = (uint8_t)ore_resize_clip8(acc1);
    o[2] = (uint8_t)ore_resize_clip8(acc2);
}
#endif
