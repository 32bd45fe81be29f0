// Window arithmetic of the 8-bit antialiased BILINEAR resample (Pillow's ImagingResample), shared by the host planner
// (ore_resize_plan.cpp) and the launcher (ore_resize.hip), which sizes a tile's LDS from the first and last window of the tile.
#pragma once
#include <stdint.h>

#define ORE_RESIZE_PREC 22           // fractional bits of the fixed-point coefficients
#define ORE_RESIZE_MAX_SIDE 8192

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
