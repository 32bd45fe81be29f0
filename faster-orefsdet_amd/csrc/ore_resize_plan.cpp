// Host planner of the 8-bit BILINEAR resample: per output index the source window and its 22-bit fixed-point weights, computed in
// double precision in the operation order of Pillow's precompute_coeffs / normalize_coeffs_8bpc so that the integers are Pillow's.
// Host only: callable without a GPU.
#include <vector>
#include "ore_common.h"
#include "ore_resize_internal.h"

extern "C" int32_t ore_resize_ksize(int32_t in, int32_t out) {
    if (!ore_resize_side_ok(in) || !ore_resize_side_ok(out)) return 0;
    return ore_resize_axis_of(in, out).ksize;
}

extern "C" int ore_resize_plan(int32_t in, int32_t out, int32_t* bounds_host, int32_t* coeffs_host, int32_t* ksize_out) {
    ORE_CHECK_ARG(ore_resize_side_ok(in) && ore_resize_side_ok(out), "ore_resize_plan: sizes %d -> %d outside [1, %d]", in, out, ORE_RESIZE_MAX_SIDE);
    ORE_CHECK_ARG(bounds_host && coeffs_host, "ore_resize_plan: null table");
    const ore_resize_axis a = ore_resize_axis_of(in, out);
    const double ss = 1.0 / a.filterscale;
    std::vector<double> k((size_t)a.ksize);
    for (int32_t xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * a.scale;
        int32_t xmin, xmax;
        ore_resize_window(a, in, xx, &xmin, &xmax);
        double ww = 0.0;
        for (int32_t x = 0; x < xmax; ++x) {
            double t = (x + xmin - center + 0.5) * ss;
            if (t < 0.0) t = -t;
            const double w = t < 1.0 ? 1.0 - t : 0.0;
            k[x] = w;
            ww += w;
        }
        for (int32_t x = 0; x < xmax; ++x)
            if (ww != 0.0) k[x] /= ww;
        int32_t* kk = coeffs_host + (size_t)xx * a.ksize;
        for (int32_t x = 0; x < a.ksize; ++x) {
            const double v = x < xmax ? k[x] : 0.0;
            kk[x] = v < 0.0 ? (int32_t)(-0.5 + v * (double)(1 << ORE_RESIZE_PREC)) : (int32_t)(0.5 + v * (double)(1 << ORE_RESIZE_PREC));
        }
        bounds_host[2 * xx] = xmin;
        bounds_host[2 * xx + 1] = xmax;
    }
    if (ksize_out) *ksize_out = a.ksize;
    return ORE_OK;
}
