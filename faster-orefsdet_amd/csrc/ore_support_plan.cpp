// Host planner of the support crops ("support crop v1", include/ore_hip.h): the integer geometry of one (frame size, box, S, context),
// the box inside the crop in fp32 (no contraction: this file is built with -ffp-contract=off), the job's form and LDS sizing, and its
// resample tables -- which are ore_resize_plan's, one call per axis, so that Pillow's coefficient arithmetic exists once, laid out in
// the job buffer as ore_resize_layout_of lays out any size pair's tables.  Host only: callable without a GPU.
#include <math.h>
#include <string.h>
#include "ore_common.h"
#include "ore_resize_internal.h"

namespace {

struct Geom {
    int32_t D, x0, y0, rx0, ry0, rx1, ry1, dx0, dy0, dx1, dy1;
    int32_t sw, sh, nw, nh;       // source and destination rectangle sizes
};

inline int32_t imax(int32_t a, int32_t b) { return a > b ? a : b; }
inline int32_t imin(int32_t a, int32_t b) { return a < b ? a : b; }

// floor / ceil of a finite float as an int32 inside [-2^30, 2^30] (a frame side is at most 8192: the clamp changes no result)
inline int32_t to_i32(float v) {
    const float lim = 1073741824.0f;
    return (int32_t)(v < -lim ? -lim : (v > lim ? lim : v));
}

bool geometry(int32_t h, int32_t w, const float* b, int32_t S, int32_t c, Geom* g) {
    if (!b || !ore_resize_side_ok(h) || !ore_resize_side_ok(w) || c < 0 || !ore_resize_side_ok(S) || S - 2 * c < 1) return false;
    for (int i = 0; i < 4; ++i)
        if (!isfinite(b[i])) return false;
    const int32_t T = S - 2 * c;
    const int32_t bx0 = imax(0, to_i32(floorf(b[0]))), by0 = imax(0, to_i32(floorf(b[1])));
    const int32_t bx1 = imin(w, to_i32(ceilf(b[2]))), by1 = imin(h, to_i32(ceilf(b[3])));
    const int32_t bw = bx1 - bx0, bh = by1 - by0;
    if (bw < 1 || bh < 1) return false;
    const int32_t L = imax(bw, bh), m = (c * L + T - 1) / T;
    g->D = L + 2 * m;
    g->x0 = bx0 - (g->D - bw) / 2;                     // D - bw, D - bh >= 0: C's division is the floor division
    g->y0 = by0 - (g->D - bh) / 2;
    g->rx0 = imax(g->x0, 0), g->rx1 = imin(g->x0 + g->D, w);
    g->ry0 = imax(g->y0, 0), g->ry1 = imin(g->y0 + g->D, h);
    const int64_t D = g->D, half = D / 2;
    g->dx0 = (int32_t)(((int64_t)(g->rx0 - g->x0) * S + half) / D), g->dx1 = (int32_t)(((int64_t)(g->rx1 - g->x0) * S + half) / D);
    g->dy0 = (int32_t)(((int64_t)(g->ry0 - g->y0) * S + half) / D), g->dy1 = (int32_t)(((int64_t)(g->ry1 - g->y0) * S + half) / D);
    g->sw = g->rx1 - g->rx0, g->sh = g->ry1 - g->ry0, g->nw = g->dx1 - g->dx0, g->nh = g->dy1 - g->dy0;
    // the box overlaps the frame, so the source rectangle is not empty; a destination rectangle can round to nothing only for a
    // rectangle thinner than D / 2S of the window, which a window around a box inside the frame does not leave: refused all the same
    return g->sw >= 1 && g->sh >= 1 && g->nw >= 1 && g->nh >= 1 && g->dx0 >= 0 && g->dy0 >= 0 && g->dx1 <= S && g->dy1 <= S;
}

inline size_t table_ints(const Geom& g) { return ore_resize_layout_of(g.sh, g.sw, g.nh, g.nw).total; }

inline ore_resize_fused_lds lds_of(const Geom& g) { return ore_resize_fused_lds_at(g.sh, g.sw, g.nh, g.nw, g.dy0, g.dx0); }

inline int32_t float_bits(float v) {
    int32_t u;
    memcpy(&u, &v, 4);
    return u;
}

inline float map_clip(float v, int32_t r0, int32_t d0, float s, int32_t S) {
    const float t = (v - (float)r0) * s;
    const float o = (float)d0 + t;
    return o < 0.0f ? 0.0f : (o > (float)S ? (float)S : o);
}

}  // namespace

extern "C" size_t ore_support_crop_job_ints(int32_t h, int32_t w, const float* box_xyxy, int32_t S, int32_t context) {
    Geom g;
    return geometry(h, w, box_xyxy, S, context, &g) ? table_ints(g) : 0;
}

extern "C" int32_t ore_support_crop_form(int32_t h, int32_t w, const float* box_xyxy, int32_t S, int32_t context) {
    Geom g;
    if (!geometry(h, w, box_xyxy, S, context, &g)) return 0;
    return lds_of(g).bytes <= (size_t)ORE_RESIZE_LDS_BYTES ? ORE_RESIZE_FORM_LDS : ORE_RESIZE_FORM_WORKSPACE;
}

extern "C" size_t ore_support_crop_workspace_bytes(int32_t h, int32_t w, const float* box_xyxy, int32_t S, int32_t context) {
    Geom g;
    if (!geometry(h, w, box_xyxy, S, context, &g) || lds_of(g).bytes <= (size_t)ORE_RESIZE_LDS_BYTES) return 0;
    return ((size_t)g.sh * g.nw * 3 + 15) & ~(size_t)15;
}

extern "C" int ore_support_crop_plan(int32_t h, int32_t w, const float* box_xyxy, int32_t S, int32_t context, const uint8_t* frame_dev,
                                     int64_t table_off, int64_t workspace_off, int32_t* record_host, int32_t* buffer_host) {
    Geom g;
    ORE_CHECK_ARG(geometry(h, w, box_xyxy, S, context, &g),
                  "ore_support_crop_plan: frame %dx%d, size %d, context %d: the box lies outside the frame or a size is out of range", h, w, S, context);
    ORE_CHECK_ARG(record_host && buffer_host, "ore_support_crop_plan: null buffer");
    const ore_resize_layout t = ore_resize_layout_of(g.sh, g.sw, g.nh, g.nw);
    ORE_CHECK_ARG(table_off >= 0 && workspace_off >= 0 && (uint64_t)table_off + t.total <= (uint64_t)INT32_MAX,
                  "ore_support_crop_plan: table offset %lld outside an int32 word index", (long long)table_off);
    const int32_t xb = (int32_t)(table_off + t.xb), yb = (int32_t)(table_off + t.yb), kx = (int32_t)(table_off + t.kx), ky = (int32_t)(table_off + t.ky);
    int rc = ore_resize_plan(g.sw, g.nw, buffer_host + xb, buffer_host + kx, nullptr);
    if (rc != ORE_OK) return rc;
    rc = ore_resize_plan(g.sh, g.nh, buffer_host + yb, buffer_host + ky, nullptr);
    if (rc != ORE_OK) return rc;
    const ore_resize_fused_lds l = lds_of(g);
    const uint64_t fp = (uint64_t)(uintptr_t)frame_dev, wo = (uint64_t)workspace_off;
    int32_t* r = record_host;
    memset(r, 0, sizeof(int32_t) * ORE_SUPPORT_JOB_INTS);
    r[ORE_SJ_FRAME_LO] = (int32_t)(uint32_t)fp, r[ORE_SJ_FRAME_HI] = (int32_t)(uint32_t)(fp >> 32);
    r[ORE_SJ_H] = h, r[ORE_SJ_W] = w;
    r[ORE_SJ_RX0] = g.rx0, r[ORE_SJ_RX0 + 1] = g.ry0, r[ORE_SJ_RX0 + 2] = g.rx1, r[ORE_SJ_RX0 + 3] = g.ry1;
    r[ORE_SJ_DX0] = g.dx0, r[ORE_SJ_DX0 + 1] = g.dy0, r[ORE_SJ_DX0 + 2] = g.dx1, r[ORE_SJ_DX0 + 3] = g.dy1;
    r[ORE_SJ_XB] = xb, r[ORE_SJ_YB] = yb, r[ORE_SJ_KX] = kx, r[ORE_SJ_KY] = ky;
    r[ORE_SJ_KSX] = t.ksx, r[ORE_SJ_KSY] = t.ksy;
    r[ORE_SJ_FORM] = l.bytes <= (size_t)ORE_RESIZE_LDS_BYTES ? ORE_RESIZE_FORM_LDS : ORE_RESIZE_FORM_WORKSPACE;
    r[ORE_SJ_LDS_R] = l.R, r[ORE_SJ_LDS_S] = l.S;
    r[ORE_SJ_WS_LO] = (int32_t)(uint32_t)wo, r[ORE_SJ_WS_HI] = (int32_t)(uint32_t)(wo >> 32);
    r[ORE_SJ_D] = g.D, r[ORE_SJ_X0] = g.x0, r[ORE_SJ_X0 + 1] = g.y0;
    const float sx = (float)g.nw / (float)g.sw, sy = (float)g.nh / (float)g.sh;
    r[ORE_SJ_BOX] = float_bits(map_clip(box_xyxy[0], g.rx0, g.dx0, sx, S));
    r[ORE_SJ_BOX + 1] = float_bits(map_clip(box_xyxy[1], g.ry0, g.dy0, sy, S));
    r[ORE_SJ_BOX + 2] = float_bits(map_clip(box_xyxy[2], g.rx0, g.dx0, sx, S));
    r[ORE_SJ_BOX + 3] = float_bits(map_clip(box_xyxy[3], g.ry0, g.dy0, sy, S));
    return ORE_OK;
}
