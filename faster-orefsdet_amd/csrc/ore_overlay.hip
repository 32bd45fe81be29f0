// Detection overlay ("overlay v1", include/ore_hip.h): boxes, scores and class names drawn onto an interleaved [h][w][3] uint8 frame
// on the device, from the rows where a detection pass left them and with the row count still a device word -- no host wait between
// the pass and the drawn frame.
//   k_overlay_prepare  one block, one thread per row: filter, integer rectangle, label rectangle and text, colours; the rank of every
//                      drawn row by (area descending, row ascending) is counted, and the row goes to that place of the instance table
//   k_overlay_draw     256 threads x 4 pixels over the frame as one flat run of pixels (4 pixels = 3 dwords at any width).  A block
//                      culls the table against its run -- against the outline band and the label, not the rectangle: the inside of a
//                      box is not drawn -- with a wave ballot into a list in draw order kept in LDS; a wave walks the list, fetches
//                      each instance with a wave-uniform address and tests it against each thread's 4-pixel span the same way before
//                      a pixel is touched.  Each pixel is read once and written at most once.  In place, a block that no instance
//                      touches does no pixel traffic.
// All pixel arithmetic is integer; no atomics, no dependence on block order: the picture is bit-exact and the same run to run.
// Compiled with -ffp-contract=off: the area and the percentage are single fp32 operations, each rounded on its own.
// "overlay v1, track colouring" (ore_overlay_draw_ids_fwd, color_by 2): only k_overlay_prepare learns it -- a row with a negative id is
// not drawn, the colour comes from the id and "#<id> " goes in front of the text; k_overlay_draw is the same kernel.
#include "ore_block.h"

namespace {

constexpr int OV_MAX_ROWS = ORE_DET_RECORD_ROWS;   // one prepare thread per row
constexpr int OV_PREP_T = 320;
constexpr int OV_TEXT = 40;                        // characters of one label
constexpr int OV_NAME = 32;                        // bytes of one row of the names table
constexpr int OV_T = 256, OV_PX = 4;               // draw block: 256 threads x 4 pixels
static_assert(OV_MAX_ROWS <= OV_PREP_T && OV_PREP_T % 64 == 0, "one prepare thread per row");

struct Inst {                                      // one drawn row, in draw order
    int32_t X0, Y0, X1, Y1;                        // integer rectangle, inclusive
    int32_t lx, ly, lw, lh;                        // label rectangle (lw = 0: no label)
    uint32_t col, tcol;                            // colour and text colour, channel k in byte k
    int32_t len, pad;                              // characters of the label; 48 bytes in all
};
struct Layout { size_t count, inst, text, total; };
__host__ __device__ inline Layout overlay_layout(int max_rows) {
    const size_t c = max_rows > 0 ? max_rows : 1;
    Layout o{};
    size_t a = 0;
    o.count = a; a += 256;
    o.inst = a; a += (c * sizeof(Inst) + 255) & ~(size_t)255;
    o.text = a; a += (c * OV_TEXT + 255) & ~(size_t)255;
    o.total = a;
    return o;
}

struct PrepArgs {
    const float* boxes; const float* scores; const int64_t* classes; const int64_t* ids; const int32_t* n_dev; int32_t n_host, max_rows;
    int32_t h, w; float score_thresh; int32_t L, S;
    const uint8_t* palette; int32_t n_palette, color_by; const uint8_t* names; int32_t n_names;
    int32_t* count; Inst* inst; uint8_t* text;
};

// (int)v for v clamped to [0, hi] first: the contract's max / min on the integer, without a float -> int conversion out of range
__device__ __forceinline__ int clamp_to_int(float v, int hi) { return (int)fminf(fmaxf(v, 0.0f), (float)hi); }

__global__ __launch_bounds__(OV_PREP_T) void k_overlay_prepare(const PrepArgs a) {
    __shared__ __attribute__((aligned(16))) float s_key[OV_PREP_T];     // the area of a drawn row, NaN of any other (no comparison holds)
    __shared__ int s_m;
    const int i = threadIdx.x;
    int n = a.n_dev ? *a.n_dev : a.n_host;
    n = n < 0 ? 0 : (n > a.max_rows ? a.max_rows : n);
    if (i == 0) s_m = 0;
    f32x4 b = {0.f, 0.f, 0.f, 0.f};
    float sc = 0.f, area = 0.f;
    int X0 = 0, Y0 = 0, X1 = -1, Y1 = -1, ok = 0;
    const bool by_track = a.color_by == 2;
    const long long id = (by_track && i < n) ? (long long)a.ids[i] : 0ll;
    if (i < n && id >= 0) {
        b = *reinterpret_cast<const f32x4*>(a.boxes + (size_t)i * 4);
        sc = a.scores[i];
        if (finite32(b.x) && finite32(b.y) && finite32(b.z) && finite32(b.w) && finite32(sc) && sc >= a.score_thresh) {
            X0 = clamp_to_int(floorf(b.x), a.w);
            Y0 = clamp_to_int(floorf(b.y), a.h);
            X1 = clamp_to_int(ceilf(b.z), a.w) - 1;
            Y1 = clamp_to_int(ceilf(b.w), a.h) - 1;
            ok = (X1 >= X0 && Y1 >= Y0) ? 1 : 0;
            const float dx = b.z - b.x, dy = b.w - b.y;
            area = dx * dy;
            if (area != area) area = 0.0f;                    // inf * 0 sorts as 0
        }
    }
    s_key[i] = ok ? area : __builtin_nanf("");
    __syncthreads();
    if (ok) {
        int rank = 0;
        for (int j = 0; j < n; j += 4) {                          // rows n .. 319 hold NaN
            const f32x4 v = *reinterpret_cast<const f32x4*>(s_key + j);
            rank += (v.x > area || (v.x == area && j < i)) ? 1 : 0;
            rank += (v.y > area || (v.y == area && j + 1 < i)) ? 1 : 0;
            rank += (v.z > area || (v.z == area && j + 2 < i)) ? 1 : 0;
            rank += (v.w > area || (v.w == area && j + 3 < i)) ? 1 : 0;
        }
        const long long cls = a.classes ? (long long)a.classes[i] : 0ll;
        long long ci = (by_track ? id : a.color_by ? cls : (long long)i) % a.n_palette;
        if (ci < 0) ci += a.n_palette;
        const uint8_t* pc = a.palette + ci * 3;
        uint32_t col = 0, tcol = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint32_t c = pc[k];
            col |= c << (8 * k);
            tcol |= (c + ((255u - c) * 7u) / 10u) << (8 * k);
        }
        Inst q{};
        q.X0 = X0; q.Y0 = Y0; q.X1 = X1; q.Y1 = Y1; q.col = col; q.tcol = tcol;
        if (a.S >= 1) {
            uint8_t* t = a.text + (size_t)rank * OV_TEXT;
            int len = 0;
            auto put = [&](uint8_t ch) { if (len < OV_TEXT) t[len++] = ch; };    // the cut at 40 characters: nothing is written past it
            if (by_track) {                                   // "#" + decimal(id) + " ": up to 21 characters
                put('#');
                unsigned long long div = 1ull;
                while ((unsigned long long)id / div >= 10ull) div *= 10ull;
                for (; div > 0ull; div /= 10ull) put((uint8_t)('0' + ((unsigned long long)id / div) % 10ull));
                put(' ');
            }
            const int len0 = len;
            if (a.names && cls >= 0 && cls < a.n_names) {
                const uint8_t* nm = a.names + (size_t)cls * OV_NAME;
                for (int k = 0; k < OV_NAME && nm[k] != 0; ++k) put(nm[k]);
            }
            if (len > len0) put(' ');
            const float p100 = sc * 100.0f;
            const int pct = (int)fminf(fmaxf(rintf(p100), 0.0f), 100.0f);
            if (pct >= 100) put('1');
            if (pct >= 10) put((uint8_t)('0' + (pct / 10) % 10));
            put((uint8_t)('0' + pct % 10));
            put('%');                                         // without an id 32 + 1 + 3 + 1 = 37: never cuts
            q.len = len;
            q.lw = len * 6 * a.S + 2 * a.S;
            q.lh = 13 * a.S;
            q.lx = min(max(X0, 0), max(a.w - q.lw, 0));
            q.ly = min(max(Y0, 0), max(a.h - q.lh, 0));
        }
        a.inst[rank] = q;
        atomicAdd(&s_m, 1);                                   // an integer count in LDS: order-free
    }
    __syncthreads();
    if (i == 0) *a.count = s_m;
}

struct DrawArgs {
    int32_t h, w; int32_t L, S, edge_alpha, label_alpha;
    uint32_t magic_cell, magic_s;                  // ceil(2^20 / 6S), ceil(2^20 / S): g / d == (g * magic) >> 20 for g < 2048, d <= 48
};

__device__ __forceinline__ uint32_t blend24(uint32_t px, uint32_t col, uint32_t al) {
    return blend8(px & 255u, col & 255u, al) | (blend8((px >> 8) & 255u, (col >> 8) & 255u, al) << 8) |
           (blend8((px >> 16) & 255u, (col >> 16) & 255u, al) << 16);
}

// does the instance draw on pixels xa .. xb of row y?  The outline band (not the rectangle's inside) or the label.
__device__ __forceinline__ bool seg_touches(const Inst& q, int L, int xa, int xb, int y) {
    const bool outline = y >= q.Y0 && y <= q.Y1 && xa <= q.X1 && xb >= q.X0 && (y - q.Y0 < L || q.Y1 - y < L || xa - q.X0 < L || q.X1 - xb < L);
    const bool label = q.lw > 0 && y >= q.ly && y < q.ly + q.lh && xa < q.lx + q.lw && xb >= q.lx;
    return outline || label;
}
// on any pixel of the whole rows ra .. rb?  (every row of a rectangle holds outline pixels)
__device__ __forceinline__ bool rows_touch(const Inst& q, int ra, int rb) {
    return (ra <= q.Y1 && rb >= q.Y0) || (q.lw > 0 && ra < q.ly + q.lh && rb >= q.ly);
}
// on the flat run of pixels from (xa, ya) to (xb, yb)?  A run within one row is tested exactly, one over several rows as its first
// row's tail, its last row's head and the whole rows between.
__device__ __forceinline__ bool run_touches(const Inst& q, int L, int w, int xa, int ya, int xb, int yb) {
    if (ya == yb) return seg_touches(q, L, xa, xb, ya);
    return seg_touches(q, L, xa, w - 1, ya) || seg_touches(q, L, 0, xb, yb) || (yb - ya >= 2 && rows_touch(q, ya + 1, yb - 1));
}

// one instance applied to pixel (x, y), value px (channel k in byte k): outline, then label background, then glyph
__device__ __forceinline__ uint32_t draw_pixel(uint32_t px, int x, int y, const Inst& q, int row, const DrawArgs& a,
                                               const uint8_t* __restrict__ text, const uint8_t* __restrict__ atlas) {
    if (x >= q.X0 && x <= q.X1 && y >= q.Y0 && y <= q.Y1 &&
        (x - q.X0 < a.L || q.X1 - x < a.L || y - q.Y0 < a.L || q.Y1 - y < a.L))
        px = blend24(px, q.col, (uint32_t)a.edge_alpha);
    const int ux = x - q.lx, uy = y - q.ly;
    if (q.lw > 0 && ux >= 0 && ux < q.lw && uy >= 0 && uy < q.lh) {
        px = blend24(px, 0u, (uint32_t)a.label_alpha);
        const int gx = ux - a.S, gy = uy - a.S;
        if (gx >= 0 && gx < q.len * 6 * a.S && gy >= 0 && gy < 11 * a.S) {
            const int cell = (int)(((uint32_t)gx * a.magic_cell) >> 20);                 // gx / 6S
            const int u = (int)(((uint32_t)(gx - cell * 6 * a.S) * a.magic_s) >> 20);    // (gx mod 6S) / S
            const int v = (int)(((uint32_t)gy * a.magic_s) >> 20);                       // gy / S
            const int ch = (int)text[(size_t)row * OV_TEXT + cell] - 32;
            if (ch >= 0 && ch < 95 && atlas[(ch * 11 + v) * 6 + u]) px = q.tcol;
        }
    }
    return px;
}

// the block's list applied, in draw order, to the cnt (1 .. 4) pixels px[] that start at (x, y) and run on in row-major order.  The
// list entry is the same for every lane: the instance is fetched with a wave-uniform address.
__device__ __forceinline__ void draw_span(uint32_t* px, int cnt, int x, int y, const int* s_list, int nhit, const DrawArgs& a,
                                          const Inst* __restrict__ inst, const uint8_t* __restrict__ text, const uint8_t* __restrict__ atlas) {
    int xs[OV_PX], ys[OV_PX];
#pragma unroll
    for (int j = 0; j < OV_PX; ++j) {
        xs[j] = x; ys[j] = y;
        if (++x == a.w) { x = 0; ++y; }
    }
    const int xb = xs[cnt - 1], yb = ys[cnt - 1];
    for (int k = 0; k < nhit; ++k) {
        const int row = __builtin_amdgcn_readfirstlane(s_list[k]);
        const Inst q = inst[row];
        if (!run_touches(q, a.L, a.w, xs[0], ys[0], xb, yb)) continue;
#pragma unroll
        for (int j = 0; j < OV_PX; ++j)
            if (j < cnt) px[j] = draw_pixel(px[j], xs[j], ys[j], q, row, a, text, atlas);
    }
}

__global__ __launch_bounds__(OV_T) void k_overlay_draw(const DrawArgs a, const uint8_t* src, uint8_t* dst, const int32_t* __restrict__ count,
                                                       const Inst* __restrict__ inst, const uint8_t* __restrict__ text,
                                                       const uint8_t* __restrict__ atlas) {
    __shared__ int s_list[OV_MAX_ROWS];
    __shared__ int s_wcount[OV_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool inplace = src == dst;
    const unsigned npix = (unsigned)a.h * (unsigned)a.w;          // <= 8192 * 8192 = 2^26
    const unsigned p_blk = blockIdx.x * (unsigned)(OV_T * OV_PX);
    const unsigned p_end = min(p_blk + (unsigned)(OV_T * OV_PX), npix) - 1u;    // the block's run of pixels, inclusive
    const int by0 = (int)(p_blk / (unsigned)a.w), by1 = (int)(p_end / (unsigned)a.w);
    const int bx0 = (int)(p_blk - (unsigned)by0 * a.w), bx1 = (int)(p_end - (unsigned)by1 * a.w);
    int m = *count;
    m = m < 0 ? 0 : (m > OV_MAX_ROWS ? OV_MAX_ROWS : m);
    int base = 0;
    for (int i0 = 0; i0 < m; i0 += OV_T) {                        // cull, list kept in draw order
        const int i = i0 + tid;
        const bool hit = i < m && run_touches(inst[i], a.L, a.w, bx0, by0, bx1, by1);
        const unsigned long long bal = __ballot(hit);
        if (lane == 0) s_wcount[wave] = __popcll(bal);
        __syncthreads();
        int pre = base, tot = 0;
        for (int w2 = 0; w2 < OV_T / 64; ++w2) { const int c = s_wcount[w2]; if (w2 < wave) pre += c; tot += c; }
        if (hit) s_list[pre + __popcll(bal & ((1ull << lane) - 1ull))] = i;
        base += tot;
        __syncthreads();
    }
    const int nhit = base;
    if (nhit == 0 && inplace) return;                             // nothing of this run changes: no pixel traffic

    const unsigned p0 = p_blk + (unsigned)tid * OV_PX;
    if (p0 >= npix) return;
    const size_t off = (size_t)p0 * 3;
    const int y = (int)(p0 / (unsigned)a.w), x = (int)(p0 - (unsigned)y * a.w);
    if (p0 + OV_PX <= npix) {                                     // 4 pixels = 3 whole dwords, aligned at any width
        const uint32_t* s = reinterpret_cast<const uint32_t*>(src + off);
        const uint32_t d0 = s[0], d1 = s[1], d2 = s[2];
        uint32_t px[OV_PX] = {d0 & 0xffffffu, (d0 >> 24) | ((d1 & 0xffffu) << 8), (d1 >> 16) | ((d2 & 0xffu) << 16), d2 >> 8};
        draw_span(px, OV_PX, x, y, s_list, nhit, a, inst, text, atlas);
        const uint32_t e0 = px[0] | (px[1] << 24), e1 = (px[1] >> 8) | (px[2] << 16), e2 = (px[2] >> 16) | (px[3] << 8);
        if (!inplace || e0 != d0 || e1 != d1 || e2 != d2) {
            uint32_t* d = reinterpret_cast<uint32_t*>(dst + off);
            d[0] = e0; d[1] = e1; d[2] = e2;
        }
    } else {                                                      // the last 1 .. 3 pixels of the frame, byte by byte
        const int cnt = (int)(npix - p0);
        uint32_t px[OV_PX] = {0u, 0u, 0u, 0u}, was[OV_PX];
        for (int j = 0; j < cnt; ++j) {
            const size_t o = off + (size_t)j * 3;
            was[j] = px[j] = src[o] | ((uint32_t)src[o + 1] << 8) | ((uint32_t)src[o + 2] << 16);
        }
        draw_span(px, cnt, x, y, s_list, nhit, a, inst, text, atlas);
        for (int j = 0; j < cnt; ++j) {
            const size_t o = off + (size_t)j * 3;
            if (px[j] != was[j] || !inplace) { dst[o] = (uint8_t)px[j]; dst[o + 1] = (uint8_t)(px[j] >> 8); dst[o + 2] = (uint8_t)(px[j] >> 16); }
        }
    }
}

}  // namespace

extern "C" size_t ore_overlay_workspace_bytes(int32_t max_rows) {
    return max_rows >= 0 && max_rows <= OV_MAX_ROWS ? overlay_layout(max_rows).total : 0;
}

// both entries: color_by 0 .. 2 and ids as k_overlay_prepare takes them, checked by the caller; `who` names the entry in messages
static int overlay_draw(const char* who, const uint8_t* src_hwc, uint8_t* dst_hwc, int32_t h, int32_t w, const float* boxes, const float* scores,
                        const int64_t* classes, const int64_t* ids, const int32_t* n_dev, int32_t n_host, int32_t max_rows, float score_thresh,
                        int32_t line_width, int32_t text_scale, int32_t edge_alpha, int32_t label_alpha,
                        const uint8_t* palette_dev, int32_t n_palette, int32_t color_by, const uint8_t* names_dev,
                        int32_t n_names, const uint8_t* atlas_dev, void* workspace, size_t workspace_bytes, void* stream) {
    ORE_CHECK_ARG(src_hwc && dst_hwc && palette_dev && workspace, "%s: null pointer", who);
    ORE_CHECK_ARG(h >= 1 && h <= ORE_OVERLAY_MAX_SIDE && w >= 1 && w <= ORE_OVERLAY_MAX_SIDE, "%s: frame %dx%d, sides 1 .. %d", who, h, w,
                  ORE_OVERLAY_MAX_SIDE);
    ORE_CHECK_ARG(max_rows >= 0 && max_rows <= OV_MAX_ROWS && (n_dev || n_host >= 0), "%s: max_rows %d (0 .. %d), n_host %d", who, max_rows,
                  OV_MAX_ROWS, n_host);
    ORE_CHECK_ARG(max_rows == 0 || (boxes && scores), "%s: null rows", who);
    ORE_CHECK_ARG(line_width >= 1 && line_width <= 16 && text_scale >= 0 && text_scale <= 8, "%s: line_width %d (1 .. 16), text_scale %d (0 .. 8)", who,
                  line_width, text_scale);
    ORE_CHECK_ARG(edge_alpha >= 0 && edge_alpha <= 255 && label_alpha >= 0 && label_alpha <= 255, "%s: edge_alpha %d, label_alpha %d (0 .. 255)", who,
                  edge_alpha, label_alpha);
    ORE_CHECK_ARG(n_palette >= 1 && n_palette <= 256 && n_names >= 0, "%s: n_palette %d (1 .. 256), n_names %d (>= 0)", who, n_palette, n_names);
    ORE_CHECK_ARG(text_scale == 0 || atlas_dev, "%s: labels need the glyph atlas", who);
    ORE_CHECK_ARG(score_thresh == score_thresh, "%s: score_thresh is NaN", who);
    const size_t bytes = (size_t)h * w * 3;
    const uintptr_t ps = (uintptr_t)src_hwc, pd = (uintptr_t)dst_hwc;
    ORE_CHECK_ARG(ps % 4 == 0 && pd % 4 == 0, "%s: the frames must be 4-byte aligned", who);
    ORE_CHECK_ARG(ps == pd || (ps < pd ? pd - ps : ps - pd) >= bytes, "%s: src and dst overlap (equal = in place, else disjoint)", who);
    const Layout lay = overlay_layout(max_rows);
    if (workspace_bytes < lay.total) {
        ore_set_error("%s: workspace %zu < %zu", who, workspace_bytes, lay.total);
        return ORE_ENOMEM;
    }
    char* ws = static_cast<char*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    PrepArgs p{boxes, scores, classes, ids, n_dev, n_host, max_rows, h, w, score_thresh, line_width, text_scale,
               palette_dev, n_palette, color_by, names_dev, names_dev ? n_names : 0,
               (int32_t*)(ws + lay.count), (Inst*)(ws + lay.inst), (uint8_t*)(ws + lay.text)};
    k_overlay_prepare<<<1, OV_PREP_T, 0, st>>>(p);
    int rc;
    if ((rc = ore_launch_status("k_overlay_prepare"))) return rc;
    const uint32_t S1 = text_scale > 0 ? (uint32_t)text_scale : 1u;
    DrawArgs d{h, w, line_width, text_scale, edge_alpha, label_alpha, ((1u << 20) + 6 * S1 - 1) / (6 * S1), ((1u << 20) + S1 - 1) / S1};
    const long long npix = (long long)h * w;
    k_overlay_draw<<<(unsigned)((npix + OV_T * OV_PX - 1) / (OV_T * OV_PX)), OV_T, 0, st>>>(
        d, src_hwc, dst_hwc, (const int32_t*)(ws + lay.count), (const Inst*)(ws + lay.inst), (const uint8_t*)(ws + lay.text), atlas_dev);
    return ore_launch_status("k_overlay_draw");
}

extern "C" int ore_overlay_draw_fwd(const uint8_t* src_hwc, uint8_t* dst_hwc, int32_t h, int32_t w, const float* boxes, const float* scores,
                                    const int64_t* classes, const int32_t* n_dev, int32_t n_host, int32_t max_rows, float score_thresh,
                                    int32_t line_width, int32_t text_scale, int32_t edge_alpha, int32_t label_alpha,
                                    const uint8_t* palette_dev, int32_t n_palette, int32_t color_by, const uint8_t* names_dev,
                                    int32_t n_names, const uint8_t* atlas_dev, void* workspace, size_t workspace_bytes, void* stream) {
    return overlay_draw("ore_overlay_draw_fwd", src_hwc, dst_hwc, h, w, boxes, scores, classes, nullptr, n_dev, n_host, max_rows, score_thresh,
                        line_width, text_scale, edge_alpha, label_alpha, palette_dev, n_palette, color_by ? 1 : 0, names_dev, n_names,
                        atlas_dev, workspace, workspace_bytes, stream);
}

extern "C" int ore_overlay_draw_ids_fwd(const uint8_t* src_hwc, uint8_t* dst_hwc, int32_t h, int32_t w, const float* boxes, const float* scores,
                                        const int64_t* classes, const int64_t* ids, const int32_t* n_dev, int32_t n_host, int32_t max_rows,
                                        float score_thresh, int32_t line_width, int32_t text_scale, int32_t edge_alpha, int32_t label_alpha,
                                        const uint8_t* palette_dev, int32_t n_palette, int32_t color_by, const uint8_t* names_dev,
                                        int32_t n_names, const uint8_t* atlas_dev, void* workspace, size_t workspace_bytes, void* stream) {
    ORE_CHECK_ARG(color_by >= 0 && color_by <= 2, "ore_overlay_draw_ids_fwd: color_by %d (0 instance, 1 class, 2 track)", color_by);
    ORE_CHECK_ARG(color_by != 2 || max_rows == 0 || ids, "ore_overlay_draw_ids_fwd: color_by 2 (track) needs ids");
    return overlay_draw("ore_overlay_draw_ids_fwd", src_hwc, dst_hwc, h, w, boxes, scores, classes, color_by == 2 ? ids : nullptr, n_dev, n_host,
                        max_rows, score_thresh, line_width, text_scale, edge_alpha, label_alpha, palette_dev, n_palette, color_by, names_dev,
                        n_names, atlas_dev, workspace, workspace_bytes, stream);
}
