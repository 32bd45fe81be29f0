// Tiled (sliced) inference for frames larger than one detector pass (fewx/modeling/tiled_inference.py TiledInference): what runs in front
// of and behind the engine passes of one frame's tiles, all on the caller's stream, no host synchronisation.
//   k_tile_gather_u8  the interleaved [h][w][3] frame -> every tile of the plan as a planar [3][th][tw] image (the engine's uint8 input),
//                     one launch; the tile origins are computed here, min(i * stride, length - extent), so no table is uploaded
//   k_tile_collect    one source's detection rows (a tile, or the resized full-frame pass) -> seam rule on the source-local coordinates
//                     -> scale and offset into the frame -> appended, in row order, to the merge pool of ore_tta_merge_fwd
// Compiled with -ffp-contract=off: every fp32 operation of the collect is rounded on its own, as numpy rounds them.
#include "ore_common.h"

namespace {

constexpr int TILE_MAX_SIDE = 8192;
constexpr int TILE_MAX_TILES = 128;
constexpr int GP = 1024;                           // pixels of one tile row a block moves at a time
constexpr int GR = 4;                              // tile rows per block
constexpr int GROW = 3 * GP + 16;                  // LDS bytes of one staged row: 3 * GP payload + up to 15 bytes of leading misalignment
static_assert(GROW % 16 == 0, "staged rows start 16-byte aligned");

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct GatherArgs {
    const uint8_t* src; uint8_t* dst;
    int32_t h, w, th, tw, stride_y, stride_x, ny, nx, swap_rb;
};

// grid (ceil(tw / GP), ceil(th / GR), ny * nx).  Stage: the source bytes of GR row segments into LDS by aligned 16-byte loads -- a
// vector that is not wholly inside the frame is read byte by byte, and only its bytes inside the frame.  Emit: every aligned 16-byte
// word of the three planar destination segments of each row is put together from LDS (stride-3 bytes) and stored once; a word that is
// not wholly inside its segment is written byte by byte, and only its bytes inside the segment.
__global__ __launch_bounds__(256) void k_tile_gather_u8(const GatherArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[GR * GROW];
    const int t = blockIdx.z, iy = t / a.nx, ix = t - iy * a.nx;
    const int y0 = min(iy * a.stride_y, a.h - a.th), x0 = min(ix * a.stride_x, a.w - a.tw);
    const int xc = blockIdx.x * GP, np = min(GP, a.tw - xc);                 // this block's columns of the tile
    const int yr = blockIdx.y * GR, nr = min(GR, a.th - yr);                 // and its rows
    const uintptr_t f_lo = (uintptr_t)a.src, f_hi = f_lo + (size_t)a.h * a.w * 3;
    constexpr int VR = GROW / 16;                                            // vectors of one staged row
    for (int i = threadIdx.x; i < nr * VR; i += 256) {
        const int r = i / VR, v = i - r * VR;
        const uintptr_t s = f_lo + ((size_t)(y0 + yr + r) * a.w + (x0 + xc)) * 3, e = s + (size_t)np * 3;
        const uintptr_t lo = (s & ~(uintptr_t)15) + (size_t)v * 16;
        if (lo >= e) continue;
        uint8_t* to = lds + r * GROW + v * 16;
        if (lo >= f_lo && lo + 16 <= f_hi) {
            *reinterpret_cast<u32x4*>(to) = *reinterpret_cast<const u32x4*>(lo);
        } else {
            for (int j = 0; j < 16; ++j)
                if (lo + j >= s && lo + j < e) to[j] = *reinterpret_cast<const uint8_t*>(lo + j);
        }
    }
    __syncthreads();
    constexpr int WR = GP / 16 + 1;                                          // aligned words one destination segment can touch
    for (int i = threadIdx.x; i < nr * 3 * WR; i += 256) {
        const int r = i / (3 * WR), c = (i - r * 3 * WR) / WR, k = i - (r * 3 + c) * WR;
        const uintptr_t d = (uintptr_t)a.dst + (((size_t)t * 3 + c) * a.th + (yr + r)) * a.tw + xc, e = d + np;
        const uintptr_t lo = (d & ~(uintptr_t)15) + (size_t)k * 16;
        if (lo >= e) continue;
        const uintptr_t s = f_lo + ((size_t)(y0 + yr + r) * a.w + (x0 + xc)) * 3;
        // byte (lo + j) of the plane is pixel (lo + j - d) of the segment: channel cs of the staged row, which starts (s & 15) bytes in
        const uint8_t* from = lds + r * GROW + (int)(s & 15) + (a.swap_rb ? 2 - c : c);
        if (lo >= d && lo + 16 <= e) {
            const uint8_t* p = from + 3 * (int)(lo - d);
            u32x4 o;
            o.x = p[0] | (unsigned)p[3] << 8 | (unsigned)p[6] << 16 | (unsigned)p[9] << 24;
            o.y = p[12] | (unsigned)p[15] << 8 | (unsigned)p[18] << 16 | (unsigned)p[21] << 24;
            o.z = p[24] | (unsigned)p[27] << 8 | (unsigned)p[30] << 16 | (unsigned)p[33] << 24;
            o.w = p[36] | (unsigned)p[39] << 8 | (unsigned)p[42] << 16 | (unsigned)p[45] << 24;
            *reinterpret_cast<u32x4*>(lo) = o;
        } else {
            for (int j = 0; j < 16; ++j)
                if (lo + j >= d && lo + j < e) *reinterpret_cast<uint8_t*>(lo + j) = from[3 * (int)(lo + j - d)];
        }
    }
}

struct TileCollectArgs {
    const float* boxes; const float* scores; const int64_t* classes; const int32_t* n_dev; int32_t n_host, max_rows;
    float sx, sy, ox, oy;                         // source-local -> frame: x * sx + ox, y * sy + oy
    int32_t edges; float margin, x_hi, y_hi;      // x_hi = fl(src_w - margin), y_hi = fl(src_h - margin)
    float* pool_boxes; float* pool_scores; int64_t* pool_classes; int32_t* pool_n; int32_t pool_cap;
    int32_t* src_counts; int32_t* src_dropped; int32_t source;
};

// one block: rows in chunks of 256, a ballot per wave and the waves' totals through LDS give every kept row its place behind the
// kept rows before it -- a stable compaction, integer only
__global__ __launch_bounds__(256) void k_tile_collect(const TileCollectArgs a) {
    __shared__ int s_base, s_n, s_wave[4];
    if (threadIdx.x == 0) {
        int n = a.n_dev ? *a.n_dev : a.n_host;
        n = n < 0 ? 0 : (n > a.max_rows ? a.max_rows : n);
        const int base = a.source == 0 ? 0 : *a.pool_n;       // the first source of a frame restarts the pool
        s_base = base < 0 || base > a.pool_cap ? a.pool_cap : base;
        s_n = n;
    }
    __syncthreads();
    const int base = s_base, n = s_n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int kept = 0, dropped = 0;                                // running totals, the same in every thread
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + threadIdx.x;
        bool keep = false, live = i < n;
        f32x4 b = {0.f, 0.f, 0.f, 0.f};
        if (live) {
            b = *reinterpret_cast<const f32x4*>(a.boxes + (size_t)i * 4);
            const bool cut = ((a.edges & 1) && b.x < a.margin) || ((a.edges & 2) && b.y < a.margin) ||
                             ((a.edges & 4) && b.z > a.x_hi) || ((a.edges & 8) && b.w > a.y_hi);
            keep = !cut;
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int before = __popcll(m & ((1ull << lane) - 1)), total = 0;
        for (int v = 0; v < 4; ++v) {
            before += v < wave ? s_wave[v] : 0;
            total += s_wave[v];
        }
        const int at = base + kept + before;
        if (keep && at < a.pool_cap) {                        // never past the pool (the host sizes it so that this does not cut)
            const float x0 = b.x * a.sx, y0 = b.y * a.sy, x1 = b.z * a.sx, y1 = b.w * a.sy;
            *reinterpret_cast<f32x4*>(a.pool_boxes + (size_t)at * 4) = f32x4{x0 + a.ox, y0 + a.oy, x1 + a.ox, y1 + a.oy};
            a.pool_scores[at] = a.scores[i];
            a.pool_classes[at] = a.classes ? a.classes[i] : 0;
        }
        kept += total;
        dropped += min(256, n - i0) - total;
        __syncthreads();                                      // s_wave is written again in the next chunk
    }
    if (threadIdx.x == 0) {
        const int room = a.pool_cap - base;
        const int taken = kept > room ? room : kept;
        *a.pool_n = base + taken;
        a.src_counts[a.source] = taken;
        a.src_dropped[a.source] = dropped;
    }
}

}  // namespace

extern "C" int ore_tile_gather_u8_fwd(const uint8_t* src_hwc, int32_t h, int32_t w, int32_t th, int32_t tw, int32_t stride_y,
                                      int32_t stride_x, int32_t ny, int32_t nx, int32_t swap_rb, uint8_t* dst, void* stream) {
    ORE_CHECK_ARG(src_hwc && dst, "ore_tile_gather_u8_fwd: null pointer");
    ORE_CHECK_ARG(h >= 1 && h <= TILE_MAX_SIDE && w >= 1 && w <= TILE_MAX_SIDE && th >= 1 && tw >= 1 && th <= h && tw <= w,
                  "ore_tile_gather_u8_fwd: frame %dx%d (sides 1 .. %d), tile %dx%d (1 .. the frame's)", h, w, TILE_MAX_SIDE, th, tw);
    ORE_CHECK_ARG(ny >= 1 && nx >= 1 && (int64_t)ny * nx <= TILE_MAX_TILES && stride_y >= 1 && stride_y <= TILE_MAX_SIDE && stride_x >= 1 &&
                      stride_x <= TILE_MAX_SIDE,
                  "ore_tile_gather_u8_fwd: grid %dx%d (1 .. %d tiles), strides %d, %d (1 .. %d)", ny, nx, TILE_MAX_TILES, stride_y, stride_x,
                  TILE_MAX_SIDE);
    ORE_CHECK_ARG((int64_t)(ny - 1) * stride_y >= h - th && (int64_t)(nx - 1) * stride_x >= w - tw,
                  "ore_tile_gather_u8_fwd: %dx%d tiles of %dx%d at strides %d, %d do not reach the far edge of a %dx%d frame", ny, nx, th, tw,
                  stride_y, stride_x, h, w);
    const uintptr_t s0 = (uintptr_t)src_hwc, s1 = s0 + (size_t)h * w * 3, d0 = (uintptr_t)dst, d1 = d0 + (size_t)ny * nx * 3 * th * tw;
    ORE_CHECK_ARG(d1 <= s0 || s1 <= d0, "ore_tile_gather_u8_fwd: dst overlaps src");
    const GatherArgs a{src_hwc, dst, h, w, th, tw, stride_y, stride_x, ny, nx, swap_rb ? 1 : 0};
    k_tile_gather_u8<<<dim3(ceil_div(tw, GP), ceil_div(th, GR), ny * nx), 256, 0, (hipStream_t)stream>>>(a);
    return ore_launch_status("k_tile_gather_u8");
}

extern "C" int ore_tile_collect_fwd(const float* boxes, const float* scores, const int64_t* classes, const int32_t* n_dev, int32_t n_host,
                                    int32_t max_rows, float sx, float sy, float ox, float oy, int32_t src_h, int32_t src_w, int32_t edges,
                                    float margin, float* pool_boxes, float* pool_scores, int64_t* pool_classes, int32_t* pool_n,
                                    int32_t pool_cap, int32_t* src_counts, int32_t* src_dropped, int32_t source, void* stream) {
    ORE_CHECK_ARG(boxes && scores && pool_boxes && pool_scores && pool_classes && pool_n && src_counts && src_dropped,
                  "ore_tile_collect_fwd: null pointer");
    ORE_CHECK_ARG(max_rows >= 0 && pool_cap >= 1 && source >= 0 && (n_dev || n_host >= 0),
                  "ore_tile_collect_fwd: max_rows %d, pool_cap %d, source %d, n_host %d", max_rows, pool_cap, source, n_host);
    ORE_CHECK_ARG(src_h >= 1 && src_h <= TILE_MAX_SIDE && src_w >= 1 && src_w <= TILE_MAX_SIDE && edges >= 0 && edges <= 15 && margin >= 0.0f,
                  "ore_tile_collect_fwd: source %dx%d (sides 1 .. %d), edges %d (0 .. 15), margin %g (>= 0)", src_h, src_w, TILE_MAX_SIDE, edges,
                  (double)margin);
    const TileCollectArgs a{boxes, scores, classes, n_dev, n_host, max_rows, sx, sy, ox, oy, edges, margin, (float)src_w - margin,
                            (float)src_h - margin, pool_boxes, pool_scores, pool_classes, pool_n, pool_cap, src_counts, src_dropped, source};
    k_tile_collect<<<1, 256, 0, (hipStream_t)stream>>>(a);
    return ore_launch_status("k_tile_collect");
}
