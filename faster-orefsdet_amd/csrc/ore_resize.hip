// 8-bit BILINEAR resize, byte for byte Pillow's Image.resize(size, BILINEAR) (ImagingResample: antialiased, separable, 22-bit fixed
// point, uint8 intermediate): interleaved [h][w][3] uint8 in, PLANAR [3][nh][nw] uint8 out -- the image layout of the engine's uint8
// entry (ore_engine_detect_begin, k_stem1<uint8>).  Replaces the CPU resize in front of the detector
// (d2z:data/transforms/augmentation_impl.py ResizeShortestEdge -> d2z:data/transforms/transform.py ResizeTransform.apply_image).
//
// Form 1 (one launch): a block owns a 16 x 64 output tile.  It stages the source rows / columns the tile's windows cover into LDS with
// 16-byte loads, runs the horizontal pass LDS -> LDS (uint8 intermediate, planar), then the vertical pass LDS -> output planes.  The
// intermediate never reaches HBM.  Form 2 (two launches): the intermediate [h][nw][3] lives in a caller workspace; taken when a tile's
// staging exceeds ORE_RESIZE_LDS_BYTES (large reductions: the window grows with the ratio).  Same bytes either way.
// k_support_fused (ore_support.hip) is form 1 inside a rectangle of a canvas; the two are kept as two bodies over the leaves of
// ore_resize_internal.h because every shared form measured was slower here (profiles/EXPERIMENTS.md): a change to the staging, the
// guards or the passes of one is to be made in the other.
//
// Exactness: coefficients are >= 0 and sum to 2^22 + at most ksize / 2 (each is rounded once), so an accumulator stays below
// 2^21 + 255 * (2^22 + 8193) < 2^31: int32 is exact.
#include "ore_common.h"
#include "ore_resize_internal.h"

namespace {

constexpr int TW = ORE_RESIZE_TW, TH = ORE_RESIZE_TH, NT = 256, NTF = ORE_RESIZE_NTF;

__device__ __forceinline__ uint32_t clip8(int32_t acc) { return ore_resize_clip8(acc); }

struct FusedArgs {
    const uint8_t* src; int32_t h, w;
    uint8_t* dst; int32_t nh, nw;
    const int32_t* xb; const int32_t* yb; const int32_t* kx; const int32_t* ky;
    int32_t ksx, ksy;
    int32_t R;            // intermediate / source rows the LDS holds
    int32_t S;            // bytes of one staged source row (multiple of 16)
    int32_t swap_rb;
};

__global__ __launch_bounds__(NTF) void k_resize_fused(const FusedArgs a) {
    extern __shared__ uint4 smem_u4[];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int tw = min(TW, a.nw - x0), th = min(TH, a.nh - y0);
    const int ksx4 = (a.ksx + 3) & ~3;
    int32_t* s_kx = reinterpret_cast<int32_t*>(smem_u4);          // [TW][ksx4], rows zero-padded to whole groups of four taps
    int32_t* s_ky = s_kx + TW * ksx4;                             // [TH][ksy]
    int32_t* s_xb = s_ky + ((TH * a.ksy + 3) & ~3);               // [TW][2]
    int32_t* s_yb = s_xb + TW * 2;                                // [TH][2]
    uint8_t* s_inter = reinterpret_cast<uint8_t*>(s_yb + TH * 2); // [3][R][TW]
    uint8_t* s_src = s_inter + 3 * a.R * TW;                      // [R][S] + 32 bytes a last row's padded taps may read

    // the tile's source extent straight from the tables (block-uniform loads), so that the coefficient rows and the source rows are
    // fetched together and one barrier covers both
    const int cx0 = a.xb[x0 * 2], ncols = a.xb[(x0 + tw - 1) * 2] + a.xb[(x0 + tw - 1) * 2 + 1] - cx0;
    const int r0 = a.yb[y0 * 2], nrows = a.yb[(y0 + th - 1) * 2] + a.yb[(y0 + th - 1) * 2 + 1] - r0;
    for (int i = tid; i < tw * ksx4; i += NTF) {
        const int x = i / ksx4, t = i - x * ksx4;
        s_kx[i] = t < a.ksx ? a.kx[(size_t)(x0 + x) * a.ksx + t] : 0;
    }
    for (int i = tid; i < th * a.ksy; i += NTF) s_ky[i] = a.ky[(size_t)y0 * a.ksy + i];
    for (int i = tid; i < tw * 2; i += NTF) s_xb[i] = a.xb[x0 * 2 + i];
    for (int i = tid; i < th * 2; i += NTF) s_yb[i] = a.yb[y0 * 2 + i];
    if (nrows < 1 || nrows > a.R || ncols < 1 || ncols * 3 + 15 > a.S) return;      // tables of another size pair: touch nothing
    const int64_t total = (int64_t)a.h * a.w * 3;
    const int al = (int)(reinterpret_cast<uintptr_t>(a.src) & 15);                  // where the image starts inside its 16-byte granule

    // ---- stage: row rr of the tile = source bytes [row_lo, row_lo + ncols * 3), copied from the 16-byte-aligned address at or below
    // its start, so that the row's first byte lands (row_lo + al) & 15 bytes into its LDS row
    const int S16 = a.S >> 4;
    for (int i = tid; i < nrows * S16; i += NTF) {
        const int rr = i / S16, v = i - rr * S16;
        const int64_t row_lo = ((int64_t)(r0 + rr) * a.w + cx0) * 3;
        const int64_t p = ore_resize_granule_at(row_lo, al, v);
        if (p >= row_lo + (int64_t)ncols * 3) continue;
        // a granule that straddles an end of the image is read byte by byte, inside only
        *reinterpret_cast<uint4*>(s_src + rr * a.S + v * 16) = ore_resize_granule_load(a.src, p, 0, total);
    }
    __syncthreads();

    // ---- horizontal pass: one (row, column) per thread, three channels.  A window is cnt * 3 contiguous bytes of the staged row: they are
    // read as aligned words, shifted to the window's first byte (v_alignbyte), and consumed four taps = three words at a time against four
    // coefficients.  Taps past cnt meet the zero padding of the coefficient row, whatever bytes lie there.
    const int p0 = a.swap_rb ? 2 : 0, p2 = 2 - p0;               // plane of the intermediate that takes source channel 0 / 2
    for (int i = tid; i < nrows * TW; i += NTF) {
        const int rr = i >> 6, x = i & (TW - 1);
        if (x >= tw) continue;
        const int64_t row_lo = ((int64_t)(r0 + rr) * a.w + cx0) * 3;
        const int at = rr * a.S + (int)((row_lo + al) & 15) + (s_xb[2 * x] - cx0) * 3;
        int32_t acc0, acc1, acc2;
        ore_resize_htaps_lds(s_src, at, (s_xb[2 * x + 1] + 3) >> 2, s_kx + x * ksx4, acc0, acc1, acc2);
        s_inter[(p0 * a.R + rr) * TW + x] = (uint8_t)clip8(acc0);
        s_inter[(1 * a.R + rr) * TW + x] = (uint8_t)clip8(acc1);
        s_inter[(p2 * a.R + rr) * TW + x] = (uint8_t)clip8(acc2);
    }
    __syncthreads();

    // ---- vertical pass: four neighbouring columns of one (plane, row) per thread, stored as one word where the address allows
    for (int i = tid; i < 3 * TH * (TW / 4); i += NTF) {
        const int x4 = (i & (TW / 4 - 1)) * 4, y = (i >> 4) & (TH - 1), c = i >> 8;
        if (y >= th || x4 >= tw) continue;
        const int ymin = s_yb[2 * y] - r0, cnt = s_yb[2 * y + 1];
        const int32_t* k = s_ky + y * a.ksy;
        const uint8_t* col = s_inter + ((size_t)c * a.R + ymin) * TW + x4;
        int32_t a0, a1, a2, a3;
        ore_resize_vtaps_lds(col, TW, cnt, k, a0, a1, a2, a3);
        uint8_t* o = a.dst + ((size_t)c * a.nh + (y0 + y)) * a.nw + x0 + x4;
        ore_resize_store4(o, tw - x4, clip8(a0), clip8(a1), clip8(a2), clip8(a3));
    }
}

// ---- form 2: horizontal pass [h][w][3] -> workspace [h][nw][3], vertical pass workspace -> planes
__global__ __launch_bounds__(NT) void k_resize_h(const uint8_t* __restrict__ src, int32_t h, int32_t w, uint8_t* __restrict__ mid, int32_t nw,
                                                const int32_t* __restrict__ xb, const int32_t* __restrict__ kx, int32_t ksx) {
    const int x = blockIdx.x * NT + threadIdx.x, r = blockIdx.y;
    if (x >= nw || r >= h) return;
    ore_resize_hpass_mem(src + (size_t)r * w * 3, w, xb, kx, ksx, x, mid + ((size_t)r * nw + x) * 3);
}

__global__ __launch_bounds__(NT) void k_resize_v(const uint8_t* __restrict__ mid, int32_t nw, uint8_t* __restrict__ dst, int32_t nh,
                                                const int32_t* __restrict__ yb, const int32_t* __restrict__ ky, int32_t ksy, int32_t swap_rb) {
    const int x = blockIdx.x * NT + threadIdx.x, y = blockIdx.y;
    if (x >= nw || y >= nh) return;
    const int ymin = yb[2 * y], cnt = yb[2 * y + 1];
    const uint8_t* p = mid + ((size_t)ymin * nw + x) * 3;
    const int32_t* k = ky + (size_t)y * ksy;
    int32_t acc0, acc1, acc2;
    ore_resize_taps_mem(p, (size_t)nw * 3, cnt, k, acc0, acc1, acc2);
    const size_t plane = (size_t)nh * nw, at = (size_t)y * nw + x;
    dst[(swap_rb ? 2 : 0) * plane + at] = (uint8_t)clip8(acc0);
    dst[plane + at] = (uint8_t)clip8(acc1);
    dst[(swap_rb ? 0 : 2) * plane + at] = (uint8_t)clip8(acc2);
}

using FusedLds = ore_resize_fused_lds;

FusedLds fused_lds(int32_t h, int32_t w, int32_t nh, int32_t nw) { return ore_resize_fused_lds_of(h, w, nh, nw, TH, TW); }

bool sizes_ok(int32_t h, int32_t w, int32_t nh, int32_t nw) {
    return ore_resize_side_ok(h) && ore_resize_side_ok(w) && ore_resize_side_ok(nh) && ore_resize_side_ok(nw);
}

}  // namespace

extern "C" int32_t ore_resize_form(int32_t h, int32_t w, int32_t nh, int32_t nw) {
    if (!sizes_ok(h, w, nh, nw)) return 0;
    return fused_lds(h, w, nh, nw).bytes <= (size_t)ORE_RESIZE_LDS_BYTES ? ORE_RESIZE_FORM_LDS : ORE_RESIZE_FORM_WORKSPACE;
}

extern "C" size_t ore_resize_workspace_bytes(int32_t h, int32_t w, int32_t nh, int32_t nw) {
    if (!sizes_ok(h, w, nh, nw)) return 0;
    return (size_t)h * nw * 3;
}

extern "C" size_t ore_resize_table_ints(int32_t h, int32_t w, int32_t nh, int32_t nw) {
    if (!sizes_ok(h, w, nh, nw)) return 0;
    return ore_resize_layout_of(h, w, nh, nw).total;
}

extern "C" int ore_resize_tables_host(int32_t h, int32_t w, int32_t nh, int32_t nw, int32_t* tables_host) {
    ORE_CHECK_ARG(sizes_ok(h, w, nh, nw), "ore_resize_tables_host: %dx%d -> %dx%d outside [1, %d]", h, w, nh, nw, ORE_RESIZE_MAX_SIDE);
    ORE_CHECK_ARG(tables_host, "ore_resize_tables_host: null table");
    const ore_resize_layout t = ore_resize_layout_of(h, w, nh, nw);
    int rc = ore_resize_plan(w, nw, tables_host + t.xb, tables_host + t.kx, nullptr);
    if (rc != ORE_OK) return rc;
    return ore_resize_plan(h, nh, tables_host + t.yb, tables_host + t.ky, nullptr);
}

extern "C" int ore_resize_bilinear_u8_fwd(const uint8_t* src_hwc, int32_t h, int32_t w, uint8_t* dst_chw, int32_t nh, int32_t nw,
                                          int32_t swap_rb, const int32_t* tables_dev, int32_t form, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    ORE_CHECK_ARG(sizes_ok(h, w, nh, nw), "ore_resize_bilinear_u8_fwd: %dx%d -> %dx%d outside [1, %d]", h, w, nh, nw, ORE_RESIZE_MAX_SIDE);
    ORE_CHECK_ARG(src_hwc && dst_chw && tables_dev, "ore_resize_bilinear_u8_fwd: null pointer");
    ORE_CHECK_ARG(form == 0 || form == ORE_RESIZE_FORM_LDS || form == ORE_RESIZE_FORM_WORKSPACE, "ore_resize_bilinear_u8_fwd: form %d", form);
    const ore_resize_layout t = ore_resize_layout_of(h, w, nh, nw);
    const int32_t ksx = t.ksx, ksy = t.ksy;
    const int32_t* xb = tables_dev + t.xb;
    const int32_t* yb = tables_dev + t.yb;
    const int32_t* kx = tables_dev + t.kx;
    const int32_t* ky = tables_dev + t.ky;
    hipStream_t s = (hipStream_t)stream;
    const FusedLds l = fused_lds(h, w, nh, nw);
    const bool fits = l.bytes <= (size_t)ORE_RESIZE_LDS_BYTES;
    ORE_CHECK_ARG(form != ORE_RESIZE_FORM_LDS || fits, "ore_resize_bilinear_u8_fwd: the LDS form needs %zu bytes for %dx%d -> %dx%d, limit %d",
                  l.bytes, h, w, nh, nw, ORE_RESIZE_LDS_BYTES);
    if (form == ORE_RESIZE_FORM_LDS || (form == 0 && fits)) {
        FusedArgs a{src_hwc, h, w, dst_chw, nh, nw, xb, yb, kx, ky, ksx, ksy, l.R, l.S, swap_rb ? 1 : 0};
        k_resize_fused<<<dim3(ceil_div(nw, TW), ceil_div(nh, TH)), NTF, l.bytes, s>>>(a);
        return ore_launch_status("k_resize_fused");
    }
    const size_t need = (size_t)h * nw * 3;
    if (!workspace || workspace_bytes < need) {
        ore_set_error("ore_resize_bilinear_u8_fwd: the two-launch form needs a workspace of %zu bytes (got %zu)", need, workspace_bytes);
        return ORE_ENOMEM;
    }
    uint8_t* mid = static_cast<uint8_t*>(workspace);
    k_resize_h<<<dim3(ceil_div(nw, NT), h), NT, 0, s>>>(src_hwc, h, w, mid, nw, xb, kx, ksx);
    int rc = ore_launch_status("k_resize_h");
    if (rc != ORE_OK) return rc;
    k_resize_v<<<dim3(ceil_div(nw, NT), nh), NT, 0, s>>>(mid, nw, dst_chw, nh, yb, ky, ksy, swap_rb ? 1 : 0);
    return ore_launch_status("k_resize_v");
}
