// Support crops on the device ("support crop v1", include/ore_hip.h): K jobs, each one box of one frame, each an S x S planar uint8
// crop = Pillow's BILINEAR resample of the job's source rectangle placed at its destination rectangle, `fill` everywhere else.  The
// resample is ore_resize.hip's (the taps, the staging address and the LDS sizing come from ore_resize_internal.h); what differs is that
// one launch serves many small resamples of different frames, and that the canvas around the destination rectangle is written too.
//
// LDS form (k_support_fused, one launch for every such job): a block owns one 16 x 64 tile of one job's CANVAS.  The part of the
// tile inside the destination rectangle is resampled as in k_resize_fused -- source rows staged with 16-byte loads, horizontal pass
// LDS -> LDS, vertical pass LDS -> output -- with the staging clipped to the job's source rectangle instead of the whole image: a
// granule that straddles an end of the rectangle's row is read byte by byte, inside only.  The intermediate is indexed by the tile's
// canvas column, so the vertical pass reads it as aligned words wherever the rectangle starts, and the same pass stores the fill
// bytes of the tile: every canvas byte is written exactly once, by word stores where the address allows.
// Workspace form (jobs whose tile staging exceeds the LDS budget: source / destination ratios from roughly 4 - 5): k_support_h writes
// the intermediate [source rows][nw][3] of every such job into its workspace slice, k_support_v reads it and writes the whole canvas.
// At most three launches per call, whatever K.
#include "ore_common.h"
#include "ore_resize_internal.h"

namespace {

constexpr int TW = ORE_RESIZE_TW, TH = ORE_RESIZE_TH, NT = 256, NTF = ORE_RESIZE_NTF;

struct Job {
    const uint8_t* src; int32_t h, w;
    int32_t rx0, ry0, rx1, ry1, dx0, dy0, dx1, dy1;
    const int32_t* xb; const int32_t* yb; const int32_t* kx; const int32_t* ky;
    int32_t ksx, ksy, form, R, S;
    int64_t ws_off;
};

// one record (block-uniform: the loads are scalar)
__device__ __forceinline__ Job load_job(const int32_t* jobs, int k) {
    const int32_t* r = jobs + (size_t)k * ORE_SUPPORT_JOB_INTS;
    Job j;
    j.src = reinterpret_cast<const uint8_t*>((uintptr_t)(((uint64_t)(uint32_t)r[ORE_SJ_FRAME_HI] << 32) | (uint32_t)r[ORE_SJ_FRAME_LO]));
    j.h = r[ORE_SJ_H], j.w = r[ORE_SJ_W];
    j.rx0 = r[ORE_SJ_RX0], j.ry0 = r[ORE_SJ_RX0 + 1], j.rx1 = r[ORE_SJ_RX0 + 2], j.ry1 = r[ORE_SJ_RX0 + 3];
    j.dx0 = r[ORE_SJ_DX0], j.dy0 = r[ORE_SJ_DX0 + 1], j.dx1 = r[ORE_SJ_DX0 + 2], j.dy1 = r[ORE_SJ_DX0 + 3];
    j.xb = jobs + r[ORE_SJ_XB], j.yb = jobs + r[ORE_SJ_YB], j.kx = jobs + r[ORE_SJ_KX], j.ky = jobs + r[ORE_SJ_KY];
    j.ksx = r[ORE_SJ_KSX], j.ksy = r[ORE_SJ_KSY], j.form = r[ORE_SJ_FORM], j.R = r[ORE_SJ_LDS_R], j.S = r[ORE_SJ_LDS_S];
    j.ws_off = (int64_t)(((uint64_t)(uint32_t)r[ORE_SJ_WS_HI] << 32) | (uint32_t)r[ORE_SJ_WS_LO]);
    return j;
}

__device__ __forceinline__ uint32_t fill_of(int32_t fill_rgb, int c) { return ((uint32_t)fill_rgb >> (8 * c)) & 255u; }

__global__ __launch_bounds__(NTF) void k_support_fused(const int32_t* __restrict__ jobs, uint8_t* __restrict__ dst, int32_t S, int32_t fill_rgb) {
    extern __shared__ uint4 smem_u4[];
    const Job a = load_job(jobs, blockIdx.z);
    if (a.form != ORE_RESIZE_FORM_LDS) return;                   // the two-pass launches write this job's canvas
    const int tid = threadIdx.x;
    const int X0 = blockIdx.x * TW, Y0 = blockIdx.y * TH;
    const int tw = min(TW, S - X0), th = min(TH, S - Y0);
    // the tile's columns [xa, xe) / rows [ya, ye) that lie inside the destination rectangle, tile-local
    const int xa = max(a.dx0 - X0, 0), xe = min(a.dx1 - X0, tw), ya = max(a.dy0 - Y0, 0), ye = min(a.dy1 - Y0, th);
    const bool any = xe > xa && ye > ya;
    const int ksx4 = (a.ksx + 3) & ~3;
    int32_t* s_kx = reinterpret_cast<int32_t*>(smem_u4);          // [TW][ksx4] by tile column, rows zero-padded to whole groups of four taps
    int32_t* s_ky = s_kx + TW * ksx4;                             // [TH][ksy] by tile row
    int32_t* s_xb = s_ky + ((TH * a.ksy + 3) & ~3);               // [TW][2]
    int32_t* s_yb = s_xb + TW * 2;                                // [TH][2]
    uint8_t* s_inter = reinterpret_cast<uint8_t*>(s_yb + TH * 2); // [3][R][TW] by tile column
    uint8_t* s_src = s_inter + 3 * a.R * TW;                      // [R][S] + 32 bytes a last row's padded taps may read
    int r0 = 0;
    if (any) {                                                    // block-uniform
        // rectangle-relative output indices of the tile's first / last column and row inside the rectangle
        const int ox = X0 - a.dx0, oy = Y0 - a.dy0;
        const int cx0 = a.xb[(ox + xa) * 2], ncols = a.xb[(ox + xe - 1) * 2] + a.xb[(ox + xe - 1) * 2 + 1] - cx0;
        r0 = a.yb[(oy + ya) * 2];
        const int nrows = a.yb[(oy + ye - 1) * 2] + a.yb[(oy + ye - 1) * 2 + 1] - r0;
        for (int i = tid; i < (xe - xa) * ksx4; i += NTF) {
            const int x = xa + i / ksx4, t = i % ksx4;
            s_kx[x * ksx4 + t] = t < a.ksx ? a.kx[(size_t)(ox + x) * a.ksx + t] : 0;
        }
        for (int i = tid; i < (ye - ya) * a.ksy; i += NTF) s_ky[ya * a.ksy + i] = a.ky[(size_t)(oy + ya) * a.ksy + i];
        for (int i = tid; i < (xe - xa) * 2; i += NTF) s_xb[xa * 2 + i] = a.xb[(ox + xa) * 2 + i];
        for (int i = tid; i < (ye - ya) * 2; i += NTF) s_yb[ya * 2 + i] = a.yb[(oy + ya) * 2 + i];
        // tables that do not belong to this rectangle pair would overrun the carve: touch nothing (the launcher checks the sizing)
        if (nrows < 1 || nrows > a.R || ncols < 1 || ncols * 3 + 15 > a.S || r0 < 0 || r0 + nrows > a.ry1 - a.ry0 || cx0 < 0 ||
            cx0 + ncols > a.rx1 - a.rx0)
            return;
        const int al = (int)(reinterpret_cast<uintptr_t>(a.src) & 15);

        // ---- stage: row rr of the tile = the bytes of source row ry0 + r0 + rr, columns [rx0 + cx0, + ncols), copied in 16-byte granules;
        // only bytes of the source rectangle's own row segment are read
        const int S16 = a.S >> 4;
        for (int i = tid; i < nrows * S16; i += NTF) {
            const int rr = i / S16, v = i - rr * S16;
            const int64_t line = (int64_t)(a.ry0 + r0 + rr) * a.w;
            const int64_t row_lo = (line + a.rx0 + cx0) * 3;
            const int64_t p = ore_resize_granule_at(row_lo, al, v);
            if (p >= row_lo + (int64_t)ncols * 3) continue;
            *reinterpret_cast<uint4*>(s_src + rr * a.S + v * 16) = ore_resize_granule_load(a.src, p, (line + a.rx0) * 3, (line + a.rx1) * 3);
        }
        __syncthreads();

        // ---- horizontal pass: one (row, tile column) per thread, three channels
        for (int i = tid; i < nrows * TW; i += NTF) {
            const int rr = i >> 6, x = i & (TW - 1);
            if (x < xa || x >= xe) continue;
            const int64_t row_lo = ((int64_t)(a.ry0 + r0 + rr) * a.w + a.rx0 + cx0) * 3;
            const int at = rr * a.S + (int)((row_lo + al) & 15) + (s_xb[2 * x] - cx0) * 3;
            int32_t acc0, acc1, acc2;
            ore_resize_htaps_lds(s_src, at, (s_xb[2 * x + 1] + 3) >> 2, s_kx + x * ksx4, acc0, acc1, acc2);
            s_inter[(0 * a.R + rr) * TW + x] = (uint8_t)ore_resize_clip8(acc0);
            s_inter[(1 * a.R + rr) * TW + x] = (uint8_t)ore_resize_clip8(acc1);
            s_inter[(2 * a.R + rr) * TW + x] = (uint8_t)ore_resize_clip8(acc2);
        }
        __syncthreads();
    }

    // ---- vertical pass and fill: four neighbouring canvas columns of one (plane, row) per thread
    for (int i = tid; i < 3 * TH * (TW / 4); i += NTF) {
        const int x4 = (i & (TW / 4 - 1)) * 4, y = (i >> 4) & (TH - 1), c = i >> 8;
        if (y >= th || x4 >= tw) continue;
        const uint32_t f = fill_of(fill_rgb, c);
        uint32_t b0 = f, b1 = f, b2 = f, b3 = f;
        if (any && y >= ya && y < ye && x4 + 3 >= xa && x4 < xe) {
            int32_t a0, a1, a2, a3;
            ore_resize_vtaps_lds(s_inter + ((size_t)c * a.R + (s_yb[2 * y] - r0)) * TW + x4, TW, s_yb[2 * y + 1], s_ky + y * a.ksy, a0, a1, a2, a3);
            if (x4 >= xa && x4 < xe) b0 = ore_resize_clip8(a0);
            if (x4 + 1 >= xa && x4 + 1 < xe) b1 = ore_resize_clip8(a1);
            if (x4 + 2 >= xa && x4 + 2 < xe) b2 = ore_resize_clip8(a2);
            if (x4 + 3 >= xa && x4 + 3 < xe) b3 = ore_resize_clip8(a3);
        }
        uint8_t* o = dst + (((size_t)blockIdx.z * 3 + c) * S + (Y0 + y)) * S + X0 + x4;
        ore_resize_store4(o, tw - x4, b0, b1, b2, b3);
    }
}

// ---- workspace form, horizontal: source rectangle [sh][sw][3] (inside the frame) -> the job's slice [sh][nw][3]
__global__ __launch_bounds__(NT) void k_support_h(const int32_t* __restrict__ jobs, uint8_t* __restrict__ ws) {
    const Job a = load_job(jobs, blockIdx.z);
    const int nw = a.dx1 - a.dx0, sh = a.ry1 - a.ry0;
    const int x = blockIdx.x * NT + threadIdx.x, r = blockIdx.y;
    if (a.form != ORE_RESIZE_FORM_WORKSPACE || x >= nw || r >= sh) return;
    ore_resize_hpass_mem(a.src + ((size_t)(a.ry0 + r) * a.w + a.rx0) * 3, a.rx1 - a.rx0, a.xb, a.kx, a.ksx, x, ws + a.ws_off + ((size_t)r * nw + x) * 3);
}

// ---- workspace form, vertical and fill: one canvas row per block, four neighbouring columns of one plane per thread.
// Not merged with k_resize_v on purpose: that one takes one pixel (three planes) per thread across a wide image and has no fill to
// write; this one covers a narrow canvas with word stores, fill included.  One mapping for both would change the speed of one of them.
__global__ __launch_bounds__(NT) void k_support_v(const int32_t* __restrict__ jobs, const uint8_t* __restrict__ ws, uint8_t* __restrict__ dst,
                                                  int32_t S, int32_t fill_rgb) {
    const Job a = load_job(jobs, blockIdx.z);
    if (a.form != ORE_RESIZE_FORM_WORKSPACE) return;
    const int nw = a.dx1 - a.dx0, sh = a.ry1 - a.ry0, Y = blockIdx.y, S4 = (S + 3) >> 2;
    const bool rowin = Y >= a.dy0 && Y < a.dy1;
    int ymin = 0, cnt = 0;
    if (rowin) {
        ymin = a.yb[2 * (Y - a.dy0)], cnt = a.yb[2 * (Y - a.dy0) + 1];
        if (ymin < 0 || cnt < 0 || cnt > a.ksy || ymin + cnt > sh) return;
    }
    const int32_t* k = a.ky + (size_t)(rowin ? Y - a.dy0 : 0) * a.ksy;
    const uint8_t* mid = ws + a.ws_off;
    for (int i = threadIdx.x; i < 3 * S4; i += NT) {
        const int c = i / S4, X = (i - c * S4) * 4;
        const uint32_t f = fill_of(fill_rgb, c);
        uint32_t b[4] = {f, f, f, f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int xr = X + j - a.dx0;
            if (!rowin || xr < 0 || xr >= nw) continue;
            int32_t acc = 1 << (ORE_RESIZE_PREC - 1);
            const uint8_t* q = mid + ((size_t)ymin * nw + xr) * 3 + c;
            for (int t = 0; t < cnt; ++t) acc += (int32_t)q[(size_t)t * nw * 3] * k[t];
            b[j] = ore_resize_clip8(acc);
        }
        ore_resize_store4(dst + (((size_t)blockIdx.z * 3 + c) * S + Y) * S + X, S - X, b[0], b[1], b[2], b[3]);
    }
}

inline int64_t word64(const int32_t* r, int lo, int hi) { return (int64_t)(((uint64_t)(uint32_t)r[hi] << 32) | (uint32_t)r[lo]); }

}  // namespace

extern "C" int ore_support_crop_u8_fwd(const int32_t* jobs_dev, const int32_t* jobs_host, size_t buffer_ints, int32_t K, int32_t S,
                                       int32_t fill_rgb, uint8_t* dst, void* workspace, size_t workspace_bytes, void* stream) {
    ORE_CHECK_ARG(jobs_dev && jobs_host && dst, "ore_support_crop_u8_fwd: null pointer");
    ORE_CHECK_ARG(K >= 1 && K <= 65535 && ore_resize_side_ok(S), "ore_support_crop_u8_fwd: K %d (1 .. 65535), size %d", K, S);
    ORE_CHECK_ARG(buffer_ints >= (size_t)K * ORE_SUPPORT_JOB_INTS && buffer_ints <= (size_t)INT32_MAX, "ore_support_crop_u8_fwd: a buffer of %zu words for %d jobs", buffer_ints, K);
    // every record against the frame, the canvas, the buffer and the workspace, and its LDS sizing against the sizing the kernel's
    // carve assumes: nothing is launched on a record that could send a kernel outside them
    size_t lds = 0;
    int32_t n_lds = 0, n_ws = 0, max_sh = 0;
    for (int32_t k = 0; k < K; ++k) {
        const int32_t* r = jobs_host + (size_t)k * ORE_SUPPORT_JOB_INTS;
        const int32_t h = r[ORE_SJ_H], w = r[ORE_SJ_W], rx0 = r[ORE_SJ_RX0], ry0 = r[ORE_SJ_RX0 + 1], rx1 = r[ORE_SJ_RX0 + 2], ry1 = r[ORE_SJ_RX0 + 3];
        const int32_t dx0 = r[ORE_SJ_DX0], dy0 = r[ORE_SJ_DX0 + 1], dx1 = r[ORE_SJ_DX0 + 2], dy1 = r[ORE_SJ_DX0 + 3];
        ORE_CHECK_ARG(word64(r, ORE_SJ_FRAME_LO, ORE_SJ_FRAME_HI) != 0 && ore_resize_side_ok(h) && ore_resize_side_ok(w),
                      "ore_support_crop_u8_fwd: job %d: frame %dx%d", k, h, w);
        ORE_CHECK_ARG(0 <= rx0 && rx0 < rx1 && rx1 <= w && 0 <= ry0 && ry0 < ry1 && ry1 <= h, "ore_support_crop_u8_fwd: job %d: source rectangle (%d, %d, %d, %d) outside the %dx%d frame",
                      k, rx0, ry0, rx1, ry1, h, w);
        ORE_CHECK_ARG(0 <= dx0 && dx0 < dx1 && dx1 <= S && 0 <= dy0 && dy0 < dy1 && dy1 <= S, "ore_support_crop_u8_fwd: job %d: destination rectangle (%d, %d, %d, %d) outside the %d canvas",
                      k, dx0, dy0, dx1, dy1, S);
        const int32_t sw = rx1 - rx0, sh = ry1 - ry0, nw = dx1 - dx0, nh = dy1 - dy0;
        const ore_resize_layout t = ore_resize_layout_of(sh, sw, nh, nw);
        ORE_CHECK_ARG(r[ORE_SJ_KSX] == t.ksx && r[ORE_SJ_KSY] == t.ksy, "ore_support_crop_u8_fwd: job %d: tap counts (%d, %d), planned (%d, %d)", k, r[ORE_SJ_KSX], r[ORE_SJ_KSY], t.ksx, t.ksy);
        // each table where its own record word puts it, with the layout's length, behind the records and inside the buffer
        const int64_t lo = (int64_t)K * ORE_SUPPORT_JOB_INTS, hi = (int64_t)buffer_ints;
        auto inside = [&](int32_t at, size_t n) { return at >= lo && (int64_t)at + (int64_t)n <= hi; };
        ORE_CHECK_ARG(inside(r[ORE_SJ_XB], t.yb - t.xb) && inside(r[ORE_SJ_YB], t.kx - t.yb) && inside(r[ORE_SJ_KX], t.ky - t.kx) &&
                      inside(r[ORE_SJ_KY], t.total - t.ky), "ore_support_crop_u8_fwd: job %d: tables outside the buffer", k);
        const ore_resize_fused_lds l = ore_resize_fused_lds_at(sh, sw, nh, nw, dy0, dx0);
        if (r[ORE_SJ_FORM] == ORE_RESIZE_FORM_LDS) {
            ORE_CHECK_ARG(l.bytes <= (size_t)ORE_RESIZE_LDS_BYTES && r[ORE_SJ_LDS_R] == l.R && r[ORE_SJ_LDS_S] == l.S,
                          "ore_support_crop_u8_fwd: job %d: the LDS form needs %zu bytes (limit %d), rows %d / %d, row bytes %d / %d", k, l.bytes,
                          ORE_RESIZE_LDS_BYTES, r[ORE_SJ_LDS_R], l.R, r[ORE_SJ_LDS_S], l.S);
            if (l.bytes > lds) lds = l.bytes;
            ++n_lds;
        } else {
            ORE_CHECK_ARG(r[ORE_SJ_FORM] == ORE_RESIZE_FORM_WORKSPACE, "ore_support_crop_u8_fwd: job %d: form %d", k, r[ORE_SJ_FORM]);
            const int64_t off = word64(r, ORE_SJ_WS_LO, ORE_SJ_WS_HI), need = (int64_t)sh * nw * 3;
            if (!workspace || off < 0 || (uint64_t)off + (uint64_t)need > (uint64_t)workspace_bytes) {
                ore_set_error("ore_support_crop_u8_fwd: job %d: the two-pass form needs %lld bytes at offset %lld of the workspace (%zu bytes)", k,
                              (long long)need, (long long)off, workspace_bytes);
                return ORE_ENOMEM;
            }
            if (sh > max_sh) max_sh = sh;
            ++n_ws;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    if (n_lds) {
        k_support_fused<<<dim3(ceil_div(S, TW), ceil_div(S, TH), K), NTF, lds, s>>>(jobs_dev, dst, S, fill_rgb);
        int rc = ore_launch_status("k_support_fused");
        if (rc != ORE_OK) return rc;
    }
    if (n_ws) {
        uint8_t* ws = static_cast<uint8_t*>(workspace);
        k_support_h<<<dim3(ceil_div(S, NT), max_sh, K), NT, 0, s>>>(jobs_dev, ws);
        int rc = ore_launch_status("k_support_h");
        if (rc != ORE_OK) return rc;
        k_support_v<<<dim3(1, S, K), NT, 0, s>>>(jobs_dev, ws, dst, S, fill_rgb);
        return ore_launch_status("k_support_v");
    }
    return ORE_OK;
}
