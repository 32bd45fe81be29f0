// The batch canvases of a training step in ONE launch ("batch canvas v1", include/ore_hip.h): every raw image of the step -- the B query
// images and the B*N support crops, each packed CHW at its own size in one device slab -- normalised into its zero-padded NCHW fp32
// canvas.  What ImageList.from_tensors does per image with .float(), (x - mean) / std, two pads and a cat.
//   k_batch_canvas    grid (chunks of a canvas, jobs): a block reads ITS job's row of the table (uniform loads: the sizes and offsets
//                     live on the device, so a captured launch serves the next step's sizes), each thread writes 4 cells of a canvas
//                     row with one 16-byte store.  Memory-bound streaming: no LDS, no reuse.
// The raw rows of a uint8 image start at any byte (w is rarely a multiple of 4): a thread reads the one or two aligned words that hold
// its 4 bytes and shifts them into place.  Nothing outside the slab is read and nothing outside `out` is written, whatever the table
// holds: a row that does not fit is skipped (destination) or becomes an all-padding canvas (source).
#include "ore_common.h"

namespace {

struct CanvasArgs {
    const uint8_t* slab; size_t slab_bytes;
    const int32_t* table;
    const float* mean; const float* stdv;
    float* out; size_t out_floats;
    int32_t n[2], Hc[2], Wc[2], u8[2];          // per group: jobs, canvas, 1 = raw uint8 (else raw fp32)
};

__device__ __forceinline__ uint64_t word_pair(const int32_t* r) { return (uint64_t)(uint32_t)r[0] | ((uint64_t)(uint32_t)r[1] << 32); }

__global__ __launch_bounds__(256) void k_batch_canvas(const CanvasArgs a) {
    const int job = blockIdx.y;
    const int g = job >= a.n[0] ? 1 : 0;
    const int Hc = a.Hc[g], Wc = a.Wc[g];
    const bool u8 = a.u8[g] != 0;
    const int32_t* r = a.table + (size_t)job * ORE_BATCH_CANVAS_JOB_INTS;
    const uint64_t src_off = word_pair(r + ORE_BCJ_SRC), dst_off = word_pair(r + ORE_BCJ_DST);
    int h = r[ORE_BCJ_H], w = r[ORE_BCJ_W];
    const size_t cells = (size_t)3 * Hc * Wc;
    // the destination: this job's whole canvas inside `out`, 16-byte aligned, of the launch's canvas size
    if (r[ORE_BCJ_HC] != Hc || r[ORE_BCJ_WC] != Wc || (dst_off & 3) || dst_off > a.out_floats || cells > a.out_floats - dst_off) return;
    // the source: 3 planes of h x w inside the slab and inside the canvas; anything else is an empty image
    const size_t esz = u8 ? 1 : 4;
    if (h < 0 || w < 0 || h > Hc || w > Wc || src_off > a.slab_bytes || (size_t)3 * h * w * esz > a.slab_bytes - src_off || (!u8 && (src_off & 3)))
        h = w = 0;
    const int Q = Wc >> 2, total = 3 * Hc * Q;
    float* const dst = a.out + dst_off;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < total; q += gridDim.x * 256) {
        const int row = q / Q, x0 = (q - row * Q) << 2;
        const int c = row / Hc, y = row - c * Hc;
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        const int n = w - x0;                                    // cells of this quad inside the image (> 0: some)
        if (y < h && n > 0) {
            const float m = a.mean[c], s = a.stdv[c];
            const size_t e = ((size_t)c * h + y) * w + x0;       // element index inside the image
            float raw[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (u8) {
                const size_t addr = src_off + e, base = addr & ~(size_t)3;
                const unsigned sh = (unsigned)(addr & 3) * 8;
                const int need = n < 4 ? n : 4;
                const uint32_t lo = *reinterpret_cast<const uint32_t*>(a.slab + base);
                // the second word only where the quad's own bytes reach into it: those bytes are the image's, so the word is the slab's
                // (slab_bytes is a multiple of 4)
                const uint32_t hi = (sh >> 3) + need > 4 ? *reinterpret_cast<const uint32_t*>(a.slab + base + 4) : 0u;
                const uint32_t bytes = (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
#pragma unroll
                for (int j = 0; j < 4; ++j) raw[j] = (float)((bytes >> (8 * j)) & 255u);
            } else {
                const float* p = reinterpret_cast<const float*>(a.slab + src_off) + e;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < n) raw[j] = p[j];
            }
            // (x - mean) / std, each rounded on its own: the subtraction and the correctly rounded division of the torch composition
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = j < n ? __fdiv_rn(__fsub_rn(raw[j], m), s) : 0.0f;
        }
        st4(dst + (size_t)row * Wc + x0, v);
    }
}

}  // namespace

extern "C" int ore_batch_canvas_fwd(const void* slab, size_t slab_bytes, const int32_t* table, int32_t n_query, int32_t Hq, int32_t Wq,
                                    int32_t query_u8, int32_t n_support, int32_t Hs, int32_t Ws, int32_t support_u8,
                                    const float* pixel_mean, const float* pixel_std, float* out, size_t out_floats, void* stream) {
    ORE_CHECK_ARG(slab && table && pixel_mean && pixel_std && out, "ore_batch_canvas_fwd: null pointer");
    ORE_CHECK_ARG(((uintptr_t)slab & 15) == 0 && (slab_bytes & 3) == 0 && ((uintptr_t)out & 15) == 0,
                  "ore_batch_canvas_fwd: the slab and the canvases start at 16-byte boundaries, the slab holds whole words (%zu bytes)", slab_bytes);
    ORE_CHECK_ARG(n_query >= 0 && n_support >= 0 && n_query + n_support >= 1 && n_query + n_support <= 65535,
                  "ore_batch_canvas_fwd: %d + %d jobs (1 .. 65535 in all)", n_query, n_support);
    const int32_t n[2] = {n_query, n_support}, Hc[2] = {Hq, Hs}, Wc[2] = {Wq, Ws};
    size_t need = 0;
    int64_t quads = 0;
    for (int g = 0; g < 2; ++g) {
        if (n[g] == 0) continue;
        ORE_CHECK_ARG(Hc[g] >= 1 && Hc[g] <= 8192 && Wc[g] >= 4 && Wc[g] <= 8192 && Wc[g] % 4 == 0,
                      "ore_batch_canvas_fwd: canvas %d x %d (sides 1 .. 8192, the width a multiple of 4)", Hc[g], Wc[g]);
        need += (size_t)n[g] * 3 * Hc[g] * Wc[g];
        const int64_t q = (int64_t)3 * Hc[g] * (Wc[g] / 4);
        quads = q > quads ? q : quads;
    }
    ORE_CHECK_ARG(need <= out_floats, "ore_batch_canvas_fwd: the canvases take %zu floats, out holds %zu", need, out_floats);
    CanvasArgs a{(const uint8_t*)slab, slab_bytes, table, pixel_mean, pixel_std, out, out_floats,
                 {n[0], n[1]}, {Hc[0], Hc[1]}, {Wc[0], Wc[1]}, {query_u8 ? 1 : 0, support_u8 ? 1 : 0}};
    int64_t gx = (quads + 511) / 512;                            // two quads per thread; the loop takes what a capped grid leaves
    gx = gx < 1 ? 1 : (gx > 2048 ? 2048 : gx);
    k_batch_canvas<<<dim3((unsigned)gx, (unsigned)(n_query + n_support)), 256, 0, (hipStream_t)stream>>>(a);
    return ore_launch_status("k_batch_canvas");
}
