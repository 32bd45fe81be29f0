// Test-time augmentation tail (d2z:modeling/test_time_augmentation.py GeneralizedRCNNWithTTA): what runs between and behind the engine
// passes of one image's variants, all on the caller's stream, no host synchronisation.
//   k_tta_hflip_u8    the flipped variant = the resized variant with its columns reversed (HFlipTransform.apply_image after
//                     ResizeTransform.apply_image): a copy of the sibling the resize kernel has already written, not a second resample
//   k_tta_collect     one variant's detection rows (count on the device or from the host) -> inverse transform (tfm.inverse().apply_box)
//                     -> appended to the pool at a device-side running offset
//   k_tta_prepare / k_tta_rank / k_tta_mask / k_tta_scan
//                     fast_rcnn_inference_single_image over the pool: finite filter, clip, score filter, stable sort by score, per-class
//                     greedy NMS (the IoU arithmetic of ore_nms_fwd, csrc/ore_detect.hip nms_mask_body), first topk survivors
// Latency-bound work on <= 8192 rows: few, plain kernels.  Compiled with -ffp-contract=off: every fp32 operation below is rounded on
// its own, as numpy rounds them.
#include "ore_block.h"

namespace {

constexpr int TTA_MAX_CAND = 8192;                 // candidates one merge takes: 128 mask words, one per thread of the scan block
constexpr int SCAN_T = 128;

__global__ __launch_bounds__(256) void k_tta_hflip_u8(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int32_t rows, int32_t nw) {
    const int x = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (x >= nw || r >= rows) return;
    dst[(size_t)r * nw + x] = src[(size_t)r * nw + (nw - 1 - x)];
}

// numpy's min / max (a NaN wins), where fminf / fmaxf would drop it
__device__ __forceinline__ float np_min(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : fminf(a, b); }
__device__ __forceinline__ float np_max(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : fmaxf(a, b); }

struct CollectArgs {
    const float* boxes; const float* scores; const int64_t* classes; const int32_t* n_dev; int32_t n_host, max_rows;
    int32_t flip; float wv;                       // HFlipTransform of the variant: x = wv - x
    float sx, sy;                                 // ResizeTransform(variant -> image).apply_coords
    int32_t pre; float px, py;                    // ResizeTransform(image -> output), the mapper's pre-transform undone
    float* pool_boxes; float* pool_scores; int64_t* pool_classes; int32_t* pool_n; int32_t pool_cap;
    int32_t* var_counts; int32_t v;
};

__global__ __launch_bounds__(256) void k_tta_collect(const CollectArgs a) {
    __shared__ int s_base, s_n;
    if (threadIdx.x == 0) {
        int n = a.n_dev ? *a.n_dev : a.n_host;
        n = n < 0 ? 0 : (n > a.max_rows ? a.max_rows : n);
        const int base = a.v == 0 ? 0 : *a.pool_n;            // the first variant of an image restarts the pool
        const int room = base < 0 || base > a.pool_cap ? 0 : a.pool_cap - base;
        s_base = base;
        s_n = n > room ? room : n;                            // never past the pool (the host sizes it so that this does not cut)
    }
    __syncthreads();
    const int base = s_base, n = s_n;
    for (int i = threadIdx.x; i < n; i += 256) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(a.boxes + (size_t)i * 4);
        float x1 = b.x, y1 = b.y, x2 = b.z, y2 = b.w;
        if (a.flip) { x1 = a.wv - x1; x2 = a.wv - x2; }
        x1 = x1 * a.sx; x2 = x2 * a.sx; y1 = y1 * a.sy; y2 = y2 * a.sy;
        if (a.pre) { x1 = x1 * a.px; x2 = x2 * a.px; y1 = y1 * a.py; y2 = y2 * a.py; }
        *reinterpret_cast<f32x4*>(a.pool_boxes + (size_t)(base + i) * 4) = f32x4{np_min(x1, x2), np_min(y1, y2), np_max(x1, x2), np_max(y1, y2)};
        a.pool_scores[base + i] = a.scores[i];
        a.pool_classes[base + i] = a.classes ? a.classes[i] : 0;
    }
    if (threadIdx.x == 0) {
        *a.pool_n = base + n;
        a.var_counts[a.v] = n;
    }
}

// rows with a non-finite value dropped, Boxes.clip to (out_h, out_w), score > score_thresh.  key = the score of a row that stays, -1 of
// one that leaves (scores that stay are > score_thresh >= 0): one sort then puts the stayers first
__global__ __launch_bounds__(256) void k_tta_prepare(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                     const int32_t* __restrict__ n_ptr, int32_t cap, float out_w, float out_h,
                                                     float score_thresh, float* __restrict__ c_boxes, float* __restrict__ key) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = min(max(*n_ptr, 0), cap);
    if (i >= n) return;
    const f32x4 b = *reinterpret_cast<const f32x4*>(boxes + (size_t)i * 4);
    const float s = scores[i];
    const bool ok = finite32(b.x) && finite32(b.y) && finite32(b.z) && finite32(b.w) && finite32(s) && s > score_thresh;
    *reinterpret_cast<f32x4*>(c_boxes + (size_t)i * 4) =
        f32x4{fminf(fmaxf(b.x, 0.0f), out_w), fminf(fmaxf(b.y, 0.0f), out_h), fminf(fmaxf(b.z, 0.0f), out_w), fminf(fmaxf(b.w, 0.0f), out_h)};
    key[i] = ok ? s : -1.0f;
}

// rank of every row by (key descending, row ascending) -- 16 lanes per row, as k_nms_prep -- and the scatter of the stayers into sorted order
__global__ __launch_bounds__(256) void k_tta_rank(const float* __restrict__ c_boxes, const float* __restrict__ key,
                                                  const int64_t* __restrict__ classes, const int32_t* __restrict__ n_ptr, int32_t cap,
                                                  float* __restrict__ s_boxes, float* __restrict__ s_scores, int32_t* __restrict__ s_cls,
                                                  int32_t* __restrict__ n_valid) {
    extern __shared__ float sc[];
    __shared__ int s_cnt;
    const int n = min(max(*n_ptr, 0), cap);
    if (threadIdx.x == 0) s_cnt = 0;
    for (int i = threadIdx.x; i < n; i += 256) sc[i] = key[i];
    __syncthreads();
    const int e = blockIdx.x * 16 + (threadIdx.x >> 4), sub = threadIdx.x & 15;
    const bool valid = e < n;
    const float se = valid ? sc[e] : 0.f;
    int c = 0;
    if (valid)
        for (int f = sub; f < n; f += 16) {
            const float sf = sc[f];
            c += (sf > se || (sf == se && f < e)) ? 1 : 0;
        }
#pragma unroll
    for (int d = 8; d > 0; d >>= 1) c += __shfl_xor(c, d);
    if (valid && sub == 0 && se > 0.0f) {
        *reinterpret_cast<f32x4*>(s_boxes + (size_t)c * 4) = *reinterpret_cast<const f32x4*>(c_boxes + (size_t)e * 4);
        s_scores[c] = se;
        s_cls[c] = (int32_t)classes[e];
    }
    if (blockIdx.x == 0) {                                    // integer count of the stayers
        int m = 0;
        for (int i = threadIdx.x; i < n; i += 256) m += sc[i] > 0.0f ? 1 : 0;
        atomicAdd(&s_cnt, m);
        __syncthreads();
        if (threadIdx.x == 0) *n_valid = s_cnt;
    }
}

// word bj of row i: bit c = "sorted row i suppresses sorted row bj * 64 + c": a later row of the same class with IoU > thr
__global__ __launch_bounds__(64) void k_tta_mask(const float* __restrict__ s_boxes, const int32_t* __restrict__ s_cls,
                                                 const int32_t* __restrict__ n_ptr, float thr, unsigned long long* __restrict__ mask, int32_t words) {
    const int n = *n_ptr;
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi || bi * 64 >= n || bj * 64 >= n) return;
    __shared__ float cb[64 * 4];
    __shared__ float ca[64];
    __shared__ int cc[64];
    const int t = threadIdx.x;
    const int j0 = bj * 64 + t;
    if (j0 < n) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(s_boxes + (size_t)j0 * 4);
        cb[t * 4 + 0] = b.x; cb[t * 4 + 1] = b.y; cb[t * 4 + 2] = b.z; cb[t * 4 + 3] = b.w;
        ca[t] = (b.z - b.x) * (b.w - b.y);
        cc[t] = s_cls[j0];
    }
    __syncthreads();
    const int i = bi * 64 + t;
    if (i >= n) return;
    const f32x4 a = *reinterpret_cast<const f32x4*>(s_boxes + (size_t)i * 4);
    const float ai = (a.z - a.x) * (a.w - a.y);
    const int ci = s_cls[i];
    const int jmax = min(64, n - bj * 64);
    unsigned long long bits = 0;
    for (int c = 0; c < jmax; ++c) {
        if (bj * 64 + c <= i || cc[c] != ci) continue;
        const float xx1 = fmaxf(a.x, cb[c * 4 + 0]), yy1 = fmaxf(a.y, cb[c * 4 + 1]);
        const float xx2 = fminf(a.z, cb[c * 4 + 2]), yy2 = fminf(a.w, cb[c * 4 + 3]);
        const float w = fmaxf(0.0f, xx2 - xx1), h = fmaxf(0.0f, yy2 - yy1);
        const float inter = w * h;
        const float ovr = inter / (ai + ca[c] - inter);
        if (ovr > thr) bits |= 1ull << c;
    }
    mask[(size_t)i * words + bj] = bits;
}

// greedy scan in sorted order, one block: thread w owns word w of the removed set.  Word by word: the owner publishes its word, then
// every thread walks that word's live bits in step (the word of a kept row that covers the current word is a uniform load), and a kept
// row's later words are OR-ed into their owners' registers.  Survivor k goes to row k of the record; stops at topk.
__global__ __launch_bounds__(SCAN_T) void k_tta_scan(const float* __restrict__ s_boxes, const float* __restrict__ s_scores,
                                                     const int32_t* __restrict__ s_cls, const int32_t* __restrict__ n_ptr,
                                                     const unsigned long long* __restrict__ mask, int32_t words, int32_t topk, int32_t rec_rows,
                                                     float* __restrict__ rec, int32_t* __restrict__ out_count) {
    __shared__ unsigned long long s_cur[2];
    const int n = *n_ptr, w = threadIdx.x;
    float* rb = rec;
    float* rs = rec + (size_t)rec_rows * 4;
    int64_t* rc = reinterpret_cast<int64_t*>(rec + (size_t)rec_rows * 5);
    unsigned long long r = 0;
    int kept = 0;
    const int nw = (n + 63) >> 6;
    for (int wi = 0; wi < nw && kept < topk; ++wi) {
        if (w == wi) s_cur[wi & 1] = r;
        __syncthreads();                                      // slot wi & 1 is written again two words on, behind the next barrier
        unsigned long long cur = s_cur[wi & 1];
        const int left = n - wi * 64;
        const unsigned long long in_range = left >= 64 ? ~0ull : ((1ull << left) - 1);
        unsigned long long alive = ~cur & in_range;
        while (alive && kept < topk) {
            const int b = __builtin_ctzll(alive);
            const int i = wi * 64 + b;
            if (w == 0) {
                *reinterpret_cast<f32x4*>(rb + (size_t)kept * 4) = *reinterpret_cast<const f32x4*>(s_boxes + (size_t)i * 4);
                rs[kept] = s_scores[i];
                rc[kept] = (int64_t)s_cls[i];
            }
            ++kept;
            cur |= mask[(size_t)i * words + wi];
            if (w > wi && w < nw) r |= mask[(size_t)i * words + w];
            alive = ~cur & in_range & ~((2ull << b) - 1);
        }
    }
    if (w == 0) *out_count = kept;
}

struct MergeLayout { size_t c_boxes, key, s_boxes, s_scores, s_cls, n_valid, mask, total; int words; };
MergeLayout merge_layout(int cap) {
    MergeLayout o{};
    const size_t c = cap > 0 ? cap : 1;
    WsCursor w;
    o.c_boxes = w.take(c * 16);
    o.key = w.take(c * 4);
    o.s_boxes = w.take(c * 16);
    o.s_scores = w.take(c * 4);
    o.s_cls = w.take(c * 4);
    o.n_valid = w.take(16);
    o.words = (int)((c + 63) / 64);
    o.mask = w.take(c * (size_t)o.words * 8);
    o.total = w.o;
    return o;
}

}  // namespace

extern "C" int ore_tta_hflip_u8_fwd(const uint8_t* src, uint8_t* dst, int32_t rows, int32_t nw, void* stream) {
    ORE_CHECK_ARG(src && dst && src != dst && rows >= 1 && rows <= 65535 && nw >= 1, "ore_tta_hflip_u8_fwd: rows %d (1 .. 65535), width %d, distinct buffers", rows, nw);
    k_tta_hflip_u8<<<dim3(ceil_div(nw, 256), rows), 256, 0, (hipStream_t)stream>>>(src, dst, rows, nw);
    return ore_launch_status("k_tta_hflip_u8");
}

extern "C" int ore_tta_collect_fwd(const float* boxes, const float* scores, const int64_t* classes, const int32_t* n_dev, int32_t n_host,
                                   int32_t max_rows, int32_t flip, int32_t variant_w, float sx, float sy, int32_t pre, float px, float py,
                                   float* pool_boxes, float* pool_scores, int64_t* pool_classes, int32_t* pool_n, int32_t pool_cap,
                                   int32_t* var_counts, int32_t variant, void* stream) {
    ORE_CHECK_ARG(boxes && scores && pool_boxes && pool_scores && pool_classes && pool_n && var_counts, "ore_tta_collect_fwd: null pointer");
    ORE_CHECK_ARG(max_rows >= 0 && pool_cap >= 1 && variant >= 0 && (n_dev || n_host >= 0), "ore_tta_collect_fwd: max_rows %d, pool_cap %d, variant %d, n_host %d",
                  max_rows, pool_cap, variant, n_host);
    CollectArgs a{boxes, scores, classes, n_dev, n_host, max_rows, flip ? 1 : 0, (float)variant_w, sx, sy, pre ? 1 : 0, px, py,
                  pool_boxes, pool_scores, pool_classes, pool_n, pool_cap, var_counts, variant};
    k_tta_collect<<<1, 256, 0, (hipStream_t)stream>>>(a);
    return ore_launch_status("k_tta_collect");
}

extern "C" size_t ore_tta_merge_workspace_bytes(int32_t cap) { return cap >= 1 && cap <= TTA_MAX_CAND ? merge_layout(cap).total : 0; }

extern "C" int ore_tta_merge_fwd(const float* pool_boxes, const float* pool_scores, const int64_t* pool_classes, const int32_t* pool_n,
                                 int32_t cap, int32_t out_h, int32_t out_w, float score_thresh, float nms_thresh, int32_t topk,
                                 void* out_record, int32_t rec_rows, int32_t* out_count, void* workspace, size_t workspace_bytes, void* stream) {
    ORE_CHECK_ARG(pool_boxes && pool_scores && pool_classes && pool_n && out_record && out_count && workspace, "ore_tta_merge_fwd: null pointer");
    ORE_CHECK_ARG(cap >= 1 && cap <= TTA_MAX_CAND, "ore_tta_merge_fwd: %d candidates (1 .. %d)", cap, TTA_MAX_CAND);
    ORE_CHECK_ARG(out_h >= 1 && out_w >= 1 && score_thresh >= 0.0f && nms_thresh > 0.0f && topk >= 1 && topk <= rec_rows && rec_rows % 2 == 0,
                  "ore_tta_merge_fwd: output %dx%d, score_thresh %g (>= 0), nms_thresh %g (> 0), topk %d (1 .. the record's %d rows, an even number)",
                  out_h, out_w, (double)score_thresh, (double)nms_thresh, topk, rec_rows);
    const MergeLayout lay = merge_layout(cap);
    if (workspace_bytes < lay.total) {
        ore_set_error("ore_tta_merge_fwd: workspace %zu < %zu", workspace_bytes, lay.total);
        return ORE_ENOMEM;
    }
    static_assert(TTA_MAX_CAND / 64 <= SCAN_T, "one scan thread per mask word");
    char* ws = static_cast<char*>(workspace);
    float* c_boxes = (float*)(ws + lay.c_boxes); float* key = (float*)(ws + lay.key);
    float* s_boxes = (float*)(ws + lay.s_boxes); float* s_scores = (float*)(ws + lay.s_scores);
    int32_t* s_cls = (int32_t*)(ws + lay.s_cls); int32_t* n_valid = (int32_t*)(ws + lay.n_valid);
    unsigned long long* mask = (unsigned long long*)(ws + lay.mask);
    hipStream_t st = (hipStream_t)stream;
    int rc;
    k_tta_prepare<<<ceil_div(cap, 256), 256, 0, st>>>(pool_boxes, pool_scores, pool_n, cap, (float)out_w, (float)out_h, score_thresh, c_boxes, key);
    if ((rc = ore_launch_status("k_tta_prepare"))) return rc;
    k_tta_rank<<<ceil_div(cap, 16), 256, (size_t)cap * 4, st>>>(c_boxes, key, pool_classes, pool_n, cap, s_boxes, s_scores, s_cls, n_valid);
    if ((rc = ore_launch_status("k_tta_rank"))) return rc;
    k_tta_mask<<<dim3(lay.words, lay.words), 64, 0, st>>>(s_boxes, s_cls, n_valid, nms_thresh, mask, lay.words);
    if ((rc = ore_launch_status("k_tta_mask"))) return rc;
    k_tta_scan<<<1, SCAN_T, 0, st>>>(s_boxes, s_scores, s_cls, n_valid, mask, lay.words, topk, rec_rows, (float*)out_record, out_count);
    return ore_launch_status("k_tta_scan");
}
