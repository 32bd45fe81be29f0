// COCO box AP on the device (detectron2.evaluation.COCOEvaluator): pycocotools' COCOeval for iouType "bbox", useCats = 1, restated
// from its published definition (evaluateImg + accumulate).  Every result is bit-exact against that definition: the IoU is the same
// fp64 expression evaluated in the same order (this file is compiled with -ffp-contract=off), matching and ordering use comparisons
// only, prefix sums are integer, and no float atomics are used (the one LDS atomic is an integer max of non-negative fp64 bit
// patterns, which is order independent).
//
// Stages, all enqueued on one stream, grids sized by host-known upper bounds (the device counts live in the workspace header):
//   k_det_count     detections per (category, image) pair
//   k_pairs_scan    one block: units (pairs with a GT or a detection), bucket offsets, kept-detection offsets
//   k_det_bucket    detections scattered into their pair's bucket (arbitrary order inside a bucket)
//   k_det_rank      rank of a detection in its pair: score descending, then input row (= the results json order, pycocotools' stable
//                   mergesort); ranks < maxDets[-1] are kept
//   k_unit_match    one wave per unit: fp64 IoU matrix (LDS, or global past the LDS size), then one lane per (area, threshold) chain
//                   running the greedy match over the unit's detections; writes a 2-bit code per (unit, area, threshold, rank) and the
//                   per-area count of non-ignored GTs; also the unit's sort keys
//   k_bitonic_*     bitonic sort of the kept detections by (category, score descending, image, rank) -- a unique key
//   k_elem_flags    per sorted detection: TP / FP bit masks over the (area, threshold) chains, rank, score
//   k_accumulate    one block per (threshold, category, area, maxDet): integer prefix sums of TP / FP, recall and precision, the
//                   right-to-left precision envelope and searchsorted(side='left') at the recall thresholds, through recall buckets
#include "ore_block.h"

namespace {

constexpr int kMaxT = 16, kMaxR = 128, kMaxA = 8, kMaxM = 4;
constexpr int kMatched = 1, kIgnored = 2;       // per-chain detection code
constexpr int kIouLds = 6144;                   // IoU matrix in LDS up to this many fp64 entries
constexpr int kGtmLds = 8192;                   // GT-matched flags in LDS up to this many bytes (chains x GTs)
constexpr int kAccThreads = 256, kAccPer = 16;  // accumulate: threads per block, consecutive elements per thread and tile
constexpr int kCntBits = 21;                    // accumulate packs three counters < 2^21 into one 64-bit scan word

struct Params {
    double iou[kMaxT];
    double rec[kMaxR];
    double area[kMaxA][2];
    int32_t max_dets[kMaxM];
    int32_t T, R, A, M;
};

struct Key {
    uint64_t hi, lo;   // hi: category << 32 | descending score bits; lo: image << 32 | rank
};

struct key_gt {
    __device__ __forceinline__ bool operator()(const Key& a, const Key& b) const { return a.hi > b.hi || (a.hi == b.hi && a.lo > b.lo); }
};

__device__ __forceinline__ uint32_t score_desc_bits(float s) {
    if (s == 0.0f) s = 0.0f;                    // -0 and +0 compare equal in the reference's sort
    const uint32_t u = __float_as_uint(s);
    return ~((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}

struct Ws {
    size_t hdr, d_cnt, d_fill, d_off, unit_of_pair, ekoff, ukoff, unit_pair, unit_eoff, unit_det, bucket, codes, npig, gtm, iou, keys,
        e_rank, e_score, e_tp, e_fp, total;
    int64_t KI, U, P;
};

inline int64_t units_cap(int64_t KI, int64_t N, int64_t G) { return KI < N + G ? KI : N + G; }

inline Ws ws_layout(int32_t K, int32_t I, int32_t N, int32_t G, int32_t AT, int32_t maxD) {
    Ws w{};
    w.KI = (int64_t)K * I;
    w.U = units_cap(w.KI, N, G);
    w.P = bitonic_size(N);
    WsCursor c;
    w.hdr = c.take(256);
    w.d_cnt = c.take(w.KI * 4);
    w.d_fill = c.take(w.KI * 4);
    w.d_off = c.take(w.KI * 4);
    w.unit_of_pair = c.take(w.KI * 4);
    w.ekoff = c.take((size_t)(K + 1) * 4);
    w.ukoff = c.take((size_t)(K + 1) * 4);
    w.unit_pair = c.take(w.U * 4);
    w.unit_eoff = c.take(w.U * 4);
    w.unit_det = c.take(w.U * maxD * 4);
    w.bucket = c.take((size_t)N * 4);
    w.codes = c.take(w.U * AT * maxD);
    w.npig = c.take(w.U * kMaxA * 4);
    w.gtm = c.take((size_t)G * AT);
    w.iou = c.take((size_t)G * maxD * 8);
    w.keys = c.take(w.P * sizeof(Key));
    w.e_rank = c.take(w.P * 4);
    w.e_score = c.take(w.P * 4);
    w.e_tp = c.take(w.P * 8);
    w.e_fp = c.take(w.P * 8);
    w.total = c.o;
    return w;
}

// ------------------------------------------------------------------ grouping

__global__ void k_det_count(const int32_t* det_image, const int32_t* det_cat, int32_t N, int32_t K, int32_t I, int32_t* d_cnt) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const int k = det_cat[j], i = det_image[j];
    if (k < 0 || k >= K || i < 0 || i >= I) return;             // not an evaluated category / image: dropped
    atomicAdd(&d_cnt[(int64_t)k * I + i], 1);
}

__global__ __launch_bounds__(1024) void k_pairs_scan(const int32_t* d_cnt, const int32_t* gt_off, int32_t K, int32_t I, int32_t maxD,
                                                     int32_t* d_off, int32_t* unit_of_pair, int32_t* unit_pair, int32_t* unit_eoff,
                                                     int32_t* ekoff, int32_t* ukoff, int32_t* hdr) {
    __shared__ int64_t sh[16];
    const int64_t KI = (int64_t)K * I;
    int64_t cu = 0, cd = 0, ce = 0;                              // running units, bucketed detections, kept detections
    for (int64_t base = 0; base < KI; base += 1024) {
        const int64_t p = base + threadIdx.x;
        int dc = 0, gc = 0;
        if (p < KI) {
            dc = d_cnt[p];
            gc = gt_off[p + 1] - gt_off[p];
        }
        const int has = (dc > 0 || gc > 0) ? 1 : 0, kept = dc < maxD ? dc : maxD;
        // three exclusive scans in one word: units per tile <= 1024 (11 bits), detections < 2^21 (the host bounds N)
        int64_t tot;
        const int64_t packed = (int64_t)has | ((int64_t)dc << 11) | ((int64_t)kept << 32);
        const int64_t inc = block_incl_scan<16>(packed, sh, tot) - packed;
        const int64_t eu = cu + (inc & 0x7ff), ed = cd + ((inc >> 11) & 0x1fffff), ee = ce + (inc >> 32);
        if (p < KI) {
            d_off[p] = (int32_t)ed;
            unit_of_pair[p] = has ? (int32_t)eu : -1;
            if (has) {
                unit_pair[eu] = (int32_t)p;
                unit_eoff[eu] = (int32_t)ee;
            }
            if (p % I == 0) {
                ukoff[p / I] = (int32_t)eu;
                ekoff[p / I] = (int32_t)ee;
            }
        }
        cu += tot & 0x7ff;
        cd += (tot >> 11) & 0x1fffff;
        ce += tot >> 32;
    }
    if (threadIdx.x == 0) {
        ukoff[K] = (int32_t)cu;
        ekoff[K] = (int32_t)ce;
        hdr[0] = (int32_t)cu;
        hdr[1] = (int32_t)ce;
    }
}

__global__ void k_det_bucket(const int32_t* det_image, const int32_t* det_cat, int32_t N, int32_t K, int32_t I, const int32_t* d_off,
                             int32_t* d_fill, int32_t* bucket) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const int k = det_cat[j], i = det_image[j];
    if (k < 0 || k >= K || i < 0 || i >= I) return;
    const int64_t p = (int64_t)k * I + i;
    bucket[d_off[p] + atomicAdd(&d_fill[p], 1)] = j;
}

__global__ void k_det_rank(const float* det_scores, const int32_t* det_image, const int32_t* det_cat, int32_t N, int32_t K, int32_t I,
                           int32_t maxD, const int32_t* d_cnt, const int32_t* d_off, const int32_t* bucket, const int32_t* unit_of_pair,
                           int32_t* unit_det) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const int k = det_cat[j], i = det_image[j];
    if (k < 0 || k >= K || i < 0 || i >= I) return;
    const int64_t p = (int64_t)k * I + i;
    const float s = det_scores[j];
    const int n = d_cnt[p], o = d_off[p];
    int rank = 0;
    for (int q = 0; q < n; ++q) {
        const int jj = bucket[o + q];
        const float ss = det_scores[jj];
        rank += (ss > s || (ss == s && jj < j)) ? 1 : 0;
    }
    if (rank < maxD) unit_det[(int64_t)unit_of_pair[p] * maxD + rank] = j;
}

// ------------------------------------------------------------------ per-image stage

// maskApi bbIou for one (detection, GT) pair; boxes xywh in fp64
__device__ __forceinline__ double bb_iou(const double* D, double da, const double* Gb, int crowd) {
    const double ga = Gb[2] * Gb[3];
    const double w = fmin(D[2] + D[0], Gb[2] + Gb[0]) - fmax(D[0], Gb[0]);
    if (w <= 0) return 0.0;
    const double h = fmin(D[3] + D[1], Gb[3] + Gb[1]) - fmax(D[1], Gb[1]);
    if (h <= 0) return 0.0;
    const double i = w * h;
    const double u = crowd ? da : da + ga - i;
    return i / u;
}

__device__ __forceinline__ bool gt_ignored(const double* gt_area, const int32_t* gt_crowd, int g, double lo, double hi) {
    const double a = gt_area[g];
    return gt_crowd[g] != 0 || a < lo || a > hi;
}

__global__ __launch_bounds__(64) void k_unit_match(Params P, const float* det_boxes, const float* det_scores, const double* gt_boxes,
                                                   const double* gt_area, const int32_t* gt_crowd, const int64_t* gt_id,
                                                   const int32_t* gt_off, int32_t I, int32_t maxD, const int32_t* hdr,
                                                   const int32_t* unit_pair, const int32_t* unit_eoff, const int32_t* unit_det,
                                                   uint8_t* codes, int32_t* npig, uint8_t* gtm_ws, double* iou_ws,
                                                   Key* keys, int64_t* out_matches, uint8_t* out_ignore, int32_t* out_npig) {
    __shared__ double s_det[128][4];
    __shared__ double s_da[128];
    __shared__ double s_iou[kIouLds];
    __shared__ uint8_t s_gtm[kGtmLds];
    const int u = blockIdx.x;
    if (u >= hdr[0]) return;
    const int p = unit_pair[u], k = p / I, img = p % I;
    const int g0 = gt_off[p], G = gt_off[p + 1] - g0;
    const int e0 = unit_eoff[u];
    const int nk = (u + 1 < hdr[0]) ? unit_eoff[u + 1] : hdr[1];
    const int D = nk - e0;
    const int AT = P.A * P.T;
    const int tid = threadIdx.x;
    for (int d = tid; d < D; d += 64) {
        const int j = unit_det[(int64_t)u * maxD + d];
        const float x0 = det_boxes[4 * j], y0 = det_boxes[4 * j + 1], x1 = det_boxes[4 * j + 2], y1 = det_boxes[4 * j + 3];
        const float w = x1 - x0, h = y1 - y0;                  // instances_to_coco_json: XYXY -> XYWH in fp32
        s_det[d][0] = x0;
        s_det[d][1] = y0;
        s_det[d][2] = w;
        s_det[d][3] = h;
        s_da[d] = (double)w * (double)h;                         // loadRes: area = bb[2] * bb[3]
        const float s = det_scores[j];
        Key key;
        key.hi = ((uint64_t)k << 32) | score_desc_bits(s);
        key.lo = ((uint64_t)img << 32) | (uint32_t)d;
        keys[e0 + d] = key;
    }
    const bool iou_lds = (int64_t)D * G <= kIouLds;
    const bool gtm_lds = (int64_t)AT * G <= kGtmLds;
    double* iou = iou_lds ? s_iou : iou_ws + (int64_t)g0 * maxD;
    uint8_t* gtm = gtm_lds ? s_gtm : gtm_ws + (int64_t)g0 * AT;
    __syncthreads();
    for (int64_t q = tid; q < (int64_t)D * G; q += 64) {
        const int d = (int)(q / G), g = (int)(q % G);
        iou[q] = bb_iou(s_det[d], s_da[d], gt_boxes + 4 * (int64_t)(g0 + g), gt_crowd[g0 + g]);
    }
    for (int64_t q = tid; q < (int64_t)AT * G; q += 64) gtm[q] = 0;
    if (tid < P.A) {
        int c = 0;
        for (int g = 0; g < G; ++g) c += gt_ignored(gt_area, gt_crowd, g0 + g, P.area[tid][0], P.area[tid][1]) ? 0 : 1;
        npig[(int64_t)u * kMaxA + tid] = c;
        if (out_npig) out_npig[(int64_t)u * P.A + tid] = c;
    }
    __syncthreads();                                             // global-memory IoU / flags: workgroup scope suffices (same block)
    if (tid < AT) {
        const int a = tid / P.T, t = tid % P.T;
        const double lo = P.area[a][0], hi = P.area[a][1];
        const double thr = fmin(P.iou[t], 1 - 1e-10);
        uint8_t* m_flags = gtm + (int64_t)tid * G;
        uint8_t* code = codes + ((int64_t)u * AT + tid) * maxD;
        for (int d = 0; d < D; ++d) {
            double best = thr;
            int m = -1;
            // GTs in the stable order of their ignore flag: the non-ignored ones, then (only if none matched) the ignored ones
            for (int phase = 0; phase < 2 && m < 0; ++phase) {
                for (int g = 0; g < G; ++g) {
                    if (gt_ignored(gt_area, gt_crowd, g0 + g, lo, hi) != (phase == 1)) continue;
                    if (m_flags[g] && !gt_crowd[g0 + g]) continue;
                    const double v = iou[(int64_t)d * G + g];
                    if (v < best) continue;
                    best = v;
                    m = g;
                }
            }
            int c = 0;
            int64_t mid = 0;
            if (m >= 0) {
                m_flags[m] = 1;
                mid = gt_id[g0 + m];
                c = (mid != 0 ? kMatched : 0) | (gt_ignored(gt_area, gt_crowd, g0 + m, lo, hi) ? kIgnored : 0);
            }
            if (!(c & kMatched) && (s_da[d] < lo || s_da[d] > hi)) c |= kIgnored;
            code[d] = (uint8_t)c;
            if (out_matches) {
                const int64_t o = (((int64_t)u * P.A + a) * P.T + t) * maxD + d;
                out_matches[o] = mid;
                out_ignore[o] = (c & kIgnored) ? 1 : 0;
            }
        }
    }
}

// ------------------------------------------------------------------ sort

__global__ void k_keys_fill(Key* keys, const int32_t* hdr, int64_t P) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < P && e >= hdr[1]) keys[e] = Key{~0ull, ~0ull};
}

// ------------------------------------------------------------------ accumulate

__global__ void k_elem_flags(const Key* keys, const int32_t* hdr, int32_t I, int32_t AT, int32_t maxD, const int32_t* unit_of_pair,
                             const int32_t* unit_det, const float* det_scores, const uint8_t* codes, int32_t* e_rank, float* e_score,
                             uint64_t* e_tp, uint64_t* e_fp) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= hdr[1]) return;
    const Key key = keys[e];
    const int k = (int)(key.hi >> 32), img = (int)(key.lo >> 32), r = (int)(key.lo & 0xffffffffu);
    const int u = unit_of_pair[(int64_t)k * I + img];
    uint64_t tp = 0, fp = 0;
    for (int c = 0; c < AT; ++c) {
        const int code = codes[((int64_t)u * AT + c) * maxD + r];
        if (!(code & kIgnored)) {
            if (code & kMatched) tp |= 1ull << c;
            else fp |= 1ull << c;
        }
    }
    e_rank[e] = r;
    e_score[e] = det_scores[unit_det[(int64_t)u * maxD + r]];
    e_tp[e] = tp;
    e_fp[e] = fp;
}

// number of recall thresholds <= rc, minus one: the last r whose searchsorted(side='left') index is at or before this element
__device__ __forceinline__ int rec_bucket(const double* rec, int R, double rc) {
    int lo = 0, hi = R;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rec[mid] <= rc) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

__global__ __launch_bounds__(kAccThreads) void k_accumulate(Params P, int32_t K, const int32_t* ekoff, const int32_t* ukoff,
                                                            const int32_t* npig, const int32_t* e_rank, const float* e_score,
                                                            const uint64_t* e_tp, const uint64_t* e_fp, double* precision,
                                                            double* recall, double* scores) {
    __shared__ int64_t sh[kAccThreads / 64];
    __shared__ double s_rec[kMaxR];
    __shared__ unsigned long long s_bmax[kMaxR];
    __shared__ float s_ss[kMaxR];
    __shared__ int s_npig;
    const int R = P.R;
    int b = blockIdx.x;
    const int m = b % P.M;
    b /= P.M;
    const int a = b % P.A;
    b /= P.A;
    const int k = b % K;
    const int t = b / K;
    const int tid = threadIdx.x;
    const int64_t ob = (((int64_t)t * R) * K + k) * P.A * P.M + (int64_t)a * P.M + m;    // precision[t][0][k][a][m]
    const int64_t rstride = (int64_t)K * P.A * P.M;
    for (int r = tid; r < R; r += kAccThreads) {
        s_rec[r] = P.rec[r];
        s_bmax[r] = 0;
        s_ss[r] = 0.0f;
    }
    if (tid == 0) {
        int c = 0;
        for (int u = ukoff[k]; u < ukoff[k + 1]; ++u) c += npig[(int64_t)u * kMaxA + a];
        s_npig = c;
    }
    __syncthreads();
    const int n_units = ukoff[k + 1] - ukoff[k];
    const int np = s_npig;
    double* rec_out = recall + (((int64_t)t * K + k) * P.A + a) * P.M + m;
    if (n_units == 0 || np == 0) {                              // no image of this category, or no non-ignored GT: -1 stays
        for (int r = tid; r < R; r += kAccThreads) {
            precision[ob + r * rstride] = -1.0;
            scores[ob + r * rstride] = -1.0;
        }
        if (tid == 0) *rec_out = -1.0;
        return;
    }
    const int maxDet = P.max_dets[m];
    const uint64_t bit = 1ull << (a * P.T + t);
    const double dnp = (double)np;
    const double eps = 2.220446049250313e-16;
    const int e0 = ekoff[k], e1 = ekoff[k + 1];
    const int64_t mask = (1ll << kCntBits) - 1;
    int64_t carry = 0;                                           // incl | tp << 21 | fp << 42 of the tiles before
    for (int base = e0; base < e1; base += kAccThreads * kAccPer) {
        const int first = base + tid * kAccPer;
        int64_t v[kAccPer];
        int64_t run = 0;
#pragma unroll
        for (int q = 0; q < kAccPer; ++q) {
            const int e = first + q;
            int64_t c = 0;
            if (e < e1 && e_rank[e] < maxDet) c = 1 | ((int64_t)((e_tp[e] & bit) != 0) << kCntBits) | ((int64_t)((e_fp[e] & bit) != 0) << (2 * kCntBits));
            run += c;
            v[q] = c;
        }
        int64_t tot;
        const int64_t pre = carry + block_incl_scan<kAccThreads / 64>(run, sh, tot) - run;
        int64_t acc = pre;
#pragma unroll
        for (int q = 0; q < kAccPer; ++q) {
            if (!v[q]) continue;
            acc += v[q];
            const int64_t n = acc & mask, tp = (acc >> kCntBits) & mask, fp = acc >> (2 * kCntBits);
            const int64_t own_tp = (v[q] >> kCntBits) & 1;
            const double dtp = (double)tp;
            const double rc = dtp / dnp;
            const double pr = dtp / ((double)fp + dtp + eps);
            const int B = rec_bucket(s_rec, R, rc);
            if (B >= 0) atomicMax(&s_bmax[B], (unsigned long long)__double_as_longlong(pr));
            const int Bprev = n == 1 ? -1 : rec_bucket(s_rec, R, (double)(tp - own_tp) / dnp);
            const float sc = e_score[first + q];
            for (int r = Bprev + 1; r <= B; ++r) s_ss[r] = sc;       // this element is searchsorted's answer for these thresholds
        }
        carry += tot;
    }
    __syncthreads();
    if (tid == 0) {
        const int64_t nd = carry & mask, tp = (carry >> kCntBits) & mask;
        const int Blast = nd ? rec_bucket(s_rec, R, (double)tp / dnp) : -1;
        *rec_out = nd ? (double)tp / dnp : 0.0;
        double run = 0.0;
        for (int r = R - 1; r >= 0; --r) {
            const double v = __longlong_as_double((long long)s_bmax[r]);
            run = v > run ? v : run;
            precision[ob + r * rstride] = r <= Blast ? run : 0.0;
            scores[ob + r * rstride] = r <= Blast ? (double)s_ss[r] : 0.0;
        }
    }
}

}  // namespace

extern "C" size_t ore_coco_eval_workspace_bytes(int32_t n_cats, int32_t n_images, int32_t n_dets, int32_t n_gts, int32_t n_iou_thrs,
                                                int32_t n_areas, int32_t max_det) {
    if (n_cats <= 0 || n_images <= 0 || n_dets < 0 || n_gts < 0 || n_iou_thrs <= 0 || n_areas <= 0 || max_det <= 0) return 0;
    return ws_layout(n_cats, n_images, n_dets, n_gts, n_areas * n_iou_thrs, max_det).total;
}

extern "C" int ore_coco_eval(const ore_coco_eval_desc* d, const ore_coco_eval_images* per_image, void* stream) {
    ORE_CHECK_ARG(d != nullptr, "ore_coco_eval: desc is NULL");
    const int32_t K = d->n_cats, I = d->n_images, N = d->n_dets, G = d->n_gts;
    ORE_CHECK_ARG(K > 0 && I > 0 && N >= 0 && G >= 0, "ore_coco_eval: n_cats %d, n_images %d, n_dets %d, n_gts %d", K, I, N, G);
    ORE_CHECK_ARG(d->n_iou_thrs > 0 && d->n_iou_thrs <= kMaxT && d->n_rec_thrs > 0 && d->n_rec_thrs <= kMaxR && d->n_areas > 0 &&
                      d->n_areas <= kMaxA && d->n_max_dets > 0 && d->n_max_dets <= kMaxM && d->n_areas * d->n_iou_thrs <= 64,
                  "ore_coco_eval: T %d (<= %d), R %d (<= %d), A %d (<= %d), M %d (<= %d), A*T <= 64", d->n_iou_thrs, kMaxT,
                  d->n_rec_thrs, kMaxR, d->n_areas, kMaxA, d->n_max_dets, kMaxM);
    ORE_CHECK_ARG(d->iou_thrs_host && d->rec_thrs_host && d->area_rngs_host && d->max_dets_host, "ore_coco_eval: parameter arrays are NULL");
    ORE_CHECK_ARG((int64_t)K * I < (1ll << 31), "ore_coco_eval: n_cats * n_images too large");
    ORE_CHECK_ARG(N < (1 << kCntBits), "ore_coco_eval: n_dets %d must be < %d", N, 1 << kCntBits);
    ORE_CHECK_ARG((N == 0 || (d->det_boxes && d->det_scores && d->det_image && d->det_cat)) && d->gt_off &&
                      (G == 0 || (d->gt_boxes && d->gt_area && d->gt_crowd && d->gt_id)) && d->precision && d->recall && d->scores,
                  "ore_coco_eval: a required device pointer is NULL");
    Params P{};
    P.T = d->n_iou_thrs;
    P.R = d->n_rec_thrs;
    P.A = d->n_areas;
    P.M = d->n_max_dets;
    int32_t maxD = 0;
    for (int t = 0; t < P.T; ++t) P.iou[t] = d->iou_thrs_host[t];
    for (int r = 0; r < P.R; ++r) P.rec[r] = d->rec_thrs_host[r];
    for (int r = 1; r < P.R; ++r) ORE_CHECK_ARG(P.rec[r - 1] <= P.rec[r], "ore_coco_eval: recall thresholds must be non-decreasing");
    for (int a = 0; a < P.A; ++a) {
        P.area[a][0] = d->area_rngs_host[2 * a];
        P.area[a][1] = d->area_rngs_host[2 * a + 1];
    }
    for (int m = 0; m < P.M; ++m) {
        P.max_dets[m] = d->max_dets_host[m];
        ORE_CHECK_ARG(P.max_dets[m] > 0 && P.max_dets[m] >= maxD, "ore_coco_eval: max_dets must be positive and non-decreasing");
        maxD = P.max_dets[m];
    }
    ORE_CHECK_ARG(maxD <= 128, "ore_coco_eval: max_dets[-1] %d > 128", maxD);
    const int AT = P.A * P.T;
    const Ws w = ws_layout(K, I, N, G, AT, maxD);
    ORE_CHECK_ARG(d->workspace && d->workspace_bytes >= w.total, "ore_coco_eval: workspace %zu bytes < %zu (ore_coco_eval_workspace_bytes)",
                  d->workspace_bytes, w.total);
    if (per_image) {
        ORE_CHECK_ARG(per_image->capacity >= w.U && per_image->n_units && per_image->unit_pair && per_image->det_index &&
                          per_image->dt_matches && per_image->dt_ignore && per_image->gt_npig,
                      "ore_coco_eval: per-image output needs every pointer and capacity >= %lld units", (long long)w.U);
    }
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)d->workspace;
    int32_t* hdr = (int32_t*)(ws + w.hdr);
    int32_t* d_cnt = (int32_t*)(ws + w.d_cnt);
    int32_t* d_fill = (int32_t*)(ws + w.d_fill);
    int32_t* d_off = (int32_t*)(ws + w.d_off);
    int32_t* unit_of_pair = (int32_t*)(ws + w.unit_of_pair);
    int32_t* ekoff = (int32_t*)(ws + w.ekoff);
    int32_t* ukoff = (int32_t*)(ws + w.ukoff);
    int32_t* unit_pair = (int32_t*)(ws + w.unit_pair);
    int32_t* unit_eoff = (int32_t*)(ws + w.unit_eoff);
    int32_t* unit_det = (int32_t*)(ws + w.unit_det);
    int32_t* bucket = (int32_t*)(ws + w.bucket);
    uint8_t* codes = (uint8_t*)(ws + w.codes);
    int32_t* npig = (int32_t*)(ws + w.npig);
    Key* keys = (Key*)(ws + w.keys);
    int32_t* e_rank = (int32_t*)(ws + w.e_rank);
    float* e_score = (float*)(ws + w.e_score);
    uint64_t* e_tp = (uint64_t*)(ws + w.e_tp);
    uint64_t* e_fp = (uint64_t*)(ws + w.e_fp);

    ORE_HIP(hipMemsetAsync(hdr, 0, 256, s));
    ORE_HIP(hipMemsetAsync(d_cnt, 0, w.KI * 4, s));
    ORE_HIP(hipMemsetAsync(d_fill, 0, w.KI * 4, s));
    const int nb = ceil_div(N > 0 ? N : 1, 256);
    if (N > 0) hipLaunchKernelGGL(k_det_count, dim3(nb), dim3(256), 0, s, d->det_image, d->det_cat, N, K, I, d_cnt);
    hipLaunchKernelGGL(k_pairs_scan, dim3(1), dim3(1024), 0, s, d_cnt, d->gt_off, K, I, maxD, d_off, unit_of_pair, unit_pair, unit_eoff,
                       ekoff, ukoff, hdr);
    if (N > 0) {
        hipLaunchKernelGGL(k_det_bucket, dim3(nb), dim3(256), 0, s, d->det_image, d->det_cat, N, K, I, d_off, d_fill, bucket);
        hipLaunchKernelGGL(k_det_rank, dim3(nb), dim3(256), 0, s, d->det_scores, d->det_image, d->det_cat, N, K, I, maxD, d_cnt, d_off,
                           bucket, unit_of_pair, unit_det);
    }
    if (w.U > 0) {
        hipLaunchKernelGGL(k_unit_match, dim3((unsigned)w.U), dim3(64), 0, s, P, d->det_boxes, d->det_scores, d->gt_boxes, d->gt_area,
                           d->gt_crowd, d->gt_id, d->gt_off, I, maxD, hdr, unit_pair, unit_eoff, unit_det, codes, npig,
                           (uint8_t*)(ws + w.gtm), (double*)(ws + w.iou), keys, per_image ? per_image->dt_matches : nullptr,
                           per_image ? per_image->dt_ignore : nullptr, per_image ? per_image->gt_npig : nullptr);
    }
    hipLaunchKernelGGL(k_keys_fill, dim3((unsigned)ceil_div((int)w.P, 256)), dim3(256), 0, s, keys, hdr, w.P);
    bitonic_sort_rows<Key, key_gt>(keys, w.P, 1, s);
    hipLaunchKernelGGL(k_elem_flags, dim3((unsigned)ceil_div((int)w.P, 256)), dim3(256), 0, s, keys, hdr, I, AT, maxD, unit_of_pair,
                       unit_det, d->det_scores, codes, e_rank, e_score, e_tp, e_fp);
    hipLaunchKernelGGL(k_accumulate, dim3((unsigned)(P.T * K * P.A * P.M)), dim3(kAccThreads), 0, s, P, K, ekoff, ukoff, npig, e_rank,
                       e_score, e_tp, e_fp, d->precision, d->recall, d->scores);
    if (per_image) {
        ORE_HIP(hipMemcpyAsync(per_image->n_units, hdr, 4, hipMemcpyDeviceToDevice, s));
        ORE_HIP(hipMemcpyAsync(per_image->unit_pair, unit_pair, w.U * 4, hipMemcpyDeviceToDevice, s));
        ORE_HIP(hipMemcpyAsync(per_image->det_index, unit_det, w.U * maxD * 4, hipMemcpyDeviceToDevice, s));
    }
    return ore_launch_status("ore_coco_eval");
}
