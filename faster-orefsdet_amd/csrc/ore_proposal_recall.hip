// Proposal recall on the device (detectron2.evaluation.COCOEvaluator "box_proposals"): the reference's _evaluate_box_proposals
// (ref:fewx/evaluation/coco_evaluation.py:453-561) for all (limit, area range) chains in one call.  Bit-exact: the IoU is the fp32
// expression of detectron2's pairwise_iou in its order (this file is compiled with -ffp-contract=off), everything after it is
// comparisons and integer counting.  The one atomic is an integer add (num_pos), which is order independent.
//
// Stages, all on one stream:
//   k_entry_scan   one block: per entry, the offset of its slot region (one slot per GT of its image) and of its IoU matrix in the
//                  workspace (only matrices past the LDS size get room there)
//   k_entry        one block per entry, 8 waves: proposal ranks (logit descending, input order on ties), the image's non-crowd GTs as
//                  fp32 XYXY, the IoU matrix of the first max-limit proposals x non-crowd GTs (LDS, or the workspace); then one wave per
//                  chain.  Its lanes own the GT columns g = lane, lane + 64, ... and keep (column max over the live rows, first arg-max
//                  row) for each; a step is one wave reduction on (value, lowest GT), the winner's column and row are retired (rows: a
//                  bit mask spread over the lanes, 32 rows each) and only the columns whose arg-max row was retired are scanned again.
//                  The recorded vector goes into the chain's key row at the entry's slots; unused slots keep the all-ones pattern.
//   k_bitonic_*    bitonic sort of every chain's key row (non-negative fp32 bit patterns order as unsigned integers; all-ones last)
//   k_counts       per (chain, threshold): num_pos minus the lower bound of the threshold in the sorted row
#include "ore_block.h"

namespace {

constexpr int kMaxA = 8, kMaxL = 4, kMaxChains = 8, kMaxT = 16;
constexpr int kMaxRows = 2048;                  // largest limit: the retired-row mask is 32 rows per lane
constexpr int kIouLds = 11264;                  // IoU matrix in LDS up to this many fp32 cells (rows x the image's GT count)
constexpr int kColLds = 256;                    // column state in LDS up to this many non-crowd GTs
constexpr int kThreads = 64 * kMaxChains;
constexpr int kGtStride = 6;                    // x0, y0, x1, y1, box area, fp32(json area)

struct Params {
    float lo[kMaxA], hi[kMaxA], thr[kMaxT];
    int32_t limit[kMaxL];
    int32_t A, L, T, maxR;
};

struct Ws {
    size_t slot_off, iou_off, order, gtb, cmax, carg, valid, iou, keys, total;
    int64_t P;
};

inline Ws ws_layout(int32_t E, int32_t N, int32_t S, int64_t cells, int32_t AL) {
    Ws w{};
    w.P = bitonic_size(S);
    WsCursor c;
    w.slot_off = c.take((size_t)(E + 1) * 4);
    w.iou_off = c.take((size_t)(E + 1) * 8);
    w.order = c.take((size_t)N * 4);
    w.gtb = c.take((size_t)S * kGtStride * 4);
    w.cmax = c.take((size_t)S * AL * 4);
    w.carg = c.take((size_t)S * AL * 4);
    w.valid = c.take((size_t)E * AL * 4);
    w.iou = c.take((size_t)cells * 4);
    w.keys = c.take((size_t)w.P * AL * 4);
    w.total = c.o;
    return w;
}

struct Entry {
    int p0, P, g0, G;                           // proposal rows, the image's GT rows (crowd included)
    bool ok;
};

__device__ __forceinline__ Entry read_entry(int e, const int32_t* entry_off, const int32_t* entry_image, const int32_t* gt_off, int32_t N,
                                            int32_t I, int32_t Gt) {
    Entry r{0, 0, 0, 0, false};
    const int p0 = entry_off[e], p1 = entry_off[e + 1], img = entry_image[e];
    if (p0 < 0 || p1 < p0 || p1 > N || img < 0 || img >= I) return r;
    const int g0 = gt_off[img], g1 = gt_off[img + 1];
    if (g0 < 0 || g1 < g0 || g1 > Gt) return r;
    return Entry{p0, p1 - p0, g0, g1 - g0, true};
}

__device__ __forceinline__ int64_t matrix_cells(const Entry& en, int maxR) { return (int64_t)(en.P < maxR ? en.P : maxR) * en.G; }

__global__ __launch_bounds__(1024) void k_entry_scan(const int32_t* entry_off, const int32_t* entry_image, const int32_t* gt_off, int32_t E,
                                                     int32_t N, int32_t I, int32_t Gt, int32_t maxR, int32_t* slot_off, int64_t* iou_off,
                                                     int32_t* status) {
    __shared__ int64_t sh[16];
    int64_t cs = 0, cc = 0;
    for (int base = 0; base < E; base += 1024) {
        const int e = base + threadIdx.x;
        int64_t slots = 0, cells = 0;
        if (e < E) {
            const Entry en = read_entry(e, entry_off, entry_image, gt_off, N, I, Gt);
            if (!en.ok) *status = 1;
            slots = en.G;
            const int64_t c = matrix_cells(en, maxR);
            cells = c > kIouLds ? c : 0;
        }
        int64_t ts, tc;
        const int64_t is = block_incl_scan<16>(slots, sh, ts), ic = block_incl_scan<16>(cells, sh, tc);
        if (e < E) {
            const int64_t so = cs + is - slots;
            slot_off[e] = (int32_t)(so < 0x7fffffff ? so : 0x7fffffff);
            iou_off[e] = cc + ic - cells;
        }
        cs += ts;
        cc += tc;
    }
    if (threadIdx.x == 0) {
        slot_off[E] = (int32_t)(cs < 0x7fffffff ? cs : 0x7fffffff);
        iou_off[E] = cc;
    }
}

__global__ __launch_bounds__(kThreads) void k_entry(Params P, const float* prop_boxes, const float* prop_logits, const int32_t* entry_off,
                                                    const int32_t* entry_image, const double* gt_boxes, const double* gt_area,
                                                    const int32_t* gt_crowd, const int32_t* gt_off, int32_t N, int32_t I, int32_t Gt,
                                                    int32_t n_slots, int64_t n_iou_cells, int64_t Psort, const int32_t* slot_off,
                                                    const int64_t* iou_off, int32_t* order, float* gtb, float* cmax_ws, int32_t* carg_ws,
                                                    float* iou_ws, uint32_t* keys, int32_t* valid, unsigned long long* num_pos,
                                                    int32_t* status) {
    __shared__ float s_iou[kIouLds];
    __shared__ float s_cmax[kMaxChains][kColLds];
    __shared__ int32_t s_carg[kMaxChains][kColLds];
    __shared__ int s_gnc;
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int AL = P.A * P.L;
    const Entry en = read_entry(e, entry_off, entry_image, gt_off, N, I, Gt);
    if (!en.ok || en.G == 0 || en.P == 0) return;              // no GT or no proposal: contributes nothing
    const int rows = en.P < P.maxR ? en.P : P.maxR;
    const int64_t cells = matrix_cells(en, P.maxR);
    const bool iou_lds = cells <= kIouLds;
    const int64_t s0 = slot_off[e], c0 = iou_off[e];
    if (s0 + en.G > n_slots || (!iou_lds && c0 + cells > n_iou_cells)) {      // past what the caller allocated
        if (tid == 0) *status = 2;
        return;
    }
    // ranks: logit descending, input order on ties
    for (int j = tid; j < en.P; j += kThreads) {
        const float s = prop_logits[en.p0 + j];
        int rank = 0;
        for (int q = 0; q < en.P; ++q) {
            const float ss = prop_logits[en.p0 + q];
            rank += (ss > s || (ss == s && q < j)) ? 1 : 0;
        }
        if (rank < rows) order[en.p0 + rank] = j;
    }
    // the non-crowd GTs in json order: XYXY = fp32(x), fp32(y), fp32(x + w), fp32(y + h), the sums in fp64
    if (wv == 0) {
        int cnt = 0;
        for (int gb = 0; gb < en.G; gb += 64) {
            const int g = gb + lane;
            const bool nc = g < en.G && gt_crowd[en.g0 + g] == 0;
            const unsigned long long m = __ballot(nc);
            if (nc) {
                const int k = cnt + __popcll(m & ((1ull << lane) - 1));
                const double* b = gt_boxes + 4 * (int64_t)(en.g0 + g);
                const float x0 = (float)b[0], y0 = (float)b[1], x1 = (float)(b[0] + b[2]), y1 = (float)(b[1] + b[3]);
                float* o = gtb + (s0 + k) * kGtStride;
                o[0] = x0;
                o[1] = y0;
                o[2] = x1;
                o[3] = y1;
                o[4] = (x1 - x0) * (y1 - y0);
                o[5] = (float)gt_area[en.g0 + g];
            }
            cnt += __popcll(m);
        }
        if (lane == 0) s_gnc = cnt;
    }
    __syncthreads();                                             // order / gtb in global memory: same block, workgroup scope suffices
    const int Gn = s_gnc;
    if (Gn == 0) return;
    float* iou = iou_lds ? s_iou : iou_ws + c0;
    for (int64_t q = tid; q < (int64_t)rows * Gn; q += kThreads) {
        const int r = (int)(q / Gn), g = (int)(q % Gn);
        int j = order[en.p0 + r];
        if ((unsigned)j >= (unsigned)en.P) j = 0;              // NaN logits leave ranks unassigned: stay inside the entry
        const float* pb = prop_boxes + 4 * (int64_t)(en.p0 + j);
        const float* gb = gtb + (s0 + g) * kGtStride;
        const float px0 = pb[0], py0 = pb[1], px1 = pb[2], py1 = pb[3];
        const float ap = (px1 - px0) * (py1 - py0);
        float iw = fminf(px1, gb[2]) - fmaxf(px0, gb[0]);
        float ih = fminf(py1, gb[3]) - fmaxf(py0, gb[1]);
        iw = iw > 0.0f ? iw : 0.0f;
        ih = ih > 0.0f ? ih : 0.0f;
        const float inter = iw * ih;
        iou[q] = inter > 0.0f ? inter / (ap + gb[4] - inter) : 0.0f;
    }
    __syncthreads();
    if (wv >= AL) return;
    // one wave per chain from here on: no block barrier below
    const int l = wv / P.A, a = wv % P.A;
    const int R = en.P < P.limit[l] ? en.P : P.limit[l];
    const float lo = P.lo[a], hi = P.hi[a];
    const bool col_lds = Gn <= kColLds;
    float* cmax = col_lds ? s_cmax[wv] : cmax_ws + (int64_t)wv * n_slots + s0;
    int32_t* carg = col_lds ? s_carg[wv] : carg_ws + (int64_t)wv * n_slots + s0;
    int nvalid = 0;
    for (int gb = 0; gb < Gn; gb += 64) {
        const int g = gb + lane;
        bool v = false;
        if (g < Gn) {
            const float a32 = gtb[(s0 + g) * kGtStride + 5];
            v = a32 >= lo && a32 <= hi;
        }
        nvalid += __popcll(__ballot(v));
        float best = -1.0f;
        int arg = 0;
        if (v) {
            for (int r = 0; r < R; ++r) {
                const float x = iou[(int64_t)r * Gn + g];
                if (x > best) {
                    best = x;
                    arg = r;
                }
            }
        }
        if (g < Gn) {
            cmax[g] = best;                                      // -1: retired (here: outside the area range)
            carg[g] = arg;
        }
    }
    if (lane == 0) {
        valid[(int64_t)e * AL + wv] = nvalid;
        if (nvalid > 0) atomicAdd(&num_pos[wv], (unsigned long long)nvalid);
    }
    if (nvalid == 0) return;
    uint32_t* out = keys + (int64_t)wv * Psort + s0;
    const int K = R < nvalid ? R : nvalid;
    uint32_t dead = 0;                                           // lane i: rows 32 i .. 32 i + 31 retired
    for (int j = 0; j < K; ++j) {
        float bv = -1.0f;
        int bg = 0x7fffffff;
        for (int gb = 0; gb < Gn; gb += 64) {
            const int g = gb + lane;
            if (g < Gn) {
                const float x = cmax[g];
                if (x > bv) {
                    bv = x;
                    bg = g;
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int og = __shfl_xor(bg, o, 64);
            if (ov > bv || (ov == bv && og < bg)) {
                bv = ov;
                bg = og;
            }
        }
        bg = __builtin_amdgcn_readfirstlane(bg);
        if (bg >= Gn) break;                                     // not reached: a live column exists while j < min(R, nvalid)
        int rb = 0;
        if (lane == (bg & 63)) rb = carg[bg];
        rb = __builtin_amdgcn_readfirstlane(__shfl(rb, bg & 63, 64));
        if (lane == 0) out[j] = __float_as_uint(bv);
        if (lane == (bg & 63)) cmax[bg] = -1.0f;
        if (lane == (rb >> 5)) dead |= 1u << (rb & 31);
        if (j + 1 == K) break;
        for (int gb = 0; gb < Gn; gb += 64) {
            const int g = gb + lane;
            const bool need = g < Gn && cmax[g] >= 0.0f && carg[g] == rb;
            if (__ballot(need) == 0) continue;
            float best = -1.0f;
            int arg = 0;
            for (int wd = 0; wd * 32 < R; ++wd) {
                uint32_t live = ~(uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl((int)dead, wd, 64));
                const int rem = R - wd * 32;
                if (rem < 32) live &= (1u << rem) - 1;
                while (live) {
                    const int r = wd * 32 + __ffs((int)live) - 1;
                    live &= live - 1;
                    if (need) {
                        const float x = iou[(int64_t)r * Gn + g];
                        if (x > best) {
                            best = x;
                            arg = r;
                        }
                    }
                }
            }
            if (need) {
                cmax[g] = best;
                carg[g] = arg;
            }
        }
    }
    for (int j = K + lane; j < nvalid; j += 64) out[j] = 0;     // +0.0f: GTs past the last proposal
}

struct u32_gt {
    __device__ __forceinline__ bool operator()(uint32_t a, uint32_t b) const { return a > b; }
};

__global__ void k_counts(Params P, const uint32_t* keys, int64_t Psort, int32_t n_slots, const unsigned long long* num_pos,
                         int64_t* counts) {
    const int c = blockIdx.x, t = threadIdx.x;
    if (t >= P.T) return;
    int64_t np = (int64_t)num_pos[c];
    if (np > n_slots) np = n_slots;
    const uint32_t* row = keys + (int64_t)c * Psort;
    const float thr = P.thr[t];
    int64_t lo = 0, hi = np;                                     // first index whose overlap is >= thr
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (__uint_as_float(row[mid]) >= thr) hi = mid;
        else lo = mid + 1;
    }
    counts[(int64_t)c * P.T + t] = np - lo;
}

}  // namespace

extern "C" int32_t ore_proposal_recall_lds_cells(void) { return kIouLds; }

extern "C" size_t ore_proposal_recall_workspace_bytes(int32_t n_entries, int32_t n_props, int32_t n_slots, int64_t n_iou_cells,
                                                      int32_t n_areas, int32_t n_limits) {
    if (n_entries < 0 || n_props < 0 || n_slots < 0 || n_iou_cells < 0 || n_areas <= 0 || n_areas > kMaxA || n_limits <= 0 ||
        n_limits > kMaxL || n_areas * n_limits > kMaxChains)
        return 0;
    return ws_layout(n_entries, n_props, n_slots, n_iou_cells, n_areas * n_limits).total;
}

extern "C" int ore_proposal_recall(const ore_proposal_recall_desc* d, void* stream) {
    ORE_CHECK_ARG(d != nullptr, "ore_proposal_recall: desc is NULL");
    const int32_t E = d->n_entries, I = d->n_images, N = d->n_props, G = d->n_gts, S = d->n_slots;
    ORE_CHECK_ARG(E >= 0 && I > 0 && N >= 0 && G >= 0 && S >= 0 && d->n_iou_cells >= 0,
                  "ore_proposal_recall: n_entries %d, n_images %d, n_props %d, n_gts %d, n_slots %d, n_iou_cells %lld", E, I, N, G, S,
                  (long long)d->n_iou_cells);
    ORE_CHECK_ARG(d->n_areas > 0 && d->n_areas <= kMaxA && d->n_limits > 0 && d->n_limits <= kMaxL &&
                      d->n_areas * d->n_limits <= kMaxChains && d->n_iou_thrs > 0 && d->n_iou_thrs <= kMaxT,
                  "ore_proposal_recall: A %d (<= %d), L %d (<= %d), A * L <= %d, T %d (<= %d)", d->n_areas, kMaxA, d->n_limits, kMaxL,
                  kMaxChains, d->n_iou_thrs, kMaxT);
    ORE_CHECK_ARG(d->area_rngs_host && d->limits_host && d->iou_thrs_host, "ore_proposal_recall: parameter arrays are NULL");
    ORE_CHECK_ARG(d->gt_off && (E == 0 || (d->entry_off && d->entry_image)) && (N == 0 || (d->prop_boxes && d->prop_logits)) &&
                      (G == 0 || (d->gt_boxes && d->gt_area && d->gt_crowd)) && d->num_pos && d->counts && d->status &&
                      (S == 0 || d->gt_overlaps),
                  "ore_proposal_recall: a required device pointer is NULL");
    const bool per_entry = d->entry_overlaps || d->entry_slot_off || d->entry_valid;
    ORE_CHECK_ARG(!per_entry || ((S == 0 || d->entry_overlaps) && d->entry_slot_off && d->entry_valid),
                  "ore_proposal_recall: the per-entry output needs entry_overlaps, entry_slot_off and entry_valid");
    Params P{};
    P.A = d->n_areas;
    P.L = d->n_limits;
    P.T = d->n_iou_thrs;
    for (int a = 0; a < P.A; ++a) {
        P.lo[a] = (float)d->area_rngs_host[2 * a];
        P.hi[a] = (float)d->area_rngs_host[2 * a + 1];
    }
    for (int l = 0; l < P.L; ++l) {
        P.limit[l] = d->limits_host[l];
        ORE_CHECK_ARG(P.limit[l] > 0 && P.limit[l] <= kMaxRows, "ore_proposal_recall: limit %d outside 1 .. %d", P.limit[l], kMaxRows);
        P.maxR = P.limit[l] > P.maxR ? P.limit[l] : P.maxR;
    }
    for (int t = 0; t < P.T; ++t) P.thr[t] = d->iou_thrs_host[t];
    const int AL = P.A * P.L;
    const Ws w = ws_layout(E, N, S, d->n_iou_cells, AL);
    ORE_CHECK_ARG(d->workspace && d->workspace_bytes >= w.total,
                  "ore_proposal_recall: workspace %zu bytes < %zu (ore_proposal_recall_workspace_bytes)", d->workspace_bytes, w.total);
    ORE_CHECK_ARG(w.P * AL < (1ll << 31), "ore_proposal_recall: n_slots %d too large", S);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)d->workspace;
    int32_t* slot_off = (int32_t*)(ws + w.slot_off);
    int64_t* iou_off = (int64_t*)(ws + w.iou_off);
    int32_t* valid = (int32_t*)(ws + w.valid);
    uint32_t* keys = (uint32_t*)(ws + w.keys);
    unsigned long long* num_pos = (unsigned long long*)d->num_pos;

    ORE_HIP(hipMemsetAsync(d->num_pos, 0, (size_t)AL * 8, s));
    ORE_HIP(hipMemsetAsync(d->status, 0, 4, s));
    ORE_HIP(hipMemsetAsync(keys, 0xff, (size_t)w.P * AL * 4, s));
    if (E > 0) ORE_HIP(hipMemsetAsync(valid, 0, (size_t)E * AL * 4, s));
    hipLaunchKernelGGL(k_entry_scan, dim3(1), dim3(1024), 0, s, d->entry_off, d->entry_image, d->gt_off, E, N, I, G, P.maxR, slot_off,
                       iou_off, d->status);
    if (E > 0 && S > 0) {
        hipLaunchKernelGGL(k_entry, dim3((unsigned)E), dim3(kThreads), 0, s, P, d->prop_boxes, d->prop_logits, d->entry_off, d->entry_image,
                           d->gt_boxes, d->gt_area, d->gt_crowd, d->gt_off, N, I, G, S, d->n_iou_cells, w.P, slot_off, iou_off,
                           (int32_t*)(ws + w.order), (float*)(ws + w.gtb), (float*)(ws + w.cmax), (int32_t*)(ws + w.carg),
                           (float*)(ws + w.iou), keys, valid, num_pos, d->status);
    }
    if (per_entry) {
        ORE_HIP(hipMemcpyAsync(d->entry_slot_off, slot_off, (size_t)(E + 1) * 4, hipMemcpyDeviceToDevice, s));
        if (E > 0) ORE_HIP(hipMemcpyAsync(d->entry_valid, valid, (size_t)E * AL * 4, hipMemcpyDeviceToDevice, s));
        if (S > 0)
            ORE_HIP(hipMemcpy2DAsync(d->entry_overlaps, (size_t)S * 4, keys, (size_t)w.P * 4, (size_t)S * 4, AL, hipMemcpyDeviceToDevice, s));
    }
    if (S > 1) bitonic_sort_rows<uint32_t, u32_gt>(keys, w.P, AL, s);
    if (S > 0) ORE_HIP(hipMemcpy2DAsync(d->gt_overlaps, (size_t)S * 4, keys, (size_t)w.P * 4, (size_t)S * 4, AL, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_counts, dim3((unsigned)AL), dim3(64), 0, s, P, keys, w.P, S, num_pos, d->counts);
    return ore_launch_status("ore_proposal_recall");
}
