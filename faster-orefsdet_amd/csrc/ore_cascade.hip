// The cascade of CustomCascadeROIHeads: K = len(MODEL.ROI_BOX_CASCADE_HEAD.IOUS) > 1 stages (ref:fewx/modeling/fsod/fsod_roi_heads.py:404-457,
// d2z:modeling/roi_heads/cascade_rcnn.py:163-307).  Eval: one launch per intermediate stage (ore_roi_cascade_refine_fwd), the
// last stage through the single-stage tail with the averaged score (ore_roi_predict_cascade_fwd); both run the predictor block of
// csrc/ore_roi_predict.h, so logits, deltas, softmax, apply_deltas and the clip are k_roi_predict_mb's and the C twin's, bit for bit.
// Training: the seam between two stages for a whole batch in one launch (ore_cascade_relabel_fwd).  Built without FMA contraction, as
// csrc/ore_roi.hip is (the Makefile's NOFMA list).
#include "ore_hip.h"
#include "ore_common.h"
#include "ore_roi_predict.h"
#include <math.h>

namespace {
using oreroi::PredP; using oreroi::CascP; using oreroi::roi_predict_mb_body; using oreroi::CASC_REFINE; using oreroi::CASC_LAST;

// the cascade's launches: the same block with the stage seam behind it (MODE = CASC_REFINE or CASC_LAST)
template <int RPB, int MODE>
__global__ __launch_bounds__(256) void k_roi_cascade_mb(PredP p, int* __restrict__ ok_out, CascP q) {
    roi_predict_mb_body<RPB, MODE>(p, ok_out, q);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The training seam between two cascade stages (d2z:modeling/roi_heads/cascade_rcnn.py:231-307: _create_proposals_from_boxes +
// _match_and_label_boxes) for B images x R rows in one launch, fixed shapes, no atomics: every row decodes its own box from the
// producing stage's (detached) deltas with k_roi_predict's arithmetic, clips it to ITS image, and walks the image's ground truth in
// index order (pairwise_iou; the first maximum wins, as torch.max does).  A row stays valid iff it was valid, its decoded box is finite
// and, after the clip, not empty (the reference removes empty boxes in training; a non-finite box would abort its Boxes.clip).
// Foreground (label 0) iff IoU >= the consuming stage's threshold; no ground truth: background, matched box zeros.  Rows that are
// not valid keep ore_sample_rois_fwd's padding contract: box (0, 0, 8, 8), label 1, valid 0, matched box zeros.
constexpr int RELABEL_MAXG = 256;
struct RelabelP {
    const float* boxes; const float* deltas; const unsigned char* valid; const float* img_hw; const float* gtp; const long long* gt_n;
    int R, G;
    float wx, wy, ww, wh, scale_clamp, thr;
    float* out_boxes; unsigned char* out_valid; long long* labels; float* gt;
};
__global__ __launch_bounds__(256) void k_cascade_relabel(RelabelP p) {
    __shared__ float gb[RELABEL_MAXG][4];
    __shared__ float ga[RELABEL_MAXG];
    const int b = blockIdx.x, t = threadIdx.x;
    const int gn = (int)max(min(p.gt_n[b], (long long)p.G), 0ll);
    const float* gtp = p.gtp + (size_t)b * p.G * 4;
    for (int g = t; g < gn; g += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(gtp + 4 * (size_t)g);
        gb[g][0] = v.x; gb[g][1] = v.y; gb[g][2] = v.z; gb[g][3] = v.w;
        ga[g] = (v.z - v.x) * (v.w - v.y);
    }
    __syncthreads();
    const float img_h = p.img_hw[2 * b], img_w = p.img_hw[2 * b + 1];
    for (int r = t; r < p.R; r += 256) {
        const size_t i = (size_t)b * p.R + r;
        f32x4 ob = {0.f, 0.f, 8.f, 8.f}, og = {0.f, 0.f, 0.f, 0.f};
        long long lab = 1;
        bool ok = p.valid[i] != 0;
        if (ok) {
            const f32x4 bx = *reinterpret_cast<const f32x4*>(p.boxes + 4 * i);
            const f32x4 d = *reinterpret_cast<const f32x4*>(p.deltas + 4 * i);
            const float w = bx.z - bx.x, hgt = bx.w - bx.y;
            const float cx = bx.x + 0.5f * w, cy = bx.y + 0.5f * hgt;
            const float dx = d.x / p.wx, dy = d.y / p.wy;
            const float dw = fminf(d.z / p.ww, p.scale_clamp), dh = fminf(d.w / p.wh, p.scale_clamp);
            const float pcx = dx * w + cx, pcy = dy * hgt + cy;
            const float pw = ore_expf(dw) * w, phh = ore_expf(dh) * hgt;
            f32x4 nb = f32x4{pcx - 0.5f * pw, pcy - 0.5f * phh, pcx + 0.5f * pw, pcy + 0.5f * phh};
            const bool finite = isfinite(nb.x) && isfinite(nb.y) && isfinite(nb.z) && isfinite(nb.w);
            nb.x = fminf(fmaxf(nb.x, 0.f), img_w); nb.y = fminf(fmaxf(nb.y, 0.f), img_h);
            nb.z = fminf(fmaxf(nb.z, 0.f), img_w); nb.w = fminf(fmaxf(nb.w, 0.f), img_h);
            ok = finite && (nb.z - nb.x) > 0.f && (nb.w - nb.y) > 0.f;
            if (ok) {
                ob = nb;
                const float ac = (nb.z - nb.x) * (nb.w - nb.y);
                float best = -1.0f;
                int bi = -1;
                for (int g = 0; g < gn; ++g) {
                    const float iw = fmaxf(fminf(gb[g][2], nb.z) - fmaxf(gb[g][0], nb.x), 0.f);
                    const float ih = fmaxf(fminf(gb[g][3], nb.w) - fmaxf(gb[g][1], nb.y), 0.f);
                    const float inter = iw * ih;
                    const float iou = inter > 0.f ? inter / (ga[g] + ac - inter) : 0.f;
                    if (iou > best) { best = iou; bi = g; }
                }
                if (bi >= 0) {
                    lab = best >= p.thr ? 0 : 1;
                    og = f32x4{gb[bi][0], gb[bi][1], gb[bi][2], gb[bi][3]};
                }
            }
        }
        *reinterpret_cast<f32x4*>(p.out_boxes + 4 * i) = ob;
        *reinterpret_cast<f32x4*>(p.gt + 4 * i) = og;
        p.labels[i] = lab;
        p.out_valid[i] = ok ? 1 : 0;
    }
}

}  // namespace

void oreroi::launch_cascade_last(const PredP& p, int* ok, const CascP& q, size_t lds, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (p.h_parts > 0) hipLaunchKernelGGL((k_roi_cascade_mb<8, CASC_LAST>), dim3(ceil_div(p.cap, 8)), dim3(256), lds, st, p, ok, q);
    else hipLaunchKernelGGL((k_roi_cascade_mb<64, CASC_LAST>), dim3(ceil_div(p.cap, 64)), dim3(256), lds, st, p, ok, q);
}

// ---- the cascade (K = len(ROI_BOX_CASCADE_HEAD.IOUS) > 1 stages): one intermediate stage, the last stage, the training seam
constexpr int FUSED_CAP = 512, FUSED_C = (60 * 1024 - 6 * 64 * 4) / (4 * 71);      // oreroi::fused_domain, for the messages
static bool cascade_domain(int32_t cap, int32_t C) { return oreroi::fused_domain(cap, C); }

extern "C" int ore_roi_cascade_refine_fwd(const float* h, int32_t C, int32_t h_parts, const float* h_bias, const float* cls_w,
                                          const float* cls_b, const float* box_w, const float* box_b, const float* boxes,
                                          const int32_t* n_dev, int32_t n_host, int32_t cap, const float* reg_weights4_host, float img_h,
                                          float img_w, float* next_boxes, float* score_sum, uint8_t* dead, int32_t accumulate, void* stream) {
    ORE_CHECK_ARG(h && cls_w && cls_b && box_w && box_b && boxes && reg_weights4_host && next_boxes && score_sum && dead,
                  "ore_roi_cascade_refine_fwd: null pointer");
    ORE_CHECK_ARG(cascade_domain(cap, C), "ore_roi_cascade_refine_fwd: an intermediate cascade stage covers 1 <= cap <= %d (got %d) and fc width "
                  "<= %d (got %d), the domain of the fused tail", FUSED_CAP, cap, FUSED_C, C);
    ORE_CHECK_ARG(h_parts >= 0 && (accumulate == 0 || accumulate == 1), "ore_roi_cascade_refine_fwd: h_parts=%d accumulate=%d", h_parts, accumulate);
    PredP p{};
    p.h = h; p.C = C; p.h_parts = h_parts; p.h_bias = h_bias; p.cls_w = cls_w; p.cls_b = cls_b; p.box_w = box_w; p.box_b = box_b;
    p.boxes = boxes; p.n_ptr = n_dev; p.n_host = n_host; p.cap = cap;
    p.wx = reg_weights4_host[0]; p.wy = reg_weights4_host[1]; p.ww = reg_weights4_host[2]; p.wh = reg_weights4_host[3];
    p.scale_clamp = logf(1000.0f / 16.0f);
    p.img_h = img_h; p.img_w = img_w;
    CascP q{score_sum, dead, next_boxes, accumulate, 1.0f};
    const size_t lds = ((size_t)64 * (C + 1) + 6 * 64) * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    if (h_parts > 0) hipLaunchKernelGGL((k_roi_cascade_mb<8, CASC_REFINE>), dim3(ceil_div(cap, 8)), dim3(256), lds, st, p, (int*)nullptr, q);
    else hipLaunchKernelGGL((k_roi_cascade_mb<64, CASC_REFINE>), dim3(ceil_div(cap, 64)), dim3(256), lds, st, p, (int*)nullptr, q);
    return ore_launch_status("k_roi_cascade_mb");
}

extern "C" int ore_roi_predict_cascade_fwd(const float* h, int32_t C, const float* cls_w, const float* cls_b, const float* box_w,
                                           const float* box_b, const float* boxes, const int32_t* n_dev, int32_t n_host, int32_t cap,
                                           const float* reg_weights4_host, float img_h, float img_w, float score_thresh, float nms_thresh,
                                           int32_t topk, float* det_boxes, float* det_scores, int64_t* det_src, int32_t* det_count,
                                           const float* post_dev, float* fin_boxes, float* fin_scores, int32_t* fin_count,
                                           int32_t* host_count, void* workspace, size_t workspace_bytes, void* stream,
                                           int32_t h_parts, const float* h_bias, const float* score_sum, const uint8_t* dead,
                                           int32_t n_stages) {
    ORE_CHECK_ARG(n_stages >= 1, "ore_roi_predict_cascade_fwd: n_stages=%d", n_stages);
    if (n_stages == 1) {
        ORE_CHECK_ARG(!score_sum && !dead, "ore_roi_predict_cascade_fwd: one stage has no earlier scores (score_sum and dead must be NULL)");
        return oreroi::roi_predict_post(h, C, h_parts, h_bias, cls_w, cls_b, box_w, box_b, boxes, n_dev, n_host, cap, reg_weights4_host, img_h,
                                        img_w, score_thresh, nms_thresh, topk, det_boxes, det_scores, det_src, det_count, post_dev, fin_boxes,
                                        fin_scores, fin_count, host_count, workspace, workspace_bytes, stream);
    }
    ORE_CHECK_ARG(score_sum && dead, "ore_roi_predict_cascade_fwd: %d stages need score_sum and dead of the stages before the last", n_stages);
    ORE_CHECK_ARG(cascade_domain(cap, C), "ore_roi_predict_cascade_fwd: the cascade tail (%d stages) covers 1 <= cap <= %d (got %d) and fc width "
                  "<= %d (got %d)", n_stages, FUSED_CAP, cap, FUSED_C, C);
    const CascP q{const_cast<float*>(score_sum), const_cast<uint8_t*>(dead), nullptr, 1, (float)(1.0 / (double)n_stages)};
    return oreroi::roi_predict_cascade(h, C, h_parts, h_bias, cls_w, cls_b, box_w, box_b, boxes, n_dev, n_host, cap, reg_weights4_host, img_h, img_w,
                            score_thresh, nms_thresh, topk, det_boxes, det_scores, det_src, det_count, post_dev, fin_boxes, fin_scores,
                            fin_count, host_count, workspace, workspace_bytes, stream, &q);
}

extern "C" int ore_cascade_relabel_fwd(const float* boxes, const float* deltas, const uint8_t* valid, const float* img_hw, const float* gtp,
                                       const int64_t* gt_n, int32_t B, int32_t R, int32_t G, const float* reg_weights4_host, float iou_thr,
                                       float* out_boxes, uint8_t* out_valid, int64_t* labels, float* gt, void* stream) {
    ORE_CHECK_ARG(boxes && deltas && valid && img_hw && (gtp || G == 0) && gt_n && reg_weights4_host && out_boxes && out_valid && labels && gt,
                  "ore_cascade_relabel_fwd: null pointer");
    ORE_CHECK_ARG(B >= 1 && B <= 65535 && R >= 1 && G >= 0 && G <= RELABEL_MAXG && (long long)B * R < (1ll << 28),
                  "ore_cascade_relabel_fwd: B=%d R=%d G=%d (0 <= G <= %d)", B, R, G, RELABEL_MAXG);
    RelabelP p{boxes, deltas, valid, img_hw, gtp, (const long long*)gt_n, R, G, reg_weights4_host[0], reg_weights4_host[1],
               reg_weights4_host[2], reg_weights4_host[3], logf(1000.0f / 16.0f), iou_thr, out_boxes, out_valid, (long long*)labels, gt};
    hipLaunchKernelGGL(k_cascade_relabel, dim3(B), dim3(256), 0, (hipStream_t)stream, p);
    return ore_launch_status("k_cascade_relabel");
}
