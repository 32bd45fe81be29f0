// The second stage's predictor block, shared by the single-stage tail (csrc/ore_roi.hip: k_roi_predict_mb) and the cascade
// (csrc/ore_cascade.hip: k_roi_cascade_mb): its parameters, the block itself, and what the two units call in each other.
#pragma once
#include "ore_common.h"

namespace oreroi {
struct PredP {
    const float* h; int C;                       // [cap][C] after fc1+ReLU, or (h_parts > 0) the raw K-split partial sums [h_parts][cap][C]
    int h_parts; const float* h_bias;            // h_parts > 0: row = ReLU(bias + sum_z h[z]) added in z order (oreconv::conv_gd_splitk)
    const float* cls_w; const float* cls_b;      // [K+1][C], [K+1]  (K = 1 foreground class)
    const float* box_w; const float* box_b;      // [4][C], [4]
    const float* boxes; const int* n_ptr; int n_host; int cap;
    float wx, wy, ww, wh, scale_clamp;
    float img_h, img_w, score_thresh;
    float* raw_boxes; float* raw_scores;         // [cap] decoded, clipped (before the filter)
    float* c_boxes; float* c_scores; int* c_src; int* c_count;   // compacted (filter_mask order)
};

// The cascade's two forms of the same block (CustomCascadeROIHeads with K = len(IOUS) > 1 stages):
//   CASC_REFINE  an intermediate stage: no filter; the decoded, clipped box is the next stage's proposal (next_boxes), the foreground
//                probability is written (accumulate = 0) or added (1) into score_sum, and a row whose unclipped box or score is not
//                finite is marked in the sticky `dead` byte (next box (0,0,0,0), score_sum 0): the reference's Boxes.clip would abort there,
//                here the row leaves the result at the end.
//   CASC_LAST    the last stage: the candidate score is (score_sum + s_last) * inv_k, dead rows fail the filter; the rest as CASC_NONE.
enum { CASC_NONE = 0, CASC_REFINE = 1, CASC_LAST = 2 };
struct CascP {
    float* score_sum; unsigned char* dead; float* next_boxes; int accumulate; float inv_k;
};

template <int RPB, int MODE>
__device__ __forceinline__ void roi_predict_mb_body(const PredP& p, int* __restrict__ ok_out, const CascP& q) {
    extern __shared__ float hs[];                 // [RPB][C+1] rows, then dots [6][64]
    const int C = p.C, LDH = C + 1;
    float* dots = hs + RPB * LDH;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r0 = blockIdx.x * RPB;
    if (p.h_parts > 0) {
        // four elements per thread and sixteen slices per step: 64 independent loads in flight (a plain z loop is one dependent L2 round
        // trip per slice and element: 69 us for 32 slices); every element still adds its slices in the order z = 0, 1, 2, ...
        // The rows are summed for every row of the block up to the CAPACITY, before the device-side count is looked at: the count is one
        // more dependent round trip in front of these loads otherwise, and the slices hold cap rows each (rows beyond the count are
        // summed and never used).
        const size_t zs = (size_t)p.cap * C;
        const int ne = max(min(RPB, p.cap - r0), 0) * C;
        for (int i0 = tid; i0 < ne; i0 += 256 * 4) {
            float v[4];
            const float* src[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = min(i0 + 256 * j, ne - 1);
                v[j] = p.h_bias ? p.h_bias[i % C] : 0.0f;
                src[j] = p.h + (size_t)r0 * C + i;
            }
            for (int z0 = 0; z0 < p.h_parts; z0 += 16) {
                float t[16][4];
#pragma unroll
                for (int k = 0; k < 16; ++k)
#pragma unroll
                    for (int j = 0; j < 4; ++j) t[k][j] = z0 + k < p.h_parts ? src[j][(size_t)(z0 + k) * zs] : 0.0f;
#pragma unroll
                for (int k = 0; k < 16; ++k)
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] += t[k][j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = i0 + 256 * j;
                if (i < ne) hs[(i / C) * LDH + (i % C)] = fmaxf(v[j], 0.0f);
            }
        }
    }
    const int n = min(p.n_ptr ? *p.n_ptr : p.n_host, p.cap);
    if (r0 >= n) {                                // rows beyond the count: flag them out (the tail reads ok[0..cap))
        if (MODE != CASC_REFINE && tid < RPB && r0 + tid < p.cap) ok_out[r0 + tid] = 0;
        return;
    }
    const int rows = min(RPB, n - r0);
    if (p.h_parts <= 0) {
        for (int i = tid; i < rows * C; i += 256) hs[(i / C) * LDH + (i % C)] = p.h[(size_t)r0 * C + i];
    }
    __syncthreads();
    if (wave < 3 && lane < rows) {
        // the weight index is wave-uniform: the compiler fetches the rows through the scalar cache (s_load), the LDS port only
        // carries this lane's fc1 row (stride C+1: conflict-free)
        const float* h = hs + lane * LDH;
        const float* __restrict__ w0 = wave == 0 ? p.cls_w : p.box_w + (size_t)(2 * wave - 2) * C;
        const float* __restrict__ w1 = w0 + C;
        float a0 = wave == 0 ? p.cls_b[0] : p.box_b[2 * wave - 2];
        float a1 = wave == 0 ? p.cls_b[1] : p.box_b[2 * wave - 1];
#pragma unroll 8
        for (int c = 0; c < C; ++c) {
            const float v = h[c];
            a0 = fmaf(w0[c], v, a0);
            a1 = fmaf(w1[c], v, a1);
        }
        dots[(2 * wave) * 64 + lane] = a0;
        dots[(2 * wave + 1) * 64 + lane] = a1;
    }
    __syncthreads();
    if (wave == 0 && lane < RPB && r0 + lane < p.cap) {
        const int r = r0 + lane;
        int ok = 0;
        if (lane < rows) {
            const float l0 = dots[lane], l1 = dots[64 + lane];
            const float d0 = dots[128 + lane], d1 = dots[192 + lane], d2 = dots[256 + lane], d3 = dots[320 + lane];
            const float m = fmaxf(l0, l1);
            const float e0 = ore_expf(l0 - m), e1 = ore_expf(l1 - m);
            float score = e0 / (e0 + e1);
            const f32x4 b = *reinterpret_cast<const f32x4*>(p.boxes + (size_t)r * 4);
            const float w = b.z - b.x, hgt = b.w - b.y;
            const float cx = b.x + 0.5f * w, cy = b.y + 0.5f * hgt;
            const float dx = d0 / p.wx, dy = d1 / p.wy;
            const float dw = fminf(d2 / p.ww, p.scale_clamp), dh = fminf(d3 / p.wh, p.scale_clamp);
            const float pcx = dx * w + cx, pcy = dy * hgt + cy;
            const float pw = ore_expf(dw) * w, phh = ore_expf(dh) * hgt;
            f32x4 ob = f32x4{pcx - 0.5f * pw, pcy - 0.5f * phh, pcx + 0.5f * pw, pcy + 0.5f * phh};
            bool finite = isfinite(ob.x) && isfinite(ob.y) && isfinite(ob.z) && isfinite(ob.w) && isfinite(score);
            ob.x = fminf(fmaxf(ob.x, 0.f), p.img_w); ob.y = fminf(fmaxf(ob.y, 0.f), p.img_h);
            ob.z = fminf(fmaxf(ob.z, 0.f), p.img_w); ob.w = fminf(fmaxf(ob.w, 0.f), p.img_h);
            if (MODE == CASC_REFINE) {
                const bool dead = !finite || (q.accumulate && q.dead[r] != 0);
                const float sum = q.accumulate ? q.score_sum[r] + score : score;      // fp32 sum in stage order
                *reinterpret_cast<f32x4*>(q.next_boxes + (size_t)r * 4) = dead ? f32x4{0.f, 0.f, 0.f, 0.f} : ob;
                q.score_sum[r] = dead ? 0.f : sum;
                q.dead[r] = dead ? 1 : 0;
            } else {
                if (MODE == CASC_LAST) {
                    score = (q.score_sum[r] + score) * q.inv_k;
                    finite = finite && q.dead[r] == 0;
                }
                *reinterpret_cast<f32x4*>(p.raw_boxes + (size_t)r * 4) = ob;
                p.raw_scores[r] = score;
                ok = (finite && score > p.score_thresh) ? 1 : 0;
            }
        }
        if (MODE != CASC_REFINE) ok_out[r] = ok;
    }
}

// csrc/ore_roi.hip: the domain of the fused tail (cap <= ROI_FUSED_CAP, the fc width its LDS rows allow), and roi_predict_post with
// the cascade's last-stage parameters (q = NULL: the single stage)
bool fused_domain(int32_t cap, int32_t C);
int roi_predict_cascade(const float* h, int32_t C, int32_t h_parts, const float* h_bias, const float* cls_w, const float* cls_b,
                        const float* box_w, const float* box_b, const float* boxes, const int32_t* n_dev, int32_t n_host, int32_t cap,
                        const float* reg_weights4_host, float img_h, float img_w, float score_thresh, float nms_thresh,
                        int32_t topk, float* det_boxes, float* det_scores, int64_t* det_src, int32_t* det_count,
                        const float* post_dev, float* fin_boxes, float* fin_scores, int32_t* fin_count,
                        int32_t* host_count, void* workspace, size_t workspace_bytes, void* stream, const CascP* q);
// csrc/ore_cascade.hip: the predictor block of the LAST cascade stage (k_roi_cascade_mb<8 | 64, CASC_LAST>, 8 rows per block when
// p.h_parts > 0) in front of k_roi_tail; the launch status is read by the caller
void launch_cascade_last(const PredP& p, int* ok, const CascP& q, size_t lds, void* stream);
}  // namespace oreroi
