// Internal helpers shared by the HIP translation units of libore_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "ore_hip.h"

void ore_set_error(const char* fmt, ...);
void ore_note_wino(int v);
int ore_last_wino(void);                // 1: this thread's last ore_conv2d_fwd / _levels_fwd call ran on the Winograd kernel
void ore_note_launch(int code, int split);   // the launcher (ORE_LAUNCH_*) and split-K of that call (ore_conv_last_launch)
void ore_flop_count_add(double flops);   // csrc/ore_util.cpp: algorithmic FLOPs of the per-op conv entry points (ore_flop_counter_read)

#define ORE_CHECK_ARG(cond, ...)              \
    do {                                      \
        if (!(cond)) {                        \
            ore_set_error(__VA_ARGS__);       \
            return ORE_EINVAL;                \
        }                                     \
    } while (0)

#define ORE_HIP(call)                                                                   \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess) {                                                         \
            ore_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            return ORE_EHIP;                                                            \
        }                                                                               \
    } while (0)

static inline int ore_launch_status(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        ore_set_error("launch %s -> %s", what, hipGetErrorString(e));
        return ORE_EHIP;
    }
    return ORE_OK;
}

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline int round_up(int a, int b) { return ceil_div(a, b) * b; }

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// 4 fp32 -> 4 bf16 (round to nearest even; two v_cvt_pk_bf16_f32 on gfx950), packed as the 16x16x16 bf16 MFMA operand
__device__ __forceinline__ s16x4 to_bf16x4(f32x4 v) {
    const bf16x2_t lo = __builtin_convertvector(f32x2{v.x, v.y}, bf16x2_t), hi = __builtin_convertvector(f32x2{v.z, v.w}, bf16x2_t);
    const u32x2 u = {__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi)};
    return __builtin_bit_cast(s16x4, u);
}

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
// 4 bf16 (packed as s16x4) -> 4 fp32, exact
__device__ __forceinline__ f32x4 from_bf16x4(s16x4 h) {
    const u32x2 u = __builtin_bit_cast(u32x2, h);
    return f32x4{__builtin_bit_cast(float, u.x << 16), __builtin_bit_cast(float, u.x & 0xffff0000u),
                 __builtin_bit_cast(float, u.y << 16), __builtin_bit_cast(float, u.y & 0xffff0000u)};
}
__device__ __forceinline__ float bf16_bits_to_f32(unsigned short h) { return __builtin_bit_cast(float, (unsigned)h << 16); }
// storage-type helpers for the kernels that exist for fp32 and bf16 tensors (T = float or ore_bf16_t)
struct ore_bf16_t { unsigned short v; };
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 ld4(const ore_bf16_t* p) { return from_bf16x4(*reinterpret_cast<const s16x4*>(p)); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ void st4(ore_bf16_t* p, f32x4 v) { *reinterpret_cast<s16x4*>(p) = to_bf16x4(v); }
__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const ore_bf16_t* p) { return bf16_bits_to_f32(p->v); }

// a raw buffer over [base, base + bytes): stride 0, num_records = bytes, so the range check is on the byte offset (flags word 0x00020000:
// 32-bit data format, nothing else)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}

// expf of the bit-exact twins (ore_detect.hip, ore_roi.hip and their CPU references): a fixed sequence of fmaf / single IEEE operations,
// the same on both sides, instead of whatever the math library of either side does.  Those files are compiled with -ffp-contract=off.
__device__ __forceinline__ float ore_expf(float x) {
    if (x > 88.0f) x = 88.0f;
    if (x < -87.0f) x = -87.0f;
    const float n = rintf(x * 1.44269504088896341f);
    float r = fmaf(n, -0.693359375f, x);
    r = fmaf(n, 2.12194440e-4f, r);
    float p = 1.9875691500e-4f;
    p = fmaf(p, r, 1.3981999507e-3f);
    p = fmaf(p, r, 8.3334519073e-3f);
    p = fmaf(p, r, 4.1665795894e-2f);
    p = fmaf(p, r, 1.6666665459e-1f);
    p = fmaf(p, r, 5.0000001201e-1f);
    const float e = fmaf(p, r * r, r) + 1.0f;
    const int ni = (int)n;
    return e * __uint_as_float((unsigned)(ni + 127) << 23);
}

// the sigmoid the proposal decode thresholds with (ore_detect.hip) and the heat maps show (ore_heatmap.hip; ore_sigmoid_host on the host)
__device__ __forceinline__ float ore_sigmoid(float x) { return 1.0f / (1.0f + ore_expf(-x)); }

namespace oreroi {
// ore_roi_predict_post_fwd with the fc1 rows still in K-split partial sums (csrc/ore_roi.hip; h_parts = 0: as the C-ABI entry)
int roi_predict_post(const float* h, int32_t C, int32_t h_parts, const float* h_bias, const float* cls_w, const float* cls_b,
                     const float* box_w, const float* box_b, const float* boxes, const int32_t* n_dev, int32_t n_host, int32_t cap,
                     const float* reg_weights4_host, float img_h, float img_w, float score_thresh, float nms_thresh,
                     int32_t topk, float* det_boxes, float* det_scores, int64_t* det_src, int32_t* det_count,
                     const float* post_dev, float* fin_boxes, float* fin_scores, int32_t* fin_count,
                     int32_t* host_count, void* workspace, size_t workspace_bytes, void* stream);
// ROIAlign forward for both feature storages (bf16: the maps are bf16 tensors): ore_roi_align_fwd / _bf16_fwd with box_image = null,
// ore_roi_align_batched_fwd with box_image [n_host] (csrc/ore_roi.hip)
int roi_align_fwd(const void* const* feat, const int32_t* ld, const int32_t* coff, const int32_t* H, const int32_t* W, const float* scales_host,
                  int32_t n_levels, int32_t min_level, int32_t C, int32_t pooled, const float* boxes, const int32_t* n_dev, int32_t n_host,
                  int32_t cap, float* out, void* stream, const int32_t* box_image, bool bf16);
// N-way pass: merge of the K per-class detection lists (det_boxes / det_scores / det_count of class slot k at k * cap rows / k * 4 words)
// into one list -- score descending, ties by class slot, then by row -- cut at topk, then detector_postprocess into fin_* and the
// caller's record (csrc/ore_roi.hip, k_roi_merge_classes).  class_ids [K] int64 device.
int roi_merge_classes(const float* det_boxes, const float* det_scores, const int32_t* det_count, int32_t K, int32_t cap,
                      const int64_t* class_ids, int32_t topk, const float* post_dev, float* fin_boxes, float* fin_scores,
                      int64_t* fin_classes, int32_t* fin_count, int32_t* host_count, void* stream);
// where the per-ROI rows of the predictor live inside that workspace (read-back for tests: ore_engine_buffer "roi_raw_*")
struct PredictWs { size_t raw_boxes, c_boxes, raw_scores, c_scores, c_src, ok, keep, nms; };
inline PredictWs predict_ws_layout(int32_t cap) {
    const size_t c = (size_t)(cap > 0 ? cap : 1);
    PredictWs w{};
    size_t o = 256;                                   // [0, 256): c_count, n_keep
    w.raw_boxes = o; o += c * 16;
    w.c_boxes = o; o += c * 16;
    w.raw_scores = o; o += c * 4;
    w.c_scores = o; o += c * 4;
    w.c_src = o; o += c * 4;
    w.ok = o; o += c * 4;
    w.keep = o; o += c * 8;
    w.nms = (o + 255) & ~(size_t)255;
    return w;
}
}
