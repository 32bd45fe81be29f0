// Storage-tagged launchers of the non-conv layer ops (csrc/ore_misc.hip): ONE launcher per op for both activation storages (ROIAlign
// forward has the same shape: oreroi::roi_align_fwd, ore_common.h).  Activation pointers are untyped; `bf16` says what they point at (false: fp32, true: bf16, the
// ORE_CONV_BF16S engines).  A launcher holds the argument checks, the geometry and the launch and picks the kernel's template instance;
// the fp32 and `_bf16` C entries of include/ore_hip.h forward to it, the engine calls it with its own storage.  Error texts name the C
// entry of the storage.
#pragma once
#include "ore_common.h"

// MaxPool2d(3, 2, ceil_mode=True): output size of an axis of n elements
static inline int ore_pool_out(int n) { int o = (n - 3 + 1) / 2 + 1; if (n < 3) o = 1; if ((o - 1) * 2 >= n) --o; return o < 1 ? 1 : o; }

namespace oremisc {
int stem1(const void* img, int32_t img_is_u8, int32_t B, int32_t H, int32_t W, int32_t Hp, int32_t Wp, const float* mean3, const float* std3,
          const float* w_oihw, const float* scale, const float* shift, int32_t Cout, void* out, int32_t out_ld, int32_t out_coff, void* stream,
          bool bf16);
int maxpool3x3s2(const void* in, int32_t in_ld, int32_t in_coff, int32_t B, int32_t H, int32_t W, int32_t C, const float* in_mul, void* out,
                 int32_t out_ld, int32_t out_coff, void* stream, bool bf16);
// gate + gate-scaled consumer weight (optional; bf16 storage: a bf16 tensor) + max-pool of x * gate, one launch (one image)
int ese_gate_pool(const float* part, int32_t P, int32_t HW, int32_t C, const float* fc_w, const float* fc_b, float* gate, const float* w_packed,
                  int32_t w_rows, void* w_scaled, const void* x, int32_t x_ld, int32_t x_coff, int32_t H, int32_t W, void* out, int32_t out_ld,
                  int32_t out_coff, void* stream, bool bf16);
int ese_gate_scaled_weight(const float* part, int32_t P, int32_t HW, int32_t C, const float* fc_w, const float* fc_b, float* gate, float* mean_ws,
                           const float* w_packed, int32_t w_rows, void* w_scaled, void* stream, bool bf16);
int correlation_levels(const void* q, int32_t q_ld, int32_t q_coff, int32_t B, int32_t n_levels, const int32_t* H, const int32_t* W, int32_t C,
                       const float* k11, const float* k13, const float* k31, void* out, int32_t out_ld, int32_t out_coff, void* stream, bool bf16);
int gn_affine_levels(const void* x, int32_t ld, int32_t coff, int32_t B, int32_t n_levels, const int32_t* HW, int32_t C, int32_t groups, float eps,
                     const float* gamma, const float* beta, float* mul, float* add, float* workspace, void* stream, bool bf16);
int head_pred_gn(const void* tower, int32_t ld, int32_t B, int32_t n_levels, const int32_t* H, const int32_t* W, int32_t groups, float eps,
                 const float* gamma, const float* beta, const float* w_packed16, const float* scale, const float* shift, int32_t ep_stride,
                 float* out, int32_t out_ld, float* workspace, void* stream, bool bf16);
// N-way fan-out correlation and the query copy in front of it (fp32 storage only)
int correlation_classes(const float* q, int32_t q_ld, int32_t q_coff, int32_t n_levels, const int32_t* H, const int32_t* W, int32_t C,
                        int32_t K, const float* k11s, const float* k13s, const float* k31s, float* out, int32_t out_ld, void* stream);
int copy_cols(const float* src, int32_t src_ld, int32_t src_coff, int32_t rows, int32_t C, float* dst, int32_t dst_ld, void* stream);
}
