// The tail of an OSA identity block (the blocks j >= 2 of a stage of V-39 / V-57 / V-99-eSE; d2z:modeling/backbone/vovnet.py:310-332):
//   out = y * gate + x,   y the concat conv's output, gate the block's eSE gate, x the block's own input (the identity)
// in ONE launch: eSE product, residual add and the copy into the next block's concat buffer.  Two maps read, one written; NHWC fp32,
// 16-byte vector accesses, no atomics, nothing crosses blocks: the result does not depend on scheduling.
#include "ore_common.h"
#include "ore_ese.h"
#include <stdlib.h>
#include <algorithm>

namespace {

// one rounding per element where an identity is added (fmaf), the plain product where there is none
__device__ __forceinline__ f32x4 gate_add(f32x4 y, f32x4 g, f32x4 x) {
    return f32x4{fmaf(y.x, g.x, x.x), fmaf(y.y, g.y, x.y), fmaf(y.z, g.z, x.z), fmaf(y.w, g.w, x.w)};
}

// One image.  Block (cg, pb) computes the sixteen gates of channel group cg from the concat conv's fused column sums like
// k_ese_gate_fused -- every pb redundantly, the same bits in each -- and runs exactly those sixteen channels over its share of the
// rows, so no launch waits for another and nothing is shared between blocks (the scheme of k_ese_gate_pool).  The pb == 0 blocks
// publish gate[].  The loads of a thread's FIRST row are issued before the block reduces the column sums and runs its fc rows: they
// share a memory round trip with the partial-sum loads and are consumed after the gate.  x == nullptr: out = y * gate (the tail of
// block 1 when a block 2 follows).
__global__ __launch_bounds__(ESE_T) void k_ese_gate_residual(const float* __restrict__ part, int P, int HW, int C, const float* __restrict__ fw,
                                                             const float* __restrict__ fb, float* __restrict__ gate,
                                                             const float* __restrict__ y, int y_ld, int y_coff,
                                                             const float* __restrict__ x, int x_ld, int x_coff,
                                                             float* __restrict__ out, int out_ld, int out_coff) {
    __shared__ EseSm sm;
    const int pb = blockIdx.y;
    const int per = (HW + gridDim.y - 1) / gridDim.y;
    const int r1 = min((pb + 1) * per, HW);
    const int j = threadIdx.x & 3, c = blockIdx.x * 16 + j * 4;
    const int r0 = pb * per + (threadIdx.x >> 2);
    const bool first = c < C && r0 < r1;
    f32x4 yv = {0.f, 0.f, 0.f, 0.f}, xv = {0.f, 0.f, 0.f, 0.f};
    if (first) {
        yv = ld4(y + (size_t)r0 * y_ld + y_coff + c);
        if (x) xv = ld4(x + (size_t)r0 * x_ld + x_coff + c);
    }
    ese_gate16(sm, part, P, HW, C, fw, fb, gate, 0, pb == 0);
    if (c >= C) return;
    const f32x4 g4 = {sm.g16[j * 4], sm.g16[j * 4 + 1], sm.g16[j * 4 + 2], sm.g16[j * 4 + 3]};
    if (first) st4(out + (size_t)r0 * out_ld + out_coff + c, x ? gate_add(yv, g4, xv) : yv * g4);
    for (int r = r0 + ESE_T / 4; r < r1; r += ESE_T / 4) {
        yv = ld4(y + (size_t)r * y_ld + y_coff + c);
        if (x) {
            xv = ld4(x + (size_t)r * x_ld + x_coff + c);
            st4(out + (size_t)r * out_ld + out_coff + c, gate_add(yv, g4, xv));
        } else
            st4(out + (size_t)r * out_ld + out_coff + c, yv * g4);
    }
}

// B images, the gates given ([B][C]): thread = (row, 4 channels), consecutive threads along the channels of a row
__global__ __launch_bounds__(256) void k_scale_residual(const float* __restrict__ y, int y_ld, int y_coff, const float* __restrict__ gate,
                                                        const float* __restrict__ x, int x_ld, int x_coff, int total, int rows_per_image,
                                                        int C4, float* __restrict__ out, int out_ld, int out_coff) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c4 = idx % C4, row = idx / C4, b = row / rows_per_image;
    const f32x4 yv = ld4(y + (size_t)row * y_ld + y_coff + c4 * 4);
    const f32x4 g = ld4(gate + ((size_t)b * C4 + c4) * 4);
    float* o = out + (size_t)row * out_ld + out_coff + c4 * 4;
    if (x) st4(o, gate_add(yv, g, ld4(x + (size_t)row * x_ld + x_coff + c4 * 4)));
    else st4(o, yv * g);
}

// Two channel slices that share memory must never meet: either the two spans are apart, or the rows coincide (same row stride) and the
// slices lie side by side in every row.
bool slices_apart(const float* a, int a_ld, int a_coff, const float* b, int b_ld, int b_coff, int64_t rows, int C) {
    const float* a0 = a + a_coff; const float* a1 = a0 + (rows - 1) * a_ld + C;
    const float* b0 = b + b_coff; const float* b1 = b0 + (rows - 1) * b_ld + C;
    if (a1 <= b0 || b1 <= a0) return true;
    if (a_ld != b_ld) return false;
    const int64_t d = (((b0 - a0) % a_ld) + a_ld) % a_ld;
    return d >= C && d <= a_ld - C;
}

int check_maps(const char* who, const float* y, int y_ld, int y_coff, const float* x, int x_ld, int x_coff, const float* out, int out_ld,
               int out_coff, int64_t rows, int C) {
    ORE_CHECK_ARG(y && out, "%s: null pointer", who);
    ORE_CHECK_ARG(rows > 0 && C > 0 && C % 4 == 0, "%s: %lld rows of %d channels (a multiple of 4)", who, (long long)rows, C);
    ORE_CHECK_ARG(y_ld % 4 == 0 && y_coff % 4 == 0 && out_ld % 4 == 0 && out_coff % 4 == 0 && (!x || (x_ld % 4 == 0 && x_coff % 4 == 0)),
                  "%s: row strides and channel offsets must be multiples of 4", who);
    ORE_CHECK_ARG(((uintptr_t)y | (uintptr_t)out | (uintptr_t)x) % 16 == 0, "%s: y, x and out must be 16-byte aligned", who);
    ORE_CHECK_ARG(y_coff >= 0 && y_coff + C <= y_ld && out_coff >= 0 && out_coff + C <= out_ld && (!x || (x_coff >= 0 && x_coff + C <= x_ld)),
                  "%s: a channel slice leaves its row", who);
    ORE_CHECK_ARG(slices_apart(y, y_ld, y_coff, out, out_ld, out_coff, rows, C), "%s: out overlaps y", who);
    ORE_CHECK_ARG(!x || slices_apart(x, x_ld, x_coff, out, out_ld, out_coff, rows, C), "%s: out overlaps x", who);
    return ORE_OK;
}

}  // namespace

extern "C" int ore_ese_gate_residual_fwd(const float* part, int32_t P, int32_t HW, int32_t C, const float* fc_w, const float* fc_b,
                                         float* gate, const float* y, int32_t y_ld, int32_t y_coff, const float* x, int32_t x_ld,
                                         int32_t x_coff, float* out, int32_t out_ld, int32_t out_coff, void* stream) {
    ORE_CHECK_ARG(part && fc_w && fc_b && gate, "ore_ese_gate_residual_fwd: null pointer");
    ORE_CHECK_ARG(P > 0 && HW > 0 && C > 0 && C <= 4096, "ore_ese_gate_residual_fwd: P %d, HW %d, C %d (at most 4096)", P, HW, C);
    int rc = check_maps("ore_ese_gate_residual_fwd", y, y_ld, y_coff, x, x_ld, x_coff, out, out_ld, out_coff, HW, C);
    if (rc) return rc;
    ORE_CHECK_ARG(((uintptr_t)part | (uintptr_t)gate) % 16 == 0, "ore_ese_gate_residual_fwd: part and gate must be 16-byte aligned");
    const int gx = ceil_div(C, 16);
    static int tb = 0;                                                // blocks aimed at (env ORE_GATE_RESIDUAL_BLOCKS for A/B)
    if (!tb) { const char* e = getenv("ORE_GATE_RESIDUAL_BLOCKS"); tb = e ? atoi(e) : 224; if (tb < 8) tb = 224; }
    int gy = ceil_div(tb, gx);                                        // ~ one block per CU, at least 64 rows per block
    gy = std::max(1, std::min(gy, ceil_div(HW, 64)));
    hipLaunchKernelGGL(k_ese_gate_residual, dim3(gx, gy), dim3(ESE_T), 0, (hipStream_t)stream, part, P, HW, C, fc_w, fc_b, gate, y, y_ld,
                       y_coff, x, x_ld, x_coff, out, out_ld, out_coff);
    return ore_launch_status("k_ese_gate_residual");
}

extern "C" int ore_scale_residual_fwd(const float* y, int32_t y_ld, int32_t y_coff, const float* gate_bc, const float* x, int32_t x_ld,
                                      int32_t x_coff, int32_t B, int32_t rows_per_image, int32_t C, float* out, int32_t out_ld,
                                      int32_t out_coff, void* stream) {
    ORE_CHECK_ARG(gate_bc && B > 0 && rows_per_image > 0, "ore_scale_residual_fwd: null gate, or no rows");
    const int64_t rows = (int64_t)B * rows_per_image;
    int rc = check_maps("ore_scale_residual_fwd", y, y_ld, y_coff, x, x_ld, x_coff, out, out_ld, out_coff, rows, C);
    if (rc) return rc;
    ORE_CHECK_ARG((uintptr_t)gate_bc % 16 == 0, "ore_scale_residual_fwd: gate must be 16-byte aligned");
    ORE_CHECK_ARG(rows * (C / 4) <= 0x7fffff00, "ore_scale_residual_fwd: %lld rows of %d channels exceed one launch", (long long)rows, C);
    const int total = (int)(rows * (C / 4));
    hipLaunchKernelGGL(k_scale_residual, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, y, y_ld, y_coff, gate_bc, x, x_ld,
                       x_coff, total, rows_per_image, C / 4, out, out_ld, out_coff);
    return ore_launch_status("k_scale_residual");
}
