// The eSE gate of one block of sixteen channels, shared by the gate kernels of ore_misc.hip and the identity-block tail of
// ore_osa_residual.hip: one text, so every launch that derives a gate from the concat conv's column sums gets the same bits.
#pragma once
#include "ore_common.h"

// gate = relu6(fc(mean) + 3) / 6 straight from the partial column sums.  Every block (16 waves, one output channel each) first reduces
// part[b][0..P)[C] to the mean vector in LDS -- redundantly, in the same fixed order in every block, so all blocks hold the same bits
// and nothing crosses blocks -- while its fc weight row is already on its way to registers; then one wave per output (coalesced row,
// shuffle reduction).
constexpr int ESE_T = 1024, ESE_FP = 8;
struct EseSm {
    __attribute__((aligned(16))) float red[4096];      // [NSL][C], NSL * C <= 4096
    __attribute__((aligned(16))) float mean_s[4096];
    float g16[16];
};
// the block's sixteen gates (channels 16 blockIdx.x ..) of image b -> sm.g16 and gate[]; ends with a barrier
__device__ __forceinline__ void ese_gate16(EseSm& sm, const float* __restrict__ part, int P, int HW, int C, const float* __restrict__ fw,
                                           const float* __restrict__ fb, float* __restrict__ gate, int b, bool write_gate) {
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int o = blockIdx.x * 16 + wave;
    float fwv[ESE_FP];                                           // the first 512 weights of this wave's row: in flight under the reduction
#pragma unroll
    for (int j = 0; j < ESE_FP; ++j) {
        const int k = lane + 64 * j;
        fwv[j] = (o < C && k < C) ? fw[(size_t)o * C + k] : 0.f;
    }
    const int Q4 = C >> 2, NSL = ESE_T / Q4;                     // C <= 4096: NSL >= 1
    {
        const int q = tid % Q4, sl = tid / Q4;
        if (sl < NSL) {
            const float* pb = part + (size_t)b * P * C + q * 4;
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
            int p = sl;
            for (; p + 7 * NSL < P; p += 8 * NSL) {              // 8 independent loads in flight, summed in a fixed order
                f32x4 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const f32x4*>(pb + (size_t)(p + u * NSL) * C);
#pragma unroll
                for (int u = 0; u < 8; ++u) a += v[u];
            }
            for (; p < P; p += NSL) a += *reinterpret_cast<const f32x4*>(pb + (size_t)p * C);
            *reinterpret_cast<f32x4*>(sm.red + sl * C + q * 4) = a;
        }
    }
    __syncthreads();
    const float inv = 1.0f / (float)HW;
    for (int c = tid; c < C; c += ESE_T) {
        float m = sm.red[c];
        for (int sl = 1; sl < NSL; ++sl) m += sm.red[sl * C + c];
        sm.mean_s[c] = m * inv;
    }
    __syncthreads();
    if (o < C) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < ESE_FP; ++j) {
            const int k = lane + 64 * j;
            if (k < C) s += fwv[j] * sm.mean_s[k];
        }
        for (int k = lane + 64 * ESE_FP; k < C; k += 64) s += fw[(size_t)o * C + k] * sm.mean_s[k];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
        if (lane == 0) {
            const float v = s + fb[o] + 3.0f;
            const float gv = fminf(fmaxf(v, 0.f), 6.0f) / 6.0f;
            if (write_gate) gate[b * C + o] = gv;
            sm.g16[wave] = gv;
        }
    }
    __syncthreads();
}
