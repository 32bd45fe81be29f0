// Building blocks the evaluation, TTA, render and tracking kernels share: the block scan and the bitonic sort of ore_coco_eval /
// ore_proposal_recall, finite32 / blend8 of ore_tta / ore_overlay / ore_heatmap / ore_track, and the workspace cursor of every layout
// struct.  Integer work and comparisons only, so a user's -ffp-contract flag does not matter here.
// The hot-path kernels of ore_detect / ore_roi / ore_train keep their own open-coded scans: through these forms they compile to
// different code, and those kernels do not change for the sake of sharing.
#pragma once
#include "ore_common.h"

// v is neither an infinity nor a NaN
__device__ __forceinline__ bool finite32(float v) { return (__builtin_bit_cast(uint32_t, v) & 0x7f800000u) != 0x7f800000u; }

// one 8-bit channel: pixel p under colour c at alpha al / 255, rounded to nearest
__device__ __forceinline__ uint32_t blend8(uint32_t p, uint32_t c, uint32_t al) { return (p * (255u - al) + c * al + 127u) / 255u; }

// ------------------------------------------------------------------ scans
// inclusive scan of v over the 64 lanes of a wave (T = int or int64_t).  No LDS, no barrier.
template <class T>
__device__ __forceinline__ T wave_incl_scan(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// inclusive scan of v over a block of NW whole waves (blockDim.x = 64 * NW, thread order); returns it and the block total.
// Barrier contract: lane 63 of every wave stores its wave total to wsum[NW]; then ONE barrier; every thread reads all of wsum; then a
// SECOND barrier.  So on return no thread still reads wsum: the caller may call again with the same wsum at once (or reuse it for anything
// else), and whatever the caller wrote to LDS before the call is visible to the block after it.  The caller guarantees that no thread
// can still be reading wsum from an earlier use of its own when the call starts (a barrier since that use), and that every thread of
// the block makes the call.
template <int NW, class T>
__device__ __forceinline__ T block_incl_scan(T v, T* wsum, T& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v = wave_incl_scan(v);
    if (lane == 63) wsum[w] = v;
    __syncthreads();
    T pre = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < NW; ++q) {
        pre += q < w ? wsum[q] : 0;
        tot += wsum[q];
    }
    __syncthreads();
    total = tot;
    return v + pre;
}

// ------------------------------------------------------------------ bitonic sort
// `rows` independent rows of P keys each (P = bitonic_size(n): a power of two, at least one LDS block), ascending under Gt ("a sorts
// after b", a functor type); the caller pads a row with keys that sort last.  The row is blockIdx.y.  Instantiate with a K or Gt of the
// including file's unnamed namespace: the kernels then stay internal to that file, as every other kernel of the library is.
constexpr int kSortL = 2048;                    // keys per LDS bitonic block (1024 threads)

static inline int64_t bitonic_size(int64_t n) {
    int64_t p = kSortL;
    while (p < n) p <<= 1;
    return p;
}

// bitonic steps k in [k_lo, k_hi] (powers of two), j from min(k, kSortL) / 2 down to 1, on one LDS block of kSortL keys
template <class K, class Gt>
__global__ __launch_bounds__(1024) void k_bitonic_local(K* keys, int64_t P, int64_t k_lo, int64_t k_hi) {
    __shared__ K s[kSortL];
    K* row = keys + (int64_t)blockIdx.y * P;
    const int64_t base = (int64_t)blockIdx.x * kSortL;
    for (int q = threadIdx.x; q < kSortL; q += 1024) s[q] = row[base + q];
    __syncthreads();
    for (int64_t k = k_lo; k <= k_hi; k <<= 1) {
        for (int j = (int)((k < kSortL ? k : kSortL) >> 1); j > 0; j >>= 1) {
            const int t = threadIdx.x;
            const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));    // lower index of the t-th pair at distance j
            const int l = i + j;
            const bool asc = ((base + i) & k) == 0;
            const K x = s[i], y = s[l];
            if ((asc && Gt()(x, y)) || (!asc && Gt()(y, x))) {
                s[i] = y;
                s[l] = x;
            }
            __syncthreads();
        }
    }
    for (int q = threadIdx.x; q < kSortL; q += 1024) row[base + q] = s[q];
}

// one step (k, j) with j >= kSortL, on global memory
template <class K, class Gt>
__global__ void k_bitonic_global(K* keys, int64_t P, int64_t k, int64_t j) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= P / 2) return;
    K* row = keys + (int64_t)blockIdx.y * P;
    const int64_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
    const bool asc = (i & k) == 0;
    const K x = row[i], y = row[l];
    if ((asc && Gt()(x, y)) || (!asc && Gt()(y, x))) {
        row[i] = y;
        row[l] = x;
    }
}

template <class K, class Gt>
static inline void bitonic_sort_rows(K* keys, int64_t P, int rows, hipStream_t s) {
    const dim3 gl((unsigned)(P / kSortL), (unsigned)rows), gg((unsigned)ceil_div((int)(P / 2), 256), (unsigned)rows);
    hipLaunchKernelGGL((k_bitonic_local<K, Gt>), gl, dim3(1024), 0, s, keys, P, (int64_t)2, (int64_t)kSortL);
    for (int64_t k = 2 * kSortL; k <= P; k <<= 1) {
        for (int64_t j = k >> 1; j >= kSortL; j >>= 1) hipLaunchKernelGGL((k_bitonic_global<K, Gt>), gg, dim3(256), 0, s, keys, P, k, j);
        hipLaunchKernelGGL((k_bitonic_local<K, Gt>), gl, dim3(1024), 0, s, keys, P, k, k);
    }
}

// ------------------------------------------------------------------ workspace layout
// running offset into a workspace, every region on a 256-byte boundary (host only)
struct WsCursor {
    size_t o = 0;
    size_t take(size_t bytes) {
        const size_t r = o;
        o += (bytes + 255) & ~(size_t)255;
        return r;
    }
};
