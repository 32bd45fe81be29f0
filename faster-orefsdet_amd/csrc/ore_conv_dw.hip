// Depthwise-separable unit of the VoVNet *-dw-* bodies (d2z:modeling/backbone/vovnet.py:110-130): depthwise 3x3 -> pointwise 1x1 ->
// FrozenBN -> ReLU, with NO norm or activation between the two convs, C_in == C_out == C.
//   k_dwpw         the whole unit in one launch: the depthwise result lives in LDS only and is the MFMA operand of the pointwise GEMM
//   k_dw3x3        the depthwise conv alone (backward's recompute of the pointwise input; flipped taps = its data gradient)
//   k_dw3x3_wgrad  + k_dw3x3_wgrad_sum: the depthwise weight gradient, a fixed split over pixels and a fixed-order second pass
// All fp32 (the process-wide bf16 operand mode does not reach these kernels), NHWC channel slices of wider buffers like every conv here.
#include "ore_common.h"

namespace {

constexpr int DW_BM = 64;          // output pixels of one k_dwpw block (4 waves x one 16-pixel MFMA tile)
constexpr int DW_KC = 64;          // channels of one K chunk: 4 MFMA sub-chunks of 16, formed (and their loads issued) together
constexpr int DW_TLD = DW_KC + 4;  // LDS row stride of the depthwise tile: the chunk + 4 floats of padding (rows stay 16-byte aligned)
constexpr int DW_MAXC = 1024;      // widest unit (the depthwise taps of all C channels are staged in LDS: 36 KiB at 1024)

// One output pixel's depthwise sum for 4 consecutive channels: 9 taps, zero outside the image (never the neighbouring image of the batch:
// iy / ix are tested against this image's H / W, and b selects the image).  wd: taps in LDS as [9][C].  A tap outside the image loads
// from the nearest pixel INSIDE it and the value is then replaced by zero (a select, not a product: whatever lies there, NaN included,
// does not reach the sum): straight-line code whose nine loads -- and those of the caller's other channel groups -- are in flight together.
template <bool FLIP>
__device__ __forceinline__ f32x4 dw_pixel(const float* in, int64_t ld_in, int b, int oy, int ox, int H, int W, int stride,
                                          const float* wd, int C, int c) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * stride - 1 + ky;
        const int cy = iy < 0 ? 0 : (iy >= H ? H - 1 : iy);
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox * stride - 1 + kx;
            const int cx = ix < 0 ? 0 : (ix >= W ? W - 1 : ix);
            const bool inside = iy == cy && ix == cx;
            const int tap = FLIP ? 8 - (ky * 3 + kx) : ky * 3 + kx;
            f32x4 x = ld4(in + (((int64_t)b * H + cy) * W + cx) * ld_in + c);
            if (!inside) x = f32x4{0.f, 0.f, 0.f, 0.f};
            const f32x4 w = ld4(wd + tap * C + c);
            acc.x = fmaf(x.x, w.x, acc.x);
            acc.y = fmaf(x.y, w.y, acc.y);
            acc.z = fmaf(x.z, w.z, acc.z);
            acc.w = fmaf(x.w, w.w, acc.w);
        }
    }
    return acc;
}

// [C][3][3] (the Conv2d weight [C,1,3,3]) -> LDS [9][C]
__device__ __forceinline__ void stage_taps(const float* w_dw, float* wd, int C) {
    for (int i = threadIdx.x; i < C * 9; i += blockDim.x) wd[(i % 9) * C + i / 9] = w_dw[i];
}

// Block: 64 consecutive output pixels (flat over B*Ho*Wo) x NT*16 output channels (blockIdx.y selects the channel group).  K runs over
// all C input channels in chunks of up to 64: 256 threads form the 64 x 64 depthwise tile into LDS (one pixel x 4 channels in each of
// the chunk's 16-channel sub-chunks per thread: up to 36 independent 16-byte loads in flight per thread -- these layers are bound by
// the latency of that chain, not by arithmetic, so a body's widths take one or two trips instead of C / 16), then every wave
// multiplies its 16 pixels against the pointwise weights: D^T = W_pw[n][k] * T[k][pixel], so a lane ends with 4 consecutive output
// channels of ONE pixel (one 16-byte store).  Within a sub-chunk lane l carries k = 4 * (l >> 4) + j in MFMA step j for both operands
// (a float4 of LDS / of the weight row), which only permutes the order the 16 products are summed in.
template <int NT>
__global__ __launch_bounds__(256) void k_dwpw(const float* in, int ld_in, int in_coff, int B, int H, int W, int Ho, int Wo, int C,
                                              int stride, const float* __restrict__ w_dw, const float* __restrict__ w_pw,
                                              const float* __restrict__ scale, const float* __restrict__ shift, float* out, int ld_out,
                                              int out_coff) {
    extern __shared__ __align__(16) float smem[];
    float* wd = smem;                                   // [9][C]
    float* T = smem + 9 * C;                            // [DW_BM][DW_TLD]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t M = (int64_t)B * Ho * Wo, m0 = (int64_t)blockIdx.x * DW_BM;
    const int n0 = blockIdx.y * NT * 16;
    stage_taps(w_dw, wd, C);
    // this thread's pixel and channel quad of the depthwise tile
    const int tp = tid >> 2, tq = (tid & 3) * 4;
    const int64_t tm = m0 + tp;
    const bool tlive = tm < M;
    int tb = 0, toy = 0, tox = 0;
    if (tlive) {
        tb = (int)(tm / ((int64_t)Ho * Wo));
        const int r = (int)(tm - (int64_t)tb * Ho * Wo);
        toy = r / Wo;
        tox = r - toy * Wo;
    }
    f32x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int li = lane & 15, lg = lane >> 4;
    __syncthreads();                                    // the taps are staged
    for (int k0 = 0; k0 < C; k0 += DW_KC) {
        const int kc = C - k0 < DW_KC ? C - k0 : DW_KC;  // channels of this chunk (a multiple of 16; the same for the whole block)
        f32x4 t[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            t[i] = (tlive && i * 16 < kc) ? dw_pixel<false>(in + in_coff, ld_in, tb, toy, tox, H, W, stride, wd, C, k0 + i * 16 + tq)
                                          : f32x4{0.f, 0.f, 0.f, 0.f};
        if (k0) __syncthreads();                        // every wave has read the previous chunk's tile
#pragma unroll
        for (int i = 0; i < 4; ++i) st4(T + tp * DW_TLD + i * 16 + tq, t[i]);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i * 16 >= kc) break;
            const f32x4 a = ld4(T + (wave * 16 + li) * DW_TLD + i * 16 + lg * 4);
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const f32x4 w = ld4(w_pw + (int64_t)(n0 + j * 16 + li) * C + k0 + i * 16 + lg * 4);
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, a.x, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, a.y, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, a.z, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, a.w, acc[j], 0, 0, 0);
            }
        }
    }
    // epilogue: lane = pixel li of the wave's tile, channels n0 + j * 16 + 4 * lg .. + 3
    const int64_t m = m0 + wave * 16 + li;
    if (m >= M) return;
    float* o = out + m * ld_out + out_coff;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = n0 + j * 16 + lg * 4;
        const f32x4 sc = scale ? ld4(scale + n) : f32x4{1.f, 1.f, 1.f, 1.f};
        const f32x4 sh = shift ? ld4(shift + n) : f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 y;
        y.x = fmaxf(fmaf(acc[j].x, sc.x, sh.x), 0.f);
        y.y = fmaxf(fmaf(acc[j].y, sc.y, sh.y), 0.f);
        y.z = fmaxf(fmaf(acc[j].z, sc.z, sh.z), 0.f);
        y.w = fmaxf(fmaf(acc[j].w, sc.w, sh.w), 0.f);
        st4(o + n, y);
    }
}

// One thread = one output pixel x 4 channels.  FLIP: taps mirrored (the data gradient at stride 1).  accumulate: out += result.
template <bool FLIP>
__global__ __launch_bounds__(256) void k_dw3x3(const float* in, int ld_in, int in_coff, int B, int H, int W, int Ho, int Wo, int C, int stride,
                                               const float* __restrict__ w_dw, float* out, int ld_out, int out_coff, int accumulate) {
    extern __shared__ __align__(16) float smem[];
    stage_taps(w_dw, smem, C);
    __syncthreads();
    const int cq = C >> 2;
    const int64_t total = (int64_t)B * Ho * Wo * cq;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = i / cq;
        const int c = (int)(i - m * cq) * 4;
        const int b = (int)(m / ((int64_t)Ho * Wo));
        const int r = (int)(m - (int64_t)b * Ho * Wo);
        const int oy = r / Wo, ox = r - oy * Wo;
        f32x4 y = dw_pixel<FLIP>(in + in_coff, ld_in, b, oy, ox, H, W, stride, smem, C, c);
        float* o = out + m * ld_out + out_coff + c;
        if (accumulate) {
            const f32x4 p = ld4(o);
            y.x += p.x; y.y += p.y; y.z += p.z; y.w += p.w;
        }
        st4(o, y);
    }
}

constexpr int WG_ROWS = 256;       // pixels of one part of the weight-gradient split (fixed: the split never depends on the device)
constexpr int WG_CH = 64;          // channels of one block (16 quads x 16 pixel lanes = 256 threads)

// part[blockIdx.x][c][tap] = sum over the part's pixels of x[b, y + ky - 1, x + kx - 1, c] * dt[b, y, x, c].  Thread (pl, q): pixels
// pl, pl + 16, ... of the part in order, channels 4q .. 4q + 3 of the block's 64; the 16 pixel lanes are then summed in lane order.
__global__ __launch_bounds__(256) void k_dw3x3_wgrad(const float* __restrict__ x, int x_ld, int x_coff, const float* __restrict__ dt, int dt_ld,
                                                     int dt_coff, int B, int H, int W, int C, float* __restrict__ part) {
    __shared__ float red[16][16 * 36 + 4];
    const int q = threadIdx.x & 15, pl = threadIdx.x >> 4;
    const int c = blockIdx.y * WG_CH + q * 4;
    const int64_t M = (int64_t)B * H * W, m0 = (int64_t)blockIdx.x * WG_ROWS;
    float acc[9][4];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t][j] = 0.f;
    if (c < C) {
        for (int p = pl; p < WG_ROWS; p += 16) {
            const int64_t m = m0 + p;
            if (m >= M) break;
            const int b = (int)(m / ((int64_t)H * W));
            const int r = (int)(m - (int64_t)b * H * W);
            const int y = r / W, xx = r - y * W;
            const f32x4 g = ld4(dt + m * dt_ld + dt_coff + c);
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int iy = y + ky - 1;
                if (iy < 0 || iy >= H) continue;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int ix = xx + kx - 1;
                    if (ix < 0 || ix >= W) continue;
                    const f32x4 v = ld4(x + (((int64_t)b * H + iy) * W + ix) * x_ld + x_coff + c);
                    float* a = acc[ky * 3 + kx];
                    a[0] = fmaf(v.x, g.x, a[0]);
                    a[1] = fmaf(v.y, g.y, a[1]);
                    a[2] = fmaf(v.z, g.z, a[2]);
                    a[3] = fmaf(v.w, g.w, a[3]);
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) red[pl][q * 36 + t * 4 + j] = acc[t][j];
    __syncthreads();
    for (int i = threadIdx.x; i < 16 * 36; i += 256) {
        const int qq = i / 36, e = i - qq * 36, t = e >> 2, j = e & 3;
        const int cc = blockIdx.y * WG_CH + qq * 4 + j;
        if (cc >= C) continue;
        float s = red[0][i];
        for (int l = 1; l < 16; ++l) s += red[l][i];
        part[((int64_t)blockIdx.x * C + cc) * 9 + t] = s;
    }
}

// dw[i] = beta * dw[i] + part[0][i] + part[1][i] + ... in that order (beta == 0: dw is not read)
__global__ void k_dw3x3_wgrad_sum(const float* __restrict__ part, int parts, int n, float beta, float* dw) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = part[i];
    for (int p = 1; p < parts; ++p) s += part[(int64_t)p * n + i];
    dw[i] = beta != 0.f ? fmaf(beta, dw[i], s) : s;
}

int check_dw_args(const char* who, const void* in, int32_t ld_in, int32_t in_coff, int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride,
                  const void* w, const void* out, int32_t ld_out, int32_t out_coff, int cmul) {
    ORE_CHECK_ARG(in && w && out, "%s: null pointer", who);
    ORE_CHECK_ARG(B > 0 && H > 0 && W > 0, "%s: empty input %d x %d x %d", who, B, H, W);
    ORE_CHECK_ARG(C > 0 && C % cmul == 0 && C <= DW_MAXC, "%s: C = %d must be a multiple of %d, at most %d", who, C, cmul, DW_MAXC);
    ORE_CHECK_ARG(stride == 1 || stride == 2, "%s: stride %d (1 or 2)", who, stride);
    ORE_CHECK_ARG(in_coff >= 0 && in_coff % 4 == 0 && ld_in % 4 == 0 && in_coff + C <= ld_in, "%s: input slice [%d, %d) of rows of %d (multiples of 4)",
                  who, in_coff, in_coff + C, ld_in);
    ORE_CHECK_ARG(out_coff >= 0 && out_coff % 4 == 0 && ld_out % 4 == 0 && out_coff + C <= ld_out,
                  "%s: output slice [%d, %d) of rows of %d (multiples of 4)", who, out_coff, out_coff + C, ld_out);
    ORE_CHECK_ARG(((uintptr_t)in | (uintptr_t)out) % 16 == 0, "%s: input and output must be 16-byte aligned (the kernels move 4 floats at a time)", who);
    return ORE_OK;
}

// An input and an output slice that share memory (the OSA chain: two channel slices of one concat buffer) must never meet: either the
// two spans are apart, or the rows coincide (same row stride) and the slices lie side by side in every row.
int check_dw_overlap(const char* who, const float* in, int32_t ld_in, int32_t in_coff, int64_t rows_in, const float* out, int32_t ld_out,
                     int32_t out_coff, int64_t rows_out, int32_t C) {
    const float* a0 = in + in_coff; const float* a1 = a0 + (rows_in - 1) * ld_in + C;
    const float* b0 = out + out_coff; const float* b1 = b0 + (rows_out - 1) * ld_out + C;
    if (a1 <= b0 || b1 <= a0) return ORE_OK;
    const int64_t d = ld_in == ld_out ? (((b0 - a0) % ld_in) + ld_in) % ld_in : -1;
    ORE_CHECK_ARG(d >= C && d <= ld_in - C, "%s: the input and output slices overlap", who);
    return ORE_OK;
}

}  // namespace

extern "C" {

int ore_dwpw_fwd(const float* in, int32_t ld_in, int32_t in_coff, int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride,
                 const float* w_dw, const float* w_pw, const float* scale, const float* shift, float* out, int32_t ld_out,
                 int32_t out_coff, void* stream) {
    int rc = check_dw_args("ore_dwpw_fwd", in, ld_in, in_coff, B, H, W, C, stride, w_dw, out, ld_out, out_coff, 16);
    if (rc) return rc;
    ORE_CHECK_ARG(w_pw, "ore_dwpw_fwd: null pointwise weights");
    ORE_CHECK_ARG(((uintptr_t)w_pw | (uintptr_t)scale | (uintptr_t)shift) % 16 == 0, "ore_dwpw_fwd: w_pw, scale and shift must be 16-byte aligned");
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const int64_t M = (int64_t)B * Ho * Wo;
    if ((rc = check_dw_overlap("ore_dwpw_fwd", in, ld_in, in_coff, (int64_t)B * H * W, out, ld_out, out_coff, M, C))) return rc;
    ORE_CHECK_ARG((M + DW_BM - 1) / DW_BM <= 0x7fffffff, "ore_dwpw_fwd: %lld output pixels", (long long)M);
    // the largest channel group (<= 8 MFMA tiles per wave) that divides C / 16
    int NT = 1;
    for (int t = 8; t >= 1; --t)
        if ((C / 16) % t == 0) { NT = t; break; }
    const dim3 grid((unsigned)((M + DW_BM - 1) / DW_BM), (unsigned)(C / 16 / NT));
    const size_t lds = ((size_t)9 * C + DW_BM * DW_TLD) * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
#define DWPW(N) case N: hipLaunchKernelGGL(k_dwpw<N>, grid, dim3(256), lds, s, in, ld_in, in_coff, B, H, W, Ho, Wo, C, stride, w_dw, w_pw, scale, shift, out, ld_out, out_coff); break;
    switch (NT) { DWPW(1) DWPW(2) DWPW(3) DWPW(4) DWPW(5) DWPW(6) DWPW(7) DWPW(8) }
#undef DWPW
    ore_flop_count_add(ore_dwpw_flops(M, C));
    return ore_launch_status("k_dwpw");
}

// The planner's rule, from profiles/dw_bench.json: the fused launch loses to k_dw3x3 + the 1x1 conv launch, in stream time and in traced
// kernel time alike, at the large stride-1 units (stem_2 at 640x640, 102400 rows x 64 channels: 41.8 against 38.3 us; stem_2 and stage 2
// of 16 images: 533 against 479, 138 against 127 us) and wins at the smaller ones (<= 25600 x 64) in stream time.
int32_t ore_dwpw_prefers_composition(int64_t rows, int32_t C, int32_t stride) {
    return stride == 1 && rows * (int64_t)C >= ((int64_t)1 << 22);
}

int ore_dwpw_planned_fwd(const float* in, int32_t ld_in, int32_t in_coff, int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride,
                         const float* w_dw, const float* w_pw, const float* scale, const float* shift, float* out, int32_t ld_out,
                         int32_t out_coff, float* scratch, size_t scratch_floats, void* stream) {
    const int Ho = stride > 0 ? (H - 1) / stride + 1 : 0, Wo = stride > 0 ? (W - 1) / stride + 1 : 0;
    const int64_t M = (int64_t)B * Ho * Wo;
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || !ore_dwpw_prefers_composition(M, C, stride))
        return ore_dwpw_fwd(in, ld_in, in_coff, B, H, W, C, stride, w_dw, w_pw, scale, shift, out, ld_out, out_coff, stream);
    if (!scratch || scratch_floats < (size_t)M * C) {
        ore_set_error("ore_dwpw_planned_fwd: scratch of %zu floats needed for the unfused form (got %zu)", (size_t)M * C, scratch_floats);
        return ORE_ENOMEM;
    }
    ORE_CHECK_ARG(C % 16 == 0 && w_pw, "ore_dwpw_planned_fwd: C = %d must be a multiple of 16, w_pw not null", C);
    int rc = ore_dw3x3_fwd(in, ld_in, in_coff, B, H, W, C, stride, w_dw, 0, scratch, C, 0, 0, stream);
    if (rc) return rc;
    ore_conv_desc d{};
    d.in = scratch; d.in_ld = C; d.B = B; d.H = Ho; d.W = Wo; d.Cin = C;
    d.w = w_pw; d.Cout = C; d.kh = d.kw = 1; d.stride = 1; d.pad = 0;
    d.scale = scale; d.shift = shift; d.relu_cout = C;
    d.out = out; d.out_ld = ld_out; d.out_coff = out_coff;
    d.splitk = 1;
    const int mode = ore_conv_get_precision();          // the unit is fp32 in every conv precision mode
    ore_conv_set_precision(ORE_CONV_FP32);
    rc = ore_conv2d_fwd(&d, stream);                    // (counts its own 2 * M * C * C)
    ore_conv_set_precision(mode);
    if (!rc) ore_flop_count_add(2.0 * (double)M * C * 9.0);
    return rc;
}

int ore_dw3x3_fwd(const float* in, int32_t ld_in, int32_t in_coff, int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride,
                  const float* w_dw, int32_t dgrad, float* out, int32_t ld_out, int32_t out_coff, int32_t accumulate, void* stream) {
    int rc = check_dw_args("ore_dw3x3_fwd", in, ld_in, in_coff, B, H, W, C, stride, w_dw, out, ld_out, out_coff, 4);
    if (rc) return rc;
    ORE_CHECK_ARG(!dgrad || stride == 1, "ore_dw3x3_fwd: the data-gradient form exists at stride 1 only (the one stride-2 unit, stem_3, is frozen)");
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    if ((rc = check_dw_overlap("ore_dw3x3_fwd", in, ld_in, in_coff, (int64_t)B * H * W, out, ld_out, out_coff, (int64_t)B * Ho * Wo, C))) return rc;
    const int64_t total = (int64_t)B * Ho * Wo * (C / 4);
    int64_t blocks = (total + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    const size_t lds = (size_t)9 * C * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    if (dgrad)
        hipLaunchKernelGGL(k_dw3x3<true>, dim3((unsigned)blocks), dim3(256), lds, s, in, ld_in, in_coff, B, H, W, Ho, Wo, C, stride, w_dw, out, ld_out,
                           out_coff, accumulate);
    else
        hipLaunchKernelGGL(k_dw3x3<false>, dim3((unsigned)blocks), dim3(256), lds, s, in, ld_in, in_coff, B, H, W, Ho, Wo, C, stride, w_dw, out, ld_out,
                           out_coff, accumulate);
    return ore_launch_status("k_dw3x3");
}

size_t ore_dw3x3_wgrad_workspace_floats(int64_t rows, int32_t C) {
    if (rows <= 0 || C <= 0) return 0;
    return (size_t)((rows + WG_ROWS - 1) / WG_ROWS) * (size_t)C * 9;
}

int ore_dw3x3_wgrad_fwd(const float* x, int32_t x_ld, int32_t x_coff, const float* dt, int32_t dt_ld, int32_t dt_coff, int32_t B, int32_t H,
                        int32_t W, int32_t C, float* dw, float beta, float* workspace, size_t workspace_floats, void* stream) {
    int rc = check_dw_args("ore_dw3x3_wgrad_fwd", x, x_ld, x_coff, B, H, W, C, 1, dt, dw, dt_ld, dt_coff, 4);
    if (rc) return rc;
    const int64_t M = (int64_t)B * H * W;
    const size_t need = ore_dw3x3_wgrad_workspace_floats(M, C);
    if (!workspace || workspace_floats < need) {
        ore_set_error("ore_dw3x3_wgrad_fwd: workspace of %zu floats needed (got %zu)", need, workspace_floats);
        return ORE_ENOMEM;
    }
    const int64_t parts = (M + WG_ROWS - 1) / WG_ROWS;
    ORE_CHECK_ARG(parts <= 0x7fffffff, "ore_dw3x3_wgrad_fwd: %lld pixels", (long long)M);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_dw3x3_wgrad, dim3((unsigned)parts, (unsigned)((C + WG_CH - 1) / WG_CH)), dim3(256), 0, s, x, x_ld, x_coff, dt, dt_ld, dt_coff,
                       B, H, W, C, workspace);
    rc = ore_launch_status("k_dw3x3_wgrad");
    if (rc) return rc;
    hipLaunchKernelGGL(k_dw3x3_wgrad_sum, dim3((unsigned)((C * 9 + 255) / 256)), dim3(256), 0, s, workspace, (int)parts, C * 9, beta, dw);
    return ore_launch_status("k_dw3x3_wgrad_sum");
}

}  // extern "C"
