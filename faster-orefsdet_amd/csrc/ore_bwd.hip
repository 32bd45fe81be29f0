// Backward kernels of the trainable layers ("..._bwd counterparts for trainable layers", 8b), the convolutions'
// gradients apart (weight gradient: ore_conv_wgrad.hip; data gradient: the forward conv kernels on the flipped weights).
//   k_pack_weight(_multi)   OIHW master weights -> the forward igemm layout, or the flipped/transposed layout that turns the forward
//                           kernel into the data-gradient conv (dX = conv(dZ, W^T flipped)); runs on device once per optimizer step
//   k_relu_affine_bwd       dZ = dY * (Y > 0) * scale[c]          (conv + FrozenBN + ReLU epilogue backward)
//   k_colsum_chunks/_final  bias gradient = column sums of dZ, two deterministic stages
//   k_corr_fwd_train, k_corr_bwd_a/_b   the correlation block of the head, forward (training form) and backward
//   k_gn_apply, k_gn_apply_levels_h, k_gn_bwd_prod/_dx, k_colsum_seg/_seg_fin, k_scale_add   GroupNorm (+ ReLU) forward / backward
//   k_maxpool_bwd, k_sumpool2, k_apool_fwd/_fwd_big/_bwd, k_group_sum/_bcast   pooling and group means, forward / backward
//   k_granule_transpose, k_combine2(_bwd)   the layout change and the gated sum of the attention branch
// What they replace: torch.autograd of F.relu / FrozenBatchNorm2d / GroupNorm / the poolings
//   (d2z:layers/wrappers.py:48-91, d2z:layers/batch_norm.py:44-66) inside d2z:engine/train_loop.py:279 `losses.backward()`.
#include "ore_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pack_weight(const float* __restrict__ w, int Co, int Ci, int kh, int kw, int mode,
                                                     float* __restrict__ dst, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int taps = kh * kw;
    if (mode == 0) {                                   // [Co16][tap][Ci]
        const int ci = (int)(i % Ci);
        const int tap = (int)((i / Ci) % taps);
        const int co = (int)(i / ((long long)Ci * taps));
        dst[i] = co < Co ? w[((size_t)co * Ci + ci) * taps + tap] : 0.0f;
    } else {                                           // [Ci16][flipped tap][Co16]
        const int Co16 = (Co + 15) / 16 * 16;
        const int co = (int)(i % Co16);
        const int tap = (int)((i / Co16) % taps);
        const int ci = (int)(i / ((long long)Co16 * taps));
        dst[i] = (co < Co && ci < Ci) ? w[((size_t)co * Ci + ci) * taps + (taps - 1 - tap)] : 0.0f;
    }
}

// All the repacks of an optimizer step in ONE launch (round 5: ~86 launches of 4.4 us per step, a third of a millisecond of a 10 ms
// single-image step).  Element i belongs to the job whose [first, first + n) holds it (binary search over <= 256 jobs in LDS).
__global__ __launch_bounds__(256) void k_pack_weight_multi(const ore_pack_job* __restrict__ jobs, int n_jobs, long long total) {
    __shared__ long long first[257];
    for (int j = threadIdx.x; j <= n_jobs; j += 256) first[j] = j < n_jobs ? jobs[j].first : total;
    __syncthreads();
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first[mid] <= g) lo = mid; else hi = mid - 1;
    }
    const ore_pack_job jb = jobs[lo];
    const long long i = g - jb.first;
    const int Co = jb.Cout, Ci = jb.Cin, taps = jb.kh * jb.kw;
    if (jb.dgrad == 0) {                               // [Co16][tap][Ci]
        const int ci = (int)(i % Ci);
        const int tap = (int)((i / Ci) % taps);
        const int co = (int)(i / ((long long)Ci * taps));
        jb.dst[i] = co < Co ? jb.src[((size_t)co * Ci + ci) * taps + tap] : 0.0f;
    } else {                                           // [Ci16][flipped tap][Co16]
        const int Co16 = (Co + 15) / 16 * 16;
        const int co = (int)(i % Co16);
        const int tap = (int)((i / Co16) % taps);
        const int ci = (int)(i / ((long long)Co16 * taps));
        jb.dst[i] = (co < Co && ci < Ci) ? jb.src[((size_t)co * Ci + ci) * taps + (taps - 1 - tap)] : 0.0f;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_relu_affine_bwd(const float* __restrict__ dy, int dy_ld, int dy_coff, const float* __restrict__ y,
                                                         int y_ld, int y_coff, const float* __restrict__ scale, long long rows, int C,
                                                         float* __restrict__ dz, int dz_ld, int dz_coff) {
    const int c4n = C / 4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * c4n) return;
    const long long r = i / c4n;
    const int c = (int)(i % c4n) * 4;
    const f32x4 g = *reinterpret_cast<const f32x4*>(dy + r * dy_ld + dy_coff + c);
    const f32x4 v = *reinterpret_cast<const f32x4*>(y + r * y_ld + y_coff + c);
    f32x4 s = f32x4{1.f, 1.f, 1.f, 1.f};
    if (scale) s = *reinterpret_cast<const f32x4*>(scale + c);
    f32x4 o;
    o.x = v.x > 0.f ? g.x * s.x : 0.f;
    o.y = v.y > 0.f ? g.y * s.y : 0.f;
    o.z = v.z > 0.f ? g.z * s.z : 0.f;
    o.w = v.w > 0.f ? g.w * s.w : 0.f;
    *reinterpret_cast<f32x4*>(dz + r * dz_ld + dz_coff + c) = o;
}

// column sums: stage 1 = 256-row chunks (64 channels x 4 row lanes per block, lanes combined in fixed order through LDS),
// stage 2 = chunks in order.  Deterministic.
constexpr int CS_ROWS = 256;
// Segmented form: the rows are `segments` equal runs of rows_per_seg; chunk boundaries restart with every segment, so a segment's
// sums are bitwise those of a call on that segment alone.  blockIdx.x = segment * cps + chunk.
__global__ __launch_bounds__(256) void k_colsum_chunks(const float* __restrict__ x, int ld, int coff, long long rows_per_seg, int cps, int C,
                                                       float* __restrict__ part) {
    __shared__ float red[4][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + cl;
    const int seg = blockIdx.x / cps, chunk = blockIdx.x - seg * cps;
    const long long s0r = (long long)seg * rows_per_seg;
    const long long r0 = s0r + (long long)chunk * CS_ROWS, r1 = min(s0r + rows_per_seg, r0 + CS_ROWS);
    float s0 = 0.f, s1 = 0.f;
    if (c < C) {
        long long r = r0 + rl;
        for (; r + 4 < r1; r += 8) { s0 += x[r * ld + coff + c]; s1 += x[(r + 4) * ld + coff + c]; }
        if (r < r1) s0 += x[r * ld + coff + c];
    }
    red[rl][cl] = s0 + s1;
    __syncthreads();
    if (rl == 0 && c < C) part[(size_t)blockIdx.x * C + c] = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
}
// stage 2: one block = 64 channels x 4 chunk lanes of one segment (lane l sums chunks l, l+4, ... in order, lanes combined in fixed order)
__global__ __launch_bounds__(256) void k_colsum_final(const float* __restrict__ part, int cps, int C, float beta, float* __restrict__ out) {
    __shared__ float red[4][64];
    const int cl = threadIdx.x & 63, kl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    part += (size_t)blockIdx.y * cps * C;
    out += (size_t)blockIdx.y * C;
    float s0 = 0.f, s1 = 0.f;
    if (c < C) {
        int k = kl;
        for (; k + 4 < cps; k += 8) { s0 += part[(size_t)k * C + c]; s1 += part[(size_t)(k + 4) * C + c]; }
        if (k < cps) s0 += part[(size_t)k * C + c];
    }
    red[kl][cl] = s0 + s1;
    __syncthreads();
    if (kl == 0 && c < C) {
        const float s = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
        out[c] = beta != 0.0f ? beta * out[c] + s : s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Depthwise support correlation with gradients (ref:fewx/modeling/fsod/fsod_cen.py:229-245, training branch):
//   a2 = relu(k11 * relu(k11 * q));  t = relu(conv1x3(q, k13));  u = conv3x1(t, k31);  attn = a2 + relu(u) + q
// Forward (training) writes [attn | q] into the 2C-wide input of conv3 and keeps t, u.  Backward in two passes so that every
// neighbourhood is a 3-tap read: pass A: dT = [t>0] * conv3x1^T(dU), per-row products for dk31; pass B: dq and the per-row products
// for dk13 / dk11.  The per-row products are then column-summed (ore_colsum_fwd) -- deterministic.
struct CorrT {
    const float* q; int q_ld, q_coff;
    int H, W, C4, rows;
    const float* k11; const float* k13; const float* k31;   // [C], [C][3], [C][3]; per image ([B][C], [B][C][3]) when kps = 1
    int kps;
};
__device__ __forceinline__ f32x4 relu4b(f32x4 v) { return f32x4{fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)}; }
__device__ __forceinline__ f32x4 gt0(f32x4 v, f32x4 g) { return f32x4{v.x > 0.f ? g.x : 0.f, v.y > 0.f ? g.y : 0.f, v.z > 0.f ? g.z : 0.f, v.w > 0.f ? g.w : 0.f}; }
__device__ __forceinline__ void ld3(const float* k, int c, f32x4* w) {
#pragma unroll
    for (int j = 0; j < 3; ++j) w[j] = f32x4{k[(c + 0) * 3 + j], k[(c + 1) * 3 + j], k[(c + 2) * 3 + j], k[(c + 3) * 3 + j]};
}

__global__ __launch_bounds__(256) void k_corr_fwd_train(CorrT p, float* __restrict__ cat, float* __restrict__ T, float* __restrict__ U) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.rows * p.C4) return;
    const int c = (idx % p.C4) * 4, row = idx / p.C4;
    const int C = p.C4 * 4, H = p.H, W = p.W;
    const int b = row / (H * W), rr = row - b * H * W, y = rr / W, x = rr - y * W, base = b * H * W;
    const size_t ko = (size_t)b * p.kps * C;
    const f32x4 w11 = *reinterpret_cast<const f32x4*>(p.k11 + ko + c);
    f32x4 w13[3], w31[3];
    ld3(p.k13 + 3 * ko, c, w13); ld3(p.k31 + 3 * ko, c, w31);
    auto Q = [&](int yy, int xx) -> f32x4 {
        if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W)
            return *reinterpret_cast<const f32x4*>(p.q + (size_t)(base + yy * W + xx) * p.q_ld + p.q_coff + c);
        return f32x4{0.f, 0.f, 0.f, 0.f};
    };
    const f32x4 qc = Q(y, x);
    const f32x4 a = relu4b(w11 * relu4b(w11 * qc));
    f32x4 u = {0.f, 0.f, 0.f, 0.f}, tc = u;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = y + dy;
        if ((unsigned)yy < (unsigned)H) {
            const f32x4 t = relu4b(w13[0] * Q(yy, x - 1) + w13[1] * (dy == 0 ? qc : Q(yy, x)) + w13[2] * Q(yy, x + 1));
            u += w31[dy + 1] * t;
            if (dy == 0) tc = t;
        }
    }
    *reinterpret_cast<f32x4*>(cat + (size_t)row * 2 * C + c) = a + relu4b(u) + qc;
    *reinterpret_cast<f32x4*>(cat + (size_t)row * 2 * C + C + c) = qc;
    *reinterpret_cast<f32x4*>(T + (size_t)row * C + c) = tc;
    *reinterpret_cast<f32x4*>(U + (size_t)row * C + c) = u;
}

// g = dcat[..., :C] (row stride 2C)
__global__ __launch_bounds__(256) void k_corr_bwd_a(CorrT p, const float* __restrict__ dcat, const float* __restrict__ T,
                                                    const float* __restrict__ U, float* __restrict__ DT, float* __restrict__ P) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.rows * p.C4) return;
    const int c = (idx % p.C4) * 4, row = idx / p.C4;
    const int C = p.C4 * 4, H = p.H, W = p.W;
    const int b = row / (H * W), rr = row - b * H * W, y = rr / W;
    f32x4 w31[3];
    ld3(p.k31 + (size_t)3 * b * p.kps * C, c, w31);
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    auto DU = [&](int dy) -> f32x4 {                                    // dU at (y+dy, x)
        if ((unsigned)(y + dy) >= (unsigned)H) return z;
        const size_t r2 = (size_t)(row + dy * W);
        return gt0(*reinterpret_cast<const f32x4*>(U + r2 * C + c), *reinterpret_cast<const f32x4*>(dcat + r2 * 2 * C + c));
    };
    auto TT = [&](int dy) -> f32x4 {
        if ((unsigned)(y + dy) >= (unsigned)H) return z;
        return *reinterpret_cast<const f32x4*>(T + (size_t)(row + dy * W) * C + c);
    };
    const f32x4 du0 = DU(0), tc = TT(0);
    const f32x4 dt = w31[0] * DU(1) + w31[1] * du0 + w31[2] * DU(-1);
    *reinterpret_cast<f32x4*>(DT + (size_t)row * C + c) = gt0(tc, dt);
    *reinterpret_cast<f32x4*>(P + (size_t)row * 7 * C + 4 * C + c) = du0 * TT(-1);      // P row = [P11 | P13 x3 | P31 x3]
    *reinterpret_cast<f32x4*>(P + (size_t)row * 7 * C + 5 * C + c) = du0 * tc;
    *reinterpret_cast<f32x4*>(P + (size_t)row * 7 * C + 6 * C + c) = du0 * TT(1);
}

__global__ __launch_bounds__(256) void k_corr_bwd_b(CorrT p, const float* __restrict__ dcat, const float* __restrict__ DT,
                                                    float* __restrict__ dq, float* __restrict__ P) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.rows * p.C4) return;
    const int c = (idx % p.C4) * 4, row = idx / p.C4;
    const int C = p.C4 * 4, W = p.W;
    const int x = row % W;
    const size_t ko = (size_t)(row / (p.H * W)) * p.kps * C;
    const f32x4 w11 = *reinterpret_cast<const f32x4*>(p.k11 + ko + c);
    f32x4 w13[3];
    ld3(p.k13 + 3 * ko, c, w13);
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    auto Qx = [&](int dx) -> f32x4 {
        if ((unsigned)(x + dx) >= (unsigned)W) return z;
        return *reinterpret_cast<const f32x4*>(p.q + (size_t)(row + dx) * p.q_ld + p.q_coff + c);
    };
    auto D = [&](int dx) -> f32x4 {
        if ((unsigned)(x + dx) >= (unsigned)W) return z;
        return *reinterpret_cast<const f32x4*>(DT + (size_t)(row + dx) * C + c);
    };
    const f32x4 g = *reinterpret_cast<const f32x4*>(dcat + (size_t)row * 2 * C + c);
    const f32x4 g2 = *reinterpret_cast<const f32x4*>(dcat + (size_t)row * 2 * C + C + c);
    const f32x4 qc = Qx(0), dtc = D(0);
    const f32x4 s1 = w11 * qc, a1 = relu4b(s1);
    const f32x4 da2 = gt0(w11 * a1, g);
    const f32x4 da1 = gt0(s1, da2 * w11);
    *reinterpret_cast<f32x4*>(P + (size_t)row * 7 * C + c) = da2 * a1 + da1 * qc;
    *reinterpret_cast<f32x4*>(dq + (size_t)row * C + c) = g + g2 + da1 * w11 + w13[0] * D(1) + w13[1] * dtc + w13[2] * D(-1);
    *reinterpret_cast<f32x4*>(P + (size_t)row * 7 * C + 1 * C + c) = dtc * Qx(-1);
    *reinterpret_cast<f32x4*>(P + (size_t)row * 7 * C + 2 * C + c) = dtc * qc;
    *reinterpret_cast<f32x4*>(P + (size_t)row * 7 * C + 3 * C + c) = dtc * Qx(1);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Small HBM-bound training ops (float4 per thread, NHWC rows x C):
//   GroupNorm(+ReLU) of the head tower with gradients; eSE scale with gradients; ceil-mode 3x3/s2 max-pool backward;
//   2x2 sum-pool (backward of the FPN's nearest-2x top-down add).
// xhat = x * r[c] + a[c] with r = rstd of the channel's group, a = -mean * rstd (from ore_groupnorm_affine_fwd with gamma=1, beta=0).
template <typename TS>
__global__ __launch_bounds__(256) void k_gn_apply(const TS* __restrict__ x, int ld, int coff, long long rows, long long rpi, int C,
                                                  const float* __restrict__ r, const float* __restrict__ a, const float* __restrict__ gamma,
                                                  const float* __restrict__ beta, int relu, TS* __restrict__ y) {
    const int c4n = C / 4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * c4n) return;
    const long long row = i / c4n;
    const int c = (int)(i % c4n) * 4;
    const size_t io = (size_t)(row / rpi) * C;                    // this row's image: r / a are [images][C]
    const f32x4 v = ld4(x + row * ld + coff + c);
    const f32x4 rr = *reinterpret_cast<const f32x4*>(r + io + c), aa = *reinterpret_cast<const f32x4*>(a + io + c);
    f32x4 o = v * rr + aa;
    if (gamma) o = o * *reinterpret_cast<const f32x4*>(gamma + c) + *reinterpret_cast<const f32x4*>(beta + c);
    if (relu) o = relu4b(o);
    st4(y + row * C + c, o);
}

// P[row][0:C] = dy' = dy * [y > 0 or !relu],  P[row][C:2C] = dy' * xhat
__global__ __launch_bounds__(256) void k_gn_bwd_prod(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ x, int ld,
                                                     int coff, long long rows, long long rpi, int C, const float* __restrict__ r,
                                                     const float* __restrict__ a, int relu, float* __restrict__ P) {
    const int c4n = C / 4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * c4n) return;
    const long long row = i / c4n;
    const int c = (int)(i % c4n) * 4;
    const size_t io = (size_t)(row / rpi) * C;
    f32x4 g = *reinterpret_cast<const f32x4*>(dy + row * C + c);
    if (relu) g = gt0(*reinterpret_cast<const f32x4*>(y + row * C + c), g);
    const f32x4 xh = *reinterpret_cast<const f32x4*>(x + row * ld + coff + c) * *reinterpret_cast<const f32x4*>(r + io + c) +
                     *reinterpret_cast<const f32x4*>(a + io + c);
    *reinterpret_cast<f32x4*>(P + row * 2 * C + c) = g;
    *reinterpret_cast<f32x4*>(P + row * 2 * C + C + c) = g * xh;
}

// dx = r * (gamma * dy' - (S1_g + xhat * S2_g) / n),  S1_g = sum_{c in g} gamma_c dbeta_c,  S2_g = sum_{c in g} gamma_c dgamma_c
__global__ __launch_bounds__(256) void k_gn_bwd_dx(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ x, int ld,
                                                   int coff, long long rows, long long rpi, int C, int cpg, const float* __restrict__ r,
                                                   const float* __restrict__ a, const float* __restrict__ gamma,
                                                   const float* __restrict__ sums /* [images][2C]: dbeta | dgamma */, int relu,
                                                   float* __restrict__ dx) {
    const int c4n = C / 4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * c4n) return;
    const long long row = i / c4n;
    const int c = (int)(i % c4n) * 4;
    const size_t img = (size_t)(row / rpi);
    r += img * C; a += img * C; sums += img * 2 * C;
    const float inv_n = 1.0f / ((float)rpi * (float)cpg);
    f32x4 g = *reinterpret_cast<const f32x4*>(dy + row * C + c);
    if (relu) g = gt0(*reinterpret_cast<const f32x4*>(y + row * C + c), g);
    const f32x4 rr = *reinterpret_cast<const f32x4*>(r + c);
    const f32x4 xh = *reinterpret_cast<const f32x4*>(x + row * ld + coff + c) * rr + *reinterpret_cast<const f32x4*>(a + c);
    const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + c);
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int g0 = ((c + k) / cpg) * cpg;
        float s1 = 0.f, s2 = 0.f;
        for (int q = 0; q < cpg; ++q) { s1 += gamma[g0 + q] * sums[g0 + q]; s2 += gamma[g0 + q] * sums[C + g0 + q]; }
        o[k] = rr[k] * (gm[k] * g[k] - (s1 + xh[k] * s2) * inv_n);
    }
    *reinterpret_cast<f32x4*>(dx + row * C + c) = o;
}

// per-image column sums of p (* q): [B][rows][C] -> out [B][C].  One block = 64 channels (16 quads) x 16 row lanes of one row slab of one
// image: 16-byte loads, four rows in flight per thread, the sixteen row lanes and then the S slabs added in a fixed order (round 5: the
// scalar four-lane form of rounds 2-4 streamed a 25600 x 112 map through TWO blocks -- 33 us per call at one image per step, and the
// product went through a separate launch and a workspace round trip).  S > 1: slab sums to part [S][B][C], k_colsum_seg_fin adds them.
template <bool HASQ>
__global__ __launch_bounds__(256) void k_colsum_seg(const float* __restrict__ p, const float* __restrict__ q, int rows, int C, float scale,
                                                    float* __restrict__ out, int per, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float red[16][64];
    const int cq = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c = blockIdx.x * 64 + cq * 4, b = blockIdx.y, S = gridDim.z, B = gridDim.y;
    const int r0 = blockIdx.z * per, r1 = min(rows, r0 + per);
    const float* pb = p + (size_t)b * rows * C + c;
    const float* qb = HASQ ? q + (size_t)b * rows * C + c : nullptr;
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0;
    if (c < C) {
        int r = r0 + rl;
        for (; r + 48 < r1; r += 64) {
            f32x4 v0 = *reinterpret_cast<const f32x4*>(pb + (size_t)r * C), v1 = *reinterpret_cast<const f32x4*>(pb + (size_t)(r + 16) * C);
            f32x4 v2 = *reinterpret_cast<const f32x4*>(pb + (size_t)(r + 32) * C), v3 = *reinterpret_cast<const f32x4*>(pb + (size_t)(r + 48) * C);
            if (HASQ) {
                v0 *= *reinterpret_cast<const f32x4*>(qb + (size_t)r * C); v1 *= *reinterpret_cast<const f32x4*>(qb + (size_t)(r + 16) * C);
                v2 *= *reinterpret_cast<const f32x4*>(qb + (size_t)(r + 32) * C); v3 *= *reinterpret_cast<const f32x4*>(qb + (size_t)(r + 48) * C);
            }
            a0 += v0; a1 += v1; a2 += v2; a3 += v3;
        }
        for (; r < r1; r += 16) {
            f32x4 v0 = *reinterpret_cast<const f32x4*>(pb + (size_t)r * C);
            if (HASQ) v0 *= *reinterpret_cast<const f32x4*>(qb + (size_t)r * C);
            a0 += v0;
        }
    }
    *reinterpret_cast<f32x4*>(&red[rl][cq * 4]) = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (threadIdx.x < 64) {
        const int cc = blockIdx.x * 64 + threadIdx.x;
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) sum += red[k][threadIdx.x];
        if (cc < C) {
            if (S == 1) out[(size_t)b * C + cc] = sum * scale;
            else part[((size_t)blockIdx.z * B + b) * C + cc] = sum;
        }
    }
}
__global__ __launch_bounds__(256) void k_colsum_seg_fin(const float* __restrict__ part, int S, int n, float scale, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float sum = 0.f;
    for (int z = 0; z < S; ++z) sum += part[(size_t)z * n + i];
    out[i] = sum * scale;
}

// out[b][row][c] = x[b][row][c] * s[b][c] + v[b][c]   (v may be NULL)
__global__ __launch_bounds__(256) void k_scale_add(const float* __restrict__ x, const float* __restrict__ sc, const float* __restrict__ v,
                                                   int B, int rows, int C, float* __restrict__ out) {
    const int c4n = C / 4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * rows * c4n) return;
    const int c = (int)(i % c4n) * 4;
    const int b = (int)(i / ((long long)rows * c4n));
    f32x4 o = reinterpret_cast<const f32x4*>(x)[i] * *reinterpret_cast<const f32x4*>(sc + (size_t)b * C + c);
    if (v) o += *reinterpret_cast<const f32x4*>(v + (size_t)b * C + c);
    reinterpret_cast<f32x4*>(out)[i] = o;
}

// MaxPool2d(3, 2, ceil_mode=True) backward: the first maximum in (ky, kx) scan order owns the window (ATen's max_pool2d)
__global__ __launch_bounds__(256) void k_maxpool_bwd(const float* __restrict__ x, const float* __restrict__ dy, int B, int H, int W, int Ho,
                                                     int Wo, int C, float* __restrict__ dx) {
    const int c4n = C / 4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * H * W * c4n) return;
    const int c = (int)(i % c4n) * 4;
    long long t = i / c4n;
    const int xq = (int)(t % W); t /= W;
    const int yq = (int)(t % H);
    const int b = (int)(t / H);
    const float* xb = x + (size_t)b * H * W * C;
    const f32x4 me = *reinterpret_cast<const f32x4*>(xb + ((size_t)yq * W + xq) * C + c);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int oy0 = max(0, (yq - 1) / 2), oy1 = min(Ho - 1, yq / 2), ox0 = max(0, (xq - 1) / 2), ox1 = min(Wo - 1, xq / 2);
    for (int oy = oy0; oy <= oy1; ++oy)
        for (int ox = ox0; ox <= ox1; ++ox) {
            if (oy * 2 > yq || oy * 2 + 2 < yq || ox * 2 > xq || ox * 2 + 2 < xq) continue;
            // is (yq, xq) the first maximum of window (oy, ox)?
            bool own[4] = {true, true, true, true};
            for (int ky = 0; ky < 3; ++ky)
                for (int kx = 0; kx < 3; ++kx) {
                    const int yy = oy * 2 + ky, xx = ox * 2 + kx;
                    if (yy >= H || xx >= W || (yy == yq && xx == xq)) continue;
                    const f32x4 o = *reinterpret_cast<const f32x4*>(xb + ((size_t)yy * W + xx) * C + c);
                    const bool before = yy < yq || (yy == yq && xx < xq);
#pragma unroll
                    for (int k = 0; k < 4; ++k) own[k] = own[k] && (before ? o[k] < me[k] : o[k] <= me[k]);
                }
            const f32x4 g = *reinterpret_cast<const f32x4*>(dy + (((size_t)b * Ho + oy) * Wo + ox) * C + c);
#pragma unroll
            for (int k = 0; k < 4; ++k) if (own[k]) acc[k] += g[k];
        }
    reinterpret_cast<f32x4*>(dx)[i] = acc;
}

// out[b][y][x][c] = sum of the (up to) 2x2 block of in[b][2y..2y+1][2x..2x+1][c]: backward of nearest-2x upsample (cropped to H x W)
__global__ __launch_bounds__(256) void k_sumpool2(const float* __restrict__ in, int ld, int B, int H, int W, int C, float* __restrict__ out) {
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2, c4n = C / 4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * Ho * Wo * c4n) return;
    const int c = (int)(i % c4n) * 4;
    long long t = i / c4n;
    const int ox = (int)(t % Wo); t /= Wo;
    const int oy = (int)(t % Ho);
    const int b = (int)(t / Ho);
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int dy = 0; dy < 2; ++dy)
        for (int dx = 0; dx < 2; ++dx) {
            const int y = oy * 2 + dy, x = ox * 2 + dx;
            if (y < H && x < W) s += *reinterpret_cast<const f32x4*>(in + (((size_t)b * H + y) * W + x) * ld + c);
        }
    reinterpret_cast<f32x4*>(out)[i] = s;
}

}  // namespace

extern "C" int ore_pack_conv_weight_fwd(const float* w_oihw, int32_t Cout, int32_t Cin, int32_t kh, int32_t kw, int32_t dgrad,
                                        float* dst, void* stream) {
    ORE_CHECK_ARG(w_oihw && dst && Cout > 0 && Cin > 0 && kh > 0 && kw > 0, "ore_pack_conv_weight_fwd: bad args");
    const int Co16 = round_up(Cout, 16), Ci16 = round_up(Cin, 16);
    ORE_CHECK_ARG(dgrad || Cin % 16 == 0, "ore_pack_conv_weight_fwd: forward layout needs Cin %% 16 == 0");
    const long long total = dgrad ? (long long)Ci16 * kh * kw * Co16 : (long long)Co16 * kh * kw * Cin;
    hipLaunchKernelGGL(k_pack_weight, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w_oihw, Cout, Cin, kh, kw,
                       dgrad ? 1 : 0, dst, total);
    return ore_launch_status("k_pack_weight");
}

extern "C" int ore_pack_conv_weights_multi_fwd(const ore_pack_job* jobs_dev, int32_t n_jobs, int64_t total, void* stream) {
    ORE_CHECK_ARG(jobs_dev && n_jobs >= 1 && n_jobs <= 256 && total >= 1 && total < (1ll << 38), "ore_pack_conv_weights_multi_fwd: 1..256 jobs");
    hipLaunchKernelGGL(k_pack_weight_multi, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, jobs_dev, n_jobs,
                       (long long)total);
    return ore_launch_status("k_pack_weight_multi");
}

extern "C" int ore_relu_affine_bwd(const float* dy, int32_t dy_ld, int32_t dy_coff, const float* y, int32_t y_ld, int32_t y_coff,
                                   const float* scale, int64_t rows, int32_t C, float* dz, int32_t dz_ld, int32_t dz_coff, void* stream) {
    ORE_CHECK_ARG(dy && y && dz && rows > 0 && C > 0 && C % 4 == 0 && dy_ld % 4 == 0 && y_ld % 4 == 0 && dz_ld % 4 == 0 &&
                  dy_coff % 4 == 0 && y_coff % 4 == 0 && dz_coff % 4 == 0, "ore_relu_affine_bwd: bad args (channels multiple of 4)");
    const long long n = rows * (C / 4);
    hipLaunchKernelGGL(k_relu_affine_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, dy_ld, dy_coff, y, y_ld,
                       y_coff, scale, (long long)rows, C, dz, dz_ld, dz_coff);
    return ore_launch_status("k_relu_affine_bwd");
}

extern "C" int ore_colsum_segments_fwd(const float* x, int32_t ld, int32_t coff, int32_t segments, int64_t rows_per_segment, int32_t C,
                                       float beta, float* out, float* workspace, size_t workspace_floats, void* stream) {
    ORE_CHECK_ARG(x && out && workspace && segments > 0 && rows_per_segment > 0 && C > 0, "ore_colsum_segments_fwd: bad args");
    const long long cps = (rows_per_segment + CS_ROWS - 1) / CS_ROWS;
    if ((size_t)(cps * segments * C) > workspace_floats) { ore_set_error("ore_colsum_segments_fwd: workspace too small"); return ORE_ENOMEM; }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_colsum_chunks, dim3((unsigned)(cps * segments), ceil_div(C, 64)), dim3(256), 0, st, x, ld, coff, (long long)rows_per_segment,
                       (int)cps, C, workspace);
    int rc = ore_launch_status("k_colsum_chunks");
    if (rc) return rc;
    hipLaunchKernelGGL(k_colsum_final, dim3(ceil_div(C, 64), segments), dim3(256), 0, st, workspace, (int)cps, C, beta, out);
    return ore_launch_status("k_colsum_final");
}

extern "C" int ore_colsum_fwd(const float* x, int32_t ld, int32_t coff, int64_t rows, int32_t C, float beta, float* out,
                              float* workspace, size_t workspace_floats, void* stream) {
    return ore_colsum_segments_fwd(x, ld, coff, 1, rows, C, beta, out, workspace, workspace_floats, stream);
}

static int corr_fill(CorrT& p, const float* q, int q_ld, int q_coff, int B, int H, int W, int C, const float* k11, const float* k13,
                     const float* k31, int k_per_image) {
    p.q = q; p.q_ld = q_ld; p.q_coff = q_coff; p.H = H; p.W = W; p.C4 = C / 4; p.rows = B * H * W;
    p.k11 = k11; p.k13 = k13; p.k31 = k31; p.kps = k_per_image ? 1 : 0;
    return ceil_div(p.rows * p.C4, 256);
}

extern "C" int ore_correlation_train_fwd(const float* q, int32_t q_ld, int32_t q_coff, int32_t B, int32_t H, int32_t W, int32_t C,
                                         const float* k11, const float* k13, const float* k31, int32_t k_per_image, float* cat2c,
                                         float* t_save, float* u_save, void* stream) {
    ORE_CHECK_ARG(q && k11 && k13 && k31 && cat2c && t_save && u_save && B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && q_ld % 4 == 0 &&
                  q_coff % 4 == 0, "ore_correlation_train_fwd: bad args");
    CorrT p{};
    const int nb = corr_fill(p, q, q_ld, q_coff, B, H, W, C, k11, k13, k31, k_per_image);
    hipLaunchKernelGGL(k_corr_fwd_train, dim3(nb), dim3(256), 0, (hipStream_t)stream, p, cat2c, t_save, u_save);
    return ore_launch_status("k_corr_fwd_train");
}

extern "C" int ore_correlation_train_bwd(const float* q, int32_t q_ld, int32_t q_coff, int32_t B, int32_t H, int32_t W, int32_t C,
                                         const float* k11, const float* k13, const float* k31, int32_t k_per_image,
                                         const float* dcat2c, const float* t_save, const float* u_save, float* dq, float* dk_7c,
                                         float* workspace, size_t workspace_floats, void* stream) {
    ORE_CHECK_ARG(q && k11 && k13 && k31 && dcat2c && t_save && u_save && dq && dk_7c && workspace && B > 0 && H > 0 &&
                  W > 0 && C > 0 && C % 4 == 0 && q_ld % 4 == 0 && q_coff % 4 == 0, "ore_correlation_train_bwd: bad args");
    const size_t rows = (size_t)B * H * W;
    const int segs = k_per_image ? B : 1;
    const size_t rps = rows / segs;
    const size_t need = rows * C * 8 + (size_t)segs * ((rps + CS_ROWS - 1) / CS_ROWS) * 7 * C;
    if (workspace_floats < need) { ore_set_error("ore_correlation_train_bwd: workspace %zu < %zu floats", workspace_floats, need); return ORE_ENOMEM; }
    float* DT = workspace; float* P = DT + rows * C;
    float* cs = P + rows * 7 * C;
    const size_t cs_floats = workspace_floats - rows * C * 8;
    CorrT p{};
    const int nb = corr_fill(p, q, q_ld, q_coff, B, H, W, C, k11, k13, k31, k_per_image);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_corr_bwd_a, dim3(nb), dim3(256), 0, st, p, dcat2c, t_save, u_save, DT, P);
    int rc = ore_launch_status("k_corr_bwd_a");
    if (rc) return rc;
    hipLaunchKernelGGL(k_corr_bwd_b, dim3(nb), dim3(256), 0, st, p, dcat2c, DT, dq, P);
    rc = ore_launch_status("k_corr_bwd_b");
    if (rc) return rc;
    return ore_colsum_segments_fwd(P, 7 * C, 0, segs, (int64_t)rps, 7 * C, 0.f, dk_7c, cs, cs_floats, stream);
}

extern "C" int ore_groupnorm_apply_fwd(const float* x, int32_t ld, int32_t coff, int32_t images, int64_t rows_per_image, int32_t C,
                                       const float* rstd_c, const float* shift_c, const float* gamma, const float* beta, int32_t relu, float* y,
                                       void* stream) {
    ORE_CHECK_ARG(x && rstd_c && shift_c && gamma && beta && y && images > 0 && rows_per_image > 0 && C > 0 && C % 4 == 0 && ld % 4 == 0 &&
                  coff % 4 == 0, "ore_groupnorm_apply_fwd: bad args");
    const long long rows = (long long)images * rows_per_image;
    const long long n = rows * (C / 4);
    hipLaunchKernelGGL(k_gn_apply<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ld, coff, rows, (long long)rows_per_image,
                       C, rstd_c, shift_c, gamma, beta, relu, y);
    return ore_launch_status("k_gn_apply");
}

// all pyramid levels of a level-major tensor in ONE launch: segment s = level * B + image owns rows [seg_row0[s], seg_row0[s+1])
struct GnLv { int nseg; int row0[13]; };
__global__ __launch_bounds__(256) void k_gn_apply_levels_h(const ore_bf16_t* __restrict__ x, int ld, int coff, GnLv lv, int C,
                                                           const float* __restrict__ mul, const float* __restrict__ add, int relu,
                                                           ore_bf16_t* __restrict__ y) {
    const int c4n = C / 4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)lv.row0[lv.nseg] * c4n) return;
    const int row = (int)(i / c4n), c = (int)(i % c4n) * 4;
    int sgi = 0;
#pragma unroll
    for (int k = 1; k < 12; ++k)
        if (k < lv.nseg && row >= lv.row0[k]) sgi = k;
    const f32x4 v = ld4(x + (size_t)row * ld + coff + c);
    f32x4 o = v * *reinterpret_cast<const f32x4*>(mul + (size_t)sgi * C + c) + *reinterpret_cast<const f32x4*>(add + (size_t)sgi * C + c);
    if (relu) o = relu4b(o);
    st4(y + (size_t)row * C + c, o);
}

extern "C" int ore_groupnorm_apply_levels_bf16_fwd(const uint16_t* x, int32_t ld, int32_t coff, int32_t B, int32_t n_levels, const int32_t* HW,
                                                   int32_t C, const float* mul_c, const float* add_c, int32_t relu, uint16_t* y, void* stream) {
    ORE_CHECK_ARG(x && HW && mul_c && add_c && y && B > 0 && n_levels >= 1 && n_levels * B <= 12 && C > 0 && C % 4 == 0 && ld % 4 == 0 && coff % 4 == 0,
                  "ore_groupnorm_apply_levels_bf16_fwd: bad args (levels x images <= 12)");
    GnLv lv{};
    lv.nseg = n_levels * B;
    int rows = 0;
    for (int l = 0; l < n_levels; ++l)
        for (int b = 0; b < B; ++b) { lv.row0[l * B + b] = rows; rows += HW[l]; }
    lv.row0[lv.nseg] = rows;
    const long long n = (long long)rows * (C / 4);
    hipLaunchKernelGGL(k_gn_apply_levels_h, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const ore_bf16_t*)x, ld, coff, lv, C,
                       mul_c, add_c, relu, (ore_bf16_t*)y);
    return ore_launch_status("k_gn_apply_levels_h");
}

// bf16 storage: y[row][C] = act(x * mul[image] + add[image]) with the folded per-(image, channel) affine of ore_groupnorm_affine_levels_*
// (gamma / beta already inside mul / add); `images` segments of rows_per_image rows share a (mul, add) row -- level-major head tensors
// call it once per level.
extern "C" int ore_groupnorm_apply_bf16_fwd(const uint16_t* x, int32_t ld, int32_t coff, int32_t images, int64_t rows_per_image, int32_t C,
                                            const float* mul_c, const float* add_c, int32_t relu, uint16_t* y, void* stream) {
    ORE_CHECK_ARG(x && mul_c && add_c && y && images > 0 && rows_per_image > 0 && C > 0 && C % 4 == 0 && ld % 4 == 0 && coff % 4 == 0,
                  "ore_groupnorm_apply_bf16_fwd: bad args");
    const long long rows = (long long)images * rows_per_image;
    const long long n = rows * (C / 4);
    hipLaunchKernelGGL(k_gn_apply<ore_bf16_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const ore_bf16_t*)x, ld, coff,
                       rows, (long long)rows_per_image, C, mul_c, add_c, (const float*)nullptr, (const float*)nullptr, relu, (ore_bf16_t*)y);
    return ore_launch_status("k_gn_apply");
}

extern "C" int ore_groupnorm_bwd(const float* dy, const float* y, const float* x, int32_t ld, int32_t coff, int32_t images,
                                 int64_t rows_per_image, int32_t C, int32_t groups, const float* rstd_c, const float* shift_c,
                                 const float* gamma, int32_t relu, float* dx, float* dbeta_dgamma_2c, float* workspace, size_t workspace_floats,
                                 void* stream) {
    ORE_CHECK_ARG(dy && y && x && rstd_c && shift_c && gamma && dx && dbeta_dgamma_2c && workspace && images > 0 && rows_per_image > 0 && C > 0 &&
                  C % 4 == 0 && groups > 0 && C % groups == 0 && ld % 4 == 0 && coff % 4 == 0, "ore_groupnorm_bwd: bad args");
    const long long rows = (long long)images * rows_per_image;
    const size_t need = (size_t)rows * 2 * C + (size_t)images * ((rows_per_image + CS_ROWS - 1) / CS_ROWS) * 2 * C;
    if (workspace_floats < need) { ore_set_error("ore_groupnorm_bwd: workspace %zu < %zu floats", workspace_floats, need); return ORE_ENOMEM; }
    float* P = workspace;
    float* cs = P + (size_t)rows * 2 * C;
    const long long n = rows * (C / 4);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_gn_bwd_prod, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dy, y, x, ld, coff, rows, (long long)rows_per_image, C,
                       rstd_c, shift_c, relu, P);
    int rc = ore_launch_status("k_gn_bwd_prod");
    if (rc) return rc;
    if ((rc = ore_colsum_segments_fwd(P, 2 * C, 0, images, rows_per_image, 2 * C, 0.f, dbeta_dgamma_2c, cs,
                                      workspace_floats - (size_t)rows * 2 * C, stream))) return rc;
    hipLaunchKernelGGL(k_gn_bwd_dx, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dy, y, x, ld, coff, rows, (long long)rows_per_image, C,
                       C / groups, rstd_c, shift_c, gamma, dbeta_dgamma_2c, relu, dx);
    return ore_launch_status("k_gn_bwd_dx");
}

// ---------------------------------------------------------------------------------------------------------------------------
// SM_Block glue (ref:fewx/modeling/fsod/fsod_cen.py:584-630, training): the H- and W-mixing Linears see the map with (segment, the
// other axis) as rows and (mixed axis, S channels) as K.  In memory that is a transpose of 16-byte granules -- for a fixed (image,
// other-axis index) an [A x Bc] matrix of S-float granules becomes [Bc x A] -- which ATen runs element by element at ~1.3 TB/s.
// One block moves one such matrix through LDS: reads and writes are both whole granule rows (512 B at 128 channels).
__global__ __launch_bounds__(256) void k_granule_transpose(const float* __restrict__ in, float* __restrict__ out, int nb2, int A, int Bc,
                                                           int S4, long long in_b1, long long in_b2, long long in_rs, long long out_b1,
                                                           long long out_b2, long long out_rs, int accumulate) {
    extern __shared__ __attribute__((aligned(16))) float gt[];    // [A][Bc * S4 + 1] granules of 4 floats (odd pitch: column reads spread)
    const int b1 = blockIdx.x / nb2, b2 = blockIdx.x - b1 * nb2;
    const int row = Bc * S4, pitch = row + 1, n = A * row;
    const float* src = in + b1 * in_b1 + b2 * in_b2;
    float* dst = out + b1 * out_b1 + b2 * out_b2;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int r = i / row, cs = i - r * row;
        *reinterpret_cast<f32x4*>(gt + (size_t)(r * pitch + cs) * 4) = *reinterpret_cast<const f32x4*>(src + r * in_rs + cs * 4);
    }
    __syncthreads();
    const int orow = A * S4;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int c = i / orow, rs = i - c * orow;
        const int r = rs / S4, s4 = rs - r * S4;
        f32x4 v = *reinterpret_cast<const f32x4*>(gt + (size_t)(r * pitch + c * S4 + s4) * 4);
        if (accumulate) v += *reinterpret_cast<const f32x4*>(dst + c * out_rs + rs * 4);   // out += transposed(in): the second of two gradients
        *reinterpret_cast<f32x4*>(dst + c * out_rs + rs * 4) = v;
    }
}

// y = w * a0[b][c] + h * a1[b][c]  (the re-weighted sum of the two mixed maps); backward: dw = dy * a0 + v, dh = dy * a1 + v with the
// optional per-(image, channel) constant v (the gradient of the mean pool that fed the re-weighting MLP)
__global__ __launch_bounds__(256) void k_combine2(const float* __restrict__ w, const float* __restrict__ h, const float* __restrict__ a0,
                                                  const float* __restrict__ a1, int B, int rows, int C, float* __restrict__ y) {
    const int c4n = C / 4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * rows * c4n) return;
    const int c = (int)(i % c4n) * 4;
    const int b = (int)(i / ((long long)rows * c4n));
    reinterpret_cast<f32x4*>(y)[i] = reinterpret_cast<const f32x4*>(w)[i] * *reinterpret_cast<const f32x4*>(a0 + (size_t)b * C + c) +
                                     reinterpret_cast<const f32x4*>(h)[i] * *reinterpret_cast<const f32x4*>(a1 + (size_t)b * C + c);
}
__global__ __launch_bounds__(256) void k_combine2_bwd(const float* __restrict__ dy, const float* __restrict__ a0, const float* __restrict__ a1,
                                                      const float* __restrict__ v, int B, int rows, int C, float* __restrict__ dw,
                                                      float* __restrict__ dh) {
    const int c4n = C / 4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * rows * c4n) return;
    const int c = (int)(i % c4n) * 4;
    const int b = (int)(i / ((long long)rows * c4n));
    const f32x4 g = reinterpret_cast<const f32x4*>(dy)[i];
    f32x4 ow = g * *reinterpret_cast<const f32x4*>(a0 + (size_t)b * C + c), oh = g * *reinterpret_cast<const f32x4*>(a1 + (size_t)b * C + c);
    if (v) { const f32x4 vv = *reinterpret_cast<const f32x4*>(v + (size_t)b * C + c); ow += vv; oh += vv; }
    reinterpret_cast<f32x4*>(dw)[i] = ow;
    reinterpret_cast<f32x4*>(dh)[i] = oh;
}

// adaptive_avg_pool2d on NHWC maps (F.adaptive_avg_pool2d semantics: bin i of an axis of length L pooled to S covers
// [floor(i L / S), ceil((i + 1) L / S)) ), forward and backward, 4 channels per thread.  The support maps reach the SM_Block through it
// (30x30 -> 32x32, ref fsod_cen.py:214-227) and the support kernels are three of them (1x1, 1x3, 3x1, :229-231); ATen's path costs an
// NCHW <-> NHWC copy of the map and an atomic backward.
__device__ __forceinline__ int apool_lo(int i, int L, int S) { return (i * L) / S; }
__device__ __forceinline__ int apool_hi(int i, int L, int S) { return ((i + 1) * L + S - 1) / S; }
__global__ __launch_bounds__(256) void k_apool_fwd(const float* __restrict__ x, int B, int H, int W, int C, int OH, int OW, float* __restrict__ y) {
    const int c4n = C / 4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * OH * OW * c4n) return;
    const int c = (int)(i % c4n) * 4;
    long long t = i / c4n;
    const int ox = (int)(t % OW); t /= OW;
    const int oy = (int)(t % OH);
    const int b = (int)(t / OH);
    const int y0 = apool_lo(oy, H, OH), y1 = apool_hi(oy, H, OH), x0 = apool_lo(ox, W, OW), x1 = apool_hi(ox, W, OW);
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    for (int yy = y0; yy < y1; ++yy)
        for (int xx = x0; xx < x1; ++xx) a += *reinterpret_cast<const f32x4*>(x + ((size_t)(b * H + yy) * W + xx) * C + c);
    reinterpret_cast<f32x4*>(y)[i] = a / (float)((y1 - y0) * (x1 - x0));
}
// large bins (the 1x1 / 1x3 / 3x1 support kernels pool 11-32 rows x 32 columns each): one block per output pixel, the bin's pixels dealt
// to 256 / (C/4) slices of threads and combined through LDS in a fixed order -- a thread per output would walk ~1000 pixels alone
__global__ __launch_bounds__(256) void k_apool_fwd_big(const float* __restrict__ x, int H, int W, int C, int OH, int OW, float* __restrict__ y) {
    __shared__ __attribute__((aligned(16))) float red[256 * 4];
    const int c4n = C / 4, nsl = 256 / c4n;                     // C <= 1024
    const int q = threadIdx.x % c4n, sl = threadIdx.x / c4n;
    const int ox = blockIdx.x % OW, oy = (blockIdx.x / OW) % OH, b = blockIdx.x / (OW * OH);
    const int y0 = apool_lo(oy, H, OH), y1 = apool_hi(oy, H, OH), x0 = apool_lo(ox, W, OW), x1 = apool_hi(ox, W, OW);
    const int bw = x1 - x0, n = (y1 - y0) * bw;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    if (sl < nsl)
        for (int i = sl; i < n; i += nsl) {
            const int yy = y0 + i / bw, xx = x0 + i % bw;
            a += *reinterpret_cast<const f32x4*>(x + ((size_t)(b * H + yy) * W + xx) * C + q * 4);
        }
    *reinterpret_cast<f32x4*>(red + threadIdx.x * 4) = a;
    __syncthreads();
    if (sl == 0) {
        for (int k = 1; k < nsl; ++k) a += *reinterpret_cast<const f32x4*>(red + (k * c4n + q) * 4);
        *reinterpret_cast<f32x4*>(y + (size_t)blockIdx.x * C + q * 4) = a / (float)n;
    }
}
// gather form of the backward: input pixel (yy, xx) collects dy / |bin| from every bin that covers it (no atomics, deterministic)
__global__ __launch_bounds__(256) void k_apool_bwd(const float* __restrict__ dy, int B, int H, int W, int C, int OH, int OW, float* __restrict__ dx) {
    const int c4n = C / 4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * H * W * c4n) return;
    const int c = (int)(i % c4n) * 4;
    long long t = i / c4n;
    const int xx = (int)(t % W); t /= W;
    const int yy = (int)(t % H);
    const int b = (int)(t / H);
    // bins that can cover yy: i with floor(i H / OH) <= yy < ceil((i + 1) H / OH)  ->  i in [yy OH / H - 1, (yy + 1) OH / H]
    const int oy0 = max(0, (yy * OH) / H - 1), oy1 = min(OH - 1, ((yy + 1) * OH) / H);
    const int ox0 = max(0, (xx * OW) / W - 1), ox1 = min(OW - 1, ((xx + 1) * OW) / W);
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    for (int oy = oy0; oy <= oy1; ++oy) {
        const int y0 = apool_lo(oy, H, OH), y1 = apool_hi(oy, H, OH);
        if (yy < y0 || yy >= y1) continue;
        for (int ox = ox0; ox <= ox1; ++ox) {
            const int x0 = apool_lo(ox, W, OW), x1 = apool_hi(ox, W, OW);
            if (xx < x0 || xx >= x1) continue;
            a += *reinterpret_cast<const f32x4*>(dy + ((size_t)(b * OH + oy) * OW + ox) * C + c) / (float)((y1 - y0) * (x1 - x0));
        }
    }
    reinterpret_cast<f32x4*>(dx)[i] = a;
}
// y[g][m] = scale * sum_{n < N} x[g*N + n][m]  (the prototype = mean over an image's shots, fsod_cen.py:228);  backward: every member gets
// scale * dy[g][m]
__global__ __launch_bounds__(256) void k_group_sum(const float* __restrict__ x, int G, int N, long long M4, float scale, float* __restrict__ y) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)G * M4) return;
    const long long g = i / M4, m = i - g * M4;
    const f32x4* src = reinterpret_cast<const f32x4*>(x) + (size_t)g * N * M4 + m;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    for (int n = 0; n < N; ++n) a += src[(size_t)n * M4];
    reinterpret_cast<f32x4*>(y)[i] = a * scale;
}
__global__ __launch_bounds__(256) void k_group_bcast(const float* __restrict__ dy, int G, int N, long long M4, float scale, float* __restrict__ dx) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)G * N * M4) return;
    const long long g = i / (N * M4), m = i % M4;
    reinterpret_cast<f32x4*>(dx)[i] = reinterpret_cast<const f32x4*>(dy)[g * M4 + m] * scale;
}

extern "C" int ore_adaptive_avgpool_nhwc_fwd(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW, float* y,
                                             void* stream) {
    ORE_CHECK_ARG(x && y && B > 0 && H > 0 && W > 0 && OH > 0 && OW > 0 && C > 0 && C % 4 == 0, "ore_adaptive_avgpool_nhwc_fwd: bad args");
    const long long n = (long long)B * OH * OW * (C / 4);
    const int bin = ((H + OH - 1) / OH + 1) * ((W + OW - 1) / OW + 1);
    if (bin >= 64 && C <= 1024) {                               // few outputs, large bins: a block per output pixel
        hipLaunchKernelGGL(k_apool_fwd_big, dim3((unsigned)(B * OH * OW)), dim3(256), 0, (hipStream_t)stream, x, H, W, C, OH, OW, y);
        return ore_launch_status("k_apool_fwd_big");
    }
    hipLaunchKernelGGL(k_apool_fwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, B, H, W, C, OH, OW, y);
    return ore_launch_status("k_apool_fwd");
}
extern "C" int ore_adaptive_avgpool_nhwc_bwd(const float* dy, int32_t B, int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW, float* dx,
                                             void* stream) {
    ORE_CHECK_ARG(dy && dx && B > 0 && H > 0 && W > 0 && OH > 0 && OW > 0 && C > 0 && C % 4 == 0, "ore_adaptive_avgpool_nhwc_bwd: bad args");
    const long long n = (long long)B * H * W * (C / 4);
    hipLaunchKernelGGL(k_apool_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, B, H, W, C, OH, OW, dx);
    return ore_launch_status("k_apool_bwd");
}
extern "C" int ore_group_mean_fwd(const float* x, int32_t G, int32_t N, int64_t M, float* y, void* stream) {
    ORE_CHECK_ARG(x && y && G > 0 && N > 0 && M > 0 && M % 4 == 0, "ore_group_mean_fwd: bad args");
    const long long n = (long long)G * (M / 4);
    hipLaunchKernelGGL(k_group_sum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, G, N, (long long)(M / 4), 1.0f / (float)N, y);
    return ore_launch_status("k_group_sum");
}
extern "C" int ore_group_mean_bwd(const float* dy, int32_t G, int32_t N, int64_t M, float* dx, void* stream) {
    ORE_CHECK_ARG(dy && dx && G > 0 && N > 0 && M > 0 && M % 4 == 0, "ore_group_mean_bwd: bad args");
    const long long n = (long long)G * N * (M / 4);
    hipLaunchKernelGGL(k_group_bcast, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, G, N, (long long)(M / 4), 1.0f / (float)N, dx);
    return ore_launch_status("k_group_bcast");
}

extern "C" int ore_granule_transpose_fwd(const float* in, float* out, int32_t nb1, int32_t nb2, int32_t A, int32_t Bc, int32_t S, int64_t in_b1,
                                         int64_t in_b2, int64_t in_rs, int64_t out_b1, int64_t out_b2, int64_t out_rs, int32_t accumulate,
                                         void* stream) {
    ORE_CHECK_ARG(in && out && in != out && nb1 > 0 && nb2 > 0 && A > 0 && Bc > 0 && S > 0 && S % 4 == 0, "ore_granule_transpose_fwd: bad args");
    ORE_CHECK_ARG(in_b1 % 4 == 0 && in_b2 % 4 == 0 && in_rs % 4 == 0 && out_b1 % 4 == 0 && out_b2 % 4 == 0 && out_rs % 4 == 0,
                  "ore_granule_transpose_fwd: strides must be multiples of 4 floats");
    const size_t lds = (size_t)A * (Bc * (S / 4) + 1) * 16;
    ORE_CHECK_ARG(lds <= 64 * 1024, "ore_granule_transpose_fwd: one [A x Bc] granule matrix must fit 64 KB of LDS (A=%d Bc=%d S=%d)", A, Bc, S);
    hipLaunchKernelGGL(k_granule_transpose, dim3((unsigned)nb1 * nb2), dim3(256), lds, (hipStream_t)stream, in, out, nb2, A, Bc, S / 4,
                       (long long)in_b1, (long long)in_b2, (long long)in_rs, (long long)out_b1, (long long)out_b2, (long long)out_rs, (int)accumulate);
    return ore_launch_status("k_granule_transpose");
}

extern "C" int ore_combine2_fwd(const float* w, const float* h, const float* a0_bc, const float* a1_bc, int32_t B, int32_t rows, int32_t C,
                                float* y, void* stream) {
    ORE_CHECK_ARG(w && h && a0_bc && a1_bc && y && B > 0 && rows > 0 && C > 0 && C % 4 == 0, "ore_combine2_fwd: bad args");
    const long long n = (long long)B * rows * (C / 4);
    hipLaunchKernelGGL(k_combine2, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, h, a0_bc, a1_bc, B, rows, C, y);
    return ore_launch_status("k_combine2");
}

extern "C" int ore_combine2_bwd(const float* dy, const float* a0_bc, const float* a1_bc, const float* add_bc, int32_t B, int32_t rows, int32_t C,
                                float* dw, float* dh, void* stream) {
    ORE_CHECK_ARG(dy && a0_bc && a1_bc && dw && dh && B > 0 && rows > 0 && C > 0 && C % 4 == 0, "ore_combine2_bwd: bad args");
    const long long n = (long long)B * rows * (C / 4);
    hipLaunchKernelGGL(k_combine2_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, a0_bc, a1_bc, add_bc, B, rows, C,
                       dw, dh);
    return ore_launch_status("k_combine2_bwd");
}

extern "C" int ore_prod_colsum_fwd(const float* p, const float* q, int32_t B, int32_t rows, int32_t C, float scale, float* out_bc,
                                   float* workspace, size_t workspace_floats, void* stream) {
    ORE_CHECK_ARG(p && out_bc && workspace && B > 0 && rows > 0 && C > 0 && C % 4 == 0, "ore_prod_colsum_fwd: bad args");
    hipStream_t st = (hipStream_t)stream;
    // row slabs: enough blocks to fill the chip when one image has many rows (a 160 x 160 map of a single query image), whole
    // multiples of 64 rows, as many as the workspace holds partial sums for
    const int cb = ceil_div(C, 64);
    int S = 1;
    if (rows >= 2048) {
        S = min(ceil_div(1024, cb * B), rows / 512);
        const size_t cap = workspace_floats / ((size_t)B * C);
        if ((size_t)S > cap) S = (int)cap;
        if (S < 1) S = 1;
    }
    const int per = round_up(ceil_div(rows, S), 64);
    S = ceil_div(rows, per);
    if (q) hipLaunchKernelGGL(k_colsum_seg<true>, dim3(cb, B, S), dim3(256), 0, st, p, q, rows, C, scale, out_bc, per, workspace);
    else hipLaunchKernelGGL(k_colsum_seg<false>, dim3(cb, B, S), dim3(256), 0, st, p, q, rows, C, scale, out_bc, per, workspace);
    if (S > 1) {
        int rc = ore_launch_status("k_colsum_seg");
        if (rc) return rc;
        hipLaunchKernelGGL(k_colsum_seg_fin, dim3(ceil_div(B * C, 256)), dim3(256), 0, st, workspace, S, B * C, scale, out_bc);
    }
    return ore_launch_status("k_colsum_seg");
}

extern "C" int ore_scale_add_channels_fwd(const float* x, const float* scale_bc, const float* add_bc, int32_t B, int32_t rows, int32_t C,
                                          float* out, void* stream) {
    ORE_CHECK_ARG(x && scale_bc && out && B > 0 && rows > 0 && C > 0 && C % 4 == 0, "ore_scale_add_channels_fwd: bad args");
    const long long n = (long long)B * rows * (C / 4);
    hipLaunchKernelGGL(k_scale_add, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, scale_bc, add_bc, B, rows, C, out);
    return ore_launch_status("k_scale_add");
}

extern "C" int ore_maxpool3x3s2_bwd(const float* x, const float* dy, int32_t B, int32_t H, int32_t W, int32_t C, float* dx, void* stream) {
    ORE_CHECK_ARG(x && dy && dx && B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "ore_maxpool3x3s2_bwd: bad args");
    // ceil mode: out = ceil((H - 3) / 2) + 1, and the last window must start inside the input
    int ho = (H - 3 + 1) / 2 + 1, wo = (W - 3 + 1) / 2 + 1;
    if ((ho - 1) * 2 >= H) --ho;
    if ((wo - 1) * 2 >= W) --wo;
    const long long n = (long long)B * H * W * (C / 4);
    hipLaunchKernelGGL(k_maxpool_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, dy, B, H, W, ho, wo, C, dx);
    return ore_launch_status("k_maxpool_bwd");
}

extern "C" int ore_sumpool2x2_fwd(const float* in, int32_t ld, int32_t B, int32_t H, int32_t W, int32_t C, float* out, void* stream) {
    ORE_CHECK_ARG(in && out && B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && ld % 4 == 0 && ld >= C, "ore_sumpool2x2_fwd: bad args");
    const long long n = (long long)B * ((H + 1) / 2) * ((W + 1) / 2) * (C / 4);
    hipLaunchKernelGGL(k_sumpool2, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, ld, B, H, W, C, out);
    return ore_launch_status("k_sumpool2");
}
