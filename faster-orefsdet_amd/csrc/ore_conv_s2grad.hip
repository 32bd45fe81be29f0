// The gradients of the two stride-2 convolutions of the VoVNet stem (MODEL.BACKBONE.FREEZE_AT: 0; what torch.autograd of
// F.conv2d(stride=2, padding=1) computes inside d2z:engine/train_loop.py:279 `losses.backward()`), 3x3 / stride 2 / pad 1, Ho = (H - 1) / 2 + 1:
//   k_wgrad_s2        dW[co][ci][ky][kx] = sum_{b,oy,ox} dZ[b,oy,ox,co] * X[b,2oy+ky-1,2ox+kx-1,ci]: a 64 x 64 (co x ci) tile and the three
//                     kx taps of one kernel row per block on the fp32 MFMA, like k_wgrad3 -- but the X rows of a tap are gathered by
//                     ADDRESS (stride 2 breaks the "X rows = dZ rows shifted in flattened pixel order" of the stride-1 kernels)
//   k_dgrad_s2        dX[b,y,x,ci] = sum_{ky,kx,co} dZ[b,(y+1-ky)/2,(x+1-kx)/2,co] * W[co][ci][ky][kx] by the PARITY decomposition: the
//                     pixels of one (y mod 2, x mod 2) class form one GEMM with K = taps x Cout, taps = 1, 2, 2, 4 (2.25 per pixel
//                     instead of the 9 of zero insertion + a stride-1 conv); all four classes in one launch
//   k_pack_s2         W OIHW -> [tap][Cout][Cin], the layout k_dgrad_s2 stages its weight tiles from
//   k_stem1_wgrad<T>  the weight gradient of stem_1 straight from the raw planar image (uint8 / fp32): (x - mean) / std and the zero
//                     padding are formed as the rows are staged, dW[co][27] = [Cout x rows] x [rows x 27 (padded to 32)]
// The two weight gradients split their rows over blocks; every split writes a slab of the caller's workspace and k_wgrad_reduce<G>
// (ore_conv_wgrad.hip, through oreconv::launch_wgrad_reduce) adds the slabs in a fixed order.  No float atomics anywhere: deterministic.
// fp32 whatever ore_conv_set_precision says (ore_hip.h).  Pinned against float64 by tests/test_hip_s2grad.py (plan restated in
// tests/s2grad_ref.py).
#include "ore_conv_internal.h"
#include <algorithm>

namespace {

constexpr int SG_T = 64;          // block tile: 64 x 64
constexpr int SG_K = 16;          // K rows per step
constexpr int SG_LD = 80;         // floats per staged 64-wide row (as WG_LD of ore_conv_wgrad.hip)
constexpr int SG_BLOCKS = 1536;   // blocks aimed at per weight-gradient launch (rows are split until the grid has this many)
constexpr unsigned SG_OOB = oreconv::kOOB;

__device__ __forceinline__ f32x4 sg_load(const __amdgpu_buffer_rsrc_t& r, unsigned v) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)v, 0, 0));
}
// 0, 1 or 2 of the 16-channel tiles of a wave's 32 channels starting at c0 hold real channels
__device__ __forceinline__ int sg_live(int C, int c0) { return C - c0 > 16 ? 2 : C - c0 > 0 ? 1 : 0; }

// ---- weight gradient, 3x3 stride 2 ---------------------------------------------------------------------------------------------------
struct WgS2P {
    const float* x; int x_ld, x_coff;
    const float* dz; int dz_ld, dz_coff;
    int H, W, Ho, Wo, Cin, Cout;
    int M, chunk;                 // dZ rows (B * Ho * Wo), rows per split (multiple of SG_K)
    unsigned x_bytes, dz_bytes;   // the whole tensors (< 2^31, host-checked): a masked load takes the offset SG_OOB and returns zeros
    float* slab; long long slab_stride;   // [S][Cout][9][Cin]
    float* dw; float beta;        // S == 1: dW (OIHW) directly
};

__global__ __launch_bounds__(256) void k_wgrad_s2(WgS2P p) {
    __shared__ float sA[2][SG_K][SG_LD];        // dZ rows x co
    __shared__ float sB[2][3][SG_K][SG_LD];     // per kx: the X rows those dZ rows meet x ci
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int lr = tid >> 4, lc = (tid & 15) * 4;                 // this thread stages row lr, columns lc .. lc + 3 of every tile
    const int n_ci = (p.Cin + SG_T - 1) / SG_T;
    const int co0 = blockIdx.x * SG_T, ci0 = (blockIdx.y % n_ci) * SG_T, ky = blockIdx.y / n_ci;
    const int m_begin = blockIdx.z * p.chunk, m_end = min(p.M, m_begin + p.chunk);
    const __amdgpu_buffer_rsrc_t rz = make_rsrc(p.dz, p.dz_bytes), rx = make_rsrc(p.x, p.x_bytes);
    const bool co_ok = co0 + lc < p.Cout, ci_ok = ci0 + lc < p.Cin;
    f32x4 acc[3][2][2];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) acc[d][a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    // (image, oy, ox) of this thread's row, carried from step to step
    int m = m_begin + lr;
    int ox = m % p.Wo, oy = (m / p.Wo) % p.Ho, b = m / (p.Wo * p.Ho);
    f32x4 va, vb[3];
    auto load = [&]() {
        const bool row = m < m_end;
        va = sg_load(rz, row && co_ok ? (unsigned)(m * p.dz_ld + p.dz_coff + co0 + lc) * 4u : SG_OOB);
        const int y = 2 * oy + ky - 1, x0 = 2 * ox - 1;
        const bool yok = row && ci_ok && y >= 0 && y < p.H;
        const unsigned base = (unsigned)(((b * p.H + y) * p.W + x0) * p.x_ld + p.x_coff + ci0 + lc) * 4u;
#pragma unroll
        for (int d = 0; d < 3; ++d) vb[d] = sg_load(rx, yok && x0 + d >= 0 && x0 + d < p.W ? base + (unsigned)(d * p.x_ld) * 4u : SG_OOB);
        m += SG_K; ox += SG_K;
        while (ox >= p.Wo) { ox -= p.Wo; if (++oy == p.Ho) { oy = 0; ++b; } }
    };
    load();
    const int nm = sg_live(p.Cout, co0 + wm * 32), nn = sg_live(p.Cin, ci0 + wn * 32);
    int buf = 0;
    for (int m0 = m_begin; m0 < m_end; m0 += SG_K) {
        *reinterpret_cast<f32x4*>(&sA[buf][lr][lc]) = va;
#pragma unroll
        for (int d = 0; d < 3; ++d) *reinterpret_cast<f32x4*>(&sB[buf][d][lr][lc]) = vb[d];
        __syncthreads();
        if (m0 + SG_K < m_end) load();                             // next step's global loads fly under this step's MFMAs
        if (nm > 0 && nn > 0) {
#pragma unroll
            for (int kk = 0; kk < SG_K / 4; ++kk) {
                const int k = kk * 4 + (lane >> 4);
                float a[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) a[t] = sA[buf][k][wm * 32 + t * 16 + (lane & 15)];
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    float bb[2];
#pragma unroll
                    for (int t = 0; t < 2; ++t) bb[t] = sB[buf][d][k][wn * 32 + t * 16 + (lane & 15)];
#pragma unroll
                    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                        for (int tn = 0; tn < 2; ++tn)
                            if (tm < nm && tn < nn) acc[d][tm][tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[tm], bb[tn], acc[d][tm][tn], 0, 0, 0);
                }
            }
        }
        buf ^= 1;                                                    // the other buffer was last read two barriers ago
    }
    // D: column = lane & 15 (ci), row = (lane >> 4) * 4 + reg (co)
    float* slab = p.slab + (size_t)blockIdx.z * p.slab_stride;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const int tap = ky * 3 + d;
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) {
                const int ci = ci0 + wn * 32 + tn * 16 + (lane & 15);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int co = co0 + wm * 32 + tm * 16 + (lane >> 4) * 4 + r;
                    if (co < p.Cout && ci < p.Cin) {
                        if (p.dw) {
                            float* o = p.dw + ((size_t)co * p.Cin + ci) * 9 + tap;
                            *o = p.beta != 0.0f ? p.beta * *o + acc[d][tm][tn][r] : acc[d][tm][tn][r];
                        } else {
                            slab[((size_t)co * 9 + tap) * p.Cin + ci] = acc[d][tm][tn][r];
                        }
                    }
                }
            }
    }
}

// ---- data gradient, 3x3 stride 2: parity decomposition -------------------------------------------------------------------------------
// Class c = 0..3 holds the pixels with (y mod 2, x mod 2) = (1,1), (1,0), (0,1), (0,0) -- heaviest first.  An odd coordinate 2j + 1
// meets kernel index 0 at output j + 1 and kernel index 2 at output j; an even coordinate 2j meets kernel index 1 at output j.
struct DgS2P {
    const float* dz; int dz_ld, dz_coff;
    const float* wp;              // [9][Cout][Cin] (k_pack_s2)
    float* dx; int dx_ld, dx_coff;
    int B, H, W, Ho, Wo, Cin, Cout;
    unsigned dz_bytes, wp_bytes;
    int blk0[5];                  // blocks [blk0[c], blk0[c + 1]) along x serve class c
};

constexpr int DG_LDZ = 20;        // floats per staged dZ pixel (16 co + 4: the 16 pixels of an MFMA operand fall into distinct banks)

__global__ void k_pack_s2(const float* __restrict__ w, int Cout, int Cin, float* __restrict__ wp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 9 * Cout * Cin) return;
    const int ci = i % Cin, co = (i / Cin) % Cout, t = i / (Cin * Cout);
    wp[i] = w[((size_t)co * Cin + ci) * 9 + t];
}

__global__ __launch_bounds__(256) void k_dgrad_s2(DgS2P p) {
    __shared__ float sZ[2][SG_T][DG_LDZ];       // pixels x co
    __shared__ float sW[2][SG_K][SG_LD];        // co x ci
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    int cls = 0;
#pragma unroll
    for (int l = 1; l < 4; ++l)
        if ((int)blockIdx.x >= p.blk0[l]) cls = l;
    const int py = cls < 2 ? 1 : 0, px = (cls & 1) == 0 ? 1 : 0;
    const int Hc = (p.H - py + 1) / 2, Wc = (p.W - px + 1) / 2, Mc = p.B * Hc * Wc;
    const int r0 = ((int)blockIdx.x - p.blk0[cls]) * SG_T, ci0 = blockIdx.y * SG_T;
    const __amdgpu_buffer_rsrc_t rz = make_rsrc(p.dz, p.dz_bytes), rw = make_rsrc(p.wp, p.wp_bytes);
    // staging roles: dZ pixel sp, co quad sc; W row wr (co), ci quad wc
    const int sp = tid >> 2, sc = (tid & 3) * 4, wr = tid >> 4, wc = (tid & 15) * 4;
    const int rs = r0 + sp;
    const bool s_ok = rs < Mc;
    const int si = rs % Wc, sj = (rs / Wc) % Hc, sb = rs / (Wc * Hc);
    const bool wc_ok = ci0 + wc < p.Cin;
    const int nck = (p.Cout + SG_K - 1) / SG_K, ntx = 1 + px, nsteps = (1 + py) * ntx * nck;
    f32x4 acc[2][2];                            // [ci tile][pixel tile]
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    int tap = 0, ck = 0;                        // the step to load next: tap (ty, tx) of the class, co chunk ck
    f32x4 vz, vw;
    auto load = [&]() {
        const int ty = tap / ntx, tx = tap - ty * ntx;
        const int ky = py ? 2 * ty : 1, kx = px ? 2 * tx : 1;
        const int oy = sj + (py && ty == 0 ? 1 : 0), ox = si + (px && tx == 0 ? 1 : 0);
        const int c0 = ck * SG_K;
        const bool zok = s_ok && oy < p.Ho && ox < p.Wo && c0 + sc < p.Cout;
        vz = sg_load(rz, zok ? (unsigned)(((sb * p.Ho + oy) * p.Wo + ox) * p.dz_ld + p.dz_coff + c0 + sc) * 4u : SG_OOB);
        const bool wok = wc_ok && c0 + wr < p.Cout;
        vw = sg_load(rw, wok ? (unsigned)(((ky * 3 + kx) * p.Cout + c0 + wr) * p.Cin + ci0 + wc) * 4u : SG_OOB);
        if (++ck == nck) { ck = 0; ++tap; }
    };
    load();
    const int nn = sg_live(p.Cin, ci0 + wn * 32), nm = sg_live(Mc, r0 + wm * 32);
    int buf = 0;
    for (int s = 0; s < nsteps; ++s) {
        *reinterpret_cast<f32x4*>(&sZ[buf][sp][sc]) = vz;
        *reinterpret_cast<f32x4*>(&sW[buf][wr][wc]) = vw;
        __syncthreads();
        if (s + 1 < nsteps) load();
        if (nm > 0 && nn > 0) {
#pragma unroll
            for (int kk = 0; kk < SG_K / 4; ++kk) {
                const int k = kk * 4 + (lane >> 4);
                float a[2], bb[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) a[t] = sW[buf][k][wn * 32 + t * 16 + (lane & 15)];
#pragma unroll
                for (int t = 0; t < 2; ++t) bb[t] = sZ[buf][wm * 32 + t * 16 + (lane & 15)][k];
#pragma unroll
                for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                    for (int tm = 0; tm < 2; ++tm)
                        if (tn < nn && tm < nm) acc[tn][tm] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[tn], bb[tm], acc[tn][tm], 0, 0, 0);
            }
        }
        buf ^= 1;
    }
    // D: column = lane & 15 (pixel), row = (lane >> 4) * 4 + reg (ci): one 16-byte store per lane and tile
#pragma unroll
    for (int tm = 0; tm < 2; ++tm) {
        const int r = r0 + wm * 32 + tm * 16 + (lane & 15);
        if (r >= Mc) continue;
        const int i = r % Wc, j = (r / Wc) % Hc, b = r / (Wc * Hc);
        float* row = p.dx + ((size_t)(b * p.H + 2 * j + py) * p.W + 2 * i + px) * p.dx_ld + p.dx_coff;
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int ci = ci0 + wn * 32 + tn * 16 + (lane >> 4) * 4;
            if (ci < p.Cin) *reinterpret_cast<f32x4*>(row + ci) = acc[tn][tm];
        }
    }
}

// ---- weight gradient of stem_1 from the raw image -------------------------------------------------------------------------------------
struct St1P {
    const void* img; int B, H, W, Ho, Wo;
    float mean[3], std[3];
    const float* dz; int dz_ld, dz_coff, Cout;
    int M, chunk;
    unsigned dz_bytes;
    float* slab; long long slab_stride;   // [S][Cout][27]
    float* dw; float beta;                // S == 1: dW [Cout][27] directly
};

constexpr int S1_LD = 48;         // floats per staged row of the 32 (27 real) columns: the four k rows of an MFMA operand fall into distinct banks

template <typename T>
__global__ __launch_bounds__(256) void k_stem1_wgrad(St1P p) {
    __shared__ float sA[2][SG_K][SG_LD];        // dZ rows x co
    __shared__ float sB[2][SG_K][S1_LD];        // rows x (c, ky, kx): (img - mean) / std where the tap is inside the image, else 0
    const T* __restrict__ img = reinterpret_cast<const T*>(p.img);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = tid >> 4, lc = (tid & 15) * 4;                 // dZ staging: row lr, columns lc .. lc + 3
    const int co0 = blockIdx.x * SG_T;
    const int m_begin = blockIdx.z * p.chunk, m_end = min(p.M, m_begin + p.chunk);
    const __amdgpu_buffer_rsrc_t rz = make_rsrc(p.dz, p.dz_bytes);
    const bool co_ok = co0 + lc < p.Cout;
    // image staging: row lr, columns q0, q0 + 1 of the 32; column q = c * 9 + ky * 3 + kx
    const int q0 = (tid & 15) * 2;
    int qc[2], qdy[2], qdx[2];
    float qm[2], qs[2];
    bool qv[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int q = q0 + e;
        qv[e] = q < 27;
        const int qq = qv[e] ? q : 0;
        qc[e] = qq / 9; qdy[e] = (qq % 9) / 3 - 1; qdx[e] = qq % 3 - 1;
        qm[e] = qc[e] == 0 ? p.mean[0] : qc[e] == 1 ? p.mean[1] : p.mean[2];
        qs[e] = qc[e] == 0 ? p.std[0] : qc[e] == 1 ? p.std[1] : p.std[2];
    }
    int m = m_begin + lr;
    int ox = m % p.Wo, oy = (m / p.Wo) % p.Ho, b = m / (p.Wo * p.Ho);
    f32x4 va;
    float vx[2];
    auto load = [&]() {
        const bool row = m < m_end;
        va = sg_load(rz, row && co_ok ? (unsigned)(m * p.dz_ld + p.dz_coff + co0 + lc) * 4u : SG_OOB);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int y = 2 * oy + qdy[e], x = 2 * ox + qdx[e];
            const bool ok = row && qv[e] && y >= 0 && y < p.H && x >= 0 && x < p.W;     // beyond (H, W): the zero padding to (Hp, Wp) and the conv's own
            vx[e] = ok ? ((float)img[((size_t)(b * 3 + qc[e]) * p.H + y) * p.W + x] - qm[e]) / qs[e] : 0.f;
        }
        m += SG_K; ox += SG_K;
        while (ox >= p.Wo) { ox -= p.Wo; if (++oy == p.Ho) { oy = 0; ++b; } }
    };
    load();
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};     // this wave's 16 co x columns 0..15 / 16..31
    const bool live = co0 + wave * 16 < p.Cout;
    int buf = 0;
    for (int m0 = m_begin; m0 < m_end; m0 += SG_K) {
        *reinterpret_cast<f32x4*>(&sA[buf][lr][lc]) = va;
        *reinterpret_cast<f32x2*>(&sB[buf][lr][q0]) = f32x2{vx[0], vx[1]};
        __syncthreads();
        if (m0 + SG_K < m_end) load();
        if (live) {
#pragma unroll
            for (int kk = 0; kk < SG_K / 4; ++kk) {
                const int k = kk * 4 + (lane >> 4);
                const float a = sA[buf][k][wave * 16 + (lane & 15)];
#pragma unroll
                for (int t = 0; t < 2; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, sB[buf][k][t * 16 + (lane & 15)], acc[t], 0, 0, 0);
            }
        }
        buf ^= 1;
    }
    float* slab = p.slab + (size_t)blockIdx.z * p.slab_stride;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int q = t * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = co0 + wave * 16 + (lane >> 4) * 4 + r;
            if (co < p.Cout && q < 27) {
                if (p.dw) {
                    float* o = p.dw + (size_t)co * 27 + q;
                    *o = p.beta != 0.0f ? p.beta * *o + acc[t][r] : acc[t][r];
                } else {
                    slab[(size_t)co * 27 + q] = acc[t][r];
                }
            }
        }
    }
}

// the row split of the two weight gradients: rows are split until the grid has SG_BLOCKS blocks, a split keeps at least 128 rows
int s2_split(long long rows, int tiles) { return (int)std::max(1ll, std::min((long long)ceil_div(SG_BLOCKS, tiles), (rows + 127) / 128)); }
int wgrad_s2_tiles(int Cin, int Cout) { return ceil_div(Cout, SG_T) * ceil_div(Cin, SG_T) * 3; }
long long out_rows(int B, int H, int W) { return (long long)B * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1); }

}  // namespace

extern "C" size_t ore_conv_wgrad_s2_workspace_floats(int32_t rows, int32_t Cin, int32_t Cout) {
    if (rows <= 0 || Cin <= 0 || Cout <= 0) return 0;
    return (size_t)((long long)Cout * 9 * Cin * s2_split(rows, wgrad_s2_tiles(Cin, Cout)));
}

extern "C" int ore_conv2d_wgrad_s2_fwd(const float* x, int32_t x_ld, int32_t x_coff, const float* dz, int32_t dz_ld, int32_t dz_coff, int32_t B,
                                       int32_t H, int32_t W, int32_t Cin, int32_t Cout, float* dw_oihw, float beta, float* workspace,
                                       size_t workspace_floats, void* stream) {
    ORE_CHECK_ARG(x && dz && dw_oihw && workspace, "ore_conv2d_wgrad_s2_fwd: null pointer");
    ORE_CHECK_ARG(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "ore_conv2d_wgrad_s2_fwd: geometry");
    ORE_CHECK_ARG(Cin % 4 == 0 && Cout % 4 == 0 && x_ld % 4 == 0 && dz_ld % 4 == 0 && x_coff % 4 == 0 && dz_coff % 4 == 0 && x_coff >= 0 &&
                  dz_coff >= 0 && x_coff + Cin <= x_ld && dz_coff + Cout <= dz_ld,
                  "ore_conv2d_wgrad_s2_fwd: channel counts/offsets must be multiples of 4 and fit ld");
    const long long M = out_rows(B, H, W);
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    // the kernel addresses both tensors through 32-bit byte offsets, SG_OOB = 2^31 marks a masked load
    ORE_CHECK_ARG((long long)B * H * W * x_ld * 4 < (1ll << 31) && (M + SG_K) * dz_ld * 4 < (1ll << 31),
                  "ore_conv2d_wgrad_s2_fwd: a tensor of 2 GiB or more (%d x %d x %d x %d)", B, H, W, max(x_ld, dz_ld));
    const long long per = (long long)Cout * 9 * Cin;
    int S = s2_split(M, wgrad_s2_tiles(Cin, Cout));
    { const long long cap = (long long)(workspace_floats / (size_t)per); if (cap < S) S = (int)cap; }
    if (S < 1) { ore_set_error("ore_conv2d_wgrad_s2_fwd: workspace too small (%zu < %lld floats)", workspace_floats, per); return ORE_ENOMEM; }
    WgS2P p{};
    p.x = x; p.x_ld = x_ld; p.x_coff = x_coff; p.dz = dz; p.dz_ld = dz_ld; p.dz_coff = dz_coff;
    p.H = H; p.W = W; p.Ho = Ho; p.Wo = Wo; p.Cin = Cin; p.Cout = Cout;
    p.M = (int)M; p.chunk = round_up(ceil_div((int)M, S), SG_K);
    S = ceil_div((int)M, p.chunk);
    p.x_bytes = (unsigned)((long long)B * H * W * x_ld * 4); p.dz_bytes = (unsigned)(M * dz_ld * 4);
    p.slab = workspace; p.slab_stride = per;
    if (S == 1) { p.dw = dw_oihw; p.beta = beta; }
    ore_flop_count_add(2.0 * (double)M * Cout * Cin * 9.0);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_wgrad_s2, dim3(ceil_div(Cout, SG_T), ceil_div(Cin, SG_T) * 3, S), dim3(256), 0, st, p);
    const int rc = ore_launch_status("k_wgrad_s2");
    if (rc || S == 1) return rc;
    return oreconv::launch_wgrad_reduce(workspace, S, Cout, 9, Cin, beta, dw_oihw, per, nullptr, 0.0f, st);
}

extern "C" size_t ore_conv_dgrad_s2_workspace_floats(int32_t Cin, int32_t Cout) {
    return Cin > 0 && Cout > 0 ? (size_t)9 * Cin * Cout : 0;
}

extern "C" int ore_conv2d_dgrad_s2_fwd(const float* dz, int32_t dz_ld, int32_t dz_coff, const float* w_oihw, int32_t B, int32_t H, int32_t W,
                                       int32_t Cin, int32_t Cout, float* dx, int32_t dx_ld, int32_t dx_coff, float* workspace,
                                       size_t workspace_floats, void* stream) {
    ORE_CHECK_ARG(dz && w_oihw && dx && workspace, "ore_conv2d_dgrad_s2_fwd: null pointer");
    ORE_CHECK_ARG(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "ore_conv2d_dgrad_s2_fwd: geometry");
    ORE_CHECK_ARG(Cin % 4 == 0 && Cout % 4 == 0 && dx_ld % 4 == 0 && dz_ld % 4 == 0 && dx_coff % 4 == 0 && dz_coff % 4 == 0 && dx_coff >= 0 &&
                  dz_coff >= 0 && dx_coff + Cin <= dx_ld && dz_coff + Cout <= dz_ld,
                  "ore_conv2d_dgrad_s2_fwd: channel counts/offsets must be multiples of 4 and fit ld");
    const long long M = out_rows(B, H, W);
    ORE_CHECK_ARG((long long)B * H * W + 4 * SG_T < (1ll << 31) && M * dz_ld * 4 < (1ll << 31) && 9ll * Cin * Cout * 4 < (1ll << 31),
                  "ore_conv2d_dgrad_s2_fwd: a gradient map of 2 GiB or more, or too many pixels (%d x %d x %d)", B, H, W);
    const size_t need = (size_t)9 * Cin * Cout;
    if (workspace_floats < need) { ore_set_error("ore_conv2d_dgrad_s2_fwd: workspace too small (%zu < %zu floats)", workspace_floats, need); return ORE_ENOMEM; }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_pack_s2, dim3(ceil_div((int)need, 256)), dim3(256), 0, st, w_oihw, Cout, Cin, workspace);
    int rc = ore_launch_status("k_pack_s2");
    if (rc) return rc;
    DgS2P p{};
    p.dz = dz; p.dz_ld = dz_ld; p.dz_coff = dz_coff; p.wp = workspace; p.dx = dx; p.dx_ld = dx_ld; p.dx_coff = dx_coff;
    p.B = B; p.H = H; p.W = W; p.Ho = (H - 1) / 2 + 1; p.Wo = (W - 1) / 2 + 1; p.Cin = Cin; p.Cout = Cout;
    p.dz_bytes = (unsigned)(M * dz_ld * 4); p.wp_bytes = (unsigned)(need * 4);
    double flops = 0.0;
    p.blk0[0] = 0;
    for (int c = 0; c < 4; ++c) {
        const int py = c < 2 ? 1 : 0, px = (c & 1) == 0 ? 1 : 0;
        const long long Mc = (long long)B * ((H - py + 1) / 2) * ((W - px + 1) / 2);
        p.blk0[c + 1] = p.blk0[c] + (int)((Mc + SG_T - 1) / SG_T);
        flops += 2.0 * (double)Mc * (1 + py) * (1 + px) * Cout * Cin;
    }
    ore_flop_count_add(flops);
    hipLaunchKernelGGL(k_dgrad_s2, dim3(p.blk0[4], ceil_div(Cin, SG_T)), dim3(256), 0, st, p);
    return ore_launch_status("k_dgrad_s2");
}

extern "C" size_t ore_stem1_wgrad_workspace_floats(int32_t rows, int32_t Cout) {
    if (rows <= 0 || Cout <= 0) return 0;
    return (size_t)((long long)Cout * 27 * s2_split(rows, ceil_div(Cout, SG_T)));
}

extern "C" int ore_stem1_wgrad_fwd(const void* img, int32_t img_is_u8, int32_t B, int32_t H, int32_t W, int32_t Hp, int32_t Wp,
                                   const float* mean3_host, const float* std3_host, const float* dz, int32_t dz_ld, int32_t dz_coff,
                                   int32_t Cout, float* dw, float beta, float* workspace, size_t workspace_floats, void* stream) {
    ORE_CHECK_ARG(img && mean3_host && std3_host && dz && dw && workspace, "ore_stem1_wgrad_fwd: null pointer");
    ORE_CHECK_ARG(B > 0 && H > 0 && W > 0 && Hp >= H && Wp >= W && Hp % 2 == 0 && Wp % 2 == 0, "ore_stem1_wgrad_fwd: geometry");
    ORE_CHECK_ARG(Cout > 0 && Cout % 16 == 0 && dz_ld % 4 == 0 && dz_coff % 4 == 0 && dz_coff >= 0 && dz_coff + Cout <= dz_ld,
                  "ore_stem1_wgrad_fwd: Cout=%d ld=%d coff=%d", Cout, dz_ld, dz_coff);
    const int Ho = Hp / 2, Wo = Wp / 2;
    const long long M = (long long)B * Ho * Wo;
    ORE_CHECK_ARG((M + SG_K) * dz_ld * 4 < (1ll << 31) && (long long)B * 3 * H * W < (1ll << 31),
                  "ore_stem1_wgrad_fwd: %d images of %dx%d exceed the kernel's 32-bit indexing", B, Hp, Wp);
    const long long per = (long long)Cout * 27;
    int S = s2_split(M, ceil_div(Cout, SG_T));
    { const long long cap = (long long)(workspace_floats / (size_t)per); if (cap < S) S = (int)cap; }
    if (S < 1) { ore_set_error("ore_stem1_wgrad_fwd: workspace too small (%zu < %lld floats)", workspace_floats, per); return ORE_ENOMEM; }
    St1P p{};
    p.img = img; p.B = B; p.H = H; p.W = W; p.Ho = Ho; p.Wo = Wo;
    for (int c = 0; c < 3; ++c) { p.mean[c] = mean3_host[c]; p.std[c] = std3_host[c]; }
    p.dz = dz; p.dz_ld = dz_ld; p.dz_coff = dz_coff; p.Cout = Cout;
    p.M = (int)M; p.chunk = round_up(ceil_div((int)M, S), SG_K);
    S = ceil_div((int)M, p.chunk);
    p.dz_bytes = (unsigned)(M * dz_ld * 4);
    p.slab = workspace; p.slab_stride = per;
    if (S == 1) { p.dw = dw; p.beta = beta; }
    ore_flop_count_add(2.0 * (double)M * Cout * 27.0);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(ceil_div(Cout, SG_T), 1, S);
    if (img_is_u8) hipLaunchKernelGGL(k_stem1_wgrad<uint8_t>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(k_stem1_wgrad<float>, grid, dim3(256), 0, st, p);
    const int rc = ore_launch_status("k_stem1_wgrad");
    if (rc || S == 1) return rc;
    // the flat [Cout][27] gradient through the shared slab sum: one "tap", 27 "input channels" (Cout % 16 == 0 keeps its 4-float groups whole)
    return oreconv::launch_wgrad_reduce(workspace, S, Cout, 1, 27, beta, dw, per, nullptr, 0.0f, st);
}
