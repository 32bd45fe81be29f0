// The conv weight gradient (what torch.autograd of F.conv2d / F.linear computes for the weight and the bias inside
// d2z:engine/train_loop.py:279 `losses.backward()`; d2z:layers/wrappers.py:48-91):
//   dW[co][ky][kx][ci] = sum_rows dZ[row][co] * X[row shifted by tap][ci],   db[co] = sum_rows dZ[row][co]
// on a 64 x 64 (co x ci) tile per block.  The rows are split over blocks (blockIdx.z); every split writes its partial sums to a slab of
// the workspace and k_wgrad_reduce<G> adds the slabs in a fixed order (deterministic); an unsplit launch writes dW / db itself.
//   k_wgrad            fp32 MFMA, one tap per block (1x1 layers, Linear-over-rows, kernel sizes other than 3x3)
//   k_wgrad3           fp32 MFMA, 3x3: one block owns the three dx taps of a kernel row
//   k_wgrad_bf<K3>     the same two forms on the bf16 MFMA (ore_conv_set_precision(ORE_CONV_BF16))
//   k_wgrad_reduce<G>  the slab sum, G groups of slabs per output
// Pinned against float64 in every launch form by tests/test_hip_wgrad.py (the host dispatch restated in tests/wgrad_ref.py).
#include "ore_conv_internal.h"
#include <stdlib.h>

namespace {

struct WgradP {
    const float* x; int x_ld, x_coff;
    const float* dz; int dz_ld, dz_coff;
    int H, W, Cin, Cout, kh, kw, pad;
    int M, chunk;            // rows, rows per split (multiple of 16)
    float* slab;             // [S][Cout][taps][Cin]
    float* dw; float beta;   // S == 1: write OIHW directly (no slab, no reduce launch)
    float* db; float beta_b; // optional bias gradient = column sums of dZ, accumulated by the blocks that stage dZ anyway (blockIdx.y == 0):
                             // slab z holds them behind its weight part (slab_stride = weight floats + Cout), S == 1 writes db directly
    long long slab_stride;
};

constexpr int WG_T = 64;     // block tile: 64 output channels x 64 input channels of one tap
constexpr int WG_K = 16;     // rows per step
constexpr int WG_LD = 80;
static_assert(WG_LD == 80, "wgrad_bias_out reuses a staging buffer with this row stride");
#ifndef ORE_WG_BLOCKS
#define ORE_WG_BLOCKS 1536
#endif
// blocks aimed at per weight-gradient launch (rows are split until the grid has this many); env ORE_WG_BLOCKS overrides the build-time
// target for A/B runs (1024 ... 3072 measured: no difference beyond noise, EXPERIMENTS.md)
static int wg_blocks() {
    static int v = 0;
    if (!v) { const char* e = getenv("ORE_WG_BLOCKS"); v = e ? atoi(e) : 0; if (v < 64) v = ORE_WG_BLOCKS; }
    return v;
}
#define WG_BLOCKS wg_blocks()

// ---- the block layer of the weight-gradient kernels (k_wgrad, k_wgrad3, k_wgrad_bf<K3>) -----------------------------------------------
// What the four launch forms share: which tile, tap and rows a block owns (wg_block), the two operands as buffer descriptors sized to
// those rows and this thread's offsets into them (WG_DESCRIPTORS, wg_z_offset / wg_x_offset, wg_step, wg_load), the image position of a
// staged row carried from step to step and the tap's validity there (wg_pos, wg_advance, WG_TAP_INSIDE, WG_MASK3), the K loop
// instantiated for the wave's live 16 x 16 tiles (wg_for_live_tiles), the slab of the split and the store of the accumulators (wg_slab,
// WG_CLEAR, WG_STORE).  What each kernel keeps: its LDS layout, its staging and MFMA loop, its masking (k_wgrad masks X, the 3x3 forms
// mask dZ), its bias reduction (16 rows of f32x4 in wgrad_bias_out, 32 rows of scalars in k_wgrad_bf).
// Functions and macros: these kernels are on the timed path, so a piece is a __forceinline__ function only where every kernel's gfx950
// code came out as it was open-coded (tools/device_asm_diff.py) and a macro elsewhere, for the reason given at CONV_WINDOW_OF_PIXEL
// (ore_conv_desc.h): a function is optimised on its own before it is inlined -- it re-associated the row sums of the descriptors, made
// selects of the short-circuit tests, and moved registers in the accumulator loops.  For the same reason the kernels copy what their
// loops use out of the WgBlock into locals, and keep the order of the statements they had.

// Which wave of the block owns which 32 x 32 quarter of the 64 x 64 tile rotates with the block index: layers whose widths are not
// multiples of 64 (96, 112, 16 ...) leave some quarters without real channels, the waves owning them issue no matrix instructions, and
// the rotation spreads those idle waves over the four SIMDs of a CU (co-resident blocks then fill the freed issue slots) instead of
// parking them all on the same two.
__device__ __forceinline__ int wg_wave() { return __builtin_amdgcn_readfirstlane((int)((threadIdx.x >> 6) + blockIdx.x + blockIdx.y + blockIdx.z) & 3); }

struct WgBlock {
    int lane;
    int wm, wn;              // this wave's 32 x 32 quarter of the tile (wg_wave)
    int co0, ci0;            // first output / input channel of the tile
    int tsel;                // blockIdx.y above the ci tiles: the tap (one-tap forms) or the kernel row 0..2 (3x3 forms)
    int dy, dx;              // the tap's offset in the image; 3x3 forms: dx = 0, the block owns dx = -1, 0, +1 of kernel row dy
    int m_begin, m_end;      // the rows of this split
};
template <bool K3>
__device__ __forceinline__ WgBlock wg_block(const WgradP& p) {
    WgBlock b;
    b.lane = threadIdx.x & 63;
    const int wave = wg_wave();
    b.wm = wave >> 1; b.wn = wave & 1;
    const int n_ci_tiles = (p.Cin + WG_T - 1) / WG_T;
    b.co0 = blockIdx.x * WG_T;
    b.ci0 = (blockIdx.y % n_ci_tiles) * WG_T;
    b.tsel = blockIdx.y / n_ci_tiles;
    b.dy = K3 ? b.tsel - 1 : b.tsel / p.kw - p.pad;
    b.dx = K3 ? 0 : b.tsel % p.kw - p.pad;
    b.m_begin = blockIdx.z * p.chunk; b.m_end = min(p.M, b.m_begin + p.chunk);
    return b;
}

// Both operands come through buffer descriptors sized to what THIS block may read: dZ rows [m_begin, m_end), X rows from the first
// row a tap can reach (m_begin + xshift, not below 0) to the last (not beyond M).  A row outside -- before the tensor, behind the
// chunk, behind the tensor -- and a column group beyond Cout / Cin (offset WG_OOB) read as zeros in hardware: no branches, no
// zero-initialised registers, and the per-step address work is one add per load.  (Byte ranges stay below 2^31: checked on the host.)
// The loop's vector instructions share the issue port with the MFMAs -- the round-4 form of the 3x3 loop spent 3.3 of them per MFMA
// and kept the matrix pipe 61 % busy.
constexpr unsigned WG_OOB = 0x80000000u;
// into x_first and the descriptors rz, rx; row_shift + col_shift: dZ row m meets X row m + row_shift + col_shift at the block's first
// tap; rows: X rows a step may read (its rows per step + 2 in the 3x3 forms; k_wgrad3 leaves one row of slack more)
#define WG_DESCRIPTORS(p, b, row_shift, col_shift, rows, x_first, rz, rx)                                        \
    {                                                                                                            \
        (x_first) = max(0, (b).m_begin + (row_shift) + (col_shift));                                             \
        const int x_last = min((p).M, (b).m_end + (row_shift) + (col_shift) + (rows));      /* exclusive */      \
        (rz) = make_rsrc((p).dz + (size_t)(b).m_begin * (p).dz_ld, (unsigned)((b).m_end - (b).m_begin) * (unsigned)(p).dz_ld * 4u); \
        (rx) = make_rsrc((p).x + (size_t)(x_first) * (p).x_ld, (unsigned)max(x_last - (x_first), 0) * (unsigned)(p).x_ld * 4u);     \
    }
// byte offsets of the first step's (row lr, column lc) of the dZ / X tile; a column group beyond Cout / Cin takes WG_OOB instead
__device__ __forceinline__ unsigned wg_z_offset(const WgradP& p, const WgBlock& b, int lr, int lc) {
    return (unsigned)(lr * p.dz_ld + p.dz_coff + b.co0 + lc) * 4u;
}
__device__ __forceinline__ unsigned wg_x_offset(const WgradP& p, const WgBlock& b, int x_row, int lc) {
    return (unsigned)(x_row * p.x_ld + p.x_coff + b.ci0 + lc) * 4u;
}
// bytes from one step's rows to the next
template <int KSTEP> __device__ __forceinline__ unsigned wg_step(int ld) { return (unsigned)(KSTEP * ld) * 4u; }
__device__ __forceinline__ f32x4 wg_load(const __amdgpu_buffer_rsrc_t& r, unsigned v) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)v, 0, 0));
}

// (x, y) of a thread's row inside its image, carried from step to step (a step advances the row by KSTEP) instead of two integer
// divisions per thread and step
__device__ __forceinline__ void wg_pos(const WgradP& p, int row, int& xq, int& yq) { xq = row % p.W; yq = (row / p.W) % p.H; }
template <int KSTEP>
__device__ __forceinline__ void wg_advance(const WgradP& p, int& xq, int& yq) {
    xq += KSTEP;
    while (xq >= p.W) { xq -= p.W; if (++yq == p.H) yq = 0; }
}
// one-tap forms: ok = tap (dy, dx) of the row at (xq, yq) reads inside the image
#define WG_TAP_INSIDE(ok, p, xq, yq, dy, dx)                                                                         \
    {                                                                                                            \
        const int ys = (yq) + (dy), xs = (xq) + (dx);                                                        \
        (ok) = ys >= 0 && ys < (p).H && xs >= 0 && xs < (p).W;                                                   \
    }
// 3x3 forms: bit 0 / 1 / 2 of msk = tap (dy, -1 / 0 / +1) of the row at (xq, yq) reads inside the image (rows behind m_end read dZ = 0: any
// mask)
#define WG_MASK3(msk, p, xq, yq, dy)                                                                                 \
    {                                                                                                            \
        const int ys = (yq) + (dy);                                                                            \
        (msk) = (ys >= 0 && ys < (p).H) ? (((xq) > 0 ? 1 : 0) | 2 | ((xq) + 1 < (p).W ? 4 : 0)) : 0;         \
    }

#define WG_CLEAR(acc, ND)                                                                                        \
    {                                                                                                            \
        _Pragma("unroll") for (int d = 0; d < (ND); ++d)                                                         \
            _Pragma("unroll") for (int a = 0; a < 2; ++a)                                                        \
                _Pragma("unroll") for (int b = 0; b < 2; ++b) (acc)[d][a][b] = f32x4{0.f, 0.f, 0.f, 0.f};        \
    }

// kloop(TM, TN) with TM x TN = the 16 x 16 tiles of this wave's 32 x 32 part that hold real channels (0, 1 or 2 of the 32 channels
// starting at c0: wg_live), as compile-time constants: a wave whose part lies beyond Cout or Cin still stages and meets the barriers,
// but issues no matrix instructions
__device__ __forceinline__ int wg_live(int C, int c0) { return C - c0 > 16 ? 2 : C - c0 > 0 ? 1 : 0; }
struct WgI0 { static constexpr int value = 0; }; struct WgI1 { static constexpr int value = 1; }; struct WgI2 { static constexpr int value = 2; };
template <class F>
__device__ __forceinline__ void wg_for_live_tiles(const WgradP& p, const WgBlock& b, F&& kloop) {
    const int nm = wg_live(p.Cout, b.co0 + b.wm * 32), nn = wg_live(p.Cin, b.ci0 + b.wn * 32);
    if (nm == 0 || nn == 0) kloop(WgI0{}, WgI0{});
    else if (nm == 2 && nn == 2) kloop(WgI2{}, WgI2{});
    else if (nm == 2) kloop(WgI2{}, WgI1{});
    else if (nn == 2) kloop(WgI1{}, WgI2{});
    else kloop(WgI1{}, WgI1{});
}

__device__ __forceinline__ float* wg_slab(const WgradP& p) { return p.slab + (size_t)blockIdx.z * p.slab_stride; }

// The accumulators acc[ND][2][2] of the ND taps tap0 .. of a layer with `taps` taps, to dW (OIHW, beta) when the rows are not split,
// else to the slab.  D: column = lane & 15 (ci), row = (lane >> 4) * 4 + reg (co)
#define WG_STORE(p, b, slab, ND, taps, tap0, acc)                                                                \
    {                                                                                                            \
        _Pragma("unroll") for (int d = 0; d < (ND); ++d) {                                                       \
            const int tap = (tap0) + d;                                                                          \
            _Pragma("unroll") for (int tm = 0; tm < 2; ++tm)                                                     \
                _Pragma("unroll") for (int tn = 0; tn < 2; ++tn) {                                               \
                    const int ci = (b).ci0 + (b).wn * 32 + tn * 16 + ((b).lane & 15);                            \
                    _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                              \
                        const int co = (b).co0 + (b).wm * 32 + tm * 16 + ((b).lane >> 4) * 4 + r;                \
                        if (co < (p).Cout && ci < (p).Cin) {                                                     \
                            if ((p).dw) {                                                                        \
                                float* o_ = (p).dw + ((size_t)co * (p).Cin + ci) * (taps) + tap;                 \
                                *o_ = (p).beta != 0.0f ? (p).beta * *o_ + (acc)[d][tm][tn][r] : (acc)[d][tm][tn][r]; \
                            } else {                                                                             \
                                (slab)[((size_t)co * (taps) + tap) * (p).Cin + ci] = (acc)[d][tm][tn][r];        \
                            }                                                                                    \
                        }                                                                                        \
                    }                                                                                            \
                }                                                                                                \
        }                                                                                                        \
    }

// column sums of the dZ rows a block staged (fp32 kernels): every thread kept the running sum of its own (row lr, columns lc..lc+3)
// loads; the 16 rows meet in LDS (one barrier, only when a bias gradient was asked for) and go to the slab's bias part, or straight to
// db when S == 1
__device__ __forceinline__ void wgrad_bias_out(const WgradP& p, float (*sA)[80], f32x4 bsum, int co0, float* slab) {
    const int tid = threadIdx.x, lr = tid >> 4, lc = (tid & 15) * 4;
    __syncthreads();                                             // the K loop's last reads of sA are done
    *reinterpret_cast<f32x4*>(&sA[lr][lc]) = bsum;
    __syncthreads();
    if (tid < 16 && co0 + lc < p.Cout) {
        f32x4 s = *reinterpret_cast<const f32x4*>(&sA[0][lc]);
#pragma unroll
        for (int r = 1; r < 16; ++r) s += *reinterpret_cast<const f32x4*>(&sA[r][lc]);
        if (p.dw) {
            float* o = p.db + co0 + lc;
            if (p.beta_b != 0.0f) s += p.beta_b * *reinterpret_cast<const f32x4*>(o);
            *reinterpret_cast<f32x4*>(o) = s;
        } else {
            *reinterpret_cast<f32x4*>(slab + (size_t)p.Cout * p.kh * p.kw * p.Cin + co0 + lc) = s;
        }
    }
}

// ---- fp32 MFMA --------------------------------------------------------------------------------------------------------------------
// One tap per block (1x1 layers, Linear-over-rows, kernel sizes other than 3x3).  The tap's validity (row of the image, column of the
// image) only exists for kernels larger than 1x1; it masks the X operand.
__global__ __launch_bounds__(256) void k_wgrad(WgradP p) {
    __shared__ float sA[2][WG_K][WG_LD];   // dZ rows x co
    __shared__ float sB[2][WG_K][WG_LD];   // X  rows x ci
    const WgBlock b = wg_block<false>(p);
    const int lane = b.lane, wm = b.wm, wn = b.wn, dy = b.dy, dx = b.dx, m_begin = b.m_begin, m_end = b.m_end;
    const int tid = threadIdx.x, lr = tid >> 4, lc = (tid & 15) * 4;     // this thread stages row lr, columns lc..lc+3 of both tiles
    f32x4 acc[1][2][2];
    WG_CLEAR(acc, 1)

    int x_first;
    __amdgpu_buffer_rsrc_t rz, rx;
    WG_DESCRIPTORS(p, b, dy * p.W, dx, WG_K, x_first, rz, rx)
    unsigned vz = b.co0 + lc < p.Cout ? wg_z_offset(p, b, lr, lc) : WG_OOB;
    unsigned vx = b.ci0 + lc < p.Cin ? wg_x_offset(p, b, m_begin + lr + dy * p.W + dx - x_first, lc) : WG_OOB;
    const unsigned step_z = wg_step<WG_K>(p.dz_ld), step_x = wg_step<WG_K>(p.x_ld);
    const bool multi = p.kh * p.kw > 1;
    int xq = 0, yq = 0;
    if (multi) wg_pos(p, m_begin + lr, xq, yq);
    auto load = [&](f32x4& va, f32x4& vb) {
        va = wg_load(rz, vz);
        bool ok = true;
        if (multi) {
            WG_TAP_INSIDE(ok, p, xq, yq, dy, dx)
            wg_advance<WG_K>(p, xq, yq);
        }
        vb = wg_load(rx, ok ? vx : WG_OOB);
        vz += step_z; vx += step_x;
    };
    f32x4 va, vb;
    load(va, vb);
    const bool do_b = p.db != nullptr && blockIdx.y == 0;
    f32x4 bsum = {0.f, 0.f, 0.f, 0.f};
    int buf = 0;
    wg_for_live_tiles(p, b, [&](auto TMc, auto TNc) {
        constexpr int TM = decltype(TMc)::value, TN = decltype(TNc)::value;
        for (int m0 = m_begin; m0 < m_end; m0 += WG_K) {
            if (do_b) bsum += va;                                  // (fp32 dZ: the bias gradient is not an MFMA operand)
            *reinterpret_cast<f32x4*>(&sA[buf][lr][lc]) = va;
            *reinterpret_cast<f32x4*>(&sB[buf][lr][lc]) = vb;
            __syncthreads();
            if (m0 + WG_K < m_end) load(va, vb);                   // next step's global loads fly under this step's MFMAs
            if constexpr (TM > 0 && TN > 0) {
#pragma unroll
                for (int kk = 0; kk < WG_K / 4; ++kk) {
                    const int k = kk * 4 + (lane >> 4);
                    float a[TM], bb[TN];
#pragma unroll
                    for (int t = 0; t < TM; ++t) a[t] = sA[buf][k][wm * 32 + t * 16 + (lane & 15)];
#pragma unroll
                    for (int t = 0; t < TN; ++t) bb[t] = sB[buf][k][wn * 32 + t * 16 + (lane & 15)];
#pragma unroll
                    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                        for (int tn = 0; tn < TN; ++tn) acc[0][tm][tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[tm], bb[tn], acc[0][tm][tn], 0, 0, 0);
                }
            }
            buf ^= 1;                                                // the other buffer was last read two barriers ago
        }
    });
    const int taps = p.kh * p.kw;
    float* slab = wg_slab(p);
    if (do_b) wgrad_bias_out(p, sA[0], bsum, b.co0, slab);
    WG_STORE(p, b, slab, 1, taps, b.tsel, acc)
}

// 3x3 variant: ONE block owns the three dx taps of one kernel row dy.  In flattened pixel order the x rows of the taps (dy, -1..+1)
// of 16 consecutive output rows are 18 consecutive rows, so a step stages dZ[16][64] and X[18][64] once and issues 48 MFMAs on them
// (k_wgrad: 16 MFMAs per staged pair) -- 2.8x fewer L2 bytes per FLOP, the limiter of k_wgrad at large M.  Taps that leave the image
// are masked on the dZ operand (per output row and dx).
__global__ __launch_bounds__(256) void k_wgrad3(WgradP p) {
    __shared__ float sA[2][WG_K][WG_LD];       // dZ rows x co
    __shared__ float sB[2][WG_K + 2][WG_LD];   // X rows (m0 + dy*W - 1 ...) x ci
    __shared__ float sMf[2][WG_K][2];          // 1 / 0: tap (dy, -1) / (dy, +1) of this output row reads inside the image row (a row whose
                                               // (dy) neighbour row leaves the image is staged as zeros: no mask for the centre tap)
    const WgBlock b = wg_block<true>(p);
    const int tid = threadIdx.x, lane = b.lane, wm = b.wm, wn = b.wn, dy = b.dy, m_begin = b.m_begin, m_end = b.m_end;
    const int lr = tid >> 4, lc = (tid & 15) * 4;
    f32x4 acc[3][2][2];
    WG_CLEAR(acc, 3)

    int x_first;
    __amdgpu_buffer_rsrc_t rz, rx;
    WG_DESCRIPTORS(p, b, dy * p.W, -1, WG_K + 3, x_first, rz, rx)
    unsigned vz = b.co0 + lc < p.Cout ? wg_z_offset(p, b, lr, lc) : WG_OOB;
    const bool ci_ok = b.ci0 + lc < p.Cin;
    unsigned vx = ci_ok ? wg_x_offset(p, b, m_begin + lr + dy * p.W - 1 - x_first, lc) : WG_OOB;
    unsigned vx2 = ci_ok && lr < 2 ? vx + wg_step<WG_K>(p.x_ld) : WG_OOB;
    const unsigned step_z = wg_step<WG_K>(p.dz_ld), step_x = wg_step<WG_K>(p.x_ld);
    int xq, yq;
    wg_pos(p, m_begin + lr, xq, yq);
    auto load = [&](f32x4& va, f32x4& vb, f32x4& vb2, int& msk) {
        va = wg_load(rz, vz);
        vb = wg_load(rx, vx);        // staged rows 0..15
        vb2 = wg_load(rx, vx2);      // staged rows 16, 17 (lr < 2)
        vz += step_z; vx += step_x; vx2 += step_x;
        WG_MASK3(msk, p, xq, yq, dy)
        wg_advance<WG_K>(p, xq, yq);
    };
    f32x4 va, vb, vb2;
    int msk;
    load(va, vb, vb2, msk);
    const bool do_b = p.db != nullptr && blockIdx.y == 0;
    f32x4 bsum = {0.f, 0.f, 0.f, 0.f};
    int buf = 0;
    wg_for_live_tiles(p, b, [&](auto TMc, auto TNc) {
        constexpr int TM = decltype(TMc)::value, TN = decltype(TNc)::value;
        for (int m0 = m_begin; m0 < m_end; m0 += WG_K) {
            if (do_b) bsum += va;
            *reinterpret_cast<f32x4*>(&sA[buf][lr][lc]) = (msk & 2) ? va : f32x4{0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<f32x4*>(&sB[buf][lr][lc]) = vb;
            if (lr < 2) *reinterpret_cast<f32x4*>(&sB[buf][WG_K + lr][lc]) = vb2;
            if ((tid & 15) == 0) { sMf[buf][lr][0] = (msk & 1) ? 1.f : 0.f; sMf[buf][lr][1] = (msk & 4) ? 1.f : 0.f; }
            __syncthreads();
            if (m0 + WG_K < m_end) load(va, vb, vb2, msk);
            if constexpr (TM > 0 && TN > 0) {
#pragma unroll
                for (int kk = 0; kk < WG_K / 4; ++kk) {
                    const int k = kk * 4 + (lane >> 4);
                    const float mL = sMf[buf][k][0], mR = sMf[buf][k][1];
                    float a[TM];
#pragma unroll
                    for (int t = 0; t < TM; ++t) a[t] = sA[buf][k][wm * 32 + t * 16 + (lane & 15)];
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        float bb[TN];
#pragma unroll
                        for (int t = 0; t < TN; ++t) bb[t] = sB[buf][k + d][wn * 32 + t * 16 + (lane & 15)];
#pragma unroll
                        for (int tm = 0; tm < TM; ++tm) {
                            // (a product with 0 / 1 instead of a select: dZ is finite where it matters -- an inf / NaN gradient row is
                            // poisoned anyway through the centre tap)
                            const float am = d == 0 ? a[tm] * mL : d == 2 ? a[tm] * mR : a[tm];
#pragma unroll
                            for (int tn = 0; tn < TN; ++tn)
                                acc[d][tm][tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(am, bb[tn], acc[d][tm][tn], 0, 0, 0);
                        }
                    }
                }
            }
            buf ^= 1;
        }
    });
    float* slab = wg_slab(p);
    if (do_b) wgrad_bias_out(p, sA[0], bsum, b.co0, slab);
    WG_STORE(p, b, slab, 3, 9, b.tsel * 3, acc)
}

// ---- bf16 MFMA weight gradient (ORE_CONV_BF16, BASELINE configs[4]; round 4) ---------------------------------------------------------
// The same tile, row split and slab reduction as k_wgrad / k_wgrad3, but the two operands travel through LDS as bf16 (rounded once,
// nearest even, as the fp32 rows are staged: half the LDS bytes) and meet on v_mfma_f32_16x16x32_bf16: ONE matrix instruction per 16 x 16
// tile and 32 rows where the fp32 kernels issue eight.  The contraction runs over ROWS, i.e. down the columns of the row-major staged
// tiles: `ds_read_b64_tr_b16` hands every lane 4 consecutive rows of its column (two reads = the 8 k of the instruction) -- the tiles are
// written as they arrive (16 contiguous bytes per thread), no transposed stores, no bank conflicts on the way in.
//   K3 = true: 3x3 / pad 1, one block owns the three dx taps of kernel row dy: X rows m0 + dy W - 1 .. m0 + dy W + 32 are staged once
//     (34 rows), tap dx reads them shifted by dx; taps that leave the image are masked on the dZ side, which is staged in three copies
//     (dZ * valid(row, dx)) so that the MFMA operand needs no per-element select;
//   K3 = false: one tap per block (1x1 layers, Linear-over-rows, other kernel sizes).
// fp32 accumulation, fp32 bias column sums of the UNROUNDED dZ -- tests/test_hip_bf16.py::test_conv_backward_bf16_vs_oracle holds the
// result to 1e-4 of the oracle's bf16 restatement.
typedef short s16x4v __attribute__((ext_vector_type(4)));
typedef short s16x8v __attribute__((ext_vector_type(8)));
constexpr int WB_K = 32;      // rows per step
constexpr int WB_LD = 72;     // bf16 per staged row: 64 + 8 (144 bytes: 16-byte aligned rows)

__device__ __forceinline__ s16x8v pack_bf16x8(f32x4 a, f32x4 b) {
    const s16x4 lo = to_bf16x4(a), hi = to_bf16x4(b);
    return s16x8v{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
// the 16 x 16 x 32 operand of one MFMA tile: 8 consecutive rows (k) of column (lane & 15), rows 8 (lane >> 4) .. + 7 of a staged tile
__device__ __forceinline__ bf16x8_t wb_frag(const short* tile_row0_col0) {
    const int lane = threadIdx.x & 63, g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
    const short* a = tile_row0_col0 + (8 * g + q) * WB_LD + 4 * pp;
    const s16x4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4v*)a);
    const s16x4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4v*)(a + 4 * WB_LD));
    const s16x8v v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8_t, v);
}

template <bool K3>
__global__ __launch_bounds__(256) void k_wgrad_bf(WgradP p) {
    constexpr int ND = K3 ? 3 : 1;                        // dZ copies (one per dx tap)
    constexpr int XR = K3 ? WB_K + 2 : WB_K;              // staged X rows
    __shared__ __attribute__((aligned(16))) short sA[2][ND][WB_K][WB_LD];
    __shared__ __attribute__((aligned(16))) short sB[2][XR][WB_LD];          // (tap dx reads rows dx .. dx + 31 of the 34)
    const WgBlock b = wg_block<K3>(p);
    const int tid = threadIdx.x, wm = b.wm, wn = b.wn, dy = b.dy, dx1 = b.dx, m_begin = b.m_begin, m_end = b.m_end;
    const int co0 = blockIdx.x * WG_T;                    // b.co0 again, for the bias sums below: from its source the compiler sees, ahead of
                                                          // inlining wg_block, that co0 + tid (tid < 64) is an OR -- the code it made before
    const int lr = tid >> 3, lc = (tid & 7) * 8;          // this thread stages row lr, columns lc .. lc + 7 of both tiles
    f32x4 acc[ND][2][2];
    WG_CLEAR(acc, ND)

    const int xshift = K3 ? dy * p.W - 1 : dy * p.W + dx1;
    int x_first;
    __amdgpu_buffer_rsrc_t rz, rx;
    WG_DESCRIPTORS(p, b, xshift, 0, WB_K + (K3 ? 2 : 0), x_first, rz, rx)
    const unsigned z0 = wg_z_offset(p, b, lr, lc), x0 = wg_x_offset(p, b, m_begin + lr + xshift - x_first, lc);
    unsigned vz0 = b.co0 + lc < p.Cout ? z0 : WG_OOB, vz1 = b.co0 + lc + 4 < p.Cout ? z0 + 16u : WG_OOB;
    unsigned vx0 = b.ci0 + lc < p.Cin ? x0 : WG_OOB, vx1 = b.ci0 + lc + 4 < p.Cin ? x0 + 16u : WG_OOB;
    const unsigned step_z = wg_step<WB_K>(p.dz_ld), step_x = wg_step<WB_K>(p.x_ld);
    unsigned vy0 = K3 && lr < 2 && vx0 != WG_OOB ? vx0 + step_x : WG_OOB, vy1 = K3 && lr < 2 && vx1 != WG_OOB ? vx1 + step_x : WG_OOB;
    const bool coords = K3 || p.kh * p.kw > 1;
    int xq = 0, yq = 0;
    if (coords) wg_pos(p, m_begin + lr, xq, yq);
    f32x4 za, zb, xa, xb, ya, yb;                          // dZ row, X row, (K3) the extra X row of threads lr < 2
    int msk = 0;
    auto load = [&](int) {
        za = wg_load(rz, vz0); zb = wg_load(rz, vz1);
        if constexpr (K3) {
            WG_MASK3(msk, p, xq, yq, dy)
            xa = wg_load(rx, vx0); xb = wg_load(rx, vx1);
            ya = wg_load(rx, vy0); yb = wg_load(rx, vy1);
            vy0 += step_x; vy1 += step_x;
        } else {
            bool xv = true;
            if (coords) WG_TAP_INSIDE(xv, p, xq, yq, dy, dx1)
            xa = wg_load(rx, xv ? vx0 : WG_OOB); xb = wg_load(rx, xv ? vx1 : WG_OOB);
        }
        if (coords) wg_advance<WB_K>(p, xq, yq);
        vz0 += step_z; vz1 += step_z; vx0 += step_x; vx1 += step_x;
    };
    load(m_begin);
    const bool do_b = p.db != nullptr && blockIdx.y == 0;
    f32x4 bs0 = {0.f, 0.f, 0.f, 0.f}, bs1 = bs0;
    int buf = 0;
    wg_for_live_tiles(p, b, [&](auto TMc, auto TNc) {
        constexpr int TM = decltype(TMc)::value, TN = decltype(TNc)::value;
        for (int m0 = m_begin; m0 < m_end; m0 += WB_K) {
            if (do_b) { bs0 += za; bs1 += zb; }
            if constexpr (K3) {
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const bool on = (msk >> d) & 1;
                    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
                    *reinterpret_cast<s16x8v*>(&sA[buf][d][lr][lc]) = pack_bf16x8(on ? za : z, on ? zb : z);
                }
                *reinterpret_cast<s16x8v*>(&sB[buf][lr][lc]) = pack_bf16x8(xa, xb);
                if (lr < 2) *reinterpret_cast<s16x8v*>(&sB[buf][WB_K + lr][lc]) = pack_bf16x8(ya, yb);
            } else {
                *reinterpret_cast<s16x8v*>(&sA[buf][0][lr][lc]) = pack_bf16x8(za, zb);
                *reinterpret_cast<s16x8v*>(&sB[buf][lr][lc]) = pack_bf16x8(xa, xb);
            }
            __syncthreads();
            if (m0 + WB_K < m_end) load(m0 + WB_K);                // next step's global loads fly under this step's MFMAs
            if constexpr (TM > 0 && TN > 0) {
#pragma unroll
                for (int d = 0; d < ND; ++d) {
                    bf16x8_t a[TM], bb[TN];
#pragma unroll
                    for (int t = 0; t < TM; ++t) a[t] = wb_frag(&sA[buf][d][0][wm * 32 + t * 16]);
#pragma unroll
                    for (int t = 0; t < TN; ++t) bb[t] = wb_frag(&sB[buf][K3 ? d : 0][wn * 32 + t * 16]);    // tap dx: the X rows shifted by d
#pragma unroll
                    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                        for (int tn = 0; tn < TN; ++tn)
                            acc[d][tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[tm], bb[tn], acc[d][tm][tn], 0, 0, 0);
                }
            }
            buf ^= 1;                                                // the other buffer was last read two barriers ago
        }
    });
    const int taps = p.kh * p.kw;
    float* slab = wg_slab(p);
    if (do_b) {                                                // column sums of the fp32 dZ rows this block staged: 32 rows meet in LDS
        __syncthreads();
        float* red = reinterpret_cast<float*>(&sA[0][0][0][0]);  // [32][64] floats = 8 KB of the 13.8+ KB staging area
        *reinterpret_cast<f32x4*>(red + lr * 64 + lc) = bs0;
        *reinterpret_cast<f32x4*>(red + lr * 64 + lc + 4) = bs1;
        __syncthreads();
        if (tid < 64 && co0 + tid < p.Cout) {
            float sacc = red[tid];
#pragma unroll
            for (int r = 1; r < 32; ++r) sacc += red[r * 64 + tid];
            if (p.dw) {
                float* ob = p.db + co0 + tid;
                *ob = p.beta_b != 0.0f ? p.beta_b * *ob + sacc : sacc;
            } else {
                slab[(size_t)p.Cout * taps * p.Cin + co0 + tid] = sacc;
            }
        }
    }
    WG_STORE(p, b, slab, ND, taps, K3 ? b.tsel * 3 : b.tsel, acc)
}

// dw_oihw[co][ci][tap] = beta * dw + sum_z slab[z][co][tap][ci].  Fixed summation order: slab z belongs to group z % G, every group is
// summed ascending by one thread, the G partial sums are added ascending (deterministic for a given S).  One thread = (4 consecutive
// ci, one group): 16-byte slab loads, G x as many loads in flight as one thread per output has -- the 1x1 layers split their rows 192-745
// ways (few tiles), and a single chain per output made their reductions 26-96 us of pure latency.
template <int G>
__global__ __launch_bounds__(256) void k_wgrad_reduce(const float* __restrict__ slab, int S, int Cout, int taps, int Cin, float beta,
                                                      float* __restrict__ dw, long long stride, float* __restrict__ db, float beta_b) {
    __shared__ __attribute__((aligned(16))) float part[256 * 4];
    constexpr int PER = 256 / G;                                  // outputs quads per block
    const long long nw = (long long)Cout * taps * Cin;
    const long long n = nw + (db ? Cout : 0);                     // the slabs' bias part follows their weight part
    const int q = threadIdx.x % PER, g = threadIdx.x / PER;
    const long long i = ((long long)blockIdx.x * PER + q) * 4;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (i < n)
        for (int z = g; z < S; z += G) s += *reinterpret_cast<const f32x4*>(slab + (size_t)z * stride + i);
    if (G > 1) {
        *reinterpret_cast<f32x4*>(part + threadIdx.x * 4) = s;
        __syncthreads();
        if (g != 0) return;
#pragma unroll
        for (int k = 1; k < G; ++k) s += *reinterpret_cast<const f32x4*>(part + (k * PER + q) * 4);
    }
    if (i >= n) return;
    if (i >= nw) {                                               // bias gradient
        float* o = db + (i - nw);
        if (beta_b != 0.0f) s += beta_b * *reinterpret_cast<const f32x4*>(o);
        *reinterpret_cast<f32x4*>(o) = s;
        return;
    }
    const int ci = (int)(i % Cin), tap = (int)((i / Cin) % taps), co = (int)(i / ((long long)Cin * taps));
    float* o = dw + ((size_t)co * Cin + ci) * taps + tap;
    if (taps == 1) {
        f32x4 v = s;
        if (beta != 0.0f) v += beta * *reinterpret_cast<const f32x4*>(o);
        *reinterpret_cast<f32x4*>(o) = v;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) o[(size_t)k * taps] = beta != 0.0f ? beta * o[(size_t)k * taps] + s[k] : s[k];
    }
}

}  // namespace

// blocks of one split: k_wgrad3 (3x3) owns the three dx taps of a kernel row per block
static int wgrad_tiles(int Cin, int Cout, int kh, int kw) {
    return ceil_div(Cout, WG_T) * ceil_div(Cin, WG_T) * (kh == 3 && kw == 3 ? 3 : kh * kw);
}
// the row split the workspace is sized for and the launch starts from: rows are split until the grid has WG_BLOCKS blocks, a split
// keeps at least 128 rows
static int wgrad_split(int rows, int Cin, int Cout, int kh, int kw) {
    return max(1, min(ceil_div(WG_BLOCKS, wgrad_tiles(Cin, Cout, kh, kw)), ceil_div(rows, 128)));
}

// The ordered slab sum of a row-split weight gradient (k_wgrad_reduce<G>), shared with ore_conv_s2grad.hip through ore_conv_internal.h
int oreconv::launch_wgrad_reduce(const float* slab, int S, int Cout, int taps, int Cin, float beta, float* dw_oihw, long long stride, float* db,
                                 float beta_b, hipStream_t st) {
    const long long pw = (long long)Cout * taps * Cin;
    // slab groups per output: enough threads to fill the chip and enough independent loads per output to hide the latency
    const long long quads = (pw + (db ? Cout : 0)) / 4;
    const int G = S >= 64 && quads <= 65536 ? 16 : S >= 16 ? 4 : 1;
    const int per_block = 256 / G;                                     // output quads per block
    void (*const reduce)(const float*, int, int, int, int, float, float*, long long, float*, float) =
        G == 1 ? k_wgrad_reduce<1> : G == 16 ? k_wgrad_reduce<16> : k_wgrad_reduce<4>;   // (instantiated, and so emitted, as <16>, <4>, <1>)
    hipLaunchKernelGGL(reduce, dim3((unsigned)((quads + per_block - 1) / per_block)), dim3(256), 0, st, slab, S, Cout, taps, Cin, beta,
                       dw_oihw, stride, db, beta_b);
    return ore_launch_status("k_wgrad_reduce");
}

extern "C" size_t ore_conv_wgrad_workspace_floats(int32_t rows, int32_t Cin, int32_t Cout, int32_t kh, int32_t kw) {
    const long long per = (long long)Cout * kh * kw * Cin + Cout;      // (+ the bias part of a slab, whether or not it is asked for)
    return (size_t)(per * wgrad_split(rows, Cin, Cout, kh, kw));
}

extern "C" int ore_conv2d_wgrad_bias_fwd(const float* x, int32_t x_ld, int32_t x_coff, const float* dz, int32_t dz_ld, int32_t dz_coff,
                                         int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t kh, int32_t kw, int32_t pad,
                                         float* dw_oihw, float beta, float* db, float beta_b, float* workspace, size_t workspace_floats,
                                         void* stream) {
    ORE_CHECK_ARG(x && dz && dw_oihw && workspace, "ore_conv2d_wgrad_fwd: null pointer");
    ORE_CHECK_ARG(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && kh > 0 && kw > 0 && kh == 2 * pad + 1 && kw == 2 * pad + 1,
                  "ore_conv2d_wgrad_fwd: stride-1 'same' convolutions only (k = 2*pad+1)");
    ORE_CHECK_ARG(Cin % 4 == 0 && Cout % 4 == 0 && x_ld % 4 == 0 && dz_ld % 4 == 0 && x_coff % 4 == 0 && dz_coff % 4 == 0 &&
                  x_coff + Cin <= x_ld && dz_coff + Cout <= dz_ld, "ore_conv2d_wgrad_fwd: channel counts/offsets must be multiples of 4 and fit ld");
    const long long M = (long long)B * H * W;
    ORE_CHECK_ARG(M < (1ll << 31), "ore_conv2d_wgrad_fwd: too many rows");
    // (the kernels address a block's rows through 32-bit buffer offsets: a chunk of rows + its halo must span less than 2^31 bytes --
    // with the <= 1536-block row split that is a tensor of several hundred GB)
    const long long pw = (long long)Cout * kh * kw * Cin;
    const long long per = pw + Cout;                                   // slab = weight part + bias part
    int S = wgrad_split((int)M, Cin, Cout, kh, kw);
    { const long long cap = (long long)(workspace_floats / (size_t)per); if (cap < S) S = (int)cap; }
    if (S < 1) { ore_set_error("ore_conv2d_wgrad_fwd: workspace too small (%zu < %lld floats)", workspace_floats, per); return ORE_ENOMEM; }
    WgradP p{};
    p.x = x; p.x_ld = x_ld; p.x_coff = x_coff; p.dz = dz; p.dz_ld = dz_ld; p.dz_coff = dz_coff;
    p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.kh = kh; p.kw = kw; p.pad = pad;
    // (the STORAGE mode (2) is an engine property, plain calls stay fp32 (ore_hip.h))
    const bool bfm = ore_conv_get_precision() == ORE_CONV_BF16;        // bf16 MFMA build: 32-row steps
    p.M = (int)M; p.chunk = round_up(ceil_div((int)M, S), bfm ? WB_K : WG_K);
    S = ceil_div((int)M, p.chunk);
    ORE_CHECK_ARG(((long long)p.chunk + 2ll * W + 64) * (long long)max(x_ld, dz_ld) * 4 < (1ll << 31),
                  "ore_conv2d_wgrad_fwd: a row split of %d rows x %d floats exceeds the 2 GiB a block addresses (give more workspace)", p.chunk, max(x_ld, dz_ld));
    p.slab = workspace; p.slab_stride = per;
    p.db = db; p.beta_b = beta_b;
    if (S == 1) { p.dw = dw_oihw; p.beta = beta; }
    ore_flop_count_add(2.0 * (double)M * Cout * Cin * kh * kw);
    hipStream_t st = (hipStream_t)stream;
    const bool k3 = kh == 3 && kw == 3;                                // one block owns the three dx taps of a kernel row
    void (*const kernel)(WgradP) = bfm ? (k3 ? k_wgrad_bf<true> : k_wgrad_bf<false>) : (k3 ? k_wgrad3 : k_wgrad);
    hipLaunchKernelGGL(kernel, dim3(ceil_div(Cout, WG_T), ceil_div(Cin, WG_T) * (k3 ? 3 : kh * kw), S), dim3(256), 0, st, p);
    int rc = ore_launch_status("k_wgrad");
    if (rc || S == 1) return rc;
    return oreconv::launch_wgrad_reduce(workspace, S, Cout, kh * kw, Cin, beta, dw_oihw, per, db, beta_b, st);
}

extern "C" int ore_conv2d_wgrad_fwd(const float* x, int32_t x_ld, int32_t x_coff, const float* dz, int32_t dz_ld, int32_t dz_coff,
                                    int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t kh, int32_t kw, int32_t pad,
                                    float* dw_oihw, float beta, float* workspace, size_t workspace_floats, void* stream) {
    return ore_conv2d_wgrad_bias_fwd(x, x_ld, x_coff, dz, dz_ld, dz_coff, B, H, W, Cin, Cout, kh, kw, pad, dw_oihw, beta, nullptr, 0.0f, workspace,
                                     workspace_floats, stream);
}
