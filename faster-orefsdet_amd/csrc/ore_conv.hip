// Implicit-GEMM NHWC convolution on the gfx950 fp32 matrix cores (v_mfma_f32_16x16x4_f32).
//
//   M = output pixels (GEMM rows, MFMA "A" side), N = Cout (MFMA "B" side: the accumulator's lane index is the
//   output channel, so NHWC stores are contiguous per 16 lanes), K = kh*kw*Cin walked tap-major in chunks of 16
//   input channels (every Cin on the path is a multiple of 16: a chunk never straddles a tap and is one 64-byte
//   run of the NHWC input).
//
// One 256-thread block owns a BM x BN output tile.  Its 4 waves are arranged WGM x WGN x WGK: WGM*WGN waves tile
// the output, WGK wave groups split every K step (BK = 16*WGK channels are staged per step, group kg consumes
// slice kg) -- the small late-stage layers (M = 400..1600 rows at batch 1) get their parallelism from K, not M.
// Per step the block stages an im2col tile A[BM][BK] (zero-filled at the border, optional per-(image,channel)
// affine+ReLU on the fly) and a weight tile B[BN][BK] through registers into LDS (row stride BK+8 floats:
// ds_read_b128 of 16 rows is bank-conflict-free), double-buffered, one barrier per step.
// Split-K across blocks (grid.z) is reduced INSIDE the launch: every slice stores its fp32 tile to a slab, an
// agent-scope release + ticket counter elects the last arriver, which acquires and sums the slabs in slice order
// (bitwise deterministic) and runs the fused epilogue.  The counters reset themselves.
//
// Fused epilogue (the contract every forward conv kernel shares: ore_conv_epilogue.h): y = acc*scale[n] + shift[n] (+ nearest-2x
// top-down add) (+ ReLU on n < relu_cout), optional per-tile column sums of y (the eSE average pool) so no extra pass over the
// activation is needed.
// Rows may span several pyramid levels (level-major), so p3/p4/p5 run as ONE launch with per-level epilogue params.
//
// Replaces F.conv2d + FrozenBatchNorm2d + ReLU / bias / Scale of the reference (see include/ore_hip.h).
#include <string.h>
#include "ore_common.h"
#include "ore_conv_epilogue.h"

namespace {
using namespace oreconv;

// 16 bytes of zeros: the source of every out-of-image / out-of-range staging load, so that the loads themselves are
// unconditional (no branch around a load => the compiler keeps them in flight behind counted vmcnt waits).
__device__ __attribute__((aligned(16))) float g_zero16[4] = {0.f, 0.f, 0.f, 0.f};

#ifdef ORE_TRACE
// Phase-timeline build (make trace -> lib/libore_hip_trace.so; tools/conv_phase_trace.py): thread 0 of every block stamps s_memtime
// at the phase boundaries of k_conv3x3_patch / k_conv_igemm into g_trace[block][64].  Never part of the product library.
__device__ unsigned long long* g_trace = nullptr;
#define ORE_TR(i) do { if (g_trace && threadIdx.x == 0 && (i) < 64) g_trace[(size_t)blockIdx.x * 64 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define ORE_TR(i) do { } while (0)
#endif

// BF: the MFMA operands are rounded to bf16 when they leave LDS (fp32 tensors in HBM and LDS, fp32 accumulation): one
// v_mfma_f32_16x16x16_bf16 takes the place of four v_mfma_f32_16x16x4_f32 (ore_conv_set_precision).
template <int BM, int BN, int WGM, int WGN, int WGK, bool AFF, bool BF = false>
__global__ __launch_bounds__(256) void k_conv_igemm(ConvP p) {
    constexpr int WM = BM / WGM, WN = BN / WGN, TM = WM / 16, TN = WN / 16;
    constexpr int BK = 16 * WGK, LD = BK + 8;   // +8: ds_read_b128 lane groups mix two k-offsets; BK+8 is conflict-free, BK+4 is 2-way
    static_assert(WGM * WGN * WGK == 4 && WM % 16 == 0 && WN % 16 == 0, "tile");
    constexpr int QPR = BK / 4;                                  // float4 per tile row
    constexpr int A_IT = (BM * QPR + 255) / 256, B_IT = (BN * QPR + 255) / 256;
    constexpr int STAGE = 2 * (BM + BN) * LD;                    // staging floats (double buffered)
    constexpr int RED = WGK > 1 ? WGK * BM * BN : 0;             // in-block K reduction scratch (all k-groups park their tiles)
    constexpr int LDSF = STAGE > RED ? STAGE : RED;
    __shared__ __attribute__((aligned(16))) float lds[LDSF + 8];
    float* As = lds;
    float* Bs = lds + 2 * BM * LD;
    int* sh_flag = reinterpret_cast<int*>(lds + LDSF);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kg = wave % WGK, wmn = wave / WGK;
    const int wm = wmn / WGN, wn = wmn % WGN;
    int bx, by;
    tile_of_block(p.xmap, bx, by);
    const int m0 = bx * BM, n0 = by * BN;
    const int nsteps = (p.nchunks + WGK - 1) / WGK;
    const int s_begin = blockIdx.z * p.steps_per_split;
    const int s_end = min(s_begin + p.steps_per_split, nsteps);
    const int cpt = p.Cin >> 4;                                  // chunks per tap

    // ---- per-thread A rows, fixed across the K loop: pointer to the (top-left tap, channel 0) element of the row's
    // receptive field, the row's image width, its segment id and a bitmask of the taps that fall inside the image.
    // Wave-private staging (PRIV): with the K dimension split over the block's 4 waves and one wave per K group, wave kg stages exactly
    // the 16-channel slice of the A and B tiles that it multiplies itself (lane -> row lane>>2 (+16 per slot), float4 lane&3 of the
    // slice).  Its LDS columns are touched by no other wave, so the K loop needs NO barrier: the four waves drift apart and cover
    // each other's load / LDS latency instead of meeting at a barrier every 64 channels.
    constexpr bool PRIV = (WGK == 4 && WGM * WGN == 1);
    static_assert(!PRIV || (BM % 16 == 0 && BN % 16 == 0 && QPR == 16), "wave-private staging: 16-row slots, 16 float4 per tile row");
    const int my_q = PRIV ? kg * 4 + (lane & 3) : tid % QPR;     // float4 slot within a tile row: the same for all float4s of a thread
    const int my_ks = my_q >> 2;
    auto slot_row = [&](int i) -> int { return PRIV ? i * 16 + (lane >> 2) : (tid + i * 256) / QPR; };
    const float* a_ptr[A_IT];
    int a_sid[A_IT], a_W[A_IT];
    unsigned a_taps[A_IT];
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
        const int f = tid + i * 256, row = slot_row(i);
        const int m = m0 + row;
        a_sid[i] = 0; a_W[i] = 0; a_taps[i] = 0u; a_ptr[i] = p.in;
        if ((PRIV || A_IT * 256 == BM * QPR || f < BM * QPR) && m < p.M) {
            int lvl, b, oy, ox;
            decode_row(p, m, lvl, b, oy, ox);
            const Lvl& L = p.lv[lvl];
            a_sid[i] = lvl * p.B + b;
            const int iy0 = oy * p.stride - p.pad, ix0 = ox * p.stride - p.pad;
            a_W[i] = L.W;
            a_ptr[i] = p.in + ((ptrdiff_t)(L.irow0 + b * L.H * L.W) + (ptrdiff_t)iy0 * L.W + ix0) * p.in_ld + p.in_coff + (my_q & 3) * 4;
            unsigned mask = 0u;
            for (int dy = 0; dy < p.kh; ++dy)
                for (int dx = 0; dx < p.kw; ++dx)
                    if ((unsigned)(iy0 + dy) < (unsigned)L.H && (unsigned)(ix0 + dx) < (unsigned)L.W) mask |= 1u << (dy * p.kw + dx);
            a_taps[i] = mask;
        }
    }
    const float* b_ptr[B_IT];
    bool b_ok[B_IT];
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
        const int f = tid + i * 256, n = n0 + slot_row(i);
        b_ok[i] = (PRIV || B_IT * 256 == BN * QPR || f < BN * QPR) && n < p.Cout16;
        b_ptr[i] = p.w + (size_t)(b_ok[i] ? n : 0) * p.K + (my_q & 3) * 4;
    }
#ifndef ORE_PF
#define ORE_PF 3
#endif
    constexpr int PF = ORE_PF;                                   // register ring depth: a load has PF K-steps to land
    constexpr int NAFF = AFF ? A_IT : 1;
    constexpr bool A_FULL = (BM * QPR) % 256 == 0, B_FULL = (BN * QPR) % 256 == 0;   // every thread stores every float4
    f32x4 ra[PF][A_IT], rb[PF][B_IT];
    f32x4 rmul[PF][NAFF], radd[PF][NAFF];                        // input affine operands travel with the data (AFF only)
    unsigned rok[PF];                                            // bit i: float4 i of the slot is a real (in-image) element

    // (dy, dx, c0) of this thread's K-slice, advanced incrementally (no divisions, no branches in the K loop).
    int n_dy, n_dx, n_c0;
    {
        const int c = s_begin * WGK + my_ks;
        const int tap = c / cpt;
        n_c0 = (c - tap * cpt) << 4;
        n_dy = tap / p.kw; n_dx = tap - n_dy * p.kw;
    }
    const float* zero = g_zero16;
    // branch-free pointer select (a ?: here is turned back into an exec-mask branch around the load by hipcc)
    auto sel = [&](bool ok, const float* ptr) -> const f32x4* {
        const uintptr_t m = (uintptr_t)0 - (uintptr_t)ok;
        return reinterpret_cast<const f32x4*>(((uintptr_t)ptr & m) | ((uintptr_t)zero & ~m));
    };
    auto gload = [&](int step, f32x4 (&ra)[A_IT], f32x4 (&rb)[B_IT], f32x4 (&rmul)[NAFF], f32x4 (&radd)[NAFF], unsigned& okm) {
        const int c = step * WGK + my_ks;
        const int dy = n_dy, dx = n_dx, c0 = n_c0;
        n_c0 += BK;
#pragma unroll
        for (int w = 0; w < WGK; ++w) {                           // BK = 16*WGK and Cin >= 16: at most WGK wraps, predicated
            const bool wrap = n_c0 >= p.Cin;
            n_c0 -= wrap ? p.Cin : 0;
            n_dx += wrap ? 1 : 0;
            const bool wy = n_dx == p.kw;
            n_dx = wy ? 0 : n_dx;
            n_dy += wy ? 1 : 0;
        }
        const bool cok = c < p.nchunks;
        const unsigned tapbit = cok ? (1u << (dy * p.kw + dx)) : 0u;
        okm = 0;
#pragma unroll
        for (int i = 0; i < A_IT; ++i) {
            const bool ok = (a_taps[i] & tapbit) != 0u;
            const float* src = a_ptr[i] + (dy * a_W[i] + dx) * p.in_ld + c0;
            ra[i] = *sel(ok, src);
            okm |= ok ? (1u << i) : 0u;
            if (AFF) {
                const int ch = a_sid[i] * p.Cin + c0 + (my_q & 3) * 4;
                rmul[i] = *sel(ok, p.in_mul + ch);
                radd[i] = *sel(ok && p.in_add != nullptr, p.in_add + ch);
            }
        }
#pragma unroll
        for (int i = 0; i < B_IT; ++i) {
            const float* src = b_ptr[i] + (c << 4);
            rb[i] = *sel(cok && b_ok[i], src);
        }
    };
    auto lstore = [&](int buf, const f32x4 (&ra)[A_IT], const f32x4 (&rb)[B_IT], const f32x4 (&rmul)[NAFF], const f32x4 (&radd)[NAFF],
                      unsigned okm) {
#pragma unroll
        for (int i = 0; i < A_IT; ++i) {
            const int f = tid + i * 256;
            f32x4 v = ra[i];
            if (AFF) {                                            // relu?(x*mul + add) on real elements only (padding stays 0)
                v = v * rmul[i] + radd[i];
                if (p.in_relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
                if (!((okm >> i) & 1u)) v = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            if (A_FULL || f < BM * QPR) *reinterpret_cast<f32x4*>(As + buf * BM * LD + slot_row(i) * LD + my_q * 4) = v;
        }
#pragma unroll
        for (int i = 0; i < B_IT; ++i) {
            const int f = tid + i * 256;
            if (B_FULL || f < BN * QPR) *reinterpret_cast<f32x4*>(Bs + buf * BN * LD + slot_row(i) * LD + my_q * 4) = rb[i];
        }
    };

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // epilogue operands fetched NOW, under the K loop's loads (a dependent global load after the last MFMA costs ~1 us of pure
    // latency on the small layers); per-level scale/shift (ep_stride != 0) keep the late path
    // The MFMA operands are swapped (weights as "A"), so accumulator (i, j) holds D^T: this lane = pixel row
    // m0 + wm*WM + i*16 + (lane&15), channels n0 + wn*WN + j*16 + (lane>>4)*4 .. +3  -> 16-byte stores.
    // Epilogue operands (scale/shift of the block's BN channels) go to LDS NOW, under the K loop's loads: a dependent global load
    // after the last MFMA costs ~1 us of pure latency on the small layers.  Per-level scale/shift (ep_stride != 0) keep the late path.
    __shared__ float sh_sc[BN], sh_sh[BN];
    const bool ep_pre = p.ep_stride == 0;
    const int cg4 = (lane >> 4) * 4;
    if (tid < BN) {
        const int n = n0 + tid;
        const bool okn = ep_pre && n < p.Cout;
        sh_sc[tid] = (okn && p.scale) ? p.scale[n] : 1.0f;
        sh_sh[tid] = (okn && p.shift) ? p.shift[n] : 0.0f;
    }
    const bool vec_ok = CONV_OUT_VEC_OK(p, false);
    // finish one accumulator vector: 4 channels of one pixel
    auto finish = [&](f32x4 a, int m, int n, f32x4& vout) -> bool {
        if (m >= p.M || n >= p.Cout) return false;
        f32x4 v;
        if (ep_pre && !p.add) {
            v = a * *reinterpret_cast<const f32x4*>(sh_sc + (n - n0)) + *reinterpret_cast<const f32x4*>(sh_sh + (n - n0));
            CONV_RELU4(v, n, p.relu_cout)
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = n + r < p.Cout ? epilogue_one<false>(p, a[r], m, n + r) : 0.0f;
        }
        float* o = p.out + (size_t)m * p.out_ld + p.out_coff + n;
        CONV_STORE4_F32(o, v, vec_ok, n, p.Cout)
        vout = v;
        return true;
    };

    const int frow = lane & 15, fk = kg * 16 + (lane >> 4) * 4;
    // one K step: (optionally) issue the loads of step st+PF into ring slot u, MFMA on LDS buffer `cur`, (optionally) park the
    // step st+1 data (ring slot u+1, in flight for two steps already) in the other LDS buffer, barrier.
#define ORE_STEP(u, st, DO_LOAD, DO_STORE)                                                                                      \
    {                                                                                                                           \
        const int cur = ((st) - s_begin) & 1;                                                                                   \
        if (DO_LOAD) gload((st) + PF, ra[u], rb[u], rmul[u], radd[u], rok[u]);                                                  \
        ORE_TR(2 + 4 * ((st) - s_begin));                                                                                       \
        f32x4 af[TM], bf[TN];                                                                                                   \
        _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                                          \
            af[i] = *reinterpret_cast<const f32x4*>(As + cur * BM * LD + (wm * WM + i * 16 + frow) * LD + fk);                  \
        _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                                          \
            bf[j] = *reinterpret_cast<const f32x4*>(Bs + cur * BN * LD + (wn * WN + j * 16 + frow) * LD + fk);                  \
        if constexpr (BF) {                                                                                                     \
            s16x4 ah[TM], bh[TN];                                                                                               \
            _Pragma("unroll") for (int i = 0; i < TM; ++i) ah[i] = to_bf16x4(af[i]);                                            \
            _Pragma("unroll") for (int j = 0; j < TN; ++j) bh[j] = to_bf16x4(bf[j]);                                            \
            _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                                      \
                _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                                  \
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(bh[j], ah[i], acc[i][j], 0, 0, 0);                    \
        } else {                                                                                                                \
            _Pragma("unroll") for (int t = 0; t < 4; ++t)                                                                       \
                _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                                  \
                    _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                              \
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[j][t], af[i][t], acc[i][j], 0, 0, 0); /* D^T */     \
        }                                                                                                                       \
        ORE_TR(3 + 4 * ((st) - s_begin));                                                                                       \
        if (DO_STORE)                                                                                                           \
            lstore(cur ^ 1, ra[((u) + 1) % PF], rb[((u) + 1) % PF], rmul[((u) + 1) % PF], radd[((u) + 1) % PF], rok[((u) + 1) % PF]); \
        ORE_TR(4 + 4 * ((st) - s_begin));                                                                                       \
        if constexpr (!PRIV) __syncthreads();                                                                                   \
        ORE_TR(5 + 4 * ((st) - s_begin));                                                                                       \
    }
    if (s_begin >= s_end) __syncthreads();                     // publishes sh_sc/sh_sh when the K loop (and its barriers) is empty
    ORE_TR(0);
    if (s_begin < s_end) {
#pragma unroll
        for (int u = 0; u < PF; ++u) gload(s_begin + u, ra[u], rb[u], rmul[u], radd[u], rok[u]);   // steps past the end load zeros
        lstore(0, ra[0], rb[0], rmul[0], radd[0], rok[0]);
        __syncthreads();                                       // (also publishes sh_sc / sh_sh)
        ORE_TR(1);
        int s0 = s_begin;
        for (; s0 + 2 * PF <= s_end; s0 += PF) {      // steady state: no branch between a load and its use -> counted vmcnt waits
#pragma unroll
            for (int u = 0; u < PF; ++u) ORE_STEP(u, s0 + u, true, true)
        }
        for (; s0 < s_end; s0 += PF) {                // tail (< 2*PF steps): loads past the end fetch the zero page, harmless
#pragma unroll
            for (int u = 0; u < PF; ++u)
                if (s0 + u < s_end) ORE_STEP(u, s0 + u, true, s0 + u + 1 < s_end)
        }
    }
#undef ORE_STEP
    ORE_TR(61);

    // ---- in-block K reduction.
    // Fast path (no cross-block split-K, no fused column sums): every k-group parks its tiles in LDS and then ALL WGK waves share
    // the epilogue -- wave kg finishes accumulator registers r = kg, kg+WGK, ... of every tile (same group order of the sum as
    // the slow path: bit-identical).  With one wave doing all the stores (slow path) the store phase of the small layers ran at a
    // quarter of the CU's wave parallelism: +3 us per launch at M=6400, +11 us at M=25600 (tools/conv_fixed_cost2.py).
    if (WGK > 1 && p.splitk <= 1 && !p.colsum) {
        constexpr int RALL = WGK * (WGM * WGN) * TM * TN * 256;
        static_assert(WGK == 1 || RALL <= LDSF, "LDS too small for the distributed K reduction");
        __syncthreads();
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
                *reinterpret_cast<f32x4*>(lds + ((kg * (WGM * WGN) + wmn) * TM * TN + i * TN + j) * 256 + lane * 4) = acc[i][j];
        __syncthreads();
        // every 16-byte item (wmn, tile, lane) is finished by exactly one of the 256 threads: 4x the store parallelism of a single wave
        constexpr int NT = (WGM * WGN) * TM * TN;                       // tiles of the block
#pragma unroll
        for (int q0 = 0; q0 < NT * 64; q0 += 256) {
            const int q = q0 + tid;
            if (q < NT * 64) {
                const int tl = q >> 6, ln = q & 63;                     // tile index ((wmn*TM + i)*TN + j), source lane
                const int j2 = tl % TN, i2 = (tl / TN) % TM, w2 = tl / (TM * TN);
                const int wm2 = w2 / WGN, wn2 = w2 % WGN;
                f32x4 a;
                CONV_SUM_WAVE_TILES(a, WGK, lds, NT, tl, ln)
                const int m = m0 + wm2 * WM + i2 * 16 + (ln & 15);
                const int n = n0 + wn2 * WN + j2 * 16 + (ln >> 4) * 4;
                f32x4 vo;
                finish(a, m, n, vo);
            }
        }
        { ORE_TR(62); return; }
    }
    // Slow path: groups kg>0 park their tiles in LDS, group 0 adds them in group order and carries on alone
    if (WGK > 1) {
        __syncthreads();
        if (kg > 0) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    *reinterpret_cast<f32x4*>(lds + (((kg - 1) * (WGM * WGN) + wmn) * TM * TN + i * TN + j) * 256 + lane * 4) = acc[i][j];
        }
        __syncthreads();
        if (kg == 0) {
#pragma unroll
            for (int g = 1; g < WGK; ++g)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] += *reinterpret_cast<const f32x4*>(lds + (((g - 1) * (WGM * WGN) + wmn) * TM * TN + i * TN + j) * 256 + lane * 4);
        }
    }

    // accumulator element (i, j, r) of this lane is row m0 + wm*WM + i*16 + (lane>>4)*4 + r, column n0 + wn*WN + j*16 + (lane&15)
    const int ntile = by * gridDim.x + bx;
    if (p.splitk > 1) {
        // ---- publish this slice's tile, elect the last arriver (cdna guide: split-K slab reducer recipe)
        float* slab = p.ws + ((size_t)ntile * p.splitk + blockIdx.z) * (BM * BN);
        if (kg == 0) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    *reinterpret_cast<f32x4*>(slab + ((wmn * TM + i) * TN + j) * 256 + lane * 4) = acc[i][j];
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const int ticket = __hip_atomic_fetch_add(p.tile_cnt + ntile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int last = ticket == p.splitk - 1;
            if (last) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(p.tile_cnt + ntile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // self-reset
            }
            *sh_flag = last;
        }
        __syncthreads();
        if (!*sh_flag) return;
        if (kg == 0) {
            const float* base = p.ws + (size_t)ntile * p.splitk * (BM * BN);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    f32x4 s = {0.f, 0.f, 0.f, 0.f};
                    for (int z = 0; z < p.splitk; ++z)
                        s += *reinterpret_cast<const f32x4*>(base + (size_t)z * (BM * BN) + ((wmn * TM + i) * TN + j) * 256 + lane * 4);
                    acc[i][j] = s;
                }
        }
    }
    if (kg != 0) {
        if (p.colsum && WGM > 1) { __syncthreads(); __syncthreads(); }   // keep barrier counts uniform (see below)
        { ORE_TR(62); return; }
    }

    // ---- fused epilogue (transposed accumulators: one pixel, 4 consecutive channels per lane and tile)
    f32x4 csum[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) csum[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int m = m0 + wm * WM + i * 16 + (lane & 15);
            const int n = n0 + wn * WN + j * 16 + cg4;
            f32x4 v;
            if (finish(acc[i][j], m, n, v)) csum[j] += v;
        }
    if (p.colsum) {
        // column sums of this tile: the 16 pixel lanes of a channel group -> xor 1, 2, 4, 8; then across the WGM waves
#pragma unroll
        for (int j = 0; j < TN; ++j) CONV_COLSUM16(csum[j])
        const bool owner = (lane & 15) == 0;                         // holds channels j*16 + cg4 .. +3
        if (WGM > 1) {
            __syncthreads();
            if (owner)
#pragma unroll
                for (int j = 0; j < TN; ++j) *reinterpret_cast<f32x4*>(lds + (wm * WGN + wn) * (TN * 16) + j * 16 + cg4) = csum[j];
            __syncthreads();
            if (wm == 0 && owner)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    f32x4 sacc = csum[j];
                    for (int w2 = 1; w2 < WGM; ++w2) sacc += *reinterpret_cast<const f32x4*>(lds + (w2 * WGN + wn) * (TN * 16) + j * 16 + cg4);
                    csum[j] = sacc;
                }
        }
        if (wm == 0 && owner)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int n = n0 + wn * WN + j * 16 + cg4 + r;
                    if (n < p.Cout16) p.colsum[(size_t)bx * p.Cout16 + n] = csum[j][r];
                }
    }
    ORE_TR(62);
}


// ------------------------------------------------------------------------------------------------------------------------
// 3x3 / stride 1 / pad 1 "patch" kernel for the large-M layers (stem_2, stage-2 layers, FPN output3, head tower).
// A block owns a TH x 16 pixel tile x 64 output channels.  Per 16 input channels it stages ONCE the (TH+2) x 18 halo patch of
// the input and the 9 x 64 x 16 weight slab into LDS, then runs all 9 taps out of LDS: 9*TM*TN*4 MFMAs (288 for TH=8) per
// barrier pair instead of 16..32, 9x fewer global A loads / address computations than the generic implicit-GEMM step.
// The next slab is prefetched into registers while the current one is being multiplied (single LDS buffer, 72 KB -> two blocks
// per CU overlap each other's staging phase).  wave w owns tile rows [w*TH/4, (w+1)*TH/4): an MFMA A fragment is one tile row of
// 16 consecutive pixels, so the tap shift (dy, dx) is a plain LDS address offset.
constexpr int PATCH_LDA = 16;   // floats per LDS row of k_conv3x3_patch (16 channels, swizzled instead of padded)

struct PatchP {
    const float* in; int in_ld, in_coff;
    int B, Cin, nlev; Lvl lv[4]; int tile0[5]; int tiles_x[4], tiles_y[4];
    const float* w; int Cout, Cout16, K;
    const float* scale; const float* shift; int ep_stride, relu_cout;
    float* out; int out_ld, out_coff;
    int xmap;                               // tile_of_block mode (1: an XCD owns a contiguous band of tiles -> halo rows re-read inside its L2)
    size_t w_lstride;                       // k_conv3x3_ws, per-level weights: level l's packed weights start w_lstride floats further (one tile per block)
};

template <int TH, bool BF = false>
__global__ __launch_bounds__(256) void k_conv3x3_patch(PatchP p) {
    // LDS rows hold the 16 channels of a slab with NO padding (64 bytes): the four 16-byte slots of row r are stored at slot ^ ((r >> 2) & 3),
    // which makes the ds_read_b128 of 16 consecutive rows (one per lane, same logical slot) hit 16 disjoint bank groups -- conflict-free
    // like the padded layout (row stride 96 bytes) at 2/3 of the footprint: 43.8 KB per block, three blocks per CU instead of two.
    constexpr int TW = 16, BN = 64, PH = TH + 2, PW = TW + 2, NPIX = PH * PW, LDA = PATCH_LDA;
    auto swz = [](int row, int slot) -> int { return row * LDA + ((slot ^ ((row >> 2) & 3)) << 2); };
    constexpr int TM = TH / 4, TN = BN / 16;
    constexpr int A_IT = (NPIX * 4 + 255) / 256, B_IT = 9;          // float4 slots per thread (B: tap j = slot j since BN*4 == 256)
    extern __shared__ __attribute__((aligned(16))) float plds[];
    float* As = plds;                       // [NPIX][LDA]
    float* Bs = plds + NPIX * LDA;          // [9][BN][LDA]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- which tile
    int pbx, pby;
    tile_of_block(p.xmap, pbx, pby);
    int lvl = 0;
#pragma unroll
    for (int l = 1; l < 4; ++l)
        if (l < p.nlev && pbx >= p.tile0[l]) lvl = l;
    const Lvl L = p.lv[lvl];
    const int tl = pbx - p.tile0[lvl];
    const int tpi = p.tiles_x[lvl] * p.tiles_y[lvl];
    const int b = tl / tpi, tr = tl - b * tpi;
    const int ty0 = (tr / p.tiles_x[lvl]) * TH, tx0 = (tr % p.tiles_x[lvl]) * TW;
    const int n0 = pby * BN;
    const int ibase = L.irow0 + b * L.H * L.W, obase = L.orow0 + b * L.H * L.W;
    const float* zero = g_zero16;
    auto sel = [&](bool ok, const float* ptr) -> const f32x4* {
        const uintptr_t m = (uintptr_t)0 - (uintptr_t)ok;
        return reinterpret_cast<const f32x4*>(((uintptr_t)ptr & m) | ((uintptr_t)zero & ~m));
    };
    // ---- staging slots
    const float* a_ptr[A_IT]; bool a_ok[A_IT]; int a_lds[A_IT];
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
        const int f = tid + i * 256, pi = f >> 2, q = f & 3;
        const int py = pi / PW, px = pi - py * PW;
        const int gy = ty0 - 1 + py, gx = tx0 - 1 + px;
        a_ok[i] = pi < NPIX && (unsigned)gy < (unsigned)L.H && (unsigned)gx < (unsigned)L.W;
        a_ptr[i] = p.in + (ptrdiff_t)(ibase + gy * L.W + gx) * p.in_ld + p.in_coff + q * 4;
        a_lds[i] = pi < NPIX ? swz(pi, q) : -1;
    }
    const int bn = tid >> 2, bq = tid & 3;
    const bool b_ok = n0 + bn < p.Cout16;
    const float* b_ptr = p.w + (size_t)(b_ok ? n0 + bn : 0) * p.K + bq * 4;
    const int b_lds = swz(bn, bq);                           // tap j adds j * BN rows: BN % 16 == 0 keeps the swizzle phase
    f32x4 ra[A_IT], rb[B_IT];
    auto gload = [&](int c0) {
#pragma unroll
        for (int i = 0; i < A_IT; ++i) ra[i] = *sel(a_ok[i], a_ptr[i] + c0);
#pragma unroll
        for (int j = 0; j < B_IT; ++j) rb[j] = *sel(b_ok, b_ptr + j * p.Cin + c0);
    };
    auto lstore = [&]() {
#pragma unroll
        for (int i = 0; i < A_IT; ++i)
            if (a_lds[i] >= 0) *reinterpret_cast<f32x4*>(As + a_lds[i]) = ra[i];
#pragma unroll
        for (int j = 0; j < B_IT; ++j) *reinterpret_cast<f32x4*>(Bs + j * BN * LDA + b_lds) = rb[j];
    };
    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int li = lane & 15, g4 = (lane >> 4) * 4;
    const int wrow = wave * TM;
    f32x4 pre_sc4[TN], pre_sh4[TN];                            // epilogue operands fetched under the main loop's loads
#pragma unroll
    for (int j = 0; j < TN; ++j)                               // CONV_SCALE_SHIFT4 (ore_conv_epilogue.h), open-coded: its n + r changes this kernel's code
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + j * 16 + g4 + r;
            pre_sc4[j][r] = (p.scale && n < p.Cout) ? p.scale[lvl * p.ep_stride + n] : 1.0f;
            pre_sh4[j][r] = (p.shift && n < p.Cout) ? p.shift[lvl * p.ep_stride + n] : 0.0f;
        }
    ORE_TR(0);
    gload(0);
    ORE_TR(1);
    for (int c0 = 0; c0 < p.Cin; c0 += 16) {
        lstore();
        ORE_TR(2 + (c0 >> 4) * 4);
        __syncthreads();
        ORE_TR(3 + (c0 >> 4) * 4);
        if (c0 + 16 < p.Cin) gload(c0 + 16);
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                f32x4 af[TM], bf[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    af[i] = *reinterpret_cast<const f32x4*>(As + swz((wrow + i + dy) * PW + li + dx, lane >> 4));
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    bf[j] = *reinterpret_cast<const f32x4*>(Bs + swz((dy * 3 + dx) * BN + j * 16 + li, lane >> 4));
                if constexpr (BF) {
                    s16x4 ah[TM], bh[TN];
#pragma unroll
                    for (int i = 0; i < TM; ++i) ah[i] = to_bf16x4(af[i]);
#pragma unroll
                    for (int j = 0; j < TN; ++j) bh[j] = to_bf16x4(bf[j]);
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(bh[j], ah[i], acc[i][j], 0, 0, 0);
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int i = 0; i < TM; ++i)
#pragma unroll
                            for (int j = 0; j < TN; ++j)
                                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[j][t], af[i][t], acc[i][j], 0, 0, 0);   // D^T: rows = channels
                }
            }
        ORE_TR(4 + (c0 >> 4) * 4);
        __syncthreads();
        ORE_TR(5 + (c0 >> 4) * 4);
    }
    // ---- epilogue.  The operands are swapped (weights as the MFMA "A"), so accumulator (i, j) holds D^T: lane = (pixel lane&15 of tile
    // row wrow+i, channels n0 + j*16 + (lane>>4)*4 .. +3) -> ONE 16-byte store per lane per tile instead of four 4-byte stores
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + j * 16 + g4;                       // first of this lane's 4 channels
        if (n >= p.Cout) continue;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int gy = ty0 + wrow + i, gx = tx0 + li;
            if (gy < L.H && gx < L.W) {
                f32x4 v = acc[i][j] * pre_sc4[j] + pre_sh4[j];
                CONV_RELU4(v, n, p.relu_cout)
                float* o = p.out + (size_t)(obase + gy * L.W + gx) * p.out_ld + p.out_coff + n;
                CONV_STORE4_F32(o, v, true, n, p.Cout)
            }
        }
    }
    ORE_TR(62);
}

// Double-buffered 8-wave variant: a block of 512 threads owns an 8 x 16 pixel tile x 64 output channels; wave w = tile row w.
// Two LDS buffers (2 x 72 KB, one block per CU): the slab k+1 written to the other buffer while slab k is multiplied, ONE barrier per
// slab, the 36 KB weight slab staged once per 128 pixels (half of the 4-wave kernel's weight traffic per pixel).
__global__ __launch_bounds__(512) void k_conv3x3_patch_db(PatchP p) {
    constexpr bool BF = false;                                  // tuner-only kernel: fp32 operands only
    constexpr int TH = 8, TW = 16, BN = 64, PH = TH + 2, PW = TW + 2, NPIX = PH * PW, LDA = 24, NT_ = 512;
    constexpr int TN = BN / 16;
    constexpr int A_IT = (NPIX * 4 + NT_ - 1) / NT_;            // 720 float4 -> 2 slots
    constexpr int B_IT = (9 * BN * 4 + NT_ - 1) / NT_;          // 2304 float4 -> 5 slots (4.5)
    constexpr int BUF = (NPIX + 9 * BN) * LDA;                  // floats per buffer
    extern __shared__ __attribute__((aligned(16))) float plds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int pbx, pby;
    tile_of_block(p.xmap, pbx, pby);
    int lvl = 0;
#pragma unroll
    for (int l = 1; l < 4; ++l)
        if (l < p.nlev && pbx >= p.tile0[l]) lvl = l;
    const Lvl L = p.lv[lvl];
    const int tl = pbx - p.tile0[lvl];
    const int tpi = p.tiles_x[lvl] * p.tiles_y[lvl];
    const int b = tl / tpi, tr = tl - b * tpi;
    const int ty0 = (tr / p.tiles_x[lvl]) * TH, tx0 = (tr % p.tiles_x[lvl]) * TW;
    const int n0 = pby * BN;
    const int ibase = L.irow0 + b * L.H * L.W, obase = L.orow0 + b * L.H * L.W;
    const float* zero = g_zero16;
    auto sel = [&](bool ok, const float* ptr) -> const f32x4* {
        const uintptr_t m = (uintptr_t)0 - (uintptr_t)ok;
        return reinterpret_cast<const f32x4*>(((uintptr_t)ptr & m) | ((uintptr_t)zero & ~m));
    };
    const float* a_ptr[A_IT]; bool a_ok[A_IT]; int a_lds[A_IT];
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
        const int f = tid + i * NT_, pi = f >> 2, q = f & 3;
        const int py = pi / PW, px = pi - py * PW;
        const int gy = ty0 - 1 + py, gx = tx0 - 1 + px;
        a_ok[i] = pi < NPIX && (unsigned)gy < (unsigned)L.H && (unsigned)gx < (unsigned)L.W;
        a_ptr[i] = p.in + (ptrdiff_t)(ibase + gy * L.W + gx) * p.in_ld + p.in_coff + q * 4;
        a_lds[i] = pi < NPIX ? pi * LDA + q * 4 : -1;
    }
    const float* b_ptr[B_IT]; bool b_ok[B_IT]; int b_lds[B_IT];
#pragma unroll
    for (int j = 0; j < B_IT; ++j) {
        const int f = tid + j * NT_;                           // float4 index over [tap][bn][q]
        const int tap = f / (BN * 4), rem = f - tap * (BN * 4), bn = rem >> 2, q = rem & 3;
        b_ok[j] = f < 9 * BN * 4 && n0 + bn < p.Cout16;
        b_ptr[j] = p.w + (size_t)(b_ok[j] ? n0 + bn : 0) * p.K + (size_t)(tap < 9 ? tap : 0) * p.Cin + q * 4;
        b_lds[j] = f < 9 * BN * 4 ? NPIX * LDA + (tap * BN + bn) * LDA + q * 4 : -1;
    }
    f32x4 ra[A_IT], rb[B_IT];
    auto gload = [&](int c0) {
#pragma unroll
        for (int i = 0; i < A_IT; ++i) ra[i] = *sel(a_ok[i], a_ptr[i] + c0);
#pragma unroll
        for (int j = 0; j < B_IT; ++j) rb[j] = *sel(b_ok[j], b_ptr[j] + c0);
    };
    auto lstore = [&](float* buf) {
#pragma unroll
        for (int i = 0; i < A_IT; ++i)
            if (a_lds[i] >= 0) *reinterpret_cast<f32x4*>(buf + a_lds[i]) = ra[i];
#pragma unroll
        for (int j = 0; j < B_IT; ++j)
            if (b_lds[j] >= 0) *reinterpret_cast<f32x4*>(buf + b_lds[j]) = rb[j];
    };
    f32x4 acc[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int li = lane & 15, g4 = (lane >> 4) * 4;
    f32x4 pre_sc4[TN], pre_sh4[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j)                               // CONV_SCALE_SHIFT4 (ore_conv_epilogue.h), open-coded: its n + r changes this kernel's code
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + j * 16 + g4 + r;
            pre_sc4[j][r] = (p.scale && n < p.Cout) ? p.scale[lvl * p.ep_stride + n] : 1.0f;
            pre_sh4[j][r] = (p.shift && n < p.Cout) ? p.shift[lvl * p.ep_stride + n] : 0.0f;
        }
    gload(0);
    lstore(plds);
    if (16 < p.Cin) gload(16);
    __syncthreads();
    int cur = 0;
    for (int c0 = 0; c0 < p.Cin; c0 += 16) {
        const float* As = plds + cur * BUF;
        const float* Bs = As + NPIX * LDA;
        // park the next slab (already in registers) in the other buffer, then fetch the one after it: both overlap the MFMAs below
        if (c0 + 16 < p.Cin) {
            lstore(plds + (cur ^ 1) * BUF);
            if (c0 + 32 < p.Cin) gload(c0 + 32);
        }
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                f32x4 bf[TN];
                const f32x4 af = *reinterpret_cast<const f32x4*>(As + ((wave + dy) * PW + li + dx) * LDA + g4);
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    bf[j] = *reinterpret_cast<const f32x4*>(Bs + ((dy * 3 + dx) * BN + j * 16 + li) * LDA + g4);
                if constexpr (BF) {
                    const s16x4 ah = to_bf16x4(af);
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(to_bf16x4(bf[j]), ah, acc[j], 0, 0, 0);
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[j][t], af[t], acc[j], 0, 0, 0);
                }
            }
        __syncthreads();            // everyone is done reading `cur` and done writing `cur ^ 1`
        cur ^= 1;
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + j * 16 + g4;
        if (n >= p.Cout) continue;
        const int gy = ty0 + wave, gx = tx0 + li;
        if (gy < L.H && gx < L.W) {
            f32x4 v = acc[j] * pre_sc4[j] + pre_sh4[j];
            CONV_RELU4(v, n, p.relu_cout)
            float* o = p.out + (size_t)(obase + gy * L.W + gx) * p.out_ld + p.out_coff + n;
            CONV_STORE4_F32(o, v, true, n, p.Cout)
        }
    }
}

// Weight-stationary 3x3 kernels (stem_2 and the Cin = 64 / 128 layers with large M: half of the network's FLOPs).
// A wave keeps the weights of 16 output channels x 9 taps x 64 input channels in REGISTERS (36 MFMA A-fragments, 144 VGPRs) for the
// whole launch; the block is persistent and walks pixel tiles (TH x 16 px), staging only the (TH+2) x 18 x CIN halo patch per tile
// (double-buffered LDS, one barrier per tile, 144*TH MFMAs per wave between barriers).  No weight re-staging, one LDS read per
// 4 MFMAs, small tiles (TH = 2) balance thousands of tiles over the resident blocks.
//   CIN = 64,  KS = 1: 4 waves = 4 groups of 16 output channels.
//   CIN = 128, KS = 2: 8 waves; waves w and w+4 share a channel group and split the input channels (64 each); the upper half
//                      parks its accumulators in LDS (parity double-buffered) and the lower half adds them before the epilogue.
// SB: bf16 STORAGE build (ore_conv_desc.storage): CIN counts 4-byte units = PAIRS of bf16 channels (32 -> 64 channels, 64 -> 128), the
// halo patch and the weights are bf16, a b128 fragment is 8 consecutive channels = the operand of v_mfma_f32_16x16x32_bf16, of which ONE
// replaces four fp32 MFMAs; the wave keeps 16 output channels x 9 taps x all input channels in 72 / 144 VGPRs.  With the matrix time
// gone (36-72 MFMAs of 16 clocks per 2x16 tile) the tile is made tall (TH = 8) so that the per-tile barrier, decode and halo overlap
// (10 / 8 rows staged per 8 rows of output) amortise.
// ST: conv stride (1, or 2 = stem_3: the tile is TH x 16 OUTPUT pixels, its input patch (2 TH + 1) x 33, lane li reads pixel 2 li + dx).
template <int TH, int CIN, int KS, bool BF = false, bool SB = false, int ST = 1>
__global__ __launch_bounds__(256 * KS, KS == 1 ? 2 : 1) void k_conv3x3_ws(PatchP p, int ntiles) {
    constexpr int CW = CIN / KS;                                // 4-byte units of a wave's K slice: 64 (fp32 builds), 32 (bf16 storage: 64 channels)
    // LDS row stride: +8 floats makes the 16-lane b128 fragment reads conflict-free at stride 1; at stride 2 the lanes are two rows apart,
    // +4 (an odd number of 16-byte units per row pair ... 2 * (CIN + 4) * 4 B) leaves a 2-way conflict instead of 4-way
    constexpr int TW = 16, PH = (TH - 1) * ST + 3, PW = (TW - 1) * ST + 3, NPIX = PH * PW, LDC = CIN + (ST == 1 ? 8 : 4), NCH = CW / 16, NTH = 256 * KS, F4 = CIN / 4;
    static_assert(SB ? (CW == 32 || (KS == 1 && CW == 64)) : CW == 64, "one 64-channel weight slice per wave");
    constexpr int A_IT = (NPIX * F4 + NTH - 1) / NTH;          // float4 slots per thread for one halo patch
    constexpr int BUF = NPIX * LDC;
    constexpr int PARK = KS > 1 ? 4 * TH * 256 : 0;            // floats per parity buffer of parked accumulators
    extern __shared__ __attribute__((aligned(16))) float plds[];
    float* park = plds + 2 * BUF;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cgp = wave & 3, kh = wave >> 2;                  // channel group, K half
    const int li = lane & 15, g4 = (lane >> 4) * 4;
    const int n0 = blockIdx.y * 64 + cgp * 16;                 // this wave's 16 output channels
    // ---- weights -> registers (MFMA A operand: row = channel n0 + li, k = kh*64 + chunk*16 + g4 + t)
    f32x4 wf[9][NCH];
    {
        const bool okw = n0 + li < p.Cout16;
        int wl = 0;                                             // per-level weights (the three FPN output convs in one launch): this block's
        if (p.w_lstride) {                                      // only tile is tile blockIdx.x (the launcher sizes the grid that way)
#pragma unroll
            for (int l = 1; l < 4; ++l)
                if (l < p.nlev && (int)blockIdx.x >= p.tile0[l]) wl = l;
        }
        const float* wrow = p.w + wl * p.w_lstride + (size_t)(okw ? n0 + li : 0) * p.K + kh * CW + g4;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                wf[tap][c] = *reinterpret_cast<const f32x4*>(wrow + tap * CIN + c * 16);
                if (!okw) wf[tap][c] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
    }
    const float* zero = g_zero16;
    auto sel = [&](bool ok, const float* ptr) -> const f32x4* {
        const uintptr_t m = (uintptr_t)0 - (uintptr_t)ok;
        return reinterpret_cast<const f32x4*>(((uintptr_t)ptr & m) | ((uintptr_t)zero & ~m));
    };
    // tile-independent part of the staging slots
    int s_py[A_IT], s_px[A_IT], s_q[A_IT], s_lds[A_IT];
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
        const int f = tid + i * NTH, pi = f / F4;
        s_q[i] = (f - pi * F4) * 4;
        s_py[i] = pi / PW; s_px[i] = pi - s_py[i] * PW;
        s_lds[i] = pi < NPIX ? pi * LDC + s_q[i] : -1;
    }
    struct TileGeo { int lvl, ty0, tx0, ibase, obase, H, W, Ho, Wo; };
    auto decode = [&](int t) -> TileGeo {
        TileGeo g;
        g.lvl = 0;
#pragma unroll
        for (int l = 1; l < 4; ++l)
            if (l < p.nlev && t >= p.tile0[l]) g.lvl = l;
        const Lvl& L = p.lv[g.lvl];
        const int tl = t - p.tile0[g.lvl];
        const int tpi = p.tiles_x[g.lvl] * p.tiles_y[g.lvl];
        const int b = tl / tpi, tr = tl - b * tpi;
        g.ty0 = (tr / p.tiles_x[g.lvl]) * TH; g.tx0 = (tr % p.tiles_x[g.lvl]) * TW;
        g.H = L.H; g.W = L.W;
        g.Ho = ST == 1 ? L.H : L.Ho; g.Wo = ST == 1 ? L.W : L.Wo;
        g.ibase = L.irow0 + b * L.H * L.W; g.obase = L.orow0 + b * g.Ho * g.Wo;
        return g;
    };
    f32x4 ra[A_IT];
    auto gload = [&](const TileGeo& g) {
#pragma unroll
        for (int i = 0; i < A_IT; ++i) {
            const int gy = g.ty0 * ST - 1 + s_py[i], gx = g.tx0 * ST - 1 + s_px[i];
            const bool ok = s_lds[i] >= 0 && (unsigned)gy < (unsigned)g.H && (unsigned)gx < (unsigned)g.W;
            ra[i] = *sel(ok, p.in + (ptrdiff_t)(g.ibase + gy * g.W + gx) * p.in_ld + p.in_coff + s_q[i]);
        }
    };
    auto lstore = [&](float* buf) {
#pragma unroll
        for (int i = 0; i < A_IT; ++i)
            if (s_lds[i] >= 0) *reinterpret_cast<f32x4*>(buf + s_lds[i]) = ra[i];
    };
    // persistent walk.  p.xmap: the blocks of one residue class (blockIdx.x % 8 = one XCD) share a CONTIGUOUS band of tiles (row-major,
    // so the halo rows two vertically adjacent tiles both read stay in that XCD's L2) and walk it with stride gridDim.x / 8.
    int t = blockIdx.x, t_end = ntiles, t_step = gridDim.x;
    if (p.xmap && (gridDim.x & 7) == 0) {
        const int r = blockIdx.x & 7, q = ntiles >> 3, rem = ntiles & 7;
        const int base = r * q + min(r, rem);
        t = base + (blockIdx.x >> 3); t_end = base + q + (r < rem ? 1 : 0); t_step = gridDim.x >> 3;
    }
    TileGeo cur_g = decode(t < t_end ? t : 0);
    if (t < t_end) { gload(cur_g); lstore(plds); }
    __syncthreads();
    int cur = 0, parity = 0;
    for (; t < t_end; t += t_step) {
        const int tn = t + t_step;
        const bool has_next = tn < t_end;
        TileGeo nxt_g = cur_g;
        if (has_next) { nxt_g = decode(tn); gload(nxt_g); }       // the next halo patch flies under this tile's MFMAs
        const float* As = plds + cur * BUF + kh * CW;
        f32x4 acc[TH];
#pragma unroll
        for (int sg = 0; sg < TH; ++sg) acc[sg] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx)
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    f32x4 af[TH];
#pragma unroll
                    for (int sg = 0; sg < TH; ++sg)
                        af[sg] = *reinterpret_cast<const f32x4*>(As + ((sg * ST + dy) * PW + li * ST + dx) * LDC + c * 16 + g4);
                    if constexpr (SB) {
#pragma unroll
                        for (int sg = 0; sg < TH; ++sg)
                            acc[sg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wf[dy * 3 + dx][c]),
                                                                              __builtin_bit_cast(bf16x8_t, af[sg]), acc[sg], 0, 0, 0);
                    } else if constexpr (BF) {
                        const s16x4 wh = to_bf16x4(wf[dy * 3 + dx][c]);
#pragma unroll
                        for (int sg = 0; sg < TH; ++sg)
                            acc[sg] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(wh, to_bf16x4(af[sg]), acc[sg], 0, 0, 0);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
#pragma unroll
                            for (int sg = 0; sg < TH; ++sg)
                                acc[sg] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[dy * 3 + dx][c][k], af[sg][k], acc[sg], 0, 0, 0);
                    }
                }
        if (KS > 1 && kh == 1) {
#pragma unroll
            for (int sg = 0; sg < TH; ++sg)
                *reinterpret_cast<f32x4*>(park + parity * PARK + ((cgp * TH + sg) * 64 + lane) * 4) = acc[sg];
        }
        if (has_next) lstore(plds + (cur ^ 1) * BUF);
        __syncthreads();            // `cur` fully read, `cur ^ 1` fully written, parked accumulators visible
        // ---- epilogue (lower K half only): lane = pixel (row ty0 + sg, column tx0 + li), channels n0 + g4 .. +3
        const int n = n0 + g4;
        if (kh == 0 && n < p.Cout) {
            f32x4 sc4, sh4;
            CONV_SCALE_SHIFT4(p, cur_g.lvl, n, sc4, sh4)
#pragma unroll
            for (int sg = 0; sg < TH; ++sg) {
                f32x4 a = acc[sg];
                if (KS > 1) a += *reinterpret_cast<const f32x4*>(park + parity * PARK + ((cgp * TH + sg) * 64 + lane) * 4);
                const int gy = cur_g.ty0 + sg, gx = cur_g.tx0 + li;
                if (gy < cur_g.Ho && gx < cur_g.Wo) {
                    f32x4 v = a * sc4 + sh4;
                    CONV_RELU4(v, n, p.relu_cout)
                    if constexpr (SB) {                          // bf16 output tensor (Cout % 64 == 0 on this path: whole vectors)
                        st4(reinterpret_cast<ore_bf16_t*>(p.out) + (size_t)(cur_g.obase + gy * cur_g.Wo + gx) * p.out_ld + p.out_coff + n, v);
                    } else {
                        float* o = p.out + (size_t)(cur_g.obase + gy * cur_g.Wo + gx) * p.out_ld + p.out_coff + n;
                        CONV_STORE4_F32(o, v, true, n, p.Cout)
                    }
                }
            }
        }
        cur ^= 1;
        parity ^= 1;
        cur_g = nxt_g;
    }
}

int g_conv_bf16 = 0;     // ore_conv_set_precision: 1 = bf16 MFMA operands (fp32 storage and accumulation)
int g_conv_mode = 0;     // the mode as set (ORE_CONV_BF16S = 2 is an engine build mode, see ore_hip.h)

// the tile table of the 3x3 tile kernels: tiles of TH output rows x 16 columns, level by level
PatchP patch_params(const ConvP& c, int TH, int xmap) {
    PatchP p{};
    p.in = c.in; p.in_ld = c.in_ld; p.in_coff = c.in_coff; p.B = c.B; p.Cin = c.Cin; p.nlev = c.nlev;
    int tiles = 0;
    for (int l = 0; l < c.nlev; ++l) {
        p.lv[l] = c.lv[l];
        p.tiles_x[l] = ceil_div(c.lv[l].Wo, 16); p.tiles_y[l] = ceil_div(c.lv[l].Ho, TH);
        p.tile0[l] = tiles;
        tiles += c.B * p.tiles_x[l] * p.tiles_y[l];
    }
    p.tile0[c.nlev] = tiles;
    p.w = c.w; p.Cout = c.Cout; p.Cout16 = c.Cout16; p.K = c.K;
    p.scale = c.scale; p.shift = c.shift; p.ep_stride = c.ep_stride; p.relu_cout = c.relu_cout;
    p.out = c.out; p.out_ld = c.out_ld; p.out_coff = c.out_coff;
    p.xmap = xmap;
    p.w_lstride = c.w_lstride;
    return p;
}

template <int TH, int CF, int KS, bool BF = false, bool SBF = false, int ST = 1>
int ws_go(const PatchP& p, dim3 grid, hipStream_t st) {
    const size_t lds = ((size_t)2 * (((TH - 1) * ST + 3) * (15 * ST + 3)) * (CF + (ST == 1 ? 8 : 4)) + (KS > 1 ? 2 * 4 * TH * 256 : 0)) * sizeof(float);
    static bool attr = false;
    if (!attr) { ORE_HIP(hipFuncSetAttribute((const void*)k_conv3x3_ws<TH, CF, KS, BF, SBF, ST>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); attr = true; }
    hipLaunchKernelGGL((k_conv3x3_ws<TH, CF, KS, BF, SBF, ST>), grid, dim3(256 * KS), lds, st, p, p.tile0[p.nlev]);
    return ore_launch_status("k_conv3x3_ws");
}

template <int TH, bool BF = false>
int patch_go(const PatchP& p, dim3 grid, hipStream_t st) {
    const size_t lds = (size_t)((TH + 2) * 18 + 9 * 64) * PATCH_LDA * sizeof(float);
    static bool attr = false;
    if (!attr) { ORE_HIP(hipFuncSetAttribute((const void*)k_conv3x3_patch<TH, BF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); attr = true; }
    hipLaunchKernelGGL((k_conv3x3_patch<TH, BF>), grid, dim3(256), lds, st, p);
    return ore_launch_status("k_conv3x3_patch");
}

template <int BM, int BN, int WGM, int WGN, int WGK, bool BF>
int igemm_go(const ConvP& p, dim3 grid, hipStream_t st) {
    if (p.in_mul) hipLaunchKernelGGL((k_conv_igemm<BM, BN, WGM, WGN, WGK, true, BF>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((k_conv_igemm<BM, BN, WGM, WGN, WGK, false, BF>), grid, dim3(256), 0, st, p);
    return ore_launch_status("k_conv_igemm");
}

}  // namespace

namespace oreconv {

// k_conv3x3_ws: bf16 storage (WS_SB: 4-row tiles, or 2-row stride-2 tiles for stem_3), fp32 storage (WS64 / WS128: 2-row tiles)
int launch_ws(const ConvP& c, const ConvPlan& pl, hipStream_t st) {
    const PatchP p = patch_params(c, pl.bm, pl.xmap);
    const dim3 grid(pl.gx, pl.gy);
    if (pl.launcher == ORE_LAUNCH_WS_SB) {
        if (pl.build[3] == 2) return ws_go<2, 32, 1, false, true, 2>(p, grid, st);
        if (pl.build[1] == 32) return ws_go<4, 32, 1, false, true>(p, grid, st);
        return ws_go<4, 64, 2, false, true>(p, grid, st);
    }
    if (pl.build[1] == 128) return ws_go<2, 128, 2>(p, grid, st);
    return pl.build[3] ? ws_go<2, 64, 1, true>(p, grid, st) : ws_go<2, 64, 1, false>(p, grid, st);
}

// k_conv3x3_patch<4 | 8> (bf16 operands: <4> only), k_conv3x3_patch_db (8-row double-buffered, 8 waves)
int launch_patch(const ConvP& c, const ConvPlan& pl, hipStream_t st) {
    const PatchP p = patch_params(c, pl.bm, pl.xmap);
    const dim3 grid(pl.gx, pl.gy);
    if (pl.launcher == ORE_LAUNCH_PATCH_DB) {
        const size_t lds = (size_t)2 * (10 * 18 + 9 * 64) * 24 * sizeof(float);
        static bool attrdb = false;
        if (!attrdb) { ORE_HIP(hipFuncSetAttribute((const void*)k_conv3x3_patch_db, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); attrdb = true; }
        hipLaunchKernelGGL(k_conv3x3_patch_db, grid, dim3(512), lds, st, p);
        return ore_launch_status("k_conv3x3_patch");
    }
    if (pl.launcher == ORE_LAUNCH_PATCH8) return patch_go<8>(p, grid, st);
    return pl.build[2] ? patch_go<4, true>(p, grid, st) : patch_go<4, false>(p, grid, st);
}

int launch_igemm(const ConvP& p, const ConvPlan& pl, hipStream_t st) {
    const dim3 grid(pl.gx, pl.gy, pl.splitk);
#define IGEMM_GO(bm_, bn_, wgm, wgn, wgk, hasbf)                                                             \
    if (pl.bm == bm_ && pl.bn == bn_ && pl.build[0] == wgm && pl.build[1] == wgn && pl.build[2] == wgk) {  \
        if constexpr (hasbf) { if (pl.build[3]) return igemm_go<bm_, bn_, wgm, wgn, wgk, true>(p, grid, st); } \
        return igemm_go<bm_, bn_, wgm, wgn, wgk, false>(p, grid, st);                                      \
    }
    ORE_IGEMM_BUILDS(IGEMM_GO)
#undef IGEMM_GO
    return ORE_EINVAL;
}

}  // namespace oreconv

extern "C" size_t ore_packed_weight_floats(int32_t Cout, int32_t Cin, int32_t kh, int32_t kw) {
    return (size_t)round_up(Cout, 16) * kh * kw * Cin;
}

extern "C" int ore_pack_conv_weight_host(const float* w, int32_t Cout, int32_t Cin, int32_t kh, int32_t kw,
                                         float* dst) {
    ORE_CHECK_ARG(w && dst && Cout > 0 && Cin > 0 && kh > 0 && kw > 0, "ore_pack_conv_weight_host: bad args");
    const size_t K = (size_t)kh * kw * Cin;
    const int C16 = round_up(Cout, 16);
    for (int n = 0; n < C16; ++n)
        for (int t = 0; t < kh * kw; ++t)
            for (int c = 0; c < Cin; ++c)
                dst[(size_t)n * K + (size_t)t * Cin + c] = n < Cout ? w[((size_t)n * Cin + c) * kh * kw + t] : 0.0f;
    return ORE_OK;
}

static inline uint16_t f32_to_bf16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);      // NaN stays a (quiet) NaN
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

extern "C" size_t ore_packed_weight_bf16_elems(int32_t Cout, int32_t Cin, int32_t kh, int32_t kw) {
    return (size_t)round_up(Cout, 16) * kh * kw * round_up(Cin, 32);
}

extern "C" int ore_pack_conv_weight_bf16_host(const float* w, int32_t Cout, int32_t Cin, int32_t kh, int32_t kw, uint16_t* dst) {
    ORE_CHECK_ARG(w && dst && Cout > 0 && Cin > 0 && kh > 0 && kw > 0, "ore_pack_conv_weight_bf16_host: bad args");
    const int C32 = round_up(Cin, 32), C16 = round_up(Cout, 16);
    const size_t K = (size_t)kh * kw * C32;
    for (int n = 0; n < C16; ++n)
        for (int t = 0; t < kh * kw; ++t)
            for (int c = 0; c < C32; ++c)
                dst[(size_t)n * K + (size_t)t * C32 + c] = (n < Cout && c < Cin) ? f32_to_bf16_rne(w[((size_t)n * Cin + c) * kh * kw + t]) : (uint16_t)0;
    return ORE_OK;
}

extern "C" size_t ore_conv_workspace_floats(void) { return ORE_CONV_WS_FLOATS; }

#ifdef ORE_TRACE
extern "C" int ore_debug_set_trace(unsigned long long* buf) {
    ORE_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_trace), &buf, sizeof(buf)));
    return ORE_OK;
}
#endif

extern "C" int ore_conv_set_precision(int32_t mode) {
    ORE_CHECK_ARG(mode == ORE_CONV_FP32 || mode == ORE_CONV_BF16 || mode == ORE_CONV_BF16S,
                  "ore_conv_set_precision: mode must be ORE_CONV_FP32, ORE_CONV_BF16 or ORE_CONV_BF16S");
    g_conv_mode = mode;
    g_conv_bf16 = mode == ORE_CONV_BF16;                          // BF16S changes what an ENGINE builds; plain fp32-tensor convs stay fp32
    return ORE_OK;
}

extern "C" int32_t ore_conv_get_precision(void) { return g_conv_mode; }

// Checks the arguments of an ore_conv2d_fwd (n_levels = 0) or ore_conv2d_levels_fwd call and fills the kernel parameter block
static int conv_setup(ConvP& p, const ore_conv_desc* d, int n_levels, const int32_t* H, const int32_t* W, int ep_stride) {
    ORE_CHECK_ARG(d && d->in && d->w && d->out, "ore_conv2d_fwd: null pointer");
    ORE_CHECK_ARG(d->Cin > 0 && d->Cin % 16 == 0, "ore_conv2d_fwd: Cin=%d must be a multiple of 16", d->Cin);
    ORE_CHECK_ARG(d->in_ld % 4 == 0 && d->in_coff % 4 == 0 && d->in_coff + d->Cin <= d->in_ld,
                  "ore_conv2d_fwd: input slice ld=%d coff=%d Cin=%d", d->in_ld, d->in_coff, d->Cin);
    ORE_CHECK_ARG(d->out_coff + d->Cout <= d->out_ld && d->Cout > 0, "ore_conv2d_fwd: output slice");
    ORE_CHECK_ARG(d->B > 0 && d->kh > 0 && d->kw > 0 && d->kh * d->kw <= 32 && d->stride > 0 && d->pad >= 0, "ore_conv2d_fwd: bad geometry (kernel up to 32 taps)");
    ORE_CHECK_ARG(((uintptr_t)d->in & 15) == 0 && ((uintptr_t)d->w & 15) == 0, "ore_conv2d_fwd: 16-byte alignment");
    ORE_CHECK_ARG(d->in_mul || !d->in_add, "ore_conv2d_fwd: in_add needs in_mul");
    ORE_CHECK_ARG(d->storage >= 0 && d->storage <= ORE_ST_BF16_F32OUT, "ore_conv2d_fwd: storage %d", d->storage);
    if (d->storage) {
        ORE_CHECK_ARG(d->in_ld % 8 == 0 && d->in_coff % 8 == 0 && !d->in_mul, "ore_conv2d_fwd: bf16 storage needs 16-byte aligned input slices and no input affine");
    }
    p = ConvP{};
    p.in = d->in; p.in_ld = d->in_ld; p.in_coff = d->in_coff;
    p.B = d->B; p.Cin = d->Cin; p.w = d->w;
    p.Cout = d->Cout; p.Cout16 = round_up(d->Cout, 16);
    p.kh = d->kh; p.kw = d->kw; p.stride = d->stride; p.pad = d->pad;
    p.K = d->kh * d->kw * d->Cin;
    p.scale = d->scale; p.shift = d->shift; p.relu_cout = d->relu_cout;
    p.in_mul = d->in_mul; p.in_add = d->in_mul ? d->in_add : nullptr; p.in_relu = d->in_relu;
    p.out = d->out; p.out_ld = d->out_ld; p.out_coff = d->out_coff;
    p.nchunks = d->kh * d->kw * (d->Cin / 16);
    p.colsum = d->colsum;
    p.wino = d->w_wino;
    p.tile_cnt = reinterpret_cast<int*>(d->workspace);
    p.ws = d->workspace ? d->workspace + ORE_CONV_CNT_INTS : nullptr;
    if (d->storage == ORE_ST_BF16 || d->storage == ORE_ST_BF16_F32OUT) {
        // bf16 tensors: the input side is handed to the kernels in 4-byte units (pairs of channels); the packed weights hold
        // round_up(Cin, 32) channels per tap (zero beyond Cin), so a 64-byte K chunk is 32 channels and a chunk that starts inside the
        // last 16 real channels reads 16 channels of whatever follows in the row -- finite activations -- against zero weights
        p.sb = 1 | (d->storage == ORE_ST_BF16 ? 2 : 0) | (d->add ? 4 : 0);
        const int cin32 = round_up(d->Cin, 32);
        p.in_ld = d->in_ld / 2; p.in_coff = d->in_coff / 2; p.Cin = cin32 / 2;
        p.K = d->kh * d->kw * p.Cin;
        p.nchunks = d->kh * d->kw * (p.Cin / 16);
        p.wino = nullptr;
    }
    if (n_levels == 0) {
        ORE_CHECK_ARG(d->H > 0 && d->W > 0, "ore_conv2d_fwd: bad geometry");
        p.nlev = 1;
        Lvl& L = p.lv[0];
        L.orow0 = 0; L.irow0 = 0; L.H = d->H; L.W = d->W;
        L.Ho = (d->H + 2 * d->pad - d->kh) / d->stride + 1;
        L.Wo = (d->W + 2 * d->pad - d->kw) / d->stride + 1;
        ORE_CHECK_ARG(L.Ho > 0 && L.Wo > 0, "ore_conv2d_fwd: empty output");
        p.M = d->B * L.Ho * L.Wo;
        p.add = d->add; p.add_ld = d->add_ld; p.add_coff = d->add_coff;
        p.add_H = (L.Ho + 1) / 2; p.add_W = (L.Wo + 1) / 2;
    } else {
        // the same conv over several pyramid levels: rows are level-major ([level][b][y][x]) in both the input and the output matrix
        ORE_CHECK_ARG(n_levels >= 1 && n_levels <= 4 && H && W, "ore_conv2d_levels_fwd: 1..4 levels");
        ORE_CHECK_ARG(d->stride == 1 && d->pad == d->kh / 2 && d->kh == d->kw && !d->add, "ore_conv2d_levels_fwd: 'same' convs only, no add");
        p.nlev = n_levels;
        int rows = 0;
        for (int l = 0; l < n_levels; ++l) {
            ORE_CHECK_ARG(H[l] > 0 && W[l] > 0, "ore_conv2d_levels_fwd: level %d geometry", l);
            p.lv[l] = {rows, rows, H[l], W[l], H[l], W[l]};
            rows += d->B * H[l] * W[l];
        }
        p.M = rows;
        p.ep_stride = ep_stride;
        if (d->w_level_stride) {                                  // per-level layers, bf16 storage: the weight-stationary 3x3 kernel or nothing
            ORE_CHECK_ARG(d->w_level_stride > 0 && d->w_level_stride % 2 == 0 && d->kh == 3 && d->storage == ORE_ST_BF16 && !d->in_mul && !d->colsum &&
                              !d->w_wino_level_stride,
                          "ore_conv2d_levels_fwd: w_level_stride is for 3x3 layers in bf16 storage (ORE_ST_BF16)");
            p.w_lstride = (size_t)d->w_level_stride / 2;          // the kernels count the bf16 side in 4-byte units
        } else if (d->w_wino_level_stride) {                      // per-level layers: the Winograd kernel or nothing
            ORE_CHECK_ARG(d->w_wino && d->w_wino_level_stride > 0 && d->kh == 3 && d->storage == ORE_ST_F32 && !d->in_mul && !d->colsum &&
                              conv_wino_covers(d->Cout, d->Cin) && (d->Cin == 64 || d->Cin == 128),
                          "ore_conv2d_levels_fwd: per-level weights need the Winograd form of a 3x3 layer with 64 / 128 input channels, fp32 storage");
            p.wino_lstride = (size_t)d->w_wino_level_stride;
        }
    }
    p.bf16 = (p.sb || p.wino_lstride) ? 0 : g_conv_bf16;       // bf16 storage and per-level Winograd weights multiply in their own precision
    return ORE_OK;
}

static int conv_run(const ore_conv_desc* d, int n_levels, const int32_t* H, const int32_t* W, int ep_stride, hipStream_t st) {
    ore_note_wino(0);
    ore_note_launch(ORE_LAUNCH_NONE, 1);
    ConvP p;
    const int rc = conv_setup(p, d, n_levels, H, W, ep_stride);
    if (rc) return rc;
    ore_flop_count_add(2.0 * (double)p.M * d->Cout * d->Cin * d->kh * d->kw);
    const ConvPlan pl = conv_plan(p, d->splitk, d->workspace_floats);
    if (pl.error) return pl.error;
    ore_note_launch(pl.launcher, pl.splitk);
    p.splitk = pl.splitk; p.steps_per_split = pl.steps_per_split; p.xmap = pl.xmap;
    switch (pl.launcher) {
    case ORE_LAUNCH_WS_SB: case ORE_LAUNCH_WS64: case ORE_LAUNCH_WS128: return launch_ws(p, pl, st);
    case ORE_LAUNCH_PATCH4: case ORE_LAUNCH_PATCH8: case ORE_LAUNCH_PATCH_DB: return launch_patch(p, pl, st);
    case ORE_LAUNCH_WINO: case ORE_LAUNCH_WINO_NU: return launch_wino(p, pl, st);
    case ORE_LAUNCH_GD: return launch_gd(p, pl, st);
    case ORE_LAUNCH_KD: return launch_kd(p, pl, st);
    case ORE_LAUNCH_RF: return launch_rf(p, pl, st);
    case ORE_LAUNCH_GS: return launch_gs(p, pl, st);
    case ORE_LAUNCH_KW: return launch_kw(p, pl, st);
    case ORE_LAUNCH_IGEMM: return launch_igemm(p, pl, st);
    }
    ore_set_error("ore_conv2d_fwd: plan names launcher %d", pl.launcher);
    return ORE_EINVAL;
}

extern "C" int ore_conv2d_fwd(const ore_conv_desc* d, void* stream) { return conv_run(d, 0, nullptr, nullptr, 0, (hipStream_t)stream); }

// Same conv over several pyramid levels in ONE launch: rows are level-major ([level][b][y][x]) in both the input
// and the output matrix; scale/shift may differ per level (ep_stride floats apart); in_mul/in_add are [level*B+b][Cin].
extern "C" int ore_conv2d_levels_fwd(const ore_conv_desc* d, int32_t n_levels, const int32_t* H, const int32_t* W,
                                     int32_t ep_stride, void* stream) {
    return conv_run(d, n_levels ? n_levels : -1, H, W, ep_stride, (hipStream_t)stream);   // (n_levels = 0 is not a level count here)
}

extern "C" int ore_conv_plan(const ore_conv_desc* d, int32_t n_levels, const int32_t* H, const int32_t* W, int32_t ep_stride, ore_conv_plan_t* out) {
    ORE_CHECK_ARG(out, "ore_conv_plan: null plan");
    *out = ConvPlan{};
    ConvP p;
    int rc = conv_setup(p, d, n_levels, H, W, ep_stride);
    if (rc == ORE_OK) {
        *out = conv_plan(p, d->splitk, d->workspace_floats);
        rc = out->error;
    }
    out->error = rc;
    return rc;
}

// rows of d->colsum: the row tiles of the kernel the call will run (d->colsum itself may still be null)
extern "C" int32_t ore_conv_colsum_rows(const ore_conv_desc* d) {
    if (!d) return 0;
    ore_conv_desc q = *d;
    if (!q.colsum) q.colsum = reinterpret_cast<float*>(q.workspace ? q.workspace : q.out);   // (any non-null address: only its presence is planned)
    ore_conv_plan_t pl;
    if (ore_conv_plan(&q, 0, nullptr, nullptr, 0, &pl) != ORE_OK) return 0;
    const int Ho = (d->H + 2 * d->pad - d->kh) / d->stride + 1, Wo = (d->W + 2 * d->pad - d->kw) / d->stride + 1;
    return ceil_div(d->B * Ho * Wo, pl.bm);
}
