// k_conv_rf -- implicit-GEMM NHWC convolution for the SMALLEST-M layers of the path (stages 4-5, their FPN laterals, the second-stage
// GEMM: M = 320 .. 1600 rows at batch 1), fp32 MFMA (v_mfma_f32_16x16x4_f32), fed straight from global memory into REGISTERS.
//
// Why a third kernel (round 4; profiles/r04_kw_phase_trace.txt).  These launches are not bound by the matrix cores (a 16x16 tile of
// stage 5 needs 0.85 us of MFMA issue) nor by bytes: k_conv_kw spends a block's 9.9 us as 1.9 us of prologue (row decode with integer
// divisions, tap masks, a cold instruction cache), 5.7 us in a K loop whose every step waits a full memory round trip (650-900
// clocks from DMA issue to landed -- the wave-private ring is two stages deep, and deeper rings were measured not to help because the
// ring's bookkeeping grows with it), and 1.5 us of reduction + epilogue.  The K slices of such a tile are tiny: 16 steps x (16 pixels
// + 16 weight rows) x 64 bytes per wave.  So this kernel drops the ring altogether:
//   * a wave's WHOLE K slice is requested up front -- MAXS steps x (1 + GB) `buffer_load_dwordx4`, each lane fetching exactly the
//     4 consecutive k of the MFMA fragment it will multiply (pixel / weight row = lane & 15, k quad = lane >> 4) -- and lands in
//     VGPRs; the K loop is then MFMAs behind counted waits, one memory latency for the whole slice instead of one per step;
//   * no LDS on the way in, no swizzle, no ring pointers; the loads go through the descriptor addressing of ore_conv_desc.h (this
//     kernel was its first user), so the issue loop has no branches;
//   * the weight requests depend on nothing but the block's coordinates: they are issued before the row decode, whose latency they
//     cover; the epilogue operands (scale / shift, the FPN top-down addend) are requested in the prologue too;
//   * K is split over the NW = 4 / 8 / 16 waves of the block (wave w owns a CONTIGUOUS range of 16-channel chunks, so its walk over
//     (tap, chunk) is one scalar add per step), partial tiles meet in LDS as in k_conv_kw; slices longer than MAXS steps run as
//     several batches.
// Epilogue semantics = ore_conv_epilogue.h's: y = acc * scale[n] + shift[n] (+ nearest-2x top-down add) (+ ReLU on n < relu_cout),
// per-tile column sums of the final values (the eSE average pool), channel-slice output.  Single level, fp32 storage, no input affine.
//
// Replaces F.conv2d + FrozenBatchNorm2d + ReLU / bias of d2z:modeling/backbone/vovnet.py:205-219,310-332 (stages 4-5), fpn.py:126-145
// (laterals 4-5), ref:fewx/modeling/fsod/fsod_roi_heads.py:500-520 (composed DSA + fc1) at batch 1.
#include "ore_conv_desc.h"
#include "ore_conv_epilogue.h"

namespace {
using namespace oreconv;

CONV_TRACE_SYMBOL(g_trace_rf)
constexpr int kTab = kRfTab;                      // chunk table entries (3x3 layers)
constexpr ChunkFmt kFmt = kChunkTapLow;

struct RfK {
    const float* in; const float* w; const float* scale; const float* shift; const float* add; float* out; float* colsum;
    unsigned in_bytes, w_bytes, sc_bytes, add_bytes;      // num_records of the buffer descriptors
    int M, K, Cout, Cout16, nchunks, nb;
    int irow0, H, W, Ho, Wo, in_ld, in_coff, stride, pad;
    int out_ld, out_coff, relu_cout, add_H, add_W, add_ld, add_coff;
    int xmap, gx, gy;
    float inv_hw, inv_wo, inv_gx, inv_gy;
};
struct RfP {
    RfK k;
    unsigned tab[kTab];      // 3x3: the chunk table, format kFmt
};

template <int GB, int NW, int MAXS, int KS>
__global__ __launch_bounds__(NW * 64) void k_conv_rf(RfP q) {
    extern __shared__ __attribute__((aligned(16))) float lds[];      // [NW][GB][64 lanes][4] partial tiles
    CONV_TR(g_trace_rf, 0); CONV_TRR(g_trace_rf, 1);
    RfK p = q.k;
    // all scalar arguments are wanted HERE: one batch of scalar loads, one wait
    asm volatile("" :: "s"(p.in), "s"(p.w), "s"(p.scale), "s"(p.shift), "s"(p.add), "s"(p.out), "s"(p.colsum), "s"(p.in_bytes), "s"(p.w_bytes),
                 "s"(p.sc_bytes), "s"(p.add_bytes), "s"(p.M), "s"(p.K), "s"(p.Cout), "s"(p.Cout16), "s"(p.nchunks), "s"(p.nb));
    asm volatile("" :: "s"(p.irow0), "s"(p.H), "s"(p.W), "s"(p.Ho), "s"(p.Wo), "s"(p.in_ld), "s"(p.in_coff), "s"(p.stride), "s"(p.pad), "s"(p.out_ld),
                 "s"(p.out_coff), "s"(p.relu_cout), "s"(p.add_H), "s"(p.add_W), "s"(p.add_ld), "s"(p.add_coff), "s"(p.xmap), "s"(p.gx), "s"(p.gy),
                 "s"(p.inv_hw), "s"(p.inv_wo), "s"(p.inv_gx), "s"(p.inv_gy));
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int bx, by;
    tile_of_block_rcp(p, bx, by);
    const int m0 = bx * 16, n0 = by * (16 * GB);
    const int r16 = lane & 15, kq = lane >> 4;
    const int bias = window_bias(p);
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(p.w, p.w_bytes), ri = make_pixel_rsrc(p, bias);

    // ---- weight side first: needs only the block's coordinates, and its requests cover the latency of everything below
    unsigned b_off[GB];
#pragma unroll
    for (int j = 0; j < GB; ++j) {
        const int n = n0 + j * 16 + r16;
        b_off[j] = n < p.Cout16 ? (unsigned)((n * p.K + kq * 4) * 4) : kOOB;
    }
    // this wave's chunks: the contiguous range [wave * nst, (wave + 1) * nst) of the K axis, one chunk per step
    const int nst = p.nb * MAXS;                                     // steps per wave (the last ones of the last waves may be empty)
    int w_c = wave * nst;
    f32x4 af[MAXS], bf[MAXS][GB];
    {
        const unsigned s_b = (unsigned)w_c * 64u;
#pragma unroll
        for (int t = 0; t < MAXS; ++t)
#pragma unroll
            for (int j = 0; j < GB; ++j) bf[t][j] = bload(rw, b_off[j] + (unsigned)(t * 64), s_b);
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- pixel side: ONE row per lane (r16), decoded with float reciprocals
    const int m = m0 + r16;
    const int hw = p.Ho * p.Wo;
    Pixel px = {0, 0, 0};
    unsigned tapmask = 0u;                                           // bit dy * KS + dx: that tap of this lane's window lies inside the image
    unsigned a_voff = kOOB;                                          // bias + byte offset of the window's first pixel, channel in_coff + kq * 4
    if (m < p.M) {
        px = pixel_of_row(p, m, hw);
        CONV_WINDOW_OF_PIXEL(KS, p, px, kq, bias, tapmask, a_voff);
    }
    // epilogue operands of the lanes that will finish a tile (waves 0 .. GB-1: tile j2 = wave, pixel r16, channel quad kq): requested
    // through range-checked descriptors (a channel beyond Cout reads 0), behind the main loads -- no branch, no wait of their own
    const int en = n0 + wave * 16 + kq * 4;
    const bool e_on = wave < GB && m < p.M && en < p.Cout;
    const __amdgpu_buffer_rsrc_t rsc = make_rsrc(p.scale, p.scale ? p.sc_bytes : 0u), rsh = make_rsrc(p.shift, p.shift ? p.sc_bytes : 0u);
    const __amdgpu_buffer_rsrc_t rad = make_rsrc(p.add, p.add ? p.add_bytes : 0u);
    const unsigned e_voff = e_on ? (unsigned)(en * 4) : kOOB;
    const unsigned e_aoff = e_on ? (unsigned)(addend_index(p, px, en) * 4) : kOOB;

    f32x4 acc[2][GB];                                                // even / odd steps: two independent accumulation chains
#pragma unroll
    for (int j = 0; j < GB; ++j) acc[0][j] = acc[1][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 e_sc = {1.f, 1.f, 1.f, 1.f}, e_sh = {0.f, 0.f, 0.f, 0.f}, e_add = {0.f, 0.f, 0.f, 0.f};
    CONV_TR(g_trace_rf, 2);
    for (int bt = 0; bt < p.nb; ++bt) {
        // ---- request the batch.  Weights (the first batch's are in flight already): one scalar base per batch, the step is an
        // instruction offset (t * 64 bytes) -- no per-step instruction besides the load.  Pixels: 1x1 layers the same (+ a select that
        // zeroes the steps beyond K); 3x3 layers read (offset | tap) of the chunk from the table in the kernel arguments.
        const unsigned s_b = (unsigned)w_c * 64u;
        if (bt > 0) {
#pragma unroll
            for (int t = 0; t < MAXS; ++t)
#pragma unroll
                for (int j = 0; j < GB; ++j) bf[t][j] = bload(rw, b_off[j] + (unsigned)(t * 64), s_b);
        }
#pragma unroll
        for (int t = 0; t < MAXS; ++t) {
            if constexpr (KS == 1) {
                const bool live = w_c + t < p.nchunks;               // a step beyond K multiplies (finite or zero) weights by zeros
                af[t] = bload(ri, (live ? a_voff : kOOB) + (unsigned)(t * 64), s_b);
            } else {
                const unsigned e = q.tab[w_c + t];
                const bool ok = (tapmask & (1u << chunk_tap(kFmt, e))) != 0u;
                af[t] = bload(ri, ok ? a_voff : kOOB, chunk_off(kFmt, e));
            }
        }
        w_c += MAXS;
        if (bt == p.nb - 1) {                                        // (uniform) the epilogue's operands ride behind the last batch
            if (p.scale) e_sc = bload(rsc, e_voff, 0u);
            if (p.shift) e_sh = bload(rsh, e_voff, 0u);
            if (p.add) e_add = bload(rad, e_aoff, 0u);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (bt == 0) CONV_TR(g_trace_rf, 3);
        // ---- multiply as the fragments land (the compiler counts the waits: loads return in order)
#pragma unroll
        for (int t = 0; t < MAXS; ++t) {
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                for (int j = 0; j < GB; ++j)
                    acc[t & 1][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[t][j][tt], af[t][tt], acc[t & 1][j], 0, 0, 0);   // D^T: lane = pixel
            if (bt == 0 && t == 0) CONV_TR(g_trace_rf, 4);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    CONV_TR(g_trace_rf, 5);

    // ---- the NW partial tiles meet in LDS; waves 0 .. GB-1 finish one 16x16 tile each
#pragma unroll
    for (int j = 0; j < GB; ++j) *reinterpret_cast<f32x4*>(lds + ((wave * GB) + j) * 256 + lane * 4) = acc[0][j] + acc[1][j];
    __syncthreads();
    CONV_TR(g_trace_rf, 6);
    if (wave < GB) {
        f32x4 a;
        CONV_SUM_WAVE_TILES(a, NW, lds, GB, wave, lane)
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (e_on) {
            if (!p.scale) e_sc = f32x4{1.f, 1.f, 1.f, 1.f};
            v = a * e_sc + e_sh + e_add;
            CONV_RELU_ZERO4(v, en, p.relu_cout, p.Cout)
            float* o = p.out + (size_t)m * p.out_ld + p.out_coff + en;
            const bool vec_ok = CONV_OUT_VEC_OK(p, false);
            CONV_STORE4_F32(o, v, vec_ok, en, p.Cout)
        }
        if (p.colsum) {                                              // column sums of the tile: the 16 pixel lanes of a channel quad
            CONV_COLSUM16(v)
            if (r16 == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int n = n0 + wave * 16 + kq * 4 + r;
                    if (n < p.Cout16) p.colsum[(size_t)bx * p.Cout16 + n] = v[r];
                }
            }
        }
    }
    CONV_TR(g_trace_rf, 8);
#ifdef ORE_TRACE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    CONV_TR(g_trace_rf, 9); CONV_TRR(g_trace_rf, 10);
#endif
}

template <int GB, int NW, int MAXS>
int rf_go(const RfP& q, bool k3, dim3 grid, hipStream_t st) {
    constexpr size_t lds = (size_t)(NW * GB * 256) * sizeof(float);
    if (!k3) hipLaunchKernelGGL((k_conv_rf<GB, NW, MAXS, 1>), grid, dim3(NW * 64), lds, st, q);
    else hipLaunchKernelGGL((k_conv_rf<GB, NW, MAXS, 3>), grid, dim3(NW * 64), lds, st, q);
    return ore_launch_status("k_conv_rf");
}

}  // namespace

namespace oreconv {

// k_conv_rf: build (GB, NW, MAXS) = pl.build[0..2]
int launch_rf(const ConvP& p, const ConvPlan& pl, hipStream_t st) {
    const int gb = pl.build[0], nw = pl.build[1], maxs = pl.build[2];
    const int steps = ceil_div(p.nchunks, nw);
    RfP q;
    Lvl L;
    fill_desc_args(q.k, p, pl, L);
    q.k.nb = ceil_div(steps, maxs);
    build_chunk_table(q.tab, kTab, p, L, kFmt);
    const bool k3 = p.kh == 3;
    const dim3 grid(pl.gx, pl.gy, 1);
#define RF_GO(g, w, s) if (gb == g && nw == w && maxs == s) return rf_go<g, w, s>(q, k3, grid, st);
    ORE_RF_BUILDS(RF_GO)
#undef RF_GO
    return ORE_EINVAL;
}

}  // namespace oreconv

CONV_TRACE_SETTER(ore_debug_set_trace_rf, g_trace_rf)
