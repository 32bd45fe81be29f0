// k_conv_kd -- implicit-GEMM NHWC convolution for the small / medium-M layers (stages 4-5, the FPN laterals, conv3, the concat convs:
// M = 400 .. 8400 rows at batch 1), fp32 MFMA (v_mfma_f32_16x16x4_f32), fed by LDS-DMA through BUFFER descriptors.
//
// Round 4.  The phase traces of k_conv_kw (profiles/r04_kw_phase_trace.txt) show its K loop at ~850 clocks per 16-channel step whatever
// the ring depth: not memory latency but ~140 instructions of tap walk, 64-bit pointer rebuilds and ring bookkeeping per step, issued by
// one wave per SIMD.  The load-shape micro-benchmark (profiles/r04_load_issue_bench.txt) shows what the memory side can do from one CU:
// 55 B/clk through LDS-DMA in 16 x 64-byte segments per instruction (58 clocks per instruction), 23 B/clk for the fragment-shaped
// register loads of k_conv_rf.  This kernel keeps k_conv_kw's data path (coalesced segments -> LDS image with the XOR swizzle on the
// source address -> ds_read_b128 fragments) and k_conv_rf's addressing:
//   * `buffer_load_dwordx4 ... lds` through range-checked descriptors (the addressing layer of ore_conv_desc.h; what is out of range
//     lands in LDS as zeros): ~6 instructions per piece and step;
//   * a wave owns a CONTIGUOUS range of the K axis and works in batches of SB steps on a double-buffered private LDS region: the DMAs of
//     batch b+1 are in flight while batch b is multiplied; waits are counted (`s_waitcnt vmcnt`), there is no barrier in the K loop.
// K is split over the NW waves of a block, partial tiles meet in LDS, epilogue = ore_conv_epilogue.h's (scale / shift, FPN top-down add,
// ReLU, per-tile column sums, channel-slice output).  Single level, fp32 storage, no input affine.
//
// Replaces F.conv2d + FrozenBatchNorm2d + ReLU / bias of d2z:modeling/backbone/vovnet.py:205-219,310-332 (stages 3-5), fpn.py:126-145
// (laterals), ref:fewx/modeling/fsod/fsod_cen.py:470 (conv3) at batch 1.
#include "ore_conv_desc.h"
#include "ore_conv_epilogue.h"

namespace {
using namespace oreconv;

CONV_TRACE_SYMBOL(g_trace_kd)
constexpr int kTab = kKdTab;                      // chunk table entries
constexpr ChunkFmt kFmt = kChunkTapHigh;

struct KdK {
    const float* in; const float* w; const float* scale; const float* shift; const float* add; float* out; float* colsum;
    unsigned in_bytes, w_bytes, sc_bytes, add_bytes;      // num_records of the buffer descriptors
    int M, K, Cout, Cout16, nchunks, nb;
    int irow0, H, W, Ho, Wo, in_ld, in_coff, stride, pad;
    int out_ld, out_coff, relu_cout, add_H, add_W, add_ld, add_coff;
    int xmap, gx, gy;
    float inv_hw, inv_wo, inv_gx, inv_gy;
    int sb;                  // bf16 STORAGE (ConvP::sb): bit 0 in / w are bf16 (sizes above in 4-byte units), bit 1 out is bf16, bit 2 add is bf16
};
struct KdP {
    KdK k;
    unsigned tab[kTab];      // 3x3: the chunk table, format kFmt
};

template <int GA, int GB, int NW, int SB, int KS, bool SBF = false>
__global__ __launch_bounds__(NW * 64) void k_conv_kd(KdP q) {
    constexpr int T = NW * 64;
    constexpr int G = GA + GB;                                    // DMA pieces (16-row groups) per step
    constexpr int STAGE_F = G * 256;                              // floats per step
    constexpr int HALF_F = SB * STAGE_F;                          // one batch
    constexpr int WAVE_F = 2 * HALF_F;                            // double-buffered private region of a wave
    constexpr int NT = GA * GB;
    static_assert(SB * G <= 63, "a batch must fit the vmcnt counter");
    extern __shared__ __attribute__((aligned(16))) float lds[];   // max(NW * WAVE_F, NW * NT * 256) + NT * 16 floats
    CONV_TR(g_trace_kd, 0); CONV_TRR(g_trace_kd, 1);
    KdK p = q.k;
    asm volatile("" :: "s"(p.in), "s"(p.w), "s"(p.scale), "s"(p.shift), "s"(p.add), "s"(p.out), "s"(p.colsum), "s"(p.in_bytes), "s"(p.w_bytes),
                 "s"(p.sc_bytes), "s"(p.add_bytes), "s"(p.M), "s"(p.K), "s"(p.Cout), "s"(p.Cout16), "s"(p.nchunks), "s"(p.nb));
    asm volatile("" :: "s"(p.irow0), "s"(p.H), "s"(p.W), "s"(p.Ho), "s"(p.Wo), "s"(p.in_ld), "s"(p.in_coff), "s"(p.stride), "s"(p.pad), "s"(p.out_ld),
                 "s"(p.out_coff), "s"(p.relu_cout), "s"(p.add_H), "s"(p.add_W), "s"(p.add_ld), "s"(p.add_coff), "s"(p.xmap), "s"(p.gx), "s"(p.gy),
                 "s"(p.inv_hw), "s"(p.inv_wo), "s"(p.inv_gx), "s"(p.inv_gy), "s"(p.sb));
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int bx, by;
    tile_of_block_rcp(p, bx, by);
    const int m0 = bx * (16 * GA), n0 = by * (16 * GB);
    const int bias = window_bias(p);
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(p.w, p.w_bytes), ri = make_pixel_rsrc(p, bias);

    // ---- per-lane DMA sources: lane L of a piece fills LDS slot L = (row L >> 2, physical quad L & 3) with logical quad (L & 3) ^ swz(row)
    const int r16 = lane >> 2, lq = (lane & 3) ^ swz(r16);
    unsigned b_voff[GB];
#pragma unroll
    for (int j = 0; j < GB; ++j) {
        const int n = n0 + j * 16 + r16;
        b_voff[j] = n < p.Cout16 ? (unsigned)((n * p.K + lq * 4) * 4) : kOOB;
    }
    const int hw = p.Ho * p.Wo;
    unsigned a_voff[GA], a_taps[GA];
#pragma unroll
    for (int i = 0; i < GA; ++i) {
        const int m = m0 + i * 16 + r16;
        a_voff[i] = kOOB; a_taps[i] = 0u;
        if (m < p.M) {
            const Pixel px = pixel_of_row(p, m, hw);
            CONV_WINDOW_OF_PIXEL(KS, p, px, lq, bias, a_taps[i], a_voff[i]);
        }
    }
    // this wave's chunks: the contiguous range [wave * nst, (wave + 1) * nst), SB steps per batch, nb batches
    const int nst = p.nb * SB;
    int w_c = wave * nst;
    float* ring = lds + wave * WAVE_F;

    auto issue = [&](float* half) {                               // the SB steps starting at chunk w_c -> `half`
        const unsigned s_b = (unsigned)w_c * 64u;                 // this batch inside a weight row / a pixel's channel vector
#pragma unroll
        for (int t = 0; t < SB; ++t) {
            float* dst = half + t * STAGE_F;
            const bool live = w_c + t < p.nchunks;                // a step beyond K stages zeros on both sides (descriptor range check via kOOB:
                                                                  // the scalar offset of a step is NOT range-checked, a weight row read past K would run
                                                                  // off the end of the tensor for the last output channel)
            if constexpr (KS == 1) {
#pragma unroll
                for (int i = 0; i < GA; ++i) {
                    const unsigned v = live ? a_voff[i] : kOOB;
                    switch (t) {                                   // the step rides in the instruction offset
#define KD_A(tt) case tt: dma<tt * 64>(ri, dst + i * 256, v, s_b); break;
                        KD_A(0) KD_A(1) KD_A(2) KD_A(3) KD_A(4) KD_A(5) KD_A(6) KD_A(7) KD_A(8) KD_A(9) KD_A(10) KD_A(11) KD_A(12) KD_A(13) KD_A(14) KD_A(15)
#undef KD_A
                    }
                }
            } else {
                const unsigned e = q.tab[w_c + t];
                const unsigned bit = 1u << chunk_tap(kFmt, e);
#pragma unroll
                for (int i = 0; i < GA; ++i) dma<0>(ri, dst + i * 256, (a_taps[i] & bit) ? a_voff[i] : kOOB, chunk_off(kFmt, e));
            }
#pragma unroll
            for (int j = 0; j < GB; ++j) {
                switch (t) {
#define KD_B(tt) case tt: dma<tt * 64>(rw, dst + (GA + j) * 256, live ? b_voff[j] : kOOB, s_b); break;
                    KD_B(0) KD_B(1) KD_B(2) KD_B(3) KD_B(4) KD_B(5) KD_B(6) KD_B(7) KD_B(8) KD_B(9) KD_B(10) KD_B(11) KD_B(12) KD_B(13) KD_B(14) KD_B(15)
#undef KD_B
                }
            }
        }
        w_c += SB;
    };

    // small tiles: even / odd steps accumulate into two independent chains (a dependent fp32 MFMA waits 40 clocks for its predecessor);
    // tiles of 4+ MFMA tiles have enough independent accumulators as they are
    constexpr int NACC = GA * GB >= 4 ? 1 : 2;
    f32x4 acc[NACC][GA][GB];
#pragma unroll
    for (int a = 0; a < NACC; ++a)
#pragma unroll
        for (int i = 0; i < GA; ++i)
#pragma unroll
            for (int j = 0; j < GB; ++j) acc[a][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // fragment read offsets (floats) inside a 16-row group: row = lane & 15, logical quad = lane >> 4
    const int frow = lane & 15;
    const int foff = frow * 16 + (((lane >> 4) ^ swz(frow)) << 2);
    CONV_TR(g_trace_kd, 2);
    issue(ring);
    CONV_TR(g_trace_kd, 3);
    // epilogue operands of this thread's items (below): requested now, behind the first batch, consumed after the K loop
    // (range-checked descriptors: a channel beyond Cout reads 0, an absent operand reads its neutral value)
    for (int bt = 0; bt < p.nb; ++bt) {
        const float* cur = ring + (bt & 1) * HALF_F;
        if (bt + 1 < p.nb) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // the other half's fragment reads (batch bt-1) have retired
            issue(ring + ((bt + 1) & 1) * HALF_F);
            wait_vmcnt<SB * G>();                                 // batch bt has landed (all but the youngest batch)
        } else {
            wait_vmcnt<0>();
        }
        if (bt == 0) CONV_TR(g_trace_kd, 4);
        // fragments of step t+1 are requested before the MFMAs of step t issue (two register sets)
        f32x4 af[2][GA], bf[2][GB];
#pragma unroll
        for (int i = 0; i < GA; ++i) af[0][i] = *reinterpret_cast<const f32x4*>(cur + i * 256 + foff);
#pragma unroll
        for (int j = 0; j < GB; ++j) bf[0][j] = *reinterpret_cast<const f32x4*>(cur + (GA + j) * 256 + foff);
#pragma unroll
        for (int t = 0; t < SB; ++t) {
            if (t + 1 < SB) {
                const float* st = cur + (t + 1) * STAGE_F;
#pragma unroll
                for (int i = 0; i < GA; ++i) af[(t + 1) & 1][i] = *reinterpret_cast<const f32x4*>(st + i * 256 + foff);
#pragma unroll
                for (int j = 0; j < GB; ++j) bf[(t + 1) & 1][j] = *reinterpret_cast<const f32x4*>(st + (GA + j) * 256 + foff);
            }
            __builtin_amdgcn_sched_barrier(0);                    // (keep the next step's reads in front of this step's MFMAs)
            if constexpr (SBF) {                                  // bf16 storage: the 64-byte row of a fragment is 32 channels, one MFMA per step
#pragma unroll
                for (int i = 0; i < GA; ++i)
#pragma unroll
                    for (int j = 0; j < GB; ++j)
                        acc[t & (NACC - 1)][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, bf[t & 1][j]), __builtin_bit_cast(bf16x8_t, af[t & 1][i]),
                                                                                            acc[t & (NACC - 1)][i][j], 0, 0, 0);
            } else {
#pragma unroll
                for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                    for (int i = 0; i < GA; ++i)
#pragma unroll
                        for (int j = 0; j < GB; ++j)
                            acc[t & (NACC - 1)][i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[t & 1][j][tt], af[t & 1][i][tt], acc[t & (NACC - 1)][i][j], 0, 0, 0);   // D^T: lane = pixel
            }
        }
    }
    CONV_TR(g_trace_kd, 5);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();                                              // every wave's ring is dead: the partial tiles take its place
    CONV_TR(g_trace_kd, 6);
#pragma unroll
    for (int i = 0; i < GA; ++i)
#pragma unroll
        for (int j = 0; j < GB; ++j)
            *reinterpret_cast<f32x4*>(lds + ((wave * NT) + i * GB + j) * 256 + lane * 4) = NACC == 2 ? acc[0][i][j] + acc[NACC - 1][i][j] : acc[0][i][j];
    __syncthreads();
    CONV_TR(g_trace_kd, 7);
    constexpr int RED_F = NW * NT * 256;
    float* cs = lds + RED_F;
    const __amdgpu_buffer_rsrc_t rsc = make_rsrc(p.scale, p.scale ? p.sc_bytes : 0u), rsh = make_rsrc(p.shift, p.shift ? p.sc_bytes : 0u);
    const __amdgpu_buffer_rsrc_t rad = make_rsrc(p.add, p.add ? p.add_bytes : 0u);
    const bool vec_ok = CONV_OUT_VEC_OK(p, p.sb & 2);
#pragma unroll
    for (int q0 = 0; q0 < NT * 64; q0 += T) {
        const int it = q0 + tid;                                  // a wave's 64 items are one 16x16 tile: lane = accumulator lane
        if (it < NT * 64) {
            const int tl = it >> 6, ln = it & 63;
            const int j2 = tl % GB, i2 = tl / GB;
            const int m = m0 + i2 * 16 + (ln & 15), en = n0 + j2 * 16 + (ln >> 4) * 4;
            const bool on = m < p.M && en < p.Cout;
            f32x4 e_sc = {1.f, 1.f, 1.f, 1.f}, e_sh = {0.f, 0.f, 0.f, 0.f}, e_add = {0.f, 0.f, 0.f, 0.f};
            const unsigned ev = on ? (unsigned)(en * 4) : kOOB;
            if (p.scale) e_sc = bload4(rsc, ev);
            if (p.shift) e_sh = bload4(rsh, ev);
            if (p.add) {
                const unsigned ai = (unsigned)addend_index(p, pixel_of_row(p, m, hw), en);
                if (p.sb & 4) {                                   // bf16 addend: four channels = 8 bytes
                    const u32x2 h = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rad, on ? (int)(ai * 2u) : (int)kOOB, 0, 0));
                    e_add = from_bf16x4(__builtin_bit_cast(s16x4, h));
                } else {
                    e_add = bload4(rad, on ? ai * 4u : kOOB);
                }
            }
            f32x4 a;
            CONV_SUM_WAVE_TILES(a, NW, lds, NT, tl, ln)
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (on) {
                v = a * e_sc + e_sh + e_add;
                CONV_RELU_ZERO4(v, en, p.relu_cout, p.Cout)
                if (p.sb & 2) {                                   // bf16 output tensor
                    CONV_STORE4_BF16(reinterpret_cast<unsigned short*>(p.out) + (size_t)m * p.out_ld + p.out_coff + en, v, vec_ok, en, p.Cout)
                    CONV_ZERO_PAST4(v, en, p.Cout)
                } else {
                    float* o = p.out + (size_t)m * p.out_ld + p.out_coff + en;
                    CONV_STORE4_F32(o, v, vec_ok, en, p.Cout)
                }
            }
            if (p.colsum) {                                       // column sums of the tile: the 16 pixel lanes of a channel quad
                CONV_COLSUM16(v)
                if ((ln & 15) == 0) *reinterpret_cast<f32x4*>(cs + tl * 16 + (ln >> 4) * 4) = v;
            }
        }
    }
    if (p.colsum) {
        __syncthreads();
        if (tid < GB * 16) {                                      // sum the block's GA row tiles in order -> one partial row per block
            const int j2 = tid >> 4, ch = tid & 15;
            float sacc = cs[j2 * 16 + ch];
#pragma unroll
            for (int i2 = 1; i2 < GA; ++i2) sacc += cs[(i2 * GB + j2) * 16 + ch];
            const int n = n0 + j2 * 16 + ch;
            if (n < p.Cout16) p.colsum[(size_t)bx * p.Cout16 + n] = sacc;
        }
    }
    CONV_TR(g_trace_kd, 8);
#ifdef ORE_TRACE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    CONV_TR(g_trace_kd, 9); CONV_TRR(g_trace_kd, 10);
#endif
}

template <int GA, int GB, int NW, int SB, bool SBF>
int kd_go(const KdP& q, bool k3, dim3 grid, hipStream_t st) {
    constexpr size_t ring = (size_t)NW * 2 * SB * (GA + GB) * 256, red = (size_t)NW * GA * GB * 256;
    constexpr size_t lds = ((ring > red ? ring : red) + GA * GB * 16) * sizeof(float);
    static_assert(lds <= 160 * 1024 && SB * (GA + GB) <= 63, "k_conv_kd build beyond the LDS / DMA-offset limits");
    static bool attr1 = false, attr3 = false;
    if (!k3) {
        if (!attr1) { ORE_HIP(hipFuncSetAttribute((const void*)k_conv_kd<GA, GB, NW, SB, 1, SBF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); attr1 = true; }
        hipLaunchKernelGGL((k_conv_kd<GA, GB, NW, SB, 1, SBF>), grid, dim3(NW * 64), lds, st, q);
    } else {
        if (!attr3) { ORE_HIP(hipFuncSetAttribute((const void*)k_conv_kd<GA, GB, NW, SB, 3, SBF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); attr3 = true; }
        hipLaunchKernelGGL((k_conv_kd<GA, GB, NW, SB, 3, SBF>), grid, dim3(NW * 64), lds, st, q);
    }
    return ore_launch_status("k_conv_kd");
}

}  // namespace

namespace oreconv {

// k_conv_kd: the plan's tile, waves (build[0]) and steps per batch (build[1]) over p's rows (several levels of a 1x1 layer: one flat GEMM)
int launch_kd(const ConvP& p, const ConvPlan& pl, hipStream_t st) {
    const int nw = pl.build[0], sb = pl.build[1];
    const int steps = ceil_div(p.nchunks, nw);
    KdP q;
    Lvl L;
    fill_desc_args(q.k, p, pl, L);
    q.k.nb = ceil_div(steps, sb);
    q.k.sb = p.sb;
    build_chunk_table(q.tab, kTab, p, L, kFmt);
    const bool k3 = p.kh == 3;
    const dim3 grid(pl.gx, pl.gy, 1);
#define KD_GO(bm_, bn_, nw_, sb_) if (pl.bm == bm_ && pl.bn == bn_ && nw == nw_ && sb == sb_) \
        return (p.sb & 1) ? kd_go<bm_ / 16, bn_ / 16, nw_, sb_, true>(q, k3, grid, st) : kd_go<bm_ / 16, bn_ / 16, nw_, sb_, false>(q, k3, grid, st);
    ORE_KD_BUILDS(KD_GO)
#undef KD_GO
    return ORE_EINVAL;
}

}  // namespace oreconv

CONV_TRACE_SETTER(ore_debug_set_trace_kd, g_trace_kd)
