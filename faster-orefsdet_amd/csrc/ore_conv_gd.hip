// k_conv_gd -- implicit-GEMM NHWC convolution, fp32 MFMA (v_mfma_f32_16x16x4_f32), shared-stage LDS-DMA through buffer descriptors.
// Serves (bs = 1 plan): stem_3 (3x3 stride 2), the stage-2 / 3 concat 1x1 convs (M = 6400 .. 25600 rows), the stage-3 FPN lateral (with
// its top-down add), conv3 over the three pyramid levels as one flat GEMM, and -- with K split over blockIdx.z -- the second-stage GEMM.
//
// Round 4.  k_conv_gs / k_conv_igemm ran the large layers at 36-48 % of the fp32 MFMA peak, and round 2's counters said why: 87 VALU + 82
// SALU instructions per 28 MFMAs per step -- the matrix pipe waits for instruction issue, not for data.  k_conv_kd showed the cure on
// the small layers (the descriptor addressing of ore_conv_desc.h) but its K-split blocks tie here, because their partial tiles meet in
// LDS and one block owns a CU.  This kernel puts the same addressing into the SHARED-stage structure:
//   * the NW = 4 or 8 waves of a block tile its BM x BN output (WGM x WGN waves) and share every staged 16-channel chunk: a chunk is
//     (BM + BN) / 16 DMA pieces of 1 KiB, piece p is issued by wave p % NW (`buffer_load_dwordx4 ... lds`, XOR swizzle on the source
//     offset as in k_conv_kw), an NS-deep ring, ONE raw barrier per chunk: a wave waits for its own pieces of chunk t (counted vmcnt,
//     later chunks stay in flight), the barrier publishes everybody's;
//   * the chunk loop is unrolled NS times (NS even) so that ring slots and LDS addresses are immediates; in step t a wave reads chunk t's
//     fragments (ds_read_b128) into one register set and multiplies chunk t-1 from the other, and its refill pieces for chunk
//     t + NS - 1 go out BETWEEN those MFMAs (a DMA instruction holds the wave at issue while the texture addresser works off its queue);
//   * no cross-wave reduction: every wave finishes its own tiles from registers (scale / shift / ReLU / top-down add, 16-byte stores); the
//     per-tile column sums of the eSE pool are reduced by shuffles + one LDS hop.
// What bounds it (profiles/r04_gd_ablation.txt): the MFMA loop with prologue and epilogue is 38 of stem_3's 45 us,
// staging adds ~6 instead of hiding, the barriers <= 2; every tiling lands within ~10 % of the others.
// fp32 storage, no input affine; a single level (with the FPN top-down addend if the layer has one) or several levels of a 1x1 layer as
// one flat GEMM.
//
// Replaces F.conv2d + FrozenBatchNorm2d + ReLU of d2z:modeling/backbone/vovnet.py:205-219 (stem_3), :310-332 (the concat convs);
// d2z:modeling/backbone/fpn.py:130-150 (lateral 3); ref:fewx/modeling/fsod/fsod_cen.py conv3 after the correlation;
// d2z:modeling/roi_heads/box_head.py fc1 (conv_gd_splitk).
#include "ore_conv_desc.h"
#include "ore_conv_epilogue.h"

namespace {
using namespace oreconv;

constexpr int kTab = kGdTab;                      // chunk table entries
constexpr ChunkFmt kFmt = kChunkTapLow;

struct GdK {
    const float* in; const float* w; const float* scale; const float* shift; const float* add; float* out; float* colsum;
    unsigned in_bytes, w_bytes, sc_bytes, add_bytes;
    int M, K, Cout, Cout16, nchunks;
    int irow0, H, W, Ho, Wo, in_ld, in_coff, stride, pad;
    int out_ld, out_coff, relu_cout, add_H, add_W, add_ld, add_coff;
    int zc_stride, out_zstride;   // K split over blockIdx.z: slice z stages chunks z * zc_stride + [0, nchunks) and writes raw sums at out + z * out_zstride (0, 0: no split)
    int xmap, gx, gy;
    float inv_hw, inv_wo, inv_gx, inv_gy;
#ifdef ORE_TRACE
    int dbg;                 // ablation (trace build only): 1 no MFMAs, 2 no DMA in the loop, 4 no fragment reads, 8 no barrier, 16 no stores, 32 no prologue DMA
#endif
};
struct GdP {
    GdK k;
    unsigned tab[kTab];      // 3x3: the chunk table, format kFmt
};

template <int GA, int GB, int WGM, int WGN, int NS, int KS, bool BF = false>
__global__ __launch_bounds__(64 * WGM * WGN) void k_conv_gd(GdP q) {
    constexpr int NW = WGM * WGN;                     // 4 waves, or 8 (two per SIMD: the builds whose blocks own a CU alone)
    static_assert((NW == 4 || NW == 8) && GA % WGM == 0 && GB % WGN == 0, "the waves tile the block");
    constexpr int G = GA + GB;                        // DMA pieces per chunk
    constexpr int PPW = (G + NW - 1) / NW;            // pieces a wave issues per chunk (piece p -> wave p % NW)
    constexpr int STAGE_F = G * 256;
    constexpr int TA = GA / WGM, TB = GB / WGN;       // MFMA tiles of a wave
    static_assert(PPW * (NS - 1) <= 63, "vmcnt");
    extern __shared__ __attribute__((aligned(16))) float lds[];      // NS * STAGE_F floats (+ the column-sum scratch, reusing the ring)
    GdK p = q.k;
    asm volatile("" :: "s"(p.in), "s"(p.w), "s"(p.scale), "s"(p.shift), "s"(p.add), "s"(p.out), "s"(p.colsum), "s"(p.in_bytes), "s"(p.w_bytes), "s"(p.sc_bytes), "s"(p.add_bytes),
                 "s"(p.M), "s"(p.K), "s"(p.Cout), "s"(p.Cout16), "s"(p.nchunks), "s"(p.irow0), "s"(p.H), "s"(p.W), "s"(p.Ho), "s"(p.Wo));
    asm volatile("" :: "s"(p.in_ld), "s"(p.in_coff), "s"(p.stride), "s"(p.pad), "s"(p.out_ld), "s"(p.out_coff), "s"(p.relu_cout), "s"(p.add_H), "s"(p.add_W), "s"(p.add_ld), "s"(p.add_coff), "s"(p.zc_stride), "s"(p.out_zstride), "s"(p.xmap), "s"(p.gx),
                 "s"(p.gy), "s"(p.inv_hw), "s"(p.inv_wo), "s"(p.inv_gx), "s"(p.inv_gy));
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WGN, wn = wave % WGN;
    int bx, by;
    tile_of_block_rcp(p, bx, by);
    const int m0 = bx * (16 * GA), n0 = by * (16 * GB);
    const int bias = window_bias(p);
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(p.w, p.w_bytes), ri = make_pixel_rsrc(p, bias);

    // ---- this wave's DMA pieces: piece index pw + 4 s (s < PPW); pieces 0 .. GA-1 are pixel groups, GA .. G-1 weight-row groups
    const int r16 = lane >> 2, lq = (lane & 3) ^ swz(r16);
    const int hw = p.Ho * p.Wo;
    unsigned pv[PPW], ptaps[PPW];                     // per-lane byte offset (or kOOB) and, for pixel pieces, the 9-bit tap mask
#pragma unroll
    for (int s = 0; s < PPW; ++s) {
        const int pi = wave + NW * s;
        pv[s] = kOOB; ptaps[s] = 0u;
        if (pi < GA) {
            const int m = m0 + pi * 16 + r16;
            if (m < p.M) {
                const Pixel px = pixel_of_row(p, m, hw);
                CONV_WINDOW_OF_PIXEL(KS, p, px, lq, bias, ptaps[s], pv[s]);
            }
        } else if (pi < G) {
            const int n = n0 + (pi - GA) * 16 + r16;
            if (n < p.Cout16) pv[s] = (unsigned)((n * p.K + lq * 4) * 4);
        }
    }
    const int zc0 = (int)blockIdx.z * p.zc_stride;
    // issue piece s of this wave's pieces of chunk c into ring slot `slot` (s, slot: constants after unrolling)
    auto issue_piece = [&](int c, int slot, int s) {
        float* dst = lds + slot * STAGE_F;
        const bool live = c < p.nchunks;
        const int cz = c + zc0;                                            // the chunk's place in K (zc0 = 0 without a K split)
        unsigned e = chunk_entry(kFmt, 0u, kNoTap);
        if constexpr (KS != 1) e = q.tab[cz < kTab ? cz : kTab - 1];
        const unsigned bit = 1u << chunk_tap(kFmt, e);
        const int pi = wave + NW * s;                                      // wave-uniform
        if (pi < GA) {
            if constexpr (KS == 1) dma<0>(ri, dst + pi * 256, live ? pv[s] : kOOB, (unsigned)cz * 64u);
            else dma<0>(ri, dst + pi * 256, (live && (ptaps[s] & bit)) ? pv[s] : kOOB, chunk_off(kFmt, e));
        } else if (pi < G) {
            dma<0>(rw, dst + pi * 256, live ? pv[s] : kOOB, (unsigned)cz * 64u);
        }
    };
    auto issue = [&](int c, int slot) {
#pragma unroll
        for (int s = 0; s < PPW; ++s) issue_piece(c, slot, s);
    };

    f32x4 acc[TA][TB];
#pragma unroll
    for (int i = 0; i < TA; ++i)
#pragma unroll
        for (int j = 0; j < TB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int frow = lane & 15;
    const int foff = frow * 16 + (((lane >> 4) ^ swz(frow)) << 2);
    const bool full = wave + NW * (PPW - 1) < G;       // this wave issues PPW pieces per chunk (else PPW - 1); wave-uniform
    // ---- prologue: NS - 1 chunks in flight
#ifdef ORE_TRACE
    if (!(q.k.dbg & 32))
#endif
#pragma unroll
    for (int u = 0; u < NS - 1; ++u) issue(u, u);
    // Chunk loop, unrolled NS times (NS even): step t waits for chunk t's pieces, passes the barrier, refills the slot chunk t-1 was
    // read from, reads chunk t's fragments into one register set and runs chunk t-1's MFMAs from the other -- a block may own its CU
    // alone (one wave per SIMD), so the fragment reads, the DMA issue and the barrier skew have to hide behind this wave's own MFMAs.
    // nchunks + 1 steps: the last one only multiplies.
    static_assert(NS % 2 == 0, "two fragment register sets alternate inside the unrolled group");
    f32x4 af[2][TA], bf[2][TB];
    const int ngroups = (p.nchunks + 1 + NS - 1) / NS;
    for (int g = 0; g < ngroups; ++g) {
        const int c0 = g * NS;
#pragma unroll
        for (int u = 0; u < NS; ++u) {
            const int t = c0 + u;
            if (t > p.nchunks) break;                                      // uniform
            // my pieces of chunk t have landed: all but the (NS - 2) younger chunks' worth of my DMAs
            if (full) wait_vmcnt<(NS - 2) * PPW>(); else wait_vmcnt<(NS - 2) * (PPW > 1 ? PPW - 1 : 0)>();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");             // my fragment reads of chunk t-1 are done: its slot may be refilled
#ifdef ORE_TRACE
            const int dbg = q.k.dbg;
#else
            constexpr int dbg = 0;
#endif
            if (!(dbg & 8)) __builtin_amdgcn_s_barrier();                  // everybody's pieces of chunk t; everybody's reads of chunk t-1
            if (t < p.nchunks && !(dbg & 4)) {
                const float* st = lds + u * STAGE_F;
#pragma unroll
                for (int i = 0; i < TA; ++i) af[u & 1][i] = *reinterpret_cast<const f32x4*>(st + (wm * TA + i) * 256 + foff);
#pragma unroll
                for (int j = 0; j < TB; ++j) bf[u & 1][j] = *reinterpret_cast<const f32x4*>(st + (GA + wn * TB + j) * 256 + foff);
            }
            __builtin_amdgcn_sched_barrier(0);                             // the reads above are issued before the MFMAs below
            // The refill of the slot chunk t-1 was read from -- this wave's pieces of chunk t + NS - 1 -- goes out BETWEEN the MFMAs
            // of chunk t-1, one piece per segment: a DMA instruction holds the wave at issue while the texture addresser works off
            // the pieces queued in front of it (every wave of the CU queues its own right after the same barrier), and issued in
            // one go ahead of the MFMAs that wait left the matrix pipe idle for as long as the staging takes.
            constexpr int MF = 4 * TA * TB, SEG = (MF + PPW) / (PPW + 1);  // MFMAs per segment; piece s follows segment s
            if constexpr (BF) {
                // bf16-OPERAND mode (ore_conv_set_precision(ORE_CONV_BF16), BASELINE configs[4]'s training form): fp32 tensors in HBM and LDS, both
                // fragments rounded to bf16 (nearest even) as they leave LDS, ONE v_mfma_f32_16x16x16_bf16 per tile where the fp32 build
                // issues four 16x16x4 (the fragment layout -- four consecutive k per lane -- is the same), fp32 accumulation
                constexpr int MFB = TA * TB, SEGB = (MFB + PPW) / (PPW + 1);
                if (t > 0 && !(dbg & 1)) {
                    s16x4 ah[TA], bh[TB];
#pragma unroll
                    for (int i = 0; i < TA; ++i) ah[i] = to_bf16x4(af[(u & 1) ^ 1][i]);
#pragma unroll
                    for (int j = 0; j < TB; ++j) bh[j] = to_bf16x4(bf[(u & 1) ^ 1][j]);
#pragma unroll
                    for (int i = 0; i < TA; ++i)
#pragma unroll
                        for (int j = 0; j < TB; ++j) {
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(bh[j], ah[i], acc[i][j], 0, 0, 0);
                            const int idx = i * TB + j;
                            if (idx % SEGB == SEGB - 1 && idx / SEGB < PPW && !(dbg & 2)) {
                                __builtin_amdgcn_sched_barrier(0);
                                issue_piece(t + NS - 1, (u + NS - 1) % NS, idx / SEGB);
                                __builtin_amdgcn_sched_barrier(0);
                            }
                        }
#pragma unroll
                    for (int s2 = (MFB / SEGB < PPW ? MFB / SEGB : PPW); s2 < PPW; ++s2)
                        if (!(dbg & 2)) issue_piece(t + NS - 1, (u + NS - 1) % NS, s2);
                } else if (!(dbg & 2)) {
                    issue(t + NS - 1, (u + NS - 1) % NS);
                }
            } else
            if (t > 0 && !(dbg & 1)) {
#pragma unroll
                for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                    for (int i = 0; i < TA; ++i)
#pragma unroll
                        for (int j = 0; j < TB; ++j) {
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[(u & 1) ^ 1][j][tt], af[(u & 1) ^ 1][i][tt], acc[i][j], 0, 0, 0);   // D^T: lane = pixel
                            const int idx = (tt * TA + i) * TB + j;
                            if (idx % SEG == SEG - 1 && idx / SEG < PPW && !(dbg & 2)) {
                                __builtin_amdgcn_sched_barrier(0);
                                issue_piece(t + NS - 1, (u + NS - 1) % NS, idx / SEG);
                                __builtin_amdgcn_sched_barrier(0);
                            }
                        }
#pragma unroll
                for (int s2 = (MF / SEG < PPW ? MF / SEG : PPW); s2 < PPW; ++s2)       // pieces no segment end was left for
                    if (!(dbg & 2)) issue_piece(t + NS - 1, (u + NS - 1) % NS, s2);
            } else if (!(dbg & 2)) {
                issue(t + NS - 1, (u + NS - 1) % NS);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    wait_vmcnt<0>();                                   // the zero-fill tail DMAs
    __syncthreads();

    // ---- epilogue (ore_conv_epilogue.h): every wave finishes its own TA x TB tiles from registers
    const __amdgpu_buffer_rsrc_t rsc = make_rsrc(p.scale, p.scale ? p.sc_bytes : 0u), rsh = make_rsrc(p.shift, p.shift ? p.sc_bytes : 0u);
    const __amdgpu_buffer_rsrc_t rad = make_rsrc(p.add, p.add ? p.add_bytes : 0u);
    const bool vec_ok = CONV_OUT_VEC_OK(p, false);
    float* cs = lds;                                   // [WGM][GB][16] column sums of the waves' row bands
    const int kq = lane >> 4;
#pragma unroll
    for (int j = 0; j < TB; ++j) {
        const int en = n0 + (wn * TB + j) * 16 + kq * 4;
        f32x4 e_sc = {1.f, 1.f, 1.f, 1.f}, e_sh = {0.f, 0.f, 0.f, 0.f};
        const unsigned ev = en < p.Cout ? (unsigned)(en * 4) : kOOB;
        if (p.scale) e_sc = bload4(rsc, ev);
        if (p.shift) e_sh = bload4(rsh, ev);
        f32x4 csum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < TA; ++i) {
            const int m = m0 + (wm * TA + i) * 16 + (lane & 15);
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
#ifdef ORE_TRACE
            if (m < p.M && en < p.Cout && !(q.k.dbg & 16)) {
#else
            if (m < p.M && en < p.Cout) {
#endif
                v = acc[i][j] * e_sc + e_sh;
                if (p.add) v += bload4(rad, (unsigned)(addend_index(p, pixel_of_row(p, m, hw), en) * 4));
                CONV_RELU_ZERO4(v, en, p.relu_cout, p.Cout)
                float* o = p.out + (size_t)blockIdx.z * p.out_zstride + (size_t)m * p.out_ld + p.out_coff + en;
                CONV_STORE4_F32(o, v, vec_ok, en, p.Cout)
            }
            csum += v;
        }
        if (p.colsum) {                                // the 16 pixel lanes of a channel quad, then the waves' row bands in order
            CONV_COLSUM16(csum)
            if ((lane & 15) == 0) *reinterpret_cast<f32x4*>(cs + (wm * GB + wn * TB + j) * 16 + kq * 4) = csum;
        }
    }
    if (p.colsum) {
        __syncthreads();
        if (tid < GB * 16) {
            const int j2 = tid >> 4, ch = tid & 15;
            float sacc = cs[j2 * 16 + ch];
#pragma unroll
            for (int w2 = 1; w2 < WGM; ++w2) sacc += cs[(w2 * GB + j2) * 16 + ch];
            const int n = n0 + j2 * 16 + ch;
            if (n < p.Cout16) p.colsum[(size_t)bx * p.Cout16 + n] = sacc;
        }
    }
}

template <int GA, int GB, int WGM, int WGN, int NS, bool BF = false>
int gd_go(const GdP& q, bool k3, dim3 grid, hipStream_t st) {
    const dim3 block(64 * WGM * WGN);
    constexpr size_t lds = (size_t)NS * (GA + GB) * 256 * sizeof(float);
    static_assert(lds <= (BF ? 64 : 128) * 1024, "LDS ring (the bf16-operand builds keep the default LDS limit)");
    if constexpr (lds > 64 * 1024) {                   // the one-block-per-CU builds
        static bool attr[2] = {false, false};
        if (!attr[k3]) {
            const void* f = k3 ? (const void*)k_conv_gd<GA, GB, WGM, WGN, NS, 3> : (const void*)k_conv_gd<GA, GB, WGM, WGN, NS, 1>;
            ORE_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            attr[k3] = true;
        }
    }
    if (!k3) hipLaunchKernelGGL((k_conv_gd<GA, GB, WGM, WGN, NS, 1, BF>), grid, block, lds, st, q);
    else hipLaunchKernelGGL((k_conv_gd<GA, GB, WGM, WGN, NS, 3, BF>), grid, block, lds, st, q);
    return ore_launch_status(BF ? "k_conv_gd<bf16 operands>" : "k_conv_gd");
}

}  // namespace

namespace oreconv {

// k_conv_gd: the plan's tile and build over p's rows (several levels of a 1x1 layer: one flat GEMM)
int launch_gd(const ConvP& p, const ConvPlan& pl, hipStream_t st) {
    GdP q;
    Lvl L;
    fill_desc_args(q.k, p, pl, L);
    q.k.zc_stride = 0; q.k.out_zstride = 0;
#ifdef ORE_TRACE
    q.k.dbg = g_knobs.gd_dbg;
#endif
    build_chunk_table(q.tab, kTab, p, L, kFmt);
    const bool k3 = p.kh == 3;
    const dim3 grid(pl.gx, pl.gy, 1);
#define GD_GO(bm_, bn_, wgm_, wgn_, ns_, bf_)                                                                             \
    if (pl.bm == bm_ && pl.bn == bn_ && pl.build[0] == wgm_ && pl.build[1] == wgn_ && pl.build[2] == ns_ && pl.build[3] == bf_) \
        return gd_go<bm_ / 16, bn_ / 16, wgm_, wgn_, ns_, bf_>(q, k3, grid, st);
    ORE_GD_BUILDS(GD_GO)
#undef GD_GO
    return ORE_EINVAL;
}

// The second-stage GEMM (d2z:modeling/roi_heads/box_head.py FastRCNNConvFCHead.fc1 with the DSA mix pre-composed into it: M <= 512
// ROIs, K = 8192, 128 outputs) as a K split over blocks: tiles of 80 x 64 outputs, S slices of K -> ceil(M / 80) * (Cout16 / 64) * S
// blocks (4 * 2 * 32 = 256 at 320 ROIs), slice z writes its raw partial sums to parts + z * M * Cout16.  Whoever consumes them adds
// the slices in z order, then bias and ReLU (k_roi_predict_mb) -- a fixed order, so the result is reproducible.  With K this long and
// M x N this small a block that walks all of K stages 1 MB through one CU (k_conv_kw / k_conv_kd on 160 blocks: 19 us, 46 MB of L2
// fills); here a block stages 144 KB.
int conv_gd_splitk(const float* in, int in_ld, const float* w, int M, int K, int Cout16, float* parts, int S, hipStream_t st) {
    ORE_CHECK_ARG(in && w && parts && M >= 1 && M < (1 << 20) && K % 16 == 0 && Cout16 % 64 == 0 && in_ld % 16 == 0 && in_ld >= K && S >= 1 &&
                      (K / 16) % S == 0, "conv_gd_splitk: bad shape M %d K %d Cout16 %d S %d", M, K, Cout16, S);
    ORE_CHECK_ARG((long long)M * in_ld * 4 < (long long)kOOB - (1 << 24) && (long long)Cout16 * K * 4 < (long long)kOOB, "conv_gd_splitk: operand beyond a buffer descriptor");
    // the GEMM as a 1x1 layer over one "image" of M pixels in a row, no epilogue operands; each slice sees its own K / S chunks
    ConvP p{};
    p.in = in; p.in_ld = in_ld; p.B = 1; p.Cin = K; p.nlev = 1; p.lv[0] = Lvl{0, 0, 1, M, 1, M};
    p.w = w; p.Cout = Cout16; p.Cout16 = Cout16; p.kh = 1; p.kw = 1; p.stride = 1; p.M = M; p.K = K;
    p.out = parts; p.out_ld = Cout16; p.nchunks = K / 16 / S;
    ConvPlan pl{};
    pl.gx = ceil_div(M, 80); pl.gy = Cout16 / 64;
    GdP q;
    Lvl L;
    fill_desc_args(q.k, p, pl, L);
    q.k.zc_stride = p.nchunks; q.k.out_zstride = M * Cout16;
#ifdef ORE_TRACE
    q.k.dbg = 0;
#endif
    build_chunk_table(q.tab, kTab, p, L, kFmt);
    return gd_go<5, 4, 1, 4, 4>(q, false, dim3(pl.gx, pl.gy, S), st);
}

}  // namespace oreconv
