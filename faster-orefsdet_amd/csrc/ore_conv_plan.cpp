// The conv planner: which kernel, build, split-K and grid every ore_conv2d_fwd / ore_conv2d_levels_fwd call runs on.  Host code only;
// the launchers (ore_conv*.hip) execute its plans and never decline one.  The tuning aids of ore_conv_set_plan_override live here too.
#include "ore_common.h"
#include "ore_conv_internal.h"

namespace oreconv {

ConvKnobs g_knobs;

namespace {

const ConvKnobs& K = g_knobs;

ConvPlan make_plan(int launcher, int bm, int bn, int b0, int b1, int b2, int b3, int gx, int gy, int xmap = 0, int splitk = 1, int sps = 0) {
    ConvPlan pl{};
    pl.launcher = launcher; pl.error = ORE_OK;
    pl.bm = bm; pl.bn = bn;
    pl.build[0] = b0; pl.build[1] = b1; pl.build[2] = b2; pl.build[3] = b3;
    pl.splitk = splitk; pl.steps_per_split = sps; pl.xmap = xmap;
    pl.gx = gx; pl.gy = gy;
    return pl;
}

ConvPlan none() { return ConvPlan{}; }                     // this kernel does not take the call: the next one is asked

ConvPlan fail(int code) {                                  // no kernel takes the call (ore_set_error has said why)
    ConvPlan pl{};
    pl.error = code;
    return pl;
}

// block -> tile mapping (tile_of_block): fabric bytes if every XCD reads what its tiles need once
int choose_xmap(const ConvP& p, int gx, int gy) {
    if (K.xmap_force >= 0) return K.xmap_force;
    const int blocks = gx * gy;
    if (blocks < 16) return 0;
    const double A = (double)p.M * p.Cin, Wb = (double)p.Cout16 * p.K;
    const int per_xcd = ceil_div(blocks, 8);
    const double cost_m = A + 8.0 * Wb;                                        // an XCD = a range of rows x all output channels
    const int spanned = per_xcd >= gx ? ceil_div(per_xcd, gx) + 1 : 2;         // N tiles an XCD's run touches in N-major order
    const double cost_n = (double)(gy < 8 ? gy : 8) * A + 8.0 * Wb * (spanned < gy ? spanned : gy) / gy;
    if (cost_n < cost_m) return 2;
    return (gx & 7) == 0 ? 0 : 1;                                              // plain mapping already keeps an M tile on one XCD
}

// tiles of TH output rows x 16 output columns over every level and image (the 3x3 tile kernels)
int patch_tiles(const ConvP& c, int TH) {
    int tiles = 0;
    for (int l = 0; l < c.nlev; ++l) tiles += c.B * ceil_div(c.lv[l].Wo, 16) * ceil_div(c.lv[l].Ho, TH);
    return tiles;
}

// ---- k_conv3x3_ws, bf16 STORAGE: 3x3 stride-1 layers with 64 / 128 input channels on the weight-stationary kernel (weights in
// registers for the whole launch, only the halo patch is staged).  c holds the input side in 4-byte units (fill_common).
ConvPlan plan_ws_sb(const ConvP& c) {
    if (!K.ws_sb_mode || !(c.sb & 1) || !(c.sb & 2)) return none();
    if (c.kh != 3 || c.kw != 3 || c.stride != 1 || c.pad != 1 || c.in_mul || c.add || c.colsum) return none();
    if ((c.Cin != 32 && c.Cin != 64) || c.Cout != c.Cout16 || c.Cout % 64 != 0) return none();
    if (c.Cin == 64 && K.ws_sb_mode == 3) return none();                       // (A/B aid: 128-channel layers back on k_conv_kw)
    if (c.out_ld % 4 != 0 || c.out_coff % 4 != 0 || ((uintptr_t)c.out & 7) != 0) return none();
    if (c.M < 6000 && !c.w_lstride) return none();
    // 64 channels: 4 waves x 16 output channels, 72 VGPRs of weights, two blocks per CU.  128 channels: 8 waves, the wave pairs (w, w+4)
    // split the input channels (72 VGPRs each; the upper half's accumulators meet the lower half's in LDS), one block per CU.
    const int TH = 4, tiles = patch_tiles(c, TH);
    int xmap = tiles >= 16 ? 1 : 0;
    const int gy = c.Cout16 / 64;
    int gx = (c.Cin == 32 ? 512 : 256) / gy;                // resident blocks
    gx &= ~7;
    if (gx > tiles) gx = tiles;
    if (c.w_lstride) { gx = tiles; xmap = 0; }             // per-level weights: one tile per block, in tile order
    return c.Cin == 32 ? make_plan(ORE_LAUNCH_WS_SB, TH, 64, TH, 32, 1, 1, gx, gy, xmap) : make_plan(ORE_LAUNCH_WS_SB, TH, 64, TH, 64, 2, 1, gx, gy, xmap);
}

// 3x3 STRIDE-2 layers with 64 input channels and a multiple of 64 output channels (stem_3), bf16 storage: weight-stationary too
// (18.8 -> 16.0 us).  The fp32 build of the same kernel was measured and dropped: 144 VGPRs of weights + an 11-vector register-staged
// 5 x 33 patch spill, and the stride-2 fragment reads are 2-way bank conflicted: 71.9 us against 50.2 on k_conv_igemm.
ConvPlan plan_ws_s2(const ConvP& c) {
    if (!(c.sb & 1) || !K.ws_s2_mode || c.kh != 3 || c.kw != 3 || c.stride != 2 || c.pad != 1 || c.in_mul || c.add || c.colsum || c.nlev != 1) return none();
    if (c.Cin != 32 || !(c.sb & 2)) return none();
    if (c.Cout != c.Cout16 || c.Cout % 64 != 0 || c.M < 6000) return none();
    if (c.out_ld % 4 != 0 || c.out_coff % 4 != 0 || ((uintptr_t)c.out & 7) != 0) return none();
    const int TH = 2, tiles = patch_tiles(c, TH);
    const int gy = c.Cout16 / 64;
    int gx = 512 / gy;
    gx &= ~7;
    if (gx > tiles) gx = tiles;
    return make_plan(ORE_LAUNCH_WS_SB, TH, 64, TH, 32, 1, 2, gx, gy, tiles >= 16 ? 1 : 0);
}

// ---- the fp32-storage 3x3 tile kernels: k_conv3x3_patch<4 | 8>, k_conv3x3_patch_db, k_conv3x3_ws<2, 64 | 128>
ConvPlan plan_patch(const ConvP& c) {
    if (c.kh != 3 || c.kw != 3 || c.stride != 1 || c.pad != 1 || c.Cout16 % 64 != 0 || c.in_mul || c.add || c.colsum) return none();
    if (c.out_ld % 4 != 0 || c.out_coff % 4 != 0 || ((uintptr_t)c.out & 15) != 0) return none();      // the epilogue stores 16 bytes per lane
    const int mode = K.patch_mode;
    if (mode == 0) return none();
    if (c.bf16 && mode > 0 && mode != 4 && mode != 102) return none();   // bf16 builds: patch<4> and ws<2,64,1> only
    int TH = mode > 0 ? mode : 4;
    bool db = TH == 16;
    if (db) TH = 8;
    bool ws = TH == 102;                                     // TH = 4 needs > 256 VGPRs (spills): only the 2-row tile is built
    if (ws) { TH = 2; if (c.Cin != 64 && (c.Cin != 128 || c.bf16)) return none(); }
    if (mode < 0 && c.M < 6000) return none();               // plan: only the large-M layers (profiles/r01_conv_tune.txt); TH=4 wins or ties
    // plan: the weight-stationary kernel wins once a resident block walks >= 4 tiles (stem_2: 3200 tiles, 71 vs 82 us); below that its
    // 36-fragment weight prologue is not amortised (stage-2 64->64 layers: 800 tiles, 29 vs 26 us)
    const long long ws_tiles = (long long)c.B * ceil_div(c.lv[0].H, 2) * ceil_div(c.lv[0].W, 16);
    if (mode < 0 && c.Cin == 64 && c.nlev == 1 && ws_tiles >= 2048) { ws = true; TH = 2; }
    // Cin = 128 (8 waves, K split in wave pairs, fp32 build only): alone on the GPU it wins from ~1600 tiles (8 x 80x80: 140 vs 154 us,
    // 8 x 160x160: 263 vs 315 us; one 160x160 image, 800 tiles: 47 vs 45 us -- tools/ws128_exp.py), but its one 512-thread,
    // 256-VGPR block per CU leaves no room for another stream's kernel: with several passes in flight the folded-serving rate DROPS
    // 2 %.  Used for training-sized launches only.
    if (mode < 0 && c.Cin == 128 && c.nlev == 1 && !c.bf16 && ws_tiles >= 8192) { ws = true; TH = 2; }
    // plan: one image of stage 2 (64 output channels, 160 x 160): the double-buffered 8-wave patch kernel beats the 4-wave one by 7-8 %
    // (64 -> 64: 27.9 -> 25.9 us, 128 -> 64: 47.0 -> 43.3 us; tools/ws_s2_exp.py); at 128 output channels / 80 x 80 it loses (42 vs 26 us)
    if (mode < 0 && !ws && !c.bf16 && c.nlev == 1 && c.Cout16 == 64 && c.M >= 16384 && c.M <= 65536) { db = true; TH = 8; }
    const int tiles = patch_tiles(c, TH), gy = c.Cout16 / 64;
    const int xmap = K.xmap_force >= 0 ? (K.xmap_force ? 1 : 0) : (tiles >= 16 ? 1 : 0);   // M-major bands of tiles per XCD
    if (ws) {
        // 64-channel layers: 4 waves, 2 blocks per CU; 128-channel layers: 8 waves (K split in wave pairs), 1 block per CU
        const bool wide = c.Cin == 128;
        const int resident = wide ? 256 : 512;               // (a grid of tiles/rounds blocks measured 7 % slower on stem_2)
        return make_plan(wide ? ORE_LAUNCH_WS128 : ORE_LAUNCH_WS64, TH, 64, TH, c.Cin, wide ? 2 : 1, wide ? 0 : c.bf16,
                         tiles < resident ? tiles : resident, gy, xmap);
    }
    // (a forced tile height other than 4 / 8 runs k_conv3x3_patch<4> over tiles of that height)
    return make_plan(db ? ORE_LAUNCH_PATCH_DB : TH == 8 ? ORE_LAUNCH_PATCH8 : ORE_LAUNCH_PATCH4, TH, 64, TH, db ? 1 : 0, (!db && TH != 8) ? c.bf16 : 0, 0,
                     tiles, gy, xmap);
}

// ---- Winograd F(2x2,3x3): large-M 3x3 layers that were handed transformed weights
ConvPlan plan_wino(const ConvP& c) {
    if ((!K.wino_mode && !c.wino_lstride) || !c.wino || c.bf16) return none();   // (per-level launches have no direct twin: mode 0 does not apply)
    if (c.kh != 3 || c.kw != 3 || c.stride != 1 || c.pad != 1 || c.in_mul || c.add || c.colsum) return none();
    if (c.Cout != c.Cout16 || !conv_wino_covers(c.Cout, c.Cin)) return none();
    if (c.out_ld % 4 != 0 || c.out_coff % 4 != 0 || ((uintptr_t)c.out & 15) != 0 || c.in_ld % 4 != 0 || c.in_coff % 4 != 0) return none();
    if (c.ep_stride % 4 != 0 || ((uintptr_t)c.scale & 15) != 0 || ((uintptr_t)c.shift & 15) != 0) return none();
    // below these row counts a launch is latency-bound, not multiply-bound (tools/wino_time.py: 128 -> 128 at 1600 rows 13.4 -> 10.3 us,
    // 96 -> 96 at 1600-1900 rows and everything at 400 rows a tie)
    if (K.wino_mode != 2 && !c.wino_lstride && c.M < ((c.Cin == 64 || c.Cin == 128) ? 1500 : 3000)) return none();
    // the kernels read each image through a buffer descriptor of its own: its bytes are the descriptor's num_records and must stay
    // below kOOB, the offset that marks a column outside the image
    for (int l = 0; l < c.nlev; ++l)
        if ((long long)c.lv[l].H * c.lv[l].W * c.in_ld * 4 >= (long long)kOOB) return none();
    const int nb = patch_tiles(c, 4);                       // batches of 4 x 16 outputs
    if (nb >= (1 << 22)) return none();                     // k_conv3x3_wino_nu decodes a batch number by fdiv
    if (c.Cin == 80 || c.Cin == 96 || c.Cin == 112) {       // k_conv3x3_wino_nu: NCGB groups of 16 output channels per block
        const int ncgb = c.Cin == 80 ? 3 : 2;
        const int gy = ceil_div(c.Cout16 / 16, ncgb);
        int gx = 256 / gy;                                  // one resident block per CU
        if (gx > nb) gx = nb;
        if (gx < 1) gx = 1;
        return make_plan(ORE_LAUNCH_WINO_NU, 4, ncgb * 16, c.Cin, ncgb, 0, 0, gx, gy);
    }
    const int coutb = c.Cin == 64 ? 64 : 32;
    const int gy = c.Cout / coutb;
    int gx = 256 / gy;                                      // one resident block per CU
    if (gx > nb) gx = nb;
    if (gx < 1) gx = 1;
    if (c.wino_lstride) gx = wino_level_blocks(c, gy, nullptr);
    return make_plan(ORE_LAUNCH_WINO, 4, coutb, c.Cin, 0, 0, 0, gx, gy);
}

// ---- k_conv_gd: shared-stage LDS-DMA kernel with descriptor addressing for the large-M layers (stem_3, the big concats)
// several pyramid levels in one launch: a 1x1 stride-1 layer over the level-major row matrix is one flat GEMM (as in k_conv_kd)
bool gd_flat(const ConvP& p) { return p.nlev > 1 && p.kh == 1 && p.kw == 1 && p.stride == 1 && p.pad == 0; }

bool gd_applies(const ConvP& p) {
    if (p.sb || p.in_mul || p.in_add || p.in_relu || (p.nlev != 1 && !gd_flat(p)) || p.ep_stride || (p.add && p.nlev != 1)) return false;
    if (p.Cin % 16 != 0 || p.in_ld % 16 != 0 || p.kh != p.kw || (p.kh != 1 && p.kh != 3)) return false;
    if (p.M >= (1 << 22) || p.nchunks > kGdTab) return false;
    const long long in_rows = gd_flat(p) ? (long long)p.lv[0].irow0 + p.M : (long long)p.lv[0].irow0 + (long long)p.B * p.lv[0].H * p.lv[0].W;
    if (in_rows * p.in_ld * 4 >= (long long)kOOB - (1 << 24) || (long long)p.Cout16 * p.K * 4 >= (long long)kOOB) return false;
    if (p.add && (long long)p.B * p.add_H * p.add_W * p.add_ld * 4 >= (long long)kOOB) return false;
    return true;
}

struct GdPlan { int bm, bn, ns; };   // ns: the ring depth, or 10 + it for the eight-wave build of the tile
GdPlan gd_tile(const ConvP& p) {
    if (K.gd_force[0] > 0) return {K.gd_force[0], K.gd_force[1], K.gd_force[2]};
    // from tools/kw_phase_trace.py gd (profiles/r04_gd_times.txt; eager launches back to back, one MI355X, bs = 1 shapes; ns >= 10: eight waves):
    //   stage-3 concat 352 -> 256 at M = 6400: 17.9 us (k_conv_gs 21.2); stage-2 concat 320 -> 112 at M = 25600: 27.7 (31.1);
    //   stem_3 3x3 / 2 64 -> 128 at M = 25600: 44.0 (k_conv_igemm 62.7).
    // Every tiling of a layer lands within ~10 % of the others (r04_gd_ablation.txt: the MFMA phase alone runs at ~75 % of the peak,
    // staging adds to it instead of hiding behind it); the choices below are the fastest measured, not a structural preference.
    // (training batch sizes -- the frozen stem_3 / concats over 16 queries + 384 support crops, M up to 1.6 M rows -- run on the same
    // tiles since round 5: bs-16 step 46.7 -> 43.8 ms, tools/bench_train.py; mode 3 = the round-4 limit M <= 32768 for A/B)
    if (p.M < 4096 || (p.M > 32768 && K.gd_mode == 3)) return {0, 0, 0};
    if (p.kh == 1 && p.Cout16 == 256 && p.nchunks >= 16) return {64, 64, 4};
    if (p.kh == 1 && p.Cout16 == 112 && p.nchunks >= 16) return {128, 64, 14};
    if (p.kh == 3 && p.stride == 2 && p.Cout16 == 128 && p.Cin == 64) return {112, 128, 14};
    // the FPN lateral of stage 3 (M = 6400) and conv3 over the three levels (M = 8400), 256 -> 128 (profiles/r04_gd_mid.txt):
    // 9.4 us against k_conv_kd's 11.7 when 64 x 64 tiles fill the CUs once, 12.6 against 20.1 when they would spill into a second round
    if (p.kh == 1 && p.Cout16 == 128 && p.nchunks == 16 && !p.colsum)
        return ceil_div(p.M, 64) * 2 <= 256 ? GdPlan{64, 64, 14} : GdPlan{32, 64, 4};
    // every other 1x1 layer at training batch sizes (the trainable concats, laterals, conv3 and their data gradients over 16 queries /
    // 384 support crops: M >= 16384 rows): 64 x 128 tiles, or 64 x 64 for narrow outputs (round 5; they ran on k_conv_gs / k_conv_igemm)
    if (K.gd_mode == 2 && p.kh == 1 && p.M >= 16384 && p.nchunks >= 4 && !p.colsum) return p.Cout16 > 64 ? GdPlan{64, 128, 4} : GdPlan{64, 64, 4};
    return {0, 0, 0};
}

ConvPlan plan_gd(const ConvP& p) {
    if (K.gd_mode == 0 || !gd_applies(p)) return none();
    const GdPlan t = gd_tile(p);
    if (t.bm == 0) return none();
    const int gx = ceil_div(p.M, t.bm), gy = ceil_div(p.Cout16, t.bn);
    const int bf = p.bf16 ? 1 : 0;
#define GD_BUILT(bm_, bn_, wgm_, wgn_, ns_, bf_)                                                                            \
    if (bf == bf_ && t.bm == bm_ && t.bn == bn_ && t.ns == ((wgm_) * (wgn_) == 8 ? 10 + ns_ : ns_))                         \
        return make_plan(ORE_LAUNCH_GD, bm_, bn_, wgm_, wgn_, ns_, bf_, gx, gy, choose_xmap(p, gx, gy));
    ORE_GD_BUILDS(GD_BUILT)
#undef GD_BUILT
    // a tile with no bf16-operand build is not this kernel's in that mode: the other kernels take the layer
    if (K.gd_force[0] > 0 && !bf) { ore_set_error("k_conv_gd: no build for tile %dx%d, ring %d", t.bm, t.bn, t.ns); return fail(ORE_EINVAL); }
    return none();
}

// ---- k_conv_kd: lean LDS-DMA kernel (buffer descriptors, chunk table in the kernel arguments, double-buffered batches)
// several pyramid levels in one launch: a 1x1 stride-1 layer over the level-major row matrix is one flat GEMM (row m reads row m)
bool kd_flat(const ConvP& p) { return p.nlev > 1 && p.kh == 1 && p.kw == 1 && p.stride == 1 && p.pad == 0 && !p.add; }

bool kd_applies(const ConvP& p) {
    // (bf16 STORAGE, p.sb & 1, is served: its sizes arrive in 4-byte units, so the staging is byte for byte the fp32 one)
    if (p.bf16 || p.in_mul || p.in_add || p.in_relu || (p.nlev != 1 && !kd_flat(p)) || p.ep_stride) return false;
    // a pixel's channel vector starts on a 16-byte boundary (the DMA piece of a lane); fp32 layers of this model all have 64-byte rows
    if (p.Cin % 16 != 0 || p.in_ld % ((p.sb & 1) ? 4 : 16) != 0 || p.in_coff % 4 != 0 || p.kh != p.kw || (p.kh != 1 && p.kh != 3)) return false;
    if ((long long)p.M * p.Cout16 >= (1ll << 31) || p.M >= (1 << 22) || p.nchunks > kKdTab) return false;
    const long long in_rows = kd_flat(p) ? (long long)p.lv[0].irow0 + p.M : (long long)p.lv[0].irow0 + (long long)p.B * p.lv[0].H * p.lv[0].W;
    if (in_rows * p.in_ld * 4 >= (long long)kOOB - (1 << 24) || (long long)p.Cout16 * p.K * 4 >= (long long)kOOB) return false;
    if (p.add && (long long)p.B * p.add_H * p.add_W * p.add_ld * 4 >= (long long)kOOB) return false;
    if ((p.sb & 1) && p.colsum && !(p.sb & 2)) return false;   // (fp32 output of a bf16 layer with column sums: no caller, not built)
    if (p.kh == 3 && (2ll * p.lv[0].W + 2) * p.in_ld * 4 + (long long)p.Cin * 4 >= (1ll << 28)) return false;   // the chunk table keeps 28 bits of offset
    return true;
}

struct KdPlan { int bm, bn, nw, sb; };

// tile / waves / batch of the automatic plan; bm == 0: the layer stays on k_conv_kw.  From tools/kw_phase_trace.py kd
// (profiles/r04_kd_phase_trace.txt): first-block-start -> last-block-end of the launch against k_conv_kw's, one MI355X, bs = 1 shapes:
//   M = 400   3x3 112->112 5.6 vs 10.8 us, 384->112 10.1 vs 22.4, 1x1 512->128 4.3 vs 6.8, 720->512 8.7 vs 12.6
//   M = 1600  3x3 96->96 8.9 vs 12.7, 256->96 14.8 vs 24.4, 1x1 384->128 6.3 vs 9.5, 544->384 15.0 vs 15.9
//   M = 6400  1x1 256->128 11.1 vs 15.1;  the second-stage GEMM (K = 8192) ties and stays where it is
KdPlan kd_tile(const ConvP& p) {
    if (K.kd_force[0] > 0) return {K.kd_force[0], K.kd_force[1], K.kd_force[2], K.kd_force[3]};
    if (K.kd_mode == 2) return {16, p.Cout16 >= 32 ? 32 : 16, 4, 4};
    if (p.nchunks > 256) return {0, 0, 0, 0};
    if (p.M <= 512) {
        if (p.Cout16 <= 128) return p.nchunks <= 64 ? KdPlan{16, 16, 4, 8} : KdPlan{16, 16, 8, 4};
        return {32, 32, 4, 4};
    }
    if (p.M <= 2048) {
        if (p.Cout16 == 96) return p.nchunks <= 64 ? KdPlan{16, 48, 4, 4} : KdPlan{16, 48, 8, 2};
        if (p.Cout16 == 128) return {16, 64, 4, 2};
        if (p.Cout16 >= 320 && p.Cout16 % 80 == 64) return {32, 80, 4, 2};       // 384 = 4 x 80 + 64: five column tiles
        return {0, 0, 0, 0};
    }
    if (p.M <= 9216 && p.Cout16 == 128 && p.kh == 1) {                            // FPN lateral 3, conv3 over the three levels
        // (fp32: k_conv_gd takes both first.)  bf16 storage: 64 x 64 tiles of conv3's 8400 rows are 264 blocks -- a second round on 256
        // CUs: 10.0 us against 8.5 on k_conv_kw's 32 x 64 tiles (tools/bf16s_sweep.py) -- so only what fits one round comes here
        if ((p.sb & 1) && ceil_div(p.M, 64) * 2 > 256) return {0, 0, 0, 0};
        return {64, 64, 4, 2};
    }
    // bf16 storage, stage 3's 3x3 layers (M = 6400, 80 output channels; fp32 runs them on the Winograd kernel): 7.0-7.6 us against
    // k_conv_kw's 9.7-10.9 (tools/bf16s_sweep.py)
    if ((p.sb & 1) && p.kh == 3 && p.Cout16 == 80) return {32, 80, 4, 2};   // (any M: the frozen stage 3 of a bf16 training step runs 16 queries and 384 support crops through it)
    return {0, 0, 0, 0};
}

ConvPlan plan_kd(const ConvP& p) {
    if (K.kd_mode == 0 || !kd_applies(p)) return none();
    const KdPlan t = kd_tile(p);
    if (t.bm == 0) return none();
    const int bn = t.bn < p.Cout16 ? t.bn : p.Cout16;
    const int steps = ceil_div(p.nchunks, t.nw), nb = ceil_div(steps, t.sb);
    if (t.nw * nb * t.sb > kKdTab) return none();
    const int gx = ceil_div(p.M, t.bm), gy = ceil_div(p.Cout16, bn);
#define KD_BUILT(bm_, bn_, nw_, sb_) \
    if (t.bm == bm_ && bn == bn_ && t.nw == nw_ && t.sb == sb_) return make_plan(ORE_LAUNCH_KD, bm_, bn_, nw_, sb_, p.sb & 1, 0, gx, gy, choose_xmap(p, gx, gy));
    ORE_KD_BUILDS(KD_BUILT)
#undef KD_BUILT
    if (K.kd_force[0] > 0) { ore_set_error("k_conv_kd: no build for tile %dx%d, %d waves, %d steps per batch", t.bm, bn, t.nw, t.sb); return fail(ORE_EINVAL); }
    return none();
}

// ---- k_conv_rf: register-fed kernel for the smallest-M layers (stages 4-5, laterals 4-5)
bool rf_covers(const ConvP& p) {
    if (K.rf_mode == 0) return false;
    if (p.sb || p.bf16 || p.in_mul || p.in_add || p.in_relu || p.nlev != 1 || p.ep_stride) return false;
    if (p.colsum && K.rf_force[0] == 0) return false;      // (the automatic plan leaves the eSE pool's layers to k_conv_kw's tiles)
    if (p.Cin % 16 != 0 || p.in_ld % 16 != 0 || p.kh != p.kw || (p.kh != 1 && p.kh != 3)) return false;
    if ((long long)p.M * p.Cout16 * p.K >= (1ll << 31) || p.M >= (1 << 22)) return false;
    if (p.add && (long long)p.B * p.add_H * p.add_W * p.add_ld * 4 >= (long long)kOOB) return false;
    const long long in_rows = (long long)p.lv[0].irow0 + (long long)p.B * p.lv[0].H * p.lv[0].W;
    if (in_rows * p.in_ld * 4 >= (long long)kOOB || (long long)p.Cout16 * p.K * 4 >= (long long)kOOB) return false;
    if (K.rf_mode == 2 || K.rf_force[0] > 0) return true;
    // automatic: the latency-bound launches -- few rows, not so many output channels that 16-row tiles re-read the pixels too often,
    // not so deep a K that a wave needs more than two batches (the second-stage GEMM stays on k_conv_kw: measured)
    // (round 4: k_conv_kd, which moves the same bytes in coalesced 64-byte segments through LDS-DMA, is ahead of this kernel on every
    // shape measured -- 5.6 vs 6.3 us on stage 5's 112->112 layers, 10.1 vs 17.2 on 384->112 -- and is asked first; what k_conv_kd
    // declines and fits here still comes here)
    return p.M <= 512 && p.Cout16 <= 128 && p.nchunks <= 256;
}

ConvPlan plan_rf(const ConvP& p) {
    if (!rf_covers(p)) return none();
    int gb = 1, nw = 4, maxs = 16;
    if (K.rf_force[0] > 0) { gb = K.rf_force[0]; nw = K.rf_force[1]; maxs = K.rf_force[2]; }
    else {
        // waves per block so that a wave's K slice fits ONE batch of registers where it can (two for the deepest layer)
        if (p.nchunks <= 64) { nw = 4; maxs = p.nchunks <= 32 ? 8 : (p.nchunks <= 48 ? 12 : 16); }
        else { nw = 8; maxs = p.nchunks <= 96 ? 12 : 16; }
    }
    const int steps = ceil_div(p.nchunks, nw), nb = ceil_div(steps, maxs);
    if (p.kh == 3 && nw * nb * maxs > kRfTab) return none();  // the chunk table of a 3x3 layer
    const int gx = ceil_div(p.M, 16), gy = ceil_div(p.Cout16, 16 * gb);
#define RF_BUILT(g, w, s) if (gb == g && nw == w && maxs == s) return make_plan(ORE_LAUNCH_RF, 16, 16 * g, g, w, s, 0, gx, gy, choose_xmap(p, gx, gy));
    ORE_RF_BUILDS(RF_BUILT)
#undef RF_BUILT
    return none();
}

// ---- k_conv_gs: shared-stage kernel for the large-M layers
ConvPlan plan_gs(const ConvP& p) {
    int bm = K.gs_force[0], bn = K.gs_force[1];
    if (bm == 0 && (p.sb & 1)) {                              // bf16 storage (plan_dma decided that this layer comes here)
        if (p.Cout16 == 112) { bm = 64; bn = 80; }
        else if (p.Cout16 % 128 == 0 && p.kh == 3) { bm = 64; bn = 128; }
        else if (p.Cout16 >= 256) { bm = 64; bn = 80; }
        else { bm = 64; bn = 64; }
    }
    if (bm == 0) {
        // measured (profiles/r02_kw_ab.txt): 2-5 % ahead of k_conv_igemm on the 1x1 concats, 3 % behind on stem_3 (3x3 stride 2) --
        // the staging mechanism is not what bounds these layers -- so only the 1x1 layers come here automatically
        if (p.M < 6400 || (p.kh != 1 && !(p.sb & 1))) return none();
        if (p.Cout16 == 112) { bm = 64; bn = 112; }
        else if (p.Cout16 % 128 == 0) { bm = 64; bn = p.M < 16384 ? 64 : 128; }      // s3cat: 64x64 21.8 us, 64x128 24.0 (400 vs 200 blocks)
        else if (p.Cout16 == 64) { bm = 64; bn = 64; }
        else return none();
    }
    const int ns = K.gs_ns == 4 || K.gs_ns == 6 ? K.gs_ns : 3;
    const int gx = ceil_div(p.M, bm), gy = ceil_div(p.Cout16, bn);
#define GS_BUILT(a, b, wgm, wgn) \
    if (bm == a && bn == b && gs_fits(a, b, ns)) return make_plan(ORE_LAUNCH_GS, a, b, wgm, wgn, ns, p.sb & 1, gx, gy, 0, 1, p.nchunks);
    ORE_GS_BUILDS(GS_BUILT)
#undef GS_BUILT
    return none();
}

// ---- k_conv_kw: wave-private K-split kernel fed by LDS-DMA
struct KwTile { int BM, BN, S; int NW = 4; };      // S = cross-block split-K (0: decide from the block count), BM = 0: layer left to k_conv_igemm / patch

// Tile plan, from tools/conv_kw_sweep.py on MI355X (profiles/r02_kw_sweep.txt).  What the sweep says: the minimal ring (NS = 2) wins
// almost everywhere -- more resident blocks per CU hide the DMA latency better than a deeper ring --, cross-block split-K pays only
// for K >= 2048 with < 128 tiles, and the 256-channel 1x1 concat at M = 6400 and the 128 -> 128 3x3 at M = 6400 stay on their round-1
// kernels.  Shapes outside the table get the tile with the most FLOP per staged byte among those that give >= 384 blocks.
KwTile kw_tile(int M, int C16, int nchunks) {
    const int steps = ceil_div(nchunks, 4);
    if (M >= 4096) {
        if (C16 >= 256) return {0, 0, 0};
        if (C16 <= 80) return {32, 16, 1};
        if (C16 == 128) return {16, 32, 1};
    } else if (M >= 1024) {
        if (C16 == 96) return {16, 48, 1};
        if (C16 == 128) return {16, 32, 1};
        if (C16 >= 256) return {32, 80, 1};
    } else {
        // the second-stage GEMM, 320 x 8192 -> 128: 8 waves split K inside the block (64 steps per wave) and NO cross-block split --
        // the release fence of a split-K block costs more than the longer chain (19.6 vs 24 us with {16, 48} x S 4)
        if (C16 <= 128 && steps >= 96) return {16, 16, 1, 8};
        if (C16 <= 128 && steps >= 32) return {16, 16, 1};           // stage-5 layer 0 (15.7 vs 17.4+ us with any cross-block split)
        if (C16 <= 128) return {16, 16, 1};
        return {16, 32, 1};
    }
    static const int bns[5] = {80, 64, 48, 32, 16};
    KwTile best = {16, 16, 0};
    float bs = -1.0f;
    int most = 0;
    for (int bm = 32; bm >= 16; bm -= 16)
        for (int b = 0; b < 5; ++b) {
            const int bn = bns[b];
            if (bn > C16) continue;
            const int nt = ceil_div(C16, bn), blocks = ceil_div(M, bm) * nt;
            const float ai = (float)(bm * bn) / (float)(bm + bn) * (float)C16 / (float)(nt * bn);
            if (blocks >= 384) { if (ai > bs) { bs = ai; best = {bm, bn, 0}; } }
            else if (bs < 0.0f && blocks > most) { most = blocks; best = {bm, bn, 0}; }
        }
    return best;
}

ConvPlan plan_kw(const ConvP& p, size_t workspace_floats) {
    KwTile t = kw_tile(p.M, p.Cout16, p.nchunks);
    if (p.sb & 1) {
        if (t.BM == 0) t = {32, 64, 1};
        if (p.M >= 4096 && (p.Cout16 == 128 || p.Cout16 == 64)) t = {32, 64, 1};
        if (p.M >= 4096 && p.Cout16 == 80) t = {16, 80, 1};
    }
    if (K.kw_force[0] > 0) t = {K.kw_force[0], K.kw_force[1] < p.Cout16 ? K.kw_force[1] : p.Cout16, K.kw_force[3]};
    if (t.BM == 0) return none();
    const int gx = ceil_div(p.M, t.BM), gy = ceil_div(p.Cout16, t.BN);
    const int blocks = gx * gy;
    int nw = t.NW;
    if (K.kw_nw_force > 0) nw = K.kw_nw_force;
    if (p.bf16 || (p.sb & 1) || t.BM != 16 || t.BN > 48 || (nw == 16 && t.BN > 32)) nw = 4;    // the 8- / 16-wave builds exist for the small fp32 tiles only
    const int steps = ceil_div(p.nchunks, nw);                            // steps per wave without a cross-block split
    int S = t.S;
    if (S <= 0) S = (blocks < 128 && steps >= 32) ? 4 : 1;
    if (S > steps) S = steps;
    int sps = ceil_div(steps, S);
    S = ceil_div(steps, sps);
    if (S > 1) {
        const size_t need = ORE_CONV_CNT_INTS + (size_t)blocks * S * t.BM * t.BN;
        if (!p.tile_cnt || workspace_floats < need || blocks > ORE_CONV_CNT_INTS) { S = 1; sps = steps; }
    }
    bool tile_built = false;
#define KW_BUILT(bm, bn) tile_built = tile_built || (t.BM == bm && t.BN == bn);
    ORE_KW_TILES(KW_BUILT)
#undef KW_BUILT
    if (!tile_built) return none();
    // incremental DMA addressing pays when a tap holds >= 16 chunks (4+ steps between pointer rebuilds): 1x1 layers, deep 3x3 layers
    const int incr = (p.Cin >> 4) >= 4 * nw;
    int ns = 2;                          // (see kw_tile: the minimal ring wins; rings 3 / 4 are tuning aids, fp32 with 4 waves only)
    if (nw == 4 && !p.bf16 && !(p.sb & 1) && K.kw_force[0] > 0 && K.kw_force[2] > 0) ns = K.kw_force[2];
    if ((nw != 4 && nw != 8 && nw != 16) || (ns != 2 && ns != 3 && ns != 4)) {
        ore_set_error("k_conv_kw: no build for tile %dx%d with %d waves, ring %d", t.BM, t.BN, nw, ns);
        return fail(ORE_EINVAL);
    }
    return make_plan(ORE_LAUNCH_KW, t.BM, t.BN, ns, nw, ns == 2 ? incr : 1, p.bf16 ? 1 : (p.sb & 1) ? 2 : 0, gx, gy, choose_xmap(p, gx, gy), S, sps);
}

// the DMA-fed kernels, in the order they are asked: k_conv_kd, k_conv_rf, k_conv_gs, k_conv_kw
ConvPlan plan_dma(const ConvP& p, size_t workspace_floats) {
    if (p.in_mul || p.Cin % 16 != 0) return none();                        // input affine not built here
    ConvPlan pl;
    if (K.kw_force[0] == 0 && K.gs_force[0] == 0) {                         // the lean LDS-DMA kernel, then the register-fed one for the
        if ((pl = plan_kd(p)).launcher || pl.error) return pl;             // smallest-M layers
        if ((pl = plan_rf(p)).launcher) return pl;
    }
    if (p.sb & 1) {                                                         // bf16 storage: every layer runs on one of the two DMA-fed kernels
        // plan from tools/bf16s_sweep.py (profiles/r03_bf16s_sweep.txt): the shared-stage kernel for the two big 1x1 concats and the
        // stride-2 stem_3, the K-split kernel with 32x64 tiles for everything else at M >= 4096 (3x3 at 128 channels: 12-21 vs 21-24 us)
        const bool gs_pick = p.M >= 6400 && ((p.kh == 1 && (p.Cout16 == 112 || p.Cout16 >= 256)) || (p.kh == 3 && p.stride == 2 && p.Cout16 % 128 == 0));
        if (K.kw_force[0] == 0 && (K.gs_force[0] > 0 || gs_pick) && (pl = plan_gs(p)).launcher) return pl;
    } else if (K.kw_force[0] == 0 && (K.gs_force[0] > 0 || p.M >= 16384 || (p.M >= 4096 && p.Cout16 >= 256))) {
        return p.bf16 ? none() : plan_gs(p);                                // (k_conv_gs has no bf16-operand build)
    }
    return plan_kw(p, workspace_floats);
}

// ---- k_conv_igemm.  Tile / split plan.  Goal: >= ~768 waves' worth of blocks (256 CUs x 3) when the layer allows it, slabs small
// enough for the in-kernel last-arriver reduction (splitk * BM*BN*4 bytes per tile stays in the tens of KB).
struct TileCfg { int BM, BN, WGM, WGN, WGK; };

void igemm_tile(int M, int Cout, int nchunks, int req_splitk, bool bf16, TileCfg* t, int* S_out, int* sps_out) {
    const int C16 = round_up(Cout, 16);
    if (K.igemm[0] > 0) {
        *t = {K.igemm[0], K.igemm[1], K.igemm[2], K.igemm[3], K.igemm[4]};
        if (t->BN > C16) t->BN = C16;
        const int nst = ceil_div(nchunks, t->WGK);
        int S = req_splitk > 0 ? req_splitk : 1;
        if (S > nst) S = nst;
        const int sps = ceil_div(nst, S);
        *S_out = ceil_div(nst, sps); *sps_out = sps;
        return;
    }
    // Plan table distilled from tools/conv_tune.py sweeps on MI355X (profiles/r01_conv_tune.txt): small tiles with the K
    // dimension split across the block's waves win almost everywhere -- they keep several blocks resident per CU, which
    // hides the per-step barrier/LDS latency that dominates this kernel -- and cross-block split-K only pays for the
    // deepest K (stage-5 layer 0).
    int bn;
    if (M >= 16384) {
        if (C16 == 64) { if (M >= 65536) *t = {32, 64, 2, 1, 2}; else *t = {64, 64, 4, 1, 1}; }
        else if (C16 % 128 == 0) *t = {64, 128, 2, 2, 1};
        else *t = {64, C16 <= 128 ? C16 : 64, 4, 1, 1};
    } else if (M >= 2048) {
        if (C16 % 64 == 0) { if (C16 >= 256 && !bf16) *t = {64, 64, 2, 1, 2}; else *t = {32, 64, 2, 1, 2}; }
        else if (C16 >= 32) *t = {32, 32, 1, 1, 4};
        else *t = {16, 16, 1, 1, 4};
    } else {
        bn = C16 >= 32 ? 32 : 16;
        *t = {16, bn, 1, 1, 4};
    }
    // K-split tiles, second pass (re-tuned after the K loop lost its barriers, profiles/r01_conv_tune.txt): with wave-private staging
    // the layers of stages 3-4 and the FPN run best at about ONE block per CU -- every CU then pulls each weight row through its
    // memory path once -- so pick the (BM, BN) of the 1x1x4 family with >= 192 blocks and the fewest staged bytes per FLOP,
    // (1/BM + 1/BN) x the padding waste of BN.  (The bf16 builds exist for the first-pass tiles only.)
    // (at M < 2048 only for N < 128: the 128- and 384-channel layers of stage 4 / the FPN -- input affine, fused column sums in the
    // epilogue -- measured slower with the picked tile inside the engine: s4cat 19.7 -> 22.6 us, lat4 11.0 -> 12.4 us)
    const bool ksplit_pick = !bf16 && C16 >= 32 && ((M >= 2048 && M < 16384 && C16 % 64 != 0) || (M >= 1024 && M < 2048 && C16 < 128));
    if (ksplit_pick) {
        static const int bms[2] = {32, 16};
        static const int bns32[8] = {128, 112, 96, 80, 64, 48, 32, 16}, bns16[4] = {64, 48, 32, 16};
        float best = 1e30f;
        for (int a = 0; a < 2; ++a) {
            const int bm = bms[a];
            const int* bns = bm == 32 ? bns32 : bns16;
            for (int b = 0; b < (bm == 32 ? 8 : 4); ++b) {
                const int bnc = bns[b];
                if (bnc > C16) continue;
                const int nt = ceil_div(C16, bnc);
                if (ceil_div(M, bm) * nt < 192) continue;
                const float cost = (1.0f / (float)bm + 1.0f / (float)bnc) * (float)(nt * bnc) / (float)C16;
                if (cost < best) { best = cost; *t = {bm, bnc, 1, 1, 4}; }
            }
        }
    }
    const int nsteps = ceil_div(nchunks, t->WGK);
    const int blocks = ceil_div(M, t->BM) * ceil_div(C16, t->BN);
    int S = req_splitk;
    if (S <= 0) {
        S = 1;
        if (nsteps >= 48 && blocks < 256) {
            S = ceil_div(300, blocks);
            if (S > 4) S = 4;
        }
    }
    if (S > nsteps) S = nsteps;
    if (S < 1) S = 1;
    const int sps = ceil_div(nsteps, S);
    S = ceil_div(nsteps, sps);
    *S_out = S; *sps_out = sps;
}

ConvPlan plan_igemm(const ConvP& p, int req_splitk, size_t workspace_floats) {
    TileCfg t; int S, sps;
    igemm_tile(p.M, p.Cout, p.nchunks, req_splitk, p.bf16, &t, &S, &sps);
    const int gx = ceil_div(p.M, t.BM), gy = ceil_div(p.Cout16, t.BN);
    if (S > 1) {
        const size_t need = ORE_CONV_CNT_INTS + (size_t)gx * gy * S * t.BM * t.BN;
        if (!p.tile_cnt || workspace_floats < need || gx * gy > ORE_CONV_CNT_INTS) {
            if (req_splitk > 1) {
                ore_set_error("ore_conv2d_fwd: split-K %d needs %zu workspace floats (have %zu) and <= %d tiles (have %d)", S, need,
                              workspace_floats, ORE_CONV_CNT_INTS, gx * gy);
                return fail(ORE_ENOMEM);
            }
            S = 1; sps = ceil_div(p.nchunks, t.WGK);       // automatic plan falls back to no split
        }
    }
#define IGEMM_BUILT(bm, bn, wgm, wgn, wgk, hasbf)                                                   \
    if (t.BM == bm && t.BN == bn && t.WGM == wgm && t.WGN == wgn && t.WGK == wgk && (hasbf || !p.bf16)) \
        return make_plan(ORE_LAUNCH_IGEMM, bm, bn, wgm, wgn, wgk, p.bf16, gx, gy, choose_xmap(p, gx, gy), S, sps);
    ORE_IGEMM_BUILDS(IGEMM_BUILT)
#undef IGEMM_BUILT
    ore_set_error("ore_conv2d_fwd: no %skernel for tile %dx%d (%d,%d,%d)", p.bf16 ? "bf16 " : "", t.BM, t.BN, t.WGM, t.WGN, t.WGK);
    return fail(ORE_EINVAL);
}

}  // namespace

// the (Cin, Cout) pairs of 3x3 stride-1 layers a Winograd build exists for
bool conv_wino_covers(int Cout, int Cin) {
    if (Cout <= 0 || Cout % 16 != 0) return false;
    if (Cin == 64) return Cout % 64 == 0;
    if (Cin == 128) return Cout % 32 == 0;
    return Cin == 80 || Cin == 96 || Cin == 112;
}

// per-level Winograd weights: a block serves one level.  The fewest rounds R for which sum_l ceil(batches_l / R) blocks fit a block row
int wino_level_blocks(const ConvP& c, int gy, int* blk0) {
    int nb[4];
    for (int l = 0; l < c.nlev; ++l) nb[l] = c.B * ceil_div(c.lv[l].W, 16) * ceil_div(c.lv[l].H, 4);
    const int G = 256 / gy > c.nlev ? 256 / gy : c.nlev;
    int R = 1;
    for (;; ++R) {
        int need = 0;
        for (int l = 0; l < c.nlev; ++l) need += ceil_div(nb[l], R);
        if (need <= G) break;
    }
    int gx = 0;
    for (int l = 0; l < c.nlev; ++l) { if (blk0) blk0[l] = gx; gx += ceil_div(nb[l], R); }
    if (blk0) blk0[c.nlev] = gx;
    return gx;
}

ConvPlan conv_plan(const ConvP& p, int req_splitk, size_t workspace_floats) {
    ConvPlan pl;
    if (p.w_lstride) {                                     // per-level layers, bf16 storage: the weight-stationary 3x3 kernel or nothing
        if ((pl = plan_ws_sb(p)).launcher) return pl;
        ore_set_error("ore_conv2d_levels_fwd: the weight-stationary bf16 kernel does not cover this per-level launch (64 / 128 channels, Cout %% 64 == 0)");
        return fail(ORE_EINVAL);
    }
    if (p.wino_lstride) {                                  // per-level layers: the Winograd kernel or nothing
        if ((pl = plan_wino(p)).launcher) return pl;
        ore_set_error("ore_conv2d_levels_fwd: the Winograd kernel does not cover this per-level launch (alignment / mode)");
        return fail(ORE_EINVAL);
    }
    if (p.sb & 1) {                                        // bf16 storage: weight-stationary 3x3 kernels, else the DMA-fed kernels (SB builds)
        if ((pl = plan_ws_sb(p)).launcher || (pl = plan_ws_s2(p)).launcher) return pl;
        pl = plan_dma(p, workspace_floats);
        if (pl.launcher || pl.error) return pl;
        ore_set_error("ore_conv2d_fwd: no bf16-storage kernel for this layer (input affine?)");
        return fail(ORE_EINVAL);
    }
    if (K.igemm[0] == 0 && req_splitk <= 1) {
        // several pyramid levels in one launch (the head tower): the 16-pixel-wide patch tiles waste 17-37 % on the 40- and 20-wide
        // levels, k_conv_kw takes it (47 -> 39 us, profiles/r02_kw_sweep.txt)
        if ((pl = plan_wino(p)).launcher) return pl;
        // large M that is not Winograd's: shared-stage LDS-DMA with descriptor addressing (stem_3, the stage-2 / 3 concats)
        if (K.kw_mode && ((pl = plan_gd(p)).launcher || pl.error)) return pl;
        const bool kw_first = K.kw_mode == 2 || (K.kw_mode == 1 && p.nlev > 1);
        if (!kw_first && (pl = plan_patch(p)).launcher) return pl;
        if (K.kw_mode) {                                   // small / medium M: the DMA-fed kernels
            pl = plan_dma(p, workspace_floats);
            if (pl.launcher || pl.error) return pl;
            if (kw_first && K.kw_mode != 2 && (pl = plan_patch(p)).launcher) return pl;   // not covered after all: the patch kernels get their turn
        }
    }
    return plan_igemm(p, req_splitk, workspace_floats);
}

}  // namespace oreconv

using namespace oreconv;

// Tuning aid (tools/conv_tune.py): force the tile configuration of subsequent ore_conv2d*_fwd calls; BM = 0 restores the
// automatic plan.  Not used by the product path.
extern "C" int ore_conv_set_plan_override(int32_t BM, int32_t BN, int32_t WGM, int32_t WGN, int32_t WGK) {
    ConvKnobs& k = g_knobs;
    switch (BM) {
    case -1: k.patch_mode = BN; k.igemm[0] = 0; break;                           // 3x3 patch kernel mode (also restores the automatic tile)
    case -2: k.kw_mode = BN; k.igemm[0] = 0; break;                              // k_conv_kw mode (0 / 1 / 2)
    case -3: k.kw_force[0] = BN; k.kw_force[1] = WGM; k.kw_force[2] = WGN; k.kw_force[3] = WGK; break;   // (tile BM, tile BN, ring depth, split-K) of k_conv_kw
    case -4: k.gs_force[0] = BN; k.gs_force[1] = WGM; if (WGN > 0) k.gs_ns = WGN; break;                 // tile (and ring depth) of k_conv_gs
    case -5: k.xmap_force = BN; break;                                           // block -> tile mapping (-1 auto, 0, 1, 2)
    case -6: k.kw_nw_force = BN; break;                                          // waves per block of k_conv_kw (4 / 8 / 16)
    case -7: k.wino_mode = BN; break;                                            // Winograd kernel 0 off / 1 automatic / 2 forced
    case -8: k.ws_sb_mode = BN; break;                                           // bf16-storage weight-stationary 3x3 kernel: 0 off, 1 auto
    case -9: k.ws_s2_mode = BN; break;                                           // weight-stationary stride-2 kernel (stem_3) 0 off / 1 on
    case -10: k.rf_mode = BN; break;                                             // register-fed small-M kernel 0 off / 1 automatic / 2 wherever it applies
    case -11: k.rf_force[0] = BN; k.rf_force[1] = WGM; k.rf_force[2] = WGN; break;   // force its build (GB, NW, MAXS)
    case -12: k.kd_mode = BN; break;                                             // lean LDS-DMA kernel 0 off / 1 automatic / 2 wherever it applies
    case -13: k.kd_force[0] = BN; k.kd_force[1] = WGM; k.kd_force[2] = WGN; k.kd_force[3] = WGK; break;   // force its build (BM, BN, NW, SB)
    case -14: k.gd_mode = BN; break;                                             // shared-stage descriptor kernel 0 off / 1 automatic
    case -15: k.gd_force[0] = BN; k.gd_force[1] = WGM; k.gd_force[2] = WGN; break;   // force its build (BM, BN, NS)
    case -16: k.gd_dbg = BN; break;                                              // its ablation flags (trace build only; no effect in the product library)
    default: k.igemm[0] = BM; k.igemm[1] = BN; k.igemm[2] = WGM; k.igemm[3] = WGN; k.igemm[4] = WGK; break;
    }
    return ORE_OK;
}

extern "C" int ore_conv_reset_plan_overrides(void) {
    g_knobs = ConvKnobs{};
    return ORE_OK;
}
