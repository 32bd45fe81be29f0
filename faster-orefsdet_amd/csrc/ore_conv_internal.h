// Shared by the conv translation units of libore_hip.so: the kernel parameter block, the planner (ore_conv_plan.cpp) that picks the
// kernel and build of every ore_conv2d*_fwd call, and the launchers that execute its plans.
#pragma once
#include "ore_common.h"

namespace oreconv {

struct Lvl { int orow0, irow0, H, W, Ho, Wo; };

struct ConvP {
    const float* in; int in_ld, in_coff;
    int B, Cin;
    int nlev; Lvl lv[4];
    const float* w;
    int Cout, Cout16, kh, kw, stride, pad, M, K;
    const float* scale; const float* shift; int ep_stride; int relu_cout;
    const float* in_mul; const float* in_add; int in_relu;
    const float* add; int add_ld, add_coff, add_H, add_W;
    float* out; int out_ld, out_coff;
    float* colsum;                       // [gridDim.x][Cout16] or null
    int splitk, steps_per_split, nchunks;
    float* ws; int* tile_cnt;
    int bf16;                            // ORE_CONV_BF16: operands rounded to bf16 as the fragments leave LDS, one 16x16x16 bf16 MFMA per 16 channels
    int xmap;                            // tile <-> block mapping of k_conv_kw: 0 = blockIdx, 1 / 2 = XCD-contiguous, M- / N-major (tile_of_block)
    int sb;                              // bf16 STORAGE mode (ore_conv_desc.storage): bit 0 = in / w are bf16 (in_ld, in_coff, Cin, K then count
                                         // PAIRS of bf16 = 4-byte units, a K chunk is 32 channels), bit 1 = out is bf16, bit 2 = add is bf16
    const float* wino;                   // Winograd F(2x2,3x3) transformed weights [16][Cout16][Cin] (ore_winograd_weight_fwd) or null
    size_t w_lstride;                    // bf16 storage, per-level weights for k_conv3x3_ws: level l's packed weights start w_lstride 4-byte units further
    size_t wino_lstride;                 // several levels, one set of weights each: level l's transformed weights start wino_lstride floats further (0 = shared)
};

// Which tile does this block compute?  Workgroups are dealt round-robin over the 8 XCDs in linear block order (observed, MI355X guide),
// each XCD has its own 4 MB L2, and with the plain (blockIdx.x, blockIdx.y) mapping the N tiles of one M tile -- the same activation
// rows -- usually land on different XCDs, and every XCD reads every weight column: the L2 -> fabric traffic of a small-M layer is up
// to 8x its operands.  xmap gives the blocks of one residue class (lin % 8 = one XCD) a CONTIGUOUS run of tiles in M-major (1: an
// XCD owns a range of rows and reads them once) or N-major order (2: an XCD owns a range of output channels and reads those weights
// once).  A pure relabelling: every tile is computed exactly once by exactly the same code, results are bit-identical.
__device__ __forceinline__ void tile_of_block(int xmap, int& bx, int& by) {
    bx = blockIdx.x; by = blockIdx.y;
    if (xmap == 0) return;
    const int gx = gridDim.x, gy = gridDim.y, T = gx * gy;
    const int lin = by * gx + bx, r = lin & 7, k = lin >> 3;
    const int q = T >> 3, rem = T & 7;
    const int t = r * q + min(r, rem) + k;               // residue class r holds q (+1 if r < rem) blocks
    if (xmap == 1) { bx = t / gy; by = t - bx * gy; }
    else { by = t / gx; bx = t - by * gx; }
}

// Row m of the GEMM -> pyramid level, image and output pixel (k_conv_igemm, k_conv_kw, k_conv_gs: rows may span several levels).
__device__ __forceinline__ void decode_row(const ConvP& p, int m, int& lvl, int& b, int& oy, int& ox) {
    lvl = 0;
#pragma unroll
    for (int l = 1; l < 4; ++l)
        if (l < p.nlev && m >= p.lv[l].orow0) lvl = l;
    const Lvl& L = p.lv[lvl];
    const int r = m - L.orow0, hw = L.Ho * L.Wo;
    b = r / hw;
    const int q = r - b * hw;
    oy = q / L.Wo;
    ox = q - oy * L.Wo;
}

// Limits of the buffer-descriptor kernels that the planner's eligibility tests share with them
constexpr unsigned kOOB = 0x80000000u;   // a byte offset beyond every buffer's num_records (< 2 GB here, and kOOB + an instruction offset
                                         // cannot wrap): the load returns zeros
constexpr int kGdTab = 64;               // k_conv_gd chunk table entries: K up to 1024 (stem_3: 36, the concats: 20 / 22)
constexpr int kKdTab = 512;              // k_conv_kd: K up to 8192 (the second-stage GEMM)
constexpr int kRfTab = 256;              // k_conv_rf (3x3 layers): covers K = 9 * 448 channels

// The instantiated builds, one list per kernel: the planner takes a build only from its kernel's list, the launcher dispatches on it.
// k_conv_igemm X(BM, BN, WGM, WGN, WGK, HASBF); HASBF: also built for bf16 operands (the tiles of the automatic plan)
#define ORE_IGEMM_BUILDS(X)                                                                                                         \
    /* large-M tiles: 4 waves along M, whole N in the block */                                                                     \
    X(128, 16, 4, 1, 1, 0) X(128, 32, 4, 1, 1, 0) X(128, 48, 4, 1, 1, 0) X(128, 64, 4, 1, 1, 0)                                     \
    X(128, 80, 4, 1, 1, 0) X(128, 96, 4, 1, 1, 0) X(128, 112, 4, 1, 1, 0) X(128, 128, 2, 2, 1, 0)                                   \
    X(64, 16, 4, 1, 1, 1) X(64, 32, 4, 1, 1, 1) X(64, 48, 4, 1, 1, 1) X(64, 64, 4, 1, 1, 1)                                         \
    X(64, 80, 4, 1, 1, 1) X(64, 96, 4, 1, 1, 1) X(64, 112, 4, 1, 1, 1) X(64, 128, 2, 2, 1, 1)                                       \
    /* mid/small-M tiles: waves split K inside the block */                                                                        \
    X(64, 64, 2, 1, 2, 0) X(64, 32, 2, 1, 2, 0) X(64, 16, 2, 1, 2, 0) X(64, 48, 2, 1, 2, 0)                                         \
    X(32, 64, 1, 1, 4, 0) X(32, 48, 1, 1, 4, 0) X(32, 32, 1, 1, 4, 1) X(32, 16, 1, 1, 4, 0)                                         \
    X(16, 64, 1, 1, 4, 0) X(16, 48, 1, 1, 4, 0) X(16, 32, 1, 1, 4, 1) X(16, 16, 1, 1, 4, 1)                                         \
    X(64, 128, 2, 1, 2, 0) X(64, 96, 2, 1, 2, 0) X(64, 80, 2, 1, 2, 0) X(64, 112, 2, 1, 2, 0)                                       \
    X(32, 128, 1, 1, 4, 0) X(32, 96, 1, 1, 4, 0) X(32, 80, 1, 1, 4, 0) X(32, 112, 1, 1, 4, 0)                                       \
    X(32, 128, 2, 1, 2, 0) X(32, 64, 2, 1, 2, 1) X(32, 32, 2, 1, 2, 0)                                                              \
    X(128, 64, 2, 1, 2, 0) X(128, 128, 2, 1, 2, 0)
// k_conv_gd X(BM, BN, WGM, WGN, NS, BF); BF = 1: the bf16-operand builds (four-wave tiles with the default LDS limit)
#define ORE_GD_BUILDS(X)                                                                                                            \
    X(64, 128, 2, 2, 4, 1) X(64, 64, 2, 2, 4, 1) X(32, 64, 1, 4, 4, 1)                                                              \
    X(64, 128, 2, 2, 4, 0) X(64, 64, 2, 2, 4, 0) X(64, 112, 4, 1, 4, 0) X(128, 64, 4, 1, 4, 0) X(128, 128, 2, 2, 4, 0)              \
    X(32, 128, 1, 4, 4, 0) X(128, 112, 4, 1, 4, 0) X(208, 64, 1, 4, 4, 0) X(224, 64, 1, 4, 4, 0) X(112, 64, 1, 4, 4, 0)             \
    X(96, 128, 2, 2, 4, 0) X(64, 128, 2, 2, 2, 0) X(128, 128, 2, 2, 2, 0) X(208, 64, 1, 4, 2, 0) X(128, 112, 4, 1, 2, 0)            \
    X(128, 128, 2, 4, 4, 0) X(112, 128, 1, 8, 4, 0) X(128, 112, 8, 1, 4, 0) X(64, 128, 2, 4, 4, 0) X(128, 64, 4, 2, 4, 0)           \
    X(64, 64, 2, 4, 4, 0) X(128, 128, 2, 4, 2, 0) X(112, 128, 1, 8, 2, 0) X(80, 64, 1, 4, 4, 0) X(80, 128, 1, 4, 4, 0)              \
    X(48, 64, 1, 4, 4, 0) X(32, 64, 1, 4, 4, 0)
// k_conv_kd X(BM, BN, NW, SB): every build keeps NW x 2 x SB x (BM + BN) / 16 KiB of LDS <= 160 KiB (16x16 at 4 waves x 8 steps = 128 KiB:
// one block per CU)
#define ORE_KD_BUILDS(X)                                                                                                            \
    X(16, 16, 4, 4) X(16, 16, 4, 8) X(16, 16, 8, 4) X(16, 16, 16, 2) X(16, 32, 4, 4) X(16, 32, 8, 2) X(32, 32, 4, 4) X(32, 32, 8, 2)  \
    X(16, 48, 4, 4) X(16, 48, 8, 2) X(16, 64, 4, 2) X(16, 80, 4, 2) X(32, 64, 4, 2) X(32, 80, 4, 2) X(64, 64, 4, 2) X(32, 48, 4, 2)    \
    X(32, 16, 4, 4)
// k_conv_rf X(GB, NW, MAXS)
#define ORE_RF_BUILDS(X) \
    X(1, 4, 8) X(1, 4, 12) X(1, 4, 16) X(1, 8, 12) X(1, 8, 16) X(1, 8, 20) X(1, 16, 12) X(2, 4, 12) X(2, 4, 16) X(2, 8, 12)
// k_conv_gs X(BM, BN, WGM, WGN), each with ring depths 3 / 4 / 6 where they fit (gs_fits)
#define ORE_GS_BUILDS(X) \
    X(64, 112, 4, 1) X(64, 128, 2, 2) X(64, 64, 2, 2) X(128, 64, 4, 1) X(128, 128, 2, 2) X(32, 128, 1, 4) X(128, 112, 4, 1) X(64, 80, 4, 1) X(32, 64, 2, 2)
// k_conv_kw X(BM, BN): 4 waves with rings 2 / 3 / 4; 8 waves for BM = 16, BN <= 48 and 16 waves for BN <= 32 (fp32 operands, ring 2)
#define ORE_KW_TILES(X) \
    X(16, 16) X(16, 32) X(16, 48) X(16, 64) X(16, 80) X(32, 16) X(32, 32) X(32, 48) X(32, 64) X(32, 80)
constexpr bool gs_fits(int bm, int bn, int ns) { return ((bm + bn) / 16 + 3) / 4 * (ns - 1) <= 63 && (size_t)ns * (bm + bn) * 64 <= 150 * 1024; }

// Tuning aids (ore_conv_set_plan_override codes in brackets; ore_conv_reset_plan_overrides restores these defaults).  Not used by the
// product path.
struct ConvKnobs {
    int patch_mode = -1;        // (-1) 3x3 patch kernels: -1 automatic, 0 never, 4 / 8 force TH, 16 = double-buffered 8-wave kernel,
                                //      102 = weight-stationary kernels (2-row tiles; Cin = 64 or 128)
    int kw_mode = 1;            // (-2) 0: k_conv_kw off, 1: automatic (after the 3x3 patch kernels), 2: wherever it applies
    int kw_force[4] = {};       // (-3) k_conv_kw {BM, BN, NS, split-K}; BM = 0 -> automatic
    int gs_force[2] = {};       // (-4) k_conv_gs {BM, BN}; 0 -> automatic
    int gs_ns = 3;              // (-4, .., .., ns > 0) ring depth of k_conv_gs (3 / 4 / 6)
    int xmap_force = -1;        // (-5) block -> tile mapping: -1 automatic, 0 / 1 / 2 forced
    int kw_nw_force = 0;        // (-6) waves per block of k_conv_kw (4 / 8 / 16); 0 -> the plan's
    int wino_mode = 1;          // (-7) Winograd: 0 off, 1 automatic (by row count), 2 wherever it applies
    int ws_sb_mode = 1;         // (-8) bf16-storage weight-stationary 3x3 kernel: 0 off (k_conv_gs / k_conv_kw), 1 automatic, 3 = 128-channel
                                //      layers back on k_conv_kw
    int ws_s2_mode = 1;         // (-9) 0 = stem_3 (3x3 stride 2, 64 input channels) stays on k_conv_igemm / k_conv_gs
    int rf_mode = 1;            // (-10) k_conv_rf: 0 off, 1 automatic, 2 wherever it applies
    int rf_force[3] = {};       // (-11) its build {GB, NW, MAXS}; 0 -> automatic
    int kd_mode = 1;            // (-12) k_conv_kd: 0 off, 1 automatic, 2 wherever it applies
    int kd_force[4] = {};       // (-13) its build {BM, BN, NW, SB}; 0 -> automatic
    int gd_mode = 1;            // (-14) k_conv_gd: 0 off, 1 automatic, 2 automatic + every 1x1 layer at training sizes, 3 automatic with
                                //       the round-4 limit M <= 32768
    int gd_force[3] = {};       // (-15) its build {BM, BN, NS}; 0 -> automatic
    int gd_dbg = 0;             // (-16) its ablation flags (trace build only)
    int igemm[5] = {};          // (BM > 0) k_conv_igemm tile {BM, BN, WGM, WGN, WGK}; BM = 0 -> automatic
};
extern ConvKnobs g_knobs;

using ConvPlan = ore_conv_plan_t;
// The kernel, build, split and grid of one conv call (ConvP as ore_conv2d*_fwd fills it; p.tile_cnt = the workspace or null).  No HIP
// calls; when no kernel takes the call the plan holds the error code and the last-error string says why.
ConvPlan conv_plan(const ConvP& p, int req_splitk, size_t workspace_floats);
bool conv_wino_covers(int Cout, int Cin);                  // a Winograd build exists for this 3x3 stride-1 layer
int wino_level_blocks(const ConvP& p, int gy, int* blk0);  // per-level Winograd weights: blocks [blk0[l], blk0[l+1]) serve level l; returns gx

// One launcher per kernel: fills its argument block from p and runs the build the plan names.
int launch_ws(const ConvP& p, const ConvPlan& pl, hipStream_t st);       // ore_conv.hip: k_conv3x3_ws (WS_SB, WS64, WS128)
int launch_patch(const ConvP& p, const ConvPlan& pl, hipStream_t st);    // k_conv3x3_patch<4 | 8>, k_conv3x3_patch_db
int launch_igemm(const ConvP& p, const ConvPlan& pl, hipStream_t st);    // k_conv_igemm
int launch_wino(const ConvP& p, const ConvPlan& pl, hipStream_t st);     // ore_conv_wino.hip: k_conv3x3_wino, k_conv3x3_wino_nu
int launch_gd(const ConvP& p, const ConvPlan& pl, hipStream_t st);       // ore_conv_gd.hip
int launch_kd(const ConvP& p, const ConvPlan& pl, hipStream_t st);       // ore_conv_kd.hip
int launch_rf(const ConvP& p, const ConvPlan& pl, hipStream_t st);       // ore_conv_rf.hip
int launch_gs(const ConvP& p, const ConvPlan& pl, hipStream_t st);       // ore_conv_kw.hip: k_conv_gs
int launch_kw(const ConvP& p, const ConvPlan& pl, hipStream_t st);       // k_conv_kw
// ore_conv_gd.hip: the second-stage GEMM as a K split over blocks (called directly, not planned)
int conv_gd_splitk(const float* in, int in_ld, const float* w, int M, int K, int Cout16, float* parts, int S, hipStream_t st);

// ore_conv_wgrad.hip: dw_oihw[co][ci][tap] = beta * dw + sum_z slab[z][co][tap][ci] over S slabs `stride` floats apart, in the fixed order of
// k_wgrad_reduce<G> (G by S and the output size); db / beta_b: the bias part behind every slab's weight part, or null.  Also used by
// ore_conv_s2grad.hip (taps = 9; taps = 1 with "Cin" = 27 for the flat [Cout][27] gradient of stem_1).
int launch_wgrad_reduce(const float* slab, int S, int Cout, int taps, int Cin, float beta, float* dw_oihw, long long stride, float* db,
                        float beta_b, hipStream_t st);

}  // namespace oreconv
