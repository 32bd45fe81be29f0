/* ore_hip.h -- C-ABI of libore_hip.so, the MI355X (gfx950) hot path of Faster-OreFSDet.
 *
 * The reference (MVME-HBUT/Faster-OreFSDet) is pure Python on PyTorch and has no FFI boundary of
 * its own; its plug-in surface is Detectron2's registry + nn.Module call protocol.  This header is
 * what the Python host side (faster-orefsdet_amd/orehip/, ctypes) binds; every entry point names
 * the reference interface it replaces (ref: = reference repo path, d2z: = path inside the
 * reference's vendored detectron2.7z).
 *
 * Conventions
 *   - all data pointers are DEVICE pointers unless the name ends in _host;
 *   - activations are fp32 NHWC with an explicit channel stride (ld) and channel offset (coff), so a
 *     layer can read/write a channel slice of a wider buffer (OSA concat is never materialised by a copy);
 *   - the caller owns every buffer; kernels are enqueued on the hipStream_t passed as void* and
 *     return without synchronising; nothing is allocated inside an op call;
 *   - return value: 0 = ok, negative = error (ORE_E*), message via ore_last_error();
 *   - thread-compatible: one ore_engine per process/GPU, no hidden global state besides the
 *     last-error string.
 */
#ifndef ORE_HIP_H_
#define ORE_HIP_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ORE_OK 0
#define ORE_EINVAL (-22)  /* bad shape / unsupported configuration */
#define ORE_ENOMEM (-12)  /* workspace too small */
#define ORE_EHIP (-5)     /* HIP runtime error */
#define ORE_ENOENT (-2)   /* unknown tensor name */

const char* ore_last_error(void);
int ore_version(void);
/* Algorithmic (direct-convolution) FLOPs of the per-op conv calls made by this process since the last reset -- ore_conv2d_fwd,
 * ore_conv2d_levels_fwd, the two weight-gradient calls, the two stem_1 calls: 2 * rows * Cout * Cin * kh * kw each -- and the number of such
 * calls.  Host-side bookkeeping only (calls captured into a hipGraph count when captured, not when replayed).  bench.py prices the
 * training step with it ("report exact sum from the layer table in code"). */
int ore_flop_counter_read(double* flops, int64_t* calls, int32_t reset);

/* ------------------------------------------------------------------ low-level ops ------------ */

/* Fused conv descriptor: implicit-GEMM NHWC conv on fp32 MFMA (v_mfma_f32_16x16x4_f32) with
 *   optional per-(batch,channel) affine(+ReLU) on the INPUT  (eSE scale folded into the consumer,
 *                                                            GroupNorm+ReLU folded into the head convs)
 *   y = acc * scale[n] + shift[n]                            (FrozenBN / bias / Scale)
 *   y += nearest2x(add)[b, oy/2, ox/2, n]                    (FPN top-down sum)
 *   ReLU on output channels n < relu_cout.
 * Replaces: F.conv2d + FrozenBatchNorm2d + ReLU  d2z:layers/wrappers.py:48-91, d2z:layers/batch_norm.py:44-66,
 *           d2z:modeling/backbone/vovnet.py:205-235 (conv3x3/conv1x1), d2z:modeling/backbone/fpn.py:126-145,
 *           ref:CenterNet2/centernet/modeling/dense_heads/centernet_head.py:141-161.
 * Requirements: Cin % 16 == 0; weights packed by ore_pack_conv_weight_host ([Cout16][kh*kw*Cin], tap-major).
 * Split-K across blocks is reduced inside the launch (last-arriver slab reduction, deterministic); it needs the
 * workspace described below. */
typedef struct ore_conv_desc {
    const float* in;   int32_t in_ld, in_coff;
    int32_t B, H, W, Cin;
    const float* w;    /* packed weights */
    int32_t Cout, kh, kw, stride, pad;
    const float* scale;   /* [Cout] or NULL (= 1) */
    const float* shift;   /* [Cout] or NULL (= 0) */
    int32_t relu_cout;    /* ReLU applied to output channels < relu_cout */
    const float* in_mul;  /* [B][Cin] or NULL */
    const float* in_add;  /* [B][Cin] or NULL */
    int32_t in_relu;      /* ReLU after the input affine */
    const float* add;  int32_t add_ld, add_coff;  /* [B][ceil(Ho/2)][ceil(Wo/2)] x add_ld, or NULL */
    float* out;        int32_t out_ld, out_coff;
    int32_t splitk;       /* 0 = choose automatically, 1 = none */
    float* workspace;  size_t workspace_floats;
    float* colsum;        /* optional [ore_conv_colsum_rows()][Cout16]: per-row-tile column sums of y (eSE average pool) */
    const float* w_wino;  /* optional: the same weights in Winograd F(2x2,3x3) form (ore_winograd_weight_fwd).  When given, 3x3
                           * stride-1 pad-1 layers that ore_winograd_covers() and that have enough rows (>= 1500 at Cin 64 / 128, >= 3000 at
                           * Cin 80 / 96 / 112) run on the Winograd kernels (2.25x fewer multiplies, fp32 throughout); NULL = direct
                           * kernels only */
    int32_t storage;      /* ORE_ST_F32 (0): every tensor is fp32.  ORE_ST_BF16: `in`, `w` (ore_pack_conv_weight_bf16_host), `add` and `out`
                           * are bf16 tensors (ld / coff count ELEMENTS), accumulation, scale / shift and colsum stay fp32, the output is
                           * rounded once (nearest even) when it is stored and colsum sums the ROUNDED values.  ORE_ST_BF16_F32OUT: the
                           * same with an fp32 `out` (the detection head's outputs).  The input buffer must extend 32 bytes past its
                           * last row when Cin % 32 == 16 (the last K chunk of a row reads 16 channels further, against zero weights).
                           * Both bf16 modes need in_ld and in_coff in multiples of 8 elements (16-byte aligned input slices) and take no
                           * input affine: a call with in_mul returns ORE_EINVAL.  Column sums with an fp32 `out` do not run on k_conv_kd
                           * (k_conv_kw takes the call). */
    int64_t w_wino_level_stride; /* ore_conv2d_levels_fwd only.  0: all levels share the weights.  Otherwise the levels are DIFFERENT layers of
                           * one shape (the three FPN output convs, d2z:modeling/backbone/fpn.py:139-145): level l's Winograd weights start
                           * l * w_wino_level_stride floats after w_wino, its scale / shift l * ep_stride floats after scale / shift; `w` is
                           * not read.  Winograd kernels only (3x3, Cin 64 / 128, fp32 storage), any row count; else ORE_EINVAL. */
    int64_t w_level_stride; /* the same for ORE_ST_BF16 storage: level l's packed bf16 weights start l * w_level_stride ELEMENTS after `w`
                           * (3x3, 64 / 128 input channels, Cout % 64 == 0: the weight-stationary kernel, one tile per block); else ORE_EINVAL. */
} ore_conv_desc;
#define ORE_ST_F32 0
#define ORE_ST_BF16 1
#define ORE_ST_BF16_F32OUT 2
/* bf16 packed weights for ORE_ST_BF16 convs: [Cout16][kh*kw][round_up(Cin, 32)] bf16 (nearest even), zero beyond Cout / Cin. */
size_t ore_packed_weight_bf16_elems(int32_t Cout, int32_t Cin, int32_t kh, int32_t kw);
int ore_pack_conv_weight_bf16_host(const float* w_oihw, int32_t Cout, int32_t Cin, int32_t kh, int32_t kw, uint16_t* dst);

/* Winograd F(2x2,3x3) form of packed 3x3 weights: U_p = G g G^T per (Cout, Cin) pair for the 16 positions p, computed on the device in
 * fp32 (the halves in G are exact), stored in the kernel's MFMA-fragment order [16][Cout16/16][Cin/16][64 lanes][4] (opaque to callers).  `packed_w` is ore_pack_conv_weight_host's layout for kh = kw = 3; U needs
 * ore_winograd_weight_floats(Cout, Cin) floats.  Call again whenever the weights change.  ore_winograd_covers: 1 if a Winograd build
 * exists for a 3x3 stride-1 pad-1 layer of these widths (Cin 64 with Cout % 64 == 0, Cin 128 with Cout % 32 == 0, Cin 80 / 96 / 112 with
 * Cout % 16 == 0); for other layers ore_conv_desc.w_wino is ignored. */
int32_t ore_winograd_covers(int32_t Cout, int32_t Cin);
size_t ore_winograd_weight_floats(int32_t Cout, int32_t Cin);
int ore_winograd_weight_fwd(const float* packed_w, int32_t Cout, int32_t Cin, float* U, void* stream);

/* Workspace contract: the first ORE_CONV_CNT_INTS 32-bit words are split-K arrival counters and must be ZERO on entry;
 * every launch leaves them zero again (the last arriver resets its counter).  The rest holds the fp32 partial slabs. */
#define ORE_CONV_CNT_INTS 4096
#define ORE_CONV_WS_FLOATS ((size_t)ORE_CONV_CNT_INTS + ((size_t)8 << 20))
size_t ore_conv_workspace_floats(void);          /* recommended workspace size (floats) */
int32_t ore_conv_colsum_rows(const ore_conv_desc* d);   /* number of row tiles (= rows of d->colsum) the plan will use */

int ore_conv2d_fwd(const ore_conv_desc* d, void* stream);
/* Tuning aid (tools/conv_tune.py): force the block tile (BM x BN, waves WGM x WGN x WGK) of subsequent conv calls;
 * BM = 0 restores the automatic plan; BM = -1 sets the 3x3 patch-kernel mode to BN (-1 automatic, 0 off, 4 / 8 forced tile
 * height, 16 = double-buffered 8-wave variant, 102 = weight-stationary persistent kernel for Cin = 64 / 128); BM = -7 sets the
 * Winograd mode to BN (0 off, 1 automatic, 2 wherever it applies).  The product path never calls it. */
int ore_conv_set_plan_override(int32_t BM, int32_t BN, int32_t WGM, int32_t WGN, int32_t WGK);
/* Test hook: the launcher this host thread's last ore_conv2d_fwd / ore_conv2d_levels_fwd call ran (ORE_LAUNCH_*; ORE_LAUNCH_NONE
 * when the call launched nothing), and in *split (if not null) the cross-block split-K S it used (1 = none). */
#define ORE_LAUNCH_NONE 0
#define ORE_LAUNCH_WINO 1           /* k_conv3x3_wino<64 | 128> */
#define ORE_LAUNCH_WINO_NU 2        /* k_conv3x3_wino_nu (80 / 96 / 112 input channels) */
#define ORE_LAUNCH_GD 3             /* k_conv_gd */
#define ORE_LAUNCH_PATCH4 4         /* k_conv3x3_patch<4> */
#define ORE_LAUNCH_PATCH8 5         /* k_conv3x3_patch<8> */
#define ORE_LAUNCH_PATCH_DB 6       /* k_conv3x3_patch_db (8-row double-buffered) */
#define ORE_LAUNCH_WS64 7           /* k_conv3x3_ws<2, 64> */
#define ORE_LAUNCH_WS128 8          /* k_conv3x3_ws<2, 128> */
#define ORE_LAUNCH_KD 9             /* k_conv_kd */
#define ORE_LAUNCH_RF 10            /* k_conv_rf */
#define ORE_LAUNCH_GS 11            /* k_conv_gs */
#define ORE_LAUNCH_KW 12            /* k_conv_kw (split-K possible) */
#define ORE_LAUNCH_IGEMM 13         /* k_conv_igemm (split-K possible) */
#define ORE_LAUNCH_WS_SB 14         /* k_conv3x3_ws, bf16 storage */
int32_t ore_conv_last_launch(int32_t* split);
/* Tuning aid: restore every ore_conv_set_plan_override setting to the automatic plan (the precision is left as it is). */
int ore_conv_reset_plan_overrides(void);
/* The plan an ore_conv2d_fwd (n_levels = 0) or ore_conv2d_levels_fwd call with these arguments makes under the current settings; no
 * GPU work.  Returns ORE_OK, or the error code the call would return (the last-error string says why; out->launcher is then
 * ORE_LAUNCH_NONE).  Pointers are only tested for null and alignment. */
typedef struct ore_conv_plan_t {
    int32_t launcher;          /* ORE_LAUNCH_* */
    int32_t error;             /* ORE_OK or the call's error code */
    int32_t bm, bn;            /* rows x output channels of a block tile (3x3 tile kernels: image rows of a tile x channels per block) */
    int32_t build[4];          /* the launcher's other build parameters (waves, ring depth, ...) */
    int32_t splitk, steps_per_split, xmap;   /* cross-block split-K, K steps per split, block -> tile mapping (tile_of_block) */
    int32_t gx, gy;            /* grid */
} ore_conv_plan_t;
int ore_conv_plan(const ore_conv_desc* d, int32_t n_levels, const int32_t* H, const int32_t* W, int32_t ep_stride, ore_conv_plan_t* out);
/* Operand precision of the MFMA conv kernels for all subsequent ore_conv2d*_fwd launches (BASELINE configs[4], "bf16 MFMA conv
 * path + fp32 NMS"; the reference itself is fp32 only, ref:configs/fsod/finetune_vovnet.yaml).  ORE_CONV_FP32 (default): fp32
 * operands, v_mfma_f32_16x16x4_f32.  ORE_CONV_BF16: tensors stay fp32 in HBM and LDS, both operands are rounded to bf16 (nearest
 * even) as they are fed to v_mfma_f32_16x16x16_bf16, fp32 accumulation and epilogue.  stem_1 (Cin = 3), the depthwise
 * correlation, GroupNorm, top-k / NMS and the second-stage GEMM of an engine always run in fp32.  An engine keeps the mode that was
 * in force when it was created.
 * What an ENGINE's pass rounds in this mode, launch by launch (tests/test_hip_bf16_engine.py holds each launch to it on the engine's own
 * buffers, tests/bf16_engine_ref.py is the contract in float64):
 *   - rounded (both operands, as they enter the conv): stem_2, stem_3, every OSA layer and concat conv, the 1x1 reduction conv of a
 *     depthwise stage, the FPN laterals, conv3 and the head's tower conv.  An input fold -- relu(x * mul + add), the eSE gate as
 *     in_mul -- is computed in fp32 and rounded AFTER it;
 *   - fp32, nothing rounded: stem_1, the max-pools, the eSE gates, the depthwise-separable units (taps and pointwise), the identity-block
 *     tails, the correlation, GroupNorm + ReLU + the head's (l,t,r,b | hm) conv (one VALU kernel), everything behind the head;
 *   - the three FPN output convs run as ONE per-level Winograd launch (w_wino_level_stride), and a per-level Winograd launch multiplies
 *     in fp32 whatever this mode says: the engine's p3 .. p5 are conv_fp32(lat, W), nearer to the fp32 network than the mode asks for.
 *     A plain ore_conv2d_fwd call of the same layer rounds its operands;
 *   - with ONE image per pass the eSE gate of a one-block stage reaches its FPN lateral folded into the weight (the gate kernel writes
 *     fp32(g * W), the lateral is a plain conv on it): conv(round(x), round(fp32(g * W))).  With more images per pass the gate is the
 *     conv's input multiplier: conv(round(fp32(x * g)), round(W)).  A one-image pass and a batched pass of the same image therefore
 *     differ at the laterals by a bf16 rounding in this mode (2e-3 .. 6e-3 of the map), whereas in fp32 they differ by summation order
 *     only.  (A stage that ends in an identity block holds its whole output: its lateral is a plain rounded conv in both passes.) */
#define ORE_CONV_FP32 0
#define ORE_CONV_BF16 1
/* ORE_CONV_BF16S -- bf16 STORAGE (BASELINE configs[4] as a byte-saving path): an engine created under this mode keeps every activation
 * between its layers as a bf16 tensor in HBM (the producer's epilogue rounds once, nearest even), packs bf16 weights, stages bf16
 * tiles in LDS and multiplies with v_mfma_f32_16x16x32_bf16 (fp32 accumulate).  fp32 stay: the image, FrozenBN / bias / eSE gate /
 * GroupNorm statistics and their arithmetic, the (l,t,r,b | heat-map) head outputs, top-k / decode / NMS, ROIAlign's output and the
 * second-stage GEMM and predictor.  One image per pass (max_batch = 1).  Plain ore_conv2d*_fwd calls are not affected by this mode:
 * they choose per call through ore_conv_desc.storage. */
#define ORE_CONV_BF16S 2
int ore_conv_set_precision(int32_t mode);
int32_t ore_conv_get_precision(void);
/* The same 'same'-padded stride-1 conv over several pyramid levels in ONE launch (shared weights; CenterNet head / conv3):
 * rows are level-major [level][b][y][x] in the input and output matrices (d->H, d->W ignored), scale/shift may differ per
 * level (ep_stride floats apart, 0 = shared), in_mul/in_add are indexed [level*B + b][Cin]. */
int ore_conv2d_levels_fwd(const ore_conv_desc* d, int32_t n_levels, const int32_t* H, const int32_t* W,
                          int32_t ep_stride, void* stream);

/* Host helper: OIHW fp32 -> packed [Cout16][kh][kw][Cin] (rows >= Cout zero). dst has ore_packed_weight_floats(). */
size_t ore_packed_weight_floats(int32_t Cout, int32_t Cin, int32_t kh, int32_t kw);
int ore_pack_conv_weight_host(const float* w_oihw_host, int32_t Cout, int32_t Cin, int32_t kh, int32_t kw,
                              float* dst_host);

/* stem_1: (x - mean)/std, zero-pad to (Hp,Wp), conv3x3 stride 2 pad 1 (3 -> Cout), FrozenBN, ReLU, in one pass.
 * img: [B][3][H][W] planar, uint8 (img_is_u8=1) or fp32 (device).  w_oihw: device [Cout][27] (= OIHW flat).
 * mean3_host/std3_host: 3 HOST floats each (passed by value to the kernel).
 * Replaces CenterNet2Detector.preprocess_image ref:fewx/modeling/fsod/fsod_cen.py:540-555 +
 * ImageList.from_tensors d2z:structures/image_list.py:69-121 + stem_1 d2z:modeling/backbone/vovnet.py:409. */
int ore_stem1_fwd(const void* img, int32_t img_is_u8, int32_t B, int32_t H, int32_t W, int32_t Hp, int32_t Wp,
                  const float* mean3_host, const float* std3_host, const float* w_oihw, const float* scale,
                  const float* shift, int32_t Cout, float* out, int32_t out_ld, int32_t out_coff, void* stream);

/* MaxPool2d(3, stride 2, ceil_mode=True) with optional per-(b,c) multiplier on the input
 * (eSE scale >= 0 commutes with max).  d2z:modeling/backbone/vovnet.py:349-350. */
int ore_maxpool3x3s2_fwd(const float* in, int32_t in_ld, int32_t in_coff, int32_t B, int32_t H, int32_t W,
                         int32_t C, const float* in_mul, float* out, int32_t out_ld, int32_t out_coff,
                         void* stream);

/* eSE gate: s[b][c] = relu6(fc(mean_hw(x))[c] + 3) / 6.   d2z:modeling/backbone/vovnet.py:238-260.
 * fc_w [C][C] (out,in), fc_b [C].  workspace >= B * (ORE_ESE_PARTS + 1) * C floats. */
#define ORE_ESE_PARTS 512
int ore_ese_gate_fwd(const float* x, int32_t ld, int32_t coff, int32_t B, int32_t HW, int32_t C,
                     const float* fc_w, const float* fc_b, float* gate, float* workspace, void* stream);

/* Same gate from partial column sums part[B][P][C] (e.g. the fused ore_conv_desc.colsum of the concat conv), one launch: every block
 * reduces the partial sums itself (same fixed order everywhere).  mean_ws: >= B*C floats, must be non-NULL (kept for callers of
 * round 2; not written since round 3). */
int ore_ese_gate_from_colsum_fwd(const float* part, int32_t P, int32_t B, int32_t HW, int32_t C,
                                 const float* fc_w, const float* fc_b, float* gate, float* mean_ws, void* stream);
/* The same for ONE image, and in the same launch the gate-scaled copy of a consumer's packed 1x1 weight: w_scaled[n][c] = w_packed[n][c] *
 * gate[c], n < w_rows (ore_pack_conv_weight layout [Cout16][C]).  The FPN lateral of the stage (d2z:modeling/backbone/fpn.py:136,
 * fed with x * gate by vovnet.py:238-260) then computes x * (g W) instead of (x * g) W on the plain conv path. */
int ore_ese_gate_scaled_weight_fwd(const float* part, int32_t P, int32_t HW, int32_t C, const float* fc_w, const float* fc_b,
                                   float* gate, float* mean_ws, const float* w_packed, int32_t w_rows, float* w_scaled, void* stream);

/* y = x * gate[b][c]  (materialises the eSE output; the fused engine folds the gate into consumers). */
int ore_scale_channels_fwd(const float* x, int32_t ld, int32_t coff, int32_t B, int32_t HW, int32_t C,
                           const float* gate, float* y, int32_t y_ld, int32_t y_coff, void* stream);

/* Query<->support depthwise correlation (ref:fewx/modeling/fsod/fsod_cen.py:454-509 eval, :229-275 train):
 *   a = relu(k11*relu(k11*q));  b = relu(dw3x1_k31(relu(dw1x3_k13(q))));  attn = a + b + q
 * q: [B][H][W] x q_ld (+q_coff), k11 [C], k13 [C][3], k31 [C][3]; attn written to out (may alias a
 * different channel slice of the same buffer as q). */
int ore_correlation_fwd(const float* q, int32_t q_ld, int32_t q_coff, int32_t B, int32_t H, int32_t W, int32_t C,
                        const float* k11, const float* k13, const float* k31,
                        float* out, int32_t out_ld, int32_t out_coff, void* stream);

/* All pyramid levels in one launch: rows level-major [level][b][y][x]; k11 [L][C], k13/k31 [L][C][3]. */
int ore_correlation_levels_fwd(const float* q, int32_t q_ld, int32_t q_coff, int32_t B, int32_t n_levels,
                               const int32_t* H, const int32_t* W, int32_t C, const float* k11, const float* k13,
                               const float* k31, float* out, int32_t out_ld, int32_t out_coff, void* stream);

/* Support kernels from a prototype [C][s][s] (NCHW, as cached in support_feature.pkl):
 * adaptive avg pools (1,1), (1,3), (3,1).  ref:fewx/modeling/fsod/fsod_cen.py:457-459. */
int ore_support_kernels_fwd(const float* proto_chw, int32_t C, int32_t s, float* k11, float* k13, float* k31,
                            void* stream);

/* GroupNorm statistics folded to a per-(b,c) affine: mul = rstd*gamma, add = beta - mean*mul.
 * ref:...centernet_head.py:72-76 (nn.GroupNorm(32, C), eps 1e-5).  Needs C | 256, groups <= 64.
 * workspace >= B * ceil(HW/64) * groups * 2 floats. */
int ore_groupnorm_affine_fwd(const float* x, int32_t ld, int32_t coff, int32_t B, int32_t HW, int32_t C,
                             int32_t groups, float eps, const float* gamma, const float* beta,
                             float* mul, float* add, float* workspace, void* stream);

/* Several pyramid levels in one launch: rows level-major, HW[l] pixels per image of level l; mul/add are
 * [level*B + b][C]; workspace >= sum_l B*ceil(HW[l]/64) * groups * 2 floats. */
int ore_groupnorm_affine_levels_fwd(const float* x, int32_t ld, int32_t coff, int32_t B, int32_t n_levels,
                                    const int32_t* HW, int32_t C, int32_t groups, float eps, const float* gamma,
                                    const float* beta, float* mul, float* add, float* workspace, void* stream);

/* ------------------------------------------------------------------ detection tail ---------- */
/* CenterNet.inference: sigmoid -> threshold -> per-level top-k -> decode -> NMS -> post-NMS top-k, all on
 * device, no host sync.  ref:fewx/modeling/fsod/fsod_rpn.py:1066-1210, ml_nms.py:4-31, d2z:layers/nms.py:10-30,
 * torchvision.ops.nms (un-vendored).  Bit-exact twin of oracle/ref_decode.c.
 * head[l]: [H*W] x head_ld floats, channels 0..3 = (l,t,r,b) after Scale+ReLU (stride units), channel 4 = hm logit.
 * Outputs: pre_* (capacity n_levels*pre_topk), keep_idx int64 (capacity same), counts[0]=n_pre, counts[1]=n_keep,
 * out_boxes/out_scores = pre_*[keep] (capacity same).  workspace: ore_detect_workspace_bytes(). */
typedef struct ore_detect_desc {
    int32_t n_levels;
    const float* head[8]; int32_t head_ld;
    int32_t H[8], W[8], stride[8];
    float score_thresh; int32_t pre_topk; float nms_thresh; int32_t post_topk;
    float* pre_boxes; float* pre_scores; int64_t* pre_loc; int32_t* pre_level;
    int64_t* keep_idx; int32_t* counts;
    float* out_boxes; float* out_scores;
    void* workspace; size_t workspace_bytes;
} ore_detect_desc;
size_t ore_detect_workspace_bytes(int32_t n_levels, int32_t pre_topk);
int ore_detect_fwd(const ore_detect_desc* d, void* stream);
/* n_images independent images (a training batch; every image its own desc, outputs and workspace, the same levels and thresholds):
 * the per-image selection / sort / IoU-mask launches of ore_detect_fwd, then the greedy scans of up to 16 images in ONE launch (block b
 * = image b) instead of 16 one-block kernels back to back.  Results are those of ore_detect_fwd image by image, bit for bit. */
int ore_detect_batch_fwd(const ore_detect_desc* d, int32_t n_images, void* stream);

/* Stand-alone NMS on n boxes (torchvision.ops.nms semantics, stable order): keep_idx int64 [n], count[0]. */
size_t ore_nms_workspace_bytes(int32_t n);
int ore_nms_fwd(const float* boxes, const float* scores, int32_t n, float thr, int64_t* keep_idx,
                int32_t* count, void* workspace, size_t workspace_bytes, void* stream);

/* NMS with the box count on the device (capacity cap): lets a producer kernel feed the NMS without a host sync.  boxes / scores hold
 * cap rows; *n_dev is clamped to cap (a larger count runs the NMS of the first cap rows). */
int ore_nms_device_n_fwd(const float* boxes, const float* scores, const int32_t* n_dev, int32_t cap, float thr,
                         int64_t* keep_idx, int32_t* count, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ second stage (ROI heads, eval) ---------- */
/* ROIPooler: FPN level assignment floor(4 + log2(sqrt(area)/224 + 1e-8)) clamped to the available levels, then
 * ROIAlignV2 (aligned=True, sampling_ratio=0) pooled x pooled.  d2z:modeling/poolers.py:22-58,190-250,
 * d2z:layers/roi_align.py:49-65 (torchvision.ops.roi_align, un-vendored, restated).
 * feat[l]: NHWC level l (ld/coff slices), scales_host[l] = 1/stride; boxes [n][4] device; the count is *n_dev if n_dev
 * is non-NULL else n_host; out [cap][pooled*pooled][C] (rows >= n are zero-filled). */
int ore_roi_align_fwd(const float* const* feat, const int32_t* ld, const int32_t* coff, const int32_t* H, const int32_t* W,
                      const float* scales_host, int32_t n_levels, int32_t min_level, int32_t C, int32_t pooled,
                      const float* boxes, const int32_t* n_dev, int32_t n_host, int32_t cap, float* out, void* stream);
/* Box predictor + fast_rcnn_inference for one image, class-agnostic box regression, one foreground class:
 * logits = cls_w h + cls_b (2), deltas = box_w h + box_b (4); score = softmax(logits)[0]; Box2BoxTransform.apply_deltas
 * (reg_weights4_host, clamp log(1000/16)); clip to (img_h, img_w); keep finite & score > score_thresh; NMS(nms_thresh);
 * keep[:topk].  ref:CenterNet2/centernet/modeling/roi_heads/custom_fast_rcnn.py:160-170, d2z:modeling/box_regression.py:77-115,
 * d2z:modeling/roi_heads/fast_rcnn.py:118-171.  det_src = index of the proposal each detection came from. */
/* The same pooling over a BATCH of images ([B][H][W][ld] per level; box i reads image box_image[i]): the 24 support crops of a
 * training step in one launch (ref:fewx/modeling/fsod/fsod_cen.py:196-200). */
int ore_roi_align_batched_fwd(const float* const* feat, const int32_t* ld, const int32_t* coff, const int32_t* H, const int32_t* W,
                              const float* scales_host, int32_t n_levels, int32_t min_level, int32_t C, int32_t pooled,
                              const float* boxes, const int32_t* box_image, int32_t n, float* out, void* stream);
/* Backward of both: dfeat[l] += scatter of dout [n][pooled*pooled][C] (fp32 atomics; the caller zeroes dfeat).
 * box_image may be NULL (one image). */
int ore_roi_align_bwd(float* const* dfeat, const int32_t* ld, const int32_t* coff, const int32_t* H, const int32_t* W,
                      const float* scales_host, int32_t n_levels, int32_t min_level, int32_t C, int32_t pooled,
                      const float* boxes, const int32_t* box_image, int32_t n, const float* dout, void* stream);
/* The same with an ORDER-INDEPENDENT sum (round 5): contributions are accumulated as 64-bit fixed-point integers (2^-40 units, integer
 * atomics) in acc[l] -- [n_images][H[l]][W[l]][C] int64, ZEROED by the caller -- and a second launch adds their value to dfeat[l]
 * (one rounding per cell).  Overlapping ROIs then give the same bits whatever order their blocks run in: the training step is
 * reproducible run to run.  |gradient sum| per cell below 2^23. */
int ore_roi_align_bwd_det(float* const* dfeat, const int32_t* ld, const int32_t* coff, const int32_t* H, const int32_t* W,
                          const float* scales_host, int32_t n_levels, int32_t min_level, int32_t C, int32_t pooled,
                          const float* boxes, const int32_t* box_image, int32_t n, const float* dout, int64_t* const* acc,
                          int32_t n_images, void* stream);

/* The same gradient as a GATHER (round 5): one block owns a 16 x 16-cell tile of one level of one image and walks the ROI list in index
 * order -- no atomics, no accumulator planes; EVERY cell of every map [n_images][H][W][ld] (channels coff .. coff + C) is written once
 * (accumulate = 0; the maps need not be zeroed) or added to (accumulate = 1).  Bit-reproducible: the additions run in ROI order.
 * box_image may be NULL only when n_images == 1.  n = 0 writes zeros.  (ref: the autograd of torchvision roi_align behind
 * d2z:modeling/poolers.py:190-250; replaces ore_roi_align_bwd_det in the training step.) */
int ore_roi_align_bwd_tiled(float* const* dfeat, const int32_t* ld, const int32_t* coff, const int32_t* H, const int32_t* W,
                            const float* scales_host, int32_t n_levels, int32_t min_level, int32_t C, int32_t pooled,
                            const float* boxes, const int32_t* box_image, int32_t n, const float* dout, int32_t n_images,
                            int32_t accumulate, void* stream);
size_t ore_roi_predict_workspace_bytes(int32_t cap);
int ore_roi_predict_fwd(const float* h, int32_t C, const float* cls_w, const float* cls_b, const float* box_w,
                        const float* box_b, const float* boxes, const int32_t* n_dev, int32_t n_host, int32_t cap,
                        const float* reg_weights4_host, float img_h, float img_w, float score_thresh, float nms_thresh,
                        int32_t topk, float* det_boxes, float* det_scores, int64_t* det_src, int32_t* det_count,
                        void* workspace, size_t workspace_bytes, void* stream);
/* The same, plus detector_postprocess (d2z:modeling/postprocessing.py:10-75, reached from
 * ref:fewx/modeling/fsod/fsod_cen.py:557-571) in the same launch when post_dev != NULL: post_dev = device {sx, sy, out_w, out_h}
 * (sx = out_w / img_w, sy = out_h / img_h as float); the detections are scaled, clipped to the output size and the empty ones
 * dropped (order kept) into fin_boxes [cap][4] / fin_scores [cap] / fin_count [1]; host_count (may be NULL) is a device-mapped
 * pinned host word that receives the same count, so the caller needs no device-to-host copy; the 64-bit word at host_count + 2 is
 * read by the kernel (system scope): when non-zero it is the device address of a caller-owned record -- boxes [cap][4] f32 | scores
 * [cap] f32 | classes [cap] i64 -- that the kernel fills as well.  cap <= 512 with post_dev. */
int ore_roi_predict_post_fwd(const float* h, int32_t C, const float* cls_w, const float* cls_b, const float* box_w,
                             const float* box_b, const float* boxes, const int32_t* n_dev, int32_t n_host, int32_t cap,
                             const float* reg_weights4_host, float img_h, float img_w, float score_thresh, float nms_thresh,
                             int32_t topk, float* det_boxes, float* det_scores, int64_t* det_src, int32_t* det_count,
                             const float* post_dev, float* fin_boxes, float* fin_scores, int32_t* fin_count,
                             int32_t* host_count, void* workspace, size_t workspace_bytes, void* stream);
/* The same with the fc1 rows still in K-split partial sums, the form the engine's second stage launches: h_parts >= 1 means h is
 * [h_parts][cap][C] raw sums and row r = ReLU(h_bias + h[0][r] + h[1][r] + ...) added in that order (h_bias [C] device, NULL = 0;
 * every slice holds cap rows, rows at and beyond the count are summed and never used); cap <= 512 only.  h_parts = 0 is
 * ore_roi_predict_post_fwd (h_bias unused). */
int ore_roi_predict_parts_fwd(const float* h, int32_t C, const float* cls_w, const float* cls_b, const float* box_w,
                              const float* box_b, const float* boxes, const int32_t* n_dev, int32_t n_host, int32_t cap,
                              const float* reg_weights4_host, float img_h, float img_w, float score_thresh, float nms_thresh,
                              int32_t topk, float* det_boxes, float* det_scores, int64_t* det_src, int32_t* det_count,
                              const float* post_dev, float* fin_boxes, float* fin_scores, int32_t* fin_count,
                              int32_t* host_count, void* workspace, size_t workspace_bytes, void* stream,
                              int32_t h_parts, const float* h_bias);

/* The cascade: CustomCascadeROIHeads with K = len(ROI_BOX_CASCADE_HEAD.IOUS) > 1 stages (ref:fewx/modeling/fsod/fsod_roi_heads.py:404-457,
 * d2z:modeling/roi_heads/cascade_rcnn.py:163-307).
 * One INTERMEDIATE eval stage in one launch.  The fc1 rows in either form of ore_roi_predict_parts_fwd (h [cap][C] finished, or h_parts >= 1
 * raw K-split sums [h_parts][cap][C] + h_bias, added in slice order, then bias, then ReLU); per row below the count: the stage's two
 * logits and four deltas (the C twin's fmaf order), the softmax foreground probability s, apply_deltas with reg_weights4_host and the
 * log(1000/16) clamp, the clip to (img_h, img_w).  next_boxes [cap][4] receives the clipped box (the next stage's proposal), score_sum
 * [cap] receives s (accumulate = 0, the first stage) or score_sum + s (1); dead [cap] is a sticky byte: set when the unclipped box or s is
 * not finite (the reference's Boxes.clip aborts there), kept once set (accumulate = 1); a dead row's next box is (0,0,0,0) and its sum 0,
 * and the last stage drops it.  Rows at and beyond the count are not written and never read by a later kernel.  Domain: that of the fused
 * tail, cap <= 512 and C <= 210; anything else is ORE_EINVAL. */
int ore_roi_cascade_refine_fwd(const float* h, int32_t C, int32_t h_parts, const float* h_bias, const float* cls_w,
                               const float* cls_b, const float* box_w, const float* box_b, const float* boxes,
                               const int32_t* n_dev, int32_t n_host, int32_t cap, const float* reg_weights4_host, float img_h,
                               float img_w, float* next_boxes, float* score_sum, uint8_t* dead, int32_t accumulate, void* stream);
/* The LAST stage: ore_roi_predict_parts_fwd with the candidate score (score_sum[r] + s_last[r]) * (float)(1.0 / n_stages) -- the fp32 sum
 * in stage order times the fp32-rounded reciprocal, as the reference averages -- and dead rows failing the filter; threshold, NMS, top-k,
 * detector_postprocess, the pinned count word and the caller's record are unchanged.  n_stages = 1 (score_sum = dead = NULL) launches what
 * ore_roi_predict_parts_fwd launches.  n_stages > 1: cap <= 512 and C <= 210 only. */
int ore_roi_predict_cascade_fwd(const float* h, int32_t C, const float* cls_w, const float* cls_b, const float* box_w,
                                const float* box_b, const float* boxes, const int32_t* n_dev, int32_t n_host, int32_t cap,
                                const float* reg_weights4_host, float img_h, float img_w, float score_thresh, float nms_thresh,
                                int32_t topk, float* det_boxes, float* det_scores, int64_t* det_src, int32_t* det_count,
                                const float* post_dev, float* fin_boxes, float* fin_scores, int32_t* fin_count,
                                int32_t* host_count, void* workspace, size_t workspace_bytes, void* stream,
                                int32_t h_parts, const float* h_bias, const float* score_sum, const uint8_t* dead,
                                int32_t n_stages);
/* The TRAINING seam between stage k - 1 and stage k for B images x R rows in one launch (no host sync, fixed shapes, no atomics; a
 * sibling of ore_sample_rois_fwd).  boxes / deltas [B][R][4] of the producing stage (deltas detached), valid [B][R] bytes, img_hw [B][2]
 * device (h, w) of every image, gtp [B][G][4] with gt_n [B] (0 <= G <= 256), reg_weights4_host of the PRODUCING stage, iou_thr of the
 * CONSUMING stage.  out_boxes = apply_deltas + clip to the row's image; out_valid = valid and finite and not empty after the clip (the
 * reference removes empty boxes in training); labels 0 (IoU with the matched ground truth >= iou_thr) / 1; gt = the matched box (max
 * IoU, first index on ties; pairwise_iou: inter > 0 ? inter / (a_gt + a_box - inter) : 0); no ground truth: label 1, gt zeros.  Rows that
 * are not valid: box (0,0,8,8), label 1, valid 0, gt zeros (the padding contract of ore_sample_rois_fwd).  out_boxes may be boxes. */
int ore_cascade_relabel_fwd(const float* boxes, const float* deltas, const uint8_t* valid, const float* img_hw, const float* gtp,
                            const int64_t* gt_n, int32_t B, int32_t R, int32_t G, const float* reg_weights4_host, float iou_thr,
                            float* out_boxes, uint8_t* out_valid, int64_t* labels, float* gt, void* stream);

/* ------------------------------------------------------------------ training targets / losses - */
/* CenterNet2 proposal-generator ground truth for only_proposal=True (class-agnostic), on device.
 * ref:fewx/modeling/fsod/fsod_rpn.py:803-901 (_get_ground_truth), :904-956 (_get_label_inds), :959-989 (assign_fpn_level /
 * assign_reg_fpn), :992-1003 (_get_reg_targets), :1038-1046 (_create_agn_heatmaps_from_dist), :1049-1065 (get_center3x3).
 * Rows are the reference's "level first" order [level][image][y][x].  gt_boxes [B][max_n][4] (x1,y1,x2,y2; max_n <= 128),
 * gt_count [B] device; soi_host [n_levels][2].  Outputs: reg_targets [rows][4] (ltrb / stride, or -1e8/stride where no object
 * owns the location), hm_targets [rows], pos_inds [<= B*max_n*n_levels] in (image, object, level) order, pos_count [1]; pos_inds and
 * pos_count may both be NULL: the positives are then left to ore_centernet_more_pos_fwd. */
int ore_centernet_targets_fwd(int32_t n_levels, const int32_t* H, const int32_t* W, const int32_t* stride, int32_t B,
                              const float* gt_boxes, const int32_t* gt_count, int32_t max_n, const float* soi_host,
                              float hm_min_overlap, float min_radius, float* reg_targets, float* hm_targets,
                              int64_t* pos_inds, int32_t* pos_count, void* stream);
/* MORE_POS positives (ref:fewx/modeling/fsod/fsod_rpn.py:664-669, :1213-1343 _add_more_pos / _get_c33_inds), the list that replaces
 * pos_inds of ore_centernet_targets_fwd when MODEL.CENTERNET.MORE_POS is set.  Levels, boxes and counts as there.  Per object, level l
 * and neighbour k = 0..8 (dx = k % 3 - 1, dy = k / 3 - 1) of the centre cell: the GIoU loss between head[row][0..3] (fp32 ltrb
 * prediction, head_ld >= 4) and the centre regression shifted by (dx, dy) stride units; 1e8 where the neighbour lies outside the map or
 * a shifted side is negative; 0 at k = 4 of a level that cares for the object and holds its centre cell.  The object keeps the candidates
 * STRICTLY below min(more_pos_topk-th smallest of its 9 * n_levels losses (NaN above every number), more_pos_thresh).
 * pos_inds [capacity B * max_n * n_levels * 9]: the kept rows in (image, object, level, k) order, duplicates kept; pos_count [1].
 * 1 <= more_pos_topk <= 9 * n_levels, more_pos_thresh > 0.  One launch on `stream`, no host sync, the same list run to run. */
int ore_centernet_more_pos_fwd(int32_t n_levels, const int32_t* H, const int32_t* W, const int32_t* stride, int32_t B,
                               const float* gt_boxes, const int32_t* gt_count, int32_t max_n, const float* soi_host,
                               const float* head, int32_t head_ld, float more_pos_thresh, int32_t more_pos_topk,
                               int64_t* pos_inds, int32_t* pos_count, void* stream);
/* Loss sums of CenterNet.losses (ref:fewx/modeling/fsod/fsod_rpn.py:702-779) with with_agn_hm + only_proposal:
 * head [rows][head_ld]: columns 0..3 = ltrb prediction (after Scale + ReLU), column 4 = agnostic heatmap logit.
 * sums4 = { sum GIoU loss over rows with max(reg_target) >= 0   (ref:CenterNet2/centernet/modeling/layers/iou_loss.py:10-63),
 *           number of such rows,
 *           sum_pos log(p)(1-p)^gamma over pos_inds, sum_all log(1-p) p^gamma (1-t)^beta [p < ignore_high_fp]
 *           (ref:CenterNet2/centernet/modeling/layers/heatmap_focal_loss.py:51-85) }
 * with p = clamp(sigmoid(logit), sigmoid_clamp, 1-sigmoid_clamp).  The caller applies the weights and the (all-reduced)
 * normalisers.  Deterministic: fixed-order two-stage reduction.  workspace: >= 4*256 floats. */
int ore_centernet_losses_fwd(const float* head, int32_t head_ld, const float* reg_targets, const float* hm_targets,
                             int32_t rows, const int64_t* pos_inds, const int32_t* pos_count, float gamma, float beta,
                             float sigmoid_clamp, float ignore_high_fp, float* sums4, float* workspace, void* stream);

/* Gradient of the three losses w.r.t. head columns 0..4 (written to dhead[rows][dhead_ld], columns 0..4; every row is written).
 * coef3 (device) = { reg_weight/reg_norm, pos_weight*alpha/num_pos_avg, neg_weight*(1-alpha)/num_pos_avg } times the upstream
 * gradient, so the normalisers (all-reduced over ranks, fsod_rpn.py:719-726,751-754) never visit the host. */
int ore_centernet_losses_bwd(const float* head, int32_t head_ld, const float* reg_targets, const float* hm_targets,
                             int32_t rows, const int64_t* pos_inds, const int32_t* pos_count, int32_t max_pos, float gamma,
                             float beta, float sigmoid_clamp, float ignore_high_fp, const float* coef3, float* dhead,
                             int32_t dhead_ld, void* stream);
/* label_and_sample_proposals for B images in one launch (d2z:modeling/roi_heads/roi_heads.py:181-295, sampling.py:10-53, matcher.py):
 * prop [B][cap][4] with prop_n [B] valid rows, gtp [B][G][4] with gt_n [B] valid rows (int64 counts on the device); candidates = proposals
 * (+ ground truth when append_gt); IoU >= iou_thr against any valid ground truth -> foreground (label 0) else background (1); R samples
 * with at most P foreground: the smallest of `keys` [B][cap (+G)] (iid uniform, the caller's) among the foreground, then among the
 * background, each in ascending key order.  boxes / gt [B][R][4], labels [B][R] int64, valid [B][R] bytes; rows beyond an image's sample
 * count are padding (box (0,0,8,8), label 1, valid 0).  cap + G <= 12800, G <= 256. */
int ore_sample_rois_fwd(const float* prop, const int64_t* prop_n, const float* gtp, const int64_t* gt_n, const float* keys, int32_t B,
                        int32_t cap, int32_t G, int32_t append_gt, int32_t R, int32_t P, float iou_thr, float* boxes, int64_t* labels,
                        float* gt, uint8_t* valid, void* stream);
/* The second stage's two losses AND their gradients in one launch (ref:CenterNet2/centernet/modeling/roi_heads/custom_fast_rcnn.py:52-81,
 * d2z:modeling/box_regression.py:41-75): rows i = b * R + j of B images x R sampled ROIs; w_i = valid_i / (n_b * B), n_b = max(#valid of
 * image b, 1); losses2[0] = sum_i w_i CE(scores_i [2], labels_i), losses2[1] = sum_i w_i [labels_i == 0] sum_k |deltas_ik -
 * get_deltas(boxes_i, gt_i; reg_weights4)_k|; dscores [B*R][2], ddeltas [B*R][4] = their gradients (scale by the upstream gradient).
 * labels int64 (0 foreground, 1 background), valid bytes, reg_weights4 host-readable.  One block, fixed summation order. */
int ore_roi_losses_fwd(const float* scores, const float* deltas, const float* boxes, const float* gt, const int64_t* labels,
                       const uint8_t* valid, int32_t B, int32_t R, const float* reg_weights4, float* losses2, float* dscores,
                       float* ddeltas, void* stream);
/* One launch of value-clip + SGD over the flat parameter bucket (row a13):
 *   g = clamp(grad_scale*grad, -clip, clip) (clip <= 0: off); g += wd*p; buf = momentum*buf + g; p -= lr*buf
 * = torch.nn.utils.clip_grad_value_ + torch.optim.SGD.step as wired by ref:fewx/solver/build.py:18-60,110-139 and
 * d2z:engine/train_loop.py:258-294.  The bucket is n_chunks x 256 floats; a chunk never straddles two parameters (each
 * parameter is padded to a multiple of 256) and chunk_lr[c]/chunk_wd[c] carry its parameter group.  The effective rate is
 * chunk_lr[c] * (*lr_scale_dev if non-NULL else lr_scale): the scheduler factor can live on device so the step is
 * hipGraph-capturable.  grad_scale = 1/world_size after a SUM all-reduce. */
int ore_sgd_step_fwd(float* params, const float* grads, float* momentum_buf, int64_t n_chunks, const float* chunk_lr,
                     const float* chunk_wd, const float* lr_scale_dev, float lr_scale, float momentum, float clip_value,
                     float grad_scale, void* stream);
/* Norm clip + SGD with or without Nesterov momentum over the same bucket (csrc/ore_optim.hip; ref:fewx/solver/build.py:19-59, :136):
 *   g^ = grad_scale*grad; norm = ||g^ over S||_p; coef = min(clip / (norm + 1e-6), 1) (a NaN stays one); g = g^*coef; g += wd*p;
 *   buf = momentum*buf + g; p -= lr*(nesterov ? g + momentum*buf : buf)
 * = torch.nn.utils.clip_grad_norm_(S, clip, p) + torch.optim.SGD(nesterov).step.  S is one parameter (the reference's per-parameter
 * clipper), or with full_model every parameter of the bucket (detectron2's later "full_model" clip type; not in the reference).
 * ore_grad_norm_geometry: the chunks one partial sum covers and the partials one pass of the per-parameter reduction takes.
 * ore_grad_norm_plan (host only): from numel[n_params], *n_chunks (sum of ceil(numel / 256)) and *n_parts; part0 [n_params + 1]
 * (first partial of every parameter, then n_parts) and part_param [part_cap >= n_parts] (the parameter of every partial) where
 * non-NULL.  Call it with NULL tables to size them.
 * ore_grad_norm_fwd: two launches (three with full_model), fixed summation order, no floating-point atomics, no host read.  Device
 * arrays: numel, chunk0 [n_params] int64 (elements; first chunk), part_param, part0 as planned (int32); workspaces partial [n_parts]
 * and acc [n_params]; outputs norm [n_params], coef [n_params] and, with full_model, total [1] (the norm over all parameters; coef
 * then holds the one coefficient n_params times).  norm_kind 2, 1, or 0 for the maximum norm.  Elements beyond numel (the padding of
 * a parameter's last chunk) are in no norm.
 * ore_sgd_step_clipnorm_fwd: the update; chunk_param [n_chunks] int32 names the parameter of a chunk.  coef NULL: the value clamp of
 * ore_sgd_step_fwd instead of the multiplication (value clipping with Nesterov).  Padding elements are not written. */
int ore_grad_norm_geometry(int32_t* chunks_per_partial, int32_t* partials_per_pass);
int ore_grad_norm_plan(const int64_t* numel, int32_t n_params, int32_t* part0, int32_t* part_param, int64_t part_cap,
                       int64_t* n_chunks, int64_t* n_parts);
int ore_grad_norm_fwd(const float* grads, int32_t n_params, const int64_t* numel, const int64_t* chunk0, const int32_t* part_param,
                      const int32_t* part0, int64_t n_parts, int32_t norm_kind, int32_t full_model, float clip_value,
                      float grad_scale, float* partial, float* acc, float* norm, float* coef, float* total, void* stream);
int ore_sgd_step_clipnorm_fwd(float* params, const float* grads, float* momentum_buf, int64_t n_chunks, const float* chunk_lr,
                              const float* chunk_wd, const int32_t* chunk_param, const int64_t* numel, const int64_t* chunk0,
                              const float* coef, const float* lr_scale_dev, float lr_scale, float momentum, float clip_value,
                              float grad_scale, int32_t nesterov, void* stream);

/* ------------------------------------------------------------------ backward of trainable layers */
/* What torch.autograd does for F.conv2d / F.linear / ReLU / FrozenBN inside `losses.backward()` (d2z:engine/train_loop.py:279;
 * layers d2z:layers/wrappers.py:48-91, d2z:layers/batch_norm.py:44-66), as explicit entry points:
 *   data gradient   = ore_conv2d_fwd over dZ with weights packed by ore_pack_conv_weight_fwd(dgrad=1)
 *                     ([Cin16][flipped tap][Cout16]; the conv then has Cin' = Cout16, Cout' = Cin, same k / pad, stride 1)
 *   weight gradient = ore_conv2d_wgrad_fwd (fp32 MFMA, rows split across blocks, slabs reduced in a fixed order)
 *   bias gradient   = ore_colsum_fwd over dZ
 *   epilogue        = ore_relu_affine_bwd: dZ = dY * (Y > 0) * scale[c]  (scale NULL = 1; in place allowed) */
int ore_pack_conv_weight_fwd(const float* w_oihw, int32_t Cout, int32_t Cin, int32_t kh, int32_t kw, int32_t dgrad,
                             float* dst, void* stream);
/* The same for up to 256 weights in one launch: jobs_dev is a DEVICE array of n_jobs descriptors, `first` the running sum of the packed
 * sizes in front of the job (Cout16 * kh * kw * Cin forward, Cin16 * kh * kw * Cout16 data gradient), `total` the sum over all jobs.
 * The array may be kept and the launch repeated (a captured training step replays it): sources and destinations are read at run time. */
typedef struct ore_pack_job {
    const float* src; float* dst;
    int32_t Cout, Cin, kh, kw, dgrad, reserved;
    int64_t first;
} ore_pack_job;
int ore_pack_conv_weights_multi_fwd(const ore_pack_job* jobs_dev, int32_t n_jobs, int64_t total, void* stream);
size_t ore_conv_wgrad_workspace_floats(int32_t rows, int32_t Cin, int32_t Cout, int32_t kh, int32_t kw);
/* dw_oihw[co][ci][ky][kx] = beta * dw_oihw + sum_{b,y,x} dz[b,y,x,co] * x[b,y+ky-pad,x+kx-pad,ci]   (stride 1, k = 2*pad+1).
 * Cin, Cout, ld, coff multiples of 4. */
int ore_conv2d_wgrad_fwd(const float* x, int32_t x_ld, int32_t x_coff, const float* dz, int32_t dz_ld, int32_t dz_coff,
                         int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t kh, int32_t kw, int32_t pad,
                         float* dw_oihw, float beta, float* workspace, size_t workspace_floats, void* stream);
/* The same launch also returns the bias gradient db[Cout] = beta_b * db + column sums of dZ (NULL = not wanted): the blocks that stage
 * the dZ rows for the matrix cores add them up on the side, so no separate reduction pass over dZ is needed
 * (torch.autograd of the bias of F.conv2d / F.linear). */
int ore_conv2d_wgrad_bias_fwd(const float* x, int32_t x_ld, int32_t x_coff, const float* dz, int32_t dz_ld, int32_t dz_coff, int32_t B,
                              int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t kh, int32_t kw, int32_t pad, float* dw_oihw,
                              float beta, float* db, float beta_b, float* workspace, size_t workspace_floats, void* stream);
/* ---- the stride-2 convolutions of the stem (MODEL.BACKBONE.FREEZE_AT: 0; csrc/ore_conv_s2grad.hip) ----
 * 3x3, stride 2, pad 1: X is [B,H,W,.], dZ is [B,Ho,Wo,.] with Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1 (H, W are always the INPUT's).
 * All three entry points are fp32 whatever the process-wide conv precision is (ore_conv_set_precision; like the depthwise units there is
 * no reduced-precision reference to pin another form to), deterministic (no float atomics, fixed summation order), enqueue on `stream`
 * without synchronising, use only the caller's workspace (capturable), treat everything outside an image as zero, read / write channel
 * slices [coff, coff + C) of rows of `ld` floats (ld, coff multiples of 4), return ORE_EINVAL for shapes they do not cover (a tensor
 * of 2 GiB or more included) and ORE_ENOMEM for a workspace that is too small, and are counted by ore_flop_counter_read.
 * Held to float64 references on an MI355X by tests/test_hip_s2grad.py; what was measured, and when: DESIGN.md 7n.
 * ore_conv2d_wgrad_s2_fwd: dw_oihw[co][ci][ky][kx] = beta * dw_oihw + sum_{b,oy,ox} dz[b,oy,ox,co] * x[b,2oy+ky-1,2ox+kx-1,ci].  Cin, Cout
 *   multiples of 4.  fp32 MFMA on a 64 x 64 (co x ci) tile; the rows B * Ho * Wo are split over blocks into slabs of the workspace
 *   (ore_conv_wgrad_s2_workspace_floats(rows, Cin, Cout) floats for the full split; less caps the split, down to one slab of
 *   Cout * 9 * Cin floats) which the reduce launch of ore_conv2d_wgrad_fwd adds in a fixed order.  beta = 0 does not read dw_oihw.
 * ore_conv2d_dgrad_s2_fwd: dx[b,y,x,ci] = sum_{ky,kx,co} dz[b,(y+1-ky)/2,(x+1-kx)/2,co] * w_oihw[co][ci][ky][kx] over the taps whose two
 *   quotients are integers inside the map.  Cin, Cout multiples of 4.  The pixels of each (y mod 2, x mod 2) class are one GEMM with
 *   K = taps x Cout, taps = 1 / 2 / 2 / 4; one launch for the four classes, after a small launch that packs the weights as
 *   [tap][Cout][Cin] into the workspace (ore_conv_dgrad_s2_workspace_floats(Cin, Cout) = 9 * Cin * Cout floats).  Every element of the
 *   dx slice is written (no accumulation).
 * ore_stem1_wgrad_fwd: dw[co][27] = beta * dw + the weight gradient of stem_1 (ore_stem1_fwd) from the raw planar image [B][3][H][W]
 *   (uint8 or fp32): (x - mean) / std and the zero padding to (Hp, Wp) are formed on the fly, as in the forward; dz is [B,Hp/2,Wp/2,.].
 *   Hp, Wp even, Cout a multiple of 16; mean3_host / std3_host are HOST floats.  Workspace: ore_stem1_wgrad_workspace_floats(rows, Cout),
 *   rows = B * Hp/2 * Wp/2 (less caps the split).  stem_1 has no data gradient. */
size_t ore_conv_wgrad_s2_workspace_floats(int32_t rows, int32_t Cin, int32_t Cout);
int ore_conv2d_wgrad_s2_fwd(const float* x, int32_t x_ld, int32_t x_coff, const float* dz, int32_t dz_ld, int32_t dz_coff, int32_t B,
                            int32_t H, int32_t W, int32_t Cin, int32_t Cout, float* dw_oihw, float beta, float* workspace,
                            size_t workspace_floats, void* stream);
size_t ore_conv_dgrad_s2_workspace_floats(int32_t Cin, int32_t Cout);
int ore_conv2d_dgrad_s2_fwd(const float* dz, int32_t dz_ld, int32_t dz_coff, const float* w_oihw, int32_t B, int32_t H, int32_t W,
                            int32_t Cin, int32_t Cout, float* dx, int32_t dx_ld, int32_t dx_coff, float* workspace,
                            size_t workspace_floats, void* stream);
size_t ore_stem1_wgrad_workspace_floats(int32_t rows, int32_t Cout);
int ore_stem1_wgrad_fwd(const void* img, int32_t img_is_u8, int32_t B, int32_t H, int32_t W, int32_t Hp, int32_t Wp,
                        const float* mean3_host, const float* std3_host, const float* dz, int32_t dz_ld, int32_t dz_coff,
                        int32_t Cout, float* dw, float beta, float* workspace, size_t workspace_floats, void* stream);
int ore_relu_affine_bwd(const float* dy, int32_t dy_ld, int32_t dy_coff, const float* y, int32_t y_ld, int32_t y_coff,
                        const float* scale, int64_t rows, int32_t C, float* dz, int32_t dz_ld, int32_t dz_coff, void* stream);
/* out[c] = beta * out[c] + sum_rows x[row][coff + c]; workspace >= ceil(rows/64) * C floats. */
int ore_colsum_fwd(const float* x, int32_t ld, int32_t coff, int64_t rows, int32_t C, float beta, float* out,
                   float* workspace, size_t workspace_floats, void* stream);
/* Segmented form: the rows are `segments` equal runs (the images of a batch); out [segments][C].  A segment's sums are bitwise those
 * of ore_colsum_fwd on that run alone (chunking restarts per segment).  workspace >= segments * ceil(rows_per_segment/256) * C. */
int ore_colsum_segments_fwd(const float* x, int32_t ld, int32_t coff, int32_t segments, int64_t rows_per_segment, int32_t C,
                            float beta, float* out, float* workspace, size_t workspace_floats, void* stream);

/* ------------------------------------------------------------------ depthwise-separable units (the *-dw-* VoVNet bodies) */
/* d2z:modeling/backbone/vovnet.py:110-130 `dw_conv3x3`: Conv2d(C, C, 3, stride, 1, groups=C, bias=False) -> Conv2d(C, C, 1, bias=False) ->
 * FrozenBN -> ReLU, nothing between the two convs.  All three entry points are fp32 whatever the process-wide conv precision is (the
 * reference has no reduced-precision path to pin a bf16 form to), read channels [coff, coff + C) of NHWC rows of `ld` floats (the
 * concat-slice convention of ore_conv_desc; ld and coff multiples of 4), treat everything outside an image as zero -- the halo of a
 * border row never comes from the neighbouring image of the batch or from the channels beside the slice -- and enqueue on `stream`
 * without synchronising.  w_dw is the Conv2d weight [C][1][3][3] as it is; pad is 1; Ho = (H - 1) / stride + 1.
 *
 * ore_dwpw_fwd: the whole unit in ONE launch (k_dwpw): out[b,oy,ox,out_coff + n] = relu(scale[n] * sum_k w_pw[n][k] * dw(in)[b,oy,ox,k]
 *   + shift[n]); the depthwise result is formed per chunk of up to 64 channels in LDS and fed to v_mfma_f32_16x16x4_f32, it never goes
 *   to memory.
 *   C % 16 == 0, C <= 1024, stride 1 or 2; w_pw [C][C] row-major = ore_pack_conv_weight_host of the 1x1 weight; scale / shift [C] or
 *   NULL (1 / 0).  Input and output may be slices of the same buffer when they do not overlap (the OSA chain).
 *   Counted by ore_flop_counter_read as ore_dwpw_flops(rows, C) = 2 * rows * C * (9 + C), rows = B * Ho * Wo.
 * ore_dw3x3_fwd: the depthwise conv alone (k_dw3x3), C % 4 == 0.  dgrad = 1: taps mirrored, i.e. the data gradient dX of a stride-1
 *   unit from dT -- stride 2 is refused there with ORE_EINVAL: the only stride-2 unit of the bodies, stem_3, is frozen at every
 *   FREEZE_AT the reference trains with.  accumulate = 1: out += result (the gradient of a concat slice that already holds a sum).
 * ore_dw3x3_wgrad_fwd: dw[c][ky][kx] = beta * dw + sum_{b,y,x} x[b,y+ky-1,x+kx-1,c] * dt[b,y,x,c] (stride 1).  Deterministic, no float
 *   atomics: the pixels are cut into parts of 256 whatever the device, each part summed in a fixed order into the workspace
 *   (ore_dw3x3_wgrad_workspace_floats(B * H * W, C) floats, the caller's), then the parts in order by a second launch.  beta = 0
 *   does not read dw. */
/* Base pointers of in / out (and w_pw, scale, shift of ore_dwpw_fwd) must be 16-byte aligned; an input and an output slice that share a
 * buffer must lie side by side in every row (same ld) -- anything else returns ORE_EINVAL.
 * ore_dwpw_planned_fwd: ore_dwpw_fwd, except where ore_dwpw_prefers_composition(rows, C, stride) -- stride 1 and rows * C >= 2^22, the one
 *   regime where the fused launch measured slower (stem_2 at 640x640) -- where it runs k_dw3x3 into `scratch` (the caller's, >= rows * C
 *   floats, else ORE_ENOMEM) and the 1x1 conv launch in fp32.  The engine and orehip.dwpw go through it.  The unfused path sets the
 *   process-wide conv precision (ore_conv_set_precision) to fp32 around that launch and restores it: like every call that depends on
 *   that mode, it must not run concurrently with another host thread that sets or relies on a different mode. */
int32_t ore_dwpw_prefers_composition(int64_t rows, int32_t C, int32_t stride);
int ore_dwpw_planned_fwd(const float* in, int32_t ld_in, int32_t in_coff, int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride,
                         const float* w_dw, const float* w_pw, const float* scale, const float* shift, float* out, int32_t ld_out,
                         int32_t out_coff, float* scratch, size_t scratch_floats, void* stream);
double ore_dwpw_flops(int64_t rows, int32_t C);
int ore_dwpw_fwd(const float* in, int32_t ld_in, int32_t in_coff, int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride,
                 const float* w_dw, const float* w_pw, const float* scale, const float* shift, float* out, int32_t ld_out,
                 int32_t out_coff, void* stream);
int ore_dw3x3_fwd(const float* in, int32_t ld_in, int32_t in_coff, int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride,
                  const float* w_dw, int32_t dgrad, float* out, int32_t ld_out, int32_t out_coff, int32_t accumulate, void* stream);
size_t ore_dw3x3_wgrad_workspace_floats(int64_t rows, int32_t C);
int ore_dw3x3_wgrad_fwd(const float* x, int32_t x_ld, int32_t x_coff, const float* dt, int32_t dt_ld, int32_t dt_coff, int32_t B, int32_t H,
                        int32_t W, int32_t C, float* dw, float beta, float* workspace, size_t workspace_floats, void* stream);

/* Depthwise support correlation with gradients (ref:fewx/modeling/fsod/fsod_cen.py:229-245, training branch).
 * k_per_image = 0: one support kernel set k11 [C], k13 / k31 [C][3] for all B images; 1: every image its own ([B][C], [B][C][3]) --
 * a training batch, where each query image comes with its own support crops.
 * fwd: cat2c [rows][2C] = [attn | q] (the input of conv3), t_save / u_save [rows][C] kept for the backward.
 * bwd: dcat2c [rows][2C] -> dq [rows][C] (both halves) and dk_7c [S][7C] = (dk11 [C] | dk13 tap-major [3][C] | dk31 tap-major [3][C])
 * with S = B if k_per_image else 1.  workspace >= rows*C*8 + S*ceil(rows/S/256)*7*C floats.  Deterministic (per-row products +
 * ordered, per-image column sums). */
int ore_correlation_train_fwd(const float* q, int32_t q_ld, int32_t q_coff, int32_t B, int32_t H, int32_t W, int32_t C,
                              const float* k11, const float* k13, const float* k31, int32_t k_per_image, float* cat2c,
                              float* t_save, float* u_save, void* stream);
int ore_correlation_train_bwd(const float* q, int32_t q_ld, int32_t q_coff, int32_t B, int32_t H, int32_t W, int32_t C,
                              const float* k11, const float* k13, const float* k31, int32_t k_per_image, const float* dcat2c,
                              const float* t_save, const float* u_save, float* dq, float* dk_7c, float* workspace,
                              size_t workspace_floats, void* stream);

/* Small HBM-bound training ops (NHWC fp32, channels multiple of 4), all deterministic:
 *   GroupNorm(+ReLU) with gradients (head tower, ref:CenterNet2/centernet/modeling/dense_heads/centernet_head.py:86-100; torch
 *     F.group_norm backward) for `images` images of rows_per_image rows each (statistics are per image).  rstd_c / shift_c
 *     [images][C] = per-channel rstd and -mean*rstd of the channel's group: what ore_groupnorm_affine_fwd returns for gamma = 1,
 *     beta = 0.  ore_groupnorm_bwd writes dx [rows][C] and per image (dbeta | dgamma) [images][2C] (the parameter gradient is their sum
 *     over the images); workspace >= rows*2*C + images*ceil(rows_per_image/256)*2*C floats.
 *   eSE (d2z:modeling/backbone/vovnet.py:238-260) pieces: ore_prod_colsum_fwd = per-image column sums of p*q (q NULL: of p) times
 *     `scale` -> [B][C] (average pool, and d gate = sum_hw dy*x); ore_scale_add_channels_fwd = x*s[b][c] + v[b][c].
 *   ore_maxpool3x3s2_bwd: MaxPool2d(3, 2, ceil_mode=True) backward, first maximum in scan order owns the window (ATen).
 *   ore_sumpool2x2_fwd: backward of the FPN's nearest-2x top-down add (d2z:modeling/backbone/fpn.py:136-141). */
int ore_groupnorm_apply_fwd(const float* x, int32_t ld, int32_t coff, int32_t images, int64_t rows_per_image, int32_t C,
                            const float* rstd_c, const float* shift_c, const float* gamma, const float* beta, int32_t relu, float* y,
                            void* stream);
int ore_groupnorm_bwd(const float* dy, const float* y, const float* x, int32_t ld, int32_t coff, int32_t images,
                      int64_t rows_per_image, int32_t C, int32_t groups, const float* rstd_c, const float* shift_c, const float* gamma,
                      int32_t relu, float* dx, float* dbeta_dgamma_2c, float* workspace, size_t workspace_floats, void* stream);
int ore_prod_colsum_fwd(const float* p, const float* q, int32_t B, int32_t rows, int32_t C, float scale, float* out_bc,
                        float* workspace, size_t workspace_floats, void* stream);
int ore_scale_add_channels_fwd(const float* x, const float* scale_bc, const float* add_bc, int32_t B, int32_t rows, int32_t C,
                               float* out, void* stream);
/* SM_Block glue (ref:fewx/modeling/fsod/fsod_cen.py:584-630, training side).
 * ore_granule_transpose_fwd: for every (i1 < nb1, i2 < nb2) the [A][Bc] matrix of S-float granules at in + i1*in_b1 + i2*in_b2 (row stride
 *   in_rs, a row = Bc*S contiguous floats) is written transposed, [Bc][A] granules, at out + i1*out_b1 + i2*out_b2 (row stride out_rs, a
 *   row = A*S contiguous floats).  All strides in floats, multiples of 4; in != out.  This is x.reshape(B,H,W,seg,S).permute(0,3,2,1,4)
 *   / .permute(0,3,1,2,4) and their inverses as one coalesced pass; accumulate != 0: out += (the second of two gradients of one map).
 * ore_combine2_fwd: y = w * a0[b][c] + h * a1[b][c];  ore_combine2_bwd: dw = dy * a0 + v, dh = dy * a1 + v (v [B][C] optional). */
/* F.adaptive_avg_pool2d on NHWC maps, forward and (gather-form, deterministic) backward: x [B][H][W][C] -> y [B][OH][OW][C]
 * (ref:fewx/modeling/fsod/fsod_cen.py:214-231: the support maps pooled to 32 / 16 / 8 and the 1x1 / 1x3 / 3x1 support kernels).
 * ore_group_mean_fwd: y[g][m] = mean over n < N of x[g*N + n][m] (the prototype = mean over an image's shots, :228), _bwd its gradient. */
int ore_adaptive_avgpool_nhwc_fwd(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW, float* y, void* stream);
int ore_adaptive_avgpool_nhwc_bwd(const float* dy, int32_t B, int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW, float* dx, void* stream);
int ore_group_mean_fwd(const float* x, int32_t G, int32_t N, int64_t M, float* y, void* stream);
int ore_group_mean_bwd(const float* dy, int32_t G, int32_t N, int64_t M, float* dx, void* stream);
int ore_granule_transpose_fwd(const float* in, float* out, int32_t nb1, int32_t nb2, int32_t A, int32_t Bc, int32_t S, int64_t in_b1,
                              int64_t in_b2, int64_t in_rs, int64_t out_b1, int64_t out_b2, int64_t out_rs, int32_t accumulate, void* stream);
int ore_combine2_fwd(const float* w, const float* h, const float* a0_bc, const float* a1_bc, int32_t B, int32_t rows, int32_t C, float* y,
                     void* stream);
int ore_combine2_bwd(const float* dy, const float* a0_bc, const float* a1_bc, const float* add_bc, int32_t B, int32_t rows, int32_t C,
                     float* dw, float* dh, void* stream);
int ore_maxpool3x3s2_bwd(const float* x, const float* dy, int32_t B, int32_t H, int32_t W, int32_t C, float* dx, void* stream);
int ore_sumpool2x2_fwd(const float* in, int32_t ld, int32_t B, int32_t H, int32_t W, int32_t C, float* out, void* stream);

/* ------------------------------------------------------------------ engine ------------------- */
/* Whole eval hot path for one model instance: owns packed weights and all
 * intermediate buffers, replays a captured hipGraph per image.
 * Replaces CenterNet2Detector.inference up to the proposals handed to the ROI heads
 * (ref:fewx/modeling/fsod/fsod_cen.py:418-527) and build_fcos_vovnet_fpn_backbone(...).forward. */
typedef struct ore_engine ore_engine;

typedef struct ore_model_cfg {
    int32_t stem_ch[3];
    int32_t stage_conv_ch[4], stage_out_ch[4];
    int32_t layers_per_block;
    int32_t fpn_ch;               /* 128 */
    int32_t strides[3];           /* 8,16,32 */
    float pixel_mean[3], pixel_std[3];
    float score_thresh; int32_t pre_topk; float nms_thresh; int32_t post_topk;
    int32_t max_batch, max_h, max_w;  /* padded input size the buffers are allocated for */
} ore_model_cfg;

int ore_engine_create(const ore_model_cfg* cfg, int32_t device, ore_engine** out);
void ore_engine_destroy(ore_engine* e);
/* Host fp32 tensor by its reference state_dict name, e.g.
 * "backbone.bottom_up.stem.stem_1/conv.weight".  All tensors must be set before the first forward. */
int ore_engine_set_tensor(ore_engine* e, const char* name, const float* data_host, const int64_t* shape, int32_t ndim);
/* Cached support prototypes [128][s][s] for level 3/4/5 (support_feature.pkl 'p3','p4','p5'), host. */
int ore_engine_set_support(ore_engine* e, int32_t level, const float* proto_chw_host, int32_t C, int32_t s);
int ore_engine_finalize(ore_engine* e);   /* fold BN, pack weights, upload */
/* The depthwise bodies (V-19-slim-dw-eSE, V-19-dw-eSE; d2z:modeling/backbone/vovnet.py:28-48): call with on = 1 BEFORE ore_engine_finalize
 * (a setter, so that ore_model_cfg keeps its layout).  finalize then needs the reference's depthwise names -- stem.stem_2/dw_conv3x3,
 * /pw_conv1x1, /pw_norm; stageK.OSAK_1.layers.i.OSAK_1_i/dw_conv3x3 ...; stageK.OSAK_1.conv_reduction.OSAK_1_reduction_0/conv, /norm where
 * a stage's input width differs from stage_conv_ch -- builds stem_2 / stem_3 and every stage layer as one ore_dwpw_fwd launch, and holds
 * one extra [rows][stage_conv_ch] buffer per stage for the reduction's output (it feeds layer 0 and is not part of the concat).
 * ore_engine_last_flops counts a unit as ore_dwpw_flops.  The units are fp32 in every conv precision; an engine created in the bf16
 * STORAGE mode refuses with ORE_EINVAL (here and in finalize). */
int ore_engine_set_depthwise(ore_engine* e, int32_t on);
/* The deep bodies (V-39-eSE, V-57-eSE, V-99-eSE; d2z:modeling/backbone/vovnet.py:50-96): blocks[s] OSA blocks in stage s + 2, each 1..16;
 * call BEFORE ore_engine_finalize (a setter, so that ore_model_cfg keeps its layout).  All ones is the default and leaves every pass as
 * it was, launch for launch.  finalize then needs, for the identity blocks j = 2..blocks[s], the reference's names
 * stageK.OSAK_j.layers.i.OSAK_j_i/conv|norm, stageK.OSAK_j.concat.OSAK_j_concat/conv|norm and stageK.OSAK_j.ese.fc.{weight,bias}
 * (layer 0 of such a block has Cin = stage_out_ch, its concat width is stage_out_ch + layers_per_block * stage_conv_ch).  The tail of
 * an identity block is ONE launch at one image per pass (ore_ese_gate_residual_fwd), two at more (ore_ese_gate_fwd +
 * ore_scale_residual_fwd).  Stage-output contract: buffer "stageK" times buffer "gateK" is the stage's output; a stage that ends in an
 * identity block holds the full output in "stageK" and ones in "gateK" (its FPN lateral runs on the unscaled weights, the max-pool
 * behind it without a multiplier), a one-block stage of the same engine keeps its folds.  Refused with ORE_EINVAL and the reason: a
 * depthwise engine (the reference has no deep depthwise body), an engine created in the bf16 STORAGE mode, a count outside 1..16. */
int ore_engine_set_blocks(ore_engine* e, const int32_t blocks[4]);
/* Optional second stage (CustomCascadeROIHeads, eval) inside the same forward/graph; call after finalize.  W_host [fc_dim]
 * [pooled*pooled*fpn_ch] (k ordered [pos][channel]) and b_host [fc_dim] are the pre-composed DSA-mix + flatten + fc1 chain
 * (ref:fewx/modeling/fsod/fsod_roi_heads.py:500-520; orehip.compose_roi_head builds them from the state_dict and the cached
 * rcnn_8 support features); cls_* [2][fc_dim],[2]; box_* [4][fc_dim],[4].  Results: buffers "det_boxes","det_scores",
 * "det_src","det_count".  At most 320 proposals enter the second stage (post-NMS top-256 plus up to 64 score ties). */
int ore_engine_set_roi_head(ore_engine* e, const float* W_host, const float* b_host, int32_t fc_dim, int32_t pooled,
                            const float* cls_w_host, const float* cls_b_host, const float* box_w_host, const float* box_b_host,
                            const float* reg_weights4_host, float score_thresh, float nms_thresh, int32_t topk);
/* The same for a cascade of n_stages = len(ROI_BOX_CASCADE_HEAD.IOUS) stages (1 .. ORE_MAX_CASCADE): host arrays of n_stages
 * host pointers -- W_host[k] / b_host[k] the composed chain with box_head[k].fc1 (orehip.compose_roi_head(stage=k)), cls_* / box_* of
 * box_predictor[k] -- and reg_weights4_host [n_stages][4].  The second stage then loops: ROIAlign(boxes_k) -> the fc1 GEMM (same K-split) ->
 * ore_roi_cascade_refine_fwd for k < n_stages - 1, ore_roi_predict_cascade_fwd for the last; the one-image pass, the folded batch pass
 * and the N-way class slots all run it (a class slot needs ore_engine_set_roi_support_slot_stage for every stage; a pass with one
 * missing is refused with the stage count in the message).  n_stages = 1 IS ore_engine_set_roi_head: the same launches.  The GEMMs
 * stay fp32 in the bf16 modes.  A later ore_engine_set_roi_head returns the engine to one stage. */
#define ORE_MAX_CASCADE 4
int ore_engine_set_roi_cascade(ore_engine* e, int32_t n_stages, const float* const* W_host, const float* const* b_host,
                               int32_t fc_dim, int32_t pooled, const float* const* cls_w_host, const float* const* cls_b_host,
                               const float* const* box_w_host, const float* const* box_b_host, const float* reg_weights4_host,
                               float score_thresh, float nms_thresh, int32_t topk);

/* Backbone+FPN only: img [B][3][H][W] (u8 or f32, device) -> p3,p4,p5 NHWC device pointers owned by the engine. */
int ore_engine_backbone_fwd(ore_engine* e, const void* img, int32_t img_is_u8, int32_t B, int32_t H, int32_t W,
                            void* stream);
/* Whole eval path for B=1: ... -> proposals.  use_graph=1 replays a captured hipGraph (captured on first use
 * for this (H,W)).  Results stay on device; query with ore_engine_buffer(). */
int ore_engine_eval_fwd(ore_engine* e, const void* img, int32_t img_is_u8, int32_t H, int32_t W, int32_t use_graph,
                        void* stream);
/* The reference's eval call for ONE image, end to end (ref:fewx/modeling/fsod/fsod_cen.py:417-452 `inference` + :557-571
 * `_postprocess` -> d2z:modeling/postprocessing.py:10-75): copies the image in (device OR host pointer), replays the graph of both
 * stages with detector_postprocess in its last kernel (scale to out_h x out_w, clip, drop empty boxes), which also writes the
 * detection count to a device-mapped pinned host word; the call returns when that word has been written (bounded poll, then an
 * ordinary stream synchronise): ONE host wait per image.  *n_det detections are then in the engine buffers "final_boxes" [n,4] /
 * "final_scores" [n] (valid until the next forward of this engine) and, when out_record != NULL, in the caller's own device memory:
 * out_record = ORE_DET_RECORD_BYTES bytes laid out [320][4] f32 boxes | [320] f32 scores | [320] int64 classes (all 0: one
 * foreground class), written by the graph's last kernel (the address travels in a pinned word next to the count); whatever the
 * caller queues on `stream` afterwards is ordered behind that kernel.  Needs ore_engine_set_roi_head. */
#define ORE_DET_RECORD_ROWS 320
#define ORE_DET_RECORD_BYTES (ORE_DET_RECORD_ROWS * 28)
/* ORE_DET_RECORD_ROWS as the library was built (bindings size the record from this, not from a literal). */
int32_t ore_det_record_rows(void);
/* 1 when the named activation buffer of this engine is a bf16 tensor (engines created under ORE_CONV_BF16S), else 0 */
int32_t ore_engine_buffer_is_bf16(ore_engine* e, const char* name);
/* bf16-tensor forms of the small kernels between the convs of an ORE_CONV_BF16S engine (same arguments as their fp32 namesakes, ld /
 * coff in ELEMENTS; reductions, gates and statistics stay fp32):
 *   stem_1 writing bf16; ceil-mode max-pool bf16 -> bf16 (eSE gate folded, rounded once); depthwise correlation bf16 -> bf16;
 *   GroupNorm statistics from a bf16 tensor; y = act(x * mul + add) bf16 -> bf16 with the folded per-(image, channel) affine;
 *   eSE gate + the gate-scaled lateral weight written as bf16 (source weight fp32, C % 32 == 0); ROIAlign over bf16 feature maps
 *   (fp32 output). */
int ore_stem1_bf16_fwd(const void* img, int32_t img_is_u8, int32_t B, int32_t H, int32_t W, int32_t Hp, int32_t Wp, const float* mean3,
                       const float* std3, const float* w_oihw, const float* scale, const float* shift, int32_t Cout, uint16_t* out,
                       int32_t out_ld, int32_t out_coff, void* stream);
int ore_ese_gate_bf16_fwd(const uint16_t* x, int32_t ld, int32_t coff, int32_t B, int32_t HW, int32_t C, const float* fc_w,
                          const float* fc_b, float* gate, float* workspace, void* stream);   /* ore_ese_gate_fwd over a bf16 map */
int ore_maxpool3x3s2_bf16_fwd(const uint16_t* in, int32_t in_ld, int32_t in_coff, int32_t B, int32_t H, int32_t W, int32_t C,
                              const float* in_mul, uint16_t* out, int32_t out_ld, int32_t out_coff, void* stream);
int ore_correlation_levels_bf16_fwd(const uint16_t* q, int32_t q_ld, int32_t q_coff, int32_t B, int32_t n_levels, const int32_t* H,
                                    const int32_t* W, int32_t C, const float* k11, const float* k13, const float* k31, uint16_t* out,
                                    int32_t out_ld, int32_t out_coff, void* stream);
int ore_groupnorm_affine_levels_bf16_fwd(const uint16_t* x, int32_t ld, int32_t coff, int32_t B, int32_t n_levels, const int32_t* HW,
                                         int32_t C, int32_t groups, float eps, const float* gamma, const float* beta, float* mul,
                                         float* add, float* workspace, void* stream);
int ore_groupnorm_apply_bf16_fwd(const uint16_t* x, int32_t ld, int32_t coff, int32_t images, int64_t rows_per_image, int32_t C,
                                 const float* mul_c, const float* add_c, int32_t relu, uint16_t* y, void* stream);
/* CenterNet head, last step, as ONE VALU kernel over all pyramid levels (level-major rows): t = relu(tower * gn_mul + gn_add) with the
 * folded GroupNorm affine of ore_groupnorm_affine_levels_*_fwd ([level*B + image][128]); (l,t,r,b | hm) = conv3x3_{128->5}(t) with the
 * packed [16][9][128] weight, y = conv * scale[level][o] + shift[level][o], ReLU on the four box outputs; out rows [.., out_ld >= 5] fp32.
 * Replaces ref:CenterNet2/centernet/modeling/dense_heads/centernet_head.py:146-159 (GN + ReLU + bbox_pred / agn_hm + Scale + ReLU).
 * The tower may be fp32 or bf16 (bf16-storage engines). */
int ore_head_pred_fwd(const float* tower, int32_t ld, int32_t B, int32_t n_levels, const int32_t* H, const int32_t* W, const float* gn_mul,
                      const float* gn_add, const float* w_packed16, const float* scale, const float* shift, int32_t ep_stride, float* out,
                      int32_t out_ld, void* stream);
int ore_head_pred_bf16_fwd(const uint16_t* tower, int32_t ld, int32_t B, int32_t n_levels, const int32_t* H, const int32_t* W,
                           const float* gn_mul, const float* gn_add, const float* w_packed16, const float* scale, const float* shift,
                           int32_t ep_stride, float* out, int32_t out_ld, void* stream);
/* GroupNorm statistics + ore_head_pred in TWO launches: the blocks of the head kernel fold the chunk statistics of their own (level,
 * image) themselves (groups must divide 128; workspace as ore_groupnorm_affine_levels_fwd). */
int ore_head_pred_gn_fwd(const float* tower, int32_t ld, int32_t B, int32_t n_levels, const int32_t* H, const int32_t* W, int32_t groups,
                         float eps, const float* gamma, const float* beta, const float* w_packed16, const float* scale, const float* shift,
                         int32_t ep_stride, float* out, int32_t out_ld, float* workspace, void* stream);
int ore_head_pred_gn_bf16_fwd(const uint16_t* tower, int32_t ld, int32_t B, int32_t n_levels, const int32_t* H, const int32_t* W,
                              int32_t groups, float eps, const float* gamma, const float* beta, const float* w_packed16, const float* scale,
                              const float* shift, int32_t ep_stride, float* out, int32_t out_ld, float* workspace, void* stream);
int ore_groupnorm_apply_levels_bf16_fwd(const uint16_t* x, int32_t ld, int32_t coff, int32_t B, int32_t n_levels, const int32_t* HW, int32_t C,
                                        const float* mul_c, const float* add_c, int32_t relu, uint16_t* y, void* stream);
int ore_ese_gate_scaled_weight_bf16_fwd(const float* part, int32_t P, int32_t HW, int32_t C, const float* fc_w, const float* fc_b,
                                        float* gate, float* mean_ws, const float* w_packed_f32, int32_t w_rows, uint16_t* w_scaled_bf16,
                                        void* stream);
/* bs = 1 engine, a stage that is followed by the max-pool: gate (as ore_ese_gate_from_colsum_fwd for one image), optionally the
 * gate-scaled copy of a consumer's packed 1x1 weight (as ore_ese_gate_scaled_weight_fwd; w_packed / w_scaled NULL = none), and
 * out[oy][ox][out_coff + c] = max over the 3x3 / stride-2 ceil-mode window of x[..][x_coff + c] * gate[c], all in ONE launch.
 * Replaces eSE + the next stage's MaxPool2d(3, 2, ceil_mode=True) of d2z:modeling/backbone/vovnet.py:238-260,359-361. */
int ore_ese_gate_pool_fwd(const float* part, int32_t P, int32_t HW, int32_t C, const float* fc_w, const float* fc_b, float* gate,
                          const float* w_packed, int32_t w_rows, float* w_scaled, const float* x, int32_t x_ld, int32_t x_coff,
                          int32_t H, int32_t W, float* out, int32_t out_ld, int32_t out_coff, void* stream);
int ore_ese_gate_pool_bf16_fwd(const float* part, int32_t P, int32_t HW, int32_t C, const float* fc_w, const float* fc_b, float* gate,
                               const float* w_packed_f32, int32_t w_rows, uint16_t* w_scaled_bf16, const uint16_t* x, int32_t x_ld,
                               int32_t x_coff, int32_t H, int32_t W, uint16_t* out, int32_t out_ld, int32_t out_coff, void* stream);
/* The tail of an OSA identity block (d2z:modeling/backbone/vovnet.py:310-332: eSE product + `xt += identity_feat`) for ONE image in
 * ONE launch: gate[C] from the concat conv's fused column sums part[P][C] (the arithmetic of ore_ese_gate_from_colsum_fwd for one
 * image), and out[r][out_coff + c] = y[r][y_coff + c] * gate[c] + x[r][x_coff + c] for all HW rows (one rounding: fmaf).  y is the concat
 * conv's output, x the block's identity (the first C channels of its own concat buffer), out the first slice of the next block's
 * concat buffer or the stage's output map.  x == NULL: out = y * gate (the tail of block 1 in front of an identity block).  C % 4 == 0,
 * C <= 4096; every ld / coff a multiple of 4 with coff + C <= ld; y, x, out, part, gate 16-byte aligned; out must not overlap y or x
 * (side by side in the rows of one buffer is fine).  No atomics: the bits do not depend on scheduling. */
int ore_ese_gate_residual_fwd(const float* part, int32_t P, int32_t HW, int32_t C, const float* fc_w, const float* fc_b, float* gate,
                              const float* y, int32_t y_ld, int32_t y_coff, const float* x, int32_t x_ld, int32_t x_coff, float* out,
                              int32_t out_ld, int32_t out_coff, void* stream);
/* The same tail for B images of rows_per_image rows with the gates given, gate_bc[B][C] (ore_ese_gate_fwd): the same arithmetic element
 * by element, the same argument rules. */
int ore_scale_residual_fwd(const float* y, int32_t y_ld, int32_t y_coff, const float* gate_bc, const float* x, int32_t x_ld, int32_t x_coff,
                           int32_t B, int32_t rows_per_image, int32_t C, float* out, int32_t out_ld, int32_t out_coff, void* stream);
int ore_roi_align_bf16_fwd(const uint16_t* const* feat, const int32_t* ld, const int32_t* coff, const int32_t* H, const int32_t* W,
                           const float* scales_host, int32_t n_levels, int32_t min_level, int32_t C, int32_t pooled, const float* boxes,
                           const int32_t* n_dev, int32_t n_host, int32_t cap, float* out, void* stream);
int ore_engine_detect_fwd(ore_engine* e, const void* img, int32_t img_is_u8, int32_t H, int32_t W, int32_t out_h, int32_t out_w,
                          void* out_record, void* stream, int32_t* n_det);
/* ore_engine_detect_fwd in two halves: _begin enqueues the pass (and returns at once), _end waits for its detection count.  What the
 * host does in between runs in the shadow of the device pass: the module-level forward uses it to validate its cached engine against
 * the parameters' version counters AFTER launching on it (a stale engine is the rare case: its result is dropped and the pass
 * repeated), which takes that check out of the per-image critical path of the reference's protocol
 * (d2z:evaluation/evaluator.py:138-161).  One pass may be pending per engine: a second _begin before _end, and _end without _begin, are ORE_EINVAL. */
int ore_engine_detect_begin(ore_engine* e, const void* img, int32_t img_is_u8, int32_t H, int32_t W, int32_t out_h, int32_t out_w,
                            void* out_record, void* stream);
int ore_engine_detect_end(ore_engine* e, void* stream, int32_t* n_det);
/* The same for B images of one size in ONE pass (B <= cfg.max_batch; img [B][3][H][W] contiguous): the dense stages -- backbone, FPN,
 * correlation, conv3, head -- run batched (a CU fetches every layer's weights once for B images instead of once per image, which is
 * what bounds the bs = 1 kernels), the detection tail and the second stage run per image.  This is how a server folds concurrent
 * single-image requests (the reference's inference protocol is one image per forward, ref:fewx/modeling/fsod/fsod_cen.py:434-527);
 * image b's results are the buffers "out_boxes#b", "counts#b", "det_boxes#b", ... ("#0" may be omitted). */
int ore_engine_eval_batch_fwd(ore_engine* e, const void* img, int32_t img_is_u8, int32_t B, int32_t H, int32_t W, int32_t use_graph,
                              void* stream);
/* N-way inference: ONE query image against K support classes in one pass (FewX's per-class loop, ref:fewx/modeling/fsod/fsod_rcnn.py:445-512
 * and ref:fewx/modeling/fsod/fsod_roi_heads.py:144-191; the CenterNet2 variant keeps only the last class).  Class slot k
 * lives where image k of a batch would, so K <= cfg.max_batch.  The pass: backbone + FPN once; the depthwise correlation fanned out to the
 * K class blocks in one launch (per class bit-identical to the single-class correlation); conv3, tower and head over the K blocks as one
 * batch; the K proposal tails through ore_detect_batch_fwd; per class the second stage with that class's composed fc1 (score filter, NMS,
 * top-k -> "det_boxes#k" / "det_scores#k" / "det_count#k"); then ONE merge kernel: the union of the K lists ordered by score descending,
 * ties by class slot, then by row within the class, cut at the set_roi_head topk (= FewX's class-aware batched_nms + top-k, since
 * per-class NMS is independent), detector_postprocess as in ore_engine_detect_fwd, classes = the class ids.  Every existing entry point
 * behaves as before when ore_engine_set_classes was never called (or n = 0).
 *   ore_engine_set_classes: n <= min(max_batch, ORE_MAX_CLASSES) class ids (host, int64), slot k <- class_ids_host[k]; n = 0 = off.  Needs a
 *     finalized fp32-storage engine (a bf16-storage engine is refused).  The first call with n >= 1 allocates the slot tables.
 *   ore_engine_set_support_slot: ore_engine_set_support for class slot `slot` (after ore_engine_set_classes).
 *   ore_engine_set_roi_support_slot: the composed DSA-mix + fc1 (W_host [fc_dim][pooled*pooled*fpn_ch], b_host [fc_dim], the output of
 *     orehip.compose_roi_head for that class's rcnn_8 features) of class slot `slot` (after ore_engine_set_roi_head and _set_classes).
 *   ore_engine_detect_classes_begin: ore_engine_detect_begin for the N-way pass (ended by ore_engine_detect_end); the record's classes
 *     are the class ids.  The merged rows are also in "final_boxes" / "final_scores" / "final_classes" / "final_count" (slot 0).
 *   ore_engine_eval_classes_fwd: the same pass without a record (use_graph as ore_engine_eval_fwd); buffers read back as a K-image batch.
 * A pass with a slot left unset is refused.  Changing the class set or a slot drops the captured N-way graphs (their key holds K). */
#define ORE_MAX_CLASSES 16
int ore_engine_set_classes(ore_engine* e, int32_t n, const int64_t* class_ids_host);
int ore_engine_set_support_slot(ore_engine* e, int32_t slot, int32_t level, const float* proto_chw_host, int32_t C, int32_t s);
int ore_engine_set_roi_support_slot(ore_engine* e, int32_t slot, const float* W_host, const float* b_host);
/* Stage `stage` of a cascade engine's class slot (stage 0 = ore_engine_set_roi_support_slot). */
int ore_engine_set_roi_support_slot_stage(ore_engine* e, int32_t slot, int32_t stage, const float* W_host, const float* b_host);
int ore_engine_detect_classes_begin(ore_engine* e, const void* img, int32_t img_is_u8, int32_t H, int32_t W, int32_t out_h, int32_t out_w,
                                    void* out_record, void* stream);
int ore_engine_eval_classes_fwd(ore_engine* e, const void* img, int32_t img_is_u8, int32_t H, int32_t W, int32_t use_graph, void* stream);
/* Named device buffers: "p3","p4","p5" (NHWC, ld=2*fpn_ch, coff=fpn_ch), "pos3".."pos5", "head3".."head5",
 * "pre_boxes","pre_scores","pre_loc","keep_idx","counts","out_boxes","out_scores", "stage2".."stage5", ...
 * Returns device pointer and fills dims[0..3] = {rows(H*W*B), channels, ld, coff}.
 * Read-only names of the buffers a pass reuses, for tests that hold a launch on the engine's own inputs (K = 2..5; each name exists
 * only where the body has the buffer, ORE_ENOENT otherwise):
 *   "ycatK"  a stage of more than one block: the output map of its concat convs (after a pass: the LAST block's, before its tail);
 *   "icatK"  the same stage: the concat buffer of the identity blocks with an even number (block 2, 4, ...): channels [0, out_ch) are the
 *            identity = the tail of the block before, then the block's layers; "icatKb": the buffer of blocks 3, 5, ... (from three
 *            blocks on).  After a pass each holds the last block that ran in it;
 *   "redK"   a depthwise stage with a 1x1 reduction conv: its output map [M][conv_ch], the input of unit 0. */
int ore_engine_buffer(ore_engine* e, const char* name, void** dev_ptr, int64_t dims[4]);
/* Algorithmic FLOPs of the dense part of the last forward (2*MAC of every conv), for roofline accounting. */
double ore_engine_last_flops(ore_engine* e);
/* Measurement aid (bench.py roofline leg): when enabled, every implicit-GEMM conv launch of an EAGER forward is
 * bracketed by hipEvents on the launch stream; read_profile synchronises, returns the summed conv-kernel time,
 * the algorithmic FLOPs of those launches and the launch count since the last read, and resets the counters. */
int ore_engine_set_profiling(ore_engine* e, int32_t enable);
int ore_engine_read_profile(ore_engine* e, double* conv_ms, double* conv_flops, int32_t* n_launches);
/* Of the conv FLOPs the last ore_engine_read_profile reported: the multiplies the matrix cores actually executed (a layer on the
 * Winograd F(2x2,3x3) kernel executes its algorithmic count / 2.25). */
double ore_engine_profile_executed_flops(ore_engine* e);
/* What bracketing ONE launch with hipEvents adds beyond the launch itself: 2*T(1) - T(2), T(n) = median time of (event, n empty
 * launches, event) on `stream`; subtracting launches x this value makes the event-based kernel time agree with rocprofv3's. */
int ore_event_pair_overhead_us(void* stream, int32_t reps, double* median_us);

/* ------------------------------------------------------------------ gradient exchange (RCCL) -- */
/* The data-parallel train step's ONE exchange: replaces DistributedDataParallel's bucketed gradient all-reduce
 * (d2z:engine/defaults.py:60-79 create_ddp_model, :383; behind losses.backward() in d2z:engine/train_loop.py:258-294).  The flat fp32
 * gradient bucket is reduced in place, slice by slice, on a HIP stream of the caller's choice; 1 / world is folded into
 * ore_sgd_step_fwd (grad_scale).  RCCL is resolved at run time (no link-time dependency; path NULL = the copy already mapped into the
 * process, else librccl.so by the loader's search path).
 *   rank 0:      ore_rccl_unique_id(id)            -> hand the 128 bytes to every rank (any side channel)
 *   every rank:  ore_rccl_comm_create(id, world, rank, &comm)      collective; call with the exchanging device current
 *   per slice:   ore_allreduce_grads(comm, grads + begin, count, stream)   returns at once; order it with events
 *   at the end:  ore_rccl_comm_destroy(comm) */
int32_t ore_rccl_load(const char* path);
int32_t ore_rccl_unique_id(void* id128);
int32_t ore_rccl_comm_create(const void* id128, int32_t world, int32_t rank, void** comm);
int32_t ore_rccl_comm_destroy(void* comm);
int32_t ore_allreduce_grads(void* comm, float* grads, size_t count, void* stream);

/* ------------------------------------------------------------------ COCO box AP --------------- */
/* pycocotools COCOeval, iouType "bbox", useCats 1 (evaluate + accumulate) on the device, bit-exact against its published definition;
 * replaces d2z:evaluation/coco_evaluation.py _evaluate_predictions_on_coco (COCOeval_opt in d2z:evaluation/fast_eval_api.py).
 * Detections: n_dets rows in results-json order; det_boxes [n][4] XYXY fp32 (XYWH = (x0, y0, x1 - x0, y1 - y0) in fp32, widened),
 * det_scores [n] fp32, det_image [n] index into the images sorted by id, det_cat [n] index into the categories sorted by id (a row
 * whose index is out of range is dropped).  Ground truth, grouped by (category, image) pair p = cat * n_images + image, json order
 * inside a pair: gt_off [n_cats * n_images + 1] int32 offsets, gt_boxes [n_gts][4] XYWH fp64, gt_area (the json "area") fp64,
 * gt_crowd int32, gt_id (the json "id") int64.  Parameters are host arrays: iou_thrs [T <= 16], rec_thrs [R <= 128, non-decreasing],
 * area_rngs [A <= 8][2], max_dets [M <= 4, non-decreasing, last <= 128]; A * T <= 64; n_dets < 2^21.
 * Outputs (fp64, -1 where COCOeval leaves -1): precision [T][R][K][A][M], recall [T][K][A][M], scores [T][R][K][A][M].
 * Deterministic, no host synchronisation; workspace: ore_coco_eval_workspace_bytes. */
typedef struct ore_coco_eval_desc {
    int32_t n_images, n_cats;
    const float* det_boxes; const float* det_scores; const int32_t* det_image; const int32_t* det_cat; int32_t n_dets;
    const double* gt_boxes; const double* gt_area; const int32_t* gt_crowd; const int64_t* gt_id; const int32_t* gt_off; int32_t n_gts;
    const double* iou_thrs_host; int32_t n_iou_thrs;
    const double* rec_thrs_host; int32_t n_rec_thrs;
    const double* area_rngs_host; int32_t n_areas;
    const int32_t* max_dets_host; int32_t n_max_dets;
    double* precision; double* recall; double* scores;
    void* workspace; size_t workspace_bytes;
} ore_coco_eval_desc;
/* Optional output of the per-image stage (evaluateImg), for tests.  A unit is a (category, image) pair with at least one GT or one
 * detection, units in pair order; capacity >= min(n_cats * n_images, n_dets + n_gts).  n_units [1]; unit_pair [cap];
 * det_index [cap][max_det]: input row of the detection of rank r (r < the unit's kept count, score descending, stable);
 * dt_matches [cap][A][T][max_det]: the matched GT's json id, 0 if none (dtMatches); dt_ignore [cap][A][T][max_det] (dtIgnore);
 * gt_npig [cap][A]: the unit's GTs that are not ignored in that area range. */
typedef struct ore_coco_eval_images {
    int32_t* n_units; int32_t* unit_pair; int32_t* det_index; int64_t* dt_matches; uint8_t* dt_ignore; int32_t* gt_npig;
    int64_t capacity;
} ore_coco_eval_images;
size_t ore_coco_eval_workspace_bytes(int32_t n_cats, int32_t n_images, int32_t n_dets, int32_t n_gts, int32_t n_iou_thrs,
                                     int32_t n_areas, int32_t max_det);
int ore_coco_eval(const ore_coco_eval_desc* desc, const ore_coco_eval_images* per_image /* NULL: not wanted */, void* stream);

/* ------------------------------------------------------------------ proposal recall ----------- */
/* Proposal AR (AR@100 .. ARl@1000 of "box_proposals") on the device: the reference's _evaluate_box_proposals
 * (ref:fewx/evaluation/coco_evaluation.py:453-561) for every (limit, area range) pair in one call, bit-exact.
 * Proposals of all prediction entries concatenated: prop_boxes [n_props][4] XYXY fp32, prop_logits [n_props] fp32; entry e owns rows
 * entry_off[e] .. entry_off[e + 1] (int32 [n_entries + 1]) and belongs to image entry_image[e] (index into the images sorted by id).
 * Ground truth per image, json order, every category: gt_off [n_images + 1] int32, gt_boxes [n_gts][4] XYWH fp64, gt_area fp64,
 * gt_crowd int32.  Host parameter arrays: area_rngs [A][2] doubles (rounded to fp32 here), limits [L] (1 .. 2048), iou_thrs [T <= 16]
 * fp32; A * L <= 8.  Chain c = l * A + a.
 * Per entry: proposals by logit descending, ties in input order; the image's non-crowd GTs as fp32 XYXY; IoU in fp32 as detectron2's
 * pairwise_iou; per chain the greedy extraction over the first limit proposals and the GTs whose fp32 area lies in [lo, hi]: largest
 * remaining IoU, ties to the lowest GT then the lowest proposal, min(P', G) times, the rest of the G-long vector 0.
 * Capacities the caller states (they bound what is written; an entry that does not fit is skipped and *status becomes non-zero):
 * n_slots >= the sum over the entries of their image's GT count (crowd included); n_iou_cells >= the sum over the entries of
 * min(P, max limit) * that GT count where this product exceeds ore_proposal_recall_lds_cells().
 * Outputs: num_pos [L * A] int64; gt_overlaps [L * A][n_slots] fp32, row c ascending, its first num_pos[c] values valid (the
 * rest all-ones bit patterns); counts [L * A][T] int64: overlaps >= iou_thrs[t]; status [1] int32: 0, or non-zero for an entry with bad
 * offsets / image index or one past the stated capacities.  Optional (all three or none): entry_overlaps [L * A][n_slots] fp32, the
 * recorded vector of entry e and chain c at [c][entry_slot_off[e] ..] with entry_valid[e][c] values; entry_slot_off [n_entries + 1]
 * int32; entry_valid [n_entries][L * A] int32.  Deterministic (integer atomics only count), no host synchronisation. */
typedef struct ore_proposal_recall_desc {
    int32_t n_entries, n_images;
    const float* prop_boxes; const float* prop_logits; int32_t n_props;
    const int32_t* entry_off; const int32_t* entry_image;
    const double* gt_boxes; const double* gt_area; const int32_t* gt_crowd; const int32_t* gt_off; int32_t n_gts;
    const double* area_rngs_host; int32_t n_areas;
    const int32_t* limits_host; int32_t n_limits;
    const float* iou_thrs_host; int32_t n_iou_thrs;
    int32_t n_slots; int64_t n_iou_cells;
    int64_t* num_pos; float* gt_overlaps; int64_t* counts; int32_t* status;
    float* entry_overlaps; int32_t* entry_slot_off; int32_t* entry_valid;
    void* workspace; size_t workspace_bytes;
} ore_proposal_recall_desc;
int32_t ore_proposal_recall_lds_cells(void);
size_t ore_proposal_recall_workspace_bytes(int32_t n_entries, int32_t n_props, int32_t n_slots, int64_t n_iou_cells, int32_t n_areas,
                                           int32_t n_limits);
int ore_proposal_recall(const ore_proposal_recall_desc* desc, void* stream);

/* ------------------------------------------------------------------ image resize -------------- */
/* Pillow's Image.resize(size, BILINEAR) for 8-bit images, byte for byte (ImagingResample: antialiased separable triangle filter,
 * 22-bit fixed-point weights, horizontal pass to a uint8 intermediate, then the vertical pass); replaces the CPU resize of
 * ResizeShortestEdge in front of the detector (d2z:data/transforms/augmentation_impl.py, d2z:data/transforms/transform.py
 * ResizeTransform.apply_image; d2z:engine/defaults.py DefaultPredictor.__call__).  Sides 1 .. 8192.
 * Planner (host only, no GPU needed), one axis: bounds_host [out][2] = (first source index, count), coeffs_host [out][ksize] with
 * ksize = ore_resize_ksize(in, out) = 2 * ceil(max(in / out, 1)) + 1 (0 for sizes out of range); entries past `count` are 0.
 * Device tables of one (h, w, nh, nw): ore_resize_table_ints() int32 values laid out x bounds [nw][2] | y bounds [nh][2] |
 * x coefficients [nw][ksize_x] | y coefficients [nh][ksize_y], filled on the host by ore_resize_tables_host and copied by the caller.
 * ore_resize_bilinear_u8_fwd: src_hwc [h][w][3] uint8 interleaved -> dst_chw [3][nh][nw] uint8 planar (the engine's uint8 image
 * layout); swap_rb exchanges channels 0 and 2.  form 0: ORE_RESIZE_FORM_LDS (one launch, the intermediate stays in LDS) where a
 * tile's staging fits 64 KiB of LDS, else ORE_RESIZE_FORM_WORKSPACE (two launches, the intermediate [h][nw][3] in `workspace`,
 * ore_resize_workspace_bytes); a form code forces that form (the LDS form where it does not fit: ORE_EINVAL).  ore_resize_form tells
 * which one form 0 takes.  Both forms write the same bytes; nothing outside dst_chw[0, 3 * nh * nw) is written. */
#define ORE_RESIZE_FORM_LDS 1
#define ORE_RESIZE_FORM_WORKSPACE 2
int32_t ore_resize_ksize(int32_t in, int32_t out);
int ore_resize_plan(int32_t in, int32_t out, int32_t* bounds_host, int32_t* coeffs_host, int32_t* ksize_out /* or NULL */);
size_t ore_resize_table_ints(int32_t h, int32_t w, int32_t nh, int32_t nw);
int ore_resize_tables_host(int32_t h, int32_t w, int32_t nh, int32_t nw, int32_t* tables_host);
int32_t ore_resize_form(int32_t h, int32_t w, int32_t nh, int32_t nw);
size_t ore_resize_workspace_bytes(int32_t h, int32_t w, int32_t nh, int32_t nw);
int ore_resize_bilinear_u8_fwd(const uint8_t* src_hwc, int32_t h, int32_t w, uint8_t* dst_chw, int32_t nh, int32_t nw, int32_t swap_rb,
                               const int32_t* tables_dev, int32_t form, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ support crops -------------- */
/* "Support crop v1": the S x S support crop of one annotated box of a frame, and the box inside the crop -- what compute_support_dict
 * and generate_support take.  A contract of this package, shaped like FewX's crop_support (a square window around the object with
 * `context` pixels of context at the crop's scale); no equality with FewX is claimed.  The resampler is the one above (Pillow's
 * BILINEAR), so Pillow is the oracle.  With frame [h][w][3] uint8, box (x1, y1, x2, y2) XYXY absolute fp32, c = context,
 * T = S - 2c, all integer arithmetic with floor division:
 *   integer box        bx0 = max(0, floor x1), by0 = max(0, floor y1), bx1 = min(w, ceil x2), by1 = min(h, ceil y2); bw = bx1 - bx0,
 *                      bh = by1 - by0; bw < 1 or bh < 1 (the box lies outside the frame) is refused
 *   window             L = max(bw, bh), m = (c * L + T - 1) / T, D = L + 2m, origin x0 = bx0 - (D - bw) / 2, y0 = by0 - (D - bh) / 2
 *   source rectangle   window clipped to the frame: rx0 = max(x0, 0), rx1 = min(x0 + D, w), ry0, ry1 likewise
 *   destination rect   dx0 = ((rx0 - x0) * S + D / 2) / D, dx1 = ((rx1 - x0) * S + D / 2) / D, dy0, dy1 likewise
 *   pixels             crop[:, dy0:dy1, dx0:dx1] = Image.fromarray(frame[ry0:ry1, rx0:rx1]).resize((dx1 - dx0, dy1 - dy0), BILINEAR),
 *                      every other pixel = fill (per channel); planar [3][S][S] in the frame's channel order
 *   support box        fp32, in this order, no contraction: sx = float(dx1 - dx0) / float(rx1 - rx0), x' = float(dx0) + (x - float(rx0)) * sx
 *                      (y likewise), then clipped to [0, S]
 * A call's K jobs live in one buffer of int32 words that the caller owns: K records of ORE_SUPPORT_JOB_INTS words, then every job's
 * resample tables (x bounds [nw][2] | y bounds [nh][2] | x coefficients [nw][ksx] | y coefficients [nh][ksy], nw = dx1 - dx0,
 * nh = dy1 - dy0, each axis exactly what ore_resize_plan(source side, destination side) writes).  Record words (ORE_SJ_*): the
 * frame's device address (low, high word) and size, the source and destination rectangles, the offsets (in words from the buffer's
 * start) and tap counts of the four tables, the job's form and LDS sizing, the byte offset of its workspace slice (low, high), D and the
 * window origin, and the support box as four float bit patterns.
 * ore_support_crop_job_ints: words of one job's tables (0: the job is refused -- box outside the frame, or sizes out of range: frame
 *   sides 1 .. 8192, 2 * context < S <= 8192).  A buffer holds K * ORE_SUPPORT_JOB_INTS + the sum of these.
 * ore_support_crop_form: ORE_RESIZE_FORM_LDS where the job's 16 x 64 output tiles fit the one-launch LDS budget of the resize (64 KiB
 *   of staged source, intermediate and tables), else ORE_RESIZE_FORM_WORKSPACE (0: refused).  ore_support_crop_workspace_bytes: the
 *   job's slice of the workspace, (ry1 - ry0) * nw * 3 bytes rounded up to 16, 0 for a job of the LDS form.
 * ore_support_crop_plan (host only, no GPU needed): writes the record to record_host[ORE_SUPPORT_JOB_INTS] and the tables to
 *   buffer_host + table_off; frame_dev is stored, not read.
 * ore_support_crop_u8_fwd: dst [K][3][S][S] uint8 from K jobs (frames of any sizes).  One launch serves every tile of every job of the
 *   LDS form; jobs of the workspace form take a horizontal launch into their workspace slices and a vertical one: at most three
 *   launches whatever K.  Every byte of dst is written exactly once, fill included; nothing else is written.  fill_rgb = channel 0 |
 *   channel 1 << 8 | channel 2 << 16.  jobs_host is the buffer as planned (read on the host to check every record against the buffer,
 *   the workspace and the canvas before anything is launched), jobs_dev its copy on the device, complete in stream order. */
#define ORE_SUPPORT_JOB_INTS 32
#define ORE_SJ_FRAME_LO 0
#define ORE_SJ_FRAME_HI 1
#define ORE_SJ_H 2
#define ORE_SJ_W 3
#define ORE_SJ_RX0 4      /* source rectangle rx0, ry0, rx1, ry1 */
#define ORE_SJ_DX0 8      /* destination rectangle dx0, dy0, dx1, dy1 */
#define ORE_SJ_XB 12      /* table offsets: x bounds, y bounds, x coefficients, y coefficients */
#define ORE_SJ_YB 13
#define ORE_SJ_KX 14
#define ORE_SJ_KY 15
#define ORE_SJ_KSX 16
#define ORE_SJ_KSY 17
#define ORE_SJ_FORM 18
#define ORE_SJ_LDS_R 19
#define ORE_SJ_LDS_S 20
#define ORE_SJ_WS_LO 21
#define ORE_SJ_WS_HI 22
#define ORE_SJ_D 24
#define ORE_SJ_X0 25      /* window origin x0, y0 */
#define ORE_SJ_BOX 27     /* support box, four float bit patterns */
size_t ore_support_crop_job_ints(int32_t h, int32_t w, const float* box_xyxy, int32_t S, int32_t context);
int32_t ore_support_crop_form(int32_t h, int32_t w, const float* box_xyxy, int32_t S, int32_t context);
size_t ore_support_crop_workspace_bytes(int32_t h, int32_t w, const float* box_xyxy, int32_t S, int32_t context);
int ore_support_crop_plan(int32_t h, int32_t w, const float* box_xyxy, int32_t S, int32_t context, const uint8_t* frame_dev,
                          int64_t table_off, int64_t workspace_off, int32_t* record_host, int32_t* buffer_host);
int ore_support_crop_u8_fwd(const int32_t* jobs_dev, const int32_t* jobs_host, size_t buffer_ints, int32_t K, int32_t S, int32_t fill_rgb,
                            uint8_t* dst, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ test-time augmentation ---- */
/* The device side of GeneralizedRCNNWithTTA (d2z:modeling/test_time_augmentation.py): everything between and behind the engine passes
 * of one image's variants, enqueued on `stream`, no host synchronisation.
 * ore_tta_hflip_u8_fwd: dst[r][x] = src[r][nw - 1 - x] for `rows` rows of nw bytes (a planar [3][nh][nw] image: rows = 3 * nh <= 65535);
 *   the flipped variant is HFlipTransform.apply_image of the resized one, so it is a copy of the bytes ore_resize_bilinear_u8_fwd wrote.
 * ore_tta_collect_fwd: one variant's detection rows -- boxes [n][4], scores [n], classes [n] int64 (NULL: all 0), n = min(*n_dev if
 *   n_dev else n_host, max_rows) -- through tfm.inverse().apply_box in fp32, every operation rounded on its own: flip != 0: x = variant_w
 *   - x; x *= sx, y *= sy (ResizeTransform variant -> image, the ratios rounded to fp32 by the caller); pre != 0: x *= px, y *= py (the
 *   mapper's pre-transform undone); then (min x, min y, max x, max y) with numpy's NaN rule.  The rows are appended to the pool (boxes
 *   [pool_cap][4], scores, classes int64) at the running offset *pool_n, which the call advances (variant == 0 restarts it at 0; rows that
 *   would pass pool_cap are cut); var_counts[variant] = the rows taken.
 * ore_tta_merge_fwd: fast_rcnn_inference_single_image (d2z:modeling/roi_heads/fast_rcnn.py) over the first min(*pool_n, cap) pool rows:
 *   rows with a non-finite value dropped, boxes clipped to (out_h, out_w), score > score_thresh, stable sort by score (ties keep pool
 *   order), greedy NMS per class id on the true coordinates with the IoU arithmetic of ore_nms_fwd, the first topk survivors -> out_record
 *   ([rec_rows][4] f32 boxes | [rec_rows] f32 scores | [rec_rows] int64 classes, rec_rows even and >= topk) and out_count[0] (device).
 *   cap <= 8192; class ids must fit 32 bits; workspace: ore_tta_merge_workspace_bytes(cap) (0 for a cap out of range).  No float
 *   atomics: bit-reproducible run to run. */
int ore_tta_hflip_u8_fwd(const uint8_t* src, uint8_t* dst, int32_t rows, int32_t nw, void* stream);
int ore_tta_collect_fwd(const float* boxes, const float* scores, const int64_t* classes, const int32_t* n_dev, int32_t n_host,
                        int32_t max_rows, int32_t flip, int32_t variant_w, float sx, float sy, int32_t pre, float px, float py,
                        float* pool_boxes, float* pool_scores, int64_t* pool_classes, int32_t* pool_n, int32_t pool_cap,
                        int32_t* var_counts, int32_t variant, void* stream);
size_t ore_tta_merge_workspace_bytes(int32_t cap);
int ore_tta_merge_fwd(const float* pool_boxes, const float* pool_scores, const int64_t* pool_classes, const int32_t* pool_n, int32_t cap,
                      int32_t out_h, int32_t out_w, float score_thresh, float nms_thresh, int32_t topk, void* out_record,
                      int32_t rec_rows, int32_t* out_count, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ detection overlay --------- */
/* Detections drawn onto an interleaved [h][w][3] uint8 frame on the device (detectron2's Visualizer.draw_instance_predictions for
 * boxes: d2z:utils/visualizer.py; the demo's VisualizationDemo / AsyncPredictor), enqueued on `stream`, no host synchronisation.  The
 * rows are read where a detection pass left them: boxes [n][4] fp32 xyxy at the frame's size, scores [n], classes [n] int64 (NULL: all
 * 0), n = min(*n_dev if n_dev else n_host, max_rows) -- a pending pass's record and its device count serve as they are.
 * dst_hwc == src_hwc draws in place; otherwise the frame is copied and drawn in the same pass (the two must not overlap).
 * Render contract "overlay v1" -- all pixel arithmetic integer, the result bit-exact and independent of scheduling:
 *   blend(p, c, a) = (p * (255 - a) + c * a + 127) / 255 per channel, integer division, a in 0 .. 255.
 *   Row i is drawn iff its four coordinates and its score are finite, score >= score_thresh (fp32) and the integer rectangle
 *     X0 = max((int)floorf(x0), 0), Y0 = max((int)floorf(y0), 0), X1 = min((int)ceilf(x1), w) - 1, Y1 = min((int)ceilf(y1), h) - 1
 *     is non-empty (X1 >= X0 and Y1 >= Y0).
 *   Draw order: area_i = (x1 - x0) * (y1 - y0) in fp32 on the raw coordinates, each operation rounded on its own (a NaN product, inf * 0,
 *     counts as 0), descending, ties by i ascending: large boxes first, small ones on top.
 *   Colour c_i = palette[(color_by ? class_i : i) mod n_palette] (non-negative mod); palette [n_palette][3] uint8 in the frame's channel
 *     order, 1 <= n_palette <= 256.
 *   Outline: the rectangle's pixels with x - X0 < L, X1 - x < L, y - Y0 < L or Y1 - y < L (L = line_width, 1 .. 16) become
 *     blend(p, c_i, edge_alpha).
 *   Label (text_scale S >= 1; S = 0 draws none): text = name + " " + pct + "%", or pct + "%" when the name is empty; name =
 *     names[class_i], table [n_names][32] ASCII NUL-padded, empty when the id is out of range or names_dev is NULL; pct =
 *     clamp((int)rintf(score * 100.0f), 0, 100), the product in fp32, half to even; at most 40 characters.  Glyph cells 6S x 11S, pad S:
 *     the label rectangle is len * 6S + 2S wide and 13S high at lx = clamp(X0, 0, max(w - width, 0)), ly = clamp(Y0, 0, max(h -
 *     height, 0)), pixels outside the frame dropped.  Its pixels become blend(p, 0, label_alpha); glyph pixel (u, v) of character ch
 *     (cell k at lx + S + k * 6S, ly + S) is set iff atlas[ch - 32][v / S][u / S] (characters outside 32 .. 126: blank) and is then
 *     replaced by the text colour t = c + ((255 - c) * 7) / 10 per channel.
 *   Per pixel the instances apply in draw order; per instance outline, then label background, then glyph.
 *   atlas_dev [95][11][6] bytes (0 / 1) for ASCII 32 .. 126 (needed when S >= 1).
 * Limits (ORE_EINVAL): sides 1 .. ORE_OVERLAY_MAX_SIDE, max_rows <= ore_det_record_rows(), L in 1 .. 16, S in 0 .. 8, alphas 0 .. 255;
 * frames 4-byte aligned.  workspace: ore_overlay_workspace_bytes(max_rows) (0 for max_rows out of range), private to the stream. */
#define ORE_OVERLAY_MAX_SIDE 8192
size_t ore_overlay_workspace_bytes(int32_t max_rows);
int ore_overlay_draw_fwd(const uint8_t* src_hwc, uint8_t* dst_hwc, int32_t h, int32_t w, const float* boxes, const float* scores,
                         const int64_t* classes, const int32_t* n_dev, int32_t n_host, int32_t max_rows, float score_thresh,
                         int32_t line_width, int32_t text_scale, int32_t edge_alpha, int32_t label_alpha, const uint8_t* palette_dev,
                         int32_t n_palette, int32_t color_by, const uint8_t* names_dev, int32_t n_names, const uint8_t* atlas_dev,
                         void* workspace, size_t workspace_bytes, void* stream);
/* "overlay v1, track colouring": ore_overlay_draw_fwd with one more row array, ids [max_rows] int64 (the ids_out of
 * ore_track_update_fwd), and one more colour source, color_by == 2 ("track").  With color_by == 2 a row is drawn iff it is drawn by
 * overlay v1 and ids[i] >= 0; its colour is c_i = palette[ids[i] mod n_palette]; its label text is "#" + decimal(ids[i]) + " " in front
 * of the text overlay v1 defines, cut at the same 40 characters, and the label rectangle follows from the new text's length.  Draw
 * order, outline, label geometry and blends are overlay v1's.  color_by 0 and 1 ignore ids (NULL allowed) and give the bytes of
 * ore_overlay_draw_fwd; color_by == 2 with ids == NULL, or a color_by outside 0 .. 2, is ORE_EINVAL. */
int ore_overlay_draw_ids_fwd(const uint8_t* src_hwc, uint8_t* dst_hwc, int32_t h, int32_t w, const float* boxes, const float* scores,
                             const int64_t* classes, const int64_t* ids, const int32_t* n_dev, int32_t n_host, int32_t max_rows,
                             float score_thresh, int32_t line_width, int32_t text_scale, int32_t edge_alpha, int32_t label_alpha,
                             const uint8_t* palette_dev, int32_t n_palette, int32_t color_by, const uint8_t* names_dev, int32_t n_names,
                             const uint8_t* atlas_dev, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ detection tracking -------- */
/* Detections followed from frame to frame on the device: every row of a frame gets the id of the track it continues, or a new one.
 * The update is enqueued on `stream` -- one launch, no host synchronisation, no allocation -- and reads the rows where a detection pass
 * left them, with ore_overlay_draw_fwd's conventions: boxes [rows][4] fp32 xyxy, scores [rows], classes [rows] int64 (NULL: all 0),
 * n = min(*n_dev if n_dev else n_host, max_rows) (a negative count is 0).  ids_out [max_rows] int64 serves ore_overlay_draw_ids_fwd as
 * it is.  The contract has the shape of detectron2's VideoVisualizer._assign_colors (IoU association among equal labels, a time to live
 * for a track the detector missed) but is one-to-one and fully ordered, which that heuristic is not: no equality with it is claimed.
 * Association contract "track v1" -- bit-exact, a function of the inputs alone:
 *   State: an ordered list of m <= capacity tracks (box[4] fp32 xyxy, class int64, id int64, ttl int32), and next_id (int64, starts at
 *     0), frames, dropped (int64).  capacity 1 .. ORE_TRACK_MAX_TRACKS.
 *   Live rows: row i < n is live iff its four coordinates and its score are finite and score >= score_thresh (fp32).  Every other row
 *     of 0 .. max_rows - 1 gets ids_out[i] = -1 and takes no part.
 *   IoU(t, d), fp32, every operation rounded on its own: area = (x1 - x0) * (y1 - y0); iw = min(x1t, x1d) - max(x0t, x0d), ih likewise;
 *     inter = (iw > 0 && ih > 0) ? iw * ih : 0; iou = inter > 0 ? inter / ((area_t + area_d) - inter) : 0.
 *   Candidates: (track t, live row d) with iou > iou_thresh (strict; a NaN compares false) and, unless class_aware == 0, equal classes.
 *   Matching: the candidates ordered by (iou descending, track slot ascending, row ascending) are taken greedily: a pair is accepted
 *     iff neither its track nor its row has been taken.  A matched row takes its track's id.
 *   New ids: the unmatched live rows get next_id, next_id + 1, ... in row order; next_id advances by their number.
 *   The new list: first the live rows in row order (the row's box and class, its id, ttl = the call's ttl), then the unmatched old
 *     tracks in their order with ttl - 1, those with a new ttl > 0 only.  A list longer than capacity is cut at capacity -- the tail,
 *     the longest-unmatched survivors, is lost -- and dropped grows by the number cut (capacity >= max_rows never loses a live row).
 *     frames += 1.
 * The state is one caller-owned device buffer of ore_track_state_bytes(capacity) bytes (0 for a capacity out of range), 16-byte
 * aligned: a 32-byte header { int32 m, capacity; int64 next_id, frames, dropped }, then boxes [capacity][4] fp32, classes [capacity]
 * int64, ids [capacity] int64, ttl [capacity] int32, rounded up to 16 bytes.  Slots m .. capacity - 1 hold zeros.  ore_track_reset
 * writes the empty state; only it and ore_track_update_fwd write the buffer, and `capacity` is the same in every call on one buffer.
 * ore_track_workspace_bytes is what `workspace` must hold (0: the update works in LDS and registers; NULL is then allowed).
 * Limits (ORE_EINVAL before any launch): capacity 1 .. ORE_TRACK_MAX_TRACKS, max_rows 0 .. ore_det_record_rows(), ttl 1 .. 1 << 20,
 * iou_thresh finite and >= 0, score_thresh not NaN; state, ids_out and the row arrays pairwise disjoint; boxes 16-byte aligned. */
#define ORE_TRACK_MAX_TRACKS 1024
size_t ore_track_state_bytes(int32_t capacity);
int ore_track_reset(void* state, int32_t capacity, void* stream);
size_t ore_track_workspace_bytes(int32_t capacity, int32_t max_rows);
int ore_track_update_fwd(void* state, int32_t capacity, const float* boxes, const float* scores, const int64_t* classes,
                         const int32_t* n_dev, int32_t n_host, int32_t max_rows, float score_thresh, float iou_thresh, int32_t ttl,
                         int32_t class_aware, int64_t* ids_out, void* workspace, size_t workspace_bytes, void* stream);

/* The wide form: the same contract "track v1" -- the same state buffer, the same ids and the same new list for the same inputs -- for
 * the rows a tiled or TTA merge hands over: up to ORE_TRACK_WIDE_MAX_ROWS rows (the merge pool's 8192) and ORE_TRACK_WIDE_MAX_TRACKS
 * tracks (that many live rows plus as many survivors) per update.  Two launches on `stream`, no host synchronisation, no allocation:
 * the candidate bits of every (track, row) tile on the whole chip, then the matching and the new list in one workgroup.  The parameters
 * are ore_track_update_fwd's; `workspace` is a 256-byte aligned device buffer of at least ore_track_wide_workspace_bytes(capacity,
 * max_rows) bytes (0 for arguments out of range), disjoint from the state, ids_out and the row arrays; its contents mean nothing
 * between calls.  ore_track_wide_state_bytes is ore_track_state_bytes with the wide limit (0 beyond it); a buffer written by the one
 * form may be handed to the other while capacity and max_rows fit both.
 * Limits (ORE_EINVAL before any launch): capacity 1 .. ORE_TRACK_WIDE_MAX_TRACKS, max_rows 0 .. ORE_TRACK_WIDE_MAX_ROWS, ttl 1 ..
 * 1 << 20, iou_thresh finite and >= 0, score_thresh not NaN, boxes 16-byte aligned, a workspace that is too small. */
#define ORE_TRACK_WIDE_MAX_TRACKS 16384
#define ORE_TRACK_WIDE_MAX_ROWS 8192
size_t ore_track_wide_state_bytes(int32_t capacity);
size_t ore_track_wide_workspace_bytes(int32_t capacity, int32_t max_rows);
int ore_track_wide_reset(void* state, int32_t capacity, void* stream);
int ore_track_wide_update_fwd(void* state, int32_t capacity, const float* boxes, const float* scores, const int64_t* classes,
                              const int32_t* n_dev, int32_t n_host, int32_t max_rows, float score_thresh, float iou_thresh, int32_t ttl,
                              int32_t class_aware, int64_t* ids_out, void* workspace, size_t workspace_bytes, void* stream);

/* The belt's shift: "track v1" matches a row to a track's last observed box, so a track survives only while the scene moves less than
 * about a quarter of a box per frame.  A conveyor belt moves rigidly and much faster; the one translation the frame shares is voted
 * here from the boxes alone and every track box is moved by it BEFORE the update, which then associates as it always has.  The launches
 * are enqueued on `stream` in front of ore_track_update_fwd / ore_track_wide_update_fwd: no host synchronisation, no allocation.
 * Contract "belt shift v1" -- bit-exact, a function of the inputs alone:
 *   Parameters: bin in {1, 2, 4, 8, 16} pixels per bin; half_bins K in 1 .. ORE_BELT_MAX_HALF_BINS, the window is (2K + 1)^2 bins, so
 *     |shift| <= K * bin per axis; size_tol fp32, finite, 0 <= size_tol < 1; min_votes 1 .. 1 << 30; frame_h, frame_w both 0 (no frame
 *     test) or both > 0; score_thresh and class_aware as in "track v1".
 *   Inputs: the tracks 0 .. m - 1 of a "track v1" state buffer as they stand at entry; the frame's rows with that contract's conventions
 *     (boxes, scores, classes or NULL, n = min(*n_dev if n_dev else n_host, max_rows)) and its rule for a live row.
 *   Per box (track or row), one fp32 operation each: w = x1 - x0, h = y1 - y0, sx = x0 + x1, sy = y0 + y1.
 *   A pair (track t, row d) votes iff d is live; the classes are equal, unless class_aware == 0; all four extents are > 0;
 *     fabsf(wt - wd) <= size_tol * fmaxf(wt, wd) and the same for h (the difference, the absolute value, the product and the comparison
 *     are single fp32 operations); and with inv = 1 / (2 * bin), qx = floorf((sxd - sxt) * inv + 0.5f), qy likewise, fabsf(qx) <= K and
 *     fabsf(qy) <= K as floats (a NaN or an infinity fails).  The pair adds 1 to H[qy][qx] (int32).
 *   Smoothing: S[qy][qx] = the sum of H over the 3 x 3 neighbourhood, bins outside the window counting 0.
 *   Peak: the bin with the largest S; ties by |qx * bin - prev_dx| + |qy * bin - prev_dy| ascending (integers; the previous shift is
 *     the belt state's dx, dy at entry, 0, 0 after a reset), then qy ascending, then qx ascending.  It is accepted iff S >= min_votes:
 *     then dx = qx * bin, dy = qy * bin, votes = S.  Otherwise (m = 0 and n = 0 included) dx and dy keep their values -- the belt keeps
 *     running -- votes = 0 and coasted += 1.  In both cases travel_x += dx, travel_y += dy and frames += 1.
 *   Apply: every track box gets x0 += dx, x1 += dx, y0 += dy, y1 += dy, one fp32 add each: a track the detector misses travels with the
 *     belt until its ttl runs out.  With a frame, a track whose moved box has x1 <= 0 || x0 >= frame_w || y1 <= 0 || y0 >= frame_h gets
 *     ttl = 1: the update that follows drops it unless a row continues it (a NaN compares false: the track stays).  Nothing else of the
 *     track state changes.
 * The belt state is a caller-owned device buffer of ore_belt_state_bytes() = 64 bytes, 16-byte aligned: int32 dx, dy, votes, reserved (0);
 * int64 travel_x, travel_y, frames, coasted; then 16 zero bytes.  ore_belt_reset writes zeros.
 * Two forms, the same result.  Form 1 (capacity <= ORE_TRACK_MAX_TRACKS and max_rows <= ore_det_record_rows()): one launch of one
 * workgroup, rows and histogram in LDS, no workspace (NULL is allowed).  Form 2 (capacity <= ORE_TRACK_WIDE_MAX_TRACKS, max_rows <=
 * ORE_TRACK_WIDE_MAX_ROWS): the histogram's clear, a vote kernel over (track group, row tile) work items on the whole chip -- each block
 * votes into its own LDS histogram and adds its non-zero bins to the workspace's with integer atomics -- and a one-workgroup finish:
 * three operations on `stream`.  `workspace`: 256-byte aligned, at least ore_belt_workspace_bytes(capacity, max_rows, half_bins) bytes
 * (what form 2 needs; 0 for arguments out of range); its contents mean nothing between calls.  ore_belt_shift_form: the form that
 * form = 0 chooses, 1 or 2, or ORE_EINVAL.  form = 1 or 2 forces one (ORE_EINVAL if form 1 cannot take the shapes); form = 3 is form 2
 * with every vote added straight to the workspace histogram, a measurement aid with the same result.
 * Limits (ORE_EINVAL before any launch): the ranges above, boxes 16-byte aligned, the belt state, the track state, the workspace and the
 * row arrays pairwise disjoint, a workspace that is too small. */
#define ORE_BELT_MAX_HALF_BINS 64
size_t ore_belt_state_bytes(void);
int ore_belt_reset(void* belt, void* stream);
size_t ore_belt_workspace_bytes(int32_t capacity, int32_t max_rows, int32_t half_bins);
int ore_belt_shift_form(int32_t capacity, int32_t max_rows, int32_t half_bins);
int ore_belt_shift_fwd(void* belt, void* track_state, int32_t capacity, const float* boxes, const float* scores, const int64_t* classes,
                       const int32_t* n_dev, int32_t n_host, int32_t max_rows, float score_thresh, int32_t class_aware, int32_t bin,
                       int32_t half_bins, float size_tol, int32_t min_votes, int32_t frame_h, int32_t frame_w, int32_t form,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ heat maps ----------------- */
/* Heat maps of a detection pass drawn over an interleaved [h][w][3] uint8 frame on the device (ref:demo_visualizer.py Have_a_Look /
 * visualize_grid_attention_v2; ref:fewx/modeling/fsod/debug.py debug_test): where the class-agnostic objectness fired, where the
 * query-support correlation responded, what a feature channel looks like.  The sources are the level buffers a pass leaves in the engine
 * (ore_engine_buffer: rows, ch, ld, coff).  Everything is enqueued on `stream`: no host synchronisation, no allocation, at most three
 * launches (two with norm "unit").
 * Render contract "heatmap v1" -- bit-exact and independent of scheduling:
 *   Inputs: the frame; 1 .. 3 level maps, level l being h_l x w_l scalars at stride s_l; the model-input size (in_h, in_w) the maps were
 *     computed at (the unpadded size); a table lut [256][3] uint8 in the frame's channel order; alpha 0 .. 255 and alpha_mode.
 *   A, scalar per location (ore_heatmap_levels_fwd; fp32, or bf16 widened exactly): channel = c takes that channel; channel =
 *     ORE_HEATMAP_MEAN builds four fp32 partial sums over the channels c % 4 == j, each in ascending channel order, combines them as
 *     (s0 + s1) + (s2 + s3) and divides by (float)ch (ch a multiple of 4; every operation rounded on its own, the division correctly
 *     rounded).  transform ORE_HEATMAP_SIGMOID then applies 1 / (1 + ore_expf(-v)), the function the proposal decode thresholds with
 *     (ore_sigmoid_host is the same sequence of operations on the host).
 *   B, quantisation: norm ORE_HEATMAP_UNIT: q = (int)(fminf(fmaxf(v, 0), 1) * 255.0f) -- truncation, NaN gives 0.  norm
 *     ORE_HEATMAP_MAX: m = the maximum over all levels of fmaxf(v, 0) (found as an integer maximum over the bits of non-negative
 *     floats: no float atomics), q = (int)(fminf(fmaxf(v / m, 0), 1) * 255.0f), and m == 0 gives q = 0 everywhere.
 *   C, per frame pixel (x, y), all integer, for every level: U = floor(((2 x + 1) * in_w * 256) / (2 * w * s_l)) - 128 clamped to [0,
 *     (w_l - 1) * 256]; x0 = U >> 8, fx = U & 255, x1 = min(x0 + 1, w_l - 1); V, y0, y1, fy likewise from y, in_h, h, h_l;
 *     top = q[y0][x0] * (256 - fx) + q[y0][x1] * fx, bot the same on row y1, val_l = (top * (256 - fy) + bot * fy + 32768) >> 16;
 *     v = max over the levels of val_l.  (Cell (i, j) sits at input pixel (j * s + s / 2, i * s + s / 2).)
 *   D, blend: col = lut[v]; A = alpha (ORE_HEATMAP_ALPHA_CONSTANT) or (alpha * v + 127) / 255 (ORE_HEATMAP_ALPHA_VALUE: cold regions
 *     stay as they are); out_c = (img_c * (255 - A) + col_c * A + 127) / 255, integer division.  dst_hwc == src_hwc draws in place,
 *     otherwise the two must not overlap; bytes outside the frame are never written.
 * ore_heatmap_levels_fwd: stages A + B of n_levels level buffers into the workspace.  src_l = row 0 of level l's buffer ([batch * h_l *
 *   w_l] rows of ld_l elements, the `ch` channels at element coff_l); level_hw = host [n_levels][2] (h_l, w_l), level_ld / level_coff =
 *   host [n_levels]; slot = the image of the batch that is read.  The uint8 map of level l is then at workspace +
 *   ore_heatmap_level_offset(n_levels, level_hw, l), h_l * w_l bytes, rows contiguous.  The workspace
 *   (ore_heatmap_workspace_bytes(n_levels, level_hw); 0 for dimensions out of range) is private to the stream.
 * ore_heatmap_draw_fwd: stages C + D from 1 .. 3 such maps (device pointers; level_stride = host [n_levels]).
 * Limits (ORE_EINVAL): frame sides 1 .. ORE_OVERLAY_MAX_SIDE, frames 4-byte aligned; map sides 1 .. ORE_HEATMAP_MAX_MAP_SIDE; in_h, in_w
 * 1 .. ORE_HEATMAP_MAX_INPUT_SIDE; strides 1 .. ORE_HEATMAP_MAX_STRIDE; the mean needs ch, ld and coff multiples of 4. */
#define ORE_HEATMAP_MAX_LEVELS 3
#define ORE_HEATMAP_MAX_MAP_SIDE 4096
#define ORE_HEATMAP_MAX_INPUT_SIDE 8192
#define ORE_HEATMAP_MAX_STRIDE 128
#define ORE_HEATMAP_MEAN (-1)
#define ORE_HEATMAP_IDENTITY 0
#define ORE_HEATMAP_SIGMOID 1
#define ORE_HEATMAP_UNIT 0
#define ORE_HEATMAP_MAX 1
#define ORE_HEATMAP_ALPHA_CONSTANT 0
#define ORE_HEATMAP_ALPHA_VALUE 1
size_t ore_heatmap_workspace_bytes(int32_t n_levels, const int32_t* level_hw);
size_t ore_heatmap_level_offset(int32_t n_levels, const int32_t* level_hw, int32_t level);
int ore_heatmap_levels_fwd(int32_t n_levels, const void* src0, const void* src1, const void* src2, const int32_t* level_hw,
                           const int32_t* level_ld, const int32_t* level_coff, int32_t ch, int32_t is_bf16, int32_t batch, int32_t slot,
                           int32_t channel, int32_t transform, int32_t norm, void* workspace, size_t workspace_bytes, void* stream);
int ore_heatmap_draw_fwd(const uint8_t* src_hwc, uint8_t* dst_hwc, int32_t h, int32_t w, int32_t n_levels, const uint8_t* map0,
                         const uint8_t* map1, const uint8_t* map2, const int32_t* level_hw, const int32_t* level_stride, int32_t in_h,
                         int32_t in_w, const uint8_t* lut_dev, int32_t alpha, int32_t alpha_mode, void* stream);
/* y[i] = 1 / (1 + ore_expf(-x[i])) on the host: ore_sigmoid of the kernels, operation by operation (fmaf fused, nothing else). */
int ore_sigmoid_host(const float* x, float* y, int64_t n);
/* The geometry of the engine's last pass, for readers of its level buffers: out[0 .. 2] = B, H, W (the batch -- the class slots of an
 * N-way pass -- and the unpadded input size); out[3 + 3 l ..] = h_l, w_l, stride_l for l = 0 .. 2 (p3 .. p5); out[12], out[13] = the
 * pass serial's low 31 bits and the bits above: a count of the passes the engine has begun, so that a reader can tell that the buffers
 * it took views of have been written again.  out[14], out[15] = 0. */
int ore_engine_last_geometry(ore_engine* e, int32_t out[16]);

/* ------------------------------------------------------------------ tiled inference ----------- */
/* The device side of TiledInference (fewx/modeling/tiled_inference.py): a frame larger than one detector pass is cut into overlapping
 * tiles at native resolution, every tile (and, optionally, the resized full frame) is one source of detection rows, and the rows of all
 * sources are merged by ore_tta_merge_fwd.  Both calls are enqueued on `stream`, no host synchronisation.
 * ore_tile_gather_u8_fwd: src_hwc [h][w][3] uint8 interleaved -> dst [ny * nx][3][th][tw] uint8 planar, the image layout of
 *   ore_engine_eval_fwd / ore_engine_eval_batch_fwd with img_is_u8 = 1, in one launch.  Tile iy * nx + ix starts at y0 = min(iy *
 *   stride_y, h - th), x0 = min(ix * stride_x, w - tw) and holds exactly frame[y0 : y0 + th, x0 : x0 + tw] transposed to planar; swap_rb
 *   exchanges channels 0 and 2.  src and its rows may start at any byte; nothing outside the frame is read and nothing outside dst[0,
 *   ny * nx * 3 * th * tw) is written.  ORE_EINVAL: a side outside 1 .. 8192, th > h, tw > w, a stride outside 1 .. 8192, a grid that
 *   does not reach the far edge ((ny - 1) * stride_y < h - th, likewise x), ny * nx > 128, dst overlapping src.
 * ore_tile_collect_fwd: one source's detection rows -- boxes [n][4] xyxy in the source's own coordinates, scores [n], classes [n] int64
 *   (NULL: all 0), n = min(*n_dev if n_dev else n_host, max_rows) -- into the pool of ore_tta_merge_fwd (boxes [pool_cap][4], scores,
 *   classes int64, running count *pool_n).
 *   Seam rule, fp32, on the source-local coordinates: `edges` bit 1 = left, 2 = top, 4 = right, 8 = bottom says the source continues
 *   into the frame on that side; a row is rejected iff (edges & 1 and x0 < margin) or (edges & 2 and y0 < margin) or (edges & 4 and
 *   x1 > fl(src_w - margin)) or (edges & 8 and y1 > fl(src_h - margin)).  A comparison with NaN is false: such a row passes here and
 *   the merge drops it.
 *   Kept rows become x' = fl(fl(x * sx) + ox), y' = fl(fl(y * sy) + oy), every operation rounded on its own (a tile: sx = sy = 1, (ox,
 *   oy) its origin; the full-frame pass: ox = oy = 0, edges = 0, the ratios computed in double and rounded to fp32 by the caller), and
 *   are appended in row order (a stable compaction) at *pool_n, which the call advances; source == 0 restarts the pool at 0; rows that
 *   would pass pool_cap are cut.  src_counts[source] = the rows appended, src_dropped[source] = the rows the seam rule rejected.
 *   ORE_EINVAL: source sides outside 1 .. 8192, edges outside 0 .. 15, margin < 0 or NaN.  No float atomics: bit-reproducible. */
int ore_tile_gather_u8_fwd(const uint8_t* src_hwc, int32_t h, int32_t w, int32_t th, int32_t tw, int32_t stride_y, int32_t stride_x,
                           int32_t ny, int32_t nx, int32_t swap_rb, uint8_t* dst, void* stream);
int ore_tile_collect_fwd(const float* boxes, const float* scores, const int64_t* classes, const int32_t* n_dev, int32_t n_host,
                         int32_t max_rows, float sx, float sy, float ox, float oy, int32_t src_h, int32_t src_w, int32_t edges,
                         float margin, float* pool_boxes, float* pool_scores, int64_t* pool_classes, int32_t* pool_n, int32_t pool_cap,
                         int32_t* src_counts, int32_t* src_dropped, int32_t source, void* stream);

/* ------------------------------------------------------------------ batch canvases ------------ */
/* "batch canvas v1": the input tensors of a training step built from its raw images in one launch -- ImageList.from_tensors
 * (d2z:structures/image_list.py) behind the normalisation (ref:fewx/modeling/fsod/fsod_cen.py:540-551), for images whose sizes differ.
 * slab: the raw images of the step on the device, each planar [3][h][w] and contiguous at its own size, uint8 or fp32.  table: one row
 * of ORE_BATCH_CANVAS_JOB_INTS int32 words per image (ORE_BCJ_*): the byte offset of the image inside the slab (low, high word; an fp32
 * image at a multiple of 4), h, w, the float offset of its canvas inside `out` (low, high; a multiple of 4), and the canvas Hc, Wc.
 * Rows 0 .. n_query - 1 are the query images (canvas Hq x Wq, raw uint8 if query_u8 else raw fp32), rows n_query .. n_query +
 * n_support - 1 the support crops (Hs x Ws, support_u8); a group may be empty.  pixel_mean / pixel_std: 3 floats each on the device.
 * Canvas cell (c, y, x) of an image = (float(raw) - mean[c]) / std[c], the subtraction and the correctly rounded division each rounded
 * on its own, where y < h and x < w, and +0.0f elsewhere; planar NCHW fp32.  Sizes and offsets are read from the table ON THE DEVICE:
 * only the job counts and the canvas sizes are launch arguments, so a captured launch serves any later contents of slab and table.
 * Every cell of every canvas a valid row names is written exactly once.  Whatever the table holds, nothing outside [slab, slab +
 * slab_bytes) is read and nothing outside [out, out + out_floats) is written: a row whose canvas is not the launch's, or does not lie
 * inside `out`, is skipped; a row whose image does not lie inside the slab or its canvas gives an all-zero canvas.
 * ORE_EINVAL: slab or out not 16-byte aligned, slab_bytes no multiple of 4, no job or more than 65535, a canvas side outside 1 .. 8192
 * or a canvas width that is no multiple of 4, out_floats smaller than the canvases. */
#define ORE_BATCH_CANVAS_JOB_INTS 8
#define ORE_BCJ_SRC 0     /* byte offset inside the slab: low, high word */
#define ORE_BCJ_H 2
#define ORE_BCJ_W 3
#define ORE_BCJ_DST 4     /* float offset inside out: low, high word */
#define ORE_BCJ_HC 6
#define ORE_BCJ_WC 7
int ore_batch_canvas_fwd(const void* slab, size_t slab_bytes, const int32_t* table, int32_t n_query, int32_t Hq, int32_t Wq,
                         int32_t query_u8, int32_t n_support, int32_t Hs, int32_t Ws, int32_t support_u8,
                         const float* pixel_mean, const float* pixel_std, float* out, size_t out_floats, void* stream);

/* ------------------------------------------------------------------ rectification ------------- */
/* A fixed camera that looks at the belt obliquely sees it in perspective: the far edge moves fewer pixels per frame than the near one
 * ("belt shift v1" votes ONE translation), and box sizes are not comparable across the frame.  The remedy is to warp every frame into
 * the belt plane with the installation's constant homography before anything else looks at it.  One launch on `stream`, no host
 * synchronisation, no allocation, no table: the nine coefficients travel as kernel arguments, so the launch can be captured.
 * Contract "rectify v1" -- bit-exact, a function of the inputs alone:
 *   Inputs: a source frame S [hs][ws][3] uint8 interleaved, any channel order; nine fp32 coefficients m00 .. m22, row-major, which map
 *     a pixel centre of the OUTPUT to continuous SOURCE coordinates (pixel (i, j) covers [j, j + 1) x [i, i + 1)); the output size (ho,
 *     wo); a fill colour of 3 bytes.  All four extents lie in 1 .. ORE_RECTIFY_MAX_SIDE.
 *   Per output pixel (i, j), every operation ONE IEEE binary32 operation in this order, nothing contracted, the divisions correctly
 *   rounded:
 *     xo = float(j) + 0.5f;  yo = float(i) + 0.5f
 *     X = (m00 * xo + m01 * yo) + m02;  Y = (m10 * xo + m11 * yo) + m12;  Z = (m20 * xo + m21 * yo) + m22
 *     u = X / Z - 0.5f;  v = Y / Z - 0.5f
 *     inside <=> X, Y, Z finite and Z > 0 and -0.5f <= u <= float(ws) - 0.5f and -0.5f <= v <= float(hs) - 0.5f (a NaN is outside)
 *     not inside: the three bytes are the fill colour
 *     U = (int)floorf(u * 256.0f + 0.5f), V likewise (the product is a scaling by a power of two, exact; the sum is one binary32
 *       addition of a value below 2^23, which the limit on the extents guarantees, so its result still resolves halves and the
 *       conversion is exact: U is u rounded to the nearest 1/256, ties upwards, up to that one rounding)
 *     x0 = U >> 8 (arithmetic), fx = U & 255; y0 = V >> 8, fy = V & 255; the taps x0, x0 + 1, y0, y0 + 1 are each clamped to the source
 *     per channel, integers, with a = S[y0][x0], b = S[y0][x0 + 1], c = S[y0 + 1][x0], d = S[y0 + 1][x0 + 1]:
 *       top = a * (256 - fx) + b * fx;  bot = c * (256 - fx) + d * fx;  out = (top * (256 - fy) + bot * fy + 32768) >> 16
 *   The identity matrix returns the source byte for byte; an integer translation returns shifted bytes, with fill where the source ends.
 *   NOT in the contract: anti-aliasing.  A strongly minifying warp aliases; choose (ho, wo) near the belt region's source resolution.
 * fill_rgb: channel 0 in bits 0 .. 7, channel 1 in bits 8 .. 15, channel 2 in bits 16 .. 23 (the frame's own channel order).  src, dst
 * and their rows may start at any byte; nothing outside src[0, hs * ws * 3) is read and nothing outside dst[0, ho * wo * 3) is written.
 * ORE_EINVAL, with a message, before any launch: a null pointer, an extent outside 1 .. ORE_RECTIFY_MAX_SIDE, a coefficient that is
 * not finite, a fill outside 0 .. 0xFFFFFF, dst overlapping src. */
#define ORE_RECTIFY_MAX_SIDE 16384
int ore_rectify_u8_fwd(const uint8_t* src, int32_t hs, int32_t ws, const float m9_host[9], uint8_t* dst, int32_t ho, int32_t wo,
                       int32_t fill_rgb, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ORE_HIP_H_ */
