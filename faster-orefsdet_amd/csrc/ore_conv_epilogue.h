// The epilogue of the forward conv kernels (k_conv_igemm, k_conv3x3_patch / _patch_db / _ws, k_conv_kw, k_conv_gs, k_conv_kd,
// k_conv_gd, k_conv_rf, k_conv3x3_wino / _wino_nu).  The planner picks one of them per call, so all of them compute the same thing
// from an fp32 accumulator `acc` of pixel row m and output channel n -- in this order:
//   1. y = acc * scale[lvl * ep_stride + n] + shift[lvl * ep_stride + n]     (a null scale is 1, a null shift is 0)
//   2. y += the top-down addend of the pixel (the coarser level, read at (oy / 2, ox / 2); fp32, or bf16 where p.sb & 4)
//   3. y = max(y, 0) on the channels n < relu_cout
//   4. the lanes n >= Cout of a channel quad are zero (they take part in the column sums)
//   5. a bf16 output tensor (p.sb & 2) is rounded ONCE, here, and what the eSE column sums add is the ROUNDED value: the stored
//      tensor is the layer's output in that mode
//   6. one 16-byte (bf16: 8-byte) store of the quad where the output allows it and the quad lies inside Cout, else channel by channel
//   7. optional column sums of y over the tile's pixels (the eSE average pool), pixel lanes first, then waves / row tiles in order.
// What is NOT here, because each kernel has its own: where the scale / shift / addend operands are fetched (LDS prefetch in
// k_conv_igemm, buffer loads behind the last batch in k_conv_rf, ...), the argument blocks, the K loops, the LDS layouts.
//
// Functions and macros.  Every kernel here is on the timed path and a refactor does not move a register there, so each piece below is
// a __forceinline__ function only where every kernel's gfx950 assembly came out identical to its open-coded form
// (tools/device_asm_diff.py); the others are macros, for the reason given at CONV_WINDOW_OF_PIXEL (ore_conv_desc.h): a function is
// optimised on its own before it is inlined.  A piece that needs the macro in one kernel is a macro in all of them.
#pragma once
#include "ore_conv_internal.h"

namespace oreconv {

// Steps 1-3 for ONE channel, operands straight from memory: the slow form of k_conv_igemm, k_conv_kw and k_conv_gs (per-level
// scale / shift, an addend, or a quad that straddles Cout).  BF16_ADD: the kernel takes a bf16 addend (p.sb & 4); k_conv_igemm does
// not and instantiates <false>, which has no such branch.
template <bool BF16_ADD>
__device__ __forceinline__ float epilogue_one(const ConvP& p, float acc, int m, int n) {
    float v = acc;
    int lvl = 0, b = 0, oy = 0, ox = 0;
    if (p.ep_stride || p.add) decode_row(p, m, lvl, b, oy, ox);
    if (p.scale) v = v * p.scale[lvl * p.ep_stride + n];
    if (p.shift) v = v + p.shift[lvl * p.ep_stride + n];
    if (p.add) {
        const size_t ai = (size_t)((b * p.add_H + (oy >> 1)) * p.add_W + (ox >> 1)) * p.add_ld + p.add_coff + n;
        v += (BF16_ADD && (p.sb & 4)) ? bf16_bits_to_f32(reinterpret_cast<const unsigned short*>(p.add)[ai]) : p.add[ai];
    }
    if (n < p.relu_cout) v = fmaxf(v, 0.0f);
    return v;
}

// Step 1's operands for the channel quad n .. n + 3 of level lvl, into the f32x4 lvalues sc and sh (p: a block with scale, shift,
// ep_stride, Cout).  CONV_SCALE_SHIFT4: channel by channel, a channel beyond Cout gets the defaults; scale_shift4_vec: one 16-byte
// load each (Cout % 4 == 0).
#define CONV_SCALE_SHIFT4(p, lvl, n, sc, sh)                                                                                         \
    {                                                                                                                                \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                                              \
            (sc)[r] = ((p).scale && (n) + r < (p).Cout) ? (p).scale[(lvl) * (p).ep_stride + (n) + r] : 1.0f;                         \
            (sh)[r] = ((p).shift && (n) + r < (p).Cout) ? (p).shift[(lvl) * (p).ep_stride + (n) + r] : 0.0f;                         \
        }                                                                                                                            \
    }
template <class P>
__device__ __forceinline__ void scale_shift4_vec(const P& p, int lvl, int n, f32x4& sc, f32x4& sh) {
    sc = f32x4{1.f, 1.f, 1.f, 1.f}; sh = f32x4{0.f, 0.f, 0.f, 0.f};
    if (p.scale) sc = *reinterpret_cast<const f32x4*>(p.scale + lvl * p.ep_stride + n);
    if (p.shift) sh = *reinterpret_cast<const f32x4*>(p.shift + lvl * p.ep_stride + n);
}

// Step 3 on a quad (f32x4 lvalue v, first channel n); _X2: the two output rows of a Winograd tile; step 4 alone; steps 3 and 4.
#define CONV_RELU4(v, n, relu_cout)                                                                                                  \
    {                                                                                                                                \
        _Pragma("unroll") for (int r = 0; r < 4; ++r)                                                                                \
            if ((n) + r < (relu_cout)) (v)[r] = fmaxf((v)[r], 0.0f);                                                                 \
    }
#define CONV_RELU4_X2(v0, v1, n, relu_cout)                                                                                          \
    {                                                                                                                                \
        _Pragma("unroll") for (int r = 0; r < 4; ++r)                                                                                \
            if ((n) + r < (relu_cout)) { (v0)[r] = fmaxf((v0)[r], 0.f); (v1)[r] = fmaxf((v1)[r], 0.f); }                             \
    }
#define CONV_ZERO_PAST4(v, n, Cout)                                                                                                  \
    {                                                                                                                                \
        _Pragma("unroll") for (int r = 0; r < 4; ++r)                                                                                \
            if ((n) + r >= (Cout)) (v)[r] = 0.0f;                                                                                    \
    }
#define CONV_RELU_ZERO4(v, n, relu_cout, Cout)                                                                                       \
    {                                                                                                                                \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                                              \
            if ((n) + r < (relu_cout)) (v)[r] = fmaxf((v)[r], 0.0f);                                                                 \
            if ((n) + r >= (Cout)) (v)[r] = 0.0f;                                                                                    \
        }                                                                                                                            \
    }

// Step 6's "the output allows it": channel stride and slice offset in whole quads, the base aligned to a quad of the storage type
// (p: a block with out, out_ld, out_coff; out_bf16: p.sb & 2, or false in a kernel without bf16 output).
#define CONV_OUT_VEC_OK(p, out_bf16)                                                                                                 \
    (((p).out_ld & 3) == 0 && ((p).out_coff & 3) == 0 && ((uintptr_t)(p).out & ((out_bf16) ? 7 : 15)) == 0)

// Step 6: quad v (first channel n) to o, a float* / unsigned short* to channel n of the pixel.  The bf16 twin is step 5 as well: it
// leaves the rounded values in v.
#define CONV_STORE4_F32(o, v, vec_ok, n, Cout)                                                                                       \
    {                                                                                                                                \
        if ((vec_ok) && (n) + 3 < (Cout)) {                                                                                          \
            *reinterpret_cast<f32x4*>(o) = (v);                                                                                      \
        } else {                                                                                                                     \
            _Pragma("unroll") for (int r = 0; r < 4; ++r)                                                                            \
                if ((n) + r < (Cout)) (o)[r] = (v)[r];                                                                               \
        }                                                                                                                            \
    }
#define CONV_STORE4_BF16(o, v, vec_ok, n, Cout)                                                                                      \
    {                                                                                                                                \
        const s16x4 h = to_bf16x4(v);                                                                                                \
        unsigned short* o_ = (o);                                                                                                    \
        if ((vec_ok) && (n) + 3 < (Cout)) {                                                                                          \
            *reinterpret_cast<s16x4*>(o_) = h;                                                                                       \
        } else {                                                                                                                     \
            _Pragma("unroll") for (int r = 0; r < 4; ++r)                                                                            \
                if ((n) + r < (Cout)) o_[r] = (unsigned short)h[r];                                                                  \
        }                                                                                                                            \
        (v) = from_bf16x4(h);                                                                                                        \
    }

// Step 7, pixel lanes: an accumulator tile keeps the 16 pixels of a channel quad in the lanes that differ in bits 0-3, so xor 1, 2, 4,
// 8 leaves every lane with the quad's sum over the tile's 16 rows (f32x4 lvalue v).
#define CONV_COLSUM16(v)                                                                                                             \
    {                                                                                                                                \
        _Pragma("unroll") for (int d = 1; d < 16; d <<= 1)                                                                           \
            _Pragma("unroll") for (int r = 0; r < 4; ++r) (v)[r] += __shfl_xor((v)[r], d);                                           \
    }

// The in-block K split: wave g parked its partial 16x16 tile tl at red[(g * NT + tl) * 256 + lane * 4]; lane ln's quad of the sum
// of the NW waves, added in wave order (bitwise deterministic), into the f32x4 lvalue a.
#define CONV_SUM_WAVE_TILES(a, NW, red, NT, tl, ln)                                                                                  \
    {                                                                                                                                \
        (a) = *reinterpret_cast<const f32x4*>((red) + (0 * (NT) + (tl)) * 256 + (ln) * 4);                                           \
        _Pragma("unroll") for (int g = 1; g < (NW); ++g) (a) += *reinterpret_cast<const f32x4*>((red) + (g * (NT) + (tl)) * 256 + (ln) * 4); \
    }

}  // namespace oreconv
