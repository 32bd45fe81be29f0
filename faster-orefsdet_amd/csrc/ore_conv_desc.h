// The descriptor-addressing layer of the buffer-descriptor conv kernels (k_conv_rf, k_conv_kd, k_conv_gd): what a kernel of this
// family needs to turn "row m of the implicit GEMM, chunk c of K" into a range-checked buffer load, and what its launcher needs to fill
// the argument block and the chunk table.  k_conv_kw takes wait_vmcnt and swz from here.  For the kernels' translation units only: the
// planner stays free of device code and does not include this header (the limits it shares with the kernels -- kOOB, the table sizes --
// are in ore_conv_internal.h).
//
// The scheme.  Every operand is read through a buffer descriptor whose num_records is the tensor's size in bytes.  The per-lane byte
// offset of a pixel row / weight row is computed ONCE per block; a K step adds a scalar offset (3x3 layers: from the chunk table in the
// kernel arguments, built by the host) or an instruction offset (weights, 1x1 layers).  Out-of-image taps, rows beyond M / Cout and
// chunks beyond K get the per-lane offset kOOB and are the descriptor's out-of-range zeros: no zero page, no 64-bit pointer select, no
// tap walk, no branch in the issue loop.  The hardware range-checks voffset + instruction offset only; the scalar offset is added
// behind the check, so a step beyond K must be killed through the per-lane offset, never through its scalar offset.
//
// An argument block K (RfK, KdK, GdK; each kernel keeps its own, the layouts differ in their tails) has these fields in common:
//   in, w, scale, shift, add, out, colsum; in_bytes, w_bytes, sc_bytes, add_bytes (num_records); M, K, Cout, Cout16, nchunks;
//   irow0, H, W, Ho, Wo, in_ld, in_coff, stride, pad; out_ld, out_coff, relu_cout; add_H, add_W, add_ld, add_coff (the FPN top-down
//   addend [B][add_H][add_W][add_ld], read at (oy / 2, ox / 2)); xmap, gx, gy; inv_hw, inv_wo, inv_gx, inv_gy (host-made reciprocals).
// Every scalar the kernel needs is in that block, compact and in ONE place, so that they arrive with a handful of wide scalar loads
// issued together at the top (hipcc otherwise fetches the fields of a big by-value struct one `s_load` + `s_waitcnt lgkmcnt(0)` at a
// time, next to their first use: fourteen serial round trips = most of the 2300-4600 clocks of prologue the traces show).
#pragma once
#include "ore_conv_internal.h"

namespace oreconv {

// ---- the chunk table of a 3x3 layer: per 16-channel chunk c of the K axis, the byte offset of its (tap, channel chunk) from the
// window's first pixel -- the scalar offset of the step -- and the tap index 0..8 in four spare bits; chunks beyond K carry tap 15
// (never valid).  Built on the host per launch and passed BY VALUE (kernel argument segment -> scalar loads): the issue loop of a wave
// has no tap arithmetic at all.  Two encodings:
struct ChunkFmt { int tap_shift; unsigned off_mask; };
constexpr ChunkFmt kChunkTapLow = {0, ~63u};           // k_conv_rf, k_conv_gd: the offset is a multiple of 64, the tap rides in bits 0-3
constexpr ChunkFmt kChunkTapHigh = {28, 0x0fffffffu};  // k_conv_kd: tap in bits 28-31 (a bf16 pixel pitch need not be a multiple of 64)
constexpr unsigned kNoTap = 15u;
__host__ __device__ __forceinline__ constexpr unsigned chunk_entry(ChunkFmt f, unsigned off, unsigned tap) { return off | (tap << f.tap_shift); }
__host__ __device__ __forceinline__ constexpr unsigned chunk_tap(ChunkFmt f, unsigned e) { return (e >> f.tap_shift) & 15u; }
__host__ __device__ __forceinline__ constexpr unsigned chunk_off(ChunkFmt f, unsigned e) { return e & f.off_mask; }

// =====================================================================================================================================
// device side
// =====================================================================================================================================

// (make_rsrc, the descriptor itself, is in ore_common.h: the weight-gradient kernels of ore_conv_wgrad.hip use it too)
// 16 bytes per lane into registers: base + voff (range-checked) + soff (not checked)
__device__ __forceinline__ f32x4 bload(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0));
}
__device__ __forceinline__ f32x4 bload4(__amdgpu_buffer_rsrc_t r, unsigned voff) { return bload(r, voff, 0u); }
// one LDS-DMA piece: 64 lanes x 16 bytes -> 1 KiB at `dst` (lane-linear), source = base + voff + soff + IMM.  The instruction offset
// of a buffer load with the LDS flag is added to the LDS address as well as to the memory address (LDS address = M0 + offset + lane * 16),
// so M0 is handed dst - IMM: the step rides in the instruction on the memory side and cancels on the LDS side.
template <int IMM>
__device__ __forceinline__ void dma(__amdgpu_buffer_rsrc_t r, float* dst, unsigned voff, unsigned soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)(dst - IMM / 4), 16, (int)voff, (int)soff, IMM, 0);
}
// n / d for 0 <= n < 2^22, d > 0, with inv = 1.0f / d: one multiply, one conversion and two corrections instead of ~40 instructions
__device__ __forceinline__ int fdiv(int n, int d, float inv) {
    int q = (int)((float)n * inv);
    int r = n - q * d;
    q += r >= d ? 1 : 0;
    r -= r >= d ? d : 0;
    q -= r < 0 ? 1 : 0;
    return q;
}
template <int N> __device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0 && N <= 63, "vmcnt immediate");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// XOR swizzle of the four 16-byte quads of a 64-byte row inside a 16-row group: with q' = q ^ SW[(r >> 2) & 3] every ds_read_b128
// lane group (rows {0-3, 12-15} of quad q with rows 4-11 of quad q+1, and its mirror) touches 16 distinct 4-bank groups.  Applied to
// the SOURCE offset of each DMA lane and, identically, to the fragment read.
__device__ __forceinline__ int swz(int r16) { return (0x1320 >> (((r16 >> 2) & 3) * 4)) & 3; }   // {0, 2, 3, 1}

// Which tile does this block compute: tile_of_block (ore_conv_internal.h) with the host-made reciprocals of the argument block.
// tile_of_block itself stays for k_conv_kw / k_conv_igemm / the patch kernels, whose ConvP argument carries no reciprocals and whose
// device code an fdiv in place of the integer division would change.
template <class K>
__device__ __forceinline__ void tile_of_block_rcp(const K& k, int& bx, int& by) {
    bx = blockIdx.x; by = blockIdx.y;
    if (k.xmap == 0) return;
    const int T = k.gx * k.gy;
    const int lin = by * k.gx + bx, r = lin & 7, kk = lin >> 3;
    const int qd = T >> 3, rem = T & 7;
    const int t = r * qd + min(r, rem) + kk;
    if (k.xmap == 1) { bx = fdiv(t, k.gy, k.inv_gy); by = t - bx * k.gy; }
    else { by = fdiv(t, k.gx, k.inv_gx); bx = t - by * k.gx; }
}

// row m of the GEMM -> image and output pixel, by fdiv.  hw = k.Ho * k.Wo: the kernel computes it once, ahead of its branches on m.
struct Pixel { int b, oy, ox; };
template <class K>
__device__ __forceinline__ Pixel pixel_of_row(const K& k, int m, int hw) {
    Pixel x;
    x.b = fdiv(m, hw, k.inv_hw);
    const int rr = m - x.b * hw;
    x.oy = fdiv(rr, k.Wo, k.inv_wo);
    x.ox = rr - x.oy * k.Wo;
    return x;
}

// The pixel descriptor starts window_bias bytes BEFORE the tensor, so that the per-lane offset of the window's first pixel (which lies
// above / left of the image for border rows) is never negative; a valid tap's scalar offset brings the address back inside the tensor,
// an invalid tap never leaves the range check.
template <class K> __device__ __forceinline__ int window_bias(const K& k) {
    const int row_bytes = k.W * k.in_ld * 4, pix_bytes = k.in_ld * 4;
    return k.pad * (row_bytes + pix_bytes);
}
template <class K> __device__ __forceinline__ __amdgpu_buffer_rsrc_t make_pixel_rsrc(const K& k, int bias) {
    return make_rsrc(reinterpret_cast<const char*>(k.in) - bias, k.in_bytes + (unsigned)bias);
}

// The KS x KS window of pixel px (a Pixel) as this lane reads it, into two unsigned lvalues: taps = bit dy * KS + dx set where that tap
// lies inside the image, voff = bias (window_bias) + byte offset of the window's first pixel at channel in_coff + 4 * quad.  The
// caller presets a row beyond M to no tap and voff = kOOB.
// A macro, not a function: a function is optimised on its own before it is inlined (the address sum is re-associated, the blocks of
// the two loops are merged in another order), and the kernels' device code then differs from the hand-written form in scheduling and
// register numbers although the arithmetic is the same.  Textual substitution keeps it bit-identical.
#define CONV_WINDOW_OF_PIXEL(KS, k, px, quad, bias, taps, voff)                                                                      \
    {                                                                                                                                \
        const int iy0 = (px).oy * (k).stride - (k).pad, ix0 = (px).ox * (k).stride - (k).pad;                                        \
        unsigned rmask = 0u, cmask = 0u, tm = 0u;                                                                                    \
        _Pragma("unroll") for (int d = 0; d < (KS); ++d) {                                                                           \
            rmask |= (unsigned)(iy0 + d) < (unsigned)(k).H ? 1u << d : 0u;                                                           \
            cmask |= (unsigned)(ix0 + d) < (unsigned)(k).W ? 1u << d : 0u;                                                           \
        }                                                                                                                            \
        _Pragma("unroll") for (int d = 0; d < (KS); ++d) tm |= ((rmask >> d) & 1u) ? cmask << (d * (KS)) : 0u;                       \
        (taps) = tm;                                                                                                                 \
        (voff) = (unsigned)((bias) + ((((k).irow0 + (px).b * (k).H * (k).W) + iy0 * (k).W + ix0) * (k).in_ld + (k).in_coff + (quad) * 4) * 4); \
    }

// element index of channel n of the top-down addend of a pixel: the coarser level, nearest-neighbour upsampled
// (d2z:modeling/backbone/fpn.py:140-144)
template <class K>
__device__ __forceinline__ int addend_index(const K& k, Pixel x, int n) {
    return ((x.b * k.add_H + (x.oy >> 1)) * k.add_W + (x.ox >> 1)) * k.add_ld + k.add_coff + n;
}

// Phase-timeline stamps (make trace; tools/conv_phase_trace.py): thread 0 of every block stamps s_memtime (shader clocks; CONV_TRR:
// s_memrealtime, 100 MHz, comparable across blocks) into sym[block][16].  CONV_TRACE_SYMBOL(sym) declares the buffer pointer (inside
// the kernel's namespace), CONV_TRACE_SETTER(fn, sym) the extern "C" function that sets it (at file scope).  Never in the product library.
#ifdef ORE_TRACE
#define CONV_TRACE_SYMBOL(sym) __device__ unsigned long long* sym = nullptr;
#define CONV_TRACE_SETTER(fn, sym) \
    extern "C" int fn(unsigned long long* buf) { ORE_HIP(hipMemcpyToSymbol(HIP_SYMBOL(sym), &buf, sizeof(buf))); return ORE_OK; }
#define CONV_TR_(sym, i, clock) do { if (sym && threadIdx.x == 0) sym[(size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 16 + (i)] = clock(); } while (0)
#define CONV_TR(sym, i) CONV_TR_(sym, i, __builtin_amdgcn_s_memtime)
#define CONV_TRR(sym, i) CONV_TR_(sym, i, __builtin_amdgcn_s_memrealtime)
#else
#define CONV_TRACE_SYMBOL(sym)
#define CONV_TRACE_SETTER(fn, sym)
#define CONV_TR(sym, i) do { } while (0)
#define CONV_TRR(sym, i) do { } while (0)
#endif

// =====================================================================================================================================
// host side
// =====================================================================================================================================

// Every field the argument blocks share, from the call and its plan.  L returns the level the kernel sees -- several levels of a 1x1
// layer run as one flat GEMM: one "image" of M pixels in a row -- for the chunk table.  What is a kernel's own (nb, sb, zc_stride /
// out_zstride, dbg) is the launcher's to set.
template <class K>
void fill_desc_args(K& k, const ConvP& p, const ConvPlan& pl, Lvl& L) {
    L = p.lv[0];
    int Bimg = p.B;
    if (p.nlev > 1) { L.H = 1; L.W = p.M; L.Ho = 1; L.Wo = p.M; Bimg = 1; }
    k.in = p.in; k.w = p.w; k.scale = p.scale; k.shift = p.shift; k.add = p.add; k.out = p.out; k.colsum = p.colsum;
    k.in_bytes = (unsigned)(((long long)L.irow0 + (long long)Bimg * L.H * L.W) * p.in_ld * 4);
    k.w_bytes = (unsigned)((long long)p.Cout16 * p.K * 4);
    k.sc_bytes = (unsigned)p.Cout * 4u;
    k.add_bytes = p.add ? (unsigned)((long long)p.B * p.add_H * p.add_W * p.add_ld * ((p.sb & 4) ? 2 : 4)) : 0u;
    k.M = p.M; k.K = p.K; k.Cout = p.Cout; k.Cout16 = p.Cout16; k.nchunks = p.nchunks;
    k.irow0 = L.irow0; k.H = L.H; k.W = L.W; k.Ho = L.Ho; k.Wo = L.Wo; k.in_ld = p.in_ld; k.in_coff = p.in_coff; k.stride = p.stride; k.pad = p.pad;
    k.out_ld = p.out_ld; k.out_coff = p.out_coff; k.relu_cout = p.relu_cout;
    k.add_H = p.add_H; k.add_W = p.add_W; k.add_ld = p.add_ld; k.add_coff = p.add_coff;
    k.xmap = pl.xmap; k.gx = pl.gx; k.gy = pl.gy;
    k.inv_hw = 1.0f / (float)(L.Ho * L.Wo); k.inv_wo = 1.0f / (float)L.Wo; k.inv_gx = 1.0f / (float)pl.gx; k.inv_gy = 1.0f / (float)pl.gy;
}

// The chunk table of a launch (n entries, format f): a 3x3 layer's chunks, tap-major, then "no tap"; a 1x1 layer reads none of it.
inline void build_chunk_table(unsigned* tab, int n, const ConvP& p, const Lvl& L, ChunkFmt f) {
    for (int c = 0; c < n; ++c) tab[c] = chunk_entry(f, 0u, kNoTap);
    if (p.kh != 3) return;
    const int cpt = p.Cin >> 4, row_bytes = L.W * p.in_ld * 4, pix_bytes = p.in_ld * 4;
    for (int c = 0; c < p.nchunks && c < n; ++c) {
        const int tap = c / cpt, cc = c - tap * cpt, dy = tap / 3, dx = tap - dy * 3;
        tab[c] = chunk_entry(f, (unsigned)(dy * row_bytes + dx * pix_bytes + cc * 64), (unsigned)tap);
    }
}

}  // namespace oreconv
