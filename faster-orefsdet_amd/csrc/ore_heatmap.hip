// Heat maps of a detection pass ("heatmap v1", include/ore_hip.h): a scalar per pyramid location -- a channel or the channel mean of a
// level buffer, optionally through the decode's sigmoid -- quantised to uint8, resampled to the frame with integer bilinear taps, merged
// across levels by max, coloured through a 256-entry table and blended over an interleaved [h][w][3] uint8 frame.  Everything is
// enqueued on the caller's stream: no host wait, no allocation.
//   k_heatmap_scalar  stages A + B, one thread per location of every level (grid-stride over at most 256 blocks).  norm "unit" writes
//                     the uint8 map at once; norm "max" keeps the fp32 scalar and leaves one maximum per block: an integer max over
//                     the bits of the non-negative floats, in LDS -- no float atomics, no dependence on block order.
//   k_heatmap_quant   norm "max" only: every block reduces the (at most 256) block maxima to m and quantises v / m.
//   k_heatmap_render  stages C + D, 256 threads x 4 pixels over the frame as one flat run of pixels (4 pixels = 3 dwords at any width).
//                     A thread divides once per level and axis (64-bit numerator) and steps the quotient and remainder from pixel to
//                     pixel; the taps are read through L1 / L2 (the maps of a 1000 x 1333 input are under 28 KB; staging a block's
//                     map rows in LDS measured slower: profiles/heatmap_lds_ab.txt), the table sits in LDS as one packed word per
//                     entry.  Each pixel is read once and written once.
// All pixel arithmetic is integer.  Compiled with -ffp-contract=off: ore_sigmoid and its host twin are the same single operations.
#include <math.h>
#include <string.h>
#include "ore_block.h"

namespace {

constexpr int HM_T = 256, HM_PX = 4;               // render block: 256 threads x 4 pixels
constexpr int HM_MAX_PARTS = 256;                  // blocks of k_heatmap_scalar = block maxima k_heatmap_quant reduces
constexpr int HM_LEVELS = ORE_HEATMAP_MAX_LEVELS;

struct Layout { size_t map[HM_LEVELS], parts, scalar, total; };
inline Layout heatmap_layout(int n, const int32_t* hw) {
    Layout o{};
    size_t a = 0, locs = 0;
    for (int l = 0; l < n; ++l) {
        const size_t c = (size_t)hw[2 * l] * (size_t)hw[2 * l + 1];
        o.map[l] = a; a += (c + 255) & ~(size_t)255;
        locs += c;
    }
    o.parts = a; a += HM_MAX_PARTS * sizeof(uint32_t);
    o.scalar = a; a += (locs * sizeof(float) + 255) & ~(size_t)255;
    o.total = a;
    return o;
}
bool dims_ok(int n, const int32_t* hw) {
    if (n < 1 || n > HM_LEVELS || !hw) return false;
    for (int l = 0; l < n; ++l)
        if (hw[2 * l] < 1 || hw[2 * l] > ORE_HEATMAP_MAX_MAP_SIDE || hw[2 * l + 1] < 1 || hw[2 * l + 1] > ORE_HEATMAP_MAX_MAP_SIDE) return false;
    return true;
}

struct ScalarArgs {
    int32_t n_levels, total;                       // locations of all levels
    const void* src[HM_LEVELS];                    // row 0 of the chosen batch slot
    int32_t count[HM_LEVELS], ld[HM_LEVELS], coff[HM_LEVELS];
    int32_t ch, channel, sigmoid, norm_max;        // channel < 0: the mean over ch channels
    uint8_t* map[HM_LEVELS];
    float* scalar; uint32_t* parts;
};

// (int)(clamp(v, 0, 1) * 255.0f): fmaxf / fminf return the other operand of a NaN, so a NaN quantises to 0
__device__ __forceinline__ uint32_t quantise(float v) { return (uint32_t)(int)(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f); }

template <typename T>
__global__ __launch_bounds__(HM_T) void k_heatmap_scalar(const ScalarArgs a) {
    __shared__ uint32_t s_max;
    if (threadIdx.x == 0) s_max = 0u;
    __syncthreads();
    uint32_t best = 0u;
    for (int i = blockIdx.x * HM_T + threadIdx.x; i < a.total; i += gridDim.x * HM_T) {
        int l = 0, j = i;
        while (l + 1 < a.n_levels && j >= a.count[l]) { j -= a.count[l]; ++l; }
        const T* row = static_cast<const T*>(a.src[l]) + (size_t)j * a.ld[l] + a.coff[l];
        float v;
        if (a.channel >= 0) {
            v = ld1(row + a.channel);
        } else {                                   // four partial sums over c % 4 == j, ascending; (s0 + s1) + (s2 + s3); / C
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
            for (int c = 0; c < a.ch; c += 4) {
                const f32x4 x = ld4(row + c);
                s.x += x.x; s.y += x.y; s.z += x.z; s.w += x.w;
            }
            v = ((s.x + s.y) + (s.z + s.w)) / (float)a.ch;
        }
        if (a.sigmoid) v = ore_sigmoid(v);
        if (a.norm_max) {
            a.scalar[i] = v;
            const float m = fmaxf(v, 0.0f);        // NaN -> 0; -0.0 must not count with its sign bit
            best = max(best, m > 0.0f ? __float_as_uint(m) : 0u);
        } else {
            a.map[l][j] = (uint8_t)quantise(v);
        }
    }
    if (a.norm_max) {
        atomicMax(&s_max, best);                   // integer max in LDS: order-free
        __syncthreads();
        if (threadIdx.x == 0) a.parts[blockIdx.x] = s_max;
    }
}

struct QuantArgs {
    int32_t n_levels, total, n_parts;
    int32_t count[HM_LEVELS];
    uint8_t* map[HM_LEVELS];
    const float* scalar; const uint32_t* parts;
};

__global__ __launch_bounds__(HM_T) void k_heatmap_quant(const QuantArgs a) {
    __shared__ uint32_t s_max;
    if (threadIdx.x == 0) s_max = 0u;
    __syncthreads();
    if ((int)threadIdx.x < a.n_parts) atomicMax(&s_max, a.parts[threadIdx.x]);
    __syncthreads();
    const float m = __uint_as_float(s_max);
    const int i = blockIdx.x * HM_T + threadIdx.x;
    if (i >= a.total) return;
    int l = 0, j = i;
    while (l + 1 < a.n_levels && j >= a.count[l]) { j -= a.count[l]; ++l; }
    a.map[l][j] = m > 0.0f ? (uint8_t)quantise(a.scalar[i] / m) : (uint8_t)0;
}

// one axis of one level: position = floor(((2 t + 1) * in * 128) / (out * stride)) = (n0 + t * step) / d, kept as quotient and remainder
struct Axis { uint32_t d, n0, step, q0, r0, sq, sr; int32_t hi; };   // (q0, r0) at t = 0; (sq, sr) = step / d, step % d; hi = (len - 1) * 256
struct RenderArgs {
    int32_t h, w, n_levels, alpha, by_value;
    const uint8_t* map[HM_LEVELS]; int32_t mw[HM_LEVELS];
    Axis ax[HM_LEVELS], ay[HM_LEVELS];
};

__device__ __forceinline__ void axis_at(const Axis& a, uint32_t t, uint32_t& q, uint32_t& r) {
    const unsigned long long n = (unsigned long long)a.n0 + (unsigned long long)t * a.step;   // < 2^36
    const unsigned long long qq = n / a.d;
    q = (uint32_t)qq; r = (uint32_t)(n - qq * a.d);
}
__device__ __forceinline__ void axis_step(const Axis& a, uint32_t& q, uint32_t& r) {
    q += a.sq; r += a.sr;
    if (r >= a.d) { r -= a.d; ++q; }
}
__device__ __forceinline__ int axis_pos(const Axis& a, uint32_t q) { return min(max((int)q - 128, 0), a.hi); }


__global__ __launch_bounds__(HM_T) void k_heatmap_render(const RenderArgs a, const uint8_t* src, uint8_t* dst, const uint8_t* __restrict__ lut) {
    __shared__ uint32_t s_lut[256];                // entry k: channel c in byte c
    const int tid = threadIdx.x;
    s_lut[tid] = lut[tid * 3] | ((uint32_t)lut[tid * 3 + 1] << 8) | ((uint32_t)lut[tid * 3 + 2] << 16);
    __syncthreads();
    const unsigned npix = (unsigned)a.h * (unsigned)a.w;          // <= 8192 * 8192 = 2^26
    const unsigned p0 = blockIdx.x * (unsigned)(HM_T * HM_PX) + (unsigned)tid * HM_PX;
    if (p0 >= npix) return;
    const int cnt = (int)min((unsigned)HM_PX, npix - p0);
    int y = (int)(p0 / (unsigned)a.w), x = (int)(p0 - (unsigned)y * a.w);
    uint32_t qx[HM_LEVELS], rx[HM_LEVELS], qy[HM_LEVELS], ry[HM_LEVELS];
#pragma unroll
    for (int l = 0; l < HM_LEVELS; ++l)
        if (l < a.n_levels) { axis_at(a.ax[l], (uint32_t)x, qx[l], rx[l]); axis_at(a.ay[l], (uint32_t)y, qy[l], ry[l]); }
    uint32_t val[HM_PX];
#pragma unroll
    for (int j = 0; j < HM_PX; ++j) {
        uint32_t v = 0u;
        if (j < cnt) {
#pragma unroll
            for (int l = 0; l < HM_LEVELS; ++l) {
                if (l >= a.n_levels) continue;
                const int U = axis_pos(a.ax[l], qx[l]), V = axis_pos(a.ay[l], qy[l]);
                const int x0 = U >> 8, fx = U & 255, y0 = V >> 8, fy = V & 255;
                const int x1 = min(x0 + 1, a.ax[l].hi >> 8), y1 = min(y0 + 1, a.ay[l].hi >> 8);
                const uint8_t* r0 = a.map[l] + (size_t)y0 * a.mw[l];
                const uint8_t* r1 = a.map[l] + (size_t)y1 * a.mw[l];
                const uint32_t top = (uint32_t)r0[x0] * (256 - fx) + (uint32_t)r0[x1] * fx;
                const uint32_t bot = (uint32_t)r1[x0] * (256 - fx) + (uint32_t)r1[x1] * fx;
                v = max(v, (top * (256 - fy) + bot * fy + 32768u) >> 16);
            }
            if (++x == a.w) {                                     // the run goes on in the next row
                x = 0; ++y;
#pragma unroll
                for (int l = 0; l < HM_LEVELS; ++l)
                    if (l < a.n_levels) { qx[l] = a.ax[l].q0; rx[l] = a.ax[l].r0; axis_step(a.ay[l], qy[l], ry[l]); }
            } else {
#pragma unroll
                for (int l = 0; l < HM_LEVELS; ++l)
                    if (l < a.n_levels) axis_step(a.ax[l], qx[l], rx[l]);
            }
        }
        val[j] = v;
    }
    uint32_t col[HM_PX], al[HM_PX];
#pragma unroll
    for (int j = 0; j < HM_PX; ++j) {
        col[j] = s_lut[val[j]];
        al[j] = a.by_value ? ((uint32_t)a.alpha * val[j] + 127u) / 255u : (uint32_t)a.alpha;
    }
    const size_t off = (size_t)p0 * 3;
    if (cnt == HM_PX) {                                           // 4 pixels = 3 whole dwords, aligned at any width
        const uint32_t* s = reinterpret_cast<const uint32_t*>(src + off);
        const uint32_t d0 = s[0], d1 = s[1], d2 = s[2];
        uint32_t b[12] = {d0 & 255u, (d0 >> 8) & 255u, (d0 >> 16) & 255u, d0 >> 24, d1 & 255u, (d1 >> 8) & 255u,
                          (d1 >> 16) & 255u, d1 >> 24, d2 & 255u, (d2 >> 8) & 255u, (d2 >> 16) & 255u, d2 >> 24};
#pragma unroll
        for (int k = 0; k < 12; ++k) b[k] = blend8(b[k], (col[k / 3] >> (8 * (k % 3))) & 255u, al[k / 3]);
        uint32_t* d = reinterpret_cast<uint32_t*>(dst + off);
        d[0] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        d[1] = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
        d[2] = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
    } else {                                                      // the last 1 .. 3 pixels of the frame, byte by byte
        for (int j = 0; j < cnt; ++j)
            for (int k = 0; k < 3; ++k) {
                const size_t o = off + (size_t)j * 3 + k;
                dst[o] = (uint8_t)blend8(src[o], (col[j] >> (8 * k)) & 255u, al[j]);
            }
    }
}

Axis make_axis(int in, int out, int stride, int len) {
    Axis a{};
    a.d = (uint32_t)out * (uint32_t)stride;                       // <= 8192 * 128 = 2^20
    a.n0 = (uint32_t)in * 128u;                                   // <= 2^21
    a.step = (uint32_t)in * 256u;
    a.q0 = a.n0 / a.d; a.r0 = a.n0 % a.d;
    a.sq = a.step / a.d; a.sr = a.step % a.d;
    a.hi = (len - 1) * 256;
    return a;
}

// ore_expf / ore_sigmoid of ore_common.h on the host: the same single operations, std::fmaf for fmaf
float expf_host(float x) {
    if (x != x) return x;                          // NaN in, NaN out (the device's conversion of a NaN is defined, the host's is not)
    if (x > 88.0f) x = 88.0f;
    if (x < -87.0f) x = -87.0f;
    const float n = rintf(x * 1.44269504088896341f);
    float r = fmaf(n, -0.693359375f, x);
    r = fmaf(n, 2.12194440e-4f, r);
    float p = 1.9875691500e-4f;
    p = fmaf(p, r, 1.3981999507e-3f);
    p = fmaf(p, r, 8.3334519073e-3f);
    p = fmaf(p, r, 4.1665795894e-2f);
    p = fmaf(p, r, 1.6666665459e-1f);
    p = fmaf(p, r, 5.0000001201e-1f);
    const float e = fmaf(p, r * r, r) + 1.0f;
    const uint32_t bits = (uint32_t)((int)n + 127) << 23;
    float s;
    memcpy(&s, &bits, sizeof(s));
    return e * s;
}

}  // namespace

extern "C" int ore_sigmoid_host(const float* x, float* y, int64_t n) {
    ORE_CHECK_ARG((x && y) || n == 0, "ore_sigmoid_host: null pointer");
    ORE_CHECK_ARG(n >= 0, "ore_sigmoid_host: n %lld", (long long)n);
    for (int64_t i = 0; i < n; ++i) y[i] = 1.0f / (1.0f + expf_host(-x[i]));
    return ORE_OK;
}

extern "C" size_t ore_heatmap_workspace_bytes(int32_t n_levels, const int32_t* level_hw) {
    return dims_ok(n_levels, level_hw) ? heatmap_layout(n_levels, level_hw).total : 0;
}

extern "C" size_t ore_heatmap_level_offset(int32_t n_levels, const int32_t* level_hw, int32_t level) {
    return dims_ok(n_levels, level_hw) && level >= 0 && level < n_levels ? heatmap_layout(n_levels, level_hw).map[level] : 0;
}

extern "C" int ore_heatmap_levels_fwd(int32_t n_levels, const void* src0, const void* src1, const void* src2, const int32_t* level_hw,
                                      const int32_t* level_ld, const int32_t* level_coff, int32_t ch, int32_t is_bf16, int32_t batch,
                                      int32_t slot, int32_t channel, int32_t transform, int32_t norm, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    ORE_CHECK_ARG(dims_ok(n_levels, level_hw), "ore_heatmap_levels_fwd: 1 .. %d levels, map sides 1 .. %d", HM_LEVELS, ORE_HEATMAP_MAX_MAP_SIDE);
    ORE_CHECK_ARG(level_ld && level_coff && workspace, "ore_heatmap_levels_fwd: null pointer");
    ORE_CHECK_ARG(ch >= 1 && channel >= ORE_HEATMAP_MEAN && channel < ch, "ore_heatmap_levels_fwd: channel %d of %d (ORE_HEATMAP_MEAN or 0 .. ch - 1)", channel, ch);
    ORE_CHECK_ARG(batch >= 1 && slot >= 0 && slot < batch, "ore_heatmap_levels_fwd: batch slot %d of %d", slot, batch);
    ORE_CHECK_ARG((transform == ORE_HEATMAP_IDENTITY || transform == ORE_HEATMAP_SIGMOID) && (norm == ORE_HEATMAP_UNIT || norm == ORE_HEATMAP_MAX),
                  "ore_heatmap_levels_fwd: transform %d, norm %d", transform, norm);
    const bool mean = channel == ORE_HEATMAP_MEAN;
    ORE_CHECK_ARG(!mean || ch % 4 == 0, "ore_heatmap_levels_fwd: the channel mean takes a channel count that is a multiple of 4, not %d", ch);
    const void* srcs[HM_LEVELS] = {src0, src1, src2};
    const size_t esz = is_bf16 ? 2 : 4;
    const Layout lay = heatmap_layout(n_levels, level_hw);
    if (workspace_bytes < lay.total) {
        ore_set_error("ore_heatmap_levels_fwd: workspace %zu < %zu", workspace_bytes, lay.total);
        return ORE_ENOMEM;
    }
    char* ws = static_cast<char*>(workspace);
    ScalarArgs s{};
    QuantArgs q{};
    long long total = 0;
    for (int l = 0; l < n_levels; ++l) {
        const long long cnt = (long long)level_hw[2 * l] * level_hw[2 * l + 1];
        ORE_CHECK_ARG(srcs[l], "ore_heatmap_levels_fwd: level %d has no source", l);
        ORE_CHECK_ARG(level_coff[l] >= 0 && level_ld[l] >= level_coff[l] + ch, "ore_heatmap_levels_fwd: level %d: %d channels at %d do not fit ld %d", l, ch,
                      level_coff[l], level_ld[l]);
        ORE_CHECK_ARG(cnt * batch <= 0x7fffffffLL, "ore_heatmap_levels_fwd: level %d has too many rows", l);
        const char* base = static_cast<const char*>(srcs[l]) + (size_t)slot * (size_t)cnt * (size_t)level_ld[l] * esz;
        // the mean reads 4 channels at a time (16 bytes fp32, 8 bytes bf16)
        ORE_CHECK_ARG(!mean || (level_ld[l] % 4 == 0 && level_coff[l] % 4 == 0 && (uintptr_t)base % (4 * esz) == 0),
                      "ore_heatmap_levels_fwd: level %d: the channel mean needs ld, coff multiples of 4 and rows aligned to 4 elements", l);
        s.src[l] = base; s.count[l] = q.count[l] = (int32_t)cnt; s.ld[l] = level_ld[l]; s.coff[l] = level_coff[l];
        s.map[l] = q.map[l] = (uint8_t*)(ws + lay.map[l]);
        total += cnt;
    }
    s.n_levels = q.n_levels = n_levels;
    s.total = q.total = (int32_t)total;                           // <= 3 * 4096^2
    s.ch = ch; s.channel = channel; s.sigmoid = transform == ORE_HEATMAP_SIGMOID; s.norm_max = norm == ORE_HEATMAP_MAX;
    s.scalar = (float*)(ws + lay.scalar); s.parts = (uint32_t*)(ws + lay.parts);
    q.scalar = s.scalar; q.parts = s.parts;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = (int)((total + HM_T - 1) / HM_T), g1 = blocks < HM_MAX_PARTS ? blocks : HM_MAX_PARTS;
    if (is_bf16) k_heatmap_scalar<ore_bf16_t><<<g1, HM_T, 0, st>>>(s);
    else k_heatmap_scalar<float><<<g1, HM_T, 0, st>>>(s);
    int rc;
    if ((rc = ore_launch_status("k_heatmap_scalar"))) return rc;
    if (!s.norm_max) return ORE_OK;
    q.n_parts = g1;
    k_heatmap_quant<<<blocks, HM_T, 0, st>>>(q);
    return ore_launch_status("k_heatmap_quant");
}

extern "C" int ore_heatmap_draw_fwd(const uint8_t* src_hwc, uint8_t* dst_hwc, int32_t h, int32_t w, int32_t n_levels, const uint8_t* map0,
                                    const uint8_t* map1, const uint8_t* map2, const int32_t* level_hw, const int32_t* level_stride,
                                    int32_t in_h, int32_t in_w, const uint8_t* lut_dev, int32_t alpha, int32_t alpha_mode, void* stream) {
    ORE_CHECK_ARG(src_hwc && dst_hwc && lut_dev && level_stride, "ore_heatmap_draw_fwd: null pointer");
    ORE_CHECK_ARG(h >= 1 && h <= ORE_OVERLAY_MAX_SIDE && w >= 1 && w <= ORE_OVERLAY_MAX_SIDE, "ore_heatmap_draw_fwd: frame %dx%d, sides 1 .. %d", h, w,
                  ORE_OVERLAY_MAX_SIDE);
    ORE_CHECK_ARG(dims_ok(n_levels, level_hw), "ore_heatmap_draw_fwd: 1 .. %d levels, map sides 1 .. %d", HM_LEVELS, ORE_HEATMAP_MAX_MAP_SIDE);
    ORE_CHECK_ARG(in_h >= 1 && in_h <= ORE_HEATMAP_MAX_INPUT_SIDE && in_w >= 1 && in_w <= ORE_HEATMAP_MAX_INPUT_SIDE,
                  "ore_heatmap_draw_fwd: model input %dx%d, sides 1 .. %d", in_h, in_w, ORE_HEATMAP_MAX_INPUT_SIDE);
    ORE_CHECK_ARG(alpha >= 0 && alpha <= 255 && (alpha_mode == ORE_HEATMAP_ALPHA_CONSTANT || alpha_mode == ORE_HEATMAP_ALPHA_VALUE),
                  "ore_heatmap_draw_fwd: alpha %d (0 .. 255), alpha_mode %d", alpha, alpha_mode);
    const size_t bytes = (size_t)h * w * 3;
    const uintptr_t ps = (uintptr_t)src_hwc, pd = (uintptr_t)dst_hwc;
    ORE_CHECK_ARG(ps % 4 == 0 && pd % 4 == 0, "ore_heatmap_draw_fwd: the frames must be 4-byte aligned");
    ORE_CHECK_ARG(ps == pd || (ps < pd ? pd - ps : ps - pd) >= bytes, "ore_heatmap_draw_fwd: src and dst overlap (equal = in place, else disjoint)");
    const uint8_t* maps[HM_LEVELS] = {map0, map1, map2};
    RenderArgs a{};
    a.h = h; a.w = w; a.n_levels = n_levels; a.alpha = alpha; a.by_value = alpha_mode == ORE_HEATMAP_ALPHA_VALUE;
    for (int l = 0; l < n_levels; ++l) {
        ORE_CHECK_ARG(maps[l], "ore_heatmap_draw_fwd: level %d has no map", l);
        ORE_CHECK_ARG(level_stride[l] >= 1 && level_stride[l] <= ORE_HEATMAP_MAX_STRIDE, "ore_heatmap_draw_fwd: level %d: stride %d (1 .. %d)", l, level_stride[l],
                      ORE_HEATMAP_MAX_STRIDE);
        a.map[l] = maps[l]; a.mw[l] = level_hw[2 * l + 1];
        a.ax[l] = make_axis(in_w, w, level_stride[l], level_hw[2 * l + 1]);
        a.ay[l] = make_axis(in_h, h, level_stride[l], level_hw[2 * l]);
    }
    const long long npix = (long long)h * w;
    k_heatmap_render<<<(unsigned)((npix + HM_T * HM_PX - 1) / (HM_T * HM_PX)), HM_T, 0, (hipStream_t)stream>>>(a, src_hwc, dst_hwc, lut_dev);
    return ore_launch_status("k_heatmap_render");
}
