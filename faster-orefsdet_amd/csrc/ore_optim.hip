// Norm clip (torch.nn.utils.clip_grad_norm_) + SGD with or without Nesterov momentum over the flat parameter bucket (row a13).
// ref:fewx/solver/build.py:19-59 (CLIP_TYPE norm: clip_grad_norm_(p, CLIP_VALUE, NORM_TYPE) once per parameter), :136 (NESTEROV):
//   g^ = grad_scale * g;  norm = ||g^ over S||_p (p = 2, 1, inf);  coef = clamp(clip / (norm + 1e-6), max = 1);  g' = g^ * coef
//   g' += wd * p;  buf = momentum * buf + g';  p -= lr * (nesterov ? g' + momentum * buf : buf)
// S is one parameter, or (full model) every parameter of the bucket.  The value-clip step without Nesterov stays k_sgd_step of
// ore_train.hip; this file is compiled with the same flags (-O3 -ffp-contract=off, IEEE division and sqrt: csrc/Makefile).
//
// The norm is three deterministic stages, no floating-point atomics, nothing that depends on the order blocks arrive in:
//   k_grad_norm_partial  block b = run r of parameter part_param[b]: GN_G consecutive chunks of that parameter (fewer at its end);
//                        elements beyond numel are never read into a sum.  A term is (g * grad_scale)^2 (2 roundings) or
//                        |g * grad_scale| (1 rounding).
//                          thread chain   GN_G additions: rows j = 0 .. GN_G / 4 - 1 of 1024 floats; thread t holds floats 4t .. 4t + 3
//                                         of each row and adds them onto 0 in the order (j, 0), (j, 1), (j, 2), (j, 3)
//                          wave butterfly 6 additions (xor 32, 16, 8, 4, 2, 1)
//                          waves in order ((w0 + w1) + w2) + w3: 3 additions                            -> partial[b]
//   k_grad_norm_param    one wave per parameter: lane l adds partials l, l + GN_W, ... of the parameter onto 0 in index order
//                        (ceil(parts / GN_W) additions), butterfly (6) -> acc[param]; norm[param] = sqrtf(acc) for p = 2, acc else;
//                        per-parameter mode: coef[param]
//   k_grad_norm_total    full model only, one block: thread t adds acc[t], acc[t + 256], ... onto 0 (ceil(P / 256) additions),
//                        butterfly (6), waves in order (3); total = sqrtf(sum) for p = 2; coef[every parameter] = the one coefficient
// Chain depth of a parameter's sum: GN_G + 6 + 3 + ceil(parts / GN_W) + 6; of the model's: that of its deepest parameter +
// ceil(P / 256) + 6 + 3.  sqrtf, the addition of 1e-6 and the division round once each.  For p = inf every addition above is a
// maximum (a selection: no rounding).  The maximum keeps a NaN (torch.max), as the sums do; the clamp is a comparison, so a NaN
// coefficient stays one (torch.clamp).
#include "ore_common.h"

namespace {

constexpr int GN_G = 16;                 // chunks of 256 floats per partial: 16 KB per block, four 16-byte loads in flight per thread
constexpr int GN_W = 64;                 // partials one pass of the per-parameter wave takes
enum { GN_LINF = 0, GN_L1 = 1, GN_L2 = 2 };

template <int KIND>
__device__ __forceinline__ float gn_term(float g, float grad_scale) {
    const float s = g * grad_scale;
    return KIND == GN_L2 ? s * s : fabsf(s);
}
// a + b, or the larger of the two with a NaN kept whichever side it is on
template <int KIND>
__device__ __forceinline__ float gn_join(float a, float b) {
    if (KIND == GN_LINF) return (b > a || b != b) ? b : a;
    return a + b;
}
template <int KIND>
__device__ __forceinline__ float gn_wave(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = gn_join<KIND>(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ float gn_coef(float norm, float clip) {
    const float c = clip / (norm + 1e-6f);
    return c > 1.0f ? 1.0f : c;
}

template <int KIND>
__global__ __launch_bounds__(256) void k_grad_norm_partial(const float* __restrict__ g, const long long* __restrict__ numel,
                                                           const long long* __restrict__ chunk0, const int* __restrict__ part_param,
                                                           const int* __restrict__ part0, float grad_scale,
                                                           float* __restrict__ partial) {
    __shared__ float red[4];
    const int b = blockIdx.x, prm = part_param[b];
    const long long e0 = (long long)(b - part0[prm]) * (GN_G * 256);       // first element of the run, inside the parameter
    const float* src = g + chunk0[prm] * 256 + e0;
    const long long left = numel[prm] - e0;                                 // > 0: the run exists because the parameter reaches it
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < GN_G / 4; ++j) {
        const long long o = (long long)j * 1024 + 4 * threadIdx.x;
        if (o < left) {                                                     // the chunk is whole in memory (padding): 16 bytes are there
            const f32x4 v = *reinterpret_cast<const f32x4*>(src + o);
            acc = gn_join<KIND>(acc, gn_term<KIND>(v.x, grad_scale));
            if (o + 1 < left) acc = gn_join<KIND>(acc, gn_term<KIND>(v.y, grad_scale));
            if (o + 2 < left) acc = gn_join<KIND>(acc, gn_term<KIND>(v.z, grad_scale));
            if (o + 3 < left) acc = gn_join<KIND>(acc, gn_term<KIND>(v.w, grad_scale));
        }
    }
    acc = gn_wave<KIND>(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[b] = gn_join<KIND>(gn_join<KIND>(gn_join<KIND>(red[0], red[1]), red[2]), red[3]);
}

template <int KIND>
__global__ __launch_bounds__(256) void k_grad_norm_param(const float* __restrict__ partial, const int* __restrict__ part0, int n_params,
                                                         float clip, int full_model, float* __restrict__ acc_out,
                                                         float* __restrict__ norm, float* __restrict__ coef) {
    const int prm = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (prm >= n_params) return;                                            // whole waves leave; there is no barrier below
    const int hi = part0[prm + 1];
    float acc = 0.0f;
    for (int q = part0[prm] + lane; q < hi; q += GN_W) acc = gn_join<KIND>(acc, partial[q]);
    acc = gn_wave<KIND>(acc);
    if (lane == 0) {
        const float nv = KIND == GN_L2 ? sqrtf(acc) : acc;
        acc_out[prm] = acc;
        norm[prm] = nv;
        if (!full_model) coef[prm] = gn_coef(nv, clip);
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void k_grad_norm_total(const float* __restrict__ acc_in, int n_params, float clip,
                                                         float* __restrict__ total, float* __restrict__ coef) {
    __shared__ float red[4];
    float acc = 0.0f;
    for (int q = threadIdx.x; q < n_params; q += 256) acc = gn_join<KIND>(acc, acc_in[q]);
    acc = gn_wave<KIND>(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    const float s = gn_join<KIND>(gn_join<KIND>(gn_join<KIND>(red[0], red[1]), red[2]), red[3]);
    const float nv = KIND == GN_L2 ? sqrtf(s) : s;
    const float c = gn_coef(nv, clip);
    if (threadIdx.x == 0) *total = nv;
    for (int q = threadIdx.x; q < n_params; q += 256) coef[q] = c;
}

// The update beside k_sgd_step: the clip is a multiplication by coef[parameter of the chunk] (coef != NULL; always applied, the
// coefficient may be 1) or the value clamp of k_sgd_step (coef == NULL).  The padding of a parameter's last chunk is left alone, so a
// NaN coefficient stays inside its parameter.
template <bool NESTEROV>
__global__ __launch_bounds__(256) void k_sgd_step_norm(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                       const float* __restrict__ chunk_lr, const float* __restrict__ chunk_wd,
                                                       const int* __restrict__ chunk_param, const long long* __restrict__ numel,
                                                       const long long* __restrict__ chunk0, const float* __restrict__ coef,
                                                       const float* __restrict__ lr_scale_dev, float lr_scale, float momentum,
                                                       float clip, float grad_scale) {
    const int c = blockIdx.x;
    const size_t i = (size_t)c * 256 + threadIdx.x;
    // the three streams first: they do not wait for the table look-ups below, and the padding is memory of the bucket (only stores are guarded)
    const float g0 = g[i], pi = p[i], b0 = buf[i];
    const int prm = chunk_param[c];
    const bool live = ((long long)c - chunk0[prm]) * 256 + threadIdx.x < numel[prm];
    const float lr = chunk_lr[c] * (lr_scale_dev ? *lr_scale_dev : lr_scale);
    const float wd = chunk_wd[c];
    float gi = g0 * grad_scale;
    if (coef) gi = gi * coef[prm];
    else if (clip > 0.0f) gi = gi > clip ? clip : (gi < -clip ? -clip : gi);
    gi = gi + wd * pi;
    const float b = momentum * b0 + gi;
    if (!live) return;
    buf[i] = b;
    p[i] = pi - lr * (NESTEROV ? gi + momentum * b : b);
}

template <int KIND>
int grad_norm_launch(const float* grads, int32_t n_params, const int64_t* numel, const int64_t* chunk0, const int32_t* part_param,
                     const int32_t* part0, int64_t n_parts, int32_t full_model, float clip_value, float grad_scale, float* partial,
                     float* acc, float* norm, float* coef, float* total, hipStream_t st) {
    hipLaunchKernelGGL(k_grad_norm_partial<KIND>, dim3((unsigned)n_parts), dim3(256), 0, st, grads, (const long long*)numel,
                       (const long long*)chunk0, part_param, part0, grad_scale, partial);
    int rc = ore_launch_status("k_grad_norm_partial");
    if (rc) return rc;
    hipLaunchKernelGGL(k_grad_norm_param<KIND>, dim3((unsigned)ceil_div(n_params, 4)), dim3(256), 0, st, partial, part0, n_params,
                       clip_value, full_model, acc, norm, coef);
    rc = ore_launch_status("k_grad_norm_param");
    if (rc || !full_model) return rc;
    hipLaunchKernelGGL(k_grad_norm_total<KIND>, dim3(1), dim3(256), 0, st, acc, n_params, clip_value, total, coef);
    return ore_launch_status("k_grad_norm_total");
}
}  // namespace

extern "C" int ore_grad_norm_geometry(int32_t* chunks_per_partial, int32_t* partials_per_pass) {
    ORE_CHECK_ARG(chunks_per_partial && partials_per_pass, "ore_grad_norm_geometry: null pointer");
    *chunks_per_partial = GN_G;
    *partials_per_pass = GN_W;
    return ORE_OK;
}

extern "C" int ore_grad_norm_plan(const int64_t* numel, int32_t n_params, int32_t* part0, int32_t* part_param, int64_t part_cap,
                                  int64_t* n_chunks, int64_t* n_parts) {
    ORE_CHECK_ARG(numel && n_params > 0 && n_chunks && n_parts, "ore_grad_norm_plan: bad args");
    ORE_CHECK_ARG(part_param == nullptr || part_cap >= 0, "ore_grad_norm_plan: part_cap=%lld", (long long)part_cap);
    int64_t chunks = 0, parts = 0;
    for (int32_t i = 0; i < n_params; ++i) {
        ORE_CHECK_ARG(numel[i] > 0 && numel[i] < (1ll << 38), "ore_grad_norm_plan: numel[%d]=%lld", i, (long long)numel[i]);
        const int64_t c = (numel[i] + 255) / 256, r = (c + GN_G - 1) / GN_G;
        ORE_CHECK_ARG(chunks + c < (1ll << 31), "ore_grad_norm_plan: more than 2^31 chunks");
        if (part0) part0[i] = (int32_t)parts;
        if (part_param) {
            ORE_CHECK_ARG(parts + r <= part_cap, "ore_grad_norm_plan: %lld partials do not fit part_cap=%lld", (long long)(parts + r),
                          (long long)part_cap);
            for (int64_t q = 0; q < r; ++q) part_param[parts + q] = i;
        }
        chunks += c;
        parts += r;
    }
    if (part0) part0[n_params] = (int32_t)parts;
    *n_chunks = chunks;
    *n_parts = parts;
    return ORE_OK;
}

extern "C" int ore_grad_norm_fwd(const float* grads, int32_t n_params, const int64_t* numel, const int64_t* chunk0,
                                 const int32_t* part_param, const int32_t* part0, int64_t n_parts, int32_t norm_kind, int32_t full_model,
                                 float clip_value, float grad_scale, float* partial, float* acc, float* norm, float* coef, float* total,
                                 void* stream) {
    ORE_CHECK_ARG(grads && numel && chunk0 && part_param && part0 && partial && acc && norm && coef, "ore_grad_norm_fwd: null pointer");
    ORE_CHECK_ARG(n_params > 0 && n_parts >= n_params && n_parts < (1ll << 31), "ore_grad_norm_fwd: n_params=%d n_parts=%lld", n_params,
                  (long long)n_parts);
    ORE_CHECK_ARG(norm_kind == GN_L2 || norm_kind == GN_L1 || norm_kind == GN_LINF, "ore_grad_norm_fwd: norm_kind=%d (2, 1, 0 = inf)", norm_kind);
    ORE_CHECK_ARG(!full_model || total, "ore_grad_norm_fwd: the full-model norm needs total");
    hipStream_t st = (hipStream_t)stream;
    if (norm_kind == GN_L2)
        return grad_norm_launch<GN_L2>(grads, n_params, numel, chunk0, part_param, part0, n_parts, full_model, clip_value, grad_scale,
                                       partial, acc, norm, coef, total, st);
    if (norm_kind == GN_L1)
        return grad_norm_launch<GN_L1>(grads, n_params, numel, chunk0, part_param, part0, n_parts, full_model, clip_value, grad_scale,
                                       partial, acc, norm, coef, total, st);
    return grad_norm_launch<GN_LINF>(grads, n_params, numel, chunk0, part_param, part0, n_parts, full_model, clip_value, grad_scale,
                                     partial, acc, norm, coef, total, st);
}

extern "C" int ore_sgd_step_clipnorm_fwd(float* params, const float* grads, float* momentum_buf, int64_t n_chunks, const float* chunk_lr,
                                         const float* chunk_wd, const int32_t* chunk_param, const int64_t* numel, const int64_t* chunk0,
                                         const float* coef, const float* lr_scale_dev, float lr_scale, float momentum, float clip_value,
                                         float grad_scale, int32_t nesterov, void* stream) {
    ORE_CHECK_ARG(params && grads && momentum_buf && chunk_lr && chunk_wd && chunk_param && numel && chunk0 && n_chunks > 0 &&
                  n_chunks < (1ll << 31), "ore_sgd_step_clipnorm_fwd: bad args");
    ORE_CHECK_ARG(!nesterov || momentum > 0.0f, "ore_sgd_step_clipnorm_fwd: Nesterov momentum requires a momentum");
    const dim3 grid((unsigned)n_chunks);
    const long long *ne = (const long long*)numel, *c0 = (const long long*)chunk0;
    if (nesterov)
        hipLaunchKernelGGL(k_sgd_step_norm<true>, grid, dim3(256), 0, (hipStream_t)stream, params, grads, momentum_buf, chunk_lr, chunk_wd,
                           chunk_param, ne, c0, coef, lr_scale_dev, lr_scale, momentum, clip_value, grad_scale);
    else
        hipLaunchKernelGGL(k_sgd_step_norm<false>, grid, dim3(256), 0, (hipStream_t)stream, params, grads, momentum_buf, chunk_lr, chunk_wd,
                           chunk_param, ne, c0, coef, lr_scale_dev, lr_scale, momentum, clip_value, grad_scale);
    return ore_launch_status("k_sgd_step_norm");
}
