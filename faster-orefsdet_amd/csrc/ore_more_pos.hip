// MORE_POS of the CenterNet2 proposal generator on device: the 3x3 block around every object's centre cell, at every
// level, as heat-map positives where the head already regresses the box well.
//   ref:fewx/modeling/fsod/fsod_rpn.py:664-669 (forward), :1213-1243 (_add_more_pos), :1246-1343 (_get_c33_inds),
//   ref:fewx/layers/iou_loss.py (the 'giou' branch).
// Candidate c = l * 9 + k of an object: neighbour k (dx = k % 3 - 1, dy = k / 3 - 1) of its centre cell on level l.  One wave per
// object, one lane per candidate (<= 36): the k-th smallest loss by rank counting over the wave, the selection by a ballot, the place
// in the list from a prefix sum over the objects' counts -- no atomics, the same list run to run.  One block: the work is a few
// dependent gathers per object, and the ordered list needs every object's count before it.
// Rows are level-major [level][image][y][x] like ore_train.hip's.  Compiled with -ffp-contract=off: which candidates are kept depends on
// exact fp32 comparisons, and the GIoU expression is k_cn_loss_partial's, operation for operation.
#include "ore_common.h"

namespace {

constexpr float MP_INF = 100000000.0f;   // fsod_rpn.py:490
constexpr int MP_MAXN = 128;             // objects per image, the limit of ore_centernet_targets_fwd
constexpr int MP_CHUNK = 1024;           // objects per pass of the block: one per thread in the scan

struct MorePosP {
    int n_levels, B, max_n, rows;
    int H[4], W[4], stride[4], row0[4];
    float soi_lo[4], soi_hi[4];
    const float* gt;                     // [B][max_n][4]
    const int* gt_count;                 // [B]
    const float* head; int head_ld;      // [rows][ld], columns 0..3 = ltrb prediction (fp32, detached)
    float thresh; int topk;
};

// torch.kthvalue's order: a < b, every number below NaN
__device__ __forceinline__ bool mp_less(float a, float b) { return a < b || (b != b && a == a); }

// Candidate c of box g in image b: its row, or -1 where the neighbour lies outside the map; with WITH_LOSS also its loss.
template <bool WITH_LOSS>
__device__ __forceinline__ long long mp_candidate(const MorePosP& p, int b, const float* __restrict__ g, int c, float& loss) {
    const int l = c / 9, k = c % 9, dx = k % 3 - 1, dy = k / 3 - 1;
    const float x1 = g[0], y1 = g[1], x2 = g[2], y2 = g[3];
    const int st = p.stride[l], Hl = p.H[l], Wl = p.W[l];
    const float fs = (float)st;
    const long long cx = (long long)(((x1 + x2) / 2.0f) / fs), cy = (long long)(((y1 + y2) / 2.0f) / fs);   // as k_cn_pos_inds
    const long long nx = cx + dx, ny = cy + dy;
    long long row = -1;
    if (nx >= 0 && nx < Wl && ny >= 0 && ny < Hl) {
        row = (long long)p.row0[l] + (long long)b * Hl * Wl + ny * Wl + nx;
        if (row >= p.rows) row = -1;
    }
    if (!WITH_LOSS) return row;
    const float gx = (float)cx * fs + (float)(st / 2), gy = (float)cy * fs + (float)(st / 2);
    const float rl = (gx - x1) / fs, rt = (gy - y1) / fs, rr = (x2 - gx) / fs, rb = (y2 - gy) / fs;
    const float w = x2 - x1, h = y2 - y1;
    const float crit = sqrtf(w * w + h * h) / 2.0f;
    // comparisons one by one: a NaN side is not >= 0, like torch's min(...) >= 0
    const bool level_mask = rl >= 0.0f && rt >= 0.0f && rr >= 0.0f && rb >= 0.0f && crit >= p.soi_lo[l] && crit <= p.soi_hi[l];
    const float tl = rl + (float)dx, tr = rr - (float)dx, tt = rt + (float)dy, tb = rb - (float)dy;   // one stride unit per cell
    const bool valid = row >= 0 && tl >= 0.0f && tt >= 0.0f && tr >= 0.0f && tb >= 0.0f;
    loss = MP_INF;
    if (valid) {
        const float* hr = p.head + (size_t)row * p.head_ld;
        const float pl = hr[0], pt = hr[1], pr = hr[2], pb = hr[3];
        const float ta = (tl + tr) * (tt + tb), pa = (pl + pr) * (pt + pb);
        const float wi = fminf(pl, tl) + fminf(pr, tr), hi = fminf(pb, tb) + fminf(pt, tt);
        const float gw = fmaxf(pl, tl) + fmaxf(pr, tr), gh = fmaxf(pb, tb) + fmaxf(pt, tt);
        const float ac = gw * gh, ai = wi * hi, au = ta + pa - ai;
        const float iou = (ai + 1.0f) / (au + 1.0f);
        loss = 1.0f - (iou - (ac - au) / ac);
        if (pl != pl || pt != pt || pr != pr || pb != pb) loss = pl + pt + pr + pb;     // torch.min / max hand a NaN on, fminf does not
    }
    // the real centre; one outside the map stays invalid and is never read (the one departure from the reference)
    if (k == 4 && level_mask && row >= 0) loss = 0.0f;
    return row;
}

__global__ __launch_bounds__(1024) void k_cn_more_pos(MorePosP p, long long* __restrict__ pos_inds, int* __restrict__ pos_count) {
    __shared__ unsigned long long smask[MP_CHUNK];
    __shared__ int soff[MP_CHUNK];
    __shared__ int wsum[16];
    __shared__ int base_sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nc = p.n_levels * 9;
    const int total = p.B * p.max_n;
    if (tid == 0) base_sh = 0;
    for (int o0 = 0; o0 < total; o0 += MP_CHUNK) {
        const int oend = min(total, o0 + MP_CHUNK);
        smask[tid] = 0ull;
        __syncthreads();
        // selection: loss < min(k-th smallest loss of the object, thresh)
        for (int o = o0 + wave; o < oend; o += 16) {
            const int b = o / p.max_n, n = o % p.max_n;
            if (n >= min(p.gt_count[b], p.max_n)) continue;                                    // wave-uniform
            float v = MP_INF;
            if (lane < nc) mp_candidate<true>(p, b, p.gt + (size_t)o * 4, lane, v);
            int rank = 0;
            for (int j = 0; j < nc; ++j) {
                const float vj = __shfl(v, j);
                rank += (mp_less(vj, v) || (!mp_less(v, vj) && j < lane)) ? 1 : 0;
            }
            const unsigned long long kb = __ballot(lane < nc && rank == p.topk - 1);           // the ranks are a permutation: one lane
            float th = __shfl(v, __ffsll((long long)kb) - 1);
            if (th > p.thresh) th = p.thresh;                                                   // a NaN k-th value stays: nothing is below it
            const unsigned long long m = __ballot(lane < nc && v < th);
            if (lane == 0) smask[o - o0] = m;
        }
        __syncthreads();
        // exclusive prefix sum of the objects' counts, in object order
        const int cnt = __popcll(smask[tid]);
        int inc = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d); if (lane >= d) inc += t; }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int base = base_sh, tot = 0;
        for (int w2 = 0; w2 < 16; ++w2) { const int s = wsum[w2]; if (w2 < wave) base += s; tot += s; }
        soff[tid] = base + inc - cnt;
        __syncthreads();
        // emission in (image, object, level, k) order; a kept candidate's loss is below thresh, so its row is inside the map
        for (int o = o0 + wave; o < oend; o += 16) {
            const unsigned long long m = smask[o - o0];
            if ((m >> lane) & 1ull) {
                float unused;
                const long long row = mp_candidate<false>(p, o / p.max_n, p.gt + (size_t)o * 4, lane, unused);
                pos_inds[soff[o - o0] + __popcll(m & ((1ull << lane) - 1ull))] = row;
            }
        }
        __syncthreads();
        if (tid == 0) base_sh += tot;
        __syncthreads();
    }
    if (tid == 0) *pos_count = base_sh;
}
}  // namespace

extern "C" int ore_centernet_more_pos_fwd(int32_t n_levels, const int32_t* H, const int32_t* W, const int32_t* stride, int32_t B,
                                          const float* gt_boxes, const int32_t* gt_count, int32_t max_n, const float* soi_host,
                                          const float* head, int32_t head_ld, float more_pos_thresh, int32_t more_pos_topk,
                                          int64_t* pos_inds, int32_t* pos_count, void* stream) {
    ORE_CHECK_ARG(H && W && stride && gt_boxes && gt_count && soi_host && head && pos_inds && pos_count,
                  "ore_centernet_more_pos_fwd: null pointer");
    ORE_CHECK_ARG(n_levels >= 1 && n_levels <= 4 && B >= 1 && max_n >= 1 && max_n <= MP_MAXN,
                  "ore_centernet_more_pos_fwd: 1..4 levels, <= %d objects/image", MP_MAXN);
    ORE_CHECK_ARG(head_ld >= 4, "ore_centernet_more_pos_fwd: head_ld=%d < 4", head_ld);
    ORE_CHECK_ARG(more_pos_topk >= 1 && more_pos_topk <= 9 * n_levels, "ore_centernet_more_pos_fwd: topk=%d outside 1..%d (9 per level)",
                  more_pos_topk, 9 * n_levels);
    ORE_CHECK_ARG(more_pos_thresh > 0.0f, "ore_centernet_more_pos_fwd: thresh=%g is not > 0", (double)more_pos_thresh);
    MorePosP p{};
    p.n_levels = n_levels; p.B = B; p.max_n = max_n;
    long long rows = 0;
    for (int l = 0; l < n_levels; ++l) {
        ORE_CHECK_ARG(H[l] >= 1 && W[l] >= 1 && stride[l] >= 1, "ore_centernet_more_pos_fwd: level %d is %dx%d, stride %d", l, H[l], W[l], stride[l]);
        ORE_CHECK_ARG(rows + (long long)B * H[l] * W[l] < (1ll << 31), "ore_centernet_more_pos_fwd: more than 2^31 rows");
        p.H[l] = H[l]; p.W[l] = W[l]; p.stride[l] = stride[l]; p.row0[l] = (int)rows;
        p.soi_lo[l] = soi_host[2 * l]; p.soi_hi[l] = soi_host[2 * l + 1];
        rows += (long long)B * H[l] * W[l];
    }
    ORE_CHECK_ARG((long long)B * max_n * 36 < (1ll << 31), "ore_centernet_more_pos_fwd: B=%d max_n=%d", B, max_n);
    p.rows = (int)rows;
    p.gt = gt_boxes; p.gt_count = gt_count; p.head = head; p.head_ld = head_ld;
    p.thresh = more_pos_thresh; p.topk = more_pos_topk;
    hipLaunchKernelGGL(k_cn_more_pos, dim3(1), dim3(1024), 0, (hipStream_t)stream, p, (long long*)pos_inds, pos_count);
    return ore_launch_status("k_cn_more_pos");
}
