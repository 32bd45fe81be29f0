// The wide form of the tracker: the association contract "track v1" (include/ore_hip.h) for up to 8192 rows and 16384 tracks -- the
// rows a tiled or TTA merge hands over.  Same state buffer, same contract, same ids as ore_track.hip wherever both take the input; the
// layout and the fp32 IoU come from ore_track.h and both files are compiled with -ffp-contract=off.  Two launches per update, on the
// caller's stream; the counts are read on the device.
//   k_track_wide_cand   the candidate bits, on the whole chip: one wave per tile of 64 tracks x 64 rows (blocks beyond the device-side
//                       m or n return at once).  Lane = track slot; the 64 rows are staged in LDS and walked in a uniform loop, a
//                       lane collects its track's word bit by bit and the ballot of a step IS the row's word over the 64 tracks.  One
//                       64-bit word per (track, row block) and the transposed word per (row, track block) go to the workspace; every
//                       word the match reads (track < m, row block < ceil(n / 64); row < n, track block < ceil(m / 64)) is written
//                       here, so nothing needs a zero fill.
//   k_track_wide_match  one workgroup of 1024 threads that strides over tracks and rows.
//     snapshot  the old list (boxes, classes, ids, ttl) is copied to the workspace: the commit rebuilds the list in place, and every
//               later read of the old list is of the copy.
//     rounds    the greedy matching over (iou descending, slot ascending, row ascending) as rounds of mutually best pairs: every
//               unmatched track picks its best unmatched candidate row (IoU recomputed from the boxes; rows ascending, so the first of
//               equal IoUs stays), every unmatched live row its best unmatched track (slots ascending); after a barrier a track whose
//               row names it back is matched.  The first remaining pair of the total order is always such a pair, so a round that
//               has candidates left commits at least one, and a pair that commits precedes every pair it conflicts with: the result
//               is the sorted scan's.  At most min(m, live rows) rounds; the loop is bounded by that count.  The matched
//               sets are bit sets in LDS (integer or: order-free); the words a track or a row still has to look at are kept as a
//               [first, last) range in the workspace, narrowed in every round.
//     commit    an ordered block scan (ore_block.h) over contiguous chunks -- 8 rows and 16 slots per thread -- gives every live row
//               its place, every new row its id and every surviving track its place behind the rows; the new list, the zeros behind
//               it, ids_out and the header are written as ore_track.hip writes them.
// No floating-point atomics, no dependence on block scheduling: the result is a function of the inputs alone.
#include "ore_track.h"

namespace {

constexpr int TW_MAX_T = ORE_TRACK_WIDE_MAX_TRACKS;
constexpr int TW_MAX_ROWS = ORE_TRACK_WIDE_MAX_ROWS;
constexpr int TW_THREADS = 1024;                     // of k_track_wide_match
constexpr int TW_ROWS_PER_THREAD = TW_MAX_ROWS / TW_THREADS, TW_SLOTS_PER_THREAD = TW_MAX_T / TW_THREADS;
static_assert(TW_ROWS_PER_THREAD == 8, "a thread's rows are one byte of the live bit set");
static_assert(TW_SLOTS_PER_THREAD * TW_THREADS == TW_MAX_T && TW_MAX_T <= 32767 && TW_MAX_ROWS <= 32767, "picks are int16");

// the workspace of one update (host and device agree through this struct)
struct WideWs {
    unsigned long long* cand;      // [capacity][rw]: bit j of word (t, w) = row 64 w + j is a candidate of track t
    unsigned long long* candT;     // [max_rows][tw]: bit j of word (d, w) = track 64 w + j is a candidate of row d
    float* boxes; int64_t* classes; int64_t* ids; int32_t* ttl;       // the old list, [capacity] each
    uint32_t* trange; uint32_t* rrange;                               // [capacity], [max_rows]: first | last << 16 of the words left
    int32_t rw, tw;                                                   // words of a track's row mask, of a row's track mask
};
size_t wide_ws_layout(void* base, int capacity, int max_rows, WideWs* out) {
    WsCursor c;
    const size_t cap = (size_t)capacity, rows = (size_t)max_rows, rw = (rows + 63) / 64, tw = (cap + 63) / 64;
    const size_t o_cand = c.take(cap * rw * 8), o_candT = c.take(rows * tw * 8), o_boxes = c.take(cap * 16), o_cls = c.take(cap * 8),
                 o_ids = c.take(cap * 8), o_ttl = c.take(cap * 4), o_tr = c.take(cap * 4), o_rr = c.take(rows * 4);
    if (out) {
        char* b = static_cast<char*>(base);
        out->cand = reinterpret_cast<unsigned long long*>(b + o_cand);
        out->candT = reinterpret_cast<unsigned long long*>(b + o_candT);
        out->boxes = reinterpret_cast<float*>(b + o_boxes);
        out->classes = reinterpret_cast<int64_t*>(b + o_cls);
        out->ids = reinterpret_cast<int64_t*>(b + o_ids);
        out->ttl = reinterpret_cast<int32_t*>(b + o_ttl);
        out->trange = reinterpret_cast<uint32_t*>(b + o_tr);
        out->rrange = reinterpret_cast<uint32_t*>(b + o_rr);
        out->rw = (int32_t)rw;
        out->tw = (int32_t)tw;
    }
    return c.o;
}

struct WideArgs {
    void* state; int32_t capacity;
    const float* boxes; const float* scores; const int64_t* classes; const int32_t* n_dev; int32_t n_host, max_rows;
    float score_thresh, iou_thresh; int32_t ttl, class_aware; int64_t* ids_out;
    WideWs ws;
};

__device__ __forceinline__ int wide_rows(const WideArgs& a) {
    const int n = a.n_dev ? *a.n_dev : a.n_host;
    return n < 0 ? 0 : (n > a.max_rows ? a.max_rows : n);
}
__device__ __forceinline__ int wide_tracks(const WideArgs& a, const Header& hd) {
    return hd.m < 0 ? 0 : (hd.m > a.capacity ? a.capacity : hd.m);
}

__global__ __launch_bounds__(TW_THREADS) void k_track_wide_reset(void* state, int capacity) {
    const State s = track_state(state, capacity);
    const int t = threadIdx.x;
    if (t == 0) *s.hd = Header{0, capacity, 0, 0, 0};
    for (int j = t; j < capacity; j += blockDim.x) {
        *reinterpret_cast<f32x4*>(s.boxes + (size_t)j * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
        s.classes[j] = 0; s.ids[j] = 0; s.ttl[j] = 0;
    }
}

// grid (row blocks, track blocks), one wave: the tile of tracks 64 by .. 64 by + 63 and rows 64 bx .. 64 bx + 63
__global__ __launch_bounds__(64) void k_track_wide_cand(const WideArgs a) {
    __shared__ __attribute__((aligned(16))) f32x4 s_box[64];
    __shared__ float s_area[64];
    __shared__ long long s_cls[64];
    const State st = track_state(a.state, a.capacity);
    const int n = wide_rows(a), m = wide_tracks(a, *st.hd);
    const int bx = blockIdx.x, by = blockIdx.y, lane = threadIdx.x;
    if (bx * 64 >= n || by * 64 >= m) return;                   // no word of this tile is ever read
    const int d = bx * 64 + lane, t = by * 64 + lane;
    f32x4 rb = {0.f, 0.f, 0.f, 0.f};
    long long rcls = 0;
    bool live = false;
    if (d < n) {
        rb = *reinterpret_cast<const f32x4*>(a.boxes + (size_t)d * 4);
        rcls = a.classes ? (long long)a.classes[d] : 0ll;
        live = track_row_live(rb, a.scores[d], a.score_thresh);
    }
    s_box[lane] = rb;
    s_area[lane] = track_area(rb);
    s_cls[lane] = rcls;
    const unsigned long long livemask = __ballot(live);
    f32x4 tb = {0.f, 0.f, 0.f, 0.f};
    long long tcls = 0;
    if (t < m) {
        tb = *reinterpret_cast<const f32x4*>(st.boxes + (size_t)t * 4);
        tcls = st.classes[t];
    }
    const float tarea = track_area(tb);
    __syncthreads();
    unsigned long long mine = 0ull, theirs = 0ull;              // this track's rows; the tracks of row `lane`
    for (int j = 0; j < 64; ++j) {                              // the same row for the whole wave: LDS broadcasts
        if (!((livemask >> j) & 1ull)) continue;
        const bool c = t < m && track_iou(tb, tarea, s_box[j], s_area[j]) > a.iou_thresh && (!a.class_aware || s_cls[j] == tcls);
        const unsigned long long bal = __ballot(c);
        if (lane == j) theirs = bal;
        mine |= (unsigned long long)c << j;
    }
    if (t < a.capacity) a.ws.cand[(size_t)t * a.ws.rw + bx] = mine;
    if (d < a.max_rows) a.ws.candT[(size_t)d * a.ws.tw + by] = theirs;
}

__device__ __forceinline__ uint32_t wide_range(int lo, int hi) { return (uint32_t)lo | ((uint32_t)hi << 16); }

__global__ __launch_bounds__(TW_THREADS) void k_track_wide_match(const WideArgs a) {
    __shared__ short s_tpick[TW_MAX_T];                         // the row a track picked in this round, -1: none
    __shared__ short s_rpick[TW_MAX_ROWS];                      // the track a row picked; of a matched row: its track
    __shared__ unsigned long long s_live[TW_MAX_ROWS / 64], s_rdone[TW_MAX_ROWS / 64], s_tdone[TW_MAX_T / 64];
    __shared__ long long s_wsum[TW_THREADS / 64];
    __shared__ int s_changed[3], s_nlive;

    const State st = track_state(a.state, a.capacity);
    const WideWs& ws = a.ws;
    const int tid = threadIdx.x;
    const int n = wide_rows(a);
    const Header hd = *st.hd;
    const int m = wide_tracks(a, hd);
    const int nw = (n + 63) >> 6, mw = (m + 63) >> 6;          // the words of the masks that kernel 1 wrote

    // ---- snapshot of the old list, the live rows, the ranges
    if (tid < TW_MAX_ROWS / 64) { s_live[tid] = 0ull; s_rdone[tid] = 0ull; }
    if (tid < TW_MAX_T / 64) s_tdone[tid] = 0ull;
    if (tid < 3) s_changed[tid] = 0;
    if (tid == 0) s_nlive = 0;
    __syncthreads();
    for (int t = tid; t < m; t += TW_THREADS) {
        *reinterpret_cast<f32x4*>(ws.boxes + (size_t)t * 4) = *reinterpret_cast<const f32x4*>(st.boxes + (size_t)t * 4);
        ws.classes[t] = st.classes[t]; ws.ids[t] = st.ids[t]; ws.ttl[t] = st.ttl[t];
        ws.trange[t] = wide_range(0, nw);
        s_tpick[t] = -1;
    }
    {
        unsigned bits = 0u;                                     // rows 8 tid .. 8 tid + 7: one byte of the live bit set
        for (int j = 0; j < TW_ROWS_PER_THREAD; ++j) {
            const int d = tid * TW_ROWS_PER_THREAD + j;
            if (d < n && track_row_live(*reinterpret_cast<const f32x4*>(a.boxes + (size_t)d * 4), a.scores[d], a.score_thresh)) bits |= 1u << j;
        }
        reinterpret_cast<unsigned char*>(s_live)[tid] = (unsigned char)bits;
        if (bits) atomicAdd(&s_nlive, __popc(bits));
        for (int d = tid; d < a.max_rows; d += TW_THREADS) s_rpick[d] = -1;
    }
    __syncthreads();
    for (int d = tid; d < n; d += TW_THREADS) ws.rrange[d] = (s_live[d >> 6] >> (d & 63)) & 1ull ? wide_range(0, mw) : 0u;
    const int n_live_rows = s_nlive;
    const int max_rounds = m < n_live_rows ? m : n_live_rows;

    // ---- rounds of mutually best pairs (a thread reads and writes the ranges of its own tracks and rows only)
    for (int round = 0; round < max_rounds; ++round) {
        if (tid == 0) s_changed[(round + 1) % 3] = 0;           // read last two barriers ago, set next after the next barrier
        for (int t = tid; t < m; t += TW_THREADS) {
            const uint32_t rg = ws.trange[t];
            int lo = (int)(rg & 0xffffu), hi = (int)(rg >> 16);
            if (lo >= hi || ((s_tdone[t >> 6] >> (t & 63)) & 1ull)) continue;
            const f32x4 tb = *reinterpret_cast<const f32x4*>(ws.boxes + (size_t)t * 4);
            const float tarea = track_area(tb);
            float best = 0.0f;
            int best_d = -1, first = hi, last = lo;
            for (int w = lo; w < hi; ++w) {
                unsigned long long rest = ws.cand[(size_t)t * ws.rw + w] & ~s_rdone[w];
                if (rest) { first = first < w ? first : w; last = w + 1; }
                while (rest) {
                    const int d = w * 64 + __builtin_ctzll(rest);
                    rest &= rest - 1ull;
                    const f32x4 b = *reinterpret_cast<const f32x4*>(a.boxes + (size_t)d * 4);
                    const float v = track_iou(tb, tarea, b, track_area(b));   // > iou_thresh >= 0
                    if (v > best) { best = v; best_d = d; }     // rows ascending: the first of equal IoUs stays
                }
            }
            ws.trange[t] = best_d >= 0 ? wide_range(first, last) : 0u;
            s_tpick[t] = (short)best_d;
        }
        for (int d = tid; d < n; d += TW_THREADS) {
            const uint32_t rg = ws.rrange[d];
            int lo = (int)(rg & 0xffffu), hi = (int)(rg >> 16);
            if (lo >= hi || ((s_rdone[d >> 6] >> (d & 63)) & 1ull)) continue;
            const f32x4 b = *reinterpret_cast<const f32x4*>(a.boxes + (size_t)d * 4);
            const float barea = track_area(b);
            float best = 0.0f;
            int best_t = -1, first = hi, last = lo;
            for (int w = lo; w < hi; ++w) {
                unsigned long long rest = ws.candT[(size_t)d * ws.tw + w] & ~s_tdone[w];
                if (rest) { first = first < w ? first : w; last = w + 1; }
                while (rest) {
                    const int t = w * 64 + __builtin_ctzll(rest);
                    rest &= rest - 1ull;
                    const f32x4 tb = *reinterpret_cast<const f32x4*>(ws.boxes + (size_t)t * 4);
                    const float v = track_iou(tb, track_area(tb), b, barea);
                    if (v > best) { best = v; best_t = t; }     // slots ascending: the first of equal IoUs stays
                }
            }
            ws.rrange[d] = best_t >= 0 ? wide_range(first, last) : 0u;
            s_rpick[d] = (short)best_t;
        }
        __syncthreads();
        for (int t = tid; t < m; t += TW_THREADS) {
            const int d = s_tpick[t];
            if (d < 0 || ((s_tdone[t >> 6] >> (t & 63)) & 1ull) || s_rpick[d] != t) continue;
            atomicOr(&s_tdone[t >> 6], 1ull << (t & 63));       // s_rpick[d] stays t: a matched row is never picked for again
            atomicOr(&s_rdone[d >> 6], 1ull << (d & 63));
            s_changed[round % 3] = 1;
        }
        __syncthreads();
        if (!s_changed[round % 3]) break;
    }
    __syncthreads();

    // ---- commit: rows 8 tid .., slots 16 tid .. per thread, places by one ordered scan of (survivors, live rows, new rows)
    const int r0 = tid * TW_ROWS_PER_THREAD, t0 = tid * TW_SLOTS_PER_THREAD;
    const unsigned livebits = reinterpret_cast<const unsigned char*>(s_live)[tid];
    const unsigned newbits = livebits & ~(unsigned)reinterpret_cast<const unsigned char*>(s_rdone)[tid];
    unsigned survbits = 0u;
    for (int j = 0; j < TW_SLOTS_PER_THREAD; ++j) {
        const int t = t0 + j;
        if (t < m && !((s_tdone[t >> 6] >> (t & 63)) & 1ull) && ws.ttl[t] - 1 > 0) survbits |= 1u << j;
    }
    const long long own = ((long long)__popc(survbits) << 40) | ((long long)__popc(livebits) << 20) | (long long)__popc(newbits);
    long long total = 0;
    const long long before = block_incl_scan<TW_THREADS / 64, long long>(own, s_wsum, total) - own;
    int p_new = (int)(before & 0xfffff), p_live = (int)((before >> 20) & 0xfffff), p_surv = (int)(before >> 40);
    const int n_new = (int)(total & 0xfffff), n_live = (int)((total >> 20) & 0xfffff), n_surv = (int)(total >> 40);
    for (int j = 0; j < TW_ROWS_PER_THREAD; ++j) {
        const int d = r0 + j;
        if (d >= a.max_rows) break;
        long long rid = -1;
        if ((livebits >> j) & 1u) {
            rid = (newbits >> j) & 1u ? hd.next_id + p_new++ : ws.ids[s_rpick[d]];
            if (p_live < a.capacity) {
                *reinterpret_cast<f32x4*>(st.boxes + (size_t)p_live * 4) = *reinterpret_cast<const f32x4*>(a.boxes + (size_t)d * 4);
                st.classes[p_live] = a.classes ? a.classes[d] : 0;
                st.ids[p_live] = rid; st.ttl[p_live] = a.ttl;
            }
            ++p_live;
        }
        a.ids_out[d] = rid;
    }
    for (int j = 0; j < TW_SLOTS_PER_THREAD; ++j) {
        if (!((survbits >> j) & 1u)) continue;
        const int t = t0 + j, p = n_live + p_surv++;
        if (p < a.capacity) {
            *reinterpret_cast<f32x4*>(st.boxes + (size_t)p * 4) = *reinterpret_cast<const f32x4*>(ws.boxes + (size_t)t * 4);
            st.classes[p] = ws.classes[t]; st.ids[p] = ws.ids[t]; st.ttl[p] = ws.ttl[t] - 1;
        }
    }
    const int all = n_live + n_surv, m_new = all < a.capacity ? all : a.capacity;
    for (int t = m_new + tid; t < m; t += TW_THREADS) {         // slots m .. capacity - 1 held zeros already
        *reinterpret_cast<f32x4*>(st.boxes + (size_t)t * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
        st.classes[t] = 0; st.ids[t] = 0; st.ttl[t] = 0;
    }
    if (tid == 0) *st.hd = Header{m_new, a.capacity, hd.next_id + n_new, hd.frames + 1, hd.dropped + (all - m_new)};
}

bool wide_capacity_ok(int32_t capacity) { return capacity >= 1 && capacity <= TW_MAX_T; }

}  // namespace

extern "C" size_t ore_track_wide_state_bytes(int32_t capacity) { return wide_capacity_ok(capacity) ? track_state_bytes(capacity) : 0; }

extern "C" size_t ore_track_wide_workspace_bytes(int32_t capacity, int32_t max_rows) {
    if (!wide_capacity_ok(capacity) || max_rows < 0 || max_rows > TW_MAX_ROWS) return 0;
    return wide_ws_layout(nullptr, capacity, max_rows, nullptr);
}

extern "C" int ore_track_wide_reset(void* state, int32_t capacity, void* stream) {
    ORE_CHECK_ARG(wide_capacity_ok(capacity), "ore_track_wide_reset: capacity %d (1 .. %d)", capacity, TW_MAX_T);
    ORE_CHECK_ARG(state && (uintptr_t)state % 16 == 0, "ore_track_wide_reset: the state is a 16-byte aligned device buffer");
    k_track_wide_reset<<<1, TW_THREADS, 0, (hipStream_t)stream>>>(state, capacity);
    return ore_launch_status("k_track_wide_reset");
}

extern "C" int ore_track_wide_update_fwd(void* state, int32_t capacity, const float* boxes, const float* scores, const int64_t* classes,
                                         const int32_t* n_dev, int32_t n_host, int32_t max_rows, float score_thresh, float iou_thresh,
                                         int32_t ttl, int32_t class_aware, int64_t* ids_out, void* workspace, size_t workspace_bytes,
                                         void* stream) {
    ORE_CHECK_ARG(wide_capacity_ok(capacity), "ore_track_wide_update_fwd: capacity %d (1 .. %d)", capacity, TW_MAX_T);
    ORE_CHECK_ARG(state && (uintptr_t)state % 16 == 0, "ore_track_wide_update_fwd: the state is a 16-byte aligned device buffer");
    ORE_CHECK_ARG(max_rows >= 0 && max_rows <= TW_MAX_ROWS && (n_dev || n_host >= 0), "ore_track_wide_update_fwd: max_rows %d (0 .. %d), n_host %d",
                  max_rows, TW_MAX_ROWS, n_host);
    ORE_CHECK_ARG(max_rows == 0 || (boxes && scores && ids_out), "ore_track_wide_update_fwd: null rows");
    ORE_CHECK_ARG(max_rows == 0 || ((uintptr_t)boxes % 16 == 0 && (uintptr_t)ids_out % 8 == 0), "ore_track_wide_update_fwd: boxes 16-byte, ids_out 8-byte aligned");
    ORE_CHECK_ARG(ttl >= 1 && ttl <= (1 << 20), "ore_track_wide_update_fwd: ttl %d (1 .. %d)", ttl, 1 << 20);
    ORE_CHECK_ARG(iou_thresh >= 0.0f && iou_thresh <= 3.0e38f, "ore_track_wide_update_fwd: iou_thresh is finite and >= 0");
    ORE_CHECK_ARG(score_thresh == score_thresh, "ore_track_wide_update_fwd: score_thresh is NaN");
    const size_t need = wide_ws_layout(nullptr, capacity, max_rows, nullptr);
    ORE_CHECK_ARG(workspace && (uintptr_t)workspace % 256 == 0 && workspace_bytes >= need,
                  "ore_track_wide_update_fwd: the workspace is a 256-byte aligned device buffer of %zu bytes (ore_track_wide_workspace_bytes), got %zu",
                  need, workspace_bytes);
    const size_t sb = track_state_bytes(capacity), r = (size_t)max_rows;
    const void* arr[6] = {state, ids_out, workspace, boxes, scores, classes};
    const size_t len[6] = {sb, r * 8, need, r * 16, r * 4, r * 8};
    for (int i = 0; i < 3; ++i)                                 // the three buffers written, against each other and every input
        for (int j = i + 1; j < 6; ++j)
            ORE_CHECK_ARG(track_disjoint(arr[i], len[i], arr[j], len[j]),
                          "ore_track_wide_update_fwd: state, ids_out, the workspace and the row arrays must be disjoint");
    WideArgs a{state, capacity, boxes, scores, classes, n_dev, n_host, max_rows, score_thresh, iou_thresh, ttl, class_aware ? 1 : 0, ids_out, {}};
    wide_ws_layout(workspace, capacity, max_rows, &a.ws);
    if (max_rows > 0) {
        k_track_wide_cand<<<dim3((unsigned)a.ws.rw, (unsigned)a.ws.tw), 64, 0, (hipStream_t)stream>>>(a);
        const int rc = ore_launch_status("k_track_wide_cand");
        if (rc) return rc;
    }
    k_track_wide_match<<<1, TW_THREADS, 0, (hipStream_t)stream>>>(a);
    return ore_launch_status("k_track_wide_match");
}
