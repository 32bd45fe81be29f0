// Detection tracking ("track v1", include/ore_hip.h): the rows of one frame are associated with the tracks of the frames before it, on the
// device, behind the pass and on its stream -- no host wait between the pass, the ids and the drawn frame.
//   k_track_reset   one block: the header and the four arrays of the caller's state buffer
//   k_track_update  ONE launch of ONE workgroup, thread t = track slot t and thread i = row i (block = max(capacity, max_rows) rounded up
//                   to a wave).  The rows are staged in LDS, a thread keeps its track in registers.
//     scan    every track runs over the live rows once (the row is the same for a whole wave: LDS broadcasts) and keeps its candidate
//             rows as a bit mask in registers -- 320 rows = 5 x 64 bits.
//     rounds  the greedy match over (iou desc, slot asc, row asc) as rounds of mutually best pairs: every remaining track walks the
//             remaining bits of its mask, finds its best row by (iou desc, row asc) and offers (iou bits, ~slot) to each of them with a
//             64-bit LDS max -- the row's best track by (iou desc, slot asc).  A track whose best row names it back commits.  The first
//             remaining pair of the total order is always such a pair, so a round without a commit ends the match; a pair that commits
//             precedes every pair it conflicts with, so the result is the sort-and-scan's.  The maximum and the taken-rows bit mask
//             (an LDS or) are order-free: the result depends on the inputs alone.
//     build   ballot / popcount prefix counts over the threads give every live row its place, every new row its id and every surviving
//             track its place behind the rows; the new list, the header and ids_out are written from registers and LDS.  Every read of
//             the state precedes a barrier that precedes every write of it.
// Compiled with -ffp-contract=off: the IoU is single fp32 operations, each rounded on its own (the expression of ore_proposal_recall).
#include "ore_track.h"                               // the state's layout and the IoU, shared with ore_track_wide.hip

namespace {

constexpr int TR_MAX_ROWS = ORE_DET_RECORD_ROWS;
constexpr int TR_MAX_T = ORE_TRACK_MAX_TRACKS;       // threads of the block: one per track slot
constexpr int TR_WORDS = (TR_MAX_ROWS + 63) / 64;    // 64-bit words of a row mask
static_assert(TR_MAX_ROWS <= TR_MAX_T && TR_MAX_T % 64 == 0 && TR_MAX_T <= 1024, "one thread per row and per track slot");

struct UpdArgs {
    void* state; int32_t capacity;
    const float* boxes; const float* scores; const int64_t* classes; const int32_t* n_dev; int32_t n_host, max_rows;
    float score_thresh, iou_thresh; int32_t ttl, class_aware; int64_t* ids_out;
};


__global__ __launch_bounds__(TR_MAX_T) void k_track_reset(void* state, int capacity) {
    const State s = track_state(state, capacity);
    const int t = threadIdx.x;
    if (t == 0) *s.hd = Header{0, capacity, 0, 0, 0};
    for (int j = t; j < capacity; j += blockDim.x) {
        *reinterpret_cast<f32x4*>(s.boxes + (size_t)j * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
        s.classes[j] = 0; s.ids[j] = 0; s.ttl[j] = 0;
    }
}

__global__ __launch_bounds__(TR_MAX_T) void k_track_update(const UpdArgs a) {
    __shared__ __attribute__((aligned(16))) f32x4 s_box[TR_MAX_ROWS];
    __shared__ float s_area[TR_MAX_ROWS];
    __shared__ long long s_cls[TR_MAX_ROWS];
    __shared__ unsigned long long s_key[TR_MAX_ROWS];           // the best offer of a round: (iou bits << 32) | ~slot
    __shared__ int s_match[TR_MAX_ROWS];                        // the track slot a row was matched to, -1: none
    __shared__ long long s_rowid[TR_MAX_ROWS];                  // the id a live row ends up with
    __shared__ unsigned long long s_live[TR_WORDS], s_taken[TR_WORDS];
    __shared__ int s_wsum[TR_MAX_T / 64][3];
    __shared__ int s_changed;

    const State st = track_state(a.state, a.capacity);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int n = a.n_dev ? *a.n_dev : a.n_host;
    n = n < 0 ? 0 : (n > a.max_rows ? a.max_rows : n);
    const Header hd = *st.hd;
    const int m = hd.m < 0 ? 0 : (hd.m > a.capacity ? a.capacity : hd.m);

    // ---- stage: the rows into LDS, the thread's track into registers
    if (t < TR_WORDS) { s_live[t] = 0ull; s_taken[t] = 0ull; }
    __syncthreads();
    bool live = false;
    f32x4 rb = {0.f, 0.f, 0.f, 0.f};
    long long rcls = 0;
    if (t < n) {
        rb = *reinterpret_cast<const f32x4*>(a.boxes + (size_t)t * 4);
        const float sc = a.scores[t];
        rcls = a.classes ? (long long)a.classes[t] : 0ll;
        live = finite32(rb.x) && finite32(rb.y) && finite32(rb.z) && finite32(rb.w) && finite32(sc) && sc >= a.score_thresh;
    }
    if (t < TR_MAX_ROWS) {
        s_box[t] = rb;
        s_area[t] = (rb.z - rb.x) * (rb.w - rb.y);
        s_cls[t] = rcls;
        s_match[t] = -1;
        const unsigned long long bal = __ballot(live);          // waves 0 .. 4 are whole: 320 = 5 x 64
        if (lane == 0) s_live[wave] = bal;
    }
    f32x4 tb = {0.f, 0.f, 0.f, 0.f};
    long long tcls = 0, tid = 0;
    int tttl = 0;
    if (t < m) {
        tb = *reinterpret_cast<const f32x4*>(st.boxes + (size_t)t * 4);
        tcls = st.classes[t]; tid = st.ids[t]; tttl = st.ttl[t];
    }
    const float tarea = (tb.z - tb.x) * (tb.w - tb.y);
    __syncthreads();

    auto iou_with = [&](int d) -> float { return track_iou(tb, tarea, s_box[d], s_area[d]); };

    // ---- scan: the candidate rows of this track
    unsigned long long cand[TR_WORDS];
#pragma unroll
    for (int w = 0; w < TR_WORDS; ++w) cand[w] = 0ull;
    if (t < m) {
#pragma unroll
        for (int w = 0; w < TR_WORDS; ++w) {
            unsigned long long rest = s_live[w];                // the same for every lane: a uniform loop
            unsigned long long c = 0ull;
            while (rest) {
                const int bit = __builtin_ctzll(rest);
                rest &= rest - 1ull;
                const int d = w * 64 + bit;
                if (iou_with(d) > a.iou_thresh && (!a.class_aware || s_cls[d] == tcls)) c |= 1ull << bit;
            }
            cand[w] = c;
        }
    }

    // ---- rounds of mutually best pairs
    bool active = false, matched = false;
#pragma unroll
    for (int w = 0; w < TR_WORDS; ++w) active = active || cand[w] != 0ull;
    for (int round = 0; round <= n; ++round) {                  // at least one commit per round that goes on: at most n + 1 rounds
        if (t < TR_MAX_ROWS) s_key[t] = 0ull;
        if (t == 0) s_changed = 0;
        __syncthreads();
        float best = 0.0f;
        int best_d = -1;
        if (active) {
#pragma unroll
            for (int w = 0; w < TR_WORDS; ++w) {
                unsigned long long rest = cand[w] & ~s_taken[w];
                cand[w] = rest;
                while (rest) {
                    const int bit = __builtin_ctzll(rest);
                    rest &= rest - 1ull;
                    const int d = w * 64 + bit;
                    const float v = iou_with(d);                // > iou_thresh >= 0: positive, its bits order as unsigned
                    atomicMax(&s_key[d], ((unsigned long long)__builtin_bit_cast(uint32_t, v) << 32) | (uint32_t)~(uint32_t)t);
                    if (v > best) { best = v; best_d = d; }     // rows ascending: the first of equal IoUs stays
                }
            }
            active = best_d >= 0;
        }
        __syncthreads();
        if (active && s_key[best_d] == (((unsigned long long)__builtin_bit_cast(uint32_t, best) << 32) | (uint32_t)~(uint32_t)t)) {
            s_match[best_d] = t;
            s_rowid[best_d] = tid;
            atomicOr(&s_taken[best_d >> 6], 1ull << (best_d & 63));
            matched = true; active = false;
            s_changed = 1;
        }
        __syncthreads();
        const int changed = s_changed;
        __syncthreads();                                        // everyone has read the flag before the next round clears it
        if (!changed) break;
    }

    // ---- build: places of the live rows, ids of the new ones, places of the surviving tracks
    const bool isnew = live && s_match[t < TR_MAX_ROWS ? t : 0] < 0;
    const int nttl = tttl - 1;
    const bool surv = t < m && !matched && nttl > 0;
    const unsigned long long b0 = __ballot(live), b1 = __ballot(isnew), b2 = __ballot(surv);
    if (lane == 0) { s_wsum[wave][0] = __popcll(b0); s_wsum[wave][1] = __popcll(b1); s_wsum[wave][2] = __popcll(b2); }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    int p_live = __popcll(b0 & below), p_new = __popcll(b1 & below), p_surv = __popcll(b2 & below);
    int n_live = 0, n_new = 0, n_surv = 0;
    const int waves = (blockDim.x + 63) >> 6;
    for (int w = 0; w < waves; ++w) {
        const int c0 = s_wsum[w][0], c1 = s_wsum[w][1], c2 = s_wsum[w][2];
        if (w < wave) { p_live += c0; p_new += c1; p_surv += c2; }
        n_live += c0; n_new += c1; n_surv += c2;
    }
    long long rid = -1;
    if (live) rid = isnew ? hd.next_id + p_new : s_rowid[t];
    if (t < a.max_rows) a.ids_out[t] = rid;
    if (live && p_live < a.capacity) {
        *reinterpret_cast<f32x4*>(st.boxes + (size_t)p_live * 4) = rb;
        st.classes[p_live] = rcls; st.ids[p_live] = rid; st.ttl[p_live] = a.ttl;
    }
    const int p_trk = n_live + p_surv;
    if (surv && p_trk < a.capacity) {
        *reinterpret_cast<f32x4*>(st.boxes + (size_t)p_trk * 4) = tb;
        st.classes[p_trk] = tcls; st.ids[p_trk] = tid; st.ttl[p_trk] = nttl;
    }
    const int total = n_live + n_surv, m_new = total < a.capacity ? total : a.capacity;
    if (t >= m_new && t < a.capacity) {                         // the slots behind the list hold zeros
        *reinterpret_cast<f32x4*>(st.boxes + (size_t)t * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
        st.classes[t] = 0; st.ids[t] = 0; st.ttl[t] = 0;
    }
    if (t == 0) *st.hd = Header{m_new, a.capacity, hd.next_id + n_new, hd.frames + 1, hd.dropped + (total - m_new)};
}

bool disjoint(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return !p || !q || np == 0 || nq == 0 || a + np <= b || b + nq <= a;
}

}  // namespace

extern "C" size_t ore_track_state_bytes(int32_t capacity) {
    return capacity >= 1 && capacity <= TR_MAX_T ? track_state_bytes(capacity) : 0;
}

extern "C" size_t ore_track_workspace_bytes(int32_t capacity, int32_t max_rows) {
    (void)capacity; (void)max_rows;
    return 0;                                                   // everything the update needs fits in LDS and registers
}

extern "C" int ore_track_reset(void* state, int32_t capacity, void* stream) {
    ORE_CHECK_ARG(capacity >= 1 && capacity <= TR_MAX_T, "ore_track_reset: capacity %d (1 .. %d)", capacity, TR_MAX_T);
    ORE_CHECK_ARG(state && (uintptr_t)state % 16 == 0, "ore_track_reset: the state is a 16-byte aligned device buffer");
    k_track_reset<<<1, round_up(capacity, 64), 0, (hipStream_t)stream>>>(state, capacity);
    return ore_launch_status("k_track_reset");
}

extern "C" int ore_track_update_fwd(void* state, int32_t capacity, const float* boxes, const float* scores, const int64_t* classes,
                                    const int32_t* n_dev, int32_t n_host, int32_t max_rows, float score_thresh, float iou_thresh,
                                    int32_t ttl, int32_t class_aware, int64_t* ids_out, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    (void)workspace; (void)workspace_bytes;
    ORE_CHECK_ARG(capacity >= 1 && capacity <= TR_MAX_T, "ore_track_update_fwd: capacity %d (1 .. %d)", capacity, TR_MAX_T);
    ORE_CHECK_ARG(state && (uintptr_t)state % 16 == 0, "ore_track_update_fwd: the state is a 16-byte aligned device buffer");
    ORE_CHECK_ARG(max_rows >= 0 && max_rows <= TR_MAX_ROWS && (n_dev || n_host >= 0), "ore_track_update_fwd: max_rows %d (0 .. %d), n_host %d",
                  max_rows, TR_MAX_ROWS, n_host);
    ORE_CHECK_ARG(max_rows == 0 || (boxes && scores && ids_out), "ore_track_update_fwd: null rows");
    ORE_CHECK_ARG(max_rows == 0 || ((uintptr_t)boxes % 16 == 0 && (uintptr_t)ids_out % 8 == 0), "ore_track_update_fwd: boxes 16-byte, ids_out 8-byte aligned");
    ORE_CHECK_ARG(ttl >= 1 && ttl <= (1 << 20), "ore_track_update_fwd: ttl %d (1 .. %d)", ttl, 1 << 20);
    ORE_CHECK_ARG(iou_thresh >= 0.0f && iou_thresh <= 3.0e38f, "ore_track_update_fwd: iou_thresh is finite and >= 0");
    ORE_CHECK_ARG(score_thresh == score_thresh, "ore_track_update_fwd: score_thresh is NaN");
    const size_t sb = track_state_bytes(capacity), r = (size_t)max_rows;
    const void* arr[5] = {state, ids_out, boxes, scores, classes};
    const size_t len[5] = {sb, r * 8, r * 16, r * 4, r * 8};
    for (int i = 0; i < 2; ++i)                                 // the two buffers written, against each other and every input
        for (int j = i + 1; j < 5; ++j)
            ORE_CHECK_ARG(disjoint(arr[i], len[i], arr[j], len[j]), "ore_track_update_fwd: state, ids_out and the row arrays must be disjoint");
    const int threads = round_up(capacity > max_rows ? capacity : max_rows, 64);
    UpdArgs a{state, capacity, boxes, scores, classes, n_dev, n_host, max_rows, score_thresh, iou_thresh, ttl, class_aware ? 1 : 0, ids_out};
    k_track_update<<<1, threads, 0, (hipStream_t)stream>>>(a);
    return ore_launch_status("k_track_update");
}
