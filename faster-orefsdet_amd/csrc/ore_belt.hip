// The belt's shift ("belt shift v1", include/ore_hip.h): before the tracker associates a frame, the one translation the whole frame
// shares is voted from the boxes alone and every track box is moved by it.  Every (track, row) pair of equal class and similar size
// adds 1 to the bin of its centre displacement; true pairs pile into one bin, false pairs spread over the window.  The launches sit on
// the pass's stream between the detection record and the "track v1" update, which then associates as it always has.
//   k_belt_reset        the 64-byte belt state
//   form 1  k_belt_one  ONE launch of ONE workgroup (capacity <= ORE_TRACK_MAX_TRACKS, max_rows <= ORE_DET_RECORD_ROWS): the rows that
//                       can vote are staged in LDS, compacted; a thread walks them with its track (the row is the same for a whole
//                       wave: LDS broadcasts) and votes with an integer LDS add into the (2K + 1)^2 histogram in LDS (66,564 B at K = 64); then
//                       the finish below.
//   form 2  k_belt_vote the votes on the whole chip: a block takes work items (1024 tracks, one per thread) x (64 rows, staged in LDS)
//                       in a strided loop and votes into its OWN LDS histogram; at the end it adds its non-zero bins to the histogram
//                       in the workspace with one integer global atomic per bin (contiguous bins per wave instruction).  The nine bins
//                       that hold the true pairs so take one add per block, not one per pair.  <DIRECT = true> votes straight into the
//                       workspace instead (form 3: the A/B aid tools/bench_belt.py times).
//           k_belt_finish  one workgroup: the workspace histogram into LDS, then the finish.
//   finish  smoothing (3x3 sum, bins outside the window count 0) and the arg-max over (S descending, distance to the previous shift
//           ascending, qy, qx ascending) per thread over strided bins, then over the wave by shuffles and over the waves in LDS; thread 0
//           decides, writes the belt state and broadcasts (dx, dy); every track box is moved and tested against the frame.
// Integer adds commute: the counts, hence everything, are a function of the inputs alone.  Compiled with -ffp-contract=off: the gates
// are single fp32 operations (the product with 1 / (2 bin), a power of two, is exact either way).
#include "ore_track.h"                               // the state's layout and track_row_live, shared with the trackers

namespace {

constexpr int BL_MAX_K = ORE_BELT_MAX_HALF_BINS;
constexpr int BL_MAX_BINS = (2 * BL_MAX_K + 1) * (2 * BL_MAX_K + 1);
constexpr int BL_THREADS = 1024;
constexpr int BL_ONE_ROWS = ORE_DET_RECORD_ROWS, BL_ONE_T = ORE_TRACK_MAX_TRACKS;
constexpr int BL_ONE_WORDS = (BL_ONE_ROWS + 63) / 64;
constexpr int BL_TILE_ROWS = 64;                     // rows of a form-2 work item: one word of live bits
constexpr int BL_MAX_BLOCKS = 256;                   // of k_belt_vote: one per CU
constexpr int BL_STATE_BYTES = 64;
static_assert(BL_ONE_T <= BL_THREADS && BL_ONE_ROWS <= BL_THREADS, "form 1: one thread per track slot and per row");

struct BeltState { int32_t dx, dy, votes, reserved; int64_t travel_x, travel_y, frames, coasted; int64_t zero[2]; };
static_assert(sizeof(BeltState) == BL_STATE_BYTES, "the documented belt state");

struct BeltArgs {
    BeltState* belt; void* state; int32_t capacity;
    const float* boxes; const float* scores; const int64_t* classes; const int32_t* n_dev; int32_t n_host, max_rows;
    float score_thresh; int32_t class_aware, bin, half_bins; float size_tol, inv; int32_t min_votes, frame_h, frame_w;
    int32_t* hist;                                   // form 2: (2K + 1)^2 int32 in the workspace
};

__device__ __forceinline__ int belt_rows(const BeltArgs& a) {
    const int n = a.n_dev ? *a.n_dev : a.n_host;
    return n < 0 ? 0 : (n > a.max_rows ? a.max_rows : n);
}
__device__ __forceinline__ int belt_tracks(const BeltArgs& a, const Header& hd) {
    return hd.m < 0 ? 0 : (hd.m > a.capacity ? a.capacity : hd.m);
}

// (w, h, sx, sy) of a box: one fp32 operation each
__device__ __forceinline__ f32x4 belt_geo(const f32x4 b) { return f32x4{b.z - b.x, b.w - b.y, b.x + b.z, b.y + b.w}; }

// the bin of the pair (track geometry tg, row geometry rg), or -1: the window and the size gate, the classes and the extents aside.
// The conditions are a conjunction, so their order is free: the window in x comes first -- five instructions that most pairs of a wide
// frame fail -- and a wave whose 64 tracks all fail it skips the rest.
__device__ __forceinline__ int belt_bin(const f32x4 tg, const f32x4 rg, const float tol, const float inv, const int K) {
    const float fk = (float)K;
    const float qx = floorf((rg.z - tg.z) * inv + 0.5f);
    if (!(fabsf(qx) <= fk)) return -1;                          // NaN and inf fail
    const float qy = floorf((rg.w - tg.w) * inv + 0.5f);
    if (!(fabsf(qy) <= fk)) return -1;
    if (!(fabsf(tg.x - rg.x) <= tol * fmaxf(tg.x, rg.x)) || !(fabsf(tg.y - rg.y) <= tol * fmaxf(tg.y, rg.y))) return -1;
    return ((int)qy + K) * (2 * K + 1) + ((int)qx + K);
}

// One workgroup of BL_THREADS threads, `hist` = the (2K + 1)^2 counts in LDS, complete and visible (a barrier behind the last add).
__device__ __forceinline__ void belt_finish(const int* hist, const BeltArgs& a, const int m) {
    __shared__ int s_bs[BL_THREADS / 64], s_bi[BL_THREADS / 64];
    __shared__ long long s_bd[BL_THREADS / 64];
    __shared__ int s_shift[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.half_bins, W = 2 * K + 1, nb = W * W;
    const BeltState old = *a.belt;
    int bs = -1, bi = 0x7fffffff;
    long long bd = 0;
    for (int i = tid; i < nb; i += BL_THREADS) {
        const int y = i / W, x = i - y * W;
        int s = 0;
#pragma unroll
        for (int dv = -1; dv <= 1; ++dv)
#pragma unroll
            for (int du = -1; du <= 1; ++du) {                  // nine independent LDS reads; outside the window: 0
                const int v = y + dv, u = x + du;
                s += ((unsigned)v < (unsigned)W && (unsigned)u < (unsigned)W) ? hist[v * W + u] : 0;
            }
        const long long ex = (long long)(x - K) * a.bin - old.dx, ey = (long long)(y - K) * a.bin - old.dy;
        const long long d = (ex < 0 ? -ex : ex) + (ey < 0 ? -ey : ey);
        if (s > bs || (s == bs && d < bd)) { bs = s; bd = d; bi = i; }      // bins ascending: the first of equal keys stays
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int os = __shfl_xor(bs, o), oi = __shfl_xor(bi, o);
        const long long od = __shfl_xor(bd, o);
        if (os > bs || (os == bs && (od < bd || (od == bd && oi < bi)))) { bs = os; bd = od; bi = oi; }
    }
    if (lane == 0) { s_bs[wave] = bs; s_bd[wave] = bd; s_bi[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < BL_THREADS / 64; ++w) {
            const int os = s_bs[w], oi = s_bi[w];
            const long long od = s_bd[w];
            if (os > bs || (os == bs && (od < bd || (od == bd && oi < bi)))) { bs = os; bd = od; bi = oi; }
        }
        BeltState nw = old;
        if (bs >= a.min_votes) {
            const int y = bi / W, x = bi - y * W;
            nw.dx = (x - K) * a.bin; nw.dy = (y - K) * a.bin; nw.votes = bs;
        } else {
            nw.votes = 0; nw.coasted = old.coasted + 1;
        }
        nw.reserved = 0; nw.zero[0] = 0; nw.zero[1] = 0;
        nw.travel_x = old.travel_x + nw.dx; nw.travel_y = old.travel_y + nw.dy; nw.frames = old.frames + 1;
        *a.belt = nw;
        s_shift[0] = nw.dx; s_shift[1] = nw.dy;
    }
    __syncthreads();
    const float dx = (float)s_shift[0], dy = (float)s_shift[1];
    const bool framed = a.frame_h > 0 || a.frame_w > 0;
    const float fw = (float)a.frame_w, fh = (float)a.frame_h;
    const State st = track_state(a.state, a.capacity);
    for (int t = tid; t < m; t += BL_THREADS) {
        f32x4 b = *reinterpret_cast<const f32x4*>(st.boxes + (size_t)t * 4);
        b.x += dx; b.z += dx; b.y += dy; b.w += dy;
        *reinterpret_cast<f32x4*>(st.boxes + (size_t)t * 4) = b;
        if (framed && (b.z <= 0.0f || b.x >= fw || b.w <= 0.0f || b.y >= fh)) st.ttl[t] = 1;   // a NaN compares false: the track stays
    }
}

__global__ __launch_bounds__(64) void k_belt_reset(BeltState* belt) {
    if (threadIdx.x == 0) *belt = BeltState{0, 0, 0, 0, 0, 0, 0, 0, {0, 0}};
}

// form 1: dynamic LDS = (2K + 1)^2 int32
__global__ __launch_bounds__(BL_THREADS) void k_belt_one(const BeltArgs a) {
    extern __shared__ __attribute__((aligned(16))) int s_hist[];
    __shared__ __attribute__((aligned(16))) f32x4 s_geo[BL_ONE_ROWS];
    __shared__ long long s_cls[BL_ONE_ROWS];
    __shared__ int s_wcnt[BL_ONE_WORDS];                        // the voting rows of each staging wave

    const State st = track_state(a.state, a.capacity);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = belt_rows(a), m = belt_tracks(a, *st.hd);
    const int K = a.half_bins, nb = (2 * K + 1) * (2 * K + 1);
    for (int i = tid; i < nb; i += BL_THREADS) s_hist[i] = 0;
    // the rows that can vote (live, both extents > 0), compacted in LDS: the vote loop is then a counted loop over them, which the
    // compiler unrolls so that the LDS reads of several rows are in flight at once.  The order of the votes does not matter.
    bool ok = false;
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    long long c = 0;
    int rank = 0;
    if (tid < BL_ONE_WORDS * 64) {                              // whole waves: 320 = 5 x 64
        if (tid < n) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(a.boxes + (size_t)tid * 4);
            g = belt_geo(b);
            c = a.classes ? (long long)a.classes[tid] : 0ll;
            ok = track_row_live(b, a.scores[tid], a.score_thresh) && g.x > 0.0f && g.y > 0.0f;
        }
        const unsigned long long bal = __ballot(ok);
        rank = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_wcnt[wave] = __popcll(bal);
    }
    __syncthreads();
    int nvote = 0;
#pragma unroll
    for (int w = 0; w < BL_ONE_WORDS; ++w) {
        const int cnt = s_wcnt[w];
        if (w < wave) rank += cnt;
        nvote += cnt;
    }
    if (ok) { s_geo[rank] = g; s_cls[rank] = c; }               // rank < nvote <= BL_ONE_ROWS
    __syncthreads();
    if (tid < m) {
        const f32x4 tg = belt_geo(*reinterpret_cast<const f32x4*>(st.boxes + (size_t)tid * 4));
        const long long tcls = st.classes[tid];
        if (tg.x > 0.0f && tg.y > 0.0f) {
#pragma unroll 4
            for (int j = 0; j < nvote; ++j) {                   // the same row for every lane: LDS broadcasts
                const int bin = belt_bin(tg, s_geo[j], a.size_tol, a.inv, K);
                if (bin >= 0 && (!a.class_aware || s_cls[j] == tcls)) atomicAdd(&s_hist[bin], 1);
            }
        }
    }
    __syncthreads();
    belt_finish(s_hist, a, m);
}

// form 2, the votes.  Work item i = (track group i / row_tiles, row tile i % row_tiles); block b takes items b, b + gridDim.x, ...
template <bool DIRECT>
__global__ __launch_bounds__(BL_THREADS) void k_belt_vote(const BeltArgs a) {
    extern __shared__ __attribute__((aligned(16))) int s_hist[];            // DIRECT: unused (0 bytes)
    __shared__ __attribute__((aligned(16))) f32x4 s_geo[BL_TILE_ROWS];
    __shared__ long long s_cls[BL_TILE_ROWS];
    __shared__ int s_nvote;                                     // the voting rows of the tile, compacted in s_geo / s_cls

    const State st = track_state(a.state, a.capacity);
    const int tid = threadIdx.x;
    const int n = belt_rows(a), m = belt_tracks(a, *st.hd);
    const int K = a.half_bins, nb = (2 * K + 1) * (2 * K + 1);
    const int row_tiles = (n + BL_TILE_ROWS - 1) / BL_TILE_ROWS, groups = (m + BL_THREADS - 1) / BL_THREADS;
    const int items = row_tiles * groups;
    if ((int)blockIdx.x >= items) return;                       // uniform: nothing to vote, nothing to flush
    if (!DIRECT) {
        for (int i = tid; i < nb; i += BL_THREADS) s_hist[i] = 0;
    }
    int* const hist = DIRECT ? a.hist : s_hist;
    int group = -1;
    f32x4 tg = {0.f, 0.f, 0.f, 0.f};
    long long tcls = 0;
    bool tok = false;
    for (int item = blockIdx.x; item < items; item += gridDim.x) {
        const int g = item / row_tiles, r0 = (item - g * row_tiles) * BL_TILE_ROWS;
        __syncthreads();                                        // the tile before has been read; the first time: the clear is done
        if (tid < BL_TILE_ROWS) {                               // wave 0
            const int d = r0 + tid;
            bool ok = false;
            f32x4 rg = {0.f, 0.f, 0.f, 0.f};
            long long c = 0;
            if (d < n) {
                const f32x4 b = *reinterpret_cast<const f32x4*>(a.boxes + (size_t)d * 4);
                rg = belt_geo(b);
                c = a.classes ? (long long)a.classes[d] : 0ll;
                ok = track_row_live(b, a.scores[d], a.score_thresh) && rg.x > 0.0f && rg.y > 0.0f;
            }
            const unsigned long long bal = __ballot(ok);
            if (ok) {
                const int rank = __popcll(bal & ((1ull << tid) - 1ull));
                s_geo[rank] = rg; s_cls[rank] = c;
            }
            if (tid == 0) s_nvote = __popcll(bal);
        }
        if (g != group) {
            group = g;
            const int t = g * BL_THREADS + tid;
            tok = false;
            if (t < m) {
                tg = belt_geo(*reinterpret_cast<const f32x4*>(st.boxes + (size_t)t * 4));
                tcls = st.classes[t];
                tok = tg.x > 0.0f && tg.y > 0.0f;
            }
        }
        __syncthreads();
        if (tok) {
            const int nvote = s_nvote;
#pragma unroll 4
            for (int j = 0; j < nvote; ++j) {
                const int bin = belt_bin(tg, s_geo[j], a.size_tol, a.inv, K);
                if (bin >= 0 && (!a.class_aware || s_cls[j] == tcls)) atomicAdd(&hist[bin], 1);
            }
        }
    }
    if (!DIRECT) {
        __syncthreads();
        for (int i = tid; i < nb; i += BL_THREADS) {
            const int v = s_hist[i];
            if (v) atomicAdd(&a.hist[i], v);
        }
    }
}

// form 2, the finish: dynamic LDS = (2K + 1)^2 int32
__global__ __launch_bounds__(BL_THREADS) void k_belt_finish(const BeltArgs a) {
    extern __shared__ __attribute__((aligned(16))) int s_hist[];
    const State st = track_state(a.state, a.capacity);
    const int m = belt_tracks(a, *st.hd);
    const int K = a.half_bins, nb = (2 * K + 1) * (2 * K + 1);
    for (int i = threadIdx.x; i < nb; i += BL_THREADS) s_hist[i] = a.hist[i];
    __syncthreads();
    belt_finish(s_hist, a, m);
}

bool belt_shape_ok(int32_t capacity, int32_t max_rows, int32_t half_bins) {
    return capacity >= 1 && capacity <= ORE_TRACK_WIDE_MAX_TRACKS && max_rows >= 0 && max_rows <= ORE_TRACK_WIDE_MAX_ROWS &&
           half_bins >= 1 && half_bins <= BL_MAX_K;
}
bool belt_one_takes(int32_t capacity, int32_t max_rows) { return capacity <= BL_ONE_T && max_rows <= BL_ONE_ROWS; }
size_t belt_hist_bytes(int32_t half_bins) {
    const size_t w = 2 * (size_t)half_bins + 1;
    return (w * w * 4 + 255) & ~(size_t)255;
}

// a histogram beyond the default dynamic LDS limit: raised once per kernel, to the largest window
template <void (*Kern)(const BeltArgs)>
int belt_lds() {
    static bool done = false;
    if (!done) {
        ORE_HIP(hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, BL_MAX_BINS * 4));
        done = true;
    }
    return ORE_OK;
}

}  // namespace

extern "C" size_t ore_belt_state_bytes(void) { return BL_STATE_BYTES; }

extern "C" int ore_belt_reset(void* belt, void* stream) {
    ORE_CHECK_ARG(belt && (uintptr_t)belt % 16 == 0, "ore_belt_reset: the belt state is a 16-byte aligned device buffer");
    k_belt_reset<<<1, 64, 0, (hipStream_t)stream>>>(static_cast<BeltState*>(belt));
    return ore_launch_status("k_belt_reset");
}

extern "C" size_t ore_belt_workspace_bytes(int32_t capacity, int32_t max_rows, int32_t half_bins) {
    return belt_shape_ok(capacity, max_rows, half_bins) ? belt_hist_bytes(half_bins) : 0;
}

extern "C" int ore_belt_shift_form(int32_t capacity, int32_t max_rows, int32_t half_bins) {
    ORE_CHECK_ARG(belt_shape_ok(capacity, max_rows, half_bins), "ore_belt_shift_form: capacity %d (1 .. %d), max_rows %d (0 .. %d), half_bins %d (1 .. %d)",
                  capacity, ORE_TRACK_WIDE_MAX_TRACKS, max_rows, ORE_TRACK_WIDE_MAX_ROWS, half_bins, BL_MAX_K);
    return belt_one_takes(capacity, max_rows) ? 1 : 2;
}

extern "C" int ore_belt_shift_fwd(void* belt, void* track_state_buf, int32_t capacity, const float* boxes, const float* scores,
                                  const int64_t* classes, const int32_t* n_dev, int32_t n_host, int32_t max_rows, float score_thresh,
                                  int32_t class_aware, int32_t bin, int32_t half_bins, float size_tol, int32_t min_votes,
                                  int32_t frame_h, int32_t frame_w, int32_t form, void* workspace, size_t workspace_bytes, void* stream) {
    ORE_CHECK_ARG(belt_shape_ok(capacity, max_rows, half_bins), "ore_belt_shift_fwd: capacity %d (1 .. %d), max_rows %d (0 .. %d), half_bins %d (1 .. %d)",
                  capacity, ORE_TRACK_WIDE_MAX_TRACKS, max_rows, ORE_TRACK_WIDE_MAX_ROWS, half_bins, BL_MAX_K);
    ORE_CHECK_ARG(n_dev || n_host >= 0, "ore_belt_shift_fwd: n_host %d", n_host);
    ORE_CHECK_ARG(form >= 0 && form <= 3, "ore_belt_shift_fwd: form %d (0: choose, 1, 2; 3: form 2 voting straight into the workspace)", form);
    ORE_CHECK_ARG(form != 1 || belt_one_takes(capacity, max_rows), "ore_belt_shift_fwd: form 1 takes capacity <= %d and max_rows <= %d, got %d and %d",
                  BL_ONE_T, BL_ONE_ROWS, capacity, max_rows);
    ORE_CHECK_ARG(bin == 1 || bin == 2 || bin == 4 || bin == 8 || bin == 16, "ore_belt_shift_fwd: bin %d (1, 2, 4, 8 or 16)", bin);
    ORE_CHECK_ARG(size_tol >= 0.0f && size_tol < 1.0f, "ore_belt_shift_fwd: size_tol is finite, >= 0 and < 1");
    ORE_CHECK_ARG(min_votes >= 1 && min_votes <= (1 << 30), "ore_belt_shift_fwd: min_votes %d (1 .. %d)", min_votes, 1 << 30);
    ORE_CHECK_ARG(frame_h >= 0 && frame_w >= 0 && (frame_h > 0) == (frame_w > 0), "ore_belt_shift_fwd: frame %d x %d (both 0: no frame test, or both > 0)",
                  frame_h, frame_w);
    ORE_CHECK_ARG(score_thresh == score_thresh, "ore_belt_shift_fwd: score_thresh is NaN");
    ORE_CHECK_ARG(belt && (uintptr_t)belt % 16 == 0, "ore_belt_shift_fwd: the belt state is a 16-byte aligned device buffer");
    ORE_CHECK_ARG(track_state_buf && (uintptr_t)track_state_buf % 16 == 0, "ore_belt_shift_fwd: the track state is a 16-byte aligned device buffer");
    ORE_CHECK_ARG(max_rows == 0 || (boxes && scores), "ore_belt_shift_fwd: null rows");
    ORE_CHECK_ARG(max_rows == 0 || (uintptr_t)boxes % 16 == 0, "ore_belt_shift_fwd: boxes 16-byte aligned");
    const int use = form ? form : (belt_one_takes(capacity, max_rows) ? 1 : 2);
    const size_t need = use == 1 ? 0 : belt_hist_bytes(half_bins);
    ORE_CHECK_ARG(use == 1 || (workspace && (uintptr_t)workspace % 256 == 0 && workspace_bytes >= need),
                  "ore_belt_shift_fwd: the workspace is a 256-byte aligned device buffer of %zu bytes (ore_belt_workspace_bytes), got %zu", need,
                  workspace_bytes);
    const size_t sb = track_state_bytes(capacity), r = (size_t)max_rows;
    const void* arr[6] = {belt, track_state_buf, use == 1 ? nullptr : workspace, boxes, scores, classes};
    const size_t len[6] = {BL_STATE_BYTES, sb, need, r * 16, r * 4, r * 8};
    for (int i = 0; i < 3; ++i)                                 // the three buffers written, against each other and every input
        for (int j = i + 1; j < 6; ++j)
            ORE_CHECK_ARG(track_disjoint(arr[i], len[i], arr[j], len[j]),
                          "ore_belt_shift_fwd: the belt state, the track state, the workspace and the row arrays must be disjoint");
    const int W = 2 * half_bins + 1;
    const size_t lds = (size_t)W * W * 4;
    BeltArgs a{static_cast<BeltState*>(belt), track_state_buf, capacity, boxes, scores, classes, n_dev, n_host, max_rows, score_thresh,
               class_aware ? 1 : 0, bin, half_bins, size_tol, 1.0f / (float)(2 * bin), min_votes, frame_h, frame_w,
               use == 1 ? nullptr : static_cast<int32_t*>(workspace)};
    hipStream_t s = (hipStream_t)stream;
    if (use == 1) {
        if (int rc = belt_lds<k_belt_one>()) return rc;
        k_belt_one<<<1, BL_THREADS, lds, s>>>(a);
        return ore_launch_status("k_belt_one");
    }
    ORE_HIP(hipMemsetAsync(workspace, 0, need, s));
    const int items = ceil_div(max_rows, BL_TILE_ROWS) * ceil_div(capacity, BL_THREADS);
    if (items > 0) {
        const int blocks = items < BL_MAX_BLOCKS ? items : BL_MAX_BLOCKS;
        if (use == 3) {
            k_belt_vote<true><<<blocks, BL_THREADS, 0, s>>>(a);
        } else {
            if (int rc = belt_lds<k_belt_vote<false>>()) return rc;
            k_belt_vote<false><<<blocks, BL_THREADS, lds, s>>>(a);
        }
        if (int rc = ore_launch_status("k_belt_vote")) return rc;
    }
    if (int rc = belt_lds<k_belt_finish>()) return rc;
    k_belt_finish<<<1, BL_THREADS, lds, s>>>(a);
    return ore_launch_status("k_belt_finish");
}
