// What the two forms of the tracker ("track v1", include/ore_hip.h) share: the layout of the caller's state buffer and the contract's
// fp32 IoU.  ore_track.hip (one workgroup, 320 rows x 1024 tracks) and ore_track_wide.hip (the whole chip, 8192 rows x 16384 tracks)
// include this file and are both compiled with -ffp-contract=off, so the two cannot drift: one expression, one layout.
#pragma once
#include "ore_block.h"

namespace {

constexpr int TR_HEADER = 32;                        // bytes: m, capacity (int32), next_id, frames, dropped (int64)

struct Header { int32_t m, capacity; int64_t next_id, frames, dropped; };
static_assert(sizeof(Header) == TR_HEADER, "the documented header");
struct State { Header* hd; float* boxes; int64_t* classes; int64_t* ids; int32_t* ttl; };
__host__ __device__ inline State track_state(void* p, int capacity) {
    char* c = static_cast<char*>(p);
    State s;
    s.hd = reinterpret_cast<Header*>(c);
    s.boxes = reinterpret_cast<float*>(c + TR_HEADER);
    s.classes = reinterpret_cast<int64_t*>(c + TR_HEADER + (size_t)capacity * 16);
    s.ids = s.classes + capacity;
    s.ttl = reinterpret_cast<int32_t*>(s.ids + capacity);
    return s;
}
inline size_t track_state_bytes(int capacity) { return ((size_t)TR_HEADER + (size_t)capacity * 36 + 15) & ~(size_t)15; }

// area = (x1 - x0) * (y1 - y0): a subtraction each, then a product
__device__ __forceinline__ float track_area(const f32x4 b) { return (b.z - b.x) * (b.w - b.y); }

// the contract's IoU of a track box and a row box with their areas: every operation a single fp32 operation
__device__ __forceinline__ float track_iou(const f32x4 tb, const float tarea, const f32x4 b, const float barea) {
    const float iw = fminf(tb.z, b.z) - fmaxf(tb.x, b.x), ih = fminf(tb.w, b.w) - fmaxf(tb.y, b.y);
    const float inter = (iw > 0.0f && ih > 0.0f) ? iw * ih : 0.0f;
    return inter > 0.0f ? inter / ((tarea + barea) - inter) : 0.0f;
}

// a row takes part: its four coordinates and its score are finite, and the score reaches the threshold
__device__ __forceinline__ bool track_row_live(const f32x4 b, const float sc, const float score_thresh) {
    return finite32(b.x) && finite32(b.y) && finite32(b.z) && finite32(b.w) && finite32(sc) && sc >= score_thresh;
}

inline bool track_disjoint(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return !p || !q || np == 0 || nq == 0 || a + np <= b || b + nq <= a;
}

}  // namespace
