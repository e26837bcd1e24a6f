// Rule 8 of lp_track_update for the stages that read the tracker state behind it (lp_watch_live.hip, lp_zones.hip): the layout of a
// stream's state, restated from lp_track.hip (16 header words, 544 words per slot), and the read of one head of one slot.  Tests pin
// it to the tracker's own read_head (tests/test_watch_live_gpu.py, tests/test_zones_gpu.py).
#pragma once

namespace lp {

namespace {

constexpr int TR_SLOTS = LP_TRACK_MAX_TRACKS;   // 128
constexpr int TR_HEADS = 8;
constexpr int TR_HDR_WORDS = 16, TR_W_BOX = 8, TR_W_TOTAL = 24, TR_W_VOTES = 32;
constexpr int TR_SLOT_WORDS = TR_W_VOTES + TR_HEADS * LP_TRACK_MAX_CLS;
static_assert(TR_SLOT_WORDS == 544 && TR_SLOTS == 128 && LP_TRACK_MAX_CLS == 64, "lp_track_read.inc restates the state layout of lp_track.hip");

// head `head` of the slot at `sl`: the argmax over nc <= 64 floats, lowest index on a tie, and its share of the head's total
__device__ __forceinline__ void track_read_head(const int* __restrict__ sl, int head, int nc, int& best, float& share) {
    const float* v = (const float*)(sl + TR_W_VOTES + head * LP_TRACK_MAX_CLS);
    int bi = 0;
    float bv = v[0];
#pragma unroll 4
    for (int c = 1; c < nc; ++c) {
        const float x = v[c];
        if (x > bv) { bv = x; bi = c; }
    }
    const float tot = __int_as_float(sl[TR_W_TOTAL + head]);
    best = bi;
    share = tot > 0.f ? bv / tot : 0.f;
}

}  // namespace

}  // namespace lp
