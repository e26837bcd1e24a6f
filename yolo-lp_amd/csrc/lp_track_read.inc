// The device pieces of a stage that walks the live tracks of lp_track_update's state: track_kernel itself (lp_track.hip) and the stages
// behind it (lp_watch_live.hip, lp_zones.hip, lp_speed.hip).  The layouts and the TrackNcls argument are lp_streams.h's; here are rule 8
// (the read of one head of one slot: the only copy, the tracker's own vote step calls it), the read of the heads a stage needs, the key
// of a read, the numbering of events in slot order, the tail of an event list, the wrapping difference, the finite-anchor test and the
// (slot, head) share of an ended record.  Each compiles to what its callers had written out (profiles/live_stage_codegen.txt, which
// also names what stayed written out); geometry, memo layouts, event contents and what lies between these phases stay in the stages' files.
#pragma once

namespace lp {

namespace {

// rule 8, head `head` of the slot at `sl`: the argmax over nc <= 64 floats, lowest index on a tie, and its share of the head's total
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

// rule 8 for the slots marked in s_need[0..T), one (slot, head) per thread and round, the voted ids to s_best[slot * 8 + head].
// `slots`: the stream's slot 0.  The caller puts a barrier in front (s_need) and behind (s_best).
template <int THREADS>
__device__ __forceinline__ void read_needed_heads(const int* __restrict__ slots, int T, const TrackNcls& ncls, const int* s_need, int* s_best) {
    for (int i = threadIdx.x; i < T * TR_HEADS; i += THREADS) {
        const int slot = i >> 3, head = i & 7;
        if (s_need[slot]) {
            int bi;
            float sh;
            track_read_head(slots + (long long)slot * TR_SLOT_WORDS, head, ncls.v[head], bi, sh);
            s_best[i] = bi;
        }
    }
}

// the key of a read: the eight voted ids, one byte each, heads 0..3 in key_lo and 4..7 in key_hi
__device__ __forceinline__ void pack_key(const int* ids, unsigned& lo, unsigned& hi) {
    lo = hi = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        lo |= (unsigned)ids[p] << (8 * p);
        hi |= (unsigned)ids[4 + p] << (8 * p);
    }
}

// ---- numbering events in slot order over the 128 slot threads (two waves) -----------------------------------------------------------
// The inclusive sum of `cnt` within the wave, the wave's sum left in s_wsum[wave].  Behind the caller's barrier the events
// of a thread start at events_before(), and s_wsum[0] + s_wsum[1] is their number.
__device__ __forceinline__ int wave_inclusive_sum(int cnt, int lane, int wave, int* s_wsum) {
    int incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(incl, d, 64);
        if (lane >= d) incl += u;
    }
    if (lane == 63) s_wsum[wave] = incl;
    return incl;
}
__device__ __forceinline__ int events_before(int incl, int cnt, int wave, const int* s_wsum) { return (wave == 1 ? s_wsum[0] : 0) + incl - cnt; }

// the lines of an event list from the count (total >= 0) to max_events are zero, and the count goes out uncapped
template <int THREADS, int COLS>
__device__ __forceinline__ void close_event_list(int32_t* __restrict__ ev, int total, int max_events, int32_t* __restrict__ count) {
    for (long long w = (long long)total * COLS + threadIdx.x; w < (long long)max_events * COLS; w += THREADS) ev[w] = 0;
    if (threadIdx.x == 0) *count = total;
}

__device__ __forceinline__ int wrap_diff(int a, int b) { return (int)((unsigned)a - (unsigned)b); }      // a - b of frame numbers or ids, wraps

// an anchor (or any pair) without NaN and infinity
__device__ __forceinline__ bool finite_pair(float x, float y) { return fabsf(x) <= 3.4028234663852886e38f && fabsf(y) <= 3.4028234663852886e38f; }

// the share of thread (slot, head) in the ended record of the slot at `sl`: the head's voted id and share, and for head < 4 one word
// of (id, first, last, hits) and of the box
__device__ __forceinline__ void write_record_share(int32_t* __restrict__ ri, float* __restrict__ rf, const int* sl, int head, int best, float share) {
    ri[RM_W_IDS + head] = best;
    rf[RM_F_SHARES + head] = share;
    if (head < 4) { ri[RM_W_TRACK + head] = sl[head]; rf[RM_F_BOX + head] = __int_as_float(sl[TR_W_BOX + head]); }
}

}  // namespace

}  // namespace lp
