// Host-side pieces shared by the per-stream entry points (lp_track.hip, lp_shots.hip, lp_lookback.hip; lp_watch_live.hip, lp_zones.hip,
// lp_speed.hip), the threshold rounding of lp_nms.hip and lp_tiles.hip, and the one statement of the tracker's state layout and of the
// ended record, read by host code and kernels alike.  No HIP header: tests/host_streams.cpp includes this file alone and runs on the CPU.
// A new per-stream kernel family takes its frame table from plan_streams and its argument checks from the *_fault functions
// (an empty string: fine; the caller hands the message to fail(), as with plane_fault and region_fault).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <cmath>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/lp_hip.h"

namespace lp {

// ---- the state of a stream of lp_track_update, in int32 / fp32 words (all zero = empty) ------------------------------------------------
// 16 header words (frame counter, next id, dropped), then per slot 544: id, first, last, hits, misses, 3 unused; box[4]; corners[8];
// vx, vy, 2 unused; total[8]; votes[8][64].  A slot is live iff hits > 0.
constexpr int TR_SLOTS = LP_TRACK_MAX_TRACKS;   // 128
constexpr int TR_HEADS = 8;
constexpr int TR_HDR_WORDS = 16;
constexpr int TR_W_BOX = 8, TR_W_COR = 12, TR_W_VEL = 20, TR_W_TOTAL = 24, TR_W_VOTES = 32;
constexpr int TR_SLOT_WORDS = TR_W_VOTES + TR_HEADS * LP_TRACK_MAX_CLS;   // 544
static_assert(TR_W_COR == TR_W_BOX + 4 && TR_W_VEL == TR_W_COR + 8, "box and corners are the row's columns 0..11, contiguous");
static_assert(TR_W_TOTAL + TR_HEADS == TR_W_VOTES && TR_SLOT_WORDS % 4 == 0 && TR_HDR_WORDS % 4 == 0, "16-byte aligned slots, votes behind the totals");
inline long long track_state_stride(int max_tracks) { return (long long)TR_HDR_WORDS + (long long)max_tracks * TR_SLOT_WORDS; }   // words per stream

// ---- an ended record: a line of ended_i / ended_f of lp_track_update, and of q_i / q_f of lp_watch_live -----------------------------
constexpr int RM_REC_WORDS = 12;                // words of a line, int32 and float alike
constexpr int RM_W_TRACK = 0, RM_W_HITS = 3;    // ended_i: the track's id (then first, last), its hits,
constexpr int RM_W_IDS = 4;                     //   and the voted ids of the eight heads at words 4..11
constexpr int RM_F_SHARES = 0, RM_F_BOX = 8;    // ended_f: their shares of the votes at floats 0..7, the last box at 8..11

// ---- thresholds: a double compared with fp32 values on the device ---------------------------------------------------------------
// largest fp32 not above t:  x > f32_not_above(t)  <=>  (double)x > t  for every fp32 x
inline float f32_not_above(double t) {
    float f = (float)t;
    if ((double)f > t) f = nextafterf(f, -INFINITY);
    return f;
}
// smallest fp32 not below t:  x >= f32_not_below(t)  <=>  (double)x >= t
inline float f32_not_below(double t) {
    float f = (float)t;
    if ((double)f < t) f = nextafterf(f, INFINITY);
    return f;
}

// ---- argument rules -------------------------------------------------------------------------------------------------------------
inline std::string stream_dims_fault(int n_streams, int max_tracks) {
    if (n_streams >= 1 && max_tracks >= 1 && max_tracks <= LP_TRACK_MAX_TRACKS) return "";
    return "need n_streams >= 1 and max_tracks in 1.." + std::to_string(LP_TRACK_MAX_TRACKS);
}

// The stages on live tracks index the state and their own buffers with an int32: n_streams x `words[k]` words each stay below 2^31.
// `limits` names them in the message ("... and <limits>").
inline std::string stream_words_fault(int n_streams, int max_tracks, std::initializer_list<long long> words, const std::string& limits) {
    bool ok = stream_dims_fault(n_streams, max_tracks).empty();
    for (long long w : words) ok = ok && (long long)n_streams * w < 0x80000000ll;
    if (ok) return "";
    return "need n_streams >= 1, max_tracks in 1.." + std::to_string(LP_TRACK_MAX_TRACKS) + " and " + limits;
}

struct TrackNcls { int v[TR_HEADS]; };               // the eight head widths as a kernel argument
inline std::string ncls_fault(const int* ncls, TrackNcls& out) {
    if (!ncls) return "null pointer (ncls)";
    for (int h = 0; h < TR_HEADS; ++h) {
        if (ncls[h] < 1 || ncls[h] > LP_TRACK_MAX_CLS)
            return "ncls of head " + std::to_string(h) + " must be in 1.." + std::to_string(LP_TRACK_MAX_CLS);
        out.v[h] = ncls[h];
    }
    return "";
}

inline std::string min_hits_fault(int min_hits) { return min_hits >= 1 ? "" : "min_hits must be >= 1"; }

// an event list of n_streams x max_events lines of `cols` words that an int32 index can address
inline std::string max_events_fault(int n_streams, int max_events, int cols) {
    if (max_events >= 0 && (long long)n_streams * max_events * cols < 0x80000000ll) return "";
    return "need max_events >= 0 and n_streams * max_events * " + std::to_string(cols) + " < 2^31";
}

inline std::string stream_of_fault(const int* stream_of, int B, int n_streams) {
    for (int b = 0; b < B; ++b)
        if (stream_of[b] < -1 || stream_of[b] >= n_streams)
            return "stream " + std::to_string(stream_of[b]) + " of frame " + std::to_string(b) + " (need -1 or 0.." +
                   std::to_string(n_streams - 1) + ")";
    return "";
}

inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return na > 0 && nb > 0 && x < y + nb && y < x + na;
}

struct Region { const void* p; size_t bytes; bool out; };
// an output overlaps another region (inputs may overlap each other)
inline bool regions_clash(const Region* reg, int n) {
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if ((reg[i].out || reg[j].out) && overlap(reg[i].p, reg[i].bytes, reg[j].p, reg[j].bytes)) return true;
    return false;
}

// ---- the frame table of one launch ----------------------------------------------------------------------------------------------
enum Untracked { UNTRACKED_DEAL, UNTRACKED_LEAVE_OUT };   // what becomes of the frames with stream_of == -1

struct StreamPlan {                                  // the caller copies it into its kernel-argument table
    int nblk;                                        // workgroups of the launch (0: nothing to launch)
    int blk_stream[LP_FRAMES_PER_LAUNCH];            // stream of workgroup k (-1: it only takes untracked frames)
    short fr_blk[LP_FRAMES_PER_LAUNCH];              // workgroup that takes frame j, -1: none
    unsigned char fr_skip[LP_FRAMES_PER_LAUNCH];     // frame j is not tracked
};

// The nf <= LP_FRAMES_PER_LAUNCH frames stream_of[0..nf) of one launch: every distinct stream gets a workgroup, in order of first
// appearance, and every frame goes to its stream's.  UNTRACKED_DEAL spreads the untracked frames over the workgroups (frame j to
// j % nblk; a launch without a tracked frame has the one workgroup of stream -1), UNTRACKED_LEAVE_OUT gives them to none (such a
// launch has nblk == 0).  blk_of: the caller's scratch of n_streams entries, all -1 on entry and again on return.
inline StreamPlan plan_streams(const int* stream_of, int nf, std::vector<int>& blk_of, Untracked untracked) {
    StreamPlan pl = {};
    for (int j = 0; j < nf; ++j) {
        const int s = stream_of[j];
        if (s < 0) continue;
        if (blk_of[(size_t)s] < 0) {
            blk_of[(size_t)s] = pl.nblk;
            pl.blk_stream[pl.nblk++] = s;
        }
        pl.fr_blk[j] = (short)blk_of[(size_t)s];
    }
    for (int k = 0; k < pl.nblk; ++k) blk_of[(size_t)pl.blk_stream[k]] = -1;
    if (untracked == UNTRACKED_DEAL && pl.nblk == 0) { pl.blk_stream[0] = -1; pl.nblk = 1; }
    for (int j = 0; j < nf; ++j)
        if (stream_of[j] < 0) {
            pl.fr_skip[j] = 1;
            pl.fr_blk[j] = untracked == UNTRACKED_DEAL ? (short)(j % pl.nblk) : (short)-1;
        }
    return pl;
}

}  // namespace lp
