// Host-side pieces shared by the per-stream entry points (lp_track.hip, lp_shots.hip, lp_lookback.hip) and the threshold
// rounding of lp_nms.hip and lp_tiles.hip.  No HIP header: tests/host_streams.cpp includes this file alone and runs on the CPU.
// A new per-stream kernel family takes its frame table from plan_streams and its argument checks from the *_fault functions
// (an empty string: fine; the caller hands the message to fail(), as with plane_fault and region_fault).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/lp_hip.h"

namespace lp {

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
