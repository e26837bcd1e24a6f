// What the scans that match voted plate reads against packed 8-byte entries have in common (lp_watch.hip: lp_watch_match and
// lp_watch_match_indel; lp_sight.hip: lp_sight_update; lp_watch_live.hip writes the records they read): the limits of an ended-record list
// (its layout is lp_streams.h's), the weight of a position, where the confusion table keeps a pair's cost, the table of the two watchlist scans and the prefix sum.
// Each rule is stated here once; its written-down form is yolov6/utils/watch.py (position_weight, confuse_table, watch_match_np),
// which the kernels match on every int32.
#pragma once

namespace lp {

namespace {

// ---- an ended record (RM_REC_WORDS, RM_W_*, RM_F_*): lp_streams.h, beside the tracker's state, whose kernel writes it -------------
// n_streams x max_ended lines that an int32 index can address; else the message that the entry points return
inline std::string ended_dims_fault(int n_streams, int max_ended) {
    if (n_streams >= 1 && max_ended >= 0 && (long long)n_streams * max_ended * RM_REC_WORDS < 0x80000000ll) return std::string();
    return "need n_streams >= 1, max_ended >= 0 and n_streams * max_ended * " + std::to_string(RM_REC_WORDS) + " < 2^31";
}
// the two limits of a match, common to every entry point
inline std::string match_limits_fault(int max_mismatch, int max_cost) {
    if (max_mismatch >= 0 && max_mismatch <= 8 && max_cost >= 0 && max_cost <= LP_WATCH_MAX_COST) return std::string();
    return "need max_mismatch in 0..8 and max_cost in 0.." + std::to_string(LP_WATCH_MAX_COST);
}

// the lines of a stream that hold a record: its ended count, held to 0..max_ended
__device__ __forceinline__ int clamp_count(int c, int max_ended) { return c < 0 ? 0 : (c > max_ended ? max_ended : c); }

// weight 1..256 of a position from the share of the votes its id holds (position_weight): 1 for a share of 0, below it, or NaN.
// The staging loops of the scans start from 1 and call this under their own `share > 0`: written as one expression the compiler
// makes a select of it, and sight_scan_kernel's table build then waits on a register it had to spill (DESIGN 3.16c).
__device__ __forceinline__ unsigned read_weight(float share) {
    unsigned w = 1u;
    if (share > 0.f) w = (unsigned)(int)fminf(share * 255.0f, 255.0f) + 1u;
    return w;
}

// where the confusion table [3][64][64] keeps the costs of read id b (0..63) at position p against the entry ids 4 * c4 .. 4 * c4 + 3:
// four bytes, one aligned word; the groups are head 0, head 1, and heads 2..7 together
__device__ __forceinline__ int confuse_offset(int p, int b, int c4) { return (p < 2 ? p : 2) * 4096 + b * 64 + c4 * 4; }

// ---- the table of the watchlist scans -------------------------------------------------------------------------------------------
constexpr int RM_COLS = 66;                     // columns of a position: 0..63 the ids, then
constexpr int RM_COL_WILD = 64, RM_COL_NONE = 65;   //   an entry byte that matches every id, and one that matches none

// T[position][column][read] for the NQ staged reads (id best[q * 8 + p], weight qp[q * 8 + p]), PITCH dwords from column to column:
// 0 where the column matches the read's id, else (weight * cost << COST_SHIFT) | MISMATCH.  One unit of work = (position, four id
// columns or the two special ones, read).  The caller puts a barrier behind it.
template <int NQ, int PITCH, unsigned COST_SHIFT, unsigned MISMATCH, int THREADS>
__device__ __forceinline__ void build_read_table(unsigned* __restrict__ T, const int* __restrict__ best, const unsigned* __restrict__ qp,
                                                 const unsigned char* __restrict__ confuse) {
    for (int u = threadIdx.x; u < 8 * 17 * NQ; u += THREADS) {
        const int q = u % NQ, pc = u / NQ, p = pc / 17, c4 = pc - p * 17;
        const int b = best[q * 8 + p];
        const unsigned w = qp[q * 8 + p];
        unsigned* col0 = T + (p * RM_COLS + c4 * 4) * PITCH + q;
        if (c4 == 16) {
            static_assert(RM_COL_WILD == 64 && RM_COL_NONE == 65, "the special columns are unit 16 of a position");
            col0[0] = 0u;
            col0[PITCH] = ((w * 16u) << COST_SHIFT) | MISMATCH;
            continue;
        }
        const bool inr = (unsigned)b < 64u;
        unsigned cw = 0x10101010u;                                     // 16 sixteenths each without a table or for an id outside 0..63
        if (confuse != nullptr && inr) cw = *(const unsigned*)(confuse + confuse_offset(p, b, c4));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            unsigned c = (cw >> (8 * k)) & 0xffu;
            c = c > 16u ? 16u : c;                                     // a table the host did not check cannot leave the cost field
            unsigned v = ((w * c) << COST_SHIFT) | MISMATCH;
            if (inr && c4 * 4 + k == b) v = 0u;                        // the read's own id: no mismatch, no cost
            col0[k * PITCH] = v;
        }
    }
}

// Inclusive prefix sum over s[0..THREADS) in place, s[threadIdx.x] written by its thread just before; THREADS == blockDim.x
template <int THREADS>
__device__ __forceinline__ void block_prefix_sum(int* s) {
    const int tid = threadIdx.x;
    __syncthreads();
    for (int d = 1; d < THREADS; d <<= 1) {
        const int v = tid >= d ? s[tid - d] : 0;
        __syncthreads();
        s[tid] += v;
        __syncthreads();
    }
}

}  // namespace

}  // namespace lp
