// Matching the reads of ended plate tracks against a device-resident watchlist: lp_watch_match and lp_watch_match_indel
// (include/lp_hip.h).  A weighted Hamming distance over the eight heads -- with indel = 1 under the twelve alignments that lose or
// gain one character --, N entries x Q reads, behind lp_track_update's ended records.  The reference has nothing here; the
// written-down specification is yolov6/utils/watch.py (watch_match_np), which these kernels match on every int32
// (tests/test_watch_gpu.py, tests/test_watch_indel_gpu.py).  Everything is integer except one fp32 product per read and position;
// the reductions are an unsigned minimum and an integer sum, so the result does not depend on the order in which workgroups arrive.
// The record layout, the weight of a position, the confusion addressing, the table builder and the prefix sum are
// lp_read_match.inc's, the first three and the last shared with lp_sight.hip; what is here is the frame of the scan, once, and the
// two scoring rules as policies of it (Positional, Indel).  Both entry points are watch_run.
//
// watch_prep_kernel (one workgroup): the clamped counts of the streams are prefix-summed in LDS, read k of the call (stream s,
//   line j) gets the position off[s] + j and its line goes to qlist[k]; keys and counts of every position are cleared.
// watch_scan_kernel<P>: one workgroup of 256 threads per LP_WATCH_BLOCK_ENTRIES entries.  Every lane owns eight entries, each one
//   8-byte load (lane t takes entries base + r * 256 + t: coalesced), their ids mapped to table columns once -- 0..63 the id, 64
//   WILD, 65 "matches nothing" -- and parked in LDS (16 KiB; held in registers across the unrolled loops they cost the kernel
//   a thousand spilled registers).  So the list is read from memory once per call, however many reads there are.  The workgroup
//   walks the valid reads in blocks of 16 (P::QB).  Per block it stages the reads and builds the LDS table
//     T[position][column][read] = 0 for a match, else (weight * cost << P::COST_SHIFT) | P::MISMATCH
//   (80-byte column pitch: 16 reads + one 16-byte slot, so that the 16-byte reads of lanes on different columns spread over all bank
//   slots); score_block(P, ...) then gives every lane, per read, the word of its best accepted entry and the number it accepted;
//   lanes that accepted something combine into LDS (64-bit minimum of the policy's key, integer add), and one thread per read with a hit
//   issues one global atomicMin and one atomicAdd.  Workgroups with nothing accepted issue no atomic.  Blocks of up to four, eight
//   and twelve reads run the same code on that many table columns only (template parameter Q4, chosen in the kernel).
//   Positional: an (entry, read) pair is eight LDS lookups and adds with no branch: one ds_read_b128 fetches a column's values
//   for four reads.  The sums sit in one register: mismatches in bits 0..3, cost in bits 8..24; both limits are tested by one
//   subtraction from (limit | guard bit) per field.  A lane keeps the minimum of (sum | r << 4) over its accepted entries --
//   (cost, index) order, since its entries ascend with r; the key is cost << 32 | index << 4 | mismatches.
//   Indel: at its policy and its score_block below.  lp_watch_match_indel with indel = 0 launches the Positional instance.
// watch_tail_kernel: one thread per line of match_i turns key and count (of either key layout) into (entry, mismatches, cost,
//   n_hits) and, for lp_watch_match_indel, the alignment code into match_align; every other line gets (-1, 0, 0, 0) and code 0.
#include "lp_internal.h"
#include "lp_streams.h"
#include "lp_read_match.inc"

namespace lp {

namespace {

constexpr int W_T = 256;                                   // threads of a scan workgroup
constexpr int W_R = LP_WATCH_BLOCK_ENTRIES / W_T;          // entries per lane
constexpr int W_PREP_T = 1024;
static_assert(W_R == 8, "lp_watch.hip is written for 8 entries per lane");
static_assert(LP_TRACK_MAX_CLS == 64, "the table has 64 id columns");

struct WatchWs {                                           // carve-up of the caller's workspace, L = n_streams * max_ended
    unsigned long long* keys;                              // [L] by read position
    int32_t* cnts;                                         // [L]
    int32_t* qlist;                                        // [L] line of read k
    int32_t* off;                                          // [n_streams] position of the stream's first read
    int32_t* nvalid;                                       // [1]
    size_t bytes;
};
WatchWs watch_carve(void* base, size_t S, size_t max_ended) {
    const size_t L = S * max_ended;
    char* p = (char*)base;
    WatchWs w;
    w.keys = (unsigned long long*)p;
    w.cnts = (int32_t*)(p + 8 * L);
    w.qlist = (int32_t*)(p + 12 * L);
    w.off = (int32_t*)(p + 16 * L);
    w.nvalid = (int32_t*)(p + 16 * L + 4 * S);
    w.bytes = (16 * L + 4 * S + 4 + 15) & ~(size_t)15;
    return w;
}

// grid (1), block (1024)
__global__ __launch_bounds__(W_PREP_T) void watch_prep_kernel(const int32_t* __restrict__ ended_count, int S, int max_ended, WatchWs ws) {
    __shared__ int s_scan[W_PREP_T];
    const int tid = threadIdx.x;
    int base = 0;
    for (int s0 = 0; s0 < S; s0 += W_PREP_T) {                         // (block-uniform control flow)
        const int s = s0 + tid;
        const int c = s < S ? clamp_count(ended_count[s], max_ended) : 0;
        s_scan[tid] = c;
        block_prefix_sum<W_PREP_T>(s_scan);
        if (s < S) ws.off[s] = base + s_scan[tid] - c;
        base += s_scan[W_PREP_T - 1];
        __syncthreads();
    }
    if (tid == 0) ws.nvalid[0] = base;
    const int L = S * max_ended;
    for (int l = tid; l < L; l += W_PREP_T) {
        const int s = l / max_ended, j = l - s * max_ended;
        ws.keys[l] = ~0ull;
        ws.cnts[l] = 0;
        if (j < clamp_count(ended_count[s], max_ended)) ws.qlist[ws.off[s] + j] = l;     // off[s] + j < L; off[] is behind a barrier
    }
}

// ids of four entry bytes -> table columns
__device__ __forceinline__ unsigned to_columns(unsigned x) {
    unsigned out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned b = (x >> (8 * k)) & 0xffu;
        out |= (b < 64u ? b : (b == 255u ? (unsigned)RM_COL_WILD : (unsigned)RM_COL_NONE)) << (8 * k);
    }
    return out;
}

// ---- the two scans ----------------------------------------------------------------------------------------------------------------
// A scan policy holds what differs between them: the layout of a table word and of the register that sums eight of them, the limits
// in that layout (one subtraction from (limit | guard bit) per field tests both) and the start value of a lane's entries past N.
// score_block(policy, ...) below is its scoring loop, down to the 64-bit keys in LDS.
struct Positional {                                        // lp_watch_match: the weighted Hamming distance, head against head
    static constexpr int QB = LP_WATCH_QUERY_BLOCK;
    static constexpr int PITCH = QB + 4;                   // dwords between two columns of the table
    static constexpr unsigned COST_SHIFT = 8, MISMATCH = 1u;           // a word is (cost << 8) | mismatches
    static constexpr unsigned GUARD = (1u << 4) | (1u << 25);          // the bits a field keeps iff it is within its limit
    static constexpr unsigned OUTSIDE = 0x10000u << COST_SHIFT;        // a cost above every limit
    typedef unsigned Limits;                               // the two limits and the guard bits, in the layout of a word
    static Limits limits(int max_mismatch, int max_cost) { return ((unsigned)max_mismatch | ((unsigned)max_cost << COST_SHIFT)) | GUARD; }
};
// lp_watch_match_indel with indel = 1: one lost or gained character.  A table word is (cost << 12) | (mismatch << 4): bits 0..3 stay
// free for the alignment code and bits 9..11 for the lane's entry number, so that an unsigned comparison of two alignment words is the
// (cost, mismatches, code) order of the rule.
struct Indel {
    static constexpr int QB = LP_WATCH_INDEL_QUERY_BLOCK;
    static constexpr int PITCH = QB + 4;                   // dwords between two columns: an odd number of 16-byte slots
    static constexpr unsigned COST_SHIFT = 12, MISM_SHIFT = 4, MISMATCH = 1u << MISM_SHIFT;
    static constexpr unsigned GUARD = (1u << 8) | (1u << 30);
    static constexpr unsigned OUTSIDE = 0x10000u << COST_SHIFT;
    struct Limits { unsigned word, gapw; };                // gapw: what a shifted alignment pays, as a table word
    static Limits limits(int max_mismatch, int max_cost, int gap_cost) {
        return {15u | ((unsigned)max_mismatch << MISM_SHIFT) | ((unsigned)max_cost << COST_SHIFT) | GUARD,
                ((unsigned)gap_cost << COST_SHIFT) | MISMATCH};
    }
};

template <class P>
struct ScanLds {
    static_assert(P::QB == 16 && ((P::PITCH / 4) & 1) == 1, "blocks of 16 reads; columns start on odd multiples of a 16-byte slot");
    unsigned T[8 * RM_COLS * P::PITCH];                    // 8 positions x 66 columns x 20 dwords = 42240 bytes
    uint2 ent[LP_WATCH_BLOCK_ENTRIES];                     // the workgroup's entries as table columns, entry r of lane t at r * 256 + t
    int best[P::QB * 8];
    unsigned qp[P::QB * 8];
    unsigned long long key[P::QB];
    int cnt[P::QB];
};

// score_block: the lane's W_R entries (r < nlane of them below N) against the 4 * Q4 reads of the table.  Per read, best = the word
// of the first of its cheapest accepted entries with the entry's number r in it, and cnt = how many it accepted; lanes that accepted
// something then combine into the block's keys and counts in LDS.  The combine and the packing of the key are written out in both
// functions: handed to a shared helper as arrays, best and cnt made the compiler schedule the positional loop in another order,
// and lp_watch_match measured 1 to 2 % slower.
template <int Q4>
__device__ __forceinline__ void score_block(Positional, ScanLds<Positional>& lds, int nlane, int idx0, unsigned limits) {
    constexpr int NQ = 4 * Q4;
    const int tid = threadIdx.x;
    unsigned best[NQ], cnt[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) { best[q] = ~0u; cnt[q] = 0u; }
#pragma unroll 1
    for (int r = 0; r < W_R; ++r) {
        unsigned acc[NQ];
        const uint2 ent = lds.ent[r * W_T + tid];
        const unsigned start = r < nlane ? 0u : Positional::OUTSIDE;
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[q] = start;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const unsigned col = ((p < 4 ? ent.x : ent.y) >> (8 * (p & 3))) & 0xffu;
            const uint4* row = (const uint4*)(lds.T + (p * RM_COLS) * Positional::PITCH) + col * (Positional::PITCH / 4);
#pragma unroll
            for (int g = 0; g < Q4; ++g) {
                const uint4 v = row[g];
                acc[4 * g] += v.x; acc[4 * g + 1] += v.y; acc[4 * g + 2] += v.z; acc[4 * g + 3] += v.w;
            }
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const bool ok = ((limits - acc[q]) & Positional::GUARD) == Positional::GUARD;
            const unsigned key = acc[q] | ((unsigned)r << 4);
            best[q] = ok && key < best[q] ? key : best[q];
            cnt[q] += ok ? 1u : 0u;
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {                                     // cost << 32 | index << 4 | mismatches
        if (cnt[q] != 0u) {
            const unsigned r = (best[q] >> 4) & 7u;
            const unsigned long long key = ((unsigned long long)(best[q] >> Positional::COST_SHIFT) << 32) |
                                           ((unsigned long long)(unsigned)(idx0 + (int)r * W_T) << 4) | (best[q] & 15u);
            atomicMin(&lds.key[q], key);
            atomicAdd(&lds.cnt[q], (int)cnt[q]);
        }
    }
}

// Heads 2..7 share a confusion group, so L[p] and R[p] are row p of the table at the column of the entry's head p + 1 / p - 1: three
// 16-byte reads per position where the positional scan has one.  Four reads (one uint4) are scored at a time, so the live
// accumulators are 3 x 4 whatever the query block; what grows with the block are the two registers per read that carry a lane's
// best entry and count across its entries.
template <int Q4>
__device__ __forceinline__ void score_block(Indel, ScanLds<Indel>& lds, int nlane, int idx0, Indel::Limits lim) {
    constexpr int NQ = 4 * Q4;
    const int tid = threadIdx.x;
    const unsigned limits = lim.word, gapw = lim.gapw;
    unsigned best[NQ], cnt[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) { best[q] = ~0u; cnt[q] = 0u; }
#pragma unroll 1
    for (int r = 0; r < W_R; ++r) {
        const uint2 ent = lds.ent[r * W_T + tid];
        const unsigned start = r < nlane ? 0u : Indel::OUTSIDE;
        const uint4* row[8];                                           // row[c]: the entry's head c as a column of position 0's table
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const unsigned col = ((c < 4 ? ent.x : ent.y) >> (8 * (c & 3))) & 0xffu;
            row[c] = (const uint4*)lds.T + col * (Indel::PITCH / 4);
        }
        constexpr int POS4 = RM_COLS * Indel::PITCH / 4;                     // uint4s between the tables of two positions
#pragma unroll
        for (int g = 0; g < Q4; ++g) {
            unsigned pre[4], del[4], ins[4];                           // prefix of U; the best opened deletion / insertion so far
            {
                const uint4 a = row[0][g], b = row[1][POS4 + g];
                pre[0] = start + a.x + b.x; pre[1] = start + a.y + b.y; pre[2] = start + a.z + b.z; pre[3] = start + a.w + b.w;
            }
#pragma unroll
            for (int p = 2; p < 8; ++p) {
                const uint4 u4 = row[p][p * POS4 + g];
                const unsigned u[4] = {u4.x, u4.y, u4.z, u4.w};
                if (p <= 6) {                                          // open at k = p: codes p - 1 (lost) and p + 4 (gained)
                    const uint4 l4 = row[p + 1][p * POS4 + g];
                    const unsigned l[4] = {l4.x, l4.y, l4.z, l4.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const unsigned od = pre[i] | (unsigned)(p - 1);
                        del[i] = (p == 2 ? od : (od < del[i] ? od : del[i])) + l[i];
                    }
                }
                if (p >= 3) {
                    const uint4 r4 = row[p - 1][p * POS4 + g];
                    const unsigned rr[4] = {r4.x, r4.y, r4.z, r4.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) ins[i] += rr[i];
                }
                if (p <= 6) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const unsigned oi = pre[i] | (unsigned)(p + 4);
                        ins[i] = p == 2 ? oi : (oi < ins[i] ? oi : ins[i]);
                    }
                }
                if (p == 7) {                                          // code 11, and the shifted alignments pay the gap
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const unsigned e = pre[i] | 11u;
                        unsigned m = del[i] < ins[i] ? del[i] : ins[i];
                        m = e < m ? e : m;
                        del[i] = m + gapw;
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) pre[i] += u[i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int q = 4 * g + i;
                const unsigned w = pre[i] < del[i] ? pre[i] : del[i];                  // code 0 wins a tie: its low bits are 0
                const bool ok = ((limits - w) & Indel::GUARD) == Indel::GUARD;
                const unsigned key = w | ((unsigned)r << 9);
                best[q] = ok && (key >> Indel::COST_SHIFT) < (best[q] >> Indel::COST_SHIFT) ? key : best[q];      // the first of the smallest cost
                cnt[q] += ok ? 1u : 0u;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {                                     // cost << 32 | index << 8 | code << 4 | mismatches
        if (cnt[q] != 0u) {
            const unsigned r = (best[q] >> 9) & 7u;
            const unsigned long long key = ((unsigned long long)(best[q] >> Indel::COST_SHIFT) << 32) |
                                           ((unsigned long long)(unsigned)(idx0 + (int)r * W_T) << 8) | ((best[q] & 15u) << 4) |
                                           ((best[q] >> Indel::MISM_SHIFT) & 15u);
            atomicMin(&lds.key[q], key);
            atomicAdd(&lds.cnt[q], (int)cnt[q]);
        }
    }
}

// One block of 4 * Q4 reads (the reads k0 .. k0 + nq - 1, nq <= 4 * Q4), from the staged best / qp to the global atomics.
template <class P, int Q4>
__device__ __forceinline__ void scan_block(ScanLds<P>& lds, int nlane, int idx0, const unsigned char* __restrict__ confuse,
                                           typename P::Limits lim, int k0, int nq, const WatchWs& ws) {
    constexpr int NQ = 4 * Q4;
    const int tid = threadIdx.x;
    build_read_table<NQ, P::PITCH, P::COST_SHIFT, P::MISMATCH, W_T>(lds.T, lds.best, lds.qp, confuse);
    __syncthreads();
    score_block<Q4>(P(), lds, nlane, idx0, lim);
    __syncthreads();
    if (tid < nq && lds.cnt[tid] > 0) {                                // one thread per read with a hit
        atomicMin(&ws.keys[k0 + tid], lds.key[tid]);
        atomicAdd(&ws.cnts[k0 + tid], lds.cnt[tid]);
    }
}

// grid (ceil(N / LP_WATCH_BLOCK_ENTRIES)), block (256)
template <class P>
__global__ __launch_bounds__(W_T) void watch_scan_kernel(const uint2* __restrict__ entries, int N, const unsigned char* __restrict__ confuse,
                                                         const int32_t* __restrict__ ended_i, const float* __restrict__ ended_f,
                                                         typename P::Limits lim, WatchWs ws) {
    __shared__ __attribute__((aligned(16))) ScanLds<P> lds;
    const int tid = threadIdx.x;
    const int nv = ws.nvalid[0];
    if (nv <= 0) return;                                               // (block-uniform)
    const int idx0 = blockIdx.x * LP_WATCH_BLOCK_ENTRIES + tid;         // < 2^24 + 2048
    int nlane = 0;                                                     // this lane's entries below N: r < nlane
#pragma unroll
    for (int r = 0; r < W_R; ++r) {
        const int idx = idx0 + r * W_T;
        uint2 v = make_uint2(0u, 0u);
        if (idx < N) { v = entries[idx]; nlane = r + 1; }
        lds.ent[r * W_T + tid] = make_uint2(to_columns(v.x), to_columns(v.y));     // read back by this lane alone
    }
    for (int k0 = 0; k0 < nv; k0 += P::QB) {                           // nv <= n_streams * max_ended: k0 + q indexes qlist, keys, cnts
        const int nq = nv - k0 < P::QB ? nv - k0 : P::QB;
        if (tid < P::QB * 8) {                                         // best / qp: [read][position]
            const int q = tid >> 3, p = tid & 7;
            int b = -1;
            unsigned qp = 1u;
            if (q < nq) {
                const long long rec = (long long)ws.qlist[k0 + q] * RM_REC_WORDS;
                b = ended_i[rec + RM_W_IDS + p];
                const float share = ended_f[rec + RM_F_SHARES + p];
                if (share > 0.f) qp = read_weight(share);
            }
            lds.best[tid] = b;
            lds.qp[tid] = qp;
        }
        if (tid < P::QB) { lds.key[tid] = ~0ull; lds.cnt[tid] = 0; }
        __syncthreads();
        // blocks of up to four, eight and twelve reads run the same code on that many table columns only.  (The choice stands here
        // and not in a helper of its own: behind one the compiler folds the four instances' flushes into one copy reached over a
        // scalar flag, the only difference from the kernel this one replaced, and lp_watch_match measured 0.3 % slower.)
        if (nq <= 4) scan_block<P, 1>(lds, nlane, idx0, confuse, lim, k0, nq, ws);
        else if (nq <= 8) scan_block<P, 2>(lds, nlane, idx0, confuse, lim, k0, nq, ws);
        else if (nq <= 12) scan_block<P, 3>(lds, nlane, idx0, confuse, lim, k0, nq, ws);
        else scan_block<P, 4>(lds, nlane, idx0, confuse, lim, k0, nq, ws);
        __syncthreads();                                               // the next block stages over best / qp / key / cnt and the table
    }
}

// grid (ceil(L / 256)), block (256).  scanned == 0 (an empty list): every line is (-1, 0, 0, 0) and the workspace is not read.
// coded == 0: the keys are Positional's and every code is 0; coded == 1: Indel's.  match_align may be null (lp_watch_match).
__global__ __launch_bounds__(256) void watch_tail_kernel(const int32_t* __restrict__ ended_count, int S, int max_ended, int scanned, int coded,
                                                         WatchWs ws, int32_t* __restrict__ match_i, int32_t* __restrict__ match_align) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= S * max_ended) return;
    const int s = l / max_ended, j = l - s * max_ended;
    int e = -1, mism = 0, cost = 0, n = 0, code = 0;
    if (scanned && j < clamp_count(ended_count[s], max_ended)) {
        const int k = ws.off[s] + j;
        n = ws.cnts[k];
        if (n > 0) {
            const unsigned long long key = ws.keys[k];
            e = coded ? (int)((key >> 8) & 0xffffffull) : (int)((key >> 4) & 0xfffffffull);
            code = coded ? (int)((key >> 4) & 15ull) : 0;
            mism = (int)(key & 15ull);
            cost = (int)(key >> 32);
        }
    }
    int32_t* out = match_i + (long long)l * 4;
    out[0] = e; out[1] = mism; out[2] = cost; out[3] = n;
    if (match_align != nullptr) match_align[l] = code;
}

// Both entry points.  with_indel: lp_watch_match_indel (indel, gap_cost and match_align are its own).
int watch_run(const std::string& fn, bool with_indel, const unsigned char* entries, int n_entries, const unsigned char* confuse,
              const int32_t* ended_i, const float* ended_f, const int32_t* ended_count, int n_streams, int max_ended, int max_mismatch,
              int max_cost, int indel, int gap_cost, int32_t* match_i, int32_t* match_align, void* workspace, size_t workspace_bytes,
              void* stream) {
    if (n_entries < 0 || n_entries > LP_WATCH_MAX_ENTRIES)
        return fail(LP_ERR_ARG, fn + "n_entries " + std::to_string(n_entries) + " (need 0.." + std::to_string(LP_WATCH_MAX_ENTRIES) + ")");
    if (const std::string f = ended_dims_fault(n_streams, max_ended); !f.empty()) return fail(LP_ERR_ARG, fn + f);
    if (const std::string f = match_limits_fault(max_mismatch, max_cost); !f.empty()) return fail(LP_ERR_ARG, fn + f);
    if (with_indel && (indel < 0 || indel > 1 || gap_cost < 0 || gap_cost > LP_WATCH_MAX_GAP_COST))
        return fail(LP_ERR_ARG, fn + "need indel in 0..1 and gap_cost in 0.." + std::to_string(LP_WATCH_MAX_GAP_COST));
    if (max_ended == 0) return LP_OK;                                  // no line to write
    const bool scan = n_entries > 0;
    if (!ended_count || !match_i || (with_indel && !match_align) || (scan && (!entries || !ended_i || !ended_f || !workspace)))
        return fail(LP_ERR_ARG, fn + "null pointer");
    const WatchWs ws = watch_carve(workspace, (size_t)n_streams, (size_t)max_ended);
    if (scan) {
        if (((uintptr_t)entries & 7) != 0 || ((uintptr_t)confuse & 3) != 0 || ((uintptr_t)workspace & 15) != 0)
            return fail(LP_ERR_ARG, fn + "entries must be 8-byte, confuse 4-byte and the workspace 16-byte aligned");
        if (workspace_bytes < ws.bytes)
            return fail(LP_ERR_ARG, fn + "workspace of " + std::to_string(workspace_bytes) + " bytes, need " + std::to_string(ws.bytes));
    }
    {   // neither output nor the workspace may overlap an input or each other
        const size_t L = (size_t)n_streams * max_ended;
        const Region reg[] = {{entries, (size_t)n_entries * 8, false},
                              {confuse, scan && confuse ? (size_t)3 * 64 * 64 : 0, false},
                              {ended_i, scan ? L * RM_REC_WORDS * 4 : 0, false},
                              {ended_f, scan ? L * RM_REC_WORDS * 4 : 0, false},
                              {ended_count, (size_t)n_streams * 4, false},
                              {match_i, L * 16, true},
                              {match_align, with_indel ? L * 4 : 0, true},
                              {workspace, scan ? ws.bytes : 0, true}};
        if (regions_clash(reg, (int)(sizeof(reg) / sizeof(reg[0]))))
            return fail(LP_ERR_ARG, fn + (with_indel ? "match_i, match_align and the workspace may overlap neither an input nor each other"
                                                     : "match_i and the workspace may overlap neither an input nor each other"));
    }

    hipStream_t st = (hipStream_t)stream;
    const int L = n_streams * max_ended;
    if (scan) {
        hipLaunchKernelGGL(watch_prep_kernel, dim3(1), dim3(W_PREP_T), 0, st, ended_count, n_streams, max_ended, ws);
        LP_HIP_CHECK(hipGetLastError());
        const dim3 grid((unsigned)ceil_div(n_entries, LP_WATCH_BLOCK_ENTRIES));
        if (indel)
            hipLaunchKernelGGL(watch_scan_kernel<Indel>, grid, dim3(W_T), 0, st, (const uint2*)entries, n_entries, confuse, ended_i, ended_f,
                               Indel::limits(max_mismatch, max_cost, gap_cost), ws);
        else                                                           // only code 0 exists: the positional scan
            hipLaunchKernelGGL(watch_scan_kernel<Positional>, grid, dim3(W_T), 0, st, (const uint2*)entries, n_entries, confuse, ended_i, ended_f,
                               Positional::limits(max_mismatch, max_cost), ws);
        LP_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(watch_tail_kernel, dim3((unsigned)ceil_div(L, 256)), dim3(256), 0, st, ended_count, n_streams, max_ended, scan ? 1 : 0,
                       indel, ws, match_i, match_align);
    LP_HIP_CHECK(hipGetLastError());
    return LP_OK;
}

}  // namespace

}  // namespace lp

using namespace lp;

extern "C" size_t lp_watch_workspace_bytes(int n_streams, int max_ended) {
    if (!ended_dims_fault(n_streams, max_ended).empty()) return 0;
    return watch_carve(nullptr, (size_t)n_streams, (size_t)max_ended).bytes;
}

extern "C" int lp_watch_match(const unsigned char* entries, int n_entries, const unsigned char* confuse, const int32_t* ended_i,
                              const float* ended_f, const int32_t* ended_count, int n_streams, int max_ended, int max_mismatch, int max_cost,
                              int32_t* match_i, void* workspace, size_t workspace_bytes, void* stream) {
    return watch_run("lp_watch_match: ", false, entries, n_entries, confuse, ended_i, ended_f, ended_count, n_streams, max_ended, max_mismatch,
                     max_cost, 0, 0, match_i, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int lp_watch_match_indel(const unsigned char* entries, int n_entries, const unsigned char* confuse, const int32_t* ended_i,
                                    const float* ended_f, const int32_t* ended_count, int n_streams, int max_ended, int max_mismatch,
                                    int max_cost, int indel, int gap_cost, int32_t* match_i, int32_t* match_align, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    return watch_run("lp_watch_match_indel: ", true, entries, n_entries, confuse, ended_i, ended_f, ended_count, n_streams, max_ended,
                     max_mismatch, max_cost, indel, gap_cost, match_i, match_align, workspace, workspace_bytes, stream);
}
