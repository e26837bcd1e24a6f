// Looking the reads of LIVE plate tracks up in a watchlist, with a memo per track: lp_watch_live (include/lp_hip.h).  The ended-record
// lookup of lp_watch_match fires when a track has been unseen for max_age frames; a car waiting at a barrier, or a stolen one still
// in the picture, needs the answer while its track lives.  The reference has nothing here; the written-down specification is
// yolov6/utils/watch_live.py (LiveWatchNp), which this file matches on every int32 (tests/test_watch_live_gpu.py).
//
// Two kernels, one in front of and one behind the unchanged scan of lp_watch.hip; both take one workgroup per stream and read the
// tracker state as lp_track_update left it (layout: lp_streams.h), never writing it.
// live_gather_kernel, steps 1 to 4 of the rule: thread t < 128 reads slot t's first words (id, first, last, hits; 16 bytes) and its
//   memo line.  A slot that is not live gets a zero memo line.  A candidate (hits >= min_hits) whose memo holds its id and whose
//   `last` equals the memo's last_at_lookup cannot have a new key -- votes change only on a match, and a match sets `last` -- so it
//   is not fresh and its votes are not read; this changes no output byte.  For every other candidate the eight threads
//   (slot, head) each read one head: the argmax over ncls[p] <= 64 floats, lowest index on a tie, and the share (track_read_head of
//   lp_track_read.inc: rule 8, the function the tracker's own vote step calls).  Thread t packs the key and
//   decides `fresh`; the fresh slots are numbered in slot order by ballot and prefix count over the two waves, as track_kernel numbers ending
//   tracks, and their lines go out in the ended-record layout (lp_read_match.inc).  Lines past the count are zeroed (q_slot -1), and pos[s][t] -- the
//   query line of slot t, -1 for none -- is left in the workspace for the scatter.
// lp_watch_match on (q_i, q_f, q_count) with max_ended = max_tracks; its match_i lies in the workspace.
// live_scatter_kernel, steps 6 and 7: thread t memoises the answer of a fresh slot (key repacked from its query line) and writes the
//   slot's row of live_i from the memo.
// lp_watch_live_indel is the same three steps with lp_watch_match_indel in the middle: its match_align lies in the workspace too, and
//   the scatter also writes the slot's word of live_align (step 8: the code of a fresh lookup, the standing one kept, else 0).
#include "lp_internal.h"
#include "lp_streams.h"
#include "lp_track_read.inc"
#include "lp_read_match.inc"

namespace lp {

namespace {

constexpr int WL_T = TR_SLOTS * TR_HEADS;       // most threads of a gather workgroup: one per (slot, head)
constexpr int WL_MEMO_WORDS = 8, WL_LIVE_COLS = 8;

struct LiveWs {                                 // carve-up of the caller's workspace, L = n_streams * max_tracks
    int32_t* pos;                               // [L] query line of a slot, -1: none
    int32_t* match_i;                           // [L, 4] of lp_watch_match
    void* watch;                                // the workspace of lp_watch_match
    size_t watch_bytes, bytes;
    int32_t* match_align;                       // [L] of lp_watch_match_indel: behind `bytes`, lp_watch_live_indel only
    size_t indel_bytes;
};
LiveWs live_carve(void* base, size_t S, size_t T) {
    const size_t L = S * T, pos_bytes = (4 * L + 15) & ~(size_t)15;
    char* p = (char*)base;
    LiveWs w;
    w.pos = (int32_t*)p;
    w.match_i = (int32_t*)(p + pos_bytes);
    w.watch = p + pos_bytes + 16 * L;
    w.watch_bytes = lp_watch_workspace_bytes((int)S, (int)T);
    w.bytes = pos_bytes + 16 * L + w.watch_bytes;                      // (every part is a multiple of 16 bytes)
    w.match_align = (int32_t*)(p + w.bytes);
    w.indel_bytes = w.bytes + pos_bytes;
    return w;
}

// the dimensions of a call, the query lines within an int32 index
std::string live_dims_fault(int n_streams, int max_tracks) {
    return stream_words_fault(n_streams, max_tracks, {(long long)max_tracks * RM_REC_WORDS},
                              "n_streams * max_tracks * " + std::to_string(RM_REC_WORDS) + " < 2^31");
}

// grid (n_streams), block (max(128, max_tracks * 8 rounded up to 64))
__global__ __launch_bounds__(WL_T) void live_gather_kernel(const int* __restrict__ state, int T, long long sstride, const TrackNcls ncls, int min_hits,
                                                          int32_t* __restrict__ memo, int32_t* __restrict__ q_i, float* __restrict__ q_f,
                                                          int32_t* __restrict__ q_slot, int32_t* __restrict__ q_count, int32_t* __restrict__ pos) {
    __shared__ int s_need[TR_SLOTS], s_pos[TR_SLOTS], s_best[TR_SLOTS * TR_HEADS];
    __shared__ float s_share[TR_SLOTS * TR_HEADS];
    __shared__ int s_wcnt[2];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* const sst = state + (long long)s * sstride + TR_HDR_WORDS;
    const long long line0 = (long long)s * T;                          // first slot / query line of the stream; line0 + T <= S * T
    const int hslot = tid >> 3, head = tid & 7;                        // the (slot, head) this thread serves
    // ---- steps 1 and 3: live, candidate, and whether the votes have to be read ------------------------------------------------------
    bool cand = false, need = false;
    int m_id = 0, m_lo = 0, m_hi = 0;
    if (tid < TR_SLOTS) {
        if (tid < T) {
            const int4 h = *(const int4*)(sst + (long long)tid * TR_SLOT_WORDS);       // id, first, last, hits
            int4* mline = (int4*)(memo + (line0 + tid) * WL_MEMO_WORDS);
            if (h.w > 0) {
                const int4 m0 = mline[0];
                m_id = m0.x; m_lo = m0.y; m_hi = m0.z;
                cand = h.w >= min_hits;
                need = cand && !(m_id == h.x + 1 && mline[1].w == h.z);
            } else {
                mline[0] = make_int4(0, 0, 0, 0);
                mline[1] = make_int4(0, 0, 0, 0);
            }
        }
        s_need[tid] = need ? 1 : 0;
    }
    __syncthreads();
    // ---- step 2: rule 8, one thread per (slot, head) -------------------------------------------------------------------------------
    if (hslot < T && s_need[hslot]) {
        track_read_head(sst + (long long)hslot * TR_SLOT_WORDS, head, ncls.v[head], s_best[tid], s_share[tid]);
    }
    __syncthreads();
    // ---- steps 3 and 4: fresh slots, numbered in slot order ------------------------------------------------------------------------
    bool fresh = false;
    if (need) {
        unsigned lo, hi;
        pack_key(s_best + tid * TR_HEADS, lo, hi);
        const int4 h = *(const int4*)(sst + (long long)tid * TR_SLOT_WORDS);
        fresh = m_id != h.x + 1 || m_lo != (int)lo || m_hi != (int)hi;
    }
    const unsigned long long fm = __ballot(fresh);
    if (tid < TR_SLOTS && lane == 0) s_wcnt[wave] = __popcll(fm);
    __syncthreads();
    const int nfresh = s_wcnt[0] + s_wcnt[1];
    if (tid < TR_SLOTS) {
        const int j = fresh ? (wave == 1 ? s_wcnt[0] : 0) + __popcll(fm & ((1ull << lane) - 1ull)) : -1;
        s_pos[tid] = j;
        if (tid < T) {
            pos[line0 + tid] = j;
            if (fresh) q_slot[line0 + j] = tid;
            if (tid >= nfresh) q_slot[line0 + tid] = -1;
        }
    }
    if (tid == 0) q_count[s] = nfresh;
    __syncthreads();
    if (hslot < T && s_pos[hslot] >= 0) {                              // the record the track would leave if it ended now
        write_record_share(q_i + (line0 + s_pos[hslot]) * RM_REC_WORDS, q_f + (line0 + s_pos[hslot]) * RM_REC_WORDS,
                           sst + (long long)hslot * TR_SLOT_WORDS, head, s_best[tid], s_share[tid]);
    }
    for (int w = nfresh * RM_REC_WORDS + tid; w < T * RM_REC_WORDS; w += blockDim.x) {       // the lines past the count
        q_i[line0 * RM_REC_WORDS + w] = 0;
        q_f[line0 * RM_REC_WORDS + w] = 0.f;
    }
}

// grid (n_streams), block (128)
__global__ __launch_bounds__(TR_SLOTS) void live_scatter_kernel(const int* __restrict__ state, int T, long long sstride,
                                                               const int32_t* __restrict__ q_i, const int32_t* __restrict__ pos,
                                                               const int32_t* __restrict__ match_i, int32_t* __restrict__ memo,
                                                               int32_t* __restrict__ live_i, const int32_t* __restrict__ match_align,
                                                               int32_t* __restrict__ live_align) {
    const int s = blockIdx.x, t = threadIdx.x;
    if (t >= T) return;
    const long long line = (long long)s * T + t;
    int align = 0;                                                     // step 8 (live_align != nullptr: lp_watch_live_indel)
    const int4 h = *(const int4*)(state + (long long)s * sstride + TR_HDR_WORDS + (long long)t * TR_SLOT_WORDS);   // id, first, last, hits
    int4* mline = (int4*)(memo + line * WL_MEMO_WORDS);
    int4 out0 = make_int4(-1, -1, 0, 0), out1 = make_int4(0, 0, 0, 0);
    const int j = pos[line];
    if (j >= 0) {                                                      // step 6 (a fresh slot is live)
        const int32_t* ri = q_i + ((long long)s * T + j) * RM_REC_WORDS;
        const int4 m = *(const int4*)(match_i + ((long long)s * T + j) * 4);            // entry, mismatches, cost, n_hits
        // pack_key of lp_track_read.inc, written out: called from here it splits this kernel's load of h (profiles/live_stage_codegen.txt)
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            lo |= (unsigned)ri[RM_W_IDS + p] << (8 * p);
            hi |= (unsigned)ri[RM_W_IDS + 4 + p] << (8 * p);
        }
        mline[0] = make_int4(h.x + 1, (int)lo, (int)hi, m.x);
        mline[1] = make_int4(m.y, m.z, m.w, h.z);
        out0 = make_int4(h.x, m.x, m.y, m.z);
        out1 = make_int4(m.w, 1, h.w, h.z);
        if (live_align != nullptr) align = match_align[(long long)s * T + j];
    } else if (h.w > 0) {
        const int4 m0 = mline[0];
        if (m0.x == h.x + 1) {
            const int4 m1 = mline[1];
            out0 = make_int4(h.x, m0.w, m1.x, m1.y);
            out1 = make_int4(m1.z, 0, h.w, m1.w);
            if (live_align != nullptr) align = live_align[line];
        }
    }
    if (live_align != nullptr) live_align[line] = align;
    int4* row = (int4*)(live_i + line * WL_LIVE_COLS);
    row[0] = out0;
    row[1] = out1;
}

}  // namespace

}  // namespace lp

using namespace lp;

extern "C" size_t lp_watch_live_state_bytes(int n_streams, int max_tracks) {
    if (!live_dims_fault(n_streams, max_tracks).empty()) return 0;
    return (size_t)n_streams * max_tracks * WL_MEMO_WORDS * 4;
}

extern "C" size_t lp_watch_live_workspace_bytes(int n_streams, int max_tracks) {
    if (!live_dims_fault(n_streams, max_tracks).empty()) return 0;
    return live_carve(nullptr, (size_t)n_streams, (size_t)max_tracks).bytes;
}

extern "C" size_t lp_watch_live_indel_workspace_bytes(int n_streams, int max_tracks) {
    if (!live_dims_fault(n_streams, max_tracks).empty()) return 0;
    return live_carve(nullptr, (size_t)n_streams, (size_t)max_tracks).indel_bytes;
}

// Both entry points.  with_indel: lp_watch_live_indel (indel, gap_cost and live_align are its own; the workspace is the larger one).
static int watch_live_run(const std::string& fn, bool with_indel, const void* track_state, int n_streams, int max_tracks, const int* ncls,
                          int min_hits, int32_t* memo, const unsigned char* entries, int n_entries, const unsigned char* confuse,
                          int max_mismatch, int max_cost, int indel, int gap_cost, int32_t* q_i, float* q_f, int32_t* q_slot, int32_t* q_count,
                          int32_t* live_i, int32_t* live_align, void* workspace, size_t workspace_bytes, void* stream) {
    TrackNcls nc;
    std::string why = live_dims_fault(n_streams, max_tracks);
    if (why.empty()) why = ncls_fault(ncls, nc);
    if (why.empty()) why = min_hits_fault(min_hits);
    if (!why.empty()) return fail(LP_ERR_ARG, fn + why);
    if (n_entries < 0 || n_entries > LP_WATCH_MAX_ENTRIES)
        return fail(LP_ERR_ARG, fn + "n_entries " + std::to_string(n_entries) + " (need 0.." + std::to_string(LP_WATCH_MAX_ENTRIES) + ")");
    if (const std::string f = match_limits_fault(max_mismatch, max_cost); !f.empty()) return fail(LP_ERR_ARG, fn + f);
    if (with_indel && (indel < 0 || indel > 1 || gap_cost < 0 || gap_cost > LP_WATCH_MAX_GAP_COST))
        return fail(LP_ERR_ARG, fn + "need indel in 0..1 and gap_cost in 0.." + std::to_string(LP_WATCH_MAX_GAP_COST));
    if (!track_state || !memo || !q_i || !q_f || !q_slot || !q_count || !live_i || !workspace || (n_entries > 0 && !entries) ||
        (with_indel && !live_align))
        return fail(LP_ERR_ARG, fn + "null pointer");
    if (((uintptr_t)track_state & 15) != 0 || ((uintptr_t)memo & 15) != 0 || ((uintptr_t)live_i & 15) != 0 || ((uintptr_t)workspace & 15) != 0)
        return fail(LP_ERR_ARG, fn + "the tracker state, the memo, live_i and the workspace must be 16-byte aligned");
    if (n_entries > 0 && (((uintptr_t)entries & 7) != 0 || ((uintptr_t)confuse & 3) != 0))
        return fail(LP_ERR_ARG, fn + "entries must be 8-byte and confuse 4-byte aligned");
    const LiveWs ws = live_carve(workspace, (size_t)n_streams, (size_t)max_tracks);
    const size_t ws_bytes = with_indel ? ws.indel_bytes : ws.bytes;
    if (workspace_bytes < ws_bytes)
        return fail(LP_ERR_ARG, fn + "workspace of " + std::to_string(workspace_bytes) + " bytes, need " + std::to_string(ws_bytes));
    const long long sstride = track_state_stride(max_tracks);
    {   // no buffer that is written may overlap the state, the list or another one
        const size_t L = (size_t)n_streams * max_tracks;
        const Region reg[] = {{track_state, (size_t)n_streams * (size_t)sstride * 4, false},
                              {entries, (size_t)n_entries * 8, false},
                              {confuse, n_entries > 0 && confuse ? (size_t)3 * 64 * 64 : 0, false},
                              {memo, L * WL_MEMO_WORDS * 4, true},
                              {q_i, L * RM_REC_WORDS * 4, true},
                              {q_f, L * RM_REC_WORDS * 4, true},
                              {q_slot, L * 4, true},
                              {q_count, (size_t)n_streams * 4, true},
                              {live_i, L * WL_LIVE_COLS * 4, true},
                              {live_align, with_indel ? L * 4 : 0, true},
                              {workspace, ws_bytes, true}};
        if (regions_clash(reg, (int)(sizeof(reg) / sizeof(reg[0]))))
            return fail(LP_ERR_ARG, fn + (with_indel ? "the memo, the queries, live_i, live_align and the workspace may overlap neither an input nor each other"
                                                     : "the memo, the queries, live_i and the workspace may overlap neither an input nor each other"));
    }

    hipStream_t st = (hipStream_t)stream;
    const int threads = max_tracks * TR_HEADS <= TR_SLOTS ? TR_SLOTS : round_up(max_tracks * TR_HEADS, 64);
    hipLaunchKernelGGL(live_gather_kernel, dim3((unsigned)n_streams), dim3((unsigned)threads), 0, st, (const int*)track_state, max_tracks, sstride, nc,
                       min_hits, memo, q_i, q_f, q_slot, q_count, ws.pos);
    LP_HIP_CHECK(hipGetLastError());
    if (int rc = with_indel ? lp_watch_match_indel(entries, n_entries, confuse, q_i, q_f, q_count, n_streams, max_tracks, max_mismatch, max_cost,
                                                   indel, gap_cost, ws.match_i, ws.match_align, ws.watch, ws.watch_bytes, stream)
                            : lp_watch_match(entries, n_entries, confuse, q_i, q_f, q_count, n_streams, max_tracks, max_mismatch, max_cost,
                                             ws.match_i, ws.watch, ws.watch_bytes, stream))
        return rc;
    hipLaunchKernelGGL(live_scatter_kernel, dim3((unsigned)n_streams), dim3(TR_SLOTS), 0, st, (const int*)track_state, max_tracks, sstride, q_i, ws.pos,
                       ws.match_i, memo, live_i, with_indel ? ws.match_align : nullptr, with_indel ? live_align : nullptr);
    LP_HIP_CHECK(hipGetLastError());
    return LP_OK;
}

extern "C" int lp_watch_live(const void* track_state, int n_streams, int max_tracks, const int* ncls, int min_hits, int32_t* memo,
                             const unsigned char* entries, int n_entries, const unsigned char* confuse, int max_mismatch, int max_cost,
                             int32_t* q_i, float* q_f, int32_t* q_slot, int32_t* q_count, int32_t* live_i, void* workspace,
                             size_t workspace_bytes, void* stream) {
    return watch_live_run("lp_watch_live: ", false, track_state, n_streams, max_tracks, ncls, min_hits, memo, entries, n_entries, confuse,
                          max_mismatch, max_cost, 0, 0, q_i, q_f, q_slot, q_count, live_i, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int lp_watch_live_indel(const void* track_state, int n_streams, int max_tracks, const int* ncls, int min_hits, int32_t* memo,
                                   const unsigned char* entries, int n_entries, const unsigned char* confuse, int max_mismatch, int max_cost,
                                   int indel, int gap_cost, int32_t* q_i, float* q_f, int32_t* q_slot, int32_t* q_count, int32_t* live_i,
                                   int32_t* live_align, void* workspace, size_t workspace_bytes, void* stream) {
    return watch_live_run("lp_watch_live_indel: ", true, track_state, n_streams, max_tracks, ncls, min_hits, memo, entries, n_entries, confuse,
                          max_mismatch, max_cost, indel, gap_cost, q_i, q_f, q_slot, q_count, live_i, live_align, workspace, workspace_bytes, stream);
}
