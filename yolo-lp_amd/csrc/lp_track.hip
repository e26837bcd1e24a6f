// Plate tracking across video frames with a per-track vote over the eight character heads: lp_track_update (include/lp_hip.h)
// keeps a small device-resident tracker per stream.  The reference has nothing here (its Inferer treats video frames
// independently, yolov6/core/inferer.py); the written-down specification is yolov6/utils/track.py::PlateTrackerNp, which this
// kernel matches bit for bit (tests/test_track_gpu.py).
//
// One workgroup of 1024 threads per stream of a launch; it takes the stream's frames of the launch in order.  Per frame:
//   1. threads 0..127 predict and expand the live slots' boxes, threads 128..255 expand the detection boxes (LDS);
//   2. all waves fill the (slot, row) IoU matrix; a pair above the threshold appends the key (descending IoU bits,
//      slot * 128 + row) -- score_key of lp_score.inc -- to the key list in LDS.  The order of the list is irrelevant: the keys are
//      distinct and sorted next.  At most 128 x 128 keys = 128 KiB, the budget of merge_tiles_kernel;
//   3. the list, padded with all-ones keys to a power of two, is sorted with the bitonic step of lp_nms_shared.inc;
//   4. wave 0 settles the matches in that order, 64 keys at a time: taken slots and rows are four 64-bit masks in registers,
//      the keys of a chunk that are still free take turns by ballot;
//   5. one thread per slot applies the match (velocity, box, corners, counters) or the miss; the tracks that end are numbered in
//      slot order by ballot, their records are written by one thread per (slot, head) and their slots zeroed;
//   6. wave 0 hands the free slots, in order, to the unmatched rows that pass new_thres, in order;
//   7. one thread per (slot, head) casts the vote of a matched or new slot and reads the head (best, share) into LDS;
//   8. all threads write the frame's output rows and track ids.
// lp_track_update_hold runs the <true> instantiation (rule 11, read-only on the state): step 5 also marks the missed slots that
// pass the two gates ST_HELD and numbers them in slot order (ballot and prefix count over the two waves of 128 slots, as end_marked
// numbers the ending tracks); step 7 reads their heads into the same two tables; step 8 also writes det_hold / count_hold /
// tid_hold: the frame's rows, then one predicted row per held slot.  Every other caller runs <false>, whose code is the kernel
// without all this (profiles/hold_codegen.txt).
// The state of a stream (16 header words, 544 words per slot: TR_*) and the ended record (RM_*) are laid out in lp_streams.h; rule 8 and
// the record writer are lp_track_read.inc's, shared with the stages that read the state behind this kernel.  The ballot numbering of
// steps 5 and 5 <true> stays written out here: as a shared function it re-lays this kernel's spilled SGPRs (profiles/live_stage_codegen.txt).
#include "lp_internal.h"
#include "lp_streams.h"
#include "lp_score.inc"
#include "lp_nms_shared.inc"
#include "lp_track_read.inc"
#include <cstring>

namespace lp {

namespace {

constexpr int TK_T = SORT_T;                    // threads of the workgroup (bitonic_step strides by SORT_T)
constexpr int TK_ROWS = LP_TRACK_MAX_DETS;      // 128
constexpr int TK_FRAMES = LP_FRAMES_PER_LAUNCH; // frames (and streams) per launch: the table travels as kernel arguments
static_assert(TR_SLOTS * TK_ROWS == SORT_LDS_KEYS && TK_T / TR_HEADS == TR_SLOTS && TK_ROWS == 128, "track kernel geometry");

enum { ST_EMPTY = 0, ST_LIVE = 1, ST_MATCHED = 2, ST_ENDING = 3, ST_NEW = 4, ST_MISSED = 5, ST_HELD = 6 };   // ST_HELD: missed and held

struct TkTable {                                // 584 bytes of kernel arguments
    int nfr;                                    // frames of this launch
    int blk_stream[TK_FRAMES];                  // stream of workgroup k (-1: it only copies skipped frames)
    short fr_blk[TK_FRAMES];                    // workgroup that takes frame j of the launch
    unsigned char fr_skip[TK_FRAMES];           // frame j is not tracked (stream_of == -1)
    unsigned char blk_flush[TK_FRAMES];         // workgroup k ends all live tracks after its frames
};
struct TkParams { float thr_f, new_f, expand_f; int max_age; TrackNcls ncls; };
struct TkHold {                                 // rule 11 (read by the <true> instantiation only)
    int min_hits, max_misses;
    float* det;                                 // [frames, max_det + T, 28], the launch's first frame (as det_out)
    int32_t* count;                             // [frames]
    int32_t* tid;                               // [frames, max_det + T]
};

typedef float box4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ box4 expand_box(float x1, float y1, float x2, float y2, float e) {
    const float ex = e * (x2 - x1), ey = e * (y2 - y1);
    const box4 b = {x1 - ex, y1 - ey, x2 + ex, y2 + ey};
    return b;
}

// inter / (area_i + area_j - inter): the fp32 ops of iou_gt (lp_nms_shared.inc) / tiles.overlaps, the quotient itself
__device__ __forceinline__ float iou_value(const box4& a, const box4& b) {
    const float xx1 = a.x > b.x ? a.x : b.x;
    const float yy1 = a.y > b.y ? a.y : b.y;
    const float xx2 = a.z < b.z ? a.z : b.z;
    const float yy2 = a.w < b.w ? a.w : b.w;
    float w = xx2 - xx1;
    if (!(w > 0.f)) w = 0.f;
    float h = yy2 - yy1;
    if (!(h > 0.f)) h = 0.f;
    const float inter = w * h;
    const float iarea = (a.z - a.x) * (a.w - a.y);
    const float jarea = (b.z - b.x) * (b.w - b.y);
    return inter / (iarea + jarea - inter);
}

__global__ void track_clear_kernel(int32_t* ended_count, int n_streams, int32_t* ended_i, float* ended_f, long long n_words) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_streams) ended_count[i] = 0;
    if (i < n_words) { ended_i[i] = 0; ended_f[i] = 0.f; }
}

// grid (workgroups of this launch), block (1024), dynamic LDS = n_max keys (8 B), n_max >= max_tracks * min(max_det, 128).
//   det / count / det_out / tid_out / slot_out (may be null): the launch's first frame; state, ended_*: the whole call's.
template <bool HOLD>
__global__ __launch_bounds__(TK_T) void track_kernel(const TkTable tab, const TkParams prm, int* __restrict__ state, int T, long long sstride,
                                                    const float* __restrict__ det, const int32_t* __restrict__ count, int max_det,
                                                    float* __restrict__ det_out, int32_t* __restrict__ tid_out, int32_t* __restrict__ slot_out,
                                                    int32_t* __restrict__ ended_i, float* __restrict__ ended_f, int32_t* __restrict__ ended_count,
                                                    int max_ended, const TkHold hold) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long skeys[];
    __shared__ __attribute__((aligned(16))) box4 s_pbox[TR_SLOTS];     // predicted, expanded boxes of the live slots
    __shared__ __attribute__((aligned(16))) box4 s_dbox[TK_ROWS];      // expanded boxes of the rows
    __shared__ int s_slot_row[TR_SLOTS], s_row_slot[TK_ROWS], s_status[TR_SLOTS], s_id[TR_SLOTS], s_endpos[TR_SLOTS], s_free[TR_SLOTS];
    __shared__ float s_share[TR_SLOTS * TR_HEADS];
    __shared__ int s_best[TR_SLOTS * TR_HEADS];
    __shared__ int s_ncls[TR_HEADS];
    __shared__ int s_nkeys, s_wcnt[2], s_nfree, s_made, s_drop;
    __shared__ int s_hslot[HOLD ? TR_SLOTS : 1], s_hcnt[2];           // HOLD: the held slots in slot order, their number per wave
    const int blk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int strm = tab.blk_stream[blk];
    int* const sst = state + (strm >= 0 ? (long long)strm * sstride : 0);
    const int hslot = tid >> 3, head = tid & 7;                        // the (slot, head) this thread serves
    int* const hsl = sst + TR_HDR_WORDS + hslot * TR_SLOT_WORDS;
    if (tid < TR_HEADS) s_ncls[tid] = prm.ncls.v[tid];
    int ended_n = strm >= 0 ? ended_count[strm] : 0;                   // (written by thread 0 at the very end only)
    __syncthreads();
    const unsigned long long lt = (1ull << lane) - 1ull;

    // the slots marked ST_ENDING (`ending` of threads 0..127, in slot order) write their records and are zeroed
    auto end_marked = [&](bool ending) {
        const unsigned long long em = __ballot(ending);
        if (tid < TR_SLOTS && lane == 0) s_wcnt[wave] = __popcll(em);
        __syncthreads();
        if (ending) s_endpos[tid] = ended_n + (wave == 1 ? s_wcnt[0] : 0) + __popcll(em & lt);
        __syncthreads();
        const bool mine = hslot < T && s_status[hslot] == ST_ENDING;
        if (mine) {
            const int pos = s_endpos[hslot];
            if (pos < max_ended) {
                int best;
                float share;
                track_read_head(hsl, head, s_ncls[head], best, share);
                write_record_share(ended_i + ((long long)strm * max_ended + pos) * RM_REC_WORDS,
                                   ended_f + ((long long)strm * max_ended + pos) * RM_REC_WORDS, hsl, head, best, share);
            }
        }
        __syncthreads();
        if (mine) {
#pragma unroll 4
            for (int w = head; w < TR_SLOT_WORDS; w += TR_HEADS) hsl[w] = 0;
        }
        ended_n += s_wcnt[0] + s_wcnt[1];
        __syncthreads();
    };

    for (int j = 0; j < tab.nfr; ++j) {                                // (block-uniform control flow throughout)
        if (tab.fr_blk[j] != blk) continue;
        const float* rows = det + (long long)j * max_det * LP_DET_COLS;
        int nc = count[j];
        nc = nc < 0 ? 0 : (nc > max_det ? max_det : nc);
        const bool skip = tab.fr_skip[j] != 0;
        const int n = skip ? 0 : (nc < TK_ROWS ? nc : TK_ROWS);
        if (!skip) {
            const int frame = sst[0];
            int next_id = sst[1], dropped = sst[2];
            // ---- 1. predicted / expanded boxes ----------------------------------------------------------------------------
            if (tid < TR_SLOTS) {
                int st = ST_EMPTY;
                if (tid < T) {
                    const int* sl = sst + TR_HDR_WORDS + tid * TR_SLOT_WORDS;
                    if (sl[3] > 0) {
                        const float k = (float)(sl[4] + 1);
                        const float dx = __int_as_float(sl[TR_W_VEL]) * k, dy = __int_as_float(sl[TR_W_VEL + 1]) * k;
                        s_pbox[tid] = expand_box(__int_as_float(sl[TR_W_BOX]) + dx, __int_as_float(sl[TR_W_BOX + 1]) + dy,
                                                 __int_as_float(sl[TR_W_BOX + 2]) + dx, __int_as_float(sl[TR_W_BOX + 3]) + dy, prm.expand_f);
                        st = ST_LIVE;
                    }
                }
                s_status[tid] = st;
                s_slot_row[tid] = -1;
                s_row_slot[tid] = -1;
            } else if (tid < TR_SLOTS + TK_ROWS) {
                const int r = tid - TR_SLOTS;
                if (r < n) s_dbox[r] = expand_box(rows[r * LP_DET_COLS], rows[r * LP_DET_COLS + 1], rows[r * LP_DET_COLS + 2],
                                                  rows[r * LP_DET_COLS + 3], prm.expand_f);
            }
            if (tid == 0) s_nkeys = 0;
            __syncthreads();
            // ---- 2. pairs ---------------------------------------------------------------------------------------------------
            for (int p = tid; p < T * n; p += TK_T) {
                const int slot = p / n, row = p - slot * n;
                if (s_status[slot] == ST_LIVE) {
                    const float iou = iou_value(s_pbox[slot], s_dbox[row]);
                    if (iou > prm.thr_f)                        // thr_f = largest fp32 <= match_thres  <=>  (double)iou > match_thres
                        skeys[atomicAdd(&s_nkeys, 1)] = score_key(iou, slot * TK_ROWS + row);
                }
            }
            __syncthreads();
            const int nk = s_nkeys;
            int np2 = 64;
            while (np2 < nk) np2 <<= 1;
            for (int s = nk + tid; s < np2; s += TK_T) skeys[s] = ~0ull;
            __syncthreads();
            // ---- 3. sort: descending IoU, ties by slot, then row ------------------------------------------------------------
            if (nk > 1) {
                for (int k = 2; k <= np2; k <<= 1)
                    for (int jj = k >> 1; jj > 0; jj >>= 1) {
                        bitonic_step(skeys, np2, 0, k, jj);
                        __syncthreads();
                    }
            }
            // ---- 4. greedy matching in that order ---------------------------------------------------------------------------
            if (wave == 0) {
                unsigned long long sm0 = 0, sm1 = 0, rm0 = 0, rm1 = 0;      // taken slots / rows (wave-uniform)
                const int most = T < n ? T : n;
                int nm = 0;
                for (int c = 0; c < nk && nm < most; c += 64) {
                    const int i = c + lane;
                    int slot = 0, row = 0;
                    bool ok = i < nk;
                    if (ok) {
                        const unsigned v = (unsigned)(skeys[i] & 0xffffffffull);
                        slot = (int)(v >> 7);
                        row = (int)(v & 127u);
                        ok = !(((slot < 64 ? sm0 : sm1) >> (slot & 63)) & 1ull) && !(((row < 64 ? rm0 : rm1) >> (row & 63)) & 1ull);
                    }
                    unsigned long long todo = __ballot(ok);
                    while (todo) {
                        const int k = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
                        const int ks = __builtin_amdgcn_readlane(slot, k), kr = __builtin_amdgcn_readlane(row, k);
                        if (lane == k) { s_slot_row[ks] = kr; s_row_slot[kr] = ks; }
                        if (ks < 64) sm0 |= 1ull << ks; else sm1 |= 1ull << (ks - 64);
                        if (kr < 64) rm0 |= 1ull << kr; else rm1 |= 1ull << (kr - 64);
                        ++nm;
                        todo &= ~__ballot(slot == ks || row == kr);         // (lane k itself included)
                    }
                }
            }
            __syncthreads();
            // ---- 5. matched and unmatched slots ------------------------------------------------------------------------------
            bool ending = false, held = false;
            if (tid < T && s_status[tid] == ST_LIVE) {
                int* sl = sst + TR_HDR_WORDS + tid * TR_SLOT_WORDS;
                const int r = s_slot_row[tid];
                if (r >= 0) {
                    const float* row = rows + r * LP_DET_COLS;
                    const float k = (float)(sl[4] + 1);
                    const float ox1 = __int_as_float(sl[TR_W_BOX]), oy1 = __int_as_float(sl[TR_W_BOX + 1]);
                    const float ox2 = __int_as_float(sl[TR_W_BOX + 2]), oy2 = __int_as_float(sl[TR_W_BOX + 3]);
                    const float nx1 = row[0], ny1 = row[1], nx2 = row[2], ny2 = row[3];
                    const float vx = ((nx1 + nx2) * 0.5f - (ox1 + ox2) * 0.5f) / k;
                    const float vy = ((ny1 + ny2) * 0.5f - (oy1 + oy2) * 0.5f) / k;
                    sl[TR_W_VEL] = __float_as_int(vx);
                    sl[TR_W_VEL + 1] = __float_as_int(vy);
                    for (int c = 0; c < 12; ++c) sl[TR_W_BOX + c] = __float_as_int(row[c]);
                    sl[3] = sl[3] + 1;
                    sl[4] = 0;
                    sl[2] = frame;
                    s_id[tid] = sl[0];
                    s_status[tid] = ST_MATCHED;
                } else {
                    const int m = sl[4] + 1;
                    sl[4] = m;
                    ending = m > prm.max_age;
                    if (HOLD) held = !ending && sl[3] >= hold.min_hits && m <= hold.max_misses;
                    s_status[tid] = ending ? ST_ENDING : (held ? ST_HELD : ST_MISSED);
                }
            }
            unsigned long long hm = 0;
            if (HOLD) {                                                // (made visible by the barriers of end_marked)
                hm = __ballot(held);
                if (tid < TR_SLOTS && lane == 0) s_hcnt[wave] = __popcll(hm);
            }
            end_marked(ending);
            if (HOLD && held) s_hslot[(wave == 1 ? s_hcnt[0] : 0) + __popcll(hm & lt)] = tid;   // (read behind the barriers of step 6)
            // ---- 6. new tracks: the free slots, in order, to the unmatched rows that pass new_thres, in order ---------------
            if (wave == 0) {
                const bool f0 = lane < T && (s_status[lane] == ST_EMPTY || s_status[lane] == ST_ENDING);
                const bool f1 = lane + 64 < T && (s_status[lane + 64] == ST_EMPTY || s_status[lane + 64] == ST_ENDING);
                const unsigned long long fm0 = __ballot(f0), fm1 = __ballot(f1);
                if (f0) s_free[__popcll(fm0 & lt)] = lane;
                if (f1) s_free[__popcll(fm0) + __popcll(fm1 & lt)] = lane + 64;
                if (lane == 0) s_nfree = __popcll(fm0) + __popcll(fm1);
            }
            __syncthreads();
            if (wave == 0) {
                auto wants = [&](int r) {
                    if (r >= n || s_row_slot[r] >= 0) return false;
                    const float* row = rows + r * LP_DET_COLS;
                    float sc = row[12] + row[13];
                    sc = sc + row[14]; sc = sc + row[15]; sc = sc + row[16]; sc = sc + row[17]; sc = sc + row[18]; sc = sc + row[19];
                    sc = sc / 8.0f;
                    return sc >= prm.new_f;                     // new_f = smallest fp32 >= new_thres  <=>  (double)sc >= new_thres
                };
                const bool c0 = wants(lane), c1 = wants(lane + 64);
                const unsigned long long cm0 = __ballot(c0), cm1 = __ballot(c1);
                const int nfree = s_nfree, ncand = __popcll(cm0) + __popcll(cm1);
                const int k0 = __popcll(cm0 & lt), k1 = __popcll(cm0) + __popcll(cm1 & lt);
                if (c0 && k0 < nfree) {
                    const int slot = s_free[k0];
                    s_row_slot[lane] = slot; s_slot_row[slot] = lane; s_status[slot] = ST_NEW; s_id[slot] = next_id + k0;
                }
                if (c1 && k1 < nfree) {
                    const int slot = s_free[k1];
                    s_row_slot[lane + 64] = slot; s_slot_row[slot] = lane + 64; s_status[slot] = ST_NEW; s_id[slot] = next_id + k1;
                }
                if (lane == 0) { s_made = ncand < nfree ? ncand : nfree; s_drop = ncand - (ncand < nfree ? ncand : nfree); }
            }
            __syncthreads();
            next_id += s_made;
            dropped += s_drop;
            // ---- 7. votes and reads, one thread per (slot, head) -------------------------------------------------------------
            {
                const int st = hslot < T ? s_status[hslot] : ST_EMPTY;
                if (st == ST_MATCHED || st == ST_NEW) {
                    const float* row = rows + s_slot_row[hslot] * LP_DET_COLS;
                    float* votes = (float*)(hsl + TR_W_VOTES + head * LP_TRACK_MAX_CLS);
                    float* total = (float*)(hsl + TR_W_TOTAL + head);
                    if (st == ST_NEW) {
#pragma unroll 4
                        for (int c = 0; c < LP_TRACK_MAX_CLS; ++c) votes[c] = 0.f;
                        *total = 0.f;
                        if (head == 0) {
                            hsl[0] = s_id[hslot]; hsl[1] = frame; hsl[2] = frame; hsl[3] = 1; hsl[4] = 0;
                            hsl[TR_W_VEL] = 0; hsl[TR_W_VEL + 1] = 0;
                        }
                        if (head < 4)
                            for (int c = head; c < 12; c += 4) hsl[TR_W_BOX + c] = __float_as_int(row[c]);
                    }
                    const float v = row[20 + head], conf = row[12 + head];
                    if (conf > 0.f && v >= 0.f && v < (float)s_ncls[head]) {
                        votes[(int)v] = votes[(int)v] + conf;
                        *total = *total + conf;
                    }
                    track_read_head(hsl, head, s_ncls[head], s_best[tid], s_share[tid]);
                } else if (HOLD && st == ST_HELD) {                    // a held slot casts no vote: its read as it stands
                    track_read_head(hsl, head, s_ncls[head], s_best[tid], s_share[tid]);
                }
            }
            __syncthreads();
            if (tid == 0) { sst[0] = frame + 1; sst[1] = next_id; sst[2] = dropped; }
        }
        // ---- 8. outputs ---------------------------------------------------------------------------------------------------------
        float* dout = det_out + (long long)j * max_det * LP_DET_COLS;
        for (int i = tid; i < max_det * LP_DET_COLS; i += TK_T) {
            const int r = i / LP_DET_COLS, col = i - r * LP_DET_COLS;
            float v = 0.f;
            if (r < nc) {
                v = rows[i];
                if (r < n && col >= 12) {
                    const int slot = s_row_slot[r];
                    if (slot >= 0) v = col < 20 ? s_share[slot * TR_HEADS + col - 12] : (float)s_best[slot * TR_HEADS + col - 20];
                }
            }
            dout[i] = v;
            if (HOLD && r < nc) hold.det[(long long)j * (max_det + T) * LP_DET_COLS + i] = v;
        }
        for (int r = tid; r < max_det; r += TK_T) {
            int v = -1, slot = -1;
            if (r < n) {
                slot = s_row_slot[r];
                if (slot >= 0) v = s_id[slot];
            }
            tid_out[(long long)j * max_det + r] = v;
            if (slot_out) slot_out[(long long)j * max_det + r] = slot;
            if (HOLD && r < nc) hold.tid[(long long)j * (max_det + T) + r] = v;
        }
        if (HOLD) {                                                    // rule 11: the held rows behind the frame's nc, then zero rows
            const int hrows = max_det + T, nheld = skip ? 0 : s_hcnt[0] + s_hcnt[1];
            float* dh = hold.det + (long long)j * hrows * LP_DET_COLS;
            for (int i = nc * LP_DET_COLS + tid; i < hrows * LP_DET_COLS; i += TK_T) {
                const int r = i / LP_DET_COLS, col = i - r * LP_DET_COLS;
                float v = 0.f;
                if (r - nc < nheld) {
                    const int slot = s_hslot[r - nc];
                    const int* sl = sst + TR_HDR_WORDS + slot * TR_SLOT_WORDS;
                    if (col < 12) {                                    // the products of step 1 of this frame: k = (float)misses
                        const float d = __int_as_float(sl[TR_W_VEL + (col & 1)]) * (float)sl[4];
                        v = __int_as_float(sl[TR_W_BOX + col]) + d;
                    } else {
                        v = col < 20 ? s_share[slot * TR_HEADS + col - 12] : (float)s_best[slot * TR_HEADS + col - 20];
                    }
                }
                dh[i] = v;
            }
            for (int r = nc + tid; r < hrows; r += TK_T)
                hold.tid[(long long)j * hrows + r] = r - nc < nheld ? sst[TR_HDR_WORDS + s_hslot[r - nc] * TR_SLOT_WORDS] : -1;
            if (tid == 0) hold.count[j] = nc + nheld;
        }
        __syncthreads();                                               // the next frame reuses the LDS tables and reads the state
    }
    if (strm >= 0 && tab.blk_flush[blk]) {                             // flush: every live track ends, in slot order
        bool ending = false;
        if (tid < TR_SLOTS) {
            ending = tid < T && sst[TR_HDR_WORDS + tid * TR_SLOT_WORDS + 3] > 0;
            s_status[tid] = ending ? ST_ENDING : ST_EMPTY;
        }
        end_marked(ending);
    }
    if (tid == 0 && strm >= 0) ended_count[strm] = ended_n;
}

}  // namespace

}  // namespace lp

using namespace lp;

extern "C" size_t lp_track_state_bytes(int n_streams, int max_tracks) {
    if (n_streams < 1 || max_tracks < 1 || max_tracks > LP_TRACK_MAX_TRACKS) return 0;
    return (size_t)n_streams * (size_t)track_state_stride(max_tracks) * 4;
}

extern "C" size_t lp_track_dropped_offset(int max_tracks, int stream_index) {
    if (stream_index < 0 || max_tracks < 1 || max_tracks > LP_TRACK_MAX_TRACKS) return (size_t)-1;
    return ((size_t)stream_index * (size_t)track_state_stride(max_tracks) + 2) * 4;
}

extern "C" int lp_track_update(void* state, int n_streams, int max_tracks, const lp_track_params* p, const float* det, const int32_t* count,
                               int B, int max_det, const int* stream_of, const unsigned char* flush, float* det_out, int32_t* tid,
                               int32_t* ended_i, float* ended_f, int32_t* ended_count, int max_ended, void* stream) {
    return lp_track_update_slots(state, n_streams, max_tracks, p, det, count, B, max_det, stream_of, flush, det_out, tid, nullptr, ended_i,
                                 ended_f, ended_count, max_ended, stream);
}

extern "C" int lp_track_update_slots(void* state, int n_streams, int max_tracks, const lp_track_params* p, const float* det,
                                     const int32_t* count, int B, int max_det, const int* stream_of, const unsigned char* flush, float* det_out,
                                     int32_t* tid, int32_t* slot, int32_t* ended_i, float* ended_f, int32_t* ended_count, int max_ended,
                                     void* stream) {
    return lp_track_update_hold(state, n_streams, max_tracks, p, det, count, B, max_det, stream_of, flush, det_out, tid, slot, ended_i,
                                ended_f, ended_count, max_ended, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int lp_track_update_hold(void* state, int n_streams, int max_tracks, const lp_track_params* p, const float* det,
                                    const int32_t* count, int B, int max_det, const int* stream_of, const unsigned char* flush, float* det_out,
                                    int32_t* tid, int32_t* slot, int32_t* ended_i, float* ended_f, int32_t* ended_count, int max_ended,
                                    const lp_track_hold_params* hp, float* det_hold, int32_t* count_hold, int32_t* tid_hold, void* stream) {
    const std::string fn = "lp_track_update: ";
    std::string why = stream_dims_fault(n_streams, max_tracks);
    if (!why.empty()) return fail(LP_ERR_ARG, fn + why);
    if (B < 0 || max_det < 1 || max_det > 0x7fffffff / LP_DET_COLS || max_ended < 0)
        return fail(LP_ERR_ARG, fn + "need B >= 0, max_det >= 1 and max_ended >= 0");
    if (hp && (hp->min_hits < 1 || hp->max_misses < 0)) return fail(LP_ERR_ARG, fn + "hold needs min_hits >= 1 and max_misses >= 0");
    if (hp && max_det > 0x7fffffff / LP_DET_COLS - max_tracks) return fail(LP_ERR_ARG, fn + "hold: max_det + max_tracks rows overflow");
    if (!p) return fail(LP_ERR_ARG, fn + "null pointer (params)");
    if (!(p->match_thres >= 0.0 && p->match_thres <= 1.0)) return fail(LP_ERR_ARG, fn + "match_thres must be in [0, 1]");
    if (!(std::fabs(p->new_thres) <= 3.0e38)) return fail(LP_ERR_ARG, fn + "new_thres must be finite (|new_thres| <= 3e38)");
    if (!(p->expand >= 0.0 && p->expand <= 1.0e6)) return fail(LP_ERR_ARG, fn + "expand must be in [0, 1e6]");
    if (p->max_age < 0) return fail(LP_ERR_ARG, fn + "max_age must be >= 0");
    TkParams prm;
    why = ncls_fault(p->ncls, prm.ncls);
    if (!why.empty()) return fail(LP_ERR_ARG, fn + why);
    if (!state || !ended_count || (max_ended > 0 && (!ended_i || !ended_f)) || (B > 0 && (!det || !count || !stream_of || !det_out || !tid)))
        return fail(LP_ERR_ARG, fn + "null pointer");
    if (((uintptr_t)state & 15) != 0) return fail(LP_ERR_ARG, fn + "state must be 16-byte aligned");
    const size_t hrows = (size_t)max_det + max_tracks;
    const size_t bytes = (size_t)B * max_det * LP_DET_COLS * sizeof(float), hbytes = (size_t)B * hrows * LP_DET_COLS * sizeof(float);
    const Region io[] = {{det, bytes, false}, {det_out, bytes, true}};
    if (regions_clash(io, 2)) return fail(LP_ERR_ARG, fn + "det_out may not alias det");
    if (hp) {
        if (B > 0 && (!det_hold || !count_hold || !tid_hold)) return fail(LP_ERR_ARG, fn + "null pointer (hold)");
        const Region held[] = {{det, bytes, false}, {det_out, bytes, false}, {det_hold, hbytes, true}};   // (det / det_out: checked above)
        if (regions_clash(held, 3)) return fail(LP_ERR_ARG, fn + "det_hold may not alias det or det_out");
    }
    why = stream_of_fault(stream_of, B, n_streams);
    if (!why.empty()) return fail(LP_ERR_ARG, fn + why);
    static std::atomic<unsigned long long> attr{0}, attr_hold{0};
    if (int rc = hp ? set_max_lds_once(track_kernel<true>, SORT_LDS_KEYS * 8, attr_hold, "track hold")
                    : set_max_lds_once(track_kernel<false>, SORT_LDS_KEYS * 8, attr, "track")) return rc;

    prm.thr_f = f32_not_above(p->match_thres);
    prm.new_f = f32_not_below(p->new_thres);
    prm.expand_f = (float)p->expand;
    prm.max_age = p->max_age;

    hipStream_t st = (hipStream_t)stream;
    const long long n_words = (long long)n_streams * max_ended * RM_REC_WORDS;
    {
        const long long n = n_words > n_streams ? n_words : n_streams;
        hipLaunchKernelGGL(track_clear_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ended_count, n_streams, ended_i, ended_f, n_words);
        LP_HIP_CHECK(hipGetLastError());
    }
    const int rows_cap = max_det < TK_ROWS ? max_det : TK_ROWS;
    int n_max = 64;
    while (n_max < max_tracks * rows_cap) n_max <<= 1;
    const size_t lds = (size_t)n_max * 8;
    const long long sstride = track_state_stride(max_tracks);
    auto launch = [&](const TkTable& tab, int nblk, int b0) -> int {
        TkHold hold = {};
        if (hp && B > 0) hold = TkHold{hp->min_hits, hp->max_misses, det_hold + (size_t)b0 * hrows * LP_DET_COLS, count_hold + b0,
                                       tid_hold + (size_t)b0 * hrows};
        hipLaunchKernelGGL(hp ? track_kernel<true> : track_kernel<false>, dim3((unsigned)nblk), dim3(TK_T), lds, st, tab, prm, (int*)state,
                           max_tracks, sstride, det ? det + (size_t)b0 * max_det * LP_DET_COLS : nullptr, count ? count + b0 : nullptr, max_det,
                           det_out ? det_out + (size_t)b0 * max_det * LP_DET_COLS : nullptr, tid ? tid + (size_t)b0 * max_det : nullptr,
                           slot ? slot + (size_t)b0 * max_det : nullptr, ended_i, ended_f, ended_count, max_ended, hold);
        LP_HIP_CHECK(hipGetLastError());
        return LP_OK;
    };
    // the last launch that holds a frame of stream s flushes it; a flushed stream without frames gets a workgroup of its own
    std::vector<int> last_chunk((size_t)n_streams, -1), blk_of((size_t)n_streams, -1);
    for (int b = 0; b < B; ++b)
        if (stream_of[b] >= 0) last_chunk[(size_t)stream_of[b]] = b / TK_FRAMES;
    for (int b0 = 0, c = 0; b0 < B; b0 += TK_FRAMES, ++c) {
        TkTable tab = {};
        tab.nfr = B - b0 < TK_FRAMES ? B - b0 : TK_FRAMES;
        const StreamPlan pl = plan_streams(stream_of + b0, tab.nfr, blk_of, UNTRACKED_DEAL);
        memcpy(tab.blk_stream, pl.blk_stream, sizeof(tab.blk_stream));
        memcpy(tab.fr_blk, pl.fr_blk, sizeof(tab.fr_blk));
        memcpy(tab.fr_skip, pl.fr_skip, sizeof(tab.fr_skip));
        for (int k = 0; k < pl.nblk; ++k) {
            const int s = pl.blk_stream[k];
            tab.blk_flush[k] = (s >= 0 && flush && flush[s] && last_chunk[(size_t)s] == c) ? 1 : 0;
        }
        if (int rc = launch(tab, pl.nblk, b0)) return rc;
    }
    if (flush) {
        TkTable tab = {};
        int nblk = 0;
        for (int s = 0; s < n_streams; ++s) {
            if (flush[s] && last_chunk[(size_t)s] < 0) {
                tab.blk_stream[nblk] = s;
                tab.blk_flush[nblk] = 1;
                ++nblk;
            }
            if (nblk == TK_FRAMES || (s == n_streams - 1 && nblk > 0)) {
                if (int rc = launch(tab, nblk, 0)) return rc;
                tab = TkTable{};
                nblk = 0;
            }
        }
    }
    return LP_OK;
}
