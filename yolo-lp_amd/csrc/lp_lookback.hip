// The look-back delay of plate redaction: lp_lookback_update (include/lp_hip.h).  Behind lp_track_update_hold a small
// device-resident delay line keeps, per stream, the redaction rows of the last `depth` frames, adds rows to those past frames
// once a new track's second detection has fixed its velocity, and hands a frame's rows out `depth` frames later.  The reference has
// nothing here; the written-down specification is yolov6/utils/lookback.py (LookbackNp), which these kernels match bit for bit
// (tests/test_lookback_gpu.py).  The file is compiled with -ffp-contract=off: the velocity and the offsets are fp32 op by op.
//
// lookback_kernel: one workgroup of 1024 threads per stream of a launch, the frame table in the kernel arguments as in
// lp_track.hip and lp_shots.hip; the untracked frames of a launch are dealt to its workgroups, which only copy them.  Per frame:
//   A  one thread per row follows its slot entry; the confirming rows are numbered in row order by ballot and prefix count over
//      the two waves of 128 rows (as end_marked numbers the ending tracks in lp_track.hip) and leave row, first frame, first
//      geometry and velocity in LDS;
//   B  one thread per target entry (frames f - D .. f - 1) walks that list in order and hands out the positions behind the
//      entry's rows (no atomics on positions, no order race); then all threads write the back rows, one 16-byte vector each;
//   C+D one pass of 16-byte vectors over the entry f % D: every thread reads its vector of the old entry (frame f - D) into the
//      release, then writes the frame's own rows over it, so the two copies need no barrier between them.
// lookback_tail_kernel (one workgroup per stream, after the call's last frame) writes the tails.
// State of a stream, in 4-byte words: f, base, dropped, one unused; per slot 16 words: id + 1, seen, first, one unused,
// geometry[12]; the D counts of the ring, padded to a multiple of 4; the D entries of rows * 28 floats.  Every part starts at a
// multiple of 16 bytes.  All zero = empty.
#include "lp_internal.h"
#include "lp_streams.h"
#include <cstring>

namespace lp {

namespace {

constexpr int LB_T = 1024;                      // threads of every workgroup here
constexpr int LB_ROWS = LP_TRACK_MAX_DETS;      // rows of a frame that take part in A
constexpr int LB_DEPTH = LP_LOOKBACK_MAX_DEPTH;
constexpr int LB_FRAMES = LP_FRAMES_PER_LAUNCH;
constexpr int LB_HDR_WORDS = 4;
constexpr int LB_SLOT_WORDS = 16;
constexpr int LB_VEC = LP_DET_COLS / 4;         // 16-byte vectors of a row

struct LbTable {                                // 452 bytes of kernel arguments
    int nfr;                                    // frames of this launch
    int blk_stream[LB_FRAMES];                  // stream of workgroup k (-1: it only copies untracked frames)
    short fr_blk[LB_FRAMES];                    // workgroup that takes frame j of the launch
    unsigned char fr_skip[LB_FRAMES];           // frame j is not tracked: released at once
};
struct LbTail {                                 // the streams s0 .. s0 + n - 1
    int s0, n;
    unsigned char flush[LB_FRAMES];
};
struct LbDims {
    int T, D, max_back, max_det, hold_rows, rows;
    long long sstride;                          // words of a stream's state
};

__host__ __device__ inline long long counts_off(int T) { return LB_HDR_WORDS + (long long)T * LB_SLOT_WORDS; }
__host__ __device__ inline long long ring_off(int T, int D) { return counts_off(T) + ((D + 3) & ~3); }
inline long long stream_words(int T, int D, long long rows) { return ring_off(T, D) + (long long)D * rows * LP_DET_COLS; }

// p[i] for i < n, else the zero vector.  The load itself is under the condition: p holds n vectors and no more (a frame of
// det_hold has hold_rows * 7 vectors, an entry rows * 7: the copies below run over the longer of the two).
__device__ __forceinline__ float4 load_or_zero(const float4* p, long long i, long long n) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < n) v = p[i];
    return v;
}

// grid (workgroups of this launch), block (1024).  det_hold / count_hold / tid / slot / rel_*: the launch's first frame.
__global__ __launch_bounds__(LB_T) void lookback_kernel(const LbTable tab, const LbDims dm, int* __restrict__ state,
                                                        const float4* __restrict__ det_hold, const int32_t* __restrict__ count_hold,
                                                        const int32_t* __restrict__ tid_in, const int32_t* __restrict__ slot_in,
                                                        float4* __restrict__ rel_det, int32_t* __restrict__ rel_count,
                                                        int32_t* __restrict__ rel_frame) {
    __shared__ int s_pos[LB_ROWS * LB_DEPTH];   // position of confirming row c in target entry k, -1: none
    __shared__ float s_geom[LB_ROWS][12];
    __shared__ float s_vel[LB_ROWS][2];
    __shared__ int s_row[LB_ROWS], s_first[LB_ROWS];
    __shared__ int s_wcnt[2], s_drop;
    const int blk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const int strm = tab.blk_stream[blk];
    const int T = dm.T, D = dm.D, rows = dm.rows;
    const long long evec = (long long)rows * LB_VEC;                   // vectors of a ring entry
    int* const sst = state + (long long)(strm < 0 ? 0 : strm) * dm.sstride;
    int* const cnts = sst + counts_off(T);
    float4* const ring = (float4*)(sst + ring_off(T, D));
    for (int j = 0; j < tab.nfr; ++j) {                                // (block-uniform control flow throughout)
        if (tab.fr_blk[j] != blk) continue;
        const float4* src = det_hold + (long long)j * dm.hold_rows * LB_VEC;
        float4* rel = rel_det + (long long)j * evec;
        int n = count_hold[j];
        n = n < 0 ? 0 : (n > dm.hold_rows ? dm.hold_rows : n);
        const long long nvec = (long long)n * LB_VEC;
        if (tab.fr_skip[j]) {                                          // released at once; no state is touched
            for (long long i = tid; i < evec; i += LB_T) rel[i] = load_or_zero(src, i, nvec);          // nvec <= hold_rows * 7
            if (tid == 0) { rel_count[j] = n; rel_frame[j] = -2; }
            continue;
        }
        const int f = sst[0], base = sst[1];
        if (tid == 0) s_drop = 0;
        // ---- A. follow the slots of the frame's rows -----------------------------------------------------------------
        const int nrow = dm.max_det < LB_ROWS ? dm.max_det : LB_ROWS;
        bool conf = false;
        int* en = nullptr;
        if (tid < nrow) {
            const int id = tid_in[(long long)j * dm.max_det + tid], t = slot_in[(long long)j * dm.max_det + tid];
            if (id >= 0 && t >= 0 && t < T) {
                en = sst + LB_HDR_WORDS + t * LB_SLOT_WORDS;
                if (en[0] != id + 1) {
                    const float* row = (const float*)src + tid * LP_DET_COLS;
                    en[0] = id + 1; en[1] = 1; en[2] = f;
                    for (int c = 0; c < 12; ++c) en[4 + c] = __float_as_int(row[c]);
                } else if (en[1] == 1) {
                    en[1] = 2;
                    conf = true;
                }
            }
        }
        unsigned long long em = 0ull;
        if (tid < LB_ROWS) {
            em = __ballot(conf);
            if (lane == 0) s_wcnt[wave] = __popcll(em);
        }
        __syncthreads();
        const int nconf = s_wcnt[0] + s_wcnt[1];
        if (nconf) {
            if (conf) {
                const int c = (wave == 1 ? s_wcnt[0] : 0) + __popcll(em & lt);
                const float* row = (const float*)src + tid * LP_DET_COLS;
                const int first = en[2];
                for (int q = 0; q < 12; ++q) s_geom[c][q] = __int_as_float(en[4 + q]);
                const float x1 = __int_as_float(en[4]), y1 = __int_as_float(en[5]), x2 = __int_as_float(en[6]), y2 = __int_as_float(en[7]);
                const float k = (float)(f - first);
                s_vel[c][0] = ((row[0] + row[2]) * 0.5f - (x1 + x2) * 0.5f) / k;
                s_vel[c][1] = ((row[1] + row[3]) * 0.5f - (y1 + y2) * 0.5f) / k;
                s_row[c] = tid;
                s_first[c] = first;
            }
            __syncthreads();
            // ---- B. the back rows: positions per target entry, then the rows ---------------------------------------------
            if (tid < D) {
                const int g = f - D + tid;
                const bool live = g >= base && g >= 0;
                const int e = live ? g % D : 0;
                int cnt = live ? cnts[e] : 0, drop = 0;
                for (int c = 0; c < nconf; ++c) {
                    const int first = s_first[c];
                    int pos = -1;
                    if (live && g >= first - dm.max_back && g != first) {
                        if (cnt < rows) pos = cnt++;
                        else ++drop;
                    }
                    s_pos[c * D + tid] = pos;
                }
                if (live) cnts[e] = cnt;
                if (drop) atomicAdd(&s_drop, drop);
            }
            __syncthreads();
            const int per = D * LB_VEC;
            for (int q = tid; q < nconf * per; q += LB_T) {
                const int c = q / per, rem = q - c * per, k = rem / LB_VEC, p = rem - k * LB_VEC;
                const int pos = s_pos[c * D + k];
                if (pos < 0) continue;
                const int g = f - D + k;
                float4 v;
                if (p < 3) {
                    const float m = (float)(g - s_first[c]);
                    const float dx = s_vel[c][0] * m, dy = s_vel[c][1] * m;
                    v = make_float4(s_geom[c][4 * p] + dx, s_geom[c][4 * p + 1] + dy, s_geom[c][4 * p + 2] + dx, s_geom[c][4 * p + 3] + dy);
                } else {
                    v = src[(long long)s_row[c] * LB_VEC + p];
                }
                ring[(long long)(g % D) * evec + (long long)pos * LB_VEC + p] = v;
            }
            __syncthreads();
        }
        // ---- C + D. release frame f - D out of the entry f % D, store the frame's rows into it ------------------------------
        const int e = f % D;
        const bool releasing = f - D >= base;
        const int relcnt = releasing ? cnts[e] : 0;
        const long long relvec = (long long)relcnt * LB_VEC;
        float4* ent = ring + (long long)e * evec;
        for (long long i = tid; i < evec; i += LB_T) {
            rel[i] = load_or_zero(ent, i, relvec);                          // relvec <= rows * 7 = evec
            ent[i] = load_or_zero(src, i, nvec);                            // nvec <= hold_rows * 7
        }
        __syncthreads();                                               // every thread has read cnts[e], f and base
        if (tid == 0) {
            rel_count[j] = relcnt;
            rel_frame[j] = releasing ? f - D : -1;
            cnts[e] = n;
            sst[0] = f + 1;
            if (releasing) sst[1] = f - D + 1;
            sst[2] += s_drop;
        }
        __syncthreads();                                               // the next frame reads the state
    }
}

// grid (streams of this launch), block (1024): the tails, after the call's last frame
__global__ __launch_bounds__(LB_T) void lookback_tail_kernel(const LbTail tab, const LbDims dm, int* __restrict__ state,
                                                             float4* __restrict__ tail_det, int32_t* __restrict__ tail_count,
                                                             int32_t* __restrict__ tail_frame) {
    const int tid = threadIdx.x, strm = tab.s0 + blockIdx.x;
    const bool flush = tab.flush[blockIdx.x] != 0;
    const int T = dm.T, D = dm.D;
    const long long evec = (long long)dm.rows * LB_VEC;
    int* const sst = state + (long long)strm * dm.sstride;
    const int* cnts = sst + counts_off(T);
    const float4* ring = (const float4*)(sst + ring_off(T, D));
    const int f = sst[0], base = sst[1];
    for (int k = 0; k < D; ++k) {
        const int g = base + k;
        const bool has = flush && g < f;
        const int e = has ? g % D : 0;
        const int cnt = has ? cnts[e] : 0;
        const long long cvec = (long long)cnt * LB_VEC;
        const float4* ent = ring + (long long)e * evec;
        float4* dst = tail_det + ((long long)strm * D + k) * evec;
        for (long long i = tid; i < evec; i += LB_T) dst[i] = load_or_zero(ent, i, cvec);     // cvec <= evec
        if (tid == 0) {
            tail_count[(long long)strm * D + k] = cnt;
            tail_frame[(long long)strm * D + k] = has ? g : -1;
        }
    }
    __syncthreads();                                                   // every thread has read base
    if (tid == 0 && flush) sst[1] = f;
}

bool lookback_dims_ok(int n_streams, int max_tracks, int depth, long long rows) {
    return stream_dims_fault(n_streams, max_tracks).empty() && depth >= 1 && depth <= LB_DEPTH && rows >= 1 && rows * LP_DET_COLS < 0x80000000ll;
}

}  // namespace

}  // namespace lp

using namespace lp;

extern "C" size_t lp_lookback_state_bytes(int n_streams, int max_tracks, int depth, int rows) {
    if (!lookback_dims_ok(n_streams, max_tracks, depth, rows)) return 0;
    return (size_t)n_streams * (size_t)stream_words(max_tracks, depth, rows) * 4;
}

extern "C" int lp_lookback_update(void* state, int n_streams, int max_tracks, int depth, int max_back, int back_cap, const float* det_hold,
                                  const int32_t* count_hold, const int32_t* tid, const int32_t* slot, int B, int max_det, int hold_rows,
                                  const int* stream_of, const unsigned char* flush, float* rel_det, int32_t* rel_count, int32_t* rel_frame,
                                  float* tail_det, int32_t* tail_count, int32_t* tail_frame, void* stream) {
    const std::string fn = "lp_lookback_update: ";
    if (depth < 1 || depth > LB_DEPTH || max_back < 0 || back_cap < 0)
        return fail(LP_ERR_ARG, fn + "need depth in 1.." + std::to_string(LB_DEPTH) + ", max_back >= 0 and back_cap >= 0");
    std::string why = stream_dims_fault(n_streams, max_tracks);
    if (!why.empty()) return fail(LP_ERR_ARG, fn + why);
    const long long rows = (long long)hold_rows + back_cap;
    if (B < 0 || max_det < 1 || hold_rows < max_det || rows * LP_DET_COLS >= 0x80000000ll)
        return fail(LP_ERR_ARG, fn + "need B >= 0, max_det >= 1, hold_rows >= max_det and (hold_rows + back_cap) * 28 < 2^31");
    if (!state || !tail_det || !tail_count || !tail_frame ||
        (B > 0 && (!det_hold || !count_hold || !tid || !slot || !stream_of || !rel_det || !rel_count || !rel_frame)))
        return fail(LP_ERR_ARG, fn + "null pointer");
    if ((((uintptr_t)state | (uintptr_t)det_hold | (uintptr_t)rel_det | (uintptr_t)tail_det) & 15) != 0)
        return fail(LP_ERR_ARG, fn + "state, det_hold, rel_det and tail_det must be 16-byte aligned");
    why = stream_of_fault(stream_of, B, n_streams);
    if (!why.empty()) return fail(LP_ERR_ARG, fn + why);
    {   // no output may overlap the state, an input or another output
        const size_t row_bytes = LP_DET_COLS * sizeof(float), nb = (size_t)B, nt = (size_t)n_streams * depth;
        const Region reg[] = {{state, (size_t)n_streams * (size_t)stream_words(max_tracks, depth, rows) * 4, false},
                              {det_hold, nb * hold_rows * row_bytes, false}, {count_hold, nb * 4, false},
                              {tid, nb * max_det * 4, false}, {slot, nb * max_det * 4, false},
                              {rel_det, nb * (size_t)rows * row_bytes, true}, {rel_count, nb * 4, true}, {rel_frame, nb * 4, true},
                              {tail_det, nt * (size_t)rows * row_bytes, true}, {tail_count, nt * 4, true}, {tail_frame, nt * 4, true}};
        if (regions_clash(reg, (int)(sizeof(reg) / sizeof(reg[0]))))
            return fail(LP_ERR_ARG, fn + "the outputs (rel_*, tail_*) may overlap neither the state, an input nor each other");
    }

    hipStream_t st = (hipStream_t)stream;
    LbDims dm;
    dm.T = max_tracks; dm.D = depth; dm.max_back = max_back; dm.max_det = max_det; dm.hold_rows = hold_rows; dm.rows = (int)rows;
    dm.sstride = stream_words(max_tracks, depth, rows);
    const size_t evec = (size_t)rows * LB_VEC;
    std::vector<int> blk_of((size_t)n_streams, -1);
    for (int b0 = 0; b0 < B; b0 += LB_FRAMES) {
        LbTable tab = {};
        tab.nfr = B - b0 < LB_FRAMES ? B - b0 : LB_FRAMES;
        const StreamPlan pl = plan_streams(stream_of + b0, tab.nfr, blk_of, UNTRACKED_DEAL);
        memcpy(tab.blk_stream, pl.blk_stream, sizeof(tab.blk_stream));
        memcpy(tab.fr_blk, pl.fr_blk, sizeof(tab.fr_blk));
        memcpy(tab.fr_skip, pl.fr_skip, sizeof(tab.fr_skip));
        hipLaunchKernelGGL(lookback_kernel, dim3((unsigned)pl.nblk), dim3(LB_T), 0, st, tab, dm, (int*)state,
                           (const float4*)(det_hold + (size_t)b0 * hold_rows * LP_DET_COLS), count_hold + b0, tid + (size_t)b0 * max_det,
                           slot + (size_t)b0 * max_det, (float4*)rel_det + (size_t)b0 * evec, rel_count + b0, rel_frame + b0);
        LP_HIP_CHECK(hipGetLastError());
    }
    for (int s0 = 0; s0 < n_streams; s0 += LB_FRAMES) {
        LbTail tab = {};
        tab.s0 = s0;
        tab.n = n_streams - s0 < LB_FRAMES ? n_streams - s0 : LB_FRAMES;
        for (int k = 0; k < tab.n; ++k) tab.flush[k] = (flush && flush[s0 + k]) ? 1 : 0;
        hipLaunchKernelGGL(lookback_tail_kernel, dim3((unsigned)tab.n), dim3(LB_T), 0, st, tab, dm, (int*)state, (float4*)tail_det, tail_count,
                           tail_frame);
        LP_HIP_CHECK(hipGetLastError());
    }
    return LP_OK;
}
