// One denoised picture per plate track: lp_stack_update (include/lp_hip.h).  Behind lp_track_update_slots, lp_plate_crops_batch and
// lp_crop_sharpness a device-resident stack keeps, per tracker slot, the sum of the rectified crops its track has shown, each
// aligned to the running sum by an integer shift, and hands out the rounded mean next to the track's record when the track ends.
// The reference has nothing here; the written-down specification is yolov6/utils/stack.py (StackNp), which these kernels match
// bit for bit (tests/test_stack_gpu.py).  The sums are integer, so their order does not matter.
//
// stack_kernel: grid (streams of the launch) x (slots), 1024 threads; the frame table travels in the kernel arguments as in
// lp_shots.hip.  A workgroup owns ONE entry for the whole launch: it keeps the entry's four header words in registers, walks the
// launch's frames of its stream in order, finds the rows of its slot by a ballot over the slot column (ascending r, normally one
// row or none) and does the bookkeeping itself, a retire followed by a fresh track in the same slot included.  A workgroup
// whose slot shows up in no frame reads the slot column and leaves.  The frame number of frame j is the stream's counter at
// the start of the launch plus the frame's ordinal within its stream (in the table), so no workgroup waits for another;
// stack_advance_kernel (one thread per stream of the launch) moves the counters behind it.
//   align: the luma of the new crop (16 bits, with `search` halo rows) and of the running sum (32 bits) are staged in 48 KiB of
//   LDS in bands of whole rows.  Every thread keeps one unsigned 64-bit cost per candidate of a pass in registers across all
//   bands (each term is below 2^24 and goes straight into 64 bits, so no 32-bit partial needs a bound), then the lanes of a wave
//   add theirs by shuffles and the 16 wave sums meet in LDS.  A pass takes some values of dy with every dx: search 1 and 2 (9
//   and 25 candidates) take one pass over the bands, search 3 three and search 4 five.
//   accumulate: 16-byte vectors of the entry's uint16 sum (eight values), the crop's bytes gathered with the shift's clamps.
//   retire: 16 means per thread, one exact unsigned division each, stored as a 16-byte vector where the record's crop allows.
// stack_final_kernel, grid (n_streams) x (slots), does rule 6 after the call's last frame.
// State of a stream: 16 bytes (the frame counter, 12 unused), then per slot an entry of 16 bytes (id + 1, n, first_frame,
// last_frame) + the uint16 sum rounded up to 16 bytes.  All zero = empty.
#include "lp_internal.h"
#include "lp_streams.h"
#include <cstring>

namespace lp {

namespace {

constexpr int ST_T = 1024;                      // threads of every workgroup here
constexpr int ST_WAVES = ST_T / 64;
constexpr int ST_HDR_BYTES = 16;
constexpr int ST_ENTRY_HDR = 16;
constexpr int ST_ROWS = LP_TRACK_MAX_DETS;      // rows of a frame that take part
constexpr int ST_FRAMES = LP_FRAMES_PER_LAUNCH;
constexpr int ST_MAX_SIDE = 1024;
constexpr int ST_MAX_SEARCH = 4;
constexpr int ST_MAX_CAND = (2 * ST_MAX_SEARCH + 1) * (2 * ST_MAX_SEARCH + 1);
constexpr int ST_PASS_ROWS(int R) { return R == 2 ? 5 : (R == 4 ? 2 : 3); }   // values of dy per pass of the search
constexpr int ST_LDS_BYTES = 49152;             // the staged luma of a band
static_assert(ST_ROWS == 128, "two waves ballot the slot column");
// a band of one row of the widest crop with the widest halo fits
static_assert((2 * ST_MAX_SEARCH + 1) * ST_MAX_SIDE * 2 + ST_MAX_SIDE * 4 + 4 <= ST_LDS_BYTES, "LDS of one band row");

struct StTable {                                // 520 bytes of kernel arguments
    int nfr, nblk;
    int blk_stream[ST_FRAMES];                  // stream of workgroup column k
    short fr_blk[ST_FRAMES];                    // workgroup column that takes frame j of the launch, -1: skipped
    unsigned char fr_ord[ST_FRAMES];            // tracked frames of the same stream before frame j in this launch
    unsigned char blk_nfr[ST_FRAMES];           // frames of workgroup column k in this launch
};
struct StCand {                                 // candidate k of the search; entries past n are (0, 0)
    int n;
    signed char dy[ST_MAX_CAND], dx[ST_MAX_CAND];
};
struct StArgs {
    const float* det; const int32_t* count; const int32_t* tid; const int32_t* slot;      // the launch's first frame
    const unsigned char* crops; const int32_t* status; const unsigned long long* sharp;  // the launch's first frame
    const int32_t* ended_i; const int32_t* ended_count;
    unsigned char* stack_crops; int32_t* stack_i;
    long long sstride, estride;
    unsigned long long min_sharp;
    int max_det, max_crops, max_ended, crop_h, crop_w, search, max_frames, band_rows;
    float min_score_f, min_width_f;
};

__device__ __forceinline__ unsigned luma_of(unsigned b, unsigned g, unsigned r) { return 29u * b + 150u * g + 77u * r; }

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {      // lane 0 has the sum
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned lo = __shfl_down((unsigned)(v & 0xffffffffull), d), hi = __shfl_down((unsigned)(v >> 32), d);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

// first e < n_rec with ended_i[e][0] == id, or -1
__device__ __forceinline__ int find_record(const int32_t* rec, int n_rec, int id) {
    for (int e = 0; e < n_rec; ++e)
        if (rec[e * 12] == id) return e;
    return -1;
}

// Rule 4, the search: the candidate of the smallest (cost, k) for `crop` against the sum `acc` of n >= 1 crops.  All threads
// call it and all get the answer; needs crop_h > 2 R and crop_w > 2 R.  R is a template argument so that a candidate's column
// shift is an immediate offset of its LDS read and the per-thread costs are addressed statically: a pass takes ST_PASS_ROWS(R)
// values of dy with all 2 R + 1 values of dx (9, 25, 21 and 18 costs per thread for R = 1..4: 1, 1, 3 and 5 passes over the bands).
// s_cost is indexed by (dy + R) * (2 R + 1) + (dx + R).
template <int R>
__device__ __forceinline__ int align_search(const unsigned char* __restrict__ crop, const unsigned short* acc, const StArgs& a,
                                            const StCand& cand, unsigned n, unsigned char* s_raw, unsigned long long (*s_cost)[ST_WAVES]) {
    constexpr int D = 2 * R + 1, DYS = ST_PASS_ROWS(R);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Hc = a.crop_h, Wc = a.crop_w, iw = Wc - 2 * R;
    unsigned short* const s_yc = (unsigned short*)s_raw;                              // rows i0-R .. i1+R-1 of the crop
    unsigned* const s_ya = (unsigned*)(s_raw + ((((a.band_rows + 2 * R) * Wc * 2) + 3) & ~3));   // rows i0 .. i1-1 of the sum
#pragma unroll
    for (int dy0 = -R; dy0 <= R; dy0 += DYS) {
        unsigned long long cost[DYS * D];
#pragma unroll
        for (int c = 0; c < DYS * D; ++c) cost[c] = 0ull;
        for (int i0 = R; i0 < Hc - R; i0 += a.band_rows) {
            const int i1 = i0 + a.band_rows < Hc - R ? i0 + a.band_rows : Hc - R;
            const unsigned char* src = crop + (long long)(i0 - R) * Wc * 3;
            const int npix = (i1 - i0 + 2 * R) * Wc;
            for (int p = tid; p < npix; p += ST_T) s_yc[p] = (unsigned short)luma_of(src[3 * p], src[3 * p + 1], src[3 * p + 2]);
            const unsigned short* as = acc + (long long)i0 * Wc * 3;
            const int napix = (i1 - i0) * Wc;
            for (int p = tid; p < napix; p += ST_T) s_ya[p] = luma_of(as[3 * p], as[3 * p + 1], as[3 * p + 2]);
            __syncthreads();
            const int nin = (i1 - i0) * iw;
            for (int p = tid; p < nin; p += ST_T) {
                const int i = p / iw, j = p - i * iw + R;
                const unsigned av = s_ya[i * Wc + j];
#pragma unroll
                for (int d = 0; d < DYS; ++d) {
                    if (dy0 + d > R) continue;                                        // (the last pass may be short)
                    const unsigned short* yr = s_yc + (i + R + dy0 + d) * Wc + j;
#pragma unroll
                    for (int x = -R; x <= R; ++x) {
                        const unsigned t = n * (unsigned)yr[x];                       // n * y <= 254 * 65280 < 2^24
                        cost[d * D + x + R] += t > av ? t - av : av - t;
                    }
                }
            }
            __syncthreads();                                                          // the next band overwrites the rows
        }
#pragma unroll
        for (int d = 0; d < DYS; ++d) {
            if (dy0 + d > R) continue;
#pragma unroll
            for (int x = 0; x < D; ++x) {
                const unsigned long long sum = wave_sum64(cost[d * D + x]);
                if (lane == 0) s_cost[(dy0 + d + R) * D + x][wave] = sum;
            }
        }
    }
    __syncthreads();
    if (tid < D * D) {
        unsigned long long t = 0;
        for (int w = 0; w < ST_WAVES; ++w) t += s_cost[tid][w];
        s_cost[tid][0] = t;
    }
    __syncthreads();
    int best = 0;
    unsigned long long best_cost = s_cost[R * D + R][0];                              // k = 0 is (0, 0)
    for (int k = 1; k < cand.n; ++k) {
        const unsigned long long c = s_cost[((int)cand.dy[k] + R) * D + (int)cand.dx[k] + R][0];
        if (c < best_cost) { best_cost = c; best = k; }                               // strict: the lower k keeps a tie
    }
    __syncthreads();                                                                  // the next search reuses s_cost
    return best;
}

// Rule 4, the sum: acc[i][j][c] (+)= crop[clamp(i+dy)][clamp(j+dx)][c]; `first`: the entry starts from zero.  Eight values = one
// 16-byte vector of the sum per thread and step; the bytes behind the last value of the entry keep what they hold.
__device__ __forceinline__ void accumulate(const unsigned char* __restrict__ crop, unsigned short* acc, int Hc, int Wc, int dy,
                                           int dx, bool first) {
    const int ne = Hc * Wc * 3, row = Wc * 3, ngrp = (ne + 7) >> 3;
    for (int grp = threadIdx.x; grp < ngrp; grp += ST_T) {
        const int e0 = grp << 3;
        uint4 v = ((const uint4*)acc)[grp];
        unsigned w[4] = {v.x, v.y, v.z, v.w};
        int i = e0 / row;
        const int rem = e0 - i * row;
        int j = rem / 3, c = rem - 3 * j;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (e0 + q < ne) {
                int si = i + dy, sj = j + dx;
                si = si < 0 ? 0 : (si > Hc - 1 ? Hc - 1 : si);
                sj = sj < 0 ? 0 : (sj > Wc - 1 ? Wc - 1 : sj);
                const unsigned px = crop[((long long)si * Wc + sj) * 3 + c];
                const int sh = 16 * (q & 1);
                const unsigned old = (w[q >> 1] >> sh) & 0xffffu;
                const unsigned nv = first ? px : old + px;                            // <= 255 * 255
                w[q >> 1] = (w[q >> 1] & ~(0xffffu << sh)) | (nv << sh);
            }
            if (++c == 3) {
                c = 0;
                if (++j == Wc) { j = 0; ++i; }
            }
        }
        ((uint4*)acc)[grp] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// Rule 5, the picture: dst[o] = (acc[o] + (n >> 1)) / n for the nbytes values of an entry.  16 values per thread and step, stored
// as one 16-byte vector from dst's first 16-byte boundary on; the bytes before it and behind the last vector one by one.
__device__ __forceinline__ void retire_mean(const unsigned short* acc, unsigned n, unsigned char* __restrict__ dst, int nbytes) {
    const int tid = threadIdx.x;
    int head = (int)((16 - ((uintptr_t)dst & 15)) & 15);
    head = head < nbytes ? head : nbytes;
    const int nvec = (nbytes - head) >> 4, tail = nbytes - head - (nvec << 4);
    const unsigned half = n >> 1;
    for (int v = tid; v < nvec; v += ST_T) {
        const int o = head + (v << 4);
        unsigned h[8];                                                                // 16 sums, two per word
        if ((head & 7) == 0) {                                                        // acc + o is 16-byte aligned
            const uint4 lo = *(const uint4*)(acc + o), hi = *(const uint4*)(acc + o + 8);
            h[0] = lo.x; h[1] = lo.y; h[2] = lo.z; h[3] = lo.w; h[4] = hi.x; h[5] = hi.y; h[6] = hi.z; h[7] = hi.w;
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) h[q] = (unsigned)acc[o + 2 * q] | ((unsigned)acc[o + 2 * q + 1] << 16);
        }
        unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const unsigned s = (h[q >> 1] >> (16 * (q & 1))) & 0xffffu;
            w[q >> 2] |= ((s + half) / n) << (8 * (q & 3));                           // <= 255
        }
        *(uint4*)(dst + o) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    if (tid < head + tail) {
        const int o = tid < head ? tid : head + (nvec << 4) + (tid - head);
        dst[o] = (unsigned char)(((unsigned)acc[o] + half) / n);
    }
}

// rule 5 for the entry (id + 1, n, first, last) with the sum `acc` (all threads): the record's picture and its stack_i line
__device__ __forceinline__ void retire_entry(int idp1, int n, int first, int last, const unsigned short* acc, int strm, const int32_t* rec,
                                             int n_rec, const StArgs& a) {
    const int e = find_record(rec, n_rec, idp1 - 1);
    if (e >= 0 && n >= 1) {
        const long long k = (long long)strm * a.max_ended + e;
        const int crop_bytes = a.crop_h * a.crop_w * 3;
        retire_mean(acc, (unsigned)n, a.stack_crops + k * crop_bytes, crop_bytes);
        if (threadIdx.x == 0) {
            a.stack_i[k * 4] = n; a.stack_i[k * 4 + 1] = first; a.stack_i[k * 4 + 2] = last; a.stack_i[k * 4 + 3] = 1;
        }
    }
}

__global__ void stack_clear_kernel(int32_t* stack_i, long long n_words) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_words) stack_i[i] = 0;
}

// grid (workgroup columns of this launch, slots), block (1024); control flow is block-uniform throughout
__global__ __launch_bounds__(ST_T) void stack_kernel(const StTable tab, const StCand cand, const StArgs a, unsigned char* __restrict__ state) {
    __shared__ __attribute__((aligned(16))) unsigned char s_raw[ST_LDS_BYTES];
    __shared__ unsigned long long s_cost[ST_MAX_CAND][ST_WAVES];
    __shared__ unsigned long long s_mask[2][2];                        // the rows of this slot in a frame; two frames in flight
    const int blk = blockIdx.x, g = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int strm = tab.blk_stream[blk];
    unsigned char* const sst = state + (long long)strm * a.sstride;
    int* const en = (int*)(sst + ST_HDR_BYTES + (long long)g * a.estride);
    unsigned short* const acc = (unsigned short*)(en + ST_ENTRY_HDR / 4);
    const int frame0 = *(const int*)sst;                               // (stack_advance_kernel moves it behind this launch)
    const int32_t* rec = a.ended_i + (long long)strm * a.max_ended * 12;
    int n_rec = a.ended_count[strm];
    n_rec = n_rec < 0 ? 0 : (n_rec < a.max_ended ? n_rec : a.max_ended);
    int idp1 = en[0], n = en[1], first = en[2], last = en[3];          // the entry's header: this workgroup alone owns it
    bool dirty = false;
    const int Hc = a.crop_h, Wc = a.crop_w, R = a.search;
    const long long crop_bytes = (long long)Hc * Wc * 3;
    int par = 0;
    for (int j = 0; j < tab.nfr; ++j) {
        if (tab.fr_blk[j] != blk) continue;
        int nrows = a.count[j];
        nrows = nrows < 0 ? 0 : (nrows > a.max_det ? a.max_det : nrows);
        nrows = nrows < a.max_crops ? nrows : a.max_crops;
        nrows = nrows < ST_ROWS ? nrows : ST_ROWS;
        if (tid < ST_ROWS) {
            const bool hit = tid < nrows && a.tid[(long long)j * a.max_det + tid] >= 0 && a.slot[(long long)j * a.max_det + tid] == g;
            const unsigned long long m = __ballot(hit);
            if (lane == 0) s_mask[par][wave] = m;
        }
        __syncthreads();
        const unsigned long long m01[2] = {s_mask[par][0], s_mask[par][1]};
        par ^= 1;
        const int frame = frame0 + tab.fr_ord[j];
        for (int w = 0; w < 2; ++w) {
            for (unsigned long long m = m01[w]; m != 0ull; m &= m - 1ull) {
                const int r = w * 64 + __ffsll((long long)m) - 1;
                const int id = a.tid[(long long)j * a.max_det + r];
                if (idp1 != id + 1) {
                    if (idp1 != 0) {
                        retire_entry(idp1, n, first, last, acc, strm, rec, n_rec, a);
                        __syncthreads();                               // the newcomer's first crop overwrites the sum
                    }
                    idp1 = id + 1;
                    n = 0;
                    dirty = true;
                }
                const float* row = a.det + ((long long)j * a.max_det + r) * LP_DET_COLS;
                float sc = row[12] + row[13];
                sc = sc + row[14]; sc = sc + row[15]; sc = sc + row[16]; sc = sc + row[17]; sc = sc + row[18]; sc = sc + row[19];
                sc = sc / 8.0f;
                const float width = row[2] - row[0];
                // min_*_f = smallest fp32 >= the double threshold  <=>  (double)x >= threshold; false for NaN
                if (a.status[(long long)j * a.max_crops + r] != 1 || !(sc >= a.min_score_f) || !(width >= a.min_width_f) ||
                    a.sharp[(long long)j * a.max_crops + r] < a.min_sharp || n >= a.max_frames)
                    continue;
                const unsigned char* crop = a.crops + ((long long)j * a.max_crops + r) * crop_bytes;
                int dy = 0, dx = 0;
                if (n > 0 && R > 0 && Hc > 2 * R && Wc > 2 * R) {
                    const int k = R == 1 ? align_search<1>(crop, acc, a, cand, (unsigned)n, s_raw, s_cost)
                                  : R == 2 ? align_search<2>(crop, acc, a, cand, (unsigned)n, s_raw, s_cost)
                                  : R == 3 ? align_search<3>(crop, acc, a, cand, (unsigned)n, s_raw, s_cost)
                                           : align_search<4>(crop, acc, a, cand, (unsigned)n, s_raw, s_cost);
                    dy = cand.dy[k];
                    dx = cand.dx[k];
                }
                accumulate(crop, acc, Hc, Wc, dy, dx, n == 0);
                __syncthreads();                                       // the next search or a retire reads the sum
                if (n == 0) first = frame;
                last = frame;
                ++n;
                dirty = true;
            }
        }
    }
    if (dirty && tid == 0) { en[0] = idp1; en[1] = n; en[2] = first; en[3] = last; }
}

// behind stack_kernel: grid (1), block (64)
__global__ void stack_advance_kernel(const StTable tab, unsigned char* __restrict__ state, long long sstride) {
    const int k = threadIdx.x;
    if (k < tab.nblk) *(int*)(state + (long long)tab.blk_stream[k] * sstride) += tab.blk_nfr[k];
}

// rule 6, after the call's last frame: grid (n_streams, slots), block (1024)
__global__ __launch_bounds__(ST_T) void stack_final_kernel(const StArgs a, unsigned char* __restrict__ state) {
    const int strm = blockIdx.x, g = blockIdx.y;
    int n_rec = a.ended_count[strm];
    n_rec = n_rec < 0 ? 0 : (n_rec < a.max_ended ? n_rec : a.max_ended);
    if (n_rec == 0) return;                                            // (block-uniform, as every return here)
    int* const en = (int*)(state + (long long)strm * a.sstride + ST_HDR_BYTES + (long long)g * a.estride);
    const int idp1 = en[0], n = en[1], first = en[2], last = en[3];
    const int32_t* rec = a.ended_i + (long long)strm * a.max_ended * 12;
    if (idp1 == 0 || find_record(rec, n_rec, idp1 - 1) < 0) return;
    retire_entry(idp1, n, first, last, (const unsigned short*)(en + ST_ENTRY_HDR / 4), strm, rec, n_rec, a);
    __syncthreads();                                                   // every thread has read the header
    if (threadIdx.x == 0) { en[0] = 0; en[1] = 0; }
}

bool stack_dims_ok(int crop_h, int crop_w) { return crop_h >= 1 && crop_w >= 1 && crop_h <= ST_MAX_SIDE && crop_w <= ST_MAX_SIDE; }
size_t stack_entry_bytes(int crop_h, int crop_w) { return (size_t)ST_ENTRY_HDR + (((size_t)crop_h * crop_w * 6 + 15) & ~(size_t)15); }
size_t stack_stream_bytes(int max_tracks, int crop_h, int crop_w) { return ST_HDR_BYTES + (size_t)max_tracks * stack_entry_bytes(crop_h, crop_w); }

// candidate k of [-R, R]^2 in the order of (dy^2 + dx^2, dy, dx)
StCand stack_candidates(int R) {
    StCand c = {};
    for (int d2 = 0; d2 <= 2 * R * R; ++d2)
        for (int dy = -R; dy <= R; ++dy)
            for (int dx = -R; dx <= R; ++dx)
                if (dy * dy + dx * dx == d2) {
                    c.dy[c.n] = (signed char)dy;
                    c.dx[c.n] = (signed char)dx;
                    ++c.n;
                }
    return c;
}

}  // namespace

}  // namespace lp

using namespace lp;

extern "C" size_t lp_stack_state_bytes(int n_streams, int max_tracks, int crop_h, int crop_w) {
    if (!stream_dims_fault(n_streams, max_tracks).empty() || !stack_dims_ok(crop_h, crop_w)) return 0;
    return (size_t)n_streams * stack_stream_bytes(max_tracks, crop_h, crop_w);
}

extern "C" int lp_stack_update(void* state, int n_streams, int max_tracks, int crop_h, int crop_w, const float* det, const int32_t* count, int B,
                               int max_det, const int32_t* tid, const int32_t* slot, const unsigned char* crops, const int32_t* status,
                               const unsigned long long* sharp, int max_crops, const int* stream_of, const int32_t* ended_i,
                               const int32_t* ended_count, int max_ended, const lp_stack_params* p, unsigned char* stack_crops,
                               int32_t* stack_i, void* stream) {
    const std::string fn = "lp_stack_update: ";
    std::string why = stream_dims_fault(n_streams, max_tracks);
    if (!why.empty()) return fail(LP_ERR_ARG, fn + why);
    if (!stack_dims_ok(crop_h, crop_w)) return fail(LP_ERR_ARG, fn + "need a crop size of 1..1024 on each side");
    if (B < 0 || max_det < 1 || max_det > 0x7fffffff / LP_DET_COLS || max_ended < 0 || max_crops < 0)
        return fail(LP_ERR_ARG, fn + "need B >= 0, max_det >= 1, max_ended >= 0 and max_crops >= 0");
    if (!p) return fail(LP_ERR_ARG, fn + "null pointer (params)");
    if (p->search < 0 || p->search > ST_MAX_SEARCH) return fail(LP_ERR_ARG, fn + "search must be in 0..4");
    if (p->max_frames < 1 || p->max_frames > 255) return fail(LP_ERR_ARG, fn + "max_frames must be in 1..255 (255 * 255 fits the 16-bit sum)");
    if (!(std::fabs(p->min_score) <= 3.0e38)) return fail(LP_ERR_ARG, fn + "min_score must be finite (|min_score| <= 3e38)");
    if (!(std::fabs(p->min_width) <= 3.0e38)) return fail(LP_ERR_ARG, fn + "min_width must be finite (|min_width| <= 3e38)");
    if (!state || !ended_count || (max_ended > 0 && (!ended_i || !stack_crops || !stack_i)) ||
        (B > 0 && (!det || !count || !tid || !slot || !stream_of)) || (B > 0 && max_crops > 0 && (!crops || !status || !sharp)))
        return fail(LP_ERR_ARG, fn + "null pointer");
    if (((uintptr_t)state & 15) != 0) return fail(LP_ERR_ARG, fn + "state must be 16-byte aligned");
    if (((uintptr_t)sharp & 7) != 0) return fail(LP_ERR_ARG, fn + "sharp must be 8-byte aligned");
    why = stream_of_fault(stream_of, B, n_streams);
    if (!why.empty()) return fail(LP_ERR_ARG, fn + why);
    const size_t crop_bytes = (size_t)crop_h * crop_w * 3;
    {
        const size_t nb = (size_t)B, nr = (size_t)n_streams * max_ended, nc = nb * max_crops;
        const Region reg[] = {{state, (size_t)n_streams * stack_stream_bytes(max_tracks, crop_h, crop_w), true},
                              {stack_crops, nr * crop_bytes, true}, {stack_i, nr * 16, true},
                              {det, nb * max_det * LP_DET_COLS * 4, false}, {count, nb * 4, false},
                              {tid, nb * max_det * 4, false}, {slot, nb * max_det * 4, false},
                              {crops, nc * crop_bytes, false}, {status, nc * 4, false}, {sharp, nc * 8, false},
                              {ended_i, nr * 48, false}, {ended_count, (size_t)n_streams * 4, false}};
        if (regions_clash(reg, (int)(sizeof(reg) / sizeof(reg[0]))))
            return fail(LP_ERR_ARG, fn + "the state, stack_crops and stack_i may overlap neither an input nor each other");
    }

    hipStream_t st = (hipStream_t)stream;
    StArgs a = {};
    a.ended_i = ended_i; a.ended_count = ended_count; a.stack_crops = stack_crops; a.stack_i = stack_i;
    a.sstride = (long long)stack_stream_bytes(max_tracks, crop_h, crop_w);
    a.estride = (long long)stack_entry_bytes(crop_h, crop_w);
    a.min_sharp = p->min_sharp;
    a.max_det = max_det; a.max_crops = max_crops; a.max_ended = max_ended; a.crop_h = crop_h; a.crop_w = crop_w;
    a.search = p->search; a.max_frames = p->max_frames;
    a.min_score_f = f32_not_below(p->min_score);
    a.min_width_f = f32_not_below(p->min_width);
    // interior rows per band: (band_rows + 2 R) rows of 16-bit luma + band_rows rows of 32-bit luma in ST_LDS_BYTES, at least one
    a.band_rows = (ST_LDS_BYTES - 4 - 2 * p->search * crop_w * 2) / (6 * crop_w);
    if (a.band_rows > crop_h) a.band_rows = crop_h;
    const StCand cand = stack_candidates(p->search);
    const long long n_words = (long long)n_streams * max_ended * 4;
    if (n_words > 0) {
        hipLaunchKernelGGL(stack_clear_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, st, stack_i, n_words);
        LP_HIP_CHECK(hipGetLastError());
    }
    std::vector<int> blk_of((size_t)n_streams, -1);
    for (int b0 = 0; b0 < B; b0 += ST_FRAMES) {
        StTable tab = {};
        tab.nfr = B - b0 < ST_FRAMES ? B - b0 : ST_FRAMES;
        const StreamPlan pl = plan_streams(stream_of + b0, tab.nfr, blk_of, UNTRACKED_LEAVE_OUT);
        if (pl.nblk == 0) continue;
        tab.nblk = pl.nblk;
        memcpy(tab.blk_stream, pl.blk_stream, sizeof(tab.blk_stream));
        memcpy(tab.fr_blk, pl.fr_blk, sizeof(tab.fr_blk));
        for (int j = 0; j < tab.nfr; ++j)
            if (pl.fr_blk[j] >= 0) tab.fr_ord[j] = tab.blk_nfr[pl.fr_blk[j]]++;
        a.det = det + (size_t)b0 * max_det * LP_DET_COLS;
        a.count = count + b0;
        a.tid = tid + (size_t)b0 * max_det;
        a.slot = slot + (size_t)b0 * max_det;
        a.crops = crops ? crops + (size_t)b0 * max_crops * crop_bytes : nullptr;
        a.status = status ? status + (size_t)b0 * max_crops : nullptr;
        a.sharp = sharp ? sharp + (size_t)b0 * max_crops : nullptr;
        hipLaunchKernelGGL(stack_kernel, dim3((unsigned)pl.nblk, (unsigned)max_tracks), dim3(ST_T), 0, st, tab, cand, a, (unsigned char*)state);
        LP_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(stack_advance_kernel, dim3(1), dim3(64), 0, st, tab, (unsigned char*)state, a.sstride);
        LP_HIP_CHECK(hipGetLastError());
    }
    if (max_ended > 0) {
        hipLaunchKernelGGL(stack_final_kernel, dim3((unsigned)n_streams, (unsigned)max_tracks), dim3(ST_T), 0, st, a, (unsigned char*)state);
        LP_HIP_CHECK(hipGetLastError());
    }
    return LP_OK;
}
