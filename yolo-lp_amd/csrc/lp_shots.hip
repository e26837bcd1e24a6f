// The best shot of every plate track: lp_crop_sharpness and lp_best_shot_update (include/lp_hip.h).  Behind lp_track_update_slots
// and lp_plate_crops_batch a small device-resident gallery keeps, per tracker slot, the sharpest rectified crop its track has
// shown so far, and hands it out next to the track's record when the track ends.  The reference has nothing here; the written-down
// specification is yolov6/utils/best_shot.py (crop_sharpness_np, BestShotNp), which these kernels match bit for bit
// (tests/test_best_shot_gpu.py).  All arithmetic is integer, so the order of the sums does not matter.
//
// crop_sharpness_kernel: one workgroup of 1024 threads per crop slot.  The crop is taken in bands of whole rows: the band's
// grey values (one byte each) are staged in LDS with one halo row above and below, then every thread sums L * L over its
// interior pixels in 32 bits (at most 1024 pixels of a 1024 x 1024 crop per thread, each below 2^20), the lanes of a wave add
// their sums in 64 bits by shuffles, and the 16 wave sums meet in LDS.  No global atomics.
//
// best_shot_kernel: one workgroup of 1024 threads per stream of a launch, the frame table in the kernel arguments as in
// lp_track.hip.  Per frame one thread per row decides (retire the slot's former occupant, take the shot), writes the small
// things itself (entry header, det row, shot_i / shot_q / shot_det) and appends the crop copies to two job lists in LDS; then
// all waves run the retire copies, a barrier, and the take copies, 1 KiB pieces (64 lanes x 16 bytes) dealt round-robin to the
// waves.  best_shot_final_kernel (one workgroup per stream, after the call's last frame) retires the entries whose tracks
// ended in the call.
// State of a stream: 16 bytes (the frame counter, 12 unused), then per slot an entry of 144 bytes + the crop rounded up to 16:
// id + 1, has-shot, key (64 bits), frame, row, status, one unused word, det[28], crop.  All zero = empty.
#include "lp_internal.h"
#include "lp_streams.h"
#include <cstring>

namespace lp {

namespace {

constexpr int BS_T = 1024;                      // threads of every workgroup here
constexpr int BS_WAVES = BS_T / 64;
constexpr int BS_HDR_BYTES = 16;
constexpr int BS_ENTRY_WORDS = 36;              // 8 header words + det[28]
constexpr int BS_W_DET = 8;
constexpr int BS_ROWS = LP_TRACK_MAX_DETS;      // rows of a frame that take part
constexpr int BS_SLOTS = LP_TRACK_MAX_TRACKS;
constexpr int BS_FRAMES = LP_FRAMES_PER_LAUNCH;
constexpr int SH_GREY_BYTES = 32768;            // LDS of a band of grey rows
constexpr int BS_MAX_SIDE = 1024;

struct BsTable {                                // 388 bytes of kernel arguments
    int nfr;
    int blk_stream[BS_FRAMES];                  // stream of workgroup k
    short fr_blk[BS_FRAMES];                    // workgroup that takes frame j of the launch, -1: skipped
};
struct BsJob { unsigned char* dst; const unsigned char* src; };

__device__ __forceinline__ unsigned grey_of(unsigned b, unsigned g, unsigned r) { return (29u * b + 150u * g + 77u * r + 128u) >> 8; }

// grid (n_slots), block (1024)
__global__ __launch_bounds__(BS_T) void crop_sharpness_kernel(const unsigned char* __restrict__ crops, const int32_t* __restrict__ status,
                                                              int crop_h, int crop_w, int band_rows, unsigned long long* __restrict__ sharp) {
    __shared__ __attribute__((aligned(16))) unsigned char s_grey[SH_GREY_BYTES];
    __shared__ unsigned long long s_wsum[BS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long slot = blockIdx.x;
    const int st = status[slot];
    if (!(st == 1 || st == 2) || crop_h < 3 || crop_w < 3) {     // (block-uniform)
        if (tid == 0) sharp[slot] = 0ull;
        return;
    }
    const unsigned char* crop = crops + slot * crop_h * crop_w * 3;
    unsigned acc = 0;
    // interior rows i0 .. i1-1 of a band; staged rows i0-1 .. i1
    for (int i0 = 1; i0 < crop_h - 1; i0 += band_rows - 2) {
        const int i1 = i0 + band_rows - 2 < crop_h - 1 ? i0 + band_rows - 2 : crop_h - 1;
        const int npix = (i1 - i0 + 2) * crop_w;
        const unsigned char* src = crop + (long long)(i0 - 1) * crop_w * 3;
        int done = 0;
        if (((uintptr_t)src & 3) == 0) {                       // four pixels = three aligned dwords
            const unsigned* s4 = (const unsigned*)src;
            const int ngrp = npix >> 2;
            for (int q = tid; q < ngrp; q += BS_T) {
                const unsigned a = s4[3 * q], b = s4[3 * q + 1], c = s4[3 * q + 2];
                const unsigned g0 = grey_of(a & 255u, (a >> 8) & 255u, (a >> 16) & 255u);
                const unsigned g1 = grey_of(a >> 24, b & 255u, (b >> 8) & 255u);
                const unsigned g2 = grey_of((b >> 16) & 255u, b >> 24, c & 255u);
                const unsigned g3 = grey_of((c >> 8) & 255u, (c >> 16) & 255u, c >> 24);
                ((unsigned*)s_grey)[q] = g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
            }
            done = ngrp << 2;
        }
        for (int p = done + tid; p < npix; p += BS_T) s_grey[p] = (unsigned char)grey_of(src[3 * p], src[3 * p + 1], src[3 * p + 2]);
        __syncthreads();
        const int iw = crop_w - 2, nin = (i1 - i0) * iw;
        for (int p = tid; p < nin; p += BS_T) {
            const int i = p / iw, j = p - i * iw + 1;
            const unsigned char* c = s_grey + (i + 1) * crop_w + j;
            const int L = 4 * (int)c[0] - (int)c[-crop_w] - (int)c[crop_w] - (int)c[-1] - (int)c[1];
            acc += (unsigned)(L * L);
        }
        __syncthreads();                                        // the next band overwrites the rows
    }
    unsigned long long sum = acc;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned lo = __shfl_down((unsigned)(sum & 0xffffffffull), d), hi = __shfl_down((unsigned)(sum >> 32), d);
        sum += ((unsigned long long)hi << 32) | lo;
    }
    if (lane == 0) s_wsum[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < BS_WAVES; ++w) t += s_wsum[w];
        sharp[slot] = t;
    }
}

__global__ void shots_clear_kernel(int32_t* shot_i, unsigned long long* shot_q, float* shot_det, long long n_rec) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_rec) shot_q[i] = 0ull;
    if (i < n_rec * 4) shot_i[i] = 0;
    if (i < n_rec * LP_DET_COLS) shot_det[i] = 0.f;
}

// Piece `p` of the copy of n bytes by one wave: 16-byte vectors where dst and src are congruent mod 16 (the bytes before
// dst's first 16-byte boundary and behind its last are taken one by one, in piece 0), bytes otherwise.
__device__ __forceinline__ void copy_piece(unsigned char* dst, const unsigned char* src, int n, int p, int lane) {
    if ((((uintptr_t)dst ^ (uintptr_t)src) & 15) == 0) {
        int head = (int)((16 - ((uintptr_t)dst & 15)) & 15);
        head = head < n ? head : n;
        const int nvec = (n - head) >> 4, tail = n - head - (nvec << 4);
        const int v = p * 64 + lane;
        if (v < nvec) ((uint4*)(dst + head))[v] = ((const uint4*)(src + head))[v];
        if (p == 0 && lane < head + tail) {
            const int o = lane < head ? lane : head + (nvec << 4) + (lane - head);
            dst[o] = src[o];
        }
    } else {
        const int o0 = (p * 64 + lane) * 16;
        for (int o = o0; o < o0 + 16 && o < n; ++o) dst[o] = src[o];
    }
}

__device__ __forceinline__ void run_jobs(const BsJob* jobs, int njobs, int crop_bytes, int wave, int lane) {
    const int npieces = (crop_bytes + 1023) >> 10;
    for (int q = wave; q < njobs * npieces; q += BS_WAVES) {
        const int job = q / npieces;
        copy_piece(jobs[job].dst, jobs[job].src, crop_bytes, q - job * npieces, lane);
    }
}

// first e < n_rec with ended_i[e][0] == id, or -1
__device__ __forceinline__ int find_record(const int32_t* rec, int n_rec, int id) {
    for (int e = 0; e < n_rec; ++e)
        if (rec[e * 12] == id) return e;
    return -1;
}

struct BsOut {
    unsigned char* shot_crops; int32_t* shot_i; unsigned long long* shot_q; float* shot_det;
};

// rule 5 for the entry at `en` of stream `strm` (one thread): the small outputs and the copy job; the entry becomes empty
__device__ __forceinline__ void retire_entry(int* en, int strm, const int32_t* rec, int n_rec, int max_ended, const BsOut& o,
                                             long long crop_bytes, BsJob* jobs, int* njobs) {
    const int e = find_record(rec, n_rec, en[0] - 1);
    if (e >= 0 && en[1] != 0) {
        const long long k = (long long)strm * max_ended + e;
        o.shot_i[k * 4] = en[4]; o.shot_i[k * 4 + 1] = en[5]; o.shot_i[k * 4 + 2] = en[6]; o.shot_i[k * 4 + 3] = 1;
        o.shot_q[k] = *(const unsigned long long*)(en + 2) & 0x7fffffffffffffffull;
        for (int c = 0; c < LP_DET_COLS; ++c) o.shot_det[k * LP_DET_COLS + c] = __int_as_float(en[BS_W_DET + c]);
        const int q = atomicAdd(njobs, 1);
        jobs[q].dst = o.shot_crops + k * crop_bytes;
        jobs[q].src = (const unsigned char*)(en + BS_ENTRY_WORDS);
    }
    en[0] = 0;
    en[1] = 0;
}

// grid (workgroups of this launch), block (1024).  det / count / tid / slot / crops / status / sharp: the launch's first frame.
__global__ __launch_bounds__(BS_T) void best_shot_kernel(const BsTable tab, unsigned char* __restrict__ state, int T, long long sstride,
                                                        long long estride, const float* __restrict__ det, const int32_t* __restrict__ count,
                                                        int max_det, const int32_t* __restrict__ tid_in, const int32_t* __restrict__ slot_in,
                                                        const unsigned char* __restrict__ crops, const int32_t* __restrict__ status,
                                                        const unsigned long long* __restrict__ sharp, int max_crops, int crop_bytes,
                                                        const int32_t* __restrict__ ended_i, const int32_t* __restrict__ ended_count,
                                                        int max_ended, float min_f, const BsOut out) {
    __shared__ BsJob s_retire[BS_ROWS], s_take[BS_ROWS];
    __shared__ int s_nretire, s_ntake;
    const int blk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int strm = tab.blk_stream[blk];
    unsigned char* const sst = state + (long long)strm * sstride;
    const int32_t* rec = ended_i + (long long)strm * max_ended * 12;
    int n_rec = ended_count[strm];
    n_rec = n_rec < 0 ? 0 : (n_rec < max_ended ? n_rec : max_ended);
    for (int j = 0; j < tab.nfr; ++j) {                                // (block-uniform control flow throughout)
        if (tab.fr_blk[j] != blk) continue;
        if (tid == 0) { s_nretire = 0; s_ntake = 0; }
        __syncthreads();
        const int frame = *(const int*)sst;
        int n = count[j];
        n = n < 0 ? 0 : (n > max_det ? max_det : n);
        n = n < max_crops ? n : max_crops;
        n = n < BS_ROWS ? n : BS_ROWS;
        if (tid < n) {
            const int r = tid;
            const int id = tid_in[(long long)j * max_det + r], g = slot_in[(long long)j * max_det + r];
            if (id >= 0 && g >= 0 && g < T) {
                int* en = (int*)(sst + BS_HDR_BYTES + (long long)g * estride);
                if (en[0] != id + 1) {
                    if (en[0] != 0) retire_entry(en, strm, rec, n_rec, max_ended, out, crop_bytes, s_retire, &s_nretire);
                    en[0] = id + 1;
                    en[1] = 0;
                }
                const float* row = det + ((long long)j * max_det + r) * LP_DET_COLS;
                const int st = status[(long long)j * max_crops + r];
                float sc = row[12] + row[13];
                sc = sc + row[14]; sc = sc + row[15]; sc = sc + row[16]; sc = sc + row[17]; sc = sc + row[18]; sc = sc + row[19];
                sc = sc / 8.0f;
                if ((st == 1 || st == 2) && sc >= min_f) {      // min_f = smallest fp32 >= min_score  <=>  (double)sc >= min_score
                    const unsigned long long key = ((unsigned long long)(st == 1) << 63) | sharp[(long long)j * max_crops + r];
                    if (en[1] == 0 || key > *(const unsigned long long*)(en + 2)) {
                        en[1] = 1;
                        *(unsigned long long*)(en + 2) = key;
                        en[4] = frame; en[5] = r; en[6] = st;
                        for (int c = 0; c < LP_DET_COLS; ++c) en[BS_W_DET + c] = __float_as_int(row[c]);
                        const int q = atomicAdd(&s_ntake, 1);
                        s_take[q].dst = (unsigned char*)(en + BS_ENTRY_WORDS);
                        s_take[q].src = crops + ((long long)j * max_crops + r) * crop_bytes;
                    }
                }
            }
        }
        __syncthreads();
        const int nretire = s_nretire, ntake = s_ntake;
        if (nretire) {
            run_jobs(s_retire, nretire, crop_bytes, wave, lane);
            __syncthreads();                                           // a take may overwrite the crop a retire has just read
        }
        if (ntake) run_jobs(s_take, ntake, crop_bytes, wave, lane);
        if (tid == 0) *(int*)sst = frame + 1;
        __syncthreads();                                               // the next frame reads the entries and reuses the lists
    }
}

// rule 6, after the call's last frame: grid (n_streams), block (1024)
__global__ __launch_bounds__(BS_T) void best_shot_final_kernel(unsigned char* __restrict__ state, int T, long long sstride, long long estride,
                                                              int crop_bytes, const int32_t* __restrict__ ended_i,
                                                              const int32_t* __restrict__ ended_count, int max_ended, const BsOut out) {
    __shared__ BsJob s_retire[BS_SLOTS];
    __shared__ int s_nretire;
    const int strm = blockIdx.x, tid = threadIdx.x;
    int n_rec = ended_count[strm];
    n_rec = n_rec < 0 ? 0 : (n_rec < max_ended ? n_rec : max_ended);
    if (n_rec == 0) return;                                            // (block-uniform)
    if (tid == 0) s_nretire = 0;
    __syncthreads();
    const int32_t* rec = ended_i + (long long)strm * max_ended * 12;
    if (tid < T) {
        int* en = (int*)(state + (long long)strm * sstride + BS_HDR_BYTES + (long long)tid * estride);
        if (en[0] != 0 && find_record(rec, n_rec, en[0] - 1) >= 0)
            retire_entry(en, strm, rec, n_rec, max_ended, out, crop_bytes, s_retire, &s_nretire);
    }
    __syncthreads();
    run_jobs(s_retire, s_nretire, crop_bytes, tid >> 6, tid & 63);
}

static_assert(BS_SLOTS == LP_TRACK_MAX_TRACKS, "stream_dims_fault states the rule of max_tracks");
bool crop_dims_ok(int crop_h, int crop_w) { return crop_h >= 1 && crop_w >= 1 && crop_h <= BS_MAX_SIDE && crop_w <= BS_MAX_SIDE; }
size_t entry_bytes(int crop_h, int crop_w) { return (size_t)BS_ENTRY_WORDS * 4 + (((size_t)crop_h * crop_w * 3 + 15) & ~(size_t)15); }
size_t shot_stream_bytes(int max_tracks, int crop_h, int crop_w) { return BS_HDR_BYTES + (size_t)max_tracks * entry_bytes(crop_h, crop_w); }

}  // namespace

}  // namespace lp

using namespace lp;

extern "C" int lp_crop_sharpness(const unsigned char* crops, const int32_t* status, int n_slots, int crop_h, int crop_w,
                                 unsigned long long* sharp, void* stream) {
    const std::string fn = "lp_crop_sharpness: ";
    if (n_slots < 0 || crop_h < 1 || crop_w < 1 || crop_h > BS_MAX_SIDE || crop_w > BS_MAX_SIDE)
        return fail(LP_ERR_ARG, fn + "need n_slots >= 0 and a crop size of 1..1024 on each side");
    if (n_slots == 0) return LP_OK;
    if (!crops || !status || !sharp) return fail(LP_ERR_ARG, fn + "null pointer");
    if (((uintptr_t)sharp & 7) != 0) return fail(LP_ERR_ARG, fn + "sharp must be 8-byte aligned");
    int band_rows = SH_GREY_BYTES / crop_w;                    // >= 32 rows: at least 30 interior rows per band
    band_rows = band_rows < crop_h ? band_rows : crop_h;
    band_rows = band_rows < 3 ? 3 : band_rows;
    hipLaunchKernelGGL(crop_sharpness_kernel, dim3((unsigned)n_slots), dim3(BS_T), 0, (hipStream_t)stream, crops, status, crop_h, crop_w,
                       band_rows, sharp);
    LP_HIP_CHECK(hipGetLastError());
    return LP_OK;
}

extern "C" size_t lp_best_shot_state_bytes(int n_streams, int max_tracks, int crop_h, int crop_w) {
    if (!stream_dims_fault(n_streams, max_tracks).empty() || !crop_dims_ok(crop_h, crop_w)) return 0;
    return (size_t)n_streams * shot_stream_bytes(max_tracks, crop_h, crop_w);
}

extern "C" int lp_best_shot_update(void* state, int n_streams, int max_tracks, int crop_h, int crop_w, const float* det, const int32_t* count,
                                   int B, int max_det, const int32_t* tid, const int32_t* slot, const unsigned char* crops,
                                   const int32_t* status, const unsigned long long* sharp, int max_crops, const int* stream_of,
                                   const int32_t* ended_i, const int32_t* ended_count, int max_ended, double min_score,
                                   unsigned char* shot_crops, int32_t* shot_i, unsigned long long* shot_q, float* shot_det, void* stream) {
    const std::string fn = "lp_best_shot_update: ";
    std::string why = stream_dims_fault(n_streams, max_tracks);
    if (!why.empty()) return fail(LP_ERR_ARG, fn + why);
    if (!crop_dims_ok(crop_h, crop_w)) return fail(LP_ERR_ARG, fn + "need a crop size of 1..1024 on each side");
    if (B < 0 || max_det < 1 || max_det > 0x7fffffff / LP_DET_COLS || max_ended < 0 || max_crops < 0)
        return fail(LP_ERR_ARG, fn + "need B >= 0, max_det >= 1, max_ended >= 0 and max_crops >= 0");
    if (!(std::fabs(min_score) <= 3.0e38)) return fail(LP_ERR_ARG, fn + "min_score must be finite (|min_score| <= 3e38)");
    if (!state || !ended_count || (max_ended > 0 && (!ended_i || !shot_crops || !shot_i || !shot_q || !shot_det)) ||
        (B > 0 && (!det || !count || !tid || !slot || !stream_of)) || (B > 0 && max_crops > 0 && (!crops || !status || !sharp)))
        return fail(LP_ERR_ARG, fn + "null pointer");
    if (((uintptr_t)state & 15) != 0) return fail(LP_ERR_ARG, fn + "state must be 16-byte aligned");
    if (((uintptr_t)sharp & 7) != 0 || ((uintptr_t)shot_q & 7) != 0) return fail(LP_ERR_ARG, fn + "sharp and shot_q must be 8-byte aligned");
    why = stream_of_fault(stream_of, B, n_streams);
    if (!why.empty()) return fail(LP_ERR_ARG, fn + why);
    const float min_f = f32_not_below(min_score);

    hipStream_t st = (hipStream_t)stream;
    const int crop_bytes = crop_h * crop_w * 3;
    const long long estride = (long long)entry_bytes(crop_h, crop_w), sstride = (long long)shot_stream_bytes(max_tracks, crop_h, crop_w);
    const BsOut out = {shot_crops, shot_i, shot_q, shot_det};
    const long long n_rec = (long long)n_streams * max_ended;
    if (n_rec > 0) {
        const long long n = n_rec * LP_DET_COLS;
        hipLaunchKernelGGL(shots_clear_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, shot_i, shot_q, shot_det, n_rec);
        LP_HIP_CHECK(hipGetLastError());
    }
    std::vector<int> blk_of((size_t)n_streams, -1);
    for (int b0 = 0; b0 < B; b0 += BS_FRAMES) {
        BsTable tab = {};
        tab.nfr = B - b0 < BS_FRAMES ? B - b0 : BS_FRAMES;
        const StreamPlan pl = plan_streams(stream_of + b0, tab.nfr, blk_of, UNTRACKED_LEAVE_OUT);
        if (pl.nblk == 0) continue;
        memcpy(tab.blk_stream, pl.blk_stream, sizeof(tab.blk_stream));
        memcpy(tab.fr_blk, pl.fr_blk, sizeof(tab.fr_blk));
        hipLaunchKernelGGL(best_shot_kernel, dim3((unsigned)pl.nblk), dim3(BS_T), 0, st, tab, (unsigned char*)state, max_tracks, sstride, estride,
                           det + (size_t)b0 * max_det * LP_DET_COLS, count + b0, max_det, tid + (size_t)b0 * max_det,
                           slot + (size_t)b0 * max_det, crops ? crops + (size_t)b0 * max_crops * crop_bytes : nullptr,
                           status ? status + (size_t)b0 * max_crops : nullptr, sharp ? sharp + (size_t)b0 * max_crops : nullptr, max_crops,
                           crop_bytes, ended_i, ended_count, max_ended, min_f, out);
        LP_HIP_CHECK(hipGetLastError());
    }
    if (max_ended > 0) {
        hipLaunchKernelGGL(best_shot_final_kernel, dim3((unsigned)n_streams), dim3(BS_T), 0, st, (unsigned char*)state, max_tracks, sstride,
                           estride, crop_bytes, ended_i, ended_count, max_ended, out);
        LP_HIP_CHECK(hipGetLastError());
    }
    return LP_OK;
}
