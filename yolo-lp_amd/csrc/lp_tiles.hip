// Tiled detection of large frames: lp_merge_tiles (include/lp_hip.h) merges the per-tile detections of every frame into one
// per-frame list on the device.  The reference has nothing here (Inferer shrinks every frame to one network input,
// yolov6/core/inferer.py:191-201); the written-down specification is yolov6/utils/tiles.py::merge_tiles_np, which this kernel
// matches bit for bit (tests/test_tiles_gpu.py).
//
// Per frame, one workgroup of 1024 threads:
//   1. every (tile, row) of the frame has a fixed candidate slot = local_tile * max_det_t + row.  A slot whose row exists and
//      passes the cut-plate filter appends the key (descending score bits, slot) -- score_key of lp_score.inc, the key lp_nms
//      sorts -- to the key list in LDS.  The order of the list is irrelevant, as in score_kernel: all keys are distinct and the
//      sort orders them, so the result is deterministic.
//   2. the list, padded with all-ones keys to a power of two, is sorted in LDS with the bitonic step of sort_kernel
//      (lp_nms_shared.inc): descending score, ties in slot order.  Real frames have tens of candidates: a 64-key sort.
//   3. greedy suppression ACROSS tiles, 64 sorted candidates at a time: all 16 waves test the chunk against the boxes kept so far
//      (a share of the list per wave; kept boxes, their tiles and slots live in LDS, beyond `kcap` entries in the caller's
//      workspace), then wave 0 settles the chunk's candidates among themselves in order.  A kept box suppresses only candidates
//      of OTHER tiles: rows of one tile have been through that tile's own NMS.
//   4. the first max_det kept rows are gathered from det_t, columns 0..11 shifted by the tile's origin; rows past the count are zero.
#include "lp_internal.h"
#include "lp_streams.h"
#include "lp_score.inc"
#include "lp_nms_shared.inc"
#include <vector>

namespace lp {

namespace {

constexpr int MT_T = SORT_T;                    // threads of the workgroup (bitonic_step strides by SORT_T)
constexpr int MT_WAVES = MT_T / 64;
constexpr int MT_TILES = 64;                    // tiles (and frames) per launch: the table travels as kernel arguments
constexpr int MT_LDS_BUDGET = 156 * 1024;       // dynamic LDS of the kernel: keys + kept list (the CU has 160 KiB; statics ~2 KiB)
constexpr int MT_KEPT_BYTES = 24;               // box (16) + tile (4) + slot (4) per kept entry

struct MtTile { int y0, x0, th, tw; };
struct MtFrame { int tile0, ntiles, h, w; };    // tile0: first tile of the frame in this launch's table
struct MtTable { MtTile t[MT_TILES]; MtFrame f[MT_TILES]; };   // 2 KiB of kernel arguments

typedef float box4 __attribute__((ext_vector_type(4)));

int pow2_at_least(int n) {
    int p = 64;
    while (p < n) p <<= 1;
    return p;
}

// inter / min(area_i, area_j) > thres (intersection over the smaller box): the fp32 ops of iou_gt with that denominator and a
// plain IEEE division.  A zero smaller area gives NaN (inter == 0: not suppressed) or +inf (suppressed), as in merge_tiles_np.
__device__ __forceinline__ bool ios_gt(float ix1, float iy1, float ix2, float iy2, float iarea, float jx1, float jy1, float jx2,
                                       float jy2, float thr_f) {
    const float xx1 = ix1 > jx1 ? ix1 : jx1;
    const float yy1 = iy1 > jy1 ? iy1 : jy1;
    const float xx2 = ix2 < jx2 ? ix2 : jx2;
    const float yy2 = iy2 < jy2 ? iy2 : jy2;
    float w = xx2 - xx1;
    if (!(w > 0.f)) w = 0.f;
    float h = yy2 - yy1;
    if (!(h > 0.f)) h = 0.f;
    const float inter = w * h;
    const float jarea = (jx2 - jx1) * (jy2 - jy1);
    const float d = iarea < jarea ? iarea : jarea;
    const float ovr = inter / d;
    return ovr > thr_f;   // thr_f = largest fp32 <= the double threshold  <=>  (double)ovr > thres
}

// grid (frames of this launch), block (1024), dynamic LDS = n_max keys (8 B) + kcap kept entries (24 B).
//   det_t / count_t: the launch's first tile; det / count / src / spill: the launch's first frame; gtile0: index of the launch's
//   first tile in the whole call (src numbers tiles over the call).  spill: per frame (spill_stride bytes apart) max_det + 64
//   entries of 24 B for kept entries at or past kcap (box4 [cap], then int tile [cap], then int slot [cap]).
__global__ __launch_bounds__(MT_T) void merge_tiles_kernel(const MtTable tab, const float* __restrict__ det_t, const int32_t* __restrict__ count_t,
                                                          int max_det_t, int gtile0, float thr_f, int metric, int border, int max_det,
                                                          int n_max, int kcap, float* __restrict__ det, int32_t* __restrict__ count,
                                                          int32_t* __restrict__ src, char* spill, size_t spill_stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long skeys[];   // [n_max] keys, then the kept list
    __shared__ __attribute__((aligned(16))) box4 s_cbox[64];    // the chunk's candidates: shifted box, local tile, slot
    __shared__ int s_ctile[64], s_cslot[64];
    __shared__ unsigned long long s_dead;
    __shared__ int s_T, s_nvalid;
    box4* const kbox = (box4*)(skeys + n_max);
    int* const ktile = (int*)(kbox + kcap);
    int* const kslot = ktile + kcap;
    const int fb = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MtFrame fr = tab.f[fb];
    const int scap = max_det + 64;                              // entries per frame of the spill area
    char* const sbase = spill + (size_t)fb * spill_stride;
    box4* const gbox = (box4*)sbase;
    int* const gtile = (int*)(gbox + scap);
    int* const gslot = gtile + scap;
    const int C = fr.ntiles * max_det_t;                        // candidate slots of this frame (<= SORT_LDS_KEYS, host-checked)

    // ---- 1. keys -------------------------------------------------------------------------------------------------------
    if (tid == 0) { s_nvalid = 0; s_T = 0; }
    __syncthreads();
    for (int s = tid; s < C; s += MT_T) {
        const int lt = s / max_det_t, r = s - lt * max_det_t;
        const int t = fr.tile0 + lt;
        int cnt = count_t[t];
        cnt = cnt < 0 ? 0 : (cnt > max_det_t ? max_det_t : cnt);
        if (r < cnt) {
            const float* row = det_t + ((long long)t * max_det_t + r) * LP_DET_COLS;
            const MtTile tl = tab.t[t];
            bool cut = false;
            if (border >= 0) {                              // a box that touches a tile side which is not a frame side
                const float x1 = row[0], y1 = row[1], x2 = row[2], y2 = row[3];
                const float bf = (float)border;
                cut = (tl.x0 > 0 && x1 <= bf) || (tl.y0 > 0 && y1 <= bf) || (tl.x0 + tl.tw < fr.w && x2 >= (float)(tl.tw - border)) ||
                      (tl.y0 + tl.th < fr.h && y2 >= (float)(tl.th - border));
            }
            if (!cut) {
                float sc = row[12] + row[13];
                sc = sc + row[14]; sc = sc + row[15]; sc = sc + row[16]; sc = sc + row[17]; sc = sc + row[18]; sc = sc + row[19];
                sc = sc / 8.0f;
                if (sc == 0.f) sc = 0.f;                    // -0 ties with +0
                skeys[atomicAdd(&s_nvalid, 1)] = score_key(sc, s);   // (any order: the keys are distinct and sorted next)
            }
        }
    }
    __syncthreads();
    const int nvalid = s_nvalid;
    int n = 64;
    while (n < nvalid) n <<= 1;
    for (int s = nvalid + tid; s < n; s += MT_T) skeys[s] = ~0ull;
    __syncthreads();

    // ---- 2. sort: valid keys first, in descending score, ties by slot ------------------------------------------------------
    if (nvalid > 0) {
        for (int k = 2; k <= n; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                bitonic_step(skeys, n, 0, k, j);
                __syncthreads();
            }
    }

    // ---- 3. greedy suppression across tiles ----------------------------------------------------------------------------------
    auto ov = [&](const box4& q, const box4& b) {                // q: an earlier (kept) box, b: the candidate
        const float qa = (q.z - q.x) * (q.w - q.y);
        return metric == 0 ? iou_gt(q.x, q.y, q.z, q.w, qa, b.x, b.y, b.z, b.w, thr_f) : ios_gt(q.x, q.y, q.z, q.w, qa, b.x, b.y, b.z, b.w, thr_f);
    };
    auto lane_f = [](float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); };
    const int nchunk = (nvalid + 63) / 64;
    int T = 0;                                                  // kept so far (block-uniform)
    for (int c = 0; c < nchunk; ++c) {
        if (wave == 0) {                                        // stage the chunk
            const int i = c * 64 + lane;
            box4 b = {0.f, 0.f, 0.f, 0.f};
            int lt = -1, slot = -1;
            if (i < nvalid) {
                slot = (int)(skeys[i] & 0xffffffffull);
                lt = slot / max_det_t;
                const int t = fr.tile0 + lt;
                const float* row = det_t + ((long long)t * max_det_t + (slot - lt * max_det_t)) * LP_DET_COLS;
                const float fx = (float)tab.t[t].x0, fy = (float)tab.t[t].y0;
                b.x = row[0] + fx; b.y = row[1] + fy; b.z = row[2] + fx; b.w = row[3] + fy;
            }
            s_cbox[lane] = b; s_ctile[lane] = lt; s_cslot[lane] = slot;
            if (lane == 0) s_dead = 0;
        }
        __syncthreads();
        const box4 bx = s_cbox[lane];
        const int tl = s_ctile[lane];
        {                                                       // against the kept list: wave w takes entries w, w + 16, ...
            bool dd = false;
            for (int k = wave; k < T; k += MT_WAVES) {          // (wave-uniform trip count)
                const box4 q = k < kcap ? kbox[k] : gbox[k];
                const int qt = k < kcap ? ktile[k] : gtile[k];
                if (!dd && tl >= 0 && qt != tl && ov(q, bx)) dd = true;
            }
            const unsigned long long m = __ballot(dd);
            if (lane == 0 && m) atomicOr(&s_dead, m);
        }
        __syncthreads();
        if (wave == 0) {                                        // the chunk among itself, in candidate order
            const bool alive = tl >= 0 && !((s_dead >> lane) & 1ull);
            unsigned long long todo = __ballot(alive), keptmask = 0;
            while (todo) {
                const int k = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
                keptmask |= 1ull << k;
                todo &= ~(1ull << k);
                const float bx0 = bx.x, bx1 = bx.y, bx2 = bx.z, bx3 = bx.w;
                const box4 q = {lane_f(bx0, k), lane_f(bx1, k), lane_f(bx2, k), lane_f(bx3, k)};
                const int qt = __builtin_amdgcn_readlane(tl, k);
                const bool hit = lane > k && tl >= 0 && qt != tl && ov(q, bx);
                todo &= ~__ballot(hit);
            }
            if ((keptmask >> lane) & 1ull) {
                const int pos = T + __popcll(keptmask & ((1ull << lane) - 1ull));
                if (pos < kcap) { kbox[pos] = bx; ktile[pos] = tl; kslot[pos] = s_cslot[lane]; }
                else if (pos < scap) { gbox[pos] = bx; gtile[pos] = tl; gslot[pos] = s_cslot[lane]; }
            }
            if (lane == 0) s_T = T + __popcll(keptmask);
        }
        __syncthreads();                                        // (orders the spill area's global stores inside the workgroup too)
        T = s_T;
        if (T >= max_det) break;                                // block-uniform
    }
    __syncthreads();

    // ---- 4. gather -----------------------------------------------------------------------------------------------------------
    const int total = T > max_det ? max_det : T;
    if (tid == 0) count[fb] = total;
    float* dout = det + (long long)fb * max_det * LP_DET_COLS;
    for (int i = tid; i < max_det * LP_DET_COLS; i += MT_T) {
        const int k = i / LP_DET_COLS, col = i - k * LP_DET_COLS;
        float v = 0.f;
        if (k < total) {
            const int slot = k < kcap ? kslot[k] : gslot[k];
            const int lt = slot / max_det_t, t = fr.tile0 + lt;
            v = det_t[((long long)t * max_det_t + (slot - lt * max_det_t)) * LP_DET_COLS + col];
            if (col < 12) v = v + (float)((col & 1) ? tab.t[t].y0 : tab.t[t].x0);
        }
        dout[i] = v;
    }
    for (int k = tid; k < max_det; k += MT_T) {
        int v = -1;
        if (k < total) {
            const int slot = k < kcap ? kslot[k] : gslot[k];
            const int lt = slot / max_det_t;
            v = (gtile0 + fr.tile0 + lt) * max_det_t + (slot - lt * max_det_t);
        }
        src[(long long)fb * max_det + k] = v;
    }
}

size_t spill_bytes_per_frame(int max_det) { return ((size_t)(max_det + 64) * MT_KEPT_BYTES + 255) / 256 * 256; }

}  // namespace

}  // namespace lp

using namespace lp;

extern "C" size_t lp_merge_tiles_workspace_bytes(int n_frames, int max_det) {
    if (n_frames < 1 || max_det < 1) return 256;
    return (size_t)n_frames * spill_bytes_per_frame(max_det);
}

extern "C" int lp_merge_tiles(const float* det_t, const int32_t* count_t, const lp_tile_ref* tiles, int n_tiles, int max_det_t,
                              const int* frame_hw, int n_frames, double thres, int metric, int border, int max_det, float* det,
                              int32_t* count, int32_t* src, void* workspace, size_t workspace_bytes, void* stream) {
    const std::string fn = "lp_merge_tiles: ";
    if (n_frames < 0 || n_tiles < 0 || max_det_t < 1 || max_det < 1 || max_det > 0x7fffffff / LP_DET_COLS - 64)
        return fail(LP_ERR_ARG, fn + "need n_frames, n_tiles >= 0 and max_det_t, max_det >= 1");
    if (!(thres >= 0.0 && thres <= 1.0)) return fail(LP_ERR_ARG, fn + "threshold must be in [0, 1]");
    if (metric != 0 && metric != 1) return fail(LP_ERR_ARG, fn + "metric must be 0 (IoU) or 1 (IoS)");
    if (n_frames == 0) {
        if (n_tiles != 0) return fail(LP_ERR_ARG, fn + "tiles without frames");
        return LP_OK;
    }
    if (!frame_hw || !det || !count || !src || !workspace || (n_tiles > 0 && (!det_t || !count_t || !tiles)))
        return fail(LP_ERR_ARG, fn + "null pointer");
    if (((uintptr_t)workspace & 15) != 0) return fail(LP_ERR_ARG, fn + "workspace must be 16-byte aligned");
    if (workspace_bytes < lp_merge_tiles_workspace_bytes(n_frames, max_det)) return fail(LP_ERR_ARG, fn + "workspace too small");
    if ((long long)n_tiles * max_det_t > 0x7fffffffLL) return fail(LP_ERR_ARG, fn + "n_tiles * max_det_t overflows the src numbering");
    for (int f = 0; f < n_frames; ++f)
        if (frame_hw[2 * f] < 1 || frame_hw[2 * f + 1] < 1) return fail(LP_ERR_ARG, fn + "bad size of frame " + std::to_string(f));
    // every tile is checked before the first launch; first[f] .. first[f + 1]: the tiles of frame f
    std::vector<int> first((size_t)n_frames + 1, 0);
    int prev = 0;
    for (int t = 0; t < n_tiles; ++t) {
        const lp_tile_ref& r = tiles[t];
        if (r.frame < prev || r.frame >= n_frames)
            return fail(LP_ERR_ARG, fn + "frame of tile " + std::to_string(t) + " (tiles of a frame must be contiguous, frames ascending)");
        const int h = frame_hw[2 * r.frame], w = frame_hw[2 * r.frame + 1];
        if (r.y0 < 0 || r.x0 < 0 || r.th < 1 || r.tw < 1 || r.th > h - r.y0 || r.tw > w - r.x0)
            return fail(LP_ERR_ARG, fn + "region of tile " + std::to_string(t) + " is not inside its frame");
        prev = r.frame;
        ++first[(size_t)r.frame + 1];
    }
    for (int f = 0; f < n_frames; ++f) {
        const int nt = first[(size_t)f + 1];
        if (nt > MT_TILES)
            return fail(LP_ERR_ARG, fn + "frame " + std::to_string(f) + " has " + std::to_string(nt) + " tiles (at most " + std::to_string(MT_TILES) + ")");
        if ((long long)nt * max_det_t > SORT_LDS_KEYS)
            return fail(LP_ERR_ARG, fn + "frame " + std::to_string(f) + ": " + std::to_string(nt) + " tiles x max_det_t " + std::to_string(max_det_t) +
                                        " = " + std::to_string((long long)nt * max_det_t) + " candidates (at most " + std::to_string(SORT_LDS_KEYS) + ")");
        first[(size_t)f + 1] += first[f];
    }
    static std::atomic<unsigned long long> attr{0};
    if (int rc = set_max_lds_once(merge_tiles_kernel, MT_LDS_BUDGET, attr, "merge tiles")) return rc;
    const float thr_f = f32_not_above(thres);
    hipStream_t st = (hipStream_t)stream;
    const size_t spf = spill_bytes_per_frame(max_det);
    for (int f0 = 0; f0 < n_frames;) {                          // whole frames per launch: <= 64 tiles and <= 64 frames
        MtTable tab = {};
        const int t0 = first[f0];
        int nf = 0, nt = 0, most = 0;
        while (f0 + nf < n_frames && nf < MT_TILES) {
            const int k = first[(size_t)f0 + nf + 1] - first[(size_t)f0 + nf];
            if (nt + k > MT_TILES) break;
            tab.f[nf] = {nt, k, frame_hw[2 * (f0 + nf)], frame_hw[2 * (f0 + nf) + 1]};
            for (int j = 0; j < k; ++j) {
                const lp_tile_ref& r = tiles[t0 + nt + j];
                tab.t[nt + j] = {r.y0, r.x0, r.th, r.tw};
            }
            nt += k;
            most = k > most ? k : most;
            ++nf;
        }
        const int n_max = pow2_at_least(most * max_det_t);
        long long kcap = ((long long)MT_LDS_BUDGET - (long long)n_max * 8) / MT_KEPT_BYTES / 64 * 64;
        if (kcap > max_det + 64) kcap = (max_det + 64 + 63) / 64 * 64;
        const size_t lds = (size_t)n_max * 8 + (size_t)kcap * MT_KEPT_BYTES;
        hipLaunchKernelGGL(merge_tiles_kernel, dim3((unsigned)nf), dim3(MT_T), lds, st, tab,
                           det_t ? det_t + (size_t)t0 * max_det_t * LP_DET_COLS : nullptr, count_t ? count_t + t0 : nullptr, max_det_t, t0, thr_f,
                           metric, border, max_det, n_max, (int)kcap, det + (size_t)f0 * max_det * LP_DET_COLS, count + f0,
                           src + (size_t)f0 * max_det, (char*)workspace + (size_t)f0 * spf, spf);
        LP_HIP_CHECK(hipGetLastError());
        f0 += nf;
    }
    return LP_OK;
}
