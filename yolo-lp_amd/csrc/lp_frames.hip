// Batched callers either side of the hot path: lp_preprocess_letterbox_batch, lp_preprocess_tiles_batch and lp_rescale_round_batch
// (include/lp_hip.h).
// They restate, for B frames of any source sizes in one launch per LP_FRAMES_PER_LAUNCH frames, what lp_prepost.hip does for
// one frame: Inferer.precess_image + letterbox (reference yolov6/core/inferer.py:191-201, yolov6/data/data_augment.py:30-61)
// and Inferer.rescale + .round() (inferer.py:203-228, :100).  Every output element is computed by the same expressions in the
// same order as the single-frame kernels, so the results are bit-identical to them (tests/test_frames_gpu.py).
//
// Descriptors are passed by value as a kernel-argument table (at most 64 entries, < 4 KiB of kernarg): nothing is uploaded,
// and the calls are safe under graph capture.
#include "lp_internal.h"
#include <vector>

namespace lp {

namespace {

constexpr int LB_COLS = 256;            // output columns of one workgroup (64 lanes x 4 pixels)
constexpr int LB_ROWS = 16;             // output rows of one workgroup (4 waves x 4 rows)

struct LbEntry {
    const unsigned char* img;
    int h0, w0, rh, rw, top, left;      // rh = rw = 0: a padding slot
    int resize, pitch;                  // pitch: bytes between source rows (w0 * 3 for a whole frame; the frame's for a region of it)
    double sy, sx;                      // h0 / rh, w0 / rw: divided on the host, as lp_preprocess_letterbox does
};
struct LbTable { LbEntry f[LP_FRAMES_PER_LAUNCH]; };

struct RsEntry { float ratio, padx, pady, wmax, hmax; };
struct RsTable { RsEntry e[LP_FRAMES_PER_LAUNCH]; };

template <typename TO> struct Vec4;
template <> struct Vec4<float> { typedef float T __attribute__((ext_vector_type(4))); };
template <> struct Vec4<f16> { typedef f16 T __attribute__((ext_vector_type(4))); };
template <> struct Vec4<bf16> { typedef bf16 T __attribute__((ext_vector_type(4))); };

// grid (column tiles x row bands, frames of this launch), block (64, 4).  Lane x owns 4 adjacent output columns; wave y owns
// rows y, y+4, y+8, y+12 of the band.  The per-column (x0, a0, a1) of the tile are computed once per workgroup into LDS.
// VEC: W % 4 == 0 and `out` 16-byte aligned, so the 4 pixels of a lane go out as one 8-byte (fp16/bf16) or 16-byte store.
template <typename TO, bool VEC>
__global__ __launch_bounds__(256) void letterbox_batch_kernel(const LbTable tab, TO* __restrict__ out, int H, int W, int n_ctiles) {
    __shared__ int s_x0[LB_COLS];
    __shared__ int s_a[LB_COLS];        // a0 | a1 << 16 (both in 0..2048)
    const LbEntry& f = tab.f[blockIdx.y];
    const int ct = blockIdx.x % n_ctiles, band = blockIdx.x / n_ctiles;
    const int tid = threadIdx.y * 64 + threadIdx.x;
    const int col0 = ct * LB_COLS;
    if (f.resize) {
        const int rx = col0 + tid - f.left;
        int x0 = 0, a0 = 0, a1 = 0;
        if (rx >= 0 && rx < f.rw) resize_coef(rx, f.sx, f.w0, &x0, &a0, &a1);
        s_x0[tid] = x0;
        s_a[tid] = a0 | (a1 << 16);
    }
    __syncthreads();

    const long long plane = (long long)H * W;
    TO* fout = out + (long long)blockIdx.y * 3 * plane;
    const int xl = threadIdx.x * 4, xc = col0 + xl;
    if (xc >= W) return;
    for (int k = 0; k < LB_ROWS / 4; ++k) {
        const int y = band * LB_ROWS + threadIdx.y + 4 * k;
        if (y >= H) break;
        const int ry = y - f.top;
        const bool row_in = ry >= 0 && ry < f.rh;
        const unsigned char *r0 = nullptr, *r1 = nullptr;
        int b0 = 0, b1 = 0;
        if (row_in) {
            if (f.resize) {
                int y0;
                resize_coef(ry, f.sy, f.h0, &y0, &b0, &b1);
                const int y1 = y0 + 1 < f.h0 ? y0 + 1 : f.h0 - 1;
                r0 = f.img + (long long)y0 * f.pitch;
                r1 = f.img + (long long)y1 * f.pitch;
            } else {
                r0 = f.img + (long long)ry * f.pitch;
            }
        }
        TO v[3][4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int rx = xc + p - f.left;
            int bgr[3] = {114, 114, 114};
            if (row_in && rx >= 0 && rx < f.rw) {
                if (!f.resize) {
                    const unsigned char* q = r0 + rx * 3;
                    bgr[0] = q[0]; bgr[1] = q[1]; bgr[2] = q[2];
                } else {
                    const int x0 = s_x0[xl + p], a = s_a[xl + p];
                    const int a0 = a & 0xffff, a1 = a >> 16;
                    const int x1 = x0 + 1 < f.w0 ? x0 + 1 : f.w0 - 1;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int h0v = r0[x0 * 3 + c] * a0 + r0[x1 * 3 + c] * a1;   // HResizeLinear (scaled by 2048)
                        const int h1v = r1[x0 * 3 + c] * a0 + r1[x1 * 3 + c] * a1;
                        bgr[c] = (((b0 * (h0v >> 4)) >> 16) + ((b1 * (h1v >> 4)) >> 16) + 2) >> 2;   // VResizeLinear
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][p] = (TO)((float)bgr[2 - c] / 255.f);   // BGR -> RGB, / 255 as lp_preprocess_letterbox
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            TO* o = fout + c * plane + (long long)y * W + xc;
            if (VEC) {
                typename Vec4<TO>::T w4 = {v[c][0], v[c][1], v[c][2], v[c][3]};
                *reinterpret_cast<typename Vec4<TO>::T*>(o) = w4;
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    if (xc + p < W) o[p] = v[c][p];
            }
        }
    }
}

// grid (ceil(max_det * 12 / 256), images of this launch): the expressions of rescale_round_kernel (lp_prepost.hip) on the first
// min(count[b], max_det) rows of image b; the count is read here, so the host never waits for it.
__global__ __launch_bounds__(256) void rescale_round_batch_kernel(float* __restrict__ det, const int32_t* __restrict__ count, int max_det,
                                                                 const RsTable tab) {
    const int b = blockIdx.y;
    int n = count[b];
    n = n < 0 ? 0 : (n > max_det ? max_det : n);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n * 12) return;
    const RsEntry& e = tab.e[b];
    const int row = i / 12, c = i - row * 12;
    float* p = det + ((long long)b * max_det + row) * LP_DET_COLS + c;
    float v = *p;
    v = v - ((c & 1) ? e.pady : e.padx);
    v = v / e.ratio;
    const float hi = (c & 1) ? e.hmax : e.wmax;
    v = v < 0.f ? 0.f : v;
    v = v > hi ? hi : v;
    *p = rintf(v);   // torch.round: half to even
}

template <typename TO>
int launch_letterbox(const LbTable& tab, int nf, void* out, int H, int W, bool vec, hipStream_t st) {
    const int n_ctiles = ceil_div(W, LB_COLS), n_bands = ceil_div(H, LB_ROWS);
    const dim3 grid((unsigned)(n_ctiles * n_bands), (unsigned)nf), block(64, 4);
    if (vec) hipLaunchKernelGGL((letterbox_batch_kernel<TO, true>), grid, block, 0, st, tab, (TO*)out, H, W, n_ctiles);
    else hipLaunchKernelGGL((letterbox_batch_kernel<TO, false>), grid, block, 0, st, tab, (TO*)out, H, W, n_ctiles);
    LP_HIP_CHECK(hipGetLastError());
    return LP_OK;
}

}  // namespace

}  // namespace lp

using namespace lp;

// One source image of a letterbox launch: a whole frame (pitch = w0 * 3) or a region of one (img = the region's first pixel,
// h0 x w0 = the region's size, pitch = the frame's).  The bilinear taps clamp at h0 / w0, i.e. at the region's edges.
struct LbSrc { const unsigned char* img; int h0, w0, pitch, rh, rw, top, left; };

// The launches of both entry points: slots [0, n) from `src`, slots [n, B) padding, LP_FRAMES_PER_LAUNCH slots per launch.
static int letterbox_run(const LbSrc* src, int n, int B, void* out, int out_dtype, int H, int W, hipStream_t st) {
    const size_t esz = dtype_size(out_dtype);
    const bool vec = W % 4 == 0 && ((uintptr_t)out & 15) == 0;
    for (int b0 = 0; b0 < B; b0 += LP_FRAMES_PER_LAUNCH) {
        const int nf = B - b0 < LP_FRAMES_PER_LAUNCH ? B - b0 : LP_FRAMES_PER_LAUNCH;
        LbTable tab = {};
        for (int j = 0; j < nf; ++j) {
            LbEntry& e = tab.f[j];
            if (b0 + j < n) {
                const LbSrc& d = src[b0 + j];
                e.img = d.img; e.h0 = d.h0; e.w0 = d.w0; e.rh = d.rh; e.rw = d.rw; e.top = d.top; e.left = d.left;
                e.pitch = d.pitch;
                e.resize = !(d.rh == d.h0 && d.rw == d.w0);
                e.sy = (double)d.h0 / d.rh;
                e.sx = (double)d.w0 / d.rw;
            }                                   // else: zero entry = a padding slot (rh = rw = 0: every pixel is 114)
        }
        void* o = (char*)out + (size_t)b0 * 3 * H * W * esz;
        int rc = LP_OK;
        switch (out_dtype) {
            case LP_F16: rc = launch_letterbox<f16>(tab, nf, o, H, W, vec, st); break;
            case LP_BF16: rc = launch_letterbox<bf16>(tab, nf, o, H, W, vec, st); break;
            default: rc = launch_letterbox<float>(tab, nf, o, H, W, vec, st); break;
        }
        if (rc != LP_OK) return rc;
    }
    return LP_OK;
}

extern "C" int lp_preprocess_letterbox_batch(const lp_frame_desc* desc, int n_frames, int B, void* out, int out_dtype, int H, int W,
                                             void* stream) {
    const char* fn = "lp_preprocess_letterbox_batch: ";
    if (out_dtype != LP_F16 && out_dtype != LP_BF16 && out_dtype != LP_F32) return fail(LP_ERR_ARG, std::string(fn) + "dtype");
    if (!out || B < 1 || n_frames < 0 || n_frames > B || (n_frames > 0 && !desc) || H < 1 || W < 1 ||
        (long long)ceil_div(H, LB_ROWS) * ceil_div(W, LB_COLS) > 0x7fffffffLL)
        return fail(LP_ERR_ARG, std::string(fn) + "bad arguments (need out, 0 <= n_frames <= B, B >= 1, H, W >= 1)");
    std::vector<LbSrc> src((size_t)n_frames);
    for (int b = 0; b < n_frames; ++b) {       // the rules of lp_preprocess_letterbox, all checked before any launch
        const lp_frame_desc& d = desc[b];
        if (!d.img || d.h0 < 1 || d.w0 < 1 || d.rh < 1 || d.rw < 1 || d.top < 0 || d.left < 0 || d.top + d.rh > H ||
            d.left + d.rw > W || d.w0 > 0x7fffffff / 3)
            return fail(LP_ERR_ARG, std::string(fn) + "bad geometry of frame " + std::to_string(b));
        src[b] = {d.img, d.h0, d.w0, d.w0 * 3, d.rh, d.rw, d.top, d.left};
    }
    return letterbox_run(src.data(), n_frames, B, out, out_dtype, H, W, (hipStream_t)stream);
}

extern "C" int lp_preprocess_tiles_batch(const lp_tile_desc* desc, int n_tiles, int B, void* out, int out_dtype, int H, int W,
                                         void* stream) {
    const char* fn = "lp_preprocess_tiles_batch: ";
    if (out_dtype != LP_F16 && out_dtype != LP_BF16 && out_dtype != LP_F32) return fail(LP_ERR_ARG, std::string(fn) + "dtype");
    if (!out || B < 1 || n_tiles < 0 || n_tiles > B || (n_tiles > 0 && !desc) || H < 1 || W < 1 ||
        (long long)ceil_div(H, LB_ROWS) * ceil_div(W, LB_COLS) > 0x7fffffffLL)
        return fail(LP_ERR_ARG, std::string(fn) + "bad arguments (need out, 0 <= n_tiles <= B, B >= 1, H, W >= 1)");
    std::vector<LbSrc> src((size_t)n_tiles);
    for (int b = 0; b < n_tiles; ++b) {        // every tile is checked before any launch
        const lp_tile_desc& d = desc[b];
        if (!d.img || d.h0 < 1 || d.w0 < 1 || d.w0 > 0x7fffffff / 3 || d.y0 < 0 || d.x0 < 0 || d.th < 1 || d.tw < 1 ||
            d.th > d.h0 - d.y0 || d.tw > d.w0 - d.x0)
            return fail(LP_ERR_ARG, std::string(fn) + "region of tile " + std::to_string(b) + " is not inside its frame");
        if (d.rh < 1 || d.rw < 1 || d.top < 0 || d.left < 0 || d.top + d.rh > H || d.left + d.rw > W)
            return fail(LP_ERR_ARG, std::string(fn) + "bad geometry of tile " + std::to_string(b));
        // the region as a view of the frame: its first pixel, its own size, the frame's row pitch
        src[b] = {d.img + ((long long)d.y0 * d.w0 + d.x0) * 3, d.th, d.tw, d.w0 * 3, d.rh, d.rw, d.top, d.left};
    }
    return letterbox_run(src.data(), n_tiles, B, out, out_dtype, H, W, (hipStream_t)stream);
}

extern "C" int lp_rescale_round_batch(float* det, const int32_t* count, int B, int max_det, const lp_rescale_desc* desc, void* stream) {
    const char* fn = "lp_rescale_round_batch: ";
    if (B < 0 || max_det < 0 || max_det > 0x7fffffff / 12)
        return fail(LP_ERR_ARG, std::string(fn) + "B and max_det must be >= 0");
    if (B == 0 || max_det == 0) return LP_OK;
    if (!det || !count || !desc) return fail(LP_ERR_ARG, std::string(fn) + "null pointer");
    for (int b = 0; b < B; ++b)
        if (!(desc[b].ratio > 0.0)) return fail(LP_ERR_ARG, std::string(fn) + "ratio of image " + std::to_string(b) + " must be > 0");
    hipStream_t st = (hipStream_t)stream;
    const unsigned gx = (unsigned)ceil_div(max_det * 12, 256);
    for (int b0 = 0; b0 < B; b0 += LP_FRAMES_PER_LAUNCH) {
        const int nf = B - b0 < LP_FRAMES_PER_LAUNCH ? B - b0 : LP_FRAMES_PER_LAUNCH;
        RsTable tab = {};
        for (int j = 0; j < nf; ++j) {
            const lp_rescale_desc& d = desc[b0 + j];   // (float) of the doubles, as lp_rescale_round passes them
            tab.e[j] = {(float)d.ratio, (float)d.padx, (float)d.pady, (float)d.img_w, (float)d.img_h};
        }
        hipLaunchKernelGGL(rescale_round_batch_kernel, dim3(gx, (unsigned)nf), dim3(256), 0, st,
                           det + (size_t)b0 * max_det * LP_DET_COLS, count + b0, max_det, tab);
        LP_HIP_CHECK(hipGetLastError());
    }
    return LP_OK;
}
