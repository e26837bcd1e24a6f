// Batched callers either side of the hot path: lp_preprocess_letterbox_batch, lp_preprocess_tiles_batch, lp_preprocess_nv12_batch
// and lp_rescale_round_batch (include/lp_hip.h).
// They restate, for B images of any source sizes in one launch per table of slots, what lp_prepost.hip does for one frame:
// Inferer.precess_image + letterbox (reference yolov6/core/inferer.py:191-201, yolov6/data/data_augment.py:30-61) and
// Inferer.rescale + .round() (inferer.py:203-228, :100).  Every output element is computed by the same expressions in the same
// order as the single-frame kernels, so the results are bit-identical to them (tests/test_frames_gpu.py).
//
// The three letterbox entry points are ONE kernel, letterbox_kernel, over two pixel sources: BgrSrc reads a region of a uint8
// [h,w,3] BGR frame (a whole frame is the region (0, 0, h0, w0)), Nv12Src a region of an NV12 frame, each tap converted to BGR in
// registers by the rule of lp_nv12_color.inc (specification: yolov6/utils/nv12.py; the reference has nothing there).  A source
// supplies its table entry, the set-up of two source rows, one unresized pixel and the four bilinear taps; the tiling, the
// coefficients, the blend, the padding and the conversion to the output dtype are the kernel's, so lp_preprocess_nv12_batch equals
// lp_preprocess_tiles_batch on the converted frame (tests/test_nv12_gpu.py).
//
// Descriptors are passed by value as a kernel-argument table (< 4 KiB of kernarg: 64 BGR entries of 56 bytes, LP_FRAMES_PER_LAUNCH,
// or 32 NV12 entries of 80, LP_NV12_PER_LAUNCH): nothing is uploaded, and the calls are safe under graph capture.
#include "lp_internal.h"
#include <vector>

namespace lp {

namespace {

#include "lp_nv12_color.inc"

constexpr int LB_COLS = 256;            // output columns of one workgroup (64 lanes x 4 pixels)
constexpr int LB_ROWS = 16;             // output rows of one workgroup (4 waves x 4 rows)

// What every slot of a letterbox table says, whatever its source: a th x tw region of a frame, resized to rh x rw at (top, left)
// of the output.  The bilinear taps clamp at th / tw, i.e. at the region's edges.
struct LbGeom {
    int th, tw, rh, rw, top, left;      // rh = rw = 0: a padding slot
    int resize, pitch;                  // pitch: bytes between rows of the source's first plane (BGR: w0 * 3; NV12: pitch_y)
    double sy, sx;                      // th / rh, tw / rw: divided on the host, as lp_preprocess_letterbox does
};
LbGeom geom_of(int th, int tw, int pitch, int rh, int rw, int top, int left) {
    return {th, tw, rh, rw, top, left, !(rh == th && rw == tw), pitch, (double)th / rh, (double)tw / rw};
}

// A pixel source: its table entry (Entry, SLOTS of them per launch) and, for one lane, the pixels of the two source rows last set.
struct BgrSrc {
    struct Entry { LbGeom g; const unsigned char* img; };      // img: the region's first pixel
    static constexpr int SLOTS = LP_FRAMES_PER_LAUNCH;
    const Entry& f;
    const unsigned char *r0 = nullptr, *r1 = nullptr;
    __device__ __forceinline__ BgrSrc(const Entry& e) : f(e) {}
    __device__ __forceinline__ void rows(int ya, int yb) {
        r0 = f.img + (long long)ya * f.g.pitch;
        r1 = f.img + (long long)yb * f.g.pitch;
    }
    __device__ __forceinline__ void pixel(int x, int* bgr) const {      // (ya, x)
        const unsigned char* q = r0 + x * 3;
        bgr[0] = q[0]; bgr[1] = q[1]; bgr[2] = q[2];
    }
    __device__ __forceinline__ void taps(int x0, int x1, int (*t)[3]) const {      // t[0..3] = (ya, x0), (ya, x1), (yb, x0), (yb, x1)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            t[0][c] = r0[x0 * 3 + c]; t[1][c] = r0[x1 * 3 + c];
            t[2][c] = r1[x0 * 3 + c]; t[3][c] = r1[x1 * 3 + c];
        }
    }
};

// A UV pair is one aligned 16-bit load; the two horizontal taps share it when they fall into one chroma site (x0 even, or the tap
// clamped), the two vertical taps when their rows do.
struct Nv12Src {
    struct Entry {
        LbGeom g;
        const unsigned char* y;         // first luma byte of the REGION
        const unsigned char* uv;        // the frame's chroma plane
        int pitch_uv, y0, x0, matrix;   // the region's origin in the frame: chroma is indexed by the absolute coordinate
    };
    static constexpr int SLOTS = LP_NV12_PER_LAUNCH;
    const Entry& f;
    const NvMat m;
    const unsigned char *r0 = nullptr, *r1 = nullptr, *c0 = nullptr, *c1 = nullptr;   // luma rows (region column 0), chroma rows
    bool one_crow = true;
    __device__ __forceinline__ Nv12Src(const Entry& e) : f(e), m(NV_MAT[e.matrix]) {}
    __device__ __forceinline__ void rows(int ya, int yb) {
        r0 = f.y + (long long)ya * f.g.pitch;
        r1 = f.y + (long long)yb * f.g.pitch;
        const int ca = (f.y0 + ya) >> 1, cb = (f.y0 + yb) >> 1;
        c0 = f.uv + (long long)ca * f.pitch_uv;
        c1 = f.uv + (long long)cb * f.pitch_uv;
        one_crow = ca == cb;
    }
    __device__ __forceinline__ void pixel(int x, int* bgr) const { bgr_of(r0[x], chroma_of(ld16(c0 + ((f.x0 + x) >> 1) * 2), m), m, bgr); }
    __device__ __forceinline__ void taps(int x0, int x1, int (*t)[3]) const {
        const int q0 = ((f.x0 + x0) >> 1) * 2, q1 = ((f.x0 + x1) >> 1) * 2;     // byte offsets of the two chroma sites
        const Chroma ch00 = chroma_of(ld16(c0 + q0), m);
        const Chroma ch01 = q1 == q0 ? ch00 : chroma_of(ld16(c0 + q1), m);
        Chroma ch10 = ch00, ch11 = ch01;
        if (!one_crow) {
            ch10 = chroma_of(ld16(c1 + q0), m);
            ch11 = q1 == q0 ? ch10 : chroma_of(ld16(c1 + q1), m);
        }
        bgr_of(r0[x0], ch00, m, t[0]);
        bgr_of(r0[x1], ch01, m, t[1]);
        bgr_of(r1[x0], ch10, m, t[2]);
        bgr_of(r1[x1], ch11, m, t[3]);
    }
};

template <typename SRC> struct LbTable { typename SRC::Entry f[SRC::SLOTS]; };
static_assert(sizeof(LbTable<BgrSrc>) < 4096 && sizeof(LbTable<Nv12Src>) < 4096, "a table travels as kernel arguments: under 4 KiB");

struct RsEntry { float ratio, padx, pady, wmax, hmax; };
struct RsTable { RsEntry e[LP_FRAMES_PER_LAUNCH]; };

template <typename TO> struct Vec4;
template <> struct Vec4<float> { typedef float T __attribute__((ext_vector_type(4))); };
template <> struct Vec4<f16> { typedef f16 T __attribute__((ext_vector_type(4))); };
template <> struct Vec4<bf16> { typedef bf16 T __attribute__((ext_vector_type(4))); };

// grid (column tiles x row bands, slots of this launch), block (64, 4).  Lane x owns 4 adjacent output columns; wave y owns
// rows y, y+4, y+8, y+12 of the band.  The per-column (x0, a0, a1) of the tile are computed once per workgroup into LDS.
// VEC: W % 4 == 0 and `out` 16-byte aligned, so the 4 pixels of a lane go out as one 8-byte (fp16/bf16) or 16-byte store.
template <typename SRC, typename TO, bool VEC>
__global__ __launch_bounds__(256) void letterbox_kernel(const LbTable<SRC> tab, TO* __restrict__ out, int H, int W, int n_ctiles) {
    __shared__ int s_x0[LB_COLS];
    __shared__ int s_a[LB_COLS];        // a0 | a1 << 16 (both in 0..2048)
    const LbGeom g = tab.f[blockIdx.y].g;     // a copy: read once per workgroup, not again from the table at every row and pixel
    const int ct = blockIdx.x % n_ctiles, band = blockIdx.x / n_ctiles;
    const int tid = threadIdx.y * 64 + threadIdx.x;
    const int col0 = ct * LB_COLS;
    if (g.resize) {
        const int rx = col0 + tid - g.left;
        int x0 = 0, a0 = 0, a1 = 0;
        if (rx >= 0 && rx < g.rw) resize_coef(rx, g.sx, g.tw, &x0, &a0, &a1);
        s_x0[tid] = x0;
        s_a[tid] = a0 | (a1 << 16);
    }
    __syncthreads();

    SRC src(tab.f[blockIdx.y]);
    const long long plane = (long long)H * W;
    TO* fout = out + (long long)blockIdx.y * 3 * plane;
    const int xl = threadIdx.x * 4, xc = col0 + xl;
    if (xc >= W) return;
    for (int k = 0; k < LB_ROWS / 4; ++k) {
        const int y = band * LB_ROWS + threadIdx.y + 4 * k;
        if (y >= H) break;
        const int ry = y - g.top;
        const bool row_in = ry >= 0 && ry < g.rh;
        int b0 = 0, b1 = 0;
        if (row_in) {
            int ya = ry, yb = ry;
            if (g.resize) {
                resize_coef(ry, g.sy, g.th, &ya, &b0, &b1);
                yb = ya + 1 < g.th ? ya + 1 : g.th - 1;
            }
            src.rows(ya, yb);
        }
        TO v[3][4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int rx = xc + p - g.left;
            int bgr[3] = {LETTERBOX_PAD, LETTERBOX_PAD, LETTERBOX_PAD};
            if (row_in && rx >= 0 && rx < g.rw) {
                if (!g.resize) {
                    src.pixel(rx, bgr);
                } else {
                    const int x0 = s_x0[xl + p], a = s_a[xl + p];
                    const int a0 = a & 0xffff, a1 = a >> 16;
                    const int x1 = x0 + 1 < g.tw ? x0 + 1 : g.tw - 1;
                    int t[4][3];
                    src.taps(x0, x1, t);
#pragma unroll
                    for (int c = 0; c < 3; ++c) bgr[c] = resize_blend(t[0][c], t[1][c], t[2][c], t[3][c], a0, a1, b0, b1);
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

template <typename SRC, typename TO>
void launch_letterbox(const LbTable<SRC>& tab, int nf, void* out, int H, int W, bool vec, hipStream_t st) {
    const int n_ctiles = ceil_div(W, LB_COLS), n_bands = ceil_div(H, LB_ROWS);
    const dim3 grid((unsigned)(n_ctiles * n_bands), (unsigned)nf), block(64, 4);
    if (vec) hipLaunchKernelGGL((letterbox_kernel<SRC, TO, true>), grid, block, 0, st, tab, (TO*)out, H, W, n_ctiles);
    else hipLaunchKernelGGL((letterbox_kernel<SRC, TO, false>), grid, block, 0, st, tab, (TO*)out, H, W, n_ctiles);
}

// The launches of the three entry points: slots [0, src.size()) from `src`, the slots up to B padding, SRC::SLOTS slots per launch.
template <typename SRC>
int letterbox_run(const std::vector<typename SRC::Entry>& src, int B, void* out, int out_dtype, int H, int W, hipStream_t st) {
    const size_t esz = dtype_size(out_dtype);
    const bool vec = W % 4 == 0 && ((uintptr_t)out & 15) == 0;
    for (int b0 = 0; b0 < B; b0 += SRC::SLOTS) {
        const int nf = B - b0 < SRC::SLOTS ? B - b0 : SRC::SLOTS;
        LbTable<SRC> tab = {};          // a zero entry = a padding slot (rh = rw = 0: every pixel is 114)
        for (int j = 0; j < nf && b0 + j < (int)src.size(); ++j) tab.f[j] = src[b0 + j];
        void* o = (char*)out + (size_t)b0 * 3 * H * W * esz;
        switch (out_dtype) {
            case LP_F16: launch_letterbox<SRC, f16>(tab, nf, o, H, W, vec, st); break;
            case LP_BF16: launch_letterbox<SRC, bf16>(tab, nf, o, H, W, vec, st); break;
            default: launch_letterbox<SRC, float>(tab, nf, o, H, W, vec, st); break;
        }
        LP_HIP_CHECK(hipGetLastError());
    }
    return LP_OK;
}

// The argument rules the three entry points share (`count`: what the entry point calls n); LP_OK, or the failure set.
int batch_fault(const std::string& fn, const char* count, const void* desc, int n, int B, const void* out, int out_dtype, int H, int W) {
    if (out_dtype != LP_F16 && out_dtype != LP_BF16 && out_dtype != LP_F32) return fail(LP_ERR_ARG, fn + "dtype");
    if (!out || B < 1 || n < 0 || n > B || (n > 0 && !desc) || H < 1 || W < 1 ||
        (long long)ceil_div(H, LB_ROWS) * ceil_div(W, LB_COLS) > 0x7fffffffLL)
        return fail(LP_ERR_ARG, fn + "bad arguments (need out, 0 <= " + count + " <= B, B >= 1, H, W >= 1)");
    return LP_OK;
}

// The rules of one slot, `what` naming it: the region (y0, x0, th, tw) inside its h0 x w0 frame (`frame_ok`: what else the entry
// point asks of the frame), the geometry (rh, rw, top, left) inside the H x W output.  An empty string: fine.
std::string region_fault(const std::string& what, bool frame_ok, int h0, int w0, int y0, int x0, int th, int tw, int rh, int rw,
                         int top, int left, int H, int W) {
    if (!frame_ok || h0 < 1 || w0 < 1 || y0 < 0 || x0 < 0 || th < 1 || tw < 1 || th > h0 - y0 || tw > w0 - x0)
        return "region of " + what + " is not inside its frame";
    if (rh < 1 || rw < 1 || top < 0 || left < 0 || top + rh > H || left + rw > W) return "bad geometry of " + what;
    return "";
}

}  // namespace

}  // namespace lp

using namespace lp;

extern "C" int lp_preprocess_letterbox_batch(const lp_frame_desc* desc, int n_frames, int B, void* out, int out_dtype, int H, int W,
                                             void* stream) {
    const std::string fn = "lp_preprocess_letterbox_batch: ";
    const int rc = batch_fault(fn, "n_frames", desc, n_frames, B, out, out_dtype, H, W);
    if (rc != LP_OK) return rc;
    std::vector<BgrSrc::Entry> src((size_t)n_frames);
    for (int b = 0; b < n_frames; ++b) {       // the rules of lp_preprocess_letterbox, all checked before any launch
        const lp_frame_desc& d = desc[b];
        const std::string what = "frame " + std::to_string(b);
        const bool frame_ok = d.img && d.h0 >= 1 && d.w0 >= 1 && d.w0 <= 0x7fffffff / 3;
        if (!frame_ok || !region_fault(what, true, d.h0, d.w0, 0, 0, d.h0, d.w0, d.rh, d.rw, d.top, d.left, H, W).empty())
            return fail(LP_ERR_ARG, fn + "bad geometry of " + what);
        src[b] = {geom_of(d.h0, d.w0, d.w0 * 3, d.rh, d.rw, d.top, d.left), d.img};     // a whole frame: the region (0, 0, h0, w0)
    }
    return letterbox_run<BgrSrc>(src, B, out, out_dtype, H, W, (hipStream_t)stream);
}

extern "C" int lp_preprocess_tiles_batch(const lp_tile_desc* desc, int n_tiles, int B, void* out, int out_dtype, int H, int W,
                                         void* stream) {
    const std::string fn = "lp_preprocess_tiles_batch: ";
    const int rc = batch_fault(fn, "n_tiles", desc, n_tiles, B, out, out_dtype, H, W);
    if (rc != LP_OK) return rc;
    std::vector<BgrSrc::Entry> src((size_t)n_tiles);
    for (int b = 0; b < n_tiles; ++b) {        // every tile is checked before any launch
        const lp_tile_desc& d = desc[b];
        const std::string why = region_fault("tile " + std::to_string(b), d.img && d.w0 <= 0x7fffffff / 3, d.h0, d.w0, d.y0, d.x0, d.th,
                                             d.tw, d.rh, d.rw, d.top, d.left, H, W);
        if (!why.empty()) return fail(LP_ERR_ARG, fn + why);
        // the region as a view of the frame: its first pixel, its own size, the frame's row pitch
        src[b] = {geom_of(d.th, d.tw, d.w0 * 3, d.rh, d.rw, d.top, d.left), d.img + ((long long)d.y0 * d.w0 + d.x0) * 3};
    }
    return letterbox_run<BgrSrc>(src, B, out, out_dtype, H, W, (hipStream_t)stream);
}

extern "C" int lp_preprocess_nv12_batch(const lp_nv12_desc* desc, int n, int B, void* out, int out_dtype, int H, int W, void* stream) {
    const std::string fn = "lp_preprocess_nv12_batch: ";
    const int rc = batch_fault(fn, "n", desc, n, B, out, out_dtype, H, W);
    if (rc != LP_OK) return rc;
    std::vector<Nv12Src::Entry> src((size_t)n);
    for (int b = 0; b < n; ++b) {              // every entry is checked before the first launch
        const lp_nv12_desc& d = desc[b];
        std::string why = plane_fault(d.y, d.uv, d.pitch_y, d.pitch_uv, d.h0, d.w0, d.matrix);
        if (!why.empty()) return fail(LP_ERR_ARG, fn + why + " (entry " + std::to_string(b) + ")");
        why = region_fault("entry " + std::to_string(b), true, d.h0, d.w0, d.y0, d.x0, d.th, d.tw, d.rh, d.rw, d.top, d.left, H, W);
        if (!why.empty()) return fail(LP_ERR_ARG, fn + why);
        src[b] = {geom_of(d.th, d.tw, d.pitch_y, d.rh, d.rw, d.top, d.left), d.y + (long long)d.y0 * d.pitch_y + d.x0, d.uv,
                  d.pitch_uv, d.y0, d.x0, d.matrix};
    }
    return letterbox_run<Nv12Src>(src, B, out, out_dtype, H, W, (hipStream_t)stream);
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
