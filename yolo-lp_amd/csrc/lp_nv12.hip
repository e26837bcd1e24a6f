// NV12 video frames: lp_preprocess_nv12_batch and lp_nv12_to_bgr_batch (include/lp_hip.h).  The reference has nothing here
// (its Inferer takes what cv2 decodes, BGR); the written-down specification is yolov6/utils/nv12.py (nv12_to_bgr_np,
// letterbox_nv12_np, region_nv12_np), which these kernels match bit for bit (tests/test_nv12_gpu.py).
//
// The rule, for pixel (i, j) of an h0 x w0 frame (both even) with planes y [h0][pitch_y] and uv [h0/2][pitch_uv] (U, V pairs):
//     Y = y[i][j], U = uv[i >> 1][2 (j >> 1)], V = uv[i >> 1][2 (j >> 1) + 1]        (chroma replicated, not interpolated)
//     c = max(Y - yoff, 0) * CY;  d = U - 128;  e = V - 128;  half = 1 << 19         (int32, arithmetic shifts)
//     R = clamp255((c + half + CVR e) >> 20), G = clamp255((c + half + CVG e + CUG d) >> 20), B = clamp255((c + half + CUB d) >> 20)
// with the integers of NV_MAT below (|accumulator| < 5.9e8 over all 2^24 triples).
//
// nv12_letterbox_kernel keeps the shape of letterbox_batch_kernel (lp_frames.hip): block (64, 4) = 256 columns x 16 rows, the
// per-column (x0, a0, a1) once per workgroup in LDS, 4 adjacent pixels of a lane per channel as one 8- or 16-byte store.  Each of
// the four bilinear taps is converted to BGR in registers and then goes through the very expressions of that kernel, so the
// result equals lp_preprocess_tiles_batch on the converted frame.  A UV pair is one aligned 16-bit load; the two horizontal taps
// share it when they fall into one chroma site (x0 even, or the tap clamped), the two vertical taps when their rows do.
//
// nv12_to_bgr_kernel streams: a lane owns 8 pixels x 2 rows = one 8-byte UV load (4 pairs), two 8-byte Y loads, two 24-byte
// runs of output.  Vector loads / stores where the plane's base and pitch (the output's base and row length) are 8-byte
// aligned; byte accesses otherwise and for a row's tail of 2, 4 or 6 pixels.
//
// Descriptors travel by value in the kernel arguments (nothing uploaded, no host sync, capturable).  An entry of the letterbox
// table is 80 bytes (two planes, two pitches, the region's origin for the chroma parity, the matrix), so a launch takes
// LP_NV12_PER_LAUNCH = 32 slots (2.5 KiB of kernarg) where the BGR kernel takes 64; the convert table is 48 bytes x 64.
#include "lp_internal.h"
#include <vector>

namespace lp {

namespace {

constexpr int NV_COLS = 256;            // output columns of one letterbox workgroup (64 lanes x 4 pixels)
constexpr int NV_ROWS = 16;             // output rows of one letterbox workgroup (4 waves x 4 rows)
constexpr int NV_SHIFT = 20;
constexpr int NV_HALF = 1 << (NV_SHIFT - 1);
constexpr int NV_MATRICES = 4;

struct NvMat { int yoff, cy, cub, cug, cvg, cvr; };
__constant__ NvMat NV_MAT[NV_MATRICES] = {
    {16, 1220542, 2116026, -409993, -852492, 1673527},      // 0 bt601, limited range (OpenCV's COLOR_YUV2BGR_NV12 table)
    {16, 1220945, 2215014, -223607, -558796, 1879825},      // 1 bt709, limited range
    {0, 1048576, 1858077, -360853, -748826, 1470104},       // 2 bt601, full range
    {0, 1048576, 1945738, -196424, -490864, 1651297},       // 3 bt709, full range
};

struct NvEntry {
    const unsigned char* y;             // first luma byte of the REGION
    const unsigned char* uv;            // the frame's chroma plane
    int pitch_y, pitch_uv;
    int y0, x0, th, tw;                 // the region: origin in the frame (chroma is indexed by the absolute coordinate), size
    int rh, rw, top, left;              // rh = rw = 0: a padding slot
    int resize, matrix;
    double sy, sx;                      // th / rh, tw / rw: divided on the host, as lp_preprocess_letterbox does
};
struct NvTable { NvEntry f[LP_NV12_PER_LAUNCH]; };

struct CvEntry {
    const unsigned char* y;
    const unsigned char* uv;
    unsigned char* out;
    int pitch_y, pitch_uv, h0, w0;
    int matrix, flags;                  // flags: 1 = 8-byte Y loads, 2 = 8-byte UV loads, 4 = 8-byte stores
};
struct CvTable { CvEntry f[LP_FRAMES_PER_LAUNCH]; };

template <typename TO> struct Vec4;
template <> struct Vec4<float> { typedef float T __attribute__((ext_vector_type(4))); };
template <> struct Vec4<f16> { typedef f16 T __attribute__((ext_vector_type(4))); };
template <> struct Vec4<bf16> { typedef bf16 T __attribute__((ext_vector_type(4))); };

struct Chroma { int b, g, r; };         // the chroma terms of one UV pair

__device__ __forceinline__ Chroma chroma_of(unsigned pair, const NvMat& m) {     // pair: U | V << 8
    const int d = (int)(pair & 255u) - 128, e = (int)(pair >> 8) - 128;
    return {m.cub * d, m.cvg * e + m.cug * d, m.cvr * e};
}
__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ __forceinline__ void bgr_of(int Y, const Chroma& ch, const NvMat& m, int* bgr) {
    const int c0 = Y - m.yoff;
    const int c = (c0 < 0 ? 0 : c0) * m.cy + NV_HALF;
    bgr[0] = clamp255((c + ch.b) >> NV_SHIFT);
    bgr[1] = clamp255((c + ch.g) >> NV_SHIFT);
    bgr[2] = clamp255((c + ch.r) >> NV_SHIFT);
}
__device__ __forceinline__ unsigned ld16(const unsigned char* p) { return *reinterpret_cast<const unsigned short*>(p); }

// grid (column tiles x row bands, slots of this launch), block (64, 4): as letterbox_batch_kernel.
template <typename TO, bool VEC>
__global__ __launch_bounds__(256) void nv12_letterbox_kernel(const NvTable tab, TO* __restrict__ out, int H, int W, int n_ctiles) {
    __shared__ int s_x0[NV_COLS];
    __shared__ int s_a[NV_COLS];        // a0 | a1 << 16 (both in 0..2048)
    const NvEntry& f = tab.f[blockIdx.y];
    const int ct = blockIdx.x % n_ctiles, band = blockIdx.x / n_ctiles;
    const int tid = threadIdx.y * 64 + threadIdx.x;
    const int col0 = ct * NV_COLS;
    if (f.resize) {
        const int rx = col0 + tid - f.left;
        int x0 = 0, a0 = 0, a1 = 0;
        if (rx >= 0 && rx < f.rw) resize_coef(rx, f.sx, f.tw, &x0, &a0, &a1);
        s_x0[tid] = x0;
        s_a[tid] = a0 | (a1 << 16);
    }
    __syncthreads();

    const NvMat m = NV_MAT[f.matrix];
    const long long plane = (long long)H * W;
    TO* fout = out + (long long)blockIdx.y * 3 * plane;
    const int xl = threadIdx.x * 4, xc = col0 + xl;
    if (xc >= W) return;
    for (int k = 0; k < NV_ROWS / 4; ++k) {
        const int y = band * NV_ROWS + threadIdx.y + 4 * k;
        if (y >= H) break;
        const int ry = y - f.top;
        const bool row_in = ry >= 0 && ry < f.rh;
        const unsigned char *r0 = nullptr, *r1 = nullptr, *c0 = nullptr, *c1 = nullptr;   // luma rows (region column 0), chroma rows
        int b0 = 0, b1 = 0;
        bool one_crow = true;
        if (row_in) {
            int ya = ry, yb = ry;
            if (f.resize) {
                resize_coef(ry, f.sy, f.th, &ya, &b0, &b1);
                yb = ya + 1 < f.th ? ya + 1 : f.th - 1;
            }
            r0 = f.y + (long long)ya * f.pitch_y;
            r1 = f.y + (long long)yb * f.pitch_y;
            const int ca = (f.y0 + ya) >> 1, cb = (f.y0 + yb) >> 1;
            c0 = f.uv + (long long)ca * f.pitch_uv;
            c1 = f.uv + (long long)cb * f.pitch_uv;
            one_crow = ca == cb;
        }
        TO v[3][4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int rx = xc + p - f.left;
            int bgr[3] = {114, 114, 114};
            if (row_in && rx >= 0 && rx < f.rw) {
                if (!f.resize) {
                    bgr_of(r0[rx], chroma_of(ld16(c0 + ((f.x0 + rx) >> 1) * 2), m), m, bgr);
                } else {
                    const int x0 = s_x0[xl + p], a = s_a[xl + p];
                    const int a0 = a & 0xffff, a1 = a >> 16;
                    const int x1 = x0 + 1 < f.tw ? x0 + 1 : f.tw - 1;
                    const int q0 = ((f.x0 + x0) >> 1) * 2, q1 = ((f.x0 + x1) >> 1) * 2;     // byte offsets of the two chroma sites
                    const Chroma ch00 = chroma_of(ld16(c0 + q0), m);
                    const Chroma ch01 = q1 == q0 ? ch00 : chroma_of(ld16(c0 + q1), m);
                    Chroma ch10 = ch00, ch11 = ch01;
                    if (!one_crow) {
                        ch10 = chroma_of(ld16(c1 + q0), m);
                        ch11 = q1 == q0 ? ch10 : chroma_of(ld16(c1 + q1), m);
                    }
                    int t00[3], t01[3], t10[3], t11[3];
                    bgr_of(r0[x0], ch00, m, t00);
                    bgr_of(r0[x1], ch01, m, t01);
                    bgr_of(r1[x0], ch10, m, t10);
                    bgr_of(r1[x1], ch11, m, t11);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int h0v = t00[c] * a0 + t01[c] * a1;   // HResizeLinear (scaled by 2048)
                        const int h1v = t10[c] * a0 + t11[c] * a1;
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

// grid (ceil(most units of a frame of this launch / 256), frames of this launch), block (256).  Unit u of a frame = 8 pixels x 2
// rows: row pair u / upr, pixels 8 (u % upr) .. of it, upr = ceil(w0 / 8).
__global__ __launch_bounds__(256) void nv12_to_bgr_kernel(const CvTable tab) {
    const CvEntry& f = tab.f[blockIdx.y];
    const unsigned upr = (unsigned)(f.w0 + 7) >> 3;
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    const unsigned rp = u / upr;
    if (rp >= (unsigned)(f.h0 >> 1)) return;
    const int gx = (int)(u - rp * upr) * 8;
    const int npx = f.w0 - gx < 8 ? f.w0 - gx : 8;                      // 8, or an even tail
    const NvMat m = NV_MAT[f.matrix];
    const unsigned char* ya = f.y + (long long)(2 * rp) * f.pitch_y + gx;
    const unsigned char* yb = ya + f.pitch_y;
    const unsigned char* cp = f.uv + (long long)rp * f.pitch_uv + gx;
    const bool full = npx == 8;
    unsigned yw[2][2] = {{0u, 0u}, {0u, 0u}}, cw[2] = {0u, 0u};        // byte k of a row = pixel k
    if (full && (f.flags & 1)) {
        const uint2 a = *reinterpret_cast<const uint2*>(ya), b = *reinterpret_cast<const uint2*>(yb);
        yw[0][0] = a.x; yw[0][1] = a.y; yw[1][0] = b.x; yw[1][1] = b.y;
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < npx) {
                yw[0][k >> 2] |= (unsigned)ya[k] << (8 * (k & 3));
                yw[1][k >> 2] |= (unsigned)yb[k] << (8 * (k & 3));
            }
    }
    if (full && (f.flags & 2)) {
        const uint2 c = *reinterpret_cast<const uint2*>(cp);
        cw[0] = c.x; cw[1] = c.y;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (2 * k < npx) cw[k >> 1] |= ld16(cp + 2 * k) << (16 * (k & 1));
    }
    unsigned ow[2][6] = {{0u, 0u, 0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u, 0u, 0u}};     // 24 output bytes of each row
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const Chroma ch = chroma_of((cw[q >> 1] >> (16 * (q & 1))) & 0xffffu, m);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int k = 2 * q + s;
                int bgr[3];
                bgr_of((int)((yw[r][k >> 2] >> (8 * (k & 3))) & 255u), ch, m, bgr);
#pragma unroll
                for (int c = 0; c < 3; ++c) ow[r][(3 * k + c) >> 2] |= (unsigned)bgr[c] << (8 * ((3 * k + c) & 3));
            }
    }
    unsigned char* oa = f.out + ((long long)(2 * rp) * f.w0 + gx) * 3;
    unsigned char* ob = oa + (long long)f.w0 * 3;
    if (full && (f.flags & 4)) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            reinterpret_cast<uint2*>(oa)[j] = make_uint2(ow[0][2 * j], ow[0][2 * j + 1]);
            reinterpret_cast<uint2*>(ob)[j] = make_uint2(ow[1][2 * j], ow[1][2 * j + 1]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 24; ++i)
            if (i < 3 * npx) {
                oa[i] = (unsigned char)(ow[0][i >> 2] >> (8 * (i & 3)));
                ob[i] = (unsigned char)(ow[1][i >> 2] >> (8 * (i & 3)));
            }
    }
}

template <typename TO>
int launch_nv12_letterbox(const NvTable& tab, int nf, void* out, int H, int W, bool vec, hipStream_t st) {
    const int n_ctiles = ceil_div(W, NV_COLS), n_bands = ceil_div(H, NV_ROWS);
    const dim3 grid((unsigned)(n_ctiles * n_bands), (unsigned)nf), block(64, 4);
    if (vec) hipLaunchKernelGGL((nv12_letterbox_kernel<TO, true>), grid, block, 0, st, tab, (TO*)out, H, W, n_ctiles);
    else hipLaunchKernelGGL((nv12_letterbox_kernel<TO, false>), grid, block, 0, st, tab, (TO*)out, H, W, n_ctiles);
    LP_HIP_CHECK(hipGetLastError());
    return LP_OK;
}

// The plane rules shared by both entry points; an empty string: fine.
std::string plane_fault(const unsigned char* y, const unsigned char* uv, int pitch_y, int pitch_uv, int h0, int w0, int matrix) {
    if (!y || !uv) return "null plane";
    if (h0 < 2 || w0 < 2 || (h0 & 1) || (w0 & 1)) return "frame size must be even and >= 2";
    if (pitch_y < w0) return "pitch_y < w0";
    if (pitch_uv < w0 || (pitch_uv & 1)) return "pitch_uv must be even and >= w0";
    if ((uintptr_t)uv & 1) return "uv must be 2-byte aligned";
    if (matrix < 0 || matrix >= NV_MATRICES) return "unknown matrix";
    return "";
}

}  // namespace

}  // namespace lp

using namespace lp;

extern "C" int lp_preprocess_nv12_batch(const lp_nv12_desc* desc, int n, int B, void* out, int out_dtype, int H, int W, void* stream) {
    const std::string fn = "lp_preprocess_nv12_batch: ";
    if (out_dtype != LP_F16 && out_dtype != LP_BF16 && out_dtype != LP_F32) return fail(LP_ERR_ARG, fn + "dtype");
    if (!out || B < 1 || n < 0 || n > B || (n > 0 && !desc) || H < 1 || W < 1 ||
        (long long)ceil_div(H, NV_ROWS) * ceil_div(W, NV_COLS) > 0x7fffffffLL)
        return fail(LP_ERR_ARG, fn + "bad arguments (need out, 0 <= n <= B, B >= 1, H, W >= 1)");
    for (int b = 0; b < n; ++b) {              // every entry is checked before the first launch
        const lp_nv12_desc& d = desc[b];
        const std::string why = plane_fault(d.y, d.uv, d.pitch_y, d.pitch_uv, d.h0, d.w0, d.matrix);
        if (!why.empty()) return fail(LP_ERR_ARG, fn + why + " (entry " + std::to_string(b) + ")");
        if (d.y0 < 0 || d.x0 < 0 || d.th < 1 || d.tw < 1 || d.th > d.h0 - d.y0 || d.tw > d.w0 - d.x0)
            return fail(LP_ERR_ARG, fn + "region of entry " + std::to_string(b) + " is not inside its frame");
        if (d.rh < 1 || d.rw < 1 || d.top < 0 || d.left < 0 || d.top + d.rh > H || d.left + d.rw > W)
            return fail(LP_ERR_ARG, fn + "bad geometry of entry " + std::to_string(b));
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t esz = dtype_size(out_dtype);
    const bool vec = W % 4 == 0 && ((uintptr_t)out & 15) == 0;
    for (int b0 = 0; b0 < B; b0 += LP_NV12_PER_LAUNCH) {
        const int nf = B - b0 < LP_NV12_PER_LAUNCH ? B - b0 : LP_NV12_PER_LAUNCH;
        NvTable tab = {};
        for (int j = 0; j < nf; ++j) {
            NvEntry& e = tab.f[j];
            if (b0 + j < n) {
                const lp_nv12_desc& d = desc[b0 + j];
                e.y = d.y + (long long)d.y0 * d.pitch_y + d.x0;
                e.uv = d.uv;
                e.pitch_y = d.pitch_y; e.pitch_uv = d.pitch_uv;
                e.y0 = d.y0; e.x0 = d.x0; e.th = d.th; e.tw = d.tw;
                e.rh = d.rh; e.rw = d.rw; e.top = d.top; e.left = d.left;
                e.resize = !(d.rh == d.th && d.rw == d.tw);
                e.matrix = d.matrix;
                e.sy = (double)d.th / d.rh;
                e.sx = (double)d.tw / d.rw;
            }                                   // else: zero entry = a padding slot (rh = rw = 0: every pixel is 114)
        }
        void* o = (char*)out + (size_t)b0 * 3 * H * W * esz;
        int rc = LP_OK;
        switch (out_dtype) {
            case LP_F16: rc = launch_nv12_letterbox<f16>(tab, nf, o, H, W, vec, st); break;
            case LP_BF16: rc = launch_nv12_letterbox<bf16>(tab, nf, o, H, W, vec, st); break;
            default: rc = launch_nv12_letterbox<float>(tab, nf, o, H, W, vec, st); break;
        }
        if (rc != LP_OK) return rc;
    }
    return LP_OK;
}

extern "C" int lp_nv12_to_bgr_batch(const lp_nv12_bgr_desc* desc, int n, void* stream) {
    const std::string fn = "lp_nv12_to_bgr_batch: ";
    if (n < 0 || (n > 0 && !desc)) return fail(LP_ERR_ARG, fn + "bad arguments (need n >= 0 and desc)");
    for (int b = 0; b < n; ++b) {              // every entry is checked before the first launch
        const lp_nv12_bgr_desc& d = desc[b];
        std::string why = plane_fault(d.y, d.uv, d.pitch_y, d.pitch_uv, d.h0, d.w0, d.matrix);
        if (why.empty() && !d.out) why = "null out";
        if (why.empty() && (long long)ceil_div(d.w0, 8) * (d.h0 / 2) > 0x7fffffffLL) why = "frame too large";
        if (!why.empty()) return fail(LP_ERR_ARG, fn + why + " (entry " + std::to_string(b) + ")");
    }
    hipStream_t st = (hipStream_t)stream;
    for (int b0 = 0; b0 < n; b0 += LP_FRAMES_PER_LAUNCH) {
        const int nf = n - b0 < LP_FRAMES_PER_LAUNCH ? n - b0 : LP_FRAMES_PER_LAUNCH;
        CvTable tab = {};
        long long most = 1;
        for (int j = 0; j < nf; ++j) {
            const lp_nv12_bgr_desc& d = desc[b0 + j];
            CvEntry& e = tab.f[j];
            e.y = d.y; e.uv = d.uv; e.out = d.out;
            e.pitch_y = d.pitch_y; e.pitch_uv = d.pitch_uv; e.h0 = d.h0; e.w0 = d.w0;
            e.matrix = d.matrix;
            e.flags = ((((uintptr_t)d.y | (uintptr_t)d.pitch_y) & 7) == 0 ? 1 : 0) |
                      ((((uintptr_t)d.uv | (uintptr_t)d.pitch_uv) & 7) == 0 ? 2 : 0) |
                      ((((uintptr_t)d.out & 7) == 0 && d.w0 % 8 == 0) ? 4 : 0);
            const long long units = (long long)ceil_div(d.w0, 8) * (d.h0 / 2);
            most = units > most ? units : most;
        }
        hipLaunchKernelGGL(nv12_to_bgr_kernel, dim3((unsigned)((most + 255) / 256), (unsigned)nf), dim3(256), 0, st, tab);
        LP_HIP_CHECK(hipGetLastError());
    }
    return LP_OK;
}
