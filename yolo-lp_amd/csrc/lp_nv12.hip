// NV12 video frames to BGR: lp_nv12_to_bgr_batch (include/lp_hip.h), and the plane rules it shares with lp_preprocess_nv12_batch
// (lp_frames.hip: the letterbox reads NV12 planes through its own pixel source).  The reference has nothing here (its Inferer
// takes what cv2 decodes, BGR); the written-down specification is yolov6/utils/nv12.py (nv12_to_bgr_np), which the kernel matches
// bit for bit (tests/test_nv12_gpu.py).  The colour rule itself is lp_nv12_color.inc.
//
// nv12_to_bgr_kernel streams: a lane owns 8 pixels x 2 rows = one 8-byte UV load (4 pairs), two 8-byte Y loads, two 24-byte
// runs of output.  Vector loads / stores where the plane's base and pitch (the output's base and row length) are 8-byte
// aligned; byte accesses otherwise and for a row's tail of 2, 4 or 6 pixels.
//
// Descriptors travel by value in the kernel arguments (nothing uploaded, no host sync, capturable): 48 bytes x 64 per launch.
#include "lp_internal.h"

namespace lp {

namespace {

#include "lp_nv12_color.inc"

struct CvEntry {
    const unsigned char* y;
    const unsigned char* uv;
    unsigned char* out;
    int pitch_y, pitch_uv, h0, w0;
    int matrix, flags;                  // flags: 1 = 8-byte Y loads, 2 = 8-byte UV loads, 4 = 8-byte stores
};
struct CvTable { CvEntry f[LP_FRAMES_PER_LAUNCH]; };

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

}  // namespace

// The plane rules shared by both NV12 entry points (lp_internal.h); an empty string: fine.
std::string plane_fault(const unsigned char* y, const unsigned char* uv, int pitch_y, int pitch_uv, int h0, int w0, int matrix) {
    if (!y || !uv) return "null plane";
    if (h0 < 2 || w0 < 2 || (h0 & 1) || (w0 & 1)) return "frame size must be even and >= 2";
    if (pitch_y < w0) return "pitch_y < w0";
    if (pitch_uv < w0 || (pitch_uv & 1)) return "pitch_uv must be even and >= w0";
    if ((uintptr_t)uv & 1) return "uv must be 2-byte aligned";
    if (matrix < 0 || matrix >= NV_MATRICES) return "unknown matrix";
    return "";
}

}  // namespace lp

using namespace lp;

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
