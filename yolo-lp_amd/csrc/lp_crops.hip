// Perspective-rectified plate crops: lp_plate_crops_batch (include/lp_hip.h).  Every detection row of a frame is cut out of
// the device frame as an upright crop_h x crop_w BGR image, along its four predicted corners (columns 4..11, label order
// TL, BL, BR, TR; reference data/transCCPD.py:128, yolov6/utils/general.py:45-50) or, when they do not form a usable quad,
// along its box.  This is the inverse of the warp the reference's plate generator applies (yolov6/data/generate/generate.py).
//
// The semantics are stated once, in fp64 geometry and an fp32 blend, and restated by the numpy mirror
// yolov6/utils/plate_crop.py::plate_crops_np in the same operation order; with -ffp-contract=off and no fast-math or
// reciprocal intrinsics the two agree bit for bit (tests/test_plate_crops_gpu.py).
//
// Descriptors are passed by value as a kernel-argument table (at most 64 entries), as in lp_frames.hip: nothing is uploaded,
// and the call is safe under graph capture.  The detection counts are read on the device.
#include <algorithm>
#include <utility>
#include <vector>

#include "lp_internal.h"

namespace lp {

namespace {

constexpr int CR_COLS = 64;             // output columns of one workgroup (one per lane)
constexpr int CR_ROWS = 16;             // output rows of one workgroup (4 waves x 4 rows)
constexpr int CR_MAX_SIDE = 1024;
constexpr int CR_MAX_GRID_Y = 65535;    // crops of one frame per launch row; larger counts loop

struct CrEntry {
    const unsigned char* img;
    int h0, w0, max_crops, out_slot;
};
struct CrTable { CrEntry f[LP_FRAMES_PER_LAUNCH]; };

// The square-to-quad projective map (Heckbert): (u, v) -> ((a u + b v + c) / w, (d u + e v + f) / w), w = g u + h v + 1,
// with (0,0) -> p0, (1,0) -> p1, (1,1) -> p2, (0,1) -> p3.
struct QuadMap { double a, b, c, d, e, f, g, h; };

__device__ __forceinline__ QuadMap square_to_quad(const double x[4], const double y[4]) {
    const double sx = x[0] - x[1] + x[2] - x[3], sy = y[0] - y[1] + y[2] - y[3];
    const double dx1 = x[1] - x[2], dx2 = x[3] - x[2], dy1 = y[1] - y[2], dy2 = y[3] - y[2];
    const double den = dx1 * dy2 - dx2 * dy1;
    QuadMap m;
    m.g = (sx * dy2 - dx2 * sy) / den;
    m.h = (dx1 * sy - sx * dy1) / den;
    m.a = x[1] - x[0] + m.g * x[1];
    m.b = x[3] - x[0] + m.h * x[3];
    m.c = x[0];
    m.d = y[1] - y[0] + m.g * y[1];
    m.e = y[3] - y[0] + m.h * y[3];
    m.f = y[0];
    return m;
}

#include "lp_plate_quad.inc"   // finite4, plate_quad: the quad a row describes, shared with lp_redact.hip

// Source coordinate of one axis: clamp(P - 0.5, 0, n - 1) (a NaN goes to 0) -> first tap, second tap, fraction.
__device__ __forceinline__ void src_axis(double p, int n, int* t0, int* t1, float* fr) {
    double s = p - 0.5;
    s = s >= 0.0 ? s : 0.0;
    s = s < (double)(n - 1) ? s : (double)(n - 1);
    const double fl = floor(s);
    int i = (int)fl;
    i = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);    // already in range: keeps every gather inside the frame whatever the input
    *t0 = i;
    *t1 = i + 1 < n ? i + 1 : n - 1;
    *fr = (float)(s - fl);
}

// grid (column tiles x row bands, crops of a frame (looped past 65535), frames of this launch), block (64, 4).  Lane x owns
// output column ct * 64 + x; wave y owns rows y, y+4, y+8, y+12 of the band.  The quad and its map are computed by every
// lane (a few dozen fp64 operations, once per workgroup); the workgroup of tile 0, band 0 writes the slot's status.
__global__ __launch_bounds__(256) void plate_crops_kernel(const CrTable tab, const float* __restrict__ det, const int32_t* __restrict__ count,
                                                          int max_det, unsigned char* __restrict__ out, int32_t* __restrict__ status,
                                                          int crop_h, int crop_w, int n_ctiles) {
    const CrEntry& fr = tab.f[blockIdx.z];
    int n = count[blockIdx.z];
    const int lim = fr.max_crops < max_det ? fr.max_crops : max_det;
    n = n < 0 ? 0 : (n > lim ? lim : n);
    const int ct = blockIdx.x % n_ctiles, band = blockIdx.x / n_ctiles;
    const bool writer = blockIdx.x == 0 && threadIdx.x == 0 && threadIdx.y == 0;
    const int j = ct * CR_COLS + threadIdx.x;
    for (int r = blockIdx.y; r < fr.max_crops; r += gridDim.y) {
        const long long slot = (long long)fr.out_slot + r;
        if (r >= n) {
            if (writer) status[slot] = 0;
            continue;
        }
        const float* row = det + ((long long)blockIdx.z * max_det + r) * LP_DET_COLS;
        double qx[4], qy[4];
        const int st = plate_quad(row, qx, qy);
        if (writer) status[slot] = st;
        if (j >= crop_w) continue;
        const QuadMap m = square_to_quad(qx, qy);
        const double u = ((double)j + 0.5) / (double)crop_w;
        unsigned char* obase = out + slot * crop_h * crop_w * 3 + (long long)j * 3;
        for (int k = 0; k < CR_ROWS / 4; ++k) {
            const int i = band * CR_ROWS + threadIdx.y + 4 * k;
            if (i >= crop_h) break;
            unsigned char* o = obase + (long long)i * crop_w * 3;
            if (st == 3) {
                o[0] = 0; o[1] = 0; o[2] = 0;
                continue;
            }
            const double v = ((double)i + 0.5) / (double)crop_h;
            const double w = m.g * u + m.h * v + 1.0;
            const double X = (m.a * u + m.b * v + m.c) / w;
            const double Y = (m.d * u + m.e * v + m.f) / w;
            int x0, x1, y0, y1;
            float fx, fy;
            src_axis(X, fr.w0, &x0, &x1, &fx);
            src_axis(Y, fr.h0, &y0, &y1, &fy);
            const unsigned char* r0 = fr.img + (long long)y0 * fr.w0 * 3;
            const unsigned char* r1 = fr.img + (long long)y1 * fr.w0 * 3;
            const long long c0 = (long long)x0 * 3, c1 = (long long)x1 * 3;
            const float gx = 1.f - fx, gy = 1.f - fy;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float p00 = r0[c0 + c], p01 = r0[c1 + c];
                const float p10 = r1[c0 + c], p11 = r1[c1 + c];
                const float val = gy * (gx * p00 + fx * p01) + fy * (gx * p10 + fx * p11);
                float q = rintf(val);
                q = q < 0.f ? 0.f : (q > 255.f ? 255.f : q);
                o[c] = (unsigned char)q;
            }
        }
    }
}

}  // namespace

}  // namespace lp

using namespace lp;

extern "C" int lp_plate_crops_batch(const lp_crop_desc* desc, int n_frames, const float* det, const int32_t* count, int max_det,
                                    unsigned char* out, int32_t* status, int n_slots, int crop_h, int crop_w, void* stream) {
    const char* fn = "lp_plate_crops_batch: ";
    if (n_frames < 0 || (n_frames > 0 && !desc) || max_det < 0 || n_slots < 0)
        return fail(LP_ERR_ARG, std::string(fn) + "bad arguments (need desc, n_frames >= 0, max_det >= 0, n_slots >= 0)");
    if (crop_h < 1 || crop_w < 1 || crop_h > CR_MAX_SIDE || crop_w > CR_MAX_SIDE)
        return fail(LP_ERR_ARG, std::string(fn) + "crop size " + std::to_string(crop_h) + "x" + std::to_string(crop_w) +
                                    " (need 1..1024 on each side)");
    std::vector<std::pair<int, int>> ranges;   // (out_slot, frame) of every frame with slots
    for (int b = 0; b < n_frames; ++b) {       // all checked before any launch
        const lp_crop_desc& d = desc[b];
        if (!d.img || d.h0 < 1 || d.w0 < 1 || d.max_crops < 0 || d.out_slot < 0 || (long long)d.out_slot + d.max_crops > n_slots)
            return fail(LP_ERR_ARG, std::string(fn) + "bad descriptor of frame " + std::to_string(b) +
                                        " (need img, h0, w0 >= 1, max_crops, out_slot >= 0, out_slot + max_crops <= n_slots)");
        if (d.max_crops > 0) ranges.push_back({d.out_slot, b});
    }
    if (ranges.empty()) return LP_OK;          // nothing to write
    std::sort(ranges.begin(), ranges.end());
    for (size_t k = 1; k < ranges.size(); ++k) {
        const lp_crop_desc& p = desc[ranges[k - 1].second];
        if (p.out_slot + p.max_crops > ranges[k].first)
            return fail(LP_ERR_ARG, std::string(fn) + "slot ranges of frames " + std::to_string(ranges[k - 1].second) + " and " +
                                        std::to_string(ranges[k].second) + " overlap");
    }
    if (!det || !count || !out || !status) return fail(LP_ERR_ARG, std::string(fn) + "null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int n_ctiles = ceil_div(crop_w, CR_COLS), n_bands = ceil_div(crop_h, CR_ROWS);
    for (int b0 = 0; b0 < n_frames; b0 += LP_FRAMES_PER_LAUNCH) {
        const int nf = n_frames - b0 < LP_FRAMES_PER_LAUNCH ? n_frames - b0 : LP_FRAMES_PER_LAUNCH;
        CrTable tab = {};
        int most = 0;
        for (int j = 0; j < nf; ++j) {
            const lp_crop_desc& d = desc[b0 + j];
            tab.f[j] = {d.img, d.h0, d.w0, d.max_crops, d.out_slot};
            most = d.max_crops > most ? d.max_crops : most;
        }
        if (most == 0) continue;
        const dim3 grid((unsigned)(n_ctiles * n_bands), (unsigned)(most < CR_MAX_GRID_Y ? most : CR_MAX_GRID_Y), (unsigned)nf);
        hipLaunchKernelGGL(plate_crops_kernel, grid, dim3(64, 4), 0, st, tab, det + (size_t)b0 * max_det * LP_DET_COLS, count + b0,
                           max_det, out, status, crop_h, crop_w, n_ctiles);
        LP_HIP_CHECK(hipGetLastError());
    }
    return LP_OK;
}
