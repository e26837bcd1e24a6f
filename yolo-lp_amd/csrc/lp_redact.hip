// Plate redaction in place: lp_redact_plates_batch (include/lp_hip.h).  Every detection row of a frame makes the pixels of its
// (expanded) quad unreadable, by a mosaic anchored to the frame or by a fill, in a BGR frame or in the two planes of an NV12 frame.
// The reference has nothing here; the written-down specification is yolov6/utils/redact.py::redact_plates_np, in the same
// operation order: fp64 geometry (no fused multiply-add: -ffp-contract=off) and integer means, so the two agree bit for bit
// (tests/test_redact_gpu.py).  The quad of a row is the rule of the crops, lp_plate_quad.inc.
//
// An in-place mosaic has a read-after-write hazard: a cell's mean must not see bytes another plate's workgroup has already
// replaced.  It is removed by the structure, not by atomics or ordering: redact_means_kernel only reads the frames and writes,
// for every cell the bounding rectangle of a row touches, one packed entry into the workspace (an entry depends on the frame alone,
// so two plates touching one cell store the same word); redact_write_kernel, launched behind it, only reads det, count and those
// entries and writes the frames.  Every means launch of a call precedes its first write launch.  Fill is the second kernel alone.
//
// Both are ONE kernel each over two pixel sinks: BgrSink (3 interleaved bytes per pixel, any alignment) and Nv12Sink (a luma
// byte, and the U, V pair of the pixel's 2 x 2 block as one aligned 16-bit access).  A sink supplies a lane's share of a cell's
// sums, the sample count of its second and third channel, and the store of one pixel; the units, the geometry, the inside test,
// the reduction and the cell table are the kernels'.
//
// lp_redact_gauss_batch is the third redaction, a Gaussian blur, with the same hazard and the same cure: redact_gauss_kernel only
// reads the frames and writes, for every frame-anchored GS_TILE x GS_TILE tile that the rectangle of a row touches, the blurred
// value of each of its pixels into a per-pixel table (the mosaic's table at cell 1; a value depends on the frame alone, so a tile
// that two plates touch is written twice with the same words); redact_write_kernel serves unchanged with cell = 1.  One workgroup
// blurs one tile: the tile and its halo go through LDS once (clamped coordinates: the replicate border), the horizontal pass fills
// a 16-bit LDS array, the vertical pass reads it; integers only, the taps are data in the kernel arguments.
//
// The size of a plate is device data, so the launch shape cannot follow it: per frame RD_WGS workgroups loop over the units
// (row r, split s), r < n_b, s < RD_SPLIT -- a frame without plates costs its workgroups one load of the count.  Descriptors
// travel by value in the kernel arguments (40 bytes x 64): nothing is uploaded, no host sync, capturable in a graph.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <vector>

#include "lp_internal.h"

namespace lp {

namespace {

#include "lp_plate_quad.inc"

constexpr int RD_WGS = 32;              // workgroups per frame (grid.x)
constexpr int RD_SPLIT = 8;             // units per row: unit (r, s) owns the pixel rows (cells) 4 s + wave, + 32, ... of the rectangle

struct RdEntry {
    unsigned char* p0;                  // BGR: the frame; NV12: the luma plane
    unsigned char* p1;                  // NV12: the chroma plane
    int pitch0, pitch1, h0, w0;
    long long ws_off;                   // first entry of the frame's cell table in the workspace
};
struct RdTable { RdEntry f[LP_FRAMES_PER_LAUNCH]; };
static_assert(sizeof(RdTable) < 4096, "the table travels as kernel arguments: under 4 KiB");

// ---- the blur of lp_redact_gauss_batch -------------------------------------------------------------------------------------
constexpr int GS_TILE = 32;             // side of a blur tile in pixels (even: an NV12 tile is whole 2 x 2 blocks)
constexpr int GS_OUT_BYTES = GS_TILE * GS_TILE * 3;      // LDS: the blurred bytes of a tile (BGR: 3 per pixel; NV12: Y, then UV)

constexpr int GS_GROUP = 4;             // adjacent outputs of a pass that one thread computes from one sliding run of samples
constexpr int GS_LOADS = 8;             // global byte loads a thread issues back to back while a tile is staged
constexpr int GS_WINDOW = 2 * LP_REDACT_MAX_RADIUS + 1 + 2 * (GS_GROUP - 1);

// The taps as the passes read them, by value in the kernel arguments: the whole window t[|i - R|], i = 0..2R, widened to int, with
// GS_GROUP - 1 zeros on either side, so that sample m of a run weighs w[m - j + GS_GROUP - 1] for output j, in or out of its window.
struct GsTaps {
    int r, rc;
    int w[GS_WINDOW], wc[GS_WINDOW];
};
static_assert(sizeof(RdTable) + sizeof(GsTaps) < 4096, "table and taps travel as kernel arguments: under 4 KiB");

// LDS of one tile of a plane of C interleaved channels at radius R: the staged bytes and the 16-bit horizontal sums
constexpr int gs_in_bytes(int tile, int R, int C) { return (tile + 2 * R) * (tile + 2 * R) * C; }
constexpr int gs_hq_bytes(int tile, int R, int C) { return (tile + 2 * R) * tile * C * 2; }

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Blur the tile [y0, y0 + th) x [x0, x0 + tw) of a ph x pw plane of C interleaved byte channels (rows `pitch` bytes apart) into
// out[th][tw * C], all 256 threads of the workgroup.  in: (th + 2R) x (tw + 2R) x C bytes, hq: (th + 2R) x tw x C shorts.
//   1. stage: the bytes of the tile + halo in row-major order, adjacent threads adjacent bytes, GS_LOADS loads in flight per thread
//      (the byte loads are latency, not bandwidth); coordinates clamped to the plane, so every frame byte is loaded once per tile
//      and the passes need no border case
//   2. horizontal: hq = (sum_k t[|k|] * in[.][x + k * C] + 32) >> 6 for every staged row (the halo rows feed the vertical pass)
//   3. vertical: out = (sum_k t[|k|] * hq[i + k][x] + 2^21) >> 22
// In both passes a thread computes GS_GROUP adjacent outputs along the pass's direction from one run of 2R + GS_GROUP samples, each
// read from LDS once, a quarter of the reads of a tap-by-tap loop.  Past a clipped tile's edge a run reads
// up to GS_GROUP - 1 samples of the next row (still inside the array as it is sized for a whole tile); they reach only outputs
// that are not stored.  The sums are int32 (at most 16384 * 255 and 16384 * 65280 < 2^31; their order is free); a tap and a
// sample are below 2^24, so the products are 24-bit multiplies (full rate).  Ends behind a barrier: out is readable, in and hq are free.
template <int C>
__device__ __forceinline__ void blur_plane(const unsigned char* __restrict__ src, int pitch, int ph, int pw, int y0, int x0, int th, int tw,
                                           int R, const int* __restrict__ win, unsigned char* in, unsigned short* hq,
                                           unsigned char* out) {
    static_assert(GS_GROUP == 4 && GS_TILE % GS_GROUP == 0, "the passes are written for runs of four");
    const int tid = threadIdx.y * 64 + threadIdx.x;
    const int ih = th + 2 * R, irow = (tw + 2 * R) * C, orow = tw * C, run = 2 * R + GS_GROUP;
    for (int p0 = tid; p0 < ih * irow; p0 += 256 * GS_LOADS) {
        unsigned char v[GS_LOADS];
#pragma unroll
        for (int u = 0; u < GS_LOADS; ++u) {       // all loads of a batch are issued before the first is used
            const int p = p0 + 256 * u < ih * irow ? p0 + 256 * u : p0;
            const int r = p / irow, b = p - r * irow, c = b / C;
            v[u] = src[(long long)clampi(y0 - R + r, ph - 1) * pitch + (long long)clampi(x0 - R + c, pw - 1) * C + (b - c * C)];
        }
#pragma unroll
        for (int u = 0; u < GS_LOADS; ++u)
            if (p0 + 256 * u < ih * irow) in[p0 + 256 * u] = v[u];
    }
    __syncthreads();
    const int ngx = (tw + GS_GROUP - 1) / GS_GROUP * C;      // runs per staged row: a group of pixels x a channel
    for (int p = tid; p < ih * ngx; p += 256) {
        const int r = p / ngx, gi = p - r * ngx, pg = gi / C, ch = gi - pg * C;
        const unsigned char* q = in + r * irow + pg * (GS_GROUP * C) + ch;
        int acc[GS_GROUP] = {0, 0, 0, 0};
        for (int m = 0; m < run; ++m) {
            const int v = q[m * C];
#pragma unroll
            for (int j = 0; j < GS_GROUP; ++j) acc[j] += __mul24(win[m - j + GS_GROUP - 1], v);
        }
        unsigned short* o = hq + r * orow + pg * (GS_GROUP * C) + ch;
#pragma unroll
        for (int j = 0; j < GS_GROUP; ++j)
            if (pg * GS_GROUP + j < tw) o[j * C] = (unsigned short)((acc[j] + 32) >> 6);
    }
    __syncthreads();
    for (int p = tid; p < (th + GS_GROUP - 1) / GS_GROUP * orow; p += 256) {
        const int g = p / orow, x = p - g * orow;
        const unsigned short* q = hq + g * (GS_GROUP * orow) + x;
        int acc[GS_GROUP] = {0, 0, 0, 0};
        for (int m = 0; m < run; ++m) {
            const int v = q[m * orow];
#pragma unroll
            for (int j = 0; j < GS_GROUP; ++j) acc[j] += __mul24(win[m - j + GS_GROUP - 1], v);
        }
#pragma unroll
        for (int j = 0; j < GS_GROUP; ++j)
            if (g * GS_GROUP + j < th) out[(g * GS_GROUP + j) * orow + x] = (unsigned char)((acc[j] + (1 << 21)) >> 22);
    }
    __syncthreads();
}

struct BgrSink {
    // this lane's share of the channel sums over the pixels [ya, yb) x [xa, xb) of one cell, lanes along the cell's rows
    static __device__ __forceinline__ void gather(const RdEntry& f, int ya, int yb, int xa, int xb, int lane, int* acc) {
        const int cw = xb - xa, n = (yb - ya) * cw;
        for (int p = lane; p < n; p += 64) {
            const int r = p / cw, c = p - r * cw;
            const unsigned char* q = f.p0 + (long long)(ya + r) * f.pitch0 + (long long)(xa + c) * 3;
            acc[0] += q[0]; acc[1] += q[1]; acc[2] += q[2];
        }
    }
    static __device__ __forceinline__ int chroma_count(int n) { return n; }      // samples of channels 1, 2 in a cell of n pixels
    static __device__ __forceinline__ void put(const RdEntry& f, int i, int j, unsigned v) {
        unsigned char* q = f.p0 + (long long)i * f.pitch0 + (long long)j * 3;
        q[0] = (unsigned char)v; q[1] = (unsigned char)(v >> 8); q[2] = (unsigned char)(v >> 16);
    }
    // LDS bytes of the staged tile and of its horizontal sums at these radii
    static int gauss_in_bytes(int R, int) { return gs_in_bytes(GS_TILE, R, 3); }
    static int gauss_hq_bytes(int R, int) { return gs_hq_bytes(GS_TILE, R, 3); }
    // the table entries (b, g, r) of the tile [y0, y0 + th) x [x0, x0 + tw)
    static __device__ __forceinline__ void gauss_tile(const RdEntry& f, const GsTaps& tp, int y0, int x0, int th, int tw,
                                                      unsigned char* in, unsigned short* hq, unsigned char* out, unsigned* table) {
        blur_plane<3>(f.p0, f.pitch0, f.h0, f.w0, y0, x0, th, tw, tp.r, tp.w, in, hq, out);
        for (int p = threadIdx.y * 64 + threadIdx.x; p < th * tw; p += 256) {
            const int i = p / tw, j = p - i * tw;
            table[(long long)(y0 + i) * f.w0 + x0 + j] = (unsigned)out[3 * p] | ((unsigned)out[3 * p + 1] << 8) | ((unsigned)out[3 * p + 2] << 16);
        }
    }
};

// h0, w0 and the cell are even, so a clipped luma cell [ya, yb) x [xa, xb) is whole 2 x 2 blocks: its chroma cell is the samples
// [ya/2, yb/2) x [xa/2, xb/2), cell/2 on a side, and both planes share one cell grid.
struct Nv12Sink {
    static __device__ __forceinline__ void gather(const RdEntry& f, int ya, int yb, int xa, int xb, int lane, int* acc) {
        const int cw = xb - xa, n = (yb - ya) * cw;
        for (int p = lane; p < n; p += 64) {
            const int r = p / cw, c = p - r * cw;
            acc[0] += f.p0[(long long)(ya + r) * f.pitch0 + xa + c];
        }
        const int hw = cw >> 1, nc = n >> 2;
        for (int p = lane; p < nc; p += 64) {
            const int r = p / hw, c = p - r * hw;
            const unsigned uv = *reinterpret_cast<const unsigned short*>(f.p1 + (long long)((ya >> 1) + r) * f.pitch1 + ((xa >> 1) + c) * 2);
            acc[1] += (int)(uv & 255u); acc[2] += (int)(uv >> 8);
        }
    }
    static __device__ __forceinline__ int chroma_count(int n) { return n >> 2; }
    // the pixel's luma byte and the chroma pair of its block: up to four pixels of a block store the same pair ("any of four")
    static __device__ __forceinline__ void put(const RdEntry& f, int i, int j, unsigned v) {
        f.p0[(long long)i * f.pitch0 + j] = (unsigned char)v;
        *reinterpret_cast<unsigned short*>(f.p1 + (long long)(i >> 1) * f.pitch1 + (j >> 1) * 2) = (unsigned short)(v >> 8);
    }
    // the two planes are blurred one after the other through the same LDS: Y at radius R, then UV (2 channels, half the tile) at Rc
    static int gauss_in_bytes(int R, int Rc) { return std::max(gs_in_bytes(GS_TILE, R, 1), gs_in_bytes(GS_TILE / 2, Rc, 2)); }
    static int gauss_hq_bytes(int R, int Rc) { return std::max(gs_hq_bytes(GS_TILE, R, 1), gs_hq_bytes(GS_TILE / 2, Rc, 2)); }
    // the table entries (y of the pixel, u and v of its block); y0, x0, th and tw are even, as h0, w0 and GS_TILE are
    static __device__ __forceinline__ void gauss_tile(const RdEntry& f, const GsTaps& tp, int y0, int x0, int th, int tw,
                                                      unsigned char* in, unsigned short* hq, unsigned char* out, unsigned* table) {
        unsigned char* out_uv = out + GS_TILE * GS_TILE;
        blur_plane<1>(f.p0, f.pitch0, f.h0, f.w0, y0, x0, th, tw, tp.r, tp.w, in, hq, out);
        blur_plane<2>(f.p1, f.pitch1, f.h0 >> 1, f.w0 >> 1, y0 >> 1, x0 >> 1, th >> 1, tw >> 1, tp.rc, tp.wc, in, hq, out_uv);
        for (int p = threadIdx.y * 64 + threadIdx.x; p < th * tw; p += 256) {
            const int i = p / tw, j = p - i * tw;
            const unsigned char* uv = out_uv + ((i >> 1) * (tw >> 1) + (j >> 1)) * 2;
            table[(long long)(y0 + i) * f.w0 + x0 + j] = (unsigned)out[p] | ((unsigned)uv[0] << 8) | ((unsigned)uv[1] << 16);
        }
    }
};

struct RdRect { int i0, i1, j0, j1; };

// clamp(v, 0, n) in double (a NaN goes to 0), then converted
__device__ __forceinline__ int clamp_to(double v, int n) {
    v = v >= 0.0 ? v : 0.0;
    v = v < (double)n ? v : (double)n;
    return (int)v;
}

// The expanded quad of one detection row into x[4], y[4] (p0 = TL, p1 = TR, p2 = BR, p3 = BL) and the rectangle its scan is
// bounded by; returns the status of plate_quad (3: x, y, rc are not set).  s = 1 + margin.
__device__ __forceinline__ int redact_quad(const float* row, double s, int h0, int w0, double x[4], double y[4], RdRect* rc) {
    const int st = plate_quad(row, x, y);
    if (st == 3) return st;
    const double cx = 0.25 * (((x[0] + x[1]) + x[2]) + x[3]);
    const double cy = 0.25 * (((y[0] + y[1]) + y[2]) + y[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        x[k] = cx + s * (x[k] - cx);
        y[k] = cy + s * (y[k] - cy);
    }
    const double xlo = fmin(fmin(x[0], x[1]), fmin(x[2], x[3])), xhi = fmax(fmax(x[0], x[1]), fmax(x[2], x[3]));
    const double ylo = fmin(fmin(y[0], y[1]), fmin(y[2], y[3])), yhi = fmax(fmax(y[0], y[1]), fmax(y[2], y[3]));
    rc->j0 = clamp_to(floor(xlo), w0); rc->j1 = clamp_to(ceil(xhi), w0);
    rc->i0 = clamp_to(floor(ylo), h0); rc->i1 = clamp_to(ceil(yhi), h0);
    return st;
}

__device__ __forceinline__ int clamp_count(int n, int max_det) { return n < 0 ? 0 : (n > max_det ? max_det : n); }

// grid (RD_WGS, frames of this launch), block (64, 4).  Unit (r, s): wave y takes the cells 4 s + y, + 32, ... of the cells that the
// row's rectangle touches (row-major); its lanes stride over the clipped cell's pixels, then an integer wave reduction (the order
// of an integer sum is free) and one store by lane 0.  Reads the frames, writes the workspace.
template <typename SINK>
__global__ __launch_bounds__(256) void redact_means_kernel(const RdTable tab, const float* __restrict__ det, const int32_t* __restrict__ count,
                                                           int max_det, double s, int cell, unsigned* __restrict__ ws) {
    const int n = clamp_count(count[blockIdx.y], max_det);
    if (n == 0) return;
    const RdEntry f = tab.f[blockIdx.y];
    unsigned* cells = ws + f.ws_off;
    const int ncj = (f.w0 + cell - 1) / cell;
    const long long units = (long long)n * RD_SPLIT;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const int r = (int)(u / RD_SPLIT), sp = (int)(u % RD_SPLIT);
        double x[4], y[4];
        RdRect rc;
        const int st = redact_quad(det + ((long long)blockIdx.y * max_det + r) * LP_DET_COLS, s, f.h0, f.w0, x, y, &rc);
        if (st == 3 || rc.i0 >= rc.i1 || rc.j0 >= rc.j1) continue;
        const int I0 = rc.i0 / cell, J0 = rc.j0 / cell, nJ = (rc.j1 - 1) / cell - J0 + 1;
        const long long ncells = (long long)((rc.i1 - 1) / cell - I0 + 1) * nJ;
        for (long long c = sp * 4 + threadIdx.y; c < ncells; c += 4 * RD_SPLIT) {
            const int I = I0 + (int)(c / nJ), J = J0 + (int)(c % nJ);
            const int ya = I * cell, xa = J * cell;
            const int yb = ya + cell < f.h0 ? ya + cell : f.h0, xb = xa + cell < f.w0 ? xa + cell : f.w0;
            int acc[3] = {0, 0, 0};
            SINK::gather(f, ya, yb, xa, xb, threadIdx.x, acc);
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                acc[0] += __shfl_xor(acc[0], m, 64);
                acc[1] += __shfl_xor(acc[1], m, 64);
                acc[2] += __shfl_xor(acc[2], m, 64);
            }
            if (threadIdx.x == 0) {
                const int n0 = (yb - ya) * (xb - xa), n1 = SINK::chroma_count(n0);      // at most 64 x 64 x 255 per sum
                const unsigned c0 = (unsigned)((2 * acc[0] + n0) / (2 * n0));
                const unsigned c1 = (unsigned)((2 * acc[1] + n1) / (2 * n1)), c2 = (unsigned)((2 * acc[2] + n1) / (2 * n1));
                cells[(long long)I * ncj + J] = c0 | (c1 << 8) | (c2 << 16);
            }
        }
    }
}

// grid (RD_WGS, frames of this launch), block (64, 4).  Unit (r, s): wave y takes the pixel rows i0 + 4 s + y, + 32, ... of the row's
// rectangle, lanes along a frame row (adjacent lanes store adjacent pixels); a pixel whose centre passes the four edge tests
// gets its cell's entry (cells != null: mosaic) or `fill`.  Unit (r, 0) writes status[r]; the rows at or past n_b are zeroed.
// Reads det, count and the workspace, writes the frames.
template <typename SINK>
__global__ __launch_bounds__(256) void redact_write_kernel(const RdTable tab, const float* __restrict__ det, const int32_t* __restrict__ count,
                                                           int max_det, double s, int cell, unsigned fill, const unsigned* __restrict__ ws,
                                                           int32_t* __restrict__ status) {
    const int n = clamp_count(count[blockIdx.y], max_det);
    const int tid = threadIdx.y * 64 + threadIdx.x;
    int32_t* st_b = status + (long long)blockIdx.y * max_det;
    for (long long r = (long long)n + blockIdx.x * 256 + tid; r < max_det; r += gridDim.x * 256) st_b[r] = 0;
    if (n == 0) return;
    const RdEntry f = tab.f[blockIdx.y];
    const unsigned* cells = ws ? ws + f.ws_off : nullptr;
    const int ncj = (f.w0 + cell - 1) / cell;
    const long long units = (long long)n * RD_SPLIT;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const int r = (int)(u / RD_SPLIT), sp = (int)(u % RD_SPLIT);
        double x[4], y[4];
        RdRect rc;
        const int st = redact_quad(det + ((long long)blockIdx.y * max_det + r) * LP_DET_COLS, s, f.h0, f.w0, x, y, &rc);
        if (sp == 0 && tid == 0) st_b[r] = st;
        if (st == 3) continue;
        // the edges a -> b = a + e along p0 -> p3 -> p2 -> p1 -> p0
        const int ord[4] = {0, 3, 2, 1};
        double ax[4], ay[4], ex[4], ey[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int a = ord[k], b = ord[(k + 1) & 3];
            ax[k] = x[a]; ay[k] = y[a];
            ex[k] = x[b] - x[a]; ey[k] = y[b] - y[a];
        }
        for (int i = rc.i0 + sp * 4 + threadIdx.y; i < rc.i1; i += 4 * RD_SPLIT) {
            const double py = (double)i + 0.5;
            double t[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) t[k] = ex[k] * (py - ay[k]);
            const unsigned* crow = cells ? cells + (long long)(i / cell) * ncj : nullptr;
            for (int j = rc.j0 + threadIdx.x; j < rc.j1; j += 64) {
                const double px = (double)j + 0.5;
                bool in = true;
#pragma unroll
                for (int k = 0; k < 4; ++k) in = in && (t[k] - ey[k] * (px - ax[k]) <= 0.0);
                if (in) SINK::put(f, i, j, crow ? crow[j / cell] : fill);
            }
        }
    }
}

// grid (RD_WGS, frames of this launch), block (64, 4), dynamic LDS [out GS_OUT_BYTES | hq | in], in at byte in_off.  Unit (r, s): the
// workgroup takes the tiles s, s + RD_SPLIT, ... of the frame-anchored tiles that the row's rectangle touches (row-major), one tile
// at a time.  Every thread derives the same rectangle from the same row, so the loops and their barriers are uniform.  Reads the
// frames, writes the workspace.
template <typename SINK>
__global__ __launch_bounds__(256) void redact_gauss_kernel(const RdTable tab, const GsTaps tp, const float* __restrict__ det,
                                                           const int32_t* __restrict__ count, int max_det, double s, int in_off,
                                                           unsigned* __restrict__ ws) {
    extern __shared__ __align__(16) unsigned char gs_lds[];
    const int n = clamp_count(count[blockIdx.y], max_det);
    if (n == 0) return;
    const RdEntry f = tab.f[blockIdx.y];
    unsigned* table = ws + f.ws_off;
    unsigned char* out = gs_lds;
    unsigned short* hq = reinterpret_cast<unsigned short*>(gs_lds + GS_OUT_BYTES);
    unsigned char* in = gs_lds + in_off;
    const long long units = (long long)n * RD_SPLIT;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const int r = (int)(u / RD_SPLIT), sp = (int)(u % RD_SPLIT);
        double x[4], y[4];
        RdRect rc;
        const int st = redact_quad(det + ((long long)blockIdx.y * max_det + r) * LP_DET_COLS, s, f.h0, f.w0, x, y, &rc);
        if (st == 3 || rc.i0 >= rc.i1 || rc.j0 >= rc.j1) continue;
        const int I0 = rc.i0 / GS_TILE, J0 = rc.j0 / GS_TILE, nJ = (rc.j1 - 1) / GS_TILE - J0 + 1;
        const long long ntiles = (long long)((rc.i1 - 1) / GS_TILE - I0 + 1) * nJ;
        for (long long t = sp; t < ntiles; t += RD_SPLIT) {
            const int y0 = (I0 + (int)(t / nJ)) * GS_TILE, x0 = (J0 + (int)(t % nJ)) * GS_TILE;
            const int th = y0 + GS_TILE < f.h0 ? GS_TILE : f.h0 - y0, tw = x0 + GS_TILE < f.w0 ? GS_TILE : f.w0 - x0;
            SINK::gauss_tile(f, tp, y0, x0, th, tw, in, hq, out, table);
        }
    }
}

// The rules of one descriptor; an empty string: fine.
std::string desc_fault(const lp_redact_desc& d) {
    if (d.format != 0 && d.format != 1) return "unknown format";
    if (d.format == 1) return plane_fault(d.p0, d.p1, d.pitch0, d.pitch1, d.h0, d.w0, 0);      // the matrix plays no part
    if (!d.p0) return "null p0";
    if (d.p1) return "p1 must be null for a BGR frame";
    if (d.h0 < 1 || d.w0 < 1 || d.w0 > 0x7fffffff / 3) return "h0, w0 must be >= 1";
    if (d.pitch0 < 3 * d.w0) return "pitch0 < 3 * w0";
    return "";
}

std::string params_fault(const lp_redact_params& p) {
    if (p.mode != 0 && p.mode != 1) return "mode must be 0 (mosaic) or 1 (fill)";
    if (p.mode == 0 && (p.cell < 2 || p.cell > LP_REDACT_MAX_CELL || (p.cell & 1))) return "cell must be even, 2..64";
    if (!(p.margin >= 0.0 && p.margin <= 4.0)) return "margin must be in [0, 4]";
    return "";
}

// entries of a frame's cell table, rounded up so that the next table starts at a 16-byte multiple
long long table_entries(const lp_redact_desc& d, int cell) {
    const long long e = (long long)ceil_div(d.h0, cell) * ceil_div(d.w0, cell);
    return (e + 3) / 4 * 4;
}

template <typename SINK>
void launch_redact(const RdTable& tab, int nf, const float* det, const int32_t* count, int max_det, const lp_redact_params& p,
                   unsigned fill, void* ws, int32_t* status, bool means, hipStream_t st) {
    const dim3 grid(RD_WGS, (unsigned)nf), block(64, 4);
    const double s = 1.0 + p.margin;
    const int cell = p.mode == 0 ? p.cell : 2;
    if (means) hipLaunchKernelGGL((redact_means_kernel<SINK>), grid, block, 0, st, tab, det, count, max_det, s, cell, (unsigned*)ws);
    else hipLaunchKernelGGL((redact_write_kernel<SINK>), grid, block, 0, st, tab, det, count, max_det, s, cell, fill,
                            (const unsigned*)(p.mode == 0 ? ws : nullptr), status);
}

// The rules of a tap vector t[0..radius]; an empty string: fine.
std::string taps_fault(int radius, const uint16_t* t, const char* name) {
    if (radius < 1 || radius > LP_REDACT_MAX_RADIUS) return std::string(name) + ": radius must be in 1..48";
    long long total = t[0];
    for (int k = 1; k <= radius; ++k) {
        if (t[k] > t[k - 1]) return std::string(name) + " must not increase";
        total += 2 * (long long)t[k];
    }
    if (total != 16384) return std::string(name) + ": t[0] + 2 * sum t[1..radius] must be 16384";
    return "";
}

std::string gauss_params_fault(const lp_redact_gauss_params& p, bool nv12) {
    if (!(p.margin >= 0.0 && p.margin <= 4.0)) return "margin must be in [0, 4]";
    const std::string why = taps_fault(p.radius, p.taps, "taps");
    if (!why.empty() || !nv12) return why;
    return taps_fault(p.radius_c, p.taps_c, "taps_c");
}

bool any_nv12(const lp_redact_desc* desc, int n_frames) {
    for (int b = 0; b < n_frames; ++b)
        if (desc[b].format == 1) return true;
    return false;
}

// dynamic LDS of redact_gauss_kernel<SINK> at these radii; *in_off: where the staged bytes start
template <typename SINK>
int gauss_lds_bytes(int R, int Rc, int* in_off) {
    *in_off = GS_OUT_BYTES + SINK::gauss_hq_bytes(R, Rc);
    return *in_off + SINK::gauss_in_bytes(R, Rc);
}
constexpr int GS_MAX_LDS = GS_OUT_BYTES + gs_hq_bytes(GS_TILE, LP_REDACT_MAX_RADIUS, 3) + gs_in_bytes(GS_TILE, LP_REDACT_MAX_RADIUS, 3);
static_assert(GS_MAX_LDS <= 160 * 1024, "a tile at the largest radius must fit the LDS of a CU");

template <typename SINK>
int gauss_lds_attr() {
    static std::atomic<unsigned long long> attr_done{0};
    return set_max_lds_once(redact_gauss_kernel<SINK>, GS_MAX_LDS, attr_done, "redact gauss");
}

template <typename SINK>
void launch_gauss(const RdTable& tab, int nf, const GsTaps& tp, const float* det, const int32_t* count, int max_det, double margin,
                  void* ws, hipStream_t st) {
    int in_off = 0;
    const int lds = gauss_lds_bytes<SINK>(tp.r, tp.rc, &in_off);
    hipLaunchKernelGGL((redact_gauss_kernel<SINK>), dim3(RD_WGS, (unsigned)nf), dim3(64, 4), (size_t)lds, st, tab, tp, det, count, max_det,
                       1.0 + margin, in_off, (unsigned*)ws);
}

}  // namespace

// the descriptor rules for the other entry points that take lp_redact_desc (lp_overlay.hip)
std::string redact_desc_fault(const lp_redact_desc& d) { return desc_fault(d); }

}  // namespace lp

using namespace lp;

extern "C" size_t lp_redact_workspace_bytes(const lp_redact_desc* desc, int n_frames, const lp_redact_params* p) {
    if (!desc || !p || n_frames < 1 || p->mode != 0 || !params_fault(*p).empty()) return 0;
    long long entries = 0;
    for (int b = 0; b < n_frames; ++b) {
        if (desc[b].h0 < 1 || desc[b].w0 < 1) return 0;
        entries += table_entries(desc[b], p->cell);
    }
    return (size_t)entries * 4;
}

extern "C" int lp_redact_plates_batch(const lp_redact_desc* desc, int n_frames, const float* det, const int32_t* count, int max_det,
                                      const lp_redact_params* p, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    const std::string fn = "lp_redact_plates_batch: ";
    if (n_frames < 0 || !desc || !p || !status) return fail(LP_ERR_ARG, fn + "bad arguments (need desc, p, status, n_frames >= 0)");
    if (max_det < 1) return fail(LP_ERR_ARG, fn + "max_det must be >= 1");
    const std::string why = params_fault(*p);
    if (!why.empty()) return fail(LP_ERR_ARG, fn + why);
    for (int b = 0; b < n_frames; ++b) {       // every frame is checked before the first launch
        const std::string bad = desc_fault(desc[b]);
        if (!bad.empty()) return fail(LP_ERR_ARG, fn + bad + " (frame " + std::to_string(b) + ")");
    }
    if (n_frames == 0) return LP_OK;
    if (!det || !count) return fail(LP_ERR_ARG, fn + "null det or count");
    const bool mosaic = p->mode == 0;
    if (mosaic) {
        const size_t need = lp_redact_workspace_bytes(desc, n_frames, p);
        if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < need)
            return fail(LP_ERR_ARG, fn + "workspace must be 16-byte aligned and hold " + std::to_string(need) + " bytes");
    }
    hipStream_t st = (hipStream_t)stream;
    const unsigned fill = (unsigned)p->fill[0] | ((unsigned)p->fill[1] << 8) | ((unsigned)p->fill[2] << 16);
    // a launch = a run of at most LP_FRAMES_PER_LAUNCH consecutive frames of one format
    struct Run { int b0, nf, format; RdTable tab; };
    std::vector<Run> runs;
    long long off = 0;
    for (int b = 0; b < n_frames; ++b) {
        const lp_redact_desc& d = desc[b];
        if (runs.empty() || runs.back().format != d.format || runs.back().nf == LP_FRAMES_PER_LAUNCH) runs.push_back({b, 0, d.format, {}});
        Run& r = runs.back();
        r.tab.f[r.nf++] = {d.p0, d.p1, d.pitch0, d.pitch1, d.h0, d.w0, off};
        if (mosaic) off += table_entries(d, p->cell);
    }
    for (int pass = mosaic ? 0 : 1; pass < 2; ++pass)      // every cell mean is taken before the first byte of a frame is replaced
        for (const Run& r : runs) {
            const float* dt = det + (size_t)r.b0 * max_det * LP_DET_COLS;
            int32_t* sb = status + (size_t)r.b0 * max_det;
            if (r.format == 1) launch_redact<Nv12Sink>(r.tab, r.nf, dt, count + r.b0, max_det, *p, fill, workspace, sb, pass == 0, st);
            else launch_redact<BgrSink>(r.tab, r.nf, dt, count + r.b0, max_det, *p, fill, workspace, sb, pass == 0, st);
            LP_HIP_CHECK(hipGetLastError());
        }
    return LP_OK;
}

extern "C" size_t lp_redact_gauss_workspace_bytes(const lp_redact_desc* desc, int n_frames, const lp_redact_gauss_params* p) {
    if (!desc || !p || n_frames < 1 || !gauss_params_fault(*p, any_nv12(desc, n_frames)).empty()) return 0;
    long long entries = 0;
    for (int b = 0; b < n_frames; ++b) {
        if (desc[b].h0 < 1 || desc[b].w0 < 1) return 0;
        entries += table_entries(desc[b], 1);
    }
    return (size_t)entries * 4;
}

extern "C" int lp_redact_gauss_batch(const lp_redact_desc* desc, int n_frames, const float* det, const int32_t* count, int max_det,
                                     const lp_redact_gauss_params* p, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    const std::string fn = "lp_redact_gauss_batch: ";
    if (n_frames < 0 || !desc || !p || !status) return fail(LP_ERR_ARG, fn + "bad arguments (need desc, p, status, n_frames >= 0)");
    if (max_det < 1) return fail(LP_ERR_ARG, fn + "max_det must be >= 1");
    const std::string why = gauss_params_fault(*p, any_nv12(desc, n_frames));
    if (!why.empty()) return fail(LP_ERR_ARG, fn + why);
    for (int b = 0; b < n_frames; ++b) {       // every frame is checked before the first launch
        const std::string bad = desc_fault(desc[b]);
        if (!bad.empty()) return fail(LP_ERR_ARG, fn + bad + " (frame " + std::to_string(b) + ")");
    }
    if (n_frames == 0) return LP_OK;
    if (!det || !count) return fail(LP_ERR_ARG, fn + "null det or count");
    const size_t need = lp_redact_gauss_workspace_bytes(desc, n_frames, p);
    if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < need)
        return fail(LP_ERR_ARG, fn + "workspace must be 16-byte aligned and hold " + std::to_string(need) + " bytes");
    hipStream_t st = (hipStream_t)stream;
    const bool nv12 = any_nv12(desc, n_frames);
    GsTaps tp = {};
    tp.r = p->radius;
    tp.rc = nv12 ? p->radius_c : 1;            // taps_c is read only with an NV12 frame
    for (int i = 0; i <= 2 * tp.r; ++i) tp.w[i + GS_GROUP - 1] = p->taps[std::abs(i - tp.r)];
    for (int i = 0; nv12 && i <= 2 * tp.rc; ++i) tp.wc[i + GS_GROUP - 1] = p->taps_c[std::abs(i - tp.rc)];
    if (int rc = gauss_lds_attr<BgrSink>()) return rc;
    if (int rc = nv12 ? gauss_lds_attr<Nv12Sink>() : LP_OK) return rc;
    // a launch = a run of at most LP_FRAMES_PER_LAUNCH consecutive frames of one format
    struct Run { int b0, nf, format; RdTable tab; };
    std::vector<Run> runs;
    long long off = 0;
    for (int b = 0; b < n_frames; ++b) {
        const lp_redact_desc& d = desc[b];
        if (runs.empty() || runs.back().format != d.format || runs.back().nf == LP_FRAMES_PER_LAUNCH) runs.push_back({b, 0, d.format, {}});
        Run& r = runs.back();
        r.tab.f[r.nf++] = {d.p0, d.p1, d.pitch0, d.pitch1, d.h0, d.w0, off};
        off += table_entries(d, 1);
    }
    lp_redact_params wp = {};                  // the write pass: the mosaic's, its table at cell 1
    wp.mode = 0;
    wp.cell = 1;
    wp.margin = p->margin;
    for (int pass = 0; pass < 2; ++pass)       // every tile is blurred before the first byte of a frame is replaced
        for (const Run& r : runs) {
            const float* dt = det + (size_t)r.b0 * max_det * LP_DET_COLS;
            int32_t* sb = status + (size_t)r.b0 * max_det;
            if (pass == 0 && r.format == 1) launch_gauss<Nv12Sink>(r.tab, r.nf, tp, dt, count + r.b0, max_det, p->margin, workspace, st);
            else if (pass == 0) launch_gauss<BgrSink>(r.tab, r.nf, tp, dt, count + r.b0, max_det, p->margin, workspace, st);
            else if (r.format == 1) launch_redact<Nv12Sink>(r.tab, r.nf, dt, count + r.b0, max_det, wp, 0u, workspace, sb, false, st);
            else launch_redact<BgrSink>(r.tab, r.nf, dt, count + r.b0, max_det, wp, 0u, workspace, sb, false, st);
            LP_HIP_CHECK(hipGetLastError());
        }
    return LP_OK;
}
