// Skipping the unchanged tiles of fixed-camera frames in tiled detection: lp_tile_gate_luma_batch, lp_tile_gate_update and
// lp_tile_gate_update_gain (include/lp_hip.h).  The reference has nothing here; the written-down specification is
// yolov6/utils/tile_gate.py (luma_blocks_np, gate_update_np, gate_update_gain_np), which these kernels match on every integer
// (tests/test_tile_gate_gpu.py, tests/test_tile_gate_gain_gpu.py).  Everything is
// integer, and the one reduction is an integer sum, so the result does not depend on the order of the lanes.
//
// gate_luma_kernel<Src>: the sums of luma over the 4 x 4 pixel blocks of a batch of frames.  ONE kernel over two pixel sources,
//   BgrLuma (3 interleaved bytes per pixel, L = (29 B + 150 G + 77 R + 128) >> 8) and YLuma (the luma plane of an NV12 frame at
//   its pitch; the chroma plane is never read).  A lane's unit is 16 pixels x 4 rows = four blocks: per row one 16-byte load
//   (Y) or three (BGR), all of a unit's loads issued before the first is used; the lanes of a wave take neighbouring units of
//   one band of four rows, so a wave's loads cover contiguous segments of four rows.  The loads are at any alignment (a BGR
//   row of w pixels is 3 w bytes: its units sit at multiples of 48 bytes from a row start that need not be aligned).  A unit
//   is loaded whole only where its 16 pixels are inside the row; the last unit of a row whose width is no multiple of 16 reads
//   its pixels byte by byte, so nothing past a row's last pixel -- and so nothing past the frame's last byte -- is read.  Rows
//   at or past h0 are not read.  Every frame byte is read once, 2 bytes are written per 16 pixels: the bound is the read of
//   the frame.  No LDS, no scratch, no atomics.
// gate_update_kernel: one workgroup per (frame of the call, tile).  Phase 1: the lanes walk the tile's cells of 4 x 4 blocks and
//   count the changed ones into one LDS word.  Barrier.  Phase 2, if the tile is flagged: its blocks are copied into ref.
//   A tile entry of the device table is checked against the frame and the size of ref before anything is indexed with it (the
//   host cannot see the table): a bad entry is flagged with ncell = -1 and touches no state.
// gate_update_gain_kernel (lp_tile_gate_update_gain; gate_update_gain_np in the specification): the same workgroup per (frame, tile),
//   for frames whose exposure or daylight drifts.  Each cell gets a Q12 gain g_c = sum(cur) / sum(ref) of 16 bits; the tile's gain
//   is their lower median, selected by two radix passes: a 256-bin LDS histogram of the high byte (integer atomics) and a scan
//   over the bins give the bin that holds the median's rank, a second histogram of the low byte among the cells of that bin gives
//   the value.  Then the cell pass compares |cur * 4096 - ref * G| with the bar, and the copy of ref follows as above.  g_c is
//   recomputed per pass, not kept: no LDS capacity, no second path.  Integer counts: the result does not depend on lane order.
// The frame tables travel by value in the kernel arguments: nothing is uploaded, no host read, nothing allocated, capturable.
#include <vector>

#include "lp_internal.h"
#include "lp_streams.h"

namespace lp {

namespace {

constexpr int TG_T = 256;                                  // threads of a workgroup, both kernels
constexpr int TG_MAX_THRES16 = 255 * 16;

struct GateFrame {
    const unsigned char* p0;                               // BGR: the frame; NV12: the luma plane
    unsigned short* blocks;                                // the frame's block grid [nby][nbx]
    int pitch0, h0, w0;
    int stream, n_tiles;                                   // lp_tile_gate_update: stream of the frame (-1: not gated), its tiles
    int pad;
};
struct GateTable { GateFrame f[LP_FRAMES_PER_LAUNCH]; };
static_assert(sizeof(GateTable) < 4096 - 64, "the table travels as kernel arguments: under 4 KiB");

// 16 bytes from any address: one global_load_dwordx4 (the target allows unaligned vector loads of global memory)
struct __attribute__((packed, aligned(1))) U4 { unsigned x, y, z, w; };
__device__ __forceinline__ uint4 load16(const unsigned char* p) {
    const U4 v = *reinterpret_cast<const U4*>(p);
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ int sum4(unsigned v) { return (int)((v & 255u) + ((v >> 8) & 255u) + ((v >> 16) & 255u) + (v >> 24)); }
__device__ __forceinline__ int luma(unsigned b, unsigned g, unsigned r) { return (int)((29u * b + 150u * g + 77u * r + 128u) >> 8); }

struct BgrLuma {
    static constexpr int BPP = 3, LOADS = 3;
    static __device__ __forceinline__ int pixel(const unsigned char* q) { return luma(q[0], q[1], q[2]); }
    // 12 bytes = the four pixels of a block's row
    static __device__ __forceinline__ int block(unsigned d0, unsigned d1, unsigned d2) {
        return luma(d0 & 255u, (d0 >> 8) & 255u, (d0 >> 16) & 255u) + luma(d0 >> 24, d1 & 255u, (d1 >> 8) & 255u) +
               luma((d1 >> 16) & 255u, d1 >> 24, d2 & 255u) + luma((d2 >> 8) & 255u, (d2 >> 16) & 255u, d2 >> 24);
    }
    static __device__ __forceinline__ void row(const uint4* v, int* s) {
        s[0] += block(v[0].x, v[0].y, v[0].z);
        s[1] += block(v[0].w, v[1].x, v[1].y);
        s[2] += block(v[1].z, v[1].w, v[2].x);
        s[3] += block(v[2].y, v[2].z, v[2].w);
    }
};
struct YLuma {
    static constexpr int BPP = 1, LOADS = 1;
    static __device__ __forceinline__ int pixel(const unsigned char* q) { return q[0]; }
    static __device__ __forceinline__ void row(const uint4* v, int* s) {
        s[0] += sum4(v[0].x); s[1] += sum4(v[0].y); s[2] += sum4(v[0].z); s[3] += sum4(v[0].w);
    }
};

// grid (ceil(max units of a frame / 256), frames of the launch), block (256); unit u of a frame = (band u / ux, column u % ux)
template <typename Src>
__global__ __launch_bounds__(TG_T) void gate_luma_kernel(GateTable tab) {
    const GateFrame& f = tab.f[blockIdx.y];
    const int ux = (f.w0 + 15) >> 4, uy = (f.h0 + 3) >> 2;
    const int u = blockIdx.x * TG_T + threadIdx.x;
    if (u >= ux * uy) return;                              // ux * uy < 2^31: checked on the host
    const int band = u / ux, col = u - band * ux;
    const int y0 = band * 4, x0 = col * 16;
    const int rows = f.h0 - y0 < 4 ? f.h0 - y0 : 4;        // >= 1
    const unsigned char* q = f.p0 + (long long)y0 * f.pitch0 + (long long)x0 * Src::BPP;
    int s[4] = {0, 0, 0, 0};
    if (x0 + 16 <= f.w0) {
        uint4 v[4][Src::LOADS];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int k = 0; k < Src::LOADS; ++k)
                v[r][k] = r < rows ? load16(q + (long long)r * f.pitch0 + 16 * k) : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int r = 0; r < 4; ++r) Src::row(v[r], s);     // a row past h0 adds the luma of zeros: 0
    } else {
        const int n = f.w0 - x0;                           // 1..15 pixels: byte loads, nothing past the row's last pixel
        for (int r = 0; r < rows; ++r)
            for (int i = 0; i < n; ++i) s[i >> 2] += Src::pixel(q + (long long)r * f.pitch0 + i * Src::BPP);
    }
    const int nbx = (f.w0 + 3) >> 2;
    unsigned short* o = f.blocks + (long long)band * nbx + col * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (col * 4 + k < nbx) o[k] = (unsigned short)s[k];
}

struct GateParams { int thres16, min_cells, refresh, max_tiles; long long ref_elems; };

// grid (max_tiles, frames of the launch), block (256); flag / ncell point at the launch's first frame
__global__ __launch_bounds__(TG_T) void gate_update_kernel(GateTable tab, const int32_t* __restrict__ tiles, unsigned short* __restrict__ ref,
                                                           int32_t* __restrict__ age, GateParams p, unsigned char* __restrict__ flag,
                                                           int32_t* __restrict__ ncell) {
    __shared__ int s_count;
    const GateFrame& f = tab.f[blockIdx.y];
    const int t = blockIdx.x, tid = threadIdx.x;
    const long long out = (long long)blockIdx.y * p.max_tiles + t;
    if (f.stream < 0 || t >= f.n_tiles) {                  // (block-uniform) not gated: all flagged; past the plan: nothing
        if (tid == 0) { flag[out] = f.stream < 0 ? 1 : 0; ncell[out] = 0; }
        return;
    }
    const long long slot = (long long)f.stream * p.max_tiles + t;
    const int32_t* e = tiles + slot * LP_TILE_GATE_TILE_WORDS;
    const int y0 = e[0], x0 = e[1], th = e[2], tw = e[3];
    const long long ref_off = e[4];
    const bool inside = y0 >= 0 && x0 >= 0 && th >= 1 && tw >= 1 && th <= f.h0 - y0 && tw <= f.w0 - x0;
    const int by0 = y0 >> 2, by1 = (y0 + th - 1) >> 2, bx0 = x0 >> 2, bx1 = (x0 + tw - 1) >> 2;
    const int nby = by1 - by0 + 1, nbx = bx1 - bx0 + 1;
    if (!inside || ref_off < 0 || ref_off + (long long)nby * nbx > p.ref_elems) {      // (block-uniform) a bad table entry
        if (tid == 0) { flag[out] = 1; ncell[out] = -1; }
        return;
    }
    const int gw = (f.w0 + 3) >> 2;                        // blocks per row of the frame's grid
    const unsigned short* cur = f.blocks + (long long)by0 * gw + bx0;
    unsigned short* rf = ref + ref_off;
    const int a = age[slot];
    if (tid == 0) s_count = 0;
    __syncthreads();
    if (a >= 0) {                                          // (block-uniform) a never-detected tile does not read its ref
        const int ncx = (nbx + 3) >> 2, ncy = (nby + 3) >> 2;
        int n = 0;
        for (int c = tid; c < ncx * ncy; c += TG_T) {
            const int cy = c / ncx, cx = c - cy * ncx;
            int A = 0, npix = 0;
            for (int j = cy * 4; j < cy * 4 + 4 && j < nby; ++j) {
                const int py = f.h0 - 4 * (by0 + j) < 4 ? f.h0 - 4 * (by0 + j) : 4;
                for (int i = cx * 4; i < cx * 4 + 4 && i < nbx; ++i) {
                    const int px = f.w0 - 4 * (bx0 + i) < 4 ? f.w0 - 4 * (bx0 + i) : 4;
                    const int d = (int)cur[(long long)j * gw + i] - (int)rf[j * nbx + i];
                    A += d < 0 ? -d : d;
                    npix += py * px;
                }
            }
            n += 16 * A > p.thres16 * npix ? 1 : 0;        // A <= 16 * 65535 and thres16 * npix <= 4080 * 256: int32
        }
        if (n) atomicAdd(&s_count, n);
    }
    __syncthreads();                                       // the count is whole, and every read of ref is behind us
    const int n = s_count;
    const bool on = a < 0 || n >= p.min_cells || (p.refresh > 0 && a + 1 >= p.refresh);
    if (on)
        for (int k = tid; k < nby * nbx; k += TG_T) {
            const int j = k / nbx, i = k - j * nbx;
            rf[k] = cur[(long long)j * gw + i];
        }
    if (tid == 0) {
        flag[out] = on ? 1 : 0;
        ncell[out] = n;
        age[slot] = on ? ((a < 0 && p.refresh > 0) ? t % p.refresh : 0) : a + 1;
    }
}

// ---- gain mode (lp_tile_gate_update_gain) ----------------------------------------------------------------------------------------------
constexpr int TG_ONE = 4096;                               // a gain of 1 in Q12
constexpr int TG_MAX_GAIN = 4 * TG_ONE;                    // the largest gain_hi: 4080 * 16384 * 16 terms stay below 2^31
constexpr unsigned TG_CELL_GAIN_CAP = 65535u;              // g_c has 16 bits: two radix passes of one byte
constexpr int TG_BINS = 256;
static_assert(TG_BINS == TG_T, "one lane per bin in the scan");

struct GateTile {                                          // a tile's blocks: cur at the frame's pitch gw, ref at nbx
    const unsigned short* cur;
    const unsigned short* rf;
    int gw, nby, nbx, ncx, cells;
};

// four block sums from any 2-byte aligned address: one global_load_dwordx2
struct __attribute__((packed, aligned(1))) U2 { unsigned x, y; };
__device__ __forceinline__ void load4(const unsigned short* p, int* o) {
    const U2 v = *reinterpret_cast<const U2*>(p);
    o[0] = (int)(v.x & 0xffffu); o[1] = (int)(v.x >> 16); o[2] = (int)(v.y & 0xffffu); o[3] = (int)(v.y >> 16);
}

// The block sums of cell c, row by row: cur[16] and rf[16], 0 where the cell has no block (a cell at the end of the tile's range).
// A whole cell is eight 8-byte loads, all issued before the first is used; a clipped one reads its blocks one by one, so nothing
// outside the tile's blocks is read.
__device__ __forceinline__ void load_cell(const GateTile& g, int c, int* cur, int* rf) {
    const int cy = c / g.ncx, cx = c - cy * g.ncx;
    const unsigned short* pc = g.cur + (long long)cy * 4 * g.gw + cx * 4;
    const unsigned short* pr = g.rf + cy * 4 * g.nbx + cx * 4;
    if (cy * 4 + 4 <= g.nby && cx * 4 + 4 <= g.nbx) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            load4(pc + (long long)j * g.gw, cur + 4 * j);
            load4(pr + j * g.nbx, rf + 4 * j);
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool in = cy * 4 + j < g.nby && cx * 4 + i < g.nbx;
            cur[4 * j + i] = in ? pc[(long long)j * g.gw + i] : 0;
            rf[4 * j + i] = in ? pr[j * g.nbx + i] : 0;
        }
}

// g_c of cell c, or -1 where the cell has no gain (R_c == 0)
__device__ __forceinline__ int cell_gain(const GateTile& g, int c) {
    int cur[16], rf[16];
    load_cell(g, c, cur, rf);
    unsigned R = 0, C = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        C += (unsigned)cur[k];
        R += (unsigned)rf[k];
    }
    if (R == 0) return -1;
    const unsigned q = (C * (unsigned)TG_ONE + (R >> 1)) / R;     // C, R <= 65280: the numerator is below 2^29
    return (int)(q < TG_CELL_GAIN_CAP ? q : TG_CELL_GAIN_CAP);
}

// The histogram half of a radix pass, called by all 256 lanes: the counts of byte (g_c >> shift) & 255 over the cells with a gain
// (shift 0: over those whose high byte is `high`) into hist, their inclusive scan over the bins into scan.  Returns the number of
// cells counted.  A lane adds a run of equal bytes with one atomic: under a plain drift every cell of a tile has the same high
// byte, and 256 lanes adding ones to one LDS word would serialise.  The counts are integers, so the result does not depend on the
// order of the lanes.
__device__ int radix_count(const GateTile& g, int shift, int high, int* hist, int* scan) {
    const int tid = threadIdx.x;
    hist[tid] = 0;
    __syncthreads();
    int run_bin = 0, run = 0;
    for (int c = tid; c < g.cells; c += TG_T) {
        const int v = cell_gain(g, c);
        if (v < 0 || (shift == 0 && (v >> 8) != high)) continue;
        const int bin = (v >> shift) & 255;
        if (bin != run_bin && run) {
            atomicAdd(&hist[run_bin], run);
            run = 0;
        }
        run_bin = bin;
        ++run;
    }
    if (run) atomicAdd(&hist[run_bin], run);
    __syncthreads();
    scan[tid] = hist[tid];                                 // one lane per bin
    __syncthreads();
    for (int d = 1; d < TG_BINS; d <<= 1) {
        const int add = tid >= d ? scan[tid - d] : 0;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    return scan[TG_BINS - 1];
}

// The selection half, called by all 256 lanes with 0 <= k < the cells counted: the bin that holds rank k; k becomes the rank
// inside that bin.  Exactly one lane finds excl <= k < incl.
__device__ int radix_select(int& k, const int* hist, const int* scan, int* sel) {
    const int tid = threadIdx.x;
    const int incl = scan[tid], excl = incl - hist[tid];
    if (excl <= k && k < incl) { sel[0] = tid; sel[1] = k - excl; }
    __syncthreads();
    const int bin = sel[0];
    k = sel[1];
    __syncthreads();                                       // hist, scan and sel are read: the next pass may overwrite them
    return bin;
}

// grid (max_tiles, frames of the launch), block (256); flag / ncell / gain point at the launch's first frame.  The prologue is
// gate_update_kernel's.  g_c is recomputed in each of the three passes over the cells (two radix passes, the cell pass) instead of
// kept in LDS: the 4K overview tile has 32400 cells = 64.8 KB as uint16, past the 64 KB a workgroup can declare, so keeping them
// would need a capacity and a second path; a pass re-reads blocks that the pass before left in the cache.
__global__ __launch_bounds__(TG_T) void gate_update_gain_kernel(GateTable tab, const int32_t* __restrict__ tiles, unsigned short* __restrict__ ref,
                                                                int32_t* __restrict__ age, GateParams p, int gain_lo, int gain_hi,
                                                                unsigned char* __restrict__ flag, int32_t* __restrict__ ncell,
                                                                int32_t* __restrict__ gain) {
    __shared__ int s_hist[TG_BINS], s_scan[TG_BINS], s_sel[2];
    __shared__ int s_count;
    const GateFrame& f = tab.f[blockIdx.y];
    const int t = blockIdx.x, tid = threadIdx.x;
    const long long out = (long long)blockIdx.y * p.max_tiles + t;
    if (f.stream < 0 || t >= f.n_tiles) {                  // (block-uniform) not gated: all flagged; past the plan: nothing
        if (tid == 0) { flag[out] = f.stream < 0 ? 1 : 0; ncell[out] = 0; gain[out] = 0; }
        return;
    }
    const long long slot = (long long)f.stream * p.max_tiles + t;
    const int32_t* e = tiles + slot * LP_TILE_GATE_TILE_WORDS;
    const int y0 = e[0], x0 = e[1], th = e[2], tw = e[3];
    const long long ref_off = e[4];
    const bool inside = y0 >= 0 && x0 >= 0 && th >= 1 && tw >= 1 && th <= f.h0 - y0 && tw <= f.w0 - x0;
    const int by0 = y0 >> 2, by1 = (y0 + th - 1) >> 2, bx0 = x0 >> 2, bx1 = (x0 + tw - 1) >> 2;
    const int nby = by1 - by0 + 1, nbx = bx1 - bx0 + 1;
    if (!inside || ref_off < 0 || ref_off + (long long)nby * nbx > p.ref_elems) {      // (block-uniform) a bad table entry
        if (tid == 0) { flag[out] = 1; ncell[out] = -1; gain[out] = 0; }
        return;
    }
    const int gw = (f.w0 + 3) >> 2;                        // blocks per row of the frame's grid
    const unsigned short* cur = f.blocks + (long long)by0 * gw + bx0;
    unsigned short* rf = ref + ref_off;
    const int a = age[slot];
    if (tid == 0) s_count = 0;
    __syncthreads();                                       // every lane has read age before lane 0 may write it
    int n = 0, g_raw = 0;
    bool on = true;
    if (a >= 0) {                                          // (block-uniform) a never-detected tile does not read its ref
        const int ncx = (nbx + 3) >> 2, ncy = (nby + 3) >> 2;
        const GateTile g = {cur, rf, gw, nby, nbx, ncx, ncx * ncy};
        // the lower median of g_c: the value of rank (m - 1) / 2, found byte by byte
        const int m = radix_count(g, 8, 0, s_hist, s_scan);
        g_raw = TG_ONE;
        if (m > 0) {                                       // (block-uniform)
            int k = (m - 1) >> 1;
            const int high = radix_select(k, s_hist, s_scan, s_sel);
            radix_count(g, 0, high, s_hist, s_scan);
            g_raw = (high << 8) | radix_select(k, s_hist, s_scan, s_sel);
        }
        const int G = g_raw < gain_lo ? gain_lo : (g_raw > gain_hi ? gain_hi : g_raw);
        int mine = 0;
        for (int c = tid; c < g.cells; c += TG_T) {
            const int cy = c / ncx, cx = c - cy * ncx;
            int sc[16], sr[16];
            load_cell(g, c, sc, sr);
            int A = 0;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int d = sc[k] * TG_ONE - sr[k] * G;  // each below 2^26 (0 - 0 where the cell has no block)
                A += d < 0 ? -d : d;                       // 16 terms of at most 4080 * 16384: below 2^31
            }
            // the frame pixels of the cell's blocks: blocks are clipped by the frame only, so the sum of py * px is a product
            const int j1 = cy * 4 + 4 < nby ? cy * 4 + 4 : nby, i1 = cx * 4 + 4 < nbx ? cx * 4 + 4 : nbx;
            const int yend = 4 * (by0 + j1) < f.h0 ? 4 * (by0 + j1) : f.h0, xend = 4 * (bx0 + i1) < f.w0 ? 4 * (bx0 + i1) : f.w0;
            const int npix = (yend - 4 * (by0 + cy * 4)) * (xend - 4 * (bx0 + cx * 4));
            mine += A > p.thres16 * npix * 256 ? 1 : 0;    // thres16 * npix * 256 <= 4080 * 256 * 256: int32
        }
        if (mine) atomicAdd(&s_count, mine);
        __syncthreads();                                   // the count is whole, and every read of ref is behind us
        n = s_count;
        on = g_raw < gain_lo || g_raw > gain_hi || n >= p.min_cells || (p.refresh > 0 && a + 1 >= p.refresh);
    }
    if (on)
        for (int k = tid; k < nby * nbx; k += TG_T) {
            const int j = k / nbx, i = k - j * nbx;
            rf[k] = cur[(long long)j * gw + i];
        }
    if (tid == 0) {
        flag[out] = on ? 1 : 0;
        ncell[out] = n;
        gain[out] = g_raw;
        age[slot] = on ? ((a < 0 && p.refresh > 0) ? t % p.refresh : 0) : a + 1;
    }
}

std::string gate_frame_fault(const lp_tile_gate_desc& d, int b, bool planes) {
    const std::string at = "frame " + std::to_string(b) + ": ";
    if (d.format != 0 && d.format != 1) return at + "format " + std::to_string(d.format) + " (0 BGR, 1 NV12)";
    if (d.h0 < 1 || d.w0 < 1) return at + "h0 and w0 must be >= 1";
    if ((long long)((d.h0 + 3) >> 2) * ((d.w0 + 15) >> 4) >= 0x7fffff00ll) return at + "too many pixels";
    if (!d.blocks) return at + "null block grid";
    if (((uintptr_t)d.blocks & 1) != 0) return at + "the block grid must be 2-byte aligned";
    if (planes) {
        if (!d.p0) return at + "null plane";
        const int need = d.format == 0 ? 3 * d.w0 : d.w0;
        if (d.w0 > 0x2aaaaaaa || d.pitch0 < need) return at + "pitch0 " + std::to_string(d.pitch0) + " below the row's " + std::to_string(need) + " bytes";
    }
    return "";
}
size_t grid_bytes(const lp_tile_gate_desc& d) { return (size_t)((d.h0 + 3) >> 2) * (size_t)((d.w0 + 3) >> 2) * 2; }
size_t plane_bytes(const lp_tile_gate_desc& d) { return (size_t)(d.h0 - 1) * (size_t)d.pitch0 + (size_t)d.w0 * (d.format == 0 ? 3 : 1); }

}  // namespace

}  // namespace lp

using namespace lp;

extern "C" int lp_tile_gate_luma_batch(const lp_tile_gate_desc* desc, int n_frames, void* stream) {
    const std::string fn = "lp_tile_gate_luma_batch: ";
    if (n_frames < 0) return fail(LP_ERR_ARG, fn + "n_frames " + std::to_string(n_frames));
    if (n_frames == 0) return LP_OK;
    if (!desc) return fail(LP_ERR_ARG, fn + "null desc");
    std::vector<Region> reg;
    for (int b = 0; b < n_frames; ++b) {
        const std::string why = gate_frame_fault(desc[b], b, true);
        if (!why.empty()) return fail(LP_ERR_ARG, fn + why);
        reg.push_back({desc[b].p0, plane_bytes(desc[b]), false});
        reg.push_back({desc[b].blocks, grid_bytes(desc[b]), true});
    }
    if (regions_clash(reg.data(), (int)reg.size())) return fail(LP_ERR_ARG, fn + "a block grid may overlap neither a frame nor another grid");
    hipStream_t st = (hipStream_t)stream;
    for (int b0 = 0; b0 < n_frames; b0 += LP_FRAMES_PER_LAUNCH) {
        const int nb = std::min(LP_FRAMES_PER_LAUNCH, n_frames - b0);
        for (int fmt = 0; fmt < 2; ++fmt) {                // the frames of one format of this run as one launch
            GateTable tab = {};
            int n = 0, units = 0;
            for (int b = b0; b < b0 + nb; ++b) {
                const lp_tile_gate_desc& d = desc[b];
                if (d.format != fmt) continue;
                tab.f[n++] = GateFrame{d.p0, d.blocks, d.pitch0, d.h0, d.w0, -1, 0, 0};
                units = std::max(units, ((d.h0 + 3) >> 2) * ((d.w0 + 15) >> 4));
            }
            if (n == 0) continue;
            const dim3 grid((unsigned)ceil_div(units, TG_T), (unsigned)n);
            if (fmt == 0) hipLaunchKernelGGL(gate_luma_kernel<BgrLuma>, grid, dim3(TG_T), 0, st, tab);
            else hipLaunchKernelGGL(gate_luma_kernel<YLuma>, grid, dim3(TG_T), 0, st, tab);
            LP_HIP_CHECK(hipGetLastError());
        }
    }
    return LP_OK;
}

// lp_tile_gate_update (gain == nullptr, gain_lo / gain_hi unused) and lp_tile_gate_update_gain: the same checks and launches
static int gate_update(const std::string& fn, bool with_gain, const lp_tile_gate_desc* desc, int n_frames, const int* stream_of, int n_streams,
                       const int32_t* tiles, const int* n_tiles, int max_tiles, unsigned short* ref, long long ref_elems, int32_t* age,
                       int thres16, int min_cells, int refresh, int gain_lo, int gain_hi, unsigned char* flag, int32_t* ncell, int32_t* gain,
                       void* stream) {
    if (n_frames < 0 || n_streams < 1) return fail(LP_ERR_ARG, fn + "need n_frames >= 0 and n_streams >= 1");
    if (max_tiles < 1 || max_tiles > LP_MERGE_MAX_TILES)
        return fail(LP_ERR_ARG, fn + "max_tiles " + std::to_string(max_tiles) + " (need 1.." + std::to_string(LP_MERGE_MAX_TILES) + " tiles per frame)");
    if ((long long)n_streams * max_tiles * LP_TILE_GATE_TILE_WORDS >= 0x80000000ll) return fail(LP_ERR_ARG, fn + "n_streams * max_tiles * 8 must stay below 2^31");
    if (thres16 < 0 || thres16 > TG_MAX_THRES16 || min_cells < 1 || refresh < 0)
        return fail(LP_ERR_ARG, fn + "need thres16 in 0.." + std::to_string(TG_MAX_THRES16) + ", min_cells >= 1 and refresh >= 0");
    if (with_gain && !(1 <= gain_lo && gain_lo <= TG_ONE && TG_ONE <= gain_hi && gain_hi <= TG_MAX_GAIN))
        return fail(LP_ERR_ARG, fn + "need 1 <= gain_lo <= " + std::to_string(TG_ONE) + " <= gain_hi <= " + std::to_string(TG_MAX_GAIN));
    if (ref_elems < 1 || ref_elems >= 0x80000000ll) return fail(LP_ERR_ARG, fn + "ref_elems " + std::to_string(ref_elems) + " (need 1..2^31-1)");
    if (!tiles || !n_tiles || !ref || !age) return fail(LP_ERR_ARG, fn + "null pointer");
    if (((uintptr_t)tiles & 3) != 0 || ((uintptr_t)ref & 1) != 0 || ((uintptr_t)age & 3) != 0 || ((uintptr_t)ncell & 3) != 0 || ((uintptr_t)gain & 3) != 0)
        return fail(LP_ERR_ARG, fn + (with_gain ? "tiles, age, ncell and gain must be 4-byte and ref 2-byte aligned" : "tiles, age and ncell must be 4-byte and ref 2-byte aligned"));
    for (int s = 0; s < n_streams; ++s)
        if (n_tiles[s] < 0 || n_tiles[s] > max_tiles)
            return fail(LP_ERR_ARG, fn + "stream " + std::to_string(s) + " has " + std::to_string(n_tiles[s]) + " tiles (need 0.." + std::to_string(max_tiles) + ")");
    if (n_frames == 0) return LP_OK;
    if (!desc || !stream_of || !flag || !ncell || (with_gain && !gain)) return fail(LP_ERR_ARG, fn + "null pointer");
    {
        const std::string why = stream_of_fault(stream_of, n_frames, n_streams);
        if (!why.empty()) return fail(LP_ERR_ARG, fn + why);
    }
    const size_t slots = (size_t)n_streams * max_tiles, outs = (size_t)n_frames * max_tiles;
    std::vector<Region> reg = {{tiles, slots * LP_TILE_GATE_TILE_WORDS * 4, false}, {ref, (size_t)ref_elems * 2, true}, {age, slots * 4, true},
                               {flag, outs, true}, {ncell, outs * 4, true}};
    if (with_gain) reg.push_back({gain, outs * 4, true});
    std::vector<char> seen((size_t)n_streams, 0);
    for (int b = 0; b < n_frames; ++b) {
        const int s = stream_of[b];
        if (s < 0) continue;                               // not gated: its descriptor is not read
        if (seen[(size_t)s]) return fail(LP_ERR_ARG, fn + "stream " + std::to_string(s) + " appears twice in one call (frame " + std::to_string(b) + ")");
        seen[(size_t)s] = 1;
        const std::string why = gate_frame_fault(desc[b], b, false);
        if (!why.empty()) return fail(LP_ERR_ARG, fn + why);
        reg.push_back({desc[b].blocks, grid_bytes(desc[b]), false});
    }
    if (regions_clash(reg.data(), (int)reg.size()))
        return fail(LP_ERR_ARG, fn + (with_gain ? "ref, age, flag, ncell and gain may overlap neither an input nor each other"
                                                : "ref, age, flag and ncell may overlap neither an input nor each other"));
    hipStream_t st = (hipStream_t)stream;
    const GateParams p = {thres16, min_cells, refresh, max_tiles, ref_elems};
    for (int b0 = 0; b0 < n_frames; b0 += LP_FRAMES_PER_LAUNCH) {
        const int nb = std::min(LP_FRAMES_PER_LAUNCH, n_frames - b0);
        GateTable tab = {};
        for (int k = 0; k < nb; ++k) {
            const int s = stream_of[b0 + k];
            if (s < 0) tab.f[k] = GateFrame{nullptr, nullptr, 0, 0, 0, -1, 0, 0};
            else tab.f[k] = GateFrame{nullptr, desc[b0 + k].blocks, 0, desc[b0 + k].h0, desc[b0 + k].w0, s, n_tiles[s], 0};
        }
        const dim3 grid((unsigned)max_tiles, (unsigned)nb);
        const size_t o = (size_t)b0 * max_tiles;
        if (with_gain)
            hipLaunchKernelGGL(gate_update_gain_kernel, grid, dim3(TG_T), 0, st, tab, tiles, ref, age, p, gain_lo, gain_hi, flag + o, ncell + o, gain + o);
        else
            hipLaunchKernelGGL(gate_update_kernel, grid, dim3(TG_T), 0, st, tab, tiles, ref, age, p, flag + o, ncell + o);
        LP_HIP_CHECK(hipGetLastError());
    }
    return LP_OK;
}

extern "C" int lp_tile_gate_update(const lp_tile_gate_desc* desc, int n_frames, const int* stream_of, int n_streams, const int32_t* tiles,
                                   const int* n_tiles, int max_tiles, unsigned short* ref, long long ref_elems, int32_t* age, int thres16,
                                   int min_cells, int refresh, unsigned char* flag, int32_t* ncell, void* stream) {
    return gate_update("lp_tile_gate_update: ", false, desc, n_frames, stream_of, n_streams, tiles, n_tiles, max_tiles, ref, ref_elems, age, thres16,
                       min_cells, refresh, 0, 0, flag, ncell, nullptr, stream);
}

extern "C" int lp_tile_gate_update_gain(const lp_tile_gate_desc* desc, int n_frames, const int* stream_of, int n_streams, const int32_t* tiles,
                                        const int* n_tiles, int max_tiles, unsigned short* ref, long long ref_elems, int32_t* age, int thres16,
                                        int min_cells, int refresh, int gain_lo, int gain_hi, unsigned char* flag, int32_t* ncell, int32_t* gain,
                                        void* stream) {
    return gate_update("lp_tile_gate_update_gain: ", true, desc, n_frames, stream_of, n_streams, tiles, n_tiles, max_tiles, ref, ref_elems, age,
                       thres16, min_cells, refresh, gain_lo, gain_hi, flag, ncell, gain, stream);
}
