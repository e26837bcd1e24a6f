// Skipping the unchanged tiles of fixed-camera frames in tiled detection: lp_tile_gate_luma_batch and lp_tile_gate_update
// (include/lp_hip.h).  The reference has nothing here; the written-down specification is yolov6/utils/tile_gate.py
// (luma_blocks_np, gate_update_np), which these kernels match on every integer (tests/test_tile_gate_gpu.py).  Everything is
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

extern "C" int lp_tile_gate_update(const lp_tile_gate_desc* desc, int n_frames, const int* stream_of, int n_streams, const int32_t* tiles,
                                   const int* n_tiles, int max_tiles, unsigned short* ref, long long ref_elems, int32_t* age, int thres16,
                                   int min_cells, int refresh, unsigned char* flag, int32_t* ncell, void* stream) {
    const std::string fn = "lp_tile_gate_update: ";
    if (n_frames < 0 || n_streams < 1) return fail(LP_ERR_ARG, fn + "need n_frames >= 0 and n_streams >= 1");
    if (max_tiles < 1 || max_tiles > LP_MERGE_MAX_TILES)
        return fail(LP_ERR_ARG, fn + "max_tiles " + std::to_string(max_tiles) + " (need 1.." + std::to_string(LP_MERGE_MAX_TILES) + " tiles per frame)");
    if ((long long)n_streams * max_tiles * LP_TILE_GATE_TILE_WORDS >= 0x80000000ll) return fail(LP_ERR_ARG, fn + "n_streams * max_tiles * 8 must stay below 2^31");
    if (thres16 < 0 || thres16 > TG_MAX_THRES16 || min_cells < 1 || refresh < 0)
        return fail(LP_ERR_ARG, fn + "need thres16 in 0.." + std::to_string(TG_MAX_THRES16) + ", min_cells >= 1 and refresh >= 0");
    if (ref_elems < 1 || ref_elems >= 0x80000000ll) return fail(LP_ERR_ARG, fn + "ref_elems " + std::to_string(ref_elems) + " (need 1..2^31-1)");
    if (!tiles || !n_tiles || !ref || !age) return fail(LP_ERR_ARG, fn + "null pointer");
    if (((uintptr_t)tiles & 3) != 0 || ((uintptr_t)ref & 1) != 0 || ((uintptr_t)age & 3) != 0 || ((uintptr_t)ncell & 3) != 0)
        return fail(LP_ERR_ARG, fn + "tiles, age and ncell must be 4-byte and ref 2-byte aligned");
    for (int s = 0; s < n_streams; ++s)
        if (n_tiles[s] < 0 || n_tiles[s] > max_tiles)
            return fail(LP_ERR_ARG, fn + "stream " + std::to_string(s) + " has " + std::to_string(n_tiles[s]) + " tiles (need 0.." + std::to_string(max_tiles) + ")");
    if (n_frames == 0) return LP_OK;
    if (!desc || !stream_of || !flag || !ncell) return fail(LP_ERR_ARG, fn + "null pointer");
    {
        const std::string why = stream_of_fault(stream_of, n_frames, n_streams);
        if (!why.empty()) return fail(LP_ERR_ARG, fn + why);
    }
    const size_t slots = (size_t)n_streams * max_tiles, outs = (size_t)n_frames * max_tiles;
    std::vector<Region> reg = {{tiles, slots * LP_TILE_GATE_TILE_WORDS * 4, false}, {ref, (size_t)ref_elems * 2, true}, {age, slots * 4, true},
                               {flag, outs, true}, {ncell, outs * 4, true}};
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
        return fail(LP_ERR_ARG, fn + "ref, age, flag and ncell may overlap neither an input nor each other");
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
        hipLaunchKernelGGL(gate_update_kernel, dim3((unsigned)max_tiles, (unsigned)nb), dim3(TG_T), 0, st, tab, tiles, ref, age, p,
                           flag + (size_t)b0 * max_tiles, ncell + (size_t)b0 * max_tiles);
        LP_HIP_CHECK(hipGetLastError());
    }
    return LP_OK;
}
