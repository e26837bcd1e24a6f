// Annotation overlay in place: lp_overlay_draw_batch (include/lp_hip.h).  Every detection row of a frame is drawn onto it: the
// outline of its box, the outline of its corner quad, a label plate and the label's glyphs (track id and the eight heads'
// characters, from a caller-supplied coverage atlas), into a BGR frame or into the two planes of an NV12 frame.  The reference
// draws nothing; the written-down specification is yolov6/utils/overlay.py::draw_plates_np, in the same operation order (fp64
// geometry without fused multiply-adds: -ffp-contract=off; integer blends), so the two agree byte for byte
// (tests/test_overlay_gpu.py).  The quad of a row is the rule of the crops and of the redaction, lp_plate_quad.inc; the blend, the
// 2 x 2 block, the segment test and the label layers are lp_overlay_paint.inc, shared with the scene overlay (lp_overlay_scene.hip).
//
// Rows are painted in row order, a later row over an earlier one, and a row's layers in the order box, quad, plate, glyphs: an
// in-place painter's algorithm, whose hazard (two rows touching one pixel from two workgroups) is removed by the structure.
//   overlay_setup_kernel: one thread per (frame, row).  It reads the row once, runs the quad rule and all the fp64 set-up, resolves
//     the style and the palette, composes the glyph list, and writes a fixed-size record (OvRec) plus the row's bounding
//     rectangle over all its layers into the workspace, and the row's status.
//   overlay_draw_kernel: one 256-thread workgroup per frame-anchored 32 x 32 tile, a thread per 2 x 2 pixel block (on NV12: four
//     luma pixels and their chroma sample).  In chunks of 256 rows the threads test the tile against the rows' rectangles and
//     compact the survivors in row order into an LDS list (ballot + prefix sum over the four waves); a tile with no survivor returns
//     before it reads a pixel.  Otherwise a thread loads its block once, walks the list in order blending in registers, and stores
//     the block once if any weight was non-zero.
// Every pixel is read and written by exactly one thread, once: no atomics, no per-pixel workspace, and the overlap order is the row
// order by construction.  Descriptors, styles and the palette travel by value in the kernel arguments: nothing is uploaded, no host
// sync, capturable in a graph.
#include <algorithm>
#include <string>

#include "lp_internal.h"

namespace lp {

std::string redact_desc_fault(const lp_redact_desc& d);      // lp_redact.hip: the rules of one descriptor

namespace {

#include "lp_plate_quad.inc"

#include "lp_overlay_paint.inc"

static_assert(sizeof(OvTable) + sizeof(lp_overlay_params) + 128 < 4096, "table and styles travel as kernel arguments: under 4 KiB");

// What the draw kernel needs of one row.  Rectangles are (i0, i1, j0, j1): rows [i0, i1), columns [j0, j1), clamped to the frame;
// all zeros: the layer is not drawn.
struct OvRec {
    double bx[4], by[4];                // the box as a polygon p0..p3
    double qx[4], qy[4];                // the corner quad
    double hw2;                         // (t / 2)^2
    int brect[4], qrect[4];             // scan rectangles of the two outlines
    int lrect[4];                       // the label rectangle, clipped
    int ly, lx;                         // its origin before clipping
    int n_glyph, pad;
    int a_line, a_plate, a_text, spare;
    unsigned col_box, col_quad, col_plate, col_text;      // c0 | c1 << 8 | c2 << 16, the frame's own bytes
    unsigned short glyph[LP_OVERLAY_MAX_GLYPHS];
};
static_assert(sizeof(OvRec) % 16 == 0, "records keep the rectangles behind them 16-byte aligned");

__device__ __forceinline__ double min4(const double v[4]) { return fmin(fmin(v[0], v[1]), fmin(v[2], v[3])); }
__device__ __forceinline__ double max4(const double v[4]) { return fmax(fmax(v[0], v[1]), fmax(v[2], v[3])); }

// the scan rectangle of an outline: the polygon's bounds grown by hw, clamped; zeros when it is empty
__device__ __forceinline__ void outline_rect(const double x[4], const double y[4], double hw, int h0, int w0, int rc[4]) {
    rc[0] = clamp_to(floor(min4(y) - hw), h0); rc[1] = clamp_to(ceil(max4(y) + hw), h0);
    rc[2] = clamp_to(floor(min4(x) - hw), w0); rc[3] = clamp_to(ceil(max4(x) + hw), w0);
    if (rc[0] >= rc[1] || rc[2] >= rc[3]) rc[0] = rc[1] = rc[2] = rc[3] = 0;
}

__device__ __forceinline__ void grow(OvRect& u, const int rc[4]) {
    if (rc[0] >= rc[1]) return;
    if (u.i0 >= u.i1) { u = {rc[0], rc[1], rc[2], rc[3]}; return; }
    u.i0 = min(u.i0, rc[0]); u.i1 = max(u.i1, rc[1]);
    u.j0 = min(u.j0, rc[2]); u.j1 = max(u.j1, rc[3]);
}

// grid (ceil(max_det / 256), frames of this launch), block 256: thread = row r of frame blockIdx.y.  det, tid, style, status, recs
// and rects start at the launch's first frame.  Styles and the palette are picked with selects: a dynamic index into the kernel
// arguments would go through scratch.
__global__ __launch_bounds__(256) void overlay_setup_kernel(const OvTable tab, const lp_overlay_params p, const float* __restrict__ det,
                                                            const int32_t* __restrict__ count, int max_det, const int32_t* __restrict__ tid,
                                                            const int32_t* __restrict__ style, const uint16_t* __restrict__ glyph_of,
                                                            int32_t* __restrict__ status, OvRec* __restrict__ recs, OvRect* __restrict__ rects) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= max_det) return;
    const int h0 = tab.f[blockIdx.y].h0, w0 = tab.f[blockIdx.y].w0;
    const long long g = (long long)blockIdx.y * max_det + r;
    const int n = clamp_count(count[blockIdx.y], max_det);
    int sty = style ? style[g] : 0;
    OvRect u = {0, 0, 0, 0};
    int st = 0;
    if (r < n && sty >= 0) {
        const float* row = det + g * LP_DET_COLS;
        double x[4], y[4];
        st = plate_quad(row, x, y);
        if (st != 3) {
            OvRec* rec = recs + g;
            sty = sty < p.n_styles ? sty : p.n_styles - 1;
            lp_overlay_style S = p.styles[0];
#pragma unroll
            for (int k = 1; k < LP_OVERLAY_MAX_STYLES; ++k)
                if (k == sty) S = p.styles[k];
            const int id = tid ? tid[g] : -1;
            unsigned col_quad = pack3(S.quad), col_plate = pack3(S.plate);
            if (id >= 0 && p.n_palette > 0) {
                const int pi = id % p.n_palette;
                unsigned c = pack3(p.palette[0]);
#pragma unroll
                for (int k = 1; k < LP_OVERLAY_MAX_PALETTE; ++k)
                    if (k == pi) c = pack3(p.palette[k]);
                col_quad = col_plate = c;
            }
            const int t = S.t;
            const double hw = 0.5 * (double)t;
            rec->hw2 = hw * hw;
            // the box: finite with sides >= 1 px (plate_quad's box rule); drawn with a status-2 row always, else on draw_box
            const double x1 = row[0], y1 = row[1], x2 = row[2], y2 = row[3];
            const bool box_ok = isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2) && x2 - x1 >= 1.0 && y2 - y1 >= 1.0;
            const double bx[4] = {x1, x2, x2, x1}, by[4] = {y1, y1, y2, y2};
            int brect[4] = {0, 0, 0, 0}, qrect[4] = {0, 0, 0, 0}, lrect[4] = {0, 0, 0, 0};
            if (box_ok && t > 0 && (st == 2 || p.draw_box)) outline_rect(bx, by, hw, h0, w0, brect);
            if (st == 1 && t > 0) outline_rect(x, y, hw, h0, w0, qrect);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                rec->bx[k] = bx[k]; rec->by[k] = by[k];
                rec->qx[k] = x[k]; rec->qy[k] = y[k];
                rec->brect[k] = brect[k]; rec->qrect[k] = qrect[k];
            }
            int ng = 0, ly = 0, lx = 0;
            if (p.label) {
                // glyphs: '#', the digits of the id, ' ' -- then the eight heads
                if (id >= 0 && p.show_id) {
                    unsigned v = (unsigned)id;
                    int nd = 1;
                    for (unsigned q = v; q >= 10u; q /= 10u) ++nd;
                    rec->glyph[ng++] = 10;
                    for (int k = ng + nd - 1; k >= ng; --k) { rec->glyph[k] = (unsigned short)(v % 10u); v /= 10u; }
                    ng += nd;
                    rec->glyph[ng++] = 11;
                }
                for (int hd = 0; hd < 8; ++hd) {
                    const float v = row[20 + hd];
                    unsigned short gl = 12;
                    if (isfinite(v) && v >= 0.0f && v < 64.0f) {
                        gl = glyph_of[hd * 64 + (int)v];
                        if ((int)gl >= p.n_glyphs) gl = 12;
                    }
                    rec->glyph[ng++] = gl;
                }
                const int W = ng * p.gw + 2 * S.pad, H = p.gh + 2 * S.pad;
                const int bx0 = bound20(floor(min4(x))), by0 = bound20(floor(min4(y))), by1 = bound20(ceil(max4(y)));
                const int q = (t + 1) / 2;
                ly = by0 - q - H;
                if (ly < 0) ly = by1 + q;
                lx = max(min(bx0, w0 - W), 0);
                lrect[0] = max(ly, 0); lrect[1] = min(ly + H, h0);
                lrect[2] = lx; lrect[3] = min(lx + W, w0);
                if (lrect[0] >= lrect[1] || lrect[2] >= lrect[3]) lrect[0] = lrect[1] = lrect[2] = lrect[3] = 0;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) rec->lrect[k] = lrect[k];
            rec->ly = ly; rec->lx = lx;
            rec->n_glyph = ng; rec->pad = S.pad;
            rec->a_line = S.a_line; rec->a_plate = S.a_plate; rec->a_text = S.a_text; rec->spare = 0;
            rec->col_box = pack3(S.box); rec->col_quad = col_quad; rec->col_plate = col_plate; rec->col_text = pack3(S.text);
            grow(u, brect); grow(u, qrect); grow(u, lrect);
        }
    }
    status[g] = st;
    rects[g] = u;
}

// Is the centre (px, py) within sqrt(hw2) of the closed polygon p0 -> p3 -> p2 -> p1 -> p0?  on_segment (lp_overlay_paint.inc) per edge.
__device__ __forceinline__ bool on_outline(const double* __restrict__ x, const double* __restrict__ y, double hw2, double px, double py) {
    const int ord[4] = {0, 3, 2, 1};
    bool in = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool hit = on_segment(x[ord[k]], y[ord[k]], x[ord[(k + 1) & 3]], y[ord[(k + 1) & 3]], hw2, px, py);
        in = in || hit;
    }
    return in;
}

template <bool NV12>
__device__ __forceinline__ void draw_outline(Block<NV12>& blk, const int* rc, const double* x, const double* y, double hw2, int wt, unsigned col,
                                             int i, int j) {
    const int r4[4] = {rc[0], rc[1], rc[2], rc[3]};
    if (!touches(r4, i, j)) return;
    int w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int pi = i + (k >> 1), pj = j + (k & 1);
        w[k] = inside(r4, pi, pj) && on_outline(x, y, hw2, (double)pj + 0.5, (double)pi + 0.5) ? wt : 0;
    }
    blk.apply(w, col);
}

// The four layers of one row onto the block at (i, j); a rectangle lies inside the frame, so a pixel inside one is a pixel of the frame.
template <bool NV12>
__device__ __forceinline__ void draw_row(Block<NV12>& blk, const OvRec* __restrict__ R, const unsigned char* __restrict__ atlas, int gh, int gw,
                                         int h0, int w0, int i, int j) {
    draw_outline(blk, R->brect, R->bx, R->by, R->hw2, R->a_line * 255, R->col_box, i, j);
    draw_outline(blk, R->qrect, R->qx, R->qy, R->hw2, R->a_line * 255, R->col_quad, i, j);
    draw_label(blk, R->lrect, R->ly, R->lx, R->pad, R->n_glyph, R->glyph, R->a_plate * 255, R->col_plate, R->a_text, R->col_text, atlas, gh, gw,
               h0, w0, i, j);
}

// grid (most tiles of a frame of this launch, frames of this launch), block 256.  count, recs and rects start at the launch's first frame.
template <bool NV12>
__global__ __launch_bounds__(256) void overlay_draw_kernel(const OvTable tab, const int32_t* __restrict__ count, int max_det,
                                                           const OvRec* __restrict__ recs, const OvRect* __restrict__ rects,
                                                           const unsigned char* __restrict__ atlas, int gh, int gw) {
    __shared__ unsigned short list[256];
    __shared__ int wave_hits[4];
    const OvEntry f = tab.f[blockIdx.y];
    const int tiles_x = (f.w0 + OV_TILE - 1) / OV_TILE, tiles_y = (f.h0 + OV_TILE - 1) / OV_TILE;
    if ((long long)blockIdx.x >= (long long)tiles_x * tiles_y) return;
    const int n = clamp_count(count[blockIdx.y], max_det);
    if (n == 0) return;
    const int ti0 = (int)(blockIdx.x / tiles_x) * OV_TILE, tj0 = (int)(blockIdx.x % tiles_x) * OV_TILE;
    const int ti1 = min(ti0 + OV_TILE, f.h0), tj1 = min(tj0 + OV_TILE, f.w0);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int i = ti0 + 2 * (t >> 4), j = tj0 + 2 * (t & 15);
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) ok[k] = i + (k >> 1) < f.h0 && j + (k & 1) < f.w0;
    const long long row0 = (long long)blockIdx.y * max_det;
    Block<NV12> blk;
    blk.dirty = false;
    bool loaded = false;
    for (int base = 0; base < n; base += 256) {
        const int r = base + t;
        bool hit = false;
        if (r < n) {
            const OvRect rc = rects[row0 + r];                            // all zeros for a row that draws nothing
            hit = rc.i0 < ti1 && rc.i1 > ti0 && rc.j0 < tj1 && rc.j1 > tj0;
        }
        const unsigned long long bal = __ballot(hit);
        if (lane == 0) wave_hits[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int wv = 0; wv < 4; ++wv) {
            const int c = wave_hits[wv];
            before += wv < wave ? c : 0;
            total += c;
        }
        if (hit) list[before + __popcll(bal & ((1ull << lane) - 1ull))] = (unsigned short)t;
        __syncthreads();
        if (total > 0) {
            if (!loaded) {
                blk.load(f, i, j, ok);
                loaded = true;
            }
            if (ok[0])
                for (int k = 0; k < total; ++k) {
                    const int rr = __builtin_amdgcn_readfirstlane(base + (int)list[k]);      // the same row in every lane
                    draw_row<NV12>(blk, recs + row0 + rr, atlas, gh, gw, f.h0, f.w0, i, j);
                }
        }
        __syncthreads();                                                  // the list is rewritten by the next chunk
    }
    if (blk.dirty) blk.store(f, i, j, ok);
}

std::string style_fault(const lp_overlay_style& s) {
    if (s.t < 0 || s.t > LP_OVERLAY_MAX_THICKNESS) return "t must be in 0..16";
    if (s.pad < 0 || s.pad > LP_OVERLAY_MAX_PAD) return "pad must be in 0..16";
    if (s.a_line < 0 || s.a_line > 256 || s.a_plate < 0 || s.a_plate > 256 || s.a_text < 0 || s.a_text > 256) return "opacities must be in 0..256";
    return "";
}

std::string params_fault(const lp_overlay_params& p) {
    if (p.n_styles < 1 || p.n_styles > LP_OVERLAY_MAX_STYLES) return "n_styles must be in 1..8";
    for (int k = 0; k < p.n_styles; ++k) {
        const std::string why = style_fault(p.styles[k]);
        if (!why.empty()) return why + " (style " + std::to_string(k) + ")";
    }
    if (p.n_palette < 0 || p.n_palette > LP_OVERLAY_MAX_PALETTE) return "n_palette must be in 0..64";
    if (p.n_glyphs < 13 || p.n_glyphs > LP_OVERLAY_MAX_ATLAS) return "n_glyphs must be in 13..1024";
    if (p.gh < 1 || p.gh > LP_OVERLAY_MAX_CELL || p.gw < 1 || p.gw > LP_OVERLAY_MAX_CELL) return "gh, gw must be in 1..64";
    return "";
}

}  // namespace

}  // namespace lp

using namespace lp;

extern "C" size_t lp_overlay_workspace_bytes(int n_frames, int max_det) {
    if (n_frames < 1 || max_det < 1) return 0;
    return (size_t)n_frames * (size_t)max_det * (sizeof(OvRec) + sizeof(OvRect));
}

extern "C" int lp_overlay_draw_batch(const lp_redact_desc* desc, int n_frames, const float* det, const int32_t* count, int max_det,
                                     const int32_t* tid, const int32_t* style, const lp_overlay_params* p, const unsigned char* atlas,
                                     const uint16_t* glyph_of, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    const std::string fn = "lp_overlay_draw_batch: ";
    if (n_frames < 0 || !desc || !p || !status || !atlas || !glyph_of)
        return fail(LP_ERR_ARG, fn + "bad arguments (need desc, p, atlas, glyph_of, status, n_frames >= 0)");
    if (max_det < 1) return fail(LP_ERR_ARG, fn + "max_det must be >= 1");
    const std::string why = params_fault(*p);
    if (!why.empty()) return fail(LP_ERR_ARG, fn + why);
    for (int b = 0; b < n_frames; ++b) {       // every frame is checked before the first launch
        const std::string bad = redact_desc_fault(desc[b]);
        if (!bad.empty()) return fail(LP_ERR_ARG, fn + bad + " (frame " + std::to_string(b) + ")");
    }
    if (n_frames == 0) return LP_OK;
    if (!det || !count) return fail(LP_ERR_ARG, fn + "null det or count");
    const size_t need = lp_overlay_workspace_bytes(n_frames, max_det);
    if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < need)
        return fail(LP_ERR_ARG, fn + "workspace must be 16-byte aligned and hold " + std::to_string(need) + " bytes");
    hipStream_t st = (hipStream_t)stream;
    OvRec* recs = (OvRec*)workspace;
    OvRect* rects = (OvRect*)(recs + (size_t)n_frames * max_det);
    // a launch pair = a run of at most LP_FRAMES_PER_LAUNCH consecutive frames of one format
    int b = 0;
    while (b < n_frames) {
        OvTable tab = {};
        const int b0 = b, format = desc[b].format;
        long long tiles = 0;
        int nf = 0;
        for (; b < n_frames && nf < LP_FRAMES_PER_LAUNCH && desc[b].format == format; ++b, ++nf) {
            const lp_redact_desc& d = desc[b];
            tab.f[nf] = {d.p0, d.p1, d.pitch0, d.pitch1, d.h0, d.w0};
            tiles = std::max(tiles, (long long)ceil_div(d.h0, OV_TILE) * ceil_div(d.w0, OV_TILE));
        }
        if (tiles > 0x7fffffffLL) return fail(LP_ERR_ARG, fn + "frame too large (frame " + std::to_string(b0) + ")");
        const size_t off = (size_t)b0 * max_det;
        hipLaunchKernelGGL(overlay_setup_kernel, dim3((unsigned)ceil_div(max_det, 256), (unsigned)nf), dim3(256), 0, st, tab, *p,
                           det + off * LP_DET_COLS, count + b0, max_det, tid ? tid + off : nullptr, style ? style + off : nullptr, glyph_of,
                           status + off, recs + off, rects + off);
        LP_HIP_CHECK(hipGetLastError());
        const dim3 grid((unsigned)tiles, (unsigned)nf);
        if (format == 1)
            hipLaunchKernelGGL(overlay_draw_kernel<true>, grid, dim3(256), 0, st, tab, count + b0, max_det, recs + off, rects + off, atlas, p->gh, p->gw);
        else
            hipLaunchKernelGGL(overlay_draw_kernel<false>, grid, dim3(256), 0, st, tab, count + b0, max_det, recs + off, rects + off, atlas, p->gh, p->gw);
        LP_HIP_CHECK(hipGetLastError());
    }
    return LP_OK;
}
