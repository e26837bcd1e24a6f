// Scene overlay in place: lp_overlay_scene_batch (include/lp_hip.h).  The lines and zones of lp_zone_update, their totals,
// occupancies and dwell alerts, and a km/h tag per drawn plate from lp_speed_update's rows are painted into BGR frames or into the
// two planes of NV12 frames, from device-resident inputs, with no host read.  The written-down specification is
// yolov6/utils/scene.py::draw_scene_np, in the same operation order (fp64 geometry without fused multiply-adds:
// -ffp-contract=off; integer blends), so the two agree byte for byte (tests/test_scene_gpu.py).  The blend, the chroma weight,
// the segment test and the label layers are those of lp_overlay.hip: lp_overlay_paint.inc holds the one copy.
//
// The ownership structure is lp_overlay.hip's: an in-place painter's algorithm whose hazard is removed by giving every pixel one
// owner.
//   scene_setup_kernel: a thread per (frame, shape) -- 8 zones, 16 lines -- and a thread per (frame, row).  It resolves the frame's
//     stream, reads the stream's map words, decides colours and opacities from occ and the events, formats the decimal glyph
//     strings, looks the row's slot up in speed_i, and writes fixed-size records with their clamped scan rectangles.
//   scene_draw_kernel: one 256-thread workgroup per frame-anchored 32 x 32 tile, a thread per 2 x 2 pixel block.  The frame's 72
//     shape layers (8 fills, 8 outlines, 16 x (segment, marker), 8 zone labels, 16 line labels: their index order IS the layer
//     order) and then its tags in chunks of 256 rows are culled against the tile into an LDS list; a tile with no survivor returns
//     before it reads a pixel.  Otherwise the zones' vertices are staged in LDS as doubles, a thread loads its block once, walks
//     the list in order blending in registers, and stores the block once if any weight was non-zero.  The fill tests every pixel:
//     no tile-wide shortcut is taken.
// Descriptors, streams and the style travel by value in the kernel arguments: nothing is uploaded, no host sync, capturable.
#include <algorithm>
#include <string>

#include "lp_internal.h"

namespace lp {

std::string redact_desc_fault(const lp_redact_desc& d);      // lp_redact.hip: the rules of one descriptor

namespace {

#include "lp_plate_quad.inc"

#include "lp_overlay_paint.inc"

constexpr int SC_ZONES = LP_ZONE_MAX_ZONES, SC_LINES = LP_ZONE_MAX_LINES, SC_VERTS = LP_ZONE_MAX_VERTS;
constexpr int SC_SHAPES = SC_ZONES + SC_LINES;                 // setup threads per frame before the rows: zones, then lines
// layer index = position in the painting order
constexpr int SC_FILL = 0, SC_OUTLINE = SC_FILL + SC_ZONES, SC_LINE = SC_OUTLINE + SC_ZONES, SC_ZLABEL = SC_LINE + 2 * SC_LINES,
              SC_LLABEL = SC_ZLABEL + SC_ZONES, SC_LAYERS = SC_LLABEL + SC_LINES;      // 72
constexpr int MAP_LINES = 16, MAP_ZHDR = 80, MAP_VERTS = 112;  // the layout of yolov6/utils/zones.py
constexpr int SC_TAG_GLYPHS = 8;                               // (2^31 - 1) mm/s is 7730941 km/h

struct ScStreams { int s[LP_FRAMES_PER_LAUNCH]; };             // the stream of each frame of a launch; < 0: the frame is skipped

// the style as the kernels take it: colours packed in the frame's own bytes
struct ScStyle {
    double hw, hw2, mm;                 // t / 2, its square, marker^2
    int t, marker, pad;
    int a_fill, a_fill_busy, a_line, a_plate, a_text;
    unsigned zone, alert, line, mark, plate, text, tag;
    int n_glyphs, gh, gw;
};
static_assert(sizeof(OvTable) + sizeof(ScStreams) + sizeof(ScStyle) + 256 < 4096, "tables and style travel as kernel arguments: under 4 KiB");

struct ScLabel {
    int ly, lx, n, spare;               // origin before clipping, glyphs
    unsigned short glyph[LP_SCENE_MAX_GLYPHS];
};
// one per frame
struct ScFrame {
    OvRect rect[SC_LAYERS];             // scan rectangle per layer
    float vert[SC_ZONES][SC_VERTS][2];
    float line[SC_LINES][4];
    int zn[SC_ZONES];                   // vertices of a drawn zone, else 0
    int zw[SC_ZONES];                   // fill weight
    unsigned zcol[SC_ZONES];
    ScLabel label[SC_SHAPES];           // zones, then lines
};
static_assert(sizeof(ScFrame) % 16 == 0 && sizeof(ScLabel) % 8 == 0, "records keep 16-byte alignment");
// one per (frame, row)
struct ScTag {
    int ly, lx, n, spare;
    unsigned short glyph[SC_TAG_GLYPHS];
};
static_assert(sizeof(ScTag) == 32, "tags are 32 bytes");

__device__ __forceinline__ OvRect rect_or_empty(int i0, int i1, int j0, int j1) {
    if (i0 >= i1 || j0 >= j1) return {0, 0, 0, 0};
    return {i0, i1, j0, j1};
}

// the decimal digits of v appended at g[n]
__device__ __forceinline__ int put_dec(unsigned short* g, int n, unsigned v) {
    int nd = 1;
    for (unsigned q = v; q >= 10u; q /= 10u) ++nd;
    for (int k = n + nd - 1; k >= n; --k) { g[k] = (unsigned short)(v % 10u); v /= 10u; }
    return n + nd;
}

// the glyphs of a name: up to the first 0xFFFF, at most 12; an index past the atlas shows '?'
__device__ __forceinline__ int put_name(unsigned short* g, const uint16_t* __restrict__ name, int n_glyphs) {
    int n = 0;
    if (name)
        for (; n < LP_SCENE_MAX_NAME; ++n) {
            const unsigned short v = name[n];
            if (v == 0xFFFFu) break;
            g[n] = (int)v < n_glyphs ? v : (unsigned short)12;
        }
    return n;
}

// a label of n glyphs anchored at the point (x, y): overlay.label_origin of the one-point polygon; returns its clipped rectangle
__device__ __forceinline__ OvRect place_label(ScLabel* lb, int n, double x, double y, const ScStyle& S, int h0, int w0) {
    const int W = n * S.gw + 2 * S.pad, H = S.gh + 2 * S.pad;
    const int ax = bound20(floor(x)), ay0 = bound20(floor(y)), ay1 = bound20(ceil(y));
    const int q = (S.t + 1) / 2;
    int ly = ay0 - q - H;
    if (ly < 0) ly = ay1 + q;
    const int lx = max(min(ax, w0 - W), 0);
    lb->ly = ly; lb->lx = lx; lb->n = n; lb->spare = 0;
    return rect_or_empty(max(ly, 0), min(ly + H, h0), lx, min(lx + W, w0));
}

__device__ __forceinline__ OvRect grown_rect(double x0, double x1, double y0, double y1, double by, int h0, int w0) {
    return rect_or_empty(clamp_to(floor(y0 - by), h0), clamp_to(ceil(y1 + by), h0), clamp_to(floor(x0 - by), w0), clamp_to(ceil(x1 + by), w0));
}

// grid (ceil((24 + max_det) / 256), frames of this launch), block 256: thread k < 8 is zone k, k < 24 line k - 8, else row k - 24 of
// frame blockIdx.y.  det, count, tid, status, heads, tags and trects start at the launch's first frame.  max_det is 0 without tags.
__global__ __launch_bounds__(256) void scene_setup_kernel(const OvTable tab, const ScStreams str, const ScStyle S, const int32_t* __restrict__ packed,
                                                          const int32_t* __restrict__ totals, const int32_t* __restrict__ occ,
                                                          const int32_t* __restrict__ zone_ev, const int32_t* __restrict__ zone_count, int max_events,
                                                          const int32_t* __restrict__ speed_i, int T, const float* __restrict__ det,
                                                          const int32_t* __restrict__ count, const int32_t* __restrict__ tid, int max_det,
                                                          const uint16_t* __restrict__ names, int32_t* __restrict__ status,
                                                          ScFrame* __restrict__ heads, ScTag* __restrict__ tags, OvRect* __restrict__ trects) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= SC_SHAPES + max_det) return;
    const int b = blockIdx.y, s = str.s[b];
    const int h0 = tab.f[b].h0, w0 = tab.f[b].w0;
    ScFrame* F = heads + b;
    const int32_t* map = packed + (long long)(s < 0 ? 0 : s) * LP_ZONE_MAP_WORDS;
    const OvRect none = {0, 0, 0, 0};
    if (k < SC_ZONES) {                                                   // zone k: fill, outline, label
        const int z = k;
        int n = 0;
        if (s >= 0 && z < map[1]) n = map[MAP_ZHDR + 4 * z];
        if (n < 3 || n > SC_VERTS) n = 0;                                 // zones.check_packed refuses such a map; nothing is drawn
        double x0 = 0.0, x1 = 0.0, y0 = 0.0, y1 = 0.0;
        for (int v = 0; v < SC_VERTS; ++v) {
            float x = 0.0f, y = 0.0f;
            if (v < n) {
                x = __int_as_float(map[MAP_VERTS + 32 * z + 2 * v]);
                y = __int_as_float(map[MAP_VERTS + 32 * z + 2 * v + 1]);
                x0 = v ? fmin(x0, (double)x) : (double)x; x1 = v ? fmax(x1, (double)x) : (double)x;
                y0 = v ? fmin(y0, (double)y) : (double)y; y1 = v ? fmax(y1, (double)y) : (double)y;
            }
            F->vert[z][v][0] = x; F->vert[z][v][1] = y;
        }
        bool busy = false, alert = false;
        if (n && occ) busy = occ[s * SC_ZONES + z] > 0;
        if (n && zone_ev) {
            const int ne = min(max(zone_count[s], 0), max_events);
            const int32_t* ev = zone_ev + (long long)s * max_events * 12;
            for (int e = 0; e < ne; ++e)
                if (ev[12 * e] == 4 && ev[12 * e + 1] == z) alert = true;
        }
        F->zn[z] = n;
        F->zw[z] = (busy ? S.a_fill_busy : S.a_fill) * 255;
        F->zcol[z] = alert ? S.alert : S.zone;
        F->rect[SC_FILL + z] = n ? grown_rect(x0, x1, y0, y1, 0.0, h0, w0) : none;
        F->rect[SC_OUTLINE + z] = n && S.t > 0 ? grown_rect(x0, x1, y0, y1, S.hw, h0, w0) : none;
        OvRect lr = none;
        ScLabel* lb = &F->label[z];
        lb->ly = lb->lx = lb->n = lb->spare = 0;
        if (n && totals) {
            int ng = put_name(lb->glyph, names ? names + ((long long)s * SC_SHAPES + SC_LINES + z) * LP_SCENE_MAX_NAME : nullptr, S.n_glyphs);
            lb->glyph[ng++] = 11;
            ng = put_dec(lb->glyph, ng, (unsigned)occ[s * SC_ZONES + z]);
            lr = place_label(lb, ng, (double)F->vert[z][0][0], (double)F->vert[z][0][1], S, h0, w0);
        }
        F->rect[SC_ZLABEL + z] = lr;
    } else if (k < SC_SHAPES) {                                           // line l: segment, marker, label
        const int l = k - SC_ZONES;
        const bool live = s >= 0 && l < min(map[0], SC_LINES);
        float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (live)
            for (int c = 0; c < 4; ++c) a[c] = __int_as_float(map[MAP_LINES + 4 * l + c]);
        for (int c = 0; c < 4; ++c) F->line[l][c] = a[c];
        const double ax = a[0], ay = a[1], bx = a[2], by = a[3];
        F->rect[SC_LINE + 2 * l] = live && S.t > 0 ? grown_rect(fmin(ax, bx), fmax(ax, bx), fmin(ay, by), fmax(ay, by), S.hw, h0, w0) : none;
        const double mx = (ax + bx) * 0.5, my = (ay + by) * 0.5;
        F->rect[SC_LINE + 2 * l + 1] = live && S.marker > 0 ? grown_rect(mx, mx, my, my, (double)S.marker, h0, w0) : none;
        OvRect lr = none;
        ScLabel* lb = &F->label[SC_ZONES + l];
        lb->ly = lb->lx = lb->n = lb->spare = 0;
        if (live && totals) {
            int ng = put_name(lb->glyph, names ? names + ((long long)s * SC_SHAPES + l) * LP_SCENE_MAX_NAME : nullptr, S.n_glyphs);
            lb->glyph[ng++] = 11; lb->glyph[ng++] = 13;
            ng = put_dec(lb->glyph, ng, (unsigned)totals[(s * 2 + 0) * SC_LINES + l]);
            lb->glyph[ng++] = 11; lb->glyph[ng++] = 14;
            ng = put_dec(lb->glyph, ng, (unsigned)totals[(s * 2 + 1) * SC_LINES + l]);
            lr = place_label(lb, ng, bx, by, S, h0, w0);
        }
        F->rect[SC_LLABEL + l] = lr;
    } else {                                                              // row r: the speed tag
        const int r = k - SC_SHAPES;
        const long long g = (long long)b * max_det + r;
        OvRect rc = none;
        int st = 0;
        ScTag* tg = tags + g;
        tg->ly = tg->lx = tg->n = tg->spare = 0;
        const int id = tid[g];
        if (s >= 0 && r < clamp_count(count[b], max_det) && id >= 0) {
            double x[4], y[4];
            if (plate_quad(det + g * LP_DET_COLS, x, y) != 3) {
                const int32_t* rows = speed_i + (long long)s * T * 8;
                int speed = -1;
                for (int t = 0; t < T; ++t)
                    if (rows[8 * t] == id && rows[8 * t + 1] >= 0) { speed = rows[8 * t + 1]; break; }      // the lowest slot wins
                if (speed >= 0) {
                    st = 1;
                    const unsigned kmh = (unsigned)(((long long)speed * 36 + 5000) / 10000);
                    const int n = put_dec(tg->glyph, 0, kmh);
                    const int W = n * S.gw + 2 * S.pad, H = S.gh + 2 * S.pad;
                    const int bx1 = bound20(ceil(fmax(fmax(x[0], x[1]), fmax(x[2], x[3]))));
                    const int by0 = bound20(floor(fmin(fmin(y[0], y[1]), fmin(y[2], y[3]))));
                    const int ly = by0, lx = max(min(bx1 + (S.t + 1) / 2, w0 - W), 0);
                    tg->ly = ly; tg->lx = lx; tg->n = n;
                    rc = rect_or_empty(max(ly, 0), min(ly + H, h0), lx, min(lx + W, w0));
                }
            }
        }
        status[g] = st;
        trects[g] = rc;
    }
}

// the crossing number of yolov6/utils/zones.py::_toggles over the n edges of a zone staged in LDS; fp64 op by op
__device__ __forceinline__ bool in_zone(const double* __restrict__ vx, const double* __restrict__ vy, int n, double px, double py) {
    unsigned par = 0u;
    for (int e = 0; e < n; ++e) {
        const int e1 = e + 1 == n ? 0 : e + 1;
        const double xi = vx[e], yi = vy[e], xj = vx[e1], yj = vy[e1];
        if ((yi > py) != (yj > py)) {
            const double a = (xj - xi) * (py - yi);
            const double c = (px - xi) * (yj - yi);
            const double t = a - c;
            if (yj > yi ? t > 0.0 : t < 0.0) par ^= 1u;
        }
    }
    return par != 0u;
}

// one shape layer (uniform across the workgroup) onto the block at (i, j)
template <bool NV12>
__device__ __forceinline__ void draw_layer(Block<NV12>& blk, int layer, const ScFrame* __restrict__ F, const ScStyle& S, const double (*vx)[SC_VERTS],
                                           const double (*vy)[SC_VERTS], const unsigned char* __restrict__ atlas, int h0, int w0, int i, int j) {
    const OvRect rc = F->rect[layer];
    const int r4[4] = {rc.i0, rc.i1, rc.j0, rc.j1};
    if (!touches(r4, i, j)) return;
    int w[4];
    if (layer < SC_LINE) {                                                // a zone's fill or outline
        const bool fill = layer < SC_OUTLINE;
        const int z = fill ? layer - SC_FILL : layer - SC_OUTLINE;
        const int n = F->zn[z], wt = fill ? F->zw[z] : S.a_line * 255;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int pi = i + (k >> 1), pj = j + (k & 1);
            const double px = (double)pj + 0.5, py = (double)pi + 0.5;
            bool hit = false;
            if (inside(r4, pi, pj)) {
                if (fill) hit = in_zone(vx[z], vy[z], n, px, py);
                else
                    for (int e = 0; e < n; ++e) {
                        const int e1 = e + 1 == n ? 0 : e + 1;
                        hit = hit || on_segment(vx[z][e], vy[z][e], vx[z][e1], vy[z][e1], S.hw2, px, py);
                    }
            }
            w[k] = hit ? wt : 0;
        }
        blk.apply(w, F->zcol[z]);
    } else if (layer < SC_ZLABEL) {                                       // a line's segment or marker
        const int l = (layer - SC_LINE) >> 1;
        const bool marker = (layer - SC_LINE) & 1;
        const double ax = F->line[l][0], ay = F->line[l][1], bx = F->line[l][2], by = F->line[l][3];
        const double mx = (ax + bx) * 0.5, my = (ay + by) * 0.5;
        const double ex = bx - ax, ey = by - ay;
        const double L = ex * ex + ey * ey;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int pi = i + (k >> 1), pj = j + (k & 1);
            const double px = (double)pj + 0.5, py = (double)pi + 0.5;
            bool hit = false;
            if (inside(r4, pi, pj)) {
                if (marker) {
                    const double dx = px - mx, dy = py - my;
                    const double s = ex * dy - ey * dx;
                    const double u = dx * ex + dy * ey;
                    const double q = fabs(u) + s;
                    hit = L > 0.0 && s >= 0.0 && q * q <= S.mm * L;
                } else {
                    hit = on_segment(ax, ay, bx, by, S.hw2, px, py);
                }
            }
            w[k] = hit ? S.a_line * 255 : 0;
        }
        blk.apply(w, marker ? S.mark : S.line);
    } else {                                                              // a zone's or a line's label
        const ScLabel* lb = &F->label[layer - SC_ZLABEL];
        draw_label(blk, r4, lb->ly, lb->lx, S.pad, lb->n, lb->glyph, S.a_plate * 255, S.plate, S.a_text, S.text, atlas, S.gh, S.gw, h0, w0, i, j);
    }
}

// grid (most tiles of a frame of this launch, frames of this launch), block 256.  count, heads, tags and trects start at the launch's
// first frame.
template <bool NV12>
__global__ __launch_bounds__(256) void scene_draw_kernel(const OvTable tab, const ScStyle S, const int32_t* __restrict__ count, int max_det,
                                                         const ScFrame* __restrict__ heads, const ScTag* __restrict__ tags,
                                                         const OvRect* __restrict__ trects, const unsigned char* __restrict__ atlas) {
    __shared__ unsigned short list[256];
    __shared__ int wave_hits[4];
    __shared__ double vx[SC_ZONES][SC_VERTS], vy[SC_ZONES][SC_VERTS];
    const OvEntry f = tab.f[blockIdx.y];
    const int tiles_x = (f.w0 + OV_TILE - 1) / OV_TILE, tiles_y = (f.h0 + OV_TILE - 1) / OV_TILE;
    if ((long long)blockIdx.x >= (long long)tiles_x * tiles_y) return;
    const ScFrame* F = heads + blockIdx.y;
    const int n_rows = max_det > 0 ? clamp_count(count[blockIdx.y], max_det) : 0;
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
    // chunk -1: the 72 shape layers, in layer order; chunks 0..: the tags, 256 rows at a time, in row order
    for (int base = -256; base < n_rows; base += 256) {
        const bool shapes = base < 0;
        bool hit = false;
        if (shapes ? t < SC_LAYERS : base + t < n_rows) {
            const OvRect rc = shapes ? F->rect[t] : trects[row0 + base + t];      // all zeros for a layer that draws nothing
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
        if (shapes && total > 0) {                                        // total is the same in every thread
            const float v = F->vert[t >> 5][(t >> 1) & 15][t & 1];        // 8 x 16 x 2 floats: one per thread
            if (t & 1) vy[t >> 5][(t >> 1) & 15] = (double)v;
            else vx[t >> 5][(t >> 1) & 15] = (double)v;
        }
        __syncthreads();
        if (total > 0) {
            if (!loaded) {
                blk.load(f, i, j, ok);
                loaded = true;
            }
            if (ok[0])
                for (int k = 0; k < total; ++k) {
                    const int item = __builtin_amdgcn_readfirstlane((int)list[k]);           // the same layer in every lane
                    if (shapes) {
                        draw_layer<NV12>(blk, item, F, S, vx, vy, atlas, f.h0, f.w0, i, j);
                    } else {
                        const long long g = row0 + base + item;
                        const OvRect rc = trects[g];
                        const int r4[4] = {rc.i0, rc.i1, rc.j0, rc.j1};
                        const ScTag* tg = tags + g;
                        draw_label(blk, r4, tg->ly, tg->lx, S.pad, tg->n, tg->glyph, S.a_plate * 255, S.tag, S.a_text, S.text, atlas, S.gh, S.gw,
                                   f.h0, f.w0, i, j);
                    }
                }
        }
        __syncthreads();                                                  // the list is rewritten by the next chunk
    }
    if (blk.dirty) blk.store(f, i, j, ok);
}

std::string scene_style_fault(const lp_scene_style& s) {
    if (s.t < 0 || s.t > LP_OVERLAY_MAX_THICKNESS) return "t must be in 0..16";
    if (s.marker < 0 || s.marker > LP_SCENE_MAX_MARKER) return "marker must be in 0..64";
    if (s.pad < 0 || s.pad > LP_OVERLAY_MAX_PAD) return "pad must be in 0..16";
    for (int a : {s.a_fill, s.a_fill_busy, s.a_line, s.a_plate, s.a_text})
        if (a < 0 || a > 256) return "opacities must be in 0..256";
    if (s.n_glyphs < LP_SCENE_FIXED_GLYPHS || s.n_glyphs > LP_OVERLAY_MAX_ATLAS) return "n_glyphs must be in 17..1024 (the atlas is too small)";
    if (s.gh < 1 || s.gh > LP_OVERLAY_MAX_CELL || s.gw < 1 || s.gw > LP_OVERLAY_MAX_CELL) return "gh, gw must be in 1..64";
    return "";
}

}  // namespace

}  // namespace lp

using namespace lp;

extern "C" size_t lp_overlay_scene_workspace_bytes(int n_frames, int max_det) {
    if (n_frames < 1 || max_det < 0) return 0;
    return (size_t)n_frames * sizeof(ScFrame) + (size_t)n_frames * (size_t)max_det * (sizeof(ScTag) + sizeof(OvRect));
}

extern "C" int lp_overlay_scene_batch(const lp_redact_desc* desc, int n_frames, const int32_t* stream_of, int n_streams, const int32_t* packed,
                                      const int32_t* totals, const int32_t* occ, const int32_t* zone_ev, const int32_t* zone_count,
                                      int max_events, const int32_t* speed_i, int max_tracks, const float* det, const int32_t* count,
                                      const int32_t* tid, int max_det, const lp_scene_style* p, const unsigned char* atlas,
                                      const uint16_t* names, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    const std::string fn = "lp_overlay_scene_batch: ";
    if (n_frames < 0 || !desc || !p || !atlas || !packed || n_streams < 1)
        return fail(LP_ERR_ARG, fn + "bad arguments (need desc, packed, p, atlas, n_frames >= 0, n_streams >= 1)");
    if ((totals == nullptr) != (occ == nullptr)) return fail(LP_ERR_ARG, fn + "totals and occ come together");
    if ((zone_ev == nullptr) != (zone_count == nullptr)) return fail(LP_ERR_ARG, fn + "zone_ev and zone_count come together");
    if (zone_ev && max_events < 1) return fail(LP_ERR_ARG, fn + "max_events must be >= 1");
    const int given = (speed_i != nullptr) + (det != nullptr) + (count != nullptr) + (tid != nullptr) + (status != nullptr);
    if (given != 0 && given != 5) return fail(LP_ERR_ARG, fn + "speed_i, det, count, tid and status come together");
    const bool tagged = given == 5;
    if (tagged && max_tracks < 1) return fail(LP_ERR_ARG, fn + "max_tracks must be >= 1");
    if (tagged && max_det < 1) return fail(LP_ERR_ARG, fn + "max_det must be >= 1");
    const std::string why = scene_style_fault(*p);
    if (!why.empty()) return fail(LP_ERR_ARG, fn + why);
    for (int b = 0; b < n_frames; ++b) {       // every frame is checked before the first launch
        const std::string bad = redact_desc_fault(desc[b]);
        if (!bad.empty()) return fail(LP_ERR_ARG, fn + bad + " (frame " + std::to_string(b) + ")");
    }
    if (n_frames == 0) return LP_OK;
    const int rows = tagged ? max_det : 0;
    const size_t need = lp_overlay_scene_workspace_bytes(n_frames, rows);
    if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < need)
        return fail(LP_ERR_ARG, fn + "workspace must be 16-byte aligned and hold " + std::to_string(need) + " bytes");
    hipStream_t st = (hipStream_t)stream;
    ScFrame* heads = (ScFrame*)workspace;
    OvRect* trects = (OvRect*)(heads + n_frames);
    ScTag* tags = (ScTag*)(trects + (size_t)n_frames * rows);
    ScStyle S = {};
    S.hw = 0.5 * (double)p->t; S.hw2 = S.hw * S.hw; S.mm = (double)p->marker * (double)p->marker;
    S.t = p->t; S.marker = p->marker; S.pad = p->pad;
    S.a_fill = p->a_fill; S.a_fill_busy = p->a_fill_busy; S.a_line = p->a_line; S.a_plate = p->a_plate; S.a_text = p->a_text;
    auto pk = [](const unsigned char c[3]) { return (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16); };
    S.zone = pk(p->zone); S.alert = pk(p->alert); S.line = pk(p->line); S.mark = pk(p->mark); S.plate = pk(p->plate); S.text = pk(p->text);
    S.tag = pk(p->tag);
    S.n_glyphs = p->n_glyphs; S.gh = p->gh; S.gw = p->gw;
    // a launch pair = a run of at most LP_FRAMES_PER_LAUNCH consecutive frames of one format
    int b = 0;
    while (b < n_frames) {
        OvTable tab = {};
        ScStreams str = {};
        const int b0 = b, format = desc[b].format;
        long long tiles = 0;
        int nf = 0;
        for (; b < n_frames && nf < LP_FRAMES_PER_LAUNCH && desc[b].format == format; ++b, ++nf) {
            const lp_redact_desc& d = desc[b];
            tab.f[nf] = {d.p0, d.p1, d.pitch0, d.pitch1, d.h0, d.w0};
            const int s = stream_of ? stream_of[b] : b;
            str.s[nf] = s >= 0 && s < n_streams ? s : -1;
            tiles = std::max(tiles, (long long)ceil_div(d.h0, OV_TILE) * ceil_div(d.w0, OV_TILE));
        }
        if (tiles > 0x7fffffffLL) return fail(LP_ERR_ARG, fn + "frame too large (frame " + std::to_string(b0) + ")");
        const size_t off = (size_t)b0 * rows;
        hipLaunchKernelGGL(scene_setup_kernel, dim3((unsigned)ceil_div(SC_SHAPES + rows, 256), (unsigned)nf), dim3(256), 0, st, tab, str, S, packed,
                           totals, occ, zone_ev, zone_count, max_events, speed_i, max_tracks, tagged ? det + off * LP_DET_COLS : nullptr,
                           tagged ? count + b0 : nullptr, tagged ? tid + off : nullptr, rows, names, tagged ? status + off : nullptr, heads + b0,
                           tags + off, trects + off);
        LP_HIP_CHECK(hipGetLastError());
        const dim3 grid((unsigned)tiles, (unsigned)nf);
        if (format == 1)
            hipLaunchKernelGGL(scene_draw_kernel<true>, grid, dim3(256), 0, st, tab, S, tagged ? count + b0 : nullptr, rows, heads + b0, tags + off,
                               trects + off, atlas);
        else
            hipLaunchKernelGGL(scene_draw_kernel<false>, grid, dim3(256), 0, st, tab, S, tagged ? count + b0 : nullptr, rows, heads + b0, tags + off,
                               trects + off, atlas);
        LP_HIP_CHECK(hipGetLastError());
    }
    return LP_OK;
}
