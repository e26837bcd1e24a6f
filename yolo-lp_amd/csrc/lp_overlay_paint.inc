// What the two in-place painters share (lp_overlay.hip: the detections; lp_overlay_scene.hip: lines, zones and speed tags); include
// inside an unnamed namespace of namespace lp, one copy of each rule.  The specification is yolov6/utils/overlay.py: ``blend``,
// ``chroma_weight``, ``segment_mask`` and the label's plate and glyph layers.  A painter gives every pixel one owner: a 256-thread
// workgroup per frame-anchored 32 x 32 tile, a thread per 2 x 2 pixel block (on NV12: four luma pixels and their chroma sample),
// which loads its block once, blends the layers in order in registers and stores it once.
constexpr int OV_TILE = 32;             // side of a tile in pixels (even: an NV12 tile is whole 2 x 2 blocks)
constexpr int OV_W_ONE = 65280;         // 256 * 255: the weight that stores the colour exactly

struct OvEntry {
    unsigned char* p0;                  // BGR: the frame; NV12: the luma plane
    unsigned char* p1;                  // NV12: the chroma plane
    int pitch0, pitch1, h0, w0;
};
struct OvTable { OvEntry f[LP_FRAMES_PER_LAUNCH]; };

struct OvRect { int i0, i1, j0, j1; };  // rows [i0, i1), columns [j0, j1), clamped to the frame; all zeros: nothing to draw
static_assert(sizeof(OvRect) == 16, "one 16-byte load per record in the cull");

__device__ __forceinline__ int clamp_count(int n, int max_det) { return n < 0 ? 0 : (n > max_det ? max_det : n); }

// clamp(v, 0, n) in double (a NaN goes to 0), then converted: redact.scan_rect's clamp
__device__ __forceinline__ int clamp_to(double v, int n) {
    v = v >= 0.0 ? v : 0.0;
    v = v < (double)n ? v : (double)n;
    return (int)v;
}

// clamp(v, -2^20, 2^20) in double, then converted
__device__ __forceinline__ int bound20(double v) {
    v = v >= -1048576.0 ? v : -1048576.0;
    v = v < 1048576.0 ? v : 1048576.0;
    return (int)v;
}

__device__ __forceinline__ unsigned pack3(const unsigned char c[3]) { return (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16); }

// (fg * w + dst * (65280 - w) + 32640) / 65280: at most 255 * 65280 + 32640 < 2^25
__device__ __forceinline__ int blend(int dst, int fg, int w) {
    return (int)((unsigned)(fg * w + dst * (OV_W_ONE - w) + OV_W_ONE / 2) / (unsigned)OV_W_ONE);
}

// The 2 x 2 block of one thread: BGR 12 bytes (pixel k = 2 di + dj, channel c at 3 k + c); NV12 y[0..3] then u, v at 4, 5.
template <bool NV12>
struct Block {
    int v[NV12 ? 6 : 12];
    bool dirty;

    __device__ __forceinline__ void load(const OvEntry& f, int i, int j, const bool ok[4]) {
        if (NV12) {
            if (!ok[0]) return;                                          // even sizes: a block is whole or outside
            const unsigned char* q = f.p0 + (long long)i * f.pitch0 + j;
            v[0] = q[0]; v[1] = q[1]; v[2] = q[f.pitch0]; v[3] = q[f.pitch0 + 1];
            const unsigned uv = *reinterpret_cast<const unsigned short*>(f.p1 + (long long)(i >> 1) * f.pitch1 + (j >> 1) * 2);
            v[4] = (int)(uv & 255u); v[5] = (int)(uv >> 8);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!ok[k]) continue;
                const unsigned char* q = f.p0 + (long long)(i + (k >> 1)) * f.pitch0 + (long long)(j + (k & 1)) * 3;
                v[3 * k] = q[0]; v[3 * k + 1] = q[1]; v[3 * k + 2] = q[2];
            }
        }
    }

    // one layer: the weights of the four pixels (0 for a pixel outside the frame) and the colour
    __device__ __forceinline__ void apply(const int w[4], unsigned col) {
        const int c0 = (int)(col & 255u), c1 = (int)((col >> 8) & 255u), c2 = (int)((col >> 16) & 255u);
        if ((w[0] | w[1] | w[2] | w[3]) == 0) return;
        dirty = true;
        if (NV12) {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = blend(v[k], c0, w[k]);
            const int wb = (w[0] + w[1] + w[2] + w[3] + 2) >> 2;       // the chroma sample: once per layer
            v[4] = blend(v[4], c1, wb);
            v[5] = blend(v[5], c2, wb);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[3 * k] = blend(v[3 * k], c0, w[k]);
                v[3 * k + 1] = blend(v[3 * k + 1], c1, w[k]);
                v[3 * k + 2] = blend(v[3 * k + 2], c2, w[k]);
            }
        }
    }

    __device__ __forceinline__ void store(const OvEntry& f, int i, int j, const bool ok[4]) const {
        if (NV12) {
            if (!ok[0]) return;
            unsigned char* q = f.p0 + (long long)i * f.pitch0 + j;
            q[0] = (unsigned char)v[0]; q[1] = (unsigned char)v[1];
            q[f.pitch0] = (unsigned char)v[2]; q[f.pitch0 + 1] = (unsigned char)v[3];
            *reinterpret_cast<unsigned short*>(f.p1 + (long long)(i >> 1) * f.pitch1 + (j >> 1) * 2) = (unsigned short)(v[4] | (v[5] << 8));
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!ok[k]) continue;
                unsigned char* q = f.p0 + (long long)(i + (k >> 1)) * f.pitch0 + (long long)(j + (k & 1)) * 3;
                q[0] = (unsigned char)v[3 * k]; q[1] = (unsigned char)v[3 * k + 1]; q[2] = (unsigned char)v[3 * k + 2];
            }
        }
    }
};

// Is the centre (px, py) within sqrt(hw2) of the segment a -> b?  fp64 op by op, no division, the order of
// yolov6/utils/overlay.py::segment_mask:
//   ex = bx - ax, ey = by - ay, L = ex * ex + ey * ey, dx = px - ax, dy = py - ay, d = dx * ex + dy * ey
//   d <= 0: dx * dx + dy * dy <= hw2;  d >= L: fx = px - bx, fy = py - by, fx * fx + fy * fy <= hw2;
//   else cr = dx * ey - dy * ex, cr * cr <= hw2 * L
__device__ __forceinline__ bool on_segment(double ax, double ay, double bx, double by, double hw2, double px, double py) {
    const double ex = bx - ax, ey = by - ay;
    const double L = ex * ex + ey * ey;
    const double dx = px - ax, dy = py - ay;
    const double d = dx * ex + dy * ey;
    const double fx = px - bx, fy = py - by;
    const double cr = dx * ey - dy * ex;
    return d <= 0.0 ? (dx * dx + dy * dy <= hw2) : (d >= L ? (fx * fx + fy * fy <= hw2) : (cr * cr <= hw2 * L));
}

__device__ __forceinline__ bool touches(const int rc[4], int i, int j) { return i + 2 > rc[0] && i < rc[1] && j + 2 > rc[2] && j < rc[3]; }
__device__ __forceinline__ bool inside(const int rc[4], int i, int j) { return i >= rc[0] && i < rc[1] && j >= rc[2] && j < rc[3]; }

// The two layers of a label onto the block at (i, j): the plate over its clipped rectangle lrect at weight w_plate, then the glyph
// cells -- rows [ly + pad, + gh), columns [lx + pad, + n * gw), clipped -- at a_text times the atlas coverage.  A rectangle lies
// inside the frame, so a pixel inside one is a pixel of the frame.
template <bool NV12>
__device__ __forceinline__ void draw_label(Block<NV12>& blk, const int* lrect, int ly, int lx, int pad, int ng,
                                           const unsigned short* __restrict__ glyph, int w_plate, unsigned col_plate, int a_text,
                                           unsigned col_text, const unsigned char* __restrict__ atlas, int gh, int gw, int h0, int w0, int i,
                                           int j) {
    const int lr[4] = {lrect[0], lrect[1], lrect[2], lrect[3]};
    if (!touches(lr, i, j)) return;
    int w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = inside(lr, i + (k >> 1), j + (k & 1)) ? w_plate : 0;
    blk.apply(w, col_plate);
    const int ty = ly + pad, tx = lx + pad;
    const int tr[4] = {max(ty, 0), min(ty + gh, h0), tx, min(tx + ng * gw, w0)};
    if (tr[0] >= tr[1] || tr[2] >= tr[3] || !touches(tr, i, j)) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int pi = i + (k >> 1), pj = j + (k & 1);
        w[k] = 0;
        if (inside(tr, pi, pj)) {
            const int gi = pi - ty, gj = pj - tx, cell = gj / gw;
            const int g = glyph[cell];
            w[k] = a_text * (int)atlas[((long long)g * gh + gi) * gw + (gj - cell * gw)];
        }
    }
    blk.apply(w, col_text);
}
