"""Annotation overlay on the CPU: the numpy restatement of ``lp_overlay_draw_batch`` (csrc/lp_overlay.hip).

Every detection row of a frame is drawn onto the frame: the outline of its box, the outline of its corner quad, and a label (a
filled plate with the track id and the eight heads' characters as glyphs of a caller-supplied atlas).  Rows are painted in row
order, a later row over an earlier one; a row paints up to four layers in the order box outline, quad outline, label plate,
label glyphs.  Every layer is a blend that ends in a byte, so one call with n rows equals n calls with one row each.

Which shape.  ``plate_crop.plate_quad(row)`` decides, unchanged: status 1 (corners) draws the box outline in the box colour --
only if ``draw_box`` and the box (columns 0..3) is finite with sides >= 1 px -- and then the quad outline in the quad colour;
status 2 (box) draws the box outline alone, in the box colour, whatever ``draw_box`` says (it is the row's only shape); status 3
draws nothing, no label either.  The label hangs on plate_quad's quad (the box for status 2).

Outline of thickness t (0..16, 0: none) of the closed polygon p0 -> p3 -> p2 -> p1 -> p0: pixel (i, j) belongs iff the squared
distance from its centre P = (j + 0.5, i + 0.5) to any of the four segments is <= (t / 2)^2 (round joins; a zero-length segment
is a point).  fp64 on the row's fp32 values, op by op (no fused multiply-add), WITHOUT a division, per segment a -> b:
    ex = bx - ax; ey = by - ay; L = ex * ex + ey * ey
    dx = px - ax; dy = py - ay; d = dx * ex + dy * ey
    d <= 0:  dx * dx + dy * dy <= hw2                                  (nearest point: a; L = 0 lands here)
    d >= L:  fx = px - bx; fy = py - by; fx * fx + fy * fy <= hw2      (nearest point: b)
    else:    cr = dx * ey - dy * ex; cr * cr <= hw2 * L                (the foot of the perpendicular)
with hw = 0.5 * t and hw2 = hw * hw.  On corners that are multiples of 0.5 every operation is exact.  The scan rectangle is the
shape's bounds grown by hw and clamped as ``redact.scan_rect`` clamps: rows [clamp(floor(min y - hw), 0, h),
clamp(ceil(max y + hw), 0, h)), columns likewise; it only bounds the scan, no pixel outside it passes the test.

Label.  Glyphs: with ``tid`` given, ``tid[b][r] >= 0`` and ``show_id``: '#', the decimal digits of the id, a space; then for the
eight heads p: v = row[20 + p], id = int(v) when v is finite and 0 <= v < 64, glyph ``glyph_of[p][id]``; the '?' glyph for any
other v and for a ``glyph_of`` entry >= G (0xFFFF is the conventional "no glyph").  At most 20 glyphs.  ``atlas`` uint8
[G, gh, gw] is coverage, with the fixed indices 0..9 digits, 10 '#', 11 space, 12 '?'.  The label is W = n * gw + 2 * pad wide
and H = gh + 2 * pad high.  With the integer bounds of plate_quad's quad, bx0 = floor(min x), by0 = floor(min y), by1 =
ceil(max y), each clamped to +-2^20 in double and then converted, and q = (t + 1) // 2: ly = by0 - q - H, and when that is < 0,
ly = by1 + q (below the plate); lx = max(min(bx0, w - W), 0).  The rectangle [ly, ly + H) x [lx, lx + W) is clipped to the
frame.  Plate layer: every pixel of the rectangle, coverage 255.  Glyph layer: coverage atlas[g_k][i - ly - pad][j - lx - pad -
k * gw] for the pixels of cell k.

Blend of opacity a (0..256) and coverage c (0..255; 255 for outlines and the plate): w = a * c <= 65280 and
    out = (fg * w + dst * (65280 - w) + 32640) // 65280
per channel in int32: w = 0 leaves the byte, w = 65280 stores fg exactly, and dst = fg stays fg at any w.

NV12: Y is blended per pixel; a chroma sample is blended once per layer with wbar = (w00 + w01 + w10 + w11 + 2) >> 2 over its
four luma pixels, U and V separately.  Colours reach the blend in the frame's own bytes: ``redact.fill_bytes(colour, matrix)``
turns (B, G, R) into (Y, U, V); the matrix plays no other part.

Styles: up to 8 ``Style`` entries; ``style`` int32 [B, max_det] selects one per row (none: style 0; below 0 the row is skipped
and its status is 0; an index past the last style takes the last).  ``palette`` uint8 [P, 3], P <= 64: a row with a
``tid >= 0`` takes palette[tid % P] as its quad and plate colours.

No other byte changes: pixels of no layer, rows at or past the count, frames with count <= 0.
"""
import math
from collections import namedtuple

import numpy as np

from yolov6.utils.nv12 import Nv12Frame, is_nv12_list
from yolov6.utils.plate_crop import ST_EMPTY, plate_quad
from yolov6.utils.redact import EDGE_ORDER, _clamp_to, fill_bytes

MAX_STYLES = 8
MAX_GLYPHS = 20                # '#' + 10 digits + ' ' + 8 heads
MAX_THICKNESS = 16
MAX_PAD = 16
MAX_PALETTE = 64
MAX_ATLAS, MAX_CELL = 1024, 64
HEADS, CLASSES = 8, 64
GLYPH_HASH, GLYPH_SPACE, GLYPH_UNKNOWN = 10, 11, 12
NO_GLYPH = 0xFFFF
W_ONE = 65280                  # 256 * 255: the weight that stores the colour exactly
BOUND = float(1 << 20)

#: colours are (B, G, R); t: outline thickness; a_*: opacity 0..256 of the outlines, the label plate, the glyphs; pad: label padding
Style = namedtuple('Style', 'box quad plate text t a_line a_plate a_text pad')
Style.__new__.__defaults__ = ((0, 200, 0), (0, 220, 255), (32, 32, 32), (255, 255, 255), 2, 256, 160, 256, 2)


def check_style(s):
    """``s`` as a ``Style`` of ints, or a ValueError."""
    s = Style(*s)
    cols = tuple(tuple(int(v) for v in c) for c in s[:4])
    if any(len(c) != 3 or not all(0 <= v <= 255 for v in c) for c in cols):
        raise ValueError('style colours must be three bytes (B, G, R) each')
    t, al, ap, at, pad = (int(v) for v in s[4:])
    if not 0 <= t <= MAX_THICKNESS:
        raise ValueError('thickness %d: need 0..%d' % (t, MAX_THICKNESS))
    if not all(0 <= a <= 256 for a in (al, ap, at)):
        raise ValueError('opacities must be in 0..256')
    if not 0 <= pad <= MAX_PAD:
        raise ValueError('pad %d: need 0..%d' % (pad, MAX_PAD))
    return Style(*cols, t, al, ap, at, pad)


def check_styles(styles):
    """A list of 1..8 checked ``Style``s (None: the default style)."""
    styles = [Style()] if styles is None else [check_style(s) for s in styles]
    if not 1 <= len(styles) <= MAX_STYLES:
        raise ValueError('need 1..%d styles, got %d' % (MAX_STYLES, len(styles)))
    return styles


def check_palette(palette):
    """``palette`` as uint8 [P, 3], 1 <= P <= 64 (None stays None)."""
    if palette is None:
        return None
    palette = np.asarray(palette)
    if palette.ndim != 2 or palette.shape[1] != 3 or not 1 <= palette.shape[0] <= MAX_PALETTE or palette.min() < 0 or palette.max() > 255:
        raise ValueError('palette must be [1..%d, 3] bytes (B, G, R)' % MAX_PALETTE)
    return palette.astype(np.uint8)


def check_font(atlas, glyph_of):
    """(atlas uint8 [G, gh, gw], glyph_of uint16 [8, 64]) checked: 13 <= G <= 1024, 1 <= gh, gw <= 64."""
    atlas, glyph_of = np.asarray(atlas), np.asarray(glyph_of)
    if atlas.dtype != np.uint8 or atlas.ndim != 3 or not (GLYPH_UNKNOWN < atlas.shape[0] <= MAX_ATLAS and 1 <= atlas.shape[1] <= MAX_CELL
                                                          and 1 <= atlas.shape[2] <= MAX_CELL):
        raise ValueError('atlas must be uint8 [13..%d, 1..%d, 1..%d]' % (MAX_ATLAS, MAX_CELL, MAX_CELL))
    if glyph_of.shape != (HEADS, CLASSES) or glyph_of.min() < 0 or glyph_of.max() > NO_GLYPH:
        raise ValueError('glyph_of must be [%d, %d] with entries in 0..0xFFFF' % (HEADS, CLASSES))
    return np.ascontiguousarray(atlas), np.ascontiguousarray(glyph_of.astype(np.uint16))


def blend(dst, fg, w):
    """The blend on arrays: ``dst`` bytes, ``fg`` a byte, ``w`` int weights 0..65280 -> uint8."""
    d = np.asarray(dst).astype(np.int32)
    w = np.asarray(w, np.int32)
    return ((int(fg) * w + d * (W_ONE - w) + W_ONE // 2) // W_ONE).astype(np.uint8)


def chroma_weight(w):
    """int32 [h/2, w/2]: (w00 + w01 + w10 + w11 + 2) >> 2 over the 2 x 2 blocks of the luma weights ``w`` [h, w] (even sizes)."""
    w = np.asarray(w, np.int32)
    return (w[0::2, 0::2] + w[0::2, 1::2] + w[1::2, 0::2] + w[1::2, 1::2] + 2) >> 2


def segment_mask(ax, ay, bx, by, px, py, hw2):
    """bool [len(py), len(px)]: the centres (px[None, :], py[:, None]) within sqrt(hw2) of the segment a -> b, in the module's order."""
    px, py = px[None, :], py[:, None]
    ex, ey = bx - ax, by - ay
    L = ex * ex + ey * ey
    dx, dy = px - ax, py - ay
    d = dx * ex + dy * ey
    fx, fy = px - bx, py - by
    cr = dx * ey - dy * ex
    return np.where(d <= 0.0, dx * dx + dy * dy <= hw2, np.where(d >= L, fx * fx + fy * fy <= hw2, cr * cr <= hw2 * L))


def outline_rect(x, y, t, h, w):
    """(i0, i1, j0, j1): the scan rectangle of the outline of thickness ``t`` of the polygon (x, y) in an h x w frame."""
    hw = 0.5 * t
    return (_clamp_to(math.floor(min(y) - hw), h), _clamp_to(math.ceil(max(y) + hw), h),
            _clamp_to(math.floor(min(x) - hw), w), _clamp_to(math.ceil(max(x) + hw), w))


def outline_mask(x, y, t, h, w):
    """(i0, i1, j0, j1, mask bool [i1 - i0, j1 - j0]): the pixels of the outline inside its scan rectangle."""
    i0, i1, j0, j1 = outline_rect(x, y, t, h, w)
    if t <= 0 or i0 >= i1 or j0 >= j1:
        return i0, i0, j0, j0, np.zeros((0, 0), bool)
    hw = 0.5 * t
    hw2 = hw * hw
    py = np.arange(i0, i1, dtype=np.float64) + 0.5
    px = np.arange(j0, j1, dtype=np.float64) + 0.5
    m = np.zeros((i1 - i0, j1 - j0), bool)
    for k in range(4):
        a, b = EDGE_ORDER[k], EDGE_ORDER[(k + 1) % 4]
        m |= segment_mask(x[a], y[a], x[b], y[b], px, py, hw2)
    return i0, i1, j0, j1, m


def box_of(row):
    """The box of a row as a quad (xs, ys) when it is finite with sides >= 1 px, else None (the box rule of ``plate_quad``)."""
    x1, y1, x2, y2 = (float(np.float32(v)) for v in row[:4])
    if all(math.isfinite(v) for v in (x1, y1, x2, y2)) and x2 - x1 >= 1.0 and y2 - y1 >= 1.0:
        return [x1, x2, x2, x1], [y1, y1, y2, y2]
    return None


def label_glyphs(row, tid, glyph_of, n_atlas, show_id=True):
    """The glyph indices of a row's label: the id part (``tid`` an int or None), then the eight heads."""
    g = []
    if tid is not None and int(tid) >= 0 and show_id:
        g = [GLYPH_HASH] + [int(c) for c in str(int(tid))] + [GLYPH_SPACE]
    for p in range(HEADS):
        v = float(np.float32(row[20 + p]))
        k = GLYPH_UNKNOWN
        if math.isfinite(v) and 0.0 <= v < float(CLASSES):
            k = int(glyph_of[p][int(v)])
            if k >= n_atlas:
                k = GLYPH_UNKNOWN
        g.append(k)
    return g


def _bound(v):
    v = v if v >= -BOUND else -BOUND
    v = v if v < BOUND else BOUND
    return int(v)


def label_origin(x, y, t, n, gh, gw, pad, w):
    """(ly, lx, H, W) of the label of n glyphs on the quad (x, y) in a frame w wide."""
    W, H = n * gw + 2 * pad, gh + 2 * pad
    bx0, by0, by1 = _bound(math.floor(min(x))), _bound(math.floor(min(y))), _bound(math.ceil(max(y)))
    q = (t + 1) // 2
    ly = by0 - q - H
    if ly < 0:
        ly = by1 + q
    return ly, max(min(bx0, w - W), 0), H, W


class _Canvas:
    """The planes of one frame under the layers: ``apply`` blends one layer's weights into them."""

    def __init__(self, frame):
        self.nv12 = isinstance(frame, Nv12Frame)
        if self.nv12:
            self.out = Nv12Frame.from_packed(frame.packed(), frame.h, frame.w, frame.matrix)
            self.h, self.w, self.matrix = frame.h, frame.w, frame.matrix
        else:
            frame = np.asarray(frame)
            if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3 or frame.shape[0] < 1 or frame.shape[1] < 1:
                raise ValueError('frame must be a uint8 [h, w, 3] array, got %s %s' % (frame.dtype, frame.shape))
            self.out = frame.copy()
            self.h, self.w, self.matrix = frame.shape[0], frame.shape[1], None

    def colour(self, bgr):
        return fill_bytes(bgr, self.matrix)

    def apply(self, i0, i1, j0, j1, wt, col):
        """Blend ``col`` (the frame's own bytes) with the weights ``wt`` int32 [i1 - i0, j1 - j0] into the rectangle."""
        if i0 >= i1 or j0 >= j1:
            return
        if not self.nv12:
            for c in range(3):
                self.out[i0:i1, j0:j1, c] = blend(self.out[i0:i1, j0:j1, c], col[c], wt)
            return
        o = self.out
        o.y[i0:i1, j0:j1] = blend(o.y[i0:i1, j0:j1], col[0], wt)
        e0, e1, f0, f1 = i0 & ~1, (i1 + 1) & ~1, j0 & ~1, (j1 + 1) & ~1          # the rectangle grown to whole 2 x 2 blocks
        full = np.zeros((e1 - e0, f1 - f0), np.int32)
        full[i0 - e0:i1 - e0, j0 - f0:j1 - f0] = wt
        wb = chroma_weight(full)
        uv = o.uv[e0 // 2:e1 // 2, f0 // 2:f1 // 2]
        uv[..., 0] = blend(uv[..., 0], col[1], wb)
        uv[..., 1] = blend(uv[..., 1], col[2], wb)


def draw_row(cv, row, atlas, glyph_of, st, tid=None, palette=None, show_id=True, label=True, draw_box=True):
    """Paint one detection row onto the canvas ``cv`` with the checked style ``st``; returns the row's status (1, 2 or 3)."""
    status, x, y = plate_quad(row)
    if status == ST_EMPTY:
        return status
    quad_col, plate_col = st.quad, st.plate
    if palette is not None and tid is not None and int(tid) >= 0:
        quad_col = plate_col = tuple(int(v) for v in palette[int(tid) % len(palette)])
    box = box_of(row)
    if box is not None and (status == 2 or draw_box):
        i0, i1, j0, j1, m = outline_mask(box[0], box[1], st.t, cv.h, cv.w)
        cv.apply(i0, i1, j0, j1, m.astype(np.int32) * (st.a_line * 255), cv.colour(st.box))
    if status == 1:
        i0, i1, j0, j1, m = outline_mask(x, y, st.t, cv.h, cv.w)
        cv.apply(i0, i1, j0, j1, m.astype(np.int32) * (st.a_line * 255), cv.colour(quad_col))
    if not label:
        return status
    G, gh, gw = atlas.shape
    g = label_glyphs(row, tid, glyph_of, G, show_id)
    ly, lx, H, W = label_origin(x, y, st.t, len(g), gh, gw, st.pad, cv.w)
    i0, i1, j0, j1 = max(ly, 0), min(ly + H, cv.h), lx, min(lx + W, cv.w)
    if i0 >= i1 or j0 >= j1:
        return status
    cv.apply(i0, i1, j0, j1, np.full((i1 - i0, j1 - j0), st.a_plate * 255, np.int32), cv.colour(plate_col))
    ti0, ti1 = max(ly + st.pad, 0), min(ly + st.pad + gh, cv.h)
    tj0, tj1 = lx + st.pad, min(lx + st.pad + len(g) * gw, cv.w)
    if ti0 < ti1 and tj0 < tj1:
        gi = np.arange(ti0, ti1) - (ly + st.pad)
        gj = np.arange(tj0, tj1) - (lx + st.pad)
        k = gj // gw
        cov = atlas[np.asarray(g)[k][None, :], gi[:, None], (gj - k * gw)[None, :]].astype(np.int32)
        cv.apply(ti0, ti1, tj0, tj1, cov * st.a_text, cv.colour(st.text))
    return status


def draw_plates_np(frames, det, count, atlas, glyph_of, tid=None, style=None, styles=None, palette=None, show_id=True, label=True,
                   draw_box=True):
    """The specification of ``lp_overlay_draw_batch``: ``frames`` a list of B uint8 [h, w, 3] BGR arrays or of B ``Nv12Frame`` with
    host planes (one kind), ``det`` [>= B, max_det, 28] and ``count`` [>= B] as the padded detectors or ``PlateTracker.update``
    (det_out) return them, ``tid`` int32 [>= B, max_det] or None, ``style`` int32 [>= B, max_det] or None, ``styles`` a list of up
    to 8 ``Style`` (None: the default), ``palette`` uint8 [P, 3] (B, G, R) or None.  Returns (frames_out, status): new frames
    of the same kind (the inputs are not written) and int32 [B, max_det] with 1 = corners, 2 = box, 3 = neither (nothing
    drawn), 0 = no such row or a row whose style is < 0."""
    frames = list(frames)
    is_nv12_list(frames)
    atlas, glyph_of = check_font(atlas, glyph_of)
    styles, palette = check_styles(styles), check_palette(palette)
    det = np.asarray(det, np.float32)
    count = np.asarray(count).reshape(-1)
    if det.ndim != 3 or det.shape[2] < 28 or det.shape[0] < len(frames) or count.shape[0] < len(frames) or det.shape[1] < 1:
        raise ValueError('det must be [>= %d, max_det >= 1, 28] with a count per frame, got %s and %s' % (len(frames), det.shape, count.shape))
    max_det = det.shape[1]
    for name, a in (('tid', tid), ('style', style)):
        if a is not None and (np.asarray(a).ndim != 2 or np.asarray(a).shape[0] < len(frames) or np.asarray(a).shape[1] != max_det):
            raise ValueError('%s must be [>= %d, %d]' % (name, len(frames), max_det))
    status = np.zeros((len(frames), max_det), np.int32)
    out = []
    for b, f in enumerate(frames):
        cv = _Canvas(f)
        for r in range(max(0, min(int(count[b]), max_det))):
            s = 0 if style is None else int(style[b][r])
            if s < 0:
                continue
            status[b, r] = draw_row(cv, det[b, r], atlas, glyph_of, styles[min(s, len(styles) - 1)],
                                    None if tid is None else int(tid[b][r]), palette, show_id, label, draw_box)
        out.append(cv.out)
    return out, status


def build_atlas(pro_names, alp_names, ads_names, size=24, font=None):
    """(atlas uint8 [G, gh, gw], glyph_of uint16 [8, 64]) rendered on the host with PIL: the thirteen fixed glyphs (digits, '#',
    space, '?'), then one glyph per distinct name of the three class lists, each centred in a cell of gh = ``size`` + 4 rows and the
    widest name's columns.  Head 0 reads ``pro_names``, head 1 ``alp_names``, heads 2..7 ``ads_names`` (at most 64 each).
    ``font``: the path of a TrueType file, else PIL's default font at ``size`` (which needs no file but draws ASCII only: a
    name with a non-ASCII character then gets 0xFFFF and shows '?' -- pass a CJK font for the provinces)."""
    from PIL import Image, ImageDraw, ImageFont
    size = int(size)
    if not 4 <= size <= MAX_CELL - 4:
        raise ValueError('size %d: need 4..%d' % (size, MAX_CELL - 4))
    fnt = ImageFont.truetype(font, size) if font else ImageFont.load_default(size)
    lists = [list(pro_names), list(alp_names)] + [list(ads_names)] * 6
    if any(len(n) > CLASSES for n in lists):
        raise ValueError('at most %d names per head' % CLASSES)
    fixed = [str(d) for d in range(10)] + ['#', ' ', '?']
    names, index = list(fixed), {n: k for k, n in enumerate(fixed)}
    glyph_of = np.full((HEADS, CLASSES), NO_GLYPH, np.uint16)
    for p, lst in enumerate(lists):
        for c, n in enumerate(lst):
            n = str(n)
            if not n or (font is None and not n.isascii()):
                continue
            if n not in index:
                if len(names) >= MAX_ATLAS:
                    raise ValueError('more than %d distinct glyphs' % MAX_ATLAS)
                index[n] = len(names)
                names.append(n)
            glyph_of[p, c] = index[n]
    boxes = [fnt.getbbox(n) for n in names]
    gh = size + 4
    gw = min(MAX_CELL, max(2, max(int(math.ceil(fnt.getlength(n))) for n in names) + 2))
    asc, desc = fnt.getmetrics()
    atlas = np.zeros((len(names), gh, gw), np.uint8)
    for k, (n, bb) in enumerate(zip(names, boxes)):
        img = Image.new('L', (gw, gh), 0)
        x = (gw - (bb[2] - bb[0])) // 2 - bb[0]
        y = (gh - (asc + desc)) // 2
        ImageDraw.Draw(img).text((x, y), n, fill=255, font=fnt)
        atlas[k] = np.asarray(img)
    return atlas, glyph_of
