"""Scene overlay on the CPU: the numpy restatement of ``lp_overlay_scene_batch`` (csrc/lp_overlay_scene.hip).

The lines and zones of ``yolov6.utils.zones``, their running totals, occupancies and dwell alerts, and the speed of
``yolov6.utils.speed`` are drawn onto the frames: what the tracker knows about the scene, in the picture an operator looks at.
The picture agrees with the rule exactly: a pixel shown inside a zone is a point ``lp_zone_update`` calls inside, and the marker
of a line sits on the side that ``zones.crossing_dir`` counts as +1.  The blend, the NV12 chroma weight, the segment test and the
canvas are those of ``yolov6.utils.overlay``; the crossing number is ``zones._toggles``.

Inputs of one call, frames of one kind: ``stream_of`` [B] names the stream of frame b (None: frame b is stream b; an entry outside
[0, S) skips the frame: no byte of it changes and its status is 0); ``packed`` int32 [S, 368] is the ``ZoneMapNp`` layout
(``zones.check_packed`` refuses anything else, so no vertex is ever non-finite); three optional groups: ``totals`` [S, 2, 16] +
``occ`` [S, 8] (absent: no labels, no zone is busy), ``zone_ev`` [S, max_events, 12] + ``zone_count`` [S] (absent: no alert
colour), ``speed_i`` [S, T, 8] + ``det`` [B, max_det, 28] + ``count`` [B] + ``tid`` [B, max_det] (absent: no tags).

Layers of one frame of stream s, in this fixed order; every layer is one ``overlay.blend`` that ends in a byte, so one call equals
the layers applied one at a time:
  1. Zone fills, z ascending.  Pixel (i, j) belongs iff the crossing number of ``zones._toggles`` over the zone's edges (Vk, Vk+1 mod n)
     at P = (j + 0.5, i + 0.5) is odd: fp64 on the fp32 vertices, op by op, no fused multiply-add, no division -- the expression of
     ``zones.inside_zone``.  Scan rectangle: ``overlay.outline_rect`` of the vertices at thickness 0.  Weight: a * 255 with a =
     ``a_fill``, or ``a_fill_busy`` when occ[s][z] > 0.  Colour: ``zone``, or ``alert`` when one of the first
     min(max(zone_count[s], 0), max_events) event lines of the stream has kind 4 (dwell) and index z.
  2. Zone outlines, z ascending: the closed polygon V0 -> V1 -> ... -> Vn-1 -> V0 by ``overlay.segment_mask`` at thickness ``t``
     (0: none), hw2 = (t / 2)^2, scan rectangle ``outline_rect`` at ``t``; weight ``a_line`` * 255; the colour of the fill.
  3. Lines, l ascending: first the segment A -> B like an outline edge, in the ``line`` colour; then, as its own layer, the
     direction marker in the ``mark`` colour at weight ``a_line`` * 255.  With M = ((ax + bx) * 0.5, (ay + by) * 0.5), e = B - A,
     L = ex * ex + ey * ey, dx = px - Mx, dy = py - My:
         s = ex * dy - ey * dx        (``zones.cross(A, B, P)`` taken about M: s > 0 is the side ``crossing_dir`` counts as +1)
         u = dx * ex + dy * ey
         q = |u| + s
     the pixel belongs iff L > 0, s >= 0 and q * q <= (m * m) * L: a right isosceles triangle of height m = ``marker`` pixels
     (0..64, 0: none), base on the line, apex on the +1 side.  fp64, each operation rounded on its own, no division, no square
     root.  Scan rectangle: rows [clamp(floor(My - m), 0, h), clamp(ceil(My + m), 0, h)), columns likewise about Mx.
  4. Zone labels z ascending, then line labels l ascending: a filled plate (``plate``, ``a_plate``) and a glyph layer (``text``,
     ``a_text``), blended as the plate label of ``overlay.py``.  Zone glyphs: the name, ' ', the decimal digits of occ[s][z].  Line
     glyphs: the name, ' ', '+', the digits of totals[s][0][l], ' ', '-', the digits of totals[s][1][l].  A value v < 0 prints as
     v + 2^32: the totals wrap.  A name is names[s][k] (k = l for lines, 16 + z for zones) up to its first 0xFFFF, at most 12
     glyphs; an index >= G shows '?'.  At most ``MAX_SCENE_GLYPHS`` = 36 = 12 + 2 + 10 + 2 + 10.  Placement, pure integer after
     the floor: the anchor point (x, y) is vertex 0 of a zone, B of a line; ax = floor(x), ay0 = floor(y), ay1 = ceil(y), each
     clamped to +-2^20 in double and then converted; W = n * gw + 2 * pad, H = gh + 2 * pad, q = (t + 1) // 2; ly = ay0 - q - H,
     and ly = ay1 + q when that is < 0; lx = max(min(ax, w - W), 0) -- ``overlay.label_origin`` of the one-point polygon.  The
     rectangle [ly, ly + H) x [lx, lx + W) is clipped to the frame.
  5. Speed tags, rows in row order.  Row r < clamp(count[b], 0, max_det) with tid[b][r] >= 0 whose ``plate_quad`` status is not 3
     gets a tag iff speed_i[s] has a slot with id == tid and speed >= 0; the lowest such slot wins.  kmh = (speed * 36 + 5000) //
     10000 in int64 (mm/s to km/h, half up).  The tag is a label of the digits of kmh on a plate in the ``tag`` colour: W and H
     as above, bx1 = ceil(max x), by0 = floor(min y) of the row's quad (clamped to +-2^20), ly = by0, lx = max(min(bx1 + q,
     w - W), 0), clipped to the frame.  status[b][r] = 1 for a row that gets a tag (whatever the clipping leaves of it), else 0.

NV12: Y is blended per pixel; a chroma sample once per layer with ``overlay.chroma_weight``.  Colours go through
``redact.fill_bytes``.  No other byte changes: pitch padding, pixels of no layer, frames whose stream has no lines, no zones and
no tags.

Scene font: ``build_scene_atlas`` -- the thirteen fixed glyphs of ``overlay.py`` (digits, '#', ' ', '?'), then '+', '-', '.', ':'
at 13..16, then the remaining printable ASCII; ``SceneAtlas.glyphs_of_text`` maps a string.  With any ``glyph_of`` table the atlas
also serves ``draw_plates``.

What it does not do: one style per call; labels do not avoid each other or the plate labels; no anti-aliasing; names are limited
to 12 glyphs of the atlas; zone and line geometry is in pixels only, there is no ground-plane grid; the tag shows the estimate at
the end of the call; not with ``--redact-lookback`` (the delayed frames are not the ones the totals belong to).
"""
import math
from collections import namedtuple

import numpy as np

from yolov6.utils import zones
from yolov6.utils.nv12 import is_nv12_list
from yolov6.utils.overlay import (GLYPH_SPACE, GLYPH_UNKNOWN, MAX_ATLAS, MAX_CELL, MAX_PAD, MAX_THICKNESS, NO_GLYPH, _bound, _Canvas,
                                  label_origin, outline_rect, segment_mask)
from yolov6.utils.plate_crop import ST_EMPTY, plate_quad
from yolov6.utils.redact import _clamp_to

MAX_NAME = 12
N_NAMES = zones.MAX_LINES + zones.MAX_ZONES            # lines 0..15, then zones 0..7
MAX_SCENE_GLYPHS = MAX_NAME + 2 + 10 + 2 + 10           # name, ' +', 10 digits, ' -', 10 digits
MAX_MARKER = 64
GLYPH_PLUS, GLYPH_MINUS, GLYPH_DOT, GLYPH_COLON = 13, 14, 15, 16
N_FIXED = 17
FIXED = [str(d) for d in range(10)] + ['#', ' ', '?', '+', '-', '.', ':']

#: colours are (B, G, R): zone fill and outline, the same under a dwell alert, lines, their markers, label plates, glyphs, tag plates;
#: t: outline and line thickness; marker: the marker's height m; a_*: opacity 0..256; pad: label padding
SceneStyle = namedtuple('SceneStyle', 'zone alert line mark plate text tag t marker a_fill a_fill_busy a_line a_plate a_text pad')
SceneStyle.__new__.__defaults__ = ((200, 160, 0), (0, 0, 255), (0, 255, 255), (0, 255, 255), (32, 32, 32), (255, 255, 255), (96, 0, 96),
                                   2, 12, 48, 96, 256, 160, 256, 2)


def check_scene_style(s):
    """``s`` as a ``SceneStyle`` of ints (None: the default), or a ValueError."""
    s = SceneStyle() if s is None else SceneStyle(*s)
    cols = tuple(tuple(int(v) for v in c) for c in s[:7])
    if any(len(c) != 3 or not all(0 <= v <= 255 for v in c) for c in cols):
        raise ValueError('style colours must be three bytes (B, G, R) each')
    t, m, af, ab, al, ap, at, pad = (int(v) for v in s[7:])
    if not 0 <= t <= MAX_THICKNESS:
        raise ValueError('thickness %d: need 0..%d' % (t, MAX_THICKNESS))
    if not 0 <= m <= MAX_MARKER:
        raise ValueError('marker %d: need 0..%d' % (m, MAX_MARKER))
    if not all(0 <= a <= 256 for a in (af, ab, al, ap, at)):
        raise ValueError('opacities must be in 0..256')
    if not 0 <= pad <= MAX_PAD:
        raise ValueError('pad %d: need 0..%d' % (pad, MAX_PAD))
    return SceneStyle(*cols, t, m, af, ab, al, ap, at, pad)


def check_scene_font(atlas):
    """``atlas`` uint8 [G, gh, gw] checked: 17 <= G <= 1024 (the seventeen fixed glyphs), 1 <= gh, gw <= 64."""
    atlas = np.asarray(getattr(atlas, 'atlas', atlas))
    if atlas.dtype != np.uint8 or atlas.ndim != 3 or not (N_FIXED <= atlas.shape[0] <= MAX_ATLAS and 1 <= atlas.shape[1] <= MAX_CELL
                                                          and 1 <= atlas.shape[2] <= MAX_CELL):
        raise ValueError('a scene atlas must be uint8 [%d..%d, 1..%d, 1..%d]' % (N_FIXED, MAX_ATLAS, MAX_CELL, MAX_CELL))
    return np.ascontiguousarray(atlas)


def check_names(names, n_streams):
    """``names`` as uint16 [S, 24, 12] (None: every name empty)."""
    if names is None:
        return np.full((n_streams, N_NAMES, MAX_NAME), NO_GLYPH, np.uint16)
    names = np.asarray(names)
    if names.shape != (n_streams, N_NAMES, MAX_NAME) or names.min() < 0 or names.max() > NO_GLYPH:
        raise ValueError('names must be [%d, %d, %d] with entries in 0..0xFFFF' % (n_streams, N_NAMES, MAX_NAME))
    return np.ascontiguousarray(names.astype(np.uint16))


class SceneAtlas:
    """A scene font: ``atlas`` uint8 [G, gh, gw] and ``chars``, the string whose k-th character glyph k draws."""

    def __init__(self, atlas, chars):
        self.atlas, self.chars = check_scene_font(atlas), str(chars)
        if len(self.chars) != len(self.atlas) or self.chars[:N_FIXED] != ''.join(FIXED):
            raise ValueError('a scene atlas starts with the %d fixed glyphs and has one character per glyph' % N_FIXED)
        self._index = {}
        for k, c in enumerate(self.chars):
            self._index.setdefault(c, k)

    def glyphs_of_text(self, text):
        """The glyph indices of ``text`` (a character the atlas lacks: '?')."""
        return [self._index.get(c, GLYPH_UNKNOWN) for c in str(text)]

    def glyph_of(self):
        """A ``draw_plates`` table uint16 [8, 64] that shows every class as '?': the atlas serves both calls."""
        return np.full((8, 64), NO_GLYPH, np.uint16)


def build_scene_atlas(size=24, font=None, chars=None):
    """A ``SceneAtlas`` rendered on the host with PIL: the seventeen fixed glyphs, then ``chars`` (default: the remaining printable
    ASCII), each centred in a cell of gh = ``size`` + 4 rows and the widest character's columns.  ``font``: the path of a TrueType
    file, else PIL's default font at ``size``."""
    from PIL import Image, ImageDraw, ImageFont
    size = int(size)
    if not 4 <= size <= MAX_CELL - 4:
        raise ValueError('size %d: need 4..%d' % (size, MAX_CELL - 4))
    fnt = ImageFont.truetype(font, size) if font else ImageFont.load_default(size)
    rest = ''.join(chr(c) for c in range(33, 127)) if chars is None else str(chars)
    names = list(FIXED)
    for c in rest:
        if c not in names:
            names.append(c)
    if len(names) > MAX_ATLAS:
        raise ValueError('more than %d distinct glyphs' % MAX_ATLAS)
    gh = size + 4
    gw = min(MAX_CELL, max(2, max(int(math.ceil(fnt.getlength(n))) for n in names) + 2))
    asc, desc = fnt.getmetrics()
    atlas = np.zeros((len(names), gh, gw), np.uint8)
    for k, n in enumerate(names):
        bb = fnt.getbbox(n)
        img = Image.new('L', (gw, gh), 0)
        ImageDraw.Draw(img).text(((gw - (bb[2] - bb[0])) // 2 - bb[0], (gh - (asc + desc)) // 2), n, fill=255, font=fnt)
        atlas[k] = np.asarray(img)
    return SceneAtlas(atlas, ''.join(names))


def names_of(parsed, font, n_streams=None):
    """names uint16 [S, 24, 12] of what ``zones.parse_zones`` returned (lines, zones, line_names, zone_names), in the glyphs of
    ``font`` (a ``SceneAtlas``); a name longer than 12 characters is cut."""
    line_names, zone_names = parsed[2], parsed[3]
    S = len(line_names) if n_streams is None else int(n_streams)
    names = np.full((S, N_NAMES, MAX_NAME), NO_GLYPH, np.uint16)
    for s in range(min(S, len(line_names))):
        for k, n in [(l, n) for l, n in enumerate(line_names[s])] + [(zones.MAX_LINES + z, n) for z, n in enumerate(zone_names[s])]:
            g = font.glyphs_of_text(n)[:MAX_NAME]
            names[s, k, :len(g)] = g
    return names


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------
def decimal_glyphs(v):
    """The digits of an int32 ``v`` as glyph indices; v < 0 prints as v + 2^32."""
    return [int(c) for c in str(int(v) & 0xFFFFFFFF)]


def kmh_of(speed):
    """mm/s to km/h, half up, in int64."""
    return int((np.int64(speed) * np.int64(36) + np.int64(5000)) // np.int64(10000))


def zone_mask(verts, h, w):
    """(i0, i1, j0, j1, mask bool [i1 - i0, j1 - j0]): the pixels of an h x w frame inside the polygon ``verts`` fp32 [n, 2]."""
    v = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 2)
    i0, i1, j0, j1 = outline_rect(list(v[:, 0]), list(v[:, 1]), 0, h, w)
    if i0 >= i1 or j0 >= j1:
        return i0, i0, j0, j0, np.zeros((0, 0), bool)
    nxt = np.roll(v, -1, axis=0)
    py = (np.arange(i0, i1, dtype=np.float64) + 0.5)[None, :, None]
    px = (np.arange(j0, j1, dtype=np.float64) + 0.5)[None, None, :]
    tg = zones._toggles(v[:, 0, None, None], v[:, 1, None, None], nxt[:, 0, None, None], nxt[:, 1, None, None], px, py)
    return i0, i1, j0, j1, (tg.sum(axis=0) & 1).astype(bool)


def polyline_mask(x, y, t, h, w, closed):
    """(i0, i1, j0, j1, mask): the pixels within t / 2 of the polyline (x, y), closed or not."""
    i0, i1, j0, j1 = outline_rect(x, y, t, h, w)
    if t <= 0 or i0 >= i1 or j0 >= j1:
        return i0, i0, j0, j0, np.zeros((0, 0), bool)
    hw = 0.5 * t
    py = np.arange(i0, i1, dtype=np.float64) + 0.5
    px = np.arange(j0, j1, dtype=np.float64) + 0.5
    m = np.zeros((i1 - i0, j1 - j0), bool)
    n = len(x)
    for k in range(n if closed else n - 1):
        m |= segment_mask(x[k], y[k], x[(k + 1) % n], y[(k + 1) % n], px, py, hw * hw)
    return i0, i1, j0, j1, m


def marker_rect(ax, ay, bx, by, m, h, w):
    """(Mx, My, i0, i1, j0, j1): the midpoint in fp64 and the marker's scan rectangle."""
    mx, my = (np.float64(ax) + np.float64(bx)) * 0.5, (np.float64(ay) + np.float64(by)) * 0.5
    return (mx, my, _clamp_to(math.floor(my - m), h), _clamp_to(math.ceil(my + m), h), _clamp_to(math.floor(mx - m), w),
            _clamp_to(math.ceil(mx + m), w))


def marker_mask(ax, ay, bx, by, m, h, w):
    """(i0, i1, j0, j1, mask): the direction marker of the line A -> B (fp32 values) of height ``m``."""
    ax, ay, bx, by = (np.float64(np.float32(v)) for v in (ax, ay, bx, by))
    mx, my, i0, i1, j0, j1 = marker_rect(ax, ay, bx, by, m, h, w)
    if m <= 0 or i0 >= i1 or j0 >= j1:
        return i0, i0, j0, j0, np.zeros((0, 0), bool)
    ex, ey = bx - ax, by - ay
    L = ex * ex + ey * ey
    dy = (np.arange(i0, i1, dtype=np.float64) + 0.5)[:, None] - my
    dx = (np.arange(j0, j1, dtype=np.float64) + 0.5)[None, :] - mx
    s = ex * dy - ey * dx
    u = dx * ex + dy * ey
    q = np.abs(u) + s
    return i0, i1, j0, j1, (L > 0.0) & (s >= 0.0) & (q * q <= (float(m) * float(m)) * L)


def alert_zones(zone_ev, zone_count, s):
    """The set of zones of stream ``s`` with a dwell event among the first min(max(zone_count[s], 0), max_events) event lines."""
    if zone_ev is None:
        return set()
    n = max(0, min(int(zone_count[s]), zone_ev.shape[1]))
    return {int(e[1]) for e in zone_ev[s, :n] if int(e[0]) == zones.KIND_DWELL}


def name_glyphs(name, n_atlas):
    """The glyphs of one names line uint16 [12]: up to the first 0xFFFF; an index past the atlas shows '?'."""
    g = []
    for v in name:
        if int(v) == NO_GLYPH:
            break
        g.append(int(v) if int(v) < n_atlas else GLYPH_UNKNOWN)
    return g


def zone_label_glyphs(name, occ, n_atlas):
    return name_glyphs(name, n_atlas) + [GLYPH_SPACE] + decimal_glyphs(occ)


def line_label_glyphs(name, plus, minus, n_atlas):
    return name_glyphs(name, n_atlas) + [GLYPH_SPACE, GLYPH_PLUS] + decimal_glyphs(plus) + [GLYPH_SPACE, GLYPH_MINUS] + decimal_glyphs(minus)


def tag_origin(x, y, t, n, gh, gw, pad, w):
    """(ly, lx) of the tag of n glyphs to the right of the quad (x, y), at its top, in a frame w wide."""
    W = n * gw + 2 * pad
    bx1, by0 = _bound(math.ceil(max(x))), _bound(math.floor(min(y)))
    return by0, max(min(bx1 + (t + 1) // 2, w - W), 0)


def tag_speed(speed_rows, tid):
    """The speed of the lowest slot of ``speed_rows`` [T, 8] with id == tid and speed >= 0, or None."""
    for row in speed_rows:
        if int(row[0]) == int(tid) and int(row[1]) >= 0:
            return int(row[1])
    return None


def scene_layers(h, w, packed_s, st, atlas, names_s, totals_s=None, occ_s=None, alerts=(), tags=()):
    """The layers of one frame of a stream as a list of (i0, i1, j0, j1, weights int32, colour (B, G, R)) in the order of the rule;
    ``tags``: (x, y, kmh) per tagged row in row order.  Rectangles with no pixel are left out."""
    G, gh, gw = atlas.shape
    p = np.asarray(packed_s, np.int32)
    nl, nz = int(p[0]), int(p[1])
    lines = p[zones.MAP_LINES:zones.MAP_LINES + 4 * nl].view(np.float32).reshape(nl, 4)
    polys = [p[zones.MAP_VERTS + 32 * z:zones.MAP_VERTS + 32 * z + 2 * int(p[zones.MAP_ZHDR + 4 * z])].view(np.float32).reshape(-1, 2)
             for z in range(nz)]
    out = []

    def add(i0, i1, j0, j1, wt, col):
        if i0 < i1 and j0 < j1:
            out.append((i0, i1, j0, j1, wt, col))

    def label(x, y, g, col):
        ly, lx = label_origin([x], [y], st.t, len(g), gh, gw, st.pad, w)[:2]
        label_layers(ly, lx, g, col)

    def label_layers(ly, lx, g, col):
        H, W = gh + 2 * st.pad, len(g) * gw + 2 * st.pad
        i0, i1, j0, j1 = max(ly, 0), min(ly + H, h), lx, min(lx + W, w)
        if i0 >= i1 or j0 >= j1:
            return
        add(i0, i1, j0, j1, np.full((i1 - i0, j1 - j0), st.a_plate * 255, np.int32), col)
        ti0, ti1 = max(ly + st.pad, 0), min(ly + st.pad + gh, h)
        tj0, tj1 = lx + st.pad, min(lx + st.pad + len(g) * gw, w)
        if ti0 < ti1 and tj0 < tj1:
            gi = np.arange(ti0, ti1) - (ly + st.pad)
            gj = np.arange(tj0, tj1) - (lx + st.pad)
            k = gj // gw
            cov = atlas[np.asarray(g)[k][None, :], gi[:, None], (gj - k * gw)[None, :]].astype(np.int32)
            add(ti0, ti1, tj0, tj1, cov * st.a_text, st.text)

    zcol = [st.alert if z in alerts else st.zone for z in range(nz)]
    for z, v in enumerate(polys):                                                                   # 1
        i0, i1, j0, j1, m = zone_mask(v, h, w)
        a = st.a_fill_busy if occ_s is not None and int(occ_s[z]) > 0 else st.a_fill
        add(i0, i1, j0, j1, m.astype(np.int32) * (a * 255), zcol[z])
    for z, v in enumerate(polys):                                                                   # 2
        v = v.astype(np.float64)
        i0, i1, j0, j1, m = polyline_mask(list(v[:, 0]), list(v[:, 1]), st.t, h, w, True)
        add(i0, i1, j0, j1, m.astype(np.int32) * (st.a_line * 255), zcol[z])
    for l in range(nl):                                                                             # 3
        ax, ay, bx, by = (float(v) for v in lines[l])
        i0, i1, j0, j1, m = polyline_mask([ax, bx], [ay, by], st.t, h, w, False)
        add(i0, i1, j0, j1, m.astype(np.int32) * (st.a_line * 255), st.line)
        i0, i1, j0, j1, m = marker_mask(ax, ay, bx, by, st.marker, h, w)
        add(i0, i1, j0, j1, m.astype(np.int32) * (st.a_line * 255), st.mark)
    if totals_s is not None:                                                                        # 4
        for z, v in enumerate(polys):
            label(float(v[0, 0]), float(v[0, 1]), zone_label_glyphs(names_s[zones.MAX_LINES + z], occ_s[z], G), st.plate)
        for l in range(nl):
            label(float(lines[l, 2]), float(lines[l, 3]), line_label_glyphs(names_s[l], totals_s[0][l], totals_s[1][l], G), st.plate)
    for x, y, kmh in tags:                                                                          # 5
        g = decimal_glyphs(kmh)
        ly, lx = tag_origin(x, y, st.t, len(g), gh, gw, st.pad, w)
        label_layers(ly, lx, g, st.tag)
    return out


def draw_scene_np(frames, packed, atlas, names=None, stream_of=None, totals=None, occ=None, zone_ev=None, zone_count=None, speed_i=None,
                  det=None, count=None, tid=None, style=None):
    """The specification of ``lp_overlay_scene_batch``: ``frames`` a list of B uint8 [h, w, 3] BGR arrays or of B ``Nv12Frame`` with
    host planes (one kind); ``packed`` int32 [S, 368] (``ZoneMapNp.packed``); ``atlas`` a ``SceneAtlas`` or its uint8 [G, gh, gw]
    array; the three optional groups of the module docstring.  Returns (frames_out, status): new frames of the same kind (the
    inputs are not written) and int32 [B, max_det] with 1 for a row that got a tag (None without ``det``)."""
    frames = list(frames)
    is_nv12_list(frames)
    atlas = check_scene_font(atlas)
    st = check_scene_style(style)
    packed = np.asarray(packed)
    zones.check_packed(packed)
    S, B = packed.shape[0], len(frames)
    names = check_names(names, S)
    if (totals is None) != (occ is None) or (zone_ev is None) != (zone_count is None):
        raise ValueError('totals and occ, zone_ev and zone_count come together')
    tag_group = (speed_i, det, count, tid)
    if any(a is None for a in tag_group) and not all(a is None for a in tag_group):
        raise ValueError('speed_i, det, count and tid come together')
    if totals is not None:
        totals, occ = np.asarray(totals, np.int32), np.asarray(occ, np.int32)
        if totals.shape != (S, 2, zones.MAX_LINES) or occ.shape != (S, zones.MAX_ZONES):
            raise ValueError('totals must be [%d, 2, 16] and occ [%d, 8]' % (S, S))
    if zone_ev is not None:
        zone_ev, zone_count = np.asarray(zone_ev, np.int32), np.asarray(zone_count, np.int32).reshape(-1)
        if zone_ev.ndim != 3 or zone_ev.shape[0] != S or zone_ev.shape[1] < 1 or zone_ev.shape[2] != zones.EV_COLS or zone_count.shape[0] != S:
            raise ValueError('zone_ev must be [%d, max_events >= 1, 12] with a count per stream' % S)
    status = None
    if det is not None:
        speed_i, det = np.asarray(speed_i, np.int32), np.asarray(det, np.float32)
        count, tid = np.asarray(count).reshape(-1), np.asarray(tid)
        if speed_i.ndim != 3 or speed_i.shape[0] != S or speed_i.shape[1] < 1 or speed_i.shape[2] != 8:
            raise ValueError('speed_i must be [%d, T >= 1, 8]' % S)
        if det.ndim != 3 or det.shape[2] < 28 or det.shape[0] < B or det.shape[1] < 1 or count.shape[0] < B or tid.ndim != 2 \
                or tid.shape[0] < B or tid.shape[1] != det.shape[1]:
            raise ValueError('det must be [>= %d, max_det >= 1, 28] with a count per frame and tid [>= %d, max_det]' % (B, B))
        status = np.zeros((B, det.shape[1]), np.int32)
    stream_of = list(range(B)) if stream_of is None else [int(s) for s in np.asarray(stream_of).reshape(-1)]
    if len(stream_of) != B:
        raise ValueError('stream_of must name the stream of each of the %d frames' % B)
    out = []
    for b, f in enumerate(frames):
        cv = _Canvas(f)
        s = stream_of[b]
        if 0 <= s < S:
            tags = []
            if det is not None:
                for r in range(max(0, min(int(count[b]), det.shape[1]))):
                    if int(tid[b][r]) < 0:
                        continue
                    q, x, y = plate_quad(det[b, r])
                    v = tag_speed(speed_i[s], tid[b][r])
                    if q == ST_EMPTY or v is None:
                        continue
                    status[b, r] = 1
                    tags.append((x, y, kmh_of(v)))
            for i0, i1, j0, j1, wt, col in scene_layers(cv.h, cv.w, packed[s], st, atlas, names[s], None if totals is None else totals[s],
                                                        None if occ is None else occ[s], alert_zones(zone_ev, zone_count, s), tags):
                cv.apply(i0, i1, j0, j1, wt, cv.colour(col))
        out.append(cv.out)
    return out, status
