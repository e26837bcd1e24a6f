"""The overlay's rule (yolov6/utils/overlay.py::draw_plates_np) against independent arithmetic: the outline pixel set against
``fractions.Fraction``; composition (one call with n rows = n calls with one); the blend's fixed points; the NV12 chroma weight;
label placement and glyph selection; counts, styles and the palette; a slow per-pixel emulation in plain integers that agrees
with the rule, and six deliberately wrong versions of it that do not, on the tests' own inputs; and ``build_atlas``."""
import math
from fractions import Fraction

import numpy as np
import pytest

from yolov6.utils.nv12 import Nv12Frame, bgr_to_nv12_np
from yolov6.utils.overlay import (GLYPH_HASH, GLYPH_SPACE, GLYPH_UNKNOWN, NO_GLYPH, Style, blend, build_atlas, chroma_weight,
                                  draw_plates_np, label_glyphs, label_origin, outline_mask)
from yolov6.utils.redact import fill_bytes

NAN = float('nan')
H, W = 30, 44
GH, GW, G = 7, 5, 40


def seeded_font(seed=5, gh=GH, gw=GW, g=G):
    """A seeded random atlas and glyph table: no test depends on a font.  One entry is 0xFFFF, one is past the atlas."""
    rng = np.random.default_rng(seed)
    atlas = rng.integers(0, 256, (g, gh, gw), dtype=np.uint8)
    glyph_of = rng.integers(0, g, (8, 64)).astype(np.uint16)
    glyph_of[0, 7] = NO_GLYPH
    glyph_of[1, 9] = g + 3
    return atlas, glyph_of


ATLAS, GLYPH_OF = seeded_font()
STYLES = [Style((10, 200, 30), (250, 40, 90), (60, 70, 200), (240, 250, 5), 3, 200, 97, 256, 1),
          Style((0, 0, 255), (255, 0, 0), (1, 2, 3), (200, 100, 50), 2, 256, 256, 131, 0)]


def row_of(box, corners=None, heads=(1, 2, 3, 4, 5, 6, 7, 8)):
    """One detection row: box (x1, y1, x2, y2), corners (TL, TR, BR, BL) as (x, y) pairs or None (NaN), the eight heads."""
    r = np.zeros(28, np.float32)
    r[:4] = box
    if corners is None:
        r[4:12] = NAN
    else:
        tl, tr, br, bl = corners
        r[4:12] = [tl[0], tl[1], bl[0], bl[1], br[0], br[1], tr[0], tr[1]]      # label order TL, BL, BR, TR
    r[12:20] = 0.5
    r[20:28] = heads
    return r


def scene():
    """Rows with half-integer coordinates in a 30 x 44 frame: two overlapping quads whose labels overlap (row 1's is shifted left
    at the right edge); a box-only row whose outline crosses both labels and whose label flips below; a status-3 row; a quad
    partly outside the frame; one wholly outside."""
    rows = [row_of((5, 9, 23, 21), ((6.5, 12), (20, 10.5), (21.5, 17), (7, 19.5))),
            row_of((13, 12, 32, 23), ((14, 14.5), (30.5, 13), (31, 20), (15.5, 21.5)), heads=(7, 9, 63, 64, -1, NAN, 1e30, 0)),
            row_of((1, 2, 40, 8)),
            row_of((3, 3, 3.5, 9)),
            row_of((34, 20, 50, 36), ((35, 22.5), (49, 21), (49.5, 33), (36, 35.5))),
            row_of((-30, -20, -10, -12), ((-29, -19.5), (-11, -19), (-10.5, -13), (-28, -12.5)))]
    return np.stack(rows)[None]


def frames_of(seed, nv12):
    bgr = np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    return [bgr_to_nv12_np(bgr, 'bt709')] if nv12 else [bgr]


def same(a, b):
    if isinstance(a, Nv12Frame):
        return np.array_equal(a.y, b.y) and np.array_equal(a.uv, b.uv)
    return np.array_equal(a, b)


# ---- the outline against fractions ------------------------------------------------------------------------------------------
def outline_set_fraction(x, y, t, h, w):
    """The outline's pixels by the definition: squared distance from the centre to the nearest point of a segment, in rationals."""
    x, y = [Fraction(v) for v in x], [Fraction(v) for v in y]
    lim = Fraction(t, 2) ** 2
    out = set()
    for i in range(h):
        for j in range(w):
            px, py = Fraction(2 * j + 1, 2), Fraction(2 * i + 1, 2)
            for a, b in ((0, 3), (3, 2), (2, 1), (1, 0)):
                ex, ey = x[b] - x[a], y[b] - y[a]
                L = ex * ex + ey * ey
                u = Fraction(0) if L == 0 else min(max(((px - x[a]) * ex + (py - y[a]) * ey) / L, Fraction(0)), Fraction(1))
                cx, cy = x[a] + u * ex - px, y[a] + u * ey - py
                if cx * cx + cy * cy <= lim:
                    out.add((i, j))
                    break
    return out


QUADS = [([4, 15.5, 16, 3.5], [3, 2.5, 9, 10.5]),                 # a slanted quad
         ([5, 12, 12, 5], [4, 4, 9, 9]),                           # an axis-aligned box on integers
         ([6.5, 6.5, 14, 7], [5, 5, 8.5, 12]),                     # a zero-length edge p0 -> p1
         ([-6, 7.5, 8, -5.5], [-3, -2.5, 6, 5.5]),                 # partly outside
         ([30, 40, 41, 31], [20, 19.5, 26, 27])]                   # wholly outside


@pytest.mark.parametrize('t', [1, 2, 3, 16])
def test_outline_equals_the_rational_definition(t):
    h, w = 16, 22
    for x, y in QUADS:
        i0, i1, j0, j1, m = outline_mask([float(v) for v in x], [float(v) for v in y], t, h, w)
        got = set((i0 + int(i), j0 + int(j)) for i, j in zip(*np.nonzero(m)))
        assert got == outline_set_fraction(x, y, t, h, w), (x, y, t)
    assert outline_mask([30.0, 40.0, 41.0, 31.0], [20.0, 19.5, 26.0, 27.0], 2, h, w)[4].size == 0
    assert outline_mask([4.0, 15.5, 16.0, 3.5], [3.0, 2.5, 9.0, 10.5], 0, h, w)[4].size == 0          # t = 0: no outline


# ---- composition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nv12', [False, True], ids=['bgr', 'nv12'])
def test_one_call_with_n_rows_equals_n_calls(nv12):
    det = scene()
    n = det.shape[1]
    tid = np.array([[3, 12, -1, 5, 40, 7]], np.int32)
    style = np.array([[0, 1, 0, 1, 0, 1]], np.int32)
    palette = np.array([[9, 99, 199], [250, 150, 50], [77, 7, 177]], np.uint8)
    frames = frames_of(1, nv12)
    kw = dict(tid=tid, style=style, styles=STYLES, palette=palette)
    (want,), st = draw_plates_np(frames, det, [n], ATLAS, GLYPH_OF, **kw)
    assert st.tolist() == [[1, 1, 2, 3, 1, 1]]
    cur = frames
    for r in range(n):
        cur, st1 = draw_plates_np(cur, det[:, r:r + 1], [1], ATLAS, GLYPH_OF, tid=tid[:, r:r + 1], style=style[:, r:r + 1],
                                  styles=STYLES, palette=palette)
        assert st1[0, 0] == st[0, r]
    assert same(cur[0], want) and not same(frames[0], want)
    # the order matters on these inputs: the labels of rows 0 and 1 overlap, row 2's outline crosses both
    (rev,), _ = draw_plates_np(frames, det[:, ::-1], [n], ATLAS, GLYPH_OF, tid=tid[:, ::-1].copy(), style=style[:, ::-1].copy(),
                               styles=STYLES, palette=palette)
    assert not same(rev, want)


# ---- blend ------------------------------------------------------------------------------------------------------------------
def test_blend_fixed_points():
    dst = np.arange(256, dtype=np.uint8)
    for fg in (0, 1, 127, 254, 255):
        assert np.array_equal(blend(dst, fg, np.zeros(256, np.int32)), dst)
        assert np.array_equal(blend(dst, fg, np.full(256, 65280, np.int32)), np.full(256, fg, np.uint8))
        for w in (1, 97 * 255, 97 * 13, 65279):
            assert int(blend(np.uint8(fg), fg, w)) == fg
    for d, fg, w in ((10, 200, 97 * 255), (255, 0, 1), (0, 255, 32640), (3, 250, 131 * 77)):
        num = fg * w + d * (65280 - w)
        assert int(blend(np.uint8(d), fg, w)) == int(Fraction(num, 65280) + Fraction(1, 2))      # nearest, half up


@pytest.mark.parametrize('nv12', [False, True], ids=['bgr', 'nv12'])
def test_alpha_zero_alpha_full_and_own_colour(nv12):
    det, frames = scene(), frames_of(2, nv12)
    n = det.shape[1]
    zero = [Style((1, 2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12), 3, 0, 0, 0, 1)]
    (out,), st = draw_plates_np(frames, det, [n], ATLAS, GLYPH_OF, styles=zero)
    assert same(out, frames[0]) and st.tolist() == [[1, 1, 2, 3, 1, 1]]
    # alpha 256 at coverage 255: the colour's bytes exactly (outlines and plate; the text layer is off)
    full = [Style((10, 200, 30), (250, 40, 90), (60, 70, 200), (0, 0, 0), 2, 256, 256, 0, 1)]
    (out,), _ = draw_plates_np(frames, det[:, :1], [1], ATLAS, GLYPH_OF, styles=full)
    cols = [fill_bytes(c, frames[0].matrix if nv12 else None) for c in full[0][:3]]
    if nv12:
        changed = out.y != frames[0].y
        assert changed.any() and set(out.y[changed].tolist()) <= set(c[0] for c in cols)
    else:
        changed = (out != frames[0]).any(axis=2)
        assert changed.any() and set(map(tuple, out[changed].tolist())) <= set(cols)
    # a frame already of the layer's colour is unchanged at any alpha
    one = [Style(*(((60, 70, 200),) * 4 + (3, 97, 201, 256, 1)))]
    flat = np.full((H, W, 3), (60, 70, 200), np.uint8)
    src = [bgr_to_nv12_np(flat, 'bt709')] if nv12 else [flat]
    (out,), _ = draw_plates_np(src, det, [n], ATLAS, GLYPH_OF, styles=one)
    assert same(out, src[0])


def test_nv12_chroma_weight_of_partly_covered_blocks():
    a = 97 * 255
    for covered in (1, 2, 3, 4):
        w = np.zeros((2, 2), np.int32)
        w.reshape(-1)[:covered] = a
        assert int(chroma_weight(w)[0, 0]) == (covered * a + 2) // 4
    # in a frame: a plate-only label (no outline, no text) whose rectangle starts and ends on odd pixels
    det = row_of((3, 13, 20, 18))[None, None]
    st = [Style((0, 0, 0), (0, 0, 0), (255, 255, 255), (0, 0, 0), 0, 0, 97, 0, 1)]
    src = Nv12Frame(np.zeros((H, W), np.uint8), np.zeros((H // 2, W // 2, 2), np.uint8), 'bt601f')
    (out,), _ = draw_plates_np([src], det, [1], ATLAS, GLYPH_OF, styles=st)
    ly, lx, hh, ww = label_origin([3.0, 20.0, 20.0, 3.0], [13.0, 13.0, 18.0, 18.0], 0, 8, GH, GW, 1, W)
    assert (ly, lx, hh, ww) == (4, 2, 9, 42) and lx + ww == W
    fy, fu, fv = fill_bytes((255, 255, 255), 'bt601f')
    cover = np.zeros((H, W), np.int32)
    cover[ly:ly + hh, lx:lx + ww] = 1
    counts = cover.reshape(H // 2, 2, W // 2, 2).sum(axis=(1, 3))
    assert set(np.unique(counts).tolist()) >= {0, 2, 4}
    for ci in range(H // 2):
        for cj in range(W // 2):
            wb = (int(counts[ci, cj]) * a + 2) >> 2
            assert int(out.uv[ci, cj, 0]) == (fu * wb + 32640) // 65280 and int(out.uv[ci, cj, 1]) == (fv * wb + 32640) // 65280
    assert np.array_equal(out.y, ((fy * a * cover + 32640) // 65280).astype(np.uint8))


# ---- label ------------------------------------------------------------------------------------------------------------------
def test_label_placement():
    x, y = [10.5, 20.0, 20.0, 10.5], [15.5, 15.5, 19.0, 19.0]
    assert label_origin(x, y, 3, 8, GH, GW, 1, W) == (15 - 2 - 9, 2, 9, 42)                    # above; shifted left to fit
    assert label_origin(x, y, 3, 4, GH, GW, 1, W) == (4, 10, 9, 22)                            # above, at the plate's left edge
    assert label_origin(x, [5.5, 5.5, 9.2, 9.2], 3, 4, GH, GW, 1, W) == (10 + 2, 10, 9, 22)    # flipped below: ceil(9.2) + q
    assert label_origin([40.0, 43.0, 43.0, 40.0], y, 2, 4, GH, GW, 1, W) == (5, W - 22, 9, 22)  # at the right edge
    assert label_origin(x, y, 2, 20, GH, GW, 2, W) == (15 - 1 - 11, 0, 11, 104)                # wider than the frame: lx = 0
    assert label_origin([-1e30, 3.0, 3.0, -1e30], [1e30, 1e30, 3e30, 3e30], 2, 4, GH, GW, 1, W)[:2] == ((1 << 20) - 1 - 9, 0)
    # a label wider than the frame is clipped; a status-2 row hangs its label on the box
    det = row_of((30, 15, 43, 20))[None, None]
    tid = np.array([[2 ** 31 - 1]], np.int32)
    src = frames_of(3, False)
    (out,), st = draw_plates_np(src, det, [1], ATLAS, GLYPH_OF, tid=tid, styles=[STYLES[1]])
    assert st[0, 0] == 2
    ly, lx, hh, ww = label_origin([30.0, 43.0, 43.0, 30.0], [15.0, 15.0, 20.0, 20.0], 2, 20, GH, GW, 0, W)
    assert (lx, ww) == (0, 100) and ly == 15 - 1 - 7
    assert (out[ly:ly + hh] != src[0][ly:ly + hh]).any(axis=2).mean() > 0.9                    # the plate layer at alpha 256
    assert np.array_equal(out[:ly], src[0][:ly])


def test_label_glyphs():
    row = row_of((0, 0, 5, 5), heads=(7, 9, 63, 64, -1, NAN, 1e30, 0))
    heads = [GLYPH_UNKNOWN, GLYPH_UNKNOWN, int(GLYPH_OF[2, 63]), GLYPH_UNKNOWN, GLYPH_UNKNOWN, GLYPH_UNKNOWN, GLYPH_UNKNOWN,
             int(GLYPH_OF[7, 0])]                      # [0][7] is 0xFFFF, [1][9] is past the atlas
    assert label_glyphs(row, None, GLYPH_OF, G) == heads
    assert label_glyphs(row, -1, GLYPH_OF, G) == heads
    assert label_glyphs(row, 0, GLYPH_OF, G) == [GLYPH_HASH, 0, GLYPH_SPACE] + heads
    assert label_glyphs(row, 9, GLYPH_OF, G) == [GLYPH_HASH, 9, GLYPH_SPACE] + heads
    assert label_glyphs(row, 10, GLYPH_OF, G) == [GLYPH_HASH, 1, 0, GLYPH_SPACE] + heads
    big = label_glyphs(row, 2 ** 31 - 1, GLYPH_OF, G)
    assert big == [GLYPH_HASH, 2, 1, 4, 7, 4, 8, 3, 6, 4, 7, GLYPH_SPACE] + heads and len(big) == 20
    assert label_glyphs(row, 10, GLYPH_OF, G, show_id=False) == heads
    assert label_glyphs(row_of((0, 0, 5, 5), heads=(0.99, 1.0, 62.5, 63.99, 5, 5, 5, 5)), None, GLYPH_OF, G)[:4] == [
        int(GLYPH_OF[0, 0]), int(GLYPH_OF[1, 1]), int(GLYPH_OF[2, 62]), int(GLYPH_OF[3, 63])]


# ---- rows -------------------------------------------------------------------------------------------------------------------
def test_counts_styles_and_palette():
    det = scene()
    n = det.shape[1]
    src = frames_of(4, False)
    full, st_full = draw_plates_np(src, det, [n], ATLAS, GLYPH_OF, styles=STYLES)
    for c in (-1, 0):
        (out,), st = draw_plates_np(src, det, [c], ATLAS, GLYPH_OF, styles=STYLES)
        assert same(out, src[0]) and not st.any()
    (out,), st = draw_plates_np(src, det, [n + 3], ATLAS, GLYPH_OF, styles=STYLES)
    assert same(out, full[0]) and np.array_equal(st, st_full)
    (two,), st = draw_plates_np(src, det, [2], ATLAS, GLYPH_OF, styles=STYLES)
    (alone,), _ = draw_plates_np(src, det[:, :2], [2], ATLAS, GLYPH_OF, styles=STYLES)
    assert same(two, alone) and st.tolist() == [[1, 1, 0, 0, 0, 0]]
    # style -1 skips a row (status 0): the frame is that of the other rows
    style = np.array([[0, -1, 1, 0, -5, 7]], np.int32)                            # 7: past the last style -> the last
    (out,), st = draw_plates_np(src, det, [n], ATLAS, GLYPH_OF, style=style, styles=STYLES)
    keep = [0, 2, 3, 5]
    (want,), _ = draw_plates_np(src, det[:, keep], [4], ATLAS, GLYPH_OF, style=np.array([[0, 1, 0, 1]], np.int32), styles=STYLES)
    assert same(out, want) and st.tolist() == [[1, 0, 2, 3, 0, 1]]
    # the palette colours quad and plate by tid % P, a row without an id keeps its style's
    palette = np.array([[9, 99, 199], [250, 150, 50], [77, 7, 177]], np.uint8)
    tid = np.array([[4, -1, 0, 0, 0, 0]], np.int32)
    (out,), _ = draw_plates_np(src, det[:, :2], [2], ATLAS, GLYPH_OF, tid=tid[:, :2], styles=STYLES[1:], palette=palette, show_id=False)
    swapped = [STYLES[1]._replace(quad=(250, 150, 50), plate=(250, 150, 50))]
    (r0,), _ = draw_plates_np(src, det[:, :1], [1], ATLAS, GLYPH_OF, styles=swapped)
    (want,), _ = draw_plates_np([r0], det[:, 1:2], [1], ATLAS, GLYPH_OF, styles=STYLES[1:])
    assert same(out, want)
    # label and draw_box switches
    (nolab,), _ = draw_plates_np(src, det[:, :1], [1], ATLAS, GLYPH_OF, styles=STYLES, label=False)
    (nobox,), _ = draw_plates_np(src, det[:, :1], [1], ATLAS, GLYPH_OF, styles=STYLES, label=False, draw_box=False)
    assert not same(nolab, nobox) and not same(nobox, src[0]) and np.array_equal(nolab[:7], src[0][:7])
    (box2,), _ = draw_plates_np(src, det[:, 2:3], [1], ATLAS, GLYPH_OF, styles=STYLES, label=False, draw_box=False)
    assert not same(box2, src[0])                                                  # a status-2 row keeps its only shape
    assert src[0].flags.writeable and same(src[0], frames_of(4, False)[0])         # the inputs are not written


# ---- a per-pixel emulation in plain integers, and wrong versions of it -----------------------------------------------------
WRONG = ('reverse', 'chroma_one', 'noround', 'noflip', 'line', 'halfwidth')


def emulate(frame, rows, tids, styles, style_of, wrong=None):
    """``draw_plates_np`` of one frame restated pixel by pixel on doubled integer coordinates (the scene's coordinates are
    multiples of 0.5), with one of ``WRONG`` built in on request.  rows with status 3 or style < 0 are the caller's to leave out."""
    nv12 = isinstance(frame, Nv12Frame)
    if nv12:
        y, uv = frame.y.astype(int).tolist(), frame.uv.astype(int).tolist()
    else:
        px = frame.astype(int).tolist()
    order = range(len(rows) - 1, -1, -1) if wrong == 'reverse' else range(len(rows))

    def mix(d, fg, w):
        return (fg * w + d * (65280 - w) + (0 if wrong == 'noround' else 32640)) // 65280

    def paint(wmap, col):
        col = fill_bytes(col, frame.matrix if nv12 else None)
        if not nv12:
            for (i, j), w in wmap.items():
                px[i][j] = [mix(px[i][j][c], col[c], w) for c in range(3)]
            return
        for (i, j), w in wmap.items():
            y[i][j] = mix(y[i][j], col[0], w)
        for ci, cj in sorted(set((i // 2, j // 2) for i, j in wmap)):
            ws = [wmap.get((2 * ci + a, 2 * cj + b), 0) for a in (0, 1) for b in (0, 1)]
            wb = ws[0] if wrong == 'chroma_one' else (sum(ws) + 2) >> 2
            uv[ci][cj] = [mix(uv[ci][cj][0], col[1], wb), mix(uv[ci][cj][1], col[2], wb)]

    def outline(X, Y, t, a):
        lim = (4 * t * t) if wrong == 'halfwidth' else t * t                  # doubled coordinates: (t / 2)^2 becomes t^2
        wmap = {}
        if t == 0:
            return wmap
        for i in range(max(0, min(Y) // 2 - t - 2), min(H, max(Y) // 2 + t + 3)):
            for j in range(max(0, min(X) // 2 - t - 2), min(W, max(X) // 2 + t + 3)):
                P = (2 * j + 1, 2 * i + 1)
                for k0, k1 in ((0, 3), (3, 2), (2, 1), (1, 0)):
                    ex, ey, dx, dy = X[k1] - X[k0], Y[k1] - Y[k0], P[0] - X[k0], P[1] - Y[k0]
                    L, d, cr = ex * ex + ey * ey, dx * ex + dy * ey, dx * ey - dy * ex
                    if wrong == 'line':
                        hit = cr * cr <= lim * L
                    elif d <= 0:
                        hit = dx * dx + dy * dy <= lim
                    elif d >= L:
                        hit = (P[0] - X[k1]) ** 2 + (P[1] - Y[k1]) ** 2 <= lim
                    else:
                        hit = cr * cr <= lim * L
                    if hit:
                        wmap[(i, j)] = a * 255
                        break
        return wmap

    for r in order:
        row, st = rows[r], styles[style_of[r]]
        c = [int(round(2 * float(v))) if math.isfinite(v) else None for v in row[:12]]
        corners = None not in c[4:]
        bx, by = [c[0], c[2], c[2], c[0]], [c[1], c[1], c[3], c[3]]
        paint(outline(bx, by, st.t, st.a_line), st.box)
        X, Y = bx, by
        if corners:
            X, Y = [c[4], c[10], c[8], c[6]], [c[5], c[11], c[9], c[7]]
            paint(outline(X, Y, st.t, st.a_line), st.quad)
        tid = tids[r]
        g = ([10] + [int(ch) for ch in '%d' % tid] + [11]) if tid >= 0 else []
        for p in range(8):
            v = float(row[20 + p])
            k = int(GLYPH_OF[p][int(v)]) if math.isfinite(v) and 0 <= v < 64 else 12
            g.append(12 if k >= G else k)
        LW, LH, q = len(g) * GW + 2 * st.pad, GH + 2 * st.pad, (st.t + 1) // 2
        ly = min(Y) // 2 - q - LH
        if ly < 0 and wrong != 'noflip':
            ly = -((-max(Y)) // 2) + q
        lx = max(min(min(X) // 2, W - LW), 0)
        cells = [(i, j) for i in range(max(ly, 0), min(ly + LH, H)) for j in range(lx, min(lx + LW, W))]
        paint({ij: st.a_plate * 255 for ij in cells}, st.plate)
        text = {}
        for i, j in cells:
            gi, gj = i - ly - st.pad, j - lx - st.pad
            if 0 <= gi < GH and 0 <= gj < len(g) * GW:
                text[(i, j)] = st.a_text * int(ATLAS[g[gj // GW]][gi][gj % GW])
        paint(text, st.text)
    if nv12:
        return Nv12Frame(np.array(y, np.uint8), np.array(uv, np.uint8), frame.matrix)
    return np.array(px, np.uint8)


def emulation_case(nv12):
    det = scene()
    tid = np.array([[3, 12, -1, 5, 40, 7]], np.int32)
    style = np.array([[0, 1, 0, 1, 0, 1]], np.int32)
    frames = frames_of(6, nv12)
    (want,), st = draw_plates_np(frames, det, [6], ATLAS, GLYPH_OF, tid=tid, style=style, styles=STYLES)
    live = [r for r in range(6) if st[0, r] != 3]
    args = (frames[0], [det[0, r] for r in live], [int(tid[0, r]) for r in live], STYLES, [int(style[0, r]) for r in live])
    return want, args


def test_the_rule_equals_a_per_pixel_integer_emulation():
    for nv12 in (False, True):
        want, args = emulation_case(nv12)
        assert same(emulate(*args), want)


@pytest.mark.parametrize('wrong', WRONG)
def test_wrong_emulations_are_caught(wrong):
    """Each deliberately wrong restatement differs from the rule on the BGR or the NV12 case: the inputs discriminate."""
    differs = False
    for nv12 in ((True,) if wrong == 'chroma_one' else (False, True)):
        want, args = emulation_case(nv12)
        differs = differs or not same(emulate(*args, wrong=wrong), want)
    assert differs


# ---- the entry point on the CPU device ---------------------------------------------------------------------------------------
def test_infer_overlay_on_the_cpu_device(tmp_path, monkeypatch):
    """Inferer(overlay=True) on the CPU: annotated/<image name> is draw_plates_np of the rows returned, on top of the mosaic when
    the frame is redacted too; with track, redact_hold and save_jpeg it writes annotated/<stem>.jpg; without overlay no folder."""
    import importlib
    import os
    import sys
    import torch
    from PIL import Image
    from conftest import REPO
    from yolov6.core.inferer import Inferer
    from yolov6.utils.redact import redact_plates_np
    from yolov6.utils.synth import build_synthetic
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    ckpt = tmp_path / 'tiny.pt'
    torch.save({'model': build_synthetic(os.path.join(REPO, 'configs', 'yololps.py'), width=0.0625, sigma=1.5).half(), 'ema': None}, str(ckpt))
    img_dir = tmp_path / 'imgs'
    img_dir.mkdir()
    rng = np.random.default_rng(12)
    frames = [rng.integers(0, 255, (120, 96, 3), dtype=np.uint8) for _ in range(2)]
    for i, f in enumerate(frames):
        Image.fromarray(f).save(str(img_dir / ('f%d.png' % i)))
    kw = dict(weights=str(ckpt), source=str(img_dir), yaml=None, img_size=[128, 128], conf_thres=0.06, iou_thres=0.45, max_det=20,
              device='cpu', not_save_img=True)
    infer.run(save_dir=str(tmp_path / 'plain'), **kw)
    assert not (tmp_path / 'plain' / 'annotated').exists()
    dets = infer.run(save_dir=str(tmp_path / 'o'), overlay=True, overlay_size=12, redact='mosaic', redact_cell=8, **kw)
    font, styles = build_atlas([], [], [], 12, None), Inferer.make_overlay_styles(12, 2, (256, 160, 256))
    assert sum(len(d) for d in dets) > 0
    for i, f in enumerate(frames):
        d = dets[i].cpu().numpy()
        det = np.zeros((1, max(len(d), 1), 28), np.float32)
        det[0, :len(d)] = d
        src = np.ascontiguousarray(f[:, :, ::-1])
        mosaic, _ = redact_plates_np([src], det, [len(d)], 'mosaic', 8, 0.1)
        (want,), _ = draw_plates_np(mosaic, det, [len(d)], *font, styles=styles)
        got = np.asarray(Image.open(str(tmp_path / 'o' / 'annotated' / ('f%d.png' % i))))
        assert np.array_equal(got, want[:, :, ::-1]) and (want != mosaic[0]).any()
    infer.run(save_dir=str(tmp_path / 'j'), overlay=True, overlay_size=12, track=True, redact='fill', redact_hold=True, save_jpeg=80, **kw)
    assert sorted(os.listdir(str(tmp_path / 'j' / 'annotated'))) == ['f0.jpg', 'f1.jpg']
    assert Image.open(str(tmp_path / 'j' / 'annotated' / 'f0.jpg')).size == (96, 120)
    with pytest.raises(ValueError):
        infer.run(save_dir=str(tmp_path / 'l'), overlay=True, track=True, redact='fill', redact_hold=True, redact_lookback=2, **kw)


# ---- the atlas builder ------------------------------------------------------------------------------------------------------
def test_build_atlas():
    pro = ['京', '沪', 'A']                                  # two provinces, one ASCII stand-in
    alp = list('ABCDEFGH')
    ads = list('ABCDEFGH0123456789')
    atlas, glyph_of = build_atlas(pro, alp, ads, size=16)
    assert atlas.dtype == np.uint8 and atlas.ndim == 3 and glyph_of.dtype == np.uint16 and glyph_of.shape == (8, 64)
    n, gh, gw = atlas.shape
    assert n == 13 + 8 and gh == 20 and 2 <= gw <= 64                # digits are shared with the fixed glyphs
    for k in list(range(11)) + [12]:
        assert atlas[k].max() > 128, k                                # the fixed glyphs are there ...
    assert atlas[11].max() == 0                                       # ... and the space is empty
    for a in range(10):
        for b in range(a + 1, 10):
            assert not np.array_equal(atlas[a], atlas[b])
    assert glyph_of[0, 0] == NO_GLYPH and glyph_of[0, 1] == NO_GLYPH and glyph_of[0, 2] == glyph_of[1, 0] == glyph_of[2, 0]
    assert glyph_of[2, 8] == 0 and glyph_of[7, 17] == 9 and glyph_of[1, 8] == NO_GLYPH and glyph_of[3, 18] == NO_GLYPH
    used = glyph_of[glyph_of != NO_GLYPH]
    assert used.max() < n
    # each name is centred in its cell: the ink's margins left and right differ by at most one column (+ the font's bearing)
    ink = np.nonzero(atlas[8].max(axis=0))[0]
    assert abs(int(ink[0]) - (gw - 1 - int(ink[-1]))) <= 2
    # the builder's output drives the rule
    det = scene()
    (out,), st = draw_plates_np(frames_of(8, False), det, [6], atlas, glyph_of)
    assert st.tolist() == [[1, 1, 2, 3, 1, 1]]
