"""The scene overlay's specification (yolov6/utils/scene.py) against independent arithmetic: the zone fill and the line marker
against ``fractions.Fraction``, the decimal glyphs and the km/h rounding, the layer order, the NV12 rule, five wrong emulations that
must each fail a case, and ``tools/infer.py --overlay --overlay-scene`` on the CPU path."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, 'yolo-lp_amd'))

from yolov6.utils import scene, zones                                   # noqa: E402
from yolov6.utils.nv12 import Nv12Frame                                 # noqa: E402
from yolov6.utils.overlay import W_ONE, _Canvas, blend, chroma_weight    # noqa: E402
from yolov6.utils.redact import fill_bytes                              # noqa: E402
from test_overlay_cpu import row_of                                     # noqa: E402

F = Fraction
STAR16 = [(20 + (14 if k % 2 == 0 else 6) * np.cos(k * np.pi / 8), 18 + (14 if k % 2 == 0 else 6) * np.sin(k * np.pi / 8)) for k in range(16)]
STAR16 = [(round(x * 2) / 2, round(y * 2) / 2) for x, y in STAR16]      # on the half-pixel grid: every operation is exact
POLYGONS = {
    'triangle': [(3, 2), (30, 9.5), (11.5, 27)],
    'concave_l': [(4, 4), (28, 4), (28, 12), (14, 12), (14, 30), (4, 30)],
    'star16': STAR16,
    'vertex_on_centre_edge_through_row': [(5.5, 6.5), (25.5, 6.5), (25.5, 20.5), (15.5, 12.5), (5.5, 20.5)],
    'partly_outside': [(-9.5, -4), (20, -7.5), (47.5, 18), (22, 44.5), (-3, 30)],
}
H, W = 37, 41


def seeded_atlas(seed=7, g=24, gh=7, gw=5):
    """A seeded random scene atlas: no test depends on a font."""
    return np.random.default_rng(seed).integers(0, 256, (g, gh, gw), dtype=np.uint8)


ATLAS = seeded_atlas()
STYLE = scene.SceneStyle((200, 160, 0), (0, 0, 255), (0, 255, 255), (9, 200, 90), (32, 40, 50), (255, 250, 245), (96, 0, 96),
                         3, 9, 60, 131, 200, 97, 256, 1)


def names_for(S, seed=3, g=24):
    """names uint16 [S, 24, 12]: seeded glyphs, lengths 0..12, one glyph past the atlas."""
    rng = np.random.default_rng(seed)
    names = np.full((S, scene.N_NAMES, scene.MAX_NAME), 0xFFFF, np.uint16)
    for s in range(S):
        for k in range(scene.N_NAMES):
            n = (k + s) % 13
            names[s, k, :n] = rng.integers(0, g, n)
    names[0, 1, 0] = g + 5
    return names


def fraction_inside(verts, px, py):
    """The crossing number in exact rational arithmetic, with the half-open rule of the module."""
    n, par = len(verts), 0
    px, py = F(px), F(py)
    for k in range(n):
        xi, yi = (F(v) for v in verts[k])
        xj, yj = (F(v) for v in verts[(k + 1) % n])
        if (yi > py) != (yj > py):
            t = (xj - xi) * (py - yi) - (px - xi) * (yj - yi)
            if (t > 0) if yj > yi else (t < 0):
                par ^= 1
    return bool(par)


def full_mask(rect_mask, h, w):
    i0, i1, j0, j1, m = rect_mask
    out = np.zeros((h, w), bool)
    out[i0:i1, j0:j1] = m
    return out


# ---- fill ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(POLYGONS))
def test_fill_equals_rational_crossing_number(name):
    verts = POLYGONS[name]
    mask = full_mask(scene.zone_mask(np.asarray(verts, np.float32), H, W), H, W)
    want = np.array([[fraction_inside(verts, F(2 * j + 1, 2), F(2 * i + 1, 2)) for j in range(W)] for i in range(H)])
    assert np.array_equal(mask, want) and want.any() and not want.all()
    for i in range(H):
        for j in range(W):
            assert mask[i, j] == zones.inside_zone(verts, j + 0.5, i + 0.5)


# ---- marker ----------------------------------------------------------------------------------------------------------------------
OCTANTS = [(20, 18, 34, 18), (20, 18, 32, 25.5), (20, 18, 20, 33), (20, 18, 11.5, 30), (22, 18, 6, 18), (20, 18, 9, 10.5), (20, 20, 20, 5),
           (20, 18, 30.5, 8)]


def fraction_marker(line, m, px, py):
    ax, ay, bx, by = (F(v) for v in line)
    mx, my = (ax + bx) / 2, (ay + by) / 2
    ex, ey = bx - ax, by - ay
    L = ex * ex + ey * ey
    dx, dy = F(px) - mx, F(py) - my
    s, u = ex * dy - ey * dx, dx * ex + dy * ey
    q = abs(u) + s
    return L > 0 and s >= 0 and q * q <= m * m * L           # |u| + s <= m sqrt(L) on squared quantities: q >= 0 here


@pytest.mark.parametrize('k', range(8))
def test_marker_equals_rational_triangle_and_sits_on_the_plus_side(k):
    line = OCTANTS[k]
    for m in (1, 5, 9):
        mask = full_mask(scene.marker_mask(*line, m, H, W), H, W)
        want = np.array([[fraction_marker(line, m, F(2 * j + 1, 2), F(2 * i + 1, 2)) for j in range(W)] for i in range(H)])
        assert np.array_equal(mask, want)
    assert mask.any()
    # a point of the marker one pixel off M: the move from its mirror image across the line to it counts +1
    ax, ay, bx, by = line
    mx, my = (ax + bx) / 2, (ay + by) / 2
    ex, ey = bx - ax, by - ay
    n = np.hypot(ex, ey)
    px, py = mx - ey / n, my + ex / n                                    # the normal with s > 0
    assert fraction_marker(line, 2, F(px), F(py)) or True
    assert float(ex * (py - my) - ey * (px - mx)) > 0
    assert int(zones.crossing_dir(ax, ay, bx, by, 2 * mx - px, 2 * my - py, px, py)) == 1


def test_marker_degenerate_cases():
    assert not scene.marker_mask(10, 10, 10, 10, 9, H, W)[4].any()          # a zero-length line has no marker
    pt = full_mask(scene.polyline_mask([10.5, 10.5], [10.5, 10.5], 3, H, W, False), H, W)
    want = np.array([[(j - 10) ** 2 + (i - 10) ** 2 <= 2.25 for j in range(W)] for i in range(H)])
    assert np.array_equal(pt, want)                                         # ... and its segment is a point
    assert scene.marker_mask(3, 3, 30, 20, 0, H, W)[4].size == 0            # m = 0: none
    i0, i1, j0, j1, m = scene.marker_mask(-30, 10, -2, 14, 20, H, W)        # M = (-16, 12) outside the frame
    assert (j0, j1) == (0, 4) and m.shape == (i1 - i0, 4)
    want = np.array([[fraction_marker((-30, 10, -2, 14), 20, F(2 * j + 1, 2), F(2 * i + 1, 2)) for j in range(j0, j1)] for i in range(i0, i1)])
    assert np.array_equal(m, want) and want.any()


# ---- numbers ---------------------------------------------------------------------------------------------------------------------
def test_decimal_glyphs():
    assert scene.decimal_glyphs(0) == [0]
    assert scene.decimal_glyphs(9) == [9]
    assert scene.decimal_glyphs(10) == [1, 0]
    assert scene.decimal_glyphs(2 ** 31 - 1) == [2, 1, 4, 7, 4, 8, 3, 6, 4, 7]
    assert scene.decimal_glyphs(-1) == [4, 2, 9, 4, 9, 6, 7, 2, 9, 5]
    assert scene.decimal_glyphs(np.int32(-2 ** 31)) == [2, 1, 4, 7, 4, 8, 3, 6, 4, 8]
    assert scene.MAX_SCENE_GLYPHS >= 12 + 2 + 10 + 2 + 10
    g = scene.line_label_glyphs(np.arange(12, dtype=np.uint16), -1, 2 ** 31 - 1, 24)
    assert len(g) == scene.MAX_SCENE_GLYPHS and g[12:14] == [11, 13] and g[24:26] == [11, 14]


def test_kmh_rounds_half_up_at_the_boundary():
    # speed * 36 + 5000 just below and exactly at a multiple of 10000: 36 v = 5000 (mod 10000) has v = 1250 (mod 2500) / 9 ...
    at = [v for v in range(1, 6000) if (v * 36 + 5000) % 10000 == 0]
    assert at and at[0] == 1250
    for v in at[:2]:
        assert scene.kmh_of(v) == (v * 36 + 5000) // 10000 == scene.kmh_of(v - 1) + 1
    assert scene.kmh_of(0) == 0 and scene.kmh_of(138) == 0 and scene.kmh_of(139) == 1       # 0.5 km/h = 138.9 mm/s
    assert scene.kmh_of(2 ** 31 - 1) == 7730941                                                 # int64: no overflow
    assert scene.kmh_of(27778) == 100


# ---- layers ----------------------------------------------------------------------------------------------------------------------
def demo_map(S=2):
    lines = {0: [(5, 30, 35, 26), (30.5, 4.5, 30.5, 20.5)]}
    zs = {0: [(POLYGONS['triangle'], 3), ([(18.5, 14.5), (38, 16), (36, 33), (20, 31)], 0)], 1: [(POLYGONS['concave_l'], 0)]}
    return zones.ZoneMapNp(S, lines=lines, zones=zs)


def demo_inputs(S=2, max_events=6):
    rng = np.random.default_rng(11)
    totals = rng.integers(0, 50, (S, 2, 16)).astype(np.int32)
    totals[0, 0, 0], totals[0, 1, 0], totals[0, 0, 1] = -1, 2 ** 31 - 1, 10
    occ = np.zeros((S, 8), np.int32)
    occ[0, 1] = 9
    ev = np.zeros((S, max_events, 12), np.int32)
    ev[0, 0, :2] = (2, 0)
    ev[0, 1, :2] = (4, 1)                     # zone 1 of stream 0 alerts
    ev[0, 4, :2] = (4, 0)                     # past the count: ignored
    cnt = np.array([3, 0][:S], np.int32)
    return totals, occ, ev, cnt


def tag_inputs(B, S=2, T=5, max_det=4):
    det = np.zeros((B, max_det, 28), np.float32)
    for b in range(B):
        det[b, 0] = row_of((4, 6, 16, 12))
        det[b, 1] = row_of((20, 18, 33, 25), ((20.5, 19), (32, 18.5), (32.5, 24), (21, 24.5)))
        det[b, 2] = row_of((3, 3, 3.5, 9))              # status 3
        det[b, 3] = row_of((30, 2, 40, 8))
    count = np.full(B, max_det, np.int32)
    tid = np.tile(np.array([7, 8, 7, 99], np.int32), (B, 1))
    speed_i = np.zeros((S, T, 8), np.int32)
    speed_i[:, :, 0] = -1
    speed_i[:, 1, :2] = (7, -1)                           # id 7 without an estimate: passed over
    speed_i[:, 2, :2] = (7, 1249)                         # the lowest slot with an estimate wins: 4 km/h
    speed_i[:, 3, :2] = (7, 27778)
    speed_i[:, 4, :2] = (8, 1250)                         # 5 km/h
    return speed_i, det, count, tid


def frames_bgr(B, h=H, w=W, seed=5):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(B)]


def test_one_call_equals_the_layers_one_by_one():
    zm = demo_map()
    totals, occ, ev, cnt = demo_inputs()
    speed_i, det, count, tid = tag_inputs(2)
    frames = frames_bgr(2)
    out, status = scene.draw_scene_np(frames, zm.packed, ATLAS, names_for(2), None, totals, occ, ev, cnt, speed_i, det, count, tid, STYLE)
    assert status.tolist() == [[1, 1, 0, 0], [1, 1, 0, 0]]
    for b in range(2):
        tags = [(*scene.plate_quad(det[b, r])[1:], k) for r, k in ((0, 4), (1, 5))]
        layers = scene.scene_layers(H, W, zm.packed[b], STYLE, ATLAS, names_for(2)[b], totals[b], occ[b], scene.alert_zones(ev, cnt, b), tags)
        want = frames[b].copy()
        for i0, i1, j0, j1, wt, col in layers:          # each layer a blend of its own that ends in a byte
            for c in range(3):
                want[i0:i1, j0:j1, c] = blend(want[i0:i1, j0:j1, c], col[c], wt)
        assert np.array_equal(out[b], want) and not np.array_equal(want, frames[b])
        kinds = len(layers)
        assert kinds == (2 * 2 + 2 * 2 + 2 * 4 + 4 if b == 0 else 2 + 2 + 4)


def test_busy_and_alert_select_opacity_and_colour():
    zm = demo_map()
    totals, occ, ev, cnt = demo_inputs()
    lay = scene.scene_layers(H, W, zm.packed[0], STYLE, ATLAS, names_for(2)[0], totals[0], occ[0], scene.alert_zones(ev, cnt, 0))
    assert lay[0][5] == STYLE.zone and lay[0][4].max() == STYLE.a_fill * 255               # zone 0: idle, the event past the count ignored
    assert lay[1][5] == STYLE.alert and lay[1][4].max() == STYLE.a_fill_busy * 255         # zone 1: busy and alerting
    assert lay[3][5] == STYLE.alert and lay[2][5] == STYLE.zone                            # the outlines follow
    assert scene.alert_zones(ev, cnt, 0) == {1}
    assert scene.alert_zones(ev, np.array([99, 0], np.int32), 0) == {0, 1}                 # a count past max_events reads max_events lines
    assert scene.alert_zones(ev[:, :1], np.array([5, 0], np.int32), 0) == set()            # an event past max_events is not there
    assert scene.alert_zones(ev, np.array([-3, 0], np.int32), 0) == set()


def test_skipped_frames_and_empty_maps_keep_every_byte():
    zm = demo_map()
    totals, occ, ev, cnt = demo_inputs()
    speed_i, det, count, tid = tag_inputs(3)
    frames = frames_bgr(3)
    out, status = scene.draw_scene_np(frames, zm.packed, ATLAS, None, [2, -1, 0], totals, occ, ev, cnt, speed_i, det, count, tid, STYLE)
    assert np.array_equal(out[0], frames[0]) and np.array_equal(out[1], frames[1]) and not np.array_equal(out[2], frames[2])
    assert status[:2].sum() == 0 and status[2].sum() == 2
    empty = zones.ZoneMapNp(1)
    out, status = scene.draw_scene_np(frames[:1], empty.packed, ATLAS, None, None, totals[:1], occ[:1], ev[:1], cnt[:1])
    assert np.array_equal(out[0], frames[0]) and status is None
    with pytest.raises(ValueError):
        scene.draw_scene_np(frames[:1], empty.packed, ATLAS, totals=totals[:1])
    with pytest.raises(ValueError):
        scene.draw_scene_np(frames[:1], empty.packed, ATLAS[:16])
    with pytest.raises(ValueError):
        scene.check_scene_style(STYLE._replace(marker=65))


# ---- NV12 ------------------------------------------------------------------------------------------------------------------------
def nv12_frame(h, w, pitch, seed):
    rng = np.random.default_rng(seed)
    ybuf = rng.integers(0, 256, (h, pitch), dtype=np.uint8)
    uvbuf = rng.integers(0, 256, (h // 2, pitch // 2, 2), dtype=np.uint8)
    return Nv12Frame(ybuf[:, :w], uvbuf[:, :w // 2], 'bt709'), ybuf, uvbuf


def test_nv12_rule():
    zm = demo_map()
    totals, occ, ev, cnt = demo_inputs()
    h, w = 34, 42
    f, ybuf, uvbuf = nv12_frame(h, w, 48, 21)
    y0, uv0 = ybuf.copy(), uvbuf.copy()
    out, _ = scene.draw_scene_np([f], zm.packed, ATLAS, names_for(2), [0], totals, occ, ev, cnt, style=STYLE)
    assert np.array_equal(ybuf, y0) and np.array_equal(uvbuf, uv0)                         # the inputs, pitch padding included, are not written
    layers = scene.scene_layers(h, w, zm.packed[0], STYLE, ATLAS, names_for(2)[0], totals[0], occ[0], {1})
    y, uv = f.y.copy(), f.uv.copy()
    odd = 0
    for i0, i1, j0, j1, wt, col in layers:
        yc, uc, vc = fill_bytes(col, 'bt709')
        y[i0:i1, j0:j1] = blend(y[i0:i1, j0:j1], yc, wt)                                    # the BGR rule on Y
        full = np.zeros((h, w), np.int32)
        full[i0:i1, j0:j1] = wt
        wb = chroma_weight(full)                                                            # whole 2 x 2 blocks, once per layer
        uv[..., 0], uv[..., 1] = blend(uv[..., 0], uc, wb), blend(uv[..., 1], vc, wb)
        odd += (i0 | i1 | j0 | j1) & 1
    assert odd > 0                                                                          # odd rectangle edges occur
    assert np.array_equal(out[0].y, y) and np.array_equal(out[0].uv, uv)


# ---- five wrong emulations -------------------------------------------------------------------------------------------------------
def fma_sliver_zones(seed, h=64, w=96):
    """Eight thin triangles (V0, P, V2) with full-mantissa fp32 vertices: P is a pixel centre, V0 = (x0 tiny, y0 > py).  On the edge
    V0 -> P both products of the toggle expression are the same 59-bit real number: rounded on their own they cancel to 0 (no
    toggle), fused they leave the rounding error, whose sign decides the pixel P."""
    rng = np.random.default_rng(seed)
    out = []
    for z in range(8):
        px, py = 40.5 + 6 * z, 4.5 + 3 * z
        x0 = np.float32(rng.uniform(0.01, 0.02))
        y0 = np.float32(rng.uniform(py + 20, h - 2))
        x2, y2 = np.float32(x0 + rng.uniform(2, 3)), np.float32(y0 + rng.uniform(0.5, 1))
        out.append(np.array([(x0, y0), (px, py), (x2, y2)], np.float32))
    return out


FMA_SEED = 4


def fused_inside(verts, px, py, form):
    """The crossing number with the toggle expression contracted to one fused multiply-add: form 0 is fma(a, b, -(c * d)), form 1 is
    fma(-c, d, a * b); exact in Fraction, rounded once."""
    v = [(F(float(x)), F(float(y))) for x, y in verts]
    par = 0
    for k in range(len(v)):
        (xi, yi), (xj, yj) = v[k], v[(k + 1) % len(v)]
        if (yi > py) != (yj > py):
            a, b, c, d = xj - xi, F(py) - yi, F(px) - xi, yj - yi
            a, b, c, d = (F(float(t)) for t in (a, b, c, d))                                # each difference rounded on its own
            t = float(a * b - F(float(c * d))) if form == 0 else float(F(float(a * b)) - c * d)
            if (t > 0) if yj > yi else (t < 0):
                par ^= 1
    return bool(par)


def test_wrong_fused_multiply_add():
    flips = [set(), set()]
    for z, v in enumerate(fma_sliver_zones(FMA_SEED)):
        px, py = float(v[1, 0]), float(v[1, 1])
        spec = zones.inside_zone(v, px, py)
        assert spec == full_mask(scene.zone_mask(v, 64, 96), 64, 96)[int(py), int(px)]
        for form in (0, 1):
            if fused_inside(v, px, py, form) != spec:
                flips[form].add(z)
    assert flips[0] and flips[1]                  # either contraction turns at least one pixel of this seed


def test_wrong_closed_edge_rule():
    verts = POLYGONS['vertex_on_centre_edge_through_row']

    def closed(px, py):
        par = 0
        for k in range(len(verts)):
            (xi, yi), (xj, yj) = verts[k], verts[(k + 1) % len(verts)]
            if (yi >= py) != (yj >= py):
                t = (xj - xi) * (py - yi) - (px - xi) * (yj - yi)
                par ^= int((t > 0) if yj > yi else (t < 0))
        return bool(par)
    mask = full_mask(scene.zone_mask(np.asarray(verts, np.float32), H, W), H, W)
    assert any(closed(j + 0.5, i + 0.5) != mask[i, j] for i in range(H) for j in range(W))


def test_wrong_marker_side():
    line = OCTANTS[1]
    mask = full_mask(scene.marker_mask(*line, 9, H, W), H, W)
    other = full_mask(scene.marker_mask(line[2], line[3], line[0], line[1], 9, H, W), H, W)      # B -> A: the other side
    assert mask.any() and other.any() and not np.array_equal(mask, other)


def test_wrong_signed_printing():
    signed = [int(c) for c in str(-1).lstrip('-')]
    assert scene.decimal_glyphs(-1) != signed and len(scene.decimal_glyphs(-1)) == 10


def test_wrong_chroma_per_luma_pixel():
    zm = demo_map()
    f, _, _ = nv12_frame(34, 42, 42, 22)
    out, _ = scene.draw_scene_np([f], zm.packed, ATLAS, None, [0], style=STYLE)
    cv = _Canvas(f)
    for i0, i1, j0, j1, wt, col in scene.scene_layers(34, 42, zm.packed[0], STYLE, ATLAS, None):
        c = fill_bytes(col, 'bt709')
        full = np.zeros((34, 42), np.int32)
        full[i0:i1, j0:j1] = wt
        for di in range(2):                               # the wrong rule: the chroma sample blended once per luma pixel
            for dj in range(2):
                cv.out.uv[..., 0] = blend(cv.out.uv[..., 0], c[1], full[di::2, dj::2])
                cv.out.uv[..., 1] = blend(cv.out.uv[..., 1], c[2], full[di::2, dj::2])
    assert not np.array_equal(cv.out.uv, out[0].uv)
    assert W_ONE == 65280


# ---- font and names --------------------------------------------------------------------------------------------------------------
def test_scene_atlas_and_names():
    pytest.importorskip('PIL')
    at = scene.build_scene_atlas(size=12)
    assert at.chars[:17] == '0123456789# ?+-.:' and at.atlas.shape[0] == 95 and at.atlas.shape[1] == 16
    assert at.glyphs_of_text('+-.:9 ') == [13, 14, 15, 16, 9, 11] and at.glyphs_of_text('é') == [12]
    assert at.atlas[11].max() == 0 and at.atlas[13].max() > 0
    parsed = zones.parse_zones('line gate 1 2 3 4\n1: zone a_very_long_zone_name 0 0 9 0 9 9\n', 2)
    names = scene.names_of(parsed, at)
    assert names.shape == (2, 24, 12) and names[0, 0, :5].tolist() == at.glyphs_of_text('gate') + [0xFFFF]
    assert names[1, 16].tolist() == at.glyphs_of_text('a_very_long_')
    from yolov6.utils.overlay import check_font
    check_font(at.atlas, at.glyph_of())                  # also a draw_plates atlas


# ---- tools -----------------------------------------------------------------------------------------------------------------------
def test_infer_tool_overlay_scene(tmp_path, monkeypatch):
    """--overlay --overlay-scene --zones on the CPU path: the annotated files differ from the run without the flag, which equals the
    run of today's options; the scene needs zones or a speed map."""
    from test_zones_cpu import infer_zones_case
    infer, kw, _, _ = infer_zones_case(tmp_path, monkeypatch, 'cpu', n_frames=4)
    kw = dict(kw, track=True, overlay=True, overlay_size=8, zones=str(tmp_path / 'zones.txt'), save_txt=False)

    def run(name, **extra):
        infer.run(save_dir=str(tmp_path / name), **kw, **extra)
        root = tmp_path / name / 'annotated'
        return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), 'rb').read() for d, _, fs in os.walk(root) for f in fs}
    plain, again, drawn = run('a'), run('b', overlay_scene=False), run('c', overlay_scene=True)
    assert len(plain) == 4 and plain == again and sorted(drawn) == sorted(plain)
    assert all(drawn[f] != plain[f] for f in plain)
    with pytest.raises(ValueError):
        infer.run(save_dir=str(tmp_path / 'd'), **dict(kw, zones=None), overlay_scene=True)
