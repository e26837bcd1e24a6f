"""Lines and zones on live plate tracks, on the CPU: the arithmetic of yolov6/utils/zones.py against exact rational arithmetic, the
edges of its rule, scenarios through PlateTrackerNp.enable_zones (a gate line both ways, min_hits, enter / dwell / left, a track
that ends inside, a missed track that keeps dwelling, a slot reused in one call, flush and reset, the chord of a call with two
frames, a stream without frames, max_events at its edges), switching it on beside every other add-on, and the parser and the
validation of the geometry.  The scene generators and comparison helpers of tests/test_zones_gpu.py live here as well."""
from fractions import Fraction

import numpy as np
import pytest

import test_track_cpu as T

f32, f64 = np.float32, np.float64
NAN, INF = float('nan'), float('inf')
SQUARE = [(200, 50), (300, 50), (300, 150), (200, 150)]
GATE = (100, 200, 100, 0)                     # A below, B above: a move to the right crosses it +1


def box_at(cx, cy, w=60, h=20):
    return (cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2)


def step_rows(trk, rows_per_frame, stream_of=None, flush=None, max_det=4):
    det, count = T.frames_of(rows_per_frame, max_det)
    trk.update(det, count, stream_of=[0] * len(rows_per_frame) if stream_of is None else stream_of, flush=flush)
    return trk.last_zone


def events(zone, s=0):
    """The written events of stream ``s`` as tuples (kind, index, id, slot, frame, value)."""
    ev, count = zone[0], zone[1]
    return [tuple(int(v) for v in ev[s, k, :6]) for k in range(min(int(count[s]), ev.shape[1]))]


def drive(trk, centres, **kw):
    """One call per centre (None: a frame without rows) on stream 0; the events of every call."""
    return [events(step_rows(trk, [[] if c is None else [T.make_row(box_at(*c))]], **kw)) for c in centres]


def tracker(zone_lines=None, zone_polys=None, min_hits=1, max_events=None, n_streams=1, **kw):
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.zones import ZoneMapNp
    trk = PlateTrackerNp(n_streams, **dict(dict(max_tracks=4, max_age=2), **kw))
    trk.enable_zones(ZoneMapNp(n_streams, {0: zone_lines or []}, {0: zone_polys or []}), min_hits, max_events)
    return trk


# ---- exact arithmetic ----------------------------------------------------------------------------------------------------------
def frac_cross(p, q, r):
    return (q[0] - p[0]) * (r[1] - p[1]) - (q[1] - p[1]) * (r[0] - p[0])


def frac_crossing(a, b, p0, p1):
    d0, d1, e0, e1 = frac_cross(a, b, p0), frac_cross(a, b, p1), frac_cross(p0, p1, a), frac_cross(p0, p1, b)
    if not ((e0 <= 0 and e1 > 0) or (e0 > 0 and e1 <= 0)):
        return 0
    return 1 if d0 <= 0 and d1 > 0 else (-1 if d0 > 0 and d1 <= 0 else 0)


def frac_inside(verts, p):
    par = 0
    for i in range(len(verts)):
        (xi, yi), (xj, yj) = verts[i], verts[(i + 1) % len(verts)]
        if (yi > p[1]) != (yj > p[1]):
            t = (xj - xi) * (p[1] - yi) - (p[0] - xi) * (yj - yi)
            par ^= int(t > 0 if yj > yi else t < 0)
    return bool(par)


def grid_points(rng, n, span):
    """[n, 2] of Fractions on the grid of multiples of 1/8 in [0, span]."""
    return [(Fraction(int(a), 8), Fraction(int(b), 8)) for a, b in rng.integers(0, 8 * span + 1, (n, 2))]


def star_polygon(rng, n, cx, cy, r0, r1, step=1.0):
    """A simple polygon of ``n`` vertices, star-shaped about (cx, cy), concave for r0 < r1; vertices on the grid of ``step``."""
    ang = np.linspace(0, 2 * np.pi, n, endpoint=False) + rng.uniform(-0.3, 0.3, n) * (np.pi / n)
    rad = np.where(np.arange(n) % 2 == 0, r1, r0) if n > 4 else np.full(n, float(r1))
    v = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1)
    return np.round(v / step) * step


@pytest.mark.parametrize('span', [4096, 1])
def test_cross_and_crossing_equal_rational_arithmetic(span):
    """On the grid of multiples of 1/8 in [0, 4096] every fp64 product is exact; span 1 makes points on lines and ends common."""
    from yolov6.utils.zones import cross, crossing_dir
    rng = np.random.default_rng(span)
    n, seen = 3000, {-1: 0, 0: 0, 1: 0}
    on_line = 0
    pts = [grid_points(rng, n, span) for _ in range(4)]
    arr = [np.array([[float(x), float(y)] for x, y in p], f32) for p in pts]
    got_c = cross(arr[0][:, 0], arr[0][:, 1], arr[1][:, 0], arr[1][:, 1], arr[2][:, 0], arr[2][:, 1])
    got_d = crossing_dir(arr[0][:, 0], arr[0][:, 1], arr[1][:, 0], arr[1][:, 1], arr[2][:, 0], arr[2][:, 1], arr[3][:, 0], arr[3][:, 1])
    for k in range(n):
        a, b, p0, p1 = (p[k] for p in pts)
        want = frac_cross(a, b, p0)
        assert Fraction(float(got_c[k])) == want
        on_line += want == 0
        d = frac_crossing(a, b, p0, p1)
        assert int(got_d[k]) == d, (a, b, p0, p1)
        seen[d] += 1
    assert min(seen.values()) > 20 and (span > 1 or on_line > 50), (seen, on_line)


@pytest.mark.parametrize('n_verts', [3, 4, 16])
def test_inside_equals_rational_arithmetic(n_verts):
    """Convex and concave polygons (16 vertices: a star) on the 1/8 grid; the points include every vertex, edge midpoints and the
    heights of the vertices, where the half-open rule decides."""
    from yolov6.utils.zones import inside_zone
    rng = np.random.default_rng(n_verts)
    n_in = n_edge = 0
    for _ in range(12):
        v = star_polygon(rng, n_verts, 2048.0, 2048.0, 400.0, 1900.0, step=0.125)
        vf = [(Fraction(float(x)), Fraction(float(y))) for x, y in v]
        pts = [tuple(p) for p in v] + [tuple((v[i] + v[(i + 1) % n_verts]) / 2) for i in range(n_verts)]
        pts += [(float(x), float(v[i, 1])) for i in range(n_verts) for x in rng.integers(0, 4097, 4)]
        pts += [(float(a) / 8, float(b) / 8) for a, b in rng.integers(0, 8 * 4096 + 1, (150, 2))]
        for p in pts:
            want = frac_inside(vf, (Fraction(p[0]), Fraction(p[1])))
            assert inside_zone(v.astype(f32), f32(p[0]), f32(p[1])) == want, (v, p)
            n_in += want
        n_edge += 2 * n_verts
    assert n_in > 100 and n_edge > 0


# ---- the edges of the rule -------------------------------------------------------------------------------------------------------
def test_points_on_the_line_its_ends_and_degenerate_moves():
    from yolov6.utils.zones import crossing_dir
    line = (0.0, 0.0, 0.0, 10.0)                                                # A = (0, 0) -> B = (0, 10): x > 0 is the negative side

    def d(p0, p1):
        return int(crossing_dir(*line, p0[0], p0[1], p1[0], p1[1]))
    assert d((5, 5), (-5, 5)) == 1 and d((-5, 5), (5, 5)) == -1
    assert d((5, 5), (0, 5)) == 0 and d((0, 5), (-5, 5)) == 1                   # a stop on the line: counted once, when it goes on
    assert d((-5, 5), (0, 5)) == -1 and d((0, 5), (5, 5)) == 0                  # ... from the other side: counted when it gets there
    assert d((0, 5), (5, 5)) + d((5, 5), (0, 5)) == 0                           # on the line, away on the negative side and back: nothing
    assert [d((-5, 5), (0, 5)), d((0, 5), (-5, 5))] == [-1, 1]                   # touches and returns: -1 then +1 ...
    assert [d((0, 5), (-5, 5)), d((-5, 5), (0, 5))] == [1, -1]                   # ... and +1 then -1
    assert d((5, 15), (-5, 15)) == 0 and d((5, -1), (-5, -1)) == 0              # past either end of the segment
    assert d((5, 10), (-5, 10)) + d((5, 0), (-5, 0)) == 1                       # through an end: exactly one of the two ends belongs to it
    assert d((0, 2), (0, 8)) == 0 and d((0, -5), (0, 15)) == 0                  # collinear
    assert d((3, 5), (3, 5)) == 0 and d((3, 2), (3, 8)) == 0                    # d0 == d1: no move, and a move parallel to the line
    for bad in (NAN, INF, -INF):
        assert d((bad, 5), (-5, 5)) == 0 and d((5, 5), (bad, 5)) == 0 and d((5, bad), (-5, 5)) == 0 and d((5, 5), (-5, bad)) == 0
    assert d((-5, 5), (INF, 5)) == 0                                            # the arithmetic alone would call this a crossing


def test_points_on_vertices_and_horizontal_edges():
    from yolov6.utils.zones import inside_zone
    sq = np.array(SQUARE, f32)
    assert inside_zone(sq, 250, 100) and not inside_zone(sq, 199, 100) and not inside_zone(sq, 250, 151)
    # the half-open rule: the left and top edges belong to the square, the right and bottom ones do not; of the corners only the first
    assert inside_zone(sq, 200, 100) and not inside_zone(sq, 300, 100)
    assert inside_zone(sq, 250, 50) and not inside_zone(sq, 250, 150)
    assert [inside_zone(sq, *p) for p in SQUARE] == [True, False, False, False]
    for bad in (NAN, INF, -INF):
        assert not inside_zone(sq, bad, 100) and not inside_zone(sq, 250, bad)
    tri = np.array([(0, 0), (10, 0), (5, 10)], f32)                             # a vertex at the height of the point
    assert inside_zone(tri, 5, 5) and not inside_zone(tri, 5, 10) and not inside_zone(tri, 11, 0) and not inside_zone(tri, -1, 0)


def test_nan_and_infinite_boxes_cause_no_event():
    trk = tracker([GATE], [(SQUARE, 1)])
    for bad in (NAN, INF, -INF):
        for k in range(4):
            box = [90.0 + 10 * k, 90.0, 150.0 + 10 * k, 110.0]
            box[k] = bad
            zone = step_rows(trk, [[T.make_row(tuple(box))]])
            assert int(zone[1][0]) == 0 and not zone[0].any() and not zone[2].any() and not zone[3].any()
    assert trk.zone_memo[0, :4, 0].any()                                        # the tracks are there, their anchors are not finite


# ---- scenarios through PlateTrackerNp --------------------------------------------------------------------------------------------
def test_a_gate_line_counts_both_directions():
    trk = tracker([GATE])
    got = drive(trk, [(70 + 6 * k, 100) for k in range(10)])                    # 70 .. 124: crosses between 94 and 100 -> 100 is on the line
    flat = [e for ev in got for e in ev]
    assert [e[:2] + e[5:] for e in flat] == [(1, 0, 1)] and flat[0][2:5] == (0, 0, 6)        # when it leaves the line, at x = 106
    assert trk.last_zone[3][0, :, 0].tolist() == [1, 0]
    got = drive(trk, [(124 - 6 * k, 100) for k in range(1, 10)])                # back: 118 .. 70, at x = 100 it is on the negative side
    flat = [e for ev in got for e in ev]
    assert [(e[0], e[1], e[5]) for e in flat] == [(1, 0, -1)] and flat[0][4] == 13
    assert trk.last_zone[3][0, :, 0].tolist() == [1, 1] and not trk.last_zone[3][0, :, 1:].any()
    assert np.array_equal(trk.zone_memo[0, 4:6], trk.last_zone[3][0])
    ev = None
    for c in [(70, 100), (76, 100)]:
        ev = step_rows(trk, [[T.make_row(box_at(*c), ids=(3, 1, 4, 1, 5, 9, 2, 6))]])
    assert int(ev[1][0]) == 0


def test_event_line_carries_anchor_key_and_hits():
    from yolov6.utils.watch_live import read_key
    trk = tracker([GATE])
    ids = (3, 1, 4, 1, 5, 9, 2, 6)
    zone = None
    for x in (91.5, 97.5, 103.5):
        zone = step_rows(trk, [[T.make_row(box_at(x, 100.25), ids=ids)]])
    assert int(zone[1][0]) == 1
    line = zone[0][0, 0]
    assert line[:6].tolist() == [1, 0, 0, 0, 2, 1] and line[6:8].view(f32).tolist() == [103.5, 100.25]
    assert tuple(line[8:10]) == read_key(ids) and line[10:].tolist() == [3, 0]


def test_min_hits_three_sees_nothing_before_and_no_crossing_on_first_sight():
    trk = tracker([GATE], [(SQUARE, 0)], min_hits=3)
    got = drive(trk, [(94, 100), (106, 100), (118, 100), (130, 100)])           # crosses at its second hit
    assert got == [[], [], [], []] and not trk.last_zone[3].any()
    assert trk.zone_memo[0, 0, 0] == 1                                          # known since the third hit
    got = drive(trk, [(118, 100), (106, 100), (94, 100)])
    assert [[e[:2] + e[5:] for e in ev] for ev in got] == [[], [], [(1, 0, -1)]]


def test_enter_dwell_exactly_once_and_left():
    trk = tracker(None, [(SQUARE, 4)])
    xs = [180, 190, 200, 210, 220, 230, 240, 250, 260, 270, 280, 290, 300, 310]
    got = drive(trk, [(x, 100) for x in xs])
    # x = 200 (frame 2) is inside; now - enter_frame reaches 4 in the call of frame 5; x = 300 (frame 12) is outside
    want = [[] for _ in xs]
    want[2], want[5], want[12] = [(2, 0, 0, 0, 2, 0)], [(4, 0, 0, 0, 5, 4)], [(3, 0, 0, 0, 12, 10)]
    assert got == want
    occ = tracker(None, [(SQUARE, 4)])
    assert [int(step_rows(occ, [[T.make_row(box_at(x, 100))]])[2][0, 0]) for x in xs] == [0, 0] + [1] * 10 + [0, 0]
    assert trk.zone_memo[0, 0, 4] == 0x100                                      # outside, the alerted bit stays until it enters again
    got = drive(trk, [(300 - 10 * k, 100) for k in range(1, 7)])
    assert got == [[(2, 0, 0, 0, 14, 0)], [], [], [(4, 0, 0, 0, 17, 4)], [], []]                # entered again: alerted again, once


def test_a_track_that_ends_inside_is_kind_5_with_the_memos_frame():
    trk = tracker(None, [(SQUARE, 0)])                                          # max_age 2: unseen for 3 frames
    got = drive(trk, [(190, 100), (210, 100), (220, 100), None, None, None, None])
    assert got == [[], [(2, 0, 0, 0, 1, 0)], [], [], [], [(5, 0, 0, 0, 2, 1)], []]
    line = trk.last_zone[0]
    assert not line.any() and not trk.zone_memo.any()


def test_a_missed_but_live_track_keeps_dwelling():
    trk = tracker(None, [(SQUARE, 3)], max_age=5)
    got = drive(trk, [(250, 100), None, None, None])
    assert got == [[(2, 0, 0, 0, 0, 0)], [], [(4, 0, 0, 0, 0, 3)], []]           # frame = the last matched frame, value = now - enter
    assert int(trk.last_zone[2][0, 0]) == 1                                     # it still occupies the zone


def test_a_slot_reused_in_one_call_ends_before_it_enters():
    far = [(500, 50), (600, 50), (600, 150), (500, 150)]
    trk = tracker(None, [(SQUARE, 0), (far, 0)], max_tracks=1, max_age=0)
    got = drive(trk, [(250, 100), (550, 100)])
    assert got == [[(2, 0, 0, 0, 0, 0)], [(5, 0, 0, 0, 0, 0), (2, 1, 1, 0, 1, 0)]]
    assert trk.last_zone[2][0].tolist() == [0, 1] + [0] * 6


def test_flush_reports_and_reset_is_silent():
    trk = tracker([GATE], [(SQUARE, 0)])
    drive(trk, [(250, 100), (256, 100)])
    zone = step_rows(trk, [], stream_of=[], flush=[1])
    assert events(zone) == [(5, 0, 0, 0, 1, 1)] and not trk.zone_memo.any()
    drive(trk, [(94, 100), (106, 100), (250, 100)][:2])
    assert trk.last_zone[3][0, 0, 0] == 1
    drive(trk, [(250, 100)])
    assert trk.zone_memo[0].any()
    trk.reset([0])
    assert not trk.zone_memo.any()                                              # the totals too
    zone = step_rows(trk, [[]])
    assert int(zone[1][0]) == 0 and not zone[3].any()


def test_two_frames_in_one_call_are_tested_on_the_chord():
    there_and_back = [[T.make_row(box_at(112, 100))], [T.make_row(box_at(94, 100))]]
    trk = tracker([GATE])
    drive(trk, [(94, 100)])
    assert int(step_rows(trk, there_and_back)[1][0]) == 0 and not trk.last_zone[3].any()
    assert int(trk.hits[0, 0]) == 3
    one = tracker([GATE])
    got = drive(one, [(94, 100), (112, 100), (94, 100)])                        # the same frames, one per call
    assert [[(e[0], e[5]) for e in ev] for ev in got] == [[], [(1, 1)], [(1, -1)]]


def test_a_stream_without_frames_is_still_processed():
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.zones import ZoneMapNp
    trk = PlateTrackerNp(2, max_tracks=4, max_age=2)
    trk.enable_zones(ZoneMapNp(2, None, [[], [(SQUARE, 0)]]))
    step_rows(trk, [[T.make_row(box_at(250, 100))]], stream_of=[1])
    for _ in range(3):
        zone = step_rows(trk, [[T.make_row(box_at(50, 50))]], stream_of=[0])
        assert zone[2][:, 0].tolist() == [0, 1] and zone[1].tolist() == [0, 0]
    zone = step_rows(trk, [], stream_of=[], flush=[0, 1])
    assert events(zone, 1) == [(5, 0, 0, 0, 0, 0)] and zone[1].tolist() == [0, 1] and zone[2][:, 0].tolist() == [0, 0]


@pytest.mark.parametrize('max_events', [0, 1, 3, 7])
def test_max_events_caps_the_lines_not_the_count(max_events):
    """Three tracks enter one zone with min_dwell 1 in one call: six events... no, three -- and three dwell alerts with them."""
    rows = [T.make_row(box_at(220 + 25 * k, 60 + 30 * k)) for k in range(3)]
    full = step_rows(tracker(None, [(SQUARE, 1)], max_events=6), [rows])
    assert int(full[1][0]) == 6 and [e[0] for e in events(full)] == [2, 4] * 3
    zone = step_rows(tracker(None, [(SQUARE, 1)], max_events=max_events), [rows])
    assert zone[0].shape == (1, max_events, 12) and int(zone[1][0]) == 6
    n = min(max_events, 6)
    assert np.array_equal(zone[0][0, :n], full[0][0, :n]) and not zone[0][0, n:].any()
    assert np.array_equal(zone[2], full[2]) and zone[2][0, 0] == 3


def test_enabling_zones_changes_nothing_else():
    """Hold, watch, live watch and sightings on both trackers, zones on one: every return, every other ``last_*`` and the state agree."""
    from yolov6.utils.sight import SightLogNp
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.watch import WatchlistNp
    from yolov6.utils.zones import ZoneMapNp
    calls = T.random_track_case(7, n_streams=3, max_det=20, n_calls=10)
    kw = dict(max_tracks=8, match_thres=0.3, new_thres=0.2, expand=0.5, max_age=2)
    entries = np.random.default_rng(0).integers(0, 24, (40, 8)).astype(np.uint8)
    trks = []
    for on in (False, True):
        t = PlateTrackerNp(3, **kw)
        t.enable_hold(min_hits=2)
        t.enable_watch(WatchlistNp(entries), max_mismatch=2)
        t.enable_live_watch(WatchlistNp(entries), min_hits=2, max_mismatch=2)
        t.enable_sightings(SightLogNp(64, 3), window=100)
        if on:
            rng = np.random.default_rng(1)
            t.enable_zones(ZoneMapNp(3, [[tuple(rng.integers(0, 600, 4)) for _ in range(6)]] * 3,
                                     [[(star_polygon(rng, 8, 300, 300, 100, 280), 2)]] * 3))
        trks.append(t)
    off, on = trks
    n_ev = 0
    for det, count, stream_of, flush in calls:
        a, b = off.update(det, count, stream_of, flush, 5), on.update(det, count, stream_of, flush, 5)
        for x, y in zip(a + off.last_hold + (off.last_watch, off.last_live, off.last_sight) + off.last_live_reads,
                        b + on.last_hold + (on.last_watch, on.last_live, on.last_sight) + on.last_live_reads):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.int32), y.view(np.int32))
        for name in PlateTrackerNp._SLOT_ARRAYS + ('frame', 'next_id', 'dropped'):
            x, y = getattr(off, name), getattr(on, name)
            assert np.array_equal(x.view(np.int32), y.view(np.int32)), name
        assert np.array_equal(off._sight[0].state, on._sight[0].state) and np.array_equal(off._live.memo, on._live.memo)
        n_ev += int(on.last_zone[1].sum())
    assert n_ev > 0 and off.last_zone is None and off.zone_memo is None
    on.enable_zones(None)
    on.update(*calls[0][:3])
    assert on.last_zone is None and on.zone_memo is None


# ---- the parser and the validation -------------------------------------------------------------------------------------------------
def test_parse_zones_round_trip(tmp_path):
    from yolov6.utils.zones import ZoneMapNp, format_zones, parse_zones
    text = """# a gate with two lanes
    line in 100 200 100 0
    line out 400.5 0 400.5 200   # the other lane
    zone bay dwell=250 200 50 300 50 300 150 200 150
    1: zone kerb 0 0 10 0.25 5 10
    1: line far 1 2 3 4
    """
    lines, zones, line_names, zone_names = parse_zones(text, 2)
    assert line_names == [['in', 'out'], ['far']] and zone_names == [['bay'], ['kerb']]
    assert lines[0] == [(100, 200, 100, 0), (400.5, 0, 400.5, 200)] and zones[0][0][1] == 250 and zones[1][0][1] == 0
    m = ZoneMapNp(2, lines, zones)
    assert m.packed[0, :2].tolist() == [2, 1] and m.packed[1, :2].tolist() == [1, 1] and m.packed[1, 80:82].tolist() == [3, 0]
    path = tmp_path / 'zones.txt'
    path.write_text(format_zones(m, line_names, zone_names))
    again = parse_zones(str(path), 2)
    assert again[2:] == (line_names, zone_names) and np.array_equal(ZoneMapNp(2, again[0], again[1]).packed, m.packed)
    for bad in ('line a 1 2 3', 'zone z 0 0 1 1', 'zone z dwell=x 0 0 1 1 2 2', 'circle c 1 2 3', '2: line a 1 2 3 4', 'line a 1 2 3 q'):
        with pytest.raises(ValueError):
            parse_zones(bad + '\n', 2)


def test_zone_map_validation():
    from yolov6.utils.zones import MAP_WORDS, ZoneMapNp, check_packed
    tri = [(0, 0), (10, 0), (5, 10)]
    poly = lambda n: [(np.cos(a) * 50 + 60, np.sin(a) * 50 + 60) for a in np.linspace(0, 2 * np.pi, n, endpoint=False)]   # noqa: E731
    ok = ZoneMapNp(1, [[(0, 0, 1, 1)] * 16], [[(poly(16), 0)] * 7 + [tri]])
    assert ok.packed.shape == (1, MAP_WORDS) and ok.packed[0, :2].tolist() == [16, 8] and ok.packed[0, 80 + 28:80 + 30].tolist() == [3, 0]
    for lines, zones in (([[(0, 0, 1, 1)] * 17], None), (None, [[tri] * 9]), (None, [[tri[:2]]]), (None, [[(poly(17), 0)]]),
                         ([[(0, 0, NAN, 1)]], None), ([[(0, 0, INF, 1)]], None), ([[(0, 0, 1e39, 1)]], None),
                         (None, [[([(0, 0), (10, NAN), (5, 10)], 0)]]), (None, [[(tri, -1)]]), (None, [[(tri, 1.5)]]), ([[], []], None)):
        with pytest.raises(ValueError):
            ZoneMapNp(1, lines, zones)
    for word, value in ((0, 17), (1, -1), (5, 1), (80, 2), (81, -1), (82, 7), (112 + 7, 1)):
        p = ZoneMapNp(1, None, [[tri]]).packed.copy()
        p[0, word] = value
        with pytest.raises(ValueError):
            check_packed(p)
    from yolov6.utils.track import PlateTrackerNp
    with pytest.raises(ValueError):
        PlateTrackerNp(2).enable_zones(ok)                                      # a map of another number of streams
    with pytest.raises(ValueError):
        PlateTrackerNp(1).enable_zones(ok, min_hits=0)
    with pytest.raises(ValueError):
        PlateTrackerNp(1).enable_zones(ok, max_events=-1)


# ---- what tests/test_zones_gpu.py shares -----------------------------------------------------------------------------------------------
EXTENT = (1800, 720)


def zone_geometry(seed, L, Z, n_streams=3, step=8.0):
    """(lines, zones) per stream for ``ZoneMapNp``: ``L`` lines (every other one parallel to an axis) and ``Z`` zones (3 and 16 vertices alternating, min_dwell 0..3) over
    the extent of ``zone_calls``, coordinates on the grid of ``step``; every stream gets its own."""
    rng = np.random.default_rng(1000 + seed)
    lines, zones = [], []
    for _ in range(n_streams):
        ls = []
        for _ in range(L):
            x, y = rng.integers(0, EXTENT[0] / step), rng.integers(0, EXTENT[1] / step)
            dx, dy = rng.integers(-40, 41), rng.integers(-40, 41)
            if len(ls) % 2 == 0:                                                # every other line is parallel to an axis
                dx, dy = (0, dy) if len(ls) % 4 == 0 else (dx, 0)
            ls.append((x * step, y * step, (x + dx) * step, (y + dy + (dx == 0 and dy == 0)) * step))
        zs = [(star_polygon(rng, 3 if z % 2 == 0 else 16, rng.integers(200, EXTENT[0] - 200), rng.integers(150, EXTENT[1] - 150), 80, 320, step),
               int(rng.integers(0, 4))) for z in range(Z)]
        lines.append(ls)
        zones.append(zs)
    return lines, zones


def zone_calls(seed, max_tracks, n_calls=12, mode='grid'):
    """``n_calls`` update calls on three streams: stream 0 has one frame a call, stream 1 two, stream 2 none ever; stream 1 is flushed
    half way.  About ``max_tracks`` objects a stream on a lattice of 150 x 60 px cells, drifting; born, dying and missed.  ``mode``
    'grid': positions and velocities are multiples of 4 px with boxes of even size, so that anchors fall on lines and vertices of a
    geometry on the 8 px grid; 'float': arbitrary fp32 positions; 'nan': grid, with NaN and infinite box coordinates thrown in."""
    rng = np.random.default_rng(seed)
    n_obj = min(max_tracks + 2, 130)
    max_det = min(max_tracks + 2, 128)
    objs = [[], []]

    def rows_of(s):
        live = objs[s]
        live[:] = [o for o in live if rng.random() > 0.04]
        for _ in range(n_obj - len(live)):
            if live and rng.random() < 0.5:
                continue
            k = int(rng.integers(0, 144))
            o = dict(x=float((k % 12) * 150 + 4 * rng.integers(0, 16)), y=float((k // 12) * 60 + 4 * rng.integers(0, 4)),
                     vx=float(4 * rng.integers(-3, 4)), vy=float(4 * rng.integers(-1, 2)))
            if mode == 'float':
                o = {k_: f32(v + rng.uniform(-1, 1)) for k_, v in o.items()}
            live.append(o)
        rows = []
        for o in live:
            o['x'], o['y'] = f32(o['x'] + o['vx']), f32(o['y'] + o['vy'])
            if rng.random() < 0.12:
                continue
            box = [o['x'], o['y'], f32(o['x'] + (80 if mode != 'float' else 80.3)), f32(o['y'] + (24 if mode != 'float' else 24.7))]
            if mode == 'nan' and rng.random() < 0.08:
                box[int(rng.integers(0, 4))] = (NAN, INF, -INF)[int(rng.integers(0, 3))]
            rows.append(T.make_row(tuple(box), rng.integers(0, 24, 8), (rng.integers(1, 9, 8) / 8.0).astype(f32)))
        order = rng.permutation(len(rows))[:max_det]
        return [rows[i] for i in order]

    calls = []
    for c in range(n_calls):
        stream_of = [1, 0, 1]
        det, count = T.frames_of([rows_of(s) for s in stream_of], max_det)
        calls.append((det, count, stream_of, [0, int(c == n_calls // 2), 0]))
    return calls


def outputs_np(trk):
    return tuple(trk.last_zone) + (trk.zone_memo,)


def assert_same(got, want, what):
    names = ('zone_ev', 'zone_count', 'zone_occ', 'zone_totals', 'memo')
    for name, g, w in zip(names, got, want):
        assert g.shape == w.shape and g.dtype == np.int32 and w.dtype == np.int32, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[0]
            raise AssertionError('%s: %s differs at %s: got %d, want %d (%d words differ)' % (what, name, tuple(bad), g[tuple(bad)], w[tuple(bad)],
                                                                                          int((g != w).sum())))


def kinds_seen(zone_ev, zone_count, seen):
    for s in range(zone_ev.shape[0]):
        for k in range(min(int(zone_count[s]), zone_ev.shape[1])):
            seen[int(zone_ev[s, k, 0])] = seen.get(int(zone_ev[s, k, 0]), 0) + 1
    return seen


@pytest.mark.parametrize('mode', ['grid', 'float', 'nan'])
def test_the_shared_scene_reaches_every_kind(mode):
    """The scene of the GPU tests on the CPU: every kind of event occurs, anchors fall exactly on lines (grid), the never-fed stream
    stays empty, and the run is deterministic."""
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.zones import ZoneMapNp, anchor_of, cross
    kw = dict(max_tracks=64, match_thres=0.3, new_thres=0.2, expand=0.25, max_age=2)
    lines, zones = zone_geometry(3, 16, 8)
    runs = []
    for _ in range(2):
        trk = PlateTrackerNp(3, **kw)
        trk.enable_zones(ZoneMapNp(3, lines, zones))
        seen, on_line, out = {}, 0, []
        for det, count, stream_of, flush in zone_calls(5, 64, mode=mode):
            trk.update(det, count, stream_of, flush)
            kinds_seen(trk.last_zone[0], trk.last_zone[1], seen)
            out.append([a.copy() for a in outputs_np(trk)])
            for s in range(2):
                for t in np.nonzero(trk.hits[s] > 0)[0]:
                    ax, ay = anchor_of(trk.box[s, t])
                    on_line += int((cross(*np.asarray(lines[s], f64).T, ax, ay) == 0).sum())
            assert not trk.zone_memo[2].any() and not trk.last_zone[0][2].any()
        runs.append(out)
        assert all(seen.get(k, 0) > 0 for k in (1, 2, 3, 4, 5)), seen
        assert mode != 'grid' or on_line > 10
    for a, b in zip(*runs):
        assert_same(a, b, 'second run')


# ---- tools/infer.py --track --zones on the CPU path ---------------------------------------------------------------------------------
ZONES_TXT = """# a 160 x 128 picture: three gate lines and its two halves
line left 40 128 40 0
line mid 80 128 80 0
line right 120 0 120 128
zone west dwell=2 0 0 80 0 80 128 0 128
zone east dwell=3 80 0 160 0 160 128 80 128
zone middle 40 20 120 20 120 100 80 110 40 100
"""


def expected_zone_files(dets, max_det, text, min_hits, **kw):
    """(crossings.txt, zones.txt) lines by hand: ``PlateTrackerNp`` with zones over the untracked per-frame detections of one stream,
    one update per frame, then the flush."""
    from yolov6.utils.track import PlateTrackerNp, plate_text
    from yolov6.utils.zones import ZoneMapNp, parse_zones
    lines, polys, line_names, zone_names = parse_zones(text, 1)
    trk = PlateTrackerNp(1, **kw)
    trk.enable_zones(ZoneMapNp(1, lines, polys), min_hits)
    cross_lines, zone_lines = [], []

    def collect(ended_i, ended_count):
        ev, count = trk.last_zone[:2]
        assert count[0] <= ev.shape[1]
        for e in ev[0, :count[0]]:
            kind, index, tid, _, frame, value = e[:6].tolist()
            if kind == 5:
                reads = [ended_i[0, k, 4:12] for k in range(int(ended_count[0])) if ended_i[0, k, 0] == tid]
                text_ = plate_text(reads[0]) if reads else '-'
            else:
                text_ = plate_text(np.array([e[8], e[9]], np.int32).view(np.uint8))
            if kind == 1:
                cross_lines.append('%d %d %s %s %+d' % (frame, tid, text_, line_names[0][index], value))
            else:
                zone_lines.append('%d %d %s %s %s %d' % (frame, tid, text_, zone_names[0][index], {2: 'enter', 3: 'left', 4: 'dwell', 5: 'ended'}[kind], value))
    for d in dets:
        pad = np.zeros((1, max_det, 28), f32)
        pad[0, :len(d)] = d
        _, _, ei, _, ec = trk.update(pad, [len(d)], max_ended=2 * trk.max_tracks)
        collect(ei, ec)
    _, _, ei, _, ec = trk.flush_all()
    collect(ei, ec)
    return cross_lines, zone_lines, trk.last_zone[3]


def infer_zones_case(tmp_path, monkeypatch, device, n_frames=8, **extra):
    """tools/infer.py with and without --zones on drifting frames: (module, keywords, untracked detections, tracker keywords)."""
    import importlib
    import os
    import sys

    import torch
    from PIL import Image
    from conftest import REPO
    from yolov6.utils.synth import build_synthetic
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    m = build_synthetic(os.path.join(REPO, 'configs', 'yololps.py'), width=0.0625, sigma=1.5)
    ckpt = tmp_path / 'tiny.pt'
    torch.save({'model': m.half(), 'ema': None, 'epoch': 0}, str(ckpt))
    (tmp_path / 'imgs').mkdir()
    for k, f in enumerate(T._moving_frames(n_frames)):
        Image.fromarray(f).save(str(tmp_path / 'imgs' / ('f%02d.png' % k)))
    (tmp_path / 'zones.txt').write_text(ZONES_TXT)
    kw = dict(weights=str(ckpt), source=str(tmp_path / 'imgs'), yaml=None, img_size=[128, 160], conf_thres=0.06, iou_thres=0.45, max_det=20,
              device=device, not_save_img=True, save_txt=True, track_max_age=2, track_iou=0.25, track_expand=0.25, **extra)
    untracked = [d.cpu().numpy() for d in infer.run(save_dir=str(tmp_path / 'o0'), **kw)]
    return infer, kw, untracked, dict(max_tracks=64, match_thres=0.25, new_thres=0.0, expand=0.25, max_age=2, ncls=m)


def check_infer_zones(tmp_path, infer, kw, untracked, tkw):
    import torch
    plain = infer.run(save_dir=str(tmp_path / 'o1'), track=True, **kw)
    assert not (tmp_path / 'o1' / 'crossings.txt').exists() and not (tmp_path / 'o1' / 'zones.txt').exists()
    n = 0
    for sub, min_hits in (('o2', 1), ('o3', 2)):
        again = infer.run(save_dir=str(tmp_path / sub), track=True, zones=str(tmp_path / 'zones.txt'), zones_min_hits=min_hits, **kw)
        for a, b in zip(plain, again):
            assert torch.equal(a, b)
        for name in ('tracks.txt', 'plates.txt'):                                # byte-identical to the run without the switch
            assert (tmp_path / sub / name).read_bytes() == (tmp_path / 'o1' / name).read_bytes()
        want_c, want_z, _ = expected_zone_files(untracked, 20, ZONES_TXT, min_hits, **tkw)
        assert (tmp_path / sub / 'crossings.txt').read_text().splitlines() == want_c, sub
        assert (tmp_path / sub / 'zones.txt').read_text().splitlines() == want_z, sub
        n += len(want_c) + len(want_z)
        assert {ln.split()[-2] for ln in want_z} >= {'enter', 'ended'}, want_z
    assert n > 4
    with pytest.raises(ValueError, match='track'):
        infer.run(save_dir=str(tmp_path / 'o4'), zones=str(tmp_path / 'zones.txt'), **kw)


def test_infer_zones_cpu(tmp_path, monkeypatch):
    check_infer_zones(tmp_path, *infer_zones_case(tmp_path, monkeypatch, 'cpu'))
