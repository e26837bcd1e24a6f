"""Speed of live plate tracks on a calibrated plane, on the CPU: the arithmetic of yolov6/utils/speed.py against exact rational
arithmetic (the world point op by op, rint ties, the validity edges, the exact integer root on the family where a float root is wrong),
a run on which a fused multiply-add gives other millimetres, the edges of the rule through PlateTrackerNp.enable_speed (ring, gap, span,
confirm, slot reuse, two frames in one call, the clock, a disabled stream, max_events, reset / flush / re-enable), an accuracy
scenario with a pinhole camera, and the host helpers.  The scene generators and comparison helpers of tests/test_speed_gpu.py live
here as well."""
import math
from fractions import Fraction

import numpy as np
import pytest

import test_track_cpu as T
import test_zones_cpu as Z

f32, f64 = np.float32, np.float64
NAN, INF = float('nan'), float('inf')
EIGHTH = (0.125, 0, 0, 0, 0.125, 0, 0, 0, 1)            # 1 px = 125 mm, exactly
PERIOD = 40000


def plane(H=EIGHTH, **kw):
    return dict(dict(H=H, period_us=PERIOD, min_span_us=1), **kw)


# ---- a tracker state written by hand ------------------------------------------------------------------------------------------------
class HandState:
    """What ``SpeedNp.step`` reads of a tracker, set by hand: ``put`` places a live track whose anchor is exactly (cx, cy) (a box of
    no extent).  ``packed()`` is the same state in the layout of lp_track_update (16 header words, 544 per slot)."""

    def __init__(self, n_streams, max_tracks):
        from yolov6.utils.track import DEFAULT_NCLS, HEADS, MAX_CLS
        S, Tn = n_streams, max_tracks
        self.n_streams, self.max_tracks, self.ncls = S, Tn, DEFAULT_NCLS
        self.frame = np.zeros(S, np.int32)
        self.id, self.first, self.last, self.hits, self.misses = (np.zeros((S, Tn), np.int32) for _ in range(5))
        self.box = np.zeros((S, Tn, 4), f32)
        self.votes, self.total = np.zeros((S, Tn, HEADS, MAX_CLS), f32), np.zeros((S, Tn, HEADS), f32)

    def read(self, s, t):
        from yolov6.utils.track import PlateTrackerNp
        return PlateTrackerNp.read(self, s, t)

    def put(self, s, t, tid, last, hits, cx, cy, ids=(1, 2, 3, 4, 5, 6, 7, 8)):
        self.id[s, t], self.last[s, t], self.hits[s, t] = tid, last, hits
        self.box[s, t] = (cx, cy, cx, cy)
        self.votes[s, t], self.total[s, t] = 0, 1
        for p, c in enumerate(ids):
            self.votes[s, t, p, c] = 1

    def clear(self, s, t):
        for a in (self.id, self.first, self.last, self.hits, self.misses, self.box, self.votes, self.total):
            a[s, t] = 0

    def packed(self):
        S, Tn = self.n_streams, self.max_tracks
        st = np.zeros((S, 16 + Tn * 544), np.int32)
        st[:, 0] = self.frame
        sl = st[:, 16:].reshape(S, Tn, 544)
        for k, a in enumerate((self.id, self.first, self.last, self.hits, self.misses)):
            sl[:, :, k] = a
        sl[:, :, 8:12] = self.box.view(np.int32)
        sl[:, :, 24:32] = self.total.view(np.int32)
        sl[:, :, 32:] = self.votes.reshape(S, Tn, 512).view(np.int32)
        return st.reshape(-1)


def hand_run(planes, steps, max_tracks=2, **kw):
    """(state, spec, outputs per step): ``steps`` = per call (frame counter, clock or None, [(slot, id, last, hits, cx, cy) or (slot,)
    to clear]) on stream 0; the outputs are (speed_i, speed_ev, speed_count, memo) copies.  ``spec.feeds`` keeps what every call saw:
    (the packed state, the clock or None), for the GPU tests."""
    from yolov6.utils.speed import GroundPlaneNp, SpeedNp
    st = HandState(len(planes), max_tracks)
    spec = SpeedNp(GroundPlaneNp(len(planes), planes), max_tracks, **kw)
    outs, spec.feeds = [], []
    for now, clk, slots in steps:
        st.frame[0] = now
        for sl in slots:
            st.clear(0, sl[0]) if len(sl) == 1 else st.put(0, *sl)
        clk = None if clk is None else np.array([clk] * len(planes), np.int64)
        spec.feeds.append((st.packed(), clk))
        outs.append(tuple(a.copy() for a in spec.step(st, clk) + (spec.memo,)))
    return st, spec, outs


def one_track(planes, points, times=None, **kw):
    """A track of id 7 in slot 0 seen at ``points`` (anchors), one call each, frame k (and clock ``times[k]``)."""
    steps = [(k + 1, None if times is None else times[k], [(0, 7, k, k + 1, cx, cy)]) for k, (cx, cy) in enumerate(points)]
    return hand_run(planes, steps, **kw)


# ---- exact arithmetic -------------------------------------------------------------------------------------------------------------------
def frac_rint(q):
    """Round a Fraction to the nearest integer, ties to even."""
    n = math.floor(q)
    r = q - n
    return n + (1 if r > Fraction(1, 2) or (r == Fraction(1, 2) and n % 2) else 0)


def rnd(q):
    """A Fraction rounded to the nearest fp64 (Fraction -> float is correctly rounded)."""
    return float(q)


def frac_world(H, ax, ay, fused=False):
    """(valid, X_mm, Y_mm) with every fp64 operation emulated: the exact result in rational arithmetic, rounded once.  ``fused``: the
    variant that contracts h0 * x + h1 * y into fma(h0, x, h1 * y) (and the two other rows likewise)."""
    F = Fraction
    x, y = F(float(f32(ax))), F(float(f32(ay)))
    h = [F(float(v)) for v in H]

    def row(a, b, c):
        t1 = rnd(b * y)
        s = rnd(a * x + F(t1)) if fused else rnd(F(rnd(a * x)) + F(t1))
        return rnd(F(s) + c)
    u, v, w = row(*h[0:3]), row(*h[3:6]), row(*h[6:9])
    if not w > 0:
        return False, 0, 0
    px, py = rnd(F(rnd(F(u) / F(w))) * 1000), rnd(F(rnd(F(v) / F(w))) * 1000)
    if not (abs(px) <= 2 ** 30 and abs(py) <= 2 ** 30):
        return False, 0, 0
    return True, frac_rint(F(px)), frac_rint(F(py))


def test_world_point_equals_rational_arithmetic_on_grid_data_and_off_it():
    """Grid data: small-integer H and anchors with w a power of two, so that every fp64 operation is exact and the result is the
    rational one; then arbitrary data against the op-by-op emulation."""
    from yolov6.utils.speed import world_point
    rng = np.random.default_rng(1)
    ties = invalid = 0
    for k in range(400):
        x, y = int(rng.integers(-64, 65)), int(rng.integers(-64, 65))
        H = [int(v) for v in rng.integers(-8, 9, 9)]
        H[6], H[7] = int(rng.integers(-2, 3)), int(rng.integers(-2, 3))
        want_w = (0, -4, 1, 2, 4, 8, 16, 32, 64)[k % 9]
        H[8] = want_w - (H[6] * x + H[7] * y)
        u, v = H[0] * x + H[1] * y + H[2], H[3] * x + H[4] * y + H[5]
        valid, xm, ym = world_point(H, f32(x), f32(y))
        assert bool(valid) == (want_w > 0)
        invalid += not valid
        if valid:
            px, py = Fraction(u, want_w) * 1000, Fraction(v, want_w) * 1000
            assert (int(xm), int(ym)) == (frac_rint(px), frac_rint(py)), (H, x, y)
            ties += (px % 1 == Fraction(1, 2)) + (py % 1 == Fraction(1, 2))
        assert (bool(valid), int(xm), int(ym)) == frac_world(H, x, y)
    assert ties >= 10 and invalid >= 50
    for _ in range(300):
        H = rng.uniform(-1, 1, 9) * (0.05, 0.05, 20, 0.05, 0.05, 20, 1e-4, 1e-3, 1)
        ax, ay = f32(rng.uniform(0, 1920)), f32(rng.uniform(0, 1080))
        valid, xm, ym = world_point(H, ax, ay)
        assert (bool(valid), int(xm), int(ym)) == frac_world(H, ax, ay)


def test_rint_ties_go_to_even():
    from yolov6.utils.speed import world_point
    for num, want in ((1, 62), (3, 188), (5, 312), (-1, -62), (-3, -188), (8, 500)):       # num / 16 m = num * 62.5 mm
        valid, xm, ym = world_point((1, 0, 0, 0, -1, 0, 0, 0, 16), f32(num), f32(num))
        assert valid and (int(xm), int(ym)) == (want, -want)


def test_validity_edges():
    from yolov6.utils.speed import world_point
    wp = lambda H, x=100.0, y=50.0: tuple(int(v) for v in world_point(H, f32(x), f32(y)))       # noqa: E731
    assert wp((1, 0, 0, 0, 1, 0, 0, 0, 1)) == (1, 100000, 50000)
    assert wp((1, 0, 0, 0, 1, 0, 0, 0.02, -1)) == (0, 0, 0)                       # w = 0.02 * 50 - 1 = 0
    assert wp((1, 0, 0, 0, 1, 0, 0, 0, -1)) == (0, 0, 0)                          # w < 0
    assert wp((1, 0, 0, 0, 1, 0, 1e308, -1e308, 1), 100.0, 100.0) == (0, 0, 0)    # w = inf - inf: NaN, with a finite H
    assert wp((1e308, 1e308, 0, 0, 1, 0, 0, 0, 1)) == (0, 0, 0)                   # u infinite
    # |X * 1000| exactly 2^30 and the next fp64 above: X goes in through h2, w = 1
    x0 = float(2 ** 30) / 1000.0
    while x0 * 1000.0 > 2.0 ** 30:
        x0 = np.nextafter(x0, 0.0)
    while np.nextafter(x0, INF) * 1000.0 <= 2.0 ** 30:
        x0 = np.nextafter(x0, INF)
    x1 = float(np.nextafter(x0, INF))
    assert x0 * 1000.0 == 2.0 ** 30 and x1 * 1000.0 > 2.0 ** 30
    assert wp((0, 0, x0, 0, 0, -x0, 0, 0, 1)) == (1, 2 ** 30, -2 ** 30)
    assert wp((0, 0, x1, 0, 0, 0, 0, 0, 1)) == (0, 0, 0) and wp((0, 0, 0, 0, 0, -x1, 0, 0, 1)) == (0, 0, 0)
    for bad in (NAN, INF, -INF):                                                 # a NaN or infinite box: no sample, no estimate
        _, _, outs = hand_run([plane()], [(1, None, [(0, 7, 0, 1, 10.0, 10.0)]), (2, None, [(0, 7, 1, 2, bad, 10.0)]),
                                           (3, None, [(0, 7, 2, 3, 12.0, bad)]), (4, None, [(0, 7, 3, 4, 18.0, 10.0)])])
        rows = [tuple(o[0][0, 0]) for o in outs]
        assert [r[7] for r in rows] == [1 | 256, 1, 1, 2 | 256] and [r[1] for r in rows] == [-1, -1, -1, 1000 * 1000000 // (3 * PERIOD)]
        assert outs[2][3][0, 0, 1] == 2                                          # memo.last follows the detection all the same


# ---- the estimator and the exact integer root -------------------------------------------------------------------------------------------
def test_estimator_equals_rational_arithmetic():
    from yolov6.utils.speed import I32_MAX, estimate
    rng = np.random.default_rng(2)
    for k in range(500):
        hi = (10, 5000, 2 ** 31)[k % 3]
        dx, dy = int(rng.integers(-hi, hi + 1)), int(rng.integers(-hi, hi + 1))
        dt = int(rng.choice([1, 7, 1000, 40000, 280000, 10 ** 6, 333333, 2 ** 40 + 1]))
        speed, vx, vy, span = estimate(dx, dy, dt)
        d2 = dx * dx + dy * dy
        s = (speed * dt) // 10 ** 6 if speed < I32_MAX else None
        root = math.isqrt(d2)
        assert root * root <= d2 < (root + 1) ** 2
        assert speed == min(math.floor(Fraction(root * 10 ** 6, dt)), I32_MAX) and (s is None or s <= root)
        for v, d in ((vx, dx), (vy, dy)):
            assert v == (1 if d >= 0 else -1) * min(math.floor(Fraction(abs(d) * 10 ** 6, dt)), I32_MAX)
        assert span == min(dt // 1000, I32_MAX)
    assert estimate(3, 4, 10 ** 6) == (5, 3, 4, 1000) and estimate(-3, 4, 3 * 10 ** 6) == (1, -1, 1, 3000)
    with pytest.raises(ValueError):
        estimate(1, 1, 0)


def root_family_cases():
    """(name, plane, two anchors, dt in frames of 1 s, dx, dy): sample differences of which the root is just below an integer --
    dx = 2 k, dy = 2 k^2, d2 = (2 k^2 + 1)^2 - 1 -- with k = j * 8, j^2 < 2^24, so that the fp32 anchors (-+j, -+j^2) and the per-axis
    scales 0.008 and 0.064 m / px give exactly -+k and -+k^2 mm; the Pythagorean (3 n, 4 n) with dy near 2^31; and d2 = 0, 1, 2, 4, 5 (3
    is not a sum of two squares)."""
    out = []
    for k in (7000, 32760):
        j = k // 8
        assert j * 8 == k and j * j < 2 ** 24
        out.append(('k%d' % k, plane((0.008, 0, 0, 0, 0.064, 0, 0, 0, 1), period_us=10 ** 6), ((-j, -j * j), (j, j * j)), 1, 2 * k, 2 * k * k))
    n = 536870500                                                               # 4 n = 2147482000: 2 n mm = 1073741 m exactly
    out.append(('pyth', plane((0.25, 0, 0, 0, 1, 0, 0, 0, 1), period_us=10 ** 6), ((-3221223, -1073741), (3221223, 1073741)), 2, 3 * n, 4 * n))
    for dx, dy in ((0, 0), (1, 0), (1, 1), (2, 0), (1, 2)):
        out.append(('d2_%d' % (dx * dx + dy * dy), plane((0.001, 0, 0, 0, 0.001, 0, 0, 0, 1), period_us=10 ** 6), ((5, 5), (5 + dx, 5 + dy)), 1, dx, dy))
    return out


def root_family_steps(a, b, frames):
    return [(1, None, [(0, 7, 0, 1, float(a[0]), float(a[1]))]), (1 + frames, None, [(0, 7, frames, 2, float(b[0]), float(b[1]))])]


@pytest.mark.parametrize('case', root_family_cases(), ids=lambda c: c[0])
def test_integer_root_is_exact_where_a_float_root_is_not(case):
    name, pl, (a, b), frames, dx, dy = case
    _, _, outs = hand_run([pl], root_family_steps(a, b, frames))
    row, memo = outs[1][0][0, 0], outs[1][3][0, 0]
    assert (int(memo[22]) - int(memo[18]), int(memo[23]) - int(memo[19])) == (dx, dy)          # both differences are exact
    d2 = dx * dx + dy * dy
    s = math.isqrt(d2)
    assert row[1] == s * 10 ** 6 // (frames * 10 ** 6) and row[2] == dx // frames and row[3] == dy // frames
    if name.startswith('k'):
        k = dx // 2
        assert s == 2 * k * k and int(math.sqrt(float(d2))) == s + 1                          # the float root is one too large
        assert name != 'k7000' or (int(math.sqrt(float(d2))), s) == (98000001, 98000000)


# ---- the fused multiply-add trap --------------------------------------------------------------------------------------------------------
FMA_H = (0.1, -0.1, 0.0, 0.07, -0.07, 0.0, 0.0, 0.0, 1e-12)


def fma_trap_points(n=12):
    """Anchors (x, x) on the diagonal, where h0 * x + h1 * y is round(p) - round(p) = 0 op by op, while a fused multiply-add leaves
    the rounding error of the product there; w = 1e-12 (a point far beyond the calibrated patch) brings it up to metres.  Found by
    search: the anchors on which the fused variant is valid and gives other millimetres."""
    rng = np.random.default_rng(5)
    pts = []
    while len(pts) < n:
        x = float(f32(rng.uniform(100, 1800)))
        a, b = frac_world(FMA_H, x, x), frac_world(FMA_H, x, x, fused=True)
        if a[0] and b[0] and a != b:
            pts.append((x, x))
    return pts


def test_a_fused_multiply_add_gives_other_millimetres():
    from yolov6.utils.speed import world_point
    pts = fma_trap_points()
    for x, y in pts:                                                            # first of all: the two variants differ on this run
        spec, fused = frac_world(FMA_H, x, y), frac_world(FMA_H, x, y, fused=True)
        assert spec[0] and fused[0] and spec != fused and spec[1:] == (0, 0)
    for x, y in pts:
        assert tuple(int(v) for v in world_point(FMA_H, f32(x), f32(y))) == (1, 0, 0)
    _, _, outs = one_track([plane(FMA_H)], pts)
    assert [tuple(o[0][0, 0, 1:7]) for o in outs[1:]] == [(0, 0, 0, 0, 0, PERIOD * min(k, 7) // 1000) for k in range(1, len(pts))]


# ---- the rule's edges through PlateTrackerNp --------------------------------------------------------------------------------------------
def tracker(planes, min_hits=1, confirm=2, max_events=None, clock=None, **kw):
    from yolov6.utils.speed import GroundPlaneNp
    from yolov6.utils.track import PlateTrackerNp
    trk = PlateTrackerNp(len(planes), **dict(dict(max_tracks=4, max_age=2), **kw))
    trk.enable_speed(GroundPlaneNp(len(planes), planes), min_hits, confirm, max_events, clock)
    return trk


def step_rows(trk, rows_per_frame, stream_of=None, flush=None, max_det=4, clock=None):
    det, count = T.frames_of(rows_per_frame, max_det)
    if clock is not None:
        trk.speed_clock[:] = clock
    trk.update(det, count, stream_of=[0] * len(rows_per_frame) if stream_of is None else stream_of, flush=flush)
    return trk.last_speed


def drive(trk, centres, clocks=None, **kw):
    """One call per centre (None: a frame without rows) on stream 0: the (row of slot 0, events) of every call."""
    out = []
    for k, c in enumerate(centres):
        sp = step_rows(trk, [[] if c is None else [T.make_row(Z.box_at(*c))]], clock=None if clocks is None else clocks[k], **kw)
        out.append((tuple(int(v) for v in sp[0][0, 0]), events(sp)))
    return out


def events(sp, s=0):
    return [tuple(int(v) for v in sp[1][s, k]) for k in range(min(int(sp[2][s]), sp[1].shape[1]))]


def line_of(x0, step, n, y=100):
    return [(x0 + step * k, y) for k in range(n)]


@pytest.mark.parametrize('n', [1, 2, 8, 9, 17])
def test_ring_of_eight_samples_wraps(n):
    """A track with exactly n pushed samples, 8 px = 1000 mm a frame: the estimate spans min(n, 8) samples, the flush reports peak and
    chord iff n >= 2."""
    trk = tracker([plane()], max_age=0)
    out = drive(trk, line_of(40, 8, n))
    for k, (row, ev) in enumerate(out):
        m = min(k, 7)
        assert ev == [] and row[0] == 0 and row[7] == min(k + 1, 8) | 256
        assert row[1:4] == ((25000, 25000, 0) if k else (-1, 0, 0)) and row[4:7] == ((40 + 8 * k) * 125, 12500, m * 40)
    memo = trk.speed_memo()[0, 0]
    assert memo[2] == n and memo[3] == n % 8 and tuple(memo[4:8]) == (0, 0, 5000, 12500)
    trk.flush_all()
    sp = trk.last_speed
    want = [(3, 0, 0, 0, n - 1, 25000, (40 + 8 * (n - 1)) * 125, 12500, 0, 0, 0, 25000)] if n >= 2 else []
    assert events(sp) == want and int(sp[2][0]) == len(want) and not trk.speed_memo().any()
    assert tuple(sp[0][0, 0]) == (-1, 0, 0, 0, 0, 0, 0, 0)


def test_gap_edge_equal_pushes_one_less_does_not():
    gap = 100000
    trk = tracker([plane(min_gap_us=gap)], clock=True)
    clocks = [0, gap - 1, gap, 2 * gap - 1, 2 * gap + 5, 3 * gap + 5]
    out = drive(trk, line_of(40, 8, 6), clocks)
    assert [r[7] for r, _ in out] == [1 | 256, 1, 2 | 256, 2, 3 | 256, 4 | 256]
    assert [r[4] for r, _ in out] == [5000, 5000, 7000, 7000, 9000, 10000]
    assert out[2][0][1] == 2000 * 10 ** 6 // gap and out[3][0][1] == out[2][0][1]             # no push: the stored estimate stays
    assert trk.speed_memo()[0, 0, 1] == 5                                        # ... while memo.last follows every detection


def test_span_edge_equal_estimates_one_less_does_not():
    span = 90000
    for dt, want in ((span, 1000 * 10 ** 6 // span), (span - 1, -1)):
        trk = tracker([plane(min_span_us=span)], clock=True)
        out = drive(trk, line_of(40, 8, 2), [1000, 1000 + dt])
        assert out[1][0][1] == want and out[1][0][7] == 2 | 256 and out[1][0][6] == (dt // 1000 if want > 0 else 0)
    trk = tracker([plane(min_span_us=span)], clock=True)                        # a clock that stands still, then runs backwards
    out = drive(trk, line_of(40, 8, 3), [5000, 5000, 4000])
    assert [r[1] for r, _ in out] == [-1, -1, -1] and [r[7] for r, _ in out] == [1 | 256, 2 | 256, 2]        # dt 0: pushed, no estimate; dt < 0: no push
    trk.flush_all()
    assert events(trk.last_speed) == [(3, 0, 0, 0, 2, 0, 6000, 12500, 0, 0, 0, 0)]      # the chord of dt = 0 is 0


T_KEY = (1 | 2 << 8 | 3 << 16 | 4 << 24, 5 | 6 << 8 | 7 << 16 | 8 << 24)        # the read of T.make_row's and HandState.put's default ids
CONFIRM_XS = (0.0, 8.0, 16.0, 17.0, 25.0, 33.0, 41.0, 49.0, 57.0)               # px of 125 mm: 1000 mm a frame with one step of 125 mm


def confirm_steps():
    return [(k + 1, None, [(0, 7, k, k + 1, x, 0.0)]) for k, x in enumerate(CONFIRM_XS)]


@pytest.mark.parametrize('confirm', [1, 3])
def test_confirm_counts_estimates_in_a_row_a_dip_resets_and_one_alert_per_track(confirm):
    """Limit 20 m/s.  The estimates over the ring: over, over, under, under (the dip), then over for good: confirm 1 alerts with the
    first estimate, confirm 3 only with the third one after the dip (without the reset it would have been the fifth estimate)."""
    limit = 20000
    _, _, outs = hand_run([plane(limit_mm_s=limit)], confirm_steps(), confirm=confirm)
    speeds = [int(o[0][0, 0, 1]) for o in outs]
    assert speeds == [-1, 25000, 25000, 17708, 19531, 20625, 21354, 21875, 21875]
    fired = [k for k, o in enumerate(outs) if int(o[2][0])]
    assert fired == [1 if confirm == 1 else 7]
    k = fired[0]
    assert tuple(outs[k][1][0, 0]) == (1, 0, 7, 0, k, speeds[k], int(CONFIRM_XS[k] * 125), 0, T_KEY[0], T_KEY[1], k + 1, limit)
    assert [int(o[0][0, 0, 7]) >> 9 & 1 for o in outs] == [0] * k + [1] * (len(outs) - k)
    over = [int(o[3][0, 0, 12]) & 0xFFFF for o in outs]
    assert over == [0, 1, 2, 0, 0, 1, 2, 3, 4] and outs[-1][3][0, 0, 12] >> 16 == 1 and outs[-1][3][0, 0, 11] == 25000


def test_a_slot_reused_in_one_call_ends_before_it_starts():
    trk = tracker([plane()], max_tracks=1, max_age=0)
    drive(trk, line_of(40, 8, 3))
    row, ev = drive(trk, [(600, 300)])[0]                                        # the old track ends, the new one takes its slot
    assert ev == [(3, 0, 0, 0, 2, 25000, 56 * 125, 12500, 0, 0, 0, 25000)]
    assert row == (1, -1, 0, 0, 75000, 37500, 0, 1 | 256)
    assert tuple(trk.speed_memo()[0, 0, :4]) == (2, 3, 1, 1) and not trk.speed_memo()[0, 0, 20:].any()


def test_two_frames_in_one_call_matched_only_the_first():
    trk = tracker([plane()])
    drive(trk, [(40, 100)])
    sp = step_rows(trk, [[T.make_row(Z.box_at(48, 100))], []])                    # now = 3, last = 1: the sample is one period back
    memo = trk.speed_memo()[0, 0]
    assert trk.frame[0] == 3 and memo[1] == 1 and tuple(memo[20:24]) == (PERIOD, 0, 6000, 12500) and sp[0][0, 0, 1] == 25000


def test_clock_given_or_not_and_an_irregular_clock():
    pts = line_of(40, 8, 5)
    plain = drive(tracker([plane()]), pts)
    same = drive(tracker([plane()], clock=True), pts, [10 ** 12 + PERIOD * k for k in range(5)])
    assert plain == same
    clocks = [7, 30007, 90007, 100007, 200007]
    out = drive(tracker([plane()], clock=True), pts, clocks)
    assert [r[1] for r, _ in out[1:]] == [1000 * k * 10 ** 6 // (clocks[k] - 7) for k in range(1, 5)]
    assert [r[6] for r, _ in out] == [(c - 7) // 1000 for c in clocks]
    trk = tracker([plane()])
    trk.speed_clock[:] = 123456789                                               # not enabled: the clock is not read
    assert drive(trk, pts) == plain


def test_a_disabled_stream_reports_none_rows_and_no_events():
    trk = tracker([None, plane()])
    for k in range(3):
        sp = step_rows(trk, [[T.make_row(Z.box_at(40 + 8 * k, 100))]] * 2, stream_of=[0, 1])
        assert (sp[0][0] == (-1, 0, 0, 0, 0, 0, 0, 0)).all() and sp[2][0] == 0 and not trk.speed_memo()[0].any()
    assert sp[0][1, 0, 1] == 25000
    trk.flush_all()
    assert list(trk.last_speed[2]) == [0, 1]


@pytest.mark.parametrize('max_events', [0, 1, 'exact', None])
def test_max_events_caps_the_lines_not_the_count(max_events):
    me = 3 if max_events == 'exact' else max_events
    trk = tracker([plane()], max_events=me)
    for k in range(3):
        step_rows(trk, [[T.make_row(Z.box_at(40 + 8 * k, 60 * j + 30)) for j in range(3)]])
    trk.flush_all()
    ev, count = trk.last_speed[1:]
    assert count[0] == 3 and ev.shape == (1, 4 if me is None else me, 12)
    assert [int(e[3]) for e in ev[0] if e[0]] == [0, 1, 2][:ev.shape[1]] and (me is not None or not ev[0, 3].any())


def test_reset_flush_and_enabling_again():
    from yolov6.utils.speed import GroundPlaneNp
    trk = tracker([plane(), plane()])
    for k in range(3):
        step_rows(trk, [[T.make_row(Z.box_at(40 + 8 * k, 100))]] * 2, stream_of=[0, 1])
    assert trk.speed_memo()[0].any() and trk.speed_memo()[1].any()
    trk.reset([1])
    assert trk.speed_memo()[0].any() and not trk.speed_memo()[1].any()
    sp = step_rows(trk, [[]], stream_of=[0])                                      # silent: stream 1 reports nothing
    assert sp[2][1] == 0 and sp[0][1, 0, 0] == -1
    trk.enable_speed(GroundPlaneNp(2, [plane(), plane()]))                       # again: everything is zero
    assert not trk.speed_memo().any() and trk.last_speed is None
    trk.enable_speed(None)
    step_rows(trk, [[]], stream_of=[0])
    assert trk.last_speed is None and trk.speed_memo() is None
    for bad in (dict(confirm=0), dict(confirm=65536), dict(min_hits=0), dict(max_events=-1)):
        with pytest.raises(ValueError):
            trk.enable_speed(GroundPlaneNp(2, [plane(), None]), **bad)
    with pytest.raises(ValueError):
        trk.enable_speed(GroundPlaneNp(1, [plane()]))


def test_min_hits_three_starts_at_the_third_detection():
    out = drive(tracker([plane()], min_hits=3), line_of(40, 8, 4))
    assert [r[0] for r, _ in out] == [-1, -1, 0, 0] and [r[7] for r, _ in out] == [0, 0, 1 | 256, 2 | 256]


def test_enabling_speed_changes_nothing_else():
    from yolov6.utils.speed import GroundPlaneNp
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.zones import ZoneMapNp
    kw = dict(max_tracks=16, match_thres=0.3, new_thres=0.2, expand=0.25, max_age=2)
    lines, zones = Z.zone_geometry(4, 6, 3)
    a, b = PlateTrackerNp(3, **kw), PlateTrackerNp(3, **kw)
    for t in (a, b):
        t.enable_zones(ZoneMapNp(3, lines, zones))
    b.enable_speed(GroundPlaneNp(3, speed_planes()))
    for det, count, stream_of, flush in Z.zone_calls(4, 16, 8):
        ra, rb = a.update(det, count, stream_of, flush), b.update(det, count, stream_of, flush)
        for x, y in zip(ra + tuple(a.last_zone) + (a.zone_memo,), rb + tuple(b.last_zone) + (b.zone_memo,)):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        for name in PlateTrackerNp._SLOT_ARRAYS:
            assert np.array_equal(getattr(a, name).view(np.uint8), getattr(b, name).view(np.uint8))
    assert a.last_speed is None and b.last_speed[0][0, :, 1].max() > 0


# ---- what tests/test_speed_gpu.py shares ------------------------------------------------------------------------------------------------
def speed_planes(third=None):
    """Planes for the three streams of ``Z.zone_calls`` (1800 x 720 px): two oblique views with a limit, ``third`` for the stream
    that is never fed."""
    return [dict(H=(0.012, 0.001, -9.0, 0.0005, -0.03, 30.0, 0.00002, -0.0011, 1.0), period_us=40000, limit_mm_s=2500, min_gap_us=0, min_span_us=80000),
            dict(H=(0.02, 0.0, -18.0, 0.0, 0.05, 2.0, 0.0, 0.0009, 0.3), period_us=33367, limit_mm_s=4000, min_gap_us=100000, min_span_us=150000), third]


def outputs_np(trk):
    return tuple(trk.last_speed) + (trk.speed_memo(),)


def assert_same(got, want, what):
    names = ('speed_i', 'speed_ev', 'speed_count', 'memo')
    for name, g, w in zip(names, got, want):
        assert g.shape == w.shape and g.dtype == np.int32 and w.dtype == np.int32, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[0]
            raise AssertionError('%s: %s differs at %s: got %d, want %d (%d words differ)' % (what, name, tuple(bad), g[tuple(bad)], w[tuple(bad)],
                                                                                          int((g != w).sum())))


def kinds_seen(speed_ev, speed_count, seen):
    return Z.kinds_seen(speed_ev, speed_count, seen)


@pytest.mark.parametrize('mode', ['grid', 'float', 'nan'])
def test_the_shared_scene_reaches_both_kinds_and_wraps_the_ring(mode):
    from yolov6.utils.speed import GroundPlaneNp
    from yolov6.utils.track import PlateTrackerNp
    kw = dict(max_tracks=64, match_thres=0.3, new_thres=0.2, expand=0.25, max_age=2)
    runs = []
    for _ in range(2):
        trk = PlateTrackerNp(3, **kw)
        trk.enable_speed(GroundPlaneNp(3, speed_planes()), confirm=2)
        seen, out = {}, []
        for det, count, stream_of, flush in Z.zone_calls(5, 64, 20, mode=mode):
            trk.update(det, count, stream_of, flush)
            kinds_seen(trk.last_speed[1], trk.last_speed[2], seen)
            out.append([a.copy() for a in outputs_np(trk)])
            assert not trk.speed_memo()[2].any() and (trk.last_speed[0][2, :, 0] == -1).all()
        runs.append(out)
        assert seen.get(1, 0) > 0 and seen.get(3, 0) > 0, seen
        assert trk.speed_memo()[:2, :, 2].max() > 8                              # the ring wrapped
        invalid = sum(int(((o[0][:, :, 0] >= 0) & ((o[0][:, :, 7] & 255) == 0)).sum()) for o in out)
        assert (invalid > 0) == (mode == 'nan')                                  # tracks whose every anchor was invalid so far
    for a, b in zip(*runs):
        assert_same(a, b, 'second run')


# ---- what the number means: a pinhole camera over a plane at plate height ---------------------------------------------------------------
def camera():
    """A 1920 x 1080 pinhole camera 6 m above the plane z = 0 (the height of the plates), pitched down by 25 degrees, looking along +Y:
    the map (X, Y) on the plane -> pixel."""
    f, cx, cy, hgt, pitch = 1400.0, 960.0, 540.0, 6.0, math.radians(25)
    c, s = math.cos(pitch), math.sin(pitch)

    def project(X, Y):
        xc, yc, zc = X, c * hgt - s * Y, c * Y + s * hgt                         # camera axes: x right, y down, z forward
        return f * xc / zc + cx, f * yc / zc + cy
    return project


def test_accuracy_of_a_vehicle_at_20_metres_a_second():
    """A vehicle at 20 m/s, 25 frames a second, straight through the view of ``camera``, H from four marks.

    The bound.  An endpoint of the estimate is rounded to whole millimetres per coordinate: it moves by at most sqrt(0.5^2 + 0.5^2)
    mm, the two endpoints together change the distance d by at most sqrt(2) mm; the floor of the root takes off less than 1 mm:
    s is in (d - sqrt(2) - 1, d + sqrt(2)].  speed = floor(s * 10^6 / dt) takes off less than 1 mm/s more.  So
        |speed - d * 10^6 / dt| < (sqrt(2) + 1) * 10^6 / dt + 1,
    with d and the comparison in float64, whose own error (a few 1e-16 relative on 1e5 mm) is covered by 1e-6 mm/s.  Against the TRUTH,
    without jitter, two more terms: the anchor is the fp32 centre of an fp32 box, off the projected point by at most 1.5 ulp of 2048,
    2^-12 * 1.5 px per axis (two roundings of the corners, one of the sum), which the plane's largest stretch J (mm / px, measured
    along the path by differences) turns into at most 2 * sqrt(2) * 1.5 * 2^-12 * J mm over the two endpoints; and the fit of H to
    exact marks, 1e-9 relative of 50 m.  With jitter the anchors are what they are: the comparison is against the same endpoint
    estimator in float64 on the un-rounded world points, and the error against the truth is printed, not bounded."""
    from yolov6.utils.speed import GroundPlaneNp, homography_from_points
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.zones import anchor_of
    project = camera()
    marks = np.array([(-3.0, 10.0), (3.0, 10.0), (3.0, 40.0), (-3.0, 40.0)])
    H = homography_from_points(np.array([project(*m) for m in marks]), marks)
    v_true, dt_frame, n = 20000.0, 40000, 40
    path = [(1.0, 44.0 - 0.8 * k) for k in range(n)]                             # 0.8 m a frame, towards the camera

    def world64(ax, ay):
        p = H @ np.array([float(ax), float(ay), 1.0])
        return p[0] / p[2] * 1000.0, p[1] / p[2] * 1000.0
    J = 0.0
    for X, Y in path:
        u, v = project(X, Y)
        for du, dv in ((1, 0), (0, 1)):
            a, b = world64(u, v), world64(u + du, v + dv)
            J = max(J, math.hypot(a[0] - b[0], a[1] - b[1]))
    J *= 1.5                                                                     # the stretch of a direction between the axes
    for jitter in (0.0, 0.5):
        rng = np.random.default_rng(8)
        trk = PlateTrackerNp(1, max_tracks=4, match_thres=0.2, new_thres=0.0, expand=0.5, max_age=2)
        trk.enable_speed(GroundPlaneNp(1, [dict(H=H, period_us=dt_frame, min_span_us=200000)]))
        anchors, worst_spec, worst_truth = [], 0.0, 0.0
        for k, (X, Y) in enumerate(path):
            u, v = project(X, Y)
            u, v = u + rng.uniform(-jitter, jitter), v + rng.uniform(-jitter, jitter)
            trk.update(*T.frames_of([[T.make_row((u - 120, v - 70, u + 120, v + 70))]], 2), stream_of=[0])
            row = trk.last_speed[0][0, 0]
            assert row[0] == 0 and (row[7] & 255) == min(k + 1, 8) and row[7] & 256, (k, row)
            anchors.append(world64(*anchor_of(trk.box[0, 0])))
            if k < 5:                                                            # under min_span: no estimate yet
                assert row[1] == -1
                continue
            o, e = anchors[max(0, k - 7)], anchors[k]
            dt = dt_frame * min(k, 7)
            want = math.hypot(e[0] - o[0], e[1] - o[1]) * 1e6 / dt
            bound = (math.sqrt(2) + 1) * 1e6 / dt + 1 + 1e-6
            print('jitter %.1f frame %2d: speed %d, float64 estimator %.3f (bound %.3f), truth %.0f' % (jitter, k, row[1], want, bound, v_true))
            assert abs(row[1] - want) < bound
            worst_spec, worst_truth = max(worst_spec, abs(row[1] - want)), max(worst_truth, abs(row[1] - v_true))
            if jitter == 0.0:
                extra = (2 * math.sqrt(2) * 1.5 * 2.0 ** -12 * J + 1e-9 * 50000 * 2) * 1e6 / dt
                assert abs(row[1] - v_true) < bound + extra, (k, row[1], bound, extra)
        print('jitter +-%.1f px: worst |speed - float64 estimator| %.3f mm/s, worst |speed - truth| %.1f mm/s (%.2f %%)'
              % (jitter, worst_spec, worst_truth, 100 * worst_truth / v_true))


# ---- the host helpers -------------------------------------------------------------------------------------------------------------------
def test_homography_from_points():
    from yolov6.utils.speed import homography_from_points
    project = camera()
    world = np.array([(-3.0, 10.0), (3.0, 10.0), (3.5, 40.0), (-2.5, 38.0), (0.5, 20.0)])
    px = np.array([project(*m) for m in world])
    for n in (4, 5):
        H = homography_from_points(px[:n], world[:n])
        p = np.c_[px[:n], np.ones(n)] @ H.T
        assert (p[:, 2] > 0).all() and np.abs(p[:, :2] / p[:, 2:] - world[:n]).max() <= 1e-9 * np.abs(world).max()
    with pytest.raises(ValueError):
        homography_from_points(px[:3], world[:3])
    with pytest.raises(ValueError, match='degenerate'):
        homography_from_points([(0, 0), (1, 1), (2, 2), (3, 3)], [(0, 0), (1, 1), (2, 2), (3, 3)])
    with pytest.raises(ValueError, match='degenerate'):
        homography_from_points([(0, 0), (1, 1), (2, 2), (5, 0)], [(0, 0), (1, 0), (2, 0), (0, 5)])
    with pytest.raises(ValueError):
        homography_from_points([(0, 0), (1, 0), (1, 1), (0, NAN)], [(0, 0), (1, 0), (1, 1), (0, 1)])


GROUND_TXT = """# two cameras
plane 0.0125 0 -1 0 0.0125 -0.8 0 0 1      # stream 0: 12.5 mm a pixel
fps 25
limit 50
1: points 0 0 0 0  160 0 8 0  160 128 8 6.4  0 128 0 6.4
1: period_us 33367
1: gap_ms 50
1: span_ms 120.5
"""


def test_parse_ground_round_trip_and_validation(tmp_path):
    from yolov6.utils.speed import MAP_WORDS, GroundPlaneNp, check_packed, format_ground, parse_ground
    planes = parse_ground(GROUND_TXT, 3)
    assert planes[2] is None and planes[0]['period_us'] == 40000 and planes[0]['limit_mm_s'] == 13889 and 'min_gap_us' not in planes[0]
    assert (planes[1]['period_us'], planes[1]['min_gap_us'], planes[1]['min_span_us']) == (33367, 50000, 120500)
    assert np.allclose(planes[1]['H'].reshape(3, 3) / planes[1]['H'][8], np.diag([0.05, 0.05, 1]), atol=1e-12)
    g = GroundPlaneNp(3, planes)
    assert g.packed.shape == (3, MAP_WORDS) and not g.packed[2].any() and list(g.packed[0, 18:23]) == [40000, 13889, 0, 200000, 1]
    assert np.array_equal(g.packed[0, :18].view(f64), np.array([0.0125, 0, -1, 0, 0.0125, -0.8, 0, 0, 1]))
    path = tmp_path / 'ground.txt'
    path.write_text(format_ground(g))
    assert np.array_equal(GroundPlaneNp(3, parse_ground(str(path), 3)).packed, g.packed)
    assert GroundPlaneNp(2, {1: plane()}).planes_np[0] is None
    for bad in ('plane 1 2 3', 'fps 25', 'plane 1 0 0 0 1 0 0 0 1\nplane 1 0 0 0 1 0 0 0 1', '3: fps 25', 'x: fps 25', 'speed 5', 'plane 1 0 0 0 1 0 0 0 nan',
                'points 0 0 0 0 1 1 1 1 2 2 2 2 3 3 3 3', 'points 0 0 0 0 1 0 1 0 1 1 1', 'plane 1 0 0 0 1 0 0 0 1\nfps 0', 'plane 1 0 0 0 1 0 0 0 1\nlimit -1',
                'plane 1 0 0 0 1 0 0 0 1\nfps 25 30'):
        with pytest.raises(ValueError):
            GroundPlaneNp(3, parse_ground(bad + '\n', 3))
    for bad in (dict(H=(1, 0, 0, 0, 1, 0, 0, 0, INF)), dict(H=(1, 2, 3)), dict(H=EIGHTH, period_us=0), dict(H=EIGHTH, period_us=10 ** 7 + 1),
                dict(H=EIGHTH, limit_mm_s=-1), dict(H=EIGHTH, min_gap_us=-1), dict(H=EIGHTH, min_span_us=0), dict(H=EIGHTH, period_us=2.5),
                dict(H=EIGHTH, fps=25), dict(period_us=40000)):
        with pytest.raises(ValueError):
            GroundPlaneNp(1, [bad])
    with pytest.raises(ValueError):
        GroundPlaneNp(1, [plane(), plane()])
    assert GroundPlaneNp(1, [plane(period_us=10 ** 7)]).packed[0, 18] == 10 ** 7
    for word, value in ((22, 2), (18, 0), (19, -1), (21, 0), (23, 1), (31, 5), (1, 0x7FF00000)):
        p = GroundPlaneNp(2, [plane(), None]).packed.copy()
        p[0, word] = value
        with pytest.raises(ValueError):
            check_packed(p)
    p = GroundPlaneNp(2, [plane(), None]).packed.copy()
    p[1, 18] = 40000                                                             # a disabled stream is all zero
    with pytest.raises(ValueError):
        check_packed(p)


# ---- tools/infer.py --track --speed on the CPU path -------------------------------------------------------------------------------------
INFER_GROUND_TXT = """# a 160 x 128 picture, 50 mm a pixel: the patch of T._moving_frames moves 4 px = 0.2 m a frame, 18 km/h at 25 fps
# (the detections of the test's random weights wander far less: the limit is set under them)
points 0 0 0 0  160 0 8 0  160 128 8 6.4  0 128 0 6.4
fps 25
limit 0.4
span_ms 80
"""


def expected_speed_files(dets, max_det, text, min_hits, confirm, **kw):
    """(speeds.txt, speeding.txt) lines by hand: ``PlateTrackerNp`` with the plane over the untracked per-frame detections of one
    stream, one update per frame, then the flush."""
    from yolov6.utils.speed import GroundPlaneNp, kmh, parse_ground
    from yolov6.utils.track import PlateTrackerNp, plate_text
    trk = PlateTrackerNp(1, **kw)
    trk.enable_speed(GroundPlaneNp(1, parse_ground(text, 1)), min_hits, confirm)
    speeds, speeding = [], []

    def collect(ended_i, ended_count):
        _, ev, count = trk.last_speed
        assert count[0] <= ev.shape[1]
        for e in ev[0, :count[0]]:
            if e[0] == 3:
                reads = [ended_i[0, k, 4:12] for k in range(int(ended_count[0])) if ended_i[0, k, 0] == e[2]]
                speeds.append('%d %s %.1f %.1f' % (e[2], plate_text(reads[0]) if reads else '-', kmh(e[5]), kmh(e[11])))
            else:
                speeding.append('%d %d %s %.1f %.1f' % (e[4], e[2], plate_text(np.array([e[8], e[9]], np.int32).view(np.uint8)), kmh(e[5]), kmh(e[11])))
    for d in dets:
        pad = np.zeros((1, max_det, 28), f32)
        pad[0, :len(d)] = d
        _, _, ei, _, ec = trk.update(pad, [len(d)], max_ended=2 * trk.max_tracks)
        collect(ei, ec)
    _, _, ei, _, ec = trk.flush_all()
    collect(ei, ec)
    return speeds, speeding


def check_infer_speed(tmp_path, infer, kw, untracked, tkw):
    import torch
    (tmp_path / 'ground.txt').write_text(INFER_GROUND_TXT)
    plain = infer.run(save_dir=str(tmp_path / 'o1'), track=True, **kw)
    assert not (tmp_path / 'o1' / 'speeds.txt').exists() and not (tmp_path / 'o1' / 'speeding.txt').exists()
    n = 0
    for sub, min_hits, confirm in (('o2', 1, 1), ('o3', 2, 2)):
        again = infer.run(save_dir=str(tmp_path / sub), track=True, speed=str(tmp_path / 'ground.txt'), speed_min_hits=min_hits, speed_confirm=confirm, **kw)
        for a, b in zip(plain, again):
            assert torch.equal(a, b)
        for name in ('tracks.txt', 'plates.txt'):                                # byte-identical to the run without the switch
            assert (tmp_path / sub / name).read_bytes() == (tmp_path / 'o1' / name).read_bytes()
        want_s, want_a = expected_speed_files(untracked, 20, INFER_GROUND_TXT, min_hits, confirm, **tkw)
        assert (tmp_path / sub / 'speeds.txt').read_text().splitlines() == want_s, sub
        assert (tmp_path / sub / 'speeding.txt').read_text().splitlines() == want_a, sub
        n += len(want_s) + len(want_a)
        assert want_s and want_a, (want_s, want_a)
    assert n > 2
    with pytest.raises(ValueError, match='track'):
        infer.run(save_dir=str(tmp_path / 'o4'), speed=str(tmp_path / 'ground.txt'), **kw)


def test_infer_speed_cpu(tmp_path, monkeypatch):
    check_infer_speed(tmp_path, *Z.infer_zones_case(tmp_path, monkeypatch, 'cpu'))
