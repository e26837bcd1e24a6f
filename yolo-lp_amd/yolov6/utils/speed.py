"""Speed of live plate tracks on a calibrated ground plane, with an alert over a limit, on the CPU: ``SpeedNp`` is the written-down
specification of ``lp_speed_update`` (include/lp_hip.h, csrc/lp_speed.hip), which matches it on every int32, the memo included, and
the CPU path of ``Inferer(track=True, speed=...)``.

The reference has nothing here: its Inferer treats frames independently (yolov6/core/inferer.py).

The tracker, the watchlists and the sightings log say WHICH plate, ``yolov6.utils.zones`` says which way and how long; all of it in
pixels of the frame, where a pixel near the horizon is many metres and one at the bottom edge a few centimetres.  This module maps
the tracker's anchor through a homography to millimetres on a plane and differences the positions over time.

Calibration of one stream (``GroundPlaneNp`` validates and packs it, ``MAP_WORDS`` = 32 int32 words per stream, the layout
``lp_speed_update`` takes): words 0..17: ``H``, a 3x3 fp64 homography, row-major h0..h8, as bit pairs (lo, hi), all finite; it maps
frame pixels to metres on the plane THE PLATES MOVE IN -- calibrate at plate height, not on the road surface; 18: ``period_us``
(1..10^7), the nominal frame period; 19: ``limit_mm_s`` (>= 0, 0: no alert); 20: ``min_gap_us`` (>= 0); 21: ``min_span_us`` (>= 1);
22: enabled (0 / 1); 23..31: 0.  A stream without a plane is all zero: it produces "none" rows and no events.

World point of an anchor.  The anchor is the tracker's own cx, cy, exactly as ``zones.anchor_of`` takes it (fp32), widened to fp64 as
x, y.  Every operation is one IEEE fp64 operation, rounded on its own, in this order, no fused multiply-add:
  u = (h0 * x + h1 * y) + h2;  v = (h3 * x + h4 * y) + h5;  w = (h6 * x + h7 * y) + h8;  X = u / w;  Y = v / w (the rule's only two
  divisions, plain correctly rounded ``/``);  PX = X * 1000.0, PY = Y * 1000.0;  X_mm = rint(PX), Y_mm = rint(PY) (ties to even).
The point is valid iff the anchor is finite (``zones.finite_point``), w > 0, |PX| <= 2^30 and |PY| <= 2^30: plain compares, false for
NaN.  From here on everything is integer.

Time of a sample: with now = the stream's frame counter as the call left it and last = the slot's last matched frame,
t_us = base - int64(int32(now - last)) * period_us (the int32 difference wraps); base = clock_us[s] when the optional clock is given
(int64 [S], set by the caller before a call), else int64(now) * period_us.  int64 sums and differences wrap; a caller keeps its clock
inside +-2^62.

Memo: int32 [S, T, ``MEMO_WORDS`` = 48], all zero = empty.  Word 0: id + 1; 1: last; 2: samples pushed (saturating at 2^31 - 1); 3: ring
head (where the next sample goes, 0..7); 4, 5: t_first (lo, hi); 6, 7: X_first, Y_first; 8..10: the stored estimate speed (-1: none
yet), vx, vy in mm/s; 11: peak; 12: over | alerted << 16 (over saturates at 65535); 13: span_ms; 14, 15: 0; 16 + 4 k ..: sample k of a
ring of ``RING`` = 8 as t_lo, t_hi, X_mm, Y_mm.  The ring holds n = min(pushed, 8) samples; the newest is at (head - 1) & 7, the oldest
at 0 while pushed < 8, else at head.

Steps.  They run after an ``update`` call, on the tracker state as that call left it.  Every stream is processed, whether or not it had
a frame in the call; the slots go in ascending order:
  1. a slot is eligible iff its stream is enabled, it is live (hits > 0) and hits >= min_hits;
  2. a non-empty memo line whose slot is not eligible, or holds another id, is GONE: if it pushed at least 2 samples it emits kind 3
     (ended) with frame = memo.last, value = peak, aux = the chord speed from the first to the newest sample by the estimator of 5 (0 if
     their dt <= 0; no min_span), the newest sample's position, key 0 and hits 0; then the line is zeroed;
  3. an eligible slot with an empty line starts: id + 1 and last are stored, the stored speed is -1; if its world point is valid it
     pushes the first sample, which also becomes ``first``;
  4. an eligible slot holding its id, with slot.last != memo.last (a new detection): memo.last = slot.last; if the point is valid and
     (no sample yet, or t - t_newest >= min_gap_us) it pushes, overwriting the oldest once the ring holds 8 (the first sample pushed,
     here or in 3, becomes ``first``).  A call that pushed is FRESH for the slot; 5 and 6 run only then;
  5. estimate, only when fresh and the ring holds at least 2 samples: o = the oldest, e = the newest sample of the ring,
     dt = t_e - t_o; if dt >= min_span_us: dx, dy int64 differences, d2 = dx * dx + dy * dy (at most 2^63), s = floor(sqrt(d2)) EXACT,
     speed = min(s * 10^6 // dt, 2^31 - 1), vx = sign(dx) * min(|dx| * 10^6 // dt, 2^31 - 1), vy likewise,
     span_ms = min(dt // 1000, 2^31 - 1), peak = max(peak, speed).  Otherwise the stored estimate stays;
  6. alert, only when 5 produced an estimate in this call and limit_mm_s > 0: if speed > limit, over += 1, and when over >= confirm
     and the alerted bit is clear it emits kind 1 (value = speed, aux = limit) and sets the bit; if speed <= limit, over = 0.  One
     alert per track;
  7. speed_i [S, T, 8], one row per slot: (id, speed, vx, vy, X_mm, Y_mm of the newest sample (0, 0 without one), span_ms,
     n | fresh << 8 | alerted << 9); a slot that is not eligible reports (-1, 0, 0, 0, 0, 0, 0, 0);
  8. speed_ev [S, max_events, 12]: kind, 0, id, slot, frame (slot.last for kind 1), value, X_mm, Y_mm of the newest sample, key_lo,
     key_hi (the voted read via ``watch_live.read_key``; 0 for kind 3), hits, aux; in slot order, step 2 before step 6 within a slot;
     speed_count [S]: the number produced, not capped -- lines at or past max_events are not written, lines from the count to
     max_events are zero.  Every word of the three outputs is written by every call.  A slot yields at most one event per call (a line
     that is gone restarts with one sample), so ``max_events`` defaults to ``max_tracks``.
``confirm`` is 1..65535.  ``reset(streams)`` zeroes those streams' memo without events; a flush ends the tracks, so that step 2
reports them; enabling again zeroes everything.  The map is fixed while a memo lives, so a disabled stream's memo stays empty.

What it does not do: the estimator is the endpoint difference over the ring (at most 8 samples, at least ``min_span_us`` apart end
to end) -- no filtering, no acceleration, no lens-distortion model; a vehicle's plate sits off the calibrated plane by its
mounting-height spread, which scales its speed by about that spread over the camera's height above the plane; positions are those at
the end of a call (a stream with several frames in one call gives one sample); ``now`` and the clock must not run backwards -- with
dt <= 0 there is no estimate; a missed frame gives no sample, the speed reported meanwhile is the last estimate; zones stay in
pixels (``yolov6.utils.scene`` draws the speed as a km/h tag); speed across cameras is ``sight``'s journey time.
"""
import math
import os

import numpy as np

from yolov6.utils.watch_live import check_min_hits, read_key
from yolov6.utils.zones import anchor_of, finite_point

MAP_WORDS, MEMO_WORDS, RING = 32, 48, 8
MAP_PERIOD, MAP_LIMIT, MAP_GAP, MAP_SPAN, MAP_ENABLED = 18, 19, 20, 21, 22
ROW_COLS, EV_COLS = 8, 12
KIND_ALERT, KIND_ENDED = 1, 3
NO_ROW = (-1, 0, 0, 0, 0, 0, 0, 0)
MAX_PERIOD_US = 10 ** 7
MAX_CONFIRM = 65535
I32_MAX = 2 ** 31 - 1
WORLD_LIMIT = float(2 ** 30)                # |X * 1000| and |Y * 1000| of a valid point
DEFAULTS = dict(period_us=40000, limit_mm_s=0, min_gap_us=0, min_span_us=200000)
f32, f64 = np.float32, np.float64


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------
def world_point(H, ax, ay):
    """(valid, X_mm, Y_mm) of the anchor (ax, ay) (fp32; scalars or arrays that broadcast) through ``H`` [9] fp64: bool and int64,
    0 where the point is not valid.  One rounded fp64 operation at a time, in the order of the module's rule."""
    h = np.asarray(H, f64).reshape(9)
    x, y = np.asarray(ax, f32).astype(f64), np.asarray(ay, f32).astype(f64)
    with np.errstate(all='ignore'):
        u = (h[0] * x + h[1] * y) + h[2]
        v = (h[3] * x + h[4] * y) + h[5]
        w = (h[6] * x + h[7] * y) + h[8]
        px, py = (u / w) * 1000.0, (v / w) * 1000.0
        valid = finite_point(ax, ay) & (w > 0) & (np.abs(px) <= WORLD_LIMIT) & (np.abs(py) <= WORLD_LIMIT)
        xm = np.rint(np.where(valid, px, 0.0)).astype(np.int64)
        ym = np.rint(np.where(valid, py, 0.0)).astype(np.int64)
    return valid, xm, ym


def estimate(dx, dy, dt):
    """(speed, vx, vy, span_ms) of step 5 for integer differences in mm and dt > 0 in microseconds (Python integers, exact)."""
    dx, dy, dt = int(dx), int(dy), int(dt)
    if dt <= 0:
        raise ValueError('dt must be > 0')
    s = math.isqrt(dx * dx + dy * dy)
    comp = lambda d: (1 if d > 0 else -1) * min(abs(d) * 10 ** 6 // dt, I32_MAX)         # noqa: E731
    return min(s * 10 ** 6 // dt, I32_MAX), comp(dx), comp(dy), min(dt // 1000, I32_MAX)


def kmh(mm_s):
    """mm/s as km/h (a float, for reports)."""
    return int(mm_s) * 0.0036


def _w32(v):
    """A Python integer as int32, wrapping."""
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


def _w64(v):
    """A Python integer as int64, wrapping."""
    return (int(v) + 2 ** 63) % 2 ** 64 - 2 ** 63


def _join(lo, hi):
    """The int64 of two int32 words (lo, hi)."""
    return _w64((int(hi) << 32) | (int(lo) & 0xFFFFFFFF))


def _split(t):
    """(lo, hi) int32 words of an int64."""
    t = int(t) & (2 ** 64 - 1)
    return _w32(t & 0xFFFFFFFF), _w32(t >> 32)


def sample_time(now, last, period_us, base=None):
    """t_us of a sample: base - int64(int32(now - last)) * period_us, base = int64(now) * period_us without a clock."""
    base = int(now) * int(period_us) if base is None else int(base)
    return _w64(base - _w32(int(now) - int(last)) * int(period_us))


# ---- the calibration ---------------------------------------------------------------------------------------------------------
def _per_stream(planes, n_streams):
    if planes is None:
        return [None] * n_streams
    if isinstance(planes, dict):
        for s in planes:
            if not 0 <= int(s) < n_streams:
                raise ValueError('plane of stream %s: need a stream in 0..%d' % (s, n_streams - 1))
        return [planes.get(s) for s in range(n_streams)]
    planes = list(planes)
    if len(planes) != n_streams:
        raise ValueError('planes must have one entry per stream (%d), or be a dict by stream' % n_streams)
    return planes


def _int_in(plane, key, lo, hi, s):
    v = plane.get(key, DEFAULTS[key])
    if isinstance(v, (bool, np.bool_)) or int(v) != v or not lo <= int(v) <= hi:
        raise ValueError('stream %d: %s must be an integer in %d..%d' % (s, key, lo, hi))
    return int(v)


class GroundPlaneNp:
    """The calibrated plane of each of ``n_streams`` streams, validated and packed (the module docstring states the layout).
    ``planes``: one entry per stream (or a dict by stream, or None): None for a stream without a plane, else a dict with ``H`` (nine
    numbers or 3 x 3: frame pixels -> metres on the plane the plates move in) and optionally ``period_us`` (default 40000),
    ``limit_mm_s`` (0: no alert), ``min_gap_us`` (0), ``min_span_us`` (200000).  ``planes_np``: the checked copies, per stream None or
    a dict with ``H`` fp64 [9] and the four integers; ``packed``: int32 [S, 32].  ValueError for a value of H that is not finite, a
    field out of range and an unknown key."""

    def __init__(self, n_streams, planes=None, device=None):
        S = int(n_streams)
        if S < 1:
            raise ValueError('n_streams must be >= 1')
        self.n_streams, self.planes_np = S, []
        self.packed = np.zeros((S, MAP_WORDS), np.int32)
        for s, plane in enumerate(_per_stream(planes, S)):
            if plane is None:
                self.planes_np.append(None)
                continue
            if not isinstance(plane, dict) or 'H' not in plane or set(plane) - set(DEFAULTS) - {'H'}:
                raise ValueError('stream %d: a plane is a dict with H and any of %s' % (s, ', '.join(DEFAULTS)))
            try:
                H = np.asarray(plane['H'], f64).reshape(-1)
            except (TypeError, ValueError):
                raise ValueError('stream %d: H must be nine numbers' % s)
            if H.size != 9 or not np.isfinite(H).all():
                raise ValueError('stream %d: H must be nine finite numbers' % s)
            p = dict(H=np.ascontiguousarray(H), period_us=_int_in(plane, 'period_us', 1, MAX_PERIOD_US, s),
                     limit_mm_s=_int_in(plane, 'limit_mm_s', 0, I32_MAX, s), min_gap_us=_int_in(plane, 'min_gap_us', 0, I32_MAX, s),
                     min_span_us=_int_in(plane, 'min_span_us', 1, I32_MAX, s))
            self.planes_np.append(p)
            row = self.packed[s]
            row[0:18] = p['H'].view(np.int32)
            row[MAP_PERIOD], row[MAP_LIMIT], row[MAP_GAP], row[MAP_SPAN], row[MAP_ENABLED] = (
                p['period_us'], p['limit_mm_s'], p['min_gap_us'], p['min_span_us'], 1)
        check_packed(self.packed)


def check_packed(packed):
    """The rules of a packed map int32 [S, MAP_WORDS] (ValueError): the enabled flag 0 / 1, a finite H, the four integers in range,
    zero padding, and a disabled stream all zero."""
    p = np.asarray(packed)
    if p.dtype != np.int32 or p.ndim != 2 or p.shape[1] != MAP_WORDS or p.shape[0] < 1:
        raise ValueError('a packed ground map is int32 [S, %d]' % MAP_WORDS)
    for s in range(p.shape[0]):
        row = np.ascontiguousarray(p[s])
        if row[MAP_ENABLED] == 0:
            ok = not row.any()
        else:
            ok = (row[MAP_ENABLED] == 1 and np.isfinite(row[0:18].view(f64)).all() and 1 <= row[MAP_PERIOD] <= MAX_PERIOD_US
                  and row[MAP_LIMIT] >= 0 and row[MAP_GAP] >= 0 and row[MAP_SPAN] >= 1 and not row[MAP_ENABLED + 1:].any())
        if not ok:
            raise ValueError('stream %d: bad plane, field or padding' % s)


def _normalise(p):
    c = p.mean(0)
    d = np.sqrt(((p - c) ** 2).sum(1)).mean()
    if not d > 0:
        raise ValueError('the points coincide')
    k = math.sqrt(2.0) / d
    return np.array([[k, 0, -k * c[0]], [0, k, -k * c[1]], [0, 0, 1]], f64)


def homography_from_points(px, world_m):
    """H fp64 [3, 3] with H (x, y, 1) ~ (X, Y, 1) for the n >= 4 correspondences ``px`` [n, 2] (frame pixels) -> ``world_m`` [n, 2]
    (metres on the plane): the normalised direct linear transform, least squares for n > 4; scaled so that w is 1 at the centroid of
    ``px``.  ValueError for fewer than four points, a degenerate set (three of four on a line, coincident points), values that are
    not finite and a solution that puts a given point at w <= 0."""
    px, world_m = np.asarray(px, f64), np.asarray(world_m, f64)
    if px.ndim != 2 or px.shape[1] != 2 or px.shape != world_m.shape or len(px) < 4:
        raise ValueError('homography_from_points needs px [n, 2] and world_m [n, 2], n >= 4')
    if not (np.isfinite(px).all() and np.isfinite(world_m).all()):
        raise ValueError('the points must be finite')
    T1, T2 = _normalise(px), _normalise(world_m)
    a = (T1 @ np.c_[px, np.ones(len(px))].T).T
    b = (T2 @ np.c_[world_m, np.ones(len(px))].T).T
    rows = []
    for (x, y, _), (X, Y, _) in zip(a, b):
        rows.append([-x, -y, -1, 0, 0, 0, X * x, X * y, X])
        rows.append([0, 0, 0, -x, -y, -1, Y * x, Y * y, Y])
    _, sv, vt = np.linalg.svd(np.asarray(rows, f64))
    if sv[7] <= 1e-10 * sv[0]:
        raise ValueError('the points are degenerate (collinear or coincident): no unique homography')
    H = np.linalg.inv(T2) @ vt[8].reshape(3, 3) @ T1
    wc = H[2] @ np.r_[px.mean(0), 1.0]
    if not abs(wc) > 0:
        raise ValueError('the points are degenerate: w vanishes at their centroid')
    H = H / wc
    if not ((np.c_[px, np.ones(len(px))] @ H[2]) > 0).all():
        raise ValueError('the horizon of the solution passes between the points')
    return H


def _number(tok, no):
    try:
        v = float(tok)
    except ValueError:
        raise ValueError('line %d: bad number %r' % (no, tok))
    if not math.isfinite(v):
        raise ValueError('line %d: %r is not finite' % (no, tok))
    return v


def parse_ground(text_or_path, n_streams=1):
    """Read the text format, one item per line, ``#`` starts a comment, ``S:`` in front names the stream (default 0):
        [S:] plane h0 h1 h2 h3 h4 h5 h6 h7 h8          the homography itself, row-major, pixels -> metres
        [S:] points x y X Y  x y X Y  ...              or at least four marks: pixel x y -> metres X Y (``homography_from_points``)
        [S:] fps F   |   [S:] period_us N              the frame period (default 25 fps)
        [S:] limit KMH                                 the speed limit in km/h (0 or absent: no alert)
        [S:] gap_ms N    [S:] span_ms N                min_gap_us / 1000 (default 0), min_span_us / 1000 (default 200)
    A stream needs exactly one of ``plane`` / ``points`` to have a plane; settings of a stream without one are an error.  Returns the
    list ``GroundPlaneNp`` takes: per stream None or a dict.  ``text_or_path``: the text itself (it has a newline) or a file's path."""
    text = str(text_or_path)
    if '\n' not in text and os.path.exists(text):
        with open(text) as f:
            text = f.read()
    S = int(n_streams)
    planes = [dict() for _ in range(S)]
    for no, raw in enumerate(text.splitlines(), 1):
        tok = raw.split('#', 1)[0].split()
        if not tok:
            continue
        s = 0
        if tok[0].endswith(':'):
            try:
                s = int(tok[0][:-1])
            except ValueError:
                raise ValueError('line %d: bad stream prefix %r' % (no, tok[0]))
            tok = tok[1:]
        if not 0 <= s < S:
            raise ValueError('line %d: stream %d outside 0..%d' % (no, s, S - 1))
        if not tok:
            raise ValueError('line %d: nothing behind the stream prefix' % no)
        word, vals = tok[0], [_number(t, no) for t in tok[1:]]
        p = planes[s]
        key = {'plane': 'H', 'points': 'H', 'fps': 'period_us', 'period_us': 'period_us', 'limit': 'limit_mm_s', 'gap_ms': 'min_gap_us',
               'span_ms': 'min_span_us'}.get(word)
        if key is None:
            raise ValueError('line %d: expected plane, points, fps, period_us, limit, gap_ms or span_ms, not %r' % (no, word))
        if key in p:
            raise ValueError('line %d: stream %d has %s twice' % (no, s, 'a plane' if key == 'H' else word))
        if word == 'plane':
            if len(vals) != 9:
                raise ValueError('line %d: a plane has nine numbers' % no)
            p['H'] = np.asarray(vals, f64)
        elif word == 'points':
            if len(vals) % 4 or len(vals) < 16:
                raise ValueError('line %d: points are at least four groups x y X Y' % no)
            q = np.asarray(vals, f64).reshape(-1, 4)
            try:
                p['H'] = homography_from_points(q[:, :2], q[:, 2:]).reshape(9)
            except ValueError as e:
                raise ValueError('line %d: %s' % (no, e))
        else:
            if len(vals) != 1 or vals[0] < 0 or (word in ('fps',) and not vals[0] > 0):
                raise ValueError('line %d: %s takes one number >= 0' % (no, word))
            v = vals[0]
            p[key] = int(np.rint({'fps': lambda: 1e6 / v, 'period_us': lambda: v, 'limit': lambda: v * 1e6 / 3600.0, 'gap_ms': lambda: v * 1000.0,
                                  'span_ms': lambda: v * 1000.0}[word]()))
    for s, p in enumerate(planes):
        if p and 'H' not in p:
            raise ValueError('stream %d has settings but neither plane nor points' % s)
    return [p or None for p in planes]


def format_ground(ground):
    """The text of a calibration (anything with ``n_streams`` and ``planes_np``) that ``parse_ground`` reads back to the same map."""
    out = []
    for s in range(ground.n_streams):
        p = ground.planes_np[s]
        if p is None:
            continue
        out.append('%d: plane %s' % (s, ' '.join(repr(float(v)) for v in p['H'])))
        out.append('%d: period_us %d' % (s, p['period_us']))
        out.append('%d: limit %r' % (s, p['limit_mm_s'] * 3600 / 1e6))
        out.append('%d: gap_ms %r' % (s, p['min_gap_us'] / 1000.0))
        out.append('%d: span_ms %r' % (s, p['min_span_us'] / 1000.0))
    return '\n'.join(out) + '\n'


# ---- the steps ---------------------------------------------------------------------------------------------------------------
def check_confirm(confirm):
    c = int(confirm)
    if c != confirm or not 1 <= c <= MAX_CONFIRM:
        raise ValueError('confirm must be an integer in 1..%d' % MAX_CONFIRM)
    return c


class SpeedNp:
    """The memo and the steps of the module's rule.  ``ground``: anything with ``n_streams`` and ``planes_np`` (``GroundPlaneNp``,
    ``runtime.GroundPlane``).  ``step(tracker, clock_us=None)`` after an ``update`` of ``tracker`` -- a ``PlateTrackerNp``, or anything
    with ``frame`` [S], ``id`` / ``last`` / ``hits`` [S, T], ``box`` [S, T, 4] and ``read(s, t)`` -- returns (speed_i [S, T, 8],
    speed_ev [S, max_events, 12], speed_count [S]) int32; ``clock_us``: int64 [S] or None."""

    def __init__(self, ground, max_tracks, min_hits=1, confirm=2, max_events=None):
        self.ground, self.n_streams, self.max_tracks = ground, int(ground.n_streams), int(max_tracks)
        if not 1 <= self.max_tracks <= 128:
            raise ValueError('max_tracks must be in 1..128')
        self.min_hits, self.confirm = check_min_hits(min_hits), check_confirm(confirm)
        self.max_events = self.max_tracks if max_events is None else int(max_events)
        if self.max_events < 0:
            raise ValueError('max_events must be >= 0')
        self.memo = np.zeros((self.n_streams, self.max_tracks, MEMO_WORDS), np.int32)

    def reset(self, streams=None):
        """Zero the memo of ``streams`` (all for None), without events."""
        for s in (range(self.n_streams) if streams is None else streams):
            self.memo[int(s)] = 0

    @staticmethod
    def _sample(m, k):
        """(t, X, Y) of sample k of the ring of memo line ``m``."""
        w = m[16 + 4 * k:20 + 4 * k]
        return _join(w[0], w[1]), int(w[2]), int(w[3])

    @classmethod
    def _newest(cls, m):
        return cls._sample(m, (int(m[3]) - 1) & (RING - 1))

    def step(self, tracker, clock_us=None):
        trk, memo = tracker, self.memo
        S, T, max_events = self.n_streams, self.max_tracks, self.max_events
        if len(trk.frame) != S or trk.hits.shape != (S, T):
            raise ValueError('the tracker has other streams or slots than the memo')
        if clock_us is not None:
            clock_us = np.asarray(clock_us)
            if clock_us.dtype != np.int64 or clock_us.shape != (S,):
                raise ValueError('clock_us must be int64 [%d]' % S)
        speed_i = np.zeros((S, T, ROW_COLS), np.int32)
        speed_ev = np.zeros((S, max_events, EV_COLS), np.int32)
        speed_count = np.zeros(S, np.int32)
        for s in range(S):
            plane = self.ground.planes_np[s]
            now, n_ev = int(trk.frame[s]), 0
            base = None if clock_us is None else int(clock_us[s])

            def emit(*line):
                nonlocal n_ev
                if n_ev < max_events:
                    speed_ev[s, n_ev] = line
                n_ev += 1

            for t in range(T):
                m = memo[s, t]
                hits, tid, last = int(trk.hits[s, t]), int(trk.id[s, t]), int(trk.last[s, t])
                eligible = plane is not None and hits > 0 and hits >= self.min_hits                      # 1
                if m[0] != 0 and (not eligible or m[0] != _w32(tid + 1)):                               # 2
                    if m[2] >= 2:
                        tn, xn, yn = self._newest(m)
                        dt, aux = _w64(tn - _join(m[4], m[5])), 0
                        if dt > 0:
                            aux = estimate(xn - int(m[6]), yn - int(m[7]), dt)[0]
                        emit(KIND_ENDED, 0, _w32(int(m[0]) - 1), t, int(m[1]), int(m[11]), xn, yn, 0, 0, 0, aux)
                    m[:] = 0
                if not eligible:
                    speed_i[s, t] = NO_ROW
                    continue
                fresh, estimated = False, False
                started = m[0] == 0
                if started or last != m[1]:                                                             # 3, 4
                    if started:
                        m[0], m[8] = _w32(tid + 1), -1
                    m[1] = last
                    valid, X, Y = world_point(plane['H'], *anchor_of(trk.box[s, t]))
                    if valid:
                        tt = sample_time(now, last, plane['period_us'], base)
                        if m[2] == 0 or _w64(tt - self._newest(m)[0]) >= plane['min_gap_us']:
                            lo, hi = _split(tt)
                            if m[2] == 0:
                                m[4:8] = (lo, hi, int(X), int(Y))
                            head = int(m[3])
                            m[16 + 4 * head:20 + 4 * head] = (lo, hi, int(X), int(Y))
                            m[3], m[2] = (head + 1) & (RING - 1), min(int(m[2]) + 1, I32_MAX)
                            fresh = True
                n = min(int(m[2]), RING)
                if fresh and n >= 2:                                                                    # 5
                    to, xo, yo = self._sample(m, int(m[3]) if m[2] >= RING else 0)
                    te, xe, ye = self._newest(m)
                    dt = _w64(te - to)
                    if dt >= plane['min_span_us']:
                        m[8], m[9], m[10], m[13] = estimate(xe - xo, ye - yo, dt)
                        m[11] = max(int(m[11]), int(m[8]))
                        estimated = True
                over, alerted = int(m[12]) & 0xFFFF, int(m[12]) >> 16 & 1
                if estimated and plane['limit_mm_s'] > 0:                                               # 6
                    if m[8] > plane['limit_mm_s']:
                        over = min(over + 1, 0xFFFF)
                        if over >= self.confirm and not alerted:
                            _, xn, yn = self._newest(m)
                            key = read_key(trk.read(s, t)[0])
                            emit(KIND_ALERT, 0, tid, t, last, int(m[8]), xn, yn, key[0], key[1], hits, plane['limit_mm_s'])
                            alerted = 1
                    else:
                        over = 0
                    m[12] = over | alerted << 16
                xn, yn = self._newest(m)[1:] if n else (0, 0)
                speed_i[s, t] = (tid, m[8], m[9], m[10], xn, yn, m[13], n | int(fresh) << 8 | alerted << 9)     # 7
            speed_count[s] = n_ev
        return speed_i, speed_ev, speed_count
