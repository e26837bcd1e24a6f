"""Tripwires and zones on live plate tracks -- line crossings with a direction, zone entry and exit, dwell alerts, occupancy and
in / out counts -- on the CPU: ``ZoneEventsNp`` is the written-down specification of ``lp_zone_update`` (include/lp_hip.h,
csrc/lp_zones.hip), which matches it on every int32, and the CPU path of ``Inferer(track=True, zones=...)``.

The reference has nothing here: its Inferer treats frames independently (yolov6/core/inferer.py).

The tracker, the watchlists and the sightings log say WHICH plate; a gate, a car park or a street also asks which way it went
and how long it has been there.  A camera that sees both lanes cannot tell an arrival from a departure without a directed line, and
a false detection on a sign outside the lane counts like a plate unless a region says where plates count.

Geometry of one stream, in pixels of its frames, fp32, all values finite: up to ``MAX_LINES`` directed segments A -> B and up to
``MAX_ZONES`` simple polygons of 3..``MAX_VERTS`` vertices (convex or not), each zone with an int ``min_dwell`` >= 0 (0: no dwell
alert).  ``ZoneMapNp`` validates and packs it (``MAP_WORDS`` int32 words per stream, the layout ``lp_zone_update`` takes):
  words 0, 1: n_lines, n_zones; 2..15: 0; 16 + 4 l ..: line l as fp32 bits ax, ay, bx, by; 80 + 4 z ..: zone z as n_verts,
  min_dwell, 0, 0; 112 + 32 z + 2 v ..: vertex v of zone z as fp32 bits x, y.  Lines, zones and vertices past their counts are 0.

Arithmetic.  A point or vertex is widened from fp32 to fp64; every later operation is one IEEE fp64 subtract or multiply, rounded
on its own, in the written order: no fused multiply-add, no division.
  cross(P, Q, R) = (Qx - Px) * (Ry - Py) - (Qy - Py) * (Rx - Px).
Every comparison is a plain float compare, false for NaN.
Anchor of a slot: ((x1 + x2) * 0.5f, (y1 + y2) * 0.5f) of the stored box in fp32: the tracker's own cx, cy.  An anchor is finite iff
|x| <= FLT_MAX and |y| <= FLT_MAX; an anchor that is not finite crosses no line (at either end of the move) and is inside no zone.
Crossing of line l by the move P0 -> P1: d0 = cross(A, B, P0), d1 = cross(A, B, P1); the direction is +1 iff d0 <= 0 and d1 > 0, -1
iff d0 > 0 and d1 <= 0 (a point on the line belongs to the negative side, so that a stop on the line is counted once); the move
counts only if it also passes between the ends: e0 = cross(P0, P1, A), e1 = cross(P0, P1, B), (e0 <= 0 and e1 > 0) or (e0 > 0 and
e1 <= 0).
Inside a zone: the crossing number over the edges (Vi, Vj), j = (i + 1) % n: an edge toggles iff (yi > py) != (yj > py) and, with
t = (xj - xi) * (py - yi) - (px - xi) * (yj - yi), t > 0 if yj > yi, else t < 0.

Memo: int32 [S, T + 2, 16], all zero = empty.  Row t < T, one per slot: id + 1, last (the track's last matched frame when the
anchor was taken), the anchor's x and y as fp32 bits, inside_mask | alerted_mask << 8, enter_frame[8], 0, 0, 0.  Row T: the +1
totals per line, row T + 1: the -1 totals; both wrap as int32.

Steps.  They run after an ``update`` call, on the tracker state as that call left it.  Every stream is processed, whether or not it
had a frame in the call; the slots go in ascending order; ``now`` is the stream's frame counter as the call left it:
  1. a slot is eligible iff it is live (hits > 0) and hits >= min_hits;
  2. a non-empty memo line whose slot is not eligible, or holds another id, is GONE: for every zone of its inside mask, ascending,
     it emits kind 5 (ended inside) with frame = memo.last, value = memo.last - enter_frame[z], the memo's anchor, key 0 and hits
     0; then the line is zeroed;
  3. an eligible slot with an empty memo line starts a track: the anchor is the current one, no crossing is tested, and every zone
     it is inside emits kind 2 (enter) with enter_frame[z] = slot.last;
  4. an eligible slot whose memo holds its id: the lines in ascending order, a crossing of memo anchor -> current anchor emits kind 1
     with value +1 / -1 and that line's total of that direction goes up by one; then the zones in ascending order: outside ->
     inside emits kind 2, sets enter_frame[z] = slot.last and clears the zone's alerted bit; inside -> outside emits kind 3 (left)
     with value = slot.last - enter_frame[z].  The memo then takes the new anchor, last and inside mask;
  5. behind each zone's transition in 3 and 4: iff the track is inside z, min_dwell[z] > 0, the alerted bit is clear and
     now - enter_frame[z] >= min_dwell[z], kind 4 (dwell) with value = now - enter_frame[z], and the bit is set.  A missed but live
     track keeps dwelling;
  6. an event line is int32 [12]: kind, the line or zone index, id, slot, frame (slot.last for kinds 1..4), value, the anchor's x
     and y as fp32 bits, key_lo, key_hi (the eight voted ids of rule 8 of ``yolov6.utils.track`` packed by
     ``watch_live.read_key``; 0 for kind 5), hits, 0;
  7. zone_ev [S, max_events, 12]: a stream's events in the order produced (by slot; within a slot step 2, the lines, then the zones
     with each transition followed by its alert); zone_count [S]: the number produced, not capped -- lines at or past max_events
     are not written, lines from the count to max_events are zero; zone_occ [S, 8]: the eligible tracks inside each zone after the
     call; zone_totals [S, 2, 16]: a copy of the two total rows.  Every word of the four is written by every call.
The int32 differences wrap.

``reset(streams)`` zeroes those streams' memo, totals included, without events; a flush ends the tracks, so that step 2 reports
them; enabling again zeroes everything.

What it does not do: positions are those at the end of a call -- a stream with several frames in one call is tested on the chord,
and a track born and ended inside one call is unseen; a track that touches a line and turns back yields +1 then -1; a track that
ends inside a zone is kind 5, not kind 3; lines and zones stay in pixels (the speed on a calibrated ground plane is
``yolov6.utils.speed`` / ``enable_speed``); the anchor is the plate, not the vehicle's footprint (``yolov6.utils.scene`` draws the lines and zones).
"""
import os

import numpy as np

from yolov6.utils.watch_live import check_min_hits, read_key

MAX_LINES, MAX_ZONES, MAX_VERTS = 16, 8, 16
MEMO_COLS, EV_COLS = 16, 12
MAP_HDR, MAP_LINES, MAP_ZHDR, MAP_VERTS = 0, 16, 80, 112
MAP_WORDS = MAP_VERTS + MAX_ZONES * MAX_VERTS * 2          # 368
KIND_CROSS, KIND_ENTER, KIND_LEFT, KIND_DWELL, KIND_ENDED = 1, 2, 3, 4, 5
EVENT_NAMES = {KIND_ENTER: 'enter', KIND_LEFT: 'left', KIND_DWELL: 'dwell', KIND_ENDED: 'ended'}
FLT_MAX = np.float32(3.4028234663852886e38)
f32, f64 = np.float32, np.float64


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------
def cross(px, py, qx, qy, rx, ry):
    """cross(P, Q, R) in fp64, op by op; scalars or arrays that broadcast."""
    px, py, qx, qy, rx, ry = (np.asarray(v, f64) for v in (px, py, qx, qy, rx, ry))
    with np.errstate(all='ignore'):
        return (qx - px) * (ry - py) - (qy - py) * (rx - px)


def finite_point(x, y):
    """Both coordinates (fp32) are finite: |v| <= FLT_MAX, false for NaN."""
    with np.errstate(all='ignore'):
        return (np.abs(np.asarray(x, f32)) <= FLT_MAX) & (np.abs(np.asarray(y, f32)) <= FLT_MAX)


def crossing_dir(ax, ay, bx, by, p0x, p0y, p1x, p1y):
    """+1, -1 or 0: the crossing of the line A -> B by the move P0 -> P1 (arrays broadcast; int32)."""
    d0, d1 = cross(ax, ay, bx, by, p0x, p0y), cross(ax, ay, bx, by, p1x, p1y)
    e0, e1 = cross(p0x, p0y, p1x, p1y, ax, ay), cross(p0x, p0y, p1x, p1y, bx, by)
    between = ((e0 <= 0) & (e1 > 0)) | ((e0 > 0) & (e1 <= 0))
    ok = between & finite_point(p0x, p0y) & finite_point(p1x, p1y)
    up, down = (d0 <= 0) & (d1 > 0), (d0 > 0) & (d1 <= 0)
    return np.where(ok, up.astype(np.int32) - down.astype(np.int32), 0).astype(np.int32)


def _toggles(xi, yi, xj, yj, px, py):
    xi, yi, xj, yj, px, py = (np.asarray(v, f64) for v in (xi, yi, xj, yj, px, py))
    with np.errstate(all='ignore'):
        t = (xj - xi) * (py - yi) - (px - xi) * (yj - yi)
    return ((yi > py) != (yj > py)) & np.where(yj > yi, t > 0, t < 0)


def inside_zone(verts, px, py):
    """The point (px, py) is inside the polygon ``verts`` [n, 2]: the crossing number of the module's rule."""
    v = np.asarray(verts, f64).reshape(-1, 2)
    w = np.roll(v, -1, axis=0)
    return bool(_toggles(v[:, 0], v[:, 1], w[:, 0], w[:, 1], px, py).sum() & 1) and bool(finite_point(px, py))


def anchor_of(box):
    """(x, y) fp32 of a stored box [4] fp32."""
    b = np.asarray(box, f32)
    with np.errstate(all='ignore'):
        return (b[0] + b[2]) * f32(0.5), (b[1] + b[3]) * f32(0.5)


def _bits(v):
    return int(np.asarray(v, f32).reshape(1).view(np.int32)[0])


def _wrap(v):
    """An integer as int32, wrapping."""
    return int(np.int64(v).astype(np.int32))


# ---- the geometry ------------------------------------------------------------------------------------------------------------
def _per_stream(items, n_streams, what):
    if items is None:
        return [[] for _ in range(n_streams)]
    if isinstance(items, dict):
        for s in items:
            if not 0 <= int(s) < n_streams:
                raise ValueError('%s of stream %s: need a stream in 0..%d' % (what, s, n_streams - 1))
        return [list(items.get(s, [])) for s in range(n_streams)]
    items = list(items)
    if len(items) != n_streams:
        raise ValueError('%s must have one list per stream (%d), or be a dict by stream' % (what, n_streams))
    return [list(v) for v in items]


class ZoneMapNp:
    """The lines and zones of ``n_streams`` streams, validated and packed (the module docstring states the layout).
    ``lines``: one list per stream (or a dict by stream, or None) of (x1, y1, x2, y2), the segment A = (x1, y1) -> B = (x2, y2);
    ``zones``: one list per stream (or a dict, or None) of (vertices [n, 2], min_dwell) pairs, or of bare vertex lists (min_dwell
    0).  ``lines_np`` / ``zones_np``: the checked copies, per stream an fp32 [L, 4] array and a list of (fp32 [n, 2], int);
    ``packed``: int32 [S, MAP_WORDS].  ValueError for more than 16 lines, 8 zones, fewer than 3 or more than 16 vertices, a value
    that is not finite in fp32 and a negative dwell."""

    def __init__(self, n_streams, lines=None, zones=None, device=None):
        S = int(n_streams)
        if S < 1:
            raise ValueError('n_streams must be >= 1')
        self.n_streams = S
        self.lines_np, self.zones_np = [], []
        for s, ls in enumerate(_per_stream(lines, S, 'lines')):
            if len(ls) > MAX_LINES:
                raise ValueError('stream %d: %d lines, at most %d' % (s, len(ls), MAX_LINES))
            a = np.asarray(ls, f64).reshape(-1, 4) if len(ls) else np.zeros((0, 4), f64)
            self.lines_np.append(self._finite(a, 'line', s))
        for s, zs in enumerate(_per_stream(zones, S, 'zones')):
            if len(zs) > MAX_ZONES:
                raise ValueError('stream %d: %d zones, at most %d' % (s, len(zs), MAX_ZONES))
            out = []
            for z in zs:
                verts, dwell = (z[0], z[1]) if len(z) == 2 and np.ndim(z[0]) == 2 else (z, 0)
                v = np.asarray(verts, f64)
                if v.ndim != 2 or v.shape[1] != 2 or not 3 <= len(v) <= MAX_VERTS:
                    raise ValueError('stream %d: a zone needs 3..%d vertices (x, y)' % (s, MAX_VERTS))
                if int(dwell) != dwell or not 0 <= int(dwell) < 2 ** 31:
                    raise ValueError('stream %d: min_dwell must be an integer >= 0' % s)
                out.append((self._finite(v, 'zone', s), int(dwell)))
            self.zones_np.append(out)
        self.packed = np.zeros((S, MAP_WORDS), np.int32)
        for s in range(S):
            p, ls, zs = self.packed[s], self.lines_np[s], self.zones_np[s]
            p[0], p[1] = len(ls), len(zs)
            p[MAP_LINES:MAP_LINES + 4 * len(ls)] = ls.reshape(-1).view(np.int32)
            for z, (v, dwell) in enumerate(zs):
                p[MAP_ZHDR + 4 * z], p[MAP_ZHDR + 4 * z + 1] = len(v), dwell
                p[MAP_VERTS + 32 * z:MAP_VERTS + 32 * z + 2 * len(v)] = v.reshape(-1).view(np.int32)
        check_packed(self.packed)

    @staticmethod
    def _finite(a, what, s):
        with np.errstate(all='ignore'):
            b = a.astype(f32)
        if not np.isfinite(b).all():
            raise ValueError('stream %d: a %s coordinate is not finite in fp32' % (s, what))
        return np.ascontiguousarray(b)


def check_packed(packed):
    """The rules of a packed map int32 [S, MAP_WORDS] (ValueError): counts in range, finite coordinates, dwell >= 0, zero padding."""
    p = np.asarray(packed)
    if p.dtype != np.int32 or p.ndim != 2 or p.shape[1] != MAP_WORDS or p.shape[0] < 1:
        raise ValueError('a packed zone map is int32 [S, %d]' % MAP_WORDS)
    for s in range(p.shape[0]):
        nl, nz = int(p[s, 0]), int(p[s, 1])
        if not (0 <= nl <= MAX_LINES and 0 <= nz <= MAX_ZONES) or p[s, 2:MAP_LINES].any() or p[s, MAP_LINES + 4 * nl:MAP_ZHDR].any():
            raise ValueError('stream %d: bad line / zone counts or padding' % s)
        ok = np.isfinite(p[s, MAP_LINES:MAP_ZHDR].view(f32)).all()
        for z in range(MAX_ZONES):
            n, dwell, pad = int(p[s, MAP_ZHDR + 4 * z]), int(p[s, MAP_ZHDR + 4 * z + 1]), p[s, MAP_ZHDR + 4 * z + 2:MAP_ZHDR + 4 * z + 4]
            v = p[s, MAP_VERTS + 32 * z:MAP_VERTS + 32 * z + 32]
            if z < nz:
                ok = ok and 3 <= n <= MAX_VERTS and dwell >= 0 and not pad.any() and not v[2 * n:].any() and np.isfinite(v.view(f32)).all()
            else:
                ok = ok and n == 0 and dwell == 0 and not pad.any() and not v.any()
        if not ok:
            raise ValueError('stream %d: bad zone header, vertex or padding' % s)


def parse_zones(text_or_path, n_streams=1):
    """Read the text format, one item per line, ``#`` starts a comment:
        [S:] line NAME x1 y1 x2 y2
        [S:] zone NAME [dwell=N] x1 y1 x2 y2 x3 y3 ...
    ``S:`` is the stream (default 0).  Returns (lines, zones, line_names, zone_names): per stream the lists ``ZoneMapNp`` takes and
    the names in index order.  ``text_or_path``: the text itself (it has a newline or starts with an item) or a file's path."""
    text = str(text_or_path)
    if '\n' not in text and os.path.exists(text):
        with open(text) as f:
            text = f.read()
    S = int(n_streams)
    lines, zones = [[] for _ in range(S)], [[] for _ in range(S)]
    line_names, zone_names = [[] for _ in range(S)], [[] for _ in range(S)]
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
        if len(tok) < 2 or tok[0] not in ('line', 'zone'):
            raise ValueError('line %d: expected `line NAME x1 y1 x2 y2` or `zone NAME [dwell=N] x1 y1 ...`' % no)
        kind, name, rest = tok[0], tok[1], tok[2:]
        dwell = 0
        if kind == 'zone' and rest and rest[0].startswith('dwell='):
            try:
                dwell = int(rest[0][6:])
            except ValueError:
                raise ValueError('line %d: bad %r' % (no, rest[0]))
            rest = rest[1:]
        try:
            vals = [float(v) for v in rest]
        except ValueError:
            raise ValueError('line %d: bad number' % no)
        if kind == 'line':
            if len(vals) != 4:
                raise ValueError('line %d: a line has four numbers' % no)
            lines[s].append(tuple(vals))
            line_names[s].append(name)
        else:
            if len(vals) % 2 or len(vals) < 6:
                raise ValueError('line %d: a zone has at least three x y pairs' % no)
            zones[s].append((np.asarray(vals, f64).reshape(-1, 2), dwell))
            zone_names[s].append(name)
    return lines, zones, line_names, zone_names


def format_zones(zone_map, line_names=None, zone_names=None):
    """The text of a map (anything with ``lines_np`` / ``zones_np``) that ``parse_zones`` reads back to the same map."""
    out = []
    for s in range(zone_map.n_streams):
        for l, a in enumerate(zone_map.lines_np[s]):
            out.append('%d: line %s %s' % (s, line_names[s][l] if line_names else 'L%d' % l, ' '.join(repr(float(v)) for v in a)))
        for z, (v, dwell) in enumerate(zone_map.zones_np[s]):
            out.append('%d: zone %s dwell=%d %s' % (s, zone_names[s][z] if zone_names else 'Z%d' % z, dwell,
                                                   ' '.join(repr(float(c)) for c in v.reshape(-1))))
    return '\n'.join(out) + '\n'


# ---- the steps ---------------------------------------------------------------------------------------------------------------
class ZoneEventsNp:
    """The memo of one tracker (a ``PlateTrackerNp``) and the steps of the module's rule.  ``zone_map``: anything with
    ``n_streams``, ``lines_np`` and ``zones_np`` (``ZoneMapNp``, ``runtime.ZoneMap``).  ``step(max_events)`` after an ``update``
    returns (zone_ev, zone_count, zone_occ, zone_totals)."""

    def __init__(self, tracker, zone_map, min_hits=1):
        if zone_map.n_streams != tracker.n_streams:
            raise ValueError('the zone map has %d streams, the tracker %d' % (zone_map.n_streams, tracker.n_streams))
        self.tracker, self.zone_map, self.min_hits = tracker, zone_map, check_min_hits(min_hits)
        self.memo = np.zeros((tracker.n_streams, tracker.max_tracks + 2, MEMO_COLS), np.int32)
        self._geo = []
        for s in range(tracker.n_streams):
            ls = np.asarray(zone_map.lines_np[s], f32).reshape(-1, 4).astype(f64)
            zs = [(np.asarray(v, f32).astype(f64), np.roll(np.asarray(v, f32).astype(f64), -1, axis=0), int(d)) for v, d in zone_map.zones_np[s]]
            self._geo.append((ls, zs))

    def reset(self, streams=None):
        """Zero the memo of ``streams`` (all for None), totals included."""
        for s in (range(self.tracker.n_streams) if streams is None else streams):
            self.memo[int(s)] = 0

    def _inside_mask(self, s, ax, ay):
        mask = 0
        if finite_point(ax, ay):
            for z, (v, w, _) in enumerate(self._geo[s][1]):
                if int(_toggles(v[:, 0], v[:, 1], w[:, 0], w[:, 1], ax, ay).sum()) & 1:
                    mask |= 1 << z
        return mask

    def step(self, max_events):
        trk, memo = self.tracker, self.memo
        S, T, max_events = trk.n_streams, trk.max_tracks, int(max_events)
        if max_events < 0:
            raise ValueError('max_events must be >= 0')
        zone_ev = np.zeros((S, max_events, EV_COLS), np.int32)
        zone_count, zone_occ = np.zeros(S, np.int32), np.zeros((S, MAX_ZONES), np.int32)
        for s in range(S):
            ls, zs = self._geo[s]
            now, n = int(trk.frame[s]), 0

            def emit(kind, index, track_id, t, frame, value, ax_bits, ay_bits, key, hits):
                nonlocal n
                if n < max_events:
                    zone_ev[s, n] = (kind, index, track_id, t, frame, _wrap(value), ax_bits, ay_bits, key[0], key[1], hits, 0)
                n += 1

            for t in range(T):
                m = memo[s, t]
                hits, tid, last = int(trk.hits[s, t]), int(trk.id[s, t]), int(trk.last[s, t])
                eligible = hits > 0 and hits >= self.min_hits                                        # 1
                if m[0] != 0 and (not eligible or m[0] != tid + 1):                                  # 2
                    for z in range(MAX_ZONES):
                        if int(m[4]) >> z & 1:
                            emit(KIND_ENDED, z, int(m[0]) - 1, t, int(m[1]), int(m[1]) - int(m[5 + z]), int(m[2]), int(m[3]), (0, 0), 0)
                    m[:] = 0
                if not eligible:
                    continue
                ax, ay = anchor_of(trk.box[s, t])
                axb, ayb = _bits(ax), _bits(ay)
                key = None

                def ev(kind, index, value):
                    nonlocal key
                    if key is None:
                        key = read_key(trk.read(s, t)[0])
                    emit(kind, index, tid, t, last, value, axb, ayb, key, hits)

                new = m[0] == 0
                old_inside = 0 if new else int(m[4]) & 0xFF
                alerted = 0 if new else int(m[4]) >> 8 & 0xFF
                enter = [0] * MAX_ZONES if new else [int(v) for v in m[5:13]]
                if not new and len(ls):                                                              # 4: the lines
                    px, py = m[2:3].view(f32)[0], m[3:4].view(f32)[0]
                    d = crossing_dir(ls[:, 0], ls[:, 1], ls[:, 2], ls[:, 3], px, py, ax, ay)
                    for l in np.nonzero(d)[0]:
                        ev(KIND_CROSS, int(l), int(d[l]))
                        row = memo[s, T if d[l] > 0 else T + 1]
                        row[l] = _wrap(int(row[l]) + 1)
                inside = self._inside_mask(s, ax, ay)
                for z, (_, _, dwell) in enumerate(zs):                                               # 3, 4: the zones; 5
                    bit = 1 << z
                    if inside & bit and not old_inside & bit:
                        enter[z] = last
                        alerted &= ~bit
                        ev(KIND_ENTER, z, 0)
                    elif old_inside & bit and not inside & bit:
                        ev(KIND_LEFT, z, last - enter[z])
                    if inside & bit and dwell > 0 and not alerted & bit and _wrap(now - enter[z]) >= dwell:
                        ev(KIND_DWELL, z, now - enter[z])
                        alerted |= bit
                    if inside & bit:
                        zone_occ[s, z] += 1
                m[:] = [tid + 1, last, axb, ayb, inside | alerted << 8] + [_wrap(v) for v in enter] + [0, 0, 0]
            zone_count[s] = n
        zone_totals = memo[:, T:T + 2, :].copy()
        return zone_ev, zone_count, zone_occ, zone_totals
