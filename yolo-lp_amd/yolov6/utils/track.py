"""Plate tracking across video frames with a per-track vote over the eight character heads, on the CPU:
``PlateTrackerNp`` is the written-down specification of ``lp_track_update`` (include/lp_hip.h, csrc/lp_track.hip), which
matches it bit for bit, and the CPU path of ``Inferer(track=True)``.  Everything is fp32, evaluated op by op in the kernel's
order (no fused multiply-add).

The reference has nothing here: its Inferer treats video frames independently (yolov6/core/inferer.py).

Rules, per frame of one stream (``det`` [max_det, 28] and ``count`` as lp_nms / lp_rescale_round_batch leave them; only the first
n = min(max(count, 0), max_det, MAX_DETS) rows take part):
  1. predict: every live slot's box is shifted by (vx * k, vy * k), k = (float)(misses + 1); product rounded, then the add;
  2. expand: the predicted box and every detection box grow by e = (float)expand * w on both sides in x, likewise in y;
  3. pairs: IoU of every (live slot, row) on the expanded boxes with the fp32 ops of ``yolov6.utils.tiles.overlaps`` ('iou');
     a pair exists iff (double)iou > match_thres.  The pairs are ordered by ``tiles._sort_keys(iou, slot * 128 + row)``
     (descending IoU, ties by slot, then row) and taken greedily while slot and row are both free;
  4. a matched slot: vx = (cx_new - cx_old) / k with cx = (x1 + x2) * 0.5f on the stored (unexpanded) box, vy likewise; box and
     corners become the row's columns 0..11; hits += 1, misses = 0, last = frame; it votes (7);
  5. an unmatched live slot: misses += 1; misses > max_age ends the track (its record is appended to the stream's ended list,
     the slot is freed: all-zero), in ascending slot order;
  6. unmatched rows in row order: score = (c12 + ... + c19) / 8.0f summed left to right (nms.py:120); with
     (double)score >= new_thres the lowest free slot (those freed in 5 included) becomes a new track: id = next_id++,
     first = last = frame, hits = 1, misses = 0, zero velocity, zero votes, then it votes.  No free slot: the row stays
     untracked and the stream's ``dropped`` counter goes up;
  7. vote, per head p: v = c[20 + p], conf = c[12 + p]; iff conf > 0 and 0 <= v < ncls[p] (float compares: false for NaN):
     votes[p][(int)v] += conf, total[p] += conf;
  8. read of a track: best_p = first index of the largest votes[p][0 .. ncls[p]) (0 for an all-zero head),
     share_p = votes[p][best_p] / total[p] if total[p] > 0 else 0;
  9. outputs: tid[r] = the track id of a matched or new row, -1 for every other r < max_det; det_out[r] = the row with columns
     12..19 replaced by the track's shares and 20..27 by (float)best_p, read after this frame's vote; other rows below
     min(max(count, 0), max_det) are copied, rows at or past it are zero;
 10. the stream's frame counter goes up.
 11. hold (``enable_hold(min_hits, max_misses)``, lp_track_update_hold; read-only on the state, for redaction): a slot is held in
     a frame iff it was live at the start of the frame, was not matched, did not end in it, has hits >= min_hits and, after
     the increment of 5, misses <= max_misses.  Its held row: k = (float)misses, dx = vx * k, dy = vy * k (the k and the
     products of step 1 of this frame); columns 0..3 = the stored box + (dx, dy, dx, dy): the box step 1 predicted before the
     expansion; columns 4..11 = the stored corners, x columns + dx and y columns + dy; columns 12..19 the track's shares and
     20..27 its voted ids (8).  Per frame, with nc = min(max(count, 0), max_det): det_hold [max_det + max_tracks, 28] = the nc
     rows of det_out, then the held rows in slot order, then zero rows; count_hold = nc + the number of held rows; tid_hold
     [max_det + max_tracks] = tid for the first nc rows, the track id for held rows, -1 elsewhere.  A frame that is not tracked
     has no held row.  (det_hold, count_hold) is the layout ``redact_plates`` takes.
"""
import numpy as np

from yolov6.utils.tiles import _sort_keys

DET_COLS = 28
MAX_TRACKS = 128          # LP_TRACK_MAX_TRACKS: slots per stream
MAX_DETS = 128            # LP_TRACK_MAX_DETS: rows of a frame that take part (128 x 128 pair keys are sorted in LDS)
MAX_CLS = 64              # LP_TRACK_MAX_CLS: classes per head
HEADS = 8
ENDED_COLS = 12           # ended_i: id, first, last, hits, best_0..7; ended_f: share_0..7, x1, y1, x2, y2
DEFAULT_NCLS = (31, 24, 37, 37, 37, 37, 37, 37)
f32 = np.float32


def ncls_of(model=None):
    """The eight head widths (npro, nalp, nads x 6): of a model (its ``detect`` head), a sequence of eight, or the shipped
    configs' (31, 24, 37, ...) for None."""
    if model is None:
        return DEFAULT_NCLS
    if isinstance(model, (tuple, list, np.ndarray)):
        out = tuple(int(v) for v in model)
    else:
        head = getattr(model, 'detect', None)
        if head is None:
            head = getattr(getattr(model, 'model', None), 'detect', None)
        if head is None:
            raise ValueError('ncls: expected eight widths or a model with a detect head')
        out = (int(head.npro), int(head.nalp)) + (int(head.nads),) * 6
    if len(out) != HEADS or not all(1 <= v <= MAX_CLS for v in out):
        raise ValueError('ncls must be eight widths in 1..%d' % MAX_CLS)
    return out


def check_params(n_streams, max_tracks, match_thres, new_thres, expand, max_age):
    """The argument rules of lp_track_update's parameters (ValueError)."""
    if int(n_streams) < 1:
        raise ValueError('n_streams must be >= 1')
    if not 1 <= int(max_tracks) <= MAX_TRACKS:
        raise ValueError('max_tracks must be in 1..%d' % MAX_TRACKS)
    if not 0.0 <= match_thres <= 1.0:
        raise ValueError('match_thres must be in [0, 1]')
    if not abs(new_thres) <= 3.0e38:
        raise ValueError('new_thres must be finite (|new_thres| <= 3e38)')
    if not 0.0 <= expand <= 1.0e6:
        raise ValueError('expand must be in [0, 1e6]')
    if int(max_age) < 0:
        raise ValueError('max_age must be >= 0')


def check_call(n_streams, B, stream_of, flush, max_ended):
    """(stream_of list [B], flush list [n_streams], max_ended) of one update call, checked."""
    stream_of = list(range(B)) if stream_of is None else [int(v) for v in stream_of]
    if len(stream_of) != B:
        raise ValueError('stream_of must name the stream of each of the %d frames' % B)
    for b, s in enumerate(stream_of):
        if not -1 <= s < n_streams:
            raise ValueError('stream %d of frame %d: need -1 (skip) or 0..%d' % (s, b, n_streams - 1))
    flush = [0] * n_streams if flush is None else [int(bool(v)) for v in flush]
    if len(flush) != n_streams:
        raise ValueError('flush must have one entry per stream')
    if int(max_ended) < 0:
        raise ValueError('max_ended must be >= 0')
    return stream_of, flush, int(max_ended)


def expand_boxes(box, e):
    """Boxes [..., 4] fp32 grown by e * width on both sides in x and e * height in y (``e`` fp32)."""
    box = np.asarray(box, f32)
    with np.errstate(all='ignore'):
        ex = e * (box[..., 2] - box[..., 0])
        ey = e * (box[..., 3] - box[..., 1])
        out = np.stack([box[..., 0] - ex, box[..., 1] - ey, box[..., 2] + ex, box[..., 3] + ey], -1)
    assert out.dtype == f32
    return out


def iou_matrix(a, b):
    """fp32 [K, N]: inter / (area_i + area_j - inter) of boxes a [K,4] (i) and b [N,4] (j), the ops of ``tiles.overlaps``
    ('iou') in its order; the quotient itself, which is a sort key here."""
    a, b = np.asarray(a, f32).reshape(-1, 4), np.asarray(b, f32).reshape(-1, 4)
    ix1, iy1, ix2, iy2 = (a[:, k][:, None] for k in range(4))
    jx1, jy1, jx2, jy2 = (b[:, k][None, :] for k in range(4))
    with np.errstate(all='ignore'):
        xx1 = np.where(ix1 > jx1, ix1, jx1)
        yy1 = np.where(iy1 > jy1, iy1, jy1)
        xx2 = np.where(ix2 < jx2, ix2, jx2)
        yy2 = np.where(iy2 < jy2, iy2, jy2)
        w = xx2 - xx1
        w = np.where(w > 0, w, f32(0))
        h = yy2 - yy1
        h = np.where(h > 0, h, f32(0))
        inter = w * h
        iarea = (ix2 - ix1) * (iy2 - iy1)
        jarea = (jx2 - jx1) * (jy2 - jy1)
        ovr = inter / (iarea + jarea - inter)
    assert ovr.dtype == f32
    return ovr


def predict_boxes(box, vel, k):
    """Rule 1: boxes [..., 4] shifted by (vx * k, vy * k) of ``vel`` [..., 2]; the products are rounded, then the adds."""
    with np.errstate(all='ignore'):
        dx, dy = vel[..., 0] * k, vel[..., 1] * k
        return np.stack([box[..., 0] + dx, box[..., 1] + dy, box[..., 2] + dx, box[..., 3] + dy], -1)


def held_geometry(box, cor, vel, k):
    """Rule 11: (box [4], corners [8]) of a held row: dx = vx * k, dy = vy * k (products rounded), then the adds."""
    with np.errstate(all='ignore'):
        d = np.array([vel[0] * k, vel[1] * k], f32)
        return box + np.tile(d, 2), cor + np.tile(d, 4)


def centre_velocity(new, old, k):
    """Rule 4: (vx, vy) [..., 2] = the move of the centre (x1 + x2) * 0.5f, (y1 + y2) * 0.5f from box ``old`` to ``new`` [..., 4],
    divided by ``k``."""
    with np.errstate(all='ignore'):
        return np.stack([((new[..., 0] + new[..., 2]) * f32(0.5) - (old[..., 0] + old[..., 2]) * f32(0.5)) / k,
                         ((new[..., 1] + new[..., 3]) * f32(0.5) - (old[..., 1] + old[..., 3]) * f32(0.5)) / k], -1)


def new_score(row):
    """Rule 6: (c12 + ... + c19) / 8.0f of a row, summed left to right."""
    with np.errstate(all='ignore'):
        score = row[12] + row[13]
        for c in range(14, 20):
            score = score + row[c]
        return score / f32(8.0)


def over_threshold(iou, thres):
    """Rule 3: (double)iou > thres of fp32 IoUs and a Python float."""
    return iou.astype(np.float64) > thres


def vote_share(v, tot):
    """Rule 8: votes / total, one fp32 division."""
    return v / tot


def plate_text(ids, pro_names=None, alp_names=None, ads_names=None):
    """The plate string of eight head ids (province, alphabet, six characters) with the three name lists of a data yaml
    (``names`` / ``alps`` / ``ads``); without names, or for an id outside its list, the ids joined by spaces."""
    ids = [int(v) for v in ids]
    if len(ids) != HEADS:
        raise ValueError('plate_text needs eight ids')
    if pro_names and alp_names and ads_names:
        lists = [pro_names, alp_names] + [ads_names] * 6
        if all(0 <= i < len(names) for i, names in zip(ids, lists)):
            return ''.join(str(names[i]) for i, names in zip(ids, lists))
    return ' '.join(str(i) for i in ids)


class PlateTrackerNp:
    """``n_streams`` independent trackers of ``max_tracks`` slots each (the module docstring states the rules).  Same
    constructor and ``update`` as ``yolov6.hip.runtime.PlateTracker``, on numpy arrays; ``device`` is ignored."""

    def __init__(self, n_streams, max_tracks=64, match_thres=0.3, new_thres=0.0, expand=0.5, max_age=5, ncls=None, device=None):
        check_params(n_streams, max_tracks, match_thres, new_thres, expand, max_age)
        self.n_streams, self.max_tracks, self.max_age = int(n_streams), int(max_tracks), int(max_age)
        self.match_thres, self.new_thres, self.expand = float(match_thres), float(new_thres), float(expand)
        self.ncls = ncls_of(ncls)
        S, T = self.n_streams, self.max_tracks
        self.frame = np.zeros(S, np.int32)
        self.next_id = np.zeros(S, np.int32)
        self.dropped = np.zeros(S, np.int32)            # rows that found no free slot, since the last reset
        self.id, self.first, self.last, self.hits, self.misses = (np.zeros((S, T), np.int32) for _ in range(5))
        self.box = np.zeros((S, T, 4), f32)
        self.cor = np.zeros((S, T, 8), f32)
        self.vel = np.zeros((S, T, 2), f32)
        self.votes = np.zeros((S, T, HEADS, MAX_CLS), f32)
        self.total = np.zeros((S, T, HEADS), f32)
        #: counters for tests and diagnostics (no part of the state): pairs above the threshold, pairs sharing their IoU
        #: with another pair of the frame, pairs taken, tracks ended
        self.stats = dict(pairs=0, ties=0, matched=0, ended=0)
        #: int32 [B, max_det] of the last ``update``: the slot of each matched or new row's track, -1 wherever its tid is -1
        #: (the ``slot`` output of lp_track_update_slots)
        self.last_slot = np.zeros((0, 1), np.int32)
        #: int32 [B, max_det] of the last ``update``: the tid it returned (what ``LookbackNp.push`` reads), else None
        self.last_tid = None
        self._hold = None
        #: (det_hold, count_hold, tid_hold) of the last ``update`` after ``enable_hold`` (rule 11), else None
        self.last_hold = None
        self._watch = None
        #: match_i [S, max_ended, 4] int32 of the last ``update`` after ``enable_watch``, line-parallel to its ended_i, else None
        self.last_watch = None
        self._watch_indel = (0, 0)
        #: match_align [S, max_ended] int32 of that lookup after ``enable_watch(..., indel=1)``, else None
        self.last_watch_align = None
        #: live_align [S, max_tracks] int32 of the last ``update`` after ``enable_live_watch(..., indel=1)``, else None
        self.last_live_align = None
        self._stack = None
        #: (stack_crops, stack_i) of the last ``update_stack`` after ``enable_stack``, line-parallel to the ended records, else None
        self.last_stack = None
        self._last_ended = None
        self._live = None
        #: live_i [S, max_tracks, 8] int32 of the last ``update`` after ``enable_live_watch``, else None
        self.last_live = None
        #: (q_i, q_f, q_slot, q_count) of that lookup: the fresh reads in the ended-record layout, else None
        self.last_live_reads = None
        self._sight = None
        #: sight_i [S, max_ended, 8] int32 of the last ``update`` after ``enable_sightings``, line-parallel to its ended_i, else None
        self.last_sight = None
        #: int32 [1]: the clock of ``enable_sightings``, incremented by one per call; the caller may set it
        self.sight_now = np.zeros(1, np.int32)
        self._zones = None
        #: (zone_ev, zone_count, zone_occ, zone_totals) of the last ``update`` after ``enable_zones``, else None
        self.last_zone = None
        self._speed = None
        #: (speed_i, speed_ev, speed_count) of the last ``update`` after ``enable_speed``, else None
        self.last_speed = None
        #: int64 [S]: the clock of ``enable_speed(..., clock=True)`` in microseconds; the caller sets it before every call
        self.speed_clock = np.zeros(S, np.int64)

    _SLOT_ARRAYS = ('id', 'first', 'last', 'hits', 'misses', 'box', 'cor', 'vel', 'votes', 'total')

    def reset(self, streams=None):
        """Zero the state of ``streams`` (all streams for None): no tracks, frame counter, next id and dropped at 0."""
        for s in (range(self.n_streams) if streams is None else streams):
            for name in self._SLOT_ARRAYS + ('frame', 'next_id', 'dropped'):
                getattr(self, name)[s] = 0
        if self._live is not None:
            self._live.reset(streams)
        if self._stack is not None:
            self._stack['np'].reset(streams)
        if self._zones is not None:
            self._zones[0].reset(streams)
        if self._speed is not None:
            self._speed[0].reset(streams)

    def enable_stack(self, search=2, max_frames=64, min_width=0.0, min_sharp=0, crop_hw=(64, 192), max_crops=16, min_score=0.0):
        """One denoised picture per track (``yolov6.utils.stack`` states the rule and its limits): from now on ``update_stack``,
        called right behind an ``update``, aligns and sums the rectified crops of that update's tracks and leaves (stack_crops
        [S, max_ended, Hc, Wc, 3] uint8, stack_i [S, max_ended, 4] int32 = n, first_frame, last_frame, valid) of the tracks it
        ended in ``last_stack``.  The first four arguments are those of ``runtime.PlateTracker.enable_stack``; ``crop_hw``,
        ``max_crops`` and ``min_score`` are what the device tracker shares with its gallery.  Every output of ``update`` and the
        state stay what they are.  Calling it again starts from empty stacks; ``enable_stack(None)`` turns it off."""
        from yolov6.utils.stack import StackNp
        self.last_stack = None
        if search is None:
            self._stack = None
            return
        if int(max_crops) < 1:
            raise ValueError('max_crops must be >= 1')
        self._stack = dict(max_crops=int(max_crops), out={},
                           np=StackNp(self.n_streams, self.max_tracks, crop_hw, search, max_frames, min_score, min_width, min_sharp))

    def update_stack(self, frames, det, count, stream_of=None):
        """The stack stage behind ``update(det, count, stream_of, ...)`` of the same arguments: ``frames[b]`` uint8 [h, w, 3] BGR
        (may be missing or None where ``stream_of`` is -1) is cut along the first ``max_crops`` rows of ``det`` as given.  Returns
        ``last_stack``; stack_crops is persistent per ``max_ended``, the crop of a record without a stack is left as it was."""
        if self._stack is None:
            raise RuntimeError('call enable_stack() first')
        if self._last_ended is None:
            raise RuntimeError('update_stack follows an update')
        sk, (ended_i, ended_count) = self._stack, self._last_ended
        key = ended_i.shape[1]
        buf = sk['out'].get(key)
        if buf is None:
            buf = sk['out'][key] = np.zeros((self.n_streams, key) + sk['np'].crop_hw + (3,), np.uint8)
        self.last_stack = sk['np'].update_from_frames(frames, det, count, self.last_tid, self.last_slot, stream_of, ended_i, ended_count,
                                                      sk['max_crops'], stack_crops=buf)
        return self.last_stack

    def enable_hold(self, min_hits=1, max_misses=None):
        """From now on every ``update`` also fills ``hold_buffers`` (rule 11): the frame's rows followed by a predicted row for
        every track of at least ``min_hits`` hits that the frame missed, for at most ``max_misses`` frames in a row (None, or
        anything above ``max_age``: ``max_age``, where the track ends).  The state and every other output stay what they are."""
        min_hits, max_misses = int(min_hits), self.max_age if max_misses is None else int(max_misses)
        if min_hits < 1 or max_misses < 0:
            raise ValueError('hold needs min_hits >= 1 and max_misses >= 0')
        self._hold = dict(min_hits=min_hits, max_misses=max_misses, out={})

    def enable_watch(self, watchlist, max_mismatch=1, max_cost=None, indel=0, gap_cost=None):
        """From now on every ``update`` / ``flush_all`` also looks the records it ended up in ``watchlist`` -- anything with
        ``entries_np`` and ``confuse_np`` (``watch.WatchlistNp``, ``runtime.Watchlist``) -- and leaves match_i [S, max_ended, 4] int32
        in ``last_watch`` (``yolov6.utils.watch`` states the rule; ``max_cost``: a float in fully confident mismatches, None: no
        limit).  ``indel=1``: one lost or gained character is tolerated at ``gap_cost`` fully confident mismatches (None: 1) and
        match_align [S, max_ended] int32 is left in ``last_watch_align`` (None without it).  Every other output stays what it is.
        ``enable_watch(None)`` turns it off."""
        from yolov6.utils import watch
        self.last_watch = self.last_watch_align = None
        self._watch_indel = watch.check_indel(indel, watch.gap_units(gap_cost))
        self._watch = None if watchlist is None else (watchlist,) + watch.check_params(max_mismatch, watch.cost_units(max_cost))

    def enable_live_watch(self, watchlist, min_hits=3, max_mismatch=1, max_cost=None, indel=0, gap_cost=None):
        """From now on every ``update`` / ``flush_all`` also looks the reads of the LIVE tracks of at least ``min_hits`` hits up in
        ``watchlist``, once per track and voted read (``yolov6.utils.watch_live`` states the rule), and leaves live_i
        [S, max_tracks, 8] int32 in ``last_live`` and the fresh reads (q_i, q_f, q_slot, q_count) in ``last_live_reads``.  Every
        other output and the state stay what they are.  ``indel`` / ``gap_cost`` as ``enable_watch``: live_align [S, max_tracks] int32
        is left in ``last_live_align`` (None without ``indel``).  Calling it again starts from an empty memo;
        ``enable_live_watch(None)`` turns it off."""
        from yolov6.utils.watch_live import LiveWatchNp
        self.last_live = self.last_live_reads = self.last_live_align = None
        self._live = None if watchlist is None else LiveWatchNp(self, watchlist, min_hits, max_mismatch, max_cost, indel, gap_cost)

    def enable_sightings(self, log, window=0, min_hits=1, max_mismatch=1, max_cost=None):
        """From now on every ``update`` / ``flush_all`` also matches the records it ended against the earlier reads in ``log`` (a
        ``sight.SightLogNp`` of the tracker's ``n_streams``) and appends them to it (``yolov6.utils.sight`` states the rule), behind
        the lookups of ``enable_watch`` and ``enable_live_watch``; sight_i [S, max_ended, 8] int32 is left in ``last_sight``.  The
        clock is ``sight_now`` [1]: read by the call, then incremented by one (a caller with a clock of its own sets it before
        every call).  Every other output and the state stay what they are; the log survives ``reset``.
        ``enable_sightings(None)`` turns it off."""
        from yolov6.utils import sight, watch
        self.last_sight = None
        if log is None:
            self._sight = None
            return
        if not isinstance(log, sight.SightLogNp) or log.n_streams != self.n_streams:
            raise ValueError('enable_sightings needs a SightLogNp of %d streams' % self.n_streams)
        _, window, min_hits = sight.check_call(0, window, min_hits)
        self._sight = (log, (window, min_hits) + watch.check_params(max_mismatch, watch.cost_units(max_cost)))

    def enable_zones(self, zone_map, min_hits=1, max_events=None):
        """From now on every ``update`` / ``flush_all`` also tests the live tracks of at least ``min_hits`` hits against the lines and
        zones of ``zone_map`` -- anything with ``n_streams``, ``lines_np`` and ``zones_np`` (``zones.ZoneMapNp``, ``runtime.ZoneMap``)
        -- behind the sightings update (``yolov6.utils.zones`` states the rule), and leaves (zone_ev [S, max_events, 12], zone_count
        [S], zone_occ [S, 8], zone_totals [S, 2, 16]) int32 in ``last_zone``; ``max_events`` defaults to 2 * max_tracks.  Every other
        output and the state stay what they are.  Calling it again starts from an empty memo and zero totals;
        ``enable_zones(None)`` turns it off."""
        from yolov6.utils.zones import ZoneEventsNp
        self.last_zone = None
        if zone_map is None:
            self._zones = None
            return
        max_events = 2 * self.max_tracks if max_events is None else int(max_events)
        if max_events < 0:
            raise ValueError('max_events must be >= 0')
        self._zones = (ZoneEventsNp(self, zone_map, min_hits), max_events)

    def enable_speed(self, ground, min_hits=1, confirm=2, max_events=None, clock=None):
        """From now on every ``update`` / ``flush_all`` also estimates the speed of the live tracks of at least ``min_hits`` hits on the
        calibrated plane of ``ground`` -- anything with ``n_streams`` and ``planes_np`` (``speed.GroundPlaneNp``,
        ``runtime.GroundPlane``) -- behind the zones update (``yolov6.utils.speed`` states the rule), and leaves (speed_i
        [S, max_tracks, 8], speed_ev [S, max_events, 12], speed_count [S]) int32 in ``last_speed``: per slot (id, speed, vx, vy in mm/s,
        X_mm, Y_mm, span_ms, flags), and the alerts (kind 1: over the plane's limit for ``confirm`` estimates in a row, once per track)
        and the ended tracks (kind 3: peak and chord speed); ``max_events`` defaults to ``max_tracks``.  With ``clock`` true the time
        of a stream's newest frame is ``speed_clock`` [S] (int64 microseconds, set by the caller before every call), else the frame
        counter times the plane's period.  Every other output and the state stay what they are.  Calling it again starts from an
        empty memo; ``enable_speed(None)`` turns it off."""
        from yolov6.utils.speed import SpeedNp
        self.last_speed = None
        if ground is None:
            self._speed = None
            return
        if ground.n_streams != self.n_streams:
            raise ValueError('the ground map has %d streams, the tracker %d' % (ground.n_streams, self.n_streams))
        self._speed = (SpeedNp(ground, self.max_tracks, min_hits, confirm, max_events), bool(clock))

    def speed_memo(self):
        """The memo of ``enable_speed``: int32 [S, max_tracks, 48], else None."""
        return None if self._speed is None else self._speed[0].memo

    @property
    def zone_memo(self):
        """The memo of ``enable_zones``: int32 [S, max_tracks + 2, 16], else None."""
        return None if self._zones is None else self._zones[0].memo

    def hold_buffers(self, B, max_det):
        """The persistent (det_hold [B,max_det+max_tracks,28] fp32, count_hold [B] int32, tid_hold [B,max_det+max_tracks] int32)
        an ``update`` of that shape fills after ``enable_hold``."""
        if self._hold is None:
            raise RuntimeError('call enable_hold() first')
        key = (int(B), int(max_det))
        out = self._hold['out'].get(key)
        if out is None:
            rows = key[1] + self.max_tracks
            out = self._hold['out'][key] = (np.zeros((key[0], rows, DET_COLS), f32), np.zeros(key[0], np.int32),
                                            np.full((key[0], rows), -1, np.int32))
        return out

    def _held_rows(self, s, was_live, slot_row):
        """Rule 11 behind step 5 of a frame: [(row [28], track id)] of the held slots of stream ``s``, in slot order."""
        hp, out = self._hold, []
        for t in np.nonzero(was_live)[0]:
            if slot_row[t] >= 0 or self.hits[s, t] < hp['min_hits'] or self.misses[s, t] > hp['max_misses']:
                continue                                  # matched; ended (hits is 0 again); too young; missed for too long
            row = np.zeros(DET_COLS, f32)
            row[0:4], row[4:12] = held_geometry(self.box[s, t], self.cor[s, t], self.vel[s, t], f32(self.misses[s, t]))
            best, share = self.read(s, t)
            row[12:20], row[20:28] = share, best.astype(f32)
            out.append((row, int(self.id[s, t])))
        return out

    def live(self, s):
        """bool [max_tracks]: the live slots of stream ``s``."""
        return self.hits[s] > 0

    def read(self, s, t):
        """(best int32 [8], share fp32 [8]) of slot ``t`` of stream ``s`` (rule 8)."""
        best, share = np.zeros(HEADS, np.int32), np.zeros(HEADS, f32)
        for p in range(HEADS):
            v = self.votes[s, t, p, :self.ncls[p]]
            best[p] = int(np.argmax(v))              # first index of the largest (the votes are never NaN)
            tot = self.total[s, t, p]
            with np.errstate(all='ignore'):
                share[p] = vote_share(v[best[p]], tot) if tot > 0 else f32(0)
        return best, share

    def _add_total(self, s, t, p, conf):
        """Rule 7: total[p] += conf, one fp32 add."""
        self.total[s, t, p] = self.total[s, t, p] + conf

    def _vote(self, s, t, row):
        for p in range(HEADS):
            v, conf = row[20 + p], row[12 + p]
            if conf > 0 and v >= 0 and v < f32(self.ncls[p]):
                with np.errstate(all='ignore'):
                    self.votes[s, t, p, int(v)] = self.votes[s, t, p, int(v)] + conf
                    self._add_total(s, t, p, conf)

    def _end(self, s, t, ended):
        best, share = self.read(s, t)
        self.stats['ended'] += 1
        ended.append((np.concatenate([[self.id[s, t], self.first[s, t], self.last[s, t], self.hits[s, t]], best]).astype(np.int32),
                      np.concatenate([share, self.box[s, t]]).astype(f32)))
        for name in self._SLOT_ARRAYS:
            getattr(self, name)[s, t] = 0

    def _frame(self, s, rows, count, ended):
        """One frame of stream ``s``: (det_out [max_det, 28], tid [max_det])."""
        T, max_det = self.max_tracks, rows.shape[0]
        nc = min(max(int(count), 0), max_det)
        n = min(nc, MAX_DETS)
        frame = int(self.frame[s])
        e = f32(self.expand)
        live = self.live(s)
        slot_row = np.full(T, -1, np.int64)
        row_slot = np.full(n, -1, np.int64)
        kf = (self.misses[s] + 1).astype(f32)
        if n and live.any():
            pred = predict_boxes(self.box[s], self.vel[s], kf)
            iou = iou_matrix(expand_boxes(pred, e), expand_boxes(rows[:n, :4], e))
            pair = live[:, None] & over_threshold(iou, self.match_thres)
            sl, rw = np.nonzero(pair)
            self.stats['pairs'] += len(sl)
            self.stats['ties'] += len(sl) - len(np.unique(iou[sl, rw]))
            for i in np.argsort(_sort_keys(iou[sl, rw], sl * MAX_DETS + rw), kind='stable'):
                if slot_row[sl[i]] < 0 and row_slot[rw[i]] < 0:
                    slot_row[sl[i]], row_slot[rw[i]] = rw[i], sl[i]
                    self.stats['matched'] += 1
        for t in np.nonzero(live)[0]:
            r = slot_row[t]
            if r >= 0:
                row, b = rows[r], self.box[s, t]
                self.vel[s, t] = centre_velocity(row[0:4], b, kf[t])
                self.box[s, t], self.cor[s, t] = row[0:4], row[4:12]
                self.hits[s, t] += 1
                self.misses[s, t] = 0
                self.last[s, t] = frame
                self._vote(s, t, row)
            else:
                self.misses[s, t] += 1
                if self.misses[s, t] > self.max_age:
                    self._end(s, t, ended)
        self._held = self._held_rows(s, live, slot_row) if self._hold is not None else []
        for r in range(n):
            if row_slot[r] >= 0:
                continue
            row = rows[r]
            if not np.float64(new_score(row)) >= self.new_thres:
                continue
            free = np.nonzero(~self.live(s))[0]
            if not len(free):
                self.dropped[s] += 1
                continue
            t = free[0]
            for name in self._SLOT_ARRAYS:
                getattr(self, name)[s, t] = 0
            self.id[s, t] = self.next_id[s]
            self.next_id[s] += 1
            self.first[s, t] = self.last[s, t] = frame
            self.hits[s, t] = 1
            self.box[s, t], self.cor[s, t] = row[0:4], row[4:12]
            self._vote(s, t, row)
            row_slot[r] = t
        det_out = np.zeros_like(rows)
        det_out[:nc] = rows[:nc]
        tid = np.full(max_det, -1, np.int32)
        for r in range(n):
            t = row_slot[r]
            if t >= 0:
                best, share = self.read(s, t)
                det_out[r, 12:20], det_out[r, 20:28], tid[r] = share, best.astype(f32), self.id[s, t]
        self.frame[s] += 1
        self._row_slot = row_slot
        return det_out, tid

    def flush_all(self, max_det=1, max_ended=None):
        """End every live track of every stream: ``update`` of zero frames with every flush flag set."""
        return self.update(np.zeros((0, int(max_det), DET_COLS), f32), np.zeros(0, np.int32), stream_of=[], flush=[1] * self.n_streams,
                           max_ended=max_ended)

    def update(self, det, count, stream_of=None, flush=None, max_ended=None):
        """``B`` frames: det [B, max_det, 28] fp32 and count [B]; ``stream_of[b]`` names the stream of frame b (default
        ``range(B)``; -1: the frame is not tracked, its rows below the count are copied and its tid is -1); the frames of a
        stream are taken in ascending b.  After its frames a stream with ``flush[s]`` ends all its live tracks in slot order.
        Returns (det_out [B,max_det,28], tid [B,max_det] int32, ended_i [S,max_ended,12] int32, ended_f [S,max_ended,12] fp32,
        ended_count [S] int32): per stream the first ``max_ended`` (default ``max_tracks``) records that ended in this call,
        records past them zero; ``ended_count`` is the number that ended and may exceed ``max_ended``."""
        det = np.ascontiguousarray(det, dtype=f32)
        if det.ndim != 3 or det.shape[2] != DET_COLS or det.shape[1] < 1:
            raise ValueError('det must be [B, max_det >= 1, 28]')
        B, max_det = det.shape[:2]
        count = np.asarray(count).astype(np.int64).reshape(-1)
        if len(count) != B:
            raise ValueError('count must be [B]')
        S = self.n_streams
        stream_of, flush, max_ended = check_call(S, B, stream_of, flush, self.max_tracks if max_ended is None else max_ended)
        det_out = np.zeros_like(det)
        tid = self.last_tid = np.full((B, max_det), -1, np.int32)
        slot = self.last_slot = np.full((B, max_det), -1, np.int32)
        ended = [[] for _ in range(S)]
        held = [[] for _ in range(B)]
        for b, s in enumerate(stream_of):
            if s < 0:
                nc = min(max(int(count[b]), 0), max_det)
                det_out[b, :nc] = det[b, :nc]
            else:
                det_out[b], tid[b] = self._frame(s, det[b], count[b], ended[s])
                slot[b, :len(self._row_slot)] = self._row_slot
                held[b] = self._held
        if self._hold is not None:
            det_hold, count_hold, tid_hold = self.last_hold = self.hold_buffers(B, max_det)
            det_hold[:], tid_hold[:] = 0, -1
            for b in range(B):
                nc = min(max(int(count[b]), 0), max_det)
                det_hold[b, :nc], tid_hold[b, :nc] = det_out[b, :nc], tid[b, :nc]
                for k, (row, track_id) in enumerate(held[b]):
                    det_hold[b, nc + k], tid_hold[b, nc + k] = row, track_id
                count_hold[b] = nc + len(held[b])
        for s in range(S):
            if flush[s]:
                for t in np.nonzero(self.live(s))[0]:
                    self._end(s, t, ended[s])
        ended_i = np.zeros((S, max_ended, ENDED_COLS), np.int32)
        ended_f = np.zeros((S, max_ended, ENDED_COLS), f32)
        ended_count = np.zeros(S, np.int32)
        for s in range(S):
            ended_count[s] = len(ended[s])
            for k, (ri, rf) in enumerate(ended[s][:max_ended]):
                ended_i[s, k], ended_f[s, k] = ri, rf
        self._last_ended = (ended_i, ended_count)
        if self._watch is not None:
            from yolov6.utils.watch import watch_match_np
            wl, mm, mc = self._watch
            if self._watch_indel[0]:
                self.last_watch, self.last_watch_align = watch_match_np(wl.entries_np, wl.confuse_np, ended_i, ended_f, ended_count, mm, mc,
                                                                        1, self._watch_indel[1], align=True)
            else:
                self.last_watch = watch_match_np(wl.entries_np, wl.confuse_np, ended_i, ended_f, ended_count, mm, mc)
        if self._live is not None:
            lw = self._live
            self.last_live = lw.step()
            self.last_live_reads = (lw.q_i, lw.q_f, lw.q_slot, lw.q_count)
            self.last_live_align = lw.live_align
        if self._sight is not None:
            from yolov6.utils.sight import sight_update_np
            log, params = self._sight
            self.last_sight = sight_update_np(log.state, log.confuse_np, log.pair_np, ended_i, ended_f, ended_count,
                                              int(self.sight_now[0]), *params)
            self.sight_now += 1
        if self._zones is not None:
            self.last_zone = self._zones[0].step(self._zones[1])
        if self._speed is not None:
            self.last_speed = self._speed[0].step(self, self.speed_clock if self._speed[1] else None)
        return det_out, tid, ended_i, ended_f, ended_count
