"""Plate tracking across video frames (lp_track_update; yolov6/utils/track.py states the rules) and the tracker's add-ons: hold,
best shot, stack, watchlist, live watchlist, sightings, lines and zones (lp_zone_update; yolov6/utils/zones.py states the rule), and the speed on a calibrated plane
(lp_speed_update; yolov6/utils/speed.py states the rule)."""
import ctypes

import torch

from yolov6.hip import abi

from ._base import _aligned_span, _check_det_count, _cuda_device, _dptr, _frames_on, _persistent, _stream_ptr
from .crops import _crop_size, _plate_crops_launch, crop_sharpness
from .frames import _bgr_frames
from .overlay import draw_scene
from .watch import SightLog, Watchlist


def _host_lists(stream_of, B, flush=None):
    """The host lists of a per-stream call as the C ABI takes them: (stream_of as int [max(B, 1)], flush as a pointer to one byte
    per stream, or None)."""
    so = (ctypes.c_int * max(B, 1))(*stream_of)
    return so, None if flush is None else ctypes.cast((ctypes.c_ubyte * len(flush))(*flush), ctypes.c_void_p)


def _zero_streams(state, n_streams, streams):
    """Zero the part of ``streams`` (all for None) in a state tensor of ``n_streams`` equal parts."""
    st = state.view(n_streams, -1)
    if streams is None:
        st.zero_()
    else:
        for s in streams:
            st[int(s)].zero_()


def _max_events(max_events, default):
    """The checked ``max_events`` of ``enable_zones`` / ``enable_speed`` (None: ``default``)."""
    if max_events is not None and int(max_events) < 0:
        raise ValueError('max_events must be >= 0')
    return default if max_events is None else int(max_events)


class _PackedMap:
    """What ``ZoneMap`` and ``GroundPlane`` are: ``ref``, the numpy form of a per-stream map, checked on the host (``host``: the names of
    its copies kept here), and its packed words on the device (``kind``, ``words``: its name in the messages, its words in lp_hip.h)."""

    def __init__(self, ref, host, check_packed, kind, words, device):
        self.n_streams, self.packed_np = ref.n_streams, ref.packed
        self.__dict__.update((name, getattr(ref, name)) for name in host)
        if self.packed_np.shape[1] != words:
            raise RuntimeError('the packed %s map and lp_hip.h disagree' % kind)
        check_packed(self.packed_np)
        self.device = _cuda_device('cuda' if device is None else device, '%s lives on a GPU (%sNp is the CPU form)' % ((type(self).__name__,) * 2))
        self.packed = torch.from_numpy(self.packed_np).to(self.device)


class ZoneMap(_PackedMap):
    """The lines and zones of ``n_streams`` streams on the device (lp_zone_update; ``yolov6.utils.zones`` states the rule and the
    packed layout): the constructor of ``zones.ZoneMapNp`` -- ``lines``: per stream a list of (x1, y1, x2, y2); ``zones``: per stream
    a list of (vertices [n, 2], min_dwell) -- validated on the host and uploaded once; a changed map is a new object.  ``lines_np`` /
    ``zones_np`` / ``packed_np``: the checked host copies; ``packed``: int32 [S, 368] on the device."""

    def __init__(self, n_streams, lines=None, zones=None, device=None):
        from yolov6.utils.zones import ZoneMapNp, check_packed
        super().__init__(ZoneMapNp(n_streams, lines, zones), ('lines_np', 'zones_np'), check_packed, 'zone', abi.LP_ZONE_MAP_WORDS, device)


class GroundPlane(_PackedMap):
    """The calibrated plane of each of ``n_streams`` streams on the device (lp_speed_update; ``yolov6.utils.speed`` states the rule and
    the packed layout): the constructor of ``speed.GroundPlaneNp`` -- ``planes``: per stream None or a dict with ``H`` (3 x 3, frame
    pixels -> metres on the plane the plates move in: calibrate at plate height) and optionally ``period_us``, ``limit_mm_s``,
    ``min_gap_us``, ``min_span_us`` -- validated on the host and uploaded once; a changed calibration is a new object.
    ``planes_np`` / ``packed_np``: the checked host copies; ``packed``: int32 [S, 32] on the device."""

    def __init__(self, n_streams, planes=None, device=None):
        from yolov6.utils.speed import GroundPlaneNp, check_packed
        super().__init__(GroundPlaneNp(n_streams, planes), ('planes_np',), check_packed, 'ground', abi.LP_SPEED_MAP_WORDS, device)


class PlateTracker:
    """``n_streams`` independent device-resident plate trackers of ``max_tracks`` slots each (lp_track_update, one workgroup per
    stream): detections of consecutive frames are associated by the IoU of expanded, velocity-predicted boxes
    (``match_thres``, ``expand``), a row that matches nothing and scores at least ``new_thres`` starts a track, a track unseen
    for more than ``max_age`` frames ends, and every track votes its eight character heads over its frames, weighted by
    confidence.  ``ncls``: the eight head widths, a model, or None for the shipped configs' (31, 24, 37 x 6).  The object owns
    the zeroed state tensor and persistent output buffers (one set per (B, max_det, max_ended): a later ``update`` of the same
    shape overwrites what the earlier one returned).  ``yolov6.utils.track.PlateTrackerNp`` is the same computation on the
    CPU, bit for bit."""

    def __init__(self, n_streams, max_tracks=64, match_thres=0.3, new_thres=0.0, expand=0.5, max_age=5, ncls=None, device=None):
        from yolov6.utils import track
        track.check_params(n_streams, max_tracks, match_thres, new_thres, expand, max_age)
        self.n_streams, self.max_tracks, self.max_age = int(n_streams), int(max_tracks), int(max_age)
        self.ncls = track.ncls_of(ncls)
        self.device = _cuda_device('cuda' if device is None else device, 'PlateTracker runs on a GPU (PlateTrackerNp is the CPU form)')
        self._ncls = (ctypes.c_int * 8)(*self.ncls)                     # what every entry point behind the tracker takes
        self._params = abi.TrackParams(float(match_thres), float(new_thres), float(expand), self.max_age, self._ncls)
        lib = abi.load()
        self._words = lib.lp_track_state_bytes(1, self.max_tracks) // 4
        self.state = torch.zeros(self.n_streams * self._words, dtype=torch.int32, device=self.device)
        self._drop_word = lib.lp_track_dropped_offset(self.max_tracks, 0) // 4
        self._out = {}
        self._slot = {}
        self._shots = None
        self._stack = None
        #: (stack_crops [S,max_ended,Hc,Wc,3] uint8, stack_i [S,max_ended,4] int32) of the last ``update_with_shots`` after
        #: ``enable_stack``, line-parallel to its ended_i, else None
        self.last_stack = None
        self._hold = None
        #: (det_hold, count_hold, tid_hold) of the last ``update`` after ``enable_hold``, else None
        self.last_hold = None
        #: the tid buffer [B,max_det] the last ``update`` filled (what ``LookbackRedactor.push`` reads), else None
        self.last_tid = None
        self._watch = None
        #: match_i [S,max_ended,4] int32 of the last ``update`` after ``enable_watch``, line-parallel to its ended_i, else None
        self.last_watch = None
        #: match_align [S,max_ended] int32 of that lookup after ``enable_watch(..., indel=1)``, else None
        self.last_watch_align = None
        #: live_align [S,max_tracks] int32 of the last ``update`` after ``enable_live_watch(..., indel=1)``, else None
        self.last_live_align = None
        self._live = None
        #: live_i [S,max_tracks,8] int32 of the last ``update`` after ``enable_live_watch``, else None
        self.last_live = None
        #: (q_i, q_f, q_slot, q_count) of that lookup: the fresh reads in the ended-record layout, else None
        self.last_live_reads = None
        self._sight = None
        #: sight_i [S,max_ended,8] int32 of the last ``update`` after ``enable_sightings``, line-parallel to its ended_i, else None
        self.last_sight = None
        #: int32 [1] on the device: the clock of ``enable_sightings``, incremented by one per call; the caller may set it
        self.sight_now = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._zones = None
        #: (zone_ev [S,max_events,12], zone_count [S], zone_occ [S,8], zone_totals [S,2,16]) int32 of the last ``update`` after
        #: ``enable_zones``, else None
        self.last_zone = None
        self._speed = None
        #: (speed_i [S,max_tracks,8], speed_ev [S,max_events,12], speed_count [S]) int32 of the last ``update`` after
        #: ``enable_speed``, else None
        self.last_speed = None
        #: int64 [S] on the device: the clock of ``enable_speed(..., clock=True)`` in microseconds; the caller fills it before every
        #: call, a captured graph reads it in place
        self.speed_clock = torch.zeros(self.n_streams, dtype=torch.int64, device=self.device)

    def reset(self, streams=None):
        """Zero the state of ``streams`` (all for None): no tracks, frame counter, next id and ``dropped`` at 0; their best-shot
        galleries (``enable_best_shot``) and stacks (``enable_stack``) are emptied with them, and their memo of
        ``enable_live_watch`` and of ``enable_zones`` (its totals included, without events).  The log of ``enable_sightings`` and
        ``sight_now`` stay as they are."""
        _zero_streams(self.state, self.n_streams, streams)
        if self._stack is not None:
            _zero_streams(self._stack['state'], self.n_streams, streams)
        if self._live is not None:
            _zero_streams(self._live['memo'], self.n_streams, streams)
        if self._shots is not None:
            _zero_streams(self._shots['state'], self.n_streams, streams)
        if self._zones is not None:
            _zero_streams(self._zones['memo'], self.n_streams, streams)
        if self._speed is not None:
            _zero_streams(self._speed['memo'], self.n_streams, streams)

    @property
    def dropped(self):
        """int32 [n_streams] view of the state: rows that found no free slot since the last reset (on the device)."""
        return self.state.view(self.n_streams, self._words)[:, self._drop_word]

    def update(self, det, count, stream_of=None, flush=None, max_ended=None):
        """``B`` frames: det [B,max_det,28] fp32 + count [B] int32 on the device (``detect_frames_padded`` /
        ``detect_tiled_padded`` / ``nms_padded`` layout); ``stream_of[b]`` (host ints, default ``range(B)``: one frame from
        each of B cameras) names the stream of frame b or is -1 for a frame that is not tracked; ``flush[s]`` ends the live
        tracks of stream s after its frames.  Returns (det_out [B,max_det,28], tid [B,max_det] int32, ended_i
        [S,max_ended,12] int32, ended_f [S,max_ended,12] fp32, ended_count [S] int32), all on the device, no host read: det_out
        is det with the class columns of every tracked row replaced by its track's voted read (columns 12..19 the vote
        shares, 20..27 the voted ids), tid the track id per row (-1: untracked), ended_* the tracks that ended in this call
        (id, first, last, hits, ids | shares, last box), ``max_ended`` per stream (default ``max_tracks``)."""
        from yolov6.utils import track
        _check_det_count(det, count)
        if det.device != self.device:
            raise ValueError('det must be on the tracker\'s device %s' % self.device)
        B, max_det, S = det.shape[0], det.shape[1], self.n_streams
        stream_of, flush, max_ended = track.check_call(S, B, stream_of, flush, self.max_tracks if max_ended is None else max_ended)
        out = self.buffers(B, max_det, max_ended)
        det_out, tid, ended_i, ended_f, ended_count = out
        self.last_tid = tid
        so, fl = _host_lists(stream_of, B, flush)
        hp, hold = None, (None, None, None)
        if self._hold is not None:
            hp, hold = ctypes.byref(self._hold['params']), self.hold_buffers(B, max_det)
            self.last_hold = hold
        with torch.cuda.device(self.device):
            abi.check(abi.load().lp_track_update_hold(_dptr(self.state), S, self.max_tracks, ctypes.byref(self._params), _dptr(det),
                                                      _dptr(count), B, max_det, so, fl, _dptr(det_out),
                                                      _dptr(tid), _dptr(self.slot_buffer(B, max_det)), _dptr(ended_i), _dptr(ended_f),
                                                      _dptr(ended_count), max_ended, hp, _dptr(hold[0]), _dptr(hold[1]), _dptr(hold[2]),
                                                      _stream_ptr(self.device)), 'lp_track_update_hold')
        if self._watch is not None:
            wl, mm, mc, indel, gap = self._watch
            self.last_watch = wl._match(ended_i, ended_f, ended_count, mm, mc, indel, gap)
            self.last_watch_align = wl.last_align
        if self._live is not None:
            self._live_watch()
        if self._sight is not None:
            log, params = self._sight
            self.last_sight = log._update(ended_i, ended_f, ended_count, self.sight_now, *params)
            self.sight_now.add_(1)
        if self._zones is not None:
            self._zone_update()
        if self._speed is not None:
            self._speed_update()
        return out

    def _live_stage_args(self, fn, packed_map, cls, min_hits):
        """The opening of ``enable_zones`` and ``enable_speed``: the map is a ``cls`` of this device and ``n_streams``; the checked min_hits."""
        from yolov6.utils import watch_live
        if not isinstance(packed_map, cls) or packed_map.device != self.device or packed_map.n_streams != self.n_streams:
            raise ValueError('%s needs a %s of %d streams on the tracker\'s device %s' % (fn, cls.__name__, self.n_streams, self.device))
        return watch_live.check_min_hits(min_hits)

    # ---- the speed of the live tracks on a calibrated plane (lp_speed_update; yolov6/utils/speed.py states the rule) ---------------
    def enable_speed(self, ground, min_hits=1, confirm=2, max_events=None, clock=False):
        """From now on every ``update`` / ``update_with_shots`` / ``flush_all*`` also enqueues, at its end on the same stream (behind
        the zones update), lp_speed_update of the live tracks of at least ``min_hits`` hits on ``ground`` (a ``GroundPlane`` of this
        device and of the tracker's ``n_streams``).  ``last_speed`` = (speed_i [S,max_tracks,8], speed_ev [S,max_events,12], speed_count
        [S]) int32: per slot (id, speed, vx, vy in mm/s, X_mm, Y_mm of the newest sample, span_ms, n | fresh << 8 | alerted << 9), or
        (-1, 0, ...) for a slot without an eligible track, speed -1 before the first estimate; per stream the events in slot order as
        (kind, 0, id, slot, frame, value, X_mm, Y_mm, key_lo, key_hi, hits, aux) with kind 1 = over the plane's limit for ``confirm``
        estimates in a row (value: the speed, aux: the limit; once per track) and 3 = ended (value: the peak, aux: the chord speed from
        its first to its last sample); their number, not capped at ``max_events`` (default ``max_tracks``).  With ``clock`` true the
        time of a stream's newest frame is ``speed_clock``, a device int64 [S] in microseconds that the caller fills before every
        call; else it is the frame counter times the plane's period.  Persistent buffers, no host read, no allocation per call.
        Returns, state and every other buffer are what they are without it.  Calling it again zeroes the memo;
        ``enable_speed(None)`` turns it off.  ``PlateTrackerNp.enable_speed`` is the same on the CPU, on every int32."""
        from yolov6.utils import speed
        self.last_speed = None
        if ground is None:
            self._speed = None
            return
        min_hits = self._live_stage_args('enable_speed', ground, GroundPlane, min_hits)
        confirm, max_events = speed.check_confirm(confirm), _max_events(max_events, self.max_tracks)
        S, T, lib = self.n_streams, self.max_tracks, abi.load()
        i32 = dict(dtype=torch.int32, device=self.device)
        self._speed = dict(
            ground=ground, clock=self.speed_clock if clock else None, min_hits=min_hits, confirm=confirm, max_events=max_events,
            memo=torch.zeros(lib.lp_speed_state_bytes(S, T) // 4, **i32).view(S, T, abi.LP_SPEED_MEMO_WORDS),
            rows=torch.empty(S, T, 8, **i32), ev=torch.empty(S, max_events, 12, **i32), count=torch.empty(S, **i32))

    def speed_memo(self):
        """The memo of ``enable_speed``: int32 [S,max_tracks,48] on the device (``yolov6.utils.speed`` states the layout), else None."""
        return None if self._speed is None else self._speed['memo']

    def _speed_update(self):
        """Enqueue lp_speed_update on the state as it stands."""
        sp = self._speed
        with torch.cuda.device(self.device):
            abi.check(abi.load().lp_speed_update(_dptr(self.state), self.n_streams, self.max_tracks, self._ncls, _dptr(sp['ground'].packed),
                                                 _dptr(sp['clock']), sp['min_hits'], sp['confirm'], _dptr(sp['memo']), _dptr(sp['rows']),
                                                 _dptr(sp['ev']), _dptr(sp['count']), sp['max_events'], _stream_ptr(self.device)),
                      'lp_speed_update')
        self.last_speed = (sp['rows'], sp['ev'], sp['count'])

    # ---- lines and zones on the live tracks (lp_zone_update; yolov6/utils/zones.py states the rule) ------------------------------
    def enable_zones(self, zone_map, min_hits=1, max_events=None):
        """From now on every ``update`` / ``update_with_shots`` / ``flush_all*`` also enqueues, at its end on the same stream (behind
        the sightings update), lp_zone_update of the live tracks of at least ``min_hits`` hits on ``zone_map`` (a ``ZoneMap`` of this
        device and of the tracker's ``n_streams``): directed line crossings, zone entry and exit, dwell alerts, tracks that ended
        inside a zone.  ``last_zone`` = (zone_ev [S,max_events,12], zone_count [S], zone_occ [S,8], zone_totals [S,2,16]) int32:
        per stream the events in slot order as (kind, index, id, slot, frame, value, anchor x, y as fp32 bits, key_lo, key_hi, hits,
        0) with kind 1 = crossed (value +1 / -1), 2 = enter, 3 = left (value: frames inside), 4 = dwell, 5 = ended inside; their
        number, not capped at ``max_events`` (default 2 * max_tracks); the eligible tracks inside each zone; the +1 and -1 totals
        per line since the memo was zeroed.  Persistent buffers, no host read, no allocation per call.  Returns, state and every
        other buffer are what they are without it.  Calling it again zeroes the memo and the totals; ``enable_zones(None)`` turns it
        off.  ``PlateTrackerNp.enable_zones`` is the same on the CPU, on every int32."""
        self.last_zone = None
        if zone_map is None:
            self._zones = None
            return
        min_hits, max_events = self._live_stage_args('enable_zones', zone_map, ZoneMap, min_hits), _max_events(max_events, 2 * self.max_tracks)
        S, T, lib = self.n_streams, self.max_tracks, abi.load()
        i32 = dict(dtype=torch.int32, device=self.device)
        self._zones = dict(
            zone_map=zone_map, min_hits=min_hits, max_events=max_events,
            memo=torch.zeros(lib.lp_zone_state_bytes(S, T) // 4, **i32).view(S, T + 2, 16),
            ev=torch.empty(S, max_events, 12, **i32), count=torch.empty(S, **i32), occ=torch.empty(S, 8, **i32),
            totals=torch.empty(S, 2, 16, **i32))

    @property
    def zone_memo(self):
        """The memo of ``enable_zones``: int32 [S,max_tracks+2,16] on the device (per slot id + 1, last, anchor x, y, inside |
        alerted << 8, enter_frame[8], 0, 0, 0; then the +1 and the -1 totals per line), else None."""
        return None if self._zones is None else self._zones['memo']

    def _zone_update(self):
        """Enqueue lp_zone_update on the state as it stands."""
        zn = self._zones
        with torch.cuda.device(self.device):
            abi.check(abi.load().lp_zone_update(_dptr(self.state), self.n_streams, self.max_tracks, self._ncls, _dptr(zn['zone_map'].packed),
                                                zn['min_hits'], _dptr(zn['memo']), _dptr(zn['ev']), _dptr(zn['count']), zn['max_events'],
                                                _dptr(zn['occ']), _dptr(zn['totals']), _stream_ptr(self.device)), 'lp_zone_update')
        self.last_zone = (zn['ev'], zn['count'], zn['occ'], zn['totals'])

    def draw_scene(self, frames, font, det_out, count, tid, stream_of=None, names=None, style=None, status=None):
        """``runtime.draw_scene`` of the tracker's own ``ZoneMap`` (``enable_zones``), ``last_zone`` and ``last_speed`` onto ``frames``
        IN PLACE, after the ``update`` that returned ``det_out`` and ``tid``: zones, lines, their counts, and -- with
        ``enable_speed`` -- a km/h tag per tracked plate.  ``stream_of`` as that ``update`` took it.  On a stream the order is crops and
        best shots, redaction, this call, then ``draw_plates``: zone fills lie under the plate outlines.  Returns the tag status
        [B,max_det] (None without ``enable_speed``).  ``yolov6.utils.scene.draw_scene_np`` on a ``PlateTrackerNp``'s ``last_zone`` /
        ``last_speed`` gives the same bytes."""
        if self._zones is None:
            raise ValueError('draw_scene needs enable_zones (a ZoneMap without lines and zones draws the speed tags alone)')
        tags = self.last_speed is not None
        return draw_scene(frames, self._zones['zone_map'], font, names=names, stream_of=stream_of, zone=self.last_zone,
                          speed=self.last_speed if tags else None, det=det_out if tags else None, count=count if tags else None,
                          tid=tid if tags else None, style=style, status=status)

    # ---- the ended reads matched against the earlier reads of all streams (lp_sight_update; yolov6/utils/sight.py states the rule) ----
    def enable_sightings(self, log, window=0, min_hits=1, max_mismatch=1, max_cost=None):
        """From now on every ``update`` / ``update_with_shots`` / ``flush_all*`` also enqueues, at its end on the same stream (behind
        the lookups of ``enable_watch`` and ``enable_live_watch``), lp_sight_update of the records it ended on ``log`` (a ``SightLog``
        of this device and of the tracker's ``n_streams``), and leaves sight_i [S,max_ended,8] int32 = (slot, mismatches, cost, n_hits,
        prev_stream, prev_id, prev_stamp, prev_seq), line-parallel to ended_i, in ``last_sight``.  The clock is ``sight_now``, a device
        int32 [1]: the call reads it in place and then increments it by one on the device, so that left alone it counts the
        tracker's calls; a caller with a clock of its own sets the tensor before every call (``sight_now.fill_(t)`` or a copy).
        ``window`` is in the clock's units.  No host read, no allocation per call; a caller
        that replays a captured update counts those appends itself (fewer than 2^31 between two ``log.clear()``).  Returns, state
        and every other buffer are what they are without it.  ``enable_sightings(None)`` turns it off."""
        from yolov6.utils import sight, watch
        self.last_sight = None
        if log is None:
            self._sight = None
            return
        if not isinstance(log, SightLog) or log.device != self.device or log.n_streams != self.n_streams:
            raise ValueError('enable_sightings needs a SightLog of %d streams on the tracker\'s device %s' % (self.n_streams, self.device))
        _, window, min_hits = sight.check_call(0, window, min_hits)
        self._sight = (log, (window, min_hits) + watch.check_params(max_mismatch, watch.cost_units(max_cost)))

    # ---- the live tracks looked up in a watchlist (lp_watch_live; yolov6/utils/watch_live.py states the rule) -----------------
    def enable_live_watch(self, watchlist, min_hits=3, max_mismatch=1, max_cost=None, indel=0, gap_cost=None):
        """From now on every ``update`` / ``update_with_shots`` / ``flush_all*`` also enqueues, at its end on the same stream
        (behind the lookup of ``enable_watch`` if that is on), the lookup of the LIVE tracks of at least ``min_hits`` hits in
        ``watchlist`` (a ``Watchlist`` on this device): once per track when it gets there, and again only when its voted read
        changes; a memo per slot, owned by the tracker, holds the answers.  ``last_live`` = live_i [S,max_tracks,8] int32, one
        row per slot: (id, entry, mismatches, cost, n_hits, fresh, hits, last_at_lookup), or (-1, -1, 0, 0, 0, 0, 0, 0) for a
        slot without a looked-up track; a row with fresh == 1 and entry >= 0 is an alert.  ``last_live_reads`` = (q_i, q_f,
        q_slot, q_count): the reads looked up in this call.  Persistent buffers, no host read, no allocation per call.  Returns,
        state and every other buffer are what they are without it.  ``indel=1`` (lp_watch_live_indel): one lost or gained
        character in heads 2..7 is tolerated at ``gap_cost`` fully confident mismatches (None: 1), and ``last_live_align`` =
        live_align [S,max_tracks] int32, the alignment code of every row's lookup (None without it); the tracker owns that tensor
        beside the memo.  Calling it again zeroes the memo;
        ``enable_live_watch(None)`` turns it off.  ``PlateTrackerNp.enable_live_watch`` is the same on the CPU, on every int32."""
        from yolov6.utils import watch, watch_live
        self.last_live = self.last_live_reads = self.last_live_align = None
        if watchlist is None:
            self._live = None
            return
        if not isinstance(watchlist, Watchlist) or watchlist.device != self.device:
            raise ValueError('enable_live_watch needs a Watchlist on the tracker\'s device %s' % self.device)
        min_hits = watch_live.check_min_hits(min_hits)
        mm, mc = watch.check_params(max_mismatch, watch.cost_units(max_cost))
        indel, gap = watch.check_indel(indel, watch.gap_units(gap_cost))
        S, T, dev, lib = self.n_streams, self.max_tracks, self.device, abi.load()
        i32 = dict(dtype=torch.int32, device=dev)
        self._live = dict(
            watchlist=watchlist, min_hits=min_hits, limits=(mm, mc),
            memo=torch.zeros(lib.lp_watch_live_state_bytes(S, T) // 4, **i32).view(S, T, 8),
            live_i=torch.empty(S, T, 8, **i32), q_i=torch.empty(S, T, 12, **i32),
            q_f=torch.empty(S, T, 12, dtype=torch.float32, device=dev), q_slot=torch.empty(S, T, **i32), q_count=torch.empty(S, **i32),
            ws=torch.empty((lib.lp_watch_live_indel_workspace_bytes if indel else lib.lp_watch_live_workspace_bytes)(S, T) + 256,
                           dtype=torch.uint8, device=dev),
            indel=(indel, gap), align=torch.zeros(S, T, **i32) if indel else None)

    @property
    def live_memo(self):
        """The memo of ``enable_live_watch``: int32 [S,max_tracks,8] on the device (id + 1, key_lo, key_hi, entry, mismatches,
        cost, n_hits, last_at_lookup), else None."""
        return None if self._live is None else self._live['memo']

    def _live_watch(self):
        """Enqueue lp_watch_live (lp_watch_live_indel after ``indel=1``) on the state as it stands."""
        lw, lib = self._live, abi.load()
        wl, (indel, gap) = lw['watchlist'], lw['indel']
        reads = (lw['q_i'], lw['q_f'], lw['q_slot'], lw['q_count'])
        head = (_dptr(self.state), self.n_streams, self.max_tracks, self._ncls, lw['min_hits'], _dptr(lw['memo']), _dptr(wl.entries), wl.n,
                _dptr(wl.confuse)) + lw['limits']
        outs = tuple(_dptr(t) for t in reads) + (_dptr(lw['live_i']),)
        tail = _aligned_span(lw['ws']) + (_stream_ptr(self.device),)
        with torch.cuda.device(self.device):
            if indel:
                abi.check(lib.lp_watch_live_indel(*head, indel, gap, *outs, _dptr(lw['align']), *tail), 'lp_watch_live_indel')
            else:
                abi.check(lib.lp_watch_live(*head, *outs, *tail), 'lp_watch_live')
        self.last_live, self.last_live_reads, self.last_live_align = lw['live_i'], reads, lw['align']      # (align: None without indel)

    # ---- the ended reads looked up in a watchlist (lp_watch_match; yolov6/utils/watch.py states the rule) ----------------------
    def enable_watch(self, watchlist, max_mismatch=1, max_cost=None, indel=0, gap_cost=None):
        """From now on every ``update`` / ``update_with_shots`` / ``flush_all*`` also enqueues, behind the tracker on the same
        stream, the lookup of the records it ended in ``watchlist`` (a ``Watchlist`` on this device) and leaves match_i
        [S,max_ended,4] int32 = (entry, mismatches, cost, n_hits), line-parallel to ended_i, in ``last_watch``.  ``max_cost``: a float
        in fully confident mismatches (``watch.cost_units``; None: no limit).  ``indel=1`` (lp_watch_match_indel): one lost or
        gained character in heads 2..7 is tolerated at ``gap_cost`` fully confident mismatches (None: 1), and match_align
        [S,max_ended] int32 is left in ``last_watch_align`` (None without it).  Returns, state and every other buffer are what
        they are without it.  ``enable_watch(None)`` turns it off."""
        from yolov6.utils import watch
        self.last_watch = self.last_watch_align = None
        if watchlist is None:
            self._watch = None
            return
        if not isinstance(watchlist, Watchlist) or watchlist.device != self.device:
            raise ValueError('enable_watch needs a Watchlist on the tracker\'s device %s' % self.device)
        self._watch = (watchlist,) + watch.check_params(max_mismatch, watch.cost_units(max_cost)) + \
            watch.check_indel(indel, watch.gap_units(gap_cost))

    # ---- redaction held over missed frames (lp_track_update_hold; rule 11 of yolov6/utils/track.py) -----------------------------
    def enable_hold(self, min_hits=1, max_misses=None):
        """From now on every ``update`` / ``update_with_shots`` also fills ``hold_buffers`` (``last_hold``): the frame's rows
        followed by a predicted row for every track of at least ``min_hits`` hits that the frame missed, for at most
        ``max_misses`` frames in a row (None, or anything above ``max_age``: ``max_age``, where the track ends).  That is the
        (det, count) to hand ``redact_plates``, so that a plate the detector loses for a frame is still covered.  Returns,
        state and every other buffer are what they are without it."""
        min_hits, max_misses = int(min_hits), self.max_age if max_misses is None else int(max_misses)
        if min_hits < 1 or max_misses < 0:
            raise ValueError('hold needs min_hits >= 1 and max_misses >= 0')
        self._hold = dict(params=abi.TrackHoldParams(min_hits, max_misses), out={})

    def hold_buffers(self, B, max_det):
        """The persistent (det_hold [B,max_det+max_tracks,28] fp32, count_hold [B] int32, tid_hold [B,max_det+max_tracks] int32)
        an ``update`` of that shape fills after ``enable_hold`` (``PlateTrackerNp.hold_buffers``)."""
        if self._hold is None:
            raise RuntimeError('call enable_hold() first')
        B, rows, dev = int(B), int(max_det) + self.max_tracks, self.device
        return _persistent(self._hold['out'], (B, int(max_det)), lambda: (
            torch.empty(B, rows, abi.LP_DET_COLS, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
            torch.empty(B, rows, dtype=torch.int32, device=dev)))

    def slot_buffer(self, B, max_det):
        """The persistent int32 [B,max_det] tensor an ``update`` of that shape fills beside its returns: the tracker slot of each
        matched or new row's track, -1 wherever tid is -1 (``PlateTrackerNp.last_slot``)."""
        key = (int(B), int(max_det))
        return _persistent(self._slot, key, lambda: torch.empty(key, dtype=torch.int32, device=self.device))

    def buffers(self, B, max_det, max_ended=None):
        """The persistent outputs of an ``update`` of B frames of max_det rows: (det_out, tid, ended_i, ended_f, ended_count)."""
        S, dev = self.n_streams, self.device
        key = (int(B), int(max_det), self.max_tracks if max_ended is None else int(max_ended))
        return _persistent(self._out, key, lambda: (
            torch.empty(key[0], key[1], abi.LP_DET_COLS, dtype=torch.float32, device=dev),
            torch.empty(key[0], key[1], dtype=torch.int32, device=dev), torch.empty(S, key[2], 12, dtype=torch.int32, device=dev),
            torch.empty(S, key[2], 12, dtype=torch.float32, device=dev), torch.empty(S, dtype=torch.int32, device=dev)))

    def _no_frames(self, max_det):
        """The (det, count) of zero frames of ``max_det`` rows: what the flushes hand ``update``."""
        return (torch.empty(0, int(max_det), abi.LP_DET_COLS, dtype=torch.float32, device=self.device),
                torch.empty(0, dtype=torch.int32, device=self.device))

    def flush_all(self, max_det=1, max_ended=None):
        """End every live track of every stream: ``update`` of zero frames with every flush flag set."""
        return self.update(*self._no_frames(max_det), stream_of=[], flush=[1] * self.n_streams, max_ended=max_ended)

    # ---- the best shot of every track (lp_crop_sharpness, lp_best_shot_update; yolov6/utils/best_shot.py states the rules) ----
    def enable_best_shot(self, crop_hw=(64, 192), max_crops=16, min_score=0.0):
        """Allocate the zeroed gallery: per slot the sharpest ``crop_hw`` crop its track has shown (``update_with_shots``).  The
        first ``max_crops`` rows of a frame compete; a row needs a mean confidence of at least ``min_score``."""
        Hc, Wc = _crop_size(crop_hw)
        if int(max_crops) < 1:
            raise ValueError('max_crops must be >= 1')
        if not abs(float(min_score)) <= 3.0e38:
            raise ValueError('min_score must be finite (|min_score| <= 3e38)')
        nbytes = abi.load().lp_best_shot_state_bytes(self.n_streams, self.max_tracks, Hc, Wc)
        self._stack = self.last_stack = None        # (a stack is made for the gallery's crop size: enable_stack again)
        self._shots = dict(crop_hw=(Hc, Wc), max_crops=int(max_crops), min_score=float(min_score), out={},
                           state=torch.zeros(nbytes, dtype=torch.uint8, device=self.device),
                           blank=torch.zeros(1, 1, 3, dtype=torch.uint8, device=self.device))

    def shot_buffers(self, B, max_ended=None):
        """The persistent buffers of an ``update_with_shots`` of B frames: (crops [B,max_crops,Hc,Wc,3] uint8, status
        [B,max_crops] int32, sharp [B,max_crops] int64, shot_crops [S,max_ended,Hc,Wc,3] uint8, shot_i [S,max_ended,4] int32,
        shot_q [S,max_ended] int64, shot_det [S,max_ended,28] fp32)."""
        if self._shots is None:
            raise RuntimeError('call enable_best_shot() first')
        sh, S, dev = self._shots, self.n_streams, self.device
        (Hc, Wc), m = sh['crop_hw'], sh['max_crops']
        key = (int(B), self.max_tracks if max_ended is None else int(max_ended))
        return _persistent(sh['out'], key, lambda: (
            torch.zeros(key[0], m, Hc, Wc, 3, dtype=torch.uint8, device=dev), torch.zeros(key[0], m, dtype=torch.int32, device=dev),
            torch.zeros(key[0], m, dtype=torch.int64, device=dev), torch.zeros(S, key[1], Hc, Wc, 3, dtype=torch.uint8, device=dev),
            torch.empty(S, key[1], 4, dtype=torch.int32, device=dev), torch.empty(S, key[1], dtype=torch.int64, device=dev),
            torch.empty(S, key[1], abi.LP_DET_COLS, dtype=torch.float32, device=dev)))

    def update_with_shots(self, frames, det, count, stream_of=None, flush=None, max_ended=None):
        """``update`` plus the best shot of every track that ends in it, enqueued back to back with no host read: the tracker,
        ``plate_crops`` of ``frames`` (contiguous uint8 CUDA [h,w,3] BGR, frame b of ``det``; shorter than B or None where
        ``stream_of`` is -1) along the rows of ``det`` as given, ``crop_sharpness``, then lp_best_shot_update.  Returns the five
        tensors of ``update`` followed by (shot_crops [S,max_ended,Hc,Wc,3] uint8, shot_i [S,max_ended,4] int32 = frame, row,
        status, valid; shot_q [S,max_ended] int64 holding the unsigned sharpness; shot_det [S,max_ended,28] fp32 = the shot's
        row with its per-frame confidences), line-parallel to ended_i / ended_f; persistent buffers per shape.  The crop of a
        record without a shot (valid 0) is left as it was.  yolov6.utils.best_shot.BestShotNp is the same computation on the
        CPU, bit for bit.  ``frames`` may be ``Nv12Frame``s instead: they are converted once (``nv12_to_bgr``) on this stream."""
        from yolov6.utils import track
        if self._shots is None:
            raise RuntimeError('call enable_best_shot() first')
        S, B = self.n_streams, det.shape[0]
        stream_of, _, max_ended = track.check_call(S, B, stream_of, flush, self.max_tracks if max_ended is None else max_ended)
        frames = list(frames) + [None] * (B - len(frames))
        if len(frames) != B:
            raise ValueError('%d frames for a batch of %d' % (len(frames), B))
        for b, f in enumerate(frames):
            if f is None and stream_of[b] >= 0:
                raise ValueError('frame %d of stream %d is missing' % (b, stream_of[b]))
        live = [f for f in frames if f is not None]
        if live and _frames_on(live, 'update_with_shots')[0] != self.device:
            raise ValueError('frames must be on the tracker\'s device %s' % self.device)
        frames = _bgr_frames(frames)        # an NV12 list is converted once, on this stream
        out = self.update(det, count, stream_of, flush, max_ended)
        crops, status, sharp = self._shot_crops(frames, det, count, stream_of, max_ended)
        if B:
            crop_sharpness(crops, status, out=sharp)
        shots = self._shot_gallery(det, count, stream_of, max_ended)
        if self._stack is not None:
            self.last_stack = self._stack_update(det, count, stream_of, max_ended)
        return out + shots

    def _shot_crops(self, frames, det, count, stream_of, max_ended):
        """The crop stage of ``update_with_shots``: (crops, status, sharp) of ``shot_buffers``, the first two written."""
        sh, B = self._shots, det.shape[0]
        crops, status, sharp = self.shot_buffers(B, max_ended)[:3]
        m = sh['max_crops']
        if B:
            # a frame that is not tracked takes no slots: its status keeps what an earlier call left, and nothing reads it
            off = [f is None or stream_of[b] < 0 for b, f in enumerate(frames)]
            _plate_crops_launch([sh['blank'] if o else f for o, f in zip(off, frames)], det, count,
                                [(0 if o else m, b * m) for b, o in enumerate(off)], crops, status, sh['crop_hw'])
        return crops, status, sharp

    def _shot_gallery(self, det, count, stream_of, max_ended):
        """The gallery stage of ``update_with_shots`` behind ``update`` of the same arguments: (shot_crops, shot_i, shot_q,
        shot_det)."""
        sh, S, (B, max_det) = self._shots, self.n_streams, det.shape[:2]
        crops, status, sharp, shot_crops, shot_i, shot_q, shot_det = self.shot_buffers(B, max_ended)
        _, tid, ended_i, _, ended_count = self.buffers(B, max_det, max_ended)
        so, _ = _host_lists(stream_of, B)
        with torch.cuda.device(self.device):
            abi.check(abi.load().lp_best_shot_update(_dptr(sh['state']), S, self.max_tracks, sh['crop_hw'][0], sh['crop_hw'][1], _dptr(det),
                                                     _dptr(count), B, max_det, _dptr(tid), _dptr(self.slot_buffer(B, max_det)), _dptr(crops),
                                                     _dptr(status), _dptr(sharp), sh['max_crops'], so, _dptr(ended_i), _dptr(ended_count),
                                                     max_ended, sh['min_score'], _dptr(shot_crops), _dptr(shot_i), _dptr(shot_q),
                                                     _dptr(shot_det), _stream_ptr(self.device)), 'lp_best_shot_update')
        return shot_crops, shot_i, shot_q, shot_det

    # ---- one denoised picture per track (lp_stack_update; yolov6/utils/stack.py states the rule and its limits) ------------------
    def enable_stack(self, search=2, max_frames=64, min_width=0.0, min_sharp=0):
        """From now on every ``update_with_shots`` / ``flush_all_with_shots`` also enqueues, behind the gallery on the same
        stream, lp_stack_update on the same crops: the rectified (status 1) crops of every track, at most ``max_frames`` (1..255)
        of them, each from a plate at least ``min_width`` frame pixels wide and of a sharpness of at least ``min_sharp``, are
        aligned by an integer shift of at most ``search`` (0..4) pixels and summed, and the rounded mean of a track that ends is
        left in ``last_stack`` = (stack_crops [S,max_ended,Hc,Wc,3] uint8, stack_i [S,max_ended,4] int32 = n, first_frame,
        last_frame, valid), line-parallel to ended_i; persistent buffers per shape, the crop of a record without a stack (valid 0)
        is left as it was.  It needs ``enable_best_shot`` first and shares its ``crop_hw``, ``max_crops`` and ``min_score``.  The
        nine returns, the tracker's and the gallery's state are what they are without it.  Calling it again starts from empty
        stacks; ``enable_stack(None)`` turns it off.  ``PlateTrackerNp.enable_stack`` with ``yolov6.utils.stack.StackNp`` is the
        same computation on the CPU, bit for bit."""
        from yolov6.utils import stack
        self.last_stack = None
        if search is None:
            self._stack = None
            return
        if self._shots is None:
            raise RuntimeError('call enable_best_shot() first')
        sh = self._shots
        search, max_frames, min_width, min_sharp, min_score = stack.check_params(search, max_frames, min_width, min_sharp, sh['min_score'])
        nbytes = abi.load().lp_stack_state_bytes(self.n_streams, self.max_tracks, *sh['crop_hw'])
        self._stack = dict(params=abi.StackParams(min_score, min_width, min_sharp, search, max_frames), out={},
                           state=torch.zeros(nbytes, dtype=torch.uint8, device=self.device))

    def stack_buffers(self, max_ended=None):
        """The persistent (stack_crops [S,max_ended,Hc,Wc,3] uint8, stack_i [S,max_ended,4] int32) of an ``update_with_shots``
        with that ``max_ended`` after ``enable_stack``."""
        if self._stack is None:
            raise RuntimeError('call enable_stack() first')
        S, dev, (Hc, Wc) = self.n_streams, self.device, self._shots['crop_hw']
        key = self.max_tracks if max_ended is None else int(max_ended)
        return _persistent(self._stack['out'], key, lambda: (torch.zeros(S, key, Hc, Wc, 3, dtype=torch.uint8, device=dev),
                                                             torch.empty(S, key, 4, dtype=torch.int32, device=dev)))

    def _stack_update(self, det, count, stream_of, max_ended):
        """The stack stage of ``update_with_shots`` behind the gallery stage of the same arguments: (stack_crops, stack_i)."""
        sh, sk, S, (B, max_det) = self._shots, self._stack, self.n_streams, det.shape[:2]
        crops, status, sharp = self.shot_buffers(B, max_ended)[:3]
        _, tid, ended_i, _, ended_count = self.buffers(B, max_det, max_ended)
        stack_crops, stack_i = self.stack_buffers(max_ended)
        so, _ = _host_lists(stream_of, B)
        with torch.cuda.device(self.device):
            abi.check(abi.load().lp_stack_update(_dptr(sk['state']), S, self.max_tracks, sh['crop_hw'][0], sh['crop_hw'][1], _dptr(det),
                                                 _dptr(count), B, max_det, _dptr(tid), _dptr(self.slot_buffer(B, max_det)), _dptr(crops),
                                                 _dptr(status), _dptr(sharp), sh['max_crops'], so, _dptr(ended_i), _dptr(ended_count),
                                                 max_ended, ctypes.byref(sk['params']), _dptr(stack_crops), _dptr(stack_i),
                                                 _stream_ptr(self.device)), 'lp_stack_update')
        return stack_crops, stack_i

    def flush_all_with_shots(self, max_det=1, max_ended=None):
        """``flush_all`` with the best shots of the tracks it ends: ``update_with_shots`` of zero frames."""
        return self.update_with_shots([], *self._no_frames(max_det), stream_of=[], flush=[1] * self.n_streams, max_ended=max_ended)
