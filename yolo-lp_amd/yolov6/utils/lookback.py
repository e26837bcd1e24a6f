"""The look-back delay of plate redaction, on the CPU: ``LookbackNp`` is the written-down specification of ``lp_lookback_update``
(include/lp_hip.h, csrc/lp_lookback.hip), which matches it bit for bit, and the CPU path of ``Inferer(redact_lookback=D)``.

A plate enters the picture small or blurred and the detector finds it a few frames later; the hold (rule 11 of
``yolov6.utils.track``) covers a track after its first detection, never before it.  The delay line keeps the redaction rows of the
last ``depth`` frames of every stream, adds rows to those past frames once a new track's second detection has fixed its velocity,
and hands the rows of a frame out ``depth`` frames later, when the frame itself is redacted.

The reference has nothing here: its Inferer treats video frames independently (yolov6/core/inferer.py).

Parameters: ``depth`` D in 1..MAX_DEPTH (32); ``max_back`` >= 0: the frames before a track's first detection that are covered
(default D); ``back_cap`` >= 0: the back rows a stored frame can take (default ``max_tracks``).  With hold_rows = max_det +
max_tracks and rows = hold_rows + back_cap every stored entry is [rows, 28] fp32 plus a count; rows * 28 must stay below 2^31.

State, all zero = empty.  Per stream: the counter ``f`` of tracked frames; ``base``: every frame below it has been released;
``dropped``: the back rows that found no room; a ring of D entries, frame g living in entry g % D.  Per tracker slot: id + 1
(0 = empty), ``seen`` (0, 1 or 2), ``first`` (the stream frame of the first detection) and the twelve geometry words of that
detection.

Inputs of a call are what a ``PlateTracker.update`` of the same frames left behind: det_hold [B, hold_rows, 28], count_hold [B],
tid [B, max_det], slot [B, max_det] (a slot names at most one row of a frame), and the host ``stream_of`` and ``flush``.  The
frames of a stream are taken in ascending b.  Per tracked frame, its stream counter at f:
  A. follow: every row r < min(max_det, MAX_DETS) with slot[b, r] = t in 0..max_tracks-1 and tid[b, r] = id >= 0, in ascending r;
     the row is det_hold[b, r], which is det_out[b, r] (rule 11).  The entry of t holds another id, or is empty: it becomes
     {id + 1, seen = 1, first = f, geometry = columns 0..11}.  It holds id with seen == 1: the row CONFIRMS the track (B) and
     seen = 2.  seen == 2: nothing happens.
  B. back rows of a confirming row, fp32 op by op, no fused multiply-add: k = (float)(f - first),
     vx = ((x1' + x2') * 0.5f - (x1 + x2) * 0.5f) / k and vy likewise (step 4 of the tracker; primes mark the confirming row,
     the unprimed values are the stored first geometry).  Targets: every frame g with max(base, f - D, first - max_back, 0) <= g < f
     and g != first, in ascending g.  The back row for g: m = (float)(g - first) (negative before the first detection, positive
     in the gap between the two), dx = vx * m, dy = vy * m (rounded products); columns 0..3 = the first box + (dx, dy, dx, dy);
     columns 4..11 = the first corners, x columns + dx and y columns + dy; columns 12..27 those of the confirming row (the
     track's shares and voted ids after this frame's vote).  The row is appended to the ring entry of g behind the rows already
     there; within one frame the appended rows come in ascending r.  An entry that already holds ``rows`` rows does not take
     the row and ``dropped`` goes up.  A track with only one detection gets no back rows.
  C. release: if f - D >= base: rel_det[b] = the entry of frame f - D (its rows, then zero rows), rel_count[b] its count,
     rel_frame[b] = f - D, then base = f - D + 1.  Otherwise rel_det[b] is all zero, rel_count[b] = 0 and rel_frame[b] = -1.
  D. store: the entry f % D becomes the first min(max(count_hold[b], 0), hold_rows) rows of det_hold[b] followed by zero rows,
     with that count.  Then f goes up.
A frame with stream_of = -1 is released at once: rel_det[b] = its own det_hold rows below the clamped count (then zero rows),
rel_count[b] that count, rel_frame[b] = -2; it touches no state.
After a stream's frames, with flush[s]: every frame still in the ring, base .. f - 1, goes to tail_det [S, D, rows, 28],
tail_count [S, D] and tail_frame [S, D] in ascending frame order; the remaining tail entries are zero rows, count 0, frame -1;
then base = f.  The slot entries stay: the tracker has ended those tracks, and new ids replace them by rule A.  A stream without a
flush gets an all-empty tail.  Every element of rel_* and tail_* is written exactly once per call.

What it does not do: the model is constant velocity from two detections only; a plate visible for more than ``depth`` frames
before its confirmation is covered for ``depth`` of them; a track that is never confirmed adds nothing; the delay is ``depth``
frames of latency, and ``depth`` frames that the caller's frame memory stays occupied.
"""
import numpy as np

from yolov6.utils.track import DET_COLS, MAX_DETS, check_call

f32 = np.float32
MAX_DEPTH = 32            # LP_LOOKBACK_MAX_DEPTH
SLOT_WORDS = 16           # a slot entry of the kernel's state: id + 1, seen, first, one unused word, geometry[12]


def check_lookback(max_tracks, depth, max_back, back_cap):
    """(depth, max_back, back_cap) of a delay line over trackers of ``max_tracks`` slots, defaults filled in (ValueError)."""
    depth = int(depth)
    if not 1 <= depth <= MAX_DEPTH:
        raise ValueError('lookback depth must be in 1..%d' % MAX_DEPTH)
    max_back = depth if max_back is None else int(max_back)
    back_cap = int(max_tracks) if back_cap is None else int(back_cap)
    if max_back < 0 or back_cap < 0:
        raise ValueError('lookback needs max_back >= 0 and back_cap >= 0')
    return depth, max_back, back_cap


def state_words(max_tracks, depth, rows):
    """int32 words of one stream of the kernel's state (lp_lookback_state_bytes / 4): 4 header words (f, base, dropped, unused),
    ``max_tracks`` slot entries of SLOT_WORDS, ``depth`` counts rounded up to a multiple of 4, ``depth`` entries of rows * 28."""
    return 4 + int(max_tracks) * SLOT_WORDS + (int(depth) + 3) // 4 * 4 + int(depth) * int(rows) * DET_COLS


class LookbackHost:
    """The host side the two delay lines share: which frame leaves at which b follows from per-stream counters kept here, so
    nothing is read back.  A subclass gives ``_update`` (the rule, on its arrays) and ``_redact``."""

    def _init_host(self, tracker, depth, max_back, back_cap, mode, cell, margin, fill, sigma=None):
        from yolov6.utils.redact import check_params, check_sigma, fill_bytes
        if getattr(tracker, '_hold', None) is None:
            raise RuntimeError('call enable_hold() on the tracker first')
        self.tracker = tracker
        self.n_streams, self.max_tracks = tracker.n_streams, tracker.max_tracks
        self.depth, self.max_back, self.back_cap = check_lookback(self.max_tracks, depth, max_back, back_cap)
        check_params(mode, cell, margin)
        fill_bytes(fill)
        self.mode, self.cell, self.margin, self.fill = mode, int(cell), float(margin), tuple(int(v) for v in fill)
        self.sigma = check_sigma(sigma) if mode == 'gauss' else sigma
        self._f = [0] * self.n_streams          # the host's copy of the counters f and base
        self._base = [0] * self.n_streams
        self._held = [dict() for _ in range(self.n_streams)]      # frame number -> the caller's frame, by reference

    def _reset_host(self, streams):
        for s in (range(self.n_streams) if streams is None else streams):
            self._f[int(s)] = self._base[int(s)] = 0
            self._held[int(s)].clear()

    def pending(self, s):
        """The number of frames of stream ``s`` inside the delay."""
        return len(self._held[int(s)])

    def push(self, frames, stream_of=None, flush=None, between=None):
        """Called right behind ``tracker.update(...)`` (or ``update_with_shots``) of the same frames, with the same ``stream_of``
        and ``flush``: ``frames[b]`` is frame b of that update (the list may be shorter than B, or hold None, where ``stream_of``
        is -1).  The frames are kept BY REFERENCE -- the caller hands them over and must not write them until they come back.
        Returns [(stream, frame_number, frame), ...]: the frames that left the delay in this call, redacted with the rows the
        delay line released for them, in release order (ascending b, then the tails of flushed streams in stream order,
        ascending frame).  An untracked frame comes back at once as (-1, -2, frame).  Whatever reads the frames (crops, best
        shots) has read them at update time, before any redaction: redaction goes last by construction.  ``between``: a
        callable run between the delay line's update and the redaction (the place of a timing event)."""
        hold = self.tracker.last_hold
        if hold is None or getattr(self.tracker, 'last_tid', None) is None:
            raise RuntimeError('push() follows an update() of a tracker with enable_hold()')
        B = hold[0].shape[0]
        stream_of, flush, _ = check_call(self.n_streams, B, stream_of, flush, 0)
        frames = list(frames) + [None] * (B - len(frames))
        if len(frames) != B:
            raise ValueError('%d frames for an update of %d' % (len(frames), B))
        for b, fr in enumerate(frames):
            if fr is None and stream_of[b] >= 0:
                raise ValueError('frame %d of stream %d is missing' % (b, stream_of[b]))
        # plan on copies of the counters; they, and the frames, are committed only behind an update that went through, so a
        # call that raises (another row width, a bad argument) leaves the host's mirror of f and base where the state is
        D, rel, tails = self.depth, [], []
        f_of, base_of = list(self._f), list(self._base)
        held = [dict() for _ in range(self.n_streams)]        # the frames this call adds
        frame_of = lambda s, g: held[s][g] if g in held[s] else self._held[s][g]   # noqa: E731
        for b, s in enumerate(stream_of):
            if s < 0:
                if frames[b] is not None:
                    rel.append((b, -1, -2, frames[b]))
                continue
            f = f_of[s]
            if f - D >= base_of[s]:
                rel.append((b, s, f - D, frame_of(s, f - D)))
                base_of[s] = f - D + 1
            held[s][f] = frames[b]
            f_of[s] = f + 1
        for s in range(self.n_streams):
            if flush[s]:
                tails.append((s, [(g, frame_of(s, g)) for g in range(base_of[s], f_of[s])]))
                base_of[s] = f_of[s]
        if B == 0 and not self._allocated():
            return []           # a flush before the first frame: nothing is inside the delay, and the entries have no size yet
        out = self._update(hold[0], hold[1], self.tracker.last_tid, self._slots(), stream_of, flush)
        for s in range(self.n_streams):
            self._held[s].update(held[s])
            for g in [g for g in self._held[s] if g < base_of[s]]:
                del self._held[s][g]
        self._f, self._base = f_of, base_of
        if between is not None:
            between()
        return self._redact(frames, rel, tails, out)

    def flush_all(self):
        """Every frame still inside the delay, redacted: ``push`` of zero frames with every flush flag set, behind the tracker's
        ``flush_all`` (an update of zero frames)."""
        return self.push([], stream_of=[], flush=[1] * self.n_streams)


class LookbackNp(LookbackHost):
    """The delay line over a ``PlateTrackerNp`` with ``enable_hold`` called (the module docstring states the rules).  Same
    constructor, ``push``, ``flush_all``, ``dropped`` and ``reset`` as ``yolov6.hip.runtime.LookbackRedactor``, on numpy arrays with
    ``redact_plates_np``; ``update`` is the rule alone."""

    def __init__(self, tracker, depth, max_back=None, back_cap=None, mode='mosaic', cell=16, margin=0.1, fill=(0, 0, 0), sigma=None):
        self._init_host(tracker, depth, max_back, back_cap, mode, cell, margin, fill, sigma)
        S, T, D = self.n_streams, self.max_tracks, self.depth
        self.f = np.zeros(S, np.int32)
        self.base = np.zeros(S, np.int32)
        self.dropped = np.zeros(S, np.int32)
        self.idp1 = np.zeros((S, T), np.int32)
        self.seen = np.zeros((S, T), np.int32)
        self.first = np.zeros((S, T), np.int32)
        self.geom = np.zeros((S, T, 12), f32)
        self.ring_count = np.zeros((S, D), np.int32)
        self.ring = None                        # [S, D, rows, 28], allocated by the first update (rows follows max_det)
        #: counters for tests and diagnostics (no part of the state): tracks confirmed, back rows appended
        self.stats = dict(confirmed=0, back_rows=0)

    def reset(self, streams=None):
        """Zero the state of ``streams`` (all for None) and forget their frames; use it together with the tracker's ``reset``."""
        for s in (range(self.n_streams) if streams is None else streams):
            for name in ('f', 'base', 'dropped', 'idp1', 'seen', 'first', 'geom', 'ring_count'):
                getattr(self, name)[s] = 0
            if self.ring is not None:
                self.ring[s] = 0
        self._reset_host(streams)

    def _slots(self):
        return self.tracker.last_slot

    def _allocated(self):
        return self.ring is not None

    def state_words(self):
        """The state as int32 [n_streams, words] in the kernel's layout (``state_words``)."""
        S, T, D = self.n_streams, self.max_tracks, self.depth
        rows = self.ring.shape[2]
        out = np.zeros((S, state_words(T, D, rows)), np.int32)
        out[:, 0], out[:, 1], out[:, 2] = self.f, self.base, self.dropped
        slots = out[:, 4:4 + T * SLOT_WORDS].reshape(S, T, SLOT_WORDS)
        slots[:, :, 0], slots[:, :, 1], slots[:, :, 2] = self.idp1, self.seen, self.first
        slots[:, :, 4:] = self.geom.view(np.int32)
        c0 = 4 + T * SLOT_WORDS
        out[:, c0:c0 + D] = self.ring_count
        out[:, c0 + (D + 3) // 4 * 4:] = self.ring.reshape(S, -1).view(np.int32)
        return out

    def _frame(self, s, b, det_hold, count_hold, tid, slot, out):
        T, D = self.max_tracks, self.depth
        hold_rows, rows = det_hold.shape[1], self.ring.shape[2]
        rel_det, rel_count, rel_frame = out[:3]
        f, base = int(self.f[s]), int(self.base[s])
        for r in range(min(tid.shape[1], MAX_DETS)):
            t, tr = int(slot[b, r]), int(tid[b, r])
            if tr < 0 or not 0 <= t < T:
                continue
            row = det_hold[b, r]
            if self.idp1[s, t] != tr + 1:
                self.idp1[s, t], self.seen[s, t], self.first[s, t] = tr + 1, 1, f
                self.geom[s, t] = row[:12]
                continue
            if self.seen[s, t] != 1:
                continue
            self.seen[s, t] = 2
            self.stats['confirmed'] += 1
            first, g0 = int(self.first[s, t]), self.geom[s, t]
            with np.errstate(all='ignore'):
                k = f32(f - first)
                vx = ((row[0] + row[2]) * f32(0.5) - (g0[0] + g0[2]) * f32(0.5)) / k
                vy = ((row[1] + row[3]) * f32(0.5) - (g0[1] + g0[3]) * f32(0.5)) / k
                for g in range(max(base, f - D, first - self.max_back, 0), f):
                    if g == first:
                        continue
                    e = g % D
                    if self.ring_count[s, e] >= rows:
                        self.dropped[s] += 1
                        continue
                    m = f32(g - first)
                    d = np.array([vx * m, vy * m], f32)
                    back = row.copy()
                    back[:12] = g0 + np.tile(d, 6)
                    self.ring[s, e, self.ring_count[s, e]] = back
                    self.ring_count[s, e] += 1
                    self.stats['back_rows'] += 1
        e = f % D
        if f - D >= base:
            rel_det[b], rel_count[b], rel_frame[b] = self.ring[s, e], self.ring_count[s, e], f - D
            self.base[s] = f - D + 1
        else:
            rel_det[b], rel_count[b], rel_frame[b] = 0, 0, -1
        n = min(max(int(count_hold[b]), 0), hold_rows)
        self.ring[s, e] = 0
        self.ring[s, e, :n] = det_hold[b, :n]
        self.ring_count[s, e] = n
        self.f[s] = f + 1

    def update(self, det_hold, count_hold, tid, slot, stream_of=None, flush=None):
        """The rule on one call's arrays (the module docstring): returns (rel_det [B, rows, 28] fp32, rel_count [B] int32,
        rel_frame [B] int32, tail_det [S, D, rows, 28] fp32, tail_count [S, D] int32, tail_frame [S, D] int32), new arrays."""
        det_hold = np.ascontiguousarray(det_hold, dtype=f32)
        if det_hold.ndim != 3 or det_hold.shape[2] != DET_COLS:
            raise ValueError('det_hold must be [B, hold_rows, 28]')
        B, hold_rows = det_hold.shape[:2]
        tid, slot = np.asarray(tid).astype(np.int64), np.asarray(slot).astype(np.int64)
        count_hold = np.asarray(count_hold).astype(np.int64).reshape(-1)
        max_det = tid.shape[1] if tid.ndim == 2 else 0
        if len(count_hold) != B or tid.shape != (B, max_det) or slot.shape != (B, max_det) or max_det < 1 or hold_rows < max_det:
            raise ValueError('count_hold must be [B], tid and slot [B, max_det] with 1 <= max_det <= hold_rows')
        S, D, rows = self.n_streams, self.depth, hold_rows + self.back_cap
        if B == 0 and self.ring is not None:
            rows = self.ring.shape[2]           # a call without frames (a flush) takes the entries as they are
        if rows * DET_COLS >= 2 ** 31:
            raise ValueError('rows * 28 must stay below 2^31')
        if self.ring is None and B == 0:         # a flush before the first frame: all-empty tails, and no size is fixed yet
            check_call(S, B, stream_of, flush, 0)
            return (np.zeros((0, rows, DET_COLS), f32), np.zeros(0, np.int32), np.zeros(0, np.int32),
                    np.zeros((S, D, rows, DET_COLS), f32), np.zeros((S, D), np.int32), np.full((S, D), -1, np.int32))
        if self.ring is None:
            self.ring = np.zeros((S, D, rows, DET_COLS), f32)
        elif self.ring.shape[2] != rows:
            raise ValueError('this delay line holds entries of %d rows, the call has %d' % (self.ring.shape[2], rows))
        stream_of, flush, _ = check_call(S, B, stream_of, flush, 0)
        out = (np.zeros((B, rows, DET_COLS), f32), np.zeros(B, np.int32), np.full(B, -1, np.int32),
               np.zeros((S, D, rows, DET_COLS), f32), np.zeros((S, D), np.int32), np.full((S, D), -1, np.int32))
        for b, s in enumerate(stream_of):
            if s < 0:
                n = min(max(int(count_hold[b]), 0), hold_rows)
                out[0][b, :n], out[1][b], out[2][b] = det_hold[b, :n], n, -2
            else:
                self._frame(s, b, det_hold, count_hold, tid, slot, out)
        for s in range(S):
            if flush[s]:
                for k, g in enumerate(range(int(self.base[s]), int(self.f[s]))):
                    out[3][s, k], out[4][s, k], out[5][s, k] = self.ring[s, g % D], self.ring_count[s, g % D], g
                self.base[s] = self.f[s]
        return out

    def _update(self, det_hold, count_hold, tid, slot, stream_of, flush):
        return self.update(det_hold, count_hold, tid, slot, stream_of, flush)

    def _redact(self, frames, rel, tails, out):
        from yolov6.utils.redact import redact_plates_np
        kw = dict(mode=self.mode, cell=self.cell, margin=self.margin, fill=self.fill, sigma=self.sigma)
        rel_det, rel_count, _, tail_det, tail_count, _ = out
        done = []
        if rel:
            red = redact_plates_np([fr for _, _, _, fr in rel], rel_det[[b for b, _, _, _ in rel]], rel_count[[b for b, _, _, _ in rel]], **kw)[0]
            done += [(s, g, fr) for (_, s, g, _), fr in zip(rel, red)]
        for s, items in tails:
            if items:
                red = redact_plates_np([fr for _, fr in items], tail_det[s], tail_count[s], **kw)[0]
                done += [(s, g, fr) for (g, _), fr in zip(items, red)]
        return done
