"""Redaction delayed by a few frames, so that the frames before a plate's first detection are covered too (lp_lookback_update;
yolov6/utils/lookback.py states the rule)."""
import numpy as np
import torch

from yolov6.hip import abi
from yolov6.utils.lookback import LookbackHost
from yolov6.utils.nv12 import Nv12Frame

from ._base import _dptr, _persistent, _stream_ptr
from .redact import redact_plates
from .tracker import PlateTracker, _host_lists, _zero_streams


class LookbackRedactor(LookbackHost):
    """Redaction delayed by ``depth`` frames, so that the frames BEFORE a plate's first detection are covered too
    (lp_lookback_update; ``yolov6.utils.lookback`` states the rule, and ``LookbackNp`` there is the same object on numpy).  It
    needs a ``PlateTracker`` with ``enable_hold`` called (RuntimeError otherwise).  ``max_back``: frames before the first detection
    that are covered (default ``depth``); ``back_cap``: back rows a stored frame can take (default ``max_tracks``); ``mode``,
    ``cell``, ``margin``, ``fill``, ``sigma``: as ``redact_plates``.

    ``push(frames, stream_of, flush)`` right after ``tracker.update(...)`` / ``update_with_shots(...)`` of the same frames
    enqueues lp_lookback_update on ``tracker.last_hold``, ``last_tid`` and ``slot_buffer`` and keeps REFERENCES to the frames per
    stream (BGR device tensors or ``Nv12Frame``s; no copy: the caller hands them over and must not write them until they come
    back), then redacts every frame that leaves the delay in this call with the rows released for it, one ``redact_plates`` call
    per push (plus one per flushed stream), and returns them as [(stream, frame_number, frame), ...] in release order; an
    untracked frame comes back at once as (-1, -2, frame).  Which frame leaves at which b follows from the host's own
    per-stream counters: no host read, and no allocation in the steady state (persistent buffers per update shape).
    ``flush`` / ``flush_all()`` hand the tail frames back the same way.

    Crops and best shots read the frames at update time, before any redaction of them is enqueued, so the order rule
    "redaction goes last" holds by construction."""

    def __init__(self, tracker, depth, max_back=None, back_cap=None, mode='mosaic', cell=16, margin=0.1, fill=(0, 0, 0), sigma=None):
        if not isinstance(tracker, PlateTracker):
            raise TypeError('LookbackRedactor needs a PlateTracker (LookbackNp is the CPU form)')
        self._init_host(tracker, depth, max_back, back_cap, mode, cell, margin, fill, sigma)
        self.device = tracker.device
        self.state = None          # allocated by the first push: the entries' rows follow max_det
        self._rows = None
        self._out, self._status, self._blank = {}, {}, {}

    def _slots(self):
        B, hold_rows = self.tracker.last_hold[0].shape[:2]
        return self.tracker.slot_buffer(B, hold_rows - self.max_tracks)

    def _allocated(self):
        return self.state is not None

    @property
    def entry_rows(self):
        """Rows of a stored entry (max_det + max_tracks + back_cap); None before the first push with frames."""
        return self._rows

    def _state_for(self, rows):
        if self.state is None:
            nbytes = abi.load().lp_lookback_state_bytes(self.n_streams, self.max_tracks, self.depth, rows)
            if nbytes == 0:
                raise ValueError('lookback: entries of %d rows do not fit (rows * 28 must stay below 2^31)' % rows)
            self._rows = rows
            self.state = torch.zeros(nbytes // 4, dtype=torch.int32, device=self.device)
        elif rows != self._rows:
            raise ValueError('this delay line holds entries of %d rows, the update has %d' % (self._rows, rows))
        return self.state

    def buffers(self, B, rows):
        """The persistent outputs of a push behind an update of B frames: (rel_det [B,rows,28], rel_count [B], rel_frame [B],
        tail_det [S,D,rows,28], tail_count [S,D], tail_frame [S,D])."""
        key, S, D, dev = (int(B), int(rows)), self.n_streams, self.depth, self.device

        def make():                             # the tails do not depend on B: every shape shares the first one's
            tails = next(iter(self._out.values()))[3:] if self._out else (
                torch.empty(S, D, key[1], abi.LP_DET_COLS, dtype=torch.float32, device=dev),
                torch.empty(S, D, dtype=torch.int32, device=dev), torch.empty(S, D, dtype=torch.int32, device=dev))
            return (torch.empty(key[0], key[1], abi.LP_DET_COLS, dtype=torch.float32, device=dev),
                    torch.empty(key[0], dtype=torch.int32, device=dev), torch.empty(key[0], dtype=torch.int32, device=dev)) + tuple(tails)
        return _persistent(self._out, key, make)

    def reset(self, streams=None):
        """Zero the state of ``streams`` (all for None) and forget their frames; use it together with ``PlateTracker.reset``."""
        if self.state is not None:
            _zero_streams(self.state, self.n_streams, streams)
        self._reset_host(streams)

    @property
    def dropped(self):
        """int32 [n_streams] on the host: the back rows that found no room since the last reset (a host read, outside the hot
        path)."""
        if self.state is None:
            return np.zeros(self.n_streams, np.int32)
        return self.state.view(self.n_streams, -1)[:, 2].cpu().numpy()

    def _update(self, det_hold, count_hold, tid, slot, stream_of, flush):
        B, hold_rows, max_det, S = det_hold.shape[0], det_hold.shape[1], tid.shape[1], self.n_streams
        if B == 0 and self.state is not None:
            hold_rows, max_det = self._rows - self.back_cap, 1      # a call without frames (a flush) takes the entries as they are
        rows = hold_rows + self.back_cap
        state = self._state_for(rows)
        out = self.buffers(B, rows)
        so, fl = _host_lists(stream_of, B, flush)
        with torch.cuda.device(self.device):
            abi.check(abi.load().lp_lookback_update(_dptr(state), S, self.max_tracks, self.depth, self.max_back, self.back_cap,
                                                    _dptr(det_hold), _dptr(count_hold), _dptr(tid), _dptr(slot), B, max_det, hold_rows,
                                                    so, fl, _dptr(out[0]), _dptr(out[1]), _dptr(out[2]),
                                                    _dptr(out[3]), _dptr(out[4]), _dptr(out[5]), _stream_ptr(self.device)),
                      'lp_lookback_update')
        return out

    def _blank_like(self, frame):
        """A scratch frame of the kind of ``frame`` for a slot of the redact call that has no frame (its count is 0)."""
        key = frame.matrix if isinstance(frame, Nv12Frame) else None
        blank = self._blank.get(key)
        if blank is None:
            if key is None:
                blank = torch.zeros(1, 1, 3, dtype=torch.uint8, device=self.device)
            else:
                blank = Nv12Frame.from_packed(torch.zeros(6, dtype=torch.uint8, device=self.device), 2, 2, key)
            self._blank[key] = blank
        return blank

    def _status_for(self, n, rows):
        return _persistent(self._status, (n, rows), lambda: torch.empty(n, rows, dtype=torch.int32, device=self.device))

    def _redact(self, frames, rel, tails, out):
        kw = dict(mode=self.mode, cell=self.cell, margin=self.margin, fill=self.fill, sigma=self.sigma)
        rel_det, rel_count, _, tail_det, tail_count, _ = out
        B, rows = rel_det.shape[:2]
        if rel:
            # one call over all B slots: slot b takes the frame that leaves at b; a slot that releases nothing has rel_count 0
            # and takes frame b itself (no byte changes), or a scratch frame where there is none
            # (a frame that enters and leaves within this push is in the list twice, at its own b with count 0 and at the b
            # that releases it: redact_plates reads and writes a frame only along its rows, so the count-0 entry touches nothing)
            leaving = {b: fr for b, _, _, fr in rel}
            lst = [leaving.get(b, frames[b]) for b in range(B)]
            lst = [self._blank_like(rel[0][3]) if fr is None else fr for fr in lst]
            redact_plates(lst, rel_det, rel_count, status=self._status_for(B, rows), **kw)
        done = [(s, g, fr) for _, s, g, fr in rel]
        for s, items in tails:
            if items:
                redact_plates([fr for _, fr in items], tail_det[s], tail_count[s], status=self._status_for(len(items), rows), **kw)
                done += [(s, g, fr) for g, fr in items]
        return done
