"""One denoised picture per plate track, on the CPU: ``StackNp`` is the written-down specification of ``lp_stack_update``
(include/lp_hip.h, csrc/lp_stack.hip), which matches it bit for bit, and the CPU path of ``Inferer(track=True, best_shots=True,
stack_shots=True)``.  The rectified crops a track shows are aligned by a small integer shift and averaged: n crops divide the
noise variance by n.  All arithmetic is integer, apart from the gallery's fp32 score and one fp32 subtraction.

The reference has nothing here: its Inferer treats video frames independently (yolov6/core/inferer.py).

The stack holds, per stream, its own frame counter and one entry per tracker slot: id + 1 (0 = empty), n (crops summed so far),
first_frame, last_frame and acc, uint16 [Hc, Wc, 3], the sum of the n aligned crops.  ``update`` is called with what the
tracker, the crop kernel and the sharpness kernel made of the same frames (the arguments of ``BestShotNp.update``).  Per stream,
frames in ascending b (``stream_of`` -1: skipped):
  1. rows r < min(max(count, 0), max_det, max_crops, MAX_DETS) with tid[r] >= 0 take part, in ascending r, g = slot[r] (a row
     whose slot is outside 0..max_tracks-1 is skipped);
  2. if entry g holds another id it is retired (5); an entry that does not hold id becomes {id + 1, n = 0};
  3. the row is eligible iff status[r] == 1 (a crop cut along the box is not rectified and is never mixed in), (double)score >=
     min_score with score = (c12 + ... + c19) / 8.0f summed left to right in fp32 (false for NaN), (double)(det[2] - det[0]) >=
     min_width, one fp32 subtraction (false for NaN: the plate's width in frame pixels, which keeps the small upsampled crops
     of an entering car out of the mean), sharp[r] >= min_sharp, and the entry's n < max_frames;
  4. align: y(p) = 29 B + 150 G + 77 R, un-rounded.  With n == 0, search == 0, Hc <= 2 search or Wc <= 2 search the shift d is
     (0, 0).  Otherwise the candidates (dy, dx) of [-search, search]^2 are numbered k = 0.. in the order of (dy^2 + dx^2, dy,
     dx) (``stack_candidates``; k = 0 is (0, 0)), cost_k = the sum over i in [R, Hc-R), j in [R, Wc-R) of
     | n * y(crop[i+dy, j+dx]) - y(acc[i, j]) | (the new crop against the running SUM, no division; n * y <= 254 * 65280 < 2^24,
     the sum over a 1024 x 1024 crop needs 44 bits: unsigned 64-bit), and d is the candidate of the smallest (cost, k).
     accumulate: acc[i, j, c] += crop[clamp(i+dy, 0, Hc-1), clamp(j+dx, 0, Wc-1), c] (an entry with n == 0 starts from zero),
     n += 1, first_frame is set when n was 0, last_frame = the stream's frame counter.  255 * 255 = 65025 fits uint16: that is
     why max_frames <= 255;
  5. retire entry g: e = the first index < min(ended_count[s], max_ended) with ended_i[s, e, 0] == the entry's id; if there is
     one and n >= 1: stack_crops[s, e] = (acc + (n >> 1)) // n per channel, stack_i[s, e] = (n, first_frame, last_frame, 1).
     Either way the entry becomes empty (id + 1 = 0, n = 0; an occupant whose record was cut off by max_ended is dropped
     silently);
  6. the stream's frame counter goes up.  After the stream's last frame (also for a stream without frames in the call) every
     non-empty entry whose id is among the call's records is retired, in slot order.  Live tracks stay.
stack_i is zero for every line at the start of a call; the crop of a line without a stack is left as it was.

What the rule does not do: the alignment is an integer translation of at most ``search`` pixels, with no rotation, scale or
sub-pixel step (the crops are already rectified along their predicted corners); every frame has the same weight; a track whose
plate really changes (an occlusion, a wiper) is averaged through it; ``min_sharp`` compares Laplacian energies, which sensor
noise raises as focus does, so a value is not comparable across cameras.
"""
import numpy as np

from yolov6.utils.best_shot import crop_sharpness_np
from yolov6.utils.plate_crop import plate_crops_np
from yolov6.utils.track import DET_COLS, MAX_DETS, MAX_TRACKS

f32 = np.float32
MAX_SEARCH, MAX_FRAMES = 4, 255


def stack_candidates(R):
    """The (dy, dx) of [-R, R]^2 in the order of (dy^2 + dx^2, dy, dx): candidate k of the alignment search."""
    R = int(R)
    if not 0 <= R <= MAX_SEARCH:
        raise ValueError('search must be in 0..%d' % MAX_SEARCH)
    return sorted(((dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)), key=lambda d: (d[0] * d[0] + d[1] * d[1], d[0], d[1]))


def check_params(search=2, max_frames=64, min_width=0.0, min_sharp=0, min_score=0.0):
    """The checked (search, max_frames, min_width, min_sharp, min_score) of a stack; raises ValueError."""
    if int(search) != search or not 0 <= int(search) <= MAX_SEARCH:
        raise ValueError('search must be an integer in 0..%d' % MAX_SEARCH)
    if int(max_frames) != max_frames or not 1 <= int(max_frames) <= MAX_FRAMES:
        raise ValueError('max_frames must be an integer in 1..%d (255 * 255 fits the 16-bit sum)' % MAX_FRAMES)
    if not abs(float(min_width)) <= 3.0e38:
        raise ValueError('min_width must be finite (|min_width| <= 3e38)')
    if not abs(float(min_score)) <= 3.0e38:
        raise ValueError('min_score must be finite (|min_score| <= 3e38)')
    if int(min_sharp) != min_sharp or not 0 <= int(min_sharp) < 2 ** 64:
        raise ValueError('min_sharp must be an integer in 0..2^64-1')
    return int(search), int(max_frames), float(min_width), int(min_sharp), float(min_score)


def luma(px):
    """int64 [...]: 29 B + 150 G + 77 R of [..., 3] BGR values, un-rounded."""
    px = np.asarray(px).astype(np.int64)
    return 29 * px[..., 0] + 150 * px[..., 1] + 77 * px[..., 2]


def align_costs(crop, acc, n, R):
    """The costs of rule 4 as Python integers, one per candidate of ``stack_candidates(R)`` (the interior must not be empty)."""
    Hc, Wc = crop.shape[:2]
    yc, ya = int(n) * luma(crop), luma(acc)[R:Hc - R, R:Wc - R]
    return [int(np.abs(yc[R + dy:Hc - R + dy, R + dx:Wc - R + dx] - ya).sum()) for dy, dx in stack_candidates(R)]


def shift_clamped(crop, dy, dx):
    """crop[clamp(i + dy), clamp(j + dx)] for every (i, j)."""
    Hc, Wc = crop.shape[:2]
    return crop[np.clip(np.arange(Hc) + dy, 0, Hc - 1)][:, np.clip(np.arange(Wc) + dx, 0, Wc - 1)]


class StackNp:
    """The stacks of ``n_streams`` trackers of ``max_tracks`` slots each for crops of ``crop_hw`` (the module docstring states
    the rules and what they do not do)."""

    def __init__(self, n_streams, max_tracks, crop_hw, search=2, max_frames=64, min_score=0.0, min_width=0.0, min_sharp=0):
        Hc, Wc = (int(v) for v in crop_hw)
        if int(n_streams) < 1:
            raise ValueError('n_streams must be >= 1')
        if not 1 <= int(max_tracks) <= MAX_TRACKS:
            raise ValueError('max_tracks must be in 1..%d' % MAX_TRACKS)
        if not (1 <= Hc <= 1024 and 1 <= Wc <= 1024):
            raise ValueError('crop size %dx%d: need 1..1024 on each side' % (Hc, Wc))
        self.search, self.max_frames, self.min_width, self.min_sharp, self.min_score = check_params(search, max_frames, min_width, min_sharp,
                                                                                                    min_score)
        self.n_streams, self.max_tracks, self.crop_hw = int(n_streams), int(max_tracks), (Hc, Wc)
        S, T = self.n_streams, self.max_tracks
        self.frame = np.zeros(S, np.int32)
        self.idp1 = np.zeros((S, T), np.int32)          # id + 1, 0 = empty
        self.n = np.zeros((S, T), np.int32)
        self.first = np.zeros((S, T), np.int32)
        self.last = np.zeros((S, T), np.int32)
        self.acc = np.zeros((S, T, Hc, Wc, 3), np.uint16)
        #: counters for tests and diagnostics (no part of the state): crops summed, those with a shift other than (0, 0), eligible
        #: rows but for a full entry, entries retired because their slot was reused / at the end of a call, records handed out with
        #: / without a stack, occupants dropped because their record was cut off
        self.stats = dict(summed=0, shifted=0, full=0, reused=0, closed=0, with_stack=0, without_stack=0, truncated=0)
        #: (stream, slot, id, dy, dx) of every crop the last ``update`` summed, in order (no part of the state)
        self.shifts = []

    _ARRAYS = ('frame', 'idp1', 'n', 'first', 'last', 'acc')

    def reset(self, streams=None):
        """Empty the stacks of ``streams`` (all for None), frame counter at 0."""
        for s in (range(self.n_streams) if streams is None else streams):
            for name in self._ARRAYS:
                getattr(self, name)[s] = 0

    def _retire(self, s, g, ids, out):
        stack_crops, stack_i = out
        hit = np.nonzero(ids == self.idp1[s, g] - 1)[0]
        n = int(self.n[s, g])
        if not len(hit):
            self.stats['truncated'] += 1
        elif n >= 1:
            e = hit[0]
            stack_crops[s, e] = ((self.acc[s, g].astype(np.uint32) + np.uint32(n >> 1)) // np.uint32(n)).astype(np.uint8)
            stack_i[s, e] = (n, self.first[s, g], self.last[s, g], 1)
            self.stats['with_stack'] += 1
        else:
            self.stats['without_stack'] += 1
        self.idp1[s, g] = self.n[s, g] = 0              # (first, last and acc keep what they held: n == 0 starts from zero)

    def _align(self, crop, acc, n):
        R, (Hc, Wc) = self.search, self.crop_hw
        if n == 0 or R == 0 or Hc <= 2 * R or Wc <= 2 * R:
            return 0, 0
        costs = align_costs(crop, acc, n, R)
        return stack_candidates(R)[min(range(len(costs)), key=lambda k: (costs[k], k))]

    def update_from_frames(self, frames, det, count, tid, slot, stream_of, ended_i, ended_count, max_crops=16, stack_crops=None):
        """``update`` behind ``plate_crops_np`` and ``crop_sharpness_np`` (``BestShotNp.update_from_frames`` states the cut)."""
        det = np.ascontiguousarray(det, dtype=f32)
        B, max_det = det.shape[:2]
        stream_of = list(range(B)) if stream_of is None else [int(v) for v in stream_of]
        frames = list(frames) + [None] * (B - len(frames))
        crops = np.zeros((B, int(max_crops)) + self.crop_hw + (3,), np.uint8)
        status = np.zeros((B, int(max_crops)), np.int32)
        for b in range(B):
            n = min(max(int(np.asarray(count).reshape(-1)[b]), 0), max_det, int(max_crops))
            if stream_of[b] >= 0 and n:
                if frames[b] is None:
                    raise ValueError('frame %d of stream %d is missing' % (b, stream_of[b]))
                crops[b, :n], status[b, :n] = plate_crops_np(frames[b], det[b, :n], self.crop_hw)
        return self.update(det, count, tid, slot, crops, status, crop_sharpness_np(crops, status), stream_of, ended_i, ended_count, stack_crops)

    def update(self, det, count, tid, slot, crops, status, sharp, stream_of, ended_i, ended_count, stack_crops=None):
        """The arguments of ``BestShotNp.update``.  Returns (stack_crops [S,max_ended,Hc,Wc,3] uint8, stack_i [S,max_ended,4]
        int32 = n, first_frame, last_frame, valid), line-parallel to the records; ``stack_crops``: an array to write into (the
        crops of records without a stack are left as they were), zeros by default."""
        det = np.ascontiguousarray(det, dtype=f32)
        if det.ndim != 3 or det.shape[2] != DET_COLS or det.shape[1] < 1:
            raise ValueError('det must be [B, max_det >= 1, 28]')
        B, max_det = det.shape[:2]
        S, T, (Hc, Wc) = self.n_streams, self.max_tracks, self.crop_hw
        count = np.asarray(count).astype(np.int64).reshape(-1)
        tid, slot = np.asarray(tid).astype(np.int64), np.asarray(slot).astype(np.int64)
        crops, status = np.asarray(crops), np.asarray(status).astype(np.int64)
        sharp = np.asarray(sharp).astype(np.uint64)
        ended_i, ended_count = np.asarray(ended_i), np.asarray(ended_count).astype(np.int64).reshape(-1)
        if len(count) != B or tid.shape != (B, max_det) or slot.shape != (B, max_det):
            raise ValueError('count must be [B], tid and slot [B, max_det]')
        if crops.dtype != np.uint8 or crops.ndim != 5 or crops.shape[0] != B or crops.shape[2:] != (Hc, Wc, 3):
            raise ValueError('crops must be uint8 [B, max_crops, %d, %d, 3]' % (Hc, Wc))
        max_crops = crops.shape[1]
        if status.shape != (B, max_crops) or sharp.shape != (B, max_crops):
            raise ValueError('status and sharp must be [B, max_crops]')
        if ended_i.ndim != 3 or ended_i.shape[0] != S or ended_i.shape[2] != 12 or len(ended_count) != S:
            raise ValueError('ended_i must be [n_streams, max_ended, 12] and ended_count [n_streams]')
        max_ended = ended_i.shape[1]
        stream_of = list(range(B)) if stream_of is None else [int(v) for v in stream_of]
        if len(stream_of) != B or not all(-1 <= s < S for s in stream_of):
            raise ValueError('stream_of must name the stream (-1: skip, or 0..%d) of each of the %d frames' % (S - 1, B))
        if stack_crops is None:
            stack_crops = np.zeros((S, max_ended, Hc, Wc, 3), np.uint8)
        elif stack_crops.shape != (S, max_ended, Hc, Wc, 3) or stack_crops.dtype != np.uint8:
            raise ValueError('stack_crops must be uint8 [n_streams, max_ended, Hc, Wc, 3]')
        out = (stack_crops, np.zeros((S, max_ended, 4), np.int32))
        ids = [ended_i[s, :min(max(int(ended_count[s]), 0), max_ended), 0] for s in range(S)]
        self.shifts = []
        for b, s in enumerate(stream_of):
            if s < 0:
                continue
            for r in range(min(max(int(count[b]), 0), max_det, max_crops, MAX_DETS)):
                t, g = int(tid[b, r]), int(slot[b, r])
                if t < 0 or not 0 <= g < T:
                    continue
                if self.idp1[s, g] != t + 1:
                    if self.idp1[s, g] != 0:
                        self.stats['reused'] += 1
                        self._retire(s, g, ids[s], out)
                    self.idp1[s, g], self.n[s, g] = t + 1, 0
                row = det[b, r]
                with np.errstate(all='ignore'):
                    score = row[12] + row[13]
                    for c in range(14, 20):
                        score = score + row[c]
                    score = score / f32(8.0)
                    width = row[2] - row[0]
                if status[b, r] != 1 or not np.float64(score) >= self.min_score or not np.float64(width) >= self.min_width \
                        or not int(sharp[b, r]) >= self.min_sharp:
                    continue
                n = int(self.n[s, g])
                if n >= self.max_frames:
                    self.stats['full'] += 1
                    continue
                dy, dx = self._align(crops[b, r], self.acc[s, g], n)
                moved = shift_clamped(crops[b, r], dy, dx).astype(np.uint16)
                if n == 0:
                    self.acc[s, g], self.first[s, g] = moved, self.frame[s]
                else:
                    self.acc[s, g] += moved
                self.n[s, g], self.last[s, g] = n + 1, self.frame[s]
                self.stats['summed'] += 1
                self.stats['shifted'] += int((dy, dx) != (0, 0))
                self.shifts.append((s, g, t, dy, dx))
            self.frame[s] += 1
        for s in range(S):
            for g in range(T):
                if self.idp1[s, g] != 0 and (ids[s] == self.idp1[s, g] - 1).any():
                    self.stats['closed'] += 1
                    self._retire(s, g, ids[s], out)
        return out
