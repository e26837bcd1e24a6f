"""The best shot of every plate track, on the CPU: ``crop_sharpness_np`` and ``BestShotNp`` are the written-down specification
of ``lp_crop_sharpness`` and ``lp_best_shot_update`` (include/lp_hip.h, csrc/lp_shots.hip), which match them bit for bit, and
the CPU path of ``Inferer(track=True, best_shots=True)``.  All arithmetic is integer.

The reference has nothing here: its Inferer treats video frames independently (yolov6/core/inferer.py).

Sharpness of a crop [Hc, Wc, 3] uint8 BGR with status 1 or 2: g = (29 B + 150 G + 77 R + 128) >> 8 per pixel,
L = 4 g(i,j) - g(i-1,j) - g(i+1,j) - g(i,j-1) - g(i,j+1) on the interior pixels, sharp = sum of L * L as an unsigned 64-bit
integer; 0 for status 0 or 3 or a side shorter than 3.  Sensor noise raises the measure as focus does: it ranks the frames of
one track and is not comparable across cameras.

The gallery holds, per stream, its own frame counter and one entry per tracker slot: id + 1 (0 = empty), a has-shot flag, a
64-bit key, the frame, row and status of the shot, its det row and its crop.  ``update`` is called with what the tracker, the
crop kernel and the sharpness kernel made of the same frames.  Per stream, frames in ascending b (``stream_of`` -1: skipped):
  1. rows r < min(max(count, 0), max_det, max_crops, MAX_DETS) with tid[r] >= 0 take part, g = slot[r] (a row whose slot is
     outside 0..max_tracks-1 is skipped);
  2. if entry g holds another id it is retired (5); an entry that does not hold id becomes {id + 1, no shot};
  3. the row is eligible iff status[r] is 1 or 2 and (double)score >= min_score, score = (c12 + ... + c19) / 8.0f summed left to
     right in fp32 as the tracker's rule 6 (false for NaN);
  4. key = ((status == 1) << 63) | sharp[r]: a crop cut along the corners beats one cut along the box.  The row becomes the
     entry's shot iff the entry has none or key > the entry's key (strict: the earlier frame keeps a tie); that copies the crop,
     the det row, the stream's frame counter, r, status and key;
  5. retire entry g: e = the first index < min(ended_count[s], max_ended) with ended_i[s, e, 0] == the entry's id; if there is
     one and the entry has a shot: shot_crops[s, e] = its crop, shot_i[s, e] = (frame, row, status, 1), shot_q[s, e] = the key
     without its top bit, shot_det[s, e] = its det row.  Either way the entry becomes empty (an occupant whose record was cut
     off by max_ended is dropped silently);
  6. the stream's frame counter goes up.  After the stream's last frame (also for a stream without frames in the call) every
     non-empty entry whose id is among the call's records is retired, in slot order.  Live tracks stay.
"""
import numpy as np

from yolov6.utils.plate_crop import plate_crops_np
from yolov6.utils.track import DET_COLS, MAX_DETS, MAX_TRACKS

f32 = np.float32
TOP = np.uint64(1) << np.uint64(63)


def crop_sharpness_np(crops, status=None):
    """uint64 [...] Laplacian energy of ``crops`` uint8 [..., Hc, Wc, 3] (BGR); ``status`` int [...] (default: all 1) as
    ``plate_crops`` returns it: slots with status 0 or 3 give 0."""
    crops = np.asarray(crops)
    if crops.dtype != np.uint8 or crops.ndim < 3 or crops.shape[-1] != 3:
        raise ValueError('crops must be uint8 [..., Hc, Wc, 3]')
    lead, (Hc, Wc) = crops.shape[:-3], crops.shape[-3:-1]
    status = np.ones(lead, np.int64) if status is None else np.asarray(status).astype(np.int64)
    if status.shape != lead:
        raise ValueError('status must have the shape %s of the crop slots' % (lead,))
    out = np.zeros(lead, np.uint64)
    if Hc < 3 or Wc < 3 or not out.size:
        return out
    c = crops.astype(np.int64)
    g = (29 * c[..., 0] + 150 * c[..., 1] + 77 * c[..., 2] + 128) >> 8
    lap = 4 * g[..., 1:-1, 1:-1] - g[..., :-2, 1:-1] - g[..., 2:, 1:-1] - g[..., 1:-1, :-2] - g[..., 1:-1, 2:]
    total = (lap * lap).sum(axis=(-2, -1)).astype(np.uint64)
    return np.where((status == 1) | (status == 2), total, np.uint64(0)).astype(np.uint64)


class BestShotNp:
    """The gallery of ``n_streams`` trackers of ``max_tracks`` slots each for crops of ``crop_hw`` (the module docstring states
    the rules)."""

    def __init__(self, n_streams, max_tracks, crop_hw, min_score=0.0):
        Hc, Wc = (int(v) for v in crop_hw)
        if int(n_streams) < 1:
            raise ValueError('n_streams must be >= 1')
        if not 1 <= int(max_tracks) <= MAX_TRACKS:
            raise ValueError('max_tracks must be in 1..%d' % MAX_TRACKS)
        if not (1 <= Hc <= 1024 and 1 <= Wc <= 1024):
            raise ValueError('crop size %dx%d: need 1..1024 on each side' % (Hc, Wc))
        if not abs(min_score) <= 3.0e38:
            raise ValueError('min_score must be finite (|min_score| <= 3e38)')
        self.n_streams, self.max_tracks, self.crop_hw, self.min_score = int(n_streams), int(max_tracks), (Hc, Wc), float(min_score)
        S, T = self.n_streams, self.max_tracks
        self.frame = np.zeros(S, np.int32)
        self.idp1 = np.zeros((S, T), np.int32)          # id + 1, 0 = empty
        self.has = np.zeros((S, T), np.int32)
        self.key = np.zeros((S, T), np.uint64)
        self.meta = np.zeros((S, T, 3), np.int32)       # frame, row, status of the shot
        self.det = np.zeros((S, T, DET_COLS), f32)
        self.crop = np.zeros((S, T, Hc, Wc, 3), np.uint8)
        #: counters for tests and diagnostics (no part of the state): first shots taken, shots replaced by a sharper one, rows
        #: that lost on an equal key, entries retired because their slot was reused / at the end of a call, records handed
        #: out with / without a shot, occupants dropped because their record was cut off
        self.stats = dict(taken=0, replaced=0, ties=0, reused=0, closed=0, with_shot=0, without_shot=0, truncated=0)

    _ARRAYS = ('frame', 'idp1', 'has', 'key', 'meta', 'det', 'crop')

    def reset(self, streams=None):
        """Empty the gallery of ``streams`` (all for None), frame counter at 0."""
        for s in (range(self.n_streams) if streams is None else streams):
            for name in self._ARRAYS:
                getattr(self, name)[s] = 0

    def _retire(self, s, g, ids, out):
        shot_crops, shot_i, shot_q, shot_det = out
        hit = np.nonzero(ids == self.idp1[s, g] - 1)[0]
        if not len(hit):
            self.stats['truncated'] += 1
        elif self.has[s, g]:
            e = hit[0]
            shot_crops[s, e] = self.crop[s, g]
            shot_i[s, e] = (*self.meta[s, g], 1)
            shot_q[s, e] = self.key[s, g] & ~TOP
            shot_det[s, e] = self.det[s, g]
            self.stats['with_shot'] += 1
        else:
            self.stats['without_shot'] += 1
        self.idp1[s, g] = self.has[s, g] = 0

    def update_from_frames(self, frames, det, count, tid, slot, stream_of, ended_i, ended_count, max_crops=16, shot_crops=None):
        """``update`` behind ``plate_crops_np`` and ``crop_sharpness_np``: the CPU form of ``PlateTracker.update_with_shots``.
        ``frames[b]``: uint8 [h, w, 3] BGR (may be missing or None where ``stream_of`` is -1: such a frame takes no crops); frame
        b is cut along its rows r < min(max(count, 0), max_det, max_crops) of ``det``."""
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
        return self.update(det, count, tid, slot, crops, status, crop_sharpness_np(crops, status), stream_of, ended_i, ended_count, shot_crops)

    def update(self, det, count, tid, slot, crops, status, sharp, stream_of, ended_i, ended_count, shot_crops=None):
        """det [B,max_det,28] fp32 + count [B] (the rows given to the tracker), tid / slot [B,max_det] and ended_i
        [S,max_ended,12] / ended_count [S] as that tracker update left them, crops [B,max_crops,Hc,Wc,3] uint8, status / sharp
        [B,max_crops]; ``stream_of`` as given to the tracker (None: ``range(B)``).  Returns (shot_crops [S,max_ended,Hc,Wc,3]
        uint8, shot_i [S,max_ended,4] int32 = frame, row, status, valid, shot_q [S,max_ended] uint64, shot_det [S,max_ended,28]
        fp32), line-parallel to the records; ``shot_crops``: an array to write into (the crops of records without a shot are left
        as they were), zeros by default."""
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
        if shot_crops is None:
            shot_crops = np.zeros((S, max_ended, Hc, Wc, 3), np.uint8)
        elif shot_crops.shape != (S, max_ended, Hc, Wc, 3) or shot_crops.dtype != np.uint8:
            raise ValueError('shot_crops must be uint8 [n_streams, max_ended, Hc, Wc, 3]')
        out = (shot_crops, np.zeros((S, max_ended, 4), np.int32), np.zeros((S, max_ended), np.uint64),
               np.zeros((S, max_ended, DET_COLS), f32))
        ids = [ended_i[s, :min(max(int(ended_count[s]), 0), max_ended), 0] for s in range(S)]
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
                    self.idp1[s, g], self.has[s, g] = t + 1, 0
                row = det[b, r]
                with np.errstate(all='ignore'):
                    score = row[12] + row[13]
                    for c in range(14, 20):
                        score = score + row[c]
                    score = score / f32(8.0)
                if status[b, r] not in (1, 2) or not np.float64(score) >= self.min_score:
                    continue
                key = (TOP if status[b, r] == 1 else np.uint64(0)) | sharp[b, r]
                if self.has[s, g] and not key > self.key[s, g]:
                    self.stats['ties'] += int(key == self.key[s, g])
                    continue
                self.stats['replaced' if self.has[s, g] else 'taken'] += 1
                self.has[s, g], self.key[s, g] = 1, key
                self.meta[s, g] = (self.frame[s], r, status[b, r])
                self.det[s, g], self.crop[s, g] = row, crops[b, r]
            self.frame[s] += 1
        for s in range(S):
            for g in range(T):
                if self.idp1[s, g] != 0 and (ids[s] == self.idp1[s, g] - 1).any():
                    self.stats['closed'] += 1
                    self._retire(s, g, ids[s], out)
        return out
