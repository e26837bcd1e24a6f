"""A log of sightings: every read that ends is matched against the recent reads of all streams, then remembered.
``sight_update_np`` is the written-down specification of ``lp_sight_update`` (include/lp_hip.h, csrc/lp_sight.hip), which matches
it on every int32 of its output and of the log, and ``SightLogNp`` is the CPU path of ``Inferer(track=True, sightings=...)``.  All
arithmetic is integer except one fp32 product per position of a read; every reduction (the minimum of a key, an integer count) is
independent of its order, so the result is reproducible bit for bit by construction.

The reference has nothing here: its Inferer treats frames independently (yolov6/core/inferer.py).

The watchlist (``yolov6.utils.watch``) relates a read to a fixed list.  This relates a read to earlier reads: the car that the exit
camera reads now is the car the entry camera read 40 minutes ago (journey time, billing, "has it been here today"), and a plate
hidden for longer than the tracker's ``max_age`` that comes back as a new track is the track that ended a moment ago.  Both are one
operation on a ring of reads that the same call scans and then writes.

Rules:
  log: ``capacity`` C slots, 1 <= C <= MAX_CAPACITY (2^24), and a fixed number of streams S.  ``state`` int32 [1 + C, 8]; row 0 is
     the header (total, 0, 0, 0, 0, 0, 0, 0), total = the reads appended since the last clear; row 1 + slot holds w0, w1 = the eight
     ids as bytes (position p in byte p & 3 of word p >> 2), w2, w3 = the eight position weights minus 1 as bytes, w4 = stream,
     w5 = track id, w6 = stamp, w7 = seq = the value of total when the read was appended.  Append number t lives in slot t % C;
     all zero = empty; fill = min(total, C) slots are filled;
  call: ``ended_i`` / ``ended_f`` / ``ended_count`` exactly as ``watch_match_np`` takes them; ``now`` int32 >= 0, the caller's clock
     (seconds, a frame or call number: the log does not interpret it); ``window`` int32 >= 0; ``min_hits`` >= 1; ``max_mismatch``
     0..8; ``max_cost`` 0..32768 (``watch.cost_units`` converts a float); ``confuse`` in ``watch.check_confuse`` format or None;
     ``pair`` uint8 [S, S] or None: pair[s_read][s_entry] != 0 means that entries logged from stream s_entry are candidates for the
     reads of stream s_read (None: every pair, the same stream included);
  a read: a line j < min(max(ended_count[s], 0), max_ended) whose hits (ended_i[s, j, 3]) are >= min_hits.  Other lines are neither
     looked up nor appended; their output row is the empty row;
  match: every read is matched against the log as it stood before the call (the reads of one call do not see each other).  Per
     position p: q_r = ``watch.position_weight(share)``, q_e = the stored weight; id_r = best if 0 <= best < 64, else "matches
     nothing"; equal ids in 0..63 cost 0; anything else is one mismatch of cost min(q_r, q_e) * c, c = confuse[g(p)][id_r][id_e]
     when both ids are in 0..63, else 16 -- symmetric in the two uncertainties, because both sides are voted reads.  There are no
     wildcards.  An entry is accepted iff its slot is filled, ``pair`` allows it (with a ``pair``, a stored stream outside 0..S-1
     is allowed nowhere), 0 <= now - stamp <= window (the difference in 64 bits), mism <= max_mismatch and cost <= max_cost.
     Among the accepted entries the winner has the smallest (cost, age rank), age rank = total - 1 - seq: 0 is the newest;
  output: ``sight_i`` int32 [S, max_ended, 8], line-parallel to ended_i: (slot, mismatches, cost, n_hits, prev_stream, prev_id,
     prev_stamp, prev_seq), n_hits = the number of accepted entries; the empty row is EMPTY = (-1, 0, 0, 0, -1, -1, 0, 0).  The
     prev_* values are copied out, because the winning slot may be overwritten by this same call's appends;
  append: after all matching, read k of the call, in (stream, line) order over the reads, is append number total + k with stamp
     ``now``: a stored id is best if it is in 0..63, else NOTHING (254); a stored weight is q_r - 1; the track id is ended_i[s, j, 0].
     If the call has V > C reads only the last C are written.  total grows by V.

What it does not do: no insertions or deletions (the reads stay positional); one best earlier sighting plus a count, not a chain;
``now`` must not run backwards (entries stamped after ``now`` simply do not match); fewer than 2^31 appends between clears (the
wrappers keep a host-side upper bound and raise before it could be passed); the log survives ``PlateTracker.reset`` -- track ids
restart there, so prev_seq, not prev_id, is the unique name of a sighting.
"""
import numpy as np

from yolov6.utils import watch
from yolov6.utils.track import ENDED_COLS, HEADS, MAX_CLS

MAX_CAPACITY = 1 << 24
NOTHING = 254                 # the stored id of a position whose voted id is outside 0..63
WORDS = 8                     # int32 words of a row of the state and of sight_i
EMPTY = (-1, 0, 0, 0, -1, -1, 0, 0)
MAX_APPENDS = (1 << 31) - 1   # total stays below 2^31
f32 = np.float32
_I32_MAX = (1 << 31) - 1


def check_log(capacity, n_streams):
    """(capacity, n_streams) as integers (ValueError outside 1..2^24 / below 1)."""
    C, S = int(capacity), int(n_streams)
    if C != capacity or not 1 <= C <= MAX_CAPACITY:
        raise ValueError('capacity must be an integer in 1..%d' % MAX_CAPACITY)
    if S != n_streams or S < 1:
        raise ValueError('n_streams must be an integer >= 1')
    return C, S


def check_pair(pair, n_streams):
    """``pair`` as the uint8 [S, S] mask (None stays None); ValueError for another shape."""
    if pair is None:
        return None
    a = np.asarray(pair)
    if a.shape != (n_streams, n_streams) or a.dtype.kind not in 'iub':
        raise ValueError('pair must be integers [%d, %d]' % (n_streams, n_streams))
    return np.ascontiguousarray(a != 0, dtype=np.uint8)


def check_call(now, window, min_hits):
    """(now, window, min_hits) as the int32 of the rule (ValueError: now or window below 0, min_hits below 1, above 2^31 - 1)."""
    out = []
    for name, v, lo in (('now', now, 0), ('window', window, 0), ('min_hits', min_hits, 1)):
        i = int(v)
        if i != v or not lo <= i <= _I32_MAX:
            raise ValueError('%s must be an integer in %d..2^31-1' % (name, lo))
        out.append(i)
    return tuple(out)


def new_state(capacity):
    """The empty log of ``capacity`` slots: int32 [1 + C, 8] of zeros."""
    return np.zeros((1 + int(capacity), WORDS), np.int32)


def _bytes_of(words):
    """int64 [..., 8]: the bytes of the two little-endian int32 words [..., 2]."""
    w = np.ascontiguousarray(words, dtype=np.int32).view(np.uint32).astype(np.int64)
    return np.stack([(w[..., p >> 2] >> (8 * (p & 3))) & 255 for p in range(HEADS)], axis=-1)


def _words_of(b):
    """The two int32 words of eight bytes (int [8], 0..255)."""
    b = [int(v) for v in b]
    w = [sum(b[4 * k + i] << (8 * i) for i in range(4)) for k in range(2)]
    return [v - (1 << 32) if v >= (1 << 31) else v for v in w]


def sight_update_np(state, confuse, pair, ended_i, ended_f, ended_count, now, window, min_hits, max_mismatch, max_cost):
    """One call of the module's rule on ``state`` (int32 [1 + C, 8], updated in place): sight_i int32 [S, max_ended, 8].  Per read
    and position one table over the 256 byte values of a stored id gives the confusion weight, so a log of 10^5 slots with a few
    dozen reads takes well under a second."""
    if not isinstance(state, np.ndarray) or state.dtype != np.int32 or state.ndim != 2 or state.shape[1] != WORDS or len(state) < 2:
        raise ValueError('state must be an int32 array [1 + capacity, %d]' % WORDS)
    C = len(state) - 1
    if C > MAX_CAPACITY:
        raise ValueError('a log holds at most %d slots' % MAX_CAPACITY)
    confuse = watch.check_confuse(confuse)
    mm, mc = watch.check_params(max_mismatch, max_cost)
    now, window, min_hits = check_call(now, window, min_hits)
    ended_i, ended_f = np.asarray(ended_i, np.int32), np.asarray(ended_f, f32)
    ended_count = np.asarray(ended_count).astype(np.int64).reshape(-1)
    S, max_ended = ended_i.shape[:2]
    if ended_i.shape != (S, max_ended, ENDED_COLS) or ended_f.shape != ended_i.shape or len(ended_count) != S:
        raise ValueError('ended_i / ended_f must be [S, max_ended, %d] and ended_count [S]' % ENDED_COLS)
    pair = check_pair(pair, S)
    total = int(state[0, 0])
    if total < 0:
        raise ValueError('the header of the log holds a negative total')
    reads = [(s, j) for s in range(S) for j in range(min(max(int(ended_count[s]), 0), max_ended)) if int(ended_i[s, j, 3]) >= min_hits]
    if total + len(reads) > MAX_APPENDS:
        raise ValueError('the log takes fewer than 2^31 appends between clears')
    out = np.zeros((S, max_ended, WORDS), np.int32)
    out[:] = EMPTY
    fill = min(total, C)
    old = state[1:1 + fill].copy()                                     # the log as it stood before the call
    if fill:
        ids_e, q_e = _bytes_of(old[:, 0:2]), _bytes_of(old[:, 2:4]) + 1
        stream_e, seq_e = old[:, 4].astype(np.int64), old[:, 7].astype(np.int64)
        age = now - old[:, 6].astype(np.int64)
        in_window = (age >= 0) & (age <= window)
        rank = total - 1 - seq_e
        byte = np.arange(256)
    for s, j in reads if fill else ():
        best, q_r = ended_i[s, j, 4:12], watch.position_weight(ended_f[s, j, :HEADS])
        cost, mism = np.zeros(fill, np.int64), np.zeros(fill, np.int64)
        for p in range(HEADS):
            b = int(best[p])
            c = np.full(256, watch.FULL, np.int64)
            miss = np.ones(256, bool)
            if 0 <= b < MAX_CLS:
                c[:MAX_CLS] = confuse[watch.GROUP_OF[p], b]
                miss = byte != b
            w = ids_e[:, p]
            cost += np.where(miss[w], np.minimum(int(q_r[p]), q_e[:, p]) * c[w], 0)
            mism += miss[w]
        ok = in_window & (mism <= mm) & (cost <= mc)
        if pair is not None:
            inside = (stream_e >= 0) & (stream_e < S)
            ok &= inside & (pair[s][np.where(inside, stream_e, 0)] != 0)
        n = int(ok.sum())
        if n:
            key = np.where(ok, (cost << 32) | rank, np.int64(1) << 62)
            e = int(np.argmin(key))                                     # ranks are distinct: one smallest (cost, age rank)
            out[s, j] = (e, mism[e], cost[e], n, old[e, 4], old[e, 5], old[e, 6], old[e, 7])
    V = len(reads)
    for k in range(max(V - C, 0), V):
        s, j = reads[k]
        best, q_r = ended_i[s, j, 4:12], watch.position_weight(ended_f[s, j, :HEADS])
        ids = [int(b) if 0 <= int(b) < MAX_CLS else NOTHING for b in best]
        t = total + k
        state[1 + t % C] = _words_of(ids) + _words_of(q_r - 1) + [s, int(ended_i[s, j, 0]), now, t]
    state[0, 0] = total + V
    return out


class SightLogNp:
    """A log of sightings on the host: what ``PlateTrackerNp.enable_sightings`` takes (``runtime.SightLog`` is the device form).
    ``state``: int32 [1 + capacity, 8]; ``total``: the reads appended since the last ``clear``."""

    def __init__(self, capacity, n_streams, confuse=None, pair=None, device=None):
        self.capacity, self.n_streams = check_log(capacity, n_streams)
        self.confuse_np = None if confuse is None else watch.check_confuse(confuse)
        self.pair_np = check_pair(pair, self.n_streams)
        self.state = new_state(self.capacity)

    @property
    def total(self):
        return int(self.state[0, 0])

    def clear(self):
        """Empty the log."""
        self.state[:] = 0

    def update(self, ended_i, ended_f, ended_count, now, window, min_hits=1, max_mismatch=1, max_cost=None):
        """``sight_update_np`` on this log; ``max_cost`` a float in fully confident mismatches (``watch.cost_units``; None: no
        limit).  The streams of the records must be the log's."""
        if np.asarray(ended_i).shape[0] != self.n_streams:
            raise ValueError('the ended records must have the log\'s %d streams' % self.n_streams)
        return sight_update_np(self.state, self.confuse_np, self.pair_np, ended_i, ended_f, ended_count, now, window, min_hits,
                               max_mismatch, watch.cost_units(max_cost))
