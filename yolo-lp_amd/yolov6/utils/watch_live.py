"""Looking the reads of LIVE plate tracks up in a watchlist, on the CPU: ``LiveWatchNp`` is the written-down specification of
``lp_watch_live`` (include/lp_hip.h, csrc/lp_watch_live.hip), which matches it on every int32, and the CPU path of
``Inferer(track=True, watchlist=..., watch_live=True)``.

The reference has nothing here: its Inferer treats frames independently (yolov6/core/inferer.py).

``enable_watch`` looks a read up when its track has ENDED, ``max_age`` frames after the plate was last seen.  That is too late for a
car waiting in front of a barrier (its track does not end while it waits) and for a stolen vehicle (reported when it has left the
picture).  This module answers while the track lives, and a memo per tracker slot keeps the answer: a lookup is a scan of the whole
list, and a stream of 25 frames a second with a handful of cars must cause a handful of lookups per car, not 25 a second.

Parameters: ``min_hits`` >= 1 (default 3); ``max_mismatch``, ``max_cost`` as ``watch.check_params`` / ``watch.cost_units``;
T = ``max_tracks`` and ``ncls`` are the tracker's.
Memo: int32 [S, T, 8], all zero = empty: id + 1, key_lo, key_hi, entry, mismatches, cost, n_hits, last_at_lookup.

Rules.  The steps run after an ``update`` call, on the tracker state as that call left it.  Every stream s < S is processed, whether
or not it had a frame in the call; every slot t < T goes through the steps in order:
  1. a slot is live iff hits > 0 (the tracker's definition); a slot that is not live gets a zero memo entry;
  2. the slot's read is rule 8 of ``yolov6.utils.track``, unchanged: best_p = the first index of the largest
     votes[p][0 .. ncls[p]) (0 for an all-zero head), share_p = votes[p][best_p] / total[p] if total[p] > 0 else 0 (one fp32
     division, the tracker's); key = the eight best_p as bytes, best_0..3 in key_lo and best_4..7 in key_hi, least significant
     byte first;
  3. a slot is a candidate iff it is live and hits >= min_hits; it is fresh iff it is a candidate and (memo.id != id + 1 or
     memo.key != key).  A missed slot (misses > 0) is a candidate like any other: that matters after the feature is switched on
     mid-run;
  4. the fresh slots of stream s, in ascending slot order, are that stream's queries j = 0, 1, ..., written in the ended-record
     layout -- the record the track would leave if it ended now: q_i[s, j] = (id, first, last, hits, best_0..7),
     q_f[s, j] = (share_0..7, box x1, y1, x2, y2), q_slot[s, j] = t, q_count[s] = their number; lines past the count are zero,
     with q_slot = -1;
  5. m = ``watch.watch_match_np(entries, confuse, q_i, q_f, q_count, max_mismatch, max_cost)``: the existing rule, unchanged
     (with ``indel=1``: ``watch_match_np(..., 1, gap_cost, align=True)``, which also gives the alignment code a of every query);
  6. for every fresh slot memo[s, t] = (id + 1, key_lo, key_hi, m.entry, m.mismatches, m.cost, m.n_hits, slot.last).  A lookup
     that found nothing is memoised too (entry = -1), so it is not repeated;
  7. live_i int32 [S, T, 8], one row per slot: for a live slot whose memo holds its id
     (id, entry, mismatches, cost, n_hits, fresh ? 1 : 0, hits, last_at_lookup); for every other slot (-1, -1, 0, 0, 0, 0, 0, 0);
  8. (``indel=1``) live_align int32 [S, T], one code per slot, kept beside the memo (the memo's eight words are unchanged): a fresh
     slot gets the code of its lookup, a slot whose row of live_i is a standing one keeps the code it has, every other slot gets 0.
     So the code of a standing hit is the one of its lookup.

What follows: an alert is a row with fresh == 1 and entry >= 0; a row with fresh == 0 and entry >= 0 is a standing hit.  A track is
looked up once when it reaches ``min_hits`` and again only when its voted read changes.  A new track in a reused slot never inherits
the memo, because the id differs.  ``reset(streams)`` and a flush clear the memo of their streams (a flush leaves no live slot).
Enabling again, for another list or other limits, zeroes the whole memo.

What it does not do: the read is the one at the end of the call (a stream with several frames in one call has each of its tracks
looked up at most once); the memoised cost is as of the lookup -- a read whose key stays put while its shares move is not scored
again, and the ended-record match of ``enable_watch`` remains the final word; and as ``yolov6.utils.watch``: at most one
insertion or deletion in heads 2..7, and only with ``indel=1``; one best entry plus a count.
"""
import numpy as np

from yolov6.utils import watch
from yolov6.utils.track import ENDED_COLS, HEADS

MEMO_COLS = 8
LIVE_COLS = 8
NO_ROW = (-1, -1, 0, 0, 0, 0, 0, 0)
f32 = np.float32


def check_min_hits(min_hits):
    """``min_hits`` as the integer of the rule (ValueError below 1)."""
    m = int(min_hits)
    if m != min_hits or m < 1:
        raise ValueError('min_hits must be an integer >= 1')
    return m


def read_key(best):
    """(key_lo, key_hi) int32 of eight voted ids (each 0..63)."""
    b = [int(v) for v in best]
    lo = b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24
    hi = b[4] | b[5] << 8 | b[6] << 16 | b[7] << 24
    return lo, hi


def alerts_of(live_i):
    """The (stream, slot) pairs of the alerts of one ``live_i`` (numpy [S, T, 8]): fresh == 1 and entry >= 0, in (stream, slot) order."""
    live_i = np.asarray(live_i)
    return [(int(s), int(t)) for s, t in np.argwhere((live_i[:, :, 5] == 1) & (live_i[:, :, 1] >= 0))]


class LiveWatchNp:
    """The memo of one tracker (a ``PlateTrackerNp``) and the steps of the module's rule.  ``watchlist``: anything with
    ``entries_np`` and ``confuse_np`` (``watch.WatchlistNp``, ``runtime.Watchlist``).  ``step()`` after an ``update`` returns live_i
    and leaves the queries in ``q_i``, ``q_f``, ``q_slot``, ``q_count`` and the match of step 5 in ``match_i``."""

    def __init__(self, tracker, watchlist, min_hits=3, max_mismatch=1, max_cost=None, indel=0, gap_cost=None):
        self.tracker, self.watchlist = tracker, watchlist
        self.min_hits = check_min_hits(min_hits)
        self.max_mismatch, self.max_cost = watch.check_params(max_mismatch, watch.cost_units(max_cost))
        self.indel, self.gap_cost = watch.check_indel(indel, watch.gap_units(gap_cost))
        S, T = tracker.n_streams, tracker.max_tracks
        self.memo = np.zeros((S, T, MEMO_COLS), np.int32)
        self.live_i = self.q_i = self.q_f = self.q_slot = self.q_count = self.match_i = None
        #: with ``indel=1``: int32 [S, T] of rule 8 (kept between steps), and the match_align of step 5; else None
        self.live_align = np.zeros((S, T), np.int32) if self.indel else None
        self.match_align = None

    def reset(self, streams=None):
        """Zero the memo of ``streams`` (all for None)."""
        for s in (range(self.tracker.n_streams) if streams is None else streams):
            self.memo[int(s)] = 0

    def step(self):
        trk, memo = self.tracker, self.memo
        S, T = trk.n_streams, trk.max_tracks
        q_i, q_f = np.zeros((S, T, ENDED_COLS), np.int32), np.zeros((S, T, ENDED_COLS), f32)
        q_slot, q_count = np.full((S, T), -1, np.int32), np.zeros(S, np.int32)
        fresh = np.zeros((S, T), bool)
        keys = np.zeros((S, T, 2), np.int32)
        live = trk.hits > 0
        memo[~live] = 0                                                                  # 1
        for s, t in np.argwhere(live & (trk.hits >= self.min_hits)):                     # 3: the candidates, in (s, t) order
            best, share = trk.read(s, t)                                                 # 2
            keys[s, t] = read_key(best)
            if memo[s, t, 0] != trk.id[s, t] + 1 or memo[s, t, 1] != keys[s, t, 0] or memo[s, t, 2] != keys[s, t, 1]:
                j = int(q_count[s])                                                      # 4
                fresh[s, t] = True
                q_i[s, j, :4] = trk.id[s, t], trk.first[s, t], trk.last[s, t], trk.hits[s, t]
                q_i[s, j, 4:] = best
                q_f[s, j, :HEADS], q_f[s, j, HEADS:] = share, trk.box[s, t]
                q_slot[s, j] = t
                q_count[s] = j + 1
        wl = self.watchlist
        if self.indel:                                                                   # 5
            m, a = watch.watch_match_np(wl.entries_np, wl.confuse_np, q_i, q_f, q_count, self.max_mismatch, self.max_cost, 1, self.gap_cost,
                                        align=True)
        else:
            m = watch.watch_match_np(wl.entries_np, wl.confuse_np, q_i, q_f, q_count, self.max_mismatch, self.max_cost)
        for s in range(S):                                                               # 6
            for j in range(int(q_count[s])):
                t = q_slot[s, j]
                memo[s, t] = (trk.id[s, t] + 1, keys[s, t, 0], keys[s, t, 1]) + tuple(m[s, j]) + (trk.last[s, t],)
        live_i = np.empty((S, T, LIVE_COLS), np.int32)                                   # 7
        live_i[:] = NO_ROW
        for s, t in np.argwhere(live & (memo[:, :, 0] == trk.id + 1)):
            live_i[s, t] = (trk.id[s, t],) + tuple(memo[s, t, 3:7]) + (int(fresh[s, t]), trk.hits[s, t], memo[s, t, 7])
        if self.indel:                                                                   # 8
            keep = np.where(live & (memo[:, :, 0] == trk.id + 1), self.live_align, 0).astype(np.int32)
            for s in range(S):
                for j in range(int(q_count[s])):
                    keep[s, q_slot[s, j]] = a[s, j]
            self.live_align, self.match_align = keep, a
        self.live_i, self.q_i, self.q_f, self.q_slot, self.q_count, self.match_i = live_i, q_i, q_f, q_slot, q_count, m
        return live_i
