"""The live-track watchlist lookup on the CPU: ``LiveWatchNp`` (yolov6/utils/watch_live.py, the specification of lp_watch_live) against
a restatement in plain loops, the scenes the feature exists for (a car that waits, a vote that flips), the edges of its rule,
``PlateTrackerNp.enable_live_watch`` leaving everything else alone, the argument checks of lp_watch_live (no device needed) and
``tools/infer.py --watch-live`` on the CPU path.  ``live_step_loops``, ``live_list_for`` and ``LiveLoops`` are shared with
tests/test_watch_live_gpu.py."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
import test_track_cpu as T
import test_watch_cpu as C

LP_ERR_ARG = -1
f32 = np.float32
NO_ROW = [-1, -1, 0, 0, 0, 0, 0, 0]
STATE_ARRAYS = ('frame', 'next_id', 'dropped', 'id', 'first', 'last', 'hits', 'misses', 'box', 'cor', 'vel', 'votes', 'total')


# ---- the rule once more, as loops over Python integers and np.float32 scalars ------------------------------------------------------
def head_read(votes, total, n):
    """(best, share) of one head: the first index of the largest of votes[0 .. n), one fp32 division."""
    best = 0
    for c in range(1, n):
        if votes[c] > votes[best]:
            best = c
    share = f32(0)
    if total > 0:
        with np.errstate(all='ignore'):
            share = f32(f32(votes[best]) / f32(total))
    return best, share


def live_step_loops(trk, memo, min_hits, entries, confuse, max_mismatch, max_cost):
    """Steps 1 to 7 on the state arrays of ``trk`` by the words of the rule: (live_i, q_i, q_f, q_slot, q_count); ``memo`` is updated."""
    S, T_ = trk.n_streams, trk.max_tracks
    q_i, q_f = np.zeros((S, T_, 12), np.int32), np.zeros((S, T_, 12), f32)
    q_slot, q_count = np.full((S, T_), -1, np.int32), np.zeros(S, np.int32)
    fresh, key = {}, {}
    for s in range(S):
        for t in range(T_):
            hits, tid = int(trk.hits[s, t]), int(trk.id[s, t])
            if hits <= 0:
                memo[s, t] = 0
                continue
            if hits < min_hits:
                continue
            reads = [head_read(trk.votes[s, t, p], trk.total[s, t, p], trk.ncls[p]) for p in range(8)]
            best = [b for b, _ in reads]
            lo = sum(b << (8 * p) for p, b in enumerate(best[:4]))
            hi = sum(b << (8 * p) for p, b in enumerate(best[4:]))
            key[s, t] = (lo, hi)
            if int(memo[s, t, 0]) != tid + 1 or (int(memo[s, t, 1]), int(memo[s, t, 2])) != (lo, hi):
                j = int(q_count[s])
                fresh[s, t] = j
                q_i[s, j] = [tid, trk.first[s, t], trk.last[s, t], hits] + best
                q_f[s, j] = [sh for _, sh in reads] + list(trk.box[s, t])
                q_slot[s, j] = t
                q_count[s] = j + 1
    m = C.match_loops(entries, confuse, q_i, q_f, q_count, max_mismatch, max_cost)
    live_i = np.zeros((S, T_, 8), np.int32)
    for s in range(S):
        for t in range(T_):
            if (s, t) in fresh:
                memo[s, t] = [int(trk.id[s, t]) + 1, key[s, t][0], key[s, t][1]] + m[s, fresh[s, t]].tolist() + [int(trk.last[s, t])]
            if trk.hits[s, t] > 0 and memo[s, t, 0] == trk.id[s, t] + 1:
                live_i[s, t] = [trk.id[s, t]] + memo[s, t, 3:7].tolist() + [int((s, t) in fresh), trk.hits[s, t], memo[s, t, 7]]
            else:
                live_i[s, t] = NO_ROW
    return live_i, q_i, q_f, q_slot, q_count


class LiveLoops:
    """``live_step_loops`` with its memo: the reference object of the comparisons, here and on the GPU."""

    def __init__(self, trk, entries, confuse, min_hits, max_mismatch, max_cost):
        self.trk, self.args = trk, (min_hits, entries, confuse, max_mismatch, max_cost)
        self.memo = np.zeros((trk.n_streams, trk.max_tracks, 8), np.int32)

    def step(self):
        return live_step_loops(self.trk, self.memo, *self.args)


def live_list_for(calls, n_streams, N, seed=0, min_hits=1, **kw):
    """A watchlist of ``N`` entries for the random tracker case ``calls``: the reads its live tracks show after each call (run once
    without a list), some unchanged, some with one position changed, some with a wildcard, planted at random indices (the last one
    included) among random entries."""
    from yolov6.utils.track import PlateTrackerNp
    rng = np.random.default_rng(seed)
    trk, reads = PlateTrackerNp(n_streams, **kw), []
    for det, count, stream_of, flush in calls:
        trk.update(det, count, stream_of, flush)
        reads += [trk.read(s, t)[0] for s, t in np.argwhere(trk.hits >= min_hits)]
    entries = C.random_entries(rng, N, n_ids=37, nothing=0.0)
    if N and reads:
        for k, at in enumerate(rng.permutation(N)[:max(N // 2, 1)]):
            r = np.array(reads[int(rng.integers(0, len(reads)))])
            u = rng.random()
            if u < 0.35:
                r[int(rng.integers(0, 8))] = int(rng.integers(0, 24))
            elif u < 0.55:
                r[int(rng.integers(0, 8))] = 255
            entries[N - 1 if k == 0 else at] = r
    return entries


def assert_same(got, want, what):
    for name, g, w in zip(('live_i', 'q_i', 'q_f', 'q_slot', 'q_count', 'memo'), got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if not np.array_equal(g.view(np.int32), w.view(np.int32)):
            bad = np.argwhere(g.view(np.int32) != w.view(np.int32))
            raise AssertionError('%s: %s differs in %d words, first at %s: got %s, want %s'
                                 % (what, name, len(bad), bad[0].tolist(), g[tuple(bad[0][:-1])], w[tuple(bad[0][:-1])]))


def outputs_np(trk):
    return (trk.last_live,) + tuple(trk.last_live_reads) + (trk._live.memo,)


# ---- LiveWatchNp against the loops -----------------------------------------------------------------------------------------------------
KW = dict(max_tracks=8, match_thres=0.3, new_thres=0.2, expand=0.5, max_age=2)


@pytest.mark.parametrize('seed,min_hits', [(0, 1), (1, 3), (2, 2)])
def test_live_watch_np_against_the_loops(seed, min_hits):
    """30 frames over 3 streams, T = 8, a list with planted entries and wildcards, a confusion table: every int32, every frame."""
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.watch import WatchlistNp
    calls = T.random_track_case(40 + seed, n_streams=3, max_det=20, Bs=(3,) * 10)
    entries = live_list_for(calls, 3, 40, seed, min_hits, **KW)
    confuse = C.random_confuse(np.random.default_rng(seed))
    trk = PlateTrackerNp(3, **KW)
    trk.enable_live_watch(WatchlistNp(entries, confuse), min_hits, max_mismatch=2, max_cost=1.5)
    ref = LiveLoops(trk, entries, confuse, min_hits, 2, 6144)
    seen = dict(fresh=0, alerts=0, standing=0, misses=0, relooked=0)
    looked = set()
    for k, (det, count, stream_of, flush) in enumerate(calls):
        trk.update(det, count, stream_of, flush)
        want = ref.step()
        assert_same(outputs_np(trk), want + (ref.memo,), 'call %d' % k)
        live_i = want[0]
        seen['fresh'] += int(want[4].sum())
        seen['alerts'] += int(((live_i[:, :, 5] == 1) & (live_i[:, :, 1] >= 0)).sum())
        seen['standing'] += int(((live_i[:, :, 5] == 0) & (live_i[:, :, 1] >= 0)).sum())
        seen['misses'] += int(((live_i[:, :, 5] == 1) & (live_i[:, :, 1] < 0)).sum())
        for s, t in np.argwhere(live_i[:, :, 5] == 1):
            seen['relooked'] += (s, int(live_i[s, t, 0])) in looked
            looked.add((s, int(live_i[s, t, 0])))
    assert all(v > 0 for v in seen.values()), seen                              # a case cannot pass by doing nothing
    assert not trk._live.memo.any()                                             # the last call flushes every stream


# ---- the two scenes the feature exists for -----------------------------------------------------------------------------------------------
PLATE = (3, 7, 11, 12, 13, 14, 15, 16)
BOX = (100, 50, 180, 75)


def car(ids=PLATE, conf=0.9, box=BOX):
    return T.make_row(box, ids, conf)


def step(trk, rows, s=0, flush=None):
    det, count = T.frames_of([rows], 4)
    return trk.update(det, count, stream_of=[s], flush=flush)


def test_a_waiting_car_is_reported_while_its_track_lives():
    """One plate, detected in every one of 40 frames, on the list: the alert fires in the frame its hits reach 3 and stands from
    then on, while the ended-record match of ``enable_watch`` reports nothing in any of the 40 frames."""
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.watch import WatchlistNp
    rng = np.random.default_rng(1)
    entries = C.random_entries(rng, 20, n_ids=37, wild=0.0, nothing=0.0)
    planted = 13
    entries[planted] = PLATE
    wl = WatchlistNp(entries)
    trk = PlateTrackerNp(1, max_tracks=8, max_age=5)
    trk.enable_watch(wl)
    trk.enable_live_watch(wl, min_hits=3)
    for k in range(40):
        step(trk, [car()])
        rows = trk.last_live[0]
        assert not (trk.last_watch[:, :, 0] >= 0).any() and trk.hits[0, 0] == k + 1
        if k < 2:
            assert rows.tolist() == [NO_ROW] * 8 and trk.last_live_reads[3].tolist() == [0]
            continue
        hit = np.nonzero(rows[:, 1] == planted)[0]
        assert hit.tolist() == [0] and rows[1:].tolist() == [NO_ROW] * 7
        assert rows[0].tolist() == [0, planted, 0, 0, 1, int(k == 2), k + 1, 2]
        assert trk.last_live_reads[3].tolist() == [int(k == 2)]


def test_a_vote_that_flips_is_looked_up_again_at_that_frame_only():
    """Head 3 reads class 5 at confidence 1/2 up to frame 5 and class 9 at 3/4 from frame 6 on: the voted id changes in the frame
    in which the fp32 sum of the 3/4s first exceeds the sum of the 1/2s, and that frame alone brings a second lookup."""
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.watch import WatchlistNp
    k0, frames = 6, 20
    old, new = list(PLATE), list(PLATE)
    old[3], new[3] = 5, 9
    va = vb = f32(0)
    flip = None
    for k in range(frames):
        if k < k0:
            va = f32(va + f32(0.5))
        else:
            vb = f32(vb + f32(0.75))
        if flip is None and vb > va:
            flip = k
    assert flip == k0 + 4
    conf_old, conf_new = np.full(8, 0.9, f32), np.full(8, 0.9, f32)
    conf_old[3], conf_new[3] = 0.5, 0.75
    wl = WatchlistNp(np.array([old, new], np.uint8))
    trk = PlateTrackerNp(1, max_tracks=8, max_age=5)
    trk.enable_live_watch(wl, min_hits=3, max_mismatch=0)
    lookups = []
    for k in range(frames):
        step(trk, [car(old, conf_old) if k < k0 else car(new, conf_new)])
        row, (q_i, _, q_slot, q_count) = trk.last_live[0, 0], trk.last_live_reads
        if q_count[0]:
            lookups.append(k)
            assert q_count[0] == 1 and q_slot[0, 0] == 0 and q_i[0, 0, 4:].tolist() == (old if k < flip else new)
        if k >= 2:
            assert row.tolist() == [0, int(k >= flip), 0, 0, 1, int(k in (2, flip)), k + 1, 2 if k < flip else flip]
    assert lookups == [2, flip]


# ---- edges ---------------------------------------------------------------------------------------------------------------------------------
def tracker(entries=(PLATE,), S=1, min_hits=3, **kw):
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.watch import WatchlistNp
    wl = WatchlistNp(np.array(entries, np.uint8).reshape(-1, 8))
    trk = PlateTrackerNp(S, max_tracks=4, **dict(dict(max_age=5), **kw))
    if min_hits is not None:
        trk.enable_live_watch(wl, min_hits=min_hits)
    return trk, wl


def test_min_hits_is_the_first_frame_that_looks_a_track_up():
    trk, _ = tracker(min_hits=1)
    step(trk, [car()])
    assert trk.last_live[0, 0].tolist() == [0, 0, 0, 0, 1, 1, 1, 0] and trk.last_live_reads[3].tolist() == [1]
    trk, _ = tracker(min_hits=4)
    for k in range(3):
        step(trk, [car()])
        assert trk.hits[0, 0] == k + 1 and trk.last_live[0].tolist() == [NO_ROW] * 4 and not trk._live.memo.any()
    step(trk, [car()])
    assert trk.last_live[0, 0].tolist() == [0, 0, 0, 0, 1, 1, 4, 3]
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match='min_hits'):
            trk.enable_live_watch(trk._live.watchlist, min_hits=bad)


def test_a_new_track_in_a_reused_slot_with_the_same_read_is_fresh_again():
    trk, _ = tracker(min_hits=2, max_age=0)
    step(trk, [car()])
    step(trk, [car()])
    assert trk.last_live[0, 0].tolist() == [0, 0, 0, 0, 1, 1, 2, 1]
    step(trk, [])                                                               # max_age 0: the track ends, its memo line with it
    assert not trk.live(0).any() and not trk._live.memo.any() and trk.last_live[0].tolist() == [NO_ROW] * 4
    step(trk, [car()])
    assert trk.id[0, 0] == 1 and trk.last_live[0].tolist() == [NO_ROW] * 4
    step(trk, [car()])
    assert trk.last_live[0, 0].tolist() == [1, 0, 0, 0, 1, 1, 2, 4]           # slot 0 again, the same read, another id: looked up
    step(trk, [car()])
    assert trk.last_live[0, 0].tolist() == [1, 0, 0, 0, 1, 0, 3, 4]


def test_flush_and_reset_clear_exactly_their_streams():
    trk, _ = tracker(S=3, min_hits=1)
    det, count = T.frames_of([[car()]] * 3, 4)
    trk.update(det, count, stream_of=[0, 1, 2])
    assert trk._live.memo[:, 0, 0].tolist() == [1, 1, 1] and (trk.last_live[:, 0, 5] == 1).all()
    trk.update(det, count, stream_of=[0, 1, 2], flush=[0, 1, 0])
    assert trk._live.memo[:, 0, 0].tolist() == [1, 0, 1] and trk.last_live[:, 0, 0].tolist() == [0, -1, 0]
    assert trk.last_live[:, 0, 5].tolist() == [0, 0, 0]
    trk.reset([2])
    assert trk._live.memo[:, 0, 0].tolist() == [1, 0, 0]
    trk.update(det[:0], count[:0], stream_of=[])                                # no frames at all: stream 0 stands, the others are empty
    assert trk.last_live[:, 0].tolist() == [[0, 0, 0, 0, 1, 0, 2, 0], NO_ROW, NO_ROW] and trk.last_live_reads[3].tolist() == [0, 0, 0]
    trk.flush_all()
    assert not trk._live.memo.any() and (trk.last_live.reshape(-1, 8) == NO_ROW).all()
    trk.reset()
    assert not trk._live.memo.any()


def test_enabling_mid_run_looks_up_every_track_past_min_hits_missed_ones_included():
    trk, wl = tracker(min_hits=None)
    far = (300, 200, 380, 225)
    other = (9, 8, 7, 6, 5, 4, 3, 2)
    for _ in range(4):
        step(trk, [car(), car(other, box=far)])
    step(trk, [car()])                                                          # the second car is missed once
    step(trk, [car(), car(box=(10, 300, 90, 325))])                             # ... and again; a third track is born
    assert trk.misses[0].tolist() == [0, 2, 0, 0] and trk.hits[0].tolist() == [6, 4, 1, 0]
    trk.enable_live_watch(wl, min_hits=3)
    assert trk.last_live is None
    det, count = T.frames_of([], 4)
    trk.update(det, count, stream_of=[])                                        # the next call, whatever it holds
    q_i, _, q_slot, q_count = trk.last_live_reads
    assert q_count.tolist() == [2] and q_slot[0].tolist() == [0, 1, -1, -1]
    assert q_i[0, 0].tolist() == [0, 0, 5, 6] + list(PLATE) and q_i[0, 1].tolist() == [1, 0, 3, 4] + list(other)
    assert trk.last_live[0].tolist() == [[0, 0, 0, 0, 1, 1, 6, 5], [1, -1, 0, 0, 0, 1, 4, 3], NO_ROW, NO_ROW]
    trk.update(det, count, stream_of=[])
    assert trk.last_live[0, :2, 5].tolist() == [0, 0] and trk.last_live_reads[3].tolist() == [0]


def test_an_empty_list_memoises_minus_one_and_does_not_look_up_again():
    trk, _ = tracker(entries=np.zeros((0, 8), np.uint8), min_hits=1)
    step(trk, [car()])
    assert trk.last_live[0, 0].tolist() == [0, -1, 0, 0, 0, 1, 1, 0] and trk._live.memo[0, 0, 3] == -1
    step(trk, [car()])
    assert trk.last_live[0, 0].tolist() == [0, -1, 0, 0, 0, 0, 2, 0] and trk.last_live_reads[3].tolist() == [0]


def test_enabling_again_zeroes_the_memo_and_none_turns_it_off():
    trk, wl = tracker(entries=[[3, 7, 11, 12, 13, 14, 15, 20]], min_hits=1)
    step(trk, [car()])
    assert trk.last_live[0, 0].tolist() == [0, 0, 1, 4096, 1, 1, 1, 0]
    trk.enable_live_watch(wl, min_hits=1, max_mismatch=0)
    assert trk.last_live is None and trk.last_live_reads is None and not trk._live.memo.any()
    step(trk, [car()])
    assert trk.last_live[0, 0].tolist() == [0, -1, 0, 0, 0, 1, 2, 1]          # looked up again, under the new limit
    trk.enable_live_watch(wl, min_hits=1, max_cost=0.5)
    step(trk, [car()])
    assert trk.last_live[0, 0].tolist() == [0, -1, 0, 0, 0, 1, 3, 2]
    trk.enable_live_watch(None)
    step(trk, [car()])
    assert trk.last_live is None and trk.last_live_reads is None
    with pytest.raises(ValueError):
        trk.enable_live_watch(wl, max_mismatch=9)


def test_a_stream_without_a_frame_in_a_call_produces_no_query():
    from yolov6.utils.watch import position_weight
    trk, _ = tracker(S=2, min_hits=2)
    det, count = T.frames_of([[car()]] * 2, 4)
    trk.update(det, count, stream_of=[0, 1])
    trk.update(det, count, stream_of=[0, 1])
    assert trk.last_live_reads[3].tolist() == [1, 1]
    new = list(PLATE)
    new[7] = 30
    for k in range(3):                                                          # stream 0 alone goes on, with a read that takes the vote over
        d, c = T.frames_of([[car(new)]], 4)
        trk.update(d, c, stream_of=[0])
        assert trk.last_live_reads[3].tolist() == [int(k == 2), 0]
        assert trk.last_live[1, 0].tolist() == [0, 0, 0, 0, 1, 0, 2, 1]
    cost = 16 * int(position_weight(trk.last_live_reads[1][0, 0, 7]))           # one mismatch, at the share the new id holds
    assert trk.last_live[0, 0].tolist() == [0, 0, 1, cost, 1, 1, 5, 4] and 16 * 128 < cost < 16 * 200


# ---- enable_live_watch changes nothing else ------------------------------------------------------------------------------------------------
def test_enable_live_watch_has_no_side_effects():
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.watch import WatchlistNp
    calls = T.random_track_case(5, n_streams=3, max_det=20, n_calls=12)
    entries = live_list_for(calls, 3, 30, 5, 1, **KW)
    wl = WatchlistNp(entries, C.random_confuse(np.random.default_rng(2)))
    plain, live = PlateTrackerNp(3, **KW), PlateTrackerNp(3, **KW)
    for trk in (plain, live):
        trk.enable_hold(min_hits=2)
        trk.enable_watch(wl, max_mismatch=2)
    live.enable_live_watch(wl, min_hits=2, max_mismatch=2)
    looked = 0
    for det, count, stream_of, flush in calls:
        a, b = plain.update(det, count, stream_of, flush, 5), live.update(det, count, stream_of, flush, 5)
        for x, y in zip(a + plain.last_hold + (plain.last_watch,), b + live.last_hold + (live.last_watch,)):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.int32), y.view(np.int32))
        for name in STATE_ARRAYS:
            x, y = getattr(plain, name), getattr(live, name)
            assert np.array_equal(x.view(np.int32), y.view(np.int32)), name
        looked += int(live.last_live_reads[3].sum())
    assert looked > 0 and plain.last_live is None and plain.last_live_reads is None


# ---- C ABI: everything is checked on the host before any launch ----------------------------------------------------------------------------
def test_watch_live_rejects_bad_arguments_before_launch():
    """Fake device addresses: a launch would fault, so LP_ERR_ARG proves the host check came first."""
    from yolov6.hip import abi
    lib = abi.load()
    v = lambda p: ctypes.c_void_p(p) if p else None   # noqa: E731
    S, T_ = 3, 8
    L = S * T_
    need, memo_bytes = lib.lp_watch_live_workspace_bytes(S, T_), lib.lp_watch_live_state_bytes(S, T_)
    assert memo_bytes == L * 32 and need >= L * 20 + lib.lp_watch_workspace_bytes(S, T_) and need % 16 == 0
    assert lib.lp_watch_live_workspace_bytes(2 * S, T_) > need and lib.lp_watch_live_state_bytes(S, 128) == S * 128 * 32
    for fn in (lib.lp_watch_live_workspace_bytes, lib.lp_watch_live_state_bytes):
        assert fn(0, T_) == 0 and fn(S, 0) == 0 and fn(S, 129) == 0 and fn(1 << 24, 128) == 0
    state_bytes = lib.lp_track_state_bytes(S, T_)

    def call(state=0x100000, S=S, T_=T_, ncls=T.NCLS, min_hits=3, memo=0x200000, entries=0x300000, n=1000, confuse=0x310000, mm=1, mc=4096,
             q_i=0x400000, q_f=0x410000, q_slot=0x420000, q_count=0x430000, live=0x440000, ws=0x500000, ws_bytes=need):
        nc = (ctypes.c_int * 8)(*ncls) if ncls is not None else None
        return lib.lp_watch_live(v(state), S, T_, nc, min_hits, v(memo), v(entries), n, v(confuse), mm, mc, v(q_i), v(q_f), v(q_slot),
                                 v(q_count), v(live), v(ws), ws_bytes, None)

    err = lambda: lib.lp_last_error()   # noqa: E731
    assert call(S=0) == LP_ERR_ARG and b'n_streams' in err() and call(T_=0) == LP_ERR_ARG and call(T_=129) == LP_ERR_ARG and b'128' in err()
    assert call(S=1 << 24, T_=128) == LP_ERR_ARG and b'2^31' in err()
    assert call(ncls=None) == LP_ERR_ARG and b'ncls' in err()
    assert call(ncls=(31, 24, 37, 0, 37, 37, 37, 37)) == LP_ERR_ARG and b'head 3' in err()
    assert call(ncls=(31, 24, 37, 37, 37, 37, 37, 65)) == LP_ERR_ARG and b'head 7' in err()
    assert call(min_hits=0) == LP_ERR_ARG and b'min_hits' in err() and call(min_hits=-3) == LP_ERR_ARG
    assert call(n=-1) == LP_ERR_ARG and b'n_entries' in err() and call(n=(1 << 24) + 1) == LP_ERR_ARG and b'16777216' in err()
    for k, bad in (('mm', -1), ('mm', 9), ('mc', -1), ('mc', 32769)):
        assert call(**{k: bad}) == LP_ERR_ARG and b'max_mismatch' in err(), (k, bad)
    for k in ('state', 'memo', 'entries', 'q_i', 'q_f', 'q_slot', 'q_count', 'live', 'ws'):
        assert call(**{k: 0}) == LP_ERR_ARG and b'null' in err(), k
    assert call(n=0, entries=0, memo=0) == LP_ERR_ARG and b'null' in err()       # an empty list needs no entries, but everything else
    for k, at in (('state', 0x100008), ('memo', 0x200004), ('live', 0x440008), ('ws', 0x500008), ('entries', 0x300004), ('confuse', 0x310002)):
        assert call(**{k: at}) == LP_ERR_ARG and b'aligned' in err(), k
    assert call(ws_bytes=need - 1) == LP_ERR_ARG and b'workspace' in err() and call(ws_bytes=0) == LP_ERR_ARG
    for k, at in (('memo', 0x100000 + state_bytes - 16), ('memo', 0x300000 + 7984), ('q_i', 0x310000 + 12284), ('q_f', 0x400000 + L * 48 - 4),
                  ('q_slot', 0x410000), ('q_count', 0x420000 + L * 4 - 4), ('live', 0x430000), ('ws', 0x440000 + L * 32 - 16),
                  ('ws', 0x200000 + L * 32 - 16), ('live', 0x500000 + need - 16), ('q_count', 0x100000)):
        assert call(**{k: at}) == LP_ERR_ARG and b'overlap' in err(), (k, hex(at))


# ---- tools/infer.py --watch-live on the CPU path ------------------------------------------------------------------------------------------
def expected_alert_lines(dets, max_det, entries, min_hits, max_mismatch, max_cost, **kw):
    """alerts.txt by the loops: ``PlateTrackerNp`` over the untracked per-frame detections of one stream, one update per frame."""
    from yolov6.utils.track import PlateTrackerNp, plate_text
    from yolov6.utils.watch import entry_text
    trk = PlateTrackerNp(1, **kw)
    ref = LiveLoops(trk, entries, None, min_hits, max_mismatch, max_cost)
    lines = []
    for d in dets:
        pad = np.zeros((1, max_det, 28), f32)
        pad[0, :len(d)] = d
        trk.update(pad, [len(d)], max_ended=2 * trk.max_tracks)
        live_i, q_i, _, q_slot, q_count = ref.step()
        for j in range(int(q_count[0])):
            tid, e, mism, cost, n, fresh, hits, last = live_i[0, q_slot[0, j]].tolist()
            if e >= 0:
                assert fresh == 1
                lines.append('%d %d %s %d %s %d %d %d %d' % (last, tid, plate_text(q_i[0, j, 4:]), e, entry_text(entries[e]), mism, cost, n, hits))
    return lines


def test_infer_watch_live_cpu(tmp_path, monkeypatch):
    from PIL import Image
    from yolov6.utils.synth import build_synthetic
    from yolov6.utils.watch import entry_text
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    m = build_synthetic(os.path.join(REPO, 'configs', 'yololps.py'), width=0.0625, sigma=1.5)
    ckpt = tmp_path / 'tiny.pt'
    torch.save({'model': m.half(), 'ema': None, 'epoch': 0}, str(ckpt))
    img_dir = tmp_path / 'imgs'
    img_dir.mkdir()
    for k, f in enumerate(T._moving_frames(6)):
        Image.fromarray(f).save(str(img_dir / ('f%02d.png' % k)))
    kw = dict(weights=str(ckpt), source=str(img_dir), yaml=None, img_size=[128, 160], conf_thres=0.06, iou_thres=0.45, max_det=20,
              device='cpu', not_save_img=True, save_txt=True, track_max_age=2, track_iou=0.25, track_expand=0.25)
    untracked = [d.numpy() for d in infer.run(save_dir=str(tmp_path / 'o0'), **kw)]
    tkw = dict(max_tracks=64, match_thres=0.25, new_thres=0.0, expand=0.25, max_age=2, ncls=m)
    _, _, ended = T.track_by_hand(untracked, 20, **tkw)
    reads = np.array([ri[4:12] for ri, _ in ended])
    far = [(v + 5) % 24 for v in reads[0]]
    rows = [far, reads[0], [255] * 7 + [int(reads[-1][7])], reads[0], [255] * 8]   # the last line accepts every read at cost 0
    wl = tmp_path / 'watch.txt'
    wl.write_text('\n'.join(entry_text(r) for r in rows) + '\n')
    entries = np.array(rows, np.uint8)
    plain = infer.run(save_dir=str(tmp_path / 'o1'), track=True, watchlist=str(wl), **kw)
    assert not (tmp_path / 'o1' / 'alerts.txt').exists()
    for sub, min_hits in (('o2', 2), ('o3', 1)):
        again = infer.run(save_dir=str(tmp_path / sub), track=True, watchlist=str(wl), watch_live=True, watch_live_min_hits=min_hits, **kw)
        for a, b in zip(plain, again):
            assert torch.equal(a, b)
        for name in ('tracks.txt', 'plates.txt', 'hits.txt'):                    # byte-identical to the run without the switch
            assert (tmp_path / sub / name).read_bytes() == (tmp_path / 'o1' / name).read_bytes()
        want = expected_alert_lines(untracked, 20, entries, min_hits, 1, 32768, **tkw)
        assert (tmp_path / sub / 'alerts.txt').read_text().splitlines() == want and len(want) >= 1, (sub, want)
    assert len(want) >= len(ended)                                              # min_hits 1: every track fires at least once
    with pytest.raises(ValueError, match='watchlist'):
        infer.run(save_dir=str(tmp_path / 'o4'), track=True, watch_live=True, **kw)
