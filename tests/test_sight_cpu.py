"""The log of sightings on the CPU: ``sight_update_np`` (yolov6/utils/sight.py, the specification of lp_sight_update) against plain
loops over Python integers on random cases, the scenarios of its rule -- entry / exit pairing with a confusable misread and a
``pair`` mask, a broken track, the edges of the window, the most recent of two equally cheap sightings, the ring, ``min_hits``, ids
that match nothing, garbage shares and counts --, each on the full sight_i and the full state, ``PlateTrackerNp.enable_sightings``,
the argument checks of lp_sight_update (no device needed) and ``tools/infer.py --track --sightings`` on the CPU path.
``update_loops``, ``random_sequence`` and ``records`` are shared with tests/test_sight_gpu.py."""
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
EMPTY = (-1, 0, 0, 0, -1, -1, 0, 0)


# ---- the rule once more, as loops over Python integers --------------------------------------------------------------------------------
def update_loops(state, confuse, pair, ended_i, ended_f, ended_count, now, window, min_hits, max_mismatch, max_cost):
    """(sight_i, the new state) by the words of the rule: lines, slots and positions one by one; ``state`` is not changed."""
    C_ = len(state) - 1
    S, max_ended = ended_i.shape[:2]
    total = int(state[0, 0])
    fill = min(total, C_)
    rows = [[int(v) for v in state[1 + e]] for e in range(fill)]
    out = np.zeros((S, max_ended, 8), np.int32)
    out[:] = EMPTY
    reads = [(s, j) for s in range(S) for j in range(min(max(int(ended_count[s]), 0), max_ended)) if int(ended_i[s, j, 3]) >= min_hits]
    byte = lambda row, w, p: ((row[w + (p >> 2)] & 0xffffffff) >> (8 * (p & 3))) & 255   # noqa: E731
    for s, j in reads:
        best_key, hits = None, 0
        for e, row in enumerate(rows):
            if pair is not None and not (0 <= row[4] < S and pair[s][row[4]]):
                continue
            if not 0 <= now - row[6] <= window:
                continue
            mism = cost = 0
            for p in range(8):
                b, w = int(ended_i[s, j, 4 + p]), byte(row, 0, p)
                if 0 <= b < 64 and w == b:
                    continue
                c = int(confuse[min(p, 2), b, w]) if (confuse is not None and 0 <= b < 64 and w < 64) else 16
                mism += 1
                cost += min(C.weight_of(ended_f[s, j, p]), byte(row, 2, p) + 1) * c
            if mism <= max_mismatch and cost <= max_cost:
                hits += 1
                key = (cost, total - 1 - row[7])
                if best_key is None or key < best_key[:2]:
                    best_key = key + (mism, e)
        if hits:
            e = best_key[3]
            out[s, j] = (e, best_key[2], best_key[0], hits, rows[e][4], rows[e][5], rows[e][6], rows[e][7])
    new = state.copy()
    V = len(reads)
    for k, (s, j) in enumerate(reads):
        if V - k > C_:
            continue
        ids = [int(b) if 0 <= int(b) < 64 else 254 for b in ended_i[s, j, 4:12]]
        q = [C.weight_of(v) - 1 for v in ended_f[s, j, :8]]
        words = [sum(v[4 * h + i] << (8 * i) for i in range(4)) for v in (ids, q) for h in range(2)]
        t = total + k
        new[1 + t % C_] = np.array(words + [s, int(ended_i[s, j, 0]) & 0xffffffff, now, t], np.uint32).view(np.int32)
    new[0, 0] = total + V
    return out, new


def records(S, max_ended, lines, hits=3):
    """The ended records of one call: ``lines`` = [(stream, track id, ids [8], share or shares [8])] in order, everything else 0."""
    ended_i, ended_f, count = np.zeros((S, max_ended, 12), np.int32), np.zeros((S, max_ended, 12), f32), np.zeros(S, np.int32)
    for s, tid, ids, share in lines:
        j = int(count[s])
        ended_i[s, j, 0], ended_i[s, j, 3], ended_i[s, j, 4:], ended_f[s, j, :8] = tid, hits, ids, share
        count[s] += 1
    return ended_i, ended_f, count


def random_sequence(seed, S, max_ended, counts_per_call, n_ids=3, garbage=0.05):
    """[(ended_i, ended_f, ended_count, now)] of one log's calls: few ids, so that later reads match earlier ones; hits 0..4; a clock
    that moves by 0..3 per call."""
    rng = np.random.default_rng(seed)
    calls, now = [], int(rng.integers(0, 5))
    for counts in counts_per_call:
        ended_i, ended_f, ended_count = C.random_reads(rng, counts, max_ended, n_ids=n_ids, garbage=garbage)
        ended_i[:, :, 3] = rng.integers(0, 5, (S, max_ended))
        calls.append((ended_i, ended_f, ended_count, now))
        now += int(rng.integers(0, 4))
    return calls


def check_both(state, confuse, pair, rec, now, window, min_hits=1, mm=1, mc=32768):
    """One call through ``sight_update_np`` (on ``state``, in place) and through the loops: the same sight_i and state; sight_i."""
    from yolov6.utils.sight import sight_update_np
    want_i, want_state = update_loops(state, confuse, pair, *rec, now, window, min_hits, mm, mc)
    got = sight_update_np(state, confuse, pair, *rec, now, window, min_hits, mm, mc)
    assert got.dtype == np.int32 and np.array_equal(got, want_i), np.argwhere(got != want_i)[:3]
    assert np.array_equal(state, want_state), np.argwhere(state != want_state)[:3]
    return got


def slot_row(ids, q, stream, tid, stamp, seq):
    """A row of the state written out: ids and weights (q_p - 1) as bytes."""
    w = [sum(int(v[4 * h + i]) << (8 * i) for i in range(4)) for v in (ids, q) for h in range(2)]
    return np.array(w + [stream, tid, stamp, seq], np.uint32).view(np.int32)


@pytest.mark.parametrize('seed', range(6))
def test_update_np_against_the_loops(seed):
    from yolov6.utils.sight import new_state
    rng = np.random.default_rng(50 + seed)
    S, M, cap = 3, 4, int(rng.integers(1, 40))
    confuse = C.random_confuse(rng) if seed % 2 == 0 else None
    pair = (rng.random((S, S)) < 0.6).astype(np.uint8) if seed % 3 == 0 else None
    state, seen = new_state(cap), 0
    calls = random_sequence(seed, S, M, [[3, 0, 9], [2, -2, 1], [4, 4, 4], [0, 0, 0], [1, 7, 2], [4, 1, 0]])
    for k, (ended_i, ended_f, ended_count, now) in enumerate(calls):
        mm, mc = [(0, 32768), (8, 32768), (2, 3000), (1, 32768), (8, 20000), (3, int(rng.integers(0, 12000)))][k]
        got = check_both(state, confuse, pair, (ended_i, ended_f, ended_count), now, int(rng.integers(4, 12)), 1 + k % 3, mm, mc)
        seen += int((got[:, :, 0] >= 0).sum())
    assert seen > 0 and state[0, 0] > cap * (cap < 20)


# ---- scenarios: the full sight_i and the full state -------------------------------------------------------------------------------------
CAR = [3, 5, 8, 1, 20, 33, 7, 0]


def test_entry_exit_pairing_with_a_confusable_misread_and_a_pair_mask():
    from yolov6.utils.sight import new_state
    from yolov6.utils.watch import confuse_table
    confuse = confuse_table([(8, 11)], weight=4)
    seen = CAR[:2] + [11] + CAR[3:]                                    # the exit camera reads position 2 as the listed confusable
    for pair, found in ((None, True), (np.array([[0, 0], [1, 0]], np.uint8), True), (np.array([[1, 1], [0, 1]], np.uint8), False)):
        state = new_state(8)
        a = check_both(state, confuse, pair, records(2, 2, [(0, 17, CAR, 1.0)]), 100, 3600)
        assert np.array_equal(a.reshape(-1, 8), [EMPTY] * 4)
        b = check_both(state, confuse, pair, records(2, 2, [(1, 4, seen, 0.5)]), 2500, 3600, mm=1, mc=600)
        want = np.array([EMPTY] * 4, np.int32).reshape(2, 2, 8)
        if found:
            want[1, 0] = (0, 1, 128 * 4, 1, 0, 17, 100, 0)             # min(256, 128) * 4 sixteenths
            assert 2500 - b[1, 0, 6] == 2400                            # the journey time
        assert np.array_equal(b, want)
        full = new_state(8)
        full[0, 0] = 2
        full[1], full[2] = slot_row(CAR, [255] * 8, 0, 17, 100, 0), slot_row(seen, [127] * 8, 1, 4, 2500, 1)
        assert np.array_equal(state, full)
    strict = new_state(8)                                              # without the table the misread costs 16 sixteenths: above 600
    check_both(strict, None, None, records(2, 2, [(0, 17, CAR, 1.0)]), 100, 3600)
    assert np.array_equal(check_both(strict, None, None, records(2, 2, [(1, 4, seen, 0.5)]), 2500, 3600, mm=1, mc=600).reshape(-1, 8), [EMPTY] * 4)


def test_a_broken_track_names_its_first_part():
    from yolov6.utils.sight import SightLogNp
    log = SightLogNp(16, 1)
    log.update(*records(1, 3, [(0, 5, CAR, 0.9), (0, 6, [9] * 8, 0.9)]), now=40, window=50)
    got = log.update(*records(1, 3, [(0, 7, CAR, 0.8)]), now=52, window=50)
    assert got[0].tolist() == [[1 - 1, 0, 0, 1, 0, 5, 40, 0], list(EMPTY), list(EMPTY)]
    assert log.total == 3 and log.state[3].tolist()[4:] == [0, 7, 52, 2]
    log.clear()
    assert log.total == 0 and not log.state.any()


def test_window_edges_and_a_stamp_after_now():
    from yolov6.utils.sight import new_state
    for now, hit in ((110, True), (111, False), (99, False), (100, True)):
        state = new_state(4)
        check_both(state, None, None, records(1, 1, [(0, 1, CAR, 1.0)]), 100, 10)
        got = check_both(state, None, None, records(1, 1, [(0, 2, CAR, 1.0)]), now, 10)
        assert got[0, 0].tolist() == ([0, 0, 0, 1, 0, 1, 100, 0] if hit else list(EMPTY)), now
        assert state[0, 0] == 2 and state[2].tolist()[4:] == [0, 2, now, 1]
    state = new_state(4)                                               # the difference is taken in 64 bits
    check_both(state, None, None, records(1, 1, [(0, 1, CAR, 1.0)]), 0, 0)
    assert check_both(state, None, None, records(1, 1, [(0, 2, CAR, 1.0)]), 2 ** 31 - 1, 2 ** 31 - 1)[0, 0, 0] == 0
    assert check_both(state, None, None, records(1, 1, [(0, 3, CAR, 1.0)]), 2 ** 31 - 1, 2 ** 31 - 2)[0, 0].tolist() == [1, 0, 0, 1, 0, 2, 2 ** 31 - 1, 1]


def test_of_two_equally_cheap_sightings_the_more_recent_wins():
    from yolov6.utils.sight import new_state
    state = new_state(8)
    near = CAR[:7] + [9]
    check_both(state, None, None, records(2, 2, [(0, 1, CAR, 1.0), (1, 2, near, 1.0)]), 5, 100)
    check_both(state, None, None, records(2, 2, [(0, 3, [30] * 8, 1.0), (1, 4, CAR, 1.0)]), 6, 100)
    got = check_both(state, None, None, records(2, 2, [(1, 9, CAR, 1.0)]), 7, 100, mm=0)
    assert got[1, 0].tolist() == [3, 0, 0, 2, 1, 4, 6, 3] and np.array_equal(got[0], [EMPTY] * 2)
    got = check_both(state, None, None, records(2, 2, [(0, 10, near, 1.0)]), 8, 100, mm=1)      # the exact one is cheaper, however old
    assert got[0, 0].tolist() == [1, 0, 0, 4, 1, 2, 5, 1]
    assert state[0, 0] == 6


def test_the_ring():
    from yolov6.utils.sight import new_state
    plate = lambda k: [k % 37] * 8   # noqa: E731
    state = new_state(5)                                               # C = 5, 7 appends over three calls
    check_both(state, None, None, records(1, 4, [(0, k, plate(k), 1.0) for k in range(3)]), 1, 99)
    check_both(state, None, None, records(1, 4, [(0, k, plate(k), 1.0) for k in range(3, 5)]), 2, 99)
    check_both(state, None, None, records(1, 4, [(0, k, plate(k), 1.0) for k in range(5, 7)]), 3, 99)
    assert state[0, 0] == 7 and state[1:, 7].tolist() == [5, 6, 2, 3, 4] and state[1:, 5].tolist() == [5, 6, 2, 3, 4]
    got = check_both(state, None, None, records(1, 4, [(0, 50, plate(1), 1.0), (0, 51, plate(2), 1.0), (0, 52, plate(6), 1.0)]), 4, 99, mm=0)
    assert got[0].tolist() == [list(EMPTY), [2, 0, 0, 1, 0, 2, 1, 2], [1, 0, 0, 1, 0, 6, 3, 6], list(EMPTY)]     # append 1 is overwritten
    state = new_state(3)                                               # V > C in one call: the last three are written
    check_both(state, None, None, records(1, 2, [(0, 1, plate(30), 1.0)]), 0, 9)
    got = check_both(state, None, None, records(2, 3, [(s, 10 * s + j, plate(3 * s + j), 1.0) for s in range(2) for j in range(3)]
                                                + []), 1, 9)
    assert state[0, 0] == 7 and sorted(state[1:, 7].tolist()) == [4, 5, 6] and state[1 + 4 % 3, 5] == 10 and (got[:, :, 0] == -1).all()
    one = new_state(1)                                                 # C = 1: the log is the last read
    check_both(one, None, None, records(1, 2, [(0, 1, plate(1), 1.0), (0, 2, plate(2), 1.0)]), 0, 9)
    got = check_both(one, None, None, records(1, 2, [(0, 3, plate(1), 1.0), (0, 4, plate(2), 1.0)]), 1, 9, mm=0)
    assert got[0].tolist() == [list(EMPTY), [0, 0, 0, 1, 0, 2, 0, 1]] and one[1].tolist()[4:] == [0, 4, 1, 3] and one[0, 0] == 4


def test_reads_of_one_call_do_not_match_each_other_and_min_hits():
    from yolov6.utils.sight import new_state
    state = new_state(8)
    got = check_both(state, None, None, records(2, 2, [(0, 1, CAR, 1.0), (0, 2, CAR, 1.0), (1, 3, CAR, 1.0)]), 0, 9)
    assert (got[:, :, 0] == -1).all() and state[0, 0] == 3
    young = records(1, 2, [(0, 4, CAR, 1.0), (0, 5, CAR, 1.0)])
    young[0][0, 0, 3] = 2                                              # line 0 has two hits: neither looked up nor appended
    state = new_state(8)
    check_both(state, None, None, records(1, 2, [(0, 1, CAR, 1.0)]), 0, 9)
    got = check_both(state, None, None, young, 1, 9, min_hits=3)
    assert got[0].tolist() == [list(EMPTY), [0, 0, 0, 1, 0, 1, 0, 0]] and state[0, 0] == 2 and state[2, 5] == 5 and not state[3:].any()


def test_ids_outside_the_classes_are_stored_as_254_and_match_nothing():
    from yolov6.utils.sight import new_state
    odd = [3, -1, 64, 255, 300, 2 ** 31 - 1, -2 ** 31, 7]
    state = new_state(4)
    check_both(state, None, None, records(1, 1, [(0, 1, odd, 1.0)]), 0, 9)
    assert state[1].tolist() == slot_row([3, 254, 254, 254, 254, 254, 254, 7], [255] * 8, 0, 1, 0, 0).tolist()
    got = check_both(state, None, None, records(1, 1, [(0, 2, odd, 0.5)]), 0, 9, mm=8)
    assert got[0, 0].tolist() == [0, 6, 6 * 128 * 16, 1, 0, 1, 0, 0]    # itself again: the six odd positions mismatch at min(128, 256)
    assert check_both(state, None, None, records(1, 1, [(0, 3, odd, 0.5)]), 0, 9, mm=5)[0, 0].tolist() == list(EMPTY)


def test_garbage_shares_and_counts():
    from yolov6.utils.sight import new_state
    shares = np.array([np.nan, 0, -1, 2, np.inf, 1e-42, 0.5, 1], f32)
    state = new_state(4)
    check_both(state, None, None, records(1, 1, [(0, 1, CAR, shares)]), 0, 9)
    assert state[1].tolist() == slot_row(CAR, [0, 0, 0, 255, 255, 0, 127, 255], 0, 1, 0, 0).tolist()
    other = [(v + 1) % 37 for v in CAR]
    got = check_both(state, None, None, records(1, 1, [(0, 2, other, 1.0)]), 0, 9, mm=8)
    assert got[0, 0].tolist() == [0, 8, 16 * (1 + 1 + 1 + 256 + 256 + 1 + 128 + 256), 1, 0, 1, 0, 0]
    rec = records(3, 2, [(0, 1, CAR, 1.0), (0, 2, CAR, 1.0), (1, 3, CAR, 1.0), (2, 4, CAR, 1.0)])
    rec[2][:] = [7, -3, 0]                                             # above max_ended, negative, zero
    state = new_state(4)
    got = check_both(state, None, None, rec, 0, 9)
    assert state[0, 0] == 2 and state[1:3, 5].tolist() == [1, 2] and (got[:, :, 0] == -1).all()


def test_the_checks_of_the_host_form():
    from yolov6.utils.sight import SightLogNp, sight_update_np, new_state
    rec = records(2, 1, [(0, 1, CAR, 1.0)])
    for bad in (dict(capacity=0), dict(capacity=(1 << 24) + 1), dict(n_streams=0), dict(pair=np.ones((3, 2))), dict(confuse=np.zeros((3, 64, 63)))):
        with pytest.raises(ValueError):
            SightLogNp(**dict(dict(capacity=4, n_streams=2), **bad))
    log = SightLogNp(4, 2)
    for bad in (dict(now=-1), dict(window=-1), dict(min_hits=0), dict(max_mismatch=9), dict(now=2 ** 31)):
        with pytest.raises(ValueError):
            log.update(*rec, **dict(dict(now=0, window=1), **bad))
    with pytest.raises(ValueError):
        log.update(*records(3, 1, []), now=0, window=1)
    full = new_state(4)
    full[0, 0] = 2 ** 31 - 1
    with pytest.raises(ValueError, match='2\\^31'):
        sight_update_np(full, None, None, *rec, 0, 1, 1, 1, 32768)
    assert log.total == 0


# ---- PlateTrackerNp.enable_sightings ----------------------------------------------------------------------------------------------------
def test_tracker_np_enable_sightings_changes_nothing_else():
    from yolov6.utils.sight import SightLogNp, sight_update_np, new_state
    from yolov6.utils.track import PlateTrackerNp
    kw = dict(max_tracks=16, max_age=2, expand=0.5)
    calls = T.random_track_case(2)
    assert len({s for _, _, so, _ in calls for s in so if s >= 0}) >= 2             # a two-stream sequence at the least
    plain, seen = PlateTrackerNp(3, **kw), PlateTrackerNp(3, **kw)
    log = SightLogNp(6, 3)
    assert seen.last_sight is None
    seen.enable_sightings(log, window=6, min_hits=1, max_mismatch=8, max_cost=6.0)
    mirror, hits = new_state(6), 0
    for k, (det, count, stream_of, flush) in enumerate(calls):
        a, b = plain.update(det, count, stream_of, flush, 5), seen.update(det, count, stream_of, flush, 5)
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.int32), y.view(np.int32))
        want = sight_update_np(mirror, None, None, b[2], b[3], b[4], k, 6, 1, 8, 6 * 4096)
        assert seen.last_sight.shape == (3, 5, 8) and np.array_equal(seen.last_sight, want) and np.array_equal(log.state, mirror)
        assert seen.sight_now[0] == k + 1
        hits += int((want[:, :, 0] >= 0).sum())
    assert hits > 0 and log.total > 6 and plain.last_sight is None
    seen.reset()
    assert log.total > 6                                               # the log survives a reset of the tracker
    seen.enable_sightings(None)
    seen.flush_all()
    assert seen.last_sight is None
    with pytest.raises(ValueError):
        seen.enable_sightings(SightLogNp(6, 2), window=1)


# ---- C ABI: everything is checked on the host before any launch ----------------------------------------------------------------------------
def test_sight_update_rejects_bad_arguments_before_launch():
    """Fake device addresses: a launch would fault, so LP_ERR_ARG proves the host check came first."""
    from yolov6.hip import abi
    lib = abi.load()
    header = open(os.path.join(REPO, 'include', 'lp_hip.h')).read()
    assert 'LP_SIGHT_BLOCK_ENTRIES %d ' % abi.LP_SIGHT_BLOCK_ENTRIES in header and 'LP_SIGHT_QUERY_BLOCK %d ' % abi.LP_SIGHT_QUERY_BLOCK in header
    assert abi.LP_SIGHT_MAX_CAPACITY == 1 << 24 and 'LP_SIGHT_MAX_CAPACITY (1 << 24)' in header
    v = lambda p: ctypes.c_void_p(p) if p else None   # noqa: E731
    S, M, cap = 3, 5, 1000
    need = lib.lp_sight_workspace_bytes(S, M)
    assert need >= S * M * 20 + 16 and need % 16 == 0 and lib.lp_sight_workspace_bytes(2 * S, M) > need
    assert lib.lp_sight_workspace_bytes(0, M) == 0 and lib.lp_sight_workspace_bytes(S, -1) == 0 and lib.lp_sight_workspace_bytes(S, 0) > 0
    assert lib.lp_sight_workspace_bytes(1 << 20, 1 << 10) == 0
    assert lib.lp_sight_state_bytes(cap) == (cap + 1) * 32 and lib.lp_sight_state_bytes(0) == 0 and lib.lp_sight_state_bytes((1 << 24) + 1) == 0
    assert lib.lp_sight_state_bytes(1 << 24) == ((1 << 24) + 1) * 32

    def call(state=0x100000, cap=cap, confuse=0x200000, pair=0x210000, ei=0x300000, ef=0x310000, ec=0x320000, S=S, M=M, now=0x340000, window=5,
             min_hits=1, mm=1, mc=4096, sight=0x330000, ws=0x400000, ws_bytes=need):
        return lib.lp_sight_update(v(state), cap, v(confuse), v(pair), v(ei), v(ef), v(ec), S, M, v(now), window, min_hits, mm, mc, v(sight),
                                   v(ws), ws_bytes, None)

    err = lambda: lib.lp_last_error()   # noqa: E731
    assert call(cap=0) == LP_ERR_ARG and b'capacity' in err() and call(cap=(1 << 24) + 1) == LP_ERR_ARG and b'16777216' in err()
    assert call(S=0) == LP_ERR_ARG and b'n_streams' in err() and call(M=-1) == LP_ERR_ARG
    assert call(S=1 << 20, M=1 << 10) == LP_ERR_ARG and b'2^31' in err()
    assert call(window=-1) == LP_ERR_ARG and b'window' in err() and call(min_hits=0) == LP_ERR_ARG and b'min_hits' in err()
    for k, bad in (('mm', -1), ('mm', 9), ('mc', -1), ('mc', 32769)):
        assert call(**{k: bad}) == LP_ERR_ARG and b'max_mismatch' in err(), (k, bad)
    for k in ('state', 'ei', 'ef', 'ec', 'now', 'sight', 'ws'):
        assert call(**{k: 0}) == LP_ERR_ARG and b'null' in err(), k
    for k, at in (('state', 0x100008), ('sight', 0x330004), ('ws', 0x400008), ('confuse', 0x200002), ('now', 0x340002)):
        assert call(**{k: at}) == LP_ERR_ARG and b'aligned' in err(), k
    assert call(ws_bytes=need - 1) == LP_ERR_ARG and b'workspace' in err() and call(ws_bytes=0) == LP_ERR_ARG
    end = (cap + 1) * 32
    for k, at in (('sight', 0x100000 + end - 16), ('ws', 0x100000 + 16), ('state', 0x200000 - end + 16), ('sight', 0x200000 + 12272),
                  ('ws', 0x210000), ('sight', 0x300000 + S * M * 48 - 16), ('sight', 0x310000), ('ws', 0x320000), ('state', 0x340000 - end + 16),
                  ('ws', 0x330000 + 16), ('sight', 0x400000 + need - 16), ('state', 0x400000 - end + 16)):
        assert call(**{k: at}) == LP_ERR_ARG and b'overlap' in err(), (k, hex(at))
    assert call(M=0) == 0 and call(M=0, state=0, ei=0, ef=0, ec=0, now=0, sight=0, ws=0, ws_bytes=0) == 0      # no line: no launch


# ---- tools/infer.py --track --sightings on the CPU path ---------------------------------------------------------------------------------
def resighting_lines(ended, nows, cap, window, min_hits=1, mm=1, mc=32768, confuse=None, names=()):
    """resightings.txt of a one-stream run by the rule: ``ended`` = the records in the order they ended, ``nows[k]`` = the frame
    number of the update that ended record k (records of one update share a call)."""
    from yolov6.utils.sight import sight_update_np, new_state
    from yolov6.utils.track import plate_text
    state, lines, k = new_state(cap), [], 0
    while k < len(ended):
        group = [i for i in range(k, len(ended)) if nows[i] == nows[k] and all(nows[x] == nows[k] for x in range(k, i + 1))]
        ended_i, ended_f = np.zeros((1, len(group), 12), np.int32), np.zeros((1, len(group), 12), f32)
        for n, i in enumerate(group):
            ended_i[0, n], ended_f[0, n] = ended[i]
        got = sight_update_np(state, confuse, None, ended_i, ended_f, [len(group)], nows[k], window, min_hits, mm, mc)[0]
        for (ri, _), m in zip((ended[i] for i in group), got.tolist()):
            if m[0] >= 0:
                lines.append('%d %d %d %s %d %d %d %d %d %d %d' % (ri[0], ri[1], ri[2], plate_text(ri[4:12], *names), m[4], m[5], m[6], nows[k],
                                                                    m[1], m[2], m[3]))
        k += len(group)
    return lines


def end_frames(ended, n_frames, max_age):
    """The frame number of the update that ended each record of a one-stream run of ``n_frames`` frames: a track last seen at frame
    ``last`` ends in the update of frame last + max_age + 1, or in the final flush (numbered n_frames)."""
    return [min(int(ri[2]) + max_age + 1, n_frames) for ri, _ in ended]


def blinking_frames(n, gap):
    """``T._moving_frames`` with the plate hidden for the frames of ``gap``: the track breaks and is re-acquired."""
    frames = T._moving_frames(n)
    for k in gap:
        frames[k][:] = frames[k][0, 0]
    return frames


def test_infer_sightings_cpu(tmp_path, monkeypatch):
    from PIL import Image
    from yolov6.utils.synth import build_synthetic
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    m = build_synthetic(os.path.join(REPO, 'configs', 'yololps.py'), width=0.0625, sigma=1.5)
    ckpt = tmp_path / 'tiny.pt'
    torch.save({'model': m.half(), 'ema': None, 'epoch': 0}, str(ckpt))
    img_dir = tmp_path / 'imgs'
    img_dir.mkdir()
    n = 10
    for k, f in enumerate(blinking_frames(n, range(3, 7))):
        Image.fromarray(f).save(str(img_dir / ('f%02d.png' % k)))
    kw = dict(weights=str(ckpt), source=str(img_dir), yaml=None, img_size=[128, 160], conf_thres=0.06, iou_thres=0.45, max_det=20,
              device='cpu', not_save_img=True, save_txt=True, track=True, track_max_age=2, track_iou=0.25, track_expand=0.25)
    untracked = infer.run(save_dir=str(tmp_path / 'o0'), **dict(kw, track=False))
    plain = infer.run(save_dir=str(tmp_path / 'o1'), **kw)
    _, _, ended = T.track_by_hand([d.numpy() for d in untracked], 20, max_tracks=64, match_thres=0.25, new_thres=0.0, expand=0.25,
                                  max_age=2, ncls=m)
    assert (tmp_path / 'o1' / 'plates.txt').read_text().splitlines() == T.plate_lines(ended) and not (tmp_path / 'o1' / 'resightings.txt').exists()
    nows = end_frames(ended, n, 2)
    assert nows == sorted(nows)
    counts = {}
    for sub, extra in (('o2', dict(sight_window=n, sight_mismatch=8)), ('o3', dict(sight_window=n, sight_mismatch=8, sight_cost=1.5, sight_min_hits=2)),
                       ('o4', dict(sight_window=0, sight_mismatch=8))):
        again = infer.run(save_dir=str(tmp_path / sub), sightings=4, **extra, **kw)
        for a, b in zip(plain, again):
            assert torch.equal(a, b)
        for name in ('tracks.txt', 'plates.txt'):                                           # byte-identical to the run without a log
            assert (tmp_path / sub / name).read_bytes() == (tmp_path / 'o1' / name).read_bytes()
        from yolov6.utils.watch import cost_units
        want = resighting_lines(ended, nows, 4, extra['sight_window'], extra.get('sight_min_hits', 1), 8, cost_units(extra.get('sight_cost')))
        assert (tmp_path / sub / 'resightings.txt').read_text().splitlines() == want, sub
        counts[sub] = len(want)
    assert counts['o2'] >= 1 and counts['o4'] < counts['o2'] and counts['o3'] < counts['o2']      # a short window and a cost limit drop lines
    with pytest.raises(ValueError, match='track'):
        infer.run(save_dir=str(tmp_path / 'o5'), sightings=4, **dict(kw, track=False))
