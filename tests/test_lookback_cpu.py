"""The look-back delay of redaction on the CPU: the rule (yolov6/utils/lookback.py::LookbackNp, the specification of
lp_lookback_update), the frame sequence whose first frames stay readable without it, the argument checks of the C entry (no
device needed), the header / binding agreement and the ``Inferer`` argument rules.  ``late_plate_frames``, ``run_np`` and
``full_entry_rows`` are exported for tests/test_lookback_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
import test_track_cpu as C

f32 = np.float32
LP_ERR_ARG = -1


def pair(depth, n_streams=1, max_back=None, back_cap=None, **kw):
    """(PlateTrackerNp with the hold, LookbackNp over it)."""
    from yolov6.utils.lookback import LookbackNp
    from yolov6.utils.track import PlateTrackerNp
    trk = PlateTrackerNp(n_streams, **kw)
    trk.enable_hold()
    return trk, LookbackNp(trk, depth, max_back, back_cap)


def step(trk, lb, det, count, stream_of=None, flush=None, track_flush=None):
    """One tracker update and the delay line's update on what it left: the six outputs, and (det_hold, count_hold) copies."""
    trk.update(det, count, stream_of, track_flush)
    dh, ch, _ = trk.last_hold
    return lb.update(dh, ch, trk.last_tid, trk.last_slot, stream_of, flush), (dh.copy(), ch.copy())


def run_np(trk, lb, rows_per_frame, max_det, flush_last=True):
    """Stream 0, one call per frame: ({frame: (rows [count, 28], count)} of everything released, the holds per frame)."""
    det, count = C.frames_of(rows_per_frame, max_det)
    got, holds = {}, []
    for k in range(len(det)):
        fl = [int(flush_last and k == len(det) - 1)] + [0] * (trk.n_streams - 1)
        (rd, rc, rf, td, tc, tf), hold = step(trk, lb, det[k:k + 1], count[k:k + 1], [0], fl)
        holds.append(hold)
        if rf[0] >= 0:
            got[int(rf[0])] = (rd[0, :rc[0]].copy(), int(rc[0]))
            assert not rd[0, rc[0]:].any()
        for j in range(lb.depth):
            if tf[0, j] >= 0:
                got[int(tf[0, j])] = (td[0, j, :tc[0, j]].copy(), int(tc[0, j]))
    return got, holds


# ---- the crafted scene: integer coordinates and velocities, fp32 exact ---------------------------------------------------------
V = (4.0, 2.0)
SKEW = np.array([0.5, 0.25, -0.5, 0.75, 1.5, -0.25, 0.25, 0.5], f32)     # the corners are no rectangle


def scene_row(k, x0=40.0, y0=30.0, ids=(3, 7, 11, 0, 36, 21, 5, 9), conf=0.5):
    row = C.make_row((x0 + V[0] * k, y0 + V[1] * k, x0 + 60 + V[0] * k, y0 + 20 + V[1] * k), ids, conf)
    row[4:12] += SKEW
    return row


def test_back_rows_of_a_track_confirmed_after_a_gap_of_three():
    """First detection in frame 2, second in frame 5 (k = 3), D = 6: back rows exactly for frames 0, 1, 3, 4."""
    trk, lb = pair(6, max_tracks=4, max_age=4)
    frames = [[], [], [scene_row(2)], [], [], [scene_row(5, conf=0.25)]] + [[scene_row(k)] for k in range(6, 9)]
    got, holds = run_np(trk, lb, frames, 3)
    assert sorted(got) == list(range(9)) and lb.stats == dict(confirmed=1, back_rows=4) and lb.dropped[0] == 0
    confirming = holds[5][0][0, 0]
    first = scene_row(2)
    for g in range(9):
        rows, n = got[g]
        own = int(holds[g][1][0])
        assert np.array_equal(rows[:own].view(np.int32), holds[g][0][0, :own].view(np.int32))      # the frame's own rows come first
        if g in (0, 1, 3, 4):
            assert n == own + 1 and own == (1 if g in (3, 4) else 0)           # (frames 3 and 4: the hold's row at zero velocity)
            m = f32(g - 2)
            assert np.array_equal(rows[own, :12], first[:12] + np.tile(np.array(V, f32) * m, 6))
            assert np.array_equal(rows[own, 12:].view(np.int32), confirming[12:].view(np.int32))
        else:
            assert n == own == 1
    assert tuple(trk.vel[0, 0]) == V


def test_velocity_is_the_trackers_bit_for_bit():
    rng = np.random.default_rng(3)
    trk, lb = pair(4, max_tracks=2, max_age=4, expand=0.5)
    a = C.make_row((10.3 + rng.random(), 20.1, 50.9, 33.3 + rng.random()))
    b = C.make_row((17.7 + rng.random(), 22.9, 58.1, 36.3 + rng.random()))
    det, count = C.frames_of([[a], [], [], [b]], 2)
    for k in range(4):
        out, _ = step(trk, lb, det[k:k + 1], count[k:k + 1], [0])
    assert lb.stats['confirmed'] == 1 and trk.hits[0, 0] == 2
    vel = trk.vel[0, 0].copy()
    assert vel[0] != np.round(vel[0]) and not np.array_equal(vel, np.zeros(2, f32))
    for g in (1, 2):
        m = f32(g)
        want = a[:12] + np.tile(np.array([vel[0] * m, vel[1] * m], f32), 6)
        e = lb.ring[0, g % 4]
        assert lb.ring_count[0, g % 4] == 2 and np.array_equal(e[1, :12].view(np.int32), want.view(np.int32))


@pytest.mark.parametrize('case', ['frame0', 'max_back', 'base'])
def test_targets_are_clipped(case):
    if case == 'frame0':            # born at frame 1, confirmed at 2: only frame 0 lies before it
        trk, lb = pair(6, max_tracks=2)
        frames, want = [[], [scene_row(1)], [scene_row(2)]], {0: 1, 1: 1, 2: 1}
    elif case == 'max_back':        # born at 4, confirmed at 5, max_back = 1: frame 3 alone
        trk, lb = pair(6, max_back=1, max_tracks=2)
        frames, want = [[]] * 4 + [[scene_row(4)], [scene_row(5)]], {0: 0, 1: 0, 2: 0, 3: 1, 4: 1, 5: 1}
    else:                           # frames 0..3 flushed (base = 4), born at 5, confirmed at 6: frame 4 alone
        trk, lb = pair(6, max_tracks=2)
        det, count = C.frames_of([[]] * 4, 2)
        tf = step(trk, lb, det, count, [0] * 4, [1])[0][5]
        assert tf[0].tolist() == [0, 1, 2, 3, -1, -1] and lb.base[0] == 4
        frames, want = [[], [scene_row(5)], [scene_row(6)]], {4: 1, 5: 1, 6: 1}
    got, _ = run_np(trk, lb, frames, 2)
    assert {g: n for g, (_, n) in got.items()} == want and lb.stats['confirmed'] == 1


def full_entry_rows(max_det, max_tracks):
    """Frames for trackers of ``max_tracks`` slots with max_age = 1: frame 0 starts ``max_tracks`` tracks, frame 1 shows
    ``max_det`` rows elsewhere (every track is held: count_hold = max_det + max_tracks, a full entry), frame 2 starts three
    tracks in the freed slots, frame 3 confirms them: all three want a back row in frames 0 and 1."""
    p = [C.make_row((100 * k, 0, 100 * k + 60, 20)) for k in range(max_tracks)]
    q = [C.make_row((100 * k, 300, 100 * k + 60, 320), conf=0.0) for k in range(max_det)]
    r2 = [scene_row(2, y0=600 + 100 * k) for k in range(3)]
    r3 = [scene_row(3, y0=600 + 100 * k) for k in range(3)]
    return [p, q, r2, r3]


def test_back_cap_one_lower_row_wins():
    trk, lb = pair(5, back_cap=1, max_tracks=3, max_age=1, new_thres=0.2)
    got, holds = run_np(trk, lb, full_entry_rows(4, 3), 4)
    assert [int(h[1][0]) for h in holds] == [3, 7, 3, 3]                       # frame 1 is full: 4 rows + 3 held
    assert lb.stats['confirmed'] == 3 and lb.dropped[0] == 2                   # entry 1 takes one of three, entry 0 all
    assert got[1][1] == 8 and got[0][1] == 6
    low = scene_row(2, y0=600)
    assert np.array_equal(got[1][0][7, :12], low[:12] - np.tile(np.array(V, f32), 6))      # the lower row's track


def test_back_cap_one_two_tracks_dropped_is_one():
    """Two tracks confirming in one frame, back_cap = 1, a full entry: the lower row wins and dropped == 1."""
    trk, lb = pair(5, back_cap=1, max_tracks=2, max_age=1, new_thres=0.2)
    frames = full_entry_rows(2, 2)
    frames[2], frames[3] = frames[2][:2], frames[3][:2]
    got, holds = run_np(trk, lb, frames, 2)
    assert int(holds[1][1][0]) == 4 and lb.stats['confirmed'] == 2 and lb.dropped[0] == 1
    assert got[1][1] == 5 and got[0][1] == 4
    assert np.array_equal(got[1][0][4, :12], scene_row(2, y0=600)[:12] - np.tile(np.array(V, f32), 6))


def test_reused_slot_starts_over():
    trk, lb = pair(4, max_tracks=1, max_age=0)
    far = C.make_row(C.FAR, ids=(9,) * 8)
    det, count = C.frames_of([[C.make_row(C.A)], [far], [far]], 2)
    for k in range(3):
        step(trk, lb, det[k:k + 1], count[k:k + 1], [0])
        assert (lb.idp1[0, 0], lb.seen[0, 0], lb.first[0, 0]) == [(1, 1, 0), (2, 1, 1), (2, 2, 1)][k]
        assert lb.stats['confirmed'] == (1 if k == 2 else 0)
    assert lb.ring_count[0].tolist() == [2, 1, 1, 0]                           # frame 0 got the back row of track 1


def test_untracked_frame_is_released_at_once_and_changes_no_state():
    trk, lb = pair(3, n_streams=2, max_tracks=2)
    det, count = C.frames_of([[scene_row(0)], [scene_row(1)]], 2)
    step(trk, lb, det, count, [0, 0])
    before = lb.state_words().copy()
    det, count = C.frames_of([[scene_row(7), scene_row(9)]], 2)
    (rd, rc, rf, td, tc, tf), (dh, ch) = step(trk, lb, det, count, [-1])
    assert rf.tolist() == [-2] and rc.tolist() == [2] and rd.shape == (1, 2 + 2 + 2, 28)
    assert np.array_equal(rd[0, :2], det[0]) and not rd[0, 2:].any()
    assert np.array_equal(lb.state_words(), before) and np.all(tf == -1) and not td.any() and not tc.any()


def test_tail_is_in_ascending_frame_order_and_release_order_within_a_call():
    trk, lb = pair(3, n_streams=2, max_tracks=2, new_thres=2.0)                # (no tracks: rows pass through)
    rows = [[C.make_row((k, k, k + 40, k + 12))] for k in range(8)]
    det, count = C.frames_of(rows, 2)
    (rd, rc, rf, td, tc, tf), _ = step(trk, lb, det[:7], count[:7], [1, 1, 0, 1, 1, 1, 1])
    assert rf.tolist() == [-1, -1, -1, -1, 0, 1, 2]                            # stream 1: frame b - 3 of it leaves at its b-th frame
    assert [rd[b, 0, 0] for b in (4, 5, 6)] == [0, 1, 3] and rc.tolist() == [0, 0, 0, 0, 1, 1, 1]     # (its frame 2 is b = 3)
    assert np.all(tf == -1) and lb.f.tolist() == [1, 6] and lb.base.tolist() == [0, 3]
    (rd, rc, rf, td, tc, tf), _ = step(trk, lb, det[7:], count[7:], [1], [0, 1])
    assert rf.tolist() == [3] and rd[0, 0, 0] == 4
    assert tf.tolist() == [[-1, -1, -1], [4, 5, 6]] and tc.tolist() == [[0, 0, 0], [1, 1, 1]]
    assert [td[1, j, 0, 0] for j in range(3)] == [5, 6, 7]
    assert lb.base.tolist() == [0, 7] and not td[0].any()
    td2 = step(trk, lb, det[:0], count[:0], [], [1, 1])[0]                     # B == 0 with a flush: tails only
    assert td2[5].tolist() == [[0, -1, -1], [-1, -1, -1]] and td2[3][0, 0, 0, 0] == 2 and td2[0].shape == (0, 6, 28)


def test_without_a_confirmed_track_the_rows_are_the_hold_rows_of_d_frames_earlier():
    calls = C.random_track_case(7, n_streams=1, max_det=6, Bs=[1] * 14)
    trk, lb = pair(4, max_tracks=4, new_thres=9.0)                             # no row ever starts a track
    holds = []
    for det, count, stream_of, flush in calls:
        (rd, rc, rf, *_), hold = step(trk, lb, det, count, [0])
        holds.append(hold)
        assert rf[0] == len(holds) - 5 or (len(holds) < 5 and rf[0] == -1)
        if rf[0] >= 0:
            dh, ch = holds[rf[0]]
            n = min(max(int(ch[0]), 0), dh.shape[1])
            assert rc[0] == n and np.array_equal(rd[0, :n].view(np.int32), dh[0, :n].view(np.int32)) and not rd[0, n:].view(np.int32).any()
    assert lb.stats['confirmed'] == 0 and lb.f[0] == 14 and lb.base[0] == 10 and sum(int(h[1][0]) for h in holds) > 0


def test_reset_and_state_layout():
    from yolov6.utils.lookback import state_words
    trk, lb = pair(5, n_streams=2, max_tracks=3)
    det, count = C.frames_of([[scene_row(0)], [scene_row(1)], [scene_row(0)]], 2)
    step(trk, lb, det, count, [0, 0, 1])
    w = lb.state_words()
    rows = 2 + 3 + 3
    assert w.shape == (2, state_words(3, 5, rows)) and w.shape[1] == 4 + 3 * 16 + 8 + 5 * rows * 28 and w.shape[1] % 4 == 0
    assert w[:, 0].tolist() == [2, 1] and w[0, 4:7].tolist() == [1, 2, 0] and w[0, 4 + 48:4 + 48 + 2].tolist() == [1, 1]
    lb.reset([0])
    w2 = lb.state_words()
    assert not w2[0].any() and np.array_equal(w2[1], w[1])


def test_arguments():
    from yolov6.utils.lookback import LookbackNp
    from yolov6.utils.track import PlateTrackerNp
    trk = PlateTrackerNp(1)
    with pytest.raises(RuntimeError):
        LookbackNp(trk, 4)
    trk.enable_hold()
    for bad in (dict(depth=0), dict(depth=33), dict(depth=4, max_back=-1), dict(depth=4, back_cap=-1), dict(depth=4, mode='blur'),
                dict(depth=4, cell=7), dict(depth=4, fill=(0, 0, 256))):
        with pytest.raises(ValueError):
            LookbackNp(trk, **bad)
    lb = LookbackNp(trk, 32, max_back=0, back_cap=0)
    assert (lb.depth, lb.max_back, lb.back_cap) == (32, 0, 0) and LookbackNp(trk, 3).max_back == 3 and LookbackNp(trk, 3).back_cap == 64
    with pytest.raises(RuntimeError):
        lb.push([np.zeros((4, 4, 3), np.uint8)])                               # no update yet


# ---- the test that fails without the feature: the frames before the first detection -------------------------------------------
H, W, PW, PH, MARGIN, LATE, DEPTH = 240, 320, 96, 32, 0.1, 3, 6
FILL = (255, 255, 255)


def late_plate_frames(n=10):
    """(frames [n] of 240 x 320 BGR random bytes in 1..254 with a 96 x 32 plate moving (7, 3) px per frame, rows per frame, box
    per frame): the detector misses frames 0 .. LATE - 1."""
    rng = np.random.default_rng(11)
    plate = rng.integers(1, 255, (PH, PW, 3), dtype=np.uint8)
    frames, rows, boxes = [], [], []
    for k in range(n):
        f = rng.integers(1, 255, (H, W, 3), dtype=np.uint8)
        x, y = 20 + 7 * k, 30 + 3 * k
        f[y:y + PH, x:x + PW] = plate
        frames.append(f)
        boxes.append((x, y, x + PW, y + PH))
        rows.append([] if k < LATE else [C.make_row(boxes[-1])])
    return frames, rows, boxes


def check_late_plate(frames, boxes, hold_only, looked_back):
    """The assertions of the sequence on two lists of redacted frames (arrays)."""
    assert len(hold_only) == len(looked_back) == len(frames)
    for k, (f, a, b) in enumerate(zip(frames, hold_only, looked_back)):
        x1, y1, x2, y2 = boxes[k]
        if k < LATE:
            assert np.array_equal(a, f), k                                      # the hold alone stores the plate readable
            assert np.all(b[y1:y2, x1:x2] == 255), k                            # every pixel of the true rectangle is the fill colour
            gx, gy = MARGIN * PW / 2, MARGIN * PH / 2
            keep = np.ones((H, W), bool)
            keep[int(np.floor(y1 - gy)):int(np.ceil(y2 + gy)), int(np.floor(x1 - gx)):int(np.ceil(x2 + gx))] = False
            assert np.array_equal(b[keep], f[keep]), k                          # and no byte outside it plus the margin changed
        else:
            assert np.array_equal(a, b) and np.all(b[y1:y2, x1:x2] == 255), k


def test_late_plate_is_covered_before_its_first_detection():
    from yolov6.utils.lookback import LookbackNp
    from yolov6.utils.redact import redact_plates_np
    from yolov6.utils.track import PlateTrackerNp
    frames, rows, boxes = late_plate_frames()
    det, count = C.frames_of(rows, 4)
    kw = dict(mode='fill', cell=16, margin=MARGIN, fill=FILL)
    trk = PlateTrackerNp(1, max_tracks=4)
    trk.enable_hold()
    hold_only = []
    for k, f in enumerate(frames):
        trk.update(det[k:k + 1], count[k:k + 1], [0])
        hold_only += redact_plates_np([f], trk.last_hold[0], trk.last_hold[1], **kw)[0]
    trk = PlateTrackerNp(1, max_tracks=4)
    trk.enable_hold()
    lb = LookbackNp(trk, DEPTH, **kw)
    out = []
    for k, f in enumerate(frames):
        trk.update(det[k:k + 1], count[k:k + 1], [0])
        done = lb.push([f], [0])
        assert [(s, g) for s, g, _ in done] == ([(0, k - DEPTH)] if k >= DEPTH else []) and lb.pending(0) == min(k + 1, DEPTH)
        out += done
    trk.flush_all(max_det=4)
    out += lb.flush_all()
    assert [(s, g) for s, g, _ in out] == [(0, k) for k in range(len(frames))] and lb.pending(0) == 0 and lb.dropped[0] == 0
    check_late_plate(frames, boxes, hold_only, [fr for _, _, fr in out])


def test_push_hands_untracked_frames_back_at_once():
    from yolov6.utils.lookback import LookbackNp
    from yolov6.utils.track import PlateTrackerNp
    frames, rows, boxes = late_plate_frames(5)
    trk = PlateTrackerNp(2, max_tracks=4)
    trk.enable_hold()
    lb = LookbackNp(trk, 2, mode='fill', margin=MARGIN, fill=FILL)
    det, count = C.frames_of(rows, 4)
    trk.update(det[2:5], count[2:5], [1, -1, -1])
    done = lb.push([frames[2], frames[3]], [1, -1, -1])                        # the third slot is padding: no frame
    assert [(s, g) for s, g, _ in done] == [(-1, -2)] and lb.pending(1) == 1
    x1, y1, x2, y2 = boxes[3]
    assert np.all(done[0][2][y1:y2, x1:x2] == 255) and (frames[3][y1:y2, x1:x2] != 255).any()
    with pytest.raises(ValueError):
        lb.push([frames[2]], [1, 1, -1])                                        # frame 1 of stream 1 is missing


def test_flush_before_the_first_frame_fixes_no_entry_size_and_a_push_that_raises_moves_nothing():
    from yolov6.utils.lookback import LookbackNp
    from yolov6.utils.track import PlateTrackerNp
    frames, rows, boxes = late_plate_frames(5)
    det, count = C.frames_of(rows, 4)
    trk = PlateTrackerNp(1, max_tracks=4)
    trk.enable_hold()
    lb = LookbackNp(trk, 2, mode='fill')
    trk.flush_all()
    assert lb.flush_all() == [] and lb.ring is None
    tails = lb.update(*trk.last_hold[:2], trk.last_tid, trk.last_slot, [], [1])    # the rule alone: all-empty tails, still no size
    assert lb.ring is None and np.all(tails[5] == -1) and not tails[3].any()
    trk.update(det[:3], count[:3], [0] * 3)
    assert [(s, g) for s, g, _ in lb.push(frames[:3], [0] * 3)] == [(0, 0)] and lb.ring.shape[2] == 4 + 4 + 4
    trk.update(np.zeros((1, 6, 28), f32), [0], [0])                            # another max_det: the push raises ...
    with pytest.raises(ValueError, match='rows'):
        lb.push(frames[3:4], [0])
    assert lb.pending(0) == 2 and (lb.f[0], lb.base[0]) == (3, 1)              # ... and neither counters nor frames have moved
    trk.update(det[3:4], count[3:4], [0])
    assert [(s, g) for s, g, _ in lb.push(frames[3:4], [0], [1])] == [(0, 1), (0, 2), (0, 3)] and lb.pending(0) == 0
    assert (lb.f[0], lb.base[0]) == (4, 4)


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------
def test_lookback_update_rejects_bad_arguments_before_launch():
    from yolov6.hip import abi
    lib = abi.load()
    v = lambda p: ctypes.c_void_p(p) if p else None   # noqa: E731

    def call(state=0x10000000, n_streams=2, max_tracks=8, depth=4, max_back=4, back_cap=8, det_hold=0x100000, count_hold=0x2000,
             tid=0x3000, slot=0x4000, B=3, max_det=10, hold_rows=18, so=(0, 1, -1), rel_det=0x200000, rel_count=0x5000, rel_frame=0x6000,
             tail_det=0x300000, tail_count=0x7000, tail_frame=0x8000):
        return lib.lp_lookback_update(v(state), n_streams, max_tracks, depth, max_back, back_cap, v(det_hold), v(count_hold), v(tid),
                                      v(slot), B, max_det, hold_rows, (ctypes.c_int * 3)(*so), None, v(rel_det), v(rel_count),
                                      v(rel_frame), v(tail_det), v(tail_count), v(tail_frame), None)

    err = lambda: lib.lp_last_error()   # noqa: E731
    for bad in (dict(depth=0), dict(depth=33), dict(max_back=-1), dict(back_cap=-1)):
        assert call(**bad) == LP_ERR_ARG and b'depth' in err(), bad
    for bad in (dict(n_streams=0), dict(max_tracks=0), dict(max_tracks=129)):
        assert call(**bad) == LP_ERR_ARG and b'max_tracks' in err(), bad
    for bad in (dict(max_det=0), dict(hold_rows=9), dict(B=-1), dict(hold_rows=2 ** 31 // 28 - 7, back_cap=8)):
        assert call(**bad) == LP_ERR_ARG and b'hold_rows' in err(), bad
    assert call(hold_rows=2 ** 31 // 28 - 8, back_cap=7, so=(0, 5, 0), rel_det=1 << 40, tail_det=1 << 42) == LP_ERR_ARG     # rows * 28 just
    assert b'stream 5' in err()                                                                                          # below 2^31
    for k in ('state', 'det_hold', 'count_hold', 'tid', 'slot', 'rel_det', 'rel_count', 'rel_frame', 'tail_det', 'tail_count', 'tail_frame'):
        assert call(**{k: 0}) == LP_ERR_ARG and b'null' in err(), k
    for k in ('state', 'det_hold', 'rel_det', 'tail_det'):
        assert call(**{k: 0x400008}) == LP_ERR_ARG and b'aligned' in err(), k
    for so in ((0, 2, 0), (-2, 0, 0)):
        assert call(so=so) == LP_ERR_ARG and b'stream' in err()
    hold_bytes, rel_bytes, tail_bytes = 3 * 18 * 112, 3 * 26 * 112, 2 * 4 * 26 * 112
    assert call(rel_det=0x100000) == LP_ERR_ARG and b'overlap' in err()
    assert call(rel_det=0x100000 + hold_bytes - 16) == LP_ERR_ARG and b'overlap' in err()
    assert call(rel_det=0x100000 - rel_bytes + 16) == LP_ERR_ARG and b'overlap' in err()
    assert call(tail_det=0x100000 + hold_bytes - 16) == LP_ERR_ARG and b'overlap' in err()
    assert call(tail_det=0x100000 - tail_bytes + 16) == LP_ERR_ARG and b'overlap' in err()
    assert call(tail_det=0x200000 + rel_bytes - 16) == LP_ERR_ARG and b'overlap' in err()
    assert call(rel_det=0x300000 + tail_bytes - 16) == LP_ERR_ARG and b'overlap' in err()
    state_bytes = lib.lp_lookback_state_bytes(2, 8, 4, 26)
    for k in ('rel_det', 'rel_count', 'rel_frame', 'tail_det', 'tail_count', 'tail_frame'):                 # no output inside the state
        assert call(**{k: 0x10000000 + state_bytes - 16}) == LP_ERR_ARG and b'overlap' in err(), k
    assert call(rel_frame=0x5000 + 8) == LP_ERR_ARG and b'overlap' in err()                                 # rel_count is 12 bytes
    assert call(tail_frame=0x7000 + 28) == LP_ERR_ARG and b'overlap' in err()                               # tail_count is 32 bytes
    assert call(tail_count=0x3000 + 116) == LP_ERR_ARG and b'overlap' in err()                              # tid is 120 bytes
    assert call(rel_count=0x2000 + 8) == LP_ERR_ARG and b'overlap' in err()                                 # count_hold is 12 bytes


def test_lookback_state_bytes():
    from yolov6.hip import abi
    from yolov6.utils.lookback import state_words
    lib = abi.load()
    assert lib.lp_lookback_state_bytes(3, 8, 5, 28) == 3 * 4 * state_words(8, 5, 28) == 3 * 4 * (4 + 128 + 8 + 5 * 28 * 28)
    assert lib.lp_lookback_state_bytes(1, 128, 32, 428) % 16 == 0 and lib.lp_lookback_state_bytes(1, 1, 1, 1) == 4 * (4 + 16 + 4 + 28)
    for bad in ((0, 8, 5, 28), (1, 0, 5, 28), (1, 129, 5, 28), (1, 8, 0, 28), (1, 8, 33, 28), (1, 8, 5, 0), (1, 8, 5, 2 ** 31 // 28 + 1)):
        assert lib.lp_lookback_state_bytes(*bad) == 0, bad


C_TYPES = {'int': ctypes.c_int, 'const int*': ctypes.POINTER(ctypes.c_int)}


def test_header_and_binding_agree_on_the_signature():
    """Every parameter of the two prototypes in include/lp_hip.h, in order, against abi.SYMBOLS (any other pointer: c_void_p)."""
    from yolov6.hip import abi
    header = open(os.path.join(REPO, 'include', 'lp_hip.h')).read()
    for name, restype, n_args in (('lp_lookback_update', ctypes.c_int, 22), ('lp_lookback_state_bytes', ctypes.c_size_t, 4)):
        m = re.search(r'^(int|size_t) %s\((.*?)\);' % name, header, re.S | re.M)
        assert m, name
        params = [re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', '', p, flags=re.S)).strip() for p in m.group(2).split(',')]
        want = []
        for p in params:
            ctype = p.rsplit(' ', 1)[0] if '*' not in p else p[:p.rindex('*') + 1]
            want.append(C_TYPES.get(ctype, ctypes.c_void_p if '*' in ctype else None))
        assert None not in want and len(want) == n_args, params
        assert abi.SYMBOLS[name] == (restype, want), name
    assert abi.LP_LOOKBACK_MAX_DEPTH == int(re.search(r'#define LP_LOOKBACK_MAX_DEPTH (\d+)', header).group(1)) == 32


# ---- Inferer ---------------------------------------------------------------------------------------------------------------------
def test_redact_lookback_needs_track_redact_and_hold():
    from yolov6.core.inferer import Inferer
    for kw in (dict(track=True, redact='fill'), dict(track=True, redact_hold=False), dict(redact='mosaic'), dict()):
        with pytest.raises(ValueError, match='redact_lookback'):
            Inferer('nowhere', 'nothing.pt', 'cpu', None, [128, 160], False, redact_lookback=4, **kw)
    for kw in (dict(redact_lookback=0), dict(redact_lookback=33), dict(redact_lookback=4, redact_lookback_max_back=-1)):
        with pytest.raises(ValueError, match='lookback'):
            Inferer('nowhere', 'nothing.pt', 'cpu', None, [128, 160], False, track=True, redact='fill', redact_hold=True, **kw)


def lookback_by_hand(frames, dets, max_det, depth, redact, **kw):
    """``PlateTrackerNp`` with the hold and ``LookbackNp`` over the untracked per-frame detections of one stream, one update
    per frame, then the flush: the redacted frames in frame order."""
    from yolov6.utils.lookback import LookbackNp
    from yolov6.utils.track import PlateTrackerNp
    trk = PlateTrackerNp(1, **kw)
    trk.enable_hold()
    lb = LookbackNp(trk, depth, **redact)
    out = []
    for f, d in zip(frames, dets):
        pad = np.zeros((1, max_det, 28), f32)
        pad[0, :len(d)] = d
        trk.update(pad, [len(d)], max_ended=2 * trk.max_tracks)
        out += lb.push([f])
    trk.flush_all()
    out += lb.flush_all()
    assert [g for _, g, _ in out] == list(range(len(frames)))
    return [f for _, _, f in out]


def late_frames(n=8, late=3):
    """``_moving_frames`` with the first ``late`` frames replaced by unrelated noise: what the later frames track is born after
    frame 0, so its confirmation reaches back."""
    frames = C._moving_frames(n)
    rng = np.random.default_rng(5)
    for k in range(late):
        frames[k] = rng.integers(0, 255, frames[k].shape, dtype=np.uint8)
    return frames


@pytest.mark.parametrize('tile', [None, (64, 64)], ids=['whole', 'tiled'])
def test_infer_redact_lookback_cpu(tmp_path, monkeypatch, tile):
    import importlib
    import sys
    import torch
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
    frames = late_frames()
    for k, f in enumerate(frames):
        Image.fromarray(f).save(str(img_dir / ('f%02d.png' % k)))
    kw = dict(weights=str(ckpt), source=str(img_dir), yaml=None, img_size=[128, 160], conf_thres=0.06, iou_thres=0.45, max_det=5,
              device='cpu', not_save_img=True, tile=tile)
    plain = infer.run(save_dir=str(tmp_path / 'o1'), **kw)
    tkw = dict(track=True, track_max_age=2, track_iou=0.25, track_expand=0.25, redact='fill', redact_hold=True)
    held = infer.run(save_dir=str(tmp_path / 'o2'), **tkw, **kw)
    back = infer.run(save_dir=str(tmp_path / 'o3'), redact_lookback=4, **tkw, **kw)
    for a, b in zip(held, back):
        assert torch.equal(a, b)                                                # every other output is what it is without the delay
    for name in ('tracks.txt', 'plates.txt'):
        assert (tmp_path / 'o2' / name).read_bytes() == (tmp_path / 'o3' / name).read_bytes()
    want = lookback_by_hand([f[:, :, ::-1] for f in frames], [d.numpy() for d in plain], 5, 4, dict(mode='fill', margin=0.1),
                            max_tracks=64, match_thres=0.25, new_thres=0.0, expand=0.25, max_age=2, ncls=m)
    differs = 0
    for k, w in enumerate(want):
        got = np.asarray(Image.open(str(tmp_path / 'o3' / 'redacted' / ('f%02d.png' % k))))
        assert np.array_equal(got, w[:, :, ::-1]), k
        differs += int(not np.array_equal(got, np.asarray(Image.open(str(tmp_path / 'o2' / 'redacted' / ('f%02d.png' % k))))))
    assert differs >= 1                                                         # at least one frame got a back row, and it shows
