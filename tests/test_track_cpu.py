"""Plate tracking on the CPU: the checks of the specification itself (yolov6/utils/track.py::PlateTrackerNp), the argument
checks of lp_track_update (no device needed) and ``tools/infer.py --track`` on the CPU path.  ``plate_scene`` and
``random_track_case`` are exported for tests/test_track_gpu.py."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

LP_ERR_ARG = -1
f32 = np.float32
NCLS = (31, 24, 37, 37, 37, 37, 37, 37)
NAN = float('nan')


def make_row(box, ids=(1, 2, 3, 4, 5, 6, 7, 8), conf=0.9):
    """One detection row: xyxy, the box's corners TL BL BR TR, eight confidences (a scalar or eight), eight ids."""
    x1, y1, x2, y2 = box
    r = np.zeros(28, f32)
    r[0:4] = box
    r[4:12] = (x1, y1, x1, y2, x2, y2, x2, y1)
    r[12:20] = conf
    r[20:28] = ids
    return r


def frames_of(rows_per_frame, max_det):
    """(det [F, max_det, 28], count [F]) of lists of rows."""
    det, count = np.zeros((len(rows_per_frame), max_det, 28), f32), np.zeros(len(rows_per_frame), np.int32)
    for b, rows in enumerate(rows_per_frame):
        for r, row in enumerate(rows):
            det[b, r] = row
        count[b] = len(rows)
    return det, count


def run_stream(trk, rows_per_frame, max_det, s=0, flush=False, max_ended=None):
    """Frame by frame (one update per frame) through stream ``s``: lists of det_out / tid per frame and all ended records."""
    outs, tids, ended = [], [], []
    for k, rows in enumerate(rows_per_frame):
        det, count = frames_of([rows], max_det)
        fl = [int(flush and k == len(rows_per_frame) - 1 and t == s) for t in range(trk.n_streams)]
        o, t, ei, ef, ec = trk.update(det, count, stream_of=[s], flush=fl, max_ended=max_ended)
        outs.append(np.array(o[0]))
        tids.append(np.array(t[0]))
        ended += [(np.array(ei[s, j]), np.array(ef[s, j])) for j in range(min(int(ec[s]), ei.shape[1]))]
    return outs, tids, ended


# ---- the scene by construction ---------------------------------------------------------------------------------------------
SCENE_MAX_AGE = 3


def plate_scene(seed=5, frames=40):
    """Three 60x20 plates moving 6, -4 and 0 px per frame in x at rows 100 px apart, all coordinates integers: consecutive boxes
    overlap with IoU >= 54/66 without any expand, and after two hits the constant velocity predicts the box exactly.  Each plate
    is missing in some frames, no gap longer than max_age = 3 except ONE gap of 4 on plate 2, which splits it into two tracks.
    In 30 % of its frames one head of a plate reads a wrong id at conf 0.5, otherwise the true id at conf 0.9.
    Returns (rows_per_frame, truth): truth[f] = [(plate, expected track id, hits of that track so far)] per row of frame f."""
    rng = np.random.default_rng(seed)
    plates = [dict(x=100, y=50, v=6, ids=(3, 7, 11, 0, 36, 21, 5, 9)), dict(x=400, y=150, v=-4, ids=(30, 23, 1, 2, 3, 4, 5, 6)),
              dict(x=250, y=250, v=0, ids=(0, 0, 35, 34, 33, 32, 31, 30))]
    missing = [{5, 6, 7, 30}, {10, 20, 21}, {15, 16, 17, 18, 33, 34}]         # plate 2: frames 15..18 = max_age + 1
    track_of = lambda p, f: 3 if (p == 2 and f > 18) else p                    # noqa: E731  (ids in creation order)
    hits = {}
    votes = {}                                                                 # (track, head) -> [true weight, wrong weight]
    rows_per_frame, truth = [], []
    for f in range(frames):
        rows, tr = [], []
        for p, pl in enumerate(plates):
            if f in missing[p]:
                continue
            t = track_of(p, f)
            hits[t] = hits.get(t, 0) + 1
            ids, conf = list(pl['ids']), [0.9] * 8
            if rng.random() < 0.3:
                h = int(rng.integers(0, 8))
                ids[h], conf[h] = (ids[h] + 1) % NCLS[h], 0.5
            for h in range(8):
                w = votes.setdefault((t, h), [0.0, 0.0])
                w[0 if ids[h] == pl['ids'][h] else 1] += conf[h]
                # by construction the true id leads every head from the third hit on (0.01: far above any fp32 rounding)
                assert hits[t] < 3 or w[0] > w[1] + 0.01, (t, h, f)
            x = pl['x'] + pl['v'] * f
            rows.append(make_row((x, pl['y'], x + 60, pl['y'] + 20), ids, conf))
            tr.append((p, t, hits[t]))
        rows_per_frame.append(rows)
        truth.append(tr)
    assert max(len(r) for r in rows_per_frame) == 3 and any(c != 0.9 for rows in rows_per_frame for r in rows for c in r[12:20])
    return rows_per_frame, truth, plates


def check_scene(outs, tids, ended, truth, plates):
    """The assertions of the scene on a tracker's outputs (per frame det_out / tid, the ended records after the flush)."""
    assert len(ended) == 4                                                     # the over-long gap splits plate 2
    by_id = {int(ri[0]): (ri, rf) for ri, rf in ended}
    assert sorted(by_id) == [0, 1, 2, 3]
    for t, p in enumerate((0, 1, 2, 2)):
        ri, rf = by_id[t]
        assert tuple(ri[4:12]) == plates[p]['ids']                             # every ended read equals the true plate
        assert np.all(rf[:8] > 0.5) and np.all(rf[:8] <= 1.0)
    assert by_id[2][0][2] == 14 and by_id[3][0][1] == 19                       # last of the first half, first of the second
    assert [int(by_id[t][0][3]) for t in range(4)] == [max(h for fr in truth for (_, tt, h) in fr if tt == t) for t in range(4)]
    for f, tr in enumerate(truth):
        assert list(tids[f][:len(tr)]) == [t for _, t, _ in tr], f             # constant along each plate between long gaps
        assert np.all(tids[f][len(tr):] == -1)
        for r, (p, t, h) in enumerate(tr):
            if h >= 3:
                assert tuple(outs[f][r, 20:28]) == plates[p]['ids'], (f, r)
                assert np.all(outs[f][r, 12:20] > 0.5)


def test_scene_four_plates():
    from yolov6.utils.track import PlateTrackerNp
    rows_per_frame, truth, plates = plate_scene()
    trk = PlateTrackerNp(1, max_tracks=8, match_thres=0.3, expand=0.5, max_age=SCENE_MAX_AGE)
    outs, tids, ended = run_stream(trk, rows_per_frame, 5, flush=True)
    check_scene(outs, tids, ended, truth, plates)
    assert not trk.live(0).any() and trk.dropped[0] == 0
    # ... and as ONE call of 40 frames
    trk = PlateTrackerNp(1, max_tracks=8, match_thres=0.3, expand=0.5, max_age=SCENE_MAX_AGE)
    det, count = frames_of(rows_per_frame, 5)
    o, t, ei, ef, ec = trk.update(det, count, stream_of=[0] * len(det), flush=[1])
    assert ec[0] == 4
    check_scene(list(o), list(t), [(ei[0, k], ef[0, k]) for k in range(4)], truth, plates)
    assert all(np.array_equal(a, b) for a, b in zip(outs, o))


# ---- the rules, case by case ----------------------------------------------------------------------------------------------------
A, FAR = (10, 10, 70, 30), (300, 200, 360, 220)


def test_iou_matrix_is_the_predicate_of_overlaps():
    from yolov6.utils.tiles import overlaps
    from yolov6.utils.track import iou_matrix
    rng = np.random.default_rng(0)
    a = rng.integers(0, 40, (30, 4)).astype(f32)
    a[:, 2:] += a[:, :2] + rng.integers(-2, 30, (30, 2)).astype(f32)            # some empty and some inverted boxes
    a[3, 1] = NAN
    b = a[rng.permutation(30)] + rng.integers(-3, 4, (30, 4)).astype(f32)
    m = iou_matrix(a, b)
    assert m.dtype == f32 and np.isnan(m[3]).all()
    for thres in (0.0, 0.3, 0.5):
        for j in range(30):
            assert np.array_equal(m[:, j].astype(np.float64) > thres, overlaps(a, b[j], thres, 'iou'))


def test_tie_is_broken_by_slot_then_row():
    from yolov6.utils.track import PlateTrackerNp
    trk = PlateTrackerNp(1, max_tracks=4, expand=0.0)
    outs, tids, _ = run_stream(trk, [[make_row(A), make_row(A)], [make_row(A), make_row(A)], [make_row(FAR), make_row(A)]], 4)
    assert list(tids[0]) == [0, 1, -1, -1]
    assert list(tids[1]) == [0, 1, -1, -1]                  # four pairs of IoU 1: (slot 0, row 0) first, then (slot 1, row 1)
    assert list(tids[2]) == [2, 0, -1, -1]                  # (slot 0, row 1) before (slot 1, row 1); row 0 starts track 2
    assert trk.stats['ties'] == 3 + 1 and list(trk.misses[0]) == [0, 1, 0, 0]


def test_pair_exactly_at_the_threshold_is_not_matched():
    from yolov6.utils.track import PlateTrackerNp
    for thres, want in ((0.5, [1]), (0.49, [0])):
        trk = PlateTrackerNp(1, max_tracks=4, match_thres=thres, expand=0.0)
        _, tids, _ = run_stream(trk, [[make_row((0, 0, 10, 10))], [make_row((0, 0, 10, 5))]], 1)     # IoU = 50 / 100
        assert list(tids[1]) == want


def test_expired_slot_is_reused_in_the_same_frame_and_capacity_drops():
    from yolov6.utils.track import PlateTrackerNp
    trk = PlateTrackerNp(1, max_tracks=1, max_age=0)
    outs, tids, ended = run_stream(trk, [[make_row(A)], [make_row(FAR, ids=(9,) * 8)], [make_row(FAR), make_row(A, conf=0.5)]], 2)
    assert list(tids[0]) == [0, -1] and list(tids[1]) == [1, -1]                # track 0 ends in frame 1, its slot holds track 1
    assert len(ended) == 1
    ri, rf = ended[0]
    assert list(ri) == [0, 0, 0, 1, 1, 2, 3, 4, 5, 6, 7, 8] and list(rf) == [1.0] * 8 + list(map(float, A))
    assert list(tids[2]) == [1, -1] and trk.dropped[0] == 1                     # no free slot: row 1 stays untracked ...
    assert np.array_equal(outs[2][1], make_row(A, conf=0.5))                    # ... and is copied unchanged
    assert trk.id[0, 0] == 1 and trk.hits[0, 0] == 2 and trk.next_id[0] == 2 and trk.frame[0] == 3


def test_new_thres_is_applied():
    from yolov6.utils.track import PlateTrackerNp
    trk = PlateTrackerNp(1, max_tracks=4, new_thres=0.5)
    _, tids, _ = run_stream(trk, [[make_row(A, conf=0.25), make_row(FAR, conf=0.5)]], 3)
    assert list(tids[0]) == [-1, 0, -1] and trk.dropped[0] == 0


def test_nan_and_out_of_range_values_cast_no_vote():
    from yolov6.utils.track import PlateTrackerNp
    trk = PlateTrackerNp(1, max_tracks=4, max_age=1, ncls=NCLS)
    first = make_row(A, ids=(5, 6, 7, 8, 9, 10, 11, 12), conf=(0.5, 0.5, 0.5, 0.0, 0.5, 0.5, 0.5, 0.5))
    second = make_row(A, ids=(31, -1, 3, 8, 9, 10, 11, 13), conf=(0.5, 0.5, NAN, 0.25, 0.5, 0.5, 0.5, 1.0))
    nanbox = make_row((NAN, 200, 360, 220))
    nanconf = make_row(FAR, conf=(0.9, NAN, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9))
    outs, tids, _ = run_stream(trk, [[first], [second, nanbox, nanconf], [make_row((300, 200, 360, 220))]], 3)
    # frame 0: head 3 has conf 0: no vote, total 0 -> share 0, id 0
    assert list(outs[0][0, 20:28]) == [5, 6, 7, 0, 9, 10, 11, 12] and list(outs[0][0, 12:20]) == [1, 1, 1, 0, 1, 1, 1, 1]
    # frame 1: id 31 of a head of 31 classes, id -1 and the NaN confidence cast nothing; head 7 is outvoted 1.0 : 0.5
    assert list(tids[1]) == [0, 1, -1]                                          # a NaN score starts nothing; a NaN box does
    assert list(outs[1][0, 20:28]) == [5, 6, 7, 8, 9, 10, 11, 13]
    assert list(outs[1][0, 12:20]) == [1, 1, 1, 1, 1, 1, 1, f32(1.0) / f32(1.5)]
    assert np.array_equal(outs[1][0, :12], second[:12])
    assert np.array_equal(outs[1][2], nanconf, equal_nan=True)
    assert np.isnan(outs[1][1, 0]) and list(outs[1][1, 20:28]) == [1, 2, 3, 4, 5, 6, 7, 8]
    # frame 2: the NaN box matches nothing, ever: a new track
    assert list(tids[2]) == [2, -1, -1]


def test_counts_outside_the_range_and_rows_past_128():
    from yolov6.utils.track import PlateTrackerNp
    trk = PlateTrackerNp(2, max_tracks=128)
    det = np.zeros((2, 130, 28), f32)
    for r in range(130):
        det[:, r] = make_row((100 * (r % 12), 40 * (r // 12), 100 * (r % 12) + 60, 40 * (r // 12) + 20))
    o, t, _, _, ec = trk.update(det, [-3, 1000])
    assert not o[0].any() and np.all(t[0] == -1) and trk.frame[0] == 1 and not trk.live(0).any()
    assert np.array_equal(t[1], np.concatenate([np.arange(128), [-1, -1]]))     # count above max_det: max_det rows; 128 take part
    assert np.array_equal(o[1][128:], det[1, 128:]) and trk.dropped[1] == 0 and ec.tolist() == [0, 0]
    assert np.array_equal(o[1][:128, :12], det[1, :128, :12]) and np.all(o[1][:128, 12:20] == 1)
    o, t, _, _, _ = trk.update(det[:, :7], [3, 5], stream_of=[-1, 1])
    assert np.array_equal(o[0, :3], det[0, :3]) and not o[0, 3:].any() and np.all(t[0] == -1) and trk.frame[0] == 1    # skipped
    assert t[1].tolist() == [0, 1, 2, 3, 4, -1, -1] and not o[1, 5:].any()


def test_interleaved_streams_are_independent():
    from yolov6.utils.track import PlateTrackerNp
    rows_per_frame, _, _ = plate_scene(frames=12)
    other = [[make_row((r[0] + 7, r[1], r[2] + 7, r[3]), r[20:28], r[12:20]) for r in rows[::-1]] for rows in rows_per_frame]
    both = PlateTrackerNp(3, max_tracks=8, max_age=1)
    det = np.zeros((24, 4, 28), f32)
    count = np.zeros(24, np.int32)
    det[0::2], count[0::2] = frames_of(rows_per_frame, 4)
    det[1::2], count[1::2] = frames_of(other, 4)
    o, t, ei, ef, ec = both.update(det, count, stream_of=[2, 0] * 12, flush=[1, 1, 1], max_ended=16)
    for s, rows in ((2, rows_per_frame), (0, other)):
        alone = PlateTrackerNp(1, max_tracks=8, max_age=1)
        d1, c1 = frames_of(rows, 4)
        o1, t1, ei1, ef1, ec1 = alone.update(d1, c1, stream_of=[0] * 12, flush=[1], max_ended=16)
        k = 0 if s == 2 else 1
        assert np.array_equal(o[k::2], o1) and np.array_equal(t[k::2], t1)
        assert np.array_equal(ei[s], ei1[0]) and np.array_equal(ef[s], ef1[0]) and ec[s] == ec1[0] > 0
    assert ec[1] == 0 and not ei[1].any() and both.frame.tolist() == [12, 0, 12]


def test_max_ended_overflow_and_flush_without_frames():
    from yolov6.utils.track import PlateTrackerNp
    trk = PlateTrackerNp(2, max_tracks=4)
    rows = [make_row((100 * k, 0, 100 * k + 60, 20), ids=(k,) * 8) for k in range(4)]
    det, count = frames_of([rows], 4)
    _, t, _, _, ec = trk.update(det, count, stream_of=[1])
    assert t[0].tolist() == [0, 1, 2, 3] and ec.tolist() == [0, 0]
    _, _, ei, ef, ec = trk.flush_all(max_ended=2)                               # zero frames; four tracks end, two are recorded
    assert ec.tolist() == [0, 4] and ei.shape == (2, 2, 12) and ei[1, :, 0].tolist() == [0, 1] and ei[1, 1, 4:].tolist() == [1] * 8
    assert ef[1, 1].tolist() == [1.0] * 8 + [100.0, 0.0, 160.0, 20.0] and not ei[0].any()
    assert not trk.live(1).any() and trk.next_id[1] == 4 and not trk.votes.any()
    assert trk.flush_all()[4].tolist() == [0, 0]
    trk.reset()
    assert trk.next_id.tolist() == [0, 0] and trk.frame.tolist() == [0, 0]


def test_plate_text():
    from yolov6.utils.track import plate_text
    assert plate_text([1, 0, 2, 2, 0, 1, 1, 2]) == '1 0 2 2 0 1 1 2'
    assert plate_text([1, 0, 2, 2, 0, 1, 1, 2], ['P', 'Q'], ['a', 'b'], ['x', 'y', 'z']) == 'Qazzxyyz'
    assert plate_text([2, 0, 2, 2, 0, 1, 1, 2], ['P', 'Q'], ['a', 'b'], ['x', 'y', 'z']) == '2 0 2 2 0 1 1 2'


# ---- random cases (shared with the GPU tests) ------------------------------------------------------------------------------------
def random_track_case(seed, n_streams=3, max_det=20, n_calls=6, max_B=8, n_obj=6, extent=600, ncls=NCLS, Bs=None):
    """A list of ``n_calls`` update calls (det, count, stream_of, flush) on ``n_streams`` streams: per stream up to ``n_obj``
    objects with integer boxes and integer velocities plus +-1 px jitter, births and deaths, rows missing, duplicate rows (equal
    IoUs), NaNs in boxes and confidences, ids with noise (also outside the head), counts below 0 and above max_det with
    arbitrary rows behind the count, skipped frames (-1), streams without frames in a call, and a flush of everything in the
    last call.  ``Bs``: the calls' frame counts (default: drawn from 1..max_B).

    These cases lie on an EXACT GRID: integer coordinates and velocities and confidences k / 8, so every fp32 operation of the
    tracker on them (expansion by 0 or 0.5, areas, sums of votes) is exact, and a kernel that fused a multiply-add, summed in
    another order or divided through a reciprocal would still produce these bits.  They test the rules, not the rounding;
    ``tests/offgrid.py`` has their off-grid twins (``offgrid_twin``) and the constructed cases on which one ulp decides."""
    rng = np.random.default_rng(seed)
    objs = [[] for _ in range(n_streams)]

    def new_obj():
        w, h = int(rng.integers(30, 90)), int(rng.integers(10, 30))
        return dict(x=int(rng.integers(0, extent)), y=int(rng.integers(0, extent)), w=w, h=h, vx=int(rng.integers(-8, 9)),
                    vy=int(rng.integers(-3, 4)), ids=[int(rng.integers(0, n)) for n in ncls])

    def frame_rows(s):
        live = objs[s]
        live[:] = [o for o in live if rng.random() > 0.06]
        for _ in range(n_obj - len(live)):                                      # births: most at once into an empty stream
            if rng.random() < (0.3 if live else 0.8):
                live.append(new_obj())
        rows = []
        for o in live:
            o['x'] += o['vx'] + int(rng.integers(-1, 2))
            o['y'] += o['vy'] + int(rng.integers(-1, 2))
            if rng.random() < 0.15:
                continue
            ids = [i if rng.random() < 0.8 else int(rng.integers(-2, n + 3)) for i, n in zip(o['ids'], ncls)]
            conf = (rng.integers(0, 9, 8) / 8.0).astype(f32)                    # 0 included
            row = make_row((o['x'], o['y'], o['x'] + o['w'], o['y'] + o['h']), ids, conf)
            if rng.random() < 0.03:
                row[int(rng.integers(0, 4))] = NAN
            if rng.random() < 0.03:
                row[12 + int(rng.integers(0, 8))] = NAN
            rows.append(row)
            if rng.random() < 0.12:
                rows.append(row.copy())                                         # a duplicate: equal IoUs with every slot
        return [rows[i] for i in rng.permutation(len(rows))]

    calls = []
    n_calls = n_calls if Bs is None else len(Bs)
    for c in range(n_calls):
        B = int(rng.integers(1, max_B + 1)) if Bs is None else int(Bs[c])
        active = [s for s in range(n_streams) if rng.random() < 0.7] or [int(rng.integers(0, n_streams))]
        stream_of = [int(rng.choice(active)) if rng.random() > 0.1 else -1 for _ in range(B)]
        det = (rng.integers(-4, 400, (B, max_det, 28)) / 4.0).astype(f32)       # whatever lies behind the count
        count = np.zeros(B, np.int32)
        for b, s in enumerate(stream_of):
            rows = frame_rows(s)[:max_det] if s >= 0 else [make_row(A)] * int(rng.integers(0, min(3, max_det) + 1))
            for r, row in enumerate(rows):
                det[b, r] = row
            u = rng.random()
            count[b] = len(rows) if u < 0.8 else (-2 if u < 0.85 else (max_det + 7 if u < 0.9 else min(len(rows) + 2, max_det)))
        last = c == n_calls - 1
        flush = [1 if last or rng.random() < 0.15 else 0 for _ in range(n_streams)]
        calls.append((det, count, stream_of, flush))
    return calls


def run_calls_np(calls, n_streams, max_ended, **kw):
    """(tracker, outputs per call) of ``PlateTrackerNp`` on a random case."""
    from yolov6.utils.track import PlateTrackerNp
    trk = PlateTrackerNp(n_streams, **kw)
    return trk, [trk.update(det, count, stream_of, flush, max_ended) for det, count, stream_of, flush in calls]


def test_random_cases_exercise_every_rule():
    tot = dict(pairs=0, ties=0, matched=0, ended=0, dropped=0, idle=0, overflow=0, untracked=0)
    for seed, kw in ((1, dict(max_tracks=4, max_age=0, expand=0.0)), (2, dict(max_tracks=16, max_age=3, expand=0.5)), (3, dict(max_tracks=1, max_age=3))):
        calls = random_track_case(seed)
        trk, outs = run_calls_np(calls, 3, 5, **kw)
        for k in trk.stats:
            tot[k] += trk.stats[k]
        tot['dropped'] += int(trk.dropped.sum())
        tot['idle'] += sum(1 for _, _, so, _ in calls for s in range(3) if s not in so)
        tot['overflow'] += sum(int((o[4] > 5).sum()) for o in outs)
        tot['untracked'] += sum(int(((o[1] == -1) & (np.arange(20) < np.clip(c[1], 0, 20)[:, None])).sum()) for o, c in zip(outs, calls))
        assert not trk.live(0).any() and not trk.live(1).any() and not trk.live(2).any()        # the last call flushes
        assert sum(int(o[4].sum()) for o in outs) == trk.stats['ended'] == int(trk.next_id.sum())
    assert all(v > 0 for v in tot.values()), tot                                # a case cannot pass by doing nothing


# ---- C ABI: everything is checked on the host before any launch -------------------------------------------------------------
def test_track_state_bytes_grows_with_both_arguments():
    from yolov6.hip import abi
    lib = abi.load()
    sb = lib.lp_track_state_bytes
    assert sb(1, 1) >= 4 * (8 * 64 + 8 + 14 + 5) and sb(2, 1) == 2 * sb(1, 1) and sb(1, 2) > sb(1, 1) and sb(3, 128) == 3 * sb(1, 128)
    assert sb(0, 4) == 0 and sb(1, 0) == 0 and sb(1, 129) == 0
    off = lib.lp_track_dropped_offset
    assert off(4, 0) < sb(1, 4) and off(4, 2) == off(4, 0) + 2 * sb(1, 4) and off(4, 0) % 4 == 0


def test_track_update_rejects_bad_arguments_before_launch():
    from yolov6.hip import abi
    lib = abi.load()
    v = lambda p: ctypes.c_void_p(p) if p else None   # noqa: E731

    def call(stream_of=(0, 1, -1), flush=(0, 1), n_streams=2, max_tracks=8, max_det=10, max_ended=4, B=None, params=True, state=0x1000,
             det=0x10000, count=0x2000, det_out=0x20000, tid=0x3000, ei=0x4000, ef=0x5000, ec=0x6000, **pk):
        p = abi.TrackParams(pk.get('match_thres', 0.3), pk.get('new_thres', 0.0), pk.get('expand', 0.5), pk.get('max_age', 5),
                            (ctypes.c_int * 8)(*pk.get('ncls', NCLS)))
        so = (ctypes.c_int * max(len(stream_of), 1))(*stream_of) if stream_of is not None else None
        fl = ctypes.cast((ctypes.c_ubyte * max(len(flush), 1))(*flush), ctypes.c_void_p) if flush is not None else None
        return lib.lp_track_update(v(state), n_streams, max_tracks, ctypes.byref(p) if params else None, v(det), v(count),
                                   len(stream_of or ()) if B is None else B, max_det, so, fl, v(det_out), v(tid), v(ei), v(ef), v(ec),
                                   max_ended, None)

    err = lambda: lib.lp_last_error()   # noqa: E731
    for k in ('state', 'det', 'count', 'det_out', 'tid', 'ei', 'ef', 'ec'):
        assert call(**{k: 0}) == LP_ERR_ARG and b'null' in err(), k
    assert call(params=False) == LP_ERR_ARG and call(stream_of=None, B=3) == LP_ERR_ARG and b'null' in err()
    assert call(state=0x1004) == LP_ERR_ARG and b'aligned' in err()
    assert call(n_streams=0) == LP_ERR_ARG and call(max_tracks=0) == LP_ERR_ARG and call(max_tracks=129) == LP_ERR_ARG and b'128' in err()
    assert call(B=-1) == LP_ERR_ARG and call(max_det=0) == LP_ERR_ARG and call(max_ended=-1) == LP_ERR_ARG
    for k, bad in (('match_thres', 1.5), ('match_thres', -0.1), ('match_thres', NAN), ('new_thres', NAN), ('new_thres', float('inf')),
                   ('expand', -1.0), ('expand', NAN), ('max_age', -1)):
        assert call(**{k: bad}) == LP_ERR_ARG and k.encode() in err(), (k, bad)
    assert call(ncls=(31, 24, 37, 0, 37, 37, 37, 37)) == LP_ERR_ARG and b'head 3' in err()
    assert call(ncls=(31, 24, 37, 37, 37, 37, 37, 65)) == LP_ERR_ARG and b'head 7' in err()
    assert call(stream_of=(0, 1, 2)) == LP_ERR_ARG and b'frame 2' in err()
    assert call(stream_of=(0, -2, 1)) == LP_ERR_ARG and b'frame 1' in err()
    assert call(det_out=0x10000) == LP_ERR_ARG and b'alias' in err()
    assert call(det_out=0x10000 + 3 * 10 * 28 * 4 - 4) == LP_ERR_ARG and b'alias' in err()


# ---- tools/infer.py --track on the CPU path ----------------------------------------------------------------------------------
def _moving_frames(n, h=128, w=160, seed=4):
    """Frames of one bright patch drifting over a fixed random background (something that changes slowly from frame to frame)."""
    rng = np.random.default_rng(seed)
    back = rng.integers(0, 255, (h, w, 3), dtype=np.uint8)
    patch = rng.integers(0, 255, (24, 64, 3), dtype=np.uint8)
    out = []
    for k in range(n):
        f = back.copy()
        f[40:64, 10 + 4 * k:74 + 4 * k] = patch
        out.append(f)
    return out


def track_by_hand(dets, max_det, **kw):
    """``PlateTrackerNp`` over the untracked per-frame detections of one stream, one update per frame, then the flush:
    (voted rows per frame, tid per frame, ended records)."""
    from yolov6.utils.track import PlateTrackerNp
    trk = PlateTrackerNp(1, **kw)
    outs, tids, ended = [], [], []
    for d in dets:
        pad = np.zeros((1, max_det, 28), f32)
        pad[0, :len(d)] = d
        o, t, ei, ef, ec = trk.update(pad, [len(d)], max_ended=2 * trk.max_tracks)
        outs.append(o[0, :len(d)])
        tids.append(t[0, :len(d)])
        ended += [(ei[0, k], ef[0, k]) for k in range(int(ec[0]))]
    _, _, ei, ef, ec = trk.flush_all()
    ended += [(ei[0, k], ef[0, k]) for k in range(int(ec[0]))]
    return outs, tids, ended


def plate_lines(ended):
    from yolov6.utils.track import plate_text
    return ['%d %d %d %d %s %s' % (ri[0], ri[1], ri[2], ri[3], plate_text(ri[4:12]), ' '.join('%g' % v for v in rf[:8])) for ri, rf in ended]


def test_infer_track_cpu(tmp_path, monkeypatch):
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
    for k, f in enumerate(_moving_frames(6)):
        Image.fromarray(f).save(str(img_dir / ('f%02d.png' % k)))
    kw = dict(weights=str(ckpt), source=str(img_dir), yaml=None, img_size=[128, 160], conf_thres=0.06, iou_thres=0.45, max_det=20,
              device='cpu', not_save_img=True, save_txt=True)
    plain = infer.run(save_dir=str(tmp_path / 'o1'), **kw)
    again = infer.run(save_dir=str(tmp_path / 'o2'), **kw)
    voted = infer.run(save_dir=str(tmp_path / 'o3'), track=True, track_max_age=2, track_iou=0.25, track_expand=0.25, **kw)
    assert len(plain) == len(again) == len(voted) == 6 and sum(len(d) for d in plain) >= 6
    for a, b, c in zip(plain, again, voted):
        assert torch.equal(a, b) and torch.equal(a[:, :12], c[:, :12])          # untracked runs are what they were; same geometry
    assert not (tmp_path / 'o1' / 'tracks.txt').exists() and not (tmp_path / 'o1' / 'plates.txt').exists()
    for k in range(6):
        t1, t2 = (tmp_path / o / 'imgs' / ('f%02d.txt' % k) for o in ('o1', 'o2'))
        assert t1.exists() == t2.exists() and (not t1.exists() or t1.read_bytes() == t2.read_bytes())
    outs, tids, ended = track_by_hand([d.numpy() for d in plain], 20, max_tracks=64, match_thres=0.25, new_thres=0.0, expand=0.25,
                                      max_age=2, ncls=m)
    for c, o in zip(voted, outs):
        assert np.array_equal(c.numpy(), o)
    files = sorted(os.listdir(str(img_dir)))
    want = ['%s %d %d' % (str(img_dir / files[k]), r, t) for k in range(6) for r, t in enumerate(tids[k].tolist())]
    assert (tmp_path / 'o3' / 'tracks.txt').read_text().splitlines() == want
    assert (tmp_path / 'o3' / 'plates.txt').read_text().splitlines() == plate_lines(ended)
    assert len(ended) >= 1 and max(int(ri[3]) for ri, _ in ended) >= 2          # something was followed over frames
