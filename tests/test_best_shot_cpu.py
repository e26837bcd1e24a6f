"""The best shot of every plate track on the CPU: the checks of the specification itself (yolov6/utils/best_shot.py:
crop_sharpness_np, BestShotNp), the per-row slot of PlateTrackerNp, the argument checks of lp_crop_sharpness /
lp_best_shot_update (no device needed) and ``tools/infer.py --track --best-shots`` on the CPU path.  ``shot_case`` and
``shots_by_hand`` are exported for tests/test_best_shot_gpu.py."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
import test_track_cpu as C

LP_ERR_ARG = -1
f32 = np.float32
CHECKER_64x192 = 12255912000        # 62 * 190 interior pixels, every one with L = +-4 * 255: 11780 * 1020^2


def checkerboard(h=64, w=192):
    i, j = np.indices((h, w))
    return np.repeat((((i + j) & 1) * 255).astype(np.uint8)[..., None], 3, -1)


# ---- sharpness --------------------------------------------------------------------------------------------------------------
def test_crop_sharpness_hand_values():
    from yolov6.utils.best_shot import crop_sharpness_np
    one = np.zeros((3, 3, 3), np.uint8)
    one[1, 1] = 255                                         # g = 255 at the only interior pixel, its neighbours 0: L = 1020
    assert crop_sharpness_np(one) == 1020 * 1020 and crop_sharpness_np(one).dtype == np.uint64
    one[1, 1] = (10, 20, 30)                                # g = (290 + 3000 + 2310 + 128) >> 8 = 22, L = 88
    assert crop_sharpness_np(one) == 88 * 88
    edge = np.zeros((3, 3, 3), np.uint8)
    edge[0, 1] = 255                                        # a neighbour of the interior pixel: L = -255
    assert crop_sharpness_np(edge) == 255 * 255
    edge[0, 0] = edge[2, 2] = 200                           # the corners are in no stencil
    assert crop_sharpness_np(edge) == 255 * 255
    assert crop_sharpness_np(np.full((64, 192, 3), 93, np.uint8)) == 0
    cb = checkerboard()
    assert int(crop_sharpness_np(cb)) == CHECKER_64x192 == 62 * 190 * 1020 * 1020 > 2 ** 32
    # status: 0 and 3 give 0; a side shorter than 3 gives 0
    both = np.stack([cb, cb, cb, cb])
    assert crop_sharpness_np(both, [0, 1, 2, 3]).tolist() == [0, CHECKER_64x192, CHECKER_64x192, 0]
    assert crop_sharpness_np(np.full((2, 2, 9, 3), 255, np.uint8)).tolist() == [0, 0]
    assert crop_sharpness_np(checkerboard(9, 2)) == 0 and crop_sharpness_np(checkerboard(3, 4)) == 2 * 1020 * 1020


# ---- the scene by construction ---------------------------------------------------------------------------------------------
def scene_shots():
    """``plate_scene`` with synthetic crops: crop (f, r) is filled with the bytes (f + 1, r + 1, track + 1), and its sharpness
    and status are chosen here.  Returns (rows_per_frame, crops [F,3,5,7,3], status [F,3], sharp [F,3], want) with
    want[track] = the frame whose crop must come out (None: no shot)."""
    rows_per_frame, truth, _ = C.plate_scene()
    F = len(rows_per_frame)
    crops = np.zeros((F, 3, 5, 7, 3), np.uint8)
    status = np.zeros((F, 3), np.int32)
    sharp = np.zeros((F, 3), np.uint64)
    frames_of_track = {}
    for f, tr in enumerate(truth):
        for r, (_, t, _) in enumerate(tr):
            crops[f, r] = (f + 1, r + 1, t + 1)
            status[f, r] = 1
            sharp[f, r] = 100 + (f * 7) % 50
            frames_of_track.setdefault(t, []).append((f, r))
    fr = {t: [f for f, _ in v] for t, v in frames_of_track.items()}
    row = {t: dict(v) for t, v in frames_of_track.items()}
    want = {}
    # track 0: the sharpest frame lies in the middle; a box crop (status 2) with far more energy comes later and must lose
    want[0] = fr[0][len(fr[0]) // 2]
    sharp[want[0], row[0][want[0]]] = 5000
    box = fr[0][-3]
    status[box, row[0][box]], sharp[box, row[0][box]] = 2, 900000
    # track 1: two frames share the largest value: the earlier one stays
    a, b = fr[1][4], fr[1][9]
    sharp[a, row[1][a]] = sharp[b, row[1][b]] = 7000
    want[1] = a
    # track 2 (plate 2 before its long gap): its last frame is the sharpest -- the case "the last frame" would also get right
    want[2] = fr[2][-1]
    sharp[want[2], row[2][want[2]]] = 6000
    # track 3 (plate 2 after the gap): no crop is ever usable
    for f in fr[3]:
        status[f, row[3][f]] = 3
    want[3] = None
    return rows_per_frame, crops, status, sharp, want


@pytest.mark.parametrize('per_frame', [True, False], ids=['one-call-per-frame', 'one-call'])
def test_scene_every_record_gets_its_sharpest_crop(per_frame):
    from yolov6.utils.best_shot import BestShotNp
    from yolov6.utils.track import PlateTrackerNp
    rows_per_frame, crops, status, sharp, want = scene_shots()
    det, count = C.frames_of(rows_per_frame, 5)
    F = len(det)
    trk = PlateTrackerNp(1, max_tracks=8, match_thres=0.3, expand=0.5, max_age=C.SCENE_MAX_AGE)
    gal = BestShotNp(1, 8, (5, 7))
    got = {}
    for lo, hi in ([(f, f + 1) for f in range(F)] if per_frame else [(0, F)]):
        flush = [int(hi == F)]
        _, tid, ei, _, ec = trk.update(det[lo:hi], count[lo:hi], stream_of=[0] * (hi - lo), flush=flush)
        sc, si, sq, sd = gal.update(det[lo:hi], count[lo:hi], tid, trk.last_slot, crops[lo:hi], status[lo:hi], sharp[lo:hi],
                                    [0] * (hi - lo), ei, ec)
        for k in range(int(ec[0])):
            got[int(ei[0, k, 0])] = (si[0, k].copy(), int(sq[0, k]), sc[0, k].copy(), sd[0, k].copy())
    assert sorted(got) == [0, 1, 2, 3]
    for t, f in want.items():
        si, sq, sc, sd = got[t]
        if f is None:
            assert si.tolist() == [0, 0, 0, 0] and sq == 0 and not sd.any() and not sc.any()
            continue
        r = int(si[1])
        assert si.tolist() == [f, r, 1, 1] and sq == int(sharp[f, r]), (t, si, sq)
        assert np.array_equal(sc, crops[f, r]) and sc[0, 0].tolist() == [f + 1, r + 1, t + 1]
        assert np.array_equal(sd, det[f, r])                # the row as given, with its per-frame confidences
    assert gal.stats['replaced'] > 0 and gal.stats['ties'] > 0 and gal.stats['without_shot'] == 1 and gal.stats['with_shot'] == 3
    assert not gal.idp1.any()                               # everything ended: the gallery is empty again


def test_min_score_and_rows_past_max_crops_are_not_eligible():
    from yolov6.utils.best_shot import BestShotNp
    from yolov6.utils.track import PlateTrackerNp
    rows = [[C.make_row(C.A, conf=0.25), C.make_row(C.FAR, conf=0.5)], [C.make_row(C.A, conf=0.75), C.make_row(C.FAR, conf=0.5)]]
    det, count = C.frames_of(rows, 3)
    crops = np.arange(2 * 2 * 3 * 4 * 3, dtype=np.uint8).reshape(2, 2, 3, 4, 3)
    status, sharp = np.ones((2, 2), np.int32), np.array([[9, 9], [5, 5]], np.uint64)
    for min_score, max_crops, want in ((0.5, 2, {0: (1, 0), 1: (0, 1)}), (0.0, 1, {0: (0, 0), 1: None}), (float('nan'), 2, None)):
        if want is None:
            with pytest.raises(ValueError):
                BestShotNp(1, 4, (3, 4), min_score)
            continue
        trk, gal = PlateTrackerNp(1, max_tracks=4), BestShotNp(1, 4, (3, 4), min_score)
        _, tid, ei, _, ec = trk.update(det, count, stream_of=[0, 0], flush=[1])
        sc, si, sq, sd = gal.update(det, count, tid, trk.last_slot, crops[:, :max_crops], status[:, :max_crops], sharp[:, :max_crops],
                                    [0, 0], ei, ec)
        assert ec[0] == 2
        for k in range(2):
            w = want[int(ei[0, k, 0])]
            if w is None:
                assert si[0, k].tolist() == [0, 0, 0, 0]
            else:
                assert si[0, k].tolist() == [w[0], w[1], 1, 1] and np.array_equal(sc[0, k], crops[w[0], w[1]])


# ---- the per-row slot of the tracker ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed, kw', [(1, dict(max_tracks=4, max_age=0, expand=0.0)), (2, dict(max_tracks=16, max_age=3, expand=0.5)),
                                      (3, dict(max_tracks=1, max_age=3))], ids=['t4', 't16', 't1'])
def test_last_slot_of_the_numpy_tracker(seed, kw):
    from yolov6.utils.track import PlateTrackerNp
    calls = C.random_track_case(seed)
    trk = PlateTrackerNp(3, **kw)
    holder = {}                                             # (stream, slot) -> id
    ended = set()
    changes = 0
    for det, count, stream_of, flush in calls:
        _, tid, ei, _, ec = trk.update(det, count, stream_of, flush, max_ended=200)
        slot = trk.last_slot
        assert slot.shape == tid.shape and slot.dtype == np.int32
        assert np.array_equal(slot == -1, tid == -1) and slot.max(initial=-1) < trk.max_tracks
        ended |= {(s, int(ei[s, k, 0])) for s in range(3) for k in range(int(ec[s]))}      # (200 records: nothing is cut off)
        for b, s in enumerate(stream_of):
            live = slot[b][slot[b] >= 0]
            assert len(set(live.tolist())) == len(live)     # distinct within a frame
            for r in np.nonzero(slot[b] >= 0)[0]:
                key, t = (s, int(slot[b, r])), int(tid[b, r])
                if key in holder and holder[key] != t:
                    assert (s, holder[key]) in ended        # a slot changes hands only after its track has ended
                    changes += 1
                holder[key] = t
    assert changes > 0 and len(holder) > 0


# ---- random cases (shared with the GPU tests) --------------------------------------------------------------------------------
def shot_case(seed, n_streams, max_tracks, max_det, Bs, crop_hw, max_crops, max_ended, n_obj=6, extent=400, max_age=3, expand=0.5,
              min_score=0.3, mid_flush=None, sharp_values=(0, 3, 3, 8, 2 ** 33 + 5)):
    """A multi-call sequence for lp_best_shot_update: ``random_track_case`` through PlateTrackerNp (tid, slot, ended records) with
    random crops, a status drawn from 0..3 (0 beyond the counted rows, as the crop kernel leaves it) and a sharpness drawn from a
    small set so that ties occur.  ``mid_flush``: the index of a call that flushes every stream.  Returns (gallery, calls) with
    calls[k] = (inputs dict, expected outputs of BestShotNp on shot_crops poisoned with 0xAB)."""
    from yolov6.utils.best_shot import BestShotNp
    from yolov6.utils.track import PlateTrackerNp
    rng = np.random.default_rng(1000 + seed)
    raw = C.random_track_case(seed, n_streams=n_streams, max_det=max_det, n_obj=n_obj, extent=extent, Bs=Bs)
    trk = PlateTrackerNp(n_streams, max_tracks=max_tracks, match_thres=0.3, new_thres=0.2, expand=expand, max_age=max_age)
    gal = BestShotNp(n_streams, max_tracks, crop_hw, min_score)
    calls = []
    for k, (det, count, stream_of, flush) in enumerate(raw):
        if mid_flush == k:
            flush = [1] * n_streams
        B = len(det)
        _, tid, ei, _, ec = trk.update(det, count, stream_of, flush, max_ended)
        crops = rng.integers(0, 256, (B, max_crops) + tuple(crop_hw) + (3,), dtype=np.uint8)
        status = rng.integers(0, 4, (B, max_crops)).astype(np.int32)
        status[np.arange(max_crops)[None, :] >= np.clip(count, 0, max_det)[:, None]] = 0
        sharp = rng.choice(np.array(sharp_values, np.uint64), (B, max_crops))
        inp = dict(det=det, count=count, tid=tid, slot=trk.last_slot.copy(), crops=crops, status=status, sharp=sharp,
                   stream_of=list(stream_of), ended_i=ei, ended_count=ec)
        poison = np.full((n_streams, max_ended) + tuple(crop_hw) + (3,), 0xAB, np.uint8)
        want = gal.update(det, count, tid, inp['slot'], crops, status, sharp, stream_of, ei, ec, shot_crops=poison)
        calls.append((inp, want))
    return gal, calls


# (seed, n_streams, max_tracks, max_det, frames per call, crop_hw, max_crops, max_ended, keywords): what each is there for is
# asserted from the gallery's counters by ``check_shot_case``; the seeds were chosen on the CPU so that the asserts hold
SHOT_CASES = [
    (5, 1, 1, 5, (1, 3, 2, 4, 1, 2), (5, 7), 5, 6, dict(n_obj=4, extent=300, max_age=0, expand=0.0)),        # a slot reused inside a call
    (1, 3, 4, 5, (4, 1, 8, 3, 6, 2, 5), (5, 7), 5, 6, dict(mid_flush=3)),
    (1, 9, 16, 20, (70, 3, 66, 1, 9, 65), (5, 7), 20, 6, dict(n_obj=8, extent=600, max_age=0)),               # crosses the 64-frame split
    (4, 3, 4, 20, (8, 2, 5, 7, 1, 6, 3, 4), (64, 192), 3, 2, dict(n_obj=8, extent=500, expand=0.0)),          # max_crops < max_det, truncation
]
SHOT_IDS = ['s1-t1-reuse', 's3-t4-midflush', 's9-t16-split', 's3-t4-crops3-ended2']


def check_shot_case(case, gal, calls):
    seed, S, T, max_det, Bs, crop_hw, max_crops, max_ended, kw = case
    st = gal.stats
    assert st['taken'] > 0 and st['replaced'] > 0 and st['ties'] > 0 and st['with_shot'] > 0 and st['without_shot'] > 0, st
    assert any(-1 in inp['stream_of'] for inp, _ in calls)
    if T == 1 or kw.get('max_age') == 0:
        assert st['reused'] > 0, st                         # a slot changed hands inside a call: retired by reuse
    if max_ended == 2:
        assert st['truncated'] > 0 and any(int(inp['ended_count'].max()) > max_ended for inp, _ in calls), st
    if max_crops < max_det:
        assert any(int(np.clip(inp['count'], 0, max_det).max()) > max_crops for inp, _ in calls)
    if max(Bs) > 64:
        so = calls[0][0]['stream_of']
        assert any(s in so[:64] and s in so[64:] for s in range(S))
    # records without a shot keep the poison, records with one do not (a random crop is not all 0xAB)
    for _, (sc, si, _, _) in calls:
        assert np.all(sc[si[..., 3] == 0] == 0xAB) and all((c != 0xAB).any() for c in sc[si[..., 3] == 1])


@pytest.mark.parametrize('case', SHOT_CASES, ids=SHOT_IDS)
def test_random_shot_cases_exercise_every_rule(case):
    seed, S, T, max_det, Bs, crop_hw, max_crops, max_ended, kw = case
    gal, calls = shot_case(seed, S, T, max_det, Bs, crop_hw, max_crops, max_ended, **kw)
    check_shot_case(case, gal, calls)
    # the valid flag is set exactly for the records whose shot_q / shot_det were written from an entry with a shot
    for inp, (sc, si, sq, sd) in calls:
        assert set(np.unique(si[..., 3]).tolist()) <= {0, 1}
        assert not sq[si[..., 3] == 0].any() and not sd[si[..., 3] == 0].any()
        assert np.isin(si[..., 2][si[..., 3] == 1], (1, 2)).all()


def test_reset_empties_one_stream():
    from yolov6.utils.best_shot import BestShotNp
    from yolov6.utils.track import PlateTrackerNp
    rows_per_frame, crops, status, sharp, _ = scene_shots()
    det, count = C.frames_of(rows_per_frame[:4], 5)
    trk, gal = PlateTrackerNp(3, max_tracks=8), BestShotNp(3, 8, (5, 7))
    for s in range(3):                                      # the same four frames into every stream, nothing ends
        _, tid, ei, _, ec = trk.update(det, count, stream_of=[s] * 4)
        gal.update(det, count, tid, trk.last_slot, crops[:4], status[:4], sharp[:4], [s] * 4, ei, ec)
    assert gal.frame.tolist() == [4, 4, 4] and (gal.idp1 != 0).sum(1).tolist() == [3, 3, 3] and gal.has.sum() == 9
    keep = gal.idp1[1].copy()
    gal.reset([0, 2])
    assert not gal.idp1[0].any() and not gal.idp1[2].any() and gal.frame.tolist() == [0, 4, 0] and np.array_equal(gal.idp1[1], keep)
    assert not gal.crop[0].any() and gal.crop[1].any()
    gal.reset()
    assert not gal.idp1.any() and not gal.crop.any() and not gal.frame.any() and not gal.has.any()


# ---- C ABI: everything is checked on the host before any launch -------------------------------------------------------------
def test_best_shot_state_bytes():
    from yolov6.hip import abi
    sb = abi.load().lp_best_shot_state_bytes
    one = sb(1, 1, 64, 192)
    assert one >= 4 + 8 + 8 + 12 + 28 * 4 + 64 * 192 * 3 and one % 16 == 0
    assert sb(3, 1, 64, 192) == 3 * one and sb(1, 2, 64, 192) > one and sb(1, 7, 5, 7) % 16 == 0
    assert sb(1, 2, 5, 7) - sb(1, 1, 5, 7) >= 5 * 7 * 3 and (sb(1, 2, 5, 7) - sb(1, 1, 5, 7)) % 16 == 0    # every entry's crop stays aligned
    assert sb(0, 1, 5, 7) == 0 and sb(1, 0, 5, 7) == 0 and sb(1, 129, 5, 7) == 0 and sb(1, 1, 0, 7) == 0 and sb(1, 1, 5, 1025) == 0


def test_shot_entry_points_reject_bad_arguments_before_launch():
    from yolov6.hip import abi
    lib = abi.load()
    v = lambda p: ctypes.c_void_p(p) if p else None   # noqa: E731
    err = lambda: lib.lp_last_error()   # noqa: E731

    def sharp(crops=0x10000, status=0x2000, n=4, h=5, w=7, out=0x3000):
        return lib.lp_crop_sharpness(v(crops), v(status), n, h, w, v(out), None)

    for k in ('crops', 'status', 'out'):
        assert sharp(**{k: 0}) == LP_ERR_ARG and b'null' in err(), k
    assert sharp(n=-1) == LP_ERR_ARG and sharp(h=0) == LP_ERR_ARG and sharp(w=1025) == LP_ERR_ARG and b'1024' in err()
    assert sharp(out=0x3004) == LP_ERR_ARG and b'aligned' in err()
    assert sharp(n=0, crops=0, status=0, out=0) == 0                            # nothing to do

    def call(stream_of=(0, 1, -1), n_streams=2, max_tracks=8, h=5, w=7, max_det=10, max_crops=4, max_ended=4, B=None, state=0x1000,
             det=0x10000, count=0x2000, tid=0x3000, slot=0x4000, crops=0x20000, status=0x5000, sharp=0x6000, ei=0x7000, ec=0x8000,
             min_score=0.0, sc=0x30000, si=0x9000, sq=0xa000, sd=0xb000):
        so = (ctypes.c_int * max(len(stream_of), 1))(*stream_of) if stream_of is not None else None
        return lib.lp_best_shot_update(v(state), n_streams, max_tracks, h, w, v(det), v(count), len(stream_of or ()) if B is None else B,
                                       max_det, v(tid), v(slot), v(crops), v(status), v(sharp), max_crops, so, v(ei), v(ec), max_ended,
                                       min_score, v(sc), v(si), v(sq), v(sd), None)

    for k in ('state', 'det', 'count', 'tid', 'slot', 'crops', 'status', 'sharp', 'ei', 'ec', 'sc', 'si', 'sq', 'sd'):
        assert call(**{k: 0}) == LP_ERR_ARG and b'null' in err(), k
    assert call(stream_of=None, B=3) == LP_ERR_ARG and b'null' in err()
    assert call(state=0x1004) == LP_ERR_ARG and b'aligned' in err()
    assert call(sharp=0x6004) == LP_ERR_ARG and call(sq=0xa004) == LP_ERR_ARG and b'aligned' in err()
    assert call(n_streams=0) == LP_ERR_ARG and call(max_tracks=0) == LP_ERR_ARG and call(max_tracks=129) == LP_ERR_ARG and b'128' in err()
    assert call(h=0) == LP_ERR_ARG and call(w=1025) == LP_ERR_ARG
    assert call(B=-1) == LP_ERR_ARG and call(max_det=0) == LP_ERR_ARG and call(max_ended=-1) == LP_ERR_ARG and call(max_crops=-1) == LP_ERR_ARG
    assert call(min_score=float('nan')) == LP_ERR_ARG and call(min_score=float('inf')) == LP_ERR_ARG and b'min_score' in err()
    assert call(stream_of=(0, 1, 2)) == LP_ERR_ARG and b'frame 2' in err()
    assert call(stream_of=(0, -2, 1)) == LP_ERR_ARG and b'frame 1' in err()


def test_track_update_slots_checks_like_track_update():
    from yolov6.hip import abi
    lib = abi.load()
    p = abi.TrackParams(0.3, 0.0, 0.5, 5, (ctypes.c_int * 8)(*C.NCLS))
    so = (ctypes.c_int * 2)(0, 5)
    v = ctypes.c_void_p
    rc = lib.lp_track_update_slots(v(0x1000), 2, 8, ctypes.byref(p), v(0x10000), v(0x2000), 2, 10, so, None, v(0x20000), v(0x3000), None,
                                   v(0x4000), v(0x5000), v(0x6000), 4, None)
    assert rc == LP_ERR_ARG and b'frame 1' in lib.lp_last_error()


# ---- tools/infer.py --track --best-shots on the CPU path ---------------------------------------------------------------------
def shots_by_hand(frames, dets, max_det, crop_hw, max_crops=16, **kw):
    """PlateTrackerNp + BestShotNp over the untracked per-frame detections of one stream, one update per frame, then the flush:
    (ended records, shots) with shots[k] = (shot_i [4], sharpness, crop or None) for record k."""
    from yolov6.utils.best_shot import BestShotNp
    from yolov6.utils.track import PlateTrackerNp
    trk = PlateTrackerNp(1, **kw)
    gal = BestShotNp(1, trk.max_tracks, crop_hw)
    ended, shots = [], []

    def collect(ei, ef, ec, out):
        sc, si, sq, _ = out
        for k in range(int(ec[0])):
            ended.append((ei[0, k], ef[0, k]))
            shots.append((si[0, k], int(sq[0, k]), sc[0, k].copy() if si[0, k, 3] else None))

    for frame, d in zip(frames, dets):
        pad = np.zeros((1, max_det, 28), f32)
        pad[0, :len(d)] = d
        _, tid, ei, ef, ec = trk.update(pad, [len(d)], max_ended=2 * trk.max_tracks)
        collect(ei, ef, ec, gal.update_from_frames([frame], pad, [len(d)], tid, trk.last_slot, [0], ei, ec, max_crops))
    _, tid, ei, ef, ec = trk.flush_all()
    collect(ei, ef, ec, gal.update_from_frames([], np.zeros((0, 1, 28), f32), [], tid, trk.last_slot, [], ei, ec, max_crops))
    return ended, shots


def check_shot_files(out_dir, ended, shots):
    """shots.txt is line-parallel to plates.txt and the PNGs decode to the expected crops (RGB)."""
    from PIL import Image
    assert (out_dir / 'plates.txt').read_text().splitlines() == C.plate_lines(ended)
    lines = (out_dir / 'shots.txt').read_text().splitlines()
    assert len(lines) == len(ended) == len(shots)
    n_png = 0
    for k, (line, (ri, _), (si, q, crop)) in enumerate(zip(lines, ended, shots)):
        name = 'shots/%d_%d.png' % (k, ri[0]) if crop is not None else '-'
        assert line == '%d %d %d %d %d %s' % (ri[0], si[0], si[1], si[2], q, name), k
        if crop is not None:
            assert np.array_equal(np.asarray(Image.open(str(out_dir / name))), crop[:, :, ::-1])
            n_png += 1
    assert sorted(os.listdir(str(out_dir / 'shots'))) == sorted('%d_%d.png' % (k, e[0][0]) for k, (e, s) in enumerate(zip(ended, shots))
                                                                if s[2] is not None)
    return n_png


def test_infer_best_shots_cpu(tmp_path, monkeypatch):
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
    frames = C._moving_frames(6)
    for k, f in enumerate(frames):
        Image.fromarray(f).save(str(img_dir / ('f%02d.png' % k)))
    kw = dict(weights=str(ckpt), source=str(img_dir), yaml=None, img_size=[128, 160], conf_thres=0.06, iou_thres=0.45, max_det=20,
              device='cpu', not_save_img=True, save_txt=True)
    plain = infer.run(save_dir=str(tmp_path / 'o1'), **kw)
    tkw = dict(track=True, track_max_age=2, track_iou=0.25, track_expand=0.25)
    voted = infer.run(save_dir=str(tmp_path / 'o2'), **tkw, **kw)
    shot = infer.run(save_dir=str(tmp_path / 'o3'), best_shots=True, crop_size=(16, 48), **tkw, **kw)
    assert all(torch.equal(a, b) for a, b in zip(voted, shot))                  # the flag changes nothing else
    assert (tmp_path / 'o2' / 'plates.txt').read_text() == (tmp_path / 'o3' / 'plates.txt').read_text()
    assert (tmp_path / 'o2' / 'tracks.txt').read_text() == (tmp_path / 'o3' / 'tracks.txt').read_text()
    assert not (tmp_path / 'o2' / 'shots.txt').exists() and not (tmp_path / 'o2' / 'shots').exists()
    bgr = [f[:, :, ::-1] for f in frames]                                       # the PNGs are RGB, the Inferer's frames BGR
    ended, shots = shots_by_hand(bgr, [d.numpy() for d in plain], 20, (16, 48), max_tracks=64, match_thres=0.25, new_thres=0.0,
                                 expand=0.25, max_age=2, ncls=m)
    assert check_shot_files(tmp_path / 'o3', ended, shots) >= 1
    with pytest.raises(ValueError):
        infer.run(save_dir=str(tmp_path / 'o4'), best_shots=True, **kw)           # needs --track
