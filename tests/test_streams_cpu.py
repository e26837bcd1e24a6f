"""The host-side pieces the per-stream entry points share (yolo-lp_amd/csrc/lp_streams.h: the stream-to-workgroup planner of
lp_track_update_hold, lp_best_shot_update and lp_lookback_update, their argument rules, the threshold rounding): the stand-alone
program tests/host_streams.cpp is built with the host compiler and run, and the calls that reach the planner's two rarer
branches go through the three numpy specifications (``untracked_launch_calls`` is exported for the GPU tests)."""
import os
import shutil
import subprocess

import numpy as np

from conftest import REPO
import test_track_cpu as C

f32 = np.float32


def test_host_program_planner_rules_and_thresholds(tmp_path):
    cxx = os.environ.get('CXX') or next((c for c in ('c++', 'g++', 'clang++') if shutil.which(c)), None)
    assert cxx, 'no host C++ compiler (c++, g++, clang++ or $CXX)'
    exe = str(tmp_path / 'host_streams')
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-o', exe, os.path.join(REPO, 'tests', 'host_streams.cpp')], check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0 and run.stdout.strip() == 'all checks passed', run.stdout


# ---- a launch of untracked frames only, and a flushed stream without a frame ---------------------------------------------------
UL = dict(n_streams=2, max_tracks=4, max_det=4, max_age=1)


def untracked_launch_calls():
    """Two calls (det, count, stream_of, flush) on ``UL``: 66 frames of which the first 64, the whole first launch, are untracked
    and the last two start a track in streams 1 and 0; then 3 untracked frames with a flush of stream 0, which has no frame in
    the call."""
    rows = [[C.make_row(C.A, conf=0.5)] * (b % 3) for b in range(64)] + [[C.make_row(C.A)], [C.make_row(C.FAR, ids=(9,) * 8)]]
    det, count = C.frames_of(rows, UL['max_det'])
    det2, count2 = C.frames_of([[C.make_row(C.FAR)], [], [C.make_row(C.A), C.make_row(C.FAR)]], UL['max_det'])
    return [(det, count, [-1] * 64 + [1, 0], [0, 0]), (det2, count2, [-1, -1, -1], [1, 0])]


def track_state_words(trk):
    """The state of a ``PlateTrackerNp`` as int32 [n_streams, words] in the layout of lp_track.hip: 16 header words (frame, next id,
    dropped), then per slot 544: id, first, last, hits, misses at 0..4, box at 8, corners at 12, velocity at 20, totals at 24, votes
    at 32."""
    S, T = trk.n_streams, trk.max_tracks
    out = np.zeros((S, 16 + T * 544), np.int32)
    out[:, 0], out[:, 1], out[:, 2] = trk.frame, trk.next_id, trk.dropped
    slots = out[:, 16:].reshape(S, T, 544)
    for k, name in enumerate(('id', 'first', 'last', 'hits', 'misses')):
        slots[:, :, k] = getattr(trk, name)
    for at, name in ((8, 'box'), (12, 'cor'), (20, 'vel'), (24, 'total'), (32, 'votes')):
        words = getattr(trk, name).reshape(S, T, -1).view(np.int32)
        slots[:, :, at:at + words.shape[2]] = words
    return out


def untracked_launch_shots(crop_hw=(5, 7), max_ended=4):
    """``untracked_launch_calls`` through PlateTrackerNp and BestShotNp with random crops, every row a candidate: (gallery,
    [(inputs, expected outputs on shot_crops poisoned with 0xAB)]) as ``shot_case`` of tests/test_best_shot_cpu.py."""
    from yolov6.utils.best_shot import BestShotNp
    from yolov6.utils.track import PlateTrackerNp
    rng = np.random.default_rng(66)
    S, T, max_det = UL['n_streams'], UL['max_tracks'], UL['max_det']
    trk, gal = PlateTrackerNp(S, max_tracks=T, max_age=UL['max_age']), BestShotNp(S, T, crop_hw, 0.0)
    calls = []
    for det, count, stream_of, flush in untracked_launch_calls():
        B = len(det)
        _, tid, ei, _, ec = trk.update(det, count, stream_of, flush, max_ended)
        crops = rng.integers(0, 256, (B, max_det) + tuple(crop_hw) + (3,), dtype=np.uint8)
        status = (np.arange(max_det)[None, :] < count[:, None]).astype(np.int32)
        sharp = rng.integers(1, 1000, (B, max_det)).astype(np.uint64)
        inp = dict(det=det, count=count, tid=tid, slot=trk.last_slot.copy(), crops=crops, status=status, sharp=sharp,
                   stream_of=list(stream_of), ended_i=ei, ended_count=ec)
        poison = np.full((S, max_ended) + tuple(crop_hw) + (3,), 0xAB, np.uint8)
        calls.append((inp, gal.update(det, count, tid, inp['slot'], crops, status, sharp, stream_of, ei, ec, shot_crops=poison)))
    return gal, calls


def test_the_three_specifications_take_the_untracked_launch_calls():
    from yolov6.utils.lookback import LookbackNp
    from yolov6.utils.track import PlateTrackerNp
    S, T = UL['n_streams'], UL['max_tracks']
    calls = untracked_launch_calls()
    assert [len(c[0]) for c in calls] == [66, 3] and calls[0][2][:64] == [-1] * 64 and calls[1][2] == [-1] * 3 and calls[1][3] == [1, 0]
    trk = PlateTrackerNp(S, max_tracks=T, max_age=UL['max_age'])
    trk.enable_hold()
    lb = LookbackNp(trk, 2)
    for k, (det, count, stream_of, flush) in enumerate(calls):
        o, tid, _, _, ec = trk.update(det, count, stream_of, flush)
        rel = lb.update(*trk.last_hold[:2], trk.last_tid, trk.last_slot, stream_of, flush)
        untracked = [b for b, s in enumerate(stream_of) if s < 0]
        assert np.all(tid[untracked] == -1) and rel[2][untracked].tolist() == [-2] * len(untracked)    # copied, released at once
        assert np.array_equal(rel[1][untracked], count[untracked])
        if k == 0:
            assert tid[64:, 0].tolist() == [0, 0] and ec.tolist() == [0, 0] and rel[2][64:].tolist() == [-1, -1]
        else:
            assert ec.tolist() == [1, 0] and not trk.live(0).any() and trk.live(1).sum() == 1           # the flush ends stream 0's track
            assert rel[5][0, 0] == 0 and rel[4][0, 0] == 1 and rel[5][1].tolist() == [-1, -1]           # and hands its one frame out
    gal, shots = untracked_launch_shots()
    sc, si, sq, _ = shots[1][1]
    assert not shots[0][1][1].any()                                          # nothing ends in the first call
    assert gal.stats['taken'] == 2 and gal.stats['with_shot'] == 1 and si[0, 0].tolist() == [0, 0, 1, 1] and sq[0, 0] > 0
    assert np.array_equal(sc[0, 0], shots[0][0]['crops'][65, 0]) and not si[1].any() and gal.idp1[0].sum() == 0 and gal.idp1[1].sum() == 1
