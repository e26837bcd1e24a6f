"""Redaction held over the frames in which a tracked plate was missed, on the CPU: rule 11 of the specification
(yolov6/utils/track.py::PlateTrackerNp.enable_hold), the argument checks of lp_track_update_hold (no device needed), a frame
sequence whose missed plate stays readable without the hold, and ``tools/infer.py --track --redact --redact-hold`` on the CPU
path.  ``missed_plate_frames`` and ``hold_by_hand`` are exported for tests/test_hold_gpu.py."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
import test_track_cpu as C

f32 = np.float32
LP_ERR_ARG = -1
STATE_ARRAYS = ('frame', 'next_id', 'dropped', 'id', 'first', 'last', 'hits', 'misses', 'box', 'cor', 'vel', 'votes', 'total')


def tracker(hold=True, n_streams=1, min_hits=1, max_misses=None, **kw):
    from yolov6.utils.track import PlateTrackerNp
    trk = PlateTrackerNp(n_streams, **kw)
    if hold:
        trk.enable_hold(min_hits, max_misses)
    return trk


def run_hold(trk, rows_per_frame, max_det, one_call=False):
    """Stream 0 through ``trk``: per frame (det_out, tid, det_hold, count_hold, tid_hold), one update per frame or one for all."""
    det, count = C.frames_of(rows_per_frame, max_det)
    out = []
    for lo, hi in ([(0, len(det))] if one_call else [(k, k + 1) for k in range(len(det))]):
        o, t = trk.update(det[lo:hi], count[lo:hi], stream_of=[0] * (hi - lo))[:2]
        dh, ch, th = trk.last_hold
        out += [(o[k].copy(), t[k].copy(), dh[k].copy(), int(ch[k]), th[k].copy()) for k in range(hi - lo)]
    return out


def check_layout(o, t, dh, ch, th, nc):
    """What holds of every frame: the frame's rows first, zero rows and -1 behind the count."""
    assert nc <= ch <= len(dh) and len(th) == len(dh)
    assert np.array_equal(dh[:nc].view(np.int32), o[:nc].view(np.int32)) and np.array_equal(th[:nc], t[:nc])
    assert not dh[ch:].view(np.int32).any() and np.all(th[ch:] == -1) and np.all(th[nc:ch] >= 0)


# ---- the crafted scene: every number dyadic, every sum exact -------------------------------------------------------------------
V = (4.0, 2.5)
SKEW = np.array([0.5, 0.25, -0.5, 0.75, 1.5, -0.25, 0.25, 0.5], f32)     # the corners are no rectangle


def scene_row(k, ids=(3, 7, 11, 0, 36, 21, 5, 9), conf=0.5):
    row = C.make_row((16 + V[0] * k, 8 + V[1] * k, 48 + V[0] * k, 24 + V[1] * k), ids, conf)
    row[4:12] += SKEW
    return row


def scene_frames():
    """One plate seen in frames 0-2, missed in 3-4, seen again in 5; in frame 1 head 7 reads another id at half the weight."""
    return [[scene_row(0)], [scene_row(1, ids=(3, 7, 11, 0, 36, 21, 5, 8), conf=(0.5,) * 7 + (0.25,))], [scene_row(2)], [], [], [scene_row(5)]]


@pytest.mark.parametrize('one_call', [False, True])
def test_crafted_scene_held_rows_are_last_geometry_plus_k_times_v(one_call):
    trk = tracker(max_tracks=4, match_thres=0.3, expand=0.5, max_age=3)
    out = run_hold(trk, scene_frames(), 3, one_call)
    last = scene_row(2)
    d = np.array(V * 6, f32)
    for f, (o, t, dh, ch, th) in enumerate(out):
        nc = 0 if f in (3, 4) else 1
        check_layout(o, t, dh, ch, th, nc)
        assert dh.shape == (3 + 4, 28) and th.shape == (7,)
        if f in (3, 4):
            k = f32(f - 2)
            assert ch == 1 and th[0] == 0                                       # the held row carries the track's id ...
            assert np.array_equal(dh[0, :12], last[:12] + k * d)                # ... the last geometry + k * v, bit for bit (exact sums)
            assert np.array_equal(dh[0, 12:28], out[2][0][0, 12:28])            # ... and its shares and voted ids: the read of frame 2
            assert tuple(dh[0, 20:28]) == (3, 7, 11, 0, 36, 21, 5, 9) and dh[0, 19] == f32(1.0) / f32(1.25)
        else:
            assert ch == 1 and t[0] == 0                                        # no held row; frame 5 continues track 0
    assert trk.hits[0, 0] == 4 and trk.next_id[0] == 1 and tuple(trk.vel[0, 0]) == V


def test_held_box_is_the_box_step_one_predicted():
    """Columns 0..3 of a held row are the prediction the matching of that frame used: a detection there has IoU 1 with it."""
    rng = np.random.default_rng(2)
    trk = tracker(max_tracks=4, expand=0.0, max_age=3)
    rows = [[C.make_row((10.3 + 3.7 * k + rng.random(), 20.1 + 1.3 * k, 50.9 + 3.7 * k, 33.3 + 1.3 * k))] for k in range(3)]
    out = run_hold(trk, rows + [[], []], 2)
    for f in (3, 4):
        with np.errstate(all='ignore'):
            k = f32(f - 2)
            dx, dy = trk.vel[0, 0, 0] * k, trk.vel[0, 0, 1] * k
            b = trk.box[0, 0]
            want = np.array([b[0] + dx, b[1] + dy, b[2] + dx, b[3] + dy], f32)
        assert out[f][3] == 1 and np.array_equal(out[f][2][0, :4], want) and not np.array_equal(want, b)


# ---- the gates -----------------------------------------------------------------------------------------------------------------
def test_min_hits_leaves_a_young_track_unheld():
    frames = [[C.make_row(C.A)], [], [C.make_row(C.A)], [C.make_row(C.A)], []]
    out = run_hold(tracker(min_hits=2, max_tracks=4, max_age=3), frames, 2)
    assert [o[3] for o in out] == [1, 0, 1, 1, 1] and out[4][4][0] == 0         # one hit: not held; two hits and more: held
    out = run_hold(tracker(min_hits=1, max_tracks=4, max_age=3), frames, 2)
    assert [o[3] for o in out] == [1, 1, 1, 1, 1] and out[1][4][0] == 0


def test_max_misses_holds_the_first_misses_only():
    frames = [[C.make_row(C.A)], [], [], [], [], []]
    for max_misses, want in ((1, [1, 1, 0, 0, 0, 0]), (0, [1, 0, 0, 0, 0, 0]), (None, [1, 1, 1, 1, 0, 0]), (99, [1, 1, 1, 1, 0, 0])):
        trk = tracker(max_misses=max_misses, max_tracks=4, max_age=3)
        out = run_hold(trk, frames, 2)
        assert [o[3] for o in out] == want, max_misses                          # (frame 4 ends the track: no row for it)
        assert not trk.live(0).any()


def test_max_age_zero_never_holds():
    calls = C.random_track_case(5)
    trk = tracker(n_streams=3, max_tracks=8, max_age=0, new_thres=0.2)
    for det, count, stream_of, flush in calls:
        o, t = trk.update(det, count, stream_of, flush)[:2]
        dh, ch, th = trk.last_hold
        nc = np.clip(count, 0, det.shape[1])
        assert np.array_equal(ch, nc) and dh.shape[1] == det.shape[1] + 8
        assert np.array_equal(dh[:, :det.shape[1]].view(np.int32), o.view(np.int32)) and not dh[:, det.shape[1]:].view(np.int32).any()
        assert np.array_equal(th[:, :det.shape[1]], t) and np.all(th[:, det.shape[1]:] == -1)
    assert trk.stats['ended'] > 0


def test_the_ending_frame_and_a_reused_slot_have_no_held_row():
    far = C.make_row(C.FAR, ids=(9,) * 8)
    out = run_hold(tracker(max_tracks=1, max_age=1), [[C.make_row(C.A)], [], []], 2)
    assert [o[3] for o in out] == [1, 1, 0] and np.all(out[2][4] == -1)         # frame 2: misses 2 > max_age, the track ends
    trk = tracker(max_tracks=1, max_age=1)
    out = run_hold(trk, [[C.make_row(C.A)], [], [far]], 2)
    o, t, dh, ch, th = out[2]
    assert t.tolist() == [1, -1] and ch == 1 and th.tolist() == [1, -1, -1]     # the freed slot holds track 1: its row, nothing held
    assert np.array_equal(dh[0, :12], far[:12]) and trk.id[0, 0] == 1


# ---- read-only -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed, kw', [(1, dict(max_tracks=4, max_age=2, expand=0.0)), (2, dict(max_tracks=16, max_age=3, expand=0.5)),
                                      (3, dict(max_tracks=1, max_age=3))])
def test_hold_changes_no_output_and_no_state(seed, kw):
    calls = C.random_track_case(seed)
    a, b = tracker(False, 3, new_thres=0.2, **kw), tracker(True, 3, new_thres=0.2, **kw)
    held = skipped = 0
    for det, count, stream_of, flush in calls:
        wa, wb = a.update(det, count, stream_of, flush, 5), b.update(det, count, stream_of, flush, 5)
        for x, y in zip(wa, wb):
            assert np.array_equal(x.view(np.int32), y.view(np.int32))
        assert np.array_equal(a.last_slot, b.last_slot) and a.last_hold is None
        for name in STATE_ARRAYS:
            assert np.array_equal(getattr(a, name).view(np.int32), getattr(b, name).view(np.int32)), name
        dh, ch, th = b.last_hold
        for k, s in enumerate(stream_of):
            nc = min(max(int(count[k]), 0), det.shape[1])
            check_layout(wb[0][k], wb[1][k], dh[k], int(ch[k]), th[k], nc)
            if s < 0:
                assert ch[k] == nc                                              # a frame that is not tracked holds nothing
                skipped += 1
            held += int(ch[k]) - nc
    assert held > 0 and skipped > 0


def test_counts_outside_the_range_skipped_frames_and_rows_past_128():
    trk = tracker(n_streams=2, max_tracks=128, max_age=2)
    det = np.zeros((2, 130, 28), f32)
    for r in range(130):
        det[:, r] = C.make_row((100 * (r % 12), 40 * (r // 12), 100 * (r % 12) + 60, 40 * (r // 12) + 20))
    o, t = trk.update(det, [-3, 1000])[:2]
    dh, ch, th = trk.last_hold
    assert dh.shape == (2, 258, 28) and ch.tolist() == [0, 130] and not dh[0].any() and np.all(th[0] == -1)
    assert np.array_equal(dh[1, :130], o[1]) and np.array_equal(th[1, :130], t[1]) and th[1, 128:].tolist() == [-1] * 130
    o, t = trk.update(det[:, :7], [3, 5], stream_of=[-1, 1])[:2]               # frame 0 is skipped; frame 1 misses 123 tracks
    dh, ch, th = trk.last_hold
    assert ch.tolist() == [3, 5 + 123] and np.array_equal(dh[0, :3], det[0, :3]) and not dh[0, 3:].any() and np.all(th[0] == -1)
    assert th[1].tolist() == list(range(128)) + [-1] * 7                        # five rows, then slots 5..127 in slot order
    assert np.array_equal(dh[1, 5:128, :12], det[1, 5:128, :12]) and np.all(dh[1, 5:128, 12:20] == 1)      # (zero velocity)
    o, t = trk.update(det[:, :7], [-3, 0], stream_of=[1, 1])[:2]               # count < 0: no row, every track held; then 123 end
    dh, ch, th = trk.last_hold
    assert ch.tolist() == [128, 5] and th[0, :128].tolist() == list(range(128)) and th[1, :6].tolist() == [0, 1, 2, 3, 4, -1]


def test_enable_hold_checks_its_arguments():
    from yolov6.utils.track import PlateTrackerNp
    trk = PlateTrackerNp(1, max_age=3)
    with pytest.raises(RuntimeError):
        trk.hold_buffers(1, 4)
    for bad in (dict(min_hits=0), dict(max_misses=-1)):
        with pytest.raises(ValueError):
            trk.enable_hold(**bad)
    trk.enable_hold()
    assert trk.hold_buffers(2, 4)[0].shape == (2, 4 + 64, 28) and trk.hold_buffers(2, 4)[0] is trk.hold_buffers(2, 4)[0]


# ---- the test that fails without the feature: a missed frame's plate stays readable --------------------------------------------
H, W, MARGIN, MISSED = 64, 96, 0.125, 3


def missed_plate_frames(n=6):
    """(frames [n] of 64 x 96 BGR with a textured 32 x 12 plate moving (4, 2) px per frame, rows per frame, box per frame): the
    detector misses frame ``MISSED``.  Texture and background are never 0, so a black fill changes every byte it writes."""
    rng = np.random.default_rng(8)
    plate = rng.integers(1, 256, (12, 32, 3), dtype=np.uint8)
    frames, rows, boxes = [], [], []
    for k in range(n):
        f = rng.integers(1, 256, (H, W, 3), dtype=np.uint8)
        x, y = 8 + 4 * k, 6 + 2 * k
        f[y:y + 12, x:x + 32] = plate
        frames.append(f)
        boxes.append((x, y, x + 32, y + 12))
        rows.append([] if k == MISSED else [C.make_row(boxes[-1])])
    return frames, rows, boxes


def test_missed_plate_is_readable_along_det_out_and_redacted_along_last_hold():
    from yolov6.utils.redact import redact_plates_np
    frames, rows, boxes = missed_plate_frames()
    trk = tracker(max_tracks=4, max_age=3)
    det, count = C.frames_of(rows, 2)
    o = trk.update(det, count, stream_of=[0] * len(det))[0]
    dh, ch, th = trk.last_hold
    plain, _ = redact_plates_np(frames, o, count, 'fill', 16, MARGIN)
    held, status = redact_plates_np(frames, dh, ch, 'fill', 16, MARGIN)
    x1, y1, x2, y2 = boxes[MISSED]
    assert np.array_equal(plain[MISSED], frames[MISSED])                        # along det_out the plate leaves as it came
    assert ch.tolist() == [1] * 6 and th[MISSED, 0] == 0 and tuple(dh[MISSED, 0, :4]) == boxes[MISSED]     # (integer velocity: exact)
    assert np.all(held[MISSED][y1:y2, x1:x2] == 0)                              # every pixel inside the held quad changed
    gx, gy = MARGIN * (x2 - x1) / 2, MARGIN * (y2 - y1) / 2
    keep = np.ones((H, W), bool)
    keep[int(np.floor(y1 - gy)):int(np.ceil(y2 + gy)), int(np.floor(x1 - gx)):int(np.ceil(x2 + gx))] = False
    assert np.array_equal(held[MISSED][keep], frames[MISSED][keep])             # no byte outside its rectangle plus margin
    for k in range(6):
        if k != MISSED:
            assert np.array_equal(held[k], plain[k]) and (held[k] != frames[k]).any()


# ---- C ABI: the hold arguments are checked on the host before any launch -------------------------------------------------------
def test_track_update_hold_rejects_bad_arguments_before_launch():
    from yolov6.hip import abi
    lib = abi.load()
    v = lambda p: ctypes.c_void_p(p) if p else None   # noqa: E731

    def call(min_hits=1, max_misses=3, det_hold=0x100000, count_hold=0x7000, tid_hold=0x8000, hp=True, max_det=10, max_tracks=8,
             det=0x10000, det_out=0x20000):
        p = abi.TrackParams(0.3, 0.0, 0.5, 5, (ctypes.c_int * 8)(*C.NCLS))
        so = (ctypes.c_int * 3)(0, 1, -1)
        h = abi.TrackHoldParams(min_hits, max_misses)
        return lib.lp_track_update_hold(v(0x1000), 2, max_tracks, ctypes.byref(p), v(det), v(0x2000), 3, max_det, so, None, v(det_out),
                                        v(0x3000), None, v(0x4000), v(0x5000), v(0x6000), 4, ctypes.byref(h) if hp else None,
                                        v(det_hold), v(count_hold), v(tid_hold), None)

    err = lambda: lib.lp_last_error()   # noqa: E731
    assert call(min_hits=0) == LP_ERR_ARG and b'min_hits' in err()
    assert call(max_misses=-1) == LP_ERR_ARG and b'max_misses' in err()
    for k in ('det_hold', 'count_hold', 'tid_hold'):
        assert call(**{k: 0}) == LP_ERR_ARG and b'null' in err(), k
    hold_bytes, det_bytes = 3 * 18 * 28 * 4, 3 * 10 * 28 * 4
    for other in (0x10000, 0x20000):                                            # det, det_out
        assert call(det_hold=other) == LP_ERR_ARG and b'alias' in err()
        assert call(det_hold=other + det_bytes - 4) == LP_ERR_ARG and b'alias' in err()
        assert call(det_hold=other - hold_bytes + 4) == LP_ERR_ARG and b'alias' in err()
    assert call(max_det=0x7fffffff // 28 - 7) == LP_ERR_ARG and b'overflow' in err()                # (max_det + 8 slots) * 28 >= 2^31
    assert call(hp=False, det=0) == LP_ERR_ARG and b'null' in err()             # hp == NULL: the checks of lp_track_update_slots


# ---- tools/infer.py --track --redact --redact-hold on the CPU path -------------------------------------------------------------
def hold_by_hand(dets, max_det, min_hits=1, **kw):
    """``PlateTrackerNp`` with the hold over the untracked per-frame detections of one stream, one update per frame: per frame
    (det_hold [max_det + max_tracks, 28], count_hold), copies."""
    trk = tracker(min_hits=min_hits, **kw)
    out = []
    for d in dets:
        pad = np.zeros((1, max_det, 28), f32)
        pad[0, :len(d)] = d
        trk.update(pad, [len(d)], max_ended=2 * trk.max_tracks)
        out.append((trk.last_hold[0][0].copy(), int(trk.last_hold[1][0])))
    return out


def gap_frames(n=6, gap=3):
    """``_moving_frames`` with frame ``gap`` replaced by unrelated noise: what was tracked is missed there, and a mosaic shows."""
    frames = C._moving_frames(n)
    frames[gap] = np.random.default_rng(99).integers(0, 255, frames[gap].shape, dtype=np.uint8)
    return frames


def test_redact_hold_needs_track_and_redact():
    from yolov6.core.inferer import Inferer
    for kw in (dict(track=True), dict(redact='mosaic'), dict()):
        with pytest.raises(ValueError, match='redact_hold'):
            Inferer('nowhere', 'nothing.pt', 'cpu', None, [128, 160], False, redact_hold=True, **kw)


def test_infer_redact_hold_cpu(tmp_path, monkeypatch):
    from PIL import Image
    from yolov6.utils.redact import redact_plates_np
    from yolov6.utils.synth import build_synthetic
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    m = build_synthetic(os.path.join(REPO, 'configs', 'yololps.py'), width=0.0625, sigma=1.5)
    ckpt = tmp_path / 'tiny.pt'
    torch.save({'model': m.half(), 'ema': None, 'epoch': 0}, str(ckpt))
    img_dir = tmp_path / 'imgs'
    img_dir.mkdir()
    frames = gap_frames()
    for k, f in enumerate(frames):
        Image.fromarray(f).save(str(img_dir / ('f%02d.png' % k)))
    kw = dict(weights=str(ckpt), source=str(img_dir), yaml=None, img_size=[128, 160], conf_thres=0.06, iou_thres=0.45, max_det=20,
              device='cpu', not_save_img=True)
    plain = infer.run(save_dir=str(tmp_path / 'o1'), **kw)
    tkw = dict(track=True, track_max_age=2, track_iou=0.25, track_expand=0.25, redact='mosaic', redact_cell=8)
    voted = infer.run(save_dir=str(tmp_path / 'o2'), **tkw, **kw)
    held = infer.run(save_dir=str(tmp_path / 'o3'), redact_hold=True, **tkw, **kw)
    for a, b in zip(voted, held):
        assert torch.equal(a, b)                                                # the rows returned are what they are without the hold
    assert (tmp_path / 'o2' / 'tracks.txt').read_bytes() == (tmp_path / 'o3' / 'tracks.txt').read_bytes()
    assert (tmp_path / 'o2' / 'plates.txt').read_bytes() == (tmp_path / 'o3' / 'plates.txt').read_bytes()
    want = hold_by_hand([d.numpy() for d in plain], 20, max_tracks=64, match_thres=0.25, new_thres=0.0, expand=0.25, max_age=2, ncls=m)
    n_held = differs = 0
    for k, (f, d, (dh, ch)) in enumerate(zip(frames, plain, want)):
        n_held += ch - len(d)
        (w,), _ = redact_plates_np([f[:, :, ::-1]], dh[None], [ch], 'mosaic', 8, 0.1)
        got = np.asarray(Image.open(str(tmp_path / 'o3' / 'redacted' / ('f%02d.png' % k))))
        assert np.array_equal(got, w[:, :, ::-1]), k
        differs += int(not np.array_equal(got, np.asarray(Image.open(str(tmp_path / 'o2' / 'redacted' / ('f%02d.png' % k))))))
    assert n_held >= 1 and differs >= 1                                         # the run holds at least one row, and it shows
