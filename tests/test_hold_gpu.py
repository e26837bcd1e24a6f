"""Redaction held over missed frames on the GPU: lp_track_update_hold against its numpy specification bit for bit (rule 11 of
yolov6/utils/track.py) over the random cases of tests/test_track_gpu.py, held slots on both sides of the wave boundary, the
extremes of the row layout, hp == NULL against lp_track_update_slots, the steady state (no allocation, captured in a graph), the
chain update -> redact_plates on BGR and NV12 frames, and Inferer(track, redact, redact_hold) against PlateTrackerNp +
redact_plates_np on the same run's detections.  Every output is poisoned before each call; guard words lie behind the three
hold outputs."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
import test_track_cpu as C
import test_hold_cpu as H
import test_streams_cpu as U
from test_track_gpu import CASES, CFG, _assert_call_equal

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = 64                                             # words behind each hold output that no call may touch


def _poison(*bufs):
    for buf in bufs:
        buf.fill_(float('nan') if buf.dtype == torch.float32 else -7)


def _guarded(trk, B, max_det):
    """Plant hold buffers of (B, max_det) that are views of larger tensors: (the three views, the three guard regions)."""
    rows = max_det + trk.max_tracks
    views, guards = [], []
    for shape, dtype in (((B, rows, 28), torch.float32), ((B,), torch.int32), ((B, rows), torch.int32)):
        n = int(np.prod(shape))
        flat = torch.empty(n + GUARD, dtype=dtype, device='cuda')
        flat[n:] = 12345
        views.append(flat[:n].view(shape))
        guards.append(flat[n:])
    trk._hold['out'][(B, max_det)] = tuple(views)
    return tuple(views), guards


def _assert_hold_equal(got, want, guards, what):
    for name, g, w in zip(('det_hold', 'count_hold', 'tid_hold'), got, want):
        g = g.cpu().numpy()
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
        gi, wi = g.view(np.int32), np.ascontiguousarray(w).view(np.int32)
        if not np.array_equal(gi, wi):
            bad = np.argwhere(gi != wi)
            raise AssertionError('%s: %s differs in %d places, first at %s: got %r, want %r'
                                 % (what, name, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))
    for name, guard in zip(('det_hold', 'count_hold', 'tid_hold'), guards):
        assert bool((guard == 12345).all()), (what, name, 'guard words overwritten')


def _run_both(calls, n_streams, max_ended, min_hits=1, max_misses=None, whole_state=False, **kw):
    """The calls through runtime.PlateTracker and PlateTrackerNp, both with the hold: all eight outputs and the slots bit for
    bit, the state's ``dropped`` (``whole_state``: every word of it).  Returns (the numpy tracker, held rows seen)."""
    from yolov6.hip import runtime
    ref = H.tracker(True, n_streams, min_hits, max_misses, **kw)
    trk = runtime.PlateTracker(n_streams, device='cuda', **kw)
    trk.enable_hold(min_hits, max_misses)
    held = 0
    for k, (det, count, stream_of, flush) in enumerate(calls):
        B, max_det = det.shape[:2]
        want = ref.update(det, count, stream_of, flush, max_ended)
        hold, guards = _guarded(trk, B, max_det)
        _poison(trk.slot_buffer(B, max_det), *trk.buffers(B, max_det, max_ended), *hold)
        got = trk.update(torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda(), stream_of, flush, max_ended)
        _assert_call_equal(got, want, 'call %d' % k)
        assert np.array_equal(trk.slot_buffer(B, max_det).cpu().numpy(), ref.last_slot)
        assert all(a is b for a, b in zip(trk.last_hold, hold))
        _assert_hold_equal(trk.last_hold, ref.last_hold, guards, 'call %d' % k)
        held += int((ref.last_hold[1] - np.clip(count, 0, max_det)).sum())
    assert np.array_equal(trk.dropped.cpu().numpy(), ref.dropped)
    if whole_state:
        assert np.array_equal(trk.state.view(n_streams, -1).cpu().numpy(), U.track_state_words(ref))
    return ref, held


def test_a_launch_of_untracked_frames_only_and_a_flushed_stream_without_a_frame():
    """The first launch of call 1 holds untracked frames only (one workgroup of no stream copies them all); call 2 flushes a
    stream that has no frame in it (a workgroup of its own behind the frames' launch)."""
    ref, held = _run_both(U.untracked_launch_calls(), U.UL['n_streams'], 4, whole_state=True, max_tracks=U.UL['max_tracks'],
                          max_age=U.UL['max_age'])
    assert ref.stats['ended'] == 1 and ref.live(1).sum() == 1 and not ref.live(0).any() and ref.frame.tolist() == [1, 1]


@pytest.mark.parametrize('case', CASES, ids=lambda c: 's%d-t%d-d%d' % c[1:4])
def test_track_update_hold_equals_numpy_spec(case):
    seed, S, T, max_det, Bs, n_obj, extent, expand, max_age = case
    calls = C.random_track_case(seed, n_streams=S, max_det=max_det, n_obj=n_obj, extent=extent, Bs=Bs)
    ref, held = _run_both(calls, S, 6, min_hits=1 + seed % 2, max_misses=None if seed % 3 else 1,
                          max_tracks=T, match_thres=0.3, new_thres=0.2, expand=expand, max_age=max_age)
    assert ref.stats['matched'] > 0 and ref.stats['ended'] > 0
    assert (held > 0) == (max_age > 0)


def test_held_slots_on_both_sides_of_the_wave_boundary():
    """66 tracks in slots 0..65; frame 1 brings rows for the even slots only, so the odd slots 1, 3, .., 63 (wave 0) and 65 (wave 1)
    are held in that order; frame 2 follows in the same call: the state after the call describes frame 2, not frame 1."""
    box = lambda k, f: (100 * (k % 10) + 3 * f, 40 * (k // 10) + f, 100 * (k % 10) + 60 + 3 * f, 40 * (k // 10) + 20 + f)   # noqa: E731
    frames = [[C.make_row(box(k, 0), ids=(k % 24,) * 8) for k in range(66)],
              [C.make_row(box(k, 1), ids=(k % 24,) * 8) for k in range(0, 66, 2)],
              [C.make_row(box(k, 2), ids=(k % 24,) * 8) for k in range(0, 66, 3)]]
    det, count = C.frames_of(frames, 70)
    ref, held = _run_both([(det, count, [0, 0, 0], [0])], 1, 8, max_tracks=128, match_thres=0.3, new_thres=0.0, expand=0.5, max_age=3)
    dh, ch, th = ref.last_hold
    assert ch.tolist() == [66, 33 + 33, 22 + 44] and th[1, 33:66].tolist() == list(range(1, 66, 2))
    assert th[2, 22:66].tolist() == [k for k in range(66) if k % 3]
    assert np.array_equal(dh[2, 22 + 1, :4], np.array(box(2, 1), f32) + np.array([3, 1, 3, 1], f32))     # slot 2: seen in frame 1, v = (3, 1)
    assert np.array_equal(dh[2, 22, :4], np.array(box(1, 0), f32))                                       # slot 1: never seen again, v = 0


def test_extremes_of_the_row_layout():
    a, far = C.make_row(C.A), C.make_row(C.FAR, ids=(9,) * 8)
    # one slot, one row: nc == 0 with the held row at row 0; nc == max_det with the held row at row max_det + T - 1
    det, count = C.frames_of([[a], [], [far], [a]], 1)
    ref, held = _run_both([(det, count, [0] * 4, [1])], 1, 4, max_tracks=1, match_thres=0.3, new_thres=0.0, expand=0.5, max_age=3)
    dh, ch, th = ref.last_hold
    assert ch.tolist() == [1, 1, 2, 1] and th.tolist() == [[0, -1], [0, -1], [-1, 0], [0, -1]] and ref.dropped[0] == 1
    assert np.array_equal(dh[2, 0], far) and np.array_equal(dh[2, 1, :12], a[:12])
    # every one of T slots held behind a full frame: row max_det + T - 1 is written
    born = [C.make_row((100 * k, 0, 100 * k + 60, 20), ids=(k,) * 8) for k in range(4)]
    other = [C.make_row((100 * k, 300, 100 * k + 60, 320)) for k in range(4)]
    det, count = C.frames_of([born, other, []], 4)
    ref, held = _run_both([(det, count, [0] * 3, [0])], 1, 4, max_tracks=4, match_thres=0.3, new_thres=0.0, expand=0.5, max_age=3)
    dh, ch, th = ref.last_hold
    assert ch.tolist() == [4, 8, 4] and th[1].tolist() == [-1] * 4 + [0, 1, 2, 3] and th[2].tolist() == [0, 1, 2, 3] + [-1] * 4
    assert ref.dropped[0] == 4 and dh[1, 7, 20] == 3


def _raw_call(lib, fn, trk, det, count, stream_of, flush, out, slot, max_ended, hold=None):
    from yolov6.hip import abi, runtime
    B, max_det = det.shape[:2]
    so, fl = (ctypes.c_int * max(B, 1))(*stream_of), (ctypes.c_ubyte * trk.n_streams)(*flush)
    args = [trk.state.data_ptr(), trk.n_streams, trk.max_tracks, ctypes.byref(trk._params), det.data_ptr(), count.data_ptr(), B, max_det,
            so, ctypes.cast(fl, ctypes.c_void_p), out[0].data_ptr(), out[1].data_ptr(), slot.data_ptr(), *(t.data_ptr() for t in out[2:]),
            max_ended]
    if fn == 'lp_track_update_hold':
        args += list(hold)
    with torch.cuda.device(trk.device):
        return getattr(lib, fn)(*args, runtime._stream_ptr(trk.device))


def test_null_hold_params_is_lp_track_update_slots():
    from yolov6.hip import abi, runtime
    seed, S, T, max_det, Bs, n_obj, extent, expand, max_age = CASES[1]
    calls = C.random_track_case(seed, n_streams=S, max_det=max_det, n_obj=n_obj, extent=extent, Bs=Bs)
    kw = dict(max_tracks=T, match_thres=0.3, new_thres=0.2, expand=expand, max_age=max_age)
    a, b = runtime.PlateTracker(S, device='cuda', **kw), runtime.PlateTracker(S, device='cuda', **kw)
    lib = abi.load()
    for det, count, stream_of, flush in calls:
        B = len(det)
        d, c = torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda()
        outs = []
        for trk, fn in ((a, 'lp_track_update_slots'), (b, 'lp_track_update_hold')):
            out, slot = trk.buffers(B, max_det, 6), trk.slot_buffer(B, max_det)
            _poison(slot, *out)
            abi.check(_raw_call(lib, fn, trk, d, c, stream_of, flush, out, slot, 6, (None, None, None, None)), fn)   # null hold outputs are ignored
            outs.append([t.clone() for t in out + (slot,)])
        for x, y in zip(*outs):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert torch.equal(a.state, b.state)


def test_bad_hold_arguments_launch_nothing():
    from yolov6.hip import abi, runtime
    lib = abi.load()
    trk = runtime.PlateTracker(1, max_tracks=4, device='cuda')
    trk.enable_hold()
    det, count = C.frames_of([[C.make_row(C.A)]], 3)
    d, c = torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda()
    out, slot, hold = trk.buffers(1, 3, 4), trk.slot_buffer(1, 3), trk.hold_buffers(1, 3)
    ok = abi.TrackHoldParams(1, 3)
    bad = [(abi.TrackHoldParams(0, 3), hold), (abi.TrackHoldParams(1, -1), hold), (ok, (None,) + hold[1:]), (ok, (hold[0], None, hold[2])),
           (ok, hold[:2] + (None,)), (ok, (out[0],) + hold[1:]), (ok, (d,) + hold[1:])]
    for hp, (dh, ch, th) in bad:
        _poison(slot, *out, *hold)
        ptrs = [ctypes.byref(hp)] + [None if t is None else ctypes.c_void_p(t.data_ptr()) for t in (dh, ch, th)]
        assert _raw_call(lib, 'lp_track_update_hold', trk, d, c, [0], [0], out, slot, 4, ptrs) == -1
        torch.cuda.synchronize()
        assert not trk.state.any() and bool((slot == -7).all()) and bool((hold[1] == -7).all()) and bool(torch.isnan(out[0]).all())


# ---- with the best shots, and in the steady state ------------------------------------------------------------------------------
def test_enable_hold_with_enable_best_shot():
    from yolov6.hip import runtime
    frames, rows, boxes = H.missed_plate_frames()
    det, count = C.frames_of(rows, 2)
    kw = dict(max_tracks=4, match_thres=0.3, new_thres=0.0, expand=0.5, max_age=3)
    ref = H.tracker(**kw)
    ref.update(det, count, stream_of=[0] * 6, flush=[1])
    outs = []
    for hold in (False, True):
        trk = runtime.PlateTracker(1, device='cuda', **kw)
        trk.enable_best_shot((16, 48), max_crops=2)
        if hold:
            trk.enable_hold()
        dev = [torch.from_numpy(f).cuda() for f in frames]
        outs.append([t.clone() for t in trk.update_with_shots(dev, torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda(), [0] * 6, [1])])
    assert len(outs[0]) == len(outs[1]) == 9
    for x, y in zip(*outs):                                             # what update_with_shots returned before
        assert torch.equal(x, y)
    assert int(outs[1][4][0]) == 1                                      # the flush ended the one track
    _assert_hold_equal(trk.last_hold, ref.last_hold, [], 'with shots')
    assert ref.last_hold[1].tolist() == [1] * 6


def test_steady_state_no_allocation_and_graph_capture():
    """As tests/test_track_gpu.py: ten updates allocate nothing after the first, the update with the hold is captured in a graph
    (no host read) and its replays match the specification."""
    from yolov6.hip import runtime
    calls = C.random_track_case(21, n_streams=4, max_det=20, Bs=(4,) * 12)
    kw = dict(max_tracks=8, match_thres=0.3, new_thres=0.2, expand=0.5, max_age=2)
    trk, ref = runtime.PlateTracker(4, device='cuda', **kw), H.tracker(True, 4, **kw)
    trk.enable_hold()
    det = torch.from_numpy(calls[0][0]).cuda()
    count = torch.from_numpy(calls[0][1]).cuda()
    stream_of = [0, 1, 3, 1]
    trk.update(det, count, stream_of)
    ref.update(calls[0][0], calls[0][1], stream_of)
    torch.cuda.synchronize()
    for k in range(1, 10):
        det.copy_(torch.from_numpy(calls[k][0]))
        count.copy_(torch.from_numpy(calls[k][1]))
        after_copy = torch.cuda.memory_stats()['allocation.all.allocated']
        got = trk.update(det, count, stream_of)
        assert torch.cuda.memory_stats()['allocation.all.allocated'] == after_copy
        want = ref.update(calls[k][0], calls[k][1], stream_of)
    _assert_call_equal(got, want, 'call 9')
    _assert_hold_equal(trk.last_hold, ref.last_hold, [], 'call 9')
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = trk.update(det, count, stream_of)
    held = 0
    for k in (10, 11):
        det.copy_(torch.from_numpy(calls[k][0]))
        count.copy_(torch.from_numpy(calls[k][1]))
        _poison(*got, *trk.last_hold)
        g.replay()
        torch.cuda.synchronize()
        _assert_call_equal(got, ref.update(calls[k][0], calls[k][1], stream_of), 'replay %d' % k)
        _assert_hold_equal(trk.last_hold, ref.last_hold, [], 'replay %d' % k)
        held += int((ref.last_hold[1] - np.clip(calls[k][1], 0, 20)).sum())
    assert held > 0


# ---- the chain on the device ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nv12', [False, True], ids=['bgr', 'nv12'])
def test_update_then_redact_along_last_hold(nv12):
    from yolov6.hip import runtime
    from yolov6.utils.nv12 import Nv12Frame, bgr_to_nv12_np
    from yolov6.utils.redact import redact_plates_np
    frames, rows, boxes = H.missed_plate_frames()
    if nv12:
        frames = [bgr_to_nv12_np(f, 'bt709') for f in frames]
        dev = [Nv12Frame(torch.from_numpy(f.y).cuda(), torch.from_numpy(f.uv).cuda(), f.matrix) for f in frames]
    else:
        dev = [torch.from_numpy(f).cuda() for f in frames]
    det, count = C.frames_of(rows, 2)
    kw = dict(max_tracks=4, match_thres=0.3, new_thres=0.0, expand=0.5, max_age=3)
    ref = H.tracker(**kw)
    ref.update(det, count, stream_of=[0] * 6)
    want, want_st = redact_plates_np(frames, ref.last_hold[0], ref.last_hold[1], 'mosaic', 8, H.MARGIN)
    trk = runtime.PlateTracker(1, device='cuda', **kw)
    trk.enable_hold()
    trk.update(torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda(), [0] * 6)
    status = runtime.redact_plates(dev, *trk.last_hold[:2], mode='mosaic', cell=8, margin=H.MARGIN)
    torch.cuda.synchronize()
    assert np.array_equal(status.cpu().numpy(), want_st) and want_st[H.MISSED, 0] == 1
    x1, y1, x2, y2 = boxes[H.MISSED]
    for k, (f, w, src) in enumerate(zip(dev, want, frames)):
        if nv12:
            assert np.array_equal(f.y.cpu().numpy(), w.y) and np.array_equal(f.uv.cpu().numpy(), w.uv), k
        else:
            assert np.array_equal(f.cpu().numpy(), w), k
    got, src = (dev[H.MISSED].y.cpu().numpy(), frames[H.MISSED].y) if nv12 else (dev[H.MISSED].cpu().numpy(), frames[H.MISSED])
    assert (got[y1:y2, x1:x2] != src[y1:y2, x1:x2]).mean() > 0.9        # the missed frame's plate is a mosaic now


# ---- Inferer(track=True, redact=MODE, redact_hold=True) ------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gap_dir(tmp_path_factory):
    from PIL import Image
    from yolov6.utils.synth import build_synthetic
    d = tmp_path_factory.mktemp('hold')
    m = build_synthetic(CFG('yololps'), width=0.0625, sigma=1.5)
    torch.save({'model': m.half(), 'ema': None}, str(d / 'tiny.pt'))
    (d / 'imgs').mkdir()
    for k, f in enumerate(H.gap_frames(10, 4)):
        Image.fromarray(f).save(str(d / 'imgs' / ('f%02d.png' % k)))
    return d


@pytest.mark.parametrize('run_kw', [dict(batch_size=1), dict(batch_size=8), dict(batch_size=8, nv12='bt709')], ids=['b1', 'b8', 'b8-nv12'])
def test_infer_redact_hold_matches_numpy_on_detect_frames(gap_dir, tmp_path, monkeypatch, run_kw):
    from PIL import Image
    from yolov6.core.inferer import Inferer
    from yolov6.data.datasets import imread_bgr
    from yolov6.hip import runtime
    from yolov6.utils.nv12 import Nv12Frame, bgr_to_nv12_np, nv12_to_bgr_np
    from yolov6.utils.redact import redact_plates_np
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    src, ckpt, out = gap_dir / 'imgs', gap_dir / 'tiny.pt', tmp_path / 'out'
    files = sorted(os.listdir(str(src)))
    res = infer.run(weights=str(ckpt), source=str(src), yaml=None, img_size=[128, 160], conf_thres=0.06, iou_thres=0.45, max_det=20, device='0',
                    not_save_img=True, half=True, save_dir=str(out), track=True, track_max_age=2, track_iou=0.25, track_expand=0.25,
                    redact='mosaic', redact_cell=8, redact_hold=True, **run_kw)
    model = Inferer(str(src), str(ckpt), '0', None, [128, 160], True).model.model
    host = [np.ascontiguousarray(imread_bgr(str(src / f))) for f in files]
    if 'nv12' in run_kw:
        host = [bgr_to_nv12_np(f, run_kw['nv12']) for f in host]
        frames = [Nv12Frame(torch.from_numpy(f.y).cuda(), torch.from_numpy(f.uv).cuda(), f.matrix) for f in host]
    else:
        frames = [torch.from_numpy(f).cuda() for f in host]
    with torch.no_grad():
        plain = runtime.detect_frames(model, frames, [128, 160], 0.06, 0.45, 20)
    kw = dict(max_tracks=64, match_thres=0.25, new_thres=0.0, expand=0.25, max_age=2, ncls=model)
    outs, _, _ = C.track_by_hand([d.cpu().numpy() for d in plain], 20, **kw)
    want = H.hold_by_hand([d.cpu().numpy() for d in plain], 20, **kw)
    n_held = 0
    for k, (f, got, voted, (dh, ch)) in enumerate(zip(host, res, outs, want)):
        assert np.array_equal(got.cpu().numpy(), voted), k                  # the rows returned are the voted rows, as without the hold
        n_held += ch - len(voted)
        (w,), _ = redact_plates_np([f], dh[None], [ch], 'mosaic', 8, 0.1)
        if 'nv12' in run_kw:
            w = nv12_to_bgr_np(w)
        png = np.asarray(Image.open(str(out / 'redacted' / files[k])))
        assert np.array_equal(png, w[:, :, ::-1]), k
    assert n_held >= 1
