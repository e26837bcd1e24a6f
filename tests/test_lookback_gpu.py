"""The look-back delay of redaction on the GPU: lp_lookback_update against its numpy specification bit for bit
(yolov6/utils/lookback.py::LookbackNp) on what PlateTrackerNp leaves of random detection sequences -- every output and the tails
poisoned before each call and compared whole, guard words behind them, the state word for word after the last call -- bad
arguments that launch nothing, the chain PlateTracker.update -> LookbackRedactor.push on BGR and NV12 frames with a mosaic and a
fill (the late plate of tests/test_lookback_cpu.py among them), the steady state (no allocation, captured in a graph) and
``tools/infer.py --redact-lookback`` against the numpy path on the same run's detections."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
import test_track_cpu as C
import test_lookback_cpu as L
import test_streams_cpu as U
from test_track_gpu import CFG

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = 64                                             # words behind each output that no call may touch
S, T, MAX_DET = 3, 8, 12
NAMES = ('rel_det', 'rel_count', 'rel_frame', 'tail_det', 'tail_count', 'tail_frame')


def _guarded(shapes):
    """Poisoned device tensors of ``shapes`` ((shape, dtype), ...) that are views of larger ones: (views, guard regions)."""
    views, guards = [], []
    for shape, dtype in shapes:
        n = int(np.prod(shape))
        flat = torch.empty(n + GUARD, dtype=dtype, device='cuda')
        flat[:n] = float('nan') if dtype == torch.float32 else -7
        flat[n:] = 12345
        views.append(flat[:n].view(shape))
        guards.append(flat[n:])
    return views, guards


def _out_shapes(B, rows, D, n_streams=S):
    return (((B, rows, 28), torch.float32), ((B,), torch.int32), ((B,), torch.int32),
            ((n_streams, D, rows, 28), torch.float32), ((n_streams, D), torch.int32), ((n_streams, D), torch.int32))


def _raw(lib, state, n_streams, max_tracks, D, max_back, back_cap, ins, B, max_det, hold_rows, stream_of, flush, outs):
    from yolov6.hip import runtime
    so = (ctypes.c_int * max(B, 1))(*stream_of)
    fl = (ctypes.c_ubyte * n_streams)(*flush)
    p = lambda t: None if t is None else ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())   # noqa: E731
    dev = torch.device('cuda', torch.cuda.current_device())
    return lib.lp_lookback_update(p(state), n_streams, max_tracks, D, max_back, back_cap, *(p(t) for t in ins), B, max_det, hold_rows, so,
                                  ctypes.cast(fl, ctypes.c_void_p), *(p(t) for t in outs), runtime._stream_ptr(dev))


def _assert_equal(got, want, guards, what):
    for name, g, w, guard in zip(NAMES, got, want, guards):
        g = g.cpu().numpy()
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        gi, wi = g.view(np.int32), np.ascontiguousarray(w).view(np.int32)
        if not np.array_equal(gi, wi):
            bad = np.argwhere(gi != wi)
            raise AssertionError('%s: %s differs in %d places, first at %s: got %r, want %r'
                                 % (what, name, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))
        assert bool((guard == 12345).all()), (what, name, 'guard words overwritten')


def _run_kernel_against_spec(calls, D, max_back, back_cap, n_streams=S, max_tracks=T, **kw):
    """The calls through PlateTrackerNp (hold enabled) and LookbackNp; the tracker's outputs are uploaded and go through
    lp_lookback_update.  Returns the numpy delay line."""
    from yolov6.hip import abi
    lib = abi.load()
    trk, lb = L.pair(D, n_streams, max_back, back_cap, max_tracks=max_tracks, **kw)
    max_det = calls[0][0].shape[1]
    hold_rows = max_det + max_tracks
    rows = hold_rows + lb.back_cap
    nbytes = lib.lp_lookback_state_bytes(n_streams, max_tracks, D, rows)
    assert nbytes > 0 and nbytes % 16 == 0
    state = torch.zeros(nbytes // 4, dtype=torch.int32, device='cuda')
    for k, (det, count, stream_of, flush) in enumerate(calls):
        B = det.shape[0]
        trk.update(det, count, stream_of, flush)
        dh, ch, _ = trk.last_hold
        want = lb.update(dh, ch, trk.last_tid, trk.last_slot, stream_of, flush)
        ins = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (dh, ch, trk.last_tid, trk.last_slot)]
        behind = torch.full((dh.size + (lb.back_cap + 1) * 28,), float('nan'), device='cuda')     # det_hold with NaNs right behind it:
        behind[:dh.size] = ins[0].view(-1)                                                        # no output may depend on them
        ins[0] = behind[:dh.size].view(dh.shape)
        outs, guards = _guarded(_out_shapes(B, rows, D, n_streams))
        abi.check(_raw(lib, state, n_streams, max_tracks, D, lb.max_back, lb.back_cap, ins, B, max_det, hold_rows, stream_of, flush, outs),
                  'lp_lookback_update')
        torch.cuda.synchronize()
        _assert_equal(outs, want, guards, 'call %d (B = %d)' % (k, B))
    got = state.view(n_streams, -1).cpu().numpy()
    want = lb.state_words()
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError('state differs in %d words, first at %s: got %d, want %d' % (len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))
    return lb


# B = 1, B = S, B = 7 (several frames of one stream in a call); random_track_case adds frames with stream_of -1, flushes in
# mid-sequence and the flush of everything in the last call.  The seeds are those whose draw gives every stream 20 to 30 frames.
BS = (1, 3, 7, 3, 1, 7, 1, 3, 7, 7, 3, 1, 7, 3, 1, 7, 3, 7, 3, 7)
KERNEL_CASES = [(31, 1, None, None), (37, 2, None, None), (38, 5, None, None), (41, 5, 1, None), (48, 5, None, 2), (50, 2, 0, 0)]


@pytest.mark.parametrize('case', KERNEL_CASES, ids=lambda c: 'D%d-back%s-cap%s' % c[1:])
def test_lookback_update_equals_numpy_spec(case):
    seed, D, max_back, back_cap = case
    calls = C.random_track_case(seed, n_streams=S, max_det=MAX_DET, n_obj=5, extent=400, Bs=BS)
    assert any(-1 in so for _, _, so, _ in calls) and any(any(fl) for _, _, _, fl in calls[:-1])
    lb = _run_kernel_against_spec(calls, D, max_back, back_cap, match_thres=0.3, new_thres=0.2, expand=0.5, max_age=2)
    assert lb.stats['confirmed'] > 0 and lb.stats['back_rows'] > 0 and all(20 <= f <= 30 for f in lb.f.tolist())


def test_calls_that_split_into_several_launches():
    """B = 70 > LP_FRAMES_PER_LAUNCH: a second frame launch on offset pointers, untracked frames dealt over many workgroups;
    66 streams: a second closing launch."""
    calls = C.random_track_case(41, n_streams=66, max_det=4, n_obj=2, extent=300, Bs=(70, 5, 66, 70))
    assert sum(so.count(-1) for _, _, so, _ in calls) >= 10 and all(len(set(so[:64])) >= 30 for _, _, so, _ in calls if len(so) > 64)
    lb = _run_kernel_against_spec(calls, 2, None, None, n_streams=66, max_tracks=2, match_thres=0.3, new_thres=0.2, expand=0.5, max_age=2)
    assert lb.stats['confirmed'] > 0 and lb.stats['back_rows'] > 0 and lb.f.max() >= 5


def test_a_launch_of_untracked_frames_only_and_a_flushed_stream_without_a_frame():
    """The first launch of call 1 holds untracked frames only: one workgroup of no stream releases them all at once; call 2 has no
    tracked frame and hands out the tail of a flushed stream."""
    lb = _run_kernel_against_spec(U.untracked_launch_calls(), 2, None, None, n_streams=U.UL['n_streams'], max_tracks=U.UL['max_tracks'],
                                  max_age=U.UL['max_age'])
    assert lb.f.tolist() == [1, 1] and lb.base.tolist() == [1, 0]


def test_full_entry_overflows_into_dropped():
    """back_cap = 2 behind a full entry (12 rows + 8 held): two of three back rows fit, ``dropped`` is compared with the state."""
    det, count = C.frames_of(L.full_entry_rows(MAX_DET, T), MAX_DET)
    calls = [(det[:3], count[:3], [0, 0, 0], [0]), (det[3:], count[3:], [0], [1])]
    lb = _run_kernel_against_spec(calls, 5, None, 2, n_streams=1, match_thres=0.3, new_thres=0.2, expand=0.5, max_age=1)
    assert lb.stats == dict(confirmed=3, back_rows=5) and lb.dropped.tolist() == [1]


def test_bad_arguments_launch_nothing():
    from yolov6.hip import abi
    lib = abi.load()
    D, B, hold_rows = 2, 2, MAX_DET + T
    rows = hold_rows + 4
    state = torch.zeros(lib.lp_lookback_state_bytes(S, T, D, rows) // 4, dtype=torch.int32, device='cuda')
    ins = [torch.ones(B, hold_rows, 28, device='cuda'), torch.full((B,), 3, dtype=torch.int32, device='cuda'),
           torch.zeros(B, MAX_DET, dtype=torch.int32, device='cuda'), torch.zeros(B, MAX_DET, dtype=torch.int32, device='cuda')]
    outs, guards = _guarded(_out_shapes(B, rows, D))
    ok = dict(D=D, max_back=2, back_cap=4, ins=ins, stream_of=[0, 1], outs=outs, max_det=MAX_DET, hold_rows=hold_rows, T=T)
    bad = [dict(D=0), dict(D=33), dict(max_back=-1), dict(back_cap=-1), dict(T=0), dict(T=129), dict(max_det=0), dict(hold_rows=MAX_DET - 1),
           dict(stream_of=[0, S]), dict(stream_of=[-2, 0]), dict(ins=[None] + ins[1:]), dict(ins=ins[:3] + [None]),
           dict(outs=[None] + outs[1:]), dict(outs=outs[:3] + [None] + outs[4:]), dict(outs=outs[:5] + [None]),
           dict(outs=[ins[0]] + outs[1:]), dict(outs=outs[:3] + [ins[0]] + outs[4:]), dict(outs=[outs[3]] + outs[1:]),
           dict(outs=[outs[0].data_ptr() + 4] + outs[1:]), dict(ins=[ins[0].data_ptr() + 8] + ins[1:]),
           dict(outs=[state.data_ptr() + 64] + outs[1:]), dict(outs=outs[:1] + [state.data_ptr() + 8] + outs[2:]),
           dict(outs=outs[:2] + [outs[1]] + outs[3:]), dict(outs=outs[:5] + [ins[2]])]
    for k, change in enumerate(bad):
        a = dict(ok, **change)
        rc = _raw(lib, state, S, a['T'], a['D'], a['max_back'], a['back_cap'], a['ins'], B, a['max_det'], a['hold_rows'], a['stream_of'],
                  [1] * S, a['outs'])
        assert rc == L.LP_ERR_ARG, (k, change.keys(), rc)
    torch.cuda.synchronize()
    assert not state.any()
    for t, guard in zip(outs, guards):
        assert bool((torch.isnan(t) if t.dtype == torch.float32 else t == -7).all()) and bool((guard == 12345).all())


# ---- the chain on the device ---------------------------------------------------------------------------------------------------
def _to_device(frames):
    from yolov6.utils.nv12 import Nv12Frame
    return [Nv12Frame(torch.from_numpy(f.y).cuda(), torch.from_numpy(f.uv).cuda(), f.matrix) if isinstance(f, Nv12Frame)
            else torch.from_numpy(f).cuda() for f in frames]


def _assert_frames_equal(got, want, what=''):
    from yolov6.utils.nv12 import Nv12Frame
    assert [(s, g) for s, g, _ in got] == [(s, g) for s, g, _ in want], what
    for k, ((_, _, a), (_, _, b)) in enumerate(zip(got, want)):
        if isinstance(b, Nv12Frame):
            assert np.array_equal(a.y.cpu().numpy(), b.y) and np.array_equal(a.uv.cpu().numpy(), b.uv), (what, k)
        else:
            assert np.array_equal(a.cpu().numpy(), b), (what, k)


@pytest.mark.parametrize('mode', ['mosaic', 'fill'])
@pytest.mark.parametrize('nv12', [False, True], ids=['bgr', 'nv12'])
def test_update_then_push_equals_the_numpy_chain(nv12, mode):
    from yolov6.hip import runtime
    from yolov6.utils.lookback import LookbackNp
    from yolov6.utils.nv12 import bgr_to_nv12_np
    from yolov6.utils.redact import redact_plates_np
    from yolov6.utils.track import PlateTrackerNp
    bgr, rows, boxes = L.late_plate_frames()
    frames = [bgr_to_nv12_np(f, 'bt709') for f in bgr] if nv12 else bgr
    dev = _to_device(frames)
    det, count = C.frames_of(rows, 4)
    kw = dict(mode=mode, cell=8, margin=L.MARGIN, fill=L.FILL)
    ref = PlateTrackerNp(2, max_tracks=4)
    trk = runtime.PlateTracker(2, max_tracks=4, device='cuda')
    ref.enable_hold(), trk.enable_hold()
    ref_lb, lb = LookbackNp(ref, L.DEPTH, **kw), runtime.LookbackRedactor(trk, L.DEPTH, **kw)
    got, want = [], []
    # four frames of stream 1 in one call (the last slot is padding without a frame), then one call per frame, then the flush
    for lo, hi in [(0, 4)] + [(k, k + 1) for k in range(4, len(frames))]:
        so = [1] * (hi - lo) + ([-1] if lo == 0 else [])
        d = np.concatenate([det[lo:hi], np.zeros((len(so) - (hi - lo), 4, 28), f32)])
        c = np.concatenate([count[lo:hi], np.zeros(len(so) - (hi - lo), np.int32)])
        ref.update(d, c, so)
        want += ref_lb.push(frames[lo:hi], so)
        trk.update(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda(), so)
        got += lb.push(dev[lo:hi], so)
    ref.flush_all(), trk.flush_all()
    want += ref_lb.flush_all()
    got += lb.flush_all()
    torch.cuda.synchronize()
    assert [(s, g) for s, g, _ in got] == [(1, k) for k in range(len(frames))] and all(a is b for (_, _, a), b in zip(got, dev))
    _assert_frames_equal(got, want)
    assert lb.dropped.tolist() == [0, 0] and ref_lb.stats == dict(confirmed=1, back_rows=3)
    if not nv12 and mode == 'fill':             # the coverage assertion of the CPU test, on the device's bytes
        hold_only, t2 = [], PlateTrackerNp(1, max_tracks=4)
        t2.enable_hold()
        for k, f in enumerate(bgr):
            t2.update(det[k:k + 1], count[k:k + 1], [0])
            hold_only += redact_plates_np([f], t2.last_hold[0], t2.last_hold[1], **kw)[0]
        L.check_late_plate(bgr, boxes, hold_only, [f.cpu().numpy() for _, _, f in got])
    else:
        src = [f.y if nv12 else f for f in frames]
        out = [(f.y if nv12 else f).cpu().numpy() for _, _, f in got]
        for k in range(L.LATE):
            x1, y1, x2, y2 = boxes[k]
            assert (out[k][y1:y2, x1:x2] != src[k][y1:y2, x1:x2]).mean() > 0.9      # the early frames' plate is covered


def test_untracked_frames_come_back_at_once_redacted():
    from yolov6.hip import runtime
    from yolov6.utils.lookback import LookbackNp
    from yolov6.utils.track import PlateTrackerNp
    bgr, rows, boxes = L.late_plate_frames(6)
    det, count = C.frames_of(rows, 4)
    dev = _to_device(bgr)
    ref, trk = PlateTrackerNp(1, max_tracks=4), runtime.PlateTracker(1, max_tracks=4, device='cuda')
    ref.enable_hold(), trk.enable_hold()
    ref_lb, lb = LookbackNp(ref, 2, mode='mosaic', cell=8), runtime.LookbackRedactor(trk, 2, mode='mosaic', cell=8)
    so = [0, -1, 0, -1, -1, 0]
    ref.update(det, count, so)
    trk.update(torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda(), so)
    want, got = ref_lb.push(bgr, so, [1]), lb.push(dev, so, [1])
    torch.cuda.synchronize()
    assert [(s, g) for s, g, _ in got] == [(-1, -2), (-1, -2), (-1, -2), (0, 0), (0, 1), (0, 2)]
    _assert_frames_equal(got, want)
    assert (got[1][2].cpu().numpy() != bgr[3]).any() and lb.pending(0) == 0


def test_flush_before_the_first_frame_and_a_push_that_raises():
    from yolov6.hip import runtime
    bgr, rows, boxes = L.late_plate_frames(5)
    dev = _to_device(bgr)
    trk = runtime.PlateTracker(1, max_tracks=4, device='cuda')
    trk.enable_hold()
    lb = runtime.LookbackRedactor(trk, 2, mode='fill')
    trk.flush_all()
    assert lb.flush_all() == [] and lb.state is None                           # no entry size is fixed by a call without frames
    det, count = C.frames_of(rows, 4)
    d, c = torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda()
    trk.update(d[:3], c[:3], [0] * 3)
    assert [(s, g) for s, g, _ in lb.push(dev[:3], [0] * 3)] == [(0, 0)] and lb.entry_rows == 4 + 4 + 4
    other = torch.zeros(1, 6, 28, device='cuda')
    trk.update(other, c[3:4], [0])                                             # another max_det: the push raises ...
    with pytest.raises(ValueError, match='rows'):
        lb.push(dev[3:4], [0])
    assert lb.pending(0) == 2                                                  # ... and neither counters nor frames have moved
    trk.update(d[3:4], c[3:4], [0])
    out = lb.push(dev[3:4], [0], [1])
    torch.cuda.synchronize()
    assert [(s, g) for s, g, _ in out] == [(0, 1), (0, 2), (0, 3)] and all(f is dev[g] for _, g, f in out)
    assert int(lb.state.view(1, -1)[0, 0]) == 4 and int(lb.state.view(1, -1)[0, 1]) == 4


# ---- the steady state ----------------------------------------------------------------------------------------------------------
def test_steady_state_no_allocation():
    from yolov6.hip import runtime
    rng = np.random.default_rng(4)
    n = 14
    rows = [[C.make_row((10 + 3 * k, 8 + k, 42 + 3 * k, 20 + k))] if k % 5 else [] for k in range(n)]
    det, count = C.frames_of(rows, 4)
    trk = runtime.PlateTracker(2, max_tracks=4, device='cuda')
    trk.enable_hold()
    lb = runtime.LookbackRedactor(trk, 2, mode='mosaic', cell=8)
    frames = [[torch.from_numpy(rng.integers(0, 255, (64, 96, 3), dtype=np.uint8)).cuda() for _ in range(2)] for _ in range(n)]
    dets = [(torch.from_numpy(det[[k, k]]).cuda(), torch.from_numpy(count[[k, k]]).cuda()) for k in range(n)]
    back = 0
    for k in range(n):
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats()['allocation.all.allocated']
        trk.update(*dets[k], [0, 1])
        out = lb.push(frames[k], [0, 1])
        if k >= 4:                                                              # ten pushes behind the warm-up
            assert torch.cuda.memory_stats()['allocation.all.allocated'] == before, k
        assert [(s, g) for s, g, _ in out] == ([(0, k - 2), (1, k - 2)] if k >= 2 else [])
        back += len(out)
    assert back == 2 * (n - 2) and lb.pending(0) == lb.pending(1) == 2


def test_update_push_captured_in_a_graph_replays_the_eager_bytes():
    """Tracker update + look-back + redact as one linear chain on one stream: four frames of one stream with the flush, D = 2, so
    that all four leave in the call; the replay on reset state and restored frames gives the eager run's bytes."""
    from yolov6.hip import runtime
    bgr, rows, boxes = L.late_plate_frames(7)
    bgr, rows = bgr[2:6], rows[2:6]                                             # first detection in the call's second frame
    det, count = C.frames_of(rows, 4)
    d, c = torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda()
    dev = _to_device(bgr)
    trk = runtime.PlateTracker(1, max_tracks=4, device='cuda')
    trk.enable_hold()
    lb = runtime.LookbackRedactor(trk, 2, mode='mosaic', cell=8)

    def chain():
        trk.update(d, c, [0] * 4, [1])
        return lb.push(dev, [0] * 4, [1])

    out = chain()
    torch.cuda.synchronize()
    assert [(s, g) for s, g, _ in out] == [(0, k) for k in range(4)]
    eager = [f.cpu().numpy() for f in dev]
    assert (eager[0] != bgr[0]).any()                                           # the frame before the first detection got its back row
    for f, src in zip(dev, bgr):
        f.copy_(torch.from_numpy(src))
    trk.reset(), lb.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = chain()
    torch.cuda.synchronize()
    for f, src in zip(dev, bgr):
        assert np.array_equal(f.cpu().numpy(), src)                             # the capture ran nothing
    g.replay()
    torch.cuda.synchronize()
    assert [(s, k) for s, k, _ in out] == [(0, k) for k in range(4)]
    for k, (f, w) in enumerate(zip(dev, eager)):
        assert np.array_equal(f.cpu().numpy(), w), k


# ---- tools/infer.py --track --redact fill --redact-hold --redact-lookback 4 ----------------------------------------------------
@pytest.fixture(scope='module')
def late_dir(tmp_path_factory):
    from PIL import Image
    from yolov6.utils.synth import build_synthetic
    d = tmp_path_factory.mktemp('lookback')
    m = build_synthetic(CFG('yololps'), width=0.0625, sigma=1.5)
    torch.save({'model': m.half(), 'ema': None}, str(d / 'tiny.pt'))
    (d / 'imgs').mkdir()
    for k, f in enumerate(L.late_frames(10, 3)):
        Image.fromarray(f).save(str(d / 'imgs' / ('f%02d.png' % k)))
    return d


def test_infer_redact_lookback_tiled(late_dir, tmp_path, monkeypatch):
    """The tiled path: the redacted files are what PlateTrackerNp -> LookbackNp make of the same tiled run's untracked rows."""
    from PIL import Image
    from yolov6.data.datasets import imread_bgr
    from yolov6.utils.synth import build_synthetic
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    src, ckpt = late_dir / 'imgs', late_dir / 'tiny.pt'
    files = sorted(os.listdir(str(src)))
    kw = dict(weights=str(ckpt), source=str(src), yaml=None, img_size=[128, 160], conf_thres=0.06, iou_thres=0.45, max_det=5, device='0',
              not_save_img=True, half=True, tile=(96, 96), batch_size=8)
    plain = infer.run(save_dir=str(tmp_path / 'plain'), **kw)
    tkw = dict(track=True, track_max_age=2, track_iou=0.25, track_expand=0.25, redact='fill', redact_hold=True)
    held = infer.run(save_dir=str(tmp_path / 'held'), **tkw, **kw)
    back = infer.run(save_dir=str(tmp_path / 'back'), redact_lookback=4, **tkw, **kw)
    for a, b in zip(held, back):
        assert torch.equal(a, b)
    host = [np.ascontiguousarray(imread_bgr(str(src / f))) for f in files]
    m = build_synthetic(CFG('yololps'), width=0.0625, sigma=1.5)
    want = L.lookback_by_hand(host, [d.cpu().numpy() for d in plain], 5, 4, dict(mode='fill', margin=0.1), max_tracks=64, match_thres=0.25,
                              new_thres=0.0, expand=0.25, max_age=2, ncls=m)
    for k, w in enumerate(want):
        assert np.array_equal(np.asarray(Image.open(str(tmp_path / 'back' / 'redacted' / files[k]))), w[:, :, ::-1]), k


@pytest.mark.parametrize('run_kw', [dict(batch_size=1), dict(batch_size=8), dict(batch_size=8, nv12='bt709')], ids=['b1', 'b8', 'b8-nv12'])
def test_infer_redact_lookback_matches_numpy_on_detect_frames(late_dir, tmp_path, monkeypatch, run_kw):
    from PIL import Image
    from yolov6.core.inferer import Inferer
    from yolov6.data.datasets import imread_bgr
    from yolov6.hip import runtime
    from yolov6.utils.nv12 import Nv12Frame, bgr_to_nv12_np, nv12_to_bgr_np
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    src, ckpt, out = late_dir / 'imgs', late_dir / 'tiny.pt', tmp_path / 'out'
    files = sorted(os.listdir(str(src)))
    res = infer.run(weights=str(ckpt), source=str(src), yaml=None, img_size=[128, 160], conf_thres=0.06, iou_thres=0.45, max_det=5, device='0',
                    not_save_img=True, half=True, save_dir=str(out), track=True, track_max_age=2, track_iou=0.25, track_expand=0.25,
                    redact='fill', redact_hold=True, redact_lookback=4, **run_kw)
    model = Inferer(str(src), str(ckpt), '0', None, [128, 160], True).model.model
    host = [np.ascontiguousarray(imread_bgr(str(src / f))) for f in files]
    if 'nv12' in run_kw:
        host = [bgr_to_nv12_np(f, run_kw['nv12']) for f in host]
        frames = [Nv12Frame(torch.from_numpy(f.y).cuda(), torch.from_numpy(f.uv).cuda(), f.matrix) for f in host]
    else:
        frames = [torch.from_numpy(f).cuda() for f in host]
    with torch.no_grad():
        plain = runtime.detect_frames(model, frames, [128, 160], 0.06, 0.45, 5)
    kw = dict(max_tracks=64, match_thres=0.25, new_thres=0.0, expand=0.25, max_age=2, ncls=model)
    outs, _, _ = C.track_by_hand([d.cpu().numpy() for d in plain], 5, **kw)
    want = L.lookback_by_hand(host, [d.cpu().numpy() for d in plain], 5, 4, dict(mode='fill', margin=0.1), **kw)
    assert sorted(os.listdir(str(out / 'redacted'))) == files
    for k, (got, voted, w) in enumerate(zip(res, outs, want)):
        assert np.array_equal(got.cpu().numpy(), voted), k                      # the rows returned are the voted rows, as without the delay
        if 'nv12' in run_kw:
            w = nv12_to_bgr_np(w)
        png = np.asarray(Image.open(str(out / 'redacted' / files[k])))
        assert np.array_equal(png, w[:, :, ::-1]), k
