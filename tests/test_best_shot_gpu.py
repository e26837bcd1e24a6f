"""The best shot of every plate track on the GPU, everything bit for bit against the numpy specification
(yolov6/utils/best_shot.py, yolov6/utils/track.py): lp_track_update_slots, lp_crop_sharpness, lp_best_shot_update over the
multi-call cases of tests/test_best_shot_cpu.py, PlateTracker.update_with_shots in the steady state (no allocation, captured in
a graph) and Inferer(track=True, best_shots=True) on its three GPU paths.  Every output is poisoned before each call."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
import test_track_cpu as C
import test_best_shot_cpu as S
import test_streams_cpu as U
from test_track_gpu import CASES, CFG, _assert_call_equal, video_dir   # noqa: F401  (video_dir: the fixture)

pytestmark = pytest.mark.gpu
f32 = np.float32


def _poison(*bufs):
    for buf in bufs:
        buf.fill_(float('nan') if buf.dtype == torch.float32 else (0xAB if buf.dtype == torch.uint8 else -7))


def _bits_equal(got, want, what):
    g = got.cpu().numpy()
    w = np.ascontiguousarray(want)
    if w.dtype == np.uint64:
        g = g.view(np.uint64)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, g.dtype, w.shape, w.dtype)
    gi, wi = g.view(np.uint8), w.view(np.uint8)
    if not np.array_equal(gi, wi):
        bad = np.argwhere(g.view(np.int32 if g.dtype.itemsize == 4 else g.dtype) != w.view(np.int32 if w.dtype.itemsize == 4 else w.dtype))
        raise AssertionError('%s differs in %d places, first at %s: got %r, want %r'
                             % (what, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


def _assert_shots_equal(got, want, what):
    for name, g, w in zip(('shot_crops', 'shot_i', 'shot_q', 'shot_det'), got, want):
        _bits_equal(g, w, '%s: %s' % (what, name))


# ---- lp_track_update_slots ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [c for c in CASES if c[0] in (12, 14, 15)], ids=lambda c: 's%d-t%d-d%d' % c[1:4])
def test_track_update_slots_equals_numpy_last_slot(case):
    """The slot output against PlateTrackerNp.last_slot, the five old outputs unchanged; lp_track_update itself (the call with a
    null slot pointer) on a second state gives the same five."""
    from yolov6.hip import abi, runtime
    from yolov6.utils.track import PlateTrackerNp
    seed, n_streams, T, max_det, Bs, n_obj, extent, expand, max_age = case
    calls = C.random_track_case(seed, n_streams=n_streams, max_det=max_det, n_obj=n_obj, extent=extent, Bs=Bs)
    kw = dict(max_tracks=T, match_thres=0.3, new_thres=0.2, expand=expand, max_age=max_age)
    ref, trk, old = PlateTrackerNp(n_streams, **kw), runtime.PlateTracker(n_streams, device='cuda', **kw), runtime.PlateTracker(n_streams, device='cuda', **kw)
    lib, seen = abi.load(), 0
    for k, (det, count, stream_of, flush) in enumerate(calls):
        B = len(det)
        want = ref.update(det, count, stream_of, flush, 6)
        _poison(trk.slot_buffer(B, max_det), *trk.buffers(B, max_det, 6))
        d, c = torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda()
        got = trk.update(d, c, stream_of, flush, 6)
        _assert_call_equal(got, want, 'call %d' % k)
        _bits_equal(trk.slot_buffer(B, max_det), ref.last_slot, 'call %d: slot' % k)
        seen += int((ref.last_slot >= 0).sum())
        out = old.buffers(B, max_det, 6)
        _poison(*out)
        so, fl = (ctypes.c_int * max(B, 1))(*stream_of), (ctypes.c_ubyte * n_streams)(*flush)
        with torch.cuda.device(old.device):
            abi.check(lib.lp_track_update(old.state.data_ptr(), n_streams, T, ctypes.byref(old._params), d.data_ptr(), c.data_ptr(), B, max_det,
                                          so, ctypes.cast(fl, ctypes.c_void_p), *(t.data_ptr() for t in out), 6,
                                          runtime._stream_ptr(old.device)), 'lp_track_update')
        _assert_call_equal(out, want, 'call %d (lp_track_update)' % k)
    assert seen > 0 and ref.stats['ended'] > 0
    assert torch.equal(trk.state, old.state)


# ---- lp_crop_sharpness -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', [(1, 1), (2, 5), (3, 3), (5, 7), (7, 9), (64, 192), (40, 1000)], ids=lambda hw: '%dx%d' % hw)
def test_crop_sharpness_equals_numpy(hw):
    """Random crops with a status from 0..3; 5x7 and 7x9 slots are 105 and 189 bytes, so their slots start at every alignment
    (the byte path and the dword path of the loader); 40x1000 takes two bands of rows."""
    from yolov6.hip import runtime
    from yolov6.utils.best_shot import crop_sharpness_np
    rng = np.random.default_rng(hw[0] * 1000 + hw[1])
    crops = rng.integers(0, 256, (3, 3) + hw + (3,), dtype=np.uint8)
    status = np.array([[0, 1, 2], [3, 1, 2], [2, 1, 1]], np.int32)
    want = crop_sharpness_np(crops, status)
    assert (want > 0).sum() == (7 if min(hw) >= 3 else 0)
    out = torch.empty(3, 3, dtype=torch.int64, device='cuda')
    _poison(out)
    got = runtime.crop_sharpness(torch.from_numpy(crops).cuda(), torch.from_numpy(status).cuda(), out=out)
    assert got is out
    _bits_equal(got, want, 'sharp %dx%d' % hw)


def test_crop_sharpness_checkerboard_exceeds_32_bits():
    from yolov6.hip import runtime
    cb = np.stack([S.checkerboard(), 255 - S.checkerboard(), np.full((64, 192, 3), 93, np.uint8)])
    got = runtime.crop_sharpness(torch.from_numpy(cb).cuda(), torch.tensor([1, 2, 1], dtype=torch.int32, device='cuda'))
    assert got.cpu().tolist() == [S.CHECKER_64x192, S.CHECKER_64x192, 0] and S.CHECKER_64x192 > 2 ** 32


# ---- lp_best_shot_update -----------------------------------------------------------------------------------------------------
def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def _run_shot_calls(calls, n_streams, T, max_det, crop_hw, max_crops, max_ended, min_score):
    """The calls of ``shot_case`` through lp_best_shot_update, every output bit for bit; returns the device state."""
    from yolov6.hip import abi, runtime
    lib, dev = abi.load(), torch.device('cuda', torch.cuda.current_device())
    state = torch.zeros(lib.lp_best_shot_state_bytes(n_streams, T, *crop_hw), dtype=torch.uint8, device=dev)
    out = (torch.empty((n_streams, max_ended) + crop_hw + (3,), dtype=torch.uint8, device=dev),
           torch.empty(n_streams, max_ended, 4, dtype=torch.int32, device=dev),
           torch.empty(n_streams, max_ended, dtype=torch.int64, device=dev),
           torch.empty(n_streams, max_ended, 28, dtype=torch.float32, device=dev))
    for k, (inp, want) in enumerate(calls):
        B = len(inp['det'])
        t = {name: _dev(inp[name]) for name in ('det', 'count', 'tid', 'slot', 'crops', 'status', 'sharp', 'ended_i', 'ended_count')}
        so = (ctypes.c_int * max(B, 1))(*inp['stream_of'])
        _poison(*out)
        with torch.cuda.device(dev):
            abi.check(lib.lp_best_shot_update(state.data_ptr(), n_streams, T, crop_hw[0], crop_hw[1], t['det'].data_ptr(), t['count'].data_ptr(),
                                              B, max_det, t['tid'].data_ptr(), t['slot'].data_ptr(), t['crops'].data_ptr(),
                                              t['status'].data_ptr(), t['sharp'].data_ptr(), max_crops, so, t['ended_i'].data_ptr(),
                                              t['ended_count'].data_ptr(), max_ended, min_score, *(o.data_ptr() for o in out),
                                              runtime._stream_ptr(dev)), 'lp_best_shot_update')
        _assert_shots_equal(out, want, 'call %d' % k)       # (want's crops of records without a shot hold the poison 0xAB)
    return state


@pytest.mark.parametrize('case', S.SHOT_CASES, ids=S.SHOT_IDS)
def test_best_shot_update_equals_numpy_spec(case):
    seed, n_streams, T, max_det, Bs, crop_hw, max_crops, max_ended, kw = case
    gal, calls = S.shot_case(seed, n_streams, T, max_det, Bs, crop_hw, max_crops, max_ended, **kw)
    S.check_shot_case(case, gal, calls)                     # what the case is there for happened
    state = _run_shot_calls(calls, n_streams, T, max_det, crop_hw, max_crops, max_ended, gal.min_score)
    # the last call flushes every stream and nothing was cut off in it, or what is left are entries whose records were cut off:
    # either way the numpy gallery and the device state agree on which entries are occupied
    words = state.view(n_streams, -1)[:, 16:].view(n_streams, T, -1)[:, :, :4].contiguous().view(torch.int32)[:, :, 0].cpu().numpy()
    assert np.array_equal(words, gal.idp1)


def test_a_launch_of_untracked_frames_only_launches_nothing_for_it():
    """The first launch of call 1 holds untracked frames only and call 2 nothing else: no workgroup; the track that call 2's flush
    ends is retired by the closing kernel.  The state is compared field by field (the crop and the det row of an entry with a
    shot; a retired entry keeps what it held)."""
    crop_hw, max_ended = (5, 7), 4
    n_streams, T, max_det = U.UL['n_streams'], U.UL['max_tracks'], U.UL['max_det']
    gal, calls = U.untracked_launch_shots(crop_hw, max_ended)
    state = _run_shot_calls(calls, n_streams, T, max_det, crop_hw, max_det, max_ended, gal.min_score).cpu().view(n_streams, -1)
    assert np.array_equal(state[:, :4].contiguous().view(torch.int32)[:, 0].numpy(), gal.frame) and gal.frame.tolist() == [1, 1]
    entries = state[:, 16:].view(n_streams, T, -1)
    head = entries[:, :, :144].contiguous().view(torch.int32).numpy()
    assert np.array_equal(head[:, :, 0], gal.idp1) and np.array_equal(head[:, :, 1], gal.has) and gal.has.sum() == 1
    for s, g in np.argwhere(gal.has):
        assert np.array_equal(head[s, g, 2:4].view(np.uint64)[0], gal.key[s, g]) and np.array_equal(head[s, g, 4:7], gal.meta[s, g])
        assert np.array_equal(head[s, g, 8:36], gal.det[s, g].view(np.int32))
        assert np.array_equal(entries[s, g, 144:144 + gal.crop[s, g].size].numpy(), gal.crop[s, g].reshape(-1))


# ---- PlateTracker.update_with_shots ---------------------------------------------------------------------------------------------
def test_update_with_shots_steady_state_and_graph_capture():
    """Tracker -> crops -> sharpness -> gallery through runtime.PlateTracker: ten calls allocate nothing after the first, the
    chain performs no host read (it is captured in a graph) and two replays match the specification."""
    from yolov6.hip import runtime
    from yolov6.utils.best_shot import BestShotNp
    from yolov6.utils.track import PlateTrackerNp
    n_streams, max_det, max_crops, crop_hw = 4, 20, 6, (8, 24)
    calls = C.random_track_case(21, n_streams=n_streams, max_det=max_det, extent=150, Bs=(4,) * 12)
    kw = dict(max_tracks=8, match_thres=0.3, new_thres=0.2, expand=0.5, max_age=2)
    trk, ref = runtime.PlateTracker(n_streams, device='cuda', **kw), PlateTrackerNp(n_streams, **kw)
    trk.enable_best_shot(crop_hw, max_crops=max_crops, min_score=0.2)
    gal = BestShotNp(n_streams, 8, crop_hw, 0.2)
    rng = np.random.default_rng(7)
    frames_np = [rng.integers(0, 256, (170 + 3 * b, 220 - 5 * b, 3), dtype=np.uint8) for b in range(4)]
    frames = [torch.from_numpy(f).cuda() for f in frames_np]
    stream_of = [0, 1, 3, 1]
    det, count = torch.from_numpy(calls[0][0]).cuda(), torch.from_numpy(calls[0][1]).cuda()
    shot_crops_np = np.zeros((n_streams, 8) + crop_hw + (3,), np.uint8)     # persistent, like the device buffer

    def spec(k):
        for f in frames_np:
            f[:] = np.roll(f, 3, axis=1)                    # the scene moves: every call sees other pixels
        out = ref.update(calls[k][0], calls[k][1], stream_of)
        return out + gal.update_from_frames(frames_np, calls[k][0], calls[k][1], out[1], ref.last_slot, stream_of, out[2], out[4],
                                            max_crops, shot_crops=shot_crops_np)

    def load(k):
        det.copy_(torch.from_numpy(calls[k][0]))
        count.copy_(torch.from_numpy(calls[k][1]))
        for f, fn in zip(frames, frames_np):
            f.copy_(torch.from_numpy(fn))

    def compare(got, want, what):
        _assert_call_equal(got[:5], want[:5], what)
        _assert_shots_equal(got[5:], want[5:], what)

    want = spec(0)
    load(0)
    compare(trk.update_with_shots(frames, det, count, stream_of), want, 'call 0')
    torch.cuda.synchronize()
    for k in range(1, 10):
        want = spec(k)
        load(k)
        before = torch.cuda.memory_stats()['allocation.all.allocated']
        got = trk.update_with_shots(frames, det, count, stream_of)
        assert torch.cuda.memory_stats()['allocation.all.allocated'] == before
        compare(got, want, 'call %d' % k)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = trk.update_with_shots(frames, det, count, stream_of)
    # capture enqueued nothing: the first replay is call 10
    for k in (10, 11):
        _poison(*got, *trk.shot_buffers(4)[:3], trk.slot_buffer(4, max_det))
        shot_crops_np[:] = 0xAB
        want = spec(k)
        load(k)
        g.replay()
        torch.cuda.synchronize()
        compare(got, want, 'replay %d' % k)
    assert gal.stats['taken'] > 0 and gal.stats['replaced'] > 0 and gal.stats['with_shot'] > 0 and ref.stats['ended'] > 0
    # flush: every live track ends and hands out its shot; the gallery is empty afterwards; reset zeroes both states
    shot_crops_np[:] = 0xAB
    _poison(*trk.shot_buffers(0))
    out = ref.flush_all()
    want = out + gal.update_from_frames([], np.zeros((0, 1, 28), f32), [], out[1], ref.last_slot, [], out[2], out[4], max_crops,
                                        shot_crops=shot_crops_np)
    compare(trk.flush_all_with_shots(), want, 'flush')
    assert int(want[4].sum()) > 0 and not gal.idp1.any()
    trk.update_with_shots(frames, det, count, stream_of)
    assert trk.state.any() and trk._shots['state'].any()
    trk.reset([0, 1])
    assert trk._shots['state'].view(n_streams, -1)[3].any() and not trk._shots['state'].view(n_streams, -1)[:2].any()
    trk.reset()
    assert not trk.state.any() and not trk._shots['state'].any()


# ---- Inferer(track=True, best_shots=True) -----------------------------------------------------------------------------------------
def _check_infer_shots(video_dir, tmp_path, sub, size, max_det, untracked, **run_kw):
    """infer.run(track=True, best_shots=True) against PlateTrackerNp + plate_crops_np + BestShotNp (the CPU path's chain) on
    ``untracked(runtime, model, frames)``'s detections."""
    from yolov6.core.inferer import Inferer
    from yolov6.data.datasets import imread_bgr
    from yolov6.hip import runtime
    infer = importlib.import_module('infer')
    src, ckpt = video_dir / sub, video_dir / 'tiny.pt'
    files = sorted(os.listdir(str(src)))
    out = tmp_path / 'out'
    res = infer.run(weights=str(ckpt), source=str(src), yaml=None, img_size=size, conf_thres=0.06, iou_thres=0.45, max_det=max_det,
                    device='0', save_txt=True, not_save_img=True, half=True, save_dir=str(out), track=True, track_max_age=2,
                    track_iou=0.25, track_expand=0.25, best_shots=True, crop_size=(16, 48), **run_kw)
    model = Inferer(str(src), str(ckpt), '0', None, size, True).model.model          # the checkpoint as Inferer prepares it
    frames_np = [np.ascontiguousarray(imread_bgr(str(src / f))) for f in files]
    with torch.no_grad():
        plain = untracked(runtime, model, [torch.from_numpy(f).cuda() for f in frames_np])
    assert len(res) == len(files) and sum(len(d) for d in plain) >= len(files)
    ended, shots = S.shots_by_hand(frames_np, [d.cpu().numpy() for d in plain], max_det, (16, 48), max_crops=Inferer.SHOT_ROWS,
                                   max_tracks=64, match_thres=0.25, new_thres=0.0, expand=0.25, max_age=2, ncls=model)
    assert S.check_shot_files(out, ended, shots) >= 1


@pytest.mark.parametrize('batch_size', [1, 8])
def test_infer_best_shots_matches_the_cpu_chain(video_dir, tmp_path, monkeypatch, batch_size):   # noqa: F811
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    _check_infer_shots(video_dir, tmp_path, 'imgs', [128, 160], 20,
                       lambda rt, model, frames: rt.detect_frames(model, frames, [128, 160], 0.06, 0.45, 20), batch_size=batch_size)


def test_infer_best_shots_tiled_matches_the_cpu_chain(video_dir, tmp_path, monkeypatch):   # noqa: F811
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    _check_infer_shots(video_dir, tmp_path, 'big', [128, 128], 50,
                       lambda rt, model, frames: rt.detect_tiled(model, frames, [128, 128], 0.06, 0.45, 50, tile_hw=(128, 128), overlap=32, batch=8),
                       batch_size=8, tile=[128, 128], tile_overlap=32)
