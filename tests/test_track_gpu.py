"""Plate tracking on the GPU: lp_track_update against its numpy specification bit for bit (yolov6/utils/track.py), the scene of
tests/test_track_cpu.py through runtime.PlateTracker, the steady state (no allocation, no host read: the update is captured
in a graph), and Inferer(track=True) against PlateTrackerNp on the same run's untracked detections."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
import test_track_cpu as C

pytestmark = pytest.mark.gpu
f32 = np.float32
CFG = lambda name: os.path.join(REPO, 'configs', name + '.py')   # noqa: E731


def _assert_call_equal(got, want, what):
    names = ('det_out', 'tid', 'ended_i', 'ended_f', 'ended_count')
    for name, g, w in zip(names, got, want):
        g = g.cpu().numpy()
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
        gi, wi = g.view(np.int32), np.ascontiguousarray(w).view(np.int32)
        if not np.array_equal(gi, wi):
            bad = np.argwhere(gi != wi)
            raise AssertionError('%s: %s differs in %d places, first at %s: got %r, want %r'
                                 % (what, name, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


def _run_both(calls, n_streams, max_ended, **kw):
    """The calls through runtime.PlateTracker (outputs poisoned before each call) and through PlateTrackerNp."""
    from yolov6.hip import runtime
    ref, outs = C.run_calls_np(calls, n_streams, max_ended, **kw)
    trk = runtime.PlateTracker(n_streams, device='cuda', **kw)
    for k, ((det, count, stream_of, flush), want) in enumerate(zip(calls, outs)):
        for buf in trk.buffers(det.shape[0], det.shape[1], max_ended):
            buf.fill_(float('nan') if buf.dtype == torch.float32 else -7)
        got = trk.update(torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda(), stream_of, flush, max_ended)
        _assert_call_equal(got, want, 'call %d' % k)
    assert np.array_equal(trk.dropped.cpu().numpy(), ref.dropped)
    assert not trk.state.view(n_streams, -1)[:, 16:].any()             # the last call flushes: every slot is all-zero again
    return ref


# (seed, n_streams, max_tracks, max_det, frames per call, objects per stream, extent, expand, max_age)
CASES = [
    (11, 1, 1, 5, (1, 3, 2, 4, 1, 2), 4, 300, 0.0, 0),
    (12, 3, 4, 5, (4, 1, 8, 3, 6, 2, 5), 6, 400, 0.5, 3),
    (13, 3, 4, 20, (8, 2, 5, 7, 1, 6, 3, 4), 8, 500, 0.0, 3),
    (14, 9, 16, 20, (70, 3, 66, 1, 9, 65), 8, 600, 0.5, 0),            # calls cross the 64-frame launch split
    (15, 3, 128, 128, (3, 2, 3, 1, 2, 3), 190, 2500, 0.5, 3),          # more rows than 128 slots; more objects than 128 rows
    (16, 1, 128, 300, (2, 1, 2, 2, 1, 2), 260, 3000, 0.0, 3),          # rows past 128 are copied untracked
    (17, 9, 1, 128, (9, 12, 1, 20, 5, 9), 5, 300, 0.5, 3),
]


@pytest.mark.parametrize('case', CASES, ids=lambda c: 's%d-t%d-d%d' % c[1:4])
def test_track_update_equals_numpy_spec(case):
    seed, S, T, max_det, Bs, n_obj, extent, expand, max_age = case
    calls = C.random_track_case(seed, n_streams=S, max_det=max_det, n_obj=n_obj, extent=extent, Bs=Bs)
    if max(Bs) > 64:                                                   # a stream has frames on both sides of a launch split
        so = calls[0][2]
        assert any(s >= 0 and s in so[:64] and s in so[64:] for s in range(S))
    ref = _run_both(calls, S, 6, max_tracks=T, match_thres=0.3, new_thres=0.2, expand=expand, max_age=max_age)
    assert ref.stats['matched'] > 0 and ref.stats['ended'] > 0
    if T <= 4:
        assert ref.dropped.sum() > 0
    if max_det >= 128 and T == 128:
        assert max(int(np.clip(c[1], 0, max_det).max()) for c in calls) > 120 and ref.dropped.sum() > 0
    if max_det == 300:
        assert max(int(np.clip(c[1], 0, max_det).max()) for c in calls) > 128


def test_track_update_full_matrix():
    """128 slots x 128 rows with every pair above the threshold: 16384 keys, the whole LDS list."""
    rng = np.random.default_rng(3)
    rows = [C.make_row((k % 7, k % 5, 1000 + k, 1000 + (k % 11)), ids=rng.integers(0, 24, 8), conf=(rng.integers(1, 9, 8) / 8.0)) for k in range(128)]
    frames = []
    for f in range(3):
        cur = [rows[i].copy() for i in rng.permutation(128)]
        for r in cur:
            r[0:4] += rng.integers(-2, 3, 4).astype(f32)
        frames.append(cur)
    det, count = C.frames_of(frames, 128)
    calls = [(det[:1], count[:1], [0], [0]), (det[1:], count[1:], [0, 0], [1])]
    ref = _run_both(calls, 1, 128, max_tracks=128, match_thres=0.3, new_thres=0.0, expand=0.5, max_age=0)
    assert ref.stats['pairs'] == 2 * 16384 and ref.stats['matched'] == 2 * 128 and ref.stats['ties'] > 0


def test_scene_through_runtime_tracker():
    from yolov6.hip import runtime
    rows_per_frame, truth, plates = C.plate_scene()
    trk = runtime.PlateTracker(1, max_tracks=8, match_thres=0.3, expand=0.5, max_age=C.SCENE_MAX_AGE, device='cuda')
    det, count = C.frames_of(rows_per_frame, 5)
    o, t, ei, ef, ec = trk.update(torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda(), stream_of=[0] * len(det), flush=[1])
    assert int(ec[0]) == 4
    ei, ef = ei.cpu().numpy(), ef.cpu().numpy()
    C.check_scene(list(o.cpu().numpy()), list(t.cpu().numpy()), [(ei[0, k], ef[0, k]) for k in range(4)], truth, plates)
    assert int(trk.dropped[0]) == 0


def test_steady_state_no_allocation_and_graph_capture():
    """Ten updates with persistent buffers allocate nothing after the first; the update performs no host read: it is captured
    in a graph (a host read during capture is an error) and the replays match the specification."""
    from yolov6.hip import runtime
    from yolov6.utils.track import PlateTrackerNp
    calls = C.random_track_case(21, n_streams=4, max_det=20, Bs=(4,) * 12)
    kw = dict(max_tracks=8, match_thres=0.3, new_thres=0.2, expand=0.5, max_age=2)
    trk, ref = runtime.PlateTracker(4, device='cuda', **kw), PlateTrackerNp(4, **kw)
    det = torch.from_numpy(calls[0][0]).cuda()
    count = torch.from_numpy(calls[0][1]).cuda()
    stream_of = [0, 1, 3, 1]
    trk.update(det, count, stream_of)
    want = ref.update(calls[0][0], calls[0][1], stream_of)
    torch.cuda.synchronize()
    for k in range(1, 10):
        det.copy_(torch.from_numpy(calls[k][0]))
        count.copy_(torch.from_numpy(calls[k][1]))
        after_copy = torch.cuda.memory_stats()['allocation.all.allocated']
        got = trk.update(det, count, stream_of)
        assert torch.cuda.memory_stats()['allocation.all.allocated'] == after_copy
        want = ref.update(calls[k][0], calls[k][1], stream_of)
    _assert_call_equal(got, want, 'call 9')
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = trk.update(det, count, stream_of)
    for k in (10, 11):                                                 # new rows, same buffers; the state moves on with every replay
        det.copy_(torch.from_numpy(calls[k][0]))
        count.copy_(torch.from_numpy(calls[k][1]))
        for buf in got:
            buf.fill_(float('nan') if buf.dtype == torch.float32 else -7)
        g.replay()
        torch.cuda.synchronize()
        _assert_call_equal(got, ref.update(calls[k][0], calls[k][1], stream_of), 'replay %d' % k)


# ---- Inferer(track=True) -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def video_dir(tmp_path_factory):
    from PIL import Image
    from yolov6.utils.synth import build_synthetic
    d = tmp_path_factory.mktemp('track')
    m = build_synthetic(CFG('yololps'), width=0.0625, sigma=1.5)
    torch.save({'model': m.half(), 'ema': None}, str(d / 'tiny.pt'))
    (d / 'imgs').mkdir()
    (d / 'big').mkdir()
    for k, f in enumerate(C._moving_frames(10)):
        Image.fromarray(f).save(str(d / 'imgs' / ('f%02d.png' % k)))
    for k, f in enumerate(C._moving_frames(4, h=200, w=300, seed=9)):
        Image.fromarray(f).save(str(d / 'big' / ('f%02d.png' % k)))
    return d


def _check_infer(video_dir, tmp_path, sub, size, max_det, untracked, **run_kw):
    """infer.run(track=True, save_crops=True) against PlateTrackerNp on ``untracked(model, frames)``'s detections."""
    from yolov6.core.inferer import Inferer
    from yolov6.data.datasets import imread_bgr
    from yolov6.hip import runtime
    from PIL import Image
    infer = importlib.import_module('infer')
    src, ckpt = video_dir / sub, video_dir / 'tiny.pt'
    files = sorted(os.listdir(str(src)))
    out = tmp_path / 'out'
    res = infer.run(weights=str(ckpt), source=str(src), yaml=None, img_size=size, conf_thres=0.06, iou_thres=0.45, max_det=max_det,
                    device='0', save_txt=True, not_save_img=True, half=True, save_dir=str(out), track=True, track_max_age=2,
                    track_iou=0.25, track_expand=0.25, save_crops=True, crop_size=(16, 48), **run_kw)
    model = Inferer(str(src), str(ckpt), '0', None, size, True).model.model          # the checkpoint as Inferer prepares it
    frames = [torch.from_numpy(np.ascontiguousarray(imread_bgr(str(src / f)))).cuda() for f in files]
    with torch.no_grad():
        plain = untracked(runtime, model, frames)
    outs, tids, ended = C.track_by_hand([d.cpu().numpy() for d in plain], max_det, max_tracks=64, match_thres=0.25, new_thres=0.0,
                                        expand=0.25, max_age=2, ncls=model)
    assert len(res) == len(files) and sum(len(d) for d in plain) >= len(files)
    for k, (got, want) in enumerate(zip(res, outs)):
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), want), k
        if len(want):
            count = torch.tensor([len(want)], dtype=torch.int32, device='cuda')
            crops, _ = runtime.plate_crops([frames[k]], torch.from_numpy(want).cuda()[None], count, (16, 48), max_crops=len(want))
            for r in range(len(want)):
                png = np.asarray(Image.open(str(out / sub / 'crops' / ('%s_%d.png' % (files[k][:-4], r)))))
                assert np.array_equal(png, crops[0, r].cpu().numpy()[:, :, ::-1])
    want = ['%s %d %d' % (str(src / files[k]), r, t) for k in range(len(files)) for r, t in enumerate(tids[k].tolist())]
    assert (out / 'tracks.txt').read_text().splitlines() == want
    assert (out / 'plates.txt').read_text().splitlines() == C.plate_lines(ended)
    assert len(ended) >= 1 and max(int(ri[3]) for ri, _ in ended) >= 2


@pytest.mark.parametrize('batch_size', [1, 8])
def test_infer_track_matches_numpy_on_detect_frames(video_dir, tmp_path, monkeypatch, batch_size):
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    _check_infer(video_dir, tmp_path, 'imgs', [128, 160], 20,
                 lambda rt, model, frames: rt.detect_frames(model, frames, [128, 160], 0.06, 0.45, 20), batch_size=batch_size)


def test_infer_track_tiled_matches_numpy_on_detect_tiled(video_dir, tmp_path, monkeypatch):
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    _check_infer(video_dir, tmp_path, 'big', [128, 128], 50,
                 lambda rt, model, frames: rt.detect_tiled(model, frames, [128, 128], 0.06, 0.45, 50, tile_hw=(128, 128), overlap=32, batch=8),
                 batch_size=8, tile=[128, 128], tile_overlap=32)
