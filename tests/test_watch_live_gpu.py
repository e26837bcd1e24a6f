"""The live-track watchlist lookup on the GPU: lp_watch_live against its numpy specification (yolov6/utils/watch_live.py) on every
int32 of every output -- slot counts from one to both waves of the numbering, head widths at their limits, list lengths around the
scan's workgroup, streams that are never fed, flushed half way or fed twice a call --, a full house of 128 fresh reads, the head read
against what the tracker wrote into det_out (one function reads both: track_read_head), more streams than the prefix kernel has threads, the steady state (no allocation, no host read:
captured in a graph behind the tracker), PlateTracker.enable_live_watch against PlateTrackerNp.enable_live_watch, and
Inferer(watch_live=True) against the CPU computation on the same detections."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
import test_track_cpu as T
import test_watch_cpu as C
import test_watch_live_cpu as L

pytestmark = pytest.mark.gpu
f32 = np.float32
POISON = -77
CFG = lambda name: os.path.join(REPO, 'configs', name + '.py')   # noqa: E731
WIDE = (1, 64) + (37,) * 6


def outputs_gpu(trk):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (trk.last_live,) + tuple(trk.last_live_reads) + (trk.live_memo,))


def poison(trk):
    """Everything lp_watch_live writes but the memo, and its workspace, may hold anything on entry."""
    lw = trk._live
    for name in ('live_i', 'q_i', 'q_slot', 'q_count'):
        lw[name].fill_(POISON)
    lw['q_f'].fill_(float('nan'))
    lw['ws'].fill_(0x5A)


def live_calls(seed, ncls, n_obj, max_det, n_calls=12):
    """``n_calls`` update calls on five streams: stream 0 has one frame a call, stream 1 two, stream 2 one and is flushed half way,
    stream 3 a frame every other call, stream 4 none ever.  Objects drift with integer velocities, are born and die, are missed in
    15 % of their frames, and a fifth of their ids is noise, so that voted reads change while a track lives; confidences are
    eighths, 0 included."""
    rng = np.random.default_rng(seed)
    objs = [[] for _ in range(4)]

    def rows_of(s):
        live = objs[s]
        live[:] = [o for o in live if rng.random() > 0.05]
        empty = not live                                                        # an empty stream fills up at once
        for _ in range(n_obj - len(live)):
            if not empty and rng.random() < 0.5:
                continue
            k = len(live) + int(rng.integers(0, 1000)) * n_obj
            live.append(dict(x=(k % 12) * 150 + int(rng.integers(0, 20)), y=(k // 12 % 12) * 60, vx=int(rng.integers(-3, 4)), vy=int(rng.integers(-1, 2)),
                             ids=[int(rng.integers(0, n)) for n in ncls]))
        rows = []
        for o in live:
            o['x'] += o['vx']
            o['y'] += o['vy']
            if rng.random() < 0.15:
                continue
            ids = [i if rng.random() < 0.8 else int(rng.integers(0, n)) for i, n in zip(o['ids'], ncls)]
            rows.append(T.make_row((o['x'], o['y'], o['x'] + 80, o['y'] + 25), ids, (rng.integers(0, 9, 8) / 8.0).astype(f32)))
        return rows[:max_det]

    calls = []
    for c in range(n_calls):
        stream_of = [1, 0, 2, 1] + ([3] if c % 2 == 0 else [])
        det, count = T.frames_of([rows_of(s) for s in stream_of], max_det)
        calls.append((det, count, stream_of, [0, 0, int(c == n_calls // 2), 0, 0]))
    return calls


# ---- kernel == specification, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('min_hits', [1, 3])
@pytest.mark.parametrize('N', [0, 1, 2049])
@pytest.mark.parametrize('ncls', [T.NCLS, WIDE], ids=['shipped', 'wide'])
@pytest.mark.parametrize('max_tracks', [1, 8, 17, 64, 65, 128])     # 17: the gather workgroup passes 128 threads; 65: a slot in the second wave
def test_watch_live_equals_numpy_spec(max_tracks, ncls, N, min_hits):
    from yolov6.hip import runtime
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.watch import WatchlistNp
    n_obj, max_det = min(max_tracks + 2, 70), 80
    kw = dict(max_tracks=max_tracks, match_thres=0.3, new_thres=0.2, expand=0.25, max_age=2, ncls=ncls)
    calls = live_calls(max_tracks, ncls, n_obj, max_det)
    entries = L.live_list_for(calls, 5, N, 3, min_hits, **kw)
    confuse = C.random_confuse(np.random.default_rng(4))
    trk, ref = runtime.PlateTracker(5, device='cuda', **kw), PlateTrackerNp(5, **kw)
    trk.enable_live_watch(runtime.Watchlist(entries, confuse), min_hits, max_mismatch=2, max_cost=1.5)
    ref.enable_live_watch(WatchlistNp(entries, confuse), min_hits, max_mismatch=2, max_cost=1.5)
    seen = dict(fresh=0, standing=0, hits=0, second_wave=0)
    for k, (det, count, stream_of, flush) in enumerate(calls):
        poison(trk)
        trk.update(torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda(), stream_of, flush)
        ref.update(det, count, stream_of, flush)
        got, want = outputs_gpu(trk), L.outputs_np(ref)
        L.assert_same(got, want, 'T %d, N %d, min_hits %d, call %d' % (max_tracks, N, min_hits, k))
        live_i = want[0]
        seen['fresh'] += int(want[4].sum())
        seen['standing'] += int(((live_i[:, :, 0] >= 0) & (live_i[:, :, 5] == 0)).sum())
        seen['hits'] += int((live_i[:, :, 1] >= 0).sum())
        seen['second_wave'] += int((live_i[:, 64:, 5] == 1).sum())
        assert not want[5][4].any() and (live_i[4] == L.NO_ROW).all() and want[4][4] == 0       # the stream that is never fed
        if k == len(calls) // 2:
            assert not want[5][2].any() and seen['fresh'] > 0                                     # the stream flushed in this call
    assert seen['fresh'] > 0 and seen['standing'] > 0 and (seen['hits'] > 0) == (N > 0), seen
    assert (seen['second_wave'] > 0) == (max_tracks > 64), seen


def test_a_full_house_of_128_fresh_reads_then_none():
    """T = 128, min_hits = 1, 128 separated detections in one frame: eight query blocks of the scan at once; the same frame again
    brings no query, and every row keeps its entry."""
    from yolov6.hip import runtime
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.watch import WatchlistNp
    rng = np.random.default_rng(8)
    rows = [T.make_row((150 * (k % 16), 60 * (k // 16), 150 * (k % 16) + 80, 60 * (k // 16) + 25), [int(rng.integers(0, n)) for n in T.NCLS], 0.75)
            for k in range(128)]
    det, count = T.frames_of([rows], 128)
    entries = C.random_entries(rng, 300, n_ids=37, wild=0.0, nothing=0.0)
    where = rng.permutation(300)[:128]
    entries[where] = det[0, :, 20:28].astype(np.uint8)                          # every read is on the list, somewhere
    kw = dict(max_tracks=128, new_thres=0.2, max_age=2)
    trk, ref = runtime.PlateTracker(1, device='cuda', **kw), PlateTrackerNp(1, **kw)
    trk.enable_live_watch(runtime.Watchlist(entries), min_hits=1, max_mismatch=0)
    ref.enable_live_watch(WatchlistNp(entries), min_hits=1, max_mismatch=0)
    d, c = torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda()
    for k in range(2):
        poison(trk)
        trk.update(d, c)
        ref.update(det, count)
        got = outputs_gpu(trk)
        L.assert_same(got, L.outputs_np(ref), 'call %d' % k)
        live_i, _, _, q_slot, q_count, _ = got
        assert q_count.tolist() == [128 if k == 0 else 0]
        assert live_i[0, :, 0].tolist() == list(range(128)) and (live_i[0, :, 5] == 1 - k).all() and (live_i[0, :, 6] == k + 1).all()
        assert (entries[live_i[0, :, 1]] == det[0, :, 20:28]).all() and (live_i[0, :, 4] >= 1).all()
        assert q_slot[0].tolist() == (list(range(128)) if k == 0 else [-1] * 128)


def test_the_head_read_is_the_trackers_own():
    """For every row of an update with tid >= 0 whose track is fresh in that call, the shares and ids of its query line are the
    columns 12..19 and 20..27 the tracker wrote for the row, bit for bit (one frame per stream and call: det_out is read after the
    frame's vote, which is the state the lookup sees)."""
    from yolov6.hip import runtime
    kw = dict(max_tracks=64, match_thres=0.3, new_thres=0.2, expand=0.25, max_age=2, ncls=WIDE)
    calls = live_calls(77, WIDE, 40, 64)
    trk = runtime.PlateTracker(5, device='cuda', **kw)
    trk.enable_live_watch(runtime.Watchlist(C.random_entries(np.random.default_rng(1), 50, n_ids=37, nothing=0.0)), min_hits=1)
    checked = 0
    for det, count, stream_of, flush in calls:
        keep = [b for b, s in enumerate(stream_of) if s != 1]                    # stream 1 has two frames a call: leave it out
        det, count, stream_of = det[keep], count[keep], [stream_of[b] for b in keep]
        det_out, tid = trk.update(torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda(), stream_of)[:2]
        slot = trk.slot_buffer(*det.shape[:2])
        torch.cuda.synchronize()
        det_out, tid, slot = det_out.cpu().numpy(), tid.cpu().numpy(), slot.cpu().numpy()
        live_i, q_i, q_f, q_slot, q_count, _ = outputs_gpu(trk)
        for b, s in enumerate(stream_of):
            for r in np.nonzero(tid[b] >= 0)[0]:
                t = int(slot[b, r])
                assert live_i[s, t, 0] == tid[b, r]
                if live_i[s, t, 5] == 1:
                    j = int(np.nonzero(q_slot[s] == t)[0][0])
                    assert j < q_count[s] and q_i[s, j, 0] == tid[b, r]
                    assert np.array_equal(q_f[s, j, :8].view(np.int32), det_out[b, r, 12:20].view(np.int32))
                    assert np.array_equal(q_i[s, j, 4:], det_out[b, r, 20:28].astype(np.int32))
                    assert np.array_equal(q_f[s, j, 8:].view(np.int32), det_out[b, r, 0:4].view(np.int32))
                    checked += 1
    assert checked > 100


def test_1500_streams():
    """More streams than the prefix kernel of lp_watch_match has threads; T = 8."""
    from yolov6.hip import runtime
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.watch import WatchlistNp
    rng = np.random.default_rng(9)
    S = 1500
    kw = dict(max_tracks=8, new_thres=0.2, max_age=2)
    entries = C.random_entries(rng, 300, n_ids=4, nothing=0.0)
    trk, ref = runtime.PlateTracker(S, device='cuda', **kw), PlateTrackerNp(S, **kw)
    trk.enable_live_watch(runtime.Watchlist(entries), min_hits=1, max_mismatch=2, max_cost=1.0)
    ref.enable_live_watch(WatchlistNp(entries), min_hits=1, max_mismatch=2, max_cost=1.0)
    n_rows = rng.integers(0, 4, S)
    for k in range(2):
        rows = [[T.make_row((150 * r, 0, 150 * r + 80, 25), rng.integers(0, 4, 8), 0.5) for r in range(n)] for n in n_rows]
        det, count = T.frames_of(rows, 4)
        poison(trk)
        trk.update(torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda())
        ref.update(det, count)
        got = outputs_gpu(trk)
        L.assert_same(got, L.outputs_np(ref), 'call %d' % k)
        assert got[4].sum() > (800 if k == 0 else 100) and (got[0][:, :, 1] >= 0).sum() > 100


# ---- behind the tracker ------------------------------------------------------------------------------------------------------------------
KW = dict(max_tracks=8, match_thres=0.3, new_thres=0.2, expand=0.5, max_age=2)


def _assert_equal(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        g = g.cpu().numpy()
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g.view(np.int32), np.ascontiguousarray(w).view(np.int32)), (what, k)


def test_steady_state_no_allocation_and_graph_capture():
    """Ten updates with the live watch enabled allocate nothing after the first; tracker and lookup perform no host read: they are
    captured in one graph (a single chain on one stream) and the replays match the specification."""
    from yolov6.hip import runtime
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.watch import WatchlistNp
    calls = T.random_track_case(21, n_streams=4, max_det=20, Bs=(4,) * 12)
    entries = L.live_list_for(calls, 4, 100, 0, 2, **KW)
    confuse = C.random_confuse(np.random.default_rng(1))
    trk, ref = runtime.PlateTracker(4, device='cuda', **KW), PlateTrackerNp(4, **KW)
    trk.enable_live_watch(runtime.Watchlist(entries, confuse), min_hits=2, max_mismatch=2, max_cost=2.5)
    ref.enable_live_watch(WatchlistNp(entries, confuse), min_hits=2, max_mismatch=2, max_cost=2.5)
    det = torch.from_numpy(calls[0][0]).cuda()
    count = torch.from_numpy(calls[0][1]).cuda()
    stream_of = [0, 1, 3, 1]
    trk.update(det, count, stream_of)
    ref.update(calls[0][0], calls[0][1], stream_of)
    torch.cuda.synchronize()
    fresh = 0
    for k in range(1, 10):
        det.copy_(torch.from_numpy(calls[k][0]))
        count.copy_(torch.from_numpy(calls[k][1]))
        after_copy = torch.cuda.memory_stats()['allocation.all.allocated']
        got = trk.update(det, count, stream_of)
        assert torch.cuda.memory_stats()['allocation.all.allocated'] == after_copy
        want = ref.update(calls[k][0], calls[k][1], stream_of)
        _assert_equal(got, want, 'call %d' % k)
        L.assert_same(outputs_gpu(trk), L.outputs_np(ref), 'call %d' % k)
        fresh += int(ref.last_live_reads[3].sum())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = trk.update(det, count, stream_of)
    for k in (10, 11):                                                          # new rows, same buffers; state and memo move on with every replay
        det.copy_(torch.from_numpy(calls[k][0]))
        count.copy_(torch.from_numpy(calls[k][1]))
        poison(trk)
        g.replay()
        want = ref.update(calls[k][0], calls[k][1], stream_of)
        _assert_equal(got, want, 'replay %d' % k)
        L.assert_same(outputs_gpu(trk), L.outputs_np(ref), 'replay %d' % k)
        fresh += int(ref.last_live_reads[3].sum())
    assert fresh > 0


def test_tracker_enable_live_watch_equals_numpy_and_changes_nothing_else():
    from yolov6.hip import runtime
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.watch import WatchlistNp, confuse_table
    from yolov6.utils.watch_live import alerts_of
    calls = T.random_track_case(31, n_streams=3, max_det=20, n_calls=12)
    entries = L.live_list_for(calls, 3, 60, 1, 2, **KW)
    confuse = confuse_table([(1, 2), (3, 8), (0, 13)], weight=3)
    plain, trk, ref = runtime.PlateTracker(3, device='cuda', **KW), runtime.PlateTracker(3, device='cuda', **KW), PlateTrackerNp(3, **KW)
    wl = runtime.Watchlist(entries, confuse)
    for t, w in ((plain, wl), (trk, wl), (ref, WatchlistNp(entries, confuse))):
        t.enable_hold(min_hits=2)
        t.enable_watch(w, max_mismatch=1, max_cost=0.75)
    assert trk.live_memo is None
    trk.enable_live_watch(wl, min_hits=2, max_mismatch=1, max_cost=0.75)
    ref.enable_live_watch(WatchlistNp(entries, confuse), min_hits=2, max_mismatch=1, max_cost=0.75)
    fresh = alerts = 0
    for k, (det, count, stream_of, flush) in enumerate(calls):
        d, c = torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda()
        a, b, want = plain.update(d, c, stream_of, flush, 5), trk.update(d, c, stream_of, flush, 5), ref.update(det, count, stream_of, flush, 5)
        _assert_equal(b + trk.last_hold + (trk.last_watch,), want + ref.last_hold + (ref.last_watch,), 'call %d' % k)
        _assert_equal(a + plain.last_hold + (plain.last_watch,), want + ref.last_hold + (ref.last_watch,), 'call %d without the live watch' % k)
        L.assert_same(outputs_gpu(trk), L.outputs_np(ref), 'call %d' % k)
        fresh += int(ref.last_live_reads[3].sum())
        alerts += len(alerts_of(ref.last_live))
    assert fresh > 0 and alerts > 0 and plain.last_live is None and torch.equal(plain.state, trk.state)
    det, count, stream_of, _ = calls[3]
    d, c = torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda()
    trk.update(d, c, stream_of)
    ref.update(det, count, stream_of)
    assert trk.live_memo.any()
    trk.reset([1])
    ref.reset([1])
    L.assert_same((trk.live_memo.cpu().numpy(),), (ref._live.memo,), 'reset')
    assert not trk.live_memo[1].any() and trk.live_memo.any()
    trk.flush_all(max_ended=5)
    assert not trk.live_memo.any() and (trk.last_live.cpu().numpy().reshape(-1, 8) == L.NO_ROW).all()
    trk.enable_live_watch(None)
    trk.flush_all(max_ended=5)
    assert trk.last_live is None and trk.last_live_reads is None and trk.live_memo is None
    with pytest.raises(ValueError):
        trk.enable_live_watch(WatchlistNp(entries))                            # a host list is not a device list
    with pytest.raises(ValueError, match='min_hits'):
        trk.enable_live_watch(wl, min_hits=0)


# ---- Inferer(track=True, watchlist=..., watch_live=True) ------------------------------------------------------------------------------------
def test_infer_watch_live_matches_the_cpu_computation(tmp_path, monkeypatch):
    """alerts.txt of the GPU run against the loops of the CPU tests on the same run's untracked detections."""
    from PIL import Image
    from yolov6.utils.synth import build_synthetic
    from yolov6.utils.watch import entry_text
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    m = build_synthetic(CFG('yololps'), width=0.0625, sigma=1.5)
    ckpt = tmp_path / 'tiny.pt'
    torch.save({'model': m.half(), 'ema': None}, str(ckpt))
    (tmp_path / 'imgs').mkdir()
    for k, f in enumerate(T._moving_frames(10)):
        Image.fromarray(f).save(str(tmp_path / 'imgs' / ('f%02d.png' % k)))
    kw = dict(weights=str(ckpt), source=str(tmp_path / 'imgs'), yaml=None, img_size=[128, 160], conf_thres=0.06, iou_thres=0.45, max_det=20,
              device='0', save_txt=True, not_save_img=True, half=True, track_max_age=2, track_iou=0.25, track_expand=0.25)
    untracked = [d.cpu().numpy() for d in infer.run(save_dir=str(tmp_path / 'o0'), **kw)]
    tkw = dict(max_tracks=64, match_thres=0.25, new_thres=0.0, expand=0.25, max_age=2, ncls=m)
    _, _, ended = T.track_by_hand(untracked, 20, **tkw)
    reads = np.array([ri[4:12] for ri, _ in ended])
    rows = [[(v + 5) % 24 for v in reads[0]], reads[0], [255] * 7 + [int(reads[-1][7])], reads[0], [255] * 8]
    (tmp_path / 'watch.txt').write_text('\n'.join(entry_text(r) for r in rows) + '\n')
    entries = np.array(rows, np.uint8)
    infer.run(save_dir=str(tmp_path / 'o1'), track=True, watchlist=str(tmp_path / 'watch.txt'), watch_live=True, watch_live_min_hits=2, **kw)
    want = L.expected_alert_lines(untracked, 20, entries, 2, 1, 32768, **tkw)
    assert (tmp_path / 'o1' / 'alerts.txt').read_text().splitlines() == want and len(want) >= 1
