"""The watchlist match on the GPU: lp_watch_match against its numpy specification (yolov6/utils/watch.py) on every int32 of match_i
-- list lengths around the scan's workgroup size, read counts around its query block, planted entries in the first and the last
workgroup, wildcards, a non-default confusion table, ids that match nothing, garbage reads --, the steady state (no allocation, no
host read: captured in a graph behind the tracker), PlateTracker.enable_watch against PlateTrackerNp.enable_watch, and
Inferer(track=True, watchlist=...) against the CPU path's computation on the same detections."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
import test_track_cpu as T
import test_watch_cpu as C

pytestmark = pytest.mark.gpu
f32 = np.float32
POISON = -77
CFG = lambda name: os.path.join(REPO, 'configs', name + '.py')   # noqa: E731


def _consts():
    from yolov6.hip import abi
    return abi.LP_WATCH_BLOCK_ENTRIES, abi.LP_WATCH_QUERY_BLOCK


E, QB = _consts()
LIST_LENGTHS = [0, 1, 63, 64, 65, E - 1, E, E + 1, 2 * E + 3]
READ_COUNTS = [0, 1, QB - 1, QB, QB + 1, 2 * QB + 1, 5, 9]     # 5, 9: blocks of up to eight and twelve reads are instances of their own
LIMITS = [(0, 32768), (1, 32768), (8, 32768), (2, 2500)]       # max_mismatch 0 / 1 / 8 and a tight max_cost


def gpu_match(entries, confuse, ended_i, ended_f, ended_count, mm, mc):
    """lp_watch_match through the C ABI on fresh device tensors (ids 64..254 included, which ``Watchlist`` refuses); match_i is
    poisoned before the call, so every line is seen to be written."""
    from yolov6.hip import abi
    lib = abi.load()
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    ptr = lambda t: None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())   # noqa: E731
    d_e, d_c, d_i, d_f, d_n = dev(entries), dev(confuse), dev(ended_i), dev(ended_f), dev(np.asarray(ended_count, np.int32))
    S, M = ended_i.shape[:2]
    match = torch.full((S, M, 4), POISON, dtype=torch.int32, device='cuda')
    need = lib.lp_watch_workspace_bytes(S, M)
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device='cuda')             # the workspace may hold anything
    assert ws.data_ptr() % 16 == 0
    abi.check(lib.lp_watch_match(ptr(d_e), len(entries), ptr(d_c), ptr(d_i), ptr(d_f), ptr(d_n), S, M, mm, mc, ptr(match), ptr(ws), need,
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'lp_watch_match')
    torch.cuda.synchronize()
    return match.cpu().numpy()


def layout(V):
    """(counts per stream, max_ended) with V valid reads: a count above max_ended, a zero and a negative one among them."""
    if V == 0:
        return [0, -2, 0, -7], 3
    M = (V + 1) // 2
    return [M + 3, 0, -4, V - M, 0], M


def valid_lines(counts, M):
    return [(s, j) for s, c in enumerate(counts) for j in range(min(max(c, 0), M))]


def make_case(seed, N, V):
    """A random case of N entries and V valid reads with planted entries: read 0's ids at index 0 and at N - 1 (the first and the
    last workgroup), read 1 changed in one position at index 1 and unchanged at N - 2 (the last workgroup's tail holds the
    strictly cheaper one)."""
    counts, M = layout(V)
    entries, confuse, ended_i, ended_f, ended_count = C.random_watch_case(seed, N, counts, M)
    lines = valid_lines(counts, M)
    planted = {}
    if N >= 6 and V >= 2:
        (s0, j0), (s1, j1) = lines[0], lines[1]
        rng = np.random.default_rng(seed + 1)
        ended_i[s0, j0, 4:], ended_i[s1, j1, 4:] = rng.integers(12, 30, 8), rng.integers(30, 37, 8)   # ids no random entry holds
        ended_f[s0, j0, :8], ended_f[s1, j1, :8] = 1.0, 0.5
        entries[0] = entries[N - 1] = ended_i[s0, j0, 4:]
        entries[1] = entries[N - 2] = ended_i[s1, j1, 4:]
        entries[1, 3] = 5
        if confuse is not None:
            confuse[2, ended_i[s1, j1, 7], 5] = 7                              # that misread costs something: 7 * 128
        planted = {(s0, j0): (0, 0, 0), (s1, j1): (N - 2, 0, 0)}
    return (entries, confuse, ended_i, ended_f, ended_count), planted


@pytest.mark.parametrize('N', LIST_LENGTHS)
def test_watch_match_equals_numpy_spec(N):
    from yolov6.utils.watch import watch_match_np
    hits = 0
    for k, V in enumerate(READ_COUNTS):
        case, planted = make_case(1000 * k + N, N, V)
        for mm, mc in LIMITS:
            got, want = gpu_match(*case, mm, mc), watch_match_np(*case, mm, mc)
            if not np.array_equal(got, want):
                bad = np.argwhere(got != want)
                raise AssertionError('N %d, %d reads, limits %s: %d ints differ, first at %s: got %s, want %s'
                                     % (N, V, (mm, mc), len(bad), bad[0].tolist(), got[tuple(bad[0][:2])], want[tuple(bad[0][:2])]))
            hits += int((got[:, :, 0] >= 0).sum())
        for (s, j), exp in planted.items():                                    # with the last limits: 2 mismatches, cost <= 2500
            assert tuple(got[s, j, :3]) == exp and got[s, j, 3] >= 2, (N, V, s, j, got[s, j])
        counts, M = layout(V)
        assert np.array_equal(got[[s for s, c in enumerate(counts) if c <= 0]].reshape(-1, 4), [C.NONE] * (M * sum(c <= 0 for c in counts)))
    assert (hits > 0) == (N > 0)


def test_planted_entries_in_the_first_and_the_last_workgroup():
    """N = 2E + 3: index 0 and N - 1 are two workgroups apart.  The lower index wins a tie and n_hits counts both; a strictly
    cheaper entry in the last workgroup's tail wins over a dearer one in the first."""
    from yolov6.utils.watch import watch_match_np
    N, V = 2 * E + 3, QB + 1
    case, planted = make_case(7, N, V)
    entries, confuse, ended_i, ended_f, ended_count = case
    (s0, j0), (s1, j1) = list(planted)
    assert (N - 1) // E == 2 and (N - 2) // E == 2
    for mm, mc in ((1, 32768), (8, 32768)):
        got = gpu_match(*case, mm, mc)
        assert np.array_equal(got, watch_match_np(*case, mm, mc))
        assert tuple(got[s0, j0, :3]) == (0, 0, 0) and got[s0, j0, 3] >= 2
        assert tuple(got[s1, j1, :3]) == (N - 2, 0, 0) and got[s1, j1, 3] >= 2       # index 1 is accepted too, at a cost above 0
    alone = gpu_match(entries[:N - 2], confuse, ended_i, ended_f, ended_count, 1, 32768)     # without the tail: index 1 it is
    assert alone[s1, j1, 0] == 1 and alone[s1, j1, 1] == 1 and alone[s1, j1, 2] > 0 and tuple(alone[s0, j0]) == (0, 0, 0, 1)


def test_wildcards_in_every_position_and_ids_that_match_nothing():
    from yolov6.utils.watch import watch_match_np
    rng = np.random.default_rng(5)
    counts, M = layout(QB + 1)
    ended_i, ended_f, ended_count = C.random_reads(rng, counts, M, garbage=0.1)
    reads = np.array([ended_i[s, j, 4:] for s, j in valid_lines(counts, M)])
    rows = []
    for r in reads:                                                             # per read: a wildcard in each position, an id 64..254 in each
        for p in range(8):
            a, b = np.clip(r, 0, 63), np.clip(r, 0, 63)
            a[p], b[p] = 255, 64 + (p * 27 + int(r[0]) % 7) % 191
            rows += [a, b]
    rows += [[255] * 8, [254] * 8, [64] * 8]
    entries = np.array(rows, np.uint8)
    assert len(entries) > E // 8 and (ended_i[:, :, 4:] < 0).any() and (ended_i[:, :, 4:] >= 64).any()
    confuse = C.random_confuse(rng)
    for mm, mc in LIMITS + [(0, 0), (1, 4096), (8, 32767)]:
        got, want = gpu_match(entries, confuse, ended_i, ended_f, ended_count, mm, mc), watch_match_np(entries, confuse, ended_i, ended_f, ended_count, mm, mc)
        assert np.array_equal(got, want), (mm, mc, np.argwhere(got != want)[:3])
        if (mm, mc) == (0, 0):                                                  # a read with all ids in range: its eight one-wildcard rows and the all-wildcard row
            clean = [(s, j) for s, j in valid_lines(counts, M) if ((ended_i[s, j, 4:] >= 0) & (ended_i[s, j, 4:] < 64)).all()]
            assert len(clean) >= 3 and all(got[s, j, 3] >= 9 and got[s, j, 1] == 0 for s, j in clean)


def test_confuse_null_is_the_table_of_sixteens_and_a_zero_weight_pair_counts():
    from yolov6.utils.watch import watch_match_np
    case, _ = make_case(11, E + 1, QB + 1)
    entries, confuse, ended_i, ended_f, ended_count = case
    assert (confuse == 0).any() and confuse[2, 3, 8] == 0
    full = np.full((3, 64, 64), 16, np.uint8)
    for mm, mc in LIMITS:
        null = gpu_match(entries, None, ended_i, ended_f, ended_count, mm, mc)
        assert np.array_equal(null, gpu_match(entries, full, ended_i, ended_f, ended_count, mm, mc))
        assert np.array_equal(null, watch_match_np(entries, None, ended_i, ended_f, ended_count, mm, mc))
    # a read of 3s against an entry of 3s with one 8: the pair (3, 8) of group 2 weighs 0, yet it is a mismatch
    read = C.one_read([3] * 8, 1.0)
    e = np.array([[3, 3, 3, 3, 3, 8, 3, 3], [8, 3, 3, 3, 3, 3, 3, 3]], np.uint8)
    c = confuse.copy()
    c[0, 3, 8] = 9
    assert gpu_match(e, c, *read, 1, 0)[0, 0].tolist() == [0, 1, 0, 1] and gpu_match(e, c, *read, 0, 32768)[0, 0].tolist() == list(C.NONE)
    assert gpu_match(e, c, *read, 1, 32768)[0, 0].tolist() == [0, 1, 0, 2] and gpu_match(e[1:], c, *read, 1, 32768)[0, 0].tolist() == [0, 1, 9 * 256, 1]


def test_position_weight_edges_on_the_device():
    below, above = np.nextafter(f32(1 / 255), f32(0)), np.nextafter(f32(1 / 255), f32(1))
    shares = np.array([0, f32(1e-42), below, f32(1 / 255), above, 1, 2, np.nan, -1, np.inf, f32(254.999 / 255), 0.5], f32)
    want = [1, 1, 1, 2, 2, 256, 256, 1, 1, 256, 255, 128]
    ended_i, ended_f = np.zeros((1, len(shares), 12), np.int32), np.zeros((1, len(shares), 12), f32)
    ended_f[0, :, 0] = shares
    entries = np.array([[9, 0, 0, 0, 0, 0, 0, 0]], np.uint8)
    got = gpu_match(entries, None, ended_i, ended_f, [len(shares)], 8, 32768)
    assert got[0].tolist() == [[0, 1, 16 * q, 1] for q in want]


def test_many_streams_and_an_empty_list():
    """More streams than the threads of the prefix kernel's workgroup, and N = 0 through ``Watchlist``."""
    from yolov6.hip import runtime
    from yolov6.utils.watch import watch_match_np
    rng = np.random.default_rng(9)
    S, M = 1500, 2
    counts = rng.integers(-1, 4, S)
    ended_i, ended_f, ended_count = C.random_reads(rng, counts, M, n_ids=4, garbage=0.0)
    entries = C.random_entries(rng, 300, n_ids=4, nothing=0.0)
    wl = runtime.Watchlist(entries)
    dev = [torch.from_numpy(a).cuda() for a in (ended_i, ended_f, ended_count)]
    got = wl.match(*dev, max_mismatch=2, max_cost=1.0).cpu().numpy()
    assert np.array_equal(got, watch_match_np(entries, None, ended_i, ended_f, ended_count, 2, 4096)) and (got[:, :, 0] >= 0).sum() > 100
    empty = runtime.Watchlist(np.zeros((0, 8), np.uint8))
    out, _ = empty.buffers(S, M)
    out.fill_(POISON)
    assert empty.n == 0 and np.array_equal(empty.match(*dev).cpu().numpy().reshape(-1, 4), [C.NONE] * (S * M))
    with pytest.raises(ValueError):
        runtime.Watchlist(np.full((1, 8), 64))


# ---- behind the tracker ------------------------------------------------------------------------------------------------------------------
KW = dict(max_tracks=8, match_thres=0.3, new_thres=0.2, expand=0.5, max_age=2)


def _assert_equal(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        g = g.cpu().numpy()
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g.view(np.int32), np.ascontiguousarray(w).view(np.int32)), (what, k)


def test_steady_state_no_allocation_and_graph_capture():
    """Ten updates with the watch enabled allocate nothing after the first; tracker and match perform no host read: they are
    captured in one graph (a single chain on one stream) and the replays match the specification."""
    from yolov6.hip import runtime
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.watch import WatchlistNp
    calls = T.random_track_case(21, n_streams=4, max_det=20, Bs=(4,) * 12)
    entries = C.watchlist_for(calls, 4, **KW)
    confuse = C.random_confuse(np.random.default_rng(1))
    trk, ref = runtime.PlateTracker(4, device='cuda', **KW), PlateTrackerNp(4, **KW)
    trk.enable_watch(runtime.Watchlist(entries, confuse), max_mismatch=2, max_cost=2.5)
    ref.enable_watch(WatchlistNp(entries, confuse), max_mismatch=2, max_cost=2.5)
    det = torch.from_numpy(calls[0][0]).cuda()
    count = torch.from_numpy(calls[0][1]).cuda()
    stream_of = [0, 1, 3, 1]
    flush = [0, 1, 0, 0]                                                        # stream 1 ends its tracks in every call: reads to match
    trk.update(det, count, stream_of, flush)
    ref.update(calls[0][0], calls[0][1], stream_of, flush)
    torch.cuda.synchronize()
    hits = 0
    for k in range(1, 10):
        det.copy_(torch.from_numpy(calls[k][0]))
        count.copy_(torch.from_numpy(calls[k][1]))
        after_copy = torch.cuda.memory_stats()['allocation.all.allocated']
        got = trk.update(det, count, stream_of, flush)
        assert torch.cuda.memory_stats()['allocation.all.allocated'] == after_copy
        want = ref.update(calls[k][0], calls[k][1], stream_of, flush)
        _assert_equal(got + (trk.last_watch,), want + (ref.last_watch,), 'call %d' % k)
        hits += int((ref.last_watch[:, :, 0] >= 0).sum())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = trk.update(det, count, stream_of, flush)
        match = trk.last_watch
    for k in (10, 11):                                                          # new rows, same buffers; the state moves on with every replay
        det.copy_(torch.from_numpy(calls[k][0]))
        count.copy_(torch.from_numpy(calls[k][1]))
        for buf in got + (match,):
            buf.fill_(float('nan') if buf.dtype == torch.float32 else -7)
        g.replay()
        torch.cuda.synchronize()
        want = ref.update(calls[k][0], calls[k][1], stream_of, flush)
        _assert_equal(got + (match,), want + (ref.last_watch,), 'replay %d' % k)
        hits += int((ref.last_watch[:, :, 0] >= 0).sum())
    assert hits > 0


def test_tracker_enable_watch_equals_numpy_and_changes_nothing_else():
    from yolov6.hip import runtime
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.watch import WatchlistNp, confuse_table
    calls = T.random_track_case(31, n_streams=3, max_det=20, n_calls=12)
    entries = C.watchlist_for(calls, 3, **KW)
    confuse = confuse_table([(1, 2), (3, 8), (0, 13)], weight=3)
    plain, trk, ref = runtime.PlateTracker(3, device='cuda', **KW), runtime.PlateTracker(3, device='cuda', **KW), PlateTrackerNp(3, **KW)
    wl = runtime.Watchlist(entries, confuse)
    trk.enable_watch(wl, max_mismatch=1, max_cost=0.75)
    ref.enable_watch(WatchlistNp(entries, confuse), max_mismatch=1, max_cost=0.75)
    hits = 0
    for k, (det, count, stream_of, flush) in enumerate(calls):
        d, c = torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda()
        a, b, want = plain.update(d, c, stream_of, flush, 5), trk.update(d, c, stream_of, flush, 5), ref.update(det, count, stream_of, flush, 5)
        _assert_equal(b + (trk.last_watch,), want + (ref.last_watch,), 'call %d' % k)
        _assert_equal(a, want, 'call %d without the watch' % k)
        hits += int((ref.last_watch[:, :, 0] >= 0).sum())
    assert hits > 0 and plain.last_watch is None and torch.equal(plain.state, trk.state)
    ended = trk.flush_all(max_ended=5)
    assert trk.last_watch.shape == (3, 5, 4) and ended[2].shape == (3, 5, 12)
    trk.enable_watch(None)
    trk.flush_all(max_ended=5)
    assert trk.last_watch is None
    with pytest.raises(ValueError):
        trk.enable_watch(WatchlistNp(entries))                                 # a host list is not a device list


# ---- Inferer(track=True, watchlist=...) ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('batch_size', [1, 8])
def test_infer_watchlist_matches_the_cpu_path(tmp_path, monkeypatch, batch_size):
    """hits.txt of the GPU run against watch_match_np on the records PlateTrackerNp ends on the same run's untracked detections."""
    from PIL import Image
    from yolov6.utils.synth import build_synthetic
    from yolov6.utils.track import plate_text
    from yolov6.utils.watch import confuse_table, cost_units, entry_text, watch_match_np
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
              device='0', save_txt=True, not_save_img=True, half=True, batch_size=batch_size, track_max_age=2, track_iou=0.25,
              track_expand=0.25)
    plain = infer.run(save_dir=str(tmp_path / 'o0'), **kw)
    _, _, ended = T.track_by_hand([d.cpu().numpy() for d in plain], 20, max_tracks=64, match_thres=0.25, new_thres=0.0, expand=0.25,
                                  max_age=2, ncls=m)
    reads, shares = np.array([ri[4:12] for ri, _ in ended]), np.array([rf[:8] for _, rf in ended], f32)
    assert len(reads) >= 2
    near = reads[1].copy()
    p = int(np.argmax(shares[1]))
    near[p] = (near[p] + 1) % 37
    rows = [reads[0], near, reads[0], [255] * 7 + [int(reads[-1][7])], [(v + 5) % 37 for v in reads[0]]]
    (tmp_path / 'watch.txt').write_text('\n'.join(entry_text(r) for r in rows) + '\n')
    entries = np.array(rows, np.uint8)
    pair = (int(reads[1][p]), int(near[p]))
    infer.run(save_dir=str(tmp_path / 'o1'), track=True, watchlist=str(tmp_path / 'watch.txt'), watch_mismatch=7, watch_cost=0.25,
              watch_confusable='%d:%d' % pair, watch_confusable_weight=2, **kw)
    plates = (tmp_path / 'o1' / 'plates.txt').read_text().splitlines()
    assert plates == T.plate_lines(ended)
    ended_i, ended_f = np.zeros((1, len(reads), 12), np.int32), np.zeros((1, len(reads), 12), f32)
    ended_i[0, :, 4:], ended_f[0, :, :8] = reads, shares
    match = watch_match_np(entries, confuse_table([pair], 2, 2), ended_i, ended_f, [len(reads)], 7, cost_units(0.25))[0]
    want = ['%s %s %d %s %d %d %d' % (' '.join(line.split()[:3]), plate_text(reads[k]), e, entry_text(entries[e]), mi, co, n)
            for k, (line, (e, mi, co, n)) in enumerate(zip(plates, match.tolist())) if e >= 0]
    assert (tmp_path / 'o1' / 'hits.txt').read_text().splitlines() == want and len(want) >= 2 and match[0, 3] >= 2
