"""The watchlist match that survives one lost or gained character, on the GPU: lp_watch_match_indel against its numpy
specification (yolov6/utils/watch.py) on every int32 of match_i and match_align, with guard words around both -- list lengths
around the scan's workgroup size with the winner in the last lane of a workgroup and in the first of the next, read counts
around the query block and around the sizes at which the scan changes its instance, more streams than the prep kernel has
threads, the constructed set of the CPU test, ids over the whole byte range --, indel = 0 against lp_watch_match bit for bit, and
lp_watch_live_indel / PlateTracker.enable_watch / enable_live_watch(indel=1) against PlateTrackerNp."""
import ctypes

import numpy as np
import pytest
import torch

import test_track_cpu as T
import test_watch_cpu as C
import test_watch_gpu as G
import test_watch_indel_cpu as X
import test_watch_live_cpu as L
import test_watch_live_gpu as LG

pytestmark = pytest.mark.gpu
f32 = np.float32
POISON = -77
GUARD = 64                                                                     # int32 words in front of and behind each output


def _consts():
    from yolov6.hip import abi
    return abi.LP_WATCH_BLOCK_ENTRIES, abi.LP_WATCH_INDEL_QUERY_BLOCK


E, QB = _consts()
LIST_LENGTHS = [0, 1, E - 1, E, E + 1, 3 * E + 1]
READ_COUNTS = [0, 1, QB - 1, QB, QB + 1, 2 * QB - 1, 2 * QB, 2 * QB + 1]
LIMITS = [(1, 32768, X.FULL), (3, 9000, 1500)]                                 # (max_mismatch, max_cost, gap_cost)


def gpu_indel(entries, confuse, ended_i, ended_f, ended_count, mm, mc, indel=1, gap=X.FULL):
    """lp_watch_match_indel through the C ABI on fresh device tensors; both outputs lie between guard words and are poisoned, so
    every line is seen to be written and nothing around them."""
    from yolov6.hip import abi
    lib = abi.load()
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    ptr = lambda t: None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())   # noqa: E731
    d_e, d_c, d_i, d_f, d_n = dev(entries), dev(confuse), dev(ended_i), dev(ended_f), dev(np.asarray(ended_count, np.int32))
    S, M = ended_i.shape[:2]
    m_buf = torch.full((2 * GUARD + S * M * 4,), POISON, dtype=torch.int32, device='cuda')
    a_buf = torch.full((2 * GUARD + S * M,), POISON, dtype=torch.int32, device='cuda')
    match, align = m_buf[GUARD:GUARD + S * M * 4], a_buf[GUARD:GUARD + S * M]
    need = lib.lp_watch_workspace_bytes(S, M)
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device='cuda')             # the workspace may hold anything
    assert ws.data_ptr() % 16 == 0
    abi.check(lib.lp_watch_match_indel(ptr(d_e), len(entries), ptr(d_c), ptr(d_i), ptr(d_f), ptr(d_n), S, M, mm, mc, indel, gap, ptr(match),
                                       ptr(align), ptr(ws), need, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
              'lp_watch_match_indel')
    torch.cuda.synchronize()
    for buf in (m_buf, a_buf):
        assert (buf[:GUARD] == POISON).all() and (buf[-GUARD:] == POISON).all()
    return match.cpu().numpy().reshape(S, M, 4), align.cpu().numpy().reshape(S, M)


def assert_spec(case, mm, mc, gap, what):
    from yolov6.utils.watch import watch_match_np
    got, want = gpu_indel(*case, mm, mc, 1, gap), watch_match_np(*case, mm, mc, 1, gap, align=True)
    for g, w, name in zip(got, want, ('match_i', 'match_align')):
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError('%s, limits %s: %d ints of %s differ, first at %s: got %s, want %s'
                                 % (what, (mm, mc, gap), len(bad), name, bad[0].tolist(), g[tuple(bad[0][:2])], w[tuple(bad[0][:2])]))
    return got


def make_case(seed, N, V):
    """A random case of N entries and V valid reads.  Reads 0 and 1 get eight different ids that no random entry holds; read 0 without its head 3
    is planted at the last index of a workgroup (or of the list) and again behind it, read 1 with a character gained at head 5 at
    the first index of the next workgroup and again at the end of the list: the lower index has to win each tie."""
    counts, M = G.layout(V)
    entries, confuse, ended_i, ended_f, ended_count = C.random_watch_case(seed, N, counts, M)
    lines = G.valid_lines(counts, M)
    planted = {}
    if confuse is not None:
        confuse[2, 12:37] = 16                                                 # the planted reads pay every mismatch in full
    if N >= 1 and V >= 1:
        rng = np.random.default_rng(seed + 1)
        (s0, j0) = lines[0]
        ended_i[s0, j0, 4:], ended_f[s0, j0, :8] = rng.permutation(np.arange(12, 37))[:8], 1.0
        full = list(ended_i[s0, j0, 4:7]) + [5] + list(ended_i[s0, j0, 7:11])     # the entry whose head 3 the read lost
        at = min(E, N) - 1
        entries[at] = full
        if N > E + 2:
            entries[E + 2] = full
        planted[(s0, j0)] = (at, 2)
        if N > E and V >= 2:
            (s1, j1) = lines[1]
            ended_i[s1, j1, 4:], ended_f[s1, j1, :8] = rng.permutation(np.arange(12, 37))[:8], 0.5
            r = ended_i[s1, j1, 4:]
            short = list(r[:5]) + list(r[6:]) + [3]                             # the entry without the read's head 5
            entries[E] = short
            if N > E + 1:
                entries[N - 1] = short
            planted[(s1, j1)] = (E, 9)
    return (entries, confuse, ended_i, ended_f, ended_count), planted


@pytest.mark.parametrize('N', LIST_LENGTHS)
def test_watch_match_indel_equals_numpy_spec(N):
    hits = shifted = 0
    for k, V in enumerate(READ_COUNTS):
        case, planted = make_case(1000 * k + N, N, V)
        for mm, mc, gap in LIMITS:
            m, a = assert_spec(case, mm, mc, gap, 'N %d, %d reads' % (N, V))
            hits += int((m[:, :, 0] >= 0).sum())
            shifted += int((a > 0).sum())
            for (s, j), (at, code) in planted.items():
                assert m[s, j, 0] == at and m[s, j, 1] == 1 and m[s, j, 2] == gap and a[s, j] == code, (N, V, s, j, m[s, j], a[s, j])
                assert m[s, j, 3] >= (2 if N > E + 2 else 1)
        counts, M = G.layout(V)
        dead = [s for s, c in enumerate(counts) if c <= 0]
        assert np.array_equal(m[dead].reshape(-1, 4), [C.NONE] * (M * len(dead))) and not a[dead].any()
    assert (hits > 0) == (N > 0) and (shifted > 0) == (N > 0)


@pytest.mark.parametrize('V', [3, 4, 5, 8, 9, 12, 13])
def test_read_counts_at_which_the_scan_changes_its_instance(V):
    case, planted = make_case(40 + V, E + 5, V)
    for mm, mc, gap in LIMITS:
        m, a = assert_spec(case, mm, mc, gap, '%d reads' % V)
    assert all(a[s, j] == code for (s, j), (_, code) in planted.items()) and len(planted) == 2


def test_more_streams_than_the_prep_kernel_has_threads():
    rng = np.random.default_rng(9)
    S = 1030
    counts = rng.integers(-1, 3, S)
    ended_i, ended_f, ended_count = C.random_reads(rng, counts, 1, n_ids=4, garbage=0.0)
    entries = C.random_entries(rng, 300, n_ids=4, nothing=0.0)
    m, a = assert_spec((entries, None, ended_i, ended_f, ended_count), 2, 32768, 1000, '%d streams' % S)
    assert (m[:, :, 0] >= 0).sum() > 100 and (a > 0).sum() > 10


@pytest.mark.parametrize('case', X.constructed(), ids=lambda c: c[0])
def test_constructed_reads_on_the_device(case):
    name, entries, confuse, reads, mm, mc, gap, want, codes = case
    m, a = assert_spec((entries, confuse) + tuple(reads), mm, mc, gap, name)
    assert m[0].tolist() == [list(w) for w in want] and a[0].tolist() == codes


def test_ids_over_the_whole_byte_range_and_a_confusion_table():
    rng = np.random.default_rng(77)
    counts, M = G.layout(QB + 3)
    N = E + 300
    entries = rng.integers(0, 256, (N, 8)).astype(np.uint8)
    entries[rng.random((N, 8)) < 0.5] = 255                                      # enough wildcards for some rows to be accepted
    ended_i = rng.integers(-3, 70, (len(counts), M, 12)).astype(np.int32)
    ended_i[0, 0, 4:] = [-1, 64, 255, 300, -2 ** 31, 2 ** 31 - 1, 63, 0]
    ended_f = rng.choice(np.array([0, 1 / 8, 0.5, 0.999, 1, 1.5, np.nan, -0.5, np.inf], f32), (len(counts), M, 12)).astype(f32)
    confuse = C.random_confuse(rng)
    case = (entries, confuse, ended_i, ended_f, np.asarray(counts, np.int32))
    seen = 0
    for mm, mc, gap in ((8, 32768, 0), (8, 32768, X.FULL), (4, 12000, 700), (2, 32768, 2048)):
        m, a = assert_spec(case, mm, mc, gap, 'bytes')
        seen += int((a > 0).sum())
    assert seen > 0 and (entries[:, 2:] > 63).any() and (entries[:, 2:] < 255).any()


def test_indel_0_is_lp_watch_match_bit_for_bit():
    for N, V in ((0, 5), (1, 1), (E + 1, QB + 1), (3 * E + 1, 2 * QB + 1)):
        case, _ = make_case(500 + N, N, V)
        for mm, mc in G.LIMITS:
            old = G.gpu_match(*case, mm, mc)
            for gap in (0, X.FULL):
                m, a = gpu_indel(*case, mm, mc, 0, gap)
                assert np.array_equal(m, old) and not a.any(), (N, V, mm, mc, gap)


def test_watchlist_match_takes_indel_and_leaves_the_codes():
    from yolov6.hip import runtime
    from yolov6.utils.watch import watch_match_np
    case, planted = make_case(3, E + 9, QB + 1)
    entries, confuse, ended_i, ended_f, ended_count = case
    entries = np.where((entries > 63) & (entries < 255), 7, entries).astype(np.uint8)       # ``Watchlist`` refuses 64..254
    wl = runtime.Watchlist(entries, confuse)
    dev = [torch.from_numpy(a).cuda() for a in (ended_i, ended_f, ended_count)]
    old = wl.match(*dev, max_mismatch=1).cpu().numpy()
    assert wl.last_align is None and np.array_equal(old, watch_match_np(entries, confuse, ended_i, ended_f, ended_count, 1, 32768))
    m = wl.match(*dev, max_mismatch=1, indel=1, gap_cost=0.5).cpu().numpy()
    want = watch_match_np(entries, confuse, ended_i, ended_f, ended_count, 1, 32768, 1, 2048, align=True)
    assert np.array_equal(m, want[0]) and np.array_equal(wl.last_align.cpu().numpy(), want[1])
    assert all(want[1][s, j] == code for (s, j), (_, code) in planted.items()) and not np.array_equal(m, old)
    with pytest.raises(ValueError):
        wl.match(*dev, indel=2)


# ---- behind the tracker -------------------------------------------------------------------------------------------------------------------
def outputs_gpu(trk):
    return LG.outputs_gpu(trk) + (trk.last_live_align.cpu().numpy(),)


def outputs_np(trk):
    return L.outputs_np(trk) + (trk.last_live_align,)


@pytest.mark.parametrize('max_tracks', [8, 128])
def test_watch_live_indel_equals_numpy_spec(max_tracks):
    """Random scenes: every entry of the list is a read some track holds at some time with a character lost or gained, so fresh
    and standing shifted hits, re-lookups and reused slots all carry codes."""
    from yolov6.hip import runtime
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.watch import WatchlistNp
    n_obj, max_det = min(max_tracks + 2, 70), 80
    kw = dict(max_tracks=max_tracks, match_thres=0.3, new_thres=0.2, expand=0.25, max_age=2, ncls=T.NCLS)
    calls = LG.live_calls(max_tracks, T.NCLS, n_obj, max_det)
    rng = np.random.default_rng(5)
    entries = L.live_list_for(calls, 5, E + 1, 3, 1, **kw)
    entries = np.array([(X.lost(r, 2 + i % 5, 5) if i % 2 else X.gained(r, 2 + i % 5, 6)) if (i % 3 and (r < 64).all()) else list(r)
                        for i, r in enumerate(entries)], np.uint8)
    confuse = C.random_confuse(rng)
    trk, ref = runtime.PlateTracker(5, device='cuda', **kw), PlateTrackerNp(5, **kw)
    trk.enable_live_watch(runtime.Watchlist(entries, confuse), 1, max_mismatch=2, max_cost=1.5, indel=1, gap_cost=0.25)
    ref.enable_live_watch(WatchlistNp(entries, confuse), 1, max_mismatch=2, max_cost=1.5, indel=1, gap_cost=0.25)
    fresh = standing = 0
    for k, (det, count, stream_of, flush) in enumerate(calls):
        LG.poison(trk)
        trk.update(torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda(), stream_of, flush)
        ref.update(det, count, stream_of, flush)
        got, want = outputs_gpu(trk), outputs_np(ref)
        L.assert_same(got[:-1], want[:-1], 'T %d, call %d' % (max_tracks, k))
        assert np.array_equal(got[-1], want[-1]), (k, np.argwhere(got[-1] != want[-1])[:3])
        live_i, al = want[0], want[-1]
        fresh += int(((al > 0) & (live_i[:, :, 5] == 1)).sum())
        standing += int(((al > 0) & (live_i[:, :, 5] == 0) & (live_i[:, :, 0] >= 0)).sum())
        assert not al[live_i[:, :, 1] < 0].any()
    assert fresh > 0 and standing > 0, (fresh, standing)


def test_a_shifted_read_alerts_with_the_flag_only_and_is_looked_up_once():
    """One car whose read lost head 4 of its entry, in every frame: no hit without the flag; with it an alert in the frame the
    track reaches min_hits, del@4, which stands -- one lookup in all -- and the ended-record match reports it when the track ends."""
    from yolov6.hip import runtime
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.watch import WatchlistNp
    entries = np.array([(9, 9, 9, 9, 9, 9, 9, 9), L.PLATE], np.uint8)
    kw = dict(max_tracks=4, max_age=2)
    off, on, ref = runtime.PlateTracker(1, device='cuda', **kw), runtime.PlateTracker(1, device='cuda', **kw), PlateTrackerNp(1, **kw)
    wl = runtime.Watchlist(entries)                                             # (a list owns its match_i: one per tracker)
    off.enable_watch(wl)
    off.enable_live_watch(wl, min_hits=3)
    for t, w in ((on, runtime.Watchlist(entries)), (ref, WatchlistNp(entries))):
        t.enable_watch(w, indel=1)
        t.enable_live_watch(w, min_hits=3, indel=1)
    ended_hits = []
    for k in range(10):
        rows = [L.car(X.SHIFTED_PLATE)] if k < 6 else []
        det, count = T.frames_of([rows], 4)
        d, c = torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda()
        off.update(d, c, stream_of=[0])
        on.update(d, c, stream_of=[0])
        ref.update(det, count, stream_of=[0])
        L.assert_same(outputs_gpu(on)[:-1], outputs_np(ref)[:-1], 'frame %d' % k)
        assert np.array_equal(on.last_live_align.cpu().numpy(), ref.last_live_align)
        assert np.array_equal(on.last_watch.cpu().numpy(), ref.last_watch) and np.array_equal(on.last_watch_align.cpu().numpy(), ref.last_watch_align)
        assert not (off.last_live[:, :, 1] >= 0).any() and not (off.last_watch[:, :, 0] >= 0).any()
        assert off.last_live_align is None and off.last_watch_align is None
        row, n_lookups = ref.last_live[0, 0].tolist(), int(ref.last_live_reads[3][0])
        assert n_lookups == int(k == 2)
        if 2 <= k < 8:                                                         # live until more than max_age frames have missed it
            assert row[:6] == [0, 1, 1, X.FULL, 1, int(k == 2)] and ref.last_live_align[0, 0] == 3
        else:
            assert row == list(L.NO_ROW) and ref.last_live_align[0, 0] == 0
        if (ref.last_watch[:, :, 0] >= 0).any():
            ended_hits.append((k, ref.last_watch[0, 0].tolist(), int(ref.last_watch_align[0, 0])))
    assert ended_hits == [(8, [1, 1, X.FULL, 1], 3)]


def test_tracker_enable_watch_indel_changes_nothing_else():
    from yolov6.hip import runtime
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.watch import WatchlistNp
    calls = T.random_track_case(31, n_streams=3, max_det=20, n_calls=12)
    entries = C.watchlist_for(calls, 3, **G.KW)
    entries[1::4] = [X.lost(r, 2 + i % 5, 5) for i, r in enumerate(entries[0::4][:len(entries[1::4])])]
    plain, trk, ref = runtime.PlateTracker(3, device='cuda', **G.KW), runtime.PlateTracker(3, device='cuda', **G.KW), PlateTrackerNp(3, **G.KW)
    trk.enable_watch(runtime.Watchlist(entries), max_mismatch=1, max_cost=1.0, indel=1, gap_cost=0.5)
    ref.enable_watch(WatchlistNp(entries), max_mismatch=1, max_cost=1.0, indel=1, gap_cost=0.5)
    shifted = 0
    for k, (det, count, stream_of, flush) in enumerate(calls):
        d, c = torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda()
        a, b, want = plain.update(d, c, stream_of, flush, 5), trk.update(d, c, stream_of, flush, 5), ref.update(det, count, stream_of, flush, 5)
        G._assert_equal(b + (trk.last_watch, trk.last_watch_align), want + (ref.last_watch, ref.last_watch_align), 'call %d' % k)
        G._assert_equal(a, want, 'call %d without the watch' % k)
        shifted += int((ref.last_watch_align > 0).sum())
    assert shifted > 0 and plain.last_watch_align is None and torch.equal(plain.state, trk.state)
