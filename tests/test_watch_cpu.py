"""The watchlist match on the CPU: ``watch_match_np`` (yolov6/utils/watch.py, the specification of lp_watch_match) against a plain
triple loop in Python integers, the edges of its rule, the helpers around it (``parse_watchlist``, ``cost_units``,
``confuse_table``), ``PlateTrackerNp.enable_watch``, the argument checks of lp_watch_match (no device needed) and
``tools/infer.py --track --watchlist`` on the CPU path.  ``random_watch_case`` and ``match_loops`` are shared with
tests/test_watch_gpu.py."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
import test_track_cpu as T

LP_ERR_ARG = -1
f32 = np.float32
NAN = float('nan')
NONE = (-1, 0, 0, 0)


# ---- the rule once more, as loops over Python integers --------------------------------------------------------------------------------
def weight_of(share):
    """q_p of one fp32 share."""
    share = f32(share)
    if not share > 0:
        return 1
    with np.errstate(all='ignore'):
        t = f32(share * f32(255.0))
    return (255 if t >= 255 else int(t)) + 1


def match_loops(entries, confuse, ended_i, ended_f, ended_count, max_mismatch, max_cost):
    """match_i by the words of the rule: lines, entries and positions one by one."""
    S, max_ended = ended_i.shape[:2]
    out = np.zeros((S, max_ended, 4), np.int32)
    out[:, :, 0] = -1
    for s in range(S):
        for j in range(min(max(int(ended_count[s]), 0), max_ended)):
            best_key, hits = None, 0
            for e in range(len(entries)):
                mism = cost = 0
                for p in range(8):
                    w, b = int(entries[e, p]), int(ended_i[s, j, 4 + p])
                    if w == 255 or (0 <= b < 64 and w == b):
                        continue
                    c = int(confuse[min(p, 2), b, w]) if (confuse is not None and 0 <= b < 64 and w < 64) else 16
                    mism += 1
                    cost += weight_of(ended_f[s, j, p]) * c
                if mism <= max_mismatch and cost <= max_cost:
                    hits += 1
                    if best_key is None or (cost, e) < best_key[:2]:
                        best_key = (cost, e, mism)
            if hits:
                out[s, j] = (best_key[1], best_key[2], best_key[0], hits)
    return out


def random_confuse(rng, zero_pair=True):
    """A non-default table: most weights 16, a third of them lower, one pair of weight 0 in group 2 (ids 3 and 8)."""
    c = np.where(rng.random((3, 64, 64)) < 0.35, rng.integers(0, 17, (3, 64, 64)), 16).astype(np.uint8)
    if zero_pair:
        c[2, 3, 8] = c[2, 8, 3] = 0
    return c


def random_reads(rng, counts, max_ended, n_ids=12, garbage=0.1):
    """(ended_i, ended_f, ended_count) with ``counts`` per stream (any integers): ids below ``n_ids`` so that entries drawn alike
    match often, a share of garbage ids (negative, >= 64), shares on a grid with 0, values above 1, NaN and negatives."""
    S = len(counts)
    ended_i = rng.integers(-50, 50, (S, max_ended, 12)).astype(np.int32)          # whatever lies in the other columns
    ids = rng.integers(0, n_ids, (S, max_ended, 8))
    junk = rng.random((S, max_ended, 8)) < garbage
    ended_i[:, :, 4:] = np.where(junk, rng.choice([-1, -7, 64, 65, 255, 300, 2 ** 31 - 1, -2 ** 31], (S, max_ended, 8)), ids)
    share = rng.choice(np.array([0, 1 / 8, 1 / 4, 0.5, 0.75, 0.999, 1, 1.5, NAN, -0.5], f32), (S, max_ended, 12),
                       p=[.05, .1, .1, .2, .2, .1, .15, .04, .03, .03])
    return ended_i, share.astype(f32), np.asarray(counts, np.int32)


def random_entries(rng, N, n_ids=12, wild=0.1, nothing=0.03):
    """uint8 [N, 8]: ids below ``n_ids``, wildcards, and ids 64..254 (which match nothing)."""
    e = rng.integers(0, n_ids, (N, 8))
    u = rng.random((N, 8))
    e = np.where(u < wild, 255, np.where(u < wild + nothing, rng.integers(64, 255, (N, 8)), e))
    return e.astype(np.uint8)


def random_watch_case(seed, N, counts, max_ended, confuse=True):
    rng = np.random.default_rng(seed)
    return (random_entries(rng, N), random_confuse(rng) if confuse else None) + random_reads(rng, counts, max_ended)


def one_read(best, share=1.0):
    """The ended records of one stream holding one read."""
    ended_i, ended_f = np.zeros((1, 1, 12), np.int32), np.zeros((1, 1, 12), f32)
    ended_i[0, 0, 4:], ended_f[0, 0, :8] = best, share
    return ended_i, ended_f, np.array([1], np.int32)


# ---- watch_match_np -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', range(6))
def test_match_np_against_the_loops(seed):
    from yolov6.utils.watch import watch_match_np
    rng = np.random.default_rng(100 + seed)
    N, max_ended = int(rng.integers(1, 60)), 4
    case = random_watch_case(seed, N, [3, 0, 9, -2, 1], max_ended, confuse=seed % 2 == 0)
    seen = 0
    for mm, mc in ((0, 32768), (1, 32768), (2, 3000), (8, 32768), (3, int(rng.integers(0, 12000)))):
        got, want = watch_match_np(*case, mm, mc), match_loops(*case, mm, mc)
        assert np.array_equal(got, want), (mm, mc, np.argwhere(got != want)[:3])
        seen += int((got[:, :, 0] >= 0).sum())
    assert np.array_equal(got[1], [NONE] * max_ended) and np.array_equal(got[3], [NONE] * max_ended) and seen > 0
    assert (case[0] == 255).any() and ((case[0] >= 64) & (case[0] < 255)).any() and (case[2][:, :, 4:] < 0).any() \
        and (case[2][:, :, 4:] >= 64).any()


def test_position_weight_edges():
    from yolov6.utils.watch import position_weight, watch_match_np
    below, above = np.nextafter(f32(1 / 255), f32(0)), np.nextafter(f32(1 / 255), f32(1))
    denormal = f32(1e-42)
    shares = np.array([0, denormal, below, f32(1 / 255), above, 1, 2, NAN, -1, np.inf, f32(254.999 / 255), 0.5], f32)
    want = [1, 1, 1, 2, 2, 256, 256, 1, 1, 256, 255, 128]
    assert denormal > 0 and f32(below * f32(255)) < 1 <= f32(above * f32(255))
    assert position_weight(shares).tolist() == want == [weight_of(v) for v in shares]
    entries = np.array([[9, 0, 0, 0, 0, 0, 0, 0]], np.uint8)                    # differs from the read in position 0 alone
    for v, q in zip(shares, want):
        got = watch_match_np(entries, None, *one_read([0] * 8, v), 8, 32768)
        assert got[0, 0].tolist() == [0, 1, 16 * q, 1], (v, q)


def test_acceptance_edges():
    from yolov6.utils.watch import watch_match_np
    read = one_read([1, 2, 3, 4, 5, 6, 7, 8], [1, 1, 0.5, 0.5, 0.25, 1, 1, 1])
    entries = np.array([[1, 2, 3, 4, 5, 6, 7, 8],                               # the read itself
                        [1, 2, 9, 4, 5, 6, 7, 8],                               # position 2 differs: cost 16 * 128 = 2048
                        [9, 9, 9, 9, 9, 9, 9, 9]], np.uint8)                    # everything differs
    all8 = 16 * (256 * 5 + 128 * 2 + 64)
    m = lambda mm, mc, e=entries: watch_match_np(e, None, *read, mm, mc)[0, 0].tolist()   # noqa: E731
    assert m(0, 32768) == [0, 0, 0, 1] and m(0, 0) == [0, 0, 0, 1]
    assert m(1, 32768) == [0, 0, 0, 2] and m(7, 32768) == [0, 0, 0, 2] and m(8, 32768) == [0, 0, 0, 3]
    assert m(8, all8 - 1) == [0, 0, 0, 2] and m(8, all8)[3] == 3
    assert m(1, 2048, entries[1:]) == [0, 1, 2048, 1] and m(1, 2047, entries[1:]) == list(NONE)      # one unit less rejects it
    assert m(0, 32768, entries[1:]) == list(NONE) and m(8, 0, entries[1:]) == list(NONE)
    assert m(8, 32768, entries[2:]) == [0, 8, all8, 1] and m(7, 32768, entries[2:]) == list(NONE)
    full = watch_match_np(entries[2:], None, *one_read([1] * 8, 1.0), 8, 32768)[0, 0].tolist()
    assert full == [0, 8, 32768, 1]                                             # the largest cost there is


def test_counts_outside_the_range_and_an_empty_list():
    from yolov6.utils.watch import watch_match_np
    rng = np.random.default_rng(3)
    ended_i, ended_f, _ = random_reads(rng, [0, 0, 0, 0], 3, garbage=0)
    entries = ended_i[:, :, 4:].reshape(-1, 8).astype(np.uint8)                 # every line is on the list
    got = watch_match_np(entries, None, ended_i, ended_f, [-3, 7, 2, 0], 0, 32768)
    assert np.array_equal(got[0], [NONE] * 3) and np.array_equal(got[3], [NONE] * 3) and np.array_equal(got[2, 2], NONE)
    assert (got[1, :, 0] >= 0).all() and (got[2, :2, 0] >= 0).all()            # a count above max_ended reads max_ended lines
    empty = watch_match_np(np.zeros((0, 8), np.uint8), None, ended_i, ended_f, [3, 3, 3, 3], 8, 32768)
    assert np.array_equal(empty.reshape(-1, 4), [NONE] * 12) and empty.dtype == np.int32


def test_ties_go_to_the_lowest_index_and_hits_count_duplicates():
    from yolov6.utils.watch import watch_match_np
    read = one_read([1, 2, 3, 4, 5, 6, 7, 8], [1, 1, 1, 1, 0.5, 0.5, 1, 1])
    two_half = [1, 2, 3, 4, 9, 9, 7, 8]          # two mismatches at share 0.5: cost 2 * 16 * 128 = 4096
    one_full = [9, 2, 3, 4, 5, 6, 7, 8]          # one mismatch at share 1: cost 16 * 256 = 4096
    far = [9, 9, 9, 4, 5, 6, 7, 8]
    m = lambda rows, mm=8: watch_match_np(np.array(rows, np.uint8), None, *read, mm, 32768)[0, 0].tolist()   # noqa: E731
    assert m([far, one_full, far, one_full, one_full]) == [1, 1, 4096, 5]
    assert m([far, one_full, far, one_full, one_full], 1) == [1, 1, 4096, 3]       # n_hits counts the duplicates
    assert m([two_half, one_full]) == [0, 2, 4096, 2]                             # equal cost: the lower index, whatever its mismatches
    assert m([one_full, two_half]) == [0, 1, 4096, 2]
    assert m([far, two_half, one_full], 1) == [2, 1, 4096, 1]
    wild = [255] * 8
    assert m([far, wild, wild]) == [1, 0, 0, 3]                                   # an entry of wildcards accepts everything at cost 0


def test_confusion_table_is_read_by_group_row_and_column():
    from yolov6.utils.watch import confuse_table, watch_match_np
    c = confuse_table([(1, 9)], group=0, weight=2)
    c[1, 2, 9], c[2, 3, 9], c[2, 9, 3] = 5, 7, 11                                # row = the read id, column = the entry id
    read = one_read([1, 2, 3, 3, 3, 3, 3, 3], 1.0)
    for p, want in ((0, 2), (1, 5), (2, 7), (7, 7)):
        e = np.array([[1, 2, 3, 3, 3, 3, 3, 3]], np.uint8)
        e[0, p] = 9
        assert watch_match_np(e, c, *read, 1, 32768)[0, 0].tolist() == [0, 1, want * 256, 1], p
    e = np.array([[1, 2, 3, 3, 3, 3, 3, 200]], np.uint8)                         # an id that matches nothing: 16, not the table
    assert watch_match_np(e, np.zeros_like(c), *read, 1, 32768)[0, 0].tolist() == [0, 1, 4096, 1]
    zero = watch_match_np(np.array([[9, 2, 3, 3, 3, 3, 3, 3]], np.uint8), np.zeros_like(c), *read, 0, 0)[0, 0].tolist()
    assert zero == list(NONE)                                                    # weight 0 is still a mismatch
    assert watch_match_np(np.array([[9, 2, 3, 3, 3, 3, 3, 3]], np.uint8), np.zeros_like(c), *read, 1, 0)[0, 0].tolist() == [0, 1, 0, 1]


# ---- the helpers ----------------------------------------------------------------------------------------------------------------------
PRO, ALP, ADS = ['京', '沪', '粤'], ['A', 'B', 'C'], [str(d) for d in range(10)] + ['A', 'B', 'D', 'Q', 'Z', 'S']


def test_parse_watchlist_round_trips_plate_text():
    from yolov6.utils.track import plate_text
    from yolov6.utils.watch import entry_text, parse_watchlist
    rng = np.random.default_rng(0)
    ids = np.stack([rng.integers(0, 3, 20), rng.integers(0, 3, 20)] + [rng.integers(0, 16, 20) for _ in range(6)], 1)
    text = [plate_text(row, PRO, ALP, ADS) for row in ids]
    assert np.array_equal(parse_watchlist(text, PRO, ALP, ADS), ids)
    assert np.array_equal(parse_watchlist([plate_text(row) for row in ids]), ids)               # without names: the ids
    lines = ['# stolen', '', '  沪B12*4?Z   # a comment', '1 2 * 4 5 6 7 63', '********']
    got = parse_watchlist(lines, PRO, ALP, ADS)
    assert got.tolist() == [[1, 1, 1, 2, 255, 4, 255, 14], [1, 2, 255, 4, 5, 6, 7, 63], [255] * 8] and got.dtype == np.uint8
    assert [entry_text(r, PRO, ALP, ADS) for r in got] == ['沪B12*4*Z', '1 2 * 4 5 6 7 63', '********']
    assert np.array_equal(parse_watchlist([entry_text(r) for r in got]), got)
    assert parse_watchlist([]).shape == (0, 8)
    for bad, no in ((['京A123456', '京A12345'], 2), (['# x', '', '1 2 3'], 3), (['1 2 3 4 5 6 7 64'], 1), (['京A1234567'], 1),
                    (['京X123456'], 1), (['1 2 3 4 5 6 7 x'], 1)):
        with pytest.raises(ValueError, match='line %d' % no):
            parse_watchlist(bad, PRO, ALP, ADS)
    with pytest.raises(ValueError, match='line 1'):
        parse_watchlist(['京A123456'])                                             # plate text without the name lists


def test_cost_units_confuse_table_and_the_checks():
    from yolov6.utils import watch
    assert watch.cost_units(None) == 32768 and watch.cost_units(0) == 0 and watch.cost_units(1) == 4096 and watch.cost_units(8) == 32768
    assert watch.cost_units(100) == 32768 and watch.cost_units(-1) == 0 and watch.cost_units(0.5) == 2048
    assert watch.cost_units(1 / 8192) == 1 and watch.cost_units(0.9 / 8192) == 0 and watch.cost_units(2047 / 4096) == 2047
    with pytest.raises(ValueError):
        watch.cost_units(NAN)
    c = watch.confuse_table('0D 0Q 8B'.split(), names=ADS)
    d, q, b = ADS.index('D'), ADS.index('Q'), ADS.index('B')
    assert c.shape == (3, 64, 64) and c.dtype == np.uint8 and (c[:2] == 16).all() and int((c != 16).sum()) == 6
    assert c[2, 0, d] == c[2, d, 0] == c[2, 0, q] == c[2, q, 0] == c[2, 8, b] == c[2, b, 8] == 4 and c[2, d, q] == 16
    assert watch.confuse_table([(1, 2)], group=1, weight=0)[1, 2, 1] == 0
    assert watch.confusable_pairs('0D 3:12') == ['0D', (3, 12)]
    for bad in (dict(pairs=['0X'], names=ADS), dict(pairs=['0D']), dict(pairs=[(1, 64)]), dict(pairs=[(1, 2)], weight=17),
                dict(pairs=[(1, 2)], group=3), dict(pairs=[(1, 2, 3)])):
        with pytest.raises(ValueError):
            watch.confuse_table(**bad)
    for bad in (np.zeros((3, 7)), np.full((2, 8), 64), np.full((2, 8), 254), np.full((1, 8), -1), np.zeros((2, 8), f32)):
        with pytest.raises(ValueError):
            watch.check_entries(bad)
    assert watch.check_entries([]).shape == (0, 8) and watch.check_entries([[0, 63, 255, 1, 2, 3, 4, 5]]).dtype == np.uint8
    for bad in ((9, 0), (-1, 0), (1, -1), (1, 32769), (1.5, 0)):
        with pytest.raises(ValueError):
            watch.check_params(*bad)
    with pytest.raises(ValueError):
        watch.check_confuse(np.full((3, 64, 64), 17))
    with pytest.raises(ValueError):
        watch.check_confuse(np.zeros((2, 64, 64), np.uint8))


# ---- PlateTrackerNp.enable_watch --------------------------------------------------------------------------------------------------------
def watchlist_for(calls, n_streams, seed=0, **kw):
    """A watchlist for the random tracker case ``calls``: the reads the case ends (run once without a list), half of them with
    one position changed, a few with wildcards, and random entries in between."""
    rng = np.random.default_rng(seed)
    _, outs = T.run_calls_np(calls, n_streams, 5, **kw)
    reads = np.concatenate([o[2][s, :min(int(o[4][s]), 5), 4:] for o in outs for s in range(n_streams)] or [np.zeros((0, 8), np.int32)])
    reads = reads[((reads >= 0) & (reads < 64)).all(1)]
    rows = []
    for r in reads[:: 2]:
        r = r.copy()
        u = rng.random()
        if u < 0.5:
            r[int(rng.integers(0, 8))] = int(rng.integers(0, 37))
        elif u < 0.7:
            r[int(rng.integers(0, 8))] = 255
        rows += [r, rng.integers(0, 37, 8)]
    return np.array(rows, np.uint8).reshape(-1, 8)


def test_tracker_np_enable_watch_changes_nothing_else():
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.watch import WatchlistNp, confuse_table, cost_units, watch_match_np
    kw = dict(max_tracks=16, max_age=2, expand=0.5)
    calls = T.random_track_case(2)
    entries = watchlist_for(calls, 3, **kw)
    wl = WatchlistNp(entries, confuse_table([(1, 2), (3, 8)], weight=3))
    plain, watched = PlateTrackerNp(3, **kw), PlateTrackerNp(3, **kw)
    assert watched.last_watch is None
    watched.enable_watch(wl, max_mismatch=2, max_cost=1.25)
    hits = 0
    for det, count, stream_of, flush in calls:
        a, b = plain.update(det, count, stream_of, flush, 5), watched.update(det, count, stream_of, flush, 5)
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.int32), y.view(np.int32))
        want = watch_match_np(entries, wl.confuse_np, b[2], b[3], b[4], 2, cost_units(1.25))
        assert watched.last_watch.shape == (3, 5, 4) and np.array_equal(watched.last_watch, want)
        assert np.array_equal(wl.match(b[2], b[3], b[4], 2, 1.25), want)
        hits += int((want[:, :, 0] >= 0).sum())
    assert hits > 0 and plain.last_watch is None
    watched.enable_watch(None)
    watched.flush_all()
    assert watched.last_watch is None
    with pytest.raises(ValueError):
        watched.enable_watch(wl, max_mismatch=9)


# ---- C ABI: everything is checked on the host before any launch ----------------------------------------------------------------------------
def test_watch_match_rejects_bad_arguments_before_launch():
    """Fake device addresses: a launch would fault, so LP_ERR_ARG proves the host check came first."""
    from yolov6.hip import abi
    lib = abi.load()
    v = lambda p: ctypes.c_void_p(p) if p else None   # noqa: E731
    S, M = 3, 5
    need = lib.lp_watch_workspace_bytes(S, M)
    assert need >= S * M * 16 + S * 4 and need % 16 == 0 and lib.lp_watch_workspace_bytes(2 * S, M) > need
    assert lib.lp_watch_workspace_bytes(0, M) == 0 and lib.lp_watch_workspace_bytes(S, -1) == 0 and lib.lp_watch_workspace_bytes(S, 0) > 0
    assert lib.lp_watch_workspace_bytes(1 << 20, 1 << 10) == 0

    def call(entries=0x100000, n=1000, confuse=0x200000, ei=0x300000, ef=0x310000, ec=0x320000, S=S, M=M, mm=1, mc=4096, match=0x330000,
             ws=0x400000, ws_bytes=need):
        return lib.lp_watch_match(v(entries), n, v(confuse), v(ei), v(ef), v(ec), S, M, mm, mc, v(match), v(ws), ws_bytes, None)

    err = lambda: lib.lp_last_error()   # noqa: E731
    assert call(n=-1) == LP_ERR_ARG and b'n_entries' in err() and call(n=(1 << 24) + 1) == LP_ERR_ARG and b'16777216' in err()
    assert call(S=0) == LP_ERR_ARG and b'n_streams' in err() and call(M=-1) == LP_ERR_ARG
    assert call(S=1 << 20, M=1 << 10) == LP_ERR_ARG and b'2^31' in err()
    for k, bad in (('mm', -1), ('mm', 9), ('mc', -1), ('mc', 32769)):
        assert call(**{k: bad}) == LP_ERR_ARG and b'max_mismatch' in err(), (k, bad)
    for k in ('entries', 'ei', 'ef', 'ec', 'match', 'ws'):
        assert call(**{k: 0}) == LP_ERR_ARG and b'null' in err(), k
    assert call(n=0, ec=0) == LP_ERR_ARG and call(n=0, match=0) == LP_ERR_ARG and b'null' in err()
    assert call(entries=0x100004) == LP_ERR_ARG and b'aligned' in err() and call(confuse=0x200002) == LP_ERR_ARG
    assert call(ws=0x400008) == LP_ERR_ARG and b'aligned' in err()
    assert call(ws_bytes=need - 1) == LP_ERR_ARG and b'workspace' in err() and call(ws_bytes=0) == LP_ERR_ARG
    for k, at in (('match', 0x100000 + 7992), ('match', 0x200000 + 12287), ('match', 0x300000 + S * M * 48 - 4), ('match', 0x310000),
                  ('match', 0x320000 + 8), ('ws', 0x100000 + 7984), ('ws', 0x300000), ('ws', 0x310000 + 16), ('ws', 0x320000),
                  ('ws', 0x330000 + 16), ('match', 0x400000 + need - 16)):
        assert call(**{k: at}) == LP_ERR_ARG and b'overlap' in err(), (k, hex(at))
    assert call(M=0) == 0 and call(M=0, n=0, entries=0, ei=0, ef=0, ec=0, match=0, ws=0, ws_bytes=0) == 0      # nothing to write: no launch


# ---- tools/infer.py --track --watchlist on the CPU path ------------------------------------------------------------------------------------
def test_infer_watchlist_cpu(tmp_path, monkeypatch):
    from PIL import Image
    from yolov6.utils.synth import build_synthetic
    from yolov6.utils.track import plate_text
    from yolov6.utils.watch import confuse_table, cost_units, entry_text, watch_match_np
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    m = build_synthetic(os.path.join(REPO, 'configs', 'yololps.py'), width=0.0625, sigma=1.5)
    ckpt = tmp_path / 'tiny.pt'
    torch.save({'model': m.half(), 'ema': None, 'epoch': 0}, str(ckpt))
    img_dir = tmp_path / 'imgs'
    img_dir.mkdir()
    for k, f in enumerate(T._moving_frames(6)):
        Image.fromarray(f).save(str(img_dir / ('f%02d.png' % k)))
    kw = dict(weights=str(ckpt), source=str(img_dir), yaml=None, img_size=[128, 160], conf_thres=0.06, iou_thres=0.45, max_det=20,
              device='cpu', not_save_img=True, save_txt=True, track=True, track_max_age=2, track_iou=0.25, track_expand=0.25)
    untracked = infer.run(save_dir=str(tmp_path / 'o0'), **dict(kw, track=False))
    plain = infer.run(save_dir=str(tmp_path / 'o1'), **kw)
    _, _, ended = T.track_by_hand([d.numpy() for d in untracked], 20, max_tracks=64, match_thres=0.25, new_thres=0.0, expand=0.25,
                                  max_age=2, ncls=m)
    plates = (tmp_path / 'o1' / 'plates.txt').read_text().splitlines()
    assert plates == T.plate_lines(ended)                                                  # the records behind the lines, exactly
    reads, shares = np.array([ri[4:12] for ri, _ in ended]), np.array([rf[:8] for _, rf in ended], f32)
    assert len(reads) >= 2 and not (tmp_path / 'o1' / 'hits.txt').exists()
    # the crafted list: read 0 itself twice (ambiguous), read 1 with its surest position changed, a wildcard line, and a stranger
    near = reads[1].copy()
    p = int(np.argmax(shares[1]))
    near[p] = (near[p] + 1) % 37
    rows = [reads[0], near, reads[0], [255] * 7 + [int(reads[-1][7])], [(v + 5) % 37 for v in reads[0]]]
    wl = tmp_path / 'watch.txt'
    wl.write_text('# crafted\n' + '\n'.join(entry_text(r) for r in rows) + '\n\n')
    entries = np.array(rows, np.uint8)
    pair = '%d:%d' % (int(reads[1][p]), int(near[p]))
    for sub, extra, confuse in (('o2', dict(), None), ('o3', dict(watch_mismatch=7, watch_cost=0.25, watch_confusable=pair, watch_confusable_weight=2),
                                                       confuse_table([(int(reads[1][p]), int(near[p]))], 2, 2))):
        again = infer.run(save_dir=str(tmp_path / sub), watchlist=str(wl), **extra, **kw)
        for a, b in zip(plain, again):
            assert torch.equal(a, b)
        for name in ('tracks.txt', 'plates.txt'):                                           # byte-identical to the run without a list
            assert (tmp_path / sub / name).read_bytes() == (tmp_path / 'o1' / name).read_bytes()
        ended_i, ended_f = np.zeros((1, len(reads), 12), np.int32), np.zeros((1, len(reads), 12), f32)
        ended_i[0, :, 4:], ended_f[0, :, :8] = reads, shares
        mm, mc = extra.get('watch_mismatch', 1), cost_units(extra.get('watch_cost'))
        match = watch_match_np(entries, confuse, ended_i, ended_f, [len(reads)], mm, mc)[0]
        want = ['%s %s %d %s %d %d %d' % (' '.join(line.split()[:3]), plate_text(reads[k]), e, entry_text(entries[e]), mi, co, n)
                for k, (line, (e, mi, co, n)) in enumerate(zip(plates, match.tolist())) if e >= 0]
        assert (tmp_path / sub / 'hits.txt').read_text().splitlines() == want
        assert match[0].tolist()[:3] == [0, 0, 0] and match[0, 3] >= 2 and len(want) >= 2
    with pytest.raises(ValueError, match='track'):
        infer.run(save_dir=str(tmp_path / 'o4'), watchlist=str(wl), **dict(kw, track=False))
