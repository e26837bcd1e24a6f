"""The watchlist match that survives one lost or gained character, on the CPU: ``watch_match_np(..., indel=1)`` of
yolov6/utils/watch.py (the specification of lp_watch_match_indel) against the rule restated as loops over Python integers and
against a small dynamic programme, a constructed set in which every alignment code wins, the ties, the edges, the wrong
emulations the set must catch, the argument checks of the two C entry points, ``PlateTrackerNp`` and the CLI columns."""
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
import test_watch_live_cpu as LV

LP_ERR_ARG = -1
f32 = np.float32
FULL = 4096                                                                    # one fully confident mismatch, in cost units


# ---- the rule once more: cells, the 12 alignments, and a dynamic programme ---------------------------------------------------------------
def cell(entries, confuse, e, col, best, share, p):
    """(cost, mismatch) of read head p against entries[e, col], by rules 1 and 2."""
    w, b = int(entries[e, col]), int(best[p])
    if w == 255 or (0 <= b < 64 and w == b):
        return 0, 0
    c = int(confuse[min(p, 2), b, w]) if (confuse is not None and 0 <= b < 64 and w < 64) else 16
    return C.weight_of(share[p]) * c, 1


def add(*pairs):
    return sum(a for a, _ in pairs), sum(b for _, b in pairs)


def alignments(pair, gap, wrong=None):
    """[(cost, mismatches)] of the 12 codes; ``pair(p, col)`` = the cell of read head p against entry head col.  ``wrong`` names
    one of the emulations that the constructed set has to tell from the rule."""
    gapc = (gap, 0 if wrong == 'gap_is_no_mismatch' else 1)
    head = [pair(0, 0), pair(1, 1)]
    out = [add(*head, *[pair(p, p) for p in range(2, 8)])]
    tail7 = [pair(7, 7)] if wrong == 'head7_compared' else []
    for k in range(2, 7):                                                      # codes 1..5: the read lost entry head k
        h = [pair(0, 1), pair(1, 2)] if wrong == 'heads01_shifted' else head
        out.append(add(*h, *[pair(p, p) for p in range(2, k)], *[pair(p, p + 1) for p in range(k, 7)], gapc, *tail7))
    for k in range(2, 7):                                                      # codes 6..10: the read gained its head k
        first = k if wrong == 'r_from_k' else k + 1
        h = [pair(1, 0)] if wrong == 'heads01_shifted' else head
        out.append(add(*h, *[pair(p, p) for p in range(2, k)], *[pair(p, p - 1) for p in range(first, 8)], gapc, *tail7))
    out.append(add(*head, *[pair(p, p) for p in range(2, 7)], gapc, *tail7))   # code 11
    return out


def pick(al, wrong=None):
    """The code of the smallest (cost, mismatches, code)."""
    if wrong == 'code_order_reversed':
        return min(range(len(al)), key=lambda c: (al[c][0], al[c][1], -c))
    if wrong == 'cost_alone':
        return min(range(len(al)), key=lambda c: (al[c][0], c))
    return min(range(len(al)), key=lambda c: (al[c][0], al[c][1], c))


def one_gap_dp(pair, gap):
    """The smallest (cost, mismatches) over heads 2..7 of every alignment with at most one gap: a diagonal step compares read head
    i with entry head j, the one gap skips a read head or an entry head, and what is left over at the end of either side is not
    compared."""
    def f(i, j, used):
        if i == 8 or j == 8:
            return (0, 0)
        best = add(pair(i, j), f(i + 1, j + 1, used))
        if not used:
            best = min(best, add((gap, 1), f(i, j + 1, True)), add((gap, 1), f(i + 1, j, True)))
        return best
    return f(2, 2, False)


def indel_loops(entries, confuse, ended_i, ended_f, ended_count, max_mismatch, max_cost, indel=1, gap=FULL, wrong=None, dp=False):
    """(match_i, match_align) by the words of the rule: lines, entries, alignments and cells one by one.  ``dp``: also check every
    entry's score against ``one_gap_dp``."""
    S, max_ended = ended_i.shape[:2]
    out, out_a = np.zeros((S, max_ended, 4), np.int32), np.zeros((S, max_ended), np.int32)
    out[:, :, 0] = -1
    for s in range(S):
        for j in range(min(max(int(ended_count[s]), 0), max_ended)):
            best_key, hits = None, 0
            for e in range(len(entries)):
                pair = lambda p, col: cell(entries, confuse, e, col, ended_i[s, j, 4:], ended_f[s, j], p)   # noqa: E731
                al = alignments(pair, gap, wrong) if indel else alignments(pair, gap)[:1]
                code = pick(al, wrong)
                cost, mism = al[code]
                if dp and indel:
                    assert add(pair(0, 0), pair(1, 1), one_gap_dp(pair, gap)) == (cost, mism), (s, j, e)
                if mism <= max_mismatch and cost <= max_cost:
                    hits += 1
                    if best_key is None or (cost, e) < best_key[:2]:
                        best_key = (cost, e, mism, code)
            if hits:
                out[s, j] = (best_key[1], best_key[2], best_key[0], hits)
                out_a[s, j] = best_key[3]
    return out, out_a


def spec(entries, confuse, reads, mm, mc, indel=1, gap=FULL):
    from yolov6.utils.watch import watch_match_np
    return watch_match_np(entries, confuse, *reads, mm, mc, indel, gap, align=True)


def reads_of(rows, shares=None):
    """The ended records of one stream holding ``rows`` (eight ids each) at full shares, or ``shares``."""
    n = len(rows)
    ended_i, ended_f = np.zeros((1, n, 12), np.int32), np.zeros((1, n, 12), f32)
    ended_i[0, :, 4:] = rows
    ended_f[0, :, :8] = 1.0 if shares is None else shares
    return ended_i, ended_f, np.array([n], np.int32)


# ---- the constructed set: every code wins somewhere, every tie and edge is in it ---------------------------------------------------------
ENTRY = (30, 20, 2, 3, 4, 5, 6, 7)
FILL = 19                                                                      # a character that is nowhere in ENTRY


def lost(entry, k, fill=FILL):
    """The read of ``entry`` that lost head k: the later heads move down, ``fill`` comes in at head 7."""
    return list(entry[:k]) + list(entry[k + 1:]) + [fill]


def gained(entry, k, fill=FILL):
    """The read of ``entry`` that gained ``fill`` at head k: the later heads move up, entry head 7 drops out."""
    return list(entry[:k]) + [fill] + list(entry[k:7])


def constructed():
    """[(name, entries, confuse, reads, max_mismatch, max_cost, gap, want match_i lines, want codes)]."""
    E = np.array([ENTRY], np.uint8)
    zero = np.full((3, 64, 64), 16, np.uint8)
    zero[2, 7, 6] = zero[2, FILL, 7] = 0
    cases = []
    rows = [list(ENTRY)] + [lost(ENTRY, k) for k in range(2, 7)] + [gained(ENTRY, k) for k in range(2, 7)]
    want = [(0, 0, 0, 1)] + [(0, 1, FULL, 1)] * 10
    cases.append(('each shifted code', E, None, reads_of(rows), 1, 32768, FULL, want, list(range(11))))
    end = list(ENTRY[:7]) + [FILL]
    cases.append(('end beats a dearer mismatch', E, None, reads_of([end]), 1, 32768, 2048, [(0, 1, 2048, 1)], [11]))
    cases.append(('unshifted wins the tie with end', E, None, reads_of([end]), 1, 32768, FULL, [(0, 1, FULL, 1)], [0]))
    same = np.array([(30, 20, 5, 5, 5, 5, 5, 9)], np.uint8)
    cases.append(('the lowest of the equal codes, lost', same, None, reads_of([lost(same[0], 3)]), 1, 32768, FULL, [(0, 1, FULL, 1)], [1]))
    cases.append(('the lowest of the equal codes, gained', same, None, reads_of([gained(same[0], 4, 5)]), 1, 32768, 2048,   # ins@2..6 and end
                  [(0, 1, 2048, 1)], [6]))
    two = np.array([(1, 1, 1, 1, 1, 1, 1, 1), ENTRY, ENTRY], np.uint8)
    cases.append(('the lowest of the equal entries', two, None, reads_of([lost(ENTRY, 4)]), 1, 32768, FULL, [(1, 1, FULL, 2)], [3]))
    cases.append(('heads 0 and 1 never shift', E, None, reads_of([list(ENTRY[1:]) + [FILL], [FILL] + list(ENTRY[:7])]), 1, 32768, FULL,
                  [C.NONE, C.NONE], [0, 0]))
    cases.append(('fewer mismatches win at equal cost', E, zero, reads_of([list(ENTRY[:6]) + [7, FILL]]), 2, 32768, 0, [(0, 1, 0, 1)], [5]))
    cases.append(('no shifted hit without a mismatch to spend', E, None, reads_of([lost(ENTRY, 3), list(ENTRY)]), 0, 32768, 0,
                  [C.NONE, (0, 0, 0, 1)], [0, 0]))
    cases.append(('max_cost at a shifted cost', E, None, reads_of([gained(ENTRY, 5)]), 1, 1000, 1000, [(0, 1, 1000, 1)], [9]))
    cases.append(('max_cost one below a shifted cost', E, None, reads_of([gained(ENTRY, 5)]), 1, 999, 1000, [C.NONE], [0]))
    cases.append(('a free gap', E, None, reads_of([lost(ENTRY, 2)]), 1, 0, 0, [(0, 1, 0, 1)], [1]))
    wild = np.array([(30, 20, 2, 3, 255, 5, 6, 7)], np.uint8)                  # WILD under L at head 3 and under R at head 5
    cases.append(('a wildcard in a shifted column', wild, None, reads_of([lost(wild[0], 2)[:3] + [FILL] + lost(wild[0], 2)[4:],
                                                                          gained(wild[0], 3)[:5] + [FILL] + gained(wild[0], 3)[6:]]),
                  1, 32768, FULL, [(0, 1, FULL, 1), (0, 1, FULL, 1)], [1, 7]))
    none = np.array([(30, 20, 2, 3, 100, 5, 6, 7)], np.uint8)                  # an id that matches nothing, met under L and under R
    cases.append(('an id that matches nothing in a shifted column', none, None, reads_of([lost(none[0], 2), gained(none[0], 3)]), 2, 32768,
                  FULL, [(0, 2, 2 * FULL, 1), (0, 2, 2 * FULL, 1)], [1, 7]))
    bad = [lost(ENTRY, 2), gained(ENTRY, 2)]
    bad[0][4], bad[1][5] = -1, 64                                              # best outside 0..63 under L (head 4) and under R (head 5)
    cases.append(('a read id outside 0..63 in a shifted column', E, None, reads_of(bad), 2, 32768, FULL,
                  [(0, 2, 2 * FULL, 1), (0, 2, 2 * FULL, 1)], [1, 6]))
    seven = np.array([(30, 20, 2, 3, 4, 5, 6, 36)], np.uint8)                  # a 7-character plate: the blank id in head 7
    cases.append(('seven characters read as eight', seven, None, reads_of([gained(seven[0], 4), gained(seven[0], 6), list(seven[0])]), 1, 32768,
                  FULL, [(0, 1, FULL, 1), (0, 1, FULL, 1), (0, 0, 0, 1)], [8, 10, 0]))
    return cases


@pytest.mark.parametrize('case', constructed(), ids=lambda c: c[0])
def test_constructed_reads(case):
    name, entries, confuse, reads, mm, mc, gap, want, codes = case
    m, a = spec(entries, confuse, reads, mm, mc, 1, gap)
    assert m[0].tolist() == [list(w) for w in want] and a[0].tolist() == codes, (name, m[0].tolist(), a[0].tolist())
    lm, la = indel_loops(entries, confuse, *reads, mm, mc, 1, gap, dp=True)
    assert np.array_equal(m, lm) and np.array_equal(a, la)


def test_every_code_wins_and_wins_alone():
    """In the first constructed case read c is won by code c, and no other alignment reaches its (cost, mismatches)."""
    _, entries, confuse, reads, mm, mc, gap, _, codes = constructed()[0]
    end = constructed()[1]
    for ended_i, g, want in [(reads[0][0, j], gap, codes[j]) for j in range(11)] + [(end[3][0][0, 0], end[6], 11)]:
        al = alignments(lambda p, col: cell(entries, confuse, 0, col, ended_i[4:], np.ones(8, f32), p), g)
        assert pick(al) == want and sorted(al).count(al[want]) == 1, (want, al)


@pytest.mark.parametrize('wrong', ['head7_compared', 'gap_is_no_mismatch', 'heads01_shifted', 'code_order_reversed', 'cost_alone', 'r_from_k'])
def test_the_constructed_set_catches_wrong_emulations(wrong):
    caught = []
    for name, entries, confuse, reads, mm, mc, gap, _, _ in constructed():
        m, a = spec(entries, confuse, reads, mm, mc, 1, gap)
        wm, wa = indel_loops(entries, confuse, *reads, mm, mc, 1, gap, wrong=wrong)
        if not (np.array_equal(m, wm) and np.array_equal(a, wa)):
            caught.append(name)
    assert caught, wrong


# ---- random data: the spec against the loops and the dynamic programme --------------------------------------------------------------------
@pytest.mark.parametrize('seed', range(4))
def test_indel_np_against_the_loops_and_the_dp(seed):
    rng = np.random.default_rng(300 + seed)
    N, max_ended = int(rng.integers(1, 40)), 3
    entries, confuse, ended_i, ended_f, ended_count = C.random_watch_case(50 + seed, N, [3, 0, 5, -2, 1], max_ended, confuse=seed % 2 == 0)
    # plant shifted copies of some reads so that shifted alignments win, not only exist
    for e in range(0, N, 3):
        src = ended_i[int(rng.choice([0, 2, 4])), 0, 4:]
        if ((src >= 0) & (src < 64)).all():
            k = int(rng.integers(2, 7))
            entries[e] = lost(src, k, 5) if rng.random() < 0.5 else gained(src, k, 5)
    shifted = 0
    for mm, mc, gap in ((1, 32768, FULL), (2, 9000, 1500), (8, 32768, 0), (3, int(rng.integers(0, 12000)), int(rng.integers(0, FULL + 1)))):
        got, want = spec(entries, confuse, (ended_i, ended_f, ended_count), mm, mc, 1, gap), \
            indel_loops(entries, confuse, ended_i, ended_f, ended_count, mm, mc, 1, gap, dp=True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (mm, mc, gap)
        assert not got[1][got[0][:, :, 0] < 0].any()
        shifted += int((got[1] > 0).sum())
    assert shifted > 0


@pytest.mark.parametrize('seed', range(3))
def test_indel_0_is_the_positional_match(seed):
    from yolov6.utils.watch import watch_match_np
    case = C.random_watch_case(70 + seed, 45, [3, 0, 4, -2, 1], 4, confuse=seed != 1)
    for mm, mc in ((0, 32768), (1, 32768), (2, 3000), (8, 32768)):
        want = C.match_loops(*case, mm, mc)
        assert np.array_equal(watch_match_np(*case, mm, mc), want)
        for gap in (0, 777, FULL):
            m, a = watch_match_np(*case, mm, mc, 0, gap, align=True)
            assert np.array_equal(m, want) and a.shape == (5, 4) and not a.any()
            assert np.array_equal(watch_match_np(*case, mm, mc, indel=0, gap_cost=gap), want)


def test_the_checks_and_the_names():
    from yolov6.utils import watch
    assert watch.gap_units(None) == FULL and watch.gap_units(1.0) == FULL and watch.gap_units(0) == 0 and watch.gap_units(7) == FULL
    assert watch.gap_units(-1) == 0 and watch.gap_units(0.5) == 2048 and watch.gap_units(1 / 8192) == 1 and watch.gap_units(0.9 / 8192) == 0
    with pytest.raises(ValueError):
        watch.gap_units(float('nan'))
    assert watch.check_indel(0, 0) == (0, 0) and watch.check_indel(1, FULL) == (1, FULL) and watch.check_indel(True, 5) == (1, 5)
    for bad in ((2, 0), (-1, 0), (0.5, 0), (1, -1), (1, FULL + 1), (1, 0.5)):
        with pytest.raises(ValueError):
            watch.check_indel(*bad)
    assert [watch.align_text(c) for c in range(12)] == ['-', 'del@2', 'del@3', 'del@4', 'del@5', 'del@6', 'ins@2', 'ins@3', 'ins@4', 'ins@5',
                                                        'ins@6', 'end']
    with pytest.raises(ValueError):
        watch.align_text(12)
    wl = watch.WatchlistNp(np.array([ENTRY], np.uint8))
    reads = reads_of([lost(ENTRY, 3)])
    assert wl.match(*reads).tolist() == [[list(C.NONE)]] and wl.last_align is None
    assert wl.match(*reads, indel=1).tolist() == [[[0, 1, FULL, 1]]] and wl.last_align.tolist() == [[2]]
    assert wl.match(*reads, indel=1, gap_cost=0.25).tolist() == [[[0, 1, 1024, 1]]]
    assert wl.match(*reads, max_cost=0.5, indel=1).tolist() == [[list(C.NONE)]] and wl.last_align.tolist() == [[0]]


# ---- PlateTrackerNp ------------------------------------------------------------------------------------------------------------------------
def test_tracker_np_defaults_leave_every_output_as_before():
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.watch import WatchlistNp, cost_units, watch_match_np
    kw = dict(max_tracks=16, max_age=2, expand=0.5)
    calls = T.random_track_case(2)
    entries = C.watchlist_for(calls, 3, **kw)
    entries[1::4] = [lost(r, 2 + i % 5, 5) for i, r in enumerate(entries[0::4][:len(entries[1::4])])]
    wl = WatchlistNp(entries)
    plain, dflt, on = PlateTrackerNp(3, **kw), PlateTrackerNp(3, **kw), PlateTrackerNp(3, **kw)
    plain.enable_watch(wl, 2, 1.25)
    plain.enable_live_watch(wl, 1, 2, 1.25)
    dflt.enable_watch(wl, 2, 1.25, indel=0, gap_cost=None)
    dflt.enable_live_watch(wl, 1, 2, 1.25, indel=0, gap_cost=0.5)
    on.enable_watch(wl, 2, 1.25, indel=1, gap_cost=0.5)
    on.enable_live_watch(wl, 1, 2, 1.25, indel=1, gap_cost=0.5)
    shifted = 0
    for det, count, stream_of, flush in calls:
        a, b, c = (t.update(det, count, stream_of, flush, 5) for t in (plain, dflt, on))
        for x, y, z in zip(a, b, c):
            assert np.array_equal(x.view(np.int32), y.view(np.int32)) and np.array_equal(x.view(np.int32), z.view(np.int32))
        assert np.array_equal(plain.last_watch, dflt.last_watch) and np.array_equal(plain.last_live, dflt.last_live)
        assert np.array_equal(plain._live.memo, dflt._live.memo)
        assert dflt.last_watch_align is None and dflt.last_live_align is None and plain.last_watch_align is None
        for x, y in zip(plain.last_live_reads, on.last_live_reads):               # the queries do not depend on the measure
            assert np.array_equal(x.view(np.int32), y.view(np.int32))
        m, al = watch_match_np(entries, None, c[2], c[3], c[4], 2, cost_units(1.25), 1, 2048, align=True)
        assert np.array_equal(on.last_watch, m) and np.array_equal(on.last_watch_align, al) and on.last_live_align.shape == (3, 16)
        shifted += int((al > 0).sum()) + int((on.last_live_align > 0).sum())
    assert shifted > 0
    on.enable_watch(None)
    on.enable_live_watch(None)
    assert on.last_watch_align is None and on.last_live_align is None
    for bad in (dict(indel=2), dict(indel=1, gap_cost=float('nan'))):
        with pytest.raises(ValueError):
            on.enable_watch(wl, **bad)
        with pytest.raises(ValueError):
            on.enable_live_watch(wl, **bad)


SHIFTED_PLATE = tuple(lost(LV.PLATE, 4, 30))


def shifted_scene(trk, frames=8):
    """One car whose read is ``LV.PLATE`` without head 4, seen in every frame; per frame (live_i row 0, live_align[0, 0] or None,
    q_count)."""
    out = []
    for _ in range(frames):
        LV.step(trk, [LV.car(SHIFTED_PLATE)])
        al = trk.last_live_align
        out.append((np.asarray(trk.last_live[0, 0].tolist()), None if al is None else int(al[0, 0]), int(trk.last_live_reads[3][0])))
    return out


def test_a_shifted_read_alerts_once_and_its_code_stands():
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.watch import WatchlistNp
    wl = WatchlistNp(np.array([(9, 9, 9, 9, 9, 9, 9, 9), LV.PLATE], np.uint8))
    off, on = PlateTrackerNp(1, max_tracks=4, max_age=5), PlateTrackerNp(1, max_tracks=4, max_age=5)
    off.enable_live_watch(wl, min_hits=3)
    on.enable_live_watch(wl, min_hits=3, indel=1)
    for k, ((r0, a0, n0), (r1, a1, n1)) in enumerate(zip(shifted_scene(off), shifted_scene(on))):
        assert n0 == n1 == int(k == 2)                                         # one lookup, at min_hits; the memo holds afterwards
        assert a0 is None and r0[1] == -1                                      # positional: nothing, ever
        if k < 2:
            assert r1.tolist() == list(LV.NO_ROW) and a1 == 0
        else:
            assert r1.tolist() == [0, 1, 1, FULL, 1, int(k == 2), k + 1, 2] and a1 == 3       # del@4, fresh once, standing after
    on.reset([0])
    assert shifted_scene(on, 1)[0][1] == 0                                      # a new track below min_hits: no row, code 0


# ---- C ABI: everything is checked on the host before any launch ----------------------------------------------------------------------------
def test_watch_match_indel_rejects_bad_arguments_before_launch():
    """Fake device addresses: a launch would fault, so LP_ERR_ARG proves the host check came first."""
    from yolov6.hip import abi
    lib = abi.load()
    v = lambda p: ctypes.c_void_p(p) if p else None   # noqa: E731
    S, M = 3, 5
    need = lib.lp_watch_workspace_bytes(S, M)

    def call(entries=0x100000, n=1000, confuse=0x200000, ei=0x300000, ef=0x310000, ec=0x320000, S=S, M=M, mm=1, mc=4096, indel=1, gap=4096,
             match=0x330000, align=0x340000, ws=0x400000, ws_bytes=need):
        return lib.lp_watch_match_indel(v(entries), n, v(confuse), v(ei), v(ef), v(ec), S, M, mm, mc, indel, gap, v(match), v(align), v(ws),
                                        ws_bytes, None)

    err = lambda: lib.lp_last_error()   # noqa: E731
    assert call(n=-1) == LP_ERR_ARG and b'n_entries' in err() and call(n=(1 << 24) + 1) == LP_ERR_ARG and b'16777216' in err()
    assert call(S=0) == LP_ERR_ARG and b'n_streams' in err() and call(M=-1) == LP_ERR_ARG
    assert call(S=1 << 20, M=1 << 10) == LP_ERR_ARG and b'2^31' in err()
    for k, bad in (('mm', -1), ('mm', 9), ('mc', -1), ('mc', 32769)):
        assert call(**{k: bad}) == LP_ERR_ARG and b'max_mismatch' in err(), (k, bad)
    for k, bad in (('indel', -1), ('indel', 2), ('gap', -1), ('gap', 4097)):
        assert call(**{k: bad}) == LP_ERR_ARG and b'indel' in err() and b'gap_cost' in err(), (k, bad)
        assert call(**{k: bad}, M=0) == LP_ERR_ARG                             # even with nothing to write
    for k in ('entries', 'ei', 'ef', 'ec', 'match', 'align', 'ws'):
        assert call(**{k: 0}) == LP_ERR_ARG and b'null' in err(), k
        assert call(**{k: 0}, indel=0) == LP_ERR_ARG and b'null' in err(), k
    assert call(n=0, ec=0) == LP_ERR_ARG and call(n=0, match=0) == LP_ERR_ARG and call(n=0, align=0) == LP_ERR_ARG and b'null' in err()
    assert call(entries=0x100004) == LP_ERR_ARG and b'aligned' in err() and call(confuse=0x200002) == LP_ERR_ARG
    assert call(ws=0x400008) == LP_ERR_ARG and b'aligned' in err()
    assert call(ws_bytes=need - 1) == LP_ERR_ARG and b'workspace' in err() and call(ws_bytes=0) == LP_ERR_ARG
    for k, at in (('match', 0x100000 + 7992), ('align', 0x100000 + 7996), ('align', 0x200000 + 12287), ('align', 0x300000 + S * M * 48 - 4),
                  ('align', 0x310000), ('align', 0x320000 + 8), ('align', 0x330000 + S * M * 16 - 4), ('match', 0x340000 + S * M * 4 - 4),
                  ('ws', 0x340000 + 16), ('align', 0x400000 + need - 4), ('ws', 0x330000 + 16)):
        assert call(**{k: at}) == LP_ERR_ARG and b'overlap' in err(), (k, hex(at))
    assert call(M=0) == 0 and call(M=0, n=0, entries=0, ei=0, ef=0, ec=0, match=0, align=0, ws=0, ws_bytes=0) == 0   # nothing to write: no launch


def test_watch_live_indel_rejects_bad_arguments_before_launch():
    from yolov6.hip import abi
    lib = abi.load()
    v = lambda p: ctypes.c_void_p(p) if p else None   # noqa: E731
    S, T_ = 2, 16
    L = S * T_
    need, old = lib.lp_watch_live_indel_workspace_bytes(S, T_), lib.lp_watch_live_workspace_bytes(S, T_)
    assert need == old + L * 4 and need % 16 == 0
    assert lib.lp_watch_live_indel_workspace_bytes(0, T_) == 0 and lib.lp_watch_live_indel_workspace_bytes(S, 129) == 0

    def call(state=0x100000, S=S, T_=T_, ncls=T.NCLS, min_hits=3, memo=0x200000, entries=0x300000, n=1000, confuse=0x310000, mm=1, mc=4096,
             indel=1, gap=4096, q_i=0x400000, q_f=0x410000, q_slot=0x420000, q_count=0x430000, live=0x440000, align=0x450000, ws=0x500000,
             ws_bytes=need):
        nc = (ctypes.c_int * 8)(*ncls) if ncls is not None else None
        return lib.lp_watch_live_indel(v(state), S, T_, nc, min_hits, v(memo), v(entries), n, v(confuse), mm, mc, indel, gap, v(q_i), v(q_f),
                                       v(q_slot), v(q_count), v(live), v(align), v(ws), ws_bytes, None)

    err = lambda: lib.lp_last_error()   # noqa: E731
    assert call(S=0) == LP_ERR_ARG and b'n_streams' in err() and call(T_=129) == LP_ERR_ARG and b'lp_watch_live_indel' in err()
    assert call(ncls=None) == LP_ERR_ARG and b'ncls' in err() and call(min_hits=0) == LP_ERR_ARG and b'min_hits' in err()
    for k, bad in (('mm', 9), ('mc', 32769)):
        assert call(**{k: bad}) == LP_ERR_ARG and b'max_mismatch' in err(), (k, bad)
    for k, bad in (('indel', -1), ('indel', 2), ('gap', -1), ('gap', 4097)):
        assert call(**{k: bad}) == LP_ERR_ARG and b'indel' in err() and b'gap_cost' in err(), (k, bad)
    for k in ('state', 'memo', 'entries', 'q_i', 'q_f', 'q_slot', 'q_count', 'live', 'align', 'ws'):
        assert call(**{k: 0}) == LP_ERR_ARG and b'null' in err(), k
    assert call(ws_bytes=need - 1) == LP_ERR_ARG and b'workspace' in err() and call(ws_bytes=old) == LP_ERR_ARG
    for k, at in (('align', 0x440000 + L * 32 - 4), ('align', 0x200000 + L * 32 - 4), ('align', 0x300000), ('align', 0x500000 + need - 4),
                  ('live', 0x450000), ('ws', 0x450000 + 16), ('align', 0x100000)):
        assert call(**{k: at}) == LP_ERR_ARG and b'overlap' in err() and b'live_align' in err(), (k, hex(at))


def test_the_header_and_the_bindings_agree():
    from yolov6.hip import abi
    header = open(os.path.join(REPO, 'include', 'lp_hip.h')).read()
    assert '#define LP_WATCH_MAX_GAP_COST %d' % abi.LP_WATCH_MAX_GAP_COST in header and abi.LP_WATCH_MAX_GAP_COST == FULL
    assert '#define LP_WATCH_INDEL_QUERY_BLOCK %d ' % abi.LP_WATCH_INDEL_QUERY_BLOCK in header
    for name in ('lp_watch_match_indel', 'lp_watch_live_indel', 'lp_watch_live_indel_workspace_bytes'):
        proto = header[header.index('\n%s %s(' % ('size_t' if name.endswith('_bytes') else 'int', name)):]
        args = [a for a in proto[proto.index('(') + 1:proto.index(');')].split(',')]
        assert len(args) == len(abi.SYMBOLS[name][1]), name
        for a, t in zip(args, abi.SYMBOLS[name][1]):
            a = a.split('/*')[0]
            want = ctypes.c_int if ('*' not in a and 'size_t' not in a) else ctypes.c_size_t if 'size_t' in a else None
            assert want is None or t is want, (name, a)


# ---- tools/infer.py --watch-indel on the CPU path ---------------------------------------------------------------------------------------
def test_infer_watch_indel_columns_appear_only_under_the_flag(tmp_path, monkeypatch):
    from PIL import Image
    from yolov6.utils.synth import build_synthetic
    from yolov6.utils.watch import align_text, entry_text, watch_match_np
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
    _, _, ended = T.track_by_hand([d.numpy() for d in untracked], 20, max_tracks=64, match_thres=0.25, new_thres=0.0, expand=0.25,
                                  max_age=2, ncls=m)                           # the records behind plates.txt
    plates = T.plate_lines(ended)
    reads, shares = np.array([ri[4:12] for ri, _ in ended]), np.array([rf[:8] for _, rf in ended], f32)
    # the list: read 0 as an entry that has one character more at head 3 (so read 0 lost it), and read 0 itself
    longer = list(reads[0][:3]) + [(int(reads[0][3]) + 1) % 37] + list(reads[0][3:7])
    rows = [longer, list(reads[0])]
    entries = np.array(rows, np.uint8)
    wl = tmp_path / 'watch.txt'
    wl.write_text('\n'.join(entry_text(r) for r in rows) + '\n')
    common = dict(watchlist=str(wl), watch_live=True, watch_live_min_hits=1, **kw)
    infer.run(save_dir=str(tmp_path / 'o1'), **common)
    infer.run(save_dir=str(tmp_path / 'o2'), watch_indel=True, watch_gap_cost=0.0, **common)
    for name in ('tracks.txt', 'plates.txt'):
        assert (tmp_path / 'o2' / name).read_bytes() == (tmp_path / 'o1' / name).read_bytes()
    assert (tmp_path / 'o1' / 'plates.txt').read_text().splitlines() == plates
    ended_i, ended_f = np.zeros((1, len(reads), 12), np.int32), np.zeros((1, len(reads), 12), f32)
    ended_i[0, :, 4:], ended_f[0, :, :8] = reads, shares
    old = watch_match_np(entries, None, ended_i, ended_f, [len(reads)], 1, 32768)[0]
    new, codes = (x[0] for x in watch_match_np(entries, None, ended_i, ended_f, [len(reads)], 1, 32768, 1, 0, align=True))
    from yolov6.utils.track import plate_text

    def lines(match, codes=None):
        return ['%s %s %d %s %d %d %d' % (' '.join(line.split()[:3]), plate_text(reads[k]), e, entry_text(entries[e]), mi, co, n) +
                ('' if codes is None else ' ' + align_text(codes[k]))
                for k, (line, (e, mi, co, n)) in enumerate(zip(plates, match.tolist())) if e >= 0]
    assert (tmp_path / 'o1' / 'hits.txt').read_text().splitlines() == lines(old)
    assert (tmp_path / 'o2' / 'hits.txt').read_text().splitlines() == lines(new, codes)
    assert old[0].tolist() == [1, 0, 0, 1] and new[0].tolist() == [0, 1, 0, 2] and codes[0] == 2        # the free gap sorts before index 1
    a1, a2 = ((tmp_path / sub / 'alerts.txt').read_text().splitlines() for sub in ('o1', 'o2'))
    cols = 7 + 2 * 8                                                           # without name lists a text is its eight ids
    assert a1 and a2 and all(len(x.split()) == cols for x in a1) and all(len(x.split()) == cols + 1 for x in a2)
    assert {x.split()[-1] for x in a2} <= {align_text(c) for c in range(12)} and any(x.endswith(' del@3') for x in a2)
    with pytest.raises(ValueError, match='watchlist'):
        infer.run(save_dir=str(tmp_path / 'o3'), watch_indel=True, **kw)
