"""The off-grid inputs of tests/offgrid.py, checked on the CPU with the numpy specifications alone: the generators are what they
claim to be, every search finds its cases, and -- in the idiom of ``test_wrong_emulations_are_caught`` of tests/test_jpeg_cpu.py --
every named wrong computation (a fused multiply-add, another summation order, a reciprocal, a float compare ...) changes at least
one output word on the off-grid set.  Whether it changes anything on the SHIPPED cases (integer boxes, confidences k / 8) is
printed, not asserted: mostly it does not, which is why the off-grid set exists."""
import math

import numpy as np
import pytest

import offgrid as O
import test_track_cpu as C
import test_watch_cpu as W
from test_tiles_cpu import random_case

f32, f64 = np.float32, np.float64
_memo = {}


# ---- the generators ---------------------------------------------------------------------------------------------------------------------
def test_overlap_quotient_is_the_quotient_of_the_specifications():
    from yolov6.utils.tiles import overlaps
    from yolov6.utils.track import iou_matrix
    rng = np.random.default_rng(1)
    a = O.offgrid_rows(rng, 40, extent=300.0)[:, :4]
    b = (a[rng.permutation(40)] + O.full_mantissa(rng, (40, 4), -20, 20)).astype(f32)
    a[3, 1], b[5, 2] = np.nan, np.nan
    b[7, 2] = b[7, 0] - f32(1.5)                                                  # an inverted box
    q = O.overlap_quotient(a[:, None, :], b[None, :, :])
    assert np.array_equal(q.view(np.int32), iou_matrix(a, b).view(np.int32)) and (q > 0.3).sum() > 20
    for metric in ('iou', 'ios'):
        q = O.overlap_quotient(a[:, None, :], b[None, :, :], metric)
        for thres in (0.0, 0.3, 0.45):
            for j in range(40):
                assert np.array_equal(q[:, j].astype(f64) > thres, overlaps(a, b[j], thres, metric))


def test_rows_and_twins_are_off_the_grid():
    rng = np.random.default_rng(2)
    rows = O.offgrid_rows(rng, 64)
    assert rows.dtype == f32 and O.is_off_grid(rows[:, :12]).all() and (rows[:, :12] >= 0).all() and (rows[:, :12] < 4000).all()
    assert (rows[:, 12:20] > 0).all() and (rows[:, 12:20] < 1).all()
    for v in O.HARD_CONF:
        assert (rows[:, 12:20] == v).any(), v
    assert O.HARD_CONF[1] == np.finfo(f32).tiny and 0 < O.HARD_CONF[2] < np.finfo(f32).tiny and O.HARD_CONF[0] == np.nextafter(f32(1), f32(0))
    for k in range(8):                                                            # permuted pairs: equal exact sums, other fp32 sums
        c, d = rows[2 * k, 12:20], rows[2 * k + 1, 12:20]
        assert sorted(c.tolist()) == sorted(d.tolist()) and math.fsum(c.tolist()) == math.fsum(d.tolist())
        assert O.sum_left(c) != O.sum_left(d)
    assert np.array_equal(O.sum_pairwise(rows[:, 12:20]), np.array([np.sum(r) for r in np.ascontiguousarray(rows[:, 12:20])], f32))
    calls = C.random_track_case(13, n_streams=3, max_det=20, n_obj=8, extent=500, Bs=(8, 2, 5, 7, 1, 6, 3, 4))
    twin = O.offgrid_twin(calls, 1013)
    moved = dup = 0
    for (det, count, so, fl), (tdet, tcount, tso, tfl) in zip(calls, twin):
        assert np.array_equal(count, tcount) and so == tso and fl == tfl
        for b in range(len(det)):
            n = min(max(int(count[b]), 0), det.shape[1])
            assert np.array_equal(det[b, n:], tdet[b, n:], equal_nan=True)
            for name, cols in (('box', slice(0, 4)), ('conf', slice(12, 20))):
                assert np.array_equal(np.isnan(det[b, :n, cols]), np.isnan(tdet[b, :n, cols])), name
            assert np.array_equal(det[b, :n, 12:20] == 0, tdet[b, :n, 12:20] == 0) and np.array_equal(det[b, :n, 20:], tdet[b, :n, 20:])
            box = tdet[b, :n, :4]
            assert O.is_off_grid(box[np.isfinite(box)]).all() and np.nanmax(np.abs(box - det[b, :n, :4]), initial=0) <= 0.51
            moved += int(np.isfinite(box).sum())
            for r in range(n):
                for r2 in range(r):
                    same = np.array_equal(det[b, r], det[b, r2], equal_nan=True)
                    assert same == np.array_equal(tdet[b, r], tdet[b, r2], equal_nan=True)
                    dup += same
    assert moved > 500 and dup > 5                                                # the twin moved coordinates and kept duplicate rows


TWIN_PARAMS = ((0.3, 0.37), (0.1, 0.3))


def _twin(expand, thres):
    return O.twin_case('s3-t4-d20', expand, thres)


def _random_tracker_case(name, expand, thres):
    """(calls, n_streams, parameters) of every random off-grid tracker case that tests/test_offgrid_gpu.py runs."""
    import lp_testing as L
    if name == 'full-matrix':
        return O.full_matrix_calls(), 1, dict(max_tracks=128, match_thres=0.3, new_thres=0.0, expand=0.3, max_age=0)
    if name == 'all-on':
        return O.offgrid_twin(L.all_on_scene(L.ALL_ON['seed']), 77), L.ALL_ON['n_streams'], L.ALL_ON['track']
    return O.twin_case(name, expand, thres)


@pytest.mark.parametrize('name,expand,thres', [(n,) + p for n in O.TWINS for p in TWIN_PARAMS] + [('full-matrix', 0.3, 0.3), ('all-on', 0.5, 0.3)])
def test_one_pair_in_twenty_changes_its_iou_bits_under_the_fused_denominator_tracker(name, expand, thres):
    calls, S, kw = _random_tracker_case(name, expand, thres)
    assert kw['expand'] == expand and kw['match_thres'] == thres
    with O.count_denominator_changes() as stats:
        O.run_tracker_np(calls, S, 6, **kw)
    print('%s expand %g: %d of %d overlapping pairs change their IoU bits' % (name, expand, stats['changed'], stats['pairs']))
    assert stats['pairs'] >= 40 and 20 * stats['changed'] >= stats['pairs'], stats


@pytest.mark.parametrize('seed', range(3))
def test_one_pair_in_twenty_changes_its_iou_bits_under_the_fused_denominator_merge(seed):
    from yolov6.utils.tiles import merge_tiles_np
    case = O.offgrid_merge_case(seed)
    assert max(sum(1 for t in case[2] if t[0] == f) for f in range(2)) <= 6 and case[0].shape[1] == 16
    for thres in O.MERGE_THRES:
        with O.count_denominator_changes() as stats:
            out = merge_tiles_np(*case, thres, 40, 'iou', -1)
        print('merge seed %d thres %g: %d of %d overlapping pairs change their IoU bits' % (seed, thres, stats['changed'], stats['pairs']))
        assert stats['pairs'] >= 20 and 20 * stats['changed'] >= stats['pairs'], stats
        assert 0 < out[1].sum() < np.clip(case[1], 0, 16).sum()                   # something was merged away


def test_every_search_finds_its_instances():
    for kind, cases in list(O.tracker_cases().items()) + list(O.merge_cases().items()):
        assert len(cases) >= O.MIN_INSTANCES, (kind, len(cases))
    for thres in O.MATCH_THRES:                                                   # both thresholds have their nearest fp32 above them
        assert O.nearest_f32_above(thres) is not None
        assert sum(1 for c in O.tracker_cases()['exact:thr_f32'] if c['kw']['match_thres'] == thres) >= O.MIN_INSTANCES
    assert O.nearest_f32_above(0.45) is None and O.nearest_f32_above(0.3) == f32(0.3)
    swaps = O.tracker_cases()
    assert sum(c['kind'] == 'swap' for c in swaps['swap:expand_fma']) >= O.MIN_INSTANCES     # mirrored pairs, exact in fp32


def test_share_scene_votes_its_heads_to_the_quantiser_edges_and_a_rounding_quantiser_changes_the_live_lookup():
    """The scene the GPU test feeds lp_watch_live: the eight heads of its track end at the shares one ulp below, at and one ulp above
    k / 255 for k = 127, 128 and at and below 254 / 255 (no vote of three ids gives a share of 1 / 255, 2 / 255 or above 1); the
    live lookup's fresh read carries exactly these shares, and its cost changes under a quantiser that rounds."""
    from yolov6.utils import track, watch
    frames, reached = O.share_scene()
    shares = O.quantiser_shares()
    assert len(frames) == 3 and reached.shape == (1, 8)
    idx = [int(np.nonzero(shares.view(np.int32) == r)[0][0]) for r in reached[0].view(np.int32)]
    assert idx == [6, 7, 8, 9, 10, 11, 12, 13]                                   # QUANT_KS[2], [3]: below, at, above; [4]: below, at
    det, count = C.frames_of(frames, 8)
    entries = np.concatenate([O.edge_reads([0])[0], np.full((1, 8), 9, np.uint8)])
    live = {}
    for name in (None, 'quant_rint', 'quant_f64'):
        with O.defect(name):
            trk = track.PlateTrackerNp(1, **dict(O.HELD_KW, new_thres=0.0))
            trk.enable_live_watch(watch.WatchlistNp(entries), min_hits=3, max_mismatch=8)
            for f in range(3):
                trk.update(det[f:f + 1], count[f:f + 1], [0])
            live[name] = (trk.last_live.copy(), trk.last_live_reads[1].copy())
    q_f = live[None][1]
    assert np.array_equal(q_f[0, 0, :8].view(np.int32), reached[0].view(np.int32))
    assert live[None][0][0, 0, 1] >= 0 and live[None][0][0, 0, 5] == 1                                 # a fresh hit ...
    assert live[None][0][0, 0, 3] != live['quant_rint'][0][0, 0, 3]                                    # ... whose cost moves
    assert np.array_equal(live[None][0], live['quant_f64'][0])


def test_held_rows_notice_a_fused_shift_and_a_velocity_through_a_reciprocal():
    """The held scene lies near the origin and holds its tracks at misses = 3 after a velocity divided by 3: box + vel * 3 as one
    fused multiply-add, and the velocity as d * (1 / 3), each change words of det_hold.  (With the objects at x = 100 .. 1800 neither
    changed a word.)  The zones and speed outputs cannot move with them: they read the stored box only (``offgrid.held_maps``)."""
    runs = {}
    for name in (None, 'held_fma', 'vel_rcp'):
        with O.defect(name):
            runs[name] = O.run_held_addons_np()
    ref, want = runs[None]
    held = sum(int(o['n_held'].sum()) for o in want)
    assert ref.stats['matched'] == 36 and ref.next_id.tolist() == [1] * O.HELD_STREAMS and held >= 40       # one track a stream
    for name in ('held_fma', 'vel_rcp'):
        words = sum(int((a['det_hold'].view(np.int32) != b['det_hold'].view(np.int32)).sum()) for a, b in zip(want, runs[name][1]))
        print('%s: %d words of det_hold differ on the held scene' % (name, words))
        assert words >= 4, name
        assert O.differing(want, runs[name][1]) == ['det_hold'], name             # zones and speed see the stored boxes only
    assert sum(int(o['zone_count'].sum()) for o in want) > 0 and sum(int((o['speed_i'][:, :, 1] > 0).sum()) for o in want) > 0


def test_every_constructed_case_decides_otherwise_under_the_computation_it_is_aimed_at():
    from yolov6.utils.tiles import merge_tiles_np
    for kind, cases in O.tracker_cases().items():
        for k, c in enumerate(cases):
            got = []
            for name in (None, c['defect']):
                with O.defect(name):
                    got.append(O.run_tracker_np(c['calls'], 1, c['max_ended'], **c['kw'])[1])
            assert 'tid' in O.differing(*got), (kind, k)
    for kind, cases in O.merge_cases().items():
        for k, c in enumerate(cases):
            for border in (-1, 1):
                got = []
                for name in (None, c['defect']):
                    with O.defect(name):
                        got.append(merge_tiles_np(*c['case'], c['thres'], c['max_det'], c['metric'], border))
                assert not np.array_equal(got[0][2], got[1][2]), (kind, k, border)
                assert got[0][1][0] + got[1][1][0] in ((2, 3) if c['kind'] != 'swap' else (2,))     # one keeps both rows, or each another row


def test_exact_threshold_cases_sit_exactly_on_the_nearest_float():
    """The IoU of the deciding pair IS float32(match_thres), which lies above match_thres: (double)iou > match_thres holds."""
    from yolov6.utils import track
    for c in O.tracker_cases()['exact:thr_f32']:
        det = c['calls'][0][0]
        e = f32(c['kw']['expand'])
        iou = track.iou_matrix(track.expand_boxes(det[0, :1, :4], e), track.expand_boxes(det[1, :1, :4], e))[0, 0]
        assert iou == f32(c['kw']['match_thres']) and float(iou) > c['kw']['match_thres']
    for metric in ('iou', 'ios'):
        for c in O.merge_cases()['exact:merge_thr_f32:' + metric]:
            det_t = c['case'][0]
            q = O.overlap_quotient(O._shifted(det_t[0, 0, :4], O.MERGE_TILES[0]), O._shifted(det_t[1, 0, :4], O.MERGE_TILES[1]), metric)
            assert q == f32(c['thres']) and float(q) > c['thres']


# ---- the wrong computations are caught ------------------------------------------------------------------------------------------------------
def _tracker_sets():
    """{'offgrid': [(name, calls, n_streams, kw, hold)], 'shipped': [...]}"""
    if 'sets' not in _memo:
        off = []
        for expand, thres in TWIN_PARAMS:
            calls, S, kw = _twin(expand, thres)
            off.append(('twin e=%g' % expand, calls, S, kw, False))
        off.append(('held', O.held_calls(), O.HELD_STREAMS, O.HELD_KW, True))
        off.append(('shares', [C.frames_of(O.share_scene()[0], 8) + ([0] * 3, [1])], 1, dict(O.HELD_KW, max_tracks=8), False))
        for kind, cases in O.tracker_cases().items():
            off += [('%s #%d' % (kind, k), c['calls'], 1, c['kw'], False) for k, c in enumerate(cases)]
        shipped = []
        for seed, S, T, max_det, Bs, n_obj, extent, expand, max_age in ((11, 1, 1, 5, (1, 3, 2, 4, 1, 2), 4, 300, 0.0, 0),
                                                                         (12, 3, 4, 5, (4, 1, 8, 3, 6, 2, 5), 6, 400, 0.5, 3),
                                                                         (13, 3, 4, 20, (8, 2, 5, 7, 1, 6, 3, 4), 8, 500, 0.0, 3)):
            calls = C.random_track_case(seed, n_streams=S, max_det=max_det, n_obj=n_obj, extent=extent, Bs=Bs)
            shipped.append(('seed %d' % seed, calls, S, dict(max_tracks=T, match_thres=0.3, new_thres=0.2, expand=expand, max_age=max_age), True))
        det, count = C.frames_of(C.plate_scene()[0], 5)
        shipped.append(('plate scene', [(det, count, [0] * len(det), [1])], 1, dict(max_tracks=8, match_thres=0.3, expand=0.5, max_age=3), True))
        _memo['sets'] = dict(offgrid=off, shipped=shipped)
    return _memo['sets']


def _print_report(rows):
    """Per case which outputs differ; the constructed cases (named 'kind:defect #k') as one line per kind."""
    kinds = {}
    for name, what in rows:
        if '#' in name:
            kinds.setdefault(name.split(' ')[0], []).append(what)
        else:
            print('    %-44s %s' % (name, what))
    for kind, whats in kinds.items():
        print('    %-44s %d cases: %s' % (kind, len(whats), ' '.join(sorted(set(' '.join(whats).split())))))


def _tracker_runs(defect):
    key = ('runs', defect)
    if key not in _memo:
        with O.defect(defect):
            _memo[key] = {which: [O.run_tracker_np(calls, S, 6, hold=hold, **kw)[1] for _, calls, S, kw, hold in cases]
                          for which, cases in _tracker_sets().items()}
    return _memo[key]


@pytest.mark.parametrize('defect', O.TRACK_DEFECTS)
def test_wrong_tracker_emulations_are_caught(defect):
    want, got = _tracker_runs(None), _tracker_runs(defect)
    report = {}
    for which, cases in _tracker_sets().items():
        report[which] = [(c[0], O.differing(w, g)) for c, w, g in zip(cases, want[which], got[which])]
        report[which] = [(n, d) for n, d in report[which] if d]
    print('%s: off-grid set: %d cases differ; shipped set: %s' % (defect, len(report['offgrid']),
                                                                  ', '.join('%s (%s)' % (n, ' '.join(d)) for n, d in report['shipped']) or 'nothing differs'))
    _print_report([(n, ' '.join(d)) for n, d in report['offgrid']])
    assert report['offgrid'], defect
    aimed = [n for n, _ in report['offgrid'] if n.split(' ')[0].endswith(':' + defect)]
    if any(k.endswith(':' + defect) for k in O.tracker_cases()):
        assert len(aimed) >= O.MIN_INSTANCES, (defect, aimed)


def _merge_sets():
    if 'merge' not in _memo:
        off = [('random seed %d %s thres %g border %d' % (seed, metric, thres, border), O.offgrid_merge_case(seed), thres, 40, metric, border)
               for seed in range(3) for metric in ('iou', 'ios') for thres in O.MERGE_THRES for border in (-1, 1)]
        for kind, cases in O.merge_cases().items():
            off += [('%s #%d' % (kind, k), c['case'], c['thres'], c['max_det'], c['metric'], -1) for k, c in enumerate(cases)]
        shipped = [('seed %d %s thres %g border %d' % (seed, metric, thres, border), random_case(seed), thres, max_det, metric, border)
                   for seed in range(6) for metric in ('iou', 'ios') for thres, max_det in ((0.45, 200), (0.1, 7), (0.0, 50)) for border in (-1, 0, 3)]
        _memo['merge'] = dict(offgrid=off, shipped=shipped)
    return _memo['merge']


def _merge_runs(defect):
    from yolov6.utils.tiles import merge_tiles_np
    key = ('merge runs', defect)
    if key not in _memo:
        with O.defect(defect):
            _memo[key] = {which: [[dict(zip(('det', 'count', 'src'), merge_tiles_np(*case, thres, max_det, metric, border)))]
                                  for _, case, thres, max_det, metric, border in cases] for which, cases in _merge_sets().items()}
    return _memo[key]


@pytest.mark.parametrize('defect', O.MERGE_DEFECTS)
def test_wrong_merge_emulations_are_caught(defect):
    want, got = _merge_runs(None), _merge_runs(defect)
    report = {which: [c[0] for c, w, g in zip(cases, want[which], got[which]) if O.differing(w, g)] for which, cases in _merge_sets().items()}
    print('%s: off-grid set: %d cases differ; shipped set: %d of %d cases differ' % (defect, len(report['offgrid']), len(report['shipped']),
                                                                                   len(_merge_sets()['shipped'])))
    _print_report([(n, '') for n in report['offgrid']])
    assert report['offgrid'], defect
    assert sum((':' + defect) in n.split(' ')[0] for n in report['offgrid']) >= O.MIN_INSTANCES, report['offgrid']


# ---- the share quantiser ----------------------------------------------------------------------------------------------------------------------
def _natural_shares():
    """ended_f shares of the off-grid tracker scene."""
    calls, S, kw = _twin(*TWIN_PARAMS[0])
    outs = O.run_tracker_np(calls, S, 6, **kw)[1]
    return np.concatenate([o['ended_f'][s, :min(int(o['ended_count'][s]), 6), :8].reshape(-1) for o in outs for s in range(S)])


def test_quantiser_edges_are_quantised_by_the_rule_and_a_wrong_boundary_is_caught():
    from yolov6.utils import watch
    position_weight = watch.position_weight
    shares = O.quantiser_shares()
    want = [q for k in O.QUANT_KS for q in (k, k + 1, k + 1)]                      # k / 255 rounds up in fp32 for every k: at and above it, k + 1
    want[-2:] = [256, 256]                                                        # 1 and above: the clamp
    assert position_weight(shares).tolist() == want == [W.weight_of(s) for s in shares]
    with O.defect('quant_rint'):                                                  # rounded to nearest in place of truncated
        wrong = watch.position_weight(shares)
    assert (wrong != np.array(want)).sum() >= len(O.QUANT_KS) - 1                 # every share one ulp below k / 255 (but the clamped one)
    nat = _natural_shares()
    assert len(nat) > 100 and O.is_off_grid(nat[(nat > 0) & (nat < 1)]).mean() > 0.9
    print('quant_rint: %d of %d edge shares, %d of %d shares of the off-grid scene are quantised otherwise'
          % ((wrong != np.array(want)).sum(), len(shares), (O._weight_rint(nat) != position_weight(nat)).sum(), len(nat)))


def test_a_wrong_quantiser_is_caught_through_the_match_and_the_log():
    """The edge reads that the GPU tests feed lp_watch_match and lp_sight_update: a quantiser that rounds changes the match's costs
    and the weights the log stores; the float64 product changes neither."""
    from yolov6.utils.sight import new_state, sight_update_np
    from yolov6.utils.watch import watch_match_np
    shares = O.quantiser_shares()
    out = {}
    for name in (None, 'quant_rint', 'quant_f64'):
        with O.defect(name):
            entries, ended_i, ended_f, ended_count = O.edge_reads(shares)
            match = watch_match_np(entries, None, ended_i, ended_f, ended_count, 1, 32768)
            state = new_state(64)
            sight = sight_update_np(state, None, None, *O.edge_reads(shares, rolled=True)[1:], 3, 5, 1, 8, 32768)
            out[name] = (match, state, sight)
    assert not np.array_equal(out[None][0][:, :, 2], out['quant_rint'][0][:, :, 2]) and not np.array_equal(out[None][1], out['quant_rint'][1])
    assert all(np.array_equal(a, b) for a, b in zip(out[None], out['quant_f64']))
    assert (out[None][0][0, :, 3] == 8).all() and out[None][1][0, 0] == len(shares)


def test_a_float64_product_quantises_every_share_like_the_rule():
    """The issue's last wrong computation, floor(share * 255.0) in float64, is no wrong computation: it differs from the rule only
    for a share whose fp32 product rounds UP to an integer, and no fp32 share does (``offgrid.quantiser_shares`` has the argument).
    Checked at the only places where it could fail, the eight floats around every k / 255, and on ten million random shares."""
    from yolov6.utils.watch import position_weight
    k = np.arange(1, 256).astype(f32)
    around = (k / f32(255)).view(np.int32)[:, None] + np.arange(-4, 4, dtype=np.int32)[None, :]
    s = around.view(f32).reshape(-1)
    assert np.array_equal(O._weight_f64(s), position_weight(s))
    prod = s * f32(255.0)
    assert not ((prod == np.round(prod)) & (s.astype(f64) * 255.0 < prod)).any()      # no fp32 product rounds up to an integer
    rng = np.random.default_rng(3)
    r = rng.random(10_000_000).astype(f32)
    assert np.array_equal(O._weight_f64(r), position_weight(r))
    nat = _natural_shares()
    edge = np.array([0, 1e-42, 2, np.nan, -1, np.inf], f32)
    assert np.array_equal(O._weight_f64(nat), position_weight(nat)) and np.array_equal(O._weight_f64(edge), position_weight(edge))
