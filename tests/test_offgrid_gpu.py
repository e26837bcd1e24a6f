"""The tracker, the cross-tile merge and the share quantiser on the GPU, off the grid on which fp32 arithmetic is exact: lp_track_update,
lp_track_update_hold (and the zones and speed updates behind it), lp_merge_tiles, lp_watch_match, lp_watch_live and lp_sight_update
against their numpy specifications, bit for bit, on the inputs of tests/offgrid.py -- full-mantissa twins of the shipped random
cases and the constructed cases on which one fused multiply-add, another summation order, a reciprocal or a float compare decides
otherwise (tests/test_offgrid_cpu.py shows that each of them would).  The comparing helpers are those of the tests of each kernel.
Every case run is appended to offgrid.log in the folder of the test logs."""
import os

import numpy as np
import pytest
import torch

import lp_testing as L
import offgrid as O
import test_speed_cpu as P
import test_track_cpu as C
import test_watch_cpu as W
import test_watch_live_cpu as WLC
import test_zones_cpu as Z
from test_all_on_gpu import AllOnGpu, assert_runs_equal
from test_hold_gpu import _assert_hold_equal, _run_both as _run_both_hold
from test_sight_gpu import GpuLog
from test_tiles_gpu import _assert_merge_equal
from test_track_gpu import _run_both
from test_watch_gpu import gpu_match
from test_watch_live_gpu import outputs_gpu as live_outputs_gpu, poison as poison_live

pytestmark = pytest.mark.gpu
f32 = np.float32
LOG_NAME = 'offgrid.log'


def _log(kernel, what, aimed_at=None):
    with open(os.path.join(L.log_dir(), LOG_NAME), 'a') as f:
        f.write('%s  %s%s\n' % (kernel, what, '  aimed at: ' + aimed_at if aimed_at else ''))


def _kw_text(kw):
    return ' '.join('%s=%r' % (k, v) for k, v in sorted(kw.items()))


# ---- lp_track_update -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('expand,thres', list(zip(O.EXPANDS, O.MATCH_THRES)), ids=['e0.3', 'e0.1'])
@pytest.mark.parametrize('name', list(O.TWINS))
def test_track_update_equals_numpy_spec_on_off_grid_twins(name, expand, thres):
    calls, S, kw = O.twin_case(name, expand, thres)
    Bs = O.TWINS[name][4]
    if max(Bs) > 64:                                                   # a stream has frames on both sides of a launch split
        so = calls[0][2]
        assert any(s >= 0 and s in so[:64] and s in so[64:] for s in range(S))
    ref = _run_both(calls, S, 6, **kw)
    assert ref.stats['matched'] > 0 and ref.stats['ended'] > 0 and ref.stats['ties'] > 0 and ref.dropped.sum() > 0
    _log('lp_track_update', 'twin %s  %s  pairs %d matched %d' % (name, _kw_text(kw), ref.stats['pairs'], ref.stats['matched']))


def test_track_update_full_matrix_off_grid():
    """128 slots x 128 rows, every pair above the threshold, fractional jitter and full-mantissa confidences: 16384 keys of
    near-equal IoUs through the sort and the settle."""
    kw = dict(max_tracks=128, match_thres=0.3, new_thres=0.0, expand=0.3, max_age=0)
    ref = _run_both(O.full_matrix_calls(), 1, 128, **kw)
    assert ref.stats['pairs'] == 2 * 16384 and ref.stats['matched'] == 2 * 128
    _log('lp_track_update', 'full matrix 128 x 128  %s  ties %d' % (_kw_text(kw), ref.stats['ties']))


def test_track_update_equals_numpy_spec_on_every_constructed_case():
    n = 0
    for kind, cases in O.tracker_cases().items():
        assert len(cases) >= O.MIN_INSTANCES, kind
        for k, c in enumerate(cases):
            ref = _run_both(c['calls'], c['n_streams'], c['max_ended'], **c['kw'])
            assert ref.stats['ended'] >= 1
            _log('lp_track_update', '%s #%d (%s)  %s' % (kind, k, c['kind'], _kw_text(c['kw'])), c['defect'])
            n += 1
    assert n >= 8 * O.MIN_INSTANCES


# ---- lp_track_update_hold, and the zones and speed updates behind it ------------------------------------------------------------------------------
def test_track_update_hold_equals_numpy_spec_on_held_rows_with_k_3():
    """Twelve streams near the origin, tracks held at misses = 3 after a velocity divided by 3: tests/test_offgrid_cpu.py shows that
    a fused box + vel * k and a velocity through a reciprocal each change words of det_hold on this scene."""
    calls = O.held_calls()
    ref, held = _run_both_hold(calls, O.HELD_STREAMS, 6, min_hits=1, max_misses=None, **O.HELD_KW)
    assert held >= 40 and ref.stats['matched'] == 36 and ref.next_id.tolist() == [1] * O.HELD_STREAMS
    _log('lp_track_update_hold', 'held rows, %d streams  %s  held %d' % (O.HELD_STREAMS, _kw_text(O.HELD_KW), held), 'held_fma, vel_rcp')


def test_held_scene_with_zones_and_speed_equals_the_numpy_chain():
    """The same calls with zones and speed behind the hold.  Both read the stored box only (``offgrid.held_maps``): this covers their
    arithmetic on off-grid stored boxes, not the held geometry."""
    from yolov6.hip import runtime
    S = O.HELD_STREAMS
    lines, zones, planes = O.held_maps()
    trk = runtime.PlateTracker(S, device='cuda', **O.HELD_KW)
    trk.enable_hold()
    trk.enable_zones(runtime.ZoneMap(S, lines, zones), min_hits=1)
    trk.enable_speed(runtime.GroundPlane(S, planes), min_hits=1, confirm=2)
    ref, wants = O.run_held_addons_np()
    n_zone = n_speed = 0
    for k, ((det, count, stream_of, flush), want) in enumerate(zip(O.held_calls(), wants)):
        trk.update(torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda(), stream_of, flush, 6)
        torch.cuda.synchronize()
        _assert_hold_equal(trk.last_hold[:1], (want['det_hold'],), [], 'call %d' % k)
        Z.assert_same(tuple(t.cpu().numpy() for t in trk.last_zone + (trk.zone_memo,)),
                      tuple(want[n] for n in ('zone_ev', 'zone_count', 'zone_occ', 'zone_totals', 'zone_memo')), 'call %d' % k)
        P.assert_same(tuple(t.cpu().numpy() for t in trk.last_speed + (trk.speed_memo(),)),
                      tuple(want[n] for n in ('speed_i', 'speed_ev', 'speed_count', 'speed_memo')), 'call %d' % k)
        n_zone += int(want['zone_count'].sum())
        n_speed += int((want['speed_i'][:, :, 1] > 0).sum())
    assert n_zone > 0 and n_speed > 0
    _log('lp_track_update_hold + lp_zone_update + lp_speed_update', 'held rows, %d streams  %s  zone events %d' % (S, _kw_text(O.HELD_KW), n_zone))


# ---- lp_merge_tiles --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('metric', ['iou', 'ios'])
def test_merge_tiles_equals_numpy_spec_off_the_grid(metric):
    total = 0
    for seed in range(3):
        case = O.offgrid_merge_case(seed)                   # two frames of five and three tiles, max_det_t = 16
        for border in (-1, 1):
            for thres in O.MERGE_THRES:
                n = _assert_merge_equal(case, thres, 40, metric, border)
                _log('lp_merge_tiles', 'random seed %d  metric=%s thres=%g border=%d  kept %d' % (seed, metric, thres, border, n))
                total += n
    assert total > 0
    n = 0
    for kind, cases in O.merge_cases().items():
        assert len(cases) >= O.MIN_INSTANCES, kind
        for k, c in enumerate(cases):
            if c['metric'] != metric:
                continue
            for border in (-1, 1):
                kept = _assert_merge_equal(c['case'], c['thres'], c['max_det'], metric, border)
                _log('lp_merge_tiles', '%s #%d  metric=%s thres=%r border=%d  kept %d' % (kind, k, metric, c['thres'], border, kept), c['defect'])
                n += 1
    assert n >= 2 * 2 * O.MIN_INSTANCES


# ---- the share quantiser: lp_watch_match, lp_sight_update, lp_watch_live --------------------------------------------------------------------------
def _twin_records():
    """(calls, n_streams, parameters, [(ended_i, ended_f, ended_count) per call]) of the off-grid tracker scene, from the specification."""
    calls, S, kw = O.twin_case('s3-t4-d20', O.EXPANDS[0], O.MATCH_THRES[0])
    outs = O.run_tracker_np(calls, S, 6, **kw)[1]
    return calls, S, kw, [(o['ended_i'], o['ended_f'], o['ended_count']) for o in outs]


def test_watch_match_at_the_quantiser_edges_and_on_the_shares_of_the_off_grid_scene():
    from yolov6.utils.watch import position_weight, watch_match_np
    shares = O.quantiser_shares()
    entries, ended_i, ended_f, ended_count = O.edge_reads(shares)
    got = gpu_match(entries, None, ended_i, ended_f, ended_count, 1, 32768)
    assert np.array_equal(got, watch_match_np(entries, None, ended_i, ended_f, ended_count, 1, 32768))
    assert got[0].tolist() == [[0, 1, 16 * int(q), 8] for q in position_weight(shares)]
    _log('lp_watch_match', 'quantiser edges k / 255, one ulp below and above, k in %s' % (O.QUANT_KS,), 'quant_rint (quant_f64 is the same function)')
    calls, S, kw, records = _twin_records()
    entries = W.watchlist_for(calls, S, **kw)
    confuse = W.random_confuse(np.random.default_rng(4))
    hits = shares_seen = 0
    for ended_i, ended_f, ended_count in records:
        for mm, mc in ((1, 32768), (2, 2500)):
            got, want = gpu_match(entries, confuse, ended_i, ended_f, ended_count, mm, mc), watch_match_np(entries, confuse, ended_i, ended_f, ended_count, mm, mc)
            assert np.array_equal(got, want), (mm, mc, np.argwhere(got != want)[:3])
            hits += int((want[:, :, 1] > 0).sum())
        shares_seen += int(np.clip(ended_count, 0, 6).sum())
    assert hits > 0 and shares_seen > 10                                       # reads matched with a mismatch: a cost that depends on q
    _log('lp_watch_match', 'ended records of twin s3-t4-d20  %s  reads %d' % (_kw_text(kw), shares_seen))


def test_sight_update_at_the_quantiser_edges_and_on_the_shares_of_the_off_grid_scene():
    from yolov6.utils.sight import new_state, sight_update_np
    _, ended_i, ended_f, ended_count = O.edge_reads(O.quantiser_shares(), rolled=True)
    state = new_state(64)
    log = GpuLog(state, None, None)
    for now in (3, 4):                                                         # the second call matches the reads against their own weights
        want = sight_update_np(state, None, None, ended_i, ended_f, ended_count, now, 5, 1, 8, 32768)
        got = log.update(ended_i, ended_f, ended_count, now, 5, 1, 8, 32768)
        assert np.array_equal(got, want) and np.array_equal(log.get_state(), state)
    assert (want[0, :, 0] >= 0).all() and state[0, 0] == 2 * ended_count[0]
    _log('lp_sight_update', 'quantiser edges k / 255, one ulp below and above, k in %s' % (O.QUANT_KS,), 'quant_rint (quant_f64 is the same function)')
    calls, S, kw, records = _twin_records()
    confuse = W.random_confuse(np.random.default_rng(4))
    state = new_state(40)
    log = GpuLog(state, confuse, None)
    hits = 0
    for now, (ended_i, ended_f, ended_count) in enumerate(records):
        want = sight_update_np(state, confuse, None, ended_i, ended_f, ended_count, now, 6, 1, 8, 32768)
        got = log.update(ended_i, ended_f, ended_count, now, 6, 1, 8, 32768)
        assert np.array_equal(got, want) and np.array_equal(log.get_state(), state), now
        hits += int((want[:, :, 1] > 0).sum())
    assert hits > 0 and state[0, 0] > 10
    _log('lp_sight_update', 'ended records of twin s3-t4-d20  %s  appended %d' % (_kw_text(kw), state[0, 0]))


def test_watch_live_at_the_reachable_quantiser_edges_and_on_the_off_grid_scene():
    from yolov6.hip import runtime
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.watch import WatchlistNp
    frames, reached = O.share_scene()                                          # the shares a vote can produce: k in 127, 128, 254
    det, count = C.frames_of(frames, 8)
    entries = np.concatenate([O.edge_reads([0])[0], np.full((1, 8), 9, np.uint8)])
    kw = dict(O.HELD_KW, new_thres=0.0)
    trk, ref = runtime.PlateTracker(1, device='cuda', **kw), PlateTrackerNp(1, **kw)
    trk.enable_live_watch(runtime.Watchlist(entries), min_hits=3, max_mismatch=8)
    ref.enable_live_watch(WatchlistNp(entries), min_hits=3, max_mismatch=8)
    for f in range(3):
        poison_live(trk)
        trk.update(torch.from_numpy(det[f:f + 1]).cuda(), torch.from_numpy(count[f:f + 1]).cuda(), [0])
        ref.update(det[f:f + 1], count[f:f + 1], [0])
        WLC.assert_same(live_outputs_gpu(trk), WLC.outputs_np(ref), 'share scene, frame %d' % f)
    q_f, q_count = ref.last_live_reads[1], ref.last_live_reads[3]
    assert q_count[0] == len(reached) and np.array_equal(q_f[0, :len(reached), :8].view(np.int32), reached.view(np.int32))
    _log('lp_watch_live', 'shares voted to k / 255 and its neighbours: %s' % sorted(set(reached.reshape(-1).tolist())), 'quant_rint')
    calls, S, kw = O.twin_case('s3-t4-d20', O.EXPANDS[0], O.MATCH_THRES[0])
    entries = W.watchlist_for(calls, S, **kw)
    confuse = W.random_confuse(np.random.default_rng(4))
    trk, ref = runtime.PlateTracker(S, device='cuda', **kw), PlateTrackerNp(S, **kw)
    trk.enable_live_watch(runtime.Watchlist(entries, confuse), min_hits=2, max_mismatch=2, max_cost=1.5)
    ref.enable_live_watch(WatchlistNp(entries, confuse), min_hits=2, max_mismatch=2, max_cost=1.5)
    fresh = hits = 0
    for k, (det, count, stream_of, flush) in enumerate(calls):
        poison_live(trk)
        trk.update(torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda(), stream_of, flush)
        ref.update(det, count, stream_of, flush)
        WLC.assert_same(live_outputs_gpu(trk), WLC.outputs_np(ref), 'twin, call %d' % k)
        fresh += int(ref.last_live_reads[3].sum())
        hits += int((ref.last_live[:, :, 1] >= 0).sum())
    assert fresh > 5 and hits > 0
    _log('lp_watch_live', 'twin s3-t4-d20  %s  fresh reads %d' % (_kw_text(kw), fresh))


# ---- every add-on at once ------------------------------------------------------------------------------------------------------------------------
def test_all_on_equals_the_numpy_chain_on_an_off_grid_scene():
    """The scene of tests/test_all_on_gpu.py, off the grid, through the same two chains: every returned tensor, every ``last_*``
    attribute and the frames that leave the delay line, call by call."""
    p = L.ALL_ON
    calls = O.offgrid_twin(L.all_on_scene(p['seed']), 77)
    ref, dev = L.AllOnNp(), AllOnGpu()
    names = [n for f in ('track',) + L.ALL_ON_FEATURES for n in L.ALL_ON_OUTPUTS[f]]
    ended = held = matched = 0
    for c, call in enumerate(calls):
        if c == p['reset_before']:
            ref.reset(p['reset_streams'])
            dev.reset(p['reset_streams'])
        want, got = ref.step(*call), dev.step(*call)
        assert set(got) == set(want) == set(names)
        assert_runs_equal([got], [want], names, 'off-grid all on, call %d' % c)
        ended += int(want['ended_count'].sum())
        held += int(want['count_hold'].sum() - np.clip(call[1], 0, p['max_det']).sum())
        matched += int((want['match_i'][:, :, 0] >= 0).sum())
    assert ended > 50 and held > 0 and matched > 0
    assert np.array_equal(dev.log.state.cpu().numpy(), ref.log.state) and np.array_equal(dev.trk.dropped.cpu().numpy(), ref.trk.dropped)
    _log('all add-ons', 'twin of the all-on scene  %s  ended %d held %d' % (_kw_text(p['track']), ended, held))
