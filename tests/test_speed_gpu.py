"""Speed of live plate tracks on the GPU: lp_speed_update against its numpy specification (yolov6/utils/speed.py) on every int32 of
speed_i, speed_ev, speed_count and of the memo, call after call -- slot counts at the wave boundary of the prefix sum and the full
workgroup, one stream and three, min_hits 1 and 3, NaN and infinite boxes; hand-built tracker states for the integer root, the run on
which a fused multiply-add gives other millimetres and the validity edges; the ring, gap, span, confirm and max_events edges of the
CPU file; the clock null and given; guard words around every buffer and a byte-identical tracker state; through
PlateTracker.enable_speed over update, update_with_shots and flush_all, alone and beside the other add-ons; one graph capture with the
clock changed between replays; the argument checks; and tools/infer.py --track --speed."""
import ctypes

import numpy as np
import pytest
import torch

import test_speed_cpu as P
import test_zones_cpu as Z

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD, GUARD_WORD, POISON = 64, 0x5EADBEE, -77          # 64 int32 = 256 bytes on either side: the alignment stays
KW = dict(match_thres=0.3, new_thres=0.2, expand=0.25, max_age=2)
LP_ERR_ARG = -1
NAMES = ('state', 'S', 'T', 'ncls', 'map', 'clock', 'min_hits', 'confirm', 'memo', 'rows', 'ev', 'count', 'max_events', 'stream')


class Guarded:
    """An int32 device tensor of ``shape`` with guard words on both sides."""

    def __init__(self, shape, fill):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), GUARD_WORD, dtype=torch.int32, device='cuda')
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        self.t.fill_(fill)

    def intact(self):
        return bool((self.buf[:GUARD] == GUARD_WORD).all()) and bool((self.buf[self.buf.numel() - GUARD:] == GUARD_WORD).all())


class SpeedCall:
    """lp_speed_update called directly on a tracker state (an int32 device tensor), with guarded buffers of its own."""

    def __init__(self, n_streams, max_tracks, ground, min_hits=1, confirm=2, ncls=None):
        from yolov6.hip import abi
        from yolov6.utils.track import DEFAULT_NCLS
        self.lib, self.S, self.T, self.ground, self.min_hits, self.confirm = abi.load(), n_streams, max_tracks, ground, min_hits, confirm
        assert self.lib.lp_speed_state_bytes(n_streams, max_tracks) == n_streams * max_tracks * 48 * 4
        self.ncls = (ctypes.c_int * 8)(*(DEFAULT_NCLS if ncls is None else ncls))
        self.memo = Guarded((n_streams, max_tracks, 48), 0)
        self.rows, self.count = Guarded((n_streams, max_tracks, 8), POISON), Guarded((n_streams,), POISON)
        self.ev = {}

    def args(self, state, clock, n_events, /, **over):
        """(the guarded speed_ev of ``n_events`` lines, the arguments of the call with ``over`` replacing some)."""
        from yolov6.hip.runtime._base import _dptr, _stream_ptr
        max_events = n_events
        ev = self.ev.get(max_events)
        if ev is None:
            ev = self.ev[max_events] = Guarded((self.S, max_events, 12), POISON)
        a = dict(state=_dptr(state), S=self.S, T=self.T, ncls=self.ncls, map=_dptr(self.ground.packed), clock=_dptr(clock), min_hits=self.min_hits,
                 confirm=self.confirm, memo=_dptr(self.memo.t), rows=_dptr(self.rows.t), ev=ctypes.c_void_p(ev.buf.data_ptr() + 4 * GUARD),
                 count=_dptr(self.count.t), max_events=max_events, stream=_stream_ptr(state.device))
        assert tuple(a) == NAMES
        a.update(over)
        return ev, tuple(a.values())

    def __call__(self, state, clock=None, max_events=None):
        max_events = self.T if max_events is None else max_events
        for g in (self.rows, self.count):
            g.t.fill_(POISON)
        ev, args = self.args(state, clock, max_events)
        ev.t.fill_(POISON)
        before = state.clone()
        assert self.lib.lp_speed_update(*args) == 0, self.lib.lp_last_error()
        torch.cuda.synchronize()
        assert torch.equal(before, state), 'the tracker state was written'
        for name, g in (('memo', self.memo), ('speed_i', self.rows), ('speed_ev', ev), ('speed_count', self.count)):
            assert g.intact(), 'guard words of %s' % name
        return tuple(g.t.cpu().numpy() for g in (self.rows, ev, self.count, self.memo))


def one_stream(calls):
    """The calls of ``Z.zone_calls`` with every frame on stream 0 (three frames a call; the flush of stream 1 becomes stream 0's)."""
    return [(det, count, [0] * len(stream_of), [flush[1]]) for det, count, stream_of, flush in calls]


def run_case(max_tracks, n_streams=3, mode='grid', min_hits=1, confirm=2, max_events=None, clock=False, seed=None, n_calls=20, planes=None):
    """The GPU tracker and the numpy tracker in lockstep over a scene; lp_speed_update behind every call against SpeedNp.
    ``max_events``: an int, None for max_tracks, or 'exact' for the largest count of the call."""
    from yolov6.hip import runtime
    from yolov6.utils.speed import SpeedNp
    from yolov6.utils.track import PlateTrackerNp
    seed = max_tracks + 3 * min_hits if seed is None else seed
    S = n_streams
    planes = (P.speed_planes() if S == 3 else P.speed_planes()[:1]) if planes is None else planes
    trk, ref = runtime.PlateTracker(S, max_tracks=max_tracks, device='cuda', **KW), PlateTrackerNp(S, max_tracks=max_tracks, **KW)
    ground = runtime.GroundPlane(S, planes)
    call = SpeedCall(S, max_tracks, ground, min_hits, confirm, trk.ncls)
    spec = SpeedNp(ground, max_tracks, min_hits, confirm)
    calls = Z.zone_calls(seed, max_tracks, n_calls, mode)
    seen, second_wave, capped, rng = {}, 0, 0, np.random.default_rng(seed)
    t_us = np.zeros(S, np.int64)
    for k, (det, count, stream_of, flush) in enumerate(calls if S == 3 else one_stream(calls)):
        trk.update(torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda(), stream_of, flush)
        ref.update(det, count, stream_of, flush)
        t_us += rng.integers(20000, 90000, S)                                    # an irregular clock
        me = max_tracks if max_events is None else max_events
        if max_events == 'exact':
            memo = spec.memo.copy()
            me = int(spec.step(ref, t_us if clock else None)[2].max())
            spec.memo[:] = memo
        spec.max_events = me
        want = spec.step(ref, t_us if clock else None) + (spec.memo,)
        got = call(trk.state, torch.from_numpy(t_us).cuda() if clock else None, me)
        P.assert_same(got, want, 'T %d, S %d, %s, min_hits %d, max_events %s, call %d' % (max_tracks, S, mode, min_hits, me, k))
        P.kinds_seen(want[1], want[2], seen)
        second_wave += int((want[1][:, :, 3] >= 64).sum())
        capped += int((want[2] > me).sum())
    return seen, second_wave, capped, want


# ---- kernel == specification, on every int32 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_tracks', [1, 5, 64, 65, 128])
def test_speed_update_equals_numpy_spec_at_every_slot_count(max_tracks):
    seen, second_wave, _, want = run_case(max_tracks)
    assert max_tracks < 5 or (seen.get(1, 0) > 0 and seen.get(3, 0) > 0), seen
    assert (second_wave > 0) == (max_tracks > 64)
    assert want[3][:2, :, 2].max() > 8                                           # rings that wrapped
    assert not want[3][2].any() and (want[0][2, :, 0] == -1).all()               # the stream without a plane


@pytest.mark.parametrize('min_hits', [1, 3])
def test_one_stream_and_min_hits(min_hits):
    seen, _, _, want = run_case(40, n_streams=1, min_hits=min_hits)
    assert seen.get(1, 0) > 0 and seen.get(3, 0) > 0, seen


@pytest.mark.parametrize('mode', ['float', 'nan'])
def test_arbitrary_fp32_boxes_and_nan_boxes_with_the_clock_given(mode):
    seen, _, _, _ = run_case(64, mode=mode, clock=True, seed=9)
    assert seen.get(1, 0) > 0 and seen.get(3, 0) > 0, seen


@pytest.mark.parametrize('max_events', [0, 1, 'exact', None])
def test_max_events_caps_the_lines_not_the_count(max_events):
    _, _, capped, _ = run_case(20, max_events=max_events, seed=5)
    assert (capped > 0) == (max_events in (0, 1))


def test_a_disabled_stream_with_tracks():
    planes = [None] + P.speed_planes()[:2]                                        # stream 0 is fed and has no plane
    _, _, _, want = run_case(16, planes=planes, seed=3)
    assert (want[0][0, :, 0] == -1).all() and not want[3][0].any() and want[3][1].any()


# ---- hand-built tracker states ------------------------------------------------------------------------------------------------------------
def replay(planes, spec, outs, max_tracks=2, **kw):
    """The feeds of a ``P.hand_run`` through lp_speed_update: every call equals the specification's."""
    from yolov6.hip import runtime
    call = SpeedCall(len(planes), max_tracks, runtime.GroundPlane(len(planes), planes), **kw)
    for k, ((state, clk), want) in enumerate(zip(spec.feeds, outs)):
        got = call(torch.from_numpy(state).cuda(), None if clk is None else torch.from_numpy(clk).cuda(), spec.max_events)
        P.assert_same(got, want, 'call %d' % k)


@pytest.mark.parametrize('case', P.root_family_cases(), ids=lambda c: c[0])
def test_integer_root_family(case):
    name, pl, (a, b), frames, dx, dy = case
    _, spec, outs = P.hand_run([pl], P.root_family_steps(a, b, frames))
    assert outs[1][0][0, 0, 1] >= 0
    replay([pl], spec, outs)


def test_the_run_on_which_a_fused_multiply_add_gives_other_millimetres():
    pts = P.fma_trap_points()
    assert all(P.frac_world(P.FMA_H, x, y) != P.frac_world(P.FMA_H, x, y, fused=True) for x, y in pts)
    _, spec, outs = P.one_track([P.plane(P.FMA_H)], pts)
    replay([P.plane(P.FMA_H)], spec, outs)


def test_validity_edges():
    """w = 0, w < 0, w NaN, u infinite, |X * 1000| at 2^30 and the next fp64 above, NaN and infinite boxes, rint ties: one slot per
    case, two calls, so that every valid one pushes twice."""
    x0 = float(2 ** 30) / 1000.0
    while x0 * 1000.0 > 2.0 ** 30:
        x0 = float(np.nextafter(x0, 0.0))
    while float(np.nextafter(x0, np.inf)) * 1000.0 <= 2.0 ** 30:
        x0 = float(np.nextafter(x0, np.inf))
    x1 = float(np.nextafter(x0, np.inf))
    Hs = [(1, 0, 0, 0, 1, 0, 0, 0, 1), (1, 0, 0, 0, 1, 0, 0, 0.02, -1), (1, 0, 0, 0, 1, 0, 0, 0, -1), (1, 0, 0, 0, 1, 0, 1e308, -1e308, 1),
          (1e308, 1e308, 0, 0, 1, 0, 0, 0, 1), (0, 0, x0, 0, 0, -x0, 0, 0, 1), (0, 0, x1, 0, 0, 0, 0, 0, 1), (0, 0, 0, 0, 0, -x1, 0, 0, 1),
          (1, 0, 0, 0, -1, 0, 0, 0, 16)]
    planes = [P.plane(H) for H in Hs]
    from yolov6.utils.speed import GroundPlaneNp, SpeedNp
    st, spec = P.HandState(len(Hs), 8), SpeedNp(GroundPlaneNp(len(Hs), planes), 8)
    anchors = [(100.0, 50.0), (np.nan, 5.0), (5.0, np.inf), (-np.inf, 5.0), (1.0, 1.0), (3.0, 3.0), (5.0, -3.0), (50.0, 50.0)]
    spec.feeds, outs = [], []
    for k in range(2):
        st.frame[:] = k + 1
        for s in range(len(Hs)):
            for t, (cx, cy) in enumerate(anchors):
                st.put(s, t, 10 + t, k, k + 1, cx + k, cy)
        spec.feeds.append((st.packed(), None))
        outs.append(tuple(a.copy() for a in spec.step(st) + (spec.memo,)))
    n = outs[1][0][:, :, 7] & 255
    assert list(n[0]) == list(n[5]) == [2, 0, 0, 0, 2, 2, 2, 2] and not n[1:3].any() and n[3, 0] == n[4, 0] == 0 and not n[6:8].any() and n[8, 0] == 2
    assert outs[0][0][8, 4, 4:6].tolist() == [62, -62] and outs[0][0][5, 0, 4:6].tolist() == [2 ** 30, -2 ** 30]
    replay(planes, spec, outs, max_tracks=8)


# ---- the edges of the rule, through both trackers --------------------------------------------------------------------------------------
def lockstep(planes, calls, max_tracks=4, clock=False, **enable):
    """``PlateTracker.enable_speed`` and ``PlateTrackerNp.enable_speed`` over ``calls`` = (rows per frame, clock or None, flush):
    equal after every call."""
    from yolov6.hip import runtime
    from yolov6.utils.speed import GroundPlaneNp
    from yolov6.utils.track import PlateTrackerNp
    kw = dict(max_tracks=max_tracks, max_age=0)
    trk, ref = runtime.PlateTracker(len(planes), device='cuda', **kw), PlateTrackerNp(len(planes), **kw)
    trk.enable_speed(runtime.GroundPlane(len(planes), planes), clock=clock, **enable)
    ref.enable_speed(GroundPlaneNp(len(planes), planes), clock=clock, **enable)
    n_ev = 0
    for k, (rows, clk, flush) in enumerate(calls):
        det, count = P.T.frames_of([rows], 4)
        if clk is not None:
            trk.speed_clock.fill_(clk)
            ref.speed_clock[:] = clk
        args = ([0], [1] + [0] * (len(planes) - 1)) if flush else ([0], None)
        trk.update(torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda(), *args)
        ref.update(det, count, *args)
        torch.cuda.synchronize()
        P.assert_same(tuple(t.cpu().numpy() for t in trk.last_speed + (trk.speed_memo(),)), P.outputs_np(ref), 'call %d' % k)
        n_ev += int(ref.last_speed[2].sum())
    return ref, n_ev


def rows_at(centres):
    return [P.T.make_row(Z.box_at(*c)) for c in centres]


def test_ring_wraps_twice_then_the_flush_reports_it():
    calls = [(rows_at([c]), None, False) for c in P.line_of(40, 8, 17)] + [([], None, True)]
    ref, n_ev = lockstep([P.plane()], calls)
    assert n_ev == 1 and ref.last_speed[1][0, 0, 5] == 25000


def test_gap_and_span_edges_with_the_clock():
    gap = 100000
    clocks = [0, gap - 1, gap, 2 * gap - 1, 2 * gap + 5, 3 * gap + 5]
    ref, _ = lockstep([P.plane(min_gap_us=gap)], [(rows_at([c]), clk, False) for c, clk in zip(P.line_of(40, 8, 6), clocks)], clock=True)
    assert ref.speed_memo()[0, 0, 2] == 4
    for dt, want in ((90000, 11111), (89999, -1)):
        ref, _ = lockstep([P.plane(min_span_us=90000)], [(rows_at([c]), clk, False) for c, clk in zip(P.line_of(40, 8, 2), (1000, 1000 + dt))], clock=True)
        assert ref.last_speed[0][0, 0, 1] == want
    ref, n_ev = lockstep([P.plane()], [(rows_at([c]), clk, False) for c, clk in zip(P.line_of(40, 8, 3), (5000, 5000, 4000))] + [([], 4000, True)],
                         clock=True)
    assert n_ev == 1 and ref.last_speed[1][0, 0, 11] == 0


@pytest.mark.parametrize('confirm', [1, 3])
def test_confirm_with_a_dip(confirm):
    pl = P.plane(limit_mm_s=20000)
    _, spec, outs = P.hand_run([pl], P.confirm_steps(), confirm=confirm)
    assert [k for k, o in enumerate(outs) if int(o[2][0])] == [1 if confirm == 1 else 7]
    replay([pl], spec, outs, confirm=confirm)


def test_slot_reuse_and_two_frames_in_one_call():
    calls = [(rows_at([c]), None, False) for c in P.line_of(40, 8, 3)] + [(rows_at([(600, 300)]), None, False)]
    ref, n_ev = lockstep([P.plane()], calls, max_tracks=1)
    assert n_ev == 1 and tuple(ref.last_speed[0][0, 0, :2]) == (1, -1)
    from yolov6.hip import runtime
    from yolov6.utils.speed import GroundPlaneNp
    from yolov6.utils.track import PlateTrackerNp
    trk, ref = runtime.PlateTracker(1, max_tracks=4, max_age=2, device='cuda'), PlateTrackerNp(1, max_tracks=4, max_age=2)
    trk.enable_speed(runtime.GroundPlane(1, [P.plane()]))
    ref.enable_speed(GroundPlaneNp(1, [P.plane()]))
    for frames in ([rows_at([(40, 100)])], [rows_at([(48, 100)]), []]):          # the second call: two frames, matched only the first
        det, count = P.T.frames_of(frames, 4)
        trk.update(torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda(), [0] * len(frames))
        ref.update(det, count, [0] * len(frames))
    P.assert_same(tuple(t.cpu().numpy() for t in trk.last_speed + (trk.speed_memo(),)), P.outputs_np(ref), 'two frames')
    assert ref.speed_memo()[0, 0, 20] == P.PERIOD and ref.last_speed[0][0, 0, 1] == 25000


# ---- through the tracker ---------------------------------------------------------------------------------------------------------------
def _same(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        w = w.cpu().numpy() if torch.is_tensor(w) else w
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g.view(np.uint8), np.ascontiguousarray(w).view(np.uint8)), (what, k)


def _speed_out(trk):
    return tuple(t.cpu().numpy() for t in trk.last_speed + (trk.speed_memo(),))


def test_tracker_enable_speed_equals_numpy_and_changes_nothing_else():
    """Three device trackers with zones, a live watchlist and sightings: ``plain`` without speed, ``trk`` with it, ``alone`` with
    speed only; and the numpy tracker.  Every return and add-on result of ``trk`` is ``plain``'s, its speed is ``alone``'s and the
    specification's."""
    from yolov6.hip import runtime
    from yolov6.utils import watch
    from yolov6.utils.speed import GroundPlaneNp
    from yolov6.utils.track import PlateTrackerNp
    lines, zones = Z.zone_geometry(4, 6, 3)
    calls = Z.zone_calls(4, 16, 12)
    kw = dict(max_tracks=16, **KW)
    plain, trk, alone = (runtime.PlateTracker(3, device='cuda', **kw) for _ in range(3))
    ref = PlateTrackerNp(3, **kw)
    entries = np.random.default_rng(2).integers(0, 24, (40, 8)).astype(np.int32)
    for t in (plain, trk):
        t.enable_best_shot((16, 48), max_crops=8)
        t.enable_zones(runtime.ZoneMap(3, lines, zones), min_hits=2)
        t.enable_live_watch(runtime.Watchlist(entries, None, 'cuda'), min_hits=2, max_mismatch=8)
        t.enable_sightings(runtime.SightLog(64, 3, device='cuda'), min_hits=1, max_mismatch=8)
    alone.enable_best_shot((16, 48), max_crops=8)
    assert trk.speed_memo() is None and trk.last_speed is None
    for t in (trk, alone):
        t.enable_speed(runtime.GroundPlane(3, P.speed_planes()), min_hits=2, confirm=2)
    ref.enable_speed(GroundPlaneNp(3, P.speed_planes()), min_hits=2, confirm=2)
    assert trk.last_speed is None and trk._speed['ev'].shape == (3, 16, 12) and trk.speed_memo().shape == (3, 16, 48)
    frame = torch.zeros(Z.EXTENT[1] + 64, Z.EXTENT[0] + 128, 3, dtype=torch.uint8, device='cuda')
    n_ev = 0
    for k, (det, count, stream_of, flush) in enumerate(calls):
        d, c = torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda()
        want = ref.update(det, count, stream_of, flush, 5)
        if k % 2:
            a, b = plain.update(d, c, stream_of, flush, 5), trk.update(d, c, stream_of, flush, 5)
            alone.update(d, c, stream_of, flush, 5)
        else:
            frames = [frame] * len(det)
            a, b = plain.update_with_shots(frames, d, c, stream_of, flush, 5), trk.update_with_shots(frames, d, c, stream_of, flush, 5)
            alone.update_with_shots(frames, d, c, stream_of, flush, 5)
            assert len(a) == len(b) == 9
        torch.cuda.synchronize()
        _same(b, a, 'call %d: speed on against off' % k)
        _same(b[:5], want, 'call %d' % k)
        assert torch.equal(plain.state, trk.state)
        _same(trk.last_zone + (trk.zone_memo, trk.last_live, trk.last_sight), plain.last_zone + (plain.zone_memo, plain.last_live, plain.last_sight),
              'call %d: the other add-ons' % k)
        P.assert_same(_speed_out(trk), P.outputs_np(ref), 'call %d' % k)
        P.assert_same(_speed_out(alone), P.outputs_np(ref), 'call %d, speed alone' % k)
        n_ev += int(ref.last_speed[2].sum())
    assert n_ev > 3 and plain.last_speed is None
    assert trk.speed_memo()[0].any() and trk.speed_memo()[1].any()
    trk.reset([1])
    ref.reset([1])
    P.assert_same((trk.speed_memo().cpu().numpy(),), (ref.speed_memo(),), 'reset')
    assert not trk.speed_memo()[1].any() and trk.speed_memo()[0].any()
    trk.flush_all(max_ended=5)
    ref.flush_all(max_ended=5)
    P.assert_same(_speed_out(trk), P.outputs_np(ref), 'flush_all')
    assert not trk.speed_memo().any() and ref.last_speed[2][0] > 0
    trk.flush_all_with_shots(max_ended=5)
    ref.flush_all(max_ended=5)
    P.assert_same(_speed_out(trk), P.outputs_np(ref), 'flush_all_with_shots')
    trk.enable_speed(None)
    trk.flush_all(max_ended=5)
    assert trk.last_speed is None and trk.speed_memo() is None
    with pytest.raises(ValueError):
        trk.enable_speed(GroundPlaneNp(3, P.speed_planes()))                    # a host map is not a device map
    with pytest.raises(ValueError):
        trk.enable_speed(runtime.GroundPlane(2, P.speed_planes()[:2]))
    with pytest.raises(ValueError, match='min_hits'):
        trk.enable_speed(runtime.GroundPlane(3, P.speed_planes()), min_hits=0)
    with pytest.raises(ValueError, match='confirm'):
        trk.enable_speed(runtime.GroundPlane(3, P.speed_planes()), confirm=0)
    with pytest.raises(ValueError):
        runtime.GroundPlane(1, [dict(H=(1, 0, 0, 0, 1, 0, 0, 0, float('nan')))])


def test_graph_capture_of_update_with_speed_and_a_clock_changed_between_replays():
    """Tracker and speed are captured in one graph on a single stream (one chain, no parallel branches); ``speed_clock`` is read in
    place: the replays, each with another clock, equal the specification."""
    from yolov6.hip import runtime
    from yolov6.utils.speed import GroundPlaneNp
    from yolov6.utils.track import PlateTrackerNp
    calls = Z.zone_calls(6, 16, 10)
    kw = dict(max_tracks=16, **KW)
    trk, ref = runtime.PlateTracker(3, device='cuda', **kw), PlateTrackerNp(3, **kw)
    trk.enable_speed(runtime.GroundPlane(3, P.speed_planes()), clock=True)
    ref.enable_speed(GroundPlaneNp(3, P.speed_planes()), clock=True)
    det, count = torch.from_numpy(calls[0][0]).cuda(), torch.from_numpy(calls[0][1]).cuda()
    stream_of = calls[0][2]
    clocks = np.cumsum(np.random.default_rng(6).integers(30000, 120000, (10, 3)), 0).astype(np.int64)

    def feed(k):
        det.copy_(torch.from_numpy(calls[k][0]))
        count.copy_(torch.from_numpy(calls[k][1]))
        trk.speed_clock.copy_(torch.from_numpy(clocks[k]))
        ref.speed_clock[:] = clocks[k]
    for k in range(3):                                                          # eager, so that every buffer exists
        feed(k)
        trk.update(det, count, stream_of)
        ref.update(calls[k][0], calls[k][1], stream_of)
    torch.cuda.synchronize()
    P.assert_same(_speed_out(trk), P.outputs_np(ref), 'eager')
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        trk.update(det, count, stream_of)
    estimates = 0
    for k in range(3, 10):
        feed(k)
        for t in trk.last_speed:
            t.fill_(POISON)
        g.replay()
        torch.cuda.synchronize()
        ref.update(calls[k][0], calls[k][1], stream_of)
        P.assert_same(_speed_out(trk), P.outputs_np(ref), 'replay %d' % k)
        estimates += int((ref.last_speed[0][:, :, 1] > 0).sum())
    assert estimates > 10


# ---- the argument checks ---------------------------------------------------------------------------------------------------------------
def test_argument_checks_launch_nothing():
    from yolov6.hip import runtime
    trk = runtime.PlateTracker(2, max_tracks=8, device='cuda', **KW)
    call = SpeedCall(2, 8, runtime.GroundPlane(2, P.speed_planes()[:2]), ncls=trk.ncls)
    clock = torch.zeros(4, dtype=torch.int64, device='cuda')
    call(trk.state, clock[:2], 16)                                              # the good call
    lib = call.lib
    assert lib.lp_speed_state_bytes(0, 8) == 0 and lib.lp_speed_state_bytes(2, 0) == 0 and lib.lp_speed_state_bytes(2, 129) == 0
    assert lib.lp_speed_state_bytes(1 << 20, 128) == 0                          # a state of 2^31 words or more
    ev, good = call.args(trk.state, clock[:2], 16)
    g = dict(zip(NAMES, good))
    ptr = lambda p, off=0: ctypes.c_void_p(p.value + off)                       # noqa: E731
    bad_ncls, wide_ncls = (ctypes.c_int * 8)(31, 24, 37, 37, 0, 37, 37, 37), (ctypes.c_int * 8)(*([65] * 8))
    cases = dict(
        no_streams=dict(S=0), no_tracks=dict(T=0), too_many_tracks=dict(T=129), negative_events=dict(max_events=-1),
        events_2_31=dict(max_events=(1 << 31) // 24 + 1), streams_2_31=dict(S=1 << 22), min_hits_0=dict(min_hits=0), confirm_0=dict(confirm=0),
        confirm_wide=dict(confirm=65536), ncls_null=dict(ncls=None), ncls_zero=dict(ncls=bad_ncls), ncls_wide=dict(ncls=wide_ncls),
        state_null=dict(state=None), map_null=dict(map=None), memo_null=dict(memo=None), rows_null=dict(rows=None), ev_null=dict(ev=None),
        count_null=dict(count=None),
        state_align=dict(state=ptr(g['state'], 4)), map_align=dict(map=ptr(g['map'], 8)), memo_align=dict(memo=ptr(g['memo'], 4)),
        rows_align=dict(rows=ptr(g['rows'], 8)), ev_align=dict(ev=ptr(g['ev'], 4)), count_align=dict(count=ptr(g['count'], 4)),
        clock_align=dict(clock=ptr(g['clock'], 4)),
        memo_on_state=dict(memo=g['state']), ev_on_map=dict(ev=g['map']), ev_on_memo=dict(ev=ptr(g['memo'], 16)), count_on_ev=dict(count=g['ev']),
        rows_on_memo=dict(rows=ptr(g['memo'], 2 * 8 * 48 * 4 - 16)), count_on_clock=dict(count=g['clock']), rows_on_count=dict(rows=g['count']))
    state = trk.state.clone()
    bufs = (call.memo, call.rows, ev, call.count)
    for name, over in cases.items():
        for b in bufs:
            b.buf.fill_(POISON)
        clock.fill_(POISON)
        _, args = call.args(trk.state, clock[:2], 16, **over)
        rc = lib.lp_speed_update(*args)
        torch.cuda.synchronize()
        assert rc == LP_ERR_ARG and b'lp_speed_update' in lib.lp_last_error(), (name, rc)
        assert all(bool((b.buf == POISON).all()) for b in bufs) and bool((clock == POISON).all()), name
    assert torch.equal(state, trk.state)
    for b in bufs:                                                              # max_events 0 takes a null speed_ev, and the clock may be null
        b.buf.fill_(0)
    _, args = call.args(trk.state, None, 0, ev=None)
    assert lib.lp_speed_update(*args) == 0
    torch.cuda.synchronize()
    assert not ev.buf.any()


# ---- Inferer(track=True, speed=FILE) ---------------------------------------------------------------------------------------------------
def test_infer_speed_matches_the_cpu_computation(tmp_path, monkeypatch):
    """speeds.txt and speeding.txt of the GPU run against PlateTrackerNp by hand on the same run's untracked detections."""
    P.check_infer_speed(tmp_path, *Z.infer_zones_case(tmp_path, monkeypatch, '0', half=True))
