"""Lines and zones on live plate tracks on the GPU: lp_zone_update against its numpy specification (yolov6/utils/zones.py) on every
int32 of zone_ev, zone_count, zone_occ, zone_totals and of the memo, call after call -- slot counts at the wave boundary of the
prefix sum and the full workgroup, geometry sizes from none to 16 lines and 8 zones, max_events at its edges, boxes on a grid
(anchors exactly on lines and vertices), arbitrary fp32 boxes (where the rounding of every fp64 operation matters: a fused
multiply-subtract fails there), NaN and infinite boxes; guard words around every buffer and a byte-identical tracker state; through
PlateTracker.enable_zones over update, update_with_shots and flush_all; the argument checks; and one graph capture."""
import ctypes

import numpy as np
import pytest
import torch

import test_zones_cpu as Z

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD, GUARD_WORD, POISON = 64, 0x5EADBEE, -77          # 64 int32 = 256 bytes on either side: the alignment stays
KW = dict(match_thres=0.3, new_thres=0.2, expand=0.25, max_age=2)
LP_ERR_ARG = -1


class Guarded:
    """An int32 device tensor of ``shape`` with guard words on both sides."""

    def __init__(self, shape, fill):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), GUARD_WORD, dtype=torch.int32, device='cuda')
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        self.t.fill_(fill)

    def intact(self):
        return bool((self.buf[:GUARD] == GUARD_WORD).all()) and bool((self.buf[self.buf.numel() - GUARD:] == GUARD_WORD).all())


class ZoneCall:
    """lp_zone_update called directly on a tracker's state, with guarded buffers of its own."""

    def __init__(self, trk, zone_map, min_hits, max_events):
        from yolov6.hip import abi
        self.lib, self.trk, self.zone_map, self.min_hits = abi.load(), trk, zone_map, min_hits
        S, T = trk.n_streams, trk.max_tracks
        assert self.lib.lp_zone_state_bytes(S, T) == S * (T + 2) * 16 * 4
        self.ncls = (ctypes.c_int * 8)(*trk.ncls)
        self.memo = Guarded((S, T + 2, 16), 0)
        self.count, self.occ, self.totals = Guarded((S,), POISON), Guarded((S, 8), POISON), Guarded((S, 2, 16), POISON)
        self.ev = {}
        self.max_events = max_events

    def args(self, n_events, **over):
        """(the guarded zone_ev of ``n_events`` lines, the arguments of the call with ``over`` replacing some)."""
        from yolov6.hip.runtime._base import _dptr, _stream_ptr
        trk, max_events = self.trk, n_events
        ev = self.ev.get(max_events)
        if ev is None:
            ev = self.ev[max_events] = Guarded((trk.n_streams, max_events, 12), POISON)
        a = dict(state=_dptr(trk.state), S=trk.n_streams, T=trk.max_tracks, ncls=self.ncls, map=_dptr(self.zone_map.packed), min_hits=self.min_hits,
                 memo=_dptr(self.memo.t), ev=ctypes.c_void_p(ev.buf.data_ptr() + 4 * GUARD), count=_dptr(self.count.t), max_events=max_events,
                 occ=_dptr(self.occ.t), totals=_dptr(self.totals.t), stream=_stream_ptr(trk.device))
        a.update(over)
        return ev, tuple(a.values())

    def __call__(self, max_events=None):
        max_events = self.max_events if max_events is None else max_events
        for g in (self.count, self.occ, self.totals):
            g.t.fill_(POISON)
        ev, args = self.args(max_events)
        ev.t.fill_(POISON)
        before = self.trk.state.clone()
        assert self.lib.lp_zone_update(*args) == 0, self.lib.lp_last_error()
        torch.cuda.synchronize()
        assert torch.equal(before, self.trk.state), 'the tracker state was written'
        for name, g in (('memo', self.memo), ('zone_ev', ev), ('zone_count', self.count), ('zone_occ', self.occ), ('zone_totals', self.totals)):
            assert g.intact(), 'guard words of %s' % name
        return tuple(g.t.cpu().numpy() for g in (ev, self.count, self.occ, self.totals, self.memo))


def run_case(max_tracks, L, Z_, mode='grid', min_hits=1, max_events=None, seed=None, n_calls=12):
    """The GPU tracker and the numpy tracker in lockstep over a scene; lp_zone_update behind every call against ZoneEventsNp.
    ``max_events``: an int, None for 2 * max_tracks, or 'exact' for the largest count of the call."""
    from yolov6.hip import runtime
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.zones import ZoneEventsNp
    seed = max_tracks + 7 * L + Z_ if seed is None else seed
    lines, zones = Z.zone_geometry(seed, L, Z_)
    trk, ref = runtime.PlateTracker(3, max_tracks=max_tracks, device='cuda', **KW), PlateTrackerNp(3, max_tracks=max_tracks, **KW)
    zmap = runtime.ZoneMap(3, lines, zones)
    spec, call = ZoneEventsNp(ref, zmap, min_hits), ZoneCall(trk, zmap, min_hits, 2 * max_tracks)
    seen, second_wave, capped = {}, 0, 0
    for k, (det, count, stream_of, flush) in enumerate(Z.zone_calls(seed, max_tracks, n_calls, mode)):
        trk.update(torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda(), stream_of, flush)
        ref.update(det, count, stream_of, flush)
        me = 2 * max_tracks if max_events is None else max_events
        if max_events == 'exact':
            memo = spec.memo.copy()
            me = int(spec.step(1)[1].max())
            spec.memo[:] = memo
        want = spec.step(me) + (spec.memo,)
        Z.assert_same(call(me), want, 'T %d, L %d, Z %d, %s, max_events %s, call %d' % (max_tracks, L, Z_, mode, me, k))
        Z.kinds_seen(want[0], want[1], seen)
        second_wave += int((want[0][:, :, 3] >= 64).sum())
        capped += int((want[1] > me).sum())
        assert not want[4][2].any() and want[1][2] == 0                          # the stream that is never fed
    return seen, second_wave, capped


# ---- kernel == specification, on every int32 -------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_tracks', [1, 5, 64, 65, 128])
def test_zone_update_equals_numpy_spec_at_every_slot_count(max_tracks):
    seen, second_wave, _ = run_case(max_tracks, 16, 8)
    assert all(seen.get(k, 0) > 0 for k in ((1, 2, 3, 4, 5) if max_tracks >= 5 else (2,))), seen
    assert (second_wave > 0) == (max_tracks > 64)


@pytest.mark.parametrize('L,Z_', [(0, 0), (1, 0), (0, 1), (16, 8)])
@pytest.mark.parametrize('min_hits', [1, 3])
def test_zone_update_equals_numpy_spec_at_every_geometry_size(L, Z_, min_hits):
    seen, _, _ = run_case(40, L, Z_, min_hits=min_hits, seed=11 + L + Z_)
    assert (seen.get(1, 0) > 0) == (L == 16) or L == 1
    assert (seen.get(2, 0) > 0) == (Z_ > 0) and (L + Z_ > 0 or not seen)


@pytest.mark.parametrize('max_events', [0, 1, 'exact', None])
def test_max_events_caps_the_lines_not_the_count(max_events):
    _, _, capped = run_case(20, 16, 8, max_events=max_events, seed=5)
    assert (capped > 0) == (max_events in (0, 1))


def diagonal_scene(n_calls=12, n=24):
    """A line and a zone edge along the diagonal from (a, a) to (b, b), a and b with full fp32 mantissas at different exponents, and
    ``n`` square boxes whose anchors (q, q) step onto the diagonal and off it again.  For a point on the diagonal both products of
    cross(A, B, P) are the same fp64 product, rounded: the difference is exactly 0 op by op, while a fused multiply-subtract leaves the
    rounding error of the product there, positive for about half of the points -- and `d <= 0` or `t < 0` answers differently."""
    from fractions import Fraction
    rng = np.random.default_rng(17)
    a, b = f32(0.1), f32(1700.3)
    lines = [[(a, a, b, b), (b, b, a, a)], [], []]
    zones = [[(np.array([(a, a), (b, b), (a, b)], f32), 2), (np.array([(b, b), (a, a), (b, a)], f32), 0)], [], []]
    p = (60 * np.arange(n) + 30 + rng.uniform(0, 9, n)).astype(f32)
    calls, flips = [], 0
    for c in range(n_calls):
        rows = []
        for k in range(n):
            phase = (c + k) % 4                                                 # off on one side, on, off on the other side, on
            dx = f32((9.25, 0, -9.25, 0)[phase])
            x1, x2 = f32(p[k] - 20), f32(p[k] + 20)
            rows.append(Z.T.make_row((f32(x1 + dx), x1, f32(x2 + dx), x2), rng.integers(0, 24, 8), 0.5))
            if phase % 2:
                q = Fraction(float((x1 + x2) * f32(0.5)))
                u, w = float(b) - float(a), float(q - Fraction(float(a)))       # both exact in fp64
                flips += Fraction(u) * Fraction(w) > Fraction(u * w)            # the residue a fused operation would see as d > 0
        det, count = Z.T.frames_of([rows], n + 2)
        calls.append((det, count, [0], None))
    return lines, zones, calls, flips


def test_arbitrary_fp32_boxes_every_fp64_operation_rounded_on_its_own():
    """Two runs on fp32 values with full mantissas, where the fp64 products are not exact: the random scene moved off its grid, and
    ``diagonal_scene``, which a kernel that fuses a multiply into the subtract fails."""
    from yolov6.hip import runtime
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.zones import ZoneEventsNp
    rng = np.random.default_rng(3)
    lines, zones = Z.zone_geometry(2, 16, 8, step=1.0)
    lines = [[tuple(f32(v + rng.uniform(-0.5, 0.5)) for v in ln) for ln in ls] for ls in lines]
    zones = [[((v + rng.uniform(-0.5, 0.5, v.shape)).astype(f32), d) for v, d in zs] for zs in zones]
    d_lines, d_zones, d_calls, flips = diagonal_scene()
    assert flips >= 20                                                          # points where the fused form gives the other answer
    for what, lines, zones, calls, T_ in (('random', lines, zones, Z.zone_calls(21, 64, 12, 'float'), 64), ('diagonal', d_lines, d_zones, d_calls, 32)):
        trk, ref = runtime.PlateTracker(3, max_tracks=T_, device='cuda', **KW), PlateTrackerNp(3, max_tracks=T_, **KW)
        zmap = runtime.ZoneMap(3, lines, zones)
        spec, call = ZoneEventsNp(ref, zmap, 1), ZoneCall(trk, zmap, 1, 128)
        seen = {}
        for k, (det, count, stream_of, flush) in enumerate(calls):
            trk.update(torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda(), stream_of, flush)
            ref.update(det, count, stream_of, flush)
            want = spec.step(128) + (spec.memo,)
            Z.assert_same(call(128), want, '%s, call %d' % (what, k))
            Z.kinds_seen(want[0], want[1], seen)
        assert all(seen.get(k, 0) > 0 for k in ((1, 2, 3, 5) if what == 'random' else (1, 2, 3))), (what, seen)


def test_nan_and_infinite_boxes():
    seen, _, _ = run_case(40, 16, 8, mode='nan', seed=9)
    assert seen.get(1, 0) > 0 and seen.get(2, 0) > 0


# ---- through the tracker ---------------------------------------------------------------------------------------------------------------
def _same(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        w = w.cpu().numpy() if torch.is_tensor(w) else w
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g.view(np.uint8), np.ascontiguousarray(w).view(np.uint8)), (what, k)


def test_tracker_enable_zones_equals_numpy_and_changes_nothing_else():
    from yolov6.hip import runtime
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.zones import ZoneMapNp
    lines, zones = Z.zone_geometry(4, 6, 3)
    calls = Z.zone_calls(4, 16, 12)
    kw = dict(max_tracks=16, **KW)
    plain, trk, ref = runtime.PlateTracker(3, device='cuda', **kw), runtime.PlateTracker(3, device='cuda', **kw), PlateTrackerNp(3, **kw)
    for t in (plain, trk):
        t.enable_best_shot((16, 48), max_crops=8)
    assert trk.zone_memo is None and trk.last_zone is None
    trk.enable_zones(runtime.ZoneMap(3, lines, zones), min_hits=2)
    ref.enable_zones(ZoneMapNp(3, lines, zones), min_hits=2)
    assert trk.last_zone is None and trk._zones['ev'].shape == (3, 32, 12)
    frame = torch.zeros(Z.EXTENT[1] + 64, Z.EXTENT[0] + 128, 3, dtype=torch.uint8, device='cuda')
    n_ev = 0
    for k, (det, count, stream_of, flush) in enumerate(calls):
        d, c = torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda()
        want = ref.update(det, count, stream_of, flush, 5)
        if k % 2:
            a, b = plain.update(d, c, stream_of, flush, 5), trk.update(d, c, stream_of, flush, 5)
        else:
            frames = [frame] * len(det)
            a, b = plain.update_with_shots(frames, d, c, stream_of, flush, 5), trk.update_with_shots(frames, d, c, stream_of, flush, 5)
            assert len(a) == len(b) == 9
        torch.cuda.synchronize()
        _same(b, a, 'call %d: zones on against off' % k)
        _same(b[:5], want, 'call %d' % k)
        assert torch.equal(plain.state, trk.state)
        Z.assert_same(tuple(t.cpu().numpy() for t in trk.last_zone + (trk.zone_memo,)), Z.outputs_np(ref), 'call %d' % k)
        n_ev += int(ref.last_zone[1].sum())
    assert n_ev > 10 and plain.last_zone is None
    assert trk.zone_memo[0].any() and trk.zone_memo[1].any()
    trk.reset([1])
    ref.reset([1])
    Z.assert_same((trk.zone_memo.cpu().numpy(),), (ref.zone_memo,), 'reset')
    assert not trk.zone_memo[1].any() and trk.zone_memo[0].any()
    trk.flush_all(max_ended=5)
    ref.flush_all(max_ended=5)
    Z.assert_same(tuple(t.cpu().numpy() for t in trk.last_zone + (trk.zone_memo,)), Z.outputs_np(ref), 'flush_all')
    assert not trk.zone_memo[:, :16].any() and not ref.last_zone[2].any()
    trk.flush_all_with_shots(max_ended=5)
    ref.flush_all(max_ended=5)
    Z.assert_same(tuple(t.cpu().numpy() for t in trk.last_zone + (trk.zone_memo,)), Z.outputs_np(ref), 'flush_all_with_shots')
    trk.enable_zones(None)
    trk.flush_all(max_ended=5)
    assert trk.last_zone is None and trk.zone_memo is None
    with pytest.raises(ValueError):
        trk.enable_zones(ZoneMapNp(3, lines, zones))                             # a host map is not a device map
    with pytest.raises(ValueError):
        trk.enable_zones(runtime.ZoneMap(2, lines[:2], zones[:2]))
    with pytest.raises(ValueError, match='min_hits'):
        trk.enable_zones(runtime.ZoneMap(3, lines, zones), min_hits=0)
    with pytest.raises(ValueError):
        runtime.ZoneMap(1, [[(0, 0, float('nan'), 1)]])


def test_graph_capture_of_update_with_zones():
    """Tracker and zones are captured in one graph on a single stream (one chain, no parallel branches); the replays equal the
    specification."""
    from yolov6.hip import runtime
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.zones import ZoneMapNp
    lines, zones = Z.zone_geometry(6, 8, 4)
    calls = Z.zone_calls(6, 16, 8)
    kw = dict(max_tracks=16, **KW)
    trk, ref = runtime.PlateTracker(3, device='cuda', **kw), PlateTrackerNp(3, **kw)
    trk.enable_zones(runtime.ZoneMap(3, lines, zones))
    ref.enable_zones(ZoneMapNp(3, lines, zones))
    det, count = torch.from_numpy(calls[0][0]).cuda(), torch.from_numpy(calls[0][1]).cuda()
    stream_of = calls[0][2]
    for k in range(3):                                                          # eager, so that every buffer exists
        det.copy_(torch.from_numpy(calls[k][0]))
        count.copy_(torch.from_numpy(calls[k][1]))
        trk.update(det, count, stream_of)
        ref.update(calls[k][0], calls[k][1], stream_of)
    torch.cuda.synchronize()
    Z.assert_same(tuple(t.cpu().numpy() for t in trk.last_zone + (trk.zone_memo,)), Z.outputs_np(ref), 'eager')
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        trk.update(det, count, stream_of)
    n_ev = 0
    for k in range(3, 8):
        det.copy_(torch.from_numpy(calls[k][0]))
        count.copy_(torch.from_numpy(calls[k][1]))
        for t in trk.last_zone:
            t.fill_(POISON)
        g.replay()
        torch.cuda.synchronize()
        ref.update(calls[k][0], calls[k][1], stream_of)
        Z.assert_same(tuple(t.cpu().numpy() for t in trk.last_zone + (trk.zone_memo,)), Z.outputs_np(ref), 'replay %d' % k)
        n_ev += int(ref.last_zone[1].sum())
    assert n_ev > 0


# ---- the argument checks -----------------------------------------------------------------------------------------------------------
def test_argument_checks_launch_nothing():
    from yolov6.hip import runtime
    trk = runtime.PlateTracker(2, max_tracks=8, device='cuda', **KW)
    lines, zones = Z.zone_geometry(1, 2, 2, n_streams=2)
    call = ZoneCall(trk, runtime.ZoneMap(2, lines, zones), 1, 16)
    call()                                                                      # the good call
    lib = call.lib
    assert lib.lp_zone_state_bytes(0, 8) == 0 and lib.lp_zone_state_bytes(2, 0) == 0 and lib.lp_zone_state_bytes(2, 129) == 0
    assert lib.lp_zone_state_bytes(1 << 20, 128) == 0                           # a state of 2^31 words or more
    ev, good = call.args(16)
    names = ('state', 'S', 'T', 'ncls', 'map', 'min_hits', 'memo', 'ev', 'count', 'max_events', 'occ', 'totals', 'stream')
    g = dict(zip(names, good))
    ptr = lambda p, off=0: ctypes.c_void_p(p.value + off)                       # noqa: E731
    bad_ncls, wide_ncls = (ctypes.c_int * 8)(31, 24, 37, 37, 0, 37, 37, 37), (ctypes.c_int * 8)(*([65] * 8))
    cases = dict(
        no_streams=dict(S=0), no_tracks=dict(T=0), too_many_tracks=dict(T=129), negative_events=dict(max_events=-1),
        events_2_31=dict(max_events=(1 << 31) // 24 + 1), streams_2_31=dict(S=1 << 22), min_hits_0=dict(min_hits=0),
        ncls_null=dict(ncls=None), ncls_zero=dict(ncls=bad_ncls), ncls_wide=dict(ncls=wide_ncls),
        state_null=dict(state=None), map_null=dict(map=None), memo_null=dict(memo=None), ev_null=dict(ev=None), count_null=dict(count=None),
        occ_null=dict(occ=None), totals_null=dict(totals=None),
        state_align=dict(state=ptr(g['state'], 4)), map_align=dict(map=ptr(g['map'], 8)), memo_align=dict(memo=ptr(g['memo'], 4)),
        ev_align=dict(ev=ptr(g['ev'], 4)), count_align=dict(count=ptr(g['count'], 4)), occ_align=dict(occ=ptr(g['occ'], 8)),
        totals_align=dict(totals=ptr(g['totals'], 12)),
        memo_on_state=dict(memo=g['state']), ev_on_map=dict(ev=g['map']), ev_on_memo=dict(ev=ptr(g['memo'], 16)), count_on_ev=dict(count=g['ev']),
        occ_on_totals=dict(occ=ptr(g['totals'], 64)), totals_on_memo=dict(totals=ptr(g['memo'], 2 * 10 * 16 * 4 - 16)), occ_on_count=dict(occ=g['count']))
    state = trk.state.clone()
    for name, over in cases.items():
        bufs = (call.memo, ev, call.count, call.occ, call.totals)
        for b in bufs:
            b.buf.fill_(POISON)
        _, args = call.args(16, **over)
        rc = lib.lp_zone_update(*args)
        torch.cuda.synchronize()
        assert rc == LP_ERR_ARG and b'lp_zone_update' in lib.lp_last_error(), (name, rc)
        assert all(bool((b.buf == POISON).all()) for b in bufs), name
    assert torch.equal(state, trk.state)
    for b in (call.memo, ev, call.count, call.occ, call.totals):                # max_events 0 takes a null zone_ev
        b.buf.fill_(0)
    _, args = call.args(0, ev=None)
    assert lib.lp_zone_update(*args) == 0
    torch.cuda.synchronize()
    assert not ev.buf.any()


# ---- Inferer(track=True, zones=FILE) --------------------------------------------------------------------------------------------------
def test_infer_zones_matches_the_cpu_computation(tmp_path, monkeypatch):
    """crossings.txt and zones.txt of the GPU run against PlateTrackerNp by hand on the same run's untracked detections."""
    Z.check_infer_zones(tmp_path, *Z.infer_zones_case(tmp_path, monkeypatch, '0', half=True))
