"""The log of sightings on the GPU: lp_sight_update through the C ABI against its numpy specification (yolov6/utils/sight.py) on
every int32 of sight_i and of the log after every call of a sequence -- capacities around the scan's workgroup size, read counts
around its query block, the ring wrapping inside a call, more reads than slots, planted sightings in the first and the last
workgroup, a non-default confusion table, a ``pair`` mask, the four limits -- with poisoned outputs, a workspace of garbage and guard
bytes around everything written; argument errors; the steady state (no allocation, no host read: captured in a graph behind the
tracker); PlateTracker.enable_sightings against PlateTrackerNp.enable_sightings; and Inferer(track=True, sightings=...) against the
rule on the same detections."""
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
import test_sight_cpu as SC

pytestmark = pytest.mark.gpu
f32 = np.float32
POISON, GUARD_WORD, GUARD = -77, 0x5EED5EED, 64              # GUARD int32 words on either side of a written buffer
CFG = lambda name: os.path.join(REPO, 'configs', name + '.py')   # noqa: E731
S = 5


def _consts():
    from yolov6.hip import abi
    return abi.LP_SIGHT_BLOCK_ENTRIES, abi.LP_SIGHT_QUERY_BLOCK


E, QB = _consts()
CAPACITIES = [1, 5, E - 1, E, E + 1, 2 * E + 3]
READ_COUNTS = [0, 1, 5, QB - 1, QB, QB + 1, 2 * QB + 1]        # 5: a block of five to eight reads is an instance of its own
LIMITS = [(0, 32768), (1, 32768), (8, 32768), (2, 2500)]       # max_mismatch 0 / 1 / 8 and a tight max_cost


class Guarded:
    """An int32 device buffer of ``words`` words between two guards; ``t`` is the 16-byte aligned inside."""

    def __init__(self, words, fill):
        self.words = int(words)
        self.all = torch.full((self.words + 2 * GUARD,), GUARD_WORD, dtype=torch.int32, device='cuda')
        self.t = self.all[GUARD:GUARD + self.words]
        self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        g = torch.cat([self.all[:GUARD], self.all[GUARD + self.words:]])
        return bool((g == GUARD_WORD).all())


class GpuLog:
    """One log driven through the C ABI: the state lives between guards; every call gets a poisoned sight_i and a workspace of
    garbage, both between guards of their own."""

    def __init__(self, state, confuse, pair):
        self.cap = len(state) - 1
        self.state = Guarded((self.cap + 1) * 8, 0)
        self.set_state(state)
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
        self.confuse, self.pair = dev(confuse), dev(pair)
        self.now = torch.zeros(1, dtype=torch.int32, device='cuda')

    def set_state(self, state):
        self.state.t.copy_(torch.from_numpy(np.ascontiguousarray(state).reshape(-1)))

    def get_state(self):
        return self.state.t.cpu().numpy().reshape(self.cap + 1, 8)

    def update(self, ended_i, ended_f, ended_count, now, window, min_hits, mm, mc):
        from yolov6.hip import abi
        lib = abi.load()
        ptr = lambda t: None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())   # noqa: E731
        d_i, d_f = torch.from_numpy(ended_i).cuda(), torch.from_numpy(ended_f).cuda()
        d_n = torch.from_numpy(np.asarray(ended_count, np.int32)).cuda()
        n_streams, M = ended_i.shape[:2]
        need = lib.lp_sight_workspace_bytes(n_streams, M)
        sight, ws = Guarded(n_streams * M * 8, POISON), Guarded(need // 4, 0x5A5A5A5A)
        self.now.fill_(now)
        abi.check(lib.lp_sight_update(ptr(self.state.t), self.cap, ptr(self.confuse), ptr(self.pair), ptr(d_i), ptr(d_f), ptr(d_n), n_streams, M,
                                      ptr(self.now), window, min_hits, mm, mc, ptr(sight.t), ptr(ws.t), need,
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'lp_sight_update')
        torch.cuda.synchronize()
        assert self.state.intact() and sight.intact() and ws.intact(), 'a guard word changed'
        return sight.t.cpu().numpy().reshape(n_streams, M, 8)


def reads_of(rng, V, n_ids=3):
    """The ended records of a call with exactly V reads at min_hits = 2: V + 2 lines inside their streams' counts -- a count above
    max_ended, a zero and a negative one among them --, two of them with one hit only."""
    W = V + 2
    M = (W + 1) // 2
    counts = [M + 3, 0, -4, W - M, 0]
    ended_i, ended_f, ended_count = C.random_reads(rng, counts, M, n_ids=n_ids, garbage=0.05)
    ended_i[:, :, 3] = rng.integers(2, 6, (S, M))
    lines = [(s, j) for s, c in enumerate(counts) for j in range(min(max(c, 0), M))]
    assert len(lines) == W
    for s, j in (lines[0], lines[-1]):
        ended_i[s, j, 3] = 1
    return ended_i, ended_f, ended_count


def prefilled_state(rng, cap, total, now, n_ids=3):
    """A consistent log after ``total`` appends: append t in slot t % cap with seq t, random reads of few ids, stamps that do not
    run backwards and end at ``now``."""
    from yolov6.utils.sight import new_state
    state = new_state(cap)
    state[0, 0] = total
    fill = min(total, cap)
    if fill:
        seqs = np.arange(total - fill, total)
        ids = rng.integers(0, n_ids, (fill, 8))
        ids = np.where(rng.random((fill, 8)) < 0.03, 254, ids).astype(np.uint32)
        q = rng.choice([0, 31, 127, 255], (fill, 8)).astype(np.uint32)
        rows = np.zeros((fill, 8), np.uint32)
        for h in range(2):
            rows[:, h] = sum(ids[:, 4 * h + i] << (8 * i) for i in range(4))
            rows[:, 2 + h] = sum(q[:, 4 * h + i] << (8 * i) for i in range(4))
        rows[:, 4] = rng.integers(0, S, fill)
        rows[:, 5] = rng.integers(0, 1000, fill)
        rows[:, 6] = now - np.sort(rng.integers(0, 12, fill))[::-1]
        rows[:, 7] = seqs
        state[1 + seqs % cap] = rows.view(np.int32)
    return state


def start_total(cap):
    """Appends before the first call: small logs start empty; the others so that the ring wraps inside a call of the sequence, with
    the last workgroup partly filled, or after several turns."""
    return {E - 1: E - 1 - 20, E: 4 * E - 30, E + 1: E + 1 - 40, 2 * E + 3: 2 * E + 3 - 10}.get(cap, 0)


def _differ(what, got, want):
    bad = np.argwhere(got != want)
    return '%s: %d ints differ, first at %s: got %s, want %s' % (what, len(bad), bad[0].tolist(), got[tuple(bad[0][:-1])], want[tuple(bad[0][:-1])])


@pytest.mark.parametrize('cap', CAPACITIES)
def test_sight_update_equals_numpy_spec(cap):
    """One call per read count on one log; every call is run under each of the four limits from the same state (the log is
    put back in between), and the sequence goes on from the last."""
    from yolov6.utils.sight import sight_update_np
    rng = np.random.default_rng(cap)
    confuse = C.random_confuse(rng)
    pair = (rng.random((S, S)) < 0.7).astype(np.uint8) if CAPACITIES.index(cap) % 2 else None
    now = 50
    state = prefilled_state(rng, cap, start_total(cap), now)
    log = GpuLog(state, confuse, pair)
    hits = wrapped = 0
    for V in READ_COUNTS[::-1] if cap == 5 else READ_COUNTS:
        rec = reads_of(rng, V)
        now += int(rng.integers(0, 3))
        before = state.copy()
        for mm, mc in LIMITS:
            state = before.copy()
            log.set_state(before)
            want = sight_update_np(state, confuse, pair, *rec, now, 6, 2, mm, mc)
            got = log.update(*rec, now, 6, 2, mm, mc)
            assert np.array_equal(got, want), _differ('capacity %d, %d reads, limits %s: sight_i' % (cap, V, (mm, mc)), got, want)
            dev_state = log.get_state()
            assert np.array_equal(dev_state, state), _differ('capacity %d, %d reads, limits %s: state' % (cap, V, (mm, mc)), dev_state, state)
            hits += int((got[:, :, 0] >= 0).sum())
        assert state[0, 0] == before[0, 0] + V
        wrapped += int(before[0, 0] % cap + V > cap)
    assert wrapped > 0 and (hits > 0 or cap == 1)
    if cap == 5:
        assert 2 * QB + 1 > cap                                                 # V > C on an empty log, in the first call


def test_planted_sightings_in_the_first_and_the_last_workgroup():
    """C = 2E + 3, full: slot 0 is the oldest entry and slot C - 1 the newest, three workgroups apart.  Of two equally cheap
    sightings the newer wins and n_hits counts both; a strictly cheaper one in the first workgroup wins over a newer, dearer one in
    the last; the call's own appends overwrite slots 0.. while sight_i still carries the old rows' words."""
    from yolov6.utils.sight import sight_update_np
    cap, V = 2 * E + 3, QB + 1
    rng = np.random.default_rng(7)
    state = prefilled_state(rng, cap, cap, 50)
    rec = reads_of(rng, V)
    ended_i, ended_f, _ = rec
    (s0, j0), (s1, j1) = (0, 1), (0, 2)                                         # two reads (line (0, 0) has one hit)
    x, y = rng.integers(12, 30, 8), rng.integers(30, 37, 8)                     # ids no random entry holds
    ended_i[s0, j0, 4:], ended_i[s1, j1, 4:] = x, y
    ended_f[s0, j0, :8], ended_f[s1, j1, :8] = 1.0, 0.5
    near = y.copy()
    near[3] = 5
    state[1 + 0] = SC.slot_row(x, [255] * 8, 1, 900, 45, 0)
    state[1 + cap - 1] = SC.slot_row(x, [255] * 8, 2, 901, 50, cap - 1)
    state[1 + 1] = SC.slot_row(y, [200] * 8, 3, 902, 45, 1)
    state[1 + cap - 2] = SC.slot_row(near, [200] * 8, 4, 903, 50, cap - 2)
    assert (cap - 1) // E == 2 and (cap - 2) // E == 2
    for mm, mc in ((1, 32768), (8, 32768)):
        want_state = state.copy()
        log = GpuLog(state, None, None)
        want = sight_update_np(want_state, None, None, *rec, 50, 6, 2, mm, mc)
        got = log.update(*rec, 50, 6, 2, mm, mc)
        assert np.array_equal(got, want) and np.array_equal(log.get_state(), want_state)
        assert got[s0, j0].tolist()[:3] == [cap - 1, 0, 0] and got[s0, j0, 3] >= 2 and got[s0, j0].tolist()[4:] == [2, 901, 50, cap - 1]
        assert got[s1, j1].tolist()[:3] == [1, 0, 0] and got[s1, j1, 3] >= 2 and got[s1, j1].tolist()[4:] == [3, 902, 45, 1]
        assert want_state[0, 0] == cap + V and want_state[1 + 1, 7] == cap + 1      # slot 1 now holds append C + 1


def test_argument_errors_are_refused_with_nothing_written():
    from yolov6.hip import abi
    lib = abi.load()
    rng = np.random.default_rng(3)
    cap = 40
    state = prefilled_state(rng, cap, 25, 50)
    ended_i, ended_f, ended_count = reads_of(rng, 6)
    M = ended_i.shape[1]
    st, sight = Guarded((cap + 1) * 8, 0), Guarded(S * M * 8, POISON)
    need = lib.lp_sight_workspace_bytes(S, M)
    ws = Guarded(need // 4, 0x5A5A5A5A)
    st.t.copy_(torch.from_numpy(state.reshape(-1)))
    d_i, d_f, d_n = torch.from_numpy(ended_i).cuda(), torch.from_numpy(ended_f).cuda(), torch.from_numpy(ended_count).cuda()
    now = torch.full((1,), 50, dtype=torch.int32, device='cuda')
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)   # noqa: E731

    def call(state=p(st.t), cap=cap, ei=p(d_i), now=p(now), window=6, min_hits=2, mm=1, mc=4096, out=p(sight.t), wsp=p(ws.t), ws_bytes=need, n=S):
        return lib.lp_sight_update(state, cap, None, None, ei, p(d_f), p(d_n), n, M, now, window, min_hits, mm, mc, out, wsp, ws_bytes,
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    bad = [dict(cap=0), dict(n=0), dict(window=-1), dict(min_hits=0), dict(mm=9), dict(mc=32769), dict(state=None), dict(now=None),
           dict(out=None), dict(state=p(st.t, 8)), dict(out=p(sight.t, 4)), dict(wsp=p(ws.t, 8)), dict(ws_bytes=need - 1),
           dict(out=p(st.t, 32)), dict(wsp=p(sight.t, 16)), dict(state=p(d_i))]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert np.array_equal(st.t.cpu().numpy().reshape(cap + 1, 8), state) and bool((sight.t == POISON).all()) and bool((ws.t == 0x5A5A5A5A).all())
    assert np.array_equal(d_i.cpu().numpy(), ended_i) and st.intact() and sight.intact() and ws.intact()
    assert call() == 0                                                          # and the good call writes every line
    torch.cuda.synchronize()
    assert not bool((sight.t == POISON).any())


def test_sight_log_object_many_streams_and_the_clock():
    """``SightLog`` with more lines than the prefix kernel has threads, ``now`` as an int and as a device tensor, ``clear``."""
    from yolov6.hip import runtime
    from yolov6.utils.sight import SightLogNp
    rng = np.random.default_rng(9)
    n_streams, M = 700, 3
    pair = (rng.random((n_streams, n_streams)) < 0.5).astype(np.uint8)
    log, ref = runtime.SightLog(300, n_streams, pair=pair), SightLogNp(300, n_streams, pair=pair)
    now_t = torch.zeros(1, dtype=torch.int32, device='cuda')
    hits = 0
    for k in range(3):
        ended_i, ended_f, ended_count = C.random_reads(rng, rng.integers(-1, 5, n_streams), M, n_ids=2, garbage=0.0)
        ended_i[:, :, 3] = rng.integers(0, 4, (n_streams, M))
        dev = [torch.from_numpy(a).cuda() for a in (ended_i, ended_f, ended_count)]
        now_t.fill_(10 + k)
        got = log.update(*dev, now=now_t if k % 2 else 10 + k, window=1, min_hits=2, max_mismatch=2, max_cost=1.0).cpu().numpy()
        want = ref.update(ended_i, ended_f, ended_count, now=10 + k, window=1, min_hits=2, max_mismatch=2, max_cost=1.0)
        assert np.array_equal(got, want) and np.array_equal(log.state.cpu().numpy(), ref.state) and log.total == ref.total
        hits += int((got[:, :, 0] >= 0).sum())
    assert hits > 20 and log.total > 300
    log.clear()
    assert log.total == 0 and not bool(log.state.any())
    with pytest.raises(ValueError):
        log.update(*[t[:5] for t in dev], now=0, window=1)


# ---- behind the tracker ------------------------------------------------------------------------------------------------------------------
KW = dict(max_tracks=8, match_thres=0.3, new_thres=0.2, expand=0.5, max_age=2)
SKW = dict(window=5, min_hits=1, max_mismatch=8, max_cost=6.0)


def _assert_equal(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        g = g.cpu().numpy()
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g.view(np.int32), np.ascontiguousarray(w).view(np.int32)), (what, k)


def test_steady_state_no_allocation_and_graph_capture():
    """Ten updates with the sightings enabled allocate nothing after the first; tracker, update of the log and the clock perform no
    host read: they are captured in one graph (a single chain on one stream) and the replays match the specification."""
    from yolov6.hip import runtime
    from yolov6.utils.sight import SightLogNp
    from yolov6.utils.track import PlateTrackerNp
    calls = T.random_track_case(21, n_streams=4, max_det=20, Bs=(4,) * 12)
    confuse = C.random_confuse(np.random.default_rng(1))
    trk, ref = runtime.PlateTracker(4, device='cuda', **KW), PlateTrackerNp(4, **KW)
    log, ref_log = runtime.SightLog(7, 4, confuse), SightLogNp(7, 4, confuse)
    trk.enable_sightings(log, **SKW)
    ref.enable_sightings(ref_log, **SKW)
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
        _assert_equal(got + (trk.last_sight, log.state, trk.sight_now), want + (ref.last_sight, ref_log.state, ref.sight_now), 'call %d' % k)
        hits += int((ref.last_sight[:, :, 0] >= 0).sum())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = trk.update(det, count, stream_of, flush)
        sight = trk.last_sight
    for k in (10, 11):                                                          # new rows, same buffers; log and clock move on with every replay
        det.copy_(torch.from_numpy(calls[k][0]))
        count.copy_(torch.from_numpy(calls[k][1]))
        for buf in got + (sight,):
            buf.fill_(float('nan') if buf.dtype == torch.float32 else -7)
        before = torch.cuda.memory_stats()['allocation.all.allocated']
        g.replay()
        torch.cuda.synchronize()
        assert torch.cuda.memory_stats()['allocation.all.allocated'] == before
        want = ref.update(calls[k][0], calls[k][1], stream_of, flush)
        _assert_equal(got + (sight, log.state, trk.sight_now), want + (ref.last_sight, ref_log.state, ref.sight_now), 'replay %d' % k)
        hits += int((ref.last_sight[:, :, 0] >= 0).sum())
    assert hits > 0 and ref_log.total > 7


def test_tracker_enable_sightings_equals_numpy_and_changes_nothing_else():
    from yolov6.hip import runtime
    from yolov6.utils.sight import SightLogNp
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.watch import confuse_table
    calls = T.random_track_case(31, n_streams=3, max_det=20, n_calls=12)
    confuse = confuse_table([(1, 2), (3, 8), (0, 13)], weight=3)
    pair = np.array([[0, 1, 1], [1, 1, 0], [1, 1, 1]], np.uint8)
    plain, trk, ref = runtime.PlateTracker(3, device='cuda', **KW), runtime.PlateTracker(3, device='cuda', **KW), PlateTrackerNp(3, **KW)
    log, ref_log = runtime.SightLog(9, 3, confuse, pair), SightLogNp(9, 3, confuse, pair)
    trk.enable_sightings(log, **SKW)
    ref.enable_sightings(ref_log, **SKW)
    hits = 0
    for k, (det, count, stream_of, flush) in enumerate(calls):
        d, c = torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda()
        a, b, want = plain.update(d, c, stream_of, flush, 5), trk.update(d, c, stream_of, flush, 5), ref.update(det, count, stream_of, flush, 5)
        _assert_equal(b + (trk.last_sight, log.state), want + (ref.last_sight, ref_log.state), 'call %d' % k)
        _assert_equal(a, want, 'call %d without the log' % k)
        hits += int((ref.last_sight[:, :, 0] >= 0).sum())
    assert hits > 0 and plain.last_sight is None and torch.equal(plain.state, trk.state) and int(trk.sight_now) == len(calls)
    total = log.total
    trk.reset()
    ended = trk.flush_all(max_ended=5)
    assert trk.last_sight.shape == (3, 5, 8) and ended[2].shape == (3, 5, 12) and log.total == total and total == ref_log.total > 9
    trk.enable_sightings(None)
    trk.flush_all(max_ended=5)
    assert trk.last_sight is None
    with pytest.raises(ValueError):
        trk.enable_sightings(ref_log, window=1)                                 # a host log is not a device log


# ---- Inferer(track=True, sightings=...) ----------------------------------------------------------------------------------------------------
def test_infer_sightings_match_the_cpu_path(tmp_path, monkeypatch):
    """resightings.txt of the GPU run against sight_update_np on the records PlateTrackerNp ends on the same run's untracked
    detections: the plate is hidden for four frames, so its second track names its first."""
    from PIL import Image
    from yolov6.utils.synth import build_synthetic
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    m = build_synthetic(CFG('yololps'), width=0.0625, sigma=1.5)
    ckpt = tmp_path / 'tiny.pt'
    torch.save({'model': m.half(), 'ema': None}, str(ckpt))
    (tmp_path / 'imgs').mkdir()
    n = 10
    for k, f in enumerate(SC.blinking_frames(n, range(3, 7))):
        Image.fromarray(f).save(str(tmp_path / 'imgs' / ('f%02d.png' % k)))
    kw = dict(weights=str(ckpt), source=str(tmp_path / 'imgs'), yaml=None, img_size=[128, 160], conf_thres=0.06, iou_thres=0.45, max_det=20,
              device='0', save_txt=True, not_save_img=True, half=True, batch_size=1, track_max_age=2, track_iou=0.25, track_expand=0.25)
    plain = infer.run(save_dir=str(tmp_path / 'o0'), **kw)
    _, _, ended = T.track_by_hand([d.cpu().numpy() for d in plain], 20, max_tracks=64, match_thres=0.25, new_thres=0.0, expand=0.25,
                                  max_age=2, ncls=m)
    infer.run(save_dir=str(tmp_path / 'o1'), track=True, sightings=4, sight_window=n, sight_mismatch=8, **kw)
    assert (tmp_path / 'o1' / 'plates.txt').read_text().splitlines() == T.plate_lines(ended)
    want = SC.resighting_lines(ended, SC.end_frames(ended, n, 2), 4, n, 1, 8, 32768)
    assert (tmp_path / 'o1' / 'resightings.txt').read_text().splitlines() == want and len(want) >= 1
