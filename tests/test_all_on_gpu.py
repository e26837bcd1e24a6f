"""The tracker's add-ons together, on the GPU: one ``runtime.PlateTracker`` with best shot, stack, hold, watchlist, live watch and
sightings enabled and a ``LookbackRedactor`` behind it, against the all-on numpy chain of tests/test_all_on_cpu.py and against the
same feature enabled alone on a second GPU tracker -- every comparison an equality of bytes; ``reset`` of one stream in the middle;
the steady state (no allocation, one update plus push captured in a graph); and ``tools/infer.py`` with every flag on its GPU paths,
every file byte-identical to the run with that flag alone.  Every output buffer is poisoned before each call."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
import lp_testing as L
import test_track_cpu as C
from test_stack_gpu import state_arrays
from test_watch_live_gpu import poison as poison_live

pytestmark = pytest.mark.gpu
P = L.ALL_ON


def _poison(*bufs):
    for buf in bufs:
        buf.fill_(float('nan') if buf.dtype == torch.float32 else (P['poison'] if buf.dtype == torch.uint8 else -7))


class AllOnGpu:
    """``lp_testing.AllOnNp`` on the device: the same features on one ``runtime.PlateTracker`` (enabled in the Inferer's order) and a
    ``LookbackRedactor``; ``step`` returns the same outputs by name, as numpy arrays."""

    def __init__(self, features=L.ALL_ON_FEATURES):
        from yolov6.hip import runtime
        _, entries, confuse = L.all_on_case()
        self.on = L.all_on_features(features)
        S = P['n_streams']
        self.trk = trk = runtime.PlateTracker(S, device='cuda', **P['track'])
        self.lb = self.log = self.wl = None
        if 'watch' in self.on or 'live' in self.on:
            self.wl = runtime.Watchlist(entries, confuse)
        if 'watch' in self.on:
            trk.enable_watch(self.wl, **P['watch'])
        if 'live' in self.on:
            trk.enable_live_watch(self.wl, P['live']['min_hits'], **P['watch'])
        if 'sight' in self.on:
            self.log = runtime.SightLog(P['sight_capacity'], S, confuse)
            trk.enable_sightings(self.log, **P['sight'])
        if 'hold' in self.on:
            trk.enable_hold(**P['hold'])
        if 'lookback' in self.on:
            self.lb = runtime.LookbackRedactor(trk, P['depth'], **P['redact'])
        if 'shot' in self.on:
            trk.enable_best_shot(P['crop_hw'], max_crops=P['max_crops'], **P['shot'])
        if 'stack' in self.on:
            trk.enable_stack(**P['stack'])

    def reset(self, streams):
        self.trk.reset(streams)
        if self.lb is not None:
            self.lb.reset(streams)

    def poison(self, B, max_det):
        trk, S, E = self.trk, P['n_streams'], P['max_ended']
        _poison(*trk.buffers(B, max_det, E), trk.slot_buffer(B, max_det))
        if 'hold' in self.on:
            _poison(*trk.hold_buffers(B, max_det))
        if 'watch' in self.on:
            _poison(self.wl.buffers(S, E)[0])
        if 'live' in self.on:
            poison_live(trk)
        if 'sight' in self.on:
            _poison(self.log.buffers(S, E)[0])
        if 'shot' in self.on:
            _poison(*trk.shot_buffers(B, E))
        if 'stack' in self.on:
            _poison(*trk.stack_buffers(E))
        if self.lb is not None:
            _poison(*(t for out in self.lb._out.values() for t in out), *self.lb._status.values())

    def enqueue(self, det, count, stream_of, flush, frames):
        """One update plus push, nothing read back: (what update returned, what push returned)."""
        if 'shot' in self.on:
            got = self.trk.update_with_shots(frames, det, count, stream_of, flush, P['max_ended'])
        else:
            got = self.trk.update(det, count, stream_of, flush, P['max_ended'])
        return got, (self.lb.push(frames, stream_of, flush) if self.lb is not None else None)

    def read(self, got, done, B, max_det):
        trk, n = self.trk, lambda t: t.cpu().numpy()                            # noqa: E731
        torch.cuda.synchronize()
        out = dict(zip(L.ALL_ON_OUTPUTS['track'], (n(got[0]), n(got[1]), n(trk.slot_buffer(B, max_det)), n(got[2]), n(got[3]), n(got[4]))))
        assert trk.last_tid is got[1]
        if 'hold' in self.on:
            out.update(zip(L.ALL_ON_OUTPUTS['hold'], map(n, trk.last_hold)))
        if 'watch' in self.on:
            out['match_i'] = n(trk.last_watch)
        if 'live' in self.on:
            out.update(zip(L.ALL_ON_OUTPUTS['live'], map(n, (trk.last_live,) + tuple(trk.last_live_reads))))
        if 'sight' in self.on:
            out['sight_i'] = n(trk.last_sight)
        if 'shot' in self.on:
            out.update(zip(L.ALL_ON_OUTPUTS['shot'], (n(got[5]), n(got[6]), n(got[7]).view(np.uint64), n(got[8]))))
        if 'stack' in self.on:
            out.update(zip(L.ALL_ON_OUTPUTS['stack'], map(n, trk.last_stack)))
        if done is not None:
            out['released'] = [(s, g, n(f)) for s, g, f in done]
        return out

    def step(self, det, count, stream_of, flush, frames):
        d, c = torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda()
        dev = [torch.from_numpy(f).cuda() for f in frames]
        self.poison(len(det), det.shape[1])
        got, done = self.enqueue(d, c, stream_of, flush, dev)
        return self.read(got, done, len(det), det.shape[1])


def gpu_run(features=L.ALL_ON_FEATURES, reset=True, first=0):
    """``lp_testing.all_on_run`` on the device."""
    calls = L.all_on_case()[0]
    chain, outs = AllOnGpu(features), []
    for c, call in enumerate(calls):
        if c < first:
            continue
        if reset and c == P['reset_before']:
            chain.reset(P['reset_streams'])
        outs.append(chain.step(*call))
    return chain, outs


_gpu = {}


def gpu_reference():
    """(chain, outputs per call) of the all-on GPU run with the reset, once per process."""
    if 'ref' not in _gpu:
        _gpu['ref'] = gpu_run()
    return _gpu['ref']


def assert_runs_equal(got, want, names, what):
    assert len(got) == len(want)
    for c, (g, w) in enumerate(zip(got, want)):
        diff = L.all_on_differences([w], [g], names)
        if diff:
            k = diff[0]
            where = ''
            if k != 'released' and g[k].shape == w[k].shape:
                bad = np.argwhere(np.ascontiguousarray(g[k]).view(np.uint8).reshape(g[k].shape + (-1,)) !=
                                  np.ascontiguousarray(w[k]).view(np.uint8).reshape(w[k].shape + (-1,)))
                where = ', %d bytes, first at %s: got %r, want %r' % (len(bad), bad[0][:-1].tolist(), g[k][tuple(bad[0][:-1])], w[k][tuple(bad[0][:-1])])
            elif k == 'released':
                where = ': got %s, want %s' % ([(s, f) for s, f, _ in g[k]][:8], [(s, f) for s, f, _ in w[k]][:8])
            raise AssertionError('%s, call %d: %s differ%s' % (what, c, diff, where))


# ---- 2. runtime.PlateTracker with everything enabled ---------------------------------------------------------------------------------
def test_all_on_equals_the_all_on_numpy_chain():
    """Every returned tensor, every ``last_*`` attribute, the slot buffer and the frames that leave the delay line, call by call."""
    _, want = L.all_on_reference()
    chain, got = gpu_reference()
    names = [n for f in ('track',) + L.ALL_ON_FEATURES for n in L.ALL_ON_OUTPUTS[f]]
    assert set(got[0]) == set(want[0]) == set(names)
    assert_runs_equal(got, want, names, 'all on against numpy')
    ref = L.all_on_reference()[0]
    assert np.array_equal(chain.trk.dropped.cpu().numpy(), ref.trk.dropped) and np.array_equal(chain.lb.dropped, ref.lb.dropped)
    assert np.array_equal(chain.log.state.cpu().numpy(), ref.log.state) and int(chain.trk.sight_now) == len(P['Bs'])


@pytest.mark.parametrize('feature', L.ALL_ON_FEATURES)
def test_all_on_equals_the_feature_alone_on_a_second_tracker(feature):
    _, want = gpu_reference()
    chain, got = gpu_run((feature,))
    names = [n for f in ('track',) + chain.on for n in L.ALL_ON_OUTPUTS[f]]
    assert set(got[0]) == set(names)
    assert_runs_equal(got, want, names, feature + ' alone against all on')


def test_after_the_final_flush_the_state_is_empty():
    """Tracker and live memo: every per-slot word is zero.  Gallery and stack: an entry is occupied (its id word) exactly where the
    numpy chain's is -- the occupants of records that ``max_ended`` cut off, which their rule keeps until the slot is reused
    (tests/test_all_on_cpu.py ties those to the cut) -- and every stream whose records all fit is empty in both."""
    chain, outs = gpu_reference()
    ref = L.all_on_reference()[0]
    trk, S, T = chain.trk, P['n_streams'], P['track']['max_tracks']
    assert not trk.state.view(S, -1)[:, 16:].any() and not trk.live_memo.any()
    head = trk._shots['state'].view(S, -1)[:, 16:].view(S, T, -1)[:, :, :8].contiguous().view(torch.int32).cpu().numpy()
    assert np.array_equal(head[:, :, 0], ref.gal.idp1) and np.array_equal(head[:, :, 1], ref.gal.has)
    stk, spare = state_arrays(trk._stack['state'], S, T, P['crop_hw'])
    assert np.array_equal(stk['idp1'], ref.trk._stack['np'].idp1) and np.array_equal(stk['n'], ref.trk._stack['np'].n) and not spare.any()
    cut = [any(int(o['ended_count'][s]) > P['max_ended'] for o in outs) for s in range(S)]
    assert any(cut) and not all(cut)
    for s in range(S):
        assert cut[s] or (not head[s, :, 0].any() and not stk['idp1'][s].any()), s


def test_reset_of_one_stream_in_the_middle_of_the_run():
    """From the reset on, streams 0 and 2 continue exactly as on a tracker that is not reset, and stream 1 as on a fresh one that
    starts at that call (the sightings aside: one log for all streams, which survives a reset by design)."""
    calls = L.all_on_case()[0]
    first = P['reset_before']
    _, with_reset = gpu_reference()
    _, without = gpu_run(reset=False)
    _, fresh = gpu_run(reset=False, first=first)
    differs = 0
    for c in range(first, len(calls)):
        so = calls[c][2]
        for s in range(P['n_streams']):
            a = L.all_on_stream_part(with_reset[c], so, s)
            b = L.all_on_stream_part(fresh[c - first] if s in P['reset_streams'] else without[c], so, s)
            assert L.all_on_differences([a], [b]) == [], (c, s)
            if s in P['reset_streams']:
                differs += len(L.all_on_differences([a], [L.all_on_stream_part(without[c], so, s)]))
    assert differs > 0


def test_steady_state_no_allocation_and_one_update_plus_push_in_a_graph():
    """Sixteen calls of four frames (streams 0, 1, 2, 1) with everything on.  The caller keeps its frames in a ring of depth + 1
    sets, so that a set is written again only after the delay line has handed its frames back.  Every call equals the numpy chain;
    once every stage has run (from the first call in which frames of every stream leave the delay) a call allocates nothing; call
    10's update plus push is captured in a graph, and its replays -- as call 10 and, one turn of the ring later, as call 15, on new
    rows and frames -- give the bytes of the numpy chain that the eager calls around them give."""
    D, so, n_calls = P['depth'], [0, 1, 2, 1], 16
    R = D + 1
    calls = C.random_track_case(21, n_streams=P['n_streams'], max_det=P['max_det'], n_obj=2, extent=40, Bs=(4,) * n_calls)
    rng = np.random.default_rng(9)
    H, W = P['frame_hw']
    base = rng.integers(0, 256, (H + 16, W + 64, 3), dtype=np.uint8)
    base[::2] //= 3
    frames_np = [[np.ascontiguousarray(base[(5 * (4 * k + b)) % 16:, (7 * (4 * k + b)) % 64:][:H, :W]) for b in range(4)] for k in range(n_calls)]
    ref, chain = L.AllOnNp(), AllOnGpu()
    ring = [[torch.zeros(H, W, 3, dtype=torch.uint8, device='cuda') for _ in range(4)] for _ in range(R)]
    det, count = torch.from_numpy(calls[0][0]).cuda(), torch.from_numpy(calls[0][1]).cuda()
    names = [n for f in ('track',) + L.ALL_ON_FEATURES for n in L.ALL_ON_OUTPUTS[f]]

    def load(k):
        det.copy_(torch.from_numpy(calls[k][0]))
        count.copy_(torch.from_numpy(calls[k][1]))
        for t, f in zip(ring[k % R], frames_np[k]):
            t.copy_(torch.from_numpy(f))
        chain.poison(4, P['max_det'])

    def check(k, got, done, what):
        want = ref.step(calls[k][0], calls[k][1], so, None, frames_np[k])
        out = chain.read(got, done, 4, P['max_det'])
        if 'replay' in what:                                                    # the frame numbers are those of the captured call
            want['released'] = [(s, 0, f) for s, _, f in want['released']]
            out['released'] = [(s, 0, f) for s, _, f in out['released']]
        assert_runs_equal([out], [want], names, what)
        return want

    seen = dict(released=0, shots=0, stacks=0, alerts=0)
    for k in list(range(10)) + [10, 10, 11, 12, 13, 14, 15]:
        load(k)
        if k in (10, 15) and 'graph' in seen:
            seen['graph'].replay()
            want = check(k, *seen['captured'], 'replay as call %d' % k)
        elif k == 10:
            torch.cuda.synchronize()
            seen['graph'] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(seen['graph']):
                seen['captured'] = chain.enqueue(det, count, so, None, ring[k % R])
            continue                                                            # the capture ran nothing: the first replay is call 10
        else:
            torch.cuda.synchronize()
            before = torch.cuda.memory_stats()['allocation.all.allocated']
            got, done = chain.enqueue(det, count, so, None, ring[k % R])
            if k > D:
                assert torch.cuda.memory_stats()['allocation.all.allocated'] == before, k
            want = check(k, got, done, 'call %d' % k)
        seen['released'] += len(want['released'])
        seen['shots'] += int(want['shot_i'][..., 3].sum())
        seen['stacks'] += int(want['stack_i'][..., 3].sum())
        seen['alerts'] += int((want['live_i'][..., 5] == 1).sum())
    assert seen['released'] == 4 * n_calls - (2 * D + D) and seen['shots'] > 0 and seen['stacks'] > 0 and seen['alerts'] > 0, seen


# ---- 3. Inferer with every flag ------------------------------------------------------------------------------------------------------
INFER_SETTINGS = {
    'b1': dict(batch_size=1),
    'b8': dict(batch_size=8),
    'b8-nv12': dict(batch_size=8, nv12='bt709'),
    'tile-gate': dict(batch_size=8, tile=[96, 96], tile_overlap=24, tile_gate=True),
}


@pytest.fixture(scope='module')
def infer_source(tmp_path_factory):
    return L.all_on_infer_source(tmp_path_factory.mktemp('all_on'))


@pytest.mark.parametrize('setting', list(INFER_SETTINGS))
def test_infer_with_every_flag_writes_the_files_of_every_flag_alone(infer_source, tmp_path, monkeypatch, setting):
    """track, best_shots, stack_shots, watchlist, watch_live, sightings, redact='mosaic', redact_hold, redact_lookback=4 and
    save_crops in one run: every file of the run with each of them alone (with what it needs: the stack with the best shot, the
    live watch with the watchlist, the look-back with the hold) is byte-identical in it.  The shots and stacks of a run without
    redaction in particular: that pins cut before redact.  (The single runs are tied to the numpy chains by the tests of each
    feature.)"""
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    ckpt, src = infer_source
    files = L.all_on_infer(infer, tmp_path, ckpt, src, setting, device='0', half=True, **INFER_SETTINGS[setting])
    n = L.assert_all_on_files(files, setting)
    print('%s: files compared %s of %d' % (setting, n, len(files['all'])))
    assert n['lookback'] > n['hold'] == n['track'] and n['stacks'] > n['shots'] > n['track'] and n['crops'] > n['track']
