"""lp_stack_update on the GPU against its specification ``StackNp`` (yolov6/utils/stack.py): outputs and the whole state byte for
byte, guard bytes around everything it writes, the tracker integration (steady state, graph capture, nothing else changes) and
``tools/infer.py --stack-shots`` against the CPU chain.
"""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
import test_track_cpu as C
import test_best_shot_cpu as S
import test_stack_cpu as K
from test_best_shot_gpu import _bits_equal, _dev
from test_track_gpu import video_dir   # noqa: F401  (video_dir: the fixture)

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = 256


def _guarded(nbytes, fill):
    """(the whole buffer, its middle ``nbytes``): GUARD bytes of 0x5A on either side."""
    whole = torch.full((nbytes + 2 * GUARD,), 0x5A, dtype=torch.uint8, device='cuda')
    mid = whole[GUARD:GUARD + nbytes]
    mid.fill_(fill)
    return whole, mid


def _guards_intact(whole, what):
    g = whole.cpu().numpy()
    assert (g[:GUARD] == 0x5A).all() and (g[-GUARD:] == 0x5A).all(), '%s: guard bytes changed' % what


def state_arrays(state, n_streams, T, crop_hw):
    """The device state as the arrays of StackNp, plus every byte the layout leaves unused."""
    Hc, Wc = crop_hw
    st = state.cpu().numpy().reshape(n_streams, -1)
    en = st[:, 16:].reshape(n_streams, T, -1)
    hdr = np.ascontiguousarray(en[:, :, :16]).view(np.int32)
    acc = np.ascontiguousarray(en[:, :, 16:16 + Hc * Wc * 6]).view(np.uint16).reshape(n_streams, T, Hc, Wc, 3)
    spare = np.concatenate([st[:, 4:16].reshape(-1), en[:, :, 16 + Hc * Wc * 6:].reshape(-1)])
    return dict(frame=np.ascontiguousarray(st[:, :4]).view(np.int32)[:, 0], idp1=hdr[..., 0], n=hdr[..., 1], first=hdr[..., 2],
                last=hdr[..., 3], acc=acc), spare


def run_stack_calls(calls, n_streams, T, crop_hw, **params):
    """calls = [(inputs, (stack_crops, stack_i) wanted, state arrays wanted)] through lp_stack_update on a zeroed state: every
    output and the whole state byte for byte after every call, stack_crops / stack_i poisoned before it, the guard bytes around the
    state and both outputs unchanged."""
    from yolov6.hip import abi, runtime
    lib, dev = abi.load(), torch.device('cuda', torch.cuda.current_device())
    p = abi.StackParams(params.get('min_score', 0.0), params.get('min_width', 0.0), params.get('min_sharp', 0), params.get('search', 2),
                        params.get('max_frames', 64))
    nbytes = lib.lp_stack_state_bytes(n_streams, T, *crop_hw)
    assert nbytes > 0
    state_whole, state = _guarded(nbytes, 0)
    for k, (inp, want, want_state) in enumerate(calls):
        B, max_det, max_crops, max_ended = len(inp['det']), inp['det'].shape[1], inp['crops'].shape[1], inp['ended_i'].shape[1]
        t = {name: _dev(inp[name]) for name in ('det', 'count', 'tid', 'slot', 'crops', 'status', 'sharp', 'ended_i', 'ended_count')}
        so = (ctypes.c_int * max(B, 1))(*inp['stream_of'])
        sc_whole, sc = _guarded(n_streams * max_ended * crop_hw[0] * crop_hw[1] * 3, 0xAB)
        si_whole, si = _guarded(n_streams * max_ended * 16, 0xF9)
        with torch.cuda.device(dev):
            abi.check(lib.lp_stack_update(state.data_ptr(), n_streams, T, crop_hw[0], crop_hw[1], t['det'].data_ptr(), t['count'].data_ptr(),
                                          B, max_det, t['tid'].data_ptr(), t['slot'].data_ptr(), t['crops'].data_ptr(),
                                          t['status'].data_ptr(), t['sharp'].data_ptr(), max_crops, so, t['ended_i'].data_ptr(),
                                          t['ended_count'].data_ptr(), max_ended, ctypes.byref(p), sc.data_ptr(), si.data_ptr(),
                                          runtime._stream_ptr(dev)), 'lp_stack_update')
        torch.cuda.synchronize()
        what = 'call %d' % k
        _bits_equal(si.view(torch.int32).view(n_streams, max_ended, 4), want[1], what + ': stack_i')
        _bits_equal(sc.view((n_streams, max_ended) + tuple(crop_hw) + (3,)), want[0], what + ': stack_crops')
        got, spare = state_arrays(state, n_streams, T, crop_hw)
        for name in ('frame', 'idp1', 'n', 'first', 'last', 'acc'):
            assert np.array_equal(got[name], want_state[name]), '%s: state %s differs' % (what, name)
        assert not spare.any(), what + ': unused state bytes written'
        for whole, name in ((state_whole, 'state'), (sc_whole, 'stack_crops'), (si_whole, 'stack_i')):
            _guards_intact(whole, '%s: %s' % (what, name))


def np_calls(calls, n_streams, T, crop_hw, **params):
    """The expectations of ``run_stack_calls`` for a list of input dicts, from a fresh StackNp (returned too)."""
    from yolov6.utils.stack import StackNp
    stk = StackNp(n_streams, T, crop_hw, **params)
    res = K.run_np(stk, calls)
    stk.all_shifts = [(dy, dx) for _, sh, _ in res for _, _, _, dy, dx in sh]      # of every crop summed, in order
    return stk, [(inp, out, state) for inp, (out, _, state) in zip(calls, res)]


# ---- random calls -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', range(4), ids=S.SHOT_IDS)
def test_stack_update_equals_numpy_spec_on_random_calls(k):
    """The random track cases: slot reuse inside a call, a mid-sequence flush, 70 frames in a call (two launches) on nine streams,
    untracked frames, counts below 0 and above max_det, max_crops < max_det with records cut off, a 64 x 192 crop."""
    seed, n_streams, T, max_det, Bs, crop_hw, max_crops, max_ended, kw = S.SHOT_CASES[k]
    stk, calls = K.stack_case(k)
    K.check_stack_case(k, stk, calls)
    assert any(-1 in inp['stream_of'] for inp, _, _ in calls)
    if k == 2:
        assert any((inp['count'] < 0).any() for inp, _, _ in calls) and any((inp['count'] > max_det).any() for inp, _, _ in calls)
        assert max(len(inp['det']) for inp, _, _ in calls) > 64
    run_stack_calls(calls, n_streams, T, crop_hw, **K.STACK_KW[k])


def test_rows_with_a_slot_outside_the_range_are_skipped():
    calls = K.reuse_calls()
    calls[0]['tid'][0, 2], calls[0]['slot'][0, 2], calls[0]['count'][0] = 7, 2, 3          # slot == max_tracks
    calls[0]['tid'][1, 2], calls[0]['slot'][1, 2], calls[0]['count'][1] = 7, -3, 3
    stk, want = np_calls(calls, 2, 2, (5, 7), search=1)
    assert stk.stats['reused'] == 2 and stk.stats['summed'] == 7
    run_stack_calls(want, 2, 2, (5, 7), search=1)


# ---- crop sizes and search radii ------------------------------------------------------------------------------------------------------
def shifted_frames(hw, R, n, seed):
    """n crops of one random picture, each cut at an offset within +-R and with a little noise of its own."""
    rng = np.random.default_rng(seed)
    big = rng.integers(0, 256, (hw[0] + 2 * R, hw[1] + 2 * R, 3)).astype(np.int64)
    off = rng.integers(-R, R + 1, (n, 2))
    frames = np.stack([big[R + oy:R + oy + hw[0], R + ox:R + ox + hw[1]] for oy, ox in off])
    return np.clip(frames + rng.integers(-6, 7, frames.shape), 0, 255).astype(np.uint8)


@pytest.mark.parametrize('R', [0, 1, 2, 4])
@pytest.mark.parametrize('hw', [(64, 192), (5, 5), (4, 9), (3, 200), (7, 13)], ids=lambda hw: '%dx%d' % hw)
def test_crop_sizes_and_search_radii(hw, R):
    """7 x 13: an odd uint16 row pitch (78 bytes) and an entry that is no multiple of 16 bytes; 5 x 5, 4 x 9 and 3 x 200 switch
    the search off for the larger radii; two slots, so that the second entry's sum starts where the first one's padding ends."""
    calls = K.one_track_calls(shifted_frames(hw, R, 4, 10 * hw[0] + R), chunk=3)
    for inp in calls:                                          # the track sits in slot 1 of 2
        inp['slot'][:] = 1
    stk, want = np_calls(calls, 1, 2, hw, search=R)
    searched = R > 0 and hw[0] > 2 * R and hw[1] > 2 * R
    assert stk.stats['summed'] == 4 and (searched or stk.stats['shifted'] == 0) and (stk.stats['shifted'] > 0 or not searched or hw[0] < 7)
    assert want[-1][1][1][0, 0].tolist() == [4, 0, 3, 1]
    run_stack_calls(want, 1, 2, hw, search=R)


def test_a_1024_x_1024_crop_crosses_every_band():
    """Three frames: the second and third are searched against the sum in bands of a few rows each."""
    hw = (1024, 1024)
    calls = K.one_track_calls(shifted_frames(hw, 2, 3, 77))
    stk, want = np_calls(calls, 1, 1, hw, search=2)
    assert stk.stats['summed'] == 3 and stk.stats['shifted'] >= 1
    run_stack_calls(want, 1, 1, hw, search=2)


# ---- the edges of the rule that exercise the kernel's arithmetic ------------------------------------------------------------------------
@pytest.mark.parametrize('crops', [K.flat_crops, K.stripe_crops, K.tie_crops], ids=['flat', 'stripes', 'tie'])
def test_ties_go_to_the_lower_candidate(crops):
    calls = K.one_track_calls(crops())
    stk, want = np_calls(calls, 1, 1, (7, 13), search=2)
    assert stk.all_shifts[-1] == ((0, -1) if crops is K.tie_crops else (0, 0))
    run_stack_calls(want, 1, 1, (7, 13), search=2)


def test_255_white_frames_fill_the_sum_and_the_256th_is_left_out():
    white = np.full((256, 5, 7, 3), 255, np.uint8)
    white[255] = 0
    calls = K.one_track_calls(white, chunk=100)
    stk, want = np_calls(calls, 1, 1, (5, 7), search=1, max_frames=255)
    assert stk.stats['full'] == 1 and (want[-2][2]['acc'] == 65025).all() and (want[-1][1][0][0, 0] == 255).all()
    run_stack_calls(want, 1, 1, (5, 7), search=1, max_frames=255)


def test_a_cost_above_32_bits_decides_the_minimum():
    hw, R = (24, 40), 2
    calls = K.one_track_calls(K.wide_cost_crops(hw, R), chunk=67)
    stk, want = np_calls(calls, 1, 1, hw, search=R, max_frames=255)
    assert stk.stats['summed'] == 201 and stk.stats['shifted'] == 1 and stk.all_shifts[200] == (-R, 0)
    run_stack_calls(want, 1, 1, hw, search=R, max_frames=255)


def test_slot_reuse_truncation_and_a_stream_without_frames():
    calls = K.reuse_calls()
    stk, want = np_calls(calls, 2, 2, (5, 7), search=1)
    assert stk.stats['reused'] == 2 and stk.stats['closed'] == 1
    run_stack_calls(want, 2, 2, (5, 7), search=1)
    calls = K.reuse_calls()
    calls[0]['ended_i'][1, 1, 0] = 99
    stk, want = np_calls(calls, 2, 2, (5, 7), search=1)
    assert stk.stats['truncated'] == 1
    run_stack_calls(want, 2, 2, (5, 7), search=1)


def test_eligibility_thresholds():
    rng = np.random.default_rng(5)
    crops = rng.integers(0, 256, (9, 5, 7, 3), dtype=np.uint8)
    rows = np.stack([C.make_row((10, 10, 110, 40))] * 9)
    rows[4, 15], rows[5, 2], rows[6, 2], rows[7, 2] = C.NAN, C.NAN, 10 + 99.5, 10 + 100.0
    calls = K.one_track_calls(crops, status=[1, 0, 2, 3, 1, 1, 1, 1, 1], rows=rows, sharp=[7, 7, 7, 7, 7, 7, 7, 7, 6])
    kw = dict(search=1, min_width=100.0, min_sharp=7, min_score=0.9)
    stk, want = np_calls(calls, 1, 1, (5, 7), **kw)
    assert stk.stats['summed'] == 2 and want[-1][1][1][0, 0].tolist() == [2, 0, 7, 1]
    run_stack_calls(want, 1, 1, (5, 7), **kw)


# ---- PlateTracker.enable_stack -----------------------------------------------------------------------------------------------------------
def _same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_enable_stack_steady_state_graph_capture_and_nothing_else_changes():
    """Twelve random calls through PlateTracker with and without ``enable_stack`` and through PlateTrackerNp.enable_stack: the
    nine tensors and the tracker's and gallery's state are bit-identical with and without it, ``last_stack`` matches the numpy
    chain, calls 1..9 allocate nothing, and the chain captured in one graph replays calls 10 and 11 to the same bytes."""
    from yolov6.hip import runtime
    from yolov6.utils.track import PlateTrackerNp
    n_streams, max_det, max_crops, crop_hw = 4, 20, 6, (8, 24)
    calls = C.random_track_case(21, n_streams=n_streams, max_det=max_det, extent=150, Bs=(4,) * 12)
    kw = dict(max_tracks=8, match_thres=0.3, new_thres=0.2, expand=0.5, max_age=2)
    skw = dict(search=2, max_frames=3, min_width=20.0, min_sharp=1)
    trk, plain, ref = runtime.PlateTracker(n_streams, device='cuda', **kw), runtime.PlateTracker(n_streams, device='cuda', **kw), \
        PlateTrackerNp(n_streams, **kw)
    with pytest.raises(RuntimeError):
        trk.enable_stack()                                      # needs the gallery first
    for t in (trk, plain):
        t.enable_best_shot(crop_hw, max_crops=max_crops, min_score=0.2)
    trk.enable_stack(**skw)
    ref.enable_stack(crop_hw=crop_hw, max_crops=max_crops, min_score=0.2, **skw)
    rng = np.random.default_rng(7)
    frames_np = [rng.integers(0, 256, (170 + 3 * b, 220 - 5 * b, 3), dtype=np.uint8) for b in range(4)]
    frames = [torch.from_numpy(f).cuda() for f in frames_np]
    stream_of = [0, 1, 3, 1]
    det, count = torch.from_numpy(calls[0][0]).cuda(), torch.from_numpy(calls[0][1]).cuda()

    def spec(k):
        for f in frames_np:
            f[:] = np.roll(f, 3, axis=1)                    # the scene moves: every call sees other pixels
        ref.update(calls[k][0], calls[k][1], stream_of)
        sc, si = ref.update_stack(frames_np, calls[k][0], calls[k][1], stream_of)
        return sc.copy(), si.copy()

    def load(k):
        det.copy_(torch.from_numpy(calls[k][0]))
        count.copy_(torch.from_numpy(calls[k][1]))
        for f, fn in zip(frames, frames_np):
            f.copy_(torch.from_numpy(fn))

    def compare(got9, want, what):
        other = plain.update_with_shots(frames, det, count, stream_of)
        torch.cuda.synchronize()
        assert plain.last_stack is None
        for a, b in zip(got9, other):
            valid = slice(None)
            if a.dim() == 5:                                    # shot_crops: lines without a shot keep what they held
                valid = got9[6][..., 3] == 1
            assert _same_bytes(a[valid], b[valid]), what
        sc, si = trk.last_stack
        _bits_equal(si, want[1], what + ': stack_i')
        _bits_equal(sc, want[0], what + ': stack_crops')

    valid = 0
    for k in range(10):
        want = spec(k)
        load(k)
        before = torch.cuda.memory_stats()['allocation.all.allocated']
        got = trk.update_with_shots(frames, det, count, stream_of)
        if k:
            assert torch.cuda.memory_stats()['allocation.all.allocated'] == before, k
        assert len(got) == 9
        compare(got, want, 'call %d' % k)
        valid += int(want[1][..., 3].sum())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = trk.update_with_shots(frames, det, count, stream_of)
    for k in (10, 11):                                          # capture enqueued nothing: the first replay is call 10
        want = spec(k)
        load(k)
        trk.last_stack[1].fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        compare(got, want, 'replay %d' % k)
        valid += int(want[1][..., 3].sum())
    assert valid > 0 and ref._stack['np'].stats['summed'] > 0 and ref._stack['np'].stats['full'] > 0
    assert torch.equal(trk.state, plain.state) and torch.equal(trk._shots['state'], plain._shots['state'])
    # the flush hands out what is left; reset empties the stacks with the rest
    ref.flush_all()
    want = ref.update_stack([], np.zeros((0, 1, 28), f32), [], [])
    trk.flush_all_with_shots()
    _bits_equal(trk.last_stack[1], want[1], 'flush: stack_i')
    assert int(want[1][..., 3].sum()) > 0
    trk.update_with_shots(frames, det, count, stream_of)
    assert trk._stack['state'].any()
    trk.reset([0, 1])
    st = trk._stack['state'].view(n_streams, -1)
    assert not st[:2].any() and st[3].any()
    trk.reset()
    assert not trk._stack['state'].any()
    trk.enable_stack(None)
    assert trk._stack is None and trk.last_stack is None


# ---- Inferer(track=True, best_shots=True, stack_shots=True) ---------------------------------------------------------------------------
@pytest.mark.parametrize('batch_size', [1, 8])
def test_infer_stack_shots_matches_the_cpu_chain(video_dir, tmp_path, monkeypatch, batch_size):   # noqa: F811
    """infer.run(..., stack_shots=True) on the GPU against PlateTrackerNp + plate_crops_np + StackNp on the same detections."""
    from yolov6.core.inferer import Inferer
    from yolov6.data.datasets import imread_bgr
    from yolov6.hip import runtime
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    src, ckpt, size, max_det = video_dir / 'imgs', video_dir / 'tiny.pt', [128, 160], 20
    files = sorted(os.listdir(str(src)))
    out = tmp_path / 'out'
    skw = dict(search=1, max_frames=4, min_width=8.0)
    res = infer.run(weights=str(ckpt), source=str(src), yaml=None, img_size=size, conf_thres=0.06, iou_thres=0.45, max_det=max_det,
                    device='0', save_txt=True, not_save_img=True, half=True, save_dir=str(out), track=True, track_max_age=2,
                    track_iou=0.25, track_expand=0.25, best_shots=True, crop_size=(16, 48), stack_shots=True, stack_search=1,
                    stack_max_frames=4, stack_min_width=8.0, batch_size=batch_size)
    model = Inferer(str(src), str(ckpt), '0', None, size, True).model.model          # the checkpoint as Inferer prepares it
    frames_np = [np.ascontiguousarray(imread_bgr(str(src / f))) for f in files]
    with torch.no_grad():
        plain = runtime.detect_frames(model, [torch.from_numpy(f).cuda() for f in frames_np], size, 0.06, 0.45, max_det)
    assert len(res) == len(files) and sum(len(d) for d in plain) >= len(files)
    ended, stacks = K.stacks_by_hand(frames_np, [d.cpu().numpy() for d in plain], max_det, (16, 48), max_crops=Inferer.SHOT_ROWS,
                                     stack_kw=skw, max_tracks=64, match_thres=0.25, new_thres=0.0, expand=0.25, max_age=2, ncls=model)
    assert K.check_stack_files(out, ended, stacks) >= 1
    assert (out / 'shots.txt').exists()
