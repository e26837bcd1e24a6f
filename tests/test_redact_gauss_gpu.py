"""Gaussian-blur redaction on the GPU: lp_redact_gauss_batch (runtime.redact_plates(mode='gauss')) byte for byte against the numpy
specification (yolov6/utils/redact.py): a sweep over sigmas, margins, formats and counts on frames with interior tiles, partial
edge tiles, halos wider than a tile and wider than the frame, with guard and padding bytes, poisoned status and workspace; the
64-frame launch split and the workspace-cap split; graph capture; every argument error; LookbackRedactor against LookbackNp; and
Inferer(redact='gauss') at batch sizes 1 and 4."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
import test_lookback_cpu as L
import test_track_cpu as C
from test_lookback_gpu import _assert_frames_equal, _to_device
from test_redact_gpu import CFG, COUNTS, MAX_DET, ST_POISON, bgr_buffer, expect_buffer, host_frames, nv12_buffer, rows_for

pytestmark = pytest.mark.gpu

# the blur tile is 32 x 32: (70, 131) and (72, 134) have interior tiles, partial edge tiles and more than two tiles a side;
# at sigma 16 (radius 48) a halo spans more than one neighbouring tile, and is larger than the small frames
BGR_SHAPES = [(37, 53), (70, 131), (1, 1), (5, 200)]
NV12_SHAPES = [(38, 54, 70, 60), (2, 2, 5, 6), (72, 134, 140, 136)]        # h, w, pitch_y, pitch_uv


def table_bytes(frames):
    return sum((f.shape[0] * f.shape[1] + 3) // 4 * 16 for f in frames)


def check_call(buf, frames, det, count, ws_poison=(0xA5, 0x00), **kw):
    """redact_plates(mode='gauss') on ``frames`` (views of ``buf``) with the workspace and the status poisoned, once per workspace
    poison from the same start: every byte of the buffer and every status must be the specification's.  Returns the number of
    changed bytes."""
    from yolov6.hip import runtime
    from yolov6.utils.redact import redact_plates_np
    start = buf.clone()
    want, want_st = redact_plates_np(host_frames(frames), det.cpu().numpy(), count.cpu().numpy(), mode='gauss', **kw)
    want_buf = expect_buffer(buf, start, frames, want)
    for poison in ws_poison:
        buf.copy_(start)
        runtime._redact_workspace(buf.device, table_bytes(frames)).fill_(poison)
        status = torch.full((len(frames), det.shape[1]), ST_POISON, dtype=torch.int32, device='cuda')
        got_st = runtime.redact_plates(frames, det, count, status=status, mode='gauss', **kw)
        torch.cuda.synchronize()
        assert got_st.data_ptr() == status.data_ptr()
        assert np.array_equal(status.cpu().numpy(), want_st)
        assert torch.equal(buf, want_buf)                           # the frames, and every guard and padding byte
    changed = int((want_buf != start).sum())
    buf.copy_(start)
    return changed


CASES = [(sigma, margin) for sigma in (0.5, 2.5, 16) for margin in (0.0, 0.25)]


@pytest.mark.parametrize('k', range(len(CASES)), ids=['sigma%g-m%g' % c for c in CASES])
def test_kernels_equal_specification(k):
    sigma, margin = CASES[k]
    buf, frames = bgr_buffer(BGR_SHAPES, 100 + k)
    count = torch.tensor([COUNTS[(b + k + 2) % 5] for b in range(4)], dtype=torch.int32, device='cuda')
    changed = check_call(buf, frames, rows_for(BGR_SHAPES, 200 + 10 * k), count, sigma=sigma, margin=margin)
    nbuf, nframes = nv12_buffer(NV12_SHAPES, 300 + k)
    ncount = torch.tensor([COUNTS[(b + k) % 5] for b in range(3)], dtype=torch.int32, device='cuda')
    changed += check_call(nbuf, nframes, rows_for(NV12_SHAPES, 400 + 10 * k), ncount, sigma=sigma, margin=margin)
    assert changed > 0


def test_every_count_on_every_frame():
    """The sweep above rotates the counts over the frames; here every frame of each kind takes every count."""
    for c in COUNTS:
        buf, frames = bgr_buffer(BGR_SHAPES, 500)
        count = torch.full((4,), c, dtype=torch.int32, device='cuda')
        changed = check_call(buf, frames, rows_for(BGR_SHAPES, 510), count, ws_poison=(0xA5,), sigma=2.5, margin=0.25)
        nbuf, nframes = nv12_buffer(NV12_SHAPES, 520)
        changed += check_call(nbuf, nframes, rows_for(NV12_SHAPES, 530), count[:3], ws_poison=(0xA5,), sigma=2.5, margin=0.25)
        assert (changed > 0) == (c > 0)


def _tiny_boxes(n, seed):
    det = torch.zeros(n, 3, 28, device='cuda')
    det[:, :, 4:12] = float('nan')
    rng = np.random.default_rng(seed)
    for b in range(n):
        x1, y1 = rng.integers(0, 5, 2)
        det[b, 0, :4] = torch.tensor([x1, y1, x1 + rng.integers(1, 4), y1 + rng.integers(1, 4)], dtype=torch.float32)
    return det, torch.ones(n, dtype=torch.int32, device='cuda')


def test_crosses_the_64_frame_split():
    det, count = _tiny_boxes(65, 601)
    buf, frames = bgr_buffer([(8, 8)] * 65, 600)
    assert check_call(buf, frames, det, count, sigma=1.0, margin=0.0) > 65
    nbuf, nframes = nv12_buffer([(8, 8, 8, 8)] * 65, 602)
    assert check_call(nbuf, nframes, det, count, sigma=1.0, margin=0.0) > 65


def test_workspace_cap_splits_the_call(monkeypatch):
    """With the cap below any table every frame is a call of its own (a frame larger than the cap still goes, alone); with room
    for exactly the first two the four frames go as 2 + 2: the bytes are those of one call."""
    from yolov6.hip import abi, runtime
    lib, calls = abi.load(), []

    class Spy:
        def __getattr__(self, name):
            if name == 'lp_redact_gauss_batch':
                return lambda desc, n, *a: calls.append(n) or lib.lp_redact_gauss_batch(desc, n, *a)
            return getattr(lib, name)
    monkeypatch.setattr(abi, 'load', lambda: Spy())
    det, count = rows_for(BGR_SHAPES, 650), torch.tensor([12, 12, 1, 12], dtype=torch.int32, device='cuda')
    for cap, want_calls in ((1, [1, 1, 1, 1]), (4 * 37 * 53 + 16 + 4 * 70 * 131 + 16, [2, 2]), (runtime.GAUSS_WS_CAP, [4])):
        monkeypatch.setattr(runtime.redact, 'GAUSS_WS_CAP', cap)
        calls.clear()
        buf, frames = bgr_buffer(BGR_SHAPES, 651)
        assert check_call(buf, frames, det, count, ws_poison=(0xA5,), sigma=2.5, margin=0.1) > 0
        assert calls == want_calls
    assert runtime.GAUSS_WS_CAP == 256 << 20


def test_redact_gauss_graph_capture():
    from yolov6.hip import runtime
    from yolov6.utils.redact import redact_plates_np
    buf, frames = bgr_buffer(BGR_SHAPES, 700)
    det = rows_for(BGR_SHAPES, 710)
    count = torch.tensor([12, 5, 3, 12], dtype=torch.int32, device='cuda')
    status = torch.empty(4, MAX_DET, dtype=torch.int32, device='cuda')
    kw = dict(mode='gauss', sigma=2.5, margin=0.25)
    runtime.redact_plates(frames, det, count, status=status, **kw)     # eager once: code loaded, workspace allocated
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                           # one stream, no parallel branches
        runtime.redact_plates(frames, det, count, status=status, **kw)
    for rep, counts in enumerate(([2, 12, 12, 0], [12, 0, 1, 7])):      # new pixels, rows and counts, same buffers, per replay
        rng = np.random.default_rng(720 + rep)
        start = torch.from_numpy(rng.integers(0, 256, buf.numel(), dtype=np.uint8)).cuda()
        buf.copy_(start)
        det.copy_(rows_for(BGR_SHAPES, 730 + rep))
        count.copy_(torch.tensor(counts, dtype=torch.int32))
        status.fill_(ST_POISON)
        want, want_st = redact_plates_np(host_frames(frames), det.cpu().numpy(), count.cpu().numpy(), **kw)
        want_buf = expect_buffer(buf, start, frames, want)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(status.cpu().numpy(), want_st)
        assert torch.equal(buf, want_buf) and not torch.equal(buf, start)


def test_argument_errors_leave_the_frames_alone():
    from yolov6.hip import abi, runtime
    lib = abi.load()
    buf, frames = bgr_buffer([(37, 53), (70, 131)], 800)
    nbuf, nframes = nv12_buffer(NV12_SHAPES[:2], 801)
    start, nstart = buf.clone(), nbuf.clone()
    det = rows_for([(37, 53), (70, 131)], 810)
    count = torch.tensor([12, 12], dtype=torch.int32, device='cuda')
    status = torch.full((2, MAX_DET), ST_POISON, dtype=torch.int32, device='cuda')
    ws = torch.empty(1 << 16, dtype=torch.uint8, device='cuda')
    assert ws.data_ptr() % 16 == 0
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def descs(nv12):
        d = (abi.RedactDesc * 2)()
        for e, f in zip(d, nframes if nv12 else frames):
            if nv12:
                e.p0, e.p1, e.pitch0, e.pitch1, e.format = f.y.data_ptr(), f.uv.data_ptr(), f.pitch_y, f.pitch_uv, 1
            else:
                e.p0, e.p1, e.pitch0, e.format = f.data_ptr(), None, 3 * f.shape[1], 0
            e.h0, e.w0 = f.shape[0], f.shape[1]
        return d

    def call(nv12=False, mods=(), par=(), taps=(), taps_c=(), **over):
        """The entry point on good arguments with some replaced: mods = ((frame, field, value), ...) on the descriptors, par =
        ((field, value), ...) on the parameters, taps / taps_c = ((k, value), ...), anything else by name."""
        d = descs(nv12)
        for b, field, value in mods:
            setattr(d[b], field, value)
        p = runtime._gauss_params(0.25, 2.5)
        for field, value in par:
            setattr(p, field, value)
        for k, value in taps:
            p.taps[k] = value
        for k, value in taps_c:
            p.taps_c[k] = value
        a = dict(desc=d, n=2, det=det.data_ptr(), count=count.data_ptr(), max_det=MAX_DET, p=ctypes.byref(p), status=status.data_ptr(),
                 ws=ws.data_ptr(), ws_bytes=ws.numel())
        a.update(over)
        return lib.lp_redact_gauss_batch(a['desc'], a['n'], a['det'], a['count'], a['max_det'], a['p'], a['status'], a['ws'],
                                         a['ws_bytes'], stream)

    good = runtime._gauss_params(0.25, 2.5)
    assert good.radius == 8 and good.radius_c == 4
    t, tc = list(good.taps), list(good.taps_c)
    need = lib.lp_redact_gauss_workspace_bytes(descs(False), 2, ctypes.byref(good))
    assert need == (37 * 53 + 3) // 4 * 16 + (70 * 131 + 3) // 4 * 16 and need <= ws.numel()       # each table at a 16-byte multiple
    bad_taps = runtime._gauss_params(0.25, 2.5)
    bad_taps.taps[0] += 2
    assert lib.lp_redact_gauss_workspace_bytes(descs(False), 2, ctypes.byref(bad_taps)) == 0
    uv1 = nframes[1].uv.data_ptr()
    bad = [dict(desc=None), dict(p=None), dict(status=None), dict(det=None), dict(count=None), dict(max_det=0), dict(n=-1),
           dict(mods=((1, 'format', 2),)), dict(mods=((1, 'p0', None),)), dict(mods=((1, 'p1', frames[0].data_ptr()),)),
           dict(mods=((1, 'pitch0', 3 * 131 - 1),)), dict(mods=((1, 'h0', 0),)), dict(mods=((0, 'w0', -5),)),
           dict(nv12=True, mods=((1, 'p1', None),)), dict(nv12=True, mods=((1, 'h0', 3),)), dict(nv12=True, mods=((0, 'pitch1', 61),)),
           dict(nv12=True, mods=((1, 'p1', uv1 + 1),)),
           dict(par=(('margin', -0.01),)), dict(par=(('margin', 4.5),)), dict(par=(('margin', float('nan')),)),
           dict(par=(('radius', 0),)), dict(par=(('radius', 49),)), dict(par=(('radius', -1),)),
           dict(par=(('radius', 7),)),                                             # the total no longer holds
           dict(taps=((0, t[0] + 2),)), dict(taps=((0, t[0] - 2),)),               # bad totals
           dict(taps=((8, t[7] + 1), (0, t[0] - 2 * (t[7] + 1 - t[8])))),          # the total holds, the last tap increases
           dict(nv12=True, par=(('radius_c', 0),)), dict(nv12=True, par=(('radius_c', 49),)),
           dict(nv12=True, taps_c=((0, tc[0] + 2),)),
           dict(nv12=True, taps_c=((4, tc[3] + 1), (0, tc[0] - 2 * (tc[3] + 1 - tc[4])))),
           dict(ws=None), dict(ws=ws.data_ptr() + 8), dict(ws_bytes=need - 1)]
    for kw in bad:
        rc = call(**kw)
        assert rc == L.LP_ERR_ARG, kw
        with pytest.raises(RuntimeError) as e:
            abi.check(rc, 'lp_redact_gauss_batch')
        if kw.get('mods'):
            assert 'frame %d' % kw['mods'][0][0] in str(e.value), (kw, str(e.value))
    torch.cuda.synchronize()
    assert torch.equal(buf, start) and torch.equal(nbuf, nstart) and bool((status == ST_POISON).all())
    # what is no error: no frames; chroma taps nobody reads (no NV12 frame); exactly the bytes asked for
    assert call(n=0) == 0 and call(n=0, det=None, count=None) == 0
    assert call(par=(('radius_c', 0),), taps_c=((0, 7),), ws_bytes=need) == 0
    torch.cuda.synchronize()
    assert not torch.equal(buf, start)
    # the public wrapper checks sigma before anything is enqueued
    buf.copy_(start)
    for sigma in (0.4, 16.5, float('nan')):
        with pytest.raises(ValueError):
            runtime.redact_plates(frames, det, count, mode='gauss', sigma=sigma)
    torch.cuda.synchronize()
    assert torch.equal(buf, start)


@pytest.mark.parametrize('nv12', [False, True], ids=['bgr', 'nv12'])
def test_lookback_redactor_equals_the_numpy_chain(nv12):
    """LookbackRedactor(mode='gauss') along the tracker's last_hold rows against the LookbackNp chain: the frames that leave the
    delay carry the specification's bytes, and the plate is blurred in the frames before its first detection."""
    from yolov6.hip import runtime
    from yolov6.utils.lookback import LookbackNp
    from yolov6.utils.nv12 import bgr_to_nv12_np
    from yolov6.utils.track import PlateTrackerNp
    bgr, rows, boxes = L.late_plate_frames()
    frames = [bgr_to_nv12_np(f, 'bt709') for f in bgr] if nv12 else bgr
    dev = _to_device(frames)
    det, count = C.frames_of(rows, 4)
    kw = dict(mode='gauss', sigma=2.5, margin=L.MARGIN)
    ref = PlateTrackerNp(2, max_tracks=4)
    trk = runtime.PlateTracker(2, max_tracks=4, device='cuda')
    ref.enable_hold(), trk.enable_hold()
    ref_lb, lb = LookbackNp(ref, L.DEPTH, **kw), runtime.LookbackRedactor(trk, L.DEPTH, **kw)
    got, want = [], []
    for lo, hi in [(0, 4)] + [(k, k + 1) for k in range(4, len(frames))]:
        so = [1] * (hi - lo) + ([-1] if lo == 0 else [])
        d = np.concatenate([det[lo:hi], np.zeros((len(so) - (hi - lo), 4, 28), np.float32)])
        c = np.concatenate([count[lo:hi], np.zeros(len(so) - (hi - lo), np.int32)])
        ref.update(d, c, so)
        want += ref_lb.push(frames[lo:hi], so)
        trk.update(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda(), so)
        got += lb.push(dev[lo:hi], so)
    ref.flush_all(), trk.flush_all()
    want += ref_lb.flush_all()
    got += lb.flush_all()
    torch.cuda.synchronize()
    assert [(s, g) for s, g, _ in got] == [(1, k) for k in range(len(frames))] and all(a is b for (_, _, a), b in zip(got, dev))
    _assert_frames_equal(got, want)
    src = [f.y if nv12 else f for f in frames]
    out = [(f.y if nv12 else f).cpu().numpy() for _, _, f in got]
    assert any((out[k] != src[k]).any() for k in range(L.LATE))          # an early frame's plate is covered


def test_infer_redact_gauss_batch_size_1_and_4(tmp_path, monkeypatch):
    """Inferer(redact='gauss') on a GPU, one frame at a time and four, BGR and NV12: the files the specification writes for the rows
    returned (the GPU's own rows, as in tests/test_redact_gpu.py)."""
    from PIL import Image
    from yolov6.utils.nv12 import bgr_to_nv12_np, nv12_to_bgr_np
    from yolov6.utils.redact import redact_plates_np
    from yolov6.utils.synth import build_synthetic
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    ckpt = tmp_path / 'tiny.pt'
    torch.save({'model': build_synthetic(CFG('yololps'), width=0.0625, sigma=1.5).half(), 'ema': None}, str(ckpt))
    img_dir = tmp_path / 'imgs'
    img_dir.mkdir()
    rng = np.random.default_rng(12)
    shapes = [(232, 144), (232, 144), (150, 250), (150, 250), (100, 60)]
    frames = []
    for i, (h, w) in enumerate(shapes):
        frames.append(rng.integers(0, 255, (h, w, 3), dtype=np.uint8))
        Image.fromarray(frames[-1]).save(str(img_dir / ('f%d.png' % i)))
    kw = dict(weights=str(ckpt), source=str(img_dir), yaml=None, img_size=[128, 128], conf_thres=0.06, iou_thres=0.45,
              max_det=20, device='0', not_save_img=True, redact='gauss', redact_sigma=2.5, redact_margin=0.25)
    runs = dict(o1=dict(), o4=dict(batch_size=4), n4=dict(batch_size=4, nv12='bt709'))
    dets = {tag: infer.run(save_dir=str(tmp_path / tag), **kw, **extra) for tag, extra in runs.items()}
    assert sum(len(d) for d in dets['o1']) > 0
    changed = 0
    for i, f in enumerate(frames):
        assert torch.equal(dets['o1'][i], dets['o4'][i])
        name = 'f%d.png' % i
        assert (tmp_path / 'o1' / 'redacted' / name).read_bytes() == (tmp_path / 'o4' / 'redacted' / name).read_bytes()
        for tag in ('o1', 'n4'):
            d = dets[tag][i].cpu().numpy()
            det = np.zeros((1, max(len(d), 1), 28), np.float32)
            det[0, :len(d)] = d
            src = np.ascontiguousarray(f[:, :, ::-1])
            if tag == 'n4':
                (want,), _ = redact_plates_np([bgr_to_nv12_np(src, 'bt709')], det, [len(d)], 'gauss', margin=0.25, sigma=2.5)
                want = nv12_to_bgr_np(want)
            else:
                (want,), _ = redact_plates_np([src], det, [len(d)], 'gauss', margin=0.25, sigma=2.5)
                changed += int((want != src).sum())
            got = np.asarray(Image.open(str(tmp_path / tag / 'redacted' / name)))
            assert np.array_equal(got, want[:, :, ::-1])
    assert changed > 0
