"""Plate redaction on the GPU: lp_redact_plates_batch (runtime.redact_plates) bit for bit against the numpy specification
(yolov6/utils/redact.py): a sweep over shapes, cells, margins, modes and counts with guard and padding bytes, poisoned status and
workspace; the 64-frame split; graph capture; every argument error; behind detect_frames_padded and PlateTracker.update on the
tiny golden model, with plate crops taken first; and Inferer(redact=...) at batch sizes 1 and 4."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden
from test_redact_cpu import quad_rows

pytestmark = pytest.mark.gpu

CFG = lambda n: os.path.join(REPO, 'configs', n + '.py')   # noqa: E731
ST_POISON = -7
MAX_DET = 12
COUNTS = [-1, 0, 5, 12, MAX_DET + 3]
BGR_SHAPES = [(37, 53), (64, 96), (1, 1), (5, 200)]
NV12_SHAPES = [(38, 54, 70, 60), (2, 2, 5, 6)]        # h, w, pitch_y, pitch_uv


def bgr_buffer(shapes, seed):
    """(buf, frames): one seeded uint8 CUDA buffer and contiguous [h,w,3] views of it at odd byte addresses, guard bytes either
    side of every frame."""
    rng = np.random.default_rng(seed)
    offs, n = [], 7
    for h, w in shapes:
        offs.append(n)
        n = (n + h * w * 3 + 5) | 1
    buf = torch.from_numpy(rng.integers(0, 256, n + 8, dtype=np.uint8)).cuda()
    frames = [buf[o:o + h * w * 3].view(h, w, 3) for o, (h, w) in zip(offs, shapes)]
    assert all(f.data_ptr() % 2 == 1 for f in frames)
    return buf, frames


def nv12_buffer(shapes, seed, matrix='bt709'):
    """(buf, frames): one seeded buffer and ``Nv12Frame``s whose planes are pitched views of it (the padding and the guards hold
    seeded bytes too)."""
    from yolov6.utils.nv12 import Nv12Frame
    rng = np.random.default_rng(seed)
    spans, n = [], 6
    for h, w, py, puv in shapes:
        oy = n
        ouv = (oy + h * py + 3) // 2 * 2
        n = ouv + (h // 2) * puv + 4
        spans.append((oy, ouv))
    buf = torch.from_numpy(rng.integers(0, 256, n, dtype=np.uint8)).cuda()
    assert buf.data_ptr() % 2 == 0
    frames = []
    for (h, w, py, puv), (oy, ouv) in zip(shapes, spans):
        y = buf[oy:oy + h * py].view(h, py)[:, :w]
        uv = buf[ouv:ouv + (h // 2) * puv].view(h // 2, puv // 2, 2)[:, :w // 2]
        frames.append(Nv12Frame(y, uv, matrix))
        assert frames[-1].pitch_y == py and frames[-1].pitch_uv == puv
    return buf, frames


def host_frames(frames):
    """Host copies of device frames, for the specification."""
    from yolov6.utils.nv12 import Nv12Frame
    return [Nv12Frame(f.y.cpu().numpy(), f.uv.cpu().numpy(), f.matrix) if isinstance(f, Nv12Frame) else f.cpu().numpy()
            for f in frames]


def expect_buffer(buf, start, frames, want):
    """The whole buffer as it must be afterwards: ``want`` (the specification's frames) in the places of ``frames`` (views of
    ``buf``), every other byte (guards, pitch padding) as in ``start``, the buffer's bytes before the call."""
    from yolov6.utils.nv12 import Nv12Frame
    out = start.clone()
    base = buf.data_ptr()
    for f, w in zip(frames, want):
        if isinstance(f, Nv12Frame):
            oy, ouv = f.y.data_ptr() - base, f.uv.data_ptr() - base
            out[oy:oy + (f.h - 1) * f.pitch_y + f.w].as_strided((f.h, f.w), (f.pitch_y, 1)).copy_(torch.from_numpy(w.y))
            out[ouv:ouv + (f.h // 2 - 1) * f.pitch_uv + f.w].as_strided((f.h // 2, f.w // 2, 2), (f.pitch_uv, 2, 1)).copy_(
                torch.from_numpy(np.ascontiguousarray(w.uv)))
        else:
            o = f.data_ptr() - base
            out[o:o + f.numel()].copy_(torch.from_numpy(w.reshape(-1)))
    return out


def rows_for(shapes, seed):
    return torch.from_numpy(np.stack([quad_rows(s[0], s[1], MAX_DET, seed + b) for b, s in enumerate(shapes)])).cuda()


def check_call(buf, frames, det, count, ws_poison=(0xA5, 0x00), **kw):
    """redact_plates on ``frames`` (views of ``buf``) with the workspace and the status poisoned, once per workspace poison from
    the same start: every byte of the buffer and every status must be the specification's.  Returns the number of changed bytes."""
    from yolov6.hip import runtime
    from yolov6.utils.redact import redact_plates_np
    start = buf.clone()
    want, want_st = redact_plates_np(host_frames(frames), det.cpu().numpy(), count.cpu().numpy(), **kw)
    want_buf = expect_buffer(buf, start, frames, want)
    for poison in ws_poison:
        buf.copy_(start)
        runtime._redact_workspace(buf.device, 1 << 20).fill_(poison)
        status = torch.full((len(frames), det.shape[1]), ST_POISON, dtype=torch.int32, device='cuda')
        got_st = runtime.redact_plates(frames, det, count, status=status, **kw)
        torch.cuda.synchronize()
        assert got_st.data_ptr() == status.data_ptr()
        assert np.array_equal(status.cpu().numpy(), want_st)
        assert torch.equal(buf, want_buf)                           # the frames, and every guard and padding byte
    changed = int((want_buf != start).sum())
    buf.copy_(start)
    return changed


CASES = [(cell, margin, mode) for cell in (2, 8, 64) for margin in (0.0, 0.25) for mode in ('mosaic', 'fill')]


@pytest.mark.parametrize('k', range(len(CASES)), ids=['cell%d-m%g-%s' % c for c in CASES])
def test_kernels_equal_specification(k):
    cell, margin, mode = CASES[k]
    kw = dict(mode=mode, cell=cell, margin=margin, fill=(17, 130, 240))
    buf, frames = bgr_buffer(BGR_SHAPES, 100 + k)
    count = torch.tensor([COUNTS[(b + k) % 5] for b in range(4)], dtype=torch.int32, device='cuda')
    changed = check_call(buf, frames, rows_for(BGR_SHAPES, 200 + 10 * k), count, **kw)
    nbuf, nframes = nv12_buffer(NV12_SHAPES, 300 + k)
    ncount = torch.tensor([COUNTS[(b + k + 2) % 5] for b in range(2)], dtype=torch.int32, device='cuda')
    changed += check_call(nbuf, nframes, rows_for(NV12_SHAPES, 400 + 10 * k), ncount, **kw)
    assert changed > 0


def test_every_count_on_every_frame():
    """The sweep above rotates the counts over the frames; here the two largest frames of each kind take every count."""
    for c in COUNTS:
        buf, frames = bgr_buffer(BGR_SHAPES[:2], 500)
        count = torch.tensor([c, c], dtype=torch.int32, device='cuda')
        changed = check_call(buf, frames, rows_for(BGR_SHAPES[:2], 510), count, ws_poison=(0xA5,), mode='mosaic', cell=8, margin=0.25)
        nbuf, nframes = nv12_buffer(NV12_SHAPES[:1], 520)
        changed += check_call(nbuf, nframes, rows_for(NV12_SHAPES[:1], 530), count[:1], ws_poison=(0xA5,), mode='mosaic', cell=8,
                              margin=0.25)
        assert (changed > 0) == (c > 0)


def test_fill_of_nv12_frames_with_two_matrices():
    """A fill is given as BGR and written in the frame's own format: two matrices in one list are two runs of the entry point."""
    nbuf, nframes = nv12_buffer([(38, 54, 70, 60), (38, 54, 54, 54), (2, 2, 5, 6)], 540)
    nframes[1].matrix = 'bt601f'
    count = torch.tensor([12, 12, 1], dtype=torch.int32, device='cuda')
    assert check_call(nbuf, nframes, rows_for([(38, 54)] * 2 + [(2, 2)], 550), count, mode='fill', fill=(250, 20, 60)) > 0


def test_crosses_the_64_frame_split():
    shapes = [(8, 8)] * 65
    buf, frames = bgr_buffer(shapes, 600)
    det = torch.zeros(65, 3, 28, device='cuda')
    det[:, :, 4:12] = float('nan')
    rng = np.random.default_rng(601)
    for b in range(65):
        x1, y1 = rng.integers(0, 5, 2)
        det[b, 0, :4] = torch.tensor([x1, y1, x1 + rng.integers(1, 4), y1 + rng.integers(1, 4)], dtype=torch.float32)
    count = torch.ones(65, dtype=torch.int32, device='cuda')
    assert check_call(buf, frames, det, count, mode='mosaic', cell=4, margin=0.0) > 65
    nbuf, nframes = nv12_buffer([(8, 8, 8, 8)] * 65, 602)
    assert check_call(nbuf, nframes, det, count, mode='mosaic', cell=4, margin=0.0) > 65


def test_redact_plates_graph_capture():
    from yolov6.hip import runtime
    from yolov6.utils.redact import redact_plates_np
    buf, frames = bgr_buffer(BGR_SHAPES, 700)
    det = rows_for(BGR_SHAPES, 710)
    count = torch.tensor([12, 5, 3, 12], dtype=torch.int32, device='cuda')
    status = torch.empty(4, MAX_DET, dtype=torch.int32, device='cuda')
    start = buf.clone()
    kw = dict(mode='mosaic', cell=8, margin=0.25)
    runtime.redact_plates(frames, det, count, status=status, **kw)     # eager once: code loaded, workspace allocated
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                           # one stream, no parallel branches
        runtime.redact_plates(frames, det, count, status=status, **kw)
    rng = np.random.default_rng(720)
    start = torch.from_numpy(rng.integers(0, 256, buf.numel(), dtype=np.uint8)).cuda()     # new pixels, rows and counts, same buffers
    buf.copy_(start)
    det.copy_(rows_for(BGR_SHAPES, 730))
    count.copy_(torch.tensor([2, 12, 12, 0], dtype=torch.int32))
    status.fill_(ST_POISON)
    want, want_st = redact_plates_np(host_frames(frames), det.cpu().numpy(), count.cpu().numpy(), **kw)
    want_buf = expect_buffer(buf, start, frames, want)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(status.cpu().numpy(), want_st)
    assert torch.equal(buf, want_buf) and not torch.equal(buf, start)


def test_argument_errors_leave_the_frames_alone():
    from yolov6.hip import abi
    lib = abi.load()
    buf, frames = bgr_buffer([(37, 53), (64, 96)], 800)
    nbuf, nframes = nv12_buffer(NV12_SHAPES, 801)
    start, nstart = buf.clone(), nbuf.clone()
    det = rows_for([(37, 53), (64, 96)], 810)
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

    def call(nv12=False, mods=(), par=(), **over):
        """The entry point on good arguments with some replaced: mods = ((frame, field, value), ...) on the descriptors, par =
        ((field, value), ...) on the parameters, anything else by name."""
        d = descs(nv12)
        for b, field, value in mods:
            setattr(d[b], field, value)
        p = abi.RedactParams(0, 8, 0.25, (ctypes.c_ubyte * 3)(1, 2, 3))
        for field, value in par:
            setattr(p, field, value)
        a = dict(desc=d, n=2, det=det.data_ptr(), count=count.data_ptr(), max_det=MAX_DET, p=ctypes.byref(p), status=status.data_ptr(),
                 ws=ws.data_ptr(), ws_bytes=ws.numel())
        a.update(over)
        return lib.lp_redact_plates_batch(a['desc'], a['n'], a['det'], a['count'], a['max_det'], a['p'], a['status'], a['ws'],
                                          a['ws_bytes'], stream)

    need = lib.lp_redact_workspace_bytes(descs(False), 2, ctypes.byref(abi.RedactParams(0, 8, 0.25, (ctypes.c_ubyte * 3)())))
    assert need == (5 * 7 + 1) * 4 + 8 * 12 * 4         # 35 entries rounded up to a 16-byte multiple, then 96
    assert lib.lp_redact_workspace_bytes(descs(False), 2, ctypes.byref(abi.RedactParams(1, 8, 0.25, (ctypes.c_ubyte * 3)()))) == 0
    uv1 = nframes[1].uv.data_ptr()
    bad = [dict(desc=None), dict(p=None), dict(status=None), dict(det=None), dict(count=None), dict(max_det=0), dict(n=-1),
           dict(mods=((1, 'format', 2),)), dict(mods=((1, 'format', -1),)), dict(mods=((1, 'p0', None),)),
           dict(mods=((1, 'p1', frames[0].data_ptr()),)), dict(mods=((1, 'pitch0', 3 * 96 - 1),)), dict(mods=((1, 'h0', 0),)),
           dict(mods=((1, 'w0', 0),)), dict(mods=((0, 'w0', -5),)),
           dict(nv12=True, mods=((1, 'p1', None),)), dict(nv12=True, mods=((1, 'p0', None),)), dict(nv12=True, mods=((1, 'h0', 3),)),
           dict(nv12=True, mods=((1, 'w0', 1),)), dict(nv12=True, mods=((1, 'h0', 0),)), dict(nv12=True, mods=((1, 'pitch0', 1),)),
           dict(nv12=True, mods=((1, 'pitch1', 1),)), dict(nv12=True, mods=((0, 'pitch1', 61),)),
           dict(nv12=True, mods=((1, 'p1', uv1 + 1),)),
           dict(par=(('mode', 2),)), dict(par=(('mode', -1),)), dict(par=(('cell', 7),)), dict(par=(('cell', 0),)),
           dict(par=(('cell', 66),)), dict(par=(('margin', -0.01),)), dict(par=(('margin', 4.5),)), dict(par=(('margin', float('nan')),)),
           dict(ws=None), dict(ws=ws.data_ptr() + 8), dict(ws_bytes=need - 1)]
    for kw in bad:
        rc = call(**kw)
        assert rc < 0, kw
        with pytest.raises(RuntimeError) as e:
            abi.check(rc, 'lp_redact_plates_batch')
        if kw.get('mods'):
            assert 'frame %d' % kw['mods'][0][0] in str(e.value), (kw, str(e.value))
    torch.cuda.synchronize()
    assert torch.equal(buf, start) and torch.equal(nbuf, nstart) and bool((status == ST_POISON).all())
    # what is no error: no frames; a fill without a workspace and with any cell; exactly the bytes asked for
    assert call(n=0) == 0 and call(n=0, det=None, count=None) == 0
    assert call(par=(('mode', 1), ('cell', 7)), ws=None, ws_bytes=0) == 0
    assert call(ws_bytes=need) == 0
    torch.cuda.synchronize()
    assert not torch.equal(buf, start)


def _tiny_golden_model():
    from yolov6.utils.synth import build_synthetic
    m = build_synthetic(CFG('yololps'), width=0.0625, sigma=1.5)
    m.load_state_dict(load_golden('lps_tiny_weights'))
    return m.eval().cuda()


def test_behind_the_detector_and_the_tracker():
    from yolov6.hip import runtime
    from yolov6.utils.plate_crop import plate_crops_np
    from yolov6.utils.redact import redact_plates_np
    m = _tiny_golden_model()
    rng = np.random.default_rng(900)
    host = [rng.integers(0, 256, (120, 96, 3), dtype=np.uint8) for _ in range(3)]
    kw = dict(mode='mosaic', cell=8, margin=0.1)
    with torch.no_grad():
        frames = [torch.from_numpy(f).cuda() for f in host]
        det, count = runtime.detect_frames_padded(m, frames, [128, 128], 0.06, 0.45, 20)
        crops, crop_st = runtime.plate_crops(frames, det, count, (16, 48), max_crops=20)       # reads the frames first
        status = runtime.redact_plates(frames, det, count, **kw)
        torch.cuda.synchronize()
        det_h, count_h = det.cpu().numpy(), count.cpu().numpy()
        assert count_h.min() > 0
        want, want_st = redact_plates_np(host, det_h, count_h, **kw)
        assert np.array_equal(status.cpu().numpy(), want_st)
        for f, w, h in zip(frames, want, host):
            assert np.array_equal(f.cpu().numpy(), w) and (w != h).any()
        for b in range(3):                                           # the crops are of the frames as they were
            n = int(count_h[b])
            ref, ref_st = plate_crops_np(host[b], det_h[b, :n], (16, 48))
            assert np.array_equal(crops[b, :n].cpu().numpy(), ref) and np.array_equal(crop_st[b, :n].cpu().numpy(), ref_st)

        # the tracker's voted rows carry the same geometry: det_out goes in as it is
        frames = [torch.from_numpy(f).cuda() for f in host]
        tracker = runtime.PlateTracker(3, device=frames[0].device)
        det_out = tracker.update(det, count)[0]
        status = runtime.redact_plates(frames, det_out, count, **kw)
        torch.cuda.synchronize()
        want_t, want_st_t = redact_plates_np(host, det_out.cpu().numpy(), count_h, **kw)
        assert np.array_equal(status.cpu().numpy(), want_st_t)
        for f, w, w0 in zip(frames, want_t, want):
            assert np.array_equal(f.cpu().numpy(), w) and np.array_equal(w, w0)


def test_infer_redact_batch_size_1_and_4(tmp_path, monkeypatch):
    """Inferer(redact='mosaic') on a GPU, one frame at a time and four: the same files, and the files the CPU path of the
    redaction (redact_plates_np) writes for the rows returned.  (The detections of the CPU model itself may differ from the
    GPU's by a pixel at a rounding boundary, tests/test_hip_model.py::test_infer_entry_point_on_gpu, so the rows are the GPU's.)"""
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
    shapes = [(232, 144), (232, 144), (232, 144), (150, 250), (150, 250), (232, 144), (100, 60)]
    frames = []
    for i, (h, w) in enumerate(shapes):
        frames.append(rng.integers(0, 255, (h, w, 3), dtype=np.uint8))
        Image.fromarray(frames[-1]).save(str(img_dir / ('f%d.png' % i)))
    kw = dict(weights=str(ckpt), source=str(img_dir), yaml=None, img_size=[128, 128], conf_thres=0.06, iou_thres=0.45,
              max_det=20, device='0', not_save_img=True, redact='mosaic', redact_cell=8, redact_margin=0.25)
    plain = infer.run(save_dir=str(tmp_path / 'plain'), **dict(kw, redact=None))
    assert not (tmp_path / 'plain' / 'redacted').exists()
    runs = dict(o1=dict(), o4=dict(batch_size=4), n4=dict(batch_size=4, nv12='bt709'), c4=dict(batch_size=4, save_crops=True, crop_size=(16, 48)))
    dets = {tag: infer.run(save_dir=str(tmp_path / tag), **kw, **extra) for tag, extra in runs.items()}
    assert sum(len(d) for d in dets['o1']) > 0
    for i, f in enumerate(frames):
        assert torch.equal(dets['o1'][i], plain[i]) and torch.equal(dets['o1'][i], dets['o4'][i]) and torch.equal(dets['o1'][i], dets['c4'][i])
        name = 'f%d.png' % i
        assert (tmp_path / 'o1' / 'redacted' / name).read_bytes() == (tmp_path / 'o4' / 'redacted' / name).read_bytes()
        assert (tmp_path / 'o1' / 'redacted' / name).read_bytes() == (tmp_path / 'c4' / 'redacted' / name).read_bytes()
        for tag in ('o1', 'n4'):
            d = dets[tag][i].cpu().numpy()
            det = np.zeros((1, max(len(d), 1), 28), np.float32)
            det[0, :len(d)] = d
            src = np.ascontiguousarray(f[:, :, ::-1])
            if tag == 'n4':
                (want,), _ = redact_plates_np([bgr_to_nv12_np(src, 'bt709')], det, [len(d)], 'mosaic', 8, 0.25)
                want = nv12_to_bgr_np(want)
            else:
                (want,), _ = redact_plates_np([src], det, [len(d)], 'mosaic', 8, 0.25)
            got = np.asarray(Image.open(str(tmp_path / tag / 'redacted' / name)))
            assert np.array_equal(got, want[:, :, ::-1])
    # the crops written next to the redacted frames were cut before the redaction
    from yolov6.utils.plate_crop import plate_crops_np
    d0 = dets['c4'][0].cpu().numpy()
    ref, _ = plate_crops_np(np.ascontiguousarray(frames[0][:, :, ::-1]), d0, (16, 48))
    for k in range(len(d0)):
        got = np.asarray(Image.open(str(tmp_path / 'c4' / 'imgs' / 'crops' / ('f0_%d.png' % k))))
        assert np.array_equal(got, ref[k][:, :, ::-1])
