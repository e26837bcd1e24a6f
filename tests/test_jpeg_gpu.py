"""Baseline JPEG on the GPU: lp_jpeg_encode_batch (runtime.encode_jpeg) byte for byte against the numpy specification
(yolov6/utils/jpeg.py): the constructed set of tests/test_jpeg_cpu.py, sizes around one MCU, the restart intervals and the scan
block, every kind of source, containment inside guard bytes with a capacity one byte short, every refusal, and Inferer(save_jpeg=Q)."""
import ctypes
import importlib
import io
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from test_jpeg_cpu import constructed_set, synthetic

pytestmark = pytest.mark.gpu

CFG = lambda n: os.path.join(REPO, 'configs', n + '.py')   # noqa: E731
GUARD = 4096
LP_ERR_ARG = -1


def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _check(frames_np, quality, restart, frames_dev=None, **kw):
    """runtime.encode_jpeg of the frames == encode_jpeg_np of each, byte for byte."""
    from yolov6.hip import runtime
    from yolov6.utils.jpeg import encode_jpeg_np
    dev = [torch.from_numpy(f).cuda() for f in frames_np] if frames_dev is None else frames_dev
    got = runtime.encode_jpeg(dev, quality, restart, **kw)
    assert len(got) == len(frames_np)
    for k, (g, f) in enumerate(zip(got, frames_np)):
        want = encode_jpeg_np(f, quality, restart)
        assert len(g) == len(want), 'frame %d: %d bytes, the specification has %d' % (k, len(g), len(want))
        assert g == want, 'frame %d differs first at byte %d' % (k, next(i for i in range(len(want)) if g[i] != want[i]))
    return got


def test_constructed_set():
    """The shared set (every DC category, AC size, ZRL count, no EOB, stuffing, every pad length, RSTm wrapping)."""
    for name, img, q, restart in constructed_set():
        _check([img], q, restart)
    by_params = {}
    for name, img, q, restart in constructed_set():      # and those that share quality and restart as one batch
        by_params.setdefault((q, restart), []).append(img)
    for (q, restart), imgs in by_params.items():
        if len(imgs) > 1:
            _check(imgs, q, restart)


@pytest.mark.parametrize('h,w,restart', [(1, 1, 16), (2, 2, 16), (16, 16, 16), (17, 15, 16), (50, 34, 16), (48, 32, 1), (48, 32, 4),
                                         (48, 32, 5), (48, 32, 16), (48, 48, 1), (16, 4112, 1), (16, 4096, 1), (16, 4080, 1)])
def test_sizes_and_restart_intervals(h, w, restart):
    """One MCU and less, sizes that are no multiple of 16, intervals that straddle MCU rows (5) or exceed the image (16), RSTm
    wrapping (9 intervals), and 257 / 256 / 255 intervals around the scan kernel's block of 256."""
    from PIL import Image
    got = _check([_noise(h, w, h * 7 + w)], 85, restart)
    im = Image.open(io.BytesIO(got[0]))
    im.load()
    assert im.size == (w, h)


def test_restart_32_of_quality_100_noise():
    """The longest interval the kernel takes, of the densest data: the LDS bit buffer at its fullest."""
    _check([_noise(64, 128, 5)], 100, 32)
    hard = np.where(np.indices((32, 256)).sum(0)[..., None] & 1, 255, 0).astype(np.uint8).repeat(3, axis=2)      # a pixel checkerboard
    _check([hard], 100, 32)


def test_mixed_sizes_pitched_views_and_crop_tensors():
    from yolov6.hip import runtime
    from yolov6.utils.jpeg import encode_jpeg_np
    shapes = [(40, 56), (1, 7), (33, 17), (16, 16), (80, 24)] * 7          # 35 frames: two launches of 32
    frames = [_noise(h, w, k) for k, (h, w) in enumerate(shapes)]
    _check(frames, 90, 16)
    big = torch.from_numpy(_noise(70, 90, 99)).cuda()
    views = [big[3:45, 5:60], big[10:11, 0:90], big[0:70, 89:90]]
    assert not views[0].is_contiguous()
    _check([v.cpu().numpy() for v in views], 75, 3, frames_dev=views)
    crops = torch.from_numpy(np.stack([_noise(64, 192, 200 + k) for k in range(3)])).cuda()
    got = runtime.encode_jpeg([crops], 90)
    assert got == [encode_jpeg_np(c, 90, 16) for c in crops.cpu().numpy()]
    assert runtime.encode_jpeg(crops[1], 90) == got[1:2]


def test_runs_under_the_workspace_cap(monkeypatch):
    """encode_jpeg_padded sends the frames in runs whose workspace stays under JPEG_WS_CAP: with a cap of two 32 x 32 frames the
    eleven frames go in nine calls (a frame larger than the cap alone in one), and the files are the same."""
    from yolov6.hip import abi, runtime
    frames = [_noise(32, 32, k) for k in range(5)] + [_noise(80, 96, 9)] + [_noise(17, 40, 20 + k) for k in range(5)]
    want = _check(frames, 80, 4)
    lib, calls = abi.load(), []

    class Counting:
        def __getattr__(self, name):
            if name == 'lp_jpeg_encode_batch':
                return lambda desc, n, *a: (calls.append(n), lib.lp_jpeg_encode_batch(desc, n, *a))[1]
            return getattr(lib, name)
    monkeypatch.setattr(runtime.jpeg, 'JPEG_WS_CAP', 2 * (4 * 776 + 16))
    monkeypatch.setattr(abi, 'load', lambda: Counting())
    assert runtime.encode_jpeg([torch.from_numpy(f).cuda() for f in frames], 80, 4) == want
    assert calls == [2, 2, 1, 1, 1, 1, 1, 1, 1]


def _nv12_dev(h, w, pitch_y, pitch_uv, matrix, seed):
    """(device Nv12Frame with pitched planes inside one buffer, host Nv12Frame of the same bytes)."""
    from yolov6.utils.nv12 import Nv12Frame
    rng = np.random.default_rng(seed)
    yb = rng.integers(0, 256, (h, pitch_y), dtype=np.uint8)
    ub = rng.integers(0, 256, (h // 2, pitch_uv), dtype=np.uint8)
    ty, tu = torch.from_numpy(yb).cuda(), torch.from_numpy(ub).cuda()
    dev = Nv12Frame(ty[:, :w], tu[:, :w].unflatten(1, (w // 2, 2)), matrix)
    host = Nv12Frame(yb[:, :w], ub[:, :w].reshape(h // 2, w // 2, 2), matrix)
    return dev, host


def test_nv12_sources():
    """bt601f planes with pitches above the width feed the transform as they are; bt709 goes through nv12_to_bgr."""
    from yolov6.hip import runtime
    from yolov6.utils.jpeg import encode_jpeg_np
    from yolov6.utils.nv12 import nv12_to_bgr_np
    pairs = [_nv12_dev(38, 54, 70, 60, 'bt601f', 1), _nv12_dev(2, 2, 5, 6, 'bt601f', 2), _nv12_dev(32, 48, 48, 48, 'bt601f', 3)]
    assert pairs[0][0].pitch_y == 70 and pairs[0][0].pitch_uv == 60
    got = runtime.encode_jpeg([d for d, _ in pairs], 90, 4)
    assert got == [encode_jpeg_np(h, 90, 4) for _, h in pairs]
    pairs = [_nv12_dev(38, 54, 70, 60, 'bt709', 4), _nv12_dev(18, 22, 22, 22, 'bt601f', 5), _nv12_dev(6, 4, 4, 4, 'bt601', 6)]
    got = runtime.encode_jpeg([d for d, _ in pairs], 80, 16)
    assert got == [encode_jpeg_np(h, 80, 16) for _, h in pairs]
    assert got[0] == encode_jpeg_np(nv12_to_bgr_np(pairs[0][1]), 80, 16)


def _raw_call(frames, quality, restart, cap, matrix=0, ws_bytes=None):
    """lp_jpeg_encode_batch on BGR device frames with out, nbytes and the workspace inside guard bytes: (rc, out, nbytes, guards ok)."""
    from yolov6.hip import abi
    from yolov6.utils.jpeg import jpeg_header
    lib = abi.load()
    n = len(frames)
    desc = (abi.JpegDesc * n)()
    for d, f in zip(desc, frames):
        d.p0, d.p1, d.pitch0, d.pitch1, d.h0, d.w0, d.format, d.matrix = f.data_ptr(), None, f.stride(0), 0, f.shape[0], f.shape[1], 0, matrix
    need = lib.lp_jpeg_workspace_bytes(desc, n, restart)
    heads = np.stack([np.frombuffer(jpeg_header(f.shape[0], f.shape[1], min(max(quality, 1), 100), min(max(restart, 1), 32)), np.uint8)
                      for f in frames])
    hd = torch.from_numpy(heads).cuda()
    fill = 0xA5
    ob = torch.full((GUARD + n * cap + GUARD,), fill, dtype=torch.uint8, device='cuda')
    nb = torch.full((64 + n + 64,), -123456, dtype=torch.int32, device='cuda')
    ws_n = (need if ws_bytes is None else ws_bytes)
    wb = torch.full((GUARD + ws_n + 256 + GUARD,), fill, dtype=torch.uint8, device='cuda')
    ws_ptr = (wb.data_ptr() + GUARD + 255) // 256 * 256
    params = abi.JpegParams(quality, restart)
    rc = lib.lp_jpeg_encode_batch(desc, n, ctypes.byref(params), ctypes.c_void_p(hd.data_ptr()), heads.shape[1],
                                  ctypes.c_void_p(ob.data_ptr() + GUARD), cap, ctypes.c_void_p(nb.data_ptr() + 64 * 4),
                                  ctypes.c_void_p(ws_ptr), ws_n, None)
    torch.cuda.synchronize()
    ob_h, nb_h, wb_h = ob.cpu().numpy(), nb.cpu().numpy(), wb.cpu().numpy()
    off = ws_ptr - wb.data_ptr()
    guards = bool((ob_h[:GUARD] == fill).all() and (ob_h[GUARD + n * cap:] == fill).all() and (nb_h[:64] == -123456).all()
                  and (nb_h[64 + n:] == -123456).all() and (wb_h[:off] == fill).all() and (wb_h[off + ws_n:] == fill).all())
    untouched = bool((ob_h == fill).all() and (nb_h == -123456).all() and (wb_h == fill).all())
    return rc, ob_h[GUARD:GUARD + n * cap].reshape(n, cap), nb_h[64:64 + n], guards, untouched


def test_containment_and_a_capacity_one_byte_short():
    from yolov6.hip import runtime
    from yolov6.utils.jpeg import encode_jpeg_np
    frames_np = [_noise(40, 56, 1), _noise(48, 64, 2), _noise(24, 24, 3)]
    want = [encode_jpeg_np(f, 95, 2) for f in frames_np]
    frames = [torch.from_numpy(f).cuda() for f in frames_np]
    cap = max(len(w) for w in want)
    rc, out, nbytes, guards, _ = _raw_call(frames, 95, 2, cap)              # the largest file fits exactly
    assert rc == 0 and guards
    assert nbytes.tolist() == [len(w) for w in want]
    for k, w in enumerate(want):
        assert out[k, :len(w)].tobytes() == w and (out[k, len(w):] == 0xA5).all()
    rc, out, nbytes, guards, _ = _raw_call(frames, 95, 2, cap - 1)          # ... and is one byte short
    assert rc == 0 and guards
    big = int(np.argmax([len(w) for w in want]))
    assert nbytes[big] == -len(want[big]) and (out[big] == 0xA5).all()
    for k, w in enumerate(want):
        if k != big:
            assert nbytes[k] == len(w) and out[k, :len(w)].tobytes() == w and (out[k, len(w):] == 0xA5).all()
    before = runtime.jpeg_stats['retries']
    assert runtime.encode_jpeg(frames, 95, 2, cap=cap - 1) == want
    assert runtime.jpeg_stats['retries'] == before + 1
    out_d, nb_d = runtime.encode_jpeg_padded(frames, 95, 2)
    assert nb_d.dtype == torch.int32 and nb_d.is_cuda and out_d.is_cuda and nb_d.cpu().tolist() == [len(w) for w in want]


def test_refusals_write_nothing():
    from yolov6.hip import abi, runtime
    lib = abi.load()
    frames = [torch.from_numpy(_noise(20, 20, 1)).cuda()]
    for kw, word in ((dict(quality=90, restart=33), 'restart'), (dict(quality=0, restart=16), 'quality'),
                     (dict(quality=101, restart=16), 'quality'), (dict(quality=90, restart=0), 'restart')):
        rc, _, _, _, untouched = _raw_call(frames, cap=4096, **kw)
        assert rc == LP_ERR_ARG and untouched and word in lib.lp_last_error().decode(), kw
    need = lib.lp_jpeg_workspace_bytes((abi.JpegDesc * 1)(abi.JpegDesc(frames[0].data_ptr(), None, 60, 0, 20, 20, 0, 0)), 1, 16)
    assert need == 4 * 768 + 16
    rc, _, _, _, untouched = _raw_call(frames, 90, 16, 4096, ws_bytes=need - 1)
    assert rc == LP_ERR_ARG and untouched and 'workspace' in lib.lp_last_error().decode()
    # an NV12 frame that is not bt601f is refused at the C entry point (the wrapper converts it first)
    y = torch.zeros(4, 4, dtype=torch.uint8, device='cuda')
    uv = torch.zeros(2, 4, dtype=torch.uint8, device='cuda')
    out = torch.full((4096,), 0xA5, dtype=torch.uint8, device='cuda')
    nb = torch.full((1,), -5, dtype=torch.int32, device='cuda')
    ws = torch.zeros(4096, dtype=torch.uint8, device='cuda')
    hd = torch.zeros(625, dtype=torch.uint8, device='cuda')
    params = abi.JpegParams(90, 16)
    for matrix, ok in ((0, False), (1, False), (3, False), (2, True)):
        desc = (abi.JpegDesc * 1)(abi.JpegDesc(y.data_ptr(), uv.data_ptr(), 4, 4, 4, 4, 1, matrix))
        assert (lib.lp_jpeg_workspace_bytes(desc, 1, 16) > 0) == ok
        if not ok:
            rc = lib.lp_jpeg_encode_batch(desc, 1, ctypes.byref(params), ctypes.c_void_p(hd.data_ptr()), 625, ctypes.c_void_p(out.data_ptr()),
                                          4096, ctypes.c_void_p(nb.data_ptr()), ctypes.c_void_p((ws.data_ptr() + 255) // 256 * 256), 2048, None)
            torch.cuda.synchronize()
            assert rc == LP_ERR_ARG and 'bt601f' in lib.lp_last_error().decode()
            assert (out.cpu().numpy() == 0xA5).all() and int(nb.cpu()[0]) == -5
    for bad in (dict(quality=0), dict(quality=101), dict(restart=33), dict(restart=0), dict(cap=0)):
        with pytest.raises(ValueError):
            runtime.encode_jpeg(frames, **bad)
    with pytest.raises(ValueError):
        runtime.encode_jpeg([])
    with pytest.raises(ValueError):
        runtime.encode_jpeg([frames[0].cpu()])


def test_infer_save_jpeg(tmp_path, monkeypatch):
    """Inferer(redact='fill', save_jpeg=90) on two tiny frames: the .jpg files are the CPU path's (redact_plates_np of the rows
    returned, then encode_jpeg_np) byte for byte, PIL opens them, and no .png is written beside them."""
    from PIL import Image
    from yolov6.utils.jpeg import encode_jpeg_np
    from yolov6.utils.plate_crop import plate_crops_np
    from yolov6.utils.redact import redact_plates_np
    from yolov6.utils.synth import build_synthetic
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    ckpt = tmp_path / 'tiny.pt'
    torch.save({'model': build_synthetic(CFG('yololps'), width=0.0625, sigma=1.5).half(), 'ema': None}, str(ckpt))
    img_dir = tmp_path / 'imgs'
    img_dir.mkdir()
    frames = [synthetic(100, 60, seed=1), synthetic(150, 250, seed=2)]
    for i, f in enumerate(frames):
        Image.fromarray(f[..., ::-1]).save(str(img_dir / ('f%d.png' % i)))
    dets = infer.run(weights=str(ckpt), source=str(img_dir), yaml=None, img_size=[128, 128], conf_thres=0.06, iou_thres=0.45, max_det=20,
                     device='0', not_save_img=True, redact='fill', save_jpeg=90, save_crops=True, crop_size=(16, 48),
                     save_dir=str(tmp_path / 'out'))
    assert sum(len(d) for d in dets) > 0
    for i, (f, d) in enumerate(zip(frames, dets)):
        rows = np.zeros((1, max(len(d), 1), 28), np.float32)
        rows[0, :len(d)] = d.cpu().numpy()
        want = redact_plates_np([f], rows, [len(d)], 'fill', 16, 0.1)[0][0]
        path = tmp_path / 'out' / 'redacted' / ('f%d.jpg' % i)
        data = path.read_bytes()
        assert data == encode_jpeg_np(want, 90, 16)
        im = Image.open(io.BytesIO(data))
        im.load()
        assert im.size == (f.shape[1], f.shape[0])
        assert not (tmp_path / 'out' / 'redacted' / ('f%d.png' % i)).exists()
        crops = plate_crops_np(f, rows[0, :len(d)], (16, 48))[0]
        for k, c in enumerate(crops):
            assert (tmp_path / 'out' / 'imgs' / 'crops' / ('f%d_%d.jpg' % (i, k))).read_bytes() == encode_jpeg_np(c, 90, 16)


def test_infer_save_jpeg_batched_nv12_tracked(tmp_path, monkeypatch):
    """The other writers and the batched path: batch_size 4 on NV12 'bt709' frames with tracking, best shots, stacks, crops and a
    redaction held and delayed by two frames: the run with save_jpeg holds, for every .png of the run without it, the .jpg of
    the same pixels (``encode_jpeg_np``), and nothing else differs."""
    from PIL import Image
    import test_track_cpu as C
    from test_jpeg_cpu import compare_png_and_jpg_runs
    from yolov6.utils.synth import build_synthetic
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    ckpt = tmp_path / 'tiny.pt'
    torch.save({'model': build_synthetic(CFG('yololps'), width=0.0625, sigma=1.5).half(), 'ema': None, 'epoch': 0}, str(ckpt))
    img_dir = tmp_path / 'imgs'
    img_dir.mkdir()
    for k, f in enumerate(C._moving_frames(6)):
        Image.fromarray(f).save(str(img_dir / ('f%02d.png' % k)))
    kw = dict(weights=str(ckpt), source=str(img_dir), yaml=None, img_size=[128, 160], conf_thres=0.06, iou_thres=0.45, max_det=20,
              device='0', not_save_img=True, save_txt=True, batch_size=4, nv12='bt709', track=True, track_max_age=2, track_iou=0.25,
              track_expand=0.25, best_shots=True, crop_size=(16, 48), stack_shots=True, stack_search=1, stack_max_frames=4,
              stack_min_width=8.0, redact='fill', redact_hold=True, redact_lookback=2, save_crops=True)
    plain = infer.run(save_dir=str(tmp_path / 'png'), **kw)
    jpg = infer.run(save_dir=str(tmp_path / 'jpg'), save_jpeg=85, **kw)
    assert all(torch.equal(a, b) for a, b in zip(plain, jpg))
    assert compare_png_and_jpg_runs(tmp_path / 'png', tmp_path / 'jpg', 85) == {'redacted', 'crops', 'shots', 'stacks'}
