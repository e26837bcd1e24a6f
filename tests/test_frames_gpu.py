"""Batched inference from raw frames on the GPU: the two batched kernels against their single-frame counterparts, and
detect_frames / FrameBatcher / Inferer(batch_size=N) against the per-frame path -- all bit for bit."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu

CFG = lambda n: os.path.join(REPO, 'configs', n + '.py')   # noqa: E731
_BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _frames(shapes, seed, odd_offsets=False):
    """Seeded uint8 CUDA frames; with ``odd_offsets`` they are slices of one buffer starting at odd byte addresses."""
    rng = np.random.default_rng(seed)
    if not odd_offsets:
        return [torch.from_numpy(rng.integers(0, 256, s + (3,), dtype=np.uint8)).cuda() for s in shapes]
    sizes = [h * w * 3 for h, w in shapes]
    buf = torch.from_numpy(rng.integers(0, 256, sum(sizes) + 2 * len(sizes) + 1, dtype=np.uint8)).cuda()
    out, off = [], 1
    for (h, w), n in zip(shapes, sizes):
        out.append(buf[off:off + n].view(h, w, 3))
        assert out[-1].data_ptr() % 2 == 1
        off = (off + n) | 1
    return out


def _geometry(shape, size, auto):
    from yolov6.data.data_augment import letterbox_geometry
    _, (rw, rh), (top, bottom, left, right), _ = letterbox_geometry(shape, size, auto=auto, stride=32)
    return rh, rw, top, left, rh + top + bottom, rw + left + right


def _letterbox_both(frames, size, dtype, B, auto=False):
    """(batched kernel output, per-frame kernel outputs stacked, with padding slots = 114/255), both written over NaN."""
    from yolov6.hip import abi
    lib = abi.load()
    geo = [_geometry(tuple(f.shape[:2]), size, auto) for f in frames]
    H, W = geo[0][4:]
    got = torch.full((B, 3, H, W), float('nan'), dtype=dtype, device='cuda')
    ref = torch.full((B, 3, H, W), float('nan'), dtype=dtype, device='cuda')
    desc = (abi.FrameDesc * max(len(frames), 1))()
    for d, f, (rh, rw, top, left, _, _) in zip(desc, frames, geo):
        d.img, d.h0, d.w0, d.rh, d.rw, d.top, d.left = f.data_ptr(), f.shape[0], f.shape[1], rh, rw, top, left
    dt = {torch.float16: abi.LP_F16, torch.bfloat16: abi.LP_BF16, torch.float32: abi.LP_F32}[dtype]
    abi.check(lib.lp_preprocess_letterbox_batch(desc, len(frames), B, ctypes.c_void_p(got.data_ptr()), dt, H, W, _stream()))
    for b, (f, (rh, rw, top, left, _, _)) in enumerate(zip(frames, geo)):
        abi.check(lib.lp_preprocess_letterbox(ctypes.c_void_p(f.data_ptr()), f.shape[0], f.shape[1], ctypes.c_void_p(ref[b].data_ptr()),
                                              dt, H, W, rh, rw, top, left, _stream()))
    ref[len(frames):] = (torch.tensor(114.0) / 255).to(dtype)
    torch.cuda.synchronize()
    return got, ref


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(_BITS[a.dtype]), b.view(_BITS[b.dtype]))


MIXED = [(1, 1), (1, 37), (300, 500), (2000, 1500), (2160, 3840), (416, 416), (37, 1), (97, 131)]


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16])
def test_letterbox_batch_equals_per_frame_kernel(dtype):
    # mixed sizes at a fixed 416x416 (416x416 itself: no resize), two padding slots
    got, ref = _letterbox_both(_frames(MIXED, 1), [416, 416], dtype, B=len(MIXED) + 2)
    assert _bits_equal(got, ref)
    # no resize at 640, and an upscale, at odd byte offsets of one buffer
    got, ref = _letterbox_both(_frames([(640, 640), (300, 500), (1, 1)], 2, odd_offsets=True), [640, 640], dtype, B=3)
    assert _bits_equal(got, ref)
    # B = 1, reference letterbox arithmetic (auto: 416 x 640 for a 1080p frame); W = 640 -> 8/16-byte stores
    got, ref = _letterbox_both(_frames([(1080, 1920)], 3), [640, 640], dtype, B=1, auto=True)
    assert got.shape == (1, 3, 384, 640) and _bits_equal(got, ref)
    # a width that is not a multiple of 4: the per-element store path
    got, ref = _letterbox_both(_frames([(300, 500), (50, 50)], 4), [98, 98], dtype, B=2)
    assert got.shape[3] == 98 and _bits_equal(got, ref)


def test_letterbox_batch_crosses_the_64_frame_split():
    shapes = [(20 + 7 * i, 90 - i) for i in range(65)]
    got, ref = _letterbox_both(_frames(shapes, 5, odd_offsets=True), [96, 128], torch.float16, B=65)
    assert _bits_equal(got, ref)
    got, ref = _letterbox_both(_frames(shapes[:63], 6), [96, 128], torch.float32, B=130)      # 67 padding slots, 3 launches
    assert _bits_equal(got, ref)
    assert bool((got[63:] == (torch.tensor(114.0) / 255)).all())


def test_rescale_round_batch_equals_per_image_kernel():
    from yolov6.hip import abi
    lib = abi.load()
    B, max_det = 67, 40
    g = torch.Generator().manual_seed(7)
    counts = torch.randint(0, max_det + 1, (B,), generator=g, dtype=torch.int32)
    counts[0], counts[1], counts[2], counts[3] = 0, max_det, max_det + 9, -3          # clamped to max_det / 0 on the device
    det = (torch.rand(B, max_det, 28, generator=g) * 900 - 100).cuda()
    shapes = [(int(h), int(w)) for h, w in zip(torch.randint(1, 3000, (B,), generator=g), torch.randint(1, 3000, (B,), generator=g))]
    net = (640, 416)
    ref = det.clone()
    for b, (h, w) in enumerate(shapes):
        ratio = min(net[0] / h, net[1] / w)
        padx, pady = (net[1] - w * ratio) / 2, (net[0] - h * ratio) / 2
        n = max(0, min(int(counts[b]), max_det))
        abi.check(lib.lp_rescale_round(ctypes.c_void_p(ref[b].data_ptr()), n, ratio, padx, pady, w, h, _stream()))
    from yolov6.hip.runtime import rescale_round_batch
    got = rescale_round_batch(det.clone(), counts.cuda(), net, shapes)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    # untouched: columns 12..27 everywhere and every row at or beyond the count
    assert torch.equal(got[..., 12:], det[..., 12:])
    for b in range(B):
        n = max(0, min(int(counts[b]), max_det))
        assert torch.equal(got[b, n:], det[b, n:])
        if n:
            assert not torch.equal(got[b, :n, :12], det[b, :n, :12])


def _per_frame(model, frames, size, dtype, auto, conf, iou, max_det):
    from yolov6.hip import runtime
    out = []
    for f in frames:
        img = runtime.preprocess_letterbox(f, size, 32, dtype, auto=auto)
        det = runtime.detect(model, img[None], conf, iou, max_det)[0]
        if len(det):
            runtime.rescale_round(img.shape[1:], det, tuple(f.shape))
        out.append(det)
    return out


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_detect_frames_equals_per_frame_path(dtype):
    from yolov6.hip import runtime
    from yolov6.utils.synth import build_synthetic
    m = build_synthetic(CFG('yololps'), width=0.0625, sigma=1.5).cuda().to(dtype)
    size, conf, iou, max_det = [256, 256], 0.06, 0.45, 50
    cases = [(_frames([(464, 288)] * 3 + [(232, 144)], 8), True, None),           # one letterboxed shape (256 x 160)
             (_frames([(464, 288), (300, 500), (97, 131), (256, 256), (1, 1)], 9), False, 8)]   # mixed sizes, 3 padding slots
    total = 0
    with torch.no_grad():
        for frames, auto, batch in cases:
            got = runtime.detect_frames(m, frames, size, conf, iou, max_det, auto=auto, batch=batch)
            ref = _per_frame(m, frames, size, dtype, auto, conf, iou, max_det)
            assert len(got) == len(frames)
            for g, r in zip(got, ref):
                assert g.shape == r.shape and torch.equal(g, r)
                total += len(g)
    assert total > 0
    with pytest.raises(ValueError):
        runtime.detect_frames(m, _frames([(464, 288), (300, 500)], 10), size, conf, iou, max_det)   # two shapes, auto=True


def test_frame_batcher_consecutive_batches():
    """Batches put back to back without a host sync (the staging and device buffers alternate): each equals its batch run
    on its own."""
    from yolov6.core.frames import FrameBatcher
    from yolov6.hip import runtime
    rng = np.random.default_rng(11)
    batches = [[rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8) for _ in range(4)] for _ in range(5)]
    batcher = FrameBatcher('cuda:0')
    outs = []
    for frames in batches:
        x, _ = runtime.preprocess_frames(batcher.put(frames), [640, 640], 32, torch.float16)
        outs.append(x)
    for frames, x in zip(batches, outs):
        alone, _ = runtime.preprocess_frames([torch.from_numpy(f).cuda() for f in frames], [640, 640], 32, torch.float16)
        assert _bits_equal(x, alone)


def test_infer_batch_size_matches_per_frame(tmp_path, monkeypatch):
    from PIL import Image
    from yolov6.utils.synth import build_synthetic
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    m = build_synthetic(CFG('yololps'), width=0.0625, sigma=1.5)
    ckpt = tmp_path / 'tiny.pt'
    torch.save({'model': m.half(), 'ema': None}, str(ckpt))
    img_dir = tmp_path / 'imgs'
    img_dir.mkdir()
    rng = np.random.default_rng(12)
    shapes = [(464, 288), (464, 288), (464, 288), (300, 500), (300, 500), (464, 288), (200, 120)]   # 3 sizes, 7 frames
    for i, (h, w) in enumerate(shapes):
        Image.fromarray(rng.integers(0, 255, (h, w, 3), dtype=np.uint8)).save(str(img_dir / ('f%d.png' % i)))
    kw = dict(weights=str(ckpt), source=str(img_dir), yaml=None, img_size=[256, 256], conf_thres=0.06, iou_thres=0.45,
              max_det=50, device='0', save_txt=True, not_save_img=True)
    for half in (False, True):
        tag = 'h' if half else 'f'
        one = infer.run(save_dir=str(tmp_path / ('o1' + tag)), half=half, **kw)
        four = infer.run(save_dir=str(tmp_path / ('o4' + tag)), half=half, batch_size=4, **kw)
        assert len(one) == len(four) == 7 and sum(len(d) for d in one) > 0
        for a, b in zip(one, four):
            assert b.is_cuda and torch.equal(a, b)
        for i in range(7):
            p1, p4 = tmp_path / ('o1' + tag) / 'imgs' / ('f%d.txt' % i), tmp_path / ('o4' + tag) / 'imgs' / ('f%d.txt' % i)
            assert p1.exists() == p4.exists()
            if p1.exists():
                assert p1.read_bytes() == p4.read_bytes()
