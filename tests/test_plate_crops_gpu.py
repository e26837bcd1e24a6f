"""Plate crops on the GPU: lp_plate_crops_batch against the numpy mirror (yolov6/utils/plate_crop.py) bit for bit, its slot
handling (poisoned output, the 64-frame split, packed against dense layouts), graph capture, detect_frames_with_crops
against detect_frames + the mirror, and Inferer(save_crops=True) at batch sizes 1 and 4."""
import ctypes
import importlib
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu

CFG = lambda n: os.path.join(REPO, 'configs', n + '.py')   # noqa: E731
POISON = 0xA5
ST_POISON = -7


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


def _quad_rows(h0, w0, n, seed):
    """n detection rows [n, 28] for an h0 x w0 frame, by r % 6: rotated and perspective plates (corners: status 1), a plate
    partly outside the frame (1), a bow-tie and a NaN corner over a valid box (2), and corners in the reverse orientation
    over a box 0.5 px wide (3).  Plates are at least 6 px wide, so every convex quad has area >= 1 whatever the frame size."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 28), np.float32)
    rows[:, 12:] = rng.random((n, 16))
    for r in range(n):
        kind = r % 6
        w = max(6.0, rng.uniform(0.1, 0.6) * w0)
        h = w / 3.1
        cx, cy = rng.uniform(0, w0), rng.uniform(0, h0)
        if kind == 2:
            cx, cy = rng.choice([-0.2, 1.2]) * w0, rng.uniform(-0.2, 1.2) * h0
        t = math.radians(rng.uniform(-35, 35))
        c, s = math.cos(t), math.sin(t)
        pts = []
        for px, py in ((-w / 2, -h / 2), (-w / 2, h / 2), (w / 2, h / 2), (w / 2, -h / 2)):     # TL, BL, BR, TR
            if kind == 1:
                px, py = px + rng.uniform(-0.12, 0.12) * w, py + rng.uniform(-0.15, 0.15) * h
            pts.append((cx + c * px - s * py, cy + s * px + c * py))
        xs, ys = [p[0] for p in pts], [p[1] for p in pts]
        rows[r, :4] = [min(xs), min(ys), max(xs), max(ys)]
        if kind == 3:
            pts = [pts[0], pts[3], pts[2], pts[1]]                  # bow-tie
        rows[r, 4:12] = [v for p in pts for v in p]
        if kind == 4:
            rows[r, 4 + 2 * rng.integers(0, 4)] = np.nan
        if kind == 5:
            rows[r, 4:12] = rows[r, [4, 5, 10, 11, 8, 9, 6, 7]]      # TL, TR, BR, BL: every cross product > 0
            rows[r, 2] = rows[r, 0] + 0.5
    return rows


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _kernel(frames, det, count, specs, n_slots, crop_hw):
    """lp_plate_crops_batch with explicit (max_crops, out_slot) per frame into poisoned out / status: host copies of both."""
    from yolov6.hip import abi
    out = torch.full((n_slots,) + tuple(crop_hw) + (3,), POISON, dtype=torch.uint8, device='cuda')
    status = torch.full((n_slots,), ST_POISON, dtype=torch.int32, device='cuda')
    desc = (abi.CropDesc * len(frames))()
    for d, f, (m, o) in zip(desc, frames, specs):
        d.img, d.h0, d.w0, d.max_crops, d.out_slot = f.data_ptr(), f.shape[0], f.shape[1], m, o
    abi.check(abi.load().lp_plate_crops_batch(desc, len(frames), ctypes.c_void_p(det.data_ptr()), ctypes.c_void_p(count.data_ptr()),
                                              det.shape[1], ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(status.data_ptr()),
                                              n_slots, crop_hw[0], crop_hw[1], _stream()), 'lp_plate_crops_batch')
    torch.cuda.synchronize()
    return out.cpu().numpy(), status.cpu().numpy()


def _mirror(frames, det, count, specs, n_slots, crop_hw):
    """What _kernel must return, from the numpy mirror: poison wherever nothing may be written."""
    from yolov6.utils.plate_crop import plate_crops_np
    out = np.full((n_slots,) + tuple(crop_hw) + (3,), POISON, dtype=np.uint8)
    status = np.full(n_slots, ST_POISON, dtype=np.int32)
    det_h, count_h = det.cpu().numpy(), count.cpu().numpy()
    for b, (f, (m, o)) in enumerate(zip(frames, specs)):
        n = max(0, min(int(count_h[b]), det.shape[1], m))
        crops, st = plate_crops_np(f.cpu().numpy(), det_h[b, :n], crop_hw)
        out[o:o + n] = crops
        status[o:o + m] = 0
        status[o:o + n] = st
    return out, status


SHAPES = [(1, 1), (37, 1), (97, 131), (464, 288), (1080, 1920), (2160, 3840)]


@pytest.mark.parametrize('crop_hw', [(64, 192), (1, 1), (13, 47), (256, 1024)])
def test_kernel_equals_mirror(crop_hw):
    max_det = 12
    for odd in (False, True):
        frames = _frames(SHAPES, 20 + odd, odd_offsets=odd)
        det = torch.from_numpy(np.stack([_quad_rows(h, w, max_det, 30 + b) for b, (h, w) in enumerate(SHAPES)])).cuda()
        # counts: > max_crops, 0, negative, > max_det (max_crops 16 > max_det), and within range
        count = torch.tensor([11, 0, -3, 40, 7, 12], dtype=torch.int32, device='cuda')
        specs = [(8, 0), (3, 8), (2, 11), (16, 30), (7, 13), (12, 46)]     # out of slot order, gaps at 20..29 and 58..59
        got, got_st = _kernel(frames, det, count, specs, 60, crop_hw)
        ref, ref_st = _mirror(frames, det, count, specs, 60, crop_hw)
        assert np.array_equal(got_st, ref_st)
        assert set(ref_st.tolist()) == {ST_POISON, 0, 1, 2, 3}
        assert np.array_equal(got, ref)                     # the crops, and the poison around them
        assert (got[20:30] == POISON).all() and (got[58:] == POISON).all()


def test_kernel_crosses_the_64_frame_split_and_packed_equals_dense():
    from yolov6.hip import runtime
    shapes = [(40 + 9 * i, 120 - i) for i in range(67)]
    frames = _frames(shapes, 40, odd_offsets=True)
    max_det = 5
    det = torch.from_numpy(np.stack([_quad_rows(h, w, max_det, 50 + b) for b, (h, w) in enumerate(shapes)])).cuda()
    counts = [(b * 3) % 7 - 1 for b in range(67)]                 # -1 .. 5
    count = torch.tensor(counts, dtype=torch.int32, device='cuda')
    crop_hw = (24, 72)
    dense_specs = [(4, 4 * b) for b in range(67)]
    got, got_st = _kernel(frames, det, count, dense_specs, 4 * 67, crop_hw)
    ref, ref_st = _mirror(frames, det, count, dense_specs, 4 * 67, crop_hw)
    assert np.array_equal(got_st, ref_st) and np.array_equal(got, ref)
    # the runtime's dense form writes the same (its slots of status 0 keep what the buffer held)
    out = torch.full((67, 4) + crop_hw + (3,), POISON, dtype=torch.uint8, device='cuda')
    crops, status = runtime.plate_crops(frames, det, count, crop_hw, max_crops=4, out=out)
    assert crops.data_ptr() == out.data_ptr() and status.shape == (67, 4)
    assert np.array_equal(crops.cpu().numpy().reshape(got.shape), got)
    assert np.array_equal(status.cpu().numpy().reshape(-1), got_st)
    # packed: max_crops_b = n_b at prefix-sum slots, as detect_frames_with_crops lays them out
    ns = [max(0, min(c, 4)) for c in counts]                       # the dense form's n_b: count clamped to max_crops 4
    offs = np.concatenate([[0], np.cumsum(ns)]).astype(int).tolist()
    packed, packed_st = _kernel(frames, det, count, list(zip(ns, offs)), offs[-1], crop_hw)
    for b in range(67):
        assert np.array_equal(packed[offs[b]:offs[b + 1]], got[4 * b:4 * b + ns[b]])
        assert np.array_equal(packed_st[offs[b]:offs[b + 1]], got_st[4 * b:4 * b + ns[b]])


def test_plate_crops_graph_capture():
    from yolov6.hip import runtime
    shapes = [(1080, 1920), (464, 288), (97, 131)]
    frames = _frames(shapes, 60)
    max_det, crop_hw = 6, (64, 192)
    det = torch.from_numpy(np.stack([_quad_rows(h, w, max_det, 70 + b) for b, (h, w) in enumerate(shapes)])).cuda()
    count = torch.tensor([6, 2, 0], dtype=torch.int32, device='cuda')
    out = torch.empty(3, 4, *crop_hw, 3, dtype=torch.uint8, device='cuda')
    status = torch.empty(3, 4, dtype=torch.int32, device='cuda')
    runtime.plate_crops(frames, det, count, crop_hw, max_crops=4, out=out, status=status)     # eager once: code loaded
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        runtime.plate_crops(frames, det, count, crop_hw, max_crops=4, out=out, status=status)
    rng = np.random.default_rng(61)
    for f in frames:                                                # new pixels, new rows, new counts, same buffers
        f.copy_(torch.from_numpy(rng.integers(0, 256, tuple(f.shape), dtype=np.uint8)))
    det.copy_(torch.from_numpy(np.stack([_quad_rows(h, w, max_det, 80 + b) for b, (h, w) in enumerate(shapes)])))
    count.copy_(torch.tensor([1, 5, 3], dtype=torch.int32))
    out.fill_(POISON)
    status.fill_(ST_POISON)
    g.replay()
    torch.cuda.synchronize()
    ref, ref_st = _mirror(frames, det, count, [(4, 4 * b) for b in range(3)], 12, crop_hw)
    assert np.array_equal(status.cpu().numpy().reshape(-1), ref_st)
    assert np.array_equal(out.cpu().numpy().reshape(ref.shape), ref)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_detect_frames_with_crops(dtype):
    from yolov6.hip import runtime
    from yolov6.utils.plate_crop import plate_crops_np
    from yolov6.utils.synth import build_synthetic
    m = build_synthetic(CFG('yololps'), width=0.0625, sigma=1.5).cuda().to(dtype)
    size, conf, iou, max_det = [256, 256], 0.06, 0.45, 50
    cases = [(_frames([(464, 288)] * 3 + [(232, 144)], 8), True, None, (64, 192)),
             (_frames([(464, 288), (300, 500), (97, 131), (256, 256), (1, 1)], 9, odd_offsets=True), False, 8, (13, 47))]
    total = 0
    with torch.no_grad():
        for frames, auto, batch, crop_hw in cases:
            ref = runtime.detect_frames(m, frames, size, conf, iou, max_det, auto=auto, batch=batch)
            dets, crops, status = runtime.detect_frames_with_crops(m, frames, size, conf, iou, max_det, crop_hw, auto=auto, batch=batch)
            assert len(dets) == len(crops) == len(status) == len(frames)
            for f, d, r, c, s in zip(frames, dets, ref, crops, status):
                assert d.shape == r.shape and torch.equal(d, r)
                assert c.shape == (len(d),) + crop_hw + (3,) and s.shape == (len(d),) and s.dtype == torch.int32
                want, want_st = plate_crops_np(f.cpu().numpy(), d.cpu().numpy(), crop_hw)
                assert np.array_equal(c.cpu().numpy(), want) and np.array_equal(s.cpu().numpy(), want_st)
                total += len(d)
            for k, (c, s) in enumerate(zip(crops, status)):        # one packed tensor: frame b's crops right behind b-1's
                before = sum(len(x) for x in dets[:k])
                assert c.untyped_storage().data_ptr() == crops[0].untyped_storage().data_ptr()
                assert c.storage_offset() == before * crop_hw[0] * crop_hw[1] * 3 and s.storage_offset() == before
    assert total > 0


def test_infer_save_crops_batch_size_1_and_4(tmp_path, monkeypatch):
    from PIL import Image
    from yolov6.utils.plate_crop import plate_crops_np
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
    shapes = [(464, 288), (464, 288), (464, 288), (300, 500), (300, 500), (464, 288), (200, 120)]   # the set of test_frames_gpu
    frames = []
    for i, (h, w) in enumerate(shapes):
        frames.append(rng.integers(0, 255, (h, w, 3), dtype=np.uint8))
        Image.fromarray(frames[-1]).save(str(img_dir / ('f%d.png' % i)))
    kw = dict(weights=str(ckpt), source=str(img_dir), yaml=None, img_size=[256, 256], conf_thres=0.06, iou_thres=0.45,
              max_det=50, device='0', save_txt=True, not_save_img=True, save_crops=True, crop_size=(32, 96))
    for half in (False, True):
        tag = 'h' if half else 'f'
        one = infer.run(save_dir=str(tmp_path / ('o1' + tag)), half=half, **kw)
        four = infer.run(save_dir=str(tmp_path / ('o4' + tag)), half=half, batch_size=4, **kw)
        assert len(one) == len(four) == 7 and sum(len(d) for d in one) > 0
        for i, (a, b) in enumerate(zip(one, four)):
            assert torch.equal(a, b)
            p1 = sorted((tmp_path / ('o1' + tag) / 'imgs' / 'crops').glob('f%d_*.png' % i))
            p4 = sorted((tmp_path / ('o4' + tag) / 'imgs' / 'crops').glob('f%d_*.png' % i))
            assert [p.name for p in p1] == [p.name for p in p4] and len(p1) == len(a)
            want, _ = plate_crops_np(frames[i][:, :, ::-1], a.cpu().numpy(), (32, 96))
            for k in range(len(a)):
                f1 = tmp_path / ('o1' + tag) / 'imgs' / 'crops' / ('f%d_%d.png' % (i, k))
                f4 = tmp_path / ('o4' + tag) / 'imgs' / 'crops' / ('f%d_%d.png' % (i, k))
                assert f1.read_bytes() == f4.read_bytes()
                assert np.array_equal(np.asarray(Image.open(str(f1))), want[k][:, :, ::-1])
