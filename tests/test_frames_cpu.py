"""Batched inference from raw frames, the parts that run without a GPU: argument checks of the two batched entry points
(lp_preprocess_letterbox_batch, lp_rescale_round_batch) through the C ABI, the batch planner, and tools/infer.py
--batch-size on the CPU path (which ignores batching)."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

LP_ERR_ARG = -1


def _desc(n, img=0x1000, h0=1160, w0=720, rh=640, rw=397, top=0, left=9):
    from yolov6.hip import abi
    d = (abi.FrameDesc * n)()
    for e in d:
        e.img, e.h0, e.w0, e.rh, e.rw, e.top, e.left = img, h0, w0, rh, rw, top, left
    return d


def _letterbox_batch(desc, n, B, dtype=2, H=640, W=416, out=0x2000):
    from yolov6.hip import abi
    return abi.load().lp_preprocess_letterbox_batch(desc, n, B, ctypes.c_void_p(out), dtype, H, W, None)


def test_letterbox_batch_rejects_bad_arguments_before_launch():
    from yolov6.hip import abi
    lib = abi.load()
    d = _desc(3)
    d[1].img = None
    assert _letterbox_batch(d, 3, 4) == LP_ERR_ARG and b'frame 1' in lib.lp_last_error()      # NULL img, named
    d = _desc(3)
    d[2].top = 1                                                                            # top + rh = 641 > H
    assert _letterbox_batch(d, 3, 4) == LP_ERR_ARG and b'frame 2' in lib.lp_last_error()
    d = _desc(2)
    d[0].left = 20                                                                          # left + rw > W
    assert _letterbox_batch(d, 2, 2) == LP_ERR_ARG and b'frame 0' in lib.lp_last_error()
    assert _letterbox_batch(_desc(2), 2, 2, dtype=7) == LP_ERR_ARG and b'dtype' in lib.lp_last_error()
    assert _letterbox_batch(_desc(3), 3, 2) == LP_ERR_ARG                                   # n_frames > B
    assert _letterbox_batch(_desc(1), -1, 2) == LP_ERR_ARG                                  # negative frame count
    assert _letterbox_batch(_desc(1), 1, 1, out=0) == LP_ERR_ARG
    assert _letterbox_batch(None, 1, 1) == LP_ERR_ARG


def test_rescale_batch_rejects_bad_arguments_before_launch():
    from yolov6.hip import abi
    lib = abi.load()
    d = (abi.RescaleDesc * 3)()
    for e in d:
        e.ratio, e.padx, e.pady, e.img_w, e.img_h = 0.55, 9.0, 0.0, 720, 1160
    det, cnt = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)
    assert lib.lp_rescale_round_batch(det, cnt, -1, 10, d, None) == LP_ERR_ARG          # negative image count
    assert lib.lp_rescale_round_batch(det, cnt, 3, -5, d, None) == LP_ERR_ARG           # negative max_det
    assert lib.lp_rescale_round_batch(None, cnt, 3, 10, d, None) == LP_ERR_ARG
    assert lib.lp_rescale_round_batch(det, None, 3, 10, d, None) == LP_ERR_ARG
    d[2].ratio = 0.0
    assert lib.lp_rescale_round_batch(det, cnt, 3, 10, d, None) == LP_ERR_ARG and b'image 2' in lib.lp_last_error()
    assert lib.lp_rescale_round_batch(det, cnt, 0, 10, d, None) == 0                    # nothing to do: no launch


def test_plan_batches():
    from yolov6.core.frames import letterbox_hw, plan_batches
    ccpd = (1160, 720, 3)
    assert letterbox_hw(ccpd, [640, 640], 32) == (640, 416)
    assert plan_batches([ccpd] * 8, [640, 640], 32, 4) == [[0, 1, 2, 3], [4, 5, 6, 7]]               # whole batches
    assert plan_batches([ccpd] * 10, [640, 640], 32, 4) == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]      # shorter tail
    # 1080p letterboxes to 384x640: a shape change ends a group, and source order is kept (no reordering)
    shapes = [ccpd, ccpd, (1080, 1920, 3), ccpd, ccpd, ccpd]
    assert plan_batches(shapes, [640, 640], 32, 4) == [[0, 1], [2], [3, 4, 5]]
    # frames of other sizes that letterbox to the same (H, W) share a batch
    assert plan_batches([ccpd, (580, 360, 3)], [640, 640], 32, 4) == [[0, 1]]
    # auto=False: every frame becomes exactly img_size, so mixed sizes merge
    assert plan_batches(shapes, [640, 640], 32, 4, auto=False) == [[0, 1, 2, 3], [4, 5]]
    assert plan_batches([], [640, 640], 32, 4) == []
    assert plan_batches([ccpd] * 3, [640, 640], 32, 1) == [[0], [1], [2]]
    with pytest.raises(ValueError):
        plan_batches([ccpd], [640, 640], 32, 0)


def test_infer_batch_size_is_ignored_on_cpu(tmp_path, monkeypatch):
    from PIL import Image
    from yolov6.utils.synth import build_synthetic
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    m = build_synthetic(os.path.join(REPO, 'configs', 'yololps.py'), width=0.0625, sigma=1.5)
    ckpt = tmp_path / 'tiny.pt'
    torch.save({'model': m.half(), 'ema': None, 'epoch': 0}, str(ckpt))
    img_dir = tmp_path / 'imgs'
    img_dir.mkdir()
    rng = np.random.default_rng(5)
    for i, (h, w) in enumerate([(232, 144), (232, 144), (160, 200)]):
        Image.fromarray(rng.integers(0, 255, (h, w, 3), dtype=np.uint8)).save(str(img_dir / ('f%d.png' % i)))
    kw = dict(weights=str(ckpt), source=str(img_dir), yaml=None, img_size=[128, 128], conf_thres=0.06, iou_thres=0.45,
              max_det=50, device='cpu', save_txt=True, not_save_img=True, half=False)
    one = infer.run(save_dir=str(tmp_path / 'o1'), **kw)
    four = infer.run(save_dir=str(tmp_path / 'o4'), batch_size=4, **kw)
    assert len(one) == len(four) == 3 and sum(len(d) for d in one) > 0
    for a, b in zip(one, four):
        assert torch.equal(a, b)
    for i in range(3):
        p1, p4 = tmp_path / 'o1' / 'imgs' / ('f%d.txt' % i), tmp_path / 'o4' / 'imgs' / ('f%d.txt' % i)
        assert p1.exists() == p4.exists()
        if p1.exists():
            assert p1.read_bytes() == p4.read_bytes()
