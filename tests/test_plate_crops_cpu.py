"""Plate crops, the parts that run without a GPU: argument checks of lp_plate_crops_batch through the C ABI, the numpy
mirror (yolov6/utils/plate_crop.py) against an independent float64 homography + grid_sample, its exact cases and status
rules, and tools/infer.py --save-crops on the CPU path."""
import ctypes
import importlib
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO

LP_ERR_ARG = -1


# ---- C ABI: everything is checked on the host before any launch ---------------------------------------------------------
def _desc(specs, img=0x1000, h0=1080, w0=1920):
    """CropDesc array from (max_crops, out_slot) pairs."""
    from yolov6.hip import abi
    d = (abi.CropDesc * max(len(specs), 1))()
    for e, (m, o) in zip(d, specs):
        e.img, e.h0, e.w0, e.max_crops, e.out_slot = img, h0, w0, m, o
    return d


def _crops(desc, n, n_slots, crop_h=64, crop_w=192, det=0x2000, count=0x3000, out=0x4000, status=0x5000, max_det=10):
    from yolov6.hip import abi
    v = lambda p: ctypes.c_void_p(p) if p else None   # noqa: E731
    return abi.load().lp_plate_crops_batch(desc, n, v(det), v(count), max_det, v(out), v(status), n_slots, crop_h, crop_w, None)


def test_plate_crops_rejects_bad_arguments_before_launch():
    from yolov6.hip import abi
    lib = abi.load()
    d = _desc([(4, 0), (4, 4), (4, 8)])
    d[1].img = None
    assert _crops(d, 3, 12) == LP_ERR_ARG and b'frame 1' in lib.lp_last_error()          # NULL img, named
    d = _desc([(4, 0), (4, 4)])
    d[0].h0 = 0
    assert _crops(d, 2, 8) == LP_ERR_ARG and b'frame 0' in lib.lp_last_error()
    d = _desc([(4, 0), (-1, 4)])
    assert _crops(d, 2, 8) == LP_ERR_ARG and b'frame 1' in lib.lp_last_error()            # negative max_crops
    d = _desc([(4, 0), (4, -4)])
    assert _crops(d, 2, 8) == LP_ERR_ARG and b'frame 1' in lib.lp_last_error()            # negative out_slot
    # slot ranges [0,4) and [3,7) overlap; so do [8,12) and [0,9) out of order; empty ranges overlap nothing
    assert _crops(_desc([(4, 0), (4, 3)]), 2, 8) == LP_ERR_ARG and b'overlap' in lib.lp_last_error()
    assert _crops(_desc([(4, 8), (9, 0)]), 2, 12) == LP_ERR_ARG and b'overlap' in lib.lp_last_error()
    assert _crops(_desc([(2, 5), (3, 2)]), 2, 8, count=0) == LP_ERR_ARG and b'null' in lib.lp_last_error()   # adjacent: fine
    # out_slot + max_crops > n_slots
    assert _crops(_desc([(4, 0), (4, 4)]), 2, 7) == LP_ERR_ARG and b'frame 1' in lib.lp_last_error()
    # crop size 0 or 1025 on either side
    for ch, cw in ((0, 192), (64, 0), (1025, 192), (64, 1025)):
        assert _crops(_desc([(4, 0)]), 1, 4, crop_h=ch, crop_w=cw) == LP_ERR_ARG and b'crop size' in lib.lp_last_error()
    # NULL det / count / out / status while a frame has slots
    for k in ('det', 'count', 'out', 'status'):
        assert _crops(_desc([(0, 0), (4, 0)]), 2, 4, **{k: 0}) == LP_ERR_ARG and b'null' in lib.lp_last_error()
    assert _crops(_desc([(4, 0)]), 1, 4, max_det=-1) == LP_ERR_ARG
    assert _crops(_desc([(4, 0)]), -1, 4) == LP_ERR_ARG
    assert _crops(None, 2, 4) == LP_ERR_ARG
    # nothing to do: LP_OK without a launch (no frames, or no frame with slots), whatever the pointers
    assert _crops(None, 0, 0, det=0, count=0, out=0, status=0) == 0
    assert _crops(_desc([(0, 0), (0, 3)]), 2, 3, det=0, count=0, out=0, status=0) == 0


# ---- the numpy mirror against an independent computation ---------------------------------------------------------------
def _reference_crop(frame, quad, crop_hw):
    """float64 DLT homography of the unit square onto ``quad`` (TL, TR, BR, BL) by torch.linalg.solve, sampled at the
    crop's pixel centres with float64 grid_sample(bilinear, border, align_corners=False); rounded to uint8."""
    src = [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)]
    A, rhs = [], []
    for (u, v), (X, Y) in zip(src, quad):
        A.append([u, v, 1, 0, 0, 0, -u * X, -v * X])
        A.append([0, 0, 0, u, v, 1, -u * Y, -v * Y])
        rhs += [X, Y]
    h = torch.linalg.solve(torch.tensor(A, dtype=torch.float64), torch.tensor(rhs, dtype=torch.float64))
    H = torch.cat([h, torch.ones(1, dtype=torch.float64)]).view(3, 3)
    Hc, Wc = crop_hw
    v, u = torch.meshgrid((torch.arange(Hc, dtype=torch.float64) + 0.5) / Hc, (torch.arange(Wc, dtype=torch.float64) + 0.5) / Wc,
                          indexing='ij')
    p = torch.stack([u, v, torch.ones_like(u)], -1) @ H.T
    X, Y = p[..., 0] / p[..., 2], p[..., 1] / p[..., 2]
    h0, w0 = frame.shape[:2]
    grid = torch.stack([2 * X / w0 - 1, 2 * Y / h0 - 1], -1)[None]
    img = torch.from_numpy(frame).double().permute(2, 0, 1)[None]
    out = F.grid_sample(img, grid, mode='bilinear', padding_mode='border', align_corners=False)[0].permute(1, 2, 0)
    return out.round().clamp(0, 255).to(torch.uint8).numpy()


def _row(box=None, tl=None, bl=None, br=None, tr=None):
    """A detection row: box (x1, y1, x2, y2) in columns 0..3, corners TL, BL, BR, TR in columns 4..11."""
    r = np.zeros(28, np.float32)
    if box is not None:
        r[:4] = box
    if tl is not None:
        r[4:12] = [*tl, *bl, *br, *tr]
    return r


def _rotated(cx, cy, w, h, deg):
    """Corners TL, BL, BR, TR of a w x h plate centred at (cx, cy), turned by ``deg`` (clockwise on screen)."""
    t = math.radians(deg)
    c, s = math.cos(t), math.sin(t)
    pts = [(-w / 2, -h / 2), (-w / 2, h / 2), (w / 2, h / 2), (w / 2, -h / 2)]
    return [(cx + c * x - s * y, cy + s * x + c * y) for x, y in pts]


def _frame(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


CASES = [  # frame (h, w), corners TL, BL, BR, TR, crop size
    ((1, 1), [(-2.0, -1.0), (-1.5, 3.0), (3.0, 2.5), (2.5, -1.5)], (8, 24)),
    ((37, 53), _rotated(26, 18, 30, 10, 17), (13, 47)),
    ((37, 53), [(-8.5, -3.0), (-6.0, 44.0), (61.0, 40.5), (58.0, -5.0)], (20, 60)),          # partly outside the frame
    ((300, 500), [(120.0, 80.0), (110.0, 190.0), (420.0, 230.0), (400.0, 60.0)], (64, 192)),  # perspective
    ((300, 500), _rotated(250, 150, 330, 110, -24), (64, 192)),
    ((1080, 1920), [(700.3, 500.8), (705.9, 640.1), (1190.4, 655.7), (1170.2, 470.6)], (64, 192)),
    ((1080, 1920), [(1800.0, 1000.0), (1790.0, 1150.0), (2100.0, 1190.0), (2050.0, 990.0)], (32, 96)),   # mostly outside
]


@pytest.mark.parametrize('k', range(len(CASES)))
def test_mirror_matches_homography_and_grid_sample(k):
    from yolov6.utils.plate_crop import plate_crops_np
    (h0, w0), (tl, bl, br, tr), crop_hw = CASES[k]
    frame = _frame(h0, w0, 100 + k)
    xs = [p[0] for p in (tl, bl, br, tr)]
    ys = [p[1] for p in (tl, bl, br, tr)]
    rows = np.stack([_row((min(xs), min(ys), max(xs), max(ys)), tl, bl, br, tr),            # status 1: the corners
                     _row((min(xs), min(ys), max(xs), max(ys)), tl, tr, br, bl)])           # bow-tie: status 2, the box
    crops, status = plate_crops_np(frame, rows, crop_hw)
    assert status.tolist() == [1, 2]
    f32 = lambda p: tuple(float(np.float32(v)) for v in p)   # noqa: E731  (the row holds fp32 values)
    ref1 = _reference_crop(frame, [f32(tl), f32(tr), f32(br), f32(bl)], crop_hw)
    bx = [float(np.float32(v)) for v in (min(xs), min(ys), max(xs), max(ys))]
    ref2 = _reference_crop(frame, [(bx[0], bx[1]), (bx[2], bx[1]), (bx[2], bx[3]), (bx[0], bx[3])], crop_hw)
    for got, ref in ((crops[0], ref1), (crops[1], ref2)):
        assert got.shape == crop_hw + (3,)
        assert int(np.abs(got.astype(np.int16) - ref.astype(np.int16)).max()) <= 1
    if (h0, w0) == (1, 1):
        assert (crops == frame[0, 0]).all()                         # a 1x1 frame: every sample is its one pixel


def test_mirror_exact_cases():
    from yolov6.utils.plate_crop import plate_crops_np, square_to_quad
    frame = _frame(120, 200, 7)
    # an integer box sampled at its own size is the frame's slice itself
    for x1, y1, x2, y2 in ((10, 20, 130, 60), (0, 0, 200, 120), (199, 119, 200, 120), (37, 5, 41, 93)):
        crops, status = plate_crops_np(frame, _row((x1, y1, x2, y2))[None], (y2 - y1, x2 - x1))
        assert status[0] == 2 and np.array_equal(crops[0], frame[y1:y2, x1:x2])
    # the map sends the unit square's corners to the quad's corners
    quads = [([10.0, 90.0, 85.0, 5.0], [20.0, 30.0, 70.0, 60.0]),
             ([1203.25, 1410.5, 1398.0, 1190.75], [611.5, 640.25, 700.0, 690.5]),
             ([3.0, 9.0, 9.0, 3.0], [4.0, 4.0, 7.0, 7.0])]
    for x, y in quads:
        a, b, c, d, e, f, g, h = square_to_quad(x, y)
        for k, (u, v) in enumerate(((0, 0), (1, 0), (1, 1), (0, 1))):
            w = g * u + h * v + 1.0
            assert abs((a * u + b * v + c) / w - x[k]) <= 1e-9 and abs((d * u + e * v + f) / w - y[k]) <= 1e-9
    a, b, c, d, e, f, g, h = square_to_quad([3.0, 9.0, 9.0, 3.0], [4.0, 4.0, 7.0, 7.0])
    assert g == 0 and h == 0                                        # an axis-aligned box is affine exactly


def test_mirror_status_rules():
    from yolov6.utils.plate_crop import plate_crops_np
    frame = _frame(100, 160, 9)
    box = (20.0, 30.0, 120.0, 70.0)
    tl, bl, br, tr = (22.0, 31.0), (20.0, 69.0), (119.0, 68.0), (121.0, 29.0)
    nan, inf = float('nan'), float('inf')
    rows = [
        (_row(box, tl, bl, br, tr), 1),                              # convex, label orientation
        (_row(box, tl, tr, br, bl), 2),                              # bow-tie (BL and TR swapped)
        (_row(box, tr, br, bl, tl), 2),                              # left-right mirrored: every cross product > 0
        (_row(box, (20.0, 30.0), (40.0, 50.0), (60.0, 70.0), (80.0, 90.0)), 2),   # collinear
        (_row(box, (20.0, 30.0), (20.0, 30.5), (20.5, 30.5), (20.5, 30.0)), 2),   # convex, area 0.25 < 1
        (_row(box, (nan, 31.0), bl, br, tr), 2),
        (_row(box, tl, bl, (inf, 68.0), tr), 2),
        (_row(box, tl, bl, br, (121.0, -inf)), 2),
        (_row((20.0, 30.0, 20.5, 70.0), tl, tr, br, bl), 3),         # invalid corners, box 0.5 wide
        (_row((20.0, 30.0, 120.0, 30.0), (nan, 0.0), bl, br, tr), 3),   # invalid corners, zero-height box
        (_row((nan, 30.0, 120.0, 70.0), tl, tr, br, bl), 3),         # invalid corners, NaN box
    ]
    crops, status = plate_crops_np(frame, np.stack([r for r, _ in rows]), (16, 48))
    assert status.tolist() == [s for _, s in rows]
    assert (crops[status == 3] == 0).all() and crops[status != 3].any()
    crops, status = plate_crops_np(frame, np.zeros((0, 28), np.float32), (16, 48))
    assert crops.shape == (0, 16, 48, 3) and status.shape == (0,)


# ---- tools/infer.py --save-crops on the CPU path --------------------------------------------------------------------------
def test_infer_save_crops_cpu(tmp_path, monkeypatch):
    from PIL import Image
    from yolov6.utils.plate_crop import plate_crops_np
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
    frames = {}
    for i, (h, w) in enumerate([(232, 144), (160, 200)]):
        frames['f%d' % i] = rng.integers(0, 255, (h, w, 3), dtype=np.uint8)
        Image.fromarray(frames['f%d' % i]).save(str(img_dir / ('f%d.png' % i)))
    out = tmp_path / 'out'
    monkeypatch.setattr(sys, 'argv', ['infer.py', '--weights', str(ckpt), '--source', str(img_dir), '--yaml', '', '--img-size', '128', '128',
                                      '--conf-thres', '0.06', '--max-det', '50', '--device', 'cpu', '--save-txt',
                                      '--not-save-img', '--save-dir', str(out), '--save-crops', '--crop-size', '24', '72'])
    infer.main(infer.get_args_parser())
    total = 0
    for stem, rgb in frames.items():
        txt = out / 'imgs' / (stem + '.txt')
        lines = txt.read_text().strip().splitlines() if txt.exists() else []
        pngs = sorted((out / 'imgs' / 'crops').glob(stem + '_*.png'))
        assert len(pngs) == len(lines)
        if not lines:
            continue
        # the rows behind the label lines: the same run's detections, in the same order
        res = infer.run(weights=str(ckpt), source=str(img_dir / (stem + '.png')), yaml=None, img_size=[128, 128],
                        conf_thres=0.06, iou_thres=0.45, max_det=50, device='cpu', not_save_img=True, save_dir=str(tmp_path / stem))
        det = res[0].float().numpy()
        assert len(det) == len(lines)
        crops, _ = plate_crops_np(rgb[:, :, ::-1], det, (24, 72))     # the PNG decodes to RGB; the frame is BGR
        for k in range(len(lines)):
            png = np.asarray(Image.open(str(out / 'imgs' / 'crops' / ('%s_%d.png' % (stem, k)))))
            assert png.shape == (24, 72, 3) and np.array_equal(png, crops[k][:, :, ::-1])
        total += len(lines)
    assert total >= 1
