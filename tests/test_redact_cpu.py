"""Plate redaction, the specification (yolov6/utils/redact.py::redact_plates_np) against things that are not the specification:
a pixel set computed in pure integer arithmetic, cell means computed in float64, the properties the rule promises (the order
of the rows does not matter, a second pass changes only what the first changed, nothing outside the plates changes), the status
codes, the counts, NV12 chroma, fill mode, and the CPU path of Inferer(redact=...)."""
import importlib
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

CFG = lambda n: os.path.join(REPO, 'configs', n + '.py')   # noqa: E731
KINDS = 6


def quad_rows(h0, w0, n, seed, snap=None):
    """n detection rows [n, 28] for an h0 x w0 frame, by r % 6: a rotated plate and a perspective plate (corners: status 1), a
    plate partly or wholly outside the frame (1), a bow-tie and a NaN corner over a valid box (2), corners in the reverse
    orientation over a box 0.5 px wide (3).  Plates are 0.15 .. 0.6 of the frame wide (at least 6 px: every convex quad has area
    >= 1), so on a small frame they overlap.  ``snap``: round every coordinate to a multiple of 1 / snap."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 28), np.float32)
    rows[:, 12:] = rng.random((n, 16))
    for r in range(n):
        kind = r % KINDS
        w = max(6.0, rng.uniform(0.15, 0.6) * w0)
        h = w / 3.1
        cx, cy = rng.uniform(0, w0), rng.uniform(0, h0)
        if kind == 2:
            cx, cy = rng.choice([-0.1, 0.0, 1.0, 1.4]) * w0, rng.uniform(-0.2, 1.2) * h0
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
        if snap:
            rows[r, :12] = np.round(rows[r, :12] * snap) / snap
        if kind == 4:
            rows[r, 4 + 2 * rng.integers(0, 4)] = np.nan
        if kind == 5:
            rows[r, 4:12] = rows[r, [4, 5, 10, 11, 8, 9, 6, 7]]      # TL, TR, BR, BL: every cross product > 0
            rows[r, 2] = rows[r, 0] + 0.5
    return rows


EXPECTED_STATUS = [1, 1, 1, 2, 2, 3]


def frame_of(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def integer_mask(row, h, w):
    """(status, mask) of a row whose twelve coordinates are multiples of 1/8, margin 0, in integers only: coordinates x 16,
    pixel centres 16 j + 8."""
    q = [int(round(float(v) * 16)) if math.isfinite(float(v)) else None for v in row[:12]]
    X, Y = [q[4], q[10], q[8], q[6]], [q[5], q[11], q[9], q[7]]      # p0 = TL, p1 = TR, p2 = BR, p3 = BL
    order = (0, 3, 2, 1)
    st = 3
    if all(v is not None for v in X + Y):
        convex = True
        for k in range(4):
            a, b, c = order[k], order[(k + 1) % 4], order[(k + 2) % 4]
            if not ((X[b] - X[a]) * (Y[c] - Y[b]) - (Y[b] - Y[a]) * (X[c] - X[b]) < 0):
                convex = False
        area2 = abs((X[2] - X[0]) * (Y[3] - Y[1]) - (X[3] - X[1]) * (Y[2] - Y[0]))       # 2 x area x 256
        if convex and area2 >= 2 * 256:
            st = 1
    if st == 3 and all(v is not None for v in q[:4]) and q[2] - q[0] >= 16 and q[3] - q[1] >= 16:
        st = 2
        X, Y = [q[0], q[2], q[2], q[0]], [q[1], q[1], q[3], q[3]]
    mask = np.zeros((h, w), bool)
    if st == 3:
        return st, mask
    for i in range(h):
        for j in range(w):
            px, py = 16 * j + 8, 16 * i + 8
            mask[i, j] = all((X[order[(k + 1) % 4]] - X[order[k]]) * (py - Y[order[k]])
                             - (Y[order[(k + 1) % 4]] - Y[order[k]]) * (px - X[order[k]]) <= 0 for k in range(4))
    return st, mask


def test_mask_equals_integer_arithmetic():
    """Rows whose coordinates are multiples of 1/8 below 4096, margin 0.  The specification is then exact in fp64: the sum of
    four such numbers and its quarter (a multiple of 1/32) are exact, so cx + 1.0 * (x - cx) gives x back; every difference of a
    pixel centre (a multiple of 1/2) and a corner, and of two corners, is a multiple of 1/8 below 2^13, i.e. at most 16
    significant bits; a product of two of them has at most 32 and the difference of two products at most 33 < 53.  So the
    fp64 test decides exactly what the integers decide -- for every pixel of the frame, also outside the scan's rectangle."""
    from yolov6.utils.redact import row_mask
    h, w = 37, 53
    rows = np.concatenate([quad_rows(h, w, 24, 3, snap=8), quad_rows(h, w, 12, 4, snap=2)])
    # corners exactly on pixel centres and edges through them: the edge belongs to the quad
    rows = np.concatenate([rows, np.zeros((2, 28), np.float32)])
    rows[-2, :12] = [10, 10, 20, 15, 10.5, 10.5, 10.5, 14.5, 19.5, 14.5, 19.5, 10.5]
    rows[-1, :12] = [0, 0, 30, 30, 15.5, 2.5, 3.5, 14.5, 15.5, 26.5, 27.5, 14.5]          # a diamond through pixel centres
    seen = set()
    for row in rows:
        st, mask = row_mask(row, h, w, 0.0)
        ist, imask = integer_mask(row, h, w)
        assert st == ist
        assert np.array_equal(mask, imask)
        seen.add(st)
    assert seen == {1, 2, 3}
    st, mask = row_mask(rows[-2], h, w, 0.0)
    assert st == 1 and mask.sum() == 10 * 5 and mask[10:15, 10:20].all()                   # both border lines of centres included


def test_axis_aligned_box_is_the_cell_mean_in_float64():
    from yolov6.utils.redact import redact_plates_np
    h, w, cell = 37, 53, 8
    frame = frame_of(h, w, 5)
    x1, y1, x2, y2 = 5, 3, 50, 37                       # cuts cells on every side, reaches the clipped last cell row
    det = np.zeros((1, 2, 28), np.float32)
    det[0, 0, :4] = [x1, y1, x2, y2]
    det[0, 0, 4:12] = np.nan
    (out,), status = redact_plates_np([frame], det, [1], 'mosaic', cell, 0.0)
    assert status.tolist() == [[2, 0]]
    want = frame.copy()
    for i in range(y1, y2):
        for j in range(x1, x2):
            ya, xa = i // cell * cell, j // cell * cell
            block = frame[ya:min(ya + cell, h), xa:min(xa + cell, w)].astype(np.float64)
            want[i, j] = np.floor(block.reshape(-1, 3).mean(axis=0) + 0.5)
    assert np.array_equal(out, want)
    changed = (out != frame).any(axis=2)
    assert not changed[:y1].any() and not changed[:, :x1].any() and not changed[:, x2:].any()
    assert changed[y1:y2, x1:x2].mean() > 0.9
    (fill,), _ = redact_plates_np([frame], det, [1], 'fill', cell, 0.0, fill=(1, 2, 3))
    want = frame.copy()
    want[y1:y2, x1:x2] = (1, 2, 3)
    assert np.array_equal(fill, want)


@pytest.mark.parametrize('hw', [(37, 53), (64, 96)])
def test_properties(hw):
    from yolov6.utils.redact import redact_plates_np
    h, w = hw
    frame = frame_of(h, w, 6)
    rows = quad_rows(h, w, 12, 7, snap=8)
    det = rows[None]
    masks = [integer_mask(r, h, w)[1] for r in rows]
    union = np.logical_or.reduce(masks)
    assert sum(m.sum() for m in masks) > union.sum() > 0            # the plates overlap: the hazard is exercised
    for mode in ('mosaic', 'fill'):
        (out,), status = redact_plates_np([frame], det, [12], mode, 8, 0.0, fill=(9, 8, 7))
        assert status[0].tolist() == EXPECTED_STATUS * 2
        assert np.array_equal(out[~union], frame[~union])           # nothing outside the union of the masks
        if mode == 'fill':
            assert (out[union] == (9, 8, 7)).all()
        perm = np.random.default_rng(8).permutation(12)
        (out_p,), status_p = redact_plates_np([frame], det[:, perm], [12], mode, 8, 0.0, fill=(9, 8, 7))
        assert np.array_equal(out_p, out) and np.array_equal(status_p[0], status[0][perm])
        (twice,), _ = redact_plates_np([out], det, [12], mode, 8, 0.0, fill=(9, 8, 7))
        assert np.array_equal(twice[~union], frame[~union])         # the second pass changes only what the first changed
        if mode == 'fill':
            assert np.array_equal(twice, out)
    # a cell wholly inside the plates is a fixed point of the mosaic
    det1 = np.zeros((1, 1, 28), np.float32)
    det1[0, 0, :4] = [0, 0, w, h]
    det1[0, 0, 4:12] = np.nan
    (once,), _ = redact_plates_np([frame], det1, [1], 'mosaic', 8, 0.0)
    (twice,), _ = redact_plates_np([once], det1, [1], 'mosaic', 8, 0.0)
    assert np.array_equal(once, twice) and (once != frame).any()


def test_margin_grows_the_plate_about_its_centre():
    from yolov6.utils.redact import redact_plates_np
    frame = frame_of(40, 60, 9)
    det = np.zeros((1, 1, 28), np.float32)
    det[0, 0, :4] = [20, 10, 40, 20]
    det[0, 0, 4:12] = np.nan
    (out,), _ = redact_plates_np([frame], det, [1], 'fill', 16, 0.5, fill=(0, 0, 0))
    want = frame.copy()
    want[7:23, 15:45] = 0           # centre (30, 15), half sizes 10 x 5 scaled by 1.5: x in [15, 45], y in [7.5, 22.5], edges included
    assert np.array_equal(out, want)


def test_counts_and_argument_checks():
    from yolov6.utils.redact import redact_plates_np
    h, w = 37, 53
    frames = [frame_of(h, w, 10 + b) for b in range(4)]
    det = np.stack([quad_rows(h, w, 6, 20 + b) for b in range(4)])
    outs, status = redact_plates_np(frames, det, [-1, 0, 3, 9], 'mosaic', 4, 0.25)
    assert np.array_equal(outs[0], frames[0]) and np.array_equal(outs[1], frames[1])
    assert status[:2].tolist() == [[0] * 6] * 2 and status[2].tolist() == [1, 1, 1, 0, 0, 0]
    assert status[3].tolist() == EXPECTED_STATUS                     # a count above max_det is max_det
    full, _ = redact_plates_np(frames[3:], det[3:], [6], 'mosaic', 4, 0.25)
    assert np.array_equal(outs[3], full[0])
    three, _ = redact_plates_np(frames[2:3], det[2:3, :3], [3], 'mosaic', 4, 0.25)
    assert np.array_equal(outs[2], three[0]) and (outs[2] != frames[2]).any()
    for kw in (dict(mode='blur'), dict(cell=3), dict(cell=0), dict(cell=66), dict(margin=-0.1), dict(margin=4.5),
               dict(margin=float('nan')), dict(mode='fill', fill=(0, 0, 256))):
        with pytest.raises(ValueError):
            redact_plates_np(frames, det, [1, 1, 1, 1], **kw)
    redact_plates_np(frames, det, [1, 1, 1, 1], mode='fill', cell=3)          # the cell is a mosaic parameter


def test_nv12_planes_and_chroma_any_of_four():
    from yolov6.utils.nv12 import bgr_to_nv12_np
    from yolov6.utils.redact import fill_bytes, redact_plates_np
    h, w = 38, 54
    nv = bgr_to_nv12_np(frame_of(h, w, 30), 'bt709')
    det = np.zeros((1, 2, 28), np.float32)
    det[0, :, 4:12] = np.nan
    det[0, 0, :4] = [5, 3, 6, 4]             # one luma pixel, (3, 5): the odd corner of the block of chroma sample (1, 2)
    det[0, 1, :4] = [20, 10, 31, 17]         # luma [10, 17) x [20, 31): chroma rows 5..8, columns 10..15
    fy, fu, fv = fill_bytes((200, 30, 90), 'bt709')
    (out,), status = redact_plates_np([nv], det, [2], 'fill', 8, 0.0, fill=(200, 30, 90))
    assert status.tolist() == [[2, 2]]
    want_y, want_uv = nv.y.copy(), nv.uv.copy()
    want_y[3, 5] = fy
    want_y[10:17, 20:31] = fy
    want_uv[1, 2] = (fu, fv)
    want_uv[5:9, 10:16] = (fu, fv)
    assert np.array_equal(out.y, want_y) and np.array_equal(out.uv, want_uv)
    assert out.matrix == 'bt709' and np.array_equal(nv.y, bgr_to_nv12_np(frame_of(h, w, 30), 'bt709').y)     # the input is not written
    # mosaic: Y in cells of 8, U and V in cells of 4 samples, float64 means, each plane on its own
    (out,), _ = redact_plates_np([nv], det, [2], 'mosaic', 8, 0.0)
    want_y, want_uv = nv.y.copy(), nv.uv.copy()
    for i, j in [(3, 5)] + [(i, j) for i in range(10, 17) for j in range(20, 31)]:
        ya, xa = i // 8 * 8, j // 8 * 8
        want_y[i, j] = np.floor(nv.y[ya:min(ya + 8, h), xa:min(xa + 8, w)].astype(np.float64).mean() + 0.5)
    for i, j in [(1, 2)] + [(i, j) for i in range(5, 9) for j in range(10, 16)]:
        ya, xa = i // 4 * 4, j // 4 * 4
        block = nv.uv[ya:min(ya + 4, h // 2), xa:min(xa + 4, w // 2)].astype(np.float64)
        want_uv[i, j] = np.floor(block.reshape(-1, 2).mean(axis=0) + 0.5)
    assert np.array_equal(out.y, want_y) and np.array_equal(out.uv, want_uv)
    with pytest.raises(ValueError):
        redact_plates_np([nv, frame_of(h, w, 31)], np.zeros((2, 1, 28), np.float32), [0, 0])     # one kind per call


def test_inferer_redact_cpu_writes_the_files(tmp_path, monkeypatch):
    from PIL import Image
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
    frames = [rng.integers(0, 255, s + (3,), dtype=np.uint8) for s in [(200, 120), (96, 160)]]
    for i, f in enumerate(frames):
        Image.fromarray(f).save(str(img_dir / ('f%d.png' % i)))
    kw = dict(weights=str(ckpt), source=str(img_dir), yaml=None, img_size=[128, 128], conf_thres=0.06, iou_thres=0.45, max_det=20,
              device='cpu', not_save_img=True)
    plain = infer.run(save_dir=str(tmp_path / 'plain'), save_txt=True, **kw)
    assert not (tmp_path / 'plain' / 'redacted').exists()
    for mode, cell in (('mosaic', 8), ('fill', 16)):
        out = tmp_path / mode
        dets = infer.run(save_dir=str(out), redact=mode, redact_cell=cell, redact_margin=0.25, **kw)
        assert sum(len(d) for d in dets) > 0
        for i, (f, d, p) in enumerate(zip(frames, dets, plain)):
            assert torch.equal(d, p)                                 # the detections are what they are without --redact
            det = np.zeros((1, max(len(d), 1), 28), np.float32)
            det[0, :len(d)] = d.numpy()
            (want,), _ = redact_plates_np([f[:, :, ::-1]], det, [len(d)], mode, cell, 0.25)
            got = np.asarray(Image.open(str(out / 'redacted' / ('f%d.png' % i))))
            assert np.array_equal(got, want[:, :, ::-1])
            assert len(d) == 0 or (got != f).any()
    # NV12 frames are redacted as NV12 and converted to be saved
    from yolov6.utils.nv12 import bgr_to_nv12_np, nv12_to_bgr_np
    dets = infer.run(save_dir=str(tmp_path / 'nv'), redact='mosaic', redact_cell=8, nv12='bt601', **kw)
    for i, (f, d) in enumerate(zip(frames, dets)):
        det = np.zeros((1, max(len(d), 1), 28), np.float32)
        det[0, :len(d)] = d.numpy()
        (want,), _ = redact_plates_np([bgr_to_nv12_np(np.ascontiguousarray(f[:, :, ::-1]), 'bt601')], det, [len(d)], 'mosaic', 8, 0.1)
        got = np.asarray(Image.open(str(tmp_path / 'nv' / 'redacted' / ('f%d.png' % i))))
        assert np.array_equal(got, nv12_to_bgr_np(want)[:, :, ::-1])
