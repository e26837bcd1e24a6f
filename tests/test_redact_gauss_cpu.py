"""Gaussian-blur redaction, the specification (yolov6/utils/redact.py: gauss_taps, gauss_blur_np, redact_plates_np(mode='gauss'))
against things that are not the specification: the taps against the float64 Gaussian, the integer blur against a float64 separable
blur with the same weights, the properties the rule promises (nothing outside the masks changes, the order of the rows does not
matter, overlapping rows agree, the pixel set and the status are the mosaic's), NV12 chroma, the counts, the frame's corner, the
sigma errors, and the CPU callers (LookbackNp, Inferer)."""
import importlib
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
import test_lookback_cpu as L
import test_track_cpu as C
from test_redact_cpu import CFG, frame_of, quad_rows

SIGMAS = [0.25, 0.5, 0.6, 0.75, 1, 1.25, 2.5, 4, 8, 10.3, 16]


def float_weights(sigma):
    """(R, g / S): the float64 Gaussian the taps quantise."""
    R = int(math.ceil(3.0 * sigma))
    g = np.exp(-np.arange(R + 1, dtype=np.float64) ** 2 / (2.0 * sigma * sigma))
    return R, g / (g[0] + 2.0 * g[1:].sum())


@pytest.mark.parametrize('sigma', SIGMAS)
def test_taps(sigma):
    from yolov6.utils.redact import MAX_RADIUS, gauss_taps
    q = gauss_taps(sigma)
    R, wgt = float_weights(sigma)
    assert len(q) == R + 1 and 1 <= R <= MAX_RADIUS
    assert int(q[0]) + 2 * int(q[1:].sum()) == 16384
    assert (np.diff(q) <= 0).all() and q.min() >= 0
    assert (np.abs(q[1:] / 16384.0 - wgt[1:]) <= 0.5 / 16384).all()


def test_taps_reject_what_has_no_radius():
    from yolov6.utils.redact import gauss_taps
    for sigma in (0.2, 16.01, float('nan'), 0.0, -1.0):
        with pytest.raises(ValueError):
            gauss_taps(sigma)


def blur_f64(plane, sigma):
    """The separable Gaussian in float64 with the same taps as weights (q / 16384) and the replicate border, unrounded."""
    from yolov6.utils.redact import gauss_taps
    q = gauss_taps(sigma).astype(np.float64) / 16384.0
    R = len(q) - 1
    p = plane.astype(np.float64)
    for axis in (1, 0):
        pad = [(0, 0)] * p.ndim
        pad[axis] = (R, R)
        e = np.pad(p, pad, mode='edge')
        n = p.shape[axis]
        p = sum(q[abs(k)] * np.take(e, np.arange(R + k, R + k + n), axis=axis) for k in range(-R, R + 1))
    return p


def planes_for_accuracy():
    out = []
    for h, w in ((37, 53), (70, 131)):
        rng = np.random.default_rng(h)
        out.append(rng.integers(0, 256, (h, w), dtype=np.uint8))
        out.append((rng.integers(0, 2, (h, w)) * 255).astype(np.uint8))
    return out


@pytest.mark.parametrize('sigma', [0.5, 1.25, 4, 16])
def test_blur_is_the_float_gaussian_within_the_tap_error(sigma):
    """|integer blur - float64 blur of the same weights| <= 0.51 + 1020 R / 16384 (the issue's bound: at most 2 R / 16384 of tap error
    per pass, times 255, over two passes, plus the roundings).  The weights here ARE the taps, so only the roundings remain and the
    bound has room; it is the bound the issue sets."""
    from yolov6.utils.redact import gauss_blur_np, gauss_taps
    taps = gauss_taps(sigma)
    R = len(taps) - 1
    bound = 0.51 + 1020.0 * R / 16384
    worst = 0.0
    for plane in planes_for_accuracy():
        d = np.abs(gauss_blur_np(plane, taps).astype(np.float64) - blur_f64(plane, sigma))
        worst = max(worst, float(d.max()))
    print('sigma %g: R %d, max |d| %.4f, bound %.4f' % (sigma, R, worst, bound))
    assert worst <= bound


def blur_true_gaussian_f64(plane, sigma):
    """As ``blur_f64`` with the float64 Gaussian g / S itself, not the quantised taps."""
    R, wgt = float_weights(sigma)
    p = plane.astype(np.float64)
    for axis in (1, 0):
        pad = [(0, 0)] * p.ndim
        pad[axis] = (R, R)
        e = np.pad(p, pad, mode='edge')
        n = p.shape[axis]
        p = sum(wgt[abs(k)] * np.take(e, np.arange(R + k, R + k + n), axis=axis) for k in range(-R, R + 1))
    return p


@pytest.mark.parametrize('sigma', [0.5, 1.25, 4, 16])
def test_blur_is_the_true_gaussian_within_the_issues_bound(sigma):
    """The same bound against the unquantised Gaussian: this is where the tap error enters."""
    from yolov6.utils.redact import gauss_blur_np, gauss_taps
    taps = gauss_taps(sigma)
    R = len(taps) - 1
    bound = 0.51 + 1020.0 * R / 16384
    worst = 0.0
    for plane in planes_for_accuracy():
        d = np.abs(gauss_blur_np(plane, taps).astype(np.float64) - blur_true_gaussian_f64(plane, sigma))
        worst = max(worst, float(d.max()))
    print('sigma %g: R %d, max |d| %.4f, bound %.4f' % (sigma, R, worst, bound))
    assert worst <= bound


def test_constant_planes_come_out_exact():
    from yolov6.utils.redact import gauss_blur_np, gauss_taps
    for sigma in (0.25, 2.5, 16):
        for v in (0, 1, 127, 128, 254, 255):
            for shape in ((1, 1), (5, 7), (37, 53, 3)):
                assert (gauss_blur_np(np.full(shape, v, np.uint8), gauss_taps(sigma)) == v).all()


def test_channels_are_blurred_separately():
    from yolov6.utils.redact import gauss_blur_np, gauss_taps
    f = frame_of(20, 31, 3)
    taps = gauss_taps(1.25)
    got = gauss_blur_np(f, taps)
    for c in range(3):
        assert np.array_equal(got[:, :, c], gauss_blur_np(np.ascontiguousarray(f[:, :, c]), taps))


def test_stripes_of_period_4_vanish_under_sigma_4():
    from yolov6.utils.redact import gauss_blur_np, gauss_taps
    taps = gauss_taps(4)
    R = len(taps) - 1
    plane = np.zeros((40, 64), np.uint8)
    plane[:, (np.arange(64) % 4) < 2] = 255
    out = gauss_blur_np(plane, taps)[:, R:64 - R]
    assert int(out.max()) - int(out.min()) <= 1 and 126 <= int(out.min()) and int(out.max()) <= 129
    out = gauss_blur_np(np.ascontiguousarray(plane.T), taps)[R:64 - R]
    assert int(out.max()) - int(out.min()) <= 1


# ---- the redaction ---------------------------------------------------------------------------------------------------------------
H, W, N = 70, 131, 12


def scene(seed=40):
    frame = frame_of(H, W, seed)
    rows = quad_rows(H, W, N, seed + 1)
    return frame, rows


@pytest.mark.parametrize('margin', [0.0, 0.25])
def test_only_the_masks_change_and_they_take_the_blurred_frame(margin):
    from yolov6.utils.redact import frame_mask, gauss_blur_np, gauss_taps, redact_frame_np
    frame, rows = scene()
    before = frame.copy()
    out, status = redact_frame_np(frame, rows, 'gauss', margin=margin, sigma=2.5)
    assert np.array_equal(frame, before)                                     # the input is not written
    want_st, mask = frame_mask(rows, H, W, margin)
    assert np.array_equal(status, want_st) and mask.any() and not mask.all()
    assert np.array_equal(out[~mask], frame[~mask])
    assert np.array_equal(out[mask], gauss_blur_np(frame, gauss_taps(2.5))[mask])
    # the pixel set and the status are the mosaic's
    mos, mos_st = redact_frame_np(frame, rows, 'mosaic', 2, margin)
    assert np.array_equal(mos_st, status)
    assert not (mos != frame).any(axis=2)[~mask].any()


def test_row_order_and_overlaps_do_not_matter_and_a_second_call_blurs_again():
    from yolov6.utils.redact import redact_frame_np, row_mask
    frame, rows = scene(50)
    out, status = redact_frame_np(frame, rows, 'gauss', margin=0.25, sigma=2.5)
    perm = np.random.default_rng(5).permutation(N)
    out_p, status_p = redact_frame_np(frame, rows[perm], 'gauss', margin=0.25, sigma=2.5)
    assert np.array_equal(out, out_p) and np.array_equal(status[perm], status_p)
    # overlapping rows: each row alone writes, inside its own mask, the bytes the whole call wrote there
    masks = [row_mask(r, H, W, 0.25)[1] for r in rows]
    assert any((masks[a] & masks[b]).any() for a in range(N) for b in range(a))
    for r, m in zip(rows, masks):
        alone, _ = redact_frame_np(frame, r[None], 'gauss', margin=0.25, sigma=2.5)
        assert np.array_equal(alone[m], out[m])
    # not idempotent: the second call blurs the blurred pixels
    twice, _ = redact_frame_np(out, rows, 'gauss', margin=0.25, sigma=2.5)
    assert (twice != out).any()


def test_default_sigma_is_8_and_other_modes_ignore_it():
    from yolov6.utils.redact import redact_frame_np
    frame, rows = scene(60)
    a, _ = redact_frame_np(frame, rows, 'gauss')
    b, _ = redact_frame_np(frame, rows, 'gauss', sigma=8.0)
    c, _ = redact_frame_np(frame, rows, 'gauss', sigma=2.5)
    assert np.array_equal(a, b) and (a != c).any()
    for mode in ('mosaic', 'fill'):
        assert np.array_equal(redact_frame_np(frame, rows, mode)[0], redact_frame_np(frame, rows, mode, sigma=99.0)[0])


def test_nv12_planes_and_chroma_any_of_four():
    from yolov6.utils.nv12 import bgr_to_nv12_np
    from yolov6.utils.redact import gauss_blur_np, gauss_taps, redact_plates_np
    h, w = 38, 54
    nv = bgr_to_nv12_np(frame_of(h, w, 30), 'bt709')
    det = np.zeros((1, 2, 28), np.float32)
    det[0, :, 4:12] = np.nan
    det[0, 0, :4] = [5, 3, 6, 4]             # one luma pixel, (3, 5): the odd corner of the block of chroma sample (1, 2)
    det[0, 1, :4] = [20, 10, 31, 17]         # luma [10, 17) x [20, 31): chroma rows 5..8, columns 10..15
    (out,), status = redact_plates_np([nv], det, [2], 'gauss', margin=0.0, sigma=1.0)
    assert status.tolist() == [[2, 2]]
    gy = gauss_blur_np(nv.y, gauss_taps(1.0))
    guv = gauss_blur_np(np.ascontiguousarray(nv.uv), gauss_taps(0.5))       # half the sigma, in chroma coordinates
    gu = gauss_blur_np(np.ascontiguousarray(nv.uv[:, :, 0]), gauss_taps(0.5))
    assert np.array_equal(guv[:, :, 0], gu)
    want_y, want_uv = nv.y.copy(), nv.uv.copy()
    want_y[3, 5] = gy[3, 5]
    want_y[10:17, 20:31] = gy[10:17, 20:31]
    want_uv[1, 2] = guv[1, 2]
    want_uv[5:9, 10:16] = guv[5:9, 10:16]
    assert np.array_equal(out.y, want_y) and np.array_equal(out.uv, want_uv)
    assert (out.y != nv.y).any() and (out.uv != nv.uv).any() and out.matrix == 'bt709'


def test_counts_are_clamped():
    from yolov6.utils.redact import redact_frame_np, redact_plates_np
    frames = [frame_of(37, 53, 70 + b) for b in range(4)]
    det = np.stack([quad_rows(37, 53, 6, 80 + b) for b in range(4)])
    outs, status = redact_plates_np(frames, det, [-1, 0, 3, 9], 'gauss', margin=0.1, sigma=1.25)
    assert np.array_equal(outs[0], frames[0]) and np.array_equal(outs[1], frames[1])
    assert not status[:2].any() and not status[2, 3:].any() and status[3].all()
    assert np.array_equal(outs[2], redact_frame_np(frames[2], det[2, :3], 'gauss', margin=0.1, sigma=1.25)[0])
    assert np.array_equal(outs[3], redact_frame_np(frames[3], det[3], 'gauss', margin=0.1, sigma=1.25)[0])
    assert (outs[2] != frames[2]).any() and (outs[3] != frames[3]).any()


def test_a_plate_on_the_corner_uses_the_clamped_halo():
    """A box over the frame's corner: its pixels are the blur of the frame extended by its own border pixels, which is the blur of
    the explicitly padded frame, cut back."""
    from yolov6.utils.redact import gauss_blur_np, gauss_taps, redact_frame_np
    frame = frame_of(20, 30, 90)
    row = np.zeros((1, 28), np.float32)
    row[0, 4:12] = np.nan
    row[0, :4] = [-5, -4, 6, 5]
    out, status = redact_frame_np(frame, row, 'gauss', margin=0.0, sigma=4)
    assert status.tolist() == [2]
    taps = gauss_taps(4)
    R = len(taps) - 1
    padded = np.pad(frame, ((R, R), (R, R), (0, 0)), mode='edge')
    want = gauss_blur_np(padded, taps)[R:R + 20, R:R + 30]
    assert np.array_equal(out[:5, :6], want[:5, :6]) and (out[:5, :6] != frame[:5, :6]).any()
    rest = np.ones((20, 30), bool)
    rest[:5, :6] = False
    assert np.array_equal(out[rest], frame[rest])


def test_sigma_errors():
    from yolov6.utils.lookback import LookbackNp
    from yolov6.utils.redact import check_params, check_sigma, redact_plates_np
    from yolov6.utils.track import PlateTrackerNp
    assert check_sigma(None) == 8.0 and check_sigma(0.5) == 0.5 and check_sigma(16) == 16.0
    assert check_params('gauss', 16, 0.1) == (2, 16, 0.1)
    frames, det = [frame_of(8, 8, 1)], np.zeros((1, 1, 28), np.float32)
    trk = PlateTrackerNp(1)
    trk.enable_hold()
    for sigma in (0.4, 16.5, float('nan')):
        with pytest.raises(ValueError):
            check_sigma(sigma)
        with pytest.raises(ValueError):
            redact_plates_np(frames, det, [0], 'gauss', sigma=sigma)
        with pytest.raises(ValueError):
            LookbackNp(trk, 2, mode='gauss', sigma=sigma)
    redact_plates_np(frames, det, [0], 'mosaic', sigma=99.0)                 # ignored, as the cell is by fill


# ---- the callers -----------------------------------------------------------------------------------------------------------------
def test_lookback_np_blurs_the_frames_before_the_first_detection():
    from yolov6.utils.lookback import LookbackNp
    from yolov6.utils.redact import redact_plates_np
    from yolov6.utils.track import PlateTrackerNp
    bgr, rows, boxes = L.late_plate_frames()
    det, count = C.frames_of(rows, 4)
    kw = dict(mode='gauss', margin=L.MARGIN, sigma=2.5)
    trk = PlateTrackerNp(1, max_tracks=4)
    trk.enable_hold()
    lb = LookbackNp(trk, L.DEPTH, **kw)
    assert lb.sigma == 2.5 and LookbackNp(trk, L.DEPTH, mode='gauss').sigma == 8.0
    got, released = [], []
    for k, f in enumerate(bgr):
        trk.update(det[k:k + 1], count[k:k + 1], [0])
        dh, ch, _ = trk.last_hold
        out = lb.update(dh, ch, trk.last_tid, trk.last_slot, [0], [0])
        if out[2][0] >= 0:
            released.append((int(out[2][0]), out[0][0].copy(), int(out[1][0])))
    # the same chain through push: every frame that leaves carries the specification's bytes for the rows released for it
    trk2 = PlateTrackerNp(1, max_tracks=4)
    trk2.enable_hold()
    lb2 = LookbackNp(trk2, L.DEPTH, **kw)
    for k, f in enumerate(bgr):
        trk2.update(det[k:k + 1], count[k:k + 1], [0])
        got += lb2.push([f], [0])
    assert [g for _, g, _ in got] == [g for g, _, _ in released] and len(got) > 0
    for (_, g, fr), (_, rd, rc) in zip(got, released):
        want = redact_plates_np([bgr[g]], rd[None], [rc], **kw)[0][0]
        assert np.array_equal(fr, want)
    trk2.flush_all()
    got += lb2.flush_all()
    assert [g for _, g, _ in got] == list(range(len(bgr)))
    assert any((got[k][2] != bgr[k]).any() for k in range(L.LATE))          # an early frame's plate is covered


def test_inferer_redact_gauss_cpu_writes_the_files(tmp_path, monkeypatch):
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
    frames = [rng.integers(0, 255, s + (3,), dtype=np.uint8) for s in [(200, 120), (96, 160)]]
    for i, f in enumerate(frames):
        Image.fromarray(f).save(str(img_dir / ('f%d.png' % i)))
    kw = dict(weights=str(ckpt), source=str(img_dir), yaml=None, img_size=[128, 128], conf_thres=0.06, iou_thres=0.45, max_det=20,
              device='cpu', not_save_img=True, redact='gauss', redact_margin=0.25)
    for tag, extra, spec in (('s', dict(redact_sigma=2.5), dict(sigma=2.5)), ('d', dict(), dict(sigma=8.0)),
                             ('n', dict(redact_sigma=2.5, nv12='bt601'), dict(sigma=2.5))):
        dets = infer.run(save_dir=str(tmp_path / tag), **kw, **extra)
        assert sum(len(d) for d in dets) > 0
        for i, (f, d) in enumerate(zip(frames, dets)):
            det = np.zeros((1, max(len(d), 1), 28), np.float32)
            det[0, :len(d)] = d.numpy()
            src = np.ascontiguousarray(f[:, :, ::-1])
            if tag == 'n':
                want = nv12_to_bgr_np(redact_plates_np([bgr_to_nv12_np(src, 'bt601')], det, [len(d)], 'gauss', margin=0.25, **spec)[0][0])
            else:
                want = redact_plates_np([src], det, [len(d)], 'gauss', margin=0.25, **spec)[0][0]
            got = np.asarray(Image.open(str(tmp_path / tag / 'redacted' / ('f%d.png' % i))))
            assert np.array_equal(got, want[:, :, ::-1])
            assert len(d) == 0 or tag == 'n' or (got != f).any()
    with pytest.raises(ValueError):
        infer.run(save_dir=str(tmp_path / 'bad'), **kw, redact_sigma=0.4)
