"""Tiled detection, the parts that run without a GPU: the tile plan, the numpy merge (yolov6/utils/tiles.py) against a
loop-by-loop restatement and on planted scenes, argument checks of lp_preprocess_tiles_batch / lp_merge_tiles through the C
ABI, and tools/infer.py --tile on the CPU path."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

LP_ERR_ARG = -1
f32 = np.float32


# ---- plan_tiles -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,tile,overlap', [((2160, 3840), 640, 128), ((700, 1000), (640, 640), 0.2), ((641, 640), 640, 0),
                                                ((1080, 1920), (384, 640), 0.25), ((1300, 777), 256, 255), ((2000, 3000), 640, 0.5)])
def test_plan_tiles_covers_the_frame(shape, tile, overlap):
    from yolov6.core.tiles import plan_tiles
    h, w = shape
    th, tw = (tile, tile) if isinstance(tile, int) else tile
    tiles = plan_tiles(shape, tile, overlap, overview=False)
    cover = np.zeros(shape, np.int32)
    for y0, x0, lh, lw in tiles:
        assert 0 <= y0 and 0 <= x0 and y0 + lh <= h and x0 + lw <= w and lh == min(th, h) and lw == min(tw, w)
        cover[y0:y0 + lh, x0:x0 + lw] += 1
    assert cover.min() >= 1
    for axis, n, t in ((0, h, th), (1, w, tw)):
        ov = int(t * overlap) if isinstance(overlap, float) and overlap < 1 else int(overlap)
        origins = sorted({tl[axis] for tl in tiles})
        assert origins[0] == 0 and origins[-1] == max(0, n - t)
        for a, b in zip(origins, origins[1:]):
            assert a < b and a + t - b >= ov                   # neighbours overlap by at least ov
    assert tiles == sorted(tiles)                               # row-major
    with_overview = plan_tiles(shape, tile, overlap)
    assert with_overview == tiles + [(0, 0, h, w)]


def test_plan_tiles_small_frames_and_overview():
    from yolov6.core.tiles import plan_frames, plan_tiles
    assert plan_tiles((300, 500), 640, 0.2) == [(0, 0, 300, 500)]                 # one tile: no overview
    assert plan_tiles((640, 640, 3), 640, 128) == [(0, 0, 640, 640)]
    assert plan_tiles((300, 1000), 640, 128) == [(0, 0, 300, 640), (0, 360, 300, 640), (0, 0, 300, 1000)]
    assert plan_tiles((300, 1000), 640, 128, overview=False) == [(0, 0, 300, 640), (0, 360, 300, 640)]
    assert len(plan_tiles((2160, 3840), 640, 128)) == 33
    assert plan_frames([(300, 500), (300, 1000)], 640, 128, overview=False) == [(0, 0, 0, 300, 500), (1, 0, 0, 300, 640), (1, 0, 360, 300, 640)]
    for bad in (640, 700, -1):
        with pytest.raises(ValueError):
            plan_tiles((2000, 2000), 640, bad)


# ---- merge_tiles_np against a loop-by-loop restatement ---------------------------------------------------------------------
def _ref_overlap(a, b, thres, metric):
    """a: the earlier (kept) box, b: the candidate; np.float32 scalars, one op at a time."""
    with np.errstate(all='ignore'):
        xx1 = a[0] if a[0] > b[0] else b[0]
        yy1 = a[1] if a[1] > b[1] else b[1]
        xx2 = a[2] if a[2] < b[2] else b[2]
        yy2 = a[3] if a[3] < b[3] else b[3]
        w = f32(xx2 - xx1)
        w = w if w > 0 else f32(0)
        h = f32(yy2 - yy1)
        h = h if h > 0 else f32(0)
        inter = f32(w * h)
        aa = f32(f32(a[2] - a[0]) * f32(a[3] - a[1]))
        ab = f32(f32(b[2] - b[0]) * f32(b[3] - b[1]))
        den = f32(f32(aa + ab) - inter) if metric == 'iou' else (aa if aa < ab else ab)
        return float(f32(inter / den)) > thres


def _ref_merge(det_t, count_t, tiles, shapes, thres, max_det, metric, border):
    F, mdt = len(shapes), det_t.shape[1]
    det, count, src = np.zeros((F, max_det, 28), f32), np.zeros(F, np.int32), np.full((F, max_det), -1, np.int32)
    for f in range(F):
        h, w = shapes[f][:2]
        cands = []
        for t, (ff, y0, x0, th, tw) in enumerate(tiles):
            if ff != f:
                continue
            for r in range(min(max(int(count_t[t]), 0), mdt)):
                row = det_t[t, r].copy()
                x1, y1, x2, y2 = row[:4]
                if border >= 0 and ((x0 > 0 and x1 <= border) or (y0 > 0 and y1 <= border) or (x0 + tw < w and x2 >= tw - border)
                                    or (y0 + th < h and y2 >= th - border)):
                    continue
                for c in range(12):
                    row[c] = f32(row[c] + f32(y0 if c % 2 else x0))
                s = f32(row[12])
                for c in range(13, 20):
                    s = f32(s + row[c])
                cands.append((f32(s / f32(8)), t, r, row))
        order = sorted(range(len(cands)), key=lambda i: -float(cands[i][0]))       # stable: ties in candidate order
        kept = []
        for i in order:
            if not any(cands[k][1] != cands[i][1] and _ref_overlap(cands[k][3], cands[i][3], thres, metric) for k in kept):
                kept.append(i)
        kept = kept[:max_det]
        count[f] = len(kept)
        for j, i in enumerate(kept):
            det[f, j], src[f, j] = cands[i][3], cands[i][1] * mdt + cands[i][2]
    return det, count, src


def random_case(seed, n_frames=3, max_det_t=12, tile=96, overlap=32):
    """Random rounded rows on a random tile plan: clustered boxes (many cross-tile overlaps), scores from a small set (ties),
    empty tiles, counts above max_det_t and below zero."""
    from yolov6.core.tiles import plan_frames
    rng = np.random.default_rng(seed)
    shapes = [(int(rng.integers(60, 330)), int(rng.integers(60, 400))) for _ in range(n_frames)]
    tiles = plan_frames(shapes, tile, overlap, overview=True)
    det_t = np.zeros((len(tiles), max_det_t, 28), f32)
    count_t = np.zeros(len(tiles), np.int32)
    for t, (f, y0, x0, th, tw) in enumerate(tiles):
        mode = rng.integers(0, 8)
        n = 0 if mode == 0 else (max_det_t if mode == 1 else int(rng.integers(1, max_det_t + 1)))
        count_t[t] = -3 if mode == 0 else (max_det_t + 5 if mode == 1 else n)      # below zero / above max_det_t: clamped
        for r in range(max_det_t):          # rows past the count hold data too: they must be ignored
            cx, cy = rng.integers(0, tw + 1), rng.integers(0, th + 1)
            bw, bh = rng.integers(0, 50), rng.integers(0, 30)
            x1, y1, x2, y2 = max(0, cx - bw), max(0, cy - bh), min(tw, cx + bw), min(th, cy + bh)
            det_t[t, r, :4] = [x1, y1, x2, y2]
            det_t[t, r, 4:12] = [x1, y1, x1, y2, x2, y2, x2, y1]
            det_t[t, r, 12:20] = rng.integers(1, 5, 8) / 8.0
            det_t[t, r, 20:] = rng.integers(0, 30, 8)
    return det_t, count_t, tiles, shapes


@pytest.mark.parametrize('metric', ['iou', 'ios'])
@pytest.mark.parametrize('border', [-1, 0, 3])
def test_merge_np_equals_loop_restatement(metric, border):
    from yolov6.utils.tiles import merge_tiles_np
    cut = False
    for seed in range(6):
        det_t, count_t, tiles, shapes = random_case(seed)
        for thres, max_det in ((0.45, 200), (0.1, 7), (0.0, 50)):
            got = merge_tiles_np(det_t, count_t, tiles, shapes, thres, max_det, metric, border)
            ref = _ref_merge(det_t, count_t, tiles, shapes, thres, max_det, metric, border)
            for g, r in zip(got, ref):
                assert g.dtype == r.dtype and np.array_equal(g.view(np.int32), r.view(np.int32))
            cut = cut or bool((got[1] == max_det).any())
            for f in range(len(shapes)):
                assert not got[0][f, got[1][f]:].any() and (got[2][f, got[1][f]:] == -1).all()
    assert cut                                                                     # max_det did cut a list


def test_merge_np_single_tile_returns_rows_unchanged():
    """Rows of one tile never suppress each other: a frame covered by one tile comes out as that tile's rows, in order --
    overlapping rows, equal scores and rows on the border included."""
    from yolov6.utils.tiles import merge_tiles_np
    rng = np.random.default_rng(3)
    det_t = np.zeros((2, 9, 28), f32)
    for t in range(2):
        det_t[t, :, :4] = [10, 10, 90, 40]                                          # all rows the same box
        det_t[t, :, 0] = np.arange(9)                                               # ... touching the left border
        det_t[t, :, 12:20] = np.sort(rng.integers(1, 4, (9, 1)), 0)[::-1] / 4.0     # descending, with ties (as the tile's NMS leaves them)
    count_t = np.array([9, 6], np.int32)
    tiles, shapes = [(0, 0, 0, 100, 120), (1, 0, 0, 50, 100)], [(100, 120), (50, 100)]
    for metric in ('iou', 'ios'):
        det, count, src = merge_tiles_np(det_t, count_t, tiles, shapes, 0.45, 20, metric, border=1)
        assert count.tolist() == [9, 6]
        assert np.array_equal(det[0, :9], det_t[0]) and np.array_equal(det[1, :6], det_t[1, :6])
        assert src[0, :9].tolist() == list(range(9)) and src[1, :6].tolist() == list(range(9, 15))


# ---- a planted scene --------------------------------------------------------------------------------------------------------
def _planted_scene(rng, tile=640, overlap=128, border=1):
    from yolov6.core.tiles import plan_tiles
    h, w = int(rng.integers(700, 2301)), int(rng.integers(700, 4001))
    side = overlap - 2 * border - 2
    boxes = []
    for _ in range(400):
        bw, bh = int(rng.integers(8, side + 1)), int(rng.integers(8, side + 1))
        x1, y1 = int(rng.integers(0, w - bw + 1)), int(rng.integers(0, h - bh + 1))
        b = (x1, y1, x1 + bw, y1 + bh)
        if all(b[2] <= o[0] or o[2] <= b[0] or b[3] <= o[1] or o[3] <= b[1] for o in boxes):
            boxes.append(b)
        if len(boxes) == 40:
            break
    tiles = plan_tiles((h, w), tile, overlap)
    assert tiles[-1] == (0, 0, h, w) and len(tiles) > 4
    det_t = np.zeros((len(tiles), len(boxes), 28), f32)
    count_t = np.zeros(len(tiles), np.int32)
    for t, (y0, x0, th, tw) in enumerate(tiles):
        overview = t == len(tiles) - 1
        n = 0
        for (x1, y1, x2, y2) in boxes:
            cx1, cy1, cx2, cy2 = max(x1, x0), max(y1, y0), min(x2, x0 + tw), min(y2, y0 + th)
            if cx2 <= cx1 or cy2 <= cy1:
                continue
            visible = (cx2 - cx1) * (cy2 - cy1) / ((x2 - x1) * (y2 - y1))
            det_t[t, n, :4] = [cx1 - x0, cy1 - y0, cx2 - x0, cy2 - y0]
            det_t[t, n, 12] = 8 * (0.4 if overview else 0.9 * visible)               # score = c12 / 8
            n += 1
        order = np.argsort(-det_t[t, :n, 12], kind='stable')                        # a tile's rows come in descending score
        det_t[t, :n] = det_t[t, order]
        count_t[t] = n
    return (h, w), boxes, [(0,) + t for t in tiles], det_t, count_t


@pytest.mark.parametrize('metric', ['iou', 'ios'])
def test_planted_scene_every_box_once(metric):
    from yolov6.utils.tiles import merge_tiles_np
    rng = np.random.default_rng(11)
    for _ in range(25):
        shape, boxes, tiles, det_t, count_t = _planted_scene(rng)
        det, count, _ = merge_tiles_np(det_t, count_t, tiles, [shape], 0.45, 1000, metric, border=1)
        got = sorted(tuple(int(v) for v in r[:4]) for r in det[0, :count[0]])
        assert got == sorted(boxes)                                                  # no miss, no duplicate, no clipped view


# ---- C ABI: everything is checked on the host before any launch -------------------------------------------------------------
def _tile_descs(n, **kw):
    from yolov6.hip import abi
    d = (abi.TileDesc * max(n, 1))()
    base = dict(img=0x1000, h0=2160, w0=3840, y0=100, x0=200, th=640, tw=640, rh=640, rw=640, top=0, left=0)
    base.update(kw)
    for e in d:
        for k, v in base.items():
            setattr(e, k, v)
    return d


def test_preprocess_tiles_rejects_bad_arguments_before_launch():
    from yolov6.hip import abi
    lib = abi.load()
    call = lambda d, n, B, dt=2, H=640, W=640, out=0x2000: lib.lp_preprocess_tiles_batch(     # noqa: E731
        d, n, B, ctypes.c_void_p(out) if out else None, dt, H, W, None)
    d = _tile_descs(3)
    assert call(d, 3, 3, out=0) == LP_ERR_ARG and call(d, 3, 2) == LP_ERR_ARG and call(d, 3, 3, dt=5) == LP_ERR_ARG
    assert call(None, 2, 2) == LP_ERR_ARG and call(d, -1, 2) == LP_ERR_ARG and call(d, 1, 1, H=0) == LP_ERR_ARG
    d[1].img = None
    assert call(d, 3, 3) == LP_ERR_ARG and b'tile 1' in lib.lp_last_error()
    for field, v in (('y0', -1), ('x0', -1), ('th', 0), ('tw', 0), ('y0', 2160 - 639), ('x0', 3840 - 639), ('th', 2061), ('h0', 0)):
        d = _tile_descs(3)
        setattr(d[2], field, v)
        assert call(d, 3, 3) == LP_ERR_ARG and b'tile 2' in lib.lp_last_error() and b'inside its frame' in lib.lp_last_error()
    for field, v in (('rh', 0), ('rw', 641), ('top', 1), ('left', -1)):
        d = _tile_descs(2)
        setattr(d[0], field, v)
        assert call(d, 2, 2) == LP_ERR_ARG and b'geometry of tile 0' in lib.lp_last_error()


def test_merge_tiles_rejects_bad_arguments_before_launch():
    from yolov6.hip import abi
    lib = abi.load()
    v = lambda p: ctypes.c_void_p(p) if p else None   # noqa: E731

    def call(tiles, shapes, max_det_t=10, thres=0.45, metric=0, border=1, max_det=100, det_t=0x1000, count_t=0x2000, det=0x3000,
             count=0x4000, src=0x5000, ws=0x6000, ws_bytes=None, n_tiles=None):
        ref = (abi.TileRef * max(len(tiles), 1))()
        for r, t in zip(ref, tiles):
            r.frame, r.y0, r.x0, r.th, r.tw = t
        hw = (ctypes.c_int * max(2 * len(shapes), 1))(*[x for s in shapes for x in s])
        need = lib.lp_merge_tiles_workspace_bytes(len(shapes), max_det)
        return lib.lp_merge_tiles(v(det_t), v(count_t), ref, len(tiles) if n_tiles is None else n_tiles, max_det_t, hw, len(shapes),
                                  thres, metric, border, max_det, v(det), v(count), v(src), v(ws), need if ws_bytes is None else ws_bytes, None)

    good, shapes = [(0, 0, 0, 64, 64), (0, 0, 36, 64, 64), (1, 0, 0, 50, 50)], [(64, 100), (50, 50)]
    assert lib.lp_merge_tiles_workspace_bytes(2, 100) >= 2 * 164 * 24
    for k in ('det_t', 'count_t', 'det', 'count', 'src', 'ws'):
        assert call(good, shapes, **{k: 0}) == LP_ERR_ARG and b'null' in lib.lp_last_error()
    assert call(good, shapes, ws=0x6004) == LP_ERR_ARG and b'aligned' in lib.lp_last_error()
    assert call(good, shapes, ws_bytes=100) == LP_ERR_ARG and b'too small' in lib.lp_last_error()
    assert call(good, shapes, thres=1.5) == LP_ERR_ARG and call(good, shapes, thres=float('nan')) == LP_ERR_ARG
    assert call(good, shapes, metric=2) == LP_ERR_ARG and b'metric' in lib.lp_last_error()
    assert call(good, shapes, max_det=0) == LP_ERR_ARG and call(good, shapes, max_det_t=0) == LP_ERR_ARG
    assert call(good, shapes, n_tiles=-1) == LP_ERR_ARG
    assert call(good, [(64, 100), (0, 50)]) == LP_ERR_ARG and b'frame 1' in lib.lp_last_error()
    # frames out of order / out of range, regions outside the frame
    assert call([good[2], good[0]], shapes) == LP_ERR_ARG and b'tile 1' in lib.lp_last_error()
    assert call([(2, 0, 0, 8, 8)], shapes) == LP_ERR_ARG and b'tile 0' in lib.lp_last_error()
    for bad in ((0, 0, 37, 64, 64), (0, 1, 0, 64, 64), (0, -1, 0, 8, 8), (0, 0, 0, 0, 8)):
        assert call([good[0], bad], shapes) == LP_ERR_ARG and b'tile 1' in lib.lp_last_error() and b'inside its frame' in lib.lp_last_error()
    # the candidate cap and the tile cap, with the numbers
    many = [(0, 0, 0, 64, 64)] * 33
    assert call(many, shapes, max_det_t=497) == LP_ERR_ARG
    msg = lib.lp_last_error()
    assert b'33 tiles' in msg and b'497' in msg and b'16401' in msg and b'16384' in msg
    assert call([(0, 0, 0, 64, 64)] * 65, shapes, max_det_t=1) == LP_ERR_ARG and b'65 tiles' in lib.lp_last_error()
    # nothing to do
    assert call([], []) == 0
    assert call([], [], det=0, count=0, src=0, ws=0, det_t=0, count_t=0) == 0


# ---- tools/infer.py --tile on the CPU path -----------------------------------------------------------------------------------
def test_infer_tile_cpu(tmp_path, monkeypatch):
    from PIL import Image
    from yolov6.core.tiles import plan_tiles
    from yolov6.utils.plate_crop import plate_crops_np
    from yolov6.utils.synth import build_synthetic
    from yolov6.utils.tiles import merge_tiles_np
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    m = build_synthetic(os.path.join(REPO, 'configs', 'yololps.py'), width=0.0625, sigma=1.5)
    ckpt = tmp_path / 'tiny.pt'
    torch.save({'model': m.half(), 'ema': None, 'epoch': 0}, str(ckpt))
    img_dir = tmp_path / 'imgs'
    img_dir.mkdir()
    rng = np.random.default_rng(21)
    frames = {}
    for i, (h, w) in enumerate([(200, 300), (100, 120)]):                           # 2 x 3 tiles + overview; one tile
        frames['f%d' % i] = rng.integers(0, 255, (h, w, 3), dtype=np.uint8)
        Image.fromarray(frames['f%d' % i]).save(str(img_dir / ('f%d.png' % i)))
    out = tmp_path / 'out'
    common = ['--weights', str(ckpt), '--source', str(img_dir), '--yaml', '', '--img-size', '128', '128', '--conf-thres', '0.06',
              '--max-det', '50', '--device', 'cpu', '--save-txt', '--not-save-img']
    monkeypatch.setattr(sys, 'argv', ['infer.py'] + common + ['--save-dir', str(out), '--tile', '128', '128', '--tile-overlap', '32',
                                                              '--merge-metric', 'ios', '--save-crops', '--crop-size', '16', '48'])
    infer.main(infer.get_args_parser())
    # by hand: every tile through the plain (untiled) CLI path as an image of its own, then merge_tiles_np
    total = 0
    for stem, rgb in frames.items():
        tiles = plan_tiles(rgb.shape, (128, 128), 32)
        assert len(tiles) == (7 if stem == 'f0' else 1)
        tdir = tmp_path / ('tiles_' + stem)
        tdir.mkdir()
        for t, (y0, x0, th, tw) in enumerate(tiles):
            Image.fromarray(np.ascontiguousarray(rgb[y0:y0 + th, x0:x0 + tw])).save(str(tdir / ('t%02d.png' % t)))
        res = infer.run(weights=str(ckpt), source=str(tdir), yaml=None, img_size=[128, 128], conf_thres=0.06, iou_thres=0.45, max_det=50,
                        device='cpu', not_save_img=True, fixed_shape=True, save_dir=str(tmp_path / ('o_' + stem)))
        assert len(res) == len(tiles)
        det_t, count_t = np.zeros((len(tiles), 50, 28), f32), np.zeros(len(tiles), np.int32)
        for t, d in enumerate(res):
            det_t[t, :len(d)], count_t[t] = d.float().numpy(), len(d)
        det, count, _ = merge_tiles_np(det_t, count_t, [(0,) + t for t in tiles], [rgb.shape], 0.45, 50, 'ios', 1)
        rows = det[0, :count[0]]
        h, w = rgb.shape[:2]
        txt = out / 'imgs' / (stem + '.txt')
        lines = txt.read_text().strip().splitlines() if txt.exists() else []
        assert len(lines) == len(rows)
        gn = np.array([w, h, w, h], np.float32)
        for line, r in zip(lines, torch.from_numpy(rows)):
            xywh = (torch.tensor([[(r[0] + r[2]) / 2, (r[1] + r[3]) / 2, r[2] - r[0], r[3] - r[1]]]) / torch.from_numpy(gn)).view(-1).tolist()
            want = (*r[20:].tolist(), *xywh, *(r[4:12] / torch.from_numpy(np.tile(gn[:2], 4))).tolist())
            assert line == ('%g ' * len(want)).rstrip() % want
        pngs = sorted((out / 'imgs' / 'crops').glob(stem + '_*.png'))
        assert len(pngs) == len(rows)
        if len(rows):
            crops, _ = plate_crops_np(rgb[:, :, ::-1], rows, (16, 48))
            for k in range(len(rows)):
                png = np.asarray(Image.open(str(out / 'imgs' / 'crops' / ('%s_%d.png' % (stem, k)))))
                assert np.array_equal(png, crops[k][:, :, ::-1])
        total += len(rows)
    assert total >= 1
    # without --tile nothing changes: the same call as before the flag existed
    plain = infer.run(weights=str(ckpt), source=str(img_dir), yaml=None, img_size=[128, 128], conf_thres=0.06, iou_thres=0.45, max_det=50,
                      device='cpu', not_save_img=True, save_dir=str(tmp_path / 'plain'))
    assert len(plain) == 2
