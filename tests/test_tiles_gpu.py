"""Tiled detection on the GPU, bit for bit: lp_preprocess_tiles_batch against the frame kernel on contiguous copies of the
regions, lp_merge_tiles against merge_tiles_np, detect_tiled against detect_frames (one tile) and against a by-hand composition
(several tiles), detect_tiled_with_crops against plate_crops, and Inferer(tile=...) against detect_tiled."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from test_tiles_cpu import random_case

pytestmark = pytest.mark.gpu

CFG = lambda n: os.path.join(REPO, 'configs', n + '.py')   # noqa: E731
_BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


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


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(_BITS[a.dtype]), b.view(_BITS[b.dtype]))


def _tiles_both(frames, plans, size, dtype, B):
    """(preprocess_tiles on the frames, preprocess_frames on contiguous copies of the regions), both written over NaN."""
    from yolov6.hip import runtime
    got = torch.full((B, 3, size[0], size[1]), float('nan'), dtype=dtype, device='cuda')
    ref = torch.full((B, 3, size[0], size[1]), float('nan'), dtype=dtype, device='cuda')
    copies = [frames[f][y0:y0 + th, x0:x0 + tw].contiguous() for f, y0, x0, th, tw in plans]
    _, g1 = runtime.preprocess_tiles(frames, plans, size, 32, dtype, batch=B, out=got)
    _, g2 = runtime.preprocess_frames(copies, size, 32, dtype, auto=False, batch=B, out=ref)
    torch.cuda.synchronize()
    assert g1 == g2
    return got, ref


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16])
def test_preprocess_tiles_equals_frame_kernel_on_region_copies(dtype):
    from yolov6.core.tiles import plan_frames
    shapes = [(300, 500), (129, 131), (1, 1), (37, 1), (700, 260)]
    for odd in (False, True):
        frames = _frames(shapes, 1 + odd, odd_offsets=odd)
        # 128 x 128 tiles on a 128 x 128 input: interior tiles are the no-resize path; frames smaller than the tile are
        # upscaled; the overviews are downscaled (taps clamp at the region's edges)
        plans = plan_frames(shapes, 128, 32)
        plans += [(0, 299, 499, 1, 1), (0, 0, 0, 1, 100), (4, 3, 5, 100, 1), (1, 1, 1, 127, 129), (0, 7, 11, 200, 333)]   # 1-pixel and odd regions
        got, ref = _tiles_both(frames, plans, [128, 128], dtype, B=len(plans) + 3)      # three padding slots
        assert _bits_equal(got, ref)
        assert bool((got[len(plans):] == (torch.tensor(114.0) / 255).to(dtype)).all())
        # a width that is not a multiple of 4: the per-element store path; resize and no-resize regions
        plans = [(0, 10, 20, 98, 98), (0, 100, 101, 200, 300), (1, 0, 0, 129, 131), (4, 600, 160, 98, 98), (4, 1, 1, 50, 99)]
        got, ref = _tiles_both(frames, plans, [98, 98], dtype, B=len(plans))
        assert got.shape[3] == 98 and _bits_equal(got, ref)


def test_preprocess_tiles_crosses_the_64_tile_split():
    from yolov6.core.tiles import plan_frames
    shapes = [(600, 700), (200, 333)]
    frames = _frames(shapes, 3, odd_offsets=True)
    plans = plan_frames(shapes, (96, 128), 40)
    assert len(plans) > 65
    got, ref = _tiles_both(frames, plans, [96, 128], torch.float16, B=len(plans))
    assert _bits_equal(got, ref)
    got, ref = _tiles_both(frames, plans[:70], [96, 128], torch.float32, B=130)          # 60 padding slots, 3 launches
    assert _bits_equal(got, ref)


# ---- lp_merge_tiles == merge_tiles_np -----------------------------------------------------------------------------------------
def _merge_gpu(det_t, count_t, tiles, shapes, thres, max_det, metric, border):
    """lp_merge_tiles through the ABI with outputs and workspace filled with NaN / 0xff first: (rc, det, count, src)."""
    from yolov6.hip import abi
    lib = abi.load()
    F = len(shapes)
    d_det_t, d_count_t = torch.from_numpy(det_t).cuda(), torch.from_numpy(count_t.astype(np.int32)).cuda()
    det = torch.full((F, max_det, 28), float('nan'), device='cuda')
    count = torch.full((F,), -1, dtype=torch.int32, device='cuda')
    src = torch.full((F, max_det), -7, dtype=torch.int32, device='cuda')
    need = lib.lp_merge_tiles_workspace_bytes(F, max_det)
    ws = torch.full((need + 16,), 0xff, dtype=torch.uint8, device='cuda')
    ref = (abi.TileRef * max(len(tiles), 1))()
    for r, t in zip(ref, tiles):
        r.frame, r.y0, r.x0, r.th, r.tw = t
    hw = (ctypes.c_int * (2 * F))(*[int(v) for s in shapes for v in s[:2]])
    rc = lib.lp_merge_tiles(ctypes.c_void_p(d_det_t.data_ptr()), ctypes.c_void_p(d_count_t.data_ptr()), ref, len(tiles), det_t.shape[1],
                            hw, F, thres, {'iou': 0, 'ios': 1}[metric], border, max_det, ctypes.c_void_p(det.data_ptr()),
                            ctypes.c_void_p(count.data_ptr()), ctypes.c_void_p(src.data_ptr()),
                            ctypes.c_void_p((ws.data_ptr() + 15) // 16 * 16), need, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, det.cpu().numpy(), count.cpu().numpy(), src.cpu().numpy()


def _assert_merge_equal(case, thres, max_det, metric, border):
    from yolov6.utils.tiles import merge_tiles_np
    det_t, count_t, tiles, shapes = case
    rc, det, count, src = _merge_gpu(det_t, count_t, tiles, shapes, thres, max_det, metric, border)
    assert rc == 0
    rdet, rcount, rsrc = merge_tiles_np(det_t, count_t, tiles, shapes, thres, max_det, metric, border)
    assert np.array_equal(count, rcount), (count, rcount)
    assert np.array_equal(src, rsrc)
    assert np.array_equal(det.view(np.int32), rdet.view(np.int32))
    return int(count.sum())


@pytest.mark.parametrize('metric', ['iou', 'ios'])
def test_merge_tiles_equals_numpy_spec(metric):
    total = 0
    for seed in range(6):
        case = random_case(seed)                         # 3 frames with different tile counts, counts out of range, empty tiles
        for border in (-1, 0, 3):
            for thres, max_det in ((0.45, 200), (0.1, 7), (0.0, 50)):
                total += _assert_merge_equal(case, thres, max_det, metric, border)
    assert total > 0
    # a launch split: more than 64 tiles in all, whole frames per launch; and many candidates per chunk
    case = random_case(50, n_frames=9, max_det_t=40, tile=96, overlap=32)
    assert len(case[2]) > 64
    assert _assert_merge_equal(case, 0.45, 300, metric, 1) > 64


def test_merge_tiles_single_tile_and_kept_list_beyond_lds():
    # one tile per frame: the tile's rows unchanged and in order, whatever overlaps
    rng = np.random.default_rng(5)
    det_t = np.zeros((2, 9, 28), np.float32)
    det_t[:, :, :4] = [10, 10, 90, 40]
    det_t[:, :, 12:20] = np.sort(rng.integers(1, 4, (2, 9, 1)), 1)[:, ::-1] / 4.0
    det_t[:, :, 20:] = rng.integers(0, 30, (2, 9, 8))
    count_t = np.array([9, 6], np.int32)
    tiles, shapes = [(0, 0, 0, 100, 120), (1, 0, 0, 50, 100)], [(100, 120), (50, 100)]
    rc, det, count, src = _merge_gpu(det_t, count_t, tiles, shapes, 0.45, 20, 'iou', 1)
    assert rc == 0 and count.tolist() == [9, 6]
    assert np.array_equal(det[0, :9], det_t[0]) and np.array_equal(det[1, :6], det_t[1, :6]) and not det[1, 6:].any()
    assert src[0, :9].tolist() == list(range(9)) and src[1, :6].tolist() == list(range(9, 15)) and (src[1, 6:] == -1).all()
    # 64 tiles x 256 rows = 16384 slots (all of the sort's LDS), thousands of disjoint boxes and zero-area rows kept: the kept
    # list outgrows its LDS share and continues in the workspace, and max_det cuts it; a small second frame (a launch of its own)
    T, mdt = 64, 256
    det_t = np.zeros((T + 1, mdt, 28), np.float32)
    count_t = np.zeros(T + 1, np.int32)
    tiles = [(0, 0, 0, 4000, 4000)] * T + [(1, 0, 0, 50, 50)]
    k = 0
    for t in range(T):
        n = int(rng.integers(30, 65))
        for r in range(n):
            gx, gy = (k % 60) * 64, (k // 60) * 64          # a grid of disjoint cells; every fourth box is repeated in the next tile
            det_t[t, r, :4] = [gx + 2, gy + 2, gx + 60, gy + 40]
            det_t[t, r, 12:20] = rng.integers(1, 9, 8) / 8.0
            k += 1 if (r % 4 or t == T - 1) else 0
            if r % 4 == 0 and t + 1 < T:
                det_t[t + 1, 255 - r // 4, :4] = det_t[t, r, :4]
                det_t[t + 1, 255 - r // 4, 12:20] = det_t[t, r, 12:20]
        count_t[t] = n
    count_t[1:T] = mdt                                       # rows n..255 of tiles 1..: zero boxes (area 0) and the repeated ones
    det_t[T, :3, :4] = [[1, 1, 20, 20], [2, 2, 21, 21], [30, 30, 40, 40]]
    det_t[T, :3, 12] = [4, 2, 6]
    count_t[T] = 3
    n = _assert_merge_equal((det_t, count_t, tiles, [(4000, 4000), (50, 50)]), 0.45, 4000, 'iou', 1)
    assert n > 1300 + 3                                      # more kept rows than the LDS share holds beside 16384 keys


def test_merge_tiles_candidate_cap_error():
    from yolov6.hip import abi
    det_t, count_t = np.zeros((33, 497, 28), np.float32), np.zeros(33, np.int32)
    rc, _, count, _ = _merge_gpu(det_t, count_t, [(0, 0, 0, 64, 64)] * 33, [(64, 64)], 0.45, 10, 'iou', 1)
    assert rc == -1 and b'16401' in abi.load().lp_last_error() and count.tolist() == [-1]      # nothing was launched
    rc, _, count, _ = _merge_gpu(det_t[:, :496], count_t, [(0, 0, 0, 64, 64)] * 33, [(64, 64)], 0.45, 10, 'iou', 1)
    assert rc == 0 and count.tolist() == [0]


# ---- detect_tiled ---------------------------------------------------------------------------------------------------------------
def _tiny(dtype):
    from yolov6.utils.synth import build_synthetic
    return build_synthetic(CFG('yololps'), width=0.0625, sigma=1.5).cuda().to(dtype)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_detect_tiled_one_tile_equals_detect_frames(dtype):
    from yolov6.hip import runtime
    m = _tiny(dtype)
    size, conf, iou, max_det = [256, 256], 0.06, 0.45, 50
    frames = _frames([(232, 144), (256, 256), (97, 131), (1, 1), (200, 256)], 8)
    with torch.no_grad():
        ref = runtime.detect_frames(m, frames, size, conf, iou, max_det, auto=False)
        for kw in (dict(overview=False), dict(tile_hw=(300, 256), overview=True, batch=3), dict(metric='ios', border=0, batch=8)):
            got = runtime.detect_tiled(m, frames, size, conf, iou, max_det, **kw)
            assert len(got) == len(ref)
            for g, r in zip(got, ref):
                assert g.shape == r.shape and torch.equal(g.view(torch.int32), r.view(torch.int32))
    assert sum(len(r) for r in ref) > 0


def test_detect_tiled_one_tile_equals_detect_frames_yololps():
    from yolov6.hip import runtime
    from yolov6.utils.synth import build_synthetic
    m = build_synthetic(CFG('yololps'), sigma=0.25).cuda().half()
    frames = _frames([(640, 640), (480, 600), (300, 640)], 9)
    with torch.no_grad():
        ref = runtime.detect_frames(m, frames, [640, 640], 0.25, 0.45, 300, auto=False)
        got = runtime.detect_tiled(m, frames, [640, 640], 0.25, 0.45, 300, tile_hw=(640, 640), overview=False, batch=4)
    print('yololps detections per frame:', [len(r) for r in ref])
    for g, r in zip(got, ref):
        assert g.shape == r.shape and torch.equal(g.view(torch.int32), r.view(torch.int32))


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_detect_tiled_equals_by_hand_and_crops(dtype):
    from yolov6.core.tiles import plan_frames
    from yolov6.hip import runtime
    from yolov6.utils.tiles import merge_tiles_np
    m = _tiny(dtype)
    size, conf, iou, max_det, B = [128, 128], 0.06, 0.45, 60, 8
    frames = _frames([(300, 420), (200, 150)], 10)
    shapes = [tuple(f.shape[:2]) for f in frames]
    total = 0
    with torch.no_grad():
        for metric, overlap in (('iou', 32), ('ios', 0.25)):
            tiles = plan_frames(shapes, size, overlap)
            assert len(tiles) > 2 * B
            tmd = min(max_det, 16384 // max(sum(1 for t in tiles if t[0] == f) for f in range(2)))
            copies = [frames[f][y0:y0 + th, x0:x0 + tw].contiguous() for f, y0, x0, th, tw in tiles]
            dets, counts = [], []
            for c0 in range(0, len(tiles), B):
                x, _ = runtime.preprocess_frames(copies[c0:c0 + B], size, 32, dtype, auto=False, batch=B)
                det, count, _ = runtime.detect_padded(m, x, conf, iou, tmd)
                dets.append(det)
                counts.append(count)
            det_t, count_t = torch.cat(dets), torch.cat(counts)
            runtime.rescale_round_batch(det_t, count_t, size, [(t[3], t[4]) for t in tiles])
            rdet, rcount, _ = merge_tiles_np(det_t.cpu().numpy(), count_t.cpu().numpy(), tiles, shapes, iou, max_det, metric, 1)
            got = runtime.detect_tiled(m, frames, size, conf, iou, max_det, overlap=overlap, metric=metric, batch=B)
            dets2, crops, status = runtime.detect_tiled_with_crops(m, frames, size, conf, iou, max_det, (24, 72), overlap=overlap,
                                                                   metric=metric, batch=B)
            d_det, d_count = torch.from_numpy(rdet).cuda(), torch.from_numpy(rcount).cuda()
            rc, rs = runtime.plate_crops(frames, d_det, d_count, (24, 72), max_crops=max_det)
            for f in range(2):
                n = int(rcount[f])
                assert got[f].shape == (n, 28) and np.array_equal(got[f].cpu().numpy().view(np.int32), rdet[f, :n].view(np.int32))
                assert torch.equal(dets2[f], got[f])
                assert crops[f].shape == (n, 24, 72, 3) and torch.equal(crops[f], rc[f, :n]) and torch.equal(status[f], rs[f, :n])
                total += n
            # the tiled result is not the per-tile lists glued together: something was merged away or cut
            assert int(count_t[:len(tiles)].clamp(0, tmd).sum()) > int(rcount.sum())
    assert total > 0


def test_infer_tile_matches_detect_tiled(tmp_path, monkeypatch):
    from PIL import Image
    from yolov6.core.inferer import Inferer
    from yolov6.data.datasets import imread_bgr
    from yolov6.hip import runtime
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
    shapes = [(300, 420), (100, 120), (200, 150), (300, 420)]
    for i, (h, w) in enumerate(shapes):
        Image.fromarray(rng.integers(0, 255, (h, w, 3), dtype=np.uint8)).save(str(img_dir / ('f%d.png' % i)))
    kw = dict(weights=str(ckpt), source=str(img_dir), yaml=None, img_size=[128, 128], conf_thres=0.06, iou_thres=0.45, max_det=50,
              device='0', save_txt=True, not_save_img=True, half=True, tile=[128, 128], tile_overlap=32, save_crops=True, crop_size=(16, 48))
    res = {b: infer.run(save_dir=str(tmp_path / ('o%d' % b)), batch_size=b, **kw) for b in (1, 8, 32)}
    model = Inferer(str(img_dir), str(ckpt), '0', None, [128, 128], True).model.model      # the checkpoint as Inferer prepares it
    total = 0
    for i in range(4):
        frame = torch.from_numpy(np.ascontiguousarray(imread_bgr(str(img_dir / ('f%d.png' % i))))).cuda()
        with torch.no_grad():
            want = runtime.detect_tiled(model, [frame], [128, 128], 0.06, 0.45, 50, tile_hw=(128, 128), overlap=32, batch=8)[0]
        for b, out in res.items():
            assert out[i].is_cuda and torch.equal(out[i], want)
            txt = tmp_path / ('o%d' % b) / 'imgs' / ('f%d.txt' % i)
            lines = txt.read_text().strip().splitlines() if txt.exists() else []
            pngs = list((tmp_path / ('o%d' % b) / 'imgs' / 'crops').glob('f%d_*.png' % i))
            assert len(lines) == len(want) == len(pngs)
        total += len(want)
    assert total > 0
