"""NV12 frames on the GPU, every comparison on bit patterns: lp_nv12_to_bgr_batch against nv12_to_bgr_np (every (Y, U, V), odd
addresses, pitches, tails), lp_preprocess_nv12_batch against the BGR kernels on the converted frame and against the numpy
definitions (whole frames and regions), the runtime entry points on NV12 frames against the same calls on the converted
frames, graph capture, and the host-side argument checks."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import REPO
from test_nv12_cpu import BAD_GEOMETRY, BAD_PLANES, BAD_REGIONS, LP_ERR_ARG, NAMES

pytestmark = pytest.mark.gpu

CFG = lambda n: REPO + '/configs/' + n + '.py'   # noqa: E731
_BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
DTYPES = [torch.float32, torch.float16, torch.bfloat16]


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(_BITS[a.dtype]), b.view(_BITS[b.dtype]))


def _host_frame(h, w, seed, matrix):
    """Random planes: every byte value, in and out of gamut."""
    from yolov6.utils.nv12 import Nv12Frame
    rng = np.random.default_rng(seed)
    return Nv12Frame(rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2, 2), dtype=np.uint8), matrix)


def _place(f, extra_y=0, extra_uv=0, y_mod=(1, 2), uv_mod=(2, 4)):
    """The host frame on the device inside one 0xEE-filled buffer: rows ``extra`` bytes longer than w, y at an address that is
    y_mod[0] modulo y_mod[1], uv at one that is uv_mod[0] modulo uv_mod[1]."""
    from yolov6.utils.nv12 import Nv12Frame
    py, puv = f.w + extra_y, f.w + extra_uv
    buf = torch.full((f.h * py + (f.h // 2) * puv + 64,), 0xEE, dtype=torch.uint8, device='cuda')
    base = buf.data_ptr()
    oy = (y_mod[0] - base) % y_mod[1]
    ouv = oy + f.h * py
    ouv += (uv_mod[0] - (base + ouv)) % uv_mod[1]
    y = torch.as_strided(buf, (f.h, f.w), (py, 1), oy)
    uv = torch.as_strided(buf, (f.h // 2, f.w // 2, 2), (puv, 2, 1), ouv)
    y.copy_(torch.from_numpy(f.y))
    uv.copy_(torch.from_numpy(f.uv))
    d = Nv12Frame(y, uv, f.matrix)
    assert y.data_ptr() % y_mod[1] == y_mod[0] and uv.data_ptr() % uv_mod[1] == uv_mod[0] and (d.pitch_y, d.pitch_uv) == (py, puv)
    return d


def _odd_out(f):
    """A [h,w,3] uint8 view at an odd address of a 0xAB-filled buffer."""
    buf = torch.full((f.h * f.w * 3 + 2,), 0xAB, dtype=torch.uint8, device='cuda')
    o = 1 - buf.data_ptr() % 2
    out = buf[o:o + f.h * f.w * 3].view(f.h, f.w, 3)
    assert out.data_ptr() % 2 == 1
    return out


def _bgr_dev(f):
    from yolov6.utils.nv12 import nv12_to_bgr_np
    return torch.from_numpy(nv12_to_bgr_np(f)).cuda()


# ---- 1. the convert kernel on every (Y, U, V) -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _all_triples():
    """One 4096 x 4096 frame holding every (Y, U, V): chroma site s = 2048 r + c has the pair s >> 6, and its 2 x 2 luma block
    the four values 4 (s & 63) + 2 a + b."""
    s = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
    pair = s >> 6
    uv = np.stack([pair & 255, pair >> 8], -1).astype(np.uint8)
    k4 = ((s & 63) * 4).astype(np.uint8)
    y = np.empty((4096, 4096), np.uint8)
    for a in (0, 1):
        for b in (0, 1):
            y[a::2, b::2] = k4 + 2 * a + b
    return y, uv


@pytest.mark.parametrize('name', NAMES)
def test_convert_every_triple(name):
    from yolov6.hip import runtime
    from yolov6.utils.nv12 import Nv12Frame, nv12_to_bgr_np
    y, uv = _all_triples()
    host = Nv12Frame(y, uv, name)
    want = torch.from_numpy(nv12_to_bgr_np(host)).cuda()
    dev = Nv12Frame(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda(), name)
    out = torch.full((4096, 4096, 3), 0xAB, dtype=torch.uint8, device='cuda')
    got = runtime.nv12_to_bgr([dev], out=[out])[0]
    assert got is out and torch.equal(got, want)
    assert len(torch.unique(want)) == 256                           # the frame is not degenerate


# ---- 2. the convert kernel: shapes, pitches, alignments --------------------------------------------------------------------------
def test_convert_shapes_pitches_alignments():
    from yolov6.hip import runtime
    from yolov6.utils.nv12 import nv12_to_bgr_np
    sizes = [(2, 2), (4, 6), (34, 70), (64, 192)]
    hosts = [_host_frame(h, w, 10 + i, NAMES[i % 4]) for i, (h, w) in enumerate(sizes)]
    # byte paths: y at an odd address, uv at 2 mod 4, rows longer than w, out at an odd address
    devs = [_place(f, extra_y=3, extra_uv=6) for f in hosts]
    outs = [_odd_out(f) for f in hosts]
    got = runtime.nv12_to_bgr(devs, out=outs)
    for f, g in zip(hosts, got):
        assert torch.equal(g.cpu(), torch.from_numpy(nv12_to_bgr_np(f))), f.shape
    # vector paths: 8-byte aligned planes and pitches (a 6-pixel tail at w = 70), out aligned by the allocator
    devs = [_place(f, extra_y=(-f.w) % 8, extra_uv=(-f.w) % 8 + 8, y_mod=(0, 8), uv_mod=(0, 8)) for f in hosts]
    got = runtime.nv12_to_bgr(devs)
    for f, g in zip(hosts, got):
        assert g.data_ptr() % 8 == 0 and torch.equal(g.cpu(), torch.from_numpy(nv12_to_bgr_np(f))), f.shape
    # mixed alignment: vector luma loads, 16-bit chroma loads, byte stores
    devs = [_place(f, extra_y=(-f.w) % 8, extra_uv=2, y_mod=(0, 8), uv_mod=(2, 4)) for f in hosts]
    got = runtime.nv12_to_bgr(devs, out=[_odd_out(f) for f in hosts])
    for f, g in zip(hosts, got):
        assert torch.equal(g.cpu(), torch.from_numpy(nv12_to_bgr_np(f))), f.shape


def test_convert_seventy_frames_mixed_matrices():
    from yolov6.hip import runtime
    from yolov6.utils.nv12 import nv12_to_bgr_np
    hosts = [_host_frame(2 + 2 * (i % 3), 2 + 2 * (i % 5), 100 + i, NAMES[i % 4]) for i in range(70)]      # two launches
    got = runtime.nv12_to_bgr([_place(f, extra_y=i % 3, extra_uv=2 * (i % 2)) for i, f in enumerate(hosts)])
    for i, (f, g) in enumerate(zip(hosts, got)):
        assert torch.equal(g.cpu(), torch.from_numpy(nv12_to_bgr_np(f))), i


# ---- 3. the fused letterbox ---------------------------------------------------------------------------------------------------
def _nan_out(B, H, W, dtype, misalign=False):
    """[B,3,H,W] filled with NaN; ``misalign``: a view one element into a larger buffer (its base is not 16-byte aligned)."""
    n = B * 3 * H * W
    flat = torch.full((n + 8,), float('nan'), dtype=dtype, device='cuda')
    o = 1 if misalign else 0
    out = flat[o:o + n].view(B, 3, H, W)
    assert (out.data_ptr() % 16 != 0) == misalign
    return out


def _letterbox_three_ways(hosts, size, dtype, B, misalign=False, place=True):
    """(fused kernel on the NV12 frames, BGR kernel on the uploaded converted frames, numpy definition), [B,3,H,W] each."""
    from yolov6.hip import runtime
    from yolov6.utils.nv12 import letterbox_nv12_np
    H, W = size
    devs = [_place(f, extra_y=i % 4, extra_uv=2 * (i % 3)) if place else f.to('cuda') for i, f in enumerate(hosts)]
    got, g1 = runtime.preprocess_frames(devs, size, 32, dtype, auto=False, batch=B, out=_nan_out(B, H, W, dtype, misalign))
    ref, g2 = runtime.preprocess_frames([_bgr_dev(f) for f in hosts], size, 32, dtype, auto=False, batch=B, out=_nan_out(B, H, W, dtype, misalign))
    assert g1 == g2
    spec = torch.full((B, 3, H, W), 114.0) / 255
    for b, f in enumerate(hosts):
        spec[b] = torch.from_numpy(letterbox_nv12_np(f, size, 32, auto=False))
    torch.cuda.synchronize()
    return got, ref, spec.to(dtype).cuda()


@pytest.mark.parametrize('dtype', DTYPES)
def test_fused_letterbox_equals_bgr_kernel_and_numpy(dtype):
    # downscale, upscale (the taps clamp on both edges), no resize, a 2 x 2 frame; mixed matrices; two padding slots
    hosts = [_host_frame(70, 126, 1, 'bt601'), _host_frame(6, 10, 2, 'bt709'), _host_frame(64, 64, 3, 'bt601f'), _host_frame(2, 2, 4, 'bt709f')]
    got, ref, spec = _letterbox_three_ways(hosts, [64, 64], dtype, B=6)
    assert _bits_equal(got, ref) and _bits_equal(got, spec)
    assert bool((got[4:] == (torch.tensor(114.0) / 255).to(dtype)).all())
    # W = 30 and an out base that is not 16-byte aligned: the scalar-store path; a resized and an unresized frame
    hosts = [_host_frame(70, 126, 5, 'bt709'), _host_frame(32, 30, 6, 'bt601')]
    got, ref, spec = _letterbox_three_ways(hosts, [32, 30], dtype, B=2, misalign=True)
    assert got.shape[3] == 30 and _bits_equal(got, ref) and _bits_equal(got, spec)


def test_fused_letterbox_seventy_frames():
    hosts = [_host_frame(4, 4, 200 + i, NAMES[i % 4]) for i in range(70)]             # three launches of 32 slots
    got, ref, spec = _letterbox_three_ways(hosts, [64, 64], torch.float16, B=70, place=False)
    assert _bits_equal(got, ref) and _bits_equal(got, spec)
    got, ref, spec = _letterbox_three_ways(hosts[:33], [64, 64], torch.float32, B=66, place=False)   # 33 padding slots over 3 launches
    assert _bits_equal(got, ref) and _bits_equal(got, spec)


# ---- 4. regions -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_regions_equal_region_copies_of_the_converted_frame(dtype):
    from yolov6.hip import runtime
    from yolov6.utils.nv12 import region_nv12_np
    host = _host_frame(20, 36, 7, 'bt709')
    dev, bgr = _place(host, extra_y=5, extra_uv=4), _bgr_dev(host)
    # odd y0 and x0 together, a single pixel at (1, 1), the bottom-right 3 x 5, the whole frame
    plans = [(0, 3, 5, 11, 17), (0, 1, 1, 1, 1), (0, 17, 31, 3, 5), (0, 0, 0, 20, 36), (0, 1, 0, 19, 36), (0, 0, 1, 20, 35)]
    B = len(plans) + 1
    for size in ([64, 64], [20, 36], [11, 17]):                                  # resized; the whole frame / the first region unresized
        H, W = size
        got, g1 = runtime.preprocess_tiles([dev], plans, size, 32, dtype, batch=B, out=_nan_out(B, H, W, dtype))
        copies = [bgr[y0:y0 + th, x0:x0 + tw].contiguous() for _, y0, x0, th, tw in plans]
        ref, g2 = runtime.preprocess_frames(copies, size, 32, dtype, auto=False, batch=B, out=_nan_out(B, H, W, dtype))
        assert g1 == g2 and _bits_equal(got, ref)
        spec = torch.full((B, 3, H, W), 114.0) / 255
        for k, (_, y0, x0, th, tw) in enumerate(plans):
            spec[k] = torch.from_numpy(region_nv12_np(host, y0, x0, th, tw, size, 32))
        assert _bits_equal(got, spec.to(dtype).cuda())


@functools.lru_cache(maxsize=1)
def _one_region_list():
    """(host frames, 33 regions of them, their numpy definition [34,3,32,32] fp32): two 64 x 96 frames into 32 x 32.  33 slots
    cross the 32-slot split of the NV12 table and stay inside the 64-slot one of the BGR table; the special regions sit on both
    sides of the split."""
    from yolov6.utils.nv12 import region_nv12_np
    hosts = [_host_frame(64, 96, 31, 'bt709'), _host_frame(64, 96, 32, 'bt601')]
    rng = np.random.default_rng(33)
    plans = [(1, 5, 7, 1, 1),                   # a single pixel: every tap clamps onto it
             (0, 11, 95, 40, 1),                # one pixel wide, at the frame's right edge
             (1, 3, 9, 32, 20),                 # ratio 1: unresized (th, tw == rh, rw), odd origin, padded left and right
             (0, 0, 0, 64, 96)]                 # the whole frame
    while len(plans) < 31:
        th, tw = int(rng.integers(2, 65)), int(rng.integers(2, 97))      # >= 2: every region letterboxes to rh, rw >= 1
        plans.append((len(plans) % 2, int(rng.integers(0, 65 - th)), int(rng.integers(0, 97 - tw)), th, tw))
    plans += [(0, 62, 1, 2, 95),                # slot 31: two rows at the bottom edge, resized to one
              (1, 31, 63, 32, 32)]              # slot 32, past the split: unresized, odd (y0, x0), touching the bottom-right corner
    spec = torch.full((34, 3, 32, 32), 114.0) / 255
    for k, (f, y0, x0, th, tw) in enumerate(plans):
        spec[k] = torch.from_numpy(region_nv12_np(hosts[f], y0, x0, th, tw, [32, 32], 32))
    return hosts, plans, spec


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
def test_one_region_list_through_both_sources_of_the_letterbox_kernel(dtype):
    """The same regions through ``preprocess_tiles`` on the BGR frames and on their NV12 form: equal bytes, and the BGR result
    equals ``region_nv12_np`` -- the numpy specification is the anchor, not the other source of the kernel."""
    from yolov6.hip import runtime
    hosts, plans, spec = _one_region_list()
    assert len(plans) == 33 and any((th, tw) == (32, 32) for *_, th, tw in plans)
    B = 34                                                                            # one padding slot
    bgr, g1 = runtime.preprocess_tiles([_bgr_dev(f) for f in hosts], plans, [32, 32], 32, dtype, batch=B, out=_nan_out(B, 32, 32, dtype))
    nv, g2 = runtime.preprocess_tiles([_place(f, extra_y=3, extra_uv=2) for f in hosts], plans, [32, 32], 32, dtype, batch=B,
                                      out=_nan_out(B, 32, 32, dtype))
    assert g1 == g2 and g1[2] == (32, 20, 0, 6) and g1[32] == (32, 32, 0, 0)             # the unresized regions are unresized
    assert _bits_equal(bgr, spec.to(dtype).cuda())
    assert _bits_equal(nv, bgr)


# ---- 5. the runtime entry points --------------------------------------------------------------------------------------------------
def _tiny(dtype):
    from yolov6.utils.synth import build_synthetic
    return build_synthetic(CFG('yololps'), width=0.0625, sigma=1.5).cuda().to(dtype)


def _encoded(shapes, seed):
    """Host NV12 frames encoded from seeded BGR noise, matrices in turn."""
    from yolov6.utils.nv12 import bgr_to_nv12_np
    rng = np.random.default_rng(seed)
    return [bgr_to_nv12_np(rng.integers(0, 256, s + (3,), dtype=np.uint8), NAMES[i % 4]) for i, s in enumerate(shapes)]


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8) if a.dtype != torch.uint8 else a,
                                                                      b.view(torch.uint8) if b.dtype != torch.uint8 else b)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_detect_entry_points_equal_the_calls_on_converted_frames(dtype):
    from yolov6.hip import runtime
    m = _tiny(dtype)
    size, conf, iou, max_det = [256, 256], 0.06, 0.45, 50
    total = 0
    with torch.no_grad():
        for shapes, auto, batch in (([(464, 288)] * 3 + [(232, 144)], True, None), ([(464, 288), (300, 500), (98, 132), (256, 256), (2, 2)], False, 8)):
            hosts = _encoded(shapes, 8)
            nv, bgr = [f.to('cuda') for f in hosts], [_bgr_dev(f) for f in hosts]
            got = runtime.detect_frames(m, nv, size, conf, iou, max_det, auto=auto, batch=batch)
            ref = runtime.detect_frames(m, bgr, size, conf, iou, max_det, auto=auto, batch=batch)
            assert len(got) == len(ref) == len(hosts) and all(_same(g, r) for g, r in zip(got, ref))
            total += sum(len(r) for r in ref)
            gd, gc, gs = runtime.detect_frames_with_crops(m, nv, size, conf, iou, max_det, (24, 72), auto=auto, batch=batch)
            rd, rc, rs = runtime.detect_frames_with_crops(m, bgr, size, conf, iou, max_det, (24, 72), auto=auto, batch=batch)
            for g, r in zip(gd + gc + gs, rd + rc + rs):
                assert _same(g, r)
            assert all(_same(g, r) for g, r in zip(gd, ref))
        hosts = _encoded([(300, 420), (200, 150)], 10)
        nv, bgr = [f.to('cuda') for f in hosts], [_bgr_dev(f) for f in hosts]
        got = runtime.detect_tiled(m, nv, [128, 128], conf, iou, 60, overlap=32, batch=8)
        ref = runtime.detect_tiled(m, bgr, [128, 128], conf, iou, 60, overlap=32, batch=8)
        assert all(_same(g, r) for g, r in zip(got, ref)) and sum(len(r) for r in ref) > 0
        gd, gc, gs = runtime.detect_tiled_with_crops(m, nv, [128, 128], conf, iou, 60, (16, 48), overlap=32, batch=8)
        rd, rc, rs = runtime.detect_tiled_with_crops(m, bgr, [128, 128], conf, iou, 60, (16, 48), overlap=32, batch=8)
        for g, r in zip(gd + gc + gs, rd + rc + rs):
            assert _same(g, r)
        with pytest.raises(ValueError, match='one kind'):
            runtime.detect_frames(m, [nv[0], bgr[1]], size, conf, iou, max_det, auto=False)
    assert total > 0


def test_update_with_shots_on_nv12_frames_over_three_calls():
    from yolov6.hip import runtime
    m = _tiny(torch.float16)
    size, conf, iou, max_det = [256, 256], 0.06, 0.45, 20
    kw = dict(max_tracks=32, match_thres=0.3, new_thres=0.0, expand=0.5, max_age=0, ncls=m, device='cuda')
    a, b = runtime.PlateTracker(2, **kw), runtime.PlateTracker(2, **kw)
    for t in (a, b):
        t.enable_best_shot((16, 48), max_crops=8)
    shots = 0
    with torch.no_grad():
        for call in range(3):
            hosts = _encoded([(232, 144), (98, 132)], 30 + call)
            nv, bgr = [f.to('cuda') for f in hosts], [_bgr_dev(f) for f in hosts]
            det, count = runtime.detect_frames_padded(m, bgr, size, conf, iou, max_det, auto=False)
            flush = [1, 1] if call == 2 else None                                  # the last call ends every live track
            got = [t.clone() for t in a.update_with_shots(nv, det, count, [0, 1], flush)]
            ref = [t.clone() for t in b.update_with_shots(bgr, det, count, [0, 1], flush)]
            assert len(got) == len(ref) == 9
            for k, (g, r) in enumerate(zip(got, ref)):
                assert _same(g, r), (call, k)
            for g, r in zip(a.shot_buffers(2)[:3], b.shot_buffers(2)[:3]):         # the crops both galleries chose from
                assert _same(g, r), call
            shots += int(ref[6][..., 3].sum())
    assert shots > 0 and torch.equal(a._shots['state'], b._shots['state'])


def test_frame_batcher_put_of_nv12_frames():
    from yolov6.core.frames import FrameBatcher
    from yolov6.hip import runtime
    from yolov6.utils.nv12 import Nv12Frame
    batches = [_encoded([(232, 144), (98, 132), (2, 2)], 40 + k) for k in range(3)]
    wide = np.zeros((232 * 3 // 2, 160), np.uint8)                                  # a pitched host frame: put packs it
    wide[:, :144] = batches[1][0].packed()
    batches[1][0] = Nv12Frame(wide[:232, :144], np.lib.stride_tricks.as_strided(wide[232:], (116, 72, 2), (160, 2, 1)), 'bt601')
    batcher = FrameBatcher('cuda:0')
    outs = []
    for hosts in batches:                                                            # back to back, no host sync in between
        devs = batcher.put(hosts)
        assert all(d.is_cuda and d.matrix == h.matrix and d.y.data_ptr() % 256 == 0 for d, h in zip(devs, hosts))
        outs.append((devs, runtime.preprocess_frames(devs, [64, 64], 32, torch.float16, auto=False)[0]))
    for k, (hosts, (devs, x)) in enumerate(zip(batches, outs)):
        alone = runtime.preprocess_frames([h.to('cuda') for h in hosts], [64, 64], 32, torch.float16, auto=False)[0]
        assert _bits_equal(x, alone), k
    for d, h in zip(outs[-1][0], batches[-1]):                                       # the last batch is still in its slot
        assert np.array_equal(d.y.cpu().numpy(), h.y) and np.array_equal(d.uv.cpu().numpy(), h.uv)
    with pytest.raises(ValueError, match='one kind'):
        batcher.put([batches[0][0], np.zeros((4, 4, 3), np.uint8)])


def test_infer_nv12_matches_infer_on_the_converted_frames(tmp_path, monkeypatch):
    """tools/infer.py --nv12 on a GPU (images encoded on the host, and a raw .nv12 stream of the same frames) against plain runs
    on the converted frames saved as images: batched with crops, tiled, and tracked with best shots."""
    import importlib
    import sys
    from PIL import Image
    from yolov6.utils.nv12 import bgr_to_nv12_np, nv12_to_bgr_np
    from yolov6.utils.synth import build_synthetic
    monkeypatch.chdir(REPO)
    sys.path.insert(0, REPO + '/tools')
    infer = importlib.import_module('infer')
    m = build_synthetic(CFG('yololps'), width=0.0625, sigma=1.5)
    ckpt = tmp_path / 'tiny.pt'
    torch.save({'model': m.half(), 'ema': None}, str(ckpt))
    rng = np.random.default_rng(12)
    src, conv, raw = tmp_path / 'src', tmp_path / 'conv', tmp_path / 'raw'
    for d in (src, conv, raw):
        d.mkdir()
    packed = []
    for i in range(5):
        rgb = rng.integers(0, 255, (232, 144, 3), dtype=np.uint8)
        Image.fromarray(rgb).save(str(src / ('f%d.png' % i)))
        f = bgr_to_nv12_np(np.ascontiguousarray(rgb[:, :, ::-1]), 'bt601')
        packed.append(f.packed())
        Image.fromarray(np.ascontiguousarray(nv12_to_bgr_np(f)[:, :, ::-1])).save(str(conv / ('f%d.png' % i)))
    np.concatenate(packed).tofile(str(raw / 'clip.nv12'))
    kw = dict(weights=str(ckpt), yaml=None, img_size=[128, 128], conf_thres=0.06, iou_thres=0.45, max_det=20, device='0', save_txt=True,
              not_save_img=True, half=True, crop_size=(16, 48))
    nv = dict(nv12='bt601', nv12_size=(144, 232))

    def same_files(a, b, pattern):
        fa, fb = sorted(p.name for p in a.glob(pattern)), sorted(p.name for p in b.glob(pattern))
        assert fa == fb and fa, (pattern, fa, fb)
        for n in fa:
            assert (a / n).read_bytes() == (b / n).read_bytes(), n

    for tag, opts in (('crops', dict(batch_size=4, save_crops=True)), ('tile', dict(batch_size=8, tile=[64, 64], tile_overlap=16, fixed_shape=True)),
                      ('one', dict(batch_size=1))):
        want = infer.run(source=str(conv), save_dir=str(tmp_path / ('w_' + tag)), **kw, **opts)
        assert len(want) == 5 and sum(len(d) for d in want) > 0
        if tag != 'tile':           # images, encoded on the host
            got = infer.run(source=str(src), save_dir=str(tmp_path / ('g_' + tag)), **kw, **opts, **nv)
            assert len(got) == 5 and all(b.is_cuda and torch.equal(a, b) for a, b in zip(want, got)), tag
            same_files(tmp_path / ('w_' + tag) / 'conv', tmp_path / ('g_' + tag) / 'src', '*.txt')
        if tag != 'one':            # the raw stream of the same frames
            stream = infer.run(source=str(raw), save_dir=str(tmp_path / ('s_' + tag)), **kw, **opts, **nv)
            assert len(stream) == 5 and all(c.is_cuda and torch.equal(a, c) for a, c in zip(want, stream)), tag
        if tag == 'crops':
            same_files(tmp_path / 'w_crops' / 'conv' / 'crops', tmp_path / 'g_crops' / 'src' / 'crops', '*.png')
    opts = dict(batch_size=2, track=True, best_shots=True, track_max_age=0)
    want = infer.run(source=str(conv), save_dir=str(tmp_path / 'w_trk'), **kw, **opts)
    got = infer.run(source=str(src), save_dir=str(tmp_path / 'g_trk'), **kw, **opts, **nv)
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    for name in ('plates.txt', 'shots.txt'):
        assert (tmp_path / 'w_trk' / name).read_bytes() == (tmp_path / 'g_trk' / name).read_bytes() and (tmp_path / 'w_trk' / name).stat().st_size > 0
    same_files(tmp_path / 'w_trk' / 'shots', tmp_path / 'g_trk' / 'shots', '*.png')


# ---- 6. capture -----------------------------------------------------------------------------------------------------------------
def test_nv12_calls_are_capturable():
    """preprocess_frames on NV12 plus nv12_to_bgr into persistent buffers in one graph on one stream: two replays, the frame
    bytes changed in between, both bit-exact."""
    from yolov6.hip import runtime
    from yolov6.utils.nv12 import Nv12Frame, letterbox_nv12_np, nv12_to_bgr_np
    shapes = [(70, 126), (64, 64)]
    bufs = [torch.zeros(h * w * 3 // 2, dtype=torch.uint8, device='cuda') for h, w in shapes]
    devs = [Nv12Frame.from_packed(b, h, w, 'bt709') for b, (h, w) in zip(bufs, shapes)]
    x = torch.full((3, 3, 64, 64), float('nan'), dtype=torch.float16, device='cuda')
    bgr = [torch.full((h, w, 3), 0xAB, dtype=torch.uint8, device='cuda') for h, w in shapes]
    runtime.preprocess_frames(devs, [64, 64], 32, torch.float16, auto=False, batch=3, out=x)     # (loads the code objects)
    runtime.nv12_to_bgr(devs, out=bgr)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        runtime.preprocess_frames(devs, [64, 64], 32, torch.float16, auto=False, batch=3, out=x)
        runtime.nv12_to_bgr(devs, out=bgr)
    for k in range(2):
        hosts = [_host_frame(h, w, 60 + 2 * k + i, 'bt709') for i, (h, w) in enumerate(shapes)]
        for b, f in zip(bufs, hosts):
            b.copy_(torch.from_numpy(f.packed().reshape(-1)))
        x.fill_(float('nan'))
        for o in bgr:
            o.fill_(0xAB)
        g.replay()
        torch.cuda.synchronize()
        for b, f in enumerate(hosts):
            assert torch.equal(bgr[b].cpu(), torch.from_numpy(nv12_to_bgr_np(f))), (k, b)
            want = torch.from_numpy(letterbox_nv12_np(f, [64, 64], 32, auto=False)).half()
            assert _bits_equal(x[b].cpu(), want), (k, b)
        assert bool((x[2] == (torch.tensor(114.0) / 255).half()).all())


# ---- 7. argument errors -----------------------------------------------------------------------------------------------------------
def test_rejected_descriptors_leave_the_outputs_untouched():
    from yolov6.hip import abi, runtime
    lib = abi.load()
    frames = [_host_frame(20, 36, 70 + i, 'bt709').to('cuda') for i in range(3)]
    st = runtime._stream_ptr(torch.device('cuda', 0))
    x = torch.full((3, 3, 64, 64), -7.0, dtype=torch.float32, device='cuda')
    outs = [torch.full((20, 36, 3), 0xAB, dtype=torch.uint8, device='cuda') for _ in frames]

    def fused(edit):
        d = (abi.Nv12Desc * 3)()
        for e, f in zip(d, frames):
            e.y, e.uv, e.pitch_y, e.pitch_uv, e.h0, e.w0 = f.y.data_ptr(), f.uv.data_ptr(), f.pitch_y, f.pitch_uv, f.h, f.w
            e.y0, e.x0, e.th, e.tw, e.rh, e.rw, e.top, e.left, e.matrix = 0, 0, 20, 36, 36, 64, 14, 0, 1
        edit(d)
        return lib.lp_preprocess_nv12_batch(d, 3, 3, ctypes.c_void_p(x.data_ptr()), abi.LP_F32, 64, 64, st)

    def convert(edit):
        d = (abi.Nv12BgrDesc * 3)()
        for e, f, o in zip(d, frames, outs):
            e.y, e.uv, e.pitch_y, e.pitch_uv, e.h0, e.w0, e.matrix, e.out = f.y.data_ptr(), f.uv.data_ptr(), f.pitch_y, f.pitch_uv, f.h, f.w, 1, o.data_ptr()
        edit(d)
        return lib.lp_nv12_to_bgr_batch(d, 3, st)

    def setter(field, v):
        def edit(d):
            cur = getattr(d[2], field)
            # the tables of test_nv12_cpu are written for a 1080 x 1920 frame: scale their values to this 20 x 36 one
            scaled = {1079: 19, 1919: 35, 1918: 34, 1921: 37, 0x80001: (cur or 0) + 1, 1081: 21, 641: 65, 281: 29}.get(v, v)
            setattr(d[2], field, scaled)
        return edit

    for field, v, word in BAD_PLANES:
        for call in (fused, convert):
            assert call(setter(field, v)) == LP_ERR_ARG, (field, v)
            msg = lib.lp_last_error()
            assert b'entry 2' in msg and word.encode() in msg, (field, v, msg)
    assert convert(setter('out', None)) == LP_ERR_ARG and b'entry 2' in lib.lp_last_error()
    for field, v in BAD_REGIONS:
        assert fused(setter(field, v)) == LP_ERR_ARG and b'region of entry 2' in lib.lp_last_error(), (field, v)
    for field, v in BAD_GEOMETRY:
        assert fused(setter(field, v)) == LP_ERR_ARG and b'geometry of entry 2' in lib.lp_last_error(), (field, v)
    torch.cuda.synchronize()
    assert bool((x == -7.0).all()) and all(bool((o == 0xAB).all()) for o in outs)      # entries 0 and 1 were fine: nothing was launched
    assert fused(lambda d: None) == 0 and convert(lambda d: None) == 0                  # the unedited descriptors do run
    torch.cuda.synchronize()
    assert not bool((x == -7.0).any()) and torch.equal(outs[2], _bgr_dev(_host_frame(20, 36, 72, 'bt709')))
