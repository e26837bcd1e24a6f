"""Every letterbox entry point against its CPU specification, bit for bit, at the edges of the kernels' structure.

Entry points: runtime.preprocess_letterbox (preprocess_kernel), runtime.preprocess_frames on BGR frames and on Nv12Frames,
runtime.preprocess_tiles on BGR and on NV12 frames (letterbox_kernel over its two pixel sources); float32, float16, bfloat16.
Specifications: BGR -- ``letterbox(auto=False)`` with the fixed-point resize, BGR -> RGB, HWC -> CHW, ``.to(dtype)``, ``/= 255`` in
that dtype, the steps of ``Inferer.precess_image``; NV12 -- ``letterbox_nv12_np`` / ``region_nv12_np``; BGR regions -- the BGR
specification on a contiguous copy of the region.  The float32 BGR results are also held, times 255, to the float64 definition
(``lp_testing.bilinear64``) within the derived bar (``lp_testing.linear_u8_bar``), so the kernels do not rest on the numpy
restatement alone.

letterbox_kernel: a workgroup covers 256 output columns x 16 rows; a lane owns 4 adjacent columns; the 4 pixels go out as one
vector store when W % 4 == 0 and the base is 16-byte aligned, else one by one; the column coefficients of a tile sit in LDS.
  outputs  (48, 260)  two column tiles, the second 4 columns wide; three row bands
           (33, 98)   the per-element stores (98 % 4 != 0); two bands and one row
           (48, 260) at a base one element off 16-byte alignment: W % 4 == 0 and still the per-element stores
  sources  (1, 1) (1, 37) (37, 1) (2, 2)   every tap clamps on one or both axes
           (5, 7)      a 9.6x enlargement, runs of clamped pixels at both ends; (5, 8): the same with an odd left pad, the image
                       starts and ends inside a lane's group of 4
           (97, 131)   an ordinary reduction, odd sizes
           (48, 200) (33, 60)   ratio 1 in the first / second output: unresized, padded left and right
           (300, 1700) spans the full 260 columns, crosses the column-tile boundary inside the image, top pad 1
           (700, 900)  a 21x reduction into (33, 98)
           (40, 4100)  source columns beyond 4096: a float32 coordinate resolves an 11-bit weight step no finer than itself
           NV12: the nearest even sizes
  regions  inside a 64 x 96 frame and inside the 40 x 4100 one: an odd origin, a single pixel, a one-pixel-wide column at the
           right edge, the bottom-right corner, the whole frame, and regions of ratio 1 in either output (unresized)
  and one unresized 16 x 16 frame holding all 256 byte values: the / 255 conversion value by value, per dtype."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import lp_testing as T
from test_nv12_gpu import DTYPES, _nan_out, _place

pytestmark = pytest.mark.gpu

OUTS = [((48, 260), False), ((33, 98), False), ((48, 260), True)]              # ((H, W), base one element off 16-byte alignment)
BGR_SHAPES = [(1, 1), (1, 37), (37, 1), (2, 2), (5, 7), (5, 8), (97, 131), (48, 200), (33, 60), (300, 1700), (700, 900), (40, 4100)]
NV12_SHAPES = [(2, 2), (2, 38), (38, 2), (6, 8), (6, 6), (98, 132), (48, 200), (32, 60), (300, 1700), (700, 900), (40, 4100)]
# (frame, y0, x0, th, tw) in frames 0 = 64 x 96 and 1 = 40 x 4100
REGION_FRAMES = [(64, 96), (40, 4100)]
REGIONS = [(0, 5, 7, 31, 45),              # an odd origin
           (0, 17, 33, 1, 1),              # a single pixel
           (0, 3, 95, 50, 1),              # one pixel wide, at the right edge
           (0, 55, 83, 9, 13),             # the bottom-right corner
           (0, 0, 0, 64, 96),              # the whole frame
           (0, 11, 3, 33, 90),             # ratio 1 in (33, 98): unresized, padded left and right
           (0, 9, 1, 48, 95),              # ratio 1 in (48, 260)
           (1, 1, 4001, 37, 97),           # an odd origin beyond column 4096
           (1, 39, 4099, 1, 1),            # the last pixel
           (1, 0, 4099, 40, 1),            # the last column
           (1, 33, 3800, 7, 300),          # the bottom-right corner
           (1, 0, 0, 40, 4100),            # the whole frame
           (1, 3, 3835, 33, 98),           # exactly (33, 98): unresized, unpadded
           (1, 0, 3001, 40, 260)]          # ratio 1 in (48, 260): unresized, padded above and below


@pytest.fixture(autouse=True)
def _fixed_point_resize(monkeypatch):
    from yolov6.data import data_augment
    monkeypatch.setattr(data_augment, 'cv2', None)             # the specification is the fixed-point scheme wherever the suite runs


def _geom(shape, size):
    from yolov6.data.data_augment import letterbox_geometry
    _, (rw, rh), (top, bottom, left, right), _ = letterbox_geometry(shape, list(size), auto=False, stride=32)
    return rh, rw, top, left


def test_the_shapes_are_the_edges_they_are_listed_for():
    assert _geom((5, 7), (48, 260)) == (48, 67, 0, 96) and _geom((5, 8), (48, 260)) == (48, 77, 0, 91)       # an odd left pad
    assert _geom((5, 7), (33, 98)) == (33, 46, 0, 26)
    assert _geom((48, 200), (48, 260)) == (48, 200, 0, 30) and _geom((33, 60), (33, 98)) == (33, 60, 0, 19)   # ratio 1
    assert _geom((300, 1700), (48, 260)) == (46, 260, 1, 0)
    assert _geom((700, 900), (33, 98))[:2] == (33, 42) and _geom((40, 4100), (48, 260))[:2] == (3, 260)
    assert _geom((33, 90), (33, 98))[:2] == (33, 90) and _geom((48, 95), (48, 260))[:2] == (48, 95)
    assert _geom((33, 98), (33, 98)) == (33, 98, 0, 0) and _geom((40, 260), (48, 260)) == (40, 260, 4, 0)
    for f, y0, x0, th, tw in REGIONS:
        assert y0 + th <= REGION_FRAMES[f][0] and x0 + tw <= REGION_FRAMES[f][1]


# ---- inputs and specifications, computed once --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bgr_host(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape + (3,), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _nv12_host(shape, seed):
    from yolov6.utils.nv12 import MATRIX_NAMES, Nv12Frame
    h, w = shape
    rng = np.random.default_rng(seed)
    return Nv12Frame(rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2, 2), dtype=np.uint8), MATRIX_NAMES[seed % 4])


def _bgr_sources():
    return [_bgr_host(s, 500 + i) for i, s in enumerate(BGR_SHAPES)]


def _nv12_sources():
    return [_nv12_host(s, 600 + i) for i, s in enumerate(NV12_SHAPES)]


def _region_frames_bgr():
    return [_bgr_host(s, 700 + i) for i, s in enumerate(REGION_FRAMES)]


def _region_frames_nv12():
    return [_nv12_host(s, 800 + i) for i, s in enumerate(REGION_FRAMES)]


def _letterboxed(img, size):
    """uint8 [H, W, 3] BGR: data_augment.letterbox(auto=False) of a host frame."""
    from yolov6.data.data_augment import letterbox
    out = letterbox(img, list(size), auto=False, stride=32)[0]
    assert out.shape == tuple(size) + (3,)
    return out


def _network_input(lb_u8, dtype):
    """Inferer.precess_image's steps after the letterbox: HWC BGR -> CHW RGB, to ``dtype``, / 255 in that dtype."""
    t = torch.from_numpy(np.ascontiguousarray(lb_u8.transpose(2, 0, 1)[::-1])).to(dtype)
    t /= 255
    return t


@functools.lru_cache(maxsize=None)
def _spec_bgr_frames(size):
    return [_letterboxed(f, size) for f in _bgr_sources()]


@functools.lru_cache(maxsize=None)
def _spec_bgr_regions(size):
    frames = _region_frames_bgr()
    return [_letterboxed(np.ascontiguousarray(frames[f][y0:y0 + th, x0:x0 + tw]), size) for f, y0, x0, th, tw in REGIONS]


@functools.lru_cache(maxsize=None)
def _spec_nv12_frames(size):
    from yolov6.utils.nv12 import letterbox_nv12_np
    return [torch.from_numpy(letterbox_nv12_np(f, list(size), 32, auto=False)) for f in _nv12_sources()]


@functools.lru_cache(maxsize=None)
def _spec_nv12_regions(size):
    from yolov6.utils.nv12 import region_nv12_np
    frames = _region_frames_nv12()
    return [torch.from_numpy(region_nv12_np(frames[f], y0, x0, th, tw, list(size), 32)) for f, y0, x0, th, tw in REGIONS]


def _place_bgr(hosts):
    """The host frames on the device inside one 0xEE-filled buffer, each a contiguous [h, w, 3] view at an odd byte address."""
    sizes = [f.size for f in hosts]
    buf = torch.full((sum(sizes) + 2 * len(sizes) + 2,), 0xEE, dtype=torch.uint8, device='cuda')
    out, off = [], 1 - buf.data_ptr() % 2
    for f, n in zip(hosts, sizes):
        v = buf[off:off + n].view(f.shape)
        v.copy_(torch.from_numpy(f))
        assert v.data_ptr() % 2 == 1 and v.is_contiguous()
        out.append(v)
        off += n + (2 if n % 2 == 0 else 1)
    return out


def _place_nv12(hosts):
    return [_place(f, extra_y=1 + i % 4, extra_uv=2 * (i % 3)) for i, f in enumerate(hosts)]


# ---- comparisons -------------------------------------------------------------------------------------------------------------------
def _assert_slot(got, want, what):
    """One [3, H, W] result against its specification, bit for bit (NaN left by the pre-fill counts as a mismatch)."""
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = int(T.bit_mismatch_count(got, want))
    if bad:
        idx = (got.float() != want.float()) | got.float().isnan()
        c, y, x = [int(v) for v in idx.nonzero()[0]]
        raise AssertionError('%s: %d of %d elements differ, first at (c %d, y %d, x %d): got %r, specification %r'
                             % (what, bad, got.numel(), c, y, x, float(got[c, y, x]), float(want[c, y, x])))


def _assert_padding(got, dtype, what):
    assert bool((got == (torch.tensor(114.0) / 255).to(dtype)).all()), what


def _assert_in_bar(got_f32, src_u8, size, what):
    """A float32 [3, H, W] result, times 255, against the float64 bilinear of the BGR source inside the placed rectangle."""
    rh, rw, top, left = _geom(src_u8.shape[:2], size)
    px = (got_f32.cpu().double() * 255).numpy()[::-1].transpose(1, 2, 0)[top:top + rh, left:left + rw]      # -> HWC BGR
    assert float(np.abs(px - np.rint(px)).max()) < 1e-3, what                  # v / 255 in float32, times 255: v again
    d = np.rint(px) - T.bilinear64(src_u8, (rw, rh))
    lo, hi = T.linear_u8_bar(src_u8.shape[:2])
    assert lo <= float(d.min()) and float(d.max()) <= hi, (what, float(d.min()), float(d.max()), (lo, hi))
    if (rh, rw) == src_u8.shape[:2]:
        assert float(np.abs(d).max()) == 0.0, what


def _tag(*parts):
    return ' '.join(str(p) for p in parts)


# ---- the single-frame kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_single_frame_kernel_equals_the_specification(dtype):
    from yolov6.hip import abi, runtime
    lib = abi.load()
    hosts = _bgr_sources()
    devs = _place_bgr(hosts)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for size, misalign in OUTS:
        H, W = size
        for k, (h, d) in enumerate(zip(hosts, devs)):
            want = _network_input(_spec_bgr_frames(size)[k], dtype)
            what = _tag('preprocess_letterbox', dtype, h.shape[:2], '->', size, 'misaligned' if misalign else '')
            if misalign:                                                       # through the C entry point: the runtime allocates its own output
                out = _nan_out(1, H, W, dtype, True)
                rh, rw, top, left = _geom(h.shape[:2], size)
                abi.check(lib.lp_preprocess_letterbox(ctypes.c_void_p(d.data_ptr()), h.shape[0], h.shape[1], ctypes.c_void_p(out.data_ptr()),
                                                      runtime._DT[dtype], H, W, rh, rw, top, left, st), 'lp_preprocess_letterbox')
                got = out[0]
            else:
                got = runtime.preprocess_letterbox(d, list(size), 32, dtype, auto=False)
            _assert_slot(got, want, what)
            if dtype == torch.float32:
                _assert_in_bar(got, h, size, what)


# ---- whole frames through the batched kernel ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_bgr_frames_equal_the_specification(dtype):
    from yolov6.hip import runtime
    hosts = _bgr_sources()
    devs = _place_bgr(hosts)
    B = len(hosts) + 1                                                         # one padding slot
    for size, misalign in OUTS:
        H, W = size
        got, geoms = runtime.preprocess_frames(devs, list(size), 32, dtype, auto=False, batch=B, out=_nan_out(B, H, W, dtype, misalign))
        for k, h in enumerate(hosts):
            what = _tag('preprocess_frames BGR', dtype, h.shape[:2], '->', size, 'misaligned' if misalign else '')
            assert geoms[k] == _geom(h.shape[:2], size), what
            _assert_slot(got[k], _network_input(_spec_bgr_frames(size)[k], dtype), what)
            if dtype == torch.float32:
                _assert_in_bar(got[k], h, size, what)
        _assert_padding(got[len(hosts):], dtype, _tag('preprocess_frames BGR padding', dtype, size))


@pytest.mark.parametrize('dtype', DTYPES)
def test_nv12_frames_equal_the_specification(dtype):
    from yolov6.hip import runtime
    hosts = _nv12_sources()
    devs = _place_nv12(hosts)
    B = len(hosts) + 1
    for size, misalign in OUTS:
        H, W = size
        got, geoms = runtime.preprocess_frames(devs, list(size), 32, dtype, auto=False, batch=B, out=_nan_out(B, H, W, dtype, misalign))
        for k, h in enumerate(hosts):
            what = _tag('preprocess_frames NV12', dtype, h.shape[:2], '->', size, 'misaligned' if misalign else '')
            assert geoms[k] == _geom(h.shape[:2], size), what
            _assert_slot(got[k], _spec_nv12_frames(size)[k].to(dtype), what)
        _assert_padding(got[len(hosts):], dtype, _tag('preprocess_frames NV12 padding', dtype, size))


# ---- regions ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_bgr_regions_equal_the_specification_on_region_copies(dtype):
    from yolov6.hip import runtime
    hosts = _region_frames_bgr()
    devs = _place_bgr(hosts)
    B = len(REGIONS) + 1
    for size, misalign in OUTS:
        H, W = size
        got, geoms = runtime.preprocess_tiles(devs, REGIONS, list(size), 32, dtype, batch=B, out=_nan_out(B, H, W, dtype, misalign))
        for k, (f, y0, x0, th, tw) in enumerate(REGIONS):
            what = _tag('preprocess_tiles BGR', dtype, REGIONS[k], '->', size, 'misaligned' if misalign else '')
            assert geoms[k] == _geom((th, tw), size), what
            _assert_slot(got[k], _network_input(_spec_bgr_regions(size)[k], dtype), what)
            if dtype == torch.float32:
                _assert_in_bar(got[k], np.ascontiguousarray(hosts[f][y0:y0 + th, x0:x0 + tw]), size, what)
        _assert_padding(got[len(REGIONS):], dtype, _tag('preprocess_tiles BGR padding', dtype, size))


@pytest.mark.parametrize('dtype', DTYPES)
def test_nv12_regions_equal_the_specification(dtype):
    from yolov6.hip import runtime
    hosts = _region_frames_nv12()
    devs = _place_nv12(hosts)
    B = len(REGIONS) + 1
    for size, misalign in OUTS:
        H, W = size
        got, geoms = runtime.preprocess_tiles(devs, REGIONS, list(size), 32, dtype, batch=B, out=_nan_out(B, H, W, dtype, misalign))
        for k, (f, y0, x0, th, tw) in enumerate(REGIONS):
            what = _tag('preprocess_tiles NV12', dtype, REGIONS[k], '->', size, 'misaligned' if misalign else '')
            assert geoms[k] == _geom((th, tw), size), what
            _assert_slot(got[k], _spec_nv12_regions(size)[k].to(dtype), what)
        _assert_padding(got[len(REGIONS):], dtype, _tag('preprocess_tiles NV12 padding', dtype, size))


# ---- the conversion, value by value ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_all_256_byte_values_unresized(dtype):
    """A 16 x 16 frame into a 16 x 16 output: no resize, no padding, so each output element is one input byte / 255 in ``dtype``.
    The expected value is computed here from the byte (float32 division, one rounding to ``dtype``), not by the specification's
    code.  NV12: full-range matrix and neutral chroma, so B = G = R = Y."""
    from yolov6.hip import runtime
    from yolov6.utils.nv12 import Nv12Frame, nv12_to_bgr_np
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    bgr = np.stack([v, v[::-1, ::-1], (v.astype(np.int32) * 7 + 3 & 255).astype(np.uint8)], -1)             # three bijections of 0..255
    want = torch.from_numpy((np.ascontiguousarray(bgr.transpose(2, 0, 1)[::-1]).astype(np.float32) / np.float32(255))).to(dtype)
    assert all(len(np.unique(bgr[:, :, c])) == 256 for c in range(3))
    assert torch.equal(want, _network_input(bgr, dtype))                       # and the specification agrees
    nv = Nv12Frame(v.copy(), np.full((8, 8, 2), 128, np.uint8), 'bt601f')
    assert np.array_equal(nv12_to_bgr_np(nv), np.stack([v, v, v], -1))
    want_nv = torch.from_numpy(np.broadcast_to(v, (3, 16, 16)).astype(np.float32) / np.float32(255)).to(dtype)
    dev, dnv = _place_bgr([bgr])[0], _place(nv, extra_y=3, extra_uv=2)
    whole = [(0, 0, 0, 16, 16)]
    results = {'preprocess_letterbox': runtime.preprocess_letterbox(dev, [16, 16], 32, dtype, auto=False),
               'preprocess_frames BGR': runtime.preprocess_frames([dev], [16, 16], 32, dtype, auto=False, out=_nan_out(1, 16, 16, dtype))[0][0],
               'preprocess_tiles BGR': runtime.preprocess_tiles([dev], whole, [16, 16], 32, dtype, out=_nan_out(1, 16, 16, dtype))[0][0]}
    for name, got in results.items():
        _assert_slot(got, want, _tag(name, dtype, 'all byte values'))
    results = {'preprocess_frames NV12': runtime.preprocess_frames([dnv], [16, 16], 32, dtype, auto=False, out=_nan_out(1, 16, 16, dtype))[0][0],
               'preprocess_tiles NV12': runtime.preprocess_tiles([dnv], whole, [16, 16], 32, dtype, out=_nan_out(1, 16, 16, dtype))[0][0]}
    for name, got in results.items():
        _assert_slot(got, want_nv, _tag(name, dtype, 'all byte values'))
    assert len(torch.unique(want.float())) == 256                              # 256 distinct values survive the conversion in every dtype
