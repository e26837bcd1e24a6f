"""NV12 frames on the CPU: the conversion rule of yolov6/utils/nv12.py against the standards' float matrices over every (Y, U, V),
the host encoder's round trip, the container (packed views, raw streams, rejected inputs), the C ABI's descriptor layout and its
host-side checks, and Inferer(nv12=...) on the CPU path."""
import ctypes
import importlib
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

LP_ERR_ARG = -1
# the specification (include/lp_hip.h): id, name, yoff, CY, CUB, CUG, CVG, CVR
TABLE = [(0, 'bt601', 16, 1220542, 2116026, -409993, -852492, 1673527),
         (1, 'bt709', 16, 1220945, 2215014, -223607, -558796, 1879825),
         (2, 'bt601f', 0, 1048576, 1858077, -360853, -748826, 1470104),
         (3, 'bt709f', 0, 1048576, 1945738, -196424, -490864, 1651297)]
NAMES = [t[1] for t in TABLE]


def _standard(kr, kb, limited):
    """(yoff, cy, cub, cug, cvg, cvr) of a YCbCr standard with luma weights kr, kb: the float matrix, written out."""
    kg = 1.0 - kr - kb
    sy, sc = (255.0 / 219.0, 255.0 / 224.0) if limited else (1.0, 1.0)
    return (16 if limited else 0, sy, 2 * (1 - kb) * sc, -kb / kg * 2 * (1 - kb) * sc, -kr / kg * 2 * (1 - kr) * sc, 2 * (1 - kr) * sc)


FLOAT = {'bt601': (16, 1.164, 2.018, -0.391, -0.813, 1.596),          # OpenCV's 3-decimal constants
         'bt709': _standard(0.2126, 0.0722, True),
         'bt601f': _standard(0.299, 0.114, False),
         'bt709f': _standard(0.2126, 0.0722, False)}


def test_table_is_the_specification():
    from yolov6.utils import nv12
    assert len(nv12.MATRICES) == 4 and list(nv12.MATRIX_NAMES) == NAMES
    for mid, name, *coef in TABLE:
        assert nv12.MATRICES[name] == (mid, *coef)
    for _, name, _, *ints in TABLE[1:]:                 # rows 1..3: round(x * 2^20) of the float matrix
        assert list(ints) == [int(round(v * 2 ** 20)) for v in FLOAT[name][1:]], name
    src = open(os.path.join(REPO, 'yolo-lp_amd', 'csrc', 'lp_nv12_color.inc')).read()
    for _, _, *coef in TABLE:                           # the kernels' table is the same one
        assert '{%s}' % ', '.join(str(c) for c in coef) in src


def test_grey_axis():
    from yolov6.utils.nv12 import yuv_to_bgr_np
    Y = np.arange(256)
    n = np.full(256, 128)
    for name in ('bt601', 'bt709'):
        out = yuv_to_bgr_np(Y, n, n, name)
        assert (out[16] == 0).all() and (out[235] == 255).all() and (out[:16] == 0).all() and (out[236:] == 255).all()
        assert (out[:, 0] == out[:, 1]).all() and (out[:, 1] == out[:, 2]).all()
    for name in ('bt601f', 'bt709f'):
        assert (yuv_to_bgr_np(Y, n, n, name) == Y[:, None]).all()


@pytest.mark.parametrize('name', NAMES)
def test_every_triple_is_within_one_of_the_float_matrix(name):
    """All 2^24 (Y, U, V): the rule's integers against clip(float64 matrix, 0, 255) with the rule's luma floor max(Y - yoff, 0):
    at most 1 apart (the fixed-point value is the float one to within 0.5001 before it is rounded to nearest)."""
    from yolov6.utils.nv12 import yuv_to_bgr_np
    yoff, cy, cub, cug, cvg, cvr = FLOAT[name]
    U, V = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    d, e = U - 128.0, V - 128.0
    chroma = np.stack([cub * d, cug * d + cvg * e, cvr * e], -1)
    worst = 0.0
    for y in range(256):
        got = yuv_to_bgr_np(np.full_like(U, y), U, V, name).astype(np.float64)
        want = np.clip(cy * max(y - yoff, 0) + chroma, 0.0, 255.0)
        worst = max(worst, float(np.abs(got - want).max()))
    print('%s: largest |fixed - float| = %.4f' % (name, worst))
    assert worst <= 1.0


def _roundtrip_bound(name):
    """Per channel (B, G, R).  The encoder rounds Y, U and V each to within 0.5, so with exact inverse matrices the decoder's
    real-valued result is within E = 0.5 (CY + |Cu| + |Cv|) / 2^20 of the integer it started from (a frame constant over 2 x 2
    blocks loses nothing to the chroma mean; inside gamut nothing is clipped on the way in); rounding that to nearest lands at
    most floor(E + 0.5) away, and the final clip to 0..255 cannot move it further from a value in 0..255."""
    from yolov6.utils.nv12 import MATRICES
    _, _, CY, CUB, CUG, CVG, CVR = MATRICES[name]
    return [int(np.floor(0.5 * (CY + abs(cu) + abs(cv)) / 2 ** 20 + 0.5)) for cu, cv in ((CUB, 0), (CUG, CVG), (0, CVR))]


@pytest.mark.parametrize('name', NAMES)
def test_encoder_round_trip(name):
    from yolov6.utils.nv12 import bgr_to_nv12_np, nv12_to_bgr_np
    rng = np.random.default_rng(5)
    bound = _roundtrip_bound(name)
    assert max(bound) <= 2
    # constant over 2 x 2 blocks, values 16..239: every such BGR is inside the YCbCr gamut (no clipping in the encoder)
    x = np.repeat(np.repeat(rng.integers(16, 240, (48, 64, 3), dtype=np.uint8), 2, 0), 2, 1)
    f = bgr_to_nv12_np(x, name)
    assert f.shape == x.shape and 0 < f.y.min() and f.y.max() < 255 and 0 < f.uv.min() and f.uv.max() < 255
    diff = np.abs(nv12_to_bgr_np(f).astype(int) - x).reshape(-1, 3).max(0)
    print('%s: round trip of a 2x2-constant frame, per channel %s (bound %s)' % (name, diff.tolist(), bound))
    assert (diff <= bound).all()
    noise = rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)      # chroma is subsampled: reported only
    d = np.abs(nv12_to_bgr_np(bgr_to_nv12_np(noise, name)).astype(int) - noise)
    print('%s: round trip of noise: max %d, mean %.2f' % (name, d.max(), d.mean()))


def test_from_packed_views_alias_the_buffer():
    from yolov6.utils.nv12 import Nv12Frame
    buf = np.zeros((12, 16), np.uint8)
    f = Nv12Frame.from_packed(buf, 8, 16, 'bt709')
    assert f.shape == (8, 16, 3) and f.matrix_id == 1 and (f.pitch_y, f.pitch_uv) == (16, 16)
    f.y[3, 5], f.uv[1, 2, 0], f.uv[3, 7, 1] = 7, 8, 9
    assert buf[3, 5] == 7 and buf[8 + 1, 4] == 8 and buf[11, 15] == 9
    t = torch.zeros(12 * 16, dtype=torch.uint8)
    g = Nv12Frame.from_packed(t, 8, 16)
    g.y[7, 15], g.uv[0, 0, 1] = 3, 4
    assert t[8 * 16 - 1] == 3 and t[8 * 16 + 1] == 4 and g.is_tensor and not g.is_cuda
    # a pitched frame: views of a wider buffer
    wide = np.arange(12 * 32, dtype=np.uint8).reshape(12, 32)
    p = Nv12Frame(wide[:8, :16], wide[8:, :16].reshape(4, 8, 2))
    assert (p.pitch_y, p.pitch_uv) == (32, 32) and np.array_equal(p.packed()[8:], wide[8:, :16])


def test_odd_sizes_and_mixed_lists_are_rejected():
    from yolov6.utils import nv12
    from yolov6.core.frames import FrameBatcher          # noqa: F401  (imports without a GPU)
    from yolov6.hip import runtime
    for h, w in ((7, 8), (8, 7), (0, 8), (1, 1)):
        with pytest.raises(ValueError):
            nv12.bgr_to_nv12_np(np.zeros((h, w, 3), np.uint8))
        with pytest.raises(ValueError):
            nv12.Nv12Frame.from_packed(np.zeros(max(h * w * 3 // 2, 1), np.uint8), h, w)
    with pytest.raises(ValueError):
        nv12.Nv12Frame(np.zeros((4, 4), np.uint8), np.zeros((2, 2, 2), np.uint8), 'bt2020')
    with pytest.raises(ValueError):
        nv12.Nv12Frame(np.zeros((4, 4), np.uint8), np.zeros((2, 4, 2), np.uint8))
    with pytest.raises(ValueError):                        # uv rows an odd number of bytes apart
        nv12.Nv12Frame(np.zeros((4, 4), np.uint8), np.lib.stride_tricks.as_strided(np.zeros(16, np.uint8), (2, 2, 2), (5, 2, 1)))
    f = nv12.bgr_to_nv12_np(np.zeros((4, 4, 3), np.uint8))
    bgr = np.zeros((4, 4, 3), np.uint8)
    assert nv12.is_nv12_list([f, f]) and not nv12.is_nv12_list([bgr]) and nv12.is_nv12_list([None, f])
    with pytest.raises(ValueError, match='one kind'):
        nv12.is_nv12_list([f, bgr])
    tf = nv12.Nv12Frame.from_packed(torch.zeros(24, dtype=torch.uint8), 4, 4)
    with pytest.raises(ValueError, match='one kind'):      # checked before anything needs a device
        runtime.preprocess_frames([tf, torch.zeros(4, 4, 3, dtype=torch.uint8)], [64, 64], 32, torch.float16)
    with pytest.raises(ValueError):                        # host planes are not device frames
        runtime.preprocess_frames([tf], [64, 64], 32, torch.float16)


def test_raw_stream_round_trip(tmp_path):
    from yolov6.utils.nv12 import bgr_to_nv12_np, read_nv12_stream
    from yolov6.data.datasets import LoadData
    rng = np.random.default_rng(2)
    frames = [bgr_to_nv12_np(rng.integers(0, 256, (6, 10, 3), dtype=np.uint8), 'bt601f') for _ in range(2)]
    path = tmp_path / 'clip.nv12'
    np.concatenate([f.packed() for f in frames]).tofile(str(path))
    assert os.path.getsize(str(path)) == 2 * 90
    for batch in (1, 2, 5):
        got = [f for chunk in read_nv12_stream(str(path), 6, 10, 'bt601f', batch) for f in chunk]
        assert len(got) == 2
        for g, f in zip(got, frames):
            assert g.matrix == 'bt601f' and np.array_equal(g.y, f.y) and np.array_equal(g.uv, f.uv)
    with pytest.raises(ValueError):
        next(read_nv12_stream(str(path), 6, 8))             # 180 bytes are not whole 6 x 8 frames
    src = LoadData(str(path), nv12_size=(10, 6), nv12_matrix='bt601f')
    items = list(src)
    assert len(items) == 2 and src.type == 'video' and np.array_equal(items[1][0].y, frames[1].y)
    with pytest.raises(ValueError):
        list(LoadData(str(path)))                           # no frame size


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def _header_struct(name):
    """[(ctype, field)] of `typedef struct name { ... } name;` in include/lp_hip.h (pointers and ints only)."""
    header = open(os.path.join(REPO, 'include', 'lp_hip.h')).read()
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r'(const unsigned char\*|unsigned char\*|int)\s+(.*)$', decl, re.S)
        assert m, decl
        ctype = ctypes.c_int if m.group(1) == 'int' else ctypes.c_void_p
        fields += [(ctype, f.strip()) for f in m.group(2).split(',')]
    return fields


@pytest.mark.parametrize('name, cls', [('lp_nv12_desc', 'Nv12Desc'), ('lp_nv12_bgr_desc', 'Nv12BgrDesc')])
def test_descriptor_layout_matches_the_header(name, cls):
    from yolov6.hip import abi
    want = _header_struct(name)
    got = getattr(abi, cls)
    assert [(t, f) for f, t in got._fields_] == want
    mirror = type('Mirror', (ctypes.Structure,), {'_fields_': [(f, t) for t, f in want]})
    assert ctypes.sizeof(got) == ctypes.sizeof(mirror) == {'lp_nv12_desc': 72, 'lp_nv12_bgr_desc': 48}[name]
    assert abi.LP_NV12_PER_LAUNCH == 32 and 'LP_NV12_PER_LAUNCH 32' in open(os.path.join(REPO, 'include', 'lp_hip.h')).read()


def _nv12_descs(n, **kw):
    from yolov6.hip import abi
    d = (abi.Nv12Desc * max(n, 1))()
    base = dict(y=0x10000, uv=0x80000, pitch_y=1920, pitch_uv=1920, h0=1080, w0=1920, y0=0, x0=0, th=1080, tw=1920, rh=360, rw=640,
                top=140, left=0, matrix=1)
    base.update(kw)
    for e in d:
        for k, v in base.items():
            setattr(e, k, v)
    return d


BAD_PLANES = [('y', None, 'null plane'), ('uv', None, 'null plane'), ('h0', 1079, 'even'), ('w0', 1919, 'even'), ('pitch_y', 1918, 'pitch_y'),
              ('pitch_uv', 1918, 'pitch_uv'), ('pitch_uv', 1921, 'pitch_uv'), ('uv', 0x80001, 'aligned'), ('matrix', 4, 'matrix'),
              ('matrix', -1, 'matrix')]
BAD_REGIONS = [('y0', -1), ('x0', -1), ('th', 0), ('tw', 0), ('y0', 1), ('x0', 2), ('th', 1081), ('tw', 1921)]
BAD_GEOMETRY = [('rh', 0), ('rw', 641), ('top', 281), ('left', -1), ('top', -1), ('left', 1)]


def test_preprocess_nv12_rejects_bad_descriptors_before_launch():
    """Fake device addresses: a launch would fault, so LP_ERR_ARG with the entry's index proves the host check came first."""
    from yolov6.hip import abi
    lib = abi.load()
    call = lambda d, n, B, dt=0, H=640, W=640, out=0x200000: lib.lp_preprocess_nv12_batch(      # noqa: E731
        d, n, B, ctypes.c_void_p(out) if out else None, dt, H, W, None)
    d = _nv12_descs(3)
    assert call(d, 3, 3, out=0) == LP_ERR_ARG and call(d, 3, 2) == LP_ERR_ARG and call(d, 3, 3, dt=5) == LP_ERR_ARG
    assert call(None, 2, 2) == LP_ERR_ARG and call(d, -1, 2) == LP_ERR_ARG and call(d, 1, 1, H=0) == LP_ERR_ARG
    for field, v, word in BAD_PLANES:
        d = _nv12_descs(3)
        setattr(d[2], field, v)
        assert call(d, 3, 3) == LP_ERR_ARG, (field, v)
        msg = lib.lp_last_error()
        assert b'entry 2' in msg and word.encode() in msg, (field, v, msg)
    for field, v in BAD_REGIONS:
        d = _nv12_descs(2)
        setattr(d[1], field, v)
        assert call(d, 2, 2) == LP_ERR_ARG and b'region of entry 1' in lib.lp_last_error(), (field, v)
    for field, v in BAD_GEOMETRY:
        d = _nv12_descs(2)
        setattr(d[0], field, v)
        assert call(d, 2, 2) == LP_ERR_ARG and b'geometry of entry 0' in lib.lp_last_error(), (field, v)


def test_nv12_to_bgr_rejects_bad_descriptors_before_launch():
    from yolov6.hip import abi
    lib = abi.load()

    def descs(n, **kw):
        d = (abi.Nv12BgrDesc * n)()
        base = dict(y=0x10000, uv=0x80000, pitch_y=1920, pitch_uv=1920, h0=1080, w0=1920, matrix=3, out=0x300001)
        base.update(kw)
        for e in d:
            for k, v in base.items():
                setattr(e, k, v)
        return d
    assert lib.lp_nv12_to_bgr_batch(None, 1, None) == LP_ERR_ARG and lib.lp_nv12_to_bgr_batch(descs(1), -1, None) == LP_ERR_ARG
    assert lib.lp_nv12_to_bgr_batch(None, 0, None) == 0
    for field, v, word in BAD_PLANES + [('out', None, 'null out')]:
        d = descs(70)
        setattr(d[66], field, v)                            # an entry of the second launch: nothing of the first is launched either
        assert lib.lp_nv12_to_bgr_batch(d, 70, None) == LP_ERR_ARG, (field, v)
        msg = lib.lp_last_error()
        assert b'entry 66' in msg and word.encode() in msg, (field, v, msg)


# ---- Inferer on the CPU ---------------------------------------------------------------------------------------------------------
def test_infer_nv12_on_the_cpu_is_the_bgr_path_on_the_converted_frames(tmp_path, monkeypatch):
    """--nv12 on the CPU = nv12_to_bgr_np, then the existing path: the same detections and label files as plain runs on the
    converted frames saved as images; a raw .nv12 stream of the same frames gives them too."""
    from PIL import Image
    from yolov6.utils.nv12 import bgr_to_nv12_np, nv12_to_bgr_np
    from yolov6.utils.synth import build_synthetic
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    m = build_synthetic(os.path.join(REPO, 'configs', 'yololps.py'), width=0.0625, sigma=1.5)
    ckpt = tmp_path / 'tiny.pt'
    torch.save({'model': m.half(), 'ema': None}, str(ckpt))
    rng = np.random.default_rng(12)
    src, conv, raw = tmp_path / 'src', tmp_path / 'conv', tmp_path / 'raw'
    for d in (src, conv, raw):
        d.mkdir()
    packed = []
    for i in range(2):
        rgb = rng.integers(0, 255, (232, 145, 3), dtype=np.uint8)               # an odd width: the encoder's stand-in cuts it to 144
        Image.fromarray(rgb).save(str(src / ('f%d.png' % i)))
        f = bgr_to_nv12_np(np.ascontiguousarray(rgb[:, :144, ::-1]), 'bt709')
        packed.append(f.packed())
        Image.fromarray(np.ascontiguousarray(nv12_to_bgr_np(f)[:, :, ::-1])).save(str(conv / ('f%d.png' % i)))
    np.concatenate(packed).tofile(str(raw / 'clip.nv12'))
    kw = dict(weights=str(ckpt), yaml=None, img_size=[256, 256], conf_thres=0.06, iou_thres=0.45, max_det=50, device='cpu',
              save_txt=True, not_save_img=True, half=False)
    want = infer.run(source=str(conv), save_dir=str(tmp_path / 'o_conv'), **kw)
    got = infer.run(source=str(src), save_dir=str(tmp_path / 'o_src'), nv12='bt709', **kw)
    stream = infer.run(source=str(raw), save_dir=str(tmp_path / 'o_raw'), nv12='bt709', nv12_size=(144, 232), **kw)
    assert len(want) == len(got) == len(stream) == 2 and sum(len(d) for d in want) > 0
    for a, b, c in zip(want, got, stream):
        assert torch.equal(a, b) and torch.equal(a, c)
    for i in range(2):
        p, q = tmp_path / 'o_conv' / 'conv' / ('f%d.txt' % i), tmp_path / 'o_src' / 'src' / ('f%d.txt' % i)
        assert p.exists() == q.exists() and (not p.exists() or p.read_bytes() == q.read_bytes())
    with pytest.raises(ValueError):
        infer.run(source=str(raw), save_dir=str(tmp_path / 'o_bad'), **kw)      # a .nv12 source without --nv12
