"""Baseline JPEG on the CPU: the specification yolov6/utils/jpeg.py alone.  Its tables against the files PIL (libjpeg) writes, the
integer DCT, quantiser and colour rule against their float64 definitions, the header segment by segment, PIL decoding every test
stream to what ``jpeg_reconstruct_np`` predicts, size and PSNR against PIL's own encoder, the symbol coverage of the constructed
set that tests/test_jpeg_gpu.py shares (``constructed_set``), and wrong emulations of the coder that the checks must catch."""
import io

import numpy as np
import pytest
from PIL import Image

QUALITIES = (50, 75, 95)


# ---- helpers shared with tests/test_jpeg_gpu.py ----------------------------------------------------
def grey(plane):
    """uint8 [h, w] -> BGR [h, w, 3] whose Y is the plane itself and whose chroma is 128."""
    return np.repeat(np.asarray(plane, np.uint8)[:, :, None], 3, axis=2)


def synthetic(h=160, w=176, seed=0):
    """The sinusoid plus sigma 20 noise of the size and PSNR comparison."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    base = 128 + 60 * np.sin(xx / 9.0) * np.cos(yy / 13.0)
    return np.clip(base[:, :, None] + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8)


def basis_image(indices, amp=400.0):
    """A grey 16 x (8 * len) strip whose k-th 8 x 8 block of the top row is 128 + amp * (the basis function of zig-zag index
    indices[k]); the bottom row is flat.  At quality 50 only that coefficient survives the quantiser."""
    from yolov6.utils.jpeg import DCT_F, ZIGZAG
    w = (8 * len(indices) + 15) // 16 * 16
    img = np.full((16, w), 128.0)
    for k, z in enumerate(indices):
        u, v = divmod(int(ZIGZAG[z]), 8)
        img[:8, 8 * k:8 * k + 8] += amp * np.outer(DCT_F[u], DCT_F[v])
    return grey(np.clip(np.rint(img), 0, 255))


def constructed_set():
    """[(name, BGR image, quality, restart)]: small images built so that together they drive the coder through every DC category,
    every AC size, one, two and three ZRL, a block without EOB, an all-zero-AC block, stuffed bytes, every pad length and a
    wrapping RSTm (``test_constructed_set_covers_the_coder``)."""
    rng = np.random.default_rng(7)
    out = [('noise100', rng.integers(0, 256, (48, 64, 3), dtype=np.uint8), 100, 1)]
    out.append(('noise100_grey', grey(rng.integers(0, 256, (32, 80), dtype=np.uint8)), 100, 2))
    out.append(('flat', np.full((32, 32, 3), 77, np.uint8), 90, 2))
    blocks = (np.add.outer(np.arange(8), np.arange(8)) & 1) * 255                       # 8 x 8 blocks alternating 0 / 255
    out.append(('extremes', grey(np.kron(blocks, np.ones((8, 8)))), 100, 4))
    edge = np.zeros((32, 32))
    edge[:, 4::8] = edge[:, 5::8] = edge[:, 6::8] = edge[:, 7::8] = 255                 # a vertical edge inside every block
    edge[16:] = edge.T.copy()[16:]                                                      # ... a horizontal one in the lower half
    out.append(('edges', grey(edge), 100, 3))
    levels = 128 + np.array([0, 1, 3, 7, 15, 31, 63, 127, 63, -64, 72, -128, 127, 0, 100, -28])     # DC steps of every size
    out.append(('steps', grey(np.kron(levels.reshape(2, 8), np.ones((8, 8)))), 100, 16))
    out.append(('steps50', grey(np.kron(levels.reshape(2, 8), np.ones((8, 8)))), 50, 5))
    out.append(('basis', basis_image([17, 20, 32, 33, 40, 48, 49, 56, 63, 1, 5, 62]), 50, 1))
    return out


def segments(data):
    """[(marker, payload)] of the segments SOI .. SOS of a stream, and the offset at which the entropy-coded data begins."""
    assert data[:2] == b'\xff\xd8'
    i, out = 2, []
    while True:
        assert data[i] == 0xFF, 'segment marker expected at %d' % i
        m, n = data[i + 1], int.from_bytes(data[i + 2:i + 4], 'big')
        out.append((m, data[i + 4:i + 2 + n]))
        i += 2 + n
        if m == 0xDA:
            return out, i


def pil_planes(data):
    """(Y, Cb, Cr) uint8 planes [h, w] PIL decodes without a colour conversion, or raises."""
    im = Image.open(io.BytesIO(data))
    im.draft('YCbCr', im.size)
    assert im.mode == 'YCbCr'
    a = np.asarray(im)
    return a[..., 0], a[..., 1], a[..., 2]


def pil_check(data, frame, quality):
    """PIL opens ``data`` with the frame's size and three components, and its Y plane is within 1 of ``jpeg_reconstruct_np``
    (libjpeg's default inverse DCT meets IEEE 1180: one level).  Returns the largest difference."""
    from yolov6.utils.jpeg import jpeg_reconstruct_np
    im = Image.open(io.BytesIO(data))
    assert im.format == 'JPEG' and im.size == (frame.shape[1], frame.shape[0]) and len(im.getbands()) == 3
    Y, _, _ = pil_planes(data)
    ref, _, _ = jpeg_reconstruct_np(frame, quality)
    d = float(np.abs(Y.astype(np.float64) - ref).max())
    assert d <= 1.0, 'decoded Y is %g away from the reconstruction' % d
    return d


def _pil_jpeg(img_bgr, quality):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img_bgr[..., ::-1])).save(buf, format='JPEG', quality=quality, subsampling=2)
    return buf.getvalue()


# ---- the tables -----------------------------------------------------------------------------------
def test_quant_tables_are_libjpegs_for_every_quality():
    from yolov6.utils.jpeg import ZIGZAG, quant_tables
    img = synthetic(16, 16)
    for q in range(1, 101):
        segs, _ = segments(_pil_jpeg(img, q))
        dqt = b''.join(p for m, p in segs if m == 0xDB)
        assert len(dqt) == 130 and dqt[0] == 0 and dqt[65] == 1, q
        ql, qc = quant_tables(q)
        assert bytes(dqt[1:65]) == bytes(ql[ZIGZAG].astype(np.uint8)), q
        assert bytes(dqt[66:130]) == bytes(qc[ZIGZAG].astype(np.uint8)), q
        assert ql.min() >= 1 and ql.max() <= 255 and qc.min() >= 1 and qc.max() <= 255
    for bad in (0, 101, -3):
        with pytest.raises(ValueError):
            quant_tables(bad)


def test_huffman_tables_are_the_ones_pil_writes():
    from yolov6.utils.jpeg import HUFF, HUFF_ORDER, huff_codes
    segs, _ = segments(_pil_jpeg(synthetic(32, 32), 80))
    dht = b''.join(p for m, p in segs if m == 0xC4)
    found, i = {}, 0
    while i < len(dht):
        n = sum(dht[i + 1:i + 17])
        found[dht[i]] = (tuple(dht[i + 1:i + 17]), tuple(dht[i + 17:i + 17 + n]))
        i += 17 + n
    assert sorted(found) == [0x00, 0x01, 0x10, 0x11]
    for name in HUFF_ORDER:
        tc_th, counts, values = HUFF[name]
        assert found[tc_th] == (tuple(counts), tuple(values)), name
        assert len(counts) == 16 and sum(counts) == len(values) == (162 if name.startswith('ac') else 12)
        codes = huff_codes(name)
        assert len(codes) == len(values) and max(n for _, n in codes.values()) <= 16
        words = sorted(format(c, '0%db' % n) for c, n in codes.values())            # prefix-free
        assert not any(b.startswith(a) for a, b in zip(words, words[1:]))


# ---- the integer steps ----------------------------------------------------------------------------
def _extreme_blocks():
    from yolov6.utils.jpeg import DCT_F
    out = [np.zeros((8, 8)), np.full((8, 8), 255.0)]
    cb = np.add.outer(np.arange(8), np.arange(8)) & 1
    out += [cb * 255.0, (1 - cb) * 255.0]
    for u in range(8):
        for v in range(8):
            s = np.outer(DCT_F[u], DCT_F[v]) >= 0
            out += [s * 255.0, (~s) * 255.0]
    return np.stack(out).astype(np.int32)


def test_integer_dct_is_within_one_of_the_float_dct_and_inside_int32():
    """20 000 random blocks and the extreme ones: |integer - float64 orthonormal DCT| < 1, the int64 evaluation of both passes
    stays inside int32, |AC| <= 1020 and DC in -1024..1016 (so categories stop at 10 and 11, which the Annex K tables cover)."""
    from yolov6.utils.jpeg import DCT_F, DCT_M, fdct_np
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.integers(0, 256, (20000, 8, 8)).astype(np.int32), _extreme_blocks()])
    got = fdct_np(x)
    want = DCT_F @ (x - 128.0) @ DCT_F.T
    dev = float(np.abs(got - want).max())
    print('largest deviation from the float64 DCT: %.4f' % dev)
    assert dev < 1.0
    M = DCT_M.astype(np.int64)
    t = (x.astype(np.int64) - 128) @ M.T
    u = M @ ((t + 128) >> 8)
    big = max(int(np.abs(t).max()) + 128, int(np.abs(u).max()) + 32768)
    print('largest intermediate: %.3g' % big)
    assert big < 2 ** 31
    assert np.array_equal(got, (u + 32768) >> 16)          # int32 arithmetic gave the int64 result
    ac = got.reshape(-1, 64)[:, 1:]
    assert np.abs(ac).max() <= 1020 and got[:, 0, 0].min() >= -1024 and got[:, 0, 0].max() <= 1016
    assert got[20000, 0, 0] == -1024 and got[20001, 0, 0] == 1016       # the flat blocks 0 and 255


def test_reciprocal_quantiser_equals_the_division():
    """The kernel's (n * ceil(2^20 / Q)) >> 20 against n // Q for n = |c| + Q // 2 over |c| <= 1024, Q in 1..255, in uint32."""
    from yolov6.utils.jpeg import quant_recip, quantise_np
    c = np.arange(-1024, 1025, dtype=np.int64)[:, None]
    Q = np.arange(1, 256, dtype=np.int64)[None, :]
    n = np.abs(c) + Q // 2
    prod = n * quant_recip(Q)
    assert prod.max() < 2 ** 32
    assert np.array_equal(prod >> 20, n // Q)
    assert np.array_equal(np.sign(c) * (prod >> 20), quantise_np(c.astype(np.int32), Q.astype(np.int32)))


def test_colour_rule_is_within_one_level_of_the_jfif_matrix():
    """All 2^24 colours: Y per pixel, and Cb, Cr of a 2 x 2 block of one colour, against the float64 JFIF (full-range BT.601)
    matrix: at most one level apart."""
    from yolov6.utils.jpeg import jpeg_planes_np
    G, B = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    worst = [0.0, 0.0, 0.0]
    for R in range(256):
        frame = np.stack([B, G, np.full_like(G, R)], -1).astype(np.uint8)             # [256, 256, 3] BGR
        frame = np.repeat(np.repeat(frame, 2, 0), 2, 1)                               # every colour as a 2 x 2 block
        Y, Cb, Cr, _ = jpeg_planes_np(frame)
        fy = 0.299 * R + 0.587 * G + 0.114 * B
        fcb = np.clip(-0.168735892 * R - 0.331264108 * G + 0.5 * B + 128.0, 0, 255)
        fcr = np.clip(0.5 * R - 0.418687589 * G - 0.081312411 * B + 128.0, 0, 255)
        for k, (got, want) in enumerate(((Y[::2, ::2], fy), (Cb, fcb), (Cr, fcr))):
            worst[k] = max(worst[k], float(np.abs(got - want).max()))
    print('largest differences Y, Cb, Cr: %.4f %.4f %.4f' % tuple(worst))
    assert max(worst) <= 1.0


def test_chroma_takes_one_rounding_for_the_2x2_mean_after_padding():
    from yolov6.utils.jpeg import jpeg_planes_np
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    Y, Cb, Cr, (h, w) = jpeg_planes_np(img)
    assert (h, w) == (5, 7) and Y.shape == (16, 16) and Cb.shape == Cr.shape == (8, 8)
    pad = img[np.minimum(np.arange(16), 4)][:, np.minimum(np.arange(16), 6)].astype(np.int64)
    B, G, R = pad[..., 0], pad[..., 1], pad[..., 2]
    assert np.array_equal(Y, (19595 * R + 38470 * G + 7471 * B + 32768) >> 16)
    for got, (cr, cg, cb) in ((Cb, (-11059, -21709, 32768)), (Cr, (32768, -27439, -5329))):
        s = (cr * R + cg * G + cb * B).reshape(8, 2, 8, 2).sum(axis=(1, 3))
        assert np.array_equal(got, np.clip(((s + (1 << 17)) >> 18) + 128, 0, 255))


def test_nv12_bt601f_planes_feed_the_transform_as_they_are():
    from yolov6.utils.jpeg import encode_jpeg_np, jpeg_planes_np
    from yolov6.utils.nv12 import Nv12Frame, nv12_to_bgr_np
    rng = np.random.default_rng(4)
    buf = rng.integers(0, 256, (18 * 3 // 2, 22), dtype=np.uint8)
    f = Nv12Frame.from_packed(buf, 18, 22, 'bt601f')
    Y, Cb, Cr, _ = jpeg_planes_np(f)
    assert np.array_equal(Y[:18, :22], f.y) and np.array_equal(Cb[:9, :11], f.uv[..., 0]) and np.array_equal(Cr[:9, :11], f.uv[..., 1])
    assert (Y[18:, :22] == f.y[17]).all() and (Cb[:9, 11:] == f.uv[:, 10:11, 0]).all()
    g = Nv12Frame.from_packed(buf, 18, 22, 'bt709')
    assert encode_jpeg_np(g, 80, 4) == encode_jpeg_np(nv12_to_bgr_np(g), 80, 4)
    pil_check(encode_jpeg_np(g, 80, 4), nv12_to_bgr_np(g), 80)


# ---- the stream -----------------------------------------------------------------------------------
def test_header_parses_segment_by_segment():
    from yolov6.utils.jpeg import HUFF, HUFF_ORDER, ZIGZAG, encode_jpeg_np, jpeg_header, quant_tables
    head = jpeg_header(1234, 4321, 37, 500)
    segs, end = segments(head)
    assert end == len(head)
    assert [m for m, _ in segs] == [0xE0, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]           # no EXIF, no comment
    assert segs[0][1] == b'JFIF\x00' + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0])                          # 1.01, density 1:1, no thumbnail
    ql, qc = quant_tables(37)
    assert segs[1][1] == b'\x00' + bytes(ql[ZIGZAG].astype(np.uint8)) + b'\x01' + bytes(qc[ZIGZAG].astype(np.uint8))
    sof = segs[2][1]
    assert sof[0] == 8 and int.from_bytes(sof[1:3], 'big') == 1234 and int.from_bytes(sof[3:5], 'big') == 4321 and sof[5] == 3
    assert sof[6:] == bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    for (m, p), name in zip(segs[3:7], HUFF_ORDER):
        assert p == bytes([HUFF[name][0]]) + bytes(HUFF[name][1]) + bytes(HUFF[name][2])
    assert segs[7][1] == (500).to_bytes(2, 'big')
    assert segs[8][1] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    data = encode_jpeg_np(synthetic(20, 40), 37, 2)
    assert data.startswith(jpeg_header(20, 40, 37, 2)) and data.endswith(b'\xff\xd9')
    for bad in ((0, 5, 50, 1), (5, 65536, 50, 1), (5, 5, 0, 1), (5, 5, 101, 1), (5, 5, 50, 0), (5, 5, 50, 65536)):
        with pytest.raises(ValueError):
            jpeg_header(*bad)
    jpeg_header(65535, 65535, 1, 65535)


def test_markers_inside_the_entropy_data_are_only_rstm_in_order():
    from yolov6.utils.jpeg import encode_jpeg_np
    data = encode_jpeg_np(synthetic(48, 48), 100, 1)
    _, start = segments(data)
    body = data[start:-2]
    marks = [body[i + 1] for i in range(len(body) - 1) if body[i] == 0xFF and body[i + 1] != 0]
    assert marks == [0xD0 + (k & 7) for k in range(8)]                                            # 9 intervals: RST0..7 and RST0
    assert data[-2:] == b'\xff\xd9'


@pytest.mark.parametrize('name', [c[0] for c in constructed_set()] + ['synthetic', 'odd'])
def test_pil_decodes_every_stream_to_the_reconstruction(name):
    from yolov6.utils.jpeg import encode_jpeg_np
    cases = {c[0]: c[1:] for c in constructed_set()}
    cases['synthetic'] = (synthetic(), 75, 11)
    cases['odd'] = (synthetic(17, 15, seed=2), 90, 16)
    img, q, restart = cases[name]
    print('largest Y difference: %g' % pil_check(encode_jpeg_np(img, q, restart), img, q))


def test_pil_chroma_inside_regions_of_constant_chroma():
    """Four colour quadrants of 48 x 48 with luma texture: Cb and Cr as PIL upsamples them are within 1 of the reconstruction at
    the pixels at least 16 px inside a quadrant (libjpeg's upsampling is no plain replication, hence the restriction)."""
    from yolov6.utils.jpeg import encode_jpeg_np, jpeg_reconstruct_np
    img = np.zeros((96, 96, 3), np.uint8)
    for (i, j), c in zip(((0, 0), (0, 1), (1, 0), (1, 1)), ((200, 60, 40), (30, 180, 90), (90, 90, 220), (128, 128, 128))):
        img[48 * i:48 * i + 48, 48 * j:48 * j + 48] = c
    for q in (50, 90, 100):
        data = encode_jpeg_np(img, q, 16)
        pil_check(data, img, q)
        _, Cb, Cr = pil_planes(data)
        _, rb, rr = jpeg_reconstruct_np(img, q)
        inside = np.zeros((96, 96), bool)
        for i in (0, 48):
            for j in (0, 48):
                inside[i + 16:i + 32, j + 16:j + 32] = True
        for got, ref in ((Cb, rb), (Cr, rr)):
            up = np.repeat(np.repeat(ref, 2, 0), 2, 1)
            assert np.abs(got.astype(np.float64) - up)[inside].max() <= 1.0, q


def _psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b) ** 2))


@pytest.mark.parametrize('q', QUALITIES)
def test_size_and_psnr_against_pils_encoder(q):
    """The 160 x 176 synthetic image, one interval per MCU row: at most PIL's size at subsampling=2 plus 2 % plus 3 bytes per
    restart marker, and a Y PSNR of at least PIL's minus 0.3 dB.  Measured: +2.0 % / +1.4 % / +1.5 % including the 9 markers and
    the DRI segment PIL does not write (q 50 / 75 / 95)."""
    from yolov6.utils.jpeg import encode_jpeg_np
    img = synthetic()
    mine, pil = encode_jpeg_np(img, q, 11), _pil_jpeg(img, q)
    n_rst = 160 // 16 - 1
    print('quality %d: %d bytes, PIL %d (%+.2f %%)' % (q, len(mine), len(pil), 100.0 * (len(mine) - len(pil)) / len(pil)))
    assert len(mine) <= len(pil) * 1.02 + 3 * n_rst
    src = 0.299 * img[..., 2] + 0.587 * img[..., 1] + 0.114 * img[..., 0]
    a, b = _psnr(pil_planes(mine)[0], src), _psnr(pil_planes(pil)[0], src)
    print('quality %d: Y PSNR %.3f dB, PIL %.3f dB (%+.3f)' % (q, a, b, a - b))
    assert a >= b - 0.3


# ---- coverage and defects -------------------------------------------------------------------------
def test_constructed_set_covers_the_coder():
    from yolov6.utils.jpeg import encode_jpeg_np, new_stats
    st = new_stats()
    most_intervals = 0
    for name, img, q, restart in constructed_set():
        assert img.nbytes < 300000
        one = new_stats()
        encode_jpeg_np(img, q, restart, stats=one)
        most_intervals = max(most_intervals, one['intervals'])
        for k, v in one.items():
            st[k] = st[k] | v if isinstance(v, set) else st[k] + v
    print({k: sorted(v) if isinstance(v, set) else v for k, v in st.items()})
    assert st['dc_cat'] == set(range(12))
    assert st['ac_size'] == set(range(1, 11))
    assert st['zrl'] >= {1, 2, 3}
    assert st['no_eob'] >= 1 and st['zero_ac'] >= 1 and st['stuffed'] >= 1
    assert st['pad'] == set(range(8))
    assert most_intervals > 8


DEFECT_IMAGES = {'zrl_missing': 'basis', 'eob_missing': 'steps50'}


@pytest.mark.parametrize('defect', ['zigzag_swap', 'no_stuffing', 'zero_padding', 'predictor_kept', 'rst_not_wrapped', 'zrl_missing',
                                    'eob_missing', 'sign_plain'])
def test_wrong_emulations_are_caught(defect):
    """A coder with one wrong rule differs from the specification's bytes AND fails the PIL check.  'zero_padding' is the
    exception on the second count: a decoder discards the pad bits of an interval unread (libjpeg's process_restart), so no
    decoder can tell 0-bits from 1-bits there; only the byte comparison catches it, and the test says so by asserting that."""
    from yolov6.utils.jpeg import encode_jpeg_np
    cases = {c[0]: c[1:] for c in constructed_set()}
    img, q, restart = cases[DEFECT_IMAGES.get(defect, 'noise100')]
    good = encode_jpeg_np(img, q, restart)
    bad = encode_jpeg_np(img, q, restart, defect=defect)
    pil_check(good, img, q)
    assert bad != good
    if defect == 'zero_padding':
        assert len(bad) <= len(good) and pil_planes(bad)[0].shape == img.shape[:2]
        return
    with pytest.raises(Exception):
        pil_check(bad, img, q)


# ---- Inferer(save_jpeg=Q) on the CPU ----------------------------------------------------------------
def _files(root):
    import os
    return sorted(os.path.relpath(os.path.join(d, f), str(root)) for d, _, fs in os.walk(str(root)) for f in fs)


def compare_png_and_jpg_runs(png_dir, jpg_dir, quality, restart=16):
    """Two ``infer`` runs that differ in save_jpeg alone: every .png of the first is a .jpg of the same stem in the second holding
    ``encode_jpeg_np`` of the PNG's pixels (which PIL decodes to the reconstruction), shots.txt and stacks.txt name the .jpg
    files, every other file is the same.  Returns the folders that held pictures."""
    import os
    from yolov6.utils.jpeg import encode_jpeg_np
    a, b = _files(png_dir), _files(jpg_dir)
    assert not any(f.endswith('.jpg') for f in a) and not any(f.endswith('.png') for f in b)
    assert [f[:-4] + '.jpg' if f.endswith('.png') else f for f in a] == b
    kinds = set()
    for f in a:
        if f.endswith('.png'):
            bgr = np.ascontiguousarray(np.asarray(Image.open(str(png_dir / f)))[:, :, ::-1])
            data = (jpg_dir / (f[:-4] + '.jpg')).read_bytes()
            assert data == encode_jpeg_np(bgr, quality, restart), f
            pil_check(data, bgr, quality)
            kinds.add(f.split(os.sep)[-2])
        elif os.path.basename(f) in ('shots.txt', 'stacks.txt'):
            assert (png_dir / f).read_text().replace('.png', '.jpg') == (jpg_dir / f).read_text()
        else:
            assert (png_dir / f).read_bytes() == (jpg_dir / f).read_bytes(), f
    return kinds


def test_infer_save_jpeg_cpu(tmp_path, monkeypatch):
    """Every picture ``infer`` writes as PNG for --redact, --save-crops, --best-shots and --stack-shots is, with save_jpeg, a .jpg
    of the same stem holding ``encode_jpeg_np`` of the same pixels; shots.txt and stacks.txt name the .jpg files; nothing else
    changes; without the flag no .jpg exists."""
    import importlib
    import os
    import sys
    import torch
    from conftest import REPO
    import test_track_cpu as C
    from yolov6.utils.synth import build_synthetic
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    ckpt = tmp_path / 'tiny.pt'
    torch.save({'model': build_synthetic(os.path.join(REPO, 'configs', 'yololps.py'), width=0.0625, sigma=1.5).half(), 'ema': None,
                'epoch': 0}, str(ckpt))
    img_dir = tmp_path / 'imgs'
    img_dir.mkdir()
    for k, f in enumerate(C._moving_frames(6)):
        Image.fromarray(f).save(str(img_dir / ('f%02d.png' % k)))
    kw = dict(weights=str(ckpt), source=str(img_dir), yaml=None, img_size=[128, 160], conf_thres=0.06, iou_thres=0.45, max_det=20,
              device='cpu', not_save_img=True, save_txt=True, track=True, track_max_age=2, track_iou=0.25, track_expand=0.25,
              best_shots=True, crop_size=(16, 48), stack_shots=True, stack_search=1, stack_max_frames=4, stack_min_width=8.0,
              redact='fill', save_crops=True)
    plain = infer.run(save_dir=str(tmp_path / 'png'), **kw)
    jpg = infer.run(save_dir=str(tmp_path / 'jpg'), save_jpeg=85, **kw)
    assert all(torch.equal(a, b) for a, b in zip(plain, jpg))
    kinds = compare_png_and_jpg_runs(tmp_path / 'png', tmp_path / 'jpg', 85)
    assert kinds == {'redacted', 'crops', 'shots', 'stacks'}
    for bad in (0, 101, 2.5):
        with pytest.raises(ValueError):
            infer.run(save_dir=str(tmp_path / 'bad'), **dict(kw, save_jpeg=bad))
