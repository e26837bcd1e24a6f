"""Baseline JPEG: the format ``lp_jpeg_encode_batch`` (csrc/lp_jpeg.hip) writes, stated in numpy byte for byte, and the CPU path.

Stream: SOI, APP0 (JFIF 1.01, density 1:1), one DQT with both tables, SOF0 (8 bits, the true h x w, three components sampled
2x2 / 1x1 / 1x1), four DHT (DC luma, AC luma, DC chroma, AC chroma), DRI, SOS, the entropy-coded data, EOI.  No EXIF, no comment.
An MCU is 16 x 16 pixels: the Y blocks top-left, top-right, bottom-left, bottom-right, then Cb, then Cr.

Padding: pixel (i, j) of the padded image reads (min(i, h-1), min(j, w-1)); 1 <= h, w <= 65535.
Colour from a uint8 [h, w, 3] BGR frame (JFIF, full-range BT.601), int32 with arithmetic shifts:
    Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
    Cb = clamp255(((sum over the 2x2 of (-11059 R - 21709 G + 32768 B) + (1 << 17)) >> 18) + 128)
    Cr = clamp255(((sum over the 2x2 of ( 32768 R - 27439 G -  5329 B) + (1 << 17)) >> 18) + 128)
the 2x2 block taken after padding.  An ``Nv12Frame`` of matrix 'bt601f' is JFIF already: its Y plane and its U, V samples are
the three planes as they are (padded by the same rule); the other matrices go through ``nv12_to_bgr_np`` and the BGR rule.
Forward DCT of a block x (int32): M[k][n] = rint(4096 a(k) cos((2n+1) k pi / 16)), a(0) = sqrt(1/8), a(k) = 1/2;
    t = ((x - 128) @ M.T + 128) >> 8;   coef = (M @ t + 32768) >> 16           (largest intermediate 1.3e8)
Quantisation: sign(c) * ((|c| + Q // 2) // Q), Q of Annex K.1 / K.2 scaled by ``quality`` as libjpeg does (``quant_tables``);
the kernel divides by the reciprocal multiply ``quant_recip`` (equal over |c| <= 1151, Q in 1..255).  Zig-zag order.
Entropy coding: the typical Huffman tables of Annex K.3 (``HUFF``), never optimised; DC difference categories, run/size symbols,
ZRL (0xF0) per sixteen zeros, EOB (0x00) unless coefficient 63 is nonzero, negative values as v + (1 << s) - 1; bits MSB first;
0x00 after every 0xFF byte.  Restart intervals of ``restart`` MCUs along the linear MCU order (they may straddle MCU rows): each
byte aligned by 1-bits, DC predictors 0 at its start, RSTm (m modulo 8) between intervals.

``encode_jpeg_np`` packs the bits in a Python loop over the blocks: it is a specification, and takes seconds per megapixel.
"""
import numpy as np

from yolov6.utils.nv12 import Nv12Frame, nv12_to_bgr_np, _host

MAX_RESTART_DEVICE = 32      # LP_JPEG_MAX_RESTART: the kernel's limit (one workgroup's LDS); the specification takes 1..65535

#: Annex K.1 / K.2, natural (row-major) order
BASE_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], np.int32)
BASE_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
    + [99] * 32, np.int32)

#: ZIGZAG[z] = natural index of the z-th coded coefficient
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63],
    np.int64)


#: Annex K.3: name -> (table class << 4 | id, the 16 counts, the values)
HUFF = {
    'dc_luma': (0x00, (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
    'ac_luma': (0x10, (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d), (
        0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
        0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
        0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
        0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
        0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
        0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
        0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
        0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
        0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
        0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
        0xf9, 0xfa)),
    'dc_chroma': (0x01, (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),
    'ac_chroma': (0x11, (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), (
        0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
        0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
        0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
        0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
        0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
        0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
        0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
        0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
        0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
        0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
        0xf9, 0xfa)),
}
HUFF_ORDER = ('dc_luma', 'ac_luma', 'dc_chroma', 'ac_chroma')

_k, _n = np.arange(8)[:, None], np.arange(8)[None, :]
#: the forward DCT's integer matrix
DCT_M = np.rint(4096.0 * np.where(_k == 0, np.sqrt(1.0 / 8.0), 0.5) * np.cos((2 * _n + 1) * _k * np.pi / 16.0)).astype(np.int32)
#: the float64 orthonormal DCT matrix (tests, ``jpeg_reconstruct_np``)
DCT_F = np.where(_k == 0, np.sqrt(1.0 / 8.0), 0.5) * np.cos((2 * _n + 1) * _k * np.pi / 16.0)


def check_params(quality, restart, device=False):
    """(quality, restart) as ints, or a ValueError: quality 1..100, restart 1..65535 (``device``: 1..32)."""
    q, r = int(quality), int(restart)
    if q != quality or not 1 <= q <= 100:
        raise ValueError('quality must be an integer in 1..100, got %r' % (quality,))
    top = MAX_RESTART_DEVICE if device else 65535
    if r != restart or not 1 <= r <= top:
        raise ValueError('restart must be an integer in 1..%d, got %r' % (top, restart))
    return q, r


def quant_tables(quality):
    """(luma, chroma): int32 [64] in natural order, Annex K scaled as libjpeg's jpeg_set_quality does."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError('quality must be in 1..100, got %r' % (quality,))
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * s + 50) // 100, 1, 255).astype(np.int32) for base in (BASE_LUMA, BASE_CHROMA))


def quant_recip(Q):
    """The kernel's multiplier: (n * quant_recip(Q)) >> 20 == n // Q for 0 <= n <= 1151 + ..., Q in 1..255 (tests/test_jpeg_cpu.py)."""
    Q = np.asarray(Q, np.int64)
    return ((1 << 20) + Q - 1) // Q


def huff_codes(name):
    """{symbol: (code, length)} of one table of ``HUFF``: the canonical code of Annex C."""
    _, counts, values = HUFF[name]
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[values[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, 'big') + payload


def jpeg_header(h, w, quality, restart):
    """Everything before the entropy-coded data: SOI .. SOS."""
    h, w = int(h), int(w)
    if not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError('JPEG sizes are 1..65535, got %d x %d' % (h, w))
    quality, restart = check_params(quality, restart)
    ql, qc = quant_tables(quality)
    out = b'\xff\xd8'
    out += _seg(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    out += _seg(0xDB, b'\x00' + bytes(ql[ZIGZAG].astype(np.uint8)) + b'\x01' + bytes(qc[ZIGZAG].astype(np.uint8)))
    out += _seg(0xC0, b'\x08' + h.to_bytes(2, 'big') + w.to_bytes(2, 'big') + b'\x03' + b'\x01\x22\x00' + b'\x02\x11\x01' + b'\x03\x11\x01')
    for name in HUFF_ORDER:
        tc_th, counts, values = HUFF[name]
        out += _seg(0xC4, bytes([tc_th]) + bytes(counts) + bytes(values))
    out += _seg(0xDD, restart.to_bytes(2, 'big'))
    out += _seg(0xDA, b'\x03' + b'\x01\x00' + b'\x02\x11' + b'\x03\x11' + b'\x00\x3f\x00')
    return out


def _pad_index(n):
    """Indices 0..ceil16(n)-1 clamped to n-1."""
    return np.minimum(np.arange((n + 15) // 16 * 16), n - 1)


def jpeg_planes_np(frame):
    """(Y [H, W], Cb [H/2, W/2], Cr [H/2, W/2]) int32 of the padded image, H and W the multiples of 16 above h and w, and (h, w)."""
    if isinstance(frame, Nv12Frame):
        if frame.matrix == 'bt601f':
            y, uv = _host(frame.y).astype(np.int32), _host(frame.uv).astype(np.int32)
            h, w = frame.h, frame.w
            ii, jj = _pad_index(h), _pad_index(w)
            ci, cj = ii[::2] >> 1, jj[::2] >> 1
            return y[ii][:, jj], uv[ci][:, cj, 0], uv[ci][:, cj, 1], (h, w)
        frame = nv12_to_bgr_np(frame)
    frame = _host(frame)
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3 or frame.shape[0] < 1 or frame.shape[1] < 1:
        raise ValueError('frame must be a uint8 [h, w, 3] BGR array or an Nv12Frame, got %s %s' % (frame.dtype, frame.shape))
    h, w = frame.shape[:2]
    if h > 65535 or w > 65535:
        raise ValueError('JPEG sizes are 1..65535, got %d x %d' % (h, w))
    p = frame[_pad_index(h)][:, _pad_index(w)].astype(np.int32)
    B, G, R = p[..., 0], p[..., 1], p[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16

    def chroma(cr, cg, cb):
        v = cr * R + cg * G + cb * B
        s = v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2]
        return np.clip(((s + (1 << 17)) >> 18) + 128, 0, 255)
    return Y, chroma(-11059, -21709, 32768), chroma(32768, -27439, -5329), (h, w)


def fdct_np(x):
    """The integer forward DCT of int32 blocks [..., 8, 8] of samples 0..255."""
    t = ((np.asarray(x, np.int32) - 128) @ DCT_M.T + 128) >> 8
    return (DCT_M @ t + 32768) >> 16


def quantise_np(c, Q):
    c = np.asarray(c, np.int32)
    return np.sign(c) * ((np.abs(c) + Q // 2) // Q)


def _blocks(plane):
    """[H, W] -> [H/8, W/8, 8, 8]"""
    H, W = plane.shape
    return plane.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3)


def jpeg_coefficients_np(frame, quality=90):
    """int16 [n_mcu, 6, 64]: the quantised coefficients in zig-zag order, MCUs in raster order, blocks Y0 Y1 Y2 Y3 Cb Cr."""
    Y, Cb, Cr, _ = jpeg_planes_np(frame)
    ql, qc = quant_tables(quality)
    my, mx = Y.shape[0] // 16, Y.shape[1] // 16
    cy = quantise_np(fdct_np(_blocks(Y)), ql.reshape(8, 8))                  # [2my, 2mx, 8, 8]
    cy = cy.reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my * mx, 4, 64)
    cc = [quantise_np(fdct_np(_blocks(P)), qc.reshape(8, 8)).reshape(my * mx, 1, 64) for P in (Cb, Cr)]
    return np.concatenate([cy] + cc, axis=1)[:, :, ZIGZAG].astype(np.int16)


def new_stats():
    """The symbol statistics ``scan_np`` gathers (the tests' coverage condition)."""
    return {'dc_cat': set(), 'ac_size': set(), 'zrl': set(), 'no_eob': 0, 'zero_ac': 0, 'stuffed': 0, 'pad': set(), 'intervals': 0}


#: wrong rules ``scan_np`` can emulate, for the tests that show each is detected; never used by the product path
DEFECTS = ('zigzag_swap', 'no_stuffing', 'zero_padding', 'predictor_kept', 'rst_not_wrapped', 'zrl_missing', 'eob_missing',
           'sign_plain')


def scan_np(coef, restart, stats=None, defect=None):
    """The entropy-coded data and EOI of int16 [n_mcu, 6, 64] zig-zag coefficients: intervals, padding, stuffing, RSTm."""
    if defect is not None and defect not in DEFECTS:
        raise ValueError('unknown defect %r' % (defect,))
    dc_t = (huff_codes('dc_luma'), huff_codes('dc_chroma'))
    ac_t = (huff_codes('ac_luma'), huff_codes('ac_chroma'))
    neg = 0 if defect == 'sign_plain' else 1          # a negative value v of size s is coded as v + (1 << s) - 1
    coef = np.asarray(coef).astype(np.int64)
    if defect == 'zigzag_swap':
        coef = coef.copy()
        coef[:, :, [1, 2]] = coef[:, :, [2, 1]]
    n_mcu = coef.shape[0]
    n_int = (n_mcu + restart - 1) // restart
    out = bytearray()
    pred = [0, 0, 0]
    for it in range(n_int):
        if defect != 'predictor_kept':
            pred = [0, 0, 0]
        acc, nbits = 0, 0
        for m in range(it * restart, min((it + 1) * restart, n_mcu)):
            for b in range(6):
                comp = 0 if b < 4 else b - 3
                blk = coef[m, b]
                d = int(blk[0]) - pred[comp]
                pred[comp] = int(blk[0])
                s = abs(d).bit_length()
                code, length = dc_t[comp > 0][s]
                acc, nbits = (acc << length) | code, nbits + length
                if s:
                    acc, nbits = (acc << s) | (d if d > 0 else (d + (1 << s) - neg) & ((1 << s) - 1)), nbits + s
                if stats is not None:
                    stats['dc_cat'].add(s)
                nz = np.nonzero(blk[1:])[0] + 1
                last, most_zrl = 0, 0
                for z in nz:
                    run = int(z) - last - 1
                    v = int(blk[z])
                    n_zrl = run >> 4
                    most_zrl = max(most_zrl, n_zrl)
                    if defect != 'zrl_missing':
                        code, length = ac_t[comp > 0][0xF0]
                        for _ in range(n_zrl):
                            acc, nbits = (acc << length) | code, nbits + length
                    s = abs(v).bit_length()
                    code, length = ac_t[comp > 0][((run & 15) << 4) | s]
                    acc, nbits = (acc << length) | code, nbits + length
                    acc, nbits = (acc << s) | (v if v > 0 else (v + (1 << s) - neg) & ((1 << s) - 1)), nbits + s
                    last = int(z)
                    if stats is not None:
                        stats['ac_size'].add(s)
                if last != 63 and defect != 'eob_missing':
                    code, length = ac_t[comp > 0][0x00]
                    acc, nbits = (acc << length) | code, nbits + length
                if stats is not None:
                    if most_zrl:
                        stats['zrl'].add(most_zrl)
                    stats['no_eob'] += last == 63
                    stats['zero_ac'] += len(nz) == 0
        pad = -nbits % 8
        acc = (acc << pad) | (0 if defect == 'zero_padding' else (1 << pad) - 1)
        raw = acc.to_bytes((nbits + pad) // 8, 'big')
        data = raw if defect == 'no_stuffing' else raw.replace(b'\xff', b'\xff\x00')
        out += data
        if stats is not None:
            stats['pad'].add(pad)
            stats['stuffed'] += raw.count(b'\xff')
            stats['intervals'] += 1
        if it < n_int - 1:
            out += bytes([0xFF, 0xD0 + (it if defect == 'rst_not_wrapped' else it & 7)])
    return bytes(out) + b'\xff\xd9'


def encode_jpeg_np(frame, quality=90, restart=16, stats=None, defect=None):
    """The complete file of one frame (a uint8 [h, w, 3] BGR array or an ``Nv12Frame``): what ``runtime.encode_jpeg`` returns for
    it, byte for byte.  ``stats``: a ``new_stats()`` dict to add this image's symbol statistics to; ``defect``: tests only."""
    quality, restart = check_params(quality, restart)
    h, w = (frame.h, frame.w) if isinstance(frame, Nv12Frame) else _host(frame).shape[:2]
    coef = jpeg_coefficients_np(frame, quality)
    return jpeg_header(h, w, quality, restart) + scan_np(coef, restart, stats, defect)


def idct_np(c):
    """float64 orthonormal inverse DCT of [..., 8, 8]."""
    return DCT_F.T @ np.asarray(c, np.float64) @ DCT_F


def jpeg_reconstruct_np(frame, quality=90):
    """(Y [h, w], Cb, Cr [ceil(h/2), ceil(w/2)]) float64 planes a decoder reconstructs before chroma upsampling and colour:
    clip(rint(IDCT(coefficient * Q) + 128), 0, 255), cropped to the true size."""
    coef = jpeg_coefficients_np(frame, quality).astype(np.float64)
    h, w = (frame.h, frame.w) if isinstance(frame, Nv12Frame) else _host(frame).shape[:2]
    my, mx = (h + 15) // 16, (w + 15) // 16
    ql, qc = quant_tables(quality)
    nat = np.empty_like(coef)
    nat[:, :, ZIGZAG] = coef
    yb = idct_np((nat[:, :4] * ql).reshape(my, mx, 2, 2, 8, 8))
    Y = yb.transpose(0, 2, 4, 1, 3, 5).reshape(my * 16, mx * 16)
    planes = [Y]
    for b in (4, 5):
        cb = idct_np((nat[:, b] * qc).reshape(my, mx, 8, 8))
        planes.append(cb.transpose(0, 2, 1, 3).reshape(my * 8, mx * 8))
    planes = [np.clip(np.rint(p + 128.0), 0, 255) for p in planes]
    return planes[0][:h, :w], planes[1][:(h + 1) // 2, :(w + 1) // 2], planes[2][:(h + 1) // 2, :(w + 1) // 2]
