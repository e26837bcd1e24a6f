"""Plate redaction on the CPU: the numpy restatement of ``lp_redact_plates_batch`` (csrc/lp_redact.hip).

Every detection row of a frame makes the pixels of its plate unreadable, in place: by a mosaic whose cell grid is anchored to the
frame, or by a fill.  The quad of a row is the rule of the crops (``plate_crop.plate_quad``: the four corners if they form a
convex quad of area >= 1, else the box), scaled by ``1 + margin`` about its centre.  A pixel belongs to a row iff its centre lies
in the quad, edges included; a mosaic pixel takes the mean (rounded half up) of its cell OF THE FRAME AS IT WAS BEFORE THE CALL, so
the result does not depend on the order of the rows, overlapping plates agree, and redacting twice changes only what the first pass changed.
A gauss pixel takes G(frame) at that pixel: the frame AS IT WAS BEFORE THE CALL under the integer separable Gaussian of
``gauss_blur_np`` (taps ``gauss_taps(sigma)``, replicate border).  G depends on the frame alone, so the order of the rows does not
matter and overlapping plates agree here too; but a second call is NOT idempotent inside the mask: it blurs the blurred pixels again.

BGR frames are uint8 [h, w, 3] arrays; an ``Nv12Frame`` is redacted in its own planes: the same cells on Y, cells of
cell/2 x cell/2 samples on U and V, a chroma sample replaced iff any of its four luma pixels is.  Gauss blurs Y with
``gauss_taps(sigma)`` and U, V with ``gauss_taps(sigma / 2)`` on the half-resolution chroma plane, in chroma coordinates (the border
clamp too).  The matrix plays no part, and the result is NOT the BGR result of the converted frame (neither a mean nor a blur
commutes with the clamped conversion).

The operations run in the kernel's order (fp64 geometry without fused multiply-adds, integer means, integer blur), so this
mirror and the kernels agree bit for bit.  It is the CPU path of ``Inferer(..., redact=...)`` and the checker of the kernels.
"""
import math

import numpy as np

from yolov6.utils.nv12 import Nv12Frame, bgr_to_nv12_np, is_nv12_list
from yolov6.utils.plate_crop import ST_EMPTY, plate_quad

MODES = ('mosaic', 'fill', 'gauss')
MAX_CELL = 64
MAX_MARGIN = 4.0
MAX_RADIUS = 48                # LP_REDACT_MAX_RADIUS: ceil(3 * MAX_SIGMA)
MIN_SIGMA, MAX_SIGMA = 0.5, 16.0
DEFAULT_SIGMA = 8.0
TAP_ONE = 16384                # the taps of a blur sum to 2^14
EDGE_ORDER = (0, 3, 2, 1)      # p0 -> p3 -> p2 -> p1 (-> p0): the label orientation TL -> BL -> BR -> TR


def check_params(mode, cell, margin):
    """(mode index, cell, margin) of the arguments every redaction entry point shares, or a ValueError."""
    if mode not in MODES:
        raise ValueError('redact mode %r: one of %s' % (mode, ', '.join(MODES)))
    cell, margin = int(cell), float(margin)
    if mode == 'mosaic' and (cell < 2 or cell > MAX_CELL or cell % 2):
        raise ValueError('mosaic cell %d: need an even side in 2..%d' % (cell, MAX_CELL))
    if not 0.0 <= margin <= MAX_MARGIN:
        raise ValueError('margin %r: need 0 <= margin <= %g' % (margin, MAX_MARGIN))
    return MODES.index(mode), cell, margin


def check_sigma(sigma):
    """The sigma of a gauss redaction as a float (None: 8.0), or a ValueError outside [0.5, 16] (a NaN included)."""
    sigma = DEFAULT_SIGMA if sigma is None else float(sigma)
    if not MIN_SIGMA <= sigma <= MAX_SIGMA:
        raise ValueError('sigma %r: need %g <= sigma <= %g' % (sigma, MIN_SIGMA, MAX_SIGMA))
    return sigma


def gauss_taps(sigma):
    """int32 [R + 1]: the taps q[0..R] of the integer Gaussian of ``sigma`` in [0.25, 16] (the chroma planes take half the
    public sigma), R = ceil(3 sigma) <= 48.  From g[k] = exp(-k^2 / (2 sigma^2)) and S = g[0] + 2 sum g[1..R] in float64:
    q[k] = floor(16384 g[k] / S + 0.5) for k >= 1 and q[0] = 16384 - 2 sum q[1..R], so q[0] + 2 sum q[1..R] is 16384 exactly.
    The taps are data: no device evaluates an exponential."""
    sigma = float(sigma)
    if not MIN_SIGMA / 2 <= sigma <= MAX_SIGMA:
        raise ValueError('sigma %r: gauss_taps needs %g <= sigma <= %g' % (sigma, MIN_SIGMA / 2, MAX_SIGMA))
    R = int(math.ceil(3.0 * sigma))
    g = [math.exp(-(k * k) / (2.0 * sigma * sigma)) for k in range(R + 1)]
    S = g[0] + 2.0 * sum(g[1:])
    q = [0] + [int(math.floor(TAP_ONE * g[k] / S + 0.5)) for k in range(1, R + 1)]
    q[0] = TAP_ONE - 2 * sum(q[1:])
    return np.asarray(q, np.int32)


def gauss_blur_np(plane, taps):
    """uint8 array of ``plane``'s shape ([h, w] or [h, w, C]; the channels are blurred separately): the separable integer blur
    with the taps q[0..R], indices clamped to the plane (replicate border).  Horizontal:
    hq = (sum_k q[|k|] p[i, clamp(j + k)] + 32) >> 6 (at most 65280: 16 bits); vertical:
    out = (sum_k q[|k|] hq[clamp(i + k), j] + 2^21) >> 22 (the sum stays below 2^31).  A constant plane comes out unchanged."""
    plane = np.asarray(plane)
    q = [int(t) for t in np.asarray(taps).reshape(-1)]
    R = len(q) - 1
    if plane.dtype != np.uint8 or plane.ndim not in (2, 3) or R < 1 or q[0] + 2 * sum(q[1:]) != TAP_ONE or min(q) < 0:
        raise ValueError('gauss_blur_np needs a uint8 [h, w] or [h, w, C] plane and taps q[0..R >= 1] >= 0 with q[0] + 2 sum q[1..R] = %d'
                         % TAP_ONE)
    h, w = plane.shape[:2]
    ii = np.clip(np.arange(-R, h + R), 0, h - 1)
    jj = np.clip(np.arange(-R, w + R), 0, w - 1)
    p = plane.astype(np.int64)[:, jj]                                   # [h, w + 2R, ...]
    acc = q[0] * p[:, R:R + w]
    for k in range(1, R + 1):
        acc += q[k] * (p[:, R - k:R - k + w] + p[:, R + k:R + k + w])
    hq = ((acc + 32) >> 6)[ii]                                          # [h + 2R, w, ...]
    acc = q[0] * hq[R:R + h]
    for k in range(1, R + 1):
        acc += q[k] * (hq[R - k:R - k + h] + hq[R + k:R + k + h])
    return ((acc + (1 << 21)) >> 22).astype(np.uint8)


def fill_bytes(fill, matrix=None):
    """The three bytes a fill writes, from ``fill`` = (B, G, R): the same for a BGR frame; for an NV12 frame of ``matrix`` the
    (Y, U, V) that ``bgr_to_nv12_np`` gives a 2 x 2 image of that colour."""
    fill = tuple(int(v) for v in fill)
    if len(fill) != 3 or not all(0 <= v <= 255 for v in fill):
        raise ValueError('fill must be three bytes (B, G, R), got %r' % (fill,))
    if matrix is None:
        return fill
    f = bgr_to_nv12_np(np.full((2, 2, 3), fill, np.uint8), matrix)
    return int(f.y[0, 0]), int(f.uv[0, 0, 0]), int(f.uv[0, 0, 1])


def expanded_quad(x, y, margin):
    """The quad (x, y) (two 4-lists) scaled by 1 + margin about the mean of its corners, fp64 in the kernel's order."""
    cx = 0.25 * (((x[0] + x[1]) + x[2]) + x[3])
    cy = 0.25 * (((y[0] + y[1]) + y[2]) + y[3])
    s = 1.0 + margin
    return [cx + s * (v - cx) for v in x], [cy + s * (v - cy) for v in y]


def _clamp_to(v, n):
    """clamp(v, 0, n) in double, then to int."""
    v = v if v >= 0.0 else 0.0
    v = v if v < float(n) else float(n)
    return int(v)


def scan_rect(x, y, h, w):
    """(i0, i1, j0, j1): the rows [i0, i1) and columns [j0, j1) the scan of the quad (x, y) is bounded by in an h x w frame."""
    return (_clamp_to(float(np.floor(min(y))), h), _clamp_to(float(np.ceil(max(y))), h),
            _clamp_to(float(np.floor(min(x))), w), _clamp_to(float(np.ceil(max(x))), w))


def row_mask(row, h, w, margin):
    """(status, mask) of one detection row in an h x w frame: ``mask`` bool [h, w], True where the pixel belongs to the row
    (all False for status 3)."""
    mask = np.zeros((h, w), bool)
    st, x, y = plate_quad(row)
    if st == ST_EMPTY:
        return st, mask
    x, y = expanded_quad(x, y, margin)
    i0, i1, j0, j1 = scan_rect(x, y, h, w)
    if i0 >= i1 or j0 >= j1:
        return st, mask
    py = (np.arange(i0, i1, dtype=np.float64) + 0.5)[:, None]
    px = (np.arange(j0, j1, dtype=np.float64) + 0.5)[None, :]
    inside = np.ones((i1 - i0, j1 - j0), bool)
    for k in range(4):
        a, b = EDGE_ORDER[k], EDGE_ORDER[(k + 1) % 4]
        ex, ey = x[b] - x[a], y[b] - y[a]
        inside &= ex * (py - y[a]) - ey * (px - x[a]) <= 0.0
    mask[i0:i1, j0:j1] = inside
    return st, mask


def frame_mask(rows, h, w, margin):
    """(status int32 [len(rows)], mask bool [h, w]): the union of the rows' masks."""
    status = np.zeros(len(rows), np.int32)
    mask = np.zeros((h, w), bool)
    for k, row in enumerate(rows):
        status[k], m = row_mask(row, h, w, margin)
        mask |= m
    return status, mask


def cell_means(plane, cell):
    """uint8 array of ``plane``'s shape ([h, w] or [h, w, C]): every sample replaced by (2 * sum + n) // (2 * n) over the n
    samples of its cell, the cells ``cell`` on a side, anchored at (0, 0) and clipped at the plane's edges."""
    h, w = plane.shape[:2]
    ys, xs = np.arange(0, h, cell), np.arange(0, w, cell)
    sums = np.add.reduceat(np.add.reduceat(plane.astype(np.int64), ys, axis=0), xs, axis=1)
    n = np.outer(np.minimum(ys + cell, h) - ys, np.minimum(xs + cell, w) - xs).astype(np.int64)
    n = n.reshape(n.shape + (1,) * (plane.ndim - 2))
    val = ((2 * sums + n) // (2 * n)).astype(np.uint8)
    return np.repeat(np.repeat(val, cell, axis=0), cell, axis=1)[:h, :w]


def redact_frame_np(frame, rows, mode='mosaic', cell=16, margin=0.1, fill=(0, 0, 0), sigma=None):
    """One frame: (redacted copy, status int32 [len(rows)]).  ``frame``: uint8 [h, w, 3] BGR, or an ``Nv12Frame`` with host
    planes (the result is a new packed ``Nv12Frame``); ``rows`` [n, >= 12] fp32 in frame pixels; ``fill`` = (B, G, R);
    ``sigma``: of the gauss mode (None: 8.0), ignored by the others as ``cell`` is by fill."""
    m, cell, margin = check_params(mode, cell, margin)
    if m == 2:
        sigma = check_sigma(sigma)
    rows = np.asarray(rows, np.float32)
    if rows.size == 0:
        rows = rows.reshape(0, 12)
    if isinstance(frame, Nv12Frame):
        out = Nv12Frame.from_packed(frame.packed(), frame.h, frame.w, frame.matrix)
        status, mask = frame_mask(rows, frame.h, frame.w, margin)
        cmask = mask.reshape(frame.h // 2, 2, frame.w // 2, 2).any(axis=(1, 3))       # any of the sample's four luma pixels
        fy, fu, fv = fill_bytes(fill, frame.matrix)
        if m == 0:
            out.y[mask] = cell_means(out.y, cell)[mask]
            out.uv[cmask] = cell_means(out.uv, cell // 2)[cmask]
        elif m == 2:
            if mask.any():
                out.y[mask] = gauss_blur_np(out.y, gauss_taps(sigma))[mask]
                out.uv[cmask] = gauss_blur_np(out.uv, gauss_taps(sigma / 2))[cmask]
        else:
            out.y[mask] = fy
            out.uv[cmask] = (fu, fv)
        return out, status
    frame = np.asarray(frame)
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3 or frame.shape[0] < 1 or frame.shape[1] < 1:
        raise ValueError('frame must be a uint8 [h, w, 3] array, got %s %s' % (frame.dtype, frame.shape))
    out = frame.copy()
    status, mask = frame_mask(rows, frame.shape[0], frame.shape[1], margin)
    if m == 2:
        if mask.any():
            out[mask] = gauss_blur_np(out, gauss_taps(sigma))[mask]
    else:
        out[mask] = cell_means(out, cell)[mask] if m == 0 else fill_bytes(fill)
    return out, status


def redact_plates_np(frames, det, count, mode='mosaic', cell=16, margin=0.1, fill=(0, 0, 0), sigma=None):
    """The specification of ``lp_redact_plates_batch`` and, for ``mode`` 'gauss' (``sigma`` in [0.5, 16], None: 8.0), of
    ``lp_redact_gauss_batch``: ``frames`` a list of B uint8 [h, w, 3] BGR arrays or of B ``Nv12Frame``
    with host planes (one kind), ``det`` [>= B, max_det, 28] and ``count`` [>= B] as the padded detectors return them, in frame
    pixels.  Rows r < clamp(count[b], 0, max_det) of frame b are redacted; ``fill`` is (B, G, R), converted with the frame's
    matrix for NV12.  Returns (frames_out, status): new frames of the same kind (the inputs are not written) and int32
    [B, max_det] with 1 = corners, 2 = box, 3 = neither usable (nothing written), 0 = no such row."""
    if check_params(mode, cell, margin)[0] == 2:
        sigma = check_sigma(sigma)
    frames = list(frames)
    is_nv12_list(frames)
    det = np.asarray(det, np.float32)
    count = np.asarray(count).reshape(-1)
    if det.ndim != 3 or det.shape[2] < 12 or det.shape[0] < len(frames) or count.shape[0] < len(frames) or det.shape[1] < 1:
        raise ValueError('det must be [>= %d, max_det >= 1, >= 12] with a count per frame, got %s and %s'
                         % (len(frames), det.shape, count.shape))
    max_det = det.shape[1]
    status = np.zeros((len(frames), max_det), np.int32)
    out = []
    for b, f in enumerate(frames):
        n = max(0, min(int(count[b]), max_det))
        o, status[b, :n] = redact_frame_np(f, det[b, :n], mode, cell, margin, fill, sigma)
        out.append(o)
    return out, status
