"""Plate redaction on the CPU: the numpy restatement of ``lp_redact_plates_batch`` (csrc/lp_redact.hip).

Every detection row of a frame makes the pixels of its plate unreadable, in place: by a mosaic whose cell grid is anchored to the
frame, or by a fill.  The quad of a row is the rule of the crops (``plate_crop.plate_quad``: the four corners if they form a
convex quad of area >= 1, else the box), scaled by ``1 + margin`` about its centre.  A pixel belongs to a row iff its centre lies
in the quad, edges included; a mosaic pixel takes the mean (rounded half up) of its cell OF THE FRAME AS IT WAS BEFORE THE CALL, so
the result does not depend on the order of the rows, overlapping plates agree, and redacting twice changes only what the first pass changed.

BGR frames are uint8 [h, w, 3] arrays; an ``Nv12Frame`` is redacted in its own planes: the same cells on Y, cells of
cell/2 x cell/2 samples on U and V, a chroma sample replaced iff any of its four luma pixels is.  The matrix plays no part, and the
result is NOT the BGR result of the converted frame (a mean does not commute with the clamped conversion).

The operations run in the kernel's order (fp64 geometry without fused multiply-adds, integer means), so this mirror and the
kernels agree bit for bit.  It is the CPU path of ``Inferer(..., redact=...)`` and the checker of the kernels.
"""
import numpy as np

from yolov6.utils.nv12 import Nv12Frame, bgr_to_nv12_np, is_nv12_list
from yolov6.utils.plate_crop import ST_EMPTY, plate_quad

MODES = ('mosaic', 'fill')
MAX_CELL = 64
MAX_MARGIN = 4.0
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


def redact_frame_np(frame, rows, mode='mosaic', cell=16, margin=0.1, fill=(0, 0, 0)):
    """One frame: (redacted copy, status int32 [len(rows)]).  ``frame``: uint8 [h, w, 3] BGR, or an ``Nv12Frame`` with host
    planes (the result is a new packed ``Nv12Frame``); ``rows`` [n, >= 12] fp32 in frame pixels; ``fill`` = (B, G, R)."""
    m, cell, margin = check_params(mode, cell, margin)
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
        else:
            out.y[mask] = fy
            out.uv[cmask] = (fu, fv)
        return out, status
    frame = np.asarray(frame)
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3 or frame.shape[0] < 1 or frame.shape[1] < 1:
        raise ValueError('frame must be a uint8 [h, w, 3] array, got %s %s' % (frame.dtype, frame.shape))
    out = frame.copy()
    status, mask = frame_mask(rows, frame.shape[0], frame.shape[1], margin)
    out[mask] = cell_means(out, cell)[mask] if m == 0 else fill_bytes(fill)
    return out, status


def redact_plates_np(frames, det, count, mode='mosaic', cell=16, margin=0.1, fill=(0, 0, 0)):
    """The specification of ``lp_redact_plates_batch``: ``frames`` a list of B uint8 [h, w, 3] BGR arrays or of B ``Nv12Frame``
    with host planes (one kind), ``det`` [>= B, max_det, 28] and ``count`` [>= B] as the padded detectors return them, in frame
    pixels.  Rows r < clamp(count[b], 0, max_det) of frame b are redacted; ``fill`` is (B, G, R), converted with the frame's
    matrix for NV12.  Returns (frames_out, status): new frames of the same kind (the inputs are not written) and int32
    [B, max_det] with 1 = corners, 2 = box, 3 = neither usable (nothing written), 0 = no such row."""
    check_params(mode, cell, margin)
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
        o, status[b, :n] = redact_frame_np(f, det[b, :n], mode, cell, margin, fill)
        out.append(o)
    return out, status
