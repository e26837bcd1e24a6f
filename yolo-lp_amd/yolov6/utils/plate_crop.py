"""Perspective-rectified plate crops on the CPU: the numpy restatement of ``lp_plate_crops_batch`` (csrc/lp_crops.hip).

Each detection row carries its plate's four corners in columns 4..11, in the label order TL, BL, BR, TR (reference
data/transCCPD.py:128, yolov6/utils/general.py:45-50).  A crop is the upright ``crop_hw`` image of the plate: the
projective map of the unit square onto the quad (Heckbert's square-to-quad form, fp64), sampled at pixel centres, with a
bilinear fp32 blend of the frame, the frame's edge replicated.  That is ``F.grid_sample(mode='bilinear',
padding_mode='border', align_corners=False)`` at the mapped points, without an anti-aliasing prefilter.

The operations run in the kernel's order (fp64 geometry, float32 blend, no fused multiply-adds), so this mirror and the
kernel agree bit for bit.  It is the CPU path of ``Inferer(..., save_crops=True)`` and the checker of the kernel.
"""
import math

import numpy as np

ST_NONE, ST_CORNERS, ST_BOX, ST_EMPTY = 0, 1, 2, 3   # status codes: not cropped, corners, box, neither usable (zeros)


def plate_quad(row):
    """(status, xs, ys) of one detection row: the quad p0 = TL, p1 = TR, p2 = BR, p3 = BL as two 4-lists of floats, from
    the corners (status 1) if they are finite, strictly convex in label orientation and of area >= 1 px^2, else from the
    box (status 2) if it is finite and at least 1 px on each side; (3, None, None) if neither."""
    c = [float(np.float32(v)) for v in row[:12]]
    x = [c[4], c[10], c[8], c[6]]
    y = [c[5], c[11], c[9], c[7]]
    if all(math.isfinite(v) for v in x + y):
        convex = True
        order = (0, 3, 2, 1)                      # TL -> BL -> BR -> TR: clockwise on screen, every cross product < 0
        for k in range(4):
            i0, i1, i2 = order[k], order[(k + 1) % 4], order[(k + 2) % 4]
            ex, ey = x[i1] - x[i0], y[i1] - y[i0]
            fx, fy = x[i2] - x[i1], y[i2] - y[i1]
            if not (ex * fy - ey * fx < 0.0):
                convex = False
        area = 0.5 * abs((x[2] - x[0]) * (y[3] - y[1]) - (x[3] - x[1]) * (y[2] - y[0]))
        if convex and area >= 1.0:
            return ST_CORNERS, x, y
    x1, y1, x2, y2 = c[0], c[1], c[2], c[3]
    if all(math.isfinite(v) for v in (x1, y1, x2, y2)) and x2 - x1 >= 1.0 and y2 - y1 >= 1.0:
        return ST_BOX, [x1, x2, x2, x1], [y1, y1, y2, y2]
    return ST_EMPTY, None, None


def square_to_quad(x, y):
    """(a, b, c, d, e, f, g, h) of the projective map (u, v) -> ((a u + b v + c) / w, (d u + e v + f) / w), w = g u + h v + 1,
    that sends (0,0), (1,0), (1,1), (0,1) to (x[k], y[k]), k = 0..3 (Heckbert)."""
    sx, sy = x[0] - x[1] + x[2] - x[3], y[0] - y[1] + y[2] - y[3]
    dx1, dx2, dy1, dy2 = x[1] - x[2], x[3] - x[2], y[1] - y[2], y[3] - y[2]
    den = dx1 * dy2 - dx2 * dy1
    g = (sx * dy2 - dx2 * sy) / den
    h = (dx1 * sy - sx * dy1) / den
    return (x[1] - x[0] + g * x[1], x[3] - x[0] + h * x[3], x[0],
            y[1] - y[0] + g * y[1], y[3] - y[0] + h * y[3], y[0], g, h)


def _axis(p, n):
    """clamp(p - 0.5, 0, n - 1) (NaN -> 0) -> first tap, second tap, float32 fraction."""
    s = p - 0.5
    s = np.where(s >= 0.0, s, 0.0)
    s = np.where(s < float(n - 1), s, float(n - 1))
    fl = np.floor(s)
    t0 = fl.astype(np.int64)
    return t0, np.minimum(t0 + 1, n - 1), (s - fl).astype(np.float32)


def sample_quad(frame_bgr, x, y, crop_hw):
    """uint8 [Hc, Wc, C] crop of ``frame_bgr`` [h, w, C] along the quad (x, y) (p0 = TL, p1 = TR, p2 = BR, p3 = BL)."""
    Hc, Wc = crop_hw
    h0, w0 = frame_bgr.shape[:2]
    a, b, c, d, e, f, g, h = square_to_quad(x, y)
    u = ((np.arange(Wc, dtype=np.float64) + 0.5) / float(Wc))[None, :]
    v = ((np.arange(Hc, dtype=np.float64) + 0.5) / float(Hc))[:, None]
    w = g * u + h * v + 1.0
    X = (a * u + b * v + c) / w
    Y = (d * u + e * v + f) / w
    x0, x1, fx = _axis(X, w0)
    y0, y1, fy = _axis(Y, h0)
    p00, p01 = frame_bgr[y0, x0].astype(np.float32), frame_bgr[y0, x1].astype(np.float32)
    p10, p11 = frame_bgr[y1, x0].astype(np.float32), frame_bgr[y1, x1].astype(np.float32)
    fx, fy = fx[..., None], fy[..., None]
    one = np.float32(1.0)
    gx, gy = one - fx, one - fy
    val = gy * (gx * p00 + fx * p01) + fy * (gx * p10 + fx * p11)
    return np.clip(np.rint(val), 0, 255).astype(np.uint8)


def plate_crops_np(frame_bgr, rows, crop_hw=(64, 192)):
    """Crops of every detection row of one frame: ``frame_bgr`` uint8 [h, w, 3], ``rows`` [n, >= 12] in source-frame pixels
    (fp32 values) -> (crops uint8 [n, Hc, Wc, 3] in the frame's channel order, status int32 [n] in {1, 2, 3})."""
    frame_bgr = np.ascontiguousarray(frame_bgr)
    if frame_bgr.dtype != np.uint8 or frame_bgr.ndim != 3 or frame_bgr.shape[0] < 1 or frame_bgr.shape[1] < 1:
        raise ValueError('frame must be a uint8 [h, w, C] array, got %s %s' % (frame_bgr.dtype, frame_bgr.shape))
    Hc, Wc = int(crop_hw[0]), int(crop_hw[1])
    if not (1 <= Hc <= 1024 and 1 <= Wc <= 1024):
        raise ValueError('crop size %dx%d: need 1..1024 on each side' % (Hc, Wc))
    rows = np.asarray(rows, dtype=np.float32)
    if rows.size == 0:
        rows = rows.reshape(0, 12)
    if rows.ndim != 2 or rows.shape[1] < 12:
        raise ValueError('rows must be [n, >= 12], got %s' % (rows.shape,))
    crops = np.zeros((len(rows), Hc, Wc, frame_bgr.shape[2]), dtype=np.uint8)
    status = np.zeros(len(rows), dtype=np.int32)
    for k, row in enumerate(rows):
        st, x, y = plate_quad(row)
        status[k] = st
        if st != ST_EMPTY:
            crops[k] = sample_quad(frame_bgr, x, y, (Hc, Wc))
    return crops, status
